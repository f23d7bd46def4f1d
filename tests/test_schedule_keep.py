"""Region editing in the host-side schedule bookkeeping (text2human_amd/schedule.py): rows kept from a source state take
part in no round, fully kept samples leave the batch first, the generator offsets follow the reference's loop started
from `unmasked = keep`, and compact / synchronous / shrinking rounds end in that loop's tokens.  CPU, numpy only."""
import numpy as np
import pytest

from text2human_amd import schedule

from schedule_util import check_plan  # noqa: E402

MASK_ID = 18432


def _schedule_with_keep(B, T, steps, density, seed, full_kept=()):
    """(step int64 [B*T] -- 0 on kept rows --, kept bool [B*T]) as the reference's loop assigns them from
    unmasked = keep"""
    rng = np.random.default_rng(seed)
    kept = rng.random(B * T) < density
    for b in full_kept:
        kept[b * T:(b + 1) * T] = True
    step = np.zeros(B * T, dtype=np.int64)
    unmasked = kept.copy()
    for t in range(steps, 0, -1):
        hit = (rng.random(B * T) < np.float32(1.0) / np.float32(t)) & ~unmasked
        unmasked |= hit
        step[hit] = t
    assert unmasked.all()
    return step, kept


@pytest.mark.parametrize('compact', [True, False])
@pytest.mark.parametrize('B,T,steps,density', [(8, 512, 256, 0.75), (3, 64, 20, 0.5), (2, 32, 5, 0.0)])
def test_every_resampled_row_is_in_exactly_one_round_and_kept_rows_in_none(B, T, steps, density, compact):
    step, kept = _schedule_with_keep(B, T, steps, density, seed=B * 31 + steps, full_kept=(1, ))
    order, start, round_steps = schedule.group_rounds(step, B, T, compact=compact, kept=kept)
    assert sorted(order.tolist()) == np.nonzero(~kept)[0].tolist()
    assert start[0] == 0 and start[-1] == (~kept).sum() and round_steps.shape == (len(start) - 1, B)
    for r in range(len(start) - 1):
        rows = order[start[r]:start[r + 1]]
        assert len(rows) > 0 and (step[rows] == round_steps[r, rows // T]).all()
    assert (round_steps[:, 1] == 0).all()                     # the fully kept sample never runs
    st = schedule.stats(round_steps, steps, kept=kept)
    assert st['rows_kept'] == kept.sum()
    if compact:
        assert st['rounds'] == max(len(np.unique(step[b * T:(b + 1) * T][~kept[b * T:(b + 1) * T]])) for b in range(B))


def test_step_zero_needs_an_explicit_kept_mark():
    step = np.array([1, 0, 2, 1])
    with pytest.raises(ValueError):
        schedule.group_rounds(step, 1, 4)
    with pytest.raises(ValueError):
        schedule.group_rounds(step, 1, 4, kept=np.array([0, 0, 1, 0], dtype=bool))     # row 1 unmarked, row 2 has a step
    order, start, _ = schedule.group_rounds(step, 1, 4, kept=np.array([0, 1, 0, 0], dtype=bool))
    assert sorted(order.tolist()) == [0, 2, 3] and start[-1] == 3


def test_all_kept_means_no_rounds():
    B, T = 3, 16
    step, kept = np.zeros(B * T, dtype=np.int64), np.ones(B * T, dtype=bool)
    order, start, round_steps = schedule.group_rounds(step, B, T, kept=kept)
    assert len(order) == 0 and start.tolist() == [0] and round_steps.shape == (0, B)
    perm, n_act = schedule.leave_order(step, B, T, kept)
    assert perm.tolist() == [0, 1, 2] and (n_act == 0).all()
    assert schedule.stats(round_steps, 7, np.zeros(0, dtype=np.int64), kept)['sample_steps_launched'] == 0


def test_leave_order_keeps_the_running_samples_a_prefix_with_fully_kept_samples():
    B, T, steps = 6, 64, 40
    step, kept = _schedule_with_keep(B, T, steps, 0.6, seed=5, full_kept=(0, 3))
    perm, n_act = schedule.leave_order(step, B, T, kept)
    assert sorted(perm.tolist()) == list(range(B)) and (np.diff(n_act) <= 0).all()
    assert set(perm[-2:].tolist()) == {0, 3} and (n_act[-2:] == 0).all()       # fully kept: last
    orig_row = (perm[:, None] * T + np.arange(T)[None, :]).reshape(-1)
    order, start, round_steps = schedule.group_rounds(step[orig_row], B, T, compact=True, kept=kept[orig_row])
    active = (round_steps > 0).sum(1)
    assert active[0] == B - 2 and (np.diff(active) <= 0).all()
    for r in range(len(active)):
        assert (round_steps[r, :active[r]] > 0).all() and (round_steps[r, active[r]:] == 0).all()
        assert (order[start[r]:start[r + 1]] // T < active[r]).all()


def test_draw_offsets_match_the_loop_started_from_keep():
    """schedule.draw_offsets on the head mask of a loop with unmasked = keep: the generator offsets of every draw, as a
    restated loop that walks the generator draw by draw"""
    B, T, steps, H = 2, 64, 12, 18
    rand_inc, expo_inc, off0 = 4, 4 * 512, 40
    step, kept = _schedule_with_keep(B, T, steps, 0.7, seed=9)
    tex = np.random.default_rng(10).integers(0, H, B * T)
    head_mask = np.zeros(steps + 1, dtype=np.int64)
    for t in range(1, steps + 1):
        for h in np.unique(tex[step == t]):
            head_mask[t] |= 1 << int(h)
    rand_off, expo_off, final = schedule.draw_offsets(head_mask, steps, off0, rand_inc, expo_inc, H)
    cur, n_expo = off0, 0
    for t in range(steps, 0, -1):
        assert rand_off[t] == cur
        cur += rand_inc
        changed = (step == t) & ~kept                       # kept rows are never "changed"
        for h in range(H):
            if ((tex == h) & changed).any():
                assert expo_off[t, h] == cur
                cur += expo_inc
                n_expo += 1
            else:
                assert expo_off[t, h] == -1
    assert final == cur
    assert final - off0 - steps * rand_inc == n_expo * expo_inc
    # all kept: only the rand draws move the generator
    assert schedule.draw_offsets(np.zeros(steps + 1), steps, off0, rand_inc, expo_inc, H)[2] == off0 + steps * rand_inc


def _toy_token(state_b, draw_row, step, head):
    """(as tests/test_schedule.py) a stand-in for transformer + categorical draw that depends on the sample's whole
    current state and on the identity of the noise element"""
    h = (int(state_b.sum()) * 1000003 + int((state_b * (np.arange(len(state_b)) + 1)).sum())) & 0x7FFFFFFF
    return (h ^ (draw_row * 2654435761) ^ (step * 40503) ^ (head * 97)) % 1024


def _initial_state(src, tex, kept, B, T):
    x = np.where(kept, src + 1024 * tex, MASK_ID).reshape(B, T)
    return x


def _reference_loop(step, tex, src, kept, B, T, steps):
    """the reference's loop from the edit's initial state (the restatement the GPU tests use, on the toy model)"""
    x = _initial_state(src, tex, kept, B, T)
    for t in range(steps, 0, -1):
        rows = np.nonzero((step == t) & ~kept)[0]
        new = [(r, _toy_token(x[r // T], r, t, int(tex[r]))) for r in rows]
        for r, v in new:
            x[r // T, r % T] = v + 1024 * int(tex[r])
    return x


def _rounds_loop(step, tex, src, kept, B, T, compact, shrink):
    """The rounds engine.sample_tokens runs with init (schedule.plan_rounds), walked with the toy model from the
    prefilled state"""
    plan = schedule.plan_rounds(step, tex, B, T, compact, shrink, kept)
    draw_rows = plan.rng_rows if plan.rng_rows is not None else plan.order   # the row of the reference's draw
    x = _initial_state(src, tex, kept, B, T)
    if plan.perm is not None:
        x = x[plan.perm]                                     # the prefill, in the schedule's sample order
    for r in range(len(plan.start) - 1):
        lo, hi = int(plan.start[r]), int(plan.start[r + 1])
        k = int(plan.active[r]) if shrink else B
        before = x.copy()
        for i in range(lo, hi):
            row, orig = int(plan.order[i]), int(draw_rows[i])
            assert row // T < k and not plan.kept[row]
            x[row // T, row % T] = _toy_token(before[row // T], orig, int(plan.round_steps[r, row // T]),
                                              int(tex[orig])) + 1024 * int(tex[orig])
    return x.reshape(-1)[schedule.in_caller_order(plan.perm, B, T)].reshape(B, T)


@pytest.mark.parametrize('B,T,steps,density,seed', [(4, 32, 16, 0.5, 0), (7, 16, 40, 0.25, 1), (3, 64, 256, 0.75, 2),
                                                    (5, 8, 6, 0.9, 3)])
def test_rounds_from_a_kept_state_give_the_restated_loops_tokens(B, T, steps, density, seed):
    step, kept = _schedule_with_keep(B, T, steps, density, seed, full_kept=(B - 1, ))
    rng = np.random.default_rng(seed + 100)
    tex = rng.integers(0, 18, B * T)
    src = rng.integers(0, 1024, B * T)
    want = _reference_loop(step, tex, src, kept, B, T, steps)
    assert (want != MASK_ID).all()
    assert (want.reshape(-1)[kept] == (src + 1024 * tex)[kept]).all()
    for compact, shrink in ((True, False), (True, True), (False, False)):
        got = _rounds_loop(step, tex, src, kept, B, T, compact, shrink)
        assert (got == want).all(), (compact, shrink)


@pytest.mark.parametrize('B,T,steps,density,seed', [(4, 32, 16, 0.5, 0), (7, 16, 40, 0.25, 1), (1, 8, 3, 0.5, 3)])
def test_plan_rounds_with_kept_rows(B, T, steps, density, seed):
    step, kept = _schedule_with_keep(B, T, steps, density, seed, full_kept=(B - 1, ) if B > 1 else ())
    check_plan(step, np.random.default_rng(seed + 100).integers(0, 18, B * T), B, T, steps, kept)
