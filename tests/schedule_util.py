"""Shared by tests/test_schedule.py and tests/test_schedule_keep.py: what every schedule.plan_rounds result must satisfy."""
import numpy as np

from text2human_amd import schedule


def _head_masks(step, tex, steps, kept=None):
    live = np.ones(len(step), dtype=bool) if kept is None else ~kept
    mask = np.zeros(steps + 1, dtype=np.int64)
    for t, h in zip(step[live], tex[live]):
        mask[t] |= 1 << int(h)
    return mask


def check_plan(step, tex, B, T, steps, kept=None):
    """The properties of schedule.plan_rounds that engine.build_schedule relies on (also tests/test_schedule_keep.py)."""
    _, expo_off, _ = schedule.draw_offsets(_head_masks(step, tex, steps, kept), steps, 40, 4, 4 * T, 18)
    for compact, shrink in ((True, True), (True, False), (False, False), (False, True)):
        plan = schedule.plan_rounds(step, tex, B, T, compact, shrink, kept, expo_off)
        if B == 1 or not (shrink and compact):
            assert plan.perm is None
        perm = plan.perm if plan.perm is not None else np.arange(B)
        if shrink and compact and B > 1:
            assert (plan.perm is None) == (schedule.leave_order(step, B, T, kept)[0] == np.arange(B)).all()
        orig_row = (perm[:, None] * T + np.arange(T)[None, :]).reshape(-1)
        assert (orig_row[schedule.in_caller_order(plan.perm, B, T)] == np.arange(B * T)).all()
        if plan.perm is None:
            assert plan.rng_rows is None
        else:
            assert plan.rng_rows.dtype == np.int32 and (plan.rng_rows == orig_row[plan.order]).all()
        if shrink and compact:
            assert (np.diff(plan.active) <= 0).all()
            for r in range(len(plan.active)):
                assert (plan.round_steps[r, :plan.active[r]] > 0).all()
                assert (plan.order[plan.start[r]:plan.start[r + 1]] // T < plan.active[r]).all()
        else:
            assert plan.active is None
        src = orig_row[plan.order]                           # every listed row, as the caller numbers it
        if kept is None:
            assert plan.kept is None and sorted(src.tolist()) == list(range(B * T))
        else:
            assert (plan.kept == kept[orig_row]).all() and not plan.kept[plan.order].any()
            assert sorted(src.tolist()) == np.nonzero(~kept)[0].tolist()
        assert plan.offs.tolist() == [int(expo_off[step[i], tex[i]]) for i in src] and (plan.offs >= 0).all()
        assert schedule.plan_rounds(step, tex, B, T, compact, shrink, kept).offs is None
