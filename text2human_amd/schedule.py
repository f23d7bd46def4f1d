"""The unmasking schedule of `sample_fn` (models/sample_model.py:279-317), computed BEFORE the
transformer runs.

In the reference loop the tokens that change at step t are `rand([B,T]) < 1/t` minus the ones
already unmasked, and the only other consumer of the generator is one full `[B*T, n_class]`
`exponential_` draw per head that has a changed token at that step.  Nothing of this depends on
the transformer's logits: the whole schedule -- which row changes at which step, and the
generator offset of every draw -- is a function of the seed and of the texture map.  Two
consequences, both used by engine.sample_tokens:

* no host round trip inside the sampling loop (the reference's data-dependent `if`,
  sample_model.py:301-302, is resolved up front);
* a sample whose tokens do not change at a step never has its logits read there, its `x_t` does
  not move, and samples never interact (attention is per sample): every sample can walk through
  ITS OWN active steps.  Round r evaluates, for every sample, its r-th active step -- about
  0.865 * steps rounds of the full batch instead of `steps`, with the same tokens (up to fp32
  summation-order ties in the last layer's few-rows tail, whose tile depends on the row count).

This module is host-side integer bookkeeping (numpy); the draws themselves are reproduced on the
device (t2h_unmask_schedule / t2h_sample_heads) or taken from an explicit noise source.
"""
from collections import namedtuple

import numpy as np


def as_int64(u64):
    """A uint64 (torch's `initial_seed()` after `torch.seed()` / a negative `manual_seed`) as the int64 with the
    same bits: what an int64 device tensor can hold; the kernels read the word back as uint64."""
    u = int(u64) & 0xFFFFFFFFFFFFFFFF
    return u - (1 << 64) if u >= (1 << 63) else u


def draw_offsets(head_mask, steps, offset0, rand_inc, expo_inc, n_heads):
    """Generator offsets of the reference's draws.

    head_mask[t] (t = steps .. 1): bit h set iff head h samples at step t.  Returns
    (rand_off int64 [steps + 1], expo_off int64 [steps + 1, n_heads] (-1 where the head draws
    nothing), final offset): the generator holds rand_off[t] before the `rand` of step t and
    expo_off[t, h] before head h's `exponential_` of that step (heads in ascending order)."""
    head_mask = np.asarray(head_mask, dtype=np.int64)
    rand_off = np.zeros(steps + 1, dtype=np.int64)
    expo_off = np.full((steps + 1, n_heads), -1, dtype=np.int64)
    cur = int(offset0)
    for t in range(steps, 0, -1):
        rand_off[t] = cur
        cur += int(rand_inc)
        m = int(head_mask[t])
        for h in range(n_heads):
            if (m >> h) & 1:
                expo_off[t, h] = cur
                cur += int(expo_inc)
    return rand_off, expo_off, cur


def draw_offsets_per_image(head_mask, steps, rand_inc, expo_inc, n_heads):
    """draw_offsets for per-image seeds: every image walks its OWN private stream from offset 0 with
    its own head mask -- head_mask [B, steps + 1], the increments those of one image's draws.  Returns (expo_off int64
    [B, steps + 1, n_heads], final int64 [B]: where image b's stream ends, the generator offset of the call on image b
    alone)."""
    head_mask = np.asarray(head_mask, dtype=np.int64)
    per = [draw_offsets(m, steps, 0, rand_inc, expo_inc, n_heads) for m in head_mask]
    return np.stack([p[1] for p in per]), np.array([p[2] for p in per], dtype=np.int64)


def _kept_mask(step_of_row, kept):
    """(steps int64 [B*T], kept bool [B*T]).  Without `kept` every row needs a step >= 1; with it (region editing: the
    rows that keep their source token) exactly the kept rows have step 0."""
    steps = np.asarray(step_of_row, dtype=np.int64).reshape(-1)
    if kept is None:
        if steps.size and steps.min() < 1:
            raise ValueError('every token row must have a step >= 1')
        return steps, np.zeros(steps.size, dtype=bool)
    kept = np.asarray(kept).reshape(-1).astype(bool)
    if kept.size != steps.size:
        raise ValueError(f'kept has {kept.size} rows, the schedule {steps.size}')
    if (steps[~kept] < 1).any() or (steps[kept] != 0).any():
        raise ValueError('every token row that is not kept must have a step >= 1, every kept row step 0')
    return steps, kept


def group_rounds(step_of_row, B, T, compact=True, kept=None):
    """Rounds of the sampling loop.

    step_of_row int [B*T]: the step (>= 1) at which each token row changes.  compact=True: round r
    of sample b is its r-th active step (descending t); compact=False: round r is the r-th step (of
    any sample) that changes a token, for every sample alike -- the reference's own loop minus the
    steps that change nothing.  kept bool [B*T] (region editing): rows that keep their source token
    (step 0); they take part in no round, and `order` lists only the other rows.  Returns
      order        int64 [B*T]   row ids sorted by (round, row) (without the kept rows),
      start        int64 [R + 1] order[start[r]:start[r + 1]] are the rows of round r,
      round_steps  int32 [R, B]  the step sample b is at in round r (0 = idle in that round)."""
    flat_steps, kept_flat = _kept_mask(step_of_row, kept)
    steps = flat_steps.reshape(B, T)
    live = ~kept_flat.reshape(B, T)
    if compact:
        uniq = [np.unique(steps[b][live[b]]) for b in range(B)]   # ascending
    else:
        g = np.unique(steps[live])
        uniq = [g] * B
    n_rounds = max([len(u) for u in uniq] + [0])
    rnd = np.full((B, T), n_rounds, dtype=np.int64)                # kept rows: after the last round
    round_steps = np.zeros((n_rounds, B), dtype=np.int32)
    for b in range(B):
        u = uniq[b]
        rnd[b][live[b]] = len(u) - 1 - np.searchsorted(u, steps[b][live[b]])   # descending t = ascending round
        if compact:
            round_steps[:len(u), b] = u[::-1]
        else:
            present = np.isin(u, steps[b][live[b]])
            round_steps[:len(u), b] = np.where(present, u, 0)[::-1]
    flat = rnd.reshape(-1)
    order = np.lexsort((np.arange(B * T), flat)).astype(np.int64)
    start = np.searchsorted(flat[order], np.arange(n_rounds + 1)).astype(np.int64)
    if kept is not None:
        order = order[:start[-1]]
    return order, start, round_steps


def leave_order(step_of_row, B, T, kept=None):
    """Order of the samples for a compact schedule in which FINISHED samples leave the batch: samples sorted by the
    number of rounds they take part in (= their distinct steps), descending, ties in index order.  With the batch in
    this order the samples still active in round r are exactly the first k_r, so the transformer of round r runs on
    the first k_r * T rows only (about 2 % of the evaluations at B = 8, 3.5 % at B = 32, are (sample, round) pairs of
    samples that have no step left).  kept (region editing): kept rows count for no round -- a fully kept sample has
    none and sorts last.  -> (perm int64 [B]: new position -> original sample, rounds per sample in the new order)"""
    flat_steps, kept_flat = _kept_mask(step_of_row, kept)
    steps, live = flat_steps.reshape(B, T), ~kept_flat.reshape(B, T)
    n_act = np.array([len(np.unique(steps[b][live[b]])) for b in range(B)], dtype=np.int64)
    perm = np.argsort(-n_act, kind='stable').astype(np.int64)
    return perm, n_act[perm]


# plan_rounds' result, in the SCHEDULE's sample order.  perm int64 [B]: new position -> original sample (None: the caller's
# order); order / start / round_steps: group_rounds; active int64 [R]: samples still running in round r, a prefix of the
# batch; rng_rows int32 / offs int64: of every listed row, its row in the caller's batch / its draw's generator offset.
RoundPlan = namedtuple('RoundPlan', 'perm order start round_steps kept active rng_rows offs')


def plan_rounds(step_of_row, tex_host, B, T, compact, shrink, kept=None, expo_off=None, per_image=False):
    """What engine.build_schedule decides on the host from what the device hands back (step_of_row, tex_host, kept:
    [B*T], the caller's order) and draw_offsets' expo_off.  shrink (compact only): finished samples leave the batch.
    per_image (per-image seeds): expo_off is [B, steps + 1, n_heads] (draw_offsets_per_image, the caller's sample
    order) -- a row's offset is taken from its own image's table and its noise row is local (row % T), reordered batch
    or not."""
    perm = rng_rows = active = offs = None
    if per_image and (expo_off is None or np.ndim(expo_off) != 3 or len(expo_off) != B):
        raise ValueError(f'plan_rounds(per_image=True): expo_off [{B}, steps + 1, n_heads] expected')
    if not per_image and expo_off is not None and np.ndim(expo_off) != 2:
        raise ValueError('plan_rounds: expo_off [steps + 1, n_heads] expected (per_image=True takes one table per image)')
    if shrink and compact and B > 1:
        perm, _ = leave_order(step_of_row, B, T, kept)
        if (perm == np.arange(B)).all():
            perm = None
    if perm is not None:
        orig_row = (perm[:, None] * T + np.arange(T)[None, :]).reshape(-1)  # original row of every reordered row
        step_of_row, tex_host = step_of_row[orig_row], tex_host[orig_row]
        kept = kept[orig_row] if kept is not None else None
    order, start, round_steps = group_rounds(step_of_row, B, T, compact, kept)
    if per_image:
        image = order // T if perm is None else perm[order // T]  # the caller's image of every listed row
        offs = expo_off[image, step_of_row[order], tex_host[order]]
        assert (offs >= 0).all()
    elif expo_off is not None:
        offs = expo_off[step_of_row[order], tex_host[order]]
        assert (offs >= 0).all()
    if shrink and compact:
        active = (round_steps > 0).sum(1).astype(np.int64)
        assert all((round_steps[r, :active[r]] > 0).all() for r in range(len(active)))  # a prefix of the batch
    if per_image:
        rng_rows = (order % T).astype(np.int32)
    elif perm is not None:
        rng_rows = orig_row[order].astype(np.int32)
    return RoundPlan(perm, order, start, round_steps, kept, active, rng_rows, offs)


def in_caller_order(perm, B, T):
    """int64 [B*T]: x[..., in_caller_order(perm, B, T)] = the token rows x of a batch reordered by `perm`, as the caller had them"""
    inv = np.arange(B) if perm is None else np.argsort(perm)
    return (inv[:, None] * T + np.arange(T)[None, :]).reshape(-1)


def padded_tables(order, per_row, start, maxr):
    """The schedule as fixed-width tables for graph replay (engine.RoundGraph, t2h_schedule_advance):
    row r of the result = the rows of round r, padded to `maxr` entries with copies of the round's LAST
    row (sampling a row twice writes the same token twice), and the same for the per-row values
    (generator offsets).  -> (rows int32 [R, maxr], values int64 [R, maxr])"""
    n_rounds = len(start) - 1
    rows_tbl = np.empty((n_rounds, maxr), dtype=np.int32)
    val_tbl = np.empty((n_rounds, maxr), dtype=np.int64)
    for r in range(n_rounds):
        lo, hi = int(start[r]), int(start[r + 1])
        k = hi - lo
        if not 0 < k <= maxr:
            raise ValueError(f'round {r} has {k} rows, tables are {maxr} wide')
        rows_tbl[r, :k], val_tbl[r, :k] = order[lo:hi], per_row[lo:hi]
        rows_tbl[r, k:], val_tbl[r, k:] = order[hi - 1], per_row[hi - 1]
    return rows_tbl, val_tbl


class RoundTables:
    """Host side of graph replay (engine.RoundGraph.run): the run's schedule as padded tables plus the round
    cursor the captured graph advances.  `advance()` is the CPU statement of t2h_schedule_advance -- copy round
    *ctr of the tables into the staging rows / values, then ctr += 1 -- so the bookkeeping (how many replays, what
    each replay sees, that the padding only repeats rows of the same round) can be exercised without a GPU
    (tests/test_schedule.py, the 2-rank gloo run of tests/test_bench_dist.py)."""

    def __init__(self, order, per_row, start, maxr, per_row32=None):
        self.rows_tbl, self.val_tbl = padded_tables(order, per_row, start, maxr)
        # second per-row channel (int32: the rows of the reference's noise tensor when the samples were reordered)
        self.aux32_tbl = (padded_tables(order, np.asarray(per_row32, dtype=np.int64), start, maxr)[1].astype(np.int32)
                          if per_row32 is not None else None)
        self.n_rounds, self.maxr = len(start) - 1, int(maxr)
        self.ctr = 0

    def advance(self):
        if self.ctr >= self.n_rounds:
            raise IndexError(f'round cursor {self.ctr} past the {self.n_rounds} rounds of this run')
        r = self.ctr
        self.ctr += 1
        return self.rows_tbl[r].copy(), self.val_tbl[r].copy()

    def replay(self, body, first_eager=True):
        """The launch pattern of RoundGraph.run: round 0 eagerly on the run that captures (first_eager), then one
        replay per remaining round; body(rows, values) is called once per round.  -> number of replays."""
        self.ctr = 0
        for _ in range(self.n_rounds):
            body(*self.advance())
        return self.n_rounds - (1 if first_eager and self.n_rounds else 0)


def confidence_schedule(m0, rounds):
    """Confidence-ordered decoding ("Confidence-ordered decoding"): rows still masked after every round of a
    sample that starts with m0 masked rows.  m_r = floor(m0 cos(pi/2 r / R)) in float64, then forced to m_R = 0 and
    m_r <= max(m_{r-1} - 1, 0): every round commits at least one row while any is masked.
    -> (m int64 [R + 1] with m[0] = m0, k int64 [R] with k[r - 1] = m[r - 1] - m[r] = rows committed in round r)"""
    m0, R = int(m0), int(rounds)
    if R < 1 or m0 < 0:
        raise ValueError(f'confidence_schedule: rounds >= 1 and m0 >= 0 expected, got {rounds}, {m0}')
    m = np.zeros(R + 1, dtype=np.int64)
    m[0] = m0
    for r in range(1, R + 1):
        v = 0 if r == R else int(np.floor(np.float64(m0) * np.cos(np.float64(np.pi) / 2 * (np.float64(r) / np.float64(R)))))
        m[r] = min(v, max(int(m[r - 1]) - 1, 0))
    return m, m[:-1] - m[1:]


def confidence_choice_temps(rounds, choice_temp):
    """tau_r = choice_temp (1 - r / R), r = 1 .. R (float64 on the host, rounded once to the fp32 the kernel reads)"""
    R = int(rounds)
    r = np.arange(1, R + 1, dtype=np.float64)
    return (np.float64(choice_temp) * (1.0 - r / np.float64(R))).astype(np.float32)


def confidence_tables(m0, rounds, choice_temps, width=None):
    """Per-image confidence schedules ("Per-image sampling controls") as the [R][width] tables
    t2h_schedule_advance walks, R = max rounds: column b of k = confidence_schedule(m0[b], rounds[b])'s commits in rows
    0 .. rounds[b] - 1 and zero below -- image b is complete after its own last round --, column b of tau =
    confidence_choice_temps(rounds[b], choice_temps[b]), zero below.  -> (k int32 [R, width], tau float32 [R, width])"""
    B = len(m0)
    if not (len(rounds) == len(choice_temps) == B):
        raise ValueError(f'confidence_tables: {B} images, {len(rounds)} rounds, {len(choice_temps)} choice temperatures')
    R = max(int(r) for r in rounds)
    w = max(B, 2) if width is None else int(width)
    k_tbl, tau_tbl = np.zeros((R, w), dtype=np.int32), np.zeros((R, w), dtype=np.float32)
    for b in range(B):
        k_tbl[:int(rounds[b]), b] = confidence_schedule(int(m0[b]), rounds[b])[1]
        tau_tbl[:int(rounds[b]), b] = confidence_choice_temps(rounds[b], choice_temps[b])
    return k_tbl, tau_tbl


def stats(round_steps, steps, active=None, kept=None):
    """Evaluation counts for the bench line: (sample, step) pairs the reference evaluates, pairs that
    change a token (the ones whose logits are read), rounds launched, and the (sample, round) pairs the
    transformer was actually run for (`active[r]` samples in round r; default: the whole batch).  With
    `kept` (region editing) also the number of kept rows."""
    n_rounds, B = round_steps.shape
    launched = int(n_rounds * B) if active is None else int(np.asarray(active).sum())
    out = dict(rounds=int(n_rounds), steps=int(steps), batch=int(B),
               sample_steps_possible=int(B * steps),
               sample_steps_needed=int((round_steps > 0).sum()),
               sample_steps_launched=launched)
    if kept is not None:
        out['rows_kept'] = int(np.asarray(kept).astype(bool).sum())
    return out
