"""Scoring a given token map on the CPU: t2h_score_heads / t2h_score_heads_per_sample of
csrc/sampler.hip through tests/emu.

What is pinned here: a token that t2h_sample_heads drew scores the very bits that launch wrote (logp, x_t, out_idx and
the logits workspace), through the scalar and the per-image entry point; rows that are not listed are not written, a row
listed twice is consistent, rank == NULL writes no rank, and none of the noise / truncation fields is read; the mode has
rank 0 and the row's largest value, the least likely class rank n_class - 1, bit-equal logits share a rank, a target
outside [0, n_class) gives NaN / -1 and touches nothing else; the value is the float64 log-softmax within 8 x what
torch's own float32 costs on the same inputs, on targets the model did not draw; rank is exact on the kernel's logits.

The small class count is n_class = 200, below the 1024 threads of the scoring workgroup and the 256 of the logits
workgroup: the unchanged logits kernel accepts it (its eight class slices are 25 wide, the last classes of a slice are
clamped loads whose stores are guarded), so no larger substitute is needed."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, 'emu'))
sys.path.insert(0, HERE)
import build_emu  # noqa: E402
import per_image_ref as PI  # noqa: E402
import score_ref as ref  # noqa: E402
from test_logp_emulated import B, C, MASK_ID, N, N_CLASS, N_HEADS, SETS, T, TEMPS, _problem  # noqa: E402

pytestmark = pytest.mark.skipif(not build_emu.available(), reason='no host clang++ for the emulation build')

SENTINEL = 12345.0
RANK_SENTINEL = -777
OUT_SENTINEL = -5          # (not -1: an untouched out_idx entry must be told from a written -1)


@pytest.fixture(scope='module')
def lib():
    from text2human_amd import _lib
    so = build_emu.load('sampler.hip')
    for name in ('t2h_sample_heads', 't2h_sample_heads_per_sample', 't2h_score_heads', 't2h_score_heads_per_sample'):
        assert getattr(so, name).argtypes == _lib.SIGNATURES[name][1]
    return so


@pytest.fixture(scope='module')
def pb():
    return _problem()


def _args(pb, listed, temp, n_class, w):
    from text2human_amd._lib import SampleHeadsArgs
    a = SampleHeadsArgs()
    t = dict(rows=torch.tensor(list(listed), dtype=torch.int32),
             x_t=torch.full((N, ), MASK_ID, dtype=torch.int64),
             out=torch.full((N_HEADS, N), OUT_SENTINEL, dtype=torch.int64),
             ws=torch.zeros(len(listed), n_class), lp=torch.full((N, ), SENTINEL))
    a.hidden, a.lnf_gamma, a.lnf_beta, a.w_heads = (pb['hidden'].data_ptr(), pb['gamma'].data_ptr(), pb['beta'].data_ptr(),
                                                    w.data_ptr())
    a.rows, a.tex, a.x_t, a.out_idx = t['rows'].data_ptr(), pb['tex'].data_ptr(), t['x_t'].data_ptr(), t['out'].data_ptr()
    a.temp, a.n_rows, a.n, a.C, a.n_class, a.n_heads = temp, len(listed), N, C, n_class, N_HEADS
    a.logits_ws, a.logp = t['ws'].data_ptr(), t['lp'].data_ptr()
    return a, t


def _result(t, listed, rank=None):
    distinct = list(dict.fromkeys(listed))
    return dict(rows=np.asarray(distinct), x_t=t['x_t'].numpy(), out=t['out'].numpy(), logp=t['lp'].numpy(),
                ws=t['ws'].numpy()[[list(listed).index(q) for q in distinct]],
                rank=None if rank is None else rank.numpy())


def draw(lib, pb, listed, temp=1.0, table=None):
    """t2h_sample_heads[_per_sample], two-launch form with logp, on `listed`"""
    a, t = _args(pb, listed, temp if table is None else -1.0, N_CLASS, pb['w'])
    for h in range(N_HEADS):
        a.expo[h] = pb['expo'].data_ptr()
    if table is not None:
        a.top_k, a.top_p_q = 0, 0
        tbl = torch.from_numpy(PI.table(table))
        rc = lib.t2h_sample_heads_per_sample(ctypes.byref(a), tbl.data_ptr(), T, None)
    else:
        rc = lib.t2h_sample_heads(ctypes.byref(a), None)
    assert rc == 0, lib.emu_last_error()
    return _result(t, listed)


def score(lib, pb, targets, listed, temp=1.0, table=None, rank=True, garbage=False, n_class=N_CLASS, w=None):
    """t2h_score_heads[_per_sample] on `listed` with targets int64 [N_HEADS, N]; every row that is not listed must keep
    its sentinels (checked here, for every launch of this file)"""
    from text2human_amd._lib import ScoreOut
    a, t = _args(pb, listed, temp if table is None else -1.0, n_class, pb['w'] if w is None else w)
    rk = torch.full((N, ), RANK_SENTINEL, dtype=torch.int32)
    s = ScoreOut()
    targets = targets.contiguous()
    s.targets = targets.data_ptr()
    if rank:
        s.rank = rk.data_ptr()
    if garbage:   # nothing of the draw is read: dangling noise pointers, wild Philox fields, impossible truncation rules
        for h in range(N_HEADS):
            a.expo[h] = 0xdead0000 + 16 * h
            a.philox_offset[h] = 0x123456789 + h
        a.philox_seed, a.philox_grid_threads = 0xfeedfacecafe, 12345
        a.row_philox_offset = a.expo_rows = a.expo_slot = a.philox_seed_dev = a.rng_rows = 0xbad0000
        a.top_k, a.top_p_q = -7, 0xffffffff
    if table is not None:
        tbl = torch.from_numpy(PI.table(table))
        rc = lib.t2h_score_heads_per_sample(ctypes.byref(a), ctypes.byref(s), tbl.data_ptr(), T, None)
    else:
        rc = lib.t2h_score_heads(ctypes.byref(a), ctypes.byref(s), None)
    assert rc == 0, lib.emu_last_error()
    res = _result(t, listed, rk)
    off = np.setdiff1d(np.arange(N), res['rows'])
    assert (res['x_t'][off] == MASK_ID).all() and (res['logp'][off] == SENTINEL).all()
    assert (res['out'][:, off] == OUT_SENTINEL).all() and (res['rank'][off] == RANK_SENTINEL).all()
    if not rank:
        assert (res['rank'] == RANK_SENTINEL).all()                              # NULL: no rank is written
    return res


def _same(a, b, rows):
    """logp, x_t and out_idx equal as bytes on `rows`, and the logits of those rows"""
    at = lambda r: [list(r['rows']).index(q) for q in rows]
    return (a['logp'][rows].tobytes() == b['logp'][rows].tobytes() and a['x_t'][rows].tobytes() == b['x_t'][rows].tobytes()
            and a['out'][:, rows].tobytes() == b['out'][:, rows].tobytes()
            and a['ws'][at(a)].tobytes() == b['ws'][at(b)].tobytes())


# An emulated launch costs about a second per listed row, so every launch lists a handful: two rows per image, in no
# particular order, one of them twice (a padded round's list)
DRAWN = [37, 3, 20, 44, 9, 29]
LISTED = DRAWN + [DRAWN[2]]


def image_rows(b):
    return [r for r in DRAWN if r // T == b]


@pytest.fixture(scope='module')
def drawn(lib, pb):
    return draw(lib, pb, LISTED)


@pytest.fixture(scope='module')
def scored(lib, pb, drawn):
    """the round trip: the drawn tokens handed back as targets"""
    return score(lib, pb, torch.from_numpy(drawn['out'].copy()), LISTED)


def test_a_drawn_map_scores_the_bits_the_draw_wrote(pb, drawn, scored):
    assert len(set(pb['tex'][DRAWN].tolist())) >= 4                              # mixed textures: the heads are routed
    assert _same(drawn, scored, DRAWN)
    lp = scored['logp'][DRAWN]
    assert np.isfinite(lp).all() and (lp <= 0).all()
    # the targets' other entries (-5 off-texture, other rows) were never read: only each row's own texture counts
    assert (scored['rank'][DRAWN] >= 0).all() and (scored['rank'][DRAWN] < N_CLASS).all()


def test_the_per_image_entry_point_round_trips_and_matches_the_scalar_launches(lib, pb):
    one_each = [image_rows(b)[0] for b in range(B)]                              # one row per image, one listed twice
    listed = one_each + [one_each[1]]
    mixed = draw(lib, pb, listed, table=SETS)                                    # (images 1, 2 truncate: other tokens)
    targets = torch.from_numpy(mixed['out'].copy())
    got = score(lib, pb, targets, listed, table=SETS)
    assert _same(mixed, got, one_each)
    for b, (temp, _, _) in enumerate(SETS):
        rows = one_each[b:b + 1]
        want = score(lib, pb, targets, rows, temp=temp)                          # the scalar launch at the image's temp
        assert _same(got, want, rows) and got['rank'][rows].tobytes() == want['rank'][rows].tobytes(), b
    r0 = one_each[:1]
    other = score(lib, pb, targets, r0, temp=TEMPS[1])                           # the temperature IS read per image
    assert (other['logp'][r0] != got['logp'][r0]).all()


def test_observer_rules(lib, pb, drawn, scored):
    targets = torch.from_numpy(drawn['out'].copy())
    few = [DRAWN[0], DRAWN[3], DRAWN[0]]
    quiet = score(lib, pb, targets, few, rank=False)                             # (unlisted rows, NULL rank: in score())
    rows = sorted(set(few))
    assert _same(quiet, scored, rows)
    wild = score(lib, pb, targets, few, garbage=True)
    assert _same(wild, scored, rows) and wild['rank'][rows].tobytes() == scored['rank'][rows].tobytes()


def test_chosen_targets(lib, pb, drawn, scored):
    r_max, r_min, r_neg, r_big = DRAWN[:4]
    lg = {r: drawn['ws'][list(drawn['rows']).index(r)] for r in DRAWN}
    tex = pb['tex']
    targets = torch.from_numpy(drawn['out'].copy())
    targets[tex[r_max], r_max] = int(lg[r_max].argmax())
    targets[tex[r_min], r_min] = int(lg[r_min].argmin())
    targets[tex[r_neg], r_neg] = -1
    targets[tex[r_big], r_big] = N_CLASS
    got = score(lib, pb, targets, DRAWN[:4])
    assert got['rank'][r_max] == 0 and got['rank'][r_min] == N_CLASS - 1
    # the largest of the row: on the kernel's own logits the float64 log-softmax of no class exceeds it.  What float32
    # may cost there: l_tok - max is exactly 0 at the mode; se is 1024 expf values (1 ulp each) added on a tree of depth
    # 1 + 6 + 15, so its relative error -- the absolute error of its logarithm -- is below 23 x 2^-24; logf adds one ulp
    # of a result below 8, 2^-21.  Together below 31 x 2^-24.
    best = ref.logits_logp(lg[r_max][None].repeat(N_CLASS, 0), np.arange(N_CLASS)).max()
    assert got['logp'][r_max] >= scored['logp'][r_max] and abs(got['logp'][r_max] - best) <= 31 * 2.0**-24
    assert got['logp'][r_min] < scored['logp'][r_min] < 0
    assert got['x_t'][r_max] == int(lg[r_max].argmax()) + N_CLASS * int(tex[r_max])
    assert got['out'][tex[r_min], r_min] == int(lg[r_min].argmin())
    for r in (r_neg, r_big):   # never indexes anything: NaN, -1, the state untouched, return code OK (score())
        assert np.isnan(got['logp'][r]) and got['rank'][r] == -1
        assert got['x_t'][r] == MASK_ID and (got['out'][:, r] == OUT_SENTINEL).all()


def test_bit_equal_logits_share_a_rank(lib, pb, drawn):
    row = DRAWN[4]
    h = int(pb['tex'][row])
    lg = drawn['ws'][list(drawn['rows']).index(row)]
    order = np.argsort(-lg, kind='stable')
    j1, j2 = int(order[5]), int(order[700])                                      # a likely class and an unlikely one
    w = pb['w'].clone()
    w[h, j2] = w[h, j1]                                                          # identical weight rows: bit-equal logits
    res = []
    for j in (j1, j2):
        targets = torch.full((N_HEADS, N), -1, dtype=torch.int64)
        targets[h, row] = j
        res.append(score(lib, pb, targets, [row], w=w))
    a, b = res
    assert a['ws'][0, j1].tobytes() == a['ws'][0, j2].tobytes() == lg[j1].tobytes()
    want = int((a['ws'][0] > a['ws'][0, j1]).sum())
    assert want == 5                                                             # strictly greater: the tie counts nobody
    assert a['rank'][row] == b['rank'][row] == want
    assert a['logp'][row].tobytes() == b['logp'][row].tobytes()
    assert a['x_t'][row] == j1 + N_CLASS * h and b['x_t'][row] == j2 + N_CLASS * h


VALUE_ROWS = [r for r in range(N) if r % 6 == 1]                                 # eight rows, all three images


@pytest.mark.parametrize('temp', TEMPS, ids=[f'temp {t}' for t in TEMPS])
def test_value_and_rank_on_targets_the_model_did_not_draw(lib, pb, temp):
    g = torch.Generator().manual_seed(int(temp * 10))
    targets = torch.randint(0, N_CLASS, (N_HEADS, N), generator=g)               # uniformly random classes
    got = score(lib, pb, targets, VALUE_ROWS, temp=temp)
    rows = np.asarray(VALUE_ROWS)
    tok = targets[pb['tex'][rows], torch.from_numpy(rows)].numpy()
    args = (pb['hidden'], pb['gamma'], pb['beta'], pb['w'], pb['tex'], rows, tok, temp)
    want = ref.row_logp(*args)
    err = float(np.abs(got['logp'][rows].astype(np.float64) - want).max())
    f32 = ref.f32_error(*args)
    print(f'temp {temp}: score vs float64 max abs err {err:.3e}; float32 torch restatement on these inputs {f32:.3e} '
          f'(bound {8 * f32:.3e}); spread of the values {want.std():.3f}')
    assert err <= 8 * f32, (err, f32)
    assert want.std() >= 100 * 8 * f32                                           # a mis-routed row cannot hide
    assert got['rank'][rows].tolist() == ref.rank(got['ws'], tok).tolist()
    assert (got['x_t'][rows] == tok + N_CLASS * pb['tex'][rows].numpy()).all()
    assert (got['out'][pb['tex'][rows].numpy(), rows] == tok).all()


def test_a_class_count_below_the_workgroup_size(lib, pb):
    n_class, temp = 200, 0.7
    w = pb['w'][:, :n_class].contiguous()
    rows = np.asarray([2, 21, 40, 47])
    g = torch.Generator().manual_seed(5)
    targets = torch.randint(0, n_class, (N_HEADS, N), generator=g)
    got = score(lib, pb, targets, rows.tolist(), temp=temp, n_class=n_class, w=w)
    tok = targets[pb['tex'][rows], torch.from_numpy(rows)].numpy()
    args = (pb['hidden'], pb['gamma'], pb['beta'], w, pb['tex'], rows, tok, temp)
    err = float(np.abs(got['logp'][rows].astype(np.float64) - ref.row_logp(*args)).max())
    f32 = ref.f32_error(*args)
    print(f'n_class {n_class}: score vs float64 max abs err {err:.3e}; float32 torch restatement {f32:.3e}')
    assert err <= 8 * f32, (err, f32)
    assert got['rank'][rows].tolist() == ref.rank(got['ws'], tok).tolist()
    assert (got['x_t'][rows] == tok + n_class * pb['tex'][rows].numpy()).all()


@pytest.mark.parametrize('missing', ['logits_ws', 'logp', 'targets', 'score', 'params'])
def test_argument_checks_write_nothing(lib, pb, missing):
    from text2human_amd._lib import ScoreOut
    a, t = _args(pb, DRAWN[:2], 1.0, N_CLASS, pb['w'])
    targets = torch.zeros((N_HEADS, N), dtype=torch.int64)
    rk = torch.full((N, ), RANK_SENTINEL, dtype=torch.int32)
    s = ScoreOut()
    s.targets, s.rank = targets.data_ptr(), rk.data_ptr()
    if missing in ('logits_ws', 'logp'):
        setattr(a, missing, None)
    elif missing == 'targets':
        s.targets = None
    tbl = torch.from_numpy(PI.table(SETS))
    sp = None if missing == 'score' else ctypes.byref(s)
    if missing == 'params':
        assert lib.t2h_score_heads_per_sample(ctypes.byref(a), sp, None, T, None) != 0
    else:
        assert lib.t2h_score_heads(ctypes.byref(a), sp, None) != 0
        assert lib.t2h_score_heads_per_sample(ctypes.byref(a), sp, tbl.data_ptr(), T, None) != 0
    assert (t['lp'] == SENTINEL).all() and (t['x_t'] == MASK_ID).all() and (t['out'] == OUT_SENTINEL).all()
    assert (t['ws'] == 0).all() and (rk == RANK_SENTINEL).all()
