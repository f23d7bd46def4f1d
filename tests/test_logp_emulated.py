"""Per-token log-probabilities of the sampling tail on the CPU: csrc/sampler.hip through tests/emu.

What is pinned here: the `logp` output changes nothing else (tokens, x_t, out_idx as bytes); rows that are not drawn are
not written; the one-launch and the two-launch form of the tail give the same bits; a row of a per-image launch has the
bits of the scalar launch with its image's settings; truncation changes the token, never the distribution the number is
taken under; the value is the float64 log-softmax within 8 x what torch's own float32 costs on the same inputs;
t2h_confidence_commit copies the confidence of the rows it commits; t2h_logp_summary counts, sums and takes the minimum
per image on a tree that does not depend on where the image sits in the batch."""
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
import logp_ref as ref  # noqa: E402
import per_image_ref as PI  # noqa: E402
import truncation_ref as TR  # noqa: E402

pytestmark = pytest.mark.skipif(not build_emu.available(), reason='no host clang++ for the emulation build')

MASK_ID = 18432
B, T = 3, 16
N, C, N_CLASS, N_HEADS = B * T, 512, 1024, 18
SENTINEL = 12345.0
TEMPS = (1.0, 0.7, 1.3)
# image 0: the defaults inside a truncating launch; 1: colder, top-k; 2: warmer, top-p
SETS = PI.settings(temp=TEMPS, top_k=(None, 5, None), top_p=(None, None, 0.6))

# what the kernels may differ from float64 by: 8 x what torch's own float32 costs on this file's inputs (logp_ref.py
# holds the measured values and the recipe; test_logp_against_float64 prints it again)
LOGP_ERR_F32 = ref.LOGP_ERR_F32


@pytest.fixture(scope='module')
def lib():
    from text2human_amd import _lib
    so = build_emu.load('sampler.hip')
    for name in ('t2h_sample_heads', 't2h_sample_heads_per_sample', 't2h_confidence_commit', 't2h_logp_summary'):
        assert getattr(so, name).argtypes == _lib.SIGNATURES[name][1]
    return so


def _problem(seed=73):
    g = torch.Generator().manual_seed(seed)
    hidden = torch.randn(N, C, generator=g) * 1.5 + 0.2
    gamma, beta = torch.randn(C, generator=g) * 0.2 + 1.0, torch.randn(C, generator=g) * 0.1
    w = torch.randn(N_HEADS, N_CLASS, C, generator=g) * 0.12
    tex = torch.randint(0, N_HEADS, (N, ), generator=g)
    expo = torch.empty(N, N_CLASS).exponential_(generator=g).contiguous()
    return dict(hidden=hidden, gamma=gamma, beta=beta, w=w, tex=tex, expo=expo)


# the drawn rows: every row but each sixth, in no particular order, one of them listed twice (a padded round's list)
ROWS = [r for r in range(N) if r % 6 != 4][::-1]
LISTED = ROWS + [ROWS[3]]


@pytest.fixture(scope='module')
def pb():
    return _problem()


def heads(lib, pb, temp=1.0, top_k=0, p_q=0, two_launch=True, logp=True, table=None, listed=None):
    """t2h_sample_heads (table: t2h_sample_heads_per_sample) on `listed` (default LISTED) -> dict(rows = the distinct
    listed rows, tok of those, x_t, out, ws of those, logp [N])"""
    from text2human_amd._lib import SampleHeadsArgs
    listed = LISTED if listed is None else list(listed)
    rows = torch.tensor(listed, dtype=torch.int32)
    a = SampleHeadsArgs()
    x_t, out = torch.full((N, ), MASK_ID, dtype=torch.int64), torch.full((N_HEADS, N), -1, dtype=torch.int64)
    ws = torch.zeros(len(listed), N_CLASS)
    lp = torch.full((N, ), SENTINEL)
    a.hidden, a.lnf_gamma, a.lnf_beta, a.w_heads = (pb['hidden'].data_ptr(), pb['gamma'].data_ptr(), pb['beta'].data_ptr(),
                                                    pb['w'].data_ptr())
    a.rows, a.tex, a.x_t, a.out_idx = rows.data_ptr(), pb['tex'].data_ptr(), x_t.data_ptr(), out.data_ptr()
    a.temp, a.n_rows, a.n, a.C, a.n_class, a.n_heads = (temp if table is None else -1.0), len(listed), N, C, N_CLASS, N_HEADS
    a.top_k, a.top_p_q = top_k, p_q
    if two_launch:
        a.logits_ws = ws.data_ptr()
    for h in range(N_HEADS):
        a.expo[h] = pb['expo'].data_ptr()
    if logp:
        a.logp = lp.data_ptr()
    if table is not None:
        tbl = torch.from_numpy(PI.table(table))
        rc = lib.t2h_sample_heads_per_sample(ctypes.byref(a), tbl.data_ptr(), T, None)
    else:
        rc = lib.t2h_sample_heads(ctypes.byref(a), None)
    assert rc == 0, lib.emu_last_error()
    distinct = list(dict.fromkeys(listed))
    r = torch.tensor(distinct)
    tok = out[pb['tex'][r], r]
    assert torch.equal(x_t[r], tok + N_CLASS * pb['tex'][r])
    not_listed = np.setdiff1d(np.arange(N), distinct)
    assert (x_t.numpy()[not_listed] == MASK_ID).all() and (lp.numpy()[not_listed] == SENTINEL).all()
    if not logp:
        assert (lp == SENTINEL).all()                                            # NULL: nothing is written
    return dict(rows=np.asarray(distinct), tok=tok.numpy(), x_t=x_t.numpy(), out=out.numpy(),
                ws=ws.numpy()[[listed.index(q) for q in distinct]], logp=lp.numpy())


# An emulated launch costs about a second per listed row (1024 OS threads per row), so only the launches that need
# every row list every row; rows are drawn independently, and a launch that is compared on some rows lists those.
def image_rows(b):
    return [r for r in ROWS if r // T == b]


FEW = [ROWS[0], ROWS[15], ROWS[30], ROWS[0]]                                     # one row per image, one listed twice


@pytest.fixture(scope='module')
def plain(lib, pb):
    """the scalar launches per temperature, two-launch form, with logp: every row at temp 1.0, else the rows of the image
    that has that temperature in SETS"""
    return {t: heads(lib, pb, temp=t, listed=None if b == 0 else image_rows(b)) for b, t in enumerate(TEMPS)}


def _same_on(a, b, rows):
    """the same tokens, as bytes, on `rows` (x_t and every head's list)"""
    return a['x_t'][rows].tobytes() == b['x_t'][rows].tobytes() and a['out'][:, rows].tobytes() == b['out'][:, rows].tobytes()


ALL = np.arange(N)


def test_logp_changes_no_token_and_writes_only_the_listed_rows(lib, pb, plain):
    with_lp = plain[1.0]
    without = heads(lib, pb, logp=False)
    assert _same_on(with_lp, without, ALL) and with_lp['ws'].tobytes() == without['ws'].tobytes()
    lp = with_lp['logp']
    assert N - len(ROWS) == N // 6                                               # (rows that keep the sentinel: heads())
    assert np.isfinite(lp[ROWS]).all() and (lp[ROWS] <= 0).all() and (lp[ROWS] != SENTINEL).all()
    assert len(set(pb['tex'][ROWS].tolist())) >= 12                              # mixed textures: the heads are routed


def test_both_forms_of_the_tail_give_the_same_bits(lib, pb, plain):
    one = heads(lib, pb, two_launch=False)
    assert _same_on(one, plain[1.0], ALL) and one['logp'].tobytes() == plain[1.0]['logp'].tobytes()
    few = sorted(set(FEW))
    one_off = heads(lib, pb, two_launch=False, logp=False, listed=FEW)          # the one-launch instance without it
    assert _same_on(one_off, one, few)


def test_a_row_of_a_mixed_batch_has_the_bits_of_the_scalar_launch(lib, pb, plain):
    mixed = heads(lib, pb, table=SETS)
    few = sorted(set(FEW))
    assert _same_on(heads(lib, pb, table=SETS, logp=False, listed=FEW), mixed, few)
    one = heads(lib, pb, table=SETS, two_launch=False, listed=FEW)               # the one-launch per-image instance
    assert _same_on(one, mixed, few) and one['logp'][few].tobytes() == mixed['logp'][few].tobytes()
    assert _same_on(heads(lib, pb, table=SETS, two_launch=False, logp=False, listed=FEW), mixed, few)
    differs = 0
    for b, (temp, k, p_q) in enumerate(SETS):
        rows = image_rows(b)
        want = heads(lib, pb, temp=temp, top_k=k, p_q=p_q, listed=rows) if (k or p_q) else plain[temp]
        assert _same_on(mixed, want, rows), b
        assert mixed['logp'][rows].tobytes() == want['logp'][rows].tobytes(), b
        if b:   # ... and without its truncation rule at least one row of the image has another token and another value
            differs += int(mixed['logp'][rows].tobytes() != plain[temp]['logp'][rows].tobytes())
    assert differs == B - 1
    # the temperature is read per image: image 0's value under image 1's temperature is another number
    r0 = image_rows(0)[:2]
    other = heads(lib, pb, temp=TEMPS[1], listed=r0)
    assert (other['logp'][r0] != mixed['logp'][r0]).all()


@pytest.mark.parametrize('top_k,p', [(5, None), (0, 0.6)], ids=['top-k 5', 'top-p 0.6'])
def test_truncation_changes_the_token_never_the_distribution(lib, pb, plain, top_k, p):
    base = plain[1.0]
    rows = np.asarray(ROWS[::2])
    at = [ROWS.index(r) for r in rows]                                           # their places in base['tok'] / base['ws']
    p_q = TR.p_q_of(p) if p else 0
    cut = heads(lib, pb, top_k=top_k, p_q=p_q, listed=rows)
    few = sorted(set(rows[:3].tolist()))
    assert _same_on(heads(lib, pb, top_k=top_k, p_q=p_q, logp=False, listed=few), cut, few)
    assert cut['ws'].tobytes() == base['ws'][at].tobytes()                       # the logits are not touched
    same = cut['tok'] == base['tok'][at]
    assert same.any() and (~same).any()                                          # at least one row did change
    assert cut['logp'][rows[same]].tobytes() == base['logp'][rows[same]].tobytes()
    assert (cut['logp'][rows[~same]] != base['logp'][rows[~same]]).all()
    # elsewhere: the full-softmax value of the token actually drawn, against float64
    want = ref.row_logp(pb['hidden'], pb['gamma'], pb['beta'], pb['w'], pb['tex'], rows, cut['tok'], 1.0)
    err = np.abs(cut['logp'][rows].astype(np.float64) - want)
    print(f'truncated draw against float64: max abs err {err.max():.3e} (changed rows {err[~same].max():.3e})')
    assert err.max() <= 8 * LOGP_ERR_F32[1.0]


@pytest.mark.parametrize('b', range(B), ids=[f'temp {t}' for t in TEMPS])
def test_logp_against_float64(lib, pb, plain, b):
    temp = TEMPS[b]
    got = plain[temp]
    args = (pb['hidden'], pb['gamma'], pb['beta'], pb['w'], pb['tex'], got['rows'], got['tok'], temp)
    want = ref.row_logp(*args)
    err = float(np.abs(got['logp'][got['rows']].astype(np.float64) - want).max())
    f32 = ref.f32_error(*args)
    print(f'temp {temp}: logp vs float64 max abs err {err:.3e}; float32 torch restatement {f32:.3e} '
          f'(recorded {LOGP_ERR_F32[temp]:.3e}); spread of the values {want.std():.3f}')
    assert err <= 8 * LOGP_ERR_F32[temp], err
    assert want.std() >= 100 * 8 * LOGP_ERR_F32[temp]                            # a mis-routed row cannot hide


# ---- t2h_confidence_commit with logp

def _commit(lib, entry, conf, tok, tex, x_t, out, k, tau, u, logp):
    from text2human_amd._lib import ConfidenceCommitArgs
    nb, t = x_t.shape
    a = ConfidenceCommitArgs()
    kk, tt = torch.tensor(k, dtype=torch.int32), torch.tensor(tau, dtype=torch.float32)
    a.conf, a.tok, a.tex, a.u = conf.data_ptr(), tok.data_ptr(), tex.data_ptr(), u.data_ptr()
    a.k, a.tau, a.mask_id, a.x_t, a.out = kk.data_ptr(), tt.data_ptr(), MASK_ID, x_t.data_ptr(), out.data_ptr()
    a.B, a.T, a.n_heads, a.n_class = nb, t, out.shape[0], 1024
    if logp is not None:
        a.logp = logp.data_ptr()
    assert getattr(lib, entry)(ctypes.byref(a), None) == 0, lib.emu_last_error()


def test_commit_copies_the_confidence_of_the_rows_it_commits(lib):
    from test_confidence_emulated import _state
    t_len, H = 96, 4
    g, tex, tok, masked, x_t, out = _state(B, t_len, H, seed=9, masked_frac=0.7)
    conf = (-torch.rand(B, t_len, generator=g) * 9).contiguous()
    u = torch.rand(B * t_len, generator=g).contiguous()
    k = [7, 20, 0]
    x0, o0 = x_t.clone(), out.clone()
    _commit(lib, 't2h_confidence_commit', conf, tok, tex, x0, o0, k, [2.0], u, None)           # today's call
    x1, o1, lp1 = x_t.clone(), out.clone(), torch.full((B * t_len, ), SENTINEL)
    _commit(lib, 't2h_confidence_commit', conf, tok, tex, x1, o1, k, [2.0], u, lp1)
    x2, o2, lp2 = x_t.clone(), out.clone(), torch.full((B * t_len, ), SENTINEL)
    _commit(lib, 't2h_confidence_commit_per_sample', conf, tok, tex, x2, o2, k, [2.0] * B, u, lp2)
    assert torch.equal(x0, x1) and torch.equal(o0, o1) and torch.equal(x0, x2) and torch.equal(o0, o2)
    committed = (x1 != x_t).view(-1).numpy()
    assert committed.reshape(B, t_len).sum(1).tolist() == k
    lp1, lp2, c = lp1.numpy(), lp2.numpy(), conf.view(-1).numpy()
    assert lp1[committed].tobytes() == c[committed].tobytes() and (lp1[~committed] == SENTINEL).all()
    assert lp1.tobytes() == lp2.tobytes()


# ---- t2h_logp_summary

def _summary(lib, logp):
    nb, t = logp.shape
    lp = torch.from_numpy(np.ascontiguousarray(logp))
    s, m, c = torch.full((nb, ), 7.0), torch.full((nb, ), 7.0), torch.full((nb, ), 7, dtype=torch.int32)
    assert lib.t2h_logp_summary(lp.data_ptr(), nb, t, s.data_ptr(), c.data_ptr(), m.data_ptr(), None) == 0, lib.emu_last_error()
    return s.numpy(), c.numpy(), m.numpy()


def test_summary_skips_nan_and_does_not_depend_on_the_batch(lib):
    t_len = 512
    rng = np.random.default_rng(5)
    logp = (-rng.gamma(1.5, 2.0, size=(3, t_len))).astype(np.float32)            # log-probabilities: <= 0, spread
    logp[0] = np.nan                                                             # no drawn row
    logp[1, 1::2] = np.nan                                                       # every other row kept by an edit
    logp[2, 17] = 0.0                                                            # a legitimate value of a drawn row
    s, c, m = _summary(lib, logp)
    want_s, want_c, want_m, abs_s = ref.summary(logp)
    assert c.tolist() == want_c.tolist() == [0, t_len // 2, t_len]
    assert m.tobytes() == want_m.tobytes() and m[0] == np.inf and s[0] == 0.0
    # any order of adding n float32 numbers is within (n - 1) 2^-24 sum |x_i| of the exact sum (first order); with
    # n = 512 that is 512 ulp-scale of the sum of magnitudes, whatever the tree
    bound = 512 * 2.0**-24 * abs_s
    err = np.abs(s.astype(np.float64) - want_s)
    print(f'summary sums against float64: abs err {err.tolist()}, bound {bound.tolist()}')
    assert (err <= bound).all()
    for perm in ([2, 0, 1], [1, 2, 0]):
        sp, cp, mp = _summary(lib, logp[perm])
        for pos, b in enumerate(perm):
            assert sp[pos].tobytes() == s[b].tobytes() and cp[pos] == c[b] and mp[pos].tobytes() == m[b].tobytes(), (perm, b)
    s1, c1, m1 = _summary(lib, logp[2:3])                                        # alone in its batch
    assert s1.tobytes() == s[2:3].tobytes() and c1[0] == c[2] and m1.tobytes() == m[2:3].tobytes()
    assert lib.t2h_logp_summary(None, 3, t_len, None, None, None, None) != 0
