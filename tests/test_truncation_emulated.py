"""Truncated sampling (top-k / top-p) on the CPU: the row-threshold selection of csrc/sampler.hip and the three pick
sites that use it, through tests/emu ("Truncated sampling"; the definition restated in
tests/truncation_ref.py).

top-k is exact: theta and the number of survivors equal the numpy restatement bit for bit, at the workgroup scope
(t2h_sample_heads) and the wave scope (t2h_confidence_tail).  top-p is checked against an fp64, order-free oracle as
strict <= kernel set <= permissive (the band is a bound on arithmetic, truncation_ref.D_BAND), on rows where the two
almost always coincide; and the two scopes must agree exactly, because only integers decide the kept set."""
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
import truncation_ref as ref  # noqa: E402

pytestmark = pytest.mark.skipif(not build_emu.available(), reason='no host clang++ for the emulation build')

MASK_ID = 18432
N_CLASS = 1024


@pytest.fixture(scope='module')
def lib():
    from text2human_amd import _lib
    so = build_emu.load('sampler.hip')
    assert so.t2h_truncation_threshold.argtypes == _lib.SIGNATURES['t2h_truncation_threshold'][1]
    return so


def threshold(lib, logits, top_k, p_q, scope):
    l = torch.from_numpy(np.ascontiguousarray(logits, dtype=np.float32))
    n, c = l.shape
    theta, kept = torch.full((n, ), 123.0), torch.full((n, ), -5, dtype=torch.int32)
    rc = lib.t2h_truncation_threshold(l.data_ptr(), n, c, int(top_k), int(p_q), scope, theta.data_ptr(), kept.data_ptr(), None)
    assert rc == 0, lib.emu_last_error()
    return theta.numpy(), kept.numpy()


def top_k_rows():
    rng = np.random.default_rng(11)
    rows = {
        'normal': (rng.standard_normal(N_CLASS) * 3).astype(np.float32),
        'heavy ties': np.round(rng.standard_normal(N_CLASS) * 2 * 4) / 4,            # logits rounded to 1/4
        'all equal': np.full(N_CLASS, 0.625),
        'negative': -np.abs(rng.standard_normal(N_CLASS) * 5) - 1,
        'mixed sign, tiny and huge': rng.standard_normal(N_CLASS) * np.exp(rng.uniform(-30, 30, N_CLASS)),
        'signed zeros': np.where(rng.random(N_CLASS) < 0.5, 0.0, -0.0) * 1.0,
        'zeros among values': np.where(rng.random(N_CLASS) < 0.3, -0.0, np.round(rng.standard_normal(N_CLASS) * 2)),
        'with -inf': np.where(rng.random(N_CLASS) < 0.1, -np.inf, rng.standard_normal(N_CLASS)),
    }
    rows['zeros among values'][::7] = 0.0
    return {k: np.asarray(v, dtype=np.float32) for k, v in rows.items()}


@pytest.mark.parametrize('scope', [0, 1])
def test_top_k_threshold_is_exact(lib, scope):
    rows = top_k_rows()
    logits = np.stack(list(rows.values()))
    for k in (1, 2, 63, 64, 65, 1023):
        theta, kept = threshold(lib, logits, k, 0, scope)
        for i, name in enumerate(rows):
            want_theta, keep = ref.kept_set(logits[i], top_k=k)
            assert theta[i].tobytes() == np.float32(want_theta).tobytes(), (name, k, theta[i], want_theta)
            assert kept[i] == keep.sum() and kept[i] >= k, (name, k, kept[i], keep.sum())
    theta, kept = threshold(lib, logits[:3], 5, 0, scope)
    assert kept[2] == N_CLASS                                    # all-equal logits: everything survives
    # both rules off, and the values that mean off at the C boundary: nothing is cut
    for k, p_q in ((0, 0), (N_CLASS, 0), (N_CLASS + 5, ref.P_ONE)):
        theta, kept = threshold(lib, logits[:2], k, p_q, scope)
        assert np.isneginf(theta).all() and (kept == N_CLASS).all()


def test_a_row_with_nans_selects_something_and_returns(lib):
    """definition 7: an ordinary input, run once -- no fault; nothing else is promised"""
    l = np.random.default_rng(5).standard_normal((2, N_CLASS)).astype(np.float32)
    l[0, ::3] = np.nan
    l[1, :] = np.nan
    for scope in (0, 1):
        theta, kept = threshold(lib, l, 10, ref.p_q_of(0.9), scope)
        assert ((kept >= 0) & (kept <= N_CLASS)).all()


def test_bad_settings_are_rejected_at_the_c_boundary(lib):
    l = torch.zeros(1, 8)
    out, kept = torch.zeros(1), torch.zeros(1, dtype=torch.int32)
    assert lib.t2h_truncation_threshold(l.data_ptr(), 1, 8, -1, 0, 0, out.data_ptr(), kept.data_ptr(), None) != 0
    assert lib.t2h_truncation_threshold(l.data_ptr(), 1, 8, 0, ref.P_ONE + 1, 0, out.data_ptr(), kept.data_ptr(), None) != 0
    assert lib.t2h_truncation_threshold(l.data_ptr(), 1, 8, 0, 0, 2, out.data_ptr(), kept.data_ptr(), None) != 0


@pytest.mark.parametrize('sigma', [0.5, 2.0, 5.0])
@pytest.mark.parametrize('p', [0.5, 0.9])
def test_top_p_set_lies_between_the_strict_and_the_permissive_oracle(lib, p, sigma):
    rng = np.random.default_rng(1000 + int(10 * sigma) + int(100 * p))
    logits = (rng.standard_normal((512, N_CLASS)) * sigma).astype(np.float32)
    p_q = ref.p_q_of(p)
    res = [threshold(lib, logits, 0, p_q, scope) for scope in (0, 1)]
    # the thread layout does not matter: integer equality between the scopes
    assert res[0][0].tobytes() == res[1][0].tobytes() and np.array_equal(res[0][1], res[1][1])
    theta, kept = res[0]
    decided = 0
    for i in range(logits.shape[0]):
        strict, perm = ref.top_p_sandwich(logits[i], p_q)
        got = logits[i] >= theta[i]
        assert got.sum() == kept[i] and kept[i] >= 1
        assert (strict <= got).all() and (got <= perm).all(), (i, strict.sum(), got.sum(), perm.sum())
        assert got[np.argmax(logits[i])]                          # the most probable class always survives
        decided += int(np.array_equal(strict, perm))
    # the sandwich is an equality on almost every row (a condition that keeps it from hiding a wrong kernel)
    assert decided >= 0.95 * logits.shape[0], decided


def test_top_k_and_top_p_together_are_top_p_on_the_top_k_survivors(lib):
    rng = np.random.default_rng(77)
    logits = (rng.standard_normal((24, N_CLASS)) * 2).astype(np.float32)
    logits[:8] = np.round(logits[:8] * 2) / 2                     # ties at the thresholds
    for k, p in ((64, 0.9), (8, 0.5), (300, 0.97)):
        p_q = ref.p_q_of(p)
        res = [threshold(lib, logits, k, p_q, scope) for scope in (0, 1)]
        assert res[0][0].tobytes() == res[1][0].tobytes() and np.array_equal(res[0][1], res[1][1])
        theta, kept = res[0]
        theta_k, kept_k = threshold(lib, logits, k, 0, 0)
        for i in range(logits.shape[0]):
            surv = logits[i] >= theta_k[i]
            strict, perm = ref.top_p_sandwich(logits[i], p_q, survivors=surv)
            got = logits[i] >= theta[i]
            assert theta[i] >= theta_k[i] and got.sum() == kept[i] <= kept_k[i]
            assert (strict <= got).all() and (got <= perm).all() and (got <= surv).all(), (k, p, i)


def test_integer_restatement_on_exponentials_that_are_exact(lib):
    """logits that are multiples of ln 2 would need an exact expf; instead: where every implementation of expf agrees
    (l - max in {0, -inf}), the integer definition is checked with equality -- G 2^20 < p_q S at the boundary."""
    l = np.full((3, N_CLASS), -np.inf, dtype=np.float32)
    l[0, [5, 9, 700]] = 1.5        # three equal classes: masses 2^32 each, G = 0 for all -> all three survive any p
    l[1, 3] = 2.0                  # one class
    l[2, :] = -3.25                # all equal: everything survives
    for p in (0.001, 0.5, 0.999):
        for scope in (0, 1):
            theta, kept = threshold(lib, l, 0, ref.p_q_of(p), scope)
            for i in range(3):
                e = np.exp(l[i] - l[i].max()).astype(np.float32)
                want_theta, keep = ref.kept_set(l[i], e, 0, ref.p_q_of(p))
                assert theta[i] == want_theta and kept[i] == keep.sum(), (p, scope, i)
    assert ref.masses(np.float32([1.0, 0.5, 0.0]))[:3] == [1 << 32, 1 << 31, 0]


# ---- the three pick sites

_libm = ctypes.CDLL('libm.so.6')
_libm.expf.restype, _libm.expf.argtypes = ctypes.c_float, [ctypes.c_float]


def scores_as_the_kernel(l, expo):
    """expf(l_j - max l) / E_j in fp32 with the C library's expf (what the emulated kernel calls)"""
    mx = np.float32(np.max(l))
    e = np.array([_libm.expf(float(np.float32(v) - mx)) for v in l], dtype=np.float32)
    return e / expo.astype(np.float32)


def _tail_problem(seed=31):
    n, C, n_class, n_heads, temp = 24, 512, 256, 2, 0.7
    g = torch.Generator().manual_seed(seed)
    hidden = torch.randn(n, C, generator=g) * 1.5 + 0.2
    gamma, beta = torch.randn(C, generator=g) * 0.2 + 1.0, torch.randn(C, generator=g) * 0.1
    w = torch.randn(n_heads, n_class, C, generator=g) * 0.12
    tex = torch.randint(0, n_heads, (n, ), generator=g)
    x_t = torch.full((n, ), MASK_ID)
    expo = torch.empty(n, n_class).exponential_(generator=g).contiguous()
    return dict(n=n, C=C, n_class=n_class, n_heads=n_heads, temp=temp, hidden=hidden, gamma=gamma, beta=beta, w=w, tex=tex,
                x_t=x_t, expo=expo)


def run_sample_heads(lib, pb, top_k, p_q, two_launch, set_fields=True):
    from text2human_amd._lib import SampleHeadsArgs
    n, n_class, n_heads = pb['n'], pb['n_class'], pb['n_heads']
    rows = torch.arange(n, dtype=torch.int32)
    b = SampleHeadsArgs()
    x2, out2 = pb['x_t'].clone(), torch.full((n_heads, n), -1, dtype=torch.int64)
    ws = torch.zeros(n, n_class)
    b.hidden, b.lnf_gamma, b.lnf_beta, b.w_heads = (pb['hidden'].data_ptr(), pb['gamma'].data_ptr(), pb['beta'].data_ptr(),
                                                    pb['w'].data_ptr())
    b.rows, b.tex, b.x_t, b.out_idx = rows.data_ptr(), pb['tex'].data_ptr(), x2.data_ptr(), out2.data_ptr()
    b.temp, b.n_rows, b.n, b.C, b.n_class, b.n_heads = pb['temp'], n, n, pb['C'], n_class, n_heads
    if two_launch:
        b.logits_ws = ws.data_ptr()
    for h in range(n_heads):
        b.expo[h] = pb['expo'].data_ptr()
    if set_fields:
        b.top_k, b.top_p_q = top_k, p_q
    assert lib.t2h_sample_heads(ctypes.byref(b), None) == 0, lib.emu_last_error()
    r = torch.arange(n)
    tok = out2[pb['tex'][r], r]
    assert torch.equal(x2, tok + n_class * pb['tex'])
    return tok.numpy(), ws.numpy()


def run_confidence_tail(lib, pb, top_k, p_q, set_fields=True):
    from text2human_amd._lib import ConfidenceTailArgs
    n, n_class, n_heads = pb['n'], pb['n_class'], pb['n_heads']
    a = ConfidenceTailArgs()
    gws = torch.full((int(lib.t2h_confidence_group_ws_ints(n, n_heads)), ), -1, dtype=torch.int32)
    lws = torch.full((n, n_class), float('nan'))
    tok, conf = torch.full((n, ), -9, dtype=torch.int32), torch.full((n, ), 7.0)
    a.hidden, a.lnf_gamma, a.lnf_beta, a.w_heads = (pb['hidden'].data_ptr(), pb['gamma'].data_ptr(), pb['beta'].data_ptr(),
                                                    pb['w'].data_ptr())
    a.tex, a.x_t, a.mask_id, a.temp = pb['tex'].data_ptr(), pb['x_t'].data_ptr(), MASK_ID, pb['temp']
    a.n, a.C, a.n_class, a.n_heads = n, pb['C'], n_class, n_heads
    a.expo = pb['expo'].data_ptr()
    a.group_ws, a.logits_ws, a.tok, a.conf = gws.data_ptr(), lws.data_ptr(), tok.data_ptr(), conf.data_ptr()
    if set_fields:
        a.top_k, a.top_p_q = top_k, p_q
    assert lib.t2h_confidence_tail(ctypes.byref(a), None) == 0, lib.emu_last_error()
    return tok.numpy().astype(np.int64), conf.numpy(), lws.numpy()


@pytest.fixture(scope='module')
def untruncated(lib):
    pb = _tail_problem()
    tok, ws = run_sample_heads(lib, pb, 0, 0, True, set_fields=False)
    tok_c, conf, _ = run_confidence_tail(lib, pb, 0, 0, set_fields=False)
    assert np.array_equal(tok, tok_c)
    return pb, tok, ws, conf


@pytest.mark.parametrize('top_k,p', [(8, None), (0, 0.5), (16, 0.9), (1, None)])
def test_all_pick_sites_draw_the_best_score_of_the_kept_set(lib, untruncated, top_k, p):
    pb, tok0, ws0, conf0 = untruncated
    p_q = ref.p_q_of(p) if p else 0
    tok2, ws = run_sample_heads(lib, pb, top_k, p_q, True)
    assert ws.tobytes() == ws0.tobytes()                          # truncation does not touch the logits
    theta, kept = threshold(lib, ws, top_k, p_q, 0)               # the kernel's own kept set, from the logits it left
    theta1, kept1 = threshold(lib, ws, top_k, p_q, 1)
    assert theta.tobytes() == theta1.tobytes() and np.array_equal(kept, kept1)
    expo = pb['expo'].numpy()
    changed = 0
    for i in range(pb['n']):
        keep = ws[i] >= theta[i]
        assert keep.sum() == kept[i]
        sc = np.where(keep, scores_as_the_kernel(ws[i], expo[i]), np.float32(-1.0))
        assert tok2[i] == int(np.argmax(sc)), (i, tok2[i], int(np.argmax(sc)))     # (argmax: first index wins)
        changed += int(tok2[i] != tok0[i])
    if top_k == 1:
        assert np.array_equal(tok2, ws.argmax(1))
    assert changed > 0                                            # the setting does something on this problem
    tok1, _ = run_sample_heads(lib, pb, top_k, p_q, False)        # one-launch form
    tok_c, conf, lws = run_confidence_tail(lib, pb, top_k, p_q)
    assert np.array_equal(tok1, tok2) and np.array_equal(tok_c, tok2)
    assert lws.tobytes() == ws.tobytes()
    # the confidence is the log-probability of the drawn token under the FULL softmax
    same = tok_c == tok0
    assert conf[same].tobytes() == conf0[same].tobytes()
    y = torch.nn.functional.layer_norm(pb['hidden'].double(), (pb['C'], ), pb['gamma'].double(), pb['beta'].double(), 1e-5)
    for i in np.nonzero(~same)[0]:
        logits = (pb['w'][int(pb['tex'][i])].double() @ y[i]) / pb['temp']
        want = float(torch.log_softmax(logits, 0)[int(tok_c[i])])
        assert abs(float(conf[i]) - want) < 2e-5, (i, float(conf[i]), want)


def test_off_is_off(lib, untruncated):
    pb, tok0, ws0, conf0 = untruncated
    for two in (True, False):
        for k, p_q in ((0, 0), (pb['n_class'], 0), (0, ref.P_ONE), (pb['n_class'] + 1, ref.P_ONE)):
            tok, _ = run_sample_heads(lib, pb, k, p_q, two)
            assert np.array_equal(tok, tok0)
    tok_c, conf, _ = run_confidence_tail(lib, pb, 0, 0)
    assert np.array_equal(tok_c, tok0) and conf.tobytes() == conf0.tobytes()
    # the Python helper never passes the "off" spellings down
    from text2human_amd import ops
    assert ops.truncation_settings(pb['n_class'], 1.0, pb['n_class']) == (0, 0)
    assert ops.truncation_settings(None, None, 1024) == (0, 0) and ops.truncation_settings(0, None) == (0, 0)
    assert ops.truncation_settings(64, 0.9, 1024) == (64, ref.p_q_of(0.9))
    with pytest.raises(ValueError, match='-3'):
        ops.truncation_settings(-3, None)
    with pytest.raises(ValueError, match='1e-09'):
        ops.truncation_settings(None, 1e-9)


def test_a_nan_row_gets_a_token_inside_the_table(lib):
    pb = _tail_problem(seed=32)
    pb['hidden'][3, 7] = float('nan')
    for two in (True, False):
        tok, _ = run_sample_heads(lib, pb, 8, ref.p_q_of(0.9), two)
        assert ((tok >= 0) & (tok < pb['n_class'])).all()
    tok_c, _, _ = run_confidence_tail(lib, pb, 8, ref.p_q_of(0.9))
    assert ((tok_c >= 0) & (tok_c < pb['n_class'])).all()
