"""The two kernels of confidence-ordered decoding on the CPU (csrc/sampler.hip through tests/emu; DESIGN.md,
"Confidence-ordered decoding").  Commit (t2h_confidence_commit): exact equality with a numpy restatement -- a stable
descending sort of the masked rows' scores, NaN last -- on random scores, scores with exact ties, NaNs, and
k in {0, 1, M - 1, M}.  Tail (t2h_confidence_tail): the token t2h_sample_heads draws on the same noise, and the
confidence against float64."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'emu'))
import build_emu  # noqa: E402
from test_sampler_emulated import raw_words, uniform_of  # noqa: E402

pytestmark = pytest.mark.skipif(not build_emu.available(), reason='no host clang++ for the emulation build')

MASK_ID = 18432


@pytest.fixture(scope='module')
def lib():
    from text2human_amd import _lib
    so = build_emu.load('sampler.hip')
    assert so.t2h_confidence_commit.argtypes == _lib.SIGNATURES['t2h_confidence_commit'][1]
    return so


def commit_restated(scores, masked, k, tok, tex, x_t, out, n_class):
    """Per sample: the k masked rows with the largest score, equal scores in row order, NaN below every number."""
    B, T = x_t.shape
    x_t, out = x_t.copy(), out.copy()
    for b in range(B):
        rows = np.nonzero(masked[b])[0]
        s = scores[b][rows].astype(np.float64)
        key = np.where(np.isnan(s), -np.inf, s)
        nan = np.isnan(s).astype(np.int64)
        order = np.lexsort((rows, -key, nan))          # NaN last, then descending score, then ascending row
        for i in rows[order][:max(int(k[b]), 0)]:
            x_t[b, i] = tok[b, i] + n_class * tex[b, i]
            out[tex[b, i], b * T + i] = tok[b, i]
    return x_t, out


def run_commit(lib, conf, tok, tex, x_t, out, k, tau=0.0, u=None, philox=None, want_scores=False):
    from text2human_amd._lib import ConfidenceCommitArgs
    B, T = x_t.shape
    n_heads = out.shape[0]
    a = ConfidenceCommitArgs()
    kk, tt = torch.tensor(k, dtype=torch.int32), torch.tensor([tau], dtype=torch.float32)
    scores = torch.full((B * T, ), 123.0)
    a.conf, a.tok, a.tex = conf.data_ptr(), tok.data_ptr(), tex.data_ptr()
    if philox is not None:
        a.philox_seed, a.philox_offset, a.philox_grid_threads = philox
    else:
        u = u if u is not None else torch.full((B * T, ), 0.5)
        a.u = u.data_ptr()
    a.k, a.tau, a.mask_id, a.x_t, a.out = kk.data_ptr(), tt.data_ptr(), MASK_ID, x_t.data_ptr(), out.data_ptr()
    a.scores = scores.data_ptr()
    a.B, a.T, a.n_heads, a.n_class = B, T, n_heads, 1024
    assert lib.t2h_confidence_commit(ctypes.byref(a), None) == 0, lib.emu_last_error()
    return scores.view(B, T)


def _state(B, T, n_heads, seed, masked_frac):
    g = torch.Generator().manual_seed(seed)
    tex = torch.randint(0, n_heads, (B, T), generator=g)
    tok = torch.randint(0, 1024, (B, T), generator=g).to(torch.int32)
    masked = torch.rand(B, T, generator=g) < masked_frac
    old = torch.randint(0, 1024, (B, T), generator=g)
    x_t = torch.where(masked, torch.full_like(old, MASK_ID), old + 1024 * tex)
    out = torch.full((n_heads, B * T), -1, dtype=torch.int64)
    idx = torch.arange(B * T)[~masked.view(-1)]
    out[tex.view(-1)[idx], idx] = old.view(-1)[idx]
    tok = torch.where(masked, tok, torch.full_like(tok, -1))   # what the tail writes for rows that are not masked
    return g, tex, tok, masked, x_t, out


@pytest.mark.parametrize('kind', ['random', 'ties', 'nan'])
def test_commit_is_a_stable_descending_top_k(lib, kind):
    B, T, H = 3, 512, 18
    g, tex, tok, masked, x_t, out = _state(B, T, H, seed={'random': 1, 'ties': 2, 'nan': 3}[kind], masked_frac=0.6)
    conf = -torch.rand(B, T, generator=g) * 9
    if kind == 'ties':
        conf = -(torch.randint(0, 6, (B, T), generator=g).float())     # six distinct values: ties everywhere
    if kind == 'nan':
        conf[torch.rand(B, T, generator=g) < 0.2] = float('nan')
        conf[0, 5], conf[0, 9] = float('-inf'), float('inf')
    conf = conf.contiguous()
    M = masked.sum(1).tolist()
    for ks in ([0, 1, M[2] - 1], [M[0], M[1] - 1, 1], [17, M[1], M[2]], [M[0] + 5, 40, 0]):
        xt, o = x_t.clone(), out.clone()
        scores = run_commit(lib, conf, tok, tex, xt, o, ks)
        m_np = masked.numpy()
        # tau = 0: the score IS the confidence; rows that are not masked report -inf
        got_s = scores.numpy()
        assert np.array_equal(got_s[m_np], conf.numpy()[m_np], equal_nan=True) and np.isneginf(got_s[~m_np]).all()
        want_x, want_o = commit_restated(conf.numpy(), m_np, ks, tok.numpy(), tex.numpy(), x_t.numpy(), out.numpy(), 1024)
        assert np.array_equal(xt.numpy(), want_x) and np.array_equal(o.numpy(), want_o), (kind, ks)
        changed = (xt != x_t).sum(1).tolist()
        assert changed == [min(k, m) for k, m in zip(ks, M)]                # exactly k rows per sample
        assert torch.equal(xt[~masked], x_t[~masked])                       # rows that were not masked never move


def test_commit_scores_are_confidence_plus_scaled_gumbel(lib):
    B, T, H, tau = 2, 512, 18, 2.25
    g, tex, tok, masked, x_t, out = _state(B, T, H, seed=4, masked_frac=0.8)
    conf = (-torch.rand(B, T, generator=g) * 9).contiguous()
    seed, off, grid = 2021, 4 * 300, 256 * 4
    u = uniform_of(raw_words(seed, off, grid, B * T))
    u[3] = 0.0                                                              # torch.rand's range is [0, 1): clamped
    uc = np.clip(u.astype(np.float64), 2.0**-24, 1 - 2.0**-24)
    want = conf.numpy().reshape(-1).astype(np.float64) + tau * -np.log(-np.log(uc))
    for kw in (dict(u=torch.from_numpy(u.copy())), dict(philox=(seed, off, grid))):
        xt, o = x_t.clone(), out.clone()
        s = run_commit(lib, conf, tok, tex, xt, o, [50, 60], tau=tau, **kw).numpy().reshape(-1)
        m = masked.numpy().reshape(-1)
        if 'philox' in kw:
            m = m & (np.arange(B * T) != 3)                                 # (element 3 was edited in the explicit draw)
        assert np.abs(s[m] - want[m]).max() < 2e-5 * np.abs(want[m]).max()
        # and the commit is the top-k of the kernel's OWN scores, exactly
        want_x, want_o = commit_restated(s.reshape(B, T), masked.numpy(), [50, 60], tok.numpy(), tex.numpy(),
                                         x_t.numpy(), out.numpy(), 1024)
        assert np.array_equal(xt.numpy(), want_x) and np.array_equal(o.numpy(), want_o)


def test_tail_draws_the_token_of_the_existing_tail_with_its_log_probability(lib):
    from text2human_amd._lib import ConfidenceTailArgs, SampleHeadsArgs
    n, C, n_class, n_heads, temp = 48, 512, 64, 3, 0.7
    g = torch.Generator().manual_seed(21)
    hidden = torch.randn(n, C, generator=g) * 1.5 + 0.2
    gamma, beta = torch.randn(C, generator=g) * 0.2 + 1.0, torch.randn(C, generator=g) * 0.1
    w = torch.randn(n_heads, n_class, C, generator=g) * 0.08
    tex = torch.randint(0, n_heads, (n, ), generator=g)
    tex[:20] = 1                                             # one head with more rows than a tile holds (16)
    masked = torch.rand(n, generator=g) < 0.7
    masked[:20] = True
    x_t = torch.where(masked, torch.full((n, ), MASK_ID), torch.randint(0, n_class, (n, ), generator=g) + n_class * tex)
    expo = torch.empty(n, n_class).exponential_(generator=g).contiguous()

    a = ConfidenceTailArgs()
    ws_ints = int(lib.t2h_confidence_group_ws_ints(n, n_heads))
    assert ws_ints == 4 + 3 * ((n + 15) // 16 + n_heads) + n
    gws = torch.full((ws_ints, ), -1, dtype=torch.int32)
    lws = torch.full((n, n_class), float('nan'))
    tok, conf = torch.full((n, ), -9, dtype=torch.int32), torch.full((n, ), 7.0)
    a.hidden, a.lnf_gamma, a.lnf_beta, a.w_heads = hidden.data_ptr(), gamma.data_ptr(), beta.data_ptr(), w.data_ptr()
    a.tex, a.x_t, a.mask_id, a.temp = tex.data_ptr(), x_t.data_ptr(), MASK_ID, temp
    a.n, a.C, a.n_class, a.n_heads = n, C, n_class, n_heads
    a.expo = expo.data_ptr()
    a.group_ws, a.logits_ws, a.tok, a.conf = gws.data_ptr(), lws.data_ptr(), tok.data_ptr(), conf.data_ptr()
    x_before = x_t.clone()
    assert lib.t2h_confidence_tail(ctypes.byref(a), None) == 0, lib.emu_last_error()
    assert torch.equal(x_t, x_before)                        # the tail decides nothing
    rows = torch.nonzero(masked).view(-1).to(torch.int32)
    assert int(gws[1]) == len(rows)
    listed = gws[4 + 3 * ((n + 15) // 16 + n_heads):][:len(rows)]
    assert sorted(listed.tolist()) == rows.tolist()          # every masked row in exactly one tile
    assert (tok[~masked] == -1).all() and torch.isneginf(conf[~masked]).all()

    # the existing tail (two-launch form) on the same rows and noise
    b = SampleHeadsArgs()
    x2 = x_t.clone()
    out2 = torch.full((n_heads, n), -1, dtype=torch.int64)
    ws2 = torch.zeros(len(rows), n_class)
    b.hidden, b.lnf_gamma, b.lnf_beta, b.w_heads = hidden.data_ptr(), gamma.data_ptr(), beta.data_ptr(), w.data_ptr()
    b.rows, b.tex, b.x_t, b.out_idx = rows.data_ptr(), tex.data_ptr(), x2.data_ptr(), out2.data_ptr()
    b.temp, b.n_rows, b.n, b.C, b.n_class, b.n_heads = temp, len(rows), n, C, n_class, n_heads
    b.logits_ws = ws2.data_ptr()
    for h in range(n_heads):
        b.expo[h] = expo.data_ptr()
    assert lib.t2h_sample_heads(ctypes.byref(b), None) == 0, lib.emu_last_error()
    r = rows.long()
    assert torch.equal(out2[tex[r], r], tok[r].long())       # integer equality
    assert torch.equal(lws[r], ws2)                          # the same logits, bit for bit

    y = torch.nn.functional.layer_norm(hidden.double(), (C, ), gamma.double(), beta.double(), 1e-5)
    for i in r.tolist():
        logits = (w[int(tex[i])].double() @ y[i]) / temp
        want = torch.log_softmax(logits, 0)[int(tok[i])]
        assert abs(float(conf[i]) - float(want)) < 2e-5, (i, float(conf[i]), float(want))
