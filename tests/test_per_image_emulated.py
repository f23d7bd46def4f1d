"""Per-image sampling controls on the CPU ("Per-image sampling controls"): the *_per_sample entry points of
csrc/sampler.hip through tests/emu, the host helper that validates the public arguments, and the per-image confidence
schedules.

The property: image b of a batch drawn with a table is, as bits, image b of the scalar entry point called with
params[b] on the same inputs -- logits, thresholds, tokens, confidences, scores and committed rows.  The numpy
restatement (tests/per_image_ref.py) pins what the scalar entry point is not asked twice for: the top-k thresholds and
the committed sets."""
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
import per_image_ref as ref  # noqa: E402
import truncation_ref as TR  # noqa: E402
from test_truncation_emulated import run_confidence_tail, run_sample_heads, threshold  # noqa: E402

needs_emu = pytest.mark.skipif(not build_emu.available(), reason='no host clang++ for the emulation build')

MASK_ID = 18432
B, T = 3, 4
# image 0: the defaults inside a truncating launch; 1: colder, top-k; 2: warmer, top-p
SETS = ref.settings(temp=(1.0, 0.7, 1.3), top_k=(None, 5, None), top_p=(None, None, 0.6))
SETS_BOTH = ref.settings(temp=(0.9, 0.9, 2.0), top_k=(3, 64, 7), top_p=(0.5, 1.0, 0.8))   # (64 = n_class: off)


@pytest.fixture(scope='module')
def lib():
    from text2human_amd import _lib
    so = build_emu.load('sampler.hip')
    for name in ('t2h_sample_heads_per_sample', 't2h_confidence_tail_per_sample', 't2h_confidence_commit_per_sample',
                 't2h_truncation_threshold_per_row'):
        assert getattr(so, name).argtypes == _lib.SIGNATURES[name][1]
    return so


def _problem(seed=41, n_class=64):
    """3 images of 4 rows, the smallest shapes the tails are built for (C = 512 is the only hidden size)"""
    n, C, n_heads = B * T, 512, 2
    g = torch.Generator().manual_seed(seed)
    hidden = torch.randn(n, C, generator=g) * 1.5 + 0.2
    gamma, beta = torch.randn(C, generator=g) * 0.2 + 1.0, torch.randn(C, generator=g) * 0.1
    w = torch.randn(n_heads, n_class, C, generator=g) * 0.12
    tex = torch.randint(0, n_heads, (n, ), generator=g)
    expo = torch.empty(n, n_class).exponential_(generator=g).contiguous()
    return dict(n=n, C=C, n_class=n_class, n_heads=n_heads, temp=1.0, hidden=hidden, gamma=gamma, beta=beta, w=w, tex=tex,
                x_t=torch.full((n, ), MASK_ID), expo=expo)


def _with(pb, temp):
    return dict(pb, temp=temp)


def heads_per_sample(lib, pb, sets, two_launch):
    from text2human_amd._lib import SampleHeadsArgs
    n, n_class, n_heads = pb['n'], pb['n_class'], pb['n_heads']
    rows = torch.arange(n, dtype=torch.int32)
    tbl = torch.from_numpy(ref.table(sets))
    a = SampleHeadsArgs()
    x2, out2 = pb['x_t'].clone(), torch.full((n_heads, n), -1, dtype=torch.int64)
    ws = torch.zeros(n, n_class)
    a.hidden, a.lnf_gamma, a.lnf_beta, a.w_heads = (pb['hidden'].data_ptr(), pb['gamma'].data_ptr(), pb['beta'].data_ptr(),
                                                    pb['w'].data_ptr())
    a.rows, a.tex, a.x_t, a.out_idx = rows.data_ptr(), pb['tex'].data_ptr(), x2.data_ptr(), out2.data_ptr()
    a.temp, a.n_rows, a.n, a.C, a.n_class, a.n_heads = -1.0, n, n, pb['C'], n_class, n_heads   # (temp is not read)
    a.top_k, a.top_p_q = 1, 1                                                                   # (nor are these)
    if two_launch:
        a.logits_ws = ws.data_ptr()
    for h in range(n_heads):
        a.expo[h] = pb['expo'].data_ptr()
    assert lib.t2h_sample_heads_per_sample(ctypes.byref(a), tbl.data_ptr(), T, None) == 0, lib.emu_last_error()
    r = torch.arange(n)
    tok = out2[pb['tex'][r], r]
    assert torch.equal(x2, tok + n_class * pb['tex'])
    return tok.numpy(), ws.numpy()


def tail_per_sample(lib, pb, sets):
    from text2human_amd._lib import ConfidenceTailArgs
    n, n_class, n_heads = pb['n'], pb['n_class'], pb['n_heads']
    tbl = torch.from_numpy(ref.table(sets))
    a = ConfidenceTailArgs()
    gws = torch.full((int(lib.t2h_confidence_group_ws_ints(n, n_heads)), ), -1, dtype=torch.int32)
    lws = torch.full((n, n_class), float('nan'))
    tok, conf = torch.full((n, ), -9, dtype=torch.int32), torch.full((n, ), 7.0)
    a.hidden, a.lnf_gamma, a.lnf_beta, a.w_heads = (pb['hidden'].data_ptr(), pb['gamma'].data_ptr(), pb['beta'].data_ptr(),
                                                    pb['w'].data_ptr())
    a.tex, a.x_t, a.mask_id, a.temp = pb['tex'].data_ptr(), pb['x_t'].data_ptr(), MASK_ID, -1.0
    a.n, a.C, a.n_class, a.n_heads = n, pb['C'], n_class, n_heads
    a.expo = pb['expo'].data_ptr()
    a.group_ws, a.logits_ws, a.tok, a.conf = gws.data_ptr(), lws.data_ptr(), tok.data_ptr(), conf.data_ptr()
    assert lib.t2h_confidence_tail_per_sample(ctypes.byref(a), tbl.data_ptr(), T, None) == 0, lib.emu_last_error()
    return tok.numpy().astype(np.int64), conf.numpy(), lws.numpy()


@needs_emu
@pytest.mark.parametrize('sets', [SETS, SETS_BOTH], ids=['mixed', 'both rules'])
def test_every_image_of_a_mixed_batch_is_the_scalar_launch_with_its_own_settings(lib, sets):
    pb = _problem()
    tok2, ws2 = heads_per_sample(lib, pb, sets, True)
    tok1, _ = heads_per_sample(lib, pb, sets, False)             # the one-launch form
    tok_c, conf_c, lws_c = tail_per_sample(lib, pb, sets)
    assert np.array_equal(tok1, tok2) and np.array_equal(tok_c, tok2) and lws_c.tobytes() == ws2.tobytes()
    differs, prev = 0, None
    for b, (temp, k, p_q) in enumerate(sets):
        sl = slice(b * T, (b + 1) * T)
        off = (k == 0 or k >= pb['n_class']) and p_q in (0, TR.P_ONE)
        # an image whose rules cut nothing is compared with the instance that has no truncation code at all
        want_tok, want_ws = run_sample_heads(lib, _with(pb, temp), k, p_q, True, set_fields=not off)
        want_c, want_conf, want_lws = run_confidence_tail(lib, _with(pb, temp), k, p_q, set_fields=not off)
        assert ws2[sl].tobytes() == want_ws[sl].tobytes() == want_lws[sl].tobytes(), b          # logits / temp[b], as bits
        assert np.array_equal(tok2[sl], want_tok[sl]), b
        assert np.array_equal(tok_c[sl], want_c[sl]) and conf_c[sl].tobytes() == want_conf[sl].tobytes(), b
        if b:   # ... and the neighbour's settings would have given other bits: the table is read per image
            differs += int(not np.array_equal(prev[0][sl], tok2[sl]) or prev[1][sl].tobytes() != ws2[sl].tobytes())
        prev = (want_tok, want_ws)
    assert differs == B - 1


@needs_emu
@pytest.mark.parametrize('scope', [0, 1])
def test_row_thresholds_follow_the_rows_image(lib, scope):
    n_class = 256
    rng = np.random.default_rng(8)
    logits = (rng.standard_normal((B * T, n_class)) * 2.5).astype(np.float32)
    logits[::3] = np.round(logits[::3] * 2) / 2                                                 # ties at the thresholds
    sets = ref.settings(temp=(1.0, 1.0, 1.0), top_k=(None, 5, 40), top_p=(None, None, 0.7))
    l = torch.from_numpy(logits)
    tbl = torch.from_numpy(ref.table(sets))
    theta, kept = torch.full((B * T, ), 123.0), torch.full((B * T, ), -5, dtype=torch.int32)
    rc = lib.t2h_truncation_threshold_per_row(l.data_ptr(), B * T, n_class, tbl.data_ptr(), T, scope, theta.data_ptr(),
                                              kept.data_ptr(), None)
    assert rc == 0, lib.emu_last_error()
    theta, kept = theta.numpy(), kept.numpy()
    for b, (_, k, p_q) in enumerate(sets):
        sl = slice(b * T, (b + 1) * T)
        want_theta, want_kept = threshold(lib, logits, k, p_q, scope)                           # the scalar entry point
        assert theta[sl].tobytes() == want_theta[sl].tobytes() and np.array_equal(kept[sl], want_kept[sl]), b
    # numpy: the top-k rule alone is exact (images 0 and 1); with top-p on top the threshold can only rise
    k_theta, k_kept = ref.top_k_thresholds(logits, sets, T)
    assert theta[:2 * T].tobytes() == k_theta[:2 * T].tobytes() and np.array_equal(kept[:2 * T], k_kept[:2 * T])
    assert np.isneginf(theta[:T]).all() and (kept[:T] == n_class).all()                          # nothing is cut
    assert (theta[2 * T:] >= k_theta[2 * T:]).all() and (kept[2 * T:] <= k_kept[2 * T:]).all() and (kept[2 * T:] >= 1).all()
    for r in range(2 * T, 3 * T):                                                               # top-p on the top-40 survivors
        strict, perm = TR.top_p_sandwich(logits[r], sets[2][2], survivors=logits[r] >= k_theta[r])
        got = logits[r] >= theta[r]
        assert (strict <= got).all() and (got <= perm).all(), r


def _commit(lib, entry, conf, tok, tex, x_t, out, k, tau, u):
    from text2human_amd._lib import ConfidenceCommitArgs
    nb, t = x_t.shape
    a = ConfidenceCommitArgs()
    kk, tt = torch.tensor(k, dtype=torch.int32), torch.tensor(tau, dtype=torch.float32)
    scores = torch.full((nb * t, ), 123.0)
    a.conf, a.tok, a.tex, a.u = conf.data_ptr(), tok.data_ptr(), tex.data_ptr(), u.data_ptr()
    a.k, a.tau, a.mask_id, a.x_t, a.out = kk.data_ptr(), tt.data_ptr(), MASK_ID, x_t.data_ptr(), out.data_ptr()
    a.scores = scores.data_ptr()
    a.B, a.T, a.n_heads, a.n_class = nb, t, out.shape[0], 1024
    assert getattr(lib, entry)(ctypes.byref(a), None) == 0, lib.emu_last_error()
    return scores.view(nb, t)


@needs_emu
def test_commit_scores_every_image_with_its_own_choice_temperature(lib):
    from test_confidence_emulated import _state
    t_len, H = 96, 4
    g, tex, tok, masked, x_t, out = _state(B, t_len, H, seed=9, masked_frac=0.7)
    conf = (-torch.rand(B, t_len, generator=g) * 9).contiguous()
    u = torch.rand(B * t_len, generator=g).contiguous()
    k, tau = [7, 20, 0], [0.0, 4.5, 2.0]
    xt, o = x_t.clone(), out.clone()
    scores = _commit(lib, 't2h_confidence_commit_per_sample', conf, tok, tex, xt, o, k, tau, u)
    changed = (xt != x_t)
    for b in range(B):
        xs, os_ = x_t.clone(), out.clone()
        want = _commit(lib, 't2h_confidence_commit', conf, tok, tex, xs, os_, k, [tau[b]], u)  # the scalar entry, tau[b]
        cols = slice(b * t_len, (b + 1) * t_len)
        assert scores[b].numpy().tobytes() == want[b].numpy().tobytes(), b
        assert torch.equal(xt[b], xs[b]) and torch.equal(o[:, cols], os_[:, cols]), b
    # numpy: the committed rows are the k[b] best of the kernel's own scores; tau = 0 leaves the confidence itself
    sets = ref.committed_rows(scores.numpy(), masked.numpy(), k)
    m = masked.numpy()
    assert [set(np.nonzero(changed[b].numpy())[0].tolist()) for b in range(B)] == sets
    assert [len(s) for s in sets] == [7, 20, 0]
    assert np.array_equal(scores[0].numpy()[m[0]], conf[0].numpy()[m[0]])
    assert not np.array_equal(scores[2].numpy()[m[2]], conf[2].numpy()[m[2]])


@needs_emu
def test_the_table_is_required_and_must_fit_the_batch(lib):
    pb = _problem()
    from text2human_amd._lib import ConfidenceTailArgs, SampleHeadsArgs
    tbl = torch.from_numpy(ref.table(SETS))
    assert lib.t2h_sample_heads_per_sample(ctypes.byref(SampleHeadsArgs()), None, T, None) != 0
    assert lib.t2h_confidence_tail_per_sample(ctypes.byref(ConfidenceTailArgs()), None, T, None) != 0
    l, th, kp = torch.zeros(B * T, 8), torch.zeros(B * T), torch.zeros(B * T, dtype=torch.int32)
    args = (l.data_ptr(), B * T, 8, tbl.data_ptr())
    assert lib.t2h_truncation_threshold_per_row(*args, T, 0, th.data_ptr(), kp.data_ptr(), None) == 0
    assert lib.t2h_truncation_threshold_per_row(*args, 5, 0, th.data_ptr(), kp.data_ptr(), None) != 0   # 5 does not divide 24
    assert lib.t2h_truncation_threshold_per_row(*args, 0, 0, th.data_ptr(), kp.data_ptr(), None) != 0
    assert lib.t2h_truncation_threshold_per_row(l.data_ptr(), B * T, 8, None, T, 0, th.data_ptr(), kp.data_ptr(), None) != 0
    assert pb['n'] == B * T


# ---- the host side: validation and the per-image schedules (no emulator)

def test_scalars_stay_scalars_and_sequences_become_a_table():
    from text2human_amd import ops, options
    sp = ops.sampling_params(3, 0.8, 7, None, 1024)
    assert sp.table is None and sp.temp == 0.8 and sp.trunc == ops.truncation_settings(7, None, 1024) == (7, 0)
    assert ops.sampling_params(3).trunc == (0, 0)
    for seq in ([1.0, 0.7, 1.3], (1.0, 0.7, 1.3), np.array([1.0, 0.7, 1.3]), torch.tensor([1.0, 0.7, 1.3])):
        sp = ops.sampling_params(3, seq, [None, 5, None], [None, None, 0.6], 1024)
        assert sp.temp is None and sp.trunc is None and sp.table.dtype == ops.SAMPLE_PARAMS_DTYPE
        assert sp.table['temp'].tolist() == [np.float32(v) for v in (1.0, 0.7, 1.3)]
        assert sp.table['top_k'].tolist() == [0, 5, 0] and sp.table['top_p_q'].tolist() == [0, 0, TR.p_q_of(0.6)]
        assert np.array_equal(ops.sample_params_tensor(sp.table, 'cpu').numpy(), ref.table(SETS))
    # a uniform sequence is not collapsed; one sequence is enough; off spellings are normalised per image
    sp = ops.sampling_params(3, [0.8] * 3, 7, None, 1024)
    assert sp.table is not None and sp.table['top_k'].tolist() == [7, 7, 7]
    sp = ops.sampling_params(2, 1.0, [1024, 2000], [1.0, None], 1024)
    assert sp.table['top_k'].tolist() == [0, 0] and sp.table['top_p_q'].tolist() == [0, 0]
    assert ops.sampling_params(2, 1.0, None, None, 1024, per_image=True).table['temp'].tolist() == [1.0, 1.0]
    assert options.per_image_values(2, 3.0, 'x') is None and options.per_image_values(2, np.float32(3.0), 'x') is None
    assert options.per_image_values(2, np.array([3, 4]), 'x') == [3, 4] and not options.is_per_image(None)


BAD = [
    (dict(temp=[1.0, 0.7]), 'temp', '2 entries'),
    (dict(top_k=[5, 5, 5, 5]), 'top_k', '4 entries'),
    (dict(top_p=np.ones((3, 1))), 'top_p', '1-D'),
    (dict(temp=[1.0, 0.0, 1.0]), 'image 1', 'temp'),
    (dict(temp=[1.0, 1.0, -2.0]), 'image 2', 'temp'),
    (dict(temp=[float('nan'), 1.0, 1.0]), 'image 0', 'temp'),
    (dict(temp=[1.0, None, 1.0]), 'image 1', 'temp'),
    (dict(top_k=[None, -1, 3]), 'image 1', 'top_k'),
    (dict(top_k=[None, 2, 3.5]), 'image 2', 'top_k'),
    (dict(top_p=[None, 0.5, 0.0]), 'image 2', 'top_p'),
    (dict(top_p=[1.5, 0.5, 0.5]), 'image 0', 'top_p'),
    (dict(top_p=[0.5, 1e-9, 0.5]), 'image 1', 'too small'),
]


class _NetStub:
    """what _begin_run reads before anything is launched"""
    name, split, x8 = 'tf', False, False
    P = {'tf.heads': torch.empty(18, 1024, 1)}


@pytest.mark.parametrize('kw,who,what', BAD, ids=[f'{list(k)[0]}-{w}' for k, w, _ in BAD])
def test_bad_per_image_values_raise_a_value_error_that_names_the_image(kw, who, what):
    from text2human_amd import engine, ops
    with pytest.raises(ValueError, match=who) as e:
        ops.sampling_params(3, **kw, n_class=1024)
    assert what in str(e.value)
    # ... from both loops, first thing: no generator has moved, nothing has been launched (there is no device here)
    segm = tex = torch.zeros(3, 512, dtype=torch.int64)
    state = torch.get_rng_state()
    for call in (lambda: engine.sample_tokens(_NetStub(), segm, tex, 16, MASK_ID, **kw),
                 lambda: engine.sample_tokens_confidence(_NetStub(), segm, tex, MASK_ID, rounds=4, **kw)):
        with pytest.raises(ValueError, match=who):
            call()
    assert torch.equal(torch.get_rng_state(), state)


@pytest.mark.parametrize('kw,who', [(dict(rounds=[4, 0, 6]), 'image 1: rounds'), (dict(rounds=[4, 8]), 'rounds: one entry'),
                                    (dict(rounds=[4, 8, 2.5]), 'image 2: rounds'),
                                    (dict(rounds=4, choice_temp=[0.0, 4.5, -1.0]), 'image 2: choice_temp'),
                                    (dict(rounds=[4, 8, 6], choice_temp=[0.0, float('nan'), 1.0]), 'image 1: choice_temp'),
                                    (dict(rounds=4, choice_temp=[1.0]), 'choice_temp: one entry')])
def test_bad_per_image_rounds_and_choice_temperatures(kw, who):
    from text2human_amd import engine
    segm = tex = torch.zeros(3, 512, dtype=torch.int64)
    with pytest.raises(ValueError, match=who):
        engine.sample_tokens_confidence(_NetStub(), segm, tex, MASK_ID, **kw)


def test_per_image_confidence_tables():
    from text2human_amd import schedule
    m0, rounds, ct = (512, 0, 137), (3, 8, 5), (0.0, 4.5, 2.0)
    k, tau = schedule.confidence_tables(m0, rounds, ct)
    assert k.shape == tau.shape == (8, 3) and k.dtype == np.int32 and tau.dtype == np.float32
    want_k, want_tau = ref.confidence_tables(m0, rounds, ct)
    assert np.array_equal(k, want_k) and tau.tobytes() == want_tau.tobytes()
    for b in range(3):
        own = schedule.confidence_schedule(m0[b], rounds[b])[1]
        assert np.array_equal(k[:rounds[b], b], own) and not k[rounds[b]:, b].any() and k[:, b].sum() == m0[b]
        assert tau[:rounds[b], b].tobytes() == schedule.confidence_choice_temps(rounds[b], ct[b]).tobytes()
        assert not tau[rounds[b]:, b].any() and tau[rounds[b] - 1, b] == 0.0                 # the last round is greedy
    assert not k[:, 1].any()                                                                  # a fully kept image
    assert tau[0, 1] == np.float32(4.5 * (1 - 1 / 8)) and tau[0, 2] == np.float32(2.0 * (1 - 1 / 5))
    # the tables the loop walks are at least two columns wide (the offsets' channel), whatever the batch
    k1, tau1 = schedule.confidence_tables((512, ), (4, ), (1.0, ))
    assert k1.shape == (4, 2) and not k1[:, 1].any() and not tau1[:, 1].any()
    with pytest.raises(ValueError):
        schedule.confidence_tables((512, 512), (4, ), (1.0, 1.0))
