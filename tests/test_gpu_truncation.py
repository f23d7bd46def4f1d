"""Truncated sampling (top-k / top-p) on the GPU (-m gpu; DESIGN.md, "Truncated sampling"): the row-threshold selection
against the restatement of tests/truncation_ref.py at both scopes, the pick kernels on explicit and in-kernel draws,
and the public calls -- every sampled token inside its row's kept set, graph replay / shrinking batch, generator
offsets, editing.  Synthetic checkpoints: nothing here says anything about image quality."""
import numpy as np
import pytest
import torch

import truncation_ref as ref
from test_truncation_emulated import top_k_rows
from text2human_amd import defaults, engine, ops, options, synthetic
from text2human_amd.models import SampleFromParsingModel

from parity_util import ACT_TOL, seed_all  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda'
MASK_ID = 18432
SETTINGS = [dict(top_k=64), dict(top_p=0.9), dict(top_k=64, top_p=0.9)]


@pytest.fixture(scope='module')
def opt():
    return options.dict_to_nonedict(defaults.sample_from_parsing())


@pytest.fixture(scope='module')
def model(opt):
    return SampleFromParsingModel(opt, state_dicts=synthetic.make_state_dicts(opt, seed=1234))


def _gen():
    return torch.cuda.default_generators[torch.cuda.current_device()]


def _threshold(logits, top_k, top_p, scope):
    theta, kept = ops.truncation_threshold(torch.from_numpy(np.ascontiguousarray(logits)).to(DEV), top_k, top_p, scope)
    return theta.cpu().numpy(), kept.cpu().numpy()


@pytest.mark.parametrize('scope', [0, 1])
def test_top_k_threshold_is_exact_on_the_device(scope):
    rows = top_k_rows()
    logits = np.stack(list(rows.values()))
    for k in (1, 2, 63, 64, 65, 1023):
        theta, kept = _threshold(logits, k, None, scope)
        for i, name in enumerate(rows):
            want_theta, keep = ref.kept_set(logits[i], top_k=k)
            assert theta[i].tobytes() == np.float32(want_theta).tobytes(), (name, k, theta[i], want_theta)
            assert kept[i] == keep.sum(), (name, k)
    theta, kept = _threshold(logits, 1024, 1.0, scope)
    assert np.isneginf(theta).all() and (kept == 1024).all()


@pytest.mark.parametrize('sigma', [0.5, 2.0, 5.0])
@pytest.mark.parametrize('p', [0.5, 0.9])
def test_top_p_set_lies_between_the_strict_and_the_permissive_oracle(p, sigma):
    rng = np.random.default_rng(1000 + int(10 * sigma) + int(100 * p))       # the rows of the emulated test
    logits = (rng.standard_normal((512, 1024)) * sigma).astype(np.float32)
    p_q = ref.p_q_of(p)
    res = [_threshold(logits, None, p, scope) for scope in (0, 1)]
    assert res[0][0].tobytes() == res[1][0].tobytes() and np.array_equal(res[0][1], res[1][1])
    theta, kept = res[0]
    decided = 0
    for i in range(logits.shape[0]):
        strict, perm = ref.top_p_sandwich(logits[i], p_q)
        got = logits[i] >= theta[i]
        assert got.sum() == kept[i]
        assert (strict <= got).all() and (got <= perm).all(), (i, strict.sum(), got.sum(), perm.sum())
        decided += int(np.array_equal(strict, perm))
    print(f'p={p} sigma={sigma}: {decided} of 512 rows decided by the oracle')
    assert decided >= 0.95 * 512, decided
    # k and p together: p on the k survivors
    theta_k, _ = _threshold(logits[:32], 64, None, 0)
    theta_kp, kept_kp = _threshold(logits[:32], 64, p, 1)
    for i in range(32):
        surv = logits[i] >= theta_k[i]
        strict, perm = ref.top_p_sandwich(logits[i], p_q, survivors=surv)
        got = logits[i] >= theta_kp[i]
        assert (strict <= got).all() and (got <= perm).all() and (got <= surv).all() and got.sum() == kept_kp[i]


def test_a_row_with_nans_returns():
    """definition 7: an ordinary input, run once"""
    l = np.random.default_rng(5).standard_normal((2, 1024)).astype(np.float32)
    l[0, ::3] = np.nan
    l[1, :] = np.nan
    theta, kept = _threshold(l, 10, 0.9, 0)
    assert ((kept >= 0) & (kept <= 1024)).all()
    theta, kept = _threshold(l, 10, 0.9, 1)
    assert ((kept >= 0) & (kept <= 1024)).all()
    torch.cuda.synchronize()


def _tail_inputs(n, seed):
    g = torch.Generator().manual_seed(seed)
    hidden = (torch.randn(n, 512, generator=g) * 1.5 + 0.2).to(DEV)
    tex = torch.randint(0, 18, (n, ), generator=g).to(DEV)
    x_t = torch.full((n, ), MASK_ID, device=DEV)
    return hidden, tex, x_t


@pytest.mark.parametrize('kw', SETTINGS + [dict(top_k=1)], ids=str)
@pytest.mark.parametrize('temp', [1.0, 0.7])
def test_pick_sites_agree_and_philox_mode_equals_explicit_draws(model, temp, kw):
    P, n = model.P, 2 * 512
    hidden, tex, x_t = _tail_inputs(n, seed=5)
    g_, b_, W = P['tf.ln_f.g'], P['tf.ln_f.b'], P['tf.heads']
    rows = torch.arange(n, dtype=torch.int32, device=DEV)
    seed_all(11)
    seed, off = _gen().initial_seed(), _gen().get_offset()
    E = torch.empty(n, 1024, device=DEV).exponential_()
    toks = {}
    ws = torch.empty(n, 1024, device=DEV)
    for name, call in (('two-launch', dict(split=True, logits_ws=ws)), ('one-launch', dict(split=False)),
                       ('philox', dict(philox=(seed, {h: off for h in range(18)})))):
        x2, out2 = x_t.clone(), torch.full((18, n), -1, dtype=torch.int64, device=DEV)
        ops.sample_heads(hidden, g_, b_, W, {h: E for h in range(18)}, rows, n, tex, temp, x2, out2, **call, **kw)
        toks[name] = out2[tex, torch.arange(n, device=DEV)]
    conf_off, tok_off = torch.empty(n, device=DEV), torch.empty(n, dtype=torch.int32, device=DEV)
    ops.confidence_tail(hidden, g_, b_, W, tex, x_t, MASK_ID, temp, ('explicit', E), tok_off, conf_off)
    for noise in (('explicit', E), ('philox', seed, off)):
        tok, conf = torch.empty(n, dtype=torch.int32, device=DEV), torch.empty(n, device=DEV)
        ops.confidence_tail(hidden, g_, b_, W, tex, x_t, MASK_ID, temp, noise, tok, conf, **kw)
        toks['confidence ' + noise[0]] = tok.long()
    for name, t in toks.items():
        assert torch.equal(t, toks['two-launch']), name
    tok = toks['two-launch']
    assert int((tok != tok_off.long()).sum()) > 0                      # the setting does something here
    # inside the kernel's own kept set, and the best score there (torch's exp against the kernel's expf: the winner's
    # score is the maximum over the kept set up to a few ulp)
    theta, kept = ops.truncation_threshold(ws, scope=0, **kw)
    theta1, kept1 = ops.truncation_threshold(ws, scope=1, **kw)
    assert torch.equal(theta, theta1) and torch.equal(kept, kept1)
    keep = ws >= theta[:, None]
    assert torch.equal(keep.sum(1).int(), kept)
    assert bool(keep.gather(1, tok[:, None]).all())
    sc = torch.where(keep, torch.exp(ws - ws.max(1, keepdim=True).values) / E, torch.full_like(ws, -1.0))
    assert bool((sc.gather(1, tok[:, None])[:, 0] >= sc.max(1).values * (1 - 1e-5)).all())
    if kw == dict(top_k=1):
        assert torch.equal(tok, ws.argmax(1))
    # the confidence: bit-identical where the token did not change, the full-softmax log-probability elsewhere
    same = tok == tok_off.long()
    assert torch.equal(conf[same], conf_off[same])
    lp = torch.log_softmax(ws.double(), 1).gather(1, tok[:, None])[:, 0]
    assert float((lp - conf.double()).abs().max()) < 1e-5


def _feed(model, B, seed):
    model.feed_data(synthetic.parsing_batch(B, seed=seed))
    return model._texture_tokens(model.texture_mask)


@pytest.mark.parametrize('kw', SETTINGS + [dict(top_k=1)], ids=str)
@pytest.mark.parametrize('B,temp', [(2, 1.0), (8, 0.7)])
def test_every_sampled_token_lies_in_its_rows_kept_set(model, B, temp, kw):
    """A hook run of the whole loop: after every round the logits of the state the round saw are evaluated once more
    (net.logits, another GEMM path: equal to ACT_TOL) and every token the round wrote is checked against them -- fewer
    than k classes are clearly more likely (top-k), the classes clearly more likely hold less than top_p (top-p); with
    top_k = 1 the token is the row's argmax."""
    steps = 24
    tex_tok = _feed(model, B, 40 + B)
    segm = model.segm_tokens.contiguous()
    net = model.sampler_fn
    present = set(tex_tok.unique().tolist())
    prev = [torch.full((B, 512), MASK_ID, dtype=torch.int64, device=DEV)]
    seen = dict(rows=0)
    tol = 2 * ACT_TOL / min(temp, 1.0)

    def hook(r, steps_r, x_t, out):
        rows = (x_t != prev[0]).view(-1).nonzero().flatten()
        snapshot = x_t.clone()
        lg = net.logits(prev[0], segm, tex_tok, heads=present)
        tex = tex_tok.view(-1)[rows]
        tok = snapshot.view(-1)[rows] - 1024 * tex
        assert bool(((tok >= 0) & (tok < 1024)).all())
        l = torch.stack([lg[int(h)].reshape(B * 512, -1)[int(i)] for i, h in zip(rows.tolist(), tex.tolist())]) / temp
        l_tok = l.gather(1, tok[:, None])
        above = l > l_tok + tol
        if 'top_k' in kw:
            assert bool((above.sum(1) < kw['top_k']).all()), (r, above.sum(1).max())
        if 'top_p' in kw:
            prob = torch.softmax(l.double(), 1)
            assert bool(((prob * above).sum(1) < kw['top_p'] + 1e-3).all()), (r, float((prob * above).sum(1).max()))
        seen['rows'] += len(rows)
        x_t.copy_(snapshot)
        prev[0] = snapshot

    seed_all(3)
    engine.sample_tokens(net, segm, tex_tok, steps, MASK_ID, temp=temp, round_hook=hook, **kw)
    assert seen['rows'] == B * 512


@pytest.mark.parametrize('kw', SETTINGS, ids=str)
def test_graph_replay_and_shrinking_batch_give_the_same_tokens(model, monkeypatch, kw):
    B, steps = 4, 48
    _feed(model, B, 51)
    got = {}
    for graph in ('1', '0'):
        for shrink in ('1', '0'):
            monkeypatch.setenv('T2H_GRAPH', graph)
            monkeypatch.setenv('T2H_SHRINK_BATCH', shrink)
            seed_all(8)
            got[graph, shrink] = torch.stack(model.sample_fn(temp=1.0, sample_steps=steps, **kw))
            assert model.sampler_fn.last_launch_mode == ('graph' if graph == '1' else 'eager')
    for key, t in got.items():
        assert torch.equal(t, got['1', '1']), key
    monkeypatch.setenv('T2H_GRAPH', '1')
    monkeypatch.setenv('T2H_SHRINK_BATCH', '1')
    seed_all(8)
    plain = torch.stack(model.sample_fn(temp=1.0, sample_steps=steps))
    assert not torch.equal(plain, got['1', '1'])                      # a graph captured for one setting is not reused
    seed_all(8)
    assert torch.equal(torch.stack(model.sample_fn(temp=1.0, sample_steps=steps, **kw)), got['1', '1'])


def test_generator_offsets_do_not_depend_on_truncation(model):
    B, steps = 2, 32
    _feed(model, B, 52)
    seed_all(4)
    src = model.sample_fn(temp=1.0, sample_steps=steps)
    keep = (torch.rand(B, 512, generator=torch.Generator().manual_seed(1)) < 0.5).to(torch.uint8)
    calls = {
        'sample_fn': lambda **kw: model.sample_fn(temp=1.0, sample_steps=steps, **kw),
        'sample_fn_confidence': lambda **kw: model.sample_fn_confidence(rounds=8, **kw),
        'resample_fn': lambda **kw: model.resample_fn(src, keep, sample_steps=steps, **kw),
        'resample_fn confidence': lambda **kw: model.resample_fn(src, keep, order='confidence', rounds=8, **kw),
    }
    for name, call in calls.items():
        seed_all(9)
        base = torch.stack(call())
        off = _gen().get_offset()
        for kw in SETTINGS:
            seed_all(9)
            got = torch.stack(call(**kw))
            assert _gen().get_offset() == off, (name, kw)
            assert not torch.equal(got, base), (name, kw)
            if name.startswith('resample_fn'):                        # kept rows are never rewritten
                k = keep.bool().to(DEV)
                assert torch.equal(got[:, k], torch.stack(src)[:, k]), (name, kw)
        seed_all(9)
        assert torch.equal(torch.stack(call(top_k=None, top_p=None)), base)
        seed_all(9)
        assert torch.equal(torch.stack(call(top_k=0, top_p=1.0)), base)
    # a bad value raises before the generator has moved
    seed_all(9)
    before = _gen().get_offset()
    for bad in (dict(top_k=-2), dict(top_p=0.0), dict(top_p=1.5)):
        with pytest.raises(ValueError):
            model.sample_fn(temp=1.0, sample_steps=steps, **bad)
        with pytest.raises(ValueError):
            model.sample_fn_confidence(rounds=8, **bad)
    assert _gen().get_offset() == before


def test_editing_with_nothing_kept_is_sample_fn(model):
    B, steps = 2, 32
    _feed(model, B, 53)
    seed_all(4)
    src = model.sample_fn(temp=1.0, sample_steps=steps)
    for kw in (dict(top_p=0.9), dict(top_k=64)):
        seed_all(6)
        want = torch.stack(model.sample_fn(temp=1.0, sample_steps=steps, **kw))
        seed_all(6)
        got = torch.stack(model.resample_fn(src, torch.zeros(B, 512, dtype=torch.uint8), sample_steps=steps, **kw))
        assert torch.equal(got, want)
    model.sample_steps = steps
    seed_all(6)
    want = torch.stack(model.sample_fn(temp=1.0, sample_steps=steps, top_p=0.9))
    seed_all(6)
    region = torch.ones(B, 1, 512, 256, dtype=torch.uint8)           # everything is in the region: nothing is kept
    model.edit_and_refine(src, region=region, top_p=0.9)
    assert torch.equal(torch.stack(model.edit_top_indices_list), want)


def test_options_switch_sample_and_refine(opt, model):
    B = 2
    _feed(model, B, 54)
    model.sample_steps = 24
    seed_all(2)
    want = torch.stack(model.sample_fn(temp=1, sample_steps=24, top_k=32, top_p=0.8))
    seen = []
    orig = model.sample_fn
    try:
        model.opt = defaults.with_truncation(options.dict_to_nonedict(dict(opt)), top_k=32, top_p=0.8)
        model.sample_fn = lambda **kw: seen.append(orig(**kw)) or seen[-1]
        seed_all(2)
        model.sample_and_refine()
    finally:
        model.sample_fn = orig
        model.opt = opt
    assert torch.equal(torch.stack(seen[0]), want)
