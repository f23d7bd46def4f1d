"""Confidence-ordered parallel decoding on the GPU (-m gpu; DESIGN.md, "Confidence-ordered decoding"): the two kernels
against t2h_sample_heads / plain torch, the whole loop teacher-forced against the restatement of tests/confidence_ref.py
on the oracle's transformer, the free-running default path, the corner schedules, editing and the option surface.
Synthetic checkpoints: nothing here says anything about image quality."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import confidence_ref as CR
from oracle import torch_ref as R
from text2human_amd import defaults, engine, ops, options, schedule, synthetic
from text2human_amd.models import SampleFromParsingModel

from parity_util import ACT_TOL, osds, seed_all  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda'
MASK_ID = 18432
SEEDS = (2021, 7)      # usable by profiles/confidence_parity.json (tools/confidence_parity_seeds.py)
SCALE = 1.0            # head scale of the default synthetic weights (tests/test_gpu_bench_parity.py)


@pytest.fixture(scope='module')
def opt():
    return options.dict_to_nonedict(defaults.sample_from_parsing())


@pytest.fixture(scope='module')
def sds(opt):
    return synthetic.make_state_dicts(opt, seed=1234)


@pytest.fixture(scope='module')
def model(opt, sds):
    return SampleFromParsingModel(opt, state_dicts=sds)


def _gen():
    return torch.cuda.default_generators[torch.cuda.current_device()]


def _tail_inputs(model, n, seed, masked_frac=0.8):
    g = torch.Generator().manual_seed(seed)
    hidden = (torch.randn(n, 512, generator=g) * 1.5 + 0.2).to(DEV)
    tex = torch.randint(0, 18, (n, ), generator=g).to(DEV)
    masked = (torch.rand(n, generator=g) < masked_frac).to(DEV)
    x_t = torch.where(masked, torch.full((n, ), MASK_ID, device=DEV), tex * 1024 + 3)
    E = torch.empty(n, 1024).exponential_(generator=g).to(DEV)
    return hidden, tex, masked, x_t, E


# float32 torch restatement of the confidence against float64, same inputs, on the CPU: 8.57e-7 (temp 1.0), 1.125e-6
# (temp 0.7); allowed here 8 x that (another summation order over 512 + 1024 terms): 6.9e-6 / 9.0e-6
C_ERR_F32 = {1.0: 8.57e-7, 0.7: 1.125e-6}


@pytest.mark.parametrize('temp', [1.0, 0.7])
def test_tail_draws_the_token_of_sample_heads_and_its_log_probability(model, temp):
    """Same hidden state fed to t2h_confidence_tail and t2h_sample_heads: the drawn tokens are equal as integers (explicit
    draws and the in-kernel Philox draws); the confidence is the float64 log-probability of that token within 8 x the
    error of the float32 torch restatement of the same formula measured against float64 on the CPU on these inputs
    (8.57e-7 at temp 1.0, 1.125e-6 at temp 0.7 -> allowed 6.9e-6 / 9.0e-6)."""
    P, n = model.P, 4 * 512
    hidden, tex, masked, x_t, E = _tail_inputs(model, n, seed=5)
    g_, b_, W = P['tf.ln_f.g'], P['tf.ln_f.b'], P['tf.heads']
    tok = torch.full((n, ), -7, dtype=torch.int32, device=DEV)
    conf = torch.zeros(n, device=DEV)
    x_before = x_t.clone()
    ops.confidence_tail(hidden, g_, b_, W, tex, x_t, MASK_ID, temp, ('explicit', E), tok, conf)
    assert torch.equal(x_t, x_before)
    assert (tok[~masked] == -1).all() and torch.isneginf(conf[~masked]).all()
    rows = masked.nonzero().flatten().to(torch.int32)
    x2, out2 = x_t.clone(), torch.full((18, n), -1, dtype=torch.int64, device=DEV)
    ops.sample_heads(hidden, g_, b_, W, {h: E for h in range(18)}, rows, len(rows), tex, temp, x2, out2)
    r = rows.long()
    want_tok = out2[tex[r], r]
    assert torch.equal(tok[r].long(), want_tok)
    # the in-kernel draw: the elements of torch's exponential_ tensor at the generator's state
    seed_all(11)
    seed, off = _gen().initial_seed(), _gen().get_offset()
    E_t = torch.empty(n, 1024, device=DEV).exponential_()
    tok_p, conf_p = torch.empty_like(tok), torch.empty_like(conf)
    ops.confidence_tail(hidden, g_, b_, W, tex, x_t, MASK_ID, temp, ('philox', seed, off), tok_p, conf_p)
    x3, out3 = x_t.clone(), torch.full((18, n), -1, dtype=torch.int64, device=DEV)
    ops.sample_heads(hidden, g_, b_, W, {h: E_t for h in range(18)}, rows, len(rows), tex, temp, x3, out3)
    assert torch.equal(tok_p[r].long(), out3[tex[r], r])
    # confidence against float64
    y = F.layer_norm(hidden.double(), (512, ), g_.double(), b_.double(), 1e-5)
    err = 0.0
    for h in range(18):
        sel = r[tex[r] == h]
        lp = torch.log_softmax((y[sel] @ W[h].double().t()) / temp, -1)
        err = max(err, float((lp.gather(1, tok[sel].long()[:, None])[:, 0] - conf[sel].double()).abs().max()))
    print(f'confidence vs float64: max abs err {err:.3e} (float32 torch restatement: {C_ERR_F32[temp]:.3e})')
    assert err <= 8 * C_ERR_F32[temp], err


def _restated_commit(scores, x_t, k):
    B, T = x_t.shape
    s, m = scores.view(B, T).double().cpu().numpy(), (x_t == MASK_ID).cpu().numpy()
    return [set(CR.top_k_rows(s[b], m[b], k[b])[0].tolist()) for b in range(B)]


def test_commit_is_the_stable_top_k_of_the_scores(model):
    B, T, n = 4, 512, 4 * 512
    hidden, tex, masked, x_flat, E = _tail_inputs(model, n, seed=6, masked_frac=0.7)
    P = model.P
    tok, conf = torch.empty(n, dtype=torch.int32, device=DEV), torch.empty(n, device=DEV)
    ops.confidence_tail(hidden, P['tf.ln_f.g'], P['tf.ln_f.b'], P['tf.heads'], tex, x_flat, MASK_ID, 1.0, ('explicit', E),
                        tok, conf)
    U = torch.rand(n, generator=torch.Generator().manual_seed(3)).to(DEV)
    hand = -(torch.randint(0, 5, (n, ), generator=torch.Generator().manual_seed(4)).float()).to(DEV)   # ties
    hand[::7] = float('nan')
    M = masked.view(B, T).sum(1).tolist()
    for name, cf, tau in (('device-made', conf, 2.5), ('hand-made', hand.contiguous(), 0.0)):
        for k in ([0, 1, M[2] - 1, M[3]], [33, 40, 50, 60]):
            x_t = x_flat.clone().view(B, T)
            out = torch.full((18, n), -1, dtype=torch.int64, device=DEV)
            scores = torch.empty(n, device=DEV)
            ops.confidence_commit(cf, tok, tex, ('explicit', U), torch.tensor(k, dtype=torch.int32, device=DEV),
                                  torch.tensor([tau], device=DEV), MASK_ID, x_t, out, 1024, scores=scores)
            want = _restated_commit(scores, x_flat.view(B, T), k)
            changed = (x_t != x_flat.view(B, T))
            for b in range(B):
                got = set(changed[b].nonzero().flatten().tolist())
                assert got == want[b] and len(got) == k[b], (name, k, b)
            assert torch.equal(x_t[~masked.view(B, T)], x_flat.view(B, T)[~masked.view(B, T)])
            rr = changed.view(-1).nonzero().flatten()
            assert torch.equal(x_t.view(-1)[rr], tok[rr].long() + 1024 * tex[rr])
            assert torch.equal(out[tex[rr], rr], tok[rr].long()) and int((out >= 0).sum()) == len(rr)
            if tau == 0.0:
                mm = masked.cpu().numpy()
                assert np.array_equal(scores.cpu().numpy()[mm], cf.cpu().numpy()[mm], equal_nan=True)


def _feed(model, B, seed):
    model.feed_data(synthetic.parsing_batch(B, seed=seed))
    return model._texture_tokens(model.texture_mask)


def _forced(model, net, sds, B, rounds, seed):
    """One teacher-forced run -> (pairs, pairs with an excused row, token mismatches, unexplained)"""
    tex_tok = _feed(model, B, seed)
    segm = model.segm_tokens.contiguous()
    sd = {k: v.to(DEV) for k, v in sds['sampler'].items()}
    seed_all(seed)
    E, U = CR.draws(B * 512, rounds, DEV)
    trace = []
    CR.run(segm, tex_tok, sd, E, U, rounds, trace=trace)
    by_r = {t['r']: t for t in trace}
    tot = dict(pairs=0, excused=0, tokens=0, unexplained=[])
    present = set(tex_tok.unique().tolist())

    def hook(r, x_t, out, tok, conf, scores):
        tr = by_r[r]
        own = [set(s) for s in _restated_commit(scores, tr['prev'], tr['k'])]
        changed = (x_t != tr['prev'])
        for b in range(B):   # the device commits the top k of its OWN scores, exactly
            assert set(changed[b].nonzero().flatten().tolist()) == own[b], (r, b)
        lg = net.logits(tr['prev'], segm, tex_tok, heads=present)
        lm = torch.zeros_like(tr['logits'])
        for h in present:
            sel = tex_tok.view(-1) == h
            lm[sel] = lg[h].reshape(B * 512, -1)[sel]
        c = CR.compare_round(tr, E[r - 1], tok.clone(), x_t.clone(), lm, ACT_TOL * SCALE)
        tot['pairs'] += B
        tot['excused'] += len(c['excused_samples'])
        tot['tokens'] += c['token_mismatches']
        tot['unexplained'] += c['unexplained_tokens'] + c['unexcused_rows']
        x_t.copy_(tr['x_t'])
        out.copy_(tr['out'])

    seed_all(seed)
    got = engine.sample_tokens_confidence(net, segm, tex_tok, MASK_ID, rounds=rounds, round_hook=hook)
    assert torch.equal(got, trace[-1]['out'])
    return tot


@pytest.mark.parametrize('path', ['exact_fp32', 'default'])
@pytest.mark.parametrize('B,rounds', [(2, 8), (2, 16), (8, 8), (8, 16)])
def test_whole_loop_teacher_forced(model, sds, opt, path, B, rounds):
    net = model.sampler_fn if path == 'default' else model._exact_sampler()
    pairs = excused = tokens = 0
    for seed in SEEDS:
        t = _forced(model, net, sds, B, rounds, seed)
        assert not t['unexplained'], t['unexplained'][:5]
        pairs, excused, tokens = pairs + t['pairs'], excused + t['excused'], tokens + t['tokens']
    print(f'{path} B={B} R={rounds}: {pairs} (round, sample) pairs, {excused} with an excused row, {tokens} token near-ties')
    assert excused <= 0.01 * pairs, (excused, pairs)


def test_default_path_free_running(model):
    B, rounds, T = 4, 16, 512
    tex_tok = _feed(model, B, 31)
    seen = []

    def hook(r, x_t, out, tok, conf, scores):
        seen.append((x_t == MASK_ID).sum(1).tolist())

    seed_all(5)
    net = model.sampler_fn
    a = engine.sample_tokens_confidence(net, model.segm_tokens.contiguous(), tex_tok, MASK_ID, rounds=rounds,
                                        round_hook=hook)
    m, _ = schedule.confidence_schedule(T, rounds)
    assert seen == [[int(m[r])] * B for r in range(1, rounds + 1)]           # exactly k_r rows per round and sample
    st = net.last_stats
    assert st['mode'] == 'confidence' and st['rounds'] == rounds and st['sample_steps_launched'] == B * rounds
    seed_all(5)
    lists = model.sample_fn_confidence(rounds=rounds)
    state_after = _gen().get_state()
    got = torch.stack(lists).view(18, -1)
    assert len(lists) == 18 and lists[0].shape == (B, T) and lists[0].dtype == torch.int64
    assert torch.equal(got, a)                                                # same seed: bit-identical
    tex = tex_tok.view(-1)
    own = got.gather(0, tex[None])[0]
    assert ((own >= 0) & (own < 1024)).all() and int((got >= 0).sum()) == B * T   # valid under the row's texture, -1 elsewhere
    seed_all(6)
    assert not torch.equal(torch.stack(model.sample_fn_confidence(rounds=rounds)).view(18, -1), got)
    seed_all(5)
    CR.draws(B * T, rounds, DEV)                                              # the 2 R torch draws of the stated shapes
    assert torch.equal(_gen().get_state(), state_after)


def test_pure_confidence_order_and_single_round(model):
    B, T = 2, 512
    tex_tok = _feed(model, B, 32)
    segm = model.segm_tokens.contiguous()
    state = dict(prev=torch.full((B, T), MASK_ID, dtype=torch.int64, device=DEV), n=0)

    def hook(r, x_t, out, tok, conf, scores):
        masked = state['prev'] == MASK_ID
        changed = x_t != state['prev']
        assert changed.sum(1).tolist() == [1] * B
        s = torch.where(masked, conf.view(B, T), torch.full_like(conf.view(B, T), float('-inf')))
        assert torch.equal(scores.view(B, T)[masked], conf.view(B, T)[masked])     # tau = 0
        assert torch.equal(changed.float().argmax(1), s.argmax(1))                 # the most confident row
        state['prev'] = x_t.clone()
        state['n'] += 1

    seed_all(8)
    out = engine.sample_tokens_confidence(model.sampler_fn, segm, tex_tok, MASK_ID, rounds=512, choice_temp=0.0,
                                          round_hook=hook)
    assert state['n'] == 512 and int((out >= 0).sum()) == B * T
    toks = {}

    def hook1(r, x_t, out, tok, conf, scores):
        toks[r] = tok.clone()

    seed_all(8)
    out = engine.sample_tokens_confidence(model.sampler_fn, segm, tex_tok, MASK_ID, rounds=1, round_hook=hook1)
    assert list(toks) == [1] and torch.equal(out.gather(0, tex_tok.view(1, -1))[0], toks[1].long())


def test_editing_in_confidence_order(model, tmp_path):
    B, T, rounds = 3, 512, 8
    _feed(model, B, 33)
    seed_all(1)
    src = model.sample_fn(temp=1, sample_steps=32)
    keep = torch.zeros(B, T, dtype=torch.uint8, device=DEV)
    keep[0, :400] = 1                       # 112 rows resampled
    keep[1, ::2] = 1                        # 256
    keep[2] = 1                             # M0 = 0: left alone
    seen = []
    orig = engine.sample_tokens_confidence

    def spy(*a, **kw):
        kw['round_hook'] = lambda r, x_t, *_: seen.append((x_t == MASK_ID).sum(1).tolist())
        return orig(*a, **kw)

    engine.sample_tokens_confidence = spy
    try:
        seed_all(2)
        got = torch.stack(model.resample_fn(src, keep, order='confidence', rounds=rounds))
    finally:
        engine.sample_tokens_confidence = orig
    ms = [schedule.confidence_schedule(m0, rounds)[0] for m0 in (112, 256, 0)]
    assert seen == [[int(m[r]) for m in ms] for r in range(1, rounds + 1)]
    k = keep.bool()
    src_t = torch.stack(src)
    kk = k.unsqueeze(0).expand(18, -1, -1)
    assert torch.equal(got[kk], src_t[kk]) and int((got >= 0).sum()) == B * T
    assert model.sampler_fn.last_stats['rows_kept'] == int(k.sum())
    assert torch.equal(torch.stack(model.resample_fn(src, torch.ones_like(keep), order='confidence')), src_t)
    # end to end, like the random order: an image, and the PNGs
    from PIL import Image
    seed_all(3)
    img = model.edit_and_refine(src, labels=(1, 2, 3), order='confidence', rounds=rounds)
    assert tuple(img.shape) == (1, 3, 512, 256) and bool(torch.isfinite(img).all())
    names = [f'e{i}.png' for i in range(B)]
    seed_all(3)
    u8 = model.edit_and_refine(src, labels=(1, 2, 3), save_dir=str(tmp_path), img_name=names, order='confidence',
                               rounds=rounds)
    for i, nm in enumerate(names):
        assert np.array_equal(np.asarray(Image.open(os.path.join(str(tmp_path), nm))), u8[i].cpu().numpy())
    with pytest.raises(ValueError):
        model.resample_fn(src, keep, order='best')


def test_sample_and_refine_takes_the_mode_from_the_options(sds, tmp_path):
    opt = options.dict_to_nonedict(defaults.with_confidence_order(defaults.sample_from_parsing(), rounds=8))
    m = SampleFromParsingModel(opt, state_dicts=sds)
    m.feed_data(synthetic.parsing_batch(2, seed=3))
    names = ['a.png', 'b.png']
    seed_all(4)
    m.sample_and_refine(str(tmp_path), names)
    assert all(os.path.getsize(os.path.join(str(tmp_path), nm)) > 0 for nm in names)
    assert m.sampler_fn.last_stats['mode'] == 'confidence' and m.sampler_fn.last_stats['rounds'] == 8
    assert tuple(m.sample_and_refine().shape) == (1, 3, 512, 256)
