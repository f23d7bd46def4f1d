"""Per-token log-probabilities of the index sampler and best-of-N on the GPU (-m gpu).

The flag is an observer: with return_logp the samplers draw the tokens, and consume the generator, of the call without
it, on the graph path and the eager one, with and without finished samples leaving the batch.  The number itself is
checked against a float64 recomputation from the state every round started from; confidence mode returns the very bits
the committing round ranked with; image b of a per-image batch has the bits of its scalar run; sample_best_of(3) is
three consecutive plain calls and a per-image maximum."""
import numpy as np
import pytest
import torch

from text2human_amd import defaults, engine, ops, options, synthetic
from text2human_amd.models import SampleFromParsingModel

import logp_ref as ref  # noqa: E402
from parity_util import ACT_TOL, seed_all  # noqa: E402

pytestmark = pytest.mark.gpu
B, T, STEPS, HEAD_SCALE = 3, 512, 16, 5.0
TEMP, TOP_K, TOP_P = (1.0, 0.7, 1.3), (None, 5, None), (None, None, 0.6)
MODES = [('1', '1'), ('1', '0'), ('0', '1'), ('0', '0')]   # (T2H_GRAPH, T2H_SHRINK_BATCH)


def allowance(temp):
    """how far a loop's logp may be from the float64 recomputation: the hidden state moves by ACT_TOL (the tail GEMM's
    tile depends on the round's row count), a logit by ACT_TOL * head_scale / temp, a softmax log-probability by at most
    twice the largest logit change; plus the kernel-level bound of tests/test_logp_emulated.py"""
    return 2 * ACT_TOL * HEAD_SCALE / temp + 8 * ref.LOGP_ERR_F32[temp]


@pytest.fixture(scope='module')
def opt():
    return options.dict_to_nonedict(defaults.sample_from_parsing())


@pytest.fixture(scope='module')
def model(opt):
    m = SampleFromParsingModel(opt, state_dicts=synthetic.make_state_dicts(opt, seed=1234, head_scale=HEAD_SCALE))
    m.feed_data(synthetic.parsing_batch(B, seed=91))
    return m


def _gen():
    return torch.cuda.default_generators[torch.cuda.current_device()]


def _run(fn, seed, **kw):
    """-> (result of fn, generator offset after the call - before it)"""
    seed_all(seed)
    off0 = _gen().get_offset()
    out = fn(**kw)
    return out, _gen().get_offset() - off0


@pytest.mark.parametrize('graph,shrink', MODES)
def test_the_flag_changes_neither_tokens_nor_generator(model, monkeypatch, graph, shrink):
    monkeypatch.setenv('T2H_GRAPH', graph)
    monkeypatch.setenv('T2H_SHRINK_BATCH', shrink)
    want, adv = _run(model.sample_fn, 17, sample_steps=STEPS)
    (lists, logp), adv_lp = _run(model.sample_fn, 17, sample_steps=STEPS, return_logp=True)
    assert model.sampler_fn.last_launch_mode == ('graph' if graph == '1' else 'eager')
    assert adv_lp == adv and torch.equal(torch.stack(lists), torch.stack(want))
    assert logp.dtype == torch.float32 and tuple(logp.shape) == (B, T)
    assert bool(torch.isfinite(logp).all()) and bool((logp <= 0).all())          # every row is drawn
    assert float(logp.std()) > 0.2


def _edit_keep():
    """the keep pattern of tests/test_gpu_per_image.py: image 0 resamples 3 rows (the fewest rounds), image 1 everything,
    image 2 every other row"""
    keep = torch.zeros(B, T, dtype=torch.uint8)
    keep[0] = 1
    keep[0, [5, 200, 411]] = 0
    keep[2, ::2] = 1
    return keep


@pytest.mark.parametrize('graph', ['1', '0'])
def test_kept_rows_are_nan_and_logp_follows_the_reordered_batch(model, monkeypatch, graph):
    monkeypatch.setenv('T2H_GRAPH', graph)
    monkeypatch.setenv('T2H_SHRINK_BATCH', '1')
    perms, real = [], engine.schedule.plan_rounds

    def plan(*a, **kw):
        p = real(*a, **kw)
        perms.append(p.perm)
        return p

    src, _ = _run(model.sample_fn, 23, sample_steps=STEPS)
    keep = _edit_keep()
    monkeypatch.setattr(engine.schedule, 'plan_rounds', plan)
    want, adv = _run(model.resample_fn, 29, top_indices_list=src, keep=keep, sample_steps=STEPS)
    (lists, logp), adv_lp = _run(model.resample_fn, 29, top_indices_list=src, keep=keep, sample_steps=STEPS, return_logp=True)
    assert adv_lp == adv and torch.equal(torch.stack(lists), torch.stack(want))
    # image 0 finishes first and leaves the batch: the schedule's sample order is not the caller's
    assert len(perms) == 2 and all(p is not None and int(p[-1]) == 0 and list(p) != [0, 1, 2] for p in perms), perms
    k = keep.bool().to(logp.device)
    assert bool(torch.isnan(logp[k]).all()) and bool(torch.isfinite(logp[~k]).all()) and bool((logp[~k] <= 0).all())
    assert int(torch.isfinite(logp[0]).sum()) == 3 and torch.isfinite(logp[0]).nonzero().view(-1).tolist() == [5, 200, 411]
    s, c, m = ops.logp_summary(logp.contiguous())
    assert c.tolist() == [3, T, T // 2] and bool((m <= 0).all())


def _hooked_run(model, seed, temp=1.0):
    """the eager loop with a round_hook -> (out, logp, [(x_t before the round, x_t after it)])"""
    net, states = model.sampler_fn, []
    tex_tok = model._texture_tokens(model.texture_mask)
    segm = model.segm_tokens.contiguous()
    prev = [torch.full((B, T), model.mask_id, dtype=torch.int64, device=segm.device)]

    def hook(r, steps, x_t, out):
        states.append((prev[0], x_t.clone()))
        prev[0] = x_t.clone()

    seed_all(seed)
    out, logp = engine.sample_tokens(net, segm, tex_tok, STEPS, model.mask_id, temp=temp, round_hook=hook,
                                     return_logp=True)
    assert net.last_launch_mode == 'eager'
    return out, logp, states, segm, tex_tok


def test_the_loops_logp_against_float64(model):
    temp = 1.0
    out, logp, states, segm, tex_tok = _hooked_run(model, 17, temp)
    net = model.sampler_fn
    want = torch.full((B * T, ), float('nan'), dtype=torch.float64, device=logp.device)
    tex = tex_tok.view(-1)
    for before, after in states:
        drawn = ((before != model.mask_id) != (after != model.mask_id)).view(-1).nonzero().view(-1)
        if drawn.numel() == 0:
            continue
        hs = set(tex[drawn].tolist())
        lg = net.logits(before, segm, tex_tok, heads=hs)
        for h in hs:
            rows = drawn[tex[drawn] == h]
            lp = torch.log_softmax(lg[h].view(B * T, -1)[rows].double() / temp, -1)
            tok = after.view(-1)[rows] - 1024 * h
            assert bool(((tok >= 0) & (tok < 1024)).all())
            want[rows] = lp.gather(1, tok[:, None])[:, 0]
    assert bool(torch.isfinite(want).all())                                      # every row was drawn in some round
    err = float((logp.double() - want).abs().max())
    print(f'loop logp vs float64: max abs err {err:.3e}, allowed {allowance(temp):.3e}, spread {float(want.std()):.3f}')
    assert err <= allowance(temp), err
    assert float(want.std()) >= 100 * allowance(temp)                            # a mis-routed row cannot hide


def test_graph_path_agrees_with_the_eager_path(model, monkeypatch):
    seed = 17
    monkeypatch.setenv('T2H_GRAPH', '1')
    (lists_g, logp_g), _ = _run(model.sample_fn, seed, sample_steps=STEPS, return_logp=True)
    assert model.sampler_fn.last_launch_mode == 'graph'
    monkeypatch.setenv('T2H_GRAPH', '0')
    (lists_e, logp_e), _ = _run(model.sample_fn, seed, sample_steps=STEPS, return_logp=True)
    assert model.sampler_fn.last_launch_mode == 'eager'
    assert torch.equal(torch.stack(lists_g), torch.stack(lists_e))               # (on this seed the tokens are all equal)
    err = float((logp_g.double() - logp_e.double()).abs().max())
    print(f'graph vs eager logp: max abs diff {err:.3e}, allowed {allowance(1.0):.3e}')
    assert err <= allowance(1.0)


def test_confidence_mode_returns_the_bits_the_committing_round_ranked_with(model):
    net = model.sampler_fn
    tex_tok = model._texture_tokens(model.texture_mask)
    segm = model.segm_tokens.contiguous()
    want_tok, adv = _run(model.sample_fn_confidence, 31, rounds=6)
    (lists, logp), adv_lp = _run(model.sample_fn_confidence, 31, rounds=6, return_logp=True)
    assert adv_lp == adv and torch.equal(torch.stack(lists), torch.stack(want_tok))
    seen = torch.full((B * T, ), float('nan'), dtype=torch.float32, device=logp.device)
    masked = [torch.ones(B * T, dtype=torch.bool, device=logp.device)]

    def hook(r, x_t, out, tok, conf, scores):
        now = (x_t == model.mask_id).view(-1)
        committed = masked[0] & ~now
        seen[committed] = conf[committed]
        masked[0] = now

    seed_all(31)
    out, logp_h = engine.sample_tokens_confidence(net, segm, tex_tok, model.mask_id, rounds=6, round_hook=hook,
                                                  return_logp=True)
    assert not bool(masked[0].any()) and torch.equal(out, torch.stack([x.reshape(-1) for x in lists]))
    assert logp_h.cpu().numpy().tobytes() == seen.cpu().numpy().tobytes()
    assert logp.reshape(-1).cpu().numpy().tobytes() == seen.cpu().numpy().tobytes()
    assert bool(torch.isfinite(seen).all()) and bool((seen <= 0).all())


def test_image_b_of_a_mixed_batch_has_the_logp_of_its_scalar_run(model):
    seqs = dict(temp=list(TEMP), top_k=list(TOP_K), top_p=list(TOP_P))
    (lists, logp), adv = _run(model.sample_fn, 17, sample_steps=STEPS, return_logp=True, **seqs)
    assert model.sampler_fn.last_launch_mode == 'graph'
    for b in range(B):
        own = {k: v[b] for k, v in seqs.items()}
        (want, want_lp), adv_b = _run(model.sample_fn, 17, sample_steps=STEPS, return_logp=True, **own)
        assert adv_b == adv and torch.equal(torch.stack(lists)[:, b], torch.stack(want)[:, b]), b
        assert logp[b].cpu().numpy().tobytes() == want_lp[b].cpu().numpy().tobytes(), b
        if b:   # ... and its own values matter: another image's scalar run gives this image other numbers
            assert not torch.equal(logp[b - 1], want_lp[b - 1]), b


BEST_SEED = 17   # (on this seed the three images do not all keep candidate 0: asserted below)


def test_best_of_three_is_three_consecutive_calls_and_a_maximum(model):
    seed_all(BEST_SEED)
    off0 = _gen().get_offset()
    cands, offs = [], []
    for _ in range(3):
        cands.append(model.sample_fn(sample_steps=STEPS, return_logp=True))
        offs.append(_gen().get_offset() - off0)
    adv3 = offs[-1]
    (lists, logp, score, choice), adv = _run(model.sample_best_of, BEST_SEED, n=3, sample_steps=STEPS)
    assert adv == adv3                                                           # the generator ends where three calls end
    assert choice.dtype == torch.int64 and tuple(choice.shape) == (B, ) and score.dtype == torch.float32
    lp = np.stack([c[1].cpu().numpy() for c in cands])
    want_choice, want_score = ref.best_of(lp)
    got = torch.stack(lists)
    for b in range(B):
        c = int(choice[b])
        assert torch.equal(got[:, b], torch.stack(cands[c][0])[:, b]), b
        assert logp[b].cpu().numpy().tobytes() == cands[c][1][b].cpu().numpy().tobytes(), b
        # the score is a float32 sum / count of T terms: within T * 2^-24 of the float64 mean's magnitude
        assert abs(float(score[b]) - want_score[b]) <= T * 2.0**-24 * abs(want_score[b]) + 1e-12, b
    assert choice.tolist() == want_choice.tolist()
    assert len(set(choice.tolist())) > 1 or int(choice[0]) != 0                  # not every image keeps candidate 0
    (l1, lp1, s1, c1), adv1 = _run(model.sample_best_of, BEST_SEED, n=1, sample_steps=STEPS)
    assert torch.equal(torch.stack(l1), torch.stack(cands[0][0])) and torch.equal(lp1, cands[0][1])
    assert c1.tolist() == [0] * B and adv1 == offs[0]                            # n = 1 is the plain call
    with pytest.raises(ValueError, match='sample_best_of.*0'):
        model.sample_best_of(0)


def test_runs_without_the_flag_keep_their_keys_and_captures(model, monkeypatch):
    monkeypatch.setenv('T2H_GRAPH', '1')
    net = model.sampler_fn
    want, _ = _run(model.sample_fn, 41, sample_steps=STEPS)
    keys = set(net._graphs)
    plain_keys = {k for k in keys if 'logp' not in k}
    captured = {k: dict(net._graphs[k].graphs) for k in plain_keys}
    _run(model.sample_fn, 41, sample_steps=STEPS, return_logp=True)
    with_flag = {k for k in net._graphs if 'logp' in k}                          # (earlier tests' flagged runs included)
    assert all(k[-1] == 'logp' for k in with_flag) and any(k[:-1] in plain_keys for k in with_flag)
    assert set(net._graphs) - with_flag == plain_keys                            # the flagged run added no plain key
    n_graphs = len(net._graphs)
    again, _ = _run(model.sample_fn, 41, sample_steps=STEPS)
    assert torch.equal(torch.stack(again), torch.stack(want))
    assert len(net._graphs) == n_graphs and {k for k in net._graphs if 'logp' not in k} == plain_keys
    for k in plain_keys:   # the very captures, not new ones under the old keys
        assert net._graphs[k].logp is None
        assert all(net._graphs[k].graphs[c] is g for c, g in captured[k].items())
