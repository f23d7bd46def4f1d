"""Scoring a given token map on the GPU (-m gpu).

The round trip: a map that sample_fn(return_logp=True) drew at generator state G, scored by score_fn at state G, returns
that call's logp bits and moves the generator as far -- on the graph path and the eager one, with and without finished
samples leaving the batch, with a scalar and with per-image temperatures, and after a region edit on the rows the edit
drew.  That pins the logp path, the schedule, the graph path and the batch reordering against each other with no
tolerance.  The number itself is checked on a map the model did not draw, against a float64 recomputation from the state
every round started from."""
import pytest
import torch

from text2human_amd import _lib, defaults, engine, ops, options, synthetic
from text2human_amd.models import SampleFromParsingModel

from parity_util import ACT_TOL, seed_all  # noqa: E402

pytestmark = pytest.mark.gpu
B, T, STEPS, HEAD_SCALE = 3, 512, 16, 5.0                                        # the fixture of tests/test_gpu_logp.py
N_CLASS = 1024
TEMPS = [1.0, 0.7, 1.3]
MODES = [('1', '1'), ('1', '0'), ('0', '1'), ('0', '0')]   # (T2H_GRAPH, T2H_SHRINK_BATCH)


def allowance(temp, f32):
    """tests/test_gpu_logp.py's: the hidden state moves by ACT_TOL (the tail GEMM's tile depends on the round's row
    count), a logit by ACT_TOL * head_scale / temp, a softmax log-probability by at most twice the largest logit change;
    plus 8 x the float32 yardstick of the rows compared"""
    return 2 * ACT_TOL * HEAD_SCALE / temp + 8 * f32


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


def _run(fn, seed, *a, **kw):
    """-> (result of fn, generator offset after the call - before it)"""
    seed_all(seed)
    off0 = _gen().get_offset()
    out = fn(*a, **kw)
    return out, _gen().get_offset() - off0


def _bytes(t):
    return t.contiguous().cpu().numpy().tobytes()


@pytest.mark.parametrize('graph,shrink', MODES)
def test_a_drawn_map_scores_the_bits_it_was_drawn_with(model, monkeypatch, graph, shrink):
    monkeypatch.setenv('T2H_GRAPH', graph)
    monkeypatch.setenv('T2H_SHRINK_BATCH', shrink)
    mode = 'graph' if graph == '1' else 'eager'
    for temp in (1.0, TEMPS):                                                    # a scalar, then one value per image
        (lists, want), adv = _run(model.sample_fn, 17, temp=temp, sample_steps=STEPS, return_logp=True)
        assert model.sampler_fn.last_launch_mode == mode
        got, adv_s = _run(model.score_fn, 17, lists, temp=temp, sample_steps=STEPS)
        assert model.sampler_fn.last_launch_mode == mode
        assert got.dtype == torch.float32 and tuple(got.shape) == (B, T)
        assert adv_s == adv and _bytes(got) == _bytes(want), temp
        (got_r, rank), adv_r = _run(model.score_fn, 17, lists, temp=temp, sample_steps=STEPS, return_rank=True)
        assert adv_r == adv and _bytes(got_r) == _bytes(want), temp              # return_rank changes neither
        assert rank.dtype == torch.int32 and tuple(rank.shape) == (B, T)
        assert bool((rank >= 0).all()) and bool((rank < N_CLASS).all())
        # the two outputs speak of the same rows: rank + 1 classes are at least as likely as the token, so its
        # probability is at most 1 / (rank + 1) (up to the float32 error of the value, 8 x ~1.2e-6)
        assert bool((got_r <= -torch.log(rank.float() + 1) + 1e-5).all())
    assert bool(torch.isfinite(want).all()) and float(want.std()) > 0.2


def _edit_keep():
    """the keep pattern of tests/test_gpu_logp.py: image 0 resamples 3 rows (and leaves the batch first), image 1
    everything, image 2 every other row"""
    keep = torch.zeros(B, T, dtype=torch.uint8)
    keep[0] = 1
    keep[0, [5, 200, 411]] = 0
    keep[2, ::2] = 1
    return keep


@pytest.mark.parametrize('graph', ['1', '0'])
def test_a_region_edit_scores_the_bits_of_the_rows_it_drew(model, monkeypatch, graph):
    monkeypatch.setenv('T2H_GRAPH', graph)
    monkeypatch.setenv('T2H_SHRINK_BATCH', '1')
    src, _ = _run(model.sample_fn, 23, sample_steps=STEPS)
    keep = _edit_keep()
    (edited, want), adv = _run(model.resample_fn, 29, src, keep, sample_steps=STEPS, return_logp=True)
    (got, rank), adv_s = _run(model.score_fn, 29, edited, keep=keep, sample_steps=STEPS, return_rank=True)
    k = keep.bool().to(got.device)
    assert adv_s == adv and _bytes(got[~k]) == _bytes(want[~k])
    assert bool(torch.isfinite(got[~k]).all()) and bool((rank[~k] >= 0).all())
    assert bool(torch.isnan(got[k]).all()) and bool((rank[k] == -1).all())      # given, not scored
    assert int(torch.isfinite(got[0]).sum()) == 3


def _random_map(seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, N_CLASS, (18, B * T), generator=g)                   # valid under every texture


def _hooked_score(model, seed, targets, temp):
    """the eager loop with a round_hook -> (logp, rank, [(x_t before the round, x_t after it)], segm, tex_tok)"""
    net, states = model.sampler_fn, []
    tex_tok = model._texture_tokens(model.texture_mask)
    segm = model.segm_tokens.contiguous()
    prev = [torch.full((B, T), model.mask_id, dtype=torch.int64, device=segm.device)]

    def hook(r, steps, x_t, out):
        states.append((prev[0], x_t.clone()))
        prev[0] = x_t.clone()

    seed_all(seed)
    logp, rank = engine.score_tokens(net, segm, tex_tok, STEPS, model.mask_id, targets.to(segm.device), temp=temp,
                                     round_hook=hook, return_rank=True)
    assert net.last_launch_mode == 'eager'
    return logp, rank, states, segm, tex_tok


@pytest.fixture(scope='module')
def arbitrary(model):
    """a map the model did not draw, scored by the hooked eager loop, and its float64 recomputation from the state every
    round started from: dict(targets, logp, rank, want float64 [B*T], f32 = the float32 yardstick of those rows)"""
    temp = 1.0
    targets = _random_map(5)
    logp, rank, states, segm, tex_tok = _hooked_score(model, 17, targets, temp)
    net = model.sampler_fn
    dev = logp.device
    want = torch.full((B * T, ), float('nan'), dtype=torch.float64, device=dev)
    want_rank = torch.full((B * T, ), -1, dtype=torch.int64, device=dev)
    near = torch.zeros(B * T, dtype=torch.int64, device=dev)
    window = 2 * ACT_TOL * HEAD_SCALE / temp                                     # both logits of a comparison move
    f32 = 0.0
    tex = tex_tok.view(-1)
    tg = targets.to(dev)
    for before, after in states:
        scored = ((before != model.mask_id) != (after != model.mask_id)).view(-1).nonzero().view(-1)
        if scored.numel() == 0:
            continue
        hs = set(tex[scored].tolist())
        lg = net.logits(before, segm, tex_tok, heads=hs)
        for h in hs:
            rows = scored[tex[scored] == h]
            tok = tg[h, rows]
            assert torch.equal(after.view(-1)[rows], tok + N_CLASS * h)          # the loop fed the TARGETS back
            l32 = lg[h].view(B * T, -1)[rows] / temp
            lp = torch.log_softmax(l32.double(), -1).gather(1, tok[:, None])[:, 0]
            lp32 = torch.log_softmax(l32, -1).gather(1, tok[:, None])[:, 0]
            f32 = max(f32, float((lp32.double() - lp).abs().max()))
            want[rows] = lp
            lt = l32.gather(1, tok[:, None])
            want_rank[rows] = (l32 > lt).sum(1)
            near[rows] = ((l32 - lt).abs() <= window).sum(1) - 1                  # (the target itself is one of them)
    assert bool(torch.isfinite(want).all())                                      # every row was scored in some round
    return dict(targets=targets, temp=temp, logp=logp, rank=rank, want=want, want_rank=want_rank, near=near, f32=f32)


def test_an_arbitrary_map_against_float64(arbitrary):
    a = arbitrary
    allowed = allowance(a['temp'], a['f32'])
    err = float((a['logp'].double() - a['want']).abs().max())
    print(f'score of a random map vs float64: max abs err {err:.3e}, allowed {allowed:.3e} (float32 yardstick of these '
          f'rows {a["f32"]:.3e}), spread {float(a["want"].std()):.3f}')
    assert err <= allowed, err
    assert float(a['want'].std()) >= 100 * allowed                               # the check cannot pass on a constant
    # rank is a count of exact comparisons on logits that move by ACT_TOL * head_scale / temp between two evaluations:
    # it may differ from the recomputation's count by no more than the classes whose logit lies within twice that of
    # the target's (`near`, counted per row on the recomputed logits)
    off = (a['rank'].long() - a['want_rank']).abs()
    print(f'rank vs the recomputation: {int((off == 0).sum())} of {off.numel()} equal, max difference {int(off.max())}; '
          f'classes near the target per row: mean {float(a["near"].float().mean()):.2f}, max {int(a["near"].max())}')
    assert bool((a['rank'] >= 0).all()) and bool((off <= a['near']).all())
    assert float(a['want_rank'].float().std()) > 100 and float(a['near'].float().mean()) < 2   # ... which binds


def test_graph_and_eager_agree(model, monkeypatch, arbitrary):
    a = arbitrary
    lists = [a['targets'][h].view(B, T) for h in range(18)]
    allowed = allowance(a['temp'], a['f32'])
    res = {}
    for graph in ('1', '0'):
        monkeypatch.setenv('T2H_GRAPH', graph)
        res[graph], _ = _run(model.score_fn, 17, lists, temp=a['temp'], sample_steps=STEPS)
        assert model.sampler_fn.last_launch_mode == ('graph' if graph == '1' else 'eager')
    err = float((res['1'].double() - res['0'].double()).abs().max())
    err_h = float((res['1'].double().view(-1) - a['want']).abs().max())
    print(f'graph vs eager score: max abs diff {err:.3e}; graph vs float64 {err_h:.3e}; allowed {allowed:.3e}')
    assert err <= allowed and err_h <= allowed


def test_image_b_of_a_batch_has_the_bits_of_its_scalar_call_and_the_summary_is_the_existing_one(model, arbitrary):
    lists = [arbitrary['targets'][h].view(B, T) for h in range(18)]
    (logp, (s, c, m)), adv = _run(model.score_fn, 17, lists, temp=TEMPS, sample_steps=STEPS, summary=True)
    assert model.sampler_fn.last_launch_mode == 'graph'
    ws, wc, wm = ops.logp_summary(logp.contiguous())
    assert _bytes(s) == _bytes(ws) and _bytes(c) == _bytes(wc) and _bytes(m) == _bytes(wm)
    assert c.tolist() == [T] * B
    for b in range(B):
        want, adv_b = _run(model.score_fn, 17, lists, temp=TEMPS[b], sample_steps=STEPS)
        assert adv_b == adv and _bytes(logp[b]) == _bytes(want[b]), b
        if b:   # ... and its own value matters: another image's scalar call gives this image other numbers
            assert not torch.equal(logp[b - 1], want[b - 1]), b
    # all three outputs at once, in the documented order
    (lp3, rk3, sm3), _ = _run(model.score_fn, 17, lists, temp=TEMPS, sample_steps=STEPS, return_rank=True, summary=True)
    assert _bytes(lp3) == _bytes(logp) and rk3.dtype == torch.int32 and _bytes(sm3[0]) == _bytes(s)


@pytest.mark.parametrize('graph', ['1', '0'])
def test_a_target_out_of_range_raises_before_the_generator_moves(model, monkeypatch, arbitrary, graph):
    monkeypatch.setenv('T2H_GRAPH', graph)
    tex = model._texture_tokens(model.texture_mask).view(-1).cpu()
    for bad, (b, t) in ((N_CLASS, (2, 77)), (-1, (1, 0))):
        targets = arbitrary['targets'].clone()
        targets[int(tex[b * T + t]), b * T + t] = bad
        targets[int(tex[2 * T + 300]), 2 * T + 300] = -1                         # a later offender: the FIRST is named
        seed_all(3)
        off0 = _gen().get_offset()
        with pytest.raises(_lib.T2HError, match=f'token row {t} of sample {b}'):
            model.score_fn([targets[h].view(B, T) for h in range(18)], sample_steps=STEPS)
        assert _gen().get_offset() == off0
    # an entry outside the range under ANOTHER texture is never read
    targets = arbitrary['targets'].clone()
    other = (int(tex[5]) + 1) % 18
    targets[other, 5] = -1
    got, _ = _run(model.score_fn, 17, [targets[h].view(B, T) for h in range(18)], sample_steps=STEPS)
    assert bool(torch.isfinite(got).all())


def test_callers_that_do_not_score_keep_their_tokens_keys_and_captures(model, monkeypatch, arbitrary):
    monkeypatch.setenv('T2H_GRAPH', '1')
    net = model.sampler_fn
    kinds = (engine.SCORE, engine.SCORE_RANK)
    want, _ = _run(model.sample_fn, 17, sample_steps=STEPS)                      # a seed the tests above used
    plain_keys = {k for k in net._graphs if k[-1] not in kinds}
    captured = {k: dict(net._graphs[k].graphs) for k in plain_keys}
    lists = [arbitrary['targets'][h].view(B, T) for h in range(18)]
    _run(model.score_fn, 17, lists, sample_steps=STEPS, return_rank=True)
    _run(model.score_fn, 17, lists, temp=TEMPS, sample_steps=STEPS)
    score_keys = {k for k in net._graphs if k[-1] in kinds}
    assert score_keys and any(k[:-1] in plain_keys for k in score_keys)          # the plain key + one trailing element
    assert {k for k in net._graphs if k[-1] not in kinds} == plain_keys          # scoring added no other key
    n_graphs = len(net._graphs)
    again, _ = _run(model.sample_fn, 17, sample_steps=STEPS)
    assert torch.equal(torch.stack(again), torch.stack(want))
    assert len(net._graphs) == n_graphs
    for k in plain_keys:   # the very captures, not new ones under the old keys
        assert net._graphs[k].targets is None and net._graphs[k].rank is None
        assert all(net._graphs[k].graphs[c] is g for c, g in captured[k].items())
    for k in score_keys:
        assert net._graphs[k].targets is not None and net._graphs[k].logp is not None
        assert (net._graphs[k].rank is not None) == (k[-1] == engine.SCORE_RANK)
