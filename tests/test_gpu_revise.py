"""Self-correction on the GPU (-m gpu): the pseudo-likelihood critic pll_fn and the revise loop.

1. definition: on the rows of fold k, pll_fn is score_fn(map, keep=keep_k[k], temp, sample_steps=1) within the
   project's bound for two evaluations whose kernel forms may differ (tests/test_gpu_score.py's allowance);
2. value: against a float64 recomputation from the hidden state of every fold's masked input;
3. determinism: same bytes twice, the generator neither read nor advanced;
4. composition: revise_fn is, byte for byte, the loop this file composes from the public pll_fn, the numpy selection of
   tests/revise_ref.py on pll_fn's own float32 output, resample_fn and the accept rule;
5. the guarantee of accept='improve', and that the rule binds;
6. seeds: an image of a batch is the single-image call with its seed;
7. the entry point.
No statement about image quality is made or tested: the weights are synthetic."""
import numpy as np
import pytest
import torch

from text2human_amd import _lib, ops, options, synthetic, defaults
from text2human_amd.models import SampleFromParsingModel

import logp_ref  # noqa: E402
import revise_ref as ref  # noqa: E402
from parity_util import ACT_TOL, seed_all  # noqa: E402
from test_gpu_score import B, HEAD_SCALE, N_CLASS, STEPS, T, TEMPS, _bytes, _gen, _random_map, allowance  # noqa: E402

pytestmark = pytest.mark.gpu
TH, TW = 32, 16
BATCH = synthetic.parsing_batch(B, seed=91)                                      # the fixture of tests/test_gpu_score.py


@pytest.fixture(scope='module')
def opt():
    return options.dict_to_nonedict(defaults.sample_from_parsing())


@pytest.fixture(scope='module')
def model(opt):
    m = SampleFromParsingModel(opt, state_dicts=synthetic.make_state_dicts(opt, seed=1234, head_scale=HEAD_SCALE))
    m.feed_data(BATCH)
    return m


@pytest.fixture(scope='module')
def drawn(model):
    """a map the sampler drew: 18 x int64 [B, T]"""
    model.feed_data(BATCH)
    seed_all(23)
    return model.sample_fn(sample_steps=STEPS)


@pytest.fixture(scope='module')
def arbitrary():
    """a map the model did not draw (valid under every texture): 18 x int64 [B, T]"""
    t = _random_map(5)
    return [t[h].view(B, T) for h in range(18)]


def _fold_rows(K):
    """bool [K, B * T] on the host: the rows of every fold"""
    f = np.tile(ref.fold_map(TH, TW, K), B)
    return torch.from_numpy(np.stack([f == k for k in range(K)]))


def _recompute(model, lists, K, hidden=False):
    """float32 logits [B*T, N_CLASS] (before the temperature) of every row's own head from the evaluation of ITS fold's
    masked input, the tokens [B*T], and with hidden=True the hidden state [B*T, C] put together the same way"""
    net, dev = model.sampler_fn, model.device
    tex_tok = model._texture_tokens(model.texture_mask)
    segm, tex = model.segm_tokens.contiguous(), tex_tok.view(-1)
    tg = torch.stack([x.reshape(-1) for x in lists]).to(dev)
    tok = tg[tex, torch.arange(B * T, device=dev)]
    full = (tok + N_CLASS * tex).view(B, T)
    folds = _fold_rows(K).to(dev)
    logits = torch.empty((B * T, N_CLASS), dtype=torch.float32, device=dev)
    hid = torch.empty((B * T, net.desc['C']), dtype=torch.float32, device=dev) if hidden else None
    for k in range(K):
        rows = folds[k].nonzero().view(-1)
        x_t = torch.where(folds[k].view(B, T), torch.full_like(full, model.mask_id), full)
        if hidden:
            hid[rows] = net.hidden(x_t, segm, tex_tok)[rows]
        hs = set(tex[rows].tolist())
        lg = net.logits(x_t, segm, tex_tok, heads=hs)
        for h in hs:
            rh = rows[tex[rows] == h]
            logits[rh] = lg[h].view(B * T, -1)[rh]
    return logits, tok, hid


def _yardsticks(logits, tok, temp_rows):
    """from recomputed logits: (want float64 [n], f32 yardstick, want_rank, near) at the per-row temperature"""
    l32 = logits / temp_rows[:, None]
    want = torch.log_softmax(l32.double(), -1).gather(1, tok[:, None])[:, 0]
    lp32 = torch.log_softmax(l32, -1).gather(1, tok[:, None])[:, 0]
    f32 = float((lp32.double() - want).abs().max())
    lt = l32.gather(1, tok[:, None])
    window = (2 * ACT_TOL * HEAD_SCALE / temp_rows)[:, None]                      # both logits of a comparison move
    return want, f32, (l32 > lt).sum(1), ((l32 - lt).abs() <= window).sum(1) - 1


def _temp_rows(temp, dev):
    t = torch.tensor(temp if isinstance(temp, list) else [temp] * B, dtype=torch.float32, device=dev)
    return t.repeat_interleave(T)


# ---- 1. definition
@pytest.mark.parametrize('graph', ['1', '0'])
@pytest.mark.parametrize('K,ks', [(4, range(4)), (2, range(2)), (16, (0, 9))])   # (16 folds at B = 3: K calls at batch B)
def test_pll_is_the_one_step_score_of_every_fold(model, drawn, monkeypatch, graph, K, ks):
    monkeypatch.setenv('T2H_GRAPH', graph)
    model.feed_data(BATCH)
    dev = model.device
    assert options.pll_batched(B, K) is (K != 16)
    logits, tok, _ = _recompute(model, drawn, K)
    folds = _fold_rows(K).to(dev)
    keep_k = ops.fold_keep(K, B, (TH, TW), device=dev)
    assert _bytes(keep_k) == ref.fold_keep(K, B, TH, TW).tobytes()
    for temp in (1.0, TEMPS):
        tr = _temp_rows(temp, dev)
        want, f32, want_rank, near = _yardsticks(logits, tok, tr)
        allowed = allowance(tr, f32)                                             # per row: its own temperature
        pll, rank = model.pll_fn(drawn, folds=K, temp=temp, return_rank=True)
        assert pll.dtype == torch.float32 and tuple(pll.shape) == (B, T) and rank.dtype == torch.int32
        assert bool(torch.isfinite(pll).all()) and bool((rank >= 0).all())
        worst = 0.0
        for k in ks:
            seed_all(41 + k)
            sc, sr = model.score_fn(drawn, keep=keep_k[k], temp=temp, sample_steps=1, return_rank=True)
            rows = folds[k]
            assert bool(torch.isnan(sc.view(-1)[~rows]).all()) and bool(torch.isfinite(sc.view(-1)[rows]).all())
            err = (pll.view(-1)[rows].double() - sc.view(-1)[rows].double()).abs()
            worst = max(worst, float((err / allowed[rows]).max()))
            assert bool((err <= allowed[rows]).all()), (K, k, temp, float(err.max()))
            for r in (rank, sr):
                assert bool(((r.view(-1)[rows].long() - want_rank[rows]).abs() <= near[rows]).all()), (K, k, temp)
        print(f'pll_fn vs one-step score_fn, folds {K}, temp {temp}, T2H_GRAPH={graph}: worst error / allowance '
              f'{worst:.3f} (float32 yardstick {f32:.3e}); classes near the target per row: mean '
              f'{float(near.float().mean()):.2f}; spread of the values {float(want.std()):.3f}')


def _keep_pattern():
    """image 0 keeps all but 3 rows, image 1 nothing, image 2 every other row"""
    keep = torch.zeros(B, T, dtype=torch.uint8)
    keep[0] = 1
    keep[0, [5, 200, 411]] = 0
    keep[2, ::2] = 1
    return keep


def test_caller_kept_rows_are_given_not_scored(model, drawn):
    model.feed_data(BATCH)
    keep = _keep_pattern()
    k = keep.bool().to(model.device)
    pll, rank, (s, c, mn) = model.pll_fn(drawn, keep=keep, return_rank=True, summary=True)
    assert bool(torch.isnan(pll[k]).all()) and bool((rank[k] == -1).all())
    assert bool(torch.isfinite(pll[~k]).all()) and bool((rank[~k] >= 0).all())
    assert c.tolist() == [3, T, T // 2]
    ws, wc, wm = ops.logp_summary(pll.contiguous())
    assert _bytes(s) == _bytes(ws) and _bytes(c) == _bytes(wc) and _bytes(mn) == _bytes(wm)
    # on the rows of fold 0: the one-step score with fold 0 AND the caller's rows kept
    keep_k = ops.fold_keep(4, B, (TH, TW), keep.to(model.device).reshape(-1).contiguous())
    assert _bytes(keep_k) == ref.fold_keep(4, B, TH, TW, keep.numpy()).tobytes()
    sc = model.score_fn(drawn, keep=keep_k[0], sample_steps=1)
    rows = (keep_k[0] == 0)
    logits, tok, _ = _recompute(model, drawn, 4)
    _, f32, _, _ = _yardsticks(logits, tok, _temp_rows(1.0, model.device))
    assert float((pll[rows].double() - sc[rows].double()).abs().max()) <= allowance(1.0, f32)


def test_a_token_without_an_index_raises_and_nothing_is_evaluated(model, arbitrary):
    model.feed_data(BATCH)
    tex = model._texture_tokens(model.texture_mask).view(-1).cpu()
    t = torch.stack([x.reshape(-1) for x in arbitrary]).clone()
    t[int(tex[2 * T + 77]), 2 * T + 77] = N_CLASS
    t[int(tex[2 * T + 300]), 2 * T + 300] = -1                                   # a later offender: the FIRST is named
    seed_all(3)
    off0 = _gen().get_offset()
    for fn in (model.pll_fn, model.revise_fn):
        calls = _lib.n_calls
        with pytest.raises(_lib.T2HError, match='token row 77 of sample 2'):
            fn([t[h].view(B, T) for h in range(18)])
        assert _lib.n_calls - calls <= 2                                         # the check itself; no transformer launch
    assert _gen().get_offset() == off0


# ---- 2. value
def test_an_arbitrary_map_against_float64(model, arbitrary):
    model.feed_data(BATCH)
    temp, K = 1.0, 4
    pll = model.pll_fn(arbitrary, folds=K, temp=temp)
    _, tok, hid = _recompute(model, arbitrary, K, hidden=True)
    net = model.sampler_fn
    g, bt, w = (x.cpu() for x in net.final_norm_and_heads())
    hid, tok = hid.cpu(), tok.cpu()
    tex = model._texture_tokens(model.texture_mask).view(-1).cpu()
    want, f32 = np.empty(B * T), 0.0
    for h in sorted(set(tex.tolist())):                                          # (per head: one weight matrix at a time)
        rows = (tex == h).nonzero().view(-1).numpy()
        want[rows] = logp_ref.row_logp(hid, g, bt, w, tex, rows, tok[rows].numpy(), temp)
        f32 = max(f32, logp_ref.f32_error(hid, g, bt, w, tex, rows, tok[rows].numpy(), temp))
    allowed = allowance(temp, f32)
    err = float(np.abs(pll.double().cpu().numpy().reshape(-1) - want).max())
    print(f'pll_fn of a random map vs float64: max abs err {err:.3e}, allowed {allowed:.3e} (float32 yardstick of these '
          f'rows {f32:.3e}), spread {want.std():.3f}')
    assert err <= allowed, err
    assert want.std() >= 100 * allowed                                           # the check cannot pass on a constant


# ---- 3. determinism
def test_two_calls_return_the_same_bytes_and_the_generator_is_not_touched(model, drawn):
    model.feed_data(BATCH)
    seed_all(7)
    torch.rand(5, device=model.device)                                           # (a nonzero offset)
    seed0, off0 = _gen().initial_seed(), _gen().get_offset()
    a = model.pll_fn(drawn, temp=TEMPS, return_rank=True)
    assert (_gen().initial_seed(), _gen().get_offset()) == (seed0, off0)
    b = model.pll_fn(drawn, temp=TEMPS, return_rank=True)
    assert _bytes(a[0]) == _bytes(b[0]) and _bytes(a[1]) == _bytes(b[1])
    seed_all(123456)                                                             # another generator state: the same result
    torch.rand(4099, device=model.device)
    off1 = _gen().get_offset()
    c = model.pll_fn(drawn, temp=TEMPS, return_rank=True)
    assert _bytes(a[0]) == _bytes(c[0]) and _bytes(a[1]) == _bytes(c[1]) and _gen().get_offset() == off1
    # the sampler's captured rounds are still the ones it had: the critic works in buffers of its own
    seed_all(23)
    again = model.sample_fn(sample_steps=STEPS)
    assert torch.equal(torch.stack(again), torch.stack(drawn))


# ---- 4. composition
def _compose(model, lists, seed, passes, fraction=None, count=None, keep=None, accept='improve', folds=4, seeds=None):
    """revise_fn put together from the public pieces -> (tokens [18, B, T] on the host, trace, generator advance)"""
    b = model.batch_size
    seed_all(seed)
    off0 = _gen().get_offset()
    cur = torch.stack(lists).cpu().clone()
    as_lists = lambda t: [t[h] for h in range(18)]
    cur_pll, (cur_sum, _, _) = model.pll_fn(as_lists(cur), keep=keep, folds=folds, summary=True)
    cur_pll, cur_sum = cur_pll.cpu(), cur_sum.cpu()
    eligible = [T] * b if keep is None else (T - (keep != 0).sum(1)).tolist()
    m = ref.row_counts(eligible, fraction, count)
    trace = []
    for p in range(passes):
        if not any(m):
            trace.append(dict(selected=np.zeros((b, T), np.uint8), sum_before=cur_sum.numpy(), sum_after=cur_sum.numpy(),
                              accepted=np.full(b, accept == 'always')))
            continue
        sel_keep, n_sel = ref.select_lowest(cur_pll.numpy(), m)
        assert n_sel.tolist() == m
        kw = {} if seeds is None else dict(seeds=[(s + p) % (1 << 64) for s in seeds])
        cand = torch.stack(model.resample_fn(as_lists(cur), torch.from_numpy(sel_keep), sample_steps=STEPS, **kw)).cpu()
        cand_pll, (cand_sum, _, _) = model.pll_fn(as_lists(cand), keep=keep, folds=folds, summary=True)
        cand_pll, cand_sum = cand_pll.cpu(), cand_sum.cpu()
        take = torch.from_numpy(ref.accept(cand_sum.numpy(), cur_sum.numpy(), accept))
        trace.append(dict(selected=1 - sel_keep, sum_before=cur_sum.numpy(), sum_after=cand_sum.numpy(),
                          accepted=take.numpy()))
        cur = torch.where(take[None, :, None], cand, cur)
        cur_pll = torch.where(take[:, None], cand_pll, cur_pll)
        cur_sum = torch.where(take, cand_sum, cur_sum)
    return cur, trace, _gen().get_offset() - off0


def _same_trace(got, want):
    assert len(got) == len(want)
    for p, (g, w) in enumerate(zip(got, want)):
        assert g['selected'].dtype == torch.uint8 and g['accepted'].dtype == torch.bool
        assert g['sum_before'].dtype == torch.float32 and g['sum_after'].dtype == torch.float32
        assert np.array_equal(g['selected'].cpu().numpy(), w['selected']), p
        assert g['sum_before'].cpu().numpy().tobytes() == w['sum_before'].tobytes(), p
        assert g['sum_after'].cpu().numpy().tobytes() == w['sum_after'].tobytes(), p
        assert g['accepted'].cpu().numpy().tolist() == w['accepted'].tolist(), p


def _revise(model, lists, seed, **kw):
    seed_all(seed)
    off0 = _gen().get_offset()
    out, trace = model.revise_fn(lists, sample_steps=STEPS, return_trace=True, **kw)
    return torch.stack(out).cpu(), trace, _gen().get_offset() - off0


def test_revise_is_the_composition_of_its_public_pieces(model, drawn):
    model.feed_data(BATCH)
    want, want_trace, want_adv = _compose(model, drawn, 31, passes=2, fraction=0.25)
    got, trace, adv = _revise(model, drawn, 31, passes=2, fraction=0.25)
    assert torch.equal(got, want) and adv == want_adv and adv > 0
    _same_trace(trace, want_trace)
    assert all(int(t['selected'][b].sum()) == 128 for t in trace for b in range(B))
    plain = model.revise_fn(drawn, passes=2, sample_steps=STEPS)                 # without the trace: the lists alone
    assert isinstance(plain, list) and len(plain) == 18 and tuple(plain[0].shape) == (B, T) and plain[0].dtype == torch.int64


def test_revise_with_counts_and_kept_rows_is_the_composition(model, drawn):
    model.feed_data(BATCH)
    keep = torch.zeros(B, T, dtype=torch.uint8)
    keep[2, ::2] = 1                                                             # every other row of image 2 is fixed
    count = [3, 0, 512]
    want, want_trace, want_adv = _compose(model, drawn, 37, passes=2, count=count, keep=keep)
    got, trace, adv = _revise(model, drawn, 37, passes=2, count=count, keep=keep)
    assert torch.equal(got, want) and adv == want_adv
    _same_trace(trace, want_trace)
    src = torch.stack(drawn).cpu()
    assert torch.equal(got[:, 1], src[:, 1])                                     # count 0: image 1 returns its input
    for t in trace:
        assert [int(t['selected'][b].sum()) for b in range(B)] == [3, 0, 256]
        assert not bool(t['selected'].cpu()[keep.bool()].any())                  # caller-kept rows are never selected
    assert torch.equal(got[:, 2, ::2], src[:, 2, ::2])
    # nothing to redo anywhere: no resample_fn call, the generator does not move, the input comes back
    got0, trace0, adv0 = _revise(model, drawn, 37, passes=2, count=0)
    assert torch.equal(got0, src) and adv0 == 0 and not any(bool(t['selected'].any()) for t in trace0)


# ---- 5. the guarantee
def _sums(model, lists, **kw):
    return model.pll_fn(lists, summary=True, **kw)[1][0].cpu()


def test_improve_never_lowers_the_critics_sum_and_the_rule_binds(model, drawn):
    model.feed_data(BATCH)
    src = torch.stack(drawn).cpu()
    before = _sums(model, drawn)
    out, trace, _ = _revise(model, drawn, 43, passes=3, fraction=0.25, accept='improve')
    after = _sums(model, [out[h] for h in range(18)])
    print(f'pll sums before {before.tolist()} after 3 improve passes {after.tolist()}; accepted per pass '
          f'{[t["accepted"].tolist() for t in trace]}')
    assert bool((after >= before).all())                                         # (floats, no tolerance: one function, twice)
    cur = src.clone()
    for p, t in enumerate(trace):
        sb, sa, acc = t['sum_before'].cpu(), t['sum_after'].cpu(), t['accepted'].cpu()
        assert acc.tolist() == (sa > sb).tolist(), p
        if p:
            prev = trace[p - 1]
            want_sb = torch.where(prev['accepted'].cpu(), prev['sum_after'].cpu(), prev['sum_before'].cpu())
            assert _bytes(sb) == _bytes(want_sb), p
    assert _bytes(trace[0]['sum_before']) == _bytes(before)
    last = trace[-1]
    assert _bytes(torch.where(last['accepted'], last['sum_after'], last['sum_before'])) == _bytes(after)
    # rows outside `selected` are unchanged in every pass: all changes of the result lie in the union of the accepted
    # passes' selections
    allowed_rows = torch.zeros(B, T, dtype=torch.bool)
    for t in trace:
        allowed_rows |= (t['selected'].cpu() != 0) & t['accepted'].cpu()[:, None]
    changed = (out != src).any(0)
    assert not bool((changed & ~allowed_rows).any())
    one, trace_1, _ = _revise(model, drawn, 43, passes=1, fraction=0.25, accept='always')
    assert not bool(((one != src).any(0) & (trace_1[0]['selected'].cpu() == 0)).any())


def test_always_takes_what_improve_rejects(model, drawn):
    """Redrawing the least likely quarter of this drawn map raises the critic's sum in each of the first four passes for
    every generator seed 40 .. 51 (the first worse candidates come in passes five and six), so no choice of seed makes a
    three-pass run at fraction 0.25 exercise the rule.  It is exercised where a candidate is as often worse as better:
    fraction = 1 -- all rows re-masked, the candidate is a fresh sample.  Seed 47: passes 2 and 3 hold worse candidates
    under 'always'."""
    model.feed_data(BATCH)
    before = _sums(model, drawn)
    out_a, trace_a, adv_a = _revise(model, drawn, 47, passes=3, fraction=1.0, accept='always')
    worse = [(p, b) for p, t in enumerate(trace_a) for b in range(B)
             if not float(t['sum_after'][b]) > float(t['sum_before'][b])]
    print(f'accept=always, fraction 1: (pass, image) that improve would have rejected: {worse}; sums per pass '
          f'{[t["sum_after"].tolist() for t in trace_a]} from {before.tolist()}')
    assert all(bool(t['accepted'].all()) and bool(t['selected'].all()) for t in trace_a)
    assert worse, 'no candidate of this fixture was worse than its map: the rule was not exercised'
    for p, t in enumerate(trace_a[:-1]):
        assert _bytes(trace_a[p + 1]['sum_before']) == _bytes(t['sum_after'])
    assert _bytes(_sums(model, [out_a[h] for h in range(18)])) == _bytes(trace_a[-1]['sum_after'])
    # the same seed under 'improve': the first candidate does not depend on the rule, and exactly the images whose
    # candidate was not better keep their map; the sums never fall
    out_i, trace_i, adv_i = _revise(model, drawn, 47, passes=3, fraction=1.0, accept='improve')
    assert _bytes(trace_i[0]['sum_after']) == _bytes(trace_a[0]['sum_after'])
    rejected = [b for b in range(B) if (0, b) in worse]
    assert [b for b in range(B) if not bool(trace_i[0]['accepted'][b])] == rejected
    assert any(not bool(t['accepted'].all()) for t in trace_i)
    after = _sums(model, [out_i[h] for h in range(18)])
    assert bool((after >= before).all())
    src = torch.stack(drawn).cpu()
    for b in range(B):
        if not any(bool(t['accepted'][b]) for t in trace_i):
            assert torch.equal(out_i[:, b], src[:, b]) and float(after[b]) == float(before[b])


# ---- 6. seeds
def _sub(batch, idx):
    return {k: (v[idx] if torch.is_tensor(v) else [v[i] for i in idx]) for k, v in batch.items()}


def test_with_seeds_an_image_is_its_single_image_call(model, drawn):
    seeds = [5, (1 << 64) - 1, 77]                                               # (image 1: pass 1 wraps to seed 0)
    model.feed_data(BATCH)
    seed_all(3)
    torch.rand(3, device=model.device)
    state = (_gen().initial_seed(), _gen().get_offset())
    out, trace = model.revise_fn(drawn, passes=2, fraction=0.25, sample_steps=STEPS, seeds=seeds, return_trace=True)
    assert (_gen().initial_seed(), _gen().get_offset()) == state                 # the global generator is untouched
    got = torch.stack(out).cpu()
    want_pll = model.pll_fn(drawn).cpu()
    try:
        for b in range(B):
            model.feed_data(_sub(BATCH, [b]))
            alone = [x[b:b + 1] for x in drawn]
            o1, t1 = model.revise_fn(alone, passes=2, fraction=0.25, sample_steps=STEPS, seeds=[seeds[b]],
                                     return_trace=True)
            assert torch.equal(torch.stack(o1).cpu()[:, 0], got[:, b]), b
            for p in range(2):
                for key in ('selected', 'sum_before', 'sum_after', 'accepted'):
                    assert _bytes(t1[p][key][0]) == _bytes(trace[p][key][b]), (b, p, key)
            assert _bytes(model.pll_fn(alone)[0]) == _bytes(want_pll[b]), b       # the critic itself: batch-independent
    finally:
        model.feed_data(BATCH)
    assert (_gen().initial_seed(), _gen().get_offset()) == state
    want, want_trace, _ = _compose(model, drawn, 3, passes=2, fraction=0.25, seeds=seeds)
    assert torch.equal(got, want)
    _same_trace(trace, want_trace)
    assert not torch.equal(got, torch.stack(drawn).cpu())
    with pytest.raises(ValueError, match='per-image seeds are not supported'):
        model.revise_fn(drawn, order='confidence', seeds=seeds)


# ---- 7. the entry point
def test_sample_and_refine_revises_what_it_sampled(model, monkeypatch, tmp_path):
    model.feed_data(BATCH)
    seen = []
    real = model.decode_indices

    def spy(top, *a, **k):
        seen.append(torch.stack([x.reshape(B, T) for x in top]).cpu())
        return real(top, *a, **k)

    monkeypatch.setattr(model, 'decode_indices', spy)
    monkeypatch.setattr(model, 'sample_steps', STEPS)
    names = [f'{i}.png' for i in range(B)]

    def run(tag, **keys):
        for k in ('revise_passes', 'revise_fraction', 'revise_folds'):
            model.opt.pop(k, None)
        model.opt.update(keys)
        d = tmp_path / tag
        d.mkdir()
        seed_all(53)
        off0 = _gen().get_offset()
        try:
            model.sample_and_refine(str(d), names)
        finally:
            for k in keys:
                model.opt.pop(k, None)
        assert sorted(p.name for p in d.iterdir()) == names
        return seen[-1], _gen().get_offset() - off0

    got, adv = run('revised', revise_passes=1)
    seed_all(53)
    off0 = _gen().get_offset()
    sampled = model.sample_fn(temp=1, sample_steps=STEPS)
    want = torch.stack(model.revise_fn(sampled, passes=1, fraction=0.25, folds=4, temp=1, sample_steps=STEPS)).cpu()
    assert torch.equal(got, want) and adv == _gen().get_offset() - off0
    assert not torch.equal(got, torch.stack(sampled).cpu())
    plain, adv_plain = run('plain')
    zero, adv_zero = run('zero', revise_passes=0)
    assert torch.equal(plain, torch.stack(sampled).cpu()) and torch.equal(zero, plain) and adv_zero == adv_plain
    got8, _ = run('folds8', revise_passes=2, revise_fraction=0.1, revise_folds=8)
    seed_all(53)
    want8 = torch.stack(model.revise_fn(model.sample_fn(temp=1, sample_steps=STEPS), passes=2, fraction=0.1, folds=8,
                                        temp=1, sample_steps=STEPS)).cpu()
    assert torch.equal(got8, want8)
