"""Per-image seeds on the GPU (-m gpu): an image of a seeded call is what the SAME code returns for a batch
that holds that image alone after torch.cuda.manual_seed(its seed) -- tokens and log-probability bits -- whatever else is
in the batch, wherever it sits, and whether or not finished samples leave the batch or rounds are graph replays.  The
oracle is the project's own single-image path, which the existing suites pin against the reference."""
import numpy as np
import pytest
import torch

from text2human_amd import defaults, engine, ops, options, sample_from_parsing, synthetic
from text2human_amd.models import SampleFromParsingModel, sample_model

from parity_util import seed_all  # noqa: E402

pytestmark = pytest.mark.gpu
B, T, STEPS = 3, 512, 16
SEEDS = [20211, (1 << 63) + 77, 5]          # (one above 2^63: a seed is a uint64)
MODES = [('1', '1'), ('1', '0'), ('0', '1'), ('0', '0')]   # (T2H_GRAPH, T2H_SHRINK_BATCH)
DEV = 'cuda'


@pytest.fixture(scope='module')
def opt():
    return options.dict_to_nonedict(defaults.sample_from_parsing())


@pytest.fixture(scope='module')
def sds(opt):
    return synthetic.make_state_dicts(opt, seed=1234)


@pytest.fixture(scope='module')
def model(opt, sds):
    return SampleFromParsingModel(opt, state_dicts=sds)


BATCH = synthetic.parsing_batch(B, seed=91)
OTHERS = synthetic.parsing_batch(B, seed=92)


def _sub(batch, idx):
    return {k: (v[idx] if torch.is_tensor(v) else [v[i] for i in idx]) for k, v in batch.items()}


def _cat(*batches):
    return {k: (torch.cat([b[k] for b in batches]) if torch.is_tensor(batches[0][k]) else sum((b[k] for b in batches), []))
            for k in batches[0]}


def _gen():
    return torch.cuda.default_generators[torch.cuda.current_device()]


def _bits(x):
    return x.contiguous().view(torch.int32)


def _seeded(model, batch, seeds, **kw):
    """-> (tokens int64 [18, b, 512], logp f32 [b, 512], last_seed_offsets) of sample_fn(seeds=, return_logp=True)"""
    model.feed_data(batch)
    lists, logp = model.sample_fn(sample_steps=STEPS, seeds=seeds, return_logp=True, **kw)
    return torch.stack(lists), logp, model.last_seed_offsets.clone()


def _alone(model, batch, b, seed, fn='sample_fn', **kw):
    """image b fed alone, manual_seed(seed), today's call -> (tokens [18, 512], logp [512], generator offset after it)"""
    model.feed_data(_sub(batch, [b]))
    torch.cuda.manual_seed(seed)
    assert _gen().get_offset() == 0
    lists, logp = getattr(model, fn)(sample_steps=STEPS, return_logp=True, **kw)
    return torch.stack(lists)[:, 0], logp[0], _gen().get_offset()


@pytest.fixture(scope='module')
def singles(model):
    """the oracle, computed once: every image of BATCH alone under its own seed (default launch modes)"""
    return [_alone(model, BATCH, b, SEEDS[b]) for b in range(B)]


# ---- 1. the batched schedule kernel against the single one, on the device
@pytest.mark.parametrize('n_img,steps', [(3, 16), (8, 256)])
def test_batched_schedule_kernel_equals_the_single_one(n_img, steps):
    g = torch.Generator().manual_seed(3)
    tex = torch.randint(0, 18, (n_img * T, ), generator=g).to(DEV)
    seeds = [int(s) for s in torch.randint(0, 1 << 62, (n_img, ), generator=g)]
    seeds[0] = (1 << 64) - 1
    step, mask, rand_inc, expo_inc = ops.unmask_schedule(None, 0, tex, steps, 18, 1024, seeds=seeds)
    assert tuple(mask.shape) == (n_img, steps + 1)
    assert (rand_inc, expo_inc) == (ops.torch_draw_geometry(T)[1], ops.torch_draw_geometry(T * 1024)[1])
    keep = (torch.rand(n_img * T, generator=g) < 0.4).to(torch.uint8).to(DEV)
    step_k, mask_k, _, _ = ops.unmask_schedule(None, 0, tex, steps, 18, 1024, keep=keep, seeds=seeds)
    for b in range(n_img):
        sl = slice(b * T, (b + 1) * T)
        ws, wm, _, _ = ops.unmask_schedule(seeds[b], 0, tex[sl].contiguous(), steps, 18, 1024)
        assert torch.equal(step[sl], ws) and torch.equal(mask[b], wm), b
        ws, wm, _, _ = ops.unmask_schedule(seeds[b], 0, tex[sl].contiguous(), steps, 18, 1024, keep=keep[sl].contiguous())
        assert torch.equal(step_k[sl], ws) and torch.equal(mask_k[b], wm), b
    assert int(step.min()) >= 1 and not torch.equal(step[:T], step[T:2 * T])


# ---- 2. each image equals its own single-image call
@pytest.mark.parametrize('graph,shrink', MODES)
def test_each_image_equals_its_own_single_image_call(model, singles, monkeypatch, graph, shrink):
    monkeypatch.setenv('T2H_GRAPH', graph)
    monkeypatch.setenv('T2H_SHRINK_BATCH', shrink)
    tok, logp, offs = _seeded(model, BATCH, SEEDS)
    assert model.sampler_fn.last_launch_mode == ('graph' if graph == '1' else 'eager')
    assert offs.dtype == torch.int64 and tuple(offs.shape) == (B, )
    for b in range(B):
        want_tok, want_logp, want_off = singles[b]
        diff = (tok[:, b] != want_tok).any(0).nonzero().flatten().tolist()
        assert not diff, f'image {b}: token rows {diff[:8]} differ from the single-image call'
        assert torch.equal(_bits(logp[b]), _bits(want_logp)), b
        assert int(offs[b]) == want_off, (b, int(offs[b]), want_off)
    # and the single-image oracle itself does not depend on the launch mode
    got = _alone(model, BATCH, 1, SEEDS[1])
    assert torch.equal(got[0], singles[1][0]) and torch.equal(_bits(got[1]), _bits(singles[1][1])) and got[2] == singles[1][2]


# ---- 2b. a round that lists more rows than the compacted last-layer tail holds (256): the batch evaluates the tail on
# all rows, the same image alone lists fewer and takes the compacted branch -- its bits may not depend on that
def test_an_image_does_not_depend_on_the_branch_its_batchs_tail_takes(model, monkeypatch):
    steps, widest, real = 4, [], engine.schedule.plan_rounds

    def plan(*a, **kw):
        p = real(*a, **kw)
        widest.append(int((p.start[1:] - p.start[:-1]).max()))
        return p

    monkeypatch.setattr(engine.schedule, 'plan_rounds', plan)
    model.feed_data(BATCH)
    lists, logp = model.sample_fn(sample_steps=steps, seeds=SEEDS, return_logp=True)
    tok = torch.stack(lists)
    assert widest[-1] > model.sampler_fn.TRIM_MAX_ROWS and model.sampler_fn.last_launch_mode == 'eager', widest
    for b in range(B):
        model.feed_data(_sub(BATCH, [b]))
        want, want_logp = model.sample_fn(sample_steps=steps, seeds=[SEEDS[b]], return_logp=True)
        assert widest[-1] <= model.sampler_fn.TRIM_MAX_ROWS, widest
        assert torch.equal(tok[:, b], torch.stack(want)[:, 0]), b
        assert torch.equal(_bits(logp[b]), _bits(want_logp[0])), b


# ---- 3. permutation and composition
def test_an_image_does_not_depend_on_its_position_or_its_neighbours(model):
    tok, logp, offs = _seeded(model, BATCH, SEEDS)
    order = [2, 0, 1]
    tok_p, logp_p, offs_p = _seeded(model, _sub(BATCH, order), [SEEDS[i] for i in order])
    for pos, b in enumerate(order):
        assert torch.equal(tok_p[:, pos], tok[:, b]) and torch.equal(_bits(logp_p[pos]), _bits(logp[b])), (pos, b)
        assert int(offs_p[pos]) == int(offs[b])
    # image 0 beside two OTHER neighbours (and in the middle)
    mixed = _cat(_sub(OTHERS, [1]), _sub(BATCH, [0]), _sub(OTHERS, [2]))
    tok_m, logp_m, offs_m = _seeded(model, mixed, [SEEDS[1], SEEDS[0], SEEDS[2]])
    assert torch.equal(tok_m[:, 1], tok[:, 0]) and torch.equal(_bits(logp_m[1]), _bits(logp[0]))
    assert int(offs_m[1]) == int(offs[0])
    assert not torch.equal(tok_m[:, 0], tok[:, 1])   # (the neighbours ARE other images)


# ---- 4. non-vacuity
def test_the_seed_is_what_makes_an_image(model):
    same = _cat(*[_sub(BATCH, [0])] * 3)
    a = SEEDS[0]
    tok, logp, _ = _seeded(model, same, [a, a, a])
    assert torch.equal(tok[:, 0], tok[:, 1]) and torch.equal(tok[:, 0], tok[:, 2])
    assert torch.equal(_bits(logp[0]), _bits(logp[1])) and torch.equal(_bits(logp[0]), _bits(logp[2]))
    tok3, _, _ = _seeded(model, same, SEEDS)
    assert torch.equal(tok3[:, 0], tok[:, 0])
    assert not torch.equal(tok3[:, 0], tok3[:, 1]) and not torch.equal(tok3[:, 1], tok3[:, 2])
    assert not torch.equal(tok3[:, 0], tok3[:, 2])
    model.feed_data(same)
    seed_all(SEEDS[0])
    plain = torch.stack(model.sample_fn(sample_steps=STEPS))
    for b in range(3):   # the unseeded call draws a [3 * 512]-row stream: none of its images is a seeded one
        assert not torch.equal(plain[:, b], tok3[:, b]), b


# ---- 5. the global generator
def test_the_global_generator_is_neither_read_nor_advanced(model):
    model.feed_data(BATCH)
    seed_all(5)
    want = torch.stack(model.sample_fn(sample_steps=STEPS))
    seed_all(5)
    torch.rand(7, device=DEV)   # (a state that is not a fresh seed's)
    state = _gen().get_state().clone()
    _seeded(model, BATCH, SEEDS)
    assert torch.equal(_gen().get_state(), state)
    seed_all(5)
    state = _gen().get_state().clone()
    model.score_fn_seeded(list(want), SEEDS, sample_steps=STEPS)
    assert torch.equal(_gen().get_state(), state)
    got = torch.stack(model.sample_fn(sample_steps=STEPS))
    assert torch.equal(got, want)   # the unseeded call: what it returns without the seeded calls in between
    assert model.last_seed_offsets is None


# ---- 6. region editing: image 0 finishes first, so the seed table must follow the batch's reordering
def _edit_keep():
    """test_gpu_per_image._edit_keep: image 0 resamples 3 rows (the fewest rounds), image 1 everything, image 2 every
    other row"""
    keep = torch.zeros(B, T, dtype=torch.uint8)
    keep[0] = 1
    keep[0, [5, 200, 411]] = 0
    keep[2, ::2] = 1
    return keep


@pytest.mark.parametrize('graph', ['1', '0'])
def test_resample_with_seeds_equals_the_single_image_edits(model, monkeypatch, graph):
    monkeypatch.setenv('T2H_GRAPH', graph)
    monkeypatch.setenv('T2H_SHRINK_BATCH', '1')
    perms, real = [], engine.schedule.plan_rounds

    def plan(*a, **kw):
        p = real(*a, **kw)
        perms.append(p.perm)
        return p

    src, _, _ = _seeded(model, BATCH, [11, 12, 13])
    keep = _edit_keep()
    monkeypatch.setattr(engine.schedule, 'plan_rounds', plan)
    model.feed_data(BATCH)
    lists, logp = model.resample_fn(list(src), keep, sample_steps=STEPS, seeds=SEEDS, return_logp=True)
    monkeypatch.setattr(engine.schedule, 'plan_rounds', real)
    assert len(perms) == 1 and perms[0] is not None and int(perms[0][-1]) == 0, perms   # image 0 left first
    got = torch.stack(lists)
    k = keep.bool().to(got.device)
    assert torch.equal(got[:, k], src[:, k])                                # kept rows are untouched
    assert bool(torch.isnan(logp[k]).all()) and bool(torch.isfinite(logp[~k]).all())
    for b in range(B):
        model.feed_data(_sub(BATCH, [b]))
        torch.cuda.manual_seed(SEEDS[b])
        want, want_logp = model.resample_fn([t[b:b + 1] for t in src], keep[b:b + 1], sample_steps=STEPS, return_logp=True)
        assert torch.equal(got[:, b], torch.stack(want)[:, 0]), b
        assert torch.equal(_bits(logp[b]), _bits(want_logp[0])), b
        assert model.last_seed_offsets is None                             # (an unseeded call leaves none)


# ---- 7. scoring
def test_score_with_seeds_returns_the_seeded_draws_logp_bits(model):
    """(seeded scoring is `score_fn_seeded(map, seeds)`: tests/test_score_options.py pins score_fn's parameter list)"""
    tok, logp, offs = _seeded(model, BATCH, SEEDS)
    model.feed_data(BATCH)
    got = model.score_fn_seeded(list(tok), SEEDS, sample_steps=STEPS)
    assert torch.equal(_bits(got), _bits(logp))
    assert torch.equal(model.last_seed_offsets, offs)
    other = model.score_fn_seeded(list(tok), [1, 2, 3], sample_steps=STEPS)   # another schedule: other conditionals
    assert not torch.equal(_bits(other), _bits(logp))


# ---- 8. per-image controls combined with seeds
def test_per_image_controls_combine_with_seeds(model):
    temp, top_k = [1.0, 0.7, 1.3], [None, 5, None]
    tok, logp, offs = _seeded(model, BATCH, SEEDS, temp=temp, top_k=top_k)
    plain, _, offs_plain = _seeded(model, BATCH, SEEDS)
    assert torch.equal(offs, offs_plain)   # (the stream does not depend on the controls)
    for b in range(B):
        want_tok, want_logp, want_off = _alone(model, BATCH, b, SEEDS[b], temp=temp[b], top_k=top_k[b])
        assert torch.equal(tok[:, b], want_tok) and torch.equal(_bits(logp[b]), _bits(want_logp)), b
        assert int(offs[b]) == want_off
    assert torch.equal(tok[:, 0], plain[:, 0]) and not torch.equal(tok[:, 1], plain[:, 1])


# ---- 9. graph reuse
def test_other_seeds_replay_the_same_graphs(model, monkeypatch):
    monkeypatch.setenv('T2H_GRAPH', '1')
    net = model.sampler_fn
    first, _, _ = _seeded(model, BATCH, SEEDS)
    assert net.last_launch_mode == 'graph'
    keys = [k for k in net._graphs if k[-1] == 'seeded' and k[0] == B]
    assert keys
    captures = lambda: sum(g.captures for g in net._graphs.values())
    n_graphs, n_captures = len(net._graphs), captures()
    second, _, _ = _seeded(model, BATCH, [s + 1 for s in SEEDS[::-1]])
    assert net.last_launch_mode == 'graph'
    assert len(net._graphs) == n_graphs and captures() == n_captures       # nothing new was captured
    assert not torch.equal(first, second)
    again, _, _ = _seeded(model, BATCH, SEEDS)
    assert torch.equal(again, first) and captures() == n_captures
    # the key gains 'seeded' and nothing else
    args = (B, T, STEPS, 128, 1.0, 18432, 18, True)
    assert engine.round_graph_key(*args, logp=True, seeded=True) == engine.round_graph_key(*args, logp=True) + ('seeded', )
    args = (B, T, STEPS, 128, 18432, 18, True)
    assert (engine.round_graph_key_per_image(*args, score=engine.SCORE, seeded=True) ==
            engine.round_graph_key_per_image(*args, score=engine.SCORE) + ('seeded', ))


# ---- 10. refusals
def test_refusals_leave_the_generator_alone(model):
    model.feed_data(BATCH)
    seed_all(3)
    torch.rand(5, device=DEV)
    off = _gen().get_offset()
    src = [torch.zeros(B, T, dtype=torch.int64) for _ in range(18)]
    keep = torch.zeros(B, T, dtype=torch.uint8)
    for call in (lambda: model.sample_fn_confidence(seeds=SEEDS),
                 lambda: model.sample_best_of(2, seeds=SEEDS),
                 lambda: model.sample_best_of(2, order='random', seeds=SEEDS, sample_steps=STEPS),
                 lambda: model.resample_fn(src, keep, order='confidence', seeds=SEEDS),
                 lambda: model.sample_fn(seeds=SEEDS[:2], sample_steps=STEPS),
                 lambda: model.sample_fn(seeds=SEEDS + [1], sample_steps=STEPS),
                 lambda: model.sample_fn(seeds=[1, -2, 3], sample_steps=STEPS),
                 lambda: model.sample_fn(seeds=[1, 2.5, 3], sample_steps=STEPS),
                 lambda: model.sample_fn(seeds=[1, True, 3], sample_steps=STEPS),
                 lambda: model.score_fn_seeded(src, SEEDS[:1], sample_steps=STEPS),
                 lambda: model.resample_fn(src, keep, seeds=[1 << 64, 1, 1], sample_steps=STEPS)):
        with pytest.raises(ValueError):
            call()
        assert _gen().get_offset() == off
    model.noise = object()   # an explicit noise source
    try:
        with pytest.raises(ValueError, match='explicit noise'):
            model.sample_fn(seeds=SEEDS, sample_steps=STEPS)
    finally:
        model.noise = None
    assert _gen().get_offset() == off


# ---- 11. the entry point: the same tokens per img_name whatever the batch size
def test_entry_point_tokens_do_not_depend_on_the_batch_size(tmp_path, monkeypatch):
    e_opt = defaults.with_per_image_seeds(defaults.sample_from_parsing())
    e_sds = synthetic.make_state_dicts(options.dict_to_nonedict(e_opt), seed=1234)
    e_opt = synthetic.write_checkpoints(e_opt, str(tmp_path / 'ckpt'), state_dicts=e_sds)
    tree = synthetic.write_dataset_tree(str(tmp_path / 'data'), n=4, seed=11)
    names = tree.pop('names')
    e_opt.update(tree)
    real, real_save = sample_model.BaseSampleModel.sample_fn, sample_model.save_u8_images
    tokens, pixels, calls = {}, {}, []

    def spy(self, *a, **k):
        top = real(self, *a, **k)
        calls.append((tuple(k['seeds']), torch.stack(top).cpu()))
        return top

    def save_spy(u8, save_dir, img_name):
        seeds, top = calls[-1]
        assert list(seeds) == [options.image_seed(2021, n) for n in img_name]
        for i, n in enumerate(img_name):
            tokens[bs][n], pixels[bs][n] = top[:, i].clone(), u8[i].cpu().numpy().copy()
        return real_save(u8, save_dir, img_name)

    monkeypatch.setattr(sample_model.BaseSampleModel, 'sample_fn', spy)
    monkeypatch.setattr(sample_model, 'save_u8_images', save_spy)
    monkeypatch.chdir(tmp_path)
    for bs in (1, 2, 4):
        tokens[bs], pixels[bs] = {}, {}
        e_opt.update(name=f'seeded_bs{bs}', sample_steps=6, manual_seed=2021)
        cfg = defaults.write_yaml(e_opt, str(tmp_path / f'bs{bs}.yml'))
        sample_from_parsing.run(pose=False, argv=['-opt', cfg, '--batch-size', str(bs)])
        assert sorted(tokens[bs]) == sorted(names)
    for n in names:
        for bs in (2, 4):
            assert torch.equal(tokens[bs][n], tokens[1][n]), (n, bs)
            print(f'{n}: PNG pixels at batch size {bs} '
                  + ('identical to' if np.array_equal(pixels[bs][n], pixels[1][n]) else
                     f'differ ({int((pixels[bs][n] != pixels[1][n]).sum())} bytes) from') + ' batch size 1')
    assert not torch.equal(tokens[1][names[0]], tokens[1][names[1]])
