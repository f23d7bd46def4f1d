"""Per-image sampling controls on the GPU (-m gpu; DESIGN.md, "Per-image sampling controls"): temp / top_k / top_p -- and
in confidence mode rounds / choice_temp -- given as one value per image.

Samples never interact and neither the schedule nor the generator depends on these controls, so the check is exact:
image b of a mixed batch is, token for token, image b of the SAME batch run with image b's values as scalars under
the same seed, and the generator ends where the scalar run leaves it.  Every comparison also asserts that it could
fail: the images with non-default values differ from the all-default run."""
import numpy as np
import pytest
import torch

from text2human_amd import defaults, engine, ops, options, synthetic
from text2human_amd.models import SampleFromParsingModel

from parity_util import seed_all  # noqa: E402

pytestmark = pytest.mark.gpu
B, T, STEPS = 3, 512, 16
TEMP, TOP_K, TOP_P = (1.0, 0.7, 1.3), (None, 5, None), (None, None, 0.6)
MODES = [('1', '1'), ('1', '0'), ('0', '1'), ('0', '0')]   # (T2H_GRAPH, T2H_SHRINK_BATCH)


@pytest.fixture(scope='module')
def opt():
    return options.dict_to_nonedict(defaults.sample_from_parsing())


@pytest.fixture(scope='module')
def sds(opt):
    return synthetic.make_state_dicts(opt, seed=1234)


@pytest.fixture(scope='module')
def model(opt, sds):
    m = SampleFromParsingModel(opt, state_dicts=sds)
    m.feed_data(synthetic.parsing_batch(B, seed=91))
    return m


def _gen():
    return torch.cuda.default_generators[torch.cuda.current_device()]


def _run(fn, seed, **kw):
    """-> (tokens int64 [18, B, 512], generator offset after the call - before it)"""
    seed_all(seed)
    off0 = _gen().get_offset()
    out = torch.stack(fn(**kw))
    return out, _gen().get_offset() - off0


def _scalars(b, **seqs):
    return {k: v[b] for k, v in seqs.items()}


def _assert_images_equal_their_scalar_runs(fn, seed, seqs, **fixed):
    """the mixed call against one scalar call per image and the all-default call; -> (mixed tokens, offset advance)"""
    mixed, adv = _run(fn, seed, **seqs, **fixed)
    plain, adv_plain = _run(fn, seed, **fixed)
    assert adv == adv_plain
    for b in range(B):
        want, adv_b = _run(fn, seed, **_scalars(b, **seqs), **fixed)
        assert torch.equal(mixed[:, b], want[:, b]), (b, int((mixed[:, b] != want[:, b]).sum()))
        assert adv_b == adv
        own = _scalars(b, **seqs)
        # non-vacuity: the image's own values matter on this seed and these weights
        if own.get('temp', 1.0) != 1.0 or own.get('top_k') or own.get('top_p') not in (None, 1.0):
            assert not torch.equal(mixed[:, b], plain[:, b]), b
    return mixed, adv


@pytest.mark.parametrize('graph,shrink', MODES)
def test_mixed_batch_equals_the_scalar_runs_image_by_image(model, monkeypatch, graph, shrink):
    monkeypatch.setenv('T2H_GRAPH', graph)
    monkeypatch.setenv('T2H_SHRINK_BATCH', shrink)
    _assert_images_equal_their_scalar_runs(model.sample_fn, 17, dict(temp=list(TEMP), top_k=list(TOP_K), top_p=list(TOP_P)),
                                           sample_steps=STEPS)
    assert model.sampler_fn.last_launch_mode == ('graph' if graph == '1' else 'eager')


@pytest.mark.parametrize('kind', ['tuple', 'numpy', 'tensor'])
def test_the_sequence_kinds_are_one_path(model, kind):
    conv = dict(tuple=tuple, numpy=np.asarray, tensor=torch.tensor)[kind]
    want, _ = _run(model.sample_fn, 17, temp=list(TEMP), top_k=[0, 5, 0], sample_steps=STEPS)
    got, _ = _run(model.sample_fn, 17, temp=conv(TEMP), top_k=conv((0, 5, 0)), sample_steps=STEPS)
    assert torch.equal(got, want)


def _edit_keep():
    """keep [B, 512]: image 0 resamples 3 rows (the fewest rounds), image 1 everything, image 2 every other row"""
    keep = torch.zeros(B, T, dtype=torch.uint8)
    keep[0] = 1
    keep[0, [5, 200, 411]] = 0
    keep[2, ::2] = 1
    return keep


@pytest.mark.parametrize('graph', ['1', '0'])
def test_the_table_follows_the_batch_when_finished_samples_leave_it(model, monkeypatch, graph):
    """region editing makes image 0 the first to finish: the engine reorders the batch (sched.perm) and must reorder
    the table with it -- otherwise image 0's values would be applied to image 1"""
    monkeypatch.setenv('T2H_GRAPH', graph)
    monkeypatch.setenv('T2H_SHRINK_BATCH', '1')
    perms, real = [], engine.schedule.plan_rounds

    def plan(*a, **kw):
        p = real(*a, **kw)
        perms.append(p.perm)
        return p

    monkeypatch.setattr(engine.schedule, 'plan_rounds', plan)
    src, _ = _run(model.sample_fn, 23, sample_steps=STEPS)
    src = list(src)
    keep = _edit_keep()
    fn = lambda **kw: model.resample_fn(src, keep, sample_steps=STEPS, **kw)
    mixed, _ = _assert_images_equal_their_scalar_runs(fn, 29, dict(temp=list(TEMP), top_k=list(TOP_K), top_p=list(TOP_P)))
    assert len(perms) == 6 and all(p is not None and int(p[-1]) == 0 for p in perms[1:]), perms   # (perms[0]: the source's run)
    k = keep.bool().to(mixed.device)
    assert torch.equal(mixed[:, k], torch.stack(src)[:, k])


def test_confidence_mode_rounds_and_choice_temperature_per_image(model):
    rounds, ct = [4, 8, 6], [0.0, 4.5, 2.0]
    seqs = dict(rounds=rounds, choice_temp=ct, temp=list(TEMP), top_k=list(TOP_K), top_p=list(TOP_P))
    seed_all(31)
    off0 = _gen().get_offset()
    mixed = torch.stack(model.sample_fn_confidence(**seqs))
    adv = _gen().get_offset() - off0
    n = B * T
    assert adv == 8 * (ops.torch_draw_geometry(n * 1024)[1] + ops.torch_draw_geometry(n)[1])
    assert model.sampler_fn.last_stats['rounds'] == 8
    assert bool((mixed.sum(0) + 17 >= 0).all())                                # every row drew a token under one head
    plain, _ = _run(model.sample_fn_confidence, 31, rounds=8)
    for b in range(B):
        want, adv_b = _run(model.sample_fn_confidence, 31, **_scalars(b, **seqs))
        assert torch.equal(mixed[:, b], want[:, b]), (b, int((mixed[:, b] != want[:, b]).sum()))
        assert adv_b == rounds[b] * adv // 8
        assert not torch.equal(mixed[:, b], plain[:, b]), b
    # rounds alone per image: the tails' table holds the scalars for every image
    only_rounds, _ = _run(model.sample_fn_confidence, 31, rounds=rounds, choice_temp=2.0, temp=0.9)
    for b in range(B):
        want, _ = _run(model.sample_fn_confidence, 31, rounds=rounds[b], choice_temp=2.0, temp=0.9)
        assert torch.equal(only_rounds[:, b], want[:, b]), b


@pytest.mark.parametrize('graph', ['1', '0'])
def test_a_uniform_sequence_gives_the_scalar_calls_tokens(model, monkeypatch, graph):
    monkeypatch.setenv('T2H_GRAPH', graph)
    want, adv = _run(model.sample_fn, 37, temp=0.8, top_k=7, sample_steps=STEPS)
    got, adv_s = _run(model.sample_fn, 37, temp=[0.8] * B, top_k=[7] * B, sample_steps=STEPS)
    assert torch.equal(got, want) and adv == adv_s
    want, adv = _run(model.sample_fn_confidence, 37, rounds=6, temp=0.8, top_k=7)
    got, adv_s = _run(model.sample_fn_confidence, 37, rounds=[6] * B, choice_temp=[4.5] * B, temp=[0.8] * B, top_k=[7] * B)
    assert torch.equal(got, want) and adv == adv_s


@pytest.mark.parametrize('order', ['random', 'confidence'])
def test_editing_with_per_image_temperatures_and_a_fully_kept_image(model, order):
    src, _ = _run(model.sample_fn, 41, sample_steps=STEPS)
    src = list(src)
    keep = torch.zeros(B, T, dtype=torch.uint8)
    keep[1, 100:300] = 1
    keep[2] = 1                                                                 # image 2 is kept as it is
    temps = [0.7, 1.3, 0.5]
    kw = dict(order=order, rounds=6) if order == 'confidence' else dict(sample_steps=STEPS)
    fn = lambda **t: model.resample_fn(src, keep, **kw, **t)
    mixed, adv = _run(fn, 43, temp=temps)
    plain, _ = _run(fn, 43)
    assert torch.equal(mixed[:, 2], torch.stack(src)[:, 2])
    assert torch.equal(mixed[:, 1, 100:300], torch.stack(src)[:, 1, 100:300])
    for b in (0, 1):
        want, adv_b = _run(fn, 43, temp=temps[b])
        assert torch.equal(mixed[:, b], want[:, b]) and adv_b == adv, b
        assert not torch.equal(mixed[:, b], plain[:, b]), b


def test_per_image_runs_share_one_graph_set_and_leave_the_scalar_graphs_alone(model, opt, sds, monkeypatch):
    monkeypatch.setenv('T2H_GRAPH', '1')
    net = model.sampler_fn
    first, _ = _run(model.sample_fn, 47, temp=0.9, sample_steps=STEPS)
    assert net.last_launch_mode == 'graph'
    n_scalar = len(net._graphs)
    a, _ = _run(model.sample_fn, 47, temp=[1.0, 0.7, 1.3], top_k=[None, 5, None], sample_steps=STEPS)
    n_per_image = len(net._graphs)
    assert n_per_image in (n_scalar, n_scalar + 1)                               # (an earlier test may have captured it)
    keys = [k for k in net._graphs if k[-1] == 'per-sample']
    assert keys and all(k[:3] == (B, T, STEPS) for k in keys)
    b, _ = _run(model.sample_fn, 47, temp=[0.5, 1.1, 0.9], top_k=[3, None, 100], top_p=[None, 0.5, 0.9], sample_steps=STEPS)
    assert len(net._graphs) == n_per_image and not torch.equal(a, b)             # other values, the same captures
    again, _ = _run(model.sample_fn, 47, temp=0.9, sample_steps=STEPS)
    assert len(net._graphs) == n_per_image and torch.equal(again, first)         # the scalar call finds its own key
    fresh = SampleFromParsingModel(opt, state_dicts=sds)
    fresh.feed_data(synthetic.parsing_batch(B, seed=91))
    want, _ = _run(fresh.sample_fn, 47, temp=0.9, sample_steps=STEPS)
    assert torch.equal(first, want)
    assert all(k[-1] != 'per-sample' for k in fresh.sampler_fn._graphs)


@pytest.mark.parametrize('kw', [dict(temp=[1.0, 0.0, 1.0]), dict(top_k=[1, 2]), dict(top_p=[None, 2.0, None]),
                                dict(rounds=[4, 0, 4]), dict(choice_temp=[0.0, -1.0, 0.0])], ids=str)
def test_bad_values_raise_before_the_generator_moves(model, kw):
    seed_all(3)
    torch.rand(5, device='cuda')
    off = _gen().get_offset()
    fn = model.sample_fn_confidence if ('rounds' in kw or 'choice_temp' in kw) else model.sample_fn
    with pytest.raises(ValueError, match='image 1|entries'):
        fn(**kw)
    assert _gen().get_offset() == off
