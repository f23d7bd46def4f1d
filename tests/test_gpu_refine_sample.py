"""Sampled bottom-index refinement on the GPU (-m gpu).

Kernel: the property code of tests/refine_ref.py (numbered as there) on the hardware, 111 token rows, 37, 512 (the
checkpoints' bottom codebook) and 1024 classes; the CPU twin is tests/test_refine_sample_emulated.py.  Model:
decode_indices / edit_and_refine with refine_temp / refine_top_k / refine_top_p on synthetic checkpoints -- the generator contract, chunk independence, the
degenerate settings, per-image controls, region editing and the overflow fall-back."""
import pytest
import torch

import decode_bands as D
import per_image_ref
import refine_ref as RR
from text2human_amd import _lib, defaults, engine, ops, options, synthetic
from text2human_amd.models import SampleFromParsingModel
from text2human_amd.models import sample_model as SM

from parity_util import seed_all  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda'
ENV = D.Env(DEV, lambda kernel_file: _lib.load(), ops._stream, lambda lib: (lib.t2h_last_error() or b'?').decode())
N = 111
CLASSES = [37, 512, 1024]
LABELS = (1, 2, 3)   # parsing labels of synthetic.parsing_batch's coarse cells: about 1/8 of the rows


def table_of(sets):
    return torch.from_numpy(per_image_ref.table(sets))


# ---------------------------------------------------------------------------------------------- the kernel

@pytest.mark.parametrize('n_class', CLASSES)
def test_equals_the_argmax_kernel_when_the_noise_says_nothing(n_class):
    RR.equals_argmax_when_the_noise_says_nothing(ENV, N, n_class)


@pytest.mark.parametrize('n_class', CLASSES)
def test_draw_is_the_fp64_race(n_class):
    RR.the_draw(ENV, N, n_class)


@pytest.mark.parametrize('n_class', CLASSES)
def test_truncation(n_class):
    RR.truncation(ENV, N, n_class)


@pytest.mark.parametrize('n_class', CLASSES)
def test_in_kernel_noise_is_the_philox_tensor(n_class):
    RR.in_kernel_noise(ENV, N, n_class)


@pytest.mark.parametrize('n_class', CLASSES)
def test_in_kernel_noise_is_torchs_exponential_draw(n_class):
    """expo = NULL at (s, 0) with ATen's grid for the tensor == torch's own draw after manual_seed(s) as explicit expo"""
    assert engine.TorchDeviceNoise(DEV).emulation_ok(N, n_class)
    s = 20261
    pb = RR.problem(N, n_class)
    torch.manual_seed(s)
    e = torch.empty(N, n_class, device=DEV).exponential_()
    gt = ops.torch_draw_geometry(N * n_class, torch.device(DEV))[0]
    want = RR.Launch(ENV, pb, expo=e.cpu()).run()
    got = RR.Launch(ENV, pb, expo=None, philox=(s, 0, gt)).run()
    assert torch.equal(got.lists, want.lists) and torch.equal(RR.G.bits(got.logp), RR.G.bits(want.logp))


@pytest.mark.parametrize('n_class', CLASSES)
def test_per_sample_table(n_class):
    RR.per_sample_table(ENV, 37, n_class, table_of)


@pytest.mark.parametrize('temp', [1.0, 2.0])
def test_it_samples_the_softmax(temp):
    RR.samples_the_softmax(ENV, temp)


def test_rejected_arguments_write_nothing():
    RR.rejected_arguments(ENV, table_of)


def test_ops_wrapper_is_the_entry_point():
    """ops.routed_head_sample: the arguments reach the struct (explicit and Philox noise, scalars and a table)"""
    pb = RR.problem(N, 37)
    dev = lambda k: pb[k].to(DEV)  # noqa: E731
    feat = torch.zeros(N, RR.LDF, device=DEV)
    feat[:, :RR.N_HEADS * RR.CF] = dev('feat')
    feat = feat[:, :RR.N_HEADS * RR.CF]                                                 # ldf > the row
    args = (feat, dev('w'), dev('b'), dev('tex'), RR.N_HEADS, RR.CF, 37)
    want = RR.Launch(ENV, pb, temp=0.7, top_k=5, top_p_q=RR.p_q_of(0.9)).run()
    out, logp, ws = ops.routed_head_sample(*args, temp=0.7, top_k=5, top_p=0.9, expo=dev('expo'), want_logp=True,
                                           want_logits=True)
    assert torch.equal(out.cpu(), want.lists) and torch.equal(logp.cpu(), want.logp) and torch.equal(ws.cpu(), want.ws)
    tbl = ops.sample_params_tensor(ops.sampling_params(3, [1.0, 0.7, 1.4], [None, 5, 64], [None, None, 0.6], 37).table, DEV)
    got = ops.routed_head_sample(*args, params=tbl, rows_per_sample=37, expo=dev('expo'))
    assert torch.equal(got.cpu(), RR.Launch(ENV, pb, table=table_of(RR.PER_SAMPLE_SETS), T=37).run().lists)
    gt = ops.torch_draw_geometry(N * 37, torch.device(DEV))[0]
    got = ops.routed_head_sample(*args, philox=(5, 8))
    assert torch.equal(got.cpu(), RR.Launch(ENV, pb, expo=None, philox=(5, 8, gt)).run().lists)
    with pytest.raises(ValueError):
        ops.routed_head_sample(*args)
    with pytest.raises(ValueError, match='temp'):
        ops.routed_head_sample(*args, temp=0.0, philox=(5, 8))


# ---------------------------------------------------------------------------------------------- the model

@pytest.fixture(scope='module')
def opt():
    return options.dict_to_nonedict(defaults.sample_from_parsing())


@pytest.fixture(scope='module')
def model(opt):
    return SampleFromParsingModel(opt, state_dicts=synthetic.make_state_dicts(opt, seed=77))


def _gen():
    return torch.cuda.default_generators[torch.cuda.current_device()]


def _feed(model, B, seed, steps=8):
    """a batch fed to the model and top tokens sampled for it (18 x [B, 512])"""
    model.feed_data(synthetic.parsing_batch(B, seed=seed))
    seed_all(seed)
    return model.sample_fn(temp=1, sample_steps=steps)


def _decode(model, top, seed, **kw):
    """-> (images, bot_lists [18, B * 512], generator offset advance) of decode_indices from seed"""
    seed_all(seed)
    off0 = _gen().get_offset()
    img, _, inter = model.decode_indices(top, return_inter=True, **kw)
    return img, torch.cat([d['bot_lists'] for d in inter], 1), _gen().get_offset() - off0, inter


def _own_logits64(model, inter, B):
    """fp64 logits of every token's own head from the head features, recomputed with the model's own ops"""
    P, ipd = model.P, model.ipd
    tq = torch.cat([d['top_quant'] for d in inter], 0)
    hc = model._head_features(tq, B)
    tex = model._texture_tokens(model.texture_mask).reshape(-1)
    n, cf = tex.numel(), ipd['cf']
    f = hc[:, :ipd['n_heads'] * cf].reshape(n, ipd['n_heads'], cf)[torch.arange(n, device=DEV), tex].double()
    l = torch.empty(n, ipd['n_class'], dtype=torch.float64, device=DEV)
    for h in tex.unique().tolist():
        rows = tex == h
        l[rows] = f[rows] @ P['ipd.seg.w'][h].double().t() + P['ipd.seg.b'].reshape(ipd['n_heads'], -1)[h].double()
    return l, tex


def test_generator_contract_and_the_restated_draw(model):
    """8: one [B * 512, n_class] exponential_ draw, the restatement's tokens on that tensor; no refine argument: the
    generator is not touched and the images are those of a plain decode_indices(top)"""
    B, seed = 2, 11
    top = _feed(model, B, 61)
    n, n_class = B * 512, model.ipd['n_class']
    img, bot, adv, inter = _decode(model, top, seed, refine_temp=1.0)
    seed_all(seed)
    off0 = _gen().get_offset()
    e = torch.empty(n, n_class, device=DEV).exponential_()
    assert adv == _gen().get_offset() - off0 > 0
    l64, tex = _own_logits64(model, inter, B)
    want, near = RR.race(l64, e)
    tok = bot[tex, torch.arange(n, device=DEV)]
    RR.assert_tokens(tok.cpu(), want.cpu(), near.cpu(), 'decode_indices(refine_temp=1)')
    assert (bot >= 0).sum() == n and not torch.equal(tok, l64.argmax(1))          # one list per token; it is a draw
    seed_all(seed)
    state = torch.cuda.get_rng_state(DEV)
    img0, _, inter0 = model.decode_indices(top, return_inter=True)
    plain, _ = model.decode_indices(top)
    none, _ = model.decode_indices(top, refine_temp=None, refine_top_k=None, refine_top_p=None)
    assert torch.equal(torch.cuda.get_rng_state(DEV), state)
    assert torch.equal(img0, plain) and torch.equal(none, plain)
    assert not torch.equal(img, plain)


def test_chunk_size_does_not_change_the_draw(model, monkeypatch):
    """9: DECODE_CHUNK 1 and 2 at B = 3: identical bot_lists and images"""
    top = _feed(model, 3, 62)
    res = []
    for chunk in (1, 2, 8):
        monkeypatch.setattr(SM, 'DECODE_CHUNK', chunk)
        img, bot, adv, _ = _decode(model, top, 12, refine_temp=0.9, refine_top_p=0.95)
        res.append((img, bot, adv))
    for img, bot, adv in res[1:]:
        assert torch.equal(bot, res[0][1]) and torch.equal(img, res[0][0]) and adv == res[0][2]


@pytest.mark.parametrize('temp', [None, 0.7, 1.6])
def test_top_k_one_is_the_argmax_path(model, temp):
    """10: refine_top_k = 1 at any temperature: the bot_lists and images of the call without refine arguments"""
    top = _feed(model, 2, 63)
    img0, bot0, adv0, _ = _decode(model, top, 13)
    img, bot, adv, _ = _decode(model, top, 13, refine_top_k=1, **({} if temp is None else dict(refine_temp=temp)))
    assert adv0 == 0 and adv > 0
    assert torch.equal(bot, bot0) and torch.equal(img, img0)


def test_per_image_controls_equal_the_scalar_calls(model):
    """11: refine_temp = [1.0, 0.5] (and a per-image top-k) == image 0 of the first scalar call, image 1 of the second"""
    top = _feed(model, 2, 64)
    img, bot, adv, _ = _decode(model, top, 14, refine_temp=[1.0, 0.5], refine_top_k=[None, 40])
    a = _decode(model, top, 14, refine_temp=1.0)
    b = _decode(model, top, 14, refine_temp=0.5, refine_top_k=40)
    assert adv == a[2] == b[2]
    assert torch.equal(bot[:, :512], a[1][:, :512]) and torch.equal(bot[:, 512:], b[1][:, 512:])
    assert torch.equal(img[0], a[0][0]) and torch.equal(img[1], b[0][1])
    assert not torch.equal(a[1][:, 512:], b[1][:, 512:])                              # the settings matter on this seed
    with pytest.raises(ValueError, match='refine_temp'):
        model.decode_indices(top, refine_temp=[1.0, 0.5, 2.0])
    state = torch.cuda.get_rng_state(DEV)
    with pytest.raises(ValueError, match='refine_top_p, image 1'):
        model.decode_indices(top, refine_top_p=[0.5, 1.5])
    assert torch.equal(torch.cuda.get_rng_state(DEV), state)


def test_region_edit_keeps_the_kept_bottom_indices(model, tmp_path):
    """12: edit_and_refine(refine_temp=1): every kept token keeps its bottom indices; inside the region the drawn
    indices differ from the argmax edit's (same seed, so the same top tokens)"""
    B = 2
    src = _feed(model, B, 65)
    _, bot_src, _, _ = _decode(model, src, 15)
    bot_src = [bot_src[i].view(B, 512) for i in range(18)]
    names = ['a.png', 'b.png']
    keep = model.region_keep(labels=LABELS).bool()
    assert 0 < int(keep.sum()) < B * 512
    kk = keep.unsqueeze(0).expand(18, -1, -1)
    res = {}
    for name, kw in (('argmax', {}), ('drawn', dict(refine_temp=1.0))):
        seed_all(16)
        model.sample_steps, steps = 8, model.sample_steps
        try:
            model.edit_and_refine(src, labels=LABELS, bot_indices_list=bot_src, save_dir=str(tmp_path), img_name=names, **kw)
        finally:
            model.sample_steps = steps
        res[name] = (torch.stack(model.edit_top_indices_list), torch.stack(model.edit_bot_indices_list))
        assert torch.equal(res[name][1][kk], torch.stack(bot_src)[kk]), name
    assert torch.equal(res['argmax'][0], res['drawn'][0])
    assert not torch.equal(res['argmax'][1][~kk], res['drawn'][1][~kk])
    # the first image alone (no files): per-image arguments are cut to it
    seed_all(16)
    img = model.edit_and_refine(src, labels=LABELS, bot_indices_list=bot_src, refine_temp=[1.0, 0.5])
    assert tuple(img.shape[:2]) == (1, 3) and model.edit_bot_indices_list[0].shape == (1, 512)


def test_overflow_fall_back_repeats_the_same_draw(opt):
    """13: a decoder whose activations leave the split rows' range (the recipe of tests/test_gpu_bench_parity.py): the
    refine-sampled call falls back to the exact-fp32 convolutions, returns the bot_lists of the same call with those
    selected up front, and the generator is advanced once"""
    sds = synthetic.make_state_dicts(opt, seed=1234)
    sds['decoder']['mid.block_1.norm2.weight'] = sds['decoder']['mid.block_1.norm2.weight'] * 3.0e5
    sds['decoder']['mid.block_1.conv2.weight'] = sds['decoder']['mid.block_1.conv2.weight'] * (1.0 / 3.0e5)
    m = SampleFromParsingModel(opt, state_dicts=sds)
    top = _feed(m, 2, 66, steps=3)
    SM._warned.discard('VQGAN refine / decode')
    with pytest.warns(UserWarning, match='exact-fp32'):
        img, bot, adv, _ = _decode(m, top, 17, refine_temp=1.0)
    assert m.decoder.use_split and m.bot_decoder_res.use_split
    m.decoder.use_split = m.bot_decoder_res.use_split = False
    try:
        img1, bot1, adv1, _ = _decode(m, top, 17, refine_temp=1.0)
    finally:
        m.decoder.use_split = m.bot_decoder_res.use_split = True
    assert adv == adv1 == ops.torch_draw_geometry(2 * 512 * m.ipd['n_class'], torch.device(DEV))[1]
    assert torch.equal(bot, bot1) and torch.equal(img, img1)
    _, bot0, adv0, _ = _decode(m, top, 17)
    assert adv0 == 0 and not torch.equal(bot, bot0)


def test_explicit_draws_give_the_same_tokens(model, monkeypatch):
    """a torch build whose Philox draws the kernels do not reproduce: the tensor is drawn for real; same tokens"""
    top = _feed(model, 2, 67)
    _, bot, adv, _ = _decode(model, top, 18, refine_temp=1.0, refine_top_k=50)
    monkeypatch.setattr(engine.TorchDeviceNoise, 'emulation_ok', lambda self, n, k: False)
    _, bot1, adv1, _ = _decode(model, top, 18, refine_temp=1.0, refine_top_k=50)
    assert torch.equal(bot, bot1) and adv == adv1


def test_bot_index_prediction_draws_too(model):
    top = _feed(model, 2, 68)
    _, bot, _, inter = _decode(model, top, 19, refine_temp=1.0)
    tq = torch.cat([d['top_quant'] for d in inter], 0)
    feature_top = tq.view(2, 32, 16, -1).permute(0, 3, 1, 2).contiguous()
    seed_all(19)
    got = torch.stack(model.bot_index_prediction(feature_top, model.texture_mask, refine_temp=1.0)).view(18, -1)
    assert torch.equal(got, bot)
    plain = torch.stack(model.bot_index_prediction(feature_top, model.texture_mask)).view(18, -1)
    assert not torch.equal(plain, bot)
