"""Garment colour control on the GPU (-m gpu): the kernel cases of tests/recolor_cases.py through the
library's C ABI against the float64 restatement of tests/recolor_ref.py, the ops wrappers against the same calls, and
garment_colors / recolor / the `recolor_*` options on a model with synthetic checkpoints."""
import ctypes
import os

import numpy as np
import pytest
import torch

from text2human_amd import _lib, defaults, ops, options, synthetic
from text2human_amd.models import SampleFromParsingModel, SampleFromPoseModel

import recolor_cases as cases  # noqa: E402
import recolor_ref as R  # noqa: E402
from parity_util import seed_all  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def _gen():
    torch.cuda.init()          # (the generators exist once the device is initialised)
    return torch.cuda.default_generators[torch.cuda.current_device()]


@pytest.fixture(scope='module')
def run():
    lib = _lib.load()
    return cases.Runner(lib, DEV, lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream), lib.t2h_last_error)


@pytest.mark.parametrize('case', cases.ALL_CASES, ids=lambda f: f.__name__)
def test_kernel_case(run, case):
    off = _gen().get_offset()
    case(run)
    assert _gen().get_offset() == off          # the generator is not touched


def test_ops_are_the_c_abi_calls(run):
    img = cases.image(3, cases.H, cases.W, 41, signed=True)
    segm = cases.segm_of(3, cases.H, cases.W, [[(1, 10, 50, 10, 50), (3, 50, 90, 10, 50)], [(2, 30, 70, 40, 80)], []])
    groups, bits = ['upper', 'lower', [2]], [cases.UP, cases.LO, cases.OU]
    st = ops.region_color_stats(img.to(DEV), segm.to(DEV), groups, img_signed=True)
    assert st.dtype == torch.float64 and tuple(st.shape) == (3, 3, 8) and st.is_cuda
    want = run.stats(img, segm, bits, True)
    assert np.array_equal(st.cpu().numpy().view(np.int64), want.view(np.int64))
    assert np.array_equal(ops.region_color_stats(img.to(DEV), segm[:, None].to(DEV), groups, img_signed=True).cpu().numpy(),
                          want)                                                   # ([B, 1, H, W] maps too)
    dst = torch.from_numpy(R.plain_target(want, (0.1, 0.7, 0.4))).to(DEV)
    out, u8 = ops.recolor_region(img.to(DEV), segm.to(DEV), groups, st, dst, luma=0.5, gain_max=2.0, feather=3,
                                 img_signed=True, want_u8=True)
    w_out, w_u8 = run.apply(img, segm, bits, want, dst.cpu().numpy(), luma=0.5, gain_max=2.0, feather=3, img_signed=True,
                            want_u8=True)
    assert torch.equal(out.cpu().view(torch.int32), w_out.view(torch.int32)) and torch.equal(u8.cpu(), w_u8)
    none, no8 = ops.recolor_region(img.to(DEV), segm.to(DEV), groups, st, dst)
    assert no8 is None and none.is_cuda
    with pytest.raises(ValueError, match='segm'):
        ops.region_color_stats(img.to(DEV), segm[:, :64].contiguous().to(DEV), groups)
    with pytest.raises(ValueError, match='src_stats'):
        ops.recolor_region(img.to(DEV), segm.to(DEV), groups, st[:, :2].contiguous(), dst)
    with pytest.raises(ValueError, match='dst_stats'):
        ops.recolor_region(img.to(DEV), segm.to(DEV), groups, st, dst.float())


# ------------------------------------------------------------------------------------------------ model level
@pytest.fixture(scope='module')
def model():
    opt = options.dict_to_nonedict(defaults.sample_from_parsing())
    m = SampleFromParsingModel(opt, state_dicts=synthetic.make_state_dicts(opt, seed=1234))
    m.feed_data(synthetic.parsing_batch(2, seed=77))
    m.sample_steps = 16
    return m


def test_model_recolor_garment_colors_and_options(model, monkeypatch, tmp_path):
    from PIL import Image
    assert SampleFromPoseModel.recolor is SampleFromParsingModel.recolor
    assert SampleFromPoseModel.garment_colors is SampleFromParsingModel.garment_colors
    B, colour, names = 2, (0.8, 0.2, 0.3), ['a.png', 'b.png']
    segm = model.segm.to(DEV, torch.float32).reshape(B, 512, 256).contiguous()

    seen = {}
    decode = model.decode_indices

    def spy(lists, *a, **kw):
        seen['lists'] = torch.stack(list(lists)).clone()
        res = decode(lists, *a, **kw)
        seen['img'] = res[0].clone()
        return res
    monkeypatch.setattr(model, 'decode_indices', spy)

    def sample(tag, **keys):
        d = tmp_path / tag
        d.mkdir()
        monkeypatch.setattr(model, 'opt', options.dict_to_nonedict(dict(model.opt, **keys)))
        seed_all(11)
        model.sample_and_refine(str(d), names)
        u8 = np.stack([np.asarray(Image.open(os.path.join(str(d), n))) for n in names])
        return seen['lists'], seen['img'], _gen().get_offset(), torch.from_numpy(u8)

    lists0, img, off0, plain8 = sample('plain')
    lists1, img1, off1, red8 = sample('red', recolor_upper=list(colour))
    # index lists, the decoded image and the generator are the same with and without the option
    assert torch.equal(lists0, lists1) and torch.equal(img, img1) and off0 == off1

    # recolor(img, upper=...) is the ops call with the model's parsing map and the upper group
    got, got8 = model.recolor(img, upper=colour, want_u8=True)
    src = ops.region_color_stats(img, segm, ['upper'])
    assert (src[:, 0, 0] > 0).all()
    dst = src.clone()
    dst[:, :, 1:4] = ops.recolor_yuv(colour).to(DEV)
    want, want8 = ops.recolor_region(img, segm, ['upper'], src, dst, want_u8=True)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32)) and torch.equal(got8, want8)
    assert torch.equal(got8.cpu(), red8) and not torch.equal(red8, plain8)        # what the option wrote
    per_image = torch.tensor([colour, colour], dtype=torch.float64, device=DEV)
    assert torch.equal(model.recolor(img, upper=per_image)[0].view(torch.int32), want.view(torch.int32))
    # ... and the float64 restatement; pixels with sum N == 0 are bit-identical to the un-recoloured image
    ref = R.recolor(img, segm, [cases.UP], src.cpu().numpy(), dst.cpu().numpy())
    err = (got.cpu().double() - ref['out']).abs().max().item()
    print(f'model recolor vs float64 reference: max abs err {err:.3e} (bound {R.TOL:.0e})')
    assert err <= R.TOL
    untouched = torch.from_numpy(~ref['touched'])
    assert untouched.any() and (~untouched).any()
    u3 = untouched[:, None].expand(-1, 3, -1, -1)
    assert torch.equal(got.cpu().view(torch.int32)[u3], img.cpu().view(torch.int32)[u3])
    assert torch.equal(red8[untouched], plain8[untouched])
    # the garment's mean chroma is the target's (where nothing was clamped the mean luma too)
    after = ops.region_color_stats(got, segm, ['upper']).cpu().numpy()
    print('upper after recolouring (mY, mU, mV):', after[:, 0, 1:4], 'target', R.colour_yuv(colour))

    # garment_colors agrees with region_color_stats
    st = ops.region_color_stats(img, segm, ['upper', 'lower', 'outer'])
    ref_st = R.stats(img, segm, [cases.UP, cases.LO, cases.OU])
    assert np.array_equal(st[..., 0].cpu().numpy(), ref_st[..., 0])
    assert np.abs(st.cpu().numpy() - ref_st)[..., 1:7].max() <= R.STATS_TOL
    gc = model.garment_colors(img)
    assert sorted(gc) == ['lower', 'outer', 'upper']
    for g, name in enumerate(('upper', 'lower', 'outer')):
        rgb, count = gc[name]
        assert rgb.dtype == torch.float32 and tuple(rgb.shape) == (B, 3) and rgb.is_cuda
        assert count.dtype == torch.int64 and torch.equal(count, st[:, g, 0].to(torch.int64))
        assert torch.equal(rgb, ops.recolor_rgb(st[:, g, 1:4]).float())
        assert np.abs(ops.recolor_yuv(rgb).cpu().numpy() - ref_st[:, g, 1:4]).max() <= 1e-6

    # an exemplar: the target is the same group's statistics in another image, explicit labels name a fourth group
    ex = torch.rand(1, 3, 512, 256, generator=torch.Generator().manual_seed(5)) * 2 - 1
    ex_segm = synthetic.parsing_batch(1, seed=3)['segm']
    got_like, _ = model.recolor(img, upper=True, labels={'hair': ([13], True)}, like=(ex, ex_segm), feather=4, gain_max=2.0)
    groups = ['upper', [13]]
    s2 = ops.region_color_stats(img, segm, groups)
    d2 = ops.region_color_stats(ex.to(DEV), ex_segm.to(DEV, torch.float32).reshape(1, 512, 256).contiguous(), groups,
                                img_signed=True).expand(B, -1, -1).contiguous()
    want_like, _ = ops.recolor_region(img, segm, groups, s2, d2, feather=4, gain_max=2.0)
    assert torch.equal(got_like.view(torch.int32), want_like.view(torch.int32))
