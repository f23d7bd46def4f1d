"""Two-band compositing on the GPU (-m gpu): the kernel cases of tests/composite_cases.py through
ops.composite_region against the float64 restatement of tests/composite_ref.py, one product-sized batch with a ragged
region, and edit_and_refine(source_image=...) / composite on the models with synthetic checkpoints."""
import os

import numpy as np
import pytest
import torch

from text2human_amd import defaults, ops, options, synthetic
from text2human_amd.models import SampleFromParsingModel, SampleFromPoseModel

import composite_cases as cases  # noqa: E402
import composite_ref as C  # noqa: E402
from parity_util import ACT_TOL, seed_all  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def run(dec, photo, keep, cells, r_hi, r_lo, want_u8=False, photo_signed=True):
    out, u8 = ops.composite_region(dec.to(DEV), photo.to(DEV), keep.to(DEV), cells, r_hi=r_hi, r_lo=r_lo,
                                   photo_signed=photo_signed, want_u8=want_u8)
    return out.cpu(), (u8.cpu() if want_u8 else None)


def _gen():
    torch.cuda.init()          # (the generators exist once the device is initialised)
    return torch.cuda.default_generators[torch.cuda.current_device()]


@pytest.mark.parametrize('case', cases.ALL_CASES, ids=lambda f: f.__name__)
def test_kernel_case(case):
    off = _gen().get_offset()
    case(run)
    assert _gen().get_offset() == off          # the generator is not touched


def test_product_size_with_a_ragged_region():
    B, th, tw = 2, 32, 16
    dec, photo = C.inputs(B, 512, 256, seed=31)
    blob = cases.ragged_region(th, tw, seed=5, n_cells=40)
    keep = C.keep_of(B, th, tw, [blob, blob[::2] + [(0, 0), (31, 15)]])
    assert int((keep == 0).sum()) == 40 + 20 + 2
    cases.check(run, dec, photo, keep, (th, tw), 4, 32, want_u8=True)


def test_shapes_and_radii_are_checked():
    x = torch.zeros(1, 3, 96, 80, device=DEV)
    k = torch.ones(1, 30, dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError, match='photo'):
        ops.composite_region(x, x[:, :, :64].contiguous(), k, (6, 5))
    with pytest.raises(ValueError, match='keep'):
        ops.composite_region(x, x.clone(), k[:, :20].contiguous(), (6, 5))
    with pytest.raises(ValueError, match='r_hi'):
        ops.composite_region(x, x.clone(), k, (6, 5), r_hi=8, r_lo=4)
    with pytest.raises(ops._lib.T2HError, match='multiple'):
        ops.composite_region(x, x.clone(), torch.ones(1, 35, dtype=torch.uint8, device=DEV), (7, 5))


# ------------------------------------------------------------------------------------------------ model level
@pytest.fixture(scope='module')
def photo():
    opt = options.dict_to_nonedict(defaults.sample_from_parsing())
    sds = synthetic.make_state_dicts(opt, seed=1234, encode=True)
    from text2human_amd.models import VQGANTextureAwareSpatialHierarchyInferenceModel as M
    hier, model = M(opt, state_dicts=sds), SampleFromParsingModel(opt, state_dicts=sds)
    B = 2
    image = torch.rand(B, 3, 512, 256, generator=torch.Generator().manual_seed(21)) * 2 - 1
    segm = synthetic.parsing_batch(B, seed=77)['segm']
    enc = hier.encode_photo(image, segm)
    region = torch.zeros(B, 1, 512, 256, dtype=torch.uint8)
    region[0, 0, 200:331, 60:171] = 1           # not aligned to the 16-pixel cells
    region[0, 0, 100:140, 30:50] = 1
    region[1, 0, 300:420, 100:256] = 1          # touches the right border
    model.feed_data(dict(segm=segm, texture_mask=enc['texture_mask']))
    model.sample_steps = 16
    return dict(model=model, image=image, enc=enc, region=region, B=B)


def _edit(photo, **kw):
    model, enc = photo['model'], photo['enc']
    seed_all(9)
    res = model.edit_and_refine(enc['top_indices_list'], region=photo['region'],
                                bot_indices_list=enc['bot_indices_list'], **kw)
    return (res, torch.stack(model.edit_top_indices_list).clone(), torch.stack(model.edit_bot_indices_list).clone(),
            _gen().get_offset())


def test_edit_with_source_image_returns_the_composite(photo, tmp_path):
    from PIL import Image
    model, image, enc, B = photo['model'], photo['image'], photo['enc'], photo['B']
    names = ['a.png', 'b.png']
    plain, top0, bot0, off0 = _edit(photo, save_dir=str(tmp_path), img_name=names)
    u8, top, bot, off = _edit(photo, save_dir=str(tmp_path), img_name=names, source_image=image)
    # compositing does not disturb sampling: same tokens, same generator offset
    assert torch.equal(top, top0) and torch.equal(bot, bot0) and off == off0
    keep = model.edit_keep
    assert keep.dtype == torch.uint8 and tuple(keep.shape) == (B, 512)
    assert torch.equal(keep, model.region_keep(region=photo['region'])) and 0 < int((keep == 0).sum()) < B * 512
    # ... and is composite() of the decoded edit, byte for byte
    bot_enc = torch.stack([t.reshape(-1) for t in enc['bot_indices_list']]).to(DEV).contiguous()
    dec_img, dec_u8 = model.decode_indices(model.edit_top_indices_list, want_u8=True,
                                           bot_keep=(bot_enc, keep.reshape(-1).contiguous()))
    assert torch.equal(dec_u8, plain)
    want_img, want_u8 = model.composite(dec_img, image, keep, want_u8=True)
    assert u8.dtype == torch.uint8 and tuple(u8.shape) == (B, 512, 256, 3) and torch.equal(u8, want_u8)
    for i, nm in enumerate(names):
        assert np.array_equal(np.asarray(Image.open(os.path.join(str(tmp_path), nm))), u8[i].cpu().numpy())
    # farther than blend_lo from every edited cell: the photo's own pixels, exactly; inside the cells: the decoder's
    d = torch.from_numpy(C.distance(keep, 32, 16, 16))
    p = C.photo01(image)
    p8 = (p * 255 + 0.5).clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1)
    far, inside = d >= 32, d == 0
    assert far.any() and inside.any()
    assert torch.equal(u8.cpu()[far], p8[far]) and torch.equal(u8.cpu()[inside], plain.cpu()[inside])
    assert torch.equal(want_img.cpu()[far[:, None].expand(-1, 3, -1, -1)], p[far[:, None].expand(-1, 3, -1, -1)])
    assert not torch.equal(u8, plain)
    # other radii without resampling
    img2, _ = model.composite(dec_img, image, keep, blend_hi=2, blend_lo=16)
    ref2 = C.composite(dec_img, image, keep, (32, 16), 2, 16)
    assert (img2.cpu().double() - ref2['out']).abs().max().item() <= C.TOL
    # the no-files form: the composite of the first image.  Its decode runs at batch 1, so against image 0 of the
    # batch form it is held to the decode's activation tolerance, and to the photo's bits where only the photo shows
    first, top1, bot1, off1 = _edit(photo, source_image=image)
    assert tuple(first.shape) == (1, 3, 512, 256) and torch.equal(top1, top0) and torch.equal(bot1, bot0[:, :1])
    err = (first - want_img[:1]).abs().max().item()
    print(f'no-files form vs image 0 of the batch form: max abs diff {err:.3e}')
    assert err <= ACT_TOL
    f0 = far[:1, None].expand(-1, 3, -1, -1)
    assert torch.equal(first.cpu()[f0], p[:1][f0])


def test_wrong_source_shape_and_radii_raise_before_anything_is_drawn(photo):
    model, image, enc = photo['model'], photo['image'], photo['enc']
    assert SampleFromPoseModel.composite is SampleFromParsingModel.composite
    seed_all(3)
    off = _gen().get_offset()
    kw = dict(region=photo['region'], bot_indices_list=enc['bot_indices_list'])
    with pytest.raises(ValueError, match=r'\(2, 3, 256, 256\)'):
        model.edit_and_refine(enc['top_indices_list'], source_image=image[:, :, :256], **kw)
    with pytest.raises(ValueError, match=r'\(1, 3, 512, 256\)'):
        model.edit_and_refine(enc['top_indices_list'], source_image=image[:1], **kw)
    with pytest.raises(ValueError, match='blend_hi'):
        model.edit_and_refine(enc['top_indices_list'], source_image=image, blend_hi=33, blend_lo=32, **kw)
    assert _gen().get_offset() == off
    keep = model.region_keep(region=photo['region'])
    img = torch.zeros(2, 3, 512, 256, device=DEV)
    with pytest.raises(ValueError, match=r'\(2, 3, 1024, 512\)'):
        model.composite(torch.zeros(2, 3, 1024, 512, device=DEV), image, keep)      # an upscale=True image
    with pytest.raises(ValueError, match=r'keep must be \[2, 512\]'):
        model.composite(img, image, keep[:1])
    with pytest.raises(ValueError, match='blend_hi'):
        model.composite(img, image, keep, blend_hi=5, blend_lo=4)
