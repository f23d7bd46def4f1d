"""The all-codebook fit, the region vote and the un-annotated photo flow on the GPU (-m gpu):
t2h_vq_fit_books_f32 / t2h_texture_vote against tests/fit_ref.py (float64), then infer_texture_attributes /
encode_photo of the hierarchy model on synthetic checkpoints.

The bounds are fit_ref's derived rounding bound; who is excused from an exact-argmin or exact-decision comparison is
decided by the float64 reference alone (its gap against that bound)."""
import numpy as np
import pytest
import torch

import fit_ref as ref
from text2human_amd import defaults, ops, options, synthetic
from text2human_amd.models import SampleFromParsingModel

pytestmark = pytest.mark.gpu
DEV = 'cuda'
PAD = 64
D = 256
SHAPES = {'full': (519, 18, 1024), 'small': (33, 3, 96)}
TILES = [0, 32, 64, 128]


def _padded(n, dtype, fill):
    whole = torch.full((n + 2 * PAD, ), fill, dtype=dtype, device=DEV)
    return whole, whole[PAD:PAD + n]


def _untouched(whole, fill):
    return bool((whole[:PAD] == fill).all()) and bool((whole[-PAD:] == fill).all())


def fit(z, books, want_index=True, tile=0):
    """through the C ABI into sentinel-padded buffers -> numpy (dmin [n, nb], jmin [n, nb] or None)"""
    from text2human_amd import _lib
    z, books = torch.as_tensor(z).to(DEV).contiguous(), torch.as_tensor(books).to(DEV).contiguous()
    n, (nb, n_e, d) = z.shape[0], books.shape
    wd, dmin = _padded(n * nb, torch.float32, 777.0)
    wj, jmin = _padded(n * nb, torch.int32, -99)
    old = ops.vq_fit_force_tile(tile)
    try:
        _lib.check(_lib.load().t2h_vq_fit_books_f32(ops._p(z), ops._p(books), ops._p(dmin), ops._p(jmin) if want_index else None,
                                                    n, nb, n_e, d, ops._stream()), 't2h_vq_fit_books_f32')
    finally:
        ops.vq_fit_force_tile(old)
    torch.cuda.synchronize()
    assert _untouched(wd, 777.0) and _untouched(wj, -99)
    if not want_index:
        assert bool((jmin == -99).all())
    return dmin.view(n, nb).cpu().numpy(), jmin.view(n, nb).cpu().numpy() if want_index else None


@pytest.fixture(scope='module')
def problems():
    """name -> (z, books, {tile: (dmin, jmin)}); the reference is evaluated inside check_fit, once per problem"""
    out = {}
    for i, (name, (n, nb, n_e)) in enumerate(SHAPES.items()):
        rs = np.random.RandomState(40 + i)
        z = rs.standard_normal((n, D)).astype(np.float32)
        books = rs.standard_normal((nb, n_e, D)).astype(np.float32)
        out[name] = (z, books, {t: fit(z, books, tile=t) for t in TILES})
    return out


@pytest.mark.parametrize('name', list(SHAPES))
def test_fit_against_float64(problems, name):
    z, books, outs = problems[name]
    dmin, jmin = outs[0]
    excused = ref.check_fit(z, books, dmin, jmin, max_excused=0.01)
    print(f'{name} {SHAPES[name]}: excused share {excused:.5f}')
    for t in TILES[1:]:   # the row tile changes no bit
        assert outs[t][0].tobytes() == dmin.tobytes() and outs[t][1].tobytes() == jmin.tobytes(), t


@pytest.mark.parametrize('name', list(SHAPES))
def test_run_to_run_and_without_index(problems, name):
    z, books, outs = problems[name]
    again = fit(z, books)
    assert again[0].tobytes() == outs[0][0].tobytes() and again[1].tobytes() == outs[0][1].tobytes()
    d2, none = fit(z, books, want_index=False)
    assert none is None and d2.tobytes() == outs[0][0].tobytes()


def test_row_alone_equals_row_in_the_batch(problems):
    z, books, outs = problems['full']
    dmin, jmin = outs[0]
    for r in (0, 127, 518):
        d1, j1 = fit(z[r:r + 1], books)
        assert d1.tobytes() == dmin[r:r + 1].tobytes() and j1.tobytes() == jmin[r:r + 1].tobytes(), r
    perm = np.random.RandomState(7).permutation(z.shape[0])
    dp, jp = fit(z[perm], books, tile=64)
    assert dp.tobytes() == dmin[perm].tobytes() and jp.tobytes() == jmin[perm].tobytes()


@pytest.mark.parametrize('name', list(SHAPES))
def test_tie_planted_and_nan_rows(problems, name):
    z, books, outs = problems[name]
    nb = books.shape[0]
    books = books.copy()
    books[1, 70] = books[1, 5]
    rs = np.random.RandomState(9)
    planted = (books[:, :8].reshape(8 * nb, D) + 1e-3 * rs.standard_normal((8 * nb, D))).astype(np.float32)
    zz = np.concatenate([z[:5], books[1, 5][None], planted]).astype(np.float32)      # row 5: the exact tie
    zz[2, 100] = np.nan
    zz[3, 7] = np.inf
    others = [h for h in range(nb) if h != 1]                                       # (book 1 was edited)
    for tile in TILES:
        dmin, jmin = fit(zz, books, tile=tile)
        assert jmin[5, 1] == 5
        assert (dmin[6:].argmin(1) == np.repeat(np.arange(nb), 8)).all()
        for r in (2, 3):
            assert np.isposinf(dmin[r]).all() and (jmin[r] == -1).all()
        keep = np.array([0, 1, 4])
        assert dmin[keep][:, others].tobytes() == outs[0][0][keep][:, others].tobytes()
        assert np.isfinite(np.delete(dmin, (2, 3), 0)).all()


def test_other_widths_are_an_error():
    from text2human_amd._lib import T2HError
    with pytest.raises(T2HError, match='d=64'):
        ops.vq_fit_books(torch.zeros(4, 64, device=DEV), torch.zeros(2, 8, 64, device=DEV))


@pytest.mark.parametrize('B,T', [(1, 512), (3, 512), (3, 15)])
def test_vote_bitwise(B, T):
    rs = np.random.RandomState(B * 1000 + T)
    dmin = (400.0 + 50.0 * rs.random_sample((B * T, 18))).astype(np.float32)
    dmin[rs.randint(0, B * T, 5), rs.randint(0, 18, 5)] = np.inf
    segm = rs.choice([0, 1, 2, 3, 4, 5, 13, 21, 23], size=(B, T)).astype(np.int64)
    if B > 1:
        segm[1][segm[1] == 2] = 0                                     # an absent group
    want = ref.vote(dmin, segm)
    got = ops.texture_vote(torch.from_numpy(dmin).to(DEV), torch.from_numpy(segm).to(DEV), B)
    for g, w in zip(got, want):
        assert g.cpu().numpy().dtype == w.dtype and g.cpu().numpy().tobytes() == w.tobytes()
    for b in range(B):                                                # an image alone = the image in the batch
        one = ops.texture_vote(torch.from_numpy(dmin[b * T:(b + 1) * T]).to(DEV), torch.from_numpy(segm[b:b + 1]).to(DEV), 1)
        for g, w in zip(one, got):
            assert torch.equal(g, w[b:b + 1])


# ------------------------------------------------------------------------------------------------ model level
KEYS = ('upper_fused_attr', 'lower_fused_attr', 'outer_fused_attr')


@pytest.fixture(scope='module')
def photo():
    opt = options.dict_to_nonedict(defaults.sample_from_parsing())
    sds = synthetic.make_state_dicts(opt, seed=1234, encode=True)
    from text2human_amd.models import VQGANTextureAwareSpatialHierarchyInferenceModel as M
    hier = M(opt, state_dicts=sds)
    B = 2
    image = torch.rand(B, 3, 512, 256, generator=torch.Generator().manual_seed(21)) * 2 - 1
    segm = synthetic.parsing_batch(B, seed=77)['segm']
    rng = torch.cuda.get_rng_state()
    inferred = hier.infer_texture_attributes(image, segm, return_costs=True)
    latents = hier._top_latent_rows.clone()
    enc = hier.encode_photo(image, segm)
    assert torch.equal(torch.cuda.get_rng_state(), rng)
    return dict(opt=opt, sds=sds, hier=hier, image=image, segm=segm, inferred=inferred, latents=latents, enc=enc)


def test_inferred_attributes_against_float64(photo):
    hier, out = photo['hier'], photo['inferred']
    segm_tok = photo['segm'][:, 0, ::16, ::16].reshape(2, -1).long().numpy()
    cost64, tolsum, count, attr64, decided = ref.region_costs64(photo['latents'].cpu().numpy(),
                                                                hier.P['top.books'].cpu().numpy(), segm_tok)
    cost, cnt = out['cost'].cpu().numpy(), out['count'].cpu().numpy()
    attr = np.stack([out[k].cpu().numpy() for k in KEYS], 1)
    assert cost.dtype == np.float64 and cost.shape == (2, 3, 18) and cnt.dtype == np.int32 and attr.dtype == np.int64
    print('count', cnt.tolist(), 'attr', attr.tolist(), 'float64 attr', attr64.tolist(), 'decided', decided.tolist())
    print('max |cost - cost64| / summed tol', float((np.abs(cost - cost64) / np.maximum(tolsum, 1e-300))[cnt > 0].max()))
    assert (cnt == count).all()
    assert (np.abs(cost - cost64) <= tolsum).all()
    assert (~decided).sum() <= 1
    assert (attr[decided] == attr64[decided]).all()
    assert (cnt > 0).any()


def test_mask_and_lists_are_todays_path_for_the_returned_mask(photo):
    hier, enc, inferred = photo['hier'], photo['enc'], photo['inferred']
    for k in KEYS + ('texture_mask', ):
        assert torch.equal(enc[k], inferred[k]), k
        assert enc[k].is_cuda
    mask = enc['texture_mask']
    assert mask.dtype == torch.float32 and mask.shape == photo['segm'].shape
    assert torch.equal(mask.cpu(), synthetic.texture_mask_from_segm(photo['segm'], *(enc[k].cpu() for k in KEYS)))
    top, bot = enc['top_indices_list'].clone(), [t.clone() for t in enc['bot_indices_list']]
    assert top.shape == (18, 2 * 512) and len(bot) == 18 and bot[0].shape == (2, 32, 16)
    hier.top_encode(photo['image'], mask)
    assert torch.equal(hier.top_indices_list, top)
    for a, b in zip(hier.bot_encode(photo['image'], mask), bot):
        assert torch.equal(a, b)


def test_given_attributes_are_todays_path(photo):
    hier = photo['hier']
    given = dict(upper_fused_attr=torch.tensor([3, 17]), lower_fused_attr=torch.tensor([0, 16]),
                 outer_fused_attr=torch.tensor([17, 9]))
    mask = synthetic.texture_mask_from_segm(photo['segm'], *(given[k] for k in KEYS))
    hier.top_encode(photo['image'], mask)
    top = hier.top_indices_list.clone()
    bot = hier.bot_encode(photo['image'], mask)
    enc = hier.encode_photo(photo['image'], photo['segm'], attrs=given)
    assert torch.equal(enc['texture_mask'].cpu(), mask)
    assert torch.equal(enc['top_indices_list'], top)
    assert all(torch.equal(a, b) for a, b in zip(enc['bot_indices_list'], bot))
    assert all(torch.equal(enc[k].cpu(), given[k]) for k in KEYS)


def test_each_image_equals_its_own_call(photo):
    hier, whole, enc = photo['hier'], photo['inferred'], photo['enc']
    for b in range(2):
        one = hier.infer_texture_attributes(photo['image'][b:b + 1], photo['segm'][b:b + 1], return_costs=True)
        for k in KEYS + ('texture_mask', 'cost', 'count'):
            assert torch.equal(one[k], whole[k][b:b + 1]), (b, k)
        e1 = hier.encode_photo(photo['image'][b:b + 1], photo['segm'][b:b + 1])
        assert torch.equal(e1['top_indices_list'], enc['top_indices_list'].view(18, 2, 512)[:, b])
        assert all(torch.equal(a, w[b:b + 1]) for a, w in zip(e1['bot_indices_list'], enc['bot_indices_list']))


def test_encoded_photo_feeds_region_editing(photo):
    model = SampleFromParsingModel(photo['opt'], state_dicts=photo['sds'])
    enc = photo['enc']
    model.feed_data(dict(segm=photo['segm'], texture_mask=enc['texture_mask']))
    model.sample_steps = 8
    img = model.edit_and_refine(enc['top_indices_list'], labels=(1, 2, 3), bot_indices_list=enc['bot_indices_list'])
    assert img.shape == (1, 3, 512, 256) and bool(torch.isfinite(img).all())
