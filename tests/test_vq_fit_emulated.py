"""The all-codebook fit and the region vote on the CPU: t2h_vq_fit_books_f32 and t2h_texture_vote of
csrc/vq_fit.hip through tests/emu against tests/fit_ref.py.

Pinned here: the distance and the argmin against float64 within the derived rounding bound (row-tile tail, code-tile
tail, one row alone; every row tile the launch can choose), the first-index tie rule, that a row's outputs are a
function of the row and the books alone (alone = inside a 130-row call, bit for bit; a permutation of the rows
permutes the outputs), NaN rows, sentinels around both outputs (with and without jmin), and the vote byte for byte."""
import ctypes
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, 'emu'))
sys.path.insert(0, HERE)
import build_emu  # noqa: E402
import fit_ref as ref  # noqa: E402

pytestmark = pytest.mark.skipif(not build_emu.available(), reason='no host clang++ for the emulation build')

PAD = 64  # sentinel elements on either side of every output
D = 256
SHAPES = [(1, 3, 96), (33, 3, 96), (130, 2, 300)]  # row-tile tail, code-tile tail, one row alone
TILES = [0, 64, 128]                               # 0 = the launch's own choice (32 rows at these sizes)
BIG_TILES = [0, 128]                               # the 130-row problem at 64 rows: the permutation test


@pytest.fixture(scope='module')
def lib():
    from text2human_amd import _lib
    so = build_emu.load('vq_fit.hip')
    for name in ('t2h_vq_fit_books_f32', 't2h_vq_fit_force_tile', 't2h_texture_vote'):
        assert getattr(so, name).argtypes == _lib.SIGNATURES[name][1]
    return so


def _padded(n, dtype, fill):
    """(whole buffer, the n elements in its middle) -- the rest are sentinels"""
    whole = np.full((n + 2 * PAD, ), fill, dtype=dtype)
    return whole, whole[PAD:PAD + n]


def _untouched(whole, fill):
    return bool((whole[:PAD] == fill).all()) and bool((whole[-PAD:] == fill).all())


def _ptr(a):
    return ctypes.c_void_p(a.ctypes.data)


def _aligned(a):
    """a 16-byte aligned float32 copy"""
    raw = np.empty(a.size + 4, np.float32)
    off = (-raw.ctypes.data // 4) % 4
    out = raw[off:off + a.size].reshape(a.shape)
    out[...] = a
    assert out.ctypes.data % 16 == 0
    return out


def fit(lib, z, books, want_index=True, tile=0):
    z, books = _aligned(z), _aligned(books)
    n, (nb, n_e, d) = z.shape[0], books.shape
    wd, dmin = _padded(n * nb, np.float32, 777.0)
    wj, jmin = _padded(n * nb, np.int32, -99)
    old = lib.t2h_vq_fit_force_tile(tile)
    try:
        rc = lib.t2h_vq_fit_books_f32(_ptr(z), _ptr(books), _ptr(dmin), _ptr(jmin) if want_index else None, n, nb, n_e, d,
                                      None)
    finally:
        lib.t2h_vq_fit_force_tile(old)
    assert rc == 0, lib.emu_last_error()
    assert _untouched(wd, 777.0) and _untouched(wj, -99)
    if not want_index:
        assert (jmin == -99).all()
    return dmin.reshape(n, nb).copy(), jmin.reshape(n, nb).copy() if want_index else None


def _problem(shape, seed):
    n, nb, n_e = shape
    rs = np.random.RandomState(seed)
    return rs.standard_normal((n, D)).astype(np.float32), rs.standard_normal((nb, n_e, D)).astype(np.float32)


_cache = {}


def _big(lib):
    """the 130-row problem and its outputs (every row tile), computed once"""
    if 'big' not in _cache:
        z, books = _problem(SHAPES[2], 2)
        _cache['big'] = (z, books, {t: fit(lib, z, books, tile=t) for t in BIG_TILES})
    return _cache['big']


@pytest.mark.parametrize('case,tile', [(c, t) for c in (0, 1) for t in TILES] + [(2, t) for t in BIG_TILES])
def test_fit_against_float64(lib, case, tile):
    if case == 2:
        z, books, outs = _big(lib)
        dmin, jmin = outs[tile]
    else:
        z, books = _problem(SHAPES[case], case)
        dmin, jmin = fit(lib, z, books, tile=tile)
    excused = ref.check_fit(z, books, dmin, jmin, max_excused=0.01)
    print(f'shape {SHAPES[case]} tile {tile}: excused {excused:.4f}')


def test_every_tile_gives_the_same_bits(lib):
    _, _, outs = _big(lib)
    for t in BIG_TILES[1:]:
        assert outs[t][0].tobytes() == outs[0][0].tobytes() and outs[t][1].tobytes() == outs[0][1].tobytes(), t


def test_without_index_output(lib):
    z, books = _problem(SHAPES[1], 1)
    dmin, jmin = fit(lib, z, books, want_index=True)
    dmin2, none = fit(lib, z, books, want_index=False)
    assert none is None and dmin2.tobytes() == dmin.tobytes()


def test_exact_tie_goes_to_the_lower_index(lib):
    z, books = _problem((3, 2, 96), 5)
    books[1, 70] = books[1, 5]
    z[1] = books[1, 5]
    for tile in TILES:
        dmin, jmin = fit(lib, z, books, tile=tile)
        assert jmin[1, 1] == 5, (tile, jmin[1])


def test_planted_book_is_found(lib):
    rs = np.random.RandomState(6)
    books = rs.standard_normal((3, 96, D)).astype(np.float32)
    z = (books[:, :12].reshape(36, D) + 1e-3 * rs.standard_normal((36, D))).astype(np.float32)
    dmin, jmin = fit(lib, z, books)
    assert (dmin.argmin(1) == np.repeat(np.arange(3), 12)).all()
    assert (jmin[np.arange(36), np.repeat(np.arange(3), 12)] == np.tile(np.arange(12), 3)).all()


def test_row_alone_equals_row_in_the_batch(lib):
    z, books, outs = _big(lib)
    dmin, jmin = outs[0]
    for r, tile in ((31, 0), (129, 64)):
        d1, j1 = fit(lib, z[r:r + 1], books, tile=tile)
        assert d1.tobytes() == dmin[r:r + 1].tobytes() and j1.tobytes() == jmin[r:r + 1].tobytes(), r


def test_row_permutation_permutes_the_outputs(lib):
    z, books, outs = _big(lib)
    dmin, jmin = outs[0]
    perm = np.random.RandomState(7).permutation(z.shape[0])
    dp, jp = fit(lib, z[perm], books, tile=64)
    assert dp.tobytes() == dmin[perm].tobytes() and jp.tobytes() == jmin[perm].tobytes()


def test_nan_row_is_flagged_alone(lib):
    z, books = _problem(SHAPES[1], 8)
    clean_d, clean_j = fit(lib, z, books)
    bad = z.copy()
    bad[7, 100] = np.nan
    bad[20, 3] = np.inf
    dmin, jmin = fit(lib, bad, books)
    for r in (7, 20):
        assert np.isposinf(dmin[r]).all() and (jmin[r] == -1).all()
    keep = np.setdiff1d(np.arange(z.shape[0]), [7, 20])
    assert dmin[keep].tobytes() == clean_d[keep].tobytes() and jmin[keep].tobytes() == clean_j[keep].tobytes()


def test_other_widths_are_an_error(lib):
    z = _aligned(np.zeros((4, 64), np.float32))
    books = _aligned(np.zeros((2, 8, 64), np.float32))
    wd, dmin = _padded(8, np.float32, 777.0)
    assert lib.t2h_vq_fit_books_f32(_ptr(z), _ptr(books), _ptr(dmin), None, 4, 2, 8, 64, None) != 0
    assert b'd=64' in lib.emu_last_error()
    assert (wd == 777.0).all()


# ---------------------------------------------------------------------------------------------------------- vote
def vote(lib, dmin, segm_tok):
    B, T = segm_tok.shape
    nb = dmin.shape[1]
    dmin = np.ascontiguousarray(dmin, np.float32)
    segm_tok = np.ascontiguousarray(segm_tok, np.int64)
    wc, cost = _padded(B * 3 * nb, np.float64, -5.0)
    wn, count = _padded(B * 3, np.int32, -99)
    wa, attr = _padded(B * 3, np.int64, -99)
    rc = lib.t2h_texture_vote(_ptr(dmin), _ptr(segm_tok), B, T, nb, _ptr(cost), _ptr(count), _ptr(attr), None)
    assert rc == 0, lib.emu_last_error()
    assert _untouched(wc, -5.0) and _untouched(wn, -99) and _untouched(wa, -99)
    return cost.reshape(B, 3, nb).copy(), count.reshape(B, 3).copy(), attr.reshape(B, 3).copy()


def _vote_problem(B, T, nb, seed):
    rs = np.random.RandomState(seed)
    dmin = (400.0 + 50.0 * rs.random_sample((B * T, nb))).astype(np.float32)
    segm = rs.choice([0, 1, 2, 3, 4, 5, 13, 21, 23], size=(B, T)).astype(np.int64)
    return dmin, segm


def _same(got, want):
    return all(g.dtype == w.dtype and g.tobytes() == w.tobytes() for g, w in zip(got, want))


@pytest.mark.parametrize('B', [1, 3])
@pytest.mark.parametrize('T', [512, 15])
def test_vote_bitwise(lib, B, T):
    dmin, segm = _vote_problem(B, T, 18, 10 * B + T)
    got = vote(lib, dmin, segm)
    assert _same(got, ref.vote(dmin, segm))
    assert (got[1].sum(1) > 0).all()


def test_vote_absent_group_gives_na(lib):
    dmin, segm = _vote_problem(2, 15, 18, 3)
    segm[1][segm[1] == 2] = 0                       # image 1 has no outer garment
    cost, count, attr = got = vote(lib, dmin, segm)
    assert _same(got, ref.vote(dmin, segm))
    assert count[1, 2] == 0 and attr[1, 2] == 17 and (cost[1, 2] == 0.0).all()
    assert count[0, 2] > 0


def test_vote_book_zero_ties_and_infinities(lib):
    T, nb = 15, 18
    segm = np.zeros((1, T), np.int64)
    segm[0, :5], segm[0, 5:10], segm[0, 10:] = 1, 3, 2
    dmin = np.full((T, nb), 10.0, np.float32)
    dmin[:5, 0] = 1.0                               # upper: book 0 wins -> NA
    dmin[5:10, 6] = dmin[5:10, 9] = 2.0             # lower: books 6 and 9 tie -> 6 -> attribute 5
    dmin[10:, :] = np.inf                           # outer: +inf everywhere but book 12 -> attribute 11
    dmin[10:, 12] = 1e30
    cost, count, attr = got = vote(lib, dmin, segm)
    assert _same(got, ref.vote(dmin, segm))
    assert attr.tolist() == [[17, 5, 11]] and count.tolist() == [[5, 5, 5]]
    dmin[10:, 12] = np.inf                          # nothing finite: NA
    assert vote(lib, dmin, segm)[2].tolist() == [[17, 5, 17]]


def test_vote_image_alone_equals_image_in_the_batch(lib):
    dmin, segm = _vote_problem(3, 512, 18, 4)
    whole = vote(lib, dmin, segm)
    for b in range(3):
        alone = vote(lib, dmin[b * 512:(b + 1) * 512], segm[b:b + 1])
        assert _same(alone, tuple(w[b:b + 1] for w in whole)), b
