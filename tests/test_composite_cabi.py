"""t2h_composite_region_f32 in the built library, without a GPU: the symbol is exported and bound, its arguments are
checked before any HIP call, and the host side of ops.composite_region (tap table, radius checks) is what DESIGN.md 4.6k
states."""
import os

import numpy as np
import pytest

from text2human_amd import _lib, build, ops


@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    return _lib.load()


def test_source_is_part_of_the_build():
    assert 'composite.hip' in build.SOURCES and 't2h_composite_region_f32' in _lib.SIGNATURES


def test_argument_validation_without_gpu(lib):
    bad = 0x1000  # (never dereferenced: every call below is rejected on the host)

    def call(dec=bad, photo=bad + 16, keep=bad, taps=bad, out=bad + 32, B=1, H=512, W=256, th=32, tw=16, r_hi=4, r_lo=32,
             R=24):
        return lib.t2h_composite_region_f32(dec, photo, keep, taps, out, None, B, H, W, th, tw, r_hi, r_lo, R, 1, None)

    for kw, word in ((dict(dec=None), b'NULL'), (dict(photo=None), b'NULL'), (dict(keep=None), b'NULL'),
                     (dict(taps=None), b'NULL'), (dict(out=None), b'NULL'), (dict(out=bad), b'alias'),
                     (dict(B=0), b'shape'), (dict(H=500), b'multiple'), (dict(W=250), b'multiple'),
                     (dict(th=16), b'multiple'), (dict(r_hi=0), b'r_hi'), (dict(r_hi=33), b'r_hi'),
                     (dict(r_lo=65), b'r_lo'), (dict(R=-1), b'R'), (dict(R=33), b'R')):
        assert call(**kw) == -1, kw
        assert word in lib.t2h_last_error(), (kw, lib.t2h_last_error())


@pytest.mark.parametrize('r_lo', [1, 4, 8, 16, 32, 43, 64])
def test_tap_table(r_lo):
    t = ops.composite_taps_host(r_lo)
    R = min(32, int(np.ceil(3 * r_lo / 4)))
    assert t.dtype == np.float32 and t.shape == (2 * R + 1, )
    assert abs(float(t.astype(np.float64).sum()) - 1.0) < 65 * 2.0 ** -24
    assert np.array_equal(t, t[::-1]) and t[R] == t.max() and (t > 0).all()
    sigma = r_lo / 4.0
    assert np.isclose(t[R + 1] / t[R], np.exp(-0.5 / sigma ** 2), rtol=1e-6)


@pytest.mark.parametrize('r_hi,r_lo', [(0, 32), (5, 4), (4, 65), (4.0, 32), (True, 32)])
def test_radii_are_checked_on_the_host(r_hi, r_lo):
    with pytest.raises(ValueError, match='r_hi'):
        ops._check_composite_radii(r_hi, r_lo)
