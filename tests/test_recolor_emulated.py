"""csrc/recolor.hip on the host emulator (tests/emu): the sources of t2h_region_color_stats and t2h_recolor_region_f32
run with real concurrent threads against the float64 restatement of tests/recolor_ref.py -- the membership rule, the
statistics' fixed summation order, the integer tent sums packed into bytes and 16-bit fields, tile classification and
its two shortcuts, the halo hanging off the image, ragged tiles, the untouched area bit for bit and the uint8 rule
(DESIGN.md 4.6l).  The cases live in tests/recolor_cases.py; tests/test_gpu_recolor.py runs the same ones on the
device."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'emu'))
import build_emu  # noqa: E402
import recolor_cases as cases  # noqa: E402
import recolor_ref as R  # noqa: E402

pytestmark = pytest.mark.skipif(not build_emu.available(), reason='no host clang++ for the emulation build')


@pytest.fixture(scope='module')
def lib():
    return build_emu.load('recolor.hip')


@pytest.fixture(scope='module')
def run(lib):
    return cases.Runner(lib, 'cpu', lambda: None, lib.emu_last_error)


@pytest.mark.parametrize('case', cases.ALL_CASES, ids=lambda f: f.__name__)
def test_kernel_case(run, case):
    case(run)


def test_reference_keeps_few_bytes_on_a_rounding_boundary():
    # uniform-random inputs: about 2 * U8_MARGIN = 0.6 % of the reference's own bytes lie within the margin of a
    # boundary (plus the clamped ones, which sit on 0.5 exactly): near 1 %, far under check_u8's cap of 5 %
    img = cases.image(2, cases.H, cases.W, 20)
    segm = cases.segm_of(2, cases.H, cases.W, [[(1, 10, 50, 10, 50), (3, 50, 90, 10, 50)], [(2, 30, 70, 40, 80)]])
    bits = [cases.UP, cases.LO, cases.OU]
    st = R.stats(img, segm, bits)
    ref = R.recolor(img, segm, bits, st, R.plain_target(st, (0.5, 0.45, 0.55)))
    share = R.u8_excluded(ref)
    print(f'share of the reference\'s bytes within {R.U8_MARGIN} of a rounding boundary: {share:.4f}')
    assert 0.002 <= share <= 0.02
    assert R.U8_MARGIN > 255 * R.TOL


def test_arguments_are_validated(lib):
    x = torch.zeros(1, 3, 32, 32)
    s = torch.ones(1, 32, 32)
    st = torch.zeros(1, 2, 8, dtype=torch.float64)
    part = torch.zeros(1, 2, 2, 8, dtype=torch.float64)
    o = torch.zeros_like(x)
    two = (ctypes.c_uint64 * 2)(0b10010, 0b101000)

    def apply(img=x, segm=s, bits=two, G=2, src=st, dst=st, luma=1.0, gain_max=4.0, feather=2, out=o, B=1, H=32, W=32):
        ptr = [None if a is None else a.data_ptr() for a in (img, segm, src, dst, out)]
        return lib.t2h_recolor_region_f32(ptr[0], 0, ptr[1], bits, G, ptr[2], ptr[3], luma, gain_max, feather, ptr[4], None,
                                          B, H, W, None)

    assert apply() == 0, lib.emu_last_error()
    overlap = (ctypes.c_uint64 * 2)(0b10010, 0b10000)
    for kw in (dict(img=None), dict(segm=None), dict(bits=None), dict(src=None), dict(dst=None), dict(out=None),
               dict(out=x), dict(G=0), dict(G=5), dict(bits=overlap), dict(feather=-1), dict(feather=9), dict(luma=-0.01),
               dict(luma=1.01), dict(luma=float('nan')), dict(gain_max=0.99), dict(gain_max=16.5),
               dict(gain_max=float('nan')), dict(B=0), dict(H=0), dict(W=-1)):
        assert apply(**kw) == -1, kw

    def stats(img=x, segm=s, bits=two, G=2, partial=part, out=st, B=1, H=32, W=32):
        ptr = [None if a is None else a.data_ptr() for a in (img, segm, partial, out)]
        return lib.t2h_region_color_stats(ptr[0], 0, ptr[1], bits, G, B, H, W, ptr[2], ptr[3], None)

    assert stats() == 0, lib.emu_last_error()
    for kw in (dict(img=None), dict(segm=None), dict(bits=None), dict(partial=None), dict(out=None), dict(G=0), dict(G=5),
               dict(bits=overlap), dict(B=0), dict(H=0), dict(W=0)):
        assert stats(**kw) == -1, kw


def test_partial_rows_are_one_per_stripe_and_group(lib):
    # the documented workspace: f64 [B][ceil(H / 16)][G][8], every row written, its sums those of the stripe's rows
    img = cases.image(2, 40, 27, 31)
    segm = cases.segm_of(2, 40, 27, [[(1, 0, 40, 0, 27)], [(3, 14, 35, 2, 20)]])
    bits = (ctypes.c_uint64 * 2)(cases.UP, cases.LO)
    part = torch.full((2, 3, 2, 8), float('nan'), dtype=torch.float64)
    st = torch.zeros(2, 2, 8, dtype=torch.float64)
    assert lib.t2h_region_color_stats(img.data_ptr(), 0, segm.data_ptr(), bits, 2, 2, 40, 27, part.data_ptr(), st.data_ptr(),
                                      None) == 0
    assert not torch.isnan(part).any()
    assert part[0, :, 0, 0].tolist() == [16 * 27, 16 * 27, 8 * 27] and part[1, :, 1, 0].tolist() == [2 * 18, 16 * 18, 3 * 18]
    assert np.array_equal(part[..., 0].sum(1).numpy(), st[..., 0].numpy())
