"""csrc/composite.hip on the host emulator (tests/emu): the source of t2h_composite_region_f32 run with real concurrent
threads against the float64 restatement of tests/composite_ref.py -- tile classification, the halo hanging off the
image, replicate borders, the ragged right-hand tiles of a 96 x 80 image (two and a half tiles wide), the LDS hand-off
between the two blur passes, the exact areas bit for bit and the uint8 rule.  The cases live in
tests/composite_cases.py; tests/test_gpu_composite.py runs the same ones on the device."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'emu'))
import build_emu  # noqa: E402
import composite_cases as cases  # noqa: E402
import composite_ref as C  # noqa: E402

pytestmark = pytest.mark.skipif(not build_emu.available(), reason='no host clang++ for the emulation build')


@pytest.fixture(scope='module')
def lib():
    return build_emu.load('composite.hip')


@pytest.fixture(scope='module')
def run(lib):
    def run_(dec, photo, keep, cells, r_hi, r_lo, want_u8=False, photo_signed=True):
        B, _, H, W = dec.shape
        taps = torch.from_numpy(C.composite_taps_host(r_lo))
        out = torch.full_like(dec, float('nan'))
        u8 = torch.full((B, H, W, 3), 7, dtype=torch.uint8) if want_u8 else None
        rc = lib.t2h_composite_region_f32(dec.data_ptr(), photo.data_ptr(), keep.data_ptr(), taps.data_ptr(),
                                          out.data_ptr(), u8.data_ptr() if want_u8 else None, B, H, W, cells[0], cells[1],
                                          r_hi, r_lo, (taps.numel() - 1) // 2, int(photo_signed), None)
        assert rc == 0, lib.emu_last_error()
        assert not torch.isnan(out).any()           # every pixel written
        return out, u8
    return run_


@pytest.mark.parametrize('case', cases.ALL_CASES, ids=lambda f: f.__name__)
def test_kernel_case(run, case):
    case(run)


def test_unsigned_photo_and_width_not_a_multiple_of_four(run):
    # cell = 3, 10 x 9 cells: a 30 x 27 image (the scalar copy path, one ragged tile), photo already in [0, 1]
    th, tw, cell = 10, 9, 3
    g = torch.Generator().manual_seed(21)
    dec, photo = torch.rand(2, 3, th * cell, tw * cell, generator=g), torch.rand(2, 3, th * cell, tw * cell, generator=g)
    keep = C.keep_of(2, th, tw, [[(4, 4)], [(0, 8), (9, 0)]])
    out, u8 = run(dec, photo, keep, (th, tw), 2, 6, want_u8=True, photo_signed=False)
    ref = C.composite(dec, photo, keep, (th, tw), 2, 6, photo_signed=False)
    assert (out.double() - ref['out']).abs().max().item() <= C.TOL
    d = torch.from_numpy(ref['d'])[:, None].expand_as(out)
    assert (d >= 6).any() and torch.equal(out[d >= 6], photo[d >= 6]) and torch.equal(out[d == 0], dec[d == 0])
    C.check_u8(u8, ref)


def test_arguments_are_validated(lib):
    x = torch.zeros(1, 3, 32, 32)
    k = torch.ones(1, 4, dtype=torch.uint8)
    t = torch.ones(1)
    o = torch.zeros_like(x)

    def call(dec=x, photo=x, keep=k, taps=t, out=o, H=32, W=32, th=2, tw=2, r_hi=4, r_lo=32, R=0):
        ptr = [None if a is None else a.data_ptr() for a in (dec, photo, keep, taps, out)]
        return lib.t2h_composite_region_f32(*ptr, None, 1, H, W, th, tw, r_hi, r_lo, R, 1, None)

    assert call() == 0
    for kw in (dict(dec=None), dict(photo=None), dict(keep=None), dict(taps=None), dict(out=None), dict(out=x),
               dict(th=3), dict(tw=5), dict(th=1, tw=2), dict(r_hi=0), dict(r_hi=5, r_lo=4), dict(r_lo=65), dict(R=-1),
               dict(R=33)):
        assert call(**kw) == -1, kw
