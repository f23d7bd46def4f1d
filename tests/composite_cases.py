"""The kernel cases of t2h_composite_region_f32, written once against a `run` callable and executed on
the host emulator (tests/test_composite_emulated.py) and on the device (tests/test_gpu_composite.py).

run(dec, photo, keep, cells, r_hi, r_lo, want_u8=False) -> (out f32 [B, 3, H, W], u8 [B, H, W, 3] or None), CPU tensors;
dec / photo / keep are CPU tensors, the photo is in the signed range.  Every case compares with tests/composite_ref.py
(float64) at composite_ref.TOL, a bound derived there, and checks the two exact areas bit for bit."""
import numpy as np
import torch

import composite_ref as C

CELL, TH, TW, B = 16, 6, 5, 3          # 96 x 80: two and a half 32-pixel tiles wide, three tall
H, W = CELL * TH, CELL * TW
INTERIOR = [[(2, 2)], [(3, 1)], [(1, 3)]]
BORDERS = [[(0, 0), (0, TW - 1), (TH - 1, 0), (TH - 1, TW - 1)],           # every corner
           [(0, 2), (3, 0), (TH - 1, 2), (2, TW - 1)],                     # every border
           [(0, 0), (2, 2), (TH - 1, 3)]]


def _bits(t):
    return t.contiguous().view(torch.int32)


def check(run, dec, photo, keep, cells, r_hi, r_lo, want_u8=False, need_exact_areas=True):
    """one run against the reference: TOL everywhere, dec's bits where d == 0, p's bits where d >= r_lo -> (out, ref)"""
    out, u8 = run(dec, photo, keep, cells, r_hi, r_lo, want_u8=want_u8)
    ref = C.composite(dec, photo, keep, cells, r_hi, r_lo)
    err = (out.double() - ref['out']).abs().max().item()
    print(f'composite {tuple(dec.shape)} r_hi {r_hi} r_lo {r_lo}: max abs err {err:.3e} (bound {C.TOL:.0e})')
    assert err <= C.TOL, err
    d = torch.from_numpy(ref['d'])[:, None].expand_as(out)
    inside, far = d == 0, d >= r_lo
    if need_exact_areas:
        assert inside.any() and far.any()
    assert torch.equal(_bits(out)[inside], _bits(dec)[inside])
    assert torch.equal(_bits(out)[far], _bits(ref['p'])[far])
    if want_u8:
        excluded = C.check_u8(u8, ref)
        print(f'  uint8: {excluded:.4f} of the bytes excluded as boundary cases of the reference')
    return out, ref


def case_a_b_h_interior(run):
    dec, photo = C.inputs(B, H, W, seed=11)
    check(run, dec, photo, C.keep_of(B, TH, TW, INTERIOR), (TH, TW), 4, 32, want_u8=True)


def case_c_borders(run):
    dec, photo = C.inputs(B, H, W, seed=12)
    check(run, dec, photo, C.keep_of(B, TH, TW, BORDERS), (TH, TW), 4, 32, want_u8=True)


def case_d_none_all_mixed(run):
    dec, photo = C.inputs(B, H, W, seed=13)
    keep = C.keep_of(B, TH, TW, [[], 'all', [(1, 1), (4, 3)]])
    out, ref = check(run, dec, photo, keep, (TH, TW), 4, 32, want_u8=True)
    assert torch.equal(_bits(out[0]), _bits(ref['p'][0]))      # no edited cell: the photo
    assert torch.equal(_bits(out[1]), _bits(dec[1]))           # all cells edited: the decoder's image


def case_e_batch_independence(run):
    dec, photo = C.inputs(B, H, W, seed=14)
    keep = C.keep_of(B, TH, TW, [[(2, 2)], [(0, 4), (5, 0)], [(3, 3), (3, 4)]])
    out, u8 = run(dec, photo, keep, (TH, TW), 4, 32, want_u8=True)
    for b in range(B):
        one, one8 = run(dec[b:b + 1].contiguous(), photo[b:b + 1].contiguous(), keep[b:b + 1].contiguous(), (TH, TW), 4,
                        32, want_u8=True)
        assert torch.equal(_bits(out[b:b + 1]), _bits(one)) and torch.equal(u8[b:b + 1], one8), b


def case_f_radii(run):
    dec, photo = C.inputs(B, H, W, seed=15)
    keep = C.keep_of(B, TH, TW, INTERIOR)
    # r_hi == r_lo: the low band drops out, out = p + w diff
    out, ref = check(run, dec, photo, keep, (TH, TW), 16, 16)
    p, w = ref['p'].double(), ref['w_lo']
    plain = (p + w * (dec.double() - p)).clamp(0, 1)
    band = (torch.from_numpy(ref['d'])[:, None] > 0).expand_as(out)
    assert (out.double() - plain)[band].abs().max().item() <= C.TOL
    # the widest halo (R = 32) under the narrowest detail band
    assert len(C.composite_taps_host(64)) == 65
    check(run, dec, photo, keep, (TH, TW), 1, 64, need_exact_areas=False)
    # cell = 8 (12 x 10 cells of the same 96 x 80 image), r_lo = 8
    keep8 = C.keep_of(B, 12, 10, [[(5, 5), (0, 0)], [(11, 9), (6, 0)], [(3, 7), (3, 8), (4, 8)]])
    check(run, dec, photo, keep8, (12, 10), 4, 8)


def _offset_inputs(seed, sign):
    """photo with p in [0.1, 0.9] and dec = p + 0.1 sign (fp32), sign +1 / -1 per pixel or a scalar"""
    g = torch.Generator().manual_seed(seed)
    photo = torch.rand(B, 3, H, W, generator=g) * 1.6 - 0.8
    return (C.photo01(photo) + 0.1 * sign).contiguous(), photo


def case_g_uniform_offset(run):
    r_hi, r_lo = 4, 32
    dec, photo = _offset_inputs(16, 1.0)
    keep = C.keep_of(B, TH, TW, INTERIOR)
    out, ref = check(run, dec, photo, keep, (TH, TW), r_hi, r_lo)
    delta = out.double() - ref['p'].double()
    assert (delta - 0.1 * ref['w_lo']).abs().max().item() <= C.TOL       # the offset fades linearly over r_lo ...
    outside = (torch.from_numpy(ref['d'])[:, None] > 0).expand_as(delta)
    jump = 0.0
    for dim in (2, 3):                                                   # ... so no step between 4-neighbours: no seam
        a, b_ = delta.narrow(dim, 0, delta.shape[dim] - 1), delta.narrow(dim, 1, delta.shape[dim] - 1)
        both = outside.narrow(dim, 0, delta.shape[dim] - 1) & outside.narrow(dim, 1, delta.shape[dim] - 1)
        jump = max(jump, (a - b_).abs()[both].max().item())
    print(f'largest step of out - p between neighbours outside the edit: {jump:.3e} (bound {0.1 / r_lo + 4e-5:.3e})')
    assert jump <= 0.1 / r_lo + 4e-5


def case_g_checkerboard(run):
    r_hi, r_lo = 4, 32
    ys, xs = torch.arange(H)[:, None], torch.arange(W)[None, :]
    sign = (1 - 2 * ((ys + xs) % 2)).float()[None, None]
    dec, photo = _offset_inputs(17, sign)
    keep = C.keep_of(B, TH, TW, INTERIOR)
    out, ref = check(run, dec, photo, keep, (TH, TW), r_hi, r_lo)
    # beyond r_hi the checkerboard is gone, up to what the blur lets through: away from the image border (where
    # replicate padding breaks the alternation) |low| = 0.1 (sum of +-taps)^2 <= 0.1 |sum of +-taps|
    taps = C.composite_taps_host(r_lo).astype(np.float64)
    R = (len(taps) - 1) // 2
    leak = abs(float((taps * (1 - 2 * (np.arange(len(taps)) % 2))).sum()))
    d = torch.from_numpy(ref['d'])[:, None].expand_as(out)
    core = torch.zeros_like(d, dtype=torch.bool)
    core[:, :, R:H - R, R:W - R] = True
    sel = core & (d >= r_hi)
    assert sel.any() and (sel & (d < r_lo)).any()
    resid = (out.double() - ref['p'].double()).abs()[sel].max().item()
    print(f'checkerboard residue beyond r_hi: {resid:.3e} (bound {0.1 * leak + 4e-5:.3e})')
    assert resid <= 0.1 * leak + 4e-5
    # and everywhere in that core: |out - p| <= 0.1 (w_hi + 2 (1 - w_hi) |sum of +-taps|)
    bound = 0.1 * (ref['w_hi'] + 2 * (1 - ref['w_hi']) * leak) + 4e-5
    assert ((out.double() - ref['p'].double()).abs() <= bound.expand_as(out))[core].all()


def ragged_region(th, tw, seed, n_cells=40):
    """a connected, ragged blob of about n_cells cells grown from a seed cell (deterministic)"""
    g = torch.Generator().manual_seed(seed)
    cells = {(th // 2, tw // 2)}
    while len(cells) < n_cells:
        r, c = sorted(cells)[int(torch.randint(0, len(cells), (1, ), generator=g))]
        dr, dc = [(-1, 0), (1, 0), (0, -1), (0, 1)][int(torch.randint(0, 4, (1, ), generator=g))]
        if 0 <= r + dr < th and 0 <= c + dc < tw:
            cells.add((r + dr, c + dc))
    return sorted(cells)


ALL_CASES = [case_a_b_h_interior, case_c_borders, case_d_none_all_mixed, case_e_batch_independence, case_f_radii,
             case_g_uniform_offset, case_g_checkerboard]
