"""The kernel cases of t2h_region_color_stats / t2h_recolor_region_f32, written once against a Runner
and executed on the host emulator (tests/test_recolor_emulated.py) and on the device (tests/test_gpu_recolor.py): the
Runner calls the C ABI of whichever library it is given, with tensors on that library's device.  Every case compares
with tests/recolor_ref.py (float64) at recolor_ref.TOL / STATS_TOL, bounds derived there, and checks the untouched
area bit for bit.  Shapes: 96 x 80 (two and a half 32-pixel tiles wide, three tall) and 30 x 27 (width not a multiple
of 4, one ragged tile)."""
import ctypes

import numpy as np
import torch

import recolor_ref as R

H, W = 96, 80
HS, WS = 30, 27
UP, LO, OU = R.bits_of(R.GROUPS['upper']), R.bits_of(R.GROUPS['lower']), R.bits_of(R.GROUPS['outer'])
STRIPE = 16


class Runner:
    """lib: a ctypes handle exporting the two entry points; device: where its pointers live; stream: () -> c_void_p"""

    def __init__(self, lib, device='cpu', stream=lambda: None, last_error=None):
        self.lib, self.device, self.stream, self.last_error = lib, device, stream, last_error

    def _bits(self, bits):
        return (ctypes.c_uint64 * len(bits))(*bits)

    def stats(self, img, segm, bits, img_signed=False):
        B, _, h, w = img.shape
        i, s = img.to(self.device).contiguous(), segm.to(self.device).contiguous()
        partial = torch.full((B, (h + STRIPE - 1) // STRIPE, len(bits), 8), float('nan'), dtype=torch.float64,
                             device=self.device)
        st = torch.full((B, len(bits), 8), float('nan'), dtype=torch.float64, device=self.device)
        rc = self.lib.t2h_region_color_stats(i.data_ptr(), int(img_signed), s.data_ptr(), self._bits(bits), len(bits), B, h,
                                             w, partial.data_ptr(), st.data_ptr(), self.stream())
        assert rc == 0, (rc, self.last_error() if self.last_error else None)
        return st.cpu().numpy()

    def apply_rc(self, img, segm, bits, src, dst, luma=1.0, gain_max=4.0, feather=2, img_signed=False, want_u8=False):
        """-> (return code, out f32 [B, 3, H, W], u8 or None) on the host"""
        B, _, h, w = img.shape
        i, s = img.to(self.device).contiguous(), segm.to(self.device).contiguous()
        sd = torch.as_tensor(np.asarray(src), dtype=torch.float64).to(self.device).contiguous()
        dd = torch.as_tensor(np.asarray(dst), dtype=torch.float64).to(self.device).contiguous()
        out = torch.full_like(i, float('nan'))
        u8 = torch.full((B, h, w, 3), 7, dtype=torch.uint8, device=self.device) if want_u8 else None
        rc = self.lib.t2h_recolor_region_f32(i.data_ptr(), int(img_signed), s.data_ptr(), self._bits(bits), len(bits),
                                             sd.data_ptr(), dd.data_ptr(), luma, gain_max, feather, out.data_ptr(),
                                             u8.data_ptr() if want_u8 else None, B, h, w, self.stream())
        return rc, out.cpu(), (u8.cpu() if want_u8 else None)

    def apply(self, *a, **kw):
        rc, out, u8 = self.apply_rc(*a, **kw)
        assert rc == 0, (rc, self.last_error() if self.last_error else None)
        assert not torch.isnan(out).any()           # every pixel written
        return out, u8


def _bits(t):
    return t.contiguous().view(torch.int32)


def image(B, h, w, seed, signed=False, lo=0.0, hi=1.0):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(B, 3, h, w, generator=g) * (hi - lo) + lo
    return (x * 2 - 1) * 1.2 if signed else x      # (signed: beyond [-1, 1], the clamp of p is exercised)


def segm_of(B, h, w, boxes, background=0.0):
    """boxes: per image a list of (label, y0, y1, x0, x1), later boxes on top -> f32 [B, h, w]"""
    s = torch.full((B, h, w), float(background))
    for b, bs in enumerate(boxes):
        for lab, y0, y1, x0, x1 in bs:
            s[b, y0:y1, x0:x1] = float(lab)
    return s


def shifted(st, colour=(0.8, 0.2, 0.3)):
    return R.plain_target(st, colour)


def check(run, img, segm, bits, dst=None, colour=(0.8, 0.2, 0.3), luma=1.0, gain_max=4.0, feather=2, img_signed=False,
          want_u8=False, need_touched=True, need_untouched=True, identity=False):
    """stats against the reference, then one apply against it: TOL everywhere, p's bits wherever sum N == 0"""
    st = run.stats(img, segm, bits, img_signed)
    ref_st = R.stats(img, segm, bits, img_signed)
    assert np.array_equal(st[..., 0], ref_st[..., 0]) and (st[..., 7] == 0).all()
    serr = np.abs(st - ref_st)[..., 1:7].max()
    assert serr <= R.STATS_TOL, serr
    dst = st if identity else shifted(st, colour) if dst is None else dst
    kw = dict(luma=luma, gain_max=gain_max, feather=feather, img_signed=img_signed)
    out, u8 = run.apply(img, segm, bits, st, dst, want_u8=want_u8, **kw)
    ref = R.recolor(img, segm, bits, st, dst, **kw)
    err = (out.double() - ref['out']).abs().max().item()
    print(f'recolor {tuple(img.shape)} G {len(bits)} feather {feather}: stats err {serr:.2e} (bound {R.STATS_TOL:.0e}), '
          f'max abs err {err:.3e} (bound {R.TOL:.0e})')
    assert err <= R.TOL, err
    touched = torch.from_numpy(ref['touched'])[:, None].expand_as(out)
    assert (not need_touched or touched.any()) and (not need_untouched or (~touched).any())
    assert torch.equal(_bits(out)[~touched], _bits(ref['p'])[~touched])
    if want_u8:
        excluded = R.check_u8(u8, ref)
        print(f'  uint8: {excluded:.4f} of the bytes excluded as boundary cases of the reference')
    return out, ref, st


def case_01_no_member(run):
    img = image(2, H, W, 1, signed=True)
    segm = segm_of(2, H, W, [[(7, 10, 50, 10, 50)], []])
    out, ref, st = check(run, img, segm, [UP, LO], img_signed=True, need_touched=False)
    assert (st == 0).all() and torch.equal(_bits(out), _bits(ref['p']))
    assert (ref['p'] == 0).any() and (ref['p'] == 1).any()                       # the clamp of p took part


def case_02_whole_image_one_group(run):
    img = image(2, H, W, 2)
    out, ref, _ = check(run, img, torch.full((2, H, W), 4.0), [UP], feather=3, need_untouched=False)
    assert (ref['N'] == 4 ** 4).all()                                            # alpha = 1 everywhere, borders included
    out, ref, _ = check(run, image(2, HS, WS, 3), torch.full((2, HS, WS), 2.0), [UP, OU], feather=8, need_untouched=False)
    assert (ref['N'][:, 1] == 9 ** 4).all() and (ref['N'][:, 0] == 0).all()


def case_03_feather_0_hard_edge(run):
    img = image(2, H, W, 4)
    segm = segm_of(2, H, W, [[(1, 20, 70, 25, 66)], [(4, 0, 33, 31, 80)]])
    out, ref, _ = check(run, img, segm, [UP], feather=0)
    inside = torch.from_numpy(ref['code'] == 0)
    assert np.array_equal(ref['touched'], ref['code'] == 0)                      # exactly the members ...
    assert torch.equal(_bits(out[0, :, 19, 25:66]), _bits(ref['p'][0, :, 19, 25:66]))   # ... p one pixel outside
    assert torch.equal(_bits(out[0, :, 20:70, 24]), _bits(ref['p'][0, :, 20:70, 24]))
    assert ((out.double() - ref['p'].double()).abs()[inside[:, None].expand_as(out)] > 1e-3).any()


def case_04_feather_8_borders_and_corners(run):
    img = image(3, H, W, 5)
    segm = segm_of(3, H, W, [[(1, 0, 5, 0, 5), (1, 0, 4, 76, 80), (1, 90, 96, 0, 6), (1, 93, 96, 77, 80)],     # corners
                             [(3, 0, 3, 30, 50), (3, 40, 60, 0, 2), (3, 94, 96, 20, 40), (3, 30, 40, 78, 80)],  # borders
                             [(2, 0, 96, 0, 1), (2, 0, 1, 0, 80)]])
    check(run, img, segm, [UP, LO, OU], feather=8, want_u8=True)
    check(run, image(2, HS, WS, 6), segm_of(2, HS, WS, [[(1, 0, 3, 0, 3), (5, 27, 30, 24, 27)], [(2, 12, 14, 0, 27)]]),
          [UP, LO, OU], feather=8)


def case_05_single_pixel(run):
    img = image(2, H, W, 7)
    segm = segm_of(2, H, W, [[(1, 40, 41, 33, 34)], [(1, 95, 96, 79, 80)]])
    for f in (0, 2, 8):
        out, ref, st = check(run, img, segm, [UP], feather=f)
        assert (st[:, 0, 0] == 1).all() and (st[:, 0, 4:7] <= R.STATS_TOL).all()
        assert int(ref['touched'][0].sum()) == (2 * f + 1) ** 2


def case_06_tile_seams(run):
    img = image(2, H, W, 8)
    segm = segm_of(2, H, W, [[(1, 25, 40, 28, 70)], [(4, 30, 34, 30, 34), (4, 31, 33, 62, 66)]])
    for f in (2, 8):
        out, ref, _ = check(run, img, segm, [UP], feather=f)
        err = (out.double() - ref['out']).abs()
        # no seam: the error at the columns / rows on either side of a tile edge is the error of any other column / row
        for a in (31, 32, 63, 64):
            assert err[..., a].max().item() <= R.TOL
        assert err[..., 31:33, :].max().item() <= R.TOL


def case_07_far_pixels_keep_their_bits(run):
    img = image(2, H, W, 9)
    segm = segm_of(2, H, W, [[(5, 40, 56, 20, 44)], [(21, 10, 20, 50, 60)]])
    for f in (1, 4):
        out, ref, _ = check(run, img, segm, [LO], feather=f)
        cheb = R.tent_counts(ref['code'] == 0, f) == 0                           # no member within Chebyshev distance f
        far = torch.from_numpy(cheb)[:, None].expand_as(out)
        assert np.array_equal(cheb, ~ref['touched']) and torch.equal(_bits(out)[far], _bits(ref['p'])[far])
    box = torch.zeros(H, W, dtype=torch.bool)
    box[40 - 4:56 + 4, 20 - 4:44 + 4] = True
    assert np.array_equal(ref['touched'][0], box.numpy())


def case_08_touching_groups(run):
    img = image(2, H, W, 10)
    two = segm_of(2, H, W, [[(1, 20, 60, 10, 40), (3, 20, 60, 40, 70)], [(4, 0, 48, 0, 80), (5, 48, 96, 0, 80)]])
    check(run, img, two, [UP, LO], feather=4, want_u8=True, need_untouched=False)
    three = segm_of(2, H, W, [[(1, 16, 48, 16, 40), (3, 48, 80, 16, 40), (2, 16, 80, 40, 64)],
                              [(2, 30, 34, 0, 80), (1, 0, 30, 0, 80), (21, 34, 96, 0, 80)]])
    check(run, img, three, [UP, LO, OU], feather=3, need_untouched=False)
    four = segm_of(2, H, W, [[(1, 16, 48, 16, 48), (3, 16, 48, 48, 80), (2, 48, 80, 16, 48), (9, 48, 80, 48, 80)],
                             [(9, 31, 33, 31, 33), (1, 0, 31, 0, 80), (2, 33, 96, 0, 31), (3, 33, 96, 33, 80)]])
    out, ref, _ = check(run, img, four, [UP, LO, OU, R.bits_of([9])], feather=2, need_untouched=False)
    assert ((ref['N'] > 0).sum(1) == 4).any()                                    # a pixel that four groups reach


def case_09_overlapping_groups(run):
    img, segm = image(1, HS, WS, 11), torch.ones(1, HS, WS)
    st = R.stats(img, segm, [UP])
    st2 = np.concatenate([st, st], 1)
    rc, _, _ = run.apply_rc(img, segm, [UP, R.bits_of([4, 9])], st2, st2)
    assert rc == -1
    rc, _, _ = run.apply_rc(img, segm, [UP, R.bits_of([9])], st2, st2)
    assert rc == 0


def case_10_group_absent_in_one_image(run):
    img = image(3, H, W, 12)
    segm = segm_of(3, H, W, [[(1, 20, 60, 20, 60)], [(3, 20, 60, 20, 60)], [(1, 0, 40, 0, 40), (3, 40, 96, 40, 80)]])
    out, ref, st = check(run, img, segm, [UP, LO], feather=2)
    assert (st[0, 1] == 0).all() and (st[1, 0] == 0).all() and (st[2, :, 0] > 0).all()
    # a target that lacks the group: the source region stays as it is
    dst = shifted(st)
    dst[0, 0] = 0.0
    out, ref, _ = check(run, img, segm, [UP, LO], dst=dst, feather=2)
    assert torch.equal(_bits(out[0]), _bits(ref['p'][0])) and not ref['touched'][0].any()


def case_11_gains_and_luma(run):
    img = image(2, H, W, 13, lo=0.3, hi=0.7)
    img[1, :, 20:60, 20:60] = torch.tensor([0.4, 0.5, 0.6])[:, None, None]      # image 1: a flat region
    segm = segm_of(2, H, W, [[(1, 20, 60, 20, 60)], [(1, 20, 60, 20, 60)]])
    st = R.stats(img, segm, [UP])
    assert (st[1, 0, 4:7] < 1e-7).all() and (st[0, 0, 4:7] > 0.01).all()
    for scale, gm in ((100.0, 4.0), (0.001, 4.0), (100.0, 16.0), (3.0, 1.0)):
        dst = st.copy()
        dst[:, :, 4:7] = st[:, :, 4:7] * scale + (1e-3 if scale > 1 else 0.0)    # (flat region: a positive target, gain 1)
        k = R.constants(st, dst, 1.0, gm)
        assert np.allclose(k['gain'][0, 0], gm if scale > 1 else 1.0 / gm) and (k['gain'][1, 0] == 1.0).all()
        check(run, img, segm, [UP], dst=dst, gain_max=gm, feather=1)
    # luma = 0: the region's mean Y stays, its chroma moves
    out, ref, st = check(run, img, segm, [UP], colour=(0.55, 0.35, 0.45), luma=0.0, feather=0)
    after = run.stats(out, segm, [UP])
    assert np.abs(after[:, 0, 1] - st[:, 0, 1]).max() <= 1e-5
    assert np.abs(after[:, 0, 2:4] - R.colour_yuv((0.55, 0.35, 0.45))[1:]).max() <= 1e-5


def case_12_out_of_range_target(run):
    img = image(2, H, W, 14)
    segm = segm_of(2, H, W, [[(1, 10, 80, 10, 70)], [(4, 30, 50, 30, 50)]])
    for colour in ((1.0, 1.0, 1.0), (0.0, 0.0, 0.0), (1.0, 0.0, 0.0)):
        out, ref, _ = check(run, img, segm, [UP], colour=colour, feather=2, want_u8=False)
        m = torch.from_numpy(ref['touched'])[:, None].expand_as(out)
        assert ((out == 0) & m).any() or ((out == 1) & m).any()                  # the clamp took part


def case_13_invalid_labels(run):
    img = image(2, H, W, 15)
    segm = segm_of(2, H, W, [[(1, 10, 30, 10, 30)], [(4, 50, 70, 40, 60)]])
    bad = [-1.0, -0.0, 0.5, 1.5, 63.5, 64.0, 65.0, 1e9, -1e9, float('nan'), float('inf'), float('-inf'), 1.0000001, 3.9999998]
    for i, v in enumerate(bad):
        segm[:, 40 + i, 0:40] = v
    bits = [UP | 1 | (1 << 63)]                                                   # labels 0, 1, 4, 63
    segm[0, 80, 0:8] = 63.0
    out, ref, st = check(run, img, segm, bits, feather=1)
    # -0.0 is label 0 (it equals 0.0), every other odd value is in no group
    assert int(st[0, 0, 0]) == 20 * 20 + 8 + (segm[0] == 0).sum().item()


def case_14_identity(run):
    img = image(2, H, W, 16)
    segm = segm_of(2, H, W, [[(1, 20, 60, 20, 60), (3, 60, 90, 20, 60)], [(2, 5, 50, 35, 75)]])
    out, ref, _ = check(run, img, segm, [UP, LO, OU], identity=True, feather=3)
    assert (out - img).abs().max().item() <= R.TOL
    assert torch.equal(_bits(out)[~torch.from_numpy(ref['touched'])[:, None].expand_as(out)],
                       _bits(img)[~torch.from_numpy(ref['touched'])[:, None].expand_as(out)])


def case_15_round_trip(run):
    img = image(2, H, W, 17, lo=0.3, hi=0.7)
    segm = segm_of(2, H, W, [[(1, 20, 60, 20, 60)], [(4, 3, 90, 35, 75)]])
    colour = (0.55, 0.45, 0.52)
    out, ref, st = check(run, img, segm, [UP], colour=colour, feather=0)
    assert out.min().item() > 0 and out.max().item() < 1                         # (nothing was clamped)
    after = run.stats(out, segm, [UP])
    assert np.abs(after[:, 0, 1:4] - R.colour_yuv(colour)).max() <= 1e-5
    assert np.array_equal(after[:, 0, 0], st[:, 0, 0])


def case_16_batch_independence_and_repeats(run):
    img = image(3, H, W, 18, signed=True)
    segm = segm_of(3, H, W, [[(1, 20, 60, 20, 60)], [(3, 0, 40, 30, 80), (2, 40, 96, 0, 33)], [(4, 60, 96, 60, 80), (5, 0, 9, 0, 9)]])
    bits = [UP, LO, OU]
    st = run.stats(img, segm, bits, True)
    dst = shifted(st, (0.2, 0.6, 0.9))
    kw = dict(feather=3, img_signed=True, want_u8=True)
    out, u8 = run.apply(img, segm, bits, st, dst, **kw)
    assert np.array_equal(st.view(np.int64), run.stats(img, segm, bits, True).view(np.int64))      # two calls, equal bits
    again, again8 = run.apply(img, segm, bits, st, dst, **kw)
    assert torch.equal(_bits(out), _bits(again)) and torch.equal(u8, again8)
    for b in range(3):
        one = run.stats(img[b:b + 1], segm[b:b + 1], bits, True)
        assert np.array_equal(one.view(np.int64), st[b:b + 1].view(np.int64)), b
        o1, o8 = run.apply(img[b:b + 1], segm[b:b + 1], bits, st[b:b + 1], dst[b:b + 1], **kw)
        assert torch.equal(_bits(out[b:b + 1]), _bits(o1)) and torch.equal(u8[b:b + 1], o8), b
    # 30 x 27: the one-by-one loads give the bits of any other batch position too
    img, segm = image(3, HS, WS, 19), segm_of(3, HS, WS, [[(1, 3, 20, 3, 20)], [(3, 0, 30, 13, 27)], [(2, 10, 11, 0, 27)]])
    st = run.stats(img, segm, bits)
    assert np.array_equal(run.stats(img[2:3], segm[2:3], bits).view(np.int64), st[2:3].view(np.int64))


def case_17_uint8_and_ragged_width(run):
    img = image(2, H, W, 20)
    segm = segm_of(2, H, W, [[(1, 10, 50, 10, 50), (3, 50, 90, 10, 50)], [(2, 30, 70, 40, 80)]])
    check(run, img, segm, [UP, LO, OU], feather=2, want_u8=True)
    img, segm = image(3, HS, WS, 21, signed=True), segm_of(3, HS, WS, [[(1, 3, 20, 3, 20)], [(3, 0, 30, 13, 27)], []])
    check(run, img, segm, [UP, LO], feather=2, img_signed=True, want_u8=True)
    check(run, img, segm, [UP, LO], feather=0, img_signed=True, want_u8=True)


ALL_CASES = [case_01_no_member, case_02_whole_image_one_group, case_03_feather_0_hard_edge,
             case_04_feather_8_borders_and_corners, case_05_single_pixel, case_06_tile_seams,
             case_07_far_pixels_keep_their_bits, case_08_touching_groups, case_09_overlapping_groups,
             case_10_group_absent_in_one_image, case_11_gains_and_luma, case_12_out_of_range_target,
             case_13_invalid_labels, case_14_identity, case_15_round_trip, case_16_batch_independence_and_repeats,
             case_17_uint8_and_ragged_width]
