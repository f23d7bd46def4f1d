"""The split-row formats at the edges of their value range, once for the CPU emulation and once for the GPU (a plain
helper module; tests/test_split_edges_emulated.py and tests/test_gpu_split_edges.py hand in a backend `be`):

    be.split_rows(x) -> (rows int16 on the CPU, overflow word)          be.split_rows_x8(x, s) -> likewise
    be.layernorm_split(x, g, b) / be.layernorm_x8(x, g, b, s) -> likewise
    be.gemm(A, B, M, N, K, x8=None | (sa, sb), cfg=-1, out_split=None | 'fp16' | scale) -> (out fp32, rows | None, word)

with A, B split rows / x8 rows as CPU int16 tensors.  The inputs are built here, deterministically: the same ones on both sides."""
import torch

import split_ref as S
from text2human_amd import ops


def rnd(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


# ---- the inputs: value-range edges of the split-row producers

LADDER_C = 256


def _rows_of(values, C=LADDER_C):
    """a flat list of fp64 values, both signs -> fp32 [rows, C], zero padded (every value must be an fp32 number)"""
    v = torch.cat([values, -values])
    assert torch.equal(v.float().double(), v), 'a ladder value is not an fp32 number'
    pad = (-v.numel()) % C
    return torch.cat([v, torch.zeros(pad, dtype=torch.float64)]).float().view(-1, C)


def _fp16_ties():
    """every tie of the fp16 rounding (2k + 1) 2^(e - 11), k over the binade [2^10, 2^11), for e in -24, -15, -14, 0, 15
    (below 2^-14 fp16 is subnormal, its step 2^-24: the formula's points there are quarter points of that step, and the
    ties of the subnormal codes themselves, (2k + 1) 2^-25 for k < 2^10, are added), up to fp16's largest number"""
    k = torch.arange(1024, 2048, dtype=torch.float64)
    ties = [(2 * k + 1) * 2.0 ** (e - 11) for e in (-24, -15, -14, 0, 15)]
    ties.append((2 * torch.arange(0, 1024, dtype=torch.float64) + 1) * 2.0 ** -25)
    t = torch.cat(ties)
    t = t[t < 65504.0]
    for e in (-24, -15, -14, 0, 15):                    # every binade is there (the top one less the tie with infinity)
        assert int(((t >= 2.0 ** e) & (t < 2.0 ** (e + 1))).sum()) >= 1023, e
    return t


def _with_residual(l):
    """x = h + l / 2048 (fp64) for the residuals l: h = 2^eh (1 + 2^-10) with |l| < 2^eh, so that fp16(x) = h -- and for
    |l| < 2^-14 also h = 0 (x = l / 2048 is below half of fp16's smallest number) -- kept only where x is an fp32
    number: the residual the producer computes, (x - h) 2048, is then l exactly"""
    out = []
    eh = torch.clamp(torch.floor(torch.log2(l.abs())) + 1, min=-14.0)
    for h in (2.0 ** eh * (1.0 + 2.0 ** -10), torch.where(l.abs() < 2.0 ** -14, 0.0, float('nan')).double()):
        for sign in (1.0, -1.0):
            x = h + sign * l / 2048.0
            ok = (x.float().double() == x) & (x.float().half().double() == h) & (x.abs() < 65504.0)
            out.append(x[ok])
    return torch.cat(out)


def split_ladder():
    """fp32 [rows, 256] for t2h_split_rows_f32: every fp16 tie of the hi plane; the same ties as the residual of the lo
    plane (binade 14 in place of 15: |l| <= 2^15 follows from |x| < 65504, so binade 15 holds no residual); +0, -0;
    the largest admissible magnitude"""
    k = torch.arange(1024, 2048, dtype=torch.float64)
    lo = torch.cat([(2 * k + 1) * 2.0 ** (e - 11) for e in (-24, -15, -14, 0, 14)] +
                   [(2 * torch.arange(0, 1024, dtype=torch.float64) + 1) * 2.0 ** -25])
    res = _with_residual(lo)
    for e in (-24, -15, -14, 0, 14):                    # every binade of l survives the filter, in both signs
        for sign in (1.0, -1.0):
            got_l = (res - res.float().half().double()) * 2048.0 * sign
            assert int(((got_l >= 2.0 ** e) & (got_l < 2.0 ** (e + 1))).sum()) >= 1024, (e, sign)
    top = torch.nextafter(torch.tensor(65504.0), torch.tensor(0.0)).double().view(1)
    x = _rows_of(torch.cat([_fp16_ties(), res, top, torch.zeros(1, dtype=torch.float64)]))
    x[-1, -1] = -0.0
    return x


def _e4m3_midpoints(top):
    """the midpoints between adjacent e4m3 codes: the subnormal codes (step 2^-9), the normal binades 2^-6 and 2^-5, and
    the binade [top, 2 top) up to 448"""
    m = torch.arange(0, 8, dtype=torch.float64) + 0.5
    mids = torch.cat([m * 2.0 ** -9, (8 + m) * 2.0 ** -9, (8 + m) * 2.0 ** -8, (8 + m) * top / 8.0])
    return mids[mids < 448.0]


X8_LADDER_SCALE = 16.0


def x8_ladder(s=X8_LADDER_SCALE):
    """fp32 [rows, 256] for t2h_split_rows_x8_f32 at scale s: the fp16 ties of split_ladder inside the 8-bit planes'
    range; every e4m3 midpoint as h s (x = mid / s, an fp16 number: l = 0) and as l s (x = h + mid / (2048 s)); +0, -0;
    the largest |x| with |x| s < 448.  An admissible x has |l| <= 2^floor(log2 |h|) and |h| s <= 448, so l s <= 256:
    the residual plane's top binade is [128, 256), not [256, 448]"""
    base = split_ladder().double().flatten()
    base = base[(base > 0) & (base * s < 448.0)]
    hmid = _e4m3_midpoints(256.0) / s
    assert torch.equal(hmid.half().double(), hmid)
    lmid = _with_residual(_e4m3_midpoints(128.0) / s)
    for lo_, hi_ in ((0.0, 2.0 ** -6), (2.0 ** -6, 2.0 ** -5), (2.0 ** -5, 2.0 ** -4), (128.0, 256.0)):
        for sign in (1.0, -1.0):                        # 8 midpoints of every e4m3 binade as l s, in both signs
            ls = (lmid - lmid.float().half().double()) * 2048.0 * s * sign
            assert len(set(ls[(ls > lo_) & (ls < hi_)].tolist())) == 8, (lo_, hi_, sign)
    hs = _e4m3_midpoints(256.0)
    for lo_, hi_ in ((0.0, 2.0 ** -6), (2.0 ** -6, 2.0 ** -5), (2.0 ** -5, 2.0 ** -4), (256.0, 448.0)):
        assert int(((hs > lo_) & (hs < hi_)).sum()) == (6 if lo_ == 256.0 else 8), (lo_, hi_)
    lmid = lmid[lmid.abs() * s < 448.0]
    top = torch.nextafter(torch.tensor(448.0 / s), torch.tensor(0.0)).double().view(1)
    x = _rows_of(torch.cat([base, hmid, lmid.abs(), top, torch.zeros(1, dtype=torch.float64)]))
    x[-1, -1] = -0.0
    return x


def threshold_values(s=X8_LADDER_SCALE):
    """(largest admissible for the fp16 planes, largest admissible for the 8-bit planes at scale s, the value that raises
    bit 0, the value that raises bit 1 only)"""
    below = lambda v: float(torch.nextafter(torch.tensor(v), torch.tensor(0.0)))  # noqa: E731
    return below(65504.0), below(448.0 / s), 65504.0, 448.0 / s


def with_row_block(x, row, col0, value):
    """a copy of the ordinary tensor x with `value` (alternating signs) in the 32 columns from col0 of one row"""
    y = x.clone()
    y[row, col0:col0 + 32] = value * (1.0 - 2.0 * (torch.arange(32) % 2))
    return y


# ---- 1. rounding ladders


def ladder_fp16_planes(be):
    """every tie of both fp16 conversions, both signs, +-0, the largest admissible magnitude: the host packer's bytes
    (round-to-nearest-even; random data meets a tie with probability zero)"""
    x = split_ladder()
    got, bits = be.split_rows(x)
    assert bits == 0
    want = ops.pack_split_rows_host(x)
    assert torch.equal(got, want), int((got != want).sum())


def ladder_x8_planes(be):
    """the same through the x8 producer at s = 16, with every midpoint between adjacent e4m3 codes as h s and as l s"""
    s = X8_LADDER_SCALE
    x = x8_ladder(s)
    got, bits = be.split_rows_x8(x, s)
    assert bits == 0
    hi, h8, l8 = ops.unpack_x8_rows_host(got, x.shape[0], x.shape[1], s)
    whi, wh8, wl8 = S.x8_planes_host(x, s)
    assert torch.equal(hi, whi), int((hi != whi).sum())
    assert torch.equal(h8, wh8), int((h8 != wh8).sum())
    assert torch.equal(l8, wl8), int((l8 != wl8).sum())
    # (the sign of zero in the fp16 plane: bytes)
    assert torch.equal(got.view(torch.uint8).view(x.shape[0], -1, 128)[:, :, :64],
                       S.x8_rows_host(x, s).view(torch.uint8).view(x.shape[0], -1, 128)[:, :, :64])


# ---- 2. exact thresholds of the overflow word


def _finite_fp16_planes(rows):
    return bool(torch.isfinite(rows.view(torch.float16).float()).all())


def _finite_x8_planes(rows, r, C, s):
    return all(bool(torch.isfinite(t).all()) for t in ops.unpack_x8_rows_host(rows, r, C, s))


def thresholds_producers(be):
    """split_rows / split_rows_x8: one row of 32 columns of an ordinary tensor at the largest admissible value (word 0,
    finite planes), at 65504 (bit 0), at |x| s = 448 (bit 1 and not bit 0)"""
    s = X8_LADDER_SCALE
    top16, top8, v16, v8 = threshold_values(s)
    x = rnd(9, 256, seed=31) * 1.5
    rows, bits = be.split_rows(with_row_block(x, 4, 96, top16))
    assert bits == 0 and _finite_fp16_planes(rows)
    assert be.split_rows(with_row_block(x, 4, 96, v16))[1] == 1
    rows, bits = be.split_rows_x8(with_row_block(x, 4, 96, top8), s)
    assert bits == 0 and _finite_x8_planes(rows, 9, 256, s)
    assert be.split_rows_x8(with_row_block(x, 4, 96, v8), s)[1] == 2
    assert be.split_rows_x8(with_row_block(x, 4, 96, v16), s)[1] == 1
    # a scale under which the fp16 range ends first: its largest admissible value
    rows, bits = be.split_rows_x8(with_row_block(x, 4, 96, top16), 2.0 ** -8)
    assert bits == 0 and _finite_x8_planes(rows, 9, 256, 2.0 ** -8)


def thresholds_layernorm(be):
    """layernorm_split / layernorm_x8: gamma = 0 on a block of 32 columns makes every row's output there beta exactly
    (LayerNorm has no input that puts an exact value into ONE row), the other columns are ordinary"""
    s = X8_LADDER_SCALE
    top16, top8, v16, v8 = threshold_values(s)
    rows, C = 7, 512
    x = rnd(rows, C, seed=32) * 2.0 + 0.5
    g, b = rnd(C, seed=33) * 0.2 + 1.0, rnd(C, seed=34) * 0.1
    g[160:192] = 0.0

    def beta(v):
        return with_row_block(b.view(1, C), 0, 160, v).view(C)

    out, bits = be.layernorm_split(x, g, beta(top16))
    assert bits == 0 and _finite_fp16_planes(out)
    assert ops.unsplit_rows_host(out, rows, C)[:, 160:192].abs().min().item() == top16
    assert be.layernorm_split(x, g, beta(v16))[1] == 1
    out, bits = be.layernorm_x8(x, g, beta(top8), s)
    assert bits == 0 and _finite_x8_planes(out, rows, C, s)
    assert be.layernorm_x8(x, g, beta(v8), s)[1] == 2
    assert be.layernorm_x8(x, g, beta(v16), s)[1] == 1


def thresholds_gemm_epilogue(be, M=128):
    """the GEMM's out_split epilogue (fp16 planes and out_x8_scale): row r of A is the unit vector e_0, column 0 of the
    other rows is 0, and 32 rows of W are v e_0 -- the product holds v (to the last bit: 1 x hi + 1 x lo / 2048) in one
    row of 32 columns and ordinary values elsewhere.  M = 128 on the emulator: at a ragged M the tiled kernel's x8
    store swaps halves between lane pairs by DPP after the lanes of masked rows have left, which the hardware allows
    and the emulator's wave-collective lane exchange waits for (tests/test_row_counts_emulated.py, GemmCase); the GPU
    twin also runs M = 70"""
    s = X8_LADDER_SCALE
    top16, top8, v16, v8 = threshold_values(s)
    N, K, r = 96, 64, 37
    a, w = rnd(M, K, seed=35) * 1.3, rnd(N, K, seed=36) * 0.25
    a[:, 0] = 0.0
    a[r] = 0.0
    a[r, 0] = 1.0

    def run(v, out_split):
        wv = w.clone()
        wv[32:64] = 0.0
        wv[32:64, 0] = v * (1.0 - 2.0 * (torch.arange(32) % 2))
        out, rows, bits = be.gemm(ops.pack_split_rows_host(a), ops.pack_split_rows_host(wv), M, N, K, cfg=2, out_split=out_split)
        assert out[r, 32:64].abs().min().item() == v == out[r, 32:64].abs().max().item()
        return rows, bits

    rows, bits = run(top16, 'fp16')
    assert bits == 0 and _finite_fp16_planes(rows)
    rows, bits = run(top8, s)
    assert bits == 0 and _finite_x8_planes(rows, M, N, s)
    assert run(v8, s)[1] == 2
    # 65504 itself (a weight must stay below it to be packed): a = 2 e_0 against w = 32752 e_0, both fp16 numbers
    a2 = a.clone()
    a2[r, 0] = 2.0
    wv = w.clone()
    wv[32:64] = 0.0
    wv[32:64, 0] = 32752.0
    A, B = ops.pack_split_rows_host(a2), ops.pack_split_rows_host(wv)
    out, rows, bits = be.gemm(A, B, M, N, K, cfg=2, out_split='fp16')
    assert out[r, 32:64].min().item() == 65504.0 and bits == 1
    assert be.gemm(A, B, M, N, K, cfg=2, out_split=2.0 ** -8)[2] == 1


# ---- 3. the GEMM on subnormal hi planes

SUBNORMAL_SHAPES = [(2, 70, 96, 128), (6, 128, 64, 128), (8, 256, 128, 128), (10, 128, 192, 128), (-1, 17, 96, 128)]


def emulate_fp16_planes(a, w):
    """the fp16-plane kernel's arithmetic in fp64: ah.bh + (ah.bl + al.bh) / 2048"""
    ah, al = [t.double() for t in ops.split_planes_host(a)]
    bh, bl = [t.double() for t in ops.split_planes_host(w)]
    return ah @ bh.t() + (ah @ bl.t() + al @ bh.t()) / ops.SPLIT_LO_SCALE


def gemm_on_subnormal_planes(be, cfg, M, N, K, x8, both):
    """w = randn 2e-5 (and a too, with `both`): most of the fp16 hi plane of such a tensor is subnormal (below 6.1e-5),
    the rest of the value sits in the residual plane.  Against the fp64 emulation of the kernel's own arithmetic,
    |got - emu| <= 2e-6 sum |a||w| with NO absolute term (tests/test_gpu_x8.py's + 1e-6 is larger than these results);
    a matrix pipe that flushed fp16 subnormals would move the result by about half of sum |a||w|"""
    a = rnd(M, K, seed=41) * (2e-5 if both else 1.3)
    w = rnd(N, K, seed=42) * 2e-5
    assert float((w.half().float().abs() < 2.0 ** -14).float().mean()) > 0.9
    if x8:
        sa, sw = ops.x8_scale_for(a.abs().max()), ops.x8_scale_for(w.abs().max(), 256.0)
        out, _, _ = be.gemm(S.x8_rows_host(a, sa), S.x8_rows_host(w, sw), M, N, K, x8=(sa, sw), cfg=cfg)
        emu = S.emulate_x8(a, w, sa, sw)
    else:
        out, _, _ = be.gemm(ops.pack_split_rows_host(a), ops.pack_split_rows_host(w), M, N, K, cfg=cfg)
        emu = emulate_fp16_planes(a, w)
    scale = a.double().abs() @ w.double().abs().t()
    rel = ((out.double() - emu).abs() / scale).max().item()
    print(f'cfg {cfg} x8 {x8} both {both}: max |got - emu| / sum|a||w| = {rel:.3e}')
    assert torch.isfinite(out).all()
    assert ((out.double() - emu).abs() <= 2e-6 * scale).all(), rel
    # and the planes do carry the product (the emulation is not vacuous)
    true = a.double() @ w.double().t()
    assert ((emu - true).abs() <= (2e-3 if x8 else 2e-5) * scale).all()


# ---- C. a near-zero weight matrix through the x8 chain


def near_zero_weight_chain(be):
    """max |w| = 1e-6: x8_scale_for -> split_rows_x8 -> gemm_split.  Without the cap the scale is 2^27 and the residual
    plane, up to 2^-14, leaves the 8-bit range by a factor 36 with the overflow word at 0"""
    M, N, K = 70, 96, 128
    a, w = rnd(M, K, seed=51) * 1.3, rnd(N, K, seed=52)
    w = w * (1e-6 / float(w.abs().max()))
    sa, sw = ops.x8_scale_for(a.abs().max()), ops.x8_scale_for(w.abs().max(), 256.0)
    assert sw == ops.X8_SCALE_MAX
    A, ba = be.split_rows_x8(a, sa)
    B, bw = be.split_rows_x8(w, sw)
    assert ba == 0 and bw == 0
    assert all(bool(torch.isfinite(t).all()) for t in ops.unpack_x8_rows_host(B, N, K, sw))
    out, _, _ = be.gemm(A, B, M, N, K, x8=(sa, sw), cfg=2)
    emu, true = S.emulate_x8(a, w, sa, sw), a.double() @ w.double().t()
    scale = a.double().abs() @ w.double().abs().t()
    got = out.double()
    assert torch.isfinite(out).all()
    # (the x8 format bar of test_gemm_x8_every_tile_configuration, as it stands there.  At this magnitude its + 1e-6
    # dominates: sum |a||w| is about 4e-5, so 2e-6 scale ~ 1e-10 and 1.5e-4 scale / sqrt K ~ 5e-10 against outputs of
    # order 4e-6 -- an error of a fifth of the result would pass these two lines.  What holds the chain to account is
    # the finite planes above, the producer's bytes below, and gemm_on_subnormal_planes' bar without an absolute term)
    assert ((got - emu).abs() <= 2e-6 * scale + 1e-6).all(), ((got - emu).abs() / scale).max().item()
    assert ((got - true).abs() <= 1.5e-4 * scale / K**0.5 + 1e-6).all(), ((got - true).abs() * K**0.5 / scale).max().item()
    # the producer's bytes are the host packer's: nothing saturated, nothing became NaN
    assert torch.equal(B.view(torch.uint8), S.x8_rows_host(w, sw).view(torch.uint8))
