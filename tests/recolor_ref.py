"""Float64 restatement of t2h_region_color_stats / t2h_recolor_region_f32 (include/t2h_hip.h), shared by
tests/test_recolor_emulated.py, tests/test_gpu_recolor.py and tools/recolor_bench.py: the membership rule of
t2h_region_keep's mode 2, the integer tent sums N_g over a replicate-padded map, the statistics, and the transform with
its per-group constants rounded once to fp32, as the header states them.  numpy / torch on the host, no kernel code."""
import numpy as np
import torch

GROUPS = dict(upper=(1, 4), lower=(3, 5, 21), outer=(2, ))   # the classes of t2h_texture_map
TOL = 1e-5          # |f32 kernel - float64 reference| on out: outputs are clamped to [0, 1], intermediates reach at most
#                     gain_max + 1, about a dozen fp32 roundings at that magnitude = 3e-6 (derived, not measured)
STATS_TOL = 1e-6    # means and deviations: three fp32 roundings of values <= 1 per pixel, no growth in the f64 sums
U8_MARGIN = 0.003   # > 255 * TOL: where the reference's out * 255 + 0.5 is farther than this from an integer, the byte is fixed


def photo01(img, img_signed):
    """the kernels' p in fp32 (torch): ((x + 1) / 2).clamp(0, 1), or x"""
    return ((img + 1) / 2).clamp(0, 1) if img_signed else img


def bits_of(labels):
    bits = 0
    for lb in labels:
        assert 0 <= int(lb) < 64
        bits |= 1 << int(lb)
    return bits


def membership(segm, bits):
    """segm f32 [B, H, W] (or [B, 1, H, W]), bits: G ints -> int64 numpy [B, H, W]: the group of every pixel, -1 = none.
    A value is a label iff 0 <= v < 64 and v is whole (t2h_region_keep, mode 2); NaN / inf / fractions are not."""
    v = np.asarray(segm.detach().cpu().reshape(segm.shape[0], segm.shape[-2], segm.shape[-1]), dtype=np.float32)
    with np.errstate(invalid='ignore'):
        valid = (v >= 0) & (v < 64) & (np.floor(v) == v)
    lab = np.where(valid, v, 0).astype(np.int64)
    code = np.full(v.shape, -1, dtype=np.int64)
    for g, b in enumerate(bits):
        hit = valid & ((np.uint64(b) >> lab.astype(np.uint64)) & np.uint64(1)).astype(bool)
        assert (code[hit] == -1).all(), 'overlapping groups'
        code[hit] = g
    return code


def yuv(p):
    """p float64 [..., 3, H, W] (torch) -> Y, U, V float64"""
    r, g, b = p[..., 0, :, :], p[..., 1, :, :], p[..., 2, :, :]
    y = 0.299 * r + 0.587 * g + 0.114 * b
    return y, b - y, r - y


def rgb(y, u, v):
    return torch.stack([y + v, y - (0.299 * v + 0.114 * u) / 0.587, y + u], dim=-3)


def colour_yuv(colour):
    """(r, g, b) or [B, 3] -> float64 numpy [..., 3] = (Y, U, V) of a plain colour"""
    c = np.asarray(colour, dtype=np.float64)
    y = 0.299 * c[..., 0] + 0.587 * c[..., 1] + 0.114 * c[..., 2]
    return np.stack([y, c[..., 2] - y, c[..., 0] - y], -1)


def stats(img, segm, bits, img_signed=False):
    """-> float64 numpy [B, G, 8] = {n, mY, mU, mV, sY, sU, sV, 0}; n == 0: zeros"""
    p = photo01(img.detach().cpu().float(), img_signed).double()
    code = membership(segm, bits)
    y, u, v = (t.numpy() for t in yuv(p))
    out = np.zeros((p.shape[0], len(bits), 8))
    for b in range(p.shape[0]):
        for g in range(len(bits)):
            m = code[b] == g
            n = int(m.sum())
            if n == 0:
                continue
            out[b, g, 0] = n
            for c, x in enumerate((y, u, v)):
                xs = x[b][m]
                mean = xs.sum() / n
                out[b, g, 1 + c] = mean
                out[b, g, 4 + c] = np.sqrt(max(0.0, (xs * xs).sum() / n - mean * mean))
    return out


def plain_target(src_stats, colour):
    """the target of a plain colour: the source's own statistics with mY, mU, mV replaced -> gains 1"""
    t = np.array(src_stats, dtype=np.float64, copy=True)
    t[..., 1:4] = np.broadcast_to(colour_yuv(colour)[..., None, :] if np.ndim(colour) == 2 else colour_yuv(colour),
                                  t[..., 1:4].shape)
    t[src_stats[..., 0] == 0] = 0.0
    return t


def tent_counts(member, f):
    """member bool / int numpy [B, H, W] -> int64 N [B, H, W]: the (f + 1 - |i|)(f + 1 - |j|) tent sum, replicate borders"""
    m = np.pad(member.astype(np.int64), ((0, 0), (f, f), (f, f)), mode='edge')
    B, H, W = member.shape
    w = [f + 1 - abs(j - f) for j in range(2 * f + 1)]
    h = sum(w[j] * m[:, :, j:j + W] for j in range(2 * f + 1))
    return sum(w[i] * h[:, i:i + H, :] for i in range(2 * f + 1))


def _f32(x):
    return np.asarray(x, dtype=np.float64).astype(np.float32).astype(np.float64)


def constants(src, dst, luma, gain_max):
    """src / dst float64 [B, G, 8] -> dict of float64 arrays [B, G(, 3)] holding fp32-representable values"""
    gm, lu = float(np.float32(gain_max)), float(np.float32(luma))
    ss, ts = src[..., 4:7], dst[..., 4:7]
    ok = (ss > 1e-6) & (ts > 0)
    with np.errstate(divide='ignore', invalid='ignore'):
        gain = np.where(ok, np.clip(ts / np.where(ok, ss, 1.0), 1.0 / gm, gm), 1.0)
    return dict(gain=_f32(gain), sm=_f32(src[..., 1:4]), dY=_f32(lu * (dst[..., 1] - src[..., 1])), tmU=_f32(dst[..., 2]),
                tmV=_f32(dst[..., 3]), active=(src[..., 0] > 0) & (dst[..., 0] > 0))


def recolor(img, segm, bits, src, dst, luma=1.0, gain_max=4.0, feather=2, img_signed=False):
    """-> dict(out float64 [B, 3, H, W], p fp32, N int64 numpy [B, G, H, W] (0 for inactive groups), touched bool
    [B, H, W] (sum of N > 0), u8f float64 [B, H, W, 3] = out * 255 + 0.5 before truncation, u8 uint8)"""
    src, dst = np.asarray(src, dtype=np.float64), np.asarray(dst, dtype=np.float64)
    p32 = photo01(img.detach().cpu().float(), img_signed)
    p = p32.double()
    B, _, H, W = p.shape
    G, f = len(bits), int(feather)
    code = membership(segm, bits)
    k = constants(src, dst, luma, gain_max)
    N = np.zeros((B, G, H, W), dtype=np.int64)
    for g in range(G):
        N[:, g] = tent_counts((code == g) & k['active'][:, g, None, None], f)
    y, u, v = yuv(p)
    acc = torch.zeros_like(p)
    D = float((f + 1) ** 4)
    for g in range(G):
        c = {n: torch.from_numpy(np.ascontiguousarray(a[:, g]))[..., None, None] for n, a in k.items() if n != 'active'}
        y2 = c['sm'][:, 0] + c['gain'][:, 0] * (y - c['sm'][:, 0]) + c['dY']
        u2 = c['tmU'] + c['gain'][:, 1] * (u - c['sm'][:, 1])
        v2 = c['tmV'] + c['gain'][:, 2] * (v - c['sm'][:, 2])
        alpha = torch.from_numpy(N[:, g] / D)[:, None]
        acc = acc + alpha * (rgb(y2, u2, v2) - p)
    touched = N.sum(1) > 0
    out = torch.where(torch.from_numpy(touched)[:, None], (p + acc).clamp(0, 1), p)
    u8f = (out * 255 + 0.5).permute(0, 2, 3, 1).contiguous()
    return dict(out=out, p=p32, N=N, touched=touched, code=code, u8f=u8f, u8=u8f.clamp(0, 255).floor().to(torch.uint8))


def u8_excluded(ref):
    """share of the reference's bytes within U8_MARGIN of a rounding boundary (a property of the reference alone)"""
    frac = ref['u8f'] - ref['u8f'].floor()
    return 1.0 - ((frac > U8_MARGIN) & (frac < 1 - U8_MARGIN)).double().mean().item()


def check_u8(got, ref, cap=0.05):
    """bytes equal where the reference is not within U8_MARGIN of a rounding boundary, within +-1 elsewhere; the
    excluded share stays under `cap` -> that share"""
    frac = ref['u8f'] - ref['u8f'].floor()
    sure = (frac > U8_MARGIN) & (frac < 1 - U8_MARGIN)
    excluded = 1.0 - sure.double().mean().item()
    assert excluded <= cap, f'{excluded:.4f} of the bytes sit on a rounding boundary of the reference'
    got = got.cpu()
    assert torch.equal(got[sure], ref['u8'][sure])
    assert ((got.int() - ref['u8'].int()).abs() <= 1).all()
    return excluded
