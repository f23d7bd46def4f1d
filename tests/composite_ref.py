"""Float64 restatement of t2h_composite_region_f32 (include/t2h_hip.h), shared by
tests/test_composite_emulated.py and tests/test_gpu_composite.py: brute-force Chebyshev distance to the edited cells,
the separable blur as two convolutions over a replicate-padded image, and the three-way output rule.  The tap table is
the product's own fp32 table (ops.composite_taps_host): the kernel and this reference read the same numbers."""
import numpy as np
import torch
import torch.nn.functional as F

from text2human_amd.ops import composite_taps_host  # noqa: F401  (re-exported for the tests)

TOL = 2e-5        # |f32 kernel - float64 reference|: two convex sums of <= 65 terms <= 1 and the combine, about
#                   (4 R + 16) 2^-24 = 9e-6 at R = 32; twice that (derived, not measured)
U8_MARGIN = 0.006  # > 255 * TOL: where the reference's out * 255 + 0.5 is farther than this from an integer, the byte is fixed


def photo01(photo, photo_signed=True):
    """the kernel's p in fp32 (torch): ((x + 1) / 2).clamp(0, 1), or x"""
    return ((photo + 1) / 2).clamp(0, 1) if photo_signed else photo


def distance(keep, th, tw, cell):
    """keep uint8 [B, th * tw] -> float64 numpy [B, H, W]: Chebyshev distance in pixels to the nearest pixel of an
    edited cell (0 inside one), +inf for an image without an edited cell.  Brute force over the edited cells."""
    k = np.asarray(keep.cpu()).reshape(-1, th, tw)
    B, H, W = k.shape[0], th * cell, tw * cell
    ys, xs = np.arange(H)[:, None], np.arange(W)[None, :]
    d = np.full((B, H, W), np.inf)
    for b in range(B):
        for r, c in zip(*np.nonzero(k[b] == 0)):
            dy = np.maximum(0, np.maximum(cell * r - ys, ys - (cell * r + cell - 1)))
            dx = np.maximum(0, np.maximum(cell * c - xs, xs - (cell * c + cell - 1)))
            d[b] = np.minimum(d[b], np.maximum(dy, dx))
    return d


def blur(x, taps):
    """x float64 [B, C, H, W], taps f32 [2R + 1] -> the separable blur, horizontal then vertical, replicate borders"""
    t = torch.as_tensor(np.asarray(taps), dtype=torch.float64)
    R = (t.numel() - 1) // 2
    C = x.shape[1]
    xp = F.pad(x, (R, R, R, R), mode='replicate')
    h = F.conv2d(xp, t.view(1, 1, 1, -1).repeat(C, 1, 1, 1), groups=C)
    return F.conv2d(h, t.view(1, 1, -1, 1).repeat(C, 1, 1, 1), groups=C)


def composite(dec, photo, keep, cells, r_hi=4, r_lo=32, photo_signed=True, taps=None):
    """-> dict(out float64 [B, 3, H, W], u8f float64 [B, H, W, 3] = out * 255 + 0.5 before truncation,
    u8 uint8 [B, H, W, 3], d float64 numpy [B, H, W], p fp32 [B, 3, H, W], w_lo / w_hi float64 [B, 1, H, W])"""
    dec, photo = dec.cpu(), photo.cpu()
    th, tw = cells
    B, _, H, W = dec.shape
    cell = H // th
    assert H == th * cell and W == tw * cell
    taps = composite_taps_host(r_lo) if taps is None else taps
    p32 = photo01(photo, photo_signed)
    p, dd = p32.double(), dec.double()
    d = distance(keep, th, tw, cell)
    dt = torch.from_numpy(d)[:, None]
    w_hi = (1 - dt / r_hi).clamp(min=0)
    w_lo = (1 - dt / r_lo).clamp(min=0)
    diff = dd - p
    low = blur(diff, taps)
    mix = (p + w_lo * low + w_hi * (diff - low)).clamp(0, 1)
    out = torch.where(dt == 0, dd, torch.where(dt >= r_lo, p, mix))
    u8f = (out * 255 + 0.5).permute(0, 2, 3, 1).contiguous()
    return dict(out=out, u8f=u8f, u8=u8f.clamp(0, 255).floor().to(torch.uint8), d=d, p=p32, w_lo=w_lo, w_hi=w_hi,
                low=low)


def check_u8(got, ref, cap=0.05):
    """case (h): bytes equal where the reference is not within U8_MARGIN of a rounding boundary, within +-1 elsewhere;
    the excluded share (a property of the reference and the seed alone) stays under `cap`"""
    frac = ref['u8f'] - ref['u8f'].floor()
    sure = (frac > U8_MARGIN) & (frac < 1 - U8_MARGIN)
    excluded = 1.0 - sure.double().mean().item()
    assert excluded <= cap, f'{excluded:.4f} of the bytes sit on a rounding boundary of the reference'
    got = got.cpu()
    assert torch.equal(got[sure], ref['u8'][sure])
    assert ((got.int() - ref['u8'].int()).abs() <= 1).all()
    return excluded


def inputs(B, H, W, seed, photo_range=1.2):
    """dec uniform in [0, 1], photo uniform in [-photo_range, photo_range] (beyond [-1, 1]: the clamp is exercised)"""
    g = torch.Generator().manual_seed(seed)
    dec = torch.rand(B, 3, H, W, generator=g)
    photo = (torch.rand(B, 3, H, W, generator=g) * 2 - 1) * photo_range
    return dec, photo


def keep_of(B, th, tw, edited):
    """edited: per image a list of (row, col) cells, or 'all' -> keep uint8 [B, th * tw]"""
    keep = torch.ones(B, th, tw, dtype=torch.uint8)
    for b, cells in enumerate(edited):
        if isinstance(cells, str):
            keep[b] = 0
        else:
            for r, c in cells:
                keep[b, r, c] = 0
    return keep.reshape(B, th * tw).contiguous()
