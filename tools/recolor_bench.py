"""Garment colour control: t2h_region_color_stats (two launches) and t2h_recolor_region_f32 (one
launch) against the same operator as eager PyTorch on the same device -- torch.isin for the membership, two grouped
conv2d over a replicate-padded map for the tent sums, masked sums for the statistics and the elementwise transform --
at B = 8, 512 x 256, three groups (upper / lower / outer) of a synthetic parsing map, feather 0 / 2 / 8, with and
without the uint8 image.  The parent has no recolouring, so the eager composition is the yardstick; it is written the
plain way and not tuned, and it is checked against tests/recolor_ref.py (float64) before anything is timed.  GPU only.

    python tools/recolor_bench.py > profiles/recolor_bench.log
    python tools/recolor_bench.py --check-eager      (no GPU needed: the eager restatement against the reference)

The measurement is one child process under `timeout -k 10`.  Warm; the two candidates alternate, HIP events around
each.  A single call on an idle device is mostly host work, so the figures are trains of 20 calls inside one pair of
events, per call, medians of 10 trains: the entry points alone into preallocated buffers (device time of the launches)
against the eager functions.  Bytes per second are the byte account of DESIGN.md 4.6l over the launch time: statistics
16 B / pixel (img 12, segm 4), apply 28 B / pixel (img 12, segm 4, out 12) plus 3 with the uint8 image."""
import ctypes
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

B, H, W = 8, 512, 256
GROUPS = ('upper', 'lower', 'outer')
LUMA, GAIN_MAX = 1.0, 4.0
COLOURS = ((0.8, 0.2, 0.3), (0.1, 0.3, 0.7), (0.9, 0.8, 0.2))
WARM, TRAINS, TRAIN = 3, 10, 20


def _events(fn):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3  # us


def _spread(t):
    s = sorted(t)
    return f'median {statistics.median(s):9.1f} us  (min {s[0]:9.1f}, max {s[-1]:9.1f}, {len(s)} trains)'


def eager_members(segm, labels):
    """segm f32 [B, H, W] -> list of bool [B, H, W], one per group (whole-number labels: isin is the membership rule)"""
    import torch
    return [torch.isin(segm, torch.tensor([float(x) for x in ids], device=segm.device)) for ids in labels]


def eager_yuv(p):
    y = 0.299 * p[:, 0] + 0.587 * p[:, 1] + 0.114 * p[:, 2]
    return y, p[:, 2] - y, p[:, 0] - y


def eager_stats(img, segm, labels, img_signed=False):
    """-> f64 [B, G, 8]; per-pixel Y / U / V in fp32, sums in float64"""
    import torch
    p = ((img + 1) / 2).clamp(0, 1) if img_signed else img
    yuv = [c.double() for c in eager_yuv(p)]
    rows = []
    for m in eager_members(segm, labels):
        md = m.double()
        n = md.sum((1, 2))
        nn = n.clamp(min=1)
        means = [(c * md).sum((1, 2)) / nn for c in yuv]
        devs = [((c * c * md).sum((1, 2)) / nn - mu * mu).clamp(min=0).sqrt() for c, mu in zip(yuv, means)]
        row = torch.stack([n] + means + devs + [torch.zeros_like(n)], 1)
        rows.append(row * (n > 0).double()[:, None])
    return torch.stack(rows, 1)


def eager_recolor(img, segm, labels, src, dst, luma=LUMA, gain_max=GAIN_MAX, feather=2, img_signed=False, want_u8=False):
    """the specification in eager torch, fp32 per pixel, constants from float64, on the tensors' device"""
    import torch
    import torch.nn.functional as F
    p = ((img + 1) / 2).clamp(0, 1) if img_signed else img
    f = int(feather)
    tent = torch.tensor([float(f + 1 - abs(j - f)) for j in range(2 * f + 1)], device=img.device)
    active = (src[..., 0] > 0) & (dst[..., 0] > 0)
    ok = (src[..., 4:7] > 1e-6) & (dst[..., 4:7] > 0)
    gain = torch.where(ok, (dst[..., 4:7] / torch.where(ok, src[..., 4:7], torch.ones_like(src[..., 4:7]))).clamp(1 / gain_max, gain_max),
                       torch.ones_like(src[..., 4:7])).float()
    sm, d_y = src[..., 1:4].float(), (luma * (dst[..., 1] - src[..., 1])).float()
    tm_u, tm_v = dst[..., 2].float(), dst[..., 3].float()
    y, u, v = eager_yuv(p)
    acc = torch.zeros_like(p)
    touched = torch.zeros_like(segm, dtype=torch.bool)
    for g, m in enumerate(eager_members(segm, labels)):
        mf = (m & active[:, g, None, None]).float()[:, None]
        n = F.conv2d(F.pad(mf, (f, f, f, f), mode='replicate'), tent.view(1, 1, 1, -1))
        n = F.conv2d(n, tent.view(1, 1, -1, 1))[:, 0]
        alpha = n / float((f + 1) ** 4)
        k = lambda t: t[:, g, None, None]  # noqa: E731
        y2 = sm[..., 0][:, g, None, None] + k(gain[..., 0]) * (y - k(sm[..., 0])) + k(d_y)
        u2 = k(tm_u) + k(gain[..., 1]) * (u - k(sm[..., 1]))
        v2 = k(tm_v) + k(gain[..., 2]) * (v - k(sm[..., 2]))
        t_rgb = torch.stack([y2 + v2, y2 - (0.299 * v2 + 0.114 * u2) / 0.587, y2 + u2], 1)
        acc = acc + alpha[:, None] * (t_rgb - p)
        touched |= n > 0
    out = torch.where(touched[:, None], (p + acc).clamp(0, 1), p)
    u8 = (out * 255 + 0.5).clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous() if want_u8 else None
    return out, u8


def inputs(batch=B, h=H, w=W, device='cpu'):
    import torch
    from text2human_amd import synthetic
    img = torch.rand(batch, 3, h, w, generator=torch.Generator().manual_seed(1))
    segm = synthetic.parsing_batch(batch, seed=77, height=h, width=w)['segm'].reshape(batch, h, w).contiguous()
    return img.to(device), segm.to(device)


def targets(src):
    """plain colours: the source's statistics with the means replaced (what model.recolor builds)"""
    import torch
    from text2human_amd import ops
    dst = src.clone()
    dst[:, :, 1:4] = ops.recolor_yuv(torch.tensor(COLOURS, dtype=torch.float64)).to(src.device)
    return dst * (src[..., :1] > 0)


def check_eager(device='cpu', batch=2, h=96, w=80):
    """the eager restatement against tests/recolor_ref.py (float64) -> the largest differences"""
    import numpy as np
    import recolor_ref as R
    from text2human_amd import ops
    img, segm = inputs(batch, h, w, device)
    labels = [ops.RECOLOR_GROUPS[n] for n in GROUPS]
    bits = [R.bits_of(ids) for ids in labels]
    st = eager_stats(img, segm, labels)
    ref_st = R.stats(img, segm, bits)
    assert np.array_equal(st[..., 0].cpu().numpy(), ref_st[..., 0]) and ref_st[..., 0].max() > 0
    d_st = float(np.abs(st.cpu().numpy() - ref_st)[..., 1:7].max())
    assert d_st <= R.STATS_TOL, d_st
    worst = 0.0
    for f in (0, 2, 8):
        out, u8 = eager_recolor(img, segm, labels, st, targets(st), feather=f, want_u8=True)
        ref = R.recolor(img, segm, bits, st.cpu().numpy(), targets(st).cpu().numpy(), LUMA, GAIN_MAX, f)
        worst = max(worst, (out.cpu().double() - ref['out']).abs().max().item())
        R.check_u8(u8, ref)
    assert worst <= R.TOL, worst
    return d_st, worst


def leg():
    import torch
    from text2human_amd import ops
    if not torch.cuda.is_available():
        raise SystemExit('no GPU: nothing is measured without one')
    d_st, d_out = check_eager('cuda')
    print(f'eager restatement against the float64 reference (96 x 80): statistics within {d_st:.1e}, out within {d_out:.1e}')
    img, segm = inputs(device='cuda')
    labels = [ops.RECOLOR_GROUPS[n] for n in GROUPS]
    G, npix = len(GROUPS), B * H * W
    lib, st = ops._lib.load(), ops._stream()
    bits = (ctypes.c_uint64 * G)(*ops.recolor_group_bits(list(GROUPS)))
    src = ops.region_color_stats(img, segm, list(GROUPS))
    e_src = eager_stats(img, segm, labels)
    dst = targets(src)
    counts = src[..., 0].mean(0).tolist()
    print(f'B = {B}, {H} x {W}, groups {GROUPS}: mean member pixels per image {[int(c) for c in counts]} of {H * W}; '
          f'max |stats - eager| = {(src - e_src).abs()[..., 1:7].max().item():.1e}')

    def trains(kernel, eager):
        tk, te = [], []
        for i in range(WARM + TRAINS):
            a = _events(lambda: [kernel() for _ in range(TRAIN)])
            b = _events(lambda: [eager() for _ in range(TRAIN)])
            if i >= WARM:
                tk.append(a / TRAIN)
                te.append(b / TRAIN)
        return tk, te

    verdicts = []
    partial = torch.empty((B, (H + ops.RECOLOR_STRIPE - 1) // ops.RECOLOR_STRIPE, G, 8), dtype=torch.float64, device='cuda')
    stats = torch.empty((B, G, 8), dtype=torch.float64, device='cuda')
    s_args = (ops._p(img), 0, ops._p(segm), bits, G, B, H, W, ops._p(partial), ops._p(stats), st)
    tk, te = trains(lambda: lib.t2h_region_color_stats(*s_args), lambda: eager_stats(img, segm, labels))
    assert torch.equal(stats, src)
    mk, me = statistics.median(tk), statistics.median(te)
    print('statistics (two launches: stripes, then one workgroup per image)')
    print(f'  (a) t2h_region_color_stats, {TRAIN} back to back   {_spread(tk)} per call')
    print(f'  (b) eager PyTorch, {TRAIN} calls back to back      {_spread(te)} per call')
    print(f'  (b) / (a) = {me / mk:.1f}; (a) reads {16 * npix / 1e6:.1f} MB at {16 * npix / (mk * 1e-6) / 1e12:.2f} TB/s')
    verdicts.append(mk <= me)
    out = torch.empty_like(img)
    u8 = torch.empty((B, H, W, 3), dtype=torch.uint8, device='cuda')
    for f in (0, 2, 8):
        for want_u8 in (False, True):
            a_args = (ops._p(img), 0, ops._p(segm), bits, G, ops._p(src), ops._p(dst), LUMA, GAIN_MAX, f, ops._p(out),
                      ops._p(u8) if want_u8 else None, B, H, W, st)
            tk, te = trains(lambda: lib.t2h_recolor_region_f32(*a_args),
                            lambda: eager_recolor(img, segm, labels, src, dst, feather=f, want_u8=want_u8))
            e_out, _ = eager_recolor(img, segm, labels, src, dst, feather=f)
            diff = (out - e_out).abs().max().item()
            nbytes = (28 + (3 if want_u8 else 0)) * npix
            mk, me = statistics.median(tk), statistics.median(te)
            print(f'apply, feather {f}, {"f32 + uint8" if want_u8 else "f32 only"} (one launch)')
            print(f'  (a) t2h_recolor_region_f32, {TRAIN} back to back   {_spread(tk)} per launch')
            print(f'  (b) eager PyTorch, {TRAIN} calls back to back      {_spread(te)} per call')
            print(f'  (b) / (a) = {me / mk:.1f}; (a) moves {nbytes / 1e6:.1f} MB at {nbytes / (mk * 1e-6) / 1e12:.2f} TB/s; '
                  f'max |a - b| = {diff:.2e}', flush=True)
            verdicts.append(mk <= me)
    print(f'verdict: the kernels are {"NOT SLOWER" if all(verdicts) else "SLOWER"} than eager PyTorch in '
          f'{sum(verdicts)} of {len(verdicts)} configurations', flush=True)


def main():
    print('recolor_bench: t2h_region_color_stats / t2h_recolor_region_f32 (a) against eager PyTorch on the same device (b)',
          flush=True)
    r = subprocess.run(['timeout', '-k', '10', '300', sys.executable, os.path.abspath(__file__), '--leg'])
    if r.returncode != 0:
        print(f'the measurement ended with status {r.returncode}', flush=True)
    return r.returncode


if __name__ == '__main__':
    if len(sys.argv) > 1 and sys.argv[1] == '--leg':
        leg()
    elif len(sys.argv) > 1 and sys.argv[1] == '--check-eager':
        print('eager restatement against the float64 reference on the host: statistics within %.1e, out within %.1e'
              % check_eager('cpu'))
    else:
        sys.exit(main())
