"""Two-band compositing: t2h_composite_region_f32 (ops.composite_region, one launch) against the same
formula as eager PyTorch on the same device -- F.pad(mode='replicate'), two grouped conv2d, a max-pool-based distance
and the elementwise combine -- at B = 8, 512 x 256, for three regions: one cell, a garment-sized block of 120 cells,
and all cells but one.  The parent has no compositing, so eager composition is the baseline; it is written the plain
way and not tuned.  GPU only.

    python tools/composite_bench.py > profiles/composite_bench.log

The measurement is one child process under `timeout -k 10`.  The two candidates alternate call by call (HIP events
around each, f32 output only, no uint8), the figure is the median of the timed calls after the warm-up, with min and
max beside it.  One call on an idle device is mostly host work, so each candidate is also timed as a train of 20 calls
inside one pair of events (the kernel: the entry point alone into one preallocated output), per call.  Beside them: the traffic floor of the operation, 3 x B 3 H W 4 bytes (read dec, read photo, write out),
and the decode stage's 2.06 ms per image (profiles/r06_bench_driver_cmd.json) for scale."""
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, H, W, TH, TW, CELL = 8, 512, 256, 32, 16, 16
R_HI, R_LO = 4, 32
WARM, ITERS, TRAIN = 10, 50, 20
DECODE_MS_PER_IMAGE = 2.06


def _events(fn):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3, out  # us


def _spread(t):
    s = sorted(t)
    return f'median {statistics.median(s):9.1f} us  (min {s[0]:9.1f}, max {s[-1]:9.1f}, {len(s)} calls)'


def eager_composite(dec, photo, keep, taps, r_hi=R_HI, r_lo=R_LO):
    """the specification in eager torch, fp32, on the tensors' device"""
    import torch
    import torch.nn.functional as F
    p = ((photo + 1) / 2).clamp(0, 1)
    edited = (keep == 0).view(-1, 1, TH, TW).float().repeat_interleave(CELL, 2).repeat_interleave(CELL, 3)
    # Chebyshev distance capped at r_lo: r_lo minus the number of dilations k = 0 .. r_lo - 1 that reach the pixel
    m, reached = edited, edited.clone()
    for _ in range(1, r_lo):
        m = F.max_pool2d(m, 3, 1, 1)
        reached += m
    d = r_lo - reached
    w_hi, w_lo = (1 - d / r_hi).clamp(min=0), (1 - d / r_lo).clamp(min=0)
    diff = dec - p
    R = (taps.numel() - 1) // 2
    low = F.conv2d(F.pad(diff, (R, R, R, R), mode='replicate'), taps.view(1, 1, 1, -1).repeat(3, 1, 1, 1), groups=3)
    low = F.conv2d(low, taps.view(1, 1, -1, 1).repeat(3, 1, 1, 1), groups=3)
    mix = (p + w_lo * low + w_hi * (diff - low)).clamp(0, 1)
    return torch.where(d == 0, dec, torch.where(d >= r_lo, p, mix))


def leg():
    import torch
    from text2human_amd import ops
    if not torch.cuda.is_available():
        raise SystemExit('no GPU: nothing is measured without one')
    g = torch.Generator().manual_seed(1)
    dec = torch.rand(B, 3, H, W, generator=g).cuda()
    photo = (torch.rand(B, 3, H, W, generator=g) * 2 - 1).cuda()
    taps = torch.from_numpy(ops.composite_taps_host(R_LO)).cuda()
    one = torch.ones(B, TH, TW, dtype=torch.uint8)
    one[:, 16, 8] = 0
    garment = torch.ones(B, TH, TW, dtype=torch.uint8)
    garment[:, 8:20, 3:13] = 0
    most = torch.zeros(B, TH, TW, dtype=torch.uint8)
    most[:, 16, 8] = 1
    floor_bytes = 3 * B * 3 * H * W * 4
    print(f'B = {B}, {H} x {W}, cells {TH} x {TW}, r_hi = {R_HI}, r_lo = {R_LO}, taps [{taps.numel()}]; traffic floor '
          f'{floor_bytes / 1e6:.1f} MB; decode stage for scale: {DECODE_MS_PER_IMAGE} ms / image = '
          f'{DECODE_MS_PER_IMAGE * B * 1e3:.0f} us at B = {B}')
    none = torch.ones(B, TH, TW, dtype=torch.uint8)  # (beside the three regions: no blended tile at all, every tile copies)
    for name, k in (('one cell', one), ('garment, 120 cells', garment), ('all cells but one', most),
                    ('no cell (every tile a copy of the photo)', none)):
        keep = k.reshape(B, TH * TW).contiguous().cuda()

        def kernel():
            return ops.composite_region(dec, photo, keep, (TH, TW), r_hi=R_HI, r_lo=R_LO)[0]

        def eager():
            return eager_composite(dec, photo, keep, taps)

        diff = (kernel() - eager()).abs().max().item()
        ta, tb = [], []
        for i in range(WARM + ITERS):
            a, _ = _events(kernel)
            b, _ = _events(eager)
            if i >= WARM:
                ta.append(a)
                tb.append(b)
        # a single call on an idle device is mostly its host side (the wrapper's checks and allocations, the launch):
        # TRAIN launches of the entry point alone into one output buffer, back to back inside one pair of events,
        # show what the kernel itself takes; the same train of eager calls beside it
        out = torch.empty_like(dec)
        lib, st = ops._lib.load(), ops._stream()
        args = (ops._p(dec), ops._p(photo), ops._p(keep), ops._p(taps), ops._p(out), None, B, H, W, TH, TW, R_HI, R_LO,
                (taps.numel() - 1) // 2, 1, st)

        def kernel_train():
            for _ in range(TRAIN):
                lib.t2h_composite_region_f32(*args)

        def eager_train():
            for _ in range(TRAIN):
                eager()

        tk, te = [], []
        for i in range(3 + 10):
            a, _ = _events(kernel_train)
            b, _ = _events(eager_train)
            if i >= 3:
                tk.append(a / TRAIN)
                te.append(b / TRAIN)
        assert torch.equal(out, kernel())
        ma, mb, mk, me = (statistics.median(t) for t in (ta, tb, tk, te))
        print(f'{name}: {int((k[0] == 0).sum())} of {TH * TW} cells edited per image')
        print(f'  (a) ops.composite_region, one call        {_spread(ta)}')
        print(f'  (b) eager PyTorch, the same formula       {_spread(tb)}')
        print(f'  (a\') the launch alone, {TRAIN} back to back  {_spread(tk)} per launch')
        print(f'  (b\') eager, {TRAIN} calls back to back       {_spread(te)} per call')
        print(f'  (b) / (a) = {mb / ma:.1f}, (b\') / (a\') = {me / mk:.1f}; (a\') moves the floor\'s bytes at '
              f'{floor_bytes / (mk * 1e-6) / 1e12:.2f} TB/s and is {100.0 * mk / (DECODE_MS_PER_IMAGE * B * 1e3):.2f} % of '
              f'the decode stage; max |a - b| = {diff:.2e}')
        print(f'  verdict: (a) is {"FASTER" if ma < mb and mk < me else "NOT faster"} than (b)', flush=True)


def main():
    print('composite_bench: t2h_composite_region_f32 (a) against eager PyTorch on the same device (b)', flush=True)
    r = subprocess.run(['timeout', '-k', '10', '300', sys.executable, os.path.abspath(__file__), '--leg'])
    if r.returncode != 0:
        print(f'the measurement ended with status {r.returncode}', flush=True)
    return r.returncode


if __name__ == '__main__':
    if len(sys.argv) > 1 and sys.argv[1] == '--leg':
        leg()
    else:
        sys.exit(main())
