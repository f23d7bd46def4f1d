"""All-codebook fit: t2h_vq_fit_books_f32 against what the library could do for the same answer before
it -- 18 launches of t2h_vq_argmin_tex_f32, each with `tex` filled with one book id -- at n = 512, 2048, 4096 and 16384
latent rows (B = 1, 4, 8, 32) on 18 x 1024 x 256 books, and the time encode_photo adds over top_encode + bot_encode at
B = 8.  GPU only.

    python tools/vq_fit_bench.py > profiles/vq_fit_parent_vs_branch.log

Every leg is a child process under `timeout -k 10`; the first leg that fails ends the run.  Inside a leg the two
candidates alternate launch by launch (HIP events around each), the figure is the median of the timed launches after
the warm-up.  (a)'s share of the f32 matrix peak = 2 n 18432 256 FLOP / time / 157.3 TFLOP/s."""
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = (512, 2048, 4096, 16384)
NB, NE, D = 18, 1024, 256
PEAK_F32_MATRIX = 157.3e12
WARM, ITERS = 5, 30


def _events(fn):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3, out  # us


def _interleaved(fa, fb, warm=WARM, iters=ITERS):
    ta, tb = [], []
    for i in range(warm + iters):
        a, _ = _events(fa)
        b, _ = _events(fb)
        if i >= warm:
            ta.append(a)
            tb.append(b)
    return ta, tb


def _spread(t):
    s = sorted(t)
    return f'median {statistics.median(s):9.1f} us  (min {s[0]:9.1f}, max {s[-1]:9.1f}, {len(s)} launches)'


def leg_kernel(n):
    import torch
    from text2human_amd import ops
    if not torch.cuda.is_available():
        raise SystemExit('no GPU: nothing is measured without one')
    g = torch.Generator().manual_seed(n)
    z = torch.randn(n, D, generator=g).cuda()
    books = torch.randn(NB, NE, D, generator=g).cuda()
    tex = [torch.full((n, ), h, dtype=torch.int64, device='cuda') for h in range(NB)]

    def fit():
        return ops.vq_fit_books(z, books)

    def routed():
        return [ops.vq_argmin_tex(z, books, tex[h]) for h in range(NB)]

    dmin, jmin = fit()
    lists = routed()
    parent_j = torch.stack([lists[h][h] for h in range(NB)], 1)
    differ = int((parent_j != jmin.long()).sum())
    ta, tb = _interleaved(fit, routed)
    ma, mb = statistics.median(ta), statistics.median(tb)
    flop = 2.0 * n * NB * NE * D
    print(f'n = {n:5d} (B = {n // 512:2d})')
    print(f'  (a) t2h_vq_fit_books_f32, one launch          {_spread(ta)}')
    print(f'  (b) 18 x t2h_vq_argmin_tex_f32 (one book each) {_spread(tb)}')
    print(f'  (b) / (a) = {mb / ma:.1f}; (a) = {flop / (ma * 1e-6) / 1e12:.1f} TFLOP/s = '
          f'{100.0 * flop / (ma * 1e-6) / PEAK_F32_MATRIX:.1f} % of the 157.3 TFLOP/s f32 matrix rate')
    print(f'  argmin of (a) and (b) differ on {differ} of {n * NB} (row, book) pairs (near-ties: the two kernels sum in '
          f'different orders)')
    print(f'  verdict: (a) is {"FASTER" if ma < mb else "NOT faster"} than (b) at n = {n}', flush=True)


def leg_photo(B=8):
    import torch
    from text2human_amd import defaults, options, synthetic
    from text2human_amd.models import VQGANTextureAwareSpatialHierarchyInferenceModel as M
    if not torch.cuda.is_available():
        raise SystemExit('no GPU: nothing is measured without one')
    opt = options.dict_to_nonedict(defaults.sample_from_parsing())
    hier = M(opt, state_dicts=synthetic.make_state_dicts(opt, seed=1234, encode=True))
    image = (torch.rand(B, 3, 512, 256, generator=torch.Generator().manual_seed(21)) * 2 - 1).cuda()
    batch = synthetic.parsing_batch(B, seed=77)
    segm, mask = batch['segm'].cuda(), batch['texture_mask'].cuda()

    def annotated():
        hier.top_encode(image, mask)
        return hier.bot_encode(image, mask)

    def photo():
        return hier.encode_photo(image, segm)

    ta, tb = _interleaved(annotated, photo, warm=3, iters=20)
    ma, mb = statistics.median(ta), statistics.median(tb)
    print(f'encode at B = {B} (host clock of the launches included: HIP events around the whole call)')
    print(f'  top_encode + bot_encode (given mask)  {_spread(ta)}')
    print(f'  encode_photo (attributes inferred)    {_spread(tb)}')
    print(f'  added by the inference: {mb - ma:.1f} us = {100.0 * (mb - ma) / ma:.2f} %', flush=True)


def main():
    legs = [(['kernel', str(n)], 180) for n in SIZES] + [(['photo'], 420)]
    print('vq_fit_bench: t2h_vq_fit_books_f32 (a) against 18 x t2h_vq_argmin_tex_f32 (b); books 18 x 1024 x 256', flush=True)
    for args, limit in legs:
        r = subprocess.run(['timeout', '-k', '10', str(limit), sys.executable, os.path.abspath(__file__), '--leg', *args])
        if r.returncode != 0:
            print(f'leg {" ".join(args)} ended with status {r.returncode}: the run stops here', flush=True)
            return r.returncode
    return 0


if __name__ == '__main__':
    if len(sys.argv) > 2 and sys.argv[1] == '--leg':
        if sys.argv[2] == 'kernel':
            leg_kernel(int(sys.argv[3]))
        else:
            leg_photo()
    else:
        sys.exit(main())
