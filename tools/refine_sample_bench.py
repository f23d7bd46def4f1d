"""Cost of the sampled bottom-index refinement kernel -- not bench.py: the default decode runs the
argmax kernel, unchanged.  On the product shapes (n = B * 512 token rows at B = 8 and B = 32, the checkpoint's head
shape: Cf features, 1024 classes, 18 heads; synthetic weights, random features and textures) it times, in one
process, interleaved:

    argmax          t2h_routed_head_argmax
    sample          t2h_routed_head_sample, Philox noise in the kernel, truncation off
    sample_trunc    the same with top_k = 64 and top_p = 0.9
    sample_logp     truncation off, logp and logits_ws written too
    philox          t2h_philox_exponential_f32 for the same n * n_class elements

Each figure is device time between two events around --iters back-to-back launches, divided by --iters; the median,
minimum and maximum of --runs such windows taken round-robin over the legs.

    python tools/refine_sample_bench.py [--batches 8 32] [--iters 200] [--runs 9] > profiles/refine_sample.log"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', type=int, nargs='+', default=[8, 32])
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--runs', type=int, default=9)
    args = ap.parse_args()
    import torch

    from text2human_amd import defaults, ops, options, synthetic
    from text2human_amd.models import SampleFromParsingModel
    if not torch.cuda.is_available():
        raise SystemExit('refine_sample_bench needs a GPU')
    opt = options.dict_to_nonedict(defaults.sample_from_parsing())
    model = SampleFromParsingModel(opt, state_dicts=synthetic.make_state_dicts(opt, seed=1234))
    P, ipd = model.P, model.ipd
    n_heads, cf, n_class = ipd['n_heads'], ipd['cf'], ipd['n_class']
    w, b = P['ipd.seg.w'], P['ipd.seg.b']
    dev = model.device
    for B in args.batches:
        n = B * 512
        g = torch.Generator(device=dev).manual_seed(B)
        feat = torch.randn(n, n_heads * cf, device=dev, generator=g).relu_()
        tex = torch.randint(0, n_heads, (n, ), device=dev, generator=g)
        head = (feat, w, b, tex, n_heads, cf, n_class)
        noise = dict(philox=(2021, 0))
        legs = {
            'argmax': lambda: ops.routed_head_argmax(*head),
            'sample': lambda: ops.routed_head_sample(*head, **noise),
            'sample_trunc': lambda: ops.routed_head_sample(*head, top_k=64, top_p=0.9, **noise),
            'sample_logp': lambda: ops.routed_head_sample(*head, want_logp=True, want_logits=True, **noise),
            'philox': lambda: ops.philox_exponential(2021, 0, n * n_class, dev),
        }
        for fn in legs.values():   # warm: code objects loaded, the allocator holds every output size
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        us = {k: [] for k in legs}
        for _ in range(args.runs):
            for k, fn in legs.items():   # round-robin
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                for _ in range(args.iters):
                    fn()
                t1.record()
                t1.synchronize()
                us[k].append(t0.elapsed_time(t1) * 1e3 / args.iters)
        med = {k: statistics.median(v) for k, v in us.items()}
        print(json.dumps(dict(batch=B, n=n, n_heads=n_heads, Cf=cf, n_class=n_class, iters=args.iters, runs=args.runs,
                              median_us={k: round(v, 2) for k, v in med.items()},
                              min_us={k: round(min(v), 2) for k, v in us.items()},
                              max_us={k: round(max(v), 2) for k, v in us.items()},
                              sample_over_argmax_plus_philox=round(med['sample'] / (med['argmax'] + med['philox']), 3),
                              sample_trunc_over_sample=round(med['sample_trunc'] / med['sample'], 3))), flush=True)


if __name__ == '__main__':
    main()
