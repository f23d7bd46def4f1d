"""Cost of truncated sampling (top-k / top-p) -- not bench.py: the headline stays the untruncated
reference loop.  Synthetic checkpoint, one GPU, warm; medians of --runs runs taken interleaved: sample_fn (256 steps)
and sample_fn_confidence (R = 16), each with truncation off, top_k = 64, top_p = 0.9 and both, at B = 8 and B = 1.

    python tools/truncation_bench.py [--runs 10] [--batches 8 1]
    python tools/truncation_bench.py --off-only      # the two untruncated legs alone (also runs on a tree without the
                                                     # feature: the parent commit built next to this one, interleaved)
    rocprofv3 --kernel-trace --stats -d DIR -o trunc --output-format csv -- python tools/truncation_bench.py --profile
    python tools/truncation_bench.py --split DIR     # where the kernel time of that call goes

Says nothing about image quality (synthetic weights)."""
import argparse
import csv
import glob
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SETTINGS = {'off': {}, 'top_k64': dict(top_k=64), 'top_p0.9': dict(top_p=0.9), 'both': dict(top_k=64, top_p=0.9)}


def split(directory):
    files = glob.glob(os.path.join(directory, '**', '*kernel_stats.csv'), recursive=True)
    if not files:
        raise SystemExit(f'no *kernel_stats.csv under {directory}')
    rows = [(r['Name'], float(r['TotalDurationNs']), int(r['Calls'])) for r in csv.DictReader(open(files[0]))]
    total = sum(ns for _, ns, _ in rows)
    pick = {n: (ns, c) for n, ns, c in rows if 'conf_pick_kernel' in n or 'sample_pick_kernel' in n}
    tail = sum(ns for n, ns, _ in rows if any(k in n for k in ('conf_group_kernel', 'conf_logits_kernel', 'conf_pick_kernel')))
    print(json.dumps(dict(total_kernel_ms=round(total / 1e6, 3), tail_share=round(tail / total, 4),
                          pick={n[:60]: dict(ms=round(ns / 1e6, 3), calls=c, avg_us=round(ns / c / 1e3, 2),
                                             share=round(ns / total, 4)) for n, (ns, c) in pick.items()})))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=10)
    ap.add_argument('--batches', type=int, nargs='+', default=[8, 1])
    ap.add_argument('--rounds', type=int, default=16)
    ap.add_argument('--off-only', action='store_true')
    ap.add_argument('--profile', action='store_true',
                    help='one warm sample_fn_confidence (B = 8, R = 16, top_k = 64, top_p = 0.9) and nothing else')
    ap.add_argument('--split', default=None)
    args = ap.parse_args()
    if args.split:
        return split(args.split)
    import torch

    from text2human_amd import defaults, options, synthetic
    from text2human_amd.models import SampleFromParsingModel
    opt = options.dict_to_nonedict(defaults.sample_from_parsing())
    model = SampleFromParsingModel(opt, state_dicts=synthetic.make_state_dicts(opt, seed=1234))

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    if args.profile:
        model.feed_data(synthetic.parsing_batch(8, seed=2021))
        for _ in range(2):
            torch.manual_seed(1)
            model.sample_fn_confidence(rounds=args.rounds, **SETTINGS['both'])
        torch.cuda.synchronize()
        return
    settings = {'off': {}} if args.off_only else SETTINGS
    for B in args.batches:
        model.feed_data(synthetic.parsing_batch(B, seed=2021))
        legs = {}
        for name, kw in settings.items():
            legs[f'sample_fn_256/{name}'] = (lambda kw=kw: model.sample_fn(temp=1, sample_steps=256, **kw))
            legs[f'confidence_R{args.rounds}/{name}'] = (lambda kw=kw: model.sample_fn_confidence(rounds=args.rounds, **kw))
        for fn in legs.values():   # warm: graphs captured, workspaces sized
            torch.manual_seed(0)
            fn()
        ms = {k: [] for k in legs}
        for i in range(args.runs):
            for k, fn in legs.items():   # interleaved
                torch.manual_seed(100 + i)
                ms[k].append(timed(fn))
        med = {k: statistics.median(v) for k, v in ms.items()}
        print(json.dumps(dict(batch=B, runs=args.runs, median_ms={k: round(v, 2) for k, v in med.items()},
                              min_ms={k: round(min(v), 2) for k, v in ms.items()},
                              max_ms={k: round(max(v), 2) for k, v in ms.items()},
                              vs_off={k: round(v / med[k.split('/')[0] + '/off'], 4) for k, v in med.items()})), flush=True)


if __name__ == '__main__':
    main()
