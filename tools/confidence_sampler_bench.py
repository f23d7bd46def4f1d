"""Timing of confidence-ordered decoding against the reference's loop (not bench.py: the headline stays the reference
loop's).  Synthetic checkpoint, one GPU, warm; medians of --runs runs taken interleaved:
(a) sample_fn, 256 steps (the default path), (b) sample_fn_confidence at R = 8, 16, 32 -- at B = 8 and B = 1.

    python tools/confidence_sampler_bench.py [--runs 10] [--batches 8 1]
    rocprofv3 --kernel-trace --stats -d DIR -o conf --output-format csv -- python tools/confidence_sampler_bench.py --profile
    python tools/confidence_sampler_bench.py --split DIR    # kernel time of a round: transformer / tail / commit

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

TAIL = ('conf_group_kernel', 'conf_logits_kernel', 'conf_pick_kernel')
COMMIT = ('conf_commit_kernel', 'schedule_advance_kernel')


def split(directory):
    files = glob.glob(os.path.join(directory, '**', '*kernel_stats.csv'), recursive=True)
    if not files:
        raise SystemExit(f'no *kernel_stats.csv under {directory}')
    tot = dict(transformer=0.0, tail=0.0, commit=0.0, other=0.0)
    for row in csv.DictReader(open(files[0])):
        name, ns = row['Name'], float(row['TotalDurationNs'])
        if any(k in name for k in TAIL):
            tot['tail'] += ns
        elif any(k in name for k in COMMIT):
            tot['commit'] += ns
        elif any(k in name for k in ('Cijk', 'at::', 'elementwise', 'fill', 'copy')):
            tot['other'] += ns
        else:
            tot['transformer'] += ns
    s = sum(tot.values())
    print(json.dumps(dict(kernel_time_ms={k: round(v / 1e6, 3) for k, v in tot.items()},
                          share={k: round(v / s, 4) for k, v in tot.items()})))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=10)
    ap.add_argument('--batches', type=int, nargs='+', default=[8, 1])
    ap.add_argument('--rounds', type=int, nargs='+', default=[8, 16, 32])
    ap.add_argument('--profile', action='store_true', help='one warm sample_fn_confidence (B = 8, R = 16) and nothing else')
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
        torch.manual_seed(1)
        model.sample_fn_confidence(rounds=16)
        torch.cuda.synchronize()
        return
    for B in args.batches:
        model.feed_data(synthetic.parsing_batch(B, seed=2021))
        legs = {'sample_fn_256': lambda: model.sample_fn(temp=1, sample_steps=256)}
        for R in args.rounds:
            legs[f'confidence_R{R}'] = (lambda R=R: model.sample_fn_confidence(rounds=R))
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
                              speedup_vs_sample_fn={k: round(med['sample_fn_256'] / v, 2) for k, v in med.items()},
                              evaluations=dict(model.sampler_fn.last_stats))), flush=True)


if __name__ == '__main__':
    main()
