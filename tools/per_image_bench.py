"""A temperature sweep as ONE batch with per-image controls against the same sweep as one scalar call per point
("Per-image sampling controls") -- not bench.py: the headline stays the scalar reference loop.  Synthetic
checkpoint, one GPU, warm; medians of --runs runs taken interleaved:

    sweep/per_image_B8   sample_fn(temp=[t0 .. t7]) on a batch of 8 copies of one parsing map: eight temperatures, one call
    sweep/scalar_8xB1    sample_fn(temp=t) on that map alone, eight calls (eight sets of captured rounds, all warm)
    uniform/scalar_B8    sample_fn(temp=1) on the batch of 8 (what the per-image call costs without the table)

    python tools/per_image_bench.py [--runs 5] [--steps 256]

Says nothing about image quality (synthetic weights)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TEMPS = [0.5, 0.6, 0.7, 0.8, 0.9, 1.0, 1.1, 1.2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=5)
    ap.add_argument('--steps', type=int, default=256)
    args = ap.parse_args()
    import torch

    from text2human_amd import defaults, options, synthetic
    from text2human_amd.models import SampleFromParsingModel
    opt = options.dict_to_nonedict(defaults.sample_from_parsing())
    sds = synthetic.make_state_dicts(opt, seed=1234)
    one = synthetic.parsing_batch(1, seed=2021)
    eight = {k: (torch.cat([v] * 8) if torch.is_tensor(v) else v * 8) for k, v in one.items()}
    batch, single = SampleFromParsingModel(opt, state_dicts=sds), SampleFromParsingModel(opt, state_dicts=sds)
    batch.feed_data(eight)
    single.feed_data(one)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def scalar_sweep():
        for t in TEMPS:
            single.sample_fn(temp=t, sample_steps=args.steps)

    legs = {'sweep/per_image_B8': lambda: batch.sample_fn(temp=TEMPS, sample_steps=args.steps),
            'sweep/scalar_8xB1': scalar_sweep,
            'uniform/scalar_B8': lambda: batch.sample_fn(temp=1, sample_steps=args.steps)}
    for fn in legs.values():   # warm: graphs captured, workspaces sized
        torch.manual_seed(0)
        fn()
    ms = {k: [] for k in legs}
    for i in range(args.runs):
        for k, fn in legs.items():   # interleaved
            torch.manual_seed(100 + i)
            ms[k].append(timed(fn))
    med = {k: statistics.median(v) for k, v in ms.items()}
    print(json.dumps(dict(temps=TEMPS, steps=args.steps, runs=args.runs, median_ms={k: round(v, 2) for k, v in med.items()},
                          min_ms={k: round(min(v), 2) for k, v in ms.items()},
                          max_ms={k: round(max(v), 2) for k, v in ms.items()},
                          scalar_sweep_over_per_image=round(med['sweep/scalar_8xB1'] / med['sweep/per_image_B8'], 3))),
          flush=True)


if __name__ == '__main__':
    main()
