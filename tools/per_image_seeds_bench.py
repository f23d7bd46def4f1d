"""Per-image seeds against the shared stream -- not bench.py: the headline stays the reference loop.
Synthetic checkpoint, one GPU, B = 8, 256 steps, graph path, warm (every graph of both keys captured); --runs interleaved
runs, wall time around the call with a device synchronisation:

    plain    sample_fn(temp=1, sample_steps)                 one schedule for the batch, the shared generator stream
    seeded   sample_fn(temp=1, sample_steps, seeds=[...])    every image on the schedule of its own seed

Every image of the seeded call follows its own schedule, so the two calls run different numbers of rounds: the figure to
compare is the time PER ROUND, reported with the rounds of both.  The script also asserts what the path promises: the
first image of every seeded batch equals the seeded call on that image alone.

    python tools/per_image_seeds_bench.py [--runs 5] [--steps 256] [--batch 8]

Says nothing about image quality (synthetic weights)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=5)
    ap.add_argument('--steps', type=int, default=256)
    ap.add_argument('--batch', type=int, default=8)
    args = ap.parse_args()
    import torch

    from text2human_amd import defaults, options, synthetic
    from text2human_amd.models import SampleFromParsingModel
    opt = options.dict_to_nonedict(defaults.sample_from_parsing())
    model = SampleFromParsingModel(opt, state_dicts=synthetic.make_state_dicts(opt, seed=1234))
    batch = synthetic.parsing_batch(args.batch, seed=2021)
    model.feed_data(batch)
    net = model.sampler_fn

    def seed(s):
        torch.manual_seed(s)
        torch.cuda.manual_seed_all(s)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    seeds_of = lambda i: [options.image_seed(1000 + i, f'{b}.png') for b in range(args.batch)]
    plain = lambda: model.sample_fn(temp=1, sample_steps=args.steps)
    seeded = lambda i: model.sample_fn(temp=1, sample_steps=args.steps, seeds=seeds_of(i))
    # warm: the graphs of every padded width the runs below meet (a width is a power of two: a few runs find them all)
    for i in range(3):
        seed(i)
        plain()
        seeded(i)
    captures = lambda: sum(g.captures for g in net._graphs.values())
    ms = {'plain': [], 'seeded': []}
    rounds = {'plain': [], 'seeded': []}
    launched = {'plain': [], 'seeded': []}
    n_cap = captures()
    firsts = []
    for i in range(args.runs):   # interleaved
        seed(100 + i)
        t, _ = timed(plain)
        ms['plain'].append(t)
        rounds['plain'].append(net.last_stats['rounds'])
        launched['plain'].append(net.last_stats['sample_steps_launched'])
        assert net.last_launch_mode == 'graph'
        t, out = timed(lambda: seeded(100 + i))
        ms['seeded'].append(t)
        rounds['seeded'].append(net.last_stats['rounds'])
        launched['seeded'].append(net.last_stats['sample_steps_launched'])
        assert net.last_launch_mode == 'graph'
        firsts.append((seeds_of(100 + i)[0], torch.stack(out)[:, 0].clone()))
    new_captures = captures() - n_cap
    # what the path promises, on the runs just timed: image 0 alone under its seed is image 0 of the batch
    model.feed_data({k: (v[:1] if torch.is_tensor(v) else v[:1]) for k, v in batch.items()})
    for s, want in firsts:
        got = torch.stack(model.sample_fn(temp=1, sample_steps=args.steps, seeds=[s]))[:, 0]
        assert torch.equal(got, want), 'image 0 of a seeded batch differs from the seeded call on image 0 alone'
    per_round = {k: [m / r for m, r in zip(ms[k], rounds[k])] for k in ms}
    print(json.dumps(dict(batch=args.batch, steps=args.steps, runs=args.runs, launch_mode='graph',
                          ms={k: [round(x, 2) for x in v] for k, v in ms.items()},
                          rounds=rounds, sample_rounds_launched=launched,
                          ms_per_round={k: [round(x, 4) for x in v] for k, v in per_round.items()},
                          median_ms={k: round(statistics.median(v), 2) for k, v in ms.items()},
                          median_ms_per_round={k: round(statistics.median(v), 4) for k, v in per_round.items()},
                          graphs_captured_during_timed_runs=new_captures,
                          image_0_alone='equal to image 0 of every timed seeded batch')), flush=True)


if __name__ == '__main__':
    main()
