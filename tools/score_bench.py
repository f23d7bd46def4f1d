"""Scoring a token map against drawing one -- not bench.py: the headline stays the reference loop.
Synthetic checkpoint, one GPU, B = 8, warm (every graph of both keys captured); --runs interleaved runs, wall time around
the call with a device synchronisation:

    sample_logp   sample_fn(temp=1, sample_steps, return_logp=True)
    score         score_fn(that call's token lists, temp=1, sample_steps) from the same generator state
    score_rank    the same with return_rank=True

The timing script also asserts the round trip: the scored logp has the bits of the drawn one.

    python tools/score_bench.py [--runs 5] [--steps 256]

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
    model.feed_data(synthetic.parsing_batch(args.batch, seed=2021))

    def seed(s):
        torch.manual_seed(s)
        torch.cuda.manual_seed_all(s)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    draw = lambda: model.sample_fn(temp=1, sample_steps=args.steps, return_logp=True)
    seed(0)
    lists, _ = draw()   # warm: graphs captured, workspaces sized
    seed(0)
    model.score_fn(lists, sample_steps=args.steps)
    model.score_fn(lists, sample_steps=args.steps, return_rank=True)
    ms = {'sample_logp': [], 'score': [], 'score_rank': []}
    for i in range(args.runs):   # interleaved
        seed(100 + i)
        t, (lists, logp) = timed(draw)
        ms['sample_logp'].append(t)
        seed(100 + i)
        t, got = timed(lambda: model.score_fn(lists, sample_steps=args.steps))
        ms['score'].append(t)
        assert got.cpu().numpy().tobytes() == logp.cpu().numpy().tobytes(), 'round trip: the bits differ'
        seed(100 + i)
        t, (got, rank) = timed(lambda: model.score_fn(lists, sample_steps=args.steps, return_rank=True))
        ms['score_rank'].append(t)
        assert got.cpu().numpy().tobytes() == logp.cpu().numpy().tobytes() and int(rank.min()) >= 0
    print(json.dumps(dict(batch=args.batch, steps=args.steps, runs=args.runs, launch_mode=model.sampler_fn.last_launch_mode,
                          ms={k: [round(x, 2) for x in v] for k, v in ms.items()},
                          median_ms={k: round(statistics.median(v), 2) for k, v in ms.items()},
                          round_trip='equal as bytes')), flush=True)


if __name__ == '__main__':
    main()
