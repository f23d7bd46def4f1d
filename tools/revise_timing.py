"""Self-correction against drawing a map -- not bench.py: the headline stays the reference loop.
Synthetic checkpoint, one GPU, one process, B = 8 and B = 1, warm (one untimed call of everything first: graphs captured,
workspaces sized); --runs interleaved runs, wall time around the call with a device synchronisation, the median of them:

    sample        sample_fn(temp=1, sample_steps)
    pll           pll_fn(that map, folds=4)
    revise        revise_fn(that map, passes=1, fraction=0.25, sample_steps)
    pll_k_calls   (B = 1) the critic as K calls at batch 1 instead of one batch of K -- the figure behind the batching rule

and the C-ABI launches each call makes.  Every step (a warm-up or one timed round of a batch size) runs under a time
limit of its own (--limit seconds): a step that exceeds it ends the script, nothing more is started on the GPU.

    python tools/revise_timing.py [--runs 5] [--steps 256] [--out profiles/revise_timing.log]

Says nothing about image quality (synthetic weights)."""
import argparse
import json
import os
import signal
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


class StepTimeout(Exception):
    pass


def limited(seconds, fn):
    """fn() under a wall-clock limit of its own"""
    def on_alarm(signum, frame):
        raise StepTimeout()
    old = signal.signal(signal.SIGALRM, on_alarm)
    signal.alarm(int(seconds))
    try:
        return fn()
    finally:
        signal.alarm(0)
        signal.signal(signal.SIGALRM, old)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=5)
    ap.add_argument('--steps', type=int, default=256)
    ap.add_argument('--limit', type=int, default=120, help='seconds per step')
    ap.add_argument('--out', default=None, help='also append the result lines to this file')
    args = ap.parse_args()
    import torch

    from text2human_amd import _lib, defaults, options, synthetic
    from text2human_amd.models import SampleFromParsingModel
    opt = options.dict_to_nonedict(defaults.sample_from_parsing())
    model = SampleFromParsingModel(opt, state_dicts=synthetic.make_state_dicts(opt, seed=1234))
    lines = []

    def emit(d):
        line = json.dumps(d)
        print(line, flush=True)
        lines.append(line)

    def seed(s):
        torch.manual_seed(s)
        torch.cuda.manual_seed_all(s)

    def timed(fn):
        torch.cuda.synchronize()
        calls, t0 = _lib.n_calls, time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, _lib.n_calls - calls, out

    def k_calls(fn):
        """fn() with the critic's evaluations as K calls at batch B (the rule's other branch)"""
        was = options.PLL_BATCH_MAX
        options.PLL_BATCH_MAX = 0
        try:
            return fn()
        finally:
            options.PLL_BATCH_MAX = was

    try:
        for batch in (8, 1):
            model.feed_data(synthetic.parsing_batch(batch, seed=2021))
            draw = lambda: model.sample_fn(temp=1, sample_steps=args.steps)
            what = {'sample': draw,
                    'pll': lambda: model.pll_fn(lists, folds=4),
                    'revise': lambda: model.revise_fn(lists, passes=1, fraction=0.25, sample_steps=args.steps)}
            if batch == 1:
                what['pll_k_calls'] = lambda: k_calls(lambda: model.pll_fn(lists, folds=4))
            seed(0)
            lists = limited(args.limit, draw)                                    # warm-up, untimed
            for name, fn in what.items():
                limited(args.limit, fn)
            ms, launches = {k: [] for k in what}, {}
            for i in range(args.runs):                                           # interleaved

                def one_round():
                    out = None
                    for name, fn in what.items():
                        seed(100 + i)
                        t, n, res = timed(fn)
                        ms[name].append(t)
                        launches[name] = n
                        if name == 'sample':
                            out = res
                    return out
                lists = limited(args.limit, one_round)
            if batch == 1:
                a = model.pll_fn(lists, folds=4)
                b = k_calls(lambda: model.pll_fn(lists, folds=4))
                same = a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
            emit(dict(batch=batch, steps=args.steps, runs=args.runs, folds=4,
                      critic_batched=options.pll_batched(batch, 4),
                      ms={k: [round(x, 2) for x in v] for k, v in ms.items()},
                      median_ms={k: round(statistics.median(v), 2) for k, v in ms.items()},
                      launches_last_run=launches,
                      **({'batched_equals_k_calls_as_bytes': same} if batch == 1 else {})))
    except StepTimeout:
        sys.exit(f'a step exceeded its limit of {args.limit} s; nothing more is started')
    if args.out:
        with open(args.out, 'a') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
