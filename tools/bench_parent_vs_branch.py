"""The headline benchmark of a parent commit against this tree, interleaved, one process per run:

    python tools/bench_parent_vs_branch.py PARENT_TREE [--pairs 3] [--steps 2] [--warmup 1]

PARENT_TREE: a built checkout of the parent commit (its own libt2h_hip.so; e.g. `git archive` into a git-ignored
directory and `python -m text2human_amd.build` there).  Runs `python bench.py --gpus 1 --steps K --warmup W` in the parent
tree, then in this one, --pairs times; prints every run's ms_per_step, and the median and min - max of both sides.  A run
that fails or exceeds its time limit ends the script: nothing more is started on the GPU after it."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def one_run(tree, steps, warmup, limit):
    t0 = time.time()
    r = subprocess.run([sys.executable, 'bench.py', '--gpus', '1', '--steps', str(steps), '--warmup', str(warmup)], cwd=tree,
                       capture_output=True, text=True, timeout=limit)
    if r.returncode != 0:
        sys.exit(f'{tree}: bench.py exited with {r.returncode}\n{r.stderr[-2000:]}')
    line = [ln for ln in r.stdout.splitlines() if ln.startswith('{')][-1]
    return json.loads(line)['ms_per_step'], time.time() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('parent')
    ap.add_argument('--pairs', type=int, default=3)
    ap.add_argument('--steps', type=int, default=2)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--limit', type=int, default=420, help='seconds per run')
    args = ap.parse_args()
    trees = {'parent': os.path.abspath(args.parent), 'branch': ROOT}
    ms = {'parent': [], 'branch': []}
    for i in range(args.pairs):
        for side in ('parent', 'branch'):
            v, wall = one_run(trees[side], args.steps, args.warmup, args.limit)
            ms[side].append(v)
            print(f'pair {i} {side}: ms_per_step {v:.2f} (wall {wall:.0f} s)', flush=True)
    for side, v in ms.items():
        print(f'{side:7s} ' + ' '.join(f'{x:.2f}' for x in v) + f'   median {statistics.median(v):.2f}   '
              f'min - max {min(v):.2f} - {max(v):.2f}', flush=True)
    spread = max(ms['parent']) - min(ms['parent'])
    d = statistics.median(ms['branch']) - statistics.median(ms['parent'])
    print(f'branch median - parent median = {d:+.2f} ms; the parent\'s own min - max spread is {spread:.2f} ms', flush=True)


if __name__ == '__main__':
    main()
