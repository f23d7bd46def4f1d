"""Which seeds the teacher-forced parity test of confidence-ordered decoding (tests/test_gpu_confidence.py) may use:
the restatement (tests/confidence_ref.py) in float32 against ITSELF in float64, on the CPU, teacher-forced onto the
float64 trajectory and compared by the test's own rule.  A seed is usable iff the restatement alone stays under the
test's 1 % of (round, sample) pairs with an excused row and has nothing unexplained.  Writes the counts per
(seed, B, R) to profiles/confidence_parity.json.

    python tools/confidence_parity_seeds.py [--seeds 2021 7 ...] [--configs 2x8 8x16 ...]
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]

import confidence_ref as CR  # noqa: E402
from oracle import torch_ref as R  # noqa: E402
from text2human_amd import defaults, options, synthetic  # noqa: E402

ACT_TOL = 2e-4


def one(sd32, sd64, seed, B, rounds):
    batch = synthetic.parsing_batch(B, seed=seed)
    tex = R.texture_tokens(batch['texture_mask'], (32, 16))
    g = torch.Generator().manual_seed(seed)
    segm = torch.randint(0, 1024, (B, 512), generator=g)     # (the tokenizer is not under test: any valid tokens)
    torch.manual_seed(seed)
    E, U = CR.draws(B * 512, rounds, 'cpu')
    trace = []
    CR.run(segm, tex, sd64, E, U, rounds, trace=trace)
    pairs = excused = tokens = 0
    unexplained = []
    for tr in trace:
        l32 = CR.own_logits(tr['prev'], segm, tex, sd32, 1.0)
        tok, _, s = CR.draw_and_score(l32, E[tr['r'] - 1], U[tr['r'] - 1], CR.tau_of(tr['r'], rounds, 4.5))
        x32, _, _ = CR.commit(tr['prev'], tr['out'], tok, s, tex, tr['k'])
        c = CR.compare_round(tr, E[tr['r'] - 1], tok, x32, l32, ACT_TOL)
        pairs += B
        excused += len(c['excused_samples'])
        tokens += c['token_mismatches']
        unexplained += c['unexplained_tokens'] + c['unexcused_rows']
    return dict(seed=seed, B=B, rounds=rounds, pairs=pairs, pairs_with_excused_row=excused, token_mismatches=tokens,
                unexplained=len(unexplained), usable=bool(excused <= 0.01 * pairs and not unexplained))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--seeds', type=int, nargs='+', default=[2021, 7])
    ap.add_argument('--configs', nargs='+', default=['2x8', '2x16', '8x8', '8x16'])
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'confidence_parity.json'))
    args = ap.parse_args()
    opt = options.dict_to_nonedict(defaults.sample_from_parsing())
    sd32 = synthetic.make_state_dicts(opt, seed=1234)['sampler']
    sd64 = {k: (v.double() if v.is_floating_point() else v) for k, v in sd32.items()}
    rows = []
    for cfg in args.configs:
        B, rounds = (int(x) for x in cfg.split('x'))
        for seed in args.seeds:
            t0 = time.time()
            rows.append(one(sd32, sd64, seed, B, rounds))
            print(json.dumps(rows[-1]), f'{time.time() - t0:.0f} s', flush=True)
            with open(args.out, 'w') as f:
                json.dump(dict(what='float32 restatement vs float64 restatement, CPU, teacher-forced; rule of '
                                    'tests/confidence_ref.py compare_round, ACT_TOL 2e-4', weights='synthetic seed 1234',
                               runs=rows), f, indent=1)


if __name__ == '__main__':
    main()
