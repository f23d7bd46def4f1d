"""Region editing cost: sample_fn against resample_fn with 1/8, 1/4 and 1/2 of every sample's token rows resampled
(k random rows per sample), B = 8, 256 steps, synthetic checkpoint.  Reports HIP-event ms per call, the rounds the
transformer ran (net.last_stats) and the predicted rounds: a token's unmasking step is uniform over 1..steps, so k
resampled rows of a sample take steps * (1 - (1 - 1/steps)^k) distinct steps on average (the batch runs as many rounds
as its slowest sample).  GPU only.

    python tools/edit_bench.py [batch=8] [steps=256]
"""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from text2human_amd import defaults, options, synthetic  # noqa: E402
from text2human_amd.models import SampleFromParsingModel  # noqa: E402

B = int(sys.argv[1]) if len(sys.argv) > 1 else 8
STEPS = int(sys.argv[2]) if len(sys.argv) > 2 else 256
T = 512
opt = options.dict_to_nonedict(defaults.sample_from_parsing())
model = SampleFromParsingModel(opt, state_dicts=synthetic.make_state_dicts(opt, seed=1234))
model.feed_data(synthetic.parsing_batch(B, seed=2021))
net = model.sampler_fn


def timed(fn, iters=5, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for i in range(iters):
        torch.manual_seed(100 + i)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    ms.sort()
    return ms[len(ms) // 2], dict(net.last_stats)


def predicted(k):
    return STEPS * (1 - (1 - 1 / STEPS)**k)


torch.manual_seed(1)
src = model.sample_fn(temp=1, sample_steps=STEPS)
full_ms, full_st = timed(lambda: model.sample_fn(temp=1, sample_steps=STEPS))
rows = [dict(case='sample_fn', resampled_per_sample=T, ms=round(full_ms, 2), rounds=full_st['rounds'],
             predicted_rounds=round(predicted(T), 1), ratio_ms=1.0, ratio_rounds=1.0)]
g = torch.Generator().manual_seed(7)
for frac in (8, 4, 2):
    k = T // frac
    keep = torch.ones(B, T, dtype=torch.uint8)
    for b in range(B):
        keep[b, torch.randperm(T, generator=g)[:k]] = 0
    keep = keep.to(model.device)
    ms, st = timed(lambda: model.resample_fn(src, keep, sample_steps=STEPS))
    rows.append(dict(case=f'resample_fn 1/{frac}', resampled_per_sample=k, ms=round(ms, 2), rounds=st['rounds'],
                     predicted_rounds=round(predicted(k), 1), ratio_ms=round(ms / full_ms, 3),
                     ratio_rounds=round(st['rounds'] / full_st['rounds'], 3),
                     predicted_ratio=round(predicted(k) / predicted(T), 3)))
print(f'# edit_bench: B={B} steps={STEPS} device={torch.cuda.get_device_name()} launch={net.last_launch_mode}')
for r in rows:
    print(json.dumps(r))
