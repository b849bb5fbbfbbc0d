#!/usr/bin/env python
"""Times the CTC forced alignment (functional.ctc_forced_align) at the benchmark shape (B = 256, T = 200, C = 62, Lmax = 75, bf16
posteriors) with HIP events after warm-up, and functional.ctc_cost_and_grad on the same tensors in the same run; prints one JSON line
per measurement.  The alignment is one max-plus sweep of the lattice the cost with its gradient sweeps twice with log-sum-exp.

    python tools/ctc_align_time.py [--reps 50]

The posteriors are peaky synthetic ones (softmax of scaled random logits, blank-heavy), like a trained model's output; label lengths
are 40 .. 75, every sample uses all 200 frames.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.realpath(__file__)))
sys.path.insert(0, ROOT)
import qcnn_amd  # noqa: E402,F401
from qcnn_amd import functional as F  # noqa: E402


def timed(fn, reps, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    times = []
    for _ in range(reps):
        ev[0].record()
        fn()
        ev[1].record()
        ev[1].synchronize()
        times.append(ev[0].elapsed_time(ev[1]))
    return float(np.median(times)), float(np.min(times))


def report(name, med_min, **kw):
    print(json.dumps(dict(name=name, median_ms=round(med_min[0], 4), min_ms=round(med_min[1], 4), **kw)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=50)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    B, T, C, Lmax = 256, 200, 62, 75
    rng = np.random.RandomState(0)
    z = rng.randn(B, T, C) * 3.0
    z[..., -1] += 3.0
    y = torch.softmax(torch.tensor(z, dtype=torch.float32), dim=-1).to(dev, torch.bfloat16)
    il = torch.full((B,), T, dtype=torch.int32, device=dev)
    labels = torch.tensor(rng.randint(0, C - 1, size=(B, Lmax)), dtype=torch.int32, device=dev)
    ll = torch.tensor(rng.randint(40, Lmax + 1, size=B), dtype=torch.int32, device=dev)
    shape = dict(B=B, T=T, C=C, Lmax=Lmax, dtype='bf16')
    align = timed(lambda: F.ctc_forced_align(y, labels, il, ll), args.reps)
    cost = timed(lambda: F.ctc_cost_and_grad(y, labels, il, ll), args.reps)
    report('ctc_forced_align', align, **shape)
    report('ctc_cost_and_grad', cost, **shape)
    report('ctc_forced_align_again', timed(lambda: F.ctc_forced_align(y, labels, il, ll), args.reps), ratio_to_cost_and_grad=round(align[0] / cost[0], 3),
           **shape)


if __name__ == '__main__':
    main()
