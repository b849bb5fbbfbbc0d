#!/usr/bin/env python
"""Time of the guarded optimiser step (qcnn_amd.training.GradGuard.step: qk_grad_guard_reduce + qk_adam_step_guarded) against the
plain fused Adam (functional.adam_step(step=<device tensor>)) on the same flat buffers, in one process, the two alternating.

    python tools/grad_guard_time.py [--rounds 15] [--iters 50] [--layers 10] [--filters 32]

n is the parameter count of TimitQCNN(layers, filters).  Each round times `iters` back-to-back calls of one form between two
events, then the same for the other; the medians over the rounds are reported, with and without the l2 `decay` term.  The guard
reads n floats more than the plain step (3 n with decay, which also re-reads param and decay) on top of the plain step's 7-8 n,
and adds two launches (the reduce's two stages; both forms bump the device counter); the extra time is expected to stay below the
plain step's own.  The guard here clips (clipnorm=5) under a static scale, so both forms do the same arithmetic every iteration.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.realpath(__file__))))
from qcnn_amd import functional as F  # noqa: E402
from qcnn_amd.models import TimitQCNN  # noqa: E402
from qcnn_amd.training import GradGuard  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=15)
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--layers', type=int, default=10)
    ap.add_argument('--filters', type=int, default=32)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    np.random.seed(0)
    model = TimitQCNN(num_layers=args.layers, start_filter=args.filters)
    with torch.no_grad():
        model(torch.randn(1, 4, 41, 40, device=dev))
    n = sum(p.numel() for p in model.parameters() if p.requires_grad)
    del model
    gen = torch.Generator(device=dev).manual_seed(0)
    p = torch.randn(n, device=dev, generator=gen)
    g = torch.randn(n, device=dev, generator=gen) * 1e-3
    m, v = torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    decay = torch.full((n,), 2e-5, device=dev)
    step = torch.zeros(1, dtype=torch.int32, device=dev)
    guard = GradGuard(dev, clipnorm=5.0, loss_scale=4096.0, dynamic=False)
    out = dict(n=n, rounds=args.rounds, iters=args.iters)
    for name, dec in (('plain', None), ('decay', decay)):
        forms = dict(adam=lambda: F.adam_step(p, g, m, v, step, lr=1e-4, grad_scale=1.0 / 4096.0, decay=dec),
                     guarded=lambda: guard.step(p, g, m, v, step, lr=1e-4, decay=dec))
        times = dict(adam=[], guarded=[])
        for fn in forms.values():
            for _ in range(10):
                fn()
        torch.cuda.synchronize()
        for _ in range(args.rounds):
            for key, fn in forms.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(args.iters):
                    fn()
                b.record()
                b.synchronize()
                times[key].append(a.elapsed_time(b) * 1e3 / args.iters)
        us = {k: statistics.median(t) for k, t in times.items()}
        out[name] = dict(adam_us=round(us['adam'], 2), guarded_us=round(us['guarded'], 2), extra_us=round(us['guarded'] - us['adam'], 2),
                         adam_min_us=round(min(times['adam']), 2), guarded_min_us=round(min(times['guarded']), 2))
    assert guard.stats()['skipped_steps'] == 0
    print(json.dumps(out))


if __name__ == '__main__':
    main()
