#!/usr/bin/env python
"""Time of the scheduled optimiser step (qcnn_amd.training.ScheduledAdam.step: qk_grad_guard_reduce + qk_adam_step_sched) against the
guarded step it extends (GradGuard.step: qk_grad_guard_reduce + qk_adam_step_guarded) on flat buffers of the same size, in one run.

    python tools/sched_adam_time.py [--calls 200] [--warmup 20] [--layers 10] [--filters 32]

n is the flat parameter count of TimitQCNN(layers, filters).  Every form is timed as `calls` back-to-back calls between two HIP
events after `warmup` untimed ones, in this order:

    guard_first   GradGuard.step, the step as it was before the schedule existed
    constant      ScheduledAdam.step, constant schedule, no EMA
    cosine        ScheduledAdam.step, cosine schedule with warm-up, no EMA
    ema           ScheduledAdam.step, cosine schedule, EMA 0.999
    guard_last    GradGuard.step again: |guard_last - guard_first| is the spread of this run

All forms run under the same guard settings (clipnorm, static loss scale) and with the l2 `decay` term.  Expected from the traffic:
the forms without EMA move what the guarded step moves (the reduction's 3 n floats and the update's 8 n) and stay within the spread;
the EMA form reads and writes n floats more, 2 n on top of 11 n.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.realpath(__file__))))
from qcnn_amd.models import TimitQCNN  # noqa: E402
from qcnn_amd.training import GradGuard, LRSchedule, ScheduledAdam  # noqa: E402


def timed(fn, warmup, calls):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=200)
    ap.add_argument('--warmup', type=int, default=20)
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
    p0 = torch.randn(n, device=dev, generator=gen)
    g = torch.randn(n, device=dev, generator=gen) * 1e-3
    decay = torch.full((n,), 2e-5, device=dev)
    guard_kw = dict(clipnorm=5.0, loss_scale=4096.0, dynamic=False)
    total = 4 * (args.warmup + args.calls)

    def guarded():
        p, m, v = p0.clone(), torch.zeros(n, device=dev), torch.zeros(n, device=dev)
        step, guard = torch.zeros(1, dtype=torch.int32, device=dev), GradGuard(dev, **guard_kw)
        return lambda: guard.step(p, g, m, v, step, lr=1e-4, decay=decay)

    def scheduled(schedule, ema_decay=0.0):
        opt = ScheduledAdam(p0.clone(), g, schedule, guard=GradGuard(dev, **guard_kw), ema_decay=ema_decay, decay=decay)
        return lambda: opt.step(zero_grad=False)
    forms = [('guard_first', guarded()),
             ('constant', scheduled(LRSchedule(1e-4))),
             ('cosine', scheduled(LRSchedule(1e-4, 'cosine', warmup_steps=args.warmup, total_steps=total))),
             ('ema', scheduled(LRSchedule(1e-4, 'cosine', warmup_steps=args.warmup, total_steps=total), ema_decay=0.999)),
             ('guard_last', guarded())]
    us = {name: timed(fn, args.warmup, args.calls) for name, fn in forms}
    spread = abs(us['guard_last'] - us['guard_first'])
    base = 0.5 * (us['guard_first'] + us['guard_last'])
    out = dict(n=n, calls=args.calls, warmup=args.warmup, spread_us=round(spread, 2))
    out.update({name + '_us': round(t, 2) for name, t in us.items()})
    out.update(constant_extra_us=round(us['constant'] - base, 2), cosine_extra_us=round(us['cosine'] - base, 2),
               ema_extra_us=round(us['ema'] - base, 2), ema_over_cosine=round(us['ema'] / us['cosine'], 4))
    print(json.dumps(out))


if __name__ == '__main__':
    main()
