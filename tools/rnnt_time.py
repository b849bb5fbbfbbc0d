#!/usr/bin/env python
"""Time of the transducer loss (functional.rnnt_cost_and_grad, include/qk_rnnt.h) against `out.copy_(x)` on its logits tensor and
against the same cost composed from torch ops with autograd (layers.rnnt_cost_composed).  All in one process on the same operands.

    python tools/rnnt_time.py [--batch 256] [--steps 200] [--lmax 75] [--classes 62] [--calls 200] [--composed-batch 256]
                              [--composed-calls 10] [--model-batch 64] [--model-steps 5]

For bf16 and fp32 logits, and for lengths drawn as a length-sorted TIMIT batch has them (frames uniform in [0.8 T, T], labels
uniform in [20, Lmax], one row at the full T and Lmax) and for all lengths at full: copy, cost + gradient, cost alone (grad = NULL),
each of the three launches alone (the ablation field of the library's diagnostic mask skips the others; the lattice and the
gradient pass then read the workspace the previous full call left, the caching allocator handing the same block back), the
composition (forward + backward; at --composed-batch rows, scaled figures are NOT reported), copy again.  The difference between
the two copy figures is the run's spread.  Each figure is the mean over `calls` back-to-back calls between two HIP events, after
warm-up.  Traffic floor: the logits are read twice and the gradient is written once -- 1.5 times the copy's bytes.  Then one
training step of TimitQTransducer(TimitQLSTM(4, 1024)) at --model-batch (training_loss, backward, fused Adam).  One JSON line.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.realpath(__file__))))
from qcnn_amd import _lib, dp, functional as F, layers  # noqa: E402
from qcnn_amd.models import TimitQLSTM, TimitQTransducer  # noqa: E402


def timed(fn, calls, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    print('%s: %.4f ms per call over %d calls' % (fn.__name__, a.elapsed_time(b) / calls, calls), file=sys.stderr, flush=True)
    return a.elapsed_time(b) / calls


def lengths_of(kind, bsz, steps, lmax, dev):
    if kind == 'full':
        return torch.full((bsz,), steps, dtype=torch.int32, device=dev), torch.full((bsz,), lmax, dtype=torch.int32, device=dev)
    rng = np.random.RandomState(5)
    il, ll = rng.randint(int(0.8 * steps), steps + 1, size=bsz), rng.randint(min(20, lmax), lmax + 1, size=bsz)
    il[0], ll[0] = steps, lmax
    return torch.tensor(il, dtype=torch.int32, device=dev), torch.tensor(ll, dtype=torch.int32, device=dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--lmax', type=int, default=75)
    ap.add_argument('--classes', type=int, default=62)
    ap.add_argument('--calls', type=int, default=200)
    ap.add_argument('--composed-batch', type=int, default=256)
    ap.add_argument('--composed-calls', type=int, default=10)
    ap.add_argument('--model-batch', type=int, default=64)
    ap.add_argument('--model-steps', type=int, default=5)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    bsz, steps, lmax, v = args.batch, args.steps, args.lmax, args.classes
    gen = torch.Generator(device=dev).manual_seed(0)
    labels = torch.randint(0, v - 1, (bsz, lmax), device=dev, generator=gen, dtype=torch.int32)
    x32 = 1.5 * torch.randn((bsz, steps, lmax + 1, v), device=dev, generator=gen)
    out = dict(batch=bsz, steps=steps, lmax=lmax, classes=v, calls=args.calls,
               workspace_mb=round(_lib.lib().qk_rnnt_workspace_bytes(bsz, steps, lmax + 1, v) * 1e-6, 1), runs=[])
    for dt, name in ((torch.bfloat16, 'bf16'), (torch.float32, 'fp32')):
        x = x32.to(dt)
        buf = torch.empty_like(x)
        nbytes = 2.0 * x.numel() * x.element_size()                 # what the copy moves
        for kind in ('timit', 'full'):
            il, ll = lengths_of(kind, bsz, steps, lmax, dev)

            def copy():
                buf.copy_(x)

            def cost_and_grad():
                F.rnnt_cost_and_grad(x, labels, il, ll)

            def cost_only():
                with torch.no_grad():
                    F.rnnt_loss(x, labels, il, ll)

            def only(skip):
                def one_pass():
                    with _lib.debug_flags(0, ablate=skip):
                        F.rnnt_cost_and_grad(x, labels, il, ll)
                return one_pass

            first = timed(copy, args.calls)
            both, cost = timed(cost_and_grad, args.calls), timed(cost_only, args.calls)
            cost_and_grad()                                          # a full call: the workspace the single passes read
            rows, lattice, grad = timed(only(2 | 4), args.calls), timed(only(1 | 4), args.calls), timed(only(1 | 2), args.calls)
            comp = None
            if args.composed_calls > 0 and name == 'bf16':
                cb = min(args.composed_batch, bsz)
                xc = x[:cb].clone().requires_grad_()

                def composed():
                    layers.rnnt_cost_composed(xc, labels[:cb], il[:cb], ll[:cb]).sum().backward()
                    xc.grad = None
                comp = timed(composed, args.composed_calls, 1)
                del xc
            last = timed(copy, args.calls)
            cp = 0.5 * (first + last)
            run = dict(dtype=name, lengths=kind, active_cells=round(float(((il.double() * (ll.double() + 1)).sum()) / (bsz * steps * (lmax + 1))), 3),
                       copy_ms=dict(first=round(first, 4), last=round(last, 4), spread=round(abs(first - last), 4), gb_per_s=round(nbytes / cp * 1e-6, 1)),
                       fused_ms=dict(cost_and_grad=round(both, 4), cost_only=round(cost, 4), row_pass=round(rows, 4), lattice_pass=round(lattice, 4),
                                     gradient_pass=round(grad, 4)),
                       fused_over_copy=round(both / cp, 3), traffic_floor_over_copy=1.5,
                       fused_gb_per_s=round(1.5 * nbytes / both * 1e-6, 1))
            if comp is not None:
                run['composed_ms'] = dict(batch=cb, fwd_bwd=round(comp, 3))
                if cb == bsz:
                    run['composed_over_fused'] = round(comp / both, 1)
            out['runs'].append(run)
            torch.cuda.empty_cache()
        del x, buf
        torch.cuda.empty_cache()
    del x32
    torch.cuda.empty_cache()

    if args.model_steps > 0:
        mb, dt = args.model_batch, torch.bfloat16
        np.random.seed(0)
        torch.manual_seed(0)
        model = TimitQTransducer(TimitQLSTM(num_layers=4, units=1024, bidirectional=True, dropout=0.2), pred_units=256, joint_units=512)
        xin = torch.randn((mb, 4, 41, steps), device=dev, generator=gen).to(dt)
        il, ll = lengths_of('timit', mb, steps, lmax, dev)
        with torch.no_grad():
            model(xin[:1], il[:1])
        model.to(dev)
        model.train()
        flat = dp.FlatParams([p for p in model.parameters() if p.requires_grad])
        m, vv = torch.zeros_like(flat.param), torch.zeros_like(flat.param)
        step = torch.zeros(1, dtype=torch.int32, device=dev)

        def train_step():
            model.training_loss(xin, labels[:mb], il, ll).backward()
            F.adam_step(flat.param, flat.grad, m, vv, step, lr=1e-4, zero_grad=True)
        out['model_step'] = dict(batch=mb, encoder='TimitQLSTM(4, 1024)', pred_units=256, joint_units=512, parameters=int(flat.numel),
                                 ms=round(timed(train_step, args.model_steps, 2), 2))
    print(json.dumps(out))


if __name__ == '__main__':
    main()
