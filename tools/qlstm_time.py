#!/usr/bin/env python
"""Time of the fused quaternion LSTM recurrence (functional.qlstm: one launch per time step, include/qk_rnn.h) against a baseline
composed from what the library had before it: per step and direction one qk_dense_fwd on h (functional.quaternion_dense) plus
torch element-wise ops for the cell, and autograd for the backward.  Both run in one process on the same operands.

    python tools/qlstm_time.py [--batch 256] [--steps 200] [--units 1024] [--calls 200] [--baseline-calls 200] [--model-steps 10]

Order: baseline, fused forward, fused forward + backward, baseline again.  The difference between the two baseline figures is the
run's spread.  Each figure is the mean over `calls` back-to-back calls between two HIP events, after warm-up.  Reported: ms per
call, the achieved TFLOP/s of the recurrent products (2 B U 4U flops per step and direction, forward; the same again for dz R^T in
the backward -- the weight gradient is the dense backward-weight kernel's and is not counted) and the time per launch (ms / T).
Then one training step of TimitQLSTM(4, units) at the same batch (ctc_mean_loss, backward, fused Adam): mean of --model-steps.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.realpath(__file__))))
from qcnn_amd import dp, functional as F  # noqa: E402
from qcnn_amd.models import TimitQLSTM  # noqa: E402


def composed(zx, R):
    """The same recurrence from dense calls and torch ops: zx (D, B, T, 4U) bf16, R (D, Q, 4U) fp32, zero state, full lengths."""
    dirs, bsz, steps, g = zx.shape
    u = g // 4
    q = u // 4
    outs = []
    for d in range(dirs):
        h = torch.zeros((bsz, u), dtype=zx.dtype, device=zx.device)
        c = torch.zeros((bsz, 4, q), dtype=torch.float32, device=zx.device)
        ys = [None] * steps
        for t in (range(steps - 1, -1, -1) if d == 1 else range(steps)):
            z = (zx[d, :, t] + F.quaternion_dense(h, R[d])).view(bsz, 4, 4, q).float()
            c = torch.sigmoid(z[:, :, 1]) * c + torch.sigmoid(z[:, :, 0]) * torch.tanh(z[:, :, 2])
            h = (torch.sigmoid(z[:, :, 3]) * torch.tanh(c)).to(zx.dtype).reshape(bsz, u)
            ys[t] = h
        outs.append(torch.stack(ys, dim=1).view(bsz, steps, 4, q))
    return torch.stack(outs, dim=3).reshape(bsz, steps, dirs * u)


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
    print('%s: %.3f ms per call over %d calls' % (fn.__name__, a.elapsed_time(b) / calls, calls), file=sys.stderr, flush=True)
    return a.elapsed_time(b) / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--units', type=int, default=1024)
    ap.add_argument('--calls', type=int, default=200)
    ap.add_argument('--baseline-calls', type=int, default=200)
    ap.add_argument('--model-steps', type=int, default=10)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    bsz, steps, u, dirs, dt = args.batch, args.steps, args.units, 2, torch.bfloat16
    q = u // 4
    gen = torch.Generator(device=dev).manual_seed(0)
    zx = torch.randn((dirs, bsz, steps, 4 * u), device=dev, generator=gen).to(dt).requires_grad_()
    R = (torch.randn((dirs, q, 4 * u), device=dev, generator=gen) * (0.6 / q ** 0.5)).requires_grad_()
    dy = torch.randn((bsz, steps, dirs * u), device=dev, generator=gen).to(dt)

    def fused_fwd():
        with torch.no_grad():
            F.qlstm(zx, R)

    def fused_both():
        y, _, _ = F.qlstm(zx, R)
        y.backward(dy)
        zx.grad = R.grad = None

    def base_fwd():
        with torch.no_grad():
            composed(zx, R)

    def base_both():
        composed(zx, R).backward(dy)
        zx.grad = R.grad = None

    out = dict(batch=bsz, steps=steps, units=u, directions=dirs, dtype='bf16', path=F.qlstm_path(dt, bsz, steps, q, dirs), calls=args.calls,
               baseline_calls=args.baseline_calls)
    with torch.no_grad():                                            # the two forms compute the same thing
        ya, yb = F.qlstm(zx, R)[0].float(), composed(zx, R).float()
        out['max_abs_difference_of_y'] = float((ya - yb).abs().max())
        del ya, yb
    first = dict(fwd=timed(base_fwd, args.baseline_calls, 1), both=timed(base_both, args.baseline_calls, 1))
    fused = dict(fwd=timed(fused_fwd, args.calls), both=timed(fused_both, args.calls))
    last = dict(fwd=timed(base_fwd, args.baseline_calls, 1), both=timed(base_both, args.baseline_calls, 1))
    flops = 2.0 * bsz * u * 4 * u * steps * dirs
    out['fused_ms'] = dict(fwd=round(fused['fwd'], 3), fwd_bwd=round(fused['both'], 3), bwd=round(fused['both'] - fused['fwd'], 3))
    out['composed_ms'] = dict(fwd_first=round(first['fwd'], 3), fwd_last=round(last['fwd'], 3), fwd_bwd_first=round(first['both'], 3),
                              fwd_bwd_last=round(last['both'], 3))
    out['spread_ms'] = dict(fwd=round(abs(first['fwd'] - last['fwd']), 3), fwd_bwd=round(abs(first['both'] - last['both']), 3))
    out['recurrent_tflops'] = dict(fwd=round(flops / fused['fwd'] * 1e-9, 2), bwd=round(flops / (fused['both'] - fused['fwd']) * 1e-9, 2))
    out['us_per_launch'] = dict(fwd=round(1e3 * fused['fwd'] / steps, 2), bwd=round(1e3 * (fused['both'] - fused['fwd']) / (steps + 1), 2))
    del zx, R, dy
    torch.cuda.empty_cache()

    if args.model_steps > 0:
        np.random.seed(0)
        torch.manual_seed(0)
        model = TimitQLSTM(num_layers=4, units=u, bidirectional=True, dropout=0.2)
        x = torch.randn((bsz, 4, 41, steps), device=dev, generator=gen).to(dt)
        il = torch.full((bsz, 1), steps, dtype=torch.int32, device=dev)
        labels = torch.randint(0, 61, (bsz, 40), device=dev, generator=gen, dtype=torch.int32)
        ll = torch.full((bsz, 1), 40, dtype=torch.int32, device=dev)
        with torch.no_grad():
            model(x[:1], il[:1])
        model.to(dev)
        model.train()
        flat = dp.FlatParams([p for p in model.parameters() if p.requires_grad])
        m, v = torch.zeros_like(flat.param), torch.zeros_like(flat.param)
        step = torch.zeros(1, dtype=torch.int32, device=dev)

        def train_step():
            model.ctc_mean_loss(x, labels, il, ll).backward()
            F.adam_step(flat.param, flat.grad, m, v, step, lr=1e-4, zero_grad=True)
        out['model_step_ms'] = round(timed(train_step, args.model_steps, 2), 2)
        out['model_parameters'] = int(flat.param.numel())
    print(json.dumps(out))


if __name__ == '__main__':
    main()
