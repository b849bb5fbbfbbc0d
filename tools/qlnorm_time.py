#!/usr/bin/env python
"""Time of the fused quaternion layer normalisation (functional.qlayer_norm, include/qk_norm.h) against `out.copy_(x)` on the same
tensors and against the same formula composed from torch ops with autograd.  All in one process on the same operands.

    python tools/qlnorm_time.py [--batch 256] [--steps 200] [--q 512] [--calls 200] [--model-steps 10]

Order: copy, fused forward, fused forward + backward (once with and once without the weight gradients), composed forward, composed
forward + backward, copy again.  The difference between the two copy figures is the run's spread.  Each figure is the mean over
`calls` back-to-back calls between two HIP events, after warm-up.  Traffic: the forward reads x and writes y -- exactly the copy's
bytes; the backward reads x and dy and writes dx -- 1.5 times those (+ the slab partials, 5 Q floats per slab).  Reported: ms per
call, the ratio to the copy and the achieved GB/s of that traffic.  Then one training step of TimitQLSTM(4, 1024) at the same batch
(ctc_mean_loss, backward, fused Adam) without and with layer_norm: mean of --model-steps.
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


def composed(x, gamma, beta, epsilon=1e-3):
    """The same formula from torch ops: x (B, T, 4Q) bf16, fp32 arithmetic, one rounding of y."""
    b, t, w = x.shape
    x4 = x.float().view(b, t, 4, w // 4)
    d = x4 - x4.mean(dim=3, keepdim=True)
    var = (d * d).mean(dim=(2, 3), keepdim=True)
    y = d * torch.rsqrt(var + epsilon) * gamma.view(1, 1, 1, -1) + beta.view(1, 1, 4, -1)
    return y.to(x.dtype).view(b, t, w)


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--q', type=int, default=512, help='quaternion units per row (two directions of 1024 units: 512)')
    ap.add_argument('--calls', type=int, default=200)
    ap.add_argument('--model-steps', type=int, default=10)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    bsz, steps, q, dt = args.batch, args.steps, args.q, torch.bfloat16
    w = 4 * q
    gen = torch.Generator(device=dev).manual_seed(0)
    x = (1.5 * torch.randn((bsz, steps, w), device=dev, generator=gen) + 0.5).to(dt).requires_grad_()
    gamma = (1 + 0.3 * torch.randn(q, device=dev, generator=gen)).requires_grad_()
    beta = (0.3 * torch.randn(w, device=dev, generator=gen)).requires_grad_()
    dy = torch.randn((bsz, steps, w), device=dev, generator=gen).to(dt)
    out_buf = torch.empty_like(x)
    xd, gd, bd = x.detach(), gamma.detach(), beta.detach()

    def copy():
        out_buf.copy_(xd)

    def fused_fwd():
        with torch.no_grad():
            F.qlayer_norm(x, gamma, beta)

    def fused_both():
        F.qlayer_norm(x, gamma, beta).backward(dy)
        x.grad = gamma.grad = beta.grad = None

    def fused_both_dx_only():
        F.qlayer_norm(x, gd, bd).backward(dy)
        x.grad = None

    def composed_fwd():
        with torch.no_grad():
            composed(x, gamma, beta)

    def composed_both():
        composed(x, gamma, beta).backward(dy)
        x.grad = gamma.grad = beta.grad = None

    out = dict(batch=bsz, steps=steps, q=q, dtype='bf16', path=F.qlayer_norm_path(dt, bsz * steps, q), calls=args.calls)
    with torch.no_grad():                                            # the two forms compute the same thing
        out['max_abs_difference_of_y'] = float((F.qlayer_norm(x, gamma, beta).float() - composed(x, gamma, beta).float()).abs().max())
    first = timed(copy, args.calls)
    fused = dict(fwd=timed(fused_fwd, args.calls), both=timed(fused_both, args.calls), both_dx=timed(fused_both_dx_only, args.calls))
    comp = dict(fwd=timed(composed_fwd, args.calls), both=timed(composed_both, args.calls))
    last = timed(copy, args.calls)
    cp = 0.5 * (first + last)
    nbytes = 2.0 * x.numel() * x.element_size()
    bwd, bwd_dx = fused['both'] - fused['fwd'], fused['both_dx'] - fused['fwd']
    out['copy_ms'] = dict(first=round(first, 4), last=round(last, 4), spread=round(abs(first - last), 4), gb_per_s=round(nbytes / cp * 1e-6, 1))
    out['fused_ms'] = dict(fwd=round(fused['fwd'], 4), fwd_bwd=round(fused['both'], 4), bwd=round(bwd, 4), bwd_without_weight_gradients=round(bwd_dx, 4))
    out['fused_over_copy'] = dict(fwd=round(fused['fwd'] / cp, 3), bwd=round(bwd / cp, 3), bwd_without_weight_gradients=round(bwd_dx / cp, 3),
                                  traffic=dict(fwd=1.0, bwd=1.5))
    out['fused_gb_per_s'] = dict(fwd=round(nbytes / fused['fwd'] * 1e-6, 1), bwd=round(1.5 * nbytes / bwd * 1e-6, 1))
    out['composed_ms'] = dict(fwd=round(comp['fwd'], 4), fwd_bwd=round(comp['both'], 4))
    out['composed_over_fused'] = dict(fwd=round(comp['fwd'] / fused['fwd'], 2), fwd_bwd=round(comp['both'] / fused['both'], 2))
    del x, dy, out_buf, xd
    torch.cuda.empty_cache()

    if args.model_steps > 0:
        out['model_step_ms'] = {}
        for name, layer_norm in (('plain', False), ('layer_norm', True), ('plain_again', False)):
            np.random.seed(0)
            torch.manual_seed(0)
            model = TimitQLSTM(num_layers=4, units=1024, bidirectional=True, dropout=0.2, layer_norm=layer_norm)
            xin = torch.randn((bsz, 4, 41, steps), device=dev, generator=gen).to(dt)
            il = torch.full((bsz, 1), steps, dtype=torch.int32, device=dev)
            labels = torch.randint(0, 61, (bsz, 40), device=dev, generator=gen, dtype=torch.int32)
            ll = torch.full((bsz, 1), 40, dtype=torch.int32, device=dev)
            with torch.no_grad():
                model(xin[:1], il[:1])
            model.to(dev)
            model.train()
            flat = dp.FlatParams([p for p in model.parameters() if p.requires_grad])
            m, v = torch.zeros_like(flat.param), torch.zeros_like(flat.param)
            step = torch.zeros(1, dtype=torch.int32, device=dev)

            def train_step():
                model.ctc_mean_loss(xin, labels, il, ll).backward()
                F.adam_step(flat.param, flat.grad, m, v, step, lr=1e-4, zero_grad=True)
            out['model_step_ms'][name] = round(timed(train_step, args.model_steps, 2), 2)
            del model, flat, m, v
            torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == '__main__':
    main()
