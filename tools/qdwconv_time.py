#!/usr/bin/env python
"""Time of the fused GLU + depthwise quaternion convolution (functional.qglu_dwconv1d, include/qk_dwconv.h) against the only other
way to get its semantics: the split GLU, torch's conv1d(groups=Q) on a permuted copy with the 4 x 4 real block of every tap
expanded, and autograd's backward.

    python tools/qdwconv_time.py [--batch 256] [--steps 200] [--calls 200] [--model-steps 10] [--timeout 240]

Every configuration (units 256 and 512, K 15 and 31, bf16) and the model comparison run as a child process of their own under
their own time limit; the first child that fails or runs out of time ends the run.  Inside a child, in this order: out.copy_(x)
moving the same total bytes as the fused forward (it reads 8 Q and writes 4 Q values per row), the fused forward and forward +
backward, the torch composition forward and forward + backward, the copy again.  The difference between the two copy figures is
the run's spread.  Each figure is the mean over `calls` back-to-back calls between two HIP events, after warm-up.  Everything
runs twice: with lengths drawn as a TIMIT batch padded to `steps` frames has them (normal around 0.6 T with a deviation of 0.17 T,
cut to [0.25 T, T], the longest row at T) and with all lengths equal to T.  Two floors are printed beside the fused forward: its
bytes at the copy's measured rate, and its arithmetic (16 multiply-adds per quaternion and tap, all T frames) at the 157 TFLOP/s
fp32 vector peak.  The model child times one training step (ctc_mean_loss, backward, fused Adam) of TimitQConformer() beside
TimitQTransformer(6, 256, 4, 1024) at the same batch.  One JSON line per child.
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.realpath(__file__))))
from qcnn_amd import dp, functional as F  # noqa: E402
from qcnn_amd.models import TimitQConformer, TimitQTransformer  # noqa: E402

FP32_VECTOR_PEAK = 157e12


def expand_taps(kernel):
    """(K, 4Q) quaternion taps -> the (4Q, 4, K) weight of conv1d(groups=Q), channel u * 4 + c: the real block of W (x) h."""
    k, w = kernel.shape
    r, i, j, q = (kernel[:, c * (w // 4):(c + 1) * (w // 4)].transpose(0, 1) for c in range(4))            # (Q, K) each
    rows = [torch.stack(row, dim=1) for row in ((r, -i, -j, -q), (i, r, -q, j), (j, q, r, -i), (q, -j, i, r))]      # (Q, 4, K) per output component
    return torch.stack(rows, dim=1).reshape(w, 4, k)


def composed(u, kernel, bias, lengths, pad_lo):
    """The semantics of qglu_dwconv1d from torch ops."""
    b, t, w = u.shape
    q = w // 8
    x = u.view(b, t, 4, 2, q)
    act = (torch.arange(t, device=u.device)[None, :] < lengths[:, None])[:, :, None, None]
    h = (x[:, :, :, 0] * torch.sigmoid(x[:, :, :, 1])) * act.to(u.dtype)
    hc = torch.nn.functional.pad(h.permute(0, 3, 2, 1).reshape(b, 4 * q, t), (pad_lo, kernel.shape[0] - 1 - pad_lo))
    y = torch.nn.functional.conv1d(hc, expand_taps(kernel).to(u.dtype), bias.view(4, q).transpose(0, 1).reshape(-1).to(u.dtype), groups=q)
    return y.view(b, q, 4, t).permute(0, 3, 2, 1).reshape(b, t, 4 * q) * act.view(b, t, 1).to(u.dtype)


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


def timit_lengths(bsz, steps, rng):
    n = np.clip(np.rint(steps * (0.6 + 0.17 * rng.randn(bsz))), steps // 4, steps).astype(np.int32)
    n[0] = steps
    return n


def kernel_child(args):
    dev = torch.device('cuda:0')
    bsz, steps, dt, taps = args.batch, args.steps, torch.bfloat16, args.taps
    Q = args.units // 4
    pad_lo = F.qdwconv_pad_lo(taps, 'same')
    gen = torch.Generator(device=dev).manual_seed(0)
    u = torch.randn((bsz, steps, 8 * Q), device=dev, generator=gen).to(dt).requires_grad_()
    dy = torch.randn((bsz, steps, 4 * Q), device=dev, generator=gen).to(dt)
    kernel = (torch.randn((taps, 4 * Q), device=dev, generator=gen) / np.sqrt(taps)).requires_grad_()
    bias = (0.1 * torch.randn((4 * Q,), device=dev, generator=gen)).requires_grad_()
    src, dst = torch.randn((bsz, steps, 6 * Q), device=dev, generator=gen).to(dt), torch.empty((bsz, steps, 6 * Q), dtype=dt, device=dev)
    nbytes = bsz * steps * 12 * Q * 2
    gflop = 2e-9 * 16 * taps * bsz * steps * Q
    out = dict(units=args.units, taps=taps, batch=bsz, steps=steps, dtype='bf16', path=F.qdwconv_path(dt, bsz, steps, Q, taps, packed=True),
               calls=args.calls, fwd_megabytes=round(nbytes / 1e6, 1), fwd_gflop=round(gflop, 2),
               arithmetic_floor_ms=round(gflop * 1e9 / FP32_VECTOR_PEAK * 1e3, 4))
    rng = np.random.RandomState(0)
    for case, n in (('timit_lengths', timit_lengths(bsz, steps, rng)), ('full_lengths', np.full(bsz, steps, dtype=np.int32))):
        lengths = torch.tensor(n, device=dev)

        def copy():
            dst.copy_(src)

        def fused_fwd():
            with torch.no_grad():
                F.qglu_dwconv1d(u, kernel, bias, lengths)

        def fused_both():
            F.qglu_dwconv1d(u, kernel, bias, lengths).backward(dy)
            u.grad = kernel.grad = bias.grad = None

        def composed_fwd():
            with torch.no_grad():
                composed(u, kernel, bias, lengths, pad_lo)

        def composed_both():
            composed(u, kernel, bias, lengths, pad_lo).backward(dy)
            u.grad = kernel.grad = bias.grad = None

        res = dict(mean_length=round(float(n.mean()), 1))
        with torch.no_grad():                                            # the two forms compute the same thing
            res['max_abs_difference_of_y'] = float((F.qglu_dwconv1d(u, kernel, bias, lengths).float() - composed(u, kernel, bias, lengths, pad_lo).float()).abs().max())
        first = timed(copy, args.calls)
        fused = dict(fwd=timed(fused_fwd, args.calls), both=timed(fused_both, args.calls))
        comp = dict(fwd=timed(composed_fwd, args.calls), both=timed(composed_both, args.calls))
        last = timed(copy, args.calls)
        rate = nbytes / (0.5 * (first + last) * 1e-3)
        res['copy_ms'] = dict(first=round(first, 4), last=round(last, 4), spread=round(abs(first - last), 4), terabytes_per_s=round(rate / 1e12, 3))
        res['fused_ms'] = dict(fwd=round(fused['fwd'], 4), fwd_bwd=round(fused['both'], 4), bwd=round(fused['both'] - fused['fwd'], 4))
        res['composed_ms'] = dict(fwd=round(comp['fwd'], 4), fwd_bwd=round(comp['both'], 4))
        res['composed_over_fused'] = dict(fwd=round(comp['fwd'] / fused['fwd'], 2), fwd_bwd=round(comp['both'] / fused['both'], 2))
        res['fused_fwd_over_traffic_floor'] = round(fused['fwd'] / (0.5 * (first + last)), 2)
        res['fused_fwd_over_arithmetic_floor'] = round(fused['fwd'] / out['arithmetic_floor_ms'], 2)
        out[case] = res
    print(json.dumps(out), flush=True)


def model_child(args):
    dev = torch.device('cuda:0')
    bsz, steps, dt = args.batch, args.steps, torch.bfloat16
    gen = torch.Generator(device=dev).manual_seed(0)
    xin = torch.randn((bsz, 4, 41, steps), device=dev, generator=gen).to(dt)
    il = torch.tensor(timit_lengths(bsz, steps, np.random.RandomState(0)), device=dev).view(bsz, 1)
    labels = torch.randint(0, 61, (bsz, 20), device=dev, generator=gen, dtype=torch.int32)
    ll = torch.full((bsz, 1), 20, dtype=torch.int32, device=dev)
    out = dict(batch=bsz, steps=steps, dtype='bf16', model_steps=args.model_steps)
    for name, make in (('TimitQConformer()', lambda: TimitQConformer()), ('TimitQTransformer(6, 256, 4, 1024)', lambda: TimitQTransformer(6, 256, 4, 1024))):
        np.random.seed(0)
        torch.manual_seed(0)
        model = make()
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
        out[name] = dict(step_ms=round(timed(train_step, args.model_steps, 2), 2), parameters=int(flat.param.numel()))
        del model, flat, m, v
        torch.cuda.empty_cache()
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--calls', type=int, default=200)
    ap.add_argument('--model-steps', type=int, default=10)
    ap.add_argument('--timeout', type=int, default=240, help='seconds for each child process')
    ap.add_argument('--child', choices=['kernel', 'model'])
    ap.add_argument('--units', type=int, default=512)
    ap.add_argument('--taps', type=int, default=15)
    args = ap.parse_args()
    if args.child == 'kernel':
        return kernel_child(args)
    if args.child == 'model':
        return model_child(args)
    common = [sys.executable, os.path.realpath(__file__), '--batch', str(args.batch), '--steps', str(args.steps), '--calls', str(args.calls),
              '--model-steps', str(args.model_steps)]
    jobs = [['--child', 'kernel', '--units', str(units), '--taps', str(taps)] for units in (256, 512) for taps in (15, 31)]
    if args.model_steps > 0:
        jobs.append(['--child', 'model'])
    for job in jobs:
        try:
            rc = subprocess.run(common + job, timeout=args.timeout).returncode
        except subprocess.TimeoutExpired:
            rc = 124
        if rc != 0:
            print('qdwconv_time: %s ended with status %d; nothing more is started' % (' '.join(job), rc), file=sys.stderr)
            return rc
    return 0


if __name__ == '__main__':
    sys.exit(main())
