#!/usr/bin/env python
"""Time of the fused quaternion self-attention (functional.qattention_packed, include/qk_attn.h) against torch's
scaled_dot_product_attention on pre-permuted contiguous (B, H, T, D) tensors with a boolean key mask, and against the same formula
composed from torch ops with autograd on the project's own layout.  All in one process on the same operands.

    python tools/qattn_time.py [--batch 256] [--steps 200] [--heads 8] [--dq 16] [--calls 200] [--model-steps 10]

Order: sdpa forward and forward + backward, fused forward and forward + backward, composed forward and forward + backward, sdpa again.
The difference between the two sdpa figures is the run's spread.  Each figure is the mean over `calls` back-to-back calls between two
HIP events, after warm-up.  Everything runs twice: with lengths drawn as a TIMIT batch padded to `steps` frames has them (normal
around 0.6 T with a deviation of 0.17 T, cut to [0.25 T, T], the longest row at T) and with all lengths equal to T.  sdpa is given
less to do than the fused call: its inputs are already permuted to heads, it produces no zeros at inactive rows and its gradients are
three separate (B, H, T, D) tensors.  Arithmetic: 4 B H T^2 D FLOP forward and 3.5 times that backward in the two-kernel form (seven
products against the forward's two), counted over all T^2 pairs; the FLOP/s figures use the pairs below lengths only.  Then one
training step of TimitQTransformer(6, 512, 8) at the same batch (ctc_mean_loss, backward, fused Adam): mean of --model-steps.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.realpath(__file__))))
from qcnn_amd import dp, functional as F  # noqa: E402
from qcnn_amd.models import TimitQTransformer  # noqa: E402


def to_heads(x, heads):
    """(B, T, 4Q) component-major -> (B, H, T, 4 dq) contiguous."""
    b, t, w = x.shape
    dq = w // 4 // heads
    return x.view(b, t, 4, heads, dq).permute(0, 3, 1, 2, 4).reshape(b, heads, t, 4 * dq)


def composed(qkv, heads, lengths):
    """The semantics of qattention_packed from torch ops: bf16 matmuls, fp32 softmax, zeros at inactive rows."""
    b, t, w = qkv.shape
    x = qkv.view(b, t, 4, 3, w // 12)
    q, k, v = (to_heads(x[:, :, :, g].reshape(b, t, w // 3), heads) for g in range(3))
    act = torch.arange(t, device=qkv.device)[None, :] < lengths[:, None]
    s = (q @ k.transpose(-1, -2)).float() * (1.0 / float(np.sqrt(q.shape[-1])))
    p = torch.softmax(s.masked_fill(~act[:, None, None, :], float('-inf')), dim=-1).to(qkv.dtype)
    o = (p @ v).view(b, heads, t, 4, -1).permute(0, 2, 3, 1, 4).reshape(b, t, w // 3)
    return o * act[:, :, None].to(o.dtype)


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--heads', type=int, default=8)
    ap.add_argument('--dq', type=int, default=16)
    ap.add_argument('--calls', type=int, default=200)
    ap.add_argument('--model-steps', type=int, default=10)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    bsz, steps, heads, dq, dt = args.batch, args.steps, args.heads, args.dq, torch.bfloat16
    Q = heads * dq
    gen = torch.Generator(device=dev).manual_seed(0)
    qkv = torch.randn((bsz, steps, 12 * Q), device=dev, generator=gen).to(dt).requires_grad_()
    do = torch.randn((bsz, steps, 4 * Q), device=dev, generator=gen).to(dt)
    x = qkv.detach().view(bsz, steps, 4, 3, Q)
    qh, kh, vh = (to_heads(x[:, :, :, g].reshape(bsz, steps, 4 * Q), heads).contiguous().requires_grad_() for g in range(3))
    doh = to_heads(do, heads).contiguous()
    out = dict(batch=bsz, steps=steps, heads=heads, dq=dq, dtype='bf16', path=F.qattention_path(dt, bsz, steps, heads, dq, packed=True),
               calls=args.calls, gflop_fwd_all_pairs=round(4e-9 * bsz * heads * steps * steps * 4 * dq, 2))
    rng = np.random.RandomState(0)
    for case, n in (('timit_lengths', timit_lengths(bsz, steps, rng)), ('full_lengths', np.full(bsz, steps, dtype=np.int32))):
        lengths = torch.tensor(n, device=dev)
        mask = (torch.arange(steps, device=dev)[None, :] < lengths[:, None])[:, None, None, :]
        gflop = 4e-9 * heads * 4 * dq * float((n.astype(np.float64) ** 2).sum())

        def sdpa_fwd():
            with torch.no_grad():
                torch.nn.functional.scaled_dot_product_attention(qh, kh, vh, attn_mask=mask)

        def sdpa_both():
            torch.nn.functional.scaled_dot_product_attention(qh, kh, vh, attn_mask=mask).backward(doh)
            qh.grad = kh.grad = vh.grad = None

        def fused_fwd():
            with torch.no_grad():
                F.qattention_packed(qkv, heads, lengths)

        def fused_both():
            F.qattention_packed(qkv, heads, lengths).backward(do)
            qkv.grad = None

        def composed_fwd():
            with torch.no_grad():
                composed(qkv, heads, lengths)

        def composed_both():
            composed(qkv, heads, lengths).backward(do)
            qkv.grad = None

        res = dict(mean_length=round(float(n.mean()), 1), gflop_fwd=round(gflop, 2))
        with torch.no_grad():                                            # the two forms compute the same thing
            res['max_abs_difference_of_o'] = float((F.qattention_packed(qkv, heads, lengths).float() - composed(qkv, heads, lengths).float()).abs().max())
        first = dict(fwd=timed(sdpa_fwd, args.calls), both=timed(sdpa_both, args.calls))
        fused = dict(fwd=timed(fused_fwd, args.calls), both=timed(fused_both, args.calls))
        comp = dict(fwd=timed(composed_fwd, args.calls), both=timed(composed_both, args.calls))
        last = dict(fwd=timed(sdpa_fwd, args.calls), both=timed(sdpa_both, args.calls))
        sd = {k: 0.5 * (first[k] + last[k]) for k in first}
        res['sdpa_ms'] = dict(fwd_first=round(first['fwd'], 4), fwd_last=round(last['fwd'], 4), fwd_bwd_first=round(first['both'], 4),
                              fwd_bwd_last=round(last['both'], 4), spread_fwd=round(abs(first['fwd'] - last['fwd']), 4),
                              spread_fwd_bwd=round(abs(first['both'] - last['both']), 4))
        res['fused_ms'] = dict(fwd=round(fused['fwd'], 4), fwd_bwd=round(fused['both'], 4), bwd=round(fused['both'] - fused['fwd'], 4))
        res['fused_tflops'] = dict(fwd=round(gflop / fused['fwd'], 2), bwd=round(3.5 * gflop / (fused['both'] - fused['fwd']), 2))
        res['composed_ms'] = dict(fwd=round(comp['fwd'], 4), fwd_bwd=round(comp['both'], 4))
        res['fused_over_sdpa'] = dict(fwd=round(fused['fwd'] / sd['fwd'], 3), fwd_bwd=round(fused['both'] / sd['both'], 3))
        res['composed_over_fused'] = dict(fwd=round(comp['fwd'] / fused['fwd'], 2), fwd_bwd=round(comp['both'] / fused['both'], 2))
        out[case] = res
    del qkv, do, qh, kh, vh, doh, x
    torch.cuda.empty_cache()

    if args.model_steps > 0:
        np.random.seed(0)
        torch.manual_seed(0)
        model = TimitQTransformer(num_layers=6, units=512, heads=8, ff_units=2048, dropout=0.1)
        xin = torch.randn((bsz, 4, 41, steps), device=dev, generator=gen).to(dt)
        il = torch.tensor(timit_lengths(bsz, steps, np.random.RandomState(0)), device=dev).view(bsz, 1)
        labels = torch.randint(0, 61, (bsz, 20), device=dev, generator=gen, dtype=torch.int32)
        ll = torch.full((bsz, 1), 20, dtype=torch.int32, device=dev)
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
        out['model_step_ms'] = round(timed(train_step, args.model_steps, 2), 2)
        out['model_parameters'] = int(flat.param.numel())
    print(json.dumps(out))


if __name__ == '__main__':
    main()
