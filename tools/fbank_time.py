#!/usr/bin/env python
"""Times the acoustic front end (features.quaternion_fbank) at B = 256 utterances of 2 s (32 000 int16 samples -> 199 frames) with HIP
events after warm-up, against one training step of TimitQCNN(10, 32) on the features it produces, and optionally against the float64
test reference on the CPU; prints one JSON line per measurement.

    python tools/fbank_time.py [--reps 20] [--cpu-ref 0]        # --cpu-ref N: also time tests/fbank_ref.py on N utterances
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.realpath(__file__)))
sys.path.insert(0, ROOT)
import qcnn_amd  # noqa: E402,F401
from qcnn_amd import dp, functional as F  # noqa: E402
from qcnn_amd.features import quaternion_fbank  # noqa: E402
from qcnn_amd.models.interspeech_model import TimitQCNN  # noqa: E402


def timed(fn, reps, warmup=3):
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
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--cpu-ref', type=int, default=0)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    B, N = 256, 32000
    rng = np.random.RandomState(0)
    t = np.arange(N) / 16000.0
    wave_np = (4000 * np.sin(2 * np.pi * rng.uniform(100, 4000, size=(B, 1)) * t) + 300 * rng.randn(B, N)).astype(np.int16)
    wave = torch.from_numpy(wave_np).to(dev)
    lengths = torch.full((B,), N, dtype=torch.int32, device=dev)
    for dt, name in ((torch.bfloat16, 'bf16'), (torch.float32, 'fp32')):
        report('fbank', timed(lambda: quaternion_fbank(wave, lengths, dtype=dt), args.reps), B=B, samples=N, frames=199, out=name)
    report('fbank_normalized', timed(lambda: quaternion_fbank(wave, lengths, dtype=torch.bfloat16, normalize='utterance'), args.reps),
           B=B, samples=N, frames=199, out='bf16')

    x, fl = quaternion_fbank(wave, lengths, dtype=torch.bfloat16, normalize='utterance')
    np.random.seed(0)
    model = TimitQCNN(num_layers=10, start_filter=32, aact='none', dropout=0.3, l2=1e-5)
    with torch.no_grad():
        model(x[:1])
    model.to(dev)
    model.train()
    flat = dp.FlatParams([p for p in model.parameters() if p.requires_grad])
    m, v = torch.zeros_like(flat.param), torch.zeros_like(flat.param)
    labels = torch.randint(0, 61, (B, 40), device=dev, dtype=torch.int32)
    ll = torch.randint(20, 41, (B, 1), device=dev, dtype=torch.int32)
    il = fl[:, None]
    step = [0]

    def train_step():
        step[0] += 1
        loss = model.training_loss(x, labels, il, ll)
        loss.backward()
        F.adam_step(flat.param, flat.grad, m, v, step[0], zero_grad=True)
    report('train_step', timed(train_step, max(3, args.reps // 2)), B=B, T=int(x.shape[-1]), model='TimitQCNN(10, 32) bf16')

    if args.cpu_ref > 0:
        sys.path.insert(0, os.path.join(ROOT, 'tests'))
        import fbank_ref as R
        t0 = time.perf_counter()
        R.quaternion_fbank(wave_np[:args.cpu_ref], [N] * args.cpu_ref)
        dt = time.perf_counter() - t0
        print(json.dumps(dict(name='cpu_float64_reference', utterances=args.cpu_ref, seconds=round(dt, 3),
                              projected_batch_seconds=round(dt * B / args.cpu_ref, 2))), flush=True)


if __name__ == '__main__':
    main()
