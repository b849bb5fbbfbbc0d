#!/usr/bin/env python
"""Times SpecAugment (functional.spec_augment, one launch of qk_spec_augment) on the TIMIT model's input at B = 256: (256, 4, 41, 199),
the default policy of features.SpecAugment, fp32 -> bf16 (the path quaternion_fbank(augment=) takes) and bf16 -> bf16, with HIP events
after warm-up.  The yardstick is the device copy out.copy_(x) on the same tensors -- the least traffic any augmenter can have -- and,
for scale, the front end that produces the input (features.quaternion_fbank).  Prints one JSON line per measurement.

    python tools/specaug_time.py [--reps 200]
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.realpath(__file__)))
sys.path.insert(0, ROOT)
import qcnn_amd  # noqa: E402,F401
from qcnn_amd import _lib as L, functional as F  # noqa: E402
from qcnn_amd.features import SpecAugment, quaternion_fbank  # noqa: E402


def timed(fn, reps, warmup=20):
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
    return med_min[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=200)
    args = ap.parse_args()
    if args.reps < 100:
        raise SystemExit('--reps must be at least 100')
    dev = torch.device('cuda:0')
    B, P, R, T = 256, 4, 41, 199
    policy = SpecAugment().policy
    gen = torch.Generator(device=dev).manual_seed(0)
    x32 = torch.randn(B, P, R, T, device=dev, generator=gen)
    lengths = torch.randint(120, T + 1, (B,), device=dev, generator=gen, dtype=torch.int32)
    counter = torch.zeros(1, dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    for xin, dt_out, name in ((x32, torch.bfloat16, 'fp32->bf16'), (x32.to(torch.bfloat16), torch.bfloat16, 'bf16->bf16')):
        out = torch.empty(xin.shape, dtype=dt_out, device=dev)
        plan = torch.empty(B, L.QK_SPECAUG_PLAN_WORDS, dtype=torch.int32, device=dev)
        pol = F._specaug_policy('specaug_time', **policy)

        def kernel(xin=xin, out=out, plan=plan, pol=pol):      # the launch alone, into preallocated tensors, like the copy below
            L.check(L.lib().qk_spec_augment(F._DTYPES[xin.dtype], F._DTYPES[out.dtype], B, P, R, T, xin.data_ptr(), lengths.data_ptr(),
                                            ctypes.byref(pol), counter.data_ptr(), out.data_ptr(), plan.data_ptr(), stream),
                    'qk_spec_augment')
        nbytes = xin.numel() * (xin.element_size() + out.element_size())
        t_aug = report('spec_augment', timed(kernel, args.reps), dtypes=name, shape=[B, P, R, T], bytes_in_plus_out=nbytes, **policy)
        t_api = report('spec_augment_python', timed(lambda: F.spec_augment(xin, lengths, counter=counter, dtype=dt_out, return_plan=True,
                                                                           **policy), args.reps), dtypes=name)
        t_copy = report('copy_', timed(lambda: out.copy_(xin), args.reps), dtypes=name, bytes_in_plus_out=nbytes)
        print(json.dumps(dict(name='ratio', dtypes=name, spec_augment_over_copy=round(t_aug / t_copy, 3),
                              python_call_over_copy=round(t_api / t_copy, 3))), flush=True)

    N = 32000
    rng = np.random.RandomState(0)
    t = np.arange(N) / 16000.0
    wave = torch.from_numpy((4000 * np.sin(2 * np.pi * rng.uniform(100, 4000, size=(B, 1)) * t) + 300 * rng.randn(B, N)).astype(np.int16)).to(dev)
    wl = torch.full((B,), N, dtype=torch.int32, device=dev)
    report('fbank', timed(lambda: quaternion_fbank(wave, wl, dtype=torch.bfloat16), args.reps), B=B, samples=N, frames=T, out='bf16')
    aug = SpecAugment()
    report('fbank_normalized', timed(lambda: quaternion_fbank(wave, wl, dtype=torch.bfloat16, normalize='utterance'), args.reps),
           B=B, samples=N, frames=T, out='bf16')
    report('fbank_normalized_augmented', timed(lambda: quaternion_fbank(wave, wl, dtype=torch.bfloat16, normalize='utterance', augment=aug),
                                               args.reps), B=B, samples=N, frames=T, out='bf16')


if __name__ == '__main__':
    main()
