#!/usr/bin/env python
"""Times speed and volume perturbation (functional.speed_perturb, one launch of qk_speed_perturb) on a batch of two-second
utterances, (256, 32000), int16 and float32, with the default policy of features.SpeedPerturb (speeds 0.9 / 1.0 / 1.1), with HIP
events: 200 timed calls after warm-up.  The bytes are those the algorithm needs -- every valid input sample read once, every output
sample written once -- so bytes over time is the achieved rate to hold against the HBM rate.  For scale, the same run times the
front end (features.quaternion_fbank) on the same batch, with and without wave_augment=.  Prints one JSON line per measurement.

    python tools/speed_perturb_time.py [--reps 200]
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
from qcnn_amd.features import SpeedPerturb, quaternion_fbank  # noqa: E402


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
    B, N = 256, 32000
    rng = np.random.RandomState(0)
    t = np.arange(N) / 16000.0
    wave16 = torch.from_numpy((4000 * np.sin(2 * np.pi * rng.uniform(100, 4000, size=(B, 1)) * t) + 300 * rng.randn(B, N)).astype(np.int16)).to(dev)
    lengths = torch.full((B,), N, dtype=torch.int32, device=dev)
    counter = torch.zeros(1, dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    sp = SpeedPerturb()
    pol, tab, _ = F._speed_policy(sp.policy['speeds'], sp.policy['gain'], sp.policy['zeros'], sp.policy['rolloff'], sp.policy['seed'])
    tables = torch.from_numpy(tab['tables'].copy()).to(dev)
    n_out = int(L.lib().qk_speed_perturb_out_samples(N, ctypes.byref(pol)))
    out = torch.empty(B, n_out, device=dev)
    olen = torch.empty(B, dtype=torch.int32, device=dev)
    plan = torch.empty(B, L.QK_SPEED_PLAN_WORDS, dtype=torch.int32, device=dev)
    for wave, name in ((wave16, 'int16'), (wave16.float(), 'float32')):
        wd = L.QK_WAVE_I16 if wave.dtype == torch.int16 else L.QK_WAVE_F32

        def kernel(wave=wave, wd=wd):                             # the launch alone, into preallocated tensors
            L.check(L.lib().qk_speed_perturb(wd, B, N, wave.data_ptr(), lengths.data_ptr(), ctypes.byref(pol), tables.data_ptr(),
                                             counter.data_ptr(), n_out, out.data_ptr(), olen.data_ptr(), plan.data_ptr(), stream),
                    'qk_speed_perturb')
        nbytes = wave.numel() * wave.element_size() + out.numel() * 4
        ms = report('speed_perturb', timed(kernel, args.reps), wave=name, shape=[B, N], out_samples=n_out, bytes_in_plus_out=nbytes,
                    speeds=[list(s) for s in sp.policy['speeds']])
        print(json.dumps(dict(name='rate', wave=name, tb_per_s=round(nbytes / (ms * 1e-3) / 1e12, 3))), flush=True)
        report('speed_perturb_python', timed(lambda: F.speed_perturb(wave, lengths, counter=counter, return_plan=True, **sp.policy),
                                             args.reps), wave=name)
        report('fbank', timed(lambda: quaternion_fbank(wave, lengths, dtype=torch.bfloat16), args.reps), wave=name, B=B, samples=N, out='bf16')
        report('fbank_speed_perturbed', timed(lambda: quaternion_fbank(wave, lengths, dtype=torch.bfloat16, wave_augment=sp), args.reps),
               wave=name, B=B, samples=N, out='bf16')


if __name__ == '__main__':
    main()
