#!/usr/bin/env python
"""Times reverberation and additive noise (qk_noise_reverb: the filter launch and the mix launch) on a batch of two-second
utterances, (256, 32000), int16 and float32, with a bank of 32 responses of 4000 taps (0.25 s at 16 kHz) and 8 noise recordings,
with HIP events: 200 timed calls after warm-up, into preallocated tensors.  Cases: rir_prob 1 and 0.5, each with noise_prob 0 and 1,
and the noise-only call.  For the rir_prob = 1 call it prints the achieved FLOP/s -- 2 * taps multiply-adds per valid output,
6.55e10 FLOP -- against the 157.3 TF fp32 vector peak (packed FMA), whose arithmetic floor is 0.42 ms.  For scale, the same run times
the front end (features.quaternion_fbank) and functional.speed_perturb on the same batch.  Prints one JSON line per measurement.

    python tools/noise_reverb_time.py [--reps 200]
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
from qcnn_amd.features import NoiseReverb, SpeedPerturb, quaternion_fbank, synthetic_noises  # noqa: E402

PEAK_FP32 = 157.3e12


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
    ap.add_argument('--taps', type=int, default=4000)
    args = ap.parse_args()
    if args.reps < 100:
        raise SystemExit('--reps must be at least 100')
    dev = torch.device('cuda:0')
    B, N, taps = 256, 32000, args.taps
    rng = np.random.RandomState(0)
    t = np.arange(N) / 16000.0
    wave16 = torch.from_numpy((4000 * np.sin(2 * np.pi * rng.uniform(100, 4000, size=(B, 1)) * t) + 300 * rng.randn(B, N)).astype(np.int16)).to(dev)
    lengths = torch.full((B,), N, dtype=torch.int32, device=dev)
    counter = torch.zeros(1, dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    hs = [np.concatenate([[1.0], 0.05 * rng.randn(taps - 1) * np.exp(-np.arange(1, taps) / (taps / 6.9))]) for _ in range(32)]
    rirs = F.prepare_rirs(hs, device=dev)
    noises = F.prepare_noises(synthetic_noises(8, 64000, seed=1), device=dev)
    assert rirs[1].tolist() == [taps] * 32
    out = torch.empty(B, N, device=dev)
    plan = torch.empty(B, L.QK_NOISE_REVERB_PLAN_WORDS, dtype=torch.int32, device=dev)
    ws_bytes = int(L.lib().qk_noise_reverb_workspace_bytes(B, N))
    ws = torch.empty(ws_bytes // 8, dtype=torch.float64, device=dev)
    flop = 2.0 * taps * B * N
    for wave, name in ((wave16, 'int16'), (wave16.float(), 'float32')):
        wd = L.QK_WAVE_I16 if wave.dtype == torch.int16 else L.QK_WAVE_F32
        for rir_prob, noise_prob in ((1.0, 0.0), (1.0, 1.0), (0.5, 0.0), (0.5, 1.0), (0.5, 0.5), (0.0, 1.0)):
            _, _, pol = F._env_args('noise_reverb_time', rirs, noises, rir_prob, noise_prob, (5.0, 20.0), 0)

            def kernel(wave=wave, wd=wd, pol=pol):                     # the launches alone, into preallocated tensors
                L.check(L.lib().qk_noise_reverb(wd, B, N, wave.data_ptr(), lengths.data_ptr(), ctypes.byref(pol), rirs[0].data_ptr(),
                                                rirs[1].data_ptr(), rirs[2].data_ptr(), noises[0].data_ptr(), noises[1].data_ptr(),
                                                counter.data_ptr(), out.data_ptr(), plan.data_ptr(), ws.data_ptr(), ws_bytes, stream),
                        'qk_noise_reverb')
            ms = report('noise_reverb', timed(kernel, args.reps), wave=name, shape=[B, N], taps=taps, rir_prob=rir_prob, noise_prob=noise_prob)
            if rir_prob == 1.0:
                reverberated = int((plan[:, 1] >= 0).sum().item())
                assert reverberated == B
                print(json.dumps(dict(name='rate', wave=name, noise_prob=noise_prob, flop=flop, tflops=round(flop / (ms * 1e-3) / 1e12, 2),
                                      share_of_fp32_peak=round(flop / (ms * 1e-3) / PEAK_FP32, 3), floor_ms=round(flop / PEAK_FP32 * 1e3, 3))),
                      flush=True)
        nr = NoiseReverb(rirs=rirs, noises=noises)
        report('noise_reverb_python_default', timed(lambda: nr(wave, lengths), args.reps), wave=name, rir_prob=0.5, noise_prob=0.5)
        report('fbank', timed(lambda: quaternion_fbank(wave, lengths, dtype=torch.bfloat16), args.reps), wave=name, B=B, samples=N, out='bf16')
        report('fbank_noise_reverb_default', timed(lambda: quaternion_fbank(wave, lengths, dtype=torch.bfloat16, wave_augment=nr), args.reps),
               wave=name, B=B, samples=N, out='bf16')
        sp = SpeedPerturb()
        report('speed_perturb', timed(lambda: F.speed_perturb(wave, lengths, counter=counter, **sp.policy), args.reps), wave=name)


if __name__ == '__main__':
    main()
