#!/usr/bin/env python
"""Times the assembly of one training batch of 256 utterances of 2 - 4 s (synthetic int16 waveforms at 16 kHz, 20 - 50 labels each;
2048 utterances, 8 length-sorted batches), on the host as examples/train_timit.py does it and on the device (qcnn_amd.data):

  host_assembly    the example's to_device up to its three device tensors, the filter bank excluded: np.zeros, the Python loop of row
                   copies for waveforms and labels, three pageable host-to-device copies, two host lists -> tensors.  Wall time per
                   batch with a synchronise, over the batches in order.  Timed FIRST and LAST; the difference of the two medians is
                   the spread of the run.
  next_batch       DeviceCorpus.next_batch in tight mode (host mirror of the permutation, output allocation, one launch, the cursor's
                   add_), wall time per batch with a synchronise.
  launch           qk_corpus_batch alone, through the C-ABI into preallocated outputs at the row's tight widths, HIP events around one
                   launch (median / min) and around `reps` launches back to back (mean).
  copy             out.copy_(x) of a (256, n_out) int16 tensor, the same output bytes: the floor of a kernel that writes them.

Prints one JSON line per measurement.

    python tools/corpus_batch_time.py [--reps 200]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.realpath(__file__)))
sys.path.insert(0, ROOT)
import qcnn_amd  # noqa: E402,F401
from qcnn_amd import _lib as L, functional as F  # noqa: E402
from qcnn_amd.data import DeviceCorpus, EpochSampler  # noqa: E402


def host_assembly(utts, idx, dev):
    """to_device of examples/train_timit.py without the front end."""
    n = [len(utts[i][0]) for i in idx]
    wave = np.zeros((len(idx), max(n)), dtype=np.int16)
    lab_len = [len(utts[i][1]) for i in idx]
    labels = np.zeros((len(idx), max(lab_len)), dtype=np.int32)
    for r, i in enumerate(idx):
        wave[r, :n[r]] = utts[i][0]
        labels[r, :lab_len[r]] = utts[i][1]
    return (torch.from_numpy(wave).to(dev), torch.tensor(n, dtype=torch.int32), torch.from_numpy(labels).to(dev),
            torch.tensor(lab_len, dtype=torch.int32, device=dev)[:, None])


def wall(fn, reps, warmup=8):
    """Median / min wall milliseconds of fn() followed by a synchronise."""
    for k in range(warmup):
        fn(k)
    torch.cuda.synchronize()
    times = []
    for k in range(reps):
        t0 = time.perf_counter()
        fn(k)
        torch.cuda.synchronize()
        times.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(times)), float(np.min(times))


def events(fn, reps, warmup=20):
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
    ev[0].record()
    for _ in range(reps):
        fn()
    ev[1].record()
    ev[1].synchronize()
    return float(np.median(times)), float(np.min(times)), ev[0].elapsed_time(ev[1]) / reps


def report(name, **kw):
    print(json.dumps(dict(name=name, **{k: round(v, 4) if isinstance(v, float) else v for k, v in kw.items()})), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=200)
    ap.add_argument('--utterances', type=int, default=2048)
    args = ap.parse_args()
    if args.reps < 50:
        raise SystemExit('--reps must be at least 50')
    dev = torch.device('cuda:0')
    B = 256
    rng = np.random.RandomState(0)
    utts = [(rng.randint(-3000, 3000, size=int(n)).astype(np.int16), rng.randint(0, 61, size=int(rng.randint(20, 51))).astype(np.int32))
            for n in rng.randint(32000, 64001, size=args.utterances)]
    corpus = DeviceCorpus([u[0] for u in utts], [u[1] for u in utts], device=dev)
    sampler = EpochSampler(corpus.wave_len, B, seed=0)
    rows = [[int(i) for i in row if i >= 0] for row in sampler.batches]
    nb = len(rows)
    report('corpus', utterances=len(utts), batches=nb, wave_pack_mb=2e-6 * corpus.arrays.wave_pack.numel())

    def host(k):
        return host_assembly(utts, rows[k % nb], dev)
    first = wall(host, args.reps)
    report('host_assembly_first', median_ms=first[0], min_ms=first[1])
    nxt = wall(lambda k: corpus.next_batch(sampler), args.reps)
    report('next_batch_tight', median_ms=nxt[0], min_ms=nxt[1])

    batches_dev, _ = sampler.on(dev)
    desc, _ = F._corpus_desc('corpus_batch_time', corpus.arrays)
    sched = L.BatchScheduleDesc(batches_dev.data_ptr(), nb, B, 0, 0)
    stream = torch.cuda.current_stream().cuda_stream
    for row in sorted({0, nb // 2, nb - 1}):
        n_out, l_out = int(corpus.wave_len[rows[row]].max()), int(corpus.label_len[rows[row]].max())
        for n_out in sorted({n_out, (n_out + 7) // 8 * 8, n_out | 1}):            # as it comes, rows 16-byte aligned, rows at all 8 shifts
            wave = torch.empty(B, n_out, dtype=torch.int16, device=dev)
            small = [torch.empty(B, dtype=torch.int32, device=dev), torch.empty(B, l_out, dtype=torch.int32, device=dev),
                     torch.empty(B, dtype=torch.int32, device=dev)]

            def launch():
                L.check(L.lib().qk_corpus_batch(ctypes.byref(desc), ctypes.byref(sched), row, None, n_out, l_out, wave.data_ptr(),
                                                small[0].data_ptr(), small[1].data_ptr(), small[2].data_ptr(), None, None, None, stream),
                        'qk_corpus_batch')
            med, mn, mean = events(launch, args.reps)
            read = 2 * int(corpus.wave_len[rows[row]].sum())
            src = torch.empty_like(wave).fill_(1)
            cmed, cmn, cmean = events(lambda: wave.copy_(src), args.reps)
            report('launch', row=row, n_out=n_out, l_out=l_out, median_ms=med, min_ms=mn, back_to_back_ms=mean,
                   written_mb=2e-6 * B * n_out, read_mb=1e-6 * read, gb_per_s=(2.0 * B * n_out + read) / (mean * 1e-3) / 1e9)
            report('copy', row=row, n_out=n_out, median_ms=cmed, min_ms=cmn, back_to_back_ms=cmean,
                   gb_per_s=4.0 * B * n_out / (cmean * 1e-3) / 1e9, launch_over_copy=mean / cmean)
    last = wall(host, args.reps)
    report('host_assembly_last', median_ms=last[0], min_ms=last[1], spread_ms=abs(last[0] - first[0]))
    report('summary', host_ms=0.5 * (first[0] + last[0]), next_batch_ms=nxt[0], host_over_next_batch=0.5 * (first[0] + last[0]) / nxt[0])


if __name__ == '__main__':
    main()
