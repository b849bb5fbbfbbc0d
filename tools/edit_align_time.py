#!/usr/bin/env python
"""Times the scoring alignment (functional.edit_alignment, csrc/qk_edit_align.hip) at the evaluation shape -- B = 256 pairs,
hyp_stride = 200 (the frames of a decode), references of 20 .. 75 of 61 symbols, hypotheses with about 8 % of the tokens dropped,
20 % replaced and 5 % extra -- with HIP events after warm-up, four ways on the same tensors in the same run: with the alignment
rows, counts only, counts with the 61-class confusion matrix, and functional.edit_distance.  One JSON line per measurement.

    python tools/edit_align_time.py [--reps 200]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.realpath(__file__)))
sys.path.insert(0, ROOT)
import qcnn_amd  # noqa: E402,F401
from qcnn_amd import functional as F  # noqa: E402


def timed(fn, reps, warmup=10):
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


def make_pairs(rng, B, hs, rs, symbols):
    hyp = np.full((B, hs), -1, dtype=np.int32)
    ref = np.full((B, rs), -1, dtype=np.int32)
    hl, rl = np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.int32)
    for b in range(B):
        r = rng.randint(0, symbols, size=rng.randint(20, rs + 1))
        h = []
        for t in r:
            u = rng.rand()
            if u >= 0.08:
                h.append(rng.randint(symbols) if u < 0.28 else t)
            if rng.rand() < 0.05:
                h.append(rng.randint(symbols))
        h = h[:hs]
        ref[b, :len(r)], rl[b] = r, len(r)
        hyp[b, :len(h)], hl[b] = h, len(h)
    return hyp, hl, ref, rl


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=200)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    B, hs, rs, symbols = 256, 200, 75, 61
    hyp, hl, ref, rl = (torch.from_numpy(a).to(dev) for a in make_pairs(np.random.RandomState(0), B, hs, rs, symbols))
    conf = torch.zeros((symbols + 1, symbols + 1), dtype=torch.int32, device=dev)
    shape = dict(B=B, hyp_stride=hs, ref_stride=rs, symbols=symbols)
    counts = F.edit_alignment(hyp, hl, ref, rl, align=False).counts.sum(0).tolist()
    full = timed(lambda: F.edit_alignment(hyp, hl, ref, rl), args.reps)
    only = timed(lambda: F.edit_alignment(hyp, hl, ref, rl, align=False), args.reps)
    matrix = timed(lambda: F.edit_alignment(hyp, hl, ref, rl, confusion=conf, align=False), args.reps)
    dist = timed(lambda: F.edit_distance(hyp, hl, ref, rl), args.reps)
    report('edit_alignment_with_rows', full, csdi=counts, **shape)
    report('edit_alignment_counts_only', only, **shape)
    report('edit_alignment_counts_and_matrix', matrix, **shape)
    report('edit_distance', dist, **shape)
    report('edit_alignment_with_rows_again', timed(lambda: F.edit_alignment(hyp, hl, ref, rl), args.reps),
           ratio_to_edit_distance=round(full[0] / dist[0], 3), **shape)


if __name__ == '__main__':
    main()
