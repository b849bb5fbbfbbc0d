#!/usr/bin/env python
"""Times the CTC decoders and the edit distance at the benchmark shape (B = 256, T = 200, C = 62, bf16 posteriors) with HIP events
after warm-up, and TimitQCNN.evaluate against the eval-mode forward alone; prints one JSON line per measurement.

    python tools/ctc_decode_time.py [--reps 20] [--cpu-ref 0]        # --cpu-ref N: also time the float64 test reference on N utterances
    python tools/ctc_decode_time.py --lm-order 2                     # only the beam search at W = 16 / 100, plain and with an n-gram LM

The posteriors are peaky synthetic ones (softmax of scaled random logits, blank-heavy), like a trained model's output.
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
from qcnn_amd import functional as F, layers  # noqa: E402
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


def time_lm(args, y, il):
    """Plain and LM-fused beam search at W = 16 and 100 in the same process, on an LM estimated from random phone sequences."""
    from qcnn_amd.lm import NgramLM
    B, T, C = y.shape
    rng = np.random.RandomState(1)
    corpus = [rng.randint(0, C - 1, size=rng.randint(20, 60)).tolist() for _ in range(2000)]
    lm = NgramLM.estimate(corpus, C - 1, args.lm_order)
    reps = max(3, args.reps // 2)
    for W in (16, 100):
        plain = timed(lambda: F.ctc_beam_search_decode(y, il, beam_width=W), reps)
        fused = timed(lambda: F.ctc_beam_search_decode_lm(y, il, lm, beam_width=W, lm_weight=args.lm_weight, insertion_bonus=0.5), reps)
        report('beam', plain, B=B, T=T, C=C, beam_width=W, dtype='bf16')
        report('beam_lm', fused, B=B, T=T, C=C, beam_width=W, dtype='bf16', lm_order=args.lm_order,
               ratio_to_plain=round(fused[0] / plain[0], 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--cpu-ref', type=int, default=0)
    ap.add_argument('--lm-order', type=int, default=0, help='time the LM beam search (order 1-3) next to the plain one, and only those')
    ap.add_argument('--lm-weight', type=float, default=0.5)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    B, T, C = 256, 200, 62
    rng = np.random.RandomState(0)
    z = rng.randn(B, T, C) * 3.0
    z[..., -1] += 3.0
    y = torch.softmax(torch.tensor(z, dtype=torch.float32), dim=-1).to(dev, torch.bfloat16)
    il = torch.full((B,), T, dtype=torch.int32, device=dev)
    if args.lm_order:
        time_lm(args, y, il)
        return
    report('greedy', timed(lambda: F.ctc_greedy_decode(y, il), args.reps), B=B, T=T, C=C, dtype='bf16')
    for W, top in ((1, 1), (16, 1), (100, 1), (100, 3)):
        report('beam', timed(lambda: F.ctc_beam_search_decode(y, il, beam_width=W, top_paths=top), max(3, args.reps // 2)),
               B=B, T=T, C=C, beam_width=W, top_paths=top, dtype='bf16')
    dec, dlen, _ = F.ctc_greedy_decode(y, il)
    labels = torch.randint(0, 61, (B, 75), device=dev, dtype=torch.int32)
    ll = torch.randint(40, 76, (B,), device=dev, dtype=torch.int32)
    report('edit_distance', timed(lambda: F.edit_distance(dec, dlen, labels, ll), args.reps), B=B, hyp_stride=T, ref_stride=75)

    np.random.seed(0)
    model = TimitQCNN(num_layers=10, start_filter=32, aact='none', dropout=0.3)
    x = torch.randn(B, 4, 41, T, device=dev).to(torch.bfloat16)
    with torch.no_grad():
        model(x[:1])
    model.to(dev)
    ilm = il.reshape(-1, 1)

    def fwd():
        model.eval()
        with torch.no_grad():
            model(x)
        model.train()
    report('eval_forward', timed(fwd, max(3, args.reps // 2)), B=B, T=T, model='TimitQCNN(10, 32)')
    report('evaluate_greedy', timed(lambda: model.evaluate(x, labels, ilm, ll), max(3, args.reps // 2)), B=B, T=T)
    report('evaluate_beam100', timed(lambda: model.evaluate(x, labels, ilm, ll, greedy=False, beam_width=100), 3, warmup=1), B=B, T=T)
    if args.cpu_ref > 0:
        sys.path.insert(0, os.path.join(ROOT, 'tests'))
        import ctc_decode_ref as R
        yn = y[:args.cpu_ref].float().cpu().numpy()
        t0 = time.perf_counter()
        R.beam_search_decode(yn, np.full(args.cpu_ref, T), 100, 1)
        dt = time.perf_counter() - t0
        print(json.dumps(dict(name='cpu_float64_reference_beam100', utterances=args.cpu_ref, seconds=round(dt, 3),
                              projected_batch_seconds=round(dt * B / args.cpu_ref, 1))), flush=True)


if __name__ == '__main__':
    main()
