"""NumPy restatement of the reverberation and additive-noise semantics in include/qk.h ("Reverberation and additive noise"): Python
integers for the draws, the fp32 bank values and samples multiplied out and summed in float64.  Written from the header's text, not
from the kernels (csrc/qk_env_aug.hip).
"""
import math

import numpy as np

from specaug_ref import randint, u

PLAN_WORDS = 8
ONE = 1 << 24


def q24(p):
    return int(round(p * ONE))


def snr_of(b, snr=(5.0, 20.0), seed=0, counter=0):
    """snr as float32: the difference, the product and the sum each rounded once."""
    lo, hi = np.float32(snr[0]), np.float32(snr[1])
    f = np.float32(u(seed, counter, b, 77) >> 8) * np.float32(2.0 ** -24)
    return np.float32(lo + np.float32(np.float32(hi - lo) * f))


def plan_row(b, length, max_samples, n_rirs=0, n_noises=0, noise_len=(), rir_prob=1.0, noise_prob=1.0, snr=(5.0, 20.0), seed=0, counter=0):
    """(n, ri or -1, ni or -1, o, snr as float32) of utterance b: the integer words of the plan row and the snr."""
    n = min(max(int(length), 0), max_samples)
    do_rir = n_rirs > 0 and (u(seed, counter, b, 72) >> 8) < q24(rir_prob)
    do_noise = n_noises > 0 and (u(seed, counter, b, 74) >> 8) < q24(noise_prob)
    ri = randint(seed, counter, b, 73, n_rirs) if do_rir else -1
    ni = randint(seed, counter, b, 75, n_noises) if do_noise else -1
    o = randint(seed, counter, b, 76, int(noise_len[ni])) if do_noise else 0
    return n, ri, ni, o, snr_of(b, snr, seed, counter)


def reverb_row(x, n, h, d):
    """r[m] = sum_j h[j] x[m + d - j] for m < n with x zero outside [0, n), and S[m] = sum_j |h[j] x[m + d - j]|: float64.  x: the
    input row (samples >= n are never touched); h: the response's Lr taps (float32)."""
    xv = np.asarray(x[:n], dtype=np.float64)
    hv = np.asarray(h, dtype=np.float64)
    if n == 0:
        return np.zeros(0), np.zeros(0)
    return np.convolve(xv, hv)[d:d + n], np.convolve(np.abs(xv), np.abs(hv))[d:d + n]


def gain(Es, En, snr):
    """a: float64 arithmetic, rounded once to float32; 0 when either energy is 0."""
    if Es == 0 or En == 0:
        return np.float32(0)
    return np.float32(math.sqrt(float(Es) / float(En)) * 10.0 ** (-float(snr) / 20.0))


def noise_reverb(x, lengths, rirs=None, noises=None, rir_prob=1.0, noise_prob=1.0, snr=(5.0, 20.0), seed=0, counter=0, gains=None):
    """x (B, max_samples), rirs = (bank (R, stride) float32, rir_len, rir_delay) or None, noises = (bank, noise_len) or None, all
    NumPy.  gains: per-utterance float32 a to use in `out` instead of the reference's own (the device's, when a test bounds the
    device's values).  Returns a dict of per-utterance lists / arrays: rows (plan_row), Lr, r, S, v (float64, length n), Es, En
    (float64), a (float32, the reference's own) and out (B, max_samples) float64 with zeros from n on."""
    x = np.asarray(x)
    B, n_max = x.shape
    n_rirs = 0 if rirs is None else rirs[0].shape[0]
    n_noises = 0 if noises is None else noises[0].shape[0]
    res = dict(rows=[], Lr=[], r=[], S=[], v=[], Es=[], En=[], a=[], out=np.zeros((B, n_max)))
    for b in range(B):
        row = plan_row(b, lengths[b], n_max, n_rirs, n_noises, () if noises is None else noises[1], rir_prob, noise_prob, snr, seed, counter)
        n, ri, ni, o, s = row
        if ri >= 0:
            Lr = int(rirs[1][ri])
            r, S = reverb_row(x[b], n, rirs[0][ri, :Lr], int(rirs[2][ri]))
        else:
            Lr = 1
            r = np.asarray(x[b, :n], dtype=np.float32).astype(np.float64)
            S = np.abs(r)
        v = np.zeros(n)
        Es = En = 0.0
        a = np.float32(0)
        if ni >= 0:
            Ln = int(noises[1][ni])
            v = noises[0][ni, (o + np.arange(n)) % Ln].astype(np.float64)
            Es, En = float(np.sum(r * r)), float(np.sum(v * v))
            a = gain(Es, En, s)
        use = a if gains is None else gains[b]
        res['out'][b, :n] = r + float(use) * v
        for key, val in (('rows', row), ('Lr', Lr), ('r', r), ('S', S), ('v', v), ('Es', Es), ('En', En), ('a', a)):
            res[key].append(val)
    return res
