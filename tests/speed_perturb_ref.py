"""NumPy restatement of the speed and volume perturbation semantics in include/qk.h ("Speed and volume perturbation"): Python
integers for the draws and the index arithmetic, the fp32-rounded filter table multiplied out in float64.  Written from the header's
text, not from the kernel (csrc/qk_wave_aug.hip) and not from qcnn_amd.functional.speed_perturb_tables.
"""
import math

import numpy as np

from specaug_ref import randint, u

PLAN_WORDS = 4
DEFAULT_SPEEDS = ((9, 10), (1, 1), (11, 10))


def half_width(p, q, zeros=6, rolloff=0.99):
    """Kw of speed p / q; 0 when p == q (no filter)."""
    if p == q:
        return 0
    return int(math.ceil(zeros / (rolloff * min(1.0, q / p))))


def table(p, q, zeros=6, rolloff=0.99):
    """T[r][j + Kw] for r in [0, q), j in [-Kw, Kw + 1]: float64, rounded once to float32."""
    fc = rolloff * min(1.0, q / p)
    kw = half_width(p, q, zeros, rolloff)
    out = np.zeros((q, 2 * kw + 2), dtype=np.float64)
    for r in range(q):
        for j in range(-kw, kw + 2):
            t = fc * (r / q - j)
            if abs(t) < zeros:
                sinc = 1.0 if t == 0 else math.sin(math.pi * t) / (math.pi * t)
                out[r, j + kw] = fc * sinc * math.cos(math.pi * t / (2 * zeros)) ** 2
    return out.astype(np.float32)


def out_length(n, p, q):
    return -((-n * q) // p)                                        # ceil(n q / p)


def out_samples(max_samples, speeds=DEFAULT_SPEEDS):
    return max(out_length(max_samples, p, q) for p, q in speeds)


def gain_of(b, gain=(1.0, 1.0), seed=0, counter=0):
    """g as float32: the difference, the product and the sum each rounded once."""
    lo, hi = np.float32(gain[0]), np.float32(gain[1])
    f = np.float32(u(seed, counter, b, 65) >> 8) * np.float32(2.0 ** -24)
    return np.float32(lo + np.float32(np.float32(hi - lo) * f))


def plan_row(b, length, max_samples, speeds=DEFAULT_SPEEDS, gain=(1.0, 1.0), seed=0, counter=0):
    """(n, i, n', g as float32) of utterance b."""
    n = min(max(int(length), 0), max_samples)
    i = randint(seed, counter, b, 64, len(speeds))
    p, q = speeds[i]
    return n, i, out_length(n, p, q), gain_of(b, gain, seed, counter)


def resample_row(x, n, p, q, g, width, zeros=6, rolloff=0.99):
    """One utterance: x its input row (any numeric dtype; samples >= n are never touched), g the gain (a float32).
    Returns (y, S), float64 of length `width`: y[m] = g sum_j T[r][j] x[i0 + j] and S[m] = g sum_j |T[r][j] x[i0 + j]| for m < n',
    both 0 from n' on."""
    y = np.zeros(width, dtype=np.float64)
    S = np.zeros(width, dtype=np.float64)
    np_ = out_length(n, p, q)
    assert np_ <= width
    g = float(g)
    xv = np.asarray(x[:n], dtype=np.float64)
    if p == q:
        y[:n] = g * xv
        S[:n] = np.abs(g * xv)
        return y, S
    kw = half_width(p, q, zeros, rolloff)
    T = table(p, q, zeros, rolloff).astype(np.float64)
    xp = np.concatenate([np.zeros(kw), xv, np.zeros(kw + 2)])      # xp[e + kw] = x[e], zero outside [0, n)
    m = np.arange(np_, dtype=np.int64)
    i0, r = (m * p) // q, (m * p) % q
    assert np_ == 0 or i0.max() <= n - 1
    taps = 2 * kw + 2
    prod = T[r] * xp[i0[:, None] + np.arange(taps)[None, :]]       # column j + kw: x[i0 + j]
    y[:np_] = g * prod.sum(axis=1)
    S[:np_] = g * np.abs(prod).sum(axis=1)
    return y, S


def speed_perturb(x, lengths, speeds=DEFAULT_SPEEDS, gain=(1.0, 1.0), zeros=6, rolloff=0.99, seed=0, counter=0, gains=None, width=None):
    """x (B, max_samples) -> dict: y and S (B, out_samples) float64, out_lengths (B,), plan as the lists n, i, n1, g (float32).
    gains: per-utterance float32 gains to use instead of the drawn ones (the device's, when a test bounds the device's values)."""
    x = np.asarray(x)
    B, n_max = x.shape
    width = out_samples(n_max, speeds) if width is None else width
    y = np.zeros((B, width))
    S = np.zeros((B, width))
    rows = [plan_row(b, lengths[b], n_max, speeds, gain, seed, counter) for b in range(B)]
    for b, (n, i, n1, g) in enumerate(rows):
        p, q = speeds[i]
        y[b], S[b] = resample_row(x[b], n, p, q, g if gains is None else gains[b], width, zeros, rolloff)
    return dict(y=y, S=S, out_lengths=np.array([r[2] for r in rows], dtype=np.int64), n=[r[0] for r in rows], i=[r[1] for r in rows],
                n1=[r[2] for r in rows], g=np.array([r[3] for r in rows], dtype=np.float32))
