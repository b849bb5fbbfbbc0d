"""float64 restatement of the scheduled optimiser step (include/qk_opt.h) for tests/test_sched_adam.py: the learning-rate schedule,
the decay of the weight EMA and one EMA update.  Written from the formulas of the header alone; it imports nothing of the package.

t is the 1-based index of a step, s = t - 1 the number of steps applied before it.
"""
import math

import numpy as np

KINDS = ('constant', 'inverse-time', 'exponential', 'cosine', 'inv-sqrt')


def warmup(t, warmup_steps):
    return min(1.0, t / float(warmup_steps)) if warmup_steps > 0 else 1.0


def factor(kind, t, warmup_steps=0, total_steps=0, decay_steps=1, rate=1.0, floor=0.0):
    s = t - 1
    if kind == 'constant':
        return 1.0
    if kind == 'inverse-time':
        return 1.0 / (1.0 + rate * s)
    if kind == 'exponential':
        return rate ** (s / float(decay_steps))
    if kind == 'cosine':
        x = (t - warmup_steps) / float(total_steps - warmup_steps)
        x = min(1.0, max(0.0, x))
        return floor + (1.0 - floor) * 0.5 * (1.0 + math.cos(math.pi * x))
    if kind == 'inv-sqrt':
        return math.sqrt(max(warmup_steps, 1) / float(max(t, warmup_steps, 1)))
    raise ValueError(kind)


def lr(kind, t, base_lr, lr_scale=1.0, **kw):
    """The rate of step t in float64 (the kernel rounds this ONCE to float32)."""
    return base_lr * warmup(t, kw.get('warmup_steps', 0)) * factor(kind, t, **kw) * lr_scale


def lr_f32(kind, t, base_lr, lr_scale=1.0, **kw):
    return np.float32(lr(kind, t, base_lr, lr_scale, **kw))


def ulp_distance(a, b):
    """Number of float32 values between two finite float32 numbers of one sign (0: equal, 1: adjacent)."""
    ia = int(np.array(a, dtype=np.float32).view(np.int32))
    ib = int(np.array(b, dtype=np.float32).view(np.int32))
    return abs(ia - ib)


def ema_decay(u, decay, warm=True):
    """Decay of EMA update u (1-based, INCLUDING this one): TensorFlow's ExponentialMovingAverage warm-up."""
    return min(decay, (1.0 + u) / (10.0 + u)) if warm else decay


def ema_update(ema_prev, p_new, d):
    """One update in float64 with the kernel's float32 coefficient omd = float32(1 - d)."""
    omd = float(np.float32(1.0 - d))
    e = np.asarray(ema_prev, dtype=np.float64)
    return e + omd * (np.asarray(p_new, dtype=np.float64) - e)
