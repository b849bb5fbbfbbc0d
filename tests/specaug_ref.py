"""NumPy restatement of the SpecAugment semantics in include/qk.h ("SpecAugment"): Python integers for the draws and the warp's
index arithmetic, float64 for the interpolation.  Written from the header's text, not from the kernel (csrc/qk_specaug.hip).
"""
import numpy as np

MAX_MASKS = 8
PLAN_WORDS = 36
M32 = 0xFFFFFFFF


def fmix(h):
    h &= M32
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & M32
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & M32
    h ^= h >> 16
    return h


def u(seed, counter, b, k):
    key = (seed + 0x9E3779B1 * counter) & M32
    return fmix(fmix((key + b) & M32) ^ ((k * 0x9E3779B1 + 0x7F4A7C15) & M32))


def randint(seed, counter, b, k, m):
    assert m >= 1
    return (u(seed, counter, b, k) * m) >> 32


def plan_row(b, length, rows, frames, time_warp=0, freq_masks=0, freq_width=0, time_masks=0, time_width=0, time_ratio=1.0, fill=0.0,
             seed=0, counter=0):
    """The 36 integers {n, c, w, 0, (f0, fw) x 8, (t0, tw) x 8} of utterance b."""
    n = min(max(int(length), 0), frames)
    W = time_warp
    c = w = 0
    if W >= 1 and n >= 2 * W + 3:
        c = W + 1 + randint(seed, counter, b, 0, n - 2 * W - 2)
        w = randint(seed, counter, b, 1, 2 * W + 1) - W
    row = [n, c, w, 0]
    for i in range(MAX_MASKS):
        f0 = fw = 0
        if i < freq_masks:
            fw = randint(seed, counter, b, 2 + 2 * i, min(freq_width, rows) + 1)
            f0 = randint(seed, counter, b, 3 + 2 * i, rows - fw + 1)
        row += [f0, fw]
    for i in range(MAX_MASKS):
        t0 = tw = 0
        if i < time_masks:
            cap = min(time_width, int(np.floor(np.float32(n) * np.float32(time_ratio))))       # one fp32 product
            tw = randint(seed, counter, b, 18 + 2 * i, cap + 1)
            t0 = randint(seed, counter, b, 19 + 2 * i, n - tw + 1)
        row += [t0, tw]
    return row


def plan(lengths, rows, frames, **policy):
    return np.array([plan_row(b, n, rows, frames, **policy) for b, n in enumerate(lengths)], dtype=np.int64).reshape(-1, PLAN_WORDS)


def warp_index(n, c, w):
    """(i0, r, den) per output frame t < n: source position i0 + r / den, exact integers.  c = 0: the identity."""
    i0 = np.arange(n, dtype=np.int64)
    r = np.zeros(n, dtype=np.int64)
    den = np.ones(n, dtype=np.int64)
    if c == 0:
        return i0, r, den
    cp = c + w
    assert 1 <= cp <= n - 2
    for t in range(n):
        if t <= cp:
            num, d = t * c, cp
        else:
            num, d = c * (n - 1 - cp) + (t - cp) * (n - 1 - c), n - 1 - cp
        i0[t], r[t], den[t] = num // d, num % d, d
    return i0, r, den


def masks_of(row, rows, frames):
    """(rows,) and (frames,) bool: the rows / frames a plan row masks."""
    fm = np.zeros(rows, dtype=bool)
    tm = np.zeros(frames, dtype=bool)
    for i in range(MAX_MASKS):
        f0, fw = row[4 + 2 * i], row[5 + 2 * i]
        fm[f0:f0 + fw] = True
        t0, tw = row[20 + 2 * i], row[21 + 2 * i]
        tm[t0:t0 + tw] = True
    return fm, tm


def spec_augment(x, lengths, **policy):
    """x (B, planes, rows, frames) -> dict of arrays of x's shape (and the plan):
        y       the float64 result (interpolation in float64 on the float64 image of x)
        masked  cells that hold `fill`
        exact   cells whose value is an input value unchanged (r = 0, no warp, or padding t >= n)
        bound   max(|x[i0]|, |x[i0 + 1]|) of interpolated cells
        plan    (B, 36)"""
    x = np.asarray(x, dtype=np.float64)
    B, P, R, T = x.shape
    fill = float(np.float32(policy.get('fill', 0.0)))
    pl = plan(lengths, R, T, **policy)
    y = x.copy()
    masked = np.zeros(x.shape, dtype=bool)
    exact = np.ones(x.shape, dtype=bool)
    bound = np.zeros(x.shape)
    for b in range(B):
        n, c, w = (int(v) for v in pl[b, :3])
        if n == 0:
            continue
        i0, r, den = warp_index(n, c, w)
        i1 = np.minimum(i0 + 1, n - 1)
        frac = r / den                                            # float64: the kernel's fp32 quotient is inside the tests' bound
        xb = x[b]
        a, bb = xb[:, :, i0], xb[:, :, i1]                        # (P, R, n)
        y[b, :, :, :n] = np.where(r == 0, a, a + frac * (bb - a))
        exact[b, :, :, :n] = (r == 0)
        bound[b, :, :, :n] = np.maximum(np.abs(a), np.abs(bb))
        fm, tm = masks_of(pl[b], R, T)
        m = fm[:, None] | tm[None, :]
        m[:, n:] = False
        masked[b] = m[None]
        y[b][masked[b]] = fill
    return dict(y=y, masked=masked, exact=exact & ~masked, bound=bound, plan=pl)
