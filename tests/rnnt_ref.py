"""Float64 numpy restatement of include/qk_rnnt.h (the transducer loss and its fused log-softmax gradient), the brute-force sum over
every alignment it is checked against, and the bounds of tests/test_rnnt.py.

BOUNDS.  The GPU tests compare the kernel with rnnt(...) of THE SAME operands: the logits are rounded to the kernel's dtype before
either side sees them, so the only rounding point between the two is the one the header names -- the stored gradient, rounded once
to the logits' dtype.  Rounding to nearest moves an entry g by at most half a unit in its last place, 2^-p |g| with p significand
bits: 2^-8 |g| = 3.9e-3 |g| in bf16 (p = 8) and 2^-11 |g| = 4.9e-4 |g| in fp16 (p = 11), so at most that share of the largest entry.
Both are below half of the 16-bit bounds of tests/test_ctc_enum.py (1e-2 and 2e-3), which are therefore kept
(test_rounding_points_stay_under_half_the_16_bit_bound measures it on the GPU cases' operands):

    cost      2e-5 relative                      (fp32 arithmetic everywhere: the cost has no 16-bit rounding point)
    gradient  5e-4 (fp32), 1e-2 (bf16), 2e-3 (fp16) of the largest entry

The rest of the 16-bit bounds is for the fp32 arithmetic in front of the rounding: alpha + beta - ll is a difference of numbers of
the size of the cost (up to ~400 in the cases here, half a unit in the last place 1.5e-5), formed after T + U dependent steps.
"""
import numpy as np

COST_BOUND = 2e-5
GRAD_BOUND = {None: 5e-4, 'bf16': 1e-2, 'fp16': 2e-3}


def rnd(a, kind):
    """Round float64 values to bf16 / fp16 (nearest even), back in float64; kind None: to float32."""
    a = np.asarray(a, dtype=np.float64)
    if kind == 'fp16':
        return a.astype(np.float16).astype(np.float64)
    f = a.astype(np.float32)
    if kind is None:
        return f.astype(np.float64)
    assert kind == 'bf16'
    u = f.view(np.uint32).astype(np.uint64)
    nan = np.isnan(f)
    u = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    out = u.astype(np.uint32).view(np.float32).astype(np.float64)
    out[nan] = np.nan
    return out


def _lae(a, b):
    m = np.maximum(a, b)
    if m == -np.inf:
        return -np.inf
    return m + np.log1p(np.exp(np.minimum(a, b) - m))


def log_softmax(x):
    m = x.max(axis=-1, keepdims=True)
    return x - (m + np.log(np.exp(x - m).sum(axis=-1, keepdims=True)))


def rnnt_row(logits, labels, tb, ub):
    """One batch row: logits (T, U1, V) float64, labels (Lmax,), clamped lengths.  Returns (cost, grad (T, U1, V), alpha, beta); an
    infeasible row gives (+inf, zeros, None, None)."""
    t_max, u1, v = logits.shape
    blank = v - 1
    grad = np.zeros_like(logits)
    lab = [int(x) for x in labels[:ub]]
    if tb == 0 or any(x < 0 or x > v - 2 for x in lab):
        return np.inf, grad, None, None
    with np.errstate(invalid='ignore'):
        lp = np.full((tb, ub + 1, v), -np.inf)
        lp[:] = log_softmax(logits[:tb, :ub + 1])                      # inactive cells are never read
    alpha = np.full((tb, ub + 1), -np.inf)
    beta = np.full((tb, ub + 1), -np.inf)
    for t in range(tb):
        for u in range(ub + 1):
            if t == 0 and u == 0:
                alpha[t, u] = 0.0
                continue
            a = alpha[t - 1, u] + lp[t - 1, u, blank] if t > 0 else -np.inf
            b = alpha[t, u - 1] + lp[t, u - 1, lab[u - 1]] if u > 0 else -np.inf
            alpha[t, u] = _lae(a, b)
    for t in range(tb - 1, -1, -1):
        for u in range(ub, -1, -1):
            if t == tb - 1 and u == ub:
                beta[t, u] = lp[t, u, blank]
                continue
            a = beta[t + 1, u] + lp[t, u, blank] if t < tb - 1 else -np.inf
            b = beta[t, u + 1] + lp[t, u, lab[u]] if u < ub else -np.inf
            beta[t, u] = _lae(a, b)
    ll = beta[0, 0]
    for t in range(tb):
        for u in range(ub + 1):
            g = np.exp(alpha[t, u] + beta[t, u] + lp[t, u] - ll)
            nb = beta[t + 1, u] if t < tb - 1 else (0.0 if u == ub else -np.inf)
            g[blank] -= np.exp(alpha[t, u] + lp[t, u, blank] + nb - ll)
            if u < ub:
                g[lab[u]] -= np.exp(alpha[t, u] + lp[t, u, lab[u]] + beta[t, u + 1] - ll)
            grad[t, u] = g
    return -ll, grad, alpha, beta


def rnnt(logits, labels, input_length, label_length, grad_kind='none'):
    """The header, batched: logits (B, T, U1, V), labels (B, Lmax), lengths (B,).  Returns (cost (B,), grad (B, T, U1, V)).
    grad_kind 'bf16' / 'fp16' / None (float32) applies the header's one rounding point to the gradient; 'none' keeps float64."""
    logits = np.asarray(logits, dtype=np.float64)
    b, t_max, u1, _ = logits.shape
    cost, grad = np.zeros(b), np.zeros_like(logits)
    for i in range(b):
        tb = int(np.clip(input_length[i], 0, t_max))
        ub = int(np.clip(label_length[i], 0, u1 - 1))
        cost[i], grad[i], _, _ = rnnt_row(logits[i], np.asarray(labels)[i] if u1 > 1 else np.zeros(0, dtype=np.int64), tb, ub)
    if grad_kind != 'none':
        grad = rnd(grad, grad_kind)
    return cost, grad


def enumerate_cost(logits, labels):
    """-log of the sum over EVERY alignment of one full row: logits (T, U + 1, V), labels (U,).  An alignment is a monotone walk
    from (0, 0) that emits label[u] (u -> u + 1) or blank (t -> t + 1) and ends with the blank out of (T - 1, U)."""
    logits = np.asarray(logits, dtype=np.float64)
    t_max, u1, v = logits.shape
    lp = log_softmax(logits)
    lab = [int(x) for x in labels]
    assert len(lab) == u1 - 1

    total = [0.0]

    def walk(t, u, acc):
        if t == t_max - 1 and u == u1 - 1:
            total[0] += np.exp(acc + lp[t, u, v - 1])
            return
        if t < t_max - 1:
            walk(t + 1, u, acc + lp[t, u, v - 1])
        if u < u1 - 1:
            walk(t, u + 1, acc + lp[t, u, lab[u]])
    walk(0, 0, 0.0)
    return -np.log(total[0])


def central_differences(logits, labels, eps=1e-5):
    """d enumerate_cost / d logits by central differences."""
    x = np.array(logits, dtype=np.float64)
    g = np.zeros_like(x)
    flat, gflat = x.reshape(-1), g.reshape(-1)
    for k in range(flat.size):
        keep = flat[k]
        flat[k] = keep + eps
        up = enumerate_cost(x, labels)
        flat[k] = keep - eps
        gflat[k] = (up - enumerate_cost(x, labels)) / (2 * eps)
        flat[k] = keep
    return g
