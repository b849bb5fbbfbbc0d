"""Float64 restatement of include/qk_norm.h: quaternion layer normalisation, forward and hand-written backward, with `lengths` and
the rounding points of the header switchable per dtype.

kind = None      no rounding: the definition
kind = 'bf16'    the two rounding points of the header, to bfloat16   (y when it is written; dx when it is written)
kind = 'fp16'    the same, to float16

x is (N, 4Q) [or (B, T, 4Q) with lengths (B,)], component-major r|i|j|k: component c, unit u at column c * Q + u.  A torch
(autograd) restatement without rounding points serves the layer / model composition tests.
"""
import numpy as np
import torch

_TORCH = {'bf16': torch.bfloat16, 'fp16': torch.float16}


def rnd(x, kind):
    """x rounded to the activation type (through float32, as the kernels hold it) and back to float64."""
    if kind is None:
        return np.asarray(x, dtype=np.float64)
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(_TORCH[kind]).double().numpy()


def active_rows(shape, lengths):
    """(N,) bool: row n = b * T + t of a (B, T, 4Q) tensor is active iff t < lengths[b]; all rows without lengths."""
    n = int(np.prod(shape[:-1]))
    if lengths is None:
        return np.ones(n, dtype=bool)
    bsz, steps = shape[0], shape[1]
    assert len(shape) == 3 and len(lengths) == bsz
    return (np.arange(steps)[None, :] < np.asarray(lengths)[:, None]).reshape(n)


def qlayer_norm(x, gamma=None, beta=None, lengths=None, epsilon=1e-3, kind=None, dy=None):
    """The reference of functional.qlayer_norm.  Inputs are taken as given (round 16-bit inputs beforehand).  Returns dict(y, mu,
    rstd, xhat) and, when dy is given, dx, dgamma (Q,), dbeta (4Q,)."""
    x = np.asarray(x, dtype=np.float64)
    shape = x.shape
    width = shape[-1]
    q = width // 4
    act = active_rows(shape, lengths)
    x4 = x.reshape(-1, 4, q)
    g = np.ones(q) if gamma is None else np.asarray(gamma, dtype=np.float64)
    b = np.zeros(width) if beta is None else np.asarray(beta, dtype=np.float64)
    mu = x4.mean(axis=2, keepdims=True)                                     # (N, 4, 1)
    var = ((x4 - mu) ** 2).mean(axis=(1, 2), keepdims=True)                 # (N, 1, 1): centred, one per row
    rstd = 1.0 / np.sqrt(var + epsilon)
    xhat = (x4 - mu) * rstd
    y = g[None, None, :] * xhat + b.reshape(1, 4, q)
    y = np.where(act[:, None, None], rnd(y, kind), 0.0)
    out = dict(y=y.reshape(shape), mu=mu.reshape(-1, 4), rstd=rstd.reshape(-1), xhat=xhat.reshape(shape))
    if dy is None:
        return out
    d4 = np.asarray(dy, dtype=np.float64).reshape(-1, 4, q) * act[:, None, None]
    gg = d4 * g[None, None, :]
    m = gg.mean(axis=2, keepdims=True)
    s = (gg * xhat).mean(axis=(1, 2), keepdims=True)
    dx = rstd * (gg - m - xhat * s)
    out['dx'] = np.where(act[:, None, None], rnd(dx, kind), 0.0).reshape(shape)
    out['dgamma'] = (d4 * xhat).sum(axis=(0, 1))
    out['dbeta'] = d4.sum(axis=0).reshape(width)
    return out


def naive_variance(x, epsilon=1e-3, dtype=np.float32):
    """rstd of every row from E[x^2] - mu^2 evaluated in `dtype`: the form the header forbids (test_centred_variance shows why)."""
    x4 = np.asarray(x, dtype=dtype).reshape(-1, 4, x.shape[-1] // 4)
    mu = x4.mean(axis=2, keepdims=True, dtype=dtype)
    var = (x4 * x4).mean(axis=(1, 2), dtype=dtype) - (mu * mu).mean(axis=(1, 2), dtype=dtype)
    return 1.0 / np.sqrt(np.maximum(var, 0).astype(np.float64) + epsilon)


# ---- torch float64 restatement (autograd), no rounding points --------------------------------------------------------------------
def qlayer_norm_t(x, gamma=None, beta=None, lengths=None, epsilon=1e-3):
    """x (..., 4Q) [(B, T, 4Q) with lengths (B,) tensor]; gamma (Q,) / beta (4Q,) tensors or None."""
    shape = x.shape
    q = shape[-1] // 4
    x4 = x.reshape(-1, 4, q)
    mu = x4.mean(dim=2, keepdim=True)
    var = ((x4 - mu) ** 2).mean(dim=(1, 2), keepdim=True)
    y = (x4 - mu) / torch.sqrt(var + epsilon)
    if gamma is not None:
        y = y * gamma.reshape(1, 1, q)
    if beta is not None:
        y = y + beta.reshape(1, 4, q)
    y = y.reshape(shape)
    if lengths is not None:
        act = (torch.arange(shape[1]).reshape(1, -1) < lengths.reshape(-1, 1)).reshape(shape[0], shape[1], 1)
        y = torch.where(act, y, torch.zeros_like(y))
    return y
