"""Float64 restatement of include/qk_attn.h: quaternion multi-head self-attention, forward and hand-written backward, with `lengths`
and the rounding points of the header switchable per dtype.

kind = None      no rounding: the definition
kind = 'bf16'    the rounding points of the header, to bfloat16: p before p v and p^T do, dS before dS k and dS^T q, and o, dq, dk,
                 dv when they are written (lse and delta stay as they are: fp32 in the kernels)
kind = 'fp16'    the same, to float16

q, k, v, do are (B, T, 4Q), component-major r|i|j|k: component c, unit u at column c * Q + u; Q = heads * dq and head h owns units
h * dq .. h * dq + dq - 1 of every component.  A torch (autograd) restatement without rounding points serves the layer / model
composition tests.
"""
import numpy as np
import torch

from qlnorm_ref import rnd


def heads_of(x, heads):
    """(B, T, 4Q) -> (B, H, T, 4 dq): a head's vector is its four runs of dq columns, component-major."""
    b, t, w = x.shape
    dq = w // 4 // heads
    return x.reshape(b, t, 4, heads, dq).transpose(0, 3, 1, 2, 4).reshape(b, heads, t, 4 * dq)


def rows_of(xh):
    """The inverse of heads_of: (B, H, T, 4 dq) -> (B, T, 4Q)."""
    b, h, t, d = xh.shape
    return xh.reshape(b, h, t, 4, d // 4).transpose(0, 2, 3, 1, 4).reshape(b, t, h * d)


def scores(q, k, heads, scale=None):
    """(B, H, T, T) float64 scale * <q_t, k_t'>, no mask: what the overflow test counts."""
    qh, kh = heads_of(np.asarray(q, dtype=np.float64), heads), heads_of(np.asarray(k, dtype=np.float64), heads)
    return (1.0 / np.sqrt(qh.shape[-1]) if scale is None else scale) * np.einsum('bhtd,bhsd->bhts', qh, kh)


def qattention(q, k, v, heads, lengths=None, scale=None, kind=None, do=None):
    """The reference of functional.qattention.  Inputs are taken as given (round 16-bit inputs beforehand); rows t >= lengths[b] are
    never read.  Returns dict(o, lse (B, H, T), p (B, H, T, T)) and, when do is given, dq, dk, dv, delta."""
    q, k, v = (np.asarray(a, dtype=np.float64) for a in (q, k, v))
    bsz, steps, width = q.shape
    n = np.full(bsz, steps) if lengths is None else np.asarray(lengths)
    act = np.arange(steps)[None, :] < n[:, None]                                  # (B, T)
    pair = act[:, None, :, None] & act[:, None, None, :]                          # (B, 1, T, T): query and key both active
    zero = lambda a: np.where(act[:, :, None], a, 0.0)                            # inactive rows are never read: NaN there is dropped
    qh, kh, vh = (heads_of(zero(a), heads) for a in (q, k, v))
    sc = 1.0 / np.sqrt(qh.shape[-1]) if scale is None else float(scale)
    s = np.where(pair, sc * np.einsum('bhtd,bhsd->bhts', qh, kh), -np.inf)
    m = np.where(act[:, None, :], s.max(axis=-1), 0.0)                            # always subtracted
    e = np.where(pair, np.exp(s - m[..., None]), 0.0)
    l = e.sum(axis=-1)
    lse = np.where(act[:, None, :], m + np.log(np.where(l > 0, l, 1.0)), 0.0)
    p = e / np.where(l > 0, l, 1.0)[..., None]
    o = zero(rnd(rows_of(np.einsum('bhts,bhsd->bhtd', rnd(p, kind), vh)), kind))
    out = dict(o=o, lse=lse, p=p)
    if do is None:
        return out
    gh, oh = heads_of(zero(np.asarray(do, dtype=np.float64)), heads), heads_of(o, heads)
    delta = (gh * oh).sum(axis=-1)                                                # (B, H, T)
    dv = np.einsum('bhts,bhtd->bhsd', rnd(p, kind), gh)
    ds = rnd(p * (np.einsum('bhtd,bhsd->bhts', gh, vh) - delta[..., None]) * sc, kind)
    out.update(dq=zero(rnd(rows_of(np.einsum('bhts,bhsd->bhtd', ds, kh)), kind)),
               dk=zero(rnd(rows_of(np.einsum('bhts,bhtd->bhsd', ds, qh)), kind)), dv=zero(rnd(rows_of(dv), kind)), delta=delta)
    return out


def split_packed(qkv):
    """(B, T, 12Q) with q | k | v inside every component -> q, k, v (B, T, 4Q) each (numpy or torch)."""
    b, t, w = qkv.shape
    x = qkv.reshape(b, t, 4, 3, w // 12)
    return tuple(x[:, :, :, g, :].reshape(b, t, w // 3) for g in range(3))


def merge_packed(q, k, v):
    """The inverse of split_packed (numpy)."""
    b, t, w = q.shape
    return np.stack([a.reshape(b, t, 4, w // 4) for a in (q, k, v)], axis=3).reshape(b, t, 3 * w)


def qattention_t(q, k, v, heads, lengths=None, scale=None):
    """torch restatement with autograd: q, k, v (B, T, 4Q) tensors, lengths (B,) tensor or None."""
    b, t, w = q.shape
    dq = w // 4 // heads
    split = lambda x: x.reshape(b, t, 4, heads, dq).permute(0, 3, 1, 2, 4).reshape(b, heads, t, 4 * dq)
    act = torch.ones(b, t, dtype=torch.bool) if lengths is None else torch.arange(t)[None, :] < lengths.reshape(-1, 1)
    zero = lambda x: torch.where(act[:, :, None], x, torch.zeros((), dtype=x.dtype))
    qh, kh, vh = split(zero(q)), split(zero(k)), split(zero(v))
    sc = 1.0 / float(np.sqrt(4 * dq)) if scale is None else float(scale)
    s = sc * qh @ kh.transpose(-1, -2)
    s = torch.where(act[:, None, None, :], s, torch.full((), -1e300, dtype=s.dtype))
    p = torch.where(act[:, None, None, :] & act[:, None, :, None], torch.softmax(s, dim=-1), torch.zeros((), dtype=s.dtype))
    o = (p @ vh).reshape(b, heads, t, 4, dq).permute(0, 2, 3, 1, 4).reshape(b, t, w)
    return zero(o)
