"""Float64 restatement of include/qk_dwconv.h: the depthwise quaternion convolution over time with an optional GLU gate in front,
forward and hand-written backward, with `lengths` and the rounding points of the header switchable per dtype.

kind = None      no rounding: the definition
kind = 'bf16'    the three rounding points of the header, to bfloat16   (y, da and dg when they are written; h stays fp32)
kind = 'fp16'    the same, to float16

a, g, y, dy are (B, T, 4Q), component-major r|i|j|k: component c, unit u at column c * Q + u; w is (K, 4Q) the same way per tap.  A
torch (autograd) restatement without rounding points, and the Conformer block built from it and from qlnorm_ref / qattn_ref /
qlstm_ref, serve the layer / model composition tests.
"""
import numpy as np
import torch

import qattn_ref as AR
import qlnorm_ref as NR
import qlstm_ref as LR
from qlnorm_ref import rnd

# p (x) q, the Hamilton product: component c of the result is sum_m SIGN[c][m] * p[m] * q[IDX[c][m]]
IDX = ((0, 1, 2, 3), (1, 0, 3, 2), (2, 3, 0, 1), (3, 2, 1, 0))
SIGN = ((1, -1, -1, -1), (1, 1, 1, -1), (1, -1, 1, 1), (1, 1, -1, 1))


def hamilton(p, q):
    """p (x) q with the four components on axis -2 (numpy or torch; the other axes broadcast)."""
    rows = [sum(SIGN[c][m] * p[..., m, :] * q[..., IDX[c][m], :] for m in range(4)) for c in range(4)]
    return torch.stack(rows, dim=-2) if isinstance(rows[0], torch.Tensor) else np.stack(rows, axis=-2)


def conj(x):
    return x * (np.array([1.0, -1.0, -1.0, -1.0])[:, None] if not isinstance(x, torch.Tensor) else torch.tensor([1.0, -1.0, -1.0, -1.0], dtype=x.dtype)[:, None])


def pad_lo_of(taps, padding):
    return {'same': (taps - 1) // 2, 'causal': taps - 1}[padding]


def sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def qdwconv(a, w, bias=None, g=None, lengths=None, padding='same', kind=None, dy=None):
    """The reference of functional.qdwconv1d (g None) / qglu_dwconv1d.  Inputs are taken as given (round 16-bit inputs beforehand);
    what rows t >= lengths[b] hold is never used.  Returns dict(y, h) and, when dy is given, da, dg (None without a gate), dw, dbias."""
    a = np.asarray(a, dtype=np.float64)
    bsz, steps, width = a.shape
    q = width // 4
    w4 = np.asarray(w, dtype=np.float64).reshape(-1, 4, q)
    taps = w4.shape[0]
    lo = pad_lo_of(taps, padding)
    n = np.full(bsz, steps) if lengths is None else np.clip(np.asarray(lengths), 0, steps)
    act = (np.arange(steps)[None, :] < n[:, None])[:, :, None, None]                  # (B, T, 1, 1)
    a4 = a.reshape(bsz, steps, 4, q)
    with np.errstate(all='ignore'):
        if g is not None:
            g4 = np.asarray(g, dtype=np.float64).reshape(bsz, steps, 4, q)
            s = sigmoid(g4)
            h = np.where(act, a4 * s, 0.0)                                             # selected, never multiplied by 0
        else:
            h = np.where(act, a4, 0.0)
    hp = np.zeros((bsz, steps + taps - 1, 4, q))
    hp[:, lo:lo + steps] = h
    y = np.zeros((bsz, steps, 4, q)) + (0.0 if bias is None else np.asarray(bias, dtype=np.float64).reshape(4, q))
    for k in range(taps):
        y = y + hamilton(w4[k], hp[:, k:k + steps])
    out = dict(y=np.where(act, rnd(y, kind), 0.0).reshape(bsz, steps, width), h=h.reshape(bsz, steps, width))
    if dy is None:
        return out
    with np.errstate(all='ignore'):
        d = np.where(act, np.asarray(dy, dtype=np.float64).reshape(bsz, steps, 4, q), 0.0)
    dp = np.zeros((bsz, steps + taps - 1, 4, q))
    dp[:, taps - 1 - lo:taps - 1 - lo + steps] = d
    dh = np.zeros((bsz, steps, 4, q))
    dw = np.zeros((taps, 4, q))
    for k in range(taps):
        dh = dh + hamilton(conj(w4[k]), dp[:, taps - 1 - k:taps - 1 - k + steps])      # dy[t' + pad_lo - k]
        dw[k] = hamilton(d, conj(hp[:, k:k + steps])).sum(axis=(0, 1))
    with np.errstate(all='ignore'):
        if g is not None:
            da = np.where(act, rnd(dh * s, kind), 0.0)
            dg = np.where(act, rnd(dh * a4 * s * (1.0 - s), kind), 0.0).reshape(bsz, steps, width)
        else:
            da, dg = np.where(act, rnd(dh, kind), 0.0), None
    out.update(da=da.reshape(bsz, steps, width), dg=dg, dw=dw.reshape(taps, width), dbias=d.sum(axis=(0, 1)).reshape(width))
    return out


def split_packed(u):
    """(B, T, 8Q) with a | g inside every component -> a, g (B, T, 4Q) each (numpy or torch)."""
    b, t, w = u.shape
    x = u.reshape(b, t, 4, 2, w // 8)
    return x[:, :, :, 0, :].reshape(b, t, w // 2), x[:, :, :, 1, :].reshape(b, t, w // 2)


def merge_packed(a, g):
    """The inverse of split_packed (numpy)."""
    b, t, w = a.shape
    return np.stack([x.reshape(b, t, 4, w // 4) for x in (a, g)], axis=3).reshape(b, t, 2 * w)


# ---- torch float64 restatement (autograd), no rounding points --------------------------------------------------------------------
def qdwconv_t(a, w, bias=None, g=None, lengths=None, padding='same'):
    bsz, steps, width = a.shape
    q = width // 4
    w4 = w.reshape(-1, 4, q)
    taps = w4.shape[0]
    lo = pad_lo_of(taps, padding)
    act = torch.ones(bsz, steps, dtype=torch.bool) if lengths is None else torch.arange(steps)[None, :] < lengths.reshape(-1, 1)
    act = act[:, :, None, None]
    h = a.reshape(bsz, steps, 4, q)
    if g is not None:
        h = h * torch.sigmoid(g.reshape(bsz, steps, 4, q))
    h = torch.where(act, h, torch.zeros((), dtype=h.dtype))
    hp = torch.nn.functional.pad(h, (0, 0, 0, 0, lo, taps - 1 - lo))
    y = sum(hamilton(w4[k], hp[:, k:k + steps]) for k in range(taps))
    if bias is not None:
        y = y + bias.reshape(4, q)
    return torch.where(act, y, torch.zeros((), dtype=y.dtype)).reshape(bsz, steps, width)


def dense_t(x, w, b):
    return x @ LR.expand_t(w) + b


def mha_t(x, p, prefix, heads, lengths):
    b, t, w = x.shape
    qkv = dense_t(x.reshape(b * t, w), p[prefix + 'kernel'], p[prefix + 'bias']).reshape(b, t, -1)
    o = AR.qattention_t(*AR.split_packed(qkv), heads, lengths)
    return dense_t(o.reshape(b * t, -1), p[prefix + 'out_kernel'], p[prefix + 'out_bias']).reshape(b, t, -1)


def conv_module_t(x, p, prefix, lengths, padding='same', epsilon=1e-3):
    """QuaternionConformerConvModule: p maps parameter names (with `prefix`) to float64 tensors."""
    b, t, w = x.shape
    u = dense_t(x.reshape(b * t, w), p[prefix + 'pw1.r'], p[prefix + 'pw1.bias']).reshape(b, t, 2 * w)
    a, g = split_packed(u)
    h = qdwconv_t(a, p[prefix + 'depthwise.kernel'], p[prefix + 'depthwise.bias'], g, lengths, padding)
    h = NR.qlayer_norm_t(h, p[prefix + 'norm.gamma'], p[prefix + 'norm.beta'], lengths, epsilon=epsilon)
    return dense_t(torch.nn.functional.silu(h).reshape(b * t, w), p[prefix + 'pw2.r'], p[prefix + 'pw2.bias']).reshape(b, t, w)


def conformer_block_t(x, p, prefix, heads, lengths, padding='same', epsilon=1e-3):
    """QuaternionConformerBlock (dropout 0)."""
    b, t, w = x.shape
    qln = lambda v, name: NR.qlayer_norm_t(v, p[prefix + name + '.gamma'], p[prefix + name + '.beta'], lengths, epsilon=epsilon)

    def ff(v, tag):
        h = torch.relu(dense_t(v.reshape(b * t, w), p[prefix + tag + '_in.r'], p[prefix + tag + '_in.bias']))
        return dense_t(h, p[prefix + tag + '_out.r'], p[prefix + tag + '_out.bias']).reshape(b, t, w)
    x = x + 0.5 * ff(qln(x, 'norm_ff1'), 'ff1')
    x = x + mha_t(qln(x, 'norm_mha'), p, prefix + 'attention.', heads, lengths)
    x = x + conv_module_t(qln(x, 'norm_conv'), p, prefix + 'conv.', lengths, padding, epsilon)
    x = x + 0.5 * ff(qln(x, 'norm_ff2'), 'ff2')
    return qln(x, 'norm_out')
