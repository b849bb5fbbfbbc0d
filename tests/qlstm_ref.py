"""Float64 restatement of include/qk_rnn.h: the quaternion LSTM recurrence, forward and hand-written back-propagation through
time, with `directions`, `lengths` and the rounding points of the header switchable per dtype.

kind = None      no rounding: the definition
kind = 'bf16'    the four rounding points of the header, to bfloat16   (R once; h_t once per step; dz_t once; dh0)
kind = 'fp16'    the same, to float16

Layouts are the header's: states (D, B, U) component-major r|i|j|k; the 4U gate columns component-major blocks of U, gate-major
i|f|g|o inside; y (B, T, D * U) with component c, direction d, unit u at column c * (D * Q) + d * Q + u.  A torch (autograd)
restatement of the forward without rounding points serves the layer / model composition tests.
"""
import numpy as np
import torch

# sign of gathered component a (row block) in produced component b (column block) of the dense table conj(W) (x) x, the table
# oracle/ref_port.py:expand_kernel(conj=True) builds; the compact part is a ^ b
_CONV_SIGN = ((1, 1, 1, 1), (-1, 1, 1, -1), (-1, -1, 1, 1), (-1, 1, -1, 1))
_TORCH = {'bf16': torch.bfloat16, 'fp16': torch.float16}


def sign(a, b):
    return _CONV_SIGN[b][a]


def rnd(x, kind):
    """x rounded to the activation type (through float32, as the kernels hold it) and back to float64."""
    if kind is None:
        return np.asarray(x, dtype=np.float64)
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(_TORCH[kind]).double().numpy()


def expand(w):
    """compact (K, 4F) -> real (4K, 4F) matrix of quaternion_dense: y = x @ expand(w)."""
    k, f = w.shape[0], w.shape[1] // 4
    e = np.zeros((4 * k, 4 * f))
    for a in range(4):
        for b in range(4):
            e[a * k:(a + 1) * k, b * f:(b + 1) * f] = sign(a, b) * w[:, (a ^ b) * f:((a ^ b) + 1) * f]
    return e


def fold(de):
    """gradient of expand: real (4K, 4F) -> compact (K, 4F)."""
    k, f = de.shape[0] // 4, de.shape[1] // 4
    dw = np.zeros((k, 4 * f))
    for a in range(4):
        for b in range(4):
            dw[:, (a ^ b) * f:((a ^ b) + 1) * f] += sign(a, b) * de[a * k:(a + 1) * k, b * f:(b + 1) * f]
    return dw


def quaternion_dense(x, w, bias=None):
    y = x @ expand(w)
    return y if bias is None else y + bias


def _sig(z):
    return 1.0 / (1.0 + np.exp(-z))


def _gates(z, q):
    """z (B, 4U) -> i, f, g, o, each (B, U) in the state layout."""
    b = z.shape[0]
    z4 = z.reshape(b, 4, 4, q)
    flat = lambda g: z4[:, :, g, :].reshape(b, 4 * q)
    return _sig(flat(0)), _sig(flat(1)), np.tanh(flat(2)), _sig(flat(3))


def _ungates(di, df, dg, do, q):
    b = di.shape[0]
    return np.stack([v.reshape(b, 4, q) for v in (di, df, dg, do)], axis=2).reshape(b, 16 * q)


def _order(steps, reverse):
    return list(range(steps - 1, -1, -1)) if reverse else list(range(steps))


def forward_dir(zx, r, lengths, h0, c0, reverse=False, kind=None):
    """One direction.  zx (B, T, 4U), r (Q, 4U), lengths (B,) ints, h0 / c0 (B, U).  Returns y (B, T, U), hT, cT, tape."""
    bsz, steps, g = zx.shape
    u = g // 4
    q = u // 4
    e = expand(rnd(r, kind))
    h, c = np.array(h0, dtype=np.float64), np.array(c0, dtype=np.float64)
    y = np.zeros((bsz, steps, u))
    tape = {}
    for t in _order(steps, reverse):
        act = (t < np.asarray(lengths))[:, None]
        gi, gf, gg, go = _gates(zx[:, t] + h @ e, q)
        c_new = gf * c + gi * gg
        h_new = rnd(go * np.tanh(c_new), kind)
        tape[t] = (h, c, gi, gf, gg, go, c_new, act)
        y[:, t] = np.where(act, h_new, 0.0)
        h, c = np.where(act, h_new, h), np.where(act, c_new, c)
    return y, h, c, (e, tape, reverse, kind, q)


def backward_dir(tape_all, dy, dhT, dcT):
    """Back-propagation through time of forward_dir.  Returns dzx (B, T, 4U), dR (Q, 4U), dh0, dc0, hprev (B, T, U)."""
    e, tape, reverse, kind, q = tape_all
    bsz, steps, u = dy.shape
    dh, dc = np.array(dhT, dtype=np.float64), np.array(dcT, dtype=np.float64)
    dzx, de, hprev = np.zeros((bsz, steps, 4 * u)), np.zeros_like(e), np.zeros((bsz, steps, u))
    for t in reversed(_order(steps, reverse)):
        h_prev, c_prev, gi, gf, gg, go, c_new, act = tape[t]
        dh_t = dh + dy[:, t]
        tc = np.tanh(c_new)
        dc_t = dc + dh_t * go * (1 - tc * tc)
        dz = _ungates(dc_t * gg * gi * (1 - gi), dc_t * c_prev * gf * (1 - gf), dc_t * gi * (1 - gg * gg), dh_t * tc * go * (1 - go), q)
        dz = np.where(act, rnd(dz, kind), 0.0)
        dzx[:, t] = dz
        hprev[:, t] = np.where(act, h_prev, 0.0)
        de += h_prev.T @ dz
        dh, dc = np.where(act, dz @ e.T, dh), np.where(act, dc_t * gf, dc)
    return dzx, fold(de), rnd(dh, kind), dc, hprev


def _merge(parts, q):
    """[(B, ..., U) per direction] -> (B, ..., D * U) in the quaternion-concatenated layout."""
    d = len(parts)
    lead = parts[0].shape[:-1]
    return np.stack([p.reshape(lead + (4, q)) for p in parts], axis=-2).reshape(lead + (4 * d * q,))


def _split(x, d, q):
    lead = x.shape[:-1]
    x5 = x.reshape(lead + (4, d, q))
    return [x5[..., k, :].reshape(lead + (4 * q,)) for k in range(d)]


def qlstm(zx, r, lengths=None, h0=None, c0=None, reverse=False, kind=None, dy=None, dhT=None, dcT=None):
    """The reference of functional.qlstm.  zx (D, B, T, 4U), r (D, Q, 4U), h0 / c0 / dhT / dcT (D, B, U) or None, dy (B, T, D * U) or
    None.  Inputs are taken as given (round 16-bit inputs beforehand).  Returns dict(y, hT, cT) and, when any of dy / dhT / dcT is
    given, dzx, dR, dh0, dc0, hprev."""
    zx, r = np.asarray(zx, dtype=np.float64), np.asarray(r, dtype=np.float64)
    dirs, bsz, steps, g = zx.shape
    u = g // 4
    q = u // 4
    lengths = np.full(bsz, steps) if lengths is None else np.asarray(lengths)
    zero = np.zeros((dirs, bsz, u))
    h0, c0 = (zero if h0 is None else np.asarray(h0, dtype=np.float64)), (zero if c0 is None else np.asarray(c0, dtype=np.float64))
    ys, hs, cs, tapes = [], [], [], []
    for d in range(dirs):
        y, h, c, tape = forward_dir(zx[d], r[d], lengths, h0[d], c0[d], reverse or d == 1, kind)
        ys.append(y); hs.append(h); cs.append(c); tapes.append(tape)
    out = dict(y=_merge(ys, q), hT=np.stack(hs), cT=np.stack(cs))
    if dy is None and dhT is None and dcT is None:
        return out
    dy = np.zeros((bsz, steps, dirs * u)) if dy is None else np.asarray(dy, dtype=np.float64)
    dhT, dcT = (zero if dhT is None else np.asarray(dhT, dtype=np.float64)), (zero if dcT is None else np.asarray(dcT, dtype=np.float64))
    res = [backward_dir(tapes[d], dyd, dhT[d], dcT[d]) for d, dyd in enumerate(_split(dy, dirs, q))]
    for i, name in enumerate(('dzx', 'dR', 'dh0', 'dc0', 'hprev')):
        out[name] = np.stack([x[i] for x in res])
    return out


# ---- torch float64 restatement (autograd), no rounding points: the layer and the model as compositions ---------------------------
def expand_t(w):
    k, f = w.shape[0], w.shape[1] // 4
    cols = []
    for b in range(4):
        cols.append(torch.cat([sign(a, b) * w[:, (a ^ b) * f:((a ^ b) + 1) * f] for a in range(4)], dim=0))
    return torch.cat(cols, dim=1)


def qlstm_t(zx, r, lengths, reverse=False):
    """One direction in torch: zx (B, T, 4U), r (Q, 4U), lengths (B,) tensor or None; zero initial state.  Returns y (B, T, U)."""
    bsz, steps, g = zx.shape
    u = g // 4
    q = u // 4
    e = expand_t(r)
    h = c = zx.new_zeros((bsz, u))
    ys = [None] * steps
    for t in _order(steps, reverse):
        act = (t < lengths).reshape(-1, 1) if lengths is not None else torch.ones((bsz, 1), dtype=torch.bool)
        z4 = (zx[:, t] + h @ e).reshape(bsz, 4, 4, q)
        gi, gf, gg, go = (z4[:, :, k, :].reshape(bsz, u) for k in range(4))
        gi, gf, gg, go = torch.sigmoid(gi), torch.sigmoid(gf), torch.tanh(gg), torch.sigmoid(go)
        c_new = gf * c + gi * gg
        h_new = go * torch.tanh(c_new)
        ys[t] = torch.where(act, h_new, torch.zeros_like(h_new))
        h, c = torch.where(act, h_new, h), torch.where(act, c_new, c)
    return torch.stack(ys, dim=1)


def layer_t(x, kernel, recurrent, bias, lengths, go_backwards=False):
    """QuaternionLSTM(return_sequences=True) in torch float64.  x (B, T, 4 in_q); weights (in_q, 4U) / (Q, 4U) / (4U,) or, with a
    leading axis of 2, the bidirectional layer.  Returns (B, T, D * U)."""
    bsz, steps, _ = x.shape
    stacked = kernel.dim() == 3
    dirs = kernel.shape[0] if stacked else 1
    ys = []
    for d in range(dirs):
        k, r, b = (kernel[d], recurrent[d], bias[d]) if stacked else (kernel, recurrent, bias)
        zx = (x.reshape(bsz * steps, -1) @ expand_t(k) + b).reshape(bsz, steps, -1)
        ys.append(qlstm_t(zx, r, lengths, reverse=go_backwards or d == 1))
    q = ys[0].shape[-1] // 4
    return torch.stack([y.reshape(bsz, steps, 4, q) for y in ys], dim=3).reshape(bsz, steps, 4 * dirs * q)
