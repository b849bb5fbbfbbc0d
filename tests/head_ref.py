"""TEST INFRASTRUCTURE -- float64 references of the model's head WITH THE KERNELS' ROUNDING POINTS, and a bound per output element.

The head is the softmax output layer (csrc/qk_out_layer.hip, and the composition it replaced: a library GEMM plus
k_softmax_rows_* of csrc/qk_aux.hip), the bench's weighted-sum loss (k_weighted_sum) and the CTC cost (csrc/qk_ctc.hip).  exp and log
are inexact, so the zero-tolerance lattice of tests/lattice_ref.py cannot reach them.  The next strongest thing: every reference
below computes in float64 and rounds to the 16-bit type (round-to-nearest-even, ONE rounding from float64) exactly where the kernel
stores or stages 16 bits; every function returns `(reference, bound)`, `bound` of the output's shape, a sum of named terms, and
`assert_within` holds EVERY element to its own bound.  numpy and torch on the CPU only; nothing here touches a device.

Notation.  u32 = 2^-24.  ulp16(v) = the spacing of the 16-bit type at |v|; half_ulp(v) = ulp16(v) / 2 is what ONE correct 16-bit
store may move v by.  (As a relative figure half an ulp runs from 2^-9 at the top of a bf16 binade to 2^-8 at its bottom -- 2^-12 to
2^-11 for fp16 -- so a bound of 2^-9 |v| / 2^-12 |v| would fail a correctly rounded store in most of every binade; the store terms
below therefore use half_ulp(v) itself, which is never wider than the format's unit roundoff 2^-8 / 2^-11 times |v| and includes the
subnormal spacing of fp16, 2^-25 as half an ulp.)

Rounding points, as read from the kernels
-----------------------------------------
k_dense_softmax_fwd   * the fp32 master kernel is converted to 16 bits (W16) before the MFMAs (pack2o into the LDS tile wt);
                      * the accumulators start at the fp32 bias and stay fp32 through max / __expf / sum / reciprocal / multiply;
                      * y is stored in 16 bits (pack2o / from_f32 at the stores).
k_dense_softmax_bwd   * W16 as above (pack2o into the register fragments wf);
                      * sc = dy_scale_dev[0] * dy_scale, one fp32 product;  dot = <y16, dy16> in fp32 (dy UNSCALED);
                      * dl = (sc * y16) * (dy16 - dot) in fp32, staged in LDS in 16 bits (dl16) before BOTH products;
                      * dx = dl16 W16^T, fp32 accumulators, stored in 16 bits;
                      * dkernel += x16^T dl16 and dbias += column sums of dl16 (`dbp += lo16(d2)`: the ROUNDED image, "what the MFMAs
                        see"), fp32 accumulators -> fp32 slabs -> fp32 sums in a fixed order -> one fp32 addition into the buffer.
k_softmax_rows_fwd    * v = logits + bias in fp32 (fp32 inputs), __expf, true division, y stored in the output type.
k_softmax_rows_bwd    * dot = <y, dy> in fp32;  q = round_T(y * (dy - dot)) stored;  dbias += column sums of q (`db += to_f32(q)`: the
                        rounded image), fp32 partials, float atomics (free order).
k_weighted_sum        * fp32 fma chain per thread, wave / workgroup sums, one float atomic per workgroup into *out; no 16-bit store.
k_ctc / k_ctc_fast    * the posteriors are READ in the activation type and widened (the reference starts from that 16-bit image);
                        everything else is fp32 with __expf / __logf; the gradient is stored in the activation type (one rounding);
                        the cost is fp32.
layers._DenseSoftmaxFn fallback (widths k_dense_softmax_* does not take): the 16-bit image of the kernel (_cast_cached), a library
                        GEMM with fp32 logits, k_softmax_rows_fwd; backward k_softmax_rows_bwd, dx = dl16 W16^T stored in 16 bits,
                        dkernel = x16^T dl16 with fp32 partial sums.

e_fast  -- the relative error of the device's fast exp, the reciprocal and the multiply behind a softmax.  The ROCm device-library
documents installed with the toolchain state no accuracy for the native exp / log, so it is MEASURED (`e_fast_of`): 8 times the
largest relative deviation of a numpy float32 softmax from the float64 one on the test's own logits, computed at run time.  It is
several orders of magnitude below half an ulp of a 16-bit type.

M       -- the CTC margin, `CTC_MARGIN` = 8 (three bits): the difference between the device's fast __expf / __logf and numpy's
float32 functions, and the free order of the atomic occupancy sums.  delta(case) = max |occ32 - occ64| is the error of the SAME
recursion in numpy float32 against float64, computed per case at run time; the kernel is allowed M times that.
"""
import numpy as np

U32 = 2.0 ** -24
CTC_MARGIN = 8.0
CTC_EPS = 1e-7                      # keras.backend.epsilon(), csrc/qk_ctc.hip: g.eps

_FMT = {                            # significand bits (hidden one included), smallest normal exponent, largest finite value
    'bf16': (8, -126, float(np.float32(3.3895313892515355e38))),
    'fp16': (11, -14, 65504.0),
}


def ulp16(v, kind):
    """Spacing of the type at |v| (float64 array).  fp32 -> the fp32 spacing."""
    v = np.abs(np.asarray(v, dtype=np.float64))
    if kind == 'fp32':
        p, emin = 24, -126
    else:
        p, emin, _ = _FMT[kind]
    _, e = np.frexp(v)                                       # v = m 2^e, 0.5 <= m < 1
    e = np.where(v == 0.0, emin, np.maximum(e - 1, emin))    # exponent of the leading bit, clamped at the subnormal range
    return np.ldexp(1.0, e - (p - 1))


def half_ulp(v, kind):
    """What one round-to-nearest store of the type may move |v| by: half the spacing at |v| (at fp16 subnormals: 2^-25)."""
    return 0.5 * ulp16(v, kind)


def round16(v, kind):
    """float64 -> the nearest value of the type, ties to even, ONE rounding (float64 array out).  'fp32' rounds to float32."""
    v = np.asarray(v, dtype=np.float64)
    if kind == 'fp32':
        return v.astype(np.float32).astype(np.float64)
    q = ulp16(v, kind)
    r = np.rint(v / q) * q                                   # v / q is exact (q a power of two), rint rounds half to even
    big = _FMT[kind][2]
    return np.where(np.abs(r) > big, np.copysign(np.inf, r), r)


def softmax64(z):
    z = np.asarray(z, dtype=np.float64)
    e = np.exp(z - z.max(axis=-1, keepdims=True))
    return e / e.sum(axis=-1, keepdims=True)


def softmax32(z):
    """The same three steps in numpy float32 (max, exp of the difference, division by the sum)."""
    z = np.asarray(z, dtype=np.float32)
    e = np.exp(z - z.max(axis=-1, keepdims=True))
    return e / e.sum(axis=-1, keepdims=True, dtype=np.float32)


def e_fast_of(z):
    """8 x the largest relative deviation of the float32 softmax from the float64 softmax OF THE SAME fp32 logits (see the header)."""
    z32 = np.asarray(z, dtype=np.float32)
    y64 = softmax64(z32.astype(np.float64))
    y32 = softmax32(z32).astype(np.float64)
    return 8.0 * float(np.max(np.abs(y32 - y64) / y64)) if y64.size else 0.0


# ---------------------------------------------------------------------------------------------------------------------
# softmax output layer
# ---------------------------------------------------------------------------------------------------------------------
def dense_softmax_fwd_ref(x16, w32, bias, kind):
    """y = softmax(x W + b).  x16: the 16-bit activations as float64; w32 / bias: the fp32 master weights (bias may be None).

    reference  y64 = softmax64(x16 W16 + b), W16 = round16(w32)  (the value BEFORE the final store: the store is a bound term)
    bound      y64 * (2 max_u E_z[r, :] + e_fast) + half_ulp(y64 + that)
      E_z[r, u] = (K + 1) u32 (|b_u| + sum_k |x_rk| |W16_ku|)   fp32 accumulation of K products onto the bias, in any order;
      2 max E_z                                                  a softmax moves by at most twice the largest logit error, relatively;
      e_fast                                                     exp, reciprocal, multiply (measured, see the header);
      half_ulp                                                   the 16-bit store of y (of the perturbed value)."""
    x16 = np.asarray(x16, dtype=np.float64)
    w16 = round16(w32, kind)
    b = np.zeros(w16.shape[1]) if bias is None else np.asarray(bias, dtype=np.float64)
    z = x16 @ w16 + b
    y64 = softmax64(z)
    ez = (x16.shape[1] + 1) * U32 * (np.abs(b)[None, :] + np.abs(x16) @ np.abs(w16))
    pre = y64 * (2.0 * ez.max(axis=1, keepdims=True) + e_fast_of(z))
    return y64, pre + half_ulp(y64 + pre, kind)


def _dl_terms(y16, dy16, sc, kind, n_ops):
    """d logits of a softmax as the kernels form it: dl64 = sc y (dy - <dy, y>), its 16-bit image, and the allowance per element.

    E_dl32 = c u32 |sc| y (|dy_u| + sum_v |dy_v| y_v), c = n_ops: the fp32 error of the expression INCLUDING its cancellation --
             the dot product is U products and U - 1 additions in any order (U roundings on every term), the difference, the two
             products and the product behind sc are four more, one more for the second-order terms: c = U + 5.
    amb    = round16(dl64 - E) != round16(dl64 + E): only there may the kernel's 16-bit dl differ from the reference's, by one ulp16."""
    dot = (dy16 * y16).sum(axis=1, keepdims=True)
    dl64 = sc * y16 * (dy16 - dot)
    e32 = n_ops * U32 * abs(sc) * np.abs(y16) * (np.abs(dy16) + (np.abs(dy16) * np.abs(y16)).sum(axis=1, keepdims=True))
    if kind == 'fp32':
        return dl64, dl64, e32 + U32 * np.abs(dl64)
    dl16 = round16(dl64, kind)
    amb = round16(dl64 - e32, kind) != round16(dl64 + e32, kind)
    return dl64, dl16, e32 + amb * ulp16(np.abs(dl64) + e32, kind)


def dense_softmax_bwd_ref(x16, w32, y16, dy16, kind, dy_scale=1.0, dy_scale_dev=None, dkernel0=None, dbias0=None):
    """The backward of the output layer on the operands x16, W16 = round16(w32), y16, dy16 (float64 arrays of 16-bit values).
    dy_scale: the host factor as the C-ABI takes it (a float); dy_scale_dev: the device factor's value or None (include/qk.h:
    dy enters multiplied by dy_scale_dev[0] * dy_scale).  dkernel0 / dbias0: what the buffers hold before the call.

    Returns {'dx': (ref, bound), 'dkernel': (ref, bound), 'dbias': (ref, bound)} with A[r, u] = E_dl32 + amb * ulp16 (see _dl_terms):
      dx      ref dl16 W16^T;   bound sum_u |W16_ku| A[r, u] + (U + 1) u32 sum_u |dl16| |W16| + half_ulp(|dx64| + the two terms before)
      dkernel ref prefill + x16^T dl16;   bound sum_r |x_rk| A[r, u] + rows u32 sum_r |x_rk| |dl16_ru| + u32 |prefill|
      dbias   ref prefill + sum_r dl16 (the kernel sums the ROUNDED image);   bound sum_r A[r, u] + rows u32 sum_r |dl16_ru| + u32 |prefill|"""
    x16, y16, dy16 = (np.asarray(a, dtype=np.float64) for a in (x16, y16, dy16))
    w16 = round16(w32, kind)
    rows, U = y16.shape
    sc = float(np.float32(dy_scale)) * (1.0 if dy_scale_dev is None else float(np.float32(dy_scale_dev)))
    _, dl16, allow = _dl_terms(y16, dy16, sc, kind, U + 5)
    dx64 = dl16 @ w16.T
    b_dx = allow @ np.abs(w16).T + (U + 1) * U32 * (np.abs(dl16) @ np.abs(w16).T)
    b_dx = b_dx + half_ulp(np.abs(dx64) + b_dx, kind)
    dk0 = np.zeros(w16.shape) if dkernel0 is None else np.asarray(dkernel0, dtype=np.float64)
    db0 = np.zeros(U) if dbias0 is None else np.asarray(dbias0, dtype=np.float64)
    ax = np.abs(x16)
    b_dw = ax.T @ allow + rows * U32 * (ax.T @ np.abs(dl16)) + U32 * np.abs(dk0)
    b_db = allow.sum(axis=0) + rows * U32 * np.abs(dl16).sum(axis=0) + U32 * np.abs(db0)
    return dict(dx=(dx64, b_dx), dkernel=(dk0 + x16.T @ dl16, b_dw), dbias=(db0 + dl16.sum(axis=0), b_db))


def softmax_rows_fwd_ref(logits32, bias, kind):
    """k_softmax_rows_fwd: y = softmax(logits + bias), fp32 inputs, output type `kind` ('fp32' as well).
    bound = y64 (2 max_u E_z + e_fast) + half_ulp of the output type,  E_z = u32 |logit + b| (the one fp32 addition)."""
    z = np.asarray(logits32, dtype=np.float64)
    if bias is not None:
        z = z + np.asarray(bias, dtype=np.float64)[None, :]
    y64 = softmax64(z)
    ez = U32 * np.abs(z) if bias is not None else np.zeros_like(z)
    pre = y64 * (2.0 * ez.max(axis=1, keepdims=True) + e_fast_of(z))
    return y64, pre + half_ulp(y64 + pre, kind)


def softmax_rows_bwd_ref(y, dy, kind, dbias0=None):
    """k_softmax_rows_bwd on y, dy of type `kind` (float64 arrays of such values).
      dlogits ref dl64 (before the store);  bound E_dl32 + half_ulp(|dl64| + E_dl32),  c = cols + 5 in E_dl32 (_dl_terms, sc = 1)
      dbias   ref prefill + sum_r round_T(dl64) (the kernel's comment: the column sum of what the GEMMs see), added with atomics, free
              order;  bound sum_r (E_dl32 + amb ulp) + rows u32 sum_r |dl_T| + u32 |prefill|"""
    y, dy = np.asarray(y, dtype=np.float64), np.asarray(dy, dtype=np.float64)
    rows, cols = y.shape
    dl64, dlt, allow = _dl_terms(y, dy, 1.0, kind, cols + 5)
    e32 = (cols + 5) * U32 * np.abs(y) * (np.abs(dy) + (np.abs(dy) * np.abs(y)).sum(axis=1, keepdims=True))
    b_dl = e32 + half_ulp(np.abs(dl64) + e32, kind)
    db0 = np.zeros(cols) if dbias0 is None else np.asarray(dbias0, dtype=np.float64)
    b_db = allow.sum(axis=0) + rows * U32 * np.abs(dlt).sum(axis=0) + U32 * np.abs(db0)
    return dict(dlogits=(dl64, b_dl), dbias=(db0 + dlt.sum(axis=0), b_db))


def weighted_sum_ref(a, w32, out_before=0.0):
    """k_weighted_sum: out_before + sum_i a_i w_i.  bound = n u32 sum |a_i w_i| + u32 |out_before|  (n fp32 roundings on every term
    at the most, whatever the order of the thread, wave, workgroup and atomic sums; the last addition meets what *out held)."""
    a = np.asarray(a, dtype=np.float64).reshape(-1)
    w = np.asarray(w32, dtype=np.float64).reshape(-1)
    return float(out_before) + float((a * w).sum()), a.size * U32 * float(np.abs(a * w).sum()) + U32 * abs(float(out_before))


# ---------------------------------------------------------------------------------------------------------------------
# numpy emulations of the kernels' arithmetic (fp32 accumulation, the 16-bit rounding points): what the CPU tests hold to
# the bounds above, on every input of the GPU tests -- the proof that the inputs keep the reference alone inside its bound
# ---------------------------------------------------------------------------------------------------------------------
def _f32(a):
    return np.asarray(a, dtype=np.float64).astype(np.float32)


def emulate_dense_softmax_fwd(x16, w32, bias, kind):
    w16 = _f32(round16(w32, kind))
    z = _f32(x16) @ w16
    if bias is not None:
        z = z + _f32(bias)[None, :]
    return round16(softmax32(z).astype(np.float64), kind)


def emulate_dl(y16, dy16, sc, kind):
    y, dy = _f32(y16), _f32(dy16)
    dot = (y * dy).sum(axis=1, keepdims=True, dtype=np.float32)
    return round16(((np.float32(sc) * y) * (dy - dot)).astype(np.float64), kind)


def emulate_dense_softmax_bwd(x16, w32, y16, dy16, kind, dy_scale=1.0, dy_scale_dev=None, dkernel0=None, dbias0=None):
    sc = np.float32(dy_scale) * (np.float32(1.0) if dy_scale_dev is None else np.float32(dy_scale_dev))
    dl = _f32(emulate_dl(y16, dy16, sc, kind))
    w16 = _f32(round16(w32, kind))
    dx = round16((dl @ w16.T).astype(np.float64), kind)
    dk = _f32(x16).T @ dl
    db = dl.sum(axis=0, dtype=np.float32)
    if dkernel0 is not None:
        dk = _f32(dkernel0) + dk
    if dbias0 is not None:
        db = _f32(dbias0) + db
    return dict(dx=dx, dkernel=dk.astype(np.float64), dbias=db.astype(np.float64))


def emulate_softmax_rows_fwd(logits32, bias, kind):
    z = _f32(logits32)
    if bias is not None:
        z = z + _f32(bias)[None, :]
    return round16(softmax32(z).astype(np.float64), kind)


def emulate_softmax_rows_bwd(y, dy, kind, dbias0=None):
    dl = emulate_dl(y, dy, 1.0, kind)
    db = _f32(dl).sum(axis=0, dtype=np.float32)
    if dbias0 is not None:
        db = _f32(dbias0) + db
    return dict(dlogits=dl, dbias=db.astype(np.float64))


def emulate_weighted_sum(a, w32, out_before=0.0):
    s = np.float32(out_before)
    for chunk in np.array_split(_f32(a).reshape(-1) * _f32(w32).reshape(-1), 64):       # partial sums, then one chain
        s = s + chunk.sum(dtype=np.float32)
    return float(s)


# ---------------------------------------------------------------------------------------------------------------------
# CTC (the header of csrc/qk_ctc.hip): u = log(y_pred + eps), lp = u - logsumexp u, alpha / beta over the extended label
# sequence (blank, l1, blank, ..., blank), cost = -log p(labels), occ[t, c] = posterior occupancy of class c at frame t,
# d cost / d y_pred = (softmax(u) - occ) / (y_pred + eps).  One recursion, run in float64 and in float32.
# ---------------------------------------------------------------------------------------------------------------------
def _lse3(a, b, c):
    m = np.maximum(np.maximum(a, b), c)
    ms = np.where(np.isfinite(m), m, 0).astype(a.dtype)
    with np.errstate(divide='ignore'):
        return np.where(np.isfinite(m), ms + np.log(np.exp(a - ms) + np.exp(b - ms) + np.exp(c - ms)), -np.inf).astype(a.dtype)


def ctc_recursion(pred, labels, input_length, label_length, dtype=np.float64, occ_states=None):
    """The cost, the occupancies and the gradient of K.ctc_batch_cost for a batch, every operation in `dtype`.
    (occ_states: only states below this index enter the occupancies -- a FAULT, planted by the tests of the checker.)
    pred (B, T, C) posteriors as the kernel reads them; labels (B, Lmax) ints; lengths (B,).  blank = C - 1.
    Returns dict(cost (B,), occ, soft, pc, g (B, T, C), feasible (B,)).  A labelling that does not fit its frames costs +inf and
    has a zero gradient; so do labels without frames; no frames and no labels cost 0; frames >= input_length get zero."""
    ft = np.dtype(dtype).type
    p = np.asarray(pred, dtype=np.float64).astype(dtype)
    B, T, C = p.shape
    lab = np.asarray(labels).reshape(B, -1).astype(np.int64)
    Lmax = lab.shape[1]
    tn = np.clip(np.asarray(input_length).reshape(-1).astype(np.int64), 0, T)
    ln = np.clip(np.asarray(label_length).reshape(-1).astype(np.int64), 0, Lmax)
    S, blank = 2 * Lmax + 1, C - 1
    sidx = np.arange(S)
    cls = np.full((B, S), blank, dtype=np.int64)
    if Lmax:
        cls[:, 1::2] = np.clip(lab, 0, C - 1)
    live = sidx[None, :] < (2 * ln + 1)[:, None]
    labs = np.full((B, S), -1, dtype=np.int64)               # label of an odd state, -1 on blanks
    if Lmax:
        labs[:, 1::2] = lab
    skip_bw = np.zeros((B, S), dtype=bool)                   # s - 2 -> s: state s a label different from the previous label
    skip_bw[:, 3:] = (sidx[3:] % 2 == 1)[None, :] & (labs[:, 3:] != labs[:, 1:-2]) & live[:, 3:]
    skip_fw = np.zeros((B, S), dtype=bool)                   # s -> s + 2
    skip_fw[:, :-2] = (sidx[:-2] % 2 == 1)[None, :] & (labs[:, :-2] != labs[:, 2:]) & live[:, 2:]
    ninf = ft(-np.inf)

    pc = p + ft(CTC_EPS)
    u = np.log(pc)
    m = u.max(axis=-1, keepdims=True)
    lse = m + np.log(np.exp(u - m).sum(axis=-1, keepdims=True, dtype=dtype))
    lp = (u - lse).astype(dtype)
    soft = np.exp(lp)
    em = np.take_along_axis(lp, np.broadcast_to(cls[:, None, :], (B, T, S)), axis=2)       # lp[b, t, cls[b, s]]

    def shifted(a, k):                                       # a[:, s - k] (k > 0) or a[:, s + |k|], -inf outside
        out = np.full_like(a, ninf)
        if k > 0:
            out[:, k:] = a[:, :-k]
        else:
            out[:, :k] = a[:, -k:]
        return out

    alpha = np.full((B, T, S), ninf, dtype=dtype)
    beta = np.full((B, T, S), ninf, dtype=dtype)
    if T:
        alpha[:, 0] = np.where(live & (sidx[None, :] < 2), em[:, 0], ninf)
    for t in range(1, T):
        a = alpha[:, t - 1]
        v = _lse3(a, shifted(a, 1), np.where(skip_bw, shifted(a, 2), ninf))
        alpha[:, t] = np.where(live, v + em[:, t], ninf)
    last = (sidx[None, :] == (2 * ln)[:, None]) | (sidx[None, :] == (2 * ln - 1)[:, None])
    for t in range(T - 1, -1, -1):
        if t + 1 < T:
            b = beta[:, t + 1]
            v = _lse3(b, shifted(b, -1), np.where(skip_fw, shifted(b, -2), ninf))
            rec = np.where(live, v + em[:, t], ninf)
        else:
            rec = np.full((B, S), ninf, dtype=dtype)
        start = np.where(live & last, em[:, t], ninf)
        beta[:, t] = np.where((tn - 1 == t)[:, None], start, np.where((tn - 1 > t)[:, None], rec, ninf))
    cost = np.zeros(B, dtype=dtype)
    feasible = np.zeros(B, dtype=bool)
    occ = np.zeros((B, T, C), dtype=dtype)
    for b in range(B):
        if tn[b] == 0:
            cost[b] = ft(np.inf) if ln[b] > 0 else ft(0.0)
            continue
        al = alpha[b, tn[b] - 1]
        s_last = 2 * ln[b]
        ll = _lse3(al[s_last:s_last + 1], al[s_last - 1:s_last] if s_last >= 1 else np.full(1, ninf, dtype=dtype), np.full(1, ninf, dtype=dtype))[0]
        cost[b] = -ll
        feasible[b] = np.isfinite(ll)
    for b in np.nonzero(feasible)[0]:
        n = tn[b]
        with np.errstate(invalid='ignore'):
            q = np.exp(alpha[b, :n] + beta[b, :n] - em[b, :n] + cost[b])
        q = np.where(np.isfinite(alpha[b, :n]) & np.isfinite(beta[b, :n]), q, 0).astype(dtype)
        if occ_states is not None:
            q[:, occ_states:] = 0
        tt = np.broadcast_to(np.arange(n)[:, None], q.shape)
        np.add.at(occ[b], (tt, np.broadcast_to(cls[b][None, :], q.shape)), q)
    g = np.zeros((B, T, C), dtype=dtype)
    for b in np.nonzero(feasible)[0]:
        n = tn[b]
        g[b, :n] = (soft[b, :n] - occ[b, :n]) / pc[b, :n]
    return dict(cost=cost, occ=occ, soft=soft, pc=pc, g=g, feasible=feasible, tn=tn, ln=ln)


def ctc_ref(pred, labels, input_length, label_length, kind, margin=CTC_MARGIN):
    """(references, bounds) of the CTC kernels on the posteriors `pred` AS THE KERNEL READS THEM (already of type `kind`).

      delta       = max |occ32 - occ64| over the case: the float32 run of the same recursion against the float64 run
      bound_g     = half_ulp(|g64| + rest) + rest,  rest = (M delta + 2^-22) / pc64;   the half_ulp term is 0 for an fp32 gradient;
                    M delta: the occupancies (and soft) in fp32 with the device's fast functions; 2^-22: the fp32 subtraction and
                    division; / pc64: the gradient divides by y_pred + eps
      bound_cost  = M |cost32 - cost64| + 2^-22 |cost64|
    Entries the kernel must write as exact zeros (frames >= input_length, infeasible samples) have reference 0 and bound 0."""
    r64 = ctc_recursion(pred, labels, input_length, label_length, np.float64)
    r32 = ctc_recursion(pred, labels, input_length, label_length, np.float32)
    assert np.array_equal(r64['feasible'], r32['feasible'])
    delta = float(np.abs(r32['occ'].astype(np.float64) - r64['occ']).max())
    f = r64['feasible']
    mask = np.zeros(r64['g'].shape, dtype=bool)
    for b in np.nonzero(f)[0]:
        mask[b, :r64['tn'][b]] = True
    rest = (margin * delta + 2.0 ** -22) / r64['pc']
    bound_g = np.where(mask, rest + (0.0 if kind == 'fp32' else half_ulp(np.abs(r64['g']) + rest, kind)), 0.0)
    c64, c32 = r64['cost'], r32['cost'].astype(np.float64)
    with np.errstate(invalid='ignore'):
        bound_c = np.where(np.isfinite(c64), margin * np.abs(c32 - c64) + 2.0 ** -22 * np.abs(c64), 0.0)
    return dict(cost=(c64, bound_c), g=(r64['g'], bound_g), delta=delta, r64=r64, live=mask)


def ctc_label_mask(labels, label_length, C):
    """(B, C) bool: class c occurs among the first label_length[b] labels of sample b (the blank is no label)."""
    lab = np.asarray(labels)
    out = np.zeros((lab.shape[0], C), dtype=bool)
    for b in range(lab.shape[0]):
        out[b, lab[b, :int(np.asarray(label_length).reshape(-1)[b])]] = True
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the checker
# ---------------------------------------------------------------------------------------------------------------------
def worst_ratio(got, ref, bound):
    """(largest err / bound, its index).  An element with bound 0 must be equal (ratio inf otherwise); NaN / wrong inf -> inf."""
    got, ref, bound = (np.asarray(a, dtype=np.float64) for a in (got, ref, bound))
    assert got.shape == ref.shape == bound.shape, (got.shape, ref.shape, bound.shape)
    if got.size == 0:
        return 0.0, ()
    with np.errstate(invalid='ignore', divide='ignore'):
        err = np.abs(got - ref)
        err = np.where(got == ref, 0.0, err)                 # equal infinities
        ratio = np.where(err == 0.0, 0.0, np.where(bound > 0.0, err / bound, np.inf))
    ratio = np.where(np.isnan(ratio), np.inf, ratio)
    i = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    return float(ratio[i]), tuple(int(v) for v in i)


def assert_within(got, ref, bound, names, labels=None):
    """Every element of `got` within `bound` of `ref`; the failure names the worst element as err / bound with its position.
    names: (what, 'rows') for the output layer -- row, column, 16-row tile, 16-column tile;
           (what, 'ctc')  for the CTC gradient -- sample, frame, class, and whether the class is a label (`labels`: ctc_label_mask);
           (what, anything else): the plain index.  Returns the worst ratio."""
    what, layout = names
    ratio, i = worst_ratio(got, ref, bound)
    if ratio <= 1.0:
        return ratio
    g, r, b = (float(np.asarray(a, dtype=np.float64)[i]) for a in (got, ref, bound))
    n_bad, _ = _count_bad(got, ref, bound)
    if layout == 'rows' and len(i) == 2:
        where = 'row %d, column %d (16-row tile %d, 16-column tile %d)' % (i[0], i[1], i[0] // 16, i[1] // 16)
    elif layout == 'ctc' and len(i) == 3:
        is_label = 'unknown' if labels is None else ('a label' if labels[i[0], i[2]] else 'blank' if i[2] == np.asarray(got).shape[2] - 1 else 'no label')
        where = 'sample %d, frame %d, class %d (%s)' % (i[0], i[1], i[2], is_label)
    else:
        where = 'index %s' % (i,)
    raise AssertionError('%s: err / bound = %.3g at %s: got %.9g, reference %.9g, bound %.3g; %d of %d elements outside their bound'
                         % (what, ratio, where, g, r, b, n_bad, np.asarray(got).size))


def _count_bad(got, ref, bound):
    got, ref, bound = (np.asarray(a, dtype=np.float64) for a in (got, ref, bound))
    with np.errstate(invalid='ignore'):
        bad = ~((np.abs(got - ref) <= bound) | (got == ref))
    return int(bad.sum()), bad


def old_criterion(got, ref):
    """The norm-wise figure of the earlier tests: max |got - ref| / max |ref|."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.abs(got - ref).max() / np.abs(ref).max())
