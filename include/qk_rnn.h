/* Quaternion LSTM (Parcollet et al., "Quaternion Recurrent Neural Networks", ICLR 2019): the recurrence of one layer, both
 * directions -- the entry points of the recurrent side, exported by the same libqk_hip.so behind version 103 of include/qk.h
 * (a fourth header and a fourth table, as include/qk_opt.h and include/qk_data.h are the second and third).
 *
 * Only the recurrence is here.  The input projection zx = quaternion_dense(x, W) + b, its gradients, and the gradient of the
 * recurrent weight (one dense backward-weight over the stacked rows of `hprev` and `dzx`) are the dense entry points of qk.h.
 *
 * SEMANTICS.  units = 4 * q_units is the total real width; Q = q_units, U = units.  A state tensor (h, c) is (B, U), component-
 * major r|i|j|k: component c, unit u is column c*Q + u.  For one direction
 *
 *     z_t = zx_t + quaternion_dense(h_{t-1}, R)          R: (Q, 4U) fp32, the compact weight of a QuaternionDense of 4U outputs;
 *                                                        the product is the dense table conj(R) (x) h of qk_dense_fwd
 *     i, f, o = sigmoid(z_t[gate 0, 1, 3]);  g = tanh(z_t[gate 2])           split activations, gate order i f g o
 *     c_t = f * c_{t-1} + i * g;   h_t = o * tanh(c_t)
 *
 * Column layout of z, zx, dzx and of R's 4U output columns (compact part p of R occupies columns [p*U, (p+1)*U)): component-major
 * blocks of U columns, gate-major inside a block: component c of gate g, unit u is column c*U + g*Q + u.
 *
 * lengths (optional, int32 (B), 0 <= lengths[b] <= T; NULL: every row has length T).  At a step with t >= lengths[b] the row is
 * INACTIVE: h and c carry over unchanged, y[b, t] = 0, no gradient flows from dy[b, t] and dzx[b, t] = 0.
 *
 * Directions.  Direction 0 walks t = 0 .. T-1; direction 1 (and direction 0 under QK_QLSTM_REVERSE) walks t = T-1 .. 0 under the
 * same rule, so a row's state stays at h0 / c0 until t = lengths[b] - 1: each utterance is reversed over its own length.
 *
 * Output layout.  y and dy are (B, T, y_stride) with y_stride >= directions * U; component c, direction d, unit u is column
 * c * (directions * Q) + d * Q + u -- the quaternion concatenation of the directions, written in place.  R, h0, c0, hT, cT, zx,
 * dzx, hprev carry a leading direction axis: R (D, Q, 4U), states (D, B, U), zx / dzx (D, B, T, 4U), hprev (D, B, T, U).
 *
 * PRECISION.  dtype is the activation type of zx, y, h0, hT, dy, dhT, dzx, dh0, hprev.  R, c0, cT, dcT, dc0 are fp32.
 * The rounding points (the test reference tests/qlstm_ref.py mirrors exactly these):
 *   1. R is rounded to the activation type once per call (16-bit types; fp32: not at all).
 *   2. h_t is rounded to the activation type once per step; that value is y[:, t] and the next step's product operand.
 *   3. dz_t is rounded to the activation type once; that value is dzx[:, t] and the next backward product operand.
 *   4. dh0 is rounded to the activation type when it is written.
 * c, the products' accumulators, the gates and the gradient carries dh / dc are fp32 throughout.
 *
 * SAVED FOR BACKWARD (`reserve`): STORED, not recomputed -- per (direction, step, row) the four post-activation gates and c_t, in
 * fp32, (D, T, B, 5, U).  fp32 keeps the list of rounding points above complete; tanh(c_t) is recomputed (one tanh per element).
 * c_{t-1} is read from the previous step's record (or c0 at a row's first step), h_{t-1} from y (or h0).
 *
 * KERNELS.  One launch per time step, issued on the caller's stream from one call: no grid barrier, no persistent kernel, no
 * second stream, nothing read on the host -- a call captures into a graph.  q_units % 16 == 0 in bf16 / fp16 runs the product on
 * the matrix cores (QK_QLSTM_PATH_MFMA16) from a COMPACT 16-bit image of R built once per call into the workspace (forward: the
 * matrix-core fragments in the order the kernel reads them; backward: a plain cast); the Hamilton signs are applied to the h / dz fragments in registers, so a step reads
 * a quarter of what the sign-expanded image would cost.  Everything else (fp32, other widths) runs a plain fp32 FMA kernel
 * (QK_QLSTM_PATH_GENERIC). */
#ifndef QK_RNN_H_
#define QK_RNN_H_

#include "qk.h"

#ifdef __cplusplus
extern "C" {
#endif

#define QK_QLSTM_REVERSE 1            /* flags: with directions == 1, walk t = T-1 .. 0 (go_backwards) */
#define QK_QLSTM_PATH_GENERIC 1
#define QK_QLSTM_PATH_MFMA16 2

typedef struct qk_qlstm_desc_t {
    int32_t dtype;           /* qk_dtype_t of the activations */
    int32_t batch;           /* B >= 1 */
    int32_t steps;           /* T >= 1 */
    int32_t q_units;         /* Q >= 1; units = 4 Q */
    int32_t directions;      /* 1 or 2 */
    int32_t y_stride;        /* elements between rows (b, t) of y and dy, >= directions * units */
    int32_t flags;           /* QK_QLSTM_REVERSE */
} qk_qlstm_desc_t;

/* 0: the descriptor is invalid (qk_last_error says why); else the QK_QLSTM_PATH_* that serves it.  Host only. */
int qk_qlstm_supported(const qk_qlstm_desc_t *desc);
/* Bytes of `workspace` for op = QK_OP_FWD or QK_OP_BWD (0 for an invalid descriptor), and of `reserve`.  Host only. */
size_t qk_qlstm_workspace_bytes(const qk_qlstm_desc_t *desc, int32_t op);
size_t qk_qlstm_reserve_bytes(const qk_qlstm_desc_t *desc);

/* Forward.  h0, c0, lengths may be NULL (zero state, full length).  Writes every element of y's D*U used columns (zeros at
 * inactive positions), hT, cT, and the records of active (row, step) pairs in reserve.  Buffers must not overlap; 16-byte
 * alignment for zx, h0, y, hT, workspace; 4-byte for the rest. */
int qk_qlstm_fwd(const qk_qlstm_desc_t *desc, const void *zx, const float *R, const int32_t *lengths, const void *h0, const float *c0,
                 void *y, void *hT, float *cT, void *reserve, void *workspace, size_t workspace_bytes, void *stream);

/* Backward of the call that wrote y and reserve.  dhT, dcT, h0, c0, lengths may be NULL.  Writes every element of dzx (zeros at
 * inactive positions), of hprev (h_{t-1} of every active (row, step), zero elsewhere: the operand of the dense backward-weight that
 * yields dR from dzx), of dh0 and of dc0.  T + 1 launches: the last one, in tail mode, yields dh0. */
int qk_qlstm_bwd(const qk_qlstm_desc_t *desc, const void *dy, const void *dhT, const float *dcT, const float *R, const int32_t *lengths,
                 const void *h0, const float *c0, const void *y, const void *reserve, void *dzx, void *hprev, void *dh0, float *dc0,
                 void *workspace, size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* QK_RNN_H_ */
