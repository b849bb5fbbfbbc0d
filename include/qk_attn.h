/* Quaternion multi-head self-attention: fused forward and backward over component-major quaternion tensors -- the entry points of
 * the attention side, exported by the same libqk_hip.so behind version 103 of include/qk.h (a sixth header and a sixth table, as
 * include/qk_opt.h, include/qk_data.h, include/qk_rnn.h and include/qk_norm.h are the second to fifth).
 *
 * SEMANTICS.  Tensors are component-major like every quaternion tensor here: a row (b, t) has 4Q columns r|i|j|k, component c,
 * unit u is column c*Q + u.  Q = H * dq: head h owns units h*dq .. h*dq + dq - 1 of every component, so a head's vector is four
 * runs of dq columns, D = 4 dq reals.  Per batch row b and head h, with n = lengths[b] (n = T when lengths is NULL):
 *
 *     s[t, t'] = scale * sum_{c,u} q[b,t,c,h,u] * k[b,t',c,h,u]        t, t' < n     (scale defaults to 1 / sqrt(4 dq))
 *     p[t, :]  = softmax over t' < n of s[t, :]                        keys t' >= n never enter, whatever they hold
 *     o[b,t,c,h,u] = sum_{t' < n} p[t, t'] * v[b,t',c,h,u]             t < n
 *     o = 0 exactly, lse = 0, and dq = dk = dv = 0 exactly             at rows t >= n  (n = 0: the whole batch row)
 *
 * The score is the real part of the quaternion inner product sum_u q_u (x) conj(k_u).  The weights are real, so every value
 * quaternion is scaled as a whole and the ratios between its components survive, the principle of QuaternionLayerNormalization
 * (include/qk_norm.h).  The score is unchanged when q and k are multiplied from the right by one common unit quaternion.
 * Rows t >= n of q, k, v and do may hold anything (NaN included): they are never used.
 *
 * DEVIATION.  The component-wise Hamilton scores of Tay et al. (ACL 2019) are deliberately NOT built: they need four score
 * matrices and four times the exp work, for weights that scale the components of one quaternion differently.
 *
 * Backward, with the forward's lse[b,h,t] = m + ln(sum exp(s - m)) saved as (B, H, T) fp32 and delta[t] = sum_{c,u} do * o:
 *
 *     P  = exp(s - lse)
 *     dv = P^T do
 *     dS = P o (do v^T - delta) * scale
 *     dq = dS k
 *     dk = dS^T q
 *
 * DESCRIPTOR.  Row n = b*steps + t of a tensor starts at n * row elements; component c starts c * comp further on; head h, unit u
 * is h*dq + u further still.  comp >= heads*dq, and row is large enough for the last component: row >= 3 comp + heads*dq.  dq, dk,
 * dv use the strides of q, k, v; do uses o's.  Columns outside the addressed runs are neither read nor written.  A (B, T, 12Q)
 * output of ONE projection with 3Q quaternion units (component c holds q | k | v at columns c*3Q + [0, Q), [Q, 2Q), [2Q, 3Q)) is
 * read in place with row = 12Q, comp = 3Q and the three base pointers Q apart.
 *
 * PRECISION.  dtype is the type of q, k, v, o, do, dq, dk, dv.  lse, delta, the row maximum and the row sum are fp32; the maximum is
 * always subtracted.  Rounding points of the 16-bit paths: the probabilities are rounded to the activation type before the P v and
 * P^T do products, dS before dS k and dS^T q, and o, dq, dk, dv when they are written.  The fp32 path rounds nowhere.  The matrix
 * kernels use an online softmax: exp(s - m) is taken relative to a running maximum and rescaled, which the tests hold to a bound,
 * not to bits, against a two-pass reference.  A key tile never lies wholly past n (the key loop stops at n), so no inf - inf arises.
 *
 * DETERMINISM.  No atomics.  The backward is two kernels: one owns key blocks and sweeps the queries for dk, dv; the other owns
 * query blocks and sweeps the keys for dq -- seven products instead of five, no sum across workgroups.  A small launch before them
 * writes delta into the workspace.  Two calls agree bit for bit.
 *
 * KERNELS.  QK_QATTN_PATH_MFMA: bf16 / fp16, dq 16 or 32 (D = 64, 128), any T >= 1, strides that keep every dq-run 16-byte aligned
 * (row % 8 == 0 and comp % 8 == 0) and 16-byte aligned pointers (a call whose descriptor qualifies but whose pointers do not runs
 * the generic kernels).  One workgroup of four waves per (b, h, 64 queries), a wave owns 16 queries; q fragments in registers, 64-key
 * K / V tiles through LDS, k q^T and v^T p on v_mfma_f32_16x16x32 with the key on the accumulator's rows, so the softmax
 * reductions stay in a lane's registers plus two shuffles and p is the next product's operand without leaving the registers;
 * exp2 with the scale folded in.  A workgroup whose tile lies at or past lengths[b] only writes zeros, and the key loop stops at
 * lengths[b].  The backward kernels have the same shape with 32-row tiles of the swept side.
 * QK_QATTN_PATH_GENERIC: fp32, every other dq >= 1 and every other alignment: one wave per (b, h, row), fp32 arithmetic throughout
 * (the 16-bit types round p and dS at the rounding points above), three passes over the other side forward (maximum, sum, output),
 * served by the cache.
 * Both: 1 launch forward, 3 backward, on the caller's stream; nothing is read on the host, no grid barrier, no persistent kernel, no
 * second stream -- a call captures into a graph. */
#ifndef QK_ATTN_H_
#define QK_ATTN_H_

#include "qk.h"

#ifdef __cplusplus
extern "C" {
#endif

#define QK_QATTN_PATH_GENERIC 1
#define QK_QATTN_PATH_MFMA 2

typedef struct qk_qattn_desc_t {
    int32_t dtype;           /* qk_dtype_t of q, k, v, o and their gradients */
    int32_t batch;           /* B >= 1 */
    int32_t steps;           /* T >= 1 */
    int32_t heads;           /* H >= 1 */
    int32_t dq;              /* quaternion units per head >= 1; Q = heads * dq */
    int32_t q_row;           /* elements between rows of q and dq */
    int32_t q_comp;          /* elements between components of q and dq, >= heads * dq */
    int32_t k_row;
    int32_t k_comp;
    int32_t v_row;
    int32_t v_comp;
    int32_t o_row;           /* o and do */
    int32_t o_comp;
    int32_t flags;           /* none defined: must be 0 */
} qk_qattn_desc_t;

/* 0: the descriptor is invalid (qk_last_error says why); else the QK_QATTN_PATH_* that serves it.  Host only. */
int qk_qattn_supported(const qk_qattn_desc_t *desc);
/* Bytes of `workspace` for op = QK_OP_FWD (none is taken: 0) or QK_OP_BWD (delta); 0 for an invalid descriptor.  Host only. */
size_t qk_qattn_workspace_bytes(const qk_qattn_desc_t *desc, int32_t op);

/* Forward.  lengths (int32 (B), each 0 .. T) may be NULL; scale <= 0 means 1 / sqrt(4 dq).  Writes every element of o's addressed
 * runs and of lse (B, H, T), zeros at inactive rows.  Buffers must not overlap. */
int qk_qattn_fwd(const qk_qattn_desc_t *desc, const void *q, const void *k, const void *v, const int32_t *lengths, float scale,
                 void *o, float *lse, void *stream);

/* Backward of the call that wrote o and lse, with the same lengths and scale.  Writes every element of the addressed runs of dq, dk
 * and dv (zeros at inactive rows).  The three gradients may be windows of one buffer, as q, k, v may. */
int qk_qattn_bwd(const qk_qattn_desc_t *desc, const void *d_o, const void *q, const void *k, const void *v, const void *o,
                 const float *lse, const int32_t *lengths, float scale, void *d_q, void *d_k, void *d_v, void *workspace,
                 size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* QK_ATTN_H_ */
