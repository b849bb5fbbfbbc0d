/* Transducer (RNN-T) loss, Graves 2012 ("Sequence Transduction with Recurrent Neural Networks") -- cost and its gradient with
 * respect to the joint network's logits, with the log-softmax fused -- exported by the same libqk_hip.so behind version 103 of
 * include/qk.h (an eighth header and an eighth table, as include/qk_opt.h, qk_data.h, qk_rnn.h, qk_norm.h, qk_attn.h and
 * qk_dwconv.h are the second to seventh).
 *
 * INPUTS.  logits (B, T, U1, V), contiguous, fp32 / bf16 / fp16: the UNNORMALISED outputs of the joint, U1 = Lmax + 1 label
 * positions per frame.  labels (B, Lmax) int32; input_length (B) and label_length (B) int32, clamped to [0, T] and [0, Lmax].
 * blank = V - 1, the convention of qk_ctc_batch_cost: labels, decodes and qk_edit_distance share one class space.
 *
 * RECURSION.  Per batch row b, with Tb = the clamped input_length[b], Ub = the clamped label_length[b] and
 * lp[t,u,v] = logits[t,u,v] - lse[t,u], lse = the log-sum-exp over v in fp32 with the maximum subtracted:
 *
 *     alpha[0,0] = 0
 *     alpha[t,u] = logaddexp(alpha[t-1,u] + lp[t-1,u,blank], alpha[t,u-1] + lp[t,u-1,label[u-1]])
 *     beta[Tb-1,Ub] = lp[Tb-1,Ub,blank]
 *     beta[t,u]  = logaddexp(beta[t+1,u] + lp[t,u,blank],    beta[t,u+1] + lp[t,u,label[u]])
 *     ll = beta[0,0] = alpha[Tb-1,Ub] + lp[Tb-1,Ub,blank]
 *     cost[b] = -ll                                          (the kernel takes ll from beta[0,0])
 *
 * (a term whose source cell lies outside 0 <= t < Tb, 0 <= u <= Ub is -inf).
 *
 * GRADIENT with respect to the logits (the log-softmax is fused; this is what is stored, rounded ONCE to the logits' dtype):
 *
 *     g[t,u,v] = exp(alpha[t,u] + beta[t,u] + lp[t,u,v] - ll)
 *              - [v == blank]    exp(alpha[t,u] + lp[t,u,blank]    + nb - ll)
 *                                nb = beta[t+1,u] for t < Tb-1;  nb = 0 at (Tb-1, Ub);  nb = -inf otherwise
 *              - [v == label[u]] exp(alpha[t,u] + lp[t,u,label[u]] + beta[t,u+1] - ll)      (u < Ub)
 *
 * Every (t, u) row of g sums to zero over v, and |g| <= 1: the stored gradient cannot leave fp16's range.
 *
 * INACTIVE CELLS, INFEASIBLE ROWS.  Cells with t >= Tb or u > Ub get g = 0 exactly; the logits there are never used, NaN included.
 * A batch row with Tb = 0, or with a label outside [0, V - 2] among its first Ub, is infeasible: cost = +inf and an all-zero
 * gradient (the convention of qk_ctc_batch_cost).  A bad label never indexes memory.
 *
 * LIMITS.  2 <= V <= 256, 1 <= U1 <= 128 (Lmax <= 127, as the CTC kernels have it), T >= 1, B >= 1, B * T * U1 < 2^31; anything
 * else is QK_ERR_UNSUPPORTED.
 *
 * WORKSPACE, all fp32, R = B * T * U1 cells, D = T + U1 - 1 anti-diagonals:
 *
 *     lse, alpha, beta      3 planes (B, T, U1), row-major as the logits' rows
 *     lpb, lpl              2 planes (B, D, U1), DIAGONAL-major: cell (t, u) at [b][t + u][u] -- lp[.,.,blank] and lp[.,.,label[u]]
 *     ll                    B values, rounded up to a multiple of 4
 *
 *     qk_rnnt_workspace_bytes(B, T, U1, V) = 4 * (3 R + 2 B D U1 + 4 ceil(B / 4)) bytes
 *
 * (B 256, T 200, U1 76, V 62: 89 MB beside 482 MB of bf16 logits.)  Only active cells of the planes are written and only active
 * cells are read: no result depends on what the workspace held.
 *
 * LAUNCHES, all on the caller's stream:
 *   1. row pass: a workgroup of 256 threads owns 32 consecutive (t, u) rows -- ONE contiguous span of 32 V elements, read with
 *      16-byte loads whatever V is (32 V elements are a multiple of 16 bytes in every dtype) and staged in LDS as fp32; eight lanes
 *      reduce a row.  Writes lse, lpb, lpl.  A workgroup none of whose rows is active reads nothing.
 *   2. lattice pass: 2 B workgroups -- alpha and beta of a batch row run concurrently -- one thread per label position u, one
 *      anti-diagonal per step, Tb + Ub dependent steps.  A step's two operands are one contiguous line of the diagonal-major
 *      planes and do not depend on the recursion: they are requested four diagonals at a time, in front of the steps that use them.  U1 <= 64 is one wave and the neighbour's
 *      value moves across lanes; above 64 it goes through LDS with one barrier per diagonal.  Writes alpha, beta, ll and cost.
 *   3. gradient pass (skipped when grad is NULL): the row pass's spans again; writes g with 16-byte stores.
 * No atomics, nothing read on the host, nothing allocated: two calls agree bit for bit and a call captures into a graph.  Pointers
 * that are not 16-byte aligned are served by element-wise loads and stores in the same kernels.
 *
 * PROFILING.  The ablation field of the library's diagnostic mask (QK_ABLATE, qk_set_debug_flags) skips launches: 1 the row pass, 2
 * the lattice pass, 4 the gradient pass (tools/rnnt_time.py times each pass alone that way).  Not part of the compute contract. */
#ifndef QK_RNNT_H_
#define QK_RNNT_H_

#include "qk.h"

#ifdef __cplusplus
extern "C" {
#endif

#define QK_RNNT_MAX_CLASSES 256
#define QK_RNNT_MAX_U1 128

/* 1 when the shape is served, else 0 (qk_last_error says why).  Host only. */
int qk_rnnt_supported(int32_t dtype, int32_t B, int32_t T, int32_t U1, int32_t V);
/* Bytes of `workspace` (the formula above); 0 for an unsupported shape.  Host only. */
size_t qk_rnnt_workspace_bytes(int32_t B, int32_t T, int32_t U1, int32_t V);

/* cost (B) fp32 and, unless grad is NULL, grad (B, T, U1, V) in the logits' dtype: every element of both is written.  labels may
 * be NULL when U1 == 1.  workspace: 16-byte aligned, at least qk_rnnt_workspace_bytes(B, T, U1, V) bytes. */
int qk_rnnt_loss(int32_t dtype, int32_t B, int32_t T, int32_t U1, int32_t V, const void *logits, const int32_t *labels,
                 const int32_t *input_length, const int32_t *label_length, float *cost, void *grad /* may be NULL */,
                 void *workspace, size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* QK_RNNT_H_ */
