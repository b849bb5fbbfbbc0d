/* Quaternion layer normalisation: one row of a component-major quaternion tensor is normalised as a whole -- the entry points of
 * the normalisation side, exported by the same libqk_hip.so behind version 103 of include/qk.h (a fifth header and a fifth table,
 * as include/qk_opt.h, include/qk_data.h and include/qk_rnn.h are the second, third and fourth).
 *
 * SEMANTICS.  x is (N, 4Q) with a row stride, component-major r|i|j|k as every quaternion tensor here: component c, unit u is
 * column c*Q + u (the output of a bidirectional QuaternionLSTM has this form with Q = directions * q_units).  Per row n
 *
 *     mu_c   = (1/Q)  * sum_u x[n,c,u]                          four means, one per component
 *     var    = (1/4Q) * sum_c sum_u (x[n,c,u] - mu_c)^2         ONE variance for the row
 *     rstd   = 1 / sqrt(var + epsilon)
 *     xhat   = (x - mu_c) * rstd
 *     y[n,c,u] = gamma[u] * xhat[n,c,u] + beta[c*Q + u]
 *
 * One real rstd per row and one real gamma per quaternion unit, (Q), are shared by the four components: every quaternion is scaled
 * as a whole and the ratios between its components survive.  beta is (4Q).  Either may be NULL (gamma = 1, beta = 0).
 *
 * Backward, with g = dy * gamma, m_c = (1/Q) sum_u g[c,u] and s = (1/4Q) sum_{c,u} g * xhat:
 *
 *     dx = rstd * (g - m_c - xhat * s)
 *     dgamma[u]  = sum_n sum_c dy[n,c,u] * xhat[n,c,u]
 *     dbeta[c,u] = sum_n dy[n,c,u]
 *
 * lengths (optional, int32 (B), with steps = T > 0 and rows = B * T): row n belongs to b = n / T, t = n % T, and a row with
 * t >= lengths[b] is INACTIVE: y is exactly 0 there (not beta), dx is exactly 0 there, its statistics are stored as 0 and it adds
 * nothing to dgamma / dbeta -- the convention of include/qk_rnn.h, so padding frames stay zero through a stack.
 *
 * Strides.  x and dx have x_stride elements between rows, y and dy have y_stride; both >= 4Q.  Columns from 4Q on are neither read
 * nor written.
 *
 * PRECISION.  dtype is the activation type of x, y, dy, dx.  gamma, beta, dgamma, dbeta and the statistics are fp32.  All sums and
 * the normalisation are fp32.  The variance is the centred form above, computed from the row held on chip (the means themselves
 * are summed relative to the row's first unit, so a large common offset costs no digits); it is never E[x^2] - mu^2.  Two rounding
 * points on the 16-bit paths: y when it is written and dx when it is written.
 *
 * SAVED FOR BACKWARD (`stats`): (N, 5) fp32 -- mu_0 .. mu_3 and rstd of the row.  xhat is recomputed from x.
 *
 * DETERMINISM.  No atomics.  Rows are cut into slabs of qk_qlnorm_slab_rows(desc) consecutive rows; the backward writes one partial
 * of dbeta | dgamma per slab, (slabs, 5Q) fp32, into the workspace, each column summed in a fixed order (row order per wave, then
 * the waves in order), and a second launch sums the slabs in slab order (contiguous runs of slabs in order, then the runs in
 * order).  Two calls agree bit for bit.
 *
 * KERNELS.  QK_QLNORM_PATH_VEC: q % 8 == 0 (bf16 / fp16) or q % 4 == 0 (fp32), q <= 1024, strides that keep rows 16-byte aligned,
 * and 16-byte aligned pointers (a call whose descriptor qualifies but whose pointers do not runs the generic kernels).  One wave
 * owns a row; a lane holds the same 8 (fp32: 4) units of all four components -- four 16-byte loads per 512 (256) units of Q, at
 * most two (four) such groups per lane: Q <= 1024 is the width up to which a row stays in registers, and wider rows take the generic
 * path.  The row is read from memory once forward, x and dy once backward; means, variance and the two backward sums are wave
 * reductions; the dbeta / dgamma partials of a slab stay in the lanes' registers over the slab and meet in LDS once.
 * QK_QLNORM_PATH_GENERIC: every other width and alignment, plain fp32 loops over the row, re-read from cache per pass.
 * Both: 1 launch forward, 1 backward (+ 1 when dgamma or dbeta is wanted; generic: + 2) on the caller's stream; nothing is read on
 * the host, no grid barrier, no persistent kernel, no second stream -- a call captures into a graph. */
#ifndef QK_NORM_H_
#define QK_NORM_H_

#include "qk.h"

#ifdef __cplusplus
extern "C" {
#endif

#define QK_QLNORM_PATH_GENERIC 1
#define QK_QLNORM_PATH_VEC 2

typedef struct qk_qlnorm_desc_t {
    int32_t dtype;           /* qk_dtype_t of the activations */
    int32_t rows;            /* N >= 1 */
    int32_t steps;           /* T; 0: no lengths.  T > 0 must divide rows */
    int32_t q;               /* Q >= 1 quaternion units per row; the row has 4 Q columns */
    int32_t x_stride;        /* elements between rows of x and dx, >= 4 q */
    int32_t y_stride;        /* elements between rows of y and dy, >= 4 q */
    int32_t flags;           /* none defined: must be 0 */
} qk_qlnorm_desc_t;

/* 0: the descriptor is invalid (qk_last_error says why); else the QK_QLNORM_PATH_* that serves it.  Host only. */
int qk_qlnorm_supported(const qk_qlnorm_desc_t *desc);
/* Rows per slab of the backward's weight-gradient partials (0 for an invalid descriptor).  Host only. */
int qk_qlnorm_slab_rows(const qk_qlnorm_desc_t *desc);
/* Bytes of `workspace` for op = QK_OP_FWD (none is taken: 0) or QK_OP_BWD (the slab partials); 0 for an invalid descriptor.  Host only. */
size_t qk_qlnorm_workspace_bytes(const qk_qlnorm_desc_t *desc, int32_t op);

/* Forward.  gamma, beta, lengths may be NULL (lengths must be NULL when steps == 0).  Writes every element of y's 4Q used columns
 * and of stats (zeros at inactive rows).  Buffers must not overlap; 4-byte alignment at least. */
int qk_qlnorm_fwd(const qk_qlnorm_desc_t *desc, const void *x, const float *gamma, const float *beta, const int32_t *lengths,
                  float epsilon, void *y, float *stats, void *stream);

/* Backward of the call that wrote stats.  gamma, lengths, dgamma, dbeta may be NULL; workspace may be NULL when dgamma and dbeta
 * both are.  Writes every element of dx's 4Q used columns (zeros at inactive rows), of dgamma (Q) and of dbeta (4Q). */
int qk_qlnorm_bwd(const qk_qlnorm_desc_t *desc, const void *dy, const void *x, const float *gamma, const int32_t *lengths,
                  const float *stats, void *dx, float *dgamma, float *dbeta, void *workspace, size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* QK_NORM_H_ */
