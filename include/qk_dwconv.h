/* Depthwise quaternion convolution over time with an optional fused GLU gate in front -- the convolution module of a Conformer
 * block -- exported by the same libqk_hip.so behind version 103 of include/qk.h (a seventh header and a seventh table, as
 * include/qk_opt.h, qk_data.h, qk_rnn.h, qk_norm.h and qk_attn.h are the second to sixth).
 *
 * SEMANTICS.  Tensors are (B, T, .) component-major r|i|j|k as every quaternion tensor here: a row (b, t) has four runs of `units`
 * = Q columns, unit u of component c at column c * comp + u.  With n = lengths[b] clamped to [0, T] (n = T when lengths is NULL),
 * K = taps and pad_lo zeros in front:
 *
 *     h[b,t,:,u] = a[b,t,:,u] * sigmoid(g[b,t,:,u])     component-wise (a "split" activation); h = a when g is NULL
 *     h          = 0                                     for t < 0 or t >= n, whatever the tensors hold there: the value is
 *                                                        SELECTED, never multiplied by 0, so a NaN in a padding frame goes nowhere
 *     y[b,t,:,u] = bias[:,u] + sum_{k<K} W[k,u] (x) h[b, t + k - pad_lo, :, u]          t < n
 *     y          = 0 exactly                             t >= n (n = 0: the whole batch row)
 *
 * (x) is the Hamilton product in the order of the convolution layers, W (x) h (conj = 0 of qk_conv_desc_t; NOT the dense table):
 *
 *     y_r = w_r h_r - w_i h_i - w_j h_j - w_k h_k          y_j = w_r h_j - w_i h_k + w_j h_r + w_k h_i
 *     y_i = w_r h_i + w_i h_r + w_j h_k - w_k h_j          y_k = w_r h_k + w_i h_j - w_j h_i + w_k h_r
 *
 * Every unit has its own K quaternion taps; nothing mixes units.  'same' padding is pad_lo = (K - 1) / 2, 'causal' pad_lo = K - 1.
 *
 * Backward, with dy taken as 0 outside [0, n):
 *
 *     dh[b,t',:,u] = sum_k conj(W[k,u]) (x) dy[b, t' + pad_lo - k, :, u]                 t' < n
 *     da = dh * sigmoid(g)      dg = dh * a * sigmoid(g) * (1 - sigmoid(g))              (da = dh without a gate)
 *     da = dg = 0 exactly                                                                t' >= n
 *     dW[k,u]      = sum_{b, t<n} dy[b,t,:,u] (x) conj(h[b, t + k - pad_lo, :, u])
 *     dbias[:,u]   = sum_{b, t<n} dy[b,t,:,u]
 *
 * WEIGHTS.  w is (K, 4Q) fp32, component-major per tap (w[k, c * Q + u]); bias is (4Q) fp32.  The kernels read both as they are:
 * there is no 16-bit image of them (the convention of gamma / beta in include/qk_norm.h).  dw (K, 4Q) and dbias (4Q) are fp32 and
 * are WRITTEN, not accumulated; either may be NULL.
 *
 * STRIDES.  a, g, da, dg have x_row elements between rows and x_comp between the components of a row; y and dy have y_row, y_comp.
 * comp >= units and row >= 3 comp + units.  Columns outside the four addressed runs are neither read nor written.  The (B, T, 8Q)
 * output of ONE projection with 2Q units (component c holds a | g at columns c * 2Q + [0, Q), [Q, 2Q)) is read in place with
 * x_row = 8Q, x_comp = 2Q and the two base pointers Q elements apart; its gradient is written as ONE (B, T, 8Q) tensor the same
 * way.  Buffers must not overlap otherwise.
 *
 * PRECISION.  dtype is the type of a, g, y, dy, da, dg: fp32, bf16 or fp16.  All arithmetic is fp32, the gated input h included: it
 * is held in fp32 where it is staged, so the 16-bit paths round in exactly THREE places -- y, da and dg when they are written.  The
 * backward recomputes sigmoid(g) from g; the forward saves nothing.
 *
 * DETERMINISM.  No atomics.  The batch rows are cut into slabs of r = ceil(B / 128) consecutive rows, S = ceil(B / r) slabs (at most
 * 128).  The backward-weight kernel keeps the K x 4 sums of a unit (and its 4 bias sums) in registers over its whole slab -- every
 * time tile of every row of it -- and writes ONE partial per slab, (S, K + 1, 4Q) fp32 (line K is dbias), into the workspace; a
 * second launch sums the slabs in slab order.  Two calls agree bit for bit.
 *
 *     qk_qdwconv_workspace_bytes(desc, QK_OP_BWD) = S * (K + 1) * 4Q * 4 bytes,  S = ceil(B / ceil(B / 128)) <= 128
 *
 * (B 256, Q 128, K 15: 4 MB beside 52 MB of y in bf16.)  The forward takes no workspace.
 *
 * KERNELS.  QK_QDWCONV_PATH_VEC: Q % 8 == 0 (bf16 / fp16) or Q % 4 == 0 (fp32), strides that are multiples of the same 8 (4) --
 * every run 16-byte aligned -- and 16-byte aligned pointers (a call whose descriptor qualifies but whose pointers do not runs the
 * generic kernels; qk_qdwconv_last_path tells).  A workgroup owns (batch row, 64-frame tile, 32 units).  Its lanes move 8 (fp32: 4)
 * consecutive units of a component run per 16-byte access, form h for the tile and its K - 1 halo frames ONCE -- one sigmoid per
 * input element -- and stage it in LDS as fp32; then a thread owns ONE unit and 8 consecutive frames, holds that unit's K taps in
 * registers and walks the K + 7 staged frames once.  Results go back through LDS and leave as 16-byte stores.  A tile at or past
 * lengths[b] only writes zeros and loads stop at lengths[b].  The backward-data kernel is the same kernel with the taps conjugated
 * and reversed and the gate's derivative in its store phase.  The backward-weight kernel stages h and dy of 32-frame tiles the same
 * way.  QK_QDWCONV_PATH_GENERIC: every other width, stride and alignment; one thread per (row, unit), plain loops.
 * Launches: 1 forward; backward 1 (+ 2 when dw or dbias is wanted), on the caller's stream; nothing is read on the host, no grid
 * barrier, no persistent kernel, no second stream, nothing allocated -- a call captures into a graph. */
#ifndef QK_DWCONV_H_
#define QK_DWCONV_H_

#include "qk.h"

#ifdef __cplusplus
extern "C" {
#endif

#define QK_QDWCONV_PATH_GENERIC 1
#define QK_QDWCONV_PATH_VEC 2

typedef struct qk_qdwconv_desc_t {
    int32_t dtype;           /* qk_dtype_t of a, g, y and their gradients */
    int32_t batch;           /* B >= 1 */
    int32_t steps;           /* T >= 1 */
    int32_t units;           /* Q >= 1 quaternion units; a row has four runs of Q columns */
    int32_t taps;            /* K, 1 .. 31 */
    int32_t pad_lo;          /* zeros in front, 0 .. taps - 1 */
    int32_t x_row;           /* elements between rows of a, g, da, dg; >= 3 x_comp + units */
    int32_t x_comp;          /* elements between their components; >= units */
    int32_t y_row;           /* the same for y and dy */
    int32_t y_comp;
    int32_t flags;           /* none defined: must be 0 */
} qk_qdwconv_desc_t;

/* 0: the descriptor is invalid (qk_last_error says why); else the QK_QDWCONV_PATH_* that serves it with 16-byte aligned pointers.
 * Host only. */
int qk_qdwconv_supported(const qk_qdwconv_desc_t *desc);
/* Bytes of `workspace` for op = QK_OP_FWD (none is taken: 0) or QK_OP_BWD (the slab partials: the formula above); 0 for an invalid
 * descriptor.  Host only. */
size_t qk_qdwconv_workspace_bytes(const qk_qdwconv_desc_t *desc, int32_t op);
/* The QK_QDWCONV_PATH_* that this thread's most recent qk_qdwconv_fwd / qk_qdwconv_bwd launched (0: none yet).  Host only. */
int qk_qdwconv_last_path(void);

/* Forward.  g, bias, lengths may be NULL.  Writes every element of y's four addressed runs (zeros at rows t >= lengths[b]). */
int qk_qdwconv_fwd(const qk_qdwconv_desc_t *desc, const void *a, const void *g, const float *w, const float *bias,
                   const int32_t *lengths, void *y, void *stream);

/* Backward.  g and dg are both NULL or both given; lengths, dw, dbias may be NULL; workspace may be NULL when dw and dbias both
 * are.  Writes every element of the addressed runs of da (and dg), zeros at rows t >= lengths[b], and every element of dw, dbias. */
int qk_qdwconv_bwd(const qk_qdwconv_desc_t *desc, const void *dy, const void *a, const void *g, const float *w,
                   const int32_t *lengths, void *da, void *dg, float *dw, float *dbias, void *workspace, size_t workspace_bytes,
                   void *stream);

#ifdef __cplusplus
}
#endif
#endif /* QK_DWCONV_H_ */
