/*
 * qk.h -- C-ABI of the MI355X (gfx950) quaternion-layer engine (libqk_hip.so).
 *
 * This is the drop-in boundary for the Hamilton-product hot path of
 * Orkis-Research/Quaternion-CNN-for-E2E-ASR.  The reference has no FFI of its own: the path
 * is ~60 lines of Keras-backend calls inside two Layer.call bodies.  Each entry point below
 * names the reference code it replaces (paths relative to the reference checkout):
 *
 *   qk_conv_fwd          QuaternionConv.call      complexnn/conv.py:288-345
 *                        (slices :294-307, signed concat :327-331, K.conv{1,2,3}d :334,
 *                         K.bias_add :336-341, activation :342-343) -- all fused in one launch,
 *                         the 4x-expanded kernel is never materialised.
 *   qk_conv_bwd_data     TF autodiff of the above w.r.t. the layer input
 *   qk_conv_bwd_weight   TF autodiff of the above w.r.t. `kernel` (conv.py:175-181) and
 *                        `bias` (conv.py:270-278): the 16 expanded blocks are folded back onto
 *                        the 4 compact parts inside the kernel.
 *   qk_dense_fwd         QuaternionDense.call     complexnn/dense.py:126-164
 *                        (signed concat :139-143 == TRANSPOSED table => conj(W) (x) x,
 *                         K.dot :149, bias/activation :159-162)
 *   qk_dense_bwd_data / qk_dense_bwd_weight       TF autodiff of dense.py:126-164
 *   qk_conv_bwd / qk_dense_bwd                    the same gradients in one fused call
 *   qk_conv_fold_taps    (no reference counterpart) im2col-style fold that turns a few-channel conv into
 *                        a 1x1 quaternion conv, so the first layer also runs on the MFMA kernels
 *   qk_maxpool2d_fwd/bwd MaxPooling2D between the TIMIT convolutions (models/interspeech_model.py:99-103),
 *                        channels_last, non-overlapping windows: HBM-bound helper
 *   qk_adam_step         the Keras Adam update the reference trains with
 *                        (working_example.py:106, keras.optimizers.Adam defaults) applied to a
 *                        flat fp32 parameter buffer -- used by the data-parallel step.
 *
 * Conventions (identical to the reference):
 *   - quaternion components r,i,j,k are four CONTIGUOUS channel blocks: input channel
 *     a*Cq+c, output channel b*F+f, bias index b*F+f;
 *   - compact kernel layout (*kernel_size, Cq, 4F) with last axis p*F+f (conv.py:165,
 *     init.py:91); dense kernel (in_q, 4*q_units) (dense.py:98, init.py:153);
 *   - activations are channels_last (N, *spatial, 4C) or channels_first (N, 4C, *spatial),
 *     dense activations are (M, 4C) row-major;
 *   - cross-correlation (no kernel flip), explicit low-side padding per axis (the caller
 *     resolves 'valid' / 'same' / 'causal' with TensorFlow's rule and passes pad_lo and the
 *     output extents).
 *
 * Ownership / threading: the caller owns EVERY buffer including the workspace; the library
 * never allocates or frees device memory and never keeps a pointer past the call.  All work is
 * enqueued on the hipStream_t passed in (no host synchronisation); the functions are
 * re-entrant.  Kernel / bias / their gradients are always float32 (Keras floatx); activations
 * (x, y, dy, dx) are float32, bfloat16 or float16 with float32 accumulation.
 *
 * Errors: every function returns 0 on success or a negative qk_status_t; qk_last_error()
 * returns a thread-local message.  Nothing throws across this boundary.
 */
#ifndef QK_H_
#define QK_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define QK_VERSION 103 /* major*10000 + minor*100 + patch */

typedef enum {
    QK_OK = 0,
    QK_ERR_INVALID_ARG = -1,   /* bad descriptor / null pointer                      */
    QK_ERR_UNSUPPORTED = -2,   /* valid request this build has no kernel for         */
    QK_ERR_WORKSPACE = -3,     /* workspace missing or too small                     */
    QK_ERR_LAUNCH = -4         /* HIP runtime reported an error on launch            */
} qk_status_t;

typedef enum { QK_F32 = 0, QK_BF16 = 1, QK_F16 = 2 } qk_dtype_t;
typedef enum { QK_CH_LAST = 0, QK_CH_FIRST = 1 } qk_layout_t;
typedef enum { QK_ACT_LINEAR = 0, QK_ACT_RELU = 1 } qk_act_t;
typedef enum { QK_OP_FWD = 0, QK_OP_BWD_DATA = 1, QK_OP_BWD_WEIGHT = 2, QK_OP_BWD = 3 } qk_op_t;

/* One quaternion convolution call (QuaternionConv.__init__/build state, conv.py:93-286). */
typedef struct {
    int32_t rank;            /* 1, 2 or 3 spatial axes                                        */
    int32_t batch;           /* N                                                             */
    int32_t in_spatial[3];   /* input extents; trailing unused axes must be 1                 */
    int32_t out_spatial[3];  /* conv_utils.conv_output_length per axis (conv.py:347-372)      */
    int32_t cq;              /* quaternion input channels  = input channels / 4 (conv.py:164) */
    int32_t fq;              /* `filters`: quaternion filters, output channels = 4*fq         */
    int32_t kernel[3];       /* kernel_size                                                   */
    int32_t stride[3];       /* strides                                                       */
    int32_t dilation[3];     /* dilation_rate                                                 */
    int32_t pad_lo[3];       /* zeros in front of each axis ('same': total/2, 'causal': d(k-1)) */
    int32_t layout;          /* qk_layout_t of x / y / dy / dx                                */
    int32_t dtype;           /* qk_dtype_t  of x / y / dy / dx                                */
    int32_t activation;      /* qk_act_t fused into fwd; bwd masks dy with (y > 0) for RELU   */
    int32_t has_bias;        /* use_bias                                                      */
    int32_t conj;            /* 0: W (x) x  (conv.py:327-331);  1: conj(W) (x) x (dense table) */
    int32_t ws_has_kernel;   /* 16-bit path: nonzero = the start of `workspace` ALREADY holds the re-laid-out 16-bit
                              * kernel an earlier call with the same descriptor, the same operation class (forward |
                              * backward-data / fused backward) and UNCHANGED weights left there: the call skips that
                              * step (one small launch per call; 26 per TIMIT training step).  0 = always safe.    */
    int32_t kernel_order;    /* memory order of the compact kernel w / dw.  0 (QK_KERNEL_TAPS_MAJOR): (*kernel_size, cq, 4 fq), the
                              * layer's own layout (conv.py:165).  1 (QK_KERNEL_CHANNEL_MAJOR, round 6): (cq, *kernel_size, 4 fq) -- the
                              * weight of a QuaternionDense applied to the flattened (channel, position) axes of a channels-first feature
                              * map, read IN PLACE as the kernel of the equivalent 'valid' convolution (the TIMIT model's first
                              * TimeDistributed dense layer, models/interspeech_model.py:140-149: row cq * F + f of the dense weight is tap f,
                              * channel cq): no permuted copy of the parameter per step, and the kernel gradient is accumulated straight
                              * into the parameter's own layout.  Served by the 16-bit matrix-core kernels only (channels_last,
                              * cq % 32 == 0, fq % 32 == 0, not a band / small-channel shape for backward-weight): QK_ERR_UNSUPPORTED
                              * otherwise -- never a silent mis-read. */
} qk_conv_desc_t;
#define QK_KERNEL_TAPS_MAJOR 0
#define QK_KERNEL_CHANNEL_MAJOR 1

/* One quaternion dense call (QuaternionDense state, dense.py:58-124). */
typedef struct {
    int32_t rows;            /* M: batch rows (B, or B*T under TimeDistributed)               */
    int32_t in_q;            /* input_dim = in_features / 4          (dense.py:96)            */
    int32_t q_units;         /* units / 4                            (dense.py:75)            */
    int32_t dtype;           /* qk_dtype_t of x / y / dy / dx                                 */
    int32_t activation;      /* qk_act_t                                                      */
    int32_t has_bias;
    int32_t ws_has_kernel;   /* as in qk_conv_desc_t                                          */
} qk_dense_desc_t;

/* Library / diagnostics ------------------------------------------------------------------ */
int qk_version(void);
const char *qk_last_error(void);

/* Diagnostic switches (tests, profiling): a process-wide bit mask, read with one relaxed atomic load on
 * every launch path.  Its initial value comes from the environment, read once (QK_NO_MFMA16, QK_NO_BAND16,
 * QK_NO_BAND32, QK_WGRAD16_ONE_TAP set => the bit; QK_ABLATE=<n> => bits 8..15).  Every combination computes the
 * same values (up to the rounding of the path selected); none is needed in production.
 *   QK_DBG_NO_MFMA16        16-bit activations run on the general fp32-MFMA kernels (exact fp32 products)
 *   QK_DBG_NO_BAND16/32     no band variants of the forward / backward-data kernels
 *   QK_DBG_WGRAD16_ONE_TAP  16-bit backward-weight: one tap per block for 32-channel layers
 *   QK_DBG_BAND16_8WAVES    16-bit band kernels in their 8-wave form (env QK_BAND16_8WAVES)
 *   QK_DBG_NO_WGRAD_BAND    16-bit backward-weight without the band kernel (env QK_NO_WGRAD_BAND)
 *   QK_DBG_NO_POINT16       16-bit one-tap-per-row shapes (1 x 1, head backward-data) on the implicit-GEMM kernel
 *                           instead of the streaming point-form kernel (env QK_NO_POINT16)
 *   bits 8..15              kernel ablation for profiling (skip the MFMA loop / epilogue / atomics): WRONG RESULTS
 * qk_set_debug_flags returns the previous mask. */
#define QK_DBG_NO_MFMA16 1u
#define QK_DBG_NO_BAND16 2u
#define QK_DBG_NO_BAND32 4u
#define QK_DBG_WGRAD16_ONE_TAP 8u
#define QK_DBG_NO_WGRAD_BAND 32u   /* 16-bit backward-weight: one block per tap (k_wgrad16) instead of the band kernel */
#define QK_DBG_NO_POINT16 64u
#define QK_DBG_CTC_TWO_SWEEPS 128u /* qk_ctc_batch_cost: the round-3 form (alpha then beta, gradient inside the backward sweep; env QK_CTC_TWO_SWEEPS) */
#define QK_DBG_DETERMINISTIC 0x10000u /* bit-reproducible gradients (env QK_DETERMINISTIC): every backward-weight kernel runs
                                         * ONE split of the reduction per gradient tile and one owner per bias column, so
                                         * each element of dw / dbias receives exactly one (atomic) addition -- no
                                         * order-dependent float sums.  Several times slower (the reduction over positions is
                                         * no longer spread over the CUs): for debugging and for repeatability tests. */
#define QK_DBG_WGRAD_BAND_V1 0x20000u /* 16-bit backward-weight band kernel in its round-2..4 form (register staging, two tile buffers; env QK_WGRAD_BAND_V1) -- A/B */
#define QK_DBG_NO_SMALL16 0x40000u /* 16-bit layers with 16 / 32 channels per component on the zero-padded band kernels instead of k_hconv16_small
                                     * (env QK_NO_SMALL16; A/B).  Safe to toggle at run time: such a layer's workspace carries both 16-bit
                                     * kernel layouts in regions of their own (round 6) */
/* Graph-level A/B switches (round 6: they were environment variables read by the Python host at call time).  The library itself
 * does not act on them -- they live in this mask so that every A/B switch of the engine has ONE home, ONE initialisation from the
 * environment (same names: QK_NO_CONV_CHAIN ...) and ONE run-time API; the host-side model code (models/interspeech_model.py,
 * layers.py) asks qk_get_debug_flags().  Each one selects the unfused composition of the same arithmetic. */
#define QK_DBG_NO_CONV_CHAIN 0x100000u     /* body convolutions as separate autograd nodes instead of qk_conv_bwd_chain */
#define QK_DBG_NO_FUSED_PRELU 0x200000u    /* PReLU (+ Dropout) as qk_postop_* passes instead of the conv epilogues */
#define QK_DBG_NO_FUSED_DROPOUT 0x400000u  /* relu + Dropout as separate passes instead of the one-output post-op */
#define QK_DBG_NO_FUSED_CTC 0x800000u      /* K.ctc_batch_cost through torch's ctc_loss instead of qk_ctc_batch_cost */
#define QK_DBG_NO_FUSED_FIRST 0x1000000u   /* first layer + frequency pooling as conv, activation and pooling passes instead of qk_conv_*_pool_* */
#define QK_DBG_NO_DENSE_IN_CHAIN 0x2000000u /* the TimeDistributed quaternion-dense layers outside the backward chain */
#define QK_DBG_NO_FUSED_SOFTMAX 0x4000000u /* Dense(62, softmax) through torch ops instead of the fused output-layer kernels */
#define QK_DBG_NO_MASK_BITS 0x8000000u     /* relu + Dropout chains re-read y as the backward-data mask instead of its bit-packed form (qk_conv_*_post_bits; env QK_NO_MASK_BITS) */
#define QK_DBG_BAND16_8WAVES 16u  /* 16-bit band kernels: 8-wave workgroups (one per CU) instead of 4-wave (two per CU) */
unsigned qk_set_debug_flags(unsigned flags);
/* Profiling only: a device buffer (64 bytes per workgroup, 65536 workgroups) into which the 16-bit band kernels drop shader-clock time stamps of their
 * phases (start, prologue done, K loop done, end) and the CU they ran on -- probe builds only (tools/probe/build_variant.sh); NULL switches it off. */
void qk_set_debug_buffer(void *device_buffer, size_t bytes);
unsigned qk_get_debug_flags(void);

/* Which kernel family served the most recent qk_* compute call of the calling thread (thread-local, like
 * qk_last_error): lets a caller see when a shape fell off the 16-bit matrix-core fast path. */
typedef enum { QK_PATH_NONE = 0, QK_PATH_MFMA16 = 1, QK_PATH_MFMA16_BAND = 2, QK_PATH_FP32_MFMA = 3,
               QK_PATH_MFMA16_POINT = 4, QK_PATH_MFMA16_SMALL = 5 /* k_hconv16_small: 16 / 32 channels per component */ } qk_path_t;
int qk_last_path(void);

/* Per-call timing for benchmarks.  While enabled, every forward / backward-data / backward-weight call (including the
 * two halves of qk_*_bwd and the fused first-layer calls) is bracketed by a pair of HIP events on the caller's stream;
 * the records stay in a process-wide list until the next qk_prof_enable(1).  `ms` covers everything the call launched
 * (kernel re-layout, memsets, the GEMM kernel); rows x n x k is the GEMM view of the layer (rows = output positions,
 * n = 4 fq, k = taps * 4 cq), so 2 * rows * n * k / ms is the call's algorithmic rate.  qk_prof_get waits for the
 * record's events (host synchronisation: call it after the region of interest).  Off by default; costs one atomic load
 * per call when off. */
typedef struct {
    int32_t op;        /* QK_OP_FWD, QK_OP_BWD_DATA or QK_OP_BWD_WEIGHT */
    int32_t dtype;
    int32_t path;      /* qk_path_t that served it */
    int64_t rows;
    int32_t n, k;
    float ms;
} qk_prof_rec_t;
int qk_prof_enable(int on);          /* returns the previous state; enabling clears the list */
int qk_prof_count(void);
int qk_prof_get(int index, qk_prof_rec_t *out);

/* Bytes of caller-owned device workspace `op` needs for this descriptor (0 = none). */
size_t qk_conv_workspace_bytes(const qk_conv_desc_t *desc, int op /* qk_op_t */);
size_t qk_dense_workspace_bytes(const qk_dense_desc_t *desc, int op /* qk_op_t */);

/* Convolution ----------------------------------------------------------------------------
 * x      [N, *in_spatial, 4*cq]  (or channels_first)        desc->dtype
 * w      [*kernel, cq, 4*fq]                                float32, compact r|i|j|k
 * bias   [4*fq] or NULL                                     float32
 * y      [N, *out_spatial, 4*fq] (or channels_first)        desc->dtype
 * stream hipStream_t (passed as void* so this header needs no HIP include)
 */
int qk_conv_fwd(const qk_conv_desc_t *desc, const void *x, const float *w, const float *bias,
                void *y, void *workspace, size_t workspace_bytes, void *stream);

/* dx = d loss / d x.  `y` (the forward output) is read only when activation == RELU. */
int qk_conv_bwd_data(const qk_conv_desc_t *desc, const void *dy, const void *y, const float *w,
                     void *dx, void *workspace, size_t workspace_bytes, void *stream);

/* dw [*kernel, cq, 4*fq] and dbias [4*fq] (NULL when !has_bias) are OVERWRITTEN.
 * Layout contract: when dbias starts on the first 256-byte boundary behind the end of dw (less than 256
 * bytes away), the bytes between the two are alignment padding OWNED BY THIS CALL and are zeroed with
 * them (one fill instead of two).  Any other placement touches dw and dbias only.
 * Optional: with activation == RELU and a 16-byte-aligned workspace of at least |dy| bytes (rounded
 * up to 256), the masked gradient dy * (y > 0) is left at the start of the workspace in dy's layout;
 * qk_conv_bwd_data may then be called on it with activation = LINEAR (no y reads).  This is how a
 * data-parallel step starts its gradient all-reduce before bwd-data. */
int qk_conv_bwd_weight(const qk_conv_desc_t *desc, const void *x, const void *dy, const void *y,
                       float *dw, float *dbias, void *workspace, size_t workspace_bytes,
                       void *stream);

/* Accumulating form: dw += ..., dbias += ... (nothing is zeroed first).  For gradient accumulation over
 * micro-batches, and for training loops whose optimiser step leaves the gradient buffer zeroed
 * (qk_adam_step_zero_grad): the 5 us fill in front of every backward-weight then disappears. */
int qk_conv_bwd_weight_acc(const qk_conv_desc_t *desc, const void *x, const void *dy, const void *y,
                           float *dw, float *dbias, void *workspace, size_t workspace_bytes,
                           void *stream);
int qk_dense_bwd_weight_acc(const qk_dense_desc_t *desc, const void *x, const void *dy, const void *y,
                            float *dw, float *dbias, void *workspace, size_t workspace_bytes,
                            void *stream);

/* Fused backward: all three gradients in one call (what TF autodiff of conv.py:288-345 yields).
 * bwd-weight runs first and, for RELU, leaves the masked dy in the workspace so that bwd-data reads
 * one tensor instead of two.  dx must not be NULL.  Workspace: qk_*_workspace_bytes(desc, QK_OP_BWD). */
int qk_conv_bwd(const qk_conv_desc_t *desc, const void *x, const void *dy, const void *y, const float *w,
                void *dx, float *dw, float *dbias, void *workspace, size_t workspace_bytes, void *stream);

/* Fused backward inside a chain of relu layers.  The relu derivative of layer L, dy * (y_L > 0), costs
 * backward-weight a second input stream (every tap block re-reads y_L); the cheap place for it is the
 * epilogue of layer L+1's backward-data, whose input x IS y_L.  Flags:
 *   QK_BWD_MASK_DX      dx is returned as dx * (x > 0): the gradient w.r.t. the pre-activation of the layer
 *                       that produced x (valid when x is a relu output);
 *   QK_BWD_DY_PREMASKED dy already carries this layer's relu mask (its consumer was called with
 *                       QK_BWD_MASK_DX): the mask is not applied again and y is not read (may be NULL).
 * With flags == 0 this is qk_conv_bwd / qk_dense_bwd.  Applying a mask twice is harmless (idempotent);
 * omitting QK_BWD_DY_PREMASKED is therefore always safe, setting it on an unmasked dy is not. */
#define QK_BWD_MASK_DX 1
#define QK_BWD_DY_PREMASKED 2
#define QK_BWD_ACCUMULATE 4   /* dw / dbias are ADDED to (as qk_*_bwd_weight_acc): gradients land in a caller-zeroed buffer */
int qk_conv_bwd_chain(const qk_conv_desc_t *desc, const void *x, const void *dy, const void *y, const float *w,
                      void *dx, float *dw, float *dbias, int32_t flags, void *workspace, size_t workspace_bytes,
                      void *stream);
int qk_dense_bwd_chain(const qk_dense_desc_t *desc, const void *x, const void *dy, const void *y, const float *w,
                       void *dx, float *dw, float *dbias, int32_t flags, void *workspace, size_t workspace_bytes,
                       void *stream);

/* PReLU + Dropout behind a layer, as the reference's TIMIT model applies them after every convolution
 * (models/interspeech_model.py:99-101,117-121: `PReLU(shared_axes=[1,0])`, `Dropout(d.dropout)`):
 *     y = drop(prelu(pre)),  prelu(v) = v > 0 ? v : alpha * v,  drop(v) = keep ? v / (1 - rate) : 0.
 * alpha: float32 on the device, ONE scalar (alpha_axis = -1) or one slope per position along spatial axis
 * `alpha_axis` (0 .. rank-1) of the tensor -- what Keras builds for shared_axes=[1,0] on a channels_first (C, F, T)
 * activation is (1, F, 1): alpha_axis = 0, alpha_len = F.  The dropout mask is never stored: keep(e) is a hash of
 * (drop_seed, flat element index of y in its channels_last buffer), identical in forward and backward; pass a new
 * seed every step.  Each element gets 8 random bits: the rate applied is round(drop_rate * 256) / 256 (the kept
 * elements are scaled by the reciprocal of THAT keep probability).  drop_rate = 0 disables dropout.
 *
 * alpha == NULL selects the relu form,  y = drop(relu(pre)),  the model's `aact == 'none'` setting (relu layers with
 * `Dropout(d.dropout)` behind every body convolution, interspeech_model.py:117-121,131-137).  There the slope is 0 by
 * definition, so ONE tensor is written (y; `pre` arguments may be NULL) and the backward needs nothing but y:
 * d pre = dy / (1 - rate) where y > 0  (y > 0 <=> pre > 0 and kept) -- no mask regeneration, no slope gradient
 * (alpha_axis / alpha_len are ignored, dalpha arguments may be NULL). */
typedef struct {
    int32_t alpha_axis;      /* -1: scalar; 0..2: spatial axis of the activation that indexes alpha       */
    int32_t alpha_len;       /* 1 for a scalar, else the extent of that axis                                */
    const float *alpha;      /* device pointer, float32; NULL: relu (+ dropout), see above                  */
    float drop_rate;         /* in [0, 1)                                                                   */
    uint32_t drop_seed;
    const uint32_t *drop_seed_dev; /* optional (NULL: off): a DEVICE counter; the kernels hash with drop_seed + 0x9E3779B1 * (*drop_seed_dev).
                                    * With the training step's number there (qk_adam_step_dev keeps it) every launch argument is the same
                                    * from step to step -- a captured graph replays and still draws new masks; forward and backward of
                                    * one step agree because the counter moves only between steps */
} qk_postop_t;

/* y = post(W (x) x + b): the convolution must be LINEAR (desc->activation); `pre` receives W (x) x + b (same
 * shape / dtype as y; needed by the backward of the post-op; NULL for the relu form), `y` the activated / dropped
 * tensor. */
int qk_conv_fwd_post(const qk_conv_desc_t *desc, const qk_postop_t *post, const void *x, const float *w,
                     const float *bias, void *pre, void *y, void *workspace, size_t workspace_bytes, void *stream);

/* Fused backward of a LINEAR layer (dy = d loss / d pre of THIS layer) whose input x = post_x(x_pre) was produced by
 * a post-op: dw, dbias as qk_conv_bwd; dx receives d loss / d x_pre (the post-op's derivative is applied in the
 * epilogue of backward-data), dalpha_x[alpha_len] (float32) is ACCUMULATED into (zero it once per step).  For the
 * relu form (post_x->alpha == NULL) x_pre and dalpha_x are not used (may be NULL): x is its own mask.
 * flags: 0 or QK_BWD_ACCUMULATE (dw / dbias are added to, as qk_conv_bwd_weight_acc). */
int qk_conv_bwd_post(const qk_conv_desc_t *desc, const void *x, const void *dy, const float *w, void *dx, float *dw,
                     float *dbias, const qk_postop_t *post_x, const void *x_pre, float *dalpha_x, int32_t flags,
                     void *workspace, size_t workspace_bytes, void *stream);

/* Bit-packed mask of the relu form.  In a run of layers y_L = drop(relu(pre_L)) the backward-data epilogue of layer L+1
 * reads y_L again only to learn `y > 0`: 16 bits per element for one.  The _bits entry points move that predicate to
 * the producer: the forward epilogue that stores y also stores ONE BIT per element, and the next layer's backward-data
 * reads the bits instead of y (y itself is still written and still the backward-weight operand).
 *
 * Layout (one for every producer and consumer): bit i belongs to element i of y in its channels_last buffer -- byte
 * i >> 3, bit i & 7; a row of 4 fq elements is fq / 2 bytes, 8 consecutive elements are one byte.  The buffer is the
 * caller's, 16-byte aligned, qk_conv_mask_bits_bytes(desc) bytes (ceil(elements / 8) rounded up to 16), separate from
 * the workspace.  The bit is exactly the predicate qk_conv_bwd_post evaluates on y: `y > 0` on the value widened to
 * float -- clear for NaN and -0, set for subnormals and +inf -- so both roads give the same dx bit for bit.
 *
 * qk_conv_mask_bits_bytes: size of the bit tensor of THIS layer's output, or 0 when no forward kernel of this layer
 *   writes bits (then qk_conv_fwd_post_bits returns QK_ERR_UNSUPPORTED).  Writers: the 16-bit band kernels, channel
 *   counts that are multiples of 32, channels_last, unit stride and dilation.
 * qk_conv_bwd_reads_mask_bits: 1 when this layer's backward-data can read the bits of its INPUT x (16-bit band and
 *   point kernels, multiples of 32), else 0 (then qk_conv_bwd_post_bits returns QK_ERR_UNSUPPORTED).
 * Both follow the diagnostic switches in force when they are called; neither launches anything.
 * qk_conv_fwd_post_bits: qk_conv_fwd_post for the relu form (post->alpha == NULL), which also writes mask_bits.
 * qk_conv_bwd_post_bits: qk_conv_bwd_post for the relu form with x_mask_bits (the bits of x) in place of reading x as
 *   the mask; x is read by backward-weight only. */
size_t qk_conv_mask_bits_bytes(const qk_conv_desc_t *desc);
int qk_conv_bwd_reads_mask_bits(const qk_conv_desc_t *desc);
int qk_conv_fwd_post_bits(const qk_conv_desc_t *desc, const qk_postop_t *post, const void *x, const float *w,
                          const float *bias, void *pre, void *y, void *mask_bits, void *workspace,
                          size_t workspace_bytes, void *stream);
int qk_conv_bwd_post_bits(const qk_conv_desc_t *desc, const void *x, const void *x_mask_bits, const void *dy,
                          const float *w, void *dx, float *dw, float *dbias, const qk_postop_t *post_x, int32_t flags,
                          void *workspace, size_t workspace_bytes, void *stream);

/* The post-op on its own (any dtype / shape, HBM-bound): `t` describes the channels_last activation
 * (batch, spatial[0..rank-1], channels) -- only batch, rank, out_spatial, fq (channels = 4 * fq) and dtype of a
 * qk_conv_desc_t are read.  bwd: dpre = d loss / d pre, dalpha accumulated.  Relu form (alpha == NULL): the
 * backward takes the forward OUTPUT y in place of `pre`, dalpha may be NULL. */
int qk_postop_fwd(const qk_conv_desc_t *t, const qk_postop_t *post, const void *pre, void *y, void *stream);
int qk_postop_bwd(const qk_conv_desc_t *t, const qk_postop_t *post, const void *pre, const void *dy, void *dpre,
                  float *dalpha, void *stream);

/* The first layer of the TIMIT model as ONE kernel per direction (models/interspeech_model.py:97-103):
 *     QuaternionConv2D(F, (3,5), padding='same', relu) on ONE quaternion channel -> MaxPooling2D over the first
 *     spatial axis with window = stride = `pool`, 'same' (partial last window).
 * The layer is HBM-bound; fused, the forward reads x (N, H, W, 4) and writes only the pooled tensor
 * (N, ceil(H / pool), W, 4F) plus `aux` (opaque to the caller, qk_conv_relu_pool_aux_bytes: 3 bits per pooled element --
 * one-hot "window row 0 / 1 / 2 held the maximum and relu let it through", all clear = nothing flows back -- in the
 * kernels' register order), the backward reads x, the pooled gradient and aux and returns dw / dbias (overwritten) -- the
 * 537 MB pre-pool activation of the B = 256 model never exists.  Supported: rank 2, QK_CH_LAST, bf16 / fp16, cq == 1, kernel
 * (3,5), unit stride / dilation, pad_lo (1,2), activation RELU, conj 0, fq % 8 == 0, pool == 3, H % 3 != 1 (the
 * kernel's windows are rows [3o, 3o + 2]; TensorFlow's 'same' rule pads one row on the LOW side when H % 3 == 1, so
 * for those heights the windows would start at row -1: not this kernel's -- 41 bins are fine); anything else returns
 * QK_ERR_UNSUPPORTED (qk_conv_relu_pool_aux_bytes: 0) and the caller runs qk_conv_fwd + qk_maxpool2d_* instead.
 * `aux` may be NULL in the forward (inference).
 * desc->layout describes x ONLY here: QK_CH_LAST = (N, H, W, 4); QK_CH_FIRST = (N, 4, H, W), the four r / i / j / k
 * component PLANES of the one quaternion channel exactly as the reference feeds its model (Input(shape=(4, 41, None)),
 * interspeech_model.py:81) -- each plane row is read with coalesced loads and the planes are interleaved while the
 * patch is staged in LDS.  The pooled tensor (and its gradient) is always channels_last: this layer is where a
 * channels_first model's data enters the engine's channels-last domain, so no separate re-layout pass exists.
 * bwd flags: 0 (dw / dbias overwritten) or QK_BWD_ACCUMULATE (added to). */
size_t qk_conv_relu_pool_aux_bytes(const qk_conv_desc_t *desc, int32_t pool);
int qk_conv_relu_pool_fwd(const qk_conv_desc_t *desc, int32_t pool, const void *x, const float *w, const float *bias,
                          void *pooled, void *aux, void *stream);
int qk_conv_relu_pool_bwd(const qk_conv_desc_t *desc, int32_t pool, const void *x, const void *dpooled, const void *aux,
                          float *dw, float *dbias, int32_t flags, void *stream);

/* The same layer in its PReLU form (the reference's aact == 'prelu'): LINEAR convolution (desc->activation), PReLU with
 * one slope per row of the conv output (post->alpha_axis 0, alpha_len == in_spatial[0] <= 64: Keras shared_axes=[1,0])
 * or one slope (alpha_axis -1), then the pooling; post->drop_rate must be 0.  `pre_pooled` (same shape / dtype as
 * `pooled`) receives the pre-activation of each window's arg-max -- the backward needs it for the derivative and the
 * slope gradient `dalpha[alpha_len]` (float32, ACCUMULATED into); aux as above (qk_conv_relu_pool_aux_bytes accepts
 * the LINEAR descriptor as well).  dw / dbias are overwritten. */
int qk_conv_prelu_pool_fwd(const qk_conv_desc_t *desc, int32_t pool, const qk_postop_t *post, const void *x, const float *w,
                           const float *bias, void *pooled, void *pre_pooled, void *aux, void *stream);
int qk_conv_prelu_pool_bwd(const qk_conv_desc_t *desc, int32_t pool, const qk_postop_t *post, const void *x, const void *dpooled,
                           const void *pre_pooled, const void *aux, float *dw, float *dbias, float *dalpha, int32_t flags,
                           void *stream);

/* Tap folding for layers with very few input channels (the first TIMIT layer has cq = 1: K = 4*taps).
 *   xcol[m, a*cq2 + t*cq + c] = x[pos(m, t), a*cq + c]      (0 in the padding and for t*cq + c >= taps*cq)
 * xcol is channels_last (N, *out_spatial, 4*cq2), cq2 a multiple of 8 with cq2 >= taps*cq.  The layer
 * then IS a 1x1 quaternion convolution on xcol with the kernel reshaped to (taps*cq -> cq2, 4*fq): the
 * Hamilton structure acts per channel, so it survives the fold.  HBM-bound gather. */
int qk_conv_fold_taps(const qk_conv_desc_t *desc, const void *x, void *xcol, int32_t cq2, void *stream);

/* Dense ---------------------------------------------------------------------------------
 * x [rows, 4*in_q], w [in_q, 4*q_units] float32, bias [4*q_units], y [rows, 4*q_units]
 */
int qk_dense_fwd(const qk_dense_desc_t *desc, const void *x, const float *w, const float *bias,
                 void *y, void *workspace, size_t workspace_bytes, void *stream);
int qk_dense_bwd_data(const qk_dense_desc_t *desc, const void *dy, const void *y, const float *w,
                      void *dx, void *workspace, size_t workspace_bytes, void *stream);
int qk_dense_bwd_weight(const qk_dense_desc_t *desc, const void *x, const void *dy, const void *y,
                        float *dw, float *dbias, void *workspace, size_t workspace_bytes,
                        void *stream);

int qk_dense_bwd(const qk_dense_desc_t *desc, const void *x, const void *dy, const void *y, const float *w,
                 void *dx, float *dw, float *dbias, void *workspace, size_t workspace_bytes, void *stream);

/* Max pooling of a channels_last activation (N, H, W, C) -- the layer between the first and second
 * TIMIT convolutions (MaxPooling2D((1,3), padding='same'), models/interspeech_model.py:99-103), which
 * on a channels_first quaternion tensor pools the frequency axis.  Not part of the Hamilton product;
 * it lives here because the engine keeps channels_first tensors physically channels_last and the
 * framework kernels for that layout run at a third of HBM speed.  Windows must not overlap
 * (stride == window) and TensorFlow's padding must fall on the high side only ('valid', or 'same'
 * with no low-side padding): a partial last window simply ignores the missing elements.
 * Ties go to the first maximum in (h, w) window order, NaN propagates (torch / TF semantics).
 * bwd recomputes the arg-max from x (no index tensor) and writes EVERY element of dx. */
typedef struct {
    int32_t batch, in_h, in_w, channels;   /* x: (batch, in_h, in_w, channels)                   */
    int32_t win_h, win_w;                  /* window == stride                                    */
    int32_t out_h, out_w;                  /* ceil(in/win) for 'same', floor(in/win) for 'valid'  */
    int32_t dtype;                         /* qk_dtype_t                                          */
} qk_pool_desc_t;
int qk_maxpool2d_fwd(const qk_pool_desc_t *desc, const void *x, void *y, void *stream);
int qk_maxpool2d_bwd(const qk_pool_desc_t *desc, const void *x, const void *dy, void *dx, void *stream);

/* Optimiser step on a flat fp32 buffer (Keras Adam: working_example.py:106).
 *   m = b1*m + (1-b1)*g ; v = b2*v + (1-b2)*g^2
 *   p -= lr * sqrt(1-b2^t)/(1-b1^t) * m / (sqrt(v) + eps)          (Keras 2.x form)
 * `grad_scale` multiplies g first (1/world_size after a sum all-reduce). */
int qk_adam_step(float *param, const float *grad, float *m, float *v, size_t n, float lr,
                 float beta1, float beta2, float eps, int32_t step, float grad_scale,
                 void *stream);

/* qk_adam_step that also writes zeros over `grad` once it has been consumed, so the next backward can
 * accumulate into it (qk_*_bwd_weight_acc) without a separate fill. */
int qk_adam_step_zero_grad(float *param, float *grad, float *m, float *v, size_t n, float lr,
                           float beta1, float beta2, float eps, int32_t step, float grad_scale,
                           void *stream);

/* K.ctc_batch_cost(y_true, y_pred, input_length, label_length) -- what the reference's TIMIT model outputs
 * (models/interspeech_model.py:37-39,178) -- and its gradient, as one launch: y_pred (batch, frames, classes) are the
 * model's softmax outputs (blank = classes - 1), labels (batch, max_label_len) int32 padded, input_length / label_length
 * (batch) int32.  Keras 2.x / TensorFlow semantics: log(y_pred + 1e-7) taken as LOGITS (normalised again per frame),
 * ctc_merge_repeated = True, frames >= input_length ignored.  cost (batch) float32 = -log p(labels | y_pred);
 * dy_pred (same dtype / shape as y_pred, or NULL) = d cost[b] / d y_pred[b].  One workgroup per sample; limits:
 * Degenerate samples: an infeasible one (more labels, counting a blank between repeats, than frames -- TensorFlow raises
 * for it) gets cost = +inf and a ZERO gradient row; input_length == 0 gives cost 0 for an empty label sequence, +inf
 * otherwise; labels outside [0, classes - 2] are clamped (TensorFlow raises).
 * max_label_len <= 127, classes <= 256, frames up to ~15 000 (LDS); QK_ERR_UNSUPPORTED beyond.
 * Workspace: qk_ctc_workspace_bytes (the alpha and beta lattices, 2 x frames x (2 max_label_len + 1) floats per sample). */
size_t qk_ctc_workspace_bytes(int32_t batch, int32_t frames, int32_t max_label_len);
int qk_ctc_batch_cost(int32_t dtype, int32_t batch, int32_t frames, int32_t classes, const void *y_pred, const int32_t *labels,
                      int32_t max_label_len, const int32_t *input_length, const int32_t *label_length, float *cost, void *dy_pred,
                      void *workspace, size_t workspace_bytes, void *stream);

/* ---- CTC decoding ----------------------------------------------------------------------------------------------------------
 * K.ctc_decode and tf.edit_distance: what turns the posteriors of the validation function (models/interspeech_model.py:182-185 of
 * the reference) into a phone error rate.  y_pred (batch, frames, classes) are softmax outputs in `dtype`, blank = classes - 1 (as in
 * K.ctc_batch_cost), u[t][c] = log(y_pred[t][c] + 1e-7); only the first Tn = min(max(input_length[b], 0), frames) frames count
 * (input_length: batch int32).  Tn = 0 gives an empty decode with log_prob 0.  All buffers are caller-owned device memory; the calls
 * launch on `stream` and never synchronise.
 *
 * Greedy (K.ctc_decode(greedy=True) = tf.nn.ctc_greedy_decoder(merge_repeated=True)), one wave per sample: per frame the argmax
 * over classes (the lowest index on ties), runs of equal symbols merged, then blanks dropped (a blank between two equal labels
 * keeps both).  decoded (batch, frames) int32 padded with -1, decoded_len (batch), log_prob (batch) = -sum_{t < Tn} max_c u[t][c]
 * (TensorFlow's neg_sum_logits, sign included, which Keras returns under the name log_prob).  classes <= 256.
 *
 * Beam search (K.ctc_decode(greedy=False, beam_width, top_paths) without a language model; an LM variant follows), one workgroup per sample: the CTC
 * prefix beam search in lp[t][c] = u[t][c] - logsumexp_c u[t][.]; from the empty prefix, each frame keeps the beam_width best of
 * the candidates (every beam staying, every beam extended by a non-blank class; an extension equal to a beam is merged into it),
 * ordered by total log-probability, ties: stay before extension, then lower source rank, then lower class; -inf never enters.
 * decoded (top_paths, batch, frames) int32 padded with -1, decoded_len (top_paths, batch), log_prob (batch, top_paths) float32 =
 * log p(prefix | y_pred) NORMALISED (TensorFlow reports per-frame shifted scores; the ranking is the same).  Paths beyond the
 * number of distinct beams are empty with log_prob -inf.  merge_repeated != 0 (TF 1.x default) collapses consecutive equal labels
 * of the returned prefix on output; log_prob stays that of the uncollapsed prefix.  Limits: beam_width <= 128,
 * top_paths <= beam_width, classes <= 256: QK_ERR_UNSUPPORTED beyond.  Workspace: qk_ctc_beam_workspace_bytes (one history word
 * per sample, frame and beam slot).
 *
 * Beam search with a phone n-gram language model (qk_ctc_beam_search_decode_lm): the same search, every candidate prefix l ranked by
 *     S(l) = log p(l | y_pred) + lm_weight log P_LM(l) + insertion_bonus |l|
 * in place of the total alone (the pb / pnb recursions, the merge, the tie rule and -inf exclusion are unchanged; P_LM(l) is the
 * product of P(l_i | the preceding lm_order - 1 labels), <s>-padded on the left).  lm_eos != 0 re-ranks the final beams by
 * S + lm_weight log P(</s> | l) before the top paths are read.  lm_table: device float32 natural-log probabilities
 * (classes^(lm_order - 1), classes), finite or -inf; with V = classes - 1 (the blank's index), index V means <s> in a context and
 * </s> as the event; the bigram context is the last label (V for the empty prefix), the trigram context last2 classes + last
 * (V where missing), order 1 has a single row.  lm_weight must be finite and >= 0, insertion_bonus finite (QK_ERR_INVALID_ARG);
 * lm_weight = 0 never reads the table, and lm_weight = insertion_bonus = 0 gives qk_ctc_beam_search_decode's results bit for
 * bit.  log_prob (batch, top_paths) keeps its meaning (acoustic log p(prefix | y_pred)); score (batch, top_paths) float32 = the S
 * the paths were ranked by; both -inf for empty paths.  merge_repeated collapses the output only: the LM scored the uncollapsed
 * prefix.  Limits as above, and lm_order in 1 .. 3, lm_order 3 only for classes <= 64 (QK_ERR_UNSUPPORTED beyond); tables up to
 * 64 KB live in LDS, larger ones stage the row of each beam's context per frame (beam_width x classes floats).  Workspace:
 * qk_ctc_beam_workspace_bytes.
 *
 * Edit distance (tf.edit_distance, unnormalised), one wave per pair: Levenshtein distance with unit costs between hypothesis b
 * (hyp + b hyp_stride, hyp_len[b] tokens) and reference b (ref + b ref_stride, ref_len[b] tokens); lengths are clamped to
 * [0, stride].  class_map (classes int32, or NULL) is applied to both first: a token t in [0, classes) becomes class_map[t], and is
 * dropped when that is negative; other tokens are compared as they are.  distance (batch) int32; ref_len_out (batch, or NULL) =
 * the reference length after the map.  ref_stride <= 1024 (QK_ERR_UNSUPPORTED beyond); any hypothesis length. */
int qk_ctc_greedy_decode(int32_t dtype, int32_t batch, int32_t frames, int32_t classes, const void *y_pred, const int32_t *input_length,
                         int32_t *decoded, int32_t *decoded_len, float *log_prob, void *stream);
size_t qk_ctc_beam_workspace_bytes(int32_t batch, int32_t frames, int32_t beam_width);
int qk_ctc_beam_search_decode(int32_t dtype, int32_t batch, int32_t frames, int32_t classes, const void *y_pred, const int32_t *input_length,
                              int32_t beam_width, int32_t top_paths, int32_t merge_repeated, int32_t *decoded, int32_t *decoded_len,
                              float *log_prob, void *workspace, size_t workspace_bytes, void *stream);
int qk_ctc_beam_search_decode_lm(int32_t dtype, int32_t batch, int32_t frames, int32_t classes, const void *y_pred,
                                 const int32_t *input_length, int32_t beam_width, int32_t top_paths, int32_t merge_repeated,
                                 int32_t lm_order, const float *lm_table, float lm_weight, float insertion_bonus, int32_t lm_eos,
                                 int32_t *decoded, int32_t *decoded_len, float *log_prob, float *score,
                                 void *workspace, size_t workspace_bytes, void *stream);
int qk_edit_distance(int32_t batch, const int32_t *hyp, int32_t hyp_stride, const int32_t *hyp_len, const int32_t *ref, int32_t ref_stride,
                     const int32_t *ref_len, const int32_t *class_map, int32_t classes, int32_t *distance, int32_t *ref_len_out, void *stream);

/* ---- Scoring alignment ----------------------------------------------------------------------------------------------------------
 * What sclite / compute-wer report beyond the distance: the split into correct, substituted, deleted and inserted tokens, the
 * aligned reference / hypothesis pairs and the confusion matrix.  Inputs are those of qk_edit_distance: hyp (batch, hyp_stride),
 * ref (batch, ref_stride) int32 with hyp_len, ref_len (batch) int32 clamped to [0, stride]; class_map (classes) int32 or NULL is
 * applied to both sequences first: a token t in [0, classes) becomes class_map[t] and is dropped when that is negative, any other
 * token passes through unchanged.  h_1..h_H and r_1..r_R are the sequences after the map.
 *
 * D[i][j] is the unit-cost Levenshtein distance between h_1..h_i and r_1..r_j.  The alignment is read backwards from (H, R) to
 * (0, 0) under this tie rule, which is part of the definition (the result is bit-repeatable):
 *   1. if i > 0, j > 0 and D[i][j] == D[i-1][j-1] + (h_i != r_j): the DIAGONAL -- correct when h_i == r_j, a substitution otherwise;
 *   2. otherwise, if j > 0 and D[i][j] == D[i][j-1] + 1: a DELETION, r_j has no partner;
 *   3. otherwise an INSERTION, h_i has no partner.
 * Equivalently: of all minimum-cost alignments, read from the end, the smallest under diagonal < deletion < insertion.
 *
 * Outputs (caller-owned device memory; every element of every non-NULL output is written by every call, except confusion, which
 * accumulates):
 *   counts   (batch, 4) int32     correct, substitutions, deletions, insertions: C + S + D = R, C + S + I = H, S + D + I is the
 *                                 distance of qk_edit_distance;
 *   ali_ref, ali_hyp (batch, A) int32, A = hyp_stride + ref_stride   the aligned pairs in forward order, as mapped tokens;
 *                                 ali_hyp = -1 marks a deletion, ali_ref = -1 an insertion; both -1 from ali_len[b] on;
 *   ali_len  (batch) int32        the number of aligned pairs (<= H + R).
 *                                 ali_ref, ali_hyp and ali_len are NULL together (the counts-only call) or not at all;
 *   confusion ((K + 1), (K + 1)) int32 row-major, K = out_classes, or NULL   confusion[r][h] is INCREMENTED for every aligned
 *                                 pair; row K holds the insertions, column K the deletions, [K][K] is never touched.  A pair with
 *                                 a token outside [0, K) is left out of the matrix but still counted in counts.  The caller zeroes
 *                                 the matrix once and accumulates over as many batches as wanted; integer adds keep the result
 *                                 independent of the execution order.
 *
 * One wave per pair: the row sweep of qk_edit_distance, a 2-bit decision per cell packed by ballots (16 bytes per row and 64
 * reference positions), one lane backtracks.  The decision table lives in LDS when the STRIDES (not the pair's own lengths) let
 * the whole image fit in 64 KB, and in the workspace otherwise: qk_edit_align_workspace_bytes is 0 in the first case and
 * batch * hyp_stride * 16 E bytes in the second (E = 1, 2, 4, 8, 17 for ref_stride < 64, 128, 256, 512, <= 1024); the workspace is
 * 8-byte aligned and may be NULL when no bytes are needed.
 * Limits: hyp_stride, ref_stride <= 1024 and, with confusion, out_classes <= 256: QK_ERR_UNSUPPORTED beyond.  Negative sizes and
 * NULL required pointers: QK_ERR_INVALID_ARG.  Every such check happens before any pointer is touched.  batch == 0 returns 0
 * without a launch.  Launches on `stream` and never synchronises. */
size_t qk_edit_align_workspace_bytes(int32_t batch, int32_t hyp_stride, int32_t ref_stride);
int qk_edit_align(int32_t batch, const int32_t *hyp, int32_t hyp_stride, const int32_t *hyp_len, const int32_t *ref, int32_t ref_stride,
                  const int32_t *ref_len, const int32_t *class_map, int32_t classes, int32_t *counts, int32_t *ali_ref, int32_t *ali_hyp,
                  int32_t *ali_len, int32_t *confusion, int32_t out_classes, void *workspace, size_t workspace_bytes, void *stream);

/* ---- CTC forced alignment ----------------------------------------------------------------------------------------------------
 * The best path of the CTC lattice of a KNOWN transcript: which frames belong to which label.  Inputs are those of
 * qk_ctc_batch_cost: y_pred (batch, frames, classes) softmax outputs in `dtype` (fp32, bf16 or fp16), blank = classes - 1; labels
 * (batch, max_label_len) int32; input_length, label_length (batch) int32.  Tn = min(max(input_length[b], 0), frames) and
 * Ln = min(max(label_length[b], 0), max_label_len); labels outside [0, classes - 2] are clamped as the cost clamps them.
 * max_label_len == 0 is allowed (labels, starts and ends may then be NULL).
 *
 * Emissions are exactly those of the cost: u[t][c] = log(y_pred[t][c] + 1e-7), lp[t][c] = u[t][c] - logsumexp_c u[t][.]; all
 * arithmetic is fp32, 16-bit inputs are widened exactly.  States are the extended sequence l' = blank, l1, blank, ..., lL, blank
 * (S = 2 Ln + 1); the transitions are those of the alpha recursion: stay, from s - 1, and from s - 2 when s is a label state and
 * l'[s] != l'[s - 2].  A path starts in state 0 or 1 and ends in state S - 1 or S - 2.  The result is the path pi through the
 * states that maximises sum_{t < Tn} lp[t][l'[pi_t]].
 * Tie rule (the result is bit-repeatable): among equal predecessors stay wins over s - 1, and s - 1 over s - 2; at the end S - 1
 * wins over S - 2; -inf never wins.
 *
 * Every element of every output is written by every call:
 *   path   (batch, frames) int32         the class at each frame t < Tn (blank = classes - 1); -1 from Tn on;
 *   starts, ends (batch, max_label_len) int32   the first frame of label i and one past its last frame -- the frames spent in
 *                                        state 2 i + 1, contiguous by construction; both -1 for i >= Ln;
 *   score  (batch) float32               the path's log-probability under lp, so that score <= -cost.
 * An infeasible sample (more labels, counting a blank between repeats, than frames) gets score = -inf and path, starts, ends all
 * -1.  Tn == 0: score = 0 if Ln == 0, else the infeasible result (path is all -1 either way).
 *
 * One workgroup per sample, one max-plus sweep with 2-bit back-pointers (64 bytes per frame), kept in LDS when the sample's frames
 * fit and in the workspace otherwise, then a backtrack; the score is summed in a fixed order, without atomics.  Limits: classes <=
 * 256, max_label_len <= 127, frames up to ~30 000 (LDS): QK_ERR_UNSUPPORTED beyond, as for an unknown dtype.  Workspace:
 * qk_ctc_align_workspace_bytes (64 bytes per sample and frame), 8-byte aligned.  Launches on `stream` and never synchronises. */
size_t qk_ctc_align_workspace_bytes(int32_t batch, int32_t frames, int32_t max_label_len);
int qk_ctc_forced_align(int32_t dtype, int32_t batch, int32_t frames, int32_t classes, const void *y_pred, const int32_t *labels,
                        int32_t max_label_len, const int32_t *input_length, const int32_t *label_length, int32_t *path,
                        int32_t *starts, int32_t *ends, float *score, void *workspace, size_t workspace_bytes, void *stream);

/* ---- Acoustic front end ----------------------------------------------------------------------------------------------------
 * Waveforms -> the model's channels_first quaternion input out (batch, 4, F, frames), F = nfilt + (append_energy != 0): the
 * python_speech_features logfbank + delta recipe (the reference's Input(shape=(4, 41, None)), models/interspeech_model.py:81, with
 * nfilt = 40).  Per utterance b of n = min(max(lengths[b], 0), max_samples) samples of row b of wave (batch, max_samples):
 *   pre-emphasis s'[0] = s[0], s'[i] = s[i] - preemph s[i-1]; n_b = qk_fbank_num_frames(n, frame_len, frame_step) frames of frame_len
 *   samples every frame_step (zero padding to (n_b - 1) frame_step + frame_len), times the window (QK_WINDOW_RECT: 1, QK_WINDOW_HAMMING:
 *   numpy.hamming(frame_len)); P = |rfft(frame, nfft)|^2 / nfft; rows 0..nfilt-1 = log(sum_k W[j][k] P[k]) with the triangles
 *   W[j] of python_speech_features.get_filterbanks on the integer FFT bins mel_bins[j] <= mel_bins[j+1] <= mel_bins[j+2] (a HOST
 *   array of nfilt + 2 entries in [0, nfft / 2]); row nfilt = log(sum_k P[k]) when append_energy; an exact zero becomes float64 eps
 *   (2.22e-16) before the log.  Plane 0 = these static rows, planes 1..3 = delta, delta^2, delta^3 along time with
 *   d[t] = sum_{k=-N..N} k x[clamp(t + k, 0, n_b - 1)] / (2 sum_{k=1..N} k^2), N = delta_n, clamped at each utterance's own frames.
 *   Frames t >= n_b are 0 in every plane.  normalize = QK_FBANK_NORM_UTTERANCE: every (b, plane, row) becomes (x - mean) /
 *   sqrt(var + 1e-8) over its n_b valid frames (biased variance); padding stays 0.
 * Arithmetic is fp32 throughout (the static rows stay fp32 until the deltas are done); out_dtype (qk_dtype_t) is rounded once, at
 * the store; the FFT's rounding error is ~1e-7 of the frame's norm in every bin, so a band far below the frame's energy has a
 * proportionally larger error in its log.  wave_dtype: QK_WAVE_I16 (int16) or QK_WAVE_F32.  frame_lengths (batch) int32 receives n_b (a CTC input_length).
 * frames >= qk_fbank_num_frames(max_samples, ...).  Limits (QK_ERR_UNSUPPORTED beyond): nfft a power of two in [256, 1024],
 * 1 <= frame_len <= nfft, nfilt <= QK_FBANK_MAX_FILT, 1 <= delta_n <= 4.  Workspace: qk_fbank_workspace_bytes (the fp32 static rows,
 * plus the fp32 planes when normalising).  Launches on `stream` and never synchronises. */
#define QK_FBANK_MAX_FILT 128
enum { QK_WAVE_F32 = 0, QK_WAVE_I16 = 1 };
enum { QK_WINDOW_RECT = 0, QK_WINDOW_HAMMING = 1 };
enum { QK_FBANK_NORM_NONE = 0, QK_FBANK_NORM_UTTERANCE = 1 };
int32_t qk_fbank_num_frames(int64_t samples, int32_t frame_len, int32_t frame_step);
size_t qk_fbank_workspace_bytes(int32_t batch, int32_t frames, int32_t rows, int32_t normalize);
int qk_fbank_quaternion(int32_t wave_dtype, int32_t batch, int64_t max_samples, const void *wave, const int32_t *lengths, int32_t frames,
                        int32_t frame_len, int32_t frame_step, int32_t nfft, float preemph, int32_t window, int32_t nfilt,
                        const int32_t *mel_bins, int32_t append_energy, int32_t delta_n, int32_t normalize, int32_t out_dtype, void *out,
                        int32_t *frame_lengths, void *workspace, size_t workspace_bytes, void *stream);

/* ---- SpecAugment ------------------------------------------------------------------------------------------------------------
 * Time warp, frequency masks and time masks (Park et al., 2019) on the model's channels_first input, as ONE launch:
 * x and out are contiguous (batch, planes, rows, frames), in_dtype / out_dtype (qk_dtype_t) any of fp32, bf16, fp16 on either side.
 * One time-frequency cell of the input is one quaternion (planes r / i / j / k = the static value and its first three time
 * derivatives), so every plane of an utterance gets the SAME warp and the SAME masks.  out must not overlap x (the warp reads
 * neighbouring frames): QK_ERR_INVALID_ARG.  The call does not synchronise, needs no workspace and uses no atomics; the draws are a
 * counter-based hash of (seed, *counter_dev, utterance, draw index) as for qk_postop_t.drop_seed_dev: bit-repeatable, and new on
 * every replay of a captured graph whose counter a device op advances.  seed and utterance index enter the key as a sum: callers
 * that augment different data with one policy (data-parallel ranks) use seeds at least `batch` apart.
 *
 * Random draws (uint32 arithmetic, mod 2^32):
 *   fmix(h):  h ^= h>>16; h *= 0x85EBCA6B; h ^= h>>13; h *= 0xC2B2AE35; h ^= h>>16
 *   key = seed + 0x9E3779B1 * counter,  counter = counter_dev ? *counter_dev : 0
 *   u(b,k) = fmix(fmix(key + b) ^ (k * 0x9E3779B1 + 0x7F4A7C15))
 *   randint(b,k,m) = (uint64(u(b,k)) * m) >> 32, a value in [0, m), for m >= 1
 *   draw indices k: 0 the warp centre, 1 the warp shift; 2+2i and 3+2i the width and start of frequency mask i; 18+2i and 19+2i
 *   the width and start of time mask i.
 * Utterance length: per utterance b, n = clamp(lengths[b], 0, frames).
 * Time warp: active iff time_warp = W >= 1 and n >= 2W + 3.
 *   c = W + 1 + randint(b,0, n - 2W - 2);  w = randint(b,1, 2W + 1) - W;  c' = c + w, which lies in [1, n-2].
 *   t <= c':  num = t c, den = c'.       t > c':  num = c (n-1-c') + (t-c') (n-1-c), den = n-1-c'.
 *   Index arithmetic is exact integer arithmetic, 64-bit where 32 bits could overflow.
 *   i0 = num / den, r = num % den, frac = float(r) / float(den);  y = x[i0] + frac (x[min(i0+1, n-1)] - x[i0]), computed in fp32.
 *   Frames 0, c' and n-1 map onto frames 0, c and n-1 exactly.  When the warp is inactive, c = w = 0 and y = x.
 * Frequency mask i < freq_masks:  fw = randint(b,2+2i, min(freq_width, rows) + 1);  f0 = randint(b,3+2i, rows - fw + 1).
 * Time mask i < time_masks:  cap = min(time_width, (int)floorf((float)n * time_ratio)), one fp32 product;
 *   tw = randint(b,18+2i, cap + 1);  t0 = randint(b,19+2i, n - tw + 1).
 * Output: for t < n the value is `fill` if the row lies in any frequency mask [f0, f0 + fw) or the frame lies in any time mask
 *   [t0, t0 + tw), otherwise the warped value; the same cells are masked in every plane; masks apply after the warp; the value
 *   is rounded once to out_dtype at the store.  For t >= n: out = x converted to out_dtype; nothing from a frame >= n reaches a
 *   frame < n.  With no warp, no masks and equal dtypes the result is a bit copy.
 * Plan row (plan: (batch, QK_SPECAUG_PLAN_WORDS) int32, or NULL): {n, c, w, 0, (f0, fw) x 8, (t0, tw) x 8}, unused masks 0, 0.
 * QK_ERR_INVALID_ARG: mask counts outside 0 .. QK_SPECAUG_MAX_MASKS, negative widths or a negative warp, time_ratio outside [0, 1]
 *   or not finite, fill not finite, batch / planes / rows / frames < 1, a NULL x / lengths / policy / out.  QK_ERR_UNSUPPORTED: a
 *   tensor of 2^31 elements or more.
 * Deviation from the paper: the derivative planes are warped like the static plane; they are NOT rescaled by the local slope of
 * the warp (augmenting the static rows before the deltas, inside the front end's kernels, would be exact). */
#define QK_SPECAUG_MAX_MASKS 8
#define QK_SPECAUG_PLAN_WORDS 36
typedef struct qk_specaug_t {
    int32_t time_warp;       /* W: the warp moves one frame by up to W frames; 0: off */
    int32_t freq_masks;      /* 0 .. QK_SPECAUG_MAX_MASKS */
    int32_t freq_width;      /* largest width of a frequency mask, rows */
    int32_t time_masks;      /* 0 .. QK_SPECAUG_MAX_MASKS */
    int32_t time_width;      /* largest width of a time mask, frames ... */
    float time_ratio;        /* ... and at most this share of the utterance's n frames; in [0, 1] */
    float fill;              /* value of a masked cell (0 = the row mean after per-utterance normalisation) */
    uint32_t seed;
} qk_specaug_t;
int qk_spec_augment(int32_t in_dtype, int32_t out_dtype, int32_t batch, int32_t planes, int32_t rows, int32_t frames,
                    const void *x, const int32_t *lengths, const qk_specaug_t *policy, const uint32_t *counter_dev /* NULL: 0 */,
                    void *out, int32_t *plan /* (batch, 36) or NULL */, void *stream);

/* ---- Speed and volume perturbation ------------------------------------------------------------------------------------------
 * The waveform augmentation of Ko et al., 2015 ("Audio augmentation for speech recognition"), in front of qk_fbank_quaternion,
 * as ONE launch: every utterance is resampled by one of the policy's speeds p/q (tempo and pitch change together, as `sox speed`
 * does: a speed above 1 shortens the utterance) and multiplied by a random linear gain.  wave is a contiguous (batch, max_samples)
 * matrix of wave_dtype (QK_WAVE_I16 or QK_WAVE_F32, as for the front end), lengths (batch) int32 the valid samples per row; out is
 * a contiguous (batch, out_samples) fp32 matrix at the input's scale (int16 input stays in [-32768, 32767] times the gain),
 * out_lengths (batch) int32.  The launch also writes out_lengths and the plan; it does not synchronise, needs no workspace and
 * uses no atomics.  The draws are the counter-based hash of the SpecAugment section: bit-repeatable from (seed, *counter_dev), and
 * new on every replay of a captured graph whose counter a device op advances.  Seeds of data-parallel ranks: as for SpecAugment.
 *
 * Per utterance b, with n = clamp(lengths[b], 0, max_samples):
 * Draws: fmix, key, u(b,k) and randint(b,k,m) exactly as in the SpecAugment section, with draw indices k = 64 (the speed) and
 *   k = 65 (the gain).  i = randint(b,64, n_speeds).  f = float(u(b,65) >> 8) * 2^-24 (exact, in [0, 1)).
 *   g = gain_lo + (gain_hi - gain_lo) * f in fp32: the difference, the product and the sum are each rounded once (no fused
 *   multiply-add), so gain_lo == gain_hi gives g = gain_lo exactly.
 * Length: p = num[i], q = den[i];  n' = ceil(n q / p);  out_lengths[b] = n';  out[b, m] = 0 for n' <= m < out_samples.
 * p == q:  out[b, m] = g * x[b, m] for m < n', one fp32 product and no filter; with g == 1 the result is a bit copy.
 * Otherwise, for m < n':  i0 = (m p) / q, r = (m p) % q in integer arithmetic (i0 <= n - 1 always holds);
 *   acc = sum_{j = -Kw}^{Kw+1} T_i[r][j] * x[b, i0 + j], with x taken as 0 outside [0, n); products and sums are fp32, in any
 *   order, fused or not;  out[b, m] = g * acc, one more fp32 product.
 * Nothing from a sample >= n of an input row ever reaches the output, whatever it holds (NaN included).
 * Filter table: built by the HOST in float64 and rounded once to fp32; the device only forms dot products, and no sinf result is
 *   part of this contract.  It is the band-limited windowed sinc of torchaudio's sinc_interp_hann with Z zero crossings:
 *   fc = rolloff * min(1, q / p);  Kw = half_width[i] = ceil(Z / fc);  for r in [0, q) and j in [-Kw, Kw + 1]:
 *   t = fc * (r / q - j);  T[r][j] = fc * sinc(t) * cos^2(pi t / (2 Z)) for |t| < Z and 0 otherwise;  sinc(t) = sin(pi t) / (pi t),
 *   sinc(0) = 1.  No per-phase normalisation.  tables + table_offset[i] holds the q phases of speed i, each 2 Kw + 2 consecutive
 *   floats (j ascending), phase r first float at r (2 Kw + 2).  A speed with num == den has no table (half_width 0; its table_offset
 *   is not read).  Z = 6 and rolloff = 0.99 give Kw = 7, 16 taps, for 9/10 and 11/10.  tables must be 4-byte aligned.
 * Plan row (plan: (batch, QK_SPEED_PLAN_WORDS) int32, or NULL): {n, i, n', the bits of g}.
 * qk_speed_perturb_out_samples: the largest ceil(max_samples q / p) over the policy's speeds -- the width the caller gives `out`,
 *   known without reading anything from the device; -1 for a NULL or invalid policy or max_samples < 1.
 * QK_ERR_INVALID_ARG: n_speeds outside 1 .. QK_SPEED_MAX_SPEEDS; a num or den outside 1 .. QK_SPEED_MAX_DEN or a ratio outside
 *   [1/2, 2]; half_width 0 where num != den, nonzero where num == den, or negative; a negative table_offset; gains not finite,
 *   negative, or gain_lo > gain_hi; out_samples below qk_speed_perturb_out_samples; out overlapping wave; a wave_dtype other than
 *   the two; a NULL wave / lengths / policy / out / out_lengths, or NULL tables when a speed has num != den; batch or
 *   max_samples < 1; pointers not aligned to their element size.
 * QK_ERR_UNSUPPORTED: 2 Kw + 2 > QK_SPEED_MAX_TAPS; max_samples or out_samples >= 2^26 (below it m p and n q fit 32 bits). */
#define QK_SPEED_MAX_SPEEDS 8
#define QK_SPEED_MAX_DEN    32
#define QK_SPEED_MAX_TAPS   64
#define QK_SPEED_PLAN_WORDS 4
typedef struct qk_speed_perturb_t {
    int32_t n_speeds;                              /* 1 .. QK_SPEED_MAX_SPEEDS */
    int32_t num[QK_SPEED_MAX_SPEEDS];              /* speed i = num[i] / den[i], both in 1 .. QK_SPEED_MAX_DEN, 1/2 <= num/den <= 2 */
    int32_t den[QK_SPEED_MAX_SPEEDS];
    int32_t half_width[QK_SPEED_MAX_SPEEDS];       /* Kw of speed i; 0 when num == den */
    int32_t table_offset[QK_SPEED_MAX_SPEEDS];     /* first float of speed i's taps in `tables` */
    float gain_lo, gain_hi;                        /* linear amplitude factor drawn from [gain_lo, gain_hi); lo == hi: constant */
    uint32_t seed;
} qk_speed_perturb_t;
int64_t qk_speed_perturb_out_samples(int64_t max_samples, const qk_speed_perturb_t *policy);
int qk_speed_perturb(int32_t wave_dtype, int32_t batch, int64_t max_samples, const void *wave, const int32_t *lengths,
                     const qk_speed_perturb_t *policy, const float *tables /* device */, const uint32_t *counter_dev /* NULL: 0 */,
                     int64_t out_samples, float *out, int32_t *out_lengths, int32_t *plan /* (batch, 4) or NULL */, void *stream);

/* ---- Reverberation and additive noise ---------------------------------------------------------------------------------------
 * The environmental corruption of Kaldi's `wav-reverberate` (Ko et al., 2017, "A study on data augmentation of reverberant speech
 * for robust speech recognition"), in front of qk_fbank_quaternion and behind qk_speed_perturb: every utterance is, with
 * probability rir_prob, convolved with one room impulse response of a bank, and gets, with probability noise_prob, one recording
 * of a noise bank added at a signal-to-noise ratio drawn from [snr_lo, snr_hi) dB.  wave is a contiguous (batch, max_samples)
 * matrix of wave_dtype (QK_WAVE_I16 or QK_WAVE_F32), lengths (batch) int32 the valid samples per row; out is a contiguous
 * (batch, max_samples) fp32 matrix at the input's scale.  The length of an utterance does not change: there is no out_lengths.
 * rirs is a (n_rirs, rir_stride) fp32 matrix on the device, row i holding rir_len[i] taps whose direct path is tap rir_delay[i];
 * noises a (n_noises, noise_stride) fp32 matrix, row i holding noise_len[i] samples; rows need 4-byte alignment only.  The call
 * is at most three launches on `stream` (two here: the filter with the energy partials, then the gain and the mix; the second is
 * left out when no noise can fire), reads nothing on the host, does not synchronise and uses no atomics, so it captures into a
 * graph; the draws are the counter-based hash of the SpecAugment section: bit-repeatable from (seed, *counter_dev), and new on
 * every replay of a captured graph whose counter a device op advances.  Seeds of data-parallel ranks: as for SpecAugment.
 * Utterances whose do_rir is false do no convolution work.  The caller owns the workspace (qk_noise_reverb_workspace_bytes,
 * 8-byte aligned): it holds the float64 energy partials of every tile of every utterance; r lives in `out` between the launches.
 *
 * Per utterance b, with n = clamp(lengths[b], 0, max_samples):
 * Draws: fmix, key, u(b,k) and randint(b,k,m) exactly as in the SpecAugment section, with draw indices k = 72 .. 77 (0 .. 33 and
 *   64, 65 are taken by SpecAugment and the speed perturbation):
 *   do_rir = n_rirs > 0 && (u(b,72) >> 8) < rir_prob_q24;        ri = randint(b,73, n_rirs)
 *   do_noise = n_noises > 0 && (u(b,74) >> 8) < noise_prob_q24;  ni = randint(b,75, n_noises);  o = randint(b,76, noise_len[ni])
 *   f = float(u(b,77) >> 8) * 2^-24 (exact, in [0, 1));  snr = snr_lo + (snr_hi - snr_lo) * f in fp32: the difference, the product
 *   and the sum are each rounded once (no fused multiply-add), so snr_lo == snr_hi gives exactly that value.
 *   The probabilities are integers in 0 .. 2^24 (probability p: round(p 2^24)); 2^24 always fires, 0 never does.
 * Reverberation: h = rirs + ri * rir_stride, Lr = rir_len[ri], d = rir_delay[ri].  For 0 <= m < n:
 *   r[m] = sum_{j=0}^{Lr-1} h[j] * x[b, m + d - j], with x taken as 0 outside [0, n): sample m of the output lines up with sample m
 *   of the input through the direct path, so the labels keep their places.  Products and sums are fp32, in any order, fused or
 *   not (the sum starts from +0, and taps beyond Lr enter as zeros: a -0 may come out as +0, and x must be finite).
 *   do_rir false: r[m] = float(x[b, m]), a bit copy for fp32 input.
 * Noise: v[m] = noises[ni * noise_stride + (o + m) % noise_len[ni]] -- the recording starts at o and wraps around.
 *   Es = sum_{m<n} r[m]^2, En = sum_{m<n} v[m]^2: the fp32 values are squared and summed in float64, in a fixed order.
 *   a = float(sqrt(Es / En) * 10^(-snr / 20)), evaluated in float64 and rounded once; a = 0 when En == 0 or Es == 0.
 *   out[b, m] = r[m] + a * v[m]: one fp32 product and one fp32 sum, or one fused multiply-add (a == 0: out = r, v is not read).
 *   do_noise false: out = r.
 * out[b, m] = +0 for n <= m < max_samples.
 * Containment: nothing from an input sample >= n reaches the output, whatever it holds (NaN included), and nothing at or beyond
 *   rir_len[i] / noise_len[i] of a bank row is ever read.
 * Plan row (plan: (batch, QK_NOISE_REVERB_PLAN_WORDS) int32, or NULL): {n, do_rir ? ri : -1, do_noise ? ni : -1, o, the bits of
 *   snr, the bits of a, the bits of float(Es), the bits of float(En)}; o, a, Es and En are 0 when do_noise is false.
 * Decided on the host, before anything touches the device --
 * QK_ERR_INVALID_ARG: a NULL wave / lengths / policy / out / workspace; batch or max_samples < 1; a wave_dtype other than the two;
 *   a negative n_rirs or n_noises; rirs / rir_len / rir_delay NULL while n_rirs > 0, noises / noise_len NULL while n_noises > 0;
 *   rir_stride or noise_stride < 1 (an empty bank gives 1); a probability outside 0 .. 2^24; snr bounds not finite or snr_lo > snr_hi; out
 *   overlapping wave; workspace_bytes below qk_noise_reverb_workspace_bytes; a pointer not aligned to its element size (the
 *   workspace: 8 bytes).
 * QK_ERR_UNSUPPORTED: rir_stride > QK_REVERB_MAX_TAPS; max_samples >= 2^26.
 * NOT checked -- they live on the device, and are the caller's duty (qcnn_amd.functional.prepare_rirs / prepare_noises guarantee
 *   them): rir_len[i] in 1 .. rir_stride, rir_delay[i] in 0 .. rir_len[i] - 1, noise_len[i] in 1 .. noise_stride.  The kernels
 *   clamp what they read into these ranges, so a bad bank gives a wrong signal, not a stray read.
 * qk_noise_reverb_workspace_bytes: known without reading anything from the device; -1 for batch < 1, max_samples < 1 or
 *   max_samples >= 2^26. */
#define QK_REVERB_MAX_TAPS 8192
#define QK_NOISE_REVERB_PLAN_WORDS 8
typedef struct qk_noise_reverb_t {
    int32_t n_rirs;                                /* rows of `rirs`; 0: no reverberation */
    int32_t rir_stride;                            /* floats per row of `rirs`, 1 .. QK_REVERB_MAX_TAPS */
    int32_t n_noises;                              /* rows of `noises`; 0: no noise */
    int32_t noise_stride;                          /* floats per row of `noises` */
    int32_t rir_prob_q24;                          /* probability of reverberation times 2^24, in 0 .. 2^24 */
    int32_t noise_prob_q24;                        /* probability of noise times 2^24, in 0 .. 2^24 */
    float snr_lo, snr_hi;                          /* signal-to-noise ratio in dB, drawn from [snr_lo, snr_hi); lo == hi: constant */
    uint32_t seed;
} qk_noise_reverb_t;
int64_t qk_noise_reverb_workspace_bytes(int32_t batch, int64_t max_samples);
int qk_noise_reverb(int32_t wave_dtype, int32_t batch, int64_t max_samples, const void *wave, const int32_t *lengths,
                    const qk_noise_reverb_t *policy,
                    const float *rirs, const int32_t *rir_len, const int32_t *rir_delay,      /* device; NULL when n_rirs == 0 */
                    const float *noises, const int32_t *noise_len,                            /* device; NULL when n_noises == 0 */
                    const uint32_t *counter_dev /* NULL: 0 */, float *out, int32_t *plan /* (batch, 8) or NULL */,
                    void *workspace, int64_t workspace_bytes, void *stream);

/* Softmax over the last axis of a (rows, cols <= 64) matrix, one wave per row -- the activation of the model's
 * TimeDistributed(Dense(62, activation='softmax')) output layer (models/interspeech_model.py:171-175) and its autodiff:
 *   fwd   y = softmax(logits + bias)          logits: fp32 (the GEMM's fp32 output), bias: fp32 or NULL, y: `dtype`
 *   bwd   dlogits = y * (dy - sum_j dy_j y_j)   (dtype; the operand of the layer's two gradient GEMMs)
 *         dbias[j] += sum over rows of dlogits  (fp32, ACCUMULATED: the caller zeroes it or hands in a gradient buffer; NULL = skip)
 * (Round 6: the model's output layer runs qk_dense_softmax_fwd / _bwd below; these two remain for callers that bring their own
 * logits -- the A/B composition behind QK_DBG_NO_FUSED_SOFTMAX.) */
int qk_softmax_rows_fwd(int32_t dtype, int64_t rows, int32_t cols, const float *logits, const float *bias, void *y, void *stream);
int qk_softmax_rows_bwd(int32_t dtype, int64_t rows, int32_t cols, const void *y, const void *dy, void *dlogits, float *dbias, void *stream);
/* The whole output layer as ONE launch per direction (round 6; csrc/qk_out_layer.hip) -- keras Dense(units, activation='softmax') on
 * the last axis of a (rows, in_dim) 16-bit matrix with fp32 master weights (models/interspeech_model.py:171-175 of the reference:
 * TimeDistributed(Dense(62, activation='softmax')), 51 200 rows x 256 at B = 256):
 *   fwd   y = softmax(x kernel + bias)                       x, y: `dtype` (QK_BF16 / QK_F16); kernel (in_dim, units), bias (units) fp32, bias may be NULL
 *   bwd   dl = s * y * (dy - sum_j dy_j y_j);  dx = dl kernel^T  (dtype);   s = (dy_scale_dev ? *dy_scale_dev : 1) * dy_scale -- a DEVICE
 *         scalar (fp32; NULL = 1) times a host factor: lets a loss node hand over an unscaled d loss / d y and its upstream gradient
 *         separately (the batch mean of qk_ctc_batch_cost: no elementwise pass over dy in between); applied in fp32;
 *         dkernel += x^T dl,  dbias += column sums of dl     (fp32, ACCUMULATED: the caller zeroes them or hands in gradient buffers; NULL = skip)
 * The products run on v_mfma_f32_16x16x32 with fp32 accumulation on the 16-bit roundings of kernel and dl; the softmax sees fp32 logits.
 * Supported: in_dim in {64, 128, 256}, 2 <= units <= 64 and even, 16-bit dtypes (qk_dense_softmax_supported; QK_ERR_UNSUPPORTED
 * otherwise -- the caller composes the layer from its parts).  The backward's workspace (caller-owned, qk_dense_softmax_bwd_workspace_bytes
 * for the CURRENT device; not needed when dkernel and dbias are both NULL) holds one slab of gradient partials per workgroup; a second
 * small launch sums the slabs in a fixed order: no float atomics, bit-repeatable gradients without QK_DBG_DETERMINISTIC. */
int qk_dense_softmax_supported(int32_t dtype, int64_t rows, int32_t in_dim, int32_t units);
int qk_dense_softmax_fwd(int32_t dtype, int64_t rows, int32_t in_dim, int32_t units, const void *x, const float *kernel, const float *bias,
                         void *y, void *stream);
size_t qk_dense_softmax_bwd_workspace_bytes(int32_t dtype, int64_t rows, int32_t in_dim, int32_t units);
int qk_dense_softmax_bwd(int32_t dtype, int64_t rows, int32_t in_dim, int32_t units, const void *x, const float *kernel, const void *y,
                         const void *dy, void *dx, float *dkernel, float *dbias, const float *dy_scale_dev, float dy_scale,
                         void *workspace, size_t workspace_bytes, void *stream);
/* *out += sum_i a[i] * w[i]  (a: `dtype`, w / out: fp32): a linear functional of the model output as one launch. */
int qk_weighted_sum(int32_t dtype, int64_t n, const void *a, const float *w, float *out, void *stream);

/* Batched form of the 16-bit kernel re-layout every forward / backward-data call otherwise does for itself: for job i,
 * write into workspaces[i] what a call of operation ops[i] (QK_OP_FWD, or QK_OP_BWD_DATA / QK_OP_BWD) with descriptor
 * descs[i] and kernel w[i] would write at the start of its workspace -- ONE launch for up to 32 jobs.  Meant to run once
 * behind each optimiser step; the calls of the next training step then pass desc.ws_has_kernel = 1 with those workspaces
 * and launch nothing but their GEMM kernel.  16-bit descriptors only (QK_ERR_INVALID_ARG otherwise); a job whose cq or fq
 * is not a multiple of 16 is SKIPPED, not refused (multiples of 16 are zero-padded to the kernels' 32-channel granule: the
 * workspace holds taps x pad32(cq) x 4 x pad32(fq) 16-bit values + 256 bytes): its calls run the fp32-MFMA kernels, which read the compact kernel in
 * place and never look at the workspace, so a model that mixes on-path and off-path layers hands over all of them. */
int qk_conv_prep_kernels(int32_t n, const qk_conv_desc_t *const *descs, const int32_t *ops, const float *const *w,
                         void *const *workspaces, void *stream);

/* qk_adam_step(_zero_grad) with the model's l2 kernel regularisers folded in.  Keras adds  l2 * sum(w^2)  of every
 * regularised kernel to the loss (models/interspeech_model.py:63,68,173: kernel_regularizer=l2(d.l2)); its gradient
 * 2 * l2 * w is applied here as  g = grad * grad_scale + decay[i] * param[i]  (decay: one coefficient per element,
 * 2 * l2 on regularised kernels and 0 on biases / slopes; NULL = no term).  The backward kernels then remain the
 * only writers of the gradient buffer, which is what lets them add into it directly (QK_BWD_ACCUMULATE) and lets a
 * data-parallel caller send a bucket the moment its last kernel has finished.  zero_grad != 0 clears grad. */
int qk_adam_step_l2(float *param, float *grad, float *m, float *v, const float *decay, size_t n, float lr,
                    float beta1, float beta2, float eps, int32_t step, float grad_scale, int32_t zero_grad,
                    void *stream);

/* qk_adam_step_l2 with the step number ON THE DEVICE: *step_dev = number of steps applied so far (start it at 0).  The kernel
 * applies step *step_dev + 1 (Keras' bias-corrected rate is formed in the kernel, in double as on the host) and a one-thread
 * launch behind it increments the counter.  No launch argument depends on the step, so a training step captured as ONE graph
 * (forward, loss, backward, this call, qk_conv_prep_kernels) replays correctly; hand the same counter to the post-ops
 * (qk_postop_t.drop_seed_dev) and the dropout masks change from replay to replay as well.  Replaces the Keras optimizer's
 * host-side `iterations` variable (the reference trains through Model.fit: /root/reference/models/interspeech_model.py:106,184).
 * decay may be NULL. */
int qk_adam_step_dev(float *param, float *grad, float *m, float *v, const float *decay, size_t n, float lr,
                     float beta1, float beta2, float eps, int32_t *step_dev, float grad_scale, int32_t zero_grad,
                     void *stream);

/* ---- Guarded optimiser step: gradient clipping and dynamic loss scaling, entirely on the device ------------------------------
 * Two calls per training step on the flat fp32 buffers of qk_adam_step_dev:
 *
 *   qk_grad_guard_reduce   one deterministic reduction over the gradient buffer: global l2 norm and the number of non-finite
 *                          elements, then the decisions of the step, written into a 32-byte DEVICE state block;
 *   qk_adam_step_guarded   qk_adam_step_dev that reads those decisions from the block.
 *
 * No launch argument depends on data and nothing is read on the host, so the pair is captured into a graph with the rest of the
 * training step; the reduction uses no atomics and a grid that depends on n alone, so its result is bit-repeatable and ranks
 * that reduced the same (all-reduced) buffer take the same decision.
 *
 * Mirrors keras.optimizers.Adam(clipnorm=, clipvalue=) of Keras 2 (Optimizer.get_gradients): clipnorm is the GLOBAL clip --
 * every gradient is multiplied by clipnorm / norm when the l2 norm over ALL of them exceeds clipnorm -- and clipvalue clamps each
 * element to [-clipvalue, clipvalue] AFTER that.  The gradient the norm is taken of is the one Adam consumes,
 * g_i = grad_i * unscale (+ decay_i * param_i), i.e. including the l2 regularisers' term, as in Keras where that term is part of
 * the loss.  ONE deviation from Keras: a step whose gradient holds an inf or a NaN is SKIPPED (param, m, v and the step counter
 * stay as they are), and with `dynamic` set the loss scale backs off on such a step and grows after growth_interval applied steps
 * in a row -- dynamic loss scaling for float16 training; Keras 2 has neither the skip nor the scale. */
typedef struct qk_grad_guard_config_t {
    float clipnorm;          /* > 0: global-norm clip; 0: off */
    float clipvalue;         /* > 0: element clamp behind the norm clip; 0: off */
    int32_t dynamic;         /* != 0: qk_grad_guard_reduce updates state.scale (below) */
    float growth_factor;     /* > 1 */
    float backoff_factor;    /* in (0, 1) */
    int32_t growth_interval; /* >= 1 */
    float min_scale;         /* 0 < min_scale <= max_scale */
    float max_scale;
} qk_grad_guard_config_t;

/* The state block, in DEVICE memory (32 bytes, 4-byte aligned; the caller initialises scale, good_steps and skipped_steps --
 * scale to the loss scale the backward was run with, 1 without loss scaling -- and may read it back at any time).  `scale` is
 * the value the NEXT backward has to multiply its gradient by: hand a pointer to it to whatever forms the loss gradient. */
typedef struct qk_grad_guard_state_t {
    float scale;             /* current loss scale (updated by qk_grad_guard_reduce when config.dynamic) */
    int32_t good_steps;      /* applied steps since the scale last changed (dynamic only) */
    int32_t skipped_steps;   /* steps skipped so far (dynamic only) */
    int32_t last_skipped;    /* 1: the step just reduced holds a non-finite gradient and is not applied */
    float last_norm;         /* its l2 norm; +inf when nonfinite_count > 0 (or when the norm exceeds fp32) */
    float last_coef;         /* (clipnorm > 0 && norm > clipnorm) ? clipnorm / norm : 1 */
    float last_unscale;      /* grad_scale / scale with the scale the step was RUN with (before the update) */
    int32_t nonfinite_count; /* inf / NaN elements among the g_i (saturates at INT32_MAX) */
} qk_grad_guard_state_t;

/* Bytes of workspace qk_grad_guard_reduce needs for n elements (host only; positive, non-decreasing in n). */
size_t qk_grad_guard_workspace_bytes(size_t n);

/* norm = sqrt(sum g_i^2), g_i = grad_i * unscale (+ decay_i * param_i) formed in fp32 with unscale = grad_scale / state->scale
 * (fp32), the squares summed in fp64 (gradients of 1e25 do not overflow the sum); non-finite g_i are counted on the elements.
 * Stage one writes one partial per workgroup into `workspace` (grid-stride, grid capped and a function of n only), stage two --
 * one workgroup -- adds them in index order and then writes last_norm, nonfinite_count, last_skipped, last_coef and last_unscale
 * and, with config->dynamic: skipped step: scale = max(scale * backoff_factor, min_scale), good_steps = 0, skipped_steps += 1;
 * applied step: good_steps += 1 and at growth_interval scale = min(scale * growth_factor, max_scale), good_steps = 0.
 * param and decay are both NULL or both given.  grad (and param, decay) need 4-byte alignment only: views at any element offset
 * of a flat buffer are read with 16-byte loads behind a peeled head.  workspace: 16-byte aligned. */
int qk_grad_guard_reduce(const float *grad, const float *param, const float *decay, size_t n, float grad_scale,
                         const qk_grad_guard_config_t *config, qk_grad_guard_state_t *state, void *workspace,
                         size_t workspace_bytes, void *stream);

/* qk_adam_step_dev on  g = (grad * state->last_unscale (+ decay * param)) * state->last_coef, clamped to +-config->clipvalue when
 * that is > 0.  With state->last_skipped set, param, m, v and *step_dev are left as they are; grad is still cleared when
 * zero_grad != 0 (the inf would otherwise stay in an accumulating buffer).  With clipping off, scale 1 and a finite gradient the
 * results are bit-identical to qk_adam_step_dev's.  Run it behind qk_grad_guard_reduce on the same stream. */
int qk_adam_step_guarded(float *param, float *grad, float *m, float *v, const float *decay, size_t n, float lr,
                         float beta1, float beta2, float eps, int32_t *step_dev, int32_t zero_grad,
                         const qk_grad_guard_config_t *config, const qk_grad_guard_state_t *state, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* QK_H_ */
