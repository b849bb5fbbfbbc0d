// C-ABI front end (include/qk.h): descriptor validation, geometry, kernel selection.
// No device allocation, no host synchronisation, nothing retained after return.
#include <limits.h>
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include "qk_seq.h"

#include <algorithm>
#include <atomic>
#include <mutex>
#include <vector>

namespace qk {

static thread_local char g_err[512] = "";
static thread_local int g_path = QK_PATH_NONE;
void note_path(int p) { g_path = p; }

namespace {
unsigned env_flags()
{
    unsigned f = 0;
    if (getenv("QK_NO_MFMA16")) f |= kDbgNoMfma16;
    if (getenv("QK_NO_BAND16")) f |= kDbgNoBand16;
    if (getenv("QK_NO_BAND32")) f |= kDbgNoBand32;
    if (getenv("QK_WGRAD16_ONE_TAP")) f |= kDbgWgradOneTap;
    if (getenv("QK_BAND16_8WAVES")) f |= kDbgBand8Waves;
    if (getenv("QK_NO_WGRAD_BAND")) f |= kDbgNoWgradBand;
    if (getenv("QK_NO_POINT16")) f |= kDbgNoPoint16;
    if (getenv("QK_CTC_TWO_SWEEPS")) f |= kDbgCtcTwoSweeps;
    if (getenv("QK_DETERMINISTIC")) f |= kDbgDeterministic;
    if (getenv("QK_WGRAD_BAND_V1")) f |= kDbgWgradBandV1;
    if (getenv("QK_NO_SMALL16")) f |= kDbgNoSmall16;
    // graph-level switches: stored here, acted on by the host-side model code (include/qk.h)
    if (getenv("QK_NO_CONV_CHAIN")) f |= QK_DBG_NO_CONV_CHAIN;
    if (getenv("QK_NO_FUSED_PRELU")) f |= QK_DBG_NO_FUSED_PRELU;
    if (getenv("QK_NO_FUSED_DROPOUT")) f |= QK_DBG_NO_FUSED_DROPOUT;
    if (getenv("QK_NO_FUSED_CTC")) f |= QK_DBG_NO_FUSED_CTC;
    if (getenv("QK_NO_FUSED_FIRST")) f |= QK_DBG_NO_FUSED_FIRST;
    if (getenv("QK_NO_DENSE_IN_CHAIN")) f |= QK_DBG_NO_DENSE_IN_CHAIN;
    if (getenv("QK_NO_FUSED_SOFTMAX")) f |= QK_DBG_NO_FUSED_SOFTMAX;
    if (getenv("QK_NO_MASK_BITS")) f |= QK_DBG_NO_MASK_BITS;
    if (const char *ab = getenv("QK_ABLATE")) f |= ((unsigned)atoi(ab) << kDbgAblateShift) & kDbgAblateMask;
    return f;
}
std::atomic<unsigned> &dbg_word()
{
    static std::atomic<unsigned> w{env_flags()};          // thread-safe one-time initialisation (C++11)
    return w;
}
struct ForceCfg { bool set; int policy, bq; };
const ForceCfg &force_cfg()
{
    static const ForceCfg fc = [] {
        ForceCfg c = {false, -1, -1};
        if (const char *f = getenv("QK_FORCE_CFG")) c.set = sscanf(f, "%d,%d", &c.policy, &c.bq) == 2;
        return c;
    }();
    return fc;
}
}  // namespace

unsigned debug_flags() { return dbg_word().load(std::memory_order_relaxed); }
static std::atomic<unsigned long long *> g_dbg_buf{nullptr};
static std::atomic<size_t> g_dbg_bytes{0};
unsigned long long *debug_buffer(size_t *bytes) { if (bytes) *bytes = g_dbg_bytes.load(); return g_dbg_buf.load(); }

// ---- per-call timing (qk_prof_*, include/qk.h) ------------------------------------------------------------------
// Off: one relaxed atomic load per compute call.  On: a pair of HIP events around the call's launches ON THE CALLER'S
// STREAM, kept in a process-wide list until the next qk_prof_enable(1); qk_prof_get synchronises the pair it reads.
// This is how bench.py times the kernels INSIDE the training step (autograd runs the backward on another thread and
// several kernels per C call, so neither Python-side events nor per-kernel wrappers can).
namespace {
struct ProfRec { int op, dtype, path; long long rows; int n, k; hipEvent_t e0, e1; };
struct Prof { std::mutex mu; std::atomic<int> on{0}; std::vector<ProfRec> recs; };
Prof &prof() { static Prof p; return p; }
}  // namespace
static thread_local int g_prof_nest = 0;     // a call that re-enters the front end (channels_first re-layout) is timed once, as a whole
struct ProfScope {
    bool live = false;
    ProfRec r;
    hipStream_t stream;
    ProfScope(int op, const qk_conv_desc_t *d, hipStream_t st) : stream(st)
    {
        if (g_prof_nest++ > 0) return;
        if (!prof().on.load(std::memory_order_relaxed) || !d) return;
        r.op = op; r.dtype = d->dtype; r.path = QK_PATH_NONE;
        r.rows = (long long)d->batch * d->out_spatial[0] * d->out_spatial[1] * d->out_spatial[2];
        r.n = 4 * d->fq;
        r.k = 4 * d->cq * d->kernel[0] * d->kernel[1] * d->kernel[2];
        if (hipEventCreate(&r.e0) != hipSuccess) return;
        if (hipEventCreate(&r.e1) != hipSuccess) { (void)hipEventDestroy(r.e0); return; }
        live = hipEventRecord(r.e0, stream) == hipSuccess;
    }
    ~ProfScope()
    {
        --g_prof_nest;
        if (!live) return;
        (void)hipEventRecord(r.e1, stream);
        r.path = g_path;
        std::lock_guard<std::mutex> lk(prof().mu);
        prof().recs.push_back(r);
    }
};
bool debug_force_cfg(int *policy, int *bq)
{
    const ForceCfg &c = force_cfg();
    if (c.set) { *policy = c.policy; *bq = c.bq; }
    return c.set;
}
int device_cu_count()
{
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0)
        return 256;
    return n;
}

void set_error(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

#define QK_DECL(sfx)                                                                              \
    int launch_hgemm_##sfx(const void *, const void *, const float *, const float *, void *,      \
                           const GemmGeom &, bool, hipStream_t);                                  \
    int launch_wgrad_##sfx(const void *, const void *, const void *, float *, float *,            \
                           const WgradGeom &, bool, hipStream_t);
QK_DECL(f32)
QK_DECL(bf16)
QK_DECL(f16)
#undef QK_DECL

// 16-bit-input MFMA fast path (qk_hgemm_bf16mfma.hip); returns 1 when it took the call
int try_hgemm_16(int dtype, const void *in, const void *mask, const float *w_f32, const float *bias,
                 void *out, const GemmGeom &g, bool w_is_transposed, void *ws, size_t ws_bytes,
                 hipStream_t stream);

// kernel a call carrying a bit-packed kind-2 mask would reach: 2 = band, 1 = point, 0 = none (qk_hgemm_bf16mfma.hip)
int hgemm16_bits_route(int dtype, const GemmGeom &g);

// 16-bit-input MFMA backward-weight, band form (qk_wgrad_band_bf16mfma.hip); returns 1 when it took the call
int try_wgrad_band_16(int dtype, const void *x, const void *dy, const void *ymask, float *dw, float *dbias,
                      const WgradGeom &g, hipStream_t stream);
// 16-bit-input MFMA backward-weight (qk_wgrad_bf16mfma.hip); returns 1 when it took the call
int try_wgrad_16(int dtype, const void *x, const void *dy, const void *ymask, float *dw, float *dbias,
                 const WgradGeom &g, hipStream_t stream);

int launch_hgemm(int dtype, const void *in, const void *mask, const float *wk, const float *bias,
                 void *out, const GemmGeom &g, bool vec_ok, hipStream_t stream)
{
    switch (dtype) {
    case QK_F32: return launch_hgemm_f32(in, mask, wk, bias, out, g, vec_ok, stream);
    case QK_BF16: return launch_hgemm_bf16(in, mask, wk, bias, out, g, vec_ok, stream);
    case QK_F16: return launch_hgemm_f16(in, mask, wk, bias, out, g, vec_ok, stream);
    }
    return QK_ERR_INVALID_ARG;
}

int launch_wgrad(int dtype, const void *x, const void *dy, const void *ymask, float *dw,
                 float *dbias, WgradGeom g, bool vec_ok, hipStream_t stream)
{
    switch (dtype) {
    case QK_F32: return launch_wgrad_f32(x, dy, ymask, dw, dbias, g, vec_ok, stream);
    case QK_BF16: return launch_wgrad_bf16(x, dy, ymask, dw, dbias, g, vec_ok, stream);
    case QK_F16: return launch_wgrad_f16(x, dy, ymask, dw, dbias, g, vec_ok, stream);
    }
    return QK_ERR_INVALID_ARG;
}

namespace {

// 4-element vector loads need 16 B (f32) / 8 B (16-bit) alignment
bool vec_aligned(const void *p, int dtype) { return aligned(p, 4 * elem_size(dtype)); }

int validate(const qk_conv_desc_t *d, bool allow_rank0)
{
    if (!d) { set_error("descriptor is NULL"); return QK_ERR_INVALID_ARG; }
    if (d->rank < (allow_rank0 ? 0 : 1) || d->rank > 3) {
        set_error("rank %d not in [1,3]", d->rank); return QK_ERR_INVALID_ARG;
    }
    if (d->batch <= 0 || d->cq <= 0 || d->fq <= 0) {
        set_error("batch/cq/fq must be positive (got %d/%d/%d)", d->batch, d->cq, d->fq);
        return QK_ERR_INVALID_ARG;
    }
    long long si = 1, so = 1, taps = 1;
    for (int i = 0; i < 3; ++i) {
        if (d->in_spatial[i] <= 0 || d->out_spatial[i] <= 0 || d->kernel[i] <= 0 ||
            d->stride[i] <= 0 || d->dilation[i] <= 0 || d->pad_lo[i] < 0) {
            set_error("axis %d: extents/kernel/stride/dilation must be > 0 and pad_lo >= 0", i);
            return QK_ERR_INVALID_ARG;
        }
        if (i >= d->rank && (d->in_spatial[i] != 1 || d->out_spatial[i] != 1 || d->kernel[i] != 1 ||
                             d->stride[i] != 1 || d->dilation[i] != 1 || d->pad_lo[i] != 0)) {
            set_error("axis %d is beyond rank %d and must be the identity (1,1,1,1,1,0)", i, d->rank);
            return QK_ERR_INVALID_ARG;
        }
        si *= d->in_spatial[i]; so *= d->out_spatial[i]; taps *= d->kernel[i];
    }
    // kernels index rows and elements with 32-bit integers
    if (si * d->batch * 4LL * d->cq > INT_MAX || so * d->batch * 4LL * d->fq > INT_MAX ||
        taps * d->cq * 4LL * d->fq > INT_MAX) {
        set_error("tensor with >= 2^31 elements: split the batch"); return QK_ERR_UNSUPPORTED;
    }
    if (d->layout != QK_CH_LAST && d->layout != QK_CH_FIRST) { set_error("bad layout %d", d->layout); return QK_ERR_INVALID_ARG; }
    if (d->dtype != QK_F32 && d->dtype != QK_BF16 && d->dtype != QK_F16) { set_error("bad dtype %d", d->dtype); return QK_ERR_INVALID_ARG; }
    if (d->activation != QK_ACT_LINEAR && d->activation != QK_ACT_RELU) { set_error("bad activation %d", d->activation); return QK_ERR_INVALID_ARG; }
    if (d->kernel_order != QK_KERNEL_TAPS_MAJOR && d->kernel_order != QK_KERNEL_CHANNEL_MAJOR) { set_error("bad kernel_order %d", d->kernel_order); return QK_ERR_INVALID_ARG; }
    if (d->kernel_order == QK_KERNEL_CHANNEL_MAJOR && (d->dtype == QK_F32 || d->layout != QK_CH_LAST || d->cq % 32 || d->fq % 32)) {
        set_error("kernel_order = QK_KERNEL_CHANNEL_MAJOR is served by the 16-bit matrix-core kernels only (16-bit dtype, channels_last, cq and fq multiples of 32)");
        return QK_ERR_UNSUPPORTED;
    }
    return 0;
}

// a channel-major kernel (qk_conv_desc_t.kernel_order) that the 16-bit kernels declined must not fall through to kernels that read taps-major
int refuse_ch_major(const qk_conv_desc_t *d, const char *what)
{
    if (d->kernel_order != QK_KERNEL_CHANNEL_MAJOR) return 0;
    set_error("%s: kernel_order = QK_KERNEL_CHANNEL_MAJOR, but the 16-bit matrix-core path did not take this shape (workspace, alignment or a diagnostic switch)", what);
    return QK_ERR_UNSUPPORTED;
}

struct Strides { long long sn, ss[3], sc; long long flat_ss; };

// element strides of an activation tensor with `ch` channels and spatial extents sp
Strides act_strides(const int32_t *sp, int ch, int layout)
{
    Strides s;
    const long long S = (long long)sp[0] * sp[1] * sp[2];
    if (layout == QK_CH_LAST) {
        s.sc = 1; s.ss[2] = ch; s.ss[1] = (long long)sp[2] * ch; s.ss[0] = (long long)sp[1] * sp[2] * ch;
        s.sn = S * ch; s.flat_ss = ch;
    } else {
        s.sc = S; s.ss[2] = 1; s.ss[1] = sp[2]; s.ss[0] = (long long)sp[1] * sp[2];
        s.sn = S * ch; s.flat_ss = 1;
    }
    return s;
}

int taps_of(const qk_conv_desc_t *d) { return d->kernel[0] * d->kernel[1] * d->kernel[2]; }

// qk_postop_t -> kernel form; `rank` / `sp` describe the tensor the post-op acts on
int to_postop(const qk_postop_t *q, int rank, const int32_t *sp, PostOp *p)
{
    memset(p, 0, sizeof(*p));
    if (!q) return 0;
    if (!(q->drop_rate >= 0.f && q->drop_rate < 1.f)) { set_error("post-op: drop_rate %g out of range", (double)q->drop_rate); return QK_ERR_INVALID_ARG; }
    if (!q->alpha) {
        // relu + dropout: y = drop(relu(pre)), one output tensor, the backward reads y only (qk_postop.h, kind 2)
        p->kind = 2; p->alpha_sel = -1; p->alpha_len = 0; p->alpha = nullptr;
    } else {
        if (q->alpha_axis < -1 || q->alpha_axis >= (rank > 0 ? rank : 1)) {
            set_error("post-op: alpha_axis %d out of range", q->alpha_axis); return QK_ERR_INVALID_ARG;
        }
        const int want = q->alpha_axis < 0 ? 1 : sp[q->alpha_axis];
        if (q->alpha_len != want) { set_error("post-op: alpha_len %d, expected %d", q->alpha_len, want); return QK_ERR_INVALID_ARG; }
        p->kind = 1; p->alpha_sel = q->alpha_axis; p->alpha_len = q->alpha_len; p->alpha = q->alpha;
    }
    p->drop_scale = 1.f / (1.f - q->drop_rate);
    unsigned thr = (unsigned)(q->drop_rate * 256.f + 0.5f);      // 8 random bits per element: rates are multiples of 1/256
    p->drop_thr = thr > 255u ? 255u : thr;
    p->drop_scale = p->drop_thr ? 256.f / (256.f - (float)p->drop_thr) : 1.f;   // the scale of the rate actually applied
    p->drop_seed = q->drop_seed;
    p->seed_dev = q->drop_seed_dev;
    return 0;
}

// the post-op as its own elementwise pass over a channels_last (batch, sp, ch) tensor
int postop_pass(int dtype, bool backward, const PostOp &p, int batch, const int32_t *sp, int ch, const void *pre,
                const void *dy, void *out, float *dalpha, hipStream_t stream)
{
    const long long rows = (long long)batch * sp[0] * sp[1] * sp[2];
    int key_div = 1, key_mod = 1;
    if (p.alpha_sel >= 0) { for (int i = p.alpha_sel + 1; i < 3; ++i) key_div *= sp[i]; key_mod = sp[p.alpha_sel]; }
    const int vec = dtype == QK_F32 ? 4 : 8;
    if (ch % vec != 0 || !aligned(pre, 16) || !aligned(out, 16) || (dy && !aligned(dy, 16))) {
        set_error("post-op: channels must be a multiple of %d and buffers 16-byte aligned", vec); return QK_ERR_UNSUPPORTED;
    }
    if (backward && p.alpha_len > 256) { set_error("post-op: alpha_len %d > 256", p.alpha_len); return QK_ERR_UNSUPPORTED; }
    if (rows * ch >= (1ll << 32)) { set_error("post-op: tensor has >= 2^32 elements"); return QK_ERR_UNSUPPORTED; }
    return launch_postop(dtype, backward, pre, dy, out, dalpha, p, rows, ch, key_div, key_mod, stream);
}

size_t w_floats(const qk_conv_desc_t *d) { return (size_t)taps_of(d) * d->cq * 4 * d->fq; }

size_t dy_bytes(const qk_conv_desc_t *d)
{
    const size_t e = (size_t)d->batch * d->out_spatial[0] * d->out_spatial[1] * d->out_spatial[2] * 4 * d->fq;
    return (e * elem_size(d->dtype) + 255) / 256 * 256;
}

// ---- channels_first 16-bit buffers on the matrix cores ----------------------------------------------------------
// The 16-bit MFMA kernels want the reduction axis (channels) contiguous.  A QK_CH_FIRST descriptor with 16-bit
// activations is therefore served by re-laying its operands out to channels_last in the caller's workspace
// (k_relayout16: HBM-bound, 64 x 64 tiles through LDS), running the channels_last kernels -- post-ops, chain flags,
// accumulation included -- and re-laying the result back.  Costs one extra read + write of every activation operand
// (~0.15 ms per 367 MB tensor) instead of the 10x slower general fp32 kernels that served these descriptors before.
// (The engine's own layers keep channels_first tensors physically channels-last and never come here; this is for a
// binder that holds true NCHW buffers.)
bool cf16_ok(const qk_conv_desc_t *d)
{
    if (d->layout != QK_CH_FIRST || d->dtype == QK_F32 || (debug_flags() & kDbgNoMfma16)) return false;
    if (d->cq % 32 || d->fq % 32 || taps_of(d) > 32) return false;
    for (int i = 0; i < 3; ++i) if (d->stride[i] != 1) return false;
    return true;
}
size_t x_bytes16(const qk_conv_desc_t *d) { return align256((size_t)d->batch * d->in_spatial[0] * d->in_spatial[1] * d->in_spatial[2] * 4 * d->cq * 2); }
size_t y_bytes16(const qk_conv_desc_t *d) { return align256((size_t)d->batch * d->out_spatial[0] * d->out_spatial[1] * d->out_spatial[2] * 4 * d->fq * 2); }
int in_positions(const qk_conv_desc_t *d) { return d->in_spatial[0] * d->in_spatial[1] * d->in_spatial[2]; }
int out_positions(const qk_conv_desc_t *d) { return d->out_spatial[0] * d->out_spatial[1] * d->out_spatial[2]; }
qk_conv_desc_t as_ch_last(const qk_conv_desc_t *d) { qk_conv_desc_t c = *d; c.layout = QK_CH_LAST; return c; }
// x-shaped / y-shaped tensor: channels_first -> channels_last and back
int x_to_last(const qk_conv_desc_t *d, const void *src, void *dst, hipStream_t s) { return launch_relayout16(src, dst, d->batch, 4 * d->cq, in_positions(d), s); }
int x_to_first(const qk_conv_desc_t *d, const void *src, void *dst, hipStream_t s) { return launch_relayout16(src, dst, d->batch, in_positions(d), 4 * d->cq, s); }
int y_to_last(const qk_conv_desc_t *d, const void *src, void *dst, hipStream_t s) { return launch_relayout16(src, dst, d->batch, 4 * d->fq, out_positions(d), s); }
int y_to_first(const qk_conv_desc_t *d, const void *src, void *dst, hipStream_t s) { return launch_relayout16(src, dst, d->batch, out_positions(d), 4 * d->fq, s); }

// Every descriptor-derived field of the implicit-GEMM geometry (GemmGeom, qk_common.h) of a forward or a backward-data call.
// The one place that knows them: the calls, qk_conv_fold_taps, the workspace size and qk_conv_prep_kernels all start here, so what
// small16_shape / band_geom decide about the LAYOUT of a cached workspace is decided on the fields the call itself dispatches on
// (neither reads sign_tbl, w_prepped or w_ch_major).  Call-specific fields -- relu, has_bias, has_mask, the post-op, ep_mask,
// w_swapped -- stay zero for the caller to set.
GemmGeom make_geom(const qk_conv_desc_t *d, bool bwd)
{
    GemmGeom g;
    memset(&g, 0, sizeof(g));
    const Strides xs = act_strides(d->in_spatial, 4 * d->cq, d->layout);
    const Strides ys = act_strides(d->out_spatial, 4 * d->fq, d->layout);
    const Strides &in = bwd ? ys : xs, &out = bwd ? xs : ys;               // backward-data gathers dy and produces dx
    const int32_t *isp = bwd ? d->out_spatial : d->in_spatial, *osp = bwd ? d->in_spatial : d->out_spatial;
    g.batch = d->batch;
    g.M = d->batch * osp[0] * osp[1] * osp[2];
    g.Q = bwd ? d->fq : d->cq; g.J = bwd ? d->cq : d->fq; g.taps = taps_of(d);
    for (int i = 0; i < 3; ++i) {
        g.osp[i] = osp[i]; g.isp[i] = isp[i]; g.ks[i] = d->kernel[i];
        if (!bwd) { g.pa[i] = d->stride[i]; g.pb[i] = d->dilation[i]; g.pc[i] = -d->pad_lo[i]; g.pd[i] = 1; }
        else { g.pa[i] = 1; g.pb[i] = -d->dilation[i]; g.pc[i] = d->pad_lo[i]; g.pd[i] = d->stride[i]; }      // the position map inverted
        g.in_ss[i] = in.ss[i];
    }
    g.in_sn = in.sn; g.in_sc = in.sc;
    g.out_sn = out.sn; g.out_ss = out.flat_ss; g.out_sc = out.sc;
    g.sign_tbl = (d->conj != 0) == bwd ? kSignConv : kSignConj;            // backward-data: the transposed table
    g.w_prepped = d->ws_has_kernel ? 1 : 0;
    g.w_ch_major = d->kernel_order == QK_KERNEL_CHANNEL_MAJOR;
    return g;
}

// The workspace of one operation of a descriptor that the channels_last kernels serve:
//   [band-layout 16-bit image of the kernel + zero line][fragment layout of k_hconv16_small][relu-masked dy]
// 16-bit forward / backward-data read the first region (the fp32-MFMA kernels read the compact kernel in place and need nothing);
// 16 / 32-channel layers keep the small-channel kernel's layout in a second region behind it (go16 finds it at `band`); the fused
// backward of a relu layer adds the masked copy of dy that backward-weight writes for backward-data.
struct KernelWs {
    size_t band;        // first region
    size_t small;       // second region (0: the shape has none), at offset `band`
    Small16 sm;         // its geometry (small != 0)
    size_t dym;         // offset of the masked dy (QK_OP_BWD of a relu layer)
    size_t total;
};
KernelWs kernel_ws(const qk_conv_desc_t *d, int op)
{
    KernelWs k;
    memset(&k, 0, sizeof(k));
    const bool bwd_data = op == QK_OP_BWD_DATA || op == QK_OP_BWD;
    if (d->dtype != QK_F32 && (op == QK_OP_FWD || bwd_data)) {
        // channel counts that are multiples of 16: zero-padded to the kernels' 32-channel granule (other counts never reach the
        // 16-bit kernels; their figure is what it always was)
        const bool on16 = d->cq % 16 == 0 && d->fq % 16 == 0;
        k.band = on16 ? band_image_bytes(taps_of(d), pad32(d->cq), pad32(d->fq)) : w_floats(d) * 2 + 256;
        GemmGeom bg;
        if (on16 && d->layout == QK_CH_LAST && d->kernel_order != QK_KERNEL_CHANNEL_MAJOR && small16_shape(make_geom(d, bwd_data), &bg, &k.sm))
            k.small = small16_region_bytes(k.sm);
    }
    k.total = k.band + k.small;
    if (op == QK_OP_BWD && d->activation == QK_ACT_RELU) { k.dym = align256(k.total); k.total = k.dym + dy_bytes(d); }
    return k;
}

// The workspace of one operation of a cf16_ok descriptor: [what the channels_last call needs: `base` bytes][one slot per operand
// re-laid out to channels_last].  Forward: x, y, pre (of a PReLU post-op); backward-data: dy, y, dx, the dx mask / x_pre;
// backward-weight: x, dy, y (its channels_last call takes no workspace: base is 0 and the slots start the buffer); fused
// backward: x, dx, dy, y -- reported as never less than the backward-data and backward-weight figures, which the un-fused forms
// of that call (a linear layer, qk_conv_bwd_post) run in the same buffer.
struct CfPlan {
    size_t base;
    size_t x, dx, dy, y, pre;       // slot offsets (those the operation uses), in the order listed above
    size_t used;                    // end of the slots (a call that leaves its LAST slot unused -- forward: pre, backward-weight: y -- needs the buffer up to that slot only)
    size_t total;                   // what qk_*_workspace_bytes reports
};
CfPlan cf_plan(const qk_conv_desc_t *d, int op)
{
    const qk_conv_desc_t c = as_ch_last(d);
    const size_t X = x_bytes16(d), Y = y_bytes16(d);
    CfPlan p;
    memset(&p, 0, sizeof(p));
    size_t at = p.base = align256(kernel_ws(&c, op).total);
    auto slot = [&at](size_t bytes) { const size_t o = at; at += bytes; return o; };
    switch (op) {
    case QK_OP_FWD: p.x = slot(X); p.y = slot(Y); p.pre = slot(Y); break;
    case QK_OP_BWD_DATA: p.dy = slot(Y); p.y = slot(Y); p.dx = slot(X); p.pre = slot(X); break;
    case QK_OP_BWD_WEIGHT: p.x = slot(X); p.dy = slot(Y); p.y = slot(Y); break;
    case QK_OP_BWD: p.x = slot(X); p.dx = slot(X); p.dy = slot(Y); p.y = slot(Y); break;
    }
    p.used = p.total = at;
    if (op == QK_OP_BWD) {
        const size_t bd = cf_plan(d, QK_OP_BWD_DATA).total, bw = cf_plan(d, QK_OP_BWD_WEIGHT).total;
        if (bd > p.total) p.total = bd;
        if (bw > p.total) p.total = bw;
    }
    return p;
}

size_t ws_bytes_impl(const qk_conv_desc_t *d, int op) { return cf16_ok(d) ? cf_plan(d, op).total : kernel_ws(d, op).total; }

// the forward call of qk_conv_fwd_post(_bits) as the 16-bit dispatcher sees it (call-specific fields of the geometry)
bool fwd_post_geom(const qk_conv_desc_t *d, const PostOp &post, const void *pre, const void *y, GemmGeom *g)
{
    *g = make_geom(d, false);
    g->relu = d->activation == QK_ACT_RELU;
    g->has_bias = d->has_bias ? 1 : 0;
    if (d->dtype == QK_F32 || !post.kind || d->layout != QK_CH_LAST || !aligned(pre, 16) || !aligned(y, 16) ||
        (long long)g->M * 4 * d->fq >= (1ll << 32)) return false;         // the dropout hash indexes elements with 32 bits
    g->post = post; g->post_fwd = 1; g->pre_out = post.kind == 1 ? const_cast<void *>(pre) : nullptr;
    return true;
}

int conv_fwd_impl(const qk_conv_desc_t *d, const void *x, const float *w, const float *bias, void *y,
                  void *ws, size_t wsb, hipStream_t stream, const PostOp *post = nullptr, void *pre = nullptr,
                  void *mask_bits = nullptr)
{
    if (!x || !w || !y) { set_error("x/w/y must not be NULL"); return QK_ERR_INVALID_ARG; }
    if (d->has_bias && !bias) { set_error("has_bias set but bias is NULL"); return QK_ERR_INVALID_ARG; }
    ProfScope prof_scope(QK_OP_FWD, d, stream);
    if (mask_bits) {
        // the bit-packed mask is written by ONE kernel family's epilogue: that kernel or an error
        GemmGeom g;
        if (cf16_ok(d) || !post || post->kind != 2 || !fwd_post_geom(d, *post, pre, y, &g)) { set_error("mask bits: relu-form post-op on 16-bit channels_last tensors only"); return QK_ERR_UNSUPPORTED; }
        g.bits_out = mask_bits;
        const int r = try_hgemm_16(d->dtype, x, nullptr, w, bias, y, g, false, ws, wsb, stream);
        if (r == 0 || r == QK_ERR_UNSUPPORTED) { set_error("mask bits: no forward kernel writes them for this layer (qk_conv_mask_bits_bytes)"); return QK_ERR_UNSUPPORTED; }
        return r < 0 ? r : 0;
    }
    if (cf16_ok(d)) {
        const qk_conv_desc_t c = as_ch_last(d);
        const CfPlan p = cf_plan(d, QK_OP_FWD);
        const bool two = post && post->kind == 1;
        if (ws && aligned(ws, 16) && wsb >= (two ? p.used : p.pre)) {
            char *b = static_cast<char *>(ws);
            void *xt = b + p.x, *yt = b + p.y, *pt = two ? b + p.pre : nullptr;
            if (int rc = x_to_last(d, x, xt, stream)) return rc;
            if (int rc = conv_fwd_impl(&c, xt, w, bias, yt, ws, p.base, stream, post, pt)) return rc;
            if (int rc = y_to_first(d, yt, y, stream)) return rc;
            return two ? y_to_first(d, pt, pre, stream) : 0;
        }
    }
    GemmGeom g = make_geom(d, false);
    g.relu = d->activation == QK_ACT_RELU;
    g.has_bias = d->has_bias ? 1 : 0;
    const bool with_post = post && post->kind;
    if (d->dtype != QK_F32) {
        if (with_post && d->layout == QK_CH_LAST && aligned(pre, 16) && aligned(y, 16) &&
            (long long)g.M * 4 * d->fq < (1ll << 32)) {                 // the dropout hash indexes elements with 32 bits
            g.post = *post; g.post_fwd = 1; g.pre_out = post->kind == 1 ? pre : nullptr;
        }
        const int r = try_hgemm_16(d->dtype, x, nullptr, w, bias, y, g, false, ws, wsb, stream);
        if (r != 0) return r < 0 ? r : 0;
        g.post.kind = 0; g.post_fwd = 0; g.pre_out = nullptr;
    }
    if (int rc = refuse_ch_major(d, "forward")) return rc;
    const bool vec = d->layout == QK_CH_LAST && d->cq % 4 == 0 && d->fq % 4 == 0 &&
                     vec_aligned(x, d->dtype) && aligned(w, 16);
    note_path(QK_PATH_FP32_MFMA);
    if (!with_post) return launch_hgemm(d->dtype, x, nullptr, w, bias, y, g, vec, stream);
    // general path: the convolution writes pre (kind 2: into y, in place), the post-op runs as its own pass
    if (d->layout != QK_CH_LAST) { set_error("post-op needs channels_last buffers"); return QK_ERR_UNSUPPORTED; }
    void *lin = post->kind == 1 ? pre : y;
    if (int rc = launch_hgemm(d->dtype, x, nullptr, w, bias, lin, g, vec, stream)) return rc;
    return postop_pass(d->dtype, false, *post, d->batch, d->out_spatial, 4 * d->fq, lin, nullptr, y, nullptr, stream);
}

int conv_bwd_data_impl(const qk_conv_desc_t *d, const void *dy, const void *y, const float *w, void *dx,
                       void *ws, size_t wsb, hipStream_t stream, const void *dx_mask = nullptr,
                       const PostOp *post = nullptr, float *dalpha = nullptr, const void *dx_mask_bits = nullptr)
{
    // post != NULL: dx_mask holds the PRE-activation of x (x = post(x_pre); kind 2: x itself); dx returns d loss / d x_pre
    const bool with_post = post && post->kind;
    if (!dy || !w || !dx) { set_error("dy/w/dx must not be NULL"); return QK_ERR_INVALID_ARG; }
    const bool mask = d->activation == QK_ACT_RELU;
    if (mask && !y) { set_error("activation is RELU: the forward output y is required"); return QK_ERR_INVALID_ARG; }
    const size_t need = ws_bytes_impl(d, QK_OP_BWD_DATA);
    if (need && (!ws || wsb < need)) {
        set_error("bwd_data needs %zu workspace bytes, got %zu", need, wsb);
        return QK_ERR_WORKSPACE;
    }
    if (need && !aligned(ws, 16)) { set_error("workspace must be 16-byte aligned"); return QK_ERR_WORKSPACE; }
    ProfScope prof_scope(QK_OP_BWD_DATA, d, stream);
    if (dx_mask_bits) {
        // (bit-packed kind-2 mask of x in place of dx_mask: the band / point kernels' epilogue or an error)
        if (cf16_ok(d) || mask || !with_post || post->kind != 2 || d->dtype == QK_F32 || d->layout != QK_CH_LAST || !aligned(dx_mask_bits, 16)) {
            set_error("mask bits: relu-form post-op on 16-bit channels_last tensors, 16-byte aligned bits"); return QK_ERR_UNSUPPORTED;
        }
        GemmGeom g = make_geom(d, true);
        g.post = *post; g.ep_bits = dx_mask_bits;
        const int r = try_hgemm_16(d->dtype, dy, nullptr, w, nullptr, dx, g, true, ws, wsb, stream);
        if (r == 0 || r == QK_ERR_UNSUPPORTED) { set_error("mask bits: no backward-data kernel reads them for this layer (qk_conv_bwd_reads_mask_bits)"); return QK_ERR_UNSUPPORTED; }
        return r < 0 ? r : 0;
    }
    if (cf16_ok(d)) {
        // (`need` above is this plan's total: every slot fits)
        const qk_conv_desc_t c = as_ch_last(d);
        const CfPlan p = cf_plan(d, QK_OP_BWD_DATA);
        char *b = static_cast<char *>(ws);
        void *dyt = b + p.dy, *yt = mask ? b + p.y : nullptr, *dxt = b + p.dx, *mt = dx_mask ? b + p.pre : nullptr;
        if (int rc = y_to_last(d, dy, dyt, stream)) return rc;
        if (mask) if (int rc = y_to_last(d, y, yt, stream)) return rc;
        if (dx_mask) if (int rc = x_to_last(d, dx_mask, mt, stream)) return rc;
        if (int rc = conv_bwd_data_impl(&c, dyt, yt, w, dxt, ws, p.base, stream, mt, post, dalpha)) return rc;
        return x_to_first(d, dxt, dx, stream);
    }
    GemmGeom g = make_geom(d, true);
    g.has_mask = mask ? 1 : 0;
    if (d->dtype != QK_F32) {
        // the 16-bit kernels apply an epilogue mask themselves (needs 16-byte aligned rows of dx_mask)
        g.ep_mask = (dx_mask && aligned(dx_mask, 16)) ? dx_mask : nullptr;
        const bool fuse_post = with_post && g.ep_mask && post->alpha_len <= 256 && d->layout == QK_CH_LAST;
        if (fuse_post) { g.post = *post; g.dalpha = dalpha; }
        else if (with_post) g.ep_mask = nullptr;
        const int r = try_hgemm_16(d->dtype, dy, mask ? y : nullptr, w, nullptr, dx, g, true, ws, wsb, stream);
        if (r < 0) return r;
        if (r > 0) {
            if (with_post && !fuse_post)
                return postop_pass(d->dtype, true, *post, d->batch, d->in_spatial, 4 * d->cq, dx_mask, dx, dx, dalpha, stream);
            if (dx_mask && !g.ep_mask) return launch_mask_gt0(d->dtype, dx, dx_mask, (size_t)g.M * 4 * d->cq, stream);
            return 0;
        }
        g.ep_mask = nullptr; g.post.kind = 0; g.dalpha = nullptr;
    }
    if (int rc = refuse_ch_major(d, "backward-data")) return rc;
    // the fp32-MFMA kernel stages the compact kernel in place with the channel/filter roles swapped
    g.w_swapped = 1;
    const bool vec = d->layout == QK_CH_LAST && d->cq % 4 == 0 && d->fq % 4 == 0 && aligned(w, 16) &&
                     vec_aligned(dy, d->dtype) && (!mask || vec_aligned(y, d->dtype));
    note_path(QK_PATH_FP32_MFMA);
    if (int rc = launch_hgemm(d->dtype, dy, mask ? y : nullptr, w, nullptr, dx, g, vec, stream)) return rc;
    if (with_post) {
        if (d->layout != QK_CH_LAST) { set_error("post-op needs channels_last buffers"); return QK_ERR_UNSUPPORTED; }
        return postop_pass(d->dtype, true, *post, d->batch, d->in_spatial, 4 * d->cq, dx_mask, dx, dx, dalpha, stream);
    }
    if (dx_mask) return launch_mask_gt0(d->dtype, dx, dx_mask, (size_t)g.M * 4 * d->cq, stream);
    return 0;
}

int conv_bwd_weight_impl(const qk_conv_desc_t *d, const void *x, const void *dy, const void *y, float *dw,
                         float *dbias, void *dy_masked_out, hipStream_t stream, bool accumulate = false,
                         void *ws = nullptr, size_t wsb = 0)
{
    if (!x || !dy || !dw) { set_error("x/dy/dw must not be NULL"); return QK_ERR_INVALID_ARG; }
    const bool mask = d->activation == QK_ACT_RELU;
    if (mask && !y) { set_error("activation is RELU: the forward output y is required"); return QK_ERR_INVALID_ARG; }
    if (d->has_bias && !dbias) { set_error("has_bias set but dbias is NULL"); return QK_ERR_INVALID_ARG; }
    ProfScope prof_scope(QK_OP_BWD_WEIGHT, d, stream);
    if (cf16_ok(d)) {
        // (ws, wsb): the caller's workspace, used for the re-layout; no masked dy is left behind in this mode
        const qk_conv_desc_t c = as_ch_last(d);
        const CfPlan p = cf_plan(d, QK_OP_BWD_WEIGHT);
        if (ws && aligned(ws, 16) && wsb >= (mask ? p.used : p.y)) {
            char *b = static_cast<char *>(ws);
            void *xt = b + p.x, *dyt = b + p.dy, *yt = mask ? b + p.y : nullptr;
            if (int rc = x_to_last(d, x, xt, stream)) return rc;
            if (int rc = y_to_last(d, dy, dyt, stream)) return rc;
            if (mask) if (int rc = y_to_last(d, y, yt, stream)) return rc;
            return conv_bwd_weight_impl(&c, xt, dyt, yt, dw, dbias, nullptr, stream, accumulate);
        }
        dy_masked_out = nullptr;               // (the workspace may be too small to double as the masked-dy output)
    }
    WgradGeom g;
    memset(&g, 0, sizeof(g));
    const Strides xs = act_strides(d->in_spatial, 4 * d->cq, d->layout);
    const Strides dys = act_strides(d->out_spatial, 4 * d->fq, d->layout);
    g.batch = d->batch;
    g.M = d->batch * d->out_spatial[0] * d->out_spatial[1] * d->out_spatial[2];
    g.Cq = d->cq; g.F = d->fq; g.taps = taps_of(d);
    for (int i = 0; i < 3; ++i) {
        g.osp[i] = d->out_spatial[i]; g.isp[i] = d->in_spatial[i]; g.ks[i] = d->kernel[i];
        g.pa[i] = d->stride[i]; g.pb[i] = d->dilation[i]; g.pc[i] = -d->pad_lo[i];
        g.x_ss[i] = xs.ss[i];
    }
    g.x_sn = xs.sn; g.x_sc = xs.sc;
    g.dy_sn = dys.sn; g.dy_ss = dys.flat_ss; g.dy_sc = dys.sc;
    g.sign_tbl = d->conj ? kSignConj : kSignConv;
    g.has_mask = mask ? 1 : 0;
    g.want_dbias = (d->has_bias && dbias) ? 1 : 0;
    g.dym = mask ? dy_masked_out : nullptr;
    g.w_ch_major = d->kernel_order == QK_KERNEL_CHANNEL_MAJOR;
    // dw / dbias are accumulated atomically: zero them first (one fill when they are adjacent, as in
    // a flat gradient buffer)
    const size_t dwb = w_floats(d) * sizeof(float), dbb = 4 * (size_t)d->fq * sizeof(float);
    const char *dw_end = reinterpret_cast<const char *>(dw) + dwb;
    const char *db_c = reinterpret_cast<const char *>(dbias);
    if (accumulate) {
        // the caller's buffers already hold what this call adds to
    } else if (g.want_dbias && (db_c == dw_end ||
                                (db_c > dw_end && db_c - dw_end < 256 && reinterpret_cast<uintptr_t>(db_c) % 256 == 0))) {
        // adjacent, or dbias on the first 256-byte boundary behind dw (a flat gradient buffer with aligned
        // views): the bytes in between are alignment padding by contract (include/qk.h) -- one fill
        if (hipMemsetAsync(dw, 0, (size_t)(db_c - reinterpret_cast<const char *>(dw)) + dbb, stream) != hipSuccess) { set_error("memset dw failed"); return QK_ERR_LAUNCH; }
    } else {
        if (hipMemsetAsync(dw, 0, dwb, stream) != hipSuccess) { set_error("memset dw failed"); return QK_ERR_LAUNCH; }
        if (g.want_dbias && hipMemsetAsync(dbias, 0, dbb, stream) != hipSuccess) { set_error("memset dbias failed"); return QK_ERR_LAUNCH; }
    }
    if (d->dtype != QK_F32) {
        int r = g.w_ch_major ? 0 : try_wgrad_band_16(d->dtype, x, dy, mask ? y : nullptr, dw, dbias, g, stream);     // (the band kernels write taps-major only)
        if (r == 0) r = try_wgrad_16(d->dtype, x, dy, mask ? y : nullptr, dw, dbias, g, stream);
        if (r != 0) return r < 0 ? r : 0;
    }
    if (int rc = refuse_ch_major(d, "backward-weight")) return rc;
    const bool vec = d->layout == QK_CH_LAST && d->cq % 4 == 0 && d->fq % 4 == 0 &&
                     vec_aligned(x, d->dtype) && vec_aligned(dy, d->dtype) && (!mask || vec_aligned(y, d->dtype));
    note_path(QK_PATH_FP32_MFMA);
    return launch_wgrad(d->dtype, x, dy, mask ? y : nullptr, dw, dbias, g, vec, stream);
}

// Fused backward: bwd-weight first (it reads dy and y once and, for RELU, also writes the masked dy
// into the workspace), then bwd-data on the masked copy with no mask loads of its own.
int conv_bwd_impl(const qk_conv_desc_t *d, const void *x, const void *dy, const void *y, const float *w,
                  void *dx, float *dw, float *dbias, void *ws, size_t wsb, hipStream_t stream, int flags = 0)
{
    if (!dx) { set_error("dx must not be NULL (use qk_*_bwd_weight when d(input) is not needed)"); return QK_ERR_INVALID_ARG; }
    if (flags & ~(QK_BWD_MASK_DX | QK_BWD_DY_PREMASKED | QK_BWD_ACCUMULATE)) { set_error("unknown backward flags 0x%x", flags); return QK_ERR_INVALID_ARG; }
    if (cf16_ok(d)) {
        // one re-layout of x, dy (and y) serves both gradient kernels; dx goes back once
        const qk_conv_desc_t c = as_ch_last(d);
        const CfPlan p = cf_plan(d, QK_OP_BWD);
        const bool need_y = d->activation == QK_ACT_RELU && !(flags & QK_BWD_DY_PREMASKED);
        if (need_y && !y) { set_error("activation is RELU: the forward output y is required"); return QK_ERR_INVALID_ARG; }
        if (!x || !dy) { set_error("x/dy must not be NULL"); return QK_ERR_INVALID_ARG; }
        if (ws && aligned(ws, 16) && wsb >= p.used) {
            char *b = static_cast<char *>(ws);
            void *xt = b + p.x, *dxt = b + p.dx, *dyt = b + p.dy, *yt = need_y ? b + p.y : nullptr;
            if (int rc = x_to_last(d, x, xt, stream)) return rc;
            if (int rc = y_to_last(d, dy, dyt, stream)) return rc;
            if (need_y) if (int rc = y_to_last(d, y, yt, stream)) return rc;
            if (int rc = conv_bwd_impl(&c, xt, dyt, yt, w, dxt, dw, dbias, ws, p.base, stream, flags)) return rc;
            return x_to_first(d, dxt, dx, stream);
        }
    }
    const bool acc = (flags & QK_BWD_ACCUMULATE) != 0;
    const void *dx_mask = (flags & QK_BWD_MASK_DX) ? x : nullptr;
    const bool relu = d->activation == QK_ACT_RELU && !(flags & QK_BWD_DY_PREMASKED);
    const size_t bd = ws_bytes_impl(d, QK_OP_BWD_DATA);
    if (!relu) {
        // linear layer, or dy arrives with the relu mask applied: both gradients straight from dy
        if (bd && (!ws || wsb < bd)) { set_error("bwd needs %zu workspace bytes, got %zu", bd, wsb); return QK_ERR_WORKSPACE; }
        qk_conv_desc_t lin = *d;
        lin.activation = QK_ACT_LINEAR;
        if (int rc = conv_bwd_weight_impl(&lin, x, dy, nullptr, dw, dbias, nullptr, stream, acc)) return rc;
        return conv_bwd_data_impl(&lin, dy, nullptr, w, dx, ws, bd, stream, dx_mask);
    }
    const size_t need = ws_bytes_impl(d, QK_OP_BWD);
    if (need && (!ws || wsb < need)) { set_error("bwd needs %zu workspace bytes, got %zu", need, wsb); return QK_ERR_WORKSPACE; }
    void *dym = static_cast<char *>(ws) + kernel_ws(d, QK_OP_BWD).dym;        // (inside the `need` bytes just checked)
    if (int rc = conv_bwd_weight_impl(d, x, dy, y, dw, dbias, dym, stream, acc)) return rc;
    qk_conv_desc_t lin = *d;
    lin.activation = QK_ACT_LINEAR;
    return conv_bwd_data_impl(&lin, dym, nullptr, w, dx, ws, bd, stream, dx_mask);
}

// qk_dense_desc_t -> the validated descriptor of the rank-0 convolution that computes it
int dense_as_conv(const qk_dense_desc_t *d, qk_conv_desc_t *cp)
{
    if (!d) { set_error("descriptor is NULL"); return QK_ERR_INVALID_ARG; }
    qk_conv_desc_t &c = *cp;
    memset(&c, 0, sizeof(c));
    c.rank = 0; c.batch = d->rows; c.cq = d->in_q; c.fq = d->q_units;
    for (int i = 0; i < 3; ++i) {
        c.in_spatial[i] = c.out_spatial[i] = c.kernel[i] = c.stride[i] = c.dilation[i] = 1;
        c.pad_lo[i] = 0;
    }
    c.layout = QK_CH_LAST; c.dtype = d->dtype; c.activation = d->activation;
    c.has_bias = d->has_bias; c.conj = 1;     // dense.py:139-143 is the transposed table
    c.ws_has_kernel = d->ws_has_kernel;
    return validate(&c, true);
}

// qk_*_bwd_weight[_acc]: the workspace doubles as the masked-dy side output when it can hold one
void *masked_dy_slot(const qk_conv_desc_t *d, void *ws, size_t wsb) { return (ws && wsb >= dy_bytes(d) && aligned(ws, 16)) ? ws : nullptr; }

int check_launch(int rc, const char *what)
{
    if (rc == QK_ERR_LAUNCH) set_error("%s: kernel launch failed: %s", what, hipGetErrorString(hipGetLastError()));
    return rc;
}

// ---- the CTC family: the checks that are the same words in several entry points; `what` is the name inside the message
template <typename... A>
int fail(int rc, const char *fmt, A... a) { set_error(fmt, a...); return rc; }          // the message, then the code
int null_arg(const char *what) { return fail(QK_ERR_INVALID_ARG, "%s: NULL argument", what); }
int lattice_extents_ok(const char *what, int batch, int frames, int classes, int max_label_len)
{
    if (batch > 0 && frames > 0 && classes >= 2 && max_label_len >= 0) return QK_OK;
    return fail(QK_ERR_INVALID_ARG, "%s: bad extents (%d, %d, %d, %d)", what, batch, frames, classes, max_label_len);
}
int count_ok(const char *what, long long elements)          // the kernels index with int
{
    return elements <= INT_MAX ? QK_OK : fail(QK_ERR_UNSUPPORTED, "%s: tensor with >= 2^31 elements", what);
}
int ctc_workspace_ok(const char *what, const void *workspace, size_t given, size_t need, size_t alignment)
{
    if (workspace && given >= need && aligned(workspace, alignment)) return QK_OK;
    return fail(QK_ERR_WORKSPACE, alignment == 8 ? "%s needs %zu workspace bytes (8-byte aligned), got %zu" : "%s needs %zu workspace bytes, got %zu",
                what, need, given);
}

// what qk_ctc_beam_search_decode_lm checks on top of qk_ctc_beam_search_decode, each at its place in the common order
struct BeamLmArgs { int order; const float *table; float weight, bonus; const float *score; };
int beam_args_ok(const char *what, int dtype, int batch, int frames, int classes, const void *y_pred, const int32_t *input_length,
                        int beam_width, int top_paths, const int32_t *decoded, const int32_t *decoded_len, const float *log_prob,
                        const void *workspace, size_t workspace_bytes, const BeamLmArgs *lm)
{
    if (batch <= 0 || frames <= 0 || classes < 2 || beam_width < 1 || top_paths < 1 || dtype < QK_F32 || dtype > QK_F16)
        return fail(QK_ERR_INVALID_ARG, "%s: bad arguments (%d, %d, %d, beam %d, paths %d, dtype %d)", what, batch, frames, classes, beam_width,
                    top_paths, dtype);
    if (lm && (!(lm->weight >= 0.f) || !isfinite(lm->weight) || !isfinite(lm->bonus)))
        return fail(QK_ERR_INVALID_ARG, "%s: lm_weight %g must be finite and >= 0, insertion_bonus %g finite", what, (double)lm->weight,
                    (double)lm->bonus);
    if (lm && (lm->order < 1 || lm->order > 3)) return fail(QK_ERR_UNSUPPORTED, "%s: lm_order %d outside 1 .. 3", what, lm->order);
    if (!y_pred || !input_length || !decoded || !decoded_len || !log_prob || (lm && (!lm->score || !lm->table))) return null_arg(what);
    if (classes > 256 || beam_width > 128 || top_paths > beam_width)
        return fail(QK_ERR_UNSUPPORTED, "%s: unsupported (classes %d <= 256, beam_width %d <= 128, top_paths %d <= beam_width)", what, classes,
                    beam_width, top_paths);
    if (lm && lm->order == 3 && classes > 64) return fail(QK_ERR_UNSUPPORTED, "%s: a trigram LM needs classes %d <= 64", what, classes);
    if (lm && !ctc_beam_lm_supported(classes, beam_width, lm->order))
        return fail(QK_ERR_UNSUPPORTED, "%s: the LM rows of %d beams x %d classes exceed the LDS budget", what, beam_width, classes);
    if (const int rc = count_ok(what, std::max((long long)batch * frames * classes, (long long)top_paths * batch * frames))) return rc;
    return ctc_workspace_ok(what, workspace, workspace_bytes, ctc_beam_workspace_bytes(batch, frames, beam_width), 4);
}

}  // namespace
}  // namespace qk

using namespace qk;

extern "C" {

int qk_version(void) { return QK_VERSION; }

const char *qk_last_error(void) { return g_err; }

unsigned qk_set_debug_flags(unsigned flags) { return dbg_word().exchange(flags, std::memory_order_relaxed); }
void qk_set_debug_buffer(void *device_buffer, size_t bytes) { g_dbg_buf.store(static_cast<unsigned long long *>(device_buffer)); g_dbg_bytes.store(bytes); }
unsigned qk_get_debug_flags(void) { return debug_flags(); }
int qk_last_path(void) { return g_path; }

int qk_prof_enable(int on)
{
    Prof &p = prof();
    std::lock_guard<std::mutex> lk(p.mu);
    const int was = p.on.exchange(on ? 1 : 0, std::memory_order_relaxed);
    if (on) {                                   // a new recording: drop the previous one
        for (ProfRec &r : p.recs) { (void)hipEventDestroy(r.e0); (void)hipEventDestroy(r.e1); }
        p.recs.clear();
    }
    return was;
}
int qk_prof_count(void)
{
    std::lock_guard<std::mutex> lk(prof().mu);
    return (int)prof().recs.size();
}
int qk_prof_get(int i, qk_prof_rec_t *out)
{
    if (!out) { set_error("qk_prof_get: out is NULL"); return QK_ERR_INVALID_ARG; }
    ProfRec r;
    {
        std::lock_guard<std::mutex> lk(prof().mu);
        if (i < 0 || i >= (int)prof().recs.size()) { set_error("qk_prof_get: record %d of %zu", i, prof().recs.size()); return QK_ERR_INVALID_ARG; }
        r = prof().recs[i];
    }
    float ms = 0.f;
    if (hipEventSynchronize(r.e1) != hipSuccess || hipEventElapsedTime(&ms, r.e0, r.e1) != hipSuccess) {
        set_error("qk_prof_get: the events of record %d could not be read", i); return QK_ERR_LAUNCH;
    }
    out->op = r.op; out->dtype = r.dtype; out->path = r.path; out->rows = r.rows; out->n = r.n; out->k = r.k; out->ms = ms;
    return QK_OK;
}

size_t qk_conv_workspace_bytes(const qk_conv_desc_t *desc, int op)
{
    if (validate(desc, false)) return 0;
    return ws_bytes_impl(desc, op);
}

size_t qk_dense_workspace_bytes(const qk_dense_desc_t *desc, int op)
{
    qk_conv_desc_t c;
    if (dense_as_conv(desc, &c)) return 0;
    return ws_bytes_impl(&c, op);
}

int qk_conv_fwd(const qk_conv_desc_t *desc, const void *x, const float *w, const float *bias, void *y,
                void *workspace, size_t workspace_bytes, void *stream)
{
    if (int rc = validate(desc, false)) return rc;
    return check_launch(conv_fwd_impl(desc, x, w, bias, y, workspace, workspace_bytes, (hipStream_t)stream), "qk_conv_fwd");
}

int qk_conv_fwd_post(const qk_conv_desc_t *desc, const qk_postop_t *post, const void *x, const float *w,
                     const float *bias, void *pre, void *y, void *workspace, size_t workspace_bytes, void *stream)
{
    if (int rc = validate(desc, false)) return rc;
    if (!post || (!pre && post->alpha)) { set_error("qk_conv_fwd_post: post must not be NULL, pre only for a relu post-op (alpha == NULL)"); return QK_ERR_INVALID_ARG; }
    if (desc->activation != QK_ACT_LINEAR) { set_error("qk_conv_fwd_post: the convolution must be LINEAR (the post-op is the activation)"); return QK_ERR_INVALID_ARG; }
    PostOp p;
    if (int rc = to_postop(post, desc->rank, desc->out_spatial, &p)) return rc;
    return check_launch(conv_fwd_impl(desc, x, w, bias, y, workspace, workspace_bytes, (hipStream_t)stream, &p, pre), "qk_conv_fwd_post");
}

int qk_conv_bwd_post(const qk_conv_desc_t *desc, const void *x, const void *dy, const float *w, void *dx, float *dw,
                     float *dbias, const qk_postop_t *post_x, const void *x_pre, float *dalpha_x, int32_t flags,
                     void *workspace, size_t workspace_bytes, void *stream)
{
    if (int rc = validate(desc, false)) return rc;
    if (!dx || !post_x) { set_error("qk_conv_bwd_post: dx / post_x must not be NULL"); return QK_ERR_INVALID_ARG; }
    if (post_x->alpha && (!x_pre || !dalpha_x)) { set_error("qk_conv_bwd_post: a PReLU post-op needs x_pre and dalpha_x"); return QK_ERR_INVALID_ARG; }
    if (flags & ~QK_BWD_ACCUMULATE) { set_error("qk_conv_bwd_post: only QK_BWD_ACCUMULATE is a valid flag here (0x%x)", flags); return QK_ERR_INVALID_ARG; }
    if (desc->activation != QK_ACT_LINEAR) { set_error("qk_conv_bwd_post: the layer must be LINEAR"); return QK_ERR_INVALID_ARG; }
    PostOp p;
    if (int rc = to_postop(post_x, desc->rank, desc->in_spatial, &p)) return rc;
    const size_t bd = ws_bytes_impl(desc, QK_OP_BWD_DATA);
    if (bd && (!workspace || workspace_bytes < bd)) { set_error("bwd needs %zu workspace bytes, got %zu", bd, workspace_bytes); return QK_ERR_WORKSPACE; }
    if (int rc = conv_bwd_weight_impl(desc, x, dy, nullptr, dw, dbias, nullptr, (hipStream_t)stream, (flags & QK_BWD_ACCUMULATE) != 0,
                                      workspace, workspace_bytes)) return check_launch(rc, "qk_conv_bwd_post");
    // relu post-op: x = drop(relu(x_pre)) is its own mask (x > 0 <=> x_pre > 0 and kept)
    const void *mask_src = p.kind == 2 ? x : x_pre;
    return check_launch(conv_bwd_data_impl(desc, dy, nullptr, w, dx, workspace, bd, (hipStream_t)stream, mask_src, &p, p.kind == 2 ? nullptr : dalpha_x), "qk_conv_bwd_post");
}

size_t qk_conv_mask_bits_bytes(const qk_conv_desc_t *desc)
{
    if (validate(desc, false) || cf16_ok(desc) || desc->activation != QK_ACT_LINEAR) return 0;
    PostOp p;
    memset(&p, 0, sizeof(p));
    p.kind = 2; p.alpha_sel = -1; p.drop_scale = 1.f;
    GemmGeom g;
    if (!fwd_post_geom(desc, p, nullptr, nullptr, &g)) return 0;
    g.bits_out = &g;                                                    // (any non-NULL value: the route asks only whether it is set)
    if (hgemm16_bits_route(desc->dtype, g) != 2) return 0;
    const size_t bytes = ((size_t)g.M * 4 * desc->fq + 7) / 8;
    return (bytes + 15) / 16 * 16;
}

int qk_conv_bwd_reads_mask_bits(const qk_conv_desc_t *desc)
{
    if (validate(desc, false) || cf16_ok(desc) || desc->activation != QK_ACT_LINEAR || desc->dtype == QK_F32 || desc->layout != QK_CH_LAST) return 0;
    GemmGeom g = make_geom(desc, true);
    g.post.kind = 2; g.post.alpha_sel = -1; g.post.drop_scale = 1.f;
    g.ep_bits = &g;
    return hgemm16_bits_route(desc->dtype, g) != 0 ? 1 : 0;
}

int qk_conv_fwd_post_bits(const qk_conv_desc_t *desc, const qk_postop_t *post, const void *x, const float *w,
                          const float *bias, void *pre, void *y, void *mask_bits, void *workspace, size_t workspace_bytes, void *stream)
{
    if (int rc = validate(desc, false)) return rc;
    if (!post || !mask_bits || !aligned(mask_bits, 16)) { set_error("qk_conv_fwd_post_bits: post / mask_bits must not be NULL, mask_bits 16-byte aligned"); return QK_ERR_INVALID_ARG; }
    if (post->alpha) { set_error("qk_conv_fwd_post_bits: the relu form only (alpha == NULL)"); return QK_ERR_UNSUPPORTED; }
    if (desc->activation != QK_ACT_LINEAR) { set_error("qk_conv_fwd_post_bits: the convolution must be LINEAR (the post-op is the activation)"); return QK_ERR_INVALID_ARG; }
    PostOp p;
    if (int rc = to_postop(post, desc->rank, desc->out_spatial, &p)) return rc;
    return check_launch(conv_fwd_impl(desc, x, w, bias, y, workspace, workspace_bytes, (hipStream_t)stream, &p, pre, mask_bits), "qk_conv_fwd_post_bits");
}

int qk_conv_bwd_post_bits(const qk_conv_desc_t *desc, const void *x, const void *x_mask_bits, const void *dy, const float *w, void *dx,
                          float *dw, float *dbias, const qk_postop_t *post_x, int32_t flags, void *workspace, size_t workspace_bytes,
                          void *stream)
{
    if (int rc = validate(desc, false)) return rc;
    if (!dx || !post_x || !x_mask_bits) { set_error("qk_conv_bwd_post_bits: dx / post_x / x_mask_bits must not be NULL"); return QK_ERR_INVALID_ARG; }
    if (post_x->alpha) { set_error("qk_conv_bwd_post_bits: the relu form only (alpha == NULL)"); return QK_ERR_UNSUPPORTED; }
    if (flags & ~QK_BWD_ACCUMULATE) { set_error("qk_conv_bwd_post_bits: only QK_BWD_ACCUMULATE is a valid flag here (0x%x)", flags); return QK_ERR_INVALID_ARG; }
    if (desc->activation != QK_ACT_LINEAR) { set_error("qk_conv_bwd_post_bits: the layer must be LINEAR"); return QK_ERR_INVALID_ARG; }
    if (!qk_conv_bwd_reads_mask_bits(desc)) { set_error("qk_conv_bwd_post_bits: no backward-data kernel reads mask bits for this layer"); return QK_ERR_UNSUPPORTED; }
    PostOp p;
    if (int rc = to_postop(post_x, desc->rank, desc->in_spatial, &p)) return rc;
    const size_t bd = ws_bytes_impl(desc, QK_OP_BWD_DATA);
    if (bd && (!workspace || workspace_bytes < bd)) { set_error("bwd needs %zu workspace bytes, got %zu", bd, workspace_bytes); return QK_ERR_WORKSPACE; }
    if (int rc = conv_bwd_weight_impl(desc, x, dy, nullptr, dw, dbias, nullptr, (hipStream_t)stream, (flags & QK_BWD_ACCUMULATE) != 0,
                                      workspace, workspace_bytes)) return check_launch(rc, "qk_conv_bwd_post_bits");
    return check_launch(conv_bwd_data_impl(desc, dy, nullptr, w, dx, workspace, bd, (hipStream_t)stream, nullptr, &p, nullptr, x_mask_bits), "qk_conv_bwd_post_bits");
}

static int postop_entry(const qk_conv_desc_t *t, const qk_postop_t *post, bool backward, const void *pre, const void *dy,
                        void *out, float *dalpha, void *stream)
{
    if (!t || !post || !pre || !out || (backward && (!dy || (!dalpha && post->alpha)))) { set_error("post-op: NULL argument"); return QK_ERR_INVALID_ARG; }
    if (t->rank < 0 || t->rank > 3 || t->batch <= 0 || t->fq <= 0) { set_error("post-op: bad tensor description"); return QK_ERR_INVALID_ARG; }
    int32_t sp[3] = {1, 1, 1};
    for (int i = 0; i < t->rank; ++i) { if (t->out_spatial[i] <= 0) { set_error("post-op: bad extent"); return QK_ERR_INVALID_ARG; } sp[i] = t->out_spatial[i]; }
    PostOp p;
    if (int rc = to_postop(post, t->rank, sp, &p)) return rc;
    return check_launch(postop_pass(t->dtype, backward, p, t->batch, sp, 4 * t->fq, pre, dy, out, dalpha, (hipStream_t)stream), "qk_postop");
}

int qk_postop_fwd(const qk_conv_desc_t *t, const qk_postop_t *post, const void *pre, void *y, void *stream)
{
    return postop_entry(t, post, false, pre, nullptr, y, nullptr, stream);
}

int qk_postop_bwd(const qk_conv_desc_t *t, const qk_postop_t *post, const void *pre, const void *dy, void *dpre,
                  float *dalpha, void *stream)
{
    return postop_entry(t, post, true, pre, dy, dpre, dalpha, stream);
}

int qk_conv_bwd_data(const qk_conv_desc_t *desc, const void *dy, const void *y, const float *w, void *dx,
                     void *workspace, size_t workspace_bytes, void *stream)
{
    if (int rc = validate(desc, false)) return rc;
    return check_launch(conv_bwd_data_impl(desc, dy, y, w, dx, workspace, workspace_bytes, (hipStream_t)stream), "qk_conv_bwd_data");
}

int qk_conv_bwd_weight(const qk_conv_desc_t *desc, const void *x, const void *dy, const void *y, float *dw,
                       float *dbias, void *workspace, size_t workspace_bytes, void *stream)
{
    if (int rc = validate(desc, false)) return rc;
    return check_launch(conv_bwd_weight_impl(desc, x, dy, y, dw, dbias, masked_dy_slot(desc, workspace, workspace_bytes), (hipStream_t)stream, false, workspace, workspace_bytes), "qk_conv_bwd_weight");
}

int qk_conv_bwd_chain(const qk_conv_desc_t *desc, const void *x, const void *dy, const void *y, const float *w,
                      void *dx, float *dw, float *dbias, int32_t flags, void *workspace, size_t workspace_bytes,
                      void *stream)
{
    if (int rc = validate(desc, false)) return rc;
    if ((flags & QK_BWD_MASK_DX) && !x) { set_error("QK_BWD_MASK_DX needs x"); return QK_ERR_INVALID_ARG; }
    return check_launch(conv_bwd_impl(desc, x, dy, y, w, dx, dw, dbias, workspace, workspace_bytes, (hipStream_t)stream, flags), "qk_conv_bwd_chain");
}

int qk_dense_bwd_chain(const qk_dense_desc_t *desc, const void *x, const void *dy, const void *y, const float *w,
                       void *dx, float *dw, float *dbias, int32_t flags, void *workspace, size_t workspace_bytes,
                       void *stream)
{
    qk_conv_desc_t c;
    if (int rc = dense_as_conv(desc, &c)) return rc;
    if ((flags & QK_BWD_MASK_DX) && !x) { set_error("QK_BWD_MASK_DX needs x"); return QK_ERR_INVALID_ARG; }
    return check_launch(conv_bwd_impl(&c, x, dy, y, w, dx, dw, dbias, workspace, workspace_bytes, (hipStream_t)stream, flags), "qk_dense_bwd_chain");
}

int qk_conv_bwd_weight_acc(const qk_conv_desc_t *desc, const void *x, const void *dy, const void *y,
                           float *dw, float *dbias, void *workspace, size_t workspace_bytes, void *stream)
{
    if (int rc = validate(desc, false)) return rc;
    return check_launch(conv_bwd_weight_impl(desc, x, dy, y, dw, dbias, masked_dy_slot(desc, workspace, workspace_bytes), (hipStream_t)stream, true, workspace, workspace_bytes), "qk_conv_bwd_weight_acc");
}

int qk_dense_bwd_weight_acc(const qk_dense_desc_t *desc, const void *x, const void *dy, const void *y,
                            float *dw, float *dbias, void *workspace, size_t workspace_bytes, void *stream)
{
    qk_conv_desc_t c;
    if (int rc = dense_as_conv(desc, &c)) return rc;
    return check_launch(conv_bwd_weight_impl(&c, x, dy, y, dw, dbias, masked_dy_slot(&c, workspace, workspace_bytes), (hipStream_t)stream, true), "qk_dense_bwd_weight_acc");
}

int qk_conv_bwd(const qk_conv_desc_t *desc, const void *x, const void *dy, const void *y, const float *w,
                void *dx, float *dw, float *dbias, void *workspace, size_t workspace_bytes, void *stream)
{
    if (int rc = validate(desc, false)) return rc;
    return check_launch(conv_bwd_impl(desc, x, dy, y, w, dx, dw, dbias, workspace, workspace_bytes, (hipStream_t)stream), "qk_conv_bwd");
}

int qk_dense_bwd(const qk_dense_desc_t *desc, const void *x, const void *dy, const void *y, const float *w,
                 void *dx, float *dw, float *dbias, void *workspace, size_t workspace_bytes, void *stream)
{
    qk_conv_desc_t c;
    if (int rc = dense_as_conv(desc, &c)) return rc;
    return check_launch(conv_bwd_impl(&c, x, dy, y, w, dx, dw, dbias, workspace, workspace_bytes, (hipStream_t)stream), "qk_dense_bwd");
}

int qk_dense_fwd(const qk_dense_desc_t *desc, const void *x, const float *w, const float *bias, void *y,
                 void *workspace, size_t workspace_bytes, void *stream)
{
    qk_conv_desc_t c;
    if (int rc = dense_as_conv(desc, &c)) return rc;
    return check_launch(conv_fwd_impl(&c, x, w, bias, y, workspace, workspace_bytes, (hipStream_t)stream), "qk_dense_fwd");
}

int qk_dense_bwd_data(const qk_dense_desc_t *desc, const void *dy, const void *y, const float *w, void *dx,
                      void *workspace, size_t workspace_bytes, void *stream)
{
    qk_conv_desc_t c;
    if (int rc = dense_as_conv(desc, &c)) return rc;
    return check_launch(conv_bwd_data_impl(&c, dy, y, w, dx, workspace, workspace_bytes, (hipStream_t)stream), "qk_dense_bwd_data");
}

int qk_dense_bwd_weight(const qk_dense_desc_t *desc, const void *x, const void *dy, const void *y, float *dw,
                        float *dbias, void *workspace, size_t workspace_bytes, void *stream)
{
    qk_conv_desc_t c;
    if (int rc = dense_as_conv(desc, &c)) return rc;
    return check_launch(conv_bwd_weight_impl(&c, x, dy, y, dw, dbias, masked_dy_slot(&c, workspace, workspace_bytes), (hipStream_t)stream), "qk_dense_bwd_weight");
}

static bool conv1_pool_ok(const qk_conv_desc_t *d, int32_t pool, int act = QK_ACT_RELU)
{
    // layout QK_CH_FIRST here describes x ONLY: (N, 4, H, W), the four component planes; the pooled tensor is channels_last
    return d->rank == 2 && (d->dtype == QK_BF16 || d->dtype == QK_F16) && d->cq == 1 &&
           d->kernel[0] == 3 && d->kernel[1] == 5 && d->stride[0] == 1 && d->stride[1] == 1 && d->dilation[0] == 1 &&
           d->dilation[1] == 1 && d->pad_lo[0] == 1 && d->pad_lo[1] == 2 && d->out_spatial[0] == d->in_spatial[0] &&
           d->out_spatial[1] == d->in_spatial[1] && d->activation == act && d->conj == 0 && d->fq % 8 == 0 && pool == 3 &&        // (fq: 16-byte runs of filters per component; blocks of 32, the last one partly used)
           // the kernel's windows are rows [3o, 3o + 2]: TensorFlow's 'same' pooling (window = stride = 3) pads one row
           // on the LOW side when H % 3 == 1 (total pad 2 -> 1 + 1), so those heights are not this kernel's
           d->in_spatial[0] % 3 != 1 &&
           (long long)d->batch * ((d->in_spatial[0] + 2) / 3) * d->in_spatial[1] * 4 * d->fq < INT_MAX;
}

size_t qk_conv_relu_pool_aux_bytes(const qk_conv_desc_t *desc, int32_t pool)
{
    if (validate(desc, false) || !(conv1_pool_ok(desc, pool) || conv1_pool_ok(desc, pool, QK_ACT_LINEAR))) return 0;
    return conv1_pool_argbits_bytes(desc->batch, desc->in_spatial[0], desc->in_spatial[1], desc->fq);
}

// PReLU form of the fused first layer: slopes per row of the conv output (alpha_axis 0, alpha_len == in_spatial[0] <= 64)
// or one slope (alpha_axis -1); no dropout (the reference has none between the first convolution and its pooling)
static int prelu_pool_post_ok(const qk_conv_desc_t *desc, const qk_postop_t *post)
{
    if (!post || !post->alpha) { set_error("qk_conv_prelu_pool: post / alpha is NULL"); return QK_ERR_INVALID_ARG; }
    if (post->drop_rate != 0.f) { set_error("qk_conv_prelu_pool: dropout is not part of this kernel"); return QK_ERR_UNSUPPORTED; }
    if (!((post->alpha_axis == -1 && post->alpha_len == 1) || (post->alpha_axis == 0 && post->alpha_len == desc->in_spatial[0] && post->alpha_len <= 64))) {
        set_error("qk_conv_prelu_pool: slopes must be one, or one per position of spatial axis 0 (at most 64)"); return QK_ERR_UNSUPPORTED;
    }
    return QK_OK;
}

// The relu and the PReLU form of the fused first layer share one body per direction.  fn: the entry point
// (qk_conv_{relu,prelu}_pool_{fwd,bwd}; its name without the direction heads the messages about the layer itself);
// prelu: the convolution is LINEAR and `post` holds the slopes.  conv1_pool_checks: what both directions check first.
static int conv1_pool_checks(const char *fn, const qk_conv_desc_t *desc, int32_t pool, bool prelu, const qk_postop_t *post, int32_t flags)
{
    if (int rc = validate(desc, false)) return rc;
    if (flags & ~QK_BWD_ACCUMULATE) { set_error("%s: only QK_BWD_ACCUMULATE is a valid flag (0x%x)", fn, flags); return QK_ERR_INVALID_ARG; }
    if (!conv1_pool_ok(desc, pool, prelu ? QK_ACT_LINEAR : QK_ACT_RELU)) {
        set_error("%.*s: geometry outside the fused first-layer kernel (see include/qk.h)", (int)strlen(fn) - 4, fn); return QK_ERR_UNSUPPORTED;
    }
    return prelu ? prelu_pool_post_ok(desc, post) : QK_OK;
}

static int conv1_pool_fwd(const char *fn, const qk_conv_desc_t *desc, int32_t pool, bool prelu, const qk_postop_t *post, const void *x,
                          const float *w, const float *bias, void *pooled, void *pre_pooled, void *aux, void *stream)
{
    if (int rc = conv1_pool_checks(fn, desc, pool, prelu, post, 0)) return rc;
    if (!x || !w || !pooled || (desc->has_bias && !bias)) { set_error("%s: NULL argument", fn); return QK_ERR_INVALID_ARG; }
    if (!aligned(x, 8) || !aligned(pooled, 16) || (aux && !aligned(aux, 16)) || (pre_pooled && !aligned(pre_pooled, 16))) { set_error("%s: alignment", fn); return QK_ERR_INVALID_ARG; }
    note_path(QK_PATH_MFMA16);
    ProfScope prof_scope(QK_OP_FWD, desc, (hipStream_t)stream);
    return check_launch(launch_conv1_pool(desc->dtype, false, x, w, bias, pooled, aux, nullptr, nullptr, desc->batch, desc->in_spatial[0],
                                          desc->in_spatial[1], desc->fq, desc->has_bias, (hipStream_t)stream, prelu ? post->alpha : nullptr,
                                          prelu ? post->alpha_len : 0, pre_pooled, nullptr, desc->layout == QK_CH_FIRST), fn);
}

static int conv1_pool_bwd(const char *fn, const qk_conv_desc_t *desc, int32_t pool, bool prelu, const qk_postop_t *post, const void *x,
                          const void *dpooled, const void *pre_pooled, const void *aux, float *dw, float *dbias, float *dalpha, int32_t flags,
                          void *stream)
{
    if (int rc = conv1_pool_checks(fn, desc, pool, prelu, post, flags)) return rc;
    if (!x || !dpooled || (prelu && !pre_pooled) || !aux || !dw || (desc->has_bias && !dbias)) { set_error("%s: NULL argument", fn); return QK_ERR_INVALID_ARG; }
    if (!aligned(x, 8) || !aligned(dpooled, 16) || !aligned(pre_pooled, 16) || !aligned(aux, 16)) { set_error("%s: alignment", fn); return QK_ERR_INVALID_ARG; }
    hipStream_t st = (hipStream_t)stream;
    note_path(QK_PATH_MFMA16);
    ProfScope prof_scope(QK_OP_BWD_WEIGHT, desc, st);
    if (!(flags & QK_BWD_ACCUMULATE) &&
        (hipMemsetAsync(dw, 0, w_floats(desc) * sizeof(float), st) != hipSuccess ||
         (desc->has_bias && hipMemsetAsync(dbias, 0, 4 * (size_t)desc->fq * sizeof(float), st) != hipSuccess))) {
        set_error("memset dw failed"); return QK_ERR_LAUNCH;
    }
    return check_launch(launch_conv1_pool(desc->dtype, true, x, nullptr, nullptr, dpooled, const_cast<void *>(aux), dw, desc->has_bias ? dbias : nullptr,
                                          desc->batch, desc->in_spatial[0], desc->in_spatial[1], desc->fq, desc->has_bias, st,
                                          prelu ? post->alpha : nullptr, prelu ? post->alpha_len : 0, pre_pooled, dalpha,
                                          desc->layout == QK_CH_FIRST), fn);
}

int qk_conv_relu_pool_fwd(const qk_conv_desc_t *desc, int32_t pool, const void *x, const float *w, const float *bias,
                          void *pooled, void *aux, void *stream)
{
    return conv1_pool_fwd("qk_conv_relu_pool_fwd", desc, pool, false, nullptr, x, w, bias, pooled, nullptr, aux, stream);
}

int qk_conv_relu_pool_bwd(const qk_conv_desc_t *desc, int32_t pool, const void *x, const void *dpooled, const void *aux,
                          float *dw, float *dbias, int32_t flags, void *stream)
{
    return conv1_pool_bwd("qk_conv_relu_pool_bwd", desc, pool, false, nullptr, x, dpooled, nullptr, aux, dw, dbias, nullptr, flags, stream);
}

int qk_conv_prelu_pool_fwd(const qk_conv_desc_t *desc, int32_t pool, const qk_postop_t *post, const void *x, const float *w,
                           const float *bias, void *pooled, void *pre_pooled, void *aux, void *stream)
{
    return conv1_pool_fwd("qk_conv_prelu_pool_fwd", desc, pool, true, post, x, w, bias, pooled, pre_pooled, aux, stream);
}

int qk_conv_prelu_pool_bwd(const qk_conv_desc_t *desc, int32_t pool, const qk_postop_t *post, const void *x, const void *dpooled,
                           const void *pre_pooled, const void *aux, float *dw, float *dbias, float *dalpha, int32_t flags, void *stream)
{
    return conv1_pool_bwd("qk_conv_prelu_pool_bwd", desc, pool, true, post, x, dpooled, pre_pooled, aux, dw, dbias, dalpha, flags, stream);
}

int qk_conv_fold_taps(const qk_conv_desc_t *desc, const void *x, void *xcol, int32_t cq2, void *stream)
{
    if (int rc = validate(desc, false)) return rc;
    if (!x || !xcol) { set_error("x/xcol must not be NULL"); return QK_ERR_INVALID_ARG; }
    if (cq2 % 8 != 0 || cq2 < taps_of(desc) * desc->cq) {
        set_error("cq2 = %d must be a multiple of 8 and >= taps*cq = %d", cq2, taps_of(desc) * desc->cq);
        return QK_ERR_INVALID_ARG;
    }
    const GemmGeom g = make_geom(desc, false);            // (the gather side of the forward geometry is all k_fold_taps reads)
    if ((long long)g.M * 4 * cq2 > INT_MAX) { set_error("folded tensor has >= 2^31 elements"); return QK_ERR_UNSUPPORTED; }
    return check_launch(launch_fold_taps(desc->dtype, x, xcol, g, cq2, (hipStream_t)stream), "qk_conv_fold_taps");
}

static int pool_geom(const qk_pool_desc_t *d, PoolGeom *g, const void *a, const void *b, const void *c)
{
    if (!d) { set_error("descriptor is NULL"); return QK_ERR_INVALID_ARG; }
    if (!a || !b || !c) { set_error("maxpool: NULL buffer"); return QK_ERR_INVALID_ARG; }
    if (d->batch <= 0 || d->in_h <= 0 || d->in_w <= 0 || d->channels <= 0 || d->win_h <= 0 || d->win_w <= 0 ||
        d->out_h <= 0 || d->out_w <= 0) {
        set_error("maxpool: extents must be positive"); return QK_ERR_INVALID_ARG;
    }
    if (d->dtype != QK_F32 && d->dtype != QK_BF16 && d->dtype != QK_F16) { set_error("maxpool: bad dtype"); return QK_ERR_INVALID_ARG; }
    // windows tile the input from position 0; only the last one may be partial
    if ((long long)(d->out_h - 1) * d->win_h >= d->in_h || (long long)(d->out_w - 1) * d->win_w >= d->in_w) {
        set_error("maxpool: out extents %dx%d do not fit %dx%d with window %dx%d", d->out_h, d->out_w, d->in_h, d->in_w, d->win_h, d->win_w);
        return QK_ERR_INVALID_ARG;
    }
    const int v = d->dtype == QK_F32 ? 4 : 8;
    if (d->channels % v != 0) { set_error("maxpool: channels must be a multiple of %d", v); return QK_ERR_UNSUPPORTED; }
    if (!aligned(a, 16) || !aligned(b, 16) || !aligned(c, 16)) { set_error("maxpool: buffers must be 16-byte aligned"); return QK_ERR_INVALID_ARG; }
    if ((long long)d->batch * d->in_h * d->in_w * d->channels > INT_MAX) { set_error("maxpool: tensor has >= 2^31 elements"); return QK_ERR_UNSUPPORTED; }
    g->batch = d->batch; g->ih = d->in_h; g->iw = d->in_w; g->C = d->channels;
    g->wh = d->win_h; g->ww = d->win_w; g->oh = d->out_h; g->ow = d->out_w;
    return 0;
}

int qk_maxpool2d_fwd(const qk_pool_desc_t *desc, const void *x, void *y, void *stream)
{
    PoolGeom g;
    if (int rc = pool_geom(desc, &g, x, y, y)) return rc;
    return check_launch(launch_maxpool(desc->dtype, false, x, nullptr, y, g, (hipStream_t)stream), "qk_maxpool2d_fwd");
}

int qk_maxpool2d_bwd(const qk_pool_desc_t *desc, const void *x, const void *dy, void *dx, void *stream)
{
    PoolGeom g;
    if (int rc = pool_geom(desc, &g, x, dy, dx)) return rc;
    // 'valid' pooling leaves trailing rows / columns outside every window: their gradient is zero
    if ((long long)g.oh * g.wh < g.ih || (long long)g.ow * g.ww < g.iw) {
        const size_t es = desc->dtype == QK_F32 ? 4 : 2;
        if (hipMemsetAsync(dx, 0, (size_t)g.batch * g.ih * g.iw * g.C * es, (hipStream_t)stream) != hipSuccess) {
            set_error("maxpool: memset failed"); return QK_ERR_LAUNCH;
        }
    }
    return check_launch(launch_maxpool(desc->dtype, true, x, dy, dx, g, (hipStream_t)stream), "qk_maxpool2d_bwd");
}

size_t qk_ctc_workspace_bytes(int32_t batch, int32_t frames, int32_t max_label_len)
{
    return (batch <= 0 || frames <= 0 || max_label_len < 0) ? 0 : ctc_workspace_bytes(batch, frames, max_label_len);
}

int qk_ctc_batch_cost(int32_t dtype, int32_t batch, int32_t frames, int32_t classes, const void *y_pred, const int32_t *labels,
                      int32_t max_label_len, const int32_t *input_length, const int32_t *label_length, float *cost, void *dy_pred,
                      void *workspace, size_t workspace_bytes, void *stream)
{
    if (int rc = lattice_extents_ok("ctc", batch, frames, classes, max_label_len)) return rc;
    if (!y_pred || !input_length || !label_length || !cost || (max_label_len > 0 && !labels)) return null_arg("ctc");
    if (int rc = ctc_workspace_ok("ctc", workspace, workspace_bytes, ctc_workspace_bytes(batch, frames, max_label_len), 4)) return rc;
    if (int rc = count_ok("ctc", (long long)batch * frames * classes)) return rc;
    const int rc = launch_ctc(dtype, batch, frames, classes, y_pred, labels, max_label_len, input_length, label_length, cost, dy_pred,
                              static_cast<float *>(workspace), (hipStream_t)stream);
    if (rc == QK_ERR_UNSUPPORTED) set_error("ctc: more than 127 labels, more than 256 classes or too many frames for one workgroup's LDS");
    return check_launch(rc, "qk_ctc_batch_cost");
}

int qk_ctc_greedy_decode(int32_t dtype, int32_t batch, int32_t frames, int32_t classes, const void *y_pred, const int32_t *input_length,
                         int32_t *decoded, int32_t *decoded_len, float *log_prob, void *stream)
{
    if (batch <= 0 || frames <= 0 || classes < 2 || dtype < QK_F32 || dtype > QK_F16)
        return fail(QK_ERR_INVALID_ARG, "ctc_greedy_decode: bad arguments (%d, %d, %d, dtype %d)", batch, frames, classes, dtype);
    if (!y_pred || !input_length || !decoded || !decoded_len || !log_prob) return null_arg("ctc_greedy_decode");
    if (classes > 256) return fail(QK_ERR_UNSUPPORTED, "ctc_greedy_decode: more than 256 classes");
    if (int rc = count_ok("ctc_greedy_decode", (long long)batch * frames * classes)) return rc;
    return check_launch(launch_ctc_greedy(dtype, batch, frames, classes, y_pred, input_length, decoded, decoded_len, log_prob,
                                          (hipStream_t)stream), "qk_ctc_greedy_decode");
}

size_t qk_ctc_beam_workspace_bytes(int32_t batch, int32_t frames, int32_t beam_width)
{
    return (batch <= 0 || frames <= 0 || beam_width <= 0) ? 0 : ctc_beam_workspace_bytes(batch, frames, beam_width);
}

int qk_ctc_beam_search_decode(int32_t dtype, int32_t batch, int32_t frames, int32_t classes, const void *y_pred, const int32_t *input_length,
                              int32_t beam_width, int32_t top_paths, int32_t merge_repeated, int32_t *decoded, int32_t *decoded_len,
                              float *log_prob, void *workspace, size_t workspace_bytes, void *stream)
{
    if (int rc = beam_args_ok("ctc_beam_search_decode", dtype, batch, frames, classes, y_pred, input_length, beam_width, top_paths, decoded,
                              decoded_len, log_prob, workspace, workspace_bytes, nullptr))
        return rc;
    return check_launch(launch_ctc_beam(dtype, batch, frames, classes, y_pred, input_length, beam_width, top_paths, merge_repeated,
                                        decoded, decoded_len, log_prob, static_cast<int *>(workspace), (hipStream_t)stream),
                        "qk_ctc_beam_search_decode");
}

int qk_ctc_beam_search_decode_lm(int32_t dtype, int32_t batch, int32_t frames, int32_t classes, const void *y_pred,
                                 const int32_t *input_length, int32_t beam_width, int32_t top_paths, int32_t merge_repeated,
                                 int32_t lm_order, const float *lm_table, float lm_weight, float insertion_bonus, int32_t lm_eos,
                                 int32_t *decoded, int32_t *decoded_len, float *log_prob, float *score,
                                 void *workspace, size_t workspace_bytes, void *stream)
{
    const BeamLmArgs lm = {lm_order, lm_table, lm_weight, insertion_bonus, score};
    if (int rc = beam_args_ok("ctc_beam_search_decode_lm", dtype, batch, frames, classes, y_pred, input_length, beam_width, top_paths,
                              decoded, decoded_len, log_prob, workspace, workspace_bytes, &lm))
        return rc;
    return check_launch(launch_ctc_beam_lm(dtype, batch, frames, classes, y_pred, input_length, beam_width, top_paths, merge_repeated, lm_order,
                                           lm_table, lm_weight, insertion_bonus, lm_eos, decoded, decoded_len, log_prob, score,
                                           static_cast<int *>(workspace), (hipStream_t)stream),
                        "qk_ctc_beam_search_decode_lm");
}

int qk_edit_distance(int32_t batch, const int32_t *hyp, int32_t hyp_stride, const int32_t *hyp_len, const int32_t *ref, int32_t ref_stride,
                     const int32_t *ref_len, const int32_t *class_map, int32_t classes, int32_t *distance, int32_t *ref_len_out, void *stream)
{
    if (batch <= 0 || hyp_stride < 0 || ref_stride < 0 || (class_map && classes <= 0))
        return fail(QK_ERR_INVALID_ARG, "edit_distance: bad arguments (%d, %d, %d, %d)", batch, hyp_stride, ref_stride, classes);
    if (!hyp_len || !ref_len || !distance || (hyp_stride > 0 && !hyp) || (ref_stride > 0 && !ref)) return null_arg("edit_distance");
    if (ref_stride > 1024) return fail(QK_ERR_UNSUPPORTED, "edit_distance: reference longer than 1024 tokens (stride %d)", ref_stride);
    return check_launch(launch_edit_distance(batch, hyp, hyp_stride, hyp_len, ref, ref_stride, ref_len, class_map, class_map ? classes : 0,
                                             distance, ref_len_out, (hipStream_t)stream), "qk_edit_distance");
}

size_t qk_edit_align_workspace_bytes(int32_t batch, int32_t hyp_stride, int32_t ref_stride)
{
    if (batch <= 0 || hyp_stride < 0 || ref_stride < 0 || hyp_stride > 1024 || ref_stride > 1024) return 0;
    return edit_align_workspace_bytes(batch, hyp_stride, ref_stride);
}

int qk_edit_align(int32_t batch, const int32_t *hyp, int32_t hyp_stride, const int32_t *hyp_len, const int32_t *ref, int32_t ref_stride,
                  const int32_t *ref_len, const int32_t *class_map, int32_t classes, int32_t *counts, int32_t *ali_ref, int32_t *ali_hyp,
                  int32_t *ali_len, int32_t *confusion, int32_t out_classes, void *workspace, size_t workspace_bytes, void *stream)
{
    if (batch < 0 || hyp_stride < 0 || ref_stride < 0 || (class_map && classes <= 0) || (confusion && out_classes < 0))
        return fail(QK_ERR_INVALID_ARG, "edit_align: bad arguments (%d, %d, %d, %d, %d)", batch, hyp_stride, ref_stride, classes, out_classes);
    if (hyp_stride > 1024 || ref_stride > 1024 || (confusion && out_classes > 256))
        return fail(QK_ERR_UNSUPPORTED, "edit_align: unsupported (hyp_stride %d <= 1024, ref_stride %d <= 1024, out_classes %d <= 256)", hyp_stride,
                    ref_stride, confusion ? out_classes : 0);
    if (batch == 0) return 0;
    if (!hyp_len || !ref_len || !counts || (hyp_stride > 0 && !hyp) || (ref_stride > 0 && !ref)) return null_arg("edit_align");
    if ((ali_ref != nullptr) != (ali_hyp != nullptr) || (ali_ref != nullptr) != (ali_len != nullptr))
        return fail(QK_ERR_INVALID_ARG, "edit_align: ali_ref, ali_hyp and ali_len are NULL together or not at all");
    const size_t need = edit_align_workspace_bytes(batch, hyp_stride, ref_stride);
    if (int rc = need > 0 ? ctc_workspace_ok("edit_align", workspace, workspace_bytes, need, 8) : QK_OK) return rc;
    return check_launch(launch_edit_align(batch, hyp, hyp_stride, hyp_len, ref, ref_stride, ref_len, class_map, class_map ? classes : 0,
                                          counts, ali_ref, ali_hyp, ali_len, confusion, confusion ? out_classes : 0, workspace,
                                          (hipStream_t)stream), "qk_edit_align");
}

size_t qk_ctc_align_workspace_bytes(int32_t batch, int32_t frames, int32_t max_label_len)
{
    return (batch <= 0 || frames <= 0 || max_label_len < 0) ? 0 : ctc_align_workspace_bytes(batch, frames);
}

int qk_ctc_forced_align(int32_t dtype, int32_t batch, int32_t frames, int32_t classes, const void *y_pred, const int32_t *labels,
                        int32_t max_label_len, const int32_t *input_length, const int32_t *label_length, int32_t *path,
                        int32_t *starts, int32_t *ends, float *score, void *workspace, size_t workspace_bytes, void *stream)
{
    const char *what = "ctc_forced_align";
    if (int rc = lattice_extents_ok(what, batch, frames, classes, max_label_len)) return rc;
    if (classes > 256 || max_label_len > 127 || dtype < QK_F32 || dtype > QK_F16)
        return fail(QK_ERR_UNSUPPORTED, "%s: unsupported (classes %d <= 256, max_label_len %d <= 127, dtype %d one of fp32 / bf16 / fp16)", what,
                    classes, max_label_len, dtype);
    if (!y_pred || !input_length || !label_length || !path || !score || (max_label_len > 0 && (!labels || !starts || !ends)))
        return null_arg(what);
    if (int rc = count_ok(what, (long long)batch * frames * classes)) return rc;
    if (!ctc_align_supported(frames, classes, max_label_len))
        return fail(QK_ERR_UNSUPPORTED, "%s: %d frames are too many for one workgroup's LDS", what, frames);
    if (int rc = ctc_workspace_ok(what, workspace, workspace_bytes, ctc_align_workspace_bytes(batch, frames), 8)) return rc;
    return check_launch(launch_ctc_align(dtype, batch, frames, classes, y_pred, labels, max_label_len, input_length, label_length, path,
                                         starts, ends, score, workspace, (hipStream_t)stream), "qk_ctc_forced_align");
}

int32_t qk_fbank_num_frames(int64_t samples, int32_t frame_len, int32_t frame_step)
{
    if (frame_len < 1 || frame_step < 1) return 0;
    if (samples <= frame_len) return 1;
    const long long n = 1 + (samples - frame_len + frame_step - 1) / frame_step;
    return n > INT_MAX ? 0 : (int32_t)n;
}

size_t qk_fbank_workspace_bytes(int32_t batch, int32_t frames, int32_t rows, int32_t normalize)
{
    if (batch <= 0 || frames <= 0 || rows <= 0) return 0;
    return fbank_workspace_bytes(batch, frames, rows, normalize == QK_FBANK_NORM_UTTERANCE);
}

int qk_fbank_quaternion(int32_t wave_dtype, int32_t batch, int64_t max_samples, const void *wave, const int32_t *lengths, int32_t frames,
                        int32_t frame_len, int32_t frame_step, int32_t nfft, float preemph, int32_t window, int32_t nfilt,
                        const int32_t *mel_bins, int32_t append_energy, int32_t delta_n, int32_t normalize, int32_t out_dtype, void *out,
                        int32_t *frame_lengths, void *workspace, size_t workspace_bytes, void *stream)
{
    if (batch <= 0 || max_samples <= 0 || max_samples > INT_MAX || frames <= 0 || frame_len <= 0 || frame_step <= 0 || nfilt <= 0 ||
        (wave_dtype != QK_WAVE_F32 && wave_dtype != QK_WAVE_I16) || (window != QK_WINDOW_RECT && window != QK_WINDOW_HAMMING) ||
        (normalize != QK_FBANK_NORM_NONE && normalize != QK_FBANK_NORM_UTTERANCE) || out_dtype < QK_F32 || out_dtype > QK_F16 ||
        !isfinite(preemph)) {
        set_error("fbank_quaternion: bad arguments (batch %d, samples %lld, frames %d, frame %d / %d, nfilt %d, dtypes %d / %d, window %d, "
                  "normalize %d)", batch, (long long)max_samples, frames, frame_len, frame_step, nfilt, wave_dtype, out_dtype, window, normalize);
        return QK_ERR_INVALID_ARG;
    }
    if (!wave || !lengths || !mel_bins || !out || !frame_lengths) { set_error("fbank_quaternion: NULL argument"); return QK_ERR_INVALID_ARG; }
    if (nfft < 256 || nfft > 1024 || (nfft & (nfft - 1)) || frame_len > nfft || nfilt > QK_FBANK_MAX_FILT || delta_n < 1 || delta_n > 4) {
        set_error("fbank_quaternion: unsupported (nfft %d a power of two in [256, 1024] and >= frame_len %d, nfilt %d <= %d, delta_n %d in [1, 4])",
                  nfft, frame_len, nfilt, QK_FBANK_MAX_FILT, delta_n);
        return QK_ERR_UNSUPPORTED;
    }
    const int need_frames = qk_fbank_num_frames(max_samples, frame_len, frame_step);
    if (frames < need_frames) { set_error("fbank_quaternion: %d frames < the %d of max_samples %lld", frames, need_frames, (long long)max_samples); return QK_ERR_INVALID_ARG; }
    FbankGeom g;
    g.B = batch; g.n_max = (int)max_samples; g.T = frames;
    g.L = frame_len; g.S = frame_step; g.nfft = nfft;
    g.nfilt = nfilt; g.F = nfilt + (append_energy ? 1 : 0);
    g.window = window; g.preemph = preemph;
    for (int j = 0; j < nfilt + 2; ++j) {
        g.bins[j] = mel_bins[j];
        if (mel_bins[j] < 0 || mel_bins[j] > nfft / 2 || (j > 0 && mel_bins[j] < mel_bins[j - 1])) {
            set_error("fbank_quaternion: mel_bins[%d] = %d (must be non-decreasing in [0, nfft / 2])", j, mel_bins[j]);
            return QK_ERR_INVALID_ARG;
        }
    }
    if ((long long)batch * 4 * g.F * frames > INT_MAX || (long long)batch * max_samples > ((long long)1 << 40)) {
        set_error("fbank_quaternion: tensor with >= 2^31 elements"); return QK_ERR_UNSUPPORTED;
    }
    g.tile = fbank_tile(frame_len, frame_step);
    g.span = (g.tile - 1) * frame_step + frame_len;
    const bool norm = normalize == QK_FBANK_NORM_UTTERANCE;
    const size_t need = fbank_workspace_bytes(batch, frames, g.F, norm);
    if (!workspace || workspace_bytes < need || !aligned(workspace, 16)) { set_error("fbank_quaternion needs %zu workspace bytes, got %zu", need, workspace_bytes); return QK_ERR_WORKSPACE; }
    return check_launch(launch_fbank(wave_dtype, wave, lengths, g, delta_n, norm, out_dtype, out, frame_lengths, workspace,
                                     (hipStream_t)stream), "qk_fbank_quaternion");
}

int qk_spec_augment(int32_t in_dtype, int32_t out_dtype, int32_t batch, int32_t planes, int32_t rows, int32_t frames,
                    const void *x, const int32_t *lengths, const qk_specaug_t *policy, const uint32_t *counter_dev,
                    void *out, int32_t *plan, void *stream)
{
    if (batch < 1 || planes < 1 || rows < 1 || frames < 1 || in_dtype < QK_F32 || in_dtype > QK_F16 || out_dtype < QK_F32 || out_dtype > QK_F16) {
        set_error("spec_augment: bad arguments (batch %d, planes %d, rows %d, frames %d, dtypes %d / %d)", batch, planes, rows, frames, in_dtype, out_dtype);
        return QK_ERR_INVALID_ARG;
    }
    if (!x || !lengths || !policy || !out) { set_error("spec_augment: NULL argument"); return QK_ERR_INVALID_ARG; }
    const qk_specaug_t &p = *policy;
    if (p.freq_masks < 0 || p.freq_masks > QK_SPECAUG_MAX_MASKS || p.time_masks < 0 || p.time_masks > QK_SPECAUG_MAX_MASKS) {
        set_error("spec_augment: freq_masks %d / time_masks %d outside 0 .. %d", p.freq_masks, p.time_masks, QK_SPECAUG_MAX_MASKS);
        return QK_ERR_INVALID_ARG;
    }
    if (p.time_warp < 0 || p.freq_width < 0 || p.time_width < 0) {
        set_error("spec_augment: time_warp %d, freq_width %d and time_width %d must be >= 0", p.time_warp, p.freq_width, p.time_width);
        return QK_ERR_INVALID_ARG;
    }
    if (!isfinite(p.time_ratio) || p.time_ratio < 0.f || p.time_ratio > 1.f || !isfinite(p.fill)) {
        set_error("spec_augment: time_ratio %g must lie in [0, 1] and fill %g be finite", (double)p.time_ratio, (double)p.fill);
        return QK_ERR_INVALID_ARG;
    }
    const long long count = (long long)batch * planes * rows * frames;
    if (count > INT_MAX) { set_error("spec_augment: tensor with >= 2^31 elements"); return QK_ERR_UNSUPPORTED; }
    const size_t in_bytes = (size_t)count * elem_size(in_dtype), out_bytes = (size_t)count * elem_size(out_dtype);
    if (!aligned(x, elem_size(in_dtype)) || !aligned(out, elem_size(out_dtype)) || (plan && !aligned(plan, 4))) {
        set_error("spec_augment: x, out and plan must be aligned to their element size"); return QK_ERR_INVALID_ARG;
    }
    const uintptr_t xa = reinterpret_cast<uintptr_t>(x), oa = reinterpret_cast<uintptr_t>(out);
    if (xa < oa + out_bytes && oa < xa + in_bytes) { set_error("spec_augment: out overlaps x (the warp reads neighbouring frames)"); return QK_ERR_INVALID_ARG; }
    return check_launch(launch_spec_augment(in_dtype, out_dtype, batch, planes, rows, frames, x, lengths, p, counter_dev, out, plan,
                                            (hipStream_t)stream), "qk_spec_augment");
}

// 0 when the policy is one qk.h admits, else the error code (message set)
static int speed_policy_check(const qk_speed_perturb_t *policy)
{
    if (!policy) { set_error("speed_perturb: policy is NULL"); return QK_ERR_INVALID_ARG; }
    const qk_speed_perturb_t &p = *policy;
    if (p.n_speeds < 1 || p.n_speeds > QK_SPEED_MAX_SPEEDS) {
        set_error("speed_perturb: n_speeds %d outside 1 .. %d", p.n_speeds, QK_SPEED_MAX_SPEEDS); return QK_ERR_INVALID_ARG;
    }
    if (!isfinite(p.gain_lo) || !isfinite(p.gain_hi) || p.gain_lo < 0.f || p.gain_lo > p.gain_hi) {
        set_error("speed_perturb: gains %g, %g must be finite with 0 <= gain_lo <= gain_hi", (double)p.gain_lo, (double)p.gain_hi);
        return QK_ERR_INVALID_ARG;
    }
    for (int i = 0; i < p.n_speeds; ++i) {
        const int num = p.num[i], den = p.den[i], kw = p.half_width[i];
        if (num < 1 || num > QK_SPEED_MAX_DEN || den < 1 || den > QK_SPEED_MAX_DEN || 2 * num < den || num > 2 * den) {
            set_error("speed_perturb: speed %d = %d / %d (both in 1 .. %d, ratio in [1/2, 2])", i, num, den, QK_SPEED_MAX_DEN);
            return QK_ERR_INVALID_ARG;
        }
        if (kw < 0 || (num == den) != (kw == 0)) {
            set_error("speed_perturb: speed %d = %d / %d with half_width %d (0 exactly when num == den)", i, num, den, kw);
            return QK_ERR_INVALID_ARG;
        }
        if (num != den && p.table_offset[i] < 0) { set_error("speed_perturb: table_offset[%d] = %d", i, p.table_offset[i]); return QK_ERR_INVALID_ARG; }
    }
    for (int i = 0; i < p.n_speeds; ++i)
        if (2 * (long long)p.half_width[i] + 2 > QK_SPEED_MAX_TAPS) {
            set_error("speed_perturb: speed %d has %lld taps, more than %d", i, 2 * (long long)p.half_width[i] + 2, QK_SPEED_MAX_TAPS);
            return QK_ERR_UNSUPPORTED;
        }
    return 0;
}

int64_t qk_speed_perturb_out_samples(int64_t max_samples, const qk_speed_perturb_t *policy)
{
    if (max_samples < 1) { set_error("speed_perturb_out_samples: max_samples %lld < 1", (long long)max_samples); return -1; }
    const int rc = speed_policy_check(policy);
    if (rc != 0 && rc != QK_ERR_UNSUPPORTED) return -1;                    // (the tap limit does not bear on the lengths)
    if (max_samples > INT64_MAX / QK_SPEED_MAX_DEN) { set_error("speed_perturb_out_samples: max_samples too large"); return -1; }
    int64_t most = 0;
    for (int i = 0; i < policy->n_speeds; ++i) {
        const int64_t len = (max_samples * policy->den[i] + policy->num[i] - 1) / policy->num[i];
        if (len > most) most = len;
    }
    return most;
}

int qk_speed_perturb(int32_t wave_dtype, int32_t batch, int64_t max_samples, const void *wave, const int32_t *lengths,
                     const qk_speed_perturb_t *policy, const float *tables, const uint32_t *counter_dev, int64_t out_samples, float *out,
                     int32_t *out_lengths, int32_t *plan, void *stream)
{
    if (batch < 1 || max_samples < 1 || (wave_dtype != QK_WAVE_F32 && wave_dtype != QK_WAVE_I16)) {
        set_error("speed_perturb: bad arguments (batch %d, max_samples %lld, wave_dtype %d)", batch, (long long)max_samples, wave_dtype);
        return QK_ERR_INVALID_ARG;
    }
    if (!wave || !lengths || !out || !out_lengths) { set_error("speed_perturb: NULL argument"); return QK_ERR_INVALID_ARG; }
    const int rc = speed_policy_check(policy);
    if (rc == QK_ERR_INVALID_ARG) return rc;
    bool filters = false;
    for (int i = 0; i < policy->n_speeds; ++i) filters |= policy->num[i] != policy->den[i];
    if (filters && !tables) { set_error("speed_perturb: tables is NULL, but a speed has num != den"); return QK_ERR_INVALID_ARG; }
    const int64_t limit = (int64_t)1 << 26;
    if (max_samples < limit && out_samples < qk_speed_perturb_out_samples(max_samples, policy)) {
        set_error("speed_perturb: out_samples %lld below the %lld that max_samples %lld needs", (long long)out_samples,
                  (long long)qk_speed_perturb_out_samples(max_samples, policy), (long long)max_samples);
        return QK_ERR_INVALID_ARG;
    }
    const size_t wave_elem = wave_dtype == QK_WAVE_I16 ? 2 : 4;
    if (!aligned(wave, wave_elem) || !aligned(out, 4) || !aligned(lengths, 4) || !aligned(out_lengths, 4) || (plan && !aligned(plan, 4)) ||
        (tables && !aligned(tables, 4)) || (counter_dev && !aligned(counter_dev, 4))) {
        set_error("speed_perturb: pointers must be aligned to their element size"); return QK_ERR_INVALID_ARG;
    }
    if (rc != 0) return rc;                                                // the tap limit
    if (max_samples >= limit || out_samples >= limit) {
        set_error("speed_perturb: max_samples %lld / out_samples %lld must be below 2^26", (long long)max_samples, (long long)out_samples);
        return QK_ERR_UNSUPPORTED;
    }
    const uintptr_t wa = reinterpret_cast<uintptr_t>(wave), oa = reinterpret_cast<uintptr_t>(out);
    const size_t wave_bytes = (size_t)batch * (size_t)max_samples * wave_elem, out_bytes = (size_t)batch * (size_t)out_samples * 4;
    if (wa < oa + out_bytes && oa < wa + wave_bytes) { set_error("speed_perturb: out overlaps wave"); return QK_ERR_INVALID_ARG; }
    return check_launch(launch_speed_perturb(wave_dtype, batch, (int)max_samples, wave, lengths, *policy, tables, counter_dev, (int)out_samples,
                                             out, out_lengths, plan, (hipStream_t)stream), "qk_speed_perturb");
}

int64_t qk_noise_reverb_workspace_bytes(int32_t batch, int64_t max_samples)
{
    if (batch < 1 || max_samples < 1 || max_samples >= ((int64_t)1 << 26)) {
        set_error("noise_reverb_workspace_bytes: batch %d, max_samples %lld (1 .. 2^26 - 1)", batch, (long long)max_samples); return -1;
    }
    return (int64_t)noise_reverb_workspace_bytes(batch, (int)max_samples);
}

int qk_noise_reverb(int32_t wave_dtype, int32_t batch, int64_t max_samples, const void *wave, const int32_t *lengths,
                    const qk_noise_reverb_t *policy, const float *rirs, const int32_t *rir_len, const int32_t *rir_delay,
                    const float *noises, const int32_t *noise_len, const uint32_t *counter_dev, float *out, int32_t *plan,
                    void *workspace, int64_t workspace_bytes, void *stream)
{
    if (batch < 1 || max_samples < 1 || (wave_dtype != QK_WAVE_F32 && wave_dtype != QK_WAVE_I16)) {
        set_error("noise_reverb: bad arguments (batch %d, max_samples %lld, wave_dtype %d)", batch, (long long)max_samples, wave_dtype);
        return QK_ERR_INVALID_ARG;
    }
    if (!wave || !lengths || !policy || !out || !workspace) { set_error("noise_reverb: NULL argument"); return QK_ERR_INVALID_ARG; }
    const qk_noise_reverb_t &p = *policy;
    if (p.n_rirs < 0 || p.n_noises < 0) { set_error("noise_reverb: n_rirs %d / n_noises %d negative", p.n_rirs, p.n_noises); return QK_ERR_INVALID_ARG; }
    if (p.n_rirs > 0 && (!rirs || !rir_len || !rir_delay)) { set_error("noise_reverb: rirs / rir_len / rir_delay is NULL with n_rirs %d", p.n_rirs); return QK_ERR_INVALID_ARG; }
    if (p.n_noises > 0 && (!noises || !noise_len)) { set_error("noise_reverb: noises / noise_len is NULL with n_noises %d", p.n_noises); return QK_ERR_INVALID_ARG; }
    if (p.rir_stride < 1 || p.noise_stride < 1) { set_error("noise_reverb: rir_stride %d / noise_stride %d < 1", p.rir_stride, p.noise_stride); return QK_ERR_INVALID_ARG; }
    const int one = 1 << 24;
    if (p.rir_prob_q24 < 0 || p.rir_prob_q24 > one || p.noise_prob_q24 < 0 || p.noise_prob_q24 > one) {
        set_error("noise_reverb: probabilities %d, %d outside 0 .. 2^24", p.rir_prob_q24, p.noise_prob_q24); return QK_ERR_INVALID_ARG;
    }
    if (!isfinite(p.snr_lo) || !isfinite(p.snr_hi) || p.snr_lo > p.snr_hi) {
        set_error("noise_reverb: snr bounds %g, %g must be finite with snr_lo <= snr_hi", (double)p.snr_lo, (double)p.snr_hi); return QK_ERR_INVALID_ARG;
    }
    const size_t wave_elem = wave_dtype == QK_WAVE_I16 ? 2 : 4;
    if (!aligned(wave, wave_elem) || !aligned(out, 4) || !aligned(lengths, 4) || (plan && !aligned(plan, 4)) || !aligned(workspace, 8) ||
        (rirs && !aligned(rirs, 4)) || (rir_len && !aligned(rir_len, 4)) || (rir_delay && !aligned(rir_delay, 4)) ||
        (noises && !aligned(noises, 4)) || (noise_len && !aligned(noise_len, 4)) || (counter_dev && !aligned(counter_dev, 4))) {
        set_error("noise_reverb: pointers must be aligned to their element size (the workspace to 8 bytes)"); return QK_ERR_INVALID_ARG;
    }
    const int64_t limit = (int64_t)1 << 26;
    if (max_samples < limit) {
        const int64_t need = (int64_t)noise_reverb_workspace_bytes(batch, (int)max_samples);
        if (workspace_bytes < need) {
            set_error("noise_reverb: workspace of %lld bytes, %lld needed", (long long)workspace_bytes, (long long)need); return QK_ERR_INVALID_ARG;
        }
        const uintptr_t wa = reinterpret_cast<uintptr_t>(wave), oa = reinterpret_cast<uintptr_t>(out);
        const size_t wave_bytes = (size_t)batch * (size_t)max_samples * wave_elem, out_bytes = (size_t)batch * (size_t)max_samples * 4;
        if (wa < oa + out_bytes && oa < wa + wave_bytes) { set_error("noise_reverb: out overlaps wave"); return QK_ERR_INVALID_ARG; }
    }
    if (p.rir_stride > QK_REVERB_MAX_TAPS) {
        set_error("noise_reverb: rir_stride %d above %d taps", p.rir_stride, QK_REVERB_MAX_TAPS); return QK_ERR_UNSUPPORTED;
    }
    if (max_samples >= limit) { set_error("noise_reverb: max_samples %lld must be below 2^26", (long long)max_samples); return QK_ERR_UNSUPPORTED; }
    return check_launch(launch_noise_reverb(wave_dtype, batch, (int)max_samples, wave, lengths, p, rirs, rir_len, rir_delay, noises, noise_len,
                                            counter_dev, out, plan, workspace, (hipStream_t)stream), "qk_noise_reverb");
}

int qk_softmax_rows_fwd(int32_t dtype, int64_t rows, int32_t cols, const float *logits, const float *bias, void *y, void *stream)
{
    if (!logits || !y || rows < 0 || cols < 1 || cols > 64 || dtype < QK_F32 || dtype > QK_F16) { set_error("qk_softmax_rows_fwd: bad argument (1 <= cols <= 64)"); return QK_ERR_INVALID_ARG; }
    if (rows == 0) return QK_OK;
    return check_launch(launch_softmax_rows(dtype, false, logits, bias, y, nullptr, rows, cols, (hipStream_t)stream), "qk_softmax_rows_fwd");
}

int qk_softmax_rows_bwd(int32_t dtype, int64_t rows, int32_t cols, const void *y, const void *dy, void *dlogits, float *dbias, void *stream)
{
    if (!y || !dy || !dlogits || rows < 0 || cols < 1 || cols > 64 || dtype < QK_F32 || dtype > QK_F16) { set_error("qk_softmax_rows_bwd: bad argument (1 <= cols <= 64)"); return QK_ERR_INVALID_ARG; }
    if (rows == 0) return QK_OK;
    return check_launch(launch_softmax_rows(dtype, true, y, dy, dlogits, dbias, rows, cols, (hipStream_t)stream), "qk_softmax_rows_bwd");
}

int qk_dense_softmax_supported(int32_t dtype, int64_t rows, int32_t in_dim, int32_t units)
{
    return dense_softmax_supported(dtype, rows, in_dim, units) ? 1 : 0;
}

int qk_dense_softmax_fwd(int32_t dtype, int64_t rows, int32_t in_dim, int32_t units, const void *x, const float *kernel, const float *bias,
                         void *y, void *stream)
{
    if (!x || !kernel || !y || rows < 0) { set_error("qk_dense_softmax_fwd: NULL buffer or negative row count"); return QK_ERR_INVALID_ARG; }
    if (!dense_softmax_supported(dtype, rows, in_dim, units)) { set_error("qk_dense_softmax_fwd: in_dim %d / units %d / dtype %d outside the kernel (in_dim 64, 128, 256; even units <= 64; 16-bit)", in_dim, units, dtype); return QK_ERR_UNSUPPORTED; }
    if (!aligned(x, 16) || !aligned(y, 4) || !aligned(kernel, 4)) { set_error("qk_dense_softmax_fwd: x must be 16-byte aligned, y 4-byte"); return QK_ERR_INVALID_ARG; }
    if (rows == 0) return QK_OK;
    return check_launch(launch_dense_softmax_fwd(dtype, rows, in_dim, units, x, kernel, bias, y, (hipStream_t)stream), "qk_dense_softmax_fwd");
}

size_t qk_dense_softmax_bwd_workspace_bytes(int32_t dtype, int64_t rows, int32_t in_dim, int32_t units)
{
    return dense_softmax_bwd_workspace_bytes(dtype, rows, in_dim, units);
}

int qk_dense_softmax_bwd(int32_t dtype, int64_t rows, int32_t in_dim, int32_t units, const void *x, const float *kernel, const void *y,
                         const void *dy, void *dx, float *dkernel, float *dbias, const float *dy_scale_dev, float dy_scale,
                         void *workspace, size_t workspace_bytes, void *stream)
{
    if (!x || !kernel || !y || !dy || !dx || rows < 0) { set_error("qk_dense_softmax_bwd: NULL buffer or negative row count"); return QK_ERR_INVALID_ARG; }
    if (!dense_softmax_supported(dtype, rows, in_dim, units)) { set_error("qk_dense_softmax_bwd: in_dim %d / units %d / dtype %d outside the kernel (in_dim 64, 128, 256; even units <= 64; 16-bit)", in_dim, units, dtype); return QK_ERR_UNSUPPORTED; }
    if (!aligned(x, 16) || !aligned(dx, 16) || !aligned(y, 4) || !aligned(dy, 4)) { set_error("qk_dense_softmax_bwd: x / dx must be 16-byte aligned, y / dy 4-byte"); return QK_ERR_INVALID_ARG; }
    if (rows == 0) return QK_OK;
    if (dkernel || dbias) {
        const size_t need = dense_softmax_bwd_workspace_bytes(dtype, rows, in_dim, units);
        if (!workspace || workspace_bytes < need || !aligned(workspace, 16)) { set_error("qk_dense_softmax_bwd needs %zu workspace bytes (16-byte aligned), got %zu", need, workspace_bytes); return QK_ERR_WORKSPACE; }
    }
    return check_launch(launch_dense_softmax_bwd(dtype, rows, in_dim, units, x, kernel, y, dy, dx, dkernel, dbias, dy_scale_dev, dy_scale, static_cast<float *>(workspace), (hipStream_t)stream), "qk_dense_softmax_bwd");
}

int qk_weighted_sum(int32_t dtype, int64_t n, const void *a, const float *w, float *out, void *stream)
{
    if (!a || !w || !out || n < 0 || dtype < QK_F32 || dtype > QK_F16) { set_error("qk_weighted_sum: bad argument"); return QK_ERR_INVALID_ARG; }
    if (n == 0) return QK_OK;
    return check_launch(launch_weighted_sum(dtype, a, w, out, n, (hipStream_t)stream), "qk_weighted_sum");
}

int qk_conv_prep_kernels(int32_t n, const qk_conv_desc_t *const *descs, const int32_t *ops, const float *const *w,
                         void *const *workspaces, void *stream)
{
    if (n < 0 || (n > 0 && (!descs || !ops || !w || !workspaces))) { set_error("qk_conv_prep_kernels: NULL argument"); return QK_ERR_INVALID_ARG; }
    for (int dt = QK_BF16; dt <= QK_F16; ++dt) {
        PrepJobs jobs;
        int m = 0;
        for (int i = 0; i <= n; ++i) {
            if (i < n) {
                const qk_conv_desc_t *d = descs[i];
                if (!d || !w[i] || !workspaces[i]) { set_error("qk_conv_prep_kernels: job %d has a NULL member", i); return QK_ERR_INVALID_ARG; }
                if (d->dtype != dt) continue;
                if (ops[i] != QK_OP_FWD && ops[i] != QK_OP_BWD_DATA && ops[i] != QK_OP_BWD) { set_error("qk_conv_prep_kernels: job %d: bad op %d", i, ops[i]); return QK_ERR_INVALID_ARG; }
                if (!aligned(workspaces[i], 16)) { set_error("qk_conv_prep_kernels: job %d: workspace not 16-byte aligned", i); return QK_ERR_INVALID_ARG; }
                if (d->cq % 16 || d->fq % 16) continue;       // outside the matrix-core path: its calls run the fp32-MFMA kernels, which never read the workspace
                const bool bwd = ops[i] != QK_OP_FWD;
                PrepJob &j = jobs.j[m++];
                j.w = w[i]; j.wq = workspaces[i]; j.taps = taps_of(d); j.cq = d->cq; j.fq = d->fq;
                j.transposed = bwd ? 1 : 0;
                j.small = 0; j.kin = 0; j.n_ot = 0;
                j.ch_major = d->kernel_order == QK_KERNEL_CHANNEL_MAJOR;
                j.neg_ijk = bwd ? (d->conj ? 1 : 0) : (d->conj ? 0 : 1);       // the sign table go16 folds into the kernel
                // 16 / 32-channel layers: a second job writes the fragment layout of k_hconv16_small into the region behind the band
                // layout (the shape alone decides that the region exists, exactly as go16 and qk_conv_workspace_bytes see it)
                const KernelWs kw = kernel_ws(d, bwd ? QK_OP_BWD_DATA : QK_OP_FWD);
                if (kw.small) {
                    PrepJob &k = jobs.j[m++];
                    k = j;
                    k.wq = static_cast<char *>(workspaces[i]) + kw.band;
                    k.small = 1; k.kin = kw.sm.kin; k.n_ot = kw.sm.n_ot;
                }
            }
            if (m >= 31 || (i == n && m > 0)) {
                if (int rc = launch_prep_w16_batch(dt, jobs, m, (hipStream_t)stream)) return check_launch(rc, "qk_conv_prep_kernels");
                m = 0;
            }
        }
    }
    for (int i = 0; i < n; ++i)
        if (descs[i]->dtype != QK_BF16 && descs[i]->dtype != QK_F16) { set_error("qk_conv_prep_kernels: job %d is not a 16-bit descriptor", i); return QK_ERR_INVALID_ARG; }
    return QK_OK;
}

int qk_adam_step(float *param, const float *grad, float *m, float *v, size_t n, float lr, float beta1,
                 float beta2, float eps, int32_t step, float grad_scale, void *stream)
{
    if (!param || !grad || !m || !v) { set_error("adam: NULL buffer"); return QK_ERR_INVALID_ARG; }
    if (step < 1) { set_error("adam: step must be >= 1"); return QK_ERR_INVALID_ARG; }
    return check_launch(launch_adam(param, const_cast<float *>(grad), m, v, nullptr, n, lr, beta1, beta2, eps, step, grad_scale, false, (hipStream_t)stream), "qk_adam_step");
}

int qk_adam_step_zero_grad(float *param, float *grad, float *m, float *v, size_t n, float lr, float beta1,
                           float beta2, float eps, int32_t step, float grad_scale, void *stream)
{
    if (!param || !grad || !m || !v) { set_error("adam: NULL buffer"); return QK_ERR_INVALID_ARG; }
    if (step < 1) { set_error("adam: step must be >= 1"); return QK_ERR_INVALID_ARG; }
    return check_launch(launch_adam(param, grad, m, v, nullptr, n, lr, beta1, beta2, eps, step, grad_scale, true, (hipStream_t)stream), "qk_adam_step_zero_grad");
}

int qk_adam_step_l2(float *param, float *grad, float *m, float *v, const float *decay, size_t n, float lr, float beta1,
                    float beta2, float eps, int32_t step, float grad_scale, int32_t zero_grad, void *stream)
{
    if (!param || !grad || !m || !v) { set_error("adam: NULL buffer"); return QK_ERR_INVALID_ARG; }
    if (step < 1) { set_error("adam: step must be >= 1"); return QK_ERR_INVALID_ARG; }
    return check_launch(launch_adam(param, grad, m, v, decay, n, lr, beta1, beta2, eps, step, grad_scale, zero_grad != 0, (hipStream_t)stream), "qk_adam_step_l2");
}

int qk_adam_step_dev(float *param, float *grad, float *m, float *v, const float *decay, size_t n, float lr, float beta1,
                     float beta2, float eps, int32_t *step_dev, float grad_scale, int32_t zero_grad, void *stream)
{
    if (!param || !grad || !m || !v || !step_dev) { set_error("adam: NULL buffer"); return QK_ERR_INVALID_ARG; }
    return check_launch(launch_adam(param, grad, m, v, decay, n, lr, beta1, beta2, eps, 1, grad_scale, zero_grad != 0, (hipStream_t)stream, step_dev), "qk_adam_step_dev");
}

static bool guard_config_ok(const qk_grad_guard_config_t *c, const char *what)
{
    if (!c) { set_error("%s: NULL config", what); return false; }
    if (!(c->clipnorm >= 0.f) || !(c->clipvalue >= 0.f)) { set_error("%s: clipnorm / clipvalue must be >= 0", what); return false; }
    if (c->dynamic && !(c->backoff_factor > 0.f && c->backoff_factor < 1.f && c->growth_factor > 1.f && c->growth_interval >= 1
                        && c->min_scale > 0.f && c->min_scale <= c->max_scale)) {
        set_error("%s: dynamic scaling needs 0 < backoff_factor < 1 < growth_factor, growth_interval >= 1, 0 < min_scale <= max_scale", what);
        return false;
    }
    return true;
}

size_t qk_grad_guard_workspace_bytes(size_t n) { return grad_guard_workspace_bytes(n); }

int qk_grad_guard_reduce(const float *grad, const float *param, const float *decay, size_t n, float grad_scale,
                         const qk_grad_guard_config_t *config, qk_grad_guard_state_t *state, void *workspace,
                         size_t workspace_bytes, void *stream)
{
    if (!grad || !state || !workspace) { set_error("qk_grad_guard_reduce: NULL grad, state or workspace"); return QK_ERR_INVALID_ARG; }
    if (n == 0) { set_error("qk_grad_guard_reduce: n must be > 0"); return QK_ERR_INVALID_ARG; }
    if ((param == nullptr) != (decay == nullptr)) { set_error("qk_grad_guard_reduce: param and decay go together"); return QK_ERR_INVALID_ARG; }
    if (!guard_config_ok(config, "qk_grad_guard_reduce")) return QK_ERR_INVALID_ARG;
    if (!aligned(grad, 4) || !aligned(state, 4) || (param && (!aligned(param, 4) || !aligned(decay, 4))) || !aligned(workspace, 16)) {
        set_error("qk_grad_guard_reduce: buffers need 4-byte alignment, the workspace 16-byte alignment");
        return QK_ERR_INVALID_ARG;
    }
    if (workspace_bytes < grad_guard_workspace_bytes(n)) {
        set_error("qk_grad_guard_reduce: workspace of %zu bytes, %zu needed", workspace_bytes, grad_guard_workspace_bytes(n));
        return QK_ERR_INVALID_ARG;
    }
    return check_launch(launch_grad_guard_reduce(grad, param, decay, n, grad_scale, *config, state, workspace, (hipStream_t)stream),
                        "qk_grad_guard_reduce");
}

int qk_adam_step_guarded(float *param, float *grad, float *m, float *v, const float *decay, size_t n, float lr, float beta1,
                         float beta2, float eps, int32_t *step_dev, int32_t zero_grad, const qk_grad_guard_config_t *config,
                         const qk_grad_guard_state_t *state, void *stream)
{
    if (!param || !grad || !m || !v || !step_dev || !state) { set_error("qk_adam_step_guarded: NULL buffer, step counter or state"); return QK_ERR_INVALID_ARG; }
    if (n == 0) { set_error("qk_adam_step_guarded: n must be > 0"); return QK_ERR_INVALID_ARG; }
    if (!guard_config_ok(config, "qk_adam_step_guarded")) return QK_ERR_INVALID_ARG;
    return check_launch(launch_adam_guarded(param, grad, m, v, decay, n, lr, beta1, beta2, eps, step_dev, zero_grad != 0, config->clipvalue,
                                            state, (hipStream_t)stream), "qk_adam_step_guarded");
}

}  // extern "C"
