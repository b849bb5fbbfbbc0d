// Depthwise quaternion convolution over time with a fused GLU gate (include/qk_dwconv.h): forward, backward-data, backward-weight.
//
// Vector kernels (QK_QDWCONV_PATH_VEC).  A workgroup of 256 threads owns (batch row, time tile, 32 units).
//   stage    thread = (frame, component, lane group): one 16-byte load of a (and of g) moves 8 (fp32: 4) consecutive units; the gated
//            input h = a * sigmoid(g) -- zero, by selection, outside [0, lengths[b]) -- is formed here ONCE per element and written to
//            LDS as fp32, [frame][component][32 units].  The tile's K - 1 halo frames are staged with it.
//   compute  thread = (unit, group of F consecutive frames): lanes 0..31 of a wave are the 32 units (ds_read_b32 serves a wave as two
//            halves of 32 lanes over 32 banks: no conflict).  The unit's taps are in registers, (KB, 4) floats with KB the
//            compile-time bucket 3 / 7 / 15 / 31 that holds K; the thread walks the F + K - 1 staged frames once, every frame
//            read from LDS once and used for up to F outputs.  All indices into the tap and accumulator arrays are compile-time
//            (the loops are unrolled; taps k >= K are skipped by a wave-uniform branch, never multiplied by a zero weight).
//   store    the F x 4 results go back into the same LDS buffer, and thread = (frame, component, lane group) again packs 8 (4)
//            units into one 16-byte store.  The backward-data kernel loads a and g of its output frames here and applies the
//            gate's derivative.
// The backward-data kernel IS the forward kernel on dy with the taps conjugated and reversed (pad_lo' = K - 1 - pad_lo).
// The backward-weight kernel stages h and dy of 32-frame tiles the same way; a thread owns (unit, 4 frames of the tile), keeps
// (KB, 4) + 4 sums in registers over EVERY tile of EVERY row of its slab, and the eight frame groups meet in LDS once per slab,
// summed in group order.  k_dw_reduce sums the slabs in slab order: no atomics anywhere.
//
// Generic kernels (QK_QDWCONV_PATH_GENERIC): any width, stride and alignment; a thread per (row, unit) with plain loops over the
// taps (the gate is re-evaluated per tap: correct before fast), a thread per (slab, tap, unit) for the weight partials.
#include "qk_common.h"
#include "qk_seq.h"
#include "../../include/qk_dwconv.h"

#include <math.h>

namespace qk {
namespace {

constexpr int kDwUnits = 32;           // units per workgroup of the vector kernels
constexpr int kDwFS = 4 * kDwUnits;    // LDS floats per staged frame
constexpr int kDwTile = 64;            // frames per tile, forward and backward-data
constexpr int kDwF = kDwTile / 8;      // frames per thread there
constexpr int kDwWTile = 32;           // frames per tile, backward-weight
constexpr int kDwWF = kDwWTile / 8;
constexpr int kDwMaxSlabs = 128;
constexpr int kDwMaxTaps = 31;

thread_local int g_dw_path = 0;

struct DwArgs {
    int B, T, Q, K, pad;             // pad: pad_lo of the descriptor
    int xr, xc, yr, yc;
    int slab_rows;
    const int *len;
    const void *a, *g, *dy;
    const float *w, *bias;
    void *y, *da, *dg;
    float *part;                     // (slabs, K + 1, 4 Q)
};

__device__ __forceinline__ float dw_sigmoid(float v) { return 1.f / (1.f + __expf(-v)); }
__device__ __forceinline__ int dw_len(const int *len, int b, int T)
{
    if (!len) return T;
    const int n = len[b];
    return n < 0 ? 0 : n > T ? T : n;
}

// acc += W (x) h: sixteen multiply-adds, each straight into its accumulator
__device__ __forceinline__ void dw_ham(float (&acc)[4], const float (&w)[4], const float (&h)[4])
{
    acc[0] = fmaf(-w[3], h[3], fmaf(-w[2], h[2], fmaf(-w[1], h[1], fmaf(w[0], h[0], acc[0]))));
    acc[1] = fmaf(-w[3], h[2], fmaf(w[2], h[3], fmaf(w[1], h[0], fmaf(w[0], h[1], acc[1]))));
    acc[2] = fmaf(w[3], h[1], fmaf(w[2], h[0], fmaf(-w[1], h[3], fmaf(w[0], h[2], acc[2]))));
    acc[3] = fmaf(w[3], h[0], fmaf(-w[2], h[1], fmaf(w[1], h[2], fmaf(w[0], h[3], acc[3]))));
}
// acc += d (x) conj(h)
__device__ __forceinline__ void dw_ham_conj(float (&acc)[4], const float (&d)[4], const float (&h)[4])
{
    acc[0] = fmaf(d[3], h[3], fmaf(d[2], h[2], fmaf(d[1], h[1], fmaf(d[0], h[0], acc[0]))));
    acc[1] = fmaf(d[3], h[2], fmaf(-d[2], h[3], fmaf(-d[0], h[1], fmaf(d[1], h[0], acc[1]))));
    acc[2] = fmaf(-d[3], h[1], fmaf(d[1], h[3], fmaf(-d[0], h[2], fmaf(d[2], h[0], acc[2]))));
    acc[3] = fmaf(d[2], h[1], fmaf(-d[1], h[2], fmaf(-d[0], h[3], fmaf(d[3], h[0], acc[3]))));
}

// Stage `frames` frames, the first one frame t_first of batch row b, of the 32 units from ub on into sh ([frame][4][32] fp32).
// GATED: src = a, gate = g (may be NULL): h = a * sigmoid(g); else src as it is.  Frames outside [0, n) and units >= Q: zeros.
template <typename T>
__device__ __forceinline__ void dw_stage(float *sh, int frames, int t_first, int n, size_t row0, int row, int comp, int ub, int Q,
                                         const T *src, const T *gate)
{
    constexpr int V = Vec16<T>::V, G = kDwUnits / V;
    for (int it = threadIdx.x; it < frames * 4 * G; it += 256) {
        const int gq = it % G, c = (it / G) & 3, j = it / (4 * G);
        const int t = t_first + j, u0 = ub + gq * V;
        float h[V];
#pragma unroll
        for (int e = 0; e < V; ++e) h[e] = 0.f;
        if (t >= 0 && t < n && u0 < Q) {
            const size_t off = (row0 + (size_t)t) * (size_t)row + (size_t)c * comp + u0;
            Vec16<T>::unpack(load16(src + off), h);
            if (gate) {
                float gv[V];
                Vec16<T>::unpack(load16(gate + off), gv);
#pragma unroll
                for (int e = 0; e < V; ++e) h[e] *= dw_sigmoid(gv[e]);
            }
        }
        float *dst = sh + j * kDwFS + c * kDwUnits + gq * V;
#pragma unroll
        for (int e = 0; e < V; e += 4) *reinterpret_cast<float4 *>(dst + e) = make_float4(h[e], h[e + 1], h[e + 2], h[e + 3]);
    }
}

// ---- vector forward (BWD = false) and backward-data (BWD = true) ------------------------------------------------------------------
template <typename T, int KB, bool BWD>
__global__ __launch_bounds__(256) void k_dw_conv(const DwArgs p)
{
    constexpr int V = Vec16<T>::V, G = kDwUnits / V;
    __shared__ __attribute__((aligned(16))) float sh[(kDwTile + KB - 1) * kDwFS];
    const int b = blockIdx.z, t0 = blockIdx.x * kDwTile, ub = blockIdx.y * kDwUnits;
    const int K = p.K, Q = p.Q;
    const int n = dw_len(p.len, b, p.T);
    const size_t row0 = (size_t)b * p.T;
    const bool live = t0 < n;                       // block-uniform
    if (live) {
        const int pad = BWD ? K - 1 - p.pad : p.pad;
        if (BWD) dw_stage<T>(sh, kDwTile + K - 1, t0 - pad, n, row0, p.yr, p.yc, ub, Q, (const T *)p.dy, nullptr);
        else dw_stage<T>(sh, kDwTile + K - 1, t0 - pad, n, row0, p.xr, p.xc, ub, Q, (const T *)p.a, (const T *)p.g);
        __syncthreads();
        const int u = threadIdx.x & (kDwUnits - 1), fg = threadIdx.x / kDwUnits;
        const int unit = ub + u;
        float w[KB][4], acc[kDwF][4];
#pragma unroll
        for (int k = 0; k < KB; ++k) {
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                float v = 0.f;
                if (k < K && unit < Q) {
                    // backward-data: tap k is conj(W[K - 1 - k])
                    v = p.w[(size_t)(BWD ? K - 1 - k : k) * 4 * Q + (size_t)c * Q + unit];
                    if (BWD && c > 0) v = -v;
                }
                w[k][c] = v;
            }
        }
#pragma unroll
        for (int f = 0; f < kDwF; ++f) {
#pragma unroll
            for (int c = 0; c < 4; ++c) acc[f][c] = (!BWD && p.bias && unit < Q) ? p.bias[(size_t)c * Q + unit] : 0.f;
        }
        const float *hp = sh + fg * kDwF * kDwFS + u;
#pragma unroll
        for (int j = 0; j < kDwF + KB - 1; ++j) {
            if (j < kDwF + K - 1) {
                const float h[4] = {hp[j * kDwFS], hp[j * kDwFS + kDwUnits], hp[j * kDwFS + 2 * kDwUnits], hp[j * kDwFS + 3 * kDwUnits]};
#pragma unroll
                for (int f = 0; f < kDwF; ++f) {
                    if (j - f >= 0 && j - f < KB) {          // compile-time after unrolling
                        if (j - f < K) dw_ham(acc[f], w[j - f < 0 ? 0 : j - f >= KB ? 0 : j - f], h);
                    }
                }
            }
        }
        __syncthreads();                            // every thread has read what it needs of the staged input
#pragma unroll
        for (int f = 0; f < kDwF; ++f) {
#pragma unroll
            for (int c = 0; c < 4; ++c) sh[(fg * kDwF + f) * kDwFS + c * kDwUnits + u] = acc[f][c];
        }
        __syncthreads();
    }
    for (int it = threadIdx.x; it < kDwTile * 4 * G; it += 256) {
        const int gq = it % G, c = (it / G) & 3, f = it / (4 * G);
        const int t = t0 + f, u0 = ub + gq * V;
        if (t >= p.T || u0 >= Q) continue;
        float o[V];
#pragma unroll
        for (int e = 0; e < V; ++e) o[e] = 0.f;
        const bool on = live && t < n;
        if (on) {
            const float *src = sh + f * kDwFS + c * kDwUnits + gq * V;
#pragma unroll
            for (int e = 0; e < V; ++e) o[e] = src[e];
        }
        if (!BWD) {
            store16((T *)p.y + (row0 + t) * (size_t)p.yr + (size_t)c * p.yc + u0, Vec16<T>::pack(o));
        } else {
            const size_t off = (row0 + t) * (size_t)p.xr + (size_t)c * p.xc + u0;
            if (p.g) {
                float og[V];
#pragma unroll
                for (int e = 0; e < V; ++e) og[e] = 0.f;
                if (on) {
                    float av[V], gv[V];
                    Vec16<T>::unpack(load16((const T *)p.a + off), av);
                    Vec16<T>::unpack(load16((const T *)p.g + off), gv);
#pragma unroll
                    for (int e = 0; e < V; ++e) {
                        const float s = dw_sigmoid(gv[e]);
                        og[e] = o[e] * av[e] * s * (1.f - s);
                        o[e] *= s;
                    }
                }
                store16((T *)p.dg + off, Vec16<T>::pack(og));
            }
            store16((T *)p.da + off, Vec16<T>::pack(o));
        }
    }
}

// ---- vector backward-weight: the partial of slab blockIdx.x for 32 units ----------------------------------------------------------
template <typename T, int KB>
__global__ __launch_bounds__(256) void k_dw_wgrad(const DwArgs p)
{
    __shared__ __attribute__((aligned(16))) float sh_h[(kDwWTile + KB - 1) * kDwFS];
    __shared__ __attribute__((aligned(16))) float sh_d[kDwWTile * kDwFS];
    const int ub = blockIdx.y * kDwUnits, K = p.K, Q = p.Q;
    const int u = threadIdx.x & (kDwUnits - 1), fg = threadIdx.x / kDwUnits;
    float acc[KB][4], accb[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) accb[c] = 0.f;
#pragma unroll
    for (int k = 0; k < KB; ++k) {
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[k][c] = 0.f;
    }
    const int b0 = blockIdx.x * p.slab_rows, b1 = min(p.B, b0 + p.slab_rows);
    for (int b = b0; b < b1; ++b) {
        const int n = dw_len(p.len, b, p.T);
        const size_t row0 = (size_t)b * p.T;
        for (int t0 = 0; t0 < n; t0 += kDwWTile) {
            __syncthreads();                        // the previous tile has been read
            dw_stage<T>(sh_h, kDwWTile + K - 1, t0 - p.pad, n, row0, p.xr, p.xc, ub, Q, (const T *)p.a, (const T *)p.g);
            dw_stage<T>(sh_d, kDwWTile, t0, n, row0, p.yr, p.yc, ub, Q, (const T *)p.dy, nullptr);
            __syncthreads();
            float d[kDwWF][4];
#pragma unroll
            for (int f = 0; f < kDwWF; ++f) {
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    d[f][c] = sh_d[(fg * kDwWF + f) * kDwFS + c * kDwUnits + u];
                    accb[c] += d[f][c];
                }
            }
            const float *hp = sh_h + fg * kDwWF * kDwFS + u;
#pragma unroll
            for (int j = 0; j < kDwWF + KB - 1; ++j) {
                if (j < kDwWF + K - 1) {
                    const float h[4] = {hp[j * kDwFS], hp[j * kDwFS + kDwUnits], hp[j * kDwFS + 2 * kDwUnits], hp[j * kDwFS + 3 * kDwUnits]};
#pragma unroll
                    for (int f = 0; f < kDwWF; ++f) {
                        if (j - f >= 0 && j - f < KB) {      // compile-time after unrolling
                            if (j - f < K) dw_ham_conj(acc[j - f < 0 ? 0 : j - f >= KB ? 0 : j - f], d[f], h);
                        }
                    }
                }
            }
        }
    }
    // the eight frame groups' sums of every (tap, component, unit), added in group order; line K is the bias
    float *line = p.part + (size_t)blockIdx.x * (K + 1) * 4 * Q;
#pragma unroll
    for (int k = 0; k <= KB; ++k) {
        if (k < K || k == KB) {
            __syncthreads();
#pragma unroll
            for (int c = 0; c < 4; ++c) sh_h[(fg * 4 + c) * kDwUnits + u] = k < KB ? acc[k < KB ? k : 0][c] : accb[c];
            __syncthreads();
            if (threadIdx.x < 4 * kDwUnits) {
                const int c = threadIdx.x / kDwUnits;
                float s = 0.f;
#pragma unroll
                for (int g = 0; g < 8; ++g) s += sh_h[(g * 4 + c) * kDwUnits + u];
                if (ub + u < Q) line[(size_t)(k < KB ? k : K) * 4 * Q + (size_t)c * Q + ub + u] = s;
            }
        }
    }
}

// ---- the slabs' partials -> dw, dbias: one thread per column, the slabs in order --------------------------------------------------
__global__ __launch_bounds__(256) void k_dw_reduce(const float *part, int slabs, int K, int Q, float *dw, float *dbias)
{
    const int cols = (K + 1) * 4 * Q, nw = K * 4 * Q;
    const int col = blockIdx.x * 256 + threadIdx.x;
    if (col >= cols) return;
    float s = 0.f;
    for (int i = 0; i < slabs; ++i) s += part[(size_t)i * cols + col];
    if (col < nw) { if (dw) dw[col] = s; }
    else if (dbias) dbias[col - nw] = s;
}

// ---- generic kernels --------------------------------------------------------------------------------------------------------------
template <typename T>
__device__ __forceinline__ void dw_gated(const DwArgs &p, size_t off, float (&h)[4])
{
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        h[c] = to_f32(((const T *)p.a)[off + (size_t)c * p.xc]);
        if (p.g) h[c] *= dw_sigmoid(to_f32(((const T *)p.g)[off + (size_t)c * p.xc]));
    }
}

template <typename T>
__global__ __launch_bounds__(256) void k_dw_fwd_gen(const DwArgs p)
{
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (size_t)p.B * p.T * p.Q) return;
    const int u = (int)(idx % p.Q);
    const size_t r = idx / p.Q;
    const int b = (int)(r / p.T), t = (int)(r % p.T), Q = p.Q;
    const int n = dw_len(p.len, b, p.T);
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    if (t < n) {
        if (p.bias) {
#pragma unroll
            for (int c = 0; c < 4; ++c) acc[c] = p.bias[(size_t)c * Q + u];
        }
        for (int k = 0; k < p.K; ++k) {
            const int tt = t + k - p.pad;
            if (tt < 0 || tt >= n) continue;
            float h[4], w[4];
            dw_gated<T>(p, ((size_t)b * p.T + tt) * (size_t)p.xr + u, h);
#pragma unroll
            for (int c = 0; c < 4; ++c) w[c] = p.w[(size_t)k * 4 * Q + (size_t)c * Q + u];
            dw_ham(acc, w, h);
        }
    }
    T *y = (T *)p.y + r * (size_t)p.yr + u;
#pragma unroll
    for (int c = 0; c < 4; ++c) y[(size_t)c * p.yc] = from_f32<T>(acc[c]);
}

template <typename T>
__global__ __launch_bounds__(256) void k_dw_bwd_gen(const DwArgs p)
{
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (size_t)p.B * p.T * p.Q) return;
    const int u = (int)(idx % p.Q);
    const size_t r = idx / p.Q;
    const int b = (int)(r / p.T), t = (int)(r % p.T), Q = p.Q;
    const int n = dw_len(p.len, b, p.T);
    float dh[4] = {0.f, 0.f, 0.f, 0.f}, dgv[4] = {0.f, 0.f, 0.f, 0.f};
    const size_t off = r * (size_t)p.xr + u;
    if (t < n) {
        for (int k = 0; k < p.K; ++k) {
            const int tt = t + p.pad - k;
            if (tt < 0 || tt >= n) continue;
            float d[4], w[4];
            const T *dy = (const T *)p.dy + ((size_t)b * p.T + tt) * (size_t)p.yr + u;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                d[c] = to_f32(dy[(size_t)c * p.yc]);
                w[c] = p.w[(size_t)k * 4 * Q + (size_t)c * Q + u];
                if (c > 0) w[c] = -w[c];
            }
            dw_ham(dh, w, d);
        }
        if (p.g) {
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const float av = to_f32(((const T *)p.a)[off + (size_t)c * p.xc]);
                const float s = dw_sigmoid(to_f32(((const T *)p.g)[off + (size_t)c * p.xc]));
                dgv[c] = dh[c] * av * s * (1.f - s);
                dh[c] *= s;
            }
        }
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        ((T *)p.da)[off + (size_t)c * p.xc] = from_f32<T>(dh[c]);
        if (p.g) ((T *)p.dg)[off + (size_t)c * p.xc] = from_f32<T>(dgv[c]);
    }
}

// the partial of slab blockIdx.z, line blockIdx.y (tap k, or K: the bias): one thread per unit, rows and frames in order
template <typename T>
__global__ __launch_bounds__(64) void k_dw_part_gen(const DwArgs p)
{
    const int u = blockIdx.x * 64 + threadIdx.x, k = blockIdx.y, Q = p.Q;
    if (u >= Q) return;
    const int b0 = blockIdx.z * p.slab_rows, b1 = min(p.B, b0 + p.slab_rows);
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int b = b0; b < b1; ++b) {
        const int n = dw_len(p.len, b, p.T);
        for (int t = 0; t < n; ++t) {
            float d[4];
            const T *dy = (const T *)p.dy + ((size_t)b * p.T + t) * (size_t)p.yr + u;
#pragma unroll
            for (int c = 0; c < 4; ++c) d[c] = to_f32(dy[(size_t)c * p.yc]);
            if (k == p.K) {
#pragma unroll
                for (int c = 0; c < 4; ++c) acc[c] += d[c];
                continue;
            }
            const int tt = t + k - p.pad;
            if (tt < 0 || tt >= n) continue;
            float h[4];
            dw_gated<T>(p, ((size_t)b * p.T + tt) * (size_t)p.xr + u, h);
            dw_ham_conj(acc, d, h);
        }
    }
    float *line = p.part + ((size_t)blockIdx.z * (p.K + 1) + k) * 4 * Q;
#pragma unroll
    for (int c = 0; c < 4; ++c) line[(size_t)c * Q + u] = acc[c];
}

// ---- host -------------------------------------------------------------------------------------------------------------------------
bool dw_desc_ok(const qk_qdwconv_desc_t *d, const char *what)
{
    if (!desc_head_ok(d, what)) return false;
    if (d->batch < 1 || d->steps < 1 || d->units < 1) {
        set_error("%s: batch, steps and units must be >= 1 (got %d, %d, %d)", what, d->batch, d->steps, d->units);
        return false;
    }
    if (d->taps < 1 || d->taps > kDwMaxTaps) { set_error("%s: taps must be 1 .. %d (got %d)", what, kDwMaxTaps, d->taps); return false; }
    if (d->pad_lo < 0 || d->pad_lo >= d->taps) { set_error("%s: pad_lo must be 0 .. taps - 1 = %d (got %d)", what, d->taps - 1, d->pad_lo); return false; }
    if (d->units > (1 << 20) || d->batch > 65535 || d->x_row > (1 << 28) || d->y_row > (1 << 28) || (long long)d->batch * d->steps * d->units > (1ll << 38)) {
        set_error("%s: shape out of range (batch %d, steps %d, units %d)", what, d->batch, d->steps, d->units);
        return false;
    }
    if (d->x_comp < d->units || d->y_comp < d->units) {
        set_error("%s: x_comp %d and y_comp %d must be >= units = %d", what, d->x_comp, d->y_comp, d->units);
        return false;
    }
    if ((long long)d->x_row < 3ll * d->x_comp + d->units || (long long)d->y_row < 3ll * d->y_comp + d->units) {
        set_error("%s: a row stride must be >= 3 comp + units (x: %d / %d, y: %d / %d, units %d)", what, d->x_row, d->x_comp, d->y_row,
                  d->y_comp, d->units);
        return false;
    }
    if (d->flags != 0) { set_error("%s: unknown flags 0x%x", what, d->flags); return false; }
    return true;
}

int dw_path(const qk_qdwconv_desc_t *d)
{
    const int v = vec_width(d->dtype);
    return d->units % v == 0 && d->x_row % v == 0 && d->x_comp % v == 0 && d->y_row % v == 0 && d->y_comp % v == 0
               ? QK_QDWCONV_PATH_VEC : QK_QDWCONV_PATH_GENERIC;
}

int dw_slab_rows(const qk_qdwconv_desc_t *d) { return (d->batch + kDwMaxSlabs - 1) / kDwMaxSlabs; }
int dw_slabs(const qk_qdwconv_desc_t *d) { const int r = dw_slab_rows(d); return (d->batch + r - 1) / r; }

DwArgs dw_args(const qk_qdwconv_desc_t *d)
{
    DwArgs a = {};
    a.B = d->batch; a.T = d->steps; a.Q = d->units; a.K = d->taps; a.pad = d->pad_lo;
    a.xr = d->x_row; a.xc = d->x_comp; a.yr = d->y_row; a.yc = d->y_comp;
    a.slab_rows = dw_slab_rows(d);
    return a;
}

template <typename T, bool BWD>
void dw_launch_conv(const DwArgs &a, hipStream_t st)
{
    const dim3 grid((unsigned)((a.T + kDwTile - 1) / kDwTile), (unsigned)((a.Q + kDwUnits - 1) / kDwUnits), (unsigned)a.B);
    if (a.K <= 3) hipLaunchKernelGGL((k_dw_conv<T, 3, BWD>), grid, dim3(256), 0, st, a);
    else if (a.K <= 7) hipLaunchKernelGGL((k_dw_conv<T, 7, BWD>), grid, dim3(256), 0, st, a);
    else if (a.K <= 15) hipLaunchKernelGGL((k_dw_conv<T, 15, BWD>), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((k_dw_conv<T, 31, BWD>), grid, dim3(256), 0, st, a);
}

template <typename T>
void dw_launch_wgrad(const DwArgs &a, int slabs, hipStream_t st)
{
    const dim3 grid((unsigned)slabs, (unsigned)((a.Q + kDwUnits - 1) / kDwUnits));
    if (a.K <= 3) hipLaunchKernelGGL((k_dw_wgrad<T, 3>), grid, dim3(256), 0, st, a);
    else if (a.K <= 7) hipLaunchKernelGGL((k_dw_wgrad<T, 7>), grid, dim3(256), 0, st, a);
    else if (a.K <= 15) hipLaunchKernelGGL((k_dw_wgrad<T, 15>), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((k_dw_wgrad<T, 31>), grid, dim3(256), 0, st, a);
}

unsigned dw_elem_blocks(const DwArgs &a) { return (unsigned)(((size_t)a.B * a.T * a.Q + 255) / 256); }

}  // namespace
}  // namespace qk

using namespace qk;

extern "C" {

int qk_qdwconv_supported(const qk_qdwconv_desc_t *desc)
{
    return dw_desc_ok(desc, "qk_qdwconv_supported") ? dw_path(desc) : 0;
}

size_t qk_qdwconv_workspace_bytes(const qk_qdwconv_desc_t *desc, int32_t op)
{
    if (!dw_desc_ok(desc, "qk_qdwconv_workspace_bytes")) return 0;
    if (op == QK_OP_FWD) return 0;
    if (op == QK_OP_BWD) return (size_t)dw_slabs(desc) * (desc->taps + 1) * 4 * desc->units * sizeof(float);
    return bad_op("qk_qdwconv_workspace_bytes", op);
}

int qk_qdwconv_last_path(void) { return g_dw_path; }

int qk_qdwconv_fwd(const qk_qdwconv_desc_t *desc, const void *a, const void *g, const float *w, const float *bias,
                   const int32_t *lengths, void *y, void *stream)
{
    const char *what = "qk_qdwconv_fwd";
    if (!dw_desc_ok(desc, what)) return QK_ERR_INVALID_ARG;
    if (!a || !w || !y) { set_error("%s: NULL buffer", what); return QK_ERR_INVALID_ARG; }
    const size_t es = elem_size(desc->dtype);
    if (!aligned(a, es) || !aligned(g, es) || !aligned(y, es) || !aligned(w, 4) || !aligned(bias, 4) || !aligned(lengths, 4)) {
        set_error("%s: misaligned buffer", what);
        return QK_ERR_INVALID_ARG;
    }
    hipStream_t st = (hipStream_t)stream;
    DwArgs p = dw_args(desc);
    p.len = lengths; p.a = a; p.g = g; p.w = w; p.bias = bias; p.y = y;
    const bool vec = dw_path(desc) == QK_QDWCONV_PATH_VEC && aligned(a, 16) && aligned(g, 16) && aligned(y, 16);
    if (vec) {
        by_dtype(desc->dtype, [&](auto t) { dw_launch_conv<decltype(t), false>(p, st); });
    } else {
        const unsigned blocks = dw_elem_blocks(p);
        by_dtype(desc->dtype, [&](auto t) { hipLaunchKernelGGL((k_dw_fwd_gen<decltype(t)>), dim3(blocks), dim3(256), 0, st, p); });
    }
    g_dw_path = vec ? QK_QDWCONV_PATH_VEC : QK_QDWCONV_PATH_GENERIC;
    return launched(what);
}

int qk_qdwconv_bwd(const qk_qdwconv_desc_t *desc, const void *dy, const void *a, const void *g, const float *w,
                   const int32_t *lengths, void *da, void *dg, float *dw, float *dbias, void *workspace, size_t workspace_bytes,
                   void *stream)
{
    const char *what = "qk_qdwconv_bwd";
    if (!dw_desc_ok(desc, what)) return QK_ERR_INVALID_ARG;
    if (!dy || !a || !w || !da) { set_error("%s: NULL buffer", what); return QK_ERR_INVALID_ARG; }
    if ((g == nullptr) != (dg == nullptr)) { set_error("%s: g and dg must both be given or both be NULL", what); return QK_ERR_INVALID_ARG; }
    const size_t es = elem_size(desc->dtype);
    if (!aligned(dy, es) || !aligned(a, es) || !aligned(g, es) || !aligned(da, es) || !aligned(dg, es) || !aligned(w, 4)
        || !aligned(lengths, 4) || !aligned(dw, 4) || !aligned(dbias, 4) || !aligned(workspace, 16)) {
        set_error("%s: misaligned buffer (16 bytes for the workspace)", what);
        return QK_ERR_INVALID_ARG;
    }
    const bool wg = dw || dbias;
    const size_t need = wg ? qk_qdwconv_workspace_bytes(desc, QK_OP_BWD) : 0;
    if (wg && workspace_ok(what, workspace, workspace_bytes, need) != QK_OK) return QK_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    DwArgs p = dw_args(desc);
    p.len = lengths; p.dy = dy; p.a = a; p.g = g; p.w = w; p.da = da; p.dg = dg; p.part = wg ? (float *)workspace : nullptr;
    const int slabs = dw_slabs(desc);
    const bool vec = dw_path(desc) == QK_QDWCONV_PATH_VEC && aligned(dy, 16) && aligned(a, 16) && aligned(g, 16) && aligned(da, 16)
                     && aligned(dg, 16);
    if (vec) {
        by_dtype(desc->dtype, [&](auto t) {
            dw_launch_conv<decltype(t), true>(p, st);
            if (wg) dw_launch_wgrad<decltype(t)>(p, slabs, st);
        });
    } else {
        const unsigned blocks = dw_elem_blocks(p);
        const dim3 pgrid((unsigned)((desc->units + 63) / 64), (unsigned)(desc->taps + 1), (unsigned)slabs);
        by_dtype(desc->dtype, [&](auto t) {
            hipLaunchKernelGGL((k_dw_bwd_gen<decltype(t)>), dim3(blocks), dim3(256), 0, st, p);
            if (wg) hipLaunchKernelGGL((k_dw_part_gen<decltype(t)>), pgrid, dim3(64), 0, st, p);
        });
    }
    if (wg) {
        const int cols = (desc->taps + 1) * 4 * desc->units;
        hipLaunchKernelGGL(k_dw_reduce, dim3((unsigned)((cols + 255) / 256)), dim3(256), 0, st, (const float *)workspace, slabs, desc->taps,
                           desc->units, dw, dbias);
    }
    g_dw_path = vec ? QK_QDWCONV_PATH_VEC : QK_QDWCONV_PATH_GENERIC;
    return launched(what);
}

}  // extern "C"
