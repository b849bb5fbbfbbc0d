// Quaternion layer normalisation (include/qk_norm.h): per row four component means, ONE centred variance, one gamma per quaternion
// unit, beta per column; forward and backward, fused.
//
// Vector kernels (QK_QLNORM_PATH_VEC).  One wave owns a row.  A lane's group p holds units (lane + 64 p) V .. + V - 1 of ALL FOUR
// components, V = 8 for the 16-bit types and 4 for fp32: four 16-byte loads per group, one per component, each a contiguous 1 KB
// per wave.  P groups per lane (template): 16-bit P = 1 (Q <= 512), 2 (Q <= 1024); fp32 P = 1, 2, 4 (Q <= 256, 512, 1024).  The
// row lives in registers from its one read to its one write; the means (summed relative to the row's first unit: x = 1000 + noise
// keeps its digits), the centred variance and the backward's five sums are xor-butterflies over the wave.  A lane keeps the same
// columns for every row its wave visits, so gamma / beta are loaded once per wave, and the backward's dbeta / dgamma partials
// stay in that lane's registers over the whole slab: the four waves of the workgroup meet in LDS once per slab (summed in wave
// order) and wave 0 writes the slab's partial.  k_qln_reduce sums the slabs: no atomics anywhere.
//
// Generic kernels (QK_QLNORM_PATH_GENERIC): any width, stride and alignment; a wave per row with lanes striding over the units,
// three (backward: two) passes over the row, the second and third served by the cache; the weight-gradient partials of a slab by
// a thread per unit.  Correct before fast.
#include "qk_common.h"
#include "qk_seq.h"
#include "../../include/qk_norm.h"

#include <math.h>

namespace qk {
namespace {

constexpr int kQnMaxQ = 1024;          // widest row the vector kernels keep in registers
constexpr int kQnSlabTarget = 768;     // slabs aimed at for large inputs: three resident workgroups (the backward's registers) on each of 256 CUs
constexpr int kQnSlabMin = 16;         // rows per slab at least (a multiple of the four waves)

// v + (v of the lane a DPP control names); every lane is active and every source lane exists
template <int CTRL>
__device__ __forceinline__ float qn_dpp_add(float v)
{
    return v + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, false));
}
// sum over the 64 lanes, every lane gets the total; the same tree for every call: bit-repeatable.  Inside a row of 16 lanes the
// butterfly runs on DPP (lane ^ 1, lane ^ 2 as quad permutations; then the quads of a half row and the half rows of a row hold one
// value each, so the two mirrors pair them); across the four rows two shuffles.
template <int N>
__device__ __forceinline__ void qn_wave_sum(float (&v)[N])
{
#pragma unroll
    for (int i = 0; i < N; ++i) {
        float t = qn_dpp_add<0xB1>(v[i]);       // quad_perm [1, 0, 3, 2]
        t = qn_dpp_add<0x4E>(t);                // quad_perm [2, 3, 0, 1]
        t = qn_dpp_add<0x141>(t);               // row_half_mirror
        v[i] = qn_dpp_add<0x140>(t);            // row_mirror
    }
#pragma unroll
    for (int off = 16; off <= 32; off <<= 1) {
#pragma unroll
        for (int i = 0; i < N; ++i) v[i] += __shfl_xor(v[i], off, 64);
    }
}
__device__ __forceinline__ float qn_first_lane(float v) { return __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(v))); }

struct QnFwd {
    int rows, steps, Q, xs, ys;
    float eps;
    const int *len;
    const void *x;
    const float *gamma, *beta;
    void *y;
    float *stats;
};

struct QnBwd {
    int rows, steps, Q, xs, ys, slab_rows;
    const int *len;
    const void *dy, *x;
    const float *gamma, *stats;
    void *dx;
    float *part;             // (slabs, 5 Q): dbeta (4 Q) | dgamma (Q) of each slab
};

__device__ __forceinline__ bool qn_active(const int *len, int steps, int row)
{
    if (!len) return true;
    const int b = row / steps;
    return row - b * steps < len[b];
}

// ---- vector forward ---------------------------------------------------------------------------------------------------------------
template <typename T, int P>
__global__ __launch_bounds__(256) void k_qln_fwd(const QnFwd a)
{
    constexpr int V = Vec16<T>::V;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int Q = a.Q;
    const T *x = (const T *)a.x;
    T *y = (T *)a.y;
    float gm[P][V], bt[P][4][V];
    bool ok[P];
#pragma unroll
    for (int p = 0; p < P; ++p) {
        const int u0 = (lane + 64 * p) * V;
        ok[p] = u0 < Q;
#pragma unroll
        for (int e = 0; e < V; ++e) {
            gm[p][e] = 1.f;
#pragma unroll
            for (int c = 0; c < 4; ++c) bt[p][c][e] = 0.f;
        }
        if (ok[p]) {
#pragma unroll
            for (int e = 0; e < V; e += 4) {
                if (a.gamma) load4(a.gamma + u0 + e, *reinterpret_cast<float (*)[4]>(&gm[p][e]));
                if (a.beta) {
#pragma unroll
                    for (int c = 0; c < 4; ++c) load4(a.beta + c * Q + u0 + e, *reinterpret_cast<float (*)[4]>(&bt[p][c][e]));
                }
            }
        }
    }
    const float inv_q = 1.f / (float)Q, inv_4q = 1.f / (4.f * (float)Q);
    for (int row = blockIdx.x * 4 + wave; row < a.rows; row += gridDim.x * 4) {
        T *yr = y + (size_t)row * a.ys;
        float *st = a.stats + (size_t)row * 5;
        if (!qn_active(a.len, a.steps, row)) {
#pragma unroll
            for (int p = 0; p < P; ++p)
                if (ok[p]) {
#pragma unroll
                    for (int c = 0; c < 4; ++c) store16(yr + c * Q + (lane + 64 * p) * V, make_uint4(0u, 0u, 0u, 0u));
                }
            if (lane < 5) st[lane] = 0.f;
            continue;
        }
        const T *xr = x + (size_t)row * a.xs;
        float v[P][4][V];
#pragma unroll
        for (int p = 0; p < P; ++p) {
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                uint4 raw = make_uint4(0u, 0u, 0u, 0u);
                if (ok[p]) raw = load16(xr + c * Q + (lane + 64 * p) * V);
                Vec16<T>::unpack(raw, v[p][c]);
            }
        }
        // the means, relative to the row's first unit (lane 0, group 0 always holds it)
        float piv[4], sum[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) { piv[c] = qn_first_lane(v[0][c][0]); sum[c] = 0.f; }
#pragma unroll
        for (int p = 0; p < P; ++p) {
            if (ok[p]) {
#pragma unroll
                for (int c = 0; c < 4; ++c) {
#pragma unroll
                    for (int e = 0; e < V; ++e) { v[p][c][e] -= piv[c]; sum[c] += v[p][c][e]; }
                }
            }
        }
        qn_wave_sum<4>(sum);
        float sq[1] = {0.f};
#pragma unroll
        for (int c = 0; c < 4; ++c) sum[c] *= inv_q;
#pragma unroll
        for (int p = 0; p < P; ++p) {
            if (ok[p]) {
#pragma unroll
                for (int c = 0; c < 4; ++c) {
#pragma unroll
                    for (int e = 0; e < V; ++e) { v[p][c][e] -= sum[c]; sq[0] += v[p][c][e] * v[p][c][e]; }
                }
            }
        }
        qn_wave_sum<1>(sq);
        const float rstd = 1.f / sqrtf(sq[0] * inv_4q + a.eps);
#pragma unroll
        for (int p = 0; p < P; ++p) {
            if (ok[p]) {
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    float o[V];
#pragma unroll
                    for (int e = 0; e < V; ++e) o[e] = gm[p][e] * (v[p][c][e] * rstd) + bt[p][c][e];
                    store16(yr + c * Q + (lane + 64 * p) * V, Vec16<T>::pack(o));
                }
            }
        }
        if (lane < 5) {
            float s = rstd;
#pragma unroll
            for (int c = 0; c < 4; ++c) s = lane == c ? piv[c] + sum[c] : s;
            st[lane] = s;
        }
    }
}

// ---- vector backward --------------------------------------------------------------------------------------------------------------
template <typename T, int P, bool WG>
__global__ __launch_bounds__(256) void k_qln_bwd(const QnBwd a)
{
    constexpr int V = Vec16<T>::V;
    __shared__ float red[3][V][64];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int Q = a.Q;
    const T *x = (const T *)a.x, *dy = (const T *)a.dy;
    T *dx = (T *)a.dx;
    float gm[P][V], acc[P][5][V];            // acc[p][c]: dbeta of component c; acc[p][4]: dgamma
    bool ok[P];
#pragma unroll
    for (int p = 0; p < P; ++p) {
        const int u0 = (lane + 64 * p) * V;
        ok[p] = u0 < Q;
#pragma unroll
        for (int e = 0; e < V; ++e) {
            gm[p][e] = 1.f;
#pragma unroll
            for (int k = 0; k < 5; ++k) acc[p][k][e] = 0.f;
        }
        if (ok[p] && a.gamma) {
#pragma unroll
            for (int e = 0; e < V; e += 4) load4(a.gamma + u0 + e, *reinterpret_cast<float (*)[4]>(&gm[p][e]));
        }
    }
    const float inv_q = 1.f / (float)Q, inv_4q = 1.f / (4.f * (float)Q);
    const int r0 = blockIdx.x * a.slab_rows, r1 = min(a.rows, r0 + a.slab_rows);
    for (int row = r0 + wave; row < r1; row += 4) {
        T *dxr = dx + (size_t)row * a.xs;
        if (!qn_active(a.len, a.steps, row)) {
#pragma unroll
            for (int p = 0; p < P; ++p)
                if (ok[p]) {
#pragma unroll
                    for (int c = 0; c < 4; ++c) store16(dxr + c * Q + (lane + 64 * p) * V, make_uint4(0u, 0u, 0u, 0u));
                }
            continue;
        }
        const T *xr = x + (size_t)row * a.xs, *dyr = dy + (size_t)row * a.ys;
        const float *st = a.stats + (size_t)row * 5;
        uint4 xraw[P][4], draw[P][4];
#pragma unroll
        for (int p = 0; p < P; ++p) {
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                xraw[p][c] = draw[p][c] = make_uint4(0u, 0u, 0u, 0u);
                if (ok[p]) {
                    xraw[p][c] = load16(xr + c * Q + (lane + 64 * p) * V);
                    draw[p][c] = load16(dyr + c * Q + (lane + 64 * p) * V);
                }
            }
        }
        const float mu[4] = {st[0], st[1], st[2], st[3]}, rstd = st[4];
        float sum[5] = {0.f, 0.f, 0.f, 0.f, 0.f};          // sum_u g per component; sum g xhat
#pragma unroll
        for (int p = 0; p < P; ++p) {
            if (ok[p]) {
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    float xv[V], dv[V];
                    Vec16<T>::unpack(xraw[p][c], xv);
                    Vec16<T>::unpack(draw[p][c], dv);
#pragma unroll
                    for (int e = 0; e < V; ++e) {
                        const float t = dv[e] * ((xv[e] - mu[c]) * rstd);          // dy xhat
                        sum[c] = fmaf(dv[e], gm[p][e], sum[c]);
                        sum[4] = fmaf(gm[p][e], t, sum[4]);
                        if (WG) { acc[p][c][e] += dv[e]; acc[p][4][e] += t; }
                    }
                }
            }
        }
        qn_wave_sum<5>(sum);
        // dx = rstd (g - m_c - xhat s) = dy (gamma rstd) - m_c rstd - xhat (s rstd): two multiply-adds per element
        const float sr = sum[4] * inv_4q * rstd;
#pragma unroll
        for (int p = 0; p < P; ++p) {
            if (ok[p]) {
                float gr[V];
#pragma unroll
                for (int e = 0; e < V; ++e) gr[e] = gm[p][e] * rstd;
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    float xv[V], dv[V], o[V];
                    Vec16<T>::unpack(xraw[p][c], xv);
                    Vec16<T>::unpack(draw[p][c], dv);
                    const float mr = sum[c] * inv_q * rstd;
#pragma unroll
                    for (int e = 0; e < V; ++e) o[e] = fmaf(-((xv[e] - mu[c]) * rstd), sr, fmaf(dv[e], gr[e], -mr));
                    store16(dxr + c * Q + (lane + 64 * p) * V, Vec16<T>::pack(o));
                }
            }
        }
    }
    if (WG) {
        // the four waves' partials of every column, summed in wave order; wave 0 writes the slab's line
        float *line = a.part + (size_t)blockIdx.x * 5 * Q;
#pragma unroll
        for (int p = 0; p < P; ++p) {
#pragma unroll
            for (int k = 0; k < 5; ++k) {
                __syncthreads();
                if (wave > 0) {
#pragma unroll
                    for (int e = 0; e < V; ++e) red[wave - 1][e][lane] = acc[p][k][e];
                }
                __syncthreads();
                if (wave == 0 && ok[p]) {
                    float o[V];
#pragma unroll
                    for (int e = 0; e < V; ++e) o[e] = ((acc[p][k][e] + red[0][e][lane]) + red[1][e][lane]) + red[2][e][lane];
#pragma unroll
                    for (int e = 0; e < V; e += 4)
                        *reinterpret_cast<float4 *>(line + k * Q + (lane + 64 * p) * V + e) = make_float4(o[e], o[e + 1], o[e + 2], o[e + 3]);
                }
            }
        }
    }
}

// ---- the slabs' partials -> dbeta, dgamma -----------------------------------------------------------------------------------------
// A workgroup owns 64 columns of the (slabs, 5 Q) partials.  W floats per thread; 1024 / (64 / W) runs of consecutive slabs, each
// summed in slab order by one thread per W columns, then the runs in order: a fixed tree.
template <int W>
__global__ __launch_bounds__(1024) void k_qln_reduce(const float *part, int slabs, int Q, float *dgamma, float *dbeta)
{
    constexpr int TPR = 64 / W, RUNS = 1024 / TPR;
    __shared__ float red[RUNS][64];
    const int cols = 5 * Q;
    const int cg = threadIdx.x % TPR, run = threadIdx.x / TPR;
    const int col = blockIdx.x * 64 + cg * W;
    const int per = (slabs + RUNS - 1) / RUNS;
    const int s0 = min(slabs, run * per), s1 = min(slabs, s0 + per);
    float acc[W];
#pragma unroll
    for (int i = 0; i < W; ++i) acc[i] = 0.f;
    if (col < cols) {
        int s = s0;
        for (; s + 4 <= s1; s += 4) {                       // four independent loads in flight, added in slab order
            float v[4][W];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
#pragma unroll
                for (int i = 0; i < W; ++i) v[k][i] = 0.f;
                const float *src = part + (size_t)(s + k) * cols + col;
                if (W == 4) load4(src, *reinterpret_cast<float (*)[4]>(&v[k][0]));
                else v[k][0] = src[0];
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
#pragma unroll
                for (int i = 0; i < W; ++i) acc[i] += v[k][i];
            }
        }
        for (; s < s1; ++s) {
            const float *src = part + (size_t)s * cols + col;
            if (W == 4) {
                float v[4];
                load4(src, v);
#pragma unroll
                for (int i = 0; i < W; ++i) acc[i] += v[i];
            } else {
                acc[0] += src[0];
            }
        }
    }
#pragma unroll
    for (int i = 0; i < W; ++i) red[run][cg * W + i] = acc[i];
    __syncthreads();
    if (threadIdx.x < 64) {
        const int c = blockIdx.x * 64 + threadIdx.x;
        if (c < cols) {
            float sum = 0.f;
            for (int r = 0; r < RUNS; ++r) sum += red[r][threadIdx.x];
            if (c < 4 * Q) { if (dbeta) dbeta[c] = sum; }
            else if (dgamma) dgamma[c - 4 * Q] = sum;
        }
    }
}

// ---- generic kernels --------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void k_qln_fwd_gen(const QnFwd a)
{
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int Q = a.Q;
    const float inv_q = 1.f / (float)Q, inv_4q = 1.f / (4.f * (float)Q);
    for (int row = blockIdx.x * 4 + wave; row < a.rows; row += gridDim.x * 4) {
        T *yr = (T *)a.y + (size_t)row * a.ys;
        float *st = a.stats + (size_t)row * 5;
        if (!qn_active(a.len, a.steps, row)) {
            for (int j = lane; j < 4 * Q; j += 64) yr[j] = from_f32<T>(0.f);
            if (lane < 5) st[lane] = 0.f;
            continue;
        }
        const T *xr = (const T *)a.x + (size_t)row * a.xs;
        float piv[4], sum[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) { piv[c] = to_f32(xr[c * Q]); sum[c] = 0.f; }
        for (int u = lane; u < Q; u += 64) {
#pragma unroll
            for (int c = 0; c < 4; ++c) sum[c] += to_f32(xr[c * Q + u]) - piv[c];
        }
        qn_wave_sum<4>(sum);
#pragma unroll
        for (int c = 0; c < 4; ++c) sum[c] *= inv_q;
        float sq[1] = {0.f};
        for (int u = lane; u < Q; u += 64) {
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const float d = (to_f32(xr[c * Q + u]) - piv[c]) - sum[c];
                sq[0] += d * d;
            }
        }
        qn_wave_sum<1>(sq);
        const float rstd = 1.f / sqrtf(sq[0] * inv_4q + a.eps);
        for (int u = lane; u < Q; u += 64) {
            const float g = a.gamma ? a.gamma[u] : 1.f;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const float d = (to_f32(xr[c * Q + u]) - piv[c]) - sum[c];
                yr[c * Q + u] = from_f32<T>(g * (d * rstd) + (a.beta ? a.beta[c * Q + u] : 0.f));
            }
        }
        if (lane < 5) {
            float s = rstd;
#pragma unroll
            for (int c = 0; c < 4; ++c) s = lane == c ? piv[c] + sum[c] : s;
            st[lane] = s;
        }
    }
}

template <typename T>
__global__ __launch_bounds__(256) void k_qln_bwd_gen(const QnBwd a)
{
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int Q = a.Q;
    const float inv_q = 1.f / (float)Q, inv_4q = 1.f / (4.f * (float)Q);
    for (int row = blockIdx.x * 4 + wave; row < a.rows; row += gridDim.x * 4) {
        T *dxr = (T *)a.dx + (size_t)row * a.xs;
        if (!qn_active(a.len, a.steps, row)) {
            for (int j = lane; j < 4 * Q; j += 64) dxr[j] = from_f32<T>(0.f);
            continue;
        }
        const T *xr = (const T *)a.x + (size_t)row * a.xs, *dyr = (const T *)a.dy + (size_t)row * a.ys;
        const float *st = a.stats + (size_t)row * 5;
        const float mu[4] = {st[0], st[1], st[2], st[3]}, rstd = st[4];
        float sum[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
        for (int u = lane; u < Q; u += 64) {
            const float gmu = a.gamma ? a.gamma[u] : 1.f;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const float xh = (to_f32(xr[c * Q + u]) - mu[c]) * rstd, g = to_f32(dyr[c * Q + u]) * gmu;
                sum[c] += g;
                sum[4] += g * xh;
            }
        }
        qn_wave_sum<5>(sum);
        const float s = sum[4] * inv_4q;
        for (int u = lane; u < Q; u += 64) {
            const float gmu = a.gamma ? a.gamma[u] : 1.f;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const float xh = (to_f32(xr[c * Q + u]) - mu[c]) * rstd, g = to_f32(dyr[c * Q + u]) * gmu;
                dxr[c * Q + u] = from_f32<T>(rstd * (g - sum[c] * inv_q - xh * s));
            }
        }
    }
}

// the partial of slab blockIdx.y: one thread per unit, the slab's rows in order
template <typename T>
__global__ __launch_bounds__(256) void k_qln_part_gen(const QnBwd a)
{
    const int Q = a.Q;
    const int u = blockIdx.x * 256 + threadIdx.x;
    if (u >= Q) return;
    const int r0 = blockIdx.y * a.slab_rows, r1 = min(a.rows, r0 + a.slab_rows);
    float acc[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
    for (int row = r0; row < r1; ++row) {
        if (!qn_active(a.len, a.steps, row)) continue;
        const T *xr = (const T *)a.x + (size_t)row * a.xs, *dyr = (const T *)a.dy + (size_t)row * a.ys;
        const float *st = a.stats + (size_t)row * 5;
        const float rstd = st[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const float d = to_f32(dyr[c * Q + u]);
            acc[c] += d;
            acc[4] += d * ((to_f32(xr[c * Q + u]) - st[c]) * rstd);
        }
    }
    float *line = a.part + (size_t)blockIdx.y * 5 * Q;
#pragma unroll
    for (int k = 0; k < 5; ++k) line[k * Q + u] = acc[k];
}

// ---- host -------------------------------------------------------------------------------------------------------------------------
bool qn_desc_ok(const qk_qlnorm_desc_t *d, const char *what)
{
    if (!desc_head_ok(d, what)) return false;
    if (d->rows < 1 || d->q < 1) { set_error("%s: rows and q must be >= 1 (got %d, %d)", what, d->rows, d->q); return false; }
    if (d->q > (1 << 26) || d->rows > (1 << 30)) { set_error("%s: shape out of range (rows %d, q %d)", what, d->rows, d->q); return false; }
    if (d->steps < 0 || (d->steps > 0 && d->rows % d->steps != 0)) {
        set_error("%s: steps = %d must be 0 or divide rows = %d", what, d->steps, d->rows);
        return false;
    }
    if (d->x_stride < 4 * d->q || d->y_stride < 4 * d->q) {
        set_error("%s: x_stride %d and y_stride %d must be >= 4 q = %d", what, d->x_stride, d->y_stride, 4 * d->q);
        return false;
    }
    if (d->flags != 0) { set_error("%s: unknown flags 0x%x", what, d->flags); return false; }
    return true;
}

int qn_path(const qk_qlnorm_desc_t *d)
{
    const int v = vec_width(d->dtype);
    return d->q % v == 0 && d->q <= kQnMaxQ && d->x_stride % v == 0 && d->y_stride % v == 0 ? QK_QLNORM_PATH_VEC : QK_QLNORM_PATH_GENERIC;
}

int qn_slab_rows(const qk_qlnorm_desc_t *d)
{
    const int per = (d->rows + kQnSlabTarget - 1) / kQnSlabTarget;
    return (per < kQnSlabMin ? kQnSlabMin : per + 3) / 4 * 4;
}
int qn_slabs(const qk_qlnorm_desc_t *d) { const int sr = qn_slab_rows(d); return (d->rows + sr - 1) / sr; }

int qn_row_grid(int rows, int cap) { const int g = (rows + 3) / 4; return g < cap ? g : cap; }
// register groups per lane of the vector kernels: 1, 2 or 4
int qn_groups(const qk_qlnorm_desc_t *d)
{
    const int need = (d->q + 64 * vec_width(d->dtype) - 1) / (64 * vec_width(d->dtype));
    return need <= 1 ? 1 : need <= 2 ? 2 : 4;
}

template <typename T>
void qn_launch_fwd_vec(int groups, int grid, const QnFwd &a, hipStream_t st)
{
    if (groups == 1) hipLaunchKernelGGL((k_qln_fwd<T, 1>), dim3(grid), dim3(256), 0, st, a);
    else if (groups == 2) hipLaunchKernelGGL((k_qln_fwd<T, 2>), dim3(grid), dim3(256), 0, st, a);
    else if (sizeof(T) == 4) hipLaunchKernelGGL((k_qln_fwd<float, 4>), dim3(grid), dim3(256), 0, st, a);
}

template <typename T, bool WG>
void qn_launch_bwd_vec(int groups, int grid, const QnBwd &a, hipStream_t st)
{
    if (groups == 1) hipLaunchKernelGGL((k_qln_bwd<T, 1, WG>), dim3(grid), dim3(256), 0, st, a);
    else if (groups == 2) hipLaunchKernelGGL((k_qln_bwd<T, 2, WG>), dim3(grid), dim3(256), 0, st, a);
    else if (sizeof(T) == 4) hipLaunchKernelGGL((k_qln_bwd<float, 4, WG>), dim3(grid), dim3(256), 0, st, a);
}

}  // namespace
}  // namespace qk

using namespace qk;

extern "C" {

int qk_qlnorm_supported(const qk_qlnorm_desc_t *desc)
{
    return qn_desc_ok(desc, "qk_qlnorm_supported") ? qn_path(desc) : 0;
}

int qk_qlnorm_slab_rows(const qk_qlnorm_desc_t *desc)
{
    return qn_desc_ok(desc, "qk_qlnorm_slab_rows") ? qn_slab_rows(desc) : 0;
}

size_t qk_qlnorm_workspace_bytes(const qk_qlnorm_desc_t *desc, int32_t op)
{
    if (!qn_desc_ok(desc, "qk_qlnorm_workspace_bytes")) return 0;
    if (op == QK_OP_FWD) return 0;
    if (op == QK_OP_BWD) return (size_t)qn_slabs(desc) * 5 * desc->q * sizeof(float);
    return bad_op("qk_qlnorm_workspace_bytes", op);
}

int qk_qlnorm_fwd(const qk_qlnorm_desc_t *desc, const void *x, const float *gamma, const float *beta, const int32_t *lengths,
                  float epsilon, void *y, float *stats, void *stream)
{
    const char *what = "qk_qlnorm_fwd";
    if (!qn_desc_ok(desc, what)) return QK_ERR_INVALID_ARG;
    if (!x || !y || !stats) { set_error("%s: NULL buffer", what); return QK_ERR_INVALID_ARG; }
    if (lengths && desc->steps == 0) { set_error("%s: lengths given with steps == 0", what); return QK_ERR_INVALID_ARG; }
    if (!(epsilon >= 0.f)) { set_error("%s: epsilon must be >= 0", what); return QK_ERR_INVALID_ARG; }
    const size_t es = elem_size(desc->dtype);
    if (!aligned(x, es) || !aligned(y, es) || !aligned(gamma, 4) || !aligned(beta, 4) || !aligned(stats, 4) || !aligned(lengths, 4)) {
        set_error("%s: misaligned buffer", what);
        return QK_ERR_INVALID_ARG;
    }
    hipStream_t st = (hipStream_t)stream;
    QnFwd a;
    a.rows = desc->rows; a.steps = desc->steps; a.Q = desc->q; a.xs = desc->x_stride; a.ys = desc->y_stride; a.eps = epsilon;
    a.len = lengths; a.x = x; a.gamma = gamma; a.beta = beta; a.y = y; a.stats = stats;
    const bool vec = qn_path(desc) == QK_QLNORM_PATH_VEC && aligned(x, 16) && aligned(y, 16) && aligned(gamma, 16) && aligned(beta, 16);
    if (vec) {
        const int grid = qn_row_grid(desc->rows, 1024), groups = qn_groups(desc);
        by_dtype(desc->dtype, [&](auto t) { qn_launch_fwd_vec<decltype(t)>(groups, grid, a, st); });
    } else {
        const int grid = qn_row_grid(desc->rows, 2048);
        by_dtype(desc->dtype, [&](auto t) { hipLaunchKernelGGL((k_qln_fwd_gen<decltype(t)>), dim3(grid), dim3(256), 0, st, a); });
    }
    return launched(what);
}

int qk_qlnorm_bwd(const qk_qlnorm_desc_t *desc, const void *dy, const void *x, const float *gamma, const int32_t *lengths,
                  const float *stats, void *dx, float *dgamma, float *dbeta, void *workspace, size_t workspace_bytes, void *stream)
{
    const char *what = "qk_qlnorm_bwd";
    if (!qn_desc_ok(desc, what)) return QK_ERR_INVALID_ARG;
    if (!dy || !x || !stats || !dx) { set_error("%s: NULL buffer", what); return QK_ERR_INVALID_ARG; }
    if (lengths && desc->steps == 0) { set_error("%s: lengths given with steps == 0", what); return QK_ERR_INVALID_ARG; }
    const size_t es = elem_size(desc->dtype);
    if (!aligned(x, es) || !aligned(dy, es) || !aligned(dx, es) || !aligned(gamma, 4) || !aligned(stats, 4) || !aligned(lengths, 4)
        || !aligned(dgamma, 4) || !aligned(dbeta, 4) || !aligned(workspace, 16)) {
        set_error("%s: misaligned buffer (16 bytes for the workspace)", what);
        return QK_ERR_INVALID_ARG;
    }
    const bool wg = dgamma || dbeta;
    const size_t need = wg ? qk_qlnorm_workspace_bytes(desc, QK_OP_BWD) : 0;
    if (wg && workspace_ok(what, workspace, workspace_bytes, need) != QK_OK) return QK_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    QnBwd a;
    a.rows = desc->rows; a.steps = desc->steps; a.Q = desc->q; a.xs = desc->x_stride; a.ys = desc->y_stride; a.slab_rows = qn_slab_rows(desc);
    a.len = lengths; a.dy = dy; a.x = x; a.gamma = gamma; a.stats = stats; a.dx = dx; a.part = wg ? (float *)workspace : nullptr;
    const int slabs = qn_slabs(desc);
    const bool vec = qn_path(desc) == QK_QLNORM_PATH_VEC && aligned(x, 16) && aligned(dy, 16) && aligned(dx, 16) && aligned(gamma, 16);
    if (vec) {
        const int groups = qn_groups(desc);
        by_dtype(desc->dtype, [&](auto t) {
            if (wg) qn_launch_bwd_vec<decltype(t), true>(groups, slabs, a, st);
            else qn_launch_bwd_vec<decltype(t), false>(groups, slabs, a, st);
        });
    } else {
        const int grid = qn_row_grid(desc->rows, 2048);
        const dim3 pgrid((unsigned)((desc->q + 255) / 256), (unsigned)slabs);
        by_dtype(desc->dtype, [&](auto t) {
            hipLaunchKernelGGL((k_qln_bwd_gen<decltype(t)>), dim3(grid), dim3(256), 0, st, a);
            if (wg) hipLaunchKernelGGL((k_qln_part_gen<decltype(t)>), pgrid, dim3(256), 0, st, a);
        });
    }
    if (wg) {
        const int blocks = (5 * desc->q + 63) / 64;
        if (desc->q % 4 == 0) hipLaunchKernelGGL((k_qln_reduce<4>), dim3(blocks), dim3(1024), 0, st, (const float *)workspace, slabs, desc->q, dgamma, dbeta);
        else hipLaunchKernelGGL((k_qln_reduce<1>), dim3(blocks), dim3(1024), 0, st, (const float *)workspace, slabs, desc->q, dgamma, dbeta);
    }
    return launched(what);
}

}  // extern "C"
