// Quaternion multi-head self-attention (include/qk_attn.h): softmax(scale * q k^T) v per (batch row, head) over component-major
// tensors, forward and backward, fused: the (T, T) scores never reach memory.
//
// Matrix kernels (QK_QATTN_PATH_MFMA; bf16 / fp16, dq 16 or 32).  All three have one shape.  A workgroup of four waves owns 64 rows
// of the LANE side (forward and k_qattn_bwd_q: queries; k_qattn_bwd_kv: keys), a wave 16 of them, and sweeps the OTHER side in tiles
// staged through LDS.  Every product is a v_mfma_f32_16x16x32 whose B operand carries the lane side on its column (= lane & 15) and
// whose accumulator rows (4 (lane >> 4) + register) are the swept side or the head dimension d:
//     S^T[swept, lane side]   = X_rm[swept, d] . Y[d, lane side]       X_rm: a row-major LDS image, Y: fragments held in registers
//     R^T[d, lane side]      += X_tr[d, swept] . W[swept, lane side]   X_tr: a transposed LDS image, W: the accumulator of S^T,
// packed to 16 bits IN PLACE (an accumulator tile as the next MFMA's B operand: two 16-row tiles a, b give the eight k-slots
// j < 4: row 4 g + j of a, j >= 4: row 4 g + j - 4 of b, and the transposed image is read in that same order).  The softmax
// reductions run over a lane's registers and the four lane groups (two shuffles); nothing else crosses lanes.
// Rows at or past lengths[b] are staged as ZEROS whatever memory holds and their probabilities are forced to 0, so padding may be
// NaN; the sweep stops at lengths[b], so no tile is wholly masked and the running maximum is finite from the first tile on.
//
// Generic kernels (QK_QATTN_PATH_GENERIC): any dtype, dq, stride and alignment.  One wave per (b, h, row), lanes over the head
// dimension, the other side one row at a time, every dot product a wave butterfly; fp32 throughout (the 16-bit types round p and
// dS at the header's rounding points).  Correct before fast.
#include "qk_common.h"
#include "qk_seq.h"
#include "../../include/qk_attn.h"

#include <math.h>

namespace qk {
namespace {

constexpr float kQaLog2e = 1.4426950408889634f;
constexpr float kQaLn2 = 0.6931471805599453f;

typedef unsigned short qa_u16;

__device__ __forceinline__ unsigned qa_bits(bf16 v) { return v.x; }
__device__ __forceinline__ unsigned qa_bits(f16 v) { return __builtin_bit_cast(qa_u16, v); }
template <typename T>
__device__ __forceinline__ unsigned qa_pack2(float lo, float hi) { return qa_bits(from_f32<T>(lo)) | (qa_bits(from_f32<T>(hi)) << 16); }
// two accumulator tiles (swept rows 4 g + r of a 16-row tile each) as one B operand: k-slot j < 4 from a, j >= 4 from b
template <typename T>
__device__ __forceinline__ uint4 qa_pack_acc(const floatx4 &a, const floatx4 &b)
{
    return make_uint4(qa_pack2<T>(a[0], a[1]), qa_pack2<T>(a[2], a[3]), qa_pack2<T>(b[0], b[1]), qa_pack2<T>(b[2], b[3]));
}

struct QaArgs {
    int B, T, H, dq;
    int q_row, q_comp, k_row, k_comp, v_row, v_comp, o_row, o_comp;
    float scale;
    const int *len;
    const void *q, *k, *v, *o, *d_o;
    void *out_o, *d_q, *d_k, *d_v;
    float *lse_out;
    const float *lse;
    float *delta;
};

__device__ __forceinline__ int qa_len(const QaArgs &a, int b)
{
    if (!a.len) return a.T;
    const int n = a.len[b];
    return n < 0 ? 0 : n > a.T ? a.T : n;
}

// ---- matrix kernels: staging and fragments ------------------------------------------------------------------------------------------
// Rows t0 .. t0 + TS - 1 of one head (base points at row 0 of the batch row, unit 0 of the head in component 0) into a row-major image
// [TS][D + 8] and / or a transposed image [D][TS + 8]; rows from n on are zeros.
template <int DQ, int TS, bool RM, bool TR>
__device__ __forceinline__ void qa_stage(const qa_u16 *base, int row, int comp, int t0, int n, qa_u16 *rm, qa_u16 *tr)
{
    constexpr int D = 4 * DQ, C8 = D / 8;
    for (int idx = threadIdx.x; idx < TS * C8; idx += 256) {
        const int r = idx / C8, d = (idx % C8) * 8;
        const int t = t0 + r;
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (t < n) v = *reinterpret_cast<const uint4 *>(base + (size_t)t * row + (size_t)(d / DQ) * comp + (d % DQ));
        if (RM) *reinterpret_cast<uint4 *>(rm + r * (D + 8) + d) = v;
        if (TR) {
            const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                tr[(d + 2 * i) * (TS + 8) + r] = (qa_u16)(w[i] & 0xffffu);
                tr[(d + 2 * i + 1) * (TS + 8) + r] = (qa_u16)(w[i] >> 16);
            }
        }
    }
}

// the lane side's B-operand fragments of row t (zeros when t >= n): element j of k-step ks is d = 32 ks + 8 g + j
template <int DQ>
__device__ __forceinline__ void qa_lane_frags(const qa_u16 *base, int row, int comp, int t, int n, int g, uint4 (&f)[DQ / 8])
{
#pragma unroll
    for (int ks = 0; ks < DQ / 8; ++ks) {
        const int d = 32 * ks + 8 * g;
        f[ks] = make_uint4(0u, 0u, 0u, 0u);
        if (t < n) f[ks] = *reinterpret_cast<const uint4 *>(base + (size_t)t * row + (size_t)(d / DQ) * comp + (d % DQ));
    }
}

template <int D>
__device__ __forceinline__ uint4 qa_frag_rm(const qa_u16 *rm, int r, int d) { return *reinterpret_cast<const uint4 *>(rm + r * (D + 8) + d); }
// k-slots of one 32-row group of the swept side in the order of qa_pack_acc
template <int TS>
__device__ __forceinline__ uint4 qa_frag_tr(const qa_u16 *tr, int d, int r32, int g)
{
    const uint2 lo = *reinterpret_cast<const uint2 *>(tr + d * (TS + 8) + r32 + 4 * g);
    const uint2 hi = *reinterpret_cast<const uint2 *>(tr + d * (TS + 8) + r32 + 16 + 4 * g);
    return make_uint4(lo.x, lo.y, hi.x, hi.y);
}

// R^T[d = 16 dt + 4 g + r][row t] of the lane side, written as 8 bytes per tile; zeros when the row is inactive
template <typename T, int DQ>
__device__ __forceinline__ void qa_store_rows(qa_u16 *base, int row, int comp, int t, bool active, int g, const floatx4 (&acc)[DQ / 4], float mul)
{
#pragma unroll
    for (int dt = 0; dt < DQ / 4; ++dt) {
        const int d = 16 * dt + 4 * g;
        uint2 w = make_uint2(0u, 0u);
        if (active) w = make_uint2(qa_pack2<T>(acc[dt][0] * mul, acc[dt][1] * mul), qa_pack2<T>(acc[dt][2] * mul, acc[dt][3] * mul));
        *reinterpret_cast<uint2 *>(base + (size_t)t * row + (size_t)(d / DQ) * comp + (d % DQ)) = w;
    }
}

// ---- forward ------------------------------------------------------------------------------------------------------------------------
template <typename T, int DQ>
__global__ __launch_bounds__(256) void k_qattn_fwd(const QaArgs a)
{
    constexpr int D = 4 * DQ, TS = 64, KS = D / 32, DT = D / 16;
    __shared__ __align__(16) qa_u16 k_rm[TS * (D + 8)];
    __shared__ __align__(16) qa_u16 v_tr[D * (TS + 8)];
    const int tiles = (a.T + 63) / 64;
    const int b = blockIdx.x / tiles, q0 = (blockIdx.x % tiles) * 64, h = blockIdx.y;
    const int n = qa_len(a, b);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4, c16 = lane & 15;
    const int tq = q0 + wave * 16 + c16;
    const size_t head = (size_t)h * DQ;
    const qa_u16 *qb = (const qa_u16 *)a.q + (size_t)b * a.T * a.q_row + head;
    const qa_u16 *kb = (const qa_u16 *)a.k + (size_t)b * a.T * a.k_row + head;
    const qa_u16 *vb = (const qa_u16 *)a.v + (size_t)b * a.T * a.v_row + head;
    const float sc2 = a.scale * kQaLog2e;

    uint4 qf[KS];
    qa_lane_frags<DQ>(qb, a.q_row, a.q_comp, tq, n, g, qf);
    floatx4 o[DT];
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) o[dt] = floatx4{0.f, 0.f, 0.f, 0.f};
    float m = -INFINITY, l = 0.f;                       // l: this lane's share of the row sum; the four groups meet at the end

    const int kend = q0 < n ? n : 0;                    // a tile at or past lengths[b] only writes zeros
    for (int kt = 0; kt < kend; kt += TS) {
        __syncthreads();
        qa_stage<DQ, TS, true, false>(kb, a.k_row, a.k_comp, kt, n, k_rm, nullptr);
        qa_stage<DQ, TS, false, true>(vb, a.v_row, a.v_comp, kt, n, nullptr, v_tr);
        __syncthreads();
        floatx4 s[4];
#pragma unroll
        for (int sub = 0; sub < 4; ++sub) {
            s[sub] = floatx4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) s[sub] = mfma16(T(), qa_frag_rm<D>(k_rm, 16 * sub + c16, 32 * ks + 8 * g), qf[ks], s[sub]);
        }
        float mx = -INFINITY;
#pragma unroll
        for (int sub = 0; sub < 4; ++sub) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const bool live = kt + 16 * sub + 4 * g + r < n;
                s[sub][r] = live ? s[sub][r] * sc2 : -INFINITY;
                mx = fmaxf(mx, s[sub][r]);
            }
        }
        mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        const float m_new = fmaxf(m, mx);               // finite: key kt < n is in this tile
        const float alpha = exp2f(m - m_new);           // first tile: exp2(-inf) = 0
        m = m_new;
        float sum = 0.f;
#pragma unroll
        for (int sub = 0; sub < 4; ++sub) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                s[sub][r] = exp2f(s[sub][r] - m_new);   // masked keys: exp2(-inf) = 0
                sum += s[sub][r];
            }
        }
        l = l * alpha + sum;
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) o[dt] *= alpha;
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            const uint4 pf = qa_pack_acc<T>(s[2 * kk], s[2 * kk + 1]);
#pragma unroll
            for (int dt = 0; dt < DT; ++dt) o[dt] = mfma16(T(), qa_frag_tr<TS>(v_tr, 16 * dt + c16, 32 * kk, g), pf, o[dt]);
        }
    }
    l += __shfl_xor(l, 16, 64);
    l += __shfl_xor(l, 32, 64);
    if (tq < a.T) {
        const bool active = tq < n;
        qa_store_rows<T, DQ>((qa_u16 *)a.out_o + (size_t)b * a.T * a.o_row + head, a.o_row, a.o_comp, tq, active, g, o, active ? 1.f / l : 0.f);
        if (g == 0) a.lse_out[((size_t)b * a.H + h) * a.T + tq] = active ? (m + log2f(l)) * kQaLn2 : 0.f;
    }
}

// ---- backward: dq (a workgroup owns 64 queries and sweeps the keys) -------------------------------------------------------------------
template <typename T, int DQ>
__global__ __launch_bounds__(256) void k_qattn_bwd_q(const QaArgs a)
{
    constexpr int D = 4 * DQ, TS = 32, KS = D / 32, DT = D / 16;
    __shared__ __align__(16) qa_u16 k_rm[TS * (D + 8)];
    __shared__ __align__(16) qa_u16 v_rm[TS * (D + 8)];
    __shared__ __align__(16) qa_u16 k_tr[D * (TS + 8)];
    const int tiles = (a.T + 63) / 64;
    const int b = blockIdx.x / tiles, q0 = (blockIdx.x % tiles) * 64, h = blockIdx.y;
    const int n = qa_len(a, b);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4, c16 = lane & 15;
    const int tq = q0 + wave * 16 + c16;
    const size_t head = (size_t)h * DQ;
    const qa_u16 *qb = (const qa_u16 *)a.q + (size_t)b * a.T * a.q_row + head;
    const qa_u16 *kb = (const qa_u16 *)a.k + (size_t)b * a.T * a.k_row + head;
    const qa_u16 *vb = (const qa_u16 *)a.v + (size_t)b * a.T * a.v_row + head;
    const qa_u16 *gb = (const qa_u16 *)a.d_o + (size_t)b * a.T * a.o_row + head;
    const float sc2 = a.scale * kQaLog2e;

    uint4 qf[KS], gf[KS];
    qa_lane_frags<DQ>(qb, a.q_row, a.q_comp, tq, n, g, qf);
    qa_lane_frags<DQ>(gb, a.o_row, a.o_comp, tq, n, g, gf);
    const bool active = tq < n;
    const size_t stat = ((size_t)b * a.H + h) * a.T;
    const float lse2 = active ? a.lse[stat + tq] * kQaLog2e : 0.f;
    const float dl = active ? a.delta[stat + tq] : 0.f;
    floatx4 acc[DT];
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) acc[dt] = floatx4{0.f, 0.f, 0.f, 0.f};

    const int kend = q0 < n ? n : 0;
    for (int kt = 0; kt < kend; kt += TS) {
        __syncthreads();
        qa_stage<DQ, TS, true, true>(kb, a.k_row, a.k_comp, kt, n, k_rm, k_tr);
        qa_stage<DQ, TS, true, false>(vb, a.v_row, a.v_comp, kt, n, v_rm, nullptr);
        __syncthreads();
        floatx4 ds[2];
#pragma unroll
        for (int sub = 0; sub < 2; ++sub) {
            floatx4 s = floatx4{0.f, 0.f, 0.f, 0.f}, dp = floatx4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                s = mfma16(T(), qa_frag_rm<D>(k_rm, 16 * sub + c16, 32 * ks + 8 * g), qf[ks], s);
                dp = mfma16(T(), qa_frag_rm<D>(v_rm, 16 * sub + c16, 32 * ks + 8 * g), gf[ks], dp);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const bool live = active && kt + 16 * sub + 4 * g + r < n;
                const float p = live ? exp2f(s[r] * sc2 - lse2) : 0.f;
                ds[sub][r] = p * (dp[r] - dl) * a.scale;
            }
        }
        const uint4 df = qa_pack_acc<T>(ds[0], ds[1]);
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) acc[dt] = mfma16(T(), qa_frag_tr<TS>(k_tr, 16 * dt + c16, 0, g), df, acc[dt]);
    }
    if (tq < a.T)
        qa_store_rows<T, DQ>((qa_u16 *)a.d_q + (size_t)b * a.T * a.q_row + head, a.q_row, a.q_comp, tq, active, g, acc, 1.f);
}

// ---- backward: dk, dv (a workgroup owns 64 keys and sweeps the queries) ---------------------------------------------------------------
template <typename T, int DQ>
__global__ __launch_bounds__(256) void k_qattn_bwd_kv(const QaArgs a)
{
    constexpr int D = 4 * DQ, TS = 32, KS = D / 32, DT = D / 16;
    __shared__ __align__(16) qa_u16 q_rm[TS * (D + 8)];
    __shared__ __align__(16) qa_u16 g_rm[TS * (D + 8)];
    __shared__ __align__(16) qa_u16 q_tr[D * (TS + 8)];
    __shared__ __align__(16) qa_u16 g_tr[D * (TS + 8)];
    __shared__ float lse_s[TS], dl_s[TS];
    const int tiles = (a.T + 63) / 64;
    const int b = blockIdx.x / tiles, k0 = (blockIdx.x % tiles) * 64, h = blockIdx.y;
    const int n = qa_len(a, b);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4, c16 = lane & 15;
    const int tk = k0 + wave * 16 + c16;
    const size_t head = (size_t)h * DQ;
    const qa_u16 *qb = (const qa_u16 *)a.q + (size_t)b * a.T * a.q_row + head;
    const qa_u16 *kb = (const qa_u16 *)a.k + (size_t)b * a.T * a.k_row + head;
    const qa_u16 *vb = (const qa_u16 *)a.v + (size_t)b * a.T * a.v_row + head;
    const qa_u16 *gb = (const qa_u16 *)a.d_o + (size_t)b * a.T * a.o_row + head;
    const float sc2 = a.scale * kQaLog2e;
    const size_t stat = ((size_t)b * a.H + h) * a.T;

    uint4 kf[KS], vf[KS];
    qa_lane_frags<DQ>(kb, a.k_row, a.k_comp, tk, n, g, kf);
    qa_lane_frags<DQ>(vb, a.v_row, a.v_comp, tk, n, g, vf);
    const bool active = tk < n;
    floatx4 dk[DT], dv[DT];
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) { dk[dt] = floatx4{0.f, 0.f, 0.f, 0.f}; dv[dt] = floatx4{0.f, 0.f, 0.f, 0.f}; }

    const int qend = k0 < n ? n : 0;
    for (int qt = 0; qt < qend; qt += TS) {
        __syncthreads();
        qa_stage<DQ, TS, true, true>(qb, a.q_row, a.q_comp, qt, n, q_rm, q_tr);
        qa_stage<DQ, TS, true, true>(gb, a.o_row, a.o_comp, qt, n, g_rm, g_tr);
        if (threadIdx.x < TS) {
            const int t = qt + threadIdx.x;
            lse_s[threadIdx.x] = t < n ? a.lse[stat + t] * kQaLog2e : 0.f;
            dl_s[threadIdx.x] = t < n ? a.delta[stat + t] : 0.f;
        }
        __syncthreads();
        floatx4 p[2], ds[2];
#pragma unroll
        for (int sub = 0; sub < 2; ++sub) {
            floatx4 s = floatx4{0.f, 0.f, 0.f, 0.f}, dp = floatx4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                s = mfma16(T(), qa_frag_rm<D>(q_rm, 16 * sub + c16, 32 * ks + 8 * g), kf[ks], s);
                dp = mfma16(T(), qa_frag_rm<D>(g_rm, 16 * sub + c16, 32 * ks + 8 * g), vf[ks], dp);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int qi = 16 * sub + 4 * g + r;
                const bool live = active && qt + qi < n;
                p[sub][r] = live ? exp2f(s[r] * sc2 - lse_s[qi]) : 0.f;
                ds[sub][r] = p[sub][r] * (dp[r] - dl_s[qi]) * a.scale;
            }
        }
        const uint4 pf = qa_pack_acc<T>(p[0], p[1]), df = qa_pack_acc<T>(ds[0], ds[1]);
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) {
            dv[dt] = mfma16(T(), qa_frag_tr<TS>(g_tr, 16 * dt + c16, 0, g), pf, dv[dt]);
            dk[dt] = mfma16(T(), qa_frag_tr<TS>(q_tr, 16 * dt + c16, 0, g), df, dk[dt]);
        }
    }
    if (tk < a.T) {
        qa_store_rows<T, DQ>((qa_u16 *)a.d_k + (size_t)b * a.T * a.k_row + head, a.k_row, a.k_comp, tk, active, g, dk, 1.f);
        qa_store_rows<T, DQ>((qa_u16 *)a.d_v + (size_t)b * a.T * a.v_row + head, a.v_row, a.v_comp, tk, active, g, dv, 1.f);
    }
}

// ---- delta[b, h, t] = sum_d do * o: a thread per (b, t, h), h fastest so neighbours read neighbouring runs ----------------------------
// the two halves of a 32-bit word of 16-bit activations
__device__ __forceinline__ float qa_half(bf16, unsigned w, bool high) { return __uint_as_float(high ? w & 0xffff0000u : w << 16); }
__device__ __forceinline__ float qa_half(f16, unsigned w, bool high) { return (float)__builtin_bit_cast(f16, (qa_u16)(high ? w >> 16 : w & 0xffffu)); }

// DQ = 16 / 32 (the matrix path: 16-bit T, every run 16-byte aligned): 16-byte loads; DQ = 0: any dtype, width and alignment
template <typename T, int DQ>
__global__ __launch_bounds__(256) void k_qattn_delta(const QaArgs a)
{
    const long long total = (long long)a.B * a.T * a.H;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int h = (int)(i % a.H);
        const long long bt = i / a.H;
        const int t = (int)(bt % a.T), b = (int)(bt / a.T);
        float sum = 0.f;
        if (t < qa_len(a, b)) {
            const T *orow = (const T *)a.o + (size_t)bt * a.o_row + (size_t)h * a.dq;
            const T *grow = (const T *)a.d_o + (size_t)bt * a.o_row + (size_t)h * a.dq;
            if constexpr (DQ > 0) {
#pragma unroll
                for (int c = 0; c < 4; ++c) {
#pragma unroll
                    for (int u = 0; u < DQ; u += 8) {
                        const uint4 gv = *reinterpret_cast<const uint4 *>(grow + (size_t)c * a.o_comp + u);
                        const uint4 ov = *reinterpret_cast<const uint4 *>(orow + (size_t)c * a.o_comp + u);
                        const unsigned gw[4] = {gv.x, gv.y, gv.z, gv.w}, ow[4] = {ov.x, ov.y, ov.z, ov.w};
#pragma unroll
                        for (int k = 0; k < 4; ++k)
                            sum += qa_half(T(), gw[k], false) * qa_half(T(), ow[k], false) + qa_half(T(), gw[k], true) * qa_half(T(), ow[k], true);
                    }
                }
            } else {
                for (int c = 0; c < 4; ++c)
                    for (int u = 0; u < a.dq; ++u) sum += to_f32(grow[(size_t)c * a.o_comp + u]) * to_f32(orow[(size_t)c * a.o_comp + u]);
            }
        }
        a.delta[((size_t)b * a.H + h) * a.T + t] = sum;
    }
}

// ---- generic kernels ----------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float qa_wave_sum(float v)
{
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) v += __shfl_xor(v, off, 64);
    return v;
}
// column of head-dimension index d inside a row: component d / dq, unit d % dq
__device__ __forceinline__ size_t qa_col(int d, int dq, int comp) { return (size_t)(d / dq) * comp + (d % dq); }

template <typename T>
__device__ __forceinline__ float qa_dot(const T *x, int xc, const T *y, int yc, int dq, int lane)
{
    float s = 0.f;
    for (int d = lane; d < 4 * dq; d += 64) s += to_f32(x[qa_col(d, dq, xc)]) * to_f32(y[qa_col(d, dq, yc)]);
    return qa_wave_sum(s);
}

// which (b, h, t) a wave serves: t fastest
__device__ __forceinline__ void qa_split(const QaArgs &a, long long w, int &b, int &h, int &t)
{
    t = (int)(w % a.T);
    h = (int)((w / a.T) % a.H);
    b = (int)(w / ((long long)a.T * a.H));
}

template <typename T>
__global__ __launch_bounds__(256) void k_qattn_fwd_gen(const QaArgs a)
{
    const int lane = threadIdx.x & 63;
    const long long total = (long long)a.B * a.H * a.T;
    const int D = 4 * a.dq;
    for (long long w = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); w < total; w += (long long)gridDim.x * 4) {
        int b, h, t;
        qa_split(a, w, b, h, t);
        const int n = qa_len(a, b);
        const size_t head = (size_t)h * a.dq;
        T *orow = (T *)a.out_o + ((size_t)b * a.T + t) * a.o_row + head;
        float *lse = a.lse_out + ((size_t)b * a.H + h) * a.T + t;
        if (t >= n) {
            for (int d = lane; d < D; d += 64) orow[qa_col(d, a.dq, a.o_comp)] = from_f32<T>(0.f);
            if (lane == 0) *lse = 0.f;
            continue;
        }
        const T *qrow = (const T *)a.q + ((size_t)b * a.T + t) * a.q_row + head;
        const T *kb = (const T *)a.k + (size_t)b * a.T * a.k_row + head;
        const T *vb = (const T *)a.v + (size_t)b * a.T * a.v_row + head;
        float m = -INFINITY;
        for (int j = 0; j < n; ++j) m = fmaxf(m, a.scale * qa_dot(qrow, a.q_comp, kb + (size_t)j * a.k_row, a.k_comp, a.dq, lane));
        float l = 0.f;
        for (int j = 0; j < n; ++j) l += expf(a.scale * qa_dot(qrow, a.q_comp, kb + (size_t)j * a.k_row, a.k_comp, a.dq, lane) - m);
        const float ls = m + logf(l);
        if (lane == 0) *lse = ls;
        for (int d0 = 0; d0 < D; d0 += 64) {
            const int d = d0 + lane;
            float acc = 0.f;
            for (int j = 0; j < n; ++j) {
                const float p = round_to<T>(expf(a.scale * qa_dot(qrow, a.q_comp, kb + (size_t)j * a.k_row, a.k_comp, a.dq, lane) - ls));
                if (d < D) acc += p * to_f32(vb[(size_t)j * a.v_row + qa_col(d, a.dq, a.v_comp)]);
            }
            if (d < D) orow[qa_col(d, a.dq, a.o_comp)] = from_f32<T>(acc);
        }
    }
}

template <typename T>
__global__ __launch_bounds__(256) void k_qattn_bwd_q_gen(const QaArgs a)
{
    const int lane = threadIdx.x & 63;
    const long long total = (long long)a.B * a.H * a.T;
    const int D = 4 * a.dq;
    for (long long w = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); w < total; w += (long long)gridDim.x * 4) {
        int b, h, t;
        qa_split(a, w, b, h, t);
        const int n = qa_len(a, b);
        const size_t head = (size_t)h * a.dq;
        T *dqrow = (T *)a.d_q + ((size_t)b * a.T + t) * a.q_row + head;
        if (t >= n) {
            for (int d = lane; d < D; d += 64) dqrow[qa_col(d, a.dq, a.q_comp)] = from_f32<T>(0.f);
            continue;
        }
        const T *qrow = (const T *)a.q + ((size_t)b * a.T + t) * a.q_row + head;
        const T *grow = (const T *)a.d_o + ((size_t)b * a.T + t) * a.o_row + head;
        const T *kb = (const T *)a.k + (size_t)b * a.T * a.k_row + head;
        const T *vb = (const T *)a.v + (size_t)b * a.T * a.v_row + head;
        const size_t stat = ((size_t)b * a.H + h) * a.T + t;
        const float ls = a.lse[stat], dl = a.delta[stat];
        for (int d0 = 0; d0 < D; d0 += 64) {
            const int d = d0 + lane;
            float acc = 0.f;
            for (int j = 0; j < n; ++j) {
                const T *krow = kb + (size_t)j * a.k_row;
                const float p = expf(a.scale * qa_dot(qrow, a.q_comp, krow, a.k_comp, a.dq, lane) - ls);
                const float dp = qa_dot(grow, a.o_comp, vb + (size_t)j * a.v_row, a.v_comp, a.dq, lane);
                const float ds = round_to<T>(p * (dp - dl) * a.scale);
                if (d < D) acc += ds * to_f32(krow[qa_col(d, a.dq, a.k_comp)]);
            }
            if (d < D) dqrow[qa_col(d, a.dq, a.q_comp)] = from_f32<T>(acc);
        }
    }
}

template <typename T>
__global__ __launch_bounds__(256) void k_qattn_bwd_kv_gen(const QaArgs a)
{
    const int lane = threadIdx.x & 63;
    const long long total = (long long)a.B * a.H * a.T;
    const int D = 4 * a.dq;
    for (long long w = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); w < total; w += (long long)gridDim.x * 4) {
        int b, h, t;
        qa_split(a, w, b, h, t);
        const int n = qa_len(a, b);
        const size_t head = (size_t)h * a.dq;
        T *dkrow = (T *)a.d_k + ((size_t)b * a.T + t) * a.k_row + head;
        T *dvrow = (T *)a.d_v + ((size_t)b * a.T + t) * a.v_row + head;
        if (t >= n) {
            for (int d = lane; d < D; d += 64) {
                dkrow[qa_col(d, a.dq, a.k_comp)] = from_f32<T>(0.f);
                dvrow[qa_col(d, a.dq, a.v_comp)] = from_f32<T>(0.f);
            }
            continue;
        }
        const T *krow = (const T *)a.k + ((size_t)b * a.T + t) * a.k_row + head;
        const T *vrow = (const T *)a.v + ((size_t)b * a.T + t) * a.v_row + head;
        const T *qb = (const T *)a.q + (size_t)b * a.T * a.q_row + head;
        const T *gb = (const T *)a.d_o + (size_t)b * a.T * a.o_row + head;
        const size_t stat = ((size_t)b * a.H + h) * a.T;
        for (int d0 = 0; d0 < D; d0 += 64) {
            const int d = d0 + lane;
            float ak = 0.f, av = 0.f;
            for (int i = 0; i < n; ++i) {
                const T *qrow = qb + (size_t)i * a.q_row, *grow = gb + (size_t)i * a.o_row;
                const float p = expf(a.scale * qa_dot(qrow, a.q_comp, krow, a.k_comp, a.dq, lane) - a.lse[stat + i]);
                const float dp = qa_dot(grow, a.o_comp, vrow, a.v_comp, a.dq, lane);
                const float ds = round_to<T>(p * (dp - a.delta[stat + i]) * a.scale);
                if (d < D) {
                    av += round_to<T>(p) * to_f32(grow[qa_col(d, a.dq, a.o_comp)]);
                    ak += ds * to_f32(qrow[qa_col(d, a.dq, a.q_comp)]);
                }
            }
            if (d < D) {
                dkrow[qa_col(d, a.dq, a.k_comp)] = from_f32<T>(ak);
                dvrow[qa_col(d, a.dq, a.v_comp)] = from_f32<T>(av);
            }
        }
    }
}

// ---- host -------------------------------------------------------------------------------------------------------------------------
bool qa_stride_ok(const char *what, const char *name, int row, int comp, int units)
{
    if (comp < units || (long long)row < 3ll * comp + units || row > (1 << 30)) {
        set_error("%s: %s_comp = %d must be >= heads * dq = %d and %s_row = %d >= 3 comp + heads * dq (and <= 2^30)", what, name, comp, units, name, row);
        return false;
    }
    return true;
}

bool qa_desc_ok(const qk_qattn_desc_t *d, const char *what)
{
    if (!desc_head_ok(d, what)) return false;
    if (d->batch < 1 || d->steps < 1 || d->heads < 1 || d->dq < 1) {
        set_error("%s: batch, steps, heads and dq must be >= 1 (got %d, %d, %d, %d)", what, d->batch, d->steps, d->heads, d->dq);
        return false;
    }
    if (d->heads > 65535 || (long long)d->heads * d->dq > (1 << 24) || (long long)d->batch * d->steps * d->heads > (1ll << 30)) {
        set_error("%s: shape out of range (batch %d, steps %d, heads %d, dq %d)", what, d->batch, d->steps, d->heads, d->dq);
        return false;
    }
    const int units = d->heads * d->dq;
    if (!qa_stride_ok(what, "q", d->q_row, d->q_comp, units) || !qa_stride_ok(what, "k", d->k_row, d->k_comp, units)
        || !qa_stride_ok(what, "v", d->v_row, d->v_comp, units) || !qa_stride_ok(what, "o", d->o_row, d->o_comp, units))
        return false;
    if (d->flags != 0) { set_error("%s: unknown flags 0x%x", what, d->flags); return false; }
    return true;
}

int qa_path(const qk_qattn_desc_t *d)
{
    if (d->dtype == QK_F32 || (d->dq != 16 && d->dq != 32)) return QK_QATTN_PATH_GENERIC;
    const int s[8] = {d->q_row, d->q_comp, d->k_row, d->k_comp, d->v_row, d->v_comp, d->o_row, d->o_comp};
    for (int i = 0; i < 8; ++i)
        if (s[i] % 8 != 0) return QK_QATTN_PATH_GENERIC;
    return QK_QATTN_PATH_MFMA;
}

QaArgs qa_args(const qk_qattn_desc_t *d, float scale, const int32_t *lengths)
{
    QaArgs a = {};
    a.B = d->batch; a.T = d->steps; a.H = d->heads; a.dq = d->dq;
    a.q_row = d->q_row; a.q_comp = d->q_comp; a.k_row = d->k_row; a.k_comp = d->k_comp;
    a.v_row = d->v_row; a.v_comp = d->v_comp; a.o_row = d->o_row; a.o_comp = d->o_comp;
    a.scale = scale > 0.f ? scale : 1.f / sqrtf(4.f * (float)d->dq);
    a.len = lengths;
    return a;
}

size_t qa_delta_bytes(const qk_qattn_desc_t *d) { return align256((size_t)d->batch * d->heads * d->steps * sizeof(float)); }
int qa_wave_grid(const qk_qattn_desc_t *d)
{
    const long long blocks = ((long long)d->batch * d->heads * d->steps + 3) / 4;
    return (int)(blocks < (1 << 20) ? blocks : (1 << 20));
}

template <typename T>
void qa_launch_fwd_gen(const qk_qattn_desc_t *d, const QaArgs &a, hipStream_t st)
{
    hipLaunchKernelGGL((k_qattn_fwd_gen<T>), dim3(qa_wave_grid(d)), dim3(256), 0, st, a);
}
template <typename T>
void qa_launch_fwd_mfma(const qk_qattn_desc_t *d, const QaArgs &a, hipStream_t st)
{
    const dim3 grid((unsigned)(d->batch * ((d->steps + 63) / 64)), (unsigned)d->heads);
    if (d->dq == 16) hipLaunchKernelGGL((k_qattn_fwd<T, 16>), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((k_qattn_fwd<T, 32>), grid, dim3(256), 0, st, a);
}
template <typename T>
void qa_launch_bwd_mfma(const qk_qattn_desc_t *d, const QaArgs &a, hipStream_t st)
{
    const dim3 grid((unsigned)(d->batch * ((d->steps + 63) / 64)), (unsigned)d->heads);
    if (d->dq == 16) {
        hipLaunchKernelGGL((k_qattn_bwd_kv<T, 16>), grid, dim3(256), 0, st, a);
        hipLaunchKernelGGL((k_qattn_bwd_q<T, 16>), grid, dim3(256), 0, st, a);
    } else {
        hipLaunchKernelGGL((k_qattn_bwd_kv<T, 32>), grid, dim3(256), 0, st, a);
        hipLaunchKernelGGL((k_qattn_bwd_q<T, 32>), grid, dim3(256), 0, st, a);
    }
}
// delta first, then (generic path) the two plain kernels; the matrix kernels follow from qa_launch_bwd_mfma
template <typename T>
void qa_launch_bwd(const qk_qattn_desc_t *d, bool mfma, const QaArgs &a, hipStream_t st)
{
    const long long threads = (long long)d->batch * d->heads * d->steps;
    const long long dblocks = (threads + 255) / 256;
    const dim3 dgrid((unsigned)(dblocks < (1 << 20) ? dblocks : (1 << 20)));
    if constexpr (sizeof(T) == 2) {
        if (mfma && d->dq == 16) hipLaunchKernelGGL((k_qattn_delta<T, 16>), dgrid, dim3(256), 0, st, a);
        else if (mfma) hipLaunchKernelGGL((k_qattn_delta<T, 32>), dgrid, dim3(256), 0, st, a);
        else hipLaunchKernelGGL((k_qattn_delta<T, 0>), dgrid, dim3(256), 0, st, a);
    } else {
        hipLaunchKernelGGL((k_qattn_delta<T, 0>), dgrid, dim3(256), 0, st, a);
    }
    if (!mfma) {
        hipLaunchKernelGGL((k_qattn_bwd_kv_gen<T>), dim3(qa_wave_grid(d)), dim3(256), 0, st, a);
        hipLaunchKernelGGL((k_qattn_bwd_q_gen<T>), dim3(qa_wave_grid(d)), dim3(256), 0, st, a);
    }
}

}  // namespace
}  // namespace qk

using namespace qk;

extern "C" {

int qk_qattn_supported(const qk_qattn_desc_t *desc)
{
    return qa_desc_ok(desc, "qk_qattn_supported") ? qa_path(desc) : 0;
}

size_t qk_qattn_workspace_bytes(const qk_qattn_desc_t *desc, int32_t op)
{
    if (!qa_desc_ok(desc, "qk_qattn_workspace_bytes")) return 0;
    if (op == QK_OP_FWD) return 0;
    if (op == QK_OP_BWD) return qa_delta_bytes(desc);
    return bad_op("qk_qattn_workspace_bytes", op);
}

int qk_qattn_fwd(const qk_qattn_desc_t *desc, const void *q, const void *k, const void *v, const int32_t *lengths, float scale,
                 void *o, float *lse, void *stream)
{
    const char *what = "qk_qattn_fwd";
    if (!qa_desc_ok(desc, what)) return QK_ERR_INVALID_ARG;
    if (!q || !k || !v || !o || !lse) { set_error("%s: NULL buffer", what); return QK_ERR_INVALID_ARG; }
    if (!isfinite(scale)) { set_error("%s: scale must be finite", what); return QK_ERR_INVALID_ARG; }
    const size_t es = elem_size(desc->dtype);
    if (!aligned(q, es) || !aligned(k, es) || !aligned(v, es) || !aligned(o, es) || !aligned(lse, 4) || !aligned(lengths, 4)) {
        set_error("%s: misaligned buffer", what);
        return QK_ERR_INVALID_ARG;
    }
    hipStream_t st = (hipStream_t)stream;
    QaArgs a = qa_args(desc, scale, lengths);
    a.q = q; a.k = k; a.v = v; a.out_o = o; a.lse_out = lse;
    const bool mfma = qa_path(desc) == QK_QATTN_PATH_MFMA && aligned(q, 16) && aligned(k, 16) && aligned(v, 16) && aligned(o, 16);
    if (mfma) by_dtype16(desc->dtype, [&](auto t) { qa_launch_fwd_mfma<decltype(t)>(desc, a, st); });      // (qa_path: never fp32)
    else by_dtype(desc->dtype, [&](auto t) { qa_launch_fwd_gen<decltype(t)>(desc, a, st); });
    return launched(what);
}

int qk_qattn_bwd(const qk_qattn_desc_t *desc, const void *d_o, const void *q, const void *k, const void *v, const void *o,
                 const float *lse, const int32_t *lengths, float scale, void *d_q, void *d_k, void *d_v, void *workspace,
                 size_t workspace_bytes, void *stream)
{
    const char *what = "qk_qattn_bwd";
    if (!qa_desc_ok(desc, what)) return QK_ERR_INVALID_ARG;
    if (!d_o || !q || !k || !v || !o || !lse || !d_q || !d_k || !d_v) { set_error("%s: NULL buffer", what); return QK_ERR_INVALID_ARG; }
    if (!isfinite(scale)) { set_error("%s: scale must be finite", what); return QK_ERR_INVALID_ARG; }
    const size_t es = elem_size(desc->dtype);
    if (!aligned(q, es) || !aligned(k, es) || !aligned(v, es) || !aligned(o, es) || !aligned(d_o, es) || !aligned(d_q, es)
        || !aligned(d_k, es) || !aligned(d_v, es) || !aligned(lse, 4) || !aligned(lengths, 4) || !aligned(workspace, 16)) {
        set_error("%s: misaligned buffer (16 bytes for the workspace)", what);
        return QK_ERR_INVALID_ARG;
    }
    const size_t need = qa_delta_bytes(desc);
    if (workspace_ok(what, workspace, workspace_bytes, need) != QK_OK) return QK_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    QaArgs a = qa_args(desc, scale, lengths);
    a.q = q; a.k = k; a.v = v; a.o = o; a.d_o = d_o; a.lse = lse; a.d_q = d_q; a.d_k = d_k; a.d_v = d_v; a.delta = (float *)workspace;
    const bool mfma = qa_path(desc) == QK_QATTN_PATH_MFMA && aligned(q, 16) && aligned(k, 16) && aligned(v, 16) && aligned(o, 16)
                      && aligned(d_o, 16) && aligned(d_q, 16) && aligned(d_k, 16) && aligned(d_v, 16);
    by_dtype(desc->dtype, [&](auto t) { qa_launch_bwd<decltype(t)>(desc, mfma, a, st); });
    if (mfma) by_dtype16(desc->dtype, [&](auto t) { qa_launch_bwd_mfma<decltype(t)>(desc, a, st); });      // (qa_path: never fp32)
    return launched(what);
}

}  // extern "C"
