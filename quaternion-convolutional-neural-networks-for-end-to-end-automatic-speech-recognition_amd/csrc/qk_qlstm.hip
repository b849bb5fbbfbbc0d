// Quaternion LSTM recurrence (include/qk_rnn.h): one launch per time step, the product h_{t-1} R (forward) / dz R^T (backward) as
// the prologue and the LSTM cell as the epilogue of the same kernel.
//
// Tile mapping of the matrix-core kernels (bf16 / fp16, q_units % 16 == 0): a workgroup of four waves owns 16 batch rows x 16
// hidden units x all four components x all four gates -- 16 accumulator tiles of v_mfma_f32_16x16x32 forward, 4 backward.  The
// four waves SPLIT THE REDUCTION (wave w takes K steps w, w + 4, ...): with one wave per tile the step was a chain of dependent
// global loads with nothing to hide them behind (measured: 61 us per launch at B = 256, U = 1024).  In the accumulator layout a
// lane holds unit (lane & 15) of rows 4 (lane >> 4) .. + 3, so every gate and component of a state element lies in ONE lane of
// each wave: the partial sums meet in LDS ([wave][value][lane], conflict-free, summed in wave order: bit-repeatable), and wave c
// then runs the cell of component c.  One barrier; nothing is needed from another workgroup.  blockIdx = (unit slice, row tile,
// direction).
//
// Operands come straight from global memory as 16-byte fragments (a lane's 8 consecutive reduction indices): h / dz rows as they
// lie, the weights from a COMPACT 16-bit image of R built once per call (forward: fragment-major, [unit slice][K step][part, gate]
// [lane][8], K zero-padded to 32, one linear 1 KB load per fragment; backward: a cast, [Q][4U]).
// The Hamilton sign of a (gathered component, produced component) pair is applied by flipping the sign bits of the h / dz fragment
// in registers: one weight fragment serves four products, and a step reads 2 Q U bytes of weights per row tile instead of 8 Q U.
//
// h has two state buffers (every workgroup reads all of h_{t-1} while others write h_t); c, the dh carry and dc are updated in
// place by the lane that owns the element.  dz_t is written to dzx[:, t] and read from there by the next launch.
#include "qk_common.h"
#include "qk_seq.h"
#include "../../include/qk_rnn.h"

#include <math.h>

namespace qk {
namespace {

// both 16-bit formats keep the sign in bit 15
__device__ __forceinline__ uint4 ql_neg(const uint4 &v)
{
    return make_uint4(v.x ^ 0x80008000u, v.y ^ 0x80008000u, v.z ^ 0x80008000u, v.w ^ 0x80008000u);
}
// sign of the product of gathered component a with compact part a ^ b in produced component b (the dense table)
__device__ __forceinline__ constexpr bool ql_minus(int a, int b) { return (kSignConj >> (a * 4 + b)) & 1u; }
__device__ __forceinline__ float ql_sigmoid(float z) { return 1.f / (1.f + expf(-z)); }

struct QlFwd {
    int B, T, Q, D, ystride, rev0, s;      // s: index of the step in walking order
    const int *len;
    const void *zx;          // (D, B, T, 4U)
    const void *w;           // 16-bit kernels: the fragment-major image (k_ql_prep); generic: R itself, fp32 (D, Q, 4U)
    const void *h_in;        // (D, B, U) or NULL (zero state: the product is skipped)
    void *h_out;
    const float *c_in;       // NULL: zero
    float *c_out;
    void *y;
    float *reserve;          // (D, T, B, 5, U)
};

struct QlBwd {
    int B, T, Q, D, ystride, rev0, s;      // s: index of the step in BACKWARD walking order; s == T: tail mode (dh0)
    const int *len;
    const void *dy;
    const void *w;           // 16-bit kernels: the image (D, Q, 4U); generic: R, fp32
    const void *dh_init;     // dhT or NULL, read at s == 0 in place of the carry
    const float *dc_init;    // dcT or NULL, read at s == 0 in place of dc
    float *dhc;              // (D, B, U) fp32: the part of dh that is not dz R^T (rows that were inactive)
    float *dc;               // (D, B, U) fp32, in place: dc0 when the walk ends
    const void *h0;
    const float *c0;
    const void *y;
    const float *reserve;
    void *dzx;               // (D, B, T, 4U): written at t, read at the previously walked step
    void *hprev;             // (D, B, T, U)
    void *dh0;
};

// The cell of state element (row b, component c, unit u) at step t; zr: the recurrent part of its four gates.
template <typename T>
__device__ __forceinline__ void ql_cell_fwd(const QlFwd &a, int d, int t, int b, int c, int u, const float (&zr)[4])
{
    const int Q = a.Q, U = 4 * Q, e = c * Q + u;
    const long long st = ((long long)d * a.B + b) * U + e;
    const bool active = !a.len || t < a.len[b];
    T *y = (T *)a.y + ((long long)b * a.T + t) * a.ystride + c * (a.D * Q) + d * Q + u;
    T *h_out = (T *)a.h_out + st;
    const float c_prev = a.c_in ? a.c_in[st] : 0.f;
    if (!active) {
        *y = from_f32<T>(0.f);
        *h_out = a.h_in ? ((const T *)a.h_in)[st] : from_f32<T>(0.f);
        if (a.c_in != a.c_out) a.c_out[st] = c_prev;
        return;
    }
    const T *zx = (const T *)a.zx + (((long long)d * a.B + b) * a.T + t) * 4 * U + c * U + u;
    const float gi = ql_sigmoid(to_f32(zx[0]) + zr[0]), gf = ql_sigmoid(to_f32(zx[Q]) + zr[1]);
    const float gg = tanhf(to_f32(zx[2 * Q]) + zr[2]), go = ql_sigmoid(to_f32(zx[3 * Q]) + zr[3]);
    const float c_new = gf * c_prev + gi * gg;
    const T h = from_f32<T>(go * tanhf(c_new));
    *y = h;
    *h_out = h;
    a.c_out[st] = c_new;
    float *rs = a.reserve + (((long long)d * a.T + t) * a.B + b) * 5 * U + e;
    rs[0] = gi; rs[U] = gf; rs[2 * U] = gg; rs[3 * U] = go; rs[4 * U] = c_new;
}

// Backward of the same element; dh_rec: its element of dz R^T of the previously walked step (0 at s == 0).
template <typename T>
__device__ __forceinline__ void ql_cell_bwd(const QlBwd &a, int d, bool rev, int t, int b, int c, int u, float dh_rec)
{
    const int Q = a.Q, U = 4 * Q, e = c * Q + u;
    const long long st = ((long long)d * a.B + b) * U + e;
    const float carry = a.s == 0 ? (a.dh_init ? to_f32(((const T *)a.dh_init)[st]) : 0.f) : a.dhc[st];
    const float dh_in = dh_rec + carry;
    if (a.s == a.T) {                                   // tail: dc already holds dc0
        ((T *)a.dh0)[st] = from_f32<T>(dh_in);
        return;
    }
    const float dc = a.s == 0 ? (a.dc_init ? a.dc_init[st] : 0.f) : a.dc[st];
    const int len = a.len ? a.len[b] : a.T;
    T *dz = (T *)a.dzx + (((long long)d * a.B + b) * a.T + t) * 4 * U + c * U + u;
    T *hp = (T *)a.hprev + (((long long)d * a.B + b) * a.T + t) * U + e;
    if (t >= len) {
        const T zero = from_f32<T>(0.f);
        dz[0] = zero; dz[Q] = zero; dz[2 * Q] = zero; dz[3 * Q] = zero;
        *hp = zero;
        a.dhc[st] = dh_in;
        a.dc[st] = dc;
        return;
    }
    const bool first = rev ? (t == len - 1) : (t == 0);
    const int tp = rev ? t + 1 : t - 1;
    const float *rs = a.reserve + (((long long)d * a.T + t) * a.B + b) * 5 * U + e;
    const float gi = rs[0], gf = rs[U], gg = rs[2 * U], go = rs[3 * U], ct = rs[4 * U];
    const int ycol = c * (a.D * Q) + d * Q + u;
    float c_prev;
    if (first) {
        c_prev = a.c0 ? a.c0[st] : 0.f;
        *hp = a.h0 ? ((const T *)a.h0)[st] : from_f32<T>(0.f);
    } else {
        c_prev = a.reserve[(((long long)d * a.T + tp) * a.B + b) * 5 * U + 4 * U + e];
        *hp = ((const T *)a.y)[((long long)b * a.T + tp) * a.ystride + ycol];
    }
    const float dh = dh_in + to_f32(((const T *)a.dy)[((long long)b * a.T + t) * a.ystride + ycol]);
    const float tc = tanhf(ct);
    const float dct = dc + dh * go * (1.f - tc * tc);
    dz[0] = from_f32<T>(dct * gg * gi * (1.f - gi));
    dz[Q] = from_f32<T>(dct * c_prev * gf * (1.f - gf));
    dz[2 * Q] = from_f32<T>(dct * gi * (1.f - gg * gg));
    dz[3 * Q] = from_f32<T>(dh * tc * go * (1.f - go));
    a.dhc[st] = 0.f;
    a.dc[st] = dct * gf;
}

// ---- matrix-core kernels: 256 threads, blockIdx = (unit slice of 16, row tile of 16, direction) --------------------------------------
inline int ql_ksteps(int Q) { return (Q + 31) / 32; }

template <typename T>
__global__ __launch_bounds__(256) void k_ql_fwd16(const QlFwd a)
{
    __shared__ float part[4 * 64 * 64];                  // [wave][value (b, g, r)][lane]: 64 KB
    const int d = blockIdx.z, row0 = blockIdx.y * 16, u0 = blockIdx.x * 16;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l16 = lane & 15, kg = lane >> 4;
    const int Q = a.Q, U = 4 * Q;
    const bool rev = d == 1 || a.rev0;
    const int t = rev ? a.T - 1 - a.s : a.s;
    floatx4 acc[4][4];
#pragma unroll
    for (int b = 0; b < 4; ++b)
#pragma unroll
        for (int g = 0; g < 4; ++g) acc[b][g] = floatx4{0.f, 0.f, 0.f, 0.f};
    if (a.h_in) {
        const int nk = (Q + 31) / 32;
        // a ragged tile's surplus lanes read the last row again; their results are never stored
        const T *h = (const T *)a.h_in + ((long long)d * a.B + min(row0 + l16, a.B - 1)) * U;
        const uint4 *w = (const uint4 *)a.w + ((long long)d * gridDim.x + blockIdx.x) * nk * 1024 + lane;
        const uint4 zero = make_uint4(0u, 0u, 0u, 0u);
        for (int ks = wave; ks < nk; ks += 4) {
            const int k = ks * 32 + 8 * kg;
            const bool kv = k < Q;                       // Q % 32 == 16: the upper half of the last K step is empty (zeros in the image)
            uint4 af[4], nf[4], bf[16];
#pragma unroll
            for (int c = 0; c < 4; ++c) af[c] = kv ? load16(h + c * Q + k) : zero;
#pragma unroll
            for (int f = 0; f < 16; ++f) bf[f] = w[(ks * 16 + f) * 64];
            // all 20 loads of the K step are in flight before the first product waits for one: left alone, the scheduler keeps two
            // in flight and the step is a chain of load latencies
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int c = 0; c < 4; ++c) nf[c] = ql_neg(af[c]);
#pragma unroll
            for (int p = 0; p < 4; ++p)
#pragma unroll
                for (int g = 0; g < 4; ++g)
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        const int b = c ^ p;
                        acc[b][g] = mfma16(T(), ql_minus(c, b) ? nf[c] : af[c], bf[p * 4 + g], acc[b][g]);
                    }
        }
    }
#pragma unroll
    for (int b = 0; b < 4; ++b)
#pragma unroll
        for (int g = 0; g < 4; ++g)
#pragma unroll
            for (int r = 0; r < 4; ++r) part[(wave * 64 + b * 16 + g * 4 + r) * 64 + lane] = acc[b][g][r];
    __syncthreads();
    const int c = wave;                                  // wave c runs the cells of component c
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int row = row0 + 4 * kg + r;
        if (row >= a.B) continue;
        float zr[4];
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int v = (c * 16 + g * 4 + r) * 64 + lane;
            zr[g] = ((part[v] + part[64 * 64 + v]) + part[2 * 64 * 64 + v]) + part[3 * 64 * 64 + v];
        }
        ql_cell_fwd<T>(a, d, t, row, c, u0 + l16, zr);
    }
}

template <typename T>
__global__ __launch_bounds__(256) void k_ql_bwd16(const QlBwd a)
{
    __shared__ float part[4 * 16 * 64];                  // [wave][value (c, r)][lane]: 16 KB
    const int d = blockIdx.z, row0 = blockIdx.y * 16, u0 = blockIdx.x * 16;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l16 = lane & 15, kg = lane >> 4;
    const int Q = a.Q, U = 4 * Q;
    const bool rev = d == 1 || a.rev0;
    const int t = rev ? a.s : a.T - 1 - a.s;             // (unused in tail mode)
    floatx4 acc[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[c] = floatx4{0.f, 0.f, 0.f, 0.f};
    if (a.s > 0) {
        const int tn = rev ? a.s - 1 : a.T - a.s;        // the step walked before this one
        const T *dz = (const T *)a.dzx + (((long long)d * a.B + min(row0 + l16, a.B - 1)) * a.T + tn) * 4 * U;
        const T *w = (const T *)a.w + (long long)d * Q * 4 * U + (long long)(u0 + l16) * 4 * U;
        const uint4 zero = make_uint4(0u, 0u, 0u, 0u);
        // U % 64 == 0: every K step of 32 is full.  Two of the wave's steps (j0, j0 + 128) per pass: 16 loads in flight together
        for (int j0 = 32 * wave; j0 < U; j0 += 256) {
            uint4 af[2][4], nf[2][4], bf[2][4];
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int j = j0 + 128 * h + 8 * kg;
                const bool jv = j0 + 128 * h < U;        // wave-uniform
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    af[h][b] = jv ? load16(dz + b * U + j) : zero;
                    bf[h][b] = jv ? load16(w + b * U + j) : zero;
                }
            }
            __builtin_amdgcn_sched_barrier(0);           // (as in the forward: no product in front of the last load)
#pragma unroll
            for (int h = 0; h < 2; ++h) {
#pragma unroll
                for (int b = 0; b < 4; ++b) nf[h][b] = ql_neg(af[h][b]);
#pragma unroll
                for (int c = 0; c < 4; ++c)
#pragma unroll
                    for (int p = 0; p < 4; ++p) {
                        const int b = c ^ p;
                        acc[c] = mfma16(T(), ql_minus(c, b) ? nf[h][b] : af[h][b], bf[h][p], acc[c]);
                    }
            }
        }
    }
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int r = 0; r < 4; ++r) part[(wave * 16 + c * 4 + r) * 64 + lane] = acc[c][r];
    __syncthreads();
    const int c = wave;                                  // wave c runs the cells of component c
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int row = row0 + 4 * kg + r;
        if (row >= a.B) continue;
        const int v = (c * 4 + r) * 64 + lane;
        ql_cell_bwd<T>(a, d, rev, t, row, c, u0 + l16, ((part[v] + part[16 * 64 + v]) + part[2 * 16 * 64 + v]) + part[3 * 16 * 64 + v]);
    }
}

// ---- generic kernels: one thread per state element, fp32 FMA; blockIdx = (256 elements of B * U, 1, direction) ---------------------------
template <typename T>
__global__ __launch_bounds__(256) void k_ql_fwd_gen(const QlFwd a)
{
    const int d = blockIdx.z, Q = a.Q, U = 4 * Q;
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long long)a.B * U) return;
    const int b = (int)(idx / U), e = (int)(idx % U), c = e / Q, u = e % Q;
    const bool rev = d == 1 || a.rev0;
    const int t = rev ? a.T - 1 - a.s : a.s;
    float zr[4] = {0.f, 0.f, 0.f, 0.f};
    if (a.h_in) {
        const T *h = (const T *)a.h_in + ((long long)d * a.B + b) * U;
        const float *R = (const float *)a.w + (long long)d * Q * 4 * U;
        for (int g4 = 0; g4 < 4; ++g4) {                 // gathered component
            const float sg = ql_minus(g4, c) ? -1.f : 1.f;
            const float *rp = R + (g4 ^ c) * U + u;
            for (int k = 0; k < Q; ++k) {
                const float hv = sg * to_f32(h[g4 * Q + k]);
                const float *rr = rp + (long long)k * 4 * U;
#pragma unroll
                for (int g = 0; g < 4; ++g) zr[g] += hv * round_to<T>(rr[g * Q]);
            }
        }
    }
    ql_cell_fwd<T>(a, d, t, b, c, u, zr);
}

template <typename T>
__global__ __launch_bounds__(256) void k_ql_bwd_gen(const QlBwd a)
{
    const int d = blockIdx.z, Q = a.Q, U = 4 * Q;
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long long)a.B * U) return;
    const int b = (int)(idx / U), e = (int)(idx % U), c = e / Q, u = e % Q;
    const bool rev = d == 1 || a.rev0;
    const int t = rev ? a.s : a.T - 1 - a.s;
    float dh = 0.f;
    if (a.s > 0) {
        const int tn = rev ? a.s - 1 : a.T - a.s;
        const T *dz = (const T *)a.dzx + (((long long)d * a.B + b) * a.T + tn) * 4 * U;
        const float *R = (const float *)a.w + (long long)d * Q * 4 * U + (long long)u * 4 * U;
        for (int pb = 0; pb < 4; ++pb) {                 // produced component of the forward product
            const float sg = ql_minus(c, pb) ? -1.f : 1.f;
            const T *dzb = dz + pb * U;
            const float *rr = R + (c ^ pb) * U;
            float s = 0.f;
            for (int j = 0; j < U; ++j) s += to_f32(dzb[j]) * round_to<T>(rr[j]);
            dh += sg * s;
        }
    }
    ql_cell_bwd<T>(a, d, rev, t, b, c, u, dh);
}

// 16-bit image of R.  Backward: as stored, (D, Q, 4U).  Forward: the B-operand fragments of k_ql_fwd16,
// [d][unit slice s][K step ks][f = part * 4 + gate][lane][e]: element (k = 32 ks + 8 (lane >> 4) + e, column part * U + gate * Q + 16 s +
// (lane & 15)) of R[d], zero where k >= Q.
template <typename T>
__global__ __launch_bounds__(256) void k_ql_prep(const float *R, T *out, int Q, int D, int fragments)
{
    const int cols = 16 * Q, nk = (Q + 31) / 32, S = Q / 16;
    const long long n = fragments ? (long long)D * S * nk * 16 * 512 : (long long)D * Q * cols;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        if (!fragments) {
            out[i] = from_f32<T>(R[i]);
            continue;
        }
        long long r = i;
        const int e = (int)(r % 8); r /= 8;
        const int lane = (int)(r % 64); r /= 64;
        const int f = (int)(r % 16); r /= 16;
        const int ks = (int)(r % nk); r /= nk;
        const int s = (int)(r % S);
        const long long d = r / S;
        const int k = 32 * ks + 8 * (lane >> 4) + e;
        const int col = (f >> 2) * 4 * Q + (f & 3) * Q + 16 * s + (lane & 15);
        out[i] = from_f32<T>(k < Q ? R[(d * Q + k) * cols + col] : 0.f);
    }
}

bool ql_desc_ok(const qk_qlstm_desc_t *d, const char *what)
{
    if (!desc_head_ok(d, what)) return false;
    if (d->batch < 1 || d->steps < 1 || d->q_units < 1) {
        set_error("%s: batch, steps and q_units must be >= 1 (got %d, %d, %d)", what, d->batch, d->steps, d->q_units);
        return false;
    }
    if (d->directions != 1 && d->directions != 2) { set_error("%s: directions must be 1 or 2 (got %d)", what, d->directions); return false; }
    if (d->flags & ~QK_QLSTM_REVERSE) { set_error("%s: unknown flags 0x%x", what, d->flags); return false; }
    if ((d->flags & QK_QLSTM_REVERSE) && d->directions != 1) { set_error("%s: QK_QLSTM_REVERSE needs directions == 1", what); return false; }
    if (d->q_units > (1 << 16) || (long long)d->batch * 4 * d->q_units >= (1ll << 31) || (long long)d->steps * d->batch >= (1ll << 31)) {
        set_error("%s: shape out of range", what);
        return false;
    }
    if ((long long)d->y_stride < (long long)d->directions * 4 * d->q_units) {
        set_error("%s: y_stride %d is smaller than directions * units = %d", what, d->y_stride, d->directions * 4 * d->q_units);
        return false;
    }
    return true;
}

int ql_path(const qk_qlstm_desc_t *d) { return d->dtype != QK_F32 && d->q_units % 16 == 0 ? QK_QLSTM_PATH_MFMA16 : QK_QLSTM_PATH_GENERIC; }
// elements of the 16-bit image of R (forward: fragment-major with K padded to 32; backward: a cast)
size_t ql_image_elems(const qk_qlstm_desc_t *d, bool fwd)
{
    const size_t Q = (size_t)d->q_units;
    return fwd ? (size_t)d->directions * (Q / 16) * ql_ksteps(d->q_units) * 16 * 512 : (size_t)d->directions * Q * 16 * Q;
}
size_t ql_image_bytes(const qk_qlstm_desc_t *d, bool fwd)
{
    return ql_path(d) == QK_QLSTM_PATH_MFMA16 ? align256(ql_image_elems(d, fwd) * 2) : 0;
}
size_t ql_state_elems(const qk_qlstm_desc_t *d) { return (size_t)d->directions * d->batch * 4 * d->q_units; }

template <typename T>
void ql_launch_prep(const float *R, void *out, const qk_qlstm_desc_t *d, int fragments, hipStream_t st)
{
    const long long n = (long long)ql_image_elems(d, fragments != 0);
    const int blocks = (int)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096);
    hipLaunchKernelGGL((k_ql_prep<T>), dim3(blocks), dim3(256), 0, st, R, (T *)out, d->q_units, d->directions, fragments);
}

template <typename A>
void ql_launch_step(const qk_qlstm_desc_t *d, bool fwd, const A &a, hipStream_t st);

template <>
void ql_launch_step<QlFwd>(const qk_qlstm_desc_t *d, bool, const QlFwd &a, hipStream_t st)
{
    const int Q = d->q_units, B = d->batch, D = d->directions;
    if (ql_path(d) == QK_QLSTM_PATH_MFMA16) {
        const dim3 grid(Q / 16, (B + 15) / 16, D);
        by_dtype16(d->dtype, [&](auto t) { hipLaunchKernelGGL((k_ql_fwd16<decltype(t)>), grid, dim3(256), 0, st, a); });
        return;
    }
    const dim3 grid((unsigned)(((long long)B * 4 * Q + 255) / 256), 1, D);
    by_dtype(d->dtype, [&](auto t) { hipLaunchKernelGGL((k_ql_fwd_gen<decltype(t)>), grid, dim3(256), 0, st, a); });
}

template <>
void ql_launch_step<QlBwd>(const qk_qlstm_desc_t *d, bool, const QlBwd &a, hipStream_t st)
{
    const int Q = d->q_units, B = d->batch, D = d->directions;
    if (ql_path(d) == QK_QLSTM_PATH_MFMA16) {
        const dim3 grid(Q / 16, (B + 15) / 16, D);
        by_dtype16(d->dtype, [&](auto t) { hipLaunchKernelGGL((k_ql_bwd16<decltype(t)>), grid, dim3(256), 0, st, a); });
        return;
    }
    const dim3 grid((unsigned)(((long long)B * 4 * Q + 255) / 256), 1, D);
    by_dtype(d->dtype, [&](auto t) { hipLaunchKernelGGL((k_ql_bwd_gen<decltype(t)>), grid, dim3(256), 0, st, a); });
}

}  // namespace
}  // namespace qk

using namespace qk;

extern "C" {

int qk_qlstm_supported(const qk_qlstm_desc_t *desc)
{
    return ql_desc_ok(desc, "qk_qlstm_supported") ? ql_path(desc) : 0;
}

size_t qk_qlstm_workspace_bytes(const qk_qlstm_desc_t *desc, int32_t op)
{
    if (!ql_desc_ok(desc, "qk_qlstm_workspace_bytes")) return 0;
    if (op == QK_OP_FWD) return ql_image_bytes(desc, true) + 2 * align256(ql_state_elems(desc) * elem_size(desc->dtype));
    if (op == QK_OP_BWD) return ql_image_bytes(desc, false) + align256(ql_state_elems(desc) * 4);
    return bad_op("qk_qlstm_workspace_bytes", op);
}

size_t qk_qlstm_reserve_bytes(const qk_qlstm_desc_t *desc)
{
    if (!ql_desc_ok(desc, "qk_qlstm_reserve_bytes")) return 0;
    return (size_t)desc->steps * ql_state_elems(desc) * 5 * 4;
}

int qk_qlstm_fwd(const qk_qlstm_desc_t *desc, const void *zx, const float *R, const int32_t *lengths, const void *h0, const float *c0,
                 void *y, void *hT, float *cT, void *reserve, void *workspace, size_t workspace_bytes, void *stream)
{
    const char *what = "qk_qlstm_fwd";
    if (!ql_desc_ok(desc, what)) return QK_ERR_INVALID_ARG;
    if (!zx || !R || !y || !hT || !cT || !reserve) { set_error("%s: NULL buffer", what); return QK_ERR_INVALID_ARG; }
    if (!aligned(zx, 16) || !aligned(h0, 16) || !aligned(y, 16) || !aligned(hT, 16) || !aligned(workspace, 16) || !aligned(R, 4)
        || !aligned(c0, 4) || !aligned(cT, 4) || !aligned(reserve, 4) || !aligned(lengths, 4)) {
        set_error("%s: misaligned buffer (16 bytes for zx, h0, y, hT, workspace; 4 for the rest)", what);
        return QK_ERR_INVALID_ARG;
    }
    const size_t need = qk_qlstm_workspace_bytes(desc, QK_OP_FWD);
    if (workspace_ok(what, workspace, workspace_bytes, need) != QK_OK) return QK_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const bool mfma = ql_path(desc) == QK_QLSTM_PATH_MFMA16;
    char *ws = (char *)workspace;
    const size_t img = ql_image_bytes(desc, true), hb = align256(ql_state_elems(desc) * elem_size(desc->dtype));
    if (mfma) by_dtype16(desc->dtype, [&](auto t) { ql_launch_prep<decltype(t)>(R, ws, desc, 1, st); });
    void *hbuf[2] = {ws + img, ws + img + hb};
    QlFwd a;
    a.B = desc->batch; a.T = desc->steps; a.Q = desc->q_units; a.D = desc->directions; a.ystride = desc->y_stride;
    a.rev0 = (desc->flags & QK_QLSTM_REVERSE) ? 1 : 0;
    a.len = lengths; a.zx = zx; a.w = mfma ? (const void *)ws : (const void *)R; a.y = y; a.reserve = (float *)reserve; a.c_out = cT;
    for (int s = 0; s < desc->steps; ++s) {
        a.s = s;
        a.h_in = s == 0 ? h0 : hbuf[(s - 1) & 1];
        a.h_out = s == desc->steps - 1 ? hT : hbuf[s & 1];
        a.c_in = s == 0 ? c0 : cT;
        ql_launch_step<QlFwd>(desc, true, a, st);
    }
    return launched(what);
}

int qk_qlstm_bwd(const qk_qlstm_desc_t *desc, const void *dy, const void *dhT, const float *dcT, const float *R, const int32_t *lengths,
                 const void *h0, const float *c0, const void *y, const void *reserve, void *dzx, void *hprev, void *dh0, float *dc0,
                 void *workspace, size_t workspace_bytes, void *stream)
{
    const char *what = "qk_qlstm_bwd";
    if (!ql_desc_ok(desc, what)) return QK_ERR_INVALID_ARG;
    if (!dy || !R || !y || !reserve || !dzx || !hprev || !dh0 || !dc0) { set_error("%s: NULL buffer", what); return QK_ERR_INVALID_ARG; }
    if (!aligned(dy, 16) || !aligned(dhT, 16) || !aligned(h0, 16) || !aligned(y, 16) || !aligned(dzx, 16) || !aligned(hprev, 16)
        || !aligned(dh0, 16) || !aligned(workspace, 16) || !aligned(R, 4) || !aligned(dcT, 4) || !aligned(c0, 4)
        || !aligned(reserve, 4) || !aligned(dc0, 4) || !aligned(lengths, 4)) {
        set_error("%s: misaligned buffer (16 bytes for the activation buffers and the workspace; 4 for the rest)", what);
        return QK_ERR_INVALID_ARG;
    }
    const size_t need = qk_qlstm_workspace_bytes(desc, QK_OP_BWD);
    if (workspace_ok(what, workspace, workspace_bytes, need) != QK_OK) return QK_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const bool mfma = ql_path(desc) == QK_QLSTM_PATH_MFMA16;
    char *ws = (char *)workspace;
    const size_t img = ql_image_bytes(desc, false);
    if (mfma) by_dtype16(desc->dtype, [&](auto t) { ql_launch_prep<decltype(t)>(R, ws, desc, 0, st); });
    QlBwd a;
    a.B = desc->batch; a.T = desc->steps; a.Q = desc->q_units; a.D = desc->directions; a.ystride = desc->y_stride;
    a.rev0 = (desc->flags & QK_QLSTM_REVERSE) ? 1 : 0;
    a.len = lengths; a.dy = dy; a.w = mfma ? (const void *)ws : (const void *)R; a.dh_init = dhT; a.dc_init = dcT;
    a.dhc = (float *)(ws + img); a.dc = dc0; a.h0 = h0; a.c0 = c0; a.y = y; a.reserve = (const float *)reserve;
    a.dzx = dzx; a.hprev = hprev; a.dh0 = dh0;
    for (int s = 0; s <= desc->steps; ++s) {             // s == steps: the tail launch (dh0)
        a.s = s;
        ql_launch_step<QlBwd>(desc, false, a, st);
    }
    return launched(what);
}

}  // extern "C"
