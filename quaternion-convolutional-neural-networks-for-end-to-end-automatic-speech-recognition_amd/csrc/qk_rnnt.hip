// Transducer (RNN-T) loss: cost and the gradient with respect to the joint's logits, log-softmax fused (include/qk_rnnt.h has the
// semantics, the workspace layout and the three launches).
//
//   k_rnnt_rows<T, GRAD = false>   row pass: lse, lp[.,.,blank], lp[.,.,label[u]] of every active (t, u) row
//   k_rnnt_lattice<NT>             alpha (blockIdx.y = 0) and beta (1) of one batch row as anti-diagonal wavefronts; cost
//   k_rnnt_rows<T, GRAD = true>    gradient pass: the same spans again, g written in the logits' dtype
//
// A (t, u) row is V elements -- 124 bytes at V = 62 in bf16 -- so a row is no unit for 16-byte accesses; 32 consecutive rows are
// (32 V elements = 64 V or 128 V bytes), and that span is what a workgroup stages in LDS, as fp32, in both row kernels.
#include "qk_common.h"
#include "qk_seq.h"
#include "../../include/qk_rnnt.h"

#include <math.h>

namespace qk {
namespace {

constexpr int kRnntRows = 32;        // (t, u) rows per workgroup of the row kernels
constexpr int kRnntLanes = 8;        // lanes that share a row (256 threads / 32 rows)
constexpr int kRnntAhead = 4;        // diagonals whose operands the lattice kernel fetches before it needs them

struct RnntArgs {
    int B, T, U1, V;
    const void *logits;
    const int *labels, *in_len, *lab_len;
    float *cost;
    void *grad;
    float *lse, *alpha, *beta;       // (B, T, U1)
    float *lpb, *lpl;                // (B, T + U1 - 1, U1), diagonal-major
    float *ll;                       // (B)
    int vec;                         // logits (and grad) are 16-byte aligned
};

__device__ __forceinline__ int rnnt_clamp(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

__device__ __forceinline__ float rnnt_logaddexp(float a, float b)
{
    const float m = fmaxf(a, b), n = fminf(a, b);
    if (m == -INFINITY) return -INFINITY;
    return m + log1pf(expf(n - m));                 // n = -inf: exp(-inf) = 0
}

template <typename T> union RnntVec {
    uint4 q;
    T e[16 / sizeof(T)];
    __device__ RnntVec() {}
};

// ---- row pass and gradient pass ------------------------------------------------------------------------------------------------------
template <typename T, bool GRAD>
__global__ __launch_bounds__(256) void k_rnnt_rows(const RnntArgs p)
{
    extern __shared__ __attribute__((aligned(16))) float xs[];          // [kRnntRows][V]
    constexpr int EPV = 16 / (int)sizeof(T);
    const int tid = threadIdx.x, i = tid / kRnntLanes, l = tid % kRnntLanes;
    const int V = p.V, U1 = p.U1, Lmax = p.U1 - 1;
    const long long R = (long long)p.B * p.T * U1;
    const long long r = (long long)blockIdx.x * kRnntRows + i;
    bool act = false;
    int b = 0, t = 0, u = 0, Tb = 0, Ub = 0;
    float llb = 0.f;
    if (r < R) {
        b = (int)(r / ((long long)p.T * U1));
        const int rem = (int)(r - (long long)b * p.T * U1);
        t = rem / U1;
        u = rem - t * U1;
        Tb = rnnt_clamp(p.in_len[b], p.T);
        Ub = rnnt_clamp(p.lab_len[b], Lmax);
        act = t < Tb && u <= Ub;
        if (GRAD && act) {
            llb = p.ll[b];
            act = isfinite(llb);                   // an infeasible batch row: all zeros
        }
    }
    const int any = __syncthreads_or(act ? 1 : 0);
    const long long e0 = (long long)blockIdx.x * kRnntRows * V;
    const long long left = R * V - e0;
    const int span = kRnntRows * V;
    const int nvalid = left < span ? (int)left : span;
    const int nchunks = span / EPV;                // 32 V elements are whole 16-byte chunks in every dtype
    if (any) {
        const T *src = (const T *)p.logits + e0;
        for (int c = tid; c < nchunks; c += 256) {
            const int e = c * EPV;
            if (p.vec && e + EPV <= nvalid) {
                RnntVec<T> v;
                v.q = *reinterpret_cast<const uint4 *>(src + e);
#pragma unroll
                for (int k = 0; k < EPV; ++k) xs[e + k] = to_f32(v.e[k]);
            } else {
                for (int k = 0; k < EPV; ++k)
                    if (e + k < nvalid) xs[e + k] = to_f32(src[e + k]);
            }
        }
    } else if (!GRAD) {
        return;
    }
    __syncthreads();
    float *row = xs + i * V;
    if (!GRAD) {
        // every lane of a row's group takes part in the shuffles; an inactive row's values go nowhere
        float m = -INFINITY;
        for (int v = l; v < V; v += kRnntLanes) m = fmaxf(m, row[v]);
#pragma unroll
        for (int o = kRnntLanes / 2; o; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
        float s = 0.f;
        for (int v = l; v < V; v += kRnntLanes) s += __expf(row[v] - m);
#pragma unroll
        for (int o = kRnntLanes / 2; o; o >>= 1) s += __shfl_xor(s, o);
        if (act && l == 0) {
            const float lse = m + logf(s);
            p.lse[r] = lse;
            const size_t dcell = ((size_t)b * (p.T + U1 - 1) + (t + u)) * U1 + u;
            p.lpb[dcell] = row[V - 1] - lse;
            if (u < Ub) {
                const int lab = p.labels[(size_t)b * Lmax + u];
                p.lpl[dcell] = (lab >= 0 && lab < V - 1) ? row[lab] - lse : -INFINITY;       // a bad label never indexes memory
            }
        }
        return;
    }
    if (act) {
        const float a = p.alpha[r], be = p.beta[r], ls = p.lse[r];
        const float nb = t < Tb - 1 ? p.beta[r + U1] : (u == Ub ? 0.f : -INFINITY);
        const float tb = __expf(((a + nb) - llb) + (row[V - 1] - ls));
        int lab = -1;
        float tl = 0.f;
        if (u < Ub) {
            lab = p.labels[(size_t)b * Lmax + u];                                         // in [0, V - 2]: the batch row is feasible
            tl = __expf(((a + p.beta[r + 1]) - llb) + (row[lab] - ls));
        }
        const float ab = (a + be) - llb;
        for (int v = l; v < V; v += kRnntLanes) {
            float g = __expf(ab + (row[v] - ls));
            if (v == V - 1) g -= tb;
            if (v == lab) g -= tl;
            row[v] = g;
        }
    } else if (r < R) {
        for (int v = l; v < V; v += kRnntLanes) row[v] = 0.f;
    }
    __syncthreads();
    T *dst = (T *)p.grad + e0;
    for (int c = tid; c < nchunks; c += 256) {
        const int e = c * EPV;
        if (p.vec && e + EPV <= nvalid) {
            RnntVec<T> v;
#pragma unroll
            for (int k = 0; k < EPV; ++k) v.e[k] = from_f32<T>(xs[e + k]);
            *reinterpret_cast<uint4 *>(dst + e) = v.q;
        } else {
            for (int k = 0; k < EPV; ++k)
                if (e + k < nvalid) dst[e + k] = from_f32<T>(xs[e + k]);
        }
    }
}

// ---- lattice pass ----------------------------------------------------------------------------------------------------------------------
// Thread u walks column u of the lattice: at step s it sits on anti-diagonal d (alpha: d = s; beta: d = Tb + Ub - 1 - s), cell
// (t = d - u, u).  Its own previous value is the vertical neighbour (t -+ 1, u); lane u -+ 1's previous value is the horizontal one.
template <int NT>
__global__ __launch_bounds__(NT) void k_rnnt_lattice(const RnntArgs p)
{
    __shared__ float ex[2][NT];                      // NT = 128: the neighbour's value crosses the two waves here
    const int b = blockIdx.x, u = threadIdx.x;
    const bool is_beta = blockIdx.y != 0;
    const int U1 = p.U1, Lmax = p.U1 - 1, V = p.V;
    const int Tb = rnnt_clamp(p.in_len[b], p.T), Ub = rnnt_clamp(p.lab_len[b], Lmax);
    int bad = Tb == 0;
    if (u < Ub) {
        const int lab = p.labels[(size_t)b * Lmax + u];
        bad |= lab < 0 || lab >= V - 1;
    }
    if (__syncthreads_or(bad)) {
        if (is_beta && u == 0) { p.cost[b] = INFINITY; p.ll[b] = INFINITY; }
        return;
    }
    const int D = p.T + U1 - 1;
    const float *pbD = p.lpb + (size_t)b * D * U1, *plD = p.lpl + (size_t)b * D * U1;
    float *out = (is_beta ? p.beta : p.alpha) + (size_t)b * p.T * U1;
    const int nsteps = Tb + Ub;                      // anti-diagonals 0 .. Tb - 1 + Ub
    float cur = -INFINITY;
    for (int s0 = 0; s0 < nsteps; s0 += kRnntAhead) {
        float ob[kRnntAhead], ol[kRnntAhead];
#pragma unroll
        for (int k = 0; k < kRnntAhead; ++k) {
            const int s = s0 + k, d = is_beta ? nsteps - 1 - s : s, t = d - u;
            ob[k] = ol[k] = -INFINITY;
            if (s < nsteps && u <= Ub && t >= 0 && t < Tb) {
                if (!is_beta) {
                    if (t > 0) ob[k] = pbD[(size_t)(d - 1) * U1 + u];                   // lp[t-1, u, blank]
                    if (u > 0) ol[k] = plD[(size_t)(d - 1) * U1 + u - 1];               // lp[t, u-1, label[u-1]]
                } else {
                    ob[k] = pbD[(size_t)d * U1 + u];                                    // lp[t, u, blank]
                    if (u < Ub) ol[k] = plD[(size_t)d * U1 + u];                        // lp[t, u, label[u]]
                }
            }
        }
#pragma unroll
        for (int k = 0; k < kRnntAhead; ++k) {
            const int s = s0 + k;
            if (s >= nsteps) break;                  // (the same for the whole workgroup)
            const int d = is_beta ? nsteps - 1 - s : s, t = d - u;
            float nbr;
            if (NT == 64) {
                nbr = is_beta ? __shfl_down(cur, 1) : __shfl_up(cur, 1);
            } else {
                ex[s & 1][u] = cur;
                __syncthreads();
                const int w = is_beta ? u + 1 : u - 1;
                nbr = (w >= 0 && w < NT) ? ex[s & 1][w] : -INFINITY;
            }
            float v = -INFINITY;
            if (u <= Ub && t >= 0 && t < Tb) {
                if (!is_beta) {
                    v = (t == 0 && u == 0) ? 0.f : rnnt_logaddexp(cur + ob[k], nbr + ol[k]);
                } else if (t == Tb - 1 && u == Ub) {
                    v = ob[k];
                } else {
                    v = rnnt_logaddexp(t < Tb - 1 ? cur + ob[k] : -INFINITY, nbr + ol[k]);
                }
                out[(size_t)t * U1 + u] = v;
            }
            cur = v;
        }
    }
    if (is_beta && u == 0) { p.ll[b] = cur; p.cost[b] = -cur; }                          // the last step left beta[0, 0] here
}

// ---- host -------------------------------------------------------------------------------------------------------------------------------
bool rnnt_shape_ok(int B, int T, int U1, int V, const char *what)
{
    if (B < 1 || T < 1) { set_error("%s: B and T must be >= 1 (got %d, %d)", what, B, T); return false; }
    if (V < 2 || V > QK_RNNT_MAX_CLASSES) { set_error("%s: V must be 2 .. %d (got %d)", what, QK_RNNT_MAX_CLASSES, V); return false; }
    if (U1 < 1 || U1 > QK_RNNT_MAX_U1) { set_error("%s: U1 must be 1 .. %d (got %d)", what, QK_RNNT_MAX_U1, U1); return false; }
    if ((long long)B * T * U1 >= (1ll << 31) || (long long)B * (T + U1 - 1) * U1 >= (1ll << 31)) {
        set_error("%s: B * T * U1 must stay below 2^31 (got %d, %d, %d)", what, B, T, U1);
        return false;
    }
    return true;
}

size_t rnnt_ll_words(int B) { return (size_t)(B + 3) / 4 * 4; }

template <typename T>
void rnnt_launch_rows(const RnntArgs &a, bool grad, hipStream_t st)
{
    const long long R = (long long)a.B * a.T * a.U1;
    const dim3 grid((unsigned)((R + kRnntRows - 1) / kRnntRows));
    const size_t lds = (size_t)kRnntRows * a.V * sizeof(float);
    if (grad) hipLaunchKernelGGL((k_rnnt_rows<T, true>), grid, dim3(256), lds, st, a);
    else hipLaunchKernelGGL((k_rnnt_rows<T, false>), grid, dim3(256), lds, st, a);
}

}  // namespace
}  // namespace qk

using namespace qk;

extern "C" {

int qk_rnnt_supported(int32_t dtype, int32_t B, int32_t T, int32_t U1, int32_t V)
{
    if (!dtype_known(dtype)) { set_error("qk_rnnt_supported: unknown dtype %d", dtype); return 0; }
    return rnnt_shape_ok(B, T, U1, V, "qk_rnnt_supported") ? 1 : 0;
}

size_t qk_rnnt_workspace_bytes(int32_t B, int32_t T, int32_t U1, int32_t V)
{
    if (!rnnt_shape_ok(B, T, U1, V, "qk_rnnt_workspace_bytes")) return 0;
    const size_t R = (size_t)B * T * U1, Dg = (size_t)B * (T + U1 - 1) * U1;
    return sizeof(float) * (3 * R + 2 * Dg + rnnt_ll_words(B));
}

int qk_rnnt_loss(int32_t dtype, int32_t B, int32_t T, int32_t U1, int32_t V, const void *logits, const int32_t *labels,
                 const int32_t *input_length, const int32_t *label_length, float *cost, void *grad, void *workspace,
                 size_t workspace_bytes, void *stream)
{
    const char *what = "qk_rnnt_loss";
    if (!dtype_known(dtype)) { set_error("%s: unknown dtype %d", what, dtype); return QK_ERR_INVALID_ARG; }
    if (!rnnt_shape_ok(B, T, U1, V, what)) return QK_ERR_UNSUPPORTED;
    if (!logits || !input_length || !label_length || !cost || (U1 > 1 && !labels)) { set_error("%s: NULL buffer", what); return QK_ERR_INVALID_ARG; }
    const size_t es = elem_size(dtype);
    if (!aligned(logits, es) || !aligned(grad, es) || !aligned(labels, 4) || !aligned(input_length, 4) || !aligned(label_length, 4)
        || !aligned(cost, 4) || !aligned(workspace, 16)) {
        set_error("%s: misaligned buffer (16 bytes for the workspace)", what);
        return QK_ERR_INVALID_ARG;
    }
    const size_t need = qk_rnnt_workspace_bytes(B, T, U1, V);
    if (workspace_ok(what, workspace, workspace_bytes, need) != QK_OK) return QK_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const size_t R = (size_t)B * T * U1, Dg = (size_t)B * (T + U1 - 1) * U1;
    RnntArgs a = {};
    a.B = B; a.T = T; a.U1 = U1; a.V = V;
    a.logits = logits; a.labels = labels; a.in_len = input_length; a.lab_len = label_length; a.cost = cost; a.grad = grad;
    float *ws = (float *)workspace;
    a.lse = ws; a.alpha = ws + R; a.beta = ws + 2 * R; a.lpb = ws + 3 * R; a.lpl = ws + 3 * R + Dg; a.ll = ws + 3 * R + 2 * Dg;
    a.vec = aligned(logits, 16) && aligned(grad, 16);
    // profiling only (QK_ABLATE / qk_set_debug_flags, as in the convolution launchers): 1 skips the row pass, 2 the lattice pass, 4 the
    // gradient pass.  A skipped pass leaves its outputs as the buffers held them; every pass only ever touches its own buffers.
    const int ablate = debug_ablate();
    if (!(ablate & 1)) by_dtype(dtype, [&](auto t) { rnnt_launch_rows<decltype(t)>(a, false, st); });
    if (!(ablate & 2)) {
        if (U1 <= 64) hipLaunchKernelGGL((k_rnnt_lattice<64>), dim3((unsigned)B, 2), dim3(64), 0, st, a);
        else hipLaunchKernelGGL((k_rnnt_lattice<128>), dim3((unsigned)B, 2), dim3(128), 0, st, a);
    }
    if (grad && !(ablate & 4)) by_dtype(dtype, [&](auto t) { rnnt_launch_rows<decltype(t)>(a, true, st); });
    return launched(what);
}

}  // extern "C"
