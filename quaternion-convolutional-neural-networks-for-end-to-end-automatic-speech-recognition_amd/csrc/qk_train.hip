// Guarded optimiser step (include/qk.h, "Guarded optimiser step"): the deterministic gradient reduction with its decision block,
// and the Adam kernel that reads the block.  All of it is HBM-bound: the reduction reads n floats (3 n with the l2 term), the
// update moves what k_adam (qk_aux.hip) moves.
#include "qk_common.h"

#include <climits>

namespace qk {
namespace {

constexpr int kGuardThreads = 256;
constexpr unsigned kGuardMaxBlocks = 2048;            // 8 workgroups per CU: enough 16-byte loads in flight to fill HBM
constexpr size_t kGuardElemsPerBlockPass = (size_t)kGuardThreads * 4;

struct GuardPartial { double sum; unsigned long long bad; };          // one per workgroup of stage one

// the grid of stage one: a function of n ALONE (the order of the additions, hence the bits of the result, follow from it)
unsigned guard_blocks(size_t n)
{
    size_t b = (n + kGuardElemsPerBlockPass - 1) / kGuardElemsPerBlockPass;
    if (b < 1) b = 1;
    if (b > kGuardMaxBlocks) b = kGuardMaxBlocks;
    return (unsigned)b;
}

// one element as Adam will consume it; inf / NaN are recognised on its bits
template <bool DECAY>
__device__ __forceinline__ void guard_elem(float g, float p, float d, float unscale, double &sum, unsigned &bad)
{
    float x = g * unscale;
    if constexpr (DECAY) x = fmaf(d, p, x);
    bad += (__float_as_uint(x) & 0x7f800000u) == 0x7f800000u ? 1u : 0u;
    sum = fma((double)x, (double)x, sum);
}

// sum / bad of the 256 threads of a workgroup, in a fixed (tree) order; valid in thread 0
__device__ __forceinline__ void guard_block_sum(double &sum, unsigned long long &bad)
{
    __shared__ double s_sum[kGuardThreads];
    __shared__ unsigned long long s_bad[kGuardThreads];
    const int t = threadIdx.x;
    s_sum[t] = sum;
    s_bad[t] = bad;
    __syncthreads();
    for (int w = kGuardThreads / 2; w > 0; w >>= 1) {
        if (t < w) {
            s_sum[t] += s_sum[t + w];
            s_bad[t] += s_bad[t + w];
        }
        __syncthreads();
    }
    sum = s_sum[0];
    bad = s_bad[0];
}

// Stage one.  `head` elements in front of the first 16-byte boundary of grad and the n % 4 tail behind the last whole float4 are
// read one by one (by the first head + tail threads of the grid); the body goes through 16-byte loads.  PD_VEC: param and decay
// sit at the same offset from a 16-byte boundary as grad (views of flat buffers at one element offset do) and are read the same
// way; otherwise element by element.
template <bool DECAY, bool PD_VEC>
__global__ void __launch_bounds__(kGuardThreads)
k_guard_partial(const float *__restrict__ grad, const float *__restrict__ param, const float *__restrict__ decay, size_t n,
                size_t head, float grad_scale, const qk_grad_guard_state_t *__restrict__ state, GuardPartial *__restrict__ part)
{
    const float unscale = grad_scale / state->scale;
    const size_t nvec = (n - head) >> 2;
    const size_t gtid = (size_t)blockIdx.x * kGuardThreads + threadIdx.x;
    const size_t stride = (size_t)gridDim.x * kGuardThreads;
    const float4 *g4 = reinterpret_cast<const float4 *>(grad + head);
    double sum = 0.0;
    unsigned bad = 0;
    for (size_t q = gtid; q < nvec; q += stride) {
        const float4 g = g4[q];
        float4 p = make_float4(0.f, 0.f, 0.f, 0.f), d = p;
        if constexpr (DECAY) {
            if constexpr (PD_VEC) {
                p = reinterpret_cast<const float4 *>(param + head)[q];
                d = reinterpret_cast<const float4 *>(decay + head)[q];
            } else {
                const float *pp = param + head + 4 * q, *dd = decay + head + 4 * q;
                p = make_float4(pp[0], pp[1], pp[2], pp[3]);
                d = make_float4(dd[0], dd[1], dd[2], dd[3]);
            }
        }
        guard_elem<DECAY>(g.x, p.x, d.x, unscale, sum, bad);
        guard_elem<DECAY>(g.y, p.y, d.y, unscale, sum, bad);
        guard_elem<DECAY>(g.z, p.z, d.z, unscale, sum, bad);
        guard_elem<DECAY>(g.w, p.w, d.w, unscale, sum, bad);
    }
    const size_t tail0 = head + 4 * nvec;
    if (gtid < head + (n - tail0)) {
        const size_t i = gtid < head ? gtid : tail0 + (gtid - head);
        guard_elem<DECAY>(grad[i], DECAY ? param[i] : 0.f, DECAY ? decay[i] : 0.f, unscale, sum, bad);
    }
    unsigned long long bad_ll = bad;
    guard_block_sum(sum, bad_ll);
    if (threadIdx.x == 0) {
        part[blockIdx.x].sum = sum;
        part[blockIdx.x].bad = bad_ll;
    }
}

// Stage two and the decisions: ONE workgroup.  Thread t adds partials t, t + 256, ... in rising order, the tree adds the threads.
__global__ void __launch_bounds__(kGuardThreads)
k_guard_finalise(const GuardPartial *__restrict__ part, unsigned nparts, float grad_scale, qk_grad_guard_config_t cfg,
                 qk_grad_guard_state_t *__restrict__ state)
{
    double sum = 0.0;
    unsigned long long bad = 0;
    for (unsigned i = threadIdx.x; i < nparts; i += kGuardThreads) {
        sum += part[i].sum;
        bad += part[i].bad;
    }
    guard_block_sum(sum, bad);
    if (threadIdx.x != 0) return;
    const float scale = state->scale;
    const bool skipped = bad > 0;
    const double norm = skipped ? (double)INFINITY : sqrt(sum);
    float coef = 1.f;
    if (cfg.clipnorm > 0.f && norm > (double)cfg.clipnorm) coef = (float)((double)cfg.clipnorm / norm);
    state->last_norm = (float)norm;
    state->nonfinite_count = bad > (unsigned long long)INT_MAX ? INT_MAX : (int)bad;
    state->last_skipped = skipped ? 1 : 0;
    state->last_coef = coef;
    state->last_unscale = grad_scale / scale;           // the factor stage one used: the scale this step's backward ran with
    if (cfg.dynamic) {
        if (skipped) {
            state->scale = fmaxf(scale * cfg.backoff_factor, cfg.min_scale);
            state->good_steps = 0;
            state->skipped_steps += 1;
        } else {
            const int good = state->good_steps + 1;
            if (good >= cfg.growth_interval) {
                state->scale = fminf(scale * cfg.growth_factor, cfg.max_scale);
                state->good_steps = 0;
            } else {
                state->good_steps = good;
            }
        }
    }
}

// k_adam (qk_aux.hip) on the gradient the guard decided on.  The update itself is k_adam's, expression for expression: with
// last_unscale == gscale, last_coef == 1 and no clamp the two kernels write the same bits.
template <bool ZERO, bool DECAY>
__global__ void __launch_bounds__(256)
k_adam_guarded(float *__restrict__ p, float *__restrict__ g, float *__restrict__ m, float *__restrict__ v,
               const float *__restrict__ decay, size_t n, float b1, float b2, float eps, const int *__restrict__ step_dev, float lr,
               float clipvalue, const qk_grad_guard_state_t *__restrict__ state)
{
    size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t stride = (size_t)gridDim.x * 256;
    if (state->last_skipped) {                // (the same answer in every thread of the grid)
        if constexpr (ZERO)
            for (; i < n; i += stride) g[i] = 0.f;
        return;
    }
    __shared__ float lr_s;
    if (threadIdx.x == 0) {
        const double t = (double)(*step_dev + 1);
        lr_s = (float)((double)lr * sqrt(1.0 - pow((double)b2, t)) / (1.0 - pow((double)b1, t)));
    }
    __syncthreads();
    const float lr_t = lr_s;
    const float unscale = state->last_unscale, coef = state->last_coef;
    for (; i < n; i += stride) {
        float gi = g[i] * unscale;
        if constexpr (DECAY) gi = fmaf(decay[i], p[i], gi);
        gi *= coef;                                                            // clipnorm first ...
        if (clipvalue > 0.f) gi = fminf(fmaxf(gi, -clipvalue), clipvalue);     // ... clipvalue second, as Keras does
        const float mi = b1 * m[i] + (1.f - b1) * gi;
        const float vi = b2 * v[i] + (1.f - b2) * gi * gi;
        m[i] = mi;
        v[i] = vi;
        p[i] -= lr_t * mi / (sqrtf(vi) + eps);
        if constexpr (ZERO) g[i] = 0.f;
    }
}
// (behind k_adam_guarded on the same stream: every block has read the old value)
__global__ void k_bump_guarded(int *c, const qk_grad_guard_state_t *__restrict__ state) { if (!state->last_skipped) *c += 1; }

inline size_t misalign16(const void *p) { return (size_t)(reinterpret_cast<uintptr_t>(p) & 15); }

}  // namespace

size_t grad_guard_workspace_bytes(size_t n) { return (size_t)guard_blocks(n) * sizeof(GuardPartial); }

int launch_grad_guard_reduce(const float *grad, const float *param, const float *decay, size_t n, float grad_scale,
                             const qk_grad_guard_config_t &cfg, qk_grad_guard_state_t *state, void *ws, hipStream_t stream)
{
    const unsigned blocks = guard_blocks(n);
    size_t head = ((16 - misalign16(grad)) & 15) >> 2;           // elements up to the first 16-byte boundary
    if (head > n) head = n;
    GuardPartial *part = static_cast<GuardPartial *>(ws);
#define QK_GP(D, V) hipLaunchKernelGGL((k_guard_partial<D, V>), dim3(blocks), dim3(kGuardThreads), 0, stream, grad, param, decay, n, head, grad_scale, state, part)
    if (!decay) QK_GP(false, false);
    else if (misalign16(param) == misalign16(grad) && misalign16(decay) == misalign16(grad)) QK_GP(true, true);
    else QK_GP(true, false);
#undef QK_GP
    hipLaunchKernelGGL(k_guard_finalise, dim3(1), dim3(kGuardThreads), 0, stream, part, blocks, grad_scale, cfg, state);
    return hipGetLastError() == hipSuccess ? 0 : QK_ERR_LAUNCH;
}

int launch_adam_guarded(float *p, float *g, float *m, float *v, const float *decay, size_t n, float lr, float b1, float b2, float eps,
                        int *step_dev, bool zero_grad, float clipvalue, const qk_grad_guard_state_t *state, hipStream_t stream)
{
    size_t blocks = (n + 255) / 256;
    if (blocks > 2048) blocks = 2048;
#define QK_ADAM_G(Z, D) hipLaunchKernelGGL((k_adam_guarded<Z, D>), dim3((unsigned)blocks), dim3(256), 0, stream, p, g, m, v, decay, n, b1, b2, eps, (const int *)step_dev, lr, clipvalue, state)
    if (zero_grad) { if (decay) QK_ADAM_G(true, true); else QK_ADAM_G(true, false); }
    else { if (decay) QK_ADAM_G(false, true); else QK_ADAM_G(false, false); }
#undef QK_ADAM_G
    hipLaunchKernelGGL(k_bump_guarded, dim3(1), dim3(1), 0, stream, step_dev, state);
    return hipGetLastError() == hipSuccess ? 0 : QK_ERR_LAUNCH;
}

}  // namespace qk
