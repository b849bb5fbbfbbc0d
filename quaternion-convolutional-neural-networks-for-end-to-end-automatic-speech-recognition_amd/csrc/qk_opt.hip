// Scheduled optimiser step (include/qk_opt.h): k_adam / k_adam_guarded with the rate formed on the device from the step counter
// and one float of device memory, an optional weight EMA behind the update, and the in-place swap that `averaged()` uses.
// HBM-bound like its two models: a step moves what k_adam_guarded moves, plus 2 n floats when ema is given.
#include "qk_common.h"

#include "../../include/qk_opt.h"

#include <math.h>

namespace qk {
namespace {

// ---- the schedule: written ONCE, evaluated by qk_lr_schedule_value on the host and by thread 0 of every workgroup ----------
// t: 1-based index of the step.  Everything in double, one rounding to fp32.
__host__ __device__ inline float sched_lr(const qk_lr_schedule_t &sc, long long t, float lr_scale)
{
    const double td = (double)t, s = (double)(t - 1);
    const double W = (double)sc.warmup_steps;
    double w = 1.0;
    if (sc.warmup_steps > 0) { w = td / W; if (w > 1.0) w = 1.0; }
    double f = 1.0;
    switch (sc.kind) {
    case QK_LR_INVERSE_TIME: f = 1.0 / (1.0 + sc.rate * s); break;
    case QK_LR_EXPONENTIAL: f = pow(sc.rate, s / (double)sc.decay_steps); break;
    case QK_LR_COSINE: {
        double x = (td - W) / ((double)sc.total_steps - W);
        x = x < 0.0 ? 0.0 : (x > 1.0 ? 1.0 : x);
        f = sc.floor + (1.0 - sc.floor) * 0.5 * (1.0 + cos(3.14159265358979323846 * x));
        break;
    }
    case QK_LR_INV_SQRT: {
        const double a = W > 1.0 ? W : 1.0;
        f = sqrt(a / (td > a ? td : a));
        break;
    }
    default: break;
    }
    return (float)(sc.base_lr * w * f * (double)lr_scale);
}

// launch constants of the EMA
struct EmaArgs { float decay; int warmup; };

// the scalars of one step, from device memory: formed by thread 0 of every workgroup and by the trailing one-thread launch (which
// records lr_eff and ema_decay: one function, so what is recorded is what was applied, bit for bit)
struct StepScalars { float lr_eff, ema_decay, omd; };

__device__ inline StepScalars step_scalars(const qk_lr_schedule_t &sc, EmaArgs ea, long long t, const qk_opt_state_t *os)
{
    StepScalars r;
    r.lr_eff = sched_lr(sc, t, os->lr_scale);
    double d = (double)ea.decay;
    if (ea.warmup) {
        const double u = (double)os->ema_updates + 1.0;
        const double dw = (1.0 + u) / (10.0 + u);
        if (dw < d) d = dw;
    }
    r.ema_decay = (float)d;
    r.omd = (float)(1.0 - d);
    return r;
}

// k_adam (qk_aux.hip) when !GUARD, k_adam_guarded (qk_train.hip) when GUARD: the element update is theirs, expression for
// expression, with the schedule's rate where they take `lr`.
template <bool ZERO, bool DECAY, bool GUARD, bool EMA>
__global__ void __launch_bounds__(256)
k_adam_sched(float *__restrict__ p, float *__restrict__ g, float *__restrict__ m, float *__restrict__ v,
             const float *__restrict__ decay, float *__restrict__ ema, size_t n, qk_lr_schedule_t sc, EmaArgs ea, float b1, float b2,
             float eps, float gscale, const int *__restrict__ step_dev, float clipvalue,
             const qk_grad_guard_state_t *__restrict__ state, const qk_opt_state_t *__restrict__ os)
{
    size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t stride = (size_t)gridDim.x * 256;
    if constexpr (GUARD) {
        if (state->last_skipped) {                // (the same answer in every thread of the grid)
            if constexpr (ZERO)
                for (; i < n; i += stride) g[i] = 0.f;
            return;
        }
    }
    __shared__ float lr_s, omd_s;
    if (threadIdx.x == 0) {
        const long long ti = (long long)*step_dev + 1;
        const StepScalars sv = step_scalars(sc, ea, ti, os);
        const double t = (double)ti;
        lr_s = (float)((double)sv.lr_eff * sqrt(1.0 - pow((double)b2, t)) / (1.0 - pow((double)b1, t)));
        omd_s = sv.omd;
    }
    __syncthreads();
    const float lr_t = lr_s, omd = omd_s;
    float unscale = gscale, coef = 1.f;
    if constexpr (GUARD) { unscale = state->last_unscale; coef = state->last_coef; }
    for (; i < n; i += stride) {
        float gi = g[i] * unscale;
        if constexpr (DECAY) gi = fmaf(decay[i], p[i], gi);
        if constexpr (GUARD) {
            gi *= coef;                                                            // clipnorm first ...
            if (clipvalue > 0.f) gi = fminf(fmaxf(gi, -clipvalue), clipvalue);     // ... clipvalue second, as Keras does
        }
        const float mi = b1 * m[i] + (1.f - b1) * gi;
        const float vi = b2 * v[i] + (1.f - b2) * gi * gi;
        m[i] = mi;
        v[i] = vi;
        const float pn = p[i] - lr_t * mi / (sqrtf(vi) + eps);
        p[i] = pn;
        if constexpr (EMA) {
            const float e = ema[i];
            ema[i] = e + omd * (pn - e);
        }
        if constexpr (ZERO) g[i] = 0.f;
    }
}

// (behind k_adam_sched on the same stream: every block has read the old values)
__global__ void k_sched_finish(int *c, qk_lr_schedule_t sc, EmaArgs ea, int has_ema, const qk_grad_guard_state_t *__restrict__ state,
                               qk_opt_state_t *__restrict__ os)
{
    if (state && state->last_skipped) return;
    const StepScalars sv = step_scalars(sc, ea, (long long)*c + 1, os);
    os->last_lr = sv.lr_eff;
    if (has_ema) {
        os->last_ema_decay = sv.ema_decay;
        os->ema_updates += 1;
    }
    *c += 1;
}

__global__ void __launch_bounds__(256) k_swap_f32(float *__restrict__ a, float *__restrict__ b, size_t n)
{
    size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t stride = (size_t)gridDim.x * 256;
    for (; i < n; i += stride) {
        const float x = a[i];
        a[i] = b[i];
        b[i] = x;
    }
}

unsigned capped_blocks(size_t n)
{
    size_t blocks = (n + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    return (unsigned)blocks;
}

bool aligned4(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 3) == 0; }

bool overlap(const float *a, const float *b, size_t n)
{
    const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b), bytes = (uintptr_t)n * sizeof(float);
    return x < y + bytes && y < x + bytes;
}

bool sched_ok(const qk_lr_schedule_t *s, const char *what)
{
    if (!s) { set_error("%s: NULL schedule", what); return false; }
    if (s->kind < QK_LR_CONSTANT || s->kind > QK_LR_INV_SQRT) { set_error("%s: unknown schedule kind %d", what, s->kind); return false; }
    if (!isfinite(s->base_lr) || !(s->base_lr > 0.0)) { set_error("%s: base_lr must be finite and > 0 (got %g)", what, s->base_lr); return false; }
    if (s->warmup_steps < 0) { set_error("%s: warmup_steps must be >= 0 (got %d)", what, s->warmup_steps); return false; }
    if ((s->kind == QK_LR_INVERSE_TIME || s->kind == QK_LR_EXPONENTIAL) && (!isfinite(s->rate) || !(s->rate > 0.0))) {
        set_error("%s: rate must be finite and > 0 for this schedule kind (got %g)", what, s->rate);
        return false;
    }
    if (s->kind == QK_LR_EXPONENTIAL && s->decay_steps < 1) { set_error("%s: decay_steps must be >= 1 (got %d)", what, s->decay_steps); return false; }
    if (s->kind == QK_LR_COSINE && s->total_steps <= s->warmup_steps) {
        set_error("%s: total_steps (%d) must exceed warmup_steps (%d) for the cosine schedule", what, s->total_steps, s->warmup_steps);
        return false;
    }
    if (!(s->floor >= 0.0 && s->floor <= 1.0)) { set_error("%s: floor must lie in [0, 1] (got %g)", what, s->floor); return false; }
    return true;
}

int launched(const char *what)
{
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess) return QK_OK;
    set_error("%s: kernel launch failed: %s", what, hipGetErrorString(e));
    return QK_ERR_LAUNCH;
}

}  // namespace
}  // namespace qk

using namespace qk;

extern "C" {

int qk_lr_schedule_value(const qk_lr_schedule_t *sched, int64_t step_index, float lr_scale, float *out)
{
    if (!sched_ok(sched, "qk_lr_schedule_value")) return QK_ERR_INVALID_ARG;
    if (!out) { set_error("qk_lr_schedule_value: NULL out"); return QK_ERR_INVALID_ARG; }
    if (step_index < 1) { set_error("qk_lr_schedule_value: step_index is 1-based (got %lld)", (long long)step_index); return QK_ERR_INVALID_ARG; }
    *out = sched_lr(*sched, (long long)step_index, lr_scale);
    return QK_OK;
}

int qk_adam_step_sched(float *param, float *grad, float *m, float *v, const float *decay, float *ema, size_t n,
                       const qk_lr_schedule_t *sched, float ema_decay, int32_t ema_warmup, float beta1, float beta2, float eps,
                       float grad_scale, int32_t *step_dev, int32_t zero_grad, const qk_grad_guard_config_t *guard_config,
                       const qk_grad_guard_state_t *guard_state, qk_opt_state_t *opt_state, void *stream)
{
    const char *what = "qk_adam_step_sched";
    if (!param || !grad || !m || !v || !step_dev || !opt_state) { set_error("%s: NULL buffer, step counter or opt_state", what); return QK_ERR_INVALID_ARG; }
    if (n == 0) { set_error("%s: n must be > 0", what); return QK_ERR_INVALID_ARG; }
    if (!sched_ok(sched, what)) return QK_ERR_INVALID_ARG;
    if ((guard_config == nullptr) != (guard_state == nullptr)) { set_error("%s: guard_config and guard_state go together (both NULL or both given)", what); return QK_ERR_INVALID_ARG; }
    float clipvalue = 0.f;
    if (guard_config) {
        if (!(guard_config->clipnorm >= 0.f) || !(guard_config->clipvalue >= 0.f)) { set_error("%s: clipnorm / clipvalue must be >= 0", what); return QK_ERR_INVALID_ARG; }
        if (grad_scale != 1.f) { set_error("%s: grad_scale must be 1 with a guard (qk_grad_guard_reduce folded it into last_unscale), got %g", what, (double)grad_scale); return QK_ERR_INVALID_ARG; }
        clipvalue = guard_config->clipvalue;
    }
    if (ema && !(ema_decay >= 0.f && ema_decay < 1.f)) { set_error("%s: ema_decay must lie in [0, 1) (got %g)", what, (double)ema_decay); return QK_ERR_INVALID_ARG; }
    if (!aligned4(param) || !aligned4(grad) || !aligned4(m) || !aligned4(v) || !aligned4(decay) || !aligned4(ema) || !aligned4(step_dev)
        || !aligned4(guard_state) || !aligned4(opt_state)) {
        set_error("%s: buffers, step counter and state blocks need 4-byte alignment", what);
        return QK_ERR_INVALID_ARG;
    }
    const EmaArgs ea = {ema ? ema_decay : 0.f, ema_warmup != 0 ? 1 : 0};
    const unsigned blocks = capped_blocks(n);
    hipStream_t st = (hipStream_t)stream;
#define QK_AS(Z, D, G, E) hipLaunchKernelGGL((k_adam_sched<Z, D, G, E>), dim3(blocks), dim3(256), 0, st, param, grad, m, v, decay, ema, n, *sched, ea, beta1, beta2, eps, grad_scale, (const int *)step_dev, clipvalue, guard_state, (const qk_opt_state_t *)opt_state)
#define QK_AS_E(Z, D, G) do { if (ema) QK_AS(Z, D, G, true); else QK_AS(Z, D, G, false); } while (0)
#define QK_AS_G(Z, D) do { if (guard_state) QK_AS_E(Z, D, true); else QK_AS_E(Z, D, false); } while (0)
    if (zero_grad) { if (decay) QK_AS_G(true, true); else QK_AS_G(true, false); }
    else { if (decay) QK_AS_G(false, true); else QK_AS_G(false, false); }
#undef QK_AS_G
#undef QK_AS_E
#undef QK_AS
    hipLaunchKernelGGL(k_sched_finish, dim3(1), dim3(1), 0, st, (int *)step_dev, *sched, ea, ema ? 1 : 0, guard_state, opt_state);
    return launched(what);
}

int qk_swap_f32(float *a, float *b, size_t n, void *stream)
{
    if (!a || !b) { set_error("qk_swap_f32: NULL buffer"); return QK_ERR_INVALID_ARG; }
    if (n == 0) { set_error("qk_swap_f32: n must be > 0"); return QK_ERR_INVALID_ARG; }
    if (!aligned4(a) || !aligned4(b)) { set_error("qk_swap_f32: buffers need 4-byte alignment"); return QK_ERR_INVALID_ARG; }
    if (overlap(a, b, n)) { set_error("qk_swap_f32: the buffers overlap"); return QK_ERR_INVALID_ARG; }
    hipLaunchKernelGGL(k_swap_f32, dim3(capped_blocks(n)), dim3(256), 0, (hipStream_t)stream, a, b, n);
    return launched("qk_swap_f32");
}

}  // extern "C"
