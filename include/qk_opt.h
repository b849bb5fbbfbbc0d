/* Scheduled optimiser step: a learning-rate schedule evaluated on the device, an optional exponential moving average of the
 * weights, and an in-place swap -- the entry points added behind version 103 of include/qk.h, exported by the same libqk_hip.so.
 *
 * qk_adam_step_dev / qk_adam_step_guarded take `lr` as a launch argument: a captured graph replays the value it was captured
 * with, so a training step that is one graph cannot warm up or decay.  Here the rate of a step is a function of the DEVICE step
 * counter and of one float in device memory (lr_scale), formed by thread 0 of every workgroup: no launch argument depends on data
 * or on the step number, nothing is read on the host, a skipped step changes nothing, and the results are bit-repeatable. */
#ifndef QK_OPT_H_
#define QK_OPT_H_

#include "qk.h"

#ifdef __cplusplus
extern "C" {
#endif

#define QK_LR_CONSTANT 0
#define QK_LR_INVERSE_TIME 1
#define QK_LR_EXPONENTIAL 2
#define QK_LR_COSINE 3
#define QK_LR_INV_SQRT 4

/* The schedule: HOST struct, launch constants only (40 bytes).  With t = *step_dev + 1 the 1-based index of the step and
 * s = t - 1 the number of steps applied so far, the rate of step t is
 *
 *     lr_eff = (float)(base_lr * w(t) * f(t) * lr_scale)          formed in double, rounded ONCE to fp32
 *
 *     w(t) = min(1, t / warmup_steps) when warmup_steps > 0, else 1
 *     QK_LR_CONSTANT       f = 1
 *     QK_LR_INVERSE_TIME   f = 1 / (1 + rate * s)                              (decay= of Keras 2's Adam)
 *     QK_LR_EXPONENTIAL    f = rate ^ (s / decay_steps)
 *     QK_LR_COSINE         f = floor + (1 - floor) * 0.5 * (1 + cos(pi * x)),  x = clamp((t - warmup_steps) / (total_steps - warmup_steps), 0, 1)
 *     QK_LR_INV_SQRT       f = sqrt(max(warmup_steps, 1) / max(t, warmup_steps, 1))
 *
 * Rejected with QK_ERR_INVALID_ARG before anything is launched: an unknown kind; base_lr not finite or <= 0; warmup_steps < 0;
 * rate not finite or <= 0 for INVERSE_TIME / EXPONENTIAL; decay_steps < 1 for EXPONENTIAL; total_steps <= warmup_steps for COSINE;
 * floor outside [0, 1]. */
typedef struct qk_lr_schedule_t {
    double base_lr;          /* > 0, finite */
    int32_t kind;            /* QK_LR_* */
    int32_t warmup_steps;    /* >= 0; 0: no warm-up */
    int32_t total_steps;     /* COSINE: the step from which f == floor */
    int32_t decay_steps;     /* EXPONENTIAL: steps per factor of `rate` */
    double rate;             /* INVERSE_TIME, EXPONENTIAL */
    double floor;            /* COSINE: in [0, 1] */
} qk_lr_schedule_t;

/* The optimiser's state block, in DEVICE memory (32 bytes, 4-byte aligned). */
typedef struct qk_opt_state_t {
    float lr_scale;          /* INPUT: the caller initialises it to 1; read by every step; anyone may overwrite it between steps */
    float last_lr;           /* lr_eff of the last APPLIED step */
    float last_ema_decay;    /* the decay of the last applied EMA update */
    int32_t ema_updates;     /* EMA updates applied so far */
    int32_t reserved[4];     /* never written */
} qk_opt_state_t;

/* One Adam step whose rate is lr_eff (above) in place of `lr`:  lr_t = (float)((double)lr_eff * sqrt(1 - b2^t) / (1 - b1^t)).
 *
 * guard_config and guard_state are both NULL or both given.  Both NULL: the update is qk_adam_step_dev's, with grad_scale.  Both
 * given: qk_adam_step_guarded's, behind qk_grad_guard_reduce on the same stream; grad_scale must then be 1 (the reduction folded
 * it into last_unscale).  With a constant schedule and lr_scale == 1 the results are bit-identical to those calls with
 * lr = (float)base_lr.
 *
 * ema may be NULL.  When given, behind the update of element i:  ema[i] += omd * (param[i] - ema[i])  in fp32 with
 * omd = (float)(1 - d),  d = ema_warmup ? min(ema_decay, (1 + u) / (10 + u)) : ema_decay  formed in double and u the number of
 * EMA updates INCLUDING this one (the warm-up of TensorFlow's ExponentialMovingAverage).  ema_decay in [0, 1).
 *
 * A skipped step (guard_state->last_skipped set) leaves param, m, v, ema, *step_dev and words 1-3 of opt_state bit-unchanged;
 * grad is still cleared when zero_grad != 0.  An applied step adds 1 to *step_dev and writes last_lr (and, with ema,
 * last_ema_decay and ema_updates) from a trailing one-thread launch.
 *
 * Alignment: every float buffer (param, grad, m, v, decay, ema), step_dev, guard_state and opt_state need 4-byte alignment
 * only; the buffers hold n elements each and must not overlap. */
int qk_adam_step_sched(float *param, float *grad, float *m, float *v, const float *decay, float *ema, size_t n,
                       const qk_lr_schedule_t *sched, float ema_decay, int32_t ema_warmup, float beta1, float beta2, float eps,
                       float grad_scale, int32_t *step_dev, int32_t zero_grad, const qk_grad_guard_config_t *guard_config,
                       const qk_grad_guard_state_t *guard_state, qk_opt_state_t *opt_state, void *stream);

/* Exchange the contents of two fp32 buffers of n elements in place, in one launch, without a temporary.  4-byte alignment; the
 * buffers must not overlap (checked on the host: QK_ERR_INVALID_ARG). */
int qk_swap_f32(float *a, float *b, size_t n, void *stream);

/* HOST only: lr_eff of step `step_index` (1-based) under `lr_scale`, by the function the kernel evaluates; validates `sched`
 * exactly as qk_adam_step_sched does. */
int qk_lr_schedule_value(const qk_lr_schedule_t *sched, int64_t step_index, float lr_scale, float *out);

#ifdef __cplusplus
}
#endif
#endif /* QK_OPT_H_ */
