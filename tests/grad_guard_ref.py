"""float64 numpy restatement of the guarded optimiser step (include/qk.h, "Guarded optimiser step"): the gradient reduction, the
clip coefficient, the loss-scale update and the guarded Keras-Adam update.  Written from the formulas of the header and from
test_adam_step_matches_keras_formula (tests/test_gpu_parity.py); shares no code with the library.

The two places where the kernels' float32 arithmetic is part of the CONTRACT are kept in float32 here: unscale = grad_scale /
scale and the scale update (the state block holds float32).  Everything else is float64.
"""
import numpy as np


def effective_grad(grad, unscale, param=None, decay=None):
    g = np.asarray(grad, np.float64) * float(unscale)
    if decay is not None:
        g = g + np.asarray(decay, np.float64) * np.asarray(param, np.float64)
    return g


def norm_and_nonfinite(grad, unscale=1.0, param=None, decay=None):
    """(l2 norm of the gradient Adam consumes, number of inf / NaN elements in it); the norm is +inf when there are any."""
    with np.errstate(all='ignore'):
        g = effective_grad(grad, unscale, param, decay)
        bad = int((~np.isfinite(g.astype(np.float32))).sum())          # the elements are float32 values on the device
        norm = float('inf') if bad else float(np.sqrt(np.sum(g * g)))
    return norm, bad


def clip_coef(norm, clipnorm):
    """Keras 2 get_gradients: the GLOBAL clip."""
    return clipnorm / norm if (clipnorm > 0 and norm > clipnorm) else 1.0


class GuardRef(object):
    def __init__(self, clipnorm=0.0, clipvalue=0.0, loss_scale=1.0, dynamic=False, growth_factor=2.0, backoff_factor=0.5,
                 growth_interval=2000, min_scale=1.0, max_scale=2.0 ** 24):
        self.clipnorm, self.clipvalue, self.dynamic = float(clipnorm), float(clipvalue), bool(dynamic)
        self.growth_factor, self.backoff_factor = np.float32(growth_factor), np.float32(backoff_factor)
        self.growth_interval, self.min_scale, self.max_scale = int(growth_interval), np.float32(min_scale), np.float32(max_scale)
        self.scale, self.good_steps, self.skipped_steps = np.float32(loss_scale), 0, 0
        self.last = {}

    def reduce(self, grad, param=None, decay=None, grad_scale=1.0):
        """The decisions of one step; updates the scale when dynamic.  Returns the `last_*` fields."""
        unscale = np.float32(grad_scale) / self.scale                 # float32, with the scale the step was run with
        norm, bad = norm_and_nonfinite(grad, unscale, param, decay)
        skipped = bad > 0
        self.last = dict(last_norm=norm, nonfinite_count=bad, last_skipped=int(skipped), last_coef=clip_coef(norm, self.clipnorm),
                         last_unscale=float(unscale))
        if self.dynamic:
            if skipped:
                self.scale = max(np.float32(self.scale * self.backoff_factor), self.min_scale)
                self.good_steps = 0
                self.skipped_steps += 1
            else:
                self.good_steps += 1
                if self.good_steps >= self.growth_interval:
                    self.scale = min(np.float32(self.scale * self.growth_factor), self.max_scale)
                    self.good_steps = 0
        return self.last

    def stats(self):
        return dict(self.last, scale=float(self.scale), good_steps=self.good_steps, skipped_steps=self.skipped_steps)

    def step(self, p, grad, m, v, t, lr=0.001, beta1=0.9, beta2=0.999, eps=1e-7, grad_scale=1.0, zero_grad=False, decay=None):
        """One guarded step on float64 arrays; t = steps applied so far.  Returns (p, m, v, t); grad is cleared IN PLACE under
        zero_grad, applied or not."""
        d = self.reduce(grad, p if decay is not None else None, decay, grad_scale)
        if not d['last_skipped']:
            g = effective_grad(grad, d['last_unscale'], p if decay is not None else None, decay) * d['last_coef']
            if self.clipvalue > 0:
                g = np.clip(g, -self.clipvalue, self.clipvalue)
            t = t + 1
            m = beta1 * m + (1 - beta1) * g
            v = beta2 * v + (1 - beta2) * g * g
            p = p - lr * np.sqrt(1 - beta2 ** t) / (1 - beta1 ** t) * m / (np.sqrt(v) + eps)
        if zero_grad:
            grad[...] = 0
        return p, m, v, t
