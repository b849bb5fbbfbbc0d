"""The guarded optimiser step: gradient clipping and dynamic loss scaling around the fused Adam, entirely on the device.

    guard = GradGuard(dev, clipnorm=5.0, loss_scale=2.0 ** 12, dynamic=True)
    step = torch.zeros(1, dtype=torch.int32, device=dev)
    ...
    model.training_loss(x, labels, il, ll, loss_scale=guard.loss_scale).backward()
    guard.step(flat.param, flat.grad, m, v, step, lr=1e-3, zero_grad=True, decay=flat.l2_decay())

`step` is two library calls (include/qk.h, "Guarded optimiser step"): qk_grad_guard_reduce -- one deterministic reduction of the
flat gradient to its global l2 norm and its count of inf / NaN elements, and the step's decisions written into a 32-byte device
block -- then qk_adam_step_guarded, the Adam kernel that reads the block.  Nothing is read on the host and no launch argument
depends on data, so the whole training step still replays as one captured graph.

clipnorm / clipvalue are those of keras.optimizers.Adam in Keras 2 (the global clip of Optimizer.get_gradients, then the element
clamp).  What Keras does not have: a step whose gradient holds an inf or a NaN is skipped -- parameters, moments and the step
counter stay as they are -- and with dynamic=True the loss scale is multiplied by backoff_factor on such a step and by
growth_factor after growth_interval applied steps in a row.
"""
import math

import torch

from . import _lib as L
from . import functional as Fq

_FIELDS = tuple(name for name, _ in L.GRAD_GUARD_STATE)
_SAVED = ('scale', 'good_steps', 'skipped_steps')          # what outlives a step


class GradGuard(object):
    """Clipping, overflow skip and (dynamic=True) loss-scale control for one flat parameter buffer on `device`.

    loss_scale   one-element float32 DEVICE tensor, a view of the state block: hand it to training_loss / ctc_batch_cost
                 (loss_scale=guard.loss_scale); the backward multiplies by whatever it holds at that moment.
    step(...)    reduce + guarded Adam, no host read.
    stats()      the state block as a dict -- the only call that synchronises.
    """

    def __init__(self, device, clipnorm=0.0, clipvalue=0.0, loss_scale=1.0, dynamic=False, growth_factor=2.0, backoff_factor=0.5,
                 growth_interval=2000, min_scale=1.0, max_scale=2.0 ** 24):
        def number(name, x):
            if isinstance(x, bool) or not isinstance(x, (int, float)) or not math.isfinite(x):
                raise ValueError('GradGuard: %s must be a finite number, not %r' % (name, x))
            return float(x)
        clipnorm, clipvalue = number('clipnorm', clipnorm), number('clipvalue', clipvalue)
        loss_scale, growth_factor = number('loss_scale', loss_scale), number('growth_factor', growth_factor)
        backoff_factor, min_scale, max_scale = number('backoff_factor', backoff_factor), number('min_scale', min_scale), number('max_scale', max_scale)
        if clipnorm < 0 or clipvalue < 0:
            raise ValueError('GradGuard: clipnorm and clipvalue must be >= 0 (0 = off)')
        if not 0 < backoff_factor < 1 < growth_factor:
            raise ValueError('GradGuard: 0 < backoff_factor < 1 < growth_factor is required')
        if isinstance(growth_interval, bool) or not isinstance(growth_interval, int) or growth_interval < 1:
            raise ValueError('GradGuard: growth_interval must be an integer >= 1')
        if not 0 < min_scale <= loss_scale <= max_scale:
            raise ValueError('GradGuard: 0 < min_scale <= loss_scale <= max_scale is required')
        self.config = L.GradGuardConfig(clipnorm, clipvalue, int(bool(dynamic)), growth_factor, backoff_factor, growth_interval,
                                        min_scale, max_scale)
        self.device = torch.device(device)
        if self.device.type != 'cuda':
            raise RuntimeError('GradGuard runs on the GPU only (device=%s)' % (device,))
        self._state = torch.zeros(len(_FIELDS), dtype=torch.float32, device=self.device)       # qk_grad_guard_state_t
        self._state_i = self._state.view(torch.int32)
        self.loss_scale = self._state[0:1]
        self.loss_scale.fill_(loss_scale)
        self._state[5] = 1.0                # last_coef / last_unscale of "no step yet"
        self._state[6] = 1.0 / loss_scale
        self._ws = None

    def _workspace(self, n):
        need = int(L.lib().qk_grad_guard_workspace_bytes(n))
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        return self._ws

    def step(self, param, grad, m, v, step_dev, lr=0.001, beta1=0.9, beta2=0.999, eps=1e-7, grad_scale=1.0, zero_grad=False,
             decay=None):
        """One optimiser step on the flat float32 buffers, as functional.adam_step(step=step_dev) takes them.  grad_scale is the
        HOST factor only (1 / world under data parallelism); the loss scale is divided out on the device, from the block."""
        Fq.grad_guard_reduce(grad, self.config, self._state, param if decay is not None else None, decay, grad_scale,
                             self._workspace(grad.numel()))
        Fq.adam_step_guarded(param, grad, m, v, step_dev, self.config, self._state, lr=lr, beta1=beta1, beta2=beta2, eps=eps,
                             zero_grad=zero_grad, decay=decay)

    def stats(self):
        """The state block (include/qk.h: qk_grad_guard_state_t) as a dict of Python numbers.  Synchronises."""
        host = self._state.cpu()
        f, i = host.tolist(), host.view(torch.int32).tolist()
        return {name: (f[k] if is_float else i[k]) for k, (name, is_float) in enumerate(L.GRAD_GUARD_STATE)}

    def state_dict(self):
        s = self.stats()
        return {k: s[k] for k in _SAVED}

    def load_state_dict(self, d):
        """Takes what state_dict() gave; checked on the host as the constructor checks, before anything is written."""
        scale, good, skipped = float(d['scale']), int(d['good_steps']), int(d['skipped_steps'])
        if not self.config.min_scale <= scale <= self.config.max_scale:           # (false for a NaN too)
            raise ValueError('GradGuard.load_state_dict: scale %r is outside this guard\'s [min_scale, max_scale] = [%g, %g]'
                             % (scale, self.config.min_scale, self.config.max_scale))
        if good < 0 or skipped < 0:
            raise ValueError('GradGuard.load_state_dict: good_steps and skipped_steps must be >= 0')
        self.loss_scale.fill_(scale)
        self._state_i[1] = good
        self._state_i[2] = skipped
