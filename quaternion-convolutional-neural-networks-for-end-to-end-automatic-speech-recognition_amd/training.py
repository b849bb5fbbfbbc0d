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

Further down: `LRSchedule` / `ScheduledAdam` -- the same step with a learning-rate schedule evaluated on the device and an optional
moving average of the weights (include/qk_opt.h) --, `ReduceOnPlateau` and `save_checkpoint` / `load_checkpoint`.
"""
import contextlib
import ctypes
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


# ---- scheduled Adam: device learning-rate schedule, weight EMA, checkpoints (include/qk_opt.h) --------------------------------

_OPT_FIELDS = tuple(name for name, _ in L.OPT_STATE)


class LRSchedule(object):
    """A learning-rate schedule evaluated ON THE DEVICE from the step counter (include/qk_opt.h: qk_lr_schedule_t).

    With t the 1-based index of a step and s = t - 1:  lr(t) = base_lr * w(t) * f(t) * lr_scale, formed in double and rounded once
    to float32; w(t) = min(1, t / warmup_steps) (1 without warm-up) and f by `kind`:

        'constant'      1
        'inverse-time'  1 / (1 + rate * s)                  -- decay= of keras.optimizers.Adam in Keras 2
        'exponential'   rate ** (s / decay_steps)
        'cosine'        floor + (1 - floor) * (1 + cos(pi * x)) / 2,  x = clamp((t - warmup_steps) / (total_steps - warmup_steps), 0, 1)
        'inv-sqrt'      sqrt(max(warmup_steps, 1) / max(t, warmup_steps, 1))

    value(step) evaluates the same function on the host (qk_lr_schedule_value)."""

    def __init__(self, base_lr, kind='constant', warmup_steps=0, total_steps=0, decay_steps=1, rate=1.0, floor=0.0):
        def number(name, x):
            if isinstance(x, bool) or not isinstance(x, (int, float)) or not math.isfinite(x):
                raise ValueError('LRSchedule: %s must be a finite number, not %r' % (name, x))
            return float(x)

        def count(name, x):
            if isinstance(x, bool) or not isinstance(x, int) or not 0 <= x < 2 ** 31:
                raise ValueError('LRSchedule: %s must be an integer in [0, 2^31), not %r' % (name, x))
            return x
        if kind not in L.QK_LR_KINDS:
            raise ValueError('LRSchedule: kind must be one of %s, not %r' % (sorted(L.QK_LR_KINDS), kind))
        base_lr, rate, floor = number('base_lr', base_lr), number('rate', rate), number('floor', floor)
        warmup_steps, total_steps = count('warmup_steps', warmup_steps), count('total_steps', total_steps)
        decay_steps = count('decay_steps', decay_steps)
        if base_lr <= 0:
            raise ValueError('LRSchedule: base_lr must be > 0')
        if kind in ('inverse-time', 'exponential') and rate <= 0:
            raise ValueError('LRSchedule: rate must be > 0 for kind=%r' % kind)
        if kind == 'exponential' and decay_steps < 1:
            raise ValueError('LRSchedule: decay_steps must be >= 1 for kind=\'exponential\'')
        if kind == 'cosine' and total_steps <= warmup_steps:
            raise ValueError('LRSchedule: total_steps must exceed warmup_steps for kind=\'cosine\'')
        if not 0 <= floor <= 1:
            raise ValueError('LRSchedule: floor must lie in [0, 1]')
        self._config = dict(base_lr=base_lr, kind=kind, warmup_steps=warmup_steps, total_steps=total_steps, decay_steps=decay_steps,
                            rate=rate, floor=floor)
        self.desc = L.LRScheduleDesc(base_lr, L.QK_LR_KINDS[kind], warmup_steps, total_steps, decay_steps, rate, floor)

    def value(self, step, lr_scale=1.0):
        """The rate of step `step` (1-based) as the kernel forms it: a float32 value, returned as a Python float."""
        out = ctypes.c_float()
        L.check(L.lib().qk_lr_schedule_value(ctypes.byref(self.desc), int(step), float(lr_scale), ctypes.byref(out)),
                'qk_lr_schedule_value')
        return out.value

    def get_config(self):
        return dict(self._config)


class ScheduledAdam(object):
    """The fused Adam on the flat buffers of dp.FlatParams with a device learning-rate schedule and, optionally, a
    `training.GradGuard` in front and an exponential moving average of the weights behind (qk_adam_step_sched).

        flat = dp.FlatParams(model.parameters(), direct=True)
        opt = ScheduledAdam(flat.param, flat.grad, LRSchedule(1e-3, 'cosine', warmup_steps=500, total_steps=20000),
                            guard=guard, ema_decay=0.999, decay=flat.l2_decay())
        ...
        opt.step()                              # (guard's reduce +) the update; no host read, captures into a graph
        with opt.averaged():                    # evaluate with the averaged weights
            per = evaluate(model)
        opt.set_lr_scale(plateau.update(per))   # newbob-style halving: a device fill, seen by the next step or replay

    It owns m, v, the device step counter, the state block (qk_opt_state_t) and, when ema_decay > 0, `ema` (initialised to a copy
    of param).  The EMA decay is warmed up as TensorFlow's ExponentialMovingAverage does, min(ema_decay, (1 + u) / (10 + u)) at
    update u, unless ema_warmup=False.  A step the guard skips changes nothing here: not the rate's step index, not the EMA.

    lr_scale      one-element float32 DEVICE view of word 0 of the block, 1 at first; the rate of every step is multiplied by what
                  it holds at that moment.  set_lr_scale(x) fills it.  Under data parallelism EVERY rank must write the same value
                  (derive it from a metric all ranks agree on), or the replicas drift apart.
    stats()       step, last_lr, lr_scale, last_ema_decay, ema_updates -- the only call that synchronises.
    """

    def __init__(self, param, grad, schedule, guard=None, ema_decay=0.0, ema_warmup=True, beta1=0.9, beta2=0.999, eps=1e-7,
                 decay=None):
        if not isinstance(schedule, LRSchedule):
            raise TypeError('ScheduledAdam: schedule must be a training.LRSchedule')
        if guard is not None and not isinstance(guard, GradGuard):
            raise TypeError('ScheduledAdam: guard must be a training.GradGuard or None')
        for name, t in (('param', param), ('grad', grad)) + ((('decay', decay),) if decay is not None else ()):
            if not torch.is_tensor(t) or not t.is_cuda or t.dtype != torch.float32 or t.dim() != 1 or not t.is_contiguous():
                raise RuntimeError('ScheduledAdam: %s must be a flat contiguous float32 device buffer' % name)
            if t.numel() != param.numel() or t.device != param.device:
                raise ValueError('ScheduledAdam: %s must match param in size and device' % name)
        if guard is not None and guard.device != param.device:
            raise ValueError('ScheduledAdam: the guard lives on %s, the buffers on %s' % (guard.device, param.device))
        if isinstance(ema_decay, bool) or not isinstance(ema_decay, (int, float)) or not 0 <= ema_decay < 1:
            raise ValueError('ScheduledAdam: ema_decay must lie in [0, 1) (0 = no averaged weights), not %r' % (ema_decay,))
        self.param, self.grad, self.schedule, self.guard, self.decay = param, grad, schedule, guard, decay
        self.ema_decay, self.ema_warmup = float(ema_decay), bool(ema_warmup)
        self.beta1, self.beta2, self.eps = float(beta1), float(beta2), float(eps)
        self.m, self.v = torch.zeros_like(param), torch.zeros_like(param)
        self.step_dev = torch.zeros(1, dtype=torch.int32, device=param.device)
        self._state = torch.zeros(len(_OPT_FIELDS), dtype=torch.float32, device=param.device)        # qk_opt_state_t
        self._state_i = self._state.view(torch.int32)
        self.lr_scale = self._state[0:1]
        self.lr_scale.fill_(1.0)
        self.ema = param.detach().clone() if self.ema_decay > 0 else None
        self._averaged = False

    def set_lr_scale(self, x):
        """Multiply the schedule by x from the next step on (a device fill: a captured graph sees it on its next replay).  Under
        data parallelism every rank must pass the same x."""
        x = float(x)
        if not math.isfinite(x) or x < 0:
            raise ValueError('ScheduledAdam.set_lr_scale: the scale must be finite and >= 0, not %r' % (x,))
        self.lr_scale.fill_(x)

    def step(self, grad_scale=1.0, zero_grad=True):
        """One optimiser step.  grad_scale is the HOST factor only (1 / world under data parallelism); with a guard the loss scale
        is divided out on the device, as in GradGuard.step."""
        if self._averaged:
            raise RuntimeError('ScheduledAdam.step inside averaged(): param holds the averaged weights; leave the context first')
        g = self.guard
        if g is not None:
            Fq.grad_guard_reduce(self.grad, g.config, g._state, self.param if self.decay is not None else None, self.decay,
                                 grad_scale, g._workspace(self.grad.numel()))
            grad_scale = 1.0
        Fq.adam_step_sched(self.param, self.grad, self.m, self.v, self.step_dev, self.schedule.desc, self._state,
                           guard_config=g.config if g is not None else None, guard_state=g._state if g is not None else None,
                           ema=self.ema, ema_decay=self.ema_decay, ema_warmup=self.ema_warmup, beta1=self.beta1, beta2=self.beta2,
                           eps=self.eps, grad_scale=grad_scale, zero_grad=zero_grad, decay=self.decay)

    def stats(self):
        """step and words 0-3 of the state block as a dict of Python numbers.  Synchronises."""
        host = self._state.cpu()
        f, i = host.tolist(), host.view(torch.int32).tolist()
        out = {'step': int(self.step_dev.item())}
        out.update({name: (f[k] if is_float else i[k]) for k, (name, is_float) in enumerate(L.OPT_STATE[:4])})
        return out

    @contextlib.contextmanager
    def averaged(self):
        """`with opt.averaged(): evaluate(model)` -- param and ema change places (functional.swap_: one launch, the version counter
        moves and the cached 16-bit kernel images are refreshed) and change back on exit, also on an exception."""
        if self.ema is None:
            raise RuntimeError('ScheduledAdam.averaged: no averaged weights are kept (ema_decay == 0)')
        if self._averaged:
            raise RuntimeError('ScheduledAdam.averaged: already inside averaged()')
        Fq.swap_(self.param, self.ema)
        self._averaged = True
        try:
            yield self
        finally:
            Fq.swap_(self.param, self.ema)
            self._averaged = False

    def state_dict(self):
        """m, v (and ema) as CPU tensors, the step count, words 0-3 of the block, the schedule's config and the guard's state."""
        if self._averaged:
            raise RuntimeError('ScheduledAdam.state_dict inside averaged(): leave the context first')
        s = self.stats()
        d = {'m': self.m.cpu(), 'v': self.v.cpu(), 'ema': None if self.ema is None else self.ema.cpu(), 'step': s['step'],
             'lr_scale': s['lr_scale'], 'last_lr': s['last_lr'], 'last_ema_decay': s['last_ema_decay'],
             'ema_updates': s['ema_updates'], 'schedule': self.schedule.get_config(),
             'guard': None if self.guard is None else self.guard.state_dict()}
        return d

    def load_state_dict(self, d):
        """Takes what state_dict() gave; everything is checked on the host before anything is written."""
        if self._averaged:
            raise RuntimeError('ScheduledAdam.load_state_dict inside averaged(): leave the context first')
        if d['schedule'] != self.schedule.get_config():
            raise ValueError('ScheduledAdam.load_state_dict: the checkpoint was written under another schedule: %r, this optimiser '
                             'has %r' % (d['schedule'], self.schedule.get_config()))
        if (d.get('ema') is None) != (self.ema is None):
            raise ValueError('ScheduledAdam.load_state_dict: the checkpoint %s averaged weights, this optimiser %s'
                             % (('holds', 'keeps none') if self.ema is None else ('holds no', 'keeps them')))
        if (d.get('guard') is None) != (self.guard is None):
            raise ValueError('ScheduledAdam.load_state_dict: checkpoint and optimiser disagree on whether there is a guard')
        for name in ('m', 'v') + (('ema',) if self.ema is not None else ()):
            t = d[name]
            if not torch.is_tensor(t) or t.dtype != torch.float32 or t.numel() != self.param.numel():
                raise ValueError('ScheduledAdam.load_state_dict: %s must be a float32 tensor of %d elements' % (name, self.param.numel()))
        step, updates = int(d['step']), int(d['ema_updates'])
        lr_scale = float(d['lr_scale'])
        if step < 0 or updates < 0 or not math.isfinite(lr_scale) or lr_scale < 0:
            raise ValueError('ScheduledAdam.load_state_dict: step, ema_updates and lr_scale must be >= 0')
        if self.guard is not None:
            self.guard.load_state_dict(d['guard'])
        self.m.copy_(d['m'].reshape(-1))
        self.v.copy_(d['v'].reshape(-1))
        if self.ema is not None:
            self.ema.copy_(d['ema'].reshape(-1))
        self.step_dev.fill_(step)
        self._state[0:3].copy_(torch.tensor([lr_scale, float(d['last_lr']), float(d['last_ema_decay'])], dtype=torch.float32))
        self._state_i[3] = updates


class ReduceOnPlateau(object):
    """Newbob-style reduction of the learning rate on a held-out metric (host logic only):

        plateau = ReduceOnPlateau(factor=0.5, patience=0)
        opt.set_lr_scale(plateau.update(per))            # after every evaluation

    update(metric) returns the scale to use from now on.  The first metric sets the best value.  A metric that does not improve on
    the best one by more than min_delta (mode='min': metric < best - min_delta; 'max': metric > best + min_delta) counts as a bad
    evaluation; when more than `patience` bad evaluations follow one another, the scale is multiplied by `factor` (not below
    min_scale) and the count starts again.  A NaN metric is a bad evaluation."""

    def __init__(self, factor=0.5, patience=0, min_delta=0.0, min_scale=1e-3, mode='min'):
        for name, x in (('factor', factor), ('min_delta', min_delta), ('min_scale', min_scale)):
            if isinstance(x, bool) or not isinstance(x, (int, float)) or not math.isfinite(x):
                raise ValueError('ReduceOnPlateau: %s must be a finite number, not %r' % (name, x))
        if not 0 < factor < 1:
            raise ValueError('ReduceOnPlateau: 0 < factor < 1 is required')
        if isinstance(patience, bool) or not isinstance(patience, int) or patience < 0:
            raise ValueError('ReduceOnPlateau: patience must be an integer >= 0')
        if min_delta < 0 or not 0 < min_scale <= 1:
            raise ValueError('ReduceOnPlateau: min_delta >= 0 and 0 < min_scale <= 1 are required')
        if mode not in ('min', 'max'):
            raise ValueError("ReduceOnPlateau: mode must be 'min' or 'max'")
        self.factor, self.patience, self.min_delta, self.min_scale, self.mode = float(factor), patience, float(min_delta), float(min_scale), mode
        self.scale, self.best, self.bad = 1.0, None, 0

    def update(self, metric):
        metric = float(metric)
        if self.best is None and not math.isnan(metric):
            self.best = metric
            return self.scale
        better = self.best is not None and (metric < self.best - self.min_delta if self.mode == 'min' else metric > self.best + self.min_delta)
        if better:
            self.best, self.bad = metric, 0
            return self.scale
        self.bad += 1
        if self.bad > self.patience:
            self.scale = max(self.scale * self.factor, self.min_scale)
            self.bad = 0
        return self.scale

    def state_dict(self):
        return {'scale': self.scale, 'best': self.best, 'bad': self.bad}

    def load_state_dict(self, d):
        scale, best, bad = float(d['scale']), d['best'], int(d['bad'])
        if not self.min_scale <= scale <= 1 or bad < 0 or (best is not None and not isinstance(best, (int, float))):
            raise ValueError('ReduceOnPlateau.load_state_dict: scale must lie in [min_scale, 1], bad must be >= 0 and best a number or None')
        self.scale, self.best, self.bad = scale, None if best is None else float(best), bad


def save_checkpoint(path, model, optimizer=None, policies=(), extra=None):
    """One torch.save of plain CPU tensors and Python numbers (loadable with weights_only=True): model.state_dict(), the optimiser's
    state_dict() (ScheduledAdam: moments, averaged weights, step, rate scale, the guard's scale), the state_dict() of each
    augmentation policy (features.SpecAugment / SpeedPerturb / NoiseReverb: seed and counter) and `extra` (epoch, the plateau
    logic's state, ...).  Synchronises."""
    ckpt = {'model': {k: v.detach().cpu().clone() for k, v in model.state_dict().items()},
            'optimizer': None if optimizer is None else optimizer.state_dict(),
            'policies': [p.state_dict() for p in policies], 'extra': extra}
    torch.save(ckpt, path)


def load_checkpoint(path, model, optimizer=None, policies=()):
    """Restore what save_checkpoint wrote and return its `extra`.  The weights go through model.load_state_dict (in place: views
    into a dp.FlatParams buffer stay views); then the version counter of every parameter's flat buffer is moved and the cached
    16-bit kernel images are refreshed, so that the next forward does not multiply by the images of the weights before the load."""
    ckpt = torch.load(path, map_location='cpu', weights_only=True)
    policies = list(policies)
    if (ckpt['optimizer'] is None) != (optimizer is None):
        raise ValueError('load_checkpoint: the checkpoint %s an optimiser state, the call %s an optimiser'
                         % (('holds', 'gives no') if optimizer is None else ('holds no', 'gives')))
    if len(ckpt['policies']) != len(policies):
        raise ValueError('load_checkpoint: the checkpoint holds %d augmentation policies, the call gives %d'
                         % (len(ckpt['policies']), len(policies)))
    model.load_state_dict(ckpt['model'])
    bases = {}
    for p in model.parameters():
        base = getattr(p, '_qk_flat_base', None)
        if base is not None:
            bases[id(base)] = base
    for base in bases.values():
        torch.autograd.graph.increment_version(base)
    if Fq._PREP_CACHE_ON:
        Fq.refresh_prepped_kernels()
    if optimizer is not None:
        optimizer.load_state_dict(ckpt['optimizer'])
    for pol, sd in zip(policies, ckpt['policies']):
        pol.load_state_dict(sd)
    return ckpt['extra']
