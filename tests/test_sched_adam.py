"""The scheduled optimiser step (include/qk_opt.h; qcnn_amd.training.LRSchedule / ScheduledAdam / ReduceOnPlateau / save_checkpoint):
the learning-rate schedule evaluated on the device, the weight EMA, the in-place swap behind averaged(), checkpoints -- against the
float64 restatement of tests/sched_adam_ref.py and, bit for bit, against the existing steps it must not deviate from.

Tolerances.  Rate: equal or ADJACENT float32 values (<= 1 ulp) -- both sides compute in double, libm cos / pow may differ in the
last bits of a double, one rounding to float32 follows.  EMA element after ONE update from the device's own previous ema and new
param: 4 * 2^-24 * (|p| + |ema_prev|) -- three float32 roundings (the difference, the product, the sum) plus the rounding of
omd, each bounded through |p - e| <= |p| + |e| and |e'| <= max(|p|, |e|).  Everything else is compared bit for bit.
"""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import guarded_alloc as GA
import sched_adam_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the grid is capped at 2048 workgroups of 256 threads: the last size sends every workgroup round its grid-stride loop a second time
SIZES = [1, 255, 256, 257, 4099, 2048 * 256 + 3]
KIND_KW = {
    'constant': dict(),
    'inverse-time': dict(rate=0.05),
    'exponential': dict(rate=0.9, decay_steps=7),
    'cosine': dict(floor=0.1),
    'inv-sqrt': dict(),
}
ADAM = dict(beta1=0.9, beta2=0.999, eps=1e-7)
BASE_LR = 5e-4


def _dev():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    return torch.device('cuda:0')


def _bits(t):
    return t.detach().contiguous().view(torch.int32).cpu()


def _header():
    return open(os.path.join(ROOT, 'include', 'qk_opt.h')).read()


def _sched_kw(kind, warmup_steps, total_steps):
    kw = dict(KIND_KW[kind], warmup_steps=warmup_steps)
    if kind == 'cosine':
        kw['total_steps'] = total_steps
    return kw


# ---- CPU part ------------------------------------------------------------------------------------------------------------------
def test_opt_header_inventory_equals_the_second_symbol_table():
    from qcnn_amd import _lib
    lib = _lib.lib()
    declared = set(re.findall(r'\b(qk_[a-z_0-9]+)\s*\(', _header()))
    declared -= {n for n in declared if n.endswith('_t')}
    assert declared == set(_lib.OPT_SYMBOLS), declared ^ set(_lib.OPT_SYMBOLS)
    for name in declared:
        assert hasattr(lib, name), name
    assert not set(_lib.OPT_SYMBOLS) & set(_lib.SYMBOLS)
    assert lib.qk_version() == 103
    main = open(os.path.join(ROOT, 'include', 'qk.h')).read()
    assert not any(name in main for name in _lib.OPT_SYMBOLS)


def test_opt_structs_match_the_header():
    from qcnn_amd import _lib
    h = _header()
    body = h[h.index('typedef struct qk_lr_schedule_t {'):h.index('} qk_lr_schedule_t;')]
    fields = re.findall(r'^\s*(double|int32_t)\s+([a-z_]+);', body, re.M)
    ctype = {'double': ctypes.c_double, 'int32_t': ctypes.c_int32}
    assert [(n, ctype[t]) for t, n in fields] == list(_lib.LRScheduleDesc._fields_)
    assert ctypes.sizeof(_lib.LRScheduleDesc) == 3 * 8 + 4 * 4 == 40
    body = h[h.index('typedef struct qk_opt_state_t {'):h.index('} qk_opt_state_t;')]
    words = []
    for t, n, rep in re.findall(r'^\s*(float|int32_t)\s+([a-z_]+)(?:\[(\d+)\])?;', body, re.M):
        words += [(n, t == 'float')] if not rep else [('%s%d' % (n, i), t == 'float') for i in range(int(rep))]
    assert words == list(_lib.OPT_STATE) and len(words) == 8
    assert [n for n, _ in words[:4]] == ['lr_scale', 'last_lr', 'last_ema_decay', 'ema_updates']
    for name, value in re.findall(r'#define (QK_LR_[A-Z_]+) (\d+)', h):
        assert getattr(_lib, name) == int(value)
    assert sorted(_lib.QK_LR_KINDS.values()) == [0, 1, 2, 3, 4] and set(_lib.QK_LR_KINDS) == set(R.KINDS)


def test_launching_entry_points_end_in_a_stream_and_the_host_one_does_not():
    from qcnn_amd import _lib
    decls = dict(re.findall(r'^int (qk_[a-z_0-9]+)\(([^;]*)\);', _header(), re.M | re.S))
    assert set(decls) == set(_lib.OPT_SYMBOLS)
    host_only = {'qk_lr_schedule_value'}
    for name, args in decls.items():
        last = ' '.join(args.split(',')[-1].split())
        res, argtypes = _lib.OPT_SYMBOLS[name]
        assert res is ctypes.c_int and len(argtypes) == len(args.split(','))
        if name in host_only:
            assert 'stream' not in args and argtypes[-1] is not ctypes.c_void_p
        else:
            assert last == 'void *stream' and argtypes[-1] is ctypes.c_void_p, name


@pytest.mark.parametrize('kind', R.KINDS)
def test_schedule_value_matches_the_reference(kind):
    from qcnn_amd.training import LRSchedule
    kw = dict(KIND_KW[kind], warmup_steps=5)
    if kind == 'cosine':
        kw['total_steps'] = 30
    sched = LRSchedule(BASE_LR, kind, **kw)
    assert sched.get_config()['kind'] == kind and sched.get_config()['base_lr'] == BASE_LR
    for scale in (1.0, 0.5):
        got = [sched.value(t, lr_scale=scale) for t in range(1, 41)]
        for t, g in zip(range(1, 41), got):
            want = R.lr_f32(kind, t, BASE_LR, scale, **kw)
            assert R.ulp_distance(g, want) <= 1, (kind, t, scale, g, float(want))
        assert all(a < b for a, b in zip(got[:4], got[1:5])), 'warm-up must rise strictly up to step 5'
        if kind == 'constant':
            assert got[4:] == [float(np.float32(BASE_LR * scale))] * 36
        if kind == 'cosine':
            assert all(R.ulp_distance(g, np.float32(0.1 * BASE_LR * scale)) <= 1 for g in got[29:])
            assert got[29] == got[39]
        if kind != 'constant':
            assert got[39] < got[4]
    # f is continuous where warm-up ends: f(warmup_steps) is 1 for the kinds anchored there, within one step's decay for the others
    f5 = R.factor(kind, 5, **kw)
    f6 = R.factor(kind, 6, **kw)
    assert 0 < f6 <= f5 <= 1.0
    if kind in ('constant', 'cosine', 'inv-sqrt'):
        assert f5 == 1.0
    assert f5 - f6 < 0.1


def test_schedule_constant_is_base_lr_exactly_and_inverse_time_is_keras_decay():
    from qcnn_amd.training import LRSchedule
    for base in (1e-3, 5e-4, 0.1, 3.0):
        s = LRSchedule(base)
        assert [s.value(t) for t in (1, 2, 1000, 2 ** 31 - 1)] == [float(np.float32(base))] * 4
    s = LRSchedule(1e-3, 'inverse-time', rate=1e-2)
    for iterations in (0, 1, 10, 999):          # Keras 2: lr * 1 / (1 + decay * iterations), iterations = steps applied so far
        assert R.ulp_distance(s.value(iterations + 1), np.float32(1e-3 / (1.0 + 1e-2 * iterations))) <= 1


BAD_SCHEDULES = [
    ('kind', dict(kind=7)), ('kind', dict(kind=-1)),
    ('base_lr', dict(base_lr=0.0)), ('base_lr', dict(base_lr=-1e-3)), ('base_lr', dict(base_lr=float('inf'))),
    ('base_lr', dict(base_lr=float('nan'))),
    ('rate', dict(kind=1, rate=0.0)), ('rate', dict(kind=2, rate=-0.5)), ('rate', dict(kind=2, rate=float('nan'))),
    ('decay_steps', dict(kind=2, rate=0.9, decay_steps=0)),
    ('total_steps', dict(kind=3, warmup_steps=5, total_steps=5)), ('total_steps', dict(kind=3, warmup_steps=5, total_steps=0)),
    ('floor', dict(floor=-0.1)), ('floor', dict(floor=1.5)), ('floor', dict(floor=float('nan'))),
    ('warmup_steps', dict(warmup_steps=-1)),
]


def _desc(**kw):
    from qcnn_amd import _lib
    d = dict(base_lr=1e-3, kind=0, warmup_steps=0, total_steps=0, decay_steps=1, rate=1.0, floor=0.0)
    d.update(kw)
    return _lib.LRScheduleDesc(d['base_lr'], d['kind'], d['warmup_steps'], d['total_steps'], d['decay_steps'], d['rate'], d['floor'])


def _host_block(n=16):
    """n floats of HOST memory: non-NULL, 4-byte aligned pointers for calls that must be refused before anything is launched."""
    buf = (ctypes.c_float * n)()
    return buf, ctypes.addressof(buf)


def _sched_call(lib, ptrs, n=8, sched=None, ema=None, grad_scale=1.0, cfg=None, gstate=None, ostate='ok', step='ok', ema_decay=0.5):
    null_sched = isinstance(sched, str)
    sched = _desc() if sched is None else sched
    return lib.qk_adam_step_sched(ptrs[0], ptrs[1], ptrs[2], ptrs[3], None, ema, n, None if null_sched else ctypes.byref(sched),
                                  ema_decay, 1, 0.9, 0.999, 1e-7, grad_scale, ptrs[4] if step == 'ok' else None, 0,
                                  ctypes.byref(cfg) if cfg is not None else None, gstate, ptrs[5] if ostate == 'ok' else None, None)


@pytest.mark.parametrize('word,kw', BAD_SCHEDULES, ids=['%s:%s' % (w, ','.join('%s=%s' % kv for kv in kw.items())) for w, kw in BAD_SCHEDULES])
def test_invalid_schedule_is_rejected_without_gpu(word, kw):
    from qcnn_amd import _lib
    lib = _lib.lib()
    out = ctypes.c_float(-1.0)
    assert lib.qk_lr_schedule_value(ctypes.byref(_desc(**kw)), 1, 1.0, ctypes.byref(out)) == _lib.QK_ERR_INVALID_ARG
    msg = lib.qk_last_error()
    assert word.encode() in msg and b'qk_lr_schedule_value' in msg, msg
    assert out.value == -1.0
    keep = [_host_block() for _ in range(6)]
    assert _sched_call(lib, [p for _, p in keep], sched=_desc(**kw)) == _lib.QK_ERR_INVALID_ARG
    msg = lib.qk_last_error()
    assert word.encode() in msg and b'qk_adam_step_sched' in msg, msg


def test_invalid_arguments_are_rejected_without_gpu():
    from qcnn_amd import _lib
    lib = _lib.lib()
    keep = [_host_block() for _ in range(8)]
    ptrs = [p for _, p in keep]
    bad = _lib.QK_ERR_INVALID_ARG
    cfg = _lib.GradGuardConfig()

    def err(rc, word):
        msg = lib.qk_last_error()
        assert rc == bad and word.encode() in msg, (rc, word, msg)
    for i in range(4):                                              # param, grad, m, v
        q = list(ptrs)
        q[i] = None
        err(_sched_call(lib, q), 'NULL')
    err(_sched_call(lib, ptrs, step=None), 'NULL')
    err(_sched_call(lib, ptrs, ostate=None), 'NULL')
    err(_sched_call(lib, ptrs, sched='null'), 'NULL')
    err(_sched_call(lib, ptrs, n=0), 'n must be')
    err(_sched_call(lib, ptrs, cfg=cfg), 'go together')             # a lone guard_config
    err(_sched_call(lib, ptrs, gstate=ptrs[6]), 'go together')      # a lone guard_state
    err(_sched_call(lib, ptrs, cfg=cfg, gstate=ptrs[6], grad_scale=0.5), 'grad_scale')
    err(_sched_call(lib, ptrs, ema=ptrs[7], ema_decay=1.0), 'ema_decay')
    err(_sched_call(lib, ptrs, ema=ptrs[7], ema_decay=-0.1), 'ema_decay')
    q = list(ptrs)
    q[2] += 2
    err(_sched_call(lib, q), 'alignment')
    out = ctypes.c_float()
    err(lib.qk_lr_schedule_value(None, 1, 1.0, ctypes.byref(out)), 'NULL')
    err(lib.qk_lr_schedule_value(ctypes.byref(_desc()), 1, 1.0, None), 'NULL')
    err(lib.qk_lr_schedule_value(ctypes.byref(_desc()), 0, 1.0, ctypes.byref(out)), '1-based')
    # qk_swap_f32
    a = ptrs[0]
    err(lib.qk_swap_f32(None, a, 4, None), 'NULL')
    err(lib.qk_swap_f32(a, None, 4, None), 'NULL')
    err(lib.qk_swap_f32(a, ptrs[1], 0, None), 'n must be')
    err(lib.qk_swap_f32(a + 1, ptrs[1], 4, None), 'alignment')
    for x, y, n in ((a, a, 4), (a, a + 4, 2), (a, a + 12, 4), (a + 12, a, 4)):     # itself; inside; one shared element, either order
        err(lib.qk_swap_f32(x, y, n, None), 'overlap')
    assert all(v == 0.0 for buf, _ in keep for v in buf)            # nothing was written


@pytest.mark.parametrize('kw', [
    dict(base_lr=0.0), dict(base_lr=-1.0), dict(base_lr=float('nan')), dict(base_lr='fast'), dict(kind='linear'),
    dict(kind='exponential', rate=0.0), dict(kind='inverse-time', rate=-1.0), dict(kind='exponential', rate=0.5, decay_steps=0),
    dict(kind='cosine', warmup_steps=10, total_steps=10), dict(kind='cosine', total_steps=0), dict(floor=1.01), dict(floor=-0.01),
    dict(warmup_steps=-1), dict(warmup_steps=2.5), dict(total_steps=True),
], ids=lambda kw: ','.join('%s=%s' % kv for kv in kw.items()))
def test_lr_schedule_refuses_bad_arguments_on_the_host(kw):
    from qcnn_amd.training import LRSchedule
    args = dict(base_lr=1e-3)
    args.update(kw)
    with pytest.raises(ValueError):
        LRSchedule(**args)


def test_reduce_on_plateau_sequences():
    from qcnn_amd.training import ReduceOnPlateau
    run = lambda p, xs: [p.update(x) for x in xs]
    # newbob: halve whenever the held-out metric does not improve
    assert run(ReduceOnPlateau(), [30.0, 28.0, 28.5, 27.0, 27.0, 27.1]) == [1.0, 1.0, 0.5, 0.5, 0.25, 0.125]
    # patience: two bad evaluations are tolerated, the third reduces and the count starts again; an improvement resets it
    assert run(ReduceOnPlateau(patience=2), [10, 11, 11, 11, 11, 11, 9, 11, 11, 11]) == [1, 1, 1, .5, .5, .5, .5, .5, .5, .25]
    # min_delta: an improvement of no more than min_delta does not count, and does not move the best value
    assert run(ReduceOnPlateau(min_delta=0.5), [10.0, 9.6, 9.5, 9.4, 8.8]) == [1.0, 0.5, 0.25, 0.25, 0.25]
    # min_scale floors the product
    assert run(ReduceOnPlateau(factor=0.1, min_scale=0.05), [1.0, 2.0, 2.0, 2.0]) == [1.0, 0.1, 0.05, 0.05]
    # mode='max' (an accuracy)
    assert run(ReduceOnPlateau(mode='max'), [0.5, 0.6, 0.6, 0.7, 0.65]) == [1.0, 1.0, 0.5, 0.5, 0.25]
    # a NaN is a bad evaluation, also as the first one
    assert run(ReduceOnPlateau(), [float('nan'), 5.0, float('nan'), 4.0]) == [0.5, 0.5, 0.25, 0.25]
    for kw in (dict(factor=1.0), dict(factor=0.0), dict(patience=-1), dict(patience=1.5), dict(min_delta=-1.0), dict(min_scale=0.0),
               dict(min_scale=2.0), dict(mode='best'), dict(factor=float('nan'))):
        with pytest.raises(ValueError):
            ReduceOnPlateau(**kw)


def test_reduce_on_plateau_state_dict_round_trip():
    from qcnn_amd.training import ReduceOnPlateau
    a = ReduceOnPlateau(patience=1)
    for x in (10.0, 11.0, 12.0, 13.0):
        a.update(x)
    assert a.state_dict() == dict(scale=0.5, best=10.0, bad=1)
    b = ReduceOnPlateau(patience=1)
    b.load_state_dict(a.state_dict())
    assert b.state_dict() == a.state_dict()
    assert [a.update(x) for x in (14.0, 9.0, 9.5, 9.5)] == [b.update(x) for x in (14.0, 9.0, 9.5, 9.5)] == [0.25, 0.25, 0.25, 0.125]
    fresh = ReduceOnPlateau()
    fresh.load_state_dict(ReduceOnPlateau().state_dict())            # best is None before the first metric
    assert fresh.update(3.0) == 1.0
    for d in (dict(scale=2.0, best=1.0, bad=0), dict(scale=1e-6, best=1.0, bad=0), dict(scale=0.5, best=1.0, bad=-1)):
        with pytest.raises(ValueError):
            fresh.load_state_dict(d)


# ---- GPU part ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def pool():
    """Seeded Gaussian host operands, shared and never written: parameters, a sequence of gradients, the l2 coefficients."""
    rng = np.random.RandomState(4321)
    n = max(SIZES)
    return dict(p=rng.randn(n).astype(np.float32), g=[rng.randn(n).astype(np.float32) for _ in range(3)],
                d=np.where(rng.rand(n) < 0.5, 2e-3, 0.0).astype(np.float32))


def _grad(pool, k, n):
    """Gradient number k: the three draws, then signed / scaled mixtures of them."""
    a, b = pool['g'][k % 3][:n], pool['g'][(k + 1) % 3][:n]
    return a if k < 3 else (a * np.float32(0.5 + 0.25 * (k % 4)) - b * np.float32(0.125 * (k // 3))).astype(np.float32)


class Bufs(object):
    """One set of optimiser buffers as VIEWS 0 and 1 elements into their allocations (4-byte alignment is the contract)."""
    OFFSETS = dict(p=0, g=1, m=1, v=0, d=1, ema=1)

    def __init__(self, dev, pool, n, with_decay, with_ema=False, new=None):
        from qcnn_amd import _lib
        new = new or (lambda *shape, **kw: torch.empty(*shape, **kw))
        self.n, self.raw = n, {}

        def view(name):
            self.raw[name] = new(n + 2, dtype=torch.float32, device=dev)
            return self.raw[name][self.OFFSETS[name]:self.OFFSETS[name] + n]
        self.p, self.g, self.m, self.v = view('p'), view('g'), view('m'), view('v')
        self.p.copy_(torch.tensor(pool['p'][:n]))
        self.g.zero_()
        self.m.zero_()
        self.v.zero_()
        self.d = self.ema = None
        if with_decay:
            self.d = view('d')
            self.d.copy_(torch.tensor(pool['d'][:n]))
        if with_ema:
            self.ema = view('ema')
            self.ema.copy_(self.p)
        self.t = torch.zeros(1, dtype=torch.int32, device=dev)
        self.raw['state'] = new(len(_lib.OPT_STATE), dtype=torch.float32, device=dev)
        self.state = self.raw['state']
        self.state[0:4] = torch.tensor([1.0, 0.0, 0.0, 0.0])

    def stats(self):
        h = self.state.cpu()
        return dict(lr_scale=float(h[0]), last_lr=np.float32(h[1].item()), last_ema_decay=np.float32(h[2].item()),
                    ema_updates=int(h.view(torch.int32)[3]), step=int(self.t))

    def named(self):
        out = dict(p=self.p, g=self.g, m=self.m, v=self.v, t=self.t, state=self.state[0:4])
        if self.ema is not None:
            out['ema'] = self.ema
        return out

    def set_grad(self, host):
        self.g.copy_(torch.tensor(host))

    def sync_from(self, other):
        for a, b in ((self.p, other.p), (self.g, other.g), (self.m, other.m), (self.v, other.v), (self.t, other.t)):
            a.copy_(b)


def _sched_step(b, sched, guard=None, grad_scale=1.0, zero_grad=False, ema_decay=0.0, ema_warmup=True):
    from qcnn_amd import functional as F
    if guard is not None:
        F.grad_guard_reduce(b.g, guard.config, guard._state, b.p if b.d is not None else None, b.d, grad_scale,
                            guard._workspace(b.n))
        grad_scale = 1.0
    F.adam_step_sched(b.p, b.g, b.m, b.v, b.t, sched.desc, b.state, guard_config=guard.config if guard is not None else None,
                      guard_state=guard._state if guard is not None else None, ema=b.ema, ema_decay=ema_decay, ema_warmup=ema_warmup,
                      grad_scale=grad_scale, zero_grad=zero_grad, decay=b.d, **ADAM)


def _assert_same(a, b, what, names=None):
    for name in names or a:
        assert torch.equal(_bits(a[name]), _bits(b[name])), '%s: %s differs' % (what, name)


COMBOS = [(False, False), (True, True)]                  # (decay, zero_grad) of the tests that do not cross them


@pytest.mark.gpu
@pytest.mark.parametrize('zero_grad', [False, True], ids=['keep_grad', 'zero_grad'])
@pytest.mark.parametrize('with_decay', [False, True], ids=['plain', 'decay'])
@pytest.mark.parametrize('n', SIZES)
def test_constant_schedule_is_bit_identical_to_the_existing_steps(pool, n, with_decay, zero_grad):
    from qcnn_amd import functional as F
    from qcnn_amd.training import GradGuard, LRSchedule
    dev = _dev()
    sched = LRSchedule(BASE_LR)
    names = ('p', 'm', 'v', 'g', 't')
    # without a guard: adam_step(step=<device tensor>)
    a, b = Bufs(dev, pool, n, with_decay), Bufs(dev, pool, n, with_decay)
    for k in range(3):
        a.set_grad(_grad(pool, k, n))
        b.set_grad(_grad(pool, k, n))
        _sched_step(a, sched, grad_scale=0.5, zero_grad=zero_grad)
        F.adam_step(b.p, b.g, b.m, b.v, b.t, lr=BASE_LR, grad_scale=0.5, zero_grad=zero_grad, decay=b.d, **ADAM)
        _assert_same(a.named(), b.named(), 'plain step %d' % (k + 1), names)
    s = a.stats()
    assert s['step'] == 3 and s['last_lr'] == np.float32(BASE_LR) and s['ema_updates'] == 0 and s['last_ema_decay'] == 0.0
    # with a guard that clips both ways under a static scale of 2^12: GradGuard.step
    kw = dict(clipnorm=0.3 * math.sqrt(n), clipvalue=1.0, loss_scale=2.0 ** 12)
    ga, gb = GradGuard(dev, **kw), GradGuard(dev, **kw)
    a, b = Bufs(dev, pool, n, with_decay), Bufs(dev, pool, n, with_decay)
    for k in range(3):
        big = (_grad(pool, k, n) * np.float32(4096.0)).astype(np.float32)
        a.set_grad(big)
        b.set_grad(big)
        _sched_step(a, sched, guard=ga, grad_scale=0.5, zero_grad=zero_grad)
        gb.step(b.p, b.g, b.m, b.v, b.t, lr=BASE_LR, grad_scale=0.5, zero_grad=zero_grad, decay=b.d, **ADAM)
        _assert_same(a.named(), b.named(), 'guarded step %d' % (k + 1), names)
        assert torch.equal(_bits(ga._state), _bits(gb._state))
    assert a.stats()['step'] == 3 and ga.stats()['last_skipped'] == 0
    assert n < 16 or ga.stats()['last_coef'] < 1.0          # (the norm clip did bite wherever the norm is about sqrt(n))


@pytest.mark.gpu
@pytest.mark.parametrize('kind', R.KINDS)
@pytest.mark.parametrize('n', SIZES)
def test_the_scheduled_rate_reaches_the_update(pool, n, kind):
    from qcnn_amd import functional as F
    from qcnn_amd.training import LRSchedule
    dev = _dev()
    kw = _sched_kw(kind, 3, 10)
    sched = LRSchedule(BASE_LR, kind, **kw)
    for with_decay, zero_grad in COMBOS:
        a, twin = Bufs(dev, pool, n, with_decay), Bufs(dev, pool, n, with_decay)
        seen = []
        for t in range(1, 13):
            a.set_grad(_grad(pool, t, n))
            twin.sync_from(a)
            _sched_step(a, sched, grad_scale=0.25, zero_grad=zero_grad)
            s = a.stats()
            want = R.lr_f32(kind, t, BASE_LR, **kw)
            assert s['step'] == t
            assert R.ulp_distance(s['last_lr'], want) <= 1, (kind, t, float(s['last_lr']), float(want))
            assert R.ulp_distance(s['last_lr'], sched.value(t)) <= 1, (kind, t, float(s['last_lr']), sched.value(t))
            F.adam_step(twin.p, twin.g, twin.m, twin.v, twin.t, lr=float(s['last_lr']), grad_scale=0.25, zero_grad=zero_grad,
                        decay=twin.d, **ADAM)
            _assert_same(a.named(), twin.named(), '%s step %d' % (kind, t), ('p', 'm', 'v', 'g', 't'))
            seen.append(float(s['last_lr']))
        assert seen[0] < seen[1] < seen[2]                       # the warm-up
        assert kind == 'constant' or seen[-1] < seen[2]          # ... and the decay


@pytest.mark.gpu
def test_lr_scale_multiplies_the_next_step_eagerly_and_in_a_captured_graph(pool):
    from qcnn_amd.training import LRSchedule, ScheduledAdam
    dev = _dev()
    n = 4099

    def fresh(kind, **kw):
        p = torch.tensor(pool['p'][:n], device=dev)
        return ScheduledAdam(p, torch.zeros_like(p), LRSchedule(BASE_LR, kind, **kw)), torch.tensor(pool['g'][0][:n], device=dev)
    opt, src = fresh('constant')
    assert opt.lr_scale.data_ptr() == opt._state.data_ptr() and opt.stats() == dict(step=0, last_lr=0.0, lr_scale=1.0, last_ema_decay=0.0, ema_updates=0)
    opt.grad.copy_(src)
    opt.step()
    first = opt.stats()['last_lr']
    assert first == float(np.float32(BASE_LR)) and float(opt.grad.abs().max()) == 0.0
    opt.set_lr_scale(0.5)
    opt.grad.copy_(src)
    opt.step()
    assert opt.stats()['last_lr'] == 0.5 * first and opt.stats()['lr_scale'] == 0.5 and opt.stats()['step'] == 2
    with pytest.raises(ValueError):
        opt.set_lr_scale(float('nan'))
    # a decaying schedule inside ONE captured graph: the fill between two replays is seen without re-capturing
    kw = dict(rate=0.05)
    eager, src = fresh('inverse-time', **kw)
    scales = [1.0, 1.0, 0.5, 0.5, 0.125]
    for s in scales:
        eager.set_lr_scale(s)
        eager.grad.copy_(src)
        eager.step()
    torch.cuda.synchronize()
    rep, src = fresh('inverse-time', **kw)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        rep.grad.copy_(src)
        rep.step()
    for t, s in enumerate(scales, 1):
        rep.set_lr_scale(s)
        graph.replay()
        got = np.float32(rep.stats()['last_lr'])
        assert R.ulp_distance(got, R.lr_f32('inverse-time', t, BASE_LR, s, **kw)) <= 1 and rep.stats()['step'] == t
        assert got == np.float32(rep.schedule.value(t, s)) or R.ulp_distance(got, rep.schedule.value(t, s)) == 1
    for name in ('param', 'm', 'v', 'grad', 'step_dev', '_state'):
        assert torch.equal(_bits(getattr(eager, name)), _bits(getattr(rep, name))), name


EMA_D = 0.375            # exactly representable; the warm-up (1 + u) / (10 + u) passes it between u = 4 (5/14) and u = 5 (6/15)


@pytest.mark.gpu
@pytest.mark.parametrize('n', SIZES)
def test_ema_follows_the_reference_one_step_at_a_time(pool, n):
    from qcnn_amd.training import LRSchedule
    dev = _dev()
    sched = LRSchedule(0.05, 'cosine', warmup_steps=2, total_steps=20)         # a rate that moves the weights visibly
    for (with_decay, zero_grad), warm in zip(COMBOS, (True, False)):
        a, plain = Bufs(dev, pool, n, with_decay, with_ema=True), Bufs(dev, pool, n, with_decay)
        worst = 0.0
        for u in range(1, 9):
            g = _grad(pool, u, n)
            a.set_grad(g)
            plain.set_grad(g)
            e_prev = a.ema.cpu().numpy().astype(np.float64)
            _sched_step(a, sched, zero_grad=zero_grad, ema_decay=EMA_D, ema_warmup=warm)
            _sched_step(plain, sched, zero_grad=zero_grad)
            _assert_same(a.named(), plain.named(), 'ema must not change the update, step %d' % u, ('p', 'm', 'v', 'g', 't'))
            d = R.ema_decay(u, EMA_D, warm)
            s = a.stats()
            assert s['ema_updates'] == u and s['last_ema_decay'] == np.float32(d), (u, s, d)
            p_new = a.p.cpu().numpy().astype(np.float64)
            want = R.ema_update(e_prev, p_new, d)
            err = np.abs(a.ema.cpu().numpy().astype(np.float64) - want)
            bound = 4.0 * 2.0 ** -24 * (np.abs(p_new) + np.abs(e_prev))
            worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
            assert (err <= bound).all(), (u, float(err.max()), int(np.argmax(err - bound)))
        print('n=%d warm=%s: worst error / bound %.3f' % (n, warm, worst))
        assert not torch.equal(_bits(a.ema), _bits(a.p))
        assert plain.stats()['ema_updates'] == 0 and plain.stats()['last_ema_decay'] == 0.0
        if warm:
            assert R.ema_decay(4, EMA_D) < EMA_D == R.ema_decay(5, EMA_D)        # both branches of the min were taken


@pytest.mark.gpu
@pytest.mark.parametrize('n', SIZES)
def test_a_skipped_step_changes_nothing_but_the_gradient_and_the_scale(pool, n):
    from qcnn_amd.training import GradGuard, LRSchedule
    dev = _dev()
    kw = dict(rate=0.05, warmup_steps=2)
    sched = LRSchedule(BASE_LR, 'inverse-time', **kw)
    for with_decay, zero_grad in COMBOS:
        guard = GradGuard(dev, loss_scale=1024.0, dynamic=True, clipnorm=5.0 * math.sqrt(n))
        a = Bufs(dev, pool, n, with_decay, with_ema=True)
        for k in range(2):
            a.set_grad(_grad(pool, k, n) * np.float32(1024.0))
            _sched_step(a, sched, guard=guard, zero_grad=zero_grad, ema_decay=EMA_D)
        assert a.stats()['step'] == 2 and a.stats()['ema_updates'] == 2 and guard.stats()['scale'] == 1024.0
        before = {k: _bits(v) for k, v in a.named().items()}
        reserved = _bits(a.state[4:8])
        bad = _grad(pool, 2, n) * np.float32(1024.0)
        bad[n // 2] = np.inf
        a.set_grad(bad)
        _sched_step(a, sched, guard=guard, zero_grad=zero_grad, ema_decay=EMA_D)
        after = a.named()
        for name in ('p', 'm', 'v', 'ema', 't', 'state'):
            assert torch.equal(before[name], _bits(after[name])), 'the skipped step changed %s' % name
        assert torch.equal(reserved, _bits(a.state[4:8]))
        if zero_grad:
            assert float(a.g.abs().max()) == 0.0
        else:
            assert torch.equal(_bits(a.g), _bits(torch.tensor(bad)))
        gs = guard.stats()
        assert gs['last_skipped'] == 1 and gs['skipped_steps'] == 1 and gs['scale'] == 512.0
        # the following finite step is step 3 of the schedule, not step 4
        a.set_grad(_grad(pool, 3, n) * np.float32(512.0))
        _sched_step(a, sched, guard=guard, zero_grad=zero_grad, ema_decay=EMA_D)
        s = a.stats()
        assert s['step'] == 3 and s['ema_updates'] == 3 and guard.stats()['last_skipped'] == 0
        assert R.ulp_distance(s['last_lr'], R.lr_f32('inverse-time', 3, BASE_LR, **kw)) <= 1
        assert R.ulp_distance(s['last_lr'], R.lr_f32('inverse-time', 4, BASE_LR, **kw)) > 1000
        assert s['last_ema_decay'] == np.float32(R.ema_decay(3, EMA_D))


@pytest.mark.gpu
def test_guard_schedule_and_ema_replay_in_one_captured_graph(pool):
    """copy static source -> grad, guard reduce + scheduled step (cosine with warm-up, EMA) as ONE captured linear graph, replayed
    over six sources of which the third holds an inf: bit-equal to the eager sequence in every buffer and both state blocks."""
    from qcnn_amd.training import GradGuard, LRSchedule, ScheduledAdam
    dev = _dev()
    n = 10007
    rng = np.random.RandomState(77)
    p0 = rng.randn(n).astype(np.float32)
    d0 = np.where(rng.rand(n) < 0.5, 2e-3, 0.0).astype(np.float32)
    sources = [(rng.randn(n) * 64).astype(np.float32) for _ in range(6)]
    sources[2][5000] = np.inf

    def fresh():
        p = torch.tensor(p0, device=dev)
        guard = GradGuard(dev, loss_scale=64.0, dynamic=True, growth_interval=2, clipnorm=30.0)
        opt = ScheduledAdam(p, torch.zeros_like(p), LRSchedule(BASE_LR, 'cosine', warmup_steps=3, total_steps=10, floor=0.1), guard=guard,
                            ema_decay=0.9, decay=torch.tensor(d0, device=dev))
        return opt, torch.zeros_like(p)

    def body(opt, src):
        opt.grad.copy_(src)
        opt.step(zero_grad=True)

    eager, src = fresh()
    for s in sources:
        src.copy_(torch.tensor(s, device=dev))
        body(eager, src)
    torch.cuda.synchronize()
    rep, src = fresh()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        body(rep, src)
    rates = []
    for s in sources:
        src.copy_(torch.tensor(s, device=dev))
        graph.replay()
        rates.append(rep.stats()['last_lr'])
    torch.cuda.synchronize()
    for name in ('param', 'grad', 'm', 'v', 'ema', 'step_dev', '_state'):
        assert torch.equal(_bits(getattr(eager, name)), _bits(getattr(rep, name))), name
    assert torch.equal(_bits(eager.guard._state), _bits(rep.guard._state))
    assert rates[2] == rates[1], 'the skipped replay must leave last_lr alone'
    applied = rates[:2] + rates[3:]
    assert len(set(applied)) == 5, rates                       # last_lr differs from replay to replay
    assert [R.ulp_distance(r, R.lr_f32('cosine', t, BASE_LR, warmup_steps=3, total_steps=10, floor=0.1)) <= 1
            for t, r in enumerate(applied, 1)] == [True] * 5
    s = rep.stats()
    assert s['step'] == 5 and s['ema_updates'] == 5 and rep.guard.stats()['skipped_steps'] == 1


def _conv_layer(dev, seed):
    """A bf16 channels-last QuaternionConv2D, 16 -> 16 quaternion channels (on the 16-bit matrix-core path: its kernel's 16-bit
    image is cached on the parameter), its parameters re-homed into one dp.FlatParams buffer."""
    from qcnn_amd import dp
    from qcnn_amd.complexnn import QuaternionConv2D
    np.random.seed(seed)
    layer = QuaternionConv2D(16, (3, 3), padding='same')
    x = torch.tensor(np.random.RandomState(seed + 1).randn(2, 8, 8, 64).astype(np.float32), device=dev).to(torch.bfloat16)
    with torch.no_grad():
        layer(x)
    flat = dp.FlatParams([q for q in layer.parameters() if q.requires_grad], direct=True)
    return layer, flat, x


def _train_step(layer, x, opt, scale=None):
    y = layer(x)
    loss = (y.float() ** 2).mean()
    (loss if scale is None else loss * scale).backward()
    opt.step()


@pytest.mark.gpu
def test_averaged_swaps_the_weights_in_and_out_and_refreshes_the_16_bit_images():
    from qcnn_amd.training import LRSchedule, ScheduledAdam
    dev = _dev()
    layer, flat, x = _conv_layer(dev, 11)
    opt = ScheduledAdam(flat.param, flat.grad, LRSchedule(2e-2, warmup_steps=2), ema_decay=0.9)
    for _ in range(4):
        _train_step(layer, x, opt)
    assert layer.kernel.__dict__.get('_qk_prep'), 'the prepped 16-bit kernel cache is not in play'
    with torch.no_grad():
        y_before = layer(x).clone()
    p_bits, e_bits = _bits(flat.param), _bits(opt.ema)
    assert not torch.equal(p_bits, e_bits)
    with opt.averaged():
        assert torch.equal(_bits(flat.param), e_bits) and torch.equal(_bits(opt.ema), p_bits)
        with torch.no_grad():
            y_avg = layer(x).clone()
        other, _, _ = _conv_layer(dev, 12)
        with torch.no_grad():
            other.kernel.copy_(layer.kernel)
            other.bias.copy_(layer.bias)
            y_fresh = other(x)
        assert torch.equal(y_avg.view(torch.int16).cpu(), y_fresh.view(torch.int16).cpu())
        assert not torch.equal(y_avg.view(torch.int16).cpu(), y_before.view(torch.int16).cpu())
        with pytest.raises(RuntimeError, match='averaged'):
            opt.step()
        with pytest.raises(RuntimeError, match='averaged'):
            opt.state_dict()
    assert torch.equal(_bits(flat.param), p_bits) and torch.equal(_bits(opt.ema), e_bits)
    with torch.no_grad():
        assert torch.equal(layer(x).view(torch.int16).cpu(), y_before.view(torch.int16).cpu())
    with pytest.raises(KeyError):
        with opt.averaged():
            raise KeyError('inside')
    assert torch.equal(_bits(flat.param), p_bits) and torch.equal(_bits(opt.ema), e_bits)
    with torch.no_grad():
        assert torch.equal(layer(x).view(torch.int16).cpu(), y_before.view(torch.int16).cpu())
    _train_step(layer, x, opt)                                   # and the optimiser steps again
    assert opt.stats()['step'] == 5
    with pytest.raises(RuntimeError, match='ema_decay'):
        with ScheduledAdam(flat.param, flat.grad, LRSchedule(1e-3)).averaged():
            pass


@pytest.mark.gpu
def test_checkpoint_resumes_bit_for_bit(tmp_path):
    from qcnn_amd import features
    from qcnn_amd.training import GradGuard, LRSchedule, ScheduledAdam, load_checkpoint, save_checkpoint
    dev = _dev()
    layer, flat, x = _conv_layer(dev, 21)
    sched_kw = dict(kind='cosine', warmup_steps=2, total_steps=9, floor=0.1)
    guard = GradGuard(dev, loss_scale=16.0, dynamic=True, clipnorm=10.0)
    opt = ScheduledAdam(flat.param, flat.grad, LRSchedule(1e-2, **sched_kw), guard=guard, ema_decay=0.9)
    aug = features.SpecAugment(seed=3)
    spec = torch.tensor(np.random.RandomState(5).randn(2, 4, 41, 40).astype(np.float32), device=dev)
    lengths = torch.tensor([40, 33], dtype=torch.int32, device=dev)
    for _ in range(3):
        aug(spec, lengths)
        _train_step(layer, x, opt, guard.loss_scale)
    path = str(tmp_path / 'ckpt.pt')
    save_checkpoint(path, layer, opt, policies=[aug], extra=dict(epoch=7, plateau=dict(scale=0.5, best=31.5, bad=0)))
    raw = torch.load(path, map_location='cpu', weights_only=True)             # plain tensors and numbers only
    assert set(raw) == {'model', 'optimizer', 'policies', 'extra'} and raw['optimizer']['step'] == 3
    with torch.no_grad():
        y_save = layer(x).clone()
    rng = np.random.RandomState(9)
    recorded = [torch.tensor((rng.randn(flat.numel) * 16).astype(np.float32), device=dev) for _ in range(2)]

    def continuation():
        for g in recorded:
            flat.grad.copy_(g)
            opt.step()
        out = {k: _bits(t) for k, t in dict(param=flat.param, grad=flat.grad, m=opt.m, v=opt.v, ema=opt.ema, step=opt.step_dev,
                                            opt_state=opt._state, guard_state=guard._state).items()}
        out['augmented'] = _bits(aug(spec, lengths))
        return out, aug.state_dict()
    first, first_policy = continuation()
    assert first_policy == dict(seed=3, counter=4)
    # scramble everything the checkpoint has to restore, and leave stale 16-bit images behind
    with torch.no_grad():
        flat.param.normal_()
        for t in (opt.m, opt.v, opt.ema):
            t.normal_()
        opt.step_dev.fill_(77)
        opt._state[0:4] = torch.tensor([0.25, 9.0, 0.5, 0.0], device=dev)
        guard.loss_scale.fill_(2.0)
        aug(spec, lengths)
        layer(x)
    extra = load_checkpoint(path, layer, opt, policies=[aug])
    assert extra == dict(epoch=7, plateau=dict(scale=0.5, best=31.5, bad=0))
    with torch.no_grad():
        assert torch.equal(layer(x).view(torch.int16).cpu(), y_save.view(torch.int16).cpu())
    assert opt.stats()['step'] == 3 and guard.stats()['scale'] == 16.0 and aug.state_dict() == dict(seed=3, counter=3)
    second, second_policy = continuation()
    assert second_policy == first_policy
    for name in first:
        assert torch.equal(first[name], second[name]), name
    other = ScheduledAdam(flat.param, flat.grad, LRSchedule(1e-2, **dict(sched_kw, total_steps=10)), guard=guard, ema_decay=0.9)
    with pytest.raises(ValueError, match='schedule'):
        load_checkpoint(path, layer, other, policies=[aug])


@pytest.mark.gpu
def test_train_timit_example_with_schedule_ema_plateau_and_resume(tmp_path):
    """The example on a three-utterance tree: every new flag at once, a checkpoint at the evaluation of step 2, and a second process
    that resumes from it and runs step 3."""
    import subprocess
    import sys
    from qcnn_amd import data
    from test_fbank import signals, sphere_bytes
    _dev()
    rng = np.random.RandomState(0)
    tree = tmp_path / 'timit'
    for split, spk, utt in (('TRAIN', 'FCJF0', 'SA1'), ('TRAIN', 'MDAB0', 'SX9'), ('TEST', 'MDAB1', 'SI2')):
        d = tree / split / 'DR1' / spk
        d.mkdir(parents=True, exist_ok=True)
        n = int(rng.randint(14000, 20000))
        (d / (utt + '.WAV')).write_bytes(sphere_bytes(signals([n], seed=int(rng.randint(1000)))[0].astype(np.int16)))
        phones = [data.TIMIT_PHONES_61[i] for i in rng.randint(0, 61, size=12)]
        cuts = np.linspace(0, n, len(phones) + 1).astype(int)
        (d / (utt + '.PHN')).write_text(''.join('%d %d %s\n' % (cuts[i], cuts[i + 1], p) for i, p in enumerate(phones)))
    ckpt = str(tmp_path / 'run.pt')
    common = [sys.executable, os.path.join(ROOT, 'examples', 'train_timit.py'), '--timit', str(tree), '--layers', '4', '--batch', '2',
              '--eval-every', '1', '--specaug', '--clipnorm', '5', '--warmup', '2', '--lr-decay', 'exponential', '--decay-steps', '2', '--ema', '0.9',
              '--halve-on-plateau', '--checkpoint', ckpt]

    def run(extra):
        r = subprocess.run(common + extra, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, env=dict(os.environ), timeout=600,
                           universal_newlines=True)
        assert r.returncode == 0, r.stdout[-4000:]
        return r.stdout
    out = run(['--steps', '2'])
    rates = [float(v) for v in re.findall(r'step\s+\d+\s+loss \S+ .*?  lr (\S+)', out)]
    assert len(rates) == 2 and 0 < rates[0] < rates[1], out[-4000:]              # the warm-up shows in the log lines
    assert len(re.findall(r'held-out ctc cost \S+ .*\[averaged weights, ema 0.9\]', out)) == 2, out[-4000:]
    assert len(re.findall(r'learning-rate scale (\S+)', out)) == 2
    saved = torch.load(ckpt, map_location='cpu', weights_only=True)
    assert saved['extra']['step'] == 2 and saved['optimizer']['step'] == 2 and saved['policies'] == [dict(seed=0, counter=2)]
    out = run(['--steps', '3', '--resume', ckpt])
    assert 'resumed from' in out and re.findall(r'step\s+(\d+)\s+loss', out) == ['3'], out[-4000:]
    saved = torch.load(ckpt, map_location='cpu', weights_only=True)
    assert saved['extra']['step'] == 3 and saved['optimizer']['step'] == 3 and saved['policies'] == [dict(seed=0, counter=3)]


# every entry of OPT_SYMBOLS against the hygiene case that exercises it, or the reason it has none
HYGIENE_COVER = {
    'qk_adam_step_sched': 'test_new_entry_points_keep_to_their_buffers: plain, guard, ema, guard+ema',
    'qk_swap_f32': 'test_new_entry_points_keep_to_their_buffers: swap_ twice',
    'qk_lr_schedule_value': 'host only: takes no device buffer (test_schedule_value_matches_the_reference)',
}


def test_every_opt_entry_point_has_a_hygiene_case_or_a_reason():
    from qcnn_amd import _lib
    assert set(HYGIENE_COVER) == set(_lib.OPT_SYMBOLS)


@pytest.mark.gpu
@pytest.mark.parametrize('zero_grad', [False, True], ids=['keep_grad', 'zero_grad'])
@pytest.mark.parametrize('with_decay', [False, True], ids=['plain', 'decay'])
@pytest.mark.parametrize('n', SIZES)
def test_new_entry_points_keep_to_their_buffers(pool, n, with_decay, zero_grad):
    """Guarded payloads under two fills; every buffer is a view 0 or 1 elements into its payload.  Guard bands, the fill in front of
    and behind each view and the reserved words of the state block must survive; the two runs must agree bit for bit."""
    from qcnn_amd import functional as F
    from qcnn_amd.training import GradGuard, LRSchedule
    dev = _dev()
    sched = LRSchedule(BASE_LR, 'exponential', rate=0.9, decay_steps=2, warmup_steps=2)
    runs = []
    for fill in (GA.FILL_A, GA.FILL_B):
        alloc = GA.GuardedAllocator(fill)
        out = {}
        for case, (use_guard, use_ema) in dict(plain=(False, False), guard=(True, False), ema=(False, True), both=(True, True)).items():
            b = Bufs(dev, pool, n, with_decay, with_ema=use_ema, new=alloc.empty)
            guard = GradGuard(dev, clipnorm=0.3 * math.sqrt(n), loss_scale=8.0) if use_guard else None
            for k in range(2):
                b.set_grad(_grad(pool, k, n) * np.float32(8.0 if use_guard else 1.0))
                _sched_step(b, sched, guard=guard, grad_scale=0.5, zero_grad=zero_grad, ema_decay=EMA_D)
            assert b.stats()['step'] == 2
            for name, raw in b.raw.items():
                image = raw.view(torch.uint8).cpu().numpy()
                if name == 'state':
                    assert (image[16:] == fill).all(), '%s: the reserved words 4-7 of the state block were written' % case
                    continue
                off = 4 * Bufs.OFFSETS[name]
                assert (image[:off] == fill).all() and (image[off + 4 * n:] == fill).all(), \
                    '%s: %s was written outside its view' % (case, name)
            out.update({'%s_%s' % (case, k): v for k, v in b.named().items()})
        # swap_: twice restores both buffers
        x, y = alloc.empty(n + 2, dtype=torch.float32, device=dev), alloc.empty(n + 2, dtype=torch.float32, device=dev)
        xv, yv = x[1:1 + n], y[0:n]
        xv.copy_(torch.tensor(pool['p'][:n]))
        yv.copy_(torch.tensor(pool['g'][0][:n]))
        x0, y0 = _bits(xv), _bits(yv)
        F.swap_(xv, yv)
        assert torch.equal(_bits(xv), y0) and torch.equal(_bits(yv), x0)
        out.update(swap_x=xv.clone(), swap_y=yv.clone())
        F.swap_(xv, yv)
        assert torch.equal(_bits(xv), x0) and torch.equal(_bits(yv), y0)
        for raw, off in ((x, 4), (y, 0)):
            image = raw.view(torch.uint8).cpu().numpy()
            assert (image[:off] == fill).all() and (image[off + 4 * n:] == fill).all(), 'swap_ wrote outside its views'
        GA.check_guards(alloc, 'n=%d fill 0x%02X: ' % (n, fill))
        assert alloc.log
        runs.append(out)
    for name in runs[0]:
        assert GA.first_bit_difference(runs[0][name], runs[1][name]) is None, name
    with pytest.raises(RuntimeError, match='overlap'):
        F.swap_(x[0:n], x[1:1 + n]) if n > 1 else F.swap_(x[0:1], x[0:1])
