"""The guarded optimiser step (include/qk.h "Guarded optimiser step", qcnn_amd.training.GradGuard): gradient clipping, overflow skip
and dynamic loss scaling on the device, against the float64 restatement of tests/grad_guard_ref.py.

Tolerances.  Norm: 1e-6 relative -- the squares are summed in float64, so what is left is the float32 rounding of each element
(2^-24 relative each, averaging out over the sum) and of the result: about 2e-7.  Clip coefficient: 1e-6 relative (clipnorm / norm,
one more float32 rounding).  Parameters / first moment after three steps: 1e-5 / 1e-6 absolute, the bounds of
test_adam_step_matches_keras_formula.  Everything the guard must NOT change is compared bit for bit.
"""
import ctypes
import math

import numpy as np
import pytest
import torch

from grad_guard_ref import GuardRef, clip_coef, norm_and_nonfinite

# stage one of the reduction runs at most 2048 workgroups of 256 threads x 4 elements per pass (csrc/qk_train.hip): beyond
# 2048 * 1024 elements every workgroup takes a second trip through its grid-stride loop; this size makes it two full trips and a
# partial third, with n % 4 == 3
N_MULTI_PASS = 2 * 2048 * 1024 + 4099
SIZES = [1, 63, 64, 255, 256, 257, 4099, 262147, N_MULTI_PASS]
_PAD = 8


def _dev():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    return torch.device('cuda:0')


# ---- CPU part ------------------------------------------------------------------------------------------------------------------
def test_reference_three_element_clip():
    g = np.array([3.0, 4.0, 12.0])
    assert norm_and_nonfinite(g) == (13.0, 0)
    ref = GuardRef(clipnorm=6.5)
    d = ref.reduce(g)
    assert d['last_norm'] == 13.0 and d['last_coef'] == 0.5 and d['last_skipped'] == 0 and d['last_unscale'] == 1.0
    assert clip_coef(13.0, 13.0) == 1.0 and clip_coef(13.0, 0.0) == 1.0 and clip_coef(13.0, 26.0) == 1.0
    # first Adam step of p = 0 with m = v = 0: p = -lr * g / (|g| + eps') -> -lr * sign(g) up to eps
    p, m, v, t = ref.step(np.zeros(3), g.copy(), np.zeros(3), np.zeros(3), 0, lr=0.1, eps=0.0)
    assert t == 1 and np.allclose(m, 0.1 * 0.5 * g, rtol=1e-15) and np.allclose(p, -0.1, rtol=1e-12)
    # clipvalue after clipnorm: 0.5 * g = [1.5, 2, 6] clamped to 1.75
    ref = GuardRef(clipnorm=6.5, clipvalue=1.75)
    _, m, _, _ = ref.step(np.zeros(3), g.copy(), np.zeros(3), np.zeros(3), 0)
    assert np.allclose(m, 0.1 * np.array([1.5, 1.75, 1.75]), rtol=1e-15)


def test_reference_skip():
    ref = GuardRef(loss_scale=8.0, dynamic=True)
    g = np.array([1.0, np.inf, 2.0])
    p0, m0, v0 = np.array([1.0, 2.0, 3.0]), np.full(3, 0.5), np.full(3, 0.25)
    p, m, v, t = ref.step(p0, g, m0, v0, 7, zero_grad=True)
    s = ref.stats()
    assert t == 7 and p is p0 and m is m0 and v is v0 and not g.any()
    assert s['last_skipped'] == 1 and s['nonfinite_count'] == 1 and s['last_norm'] == float('inf')
    assert s['scale'] == 4.0 and s['good_steps'] == 0 and s['skipped_steps'] == 1 and s['last_unscale'] == 0.125
    assert GuardRef().reduce(np.array([np.nan, 1.0, np.nan]))['nonfinite_count'] == 2
    # without `dynamic` the step is skipped all the same, the scale stays
    ref = GuardRef(loss_scale=8.0)
    assert ref.reduce(g + np.inf)['last_skipped'] == 1 and ref.stats()['scale'] == 8.0 and ref.stats()['skipped_steps'] == 0


def test_reference_growth_exactly_at_the_interval():
    ref = GuardRef(loss_scale=8.0, dynamic=True, growth_interval=3)
    g = np.ones(4)
    seen = []
    for _ in range(7):
        ref.reduce(g)
        seen.append((ref.stats()['scale'], ref.stats()['good_steps']))
    assert seen == [(8.0, 1), (8.0, 2), (16.0, 0), (16.0, 1), (16.0, 2), (32.0, 0), (32.0, 1)]


def test_reference_backoff_floor_and_growth_cap():
    ref = GuardRef(loss_scale=2.0, dynamic=True, backoff_factor=0.25, min_scale=1.0)
    ref.reduce(np.array([np.inf]))
    assert ref.stats()['scale'] == 1.0 and ref.stats()['skipped_steps'] == 1
    ref.reduce(np.array([np.nan]))
    assert ref.stats()['scale'] == 1.0 and ref.stats()['skipped_steps'] == 2
    ref = GuardRef(loss_scale=12.0, dynamic=True, growth_interval=1, max_scale=16.0)
    ref.reduce(np.ones(2))
    assert ref.stats()['scale'] == 16.0
    ref.reduce(np.ones(2))
    assert ref.stats()['scale'] == 16.0 and ref.stats()['good_steps'] == 0


def test_reference_norm_matches_torch_float64():
    rng = np.random.RandomState(3)
    g = rng.randn(4099) * 10.0 ** rng.uniform(-6, 3, 4099)
    p, d = rng.randn(4099), rng.choice([0.0, 0.5, 1.0], 4099)
    want = float(torch.linalg.vector_norm(torch.tensor(g, dtype=torch.float64) * 0.125))
    assert abs(norm_and_nonfinite(g, 0.125)[0] - want) <= 1e-12 * want
    want = float(torch.linalg.vector_norm(torch.tensor(g * 0.125 + d * p, dtype=torch.float64)))
    assert abs(norm_and_nonfinite(g, 0.125, p, d)[0] - want) <= 1e-12 * want


@pytest.mark.parametrize('kw', [
    dict(clipnorm=-1.0), dict(clipvalue=-0.5), dict(clipnorm=float('nan')), dict(clipvalue=float('inf')),
    dict(backoff_factor=0.0), dict(backoff_factor=1.0), dict(backoff_factor=1.5), dict(growth_factor=1.0), dict(growth_factor=0.5),
    dict(growth_interval=0), dict(growth_interval=2.5), dict(min_scale=0.0), dict(min_scale=-1.0),
    dict(loss_scale=0.5), dict(loss_scale=2.0 ** 25), dict(min_scale=4.0, loss_scale=2.0), dict(max_scale=0.5),
    dict(loss_scale=float('inf'), max_scale=float('inf')), dict(loss_scale='big'),
], ids=lambda kw: ','.join('%s=%s' % kv for kv in kw.items()))
def test_grad_guard_refuses_bad_hyper_parameters_before_any_device_use(kw):
    from qcnn_amd.training import GradGuard
    with pytest.raises(ValueError):
        GradGuard(torch.device('cuda:0'), **kw)         # raised on the host: no GPU is needed to get here


def test_library_exports_the_guard_symbols_and_keeps_its_version():
    from qcnn_amd import _lib
    lib = _lib.lib()
    for name in ('qk_grad_guard_workspace_bytes', 'qk_grad_guard_reduce', 'qk_adam_step_guarded'):
        assert name in _lib.SYMBOLS and getattr(lib, name) is not None
    assert lib.qk_version() == 103
    assert ctypes.sizeof(_lib.GradGuardConfig) == 32 and len(_lib.GRAD_GUARD_STATE) == 8


def test_workspace_bytes_is_positive_and_non_decreasing():
    from qcnn_amd import _lib
    f = _lib.lib().qk_grad_guard_workspace_bytes
    ns = sorted(set([1, 2, 3, 1023, 1024, 1025] + [2 ** k + d for k in range(1, 25) for d in (-1, 0, 1)]))
    assert ns[0] == 1 and ns[-1] == 2 ** 24 + 1
    got = [int(f(n)) for n in ns if n <= 2 ** 24]
    assert got[0] > 0 and all(b >= a for a, b in zip(got, got[1:]))


# ---- GPU part ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def pool():
    """One set of host arrays (float64 views for the reference) and their device copies, shared by the reduction cases and never
    written: gradient = standard normal x 10^U(-6, 3); the parameters have the same spread and the coefficients are 0 / 0.5 / 1, so
    that the decay term weighs as much in the norm as the gradient does."""
    dev = _dev()
    rng = np.random.RandomState(1234)
    n = N_MULTI_PASS + _PAD
    g = (rng.randn(n) * 10.0 ** rng.uniform(-6, 3, n)).astype(np.float32)
    p = (rng.randn(n) * 10.0 ** rng.uniform(-6, 3, n)).astype(np.float32)
    d = rng.choice(np.array([0.0, 0.5, 1.0], np.float32), n)
    host = dict(g=g.astype(np.float64), p=p.astype(np.float64), d=d.astype(np.float64))
    return host, dict(g=torch.tensor(g, device=dev), p=torch.tensor(p, device=dev), d=torch.tensor(d, device=dev))


def _bits(t):
    return t.detach().contiguous().view(torch.int32).cpu()


@pytest.mark.gpu
@pytest.mark.parametrize('n', SIZES)
def test_reduce_matches_the_reference(pool, n):
    from qcnn_amd import functional as F
    host, dv = pool
    for off in (0, 1, 3):
        # (offset of param, offset of decay): the gradient's own -- one flat layout, 16-byte loads -- and two others, which
        # takes the element-wise reads of param / decay
        for pd in (None, (off, off), (off + 1, off + 2)):
            for gs in (1.0, 0.125):
                g = dv['g'][off:off + n]
                kw = {}
                if pd is not None:
                    kw = dict(param=dv['p'][pd[0]:pd[0] + n], decay=dv['d'][pd[1]:pd[1] + n])
                norm, bad = F.grad_norm(g, grad_scale=gs, **kw)
                norm2, bad2 = F.grad_norm(g, grad_scale=gs, **kw)
                if pd is None:
                    want, _ = norm_and_nonfinite(host['g'][off:off + n], gs)
                else:
                    want, _ = norm_and_nonfinite(host['g'][off:off + n], gs, host['p'][pd[0]:pd[0] + n], host['d'][pd[1]:pd[1] + n])
                got = float(norm)
                print('n=%d off=%d pd=%s gs=%g: norm %.9g want %.9g rel %.3g' % (n, off, pd, gs, got, want, abs(got - want) / want))
                assert int(bad) == 0 and int(bad2) == 0
                assert abs(got - want) <= 1e-6 * want, (n, off, pd, gs, got, want)
                assert torch.equal(_bits(norm), _bits(norm2)), 'two reductions of one input differ in their bits'


@pytest.mark.gpu
def test_reduce_large_finite_elements_do_not_overflow_the_sum():
    from qcnn_amd import functional as F
    dev = _dev()
    n = 4099
    g = torch.full((n,), 1e25, device=dev)
    norm, bad = F.grad_norm(g)
    want = float(np.float32(1e25)) * math.sqrt(n)
    assert int(bad) == 0 and math.isfinite(float(norm)) and abs(float(norm) - want) <= 1e-6 * want


@pytest.mark.gpu
@pytest.mark.parametrize('value', [float('inf'), float('-inf'), float('nan')], ids=['inf', '-inf', 'nan'])
def test_reduce_counts_one_non_finite_element_wherever_it_sits(pool, value):
    from qcnn_amd import functional as F
    _, dv = pool
    n = 4099                                   # n % 4 == 3
    for off in (0, 1):                         # 16-byte aligned; three head elements, whole float4s behind them, no tail
        for where in (0, n - 1, n - 2, 2, 2048):       # first, last, inside the n % 4 tail (off = 0) / the peeled head (off = 1), body
            g = dv['g'][off:off + n].clone()
            buf = torch.empty(n + 4, device=g.device)
            view = buf[off:off + n]
            view.copy_(g)
            view[where] = value
            norm, bad = F.grad_norm(view)
            assert int(bad) == 1 and float(norm) == float('inf'), (off, where, int(bad), float(norm))
            norm, bad = F.grad_norm(view, param=dv['p'][off:off + n], decay=dv['d'][off:off + n], grad_scale=0.125)
            assert int(bad) == 1 and float(norm) == float('inf'), (off, where, int(bad), float(norm))


def _buffers(dev, n, seed, with_decay):
    rng = np.random.RandomState(seed)
    p, g = rng.randn(n).astype(np.float32), rng.randn(n).astype(np.float32)
    d = np.where(rng.rand(n) < 0.5, 2e-3, 0.0).astype(np.float32) if with_decay else None
    return p, g, d


def _run_steps(dev, p, grads, d, stepper, zero_grad=False):
    """Three (len(grads)) optimiser steps on fresh device buffers; stepper(tp, tg, tm, tv, tstep, decay)."""
    tp = torch.tensor(p, device=dev)
    tg = torch.empty_like(tp)
    tm, tv = torch.zeros_like(tp), torch.zeros_like(tp)
    tstep = torch.zeros(1, dtype=torch.int32, device=dev)
    td = torch.tensor(d, device=dev) if d is not None else None
    for g in grads:
        tg.copy_(torch.tensor(g, device=dev))
        stepper(tp, tg, tm, tv, tstep, td)
    return tp, tm, tv, tstep


ADAM = dict(lr=5e-4, beta1=0.9, beta2=0.999, eps=1e-7)


@pytest.mark.gpu
@pytest.mark.parametrize('with_decay', [False, True], ids=['plain', 'decay'])
def test_inert_guard_is_bit_identical_to_adam_step(with_decay):
    from qcnn_amd import functional as F
    from qcnn_amd.training import GradGuard
    dev = _dev()
    n = 10007
    p, g, d = _buffers(dev, n, 0, with_decay)
    grads = [g, (0.5 * g[::-1]).copy(), (g * g).astype(np.float32)]
    want = _run_steps(dev, p, grads, d, lambda tp, tg, tm, tv, ts, td: F.adam_step(tp, tg, tm, tv, ts, grad_scale=0.5, decay=td, **ADAM))
    guard = GradGuard(dev)
    got = _run_steps(dev, p, grads, d, lambda tp, tg, tm, tv, ts, td: guard.step(tp, tg, tm, tv, ts, grad_scale=0.5, decay=td, **ADAM))
    for a, b, name in zip(got, want, 'pmvt'):
        assert torch.equal(_bits(a), _bits(b)), name
    assert int(got[3]) == 3 and guard.stats()['last_skipped'] == 0 and guard.stats()['last_coef'] == 1.0
    # the same gradients x 2^12 under loss_scale = 2^12: the unscaling is exact
    guard = GradGuard(dev, loss_scale=2.0 ** 12)
    big = [(x * np.float32(4096.0)).astype(np.float32) for x in grads]
    got = _run_steps(dev, p, big, d, lambda tp, tg, tm, tv, ts, td: guard.step(tp, tg, tm, tv, ts, grad_scale=0.5, decay=td, **ADAM))
    for a, b, name in zip(got, want, 'pmvt'):
        assert torch.equal(_bits(a), _bits(b)), 'loss_scale 2^12: ' + name
    assert guard.stats()['scale'] == 4096.0 and guard.stats()['last_unscale'] == 0.5 / 4096.0


@pytest.mark.gpu
@pytest.mark.parametrize('with_decay', [False, True], ids=['plain', 'decay'])
def test_clipping_matches_the_reference(with_decay):
    from qcnn_amd.training import GradGuard
    dev = _dev()
    n = 10007
    p, g, d = _buffers(dev, n, 1, with_decay)
    grads = [g, (0.5 * g[::-1]).copy(), (g * g).astype(np.float32)]
    d64 = d.astype(np.float64) if d is not None else None
    norm0, _ = norm_and_nonfinite(g, 1.0, p if with_decay else None, d64)          # ~ sqrt(n) = 100
    for kw in (dict(clipnorm=0.3 * norm0), dict(clipnorm=0.3 * norm0, clipvalue=0.2), dict(clipvalue=0.7)):
        guard, ref = GradGuard(dev, **kw), GuardRef(**kw)
        p64, m64, v64, t = p.astype(np.float64), np.zeros(n), np.zeros(n), 0
        coefs = []

        def stepper(tp, tg, tm, tv, ts, td):
            guard.step(tp, tg, tm, tv, ts, decay=td, **ADAM)
            coefs.append(guard.stats())
        tp, tm, tv, ts = _run_steps(dev, p, grads, d, stepper)
        for k, gk in enumerate(grads):
            p64, m64, v64, t = ref.step(p64, gk.astype(np.float64), m64, v64, t, decay=d64, **ADAM)
            s = coefs[k]
            print(kw, 'step', k, 'coef %.9g want %.9g norm %.9g want %.9g' % (s['last_coef'], ref.last['last_coef'], s['last_norm'], ref.last['last_norm']))
            assert abs(s['last_coef'] - ref.last['last_coef']) <= 1e-6 * ref.last['last_coef']
            assert abs(s['last_norm'] - ref.last['last_norm']) <= 1e-6 * ref.last['last_norm']
            if k == 0 and 'clipnorm' in kw:
                assert s['last_coef'] < 0.31             # the clip did bite
        ep, em = np.abs(tp.cpu().numpy() - p64).max(), np.abs(tm.cpu().numpy() - m64).max()
        print(kw, 'max |p - ref| %.3g  max |m - ref| %.3g' % (ep, em))
        assert int(ts) == 3 and ep <= 1e-5 and em <= 1e-6


@pytest.mark.gpu
def test_clipnorm_above_the_norm_changes_nothing():
    from qcnn_amd.training import GradGuard
    dev = _dev()
    n = 10007
    p, g, d = _buffers(dev, n, 2, True)
    grads = [g, (0.5 * g[::-1]).copy(), (g * g).astype(np.float32)]
    runs = []
    for kw in (dict(), dict(clipnorm=1e4)):                  # the norms are ~ 100, 50 and 170
        guard = GradGuard(dev, **kw)
        runs.append(_run_steps(dev, p, grads, d, lambda tp, tg, tm, tv, ts, td: guard.step(tp, tg, tm, tv, ts, decay=td, **ADAM)))
        assert guard.stats()['last_coef'] == 1.0 and 100 < guard.stats()['last_norm'] < 1e4
    for a, b, name in zip(runs[0], runs[1], 'pmvt'):
        assert torch.equal(_bits(a), _bits(b)), name


@pytest.mark.gpu
def test_skip_and_scale_dynamics_follow_the_reference():
    from qcnn_amd.training import GradGuard
    dev = _dev()
    n = 4099
    p, g, d = _buffers(dev, n, 3, True)
    kw = dict(loss_scale=1024.0, dynamic=True, growth_interval=2, backoff_factor=0.25, clipnorm=50.0)
    guard, ref = GradGuard(dev, **kw), GuardRef(**kw)
    tp, tg = torch.tensor(p, device=dev), torch.zeros(n, device=dev)
    tm, tv, td = torch.zeros_like(tp), torch.zeros_like(tp), torch.tensor(d, device=dev)
    ts = torch.zeros(1, dtype=torch.int32, device=dev)
    p64, m64, v64, t, d64 = p.astype(np.float64), np.zeros(n), np.zeros(n), 0, d.astype(np.float64)
    rng = np.random.RandomState(9)
    kinds = ['ok', 'inf', 'ok', 'nan', 'ok', 'ok', 'ok', 'ok']
    for k, kind in enumerate(kinds):
        gk = (rng.randn(n) * 1024.0).astype(np.float32)       # the test WRITES the gradient, bad element included
        if kind == 'inf':
            gk[n - 1] = np.inf
        if kind == 'nan':
            gk[17] = np.nan
        tg.copy_(torch.tensor(gk, device=dev))
        before = [_bits(x) for x in (tp, tm, tv, ts)]
        guard.step(tp, tg, tm, tv, ts, zero_grad=True, decay=td, **ADAM)
        p64, m64, v64, t = ref.step(p64, gk.astype(np.float64), m64, v64, t, zero_grad=True, decay=d64, **ADAM)
        got, want = guard.stats(), ref.stats()
        print(k, kind, got)
        for key in ('scale', 'good_steps', 'skipped_steps', 'last_skipped', 'nonfinite_count', 'last_unscale'):
            assert got[key] == want[key], (k, key, got[key], want[key])
        assert float(tg.abs().max()) == 0.0, 'grad must be cleared, applied or not'
        assert int(ts) == t
        if kind != 'ok':
            assert got['last_skipped'] == 1 and got['last_norm'] == float('inf')
            for a, b, name in zip(before, (tp, tm, tv, ts), 'pmvt'):
                assert torch.equal(a, _bits(b)), 'step %d (%s) changed %s' % (k, kind, name)
        else:
            assert abs(got['last_norm'] - want['last_norm']) <= 1e-6 * want['last_norm']
    assert t == 6 and guard.stats()['skipped_steps'] == 2
    assert np.abs(tp.cpu().numpy() - p64).max() <= 1e-5 and np.abs(tm.cpu().numpy() - m64).max() <= 1e-6
    # state_dict round trip into a fresh guard
    other = GradGuard(dev, **kw)
    other.load_state_dict(guard.state_dict())
    assert other.state_dict() == guard.state_dict() == dict(scale=want['scale'], good_steps=want['good_steps'], skipped_steps=2)


@pytest.mark.gpu
def test_guarded_step_replays_in_a_captured_graph():
    """copy static source -> grad, GradGuard.step(zero_grad=True) as ONE captured linear graph, replayed with a finite, an inf and
    a finite source: bit-equal to the eager sequence.  That the capture succeeds at all shows the step reads nothing on the host."""
    from qcnn_amd.training import GradGuard
    dev = _dev()
    n = 10007
    p, g, d = _buffers(dev, n, 4, True)
    bad = (g * 3).astype(np.float32)
    bad[5000] = np.inf
    sources = [g * 64, bad, (g[::-1] * 64).copy()]
    kw = dict(loss_scale=64.0, dynamic=True, growth_interval=2, clipnorm=30.0)

    def fresh():
        tp = torch.tensor(p, device=dev)
        return dict(p=tp, g=torch.zeros_like(tp), m=torch.zeros_like(tp), v=torch.zeros_like(tp), d=torch.tensor(d, device=dev),
                    t=torch.zeros(1, dtype=torch.int32, device=dev), src=torch.zeros_like(tp), guard=GradGuard(dev, **kw))

    def body(b):
        b['g'].copy_(b['src'])
        b['guard'].step(b['p'], b['g'], b['m'], b['v'], b['t'], zero_grad=True, decay=b['d'], **ADAM)

    eager = fresh()
    for s in sources:
        eager['src'].copy_(torch.tensor(s, device=dev))
        body(eager)
    torch.cuda.synchronize()
    rep = fresh()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        body(rep)
    for s in sources:
        rep['src'].copy_(torch.tensor(s, device=dev))
        graph.replay()
    torch.cuda.synchronize()
    for name in 'pmvtg':
        assert torch.equal(_bits(eager[name]), _bits(rep[name])), name
    assert torch.equal(_bits(eager['guard']._state), _bits(rep['guard']._state))
    s = rep['guard'].stats()
    assert int(rep['t']) == 2 and s['skipped_steps'] == 1 and s['scale'] == 32.0 and s['good_steps'] == 1


def _small_model(dev, seed):
    """The small TIMIT model of test_fp16_timit_step_under_ctc_matches_fp32_with_loss_scaling_and_underflows_without."""
    from qcnn_amd.models import TimitQCNN
    np.random.seed(seed)
    torch.manual_seed(seed)
    model = TimitQCNN(num_layers=4, start_filter=32, act='relu', aact='none', dropout=0.0, l2=1e-5, fuse_head=True, chain_convs=True)
    rng = np.random.RandomState(seed + 1)
    x = torch.tensor(rng.randn(4, 4, 41, 40).astype(np.float32), device=dev)
    with torch.no_grad():
        model(x)
        for name, p in model.named_parameters():
            if name.endswith('bias'):
                p.copy_(torch.tensor(0.1 * rng.randn(*p.shape), dtype=torch.float32))
    model.to(dev)
    rng = np.random.RandomState(5)
    labels = torch.tensor(rng.randint(0, 61, (4, 10)), device=dev, dtype=torch.int32)
    il = torch.full((4, 1), 40, dtype=torch.int32, device=dev)
    ll = torch.tensor([[10], [7], [9], [4]], dtype=torch.int32, device=dev)
    return model, x.to(torch.float16), labels, il, ll


@pytest.mark.gpu
def test_device_tensor_loss_scale_gives_the_float_forms_gradient_bit_for_bit():
    from qcnn_amd import _lib, dp
    dev = _dev()
    model, x16, labels, il, ll = _small_model(dev, 23)
    flat = dp.FlatParams([q for q in model.parameters() if q.requires_grad])
    scale_dev = torch.full((1,), 4096.0, device=dev)
    out = []
    with _lib.debug_flags(_lib.QK_DBG_DETERMINISTIC):
        for scale in (4096.0, scale_dev, 1.0):
            flat.zero_grad()
            loss = model.training_loss(x16, labels, il, ll, loss_scale=scale)
            loss.backward()
            out.append((float(loss), flat.grad.clone()))
    assert out[0][0] == out[1][0] == out[2][0] and math.isfinite(out[0][0])
    assert float(out[0][1].abs().max()) > 0
    assert torch.equal(_bits(out[0][1]), _bits(out[1][1]))
    assert not torch.equal(_bits(out[0][1]), _bits(out[2][1]))           # (the scale does reach the gradient)
    # the unfused forms take the tensor as well
    y = model(x16)
    from qcnn_amd.layers import ctc_batch_cost
    ga, = torch.autograd.grad(ctc_batch_cost(y, labels, il, ll, loss_scale=4096.0).mean(), y, retain_graph=True)
    gb, = torch.autograd.grad(ctc_batch_cost(y, labels, il, ll, loss_scale=scale_dev).mean(), y)
    assert torch.equal(ga.view(torch.int16).cpu(), gb.view(torch.int16).cpu())
    with pytest.raises(TypeError):
        model.ctc_loss(x16, labels, il, ll, loss_scale=torch.tensor([4096.0]))          # a host tensor


@pytest.mark.gpu
def test_a_misshapen_tensor_loss_scale_is_refused_on_every_path_before_the_backward():
    from qcnn_amd import _lib
    from qcnn_amd.layers import ctc_batch_cost
    dev = _dev()
    model, x16, labels, il, ll = _small_model(dev, 23)
    y = model(x16).detach().requires_grad_()
    bad = [torch.full((1,), 4096.0, device=dev, dtype=torch.float64), torch.full((2,), 4096.0, device=dev),
           torch.full((1,), 4096.0)]
    for scale in bad:
        with pytest.raises(TypeError):
            model.training_loss(x16, labels, il, ll, loss_scale=scale)
        with pytest.raises(TypeError):
            ctc_batch_cost(y, labels, il, ll, loss_scale=scale)
        with _lib.debug_flags(_lib.QK_DBG_NO_FUSED_CTC):           # the torch path of layers.ctc_batch_cost
            with pytest.raises(TypeError):
                ctc_batch_cost(y, labels, il, ll, loss_scale=scale)
    with _lib.debug_flags(_lib.QK_DBG_NO_FUSED_CTC):               # ... which takes the right tensor like the kernel path does
        good = torch.full((1,), 4096.0, device=dev)
        ga, = torch.autograd.grad(ctc_batch_cost(y, labels, il, ll, loss_scale=4096.0).mean(), y)
        gb, = torch.autograd.grad(ctc_batch_cost(y, labels, il, ll, loss_scale=good).mean(), y)
    assert float(ga.float().abs().max()) > 0 and torch.equal(ga.view(torch.int16).cpu(), gb.view(torch.int16).cpu())


@pytest.mark.gpu
@pytest.mark.parametrize('d', [
    dict(scale=0.5, good_steps=0, skipped_steps=0), dict(scale=128.0, good_steps=0, skipped_steps=0),
    dict(scale=float('nan'), good_steps=0, skipped_steps=0), dict(scale=8.0, good_steps=-1, skipped_steps=0),
    dict(scale=8.0, good_steps=0, skipped_steps=-3)], ids=['below_min', 'above_max', 'nan', 'good<0', 'skipped<0'])
def test_load_state_dict_checks_what_the_constructor_checks(d):
    from qcnn_amd.training import GradGuard
    guard = GradGuard(_dev(), loss_scale=8.0, dynamic=True, min_scale=1.0, max_scale=64.0)
    with pytest.raises(ValueError):
        guard.load_state_dict(d)
    assert guard.state_dict() == dict(scale=8.0, good_steps=0, skipped_steps=0)          # nothing was written
    guard.load_state_dict(dict(scale=64.0, good_steps=5, skipped_steps=2))
    assert guard.state_dict() == dict(scale=64.0, good_steps=5, skipped_steps=2)


@pytest.mark.gpu
def test_fp16_training_with_a_dynamic_guard_backs_off_from_an_overflowing_scale():
    """float16 activations, loss scale started at 2^30 -- d cost / d y_pred x 2^30 / batch is far beyond float16's 65504, so the first
    backward overflows -- backoff 1 / 16: within 8 steps the guard has skipped at least once, applied at least once, the parameters
    are finite and the scale has come down."""
    from qcnn_amd import _lib, dp
    from qcnn_amd.training import GradGuard
    dev = _dev()
    model, x16, labels, il, ll = _small_model(dev, 23)
    flat = dp.FlatParams([q for q in model.parameters() if q.requires_grad])
    p0 = flat.param.clone()
    guard = GradGuard(dev, loss_scale=2.0 ** 30, dynamic=True, backoff_factor=1.0 / 16, max_scale=2.0 ** 30)
    m, v = torch.zeros_like(flat.param), torch.zeros_like(flat.param)
    step = torch.zeros(1, dtype=torch.int32, device=dev)
    with _lib.debug_flags(_lib.QK_DBG_DETERMINISTIC):
        for k in range(8):
            loss = model.training_loss(x16, labels, il, ll, loss_scale=guard.loss_scale)
            loss.backward()
            guard.step(flat.param, flat.grad, m, v, step, lr=1e-4, zero_grad=True)
            print(k, float(loss), guard.stats())
    s = guard.stats()
    applied = int(step)
    assert s['skipped_steps'] >= 1 and applied >= 1 and s['skipped_steps'] + applied == 8
    assert bool(torch.isfinite(flat.param).all()) and bool(torch.isfinite(m).all()) and bool(torch.isfinite(v).all())
    assert s['scale'] <= 2.0 ** 30 / 16
    assert not torch.equal(flat.param, p0)


@pytest.mark.gpu
def test_c_abi_refuses_null_state_zero_n_and_a_small_workspace():
    from qcnn_amd import _lib
    dev = _dev()
    lib = _lib.lib()
    n = 4099
    g = torch.ones(n, device=dev)
    state = torch.zeros(8, device=dev)
    state[0] = 1.0
    need = int(lib.qk_grad_guard_workspace_bytes(n))
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    cfg = _lib.GradGuardConfig()
    stream = torch.cuda.current_stream(dev).cuda_stream
    ok = lib.qk_grad_guard_reduce(g.data_ptr(), None, None, n, 1.0, ctypes.byref(cfg), state.data_ptr(), ws.data_ptr(), need, stream)
    assert ok == 0 and float(state[4]) == pytest.approx(math.sqrt(n), rel=1e-6)
    bad = [
        lib.qk_grad_guard_reduce(g.data_ptr(), None, None, n, 1.0, ctypes.byref(cfg), None, ws.data_ptr(), need, stream),
        lib.qk_grad_guard_reduce(g.data_ptr(), None, None, 0, 1.0, ctypes.byref(cfg), state.data_ptr(), ws.data_ptr(), need, stream),
        lib.qk_grad_guard_reduce(g.data_ptr(), None, None, n, 1.0, ctypes.byref(cfg), state.data_ptr(), ws.data_ptr(), need - 1, stream),
        lib.qk_grad_guard_reduce(g.data_ptr(), None, None, n, 1.0, None, state.data_ptr(), ws.data_ptr(), need, stream),
        lib.qk_grad_guard_reduce(g.data_ptr(), g.data_ptr(), None, n, 1.0, ctypes.byref(cfg), state.data_ptr(), ws.data_ptr(), need, stream),
        lib.qk_adam_step_guarded(g.data_ptr(), g.data_ptr(), g.data_ptr(), g.data_ptr(), None, n, 1e-3, 0.9, 0.999, 1e-7, ws.data_ptr(), 0,
                                 ctypes.byref(cfg), None, stream),
        lib.qk_adam_step_guarded(g.data_ptr(), g.data_ptr(), g.data_ptr(), g.data_ptr(), None, 0, 1e-3, 0.9, 0.999, 1e-7, ws.data_ptr(), 0,
                                 ctypes.byref(cfg), state.data_ptr(), stream),
    ]
    assert bad == [_lib.QK_ERR_INVALID_ARG] * len(bad), bad
    assert b'qk_adam_step_guarded' in lib.qk_last_error()
    torch.cuda.synchronize()
    assert float(g.min()) == 1.0 and float(g.max()) == 1.0            # the refused calls launched nothing
