"""Quaternion layer normalisation (include/qk_norm.h; qcnn_amd.functional.qlayer_norm, qcnn_amd.complexnn.QuaternionLayerNormalization,
qcnn_amd.models.TimitQLSTM(layer_norm=True)) against the float64 restatement of tests/qlnorm_ref.py.

Bounds (relative to max|want| per tensor).  fp32: against the float64 reference, the project's fp32 bound 1e-4.  bf16 / fp16: against
the reference WITH the header's two rounding points, at the bounds of tests/test_gpu_parity.py: 16-bit outputs (y, dx) 1e-2 / 2e-3,
fp32 outputs (dgamma, dbeta) 2e-3 / 1e-3.  test_rounding_points_move_the_reference_by_less_than_the_16_bit_bound shows on the same
inputs that the rounding points alone stay inside 1e-2 / 2e-3 of the float64 reference and are in play.
"""
import ctypes
import functools
import os
import re

import numpy as np
import pytest
import torch

import guarded_alloc as GA
import qlnorm_ref as R
import qlstm_ref as LR
from qcnn_amd import _lib, functional as F
from qcnn_amd.complexnn import QuaternionLayerNormalization
from qcnn_amd.models import TimitQLSTM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = {torch.float32: None, torch.bfloat16: 'bf16', torch.float16: 'fp16'}
DTYPE_IDS = ['fp32', 'bf16', 'fp16']
BOUND_16 = {'bf16': 1e-2, 'fp16': 2e-3}          # 16-bit outputs
BOUND_32 = {'bf16': 2e-3, 'fp16': 1e-3}          # fp32 outputs of the 16-bit paths
OUT_16, OUT_32 = ('y', 'dx'), ('dgamma', 'dbeta')
# the GPU shapes: 490 rows = 31 slabs of 16 rows, the last one ragged (10 rows); 8 quaternion units = the smallest vector width (most
# lanes idle), 72 = a partly filled wave, 520 = one more than a full pass of 64 lanes x 8 units (a second register group; fp32: a
# third of four), 5 = the generic kernels
B, T, QS = 70, 7, (8, 72, 520, 5)
EPS = 1e-3


def _dev():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    return torch.device('cuda:0')


def _rel(got, want):
    return float(np.abs(np.asarray(got, dtype=np.float64) - want).max()) / max(float(np.abs(want).max()), 1e-30)


def _f32(a):
    return a.astype(np.float32).astype(np.float64)


def _lengths(bsz, steps, seed):
    """lengths that contain 0, 1, steps - 2 and steps, the rest random."""
    rng = np.random.RandomState(seed)
    out = rng.randint(0, steps + 1, size=bsz)
    out[:4] = [0, 1, steps - 2, steps]
    return out.astype(np.int32)


def _expected_path(dtype, q):
    return 'vec' if q % (4 if dtype == torch.float32 else 8) == 0 and q <= 1024 else 'generic'


@functools.lru_cache(maxsize=None)
def _inputs(q, kind, offset=0.0):
    """Seeded operands (never written), 16-bit ones already rounded to `kind`; gamma / beta are fp32 values."""
    rng = np.random.RandomState(2000 + q)
    d = dict(x=R.rnd(_f32(offset + 1.5 * rng.randn(B, T, 4 * q) + rng.randn(4 * q)), kind), gamma=_f32(1 + 0.3 * rng.randn(q)),
             beta=_f32(0.3 * rng.randn(4 * q)), dy=R.rnd(_f32(rng.randn(B, T, 4 * q)), kind), lengths=_lengths(B, T, q))
    for v in d.values():
        v.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def _reference(q, kind, lengths=True, affine=True, offset=0.0):
    """The reference's outputs for _inputs(...), computed once and shared."""
    i = _inputs(q, kind, offset)
    return R.qlayer_norm(i['x'], i['gamma'] if affine else None, i['beta'] if affine else None, i['lengths'] if lengths else None,
                         epsilon=EPS, kind=kind, dy=i['dy'])


# ---- CPU part ------------------------------------------------------------------------------------------------------------------
def test_reference_backward_agrees_with_central_differences():
    """N = 6 (B = 2, T = 3, lengths 3 / 1), Q = 3: 1e-7 relative for dx, dgamma, dbeta."""
    rng = np.random.RandomState(5)
    lengths = np.array([3, 1])
    par = dict(x=1.5 * rng.randn(2, 3, 12) + rng.randn(12), gamma=1 + 0.3 * rng.randn(3), beta=0.3 * rng.randn(12))
    w = rng.randn(2, 3, 12)

    def loss(p):
        return float((R.qlayer_norm(p['x'], p['gamma'], p['beta'], lengths, epsilon=EPS)['y'] * w).sum())
    got = R.qlayer_norm(par['x'], par['gamma'], par['beta'], lengths, epsilon=EPS, dy=w)
    eps = 1e-5
    for name, gname in (('x', 'dx'), ('gamma', 'dgamma'), ('beta', 'dbeta')):
        want = np.zeros_like(par[name])
        flat, wflat = par[name].reshape(-1), want.reshape(-1)
        for k in range(flat.size):
            keep = flat[k]
            flat[k] = keep + eps
            up = loss(par)
            flat[k] = keep - eps
            wflat[k] = (up - loss(par)) / (2 * eps)
            flat[k] = keep
        assert float(np.abs(want).max()) > 0.1 and _rel(got[gname], want) <= 1e-7, (gname, _rel(got[gname], want))


def test_norm_header_inventory_equals_the_fifth_symbol_table():
    lib = _lib.lib()
    h = open(os.path.join(ROOT, 'include', 'qk_norm.h')).read()
    declared = set(re.findall(r'\b(qk_[a-z_0-9]+)\s*\(', h))
    declared -= {n for n in declared if n.endswith('_t')}
    assert declared == set(_lib.NORM_SYMBOLS), declared ^ set(_lib.NORM_SYMBOLS)
    for name in declared:
        assert hasattr(lib, name), name
    for other in (_lib.SYMBOLS, _lib.OPT_SYMBOLS, _lib.DATA_SYMBOLS, _lib.RNN_SYMBOLS):
        assert not set(_lib.NORM_SYMBOLS) & set(other)
    main = open(os.path.join(ROOT, 'include', 'qk.h')).read()
    assert not any(name in main for name in _lib.NORM_SYMBOLS) and 'qlnorm' not in main
    decls = {name: (res, args) for res, name, args in re.findall(r'^(int|size_t) (qk_[a-z_0-9]+)\(([^;]*)\);', h, re.M | re.S)}
    assert set(decls) == set(_lib.NORM_SYMBOLS)
    for name, (res, args) in decls.items():
        restype, argtypes = _lib.NORM_SYMBOLS[name]
        assert restype is (ctypes.c_int if res == 'int' else ctypes.c_size_t), name
        assert len(argtypes) == len(args.split(',')), name
        last = ' '.join(args.split(',')[-1].split())
        if name in ('qk_qlnorm_fwd', 'qk_qlnorm_bwd'):
            assert last == 'void *stream' and argtypes[-1] is ctypes.c_void_p, name
        else:                                                       # host only
            assert 'stream' not in args, name
    body = h[h.index('typedef struct qk_qlnorm_desc_t {'):h.index('} qk_qlnorm_desc_t;')]
    fields = re.findall(r'^\s*int32_t ([a-z_]+);', body, re.M)
    assert fields == ['dtype', 'rows', 'steps', 'q', 'x_stride', 'y_stride', 'flags']
    assert [(n, ctypes.c_int32) for n in fields] == list(_lib.QLNormDesc._fields_) and ctypes.sizeof(_lib.QLNormDesc) == 28
    for macro in ('QK_QLNORM_PATH_GENERIC', 'QK_QLNORM_PATH_VEC'):
        assert int(re.search(r'#define %s (\d+)' % macro, h).group(1)) == getattr(_lib, macro)
    assert lib.qk_version() == 103


def test_dispatch_predicate_and_descriptor_checks_need_no_gpu():
    for dtype, q in ((torch.bfloat16, 8), (torch.float16, 72), (torch.bfloat16, 520), (torch.float16, 1024), (torch.float32, 4),
                     (torch.float32, 520), (torch.float32, 1024), (torch.bfloat16, 5), (torch.float16, 4), (torch.bfloat16, 12),
                     (torch.float32, 6), (torch.bfloat16, 1032), (torch.float32, 1028)):
        assert F.qlayer_norm_path(dtype, B * T, q) == _expected_path(dtype, q), (dtype, q)
    assert [_expected_path(torch.bfloat16, q) for q in QS] == ['vec', 'vec', 'vec', 'generic']
    lib = _lib.lib()
    sup = lambda d: lib.qk_qlnorm_supported(ctypes.byref(d))
    # strides that break the 16-byte alignment of a row send a vector width to the generic kernels
    assert sup(F.qlayer_norm_desc(torch.bfloat16, 6, 8, x_stride=40)) == _lib.QK_QLNORM_PATH_VEC
    assert sup(F.qlayer_norm_desc(torch.bfloat16, 6, 8, x_stride=36)) == sup(F.qlayer_norm_desc(torch.float32, 6, 4, y_stride=18)) == _lib.QK_QLNORM_PATH_GENERIC
    good = F.qlayer_norm_desc(torch.bfloat16, B * T, 72, steps=T)
    slab = lib.qk_qlnorm_slab_rows(ctypes.byref(good))
    assert 0 < slab <= 245 and (B * T) % slab and slab % 4 == 0          # the GPU shapes: at least two slabs and a ragged last one
    assert lib.qk_qlnorm_workspace_bytes(ctypes.byref(good), _lib.QK_OP_BWD) == -(-B * T // slab) * 5 * 72 * 4
    assert lib.qk_qlnorm_workspace_bytes(ctypes.byref(good), _lib.QK_OP_FWD) == 0
    for field, value in (('dtype', 7), ('rows', 0), ('q', 0), ('x_stride', 287), ('y_stride', 287), ('steps', 8), ('steps', -1), ('flags', 1)):
        bad = F.qlayer_norm_desc(torch.bfloat16, B * T, 72, steps=T)
        setattr(bad, field, value)
        assert sup(bad) == 0 and lib.qk_last_error(), field
        assert lib.qk_qlnorm_workspace_bytes(ctypes.byref(bad), _lib.QK_OP_BWD) == 0 and lib.qk_qlnorm_slab_rows(ctypes.byref(bad)) == 0, field
        assert lib.qk_qlnorm_fwd(ctypes.byref(bad), None, None, None, None, EPS, None, None, None) == _lib.QK_ERR_INVALID_ARG, field
        assert lib.qk_qlnorm_bwd(ctypes.byref(bad), *([None] * 9), 0, None) == _lib.QK_ERR_INVALID_ARG, field
    assert lib.qk_qlnorm_fwd(ctypes.byref(good), None, None, None, None, EPS, None, None, None) == _lib.QK_ERR_INVALID_ARG      # NULL buffers
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        F.qlayer_norm(torch.zeros(3, 32))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        QuaternionLayerNormalization()(torch.zeros(3, 32))


def test_layer_surface():
    layer = QuaternionLayerNormalization(epsilon=1e-4, name='ln')
    layer.ensure_built((None, None, 20), torch.device('cpu'))
    assert [(n, tuple(p.shape)) for n, p in layer.weights] == [('gamma', (5,)), ('beta', (20,))]
    assert (layer.gamma.detach() == 1).all() and (layer.beta.detach() == 0).all() and not layer.regularization_losses()
    assert layer.compute_output_shape((3, 11, 20)) == (3, 11, 20)
    cfg = layer.get_config()
    assert cfg['epsilon'] == 1e-4 and cfg['center'] and cfg['scale'] and cfg['name'] == 'ln'
    again = QuaternionLayerNormalization.from_config(cfg)
    assert again.get_config() == cfg
    for kw, names in ((dict(center=False), ['gamma']), (dict(scale=False), ['beta']), (dict(center=False, scale=False), [])):
        part = QuaternionLayerNormalization(**kw)
        part.ensure_built((None, 20), torch.device('cpu'))
        assert [n for n, _ in part.weights] == names and [n for n, _ in part.named_parameters()] == names
        assert QuaternionLayerNormalization.from_config(part.get_config()).get_config() == part.get_config()
    const = QuaternionLayerNormalization(gamma_initializer={'class_name': 'Constant', 'config': {'value': 0.5}})
    const.ensure_built((None, 8), torch.device('cpu'))
    assert (const.gamma.detach() == 0.5).all()
    with pytest.raises(ValueError):
        QuaternionLayerNormalization().ensure_built((None, 30), torch.device('cpu'))
    plain = TimitQLSTM(num_layers=2, units=32, dropout=0.0)
    normed = TimitQLSTM(num_layers=2, units=32, dropout=0.0, layer_norm=True)
    for m in (plain, normed):
        for k, layer in enumerate(m.rnn):
            layer.ensure_built((None, None, 164 if k == 0 else 64), torch.device('cpu'))
        m.pred.layer.ensure_built((None, 64), torch.device('cpu'))
    for layer in normed.norm:
        layer.ensure_built((None, None, 64), torch.device('cpu'))
    today = ['rnn.0.kernel', 'rnn.0.recurrent_kernel', 'rnn.0.bias', 'rnn.1.kernel', 'rnn.1.recurrent_kernel', 'rnn.1.bias',
             'pred.layer.kernel', 'pred.layer.bias']
    new = ['norm.0.gamma', 'norm.0.beta', 'norm.1.gamma', 'norm.1.beta']
    assert [n for n, _ in plain.named_parameters()] == today and not hasattr(plain, 'norm')
    assert sorted(n for n, _ in normed.named_parameters()) == sorted(today + new)
    assert sorted(set(normed.state_dict()) - set(plain.state_dict())) == sorted(new) and set(plain.state_dict()) <= set(normed.state_dict())
    assert tuple(normed.norm[1].gamma.shape) == (16,) and tuple(normed.norm[1].beta.shape) == (64,)


def test_reference_inactive_rows_constant_rows_and_full_lengths():
    rng = np.random.RandomState(9)
    x, gamma, beta, dy = 1.5 * rng.randn(4, T, 20) + 3, 1 + 0.3 * rng.randn(5), 0.3 * rng.randn(20), rng.randn(4, T, 20)
    lengths = np.array([0, 1, T - 2, T])
    o = R.qlayer_norm(x, gamma, beta, lengths, epsilon=EPS, dy=dy)
    assert (o['y'][0] == 0).all() and (o['dx'][0] == 0).all() and (o['y'][1, 1:] == 0).all() and (o['dx'][2, T - 2:] == 0).all()
    assert np.abs(o['y'][1, 0]).min() > 0 and np.abs(o['y'][3]).min() > 0
    # an inactive row adds nothing to the weight gradients: whatever its dy and x hold
    x2, dy2 = x.copy(), dy.copy()
    x2[0], dy2[0], x2[1, 1:], dy2[1, 1:] = 7.0, 100.0, -3.0, -50.0
    o2 = R.qlayer_norm(x2, gamma, beta, lengths, epsilon=EPS, dy=dy2)
    assert (o2['dgamma'] == o['dgamma']).all() and (o2['dbeta'] == o['dbeta']).all()
    # lengths all equal to T: the call without lengths
    full, none = R.qlayer_norm(x, gamma, beta, np.full(4, T), epsilon=EPS, dy=dy), R.qlayer_norm(x, gamma, beta, None, epsilon=EPS, dy=dy)
    for name in ('y', 'dx', 'dgamma', 'dbeta'):
        assert (full[name] == none[name]).all(), name
    # a constant row (every unit equal per component): xhat = 0, y = beta, rstd = 1 / sqrt(epsilon), dx = rstd (g - m_c), all finite;
    # Q = 1 is always such a row, and there g = m_c: dx = 0
    const = np.repeat(rng.randn(3, 4, 1), 5, axis=2).reshape(3, 20)
    for xc, g, b, d in ((const, gamma, beta, dy[0, :3]), (rng.randn(3, 4), gamma[:1], beta[:4], dy[0, :3, :4])):
        oc = R.qlayer_norm(xc, g, b, epsilon=EPS, dy=d)
        assert all(np.isfinite(v).all() for v in oc.values())
        assert np.abs(oc['xhat']).max() <= 1e-13 and np.abs(oc['y'] - b).max() <= 1e-13 and np.abs(oc['rstd'] * np.sqrt(EPS) - 1).max() <= 1e-12
        gg = (d.reshape(3, 4, -1) * g)
        assert np.abs(oc['dx'] - ((gg - gg.mean(axis=2, keepdims=True)) / np.sqrt(EPS)).reshape(xc.shape)).max() <= 1e-9
        if g.size == 1:
            assert np.abs(oc['dx']).max() <= 1e-12


@pytest.mark.parametrize('kind', ['bf16', 'fp16'])
@pytest.mark.parametrize('q', QS)
def test_rounding_points_move_the_reference_by_less_than_the_16_bit_bound(q, kind):
    """On the GPU tests' own inputs: the reference with rounding points stays within 1e-2 (bf16) / 2e-3 (fp16) of the float64 one
    (measured over the four widths: at most 2.9e-3 / 3.5e-4 on y, 3.0e-3 / 3.7e-4 on dx), and is not identical to it."""
    i = _inputs(q, kind)
    pure = R.qlayer_norm(i['x'], i['gamma'], i['beta'], i['lengths'], epsilon=EPS, dy=i['dy'])
    rounded = _reference(q, kind)
    errs = {name: _rel(rounded[name], pure[name]) for name in OUT_16 + OUT_32}
    print(q, kind, errs)
    assert max(errs.values()) <= BOUND_16[kind], errs
    assert min(errs[name] for name in OUT_16) > 1e-5 and max(errs[name] for name in OUT_32) == 0, errs


def test_uncentred_variance_in_fp32_misses_the_bound_the_centred_form_keeps():
    """x = 1000 + randn, Q = 72 (the inputs of test_centred_variance_keeps_its_digits_at_a_large_offset): E[x^2] - mu^2 evaluated in
    fp32 is off by far more than the fp32 bound in rstd; so the GPU test tells the two forms apart."""
    i = _inputs(72, None, offset=1000.0)
    want = _reference(72, None, lengths=False, offset=1000.0)['rstd']
    assert _rel(R.naive_variance(i['x'], EPS), want) > 1e-2
    assert _rel(R.naive_variance(i['x'], EPS, dtype=np.float64), want) <= 1e-6


# every entry of NORM_SYMBOLS against the hygiene case that exercises it, or the reason it has none
HYGIENE_COVER = {
    'qk_qlnorm_fwd': 'test_forward_and_backward_keep_to_their_buffers: vec (bf16, Q = 72, lengths) and generic (fp32, Q = 5)',
    'qk_qlnorm_bwd': 'test_forward_and_backward_keep_to_their_buffers: the same calls',
    'qk_qlnorm_supported': 'host only: takes no device buffer (test_dispatch_predicate_and_descriptor_checks_need_no_gpu)',
    'qk_qlnorm_slab_rows': 'host only: takes no device buffer (the same test)',
    'qk_qlnorm_workspace_bytes': 'host only: *_bytes',
}


def test_every_norm_entry_point_has_a_hygiene_case_or_a_reason():
    assert set(HYGIENE_COVER) == set(_lib.NORM_SYMBOLS)


# ---- GPU part ------------------------------------------------------------------------------------------------------------------
def _run(dev, dtype, q, lengths=True, affine=True, offset=0.0):
    """functional.qlayer_norm forward and backward on _inputs(...): name -> tensor."""
    i = _inputs(q, KINDS[dtype], offset)
    t = lambda a, dt=dtype: torch.tensor(a, dtype=dt, device=dev)
    x = t(i['x']).requires_grad_()
    gamma = t(i['gamma'], torch.float32).requires_grad_() if affine else None
    beta = t(i['beta'], torch.float32).requires_grad_() if affine else None
    ln = torch.tensor(i['lengths'], device=dev) if lengths else None
    y = F.qlayer_norm(x, gamma, beta, ln, epsilon=EPS)
    y.backward(t(i['dy']))
    res = dict(y=y.detach(), dx=x.grad)
    if affine:
        res.update(dgamma=gamma.grad, dbeta=beta.grad)
    return res


def _check(got, want, dtype, what=''):
    kind = KINDS[dtype]
    errs = {}
    for name, g in got.items():
        assert g.dtype == (torch.float32 if name in OUT_32 else dtype) and tuple(g.shape) == want[name].shape, name
        errs[name] = (_rel(g.float().cpu().numpy(), want[name]), 1e-4 if kind is None else BOUND_16[kind] if name in OUT_16 else BOUND_32[kind])
    print(what, errs)
    assert all(e <= b for e, b in errs.values()), errs


@pytest.mark.gpu
@pytest.mark.parametrize('affine', [True, False], ids=['gamma_beta', 'plain'])
@pytest.mark.parametrize('lengths', [True, False], ids=['lengths', 'all_rows'])
@pytest.mark.parametrize('q', QS)
@pytest.mark.parametrize('dtype', list(KINDS), ids=DTYPE_IDS)
def test_forward_and_backward_match_the_reference(dtype, q, lengths, affine):
    dev = _dev()
    assert F.qlayer_norm_path(dtype, B * T, q) == _expected_path(dtype, q)
    got = _run(dev, dtype, q, lengths, affine)
    _check(got, _reference(q, KINDS[dtype], lengths, affine), dtype)
    if lengths:                    # asserted, not tolerated: inactive rows are exactly zero
        ln = _inputs(q, KINDS[dtype])['lengths']
        inactive = torch.tensor(np.arange(T)[None, :] >= ln[:, None], device=dev)
        assert int(inactive.sum()) > T and int(got['y'][inactive].ne(0).sum()) == 0 and int(got['dx'][inactive].ne(0).sum()) == 0


@pytest.mark.gpu
@pytest.mark.parametrize('which', ['gamma_only', 'beta_only'])
def test_one_weight_alone_and_two_dimensional_input(which):
    dev = _dev()
    i = _inputs(72, 'bf16')
    t = lambda a, dt=torch.bfloat16: torch.tensor(a, dtype=dt, device=dev)
    x = t(i['x']).reshape(B * T, 288).requires_grad_()
    w = t(i['gamma' if which == 'gamma_only' else 'beta'], torch.float32).requires_grad_()
    y = F.qlayer_norm(x, gamma=w, epsilon=EPS) if which == 'gamma_only' else F.qlayer_norm(x, beta=w, epsilon=EPS)
    y.backward(t(i['dy']).reshape(B * T, 288))
    want = R.qlayer_norm(i['x'], i['gamma'] if which == 'gamma_only' else None, i['beta'] if which == 'beta_only' else None, None,
                         epsilon=EPS, kind='bf16', dy=i['dy'])
    got = dict(y=y.detach().view(B, T, 288), dx=x.grad.view(B, T, 288))
    got['dgamma' if which == 'gamma_only' else 'dbeta'] = w.grad
    _check(got, want, torch.bfloat16, which)


@pytest.mark.gpu
def test_centred_variance_keeps_its_digits_at_a_large_offset():
    """fp32, Q = 72, x = 1000 + noise: y and dx within 1e-4 of the float64 reference on the same fp32-rounded input (E[x^2] - mu^2 in
    fp32 loses about a tenth of a unit variance here: test_uncentred_variance_in_fp32_misses_the_bound_the_centred_form_keeps)."""
    dev = _dev()
    got = _run(dev, torch.float32, 72, lengths=False, offset=1000.0)
    _check(got, _reference(72, None, lengths=False, offset=1000.0), torch.float32, 'offset 1000')


def _raw_call(dev, dtype, q, xw, x_off, yw, y_off, use_lengths=True):
    """qk_qlnorm_fwd / _bwd through ctypes: x and dx are column windows [x_off, x_off + 4q) of (N, xw) buffers, y and dy windows
    [y_off, y_off + 4q) of (N, yw) buffers.  Returns the four wide buffers (x, y, dy, dx) and dgamma, dbeta."""
    lib = _lib.lib()
    i = _inputs(q, KINDS[dtype])
    N, W = B * T, 4 * q
    t = lambda a, dt=dtype: torch.tensor(a, dtype=dt, device=dev)
    wide = lambda width, fill: torch.full((N, width), fill, dtype=dtype, device=dev)
    xb, yb, dyb, dxb = wide(xw, 3.0), wide(yw, 5.0), wide(yw, 7.0), wide(xw, 9.0)
    xb[:, x_off:x_off + W] = t(i['x']).view(N, W)
    dyb[:, y_off:y_off + W] = t(i['dy']).view(N, W)
    gamma, beta = t(i['gamma'], torch.float32), t(i['beta'], torch.float32)
    ln = torch.tensor(i['lengths'], device=dev) if use_lengths else None
    stats = torch.empty((N, 5), dtype=torch.float32, device=dev)
    dgamma, dbeta = torch.empty(q, dtype=torch.float32, device=dev), torch.empty(W, dtype=torch.float32, device=dev)
    desc = F.qlayer_norm_desc(dtype, N, q, steps=T if use_lengths else 0, x_stride=xw, y_stride=yw)
    n = int(lib.qk_qlnorm_workspace_bytes(ctypes.byref(desc), _lib.QK_OP_BWD))
    ws = torch.empty(n, dtype=torch.uint8, device=dev)
    es = xb.element_size()
    stream = torch.cuda.current_stream(dev).cuda_stream
    p = lambda v: v.data_ptr() if v is not None else None
    with torch.cuda.device(dev):
        _lib.check(lib.qk_qlnorm_fwd(ctypes.byref(desc), xb.data_ptr() + x_off * es, p(gamma), p(beta), p(ln), EPS, yb.data_ptr() + y_off * es,
                                     p(stats), stream), 'qk_qlnorm_fwd')
        _lib.check(lib.qk_qlnorm_bwd(ctypes.byref(desc), dyb.data_ptr() + y_off * es, xb.data_ptr() + x_off * es, p(gamma), p(ln), p(stats),
                                     dxb.data_ptr() + x_off * es, p(dgamma), p(dbeta), p(ws), n, stream), 'qk_qlnorm_bwd')
    torch.cuda.synchronize(dev)
    return xb, yb, dyb, dxb, dgamma, dbeta


@pytest.mark.gpu
@pytest.mark.parametrize('dtype,q,xw,x_off,yw,y_off,same', [(torch.bfloat16, 72, 328, 16, 304, 8, True), (torch.float32, 520, 2088, 4, 2084, 4, True),
                                                             (torch.float32, 5, 27, 3, 23, 1, True), (torch.bfloat16, 72, 296, 1, 296, 1, False),
                                                             (torch.float16, 8, 35, 2, 33, 1, False)],
                         ids=['vec_bf16', 'vec_fp32', 'generic_fp32', 'vec_width_misaligned_pointers', 'vec_width_odd_strides'])
def test_strided_rows_equal_the_contiguous_call_and_leave_the_other_columns_alone(dtype, q, xw, x_off, yw, y_off, same):
    """x / dx are column windows of wider buffers, y / dy of others.  same: the strided call runs the kernels of the dense call, and
    the results are bit-equal; else (a vector width whose rows or pointers are not 16-byte aligned runs the generic kernels) they
    keep the parity bounds.  The columns outside the windows are untouched either way."""
    dev = _dev()
    W, V = 4 * q, 4 if dtype == torch.float32 else 8
    desc = F.qlayer_norm_desc(dtype, B * T, q, steps=T, x_stride=xw, y_stride=yw)
    path = _lib.QK_QLNORM_PATH_NAMES[_lib.lib().qk_qlnorm_supported(ctypes.byref(desc))]
    assert path == (_expected_path(dtype, q) if xw % V == 0 and yw % V == 0 else 'generic')
    dense = _raw_call(dev, dtype, q, W, 0, W, 0)
    xb, yb, dyb, dxb, dgamma, dbeta = _raw_call(dev, dtype, q, xw, x_off, yw, y_off)
    if same:
        for got, want in ((yb[:, y_off:y_off + W], dense[1]), (dxb[:, x_off:x_off + W], dense[3]), (dgamma, dense[4]), (dbeta, dense[5])):
            assert GA.first_bit_difference(got, want) is None
    else:
        _check(dict(y=yb[:, y_off:y_off + W].reshape(B, T, W), dx=dxb[:, x_off:x_off + W].reshape(B, T, W), dgamma=dgamma, dbeta=dbeta),
               _reference(q, KINDS[dtype]), dtype, 'generic kernels at a vector width')
    keep = lambda buf, off: torch.cat([buf[:, :off], buf[:, off + W:]], dim=1)
    assert bool((keep(yb, y_off) == 5.0).all()) and bool((keep(dxb, x_off) == 9.0).all())
    assert bool((keep(xb, x_off) == 3.0).all()) and bool((keep(dyb, y_off) == 7.0).all())
    # the same through the autograd function: a column window of a wider tensor is read in place
    x = xb[:, x_off:x_off + W].view(B, T, W).detach().requires_grad_()
    i = _inputs(q, KINDS[dtype])
    t = lambda a, dt: torch.tensor(a, dtype=dt, device=dev)
    gamma, beta = t(i['gamma'], torch.float32).requires_grad_(), t(i['beta'], torch.float32).requires_grad_()
    y = F.qlayer_norm(x, gamma, beta, torch.tensor(i['lengths'], device=dev), epsilon=EPS)
    y.backward(dyb[:, y_off:y_off + W].view(B, T, W))
    if same:
        assert GA.first_bit_difference(y.detach().reshape(B * T, W), dense[1]) is None
        assert GA.first_bit_difference(x.grad.reshape(B * T, W), dense[3]) is None
    else:
        _check(dict(y=y.detach(), dx=x.grad), _reference(q, KINDS[dtype]), dtype, 'autograd, generic kernels at a vector width')


@pytest.mark.gpu
@pytest.mark.parametrize('dtype,q', [(torch.bfloat16, 520), (torch.float16, 72), (torch.float32, 5)], ids=['vec_two_groups', 'vec_one_group', 'generic'])
def test_two_calls_agree_bit_for_bit(dtype, q):
    """No atomics: the slab partials and their sum have a fixed order, without the deterministic debug flag."""
    dev = _dev()
    first, again = _run(dev, dtype, q), _run(dev, dtype, q)
    for name in first:
        assert GA.first_bit_difference(first[name], again[name]) is None, name


def _layer_case(dev, seed=12):
    rng = np.random.RandomState(seed)
    layer = QuaternionLayerNormalization()
    x = torch.tensor(1.5 * rng.randn(4, 9, 40) + 0.5, dtype=torch.float32, device=dev)
    lengths = torch.tensor([9, 4, 7, 1], dtype=torch.int32, device=dev)
    w = torch.tensor(rng.randn(4, 9, 40), dtype=torch.float32, device=dev)
    layer.ensure_built(x.shape, dev)
    with torch.no_grad():
        layer.gamma.add_(torch.tensor(0.3 * rng.randn(10), dtype=torch.float32, device=dev))
        layer.beta.add_(torch.tensor(0.3 * rng.randn(40), dtype=torch.float32, device=dev))
    return layer, x, lengths, w


@pytest.mark.gpu
@pytest.mark.parametrize('with_lengths', [True, False], ids=['lengths', 'all_rows'])
def test_layer_matches_the_float64_composition(with_lengths):
    """fp32, B = 4, T = 9, Q = 10: output, input gradient and both parameter gradients within the fp32 bound 1e-4."""
    dev = _dev()
    layer, x, lengths, w = _layer_case(dev)
    x.requires_grad_()
    y = layer(x, lengths=lengths if with_lengths else None)
    (y * w).sum().backward()
    x64 = x.detach().double().cpu().requires_grad_()
    p64 = [p.detach().double().cpu().requires_grad_() for _, p in layer.weights]
    y64 = R.qlayer_norm_t(x64, p64[0], p64[1], lengths.cpu() if with_lengths else None, epsilon=layer.epsilon)
    (y64 * w.double().cpu()).sum().backward()
    assert _rel(y.detach().cpu().numpy(), y64.detach().numpy()) <= 1e-4 and _rel(x.grad.cpu().numpy(), x64.grad.numpy()) <= 1e-4
    for (name, p), q64 in zip(layer.weights, p64):
        assert _rel(p.grad.cpu().numpy(), q64.grad.numpy()) <= 1e-4, name
    assert tuple(QuaternionLayerNormalization(center=False, scale=False)(x.detach()).shape) == (4, 9, 40)


def _small_model(dev, seed, dropout=0.0):
    """TimitQLSTM(num_layers=2, units=64, layer_norm=True) at B = 4, T = 9 with its batch; parameters fp32, built, the normalisation
    weights moved off their initial ones / zeros."""
    np.random.seed(seed)
    torch.manual_seed(seed)
    model = TimitQLSTM(num_layers=2, units=64, bidirectional=True, dropout=dropout, l2=0.0, layer_norm=True)
    rng = np.random.RandomState(seed + 1)
    x = torch.tensor(rng.randn(4, 4, 41, 9).astype(np.float32), device=dev)
    labels = torch.tensor(rng.randint(0, 61, (4, 3)), device=dev, dtype=torch.int32)
    il = torch.tensor([[9], [7], [8], [5]], dtype=torch.int32, device=dev)
    ll = torch.tensor([[3], [2], [3], [1]], dtype=torch.int32, device=dev)
    model.to(dev)
    with torch.no_grad():
        model(x, il)
    model.to(dev)
    with torch.no_grad():
        for layer in model.norm:
            layer.gamma.add_(torch.tensor(0.2 * rng.randn(*layer.gamma.shape), dtype=torch.float32, device=dev))
            layer.beta.add_(torch.tensor(0.2 * rng.randn(*layer.beta.shape), dtype=torch.float32, device=dev))
    return model, x, labels, il, ll


def _model_reference(model, x, labels, il, ll):
    """mean CTC cost of the float64 composition (qlstm_ref.layer_t + qlnorm_ref.qlayer_norm_t) and its gradients, by parameter name."""
    p64 = {n: p.detach().double().cpu().requires_grad_() for n, p in model.named_parameters()}
    b, _, f, t = x.shape
    o = x.double().cpu().permute(0, 3, 1, 2).reshape(b, t, 4 * f)
    lengths = il.reshape(-1).cpu()
    for k in range(len(model.rnn)):
        o = LR.layer_t(o, p64['rnn.%d.kernel' % k], p64['rnn.%d.recurrent_kernel' % k], p64['rnn.%d.bias' % k], lengths)
        o = R.qlayer_norm_t(o, p64['norm.%d.gamma' % k], p64['norm.%d.beta' % k], lengths, epsilon=model.norm[k].epsilon)
    pred = torch.softmax(o @ p64['pred.layer.kernel'] + p64['pred.layer.bias'], dim=-1)
    logp = torch.log_softmax(torch.log(pred + 1e-7), dim=-1).transpose(0, 1)              # K.ctc_batch_cost (layers.ctc_batch_cost)
    cost = torch.nn.functional.ctc_loss(logp, labels.long().cpu(), lengths.long(), ll.reshape(-1).long().cpu(), blank=61, reduction='none')
    loss = cost.mean()
    loss.backward()
    return float(loss.detach()), {n: p.grad.numpy() for n, p in p64.items()}


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['fp32', 'bf16'])
def test_model_loss_and_gradients_match_the_composition_of_reference_pieces(dtype):
    """TimitQLSTM(2, 64, layer_norm=True) through ctc_mean_loss: fp32 within 1e-4; bf16 activations within 2e-2."""
    dev = _dev()
    model, x, labels, il, ll = _small_model(dev, 31)
    tol = 1e-4 if dtype == torch.float32 else 2e-2
    loss = model.ctc_mean_loss(x.to(dtype), labels, il, ll)
    loss.backward()
    want_loss, want = _model_reference(model, x.to(dtype).float(), labels, il, ll)
    errs = {n: _rel(p.grad.cpu().numpy(), want[n]) for n, p in model.named_parameters()}
    print(float(loss), want_loss, errs)
    assert len(errs) == 2 * 5 + 2 and abs(float(loss) - want_loss) <= tol * abs(want_loss)
    assert max(errs.values()) <= tol, errs


@pytest.mark.gpu
def test_three_guarded_scheduled_steps_lower_the_loss_and_checkpoint(tmp_path):
    """dp.FlatParams, GradGuard, ScheduledAdam and save_checkpoint take the new parameters as they are."""
    from qcnn_amd import dp
    from qcnn_amd.training import GradGuard, LRSchedule, ScheduledAdam, load_checkpoint, save_checkpoint
    dev = _dev()
    model, x, labels, il, ll = _small_model(dev, 41)
    x16 = x.to(torch.bfloat16)
    flat = dp.FlatParams([p for p in model.parameters() if p.requires_grad], direct=True)
    guard = GradGuard(dev, clipnorm=50.0, loss_scale=4.0)
    opt = ScheduledAdam(flat.param, flat.grad, LRSchedule(5e-3), guard=guard)
    losses = []
    for _ in range(3):
        loss = model.training_loss(x16, labels, il, ll, loss_scale=guard.loss_scale)
        loss.backward()
        opt.step()
        losses.append(float(loss))
    with torch.no_grad():
        losses.append(float(model.training_loss(x16, labels, il, ll)))
    print(losses)
    assert opt.stats()['step'] == 3 and guard.stats()['skipped_steps'] == 0
    assert all(np.isfinite(losses)) and losses[3] < losses[0]
    path = str(tmp_path / 'qlstm_norm.pt')
    save_checkpoint(path, model, opt)
    saved = torch.load(path, map_location='cpu', weights_only=True)
    assert {'norm.0.gamma', 'norm.0.beta', 'norm.1.gamma', 'norm.1.beta', 'rnn.1.bias', 'pred.layer.kernel'} <= set(saved['model'])
    before = flat.param.clone()
    flat.param.zero_()
    load_checkpoint(path, model, opt)
    assert torch.equal(flat.param, before) and float(model.norm[1].gamma.detach().abs().min()) > 0
    assert model.evaluate(x16, labels, il, ll).symbols == int(ll.sum())


@pytest.mark.gpu
@pytest.mark.parametrize('dtype,q', [(torch.bfloat16, 72), (torch.float32, 5)], ids=['vec', 'generic'])
def test_forward_and_backward_replay_from_a_captured_graph(dtype, q):
    """functional.qlayer_norm forward + backward captured on one stream and replayed three times: bit-equal to the eager call.  That
    it captures at all shows that the launches read nothing on the host."""
    dev = _dev()
    eager = _run(dev, dtype, q)
    i = _inputs(q, KINDS[dtype])
    t = lambda a, dt=dtype: torch.tensor(a, dtype=dt, device=dev)
    x, dy, ln = t(i['x']).requires_grad_(), t(i['dy']), torch.tensor(i['lengths'], device=dev)
    gamma, beta = t(i['gamma'], torch.float32).requires_grad_(), t(i['beta'], torch.float32).requires_grad_()

    def body():
        y = F.qlayer_norm(x, gamma, beta, ln, epsilon=EPS)
        return (y.detach(),) + torch.autograd.grad(y, (x, gamma, beta), dy)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        body()                                                       # warm-up, eagerly (allocator, code objects)
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize(dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = body()
    for o in outs:
        o.zero_()
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize(dev)
    for name, o in zip(('y', 'dx', 'dgamma', 'dbeta'), outs):
        assert GA.first_bit_difference(o, eager[name]) is None, name


@pytest.mark.gpu
@pytest.mark.parametrize('dtype,q', [(torch.bfloat16, 72), (torch.float32, 5)], ids=['vec_bf16', 'generic'])
def test_forward_and_backward_keep_to_their_buffers(monkeypatch, dtype, q):
    """functional.qlayer_norm forward and backward under guard bands and the two fills: no stray write, every returned element
    written, the two runs bit-identical (nothing depends on what the workspace, the statistics or an output held before the call)."""
    dev = _dev()

    def run(alloc):
        return _run(dev, dtype, q)
    res = GA.run_twice(run, monkeypatch, modules=(F,))
    GA.assert_hygiene(res, 'qlayer_norm %s q=%d: ' % (dtype, q))
    sites = {a.site.split(':')[0] for a in res.allocs[0].log}
    assert sites == {'functional.py'} and len(res.allocs[0].log) == 6        # y, stats, dx, dgamma, dbeta, workspace
