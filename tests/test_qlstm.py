"""The quaternion LSTM (include/qk_rnn.h; qcnn_amd.functional.qlstm, qcnn_amd.complexnn.QuaternionLSTM, qcnn_amd.models.TimitQLSTM)
against the float64 restatement of tests/qlstm_ref.py.

Bounds (relative to max|want| per tensor).  fp32: against the float64 reference, the project's fp32 bound 1e-4.  bf16 / fp16: against
the reference WITH the header's rounding points, at the bounds of tests/test_gpu_parity.py: 16-bit outputs (y, hT, dzx, dh0) 1e-2 /
2e-3, fp32 outputs (dR, dc0, cT) 2e-3 / 1e-3.  test_rounding_points_move_the_reference_by_less_than_the_16_bit_bound shows on the
same inputs that the rounding points alone stay inside 1e-2 / 2e-3 of the float64 reference (the inputs are not degenerate).
"""
import ctypes
import functools
import os
import re

import numpy as np
import pytest
import torch

import guarded_alloc as GA
import qlstm_ref as R
from qcnn_amd import _lib, functional as F
from qcnn_amd.complexnn import QuaternionLSTM
from qcnn_amd.models import TimitQLSTM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = {torch.float32: None, torch.bfloat16: 'bf16', torch.float16: 'fp16'}
BOUND_16 = {'bf16': 1e-2, 'fp16': 2e-3}          # 16-bit outputs
BOUND_32 = {'bf16': 2e-3, 'fp16': 1e-3}          # fp32 outputs of the 16-bit paths
OUT_16, OUT_32 = ('y', 'hT', 'dzx', 'dh0'), ('dR', 'dc0', 'cT')
# the GPU shapes: 70 rows = more than one row tile and a ragged last one; 16 / 48 quaternion units = one and three unit slices, one
# width that is no multiple of 32; 5 = the generic kernel; 7 steps = both h buffers reused several times
B, T, QS = 70, 7, (16, 48, 5)


def _dev():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    return torch.device('cuda:0')


def _rel(got, want):
    return float(np.abs(np.asarray(got, dtype=np.float64) - want).max()) / max(float(np.abs(want).max()), 1e-30)


def _lengths(bsz, steps, seed):
    """lengths that contain 0, 1, steps - 2 and steps, the rest random."""
    rng = np.random.RandomState(seed)
    out = rng.randint(0, steps + 1, size=bsz)
    fixed = [0, 1, steps - 2, steps]
    out[:min(bsz, 4)] = fixed[:min(bsz, 4)]
    return out.astype(np.int32)


@functools.lru_cache(maxsize=None)
def _inputs(q, dirs, kind, bsz=B, steps=T):
    """Seeded operands (never written), 16-bit ones already rounded to `kind`: the recurrent term is of the order of zx."""
    rng = np.random.RandomState(1000 + 16 * q + dirs)
    u = 4 * q
    d = dict(zx=R.rnd(rng.randn(dirs, bsz, steps, 4 * u), kind), R=(0.6 / np.sqrt(q)) * rng.randn(dirs, q, 4 * u).astype(np.float32).astype(np.float64),
             h0=R.rnd(0.5 * rng.randn(dirs, bsz, u), kind), c0=rng.randn(dirs, bsz, u).astype(np.float32).astype(np.float64),
             dy=R.rnd(rng.randn(bsz, steps, dirs * u), kind), dhT=R.rnd(rng.randn(dirs, bsz, u), kind),
             dcT=rng.randn(dirs, bsz, u).astype(np.float32).astype(np.float64), lengths=_lengths(bsz, steps, q))
    for v in d.values():
        v.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def _reference(q, dirs, kind, state, reverse=False, bsz=B, steps=T):
    """The reference's outputs for _inputs(...), computed once and shared."""
    i = _inputs(q, dirs, kind, bsz, steps)
    st = dict(h0=i['h0'], c0=i['c0'], dhT=i['dhT'], dcT=i['dcT']) if state else {}
    return R.qlstm(i['zx'], i['R'], i['lengths'], kind=kind, dy=i['dy'], reverse=reverse, **st)


# ---- CPU part ------------------------------------------------------------------------------------------------------------------
def test_reference_bptt_agrees_with_central_differences():
    """B = 3, T = 4, q_units = 2, both directions, lengths 4 / 2 / 0, every optional input: 1e-7 relative."""
    rng = np.random.RandomState(3)
    dirs, bsz, steps, q = 2, 3, 4, 2
    u = 4 * q
    lengths = np.array([4, 2, 0])
    par = dict(zx=rng.randn(dirs, bsz, steps, 4 * u), r=0.5 * rng.randn(dirs, q, 4 * u), h0=0.5 * rng.randn(dirs, bsz, u),
               c0=rng.randn(dirs, bsz, u))
    wy, wh, wc = rng.randn(bsz, steps, dirs * u), rng.randn(dirs, bsz, u), rng.randn(dirs, bsz, u)

    def loss(p):
        o = R.qlstm(p['zx'], p['r'], lengths, p['h0'], p['c0'])
        return float((o['y'] * wy).sum() + (o['hT'] * wh).sum() + (o['cT'] * wc).sum())
    got = R.qlstm(par['zx'], par['r'], lengths, par['h0'], par['c0'], dy=wy, dhT=wh, dcT=wc)
    eps = 1e-5
    for name, gname in (('zx', 'dzx'), ('r', 'dR'), ('h0', 'dh0'), ('c0', 'dc0')):
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


def test_rnn_header_inventory_equals_the_fourth_symbol_table():
    lib = _lib.lib()
    h = open(os.path.join(ROOT, 'include', 'qk_rnn.h')).read()
    declared = set(re.findall(r'\b(qk_[a-z_0-9]+)\s*\(', h))
    declared -= {n for n in declared if n.endswith('_t')}
    assert declared == set(_lib.RNN_SYMBOLS), declared ^ set(_lib.RNN_SYMBOLS)
    for name in declared:
        assert hasattr(lib, name), name
    for other in (_lib.SYMBOLS, _lib.OPT_SYMBOLS, _lib.DATA_SYMBOLS):
        assert not set(_lib.RNN_SYMBOLS) & set(other)
    main = open(os.path.join(ROOT, 'include', 'qk.h')).read()
    assert not any(name in main for name in _lib.RNN_SYMBOLS)
    decls = {name: (res, args) for res, name, args in re.findall(r'^(int|size_t) (qk_[a-z_0-9]+)\(([^;]*)\);', h, re.M | re.S)}
    assert set(decls) == set(_lib.RNN_SYMBOLS)
    for name, (res, args) in decls.items():
        restype, argtypes = _lib.RNN_SYMBOLS[name]
        assert restype is (ctypes.c_int if res == 'int' else ctypes.c_size_t), name
        assert len(argtypes) == len(args.split(',')), name
        last = ' '.join(args.split(',')[-1].split())
        if name in ('qk_qlstm_fwd', 'qk_qlstm_bwd'):
            assert last == 'void *stream' and argtypes[-1] is ctypes.c_void_p, name
        else:                                                       # host only
            assert 'stream' not in args, name
    body = h[h.index('typedef struct qk_qlstm_desc_t {'):h.index('} qk_qlstm_desc_t;')]
    fields = re.findall(r'^\s*int32_t ([a-z_]+);', body, re.M)
    assert [(n, ctypes.c_int32) for n in fields] == list(_lib.QLSTMDesc._fields_) and ctypes.sizeof(_lib.QLSTMDesc) == 28
    for macro in ('QK_QLSTM_REVERSE', 'QK_QLSTM_PATH_GENERIC', 'QK_QLSTM_PATH_MFMA16'):
        assert int(re.search(r'#define %s (\d+)' % macro, h).group(1)) == getattr(_lib, macro)


def test_dispatch_predicate_and_descriptor_checks_need_no_gpu():
    assert F.qlstm_path(torch.bfloat16, B, T, 16) == F.qlstm_path(torch.float16, B, T, 48, 2) == 'mfma16'
    assert F.qlstm_path(torch.float32, B, T, 16) == F.qlstm_path(torch.bfloat16, B, T, 5) == F.qlstm_path(torch.float16, B, T, 24) == 'generic'
    lib = _lib.lib()
    good = F.qlstm_desc(torch.bfloat16, 4, 3, 16, 2)
    assert lib.qk_qlstm_reserve_bytes(ctypes.byref(good)) == 2 * 3 * 4 * 5 * 64 * 4
    assert lib.qk_qlstm_workspace_bytes(ctypes.byref(good), _lib.QK_OP_FWD) > 0 and lib.qk_qlstm_workspace_bytes(ctypes.byref(good), _lib.QK_OP_BWD) > 0
    for field, value in (('dtype', 7), ('batch', 0), ('steps', 0), ('q_units', 0), ('directions', 3), ('y_stride', 127), ('flags', 1), ('flags', 2)):
        bad = F.qlstm_desc(torch.bfloat16, 4, 3, 16, 2)
        setattr(bad, field, value)
        assert lib.qk_qlstm_supported(ctypes.byref(bad)) == 0, field
        assert lib.qk_qlstm_workspace_bytes(ctypes.byref(bad), _lib.QK_OP_FWD) == 0 and lib.qk_qlstm_reserve_bytes(ctypes.byref(bad)) == 0
        assert lib.qk_qlstm_fwd(ctypes.byref(bad), *([None] * 10), 0, None) == _lib.QK_ERR_INVALID_ARG and lib.qk_last_error()
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        F.qlstm(torch.zeros(1, 2, 3, 64), torch.zeros(1, 4, 64))


def test_layer_surface():
    np.random.seed(4)
    layer = QuaternionLSTM(32, bidirectional=True, seed=7, name='rec')
    layer.ensure_built((None, None, 20), torch.device('cpu'))
    assert [(n, tuple(p.shape)) for n, p in layer.weights] == [('kernel', (2, 5, 128)), ('recurrent_kernel', (2, 8, 128)), ('bias', (2, 128))]
    bias = layer.bias.detach().numpy().reshape(2, 4, 4, 8)               # (direction, component, gate, unit)
    assert (bias[:, :, 1] == 1).all() and (bias[:, :, (0, 2, 3)] == 0).all()
    k = layer.kernel.detach().numpy()
    assert np.abs(k).min() > 0 and not np.allclose(k[0], k[1]) and not np.allclose(k[0, :, :8], k[0, :, 8:16])      # gates drawn independently
    assert layer.compute_output_shape((3, 11, 20)) == (3, 11, 64)
    cfg = layer.get_config()
    assert cfg['units'] == 32 and cfg['bidirectional'] and cfg['seed'] == 7 and cfg['name'] == 'rec' and cfg['unit_forget_bias']
    again = QuaternionLSTM.from_config(cfg)
    assert again.get_config() == cfg
    single = QuaternionLSTM(32, return_sequences=False, return_state=True, go_backwards=True, unit_forget_bias=False)
    single.ensure_built((None, None, 20), torch.device('cpu'))
    assert [tuple(p.shape) for _, p in single.weights] == [(5, 128), (8, 128), (128,)] and float(single.bias.detach().abs().max()) == 0
    assert single.compute_output_shape((3, 11, 20)) == [(3, 32), (3, 32), (3, 32)]
    with pytest.raises(ValueError):
        QuaternionLSTM(30)
    with pytest.raises(ValueError):
        QuaternionLSTM(32, go_backwards=True, bidirectional=True)
    model = TimitQLSTM(num_layers=3, units=32, bidirectional=False, dropout=0.0)
    assert len(model.rnn) == 3 and model.rnn[0].units == 32 and not model.rnn[0].bidirectional


def test_reference_rows_of_length_zero_and_full_length():
    """A length-0 row keeps its state, outputs zeros and passes dhT / dcT through; a length-T row equals the call without lengths."""
    i = _inputs(5, 2, None, bsz=4, steps=T)
    o = _reference(5, 2, None, True, bsz=4, steps=T)
    assert list(i['lengths']) == [0, 1, T - 2, T]
    assert (o['y'][0] == 0).all() and (o['dzx'][:, 0] == 0).all() and (o['hprev'][:, 0] == 0).all()
    assert (o['hT'][:, 0] == i['h0'][:, 0]).all() and (o['cT'][:, 0] == i['c0'][:, 0]).all()
    assert (o['dh0'][:, 0] == i['dhT'][:, 0]).all() and (o['dc0'][:, 0] == i['dcT'][:, 0]).all()
    assert (o['y'][1, 1:] == 0).all() and np.abs(o['y'][1, 0]).min() > 0 and (o['dzx'][:, 1, 1:] == 0).all()
    full = R.qlstm(i['zx'][:, 3:], i['R'], None, i['h0'][:, 3:], i['c0'][:, 3:], dy=i['dy'][3:], dhT=i['dhT'][:, 3:], dcT=i['dcT'][:, 3:])
    for name in ('y', 'hT', 'cT', 'dh0', 'dc0'):
        row = o[name][3:] if name == 'y' else o[name][:, 3:]
        assert np.allclose(row, full[name], rtol=0, atol=1e-12), name           # (1e-12: the matrix products see another batch size)
    assert np.allclose(o['dzx'][:, 3:], full['dzx'], rtol=0, atol=1e-12)
    # the backward direction of a short row starts from h0 / c0 at its own last frame: reversing the row's frames gives the forward walk
    fwd = R.qlstm(i['zx'][1:2, 2:3, :T - 2][:, :, ::-1], i['R'][1:2], None, i['h0'][1:2, 2:3], i['c0'][1:2, 2:3])
    u = i['h0'].shape[-1]
    back = np.stack([o['y'][2, :T - 2].reshape(T - 2, 4, 2, u // 4)[:, :, 1]], axis=0).reshape(1, T - 2, u)
    assert np.allclose(back[:, ::-1], fwd['y'], rtol=0, atol=1e-12)


@pytest.mark.parametrize('kind', ['bf16', 'fp16'])
@pytest.mark.parametrize('q', QS)
def test_rounding_points_move_the_reference_by_less_than_the_16_bit_bound(q, kind):
    """On the GPU tests' own inputs: the reference with rounding points stays within 1e-2 (bf16) / 2e-3 (fp16) of the float64 one,
    and is not identical to it (the rounding points are in play)."""
    i = _inputs(q, 2, kind)
    pure = R.qlstm(i['zx'], i['R'], i['lengths'], i['h0'], i['c0'], dy=i['dy'], dhT=i['dhT'], dcT=i['dcT'])
    rounded = _reference(q, 2, kind, True)
    errs = {name: _rel(rounded[name], pure[name]) for name in OUT_16 + OUT_32}
    print(q, kind, errs)
    assert max(errs.values()) <= BOUND_16[kind], errs
    assert min(errs[name] for name in ('y', 'dzx', 'dR')) > 1e-5, errs


# every entry of RNN_SYMBOLS against the hygiene case that exercises it, or the reason it has none
HYGIENE_COVER = {
    'qk_qlstm_fwd': 'test_forward_and_backward_keep_to_their_buffers: mfma16 (two directions, states, lengths) and generic',
    'qk_qlstm_bwd': 'test_forward_and_backward_keep_to_their_buffers: the same calls',
    'qk_qlstm_supported': 'host only: takes no device buffer (test_dispatch_predicate_and_descriptor_checks_need_no_gpu)',
    'qk_qlstm_workspace_bytes': 'host only: *_bytes',
    'qk_qlstm_reserve_bytes': 'host only: *_bytes',
}


def test_every_rnn_entry_point_has_a_hygiene_case_or_a_reason():
    assert set(HYGIENE_COVER) == set(_lib.RNN_SYMBOLS)


# ---- GPU part ------------------------------------------------------------------------------------------------------------------
def _run(dev, dtype, q, dirs, state, reverse=False, lengths=True, bsz=B, steps=T, select=None):
    """functional.qlstm forward and backward on _inputs(...) [direction `select` of them]: name -> tensor."""
    i = _inputs(q, dirs, KINDS[dtype], bsz, steps)
    pick = (lambda a: a) if select is None else (lambda a: a[select:select + 1])
    t = lambda a, dt=dtype: torch.tensor(a, dtype=dt, device=dev)
    zx, Rw = t(pick(i['zx'])).requires_grad_(), t(pick(i['R']), torch.float32).requires_grad_()
    h0 = t(pick(i['h0'])).requires_grad_() if state else None
    c0 = t(pick(i['c0']), torch.float32).requires_grad_() if state else None
    ln = torch.tensor(i['lengths'], device=dev) if lengths else None
    y, hT, cT = F.qlstm(zx, Rw, ln, h0, c0, reverse=reverse)
    dy = i['dy'] if select is None else R._split(i['dy'], dirs, q)[select]
    outs, grads = [y], [t(dy)]
    if state:
        outs += [hT, cT]
        grads += [t(pick(i['dhT'])), t(pick(i['dcT']), torch.float32)]
    torch.autograd.backward(outs, grads)
    res = dict(y=y.detach(), hT=hT.detach(), cT=cT.detach(), dzx=zx.grad, dR=Rw.grad)
    if state:
        res.update(dh0=h0.grad, dc0=c0.grad)
    return res


@pytest.mark.gpu
@pytest.mark.parametrize('state', [False, True], ids=['zero_state', 'h0_c0_dhT_dcT'])
@pytest.mark.parametrize('dirs', [1, 2])
@pytest.mark.parametrize('q', QS)
@pytest.mark.parametrize('dtype', list(KINDS), ids=['fp32', 'bf16', 'fp16'])
def test_forward_and_backward_match_the_reference(dtype, q, dirs, state):
    dev = _dev()
    kind = KINDS[dtype]
    assert F.qlstm_path(dtype, B, T, q, dirs) == ('mfma16' if kind and q % 16 == 0 else 'generic')
    with _lib.debug_flags(_lib.QK_DBG_DETERMINISTIC):
        got = _run(dev, dtype, q, dirs, state)
    want = _reference(q, dirs, kind, state)
    errs = {}
    for name, g in got.items():
        assert g.dtype == (torch.float32 if name in OUT_32 else dtype) and tuple(g.shape) == want[name].shape, name
        errs[name] = (_rel(g.float().cpu().numpy(), want[name]), 1e-4 if kind is None else BOUND_16[kind] if name in OUT_16 else BOUND_32[kind])
    print(errs)
    assert all(e <= b for e, b in errs.values()), errs
    # asserted, not tolerated: inactive positions are exactly zero; a row of length 0 returns its initial state bit for bit
    ln = _inputs(q, dirs, kind)['lengths']
    inactive = torch.tensor(np.arange(T)[None, :] >= ln[:, None], device=dev)
    assert int(got['y'][inactive].ne(0).sum()) == 0 and int(got['dzx'][:, inactive].ne(0).sum()) == 0
    i = _inputs(q, dirs, kind)
    assert ln[0] == 0
    h_init = torch.tensor(i['h0'][:, 0], dtype=dtype, device=dev) if state else torch.zeros_like(got['hT'][:, 0])
    c_init = torch.tensor(i['c0'][:, 0], dtype=torch.float32, device=dev) if state else torch.zeros_like(got['cT'][:, 0])
    assert GA.first_bit_difference(got['hT'][:, 0], h_init) is None and GA.first_bit_difference(got['cT'][:, 0], c_init) is None


@pytest.mark.gpu
@pytest.mark.parametrize('dtype,q', [(torch.bfloat16, 48), (torch.float32, 5)], ids=['mfma16', 'generic'])
def test_two_directions_equal_two_single_direction_calls_and_calls_repeat_bit_for_bit(dtype, q):
    dev = _dev()
    with _lib.debug_flags(_lib.QK_DBG_DETERMINISTIC):
        both, again = _run(dev, dtype, q, 2, True), _run(dev, dtype, q, 2, True)
        fwd, bwd = _run(dev, dtype, q, 2, True, select=0), _run(dev, dtype, q, 2, True, reverse=True, select=1)
    for name in both:                                              # no atomics in the recurrence
        assert GA.first_bit_difference(both[name], again[name]) is None, name
    for d, one in enumerate((fwd, bwd)):
        y_d = both['y'].reshape(B, T, 4, 2, q)[:, :, :, d].reshape(B, T, 4 * q)
        assert GA.first_bit_difference(y_d, one['y']) is None, d
        for name in ('hT', 'cT', 'dzx', 'dR', 'dh0', 'dc0'):
            assert GA.first_bit_difference(both[name][d:d + 1], one[name]) is None, (d, name)


@pytest.mark.gpu
def test_call_without_lengths_and_three_dimensional_form():
    dev = _dev()
    got = _run(dev, torch.bfloat16, 16, 1, False, lengths=False)
    i = _inputs(16, 1, 'bf16')
    want = R.qlstm(i['zx'], i['R'], None, kind='bf16', dy=i['dy'])
    for name in ('y', 'hT', 'dzx'):
        assert _rel(got[name].float().cpu().numpy(), want[name]) <= BOUND_16['bf16'], name
    for name in ('cT', 'dR'):
        assert _rel(got[name].float().cpu().numpy(), want[name]) <= BOUND_32['bf16'], name
    t = lambda a, dt=torch.bfloat16: torch.tensor(a, dtype=dt, device=dev)
    y3, h3, c3 = F.qlstm(t(i['zx'][0]), t(i['R'][0], torch.float32))
    assert tuple(h3.shape) == tuple(c3.shape) == (B, 64) and GA.first_bit_difference(y3, got['y']) is None


def _layer_case(dev, dtype, bidirectional, go_backwards=False):
    np.random.seed(12)
    layer = QuaternionLSTM(64, bidirectional=bidirectional, go_backwards=go_backwards, seed=5)
    rng = np.random.RandomState(13)
    x = torch.tensor(rng.randn(4, 9, 20), dtype=dtype, device=dev)
    lengths = torch.tensor([9, 4, 7, 1], dtype=torch.int32, device=dev)
    w = torch.tensor(rng.randn(4, 9, 64 * (2 if bidirectional else 1)), dtype=torch.float32, device=dev)
    return layer, x, lengths, w


@pytest.mark.gpu
@pytest.mark.parametrize('mode', ['forward', 'backwards', 'bidirectional'])
def test_layer_matches_the_composition_of_reference_pieces(mode):
    """fp32, B = 4, T = 9: output and every parameter gradient within the fp32 bound 1e-4 of the float64 composition."""
    dev = _dev()
    layer, x, lengths, w = _layer_case(dev, torch.float32, mode == 'bidirectional', mode == 'backwards')
    y = layer(x, lengths=lengths)
    (y * w).sum().backward()
    p64 = [p.detach().double().cpu().requires_grad_() for _, p in layer.weights]
    y64 = R.layer_t(x.double().cpu(), p64[0], p64[1], p64[2], lengths.cpu(), go_backwards=mode == 'backwards')
    (y64 * w.double().cpu()).sum().backward()
    assert _rel(y.detach().cpu().numpy(), y64.detach().numpy()) <= 1e-4
    for (name, p), q64 in zip(layer.weights, p64):
        assert _rel(p.grad.cpu().numpy(), q64.grad.numpy()) <= 1e-4, name
    out, hT, cT = QuaternionLSTM(64, return_sequences=False, return_state=True, seed=5)(x, lengths=lengths)
    assert tuple(out.shape) == tuple(hT.shape) == tuple(cT.shape) == (4, 64) and torch.equal(out, hT)


def _small_model(dev, seed, dropout=0.0):
    """TimitQLSTM(num_layers=2, units=64) at B = 4, T = 9 with its batch; parameters fp32, built."""
    np.random.seed(seed)
    torch.manual_seed(seed)
    model = TimitQLSTM(num_layers=2, units=64, bidirectional=True, dropout=dropout, l2=0.0)
    rng = np.random.RandomState(seed + 1)
    x = torch.tensor(rng.randn(4, 4, 41, 9).astype(np.float32), device=dev)
    labels = torch.tensor(rng.randint(0, 61, (4, 3)), device=dev, dtype=torch.int32)
    il = torch.tensor([[9], [7], [8], [5]], dtype=torch.int32, device=dev)
    ll = torch.tensor([[3], [2], [3], [1]], dtype=torch.int32, device=dev)
    model.to(dev)
    with torch.no_grad():
        model(x, il)
    model.to(dev)
    return model, x, labels, il, ll


def _model_reference(model, x, labels, il, ll):
    """mean CTC cost of the float64 composition and its gradients, by parameter name."""
    p64 = {n: p.detach().double().cpu().requires_grad_() for n, p in model.named_parameters()}
    b, _, f, t = x.shape
    o = x.double().cpu().permute(0, 3, 1, 2).reshape(b, t, 4 * f)
    lengths = il.reshape(-1).cpu()
    for k in range(len(model.rnn)):
        o = R.layer_t(o, p64['rnn.%d.kernel' % k], p64['rnn.%d.recurrent_kernel' % k], p64['rnn.%d.bias' % k], lengths)
    pred = torch.softmax(o @ p64['pred.layer.kernel'] + p64['pred.layer.bias'], dim=-1)
    logp = torch.log_softmax(torch.log(pred + 1e-7), dim=-1).transpose(0, 1)              # K.ctc_batch_cost (layers.ctc_batch_cost)
    cost = torch.nn.functional.ctc_loss(logp, labels.long().cpu(), lengths.long(), ll.reshape(-1).long().cpu(), blank=61, reduction='none')
    loss = cost.mean()
    loss.backward()
    return float(loss), {n: p.grad.numpy() for n, p in p64.items()}


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['fp32', 'bf16'])
def test_model_loss_and_gradients_match_the_composition_of_reference_pieces(dtype):
    """TimitQLSTM(2, 64) through ctc_mean_loss: fp32 within 1e-4; bf16 activations within 2e-2, the bound tests/test_timit_parity.py
    holds the bf16 TimitQCNN to against its float64 composition."""
    dev = _dev()
    model, x, labels, il, ll = _small_model(dev, 31)
    tol = 1e-4 if dtype == torch.float32 else 2e-2
    loss = model.ctc_mean_loss(x.to(dtype), labels, il, ll)
    loss.backward()
    want_loss, want = _model_reference(model, x.to(dtype).float(), labels, il, ll)
    errs = {n: _rel(p.grad.cpu().numpy(), want[n]) for n, p in model.named_parameters()}
    print(float(loss), want_loss, errs)
    assert len(errs) == 2 * 3 + 2 and abs(float(loss) - want_loss) <= tol * abs(want_loss)
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
    path = str(tmp_path / 'qlstm.pt')
    save_checkpoint(path, model, opt)
    saved = torch.load(path, map_location='cpu', weights_only=True)
    assert {'rnn.0.kernel', 'rnn.1.recurrent_kernel', 'rnn.1.bias', 'pred.layer.kernel'} <= set(saved['model'])
    before = flat.param.clone()
    flat.param.zero_()
    load_checkpoint(path, model, opt)
    assert torch.equal(flat.param, before)
    decoded, _ = model.decode(x16, il)
    assert decoded[0].shape[0] == 4
    assert model.evaluate(x16, labels, il, ll).symbols == int(ll.sum())


@pytest.mark.gpu
def test_training_step_replays_in_a_captured_graph():
    """The whole step of the small model (dropout off) -- loss, backward, guarded Adam -- captured on one stream and replayed three
    times: bit-equal to three eager steps of a twin.  That it captures at all shows that the T launches read nothing on the host."""
    from qcnn_amd import dp
    from qcnn_amd.training import GradGuard
    dev = _dev()

    def fresh():
        model, x, labels, il, ll = _small_model(dev, 51)
        flat = dp.FlatParams([p for p in model.parameters() if p.requires_grad])
        s = dict(model=model, flat=flat, m=torch.zeros_like(flat.param), v=torch.zeros_like(flat.param),
                 t=torch.zeros(1, dtype=torch.int32, device=dev), guard=GradGuard(dev, clipnorm=50.0, loss_scale=4.0),
                 batch=(x.to(torch.bfloat16), labels, il, ll), loss=torch.zeros((), device=dev))
        return s

    def body(s):
        loss = s['model'].training_loss(*s['batch'], loss_scale=s['guard'].loss_scale)
        loss.backward()
        s['loss'].copy_(loss.detach().float())
        s['guard'].step(s['flat'].param, s['flat'].grad, s['m'], s['v'], s['t'], lr=5e-3, zero_grad=True)

    with _lib.debug_flags(_lib.QK_DBG_DETERMINISTIC):
        eager = fresh()
        for _ in range(4):                                           # one warm-up step and three more
            body(eager)
        rep = fresh()
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            body(rep)                                                # the warm-up step, eagerly (allocator, code objects)
        torch.cuda.current_stream(dev).wait_stream(side)
        torch.cuda.synchronize(dev)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            body(rep)
        for _ in range(3):
            graph.replay()
        torch.cuda.synchronize(dev)
    assert int(rep['t']) == int(eager['t']) == 4
    assert GA.first_bit_difference(rep['loss'], eager['loss']) is None
    assert GA.first_bit_difference(rep['flat'].param, eager['flat'].param) is None


@pytest.mark.gpu
@pytest.mark.parametrize('dtype,q,dirs', [(torch.bfloat16, 48, 2), (torch.float16, 16, 1), (torch.float32, 5, 2)], ids=['mfma16_bf16', 'mfma16_fp16', 'generic'])
def test_forward_and_backward_keep_to_their_buffers(monkeypatch, dtype, q, dirs):
    """functional.qlstm forward and backward under guard bands and the two fills: no stray write, every output element written, the
    two runs bit-identical (nothing depends on what the workspace, the reserve or an output held before the call)."""
    dev = _dev()

    def run(alloc):
        return _run(dev, dtype, q, dirs, True)
    with _lib.debug_flags(_lib.QK_DBG_DETERMINISTIC):
        res = GA.run_twice(run, monkeypatch, modules=(F,))
    GA.assert_hygiene(res, 'qlstm %s q=%d D=%d: ' % (dtype, q, dirs))
    sites = {a.site.split(':')[0] for a in res.allocs[0].log}
    assert sites == {'functional.py'} and len(res.allocs[0].log) >= 10      # y, hT, cT, workspace, reserve, dzx, hprev, dh0, dc0, workspace, dR
