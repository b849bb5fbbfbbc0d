"""Depthwise quaternion convolution with a fused GLU gate (include/qk_dwconv.h; qcnn_amd.functional.qdwconv1d / qglu_dwconv1d,
qcnn_amd.complexnn.QuaternionDepthwiseConv1D / QuaternionConformerConvModule / QuaternionConformerBlock,
qcnn_amd.models.TimitQConformer) against the float64 restatement of tests/qdwconv_ref.py.

Bounds (relative to max|want| per tensor).  fp32: against the float64 reference, the project's fp32 bound 1e-4.  bf16 / fp16: against
the reference WITH the header's three rounding points, at the bounds of tests/test_gpu_parity.py: 16-bit outputs (y, da, dg) 1e-2 /
2e-3, fp32 outputs (dw, dbias) 2e-3 / 1e-3.  test_rounding_points_move_the_reference_by_less_than_half_the_16_bit_bound shows on the
same inputs that the rounding points alone stay inside half of those bounds.
"""
import ctypes
import functools
import os
import re

import numpy as np
import pytest
import torch

import guarded_alloc as GA
import lattice_ref as LAT
import qdwconv_ref as R
from qcnn_amd import _lib, functional as F
from qcnn_amd.complexnn import QuaternionConformerBlock, QuaternionConformerConvModule, QuaternionDepthwiseConv1D
from qcnn_amd.models import TimitQCNN, TimitQConformer, TimitQLSTM, TimitQTransformer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = {torch.float32: None, torch.bfloat16: 'bf16', torch.float16: 'fp16'}
DTYPE_IDS = ['fp32', 'bf16', 'fp16']
BOUND_16 = {'bf16': 1e-2, 'fp16': 2e-3}          # 16-bit outputs
BOUND_32 = {'bf16': 2e-3, 'fp16': 1e-3}          # fp32 outputs of the 16-bit paths
OUT_16, OUT_32 = ('y', 'da', 'dg'), ('dw', 'dbias')
# the GPU shapes: the vector kernels' tile is 64 frames, so T = 150 is two tiles and a ragged third of 22 frames (the 32-frame tiles
# of the backward-weight kernel: four and a ragged fifth); the lengths put a row's end at 0, at 1, on a tile border, one past it,
# inside the last tile and at T.  8 quaternion units = the smallest vector width (three quarters of a workgroup's lanes idle), 72 =
# two unit blocks of 32 and a ragged third, 5 = the generic kernels.
TILE = 64
B, T, QS = 6, 150, (8, 72, 5)
LENGTHS = np.array([0, 1, TILE, TILE + 1, T - 2, T], dtype=np.int32)
TAPS = ((1, 'same'), (3, 'same'), (15, 'same'), (31, 'same'), (15, 'causal'))
TAP_IDS = ['k1', 'k3', 'k15', 'k31', 'k15_causal']


def _dev():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    return torch.device('cuda:0')


def _rel(got, want):
    return float(np.abs(np.asarray(got, dtype=np.float64) - want).max()) / max(float(np.abs(want).max()), 1e-30)


def _f32(a):
    return a.astype(np.float32).astype(np.float64)


def _expected_path(dtype, q):
    return 'vec' if q % (4 if dtype == torch.float32 else 8) == 0 else 'generic'


@functools.lru_cache(maxsize=None)
def _inputs(q, taps, kind):
    """Seeded operands (never written), 16-bit ones already rounded to `kind`; the kernel and the bias are fp32 values."""
    rng = np.random.RandomState(3000 + 37 * q + taps)
    d = dict(a=R.rnd(_f32(rng.randn(B, T, 4 * q)), kind), g=R.rnd(_f32(1.5 * rng.randn(B, T, 4 * q)), kind),
             dy=R.rnd(_f32(rng.randn(B, T, 4 * q)), kind), w=_f32(rng.randn(taps, 4 * q) / np.sqrt(taps)), bias=_f32(0.3 * rng.randn(4 * q)))
    for v in d.values():
        v.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def _reference(q, taps, padding, kind, gated=True, rounded=True):
    """The reference's outputs for _inputs(...), computed once and shared."""
    i = _inputs(q, taps, kind)
    return R.qdwconv(i['a'], i['w'], i['bias'], i['g'] if gated else None, LENGTHS, padding, kind if rounded else None, i['dy'])


# ---- CPU part ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('gated', [True, False], ids=['gated', 'plain'])
@pytest.mark.parametrize('padding', ['same', 'causal'])
def test_reference_backward_agrees_with_central_differences(padding, gated):
    """B 2, T 5, Q 2, K 3, lengths 5 / 2: 1e-7 relative for da, dg, dw, dbias."""
    rng = np.random.RandomState(5)
    lengths = np.array([5, 2])
    par = dict(a=rng.randn(2, 5, 8), g=rng.randn(2, 5, 8), w=rng.randn(3, 8), bias=rng.randn(8))
    dy = rng.randn(2, 5, 8)

    def run(p, d=None):
        return R.qdwconv(p['a'], p['w'], p['bias'], p['g'] if gated else None, lengths, padding, dy=d)
    got = run(par, dy)
    eps = 1e-5
    for name, gname in (('a', 'da'), ('g', 'dg'), ('w', 'dw'), ('bias', 'dbias')):
        if name == 'g' and not gated:
            assert got['dg'] is None
            continue
        want = np.zeros_like(par[name])
        flat, wflat = par[name].reshape(-1), want.reshape(-1)
        for k in range(flat.size):
            keep = flat[k]
            flat[k] = keep + eps
            up = float((run(par)['y'] * dy).sum())
            flat[k] = keep - eps
            wflat[k] = (up - float((run(par)['y'] * dy).sum())) / (2 * eps)
            flat[k] = keep
        assert float(np.abs(want).max()) > 0.1 and _rel(got[gname], want) <= 1e-7, (gname, _rel(got[gname], want))
    # rows t >= lengths[b] take no gradient and give zeros
    assert (got['y'][1, 2:] == 0).all() and (got['da'][1, 2:] == 0).all() and np.abs(got['y'][1, :2]).min() > 0


@pytest.mark.parametrize('taps,padding', [(1, 'same'), (4, 'same'), (5, 'causal')])
def test_reference_forward_equals_a_grouped_real_convolution(taps, padding):
    """The plain forward against torch's conv1d(groups=Q) in float64 with the 4 x 4 real block of every tap written out by hand:
    the Hamilton table and the component-major layout, independently.  1e-12."""
    rng = np.random.RandomState(8)
    bsz, steps, q = 3, 9, 5
    x, w, bias = rng.randn(bsz, steps, 4 * q), rng.randn(taps, 4 * q), rng.randn(4 * q)
    wr, wi, wj, wk = (torch.tensor(w[:, c * q:(c + 1) * q]) for c in range(4))             # (K, Q) each
    block = [[wr, -wi, -wj, -wk],                                                           # y_r from h_r h_i h_j h_k
             [wi, wr, -wk, wj],                                                             # y_i
             [wj, wk, wr, -wi],                                                             # y_j
             [wk, -wj, wi, wr]]                                                             # y_k
    weight = torch.zeros(4 * q, 4, taps, dtype=torch.float64)                               # channel u * 4 + c: a group is one unit
    for co in range(4):
        for ci in range(4):
            weight[co::4, ci, :] = block[co][ci].transpose(0, 1)
    xin = torch.tensor(x).reshape(bsz, steps, 4, q).permute(0, 3, 2, 1).reshape(bsz, 4 * q, steps)
    lo = R.pad_lo_of(taps, padding)
    out = torch.nn.functional.conv1d(torch.nn.functional.pad(xin, (lo, taps - 1 - lo)), weight,
                                     torch.tensor(bias).reshape(4, q).transpose(0, 1).reshape(-1), groups=q)
    want = out.reshape(bsz, q, 4, steps).permute(0, 3, 2, 1).reshape(bsz, steps, 4 * q).numpy()
    got = R.qdwconv(x, w, bias, None, None, padding)['y']
    assert np.abs(got - want).max() <= 1e-12
    assert np.abs(R.qdwconv_t(torch.tensor(x), torch.tensor(w), torch.tensor(bias), None, None, padding).numpy() - want).max() <= 1e-12


def test_dwconv_header_inventory_equals_the_seventh_symbol_table():
    lib = _lib.lib()
    h = open(os.path.join(ROOT, 'include', 'qk_dwconv.h')).read()
    declared = set(re.findall(r'\b(qk_[a-z_0-9]+)\s*\(', h))
    declared -= {n for n in declared if n.endswith('_t')}
    assert declared == set(_lib.DWCONV_SYMBOLS), declared ^ set(_lib.DWCONV_SYMBOLS)
    for name in declared:
        assert hasattr(lib, name), name
    for other in (_lib.SYMBOLS, _lib.OPT_SYMBOLS, _lib.DATA_SYMBOLS, _lib.RNN_SYMBOLS, _lib.NORM_SYMBOLS, _lib.ATTN_SYMBOLS):
        assert not set(_lib.DWCONV_SYMBOLS) & set(other)
    main = open(os.path.join(ROOT, 'include', 'qk.h')).read()
    assert not any(name in main for name in _lib.DWCONV_SYMBOLS) and 'qdwconv' not in main
    decls = {name: (res, args) for res, name, args in re.findall(r'^(int|size_t) (qk_[a-z_0-9]+)\(([^;]*)\);', h, re.M | re.S)}
    assert set(decls) == set(_lib.DWCONV_SYMBOLS)
    for name, (res, args) in decls.items():
        restype, argtypes = _lib.DWCONV_SYMBOLS[name]
        assert restype is (ctypes.c_int if res == 'int' else ctypes.c_size_t), name
        assert len(argtypes) == (0 if args.strip() == 'void' else len(args.split(','))), name
        last = ' '.join(args.split(',')[-1].split())
        if name in ('qk_qdwconv_fwd', 'qk_qdwconv_bwd'):
            assert last == 'void *stream' and argtypes[-1] is ctypes.c_void_p, name
        else:                                                       # host only
            assert 'stream' not in args, name
    body = h[h.index('typedef struct qk_qdwconv_desc_t {'):h.index('} qk_qdwconv_desc_t;')]
    fields = re.findall(r'^\s*int32_t ([a-z_]+);', body, re.M)
    assert fields == ['dtype', 'batch', 'steps', 'units', 'taps', 'pad_lo', 'x_row', 'x_comp', 'y_row', 'y_comp', 'flags']
    assert [(n, ctypes.c_int32) for n in fields] == list(_lib.QDWConvDesc._fields_) and ctypes.sizeof(_lib.QDWConvDesc) == 44
    for macro in ('QK_QDWCONV_PATH_GENERIC', 'QK_QDWCONV_PATH_VEC'):
        assert int(re.search(r'#define %s (\d+)' % macro, h).group(1)) == getattr(_lib, macro)
    assert lib.qk_version() == 103


def test_dispatch_predicate_and_descriptor_checks_need_no_gpu():
    lib = _lib.lib()
    sup = lambda d: lib.qk_qdwconv_supported(ctypes.byref(d))
    for dtype, q in ((torch.bfloat16, 8), (torch.float16, 72), (torch.bfloat16, 128), (torch.float32, 4), (torch.float32, 72),
                     (torch.bfloat16, 5), (torch.float16, 4), (torch.bfloat16, 12), (torch.float32, 6), (torch.float32, 5)):
        for packed in (False, True):
            assert F.qdwconv_path(dtype, B, T, q, 15, packed=packed) == _expected_path(dtype, q), (dtype, q, packed)
    assert [_expected_path(torch.bfloat16, q) for q in QS] == ['vec', 'vec', 'generic']
    # strides that break the 16-byte alignment of a run send a vector width to the generic kernels
    assert sup(F.qdwconv_desc(torch.bfloat16, B, T, 8, 15, 7, x=(72, 16))) == _lib.QK_QDWCONV_PATH_VEC
    assert sup(F.qdwconv_desc(torch.bfloat16, B, T, 8, 15, 7, x=(68, 16))) == _lib.QK_QDWCONV_PATH_GENERIC
    assert sup(F.qdwconv_desc(torch.bfloat16, B, T, 8, 15, 7, x=(72, 12))) == _lib.QK_QDWCONV_PATH_GENERIC
    assert sup(F.qdwconv_desc(torch.float32, B, T, 4, 15, 7, y=(18, 4))) == sup(F.qdwconv_desc(torch.float16, B, T, 8, 3, 1, y=(36, 9))) \
        == _lib.QK_QDWCONV_PATH_GENERIC
    good = F.qdwconv_desc(torch.bfloat16, B, T, 72, 15, 7)
    assert lib.qk_qdwconv_workspace_bytes(ctypes.byref(good), _lib.QK_OP_BWD) == B * 16 * 4 * 72 * 4       # six slabs of one row
    assert lib.qk_qdwconv_workspace_bytes(ctypes.byref(good), _lib.QK_OP_FWD) == 0
    big = F.qdwconv_desc(torch.bfloat16, 256, 200, 128, 15, 7)                                              # 128 slabs of two rows
    assert lib.qk_qdwconv_workspace_bytes(ctypes.byref(big), _lib.QK_OP_BWD) == 128 * 16 * 512 * 4
    odd = F.qdwconv_desc(torch.bfloat16, 300, 200, 128, 31, 15)                                             # r = 3: 100 slabs
    assert lib.qk_qdwconv_workspace_bytes(ctypes.byref(odd), _lib.QK_OP_BWD) == 100 * 32 * 512 * 4
    for field, value in (('dtype', 7), ('batch', 0), ('steps', 0), ('units', 0), ('taps', 0), ('taps', 32), ('pad_lo', 15), ('pad_lo', -1),
                         ('x_comp', 71), ('y_comp', 71), ('x_row', 287), ('y_row', 287), ('flags', 1)):
        bad = F.qdwconv_desc(torch.bfloat16, B, T, 72, 15, 7)
        setattr(bad, field, value)
        assert sup(bad) == 0 and lib.qk_last_error(), field
        assert lib.qk_qdwconv_workspace_bytes(ctypes.byref(bad), _lib.QK_OP_BWD) == 0, field
        assert lib.qk_qdwconv_fwd(ctypes.byref(bad), *([None] * 7)) == _lib.QK_ERR_INVALID_ARG, field
        assert lib.qk_qdwconv_bwd(ctypes.byref(bad), *([None] * 10), 0, None) == _lib.QK_ERR_INVALID_ARG, field
    assert lib.qk_qdwconv_fwd(ctypes.byref(good), *([None] * 7)) == _lib.QK_ERR_INVALID_ARG                # NULL buffers
    assert F.qdwconv_pad_lo(15, 'same') == 7 and F.qdwconv_pad_lo(4, 'same') == 1 and F.qdwconv_pad_lo(15, 'causal') == 14
    with pytest.raises(ValueError):
        F.qdwconv_pad_lo(15, 'valid')
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        F.qdwconv1d(torch.zeros(2, 3, 32), torch.zeros(3, 32))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        QuaternionDepthwiseConv1D(3)(torch.zeros(2, 3, 32))


PER_BLOCK = ['norm_ff1.gamma', 'norm_ff1.beta', 'ff1_in.r', 'ff1_in.bias', 'ff1_out.r', 'ff1_out.bias', 'norm_mha.gamma', 'norm_mha.beta',
             'attention.kernel', 'attention.bias', 'attention.out_kernel', 'attention.out_bias', 'norm_conv.gamma', 'norm_conv.beta',
             'conv.pw1.r', 'conv.pw1.bias', 'conv.depthwise.kernel', 'conv.depthwise.bias', 'conv.norm.gamma', 'conv.norm.beta',
             'conv.pw2.r', 'conv.pw2.bias', 'norm_ff2.gamma', 'norm_ff2.beta', 'ff2_in.r', 'ff2_in.bias', 'ff2_out.r', 'ff2_out.bias',
             'norm_out.gamma', 'norm_out.beta']


def test_layer_block_and_model_surface():
    cpu = torch.device('cpu')
    layer = QuaternionDepthwiseConv1D(7, padding='causal', name='dw', seed=3)
    layer.ensure_built((None, None, 40), cpu)
    assert [(n, tuple(p.shape)) for n, p in layer.weights] == [('kernel', (7, 40)), ('bias', (40,))]
    assert float(layer.bias.detach().abs().max()) == 0 and float(layer.kernel.detach().abs().min()) > 0
    # the polar initialiser at the depthwise fan-in: modulus ~ Rayleigh(1 / sqrt(2 K)), so E|w|^2 = 2 s^2 = 1 / K per quaternion
    big = QuaternionDepthwiseConv1D(15, seed=3)
    big.ensure_built((None, None, 4 * 512), cpu)
    assert abs(float((big.kernel.detach() ** 2).sum()) / (15 * 512) * 15 - 1.0) < 0.05
    assert layer.compute_output_shape((3, 11, 40)) == (3, 11, 40)
    cfg = layer.get_config()
    assert cfg['kernel_size'] == 7 and cfg['padding'] == 'causal' and cfg['gated'] is False and cfg['use_bias'] and cfg['name'] == 'dw'
    assert QuaternionDepthwiseConv1D.from_config(cfg).get_config() == cfg
    gated = QuaternionDepthwiseConv1D(5, gated=True, use_bias=False)
    gated.ensure_built((None, None, 80), cpu)
    assert [(n, tuple(p.shape)) for n, p in gated.weights] == [('kernel', (5, 40))] and gated.compute_output_shape((3, 11, 80)) == (3, 11, 40)
    for bad in (dict(kernel_size=0), dict(kernel_size=32), dict(kernel_size=3, padding='valid')):
        with pytest.raises(ValueError):
            QuaternionDepthwiseConv1D(**bad)
    with pytest.raises(ValueError):
        QuaternionDepthwiseConv1D(3, gated=True).ensure_built((None, None, 36), cpu)
    module = QuaternionConformerConvModule(64, kernel_size=7, seed=11, name='cm')
    module.ensure_built((None, 5, 64), cpu)
    assert [n for n, _ in module.named_parameters()] == ['pw1.r', 'pw1.bias', 'depthwise.kernel', 'depthwise.bias', 'norm.gamma', 'norm.beta',
                                                         'pw2.r', 'pw2.bias']
    assert tuple(module.pw1.r.shape) == (16, 128) and tuple(module.depthwise.kernel.shape) == (7, 64) and tuple(module.pw2.r.shape) == (16, 64)
    halves = module.pw1.r.detach().view(16, 4, 2, 16)                 # a | g inside every component: two independent draws
    assert not torch.equal(halves[:, :, 0], halves[:, :, 1]) and float(halves.abs().min()) > 0
    assert QuaternionConformerConvModule.from_config(module.get_config()).get_config() == module.get_config()
    assert module.compute_output_shape((3, 5, 64)) == (3, 5, 64)
    block = QuaternionConformerBlock(64, 2, 128, kernel_size=7, dropout=0.1, name='cb')
    block.ensure_built((None, 5, 64), cpu)
    assert [n for n, _ in block.named_parameters()] == PER_BLOCK and list(block.state_dict()) == PER_BLOCK
    assert QuaternionConformerBlock.from_config(block.get_config()).get_config() == block.get_config()
    assert block.get_config()['kernel_size'] == 7 and block.compute_output_shape((3, 5, 64)) == (3, 5, 64)
    model = TimitQConformer(2, 64, heads=2, ff_units=128, kernel_size=7)
    model.embed.ensure_built((None, 164), cpu)
    for blk in model.blocks:
        blk.ensure_built((None, 5, 64), cpu)
    model.pred.layer.ensure_built((None, 64), cpu)
    assert list(model.state_dict()) == ['embed.r', 'embed.bias'] + ['blocks.%d.%s' % (i, n) for i in range(2) for n in PER_BLOCK] + [
        'pred.layer.kernel', 'pred.layer.bias']
    # the count, written out.  embed: 41 x 64 + 64.  A block: six normalisations of 16 + 64; two feed-forward pairs of (16 x 128 +
    # 128) + (32 x 64 + 64); attention 16 x 192 + 192 + 16 x 64 + 64; convolution module (16 x 128 + 128) + (7 x 64 + 64) + (16 x 64 +
    # 64).  Output layer 64 x 62 + 62.
    per_block = 6 * 80 + 2 * (2176 + 2112) + 4352 + (2176 + 512 + 1088)
    assert per_block == 17184
    assert sum(p.numel() for p in model.parameters()) == 2688 + 2 * per_block + 4030 == 41086
    assert isinstance(model, TimitQTransformer) and all(hasattr(model, n) for n in ('ctc_loss', 'decode', 'evaluate', 'align', 'error_breakdown'))
    assert not hasattr(model, 'final_norm')
    # the other models are what they were
    tf = TimitQTransformer(2, 64, heads=2, ff_units=128, dropout=0)
    tf.embed.build((None, 164))
    for blk in tf.blocks:
        blk.build((None, 5, 64))
    tf.final_norm.build((None, 5, 64))
    per_tf = ['norm1.gamma', 'norm1.beta', 'attention.kernel', 'attention.bias', 'attention.out_kernel', 'attention.out_bias', 'norm2.gamma',
              'norm2.beta', 'ff1.r', 'ff1.bias', 'ff2.r', 'ff2.bias']
    assert list(tf.state_dict()) == ['embed.r', 'embed.bias'] + ['blocks.%d.%s' % (i, n) for i in range(2) for n in per_tf] + [
        'final_norm.gamma', 'final_norm.beta']
    lstm = TimitQLSTM(1, 64)
    lstm.rnn[0].build((None, 5, 164))
    assert list(lstm.state_dict()) == ['rnn.0.kernel', 'rnn.0.recurrent_kernel', 'rnn.0.bias']
    for other in (TimitQCNN(), lstm, tf):
        assert not any(w in n for n, _ in other.named_modules() for w in ('depthwise', 'pw1', 'pw2', 'norm_conv'))


@pytest.mark.parametrize('kind', ['bf16', 'fp16'])
@pytest.mark.parametrize('taps,padding', [(3, 'same'), (31, 'same'), (15, 'causal')])
@pytest.mark.parametrize('q', QS)
def test_rounding_points_move_the_reference_by_less_than_half_the_16_bit_bound(q, taps, padding, kind):
    """On the GPU tests' own inputs: the reference with the three rounding points stays within half of 1e-2 (bf16) / 2e-3 (fp16) of
    the float64 one on y, da, dg -- a store rounds by at most 2^-9 / 2^-12 of the element -- is not identical to it, and leaves dw
    and dbias (sums of the inputs, never of a rounded output) exactly alone."""
    pure, rounded = _reference(q, taps, padding, kind, rounded=False), _reference(q, taps, padding, kind)
    errs = {name: _rel(rounded[name], pure[name]) for name in OUT_16 + OUT_32}
    print(q, taps, padding, kind, errs)
    assert max(errs[name] for name in OUT_16) <= 0.5 * BOUND_16[kind], errs
    assert min(errs[name] for name in OUT_16) > 1e-5 and max(errs[name] for name in OUT_32) == 0, errs


# ---- GPU part ------------------------------------------------------------------------------------------------------------------
def _run(dev, dtype, q, taps, padding, gated=True, lengths=True, ops=None, weights=True):
    """functional.qglu_dwconv1d (plain: qdwconv1d) forward and backward on _inputs(...) (or on `ops`): name -> tensor."""
    i = ops if ops is not None else _inputs(q, taps, KINDS[dtype])
    t = lambda a, dt=dtype: torch.tensor(np.asarray(a), dtype=dt, device=dev)
    ln = torch.tensor(LENGTHS, device=dev) if lengths else None
    w = t(i['w'], torch.float32).requires_grad_(weights)
    bias = t(i['bias'], torch.float32).requires_grad_(weights)
    if gated:
        x = t(R.merge_packed(i['a'], i['g'])).requires_grad_()
        y = F.qglu_dwconv1d(x, w, bias, ln, padding)
    else:
        x = t(i['a']).requires_grad_()
        y = F.qdwconv1d(x, w, bias, ln, padding)
    y.backward(t(i['dy']))
    res = dict(y=y.detach())
    if gated:
        res['da'], res['dg'] = R.split_packed(x.grad)
    else:
        res['da'] = x.grad
    if weights:
        res.update(dw=w.grad, dbias=bias.grad)
    return res


def _check(got, want, dtype, what=''):
    kind = KINDS[dtype]
    errs = {}
    for name, g in got.items():
        assert g.dtype == (torch.float32 if name in OUT_32 else dtype) and tuple(g.shape) == want[name].shape, name
        errs[name] = (_rel(g.float().cpu().numpy(), want[name]), 1e-4 if kind is None else BOUND_16[kind] if name in OUT_16 else BOUND_32[kind])
    print(what, errs)
    assert all(e <= b for e, b in errs.values()), errs


def _inactive(dev):
    return torch.tensor(np.arange(T)[None, :] >= LENGTHS[:, None], device=dev)


@pytest.mark.gpu
@pytest.mark.parametrize('gated', [True, False], ids=['gated', 'plain'])
@pytest.mark.parametrize('taps,padding', TAPS, ids=TAP_IDS)
@pytest.mark.parametrize('q', QS)
@pytest.mark.parametrize('dtype', list(KINDS), ids=DTYPE_IDS)
def test_forward_and_backward_match_the_reference(dtype, q, taps, padding, gated):
    dev = _dev()
    assert F.qdwconv_path(dtype, B, T, q, taps, packed=gated) == _expected_path(dtype, q)
    got = _run(dev, dtype, q, taps, padding, gated)
    assert F.qdwconv_last_path() == _expected_path(dtype, q)
    _check(got, _reference(q, taps, padding, KINDS[dtype], gated), dtype)
    off = _inactive(dev)                           # asserted, not tolerated: inactive rows are exactly zero
    for name in ('y', 'da') + (('dg',) if gated else ()):
        assert int(got[name][off].ne(0).sum()) == 0, name


@pytest.mark.gpu
@pytest.mark.parametrize('dtype,q', [(torch.bfloat16, 72), (torch.float32, 5)], ids=['vec', 'generic'])
def test_without_lengths_without_bias_and_without_weight_gradients(dtype, q):
    dev = _dev()
    i = _inputs(q, 15, KINDS[dtype])
    want = R.qdwconv(i['a'], i['w'], None, i['g'], None, 'same', KINDS[dtype], i['dy'])
    t = lambda a, dt=dtype: torch.tensor(np.asarray(a), dtype=dt, device=dev)
    x, w = t(R.merge_packed(i['a'], i['g'])).requires_grad_(), t(i['w'], torch.float32)
    y = F.qglu_dwconv1d(x, w)
    y.backward(t(i['dy']))
    da, dg = R.split_packed(x.grad)
    _check(dict(y=y.detach(), da=da, dg=dg), want, dtype, 'no lengths, no bias')


@pytest.mark.gpu
@pytest.mark.parametrize('taps,padding', [(15, 'same'), (31, 'same'), (15, 'causal'), (31, 'causal')])
@pytest.mark.parametrize('q', [72, 5], ids=['vec', 'generic'])
@pytest.mark.parametrize('dtype', list(KINDS), ids=DTYPE_IDS)
def test_lattice_operands_give_the_reference_exactly_on_the_plain_path(dtype, q, taps, padding):
    """x, dy, taps and bias from {-1, 0, 1}: every product and every partial sum is an integer, |y| <= 4 K + 1 <= 125 and |dx| <= 4 K
    are exact in bf16, the dw sums stay below B T 4 < 2^24: y, dx, dw, dbias equal the reference as numbers, in all three dtypes."""
    dev = _dev()
    rng = np.random.RandomState(700 + taps)
    ops = dict(a=LAT.integer_lattice(rng, (B, T, 4 * q)), dy=LAT.integer_lattice(rng, (B, T, 4 * q)), w=LAT.integer_lattice(rng, (taps, 4 * q)),
               bias=LAT.integer_lattice(rng, (4 * q,)))
    want = R.qdwconv(ops['a'], ops['w'], ops['bias'], None, LENGTHS, padding, None, ops['dy'])
    assert np.abs(want['y']).max() <= 4 * taps + 1 <= LAT.exact_range(dtype) and np.abs(want['dw']).max() < LAT.FP32_EXACT
    assert np.abs(want['y']).max() > 8 and np.abs(want['dw']).max() > 8
    got = _run(dev, dtype, q, taps, padding, gated=False, ops=ops)
    for name in ('y', 'da', 'dw', 'dbias'):
        assert np.array_equal(got[name].float().cpu().numpy().astype(np.float64), want[name]), name


@pytest.mark.gpu
@pytest.mark.parametrize('dtype,q,taps,padding,gated', [(torch.bfloat16, 72, 15, 'same', True), (torch.float16, 8, 31, 'causal', False),
                                                         (torch.float32, 72, 3, 'same', True), (torch.float32, 5, 15, 'same', True),
                                                         (torch.bfloat16, 5, 3, 'causal', False)],
                         ids=['vec_bf16_gated', 'vec_fp16_plain', 'vec_fp32_gated', 'generic_fp32_gated', 'generic_bf16_plain'])
def test_nan_in_the_padding_frames_changes_no_bit(dtype, q, taps, padding, gated):
    """NaN in a, g and dy at every row t >= lengths[b]: all outputs are bit-identical to the run with zeros there, and y, da, dg are
    exactly 0 at those rows (the value is selected, never multiplied by 0)."""
    dev = _dev()
    i = _inputs(q, taps, KINDS[dtype])
    off = (np.arange(T)[None, :] >= LENGTHS[:, None])[:, :, None]
    runs = []
    for fill in (0.0, np.nan):
        ops = dict(i, a=np.where(off, fill, i['a']), g=np.where(off, fill, i['g']), dy=np.where(off, fill, i['dy']))
        runs.append(_run(dev, dtype, q, taps, padding, gated, ops=ops))
    mask = _inactive(dev)
    for name in runs[0]:
        assert GA.first_bit_difference(runs[0][name], runs[1][name]) is None, name
        assert bool(torch.isfinite(runs[1][name]).all()), name
        if name in OUT_16:
            assert int(runs[1][name][mask].ne(0).sum()) == 0, name


@pytest.mark.gpu
@pytest.mark.parametrize('dtype,q,taps', [(torch.bfloat16, 72, 31), (torch.float16, 8, 3), (torch.float32, 5, 15)],
                         ids=['vec_two_blocks', 'vec_one_block', 'generic'])
def test_two_calls_agree_bit_for_bit(dtype, q, taps):
    """No atomics: the slab partials and their sum have a fixed order."""
    dev = _dev()
    first, again = _run(dev, dtype, q, taps, 'same'), _run(dev, dtype, q, taps, 'same')
    for name in first:
        assert GA.first_bit_difference(first[name], again[name]) is None, name


def _raw_call(dev, dtype, q, taps, padding, packed, extra=0, shift=0):
    """qk_qdwconv_fwd / _bwd through ctypes on _inputs(...).  packed: a | g are windows of ONE (B, T, 8 Q + extra) buffer and da | dg
    of one gradient buffer of that shape, prefilled with 9; else four dense (B, T, 4 Q) buffers.  shift: elements by which every
    activation buffer's base pointer is moved off its 16-byte alignment.  Returns name -> tensor, the wide gradient buffer, and the
    path names the forward and the backward reported."""
    lib = _lib.lib()
    i = _inputs(q, taps, KINDS[dtype])
    W = 4 * q
    t = lambda a, dt=dtype: torch.tensor(np.asarray(a), dtype=dt, device=dev)

    def shifted(shape, fill=0.0):
        n = int(np.prod(shape))
        base = torch.full((n + 8,), fill, dtype=dtype, device=dev)
        return base[shift:shift + n].view(shape)
    row = 8 * q + extra if packed else W
    comp = 2 * q if packed else q
    es = torch.empty(0, dtype=dtype).element_size()
    if packed:
        xb, gb = shifted((B, T, row), 3.0), shifted((B, T, row), 9.0)
        xb[:, :, :8 * q] = t(R.merge_packed(i['a'], i['g']))
        a_ptr, g_ptr, da_ptr, dg_ptr = xb.data_ptr(), xb.data_ptr() + q * es, gb.data_ptr(), gb.data_ptr() + q * es
    else:
        ab, gg, dab, dgb = shifted((B, T, W)), shifted((B, T, W)), shifted((B, T, W), 9.0), shifted((B, T, W), 9.0)
        ab.copy_(t(i['a']))
        gg.copy_(t(i['g']))
        xb, gb = None, None
        a_ptr, g_ptr, da_ptr, dg_ptr = ab.data_ptr(), gg.data_ptr(), dab.data_ptr(), dgb.data_ptr()
    y, dy = shifted((B, T, W), 5.0), shifted((B, T, W))
    dy.copy_(t(i['dy']))
    w, bias, ln = t(i['w'], torch.float32), t(i['bias'], torch.float32), torch.tensor(LENGTHS, device=dev)
    dw, dbias = torch.empty((taps, W), dtype=torch.float32, device=dev), torch.empty(W, dtype=torch.float32, device=dev)
    desc = F.qdwconv_desc(dtype, B, T, q, taps, F.qdwconv_pad_lo(taps, padding), x=(row, comp))
    n = int(lib.qk_qdwconv_workspace_bytes(ctypes.byref(desc), _lib.QK_OP_BWD))
    ws = torch.empty(n, dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    with torch.cuda.device(dev):
        _lib.check(lib.qk_qdwconv_fwd(ctypes.byref(desc), a_ptr, g_ptr, w.data_ptr(), bias.data_ptr(), ln.data_ptr(), y.data_ptr(), stream),
                   'qk_qdwconv_fwd')
        fwd_path = F.qdwconv_last_path()
        _lib.check(lib.qk_qdwconv_bwd(ctypes.byref(desc), dy.data_ptr(), a_ptr, g_ptr, w.data_ptr(), ln.data_ptr(), da_ptr, dg_ptr,
                                      dw.data_ptr(), dbias.data_ptr(), ws.data_ptr(), n, stream), 'qk_qdwconv_bwd')
    torch.cuda.synchronize(dev)
    if packed:
        da, dg = R.split_packed(gb[:, :, :8 * q])
    else:
        da, dg = dab, dgb
    return dict(y=y, da=da, dg=dg, dw=dw, dbias=dbias), (xb, gb), (fwd_path, F.qdwconv_last_path())


@pytest.mark.gpu
@pytest.mark.parametrize('dtype,q,taps,padding', [(torch.bfloat16, 72, 15, 'same'), (torch.float32, 8, 31, 'causal'), (torch.float16, 5, 3, 'same')],
                         ids=['vec_bf16', 'vec_fp32', 'generic_fp16'])
def test_packed_projection_output_equals_the_contiguous_call_bit_for_bit(dtype, q, taps, padding):
    """The (B, T, 8 Q) projection output read in place and the ONE packed gradient against the call on four dense buffers: the same
    kernels, the same bits.  Then with 8 (fp32: 4) more columns per row: the columns outside the addressed runs keep their fill.  The
    autograd function on the packed tensor gives the same bits again."""
    dev = _dev()
    V = 4 if dtype == torch.float32 else 8
    dense, _, paths = _raw_call(dev, dtype, q, taps, padding, packed=False)
    assert paths == (_expected_path(dtype, q),) * 2
    for extra in (0, V):
        got, (xb, gb), paths = _raw_call(dev, dtype, q, taps, padding, packed=True, extra=extra)
        assert paths == (_expected_path(dtype, q),) * 2
        for name in dense:
            assert GA.first_bit_difference(got[name].contiguous(), dense[name].contiguous()) is None, (name, extra)
        if extra:
            assert bool((gb[:, :, 8 * q:] == 9.0).all()) and bool((xb[:, :, 8 * q:] == 3.0).all())
    auto = _run(dev, dtype, q, taps, padding)
    for name in dense:
        assert GA.first_bit_difference(auto[name].contiguous(), dense[name].contiguous()) is None, name


@pytest.mark.gpu
@pytest.mark.parametrize('dtype,q,taps', [(torch.bfloat16, 72, 15), (torch.float32, 8, 3)], ids=['bf16', 'fp32'])
def test_misaligned_base_pointers_run_the_generic_kernels_inside_the_bounds(dtype, q, taps):
    """A descriptor that qualifies for the vector kernels with base pointers one element off their 16-byte alignment: both calls
    report the generic path and keep the parity bounds."""
    dev = _dev()
    assert F.qdwconv_path(dtype, B, T, q, taps, packed=True) == 'vec'
    got, _, paths = _raw_call(dev, dtype, q, taps, 'same', packed=True, shift=1)
    assert paths == ('generic', 'generic')
    _check(got, _reference(q, taps, 'same', KINDS[dtype]), dtype, 'generic kernels at a vector width')
    # the autograd function on a misaligned view of a packed tensor
    i = _inputs(q, taps, KINDS[dtype])
    t = lambda a, dt=dtype: torch.tensor(np.asarray(a), dtype=dt, device=dev)
    flat = torch.zeros(B * T * 8 * q + 8, dtype=dtype, device=dev)
    flat[1:1 + B * T * 8 * q] = t(R.merge_packed(i['a'], i['g'])).reshape(-1)
    x = flat[1:1 + B * T * 8 * q].view(B, T, 8 * q).detach().requires_grad_()
    y = F.qglu_dwconv1d(x, t(i['w'], torch.float32), t(i['bias'], torch.float32), torch.tensor(LENGTHS, device=dev))
    assert F.qdwconv_last_path() == 'generic'
    y.backward(t(i['dy']))
    da, dg = R.split_packed(x.grad)
    _check(dict(y=y.detach(), da=da, dg=dg), _reference(q, taps, 'same', KINDS[dtype]), dtype, 'autograd on a misaligned view')


@pytest.mark.gpu
@pytest.mark.parametrize('dtype,q,taps,gated', [(torch.bfloat16, 72, 15, True), (torch.float32, 8, 31, False), (torch.float32, 5, 3, True)],
                         ids=['vec_bf16_gated', 'vec_fp32_plain', 'generic'])
def test_forward_and_backward_keep_to_their_buffers(monkeypatch, dtype, q, taps, gated):
    """Under guard bands and the two fills: no stray write around y, the (packed) gradient, dw, dbias or the workspace; every returned
    element written; the two runs bit-identical (nothing depends on what the workspace or an output held before the call)."""
    dev = _dev()

    def run(alloc):
        return _run(dev, dtype, q, taps, 'same', gated)
    res = GA.run_twice(run, monkeypatch, modules=(F,))
    GA.assert_hygiene(res, 'qdwconv %s q=%d K=%d: ' % (dtype, q, taps))
    sites = {a.site.split(':')[0] for a in res.allocs[0].log}
    assert sites == {'functional.py'} and len(res.allocs[0].log) == 5        # y, the gradient, dw, dbias, workspace
    ws = [a for a in res.allocs[0].log if a.dtype == torch.uint8]
    assert len(ws) == 1 and ws[0].nbytes == B * (taps + 1) * 16 * q


@pytest.mark.gpu
@pytest.mark.parametrize('dtype,q,taps', [(torch.bfloat16, 72, 15), (torch.float32, 5, 7)], ids=['vec', 'generic'])
def test_forward_and_backward_replay_from_a_captured_graph(dtype, q, taps):
    """Forward + backward captured once on one stream, replayed with NEW input values: bit-equal to the eager call on those values.
    That it captures at all shows that the launches read nothing on the host and allocate nothing."""
    dev = _dev()
    new = _inputs(q, taps, KINDS[dtype])
    eager = _run(dev, dtype, q, taps, 'same')
    t = lambda a, dt=dtype: torch.tensor(np.asarray(a), dtype=dt, device=dev)
    x = torch.ones((B, T, 8 * q), dtype=dtype, device=dev).requires_grad_()
    dy, ln = torch.ones((B, T, 4 * q), dtype=dtype, device=dev), torch.tensor(LENGTHS, device=dev)
    w, bias = t(0 * new['w'] + 0.25, torch.float32).requires_grad_(), t(0 * new['bias'], torch.float32).requires_grad_()

    def body():
        y = F.qglu_dwconv1d(x, w, bias, ln)
        return (y.detach(),) + torch.autograd.grad(y, (x, w, bias), dy)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        body()                                                       # warm-up, eagerly (allocator, code objects)
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize(dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = body()
    with torch.no_grad():                                            # new values into the captured operands
        x.copy_(t(R.merge_packed(new['a'], new['g'])))
        dy.copy_(t(new['dy']))
        w.copy_(t(new['w'], torch.float32))
        bias.copy_(t(new['bias'], torch.float32))
    for o in outs:
        o.zero_()
    graph.replay()
    torch.cuda.synchronize(dev)
    da, dg = R.split_packed(outs[1])
    for name, o in (('y', outs[0]), ('da', da), ('dg', dg), ('dw', outs[2]), ('dbias', outs[3])):
        assert GA.first_bit_difference(o.contiguous(), eager[name].contiguous()) is None, name


@pytest.mark.gpu
@pytest.mark.parametrize('padding', ['same', 'causal'])
def test_conv_module_matches_the_float64_composition(padding):
    """QuaternionConformerConvModule(40, kernel_size=5) at B 4, T 20, fp32: output, input gradient and the eight parameter gradients
    within 1e-4 of dense + qdwconv_ref + qlnorm_ref in float64."""
    dev = _dev()
    rng = np.random.RandomState(12)
    layer = QuaternionConformerConvModule(40, kernel_size=5, padding=padding, seed=7)
    x = torch.tensor(rng.randn(4, 20, 40), dtype=torch.float32, device=dev)
    lengths = torch.tensor([20, 7, 13, 1], dtype=torch.int32, device=dev)
    wgt = torch.tensor(rng.randn(4, 20, 40), dtype=torch.float32, device=dev)
    layer.ensure_built(x.shape, dev)
    with torch.no_grad():
        for name in ('pw1', 'depthwise', 'pw2'):
            bias = getattr(layer, name).bias
            bias.add_(torch.tensor(0.3 * rng.randn(*bias.shape), dtype=torch.float32, device=dev))
    x.requires_grad_()
    y = layer(x, lengths=lengths)
    (y * wgt).sum().backward()
    p64 = {n: p.detach().double().cpu().requires_grad_() for n, p in layer.named_parameters()}
    x64 = x.detach().double().cpu().requires_grad_()
    y64 = R.conv_module_t(x64, p64, '', lengths.cpu(), padding, layer.norm.epsilon)
    (y64 * wgt.double().cpu()).sum().backward()
    errs = dict(y=_rel(y.detach().cpu().numpy(), y64.detach().numpy()), dx=_rel(x.grad.cpu().numpy(), x64.grad.numpy()))
    errs.update({n: _rel(p.grad.cpu().numpy(), p64[n].grad.numpy()) for n, p in layer.named_parameters()})
    print(errs)
    assert len(errs) == 10 and max(errs.values()) <= 1e-4, errs


def _small_model(dev, seed):
    """TimitQConformer(2, 64, heads=2, ff_units=128, kernel_size=7, dropout=0) at B 4, T 20 with its batch; parameters fp32, built."""
    np.random.seed(seed)
    torch.manual_seed(seed)
    model = TimitQConformer(2, 64, heads=2, ff_units=128, kernel_size=7, dropout=0)
    rng = np.random.RandomState(seed + 1)
    x = torch.tensor(rng.randn(4, 4, 41, 20).astype(np.float32), device=dev)
    labels = torch.tensor(rng.randint(0, 61, (4, 3)), device=dev, dtype=torch.int32)
    il = torch.tensor([[20], [15], [18], [9]], dtype=torch.int32, device=dev)
    ll = torch.tensor([[3], [2], [3], [1]], dtype=torch.int32, device=dev)
    model.to(dev)
    with torch.no_grad():
        model(x, il)
    model.to(dev)
    return model, x, labels, il, ll


def _model_reference(model, x, labels, il, ll):
    """mean CTC cost of the float64 composition (dense, qlnorm_ref, qattn_ref, qdwconv_ref) and its gradients, by parameter name."""
    from qcnn_amd.models.qtransformer_model import sinusoidal_positions
    p64 = {n: p.detach().double().cpu().requires_grad_() for n, p in model.named_parameters()}
    b, _, f, t = x.shape
    lengths = il.reshape(-1).cpu()
    o = R.dense_t(x.double().cpu().permute(0, 3, 1, 2).reshape(b * t, 4 * f), p64['embed.r'], p64['embed.bias']).reshape(b, t, -1)
    o = o + sinusoidal_positions(t, o.shape[-1]).double()
    for i, blk in enumerate(model.blocks):
        o = R.conformer_block_t(o, p64, 'blocks.%d.' % i, blk.heads, lengths, blk.padding, blk.norm_out.epsilon)
    pred = torch.softmax(o @ p64['pred.layer.kernel'] + p64['pred.layer.bias'], dim=-1)
    logp = torch.log_softmax(torch.log(pred + 1e-7), dim=-1).transpose(0, 1)              # K.ctc_batch_cost (layers.ctc_batch_cost)
    cost = torch.nn.functional.ctc_loss(logp, labels.long().cpu(), lengths.long(), ll.reshape(-1).long().cpu(), blank=61, reduction='none')
    loss = cost.mean()
    loss.backward()
    return float(loss.detach()), {n: p.grad.numpy() for n, p in p64.items()}


@pytest.mark.gpu
def test_model_step_matches_the_composition_and_ignores_padding_frames():
    """TimitQConformer(2, 64, heads=2, ff_units=128, kernel_size=7, dropout=0) through ctc_mean_loss at B 4, T 20, fp32: the loss and
    all 64 parameter gradients within 1e-4 of the float64 composition; the posteriors at frames < input_length are bit-unchanged when
    the padding frames of the input are replaced by noise; one guarded scheduled step runs on the parameters as they are."""
    from qcnn_amd import dp
    from qcnn_amd.training import GradGuard, LRSchedule, ScheduledAdam
    dev = _dev()
    model, x, labels, il, ll = _small_model(dev, 31)
    loss = model.ctc_mean_loss(x, labels, il, ll)
    loss.backward()
    want_loss, want = _model_reference(model, x, labels, il, ll)
    errs = {n: _rel(p.grad.cpu().numpy(), want[n]) for n, p in model.named_parameters()}
    print(float(loss.detach()), want_loss, errs)
    assert len(errs) == 2 + 2 * 30 + 2
    assert abs(float(loss.detach()) - want_loss) <= 1e-4 * abs(want_loss) and max(errs.values()) <= 1e-4, errs
    with torch.no_grad():
        model.eval()
        clean = model(x, il)
        noisy_x = x.clone()
        pad = torch.arange(20, device=dev)[None, :] >= il.reshape(-1, 1)
        noisy_x.permute(0, 3, 1, 2)[pad] = 37.0 * torch.randn(int(pad.sum()), 4, 41, device=dev)
        noisy = model(noisy_x, il)
        assert int(pad.sum()) > 0 and not torch.equal(noisy_x, x)
        assert GA.first_bit_difference(noisy[~pad], clean[~pad]) is None
        model.train()
    for p in model.parameters():
        p.grad = None
    flat = dp.FlatParams([p for p in model.parameters() if p.requires_grad], direct=True)
    guard = GradGuard(dev, clipnorm=50.0, loss_scale=4.0)
    opt = ScheduledAdam(flat.param, flat.grad, LRSchedule(5e-3), guard=guard)
    x16 = x.to(torch.bfloat16)
    model.training_loss(x16, labels, il, ll, loss_scale=guard.loss_scale).backward()
    opt.step()
    assert opt.stats()['step'] == 1 and guard.stats()['skipped_steps'] == 0
    assert np.isfinite(float(model.training_loss(x16, labels, il, ll)))
