"""Quaternion multi-head self-attention (include/qk_attn.h; csrc/qk_qattn.hip): the float64 reference against central differences and
against torch's scaled_dot_product_attention, the header inventory, dispatch and descriptor checks, the layer and model surface on
the CPU; on the GPU parity of forward and backward for three dtypes and four head widths, overflow, poisoned padding, repeatability,
strided and packed operands, buffer hygiene, graph replay, the layer and the TIMIT model.

Bounds, relative to max|want| per tensor: fp32 1e-4 against float64; bf16 1e-2 and fp16 2e-3 against the reference WITH the header's
rounding points (test_rounding_points_... shows that those alone move the float64 result by less than half of each bound)."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest
import torch

import guarded_alloc as GA
import qattn_ref as R
import qlnorm_ref as NR
import qlstm_ref as LR
from qcnn_amd import _lib, functional as F
from qcnn_amd.keras_like import regularizers
from qcnn_amd.complexnn import QuaternionMultiHeadAttention, QuaternionTransformerEncoderLayer
from qcnn_amd.models import TimitQCNN, TimitQLSTM, TimitQTransformer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = {torch.float32: None, torch.bfloat16: 'bf16', torch.float16: 'fp16'}
DTYPE_IDS = ['fp32', 'bf16', 'fp16']
BOUND = {None: 1e-4, 'bf16': 1e-2, 'fp16': 2e-3}
# the GPU shapes: T = 150 is two 64-key tiles of the forward and a ragged third (four 32-row tiles of the backward and a ragged
# fifth; three 64-row workgroups, the last ragged); the lengths put a batch row at 0, at 1, on a tile edge, one past it, two short of
# T and at T.  dq 16 / 32 run the matrix kernels in bf16 / fp16 (D = 64 / 128), dq 8 / 5 the generic ones; fp32 is always generic.
B, T, H = 6, 150, 3
LENGTHS = np.array([0, 1, 64, 65, 148, 150], dtype=np.int32)
DQS = (16, 32, 8, 5)
NAMES = ('o', 'dq', 'dk', 'dv')
OVERFLOW_SCALE = 3.0          # unit-variance q, k at dq = 16: the scores pass +-100 (asserted on the reference's own count)


def _dev():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    return torch.device('cuda:0')


def _rel(got, want):
    return float(np.abs(np.asarray(got, dtype=np.float64) - want).max()) / max(float(np.abs(want).max()), 1e-30)


def _f32(a):
    return a.astype(np.float32).astype(np.float64)


def _expected_path(dtype, dq):
    return 'mfma' if dtype != torch.float32 and dq in (16, 32) else 'generic'


@functools.lru_cache(maxsize=None)
def _inputs(dq, kind, steps=T):
    """Seeded unit-variance operands (never written), already rounded to `kind`."""
    rng = np.random.RandomState(3000 + dq + steps)
    d = {name: R.rnd(_f32(rng.randn(B, steps, 4 * H * dq)), kind) for name in ('q', 'k', 'v', 'do')}
    d['lengths'] = np.minimum(LENGTHS, steps).astype(np.int32)
    for v in d.values():
        v.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def _reference(dq, kind, lengths=True, steps=T, scale=None, ref_kind='same'):
    """The reference's outputs for _inputs(...), computed once and shared."""
    i = _inputs(dq, kind, steps)
    return R.qattention(i['q'], i['k'], i['v'], H, i['lengths'] if lengths else None, scale=scale, kind=kind if ref_kind == 'same' else ref_kind,
                        do=i['do'])


# ---- CPU part ------------------------------------------------------------------------------------------------------------------
def test_reference_backward_agrees_with_central_differences():
    """B 2, T 4, H 2, dq 1, lengths 4 / 2: 1e-7 relative for dq, dk, dv."""
    rng = np.random.RandomState(5)
    lengths = np.array([4, 2])
    par = {n: rng.randn(2, 4, 8) for n in ('q', 'k', 'v')}
    w = rng.randn(2, 4, 8)

    def loss(p):
        return float((R.qattention(p['q'], p['k'], p['v'], 2, lengths)['o'] * w).sum())
    got = R.qattention(par['q'], par['k'], par['v'], 2, lengths, do=w)
    eps = 1e-5
    for name in ('q', 'k', 'v'):
        want = np.zeros_like(par[name])
        flat, wflat = par[name].reshape(-1), want.reshape(-1)
        for j in range(flat.size):
            keep = flat[j]
            flat[j] = keep + eps
            up = loss(par)
            flat[j] = keep - eps
            wflat[j] = (up - loss(par)) / (2 * eps)
            flat[j] = keep
        assert float(np.abs(want).max()) > 0.05 and _rel(got['d' + name], want) <= 1e-7, (name, _rel(got['d' + name], want))
        assert not want[1, 2:].any() and not got['d' + name][1, 2:].any()


def test_reference_agrees_with_torch_scaled_dot_product_attention():
    """An independent check of the layout mapping: heads permuted by hand, a boolean key mask, float64 on the CPU, 1e-12."""
    rng = np.random.RandomState(6)
    bsz, steps, heads, dq = 3, 7, 2, 3
    lengths = np.array([7, 4, 1])
    q, k, v = (rng.randn(bsz, steps, 4 * heads * dq) for _ in range(3))
    want = R.qattention(q, k, v, heads, lengths)

    def split(a):                                  # column c * Q + h * dq + u -> (b, h, t, c * dq + u)
        return torch.tensor(a).view(bsz, steps, 4, heads, dq).permute(0, 3, 1, 2, 4).reshape(bsz, heads, steps, 4 * dq)
    mask = torch.tensor(np.arange(steps)[None, :] < lengths[:, None])[:, None, None, :]
    o = torch.nn.functional.scaled_dot_product_attention(split(q), split(k), split(v), attn_mask=mask)
    o = o.view(bsz, heads, steps, 4, dq).permute(0, 2, 3, 1, 4).reshape(bsz, steps, 4 * heads * dq).numpy()
    o = np.where((np.arange(steps)[None, :] < lengths[:, None])[:, :, None], o, 0.0)
    assert _rel(want['o'], o) <= 1e-12
    assert _rel(R.qattention_t(*(torch.tensor(a) for a in (q, k, v)), heads, torch.tensor(lengths)).numpy(), o) <= 1e-12


def test_attn_header_inventory_equals_the_sixth_symbol_table():
    lib = _lib.lib()
    h = open(os.path.join(ROOT, 'include', 'qk_attn.h')).read()
    declared = set(re.findall(r'\b(qk_[a-z_0-9]+)\s*\(', h))
    declared -= {n for n in declared if n.endswith('_t')}
    assert declared == set(_lib.ATTN_SYMBOLS), declared ^ set(_lib.ATTN_SYMBOLS)
    for name in declared:
        assert hasattr(lib, name), name
    for other in (_lib.SYMBOLS, _lib.OPT_SYMBOLS, _lib.DATA_SYMBOLS, _lib.RNN_SYMBOLS, _lib.NORM_SYMBOLS):
        assert not set(_lib.ATTN_SYMBOLS) & set(other)
    main = open(os.path.join(ROOT, 'include', 'qk.h')).read()
    assert not any(name in main for name in _lib.ATTN_SYMBOLS) and 'qattn' not in main
    decls = {name: (res, args) for res, name, args in re.findall(r'^(int|size_t) (qk_[a-z_0-9]+)\(([^;]*)\);', h, re.M | re.S)}
    assert set(decls) == set(_lib.ATTN_SYMBOLS)
    for name, (res, args) in decls.items():
        restype, argtypes = _lib.ATTN_SYMBOLS[name]
        assert restype is (ctypes.c_int if res == 'int' else ctypes.c_size_t), name
        assert len(argtypes) == len(args.split(',')), name
        last = ' '.join(args.split(',')[-1].split())
        if name in ('qk_qattn_fwd', 'qk_qattn_bwd'):
            assert last == 'void *stream' and argtypes[-1] is ctypes.c_void_p, name
        else:                                                       # host only
            assert 'stream' not in args, name
    body = h[h.index('typedef struct qk_qattn_desc_t {'):h.index('} qk_qattn_desc_t;')]
    fields = re.findall(r'^\s*int32_t ([a-z_]+);', body, re.M)
    assert fields == ['dtype', 'batch', 'steps', 'heads', 'dq', 'q_row', 'q_comp', 'k_row', 'k_comp', 'v_row', 'v_comp', 'o_row', 'o_comp', 'flags']
    assert [(n, ctypes.c_int32) for n in fields] == list(_lib.QAttnDesc._fields_) and ctypes.sizeof(_lib.QAttnDesc) == 56
    for macro in ('QK_QATTN_PATH_GENERIC', 'QK_QATTN_PATH_MFMA'):
        assert int(re.search(r'#define %s (\d+)' % macro, h).group(1)) == getattr(_lib, macro)
    assert 'Tay et al.' in h and 'DEVIATION' in h
    assert lib.qk_version() == 103


def test_dispatch_predicate_and_descriptor_checks_need_no_gpu():
    for dtype in KINDS:
        for dq in (16, 32, 8, 5, 1, 64, 24):
            assert F.qattention_path(dtype, B, T, H, dq) == _expected_path(dtype, dq), (dtype, dq)
            assert F.qattention_path(dtype, B, 1, H, dq) == _expected_path(dtype, dq), (dtype, dq)
    assert F.qattention_path(torch.bfloat16, B, T, H, 16, packed=True) == 'mfma'
    lib = _lib.lib()
    sup = lambda d: lib.qk_qattn_supported(ctypes.byref(d))
    Q = H * 16
    # (dtype, dq, one (row, comp) pair for q, k, v and o) -> path: strides that break the 16-byte alignment of a dq-run go generic
    for dtype, dq, pair, want in ((torch.bfloat16, 16, (4 * Q, Q), 'mfma'), (torch.bfloat16, 16, (12 * Q, 3 * Q), 'mfma'),
                                  (torch.float16, 16, (4 * Q + 8, Q), 'mfma'), (torch.float16, 16, (4 * Q + 32, Q + 8), 'mfma'),
                                  (torch.bfloat16, 16, (4 * Q + 4, Q), 'generic'), (torch.bfloat16, 16, (4 * Q + 8, Q + 1), 'generic'),
                                  (torch.float16, 32, (8 * Q + 1, 2 * Q), 'generic'), (torch.float32, 16, (4 * Q, Q), 'generic')):
        desc = F.qattention_desc(dtype, B, T, H, dq, pair, pair, pair, pair)
        assert _lib.QK_QATTN_PATH_NAMES[sup(desc)] == want, (dtype, dq, pair)
    for which in ('q', 'k', 'v', 'o'):                               # one misaligned tensor is enough
        desc = F.qattention_desc(torch.bfloat16, B, T, H, 16, **{which: (4 * Q + 2, Q)})
        assert sup(desc) == _lib.QK_QATTN_PATH_GENERIC, which
    good = F.qattention_desc(torch.bfloat16, B, T, H, 16)
    assert lib.qk_qattn_workspace_bytes(ctypes.byref(good), _lib.QK_OP_BWD) >= B * H * T * 4
    assert lib.qk_qattn_workspace_bytes(ctypes.byref(good), _lib.QK_OP_FWD) == 0
    assert lib.qk_qattn_workspace_bytes(ctypes.byref(good), _lib.QK_OP_BWD_DATA) == 0 and lib.qk_last_error()
    bad_fields = [('dtype', 7), ('batch', 0), ('steps', 0), ('heads', 0), ('dq', 0), ('flags', 1), ('dq', -16), ('heads', 1 << 20)]
    for name in ('q', 'k', 'v', 'o'):
        bad_fields += [(name + '_comp', Q - 1), (name + '_row', 4 * Q - 1), (name + '_row', -4 * Q), (name + '_comp', 0)]
    for field, value in bad_fields:
        bad = F.qattention_desc(torch.bfloat16, B, T, H, 16)
        setattr(bad, field, value)
        assert sup(bad) == 0 and lib.qk_last_error(), field
        assert lib.qk_qattn_workspace_bytes(ctypes.byref(bad), _lib.QK_OP_BWD) == 0, field
        assert lib.qk_qattn_fwd(ctypes.byref(bad), None, None, None, None, 0.0, None, None, None) == _lib.QK_ERR_INVALID_ARG, field
        assert lib.qk_qattn_bwd(ctypes.byref(bad), *([None] * 7), 0.0, None, None, None, None, 0, None) == _lib.QK_ERR_INVALID_ARG, field
    assert lib.qk_qattn_fwd(ctypes.byref(good), None, None, None, None, 0.0, None, None, None) == _lib.QK_ERR_INVALID_ARG      # NULL buffers
    assert lib.qk_qattn_bwd(ctypes.byref(good), *([None] * 7), 0.0, None, None, None, None, 0, None) == _lib.QK_ERR_INVALID_ARG
    assert lib.qk_qattn_supported(None) == 0
    x = torch.zeros(2, 3, 32)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        F.qattention(x, x, x, 2)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        F.qattention_packed(torch.zeros(2, 3, 96), 2)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        QuaternionMultiHeadAttention(32, 2)(x)


def _moved(dq, kind, lengths=True, scale=None):
    """How far the rounding points alone move the float64 result on _inputs(dq, kind): name -> relative to max|want|."""
    plain, rounded = _reference(dq, kind, lengths, scale=scale, ref_kind=None), _reference(dq, kind, lengths, scale=scale)
    return {n: _rel(rounded[n], plain[n]) for n in NAMES}


@pytest.mark.parametrize('kind', ['bf16', 'fp16'])
@pytest.mark.parametrize('dq', DQS)
def test_rounding_points_move_the_reference_by_less_than_half_the_16_bit_bound(dq, kind):
    """On the GPU tests' own inputs: under half the bound, which leaves the kernel the other half; and the rounding is in play."""
    moved = _moved(dq, kind)
    print(dq, kind, moved)
    assert 1e-5 < max(moved.values()) and max(moved.values()) <= 0.5 * BOUND[kind], moved


def test_rounding_points_on_the_overflow_inputs():
    """The overflow case (dq 16, bf16, scale OVERFLOW_SCALE): o and dv stay under half the bound (3.2e-3, 2.4e-3).  dq and dk do not:
    the rounding points alone move them by 5.7e-3 and 1.1e-2, at or past the whole bound, so no bound on them would test the kernel and
    the GPU test holds the bf16 dq / dk of that case to finiteness (test_overflow_...)."""
    s = R.scores(_inputs(16, 'bf16')['q'], _inputs(16, 'bf16')['k'], H, OVERFLOW_SCALE)
    assert s.max() > 100 and s.min() < -100
    moved = _moved(16, 'bf16', scale=OVERFLOW_SCALE)
    print(moved)
    assert 1e-5 < moved['o'] <= 0.5 * BOUND['bf16'] and moved['dv'] <= 0.5 * BOUND['bf16'], moved
    assert max(moved['dq'], moved['dk']) > 0.5 * BOUND['bf16'], moved


def test_reference_inactive_rows_poison_full_lengths_and_rotation():
    i = _inputs(5, None, 9)
    lengths = np.array([0, 1, 4, 5, 7, 9])
    q, k, v, do = i['q'], i['k'], i['v'], i['do']
    want = R.qattention(q, k, v, H, lengths, do=do)
    inactive = np.arange(9)[None, :] >= lengths[:, None]
    for n in NAMES:
        assert not want[n][inactive].any() and want[n][~inactive].any(), n
    assert not want['lse'].transpose(0, 2, 1)[inactive].any() and not want['o'][0].any()          # n = 0: the whole batch row
    # keys past n and inactive rows may hold anything
    for junk in (1e30, np.nan):
        pq, pk, pv, pdo = (np.where(inactive[:, :, None], junk, a) for a in (q, k, v, do))
        got = R.qattention(pq, pk, pv, H, lengths, do=pdo)
        for n in NAMES + ('lse',):
            assert np.array_equal(got[n], want[n]), (junk, n)
    full, none = R.qattention(q, k, v, H, np.full(B, 9), do=do), R.qattention(q, k, v, H, None, do=do)
    for n in NAMES + ('lse',):
        assert np.array_equal(full[n], none[n]), n
    # q and k multiplied from the right by one common unit quaternion: the scores, hence o, do not move
    rng = np.random.RandomState(9)
    u = rng.randn(4)
    u /= np.linalg.norm(u)

    def rotate(x):                                 # x (x) u, component-major
        a = x.reshape(B, 9, 4, -1)
        r, im, j, kk = a[:, :, 0], a[:, :, 1], a[:, :, 2], a[:, :, 3]
        return np.stack([r * u[0] - im * u[1] - j * u[2] - kk * u[3], r * u[1] + im * u[0] + j * u[3] - kk * u[2],
                         r * u[2] - im * u[3] + j * u[0] + kk * u[1], r * u[3] + im * u[2] - j * u[1] + kk * u[0]], axis=2).reshape(x.shape)
    assert _rel(R.qattention(rotate(q), rotate(k), v, H, lengths)['o'], want['o']) <= 1e-12
    assert _rel(R.qattention(rotate(q), k, v, H, lengths)['o'], want['o']) > 1e-3


def test_layer_and_model_surface():
    layer = QuaternionMultiHeadAttention(64, 2, seed=3, name='mha')
    assert layer.name == 'mha' and layer.compute_output_shape((None, 7, 32)) == (None, 7, 64)
    np.random.seed(11)                              # qdense_init draws the imaginary directions from the global generator
    layer.build((None, 7, 32))
    assert [(n, tuple(p.shape)) for n, p in layer.weights] == [('kernel', (8, 192)), ('bias', (192,)), ('out_kernel', (16, 64)), ('out_bias', (64,))]
    again = QuaternionMultiHeadAttention.from_config(layer.get_config())
    assert again.get_config() == layer.get_config()
    np.random.seed(11)
    again.build((None, 7, 32))
    assert torch.equal(again.kernel, layer.kernel) and torch.equal(again.out_kernel, layer.out_kernel)
    # the q, k and v blocks are independent draws, laid q | k | v inside every component
    blocks = [layer.kernel.detach().view(8, 4, 3, 16)[:, :, g] for g in range(3)]
    assert not torch.equal(blocks[0], blocks[1]) and not torch.equal(blocks[1], blocks[2]) and float(layer.bias.detach().abs().max()) == 0
    assert layer.regularization_losses() == []
    reg = QuaternionMultiHeadAttention(64, 2, kernel_regularizer=regularizers.l2(1e-4), use_bias=False)
    reg.build((None, 7, 32))
    assert [n for n, _ in reg.weights] == ['kernel', 'out_kernel'] and len(reg.regularization_losses()) == 2
    assert QuaternionMultiHeadAttention.from_config(reg.get_config()).get_config() == reg.get_config()
    with pytest.raises(ValueError):
        QuaternionMultiHeadAttention(64, 3)                           # 3 heads do not divide 16 units
    with pytest.raises(ValueError):
        QuaternionMultiHeadAttention(66, 2)
    block = QuaternionTransformerEncoderLayer(64, 2, 128, dropout=0.1, name='enc')
    block.build((None, 7, 64))
    assert [n for n, _ in block.named_parameters()] == ['norm1.gamma', 'norm1.beta', 'attention.kernel', 'attention.bias', 'attention.out_kernel',
                                                        'attention.out_bias', 'norm2.gamma', 'norm2.beta', 'ff1.r', 'ff1.bias', 'ff2.r', 'ff2.bias']
    assert QuaternionTransformerEncoderLayer.from_config(block.get_config()).get_config() == block.get_config()
    assert tuple(block.ff1.r.shape) == (16, 128) and tuple(block.ff2.r.shape) == (32, 64)
    model = TimitQTransformer(2, 64, heads=2, ff_units=128, dropout=0)
    model.embed.build((None, 164))
    for blk in model.blocks:
        blk.build((None, 5, 64))
    model.final_norm.build((None, 5, 64))
    per_block = ['norm1.gamma', 'norm1.beta', 'attention.kernel', 'attention.bias', 'attention.out_kernel', 'attention.out_bias', 'norm2.gamma',
                 'norm2.beta', 'ff1.r', 'ff1.bias', 'ff2.r', 'ff2.bias']
    assert list(model.state_dict()) == ['embed.r', 'embed.bias'] + ['blocks.%d.%s' % (i, n) for i in range(2) for n in per_block] + [
        'final_norm.gamma', 'final_norm.beta']
    assert isinstance(model, TimitQLSTM) and all(hasattr(model, n) for n in ('ctc_loss', 'decode', 'evaluate', 'align', 'error_breakdown'))
    # the other models are what they were: no new module, parameter or key without an option
    lstm = TimitQLSTM(1, 64)
    lstm.rnn[0].build((None, 5, 164))
    assert list(lstm.state_dict()) == ['rnn.0.kernel', 'rnn.0.recurrent_kernel', 'rnn.0.bias']
    for other in (TimitQCNN(), lstm):
        names = [n for n, _ in other.named_modules()]
        assert not any(w in n for n in names for w in ('attention', 'blocks', 'embed', 'final_norm'))


# every entry of ATTN_SYMBOLS against the hygiene case that exercises it, or the reason it has none
HYGIENE_COVER = {
    'qk_qattn_fwd': 'test_forward_and_backward_keep_to_their_buffers: mfma (bf16, dq 16, lengths) and generic (fp32, dq 5)',
    'qk_qattn_bwd': 'test_forward_and_backward_keep_to_their_buffers: the same calls',
    'qk_qattn_supported': 'host only: takes no device buffer (test_dispatch_predicate_and_descriptor_checks_need_no_gpu)',
    'qk_qattn_workspace_bytes': 'host only: *_bytes',
}


def test_every_attn_entry_point_has_a_hygiene_case_or_a_reason():
    assert set(HYGIENE_COVER) == set(_lib.ATTN_SYMBOLS)


# ---- GPU part ------------------------------------------------------------------------------------------------------------------
def _run(dev, dtype, dq, lengths=True, steps=T, scale=None, poison=None, packed=False):
    """functional.qattention (packed: qattention_packed) forward and backward on _inputs(...): name -> tensor."""
    i = _inputs(dq, KINDS[dtype], steps)
    ops = {n: i[n] for n in ('q', 'k', 'v', 'do')}
    if poison is not None:
        inactive = (np.arange(steps)[None, :] >= i['lengths'][:, None])[:, :, None]
        ops = {n: np.where(inactive, poison, a) for n, a in ops.items()}
    t = lambda a: torch.tensor(a, dtype=dtype, device=dev)
    ln = torch.tensor(i['lengths'], device=dev) if lengths else None
    if packed:
        qkv = t(R.merge_packed(ops['q'], ops['k'], ops['v'])).requires_grad_()
        o = F.qattention_packed(qkv, H, ln, scale)
        o.backward(t(ops['do']))
        dq_, dk_, dv_ = R.split_packed(qkv.grad)
        return dict(o=o.detach(), dq=dq_, dk=dk_, dv=dv_, dqkv=qkv.grad)
    q, k, v = (t(ops[n]).requires_grad_() for n in ('q', 'k', 'v'))
    o = F.qattention(q, k, v, H, ln, scale)
    o.backward(t(ops['do']))
    return dict(o=o.detach(), dq=q.grad, dk=k.grad, dv=v.grad)


def _check(got, want, dtype, what='', names=NAMES):
    errs = {}
    for name in names:
        g = got[name]
        assert g.dtype == dtype and tuple(g.shape) == want[name].shape, name
        errs[name] = _rel(g.float().cpu().numpy(), want[name])
    print(what, errs)
    assert all(e <= BOUND[KINDS[dtype]] for e in errs.values()), errs


def _assert_inactive_zero(got, lengths, steps, dev):
    inactive = torch.tensor(np.arange(steps)[None, :] >= lengths[:, None], device=dev)
    assert int(inactive.sum()) > 0
    for name in NAMES:                                   # asserted, not tolerated
        assert int(got[name][inactive].ne(0).sum()) == 0, name


@pytest.mark.gpu
@pytest.mark.parametrize('lengths', [True, False], ids=['lengths', 'all_rows'])
@pytest.mark.parametrize('dq', DQS)
@pytest.mark.parametrize('dtype', list(KINDS), ids=DTYPE_IDS)
def test_forward_and_backward_match_the_reference(dtype, dq, lengths):
    dev = _dev()
    assert F.qattention_path(dtype, B, T, H, dq) == _expected_path(dtype, dq)
    got = _run(dev, dtype, dq, lengths)
    _check(got, _reference(dq, KINDS[dtype], lengths), dtype)
    if lengths:
        _assert_inactive_zero(got, LENGTHS, T, dev)


@pytest.mark.gpu
@pytest.mark.parametrize('dtype,dq', [(torch.bfloat16, 16), (torch.float16, 32), (torch.float32, 5)], ids=['mfma_bf16', 'mfma_fp16', 'generic'])
def test_saved_lse_and_a_single_step(dtype, dq):
    """lse through the C-ABI (the autograd function keeps it to itself): fp32, 1e-4 on the 16-bit paths too, exact zeros at inactive
    rows; and T = 1, where every active row attends to itself alone: p = 1, o = v and dv = do exactly, and dq = dk = 0 in exact
    arithmetic (dS = dP - delta = 0).  The kernels form dP and delta as two fp32 sums of the same 4 dq products in different orders, so
    dq and dk are held to an absolute 1e-4: 4 dq 2^-24 sum|do v| scale |k| is below 1e-5 for these unit-variance operands."""
    dev = _dev()
    i = _inputs(dq, KINDS[dtype])
    raw = _raw_call(dev, dtype, dq, 4 * H * dq, 0)
    want = _reference(dq, KINDS[dtype])['lse']
    assert float(np.abs(raw['lse'].cpu().numpy() - want).max()) <= 1e-4 * max(1.0, float(np.abs(want).max()))
    inactive = torch.tensor(np.arange(T)[None, :] >= i['lengths'][:, None], device=dev)
    assert int(raw['lse'].transpose(1, 2)[inactive].ne(0).sum()) == 0
    got = _run(dev, dtype, dq, steps=1)
    want1 = _reference(dq, KINDS[dtype], steps=1)
    _check(got, want1, dtype, 'T = 1', ('o', 'dv'))
    assert float(np.abs(want1['dq']).max()) <= 1e-12 and float(np.abs(want1['dk']).max()) <= 1e-12
    assert float(got['dq'].float().abs().max()) <= 1e-4 and float(got['dk'].float().abs().max()) <= 1e-4
    one = _inputs(dq, KINDS[dtype], 1)
    assert int(got['o'][0].ne(0).sum()) == 0
    if dtype != torch.float32:                     # p within an fp32 ulp of 1: the rounding of o gives v back
        assert torch.equal(got['o'][1:], torch.tensor(one['v'][1:], dtype=dtype, device=dev))


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['fp32_generic', 'bf16_mfma'])
def test_overflow_scores_past_a_hundred_stay_finite_and_within_the_bounds(dtype):
    """dq 16 with scale OVERFLOW_SCALE: the scores pass +-100, exp of them unshifted would overflow fp32.  Everything is finite; fp32
    keeps 1e-4 on all four tensors, bf16 keeps its bound on o and dv.  The bf16 dq and dk are held to finiteness only: there the
    rounding points alone move the float64 result by more than half the bound (test_rounding_points_on_the_overflow_inputs: 5.7e-3
    and 1.1e-2), so no bound on them would test the kernel."""
    dev = _dev()
    kind = KINDS[dtype]
    i = _inputs(16, kind)
    s = R.scores(i['q'], i['k'], H, OVERFLOW_SCALE)
    assert s.max() > 100 and s.min() < -100
    got = _run(dev, dtype, 16, scale=OVERFLOW_SCALE)
    for name in NAMES:
        assert bool(torch.isfinite(got[name]).all()), name
    _check(got, _reference(16, kind, scale=OVERFLOW_SCALE), dtype, 'overflow', NAMES if kind is None else ('o', 'dv'))
    _assert_inactive_zero(got, LENGTHS, T, dev)


@pytest.mark.gpu
@pytest.mark.parametrize('dtype,dq', [(torch.bfloat16, 16), (torch.float16, 32), (torch.float32, 5), (torch.bfloat16, 8)],
                         ids=['mfma_bf16', 'mfma_fp16', 'generic_fp32', 'generic_bf16'])
def test_poisoned_padding_changes_no_bit(dtype, dq):
    """Rows t >= lengths[b] of q, k, v, do filled with NaN: bit-equal to the run with zeros there."""
    dev = _dev()
    clean, poisoned = _run(dev, dtype, dq, poison=0.0), _run(dev, dtype, dq, poison=np.nan)
    for name in NAMES:
        assert GA.first_bit_difference(poisoned[name], clean[name]) is None, name
    _check(poisoned, _reference(dq, KINDS[dtype]), dtype, 'poisoned')


@pytest.mark.gpu
@pytest.mark.parametrize('dtype,dq', [(torch.bfloat16, 32), (torch.float16, 16), (torch.float32, 5)], ids=['mfma_bf16', 'mfma_fp16', 'generic'])
def test_two_calls_agree_bit_for_bit(dtype, dq):
    """No atomics: dk / dv and dq come from kernels that own their output rows."""
    dev = _dev()
    first, again = _run(dev, dtype, dq), _run(dev, dtype, dq)
    for name in first:
        assert GA.first_bit_difference(first[name], again[name]) is None, name


def _raw_call(dev, dtype, dq, width, off, use_lengths=True):
    """qk_qattn_fwd / _bwd through ctypes: every tensor is the column window [off, off + 4Q) of its own (B * T, width) buffer with its
    own fill.  Returns name -> wide buffer, and lse."""
    lib = _lib.lib()
    i = _inputs(dq, KINDS[dtype])
    Q = H * dq
    N, W = B * T, 4 * Q
    bufs = {n: torch.full((N, width), fill, dtype=dtype, device=dev)
            for n, fill in (('q', 3.0), ('k', 5.0), ('v', 7.0), ('o', 9.0), ('do', 11.0), ('dq', 13.0), ('dk', 15.0), ('dv', 17.0))}
    for n in ('q', 'k', 'v', 'do'):
        bufs[n][:, off:off + W] = torch.tensor(i[n], dtype=dtype, device=dev).view(N, W)
    ln = torch.tensor(i['lengths'], device=dev) if use_lengths else None
    lse = torch.empty((B, H, T), dtype=torch.float32, device=dev)
    pair = (width, Q)
    desc = F.qattention_desc(dtype, B, T, H, dq, pair, pair, pair, pair)
    n = int(lib.qk_qattn_workspace_bytes(ctypes.byref(desc), _lib.QK_OP_BWD))
    ws = torch.empty(n, dtype=torch.uint8, device=dev)
    es = bufs['q'].element_size()
    stream = torch.cuda.current_stream(dev).cuda_stream
    p = lambda name: bufs[name].data_ptr() + off * es
    lp = ln.data_ptr() if ln is not None else None
    with torch.cuda.device(dev):
        _lib.check(lib.qk_qattn_fwd(ctypes.byref(desc), p('q'), p('k'), p('v'), lp, 0.0, p('o'), lse.data_ptr(), stream), 'qk_qattn_fwd')
        _lib.check(lib.qk_qattn_bwd(ctypes.byref(desc), p('do'), p('q'), p('k'), p('v'), p('o'), lse.data_ptr(), lp, 0.0, p('dq'), p('dk'),
                                    p('dv'), ws.data_ptr(), n, stream), 'qk_qattn_bwd')
    torch.cuda.synchronize(dev)
    bufs['lse'] = lse
    return bufs


@pytest.mark.gpu
@pytest.mark.parametrize('dtype,dq,width,off,same', [(torch.bfloat16, 16, 4 * 48 + 24, 8, True), (torch.float32, 5, 67, 3, True),
                                                     (torch.bfloat16, 16, 4 * 48 + 24, 1, False), (torch.float16, 32, 4 * 96 + 3, 0, False)],
                         ids=['mfma_bf16', 'generic_fp32', 'mfma_width_misaligned_pointers', 'mfma_width_odd_strides'])
def test_column_windows_equal_the_dense_call_and_leave_the_other_columns_alone(dtype, dq, width, off, same):
    """Every tensor is a column window of a wider buffer.  same: the strided call runs the kernels of the dense call and the results
    are bit-equal; else (a matrix-kernel width whose runs or pointers are not 16-byte aligned runs the generic kernels) they keep the
    parity bounds.  The columns outside the windows are untouched either way."""
    dev = _dev()
    W = 4 * H * dq
    dense = _raw_call(dev, dtype, dq, W, 0)
    wide = _raw_call(dev, dtype, dq, width, off)
    window = lambda n: wide[n][:, off:off + W]
    if same:
        for n in NAMES:
            assert GA.first_bit_difference(window(n), dense[n]) is None, n
        assert GA.first_bit_difference(wide['lse'], dense['lse']) is None
    else:
        _check({n: window(n).reshape(B, T, W) for n in NAMES}, _reference(dq, KINDS[dtype]), dtype, 'generic kernels at a matrix-kernel width')
    for n, fill in (('q', 3.0), ('k', 5.0), ('v', 7.0), ('o', 9.0), ('do', 11.0), ('dq', 13.0), ('dk', 15.0), ('dv', 17.0)):
        outside = torch.cat([wide[n][:, :off], wide[n][:, off + W:]], dim=1)
        assert bool((outside == fill).all()), n
    # the same through the autograd function: column windows of wider tensors are read in place
    i = _inputs(dq, KINDS[dtype])
    q, k, v = (wide[n][:, off:off + W].view(B, T, W).detach().requires_grad_() for n in ('q', 'k', 'v'))
    assert F._attn_rows(q, W)[0].data_ptr() == q.data_ptr()
    o = F.qattention(q, k, v, H, torch.tensor(i['lengths'], device=dev))
    o.backward(wide['do'][:, off:off + W].view(B, T, W))
    got = dict(o=o.detach(), dq=q.grad, dk=k.grad, dv=v.grad)
    if same:
        assert GA.first_bit_difference(got['o'].reshape(B * T, W), dense['o']) is None
    _check(got, _reference(dq, KINDS[dtype]), dtype, 'autograd on windows')


@pytest.mark.gpu
@pytest.mark.parametrize('dtype,dq', [(torch.bfloat16, 16), (torch.float16, 32), (torch.float32, 8)], ids=['mfma_bf16', 'mfma_fp16', 'generic'])
def test_packed_projection_output_equals_the_three_tensor_call(dtype, dq):
    """qattention_packed on a (B, T, 12Q) buffer: same path as the dense call, bit-equal to it, and ONE (B, T, 12Q) gradient."""
    dev = _dev()
    assert F.qattention_path(dtype, B, T, H, dq, packed=True) == _expected_path(dtype, dq)
    dense, packed = _run(dev, dtype, dq), _run(dev, dtype, dq, packed=True)
    assert tuple(packed['dqkv'].shape) == (B, T, 12 * H * dq) and packed['dqkv'].is_contiguous()
    for name in NAMES:
        assert GA.first_bit_difference(packed[name].contiguous(), dense[name]) is None, name


@pytest.mark.gpu
@pytest.mark.parametrize('dtype,dq', [(torch.bfloat16, 16), (torch.float32, 5)], ids=['mfma', 'generic'])
def test_forward_and_backward_replay_from_a_captured_graph(dtype, dq):
    """functional.qattention forward + backward captured on one stream and replayed three times: bit-equal to the eager call.  That it
    captures at all shows that the launches read nothing on the host."""
    dev = _dev()
    eager = _run(dev, dtype, dq)
    i = _inputs(dq, KINDS[dtype])
    t = lambda a: torch.tensor(a, dtype=dtype, device=dev)
    q, k, v = (t(i[n]).requires_grad_() for n in ('q', 'k', 'v'))
    do, ln = t(i['do']), torch.tensor(i['lengths'], device=dev)

    def body():
        o = F.qattention(q, k, v, H, ln)
        return (o.detach(),) + torch.autograd.grad(o, (q, k, v), do)
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
    for name, o in zip(NAMES, outs):
        assert GA.first_bit_difference(o, eager[name]) is None, name


@pytest.mark.gpu
@pytest.mark.parametrize('dtype,dq,packed', [(torch.bfloat16, 16, False), (torch.bfloat16, 16, True), (torch.float32, 5, False)],
                         ids=['mfma_bf16', 'mfma_bf16_packed', 'generic'])
def test_forward_and_backward_keep_to_their_buffers(monkeypatch, dtype, dq, packed):
    """functional.qattention forward and backward under guard bands and the two fills: no stray write, every returned element written,
    the two runs bit-identical (nothing depends on what the workspace, lse or an output held before the call)."""
    dev = _dev()

    def run(alloc):
        return _run(dev, dtype, dq, packed=packed)
    res = GA.run_twice(run, monkeypatch, modules=(F,))
    GA.assert_hygiene(res, 'qattention %s dq=%d: ' % (dtype, dq))
    sites = {a.site.split(':')[0] for a in res.allocs[0].log}
    assert sites == {'functional.py'} and len(res.allocs[0].log) == (4 if packed else 6)        # o, lse, the gradient(s), workspace


def _dense_t(x, w, b):
    return x @ LR.expand_t(w) + b


def _mha_t(x, p, prefix, heads, lengths):
    b, t, w = x.shape
    qkv = _dense_t(x.reshape(b * t, w), p[prefix + 'kernel'], p[prefix + 'bias']).reshape(b, t, -1)
    o = R.qattention_t(*R.split_packed(qkv), heads, lengths)
    return _dense_t(o.reshape(b * t, -1), p[prefix + 'out_kernel'], p[prefix + 'out_bias']).reshape(b, t, -1)


@pytest.mark.gpu
@pytest.mark.parametrize('dtype,units,heads', [(torch.float32, 64, 2), (torch.bfloat16, 128, 2)], ids=['fp32_generic', 'bf16_mfma'])
def test_layer_matches_the_float64_composition(dtype, units, heads):
    """QuaternionMultiHeadAttention at B 4, T 20, in_q 10: output, input gradient and the four parameter gradients against dense +
    qattn_ref in float64: fp32 within 1e-4; bf16 activations (dq 16: the matrix kernels) within 2e-2."""
    dev = _dev()
    rng = np.random.RandomState(12)
    layer = QuaternionMultiHeadAttention(units, heads, seed=7)
    x = torch.tensor(rng.randn(4, 20, 40), dtype=torch.float32, device=dev).to(dtype)
    lengths = torch.tensor([20, 7, 13, 1], dtype=torch.int32, device=dev)
    w = torch.tensor(rng.randn(4, 20, units), dtype=torch.float32, device=dev).to(dtype)
    layer.ensure_built(x.shape, dev)
    with torch.no_grad():
        layer.bias.add_(torch.tensor(0.3 * rng.randn(3 * units), dtype=torch.float32, device=dev))
        layer.out_bias.add_(torch.tensor(0.3 * rng.randn(units), dtype=torch.float32, device=dev))
    x.requires_grad_()
    y = layer(x, lengths=lengths)
    y.backward(w)
    x64 = x.detach().double().cpu().requires_grad_()
    p64 = {n: p.detach().double().cpu().requires_grad_() for n, p in layer.weights}
    y64 = _mha_t(x64, p64, '', heads, lengths.cpu())
    (y64 * w.double().cpu()).sum().backward()
    tol = 1e-4 if dtype == torch.float32 else 2e-2
    errs = dict(y=_rel(y.detach().float().cpu().numpy(), y64.detach().numpy()), dx=_rel(x.grad.float().cpu().numpy(), x64.grad.numpy()))
    errs.update({n: _rel(p.grad.cpu().numpy(), p64[n].grad.numpy()) for n, p in layer.weights})
    print(errs)
    assert max(errs.values()) <= tol, errs


def _small_model(dev, seed):
    """TimitQTransformer(2, 64, heads=2, ff_units=128, dropout=0) at B 4, T 20 with its batch; parameters fp32, built."""
    np.random.seed(seed)
    torch.manual_seed(seed)
    model = TimitQTransformer(2, 64, heads=2, ff_units=128, dropout=0)
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
    """mean CTC cost of the float64 composition (dense, qlnorm_ref, qattn_ref) and its gradients, by parameter name."""
    from qcnn_amd.models.qtransformer_model import sinusoidal_positions
    p64 = {n: p.detach().double().cpu().requires_grad_() for n, p in model.named_parameters()}
    b, _, f, t = x.shape
    lengths = il.reshape(-1).cpu()
    o = _dense_t(x.double().cpu().permute(0, 3, 1, 2).reshape(b * t, 4 * f), p64['embed.r'], p64['embed.bias']).reshape(b, t, -1)
    o = o + sinusoidal_positions(t, o.shape[-1]).double()
    for i in range(len(model.blocks)):
        pre = 'blocks.%d.' % i
        h = NR.qlayer_norm_t(o, p64[pre + 'norm1.gamma'], p64[pre + 'norm1.beta'], lengths, epsilon=model.blocks[i].norm1.epsilon)
        o = o + _mha_t(h, p64, pre + 'attention.', model.blocks[i].heads, lengths)
        h = NR.qlayer_norm_t(o, p64[pre + 'norm2.gamma'], p64[pre + 'norm2.beta'], lengths, epsilon=model.blocks[i].norm2.epsilon)
        h = torch.relu(_dense_t(h.reshape(b * t, -1), p64[pre + 'ff1.r'], p64[pre + 'ff1.bias']))
        o = o + _dense_t(h, p64[pre + 'ff2.r'], p64[pre + 'ff2.bias']).reshape(b, t, -1)
    o = NR.qlayer_norm_t(o, p64['final_norm.gamma'], p64['final_norm.beta'], lengths, epsilon=model.final_norm.epsilon)
    pred = torch.softmax(o @ p64['pred.layer.kernel'] + p64['pred.layer.bias'], dim=-1)
    logp = torch.log_softmax(torch.log(pred + 1e-7), dim=-1).transpose(0, 1)              # K.ctc_batch_cost (layers.ctc_batch_cost)
    cost = torch.nn.functional.ctc_loss(logp, labels.long().cpu(), lengths.long(), ll.reshape(-1).long().cpu(), blank=61, reduction='none')
    loss = cost.mean()
    loss.backward()
    return float(loss.detach()), {n: p.grad.numpy() for n, p in p64.items()}


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['fp32', 'bf16'])
def test_model_step_matches_the_composition_and_ignores_padding_frames(dtype):
    """TimitQTransformer(2, 64, heads=2, ff_units=128, dropout=0) through ctc_mean_loss at B 4, T 20.  fp32: the loss and all 32
    parameter gradients within 1e-4 of the float64 composition.  bf16: the composition has no rounding points and the model chains
    17 stages that each round (the project's 1e-2 per stage would add up to a bound that tests nothing), so the gradients are held to
    finiteness and the loss to 1e-2 of the fp32 model's; each stage's own bf16 parity is its own test.  Both: one guarded scheduled step
    runs on the parameters, and the posteriors at frames < input_length are bit-unchanged when the padding frames of the input are
    replaced by noise."""
    from qcnn_amd import dp
    from qcnn_amd.training import GradGuard, LRSchedule, ScheduledAdam
    dev = _dev()
    model, x, labels, il, ll = _small_model(dev, 31)
    xd = x.to(dtype)
    loss = model.ctc_mean_loss(xd, labels, il, ll)
    loss.backward()
    want_loss, want = _model_reference(model, x, labels, il, ll)
    errs = {n: _rel(p.grad.cpu().numpy(), want[n]) for n, p in model.named_parameters()}
    print(float(loss.detach()), want_loss, errs)
    assert len(errs) == 2 + 2 * 12 + 2 + 2
    if dtype == torch.float32:
        assert abs(float(loss.detach()) - want_loss) <= 1e-4 * abs(want_loss) and max(errs.values()) <= 1e-4, errs
    else:
        assert abs(float(loss.detach()) - want_loss) <= 1e-2 * abs(want_loss)
        assert all(bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0 for p in model.parameters())
    with torch.no_grad():
        model.eval()
        clean = model(xd, il)
        noisy_x = xd.clone()
        pad = torch.arange(20, device=dev)[None, :] >= il.reshape(-1, 1)
        noisy_x.permute(0, 3, 1, 2)[pad] = 37.0 * torch.randn(int(pad.sum()), 4, 41, device=dev).to(dtype)
        noisy = model(noisy_x, il)
        assert int(pad.sum()) > 0 and not torch.equal(noisy_x, xd)
        assert GA.first_bit_difference(noisy[~pad], clean[~pad]) is None
        model.train()
    for p in model.parameters():
        p.grad = None
    flat = dp.FlatParams([p for p in model.parameters() if p.requires_grad], direct=True)
    guard = GradGuard(dev, clipnorm=50.0, loss_scale=4.0)
    opt = ScheduledAdam(flat.param, flat.grad, LRSchedule(5e-3), guard=guard)
    model.training_loss(xd, labels, il, ll, loss_scale=guard.loss_scale).backward()
    opt.step()
    assert opt.stats()['step'] == 1 and guard.stats()['skipped_steps'] == 0
    assert np.isfinite(float(model.training_loss(xd, labels, il, ll)))
