"""Transducer (RNN-T) loss (include/qk_rnnt.h; qcnn_amd.functional.rnnt_loss / rnnt_cost_and_grad, qcnn_amd.layers.rnnt_batch_cost,
qcnn_amd.models.TimitQTransducer) against the float64 restatement and the brute-force enumeration of tests/rnnt_ref.py.

Bounds: tests/rnnt_ref.py states them and where they come from -- cost 2e-5 relative; gradient, against the largest entry, 5e-4
(fp32), 1e-2 (bf16), 2e-3 (fp16), the figures of tests/test_ctc_enum.py.  Both sides see the SAME operands (logits already rounded
to the kernel's dtype), so the one rounding point between them is the stored gradient.

Rounding points (test_rounding_points_stay_under_half_the_16_bit_bound, on the GPU cases' operands): rounding the stored gradient
moves the float64 reference by at most 2.3e-3 of the largest entry in bf16 (half bound 5e-3; the largest shift is at U1 = 128) and
3.9e-4 in fp16 (half bound 1e-3; at V = 3).  Rounding the fp32 logits themselves to 16 bits is NOT a rounding point of the kernel:
it happens in front of both sides.  For the record it moves the cost by up to 2.6e-4 relative in bf16 and 5.6e-5 in fp16 (both above
the cost bound, which is why parity is taken on the rounded operands) and the gradient by up to 9.0e-3 (U1 = 65) and 7.0e-4 (U1 =
128) of the largest entry.
"""
import ctypes
import functools
import os
import re

import numpy as np
import pytest
import torch

import guarded_alloc as GA
import qlstm_ref as QR
import rnnt_ref as R
from qcnn_amd import _lib, functional as F, layers
from qcnn_amd.models import TimitQCNN, TimitQConformer, TimitQLSTM, TimitQTransducer, TimitQTransformer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = {torch.float32: None, torch.bfloat16: 'bf16', torch.float16: 'fp16'}
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
DTYPE_IDS = ['fp32', 'bf16', 'fp16']
# (B, T, Lmax, V): the issue's shapes.  U1 = 64 is one full wave of the lattice kernel, 65 crosses into its two-wave form, 128 is
# the limit; V = 61 makes a row an odd number of bytes in the 16-bit types; 17 * 6 * 5 = 510 rows are 16 row tiles of 32.
SHAPES = [(3, 12, 5, 62), (2, 9, 7, 3), (3, 40, 63, 62), (3, 40, 64, 62), (2, 20, 127, 5), (2, 1, 6, 61), (17, 6, 4, 62)]
SHAPE_IDS = ['b3_t12_l5_v62', 'b2_t9_l7_v3', 'u1_64', 'u1_65', 'u1_128', 't1_v61', 'b17']
TINY = [(1, 0, 2), (1, 3, 3), (4, 0, 3), (3, 2, 4), (5, 3, 4), (4, 4, 3)]           # (T, U, V) of the enumeration


def _dev():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    return torch.device('cuda:0')


def _rel(got, want):
    return float(np.abs(np.asarray(got, dtype=np.float64) - want).max()) / max(float(np.abs(want).max()), 1e-30)


@functools.lru_cache(maxsize=None)
def _case(idx, kind, rounded=True):
    """Seeded operands of SHAPES[idx] (never written): ragged lengths with a row at full T and Lmax, a row with Ub = 0 and a row with
    Tb = 1 in every batch (at B = 2 the second row is both); the logits rounded to `kind`."""
    b, t, lmax, v = SHAPES[idx]
    rng = np.random.RandomState(7100 + idx)
    il, ll = rng.randint(1, t + 1, size=b), rng.randint(0, lmax + 1, size=b)
    il[0], ll[0] = t, lmax
    if b == 2:
        il[1], ll[1] = 1, 0
    else:
        ll[1], il[2] = 0, 1
    labels = rng.randint(0, v - 1, size=(b, lmax))
    x = (1.5 * rng.randn(b, t, lmax + 1, v)).astype(np.float32).astype(np.float64)
    d = dict(x=R.rnd(x, kind) if rounded else x, labels=labels, il=il.astype(np.int32), ll=ll.astype(np.int32))
    for a in d.values():
        a.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def _reference(idx, kind, rounded=True, grad_kind='same'):
    c = _case(idx, kind, rounded)
    cost, grad = R.rnnt(c['x'], c['labels'], c['il'], c['ll'], grad_kind=kind if grad_kind == 'same' else grad_kind)
    cost.setflags(write=False)
    grad.setflags(write=False)
    return cost, grad


def _active(c):
    t, u1 = c['x'].shape[1:3]
    return (np.arange(t)[None, :, None] < c['il'][:, None, None]) & (np.arange(u1)[None, None, :] <= c['ll'][:, None, None])


def _tiny(t, u, v):
    rng = np.random.RandomState(90 + 16 * t + 4 * u + v)
    return rng.randn(1, t, u + 1, v), rng.randint(0, v - 1, size=(1, u))


def _gpu_call(c, dtype, dev, grad=True):
    x = torch.tensor(c['x'], dtype=dtype, device=dev)
    args = (torch.tensor(c['labels'], device=dev), torch.tensor(c['il'], device=dev), torch.tensor(c['ll'], device=dev))
    if grad:
        return F.rnnt_cost_and_grad(x, *args)
    return F.rnnt_loss(x, *args).reshape(-1), None


# ---- CPU part -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('t,u,v', TINY)
def test_reference_equals_the_enumeration_and_central_differences(t, u, v):
    """The recursion of the header against the sum over every alignment (1e-10) and its gradient against central differences of that
    sum (1e-6); every gradient row sums to zero and |g| <= 1."""
    x, labels = _tiny(t, u, v)
    cost, grad = R.rnnt(x, labels, [t], [u])
    want = R.enumerate_cost(x[0], labels[0])
    assert abs(cost[0] - want) <= 1e-10 * max(1.0, abs(want)), (cost[0], want)
    num = R.central_differences(x[0], labels[0])
    assert np.abs(grad[0] - num).max() <= 1e-6, np.abs(grad[0] - num).max()
    assert np.abs(grad.sum(axis=-1)).max() <= 1e-12 and np.abs(grad).max() <= 1.0 and np.abs(grad).max() > 0


def test_reference_conventions():
    """Inactive cells take no gradient and are never read (NaN); Tb = 0 and labels outside [0, V - 2] inside the label length are
    infeasible; a bad label BEHIND the label length is padding."""
    rng = np.random.RandomState(3)
    x = rng.randn(4, 5, 4, 6)
    labels = np.array([[1, 2, 0], [5, 1, 1], [0, -1, 2], [2, 9, -7]])
    il, ll = np.array([5, 4, 3, 3]), np.array([3, 2, 2, 1])
    cost, grad = R.rnnt(x, labels, il, ll)
    assert np.isfinite(cost[0]) and np.isinf(cost[1]) and np.isinf(cost[2]) and np.isfinite(cost[3])
    assert (grad[1] == 0).all() and (grad[2] == 0).all() and (grad[3, 3:] == 0).all() and (grad[3, :, 2:] == 0).all()
    assert np.isinf(R.rnnt(x, labels, [0, 0, 0, 0], ll)[0]).all()
    noisy = x.copy()
    noisy[3, 3:] = np.nan
    noisy[3, :, 2:] = np.nan
    cost2, grad2 = R.rnnt(noisy, labels, il, ll)
    assert np.array_equal(cost2, cost) and np.array_equal(grad2, grad)


@pytest.mark.parametrize('idx', [0, 1, 5, 6], ids=[SHAPE_IDS[i] for i in (0, 1, 5, 6)])
def test_torch_path_equals_the_reference(idx):
    """layers.rnnt_batch_cost on CPU tensors (log_softmax, the anti-diagonal recursion, autograd) against the float64 reference at
    the fp32 bounds of the project's CTC torch path: 2e-6 on the cost, 1e-4 on the gradient; NaN in the padding cells goes nowhere."""
    c = _case(idx, None)
    cost, grad = _reference(idx, None, True, 'none')
    x = torch.tensor(c['x'], dtype=torch.float32)
    x = torch.where(torch.tensor(_active(c))[..., None], x, torch.full((), float('nan'))).requires_grad_()
    got = layers.rnnt_batch_cost(x, torch.tensor(c['labels']), torch.tensor(c['il']), torch.tensor(c['ll']))
    assert got.shape == (x.shape[0], 1)
    got.sum().backward()
    assert _rel(got.detach().numpy().reshape(-1), cost) <= 2e-6
    assert _rel(x.grad.numpy(), grad) <= 1e-4
    assert (x.grad.numpy()[~_active(c)] == 0).all()


def test_torch_path_conventions_and_loss_scale():
    rng = np.random.RandomState(4)
    x = torch.tensor(rng.randn(3, 4, 3, 5), dtype=torch.float32, requires_grad=True)
    labels = torch.tensor([[1, 2], [4, 0], [0, 7]])
    il, ll = torch.tensor([4, 4, 0]), torch.tensor([[2], [1], [1]])
    cost = layers.rnnt_batch_cost(x, labels, il, ll)
    assert np.isfinite(float(cost[0].detach())) and np.isinf(float(cost[1].detach())) and np.isinf(float(cost[2].detach()))
    cost[0].backward()
    g1 = x.grad.clone()
    assert (g1[1:] == 0).all() and float(g1[0].abs().max()) > 0
    x.grad = None
    scaled = layers.rnnt_batch_cost(x, labels, il, ll, loss_scale=8.0)
    assert torch.equal(scaled.detach(), cost.detach())
    scaled[0].backward()
    assert torch.equal(x.grad, 8.0 * g1)
    with pytest.raises(ValueError):
        layers.rnnt_batch_cost(x, labels[:, :1], il, ll)


def test_rnnt_header_inventory_equals_the_eighth_symbol_table():
    lib = _lib.lib()
    h = open(os.path.join(ROOT, 'include', 'qk_rnnt.h')).read()
    declared = set(re.findall(r'\b(qk_rnnt_[a-z_0-9]+)\s*\(', h))
    assert declared == set(_lib.RNNT_SYMBOLS), declared ^ set(_lib.RNNT_SYMBOLS)
    for name in declared:
        assert hasattr(lib, name), name
    for other in (_lib.SYMBOLS, _lib.OPT_SYMBOLS, _lib.DATA_SYMBOLS, _lib.RNN_SYMBOLS, _lib.NORM_SYMBOLS, _lib.ATTN_SYMBOLS, _lib.DWCONV_SYMBOLS):
        assert not set(_lib.RNNT_SYMBOLS) & set(other)
    main = open(os.path.join(ROOT, 'include', 'qk.h')).read()
    assert 'rnnt' not in main
    declared_main = set(re.findall(r'\b(qk_[a-z_0-9]+)\s*\(', main))
    declared_main -= {n for n in declared_main if n.endswith('_t')}
    assert declared_main == set(_lib.SYMBOLS)                                         # the pinned inventory of include/qk.h is unchanged
    decls = {name: (res, args) for res, name, args in re.findall(r'^(int|size_t) (qk_[a-z_0-9]+)\(([^;]*)\);', h, re.M | re.S)}
    assert set(decls) == set(_lib.RNNT_SYMBOLS)
    for name, (res, args) in decls.items():
        restype, argtypes = _lib.RNNT_SYMBOLS[name]
        assert restype is (ctypes.c_int if res == 'int' else ctypes.c_size_t), name
        assert len(argtypes) == len(re.sub(r'/\*.*?\*/', '', args, flags=re.S).split(',')), name
        if name == 'qk_rnnt_loss':
            assert ' '.join(args.split(',')[-1].split()) == 'void *stream' and argtypes[-1] is ctypes.c_void_p
        else:                                                       # host only
            assert 'stream' not in args, name
    for macro in ('QK_RNNT_MAX_CLASSES', 'QK_RNNT_MAX_U1'):
        assert int(re.search(r'#define %s (\d+)' % macro, h).group(1)) == getattr(_lib, macro)
    assert lib.qk_version() == 103


def test_support_predicate_workspace_formula_and_descriptor_errors_need_no_gpu():
    lib = _lib.lib()
    for dtype in (_lib.QK_F32, _lib.QK_BF16, _lib.QK_F16):
        assert lib.qk_rnnt_supported(dtype, 256, 200, 76, 62) == 1
        assert lib.qk_rnnt_supported(dtype, 1, 1, 1, 2) == 1 and lib.qk_rnnt_supported(dtype, 2, 20, 128, 256) == 1
    assert lib.qk_rnnt_supported(7, 3, 12, 6, 62) == 0 and lib.qk_last_error()

    def formula(b, t, u1):
        return 4 * (3 * b * t * u1 + 2 * b * (t + u1 - 1) * u1 + (b + 3) // 4 * 4)
    for b, t, lmax, v in SHAPES + [(256, 200, 75, 62)]:
        assert lib.qk_rnnt_workspace_bytes(b, t, lmax + 1, v) == formula(b, t, lmax + 1)
    assert formula(256, 200, 76) == 89498624
    for b, t, u1, v in ((3, 12, 6, 1), (3, 12, 6, 257), (3, 12, 129, 62), (3, 12, 0, 62), (3, 0, 6, 62), (0, 12, 6, 62), (1 << 16, 1 << 10, 128, 62)):
        assert lib.qk_rnnt_supported(_lib.QK_F32, b, t, u1, v) == 0 and lib.qk_last_error(), (b, t, u1, v)
        assert lib.qk_rnnt_workspace_bytes(b, t, u1, v) == 0
        assert lib.qk_rnnt_loss(_lib.QK_F32, b, t, u1, v, *([None] * 7), 0, None) == _lib.QK_ERR_UNSUPPORTED, (b, t, u1, v)
    assert lib.qk_rnnt_loss(7, 3, 12, 6, 62, *([None] * 7), 0, None) == _lib.QK_ERR_INVALID_ARG                  # dtype
    assert lib.qk_rnnt_loss(_lib.QK_F32, 3, 12, 6, 62, *([None] * 7), 0, None) == _lib.QK_ERR_INVALID_ARG        # NULL buffers
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        F.rnnt_loss(torch.zeros(2, 3, 2, 5), torch.zeros(2, 1, dtype=torch.int32), torch.tensor([3, 3]), torch.tensor([1, 1]))
    assert not F.rnnt_supported(torch.zeros(2, 3, 2, 5), torch.zeros(2, 1, dtype=torch.int32))


TRANSDUCER_KEYS = ['embed.embeddings', 'pred_rnn.0.kernel', 'pred_rnn.0.recurrent_kernel', 'pred_rnn.0.bias', 'pred_rnn.1.kernel',
                   'pred_rnn.1.recurrent_kernel', 'pred_rnn.1.bias', 'joint_enc.r', 'joint_enc.bias', 'joint_pred.r', 'joint_out.kernel',
                   'joint_out.bias']


def test_model_surface():
    cpu = torch.device('cpu')
    enc = TimitQLSTM(1, 64, bidirectional=False)
    enc.rnn[0].build((None, 5, 164))
    before = list(enc.state_dict())
    assert before == ['rnn.0.kernel', 'rnn.0.recurrent_kernel', 'rnn.0.bias']
    model = TimitQTransducer(enc, pred_units=32, pred_layers=2, joint_units=48, dropout=0.0)
    model.ensure_built(64, cpu)
    assert list(enc.state_dict()) == before
    assert list(model.state_dict()) == ['encoder.' + k for k in before] + TRANSDUCER_KEYS
    shapes = {n: tuple(p.shape) for n, p in model.named_parameters()}
    assert shapes['embed.embeddings'] == (62, 32) and shapes['pred_rnn.1.kernel'] == (8, 128) and shapes['pred_rnn.0.recurrent_kernel'] == (8, 128)
    assert shapes['joint_enc.r'] == (16, 48) and shapes['joint_enc.bias'] == (48,) and shapes['joint_pred.r'] == (8, 48)
    assert shapes['joint_out.kernel'] == (48, 62) and shapes['joint_out.bias'] == (62,) and model.joint_pred.bias is None
    cfg = model.embed.get_config()
    assert cfg['input_dim'] == 62 and cfg['output_dim'] == 32 and cfg['name'] == 'pred_embed'
    assert type(model.embed).from_config(cfg).get_config() == cfg
    rnn_cfg = model.pred_rnn[0].get_config()
    assert rnn_cfg['units'] == 32 and rnn_cfg['bidirectional'] is False and rnn_cfg['return_state'] is True
    # the encoder's CTC output layer is unused: once built it is frozen, so it stays out of the optimiser's list and of the l2 term
    enc.pred.layer.ensure_built((None, 64), cpu)
    assert not any(p.requires_grad for p in enc.pred.parameters())
    trainable = [n for n, p in model.named_parameters() if p.requires_grad]
    assert trainable == ['encoder.' + k for k in before] + TRANSDUCER_KEYS
    reg = TimitQTransducer(TimitQLSTM(1, 64, bidirectional=False, l2=1e-3), pred_units=32, joint_units=48, l2=1e-3)
    reg.ensure_built(64, cpu)
    reg.encoder.rnn[0].build((None, 5, 164))
    reg.encoder.pred.layer.ensure_built((None, 64), cpu)
    want = 1e-3 * sum(float((p.detach().double() ** 2).sum()) for n, p in reg.named_parameters()
                      if n.split('.')[-1] in ('kernel', 'recurrent_kernel', 'r') and not n.startswith('encoder.pred'))
    assert abs(float(reg.regularization_loss().detach()) - want) <= 1e-5 * want
    for bad in (dict(pred_units=30), dict(joint_units=0), dict(pred_layers=0)):
        with pytest.raises(ValueError):
            TimitQTransducer(TimitQLSTM(1, 64), **bad)
    with pytest.raises(TypeError):
        TimitQTransducer(torch.nn.Linear(3, 3))
    # the three CTC models: nothing of the transducer in them
    for other in (TimitQCNN(), TimitQLSTM(1, 64), TimitQTransformer(2, 64, heads=2, ff_units=128), TimitQConformer(2, 64, heads=2, ff_units=128, kernel_size=7)):
        assert not any(w in n for n, _ in other.named_modules() for w in ('pred_rnn', 'joint', 'embed.embeddings'))
    lstm = TimitQLSTM(2, 64)
    for layer, width in zip(lstm.rnn, (164, 128)):
        layer.build((None, 5, width))
    lstm.pred.layer.ensure_built((None, 128), cpu)
    assert list(lstm.state_dict()) == ['rnn.0.kernel', 'rnn.0.recurrent_kernel', 'rnn.0.bias', 'rnn.1.kernel', 'rnn.1.recurrent_kernel',
                                       'rnn.1.bias', 'pred.layer.kernel', 'pred.layer.bias']
    assert all(p.requires_grad for p in lstm.parameters())


@pytest.mark.parametrize('kind', ['bf16', 'fp16'])
def test_rounding_points_stay_under_half_the_16_bit_bound(kind):
    """On the GPU cases' operands: the header's one rounding point (the stored gradient) moves the float64 reference by less than
    half of the 16-bit gradient bound; the cost has no rounding point.  (What rounding the LOGITS does is printed: it is not a
    rounding point of the kernel -- the module docstring has the figures.)"""
    worst = 0.0
    for idx in range(len(SHAPES)):
        _, exact = _reference(idx, kind, True, 'none')
        _, stored = _reference(idx, kind)
        assert np.abs(exact).max() > 0.5
        worst = max(worst, _rel(stored, exact))
        cost32, grad32 = _reference(idx, kind, False, 'none')
        cost16, _ = _reference(idx, kind, True, 'none')
        print(SHAPE_IDS[idx], kind, 'stored gradient %.3g; logits rounding: cost %.3g gradient %.3g'
              % (_rel(stored, exact), _rel(cost16, cost32), _rel(exact, grad32)))
    assert worst < 0.5 * R.GRAD_BOUND[kind], worst


# ---- GPU part -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize('idx', range(len(SHAPES)), ids=SHAPE_IDS)
def test_cost_and_gradient_match_the_reference(idx, dtype):
    """Parity on the rounded operands; inactive cells exactly zero; active rows sum to zero within the dtype's rounding of their
    entries: sum |g| <= 2 over a row (the positive and the negative parts are each at most 1) and every stored entry is within
    2^-p + 5e-4 (its rounding and the fp32 arithmetic bound) of itself, so |sum| <= 2 (2^-p + 5e-4)."""
    dev = _dev()
    kind = KINDS[dtype]
    c = _case(idx, kind)
    want_cost, want_grad = _reference(idx, kind)
    cost, grad = _gpu_call(c, dtype, dev)
    assert cost.dtype == torch.float32 and grad.dtype == dtype and grad.shape == c['x'].shape
    cost, grad = cost.cpu().double().numpy(), grad.cpu().double().numpy()
    ce, ge = _rel(cost, want_cost), _rel(grad, want_grad)
    print(SHAPES[idx], kind, 'cost %.3g gradient %.3g' % (ce, ge))
    assert np.isfinite(want_cost).all() and ce <= R.COST_BOUND, ce
    assert ge <= R.GRAD_BOUND[kind], ge
    act = _active(c)
    assert (grad[~act] == 0).all() and act.sum() < act.size
    p = {None: 24, 'bf16': 8, 'fp16': 11}[kind]
    assert np.abs(grad.sum(axis=-1)[act]).max() <= 2 * (2.0 ** -p + 5e-4)
    assert np.abs(grad).max() <= 1.0


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
def test_tiny_cases_match_the_enumeration(dtype):
    dev = _dev()
    kind = KINDS[dtype]
    for t, u, v in TINY:
        x, labels = _tiny(t, u, v)
        x = R.rnd(x, kind)
        c = dict(x=x, labels=labels, il=np.array([t], dtype=np.int32), ll=np.array([u], dtype=np.int32))
        cost, grad = _gpu_call(c, dtype, dev)
        want = R.enumerate_cost(x[0], labels[0])
        _, want_grad = R.rnnt(x, labels, [t], [u], grad_kind=kind)
        assert abs(float(cost[0]) - want) <= R.COST_BOUND * abs(want), (t, u, v)
        assert _rel(grad.cpu().double().numpy(), want_grad) <= R.GRAD_BOUND[kind], (t, u, v)


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
def test_infeasible_rows_and_padding_cells(dtype):
    """Tb = 0, a label == V - 1 and a negative label give +inf and an all-zero gradient; the feasible rows of the batch are bit-equal
    to the same rows in a batch of their own; NaN in every inactive cell changes no bit."""
    dev = _dev()
    rng = np.random.RandomState(17)
    v = 7
    x = R.rnd(rng.randn(5, 6, 5, v), KINDS[dtype])
    labels = np.array([[1, 2, 0, 3], [1, 1, 1, 1], [0, v - 1, 2, 2], [2, -1, 0, 0], [5, 0, 6, -3]])
    il, ll = np.array([6, 0, 5, 6, 4], dtype=np.int32), np.array([4, 2, 3, 2, 2], dtype=np.int32)
    c = dict(x=x, labels=labels, il=il, ll=ll)
    cost, grad = _gpu_call(c, dtype, dev)
    assert torch.isinf(cost[1:4]).all() and (cost[1:4] > 0).all() and torch.isfinite(cost[[0, 4]]).all()
    assert (grad[1:4] == 0).all() and float(grad[0].abs().max()) > 0 and float(grad[4].abs().max()) > 0
    keep = [0, 4]
    alone = dict(x=x[keep], labels=labels[keep], il=il[keep], ll=ll[keep])
    cost2, grad2 = _gpu_call(alone, dtype, dev)
    assert GA.first_bit_difference(cost[keep], cost2) is None and GA.first_bit_difference(grad[keep].contiguous(), grad2) is None
    want_cost, want_grad = R.rnnt(x, labels, il, ll, grad_kind=KINDS[dtype])
    assert _rel(cost2.cpu().double().numpy(), want_cost[keep]) <= R.COST_BOUND
    assert _rel(grad.cpu().double().numpy(), want_grad) <= R.GRAD_BOUND[KINDS[dtype]]
    noisy = x.copy()
    noisy[~_active(c)] = np.nan
    cost3, grad3 = _gpu_call(dict(c, x=noisy), dtype, dev)
    assert np.isnan(noisy).sum() > 0
    assert GA.first_bit_difference(cost3, cost) is None and GA.first_bit_difference(grad3, grad) is None


@pytest.mark.gpu
@pytest.mark.parametrize('dtype,idx', [(torch.bfloat16, 0), (torch.float32, 3)], ids=['bf16_one_wave', 'fp32_two_waves'])
def test_no_gradient_repeat_and_graph_replay_give_the_same_bits(dtype, idx):
    """grad = NULL (no requires_grad) gives the same cost; two calls agree; the call captures into a graph, and the replay after the
    logits buffer was refilled with the same values gives the same bits."""
    dev = _dev()
    c = _case(idx, KINDS[dtype])
    cost, grad = _gpu_call(c, dtype, dev)
    cost_only, _ = _gpu_call(c, dtype, dev, grad=False)
    assert GA.first_bit_difference(cost_only, cost) is None
    again = _gpu_call(c, dtype, dev)
    assert GA.first_bit_difference(again[0], cost) is None and GA.first_bit_difference(again[1], grad) is None
    x = torch.ones(c['x'].shape, dtype=dtype, device=dev)
    args = (torch.tensor(c['labels'], device=dev, dtype=torch.int32), torch.tensor(c['il'], device=dev), torch.tensor(c['ll'], device=dev))
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        F.rnnt_cost_and_grad(x, *args)                               # warm-up, eagerly (allocator, code objects)
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize(dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = F.rnnt_cost_and_grad(x, *args)
    for _ in range(2):
        x.copy_(torch.tensor(c['x'], dtype=dtype, device=dev))
        for o in outs:
            o.zero_()
        graph.replay()
        torch.cuda.synchronize(dev)
        assert GA.first_bit_difference(outs[0], cost) is None and GA.first_bit_difference(outs[1], grad) is None


@pytest.mark.gpu
@pytest.mark.parametrize('dtype,idx', [(torch.bfloat16, 0), (torch.float16, 5), (torch.float32, 3)], ids=['bf16', 'fp16_odd_rows', 'fp32_two_waves'])
def test_loss_keeps_to_its_buffers(monkeypatch, dtype, idx):
    """Under guard bands and the two fills: no write outside cost, grad or the workspace, every returned element written, and no
    returned bit depends on what the three buffers held."""
    dev = _dev()
    c = _case(idx, KINDS[dtype])

    def run(alloc):
        cost, grad = _gpu_call(c, dtype, dev)
        return dict(cost=cost, grad=grad)
    res = GA.run_twice(run, monkeypatch, modules=(F,))
    GA.assert_hygiene(res, 'rnnt %s %s: ' % (dtype, SHAPES[idx]))
    log = res.allocs[0].log
    assert {a.site.split(':')[0] for a in log} == {'functional.py'} and len(log) == 3          # cost, grad, workspace
    b, t, lmax, v = SHAPES[idx]
    ws = [a for a in log if a.dtype == torch.uint8]
    assert len(ws) == 1 and ws[0].nbytes == _lib.lib().qk_rnnt_workspace_bytes(b, t, lmax + 1, v)
    want_cost, want_grad = _reference(idx, KINDS[dtype])
    assert _rel(res.outputs[0]['grad'].cpu().double().numpy(), want_grad) <= R.GRAD_BOUND[KINDS[dtype]]


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', [torch.float32, torch.float16], ids=['fp32', 'fp16'])
def test_autograd_node_and_loss_scale(dtype):
    """rnnt_loss(...).mean().backward() is the stored gradient divided by B; loss_scale, a number or a device tensor, scales the
    gradient only (multiplied in fp32, rounded once)."""
    dev = _dev()
    c = _case(0, KINDS[dtype])
    cost, grad = _gpu_call(c, dtype, dev)
    args = (torch.tensor(c['labels'], device=dev), torch.tensor(c['il'], device=dev), torch.tensor(c['ll'], device=dev))
    x = torch.tensor(c['x'], dtype=dtype, device=dev, requires_grad=True)
    out = F.rnnt_loss(x, *args)
    assert out.shape == (3, 1) and GA.first_bit_difference(out.detach().reshape(-1), cost) is None
    out.mean().backward()
    third = torch.tensor(1.0 / 3.0, dtype=torch.float32, device=dev)
    want = grad * third.to(dtype)
    assert GA.first_bit_difference(x.grad, want) is None
    for scale in (256.0, torch.full((1,), 256.0, device=dev)):
        x.grad = None
        out = layers.rnnt_batch_cost(x, *args, loss_scale=scale)
        assert GA.first_bit_difference(out.detach().reshape(-1), cost) is None
        out.sum().backward()
        assert GA.first_bit_difference(x.grad, (grad.float() * 256.0).to(dtype)) is None
    with pytest.raises(ValueError):
        F.rnnt_loss(x, *args, loss_scale=0.0)
    with pytest.raises(RuntimeError):
        F.rnnt_loss(torch.zeros(1, 2, 130, 4, device=dev), torch.zeros(1, 129, dtype=torch.int32, device=dev), args[1][:1], args[2][:1])


# ---- the model --------------------------------------------------------------------------------------------------------------------------
def _small_model(dev, seed):
    """TimitQTransducer(TimitQLSTM(1, 64, one direction), pred_units 64, joint_units 64, no dropout) at B = 3, T = 12 with its batch."""
    np.random.seed(seed)
    torch.manual_seed(seed)
    model = TimitQTransducer(TimitQLSTM(1, 64, bidirectional=False, dropout=0.0), pred_units=64, joint_units=64, dropout=0.0)
    rng = np.random.RandomState(seed + 1)
    x = torch.tensor(rng.randn(3, 4, 41, 12).astype(np.float32), device=dev)
    labels = torch.tensor(rng.randint(0, 61, (3, 4)), device=dev, dtype=torch.int32)
    il = torch.tensor([[12], [7], [10]], dtype=torch.int32, device=dev)
    ll = torch.tensor([[4], [2], [0]], dtype=torch.int32, device=dev)
    with torch.no_grad():
        model(x, il)
    model.to(dev)
    return model, x, labels, il, ll


def _qdense_t(x, r, bias=None):
    out = x @ QR.expand_t(r)
    return out + bias if bias is not None else out


def _model_reference(model, x, labels, il, ll):
    """Mean transducer cost of the float64 composition of the same weights and its gradients, by parameter name: qlstm_ref's torch
    layers, an embedding lookup, the joint written out, and rnnt_ref for the cost and d cost / d logits."""
    p64 = {n: p.detach().double().cpu().requires_grad_() for n, p in model.named_parameters()}
    b, _, f, t = x.shape
    lengths, ub = il.reshape(-1).cpu(), ll.reshape(-1).cpu().long()
    o = x.double().cpu().permute(0, 3, 1, 2).reshape(b, t, 4 * f)
    enc = QR.layer_t(o, p64['encoder.rnn.0.kernel'], p64['encoder.rnn.0.recurrent_kernel'], p64['encoder.rnn.0.bias'], lengths)
    lab = labels.cpu().long()
    lab = torch.where(torch.arange(lab.shape[1])[None, :] < ub[:, None], lab, torch.full((), 61, dtype=torch.long))
    tokens = torch.cat([torch.full((b, 1), 61, dtype=torch.long), lab], dim=1)
    g = QR.layer_t(p64['embed.embeddings'][tokens], p64['pred_rnn.0.kernel'], p64['pred_rnn.0.recurrent_kernel'], p64['pred_rnn.0.bias'], ub + 1)
    fe = _qdense_t(enc.reshape(b * t, -1), p64['joint_enc.r'], p64['joint_enc.bias']).reshape(b, t, 1, -1)
    fp = _qdense_t(g.reshape(b * tokens.shape[1], -1), p64['joint_pred.r']).reshape(b, 1, tokens.shape[1], -1)
    logits = torch.tanh(fe + fp) @ p64['joint_out.kernel'] + p64['joint_out.bias']
    cost, grad = R.rnnt(logits.detach().numpy(), labels.cpu().numpy(), lengths.numpy(), ub.numpy())
    logits.backward(torch.tensor(grad) / b)
    return float(cost.mean()), {n: p.grad.numpy() for n, p in p64.items()}


@pytest.mark.gpu
def test_model_loss_and_gradients_match_the_float64_composition():
    """fp32: the mean transducer cost and all 12 parameter gradients within 1e-4 of the composition (the project's fp32 bound for a
    model step); the cost does not depend on what the padding frames and the padding labels hold."""
    dev = _dev()
    model, x, labels, il, ll = _small_model(dev, 31)
    cost = model.transducer_loss(x, labels, il, ll)
    assert cost.shape == (3, 1)
    loss = cost.mean()
    loss.backward()
    want_loss, want = _model_reference(model, x, labels, il, ll)
    errs = {n: _rel(p.grad.cpu().numpy(), want[n]) for n, p in model.named_parameters()}
    print(float(loss.detach()), want_loss, errs)
    assert len(errs) == 12 and all(float(np.abs(w).max()) > 0 for w in want.values())
    assert abs(float(loss.detach()) - want_loss) <= 1e-4 * abs(want_loss) and max(errs.values()) <= 1e-4, errs
    with torch.no_grad():
        noisy_x = x.clone()
        pad = torch.arange(12, device=dev)[None, :] >= il.reshape(-1, 1)
        noisy_x.permute(0, 3, 1, 2)[pad] = 37.0 * torch.randn(int(pad.sum()), 4, 41, device=dev)
        noisy_labels = labels.clone()
        lpad = torch.arange(4, device=dev)[None, :] >= ll.reshape(-1, 1)
        noisy_labels[lpad] = torch.tensor([99, -5, 61, 7, 1000, -1], dtype=torch.int32, device=dev)[:int(lpad.sum())]
        assert int(pad.sum()) > 0 and int(lpad.sum()) == 6
        assert GA.first_bit_difference(model.transducer_loss(noisy_x, noisy_labels, il, ll), cost.detach()) is None


@pytest.mark.gpu
def test_guarded_scheduled_steps_lower_the_loss_and_checkpoint(tmp_path):
    """dp.FlatParams, GradGuard, ScheduledAdam and save_checkpoint take the model's parameters as they are; bf16 activations."""
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
    path = str(tmp_path / 'qtransducer.pt')
    save_checkpoint(path, model, opt)
    saved = torch.load(path, map_location='cpu', weights_only=True)
    assert {'encoder.rnn.0.kernel', 'embed.embeddings', 'pred_rnn.0.recurrent_kernel', 'joint_pred.r', 'joint_out.bias'} <= set(saved['model'])
    before = flat.param.clone()
    flat.param.zero_()
    load_checkpoint(path, model, opt)
    assert torch.equal(flat.param, before)


def _host_decode(model, x, il, max_symbols):
    """The decode as a host-controlled loop over the same modules on the same batch: per-row Python lists, a host decision per symbol.
    Returns (symbols per row, log-probability per row, frames per row that max_symbols ended instead of a blank, and the sum of the
    blank log-probabilities at those forced advances: what the row's log-probability lacks to be that of a complete alignment)."""
    b, t_max = x.shape[0], x.shape[3]
    lens = [int(v) for v in il.reshape(-1).cpu()]
    was = model.training
    model.eval()
    with torch.no_grad():
        enc = model.encoder.features(x, il)
        fe = model.joint_enc(enc.reshape(b * t_max, -1)).view(b, t_max, -1)
        g, state = model.predict_step(torch.full((b,), 61, dtype=torch.long, device=x.device), dtype=enc.dtype)
        hyps, logp, capped, missing = [[] for _ in range(b)], [0.0] * b, [0] * b, [0.0] * b
        for t in range(t_max):
            live = [t < n for n in lens]
            for _ in range(max_symbols):
                if not any(live):
                    break
                lsm = model.joint_step(fe[:, t], g).cpu().numpy()
                sym = [int(np.argmax(row)) for row in lsm]                     # numpy: the first maximum
                emit = [live[i] and sym[i] != 61 for i in range(b)]
                for i in range(b):
                    if live[i]:
                        logp[i] += float(lsm[i, sym[i]])
                    if emit[i]:
                        hyps[i].append(sym[i])
                g2, state2 = model.predict_step(torch.tensor([s if e else 61 for s, e in zip(sym, emit)], device=x.device), state)
                mask = torch.tensor(emit, device=x.device)
                g = torch.where(mask[:, None], g2, g)
                state = [(torch.where(mask[:, None], h2, h), torch.where(mask[:, None], c2, c)) for (h, c), (h2, c2) in zip(state, state2)]
                live = emit
            if any(live):                                                      # frames ended by max_symbols, not by a blank
                lsm = model.joint_step(fe[:, t], g).cpu().numpy()
                for i in range(b):
                    if live[i]:
                        capped[i] += 1
                        missing[i] += float(lsm[i, 61])
    model.train(was)
    return hyps, logp, capped, missing


@pytest.mark.gpu
def test_greedy_decode_matches_a_host_loop_and_scores():
    """decode() equals the host-controlled loop; max_symbols = 1 never emits more than Tb symbols; one path cannot outweigh the sum
    over all paths: log_prob <= -transducer_loss(decoded) (1e-4 relative slack for the fp32 summation order) for a row whose frames
    all ended with a drawn blank.  A frame that max_symbols ended advances WITHOUT a blank factor, so there log_prob is no alignment's
    probability (a random model that emits once at a frame emits there until the limit: measured -48.1 against -66.6); for such a
    row the blank log-probabilities at the forced advances are added first, which makes the path a complete alignment of the decode
    and the comparison the same statement."""
    dev = _dev()
    model, x, labels, il, ll = _small_model(dev, 53)
    with torch.no_grad():
        # lift blank above the largest other logit in 70 % of the frames of a random model (first draw of a frame)
        start = model(x, il)[:, :, 0, :].float()
        gap = (start[..., :61].max(dim=-1).values - start[..., 61]).reshape(-1)
        model.joint_out.bias[61] += float(torch.quantile(gap, 0.7))
    lens = [int(v) for v in il.reshape(-1).cpu()]
    complete = 0
    for max_symbols in (1, 3, 8):
        (decoded,), log_prob = model.decode(x, il, max_symbols=max_symbols)
        hyps, logp, capped, missing = _host_decode(model, x, il, max_symbols)
        assert decoded.dtype == torch.int64 and decoded.shape == (3, max(len(h) for h in hyps)) and log_prob.shape == (3, 1)
        rows = [[int(v) for v in row if v >= 0] for row in decoded.cpu()]
        assert rows == hyps and all((row[len(h):] == -1).all() for row, h in zip(decoded.cpu(), hyps))
        assert np.abs(log_prob.cpu().numpy().reshape(-1) - np.array(logp)).max() <= 1e-5 * np.abs(logp).max()
        assert all(len(h) <= max_symbols * n for h, n in zip(hyps, lens))
        print(max_symbols, [len(h) for h in hyps], capped, logp, missing)
        dlen = (decoded >= 0).sum(dim=1).to(torch.int32)
        with torch.no_grad():
            was = model.training
            model.eval()
            total = -model.transducer_loss(x, decoded.clamp(min=0).to(torch.int32), il, dlen).reshape(-1)
            model.train(was)
        for i in range(3):
            assert (capped[i] == 0) == (missing[i] == 0.0) and missing[i] <= 0.0
            complete += int(len(hyps[i]) > 0)
            path = float(log_prob[i]) + missing[i]
            assert path <= float(total[i]) + 1e-4 * abs(float(total[i])), (max_symbols, i, float(log_prob[i]), missing[i], float(total[i]))
    assert complete > 0 and sum(len(h) for h in hyps) > 0          # non-empty decodes were compared
    res = model.evaluate(x, labels, il, ll, max_symbols=3)
    (decoded,), log_prob = model.decode(x, il, max_symbols=3)
    errors, symbols, per = layers.label_error_rate(decoded, None, labels, ll)
    assert torch.equal(res.decoded, decoded) and torch.equal(res.log_prob, log_prob)
    assert int(res.errors) == int(errors) and int(res.symbols) == int(symbols) == 6 and float(res.per) == float(per)
    with torch.no_grad():
        model.eval()
        assert float(res.loss) == float(model.transducer_loss(x, labels, il, ll).mean())
        model.train()
    assert model.training
