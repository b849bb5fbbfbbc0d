"""The sequence kernels where their loops take a second pass: the quaternion LSTM (include/qk_rnn.h), layer normalisation
(include/qk_norm.h) and the depthwise / GLU convolution (include/qk_dwconv.h) at the widths, row counts and batches at which the
loops of csrc/qk_qlstm.hip, qk_qlnorm.hip and qk_qdwconv.hip run more than once, against the float64 references of
tests/qlstm_ref.py, qlnorm_ref.py and qdwconv_ref.py.  The per-layer suites (test_qlstm.py, test_qlnorm.py, test_qdwconv.py) keep
the tile edges along time and the lengths; their shapes leave the loops below at zero or one trip.

Bounds (relative to max|want| per tensor), the project's own: fp32 1e-4 against the float64 reference; bf16 / fp16 against the
reference WITH the header's rounding points, 16-bit outputs 1e-2 / 2e-3, fp32 outputs of the 16-bit paths 2e-3 / 1e-3.  The
test_*_rounding_points_* tests show on the very inputs of the GPU tests that the rounding points alone move the float64 result
by at most HALF of 1e-2 / 2e-3 and by more than 1e-5.

Which case guards which loop (trip counts per wave / thread with today's constants):

  loop                                                   case                                   trips
  -----------------------------------------------------  -------------------------------------  ------------------------------------
  qk_qlstm.hip k_ql_fwd16  for (ks = wave; ks < nk;      test_lstm_wide_rows  Q = 144           nk = 5: wave 0 two trips, the second
                                ks += 4)                                                        the half-empty K step (kv false);
                                                                                                image offset (ks*16+f)*64 at ks = 4
                                                         test_lstm_wide_rows  Q = 160           nk = 5: wave 0 two full trips
  qk_qlstm.hip k_ql_bwd16  for (j0 = 32*wave; j0 < U;    test_lstm_wide_rows  Q = 144, U = 576  three passes; the third by waves 0, 1
                                j0 += 256), h = 0, 1                                            only, its h = 1 half empty
                                                         test_lstm_wide_rows  Q = 160, U = 640  three passes by all waves; the third
                                                                                                with an empty h = 1 half
  qk_qlstm.hip generic     for k < Q, for j < U          test_lstm_wide_rows  fp32              144 / 160 and 576 / 640 trips
  dense backward-weight behind dR (140 x 576 / 640)      test_lstm_wide_rows                    the dense path is printed and named
  qk_qlstm.hip host loop   for (s = 0; s < T; ++s)       test_lstm_long_walk  T = 40            the two h buffers alternate 20 times
                                                         test_lstm_degenerate_extents  T = 1    one launch: h_in = h0, h_out = hT,
                                                                                                c_in = c0; backward s = 0, then tail
  row tile of 16, min(row0 + l16, B - 1)                 test_lstm_degenerate_extents  B = 1,   a tile with ONE valid row: fifteen
                                                         B = 17                                 lanes re-read row B - 1
  ql_sigmoid / tanhf / expf overflow                     test_lstm_saturated_gates              |z| > 100: expf(-z) = inf
  inactive (b, t): zx / dy never read                    test_lstm_nan_in_the_padding_...       NaN there changes no bit
  desc.y_stride > D U                                    test_lstm_y_stride_windows             y / dy windows of wider buffers
  qk_qlnorm.hip qn_slab_rows > 16, k_qln_bwd             test_lnorm_many_rows  15 400 rows      slab_rows = 24: six trips per wave;
      for (row = r0 + wave; row < r1; row += 4)                                                 the last slab has 16 rows: four
  qk_qlnorm.hip k_qln_reduce  for (; s + 4 <= s1;        test_lnorm_many_rows, test_lnorm_      642 slabs.  W = 4 (q = 8): per = 11,
      s += 4) and its tail  for (; s < s1; ++s)          exact_bias_gradient                    two unrolled trips + three tail; run
                                                                                                58 holds 4 slabs, runs 59 .. 63 none.
                                                                                                W = 1 (q = 5): per = 41, ten unrolled
                                                                                                + one tail; run 15 holds 27
  qk_qlnorm.hip forward / generic backward               test_lnorm_many_rows                   15 400 rows > 4 * 1024 (vector: four
      row += gridDim.x * 4                                                                      passes) and > 4 * 2048 (generic: two)
  qk_qlnorm.hip k_qln_part_gen  for (row = r0; ..)       test_lnorm_many_rows  q = 5            24 rows per slab
  qk_qdwconv.hip dw_slab_rows >= 2, k_dw_wgrad /         test_dwconv_multi_row_slabs,           B = 130: 65 slabs of 2 rows, slab 0 =
      k_dw_part_gen  for (b = b0; b < b1; ++b)           test_dwconv_lattice_at_those_batches   (empty, full), slab 1 empty.  B = 257:
                                                                                                86 slabs of 3, the last of 2; slab 1
                                                                                                empty
  qk_qdwconv.hip KB buckets 3 / 7 / 15 / 31,             test_dwconv_tap_counts_inside_...      K = 4, 5, 7 in KB = 7 (7: the full
      guards j - f < K, pad_lo = (K - 1) / 2                                                    bucket in bf16 / fp16), 9 causal in
                                                                                                KB = 15, 17 in KB = 31; K = 4: the
                                                                                                asymmetric 'same'

Not here: the attention kernels (tests/test_qattn.py drives every tile loop to three trips at T = 150; the grid caps of 2^20
workgroups cannot be reached at a test-sized shape).
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import guarded_alloc as GA
import lattice_ref as LAT
import qdwconv_ref as DR
import qlnorm_ref as NR
import qlstm_ref as LR
from qcnn_amd import _lib, functional as F

KINDS = {torch.float32: None, torch.bfloat16: 'bf16', torch.float16: 'fp16'}
DTYPES = {None: torch.float32, 'bf16': torch.bfloat16, 'fp16': torch.float16}
DTYPE_IDS = ['fp32', 'bf16', 'fp16']
BOUND_16 = {'bf16': 1e-2, 'fp16': 2e-3}          # 16-bit outputs
BOUND_32 = {'bf16': 2e-3, 'fp16': 1e-3}          # fp32 outputs of the 16-bit paths
EPS = 1e-3


def _dev():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    return torch.device('cuda:0')


def _rel(got, want):
    return float(np.abs(np.asarray(got, dtype=np.float64) - want).max()) / max(float(np.abs(want).max()), 1e-30)


def _f32(a):
    return a.astype(np.float32).astype(np.float64)


def _freeze(d):
    for v in d.values():
        v.setflags(write=False)
    return d


def _check(got, want, dtype, out32, what=''):
    """Every tensor of `got` against `want` at the project's bounds; dtypes and shapes too."""
    kind = KINDS[dtype]
    errs = {}
    for name, g in got.items():
        assert g.dtype == (torch.float32 if name in out32 else dtype) and tuple(g.shape) == want[name].shape, name
        assert bool(torch.isfinite(g).all()), name
        errs[name] = (_rel(g.float().cpu().numpy(), want[name]), 1e-4 if kind is None else BOUND_32[kind] if name in out32 else BOUND_16[kind])
    print(what, errs)
    assert all(e <= b for e, b in errs.values()), errs


def _budget(rounded, pure, kind, names16, names32, exact32, what):
    """The rounding points alone: at most half the 16-bit bound on every output, in play (> 1e-5) on the 16-bit outputs; the fp32
    outputs either move too (exact32 False) or are sums of the inputs alone and do not move at all."""
    errs = {name: _rel(rounded[name], pure[name]) for name in names16 + names32}
    print(what, kind, errs)
    assert max(errs.values()) <= 0.5 * BOUND_16[kind], errs
    assert min(errs[name] for name in names16) > 1e-5, errs
    if exact32:
        assert max(errs[name] for name in names32) == 0, errs
    return errs


# ==== A. the LSTM recurrence =======================================================================================================
L_OUT_16, L_OUT_32 = ('y', 'hT', 'dzx', 'dh0'), ('dR', 'dc0', 'cT')
# a case: (q_units, directions, batch, steps, lengths mode, scale of zx)
L_WIDE = {144: (144, 2, 20, 7, 'mixed', 1.0), 160: (160, 2, 20, 7, 'mixed', 1.0)}
L_LONG = (16, 2, 20, 40, 'mixed', 1.0)
L_DEGENERATE = {'t1_mfma16': (torch.bfloat16, (16, 2, 20, 1, 'mixed', 1.0)), 't1_generic': (torch.float32, (5, 2, 20, 1, 'mixed', 1.0)),
                'b1_full': (torch.bfloat16, (48, 2, 1, 7, 'full', 1.0)), 'b17_full': (torch.bfloat16, (48, 2, 17, 7, 'full', 1.0)),
                'b17_zero_full_random': (torch.bfloat16, (48, 2, 17, 7, 'zero_full', 1.0))}
L_SATURATED = (16, 2, 20, 7, 'mixed', 40.0)
L_POISON = {'mfma16_bf16_one_direction': (torch.bfloat16, (16, 1, 20, 7, 'mixed', 1.0)), 'mfma16_fp16_two_directions': (torch.float16, (48, 2, 20, 7, 'mixed', 1.0)),
            'generic_fp32_two_directions': (torch.float32, (5, 2, 20, 7, 'mixed', 1.0))}
L_STRIDE = {'mfma16': (torch.bfloat16, (16, 2, 20, 7, 'mixed', 1.0), 152, 8), 'generic': (torch.float32, (5, 2, 20, 7, 'mixed', 1.0), 47, 4)}


def _lstm_lengths(bsz, steps, mode, seed):
    """mixed: 0, 1, steps - 2 and steps (T = 1: 0, 1, 0, 1) in front, the rest random; full: every row steps; zero_full: 0, steps,
    the rest random with a last row that is not empty."""
    rng = np.random.RandomState(seed)
    out = rng.randint(0, steps + 1, size=bsz)
    if mode == 'full':
        out[:] = steps
    elif mode == 'zero_full':
        out[:2] = [0, steps]
        out[-1] = max(1, steps - 1)
    else:
        fixed = [0, 1, max(steps - 2, 0), steps]
        out[:min(bsz, 4)] = fixed[:min(bsz, 4)]
    return out.astype(np.int32)


@functools.lru_cache(maxsize=None)
def _lstm_inputs(case, kind):
    """Seeded operands (never written), 16-bit ones already rounded to `kind`, drawn as tests/test_qlstm.py draws them: the recurrent
    term is of the order of zx.  `scale` multiplies zx before it is rounded."""
    q, dirs, bsz, steps, mode, scale = case
    rng = np.random.RandomState(5000 + 16 * q + dirs + 101 * bsz + 7 * steps + 1009 * ('mixed', 'full', 'zero_full').index(mode))
    u = 4 * q
    d = dict(zx=LR.rnd(scale * rng.randn(dirs, bsz, steps, 4 * u), kind), R=_f32((0.6 / np.sqrt(q)) * rng.randn(dirs, q, 4 * u)),
             h0=LR.rnd(0.5 * rng.randn(dirs, bsz, u), kind), c0=_f32(rng.randn(dirs, bsz, u)), dy=LR.rnd(rng.randn(bsz, steps, dirs * u), kind),
             dhT=LR.rnd(rng.randn(dirs, bsz, u), kind), dcT=_f32(rng.randn(dirs, bsz, u)), lengths=_lstm_lengths(bsz, steps, mode, q + steps))
    return _freeze(d)


@functools.lru_cache(maxsize=None)
def _lstm_reference(case, kind, rounded=True):
    """The reference's outputs for _lstm_inputs(case, kind), computed once and shared; rounded False: without the rounding points."""
    i = _lstm_inputs(case, kind)
    # what numpy would warn of is an error here: the float64 reference stays warning-free, the saturated case included
    with np.errstate(over='raise', invalid='raise', divide='raise'):
        return LR.qlstm(i['zx'], i['R'], i['lengths'], i['h0'], i['c0'], kind=kind if rounded else None, dy=i['dy'], dhT=i['dhT'], dcT=i['dcT'])


def _lstm_inactive(case, kind):
    steps = case[3]
    return np.arange(steps)[None, :] >= _lstm_inputs(case, kind)['lengths'][:, None]


# ---- CPU part ---------------------------------------------------------------------------------------------------------------------
L_BUDGET = [('wide_144', L_WIDE[144]), ('wide_160', L_WIDE[160]), ('long_walk', L_LONG), ('saturated', L_SATURATED)] \
    + [(name, case) for name, (dtype, case) in L_DEGENERATE.items() if KINDS[dtype]] \
    + [('poison_' + name, case) for name, (dtype, case) in L_POISON.items() if KINDS[dtype]]


@pytest.mark.parametrize('kind', ['bf16', 'fp16'])
@pytest.mark.parametrize('name,case', L_BUDGET, ids=[n for n, _ in L_BUDGET])
def test_lstm_rounding_points_move_the_reference_by_at_most_half_the_16_bit_bound(name, case, kind):
    """Every LSTM input family of this module, the 40-step walk and the saturated gates included.  Measured, the largest shift of
    any output over the cases: 3.7e-3 (bf16; dR at Q = 144) / 4.6e-4 (fp16; dzx at T = 1); the 40-step walk 2.7e-3 / 3.3e-4; the
    saturated gates 4.5e-3 / 4.2e-4 (dzx).  Half the bounds is 5e-3 / 1e-3."""
    errs = _budget(_lstm_reference(case, kind), _lstm_reference(case, kind, rounded=False), kind, ('y', 'dzx'), ('hT', 'dh0') + L_OUT_32, False, name)
    assert errs['dR'] > 1e-5, errs


def test_lstm_cases_are_what_the_audit_table_says():
    """The shapes drive the loops as the module's table claims, and the inputs have the properties the cases rest on."""
    for q, passes, last_waves in ((144, 3, 2), (160, 3, 4)):
        u = 4 * q
        assert (q + 31) // 32 == 5 and u % 64 == 0                      # nk = 5: wave 0 takes K steps 0 and 4
        assert len(range(0, u, 256)) == passes and sum(1 for w in range(4) if 512 + 32 * w < u) == last_waves
        assert all(512 + 32 * w + 128 >= u for w in range(4))            # the third pass has no h = 1 half
        assert list(_lstm_inputs(L_WIDE[q], None)['lengths'][:4]) == [0, 1, 5, 7]
    assert 144 % 32 == 16 and 160 % 32 == 0                              # the second K step of Q = 144 is the half-empty one
    for kind in (None, 'bf16'):
        i = _lstm_inputs(L_SATURATED, kind)
        assert float(np.abs(i['zx']).max()) > 100
        o = _lstm_reference(L_SATURATED, kind)
        assert all(np.isfinite(v).all() for v in o.values()) and float(np.abs(o['dzx']).max()) > 1e-3
    assert list(_lstm_inputs(L_DEGENERATE['t1_mfma16'][1], 'bf16')['lengths'][:4]) == [0, 1, 0, 1]
    ln = _lstm_inputs(L_DEGENERATE['b17_zero_full_random'][1], 'bf16')['lengths']
    assert list(ln[:2]) == [0, 7] and ln[16] >= 1 and list(_lstm_inputs(L_DEGENERATE['b1_full'][1], 'bf16')['lengths']) == [7]
    for dtype, case, width, off in L_STRIDE.values():
        es = 4 if dtype == torch.float32 else 2
        assert (off * es) % 16 == 0 and off > 0 and width > off + case[1] * 4 * case[0]      # a 16-byte aligned base, columns on both sides


# ---- GPU part ---------------------------------------------------------------------------------------------------------------------
def _lstm_run(dev, dtype, case, ops=None):
    """functional.qlstm forward and backward on _lstm_inputs(case) (or on `ops`), every optional input given: name -> tensor."""
    i = ops if ops is not None else _lstm_inputs(case, KINDS[dtype])
    t = lambda a, dt=dtype: torch.tensor(np.asarray(a), dtype=dt, device=dev)
    zx, Rw = t(i['zx']).requires_grad_(), t(i['R'], torch.float32).requires_grad_()
    h0, c0 = t(i['h0']).requires_grad_(), t(i['c0'], torch.float32).requires_grad_()
    with _lib.debug_flags(_lib.QK_DBG_DETERMINISTIC):
        y, hT, cT = F.qlstm(zx, Rw, torch.tensor(i['lengths'], device=dev), h0, c0)
        torch.autograd.backward([y, hT, cT], [t(i['dy']), t(i['dhT']), t(i['dcT'], torch.float32)])
    return dict(y=y.detach(), hT=hT.detach(), cT=cT.detach(), dzx=zx.grad, dR=Rw.grad, dh0=h0.grad, dc0=c0.grad)


def _lstm_check(dev, dtype, case, got, what):
    """Parity on the seven tensors; asserted, not tolerated: exact zeros at inactive positions, and a row of length 0 returns its
    initial state and its incoming state gradients bit for bit."""
    kind = KINDS[dtype]
    _check(got, _lstm_reference(case, kind), dtype, L_OUT_32, what)
    i = _lstm_inputs(case, kind)
    off = _lstm_inactive(case, kind)
    if off.any():
        mask = torch.tensor(off, device=dev)
        assert int(got['y'][mask].ne(0).sum()) == 0 and int(got['dzx'][:, mask].ne(0).sum()) == 0
    for b in np.flatnonzero(i['lengths'] == 0):
        for name, src, dt in (('hT', 'h0', dtype), ('cT', 'c0', torch.float32), ('dh0', 'dhT', dtype), ('dc0', 'dcT', torch.float32)):
            init = torch.tensor(i[src][:, b], dtype=dt, device=dev)
            assert GA.first_bit_difference(got[name][:, b].contiguous(), init) is None, (name, b)


@pytest.mark.gpu
@pytest.mark.parametrize('q', [144, 160])
@pytest.mark.parametrize('dtype', list(KINDS), ids=DTYPE_IDS)
def test_lstm_wide_rows(dtype, q):
    """Q = 144 / 160, B = 20, T = 7, two directions, every state input: a second (Q = 144: half-empty) K step in the forward, three
    passes in the backward.  dR comes from the dense backward-weight at 140 x 576 / 640 rows: the path that served it is printed and
    must be one of the dense kernels."""
    dev = _dev()
    case = L_WIDE[q]
    assert F.qlstm_path(dtype, case[2], case[3], q, 2) == ('mfma16' if KINDS[dtype] else 'generic')
    with _lib.profile() as p:                            # (qk_last_path is per thread, and the backward runs on autograd's)
        got = _lstm_run(dev, dtype, case)
        torch.cuda.synchronize(dev)
        dense = [r for r in p.records() if r['op'] == 'bwd_weight']
    print('dense backward-weight calls behind dR:', dense)
    _lstm_check(dev, dtype, case, got, 'wide rows q=%d' % q)
    # recorded, not prescribed (today the 16-bit call runs 'mfma16' at U = 640 and 'fp32_mfma' at U = 576): one call per direction over
    # the B T stacked rows, served by a kernel; fp32 by the fp32 one
    assert len(dense) == 2 and all((r['rows'], r['n'], r['k']) == (case[2] * case[3], 16 * q, 4 * q) for r in dense), dense
    assert all(r['path'] in ('mfma16', 'mfma16_small', 'fp32_mfma') for r in dense) and (dtype != torch.float32 or dense[0]['path'] == 'fp32_mfma'), dense


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['fp32', 'bf16'])
def test_lstm_long_walk(dtype):
    """Q = 16, B = 20, T = 40: the two h buffers alternate 20 times and the rounding points compound over 40 steps."""
    dev = _dev()
    _lstm_check(dev, dtype, L_LONG, _lstm_run(dev, dtype, L_LONG), 'long walk')


@pytest.mark.gpu
@pytest.mark.parametrize('name', list(L_DEGENERATE))
def test_lstm_degenerate_extents(name):
    """T = 1 (one forward launch from h0 / c0 straight into hT / cT; a backward of s = 0 and the tail launch) on both kernel families;
    B = 1 and B = 17 (a row tile with one valid row) on the matrix-core kernels."""
    dev = _dev()
    dtype, case = L_DEGENERATE[name]
    assert F.qlstm_path(dtype, case[2], case[3], case[0], 2) == ('mfma16' if KINDS[dtype] else 'generic')
    _lstm_check(dev, dtype, case, _lstm_run(dev, dtype, case), name)


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['fp32', 'bf16'])
def test_lstm_saturated_gates(dtype):
    """zx scaled by 40 (max |zx| > 100: expf(-z) overflows fp32 on one side): every output finite and inside the bounds."""
    dev = _dev()
    assert float(np.abs(_lstm_inputs(L_SATURATED, KINDS[dtype])['zx']).max()) > 100
    _lstm_check(dev, dtype, L_SATURATED, _lstm_run(dev, dtype, L_SATURATED), 'saturated')


@pytest.mark.gpu
@pytest.mark.parametrize('name', list(L_POISON))
def test_lstm_nan_in_the_padding_frames_changes_no_bit(name):
    """NaN in zx and dy at every (b, t >= lengths[b]): all seven outputs are finite and bit-identical to the run with zeros there."""
    dev = _dev()
    dtype, case = L_POISON[name]
    i = _lstm_inputs(case, KINDS[dtype])
    off = _lstm_inactive(case, KINDS[dtype])
    assert off.sum() > case[3]
    runs = []
    for fill in (0.0, np.nan):
        ops = dict(i, zx=np.where(off[None, :, :, None], fill, i['zx']), dy=np.where(off[:, :, None], fill, i['dy']))
        runs.append(_lstm_run(dev, dtype, case, ops))
    for name_ in runs[0]:
        assert bool(torch.isfinite(runs[1][name_]).all()), name_
        assert GA.first_bit_difference(runs[0][name_], runs[1][name_]) is None, name_
    _check(runs[1], _lstm_reference(case, KINDS[dtype]), dtype, L_OUT_32, 'poisoned ' + name)


def _lstm_raw_call(dev, dtype, case, width, off):
    """qk_qlstm_fwd / _bwd through ctypes: y and dy are column windows [off, off + D U) of (B, T, width) buffers prefilled with 5 and
    7.  Returns name -> tensor (y: the window) and the two wide buffers."""
    lib = _lib.lib()
    q, dirs, bsz, steps = case[:4]
    u = 4 * q
    i = _lstm_inputs(case, KINDS[dtype])
    t = lambda a, dt=dtype: torch.tensor(np.asarray(a), dtype=dt, device=dev)
    zx, Rw, h0, c0, ln = t(i['zx']), t(i['R'], torch.float32), t(i['h0']), t(i['c0'], torch.float32), torch.tensor(i['lengths'], device=dev)
    dhT, dcT = t(i['dhT']), t(i['dcT'], torch.float32)
    yb = torch.full((bsz, steps, width), 5.0, dtype=dtype, device=dev)
    dyb = torch.full((bsz, steps, width), 7.0, dtype=dtype, device=dev)
    dyb[:, :, off:off + dirs * u] = t(i['dy'])
    empty = lambda shape, dt=dtype: torch.empty(shape, dtype=dt, device=dev)
    hT, cT = empty((dirs, bsz, u)), empty((dirs, bsz, u), torch.float32)
    dzx, hprev = empty((dirs, bsz, steps, 4 * u)), empty((dirs, bsz, steps, u))
    dh0, dc0 = empty((dirs, bsz, u)), empty((dirs, bsz, u), torch.float32)
    desc = F.qlstm_desc(dtype, bsz, steps, q, dirs)
    desc.y_stride = width
    assert lib.qk_qlstm_supported(ctypes.byref(desc)) == (_lib.QK_QLSTM_PATH_MFMA16 if KINDS[dtype] and q % 16 == 0 else _lib.QK_QLSTM_PATH_GENERIC)
    nf = int(lib.qk_qlstm_workspace_bytes(ctypes.byref(desc), _lib.QK_OP_FWD))
    nb = int(lib.qk_qlstm_workspace_bytes(ctypes.byref(desc), _lib.QK_OP_BWD))
    nr = int(lib.qk_qlstm_reserve_bytes(ctypes.byref(desc)))
    assert nf > 0 and nb > 0 and nr > 0
    wsf, wsb, reserve = empty(nf, torch.uint8), empty(nb, torch.uint8), empty(nr, torch.uint8)
    es = yb.element_size()
    y_ptr, dy_ptr = yb.data_ptr() + off * es, dyb.data_ptr() + off * es
    assert y_ptr % 16 == 0 and dy_ptr % 16 == 0
    stream = torch.cuda.current_stream(dev).cuda_stream
    with torch.cuda.device(dev):
        _lib.check(lib.qk_qlstm_fwd(ctypes.byref(desc), zx.data_ptr(), Rw.data_ptr(), ln.data_ptr(), h0.data_ptr(), c0.data_ptr(), y_ptr,
                                    hT.data_ptr(), cT.data_ptr(), reserve.data_ptr(), wsf.data_ptr(), nf, stream), 'qk_qlstm_fwd')
        _lib.check(lib.qk_qlstm_bwd(ctypes.byref(desc), dy_ptr, dhT.data_ptr(), dcT.data_ptr(), Rw.data_ptr(), ln.data_ptr(), h0.data_ptr(),
                                    c0.data_ptr(), y_ptr, reserve.data_ptr(), dzx.data_ptr(), hprev.data_ptr(), dh0.data_ptr(), dc0.data_ptr(),
                                    wsb.data_ptr(), nb, stream), 'qk_qlstm_bwd')
    torch.cuda.synchronize(dev)
    out = dict(y=yb[:, :, off:off + dirs * u].contiguous(), hT=hT, cT=cT, dzx=dzx, hprev=hprev, dh0=dh0, dc0=dc0)
    return out, yb, dyb


@pytest.mark.gpu
@pytest.mark.parametrize('name', list(L_STRIDE))
def test_lstm_y_stride_windows_equal_the_dense_call_and_leave_the_other_columns_alone(name):
    """desc.y_stride > D U: y is written into, and y / dy are read from, column windows of wider buffers.  Every result is bit-equal
    to the dense call's (which itself keeps the parity bounds), and every column outside the windows keeps its fill."""
    dev = _dev()
    dtype, case, width, off = L_STRIDE[name]
    du = case[1] * 4 * case[0]
    dense, _, _ = _lstm_raw_call(dev, dtype, case, du, 0)
    want = _lstm_reference(case, KINDS[dtype])
    _check({k: v for k, v in dense.items() if k != 'hprev'}, want, dtype, L_OUT_32, 'dense raw call ' + name)
    assert _rel(dense['hprev'].float().cpu().numpy(), want['hprev']) <= (BOUND_16[KINDS[dtype]] if KINDS[dtype] else 1e-4)
    got, yb, dyb = _lstm_raw_call(dev, dtype, case, width, off)
    for key in dense:
        assert GA.first_bit_difference(got[key], dense[key]) is None, key
    keep = lambda buf: torch.cat([buf[:, :, :off], buf[:, :, off + du:]], dim=2)
    assert keep(yb).numel() > 0 and bool((keep(yb) == 5.0).all()) and bool((keep(dyb) == 7.0).all())


# ==== B. layer normalisation =======================================================================================================
N_OUT_16, N_OUT_32 = ('y', 'dx'), ('dgamma', 'dbeta')
NB, NT, N_QS = 2200, 7, (8, 5)                   # 15 400 rows; 8: the vector kernels, 5: the generic ones


def _norm_path(dtype, q):
    return 'vec' if q % (4 if dtype == torch.float32 else 8) == 0 else 'generic'


@functools.lru_cache(maxsize=None)
def _norm_inputs(q, kind, lattice=False):
    """Seeded operands (never written) drawn as tests/test_qlnorm.py draws them; lattice: dy from {-1, 0, 1}."""
    rng = np.random.RandomState(6000 + q)
    x = NR.rnd(_f32(1.5 * rng.randn(NB, NT, 4 * q) + rng.randn(4 * q)), kind)
    gamma, beta = _f32(1 + 0.3 * rng.randn(q)), _f32(0.3 * rng.randn(4 * q))
    dy = NR.rnd(_f32(rng.randn(NB, NT, 4 * q)), kind)
    lengths = rng.randint(0, NT + 1, size=NB).astype(np.int32)
    lengths[:4] = [0, 1, NT - 2, NT]
    if lattice:
        dy = LAT.integer_lattice(np.random.RandomState(6100 + q), (NB, NT, 4 * q)).astype(np.float64)
    return _freeze(dict(x=x, gamma=gamma, beta=beta, dy=dy, lengths=lengths))


@functools.lru_cache(maxsize=None)
def _norm_reference(q, kind, rounded=True):
    i = _norm_inputs(q, kind)
    return NR.qlayer_norm(i['x'], i['gamma'], i['beta'], i['lengths'], epsilon=EPS, kind=kind if rounded else None, dy=i['dy'])


@functools.lru_cache(maxsize=None)
def _norm_exact_dbeta(q, kind):
    """The plain float64 sum of the lattice dy over the active rows."""
    i = _norm_inputs(q, kind, lattice=True)
    act = NR.active_rows(i['dy'].shape, i['lengths'])
    return i['dy'].reshape(NB * NT, 4 * q)[act].sum(axis=0)


# ---- CPU part ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['bf16', 'fp16'])
@pytest.mark.parametrize('q', N_QS)
def test_lnorm_rounding_points_move_the_reference_by_at_most_half_the_16_bit_bound(q, kind):
    """15 400 rows: the two rounding points move y and dx by at most 3.3e-3 (bf16) / 4.5e-4 (fp16) (measured) and leave dgamma and
    dbeta, sums of the inputs alone, exactly where they are."""
    _budget(_norm_reference(q, kind), _norm_reference(q, kind, rounded=False), kind, N_OUT_16, N_OUT_32, True, 'lnorm q=%d' % q)


@pytest.mark.parametrize('q', N_QS)
@pytest.mark.parametrize('dtype', list(KINDS), ids=DTYPE_IDS)
def test_lnorm_geometry_of_the_many_rows_case(dtype, q):
    """Through the host-only entry points: the case cannot be emptied silently by a later change of the slab constants.  Conditions,
    not numbers (today: slab_rows 24, 642 slabs, a last slab of 16 rows)."""
    lib = _lib.lib()
    rows = NB * NT
    desc = F.qlayer_norm_desc(dtype, rows, q, steps=NT)
    slab = lib.qk_qlnorm_slab_rows(ctypes.byref(desc))
    assert slab > 16 and rows % slab != 0                               # more than the minimum; a ragged last slab
    assert slab // 4 >= 5 and 0 < (rows % slab + 3) // 4 < slab // 4     # a wave walks past four rows of a slab, fewer of the last
    nbytes = int(lib.qk_qlnorm_workspace_bytes(ctypes.byref(desc), _lib.QK_OP_BWD))
    assert nbytes % (5 * q * 4) == 0
    slabs = nbytes // (5 * q * 4)
    assert slabs == -(-rows // slab)
    runs = 64 if q % 4 == 0 else 16                                     # k_qln_reduce<4> / <1>: 1024 threads over 16 / 64 column groups
    per = -(-slabs // runs)
    assert per >= 5 and per % 4 != 0                                    # the unrolled loop AND its tail run in every full run
    assert slabs % per != 0                                             # and the last non-empty run is a short one
    assert rows > 4 * 2048 > 4 * 1024                                   # both grid-stride loops (caps 1024 / 2048 workgroups) pass twice
    assert F.qlayer_norm_path(dtype, rows, q) == _norm_path(dtype, q)
    top = float(np.abs(_norm_exact_dbeta(q, KINDS[dtype])).max())
    assert 8 < top < LAT.FP32_EXACT and rows < LAT.FP32_EXACT


# ---- GPU part ---------------------------------------------------------------------------------------------------------------------
def _norm_run(dev, dtype, q, lattice=False):
    i = _norm_inputs(q, KINDS[dtype], lattice)
    t = lambda a, dt=dtype: torch.tensor(a, dtype=dt, device=dev)
    x, gamma, beta = t(i['x']).requires_grad_(), t(i['gamma'], torch.float32).requires_grad_(), t(i['beta'], torch.float32).requires_grad_()
    y = F.qlayer_norm(x, gamma, beta, torch.tensor(i['lengths'], device=dev), epsilon=EPS)
    y.backward(t(i['dy']))
    return dict(y=y.detach(), dx=x.grad, dgamma=gamma.grad, dbeta=beta.grad)


@pytest.mark.gpu
@pytest.mark.parametrize('q', N_QS)
@pytest.mark.parametrize('dtype', list(KINDS), ids=DTYPE_IDS)
def test_lnorm_many_rows(dtype, q):
    """B = 2200, T = 7 with lengths, affine: slabs of more than 16 rows with a ragged last one, both loops of the slab reduction, a
    second pass of the grid-stride loops.  Parity on y, dx, dgamma, dbeta; inactive rows exactly zero."""
    dev = _dev()
    assert F.qlayer_norm_path(dtype, NB * NT, q) == _norm_path(dtype, q)
    got = _norm_run(dev, dtype, q)
    _check(got, _norm_reference(q, KINDS[dtype]), dtype, N_OUT_32, 'lnorm many rows q=%d' % q)
    ln = _norm_inputs(q, KINDS[dtype])['lengths']
    inactive = torch.tensor(np.arange(NT)[None, :] >= ln[:, None], device=dev)
    assert int(inactive.sum()) > NT and int(got['y'][inactive].ne(0).sum()) == 0 and int(got['dx'][inactive].ne(0).sum()) == 0


@pytest.mark.gpu
@pytest.mark.parametrize('q', N_QS)
@pytest.mark.parametrize('dtype', list(KINDS), ids=DTYPE_IDS)
def test_lnorm_exact_bias_gradient(dtype, q):
    """dy from {-1, 0, 1}: dbeta is a sum of integers below 2^24, exact in fp32 in any order, and must EQUAL the float64 sum over
    the active rows.  One dropped or doubled row of 15 400 moves dbeta by one unit, 4e-3 of its maximum: at the edge of what the
    16-bit parity bound of test_lnorm_many_rows could let pass."""
    dev = _dev()
    got = _norm_run(dev, dtype, q, lattice=True)
    want = _norm_exact_dbeta(q, KINDS[dtype])
    assert got['dbeta'].dtype == torch.float32
    LAT.assert_equal_exact(got['dbeta'].cpu().numpy(), want, 'dbeta', 'bias')


# ==== C. depthwise / GLU convolution ===============================================================================================
D_OUT_16, D_OUT_32 = ('y', 'da', 'dg'), ('dw', 'dbias')
DT, DK, D_BATCHES, D_QS = 40, 5, (130, 257), (8, 5)
D_HEAD = {130: [0, DT, 0, 0, 1], 257: [0, DT, 1, 0, 0, 0]}           # slab 0 mixes an empty row with a full one; slab 1 is empty
# the tap counts strictly inside the buckets, the full KB = 7 bucket and the asymmetric 'same' of an even K, at the shape of
# tests/test_qdwconv.py
D_TAPS = ((4, 'same'), (5, 'same'), (7, 'same'), (9, 'causal'), (17, 'same'))
D_TAP_IDS = ['k4', 'k5', 'k7', 'k9_causal', 'k17']
D_TAP_B, D_TAP_T = 6, 150
D_TAP_LENGTHS = np.array([0, 1, 64, 65, D_TAP_T - 2, D_TAP_T], dtype=np.int32)


def _dw_path(dtype, q):
    return 'vec' if q % (4 if dtype == torch.float32 else 8) == 0 else 'generic'


def _dw_lengths(bsz):
    if bsz == D_TAP_B:
        return D_TAP_LENGTHS
    out = np.random.RandomState(7100 + bsz).randint(0, DT + 1, size=bsz).astype(np.int32)
    out[:len(D_HEAD[bsz])] = D_HEAD[bsz]
    return out


@functools.lru_cache(maxsize=None)
def _dw_inputs(bsz, steps, q, taps, kind):
    """Seeded operands (never written) drawn as tests/test_qdwconv.py draws them."""
    rng = np.random.RandomState(7000 + 37 * q + taps + bsz)
    d = dict(a=DR.rnd(_f32(rng.randn(bsz, steps, 4 * q)), kind), g=DR.rnd(_f32(1.5 * rng.randn(bsz, steps, 4 * q)), kind),
             dy=DR.rnd(_f32(rng.randn(bsz, steps, 4 * q)), kind), w=_f32(rng.randn(taps, 4 * q) / np.sqrt(taps)), bias=_f32(0.3 * rng.randn(4 * q)),
             lengths=_dw_lengths(bsz))
    return _freeze(d)


@functools.lru_cache(maxsize=None)
def _dw_reference(bsz, steps, q, taps, padding, kind, rounded=True):
    i = _dw_inputs(bsz, steps, q, taps, kind)
    return DR.qdwconv(i['a'], i['w'], i['bias'], i['g'], i['lengths'], padding, kind if rounded else None, i['dy'])


@functools.lru_cache(maxsize=None)
def _dw_lattice(bsz, q):
    """a, dy, w, bias from {-1, 0, 1} and the reference of the plain path on them."""
    rng = np.random.RandomState(7200 + bsz + q)
    ops = dict(a=LAT.integer_lattice(rng, (bsz, DT, 4 * q)), dy=LAT.integer_lattice(rng, (bsz, DT, 4 * q)), w=LAT.integer_lattice(rng, (DK, 4 * q)),
               bias=LAT.integer_lattice(rng, (4 * q,)), lengths=_dw_lengths(bsz))
    _freeze(ops)
    return ops, DR.qdwconv(ops['a'], ops['w'], ops['bias'], None, ops['lengths'], 'same', None, ops['dy'])


# ---- CPU part ---------------------------------------------------------------------------------------------------------------------
D_BUDGET = [(b, DT, q, DK, 'same') for b in D_BATCHES for q in D_QS] + [(D_TAP_B, D_TAP_T, q, k, p) for k, p in D_TAPS for q in D_QS]


@pytest.mark.parametrize('kind', ['bf16', 'fp16'])
@pytest.mark.parametrize('bsz,steps,q,taps,padding', D_BUDGET, ids=['b%d_q%d_k%d_%s' % (b, q, k, p) for b, _, q, k, p in D_BUDGET])
def test_dwconv_rounding_points_move_the_reference_by_at_most_half_the_16_bit_bound(bsz, steps, q, taps, padding, kind):
    """Both input families of the convolution cases: the three rounding points move y, da, dg by at most 3.5e-3 (bf16) / 4.1e-4
    (fp16) (measured) and leave dw and dbias, sums of the inputs alone, exactly where they are."""
    _budget(_dw_reference(bsz, steps, q, taps, padding, kind), _dw_reference(bsz, steps, q, taps, padding, kind, rounded=False), kind,
            D_OUT_16, D_OUT_32, True, 'dwconv B=%d q=%d K=%d %s' % (bsz, q, taps, padding))


@pytest.mark.parametrize('q', D_QS)
@pytest.mark.parametrize('dtype', list(KINDS), ids=DTYPE_IDS)
def test_dwconv_geometry_of_the_multi_row_slab_cases(dtype, q):
    """From qk_qdwconv_workspace_bytes: fewer slabs than rows at both batches (so slabs of two or more rows), and a ragged last slab
    at one of them.  (Today: B = 130 gives 65 slabs of exactly 2 rows; B = 257 gives 86 slabs of 3 rows and a last one of 2.)  The
    lengths put an empty row next to a full one in slab 0 and make slab 1 all empty."""
    lib = _lib.lib()
    ragged = []
    for bsz in D_BATCHES:
        desc = F.qdwconv_desc(dtype, bsz, DT, q, DK, F.qdwconv_pad_lo(DK, 'same'))
        nbytes = int(lib.qk_qdwconv_workspace_bytes(ctypes.byref(desc), _lib.QK_OP_BWD))
        line = (DK + 1) * 4 * q * 4
        assert nbytes > 0 and nbytes % line == 0
        slabs = nbytes // line
        rows = -(-bsz // slabs)                                          # rows per slab
        assert slabs < bsz and rows >= 2 and slabs == -(-bsz // rows)
        ragged.append(bsz % rows != 0)
        ln = _dw_lengths(bsz)
        assert min(ln[:rows]) == 0 and max(ln[:rows]) == DT              # slab 0: an empty row and a full one
        assert (ln[rows:2 * rows] == 0).all()                            # slab 1: nothing
        assert F.qdwconv_path(dtype, bsz, DT, q, DK, packed=True) == _dw_path(dtype, q)
    assert ragged[1] and any(ragged)                                     # B = 257 is no multiple of its rows per slab
    assert F.qdwconv_pad_lo(4, 'same') == 1 and F.qdwconv_pad_lo(9, 'causal') == 8
    for bsz in D_BATCHES:
        ops, want = _dw_lattice(bsz, q)
        assert np.abs(want['y']).max() <= 4 * DK + 1 <= LAT.exact_range(dtype) and np.abs(want['da']).max() <= 4 * DK
        assert bsz * DT * 4 < LAT.FP32_EXACT and np.abs(want['y']).max() > 4 and np.abs(want['dw']).max() > 8


# ---- GPU part ---------------------------------------------------------------------------------------------------------------------
def _dw_run(dev, dtype, ops, padding, gated):
    """functional.qglu_dwconv1d (plain: qdwconv1d) forward and backward on `ops`: name -> tensor."""
    t = lambda a, dt=dtype: torch.tensor(np.asarray(a), dtype=dt, device=dev)
    ln = torch.tensor(ops['lengths'], device=dev)
    w, bias = t(ops['w'], torch.float32).requires_grad_(), t(ops['bias'], torch.float32).requires_grad_()
    if gated:
        x = t(DR.merge_packed(ops['a'], ops['g'])).requires_grad_()
        y = F.qglu_dwconv1d(x, w, bias, ln, padding)
    else:
        x = t(ops['a']).requires_grad_()
        y = F.qdwconv1d(x, w, bias, ln, padding)
    y.backward(t(ops['dy']))
    res = dict(y=y.detach())
    if gated:
        res['da'], res['dg'] = DR.split_packed(x.grad)
    else:
        res['da'] = x.grad
    res.update(dw=w.grad, dbias=bias.grad)
    return res


def _dw_zero_rows(dev, got, lengths, steps, names):
    mask = torch.tensor(np.arange(steps)[None, :] >= lengths[:, None], device=dev)
    for name in names:
        assert int(got[name][mask].ne(0).sum()) == 0, name


@pytest.mark.gpu
@pytest.mark.parametrize('q', D_QS)
@pytest.mark.parametrize('bsz', D_BATCHES)
@pytest.mark.parametrize('dtype', list(KINDS), ids=DTYPE_IDS)
def test_dwconv_multi_row_slabs(dtype, bsz, q):
    """B = 130 / 257, T = 40, K = 5 'same', gated: the weight-gradient kernels walk two / three rows per slab, a slab that mixes an
    empty row with a full one, an all-empty slab and (B = 257) a ragged last slab."""
    dev = _dev()
    ops = _dw_inputs(bsz, DT, q, DK, KINDS[dtype])
    got = _dw_run(dev, dtype, ops, 'same', True)
    assert F.qdwconv_last_path() == _dw_path(dtype, q)
    _check(got, _dw_reference(bsz, DT, q, DK, 'same', KINDS[dtype]), dtype, D_OUT_32, 'dwconv B=%d q=%d' % (bsz, q))
    _dw_zero_rows(dev, got, ops['lengths'], DT, D_OUT_16)


@pytest.mark.gpu
@pytest.mark.parametrize('q', D_QS)
@pytest.mark.parametrize('bsz', D_BATCHES)
@pytest.mark.parametrize('dtype', list(KINDS), ids=DTYPE_IDS)
def test_dwconv_lattice_at_those_batches_gives_the_reference_exactly(dtype, bsz, q):
    """The construction of test_qdwconv.py's lattice test on the plain path at B = 130 / 257: every product and partial sum is an
    integer, |y| <= 4 K + 1 = 21 and |da| <= 20 are exact in bf16, the dw / dbias sums stay below B T 4 < 2^24: y, da, dw, dbias
    equal the reference as numbers.  A dropped or doubled row of a slab cannot hide inside a tolerance."""
    dev = _dev()
    ops, want = _dw_lattice(bsz, q)
    got = _dw_run(dev, dtype, ops, 'same', False)
    assert F.qdwconv_last_path() == _dw_path(dtype, q)
    for name in ('y', 'da', 'dw', 'dbias'):
        LAT.assert_equal_exact(got[name].float().cpu().numpy(), want[name], name)


@pytest.mark.gpu
@pytest.mark.parametrize('taps,padding', D_TAPS, ids=D_TAP_IDS)
@pytest.mark.parametrize('q', D_QS)
@pytest.mark.parametrize('dtype', list(KINDS), ids=DTYPE_IDS)
def test_dwconv_tap_counts_inside_the_buckets(dtype, q, taps, padding):
    """B = 6, T = 150 with the lengths of tests/test_qdwconv.py, gated: K strictly inside a register bucket (the j - f < K guards),
    the full KB = 7 bucket in every dtype, and an even K (pad_lo = (K - 1) / 2: one more frame on the right)."""
    dev = _dev()
    ops = _dw_inputs(D_TAP_B, D_TAP_T, q, taps, KINDS[dtype])
    assert F.qdwconv_path(dtype, D_TAP_B, D_TAP_T, q, taps, packed=True) == _dw_path(dtype, q)
    got = _dw_run(dev, dtype, ops, padding, True)
    assert F.qdwconv_last_path() == _dw_path(dtype, q)
    _check(got, _dw_reference(D_TAP_B, D_TAP_T, q, taps, padding, KINDS[dtype]), dtype, D_OUT_32, 'dwconv K=%d %s q=%d' % (taps, padding, q))
    _dw_zero_rows(dev, got, ops['lengths'], D_TAP_T, D_OUT_16)
