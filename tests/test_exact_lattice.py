"""Exact-arithmetic parity: lattice operands, tolerance ZERO.

The oracle comparisons of tests/test_gpu_parity.py and tests/test_fullsize_oracle_parity.py use one norm-wise figure,
max|got - want| / max|want|, with bounds forced by the rounding of 16-bit outputs on Gaussian operands (1e-2 bf16 / 2e-3 fp16
for y and dx, 2e-3 / 1e-3 for dkernel and dbias).  A fault that moves single cells by about one term -- a tail lane of a DMA
chunk, the last K step of a padded form, a store that truncates -- sits inside those bounds, and a larger one is reported as
one number without a position.  Here the operands come from a small lattice
(tests/lattice_ref.py) on which every product, every partial sum in any order and every stored value is exactly
representable, so the HIP result must EQUAL the float64 oracle, and a mismatch is reported by position and tile.

What the norm-wise figure does with three planted faults (conv2d_body64_small, the bf16-rounded Gaussian operands of
test_half_matches_oracle_on_rounded_inputs; printed by the CPU tests below, `pytest -s`):

  (a) one term removed from one y cell                          rel err 9.26e-4   bound 1e-2 (bf16) / 2e-3 (fp16): INSIDE
  (b) the last 64 output positions left out of dkernel          rel err 0.37      bound 2e-3 (bf16) / 1e-3 (fp16): outside
      the same at the M = 22 400 rows of the sampled body
      cases (256 sampled entries; falls as sqrt(64 / M))        rel err 5.11e-2   outside
  (c) one Hamilton block's sign flipped for one (tap, channel)
      in one 32-filter column block of dkernel                  rel err 0.535     bound 2e-3 (bf16) / 1e-3 (fp16): outside

So the measured gap is the single-cell class (a) -- a term, a tail lane, a one-ulp store, anything that moves one cell by about
|x w| -- which sits an order of magnitude inside the bf16 bound; a whole dropped slice of M or a flipped block does show in the
norm-wise figure at these sizes (for (b), 0.0511 * sqrt(22 400 / 716 800) = 9e-3 at the benchmark's rows: still outside).
On the lattice each of the three fails assert_equal_exact, which names the planted position.

16-bit outputs on the DYADIC lattice are not exactly representable: they are held to the float64 result rounded ONCE to
the type, round-to-nearest-even (csrc/qk_common.h) -- ties are frequent there, so truncation or round-half-away fails.
"""
import re

import numpy as np
import pytest
import torch

import lattice_ref as LR
import test_fullsize_oracle_parity as FS
import test_gpu_parity as P
from oracle import oracle

SEED = 2024
DTYPES = {'fp32': torch.float32, 'bf16': torch.bfloat16, 'fp16': torch.float16}

# kernel densities below the default 0.5, per case: where the oracle's results would otherwise leave the exact range of the
# 16-bit type (assert_preconditions decides; a case that violates it FAILS)
KERNEL_DENSITY = {}


def _by_name(*names):
    return [c for c in P.ORACLE_CASES if c[0] in names]


def _ids(cases):
    return [c[0] for c in cases]


# ---------------------------------------------------------------------------------------------------------------------
# one oracle evaluation per (case, lattice), shared by every dtype / path / entry point that is compared with it
# ---------------------------------------------------------------------------------------------------------------------
_CASES = {}


def _lattice_case(case, lattice='integer'):
    """(x, kernel, bias, dy, want, abs_terms): RandomState(2024), draws in the order x, kernel, bias, dy; read-only."""
    name, rank, xs, ws, kw = case[:5]
    use_bias = case[5] if len(case) > 5 else True
    key = (name, lattice)
    if key not in _CASES:
        rng = np.random.RandomState(SEED)
        _, ys = oracle.make_desc(xs, ws, rank, use_bias=use_bias, **kw)
        x, w, b, dy = LR.layer_operands(rng, xs, ws, ys, use_bias, lattice, kernel_density=KERNEL_DENSITY.get(name, 0.5))
        y = oracle.forward(x, w, b, rank, **kw)
        dx, dw, db = oracle.backward(x, w, b, dy, rank, y=y, **kw)
        want = dict(y=y, dx=dx, dkernel=dw)
        if use_bias:
            want['dbias'] = db
        terms = LR.term_bounds(x, w, b, dy, int(np.prod(ys)) // ws[-1])
        for a in (x, w, b, dy) + tuple(want.values()):
            if a is not None:
                a.flags.writeable = False
        _CASES[key] = (x, w, b, dy, want, {k: v for k, v in terms.items() if k in want})
    return _CASES[key]


def _compare(got, want, rank, kw, what=''):
    lay = LR.layout_of(rank, kw)
    hints = dict(y=lay, dx=lay, dkernel='kernel', dbias='bias')
    for k, v in got.items():
        LR.assert_equal_exact(v, want[k], what + k, hints[k])


# ---------------------------------------------------------------------------------------------------------------------
# 2. CPU: the checker itself (planted faults, the precondition checker)
# ---------------------------------------------------------------------------------------------------------------------
BODY64 = _by_name('conv2d_body64_small')[0]


def _gaussian_body64():
    if 'gauss' not in _CASES:
        _, rank, xs, ws, kw = BODY64
        _CASES['gauss'] = P._oracle_case(rank, xs, ws, kw, seed=11, dtype=torch.bfloat16)
    return _CASES['gauss']


def _plant_missing_term(x, w, y):
    """A copy of y with the centre-tap term x_r[c = 5] * w_r[1, 2, 5, f] removed from the first cell (component r) where the
    term is non-zero and the cell stays positive; returns (copy, (h, wd, f))."""
    fq = w.shape[-1] // 4
    term = np.asarray(x, np.float64)[0, :, :, 5][:, :, None] * np.asarray(w, np.float64)[1, 2, 5, :fq][None, None, :]
    cell = np.asarray(y, np.float64)[0, :, :, :fq]
    ok = (term != 0) & (cell > 0) & (cell - term > 0)
    h, wd, f = (int(v[0]) for v in np.nonzero(ok))
    out = np.array(y, dtype=np.float64)
    out[0, h, wd, f] -= term[h, wd, f]
    return out, (h, wd, f)


def _plant_dropped_slice(x, w, b, dy, y):
    """dkernel with the last 64 output positions left out of the sum over M."""
    _, rank, _, _, kw = BODY64
    cut = np.array(dy, dtype=np.float64)
    cut.reshape(-1, cut.shape[-1])[-64:] = 0
    return oracle.backward(x, w, b, cut, rank, y=y, **kw)[1]


PLANT_TAP, PLANT_CQ, PLANT_A, PLANT_B, PLANT_BLOCK = (1, 3), 7, 1, 3, 1


def _plant_sign_flip(x, w, b, dy, y, dw):
    """dkernel with the sign of ONE Hamilton block flipped -- input component i against output component k, which lands in
    compact part j = i ^ k -- for tap (1, 3), input channel 7, filters 32..63.  The block's own contribution is the oracle's
    kernel gradient with every other component of x and every other column of dy zeroed."""
    _, rank, _, _, kw = BODY64
    cq, fq = w.shape[-2], w.shape[-1] // 4
    xa, dyb = np.zeros(x.shape), np.zeros(dy.shape)
    xa[..., PLANT_A * cq + PLANT_CQ] = x[..., PLANT_A * cq + PLANT_CQ]
    cols = slice(PLANT_B * fq + 32 * PLANT_BLOCK, PLANT_B * fq + 32 * PLANT_BLOCK + 32)
    dyb[..., cols] = dy[..., cols]
    part = oracle.backward(xa, w, b, dyb, rank, y=y, **kw)[1]
    lo = (PLANT_A ^ PLANT_B) * fq + 32 * PLANT_BLOCK
    out = np.array(dw, dtype=np.float64)
    out[PLANT_TAP[0], PLANT_TAP[1], PLANT_CQ, lo:lo + 32] -= 2 * part[PLANT_TAP[0], PLANT_TAP[1], PLANT_CQ, lo:lo + 32]
    return out


def _rejected(got, want, name, hint):
    with pytest.raises(AssertionError) as e:
        LR.assert_equal_exact(got, want, name, hint)
    return str(e.value)


def test_planted_missing_term_in_one_y_cell_is_named():
    x, w, b, dy, want, _ = _lattice_case(BODY64)
    LR.assert_equal_exact(want['y'].astype(np.float32), want['y'], 'y', 'channels_last')          # the checker accepts the truth
    bad, (h, wd, f) = _plant_missing_term(x, w, want['y'])
    msg = _rejected(bad, want['y'], 'y', 'channels_last')
    assert msg.startswith('y: 1 of %d values differ' % bad.size), msg
    row = h * want['y'].shape[2] + wd
    assert 'sample 0, position (%d, %d), component r, channel %d [64-row tile %d, 32-column block %d]' \
        % (h, wd, f, row // 64, f // 32) in msg, msg
    gx, gw, gb, gdy, gwant = _gaussian_body64()
    gbad, _ = _plant_missing_term(gx, gw, gwant['y'])
    print('\n(a) one missing term of one y cell, Gaussian operands: rel err %.3g  (bound 1e-2 bf16 / 2e-3 fp16)'
          % P._rel_err(gbad, gwant['y']))


def test_planted_dropped_slice_of_m_in_dkernel_is_named():
    x, w, b, dy, want, _ = _lattice_case(BODY64)
    bad = _plant_dropped_slice(x, w, b, dy, want['y'])
    msg = _rejected(bad, want['dkernel'], 'dkernel', 'kernel')
    n_bad = int(re.match(r'dkernel: (\d+) of', msg).group(1))
    assert n_bad == int((bad != want['dkernel']).sum()) and n_bad > bad.size // 2, msg
    tap0, tap1, cq, ch = (int(v) for v in np.unravel_index(int(np.flatnonzero(bad != want['dkernel'])[0]), bad.shape))
    fq = bad.shape[-1] // 4
    assert 'first: tap (%d, %d), input channel %d, component %s, filter %d [64-row tile' \
        % (tap0, tap1, cq, 'rijk'[ch // fq], ch % fq) in msg, msg
    gx, gw, gb, gdy, gwant = _gaussian_body64()
    gbad = _plant_dropped_slice(gx, gw, gb, gdy, gwant['y'])
    print('\n(b) last 64 positions left out of dkernel, Gaussian operands, M = 560: rel err %.3g  (bound 2e-3 bf16 / 1e-3 fp16)'
          % P._rel_err(gbad, gwant['dkernel']))
    # the figure falls as sqrt(64 / M): the same fault at the M = 22 400 rows of the sampled body cases below (sampled oracle)
    rng = np.random.RandomState(11)
    xs, ws = (8, 14, 200, 256), (3, 5, 64, 256)
    bx, bdy = rng.randn(*xs).astype(np.float32), rng.randn(*xs).astype(np.float32)
    iw = FS.sample_indices(rng, ws, 256)
    full = oracle.backward_at(bx, np.zeros(ws), bdy, 2, dw_idx=iw, padding='same', activation=None)[1]
    bdy.reshape(-1, 256)[-64:] = 0
    cut = oracle.backward_at(bx, np.zeros(ws), bdy, 2, dw_idx=iw, padding='same', activation=None)[1]
    print('    the same fault at M = 22 400 (256 sampled entries): rel err %.3g' % P._rel_err(cut, full))


def test_planted_sign_flip_of_one_hamilton_block_in_dkernel_is_named():
    x, w, b, dy, want, _ = _lattice_case(BODY64)
    bad = _plant_sign_flip(x, w, b, dy, want['y'], want['dkernel'])
    msg = _rejected(bad, want['dkernel'], 'dkernel', 'kernel')
    n_bad = int(re.match(r'dkernel: (\d+) of', msg).group(1))
    assert 16 <= n_bad <= 32, msg
    for line in msg.splitlines()[1:]:
        assert re.search(r'tap \(1, 3\), input channel 7, component j, filter (3[2-9]|[45]\d|6[0-3]) '
                         r'\[64-row tile %d, 32-column block 1\]' % (((1 * 5 + 3) * 64 + 7) // 64), line), msg
    gx, gw, gb, gdy, gwant = _gaussian_body64()
    print('\n(c) one sign block flipped in dkernel, Gaussian operands: rel err %.3g  (bound 2e-3 bf16 / 1e-3 fp16)'
          % P._rel_err(_plant_sign_flip(gx, gw, gb, gdy, gwant['y'], gwant['dkernel']), gwant['dkernel']))


def test_precondition_checker_refuses_operands_that_are_too_dense():
    rng = np.random.RandomState(SEED)
    xs, ws = (32, 4 * 8192), (8192, 32)
    x, w, b, _ = LR.layer_operands(rng, xs, ws, None, True, 'integer', density=1.0, kernel_density=1.0)
    y = oracle.forward(x, w, b, 0, activation=None)
    terms = LR.term_bounds(x, w, b, None, 32)
    assert 256 < np.abs(y).max() <= 2048
    with pytest.raises(AssertionError, match='y: max .* exceeds the exact range 256 of bfloat16'):
        LR.assert_preconditions(dict(y=y), torch.bfloat16, abs_terms=terms)
    LR.assert_preconditions(dict(y=y), torch.float16, abs_terms=terms)             # 11 significand bits hold it
    LR.assert_preconditions(dict(dkernel=y), torch.bfloat16, abs_terms=terms)      # an fp32 output: 2^24
    with pytest.raises(AssertionError, match='leaves the lattice'):
        LR.assert_preconditions(dict(y=y + 0.5), torch.float16)
    LR.assert_preconditions(dict(y=y + 0.5), torch.float16, unit=1.0 / 64, exact_store=False)
    with pytest.raises(AssertionError, match='sum of absolute terms'):
        LR.assert_preconditions(dict(y=y), torch.float16, abs_terms=dict(dkernel=4.0 * 2 ** 22))
    with pytest.raises(AssertionError, match='sum of absolute terms'):
        LR.assert_preconditions(dict(y=y), torch.float16, unit=1.0 / 64, abs_terms=dict(dkernel=2.0 ** 18), exact_store=False)
    assert LR.exact_range(torch.bfloat16) == 256 and LR.exact_range(torch.float16) == 2048 and LR.exact_range(torch.float32) == 2 ** 24
    for dt, top in ((torch.bfloat16, 256), (torch.float16, 2048)):                 # exact_range is the edge: top + 1 is the first loss
        ints = torch.arange(-top, top + 1, dtype=torch.float64)
        assert torch.equal(ints.to(dt).double(), ints) and float(torch.tensor(top + 1.0).to(dt)) != top + 1


def test_dyadic_lattice_makes_bf16_stores_round_with_frequent_ties():
    """What makes the one-rounding test below bite: on the dyadic lattice a body layer's y and dx are multiples of 1/16, so
    in bf16 every odd multiple of magnitude 16 and above rounds, most of them as exact ties -- truncation, and round-half-away
    on the ties whose kept significand is even, give other numbers than round-to-nearest-even.  (In fp16, and at the first
    layer's 60 terms, these values are representable: the same test then demands exact equality.)"""
    want = _lattice_case(BODY64, 'dyadic')[4]
    for name in ('y', 'dx'):
        v = want[name].astype(np.float32)
        assert np.array_equal(v.astype(np.float64), want[name])
        bits = v.view(np.uint32)
        low = bits & np.uint32(0xffff)
        ties = low == 0x8000
        assert int((low != 0).sum()) >= 1000 and int(ties.sum()) >= 1000, (name, int((low != 0).sum()), int(ties.sum()))
        rne = _store_once(want[name], torch.bfloat16)
        trunc = (bits & np.uint32(0xffff0000)).view(np.float32).astype(np.float64)
        away = ((bits + np.uint32(0x8000)) & np.uint32(0xffff0000)).view(np.float32).astype(np.float64)
        assert int((trunc != rne).sum()) >= 1000 and int((away != rne).sum()) >= 100, name
        assert np.array_equal(away != rne, ties & ((bits >> np.uint32(16)) & np.uint32(1) == 0))


def test_lattice_generators_stay_on_their_lattice():
    rng = np.random.RandomState(1)
    v = LR.integer_lattice(rng, (4000,), 0.25)
    assert set(np.unique(v)) == {-1.0, 0.0, 1.0} and abs((v != 0).mean() - 0.25) < 0.03 and abs(v.sum()) < 150
    assert set(np.unique(LR.integer_bias(rng, 500))) == {-2.0, -1.0, 0.0, 1.0, 2.0}
    a = LR.dyadic_lattice(rng, (4000,), 'activation')
    assert np.array_equal(a * 8, np.rint(a * 8)) and np.abs(a).max() == 1.0 and len(np.unique(a)) == 17
    assert set(np.unique(LR.dyadic_lattice(rng, (4000,), 'kernel'))) == {-1.0, -0.5, 0.0, 0.5, 1.0}
    bb = LR.dyadic_lattice(rng, (500,), 'bias')
    assert np.array_equal(bb * 2, np.rint(bb * 2)) and np.abs(bb).max() == 2.0


# ---------------------------------------------------------------------------------------------------------------------
# 3a. every default kernel path, integer lattice, zero tolerance
# ---------------------------------------------------------------------------------------------------------------------
def _check_layer(case, dtype, run, what='', **extra_kw):
    import qcnn_amd
    _, rank, xs, ws, kw = case[:5]
    x, w, b, dy, want, terms = _lattice_case(case)
    LR.assert_preconditions(want, dtype, abs_terms=terms)
    got = run(qcnn_amd.functional, x, w, b, dy, rank, dict(kw, **extra_kw), dtype)
    assert set(got) == set(want)
    _compare(got, want, rank, kw, what)


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', ['fp32', 'bf16', 'fp16'])
@pytest.mark.parametrize('case', P.HALF_CASES, ids=_ids(P.HALF_CASES))
def test_default_paths_are_exact_on_the_integer_lattice(case, dtype):
    _check_layer(case, DTYPES[dtype], P._run_layer)


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', ['bf16', 'fp16'])
@pytest.mark.parametrize('case', P.NATIVE_16BIT, ids=_ids(P.NATIVE_16BIT))
def test_native_channels_first_layout_is_exact_on_the_integer_lattice(case, dtype):
    run = lambda F, x, w, b, dy, rank, kw, dt: P._run_layer(F, x, w, b, dy, rank, kw, dt, internal_layout='native')
    _check_layer(case, DTYPES[dtype], run, fold_small_cq=False)


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', ['fp32', 'bf16', 'fp16'])
@pytest.mark.parametrize('case', P.CONJ_CASES, ids=_ids(P.CONJ_CASES))
def test_conj_and_tap_skipping_convolutions_are_exact_on_the_integer_lattice(case, dtype):
    _check_layer(case, DTYPES[dtype], P._run_layer)


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', ['fp32', 'bf16'])
@pytest.mark.parametrize('case', P.RAGGED_CASES, ids=_ids(P.RAGGED_CASES))
def test_ragged_and_degenerate_shapes_are_exact_on_the_integer_lattice(case, dtype):
    _check_layer(case, DTYPES[dtype], P._run_layer)


@pytest.mark.gpu
@pytest.mark.parametrize('layout', ['channels_last', 'native'])
@pytest.mark.parametrize('dtype', ['fp32', 'bf16'])
@pytest.mark.parametrize('case', P.FUZZ_CASES, ids=_ids(P.FUZZ_CASES))
def test_random_layer_configurations_are_exact_on_the_integer_lattice(case, dtype, layout):
    _check_layer(case, DTYPES[dtype], P._run_native if layout == 'native' else P._run_layer)


# ---------------------------------------------------------------------------------------------------------------------
# 3c. the A/B-switch kernels (same switches x cases as test_ab_switch_kernels_match_oracle)
# ---------------------------------------------------------------------------------------------------------------------
AB_SWITCHES = [m.args[1] for m in P.test_ab_switch_kernels_match_oracle.pytestmark if m.args[0] == 'switch'][0]


@pytest.mark.gpu
@pytest.mark.parametrize('switch', AB_SWITCHES)
@pytest.mark.parametrize('case', P.AB_SWITCH_CASES, ids=_ids(P.AB_SWITCH_CASES))
def test_ab_switch_kernels_are_exact_on_the_integer_lattice(case, switch):
    from qcnn_amd import _lib

    def run(*a):
        with _lib.debug_flags(getattr(_lib, switch)):
            return P._run_layer(*a)
    _check_layer(case, torch.bfloat16, run, what='under %s: ' % switch)


# ---------------------------------------------------------------------------------------------------------------------
# 3b / 3f. the C-ABI entry points on their own: fwd, bwd_data, bwd_weight, the fused bwd, the accumulate forms
# ---------------------------------------------------------------------------------------------------------------------
ABI_CASES = P.AB_SWITCH_CASES + _by_name('conv2d_16to16_5tap_relu', 'dense_point_64', 'conv2d_first_layer')


def _abi_call(F, case, dtype, activation):
    _, rank, xs, ws, kw = case
    if rank == 0:
        return F.dense_call(xs, ws, dtype, activation, True)
    return F.conv_call(xs, ws, dtype, rank, kw.get('strides', 1), kw['padding'], kw.get('data_format', 'channels_last'),
                       kw.get('dilation_rate', 1), activation, True, kw.get('conj', False))


def _store_once(a, dtype):
    """The float64 result converted ONCE to the storage type, round-to-nearest-even (csrc/qk_common.h)."""
    return torch.tensor(np.asarray(a)).float().to(dtype).double().numpy()


def _abi_entry_points(case, dtype, lattice):
    """Every entry point against the oracle; the relu mask handed to the backward calls is the ORACLE's y in the storage
    type, so that each entry point stands on its own."""
    import qcnn_amd
    F = qcnn_amd.functional
    dev = P._dev()
    _, rank, xs, ws, kw = case
    x, w, b, dy, want, terms = _lattice_case(case, lattice)
    if lattice == 'integer':
        LR.assert_preconditions(want, dtype, abs_terms=terms)
        want16 = want
    else:
        LR.assert_preconditions(want, dtype, unit=1.0 / 64, abs_terms=terms, exact_store=False)
        want16 = dict(want, y=_store_once(want['y'], dtype), dx=_store_once(want['dx'], dtype))
    lay = LR.layout_of(rank, kw)
    hints = dict(y=lay, dx=lay, dkernel='kernel', dbias='bias')
    relu = kw.get('activation') == 'relu'
    call = _abi_call(F, case, dtype, kw.get('activation'))
    xt, dyt = torch.tensor(x, device=dev).to(dtype), torch.tensor(dy, device=dev).to(dtype)
    wt, bt = torch.tensor(w, device=dev), torch.tensor(b, device=dev)
    ymask = torch.tensor(want['y'], device=dev).to(dtype) if relu else None
    h = lambda t: t.float().cpu().numpy()

    def check(entry, **got):
        for k, v in got.items():
            LR.assert_equal_exact(h(v), want16[k], '%s: %s' % (entry, k), hints[k])
    check('fwd', y=call.fwd(xt, wt, bt))
    check('bwd_data', dx=call.bwd_data(dyt, ymask, wt))
    dw, db = call.bwd_weight(xt, dyt, ymask, True)
    check('bwd_weight', dkernel=dw, dbias=db)
    dx, dw, db = call.bwd(xt, dyt, ymask, wt, True)
    check('bwd', dx=dx, dkernel=dw, dbias=db)
    return F, call, (xt, dyt, wt, bt, ymask), check


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', ['bf16', 'fp16'])
@pytest.mark.parametrize('case', ABI_CASES, ids=_ids(ABI_CASES))
def test_c_abi_entry_points_are_exact_on_the_integer_lattice(case, dtype):
    dtype = DTYPES[dtype]
    F, call, (xt, dyt, wt, bt, ymask), _ = _abi_entry_points(case, dtype, 'integer')
    _, rank, xs, ws, kw = case
    x, w, b, dy, want, _ = _lattice_case(case)
    dev = xt.device
    rng = np.random.RandomState(7)
    fill_w = rng.randint(-3, 4, size=ws).astype(np.float32)
    fill_b = rng.randint(-3, 4, size=ws[-1]).astype(np.float32)
    # qk_*_bwd_weight_acc: exactly pre-fill + gradient
    acc_w, acc_b = torch.tensor(fill_w, device=dev), torch.tensor(fill_b, device=dev)
    call.bwd_weight(xt, dyt, ymask, True, out=(acc_w, acc_b), accumulate=True)
    LR.assert_equal_exact(acc_w.cpu().numpy(), fill_w + want['dkernel'], 'bwd_weight_acc: dkernel', 'kernel')
    LR.assert_equal_exact(acc_b.cpu().numpy(), fill_b + want['dbias'], 'bwd_weight_acc: dbias', 'bias')
    if rank == 0 or kw.get('data_format') == 'channels_first':
        return                       # qk_conv_bwd_post takes convolution descriptors on channels_last buffers only (include/qk.h)
    # qk_conv_bwd_post with QK_BWD_ACCUMULATE, the relu form of the producer's post-op without dropout: the LINEAR layer's
    # backward on the pre-masked dy (the same gradients as the relu layer's), dx multiplied by (x > 0)
    lin = _abi_call(F, case, dtype, None)
    dym = dyt * (ymask > 0) if ymask is not None else dyt
    acc_w, acc_b = torch.tensor(fill_w, device=dev), torch.tensor(fill_b, device=dev)
    dx, _, _ = lin.bwd_post(xt, dym, wt, True, F.PostOp(None, -1, 0.0, 1), None, None, direct=(acc_w, acc_b))
    lay = LR.layout_of(rank, kw)
    LR.assert_equal_exact(dx.float().cpu().numpy(), want['dx'] * (x > 0), 'bwd_post: dx', lay)
    LR.assert_equal_exact(acc_w.cpu().numpy(), fill_w + want['dkernel'], 'bwd_post (accumulate): dkernel', 'kernel')
    LR.assert_equal_exact(acc_b.cpu().numpy(), fill_b + want['dbias'], 'bwd_post (accumulate): dbias', 'bias')


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', ['bf16', 'fp16'])
@pytest.mark.parametrize('case', ABI_CASES, ids=_ids(ABI_CASES))
def test_16bit_stores_round_once_to_nearest_even_on_the_dyadic_lattice(case, dtype):
    """fp32 outputs exact; 16-bit outputs equal the float64 result rounded once (ties to even)."""
    _abi_entry_points(case, DTYPES[dtype], 'dyadic')


# ---------------------------------------------------------------------------------------------------------------------
# 3d. post-op forms, exact: dropout 0.5 (scale exactly 2), PReLU slopes from {1/4, 1/2, 1, 2}
# ---------------------------------------------------------------------------------------------------------------------
SLOPES = np.array([0.25, 0.5, 1.0, 2.0])
RATE = 0.5


def _survives_store(a, dtype):
    a = np.asarray(a, dtype=np.float64)
    return np.array_equal(torch.tensor(a).to(dtype).double().numpy(), a)


def _keep(shape, seed):
    return FS.drop_factor_at(np.arange(int(np.prod(shape))), seed, RATE).reshape(shape)


POST_LAYERS = [
    # the second body layer and the conj 'valid' head of the existing chain tests (test_conv_chain_with_*_matches_oracle_composition)
    ('body_32to64', (2, 6, 40, 128), (3, 5, 32, 256), dict(padding='same'), 1.0 / 8),
    ('head_conj_valid', (2, 6, 40, 256), (6, 1, 64, 128), dict(padding='valid', conj=True), 1.0 / 8),
]


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', ['fp32', 'bf16', 'fp16'])
@pytest.mark.parametrize('form', ['relu', 'prelu_one_slope', 'prelu_slope_per_row'])
@pytest.mark.parametrize('layer', POST_LAYERS, ids=_ids(POST_LAYERS))
def test_conv_post_op_launches_are_exact_on_the_integer_lattice(layer, form, dtype):
    """qk_conv_fwd_post / qk_conv_bwd_post: the layer's input is itself a post-op output x = post_x(x_pre) of an integer x_pre,
    its output goes through post_y; values, the stored pre-activation, d x_pre, dkernel, dbias and d alpha of post_x against the
    float64 composition (oracle's LINEAR layer + numpy post-op + the restated counter hash)."""
    import qcnn_amd
    F = qcnn_amd.functional
    dev = P._dev()
    dtype = DTYPES[dtype]
    _, xs, ws, kw, dens = layer
    rng = np.random.RandomState(SEED)
    x_pre, w, b, _ = LR.layer_operands(rng, xs, ws, None, True, 'integer', kernel_density=dens)
    seed_x, seed_y = 1234, 98765
    prelu = form != 'relu'
    _, ys = oracle.make_desc(xs, ws, 2, **kw)

    def slopes(shape):
        if not prelu:
            return None, -1, 0.0
        per_row = form == 'prelu_slope_per_row' and shape[1] > 1          # one slope per position of spatial axis 0
        a = SLOPES[rng.randint(0, 4, size=shape[1] if per_row else 1)].astype(np.float32)
        return a, (0 if per_row else -1), (a.astype(np.float64).reshape(1, -1, 1, 1) if per_row else float(a[0]))
    al_x, ax_x, ab_x = slopes(xs)
    al_y, ax_y, ab_y = slopes(ys)
    keep_x, keep_y = _keep(xs, seed_x), _keep(ys, seed_y)
    x = P._np_post(x_pre.astype(np.float64), ab_x, keep_x)
    pre = oracle.forward(x, w, b, 2, activation=None, **kw)
    y = P._np_post(pre, ab_y, keep_y)
    dy = LR.integer_lattice(rng, ys)
    dx_lin, dw, db = oracle.backward(x, w, b, dy, 2, activation=None, **kw)
    g = dx_lin * keep_x
    if prelu:
        dx = np.where(x_pre > 0, g, np.where(x_pre < 0, ab_x * g, 0.0))
        neg = g * np.minimum(x_pre, 0)
        dalpha = neg.sum(axis=(0, 2, 3)) if form == 'prelu_slope_per_row' else neg.sum().reshape(1)
    else:
        dx = g * (x > 0)
    # preconditions on the float64 composition: every 16-bit tensor survives its store, every fp32 sum stays below 2^24 units
    # of 1/8 (x is a multiple of 1/2, so is pre; dy, kernel integers)
    for name, a in (('x', x), ('pre', pre), ('y', y), ('dx', dx)):
        assert _survives_store(a, dtype), '%s leaves the exact range of %s: lower the kernel density' % (name, dtype)
    terms = LR.term_bounds(x, w, b, dy, int(np.prod(ys[:-1])))
    results = dict(dkernel=dw, dbias=db)
    if prelu:
        terms['dalpha'] = float(np.abs(neg).sum())
        results['dalpha'] = dalpha
    LR.assert_preconditions(results, dtype, unit=1.0 / 8, abs_terms=terms)
    t16 = lambda a: torch.tensor(np.asarray(a, dtype=np.float32), device=dev).to(dtype)
    t32 = lambda a: None if a is None else torch.tensor(np.asarray(a, dtype=np.float32), device=dev)
    xt, dyt, wt, bt = t16(x), t16(dy), t32(w), t32(b)
    post_x, post_y = F.PostOp(t32(al_x), ax_x, RATE, seed_x), F.PostOp(t32(al_y), ax_y, RATE, seed_y)
    assert post_x.applied_rate == 0.5
    call = F.conv_call(xs, ws, dtype, 2, 1, kw['padding'], 'channels_last', 1, None, True, kw.get('conj', False))
    got_pre, got_y = call.fwd_post(xt, wt, bt, post_y)
    h = lambda t: t.float().cpu().numpy()
    LR.assert_equal_exact(h(got_y), y, 'fwd_post: y', 'channels_last')
    if prelu:
        LR.assert_equal_exact(h(got_pre), pre, 'fwd_post: pre', 'channels_last')
    else:
        assert got_pre is None
    da = torch.zeros(al_x.size, device=dev) if prelu else None
    got_dx, got_dw, got_db = call.bwd_post(xt, dyt, wt, True, post_x, t16(x_pre) if prelu else None, da)
    LR.assert_equal_exact(h(got_dx), dx, 'bwd_post: d x_pre', 'channels_last')
    LR.assert_equal_exact(h(got_dw), dw, 'bwd_post: dkernel', 'kernel')
    LR.assert_equal_exact(h(got_db), db, 'bwd_post: dbias', 'bias')
    if prelu:
        LR.assert_equal_exact(h(da), dalpha, 'bwd_post: d alpha')


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', ['fp32', 'bf16', 'fp16'])
@pytest.mark.parametrize('layer', POST_LAYERS, ids=_ids(POST_LAYERS))
def test_chain_flag_backward_is_exact_on_the_integer_lattice(layer, dtype):
    """qk_conv_bwd_chain with QK_BWD_MASK_DX | QK_BWD_DY_PREMASKED inside a relu chain: x is a relu output (its own mask), dy
    arrives masked by the consumer, dx leaves masked by (x > 0)."""
    import qcnn_amd
    from qcnn_amd import _lib
    F = qcnn_amd.functional
    dev = P._dev()
    dtype = DTYPES[dtype]
    _, xs, ws, kw, _ = layer
    rng = np.random.RandomState(SEED + 1)
    x, w, b, _ = LR.layer_operands(rng, xs, ws, None, True, 'integer')
    x = np.maximum(x, 0)
    y = oracle.forward(x, w, b, 2, activation='relu', **kw)
    dym = LR.integer_lattice(rng, y.shape) * (y > 0)
    dx, dw, db = oracle.backward(x, w, b, dym, 2, activation=None, **kw)
    dx = dx * (x > 0)
    want = dict(y=y, dx=dx, dkernel=dw, dbias=db)
    LR.assert_preconditions(want, dtype, abs_terms=LR.term_bounds(x, w, b, dym, int(np.prod(y.shape[:-1]))))
    call = F.conv_call(xs, ws, dtype, 2, 1, kw['padding'], 'channels_last', 1, 'relu', True, kw.get('conj', False))
    xt, dyt = torch.tensor(x, device=dev).to(dtype), torch.tensor(dym, device=dev).to(dtype)
    wt, bt = torch.tensor(w, device=dev), torch.tensor(b, device=dev)
    yt = call.fwd(xt, wt, bt)
    got = call.bwd(xt, dyt, yt, wt, True, flags=_lib.QK_BWD_MASK_DX | _lib.QK_BWD_DY_PREMASKED)
    _compare(dict(zip(('y', 'dx', 'dkernel', 'dbias'), [t.float().cpu().numpy() for t in (yt,) + tuple(got)])), want, 2, kw)


def _first_layer_operands(shape, fq):
    rng = np.random.RandomState(SEED)
    x, w, b, _ = LR.layer_operands(rng, shape, (3, 5, 1, 4 * fq), None, True, 'integer')
    return rng, x.astype(np.float64), w.astype(np.float64), b.astype(np.float64)


def _route(pooled, arg, dp, like):
    d = np.zeros_like(like)
    n, ho, wd, c = pooled.shape
    ii = np.meshgrid(np.arange(n), np.arange(ho), np.arange(wd), np.arange(c), indexing='ij')
    np.add.at(d, (ii[0], arg, ii[2], ii[3]), dp)
    return d


@pytest.mark.gpu
@pytest.mark.parametrize('planes', [False, True], ids=['x_channels_last', 'x_component_planes'])
@pytest.mark.parametrize('dtype', ['bf16', 'fp16'])
@pytest.mark.parametrize('shape,fq', [((1, 8, 19, 4), 32), ((1, 8, 19, 4), 8)], ids=['partial_window_odd_width', 'f8_quarter_block'])
def test_fused_first_layer_conv_relu_pool_is_exact_on_the_integer_lattice(shape, fq, dtype, planes):
    """qk_conv_relu_pool_fwd / _bwd at the smallest shapes of test_fused_first_layer_conv_relu_pool_matches_oracle: pooled values,
    dkernel, dbias.  Integer outputs tie often inside a window: the first maximum wins on both sides (TF / torch)."""
    import qcnn_amd
    Fq = qcnn_amd.functional
    dev = P._dev()
    dtype = DTYPES[dtype]
    rng, x, w, b = _first_layer_operands(shape, fq)
    kw = dict(padding='same', activation='relu')
    y = oracle.forward(x, w, b, 2, **kw)
    pooled, arg = P._np_pool_h_same(y)
    dp = LR.integer_lattice(rng, pooled.shape).astype(np.float64)
    dy = _route(pooled, arg, dp, y)
    _, dw, db = oracle.backward(x, w, b, dy, 2, y=y, **kw)
    LR.assert_preconditions(dict(y=pooled, dkernel=dw, dbias=db), dtype, abs_terms=LR.term_bounds(x, w, b, dy, y.size // (4 * fq)))
    xt = torch.tensor(x, device=dev).to(dtype)
    wt = torch.tensor(w, device=dev, dtype=torch.float32, requires_grad=True)
    bt = torch.tensor(b, device=dev, dtype=torch.float32, requires_grad=True)
    lay = 'channels_last'
    if planes:
        xt, lay = xt.permute(0, 3, 1, 2).contiguous(), 'channels_first'
    assert Fq.conv_relu_pool_supported(xt, wt, 3, lay)
    out = Fq.conv_relu_pool(xt, wt, bt, 3, lay)
    out.backward(torch.tensor(dp, device=dev).to(dtype))
    LR.assert_equal_exact(out.detach().float().cpu().numpy(), pooled, 'pooled', 'channels_last')
    LR.assert_equal_exact(wt.grad.cpu().numpy(), dw, 'dkernel', 'kernel')
    LR.assert_equal_exact(bt.grad.cpu().numpy(), db, 'dbias', 'bias')


@pytest.mark.gpu
@pytest.mark.parametrize('planes', [False, True], ids=['x_channels_last', 'x_component_planes'])
@pytest.mark.parametrize('dtype', ['bf16', 'fp16'])
@pytest.mark.parametrize('shape,fq,per_row', [((2, 11, 33, 4), 32, False), ((3, 41, 50, 4), 16, True)],
                         ids=['11x33_one_slope', '41x50_f16_slope_per_row'])
def test_fused_first_layer_conv_prelu_pool_is_exact_on_the_integer_lattice(shape, fq, per_row, dtype, planes):
    """qk_conv_prelu_pool_fwd / _bwd: pooled values, dkernel, dbias and d alpha, slopes from {1/4, 1/2, 1, 2}."""
    import qcnn_amd
    Fq = qcnn_amd.functional
    dev = P._dev()
    dtype = DTYPES[dtype]
    rng, x, w, b = _first_layer_operands(shape, fq)
    H = shape[1]
    alpha = SLOPES[rng.randint(0, 4, size=H if per_row else 1)]
    a_b = alpha.reshape(1, -1, 1, 1)
    pre = oracle.forward(x, w, b, 2, padding='same', activation=None)
    act = np.maximum(pre, 0) + a_b * np.minimum(pre, 0)
    pooled, arg = P._np_pool_h_same(act)
    dp = LR.integer_lattice(rng, pooled.shape).astype(np.float64)
    dact = _route(pooled, arg, dp, act)
    dpre = dact * np.where(pre > 0, 1.0, np.where(pre < 0, a_b, 0.0))
    neg = dact * np.minimum(pre, 0)
    dalpha = neg.sum(axis=(0, 2, 3)) if per_row else neg.sum().reshape(1)
    _, dw, db = oracle.backward(x, w, b, dpre, 2, padding='same', activation=None)
    # preconditions: the pooled values survive the store; the fp32 sums stay below 2^24 units of 1/4 (the smallest slope)
    assert _survives_store(pooled, dtype)
    terms = LR.term_bounds(x, w, b, dpre, pre.size // (4 * fq))
    terms['dalpha'] = float(np.abs(neg).sum())
    LR.assert_preconditions(dict(dkernel=dw, dbias=db, dalpha=dalpha), dtype, unit=0.25, abs_terms=terms)
    xt = torch.tensor(x, device=dev).to(dtype)
    wt = torch.tensor(w, device=dev, dtype=torch.float32, requires_grad=True)
    bt = torch.tensor(b, device=dev, dtype=torch.float32, requires_grad=True)
    at = torch.tensor(alpha.reshape((1, H, 1) if per_row else (1, 1, 1)), device=dev, dtype=torch.float32, requires_grad=True)
    axis = 0 if per_row else -1
    lay = 'channels_last'
    if planes:
        xt, lay = xt.permute(0, 3, 1, 2).contiguous(), 'channels_first'
    assert Fq.conv_prelu_pool_supported(xt, wt, at, axis, 3, lay)
    out = Fq.conv_prelu_pool(xt, wt, bt, at, axis, 3, lay)
    out.backward(torch.tensor(dp, device=dev).to(dtype))
    LR.assert_equal_exact(out.detach().float().cpu().numpy(), pooled, 'pooled', 'channels_last')
    LR.assert_equal_exact(wt.grad.cpu().numpy(), dw, 'dkernel', 'kernel')
    LR.assert_equal_exact(bt.grad.cpu().numpy(), db, 'dbias', 'bias')
    LR.assert_equal_exact(at.grad.reshape(-1).cpu().numpy(), dalpha, 'd alpha')


# ---------------------------------------------------------------------------------------------------------------------
# 3e. many M splits and long lines: the body layers in the bench's pair of launches, sampled oracle, zero tolerance
# ---------------------------------------------------------------------------------------------------------------------
BODY_LATTICE = [
    # id, dtype, batch, cq, fq, kernel density (x and dy stay at 0.5)
    ('64to64_bf16', 'bf16', 8, 64, 64, 1.0 / 24),
    ('32to64_bf16', 'bf16', 8, 32, 64, 1.0 / 24),
    ('32to32_bf16', 'bf16', 8, 32, 32, 1.0 / 12),
    ('16to16_bf16', 'bf16', 8, 16, 16, 1.0 / 6),
    ('16to32_bf16', 'bf16', 8, 16, 32, 1.0 / 12),
    ('256to256_fp16', 'fp16', 2, 256, 256, 1.0 / 24),
]


def _body_operands(case):
    """Operands and the OPERAND-ONLY precondition (the full oracle is too slow here): max absolute column sum of the expanded
    kernel x max|x| + max|bias| bounds the integer part of y, max absolute row sum x max|dy| that of dx (the dropout scale 2 of
    either is a power of two); the fp32 gradients gather at most 4 M / M unit terms."""
    _, dt, batch, cq, fq, dens = case
    xs, ws = (batch, 14, 200, 4 * cq), (3, 5, cq, 4 * fq)
    rng = np.random.RandomState(SEED)
    x, w, b, dy = LR.layer_operands(rng, xs, ws, xs[:-1] + (4 * fq,), True, 'integer', kernel_density=dens)
    col, row = LR.expanded_kernel_sums(w)
    bounds = dict(y=col * float(np.abs(x).max()) + float(np.abs(b).max()), dx=row * float(np.abs(dy).max()))
    LR.assert_bounds_in_range(bounds, DTYPES[dt])
    m = int(np.prod(xs[:-1]))
    LR.assert_preconditions({}, DTYPES[dt], abs_terms=dict(dkernel=4.0 * m + 3, dbias=1.0 * m + 3))
    return xs, ws, x, w, b, dy, bounds


@pytest.mark.parametrize('case', BODY_LATTICE, ids=_ids(BODY_LATTICE))
def test_sampled_body_cases_lie_inside_the_exact_range(case):
    """CPU: the operand-only precondition of the sampled GPU cases, and that it is not vacuous (the bound is within a factor
    of four of the limit, so the sums the kernels form are long)."""
    bounds = _body_operands(case)[-1]
    print(case[0], bounds)
    assert max(bounds.values()) >= LR.exact_range(DTYPES[case[1]]) / 4


@pytest.mark.gpu
@pytest.mark.parametrize('case', BODY_LATTICE, ids=_ids(BODY_LATTICE))
def test_body_layer_in_the_bench_form_is_exact_at_sampled_positions(case):
    """qk_conv_fwd_post (relu + dropout 0.5) then qk_conv_bwd_post accumulating into integer pre-fills, M = 22 400 rows (5 600
    at K = 15 360 in fp16): many M splits of the backward-weight kernels, lines longer than a K step."""
    import qcnn_amd
    from qcnn_amd import _lib
    F = qcnn_amd.functional
    dev = P._dev()
    dtype = DTYPES[case[1]]
    xs, ws, x, w, b, dy, _ = _body_operands(case)
    seed = 0x5EED1234
    xt, dyt = torch.tensor(x, device=dev).to(dtype), torch.tensor(dy, device=dev).to(dtype)
    wt, bt = torch.tensor(w, device=dev), torch.tensor(b, device=dev)
    call = F.conv_call(xs, ws, dtype, 2, 1, 'same', 'channels_last', 1, None, True)
    pre, y = call.fwd_post(xt, wt, bt, F.PostOp(None, -1, RATE, seed))
    assert pre is None
    path_f = _lib.last_path()
    rng = np.random.RandomState(5)
    dw0 = torch.tensor(rng.randint(-3, 4, size=ws).astype(np.float32), device=dev)
    db0 = torch.tensor(rng.randint(-3, 4, size=ws[-1]).astype(np.float32), device=dev)
    dw, db = dw0.clone(), db0.clone()
    dx, _, _ = call.bwd_post(xt, dyt, wt, True, F.PostOp(None, -1, RATE, 1), None, None, direct=(dw, db))
    torch.cuda.synchronize()
    assert path_f.startswith('mfma16') and _lib.last_path().startswith('mfma16'), (path_f, _lib.last_path())
    chk = FS.LayerCheck(2, dict(padding='same'), x, w.astype(np.float64), b.astype(np.float64), FS._host(y), dy, FS._host(dx),
                        (dw - dw0).cpu().numpy(), (db - db0).cpu().numpy(), 'post', (seed, RATE), RATE)
    chk.check(np.random.RandomState(1), 0.0, 0.0)
