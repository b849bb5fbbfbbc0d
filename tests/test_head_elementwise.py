"""Element-wise parity of the model's head: the softmax output layer, its fallback kernels, the weighted-sum loss and the CTC cost.

The earlier tests of these kernels (tests/test_models.py, tests/test_ctc_enum.py) assert one norm-wise figure,
max |got - want| / max |want|.  d cost / d y_pred = (softmax(u) - occupancy) / (y_pred + 1e-7) spans five decades, so at the bf16
tolerance (1e-2) that figure looks at a few per cent of the gradient table; on the output layer it cannot see a tail row, a
two-column store at the width's edge or a lost K group in a row of small magnitude.  Here every output element is held to a bound
derived for THAT element from a float64 reference that rounds where the kernel rounds (tests/head_ref.py: the rounding points, the
terms of every bound, where the CTC margin M and e_fast are defined).

CPU tests (`-m "not gpu"`): a numpy emulation of each kernel's arithmetic (fp32 accumulation, the 16-bit rounding points) passes
its own bound on every input family and shape of the GPU tests -- no element excluded -- and each planted fault fails the checker;
for the faults marked (*) the old criterion is shown to accept them: the record of the gap.
GPU tests (`-m gpu`): every op through qcnn_amd.functional, fixed seeds; each prints its worst err / bound (`pytest -s`).
"""
import numpy as np
import pytest
import torch

import head_ref as H
from oracle import ctc_enum, ref_model

TORCH = {'fp32': torch.float32, 'bf16': torch.bfloat16, 'fp16': torch.float16}
KINDS16 = ['bf16', 'fp16']
KINDS = ['fp32', 'bf16', 'fp16']
CPU_LOOP_ROWS = 2048 + 21           # stands in for the two persistent-loop shapes on the CPU

# (rows, K, U); 'fwd_loop' = 64 * 2 * CUs + 21 rows (the forward's persistent waves take a second tile),
#               'bwd_loop' = 32 * CUs + 37 rows at K = 256 (one workgroup per CU: a second 32-row block)
OUT_SHAPES = ([(r, 64, u) for r in (1, 15, 16, 17) for u in (2, 62)]                                  # single wave tile edges
              + [(r, 128, u) for r in (31, 32, 33, 63, 65, 97) for u in (14, 16, 18)]                  # 32-row block, 64-row workgroup edges
              + [(97, 256, u) for u in (34, 48, 50, 62, 64)]                                           # column-tile edges
              + [('fwd_loop', 64, 62), ('bwd_loop', 256, 62)])


def _out_id(s):
    return '%sx%dx%d' % s


def _note(op, kind, ratio):
    print('head-elementwise worst err/bound: %-28s %-4s %.3f' % (op, kind, ratio))


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    return torch.device('cuda:0')


def _rows(rows, on_gpu):
    if not isinstance(rows, str):
        return rows
    if not on_gpu:
        return CPU_LOOP_ROWS
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    return 64 * 2 * cus + 21 if rows == 'fwd_loop' else 32 * cus + 37


def out_layer_inputs(rows, K, U, kind, use_bias):
    """x standard normal, kernel scaled so that the logits have a standard deviation of 2.5 (order 1 to 4), bias 0.5 randn, dy
    standard normal; y16 = round16(softmax64) -- the backward's operand does not depend on the forward kernel.  Prefills nonzero."""
    rng = np.random.RandomState((rows * 131 + K * 7 + U) % (2 ** 31))
    x16 = H.round16(rng.randn(rows, K), kind)
    w32 = (rng.randn(K, U) * (2.5 / np.sqrt(K))).astype(np.float32)
    b = (0.5 * rng.randn(U)).astype(np.float32)
    dy16 = H.round16(rng.randn(rows, U), kind)
    dk0 = rng.randn(K, U).astype(np.float32)
    db0 = rng.randn(U).astype(np.float32)
    bias = b if use_bias else None
    z = x16 @ H.round16(w32, kind) + (b.astype(np.float64) if use_bias else 0.0)
    y16 = H.round16(H.softmax64(z), kind)
    return dict(x=x16, w=w32, b=bias, dy=dy16, y=y16, dk0=dk0, db0=db0)


def _check_out_fwd(got, d, kind, what):
    ref, bound = H.dense_softmax_fwd_ref(d['x'], d['w'], d['b'], kind)
    return H.assert_within(got, ref, bound, (what + ' y', 'rows'))


def _check_out_bwd(got, d, kind, what, prefilled=True, **scale):
    refs = H.dense_softmax_bwd_ref(d['x'], d['w'], d['y'], d['dy'], kind, dkernel0=d['dk0'] if prefilled else None,
                                   dbias0=d['db0'] if prefilled else None, **scale)
    out = {}
    for k in got:
        g = got[k].reshape(refs[k][0].shape)
        out[k] = H.assert_within(g, refs[k][0], refs[k][1], ('%s %s' % (what, k), 'rows'))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# CTC inputs
# ---------------------------------------------------------------------------------------------------------------------
CTC_SHAPES = [(3, 9, 2, 4),          # smallest: blank plus one label, repeats only
              (4, 24, 6, 11),        # one wave of states
              (4, 80, 20, 31),       # S = 63
              (4, 80, 20, 32),       # S = 65: the wave edge of the occupancy reduce
              (3, 140, 20, 127),     # S = 255, the launcher's limit
              (3, 70, 256, 9),       # C = 256, the limit; the table does not fit 64 KB under two-sweeps
              (3, 80, 256, 9),       # too large for the fast form by default
              (4, 1, 6, 1),          # T = 1 and input_length 0
              (5, 200, 62, 50)]      # the model's own width, ragged
CTC_BATCH = (256, 200, 62, 50)
# By launch_ctc's arithmetic neither the fast form ((320 + 5 * 13 + 4 + 2 * 320 * 62) * 4 = 160 276 bytes > 150 KB) nor the table form
# ((320 + 4 * 13 + 2 * 62 + 4) * 4 + 320 * 62 * 4 = 81 376 bytes > 64 KB) takes it: the two-sweep kernel that gathers its emissions
# from global memory, with default flags.  Two samples only (see ctc_inputs), so it is not one of CTC_SHAPES.
CTC_FROM_GLOBAL = (2, 320, 62, 6)
FAMILIES = ['diffuse', 'peaked']
_CTC_IN, _CTC_REF = {}, {}


def _need(labels):
    """Frames a labelling needs: its labels plus one blank between equal neighbours."""
    labels = list(labels)
    return len(labels) + sum(1 for a, b in zip(labels, labels[1:]) if a == b)


def _alignment(rng, labels, frames, blank):
    """A random frame-level path of `frames` symbols that collapses to `labels` (needs _need(labels) <= frames)."""
    path = []
    for i, c in enumerate(labels):
        if i and labels[i - 1] == c:
            path.append(blank)
        path.append(int(c))
    if not path:
        return [blank] * frames
    reps = 1 + rng.multinomial(frames - len(path), np.ones(len(path)) / len(path))
    return [c for c, n in zip(path, reps) for _ in range(n)]


def ctc_inputs(shape, family):
    """(p64 (B, T, C), labels, input_length, label_length), read-only.  B = 2: sample 0 feasible with a repeated label and an
    input_length below T, sample 1 infeasible.  Otherwise sample 0 at full length (T frames, Lmax labels) with a repeated
    label; sample 1 without labels; sample 2 infeasible (fewer frames than labels); the others ragged with a repeat.  T = 1: samples
    2 and 3 have input_length 0 (with and without a label).  p = 0.98 softmax(logits) + 0.02 / C, so |g| <= 1 / p <= 50 C;
    'diffuse': logits = 2 randn; 'peaked': the same raised by 4 along a random valid alignment of each feasible sample."""
    key = (shape, family)
    if key in _CTC_IN:
        return _CTC_IN[key]
    B, T, C, Lmax = shape
    rng = np.random.RandomState(T * 1009 + C * 31 + Lmax + B)
    blank = C - 1
    labels = np.zeros((B, Lmax), dtype=np.int64)
    for b in range(B):
        for i in range(Lmax):
            c = rng.randint(0, C - 1)
            while C > 2 and i and c == labels[b, i - 1]:
                c = rng.randint(0, C - 1)
            labels[b, i] = c
    il = np.zeros(B, dtype=np.int64)
    ll = np.zeros(B, dtype=np.int64)
    if T == 1:
        il[:], ll[:] = [1, 1, 0, 0][:B], [1, 0, 1, 0][:B]
    elif B == 2:
        ll[:] = Lmax
        labels[0, 1] = labels[0, 0]
        il[:] = rng.randint(T // 2, T), max(1, Lmax // 2)
    else:
        for b in range(B):
            if b == 0:
                ll[b] = Lmax
                if Lmax >= 2 and Lmax + 1 <= T:
                    labels[b, 1] = labels[b, 0]
                il[b] = T
            elif b == 1:
                ll[b], il[b] = 0, rng.randint(T // 2, T)
            elif b == 2:
                ll[b], il[b] = Lmax, max(1, Lmax // 2)
            else:
                ll[b] = rng.randint(2, Lmax + 1) if Lmax >= 2 else Lmax
                k = rng.randint(1, ll[b])
                labels[b, k] = labels[b, k - 1]
                il[b] = rng.randint(_need(labels[b, :ll[b]]), T + 1)
    feasible = np.array([_need(labels[b, :ll[b]]) <= il[b] for b in range(B)])
    if B == 2:
        assert feasible[0] and not feasible[1] and il[0] < T and _need(labels[0, :ll[0]]) > ll[0]
    elif T > 1:
        assert feasible[0] and feasible[1] and not feasible[2] and feasible[3:].all() and il[0] == T and ll[0] == Lmax
        assert _need(labels[0, :ll[0]]) > ll[0]                        # sample 0 does hold a repeated label
    logits = 2.0 * rng.randn(B, T, C)
    if family == 'peaked':
        for b in np.nonzero(feasible)[0]:
            path = _alignment(rng, labels[b, :ll[b]], int(il[b]), blank)
            assert ctc_enum.collapse(path, blank) == tuple(labels[b, :ll[b]]) and len(path) == il[b]
            logits[b, np.arange(il[b]), path] += 4.0
    p = 0.98 * H.softmax64(logits) + 0.02 / C
    for a in (p, labels, il, ll):
        a.flags.writeable = False
    _CTC_IN[key] = (p, labels, il, ll)
    return _CTC_IN[key]


def ctc_reference(shape, family, kind):
    """The posteriors as the kernel reads them (rounded to `kind`) and head_ref.ctc_ref on them; computed once, shared, read-only."""
    key = (shape, family, kind)
    if key not in _CTC_REF:
        p, labels, il, ll = ctc_inputs(shape, family)
        pk = H.round16(p, kind)
        ref = H.ctc_ref(pk, labels, il, ll, kind)
        ref['pred'] = pk
        ref['label_mask'] = H.ctc_label_mask(labels, ll, shape[2])
        for v in (pk, ref['g'][0], ref['g'][1], ref['cost'][0], ref['cost'][1]):
            v.flags.writeable = False
        _CTC_REF[key] = ref
    return _CTC_REF[key]


def _check_ctc(cost, g, ref, what):
    """Cost and every gradient entry against their bounds; bound 0 (frames past input_length, infeasible samples) means EXACTLY zero."""
    rc = H.assert_within(cost, ref['cost'][0], ref['cost'][1], (what + ' cost', 'plain'))
    rg = H.assert_within(g, ref['g'][0], ref['g'][1], (what + ' gradient', 'ctc'), labels=ref['label_mask'])
    assert np.all(np.asarray(g)[~ref['live']] == 0.0), what + ': a frame past input_length or an infeasible sample is not exactly zero'
    return rc, rg


def _row_sum_check(g, pred, ref, kind, what):
    """Reference-free: soft and the occupancies of a live frame both sum to 1, so sum_c g[t, c] (p[t, c] + 1e-7) = 0 up to the sum
    over the frame's classes of bound_g * pc = half_ulp(g) pc + M delta + 2^-22 (head_ref.ctc_ref), with the kernel's OWN g in the first term."""
    C = g.shape[2]
    pc = pred + H.CTC_EPS
    s = np.abs((g * pc).sum(axis=2))
    store = 0.0 if kind == 'fp32' else H.half_ulp(g, kind) * (g != 0.0)
    tol = (store * pc).sum(axis=2) + C * (H.CTC_MARGIN * ref['delta'] + 2.0 ** -22)
    live = ref['live'][:, :, 0]
    worst = float((s[live] / tol[live]).max()) if live.any() else 0.0
    assert worst <= 1.0, '%s: |sum_c g (p + eps)| / bound = %.3g at (sample, frame) %s' % (
        what, worst, np.unravel_index(int(np.argmax(np.where(live, s / tol, 0))), s.shape))
    return worst


# =====================================================================================================================
# CPU tests
# =====================================================================================================================
def test_round16_is_one_round_to_nearest_even():
    rng = np.random.RandomState(0)
    v = np.concatenate([rng.randn(4000) * 10.0 ** rng.randint(-9, 5, 4000), [0.0, 65504.0, 65519.9, 65520.0, 2.0 ** -24, 2.0 ** -25, 3 * 2.0 ** -25,
                                                                           1.00390625, 1.01171875, 1.00048828125]]).astype(np.float32)
    for kind in KINDS16:
        want = torch.from_numpy(v).to(TORCH[kind]).double().numpy()           # float32 -> 16 bits: one rounding, ties to even
        got = H.round16(v.astype(np.float64), kind)
        assert np.array_equal(got, want), kind
        q = H.ulp16(want[np.isfinite(want)], kind)
        assert np.array_equal(H.round16(want[np.isfinite(want)] + 0.25 * q, kind), want[np.isfinite(want)])
    # from float64 the rounding is ONE step: a value just above a bf16 tie that float32 would round onto the tie
    tie = 1.0 + 2.0 ** -8
    assert H.round16(tie + 2.0 ** -40, 'bf16') == 1.0 + 2.0 ** -7 and H.round16(tie, 'bf16') == 1.0


def test_ctc_recursion_equals_the_enumeration_and_the_keras_restatement():
    """head_ref.ctc_recursion (float64) against oracle/ctc_enum.py (every alignment enumerated) and, cost and gradient, against
    oracle/ref_model.ctc_cost (torch.ctc_loss behind the Keras recipe) on a ragged case with repeats -- two independent definitions."""
    for name, y, labels, il, ll in ctc_enum.tiny_cases():
        want = ctc_enum.ctc_cost_enum(y, labels, il, ll)[:, 0]
        got = H.ctc_recursion(y, labels, il, ll)['cost']
        assert np.array_equal(np.isfinite(got), np.isfinite(want)), name
        f = np.isfinite(want)
        assert np.abs(got[f] - want[f]).max() <= 1e-12 * max(1.0, np.abs(want[f]).max()), name
    for shape in ((4, 24, 6, 11), (4, 80, 20, 32)):
        p, labels, il, ll = ctc_inputs(shape, 'peaked')
        r = H.ctc_recursion(p, labels, il, ll)
        pt = torch.tensor(p, dtype=torch.float64, requires_grad=True)
        cost = ref_model.ctc_cost(pt, torch.tensor(labels), torch.tensor(il), torch.tensor(ll))
        f = r['feasible']
        assert np.array_equal(np.isfinite(cost.detach().numpy()), f)
        assert np.abs(cost.detach().numpy()[f] - r['cost'][f]).max() <= 1e-10
        cost[torch.tensor(f)].sum().backward()
        assert np.abs(pt.grad.numpy()[f] - r['g'][f]).max() <= 1e-9 * np.abs(r['g']).max()
        for b in np.nonzero(f)[0]:                                             # the occupancies of a live frame sum to 1
            assert np.abs(r['occ'][b, :il[b]].sum(-1) - 1.0).max() <= 1e-12


@pytest.mark.parametrize('kind', KINDS16)
@pytest.mark.parametrize('shape', OUT_SHAPES, ids=_out_id)
def test_output_layer_emulation_is_within_its_own_bound(shape, kind):
    rows, K, U = _rows(shape[0], False), shape[1], shape[2]
    for use_bias in (True, False):
        d = out_layer_inputs(rows, K, U, kind, use_bias)
        what = 'emulated %dx%dx%d %s bias=%s' % (rows, K, U, kind, use_bias)
        _check_out_fwd(H.emulate_dense_softmax_fwd(d['x'], d['w'], d['b'], kind), d, kind, what)
        got = H.emulate_dense_softmax_bwd(d['x'], d['w'], d['y'], d['dy'], kind, dkernel0=d['dk0'], dbias0=d['db0'])
        _check_out_bwd(got, d, kind, what)
    for scale in (dict(dy_scale=0.37), dict(dy_scale=1.0 / 256, dy_scale_dev=1536.0)):
        got = H.emulate_dense_softmax_bwd(d['x'], d['w'], d['y'], d['dy'], kind, dkernel0=d['dk0'], dbias0=d['db0'], **scale)
        _check_out_bwd(got, d, kind, what + ' %s' % scale, **scale)


@pytest.mark.parametrize('kind', KINDS16)
def test_fallback_composition_emulation_is_within_its_own_bound(kind):
    """The odd width of the layers._DenseSoftmaxFn fallback (U = 61) with gradient buffers that start at zero, as autograd hands them."""
    d = out_layer_inputs(CPU_LOOP_ROWS, 256, 61, kind, True)
    what = 'emulated fallback %dx256x61 %s' % (CPU_LOOP_ROWS, kind)
    _check_out_fwd(H.emulate_dense_softmax_fwd(d['x'], d['w'], d['b'], kind), d, kind, what)
    _check_out_bwd(H.emulate_dense_softmax_bwd(d['x'], d['w'], d['y'], d['dy'], kind), d, kind, what, prefilled=False)


SM_COLS = (1, 2, 31, 32, 33, 62, 63, 64)
SM_ROWS = (1, 3, 4, 5, 1027)
SM_LAP_ROWS = 4 * 8192 + 5      # launch_softmax_rows: at most 2048 workgroups forward (8192 waves, one row each per lap) and 512 backward
#                                 (2048 waves x 4 rows per lap): past 32 768 rows both grids are capped and every wave loops again


def softmax_rows_inputs(rows, cols, kind):
    rng = np.random.RandomState(rows * 67 + cols)
    logits = (2.5 * rng.randn(rows, cols)).astype(np.float32)
    bias = (0.5 * rng.randn(cols)).astype(np.float32)
    y = H.round16(H.softmax64(logits.astype(np.float64) + bias), kind)
    dy = H.round16(rng.randn(rows, cols), kind)
    return dict(logits=logits, bias=bias, y=y, dy=dy, db0=rng.randn(cols).astype(np.float32))


def _check_softmax_rows(fwd, bwd, d, kind, what, bias=True):
    out = {}
    if fwd is not None:
        ref, bound = H.softmax_rows_fwd_ref(d['logits'], d['bias'] if bias else None, kind)
        out['y'] = H.assert_within(fwd, ref, bound, (what + ' y', 'rows'))
    if bwd is not None:
        refs = H.softmax_rows_bwd_ref(d['y'], d['dy'], kind, dbias0=d['db0'])
        for k in ('dlogits', 'dbias'):
            out[k] = H.assert_within(bwd[k], refs[k][0], refs[k][1], ('%s %s' % (what, k), 'rows'))
    return out


@pytest.mark.parametrize('kind', KINDS)
def test_softmax_rows_emulation_is_within_its_own_bound(kind):
    for rows, cols in [(r, c) for r in SM_ROWS for c in SM_COLS] + [(CPU_LOOP_ROWS, 62)]:
        d = softmax_rows_inputs(rows, cols, kind)
        _check_softmax_rows(H.emulate_softmax_rows_fwd(d['logits'], d['bias'], kind),
                            H.emulate_softmax_rows_bwd(d['y'], d['dy'], kind, dbias0=d['db0']), d, kind, 'emulated %dx%d %s' % (rows, cols, kind))
        _check_softmax_rows(H.emulate_softmax_rows_fwd(d['logits'], None, kind), None, d, kind, 'emulated %dx%d %s no bias' % (rows, cols, kind), bias=False)


WS_N = (1, 255, 257, 65539)


def weighted_sum_inputs(n, kind):
    rng = np.random.RandomState(n)
    return H.round16(rng.randn(n), kind), rng.randn(n).astype(np.float32), float(np.float32(rng.randn() * 3.0))


@pytest.mark.parametrize('kind', KINDS)
def test_weighted_sum_emulation_is_within_its_own_bound(kind):
    for n in WS_N:
        a, w, out0 = weighted_sum_inputs(n, kind)
        ref, bound = H.weighted_sum_ref(a, w, out0)
        H.assert_within(np.array([H.emulate_weighted_sum(a, w, out0)]), np.array([ref]), np.array([bound]), ('emulated weighted_sum n=%d' % n, 'plain'))


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('family', FAMILIES)
@pytest.mark.parametrize('shape', CTC_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_ctc_float32_recursion_is_within_its_own_bound(shape, family, kind):
    """The float32 run of the recursion, its gradient rounded to the output type, passes the bound of the float64 reference (margin
    M against a deviation of 1 delta by construction); every fp16 case keeps the reference inside fp16's range."""
    ref = ctc_reference(shape, family, kind)
    p, labels, il, ll = ctc_inputs(shape, family)
    r32 = H.ctc_recursion(ref['pred'], labels, il, ll, np.float32)
    _check_ctc(r32['cost'].astype(np.float64), H.round16(r32['g'].astype(np.float64), kind), ref, 'float32 recursion %s %s %s' % (shape, family, kind))
    assert np.abs(ref['g'][0]).max() < 3e4 and np.abs(ref['g'][0]).max() <= 50.0 * shape[2] * (1 + 2.0 ** -8)
    c = ref['cost'][0]
    if shape[1] > 1:
        assert np.isfinite(c[0]) and np.isfinite(c[1]) and np.isinf(c[2]) and c[2] > 0 and np.all(ref['g'][0][2] == 0.0)
    else:
        assert np.isfinite(c[0]) and np.isfinite(c[1]) and np.isinf(c[2]) and c[3] == 0.0


# ---- planted faults ---------------------------------------------------------------------------------------------------
OLD_TOL = dict(ctc_g=dict(bf16=1e-2), y=dict(bf16=8e-3, fp16=1e-3), dx=dict(bf16=2e-2, fp16=4e-3))     # tests/test_models.py, tests/test_ctc_enum.py


def _rejected(got, ref, bound, names, **kw):
    with pytest.raises(AssertionError) as e:
        H.assert_within(got, ref, bound, names, **kw)
    return str(e.value)


def test_planted_ctc_faults_are_rejected_and_two_pass_the_old_criterion():
    kind = 'bf16'
    shape = CTC_SHAPES[-1]
    for family in FAMILIES:
        ref = ctc_reference(shape, family, kind)
        p, labels, il, ll = ctc_inputs(shape, family)
        g_ref, bound = ref['g']
        clean = H.round16(g_ref, kind)
        H.assert_within(clean, g_ref, bound, ('clean', 'ctc'))
        # (*) every non-label, non-blank class of ONE frame set to 0 (the frame whose largest such posterior is largest)
        b = 3
        other = ~ref['label_mask'][b]
        other[-1] = False
        t = int(np.argmax(ref['pred'][b, :il[b]][:, other].max(axis=1)))
        bad = clean.copy()
        bad[b, t, other] = 0.0
        msg = _rejected(bad, g_ref, bound, ('planted', 'ctc'), labels=ref['label_mask'])
        assert 'sample 3, frame %d' % t in msg and 'no label' in msg, msg
        assert H.old_criterion(bad, g_ref) <= OLD_TOL['ctc_g'][kind]
        # the frame at input_length - 1 copied from the frame before it
        b = 4
        bad = clean.copy()
        bad[b, il[b] - 1] = bad[b, il[b] - 2]
        msg = _rejected(bad, g_ref, bound, ('planted', 'ctc'), labels=ref['label_mask'])
        assert 'sample 4, frame %d' % (il[b] - 1) in msg, msg
    # (*) the occupancy of the states at index 64 and above dropped, L = 40 (S = 81: a second wave of states).  Three frames per label,
    # the posteriors peaked along that alignment; the MIDDLE frame of the first two labels all but denies its label (nothing else can
    # take a run's middle frame: occupancy 1 over a posterior at the floor), which sets max |g| ~ 1 / floor in the first wave of
    # states -- the old figure is blind to everything two decades below that, a lost second wave included
    rng = np.random.RandomState(5)
    T, C, L = 120, 62, 40
    labels = np.zeros((1, L), dtype=np.int64)
    for i in range(L):
        labels[0, i] = (labels[0, i - 1] + 1 + rng.randint(0, C - 2)) % (C - 1) if i else rng.randint(0, C - 1)
    path = np.repeat(labels[0], 3)
    logits = 2.0 * rng.randn(1, T, C)
    logits[0, np.arange(T), path] += 12.0
    logits[0, [1, 4], path[[1, 4]]] = -12.0
    pk = H.round16(0.98 * H.softmax64(logits) + 0.02 / C, kind)
    ref = H.ctc_ref(pk, labels, [T], [L], kind)
    H.assert_within(H.round16(ref['g'][0], kind), ref['g'][0], ref['g'][1], ('clean', 'ctc'))
    bad = H.round16(H.ctc_recursion(pk, labels, [T], [L], occ_states=64)['g'], kind)
    msg = _rejected(bad, ref['g'][0], ref['g'][1], ('planted', 'ctc'), labels=H.ctc_label_mask(labels, [L], C))
    assert 'a label' in msg or 'blank' in msg, msg
    assert H.old_criterion(bad, ref['g'][0]) <= OLD_TOL['ctc_g'][kind]


def test_planted_output_layer_faults_are_rejected_and_two_pass_the_old_criterion():
    rows, K, U = CPU_LOOP_ROWS, 64, 62
    for kind in KINDS16:
        d = out_layer_inputs(rows, K, U, kind, True)
        y_ref, y_bound = H.dense_softmax_fwd_ref(d['x'], d['w'], d['b'], kind)
        clean = H.round16(y_ref, kind)
        H.assert_within(clean, y_ref, y_bound, ('clean y', 'rows'))
        # (*) one element of the last, partial 16-row tile moved by two 16-bit ulps
        r, c = rows - 1, int(np.argsort(clean[rows - 1])[U // 2])
        bad = clean.copy()
        bad[r, c] += 2.0 * H.ulp16(bad[r, c], kind)
        msg = _rejected(bad, y_ref, y_bound, ('planted y', 'rows'))
        assert 'row %d, column %d (16-row tile %d' % (r, c, r // 16) in msg, msg
        assert H.old_criterion(bad, y_ref) <= OLD_TOL['y'][kind]
        # columns U - 2 and U - 1 swapped in one row
        bad = clean.copy()
        bad[rows - 7, [U - 2, U - 1]] = bad[rows - 7, [U - 1, U - 2]]
        assert 'row %d, column' % (rows - 7) in _rejected(bad, y_ref, y_bound, ('planted y', 'rows'))

        refs = H.dense_softmax_bwd_ref(d['x'], d['w'], d['y'], d['dy'], kind, dkernel0=d['dk0'], dbias0=d['db0'])
        got = H.emulate_dense_softmax_bwd(d['x'], d['w'], d['y'], d['dy'], kind, dkernel0=d['dk0'], dbias0=d['db0'])
        dl = H.emulate_dl(d['y'], d['dy'], 1.0, kind)
        w16 = H.round16(d['w'], kind)
        # (*) dx: one K group of 8 (logit columns 8 .. 15 of the product dl W^T) missing from one row whose |dx| is below 1 % of the largest
        dx_ref, dx_bound = refs['dx']
        r = int(np.argmin(np.abs(dx_ref).max(axis=1)))
        assert np.abs(dx_ref[r]).max() < 0.01 * np.abs(dx_ref).max()
        bad = got['dx'].copy()
        keep = np.ones(U, dtype=bool)
        keep[8:16] = False
        bad[r] = H.round16(dl[r, keep] @ w16[:, keep].T, kind)
        assert 'row %d,' % r in _rejected(bad, dx_ref, dx_bound, ('planted dx', 'rows'))
        assert H.old_criterion(bad, dx_ref) <= OLD_TOL['dx'][kind]
        # dW: the last, partial 32-row block left out
        full = (rows // 32) * 32
        bad = d['dk0'].astype(np.float64) + d['x'][:full].T @ dl[:full]
        _rejected(bad, refs['dkernel'][0], refs['dkernel'][1], ('planted dkernel', 'rows'))
        # dbias: the prefill overwritten instead of added to
        _rejected(dl.sum(axis=0), refs['dbias'][0], refs['dbias'][1], ('planted dbias', 'plain'))


# =====================================================================================================================
# GPU tests
# =====================================================================================================================
def _dev(a, kind, dev):
    return torch.from_numpy(np.array(a)).to(TORCH[kind]).to(dev)                # (a copy: the shared references are read-only)


def _host(t):
    return t.detach().double().cpu().numpy()


def _run_out_bwd(Fq, d, kind, dev, grads=True, **scale):
    dk = _dev(d['dk0'], 'fp32', dev) if grads else None
    db = _dev(d['db0'], 'fp32', dev) if grads else None
    kw = dict(scale)
    if 'dy_scale_dev' in kw:
        kw['dy_scale_dev'] = torch.tensor([kw['dy_scale_dev']], dtype=torch.float32, device=dev)
    dx = Fq.dense_softmax_bwd(_dev(d['x'], kind, dev), _dev(d['w'], 'fp32', dev), _dev(d['y'], kind, dev), _dev(d['dy'], kind, dev), dk, db, **kw)
    torch.cuda.synchronize()
    got = dict(dx=_host(dx))
    if grads:
        got.update(dkernel=_host(dk), dbias=_host(db))
    return got


@pytest.mark.gpu
@pytest.mark.parametrize('kind', KINDS16)
@pytest.mark.parametrize('shape', OUT_SHAPES, ids=_out_id)
def test_output_layer_kernels_elementwise(shape, kind):
    """qk_dense_softmax_fwd / _bwd at the tile edges of csrc/qk_out_layer.hip, with and without bias: y, dx, dkernel and dbias
    (both prefilled) element by element."""
    dev = _need_gpu()
    from qcnn_amd import functional as Fq
    rows, K, U = _rows(shape[0], True), shape[1], shape[2]
    for use_bias in (True, False):
        d = out_layer_inputs(rows, K, U, kind, use_bias)
        what = '%dx%dx%d %s bias=%s' % (rows, K, U, kind, use_bias)
        x = _dev(d['x'], kind, dev)
        assert Fq.dense_softmax_supported(x, U)
        y = Fq.dense_softmax_fwd(x, _dev(d['w'], 'fp32', dev), _dev(d['b'], 'fp32', dev) if use_bias else None)
        torch.cuda.synchronize()
        _note('dense_softmax_fwd y', kind, _check_out_fwd(_host(y), d, kind, what))
        for k, v in _check_out_bwd(_run_out_bwd(Fq, d, kind, dev), d, kind, what).items():
            _note('dense_softmax_bwd ' + k, kind, v)


@pytest.mark.gpu
@pytest.mark.parametrize('kind', KINDS16)
def test_output_layer_backward_scales_and_absent_gradients(kind):
    """dy_scale != 1, a device scale times a host factor, and dkernel / dbias absent (no slab reduction): dx must not change."""
    dev = _need_gpu()
    from qcnn_amd import functional as Fq
    d = out_layer_inputs(97, 256, 62, kind, True)
    for scale in (dict(dy_scale=0.37), dict(dy_scale=1.0 / 256, dy_scale_dev=1536.0)):
        for k, v in _check_out_bwd(_run_out_bwd(Fq, d, kind, dev, **scale), d, kind, '97x256x62 %s %s' % (kind, scale), **scale).items():
            _note('dense_softmax_bwd scaled ' + k, kind, v)
    got = _run_out_bwd(Fq, d, kind, dev, grads=False)
    _note('dense_softmax_bwd dx only', kind, _check_out_bwd(got, d, kind, '97x256x62 %s no gradients' % kind)['dx'])


@pytest.mark.gpu
@pytest.mark.parametrize('kind', KINDS)
def test_softmax_rows_kernels_elementwise(kind):
    """qk_softmax_rows_fwd / _bwd (the fallback of layers._DenseSoftmaxFn; no other test launches them): every width edge of the
    one-wave-per-row layout, the four-rows-per-wave tail of the backward, a capped grid, dbias prefilled and accumulated."""
    dev = _need_gpu()
    from qcnn_amd import functional as Fq
    worst = {}
    for rows, cols in [(r, c) for r in SM_ROWS for c in SM_COLS] + [(SM_LAP_ROWS, 62)]:
        d = softmax_rows_inputs(rows, cols, kind)
        what = '%dx%d %s' % (rows, cols, kind)
        lg, bs = _dev(d['logits'], 'fp32', dev), _dev(d['bias'], 'fp32', dev)
        y = Fq.softmax_rows_fwd(lg, bs, TORCH[kind])
        y0 = Fq.softmax_rows_fwd(lg, None, TORCH[kind])
        db = _dev(d['db0'], 'fp32', dev)
        dl = Fq.softmax_rows_bwd(_dev(d['y'], kind, dev), _dev(d['dy'], kind, dev), db)
        torch.cuda.synchronize()
        out = _check_softmax_rows(_host(y), dict(dlogits=_host(dl), dbias=_host(db)), d, kind, what)
        out['y no bias'] = _check_softmax_rows(_host(y0), None, d, kind, what + ' no bias', bias=False)['y']
        for k, v in out.items():
            worst[k] = max(worst.get(k, 0.0), v)
    for k, v in worst.items():
        _note('softmax_rows ' + k, kind, v)


@pytest.mark.gpu
def test_dense_softmax_fallback_composition_elementwise(monkeypatch):
    """layers.Dense(61, activation='softmax') on 8192 bf16 rows of width 256: an odd width, so layers._DenseSoftmaxFn composes a
    library GEMM with fp32 logits and qk_softmax_rows_fwd / _bwd.  y and the three gradients against float64 with the composition's
    rounding points (16-bit kernel image, fp32 logits, 16-bit d logits; the backward's y is the forward's own output)."""
    dev = _need_gpu()
    from qcnn_amd import functional as Fq
    from qcnn_amd.layers import Dense
    kind, rows, K, U = 'bf16', 8192, 256, 61
    d = out_layer_inputs(rows, K, U, kind, True)
    calls = []
    for name in ('softmax_rows_fwd', 'softmax_rows_bwd'):
        monkeypatch.setattr(Fq, name, (lambda f, n: lambda *a, **k: (calls.append(n), f(*a, **k))[1])(getattr(Fq, name), name))
    np.random.seed(3)
    layer = Dense(U, activation='softmax', kernel_initializer='random_uniform')
    layer._build_device = dev
    layer.build((None, K))
    with torch.no_grad():
        layer.kernel.copy_(_dev(d['w'], 'fp32', dev))
        layer.bias.copy_(_dev(d['b'], 'fp32', dev))
    x = _dev(d['x'], kind, dev).requires_grad_(True)
    assert not Fq.dense_softmax_supported(x, U)
    y = layer(x)
    y.backward(_dev(d['dy'], kind, dev))
    torch.cuda.synchronize()
    assert calls == ['softmax_rows_fwd', 'softmax_rows_bwd'], calls
    what = 'Dense(61) fallback 8192x256 bf16'
    _note('fallback y', kind, _check_out_fwd(_host(y), d, kind, what))
    d2 = dict(d, y=_host(y))
    got = dict(dx=_host(x.grad), dkernel=_host(layer.kernel.grad), dbias=_host(layer.bias.grad))
    for k, v in _check_out_bwd(got, d2, kind, what, prefilled=False).items():
        _note('fallback ' + k, kind, v)


@pytest.mark.gpu
@pytest.mark.parametrize('kind', KINDS)
def test_weighted_sum_kernel_elementwise(kind):
    """qk_weighted_sum ADDS to *out: through the C-ABI with `out` prefilled, and through functional.weighted_sum (out = 0)."""
    dev = _need_gpu()
    from qcnn_amd import functional as Fq
    worst = 0.0
    for n in WS_N:
        a, w, out0 = weighted_sum_inputs(n, kind)
        ad, wd = _dev(a, kind, dev), _dev(w, 'fp32', dev)
        out = torch.tensor([out0], dtype=torch.float32, device=dev)
        with Fq._on_device(dev):
            rc = Fq.L.lib().qk_weighted_sum(Fq._DTYPES[TORCH[kind]], n, Fq._ptr(ad), Fq._ptr(wd), Fq._ptr(out), Fq._stream(ad))
        Fq.L.check(rc, 'qk_weighted_sum')
        plain = Fq.weighted_sum(ad, wd)
        torch.cuda.synchronize()
        for got, o0 in ((out, out0), (plain, 0.0)):
            ref, bound = H.weighted_sum_ref(a, w, o0)
            worst = max(worst, H.assert_within(_host(got).reshape(1), np.array([ref]), np.array([bound]), ('weighted_sum n=%d %s out0=%g' % (n, kind, o0), 'plain')))
    _note('weighted_sum', kind, worst)


def _ctc_forms():
    from qcnn_amd import _lib
    return (('default', 0), ('two_sweeps', _lib.QK_DBG_CTC_TWO_SWEEPS), ('default_det', _lib.QK_DBG_DETERMINISTIC),
            ('two_sweeps_det', _lib.QK_DBG_CTC_TWO_SWEEPS | _lib.QK_DBG_DETERMINISTIC))


def _run_ctc(Fq, pred, labels, il, ll, kind, dev, flags):
    from qcnn_amd import _lib
    pd = _dev(pred, kind, dev)
    lab = torch.from_numpy(np.array(labels))
    assert Fq.ctc_supported(pd, lab)
    with _lib.debug_flags(flags):
        cost, g = Fq.ctc_cost_and_grad(pd, lab, torch.from_numpy(np.array(il)), torch.from_numpy(np.array(ll)))
        torch.cuda.synchronize()
    return _host(cost), _host(g)


@pytest.mark.gpu
@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('family', FAMILIES)
@pytest.mark.parametrize('shape', CTC_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_ctc_kernels_elementwise(shape, family, kind):
    """qk_ctc_batch_cost through functional.ctc_cost_and_grad (the kernel's stored cost and gradient, no autograd product), in its
    four forms: cost and EVERY gradient entry against the bound of head_ref.ctc_ref (M = 8), frames at and past input_length and
    infeasible samples exactly zero; on the model's own width also the reference-free row sums."""
    dev = _need_gpu()
    from qcnn_amd import functional as Fq
    ref = ctc_reference(shape, family, kind)
    p, labels, il, ll = ctc_inputs(shape, family)
    for form, flags in _ctc_forms():
        what = 'ctc %s %s %s %s' % ('x'.join(map(str, shape)), family, kind, form)
        cost, g = _run_ctc(Fq, ref['pred'], labels, il, ll, kind, dev, flags)
        rc, rg = _check_ctc(cost, g, ref, what)
        _note('ctc cost (%s)' % form, kind, rc)
        _note('ctc gradient (%s)' % form, kind, rg)
        if shape == CTC_SHAPES[-1]:
            _note('ctc row sums (%s)' % form, kind, _row_sum_check(g, ref['pred'], ref, kind, what))


@pytest.mark.gpu
@pytest.mark.parametrize('kind', KINDS)
def test_ctc_two_sweep_kernel_with_emissions_from_global_memory(kind):
    """The form no shape of CTC_SHAPES selects with default flags: k_ctc<T, false>, whose phase 0 forms log(p + eps) from global
    memory on both passes of the normaliser and whose sweeps gather every emission one frame ahead.  Reference and bounds as in
    test_ctc_kernels_elementwise; one sample ends before T, the other is infeasible."""
    dev = _need_gpu()
    from qcnn_amd import functional as Fq
    shape, family = CTC_FROM_GLOBAL, 'diffuse'
    B, T, C, Lmax = shape
    S = 2 * Lmax + 1
    assert (T + 5 * S + 4 + 2 * T * C) * 4 > 150 * 1024 and (T + 4 * S + 2 * C + 4) * 4 + T * C * 4 > 64 * 1024
    ref = ctc_reference(shape, family, kind)
    p, labels, il, ll = ctc_inputs(shape, family)
    assert il[0] < T and np.isfinite(ref['cost'][0][0]) and np.isinf(ref['cost'][0][1]) and np.all(ref['g'][0][1] == 0.0)
    for form, flags in _ctc_forms():
        what = 'ctc %s %s %s %s' % ('x'.join(map(str, shape)), family, kind, form)
        cost, g = _run_ctc(Fq, ref['pred'], labels, il, ll, kind, dev, flags)
        rc, rg = _check_ctc(cost, g, ref, what)
        _note('ctc from global cost (%s)' % form, kind, rc)
        _note('ctc from global gradient (%s)' % form, kind, rg)
        _note('ctc from global row sums (%s)' % form, kind, _row_sum_check(g, ref['pred'], ref, kind, what))


@pytest.mark.gpu
def test_ctc_training_batch_row_sums_and_sampled_utterances():
    """The benchmark's batch (256, 200, 62, 50) in bf16: reference-free row sums on every live frame of every utterance, and the
    element-wise bound on eight sampled utterances (the full-length, the empty, the infeasible one and five others) -- and, the
    reference of the whole batch being there for delta(case) anyway, on the other 248 as well."""
    dev = _need_gpu()
    from qcnn_amd import functional as Fq
    kind = 'bf16'
    p, labels, il, ll = ctc_inputs(CTC_BATCH, 'diffuse')
    ref = ctc_reference(CTC_BATCH, 'diffuse', kind)
    cost, g = _run_ctc(Fq, ref['pred'], labels, il, ll, kind, dev, 0)
    _note('ctc batch row sums', kind, _row_sum_check(g, ref['pred'], ref, kind, 'ctc training batch'))
    pick = np.array([0, 1, 2, 3, 64, 129, 200, 255])
    sub = dict(cost=tuple(a[pick] for a in ref['cost']), g=tuple(a[pick] for a in ref['g']), live=ref['live'][pick], label_mask=ref['label_mask'][pick])
    rc, rg = _check_ctc(cost[pick], g[pick], sub, 'ctc training batch, sampled utterances')
    _note('ctc batch cost (sampled)', kind, rc)
    _note('ctc batch gradient (sampled)', kind, rg)
    rc, rg = _check_ctc(cost, g, ref, 'ctc training batch')
    _note('ctc batch cost', kind, rc)
    _note('ctc batch gradient', kind, rg)
