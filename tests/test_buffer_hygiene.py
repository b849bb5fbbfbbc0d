"""Buffer hygiene of every C-ABI entry point that takes a device pointer: guard bands and two-fill runs (tests/guarded_alloc.py).

The parity tests ask whether the returned values are right.  These ask two other things of the same calls:
  1. did the call write anything OUTSIDE the buffers it was given (guard bands of 4 KiB on both sides of every output, workspace,
     aux and plan buffer, no slack between the payload and the high guard);
  2. does any returned byte depend on what a buffer held BEFORE the call (the same call under two fills that differ in every byte:
     an element that holds the fill in both runs was never written; any other difference between the runs is a read of
     uninitialised memory -- a missing memset in front of atomics, a flag word assumed zero).
What they cannot see: reads out of bounds, and writes farther than 4 KiB from the buffer.

Operands are lattice values (tests/lattice_ref.py) wherever a result is summed with fp32 atomics: every partial sum is then exact in
any order, so two runs must agree bit for bit.  NOT_BITWISE lists the outputs for which that cannot be arranged; they are held to
the bound of their own element-wise parity test in both runs instead.

CASES is the inventory: case name -> the C-ABI entry points it must be seen calling (a recorder around the loaded library checks
it on the GPU); together with EXCLUDED it must cover _lib.SYMBOLS exactly, so a new entry point fails the CPU test until it is
placed.
"""
import ctypes
import fnmatch
import json
import os

import numpy as np
import pytest
import torch

import guarded_alloc as GA
import lattice_ref as LR
import test_gpu_parity as P
import test_head_elementwise as TH
from conftest import GOLDEN

SEED = 2024
DTYPES = {'fp32': torch.float32, 'bf16': torch.bfloat16, 'fp16': torch.float16}

# ---------------------------------------------------------------------------------------------------------------------
# the inventory
# ---------------------------------------------------------------------------------------------------------------------
CASES = {
    'conv_entry_points': ('qk_conv_fwd', 'qk_conv_bwd_data', 'qk_conv_bwd_weight', 'qk_conv_bwd', 'qk_conv_bwd_chain', 'qk_conv_bwd_weight_acc'),
    'dense_entry_points': ('qk_dense_fwd', 'qk_dense_bwd_data', 'qk_dense_bwd_weight', 'qk_dense_bwd', 'qk_dense_bwd_chain',
                           'qk_dense_bwd_weight_acc'),
    'conv_post_ops': ('qk_conv_fwd_post', 'qk_conv_bwd_post'),
    'conv_post_bits': ('qk_conv_fwd_post_bits', 'qk_conv_bwd_post_bits'),
    'post_op': ('qk_postop_fwd', 'qk_postop_bwd'),
    'folded_taps': ('qk_conv_fold_taps', 'qk_conv_fwd', 'qk_conv_bwd_weight'),
    'cached_workspace': ('qk_conv_fwd', 'qk_conv_bwd'),
    'prepped_kernels': ('qk_conv_prep_kernels', 'qk_adam_step_zero_grad', 'qk_conv_fwd', 'qk_conv_bwd_chain'),
    'conv_relu_pool': ('qk_conv_relu_pool_fwd', 'qk_conv_relu_pool_bwd'),
    'conv_prelu_pool': ('qk_conv_prelu_pool_fwd', 'qk_conv_prelu_pool_bwd'),
    'maxpool': ('qk_maxpool2d_fwd', 'qk_maxpool2d_bwd'),
    'softmax_rows': ('qk_softmax_rows_fwd', 'qk_softmax_rows_bwd'),
    'dense_softmax': ('qk_dense_softmax_fwd', 'qk_dense_softmax_bwd'),
    'weighted_sum': ('qk_weighted_sum',),
    'ctc_cost': ('qk_ctc_batch_cost',),
    'ctc_greedy': ('qk_ctc_greedy_decode',),
    'ctc_beam': ('qk_ctc_beam_search_decode',),
    'ctc_beam_lm': ('qk_ctc_beam_search_decode_lm',),
    'ctc_forced_align': ('qk_ctc_forced_align',),
    'edit_distance': ('qk_edit_distance',),
    'edit_alignment': ('qk_edit_align',),
    'fbank': ('qk_fbank_quaternion',),
    'spec_augment': ('qk_spec_augment',),
    'speed_perturb': ('qk_speed_perturb',),
    'noise_reverb': ('qk_noise_reverb',),
    'adam': ('qk_adam_step', 'qk_adam_step_zero_grad', 'qk_adam_step_l2', 'qk_adam_step_dev'),
    'grad_guard': ('qk_grad_guard_reduce', 'qk_adam_step_guarded'),
    'flat_gradient_buffer': ('qk_conv_bwd_weight_acc', 'qk_conv_bwd_chain', 'qk_conv_bwd_weight'),
}

COVERED = {}
for _case, _symbols in CASES.items():
    for _s in _symbols:
        COVERED.setdefault(_s, []).append(_case)

# entry points that take no device pointer (or, the debug buffer, none that a kernel of a test writes through): nothing to guard
EXCLUDED = {
    'qk_version': 'host only: the version number',
    'qk_prof_enable': 'host only: qk_prof_*',
    'qk_prof_count': 'host only: qk_prof_*',
    'qk_prof_get': 'host only: qk_prof_* (copies a record into a host struct)',
    'qk_last_error': 'host only: qk_last_*',
    'qk_last_path': 'host only: qk_last_*',
    'qk_set_debug_flags': 'host only: debug flags',
    'qk_get_debug_flags': 'host only: debug flags',
    'qk_set_debug_buffer': 'debug flags: registers a diagnostic buffer, launches nothing',
    'qk_conv_workspace_bytes': 'host only: *_bytes',
    'qk_dense_workspace_bytes': 'host only: *_bytes',
    'qk_conv_mask_bits_bytes': 'host only: *_bytes',
    'qk_conv_bwd_reads_mask_bits': 'host only: a predicate on the descriptor, the partner of qk_conv_mask_bits_bytes',
    'qk_conv_relu_pool_aux_bytes': 'host only: *_bytes',
    'qk_ctc_workspace_bytes': 'host only: *_bytes',
    'qk_ctc_beam_workspace_bytes': 'host only: *_bytes',
    'qk_edit_align_workspace_bytes': 'host only: *_bytes',
    'qk_ctc_align_workspace_bytes': 'host only: *_bytes',
    'qk_fbank_num_frames': 'host only: frame count of a sample count',
    'qk_fbank_workspace_bytes': 'host only: *_bytes',
    'qk_speed_perturb_out_samples': 'host only: output length of a policy',
    'qk_noise_reverb_workspace_bytes': 'host only: *_bytes',
    'qk_dense_softmax_supported': 'host only: *_supported',
    'qk_dense_softmax_bwd_workspace_bytes': 'host only: *_bytes',
    'qk_grad_guard_workspace_bytes': 'host only: *_bytes',
}
# the only kinds of name EXCLUDED may hold: none of them launches a kernel
EXCLUDED_PATTERNS = ('*_bytes', '*_supported', 'qk_version', 'qk_prof_*', 'qk_last_*', 'qk_set_debug_flags', 'qk_get_debug_flags',
                     'qk_set_debug_buffer', 'qk_fbank_num_frames', 'qk_speed_perturb_out_samples', 'qk_conv_bwd_reads_mask_bits')

# (case, output) -> why the two runs need not agree bit for bit.  Such an output is compared, in BOTH runs, with the reference and
# the bound of its own element-wise parity test (imported from tests/test_head_elementwise.py, not restated).
NOT_BITWISE = {
    ('softmax_rows', 'dbias'): 'qk_softmax_rows_bwd adds one fp32 atomic per class and workgroup into the prefilled dbias; with more '
                               'than one workgroup (rows > 16) the order of three or more addends is free, and y * (dy - <dy, y>) is '
                               'not a lattice value',
}


def test_every_entry_point_is_covered_or_excluded_with_a_reason():
    from qcnn_amd import _lib
    symbols = set(_lib.SYMBOLS)
    assert set(COVERED) | set(EXCLUDED) == symbols, (sorted(symbols - set(COVERED) - set(EXCLUDED)), sorted((set(COVERED) | set(EXCLUDED)) - symbols))
    assert not set(COVERED) & set(EXCLUDED), sorted(set(COVERED) & set(EXCLUDED))
    for name, reason in EXCLUDED.items():
        assert reason and any(fnmatch.fnmatchcase(name, p) for p in EXCLUDED_PATTERNS), '%s is not a host-only kind of entry point' % name
    # every entry point that launches ends in its `void *stream` argument: no excluded one does, every covered one does
    ends_in_stream = lambda name: bool(_lib.SYMBOLS[name][1]) and _lib.SYMBOLS[name][1][-1] is ctypes.c_void_p
    assert not [n for n in EXCLUDED if ends_in_stream(n)] and not [n for n in COVERED if not ends_in_stream(n)]
    here = [k for k, v in globals().items() if k.startswith('test_') and callable(v)]
    for case in CASES:
        assert any(case in t for t in here), 'no test function for case %s' % case


def test_the_inventory_fails_for_an_entry_point_without_a_placement(monkeypatch):
    from qcnn_amd import _lib
    monkeypatch.setitem(_lib.SYMBOLS, 'qk_some_new_kernel', (None, []))
    with pytest.raises(AssertionError, match='qk_some_new_kernel'):
        test_every_entry_point_is_covered_or_excluded_with_a_reason()


def test_the_not_bitwise_table_is_pinned():
    assert sorted(NOT_BITWISE) == [('softmax_rows', 'dbias')]
    assert all(case in CASES and len(reason) > 40 for (case, _), reason in NOT_BITWISE.items())


# ---------------------------------------------------------------------------------------------------------------------
# CPU: the checker itself, on planted faults (plain Python functions on CPU tensors through the proxy)
# ---------------------------------------------------------------------------------------------------------------------
def _cpu_twice(fn):
    return GA.run_twice(lambda ga: fn(ga.proxy()), device_type='cpu')


def _rejected(check, *args):
    with pytest.raises(AssertionError) as e:
        check(*args)
    return str(e.value)


def _clean(t):
    x = t.arange(12, dtype=t.float32).reshape(3, 4)
    out = t.empty((3, 4), dtype=t.float32)
    out.copy_(2 * x)
    return dict(out=out)


def test_checker_accepts_a_clean_function():
    res = _cpu_twice(_clean)
    GA.assert_hygiene(res)
    a = res.allocs[0].log[0]
    assert len(res.allocs[0].log) == 1 and a.nbytes == 48 and a.buf.numel() == GA.G + 48 + GA.G + 256 and a.shape == (3, 4)
    assert a.site.startswith('test_buffer_hygiene.py:') and a.buf.data_ptr() % 256 == 0
    assert res.outputs[0]['out'].data_ptr() == a.buf.data_ptr() + GA.G
    assert GA.FILL_A ^ GA.FILL_B == 0xFE and 0 not in (GA.FILL_A, GA.FILL_B) and 0xFF not in (GA.FILL_A, GA.FILL_B)
    for fill in (GA.FILL_A, GA.FILL_B):          # every 2- and 4-byte float read of a fill is finite
        raw = torch.full((4,), fill, dtype=torch.uint8)
        assert all(bool(torch.isfinite(raw.view(dt).float()).all()) for dt in (torch.float16, torch.bfloat16, torch.float32))


def test_checker_names_a_write_one_element_past_the_end():
    def fn(t):
        out = t.zeros(10, dtype=t.bfloat16)
        out.as_strided((11,), (1,))[10] = 1.0                      # element 10 of a 10-element buffer
        return dict(out=out)
    msg = _rejected(GA.assert_guards_intact, _cpu_twice(fn))
    assert 'run A' in msg and 'high guard of zeros at test_buffer_hygiene.py:' in msg and 'shape (10,), torch.bfloat16 (20 bytes)' in msg, msg
    assert '2 bytes overwritten, first at byte 0, last at byte 1 past the payload end (elements 0 .. 0 past the end)' in msg, msg
    assert 'low guard' not in msg


def test_checker_names_a_write_one_element_before_the_start():
    def fn(t):
        out = t.zeros(10, dtype=t.float32)
        out.as_strided((1,), (1,), out.storage_offset() - 1)[0] = 1.0
        return dict(out=out)
    msg = _rejected(GA.assert_guards_intact, _cpu_twice(fn))
    assert 'low guard of zeros at test_buffer_hygiene.py:' in msg and 'first at byte -4, last at byte -1 relative to the payload start' in msg, msg
    assert 'high guard' not in msg


def test_checker_names_an_output_element_that_was_never_written():
    def fn(t):
        out = t.empty((3, 4), dtype=t.float32)
        out[0], out[2], out[1, :3] = 1.0, -1.0, 0.0                # element (1, 3) is left as allocated
        return dict(out=out)
    res = _cpu_twice(fn)
    GA.assert_guards_intact(res)
    msg = _rejected(GA.assert_no_stale_element, res)
    assert 'out: 1 of 12 elements were never written' in msg and 'first: index (1, 3)' in msg, msg

    def fn2(t):
        out = t.empty(9, dtype=t.int32)
        out[:4] = 1
        out[5:] = -1
        return dict(decoded=out)
    msg = _rejected(GA.assert_no_stale_element, _cpu_twice(fn2))
    assert 'decoded: 1 of 9 elements were never written' in msg and 'first: index (4,)' in msg, msg


def test_checker_catches_a_result_that_reads_an_unzeroed_scratch_buffer():
    def fn(t):
        x = t.arange(8, dtype=t.float32)
        scratch = t.empty(8, dtype=t.float32)                     # a workspace assumed zero: never cleared
        out = t.empty(8, dtype=t.float32)
        out.copy_(x + 0.5 * scratch)                               # every element of out IS written
        return dict(out=out)
    res = _cpu_twice(fn)
    GA.assert_guards_intact(res)
    GA.assert_no_stale_element(res)                               # check 2 passes ...
    msg = _rejected(GA.assert_bitwise_equal, res)                 # ... check 3 does not
    assert 'out: 8 of 8 elements differ between the run under fill 0xCB and the run under fill 0x35' in msg and 'first: index (0,)' in msg, msg


def test_checker_refuses_a_function_whose_buffers_bypass_the_allocator():
    def fn(t):
        return dict(out=t.ones(4) * 2)                            # torch.ones is not intercepted
    res = _cpu_twice(fn)
    msg = _rejected(GA.assert_allocations_seen, res)
    assert 'the proxy saw no allocation' in msg
    with pytest.raises(AssertionError, match='saw no allocation'):
        GA.assert_hygiene(res)


def test_proxy_passes_through_what_it_must_not_guard():
    ga = GA.GuardedAllocator(GA.FILL_A, 'cuda')                   # guards 'cuda': CPU-side host tensors pass through
    t = ga.proxy()
    assert t.empty(5).numel() == 5 and t.zeros((2, 3), dtype=t.int32).sum() == 0 and not ga.log
    assert t.float32 is torch.float32 and t.nn is torch.nn
    ga = GA.GuardedAllocator(GA.FILL_B, 'cpu')
    t = ga.proxy()
    assert t.empty(0).numel() == 0 and t.zeros((3, 0)).shape == (3, 0) and not ga.log          # zero-size requests
    z = t.zeros((), dtype=t.float32)
    e = t.empty_like(torch.ones(2, 3, dtype=torch.float16).t())
    assert z.shape == () and float(z) == 0.0 and e.shape == (3, 2) and e.stride() == (1, 3) and e.dtype == torch.float16
    assert [a.nbytes for a in ga.log] == [4, 12] and bool((e.contiguous().view(torch.uint8) == GA.FILL_B).all())
    assert bool((t.zeros_like(e) == 0).all()) and len(ga.log) == 3
    GA.check_guards(ga)


# ---------------------------------------------------------------------------------------------------------------------
# GPU: the harness of a case
# ---------------------------------------------------------------------------------------------------------------------
class _Recorder(object):
    """Delegates to the loaded library and logs the name of every entry point fetched from it."""

    def __init__(self, real):
        object.__setattr__(self, '_real', real)
        object.__setattr__(self, 'calls', [])

    def __getattr__(self, name):
        attr = getattr(self._real, name)
        if name.startswith('qk_'):
            self.calls.append(name)
        return attr


def _mods():
    import qcnn_amd
    from qcnn_amd import _lib, dp, layers, training
    return qcnn_amd.functional, _lib, layers, training, dp


def _run_case(monkeypatch, case, fn, what='', not_bitwise=None):
    """fn(ga) twice under the two fills with the proxy in functional, layers, training and dp and the recorder around the library;
    then: every entry point CASES assigns to `case` was called, the proxy saw allocations, checks 1, 2 and 3."""
    Fq, L, layers, training, dp = _mods()
    rec = _Recorder(L.lib())
    monkeypatch.setattr(L, '_lib', rec)
    res = GA.run_twice(fn, monkeypatch, (Fq, layers, training, dp), 'cuda', between=Fq.invalidate_cached_kernels)
    what = '%s %s: ' % (case, what)
    missing = [s for s in CASES[case] if s not in rec.calls]
    assert not missing, '%sentry points never called: %s (called: %s)' % (what, missing, sorted(set(rec.calls)))
    GA.assert_hygiene(res, what, not_bitwise)
    return res


def _ids(cases):
    return [c[0] for c in cases]


def _t(a, dev, dtype=torch.float32):
    return torch.tensor(np.asarray(a, dtype=np.float32), device=dev).to(dtype)


def _ints(rng, shape):
    return rng.randint(-3, 4, size=shape).astype(np.float32)


with open(os.path.join(GOLDEN, 'g18_dispatcher.json')) as _f:
    DISPATCH_PATHS = json.load(_f)['dispatch_paths']       # what test_every_small_case_is_served_by_the_kernel_family_recorded_for_it records


# ---------------------------------------------------------------------------------------------------------------------
# layers: every C-ABI entry point of a layer, at the ragged, native-layout and per-kernel-family shapes
# ---------------------------------------------------------------------------------------------------------------------
# one member of P.HALF_CASES per kernel family that qk_last_path tells apart (the smallest that reaches it)
FAMILY_OF = {'conv1d_16to48_valid': 'mfma16_band', 'conv1d_1x1_32to32': 'mfma16_point', 'conv2d_16to16_5tap': 'mfma16_small',
             'conv2d_body_small': 'mfma16', 'conv1d_odd_channels': 'fp32_mfma', 'dense_point_64to32': 'mfma16_point'}
FAMILY_CASES = [c for c in P.HALF_CASES if c[0] in FAMILY_OF]
LAYER_PARAMS = ([pytest.param('ragged', c, d, id='ragged/%s-%s' % (c[0], d)) for c in P.RAGGED_CASES for d in ('fp32', 'bf16')]
                + [pytest.param('native', c, d, id='native/%s-%s' % (c[0], d)) for c in P.NATIVE_16BIT for d in ('bf16', 'fp16')]
                + [pytest.param('half', c, d, id='half/%s-%s' % (c[0], d)) for c in FAMILY_CASES for d in ('fp32', 'bf16', 'fp16')])
AB_SMALLEST = min(P.AB_SWITCH_CASES, key=lambda c: int(np.prod(c[2])))
AB_SWITCHES = [m.args[1] for m in P.test_ab_switch_kernels_match_oracle.pytestmark if m.args[0] == 'switch'][0]


def _layer_call(Fq, case, dtype, native):
    """(call, physical x shape) as P._dispatch_paths builds them: HALF / RAGGED cases on physically channels_last buffers, NATIVE_16BIT
    on true channels_first ones."""
    _, rank, xs, ws, kw = case[:5]
    if rank == 0:
        return Fq.dense_call(tuple(xs), tuple(ws), dtype, kw.get('activation'), True), tuple(xs)
    layout = kw.get('data_format', 'channels_last')
    if layout == 'channels_first' and not native:
        xs, layout = (xs[0],) + tuple(xs[2:]) + (xs[1],), 'channels_last'
    call = Fq.conv_call(tuple(xs), tuple(ws), dtype, rank, kw.get('strides', 1), kw.get('padding', 'valid'), layout,
                        kw.get('dilation_rate', 1), kw.get('activation'), True, kw.get('conj', False))
    return call, tuple(xs)


def _entry_points(monkeypatch, group, case, dtype, switch=None):
    Fq, L, _, _, _ = _mods()
    dev = P._dev()
    dtype = DTYPES[dtype]
    native = group == 'native'
    rank, ws = case[1], case[3]
    want_paths = DISPATCH_PATHS['%s/%s' % (group, case[0])] if (dtype == torch.bfloat16 and switch is None) else None
    paths = []

    def fn(ga):
        call, xs = _layer_call(Fq, case, dtype, native)
        rng = np.random.RandomState(SEED)
        x, w, b, dy = LR.layer_operands(rng, xs, ws, call.y_shape, True, 'integer')
        fill_w, fill_b = _ints(rng, ws), _ints(rng, ws[-1])
        xt, dyt, wt, bt = _t(x, dev, dtype), _t(dy, dev, dtype), _t(w, dev), _t(b, dev)
        y = call.fwd(xt, wt, bt)
        p = [L.last_path()]
        ymask = y if call.relu else None
        dx = call.bwd_data(dyt, ymask, wt)
        p.append(L.last_path())
        dw, db = call.bwd_weight(xt, dyt, ymask, True)
        p.append(L.last_path())
        paths.append(p)
        fdx, fdw, fdb = call.bwd(xt, dyt, ymask, wt, True)
        # the forms that update caller-owned buffers in place: allocated by the test through the same guarded allocator
        acc_w, acc_b = ga.tensor(fill_w, device=dev), ga.tensor(fill_b, device=dev)
        call.bwd_weight(xt, dyt, ymask, True, out=(acc_w, acc_b), accumulate=True)
        ch_w, ch_b = ga.tensor(fill_w, device=dev), ga.tensor(fill_b, device=dev)
        ch_dx = ga.empty(call.x_shape, dtype=dtype, device=dev)
        flags = L.QK_BWD_ACCUMULATE
        if call.relu and not native:
            flags |= L.QK_BWD_MASK_DX | L.QK_BWD_DY_PREMASKED
        call.bwd(xt, dyt, ymask, wt, True, out=(ch_dx, ch_w, ch_b), flags=flags)
        return (dict(y=y, dx=dx, dkernel=dw, dbias=db, fused_dx=fdx, fused_dkernel=fdw, fused_dbias=fdb, chain_dx=ch_dx),
                dict(acc_dkernel=acc_w, acc_dbias=acc_b, chain_dkernel=ch_w, chain_dbias=ch_b))

    name = 'dense_entry_points' if rank == 0 else 'conv_entry_points'
    what = '%s/%s %s%s' % (group, case[0], dtype, ' under %s' % switch if switch else '')
    if switch:
        with L.debug_flags(getattr(L, switch)):
            _run_case(monkeypatch, name, fn, what)
    else:
        _run_case(monkeypatch, name, fn, what)
    if want_paths is not None:
        assert paths[0] == want_paths and paths[1] == want_paths, '%s: served by %s, recorded %s' % (what, paths, want_paths)
        if case[0] in FAMILY_OF:
            assert FAMILY_OF[case[0]] in want_paths


@pytest.mark.gpu
@pytest.mark.parametrize('group,case,dtype', LAYER_PARAMS)
def test_conv_entry_points_and_dense_entry_points(monkeypatch, group, case, dtype):
    """qk_{conv,dense}_fwd, _bwd_data, _bwd_weight, _bwd, _bwd_chain (flags) and _bwd_weight_acc with their workspaces: all of
    P.RAGGED_CASES (tails are where stray stores happen), P.NATIVE_16BIT (the workspace re-layout through k_relayout16) and one
    P.HALF_CASES member per kernel family; in bf16 the family that served each call is the one the dispatch test records."""
    _entry_points(monkeypatch, group, case, dtype)


@pytest.mark.gpu
@pytest.mark.parametrize('switch', AB_SWITCHES)
def test_conv_entry_points_under_the_ab_switches(monkeypatch, switch):
    """The kernels the default dispatch no longer reaches, on the smallest of P.AB_SWITCH_CASES."""
    _entry_points(monkeypatch, 'half', AB_SMALLEST, 'bf16', switch)


def test_the_family_cases_cover_every_family_the_dispatch_test_tells_apart():
    assert {FAMILY_OF[c[0]] for c in FAMILY_CASES} == {'mfma16_band', 'mfma16_point', 'mfma16_small', 'mfma16', 'fp32_mfma'}
    for c in FAMILY_CASES:
        assert FAMILY_OF[c[0]] in DISPATCH_PATHS['half/' + c[0]]
    assert AB_SMALLEST[0] == 'conv2d_32to64'


# the first shape of tests/test_mask_bits.py: a band-kernel layer whose bit tensor has no padding bytes (elements / 8 is a multiple of 16)
POST_SHAPE = (3, 6, 50, 32, 32)
SLOPES = np.array([0.25, 0.5, 1.0, 2.0])


# the two layers of test_conv_post_op_launches_are_exact_on_the_integer_lattice, the body layer at the first shape of tests/test_mask_bits.py
POST_LAYERS = [('body_32to32', POST_SHAPE[:3] + (4 * POST_SHAPE[3],), (3, 5, POST_SHAPE[3], 4 * POST_SHAPE[4]), dict(padding='same')),
               ('head_conj_valid', (2, 6, 40, 256), (6, 1, 64, 128), dict(padding='valid', conj=True))]


def _post_call(Fq, xs, ws, kw, dt):
    return Fq.conv_call(xs, ws, dt, 2, 1, kw['padding'], 'channels_last', 1, None, True, kw.get('conj', False))


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', ['fp32', 'bf16', 'fp16'])
@pytest.mark.parametrize('form', ['prelu', 'relu'])
@pytest.mark.parametrize('layer', POST_LAYERS, ids=_ids(POST_LAYERS))
def test_conv_post_ops(monkeypatch, layer, form, dtype):
    """qk_conv_fwd_post / qk_conv_bwd_post: the PReLU form (pre, y, d x_pre, and d alpha accumulated in place into a guarded buffer)
    and the relu form (one output tensor, x re-read as the mask), once overwriting dkernel / dbias and once with QK_BWD_ACCUMULATE.
    Slopes are powers of two and the dropout scale is exactly 2, so the slope gradient's atomics add lattice values."""
    Fq = _mods()[0]
    dev = P._dev()
    dt = DTYPES[dtype]
    _, xs, ws, kw = layer
    H = xs[1]

    def fn(ga):
        rng = np.random.RandomState(SEED)
        call = _post_call(Fq, xs, ws, kw, dt)
        x_pre, w, b, dy = LR.layer_operands(rng, xs, ws, call.y_shape, True, 'integer', kernel_density=1.0 / 8)
        prelu = form == 'prelu'
        alpha_x = _t(SLOPES[rng.randint(0, 4, size=H)], dev) if prelu else None          # one slope per position of spatial axis 0
        alpha_y = _t(SLOPES[rng.randint(0, 4, size=1)], dev) if prelu else None
        xt, dyt, wt, bt = _t(np.maximum(x_pre, 0) * 2, dev, dt), _t(dy, dev, dt), _t(w, dev), _t(b, dev)
        pre, y = call.fwd_post(xt, wt, bt, Fq.PostOp(alpha_y, -1, 0.5, 98765))
        assert (pre is not None) == prelu
        dalpha = ga.zeros(H, dtype=torch.float32, device=dev) if prelu else None
        post_x = Fq.PostOp(alpha_x, 0 if prelu else -1, 0.5, 1234)
        dx, dw, db = call.bwd_post(xt, dyt, wt, True, post_x, _t(x_pre, dev, dt) if prelu else None, dalpha)
        acc_w, acc_b = ga.tensor(_ints(rng, ws), device=dev), ga.tensor(_ints(rng, ws[-1]), device=dev)
        adx, _, _ = call.bwd_post(xt, dyt, wt, True, post_x, _t(x_pre, dev, dt) if prelu else None, dalpha, direct=(acc_w, acc_b))
        return dict(pre=pre, y=y, dx=dx, dkernel=dw, dbias=db, dx_accumulate_form=adx), dict(dalpha=dalpha, acc_dkernel=acc_w, acc_dbias=acc_b)
    _run_case(monkeypatch, 'conv_post_ops', fn, '%s %s %s' % (layer[0], form, dtype))


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', ['bf16', 'fp16'])
def test_conv_post_bits(monkeypatch, dtype):
    """qk_conv_fwd_post_bits / qk_conv_bwd_post_bits (relu + dropout 0.5): y and the bit-packed mask written beside it, dx through the
    bits of x, dkernel / dbias overwritten and accumulated."""
    Fq = _mods()[0]
    dev = P._dev()
    dt = DTYPES[dtype]
    _, xs, ws, kw = POST_LAYERS[0]

    def fn(ga):
        rng = np.random.RandomState(SEED)
        call = _post_call(Fq, xs, ws, kw, dt)
        x_pre, w, b, dy = LR.layer_operands(rng, xs, ws, call.y_shape, True, 'integer', kernel_density=1.0 / 8)
        xt, dyt, wt, bt = _t(np.maximum(x_pre, 0) * 2, dev, dt), _t(dy, dev, dt), _t(w, dev), _t(b, dev)
        nb = call.mask_bits_bytes()
        assert nb == int(np.prod(call.y_shape)) // 8 and call.reads_mask_bits()          # no padding bytes behind the last element's bit
        bits, y = call.fwd_post(xt, wt, bt, Fq.PostOp(None, -1, 0.5, 777), bits_bytes=nb)
        xbits = _t(np.packbits(np.asarray(x_pre > 0).reshape(-1), bitorder='little'), dev, torch.uint8)
        post_x = Fq.PostOp(None, -1, 0.5, 1234)
        dx, dw, db = call.bwd_post(xt, dyt, wt, True, post_x, None, None, x_bits=xbits)
        acc_w, acc_b = ga.tensor(_ints(rng, ws), device=dev), ga.tensor(_ints(rng, ws[-1]), device=dev)
        adx, _, _ = call.bwd_post(xt, dyt, wt, True, post_x, None, None, direct=(acc_w, acc_b), x_bits=xbits)
        return dict(bits=bits, y=y, dx=dx, dkernel=dw, dbias=db, dx_accumulate_form=adx), dict(acc_dkernel=acc_w, acc_dbias=acc_b)
    _run_case(monkeypatch, 'conv_post_bits', fn, dtype)


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', ['fp32', 'bf16', 'fp16'])
@pytest.mark.parametrize('shape,axis', [((3, 5, 7, 16), 0), ((2, 6, 9, 32), 1), ((4, 11, 24), -1), ((50, 64), -1)],
                         ids=['axis0', 'axis1', 'scalar3d', 'scalar2d'])
def test_post_op_prelu_dropout_and_relu_dropout(monkeypatch, shape, axis, dtype):
    """prelu_dropout / relu_dropout forward and backward (qk_postop_fwd / _bwd) at the shapes of test_prelu_dropout_op_matches_numpy."""
    Fq = _mods()[0]
    dev = P._dev()
    dt = DTYPES[dtype]

    def fn(ga):
        rng = np.random.RandomState(SEED)
        x, dy = LR.integer_lattice(rng, shape), LR.integer_lattice(rng, shape)
        alen = shape[1 + axis] if axis >= 0 else 1
        out = {}
        xt = _t(x, dev, dt).requires_grad_(True)
        at = _t(SLOPES[rng.randint(0, 4, size=alen)], dev).requires_grad_(True)
        y = Fq.prelu_dropout(xt, at, axis, 0.5, 12345)
        y.backward(_t(dy, dev, dt))
        out.update(prelu_y=y, prelu_dx=xt.grad, prelu_dalpha=at.grad)
        xr = _t(x, dev, dt).requires_grad_(True)
        yr = Fq.relu_dropout(xr, 0.5, 321)
        yr.backward(_t(dy, dev, dt))
        out.update(relu_y=yr, relu_dx=xr.grad)
        return out
    _run_case(monkeypatch, 'post_op', fn, '%s axis %d %s' % (shape, axis, dtype))


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', ['fp32', 'bf16'])
def test_folded_taps_first_layer(monkeypatch, dtype):
    """qk_conv_fold_taps and its xcol buffer: the 7 x 7 one-channel case of test_tap_folding_with_more_than_32_folded_channels."""
    Fq = _mods()[0]
    dev = P._dev()
    dt = DTYPES[dtype]
    xs, ws = (2, 19, 23, 4), (7, 7, 1, 32)

    def fn(ga):
        rng = np.random.RandomState(SEED)
        x, w, b, dy = LR.layer_operands(rng, xs, ws, xs[:-1] + (ws[-1],), True, 'integer')
        wt, bt = _t(w, dev).requires_grad_(True), _t(b, dev).requires_grad_(True)
        y = Fq.quaternion_conv(_t(x, dev, dt), wt, bt, padding='same', activation='relu')
        y.backward(_t(dy, dev, dt))
        return dict(y=y, dkernel=wt.grad, dbias=bt.grad)
    res = _run_case(monkeypatch, 'folded_taps', fn, dtype)
    sites = [a for a in res.allocs[0].log if a.shape == xs[:-1] + (4 * (64 if dt != torch.float32 else 56),)]
    assert sites, 'the folded copy xcol did not come through the guarded allocator: %s' % [a.describe() for a in res.allocs[0].log]


@pytest.mark.gpu
def test_cached_workspace_second_call_of_a_layer(monkeypatch):
    """The same layer twice within a run: the second forward and backward find the 16-bit re-layout of the kernel cached on the
    parameter (desc.ws_has_kernel = 1) and launch nothing but the GEMM; both calls must return the same bits."""
    Fq = _mods()[0]
    dev = P._dev()
    _, rank, xs, ws, kw = AB_SMALLEST
    hits = []

    def fn(ga):
        rng = np.random.RandomState(SEED)
        x, w, b, dy = LR.layer_operands(rng, xs, ws, xs[:-1] + (ws[-1],), True, 'integer')
        wt, bt = _t(w, dev).requires_grad_(True), _t(b, dev).requires_grad_(True)
        out = {}
        for i in (1, 2):
            xt = _t(x, dev, torch.bfloat16).requires_grad_(True)
            n_ws = sum(1 for a in ga.log if a.dtype == torch.uint8)
            y = Fq.quaternion_conv(xt, wt, bt, **kw)
            y.backward(_t(dy, dev, torch.bfloat16))
            hits.append(sum(1 for a in ga.log if a.dtype == torch.uint8) - n_ws)
            out.update({'y%d' % i: y, 'dx%d' % i: xt.grad})
        out.update(dkernel=wt.grad, dbias=bt.grad)
        assert len(wt.__dict__.get('_qk_prep', {})) >= 1                  # the forward's image of the kernel at least
        return out
    res = _run_case(monkeypatch, 'cached_workspace', fn)
    # the first call allocates the workspace it caches, the second call does not (a relu layer's fused backward also carries the
    # masked dy in its workspace: that one is allocated per call)
    assert 0 <= hits[1] < hits[0] <= 2 and hits[2:] == hits[:2], 'workspace allocations per call: %s' % hits
    for run in res.outputs:
        assert GA.first_bit_difference(run['y1'], run['y2']) is None and GA.first_bit_difference(run['dx1'], run['dx2']) is None


def _three_layers(dev, dp, rng, shapes=((3, 32, 128), (3, 32, 128), (1, 32, 128))):
    """Three small 1-D layers re-homed into one dp.FlatParams buffer with direct gradients (the set-up of
    test_flat_buffer_step_on_two_half_batches_equals_full_batch, three deep); the default shapes run on the 16-bit band and point
    kernels."""
    params = []
    for ws in shapes:
        params.append(torch.nn.Parameter(_t(LR.integer_lattice(rng, ws, 1.0 / 8), dev)))
        params.append(torch.nn.Parameter(_t(LR.integer_bias(rng, ws[-1]), dev)))
    return params, dp.FlatParams(params, direct=True)


@pytest.mark.gpu
def test_prepped_kernels_refresh_behind_the_optimiser_step(monkeypatch):
    """refresh_prepped_kernels (qk_conv_prep_kernels) behind adam_step on a dp.FlatParams buffer: the workspaces it rewrites are the
    guarded ones the layers cached, and the next forward, which launches no re-layout of its own, equals a forward that does."""
    Fq, _, _, _, dp = _mods()
    dev = P._dev()
    dt = torch.bfloat16

    def fn(ga):
        rng = np.random.RandomState(SEED)
        params, flat = _three_layers(dev, dp, rng)
        x = _t(LR.integer_lattice(rng, (2, 43, 128)), dev, dt)
        chain = lambda: Fq.quaternion_conv_chain(x, [(params[2 * i], params[2 * i + 1], dict(padding='same', activation='relu')) for i in range(3)])
        y = chain()
        y.backward(_t(LR.integer_lattice(rng, tuple(y.shape)), dev, dt))
        m, v = ga.zeros(flat.numel, dtype=torch.float32, device=dev), ga.zeros(flat.numel, dtype=torch.float32, device=dev)
        n_prepped = sum(len(p.__dict__.get('_qk_prep', {})) for p in params)
        Fq.adam_step(flat.param, flat.grad, m, v, 1, lr=0.25, zero_grad=True)           # ... and refresh_prepped_kernels(flat.param)
        y2 = chain()
        Fq.invalidate_cached_kernels()
        y3 = chain()
        assert n_prepped >= 3
        return dict(y=y, y_after_refresh=y2, y_after_relayout=y3), dict(param=flat.param, grad=flat.grad)
    res = _run_case(monkeypatch, 'prepped_kernels', fn)
    for run in res.outputs:
        assert GA.first_bit_difference(run['y_after_refresh'], run['y_after_relayout']) is None
        assert GA.first_bit_difference(run['y'], run['y_after_refresh']) is not None          # the step did move the weights


# kernel shapes (taps, Cq, 4 F) of three chained 1-D layers and the channel count of their input
FLAT_LAYERS = {
    # element counts that are no multiple of 64: FlatParams leaves alignment gaps of 12 / 28 / 12 / 36 / 52 / 44 floats behind the views
    'gaps_off_the_matrix_cores': (((3, 7, 36), (3, 9, 28), (1, 7, 20)), 28),
    # the 16-bit band and point kernels: no gaps (every count is a multiple of 64), each view borders its neighbour directly
    'adjacent_views_band_kernels': (((3, 32, 128), (3, 32, 128), (1, 32, 128)), 128),
}


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', ['fp32', 'bf16'])
@pytest.mark.parametrize('layers', sorted(FLAT_LAYERS))
def test_flat_gradient_buffer_keeps_every_layer_to_its_own_views(monkeypatch, layers, dtype):
    """In a dp.FlatParams gradient buffer the neighbour of a layer's dw is another layer's gradient.  The buffer is prefilled with
    the fill pattern and the views are then zeroed (the state adam_step(zero_grad=True) leaves them in; a gradient ADDED to the
    pattern itself, -2.7e7, would round); one backward of the three layers follows, in two forms: accumulating
    (qk_conv_bwd_weight_acc for the first layer, qk_conv_bwd_chain with QK_BWD_ACCUMULATE for the others) and overwriting
    (qk_conv_bwd_weight with the views as dw / dbias).  Every element that lies in no view must still hold the fill -- except, in
    the overwriting form, the alignment gap between a layer's dw and its OWN dbias, which include/qk.h lets that call zero with
    them.  And no layer's views may differ from what that layer's own backward leaves when it runs alone."""
    Fq, L, _, _, dp = _mods()
    dev = P._dev()
    dt = DTYPES[dtype]
    shapes, cin = FLAT_LAYERS[layers]

    def fn(ga):
        rng = np.random.RandomState(SEED)
        params, flat = _three_layers(dev, dp, rng, shapes)
        n = flat.numel
        in_view, own_gap = np.zeros(n, dtype=bool), np.zeros(n, dtype=bool)
        for p, o in zip(flat.params, flat.offsets):
            in_view[o:o + p.numel()] = True
        for i in range(3):                                   # between layer i's dw and its own dbias
            own_gap[flat.offsets[2 * i] + params[2 * i].numel():flat.offsets[2 * i + 1]] = True
        assert not (in_view & own_gap).any() and (layers != 'gaps_off_the_matrix_cores' or (~in_view).sum() == 12 + 28 + 12 + 36 + 52 + 44)
        acts, calls = [_t(np.maximum(LR.integer_lattice(rng, (2, 43, cin)), 0), dev, dt)], []
        for i in range(3):
            w = params[2 * i]
            calls.append(Fq.conv_call(tuple(acts[-1].shape), tuple(w.shape), dt, 1, 1, 'same', 'channels_last', 1, 'relu', True))
            acts.append(calls[-1].fwd(acts[-1], w.data, params[2 * i + 1].data))
        dys = [_t(LR.integer_lattice(rng, tuple(a.shape)), dev, dt) for a in acts[1:]]
        views = [flat.grad_view(j) for j in range(6)]

        def prefill():
            flat.grad.view(torch.uint8).fill_(ga.fill)
            for v in views:
                v.zero_()

        def backward(i, form):
            out = (views[2 * i], views[2 * i + 1])
            if form == 'overwrite':
                calls[i].bwd_weight(acts[i], dys[i], acts[i + 1], True, out=out)
            elif i == 0:
                calls[i].bwd_weight(acts[i], dys[i], acts[i + 1], True, out=out, accumulate=True)
            else:
                dx = ga.empty(calls[i].x_shape, dtype=dt, device=dev)
                calls[i].bwd(acts[i], dys[i], acts[i + 1], params[2 * i].data, True, out=(dx,) + out, flags=L.QK_BWD_ACCUMULATE)
        results = {}
        for form in ('accumulate', 'overwrite'):
            alone = []
            for i in range(3):
                prefill()
                backward(i, form)
                alone.append(flat.grad.clone())
            prefill()
            for i in (2, 1, 0):
                backward(i, form)
            torch.cuda.synchronize()
            got = flat.grad.view(torch.uint8).reshape(n, 4).cpu().numpy()
            still_fill, zero = (got == ga.fill).all(axis=1), (got == 0).all(axis=1)
            allowed = in_view | still_fill | ((own_gap & zero) if form == 'overwrite' else False)
            assert allowed.all(), '%s: elements of the flat gradient buffer outside every view were written: %s' % (form, np.flatnonzero(~allowed)[:8])
            for i in range(3):
                for j in (2 * i, 2 * i + 1):
                    o, cnt = flat.offsets[j], params[j].numel()
                    assert GA.first_bit_difference(flat.grad[o:o + cnt], alone[i][o:o + cnt]) is None, \
                        '%s: view %d differs from what its layer writes when run alone' % (form, j)
                    for k in range(3):
                        assert k == i or not bool(alone[k][o:o + cnt].any()), '%s: layer %d alone wrote into view %d of layer %d' % (form, k, j, i)
            assert all(bool(views[2 * i].any()) for i in range(3))
            results.update({'%s/view%d' % (form, j): v.clone() for j, v in enumerate(views)})
        return dict(y=acts[-1]), results
    _run_case(monkeypatch, 'flat_gradient_buffer', fn, '%s %s' % (layers, dtype))


# ---------------------------------------------------------------------------------------------------------------------
# the fused first layer
# ---------------------------------------------------------------------------------------------------------------------
FIRST_SHAPE = (1, 8, 19, 4)


def _first_layer(monkeypatch, case, dtype, fq, planes):
    Fq = _mods()[0]
    dev = P._dev()
    dt = DTYPES[dtype]
    lay = 'channels_first' if planes else 'channels_last'
    prelu = case == 'conv_prelu_pool'

    def fn(ga):
        rng = np.random.RandomState(SEED)
        x, w, b, _ = LR.layer_operands(rng, FIRST_SHAPE, (3, 5, 1, 4 * fq), None, True, 'integer')
        xt = _t(x, dev, dt)
        if planes:
            xt = xt.permute(0, 3, 1, 2).contiguous()
        wt, bt = _t(w, dev).requires_grad_(True), _t(b, dev).requires_grad_(True)
        if prelu:
            at = _t(SLOPES[rng.randint(0, 4, size=FIRST_SHAPE[1])].reshape(1, -1, 1), dev).requires_grad_(True)
            assert Fq.conv_prelu_pool_supported(xt, wt, at, 0, 3, lay)
            out = Fq.conv_prelu_pool(xt, wt, bt, at, 0, 3, lay)
        else:
            assert Fq.conv_relu_pool_supported(xt, wt, 3, lay)
            out = Fq.conv_relu_pool(xt, wt, bt, 3, lay)
        out.backward(_t(LR.integer_lattice(rng, tuple(out.shape)), dev, dt))
        res = dict(pooled=out, dkernel=wt.grad, dbias=bt.grad)
        if prelu:
            res['dalpha'] = at.grad
        return res
    res = _run_case(monkeypatch, case, fn, '%s F=%d %s' % (dtype, fq, lay))
    # the arg-max side tensor (aux) came through the allocator: its guards were checked, and the backward that reads it gave the
    # same bits under both fills
    assert any(a.dtype == torch.uint8 and a.kind == 'empty' for a in res.allocs[0].log), [a.describe() for a in res.allocs[0].log]


@pytest.mark.gpu
@pytest.mark.parametrize('planes', [False, True], ids=['x_channels_last', 'x_component_planes'])
@pytest.mark.parametrize('fq', [32, 8])
@pytest.mark.parametrize('dtype', ['bf16', 'fp16'])
def test_conv_relu_pool(monkeypatch, dtype, fq, planes):
    _first_layer(monkeypatch, 'conv_relu_pool', dtype, fq, planes)


@pytest.mark.gpu
@pytest.mark.parametrize('planes', [False, True], ids=['x_channels_last', 'x_component_planes'])
@pytest.mark.parametrize('fq', [32, 8])
@pytest.mark.parametrize('dtype', ['bf16', 'fp16'])
def test_conv_prelu_pool(monkeypatch, dtype, fq, planes):
    _first_layer(monkeypatch, 'conv_prelu_pool', dtype, fq, planes)


# ---------------------------------------------------------------------------------------------------------------------
# aux kernels
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('dtype', ['fp32', 'bf16', 'fp16'])
@pytest.mark.parametrize('shape,window,out_hw', [((2, 9, 7, 24), (2, 3), (5, 3)), ((2, 41, 5, 8), (3, 1), (13, 5)), ((1, 4, 6, 40), (2, 2), (2, 3))],
                         ids=['partial_last_windows', 'valid_trailing_rows', 'full_windows'])
def test_maxpool_forward_and_backward(monkeypatch, shape, window, out_hw, dtype):
    """qk_maxpool2d_fwd / _bwd: partial last windows in both axes, rows outside every window ('valid': their gradient is the zero of a
    fill in front of the kernel), channel counts that are one, three and five vectors (fp32: 4-channel vectors, so 12 / 4 / 20)."""
    Fq = _mods()[0]
    dev = P._dev()
    dt = DTYPES[dtype]
    if dt == torch.float32:
        shape = shape[:3] + (shape[3] // 2,)

    def fn(ga):
        rng = np.random.RandomState(SEED)
        xt = _t(LR.integer_lattice(rng, shape), dev, dt).requires_grad_(True)
        assert Fq.maxpool2d_supported(xt, window, window)
        y = Fq.maxpool2d_channels_last(xt, window, out_hw)
        y.backward(_t(LR.integer_lattice(rng, tuple(y.shape)), dev, dt))
        return dict(y=y, dx=xt.grad)
    _run_case(monkeypatch, 'maxpool', fn, '%s %s' % (shape, dtype))


def _within_own_bound(check):
    """A NOT_BITWISE output: both runs against the reference and bound of the entry point's own parity test."""
    return lambda a, b, name: [check(TH._host(t)) for t in (a, b)]


@pytest.mark.gpu
@pytest.mark.parametrize('kind', TH.KINDS)
@pytest.mark.parametrize('rows,cols', [(5, 62), (TH.SM_ROWS[-1], 33)], ids=['one_workgroup', 'many_workgroups'])
def test_softmax_rows_forward_and_backward(monkeypatch, rows, cols, kind):
    """qk_softmax_rows_fwd / _bwd with dbias prefilled (a caller-owned buffer, updated in place), on the inputs of
    test_softmax_rows_kernels_elementwise."""
    Fq = _mods()[0]
    dev = P._dev()
    d = TH.softmax_rows_inputs(rows, cols, kind)

    def fn(ga):
        y = Fq.softmax_rows_fwd(TH._dev(d['logits'], 'fp32', dev), TH._dev(d['bias'], 'fp32', dev), TH.TORCH[kind])
        y0 = Fq.softmax_rows_fwd(TH._dev(d['logits'], 'fp32', dev), None, TH.TORCH[kind])
        db = ga.tensor(d['db0'], device=dev)
        dl = Fq.softmax_rows_bwd(TH._dev(d['y'], kind, dev), TH._dev(d['dy'], kind, dev), db)
        return dict(y=y, y_no_bias=y0, dlogits=dl), dict(dbias=db)
    nb = None
    if rows > 16:                 # more than one workgroup adds into dbias: NOT_BITWISE[('softmax_rows', 'dbias')]
        ref, bound = TH.H.softmax_rows_bwd_ref(d['y'], d['dy'], kind, dbias0=d['db0'])['dbias']
        nb = dict(dbias=_within_own_bound(lambda got: TH.H.assert_within(got, ref, bound, ('softmax_rows %dx%d %s dbias' % (rows, cols, kind), 'rows'))))
    _run_case(monkeypatch, 'softmax_rows', fn, '%dx%d %s' % (rows, cols, kind), not_bitwise=nb)


@pytest.mark.gpu
@pytest.mark.parametrize('kind', TH.KINDS16)
@pytest.mark.parametrize('shape', [(17, 64, 62), (97, 128, 18), (97, 256, 50)], ids=TH._out_id)
def test_dense_softmax_forward_and_backward(monkeypatch, shape, kind):
    """qk_dense_softmax_fwd / _bwd with its slab workspace and prefilled dkernel / dbias (no float atomics: a fixed-order slab
    reduction, so ordinary operands are bit-repeatable), at three of the tile-edge shapes of test_output_layer_kernels_elementwise."""
    Fq = _mods()[0]
    dev = P._dev()
    rows, K, U = shape
    d = TH.out_layer_inputs(rows, K, U, kind, True)

    def fn(ga):
        x, w = TH._dev(d['x'], kind, dev), TH._dev(d['w'], 'fp32', dev)
        assert Fq.dense_softmax_supported(x, U)
        y = Fq.dense_softmax_fwd(x, w, TH._dev(d['b'], 'fp32', dev))
        dk, db = ga.tensor(d['dk0'], device=dev), ga.tensor(d['db0'], device=dev)
        dx = Fq.dense_softmax_bwd(x, w, TH._dev(d['y'], kind, dev), TH._dev(d['dy'], kind, dev), dk, db)
        dx_only = Fq.dense_softmax_bwd(x, w, TH._dev(d['y'], kind, dev), TH._dev(d['dy'], kind, dev), None, None)
        return dict(y=y, dx=dx, dx_without_gradients=dx_only), dict(dkernel=dk, dbias=db)
    res = _run_case(monkeypatch, 'dense_softmax', fn, '%s %s' % (shape, kind))
    assert any(a.dtype == torch.uint8 for a in res.allocs[0].log), 'the slab workspace did not come through the guarded allocator'


@pytest.mark.gpu
@pytest.mark.parametrize('kind', TH.KINDS)
@pytest.mark.parametrize('n', [257, 4099])
def test_weighted_sum(monkeypatch, n, kind):
    """qk_weighted_sum ADDS to *out: through functional.weighted_sum (its own zeroed scalar) and through the C-ABI on a guarded,
    prefilled scalar.  Integer operands: the one atomic per workgroup adds exact values."""
    Fq = _mods()[0]
    dev = P._dev()

    def fn(ga):
        rng = np.random.RandomState(SEED)
        a, w = _t(LR.integer_lattice(rng, (n,)), dev, TH.TORCH[kind]), _t(_ints(rng, n), dev)
        plain = Fq.weighted_sum(a, w)
        out = ga.tensor(np.array([5.0], dtype=np.float32), device=dev)
        with Fq._on_device(dev):
            rc = Fq.L.lib().qk_weighted_sum(Fq._DTYPES[TH.TORCH[kind]], n, Fq._ptr(a), Fq._ptr(w), Fq._ptr(out), Fq._stream(a))
        Fq.L.check(rc, 'qk_weighted_sum')
        return dict(plain=plain), dict(out=out)
    _run_case(monkeypatch, 'weighted_sum', fn, 'n=%d %s' % (n, kind))


# ---------------------------------------------------------------------------------------------------------------------
# the CTC family: ragged lengths that include 0, 1 and T, so the -1 / 0 padding regions are large
# ---------------------------------------------------------------------------------------------------------------------
CTC_SHAPES = [(8, 40, 4, 6), (8, 40, 62, 20), (3, 1, 4, 2)]          # (B, T, C, Lmax)
CTC_IDS = ['x'.join(map(str, s)) for s in CTC_SHAPES]


def _ctc_inputs(shape):
    """(posteriors (B, T, C) float64, labels, input_length, label_length).  input_length takes 0, 1 and T; label_length 0, 1 and Lmax;
    one sample has more labels than frames (infeasible).  No class occurs more than TWICE among a sample's labels: a class then
    receives at most two occupancy atomics per frame (the blanks are one wave-reduced addend), and a sum of two floats does not
    depend on their order -- the gradient is bit-repeatable without QK_DBG_DETERMINISTIC."""
    B, T, C, Lmax = shape
    rng = np.random.RandomState(B * 1000 + T * 10 + C)
    z = 1.5 * rng.randn(B, T, C)
    e = np.exp(z - z.max(-1, keepdims=True))
    y = 0.98 * e / e.sum(-1, keepdims=True) + 0.02 / C
    labels = np.zeros((B, Lmax), dtype=np.int64)
    for b in range(B):
        pool = np.repeat(np.arange(C - 1), 2)
        labels[b] = rng.permutation(pool)[:Lmax]
    il = np.array(([T, 0, 1, T, T // 2, 3, T - 1, T])[:B])
    ll = np.array(([Lmax, 1, 1, 0, 1, Lmax, 2, Lmax // 2])[:B])
    if T == 1:
        il, ll = np.array([1, 0, 1][:B]), np.array([1, 1, 0][:B])
    assert all(np.bincount(labels[b], minlength=C).max() <= 2 for b in range(B))
    return y, labels, il, ll


def _ctc_dev(shape, dtype, dev):
    y, labels, il, ll = _ctc_inputs(shape)
    i32 = lambda a: torch.tensor(a, dtype=torch.int32, device=dev)
    return _t(y, dev, dtype), i32(labels), i32(il), i32(ll)


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', ['fp32', 'bf16', 'fp16'])
@pytest.mark.parametrize('form', ['k_ctc_fast', 'k_ctc'])
@pytest.mark.parametrize('shape', CTC_SHAPES, ids=CTC_IDS)
def test_ctc_cost_and_gradient(monkeypatch, shape, form, dtype):
    """qk_ctc_batch_cost with its lattice workspace on both kernels of launch_ctc (csrc/qk_ctc.hip): the fast form is taken whenever
    the sample's two (T, C) tables fit 150 KB of LDS -- every shape of this size -- and k_ctc otherwise or under
    QK_DBG_CTC_TWO_SWEEPS, which is how it is reached here; the gradient is zero past input_length and for the infeasible sample."""
    Fq, L, _, _, _ = _mods()
    dev = P._dev()

    def fn(ga):
        y, labels, il, ll = _ctc_dev(shape, DTYPES[dtype], dev)
        assert Fq.ctc_supported(y, labels)
        cost, g = Fq.ctc_cost_and_grad(y, labels, il, ll)
        return dict(cost=cost, gradient=g)
    with L.debug_flags(L.QK_DBG_CTC_TWO_SWEEPS if form == 'k_ctc' else 0):
        res = _run_case(monkeypatch, 'ctc_cost', fn, '%s %s %s' % (shape, form, dtype))
    _, _, il, _ = _ctc_inputs(shape)
    g = res.outputs[0]['gradient'].float().cpu().numpy()
    for b, n in enumerate(il):
        assert not g[b, n:].any(), 'gradient past input_length of sample %d' % b


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', ['fp32', 'bf16'])
@pytest.mark.parametrize('shape', CTC_SHAPES, ids=CTC_IDS)
def test_ctc_greedy_decode(monkeypatch, shape, dtype):
    Fq = _mods()[0]
    dev = P._dev()

    def fn(ga):
        y, _, il, _ = _ctc_dev(shape, DTYPES[dtype], dev)
        dec, dlen, lp = Fq.ctc_greedy_decode(y, il)
        return dict(decoded=dec, decoded_len=dlen, log_prob=lp)
    res = _run_case(monkeypatch, 'ctc_greedy', fn, '%s %s' % (shape, dtype))
    dec, dlen = res.outputs[0]['decoded'].cpu().numpy(), res.outputs[0]['decoded_len'].cpu().numpy()
    for b in range(shape[0]):
        assert (dec[b, dlen[b]:] == -1).all() and (dec[b, :dlen[b]] >= 0).all()


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', ['fp32', 'bf16'])
@pytest.mark.parametrize('width,top', [(1, 1), (128, 3)], ids=['W1', 'W128_unpruned'])
@pytest.mark.parametrize('shape', [(8, 5, 4, 6), (8, 40, 62, 20)], ids=['8x5x4', '8x40x62'])
def test_ctc_beam_search_decode(monkeypatch, shape, width, top, dtype):
    """qk_ctc_beam_search_decode with its history workspace: W = 1, and W = 128 (at T = 5, C = 4 every prefix fits: nothing is pruned;
    paths beyond the number of distinct beams come back empty, -1 everywhere)."""
    Fq = _mods()[0]
    dev = P._dev()

    def fn(ga):
        y, _, il, _ = _ctc_dev(shape, DTYPES[dtype], dev)
        dec, dlen, lp = Fq.ctc_beam_search_decode(y, il, beam_width=width, top_paths=top)
        return dict(decoded=dec, decoded_len=dlen, log_prob=lp)
    res = _run_case(monkeypatch, 'ctc_beam', fn, '%s W=%d %s' % (shape, width, dtype))
    dec, dlen = res.outputs[0]['decoded'].cpu().numpy(), res.outputs[0]['decoded_len'].cpu().numpy()
    for p in range(top):
        for b in range(shape[0]):
            assert (dec[p, b, dlen[p, b]:] == -1).all() and (dec[p, b, :dlen[p, b]] >= 0).all()


@pytest.mark.gpu
@pytest.mark.parametrize('order', [2, 3])
@pytest.mark.parametrize('shape', [(8, 5, 4, 6), (8, 40, 62, 20)], ids=['8x5x4', '8x40x62'])
def test_ctc_beam_lm_decode(monkeypatch, shape, order):
    """qk_ctc_beam_search_decode_lm: the whole table in LDS (C = 4; C = 62 bigram) and the per-beam context rows (C = 62 trigram)."""
    Fq = _mods()[0]
    from qcnn_amd.lm import NgramLM
    dev = P._dev()
    C = shape[2]
    rng = np.random.RandomState(C + order)
    z = rng.randn(C ** (order - 1), C) * 1.5
    lm = NgramLM(z - np.log(np.exp(z).sum(-1, keepdims=True)), C - 1, order)

    def fn(ga):
        y, _, il, _ = _ctc_dev(shape, torch.float32, dev)
        dec, dlen, lp, score = Fq.ctc_beam_search_decode_lm(y, il, lm, beam_width=16, top_paths=3, lm_weight=0.5, insertion_bonus=0.25)
        return dict(decoded=dec, decoded_len=dlen, log_prob=lp, score=score)
    _run_case(monkeypatch, 'ctc_beam_lm', fn, '%s order %d' % (shape, order))


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', ['fp32', 'bf16'])
@pytest.mark.parametrize('shape', CTC_SHAPES, ids=CTC_IDS)
def test_ctc_forced_align(monkeypatch, shape, dtype):
    Fq = _mods()[0]
    dev = P._dev()

    def fn(ga):
        y, labels, il, ll = _ctc_dev(shape, DTYPES[dtype], dev)
        r = Fq.ctc_forced_align(y, labels, il, ll)
        return dict(path=r.path, starts=r.starts, ends=r.ends, score=r.score)
    res = _run_case(monkeypatch, 'ctc_forced_align', fn, '%s %s' % (shape, dtype))
    _, _, il, ll = _ctc_inputs(shape)
    out = {k: v.cpu().numpy() for k, v in res.outputs[0].items()}
    for b in range(shape[0]):
        ok = np.isfinite(out['score'][b])
        assert (out['path'][b, il[b] if ok else 0:] == -1).all() and (out['starts'][b, ll[b] if ok else 0:] == -1).all()
        assert (out['ends'][b, ll[b] if ok else 0:] == -1).all()


def _token_inputs(dev):
    """(hyp (B, 9), hyp_len, ref (B, 7), ref_len, class_map): lengths 0, 1 and the stride on both sides."""
    rng = np.random.RandomState(77)
    B, K = 8, 6
    hyp, ref = rng.randint(0, K, size=(B, 9)), rng.randint(0, K, size=(B, 7))
    hl, rl = np.array([9, 0, 1, 9, 4, 0, 9, 3]), np.array([7, 7, 0, 1, 7, 0, 2, 7])
    cmap = np.array([0, 1, 2, 2, -1, 4])
    i32 = lambda a: torch.tensor(a, dtype=torch.int32, device=dev)
    return i32(hyp), i32(hl), i32(ref), i32(rl), i32(cmap), K


@pytest.mark.gpu
@pytest.mark.parametrize('mapped', [False, True], ids=['plain', 'class_map'])
def test_edit_distance(monkeypatch, mapped):
    Fq = _mods()[0]
    dev = P._dev()

    def fn(ga):
        hyp, hl, ref, rl, cmap, _ = _token_inputs(dev)
        dist, rlen = Fq._edit_distance(hyp, hl, ref, rl, cmap if mapped else None)
        return dict(distance=dist, ref_len=rlen)
    _run_case(monkeypatch, 'edit_distance', fn)


@pytest.mark.gpu
@pytest.mark.parametrize('confusion', [False, True], ids=['no_confusion', 'confusion'])
@pytest.mark.parametrize('align', [True, False], ids=['align', 'counts_only'])
def test_edit_alignment(monkeypatch, align, confusion):
    """qk_edit_align: the aligned pairs with their -1 tails, the counts, and the caller-owned confusion matrix accumulated in place
    (integer atomics: order-independent)."""
    Fq = _mods()[0]
    dev = P._dev()

    def fn(ga):
        hyp, hl, ref, rl, cmap, K = _token_inputs(dev)
        conf = ga.tensor(np.arange((K + 1) ** 2).reshape(K + 1, K + 1), dtype=torch.int32, device=dev) if confusion else None
        r = Fq.edit_alignment(hyp, hl, ref, rl, class_map=cmap, confusion=conf, align=align)
        return dict(ref=r.ref, hyp=r.hyp, length=r.length, counts=r.counts), dict(confusion=conf)
    res = _run_case(monkeypatch, 'edit_alignment', fn)
    if align:
        out = {k: v.cpu().numpy() for k, v in res.outputs[0].items()}
        for b in range(8):
            assert (out['ref'][b, out['length'][b]:] == -1).all() and (out['hyp'][b, out['length'][b]:] == -1).all()


# ---------------------------------------------------------------------------------------------------------------------
# the front end: ragged lengths with one utterance far shorter than max_samples, plans requested
# ---------------------------------------------------------------------------------------------------------------------
def _waves(dev, n_max, dtype):
    rng = np.random.RandomState(9)
    w = (rng.randn(4, n_max) * 3000).astype(np.int16)
    lengths = torch.tensor([n_max, 1, 401, 0], dtype=torch.int32, device=dev)
    t = torch.tensor(w, device=dev)
    return (t if dtype == 'int16' else t.float()), lengths


@pytest.mark.gpu
@pytest.mark.parametrize('normalize', [None, 'utterance'], ids=['plain', 'normalized'])
@pytest.mark.parametrize('dtype', ['fp32', 'bf16'])
def test_fbank_quaternion(monkeypatch, dtype, normalize):
    """qk_fbank_quaternion with its static-row (and, normalising, fp32 feature) workspace: nfft 512 (the smallest its own GPU test
    runs), 6 frames, utterances of n_max, 1, 401 and 0 samples -- frames beyond flen stay 0."""
    from qcnn_amd import features
    dev = P._dev()

    def fn(ga):
        wave, lengths = _waves(dev, 1200, 'int16')
        x, flen = features.quaternion_fbank(wave, lengths, normalize=normalize, dtype=DTYPES[dtype])
        return dict(features=x, frame_lengths=flen)
    res = _run_case(monkeypatch, 'fbank', fn, '%s %s' % (dtype, normalize))
    x, flen = res.outputs[0]['features'].float().cpu().numpy(), res.outputs[0]['frame_lengths'].cpu().numpy()
    assert x.shape == (4, 4, 41, 6) and list(flen) == [6, 1, 2, 1]
    for b in range(4):
        assert not x[b, :, :, flen[b]:].any()


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', ['fp32', 'bf16'])
@pytest.mark.parametrize('shape', [(3, 4, 7, 1), (5, 4, 41, 53)], ids=['3x4x7x1', '5x4x41x53'])
def test_spec_augment(monkeypatch, shape, dtype):
    Fq = _mods()[0]
    dev = P._dev()

    def fn(ga):
        rng = np.random.RandomState(3)
        x = _t(rng.randn(*shape), dev, DTYPES[dtype])
        lengths = torch.tensor(([shape[3], 0, 1, shape[3] // 2, 2])[:shape[0]], dtype=torch.int32, device=dev)
        out, plan = Fq.spec_augment(x, lengths, time_warp=3, freq_masks=2, freq_width=5, time_masks=2, time_width=12, time_ratio=0.5,
                                    seed=11, return_plan=True)
        return dict(out=out, plan=plan)
    _run_case(monkeypatch, 'spec_augment', fn, '%s %s' % (shape, dtype))


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', ['int16', 'fp32'])
def test_speed_perturb(monkeypatch, dtype):
    Fq = _mods()[0]
    dev = P._dev()

    def fn(ga):
        wave, lengths = _waves(dev, 1200, dtype)
        out, olen, plan = Fq.speed_perturb(wave, lengths, gain=(0.5, 2.0), seed=5, return_plan=True)
        return dict(out=out, out_lengths=olen, plan=plan)
    res = _run_case(monkeypatch, 'speed_perturb', fn, dtype)
    out, olen = res.outputs[0]['out'].cpu().numpy(), res.outputs[0]['out_lengths'].cpu().numpy()
    for b in range(4):
        assert not out[b, olen[b]:].any()                           # zero from out_lengths[b] on


@pytest.mark.gpu
@pytest.mark.parametrize('banks', ['rirs_and_noises', 'noises_only', 'rirs_only'])
@pytest.mark.parametrize('dtype', ['int16', 'fp32'])
def test_noise_reverb(monkeypatch, dtype, banks):
    """qk_noise_reverb with its float64 energy-partial workspace (written by the filter launch, read by the mix launch)."""
    Fq = _mods()[0]
    dev = P._dev()
    rng = np.random.RandomState(21)
    rirs = Fq.prepare_rirs([rng.randn(n) * np.exp(-np.arange(n) / 20.0) for n in (1, 17, 300)], device=dev) if 'rirs' in banks else None
    noises = Fq.prepare_noises([rng.randn(n) * 100 for n in (7, 300, 3000)], device=dev) if 'noises' in banks else None

    def fn(ga):
        wave, lengths = _waves(dev, 2051, dtype)
        out, plan = Fq.noise_reverb(wave, lengths, rirs=rirs, noises=noises, snr=(-5.0, 25.0), seed=4, return_plan=True)
        return dict(out=out, plan=plan)
    res = _run_case(monkeypatch, 'noise_reverb', fn, '%s %s' % (dtype, banks))
    out = res.outputs[0]['out'].cpu().numpy()
    for b, n in enumerate([2051, 1, 401, 0]):
        assert not out[b, n:].any()                                 # zero from lengths[b] on


# ---------------------------------------------------------------------------------------------------------------------
# the optimiser: guarded p, g, m, v, decay, state and workspace; n % 4 == 3
# ---------------------------------------------------------------------------------------------------------------------
N_OPT = 4099
ADAM = dict(lr=5e-4, beta1=0.9, beta2=0.999, eps=1e-7)


def _opt_buffers(ga, dev, seed=0):
    rng = np.random.RandomState(seed)
    mk = lambda a: ga.tensor(a.astype(np.float32), device=dev)
    return dict(p=mk(rng.randn(N_OPT)), g=mk(rng.randn(N_OPT)), m=mk(0.1 * rng.randn(N_OPT)), v=mk(0.01 * rng.rand(N_OPT)),
                decay=mk(np.where(rng.rand(N_OPT) < 0.5, 2e-3, 0.0)))


@pytest.mark.gpu
def test_adam_step_forms(monkeypatch):
    """qk_adam_step, _zero_grad, _l2 and _dev on guarded buffers.  include/qk.h documents 4-byte alignment for qk_grad_guard_reduce
    only (its peeled head); the Adam entry points say nothing of the kind, so their buffers keep the allocator's 256-byte alignment
    here -- an offset view is outside their documented contract."""
    Fq = _mods()[0]
    dev = P._dev()

    def fn(ga):
        out = {}
        for form in ('plain', 'zero_grad', 'l2', 'dev'):
            t = _opt_buffers(ga, dev)
            if form == 'plain':
                Fq.adam_step(t['p'], t['g'], t['m'], t['v'], 3, grad_scale=0.5, **ADAM)
            elif form == 'zero_grad':
                Fq.adam_step(t['p'], t['g'], t['m'], t['v'], 3, grad_scale=0.5, zero_grad=True, **ADAM)
                assert not bool(t['g'].any())
            elif form == 'l2':
                Fq.adam_step(t['p'], t['g'], t['m'], t['v'], 3, grad_scale=0.5, decay=t['decay'], **ADAM)
            else:
                step = ga.zeros(1, dtype=torch.int32, device=dev)
                Fq.adam_step(t['p'], t['g'], t['m'], t['v'], step, grad_scale=0.5, decay=t['decay'], zero_grad=True, **ADAM)
                out['dev/step'] = step
            out.update({'%s/%s' % (form, k): v for k, v in t.items()})
        assert int(out['dev/step']) == 1
        return {}, out
    _run_case(monkeypatch, 'adam', fn)


@pytest.mark.gpu
def test_grad_guard_reduce_norm_and_guarded_step(monkeypatch):
    """qk_grad_guard_reduce (through grad_guard_reduce, grad_norm and training.GradGuard, whose state block and workspace come
    through the proxy) and qk_adam_step_guarded.  include/qk.h gives grad, param and decay of the reduction 4-byte alignment
    ("views at any element offset of a flat buffer"): it is repeated on views that start 1, 2 and 3 elements into a guarded
    payload, and the elements in front of and behind each view must keep the fill."""
    Fq, L, _, training, _ = _mods()
    dev = P._dev()

    def fn(ga):
        out, keep = {}, {}
        t = _opt_buffers(ga, dev)
        guard = training.GradGuard(dev, clipnorm=1.0, clipvalue=0.5, loss_scale=4.0, dynamic=True)
        step = ga.zeros(1, dtype=torch.int32, device=dev)
        guard.step(t['p'], t['g'], t['m'], t['v'], step, grad_scale=0.5, decay=t['decay'], zero_grad=True, **ADAM)
        keep.update(t, step=step, state=guard._state)
        assert int(step) == 1
        norm, bad = Fq.grad_norm(_opt_buffers(ga, dev, 1)['g'])
        out.update(norm=norm, nonfinite=bad)
        for off in (1, 2, 3):
            bufs = {k: ga.empty(N_OPT + 4, dtype=torch.float32, device=dev) for k in ('g', 'p', 'decay')}
            src = _opt_buffers(GA.GuardedAllocator(ga.fill, 'cuda'), dev, 2)
            views = {k: b[off:off + N_OPT] for k, b in bufs.items()}
            for k, view in views.items():
                view.copy_(src[k])
            state = ga.zeros(len(L.GRAD_GUARD_STATE), dtype=torch.float32, device=dev)
            state[0] = 1.0
            Fq.grad_guard_reduce(views['g'], L.GradGuardConfig(), state, views['p'], views['decay'], 0.125)
            keep['state_at_offset_%d' % off] = state
            for k, b in bufs.items():
                raw = b.view(torch.uint8)
                assert bool((raw[:4 * off] == ga.fill).all()) and bool((raw[4 * (off + N_OPT):] == ga.fill).all()), (k, off)
                assert GA.first_bit_difference(views[k], src[k]) is None          # ... and the reduction only read
        return out, keep
    _run_case(monkeypatch, 'grad_guard', fn)
