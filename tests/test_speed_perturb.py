"""On-device speed and volume perturbation (qcnn_amd.functional.speed_perturb, qcnn_amd.features.SpeedPerturb,
csrc/qk_wave_aug.hip) against the NumPy restatement of include/qk.h's "Speed and volume perturbation" section in
tests/speed_perturb_ref.py.
"""
import ctypes
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import speed_perturb_ref as R
from qcnn_amd import _lib as L
from qcnn_amd import data, features
from qcnn_amd import functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULT = ((9, 10), (1, 1), (11, 10))
SPEED_SETS = {
    'default': DEFAULT,
    '2/3': ((2, 3),),
    '3/2': ((3, 2),),
    '31/32,32/31': ((31, 32), (32, 31)),
    '1/2,2/1': ((1, 2), (2, 1)),
    'eight': ((9, 10), (1, 1), (11, 10), (2, 3), (3, 2), (31, 32), (19, 20), (21, 20)),
}
SHAPES = {
    '5x700': ((5, 700), [700, 693, 350, 9, 0]),
    '3x40': ((3, 40), [40, 1, 5]),                      # shorter than Kw
    '2x9001': ((2, 9001), [9001, 8192]),                # several tiles, a length on a power of two
    '1x70001': ((1, 70001), [70001]),
}


@functools.lru_cache(maxsize=None)
def waveform(shape, dtype):
    rng = np.random.RandomState(shape[1])
    if dtype == 'int16':
        x = rng.randint(-32768, 32768, size=shape).astype(np.int16)
    else:
        x = rng.randn(*shape).astype(np.float32)
    x.setflags(write=False)
    return x


def policy_struct(speeds=DEFAULT, gain=(1.0, 1.0), seed=0, zeros=6, rolloff=0.99):
    """A qk_speed_perturb_t filled from the reference's half widths (offsets as speed_perturb_tables lays them out)."""
    pol = L.SpeedPerturbPolicy()
    pol.n_speeds = len(speeds)
    at = 0
    for i, (p, q) in enumerate(speeds):
        kw = R.half_width(p, q, zeros, rolloff)
        pol.num[i], pol.den[i], pol.half_width[i], pol.table_offset[i] = p, q, kw, at
        at += 0 if p == q else q * (2 * kw + 2)
    pol.gain_lo, pol.gain_hi, pol.seed = gain[0], gain[1], seed
    return pol


# ---- CPU: the library's surface ------------------------------------------------------------------------------------------------
def test_library_exports_speed_perturb():
    for name in ('qk_speed_perturb', 'qk_speed_perturb_out_samples'):
        assert name in L.SYMBOLS
        assert hasattr(ctypes.CDLL(L.LIB_PATH), name)
    assert (L.QK_SPEED_MAX_SPEEDS, L.QK_SPEED_MAX_DEN, L.QK_SPEED_MAX_TAPS, L.QK_SPEED_PLAN_WORDS) == (8, 32, 64, 4)
    assert ctypes.sizeof(L.SpeedPerturbPolicy) == 4 + 4 * 8 * 4 + 4 + 4 + 4
    assert L.lib().qk_version() == 103
    pol = policy_struct()
    assert L.lib().qk_speed_perturb_out_samples(32000, ctypes.byref(pol)) == 35556 == R.out_samples(32000)
    assert L.lib().qk_speed_perturb_out_samples(9, ctypes.byref(policy_struct(((3, 2), (1, 1))))) == 9
    assert L.lib().qk_speed_perturb_out_samples(0, ctypes.byref(pol)) == -1
    assert L.lib().qk_speed_perturb_out_samples(100, None) == -1


def test_c_abi_refuses_bad_arguments_without_a_gpu():
    """Every refusal of the header, through raw ctypes: all of them are decided on the host before any launch, so fake (never
    dereferenced) device addresses do."""
    B, N = 2, 1000
    WAVE, LEN, TAB, OUT, OLEN = 0x10000000, 0x20000000, 0x30000000, 0x40000000, 0x50000000
    lib = L.lib()
    good = policy_struct()
    n_out = lib.qk_speed_perturb_out_samples(N, ctypes.byref(good))
    assert n_out == 1112

    def call(pol=good, dtype=L.QK_WAVE_F32, batch=B, n=N, wave=WAVE, lengths=LEN, tables=TAB, n_out=n_out, out=OUT, olen=OLEN, plan=None):
        return lib.qk_speed_perturb(dtype, batch, n, wave, lengths, ctypes.byref(pol) if pol is not None else None, tables, None, n_out,
                                    out, olen, plan, None)

    def changed(name=None, i=None, v=None, **kw):
        """The default policy with one field (or element i of one array field) replaced."""
        pol = policy_struct(**kw)
        if name is not None and i is None:
            setattr(pol, name, v)
        elif name is not None:
            getattr(pol, name)[i] = v
        return pol
    inval = L.QK_ERR_INVALID_ARG
    for pol in (changed('n_speeds', None, 0), changed('n_speeds', None, 9), changed('n_speeds', None, -1),
                changed('num', 0, 0), changed('num', 0, 33), changed('den', 2, 0), changed('den', 2, 33),
                changed('num', 0, 4),                                # 4 / 10 < 1/2
                changed('num', 0, 21),                               # 21 / 10 > 2
                changed('half_width', 0, 0),                         # num != den without a filter
                changed('half_width', 1, 7),                         # num == den with one
                changed('half_width', 0, -1),
                changed('table_offset', 2, -1),
                changed(gain=(float('nan'), 1.0)), changed(gain=(0.5, float('inf'))), changed(gain=(-0.5, 1.0)), changed(gain=(2.0, 1.0))):
        assert call(pol) == inval, lib.qk_last_error()
    assert call(n_out=n_out - 1) == inval and b'out_samples' in lib.qk_last_error()
    assert call(out=WAVE) == inval and b'overlap' in lib.qk_last_error()
    assert call(out=WAVE + 4 * (B * N - 1)) == inval                       # ... by one sample
    assert call(wave=OUT + 4 * (B * n_out - 1)) == inval
    assert call(dtype=L.QK_WAVE_I16, out=WAVE + 2 * B * N - 4) == inval    # int16 rows are half as long: this still overlaps ...
    assert call(dtype=2) == inval
    for kw in (dict(wave=None), dict(lengths=None), dict(pol=None), dict(out=None), dict(olen=None), dict(tables=None)):
        assert call(**kw) == inval, kw
    assert call(batch=0) == inval and call(n=0) == inval and call(batch=-1) == inval
    assert call(wave=WAVE + 2) == inval and call(out=OUT + 2) == inval     # alignment to the element size
    unsup = L.QK_ERR_UNSUPPORTED
    assert call(changed('half_width', 0, 32)) == unsup               # 66 taps
    assert call(n=1 << 26, n_out=1 << 27) == unsup
    big = policy_struct(((1, 1), (1, 2)))
    assert call(big, n=(1 << 25) + 1, n_out=(1 << 26) + 2) == unsup        # out_samples alone reaches 2^26


def test_python_refuses_bad_arguments_and_cpu_tensors_without_a_gpu():
    x = torch.zeros(2, 1000)
    n = [1000, 10]
    for kw in (dict(speeds=()), dict(speeds=((1, 1),) * 9), dict(speeds=((0, 1),)), dict(speeds=((33, 32),)), dict(speeds=((1, 33),)),
               dict(speeds=((4, 10),)), dict(speeds=((21, 10),)), dict(speeds=((9, 10, 11),)), dict(gain=(-1.0, 1.0)), dict(gain=(2.0, 1.0)),
               dict(gain=(float('nan'), 1.0)), dict(gain=(1.0, float('inf'))), dict(gain=1.0), dict(zeros=0), dict(zeros=-6),
               dict(rolloff=0.0), dict(rolloff=1.5), dict(rolloff=float('nan')), dict(seed=-1), dict(seed=2 ** 32),
               ):
        with pytest.raises(ValueError):
            F.speed_perturb(x, n, **kw)
        with pytest.raises(ValueError):
            features.SpeedPerturb(**kw)
    features.SpeedPerturb(speeds=((1, 2),), zeros=16)                      # ceil(16 / 0.99) = 17 -> 36 taps
    with pytest.raises(ValueError, match='taps'):
        features.SpeedPerturb(speeds=((2, 1),), zeros=16)                  # ceil(16 / 0.495) = 33 -> 68 taps
    with pytest.raises(ValueError, match='taps'):
        F.speed_perturb(x, n, speeds=((2, 1),), zeros=16)
    for kw in (dict(speeds=((0.9, 1),)), dict(speeds=(0.9, 1.0, 1.1)), dict(zeros=6.0), dict(seed=1.5), dict(speeds=((True, 1),))):
        with pytest.raises(TypeError):
            F.speed_perturb(x, n, **kw)
        with pytest.raises(TypeError):
            features.SpeedPerturb(**kw)
    with pytest.raises(TypeError):
        F.speed_perturb(x.double(), n)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        F.speed_perturb(x, n)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        features.SpeedPerturb()(x, n)
    with pytest.raises(TypeError):
        features.quaternion_fbank(torch.zeros(2, 1000), wave_augment='speed')
    with pytest.raises(TypeError):
        features.quaternion_fbank(torch.zeros(2, 1000), wave_augment=features.SpecAugment())


def test_policy_state_dict_round_trip_and_checks():
    a = features.SpeedPerturb(seed=5)
    assert a.state_dict() == {'seed': 5, 'counter': 0}
    a.load_state_dict({'seed': 9, 'counter': 0xFFFFFFFF})
    assert a.state_dict() == {'seed': 9, 'counter': 0xFFFFFFFF} and a.seed == 9
    for bad in ({'seed': -1, 'counter': 0}, {'seed': 0, 'counter': 2 ** 32}, {'seed': 0.5, 'counter': 0}, {'seed': 0, 'counter': True}):
        with pytest.raises(ValueError):
            a.load_state_dict(bad)
    assert a.state_dict() == {'seed': 9, 'counter': 0xFFFFFFFF}           # a refused dict changes nothing
    with pytest.raises(KeyError):
        a.load_state_dict({'seed': 1})
    assert a.state_dict() == {'seed': 9, 'counter': 0xFFFFFFFF}


def test_table_facts():
    tab = F.speed_perturb_tables(DEFAULT, 6, 0.99)
    assert tab['num'] == [9, 1, 11] and tab['den'] == [10, 1, 10]
    assert tab['half_width'] == [7, 0, 7] and tab['table_offset'] == [0, 0, 160]
    assert tab['tables'].dtype == np.float32 and tab['tables'].shape == (320,)
    assert F.speed_perturb_tables(DEFAULT, 6, 0.99) is tab                 # cached
    for i, (p, q) in ((0, (9, 10)), (2, (11, 10))):
        t = tab['tables'][tab['table_offset'][i]:][:160].reshape(10, 16)
        assert np.array_equal(t, R.table(p, q))                            # the package's table is the header's, bit for bit
        sums = t.astype(np.float64).sum(axis=1)
        assert np.all(sums >= 1.0000) and np.all(sums <= 1.0010), sums
    only = F.speed_perturb_tables(((1, 1),), 6, 0.99)
    assert only['half_width'] == [0] and only['tables'].size == 0          # num == den has no table
    for (p, q) in ((2, 3), (3, 2), (31, 32), (32, 31), (1, 2), (2, 1)):
        t = F.speed_perturb_tables(((p, q),), 6, 0.99)
        kw = R.half_width(p, q)
        assert t['half_width'] == [kw] and np.array_equal(t['tables'].reshape(q, 2 * kw + 2), R.table(p, q))
    assert R.half_width(2, 1) == 13 and R.half_width(1, 2) == 7


# ---- CPU: hand facts of the reference ------------------------------------------------------------------------------------------
def test_reference_lengths_and_indices():
    for p, q in ((9, 10), (11, 10), (2, 3), (3, 2), (31, 32)):
        for n in (0, 1, 2, 15, 16, 1000):
            n1 = R.out_length(n, p, q)
            assert n1 == int(np.ceil(n * q / p)) and (n1 - 1) * p < n * q <= n1 * p or n == n1 == 0
            for m in range(n1):
                assert (m * p) // q <= n - 1
            y, S = R.resample_row(np.ones(n), n, p, q, np.float32(1), n1 + 3)
            assert not y[n1:].any() and not S[n1:].any()
    assert R.plan_row(0, 2000, 1000)[0] == 1000 and R.plan_row(0, -5, 1000)[0] == 0             # the clamp
    assert R.out_samples(1000) == 1112 and R.out_samples(1000, ((3, 2), (1, 1))) == 1000


def test_reference_passband_accuracy():
    """The filter and its orientation (r / q - j), independently of the kernel: a sine below the cut-off comes out as the same sine
    on the new time axis.  The issue's bound: 5e-3 over the interior (computed with this filter: at most 2.9e-3, at 3/2, f = 0.2)."""
    n = 2000
    worst = 0.0
    for p, q in ((9, 10), (11, 10), (2, 3), (3, 2)):
        for f in (0.01, 0.05, 0.125, 0.2):
            x = np.sin(2 * np.pi * f * np.arange(n))
            n1 = R.out_length(n, p, q)
            y, _ = R.resample_row(x, n, p, q, np.float32(1), n1)
            m = np.arange(n1)[40:-40]
            err = np.abs(y[40:-40] - np.sin(2 * np.pi * f * m * p / q)).max()
            worst = max(worst, err)
            assert err <= 5e-3, (p, q, f, err)
    print('passband: worst interior error %.3g' % worst)


def test_reference_draw_distribution():
    rows = [R.plan_row(b, 1, 1, DEFAULT, (0.5, 2.0), seed=11) for b in range(4096)]
    counts = np.bincount([r[1] for r in rows], minlength=3)
    sd = np.sqrt(4096 * (1 / 3) * (2 / 3))
    assert counts.sum() == 4096 and len(counts) == 3 and np.all(np.abs(counts - 4096 / 3) <= 5 * sd), counts
    g = np.array([r[3] for r in rows])
    assert g.dtype == np.float32 and np.all(g >= 0.5) and np.all(g < 2.0) and g.min() < 0.51 and g.max() > 1.99
    assert len(np.unique(g)) > 4000
    assert all(R.plan_row(b, 1, 1, DEFAULT, (0.75, 0.75), seed=b)[3] == np.float32(0.75) for b in range(64))       # lo == hi: constant


# ---- device (GPU) --------------------------------------------------------------------------------------------------------------
def _dev():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    return torch.device('cuda:0')


def check_values(x, lengths, out, out_lengths, plan, speeds, **policy):
    """out / out_lengths / plan: the device's, as NumPy.  Integers exact; values within the fp32 dot-product bound
    (K + 2) 2^-24 S with K = 2 Kw + 2 taps (gamma_K sum |h x|, plus one rounding for the gain), S from the device's own g."""
    gains = plan[:, 3].copy().view(np.float32)
    ref = R.speed_perturb(x, lengths, speeds=speeds, gains=gains, width=out.shape[1], **policy)
    assert np.array_equal(plan[:, 0], ref['n']) and np.array_equal(plan[:, 1], ref['i']) and np.array_equal(plan[:, 2], ref['n1'])
    assert np.array_equal(out_lengths, ref['out_lengths'])
    assert out.shape[1] == R.out_samples(x.shape[1], speeds)
    worst = 0.0
    for b in range(x.shape[0]):
        p, q = speeds[ref['i'][b]]
        K = 2 * R.half_width(p, q, policy.get('zeros', 6), policy.get('rolloff', 0.99)) + 2
        n1 = ref['n1'][b]
        assert np.array_equal(out[b, n1:].view(np.int32), np.zeros(out.shape[1] - n1, dtype=np.int32))       # +0 exactly, not NaN
        err = np.abs(out[b].astype(np.float64) - ref['y'][b])
        bound = (K + 2) * 2.0 ** -24 * ref['S'][b]
        assert np.all(out[b][ref['S'][b] == 0] == 0)
        assert np.all(err <= bound), (b, p, q, float((err / np.maximum(bound, 1e-300)).max()))
        if n1:
            worst = max(worst, float((err[:n1] / np.maximum(bound[:n1], 1e-300)).max()))
    print('worst error / bound: %.3f' % worst)
    return ref


PLAN_LENGTHS = ([0, 1, 2, 15, 16, 17, 999, 1000, 1200] * 8)[:67]


@pytest.mark.gpu
@pytest.mark.parametrize('seed', [0, 1, 0xFFFFFFFF])
def test_plan_parity(seed):
    dev = _dev()
    B, N = 67, 1000
    x = torch.zeros(B, N, device=dev)
    lengths = torch.tensor(PLAN_LENGTHS, dtype=torch.int32, device=dev)
    gain = (0.5, 2.0)
    plans = []
    for counter in (0, 7):
        cdev = torch.tensor([counter], dtype=torch.int32, device=dev)
        out, olen, plan = F.speed_perturb(x, lengths, gain=gain, seed=seed, counter=cdev, return_plan=True)
        assert plan.dtype == torch.int32 and tuple(plan.shape) == (B, 4) and olen.dtype == torch.int32 and tuple(olen.shape) == (B,)
        assert tuple(out.shape) == (B, 1112) and out.dtype == torch.float32
        p = plan.cpu().numpy()
        rows = [R.plan_row(b, PLAN_LENGTHS[b], N, DEFAULT, gain, seed, counter) for b in range(B)]
        assert np.array_equal(p[:, :3], np.array([r[:3] for r in rows]))
        assert np.array_equal(olen.cpu().numpy(), [r[2] for r in rows])
        want = np.array([r[3] for r in rows], dtype=np.float32)
        got = p[:, 3].copy().view(np.float32)
        assert np.all(np.abs(got.astype(np.float64) - want) <= 2 * np.spacing(want)), (seed, counter)
        plans.append(p)
        if counter == 0:
            p0 = F.speed_perturb(x, lengths, gain=gain, seed=seed, counter=None, return_plan=True)[2]
            assert torch.equal(p0, plan)
    assert not np.array_equal(plans[0], plans[1])
    assert set(plans[0][:, 1]) == {0, 1, 2}


@pytest.mark.gpu
def test_device_draw_distribution():
    dev = _dev()
    x = torch.zeros(4096, 1, dtype=torch.int16, device=dev)
    plan = F.speed_perturb(x, torch.ones(4096, dtype=torch.int32, device=dev), gain=(0.5, 2.0), seed=11, return_plan=True)[2].cpu().numpy()
    counts = np.bincount(plan[:, 1], minlength=3)
    sd = np.sqrt(4096 * (1 / 3) * (2 / 3))
    assert counts.sum() == 4096 and len(counts) == 3 and np.all(np.abs(counts - 4096 / 3) <= 5 * sd), counts
    g = plan[:, 3].copy().view(np.float32)
    assert np.all(g >= 0.5) and np.all(g < 2.0)


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', ['int16', 'float32'])
@pytest.mark.parametrize('speeds', list(SPEED_SETS))
@pytest.mark.parametrize('shape', list(SHAPES))
def test_value_parity(shape, speeds, dtype):
    dev = _dev()
    (B, N), lengths = SHAPES[shape]
    x = waveform((B, N), dtype)
    policy = dict(gain=(0.5, 2.0), seed=list(SHAPES).index(shape) * 16 + list(SPEED_SETS).index(speeds))
    out, olen, plan = F.speed_perturb(torch.from_numpy(x.copy()).to(dev), lengths, speeds=SPEED_SETS[speeds], return_plan=True, **policy)
    check_values(x, lengths, out.cpu().numpy(), olen.cpu().numpy(), plan.cpu().numpy(), SPEED_SETS[speeds], **policy)


@pytest.mark.gpu
def test_every_speed_of_the_set_of_eight_and_other_filters():
    dev = _dev()
    x = waveform((40, 300), 'float32')
    lengths = [300 - 7 * b for b in range(40)]
    speeds = SPEED_SETS['eight']
    out, olen, plan = F.speed_perturb(torch.from_numpy(x.copy()).to(dev), lengths, speeds=speeds, seed=3, return_plan=True)
    ref = check_values(x, lengths, out.cpu().numpy(), olen.cpu().numpy(), plan.cpu().numpy(), speeds, seed=3)
    assert set(ref['i']) == set(range(8))
    for policy in (dict(zeros=3, rolloff=0.9), dict(zeros=15, rolloff=1.0)):                      # 3/2 with Z = 15: Kw = 23, 48 taps
        out, olen, plan = F.speed_perturb(torch.from_numpy(x.copy()).to(dev), lengths, speeds=((2, 3), (3, 2)), return_plan=True, **policy)
        check_values(x, lengths, out.cpu().numpy(), olen.cpu().numpy(), plan.cpu().numpy(), ((2, 3), (3, 2)), **policy)


@pytest.mark.gpu
def test_lengths_are_clamped():
    dev = _dev()
    x = waveform((5, 700), 'float32')
    lengths = [5000, -3, 701, 700, 2 ** 31 - 1]
    out, olen, plan = F.speed_perturb(torch.from_numpy(x.copy()).to(dev), lengths, seed=2, return_plan=True)
    ref = check_values(x, lengths, out.cpu().numpy(), olen.cpu().numpy(), plan.cpu().numpy(), DEFAULT, seed=2)
    assert ref['n'] == [700, 0, 700, 700, 700]


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', ['int16', 'float32'])
def test_padding_never_leaks(dtype):
    """Samples >= n hold NaN (float32) or 32767 (int16) and `out` is pre-filled with NaN (hence the raw C call: the caller owns
    `out`): the valid outputs match the reference, which never touches those samples, and everything from n' on is exactly 0."""
    dev = _dev()
    (B, N), lengths = SHAPES['5x700']
    x = waveform((B, N), dtype).copy()
    for b, n in enumerate(lengths):
        x[b, n:] = 32767 if dtype == 'int16' else np.nan
    xd = torch.from_numpy(x).to(dev)
    ld = torch.tensor(lengths, dtype=torch.int32, device=dev)
    for speeds in (DEFAULT, ((2, 3), (3, 2), (1, 1))):
        pol = policy_struct(speeds, seed=9)
        tables = torch.from_numpy(F.speed_perturb_tables(speeds, 6, 0.99)['tables'].copy()).to(dev)
        n_out = R.out_samples(N, speeds)
        out = torch.full((B, n_out), float('nan'), device=dev)
        olen = torch.full((B,), -1, dtype=torch.int32, device=dev)
        plan = torch.full((B, 4), -1, dtype=torch.int32, device=dev)
        rc = L.lib().qk_speed_perturb(L.QK_WAVE_I16 if dtype == 'int16' else L.QK_WAVE_F32, B, N, xd.data_ptr(), ld.data_ptr(), ctypes.byref(pol),
                                      tables.data_ptr(), None, n_out, out.data_ptr(), olen.data_ptr(), plan.data_ptr(),
                                      torch.cuda.current_stream().cuda_stream)
        assert rc == 0, L.lib().qk_last_error()
        o = out.cpu().numpy()
        assert np.all(np.isfinite(o))
        ref = check_values(x, lengths, o, olen.cpu().numpy(), plan.cpu().numpy(), speeds, seed=9)
        for b in range(B):
            assert not o[b, ref['n1'][b]:].any()
        assert len(set(ref['i'])) > 1


@pytest.mark.gpu
def test_identity_and_constant_gain():
    dev = _dev()
    lengths = [700, 693, 350, 9, 0]
    for dtype in ('int16', 'float32'):
        x = waveform((5, 700), dtype).copy()
        if dtype == 'float32':
            x[0, :2] = [-0.0, np.inf]
        xd = torch.from_numpy(x).to(dev)
        for view in (xd, xd.reshape(-1)[1:1 + 4 * 700].reshape(4, 700)):                        # the second is not 16-byte aligned
            n = lengths[:view.shape[0]]
            out, olen = F.speed_perturb(view, n, speeds=((1, 1),))
            assert tuple(out.shape) == tuple(view.shape) and olen.tolist() == n
            half = F.speed_perturb(view, n, speeds=((1, 1),), gain=(0.5, 0.5))[0]
            for b, nb in enumerate(n):
                want = view[b, :nb].float()
                assert torch.equal(out[b, :nb].view(torch.int32), want.view(torch.int32))       # a bit copy
                assert torch.equal(half[b, :nb].view(torch.int32), (want * 0.5).view(torch.int32))
                assert not out[b, nb:].any() and not half[b, nb:].any()


@pytest.mark.gpu
def test_determinism():
    dev = _dev()
    x = torch.from_numpy(waveform((5, 700), 'int16').copy()).to(dev)
    lengths = [700, 693, 350, 9, 0]
    policy = dict(gain=(0.5, 2.0), seed=6)
    c3 = torch.full((1,), 3, dtype=torch.int32, device=dev)
    a = F.speed_perturb(x, lengths, counter=c3, return_plan=True, **policy)
    b = F.speed_perturb(x, lengths, counter=c3.clone(), return_plan=True, **policy)
    assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    c = F.speed_perturb(x, lengths, counter=c3 + 1, return_plan=True, **policy)
    assert not torch.equal(a[2], c[2])
    d = F.speed_perturb(x, lengths, counter=c3.view(torch.uint32), return_plan=True, **policy)
    assert torch.equal(d[2], a[2])
    e = F.speed_perturb(x, lengths, counter=c3, return_plan=True, **dict(policy, seed=7))
    assert not torch.equal(a[2], e[2])


@pytest.mark.gpu
def test_graph_capture_draws_anew_on_every_replay():
    dev = _dev()
    x = torch.from_numpy(waveform((5, 700), 'int16').copy()).to(dev)
    lengths = torch.tensor([700, 693, 350, 9, 0], dtype=torch.int32, device=dev)
    policy = dict(gain=(0.5, 2.0), seed=7)
    sp = features.SpeedPerturb(**policy)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        sp(x, lengths)                                                     # warm-up: the counter and the tables now live on the device
    torch.cuda.current_stream().wait_stream(side)
    assert sp.state_dict()['counter'] == 1
    c = 5
    sp.load_state_dict({'seed': 7, 'counter': c})
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                          # one stream, no parallel branches
        out, olen = sp(x, lengths)
        plan = sp.last_plan
    seen = []
    for k in range(3):
        graph.replay()
        seen.append((out.clone(), olen.clone(), plan.clone()))
    torch.cuda.synchronize()
    xn, ln = x.cpu().numpy(), lengths.cpu().numpy()
    for k, (o, ol, p) in enumerate(seen):
        ck = torch.tensor([c + k], dtype=torch.int32, device=dev)
        eo, eol, ep = F.speed_perturb(x, lengths, counter=ck, return_plan=True, **policy)
        assert torch.equal(o.view(torch.int32), eo.view(torch.int32)) and torch.equal(ol, eol) and torch.equal(p, ep), k
        check_values(xn, ln, o.cpu().numpy(), ol.cpu().numpy(), p.cpu().numpy(), DEFAULT, counter=c + k, **policy)
    assert not torch.equal(seen[0][2], seen[1][2]) and not torch.equal(seen[1][2], seen[2][2]) and not torch.equal(seen[0][2], seen[2][2])
    assert sp.state_dict() == {'seed': 7, 'counter': c + 3}


@pytest.mark.gpu
def test_quaternion_fbank_wave_augment():
    from test_fbank import signals
    dev = _dev()
    n = [16000, 9000, 4001, 401]
    wave = torch.from_numpy(signals(n, seed=6)).to(dev)
    policy = dict(gain=(0.5, 2.0), seed=8)
    for norm, dt in ((None, torch.float32), ('utterance', torch.bfloat16)):
        sp = features.SpeedPerturb(**policy)
        got, gfl = features.quaternion_fbank(wave, n, normalize=norm, dtype=dt, wave_augment=sp)
        pw, pl, plan = F.speed_perturb(wave, n, return_plan=True, **policy)
        want, wfl = features.quaternion_fbank(pw, pl, normalize=norm, dtype=dt)
        assert got.dtype == dt and torch.equal(gfl, wfl) and torch.equal(sp.last_plan, plan) and sp.state_dict()['counter'] == 1
        assert torch.equal(got.view(torch.int32 if dt == torch.float32 else torch.int16), want.view(torch.int32 if dt == torch.float32 else torch.int16))
        assert got.shape[3] == features.num_frames(R.out_samples(16000))
        assert gfl.tolist() == [features.num_frames(v) for v in pl.tolist()]
        assert pl.tolist() == [R.plan_row(b, n[b], 16000, DEFAULT, seed=8)[2] for b in range(4)]
        none = features.quaternion_fbank(wave, n, normalize=norm, dtype=dt, wave_augment=None)
        plain = features.quaternion_fbank(wave, n, normalize=norm, dtype=dt)
        assert torch.equal(none[0], plain[0]) and torch.equal(none[1], plain[1]) and none[0].shape != got.shape
        # with SpecAugment behind it
        sa = features.SpecAugment(time_warp=3, freq_masks=1, freq_width=4, time_masks=1, time_width=10, seed=2)
        both = features.quaternion_fbank(wave, n, normalize=norm, dtype=dt, wave_augment=features.SpeedPerturb(**policy), augment=sa)
        want32, wfl = features.quaternion_fbank(pw, pl, normalize=norm, dtype=torch.float32)
        assert torch.equal(both[0], F.spec_augment(want32, wfl, dtype=dt, **sa.policy)) and torch.equal(both[1], wfl)


@pytest.mark.gpu
def test_train_timit_example_with_speed_perturb(tmp_path):
    from test_fbank import signals, sphere_bytes
    _dev()
    rng = np.random.RandomState(0)
    for split, spk, utt in (('TRAIN', 'FCJF0', 'SA1'), ('TRAIN', 'MDAB0', 'SX9'), ('TEST', 'MDAB1', 'SI2')):
        d = tmp_path / split / 'DR1' / spk
        d.mkdir(parents=True, exist_ok=True)
        n = int(rng.randint(14000, 20000))
        (d / (utt + '.WAV')).write_bytes(sphere_bytes(signals([n], seed=int(rng.randint(1000)))[0].astype(np.int16)))
        phones = [data.TIMIT_PHONES_61[i] for i in rng.randint(0, 61, size=12)]
        cuts = np.linspace(0, n, len(phones) + 1).astype(int)
        (d / (utt + '.PHN')).write_text(''.join('%d %d %s\n' % (cuts[i], cuts[i + 1], p) for i, p in enumerate(phones)))
    cmd = [sys.executable, os.path.join(ROOT, 'examples', 'train_timit.py'), '--timit', str(tmp_path), '--speed-perturb', '--volume', '0.5,2',
           '--steps', '2', '--eval-every', '2', '--layers', '4', '--batch', '2']
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, env=dict(os.environ), timeout=600, universal_newlines=True)
    assert r.returncode == 0, r.stdout[-4000:]
    losses = re.findall(r'step\s+\d+\s+loss (\S+)', r.stdout)
    assert len(losses) == 2, r.stdout[-4000:]
    assert all(np.isfinite(float(v)) for v in losses)
    assert len(re.findall(r'held-out ctc cost (\S+)', r.stdout)) == 1
