"""On-device reverberation and additive noise (qcnn_amd.functional.noise_reverb, qcnn_amd.features.NoiseReverb,
csrc/qk_env_aug.hip) against the NumPy restatement of include/qk.h's "Reverberation and additive noise" section in
tests/noise_reverb_ref.py.
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

import noise_reverb_ref as R
from qcnn_amd import _lib as L
from qcnn_amd import data, features
from qcnn_amd import functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_MAX = 9001
LENGTHS = [0, 1, 9, 200, 2047, 2048, 2049, 9001]               # 200 is shorter than the responses of 300, 513 and 1025 taps
RIR_TAPS = (1, 2, 17, 300, 513, 1025)
RIR_DELAY = (0, 1, 5, 0, 512, 5)                                 # 0, 5 and Lr - 1
NOISE_LEN = (1, 7, 300, 12000)                                   # 300 wraps many times, 12000 > n


@functools.lru_cache(maxsize=None)
def waveform(shape, dtype):
    rng = np.random.RandomState(shape[1])
    if dtype == 'int16':
        x = rng.randint(-32768, 32768, size=shape).astype(np.int16)
    else:
        x = rng.randn(*shape).astype(np.float32)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def rir_bank(which=None, pad=0.0):
    """(bank, rir_len, rir_delay) as NumPy, written by hand (delays that are not at the peak): all of RIR_TAPS, or the one response
    `which`; `pad` fills the rows behind rir_len."""
    taps = RIR_TAPS if which is None else (RIR_TAPS[which],)
    delay = RIR_DELAY if which is None else (RIR_DELAY[which],)
    rng = np.random.RandomState(7)
    bank = np.full((len(taps), 1025 + 3), pad, dtype=np.float32)
    for i, lr in enumerate(taps):
        h = rng.randn(lr) * np.exp(-np.arange(lr) / 200.0)
        bank[i, :lr] = (h / np.sqrt(np.sum(h * h))).astype(np.float32)
    out = bank, np.array(taps, dtype=np.int32), np.array(delay, dtype=np.int32)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def noise_bank(pad=0.0):
    rng = np.random.RandomState(8)
    bank = np.full((len(NOISE_LEN), max(NOISE_LEN) + 5), pad, dtype=np.float32)
    for i, ln in enumerate(NOISE_LEN):
        bank[i, :ln] = (rng.randn(ln) * (i + 1)).astype(np.float32)
    out = bank, np.array(NOISE_LEN, dtype=np.int32)
    for a in out:
        a.setflags(write=False)
    return out


def as_tensors(bank, dev=None):
    return None if bank is None else tuple(torch.from_numpy(a.copy()).to(dev) if dev is not None else torch.from_numpy(a.copy()) for a in bank)


def policy_struct(n_rirs=2, rir_stride=100, n_noises=3, noise_stride=500, rir_prob=1 << 23, noise_prob=1 << 24, snr=(5.0, 20.0), seed=0):
    return L.NoiseReverbPolicy(n_rirs, rir_stride, n_noises, noise_stride, rir_prob, noise_prob, snr[0], snr[1], seed)


# ---- CPU: the library's surface ------------------------------------------------------------------------------------------------
def test_library_exports_noise_reverb():
    for name in ('qk_noise_reverb', 'qk_noise_reverb_workspace_bytes'):
        assert name in L.SYMBOLS
        assert hasattr(ctypes.CDLL(L.LIB_PATH), name)
    assert (L.QK_REVERB_MAX_TAPS, L.QK_NOISE_REVERB_PLAN_WORDS) == (8192, 8)
    header = open(os.path.join(ROOT, 'include', 'qk.h')).read()
    assert '#define QK_REVERB_MAX_TAPS 8192' in header and '#define QK_NOISE_REVERB_PLAN_WORDS 8' in header
    body = header[header.index('typedef struct qk_noise_reverb_t {'):header.index('} qk_noise_reverb_t;')]
    fields = re.findall(r'(?:int32_t|uint32_t|float)\s+([a-z_0-9, ]+);', body)
    assert [f.strip() for group in fields for f in group.split(',')] == [f[0] for f in L.NoiseReverbPolicy._fields_]
    assert ctypes.sizeof(L.NoiseReverbPolicy) == 9 * 4
    lib = L.lib()
    assert lib.qk_noise_reverb_workspace_bytes(1, 1) == 16                  # one (Es, En) float64 pair per tile
    assert lib.qk_noise_reverb_workspace_bytes(256, 32000) == 256 * 8 * 16
    assert lib.qk_noise_reverb_workspace_bytes(0, 100) == -1 and lib.qk_noise_reverb_workspace_bytes(1, 0) == -1
    assert lib.qk_noise_reverb_workspace_bytes(1, 1 << 26) == -1


def test_c_abi_refuses_bad_arguments_without_a_gpu():
    """Every refusal of the header, through raw ctypes, one argument or field changed at a time: all of them are decided on the host
    before any launch, so fake (never dereferenced) device addresses do."""
    B, N = 2, 1000
    WAVE, LEN, OUT, WS = 0x10000000, 0x20000000, 0x40000000, 0x50000000
    RIR, RLEN, RDEL, NOI, NLEN = 0x60000000, 0x61000000, 0x62000000, 0x70000000, 0x71000000
    lib = L.lib()
    need = lib.qk_noise_reverb_workspace_bytes(B, N)
    assert need == 32

    def call(pol=policy_struct(), dtype=L.QK_WAVE_F32, batch=B, n=N, wave=WAVE, lengths=LEN, rirs=RIR, rlen=RLEN, rdel=RDEL, noises=NOI,
             nlen=NLEN, counter=None, out=OUT, plan=None, ws=WS, ws_bytes=need):
        return lib.qk_noise_reverb(dtype, batch, n, wave, lengths, ctypes.byref(pol) if pol is not None else None, rirs, rlen, rdel, noises,
                                   nlen, counter, out, plan, ws, ws_bytes, None)
    inval, unsup = L.QK_ERR_INVALID_ARG, L.QK_ERR_UNSUPPORTED
    for kw in (dict(wave=None), dict(lengths=None), dict(pol=None), dict(out=None), dict(ws=None),
               dict(batch=0), dict(batch=-1), dict(n=0), dict(n=-5), dict(dtype=2), dict(dtype=-1),
               dict(pol=policy_struct(n_rirs=-1)), dict(pol=policy_struct(n_noises=-1)),
               dict(rirs=None), dict(rlen=None), dict(rdel=None), dict(noises=None), dict(nlen=None),
               dict(pol=policy_struct(rir_stride=0)), dict(pol=policy_struct(noise_stride=0)), dict(pol=policy_struct(noise_stride=-3)),
               dict(pol=policy_struct(rir_prob=-1)), dict(pol=policy_struct(rir_prob=(1 << 24) + 1)),
               dict(pol=policy_struct(noise_prob=-1)), dict(pol=policy_struct(noise_prob=(1 << 24) + 1)),
               dict(pol=policy_struct(snr=(float('nan'), 20.0))), dict(pol=policy_struct(snr=(5.0, float('inf')))),
               dict(pol=policy_struct(snr=(float('-inf'), 5.0))), dict(pol=policy_struct(snr=(20.0, 5.0))),
               dict(out=WAVE), dict(out=WAVE + 4 * (B * N - 1)), dict(wave=OUT + 4 * (B * N - 1)),
               dict(dtype=L.QK_WAVE_I16, out=WAVE + 2 * B * N - 4),
               dict(ws_bytes=need - 1), dict(ws_bytes=0), dict(ws_bytes=-1),
               dict(wave=WAVE + 2), dict(dtype=L.QK_WAVE_I16, wave=WAVE + 1), dict(out=OUT + 2), dict(lengths=LEN + 2), dict(ws=WS + 4),
               dict(rirs=RIR + 2), dict(rlen=RLEN + 1), dict(rdel=RDEL + 2), dict(noises=NOI + 1), dict(nlen=NLEN + 2),
               dict(plan=0x30000002), dict(counter=0x30000002)):
        assert call(**kw) == inval, (kw, lib.qk_last_error())
    assert call(out=WAVE) == inval and b'overlap' in lib.qk_last_error()
    assert call(ws_bytes=need - 1) == inval and b'workspace' in lib.qk_last_error()
    assert call(pol=policy_struct(rir_stride=8193)) == unsup and b'taps' in lib.qk_last_error()
    assert call(n=1 << 26, ws_bytes=1 << 40) == unsup and b'2^26' in lib.qk_last_error()
    # what the header allows: empty banks with NULL pointers are no error of their own (the next refusal is the workspace's)
    none = policy_struct(n_rirs=0, rir_stride=1, n_noises=0, noise_stride=1)
    assert call(pol=none, rirs=None, rlen=None, rdel=None, noises=None, nlen=None, ws_bytes=0) == inval and b'workspace' in lib.qk_last_error()
    assert call(pol=policy_struct(rir_stride=8192, rir_prob=0, noise_prob=0, snr=(7.0, 7.0)), ws_bytes=0) == inval and b'workspace' in lib.qk_last_error()


def test_python_refuses_bad_arguments_and_cpu_tensors_without_a_gpu():
    x = torch.zeros(2, 1000)
    n = [1000, 10]
    rirs, noises = as_tensors(rir_bank()), as_tensors(noise_bank())
    for kw in (dict(rir_prob=-0.1), dict(rir_prob=1.5), dict(noise_prob=float('nan')), dict(noise_prob=2), dict(rir_prob=True), dict(rir_prob='1'),
               dict(snr=(20.0, 5.0)), dict(snr=(float('nan'), 5.0)), dict(snr=(5.0, float('inf'))), dict(snr=5.0), dict(snr=(1.0, 2.0, 3.0)),
               dict(seed=-1), dict(seed=2 ** 32),
               dict(rirs=(rirs[0][0], rirs[1], rirs[2])),                                       # a vector, not a matrix
               dict(rirs=(rirs[0], rirs[1][:2], rirs[2])),                                      # one length per row
               dict(rirs=(torch.zeros(1, 8193), torch.ones(1, dtype=torch.int32), torch.zeros(1, dtype=torch.int32))),       # too many taps
               dict(noises=(noises[0][:0], noises[1][:0]))):
        with pytest.raises(ValueError):
            F.noise_reverb(x, n, **dict(dict(rirs=rirs, noises=noises), **kw))
        with pytest.raises(ValueError):
            features.NoiseReverb(**dict(dict(rirs=rirs, noises=noises), **kw))
    for kw in (dict(seed=1.5), dict(seed=True), dict(rirs=rirs[:2]), dict(rirs=rirs[0]), dict(noises='noise'), dict(noises=rirs),
               dict(rirs=(rirs[0].double(), rirs[1], rirs[2])), dict(noises=(noises[0], noises[1].long())),
               dict(rirs=tuple(t.numpy() for t in rirs))):
        with pytest.raises(TypeError):
            F.noise_reverb(x, n, **dict(dict(rirs=rirs, noises=noises), **kw))
        with pytest.raises(TypeError):
            features.NoiseReverb(**dict(dict(rirs=rirs, noises=noises), **kw))
    with pytest.raises(TypeError):
        F.noise_reverb(x.double(), n, rirs=rirs)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        F.noise_reverb(x, n, rirs=rirs, noises=noises)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        F.noise_reverb(x.short(), n)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        features.NoiseReverb(rirs=rirs, noises=noises)(x, n)


def test_quaternion_fbank_wave_augment_forms_without_a_gpu():
    """The tuple / list form is taken (the call then gets as far as the CPU-tensor refusal); anything else is a TypeError."""
    x = torch.zeros(2, 1000)
    sp, nr = features.SpeedPerturb(), features.NoiseReverb(rirs=as_tensors(rir_bank()))
    for ok in (None, sp, nr, (sp, nr), [sp, nr], (nr,), ()):
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            features.quaternion_fbank(x, wave_augment=ok)
    for bad in ('speed', features.SpecAugment(), (sp, 'noise'), (sp, features.SpecAugment()), [None], 3, ((sp, nr),)):
        with pytest.raises(TypeError):
            features.quaternion_fbank(x, wave_augment=bad)


def test_prepare_rirs_and_noises_facts():
    rng = np.random.RandomState(0)
    h0 = np.concatenate([np.zeros(3), [0.5, -2.0, 2.0, 0.1]])               # the FIRST peak of |h| is sample 4
    h1 = rng.randn(9000)
    h1[10] = 100.0
    h2 = np.array([-3.0])
    bank, length, delay = F.prepare_rirs([h0, h1, h2])
    assert bank.dtype == torch.float32 and length.dtype == torch.int32 and delay.dtype == torch.int32 and not bank.is_cuda
    assert tuple(bank.shape) == (3, 8192) and length.tolist() == [7, 8192, 1] and delay.tolist() == [4, 10, 0]      # cut at 8192 taps
    b = bank.numpy().astype(np.float64)
    assert np.allclose((b * b).sum(axis=1), 1.0, rtol=0, atol=1e-6)          # unit energy (after the fp32 rounding)
    assert not b[0, 7:].any() and not b[2, 1:].any()                         # zero padding
    assert np.array_equal(bank[0, :7].numpy(), (h0 / np.sqrt(np.sum(h0 * h0))).astype(np.float32))       # float64, rounded once
    assert np.array_equal(bank[1].numpy(), (h1[:8192] / np.sqrt(np.sum(h1[:8192] ** 2))).astype(np.float32))
    assert bank[2, 0].item() == -1.0
    cut = F.prepare_rirs([h0, h1], max_taps=5)
    assert tuple(cut[0].shape) == (2, 5) and cut[1].tolist() == [5, 5] and cut[2].tolist() == [4, int(np.argmax(np.abs(h1[:5])))]
    assert np.allclose((cut[0].numpy().astype(np.float64) ** 2).sum(axis=1), 1.0, atol=1e-6)
    for bad in ([], [np.zeros(4)], [np.zeros((2, 2))], [np.array([1.0, np.nan])], [np.zeros(0)]):
        with pytest.raises(ValueError):
            F.prepare_rirs(bad)
    with pytest.raises(ValueError):
        F.prepare_rirs([np.concatenate([np.zeros(5), [1.0]])], max_taps=5)   # nothing left after the cut
    with pytest.raises(ValueError):
        F.prepare_rirs([h0], max_taps=8193)
    with pytest.raises(TypeError):
        F.prepare_rirs([np.array([1, 2, 3])])                                # integers are no impulse response
    with pytest.raises(TypeError):
        F.prepare_rirs(h0)
    nb, nl = F.prepare_noises([np.array([1, -2, 3], dtype=np.int16), rng.randn(10)])
    assert nb.dtype == torch.float32 and tuple(nb.shape) == (2, 10) and nl.tolist() == [3, 10] and nb[0].tolist() == [1, -2, 3] + [0] * 7
    with pytest.raises(ValueError):
        F.prepare_noises([])
    # the synthetic banks: usable as they come
    rirs = features.synthetic_rirs(5, seed=3)
    assert len(rirs) == 5 and all(h.dtype == np.float64 and h.ndim == 1 for h in rirs)
    assert all(np.array_equal(a, b) for a, b in zip(rirs, features.synthetic_rirs(5, seed=3)))
    bank, length, delay = F.prepare_rirs(rirs)
    for i, h in enumerate(rirs):
        assert h[delay[i]] == 1.0 and not h[:delay[i]].any() and delay[i] <= 32          # the unit direct path, within 2 ms
        assert 0.2 * 16000 <= h.size - delay[i] <= 0.8 * 16000 + 1
        assert np.sum(h[delay[i] + 1:] ** 2) <= 1.0 + 1e-9                                # reverberant energy at most the direct one
    noises = features.synthetic_noises(4, 4096, seed=1)
    assert all(v.shape == (4096,) and abs(np.mean(v * v) - 1.0) < 1e-9 for v in noises)
    spec = np.abs(np.fft.rfft(noises[1])) ** 2                               # 1/f: the lowest octaves carry more than the highest
    assert spec[1:65].mean() > 10 * spec[1024:2049].mean()
    white = np.abs(np.fft.rfft(noises[0])) ** 2
    assert 0.5 < white[1:65].mean() / white[1024:2049].mean() < 2.0


def test_policy_state_dict_round_trip_and_checks():
    a = features.NoiseReverb(noises=as_tensors(noise_bank()), seed=5)
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
    assert features.NoiseReverb().policy['rir_prob'] == 0.5 and features.NoiseReverb().policy['snr'] == (5.0, 20.0)


# ---- CPU: hand facts of the reference ------------------------------------------------------------------------------------------
def test_reference_unit_impulse_and_alignment():
    x = waveform((3, 500), 'float32')
    lengths = [500, 77, 0]
    unit = (np.array([[1.0, 9.0]], dtype=np.float32), np.array([1], dtype=np.int32), np.array([0], dtype=np.int32))
    ref = R.noise_reverb(x, lengths, rirs=unit)
    for b, n in enumerate(lengths):
        assert np.array_equal(ref['r'][b], x[b, :n].astype(np.float64)) and np.array_equal(ref['out'][b, :n], ref['r'][b])
        assert not ref['out'][b, n:].any()
    # a delayed impulse with the delay at the impulse is the identity too; with delay 0 it shifts the signal and zero-fills
    late = (np.array([[0.0, 0.0, 1.0]], dtype=np.float32), np.array([3], dtype=np.int32), np.array([2], dtype=np.int32))
    assert np.array_equal(R.noise_reverb(x, lengths, rirs=late)['r'][0], x[0].astype(np.float64))
    shift = (late[0], late[1], np.array([0], dtype=np.int32))
    r = R.noise_reverb(x, lengths, rirs=shift)['r'][1]
    assert np.array_equal(r[2:], x[1, :75].astype(np.float64)) and not r[:2].any()
    # the tail is cut at n: sample n - 1 sees only what lies inside the utterance
    two = (np.array([[1.0, 0.5]], dtype=np.float32), np.array([2], dtype=np.int32), np.array([1], dtype=np.int32))
    r = R.noise_reverb(x, lengths, rirs=two)['r'][1]
    assert r[76] == 0.5 * float(x[1, 76]) and r[0] == float(x[1, 1]) + 0.5 * float(x[1, 0])


def test_reference_measured_snr_is_the_drawn_one():
    x = waveform((6, 3000), 'int16')
    lengths = [3000, 2999, 1500, 301, 7, 1]
    ref = R.noise_reverb(x, lengths, rirs=rir_bank(), noises=noise_bank(), snr=(-5.0, 25.0), seed=4)
    for b, n in enumerate(lengths):
        row = ref['rows'][b]
        assert row[2] >= 0 and -5.0 <= row[4] < 25.0 and ref['a'][b] > 0
        added = ref['out'][b, :n] - ref['r'][b]
        measured = 10.0 * np.log10(np.sum(ref['r'][b] ** 2) / np.sum(added ** 2))
        assert abs(measured - float(row[4])) <= 1e-5, (b, measured, row[4])            # a is rounded to fp32: 20 log10(1 + 2^-24) dB
    assert all(R.snr_of(b, (7.5, 7.5), seed=b) == np.float32(7.5) for b in range(64))      # lo == hi: constant
    silent = R.noise_reverb(np.zeros((1, 100), dtype=np.float32), [100], noises=noise_bank())
    assert silent['a'][0] == 0 and not silent['out'].any()


def test_reference_draw_distribution():
    B = 4096
    rows = [R.plan_row(b, 1, 1, n_rirs=6, n_noises=4, noise_len=NOISE_LEN, rir_prob=0.3, noise_prob=0.7, snr=(5.0, 20.0), seed=11) for b in range(B)]
    for col, p in ((1, 0.3), (2, 0.7)):
        fired = sum(r[col] >= 0 for r in rows)
        assert abs(fired - B * p) <= 5 * np.sqrt(B * p * (1 - p)), (col, fired)
    assert {r[1] for r in rows} == {-1, 0, 1, 2, 3, 4, 5} and {r[2] for r in rows} == {-1, 0, 1, 2, 3}
    assert all(0 <= r[3] < NOISE_LEN[r[2]] for r in rows if r[2] >= 0) and all(r[3] == 0 for r in rows if r[2] < 0)
    s = np.array([r[4] for r in rows])
    assert s.dtype == np.float32 and np.all(s >= 5.0) and np.all(s < 20.0) and s.min() < 5.1 and s.max() > 19.9
    always = [R.plan_row(b, 1, 1, n_rirs=1, n_noises=1, noise_len=(5,), rir_prob=1.0, noise_prob=1.0) for b in range(B)]
    never = [R.plan_row(b, 1, 1, n_rirs=1, n_noises=1, noise_len=(5,), rir_prob=0.0, noise_prob=0.0) for b in range(B)]
    assert all(r[1] == 0 and r[2] == 0 for r in always) and all(r[1] == -1 and r[2] == -1 for r in never)


# ---- device (GPU) --------------------------------------------------------------------------------------------------------------
def _dev():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    return torch.device('cuda:0')


def check_values(x, lengths, out, plan, rirs, noises, **policy):
    """out / plan: the device's, as NumPy.  Integers and snr bits exact.  Values, with the device's own a from the plan:
    |out - ref| <= (Lr + 2) 2^-24 sum_j |h[j] x[.]| + 2^-23 (|r| + |a v|) per sample -- the fp32 dot-product bound plus the mix.
    Plan Es within sum(2 |r| bound + bound^2) + 2^-23 Es of the reference, plan En within 2^-23 relative, a within 2 fp32 ulp of the
    float64 formula at the plan's Es, En and snr.  Returns (reference, worst value ratio, worst energy ratio, worst a error in ulp);
    the worst ratios are printed (measured over this file's cases on an MI355X: 0.43 of the value bound, 0.11 of the energy bound,
    1.00 ulp)."""
    a_dev = plan[:, 5].copy().view(np.float32)
    ref = R.noise_reverb(x, lengths, rirs=rirs, noises=noises, gains=a_dev, **policy)
    worst_v = worst_e = worst_a = 0.0
    for b in range(x.shape[0]):
        n, ri, ni, o, snr = ref['rows'][b]
        assert plan[b, :4].tolist() == [n, ri, ni, o], (b, plan[b].tolist(), ref['rows'][b])
        assert plan[b, 4] == np.float32(snr).view(np.int32), (b, plan[b, 4:5].view(np.float32), snr)
        assert np.array_equal(out[b, n:].view(np.int32), np.zeros(out.shape[1] - n, dtype=np.int32))       # +0 exactly, not NaN
        r, S, v = ref['r'][b], ref['S'][b], ref['v'][b]
        conv = (ref['Lr'][b] + 2) * 2.0 ** -24 * S
        bound = conv + 2.0 ** -23 * (np.abs(r) + np.abs(float(a_dev[b]) * v))
        err = np.abs(out[b, :n].astype(np.float64) - ref['out'][b, :n])
        assert np.all(err <= bound), (b, ri, ni, float((err / np.maximum(bound, 1e-300)).max()))
        if n:
            worst_v = max(worst_v, float((err / np.maximum(bound, 1e-300)).max()))
        Es_dev, En_dev = (float(w) for w in plan[b, 6:8].copy().view(np.float32))
        if ni < 0:
            assert plan[b, 5:8].tolist() == [0, 0, 0]
            continue
        e_bound = float(np.sum(2 * np.abs(r) * conv + conv * conv)) + 2.0 ** -23 * ref['Es'][b]
        assert abs(Es_dev - ref['Es'][b]) <= e_bound, (b, Es_dev, ref['Es'][b], e_bound)
        assert abs(En_dev - ref['En'][b]) <= 2.0 ** -23 * ref['En'][b], (b, En_dev, ref['En'][b])
        if e_bound:
            worst_e = max(worst_e, abs(Es_dev - ref['Es'][b]) / e_bound)
        want = R.gain(Es_dev, En_dev, plan[b, 4:5].copy().view(np.float32)[0])
        ulps = abs(float(a_dev[b]) - float(want)) / float(np.spacing(want)) if want else abs(float(a_dev[b]))
        assert ulps <= 2, (b, a_dev[b], want)
        worst_a = max(worst_a, ulps)
    print('worst value error / bound: %.3f   energy: %.3f   a: %.2f ulp' % (worst_v, worst_e, worst_a))
    return ref, worst_v, worst_e, worst_a


@pytest.mark.gpu
@pytest.mark.parametrize('seed', [0, 1, 0xFFFFFFFF])
def test_plan_parity(seed):
    dev = _dev()
    B, N = 67, 1000
    lengths = ([0, 1, 2, 15, 16, 17, 999, 1000, 1200] * 8)[:B]
    x = torch.zeros(B, N, device=dev)
    rirs, noises = rir_bank(), noise_bank()
    policy = dict(rir_prob=0.5, noise_prob=0.5, snr=(-3.0, 30.0), seed=seed)
    plans = []
    for counter in (0, 7):
        cdev = torch.tensor([counter], dtype=torch.int32, device=dev)
        out, plan = F.noise_reverb(x, lengths, rirs=as_tensors(rirs, dev), noises=as_tensors(noises, dev), counter=cdev, return_plan=True, **policy)
        assert plan.dtype == torch.int32 and tuple(plan.shape) == (B, 8) and tuple(out.shape) == (B, N) and out.dtype == torch.float32
        p = plan.cpu().numpy()
        rows = [R.plan_row(b, lengths[b], N, 6, 4, NOISE_LEN, counter=counter, **policy) for b in range(B)]
        assert np.array_equal(p[:, :4], np.array([r[:4] for r in rows]))
        assert np.array_equal(p[:, 4], np.array([r[4] for r in rows], dtype=np.float32).view(np.int32))
        assert not p[p[:, 2] < 0][:, 5:].any() and not out.any()           # a silent utterance: a = 0, Es = 0
        plans.append(p)
        if counter == 0:
            p0 = F.noise_reverb(x, lengths, rirs=as_tensors(rirs, dev), noises=as_tensors(noises, dev), counter=None, return_plan=True, **policy)[1]
            assert torch.equal(p0, plan)
    assert not np.array_equal(plans[0], plans[1])
    assert {-1, 0, 1, 2, 3, 4, 5} == set(plans[0][:, 1]) | set(plans[1][:, 1]) and {-1, 0, 1, 2, 3} == set(plans[0][:, 2]) | set(plans[1][:, 2])


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', ['int16', 'float32'])
@pytest.mark.parametrize('which', list(range(len(RIR_TAPS))) + [None])
def test_value_parity(which, dtype):
    """One response against every length (which = 0 .. 5: 1, 2, 17, 300, 513 and 1025 taps with delays 0, Lr - 1, 5, 0, Lr - 1, 5), and
    the mixed banks with both coins at 0.7; every noise length in each."""
    dev = _dev()
    x = waveform((len(LENGTHS), N_MAX), dtype)
    rirs, noises = rir_bank(which), noise_bank()
    policy = dict(rir_prob=1.0 if which is not None else 0.7, noise_prob=1.0 if which is not None else 0.7, snr=(0.0, 20.0),
                  seed=1000 * (which + 1) if which is not None else 109)      # (seeds a batch apart: seed and utterance enter the key as a sum)
    out, plan = F.noise_reverb(torch.from_numpy(x.copy()).to(dev), LENGTHS, rirs=as_tensors(rirs, dev), noises=as_tensors(noises, dev),
                               return_plan=True, **policy)
    ref = check_values(x, LENGTHS, out.cpu().numpy(), plan.cpu().numpy(), rirs, noises, **policy)[0]
    if which is not None:
        assert all(r[1] == 0 and r[2] >= 0 for r in ref['rows'])


@pytest.mark.gpu
def test_every_response_meets_every_noise_and_unaligned_rows():
    """Seeds chosen on the host (the draws are the reference's) so that the mixed banks show every response and every recording at
    the long lengths; the second view starts 4 bytes off the 16-byte grid."""
    dev = _dev()
    x = waveform((9, N_MAX), 'float32')
    xd = torch.from_numpy(x.copy()).to(dev)
    rirs, noises = rir_bank(), noise_bank()
    seen_r, seen_n = set(), set()
    for seed in (11, 1011, 2011, 3011):
        policy = dict(rir_prob=0.8, noise_prob=0.8, snr=(5.0, 15.0), seed=seed)
        view = xd.reshape(-1)[1:1 + 8 * N_MAX].reshape(8, N_MAX)
        out, plan = F.noise_reverb(view, LENGTHS, rirs=as_tensors(rirs, dev), noises=as_tensors(noises, dev), return_plan=True, **policy)
        ref = check_values(view.cpu().numpy(), LENGTHS, out.cpu().numpy(), plan.cpu().numpy(), rirs, noises, **policy)[0]
        seen_r |= {r[1] for r in ref['rows'][3:]}
        seen_n |= {r[2] for r in ref['rows'][3:]}
    assert seen_r == {-1, 1, 2, 3, 4, 5} and seen_n == {-1, 0, 1, 2, 3}    # (the 1-tap response meets every length in test_value_parity)


@pytest.mark.gpu
def test_long_response_and_clamped_lengths():
    """A 4000-tap response (16 tap chunks, the skipped ones among them) and one of the full 8192, on rows of several tiles; lengths
    outside [0, max_samples] are clamped."""
    dev = _dev()
    x = waveform((5, 10000), 'int16')
    lengths = [50000, -3, 10000, 4500, 2 ** 31 - 1]
    rng = np.random.RandomState(3)
    hs = [rng.randn(4000) * np.exp(-np.arange(4000) / 600.0), rng.randn(8192) * np.exp(-np.arange(8192) / 1500.0)]
    hs[0][37] = 9.0
    hs[1][3] = 9.0
    bank = F.prepare_rirs(hs)
    assert bank[1].tolist() == [4000, 8192] and bank[2].tolist() == [37, 3]
    rirs = tuple(t.numpy() for t in bank)
    policy = dict(rir_prob=1.0, noise_prob=1.0, snr=(10.0, 10.0), seed=5)
    out, plan = F.noise_reverb(torch.from_numpy(x.copy()).to(dev), lengths, rirs=tuple(t.to(dev) for t in bank), noises=as_tensors(noise_bank(), dev),
                               return_plan=True, **policy)
    ref = check_values(x, lengths, out.cpu().numpy(), plan.cpu().numpy(), rirs, noise_bank(), **policy)[0]
    assert [r[0] for r in ref['rows']] == [10000, 0, 10000, 4500, 10000] and {r[1] for r in ref['rows']} == {0, 1}
    assert all(r[4] == np.float32(10.0) for r in ref['rows'])


@pytest.mark.gpu
def test_exact_cases():
    dev = _dev()
    noises = as_tensors(noise_bank(), dev)
    unit = tuple(torch.tensor(v, dtype=t, device=dev) for v, t in (([[1.0, 7.0, 7.0]], torch.float32), ([1], torch.int32), ([0], torch.int32)))
    for dtype in ('int16', 'float32'):
        x = waveform((len(LENGTHS), N_MAX), dtype)
        xd = torch.from_numpy(x.copy()).to(dev)
        # probabilities 0: a bit copy of float(x), zeros behind n -- with banks and without
        for kw in (dict(rirs=as_tensors(rir_bank(), dev), noises=noises, rir_prob=0.0, noise_prob=0.0), dict()):
            out, plan = F.noise_reverb(xd, LENGTHS, return_plan=True, seed=3, **kw)
            for b, n in enumerate(LENGTHS):
                assert torch.equal(out[b, :n].view(torch.int32), xd[b, :n].float().view(torch.int32)) and not out[b, n:].any()
            assert plan[:, 0].tolist() == LENGTHS and plan[:, 1].tolist() == [-1] * 8 and plan[:, 2].tolist() == [-1] * 8
            assert not plan[:, 3].any() and not plan[:, 5:].any()
        # the unit impulse equals no reverberation, bit for bit -- alone and under the same noise
        a = F.noise_reverb(xd, LENGTHS, rirs=unit, seed=3)
        assert torch.equal(a.view(torch.int32), out.view(torch.int32))
        a, pa = F.noise_reverb(xd, LENGTHS, rirs=unit, noises=noises, seed=3, return_plan=True)
        c, pc = F.noise_reverb(xd, LENGTHS, noises=noises, seed=3, return_plan=True)
        assert torch.equal(a.view(torch.int32), c.view(torch.int32)) and torch.equal(pa[:, 2:], pc[:, 2:]) and pa[:, 1].tolist() == [0] * 8
        assert not torch.equal(a, out)
        # an all-zero noise: a == 0 and the output is r; a zero utterance under noise: a == 0 and the output is zero
        zero = (torch.zeros(2, 50, device=dev), torch.tensor([50, 3], dtype=torch.int32, device=dev))
        z, pz = F.noise_reverb(xd, LENGTHS, noises=zero, seed=3, return_plan=True)
        assert torch.equal(z.view(torch.int32), out.view(torch.int32)) and not pz[:, 5].any() and not pz[:, 7].any() and pz[1:, 6].all()
        s, ps = F.noise_reverb(torch.zeros_like(xd), LENGTHS, rirs=as_tensors(rir_bank(), dev), noises=noises, seed=3, return_plan=True)
        assert not s.view(torch.int32).any() and not ps[:, 5].any() and not ps[:, 6].any() and ps[1:, 7].all()


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', ['int16', 'float32'])
def test_padding_never_leaks(dtype):
    """Samples >= n hold NaN (float32) or 32767 (int16), the bank rows hold NaN behind rir_len / noise_len: the output is finite,
    equals the clean run bit for bit, and matches the reference, which never touches any of them."""
    dev = _dev()
    x = waveform((len(LENGTHS), N_MAX), dtype)
    dirty = x.copy()
    for b, n in enumerate(LENGTHS):
        dirty[b, n:] = 32767 if dtype == 'int16' else np.nan
    policy = dict(rir_prob=0.7, noise_prob=0.7, snr=(0.0, 20.0), seed=21)
    clean = F.noise_reverb(torch.from_numpy(x.copy()).to(dev), LENGTHS, rirs=as_tensors(rir_bank(), dev), noises=as_tensors(noise_bank(), dev),
                           return_plan=True, **policy)
    rirs, noises = rir_bank(pad=float('nan')), noise_bank(pad=float('nan'))
    assert np.isnan(rirs[0]).any() and np.isnan(noises[0]).any()
    out, plan = F.noise_reverb(torch.from_numpy(dirty).to(dev), LENGTHS, rirs=as_tensors(rirs, dev), noises=as_tensors(noises, dev),
                               return_plan=True, **policy)
    assert torch.isfinite(out).all()
    assert torch.equal(out.view(torch.int32), clean[0].view(torch.int32)) and torch.equal(plan, clean[1])
    ref = check_values(dirty, LENGTHS, out.cpu().numpy(), plan.cpu().numpy(), rirs, noises, **policy)[0]
    assert {r[1] >= 0 for r in ref['rows']} == {True, False} and {r[2] >= 0 for r in ref['rows']} == {True, False}


@pytest.mark.gpu
def test_determinism():
    dev = _dev()
    x = torch.from_numpy(waveform((len(LENGTHS), N_MAX), 'int16').copy()).to(dev)
    banks = dict(rirs=as_tensors(rir_bank(), dev), noises=as_tensors(noise_bank(), dev))
    policy = dict(rir_prob=0.7, noise_prob=0.7, seed=6)
    c3 = torch.full((1,), 3, dtype=torch.int32, device=dev)
    a = F.noise_reverb(x, LENGTHS, counter=c3, return_plan=True, **banks, **policy)
    b = F.noise_reverb(x, LENGTHS, counter=c3.clone(), return_plan=True, **banks, **policy)
    assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1], b[1])
    c = F.noise_reverb(x, LENGTHS, counter=c3 + 1, return_plan=True, **banks, **policy)
    assert not torch.equal(a[1], c[1])
    d = F.noise_reverb(x, LENGTHS, counter=c3.view(torch.uint32), return_plan=True, **banks, **policy)
    assert torch.equal(d[1], a[1])
    e = F.noise_reverb(x, LENGTHS, counter=c3, return_plan=True, **banks, **dict(policy, seed=7))
    assert not torch.equal(a[1], e[1])


@pytest.mark.gpu
def test_graph_capture_draws_anew_on_every_replay():
    dev = _dev()
    x = torch.from_numpy(waveform((len(LENGTHS), N_MAX), 'int16').copy()).to(dev)
    lengths = torch.tensor(LENGTHS, dtype=torch.int32, device=dev)
    policy = dict(rirs=as_tensors(rir_bank(), dev), noises=as_tensors(noise_bank(), dev), rir_prob=0.5, noise_prob=0.5, seed=7)
    nr = features.NoiseReverb(**policy)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        nr(x, lengths)                                                     # warm-up: the counter now lives on the device
    torch.cuda.current_stream().wait_stream(side)
    assert nr.state_dict()['counter'] == 1
    c = 5
    nr.load_state_dict({'seed': 7, 'counter': c})
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                          # one stream, no parallel branches
        out, olen = nr(x, lengths)
        plan = nr.last_plan
    assert olen is lengths
    seen = []
    for k in range(3):
        graph.replay()
        seen.append((out.clone(), plan.clone()))
    torch.cuda.synchronize()
    for k, (o, p) in enumerate(seen):
        ck = torch.tensor([c + k], dtype=torch.int32, device=dev)
        eo, ep = F.noise_reverb(x, lengths, counter=ck, return_plan=True, **policy)
        assert torch.equal(o.view(torch.int32), eo.view(torch.int32)) and torch.equal(p, ep), k
    check_values(x.cpu().numpy(), LENGTHS, seen[2][0].cpu().numpy(), seen[2][1].cpu().numpy(), rir_bank(), noise_bank(), rir_prob=0.5,
                 noise_prob=0.5, seed=7, counter=c + 2)
    assert not torch.equal(seen[0][1], seen[1][1]) and not torch.equal(seen[1][1], seen[2][1]) and not torch.equal(seen[0][1], seen[2][1])
    assert nr.state_dict() == {'seed': 7, 'counter': c + 3}


@pytest.mark.gpu
def test_quaternion_fbank_wave_augment_tuple():
    from test_fbank import signals
    dev = _dev()
    n = [16000, 9000, 4001, 401]
    wave = torch.from_numpy(signals(n, seed=6)).to(dev)
    banks = dict(rirs=F.prepare_rirs(features.synthetic_rirs(4, seed=1), device=dev), noises=F.prepare_noises(features.synthetic_noises(3, 5000, seed=2), device=dev))
    sp_policy, nr_policy = dict(gain=(0.5, 2.0), seed=8), dict(rir_prob=0.7, noise_prob=0.7, snr=(5.0, 15.0), seed=9)
    for norm, dt in ((None, torch.float32), ('utterance', torch.bfloat16)):
        sp, nr = features.SpeedPerturb(**sp_policy), features.NoiseReverb(**banks, **nr_policy)
        got, gfl = features.quaternion_fbank(wave, n, normalize=norm, dtype=dt, wave_augment=(sp, nr))
        pw, pl = F.speed_perturb(wave, n, **sp_policy)
        cw, plan = F.noise_reverb(pw, pl, return_plan=True, **banks, **nr_policy)
        want, wfl = features.quaternion_fbank(cw, pl, normalize=norm, dtype=dt)
        bits = torch.int32 if dt == torch.float32 else torch.int16
        assert got.dtype == dt and torch.equal(gfl, wfl) and torch.equal(got.view(bits), want.view(bits))
        assert torch.equal(nr.last_plan, plan) and nr.state_dict()['counter'] == 1 and sp.state_dict()['counter'] == 1
        assert (plan[:, 1] >= 0).any() and (plan[:, 2] >= 0).any() and plan[:, 0].tolist() == pl.tolist()
        assert not torch.equal(got, features.quaternion_fbank(pw, pl, normalize=norm, dtype=dt)[0])
        # a lone NoiseReverb keeps the shape of the plain front end; a list is a tuple
        alone = features.quaternion_fbank(wave, n, normalize=norm, dtype=dt, wave_augment=features.NoiseReverb(**banks, **nr_policy))
        plain = features.quaternion_fbank(wave, n, normalize=norm, dtype=dt)
        assert alone[0].shape == plain[0].shape and torch.equal(alone[1], plain[1]) and not torch.equal(alone[0], plain[0])
        lst = features.quaternion_fbank(wave, n, normalize=norm, dtype=dt, wave_augment=[features.SpeedPerturb(**sp_policy), features.NoiseReverb(**banks, **nr_policy)])
        assert torch.equal(lst[0].view(bits), got.view(bits))


@pytest.mark.gpu
def test_train_timit_example_with_noise_reverb(tmp_path):
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
    noise_dir = tmp_path / 'noise'
    noise_dir.mkdir()
    (noise_dir / 'hum.wav').write_bytes(sphere_bytes((3000 * np.sin(np.arange(7000) * 0.05)).astype(np.int16)))
    cmd = [sys.executable, os.path.join(ROOT, 'examples', 'train_timit.py'), '--timit', str(tmp_path), '--speed-perturb', '--noise-reverb',
           '--noise-dir', str(noise_dir), '--rir-prob', '1', '--noise-prob', '1', '--snr', '0,10', '--steps', '2', '--eval-every', '2',
           '--layers', '4', '--batch', '2']
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, env=dict(os.environ), timeout=600, universal_newlines=True)
    assert r.returncode == 0, r.stdout[-4000:]
    losses = re.findall(r'step\s+\d+\s+loss (\S+)', r.stdout)
    assert len(losses) == 2, r.stdout[-4000:]
    assert all(np.isfinite(float(v)) for v in losses)
    assert len(re.findall(r'held-out ctc cost (\S+)', r.stdout)) == 1
