"""On-device SpecAugment (qcnn_amd.functional.spec_augment, qcnn_amd.features.SpecAugment, csrc/qk_specaug.hip) against the NumPy
restatement of include/qk.h's "SpecAugment" section in tests/specaug_ref.py.
"""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import specaug_ref as R
from qcnn_amd import _lib as L
from qcnn_amd import data, features
from qcnn_amd import functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = dict(time_warp=3, freq_masks=2, freq_width=5, time_masks=2, time_width=12, time_ratio=0.5)
POLICIES = {
    'warp': dict(time_warp=3),
    'freq': dict(freq_masks=2, freq_width=5),
    'time': dict(time_masks=2, time_width=12),
    'all': ALL,
    'masks8+8': dict(time_warp=2, freq_masks=8, freq_width=3, time_masks=8, time_width=4),
    'freq_width>=rows': dict(freq_masks=1, freq_width=64),
    'time_ratio0': dict(time_warp=1, time_masks=2, time_width=10, time_ratio=0.0),
    'fill-1.5': dict(ALL, fill=-1.5),
}
SHAPES = [(5, 4, 41, 53), (3, 4, 7, 1), (2, 1, 3, 130), (4, 4, 41, 199), (2, 4, 41, 64)]


def lengths_for(B, T):
    return [T, max(T - 7, 0), T // 2, min(9, T), 0][:B]


def histogram_ok(widths):
    """Each of the 9 widths 0 .. 8 within 5 binomial standard deviations of 4096 / 9."""
    counts = np.bincount(np.asarray(widths), minlength=9)
    assert counts.sum() == 4096 and len(counts) == 9
    p = 1.0 / 9
    sd = np.sqrt(4096 * p * (1 - p))
    assert np.all(np.abs(counts - 4096 * p) <= 5 * sd), counts
    return True


# ---- CPU: the library's surface ------------------------------------------------------------------------------------------------
def test_library_exports_spec_augment():
    assert 'qk_spec_augment' in L.SYMBOLS
    assert hasattr(ctypes.CDLL(L.LIB_PATH), 'qk_spec_augment')
    assert (L.QK_SPECAUG_MAX_MASKS, L.QK_SPECAUG_PLAN_WORDS) == (8, 36)
    assert ctypes.sizeof(L.SpecAugPolicy) == 32
    assert L.lib().qk_version() == 103


def test_refuses_bad_arguments_and_cpu_tensors_without_a_gpu():
    x = torch.zeros(2, 4, 41, 20)
    n = [20, 10]
    for kw in (dict(freq_masks=9), dict(freq_masks=-1), dict(time_masks=9), dict(time_masks=-1), dict(freq_width=-1), dict(time_width=-1),
               dict(time_warp=-1), dict(time_ratio=1.5), dict(time_ratio=-0.1), dict(time_ratio=float('nan')), dict(fill=float('inf')),
               dict(fill=float('nan')), dict(seed=-1), dict(seed=2 ** 32)):
        with pytest.raises(ValueError):
            F.spec_augment(x, n, **kw)
        with pytest.raises(ValueError):
            features.SpecAugment(**kw)
    with pytest.raises(TypeError):
        F.spec_augment(x, n, time_warp=1.5)
    with pytest.raises(TypeError):
        F.spec_augment(x, n, dtype=torch.float64)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        F.spec_augment(x, n, time_warp=2)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        features.SpecAugment()(x, n)
    with pytest.raises(TypeError):
        features.quaternion_fbank(torch.zeros(2, 1000), augment='specaug')


def test_policy_state_dict_round_trip_and_checks():
    a = features.SpecAugment(seed=5)
    assert a.state_dict() == {'seed': 5, 'counter': 0}
    a.load_state_dict({'seed': 9, 'counter': 0xFFFFFFFF})
    assert a.state_dict() == {'seed': 9, 'counter': 0xFFFFFFFF} and a.seed == 9
    for bad in ({'seed': -1, 'counter': 0}, {'seed': 0, 'counter': 2 ** 32}, {'seed': 0.5, 'counter': 0}, {'seed': 0, 'counter': True}):
        with pytest.raises(ValueError):
            a.load_state_dict(bad)
    assert a.state_dict() == {'seed': 9, 'counter': 0xFFFFFFFF}           # a refused dict changes nothing
    with pytest.raises(KeyError):
        a.load_state_dict({'seed': 1})


# ---- CPU: hand facts of the reference ------------------------------------------------------------------------------------------
def test_reference_hash_is_uint32_and_keyed():
    assert R.fmix(0) == 0 and R.fmix(1) == 0x514E28B7                     # murmur3's finaliser
    us = {R.u(s, c, b, k) for s in (0, 2) for c in (0, 1) for b in (0, 1) for k in (0, 1)}
    assert len(us) == 16 and all(0 <= v <= 0xFFFFFFFF for v in us)
    assert R.u(0, 0, 1, 5) == R.u(1, 0, 0, 5)                             # seed and utterance index enter as a sum
    assert R.u(0, 1, 0, 3) == R.u(0x9E3779B1, 0, 0, 3)                    # key = seed + 0x9E3779B1 * counter
    assert R.u(5, 0xFFFFFFFF, 2, 3) == R.u((5 - 0x9E3779B1) & 0xFFFFFFFF, 0, 2, 3)      # mod 2^32


def test_reference_identity_policy_changes_nothing():
    x = np.random.RandomState(0).randn(3, 4, 7, 20).astype(np.float32)
    ref = R.spec_augment(x, [20, 5, 0])
    assert np.array_equal(ref['y'], x.astype(np.float64)) and not ref['masked'].any() and ref['exact'].all()
    assert np.array_equal(ref['plan'][:, 0], [20, 5, 0]) and not ref['plan'][:, 1:].any()


def test_reference_warp_pins_three_frames_and_is_monotone():
    for n in (9, 10, 53, 199):
        for b in range(40):
            W = 3
            row = R.plan_row(b, n, 41, 256, time_warp=W, seed=b)
            assert row[0] == n
            c, w = row[1], row[2]
            cp = c + w
            assert W + 1 <= c <= n - W - 2 and -W <= w <= W and 1 <= cp <= n - 2
            i0, r, den = R.warp_index(n, c, w)
            assert (i0[0], r[0]) == (0, 0) and (i0[cp], r[cp]) == (c, 0) and (i0[n - 1], r[n - 1]) == (n - 1, 0)
            pos = i0 + r / den
            assert np.all(np.diff(pos) >= 0) and np.all(r < den) and np.all(i0 <= n - 1)
    assert R.plan_row(0, 8, 41, 53, time_warp=3)[1:3] == [0, 0]           # n = 2 W + 2: inactive
    assert R.plan_row(0, 9, 41, 53, time_warp=3)[1] == 4                  # n = 2 W + 3: the one admissible centre
    assert R.plan_row(0, 60, 41, 53, time_warp=3)[0] == 53                # the clamp


def test_reference_intervals_lie_inside_and_time_ratio_caps():
    rows, T = 41, 199
    for b in range(200):
        n = [0, 1, 2, 17, 100, 199, 250][b % 7]
        row = R.plan_row(b, n, rows, T, freq_masks=8, freq_width=50, time_masks=8, time_width=30, time_ratio=0.2, seed=3, counter=b)
        nn = min(n, T)
        for i in range(8):
            f0, fw = row[4 + 2 * i], row[5 + 2 * i]
            t0, tw = row[20 + 2 * i], row[21 + 2 * i]
            assert 0 <= f0 and 0 <= fw <= rows and f0 + fw <= rows
            assert 0 <= t0 and 0 <= tw and t0 + tw <= nn
            assert tw <= min(30, int(np.floor(np.float32(nn) * np.float32(0.2))))
    row = R.plan_row(0, 100, rows, T, time_masks=8, time_width=30, time_ratio=0.0)
    assert not any(row[21 + 2 * i] for i in range(8))
    row = R.plan_row(0, 100, rows, T, freq_masks=2, freq_width=8)
    assert not any(row[8:20]) and not any(row[20:])                       # unused masks are 0, 0


def test_reference_randint_is_uniform():
    pol = dict(freq_masks=1, freq_width=8, seed=11)
    assert histogram_ok([R.plan_row(b, 1, 41, 1, **pol)[5] for b in range(4096)])


# ---- device (GPU) --------------------------------------------------------------------------------------------------------------
def _dev():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    return torch.device('cuda:0')


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def check_values(got, plan, x, lengths, policy):
    """got / plan: the device's fp32 output and plan as NumPy; x fp32 NumPy.  The three classes of cells of the issue."""
    ref = R.spec_augment(x, lengths, **policy)
    assert np.array_equal(plan, ref['plan'])
    fill = np.float32(policy.get('fill', 0.0))
    m, e = ref['masked'], ref['exact']
    assert np.array_equal(_bits(got)[m], _bits(np.full(int(m.sum()), fill)))
    assert np.array_equal(_bits(got)[e], _bits(ref['y'][e]))
    i = ~(m | e)
    err = np.abs(got.astype(np.float64) - ref['y'])[i]
    assert np.all(err <= 1e-6 * ref['bound'][i]), float((err / np.maximum(ref['bound'][i], 1e-300)).max())
    return ref


PLAN_POLICY = dict(time_warp=3, freq_masks=2, freq_width=8, time_masks=2, time_width=10, time_ratio=0.5)
PLAN_LENGTHS = ([0, 1, 2, 8, 9, 10, 52, 53, 60] * 8)[:67]


@pytest.mark.gpu
@pytest.mark.parametrize('seed', [0, 1, 0xFFFFFFFF])
def test_plan_parity_exact_integers(seed):
    dev = _dev()
    B, T = 67, 53
    x = torch.zeros(B, 1, 41, T, device=dev)
    lengths = torch.tensor(PLAN_LENGTHS, dtype=torch.int32, device=dev)
    for counter in (0, 1, 0xFFFFFFFF):
        want = R.plan(PLAN_LENGTHS, 41, T, seed=seed, counter=counter, **PLAN_POLICY)
        cdev = torch.tensor([counter - (1 << 32) if counter >= 1 << 31 else counter], dtype=torch.int32, device=dev)
        _, plan = F.spec_augment(x, lengths, seed=seed, counter=cdev, return_plan=True, **PLAN_POLICY)
        assert plan.dtype == torch.int32 and tuple(plan.shape) == (B, 36)
        assert np.array_equal(plan.cpu().numpy(), want), (seed, counter)
        if counter == 0:
            _, plan0 = F.spec_augment(x, lengths, seed=seed, counter=None, return_plan=True, **PLAN_POLICY)
            assert torch.equal(plan0, plan)
    active = want[:, 1] > 0
    assert np.array_equal(active, np.minimum(PLAN_LENGTHS, T) >= 9)       # active iff n >= 2 W + 3


@pytest.mark.gpu
def test_device_randint_is_uniform():
    dev = _dev()
    x = torch.zeros(4096, 1, 41, 1, device=dev)
    _, plan = F.spec_augment(x, torch.ones(4096, dtype=torch.int32, device=dev), freq_masks=1, freq_width=8, seed=11, return_plan=True)
    assert histogram_ok(plan[:, 5].cpu().numpy())


@pytest.mark.gpu
@pytest.mark.parametrize('shape', SHAPES, ids=['x'.join(map(str, s)) for s in SHAPES])
@pytest.mark.parametrize('name', list(POLICIES))
def test_value_parity_fp32(shape, name):
    dev = _dev()
    policy = dict(POLICIES[name], seed=SHAPES.index(shape) * 16 + list(POLICIES).index(name))
    B, _, _, T = shape
    lengths = lengths_for(B, T)
    x = np.random.RandomState(0).randn(*shape).astype(np.float32)
    got, plan = F.spec_augment(torch.from_numpy(x).to(dev), lengths, return_plan=True, **policy)
    assert got.dtype == torch.float32 and tuple(got.shape) == shape
    check_values(got.cpu().numpy(), plan.cpu().numpy(), x, lengths, policy)


@pytest.mark.gpu
@pytest.mark.parametrize('shape,lengths', [((1, 2, 2, 12301), [12301]), ((2, 1, 1, 33001), [33001, 32768])], ids=['row>lds', 'n>32767'])
def test_value_parity_long_rows(shape, lengths):
    """Rows beyond the staging budget take their taps from memory; n > 32767 takes the 64-bit index arithmetic."""
    dev = _dev()
    policy = dict(time_warp=40, freq_masks=1, freq_width=1, time_masks=2, time_width=300, seed=3)
    x = np.random.RandomState(1).randn(*shape).astype(np.float32)
    got, plan = F.spec_augment(torch.from_numpy(x).to(dev), lengths, return_plan=True, **policy)
    ref = check_values(got.cpu().numpy(), plan.cpu().numpy(), x, lengths, policy)
    assert ref['plan'][0, 1] > 0


@pytest.mark.gpu
def test_padding_is_copied_and_never_leaks():
    dev = _dev()
    shape = SHAPES[0]
    lengths = [53, 46, 26, 9, 0]
    x = np.random.RandomState(2).randn(*shape).astype(np.float32)
    for b, n in enumerate(lengths):
        x[b, :, :, n:] = 1e30
    policy = dict(ALL, seed=4)
    got, plan = F.spec_augment(torch.from_numpy(x).to(dev), lengths, return_plan=True, **policy)
    g = got.cpu().numpy()
    for b, n in enumerate(lengths):
        assert np.all(g[b, :, :, n:] == np.float32(1e30)) and np.all(np.abs(g[b, :, :, :n]) < 1e3)
    check_values(g, plan.cpu().numpy(), x, lengths, policy)


@pytest.mark.gpu
def test_16bit_outputs_and_inputs():
    dev = _dev()
    shape = SHAPES[0]                                                      # 53 frames: rows misaligned for 16-byte accesses
    lengths = lengths_for(shape[0], shape[3])
    x = torch.from_numpy(np.random.RandomState(3).randn(*shape).astype(np.float32)).to(dev)
    policy = dict(ALL, seed=5, fill=-1.5)
    ref = F.spec_augment(x, lengths, **policy)
    for dt in (torch.bfloat16, torch.float16):
        got = F.spec_augment(x, lengths, dtype=dt, **policy)
        assert got.dtype == dt and torch.equal(got, ref.to(dt))
        x16 = x.to(dt)
        up = F.spec_augment(x16.float(), lengths, **policy)
        assert torch.equal(F.spec_augment(x16, lengths, dtype=torch.float32, **policy), up)
        got16 = F.spec_augment(x16, lengths, **policy)
        assert got16.dtype == dt and torch.equal(got16, up.to(dt))
        other = torch.float16 if dt == torch.bfloat16 else torch.bfloat16
        assert torch.equal(F.spec_augment(x16, lengths, dtype=other, **policy), up.to(other))
        unwarped = dict(policy, time_warp=0)                               # (the unstaged kernel's vector loads)
        assert torch.equal(F.spec_augment(x16, lengths, **unwarped), F.spec_augment(x16.float(), lengths, **unwarped).to(dt))


@pytest.mark.gpu
def test_identity_and_determinism():
    dev = _dev()
    shape = SHAPES[0]
    lengths = lengths_for(shape[0], shape[3])
    x = torch.from_numpy(np.random.RandomState(4).randn(*shape).astype(np.float32)).to(dev)
    x[0, 0, 0, :4] = torch.tensor([-0.0, float('inf'), float('nan'), 1e-45], device=dev)
    for dt in (torch.float32, torch.bfloat16, torch.float16):
        xd = x.to(dt)
        for view in (xd, xd.reshape(-1)[1:1 + 4 * 4 * 41 * 53].reshape(4, 4, 41, 53)):          # the second is not 16-byte aligned
            n = lengths[:view.shape[0]]
            got = F.spec_augment(view, n)
            assert got.data_ptr() != view.data_ptr()
            bits = torch.int32 if dt == torch.float32 else torch.int16
            assert torch.equal(got.view(bits), view.contiguous().view(bits))
    policy = dict(ALL, seed=6)
    a, pa = F.spec_augment(x, lengths, return_plan=True, **policy)
    b, pb = F.spec_augment(x, lengths, return_plan=True, **policy)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and torch.equal(pa, pb)
    c1 = torch.ones(1, dtype=torch.int32, device=dev)
    _, pc = F.spec_augment(x, lengths, counter=c1, return_plan=True, **policy)
    assert not torch.equal(pa, pc)
    _, pu = F.spec_augment(x, lengths, counter=c1.view(torch.uint32), return_plan=True, **policy)
    assert torch.equal(pu, pc)


@pytest.mark.gpu
def test_graph_capture_draws_new_masks_on_every_replay():
    dev = _dev()
    shape = SHAPES[0]
    lengths = torch.tensor(lengths_for(shape[0], shape[3]), dtype=torch.int32, device=dev)
    x = torch.from_numpy(np.random.RandomState(5).randn(*shape).astype(np.float32)).to(dev)
    policy = dict(ALL, seed=7)
    aug = features.SpecAugment(**policy)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        aug(x, lengths)                                                    # warm-up: the counter now lives on the device
    torch.cuda.current_stream().wait_stream(side)
    assert aug.state_dict()['counter'] == 1
    aug.load_state_dict({'seed': 7, 'counter': 0})
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = aug(x, lengths, dtype=torch.bfloat16)
        plan = aug.last_plan
    seen = []
    for k in range(3):
        graph.replay()
        seen.append((out.clone(), plan.clone()))
    torch.cuda.synchronize()
    for k, (o, p) in enumerate(seen):
        ck = torch.tensor([k], dtype=torch.int32, device=dev)
        eo, ep = F.spec_augment(x, lengths, counter=ck, dtype=torch.bfloat16, return_plan=True, **policy)
        assert torch.equal(o, eo) and torch.equal(p, ep), k
    assert not torch.equal(seen[0][1], seen[1][1]) and not torch.equal(seen[1][1], seen[2][1]) and not torch.equal(seen[0][1], seen[2][1])
    assert aug.state_dict() == {'seed': 7, 'counter': 3}


@pytest.mark.gpu
def test_quaternion_fbank_augment():
    from test_fbank import signals
    dev = _dev()
    n = [16000, 9000, 4001, 401]
    wave = torch.from_numpy(signals(n, seed=6)).to(dev)
    policy = dict(time_warp=5, freq_masks=2, freq_width=8, time_masks=2, time_width=25, time_ratio=0.2, seed=8)
    for norm in (None, 'utterance'):
        plain32, fl = features.quaternion_fbank(wave, n, normalize=norm, dtype=torch.float32)
        for dt in (torch.float32, torch.bfloat16):
            aug = features.SpecAugment(**policy)
            got, gfl = features.quaternion_fbank(wave, n, normalize=norm, dtype=dt, augment=aug)
            want, plan = F.spec_augment(plain32, fl, dtype=dt, return_plan=True, **policy)
            assert got.dtype == dt and torch.equal(gfl, fl)
            assert torch.equal(got, want) and torch.equal(aug.last_plan, plan)
            assert aug.state_dict()['counter'] == 1
            none = features.quaternion_fbank(wave, n, normalize=norm, dtype=dt, augment=None)[0]
            assert torch.equal(none, features.quaternion_fbank(wave, n, normalize=norm, dtype=dt)[0])
            assert torch.equal(none, plain32.to(dt)) and not torch.equal(none, got)


@pytest.mark.gpu
def test_raw_ctypes_argument_checks():
    dev = _dev()
    B, P, Rr, T = 2, 4, 7, 20
    x = torch.randn(B, P, Rr, T, device=dev)
    out = torch.empty_like(x)
    lengths = torch.tensor([20, 11], dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream().cuda_stream

    def call(pol, xo=x, oo=out, shape=(B, P, Rr, T), plan=None):
        return L.lib().qk_spec_augment(L.QK_F32, L.QK_F32, shape[0], shape[1], shape[2], shape[3], xo.data_ptr(), lengths.data_ptr(),
                                       ctypes.byref(pol), None, oo.data_ptr(), plan, stream)
    good = L.SpecAugPolicy(2, 2, 3, 2, 5, 1.0, 0.0, 1)
    assert call(good) == 0                                                 # plan = NULL is accepted
    plan = torch.empty(B, 36, dtype=torch.int32, device=dev)
    assert call(good, plan=plan.data_ptr()) == 0
    assert np.array_equal(plan.cpu().numpy(), R.plan([20, 11], Rr, T, time_warp=2, freq_masks=2, freq_width=3, time_masks=2, time_width=5,
                                                     seed=1))
    assert call(good, oo=x) == L.QK_ERR_INVALID_ARG                        # out overlaps x
    assert call(good, oo=x.reshape(-1)[8:]) == L.QK_ERR_INVALID_ARG        # ... partly
    assert b'overlap' in L.lib().qk_last_error()
    assert call(L.SpecAugPolicy(0, 9, 3, 0, 0, 1.0, 0.0, 0)) == L.QK_ERR_INVALID_ARG
    assert call(L.SpecAugPolicy(0, 0, 0, 9, 3, 1.0, 0.0, 0)) == L.QK_ERR_INVALID_ARG
    assert call(L.SpecAugPolicy(0, 0, 0, 1, 3, 1.5, 0.0, 0)) == L.QK_ERR_INVALID_ARG
    assert call(L.SpecAugPolicy(0, 0, 0, 1, 3, float('nan'), 0.0, 0)) == L.QK_ERR_INVALID_ARG
    assert call(L.SpecAugPolicy(0, 0, 0, 0, 0, 1.0, float('inf'), 0)) == L.QK_ERR_INVALID_ARG
    assert call(L.SpecAugPolicy(-1, 0, 0, 0, 0, 1.0, 0.0, 0)) == L.QK_ERR_INVALID_ARG
    assert call(L.SpecAugPolicy(0, 1, -1, 0, 0, 1.0, 0.0, 0)) == L.QK_ERR_INVALID_ARG
    assert call(L.SpecAugPolicy(0, 0, 0, 1, -1, 1.0, 0.0, 0)) == L.QK_ERR_INVALID_ARG
    for shape in ((0, P, Rr, T), (B, 0, Rr, T), (B, P, 0, T), (B, P, Rr, 0)):
        assert call(good, shape=shape) == L.QK_ERR_INVALID_ARG
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_train_timit_example_with_specaug(tmp_path):
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
    cmd = [sys.executable, os.path.join(ROOT, 'examples', 'train_timit.py'), '--timit', str(tmp_path), '--specaug', '--steps', '2',
           '--eval-every', '2', '--layers', '4', '--batch', '2']
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, env=dict(os.environ), timeout=600, universal_newlines=True)
    assert r.returncode == 0, r.stdout[-4000:]
    losses = re.findall(r'step\s+\d+\s+loss (\S+)', r.stdout)
    assert len(losses) == 2, r.stdout[-4000:]
    assert all(np.isfinite(float(v)) for v in losses)
    assert len(re.findall(r'held-out ctc cost (\S+)', r.stdout)) == 1
