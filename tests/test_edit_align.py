"""Scoring alignment (functional.edit_alignment, csrc/qk_edit_align.hip; include/qk.h, "Scoring alignment") against the plain
restatement in tests/edit_align_ref.py, which is itself pinned to an enumeration of every monotone alignment; the callers around it
(layers.error_breakdown, layers.top_confusions, data.TIMIT_PHONES_39, TimitQCNN.error_breakdown) and examples/train_timit.py
--confusions.  Every comparison is integer-exact.
"""
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import edit_align_ref as R
from qcnn_amd import _lib, data, functional as Fq, layers
from qcnn_amd.models.interspeech_model import TimitQCNN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- CPU: the reference against the definition -------------------------------------------------------------------------------------
def test_reference_equals_the_enumerated_optimum_under_the_tie_rule():
    """Of all minimum-cost alignments, read from the end, the smallest under diagonal < deletion < insertion."""
    pairs = R.tiny_pairs()
    assert len(pairs) == 961
    several = differ = 0
    for h, r in pairs:
        every = R.enumerate_alignments(h, r)
        best = min(cost for cost, _, _ in every)
        optimal = [a for a in every if a[0] == best]
        want = min(optimal, key=lambda a: a[1][::-1])
        got = R.align(h, r)
        assert got['distance'] == best and tuple(got['ops']) == want[1] and got['counts'][1:] == want[2], (h, r)
        c, s, d, i = got['counts']
        assert c + s + d == len(r) and c + s + i == len(h) and s + d + i == best, (h, r)
        several += len(optimal) > 1
        differ += len({a[2] for a in optimal}) > 1
    print('pairs with several optimal alignments: %d, with optimal alignments of different (S, D, I): %d' % (several, differ))
    assert several >= 400 and differ >= 100, (several, differ)


def test_reference_class_map_drops_and_passes_through():
    cm = [1, -1, 0]
    assert R.apply_map([0, 1, 2, 3, -5, 1], cm) == [1, 0, 3, -5]
    res = R.align([1, 1], [1], cm)                          # everything drops
    assert res['counts'] == (0, 0, 0, 0) and res['pairs'] == []
    res = R.align([0, 7], [2, 7, 1, 0], cm)                 # h = 1 7, r = 0 7 1
    assert (res['H'], res['R']) == (2, 3) and res['counts'] == (1, 1, 1, 0)
    assert res['pairs'] == [(0, 1), (7, 7), (1, -1)]
    assert R.confusion_of([res], 2).tolist() == [[0, 1, 0], [0, 0, 1], [0, 0, 0]]       # 7 lies outside [0, 2): left out


# ---- CPU: the API ------------------------------------------------------------------------------------------------------------------------
def test_edit_alignment_api_refuses_cpu_tensors_and_bad_shapes():
    hyp, ref = torch.zeros(2, 5, dtype=torch.int32), torch.zeros(2, 4, dtype=torch.int32)
    hl, rl = torch.tensor([5, 5]), torch.tensor([4, 2])
    with pytest.raises(RuntimeError, match='CPU'):
        Fq.edit_alignment(hyp, hl, ref, rl)
    with pytest.raises(RuntimeError, match='CPU'):
        layers.error_breakdown(hyp, None, ref, rl)
    with pytest.raises(ValueError, match='2 hypotheses, 3 references'):
        Fq.edit_alignment(hyp, hl, torch.zeros(3, 4, dtype=torch.int32), torch.tensor([1, 1, 1]))
    with pytest.raises(ValueError, match='1024'):
        Fq.edit_alignment(torch.zeros(2, 1025, dtype=torch.int32), hl, ref, rl)
    with pytest.raises(ValueError, match='1024'):
        Fq.edit_alignment(hyp, hl, torch.zeros(2, 1025, dtype=torch.int32), rl)
    for bad in (torch.zeros(3, 4, dtype=torch.int32), torch.zeros(3, 3, dtype=torch.int64), torch.zeros(9, dtype=torch.int32),
                torch.zeros(3, 6, dtype=torch.int32)[:, ::2], np.zeros((3, 3), dtype=np.int32)):
        with pytest.raises(ValueError, match='confusion'):
            Fq.edit_alignment(hyp, hl, ref, rl, confusion=bad)
    with pytest.raises(ValueError, match='256'):
        Fq.edit_alignment(hyp, hl, ref, rl, confusion=torch.zeros(258, 258, dtype=torch.int32))
    assert Fq.EditAlignment._fields == ('ref', 'hyp', 'length', 'counts')
    assert layers.ErrorBreakdown._fields == ('correct', 'substitutions', 'deletions', 'insertions', 'symbols', 'per')


def test_c_abi_argument_checks_come_before_any_pointer_is_touched():
    lib = _lib.lib()
    d = 16          # never dereferenced

    def call(B=2, hyp=d, hs=5, hl=d, ref=d, rs=4, rl=d, cm=None, classes=0, counts=d, ar=d, ah=d, al=d, conf=None, K=0, ws=None, n=0):
        return lib.qk_edit_align(B, hyp, hs, hl, ref, rs, rl, cm, classes, counts, ar, ah, al, conf, K, ws, n, None)
    assert call(B=-1) == _lib.QK_ERR_INVALID_ARG and call(hs=-1) == _lib.QK_ERR_INVALID_ARG and call(rs=-2) == _lib.QK_ERR_INVALID_ARG
    assert call(cm=d, classes=0) == _lib.QK_ERR_INVALID_ARG and call(conf=d, K=-1) == _lib.QK_ERR_INVALID_ARG
    assert call(hs=1025) == _lib.QK_ERR_UNSUPPORTED and call(rs=1025) == _lib.QK_ERR_UNSUPPORTED
    assert b'1024' in lib.qk_last_error()
    assert call(conf=d, K=257) == _lib.QK_ERR_UNSUPPORTED
    assert b'256' in lib.qk_last_error()
    assert call(B=0) == 0 and call(B=0, hyp=None, hl=None, ref=None, rl=None, counts=None, ar=None, ah=None, al=None) == 0
    for name in ('hyp', 'hl', 'ref', 'rl', 'counts'):
        assert call(**{name: None}) == _lib.QK_ERR_INVALID_ARG, name
    assert call(ar=None) == _lib.QK_ERR_INVALID_ARG and call(ah=None, al=None) == _lib.QK_ERR_INVALID_ARG      # NULL together or not at all
    assert b'together' in lib.qk_last_error()
    # the decision table: LDS when the strides let the whole image fit in 64 KB (no workspace), the workspace otherwise
    assert lib.qk_edit_align_workspace_bytes(256, 200, 75) == 0 and lib.qk_edit_align_workspace_bytes(256, 800, 75) == 0
    need = lib.qk_edit_align_workspace_bytes(3, 1024, 1024)
    assert need == 3 * 1024 * 17 * 16
    assert lib.qk_edit_align_workspace_bytes(0, 1024, 1024) == 0 and lib.qk_edit_align_workspace_bytes(2, 1025, 4) == 0
    assert call(B=3, hs=1024, rs=1024, ws=None, n=need) == _lib.QK_ERR_WORKSPACE
    assert call(B=3, hs=1024, rs=1024, ws=d, n=need - 8) == _lib.QK_ERR_WORKSPACE
    assert call(B=3, hs=1024, rs=1024, ws=d + 4, n=need) == _lib.QK_ERR_WORKSPACE


def test_top_confusions_on_a_hand_made_matrix():
    m = np.zeros((4, 4), dtype=np.int32)       # K = 3
    m[0, 0] = 50                               # the diagonal is never reported
    m[2, 1] = 5
    m[0, 2] = 5                                # tie with (2, 1): (0, 2) first
    m[3, 1] = 7                                # an insertion of 1
    m[1, 3] = 5                                # a deletion of 1: ties with both, between them by (ref, hyp)
    m[1, 0] = 1
    assert layers.top_confusions(m, k=10) == [(None, 1, 7), (0, 2, 5), (1, None, 5), (2, 1, 5), (1, 0, 1)]
    assert layers.top_confusions(torch.from_numpy(m), k=3, names=('a', 'b', 'c')) == [('<ins>', 'b', 7), ('a', 'c', 5), ('b', '<del>', 5)]
    assert layers.top_confusions(m, k=0) == [] and layers.top_confusions(np.zeros((4, 4), dtype=np.int32)) == []
    with pytest.raises(ValueError, match='square'):
        layers.top_confusions(np.zeros((3, 4)))
    with pytest.raises(ValueError, match='names'):
        layers.top_confusions(m, names=('a', 'b'))


def test_timit_phones_39_follow_the_class_map():
    cm = data.timit_61_to_39_class_map()
    names = data.TIMIT_PHONES_39
    assert len(names) == 39 == len(set(names)) and cm.max() == 38
    for c, p in enumerate(data.TIMIT_PHONES_61):
        if p == 'q':
            assert cm[c] == -1
        else:
            assert names[cm[c]] == data._FOLD_39.get(p, p), p
    assert names[0] == 'aa' and names[cm[data.TIMIT_PHONES_61.index('h#')]] == 'sil' and 'q' not in names
    seen = [cm[c] for c in range(61) if cm[c] >= 0]
    assert sorted(set(seen), key=seen.index) == list(range(39))                  # numbered by first appearance


# ---- GPU -----------------------------------------------------------------------------------------------------------------------------
def _dev():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    return torch.device('cuda:0')


def _device_args(dev, pairs, hs, rs):
    hyp, hl = R.padded([p[0] for p in pairs], hs)
    ref, rl = R.padded([p[1] for p in pairs], rs)
    return tuple(torch.from_numpy(a).to(dev) for a in (hyp, hl, ref, rl))


def _check(dev, pairs, hs, rs, class_map=None, K=None):
    """One device call on the pairs against the reference: counts, rows, lengths, matrix, the identities, the counts-only call."""
    hyp, hl, ref, rl = _device_args(dev, pairs, hs, rs)
    conf = torch.zeros((K + 1, K + 1), dtype=torch.int32, device=dev) if K is not None else None
    cm = torch.tensor(class_map, dtype=torch.int32) if class_map is not None else None
    res = Fq.edit_alignment(hyp, hl, ref, rl, class_map=cm, confusion=conf)
    B, A = len(pairs), hs + rs
    assert res.ref.shape == res.hyp.shape == (B, A) and res.length.shape == (B,) and res.counts.shape == (B, 4)
    assert all(t.dtype == torch.int32 and t.device == hyp.device for t in res)
    dist = Fq.edit_distance(hyp, hl, ref, rl, class_map=cm).cpu().numpy()
    only = Fq.edit_alignment(hyp, hl, ref, rl, class_map=cm, align=False)
    assert only.ref is None and only.hyp is None and only.length is None and torch.equal(only.counts, res.counts)
    ar, ah, al, counts = (t.cpu().numpy() for t in res)
    want = [R.align(h, r, class_map) for h, r in pairs]
    for b, w in enumerate(want):
        c, s, d, i = (int(v) for v in counts[b])
        assert (c, s, d, i) == w['counts'], (b, counts[b], w['counts'])
        assert c + s + d == w['R'] and c + s + i == w['H'] and s + d + i == dist[b] == w['distance'], b
        n = len(w['pairs'])
        assert al[b] == n, (b, al[b], n)
        assert [(int(x), int(y)) for x, y in zip(ar[b, :n], ah[b, :n])] == w['pairs'], b
        assert (ar[b, n:] == -1).all() and (ah[b, n:] == -1).all(), b
    if K is not None:
        assert np.array_equal(conf.cpu().numpy(), R.confusion_of(want, K))
    return want, counts


@functools.lru_cache(maxsize=None)
def _tiny():
    return tuple(R.tiny_pairs())


@pytest.mark.gpu
def test_every_tiny_pair_equals_the_reference():
    dev = _dev()
    want, counts = _check(dev, list(_tiny()), 4, 4, K=2)
    assert counts.sum(0).min() > 200                       # every kind of operation is well populated


# ref_stride classes around the kernel's lane widths (E = 1, 2, 2, 4, 8, 17 positions per lane) crossed with three hypothesis strides.
# The decision table is in LDS when the strides let the whole LDS image fit in 64 KB: 16 E bytes per hypothesis position plus the two
# sequences and the reversed operations; these four shapes are over it and take the workspace form, the other fourteen the LDS form.
_REF_STRIDES, _HYP_STRIDES = (63, 64, 127, 128, 300, 1024), (5, 200, 1024)
_E = {63: 1, 64: 2, 127: 2, 128: 4, 300: 8, 1024: 17}
_WORKSPACE_FORM = {(200, 1024), (1024, 128), (1024, 300), (1024, 1024)}        # (hyp_stride, ref_stride)


def _stride_batch(kind, hs, rs):
    """A pair at full stride on both sides, one with R = 0, one with H = 0 and a random one."""
    rng = np.random.RandomState(hs * 2048 + rs + (0 if kind == 'four_symbols' else 1))
    if kind == 'four_symbols':
        seq = lambda n: [int(t) for t in rng.randint(0, 4, size=n)]
        return [(seq(hs), seq(rs)), (seq(min(hs, 9)), []), ([], seq(min(rs, 11))), (seq(rng.randint(1, hs + 1)), seq(rng.randint(1, rs + 1)))]
    full_ref = [int(t) for t in rng.randint(0, 61, size=rs)]
    full_hyp = R.corrupt(rng, full_ref, 61)[:hs]
    full_hyp += [int(t) for t in rng.randint(0, 61, size=hs - len(full_hyp))]
    some = R.timit_like(rng, 3, lo=min(20, rs), hi=min(75, rs), max_hyp=hs)
    return [(full_hyp, full_ref), (some[0][0], []), ([], some[1][1]), some[2]]


@pytest.mark.gpu
@pytest.mark.parametrize('kind', ['four_symbols', 'timit_like'])
@pytest.mark.parametrize('hs', _HYP_STRIDES)
@pytest.mark.parametrize('rs', _REF_STRIDES)
def test_stride_classes_and_both_storage_forms(rs, hs, kind):
    dev = _dev()
    pairs = _stride_batch(kind, hs, rs)
    assert len(pairs[0][0]) == hs and len(pairs[0][1]) == rs and pairs[1][1] == [] and pairs[2][0] == []
    ws = _lib.lib().qk_edit_align_workspace_bytes(len(pairs), hs, rs)
    assert ws == (len(pairs) * hs * _E[rs] * 16 if (hs, rs) in _WORKSPACE_FORM else 0), (hs, rs, ws)
    _check(dev, pairs, hs, rs, K=4 if kind == 'four_symbols' else 61)


@pytest.mark.gpu
def test_timit_like_batch_populates_every_count():
    dev = _dev()
    pairs = R.timit_like(np.random.RandomState(0), 256, max_hyp=200)
    _, counts = _check(dev, pairs, 200, 75, K=61)
    print('C / S / D / I = %s' % (counts.sum(0),))
    assert counts.sum(0).min() >= 300


def _class_map_pairs():
    rng = np.random.RandomState(7)
    pairs = R.timit_like(rng, 12, symbols=62, max_hyp=90)                # the blank (61) and q among the tokens: both drop
    q = data.TIMIT_PHONES_61.index('q')
    pairs.append(([q, 61, q], [61, q]))                                  # everything drops
    pairs.append(([3, 70, -4, q, 5], [3, 70, 99, 5, 61]))                # tokens outside [0, classes) pass through
    pairs.append(([q] * 5, pairs[0][1]))                                 # only the hypothesis drops: all deletions
    return pairs, q


@pytest.mark.gpu
def test_class_map_61_to_39_with_dropped_and_passed_through_tokens():
    dev = _dev()
    pairs, q = _class_map_pairs()
    cm = data.timit_61_to_39_class_map()
    assert cm[q] == -1 and cm[61] == -1 and len(cm) == 62
    want, counts = _check(dev, pairs, 90, 75, class_map=cm.tolist(), K=39)
    assert want[12]['pairs'] == [] and tuple(counts[12]) == (0, 0, 0, 0)
    assert want[13]['pairs'] == [(cm[3], cm[3]), (70, 70), (99, -4), (cm[5], cm[5])] and tuple(counts[13]) == (3, 1, 0, 0)
    assert counts[14, 2] == want[14]['R'] > 0 and counts[14, 0] == counts[14, 1] == counts[14, 3] == 0


@pytest.mark.gpu
def test_every_output_element_is_written_and_nothing_else():
    dev = _dev()
    rng = np.random.RandomState(3)
    seq = lambda n: [int(t) for t in rng.randint(0, 3, size=n)]
    pairs = [(seq(7), seq(9)), ([], []), (seq(4), []), ([], seq(5)), (seq(7), seq(2)), (seq(1), seq(9))]
    hs, rs, K, guard, fill = 7, 9, 3, 64, 0x7f7f7f7f
    B, A = len(pairs), hs + rs
    hyp, hl, ref, rl = _device_args(dev, pairs, hs, rs)
    sizes = dict(counts=B * 4, ali_ref=B * A, ali_hyp=B * A, ali_len=B)
    bufs = {k: torch.full((n + guard,), fill, dtype=torch.int32, device=dev) for k, n in sizes.items()}
    conf = torch.full(((K + 1) * (K + 1) + guard,), 7, dtype=torch.int32, device=dev)
    lib = _lib.lib()
    assert lib.qk_edit_align_workspace_bytes(B, hs, rs) == 0
    rc = lib.qk_edit_align(B, hyp.data_ptr(), hs, hl.data_ptr(), ref.data_ptr(), rs, rl.data_ptr(), None, 0, bufs['counts'].data_ptr(),
                           bufs['ali_ref'].data_ptr(), bufs['ali_hyp'].data_ptr(), bufs['ali_len'].data_ptr(), conf.data_ptr(), K, None, 0,
                           torch.cuda.current_stream(dev).cuda_stream)
    assert rc == 0, lib.qk_last_error()
    torch.cuda.synchronize()
    for k, size in sizes.items():
        got = bufs[k].cpu().numpy()
        assert not (got[:size] == fill).any(), k
        assert (got[size:] == fill).all(), k
    want = [R.align(h, r) for h, r in pairs]
    got = conf.cpu().numpy()
    assert np.array_equal(got[:(K + 1) * (K + 1)].reshape(K + 1, K + 1), 7 + R.confusion_of(want, K))
    assert got[(K + 1) * (K + 1) - 1] == 7 and (got[(K + 1) * (K + 1):] == 7).all()
    assert np.array_equal(bufs['counts'][:B * 4].cpu().numpy().reshape(B, 4), np.array([w['counts'] for w in want]))
    # the counts-only call writes the counts and nothing else
    again = torch.full((B * 4 + guard,), fill, dtype=torch.int32, device=dev)
    rc = lib.qk_edit_align(B, hyp.data_ptr(), hs, hl.data_ptr(), ref.data_ptr(), rs, rl.data_ptr(), None, 0, again.data_ptr(), None, None, None,
                           None, 0, None, 0, torch.cuda.current_stream(dev).cuda_stream)
    assert rc == 0, lib.qk_last_error()
    assert torch.equal(again[:B * 4], bufs['counts'][:B * 4]) and (again[B * 4:] == fill).all()


@pytest.mark.gpu
def test_confusion_accumulates_over_batches():
    dev = _dev()
    rng = np.random.RandomState(11)
    first, second = R.timit_like(rng, 8, max_hyp=100), R.timit_like(rng, 5, max_hyp=100)
    conf = torch.zeros((62, 62), dtype=torch.int32, device=dev)
    results = []
    for pairs in (first, second):
        hyp, hl, ref, rl = _device_args(dev, pairs, 100, 75)
        results.append(Fq.edit_alignment(hyp, hl, ref, rl, confusion=conf, align=False))
    want = [R.align(h, r) for h, r in first + second]
    assert np.array_equal(conf.cpu().numpy(), R.confusion_of(want, 61)) and int(conf[61, 61]) == 0
    got = torch.cat([r.counts for r in results]).cpu().numpy()
    assert np.array_equal(got, np.array([w['counts'] for w in want]))
    # layers.error_breakdown: the batch sums, and label_error_rate's PER bit for bit
    hyp, hl, ref, rl = _device_args(dev, first, 100, 75)
    eb = layers.error_breakdown(hyp, None, ref, rl)                  # -1-padded rows
    errors, symbols, per = layers.label_error_rate(hyp, None, ref, rl)
    sums = np.array([w['counts'] for w in want[:8]]).sum(0)
    assert [int(v) for v in eb[:4]] == list(sums) and int(eb.symbols) == int(symbols) == sums[:3].sum()
    assert int(eb.substitutions + eb.deletions + eb.insertions) == int(errors) and torch.equal(eb.per, per)
    assert all(t.device == hyp.device and t.dim() == 0 for t in eb)


@pytest.mark.gpu
@pytest.mark.parametrize('shape', [(200, 75), (1024, 300)], ids=['lds', 'workspace'])
def test_two_calls_give_identical_bits(shape):
    dev = _dev()
    hs, rs = shape
    rng = np.random.RandomState(5)
    pairs = [([int(t) for t in rng.randint(0, 4, size=rng.randint(0, hs + 1))], [int(t) for t in rng.randint(0, 4, size=rng.randint(0, rs + 1))])
             for _ in range(16)]
    hyp, hl, ref, rl = _device_args(dev, pairs, hs, rs)
    ca, cb = (torch.zeros((5, 5), dtype=torch.int32, device=dev) for _ in range(2))
    a, b = Fq.edit_alignment(hyp, hl, ref, rl, confusion=ca), Fq.edit_alignment(hyp, hl, ref, rl, confusion=cb)
    for name, u, v in zip(a._fields, a, b):
        assert torch.equal(u, v), name
    assert torch.equal(ca, cb) and int(ca.sum()) == int(a.length.sum()) > 0


@pytest.mark.gpu
def test_model_error_breakdown_is_the_breakdown_of_its_decode():
    dev = _dev()
    g = torch.Generator(device=dev).manual_seed(4)
    x = torch.randn(2, 4, 41, 24, device=dev, generator=g).to(torch.bfloat16)
    labels = torch.randint(0, 61, (2, 6), device=dev, generator=g, dtype=torch.int32)
    ll = torch.tensor([[6], [3]], dtype=torch.int32, device=dev)
    il = torch.tensor([24, 20], dtype=torch.int32, device=dev)
    np.random.seed(0)
    torch.manual_seed(0)
    model = TimitQCNN(num_layers=2, start_filter=32, dropout=0.3)
    with torch.no_grad():
        model(x[:1])
    model.to(dev)
    model.train()
    cm = torch.from_numpy(data.timit_61_to_39_class_map())
    conf = torch.zeros((40, 40), dtype=torch.int32, device=dev)
    got = model.error_breakdown(x, labels, il, ll, class_map=cm, confusion=conf)
    assert model.training
    decoded, _ = model.decode(x, il)
    conf2 = torch.zeros_like(conf)
    want = layers.error_breakdown(decoded[0], None, labels, ll, cm, confusion=conf2)
    for name, u, v in zip(got._fields, got, want):
        assert torch.equal(u, v), name
    assert torch.equal(conf, conf2) and int(conf.sum()) == int(got.correct + got.substitutions + got.deletions + got.insertions)
    ev = model.evaluate(x, labels, il, ll, class_map=cm)
    assert torch.equal(got.per, ev.per) and int(got.symbols) == int(ev.symbols)
    assert int(got.substitutions + got.deletions + got.insertions) == int(ev.errors)
    with pytest.raises(ValueError, match='beam'):
        model.error_breakdown(x, labels, il, ll, lm=object())


def _sphere_bytes(samples):
    fields = ['database_id -s5 TIMIT', 'sample_count -i %d' % len(samples), 'sample_rate -i 16000', 'channel_count -i 1',
              'sample_n_bytes -i 2', 'sample_sig_bits -i 16', 'sample_byte_format -s2 01', 'sample_coding -s3 pcm', 'end_head']
    head = ('NIST_1A\n   1024\n' + '\n'.join(fields) + '\n').encode('ascii')
    return head + b' ' * (1024 - len(head)) + np.asarray(samples, dtype='<i2').tobytes()


@pytest.mark.gpu
def test_train_timit_example_prints_the_breakdown_and_the_confusions(tmp_path):
    _dev()
    rng = np.random.RandomState(0)
    for split, spk, utt in (('TRAIN', 'FCJF0', 'SA1'), ('TRAIN', 'MDAB0', 'SX9'), ('TEST', 'MDAB1', 'SI2'), ('TEST', 'FAKS0', 'SA2')):
        d = tmp_path / split / 'DR1' / spk
        d.mkdir(parents=True, exist_ok=True)
        n = int(rng.randint(14000, 20000))
        tone = 3000 * np.sin(2 * np.pi * rng.uniform(200, 3000) * np.arange(n) / 16000) + 300 * rng.randn(n)
        (d / (utt + '.WAV')).write_bytes(_sphere_bytes(tone.astype(np.int16)))
        phones = [data.TIMIT_PHONES_61[i] for i in rng.randint(0, 61, size=12)]
        cuts = np.linspace(0, n, len(phones) + 1).astype(int)
        (d / (utt + '.PHN')).write_text(''.join('%d %d %s\n' % (cuts[i], cuts[i + 1], p) for i, p in enumerate(phones)))
    cmd = [sys.executable, os.path.join(ROOT, 'examples', 'train_timit.py'), '--timit', str(tmp_path), '--confusions', '3', '--steps', '1',
           '--eval-every', '1', '--layers', '4', '--batch', '2']
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, env=dict(os.environ), timeout=600, universal_newlines=True)
    assert r.returncode == 0, r.stdout[-4000:]
    lines = re.findall(r'held-out %cor (\S+)\s+%sub (\S+)\s+%del (\S+)\s+%ins (\S+)\s+\((\d+) reference phones, (\d+) batches\)', r.stdout)
    assert len(lines) == 1, r.stdout[-4000:]
    cor, sub, dele, ins = (float(v) for v in lines[0][:4])
    assert abs(cor + sub + dele - 100.0) < 0.02 and ins >= 0 and 0 < int(lines[0][4]) <= 24 and int(lines[0][5]) == 1
    pairs = re.findall(r'confusion (\S+)\s+-> (\S+)\s+(\d+)', r.stdout)
    assert len(pairs) == 3, r.stdout[-4000:]
    names = set(data.TIMIT_PHONES_39) | {'<ins>', '<del>'}
    assert all(a in names and b in names and a != b and int(n) > 0 for a, b, n in pairs)
    assert [int(n) for _, _, n in pairs] == sorted((int(n) for _, _, n in pairs), reverse=True)
    per = re.findall(r'PER\(39\) (\S+) \((\d+) / (\d+)\)', r.stdout)
    assert len(per) == 1 and int(per[0][2]) == int(lines[0][4])          # the same reference phones as evaluate() counts
