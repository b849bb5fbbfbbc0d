"""The device-resident corpus (include/qk_data.h; qcnn_amd.functional.corpus_batch, qcnn_amd.data.DeviceCorpus / EpochSampler):
epoch shuffling and batch assembly on the device, against the NumPy + Python-integer restatement of tests/device_corpus_ref.py and
the host-side assembly of examples/train_timit.py.  Every comparison is between integers: every tolerance is zero.
"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import device_corpus_ref as R
import guarded_alloc as GA

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# 37 utterances: empty, shorter than / equal to / one past one 16-byte group, and up to about 700 samples
LENGTHS = [0, 1, 7, 8, 9, 15, 16, 17, 23, 24, 25, 31, 33, 63, 64, 65, 100, 127, 128, 129, 200, 255, 256, 257, 300, 333, 400, 401, 450,
           499, 512, 513, 600, 640, 655, 699, 700]
SEED = 20231


def _dev():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    return torch.device('cuda:0')


def _header():
    return open(os.path.join(ROOT, 'include', 'qk_data.h')).read()


def _make_corpus(lengths, seed, max_labels=12):
    """Seeded utterances in a shuffled order: full-range int16 samples (never 0: a dropped sample cannot hide in the padding), label
    counts 0 .. max_labels (never label 0), aux words that are distinct per (utterance, label)."""
    rng = np.random.RandomState(seed)
    lengths = [int(lengths[i]) for i in rng.permutation(len(lengths))]
    waves, labels, aux = [], [], []
    for u, n in enumerate(lengths):
        w = rng.randint(-32768, 32768, size=n).astype(np.int16)
        w[w == 0] = 1
        waves.append(w)
        count = u % (max_labels + 1)
        labels.append(rng.randint(1, 62, size=count).astype(np.int32))
        aux.append((1000 * u + np.arange(count)).astype(np.int64))
    return waves, labels, aux


@pytest.fixture(scope='module')
def corpus37():
    """(waves, labels, aux): shared and never written."""
    return _make_corpus(LENGTHS, 7)


# ---- CPU part ------------------------------------------------------------------------------------------------------------------
def test_data_header_inventory_equals_the_third_symbol_table():
    from qcnn_amd import _lib
    lib = _lib.lib()
    h = _header()
    declared = set(re.findall(r'\b(qk_[a-z_0-9]+)\s*\(', h))
    declared -= {n for n in declared if n.endswith('_t')}
    assert declared == set(_lib.DATA_SYMBOLS), declared ^ set(_lib.DATA_SYMBOLS)
    for name in declared:
        assert hasattr(lib, name), name
    assert not set(_lib.DATA_SYMBOLS) & set(_lib.SYMBOLS) and not set(_lib.DATA_SYMBOLS) & set(_lib.OPT_SYMBOLS)
    main = open(os.path.join(ROOT, 'include', 'qk.h')).read()
    assert not any(name in main for name in _lib.DATA_SYMBOLS)
    decls = dict(re.findall(r'^int (qk_[a-z_0-9]+)\(([^;]*)\);', h, re.M | re.S))
    assert set(decls) == set(_lib.DATA_SYMBOLS)
    for name, args in decls.items():
        res, argtypes = _lib.DATA_SYMBOLS[name]
        assert res is ctypes.c_int and len(argtypes) == len(args.split(',')), name
        last = ' '.join(args.split(',')[-1].split())
        if name == 'qk_epoch_permutation':                          # host only
            assert 'stream' not in args
        else:
            assert last == 'void *stream' and argtypes[-1] is ctypes.c_void_p, name
    assert int(re.search(r'#define QK_CORPUS_PLAN_WORDS (\d+)', h).group(1)) == _lib.QK_CORPUS_PLAN_WORDS == 4


def test_data_structs_match_the_header():
    from qcnn_amd import _lib
    h = _header()
    ctype = {'const int16_t *': ctypes.c_void_p, 'const int64_t *': ctypes.c_void_p, 'const int32_t *': ctypes.c_void_p,
             'int64_t ': ctypes.c_int64, 'int32_t ': ctypes.c_int32, 'uint32_t ': ctypes.c_uint32}
    for struct, cls in (('qk_corpus_t', _lib.CorpusDesc), ('qk_batch_schedule_t', _lib.BatchScheduleDesc)):
        body = h[h.index('typedef struct %s {' % struct):h.index('} %s;' % struct)]
        fields = re.findall(r'^\s*(const int16_t \*|const int64_t \*|const int32_t \*|int64_t |int32_t |uint32_t )([a-z_]+);', body, re.M)
        assert [(n, ctype[t]) for t, n in fields] == list(cls._fields_), struct
    assert ctypes.sizeof(_lib.CorpusDesc) == 7 * 8 + 2 * 8 + 2 * 4 and ctypes.sizeof(_lib.BatchScheduleDesc) == 8 + 4 * 4


PERM_NB = list(range(1, 71)) + [255, 256, 257]


def test_reference_permutation_is_a_bijection_and_changes_with_the_epoch():
    longest = [0]
    for nb in PERM_NB:
        for seed in (0, 1, 0x9E3779B1, 0xFFFFFFFF):
            orders = []
            for epoch in (0, 1, 2, 0xFFFFFFFF):
                walked = [0]
                order = [R.perm(seed, epoch, pos, nb, walked) for pos in range(nb)]
                assert sorted(order) == list(range(nb)), (nb, seed, epoch)
                longest[0] = max(longest[0], walked[0])
                orders.append(order)
            if nb >= 8:
                assert orders[0] != orders[1] and orders[1] != orders[2], (nb, seed)
    assert longest[0] >= 2                                           # (the walk was walked)


def test_library_and_python_mirror_follow_the_reference_permutation():
    from qcnn_amd import data, functional as F
    for nb in (1, 2, 3, 4, 5, 16, 17, 37, 64, 65, 255, 256, 257, 1000):
        for seed, epoch in ((0, 0), (3, 1), (0xFFFFFFFF, 0xFFFFFFFF), (12345, 77)):
            want = R.epoch_permutation(seed, epoch, nb)
            assert F.epoch_permutation(seed, epoch, nb).tolist() == want, (nb, seed, epoch)
            assert [data.epoch_perm(seed, epoch, pos, nb) for pos in range(nb)] == want, (nb, seed, epoch)
    for bad in (dict(seed=-1), dict(seed=1 << 32), dict(epoch=1.5), dict(num_batches=0), dict(num_batches=True)):
        with pytest.raises(ValueError):
            F.epoch_permutation(**dict(dict(seed=0, epoch=0, num_batches=4), **bad))


def _host_block(n=64):
    """n words of HOST memory and a 16-byte aligned address inside them: non-NULL pointers for calls that must be refused before
    anything is launched."""
    buf = (ctypes.c_int64 * n)()
    return buf, (ctypes.addressof(buf) + 15) & ~15


def test_invalid_arguments_are_rejected_without_gpu():
    from qcnn_amd import _lib
    lib = _lib.lib()
    keep = [_host_block() for _ in range(16)]
    p = [a for _, a in keep]

    def call(corpus=None, sched=None, n_out=8, l_out=4, outs=None, null_corpus=False, null_sched=False, cursor=None):
        c = dict(wave_pack=p[0], wave_off=p[1], wave_len=p[2], label_pack=p[3], label_off=p[4], label_len=p[5], aux_pack=p[6],
                 wave_samples=64, label_words=16, num_utts=2, reserved=0)
        c.update(corpus or {})
        s = dict(batches=p[7], num_batches=2, batch=2, seed=0, shuffle=1)
        s.update(sched or {})
        o = dict(wave_out=p[8], lengths_out=p[9], labels_out=p[10], label_length_out=p[11], aux_out=p[12], utt_out=p[13], plan=p[14])
        o.update(outs or {})
        cd = _lib.CorpusDesc(*[c[n] for n, _ in _lib.CorpusDesc._fields_])
        sd = _lib.BatchScheduleDesc(*[s[n] for n, _ in _lib.BatchScheduleDesc._fields_])
        return lib.qk_corpus_batch(None if null_corpus else ctypes.byref(cd), None if null_sched else ctypes.byref(sd), 0, cursor, n_out,
                                   l_out, o['wave_out'], o['lengths_out'], o['labels_out'], o['label_length_out'], o['aux_out'],
                                   o['utt_out'], o['plan'], None)

    def err(rc, word, status=_lib.QK_ERR_INVALID_ARG):
        msg = lib.qk_last_error()
        assert rc == status and word.encode() in msg and b'qk_corpus_batch' in msg, (rc, word, msg)
    err(call(null_corpus=True), 'NULL')
    err(call(null_sched=True), 'NULL')
    for name in ('wave_pack', 'wave_off', 'wave_len', 'label_pack', 'label_off', 'label_len'):
        err(call(corpus={name: None}), 'NULL')
    err(call(sched=dict(batches=None)), 'NULL')
    for name in ('wave_out', 'lengths_out', 'labels_out', 'label_length_out'):
        err(call(outs={name: None}), 'NULL')
    err(call(corpus=dict(aux_pack=None)), 'aux_pack')               # aux_out without aux words
    err(call(sched=dict(batch=0)), 'batch')
    err(call(sched=dict(num_batches=0)), 'num_batches')
    err(call(n_out=0), 'n_out')
    err(call(l_out=0), 'l_out')
    err(call(corpus=dict(num_utts=-1)), 'num_utts')
    err(call(sched=dict(shuffle=2)), 'shuffle')
    err(call(corpus=dict(wave_pack=p[0] + 8)), 'alignment')
    err(call(outs=dict(wave_out=p[8] + 1)), 'alignment')
    err(call(cursor=p[15] + 2), 'alignment')
    err(call(sched=dict(batch=1 << 16), n_out=1 << 15), '2^31', _lib.QK_ERR_UNSUPPORTED)
    err(call(sched=dict(batch=1 << 16), l_out=1 << 15), '2^31', _lib.QK_ERR_UNSUPPORTED)
    out = (ctypes.c_int32 * 4)()
    assert lib.qk_epoch_permutation(0, 0, 0, out) == _lib.QK_ERR_INVALID_ARG
    assert lib.qk_epoch_permutation(0, 0, 4, None) == _lib.QK_ERR_INVALID_ARG
    assert all(v == 0 for buf, _ in keep for v in buf) and list(out) == [0] * 4       # nothing was written


def test_sampler_batches_are_the_examples_length_batches():
    from qcnn_amd.data import EpochSampler
    rng = np.random.RandomState(3)
    counts = rng.randint(0, 40, size=37).tolist()                   # many ties: the sort must be the example's stable sort
    for batch in (1, 4, 9, 37, 50):
        s = EpochSampler(counts, batch, shuffle=False)
        assert s.batches.dtype == np.int32 and np.array_equal(s.batches, R.padded_batches(counts, batch))
        rows = R.length_batches(counts, batch)
        assert [[int(i) for i in row if i >= 0] for row in s.batches] == rows
        assert s.row_samples.tolist() == [max(counts[i] for i in row) for row in rows]
    s = EpochSampler(counts, 4, drop_last=True)
    assert np.array_equal(s.batches, R.padded_batches(counts, 4, drop_last=True)) and s.batches.shape == (9, 4) and s.batches.min() >= 0
    assert EpochSampler(counts[:36], 4, drop_last=True).batches.shape == (9, 4)      # nothing to drop
    for kw in (dict(batch=0), dict(batch=2.5), dict(batch=True), dict(seed=-1), dict(seed=1 << 32), dict(batch=38, drop_last=True)):
        with pytest.raises(ValueError):
            EpochSampler(counts, **dict(dict(batch=4), **kw))
    with pytest.raises(ValueError):
        EpochSampler([], 4)


def test_sampler_peek_follows_the_reference_and_state_round_trips():
    from qcnn_amd.data import EpochSampler
    rng = np.random.RandomState(4)
    counts = rng.randint(0, 700, size=37).tolist()
    label_counts = rng.randint(0, 13, size=37).tolist()
    for shuffle in (True, False):
        s = EpochSampler(counts, 4, seed=SEED, shuffle=shuffle)
        assert s.state_dict() == dict(seed=SEED, counter=0)          # before first use
        nb = s.num_batches
        assert nb == 10
        for position in list(range(2 * nb + 3)) + [0xFFFFFFFF]:
            s.load_state_dict(dict(seed=SEED, counter=position))
            pk = s.peek(label_counts)
            p, epoch, pos, row = R.plan(position, nb, SEED, shuffle)
            assert (pk.position, pk.epoch, pk.pos, pk.row) == (p, epoch, pos, row)
            idx = R.length_batches(counts, 4)[row]
            assert pk.indices == idx
            assert pk.n_out == max(1, max(counts[i] for i in idx)) and pk.l_out == max(1, max(label_counts[i] for i in idx))
            assert s.peek().l_out is None and s.peek().n_out == pk.n_out
        assert s.state_dict() == dict(seed=SEED, counter=0xFFFFFFFF)
    fresh = EpochSampler(counts, 4, seed=1)
    fresh.load_state_dict(dict(seed=SEED, counter=13))               # before the first device use: kept for the cursor's creation
    assert fresh.state_dict() == dict(seed=SEED, counter=13) and fresh.epoch == 1 and fresh.peek().pos == 3
    for d in (dict(seed=-1, counter=0), dict(seed=0, counter=1 << 32), dict(seed=0, counter=True), dict(seed=0.0, counter=0)):
        with pytest.raises(ValueError):
            fresh.load_state_dict(d)
    assert fresh.state_dict() == dict(seed=SEED, counter=13)


def test_packing_layout(corpus37):
    from qcnn_amd.data import pack_corpus
    waves, labels, aux = corpus37
    for with_aux in (True, False):
        h = pack_corpus(waves, labels, aux if with_aux else None)
        assert h['wave_pack'].dtype == np.int16 and h['wave_off'].dtype == np.int64 and h['wave_len'].dtype == np.int32
        assert h['label_pack'].dtype == np.int32 and h['label_off'].dtype == np.int64 and h['label_len'].dtype == np.int32
        assert (h['wave_off'] % 8 == 0).all() and h['wave_pack'].size % 8 == 0
        assert h['wave_len'].tolist() == [len(w) for w in waves] and 0 in h['wave_len'] and 0 in h['label_len']
        covered = np.zeros(h['wave_pack'].size, dtype=bool)
        for u, w in enumerate(waves):
            off = int(h['wave_off'][u])
            assert np.array_equal(h['wave_pack'][off:off + len(w)], w) and not covered[off:off + len(w)].any()
            assert off + (len(w) + 7) // 8 * 8 <= h['wave_pack'].size
            covered[off:off + len(w)] = True
            lo = int(h['label_off'][u])
            assert np.array_equal(h['label_pack'][lo:lo + len(labels[u])], labels[u])
            if with_aux:
                assert np.array_equal(h['aux_pack'][lo:lo + len(labels[u])], aux[u])
        assert (h['wave_pack'][~covered] == 0).all()                 # the gaps are zero
        assert (h['aux_pack'] is None) == (not with_aux)
    h = pack_corpus([np.zeros(0, np.int16)], [np.zeros(0, np.int32)])                  # a corpus of one empty utterance
    assert h['wave_pack'].size == 8 and h['label_pack'].size == 1 and h['wave_len'].tolist() == [0]
    with pytest.raises(TypeError):
        pack_corpus([np.zeros(3, np.float32)], [np.zeros(1, np.int32)])
    with pytest.raises(ValueError):
        pack_corpus([np.zeros(3, np.int16)], [np.zeros(2, np.int32)], aux=[np.zeros(3, np.int64)])
    with pytest.raises(ValueError):
        pack_corpus([], [])


def test_device_corpus_refuses_a_cpu_device(corpus37):
    from qcnn_amd.data import DeviceCorpus
    waves, labels, _ = corpus37
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        DeviceCorpus(waves, labels, device='cpu')


# every entry of DATA_SYMBOLS against the hygiene case that exercises it, or the reason it has none
HYGIENE_COVER = {
    'qk_corpus_batch': 'test_corpus_batch_keeps_to_its_buffers: functional.corpus_batch, DeviceCorpus.batch / next_batch (tight and fixed)',
    'qk_epoch_permutation': 'host only: takes no device buffer (test_library_and_python_mirror_follow_the_reference_permutation)',
}


def test_every_data_entry_point_has_a_hygiene_case_or_a_reason():
    from qcnn_amd import _lib
    assert set(HYGIENE_COVER) == set(_lib.DATA_SYMBOLS)


# ---- GPU part ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def device_corpus(corpus37):
    """(with aux, without aux) DeviceCorpus of the 37 utterances: built once, never written."""
    from qcnn_amd.data import DeviceCorpus
    dev = _dev()
    waves, labels, aux = corpus37
    return DeviceCorpus(waves, labels, aux, device=dev), DeviceCorpus(waves, labels, device=dev)


def _assert_batch(got, want, what):
    for name in ('wave', 'lengths', 'labels', 'label_length', 'aux', 'utt', 'plan'):
        g, w = getattr(got, name), want[name]
        if g is None:
            continue
        assert w is not None, '%s: %s was returned but not expected' % (what, name)
        g = g.cpu().numpy()
        assert g.dtype == w.dtype and g.shape == w.shape, '%s: %s is %s %s, expected %s %s' % (what, name, g.dtype, g.shape, w.dtype, w.shape)
        if not np.array_equal(g, w):
            bad = np.argwhere(g != w)
            raise AssertionError('%s: %s differs in %d elements, first at %s: %d, expected %d'
                                 % (what, name, len(bad), tuple(bad[0]), g[tuple(bad[0])], w[tuple(bad[0])]))


def _width(mode, tight):
    return {'tight': tight, 'plus1': tight + 1, 'plus7': tight + 7, 'round8': (tight + 7) // 8 * 8}[mode]


@pytest.mark.gpu
@pytest.mark.parametrize('mode', ['tight', 'plus1', 'plus7', 'round8'])
@pytest.mark.parametrize('batch', [4, 9])
def test_every_output_equals_the_reference(corpus37, device_corpus, batch, mode):
    """Every row of the schedule (the short last row included), shuffled and not, with and without aux / utt / plan.  With 9 rows
    and an odd n_out the row starts cover all eight 2-byte residues of a 16-byte group."""
    from qcnn_amd import functional as F
    dev = _dev()
    waves, labels, aux = corpus37
    counts = [len(w) for w in waves]
    batches = R.padded_batches(counts, batch)
    nb = batches.shape[0]
    assert (batches[-1] < 0).sum() == batch - 1                      # 37 = 9 * 4 + 1 = 4 * 9 + 1
    rows = torch.from_numpy(batches).to(dev)
    seen_residues = set()
    for k, position in enumerate(list(range(nb)) + [nb + 1, 3 * nb - 1]):
        for shuffle in (False, True):
            row = R.plan(position, nb, SEED, shuffle)[3]
            idx = [i for i in batches[row] if i >= 0]
            n_out = _width(mode, max(1, max(counts[i] for i in idx)))
            l_out = max(1, max(len(labels[i]) for i in idx)) + (k % 2)
            with_aux, extras = bool((k + shuffle) % 2), bool(k % 3)
            corpus = device_corpus[0 if with_aux else 1]
            got = F.corpus_batch(corpus.arrays, rows, position=position, seed=SEED, shuffle=shuffle, n_out=n_out, l_out=l_out,
                                 return_utt=extras, return_plan=extras)
            assert (got.aux is not None) == with_aux and (got.utt is not None) == extras and (got.plan is not None) == extras
            want = R.corpus_batch(waves, labels, aux if with_aux else None, batches, position, SEED, shuffle, n_out, l_out)
            _assert_batch(got, want, 'batch %d %s position %d shuffle %d' % (batch, mode, position, shuffle))
            seen_residues |= {(got.wave.data_ptr() + 2 * b * n_out) % 16 for b in range(batch)}
            if with_aux:                                             # aux=False on a corpus that has aux words
                plain = F.corpus_batch(corpus.arrays, rows, position=position, seed=SEED, shuffle=shuffle, n_out=n_out, l_out=l_out, aux=False)
                assert plain.aux is None
                _assert_batch(plain, want, 'aux=False')
    if batch == 9:
        assert len(seen_residues) >= (8 if mode != 'round8' else 1), sorted(seen_residues)


@pytest.mark.gpu
def test_cursor_out_of_range_indices_and_the_epoch_order(corpus37, device_corpus):
    from qcnn_amd import functional as F
    dev = _dev()
    waves, labels, aux = corpus37
    counts = [len(w) for w in waves]
    batches = R.padded_batches(counts, 4)
    batches[2, 1], batches[5, 0], batches[5, 3], batches[7, 2] = 37, -5, 1000, 2 ** 31 - 1       # empty slots, never addresses
    nb = batches.shape[0]
    rows = torch.from_numpy(batches).to(dev)
    corpus = device_corpus[0]
    cursor = torch.zeros(1, dtype=torch.int32, device=dev)
    n_out, l_out = max(counts) + 3, 13
    visited = []
    for position in list(range(2 * nb)) + [0x7FFFFFFF, 0x80000000, 0xFFFFFFFF]:
        cursor.fill_(position - (1 << 32) if position >= 1 << 31 else position)
        got = F.corpus_batch(corpus.arrays, rows, position=12345, cursor=cursor, seed=SEED, shuffle=True, n_out=n_out, l_out=l_out,
                             return_utt=True, return_plan=True)          # the cursor wins over `position`
        want = R.corpus_batch(waves, labels, aux, batches, position, SEED, True, n_out, l_out)
        _assert_batch(got, want, 'cursor %d' % position)
        visited.append(int(got.plan[3]))
    for epoch in (0, 1):
        order = visited[epoch * nb:(epoch + 1) * nb]
        assert order == R.epoch_permutation(SEED, epoch, nb) == F.epoch_permutation(SEED, epoch, nb).tolist()
        assert sorted(order) == list(range(nb))
    assert visited[:nb] != visited[nb:2 * nb]
    for kw in (dict(position=-1), dict(position=1 << 32), dict(seed=1 << 32), dict(n_out=0), dict(l_out=0), dict(l_out=2.0),
               dict(cursor=torch.zeros(1, dtype=torch.int32)), dict(cursor=torch.zeros(2, dtype=torch.int32, device=dev)),
               dict(cursor=torch.zeros(1, dtype=torch.int64, device=dev))):
        with pytest.raises(ValueError):
            F.corpus_batch(corpus.arrays, rows, **dict(dict(n_out=8, l_out=4), **kw))
    with pytest.raises(TypeError):
        F.corpus_batch(corpus.arrays, rows.cpu(), n_out=8, l_out=4)
    with pytest.raises(TypeError):
        F.corpus_batch(corpus.arrays, rows.to(torch.int64), n_out=8, l_out=4)
    with pytest.raises(ValueError, match='aux'):
        F.corpus_batch(device_corpus[1].arrays, rows, n_out=8, l_out=4, aux=True)


@pytest.mark.gpu
def test_rows_longer_than_one_workgroup_and_views_at_odd_offsets():
    """Rows of several 16 KiB pieces (more than one workgroup per row, and more than one workgroup of labels), gathered into a
    wave_out that starts 2 bytes off a 16-byte boundary, through the C-ABI."""
    from qcnn_amd import _lib, functional as F
    from qcnn_amd.data import DeviceCorpus
    dev = _dev()
    waves, labels, aux = _make_corpus([20000, 8200, 16391, 3, 8191, 24999], 11, max_labels=90)
    labels[0], aux[0] = np.arange(1, 91, dtype=np.int32), np.arange(5000, 5090, dtype=np.int64)
    corpus = DeviceCorpus(waves, labels, aux, device=dev)
    batches = np.array([[0, 1, 2, 3], [4, 5, -1, 0]], dtype=np.int32)
    rows = torch.from_numpy(batches).to(dev)
    for position, n_out, l_out in ((0, 20003, 100), (1, 25000, 90), (1, 16385, 7)):
        got = F.corpus_batch(corpus.arrays, rows, position=position, n_out=n_out, l_out=l_out, return_utt=True, return_plan=True)
        _assert_batch(got, R.corpus_batch(waves, labels, aux, batches, position, 0, False, n_out, l_out), 'long rows %d' % n_out)
    # raw call into views: wave_out one element into its allocation, the small outputs one word in
    n_out, l_out, b = 16385, 7, 4
    desc, _ = F._corpus_desc('test', corpus.arrays)
    sched = _lib.BatchScheduleDesc(rows.data_ptr(), 2, b, 0, 0)
    raw = {k: torch.full((n,), -77, dtype=t, device=dev) for k, (n, t) in dict(
        wave=(b * n_out + 9, torch.int16), lengths=(b + 2, torch.int32), labels=(b * l_out + 2, torch.int32),
        label_length=(b + 2, torch.int32), aux=(b * l_out + 2, torch.int32), utt=(b + 2, torch.int32), plan=(6, torch.int32)).items()}
    rc = _lib.lib().qk_corpus_batch(ctypes.byref(desc), ctypes.byref(sched), 1, None, n_out, l_out, raw['wave'].data_ptr() + 2,
                                    *[raw[k].data_ptr() + 4 for k in ('lengths', 'labels', 'label_length', 'aux', 'utt', 'plan')],
                                    torch.cuda.current_stream().cuda_stream)
    _lib.check(rc, 'qk_corpus_batch')
    want = R.corpus_batch(waves, labels, aux, batches, 1, 0, False, n_out, l_out)
    for k, t in raw.items():
        h = t.cpu().numpy()
        assert h[0] == -77 and (h[1 + want[k].size:] == -77).all(), '%s: written outside its view' % k
        assert np.array_equal(h[1:1 + want[k].size].reshape(want[k].shape), want[k]), k


@pytest.mark.gpu
def test_truncation_clamps_in_the_c_abi_and_raises_in_python(corpus37, device_corpus):
    from qcnn_amd import functional as F
    from qcnn_amd.data import EpochSampler
    dev = _dev()
    waves, labels, aux = corpus37
    counts = [len(w) for w in waves]
    batches = R.padded_batches(counts, 4, drop_last=True)
    rows = torch.from_numpy(batches).to(dev)
    corpus = device_corpus[0]
    cut_labels = False
    for n_out, l_out in ((1, 1), (5, 2), (8, 3), (13, 1), (300, 5)):
        for position in (0, 4, 8):
            got = F.corpus_batch(corpus.arrays, rows, position=position, n_out=n_out, l_out=l_out, return_utt=True, return_plan=True)
            want = R.corpus_batch(waves, labels, aux, batches, position, 0, False, n_out, l_out)
            _assert_batch(got, want, 'clamped to %d, %d' % (n_out, l_out))
            cut_labels |= any(len(labels[i]) > l_out for i in batches[position])
    assert (want['lengths'] == 300).all() and cut_labels             # waveforms and labels were cut
    sampler = EpochSampler(corpus.wave_len, 4, seed=SEED, drop_last=True)
    need_n, need_l = max(counts[i] for i in batches.reshape(-1)), max(len(labels[i]) for i in batches.reshape(-1))
    for kw in (dict(n_out=need_n - 1, l_out=need_l), dict(n_out=need_n, l_out=need_l - 1)):
        with pytest.raises(ValueError, match='would cut'):
            corpus.next_batch(sampler, **kw)
    with pytest.raises(ValueError, match='go together'):
        corpus.next_batch(sampler, n_out=need_n)
    with pytest.raises(ValueError, match='drop_last'):
        corpus.next_batch(EpochSampler(corpus.wave_len, 4, seed=SEED), n_out=need_n, l_out=need_l)
    assert sampler.state_dict() == dict(seed=SEED, counter=0)        # a refused call moves nothing
    with pytest.raises(ValueError):
        corpus.batch([0, 37])
    with pytest.raises(ValueError):
        corpus.batch([])


@pytest.mark.gpu
@pytest.mark.parametrize('batch', [4, 9])
def test_tight_mode_is_byte_identical_to_the_host_assembly(corpus37, device_corpus, batch):
    from qcnn_amd.data import EpochSampler
    _dev()
    waves, labels, aux = corpus37
    counts = [len(w) for w in waves]
    host_rows = R.length_batches(counts, batch)
    nb = len(host_rows)
    for corpus in device_corpus:
        sampler = EpochSampler(corpus.wave_len, batch, seed=SEED)
        visited = []
        for position in range(2 * nb):
            pk = sampler.peek()
            assert pk.position == position and sampler.epoch == position // nb
            out = corpus.next_batch(sampler)
            idx = host_rows[R.plan(position, nb, SEED, True)[3]]
            assert pk.indices == idx
            visited.append(pk.row)
            wave, n, lab, lab_len = R.host_batch(waves, labels, idx)
            assert len(out) == (5 if corpus.has_aux else 4)
            for g, w in zip(out[:4], (wave, n, lab, lab_len[:, None])):
                assert g.is_contiguous() and g.dtype == torch.from_numpy(w).dtype and tuple(g.shape) == w.shape, (position, g.shape, w.shape)
                assert np.array_equal(g.cpu().numpy(), w), position
            if corpus.has_aux:
                want_aux = np.full(lab.shape, -1, dtype=np.int32)
                for r, i in enumerate(idx):
                    want_aux[r, :len(aux[i])] = aux[i]
                assert np.array_equal(out[4].cpu().numpy(), want_aux)
            assert corpus.last_utt.cpu().tolist()[:len(idx)] == idx and corpus.last_plan.cpu().tolist() == R.plan(position, nb, SEED, True)
        assert sorted(visited[:nb]) == sorted(visited[nb:]) == list(range(nb)) and visited[:nb] != visited[nb:]
        assert sampler.state_dict() == dict(seed=SEED, counter=2 * nb)
        # an explicit index list
        idx = [36, 0, 5, 5, 17]
        wave, n, lab, lab_len = R.host_batch(waves, labels, idx)
        out = corpus.batch(idx)
        for g, w in zip(out[:4], (wave, n, lab, lab_len[:, None])):
            assert np.array_equal(g.cpu().numpy(), w)


@pytest.mark.gpu
def test_fixed_mode_replays_new_batches_from_one_captured_graph(corpus37, device_corpus):
    """One next_batch captured on a single stream (a linear graph); 2 * num_batches + 1 replays cross two epoch boundaries."""
    from qcnn_amd.data import EpochSampler
    dev = _dev()
    waves, labels, aux = corpus37
    counts = [len(w) for w in waves]
    corpus = device_corpus[0]
    batches = R.padded_batches(counts, 4, drop_last=True)
    nb = batches.shape[0]
    n_out, l_out = max(counts) + 3, 12
    corpus.next_batch(EpochSampler(corpus.wave_len, 4, drop_last=True), n_out=n_out, l_out=l_out)      # (loads the kernel before the capture)
    sampler = EpochSampler(corpus.wave_len, 4, seed=SEED, drop_last=True)
    assert np.array_equal(sampler.batches, batches)
    sampler.on(dev)                                                  # the cursor and the schedule move before the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = corpus.next_batch(sampler, n_out=n_out, l_out=l_out)
        utt, plan = corpus.last_utt, corpus.last_plan
    sampler.load_state_dict(dict(seed=SEED, counter=0))              # capturing ran nothing: both cursors back to 0

    def replay_and_check(position):
        graph.replay()
        want = R.corpus_batch(waves, labels, aux, batches, position, SEED, True, n_out, l_out)
        assert utt.cpu().tolist() == want['utt'].tolist() and plan.cpu().tolist() == want['plan'].tolist(), position
        for g, name in zip(out, ('wave', 'lengths', 'labels', 'label_length', 'aux')):
            assert np.array_equal(g.cpu().numpy().reshape(want[name].shape), want[name]), (position, name)
        return int(want['plan'][3])
    visited = [replay_and_check(position) for position in range(2 * nb + 1)]
    assert sorted(visited[:nb]) == sorted(visited[nb:2 * nb]) == list(range(nb)) and visited[:nb] != visited[nb:2 * nb]
    assert visited[:nb] == R.epoch_permutation(SEED, 0, nb) and visited[2 * nb] == R.perm(SEED, 2, 0, nb)
    assert sampler.state_dict() == dict(seed=SEED, counter=2 * nb + 1)          # read from the device: the replays moved only that cursor
    assert sampler.position == 2 * nb + 1 and sampler.epoch == 2
    sampler.load_state_dict(dict(seed=SEED, counter=nb + 3))         # resume in the middle of epoch 1
    resumed = [replay_and_check(position) for position in range(nb + 3, 2 * nb)]
    assert resumed == visited[nb + 3:2 * nb]


@pytest.mark.gpu
def test_corpus_batch_keeps_to_its_buffers(corpus37, device_corpus, monkeypatch):
    """The same calls under guard bands and the two fills: no stray write, no unwritten element, bit-identical outputs."""
    from qcnn_amd import functional as F
    from qcnn_amd.data import EpochSampler
    dev = _dev()
    waves, labels, aux = corpus37
    counts = [len(w) for w in waves]
    rows9 = torch.from_numpy(R.padded_batches(counts, 9)).to(dev)

    def run(alloc):
        out = {}

        def keep(tag, res):
            names = res._fields if hasattr(res, '_fields') else ('wave', 'lengths', 'labels', 'label_length', 'aux')
            out.update({'%s_%s' % (tag, n): t for n, t in zip(names, res) if t is not None})
        for mode in ('tight', 'plus1', 'plus7', 'round8'):
            for position in (0, 2, 4):                               # 4: the short last row
                idx = [i for i in R.padded_batches(counts, 9)[position] if i >= 0]
                n_out = _width(mode, max(1, max(counts[i] for i in idx)))
                for corpus, extras in ((device_corpus[0], True), (device_corpus[1], False)):
                    keep('f_%s_%d_%d' % (mode, position, extras),
                         F.corpus_batch(corpus.arrays, rows9, position=position, n_out=n_out, l_out=13, return_utt=extras, return_plan=extras))
        corpus = device_corpus[0]
        tight = EpochSampler(corpus.wave_len, 4, seed=SEED)
        for k in range(tight.num_batches):
            keep('tight_%d' % k, corpus.next_batch(tight))
            out['tight_%d_utt' % k], out['tight_%d_plan' % k] = corpus.last_utt, corpus.last_plan
        fixed = EpochSampler(corpus.wave_len, 4, seed=SEED, drop_last=True)
        for k in range(3):
            keep('fixed_%d' % k, corpus.next_batch(fixed, n_out=max(counts) + 5, l_out=12))
        keep('explicit', corpus.batch([36, 0, 5, 17, 5]))
        return out
    res = GA.run_twice(run, monkeypatch, modules=(F,))
    GA.assert_hygiene(res, 'corpus_batch: ')


@pytest.mark.gpu
def test_filter_bank_of_a_gathered_batch_equals_that_of_the_host_batch(corpus37, device_corpus):
    from qcnn_amd.features import quaternion_fbank
    dev = _dev()
    waves, labels, _ = corpus37
    counts = [len(w) for w in waves]
    idx = R.length_batches(counts, 4)[-2]                            # the last full row: 600 .. 699 samples
    wave, n, _, _ = R.host_batch(waves, labels, idx)
    got_wave, got_n = device_corpus[1].batch(idx)[:2]
    want = quaternion_fbank(torch.from_numpy(wave).to(dev), torch.tensor(n.tolist(), dtype=torch.int32), normalize='utterance')
    got = quaternion_fbank(got_wave, got_n, normalize='utterance')
    assert got[0].shape == want[0].shape and got[0].shape[0] == 4 and got[0].shape[-1] >= 3
    assert torch.equal(got[0].view(torch.int32).cpu(), want[0].view(torch.int32).cpu())
    assert torch.equal(got[1].cpu(), want[1].cpu())


@pytest.mark.gpu
def test_train_timit_example_with_device_corpus(tmp_path):
    """The example on a ten-utterance tree with --device-corpus: four batches per epoch, so step 5 is in epoch 1; the checkpoint
    carries the sampler's position behind the augmentation counter.  (This test is about the script: one child process.)"""
    import subprocess
    import sys
    from qcnn_amd import data
    from test_fbank import signals, sphere_bytes
    _dev()
    rng = np.random.RandomState(0)
    tree = tmp_path / 'timit'
    for split, count in (('TRAIN', 7), ('TEST', 3)):
        for k in range(count):
            d = tree / split / 'DR1' / ('S%02d' % k)
            d.mkdir(parents=True)
            n = int(rng.randint(14000, 20000))
            (d / ('SA%d.WAV' % k)).write_bytes(sphere_bytes(signals([n], seed=int(rng.randint(1000)))[0].astype(np.int16)))
            phones = [data.TIMIT_PHONES_61[i] for i in rng.randint(0, 61, size=int(rng.randint(8, 14)))]
            cuts = np.linspace(0, n, len(phones) + 1).astype(int)
            (d / ('SA%d.PHN' % k)).write_text(''.join('%d %d %s\n' % (cuts[i], cuts[i + 1], p) for i, p in enumerate(phones)))
    ckpt = str(tmp_path / 'run.pt')
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'examples', 'train_timit.py'), '--timit', str(tree), '--layers', '4', '--batch', '2',
                        '--steps', '5', '--eval-every', '5', '--align-eval', '--specaug', '--seed', '5', '--device-corpus', '--checkpoint', ckpt],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, env=dict(os.environ), timeout=600, universal_newlines=True)
    assert r.returncode == 0, r.stdout[-4000:]
    assert '4 batches per epoch' in r.stdout, r.stdout[-4000:]
    assert re.findall(r'step\s+(\d+)\s+loss \S+  epoch (\d+)', r.stdout) == [('1', '0'), ('5', '1')], r.stdout[-4000:]
    assert len(re.findall(r'held-out boundary agreement within 20 ms \S+ \(\d+ / \d+\)', r.stdout)) == 1, r.stdout[-4000:]
    saved = torch.load(ckpt, map_location='cpu', weights_only=True)
    assert saved['extra']['step'] == 5 and saved['policies'] == [dict(seed=5, counter=5), dict(seed=5, counter=5)]
