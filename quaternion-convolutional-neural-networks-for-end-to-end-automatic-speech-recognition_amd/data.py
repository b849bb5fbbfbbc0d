"""Data readers: the DECODA text format -- counterpart of working_example.py:dataPrepDecodaQuaternion (:19-66) -- and TIMIT
(SPHERE / RIFF audio, .PHN phone labels, the 61 -> 39 scoring map); and the device-resident corpus: pack_corpus / DeviceCorpus /
EpochSampler (epoch shuffling and batch assembly on the device, include/qk_data.h).

DECODA:

One document per line: 250 space-separated `r,i,j,k` tokens, a TAB, 8 space-separated `l,l,l,l`
label tokens of which the first value is kept.  Returns float64 arrays like the reference:
x (N, 250, 4) for isquat (all components) or (N, 250, 3) (components 1..3), y (N, 8) one-hot.
"""
import collections

import numpy as np
import torch


def dataPrepDecodaQuaternion(filename, isquat=True):
    nb_topics, nb_classes = 250, 8
    with open(filename, 'r') as f:
        raw = f.readlines()
    x = np.zeros((len(raw), nb_topics, 4 if isquat else 3))
    y = np.zeros((len(raw), nb_classes))
    for d, doc in enumerate(raw):
        feats, labels = doc.split('\t')[0].split(' '), doc.split('\t')[1].split(' ')
        for e, element in enumerate(feats):
            comp = element.split(',')
            x[d, e] = [float(c) for c in (comp[:4] if isquat else comp[1:4])]
        for l, label in enumerate(labels):
            y[d, l] = float(label.split(',')[0])
    return x, y


# ---- TIMIT -------------------------------------------------------------------------------------------------------------------------
# The 61 phone labels of the corpus' .PHN files; label c is class c of the model's 62 outputs, and class 61 is the CTC blank.
TIMIT_PHONES_61 = ('aa', 'ae', 'ah', 'ao', 'aw', 'ax', 'ax-h', 'axr', 'ay', 'b', 'bcl', 'ch', 'd', 'dcl', 'dh', 'dx', 'eh', 'el', 'em',
                   'en', 'eng', 'epi', 'er', 'ey', 'f', 'g', 'gcl', 'h#', 'hh', 'hv', 'ih', 'ix', 'iy', 'jh', 'k', 'kcl', 'l', 'm', 'n',
                   'ng', 'nx', 'ow', 'oy', 'p', 'pau', 'pcl', 'q', 'r', 's', 'sh', 't', 'tcl', 'th', 'uh', 'uw', 'ux', 'v', 'w', 'y',
                   'z', 'zh')
TIMIT_BLANK = len(TIMIT_PHONES_61)

# Lee & Hon (1989) folding for scoring: phone -> the 39-set representative ('q' is deleted).
_FOLD_39 = {'ao': 'aa', 'ax': 'ah', 'ax-h': 'ah', 'axr': 'er', 'hv': 'hh', 'ix': 'ih', 'el': 'l', 'em': 'm', 'en': 'n', 'nx': 'n',
            'eng': 'ng', 'zh': 'sh', 'ux': 'uw', 'pcl': 'sil', 'tcl': 'sil', 'kcl': 'sil', 'bcl': 'sil', 'dcl': 'sil', 'gcl': 'sil',
            'h#': 'sil', 'pau': 'sil', 'epi': 'sil', 'q': None}


def timit_61_to_39_class_map():
    """(62,) int32 class map for label_error_rate / TimitQCNN.evaluate: each of the 61 classes -> its Lee & Hon class in 0..38
    (numbered in order of first appearance in TIMIT_PHONES_61), 'q' -> -1 (dropped), the blank -> -1."""
    names = []
    cmap = np.full(TIMIT_BLANK + 1, -1, dtype=np.int32)
    for c, p in enumerate(TIMIT_PHONES_61):
        folded = _FOLD_39.get(p, p)
        if folded is None:
            continue
        if folded not in names:
            names.append(folded)
        cmap[c] = names.index(folded)
    return cmap


def _folded_names():
    names = []
    for p in TIMIT_PHONES_61:
        folded = _FOLD_39.get(p, p)
        if folded is not None and folded not in names:
            names.append(folded)
    return tuple(names)


# The 39 folded names in the numbering of timit_61_to_39_class_map() (first appearance): the row / column names of a 39-class
# confusion matrix (layers.top_confusions).
TIMIT_PHONES_39 = _folded_names()


def read_phn(path):
    """Phone names of a TIMIT .PHN file (lines `start end phone`), in order."""
    with open(path, 'r') as f:
        return [line.split()[2] for line in f if line.strip()]


def read_phn_segments(path):
    """[(start_sample, end_sample, phone)] of a TIMIT .PHN file (lines `start end phone`), in order: the hand-labelled boundaries
    read_phn leaves out -- the reference of a forced alignment (layers.boundary_agreement)."""
    out = []
    with open(path, 'r') as f:
        for line in f:
            if line.strip():
                start, end, phone = line.split()[:3]
                out.append((int(start), int(end), phone))
    return out


def _read_sphere(data, path):
    lines = data[:1024].split(b'\n')
    hdr_bytes = int(lines[1].strip())
    fields = {}
    for line in data[:hdr_bytes].split(b'\n')[2:]:
        parts = line.decode('ascii', 'replace').split(None, 2)
        if not parts or parts[0] == 'end_head':
            break
        if len(parts) == 3:
            fields[parts[0]] = parts[2].strip()
    coding = fields.get('sample_coding', 'pcm')
    if 'shorten' in coding:
        raise ValueError('%s: Shorten-compressed NIST SPHERE; decompress it first (e.g. with sph2pipe)' % path)
    if coding != 'pcm' or int(fields.get('sample_n_bytes', 2)) != 2 or int(fields.get('channel_count', 1)) != 1:
        raise ValueError('%s: only uncompressed 16-bit mono pcm SPHERE is supported (coding %r, %s bytes, %s channels)'
                         % (path, coding, fields.get('sample_n_bytes'), fields.get('channel_count')))
    order = fields.get('sample_byte_format', '01')
    if order not in ('01', '10'):
        raise ValueError('%s: unknown sample_byte_format %r' % (path, order))
    count = int(fields['sample_count']) if 'sample_count' in fields else (len(data) - hdr_bytes) // 2
    x = np.frombuffer(data, dtype='<i2' if order == '01' else '>i2', count=count, offset=hdr_bytes)
    return x.astype(np.int16)


def read_audio(path):
    """Samples of a TIMIT .WAV (NIST SPHERE: NIST_1A header, uncompressed 16-bit pcm, either byte order) or a RIFF WAV file
    (16-bit mono), as an int16 numpy array.  Shorten-compressed SPHERE raises ValueError."""
    with open(path, 'rb') as f:
        data = f.read()
    if data[:8] == b'NIST_1A\n':
        return _read_sphere(data, path)
    if data[:4] == b'RIFF':
        import io
        import wave
        with wave.open(io.BytesIO(data)) as w:
            if w.getsampwidth() != 2 or w.getnchannels() != 1:
                raise ValueError('%s: only 16-bit mono RIFF WAV is supported' % path)
            return np.frombuffer(w.readframes(w.getnframes()), dtype='<i2').astype(np.int16)
    raise ValueError('%s: neither NIST SPHERE nor RIFF WAV' % path)


# ---- Device-resident corpus (include/qk_data.h) ---------------------------------------------------------------------------------
def pack_corpus(waves, labels, aux=None):
    """Pack a corpus on the host in the layout of qk_corpus_t: a dict of numpy arrays wave_pack (int16; every utterance starts on a
    multiple of 8 samples, the gaps and the rounded-up end are zero), wave_off (int64), wave_len (int32), label_pack (int32),
    label_off (int64), label_len (int32) and aux_pack (int32, one word per label, or None).  Empty utterances and empty label
    sequences are allowed; the packs hold at least 8 samples / one word."""
    waves = [np.asarray(w) for w in waves]
    labels = [np.asarray(l) for l in labels]
    if not waves or len(labels) != len(waves) or (aux is not None and len(aux) != len(waves)):
        raise ValueError('pack_corpus: need at least one utterance and one label (and aux) sequence per utterance')
    for name, seqs, kinds in (('waveforms', waves, (np.int16,)), ('labels', labels, (np.int32, np.int64))):
        for i, a in enumerate(seqs):
            if a.ndim != 1 or (a.size and a.dtype.type not in kinds):
                raise TypeError('pack_corpus: %s[%d] must be a 1-D %s array, got %s of shape %s'
                                % (name, i, ' / '.join(k.__name__ for k in kinds), a.dtype, a.shape))
    wave_len = np.array([w.size for w in waves], dtype=np.int64)
    label_len = np.array([l.size for l in labels], dtype=np.int64)
    if wave_len.max() >= 1 << 31 or label_len.max() >= 1 << 31:
        raise ValueError('pack_corpus: an utterance of 2^31 samples or labels is not supported')
    padded = (wave_len + 7) // 8 * 8
    wave_off = np.concatenate([[0], np.cumsum(padded)[:-1]]).astype(np.int64)
    label_off = np.concatenate([[0], np.cumsum(label_len)[:-1]]).astype(np.int64)
    wave_pack = np.zeros(max(int(padded.sum()), 8), dtype=np.int16)
    label_pack = np.zeros(max(int(label_len.sum()), 1), dtype=np.int32)
    aux_pack = None if aux is None else np.full(label_pack.size, -1, dtype=np.int32)
    for u, (w, l) in enumerate(zip(waves, labels)):
        wave_pack[wave_off[u]:wave_off[u] + w.size] = w
        label_pack[label_off[u]:label_off[u] + l.size] = l
        if aux is not None:
            a = np.asarray(aux[u])
            if a.shape != l.shape:
                raise ValueError('pack_corpus: aux[%d] must hold one word per label (%d), got shape %s' % (u, l.size, a.shape))
            if a.size and (a.min() < -(1 << 31) or a.max() >= 1 << 31):
                raise ValueError('pack_corpus: aux[%d] does not fit int32' % u)
            aux_pack[label_off[u]:label_off[u] + l.size] = a
    return dict(wave_pack=wave_pack, wave_off=wave_off, wave_len=wave_len.astype(np.int32), label_pack=label_pack, label_off=label_off,
                label_len=label_len.astype(np.int32), aux_pack=aux_pack)


def epoch_perm(seed, epoch, pos, num_batches):
    """Python mirror of `perm` (include/qk_data.h): the row of the schedule that position `pos` of epoch `epoch` reads."""
    m32 = 0xFFFFFFFF

    def fmix(h):
        h ^= h >> 16
        h = h * 0x85EBCA6B & m32
        h ^= h >> 13
        h = h * 0xC2B2AE35 & m32
        return h ^ h >> 16
    k = 2
    while 1 << k < num_batches:
        k += 2
    half = k // 2
    mask = (1 << half) - 1
    key = fmix((seed + 0x9E3779B1 * epoch) & m32)
    x = pos
    while True:
        l, r = x >> half, x & mask
        for rnd in range(4):
            l, r = r, l ^ (fmix(key ^ ((r * 0x9E3779B1 + rnd * 0x7F4A7C15 + 0x165667B1) & m32)) & mask)
        x = l << half | r
        if x < num_batches:
            return x


Peek = collections.namedtuple('Peek', 'position epoch pos row indices n_out l_out')


class EpochSampler(object):
    """Epochs over length-sorted batches, shuffled on the device: the schedule and the cursor of DeviceCorpus.next_batch.

        sampler = EpochSampler(corpus.wave_len, batch=32, seed=args.seed)
        wave, lengths, labels, label_length = corpus.next_batch(sampler)

    batches: the utterance indices sorted by sample count (a stable sort) and cut into rows of `batch`; a short last row is padded
    with -1 (empty slots), or left out with drop_last.  Position p of the endless sequence reads row perm(seed, p // num_batches,
    p % num_batches) -- the keyed permutation of include/qk_data.h -- or row p % num_batches without shuffle: every epoch visits
    every row once, in a new order.  Data-parallel ranks use disjoint `batches` (build one sampler per rank from its share of the
    utterances).

    The position lives twice: in a host cursor, from which peek() and the tight mode of next_batch know the next row without
    reading the device, and in a one-element device cursor that next_batch advances with a device op, as the augmentation policies
    advance their counters -- the kernel reads that one in fixed mode, so a captured graph gathers a new batch on every replay.
    Replays advance only the device cursor; state_dict() reads it (that synchronises) and brings the host cursor up to date.
    state_dict() / load_state_dict() carry {'seed', 'counter'} like the policies': pass the sampler in save_checkpoint(policies=)."""

    def __init__(self, sample_counts, batch, seed=0, shuffle=True, drop_last=False):
        counts = [int(c) for c in np.asarray(sample_counts).reshape(-1)]
        if isinstance(batch, bool) or not isinstance(batch, (int, np.integer)) or batch < 1:
            raise ValueError('EpochSampler: batch must be an integer >= 1, got %r' % (batch,))
        if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or not 0 <= seed <= 0xFFFFFFFF:
            raise ValueError('EpochSampler: seed must be an integer in [0, 2^32), got %r' % (seed,))
        order = sorted(range(len(counts)), key=lambda i: counts[i])
        rows = [order[i:i + batch] for i in range(0, len(order), batch)]
        if drop_last and rows and len(rows[-1]) < batch:
            rows.pop()
        if not rows:
            raise ValueError('EpochSampler: %d utterances give no batch of %d%s' % (len(counts), batch, ' with drop_last' if drop_last else ''))
        self.batches = np.full((len(rows), int(batch)), -1, dtype=np.int32)
        for r, row in enumerate(rows):
            self.batches[r, :len(row)] = row
        self.row_samples = np.array([max(counts[i] for i in row) for row in rows], dtype=np.int64)
        self.seed, self.shuffle, self.drop_last = int(seed), bool(shuffle), bool(drop_last)
        self.position = 0               # the host cursor
        self._cursor = None             # one int32 on the device of the first batch; the kernel reads its 32 bits as unsigned
        self._batches_dev = None

    num_batches = property(lambda self: self.batches.shape[0])
    batch = property(lambda self: self.batches.shape[1])
    epoch = property(lambda self: self.position // self.num_batches)

    def peek(self, label_counts=None):
        """What the next batch is, from the host cursor alone (no device read): position, epoch, pos, the row of `batches`, its valid
        indices, and the tight widths: n_out (the row's longest utterance) and, given the label counts per utterance, l_out."""
        epoch, pos = divmod(self.position, self.num_batches)
        row = epoch_perm(self.seed, epoch, pos, self.num_batches) if self.shuffle else pos
        indices = [int(i) for i in self.batches[row] if i >= 0]
        l_out = None if label_counts is None else max(1, max(int(label_counts[i]) for i in indices))
        return Peek(self.position, epoch, pos, row, indices, max(1, int(self.row_samples[row])), l_out)

    def on(self, device):
        """(batches, cursor) on `device`: created by the first call, which fixes the sampler's device."""
        device = torch.device(device)
        if self._cursor is None:
            v = self.position - (1 << 32) if self.position >= 1 << 31 else self.position
            self._cursor = torch.full((1,), v, dtype=torch.int32, device=device)
            self._batches_dev = torch.from_numpy(self.batches).to(device)
        elif self._cursor.device != device:
            raise ValueError('EpochSampler: this sampler\'s cursor lives on %s, the corpus on %s' % (self._cursor.device, device))
        return self._batches_dev, self._cursor

    def advance(self):
        """One batch further: the device cursor by a device op (wraps mod 2^32, like the kernel's arithmetic), the host cursor with it."""
        self._cursor.add_(1)
        self.position = (self.position + 1) & 0xFFFFFFFF

    def state_dict(self):
        if self._cursor is not None:
            self.position = int(self._cursor.item()) & 0xFFFFFFFF
        return {'seed': self.seed, 'counter': self.position}

    def load_state_dict(self, d):
        """Takes what state_dict() gave; checked on the host before anything is written."""
        seed, counter = d['seed'], d['counter']
        for name, v in (('seed', seed), ('counter', counter)):
            if isinstance(v, bool) or not isinstance(v, int) or not 0 <= v <= 0xFFFFFFFF:
                raise ValueError('EpochSampler.load_state_dict: %s must be an integer in [0, 2^32), got %r' % (name, v))
        self.seed, self.position = seed, counter
        if self._cursor is not None:
            self._cursor.fill_(counter - (1 << 32) if counter >= 1 << 31 else counter)


class DeviceCorpus(object):
    """A corpus that lives on the device: packed on the host once (pack_corpus), one upload per array, batches assembled by one
    launch each (functional.corpus_batch, csrc/qk_data.hip).

        corpus = DeviceCorpus([u[0] for u in train], [u[1] for u in train], device=dev)
        sampler = EpochSampler(corpus.wave_len, batch, seed=seed)
        wave, lengths, labels, label_length = corpus.next_batch(sampler)
        x, frame_lengths = quaternion_fbank(wave, lengths, normalize='utterance')

    waves: int16 arrays; labels: int32 arrays; aux: optional integer arrays of one word per label (the hand-labelled start samples).
    wave_len, label_len and wave_off stay on the host as numpy arrays; .arrays is the functional.CorpusArrays of device tensors."""

    def __init__(self, waves, labels, aux=None, device=None):
        from . import functional as F
        device = torch.device('cuda' if device is None else device)
        if device.type != 'cuda':
            raise RuntimeError('DeviceCorpus: device %s is not a GPU. Batches are assembled only on the MI355X HIP path '
                               '(libqk_hip.so); there is no CPU fallback.' % device)
        if device.index is None:
            device = torch.device('cuda', torch.cuda.current_device())
        host = pack_corpus(waves, labels, aux)
        self.wave_len, self.label_len, self.wave_off = host['wave_len'], host['label_len'], host['wave_off']
        self.num_utts, self.device = int(self.wave_len.size), device
        self.arrays = F.CorpusArrays(**{k: None if v is None else torch.from_numpy(v).to(device) for k, v in host.items()})
        self.last_utt = self.last_plan = None

    has_aux = property(lambda self: self.arrays.aux_pack is not None)

    def _result(self, out, valid=None, widths=None):
        self.last_utt, self.last_plan = out.utt, out.plan
        wave, labels, aux = out.wave, out.labels, out.aux
        if widths is not None and widths != (wave.shape[1], labels.shape[1]):     # a batch of empty utterances or of no labels: the
            wave, labels = wave[:, :widths[0]], labels[:, :widths[1]]             # kernel's widths start at 1, the host assembly's at 0
            aux = aux if aux is None else aux[:, :widths[1]]
        res = (wave, out.lengths, labels, out.label_length[:, None]) + ((aux,) if aux is not None else ())
        return res if valid is None else tuple(t[:valid] for t in res)

    def _tight(self, indices):
        return int(self.wave_len[indices].max()), int(self.label_len[indices].max())

    def batch(self, indices):
        """The batch of an explicit list of utterance indices, at its tight widths: (wave (B, n) int16 zero-padded, lengths (B,)
        int32, labels (B, l) int32 zero-padded, label_length (B, 1) int32[, aux (B, l) int32 padded with -1])."""
        from . import functional as F
        indices = [int(i) for i in indices]
        if not indices or min(indices) < 0 or max(indices) >= self.num_utts:
            raise ValueError('DeviceCorpus.batch: need at least one index, all in [0, %d)' % self.num_utts)
        rows = torch.tensor([indices], dtype=torch.int32).to(self.device)
        widths = self._tight(indices)
        return self._result(F.corpus_batch(self.arrays, rows, n_out=max(1, widths[0]), l_out=max(1, widths[1]), return_utt=True,
                                           return_plan=True), None, widths)

    def next_batch(self, sampler, n_out=None, l_out=None):
        """The sampler's next batch, as batch() returns it, and the sampler one position further; .last_utt (B,) and .last_plan (4,)
        hold the utterance indices and {p, epoch, pos, row} of the call, on the device.

        Tight mode (the default): the host cursor names the row, so the widths are the row's maxima and a short last batch comes
        sliced to its valid rows -- shapes and bytes of a host-assembled batch.  Fixed mode (n_out= and l_out= given): the kernel
        reads the DEVICE cursor and the call has no step-dependent argument, so it captures into a graph that gathers a new batch
        on every replay (call it once before capturing).  Fixed mode needs drop_last=True and widths of at least the schedule's
        longest utterance and label sequence: ValueError before anything is launched."""
        from . import functional as F
        if not isinstance(sampler, EpochSampler):
            raise TypeError('DeviceCorpus.next_batch: sampler must be an EpochSampler, got %r' % (sampler,))
        if int(sampler.batches.max()) >= self.num_utts:
            raise ValueError('DeviceCorpus.next_batch: the sampler names utterance %d, the corpus holds %d' % (sampler.batches.max(), self.num_utts))
        if (n_out is None) != (l_out is None):
            raise ValueError('DeviceCorpus.next_batch: n_out and l_out go together (both: fixed mode; neither: tight mode)')
        rows, cursor = sampler.on(self.device)
        kw = dict(seed=sampler.seed, shuffle=sampler.shuffle, return_utt=True, return_plan=True)
        if n_out is None:
            nxt = sampler.peek()
            valid, widths = len(nxt.indices) if len(nxt.indices) < sampler.batch else None, self._tight(nxt.indices)
            out = F.corpus_batch(self.arrays, rows, position=nxt.position, n_out=max(1, widths[0]), l_out=max(1, widths[1]), **kw)  # (the corpus' own lengths: nothing is cut)
        else:
            if not sampler.drop_last:
                raise ValueError('DeviceCorpus.next_batch: fixed mode needs a sampler with drop_last=True (no short batch in a fixed shape)')
            used = sampler.batches.reshape(-1)
            need_n, need_l = int(self.wave_len[used].max()), int(self.label_len[used].max())
            if n_out < need_n or l_out < need_l:
                raise ValueError('DeviceCorpus.next_batch: n_out = %r, l_out = %r would cut utterances: the schedule needs at least '
                                 '%d samples and %d labels' % (n_out, l_out, need_n, need_l))
            out = F.corpus_batch(self.arrays, rows, cursor=cursor, n_out=n_out, l_out=l_out, **kw)
            valid = widths = None
        sampler.advance()
        return self._result(out, valid, widths)
