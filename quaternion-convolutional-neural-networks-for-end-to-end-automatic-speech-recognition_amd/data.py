"""Data readers: the DECODA text format -- counterpart of working_example.py:dataPrepDecodaQuaternion (:19-66) -- and TIMIT
(SPHERE / RIFF audio, .PHN phone labels, the 61 -> 39 scoring map).

DECODA:

One document per line: 250 space-separated `r,i,j,k` tokens, a TAB, 8 space-separated `l,l,l,l`
label tokens of which the first value is kept.  Returns float64 arrays like the reference:
x (N, 250, 4) for isquat (all components) or (N, 250, 3) (components 1..3), y (N, 8) one-hot.
"""
import numpy as np


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
