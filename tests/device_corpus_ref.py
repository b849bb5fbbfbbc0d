"""NumPy + Python-integer restatement of include/qk_data.h for tests/test_device_corpus.py: the keyed permutation of an epoch, the
batch a position names, and the host-side batch assembly of examples/train_timit.py that the device path replaces.  Nothing here
imports the package under test."""
import numpy as np

M32 = 0xFFFFFFFF


def fmix(h):
    """fmix of the SpecAugment section of include/qk.h, on Python integers."""
    h &= M32
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & M32
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & M32
    h ^= h >> 16
    return h


def perm(seed, epoch, pos, nb, count_passes=None):
    """perm(seed, epoch, pos, nb) of include/qk_data.h.  count_passes: an optional one-element list that receives the passes walked."""
    k = 2
    while (1 << k) < nb:
        k += 2
    half = k // 2
    mask = (1 << half) - 1
    key = fmix(seed + 0x9E3779B1 * epoch)
    x, passes = pos, 0
    while True:
        left, right = x >> half, x & mask
        for r in range(4):
            left, right = right, left ^ (fmix(key ^ ((right * 0x9E3779B1 + r * 0x7F4A7C15 + 0x165667B1) & M32)) & mask)
        x = (left << half) | right
        passes += 1
        assert passes <= 1 << k, 'a cycle of a bijection on 2^k points is no longer than 2^k'
        if x < nb:
            if count_passes is not None:
                count_passes[0] = passes
            return x


def epoch_permutation(seed, epoch, nb):
    return [perm(seed, epoch, pos, nb) for pos in range(nb)]


def plan(position, nb, seed, shuffle):
    """{p, epoch, pos, row} of a position."""
    p = position & M32
    epoch, pos = divmod(p, nb)
    return [p, epoch, pos, perm(seed, epoch, pos, nb) if shuffle else pos]


# ---- examples/train_timit.py, restated ---------------------------------------------------------------------------------------------
def length_batches(counts, batch):
    """length_batches of the example on the sample counts: indices sorted by count (stable), cut into lists of up to `batch`."""
    order = sorted(range(len(counts)), key=lambda i: counts[i])
    return [order[i:i + batch] for i in range(0, len(order), batch)]


def padded_batches(counts, batch, drop_last=False):
    rows = length_batches(counts, batch)
    if drop_last and len(rows[-1]) < batch:
        rows.pop()
    out = np.full((len(rows), batch), -1, dtype=np.int32)
    for r, row in enumerate(rows):
        out[r, :len(row)] = row
    return out


def host_batch(waves, labels, idx):
    """The assembly of to_device of the example: (wave (B, max n) int16, n (B,), labels (B, max l) int32, label lengths (B,))."""
    n = [len(waves[i]) for i in idx]
    wave = np.zeros((len(idx), max(n)), dtype=np.int16)
    lab_len = [len(labels[i]) for i in idx]
    lab = np.zeros((len(idx), max(lab_len)), dtype=np.int32)
    for r, i in enumerate(idx):
        wave[r, :n[r]] = waves[i]
        lab[r, :lab_len[r]] = labels[i]
    return wave, np.array(n, dtype=np.int32), lab, np.array(lab_len, dtype=np.int32)


# ---- qk_corpus_batch ---------------------------------------------------------------------------------------------------------------
def corpus_batch(waves, labels, aux, batches, position, seed, shuffle, n_out, l_out):
    """Every output of qk_corpus_batch as a dict of numpy arrays (aux: None without aux words)."""
    nb, b = batches.shape
    pl = plan(position, nb, seed, shuffle)
    out = dict(wave=np.zeros((b, n_out), dtype=np.int16), lengths=np.zeros(b, dtype=np.int32),
               labels=np.zeros((b, l_out), dtype=np.int32), label_length=np.zeros(b, dtype=np.int32),
               aux=None if aux is None else np.full((b, l_out), -1, dtype=np.int32), utt=np.full(b, -1, dtype=np.int32),
               plan=np.array(pl, dtype=np.uint32).astype(np.int32))
    for s, u in enumerate(batches[pl[3]]):
        if u < 0 or u >= len(waves):
            continue
        n, l = min(len(waves[u]), n_out), min(len(labels[u]), l_out)
        out['wave'][s, :n] = waves[u][:n]
        out['lengths'][s] = n
        out['labels'][s, :l] = labels[u][:l]
        out['label_length'][s] = l
        if aux is not None:
            out['aux'][s, :l] = aux[u][:l]
        out['utt'][s] = u
    return out
