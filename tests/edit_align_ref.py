"""Plain restatement of the scoring alignment of include/qk.h, "Scoring alignment", for tests/test_edit_align.py: the Levenshtein DP
with the backtrack rule (align), an enumeration of every monotone alignment (enumerate_alignments) that pins the rule on tiny pairs,
and the generators of the test data.  Numpy only; nothing here touches the device."""
import itertools

import numpy as np

DIAG, DEL, INS = 0, 1, 2        # the order of the tie rule: diagonal < deletion < insertion


def clamp(n, stride):
    return min(max(int(n), 0), int(stride))


def apply_map(seq, class_map):
    """A token t in [0, classes) becomes class_map[t] and is dropped when that is negative; any other token passes through."""
    if class_map is None:
        return [int(t) for t in seq]
    out = []
    for t in seq:
        t = int(t)
        if 0 <= t < len(class_map):
            t = int(class_map[t])
            if t < 0:
                continue
        out.append(t)
    return out


def distance_table(h, r):
    """D[i][j] (H + 1, R + 1) int64, one vectorised row at a time: the chain of deletions inside a row is a running minimum."""
    H, R = len(h), len(r)
    ra = np.asarray(r, dtype=np.int64).reshape(R)
    cols = np.arange(R + 1)
    D = np.empty((H + 1, R + 1), dtype=np.int64)
    D[0] = cols
    for i in range(1, H + 1):
        row = np.empty(R + 1, dtype=np.int64)
        row[0] = i
        row[1:] = np.minimum(D[i - 1, 1:] + 1, D[i - 1, :-1] + (ra != h[i - 1]))
        D[i] = cols + np.minimum.accumulate(row - cols)
    return D


def align(h, r, class_map=None):
    """The alignment of hypothesis h to reference r (sequences of ints, already cut to their lengths).  Returns a dict:
    counts (C, S, D, I); ops [DIAG | DEL | INS] and pairs [(ref token | -1, hyp token | -1)] in forward order; distance; H, R after
    the map."""
    h, r = apply_map(h, class_map), apply_map(r, class_map)
    D = distance_table(h, r)
    i, j = len(h), len(r)
    ops, pairs = [], []
    c = s = d = ins = 0
    while i > 0 or j > 0:
        if i > 0 and j > 0 and D[i, j] == D[i - 1, j - 1] + (h[i - 1] != r[j - 1]):
            ops.append(DIAG)
            pairs.append((r[j - 1], h[i - 1]))
            if h[i - 1] == r[j - 1]:
                c += 1
            else:
                s += 1
            i, j = i - 1, j - 1
        elif j > 0 and D[i, j] == D[i, j - 1] + 1:
            ops.append(DEL)
            pairs.append((r[j - 1], -1))
            d += 1
            j -= 1
        else:
            assert i > 0 and D[i, j] == D[i - 1, j] + 1
            ops.append(INS)
            pairs.append((-1, h[i - 1]))
            ins += 1
            i -= 1
    return dict(counts=(c, s, d, ins), ops=ops[::-1], pairs=pairs[::-1], distance=int(D[len(h), len(r)]), H=len(h), R=len(r))


def enumerate_alignments(h, r):
    """Every monotone alignment of h to r as (cost, ops in forward order, (S, D, I)): all orders of diagonals, deletions and
    insertions that consume both sequences.  Exponential: tiny pairs only."""
    h, r = list(h), list(r)
    out = []

    def walk(i, j, ops, s, d, ins):
        if i == len(h) and j == len(r):
            out.append((s + d + ins, tuple(ops), (s, d, ins)))
            return
        if i < len(h) and j < len(r):
            walk(i + 1, j + 1, ops + [DIAG], s + (h[i] != r[j]), d, ins)
        if j < len(r):
            walk(i, j + 1, ops + [DEL], s, d + 1, ins)
        if i < len(h):
            walk(i + 1, j, ops + [INS], s, d, ins + 1)
    walk(0, 0, [], 0, 0, 0)
    return out


def tiny_pairs():
    """All 961 (h, r) pairs over the alphabet {0, 1} with lengths 0 .. 4 each."""
    seqs = [list(s) for n in range(5) for s in itertools.product((0, 1), repeat=n)]
    return [(h, r) for h in seqs for r in seqs]


def confusion_of(results, K):
    """The (K + 1, K + 1) matrix a list of align() results adds up to: row K insertions, column K deletions, pairs with a token
    outside [0, K) left out."""
    m = np.zeros((K + 1, K + 1), dtype=np.int64)
    for res in results:
        for op, (rt, ht) in zip(res['ops'], res['pairs']):
            r_in, h_in = 0 <= rt < K, 0 <= ht < K
            if op == DIAG:
                if r_in and h_in:
                    m[rt, ht] += 1
            elif op == DEL:
                if r_in:
                    m[rt, K] += 1
            elif h_in:
                m[K, ht] += 1
    return m


def padded(seqs, stride, fill=-1):
    """(len(seqs), stride) int32 rows and their lengths."""
    out = np.full((len(seqs), stride), fill, dtype=np.int32)
    for b, s in enumerate(seqs):
        out[b, :len(s)] = s
    return out, np.array([len(s) for s in seqs], dtype=np.int32)


def corrupt(rng, ref, symbols, p_drop=0.08, p_sub=0.20, p_extra=0.05):
    """A recogniser-like hypothesis of `ref`: about 8 % of the tokens dropped, 20 % replaced, 5 % followed by an extra one."""
    hyp = []
    for t in ref:
        u = rng.rand()
        if u < p_drop:
            pass
        elif u < p_drop + p_sub:
            hyp.append(int(rng.randint(symbols)))
        else:
            hyp.append(int(t))
        if rng.rand() < p_extra:
            hyp.append(int(rng.randint(symbols)))
    return hyp


def timit_like(rng, n, symbols=61, lo=20, hi=75, max_hyp=None):
    """n (hyp, ref) pairs: a reference of lo .. hi of `symbols` symbols and its corrupt() hypothesis (cut to max_hyp tokens)."""
    pairs = []
    for _ in range(n):
        ref = [int(t) for t in rng.randint(0, symbols, size=rng.randint(lo, hi + 1))]
        hyp = corrupt(rng, ref, symbols)
        pairs.append((hyp[:max_hyp] if max_hyp is not None else hyp, ref))
    return pairs
