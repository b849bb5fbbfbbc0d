"""TEST INFRASTRUCTURE -- CTC forced alignment (include/qk.h, "CTC forced alignment") restated in float64.

Two independent statements of the same definition:

  * viterbi(): the max-plus recursion over the extended label sequence blank, l1, blank, ..., lL, blank with the alpha recursion's
    transitions (stay, from s - 1, from s - 2 when s is a label state whose label differs from the one two states back), the start in
    state 0 or 1, the end in state S - 1 or S - 2, and the header's tie rule (stay over s - 1 over s - 2; S - 1 over S - 2; -inf never
    wins);
  * enumerate_paths(): every one of the C^Tn frame-level class paths that collapses (oracle.ctc_enum.collapse) to the labels, scored
    directly -- no recursion, no states.

Emissions are those of K.ctc_batch_cost: lp[t] = log_softmax(log(y_pred[t] + 1e-7)).  Only tests import this.
"""
import itertools

import numpy as np

from oracle.ctc_enum import collapse

EPSILON = 1e-7


def log_probs(y_b, eps=EPSILON):
    """lp (T, C) float64 of one sample's posteriors."""
    u = np.log(np.asarray(y_b, dtype=np.float64) + eps)
    m = u.max(axis=-1, keepdims=True)
    return u - (m + np.log(np.exp(u - m).sum(axis=-1, keepdims=True)))


def clamp_lengths(T, Lmax, tn, ln):
    return min(max(int(tn), 0), T), min(max(int(ln), 0), Lmax)


def path_score(lp, path):
    """Log-probability of a frame-level class path (its length is the number of frames that count)."""
    return float(sum(lp[t, c] for t, c in enumerate(path)))


def segments(states, ln):
    """(starts, ends) of the label states of a state path: label i holds the frames spent in state 2 i + 1."""
    starts, ends = [-1] * ln, [-1] * ln
    for t, s in enumerate(states):
        if s & 1:
            if starts[s >> 1] < 0:
                starts[s >> 1] = t
            ends[s >> 1] = t + 1
    return starts, ends


def viterbi_one(y_b, labels_b, tn, ln, eps=EPSILON):
    """One sample: dict(score, path (list of classes, Tn long), states, starts, ends), or score -inf and path None when no path
    fits.  Tn = 0: score 0 for an empty labelling (the empty path), infeasible otherwise."""
    y_b = np.asarray(y_b)
    T, C = y_b.shape
    tn, ln = clamp_lengths(T, len(labels_b), tn, ln)
    blank = C - 1
    raw = [int(v) for v in labels_b[:ln]]
    S = 2 * ln + 1
    cls = np.full(S, blank, dtype=np.int64)
    cls[1::2] = np.clip(raw, 0, C - 1) if ln else []
    skip = np.zeros(S, dtype=bool)
    for s in range(3, S, 2):
        skip[s] = raw[s >> 1] != raw[(s >> 1) - 1]
    none = dict(score=-np.inf, path=None, states=None, starts=None, ends=None)
    if tn == 0:
        return dict(score=0.0, path=[], states=[], starts=[], ends=[]) if ln == 0 else none
    lp = log_probs(y_b[:tn], eps)
    v = np.full(S, -np.inf)
    v[:2] = lp[0, cls[:2]]
    back = np.zeros((tn, S), dtype=np.int8)
    for t in range(1, tn):
        a1 = np.concatenate(([-np.inf], v[:-1]))
        a2 = np.where(skip, np.concatenate(([-np.inf, -np.inf], v[:-2])), -np.inf) if S > 2 else np.full(S, -np.inf)
        best, bk = v.copy(), np.zeros(S, dtype=np.int8)
        m = a1 > best                       # strict: stay wins a tie, and -inf never wins
        best[m], bk[m] = a1[m], 1
        m = a2 > best
        best[m], bk[m] = a2[m], 2
        v = best + lp[t, cls]
        back[t] = bk
    s = S - 1
    if S >= 2 and v[S - 2] > v[S - 1]:
        s = S - 2
    if v[s] == -np.inf:
        return none
    score = float(v[s])
    states = [0] * tn
    states[tn - 1] = s
    for t in range(tn - 1, 0, -1):
        s -= int(back[t, s])
        states[t - 1] = s
    starts, ends = segments(states, ln)
    return dict(score=score, path=[int(cls[s]) for s in states], states=states, starts=starts, ends=ends)


def viterbi(y_pred, labels, input_length, label_length, eps=EPSILON):
    y = np.asarray(y_pred)
    lab = np.asarray(labels).reshape(y.shape[0], -1)
    il, ll = np.asarray(input_length).reshape(-1), np.asarray(label_length).reshape(-1)
    return [viterbi_one(y[b], lab[b], il[b], ll[b], eps) for b in range(y.shape[0])]


def enumerate_paths(y_b, labels_b, tn, ln, eps=EPSILON):
    """(best score, best path, second-best score) over ALL C^Tn class paths that collapse to the labels; -inf / None where fewer than
    one / two exist.  Tiny cases only."""
    y_b = np.asarray(y_b)
    T, C = y_b.shape
    tn, ln = clamp_lengths(T, len(labels_b), tn, ln)
    assert C ** tn <= 1 << 16, 'enumeration is for tiny cases only'
    target = tuple(int(v) for v in labels_b[:ln])
    lp = log_probs(y_b[:tn], eps) if tn else np.zeros((0, C))
    best, best_path, second = -np.inf, None, -np.inf
    for path in itertools.product(range(C), repeat=tn):
        if collapse(path, C - 1) != target:
            continue
        sc = path_score(lp, path)
        if sc > best:
            best, best_path, second = sc, list(path), best
        elif sc > second:
            second = sc
    return best, best_path, second


def runs(path, blank):
    """[(class, start, end)] of the maximal non-blank runs of a class path."""
    out, t = [], 0
    while t < len(path):
        u = t
        while u < len(path) and path[u] == path[t]:
            u += 1
        if path[t] != blank:
            out.append((int(path[t]), t, u))
        t = u
    return out


def planted_path(rng, labels_b, T, blank):
    """A random valid alignment of the labels to T frames (a class per frame): a blank between equal neighbours, every other blank
    present with probability one half, the remaining frames spread at random over the tokens."""
    tokens = []
    for i, c in enumerate(labels_b):
        if (i == 0 and rng.rand() < 0.5) or (i > 0 and (labels_b[i - 1] == c or rng.rand() < 0.5)):
            tokens.append(blank)
        tokens.append(int(c))
    if not tokens or rng.rand() < 0.5:
        tokens.append(blank)
    assert len(tokens) <= T
    dur = np.ones(len(tokens), dtype=np.int64) + rng.multinomial(T - len(tokens), np.ones(len(tokens)) / len(tokens))
    return [c for c, d in zip(tokens, dur) for _ in range(d)]


def planted_posteriors(paths, T, C, peak=0.9):
    """y (B, T, C): `peak` on each path's class, the rest spread evenly; frames behind a path are uniform."""
    y = np.full((len(paths), T, C), 1.0 / C)
    for b, path in enumerate(paths):
        y[b, :len(path)] = (1.0 - peak) / (C - 1)
        y[b, np.arange(len(path)), path] = peak
    return y
