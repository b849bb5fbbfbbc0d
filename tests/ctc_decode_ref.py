"""TEST INFRASTRUCTURE -- float64 restatement of the CTC decoders and the edit distance (include/qk.h, "CTC decoding").

K.ctc_decode (Keras 2.x) is tf.nn.ctc_greedy_decoder(merge_repeated=True) for greedy=True and tf.nn.ctc_beam_search_decoder without a
language model for greedy=False.  The per-frame log-probabilities are the ones K.ctc_batch_cost trains with (oracle/ctc_enum.frame_probs):
u = log(y_pred + 1e-7), lp = u - logsumexp(u); blank = C - 1; only the first min(max(input_length, 0), T) frames count.

The beam search is written from the definition (prefix beam search over pb / pnb, merge of an extension into an existing beam, keep the
beam_width best by total with the tie rule: stay before extension, then lower source rank, then lower class) and reports its smallest
selection margin, so that a test can tell a decision an fp32 kernel must reproduce from one it may legitimately take the other way.
Only tests/ import this.
"""
import math

import numpy as np

from oracle import ctc_enum

EPSILON = ctc_enum.EPSILON


def _lse(a, b):
    m = max(a, b)
    if m == -math.inf:
        return -math.inf
    return m + math.log1p(math.exp(min(a, b) - m))


def frame_logprobs(y_b):
    """lp[t][c] = log softmax(log(y + eps)) in float64 (the probabilities of oracle.ctc_enum.frame_probs)."""
    u = np.log(np.asarray(y_b, dtype=np.float64) + EPSILON)
    m = u.max(axis=-1, keepdims=True)
    return u - (m + np.log(np.exp(u - m).sum(axis=-1, keepdims=True)))


def _frames(input_length, b, T):
    il = np.asarray(input_length).reshape(-1)
    return min(max(int(il[b]), 0), T)


def greedy_decode(y_pred, input_length):
    """tf.nn.ctc_greedy_decoder(merge_repeated=True): list of label tuples, log_prob (B,) = -sum_t max_c log(y[t][c] + eps).
    The argmax is taken over y itself (log(y + eps) is strictly increasing: the same class), the lowest index on ties."""
    y = np.asarray(y_pred, dtype=np.float64)
    B, T, C = y.shape
    out, lp = [], np.zeros(B)
    for b in range(B):
        tn = _frames(input_length, b, T)
        best = [int(np.argmax(y[b, t])) for t in range(tn)]          # np.argmax: first occurrence of the maximum
        out.append(ctc_enum.collapse(best, C - 1))
        lp[b] = -sum(math.log(y[b, t, k] + EPSILON) for t, k in enumerate(best))
    return out, lp


def collapse_repeats(seq):
    out = []
    for v in seq:
        if not out or out[-1] != v:
            out.append(v)
    return tuple(out)


def beam_search_one(y_b, tn, beam_width, top_paths, merge_repeated=True):
    """Prefix beam search of one utterance.  Returns (paths, log_probs, margin): up to top_paths label tuples in descending order of
    their total log-probability (normalised: log p(prefix | y)), their totals (padded with -inf up to top_paths; the paths with ()),
    and the smallest selection margin: over all frames, the gap between the beam_width-th candidate and the best candidate scoring
    strictly below it, and the gaps between consecutive returned paths (inf when nothing was ever cut).  Candidates with EXACTLY the
    score of the beam_width-th one are split by the tie rule; with continuous inputs such ties are structural (the extensions of one
    beam by classes of equal posterior, e.g. exact zeros), and an fp32 kernel sees the same ties."""
    lp = frame_logprobs(y_b)
    C = lp.shape[1]
    blank = C - 1
    NEG = -math.inf
    beams = [((), 0.0, NEG)]                            # (prefix, pb, pnb) in rank order
    margin = math.inf
    cls = np.arange(C - 1)
    for t in range(tn):
        lpt = lp[t]
        nb = len(beams)
        index = {pre: k for k, (pre, _, _) in enumerate(beams)}
        pb = np.array([e[1] for e in beams])
        pnb = np.array([e[2] for e in beams])
        totals = np.logaddexp(pb, pnb)
        last = np.array([e[0][-1] if e[0] else -1 for e in beams])
        stay_pb = totals + lpt[blank]
        stay_pnb = np.where(last >= 0, pnb + lpt[np.maximum(last, 0)], NEG)
        merged = np.zeros((nb, C - 1), dtype=bool)
        for m, (pre, _, _) in enumerate(beams):
            if not pre:
                continue
            k = index.get(pre[:-1])
            if k is None:
                continue
            c = pre[-1]
            ext = (pb[k] if last[k] == c else totals[k]) + lpt[c]
            stay_pnb[m] = np.logaddexp(stay_pnb[m], ext)
            merged[k, c] = True
        stay_tot = np.logaddexp(stay_pb, stay_pnb)
        ext = np.where(cls[None, :] == last[:, None], pb[:, None], totals[:, None]) + lpt[None, :C - 1]
        ok = ~merged & (ext > NEG)
        kk, cc = np.nonzero(ok)
        score = np.concatenate([stay_tot, ext[kk, cc]])
        kind = np.concatenate([np.zeros(nb, dtype=np.int64), np.ones(kk.size, dtype=np.int64)])
        src = np.concatenate([np.arange(nb), kk])
        cl = np.concatenate([np.zeros(nb, dtype=np.int64), cc])
        valid = score > NEG
        score, kind, src, cl = score[valid], kind[valid], src[valid], cl[valid]
        order = np.lexsort((cl, src, kind, -score))
        if order.size > beam_width:
            sw = score[order[beam_width - 1]]
            below = score[order[beam_width:]]
            below = below[below < sw]
            if below.size:
                margin = min(margin, float(sw - below.max()))
        nbeams = []
        for i in order[:beam_width]:
            k = int(src[i])
            if kind[i] == 0:
                nbeams.append((beams[k][0], float(stay_pb[k]), float(stay_pnb[k])))
            else:
                nbeams.append((beams[k][0] + (int(cl[i]),), NEG, float(score[i])))
        beams = nbeams
    totals = [float(np.logaddexp(pb, pnb)) for _, pb, pnb in beams]
    paths, lps = [], []
    for p in range(top_paths):
        if p < len(beams):
            pre = beams[p][0]
            paths.append(collapse_repeats(pre) if merge_repeated else pre)
            lps.append(totals[p])
        else:
            paths.append(())
            lps.append(-math.inf)
    for p in range(min(top_paths, len(beams)) - 1):
        margin = min(margin, lps[p] - lps[p + 1])
    return paths, np.array(lps), margin


def beam_search_decode(y_pred, input_length, beam_width=100, top_paths=1, merge_repeated=True):
    """beam_search_one over a batch: (paths[b][k], log_prob (B, top_paths), margin (B,))."""
    y = np.asarray(y_pred, dtype=np.float64)
    B, T, C = y.shape
    paths, lps, margins = [], np.zeros((B, top_paths)), np.zeros(B)
    for b in range(B):
        p, l, m = beam_search_one(y[b], _frames(input_length, b, T), beam_width, top_paths, merge_repeated)
        paths.append(p)
        lps[b] = l
        margins[b] = m
    return paths, lps, margins


def top_labelings_enum(y_b, tn):
    """Every labelling with its log-probability, by enumerating all C^tn frame paths (oracle.ctc_enum's definition), most probable first
    (ties: the shorter, then lexicographically smaller labelling)."""
    import itertools
    p = ctc_enum.frame_probs(np.asarray(y_b, dtype=np.float64)[:tn])
    C = np.asarray(y_b).shape[-1]
    acc = {}
    for path in itertools.product(range(C), repeat=tn):
        pr = 1.0
        for t, c in enumerate(path):
            pr *= p[t, c]
        lab = ctc_enum.collapse(path, C - 1)
        acc[lab] = acc.get(lab, 0.0) + pr
    items = sorted(acc.items(), key=lambda kv: (-kv[1], len(kv[0]), kv[0]))
    return [(lab, math.log(pr)) for lab, pr in items]


def edit_distance(a, b):
    """Levenshtein distance with unit costs (tf.edit_distance, normalize=False)."""
    a, b = list(a), list(b)
    prev = list(range(len(b) + 1))
    for i, x in enumerate(a, 1):
        cur = [i] + [0] * len(b)
        for j, y in enumerate(b, 1):
            cur[j] = min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (x != y))
        prev = cur
    return prev[-1]


def apply_class_map(seq, class_map):
    if class_map is None:
        return list(seq)
    cm = list(class_map)
    out = []
    for t in seq:
        if 0 <= t < len(cm):
            if cm[t] >= 0:
                out.append(cm[t])
        else:
            out.append(t)
    return out
