"""TEST INFRASTRUCTURE -- float64 restatement of the CTC prefix beam search fused with a phone n-gram LM (include/qk.h, "CTC decoding").

A prefix l is ranked by S(l) = log p_ctc(l | y) + alpha log P_LM(l) + beta |l| (+ alpha log P_LM(</s> | l) at the last frame with eos);
the pb / pnb recursions and the merge are those of ctc_decode_ref.beam_search_one.  The LM is a dense natural-log table
(C^(order - 1), C) with V = C - 1 = <s> in a context and </s> as the event (qcnn_amd.lm.NgramLM.logp).  Only tests/ import this.
"""
import math

import numpy as np

import ctc_decode_ref as R


def ctx_index(prefix, order, C):
    V = C - 1
    if order == 1:
        return 0
    last = prefix[-1] if len(prefix) >= 1 else V
    if order == 2:
        return last
    last2 = prefix[-2] if len(prefix) >= 2 else V
    return last2 * C + last


def lm_logprob(prefix, table, order, eos):
    """log P_LM(prefix) (+ log P(</s> | prefix) with eos) from the dense table, in float64."""
    table = np.asarray(table, dtype=np.float64)
    C = table.shape[1]
    tot = 0.0
    for i, w in enumerate(prefix):
        tot += table[ctx_index(prefix[:i], order, C), w]
    if eos:
        tot += table[ctx_index(prefix, order, C), C - 1]
    return tot


def fused(prefix, ctc_lp, table, order, alpha, beta, eos):
    """S(prefix) given log p_ctc(prefix | y); alpha = 0 never reads the table."""
    lmv = alpha * lm_logprob(prefix, table, order, eos) if alpha != 0 else 0.0
    return ctc_lp + lmv + beta * len(prefix)


def beam_search_lm_one(y_b, tn, beam_width, top_paths, table, order, alpha, beta, eos=True, merge_repeated=True):
    """Prefix beam search of one utterance ranked by S.  Returns (paths, log_probs, scores, margin): up to top_paths label tuples in
    descending order of their final S, their acoustic totals log p(prefix | y), their S (both padded with -inf, the paths with ()),
    and the smallest selection margin in S (as in ctc_decode_ref.beam_search_one, plus the gaps between the returned paths)."""
    table = np.asarray(table, dtype=np.float64)
    lp = R.frame_logprobs(y_b)
    C = lp.shape[1]
    blank = C - 1
    NEG = -math.inf
    use = alpha != 0

    def lm_row(pre):
        return table[ctx_index(pre, order, C)] if use else np.zeros(C)

    beams = [((), 0.0, NEG, 0.0)]                       # (prefix, pb, pnb, F = alpha log P_LM + beta |prefix|), in rank order
    margin = math.inf
    cls = np.arange(C - 1)
    for t in range(tn):
        lpt = lp[t]
        nb = len(beams)
        index = {b[0]: k for k, b in enumerate(beams)}
        pb = np.array([e[1] for e in beams])
        pnb = np.array([e[2] for e in beams])
        F = np.array([e[3] for e in beams])
        totals = np.logaddexp(pb, pnb)
        last = np.array([e[0][-1] if e[0] else -1 for e in beams])
        stay_pb = totals + lpt[blank]
        stay_pnb = np.where(last >= 0, pnb + lpt[np.maximum(last, 0)], NEG)
        merged = np.zeros((nb, C - 1), dtype=bool)
        for m, (pre, _, _, _) in enumerate(beams):
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
        rows = np.stack([lm_row(b[0])[:C - 1] for b in beams])
        with np.errstate(invalid='ignore'):
            ext_F = F[:, None] + alpha * rows + beta if use else F[:, None] + beta + np.zeros_like(ext)
        ext_S = ext + ext_F
        ok = ~merged & (ext_S > NEG)
        kk, cc = np.nonzero(ok)
        ac = np.concatenate([stay_tot, ext[kk, cc]])
        score = np.concatenate([stay_tot + F, ext_S[kk, cc]])
        newF = np.concatenate([F, ext_F[kk, cc]])
        kind = np.concatenate([np.zeros(nb, dtype=np.int64), np.ones(kk.size, dtype=np.int64)])
        src = np.concatenate([np.arange(nb), kk])
        cl = np.concatenate([np.zeros(nb, dtype=np.int64), cc])
        valid = score > NEG
        ac, score, newF, kind, src, cl = ac[valid], score[valid], newF[valid], kind[valid], src[valid], cl[valid]
        order_ = np.lexsort((cl, src, kind, -score))
        if order_.size > beam_width:
            sw = score[order_[beam_width - 1]]
            below = score[order_[beam_width:]]
            below = below[below < sw]
            if below.size:
                margin = min(margin, float(sw - below.max()))
        nbeams = []
        for i in order_[:beam_width]:
            k = int(src[i])
            if kind[i] == 0:
                nbeams.append((beams[k][0], float(stay_pb[k]), float(stay_pnb[k]), float(newF[i])))
            else:
                nbeams.append((beams[k][0] + (int(cl[i]),), NEG, float(ac[i]), float(newF[i])))
        beams = nbeams
    totals = [float(np.logaddexp(b[1], b[2])) for b in beams]
    fin = []
    for (pre, _, _, f), tot in zip(beams, totals):
        e = alpha * table[ctx_index(pre, order, C), C - 1] if (eos and use) else 0.0
        fin.append(tot + f + e)
    rank = sorted(range(len(beams)), key=lambda i: (-fin[i], i))
    paths, lps, scs = [], [], []
    for p in range(top_paths):
        if p < len(beams):
            i = rank[p]
            pre = beams[i][0]
            paths.append(R.collapse_repeats(pre) if merge_repeated else pre)
            lps.append(totals[i])
            scs.append(fin[i])
        else:
            paths.append(())
            lps.append(-math.inf)
            scs.append(-math.inf)
    for p in range(min(top_paths, len(beams)) - 1):
        margin = min(margin, scs[p] - scs[p + 1])
    if eos and use and len(beams) > 1:                  # the re-rank is a selection too
        s = sorted(fin, reverse=True)
        margin = min(margin, s[0] - s[1])
    return paths, np.array(lps), np.array(scs), margin


def beam_search_lm_decode(y_pred, input_length, beam_width, top_paths, table, order, alpha, beta, eos=True, merge_repeated=True):
    """beam_search_lm_one over a batch: (paths[b][k], log_prob (B, top_paths), score (B, top_paths), margin (B,))."""
    y = np.asarray(y_pred, dtype=np.float64)
    B, T, _ = y.shape
    il = np.asarray(input_length).reshape(-1)
    paths, lps, scs, margins = [], np.zeros((B, top_paths)), np.zeros((B, top_paths)), np.zeros(B)
    for b in range(B):
        tn = min(max(int(il[b]), 0), T)
        p, l, s, m = beam_search_lm_one(y[b], tn, beam_width, top_paths, table, order, alpha, beta, eos, merge_repeated)
        paths.append(p)
        lps[b], scs[b], margins[b] = l, s, m
    return paths, lps, scs, margins


def best_by_enumeration(y_b, tn, table, order, alpha, beta, eos):
    """Every labelling of ctc_decode_ref.top_labelings_enum with its S, best first (ties: shorter, then lexicographically smaller)."""
    items = [(lab, ctc_lp, fused(lab, ctc_lp, table, order, alpha, beta, eos)) for lab, ctc_lp in R.top_labelings_enum(y_b, tn)]
    items.sort(key=lambda e: (-e[2], len(e[0]), e[0]))
    return items
