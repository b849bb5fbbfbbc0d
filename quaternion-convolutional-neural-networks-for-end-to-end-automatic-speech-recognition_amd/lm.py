"""Phone n-gram language models for CTC beam search decoding (functional.ctc_beam_search_decode_lm, include/qk.h "CTC decoding").

NgramLM holds a dense table of natural-log probabilities, shape (C^(order - 1), C) with C = num_labels + 1 (the CTC class count; the
blank's index V = C - 1 is reused): in a context, index V means <s>; in the event column, index V means </s>.  The bigram context is the
last label (V for the empty prefix), the trigram context last2 * C + last (V where missing); order 1 has a single row.

Estimation (interpolated Kneser-Ney) and ARPA I/O run on the host in numpy; the estimator is not a hot path.  Each sentence is padded
as `<s> w_1 .. w_n </s>` with ONE <s>, as ARPA tools do, so a trigram row whose context begins at <s> (last2 = V) is the bigram
distribution after <s>, reached through back-off.
"""
import math

import numpy as np
import torch

LN10 = math.log(10.0)
ARPA_LOG_ZERO = -99.0          # log10 of 0 as ARPA files write it


def _ctx_index(prefix, order, V, C):
    if order == 1:
        return 0
    last = prefix[-1] if len(prefix) >= 1 else V
    if order == 2:
        return last
    last2 = prefix[-2] if len(prefix) >= 2 else V
    return last2 * C + last


class NgramLM(object):
    """A phone n-gram LM of order 1 to 3 over num_labels labels (the CTC classes without the blank).

    logp: (C^(order - 1), C) natural-log probabilities (finite or -inf), C = num_labels + 1.  Build one with estimate() or from_arpa()."""

    def __init__(self, logp, num_labels, order, levels=None, discounts=None):
        order, num_labels = int(order), int(num_labels)
        if not 1 <= order <= 3:
            raise ValueError('NgramLM: order %d outside 1 .. 3' % order)
        if num_labels < 1:
            raise ValueError('NgramLM: num_labels must be >= 1')
        C = num_labels + 1
        logp = np.asarray(logp, dtype=np.float64)
        if logp.shape != (C ** (order - 1), C):
            raise ValueError('NgramLM: table shape %s, expected %s' % (logp.shape, (C ** (order - 1), C)))
        if np.isnan(logp).any() or (logp == np.inf).any():
            raise ValueError('NgramLM: table entries must be finite or -inf')
        self.logp, self.num_labels, self.order = logp, num_labels, order
        self.discounts = discounts
        self._levels = levels            # per order n: (listed (C,)*n bool, log P_n (C,)*n, log back-off (C,)*n or None)
        self._tables = {}

    @property
    def classes(self):
        return self.num_labels + 1

    # ---- estimation -----------------------------------------------------------------------------------------------------------
    @classmethod
    def estimate(cls, sequences, num_labels, order, discount=None):
        """Interpolated Kneser-Ney from label sequences (each an iterable of ints in [0, num_labels)).

        Counts a_n of the n-grams of order n: raw counts at the highest order and for n-grams that begin with <s>, otherwise
        continuation counts N1+(. g) (the number of distinct symbols, <s> included, seen before g).  With A(h) = sum_w a_n(h, w) and
        N1(h) = #{w: a_n(h, w) > 0}:
            P_n(w | h) = max(a_n(h, w) - D_n, 0) / A(h) + D_n N1(h) / A(h) P_{n-1}(w | h[1:])   if A(h) > 0, else P_{n-1}(w | h[1:]),
        P_0 = 1 / (num_labels + 1), uniform over the labels and </s>; <s> is never an event.  discount: None (Ney's
        D_n = n1 / (n1 + 2 n2) from the counts of a_n equal to 1 and 2; 0.5 where no n-gram of that order has a_n = 1), one number for
        every order, or one per order; each in [0, 1]."""
        order, V = int(order), int(num_labels)
        if not 1 <= order <= 3:
            raise ValueError('NgramLM.estimate: order %d outside 1 .. 3' % order)
        C = V + 1
        if discount is None:
            disc = [None] * order
        elif np.ndim(discount) == 0:
            disc = [float(discount)] * order
        else:
            disc = [float(d) for d in discount]
            if len(disc) != order:
                raise ValueError('NgramLM.estimate: %d discounts for order %d' % (len(disc), order))
        for d in disc:
            if d is not None and not 0.0 <= d <= 1.0:
                raise ValueError('NgramLM.estimate: discounts must lie in [0, 1], got %r' % (d,))
        # raw counts of every order; index V is <s> in a history slot and </s> in the event slot
        windows = [[] for _ in range(order + 1)]
        for seq in sequences:
            s = np.asarray(list(seq), dtype=np.int64).reshape(-1)
            if s.size and (s.min() < 0 or s.max() >= V):
                raise ValueError('NgramLM.estimate: labels must lie in [0, %d)' % V)
            pad = np.concatenate([[V], s, [V]])
            for n in range(1, order + 1):
                if pad.size < n:
                    continue
                w = np.lib.stride_tricks.sliding_window_view(pad, n)
                if n == 1:
                    w = w[1:]                            # <s> is not an event
                windows[n].append(np.ravel_multi_index(tuple(w.T), (C,) * n))
        raw = [None]
        for n in range(1, order + 1):
            idx = np.concatenate(windows[n]) if windows[n] else np.zeros(0, dtype=np.int64)
            raw.append(np.bincount(idx, minlength=C ** n).astype(np.float64).reshape((C,) * n))
        probs, discounts, counts = [None], [], [None]
        lower = np.full((C,), 1.0 / C)
        for n in range(1, order + 1):
            if n == order:
                a = raw[n]
            else:
                a = (raw[n + 1] > 0).sum(axis=0).astype(np.float64)
                if n >= 2:
                    a[V] = raw[n][V]                     # n-grams that begin with <s>: raw counts
            d = disc[n - 1]
            if d is None:
                n1, n2 = float((a == 1).sum()), float((a == 2).sum())
                d = n1 / (n1 + 2.0 * n2) if n1 > 0 else 0.5
            A = a.sum(axis=-1, keepdims=True)
            N1 = (a > 0).sum(axis=-1, keepdims=True)
            low = lower if n == 1 else np.broadcast_to(lower[None], (C,) * n)
            with np.errstate(divide='ignore', invalid='ignore'):
                p = np.where(A > 0, np.maximum(a - d, 0.0) / A + d * N1 / A * low, low)
            probs.append(p)
            counts.append(a)
            discounts.append(d)
            lower = p
        # ARPA view: listed n-grams, their log P and the back-off weight of each history (gamma of the order above)
        levels = []
        with np.errstate(divide='ignore'):
            for n in range(1, order + 1):
                listed = np.ones((C,), dtype=bool) if n == 1 else counts[n] > 0
                bow = None
                if n < order:
                    a = counts[n + 1]
                    A = a.sum(axis=-1)
                    N1 = (a > 0).sum(axis=-1)
                    gamma = np.where(A > 0, discounts[n] * N1 / np.where(A > 0, A, 1.0), 1.0)
                    bow = np.log(gamma)
                levels.append((listed, np.log(probs[n]), bow))
            table = np.log(probs[order]).reshape(C ** (order - 1), C)
        return cls(table, V, order, levels=levels, discounts=discounts)

    # ---- ARPA -----------------------------------------------------------------------------------------------------------------
    @classmethod
    def from_arpa(cls, path, symbols):
        """Read an ARPA back-off LM.  symbols: the label names, label i = symbols[i] (TIMIT: data.TIMIT_PHONES_61).  Values are log10
        on disk and natural log here (<= -99 reads as -inf).  An n-gram that is not listed is bow(h) + log P(w | h[1:]), with a back-off
        of 0 for a context that is not listed.  <unk> entries are ignored; any other symbol outside symbols, <s> and </s> raises
        ValueError.  <s> is a context only (its unigram probability is ignored); n-grams with </s> in the context are skipped."""
        sym = {s: i for i, s in enumerate(symbols)}
        if len(sym) != len(symbols) or '<s>' in sym or '</s>' in sym:
            raise ValueError('NgramLM.from_arpa: symbols must be distinct and exclude <s> / </s>')
        V = len(symbols)
        C = V + 1
        entries = {}
        order = 0
        section = None
        with open(path) as f:
            for raw_line in f:
                line = raw_line.strip()
                if not line:
                    continue
                if line == '\\data\\':
                    section = 'data'
                    continue
                if line == '\\end\\':
                    break
                if line.startswith('\\') and line.endswith('-grams:'):
                    section = int(line[1:line.index('-')])
                    order = max(order, section)
                    entries.setdefault(section, [])
                    continue
                if section == 'data':
                    if line.startswith('ngram'):
                        n, cnt = line[5:].split('=')
                        if int(cnt) > 0:
                            order = max(order, int(n))
                    continue
                if not isinstance(section, int):
                    continue
                fields = line.split()
                n = section
                if len(fields) not in (n + 1, n + 2):
                    raise ValueError('NgramLM.from_arpa: malformed %d-gram line %r' % (n, line))
                toks = fields[1:n + 1]
                if '<unk>' in toks:
                    continue
                for t in toks:
                    if t not in sym and t not in ('<s>', '</s>'):
                        raise ValueError('NgramLM.from_arpa: symbol %r is not in the label set' % t)
                entries[n].append((float(fields[0]), toks, float(fields[n + 1]) if len(fields) == n + 2 else None))
        if not 1 <= order <= 3:
            raise ValueError('NgramLM.from_arpa: order %d outside 1 .. 3' % order)

        def val(x):
            return -math.inf if x <= ARPA_LOG_ZERO else x * LN10

        def hist_idx(toks):
            """history-slot indices, or None when the tokens cannot form a context (</s>, or <s> after the first slot)"""
            out = []
            for k, t in enumerate(toks):
                if t == '</s>' or (t == '<s>' and k > 0):
                    return None
                out.append(V if t == '<s>' else sym[t])
            return tuple(out)

        levels = []
        lower = None
        for n in range(1, order + 1):
            listed = np.zeros((C,) * n, dtype=bool)
            bow = np.zeros((C,) * n) if n < order else None
            lp = np.full((C,) * n, -math.inf)
            if n >= 2:
                lp = np.broadcast_to(lower[None], (C,) * n).copy() + levels[-1][2][..., None]
            for lp10, toks, b10 in entries.get(n, []):
                h = hist_idx(toks[:-1])
                if h is None:
                    continue
                ev = toks[-1]
                if b10 is not None and bow is not None and ev != '</s>':
                    hb = hist_idx(toks)
                    if hb is not None:
                        bow[hb] = val(b10)
                if ev == '<s>':
                    continue
                idx = h + (V if ev == '</s>' else sym[ev],)
                lp[idx] = val(lp10)
                listed[idx] = True
            levels.append((listed, lp, bow))
            lower = lp
        table = lower.reshape(C ** (order - 1), C)
        return cls(table, V, order, levels=levels)

    def to_arpa(self, path, symbols):
        """Write the LM as ARPA text (log10 values, 7 decimals).  Needs the n-gram levels of estimate() or from_arpa()."""
        if self._levels is None:
            raise ValueError('NgramLM.to_arpa: this LM carries no n-gram levels (built from a bare table)')
        V = self.num_labels
        if len(symbols) != V:
            raise ValueError('NgramLM.to_arpa: %d symbols for %d labels' % (len(symbols), V))
        names = list(symbols)

        def ev_name(i):
            return '</s>' if i == V else names[i]

        def h_name(i):
            return '<s>' if i == V else names[i]

        def fmt(x):
            return '%.7f' % (ARPA_LOG_ZERO if x == -math.inf else x / LN10)

        blocks = []
        for n, (listed, lp, bow) in enumerate(self._levels, 1):
            lines = []
            if n == 1 and self.order >= 2:
                lines.append('%s\t<s>\t%s' % (fmt(-math.inf), fmt(bow[V])))
            elif n == 1:
                lines.append('%s\t<s>' % fmt(-math.inf))
            for idx in zip(*np.nonzero(listed)):
                idx = tuple(int(i) for i in idx)
                if any(i == V for i in idx[1:-1]):           # <s> only opens a context
                    continue
                toks = [h_name(i) for i in idx[:-1]] + [ev_name(idx[-1])]
                line = '%s\t%s' % (fmt(lp[idx]), ' '.join(toks))
                if bow is not None and idx[-1] != V:
                    line += '\t' + fmt(bow[idx])
                lines.append(line)
            blocks.append(lines)
        with open(path, 'w') as f:
            f.write('\\data\\\n')
            for n, lines in enumerate(blocks, 1):
                f.write('ngram %d=%d\n' % (n, len(lines)))
            for n, lines in enumerate(blocks, 1):
                f.write('\n\\%d-grams:\n' % n)
                f.write('\n'.join(lines) + '\n')
            f.write('\n\\end\\\n')

    # ---- scoring --------------------------------------------------------------------------------------------------------------
    def log_prob(self, seq, eos=True):
        """Natural-log P_LM(seq) (times P(</s> | seq) when eos) from the dense table."""
        V, C = self.num_labels, self.classes
        seq = [int(v) for v in seq]
        total = 0.0
        for i, w in enumerate(seq):
            if not 0 <= w < V:
                raise ValueError('NgramLM.log_prob: label %d outside [0, %d)' % (w, V))
            total += self.logp[_ctx_index(seq[:i], self.order, V, C), w]
        if eos:
            total += self.logp[_ctx_index(seq, self.order, V, C), V]
        return total

    def perplexity(self, seqs):
        """exp(-sum log P_LM(seq </s>) / number of events), the events being every label and one </s> per sequence."""
        lp, n = 0.0, 0
        for s in seqs:
            s = list(s)
            lp += self.log_prob(s, eos=True)
            n += len(s) + 1
        return math.exp(-lp / max(n, 1))

    def table(self, device):
        """The dense (C^(order - 1), C) float32 table on `device`, built once per device."""
        key = str(torch.device(device))
        t = self._tables.get(key)
        if t is None:
            t = torch.tensor(self.logp, dtype=torch.float32).to(device).contiguous()
            self._tables[key] = t
        return t
