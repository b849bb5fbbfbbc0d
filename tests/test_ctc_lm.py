"""Phone n-gram LM fused into the CTC beam search (qcnn_amd.lm.NgramLM, functional.ctc_beam_search_decode_lm,
qk_ctc_beam_search_decode_lm; include/qk.h, "CTC decoding") against the float64 restatement in tests/ctc_lm_ref.py.

CPU: the interpolated Kneser-Ney estimator (normalisation, hand-computed values, ARPA round trip, back-off of a hand-written ARPA file),
the reference against the definition S = log p_ctc + alpha log P_LM + beta |l| over every labelling, and the refusals of the API.
GPU: the kernel on the exhaustive cases, bit-identity with the plain beam search at alpha = beta = 0, the benchmark shape with a
bigram and a trigram LM, a case where the LM changes the answer, the staged-row layout at C = 200, and the model-level wiring.
"""
import math

import numpy as np
import pytest
import torch

import ctc_decode_ref as R
import ctc_lm_ref as LR
from qcnn_amd import _lib, functional as Fq, layers
from qcnn_amd.lm import NgramLM


def _soft(rng, *shape, scale=1.5):
    z = rng.randn(*shape) * scale
    e = np.exp(z - z.max(-1, keepdims=True))
    return e / e.sum(-1, keepdims=True)


def _random_table(rng, C, order, scale=1.5):
    z = rng.randn(C ** (order - 1), C) * scale
    return z - np.log(np.exp(z).sum(-1, keepdims=True))


def _random_corpus(rng, V, n=200, lo=3, hi=20):
    """Label sequences with some structure: a random first-order chain, so that the bigram and trigram statistics differ."""
    trans = rng.dirichlet(np.full(V, 0.3), size=V)
    out = []
    for _ in range(n):
        L = rng.randint(lo, hi)
        s = [rng.randint(V)]
        for _ in range(L - 1):
            s.append(int(rng.choice(V, p=trans[s[-1]])))
        out.append(s)
    return out


# ---- CPU: the estimator ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('order', [1, 2, 3])
def test_estimated_distributions_sum_to_one(order):
    rng = np.random.RandomState(order)
    V = 7
    lm = NgramLM.estimate(_random_corpus(rng, V, n=60), V, order)
    assert lm.logp.shape == ((V + 1) ** (order - 1), V + 1)
    assert np.abs(np.exp(lm.logp).sum(axis=1) - 1.0).max() < 1e-9
    assert len(lm.discounts) == order and all(0.0 <= d <= 1.0 for d in lm.discounts)
    lm2 = NgramLM.estimate(_random_corpus(rng, V, n=60), V, order, discount=0.7)
    assert np.abs(np.exp(lm2.logp).sum(axis=1) - 1.0).max() < 1e-9


def test_estimator_reproduces_hand_computed_kneser_ney():
    a, b, c = 0, 1, 2
    V = 3                                   # index 3: <s> as a context, </s> as the event
    corpus = [[a, b], [a, c], [b]]
    # bigram, D = 0.5 at both orders.  Bigram counts: <s>a 2, <s>b 1, ab 1, ac 1, b</s> 2, c</s> 1.  Unigram continuation counts:
    # a 1 ({<s>}), b 2 ({<s>, a}), c 1 ({a}), </s> 2 ({b, c}); total 6, 4 types: P1 = (a - .5) / 6 + .5 * 4 / 6 / 4
    lm = NgramLM.estimate(corpus, V, 2, discount=0.5)
    P = np.exp(lm.logp)
    p1 = {a: 1 / 6, b: 2 / 6, c: 1 / 6, V: 2 / 6}
    assert abs(P[V, a] - (1.5 / 3 + (0.5 * 2 / 3) * p1[a])) < 1e-12 and abs(P[V, a] - 5 / 9) < 1e-12
    assert abs(P[V, b] - 5 / 18) < 1e-12
    assert abs(P[V, c] - 1 / 18) < 1e-12                               # unseen after <s>: back-off mass only
    assert abs(P[a, b] - 5 / 12) < 1e-12                               # .5 / 2 + (.5 * 2 / 2) * 2 / 6
    assert abs(P[a, V] - 1 / 6) < 1e-12
    assert abs(P[c, V] - 2 / 3) < 1e-12                                # .5 / 1 + .5 * 1 / 1 * 2 / 6
    # unigram: raw counts a 2, b 2, c 1, </s> 3 (total 8, 4 types)
    lm1 = NgramLM.estimate(corpus, V, 1, discount=0.5)
    assert abs(math.exp(lm1.logp[0, V]) - 3 / 8) < 1e-12
    assert abs(math.exp(lm1.logp[0, c]) - (0.5 / 8 + 0.25 / 4)) < 1e-12
    # Ney's discount: bigram counts 2,1,1,1,2,1 -> n1 = 4, n2 = 2 -> 1/2; unigram continuation counts 1,2,1,2 -> 2 / 6
    assert np.allclose(NgramLM.estimate(corpus, V, 2).discounts, [1 / 3, 0.5])
    # log_prob and perplexity from the table
    want = math.log(P[V, a]) + math.log(P[a, b]) + math.log(P[b, V])
    assert abs(lm.log_prob([a, b]) - want) < 1e-12
    assert abs(lm.log_prob([a, b], eos=False) - (want - math.log(P[b, V]))) < 1e-12
    ppl = math.exp(-(lm.log_prob([a, b]) + lm.log_prob([b])) / 5)
    assert abs(lm.perplexity([[a, b], [b]]) - ppl) < 1e-9


@pytest.mark.parametrize('order', [1, 2, 3])
def test_arpa_round_trip(tmp_path, order):
    rng = np.random.RandomState(10 + order)
    V = 6
    symbols = ['p%d' % i for i in range(V)]
    lm = NgramLM.estimate(_random_corpus(rng, V, n=40), V, order)
    path = str(tmp_path / 'lm.arpa')
    lm.to_arpa(path, symbols)
    back = NgramLM.from_arpa(path, symbols)
    assert back.order == order and back.num_labels == V
    assert np.isfinite(back.logp).all()
    assert np.abs(back.logp - lm.logp).max() < 1e-5                   # 7 printed decimals of log10, a few terms per entry
    path2 = str(tmp_path / 'lm2.arpa')
    back.to_arpa(path2, symbols)
    assert np.abs(NgramLM.from_arpa(path2, symbols).logp - lm.logp).max() < 1e-5


_HAND_ARPA = """
\\data\\
ngram 1=6
ngram 2=3

\\1-grams:
-1.0\t<s>\t-0.3
-0.5\ta\t-0.2
-0.7\tb
-0.9\tc\t-0.1
-0.6\t</s>
-1.5\t<unk>

\\2-grams:
-0.1\t<s> a
-0.4\ta b
-0.3\tc </s>

\\end\\
"""


def test_hand_written_arpa_resolves_through_back_offs(tmp_path):
    path = tmp_path / 'hand.arpa'
    path.write_text(_HAND_ARPA)
    lm = NgramLM.from_arpa(str(path), ['a', 'b', 'c'])
    a, b, c, V = 0, 1, 2, 3
    want = {(V, a): -0.1, (V, b): -0.3 - 0.7, (V, c): -0.3 - 0.9, (V, V): -0.3 - 0.6,
            (a, a): -0.2 - 0.5, (a, b): -0.4, (a, c): -0.2 - 0.9, (a, V): -0.2 - 0.6,
            (b, a): -0.5, (b, b): -0.7, (b, c): -0.9, (b, V): -0.6,          # no back-off weight on b: 0
            (c, a): -0.1 - 0.5, (c, V): -0.3}
    for (h, w), v in want.items():
        assert abs(lm.logp[h, w] - v * math.log(10)) < 1e-12, (h, w)
    bad = tmp_path / 'bad.arpa'
    bad.write_text(_HAND_ARPA.replace('-0.4\ta b', '-0.4\ta zz'))
    with pytest.raises(ValueError, match='zz'):
        NgramLM.from_arpa(str(bad), ['a', 'b', 'c'])


# ---- CPU: the reference against the definition --------------------------------------------------------------------------------
def _exhaustive_cases():
    """(y (T, C), tn): C = 3 with T <= 6 and C = 4 with T <= 4 -- every prefix fits into 128 beams, so nothing is pruned."""
    rng = np.random.RandomState(21)
    return [(_soft(rng, T, C), T) for C, T in ((3, 6), (3, 4), (4, 4), (4, 3), (4, 1))]


_LM_SETTINGS = [(order, alpha, beta, eos) for order in (1, 2, 3) for alpha, beta in ((0.8, -0.6), (1.3, 0.0), (0.5, 0.9))
                for eos in (True, False)]


@pytest.mark.parametrize('order,alpha,beta,eos', _LM_SETTINGS)
def test_reference_lm_beam_search_without_pruning_equals_enumeration(order, alpha, beta, eos):
    rng = np.random.RandomState(order * 100 + int(alpha * 10))
    for y, tn in _exhaustive_cases():
        C = y.shape[1]
        table = _random_table(rng, C, order)
        want = LR.best_by_enumeration(y, tn, table, order, alpha, beta, eos)
        paths, lps, scs, _ = LR.beam_search_lm_one(y, tn, 128, 3, table, order, alpha, beta, eos, merge_repeated=False)
        for k in range(min(3, len(want))):
            assert abs(scs[k] - want[k][2]) < 1e-10, (k, scs[k], want[k])
            gap_hi = want[k - 1][2] - want[k][2] if k > 0 else 1.0
            gap_lo = want[k][2] - want[k + 1][2] if k + 1 < len(want) else 1.0
            if min(gap_hi, gap_lo) > 1e-9:
                assert paths[k] == want[k][0], (k, paths[k], want[k])
                assert abs(lps[k] - want[k][1]) < 1e-10


def test_reference_with_zero_weights_is_the_plain_beam_search():
    rng = np.random.RandomState(3)
    for y, tn in _exhaustive_cases() + [(_soft(rng, 30, 12, scale=3.0), 30)]:
        table = _random_table(rng, y.shape[1], 2)
        for W in (3, 128):
            p0, l0, m0 = R.beam_search_one(y, tn, W, 3, merge_repeated=True)
            p1, l1, s1, m1 = LR.beam_search_lm_one(y, tn, W, 3, table, 2, 0.0, 0.0, eos=True, merge_repeated=True)
            assert p0 == p1 and np.array_equal(l0, l1) and np.array_equal(l1, s1) and m0 == m1


# ---- CPU: refusals ------------------------------------------------------------------------------------------------------------
def test_lm_api_refuses_bad_arguments_without_a_gpu():
    rng = np.random.RandomState(0)
    y = torch.rand(2, 5, 4)
    il = torch.tensor([5, 5])
    lm = NgramLM.estimate(_random_corpus(rng, 3, n=10), 3, 2)
    with pytest.raises(RuntimeError, match='CPU'):
        Fq.ctc_beam_search_decode_lm(y, il, lm)
    with pytest.raises(ValueError, match='shape'):
        NgramLM(np.zeros((3, 4)), 3, 2)                                  # a bigram table over C = 4 is (4, 4)
    with pytest.raises(ValueError, match='labels'):
        Fq.ctc_beam_search_decode_lm(torch.rand(2, 5, 6), il, lm)       # 3 LM labels, 5 + blank classes
    lm3 = NgramLM(np.full((65 * 65, 65), -math.log(65)), 64, 3)
    with pytest.raises(ValueError, match='trigram'):
        Fq.ctc_beam_search_decode_lm(torch.rand(2, 5, 65), il, lm3)
    for bad in (-0.1, float('nan'), float('inf')):
        with pytest.raises(ValueError, match='lm_weight'):
            Fq.ctc_beam_search_decode_lm(y, il, lm, lm_weight=bad)
    with pytest.raises(ValueError, match='insertion_bonus'):
        Fq.ctc_beam_search_decode_lm(y, il, lm, insertion_bonus=float('inf'))
    with pytest.raises(ValueError, match='greedy'):
        layers.ctc_decode(y, il, greedy=True, lm=lm)
    from qcnn_amd.models.interspeech_model import TimitQCNN
    model = TimitQCNN(num_layers=2, start_filter=8)
    with pytest.raises(ValueError, match='greedy'):
        model.evaluate(None, None, None, None, greedy=True, lm=lm)
    with pytest.raises(ValueError, match='greedy'):
        model.decode(None, greedy=True, lm=lm)
    with pytest.raises(ValueError, match='greedy'):
        model.transcribe(None, greedy=True, lm=lm)


def test_lm_c_abi_refuses_unsupported_arguments_without_a_gpu():
    lib = _lib.lib()
    d = 16          # never dereferenced: argument checks come first
    n = lib.qk_ctc_beam_workspace_bytes(2, 5, 8)

    def call(C=62, W=8, top=1, order=2, alpha=0.5, beta=0.0, ws=n):
        return lib.qk_ctc_beam_search_decode_lm(0, 2, 5, C, d, d, W, top, 1, order, d, alpha, beta, 1, d, d, d, d, d, ws, None)
    assert call(order=0) == _lib.QK_ERR_UNSUPPORTED
    assert call(order=4) == _lib.QK_ERR_UNSUPPORTED
    assert call(C=65, order=3) == _lib.QK_ERR_UNSUPPORTED
    assert b'64' in lib.qk_last_error()
    assert call(C=257) == _lib.QK_ERR_UNSUPPORTED
    assert call(W=129) == _lib.QK_ERR_UNSUPPORTED
    assert call(W=8, top=9) == _lib.QK_ERR_UNSUPPORTED
    assert call(alpha=-1.0) == _lib.QK_ERR_INVALID_ARG
    assert call(alpha=float('nan')) == _lib.QK_ERR_INVALID_ARG
    assert call(alpha=float('inf')) == _lib.QK_ERR_INVALID_ARG
    assert call(beta=float('-inf')) == _lib.QK_ERR_INVALID_ARG
    assert call(ws=n - 4) == _lib.QK_ERR_WORKSPACE
    assert lib.qk_ctc_beam_search_decode_lm(0, 2, 5, 62, d, d, 8, 1, 1, 2, None, 0.5, 0.0, 1, d, d, d, d, d, n, None) == \
        _lib.QK_ERR_INVALID_ARG                                          # no table
    assert lib.qk_ctc_beam_search_decode_lm(0, 2, 5, 62, d, d, 8, 1, 1, 2, d, 0.5, 0.0, 1, d, d, d, None, d, n, None) == \
        _lib.QK_ERR_INVALID_ARG                                          # no score buffer


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------
def _dev():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    return torch.device('cuda:0')


_TORCH = {'fp32': torch.float32, 'bf16': torch.bfloat16}


@pytest.mark.gpu
@pytest.mark.parametrize('order', [1, 2, 3])
def test_lm_beam_search_equals_enumeration_when_nothing_is_pruned(order):
    dev = _dev()
    rng = np.random.RandomState(40 + order)
    top = 3
    for alpha, beta, eos in ((0.8, -0.6, True), (1.3, 0.0, False), (0.5, 0.9, True)):
        for y, tn in _exhaustive_cases():
            C = y.shape[1]
            lm = NgramLM(_random_table(rng, C, order), C - 1, order)
            want = LR.best_by_enumeration(y, tn, lm.logp, order, alpha, beta, eos)
            yt = torch.tensor(y[None], dtype=torch.float32, device=dev)
            dec, dlen, lp, sc = Fq.ctc_beam_search_decode_lm(yt, torch.tensor([tn]), lm, beam_width=128, top_paths=top,
                                                             merge_repeated=False, lm_weight=alpha, insertion_bonus=beta, eos=eos)
            dec, dlen, lp, sc = dec.cpu().numpy(), dlen.cpu().numpy(), lp.cpu().numpy(), sc.cpu().numpy()
            for k in range(top):
                if k >= len(want):
                    assert dlen[k, 0] == 0 and lp[0, k] == -np.inf and sc[0, k] == -np.inf
                    continue
                gap_hi = want[k - 1][2] - want[k][2] if k > 0 else 1.0
                gap_lo = want[k][2] - want[k + 1][2] if k + 1 < len(want) else 1.0
                assert abs(sc[0, k] - want[k][2]) < 1e-4, (order, k, sc[0, k], want[k])
                if min(gap_hi, gap_lo) > 1e-6:
                    assert tuple(dec[k, 0, :dlen[k, 0]]) == want[k][0], (order, alpha, beta, eos, k, want[k])
                    assert abs(lp[0, k] - want[k][1]) < 1e-4


def _peaky(rng, B, T, C):
    z = rng.randn(B, T, C) * 3.0
    z[..., -1] += 3.0
    e = np.exp(z - z.max(-1, keepdims=True))
    y = (e / e.sum(-1, keepdims=True)).astype(np.float32)
    y[y < 1e-3] = 0.0
    return y


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', ['fp32', 'bf16'])
def test_zero_weights_are_bit_identical_to_the_plain_beam_search(dtype):
    dev = _dev()
    rng = np.random.RandomState(12)
    B, T, C, W = 256, 200, 62, 100
    y = torch.tensor(_peaky(rng, B, T, C)).to(dev, _TORCH[dtype])
    il = torch.full((B,), T, dtype=torch.int32)
    il[rng.choice(B, 40, replace=False)] = torch.tensor(rng.randint(0, T, size=40), dtype=torch.int32)
    il = il.to(dev)
    corpus = _random_corpus(rng, C - 1, n=300)
    for order, top, merge in ((2, 1, True), (3, 3, False)):
        lm = NgramLM.estimate(corpus, C - 1, order)
        d0, l0, p0 = Fq.ctc_beam_search_decode(y, il, beam_width=W, top_paths=top, merge_repeated=merge)
        d1, l1, p1, s1 = Fq.ctc_beam_search_decode_lm(y, il, lm, beam_width=W, top_paths=top, merge_repeated=merge, lm_weight=0.0,
                                                      insertion_bonus=0.0, eos=True)
        assert torch.equal(d0, d1) and torch.equal(l0, l1)
        assert torch.equal(p0.view(torch.int32), p1.view(torch.int32))          # bit for bit
        assert torch.equal(p1, s1)


@pytest.mark.gpu
@pytest.mark.parametrize('order', [2, 3])
def test_lm_beam_search_at_the_benchmark_shape_matches_the_sampled_reference(order):
    """B = 256, T = 200, C = 62, W = 100 with an LM estimated from random sequences (order 2: the table in LDS; order 3: one staged row
    per beam) against the float64 reference on sampled utterances: paths equal where the selection margin is >= 1e-3, scores to 1e-3."""
    dev = _dev()
    rng = np.random.RandomState(30 + order)
    B, T, C, W = 256, 200, 62, 100
    y = torch.tensor(_peaky(rng, B, T, C)).to(dev)
    il = torch.full((B,), T, dtype=torch.int32)
    il[rng.choice(B, 40, replace=False)] = torch.tensor(rng.randint(1, T, size=40), dtype=torch.int32)
    lm = NgramLM.estimate(_random_corpus(rng, C - 1, n=400), C - 1, order)
    alpha, beta = 0.6, 0.4
    sample = rng.choice(B, 4, replace=False)
    yn = y.float().cpu().numpy()
    ref_paths, ref_lp, ref_sc, margins = LR.beam_search_lm_decode(yn[sample], il.numpy()[sample], W, 2, lm.logp, order, alpha, beta,
                                                                  eos=True, merge_repeated=False)
    dec, dlen, lp, sc = Fq.ctc_beam_search_decode_lm(y, il.to(dev), lm, beam_width=W, top_paths=2, merge_repeated=False,
                                                     lm_weight=alpha, insertion_bonus=beta, eos=True)
    dec, dlen, lp, sc = dec.cpu().numpy(), dlen.cpu().numpy(), lp.cpu().numpy(), sc.cpu().numpy()
    assert (sc[:, 0] >= sc[:, 1]).all()
    exact = 0
    for i, b in enumerate(sample):
        assert abs(sc[b, 0] - ref_sc[i, 0]) < 1e-3, (b, sc[b, 0], ref_sc[i, 0])
        if margins[i] >= 1e-3:
            exact += 1
            for k in range(2):
                assert tuple(dec[k, b, :dlen[k, b]]) == ref_paths[i][k], (b, k)
                assert abs(sc[b, k] - ref_sc[i, k]) < 1e-3 and abs(lp[b, k] - ref_lp[i, k]) < 1e-3
    # the score is the definition's S of the returned path, through the table
    for b in range(0, B, 17):
        n = int(il[b])
        path = tuple(dec[0, b, :dlen[0, b]])
        want = lp[b, 0] + alpha * lm.log_prob(path, eos=True) + beta * len(path)
        assert abs(sc[b, 0] - want) < 1e-3 * max(1.0, n / 50), (b, sc[b, 0], want)
    print('order %d: utterances with selection margin >= 1e-3: %d of %d; margins %s' % (order, exact, len(sample),
                                                                                        np.round(margins, 5).tolist()))


@pytest.mark.gpu
def test_the_lm_breaks_an_acoustic_tie():
    """Frame 1 gives classes b and c exactly the same posterior after a: the plain decoder keeps the lower class (b, the tie rule);
    an LM that prefers c after a makes the fused decoder return a c."""
    dev = _dev()
    a, b, c, blank = 0, 1, 2, 3
    y = np.array([[0.9, 0.03, 0.03, 0.04],
                  [0.02, 0.45, 0.45, 0.08],
                  [0.01, 0.01, 0.01, 0.97]], dtype=np.float32)
    yt = torch.tensor(y[None], device=dev)
    il = torch.tensor([3])
    lm = NgramLM.estimate([[a, c]] * 10 + [[a, b]], 3, 2)
    assert lm.logp[a, c] > lm.logp[a, b]
    dec, dlen, _ = Fq.ctc_beam_search_decode(yt, il, beam_width=8)
    assert dec[0, 0, :dlen[0, 0]].tolist() == [a, b]
    dec, dlen, lp, sc = Fq.ctc_beam_search_decode_lm(yt, il, lm, beam_width=8, lm_weight=0.5)
    assert dec[0, 0, :dlen[0, 0]].tolist() == [a, c]
    want = LR.best_by_enumeration(y, 3, lm.logp, 2, 0.5, 0.0, True)[0]
    assert want[0] == (a, c) and abs(float(sc[0, 0]) - want[2]) < 1e-5 and abs(float(lp[0, 0]) - want[1]) < 1e-5
    dec, lpk = layers.ctc_decode(yt, il, greedy=False, beam_width=8, lm=lm, lm_weight=0.5)
    assert dec[0][0].tolist() == [a, c] and torch.equal(lpk, sc)                # the fused score in the log_prob slot


@pytest.mark.gpu
def test_staged_rows_beyond_64_kb_of_table():
    """A bigram over C = 200 is 160 KB: the kernel stages one row per live beam (W = 128: 100 KB of LDS)."""
    dev = _dev()
    rng = np.random.RandomState(8)
    B, T, C, W = 3, 12, 200, 128
    y = _peaky(rng, B, T, C)
    il = np.array([12, 7, 0])
    lm = NgramLM.estimate(_random_corpus(rng, C - 1, n=300), C - 1, 2)
    ref_paths, ref_lp, ref_sc, margins = LR.beam_search_lm_decode(y, il, W, 1, lm.logp, 2, 0.7, -0.2, eos=True)
    dec, dlen, lp, sc = Fq.ctc_beam_search_decode_lm(torch.tensor(y, device=dev), torch.tensor(il), lm, beam_width=W, lm_weight=0.7,
                                                     insertion_bonus=-0.2)
    for b in range(B):
        assert abs(float(sc[b, 0]) - ref_sc[b, 0]) < 1e-3, (b, float(sc[b, 0]), ref_sc[b, 0])
        if margins[b] >= 1e-3:
            assert tuple(dec[0, b, :dlen[0, b]].tolist()) == ref_paths[b][0]
    assert int(dlen[0, 2]) == 0 and float(lp[2, 0]) == 0.0
    assert abs(float(sc[2, 0]) - 0.7 * lm.logp[C - 1, C - 1]) < 1e-5       # no frames: S = alpha log P(</s> | <s>)


@pytest.mark.gpu
def test_model_level_lm_wiring():
    from qcnn_amd import features
    from qcnn_amd.models.interspeech_model import TimitQCNN
    dev = _dev()
    np.random.seed(0)
    torch.manual_seed(0)
    B, T = 6, 48
    g = torch.Generator(device=dev).manual_seed(1)
    x = torch.randn(B, 4, 41, T, device=dev, generator=g).to(torch.bfloat16)
    labels = torch.randint(0, 61, (B, 12), device=dev, generator=g, dtype=torch.int32)
    il = torch.full((B, 1), T, dtype=torch.int32, device=dev)
    ll = torch.randint(4, 13, (B, 1), device=dev, generator=g, dtype=torch.int32)
    model = TimitQCNN(num_layers=4, start_filter=32, aact='none', dropout=0.3)
    with torch.no_grad():
        model(x[:1])
    model.to(dev)
    lm = NgramLM.estimate(_random_corpus(np.random.RandomState(2), 61, n=100), 61, 2)
    r0 = model.evaluate(x, labels, il, ll, greedy=False, beam_width=16)
    r1 = model.evaluate(x, labels, il, ll, greedy=False, beam_width=16, lm=lm, lm_weight=0.0)
    assert torch.equal(r0.decoded, r1.decoded) and int(r0.errors) == int(r1.errors) and float(r0.per) == float(r1.per)
    r2 = model.evaluate(x, labels, il, ll, greedy=False, beam_width=16, lm=lm, lm_weight=1.0, insertion_bonus=0.5)
    assert math.isfinite(float(r2.per))
    lengths = [16000, 9000, 401]
    wave = torch.tensor(np.random.RandomState(3).randn(3, 16000) * 3000, dtype=torch.int16, device=dev)
    dec, score = model.transcribe(wave, lengths, greedy=False, beam_width=8, lm=lm, lm_weight=0.8, dtype=torch.bfloat16)
    xw, fl = features.quaternion_fbank(wave, lengths, dtype=torch.bfloat16)
    want, wscore = model.decode(xw, fl, greedy=False, beam_width=8, lm=lm, lm_weight=0.8)
    assert all(torch.equal(p, q) for p, q in zip(dec, want)) and torch.equal(score, wscore)
    assert score.shape == (3, 1) and torch.isfinite(score).all()


@pytest.mark.gpu
def test_train_timit_example_reports_the_lm(tmp_path):
    import os
    import re
    import subprocess
    import sys
    from test_fbank import signals, sphere_bytes
    from qcnn_amd import data
    _dev()
    rng = np.random.RandomState(1)
    for split, spk, utt in (('TRAIN', 'FCJF0', 'SA1'), ('TRAIN', 'MDAB0', 'SX9'), ('TEST', 'MDAB1', 'SI2'), ('TEST', 'FAKS0', 'SA2')):
        d = tmp_path / split / 'DR1' / spk
        d.mkdir(parents=True, exist_ok=True)
        n = int(rng.randint(14000, 20000))
        (d / (utt + '.WAV')).write_bytes(sphere_bytes(signals([n], seed=int(rng.randint(1000)))[0].astype(np.int16)))
        phones = [data.TIMIT_PHONES_61[i] for i in rng.randint(0, 61, size=12)]
        cuts = np.linspace(0, n, len(phones) + 1).astype(int)
        (d / (utt + '.PHN')).write_text(''.join('%d %d %s\n' % (cuts[i], cuts[i + 1], p) for i, p in enumerate(phones)))
    root = os.path.dirname(os.path.dirname(os.path.realpath(__file__)))
    cmd = [sys.executable, os.path.join(root, 'examples', 'train_timit.py'), '--timit', str(tmp_path), '--steps', '2',
           '--eval-every', '1', '--layers', '4', '--batch', '2', '--lm-order', '2', '--beam-width', '8']
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600, universal_newlines=True)
    assert r.returncode == 0, r.stdout[-4000:]
    ppl = re.findall(r'2-gram phone LM from 2 TRAIN transcripts: held-out perplexity (\S+)', r.stdout)
    assert len(ppl) == 1 and np.isfinite(float(ppl[0])) and float(ppl[0]) > 1.0, r.stdout[-4000:]
    lines = re.findall(r'held-out beam 8 PER\(39\) without LM (\S+)\s+with 2-gram LM (\S+)', r.stdout)
    assert len(lines) == 2, r.stdout[-4000:]
    assert all(np.isfinite(float(a)) and np.isfinite(float(b)) for a, b in lines)
