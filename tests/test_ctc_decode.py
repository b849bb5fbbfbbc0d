"""K.ctc_decode (greedy / beam search) and tf.edit_distance on the device (include/qk.h, "CTC decoding"; functional.ctc_*_decode,
functional.edit_distance, layers.ctc_decode / label_error_rate) against the float64 restatement in tests/ctc_decode_ref.py.

CPU: the reference is pinned to the definition (its unpruned beam search equals the enumeration of all frame paths of oracle.ctc_enum,
to 1e-10; its greedy decoder equals argmax-collapse on hand cases) and the API refuses CPU tensors and unsupported arguments.
GPU: greedy bit-exact (decodes, lengths) in fp32 / bf16 / fp16 with edge cases; beam search on the exhaustive cases and at the
benchmark shape (B = 256, T = 200, C = 62, W = 100); the edit distance exact against a Python DP.
"""
import numpy as np
import pytest
import torch

import ctc_decode_ref as R
from qcnn_amd import functional as Fq
from qcnn_amd import layers


def _soft(rng, *shape, scale=1.5):
    z = rng.randn(*shape) * scale
    e = np.exp(z - z.max(-1, keepdims=True))
    return e / e.sum(-1, keepdims=True)


def _exhaustive_cases():
    """(y (T, C), tn): C = 3 with T <= 6 and C = 4 with T <= 4 -- every prefix fits into 128 beams, so nothing is pruned."""
    rng = np.random.RandomState(5)
    cases = []
    for C, T in ((3, 6), (3, 5), (3, 2), (4, 4), (4, 3), (4, 1)):
        for _ in range(2):
            cases.append((_soft(rng, T, C), T))
    return cases


# ---- CPU: the reference against the definition -------------------------------------------------------------------------------
def test_reference_beam_search_without_pruning_equals_enumeration():
    for y, tn in _exhaustive_cases():
        want = R.top_labelings_enum(y, tn)
        paths, lps, _ = R.beam_search_one(y, tn, 128, 5, merge_repeated=False)
        for k in range(min(5, len(want))):
            assert abs(lps[k] - want[k][1]) < 1e-10, (k, lps[k], want[k])
            if k + 1 >= len(want) or want[k][1] - want[k + 1][1] > 1e-9:          # (an exact tie may be listed in either order)
                if k == 0 or want[k - 1][1] - want[k][1] > 1e-9:
                    assert paths[k] == want[k][0], (k, paths[k], want[k])
        for k in range(len(want), 5):
            assert paths[k] == () and lps[k] == -np.inf


def test_reference_greedy_is_argmax_collapse():
    C = 4                                   # blank = 3
    A, Bc, blank = 0, 1, 3

    def onehot(seq, tie=None):
        y = np.full((len(seq), C), 0.05)
        for t, c in enumerate(seq):
            y[t, c] = 0.85
        if tie is not None:
            t, c = tie
            y[t, c] = 0.85                  # a second maximum: the lower index wins
        return y
    y = onehot([A, Bc, Bc, blank, Bc, Bc])
    dec, lp = R.greedy_decode(y[None], [6])
    assert dec[0] == (A, Bc, Bc)            # A B B * B B -> A B B
    assert abs(lp[0] + 6 * np.log(0.85 + 1e-7)) < 1e-12
    dec, _ = R.greedy_decode(onehot([blank, 2, 2, blank], tie=(1, 1))[None], [4])
    assert dec[0] == (1, 2)                 # frame 1: classes 1 and 2 tie, 1 wins; frame 2: 2
    dec, _ = R.greedy_decode(onehot([A, A, blank, blank])[None], [2])
    assert dec[0] == (A,)
    dec, lp = R.greedy_decode(onehot([A])[None], [0])
    assert dec[0] == () and lp[0] == 0.0
    assert R.edit_distance([1, 2, 3], [1, 3]) == 1 and R.edit_distance([], [1, 2]) == 2 and R.edit_distance([4, 5], []) == 2
    assert R.apply_class_map([0, 1, 2, 7], [0, 0, -1]) == [0, 0, 7]


def test_decode_api_rejects_cpu_tensors_and_unsupported_arguments():
    y = torch.rand(2, 5, 4)
    il = torch.tensor([5, 5])
    with pytest.raises(RuntimeError, match='CPU'):
        Fq.ctc_greedy_decode(y, il)
    with pytest.raises(RuntimeError, match='CPU'):
        Fq.ctc_beam_search_decode(y, il)
    with pytest.raises(RuntimeError, match='CPU'):
        Fq.edit_distance(torch.zeros(2, 3, dtype=torch.int32), [3, 3], torch.zeros(2, 3, dtype=torch.int32), [3, 3])
    with pytest.raises(ValueError, match='beam_width'):
        Fq.ctc_beam_search_decode(y, il, beam_width=129)
    with pytest.raises(ValueError, match='beam_width'):
        Fq.ctc_beam_search_decode(y, il, beam_width=0)
    with pytest.raises(ValueError, match='top_paths'):
        Fq.ctc_beam_search_decode(y, il, beam_width=4, top_paths=5)
    with pytest.raises(RuntimeError, match='CPU'):
        layers.ctc_decode(y, il)


def test_c_abi_refuses_unsupported_decoder_shapes_without_a_gpu():
    from qcnn_amd import _lib
    lib = _lib.lib()
    dummy = 16      # never dereferenced: argument checks come first
    assert lib.qk_ctc_greedy_decode(0, 2, 5, 257, dummy, dummy, dummy, dummy, dummy, None) == _lib.QK_ERR_UNSUPPORTED
    assert b'256' in lib.qk_last_error()
    n = lib.qk_ctc_beam_workspace_bytes(2, 5, 8)
    assert n == 2 * 5 * 8 * 4
    args = lambda C, W, P: (0, 2, 5, C, dummy, dummy, W, P, 1, dummy, dummy, dummy, dummy, 1 << 20, None)
    assert lib.qk_ctc_beam_search_decode(*args(62, 129, 1)) == _lib.QK_ERR_UNSUPPORTED
    assert lib.qk_ctc_beam_search_decode(*args(62, 8, 9)) == _lib.QK_ERR_UNSUPPORTED
    assert lib.qk_ctc_beam_search_decode(*args(257, 8, 1)) == _lib.QK_ERR_UNSUPPORTED
    assert lib.qk_ctc_beam_search_decode(0, 2, 5, 62, dummy, dummy, 8, 1, 1, dummy, dummy, dummy, dummy, n - 4, None) == _lib.QK_ERR_WORKSPACE
    assert lib.qk_edit_distance(2, dummy, 4, dummy, dummy, 1025, dummy, None, 0, dummy, None, None) == _lib.QK_ERR_UNSUPPORTED
    assert lib.qk_ctc_greedy_decode(0, 2, 5, 1, dummy, dummy, dummy, dummy, dummy, None) == _lib.QK_ERR_INVALID_ARG


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------
def _dev():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    return torch.device('cuda:0')


_TORCH = {'fp32': torch.float32, 'bf16': torch.bfloat16, 'fp16': torch.float16}


def _greedy_check(y, il):
    """Kernel vs reference on the posteriors the kernel actually read (the rounded 16-bit values)."""
    dec, dlen, lp = Fq.ctc_greedy_decode(y, il)
    yn = y.float().cpu().numpy()
    want, wlp = R.greedy_decode(yn, il.cpu().numpy())
    dec, dlen, lp = dec.cpu().numpy(), dlen.cpu().numpy(), lp.cpu().numpy()
    T = y.shape[1]
    for b, seq in enumerate(want):
        assert dlen[b] == len(seq), (b, dlen[b], seq)
        assert tuple(dec[b, :dlen[b]]) == seq, b
        assert (dec[b, dlen[b]:] == -1).all()
        tn = min(max(int(il.reshape(-1)[b]), 0), T)
        assert abs(lp[b] - wlp[b]) <= 1e-6 * abs(wlp[b]) + 2e-7 * tn, (b, lp[b], wlp[b])


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', ['fp32', 'bf16', 'fp16'])
def test_greedy_decode_matches_reference_bit_exactly(dtype):
    dev = _dev()
    rng = np.random.RandomState(1)
    B, T, C = 33, 150, 62
    y = torch.tensor(_soft(rng, B, T, C, scale=2.0), dtype=torch.float32)
    y[:, :, C - 1] += 0.3                                                # blank-heavy
    y[3] = 0.0
    y[3, :, C - 1] = 1.0                                                 # all-blank frames: empty decode
    y[4, 10:40] = 1.0 / C                                                # exact ties over every class: the lowest index
    il = torch.tensor(rng.randint(1, T + 1, size=B), dtype=torch.int32)
    il[0], il[1], il[2] = 0, T + 17, -3                                  # no frames, more than T, negative
    yd = y.to(dev, _TORCH[dtype])
    if dtype == 'bf16':
        assert (yd.float().topk(2, dim=-1).values.diff(dim=-1) == 0).any()       # real argmax ties after rounding
    _greedy_check(yd, il.to(dev))
    _greedy_check(yd, il.reshape(-1, 1))                                 # (B, 1) lengths, on the host
    for C2 in (2, 256):
        y2 = torch.tensor(_soft(rng, 5, 70, C2, scale=1.0), dtype=torch.float32).to(dev, _TORCH[dtype])
        _greedy_check(y2, torch.tensor([70, 1, 0, 69, 35], dtype=torch.int32, device=dev))


@pytest.mark.gpu
@pytest.mark.parametrize('top_paths', [1, 2, 3, 4, 5])
def test_beam_search_equals_enumeration_when_nothing_is_pruned(top_paths):
    dev = _dev()
    for y, tn in _exhaustive_cases():
        want = R.top_labelings_enum(y, tn)
        yt = torch.tensor(y[None], dtype=torch.float32, device=dev)
        dec, dlen, lp = Fq.ctc_beam_search_decode(yt, torch.tensor([tn]), beam_width=128, top_paths=top_paths, merge_repeated=False)
        dec, dlen, lp = dec.cpu().numpy(), dlen.cpu().numpy(), lp.cpu().numpy()
        for k in range(top_paths):
            if k >= len(want):
                assert dlen[k, 0] == 0 and lp[0, k] == -np.inf and (dec[k, 0] == -1).all()
                continue
            assert abs(lp[0, k] - want[k][1]) < 1e-5, (k, lp[0, k], want[k])
            gap_hi = want[k - 1][1] - want[k][1] if k > 0 else 1.0
            gap_lo = want[k][1] - want[k + 1][1] if k + 1 < len(want) else 1.0
            if min(gap_hi, gap_lo) > 1e-4:
                assert tuple(dec[k, 0, :dlen[k, 0]]) == want[k][0], (k, want[k])
        # the top path's probability through the CTC cost kernel: log_prob == -qk_ctc_batch_cost(that labelling)
        lab = torch.tensor([list(want[0][0]) + [0]], dtype=torch.int32)
        cost = layers.ctc_batch_cost(yt, lab.to(dev), torch.tensor([[tn]]), torch.tensor([[len(want[0][0])]]))
        assert abs(float(cost) + lp[0, 0]) < 1e-5


def _peaky(rng, B, T, C):
    """Peaky synthetic posteriors (softmax of scaled random logits, blank-heavy, small values cut to exact zeros) -- what a trained
    model's output looks like."""
    z = rng.randn(B, T, C) * 3.0
    z[..., -1] += 3.0
    e = np.exp(z - z.max(-1, keepdims=True))
    y = (e / e.sum(-1, keepdims=True)).astype(np.float32)
    y[y < 1e-3] = 0.0
    return y


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', ['fp32', 'bf16'])
def test_beam_search_at_the_benchmark_shape_matches_the_sampled_reference(dtype):
    """B = 256, T = 200, C = 62, W = 100 against the float64 reference on 16 sampled utterances.  Beam membership is discontinuous in
    the scores: an utterance whose smallest selection margin (reference) is >= 1e-3 nats must decode exactly; for every utterance the
    top path's log_prob is within 1e-3 of the reference's, and every returned log_prob is at most the labelling's full probability
    (-qk_ctc_batch_cost of the uncollapsed prefix: the beam only ever loses alignments)."""
    dev = _dev()
    rng = np.random.RandomState(11)
    B, T, C, W = 256, 200, 62, 100
    y = torch.tensor(_peaky(rng, B, T, C)).to(dev, _TORCH[dtype])
    il = torch.full((B,), T, dtype=torch.int32)
    il[rng.choice(B, 40, replace=False)] = torch.tensor(rng.randint(1, T, size=40), dtype=torch.int32)
    sample = rng.choice(B, 16, replace=False)
    yn = y.float().cpu().numpy()
    ref_paths, ref_lp, margins = R.beam_search_decode(yn[sample], il.numpy()[sample], W, 3, merge_repeated=False)
    runs = {}
    for top, merge in ((1, True), (3, False), (3, True)):
        dec, dlen, lp = Fq.ctc_beam_search_decode(y, il.to(dev), beam_width=W, top_paths=top, merge_repeated=merge)
        runs[top, merge] = (dec.cpu().numpy(), dlen.cpu().numpy(), lp.cpu().numpy())
        assert (lp[:, :-1] >= lp[:, 1:]).all() if top > 1 else True
    exact = 0
    for i, b in enumerate(sample):
        for (top, merge), (dec, dlen, lp) in runs.items():
            assert abs(lp[b, 0] - ref_lp[i, 0]) < 1e-3, (b, top, merge, lp[b, 0], ref_lp[i, 0])
            if margins[i] >= 1e-3:
                for k in range(top):
                    want = R.collapse_repeats(ref_paths[i][k]) if merge else ref_paths[i][k]
                    assert tuple(dec[k, b, :dlen[k, b]]) == want, (b, k, top, merge)
                    assert abs(lp[b, k] - ref_lp[i, k]) < 1e-3
        exact += margins[i] >= 1e-3
    # log_prob <= log p(labelling) through the cost kernel, for the uncollapsed top-3 prefixes
    dec, dlen, lp = runs[3, False]
    L = int(dlen.max())
    for k in range(3):
        lab = torch.tensor(np.maximum(dec[k, :, :max(L, 1)], 0), dtype=torch.int32, device=dev)
        ok = torch.tensor(dlen[k] <= 127)
        cost = layers.ctc_batch_cost(y, lab, il.to(dev), torch.tensor(dlen[k], device=dev)).float().cpu().reshape(-1)
        full = -cost.numpy()
        fin = np.isfinite(lp[:, k]) & ok.numpy()
        assert (lp[fin, k] <= full[fin] + 1e-3).all()
        assert (lp[fin, k] >= full[fin] - 5.0).all()            # and the beam kept most of it
    print('utterances with selection margin >= 1e-3: %d of 16; margins %s' % (exact, np.round(margins, 5).tolist()))


@pytest.mark.gpu
def test_beam_width_one_is_a_best_path_search_and_merges_repeats():
    dev = _dev()
    rng = np.random.RandomState(3)
    y = _peaky(rng, 8, 60, 62)
    il = np.array([60, 59, 1, 0, 60, 30, 45, 60])
    ref_paths, ref_lp, _ = R.beam_search_decode(y, il, 1, 1, merge_repeated=True)
    dec, dlen, lp = Fq.ctc_beam_search_decode(torch.tensor(y, device=dev), torch.tensor(il), beam_width=1, top_paths=1)
    for b in range(8):
        assert tuple(dec[0, b, :dlen[0, b]].tolist()) == ref_paths[b][0]
        assert abs(float(lp[b, 0]) - ref_lp[b, 0]) < 1e-3
    assert int(dlen[0, 3]) == 0 and float(lp[3, 0]) == 0.0              # no frames: empty decode, log_prob 0


@pytest.mark.gpu
def test_edit_distance_is_exact():
    dev = _dev()
    rng = np.random.RandomState(7)
    B, Lh, Lr = 24, 778, 1024
    hyp = rng.randint(0, 8, size=(B, Lh))
    ref = rng.randint(0, 8, size=(B, Lr))
    hl = rng.randint(0, 80, size=B)
    rl = rng.randint(0, 80, size=B)
    hl[0], rl[1], hl[2], rl[2] = 0, 0, 0, 0                             # empty hypothesis / reference / both
    hl[3], rl[3] = Lh, Lr                                               # hypothesis of 778 tokens, reference of 1024
    hl[4], rl[4] = Lh, 300
    rl[5], hl[5] = 1000, 50
    cmap = np.array([0, 1, 1, -1, 2, 3, -1, 4])                        # folds and drops
    for cm in (None, cmap):
        got = Fq.edit_distance(torch.tensor(hyp, device=dev), torch.tensor(hl), torch.tensor(ref, device=dev), torch.tensor(rl),
                               class_map=None if cm is None else torch.tensor(cm))
        got = got.cpu().numpy()
        for b in range(B):
            want = R.edit_distance(R.apply_class_map(hyp[b, :hl[b]], cm), R.apply_class_map(ref[b, :rl[b]], cm))
            assert got[b] == want, (b, cm is not None, got[b], want)
    # short references take the narrow kernels; the label error rate sums distances over mapped reference lengths
    for Lr2 in (5, 63, 64, 127, 200, 511, 512):
        r2 = rng.randint(0, 8, size=(6, Lr2))
        rl2 = rng.randint(0, Lr2 + 1, size=6)
        got = Fq.edit_distance(torch.tensor(hyp[:6, :90], device=dev), torch.tensor(np.minimum(hl[:6], 90)),
                               torch.tensor(r2, device=dev), torch.tensor(rl2)).cpu().numpy()
        for b in range(6):
            assert got[b] == R.edit_distance(hyp[b, :min(hl[b], 90)], r2[b, :rl2[b]]), (Lr2, b)
    dec = torch.tensor(np.where(np.arange(Lh)[None, :] < hl[:, None], hyp, -1), device=dev)
    err, sym, per = layers.label_error_rate(dec, None, torch.tensor(ref), torch.tensor(rl).reshape(-1, 1), class_map=cmap)
    want_err = sum(R.edit_distance(R.apply_class_map(hyp[b, :hl[b]], cmap), R.apply_class_map(ref[b, :rl[b]], cmap)) for b in range(B))
    want_sym = sum(len(R.apply_class_map(ref[b, :rl[b]], cmap)) for b in range(B))
    assert int(err) == want_err and int(sym) == want_sym and abs(float(per) - want_err / want_sym) < 1e-6
    norm = layers.edit_distance(dec, None, torch.tensor(ref, device=dev), torch.tensor(rl), normalize=True).cpu().numpy()
    b = int(np.nonzero(rl[6:] > 0)[0][0]) + 6
    assert abs(norm[b] - R.edit_distance(hyp[b, :hl[b]], ref[b, :rl[b]]) / rl[b]) < 1e-6


@pytest.mark.gpu
def test_layers_ctc_decode_has_the_keras_shapes():
    dev = _dev()
    rng = np.random.RandomState(4)
    y = torch.tensor(_peaky(rng, 6, 40, 62), device=dev)
    il = torch.tensor([[40], [12], [0], [40], [5], [33]])
    dec, lp = layers.ctc_decode(y, il)
    want, wlp = R.greedy_decode(y.cpu().numpy(), il.numpy())
    assert len(dec) == 1 and dec[0].dtype == torch.int64 and lp.shape == (6, 1)
    assert dec[0].shape == (6, max(len(s) for s in want))
    for b, s in enumerate(want):
        row = dec[0][b].tolist()
        assert tuple(row[:len(s)]) == s and all(v == -1 for v in row[len(s):])
    dec, lp = layers.ctc_decode(y, il, greedy=False, beam_width=16, top_paths=3)
    assert len(dec) == 3 and lp.shape == (6, 3) and all(d.dtype == torch.int64 and d.shape[0] == 6 for d in dec)
