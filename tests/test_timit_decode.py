"""TimitQCNN.decode / evaluate: the validation step of the reference (models/interspeech_model.py:182-185, val_function) carried through
to a phone error rate on the device, and the regression that made evaluation between training steps unsafe.

  * decode(x) == layers.ctc_decode(eval-mode model(x)) bit for bit; evaluate().loss == eval-mode ctc_mean_loss; the training flag is
    restored and no autograd graph is built;
  * the greedy and beam decodes of the reference-generated posteriors of golden fixture G17 (`pred`) equal tests/ctc_decode_ref.py;
  * evaluating between training steps leaves the trajectory bit-identical (deterministic mode): before the fix, the first dense layer's
    16-bit kernel re-layout was cached under one key for the channel-major reading the training forward uses and the plain dense layout
    the evaluation forward uses (functional._Call._prep_key).
"""
import glob
import os

import numpy as np
import pytest
import torch

import ctc_decode_ref as R
from conftest import GOLDEN
from qcnn_amd import _lib, dp, functional as F, layers
from qcnn_amd.models.interspeech_model import TimitQCNN

pytestmark = pytest.mark.gpu


def _dev():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    return torch.device('cuda:0')


def _model(dev, x, fuse_head=True, dropout=0.3, seed=0):
    np.random.seed(seed)
    torch.manual_seed(seed)
    m = TimitQCNN(num_layers=4, start_filter=32, aact='none', dropout=dropout, fuse_head=fuse_head)
    with torch.no_grad():
        m(x[:1])                                                  # build on first call, like Keras
    return m.to(dev)


def _batch(dev, B=8, T=48, seed=1):
    g = torch.Generator(device=dev).manual_seed(seed)
    x = torch.randn(B, 4, 41, T, device=dev, generator=g).to(torch.bfloat16)
    labels = torch.randint(0, 61, (B, 12), device=dev, generator=g, dtype=torch.int32)
    il = torch.full((B, 1), T, dtype=torch.int32, device=dev)
    ll = torch.randint(4, 13, (B, 1), device=dev, generator=g, dtype=torch.int32)
    return x, labels, il, ll


def test_decode_and_evaluate_compose_the_eval_forward():
    dev = _dev()
    x, labels, il, ll = _batch(dev)
    model = _model(dev, x)
    model.train()
    with torch.no_grad():
        model.eval()
        y = model(x)
        want_loss = model.ctc_mean_loss(x, labels, il, ll)
        model.train()
    for greedy in (True, False):
        got, glp = model.decode(x, greedy=greedy, beam_width=16, top_paths=1 if greedy else 2)
        assert model.training
        want, wlp = layers.ctc_decode(y, torch.full((x.shape[0],), x.shape[-1]), greedy=greedy, beam_width=16,
                                      top_paths=1 if greedy else 2)
        assert len(got) == len(want) and all(torch.equal(a, b) for a, b in zip(got, want))
        assert torch.equal(glp, wlp) and glp.grad_fn is None
    cm = torch.arange(62, dtype=torch.int32)
    cm[61] = -1
    cm[:10] = 0                                                   # fold ten classes into one (the TIMIT 61 -> 39 pattern)
    res = model.evaluate(x, labels, il, ll, class_map=cm)
    assert model.training
    assert res.loss.grad_fn is None and not res.loss.requires_grad
    assert abs(float(res.loss) - float(want_loss)) <= 1e-6 * abs(float(want_loss))
    dec, _ = layers.ctc_decode(y, il)
    err, sym, per = layers.label_error_rate(dec[0], None, labels, ll, class_map=cm)
    assert torch.equal(res.decoded, dec[0]) and int(res.errors) == int(err) and int(res.symbols) == int(sym)
    hyp = dec[0].cpu().numpy()
    lab = labels.cpu().numpy()
    want_err = sum(R.edit_distance(R.apply_class_map([v for v in hyp[b] if v >= 0], cm.tolist()),
                                   R.apply_class_map(lab[b, :int(ll[b])], cm.tolist())) for b in range(x.shape[0]))
    want_sym = sum(len(R.apply_class_map(lab[b, :int(ll[b])], cm.tolist())) for b in range(x.shape[0]))
    assert int(res.errors) == want_err and int(res.symbols) == want_sym
    assert abs(float(res.per) - want_err / want_sym) < 1e-6
    model.eval()
    model.evaluate(x, labels, il, ll, greedy=False, beam_width=8)
    assert not model.training                                    # the flag is restored, not forced to True


@pytest.mark.parametrize('path', sorted(glob.glob(os.path.join(GOLDEN, 'g17_timit_*.npz'))), ids=os.path.basename)
def test_decoders_on_the_reference_posteriors_of_g17(path):
    dev = _dev()
    z = np.load(path)
    pred, il = z['pred'].astype(np.float32), z['input_length']
    y = torch.tensor(pred, device=dev)
    want, _ = R.greedy_decode(pred, il)
    dec, dlen, _ = F.ctc_greedy_decode(y, torch.tensor(il))
    for b, s in enumerate(want):
        assert tuple(dec[b, :dlen[b]].tolist()) == s
    for W in (1, 8, 100):
        top = min(2, W)
        paths, lps, margins = R.beam_search_decode(pred, il, W, top, merge_repeated=True)
        dec, dlen, lp = F.ctc_beam_search_decode(y, torch.tensor(il), beam_width=W, top_paths=top)
        for b in range(pred.shape[0]):
            assert abs(float(lp[b, 0]) - lps[b, 0]) < 1e-4
            if margins[b] >= 1e-3:
                for k in range(top):
                    assert tuple(dec[k, b, :dlen[k, b]].tolist()) == paths[b][k], (W, b, k)


def _train(dev, fuse_head, evaluate_between, x, labels, il, ll, xe, le, ile, lle):
    model = _model(dev, x, fuse_head=fuse_head)
    model.train()
    flat = dp.FlatParams([p for p in model.parameters() if p.requires_grad], direct=True)
    m, v = torch.zeros_like(flat.param), torch.zeros_like(flat.param)
    torch.manual_seed(7)                                          # the dropout masks of the three steps
    evals = []
    for step in range(1, 4):
        loss = model.ctc_mean_loss(x, labels, il, ll)
        loss.backward()
        F.adam_step(flat.param, flat.grad, m, v, step, lr=1e-3, zero_grad=True)
        if evaluate_between:
            evals.append(model.evaluate(xe, le, ile, lle))
    torch.cuda.synchronize()
    return model, flat.param.clone(), m.clone(), v.clone(), evals


@pytest.mark.parametrize('fuse_head', [False, True])
def test_evaluation_between_training_steps_does_not_disturb_training(fuse_head):
    dev = _dev()
    x, labels, il, ll = _batch(dev, seed=1)
    xe, le, ile, lle = _batch(dev, B=6, seed=2)
    with _lib.debug_flags(_lib.QK_DBG_DETERMINISTIC):
        _, p0, m0, v0, _ = _train(dev, fuse_head, False, x, labels, il, ll, xe, le, ile, lle)
        model, p1, m1, v1, evals = _train(dev, fuse_head, True, x, labels, il, ll, xe, le, ile, lle)
        for a, b, name in ((p0, p1, 'parameters'), (m0, m1, 'first moment'), (v0, v1, 'second moment')):
            assert torch.equal(a, b), '%s differ when evaluate() runs between the steps: max |diff| %g' % (name, float((a - b).abs().max()))
        # after training, evaluation equals that of a fresh model (empty caches) holding the same weights
        got = model.evaluate(xe, le, ile, lle)
        fresh = _model(dev, x, fuse_head=fuse_head, seed=3)
        fresh.load_state_dict(model.state_dict())
        want = fresh.evaluate(xe, le, ile, lle)
    assert torch.equal(got.loss, want.loss) and torch.equal(got.decoded, want.decoded) and torch.equal(got.errors, want.errors)
    assert torch.equal(got.loss, evals[-1].loss) and torch.equal(got.decoded, evals[-1].decoded)
