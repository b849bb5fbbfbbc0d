#!/usr/bin/env python
"""Training loop for the TIMIT quaternion CNN on the TIMIT corpus itself: waveforms and .PHN transcriptions in, phone error rate out,
all on one GPU.  The reference ships the model (models/interspeech_model.py:getTimitModel2D) and its input shape (4, 41, None) but no
feature code; here the features come from qcnn_amd.features.quaternion_fbank (40 log mel energies + log energy, and their first three
time derivatives as the quaternion components), computed on the device per batch.

    python examples/train_timit.py --timit /path/to/TIMIT --steps 2000 --eval-every 200

--timit DIR is walked for `*.WAV` + `*.PHN` pairs under TRAIN/ (training) and TEST/ (held out).  Utterances are batched by length;
the loss is TimitQCNN.training_loss (mean CTC cost + the l2 terms) with the fused Adam kernel; every --eval-every steps the held-out
CTC cost and the 39-class phone error rate (Lee & Hon folding) of one held-out batch are printed.

--clipnorm / --clipvalue (Keras' Adam(clipnorm=, clipvalue=)), --dtype float16 and --dynamic-loss-scale switch the optimiser step to
qcnn_amd.training.GradGuard: gradient norm, overflow check, clipping and the loss-scale update run on the device, a step with an inf /
NaN gradient is skipped, and every log line shows the norm, the scale and the number of skipped steps.

--lm-order N (1-3; 0 = off) estimates an interpolated Kneser-Ney phone N-gram LM (qcnn_amd.lm.NgramLM) from the TRAIN transcripts,
prints its held-out perplexity, and adds to every evaluation the PER(39) of the beam search (--beam-width) without and with the LM
fused in (--lm-weight, --insertion-bonus).

    python examples/train_timit.py --timit /path/to/TIMIT --eval-every 200 --lm-order 2 --lm-weight 0.5 --beam-width 16

--specaug augments the TRAINING batches with qcnn_amd.features.SpecAugment (time warp, frequency and time masks on the device, one
launch, seeded from --seed; --time-warp, --freq-masks, --freq-width, --time-masks, --time-width, --time-ratio).  Evaluation batches
are never augmented.  The default policy is scaled from the paper's LibriSpeech policy; no phone error rate has been measured with it.

--speed-perturb resamples every utterance of a TRAINING batch by one of --speeds (default 0.9,1.0,1.1; tempo and pitch change
together, as `sox speed` does) and multiplies it by a gain drawn from --volume LO,HI (default 1,1), on the device in front of the
filter bank (qcnn_amd.features.SpeedPerturb, one launch, seeded from --seed).  The labels are unchanged: a sped-up utterance has
fewer frames for the same labels.  Evaluation batches are never perturbed; it combines with --specaug.  No phone error rate has been
measured with it.

--noise-reverb convolves, with probability --rir-prob (default 0.5), every utterance of a TRAINING batch with a room impulse response
and adds, with probability --noise-prob (default 0.5), a noise recording at a signal-to-noise ratio drawn from --snr LO,HI dB (default
5,20), on the device behind --speed-perturb and in front of the filter bank (qcnn_amd.features.NoiseReverb, two launches, seeded from
--seed).  --rir-dir DIR / --noise-dir DIR name directories of audio files (any format qcnn_amd.data.read_audio reads; walked
recursively); without them synthetic banks are used (qcnn_amd.features.synthetic_rirs / synthetic_noises).  Lengths and labels are
unchanged.  Evaluation batches are never corrupted; it combines with --speed-perturb and --specaug.  No phone error rate has been
measured with it.

--align-eval adds to every evaluation the forced alignment of the held-out batch to its transcripts (TimitQCNN.align) and prints the
share of phone boundaries it places within 20 ms of the hand-labelled ones in the .PHN files (a boundary is the centre of the
phone's first frame, qcnn_amd.features.frames_to_samples).  Nobody has measured this figure for a trained model yet.

--confusions N (0 = off) adds to every evaluation the split of the 39-class errors of ALL held-out batches into %cor / %sub / %del /
%ins (of the reference phones, as sclite prints them; TimitQCNN.error_breakdown) and the N largest confusion pairs of the 39-class
matrix, which is accumulated on the device over the batches (`<ins>` / `<del>` stand for the missing partner).

--warmup N, --lr-decay {inverse-time,exponential,cosine,inv-sqrt} (with --decay-steps, --decay-rate, --lr-floor), --ema D,
--halve-on-plateau (with --plateau-patience), --checkpoint PATH and --resume PATH switch the optimiser step to
qcnn_amd.training.ScheduledAdam: the rate of every step is formed on the device from the step counter (--lr is the base rate;
cosine decays over --steps), with --ema an exponential moving average of the weights is kept and every evaluation runs with the
AVERAGED weights (the log line says so), with --halve-on-plateau the rate is halved whenever the held-out PER(39) has not improved
for more than --plateau-patience evaluations (newbob), and every log line shows the rate of the last applied step.  --checkpoint
writes model, optimiser, augmentation counters, step and batch-order state at every evaluation; --resume continues from such a file
(give the same options; under cosine that includes --steps, which is the schedule's length).  It combines with the guard options above.  No phone error rate has been measured with any of them.

--model qlstm trains qcnn_amd.models.TimitQLSTM in place of the quaternion CNN: --rnn-layers bidirectional QuaternionLSTM layers of
--rnn-units units (default 4 x 1024) on the same filter-bank input, --dropout between them, the same output layer, loss, decoding
and evaluation; the frame counts of a batch are the recurrent layers' lengths.  --layers / --filters / --aact do not apply to it.
--layer-norm puts a quaternion layer normalisation (qcnn_amd.complexnn.QuaternionLayerNormalization) behind every recurrent layer.
No phone error rate has been measured with it.

--model qtransformer trains qcnn_amd.models.TimitQTransformer: a QuaternionDense projection to --tf-units plus a fixed sinusoidal
position table, --tf-layers pre-norm encoder blocks (quaternion layer normalisation, QuaternionMultiHeadAttention with --tf-heads
heads, a feed-forward pair of QuaternionDense layers --tf-ff wide; --dropout in both residual branches), a final normalisation and
the same output layer, loss, decoding and evaluation; the frame counts of a batch are the attention's lengths, so padding frames
are never attended to.  --tf-units = 64 or 128 times --tf-heads runs the attention on the matrix cores in bf16 / fp16.
No phone error rate has been measured with it.

--model qconformer trains qcnn_amd.models.TimitQConformer: the same projection and position table, --tf-layers macaron Conformer
blocks (half-step feed-forward, QuaternionMultiHeadAttention, the convolution module -- a gated pointwise projection, a depthwise
quaternion convolution of --conv-kernel taps over time in one fused kernel, layer normalisation, swish, a pointwise projection --
half-step feed-forward, a closing normalisation) and the same output layer; the frame counts of a batch are the lengths of the
attention and of the convolution, so padding frames are neither attended to nor convolved over.  The --tf-* options apply to it.
Nobody has measured a phone error rate with it.

--model qtransducer trains qcnn_amd.models.TimitQTransducer: --encoder qlstm | qtransformer | qconformer (built from the same
--rnn-* / --tf-* / --conv-kernel options; its CTC output layer stays unused) under the transducer loss, with a quaternion LSTM
prediction network of --pred-units over the label history and a joint network of --joint-units.  The loss is
TimitQTransducer.training_loss (mean transducer cost + the l2 terms; three HIP launches for the cost and its gradient); with
--eval-every the held-out batch is decoded greedily (time-synchronous, at most 4 symbols per frame) and scored with the same phone
error rate.  --lm-order, --align-eval and --confusions belong to the CTC models.  Nobody has measured a phone error rate with it.

--device-corpus packs TRAIN and TEST once into device memory (qcnn_amd.data.DeviceCorpus) and takes every training batch from
DeviceCorpus.next_batch: one launch gathers the padded waveforms, lengths and labels of the next row of an EpochSampler, whose
order is a keyed permutation of the length-sorted batches evaluated on the device -- real epochs (every batch once per epoch, a new
order each epoch; the log line shows the epoch) in place of draws with replacement, and no per-step host assembly or copy.  Held-out
batches come from DeviceCorpus.batch.  The sampler's position is saved with the augmentation counters by --checkpoint.  Without the
flag the script behaves exactly as before.
"""
import argparse
import contextlib
import fractions
import os
import sys
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.realpath(__file__))))
import qcnn_amd  # noqa: E402,F401
from qcnn_amd import dp, functional as F, layers  # noqa: E402
from qcnn_amd.data import DeviceCorpus, EpochSampler, TIMIT_PHONES_39, TIMIT_PHONES_61, read_audio, read_phn, read_phn_segments, timit_61_to_39_class_map  # noqa: E402
from qcnn_amd.features import (NoiseReverb, SpecAugment, SpeedPerturb, frames_to_samples, quaternion_fbank, synthetic_noises,  # noqa: E402
                               synthetic_rirs)
from qcnn_amd.lm import NgramLM  # noqa: E402
from qcnn_amd.models import getTimitModel2D  # noqa: E402
from qcnn_amd.training import GradGuard, LRSchedule, ReduceOnPlateau, ScheduledAdam, load_checkpoint, save_checkpoint  # noqa: E402


def load_split(root, boundaries=False):
    """[(int16 samples, int32 phone classes)] of every WAV / PHN pair under root, sorted by path; with `boundaries` each entry also
    carries the phones' hand-labelled start samples (int64)."""
    index = {p: c for c, p in enumerate(TIMIT_PHONES_61)}
    utts = []
    for d, _, files in sorted(os.walk(root)):
        by_lower = {f.lower(): f for f in files}
        for f in sorted(files):
            stem, ext = os.path.splitext(f)
            if ext.lower() != '.wav' or (stem + '.phn').lower() not in by_lower:
                continue
            wav = read_audio(os.path.join(d, f))
            phn = os.path.join(d, by_lower[(stem + '.phn').lower()])
            phones = read_phn(phn)
            utt = (wav, np.array([index[p] for p in phones], dtype=np.int32))
            if boundaries:
                utt += (np.array([seg[0] for seg in read_phn_segments(phn)], dtype=np.int64),)
            utts.append(utt)
    return utts


def find_split(root, name):
    for d in os.listdir(root):
        if d.lower() == name.lower() and os.path.isdir(os.path.join(root, d)):
            return os.path.join(root, d)
    raise SystemExit('%s: no %s/ directory' % (root, name))


def length_batches(utts, batch):
    """Index lists of up to `batch` utterances of similar length (sorted by sample count, then cut)."""
    order = sorted(range(len(utts)), key=lambda i: len(utts[i][0]))
    return [order[i:i + batch] for i in range(0, len(order), batch)]


def parse_speeds(text):
    """'0.9,1.0,1.1' -> ((9, 10), (1, 1), (11, 10)): each speed as the closest fraction with a denominator <= 32."""
    out = []
    for word in text.split(','):
        f = fractions.Fraction(word.strip()).limit_denominator(32)
        if not 0 < f.numerator <= 32:
            raise argparse.ArgumentTypeError('speed %r: not a fraction of two numbers in 1 .. 32' % word)
        out.append((f.numerator, f.denominator))
    return tuple(out)


def parse_volume(text):
    lo, hi = (float(v) for v in text.split(','))
    return lo, hi


def read_audio_dir(root, what):
    """Every audio file under `root` that read_audio can read, as a list of 1-D arrays (sorted by path)."""
    out = []
    for d, _, files in sorted(os.walk(root)):
        for f in sorted(files):
            try:
                wav = np.asarray(read_audio(os.path.join(d, f)))
            except (ValueError, OSError):
                continue
            if wav.ndim == 1 and wav.size:
                out.append(wav)
    if not out:
        raise SystemExit('%s: no readable audio file for the %s bank' % (root, what))
    return out


def to_device(utts, idx, dev, dtype, augment=None, wave_augment=None):
    """Features (quaternion_fbank, per-utterance normalisation; the waveform policies of `wave_augment` -- SpeedPerturb, NoiseReverb
    -- when given and SpecAugment when `augment` is: training batches only), frame counts, padded labels and label lengths of one batch."""
    n = [len(utts[i][0]) for i in idx]
    wave = np.zeros((len(idx), max(n)), dtype=np.int16)
    lab_len = [len(utts[i][1]) for i in idx]
    labels = np.zeros((len(idx), max(lab_len)), dtype=np.int32)
    for r, i in enumerate(idx):
        wave[r, :n[r]] = utts[i][0]
        labels[r, :lab_len[r]] = utts[i][1]
    x, frame_lengths = quaternion_fbank(torch.from_numpy(wave).to(dev), torch.tensor(n, dtype=torch.int32), normalize='utterance',
                                        dtype=dtype, augment=augment, wave_augment=wave_augment)
    labels = torch.from_numpy(labels).to(dev)
    label_length = torch.tensor(lab_len, dtype=torch.int32, device=dev)[:, None]
    return x, frame_lengths[:, None], labels, label_length


def device_batch(parts, dtype, augment=None, wave_augment=None):
    """to_device for a batch that a DeviceCorpus gathered (parts: what DeviceCorpus.batch / next_batch return): only the front end
    is left to do."""
    wave, lengths, labels, label_length = parts[:4]
    x, frame_lengths = quaternion_fbank(wave, lengths, normalize='utterance', dtype=dtype, augment=augment, wave_augment=wave_augment)
    return x, frame_lengths[:, None], labels, label_length


def reference_starts(utts, idx, width, dev):
    """(B, width) int64 start samples of the batch's phones (load_split(boundaries=True)), padded with -1."""
    ref = np.full((len(idx), width), -1, dtype=np.int64)
    for r, i in enumerate(idx):
        ref[r, :len(utts[i][2])] = utts[i][2]
    return torch.from_numpy(ref).to(dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--timit', required=True, help='corpus root holding TRAIN/ and TEST/')
    ap.add_argument('--steps', type=int, default=1000)
    ap.add_argument('--batch', type=int, default=32, help='utterances per step')
    ap.add_argument('--layers', type=int, default=10)
    ap.add_argument('--filters', type=int, default=32)
    ap.add_argument('--aact', default='none', choices=['none', 'prelu'])
    ap.add_argument('--dropout', type=float, default=0.3)
    ap.add_argument('--l2', type=float, default=1e-5)
    ap.add_argument('--lr', type=float, default=5e-4)
    ap.add_argument('--eval-every', type=int, default=100, help='held-out CTC cost and PER every N steps (0: off)')
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--lm-order', type=int, default=0, choices=[0, 1, 2, 3], help='phone n-gram LM order for the beam search (0: off)')
    ap.add_argument('--lm-weight', type=float, default=0.5)
    ap.add_argument('--insertion-bonus', type=float, default=0.0)
    ap.add_argument('--beam-width', type=int, default=16, help='beam width of the LM comparison')
    ap.add_argument('--clipnorm', type=float, default=0.0, help='global gradient-norm clip, as Adam(clipnorm=) in Keras (0: off)')
    ap.add_argument('--clipvalue', type=float, default=0.0, help='element-wise gradient clamp behind it, as Adam(clipvalue=) (0: off)')
    ap.add_argument('--dtype', default='bfloat16', choices=['bfloat16', 'float16'], help='activation dtype')
    ap.add_argument('--dynamic-loss-scale', action='store_true',
                    help='loss scale on the device, starting at 2^12: halved on an overflowing (skipped) step, doubled after 2000 good ones')
    ap.add_argument('--specaug', action='store_true', help='SpecAugment on the training batches (never on evaluation batches)')
    ap.add_argument('--time-warp', type=int, default=5, help='SpecAugment: a frame moves by up to this many frames (0: no warp)')
    ap.add_argument('--freq-masks', type=int, default=2)
    ap.add_argument('--freq-width', type=int, default=8, help='largest frequency mask, rows of 41')
    ap.add_argument('--time-masks', type=int, default=2)
    ap.add_argument('--time-width', type=int, default=25, help='largest time mask, frames ...')
    ap.add_argument('--time-ratio', type=float, default=0.2, help='... and at most this share of the utterance')
    ap.add_argument('--speed-perturb', action='store_true',
                    help='speed and volume perturbation of the training waveforms (never of evaluation batches); labels are unchanged')
    ap.add_argument('--speeds', type=parse_speeds, default=((9, 10), (1, 1), (11, 10)),
                    help='speed perturbation: comma-separated speeds, each taken as a fraction with a denominator <= 32')
    ap.add_argument('--volume', type=parse_volume, default=(1.0, 1.0), help='speed perturbation: LO,HI of the linear gain drawn per utterance')
    ap.add_argument('--noise-reverb', action='store_true',
                    help='reverberation and additive noise on the training waveforms (never on evaluation batches), behind --speed-perturb')
    ap.add_argument('--rir-dir', default=None, help='noise-reverb: directory of room impulse responses (default: synthetic ones)')
    ap.add_argument('--noise-dir', default=None, help='noise-reverb: directory of noise recordings (default: synthetic ones)')
    ap.add_argument('--rir-prob', type=float, default=0.5, help='noise-reverb: probability of reverberating an utterance')
    ap.add_argument('--noise-prob', type=float, default=0.5, help='noise-reverb: probability of adding noise to an utterance')
    ap.add_argument('--snr', type=parse_volume, default=(5.0, 20.0), help='noise-reverb: LO,HI of the signal-to-noise ratio in dB')
    ap.add_argument('--align-eval', action='store_true',
                    help='at every evaluation, force-align the held-out batch and print the share of boundaries within 20 ms of the .PHN ones')
    ap.add_argument('--confusions', type=int, default=0, metavar='N',
                    help='at every evaluation, print %%cor / %%sub / %%del / %%ins of all held-out batches and the top N confusion pairs (0 = off)')
    ap.add_argument('--warmup', type=int, default=0, metavar='N', help='linear warm-up of the learning rate over the first N steps (0: off)')
    ap.add_argument('--lr-decay', default='none', choices=['none', 'inverse-time', 'exponential', 'cosine', 'inv-sqrt'],
                    help='learning-rate schedule behind the warm-up, evaluated on the device (cosine: over --steps)')
    ap.add_argument('--decay-steps', type=int, default=1000, help='exponential: steps per factor of --decay-rate')
    ap.add_argument('--decay-rate', type=float, default=None,
                    help='inverse-time: the decay= of Keras\' Adam (default 1e-4); exponential: the factor per --decay-steps (default 0.5)')
    ap.add_argument('--lr-floor', type=float, default=0.0, help='cosine: share of --lr the schedule ends at')
    ap.add_argument('--ema', type=float, default=0.0, metavar='D',
                    help='keep an exponential moving average of the weights with decay D and evaluate with it (0: off)')
    ap.add_argument('--halve-on-plateau', action='store_true', help='halve the rate when the held-out PER(39) stops improving')
    ap.add_argument('--plateau-patience', type=int, default=0, help='evaluations without improvement that are tolerated')
    ap.add_argument('--checkpoint', default=None, metavar='PATH', help='write a checkpoint at every evaluation')
    ap.add_argument('--resume', default=None, metavar='PATH', help='continue from a checkpoint written by --checkpoint')
    ap.add_argument('--device-corpus', action='store_true',
                    help='keep TRAIN and TEST in device memory, shuffle epochs and assemble every batch on the device')
    ap.add_argument('--model', default='qcnn', choices=['qcnn', 'qlstm', 'qtransformer', 'qconformer', 'qtransducer'],
                    help='qcnn: the reference model; qlstm: a stack of quaternion LSTM layers; qtransformer: quaternion self-attention encoder blocks; '
                         'qconformer: Conformer blocks (self-attention + gated depthwise quaternion convolution); '
                         'qtransducer: one of the three sequence encoders (--encoder) under the transducer loss')
    ap.add_argument('--encoder', default='qlstm', choices=['qlstm', 'qtransformer', 'qconformer'], help='qtransducer: the encoder')
    ap.add_argument('--pred-units', type=int, default=256, help='qtransducer: width of the prediction network (a multiple of 4)')
    ap.add_argument('--joint-units', type=int, default=512, help='qtransducer: width of the joint network (a multiple of 4)')
    ap.add_argument('--rnn-layers', type=int, default=4, help='qlstm: number of bidirectional QuaternionLSTM layers')
    ap.add_argument('--rnn-units', type=int, default=1024, help='qlstm: units per direction (a multiple of 64 runs on the matrix cores)')
    ap.add_argument('--layer-norm', action='store_true', help='qlstm: a quaternion layer normalisation behind every recurrent layer')
    ap.add_argument('--tf-layers', type=int, default=6, help='qtransformer: number of encoder blocks')
    ap.add_argument('--tf-units', type=int, default=512, help='qtransformer: model width (64 or 128 per head runs the attention on the matrix cores)')
    ap.add_argument('--tf-heads', type=int, default=8, help='qtransformer: attention heads (must divide tf-units / 4)')
    ap.add_argument('--tf-ff', type=int, default=2048, help='qtransformer: width of the feed-forward layer')
    ap.add_argument('--conv-kernel', type=int, default=15, help='qconformer: taps of the depthwise convolution over time (1 .. 31)')
    args = ap.parse_args()
    transducer = args.model == 'qtransducer'
    body = args.encoder if transducer else args.model          # which encoder / CTC model is built
    if args.layer_norm and body != 'qlstm':
        ap.error('--layer-norm needs --model qlstm (or --model qtransducer --encoder qlstm)')
    if transducer and (args.lm_order > 0 or args.align_eval or args.confusions > 0):
        ap.error('--model qtransducer decodes greedily: --lm-order, --align-eval and --confusions belong to the CTC models')
    dev = torch.device('cuda:0')
    torch.cuda.set_device(dev)
    dtype = getattr(torch, args.dtype)

    train = load_split(find_split(args.timit, 'TRAIN'))
    test = load_split(find_split(args.timit, 'TEST'), boundaries=args.align_eval)
    if not train:
        raise SystemExit('%s: no WAV / PHN pairs under TRAIN/' % args.timit)
    print('%d training and %d held-out utterances' % (len(train), len(test)))
    batches = length_batches(train, args.batch)
    held_out_all = length_batches(test, args.batch) if test else []
    held_out = held_out_all[0] if test else None
    class_map = torch.from_numpy(timit_61_to_39_class_map())
    corpus = sampler = test_corpus = None
    if args.device_corpus:
        corpus = DeviceCorpus([u[0] for u in train], [u[1] for u in train], device=dev)
        sampler = EpochSampler(corpus.wave_len, args.batch, seed=args.seed & 0xFFFFFFFF)
        if test:
            test_corpus = DeviceCorpus([u[0] for u in test], [u[1] for u in test], aux=[u[2] for u in test] if args.align_eval else None,
                                       device=dev)
        print('device-resident corpus: %.1f MB of waveforms, %d batches per epoch'
              % (2e-6 * (corpus.arrays.wave_pack.numel() + (test_corpus.arrays.wave_pack.numel() if test_corpus is not None else 0)),
                 sampler.num_batches))

    def held_out_batch(idx):
        """(features, frame counts, labels, label lengths, reference start samples or None) of a held-out batch."""
        if test_corpus is None:
            starts = reference_starts(test, idx, max(len(test[i][1]) for i in idx), dev) if args.align_eval else None
            return to_device(test, idx, dev, dtype) + (starts,)
        parts = test_corpus.batch(idx)
        return device_batch(parts, dtype) + (parts[4].to(torch.int64) if args.align_eval else None,)
    lm = None
    if args.lm_order > 0:
        lm = NgramLM.estimate([u[1] for u in train], len(TIMIT_PHONES_61), args.lm_order)
        ppl = lm.perplexity([u[1] for u in test]) if test else float('nan')
        print('%d-gram phone LM from %d TRAIN transcripts: held-out perplexity %.3f' % (args.lm_order, len(train), ppl))

    d = types.SimpleNamespace(num_layers=args.layers, start_filter=args.filters, act='relu', aact=args.aact, dropout=args.dropout,
                              l2=args.l2, model='quaternion', quat_init='quaternion')
    np.random.seed(args.seed)
    torch.manual_seed(args.seed)
    if body == 'qlstm':
        from qcnn_amd.models import TimitQLSTM
        model = TimitQLSTM(num_layers=args.rnn_layers, units=args.rnn_units, bidirectional=True, dropout=args.dropout, l2=args.l2,
                           layer_norm=args.layer_norm)
        print('model: %d bidirectional quaternion LSTM layers of %d units%s' % (args.rnn_layers, args.rnn_units,
                                                                                ', layer normalisation' if args.layer_norm else ''))
    elif body == 'qtransformer':
        from qcnn_amd.models import TimitQTransformer
        model = TimitQTransformer(num_layers=args.tf_layers, units=args.tf_units, heads=args.tf_heads, ff_units=args.tf_ff, dropout=args.dropout,
                                  l2=args.l2)
        print('model: %d quaternion transformer encoder blocks of %d units, %d heads, feed-forward %d'
              % (args.tf_layers, args.tf_units, args.tf_heads, args.tf_ff))
    elif body == 'qconformer':
        from qcnn_amd.models import TimitQConformer
        model = TimitQConformer(num_layers=args.tf_layers, units=args.tf_units, heads=args.tf_heads, ff_units=args.tf_ff,
                                kernel_size=args.conv_kernel, dropout=args.dropout, l2=args.l2)
        print('model: %d quaternion Conformer blocks of %d units, %d heads, feed-forward %d, %d-tap depthwise convolution'
              % (args.tf_layers, args.tf_units, args.tf_heads, args.tf_ff, args.conv_kernel))
    else:
        model, _ = getTimitModel2D(d)
    if transducer:
        from qcnn_amd.models import TimitQTransducer
        model = TimitQTransducer(model, pred_units=args.pred_units, joint_units=args.joint_units, dropout=args.dropout, l2=args.l2)
        print('transducer: the model above as encoder, prediction network of %d units, joint of %d units' % (args.pred_units, args.joint_units))
    x0 =(to_device(train, batches[0][:1], dev, dtype) if corpus is None else device_batch(corpus.batch(batches[0][:1]), dtype))[0]
    with torch.no_grad():
        model(x0)                                                 # build-on-first-call, like Keras
    model.to(dev)
    model.train()
    flat = dp.FlatParams([p for p in model.parameters() if p.requires_grad])   # the l2 terms come through training_loss
    m, v = torch.zeros_like(flat.param), torch.zeros_like(flat.param)
    rng = np.random.RandomState(args.seed)
    augment = None
    if args.specaug:
        augment = SpecAugment(time_warp=args.time_warp, freq_masks=args.freq_masks, freq_width=args.freq_width, time_masks=args.time_masks,
                              time_width=args.time_width, time_ratio=args.time_ratio, seed=args.seed & 0xFFFFFFFF)
    wave_augment = None
    if args.speed_perturb:
        wave_augment = SpeedPerturb(speeds=args.speeds, gain=args.volume, seed=args.seed & 0xFFFFFFFF)
    if args.noise_reverb:
        rirs = [np.asarray(h, dtype=np.float64) for h in read_audio_dir(args.rir_dir, 'rir')] if args.rir_dir else synthetic_rirs(32, seed=args.seed & 0xFFFFFFFF)
        noises = read_audio_dir(args.noise_dir, 'noise') if args.noise_dir else synthetic_noises(8, 64000, seed=args.seed & 0xFFFFFFFF)
        noise_reverb = NoiseReverb(rirs=F.prepare_rirs(rirs, device=dev), noises=F.prepare_noises(noises, device=dev),
                                   rir_prob=args.rir_prob, noise_prob=args.noise_prob, snr=args.snr, seed=args.seed & 0xFFFFFFFF)
        wave_augment = noise_reverb if wave_augment is None else (wave_augment, noise_reverb)
    # clipping / float16 / dynamic scaling: the guarded step (qcnn_amd.training.GradGuard).  Norm, overflow check, clip and scale
    # update all happen on the device, and so does the step count (a skipped step does not advance it).
    guard = None
    if args.clipnorm > 0 or args.clipvalue > 0 or args.dynamic_loss_scale or dtype == torch.float16:
        guard = GradGuard(dev, clipnorm=args.clipnorm, clipvalue=args.clipvalue, dynamic=args.dynamic_loss_scale,
                          loss_scale=2.0 ** 12 if dtype == torch.float16 or args.dynamic_loss_scale else 1.0)
        step_dev = torch.zeros(1, dtype=torch.int32, device=dev)
    # warm-up / decay / averaged weights / plateau halving / checkpoints: the scheduled step (qcnn_amd.training.ScheduledAdam).  The
    # rate is formed on the device from the step counter; the guard, when there is one, runs in front of it.
    opt = plateau = None
    first_step = 1
    if (args.warmup > 0 or args.lr_decay != 'none' or args.ema > 0 or args.halve_on_plateau or args.checkpoint or args.resume):
        kind = 'constant' if args.lr_decay == 'none' else args.lr_decay
        rate = args.decay_rate if args.decay_rate is not None else {'inverse-time': 1e-4, 'exponential': 0.5}.get(kind, 1.0)
        schedule = LRSchedule(args.lr, kind, warmup_steps=args.warmup, total_steps=args.steps if kind == 'cosine' else 0, decay_steps=args.decay_steps, rate=rate,
                              floor=args.lr_floor)
        opt = ScheduledAdam(flat.param, flat.grad, schedule, guard=guard, ema_decay=args.ema)
        plateau = ReduceOnPlateau(patience=args.plateau_patience) if args.halve_on_plateau else None
        policies = [q for q in (augment,) + (wave_augment if isinstance(wave_augment, tuple) else (wave_augment,)) + (sampler,) if q is not None]
        if args.resume:
            extra = load_checkpoint(args.resume, model, opt, policies)
            first_step = extra['step'] + 1
            rng.set_state(('MT19937', extra['rng_keys'].numpy().astype(np.uint32), extra['rng_pos'], 0, 0.0))
            if plateau is not None and extra['plateau'] is not None:
                plateau.load_state_dict(extra['plateau'])
            print('resumed from %s at step %d (%d applied)' % (args.resume, extra['step'], opt.stats()['step']))
    eval_weights = opt.averaged if opt is not None and args.ema > 0 else contextlib.nullcontext
    for step in range(first_step, args.steps + 1):
        if sampler is None:
            x, il, labels, ll = to_device(train, batches[rng.randint(len(batches))], dev, dtype, augment, wave_augment)
        else:
            epoch = sampler.epoch                                     # (the host cursor: no device read)
            x, il, labels, ll = device_batch(corpus.next_batch(sampler), dtype, augment, wave_augment)
        if guard is None:
            loss = model.training_loss(x, labels, il, ll)
        else:
            loss = model.training_loss(x, labels, il, ll, loss_scale=guard.loss_scale)
        loss.backward()
        if opt is not None:
            opt.step(zero_grad=True)
        elif guard is None:
            F.adam_step(flat.param, flat.grad, m, v, step, lr=args.lr, zero_grad=True)
        else:
            guard.step(flat.param, flat.grad, m, v, step_dev, lr=args.lr, zero_grad=True)
        if step == 1 or step % 50 == 0 or step == args.steps:
            line = 'step %5d  loss %.4f' % (step, float(loss)) + ('  epoch %d' % epoch if sampler is not None else '')
            if guard is not None:
                s = guard.stats()                                     # (the one host read of the guard, at log lines only)
                line += '  grad norm %.4g  loss scale %g  skipped %d' % (s['last_norm'], s['scale'], s['skipped_steps'])
            if opt is not None:
                s = opt.stats()                                       # (likewise)
                line += '  lr %.4g' % s['last_lr'] + ('  ema decay %.4g' % s['last_ema_decay'] if args.ema > 0 else '')
            print(line)
        if not (args.eval_every > 0 and step % args.eval_every == 0 and held_out is not None):
            continue
        with eval_weights():                                          # --ema: param and ema change places for the evaluation
            xe, ile, le, lle, starts = held_out_batch(held_out)
            res = model.evaluate(xe, le, ile, lle, class_map=class_map)
            print('step %5d  held-out %s cost %.4f  PER(39) %.4f (%d / %d)%s'
                  % (step, 'transducer' if transducer else 'ctc', float(res.loss), float(res.per), int(res.errors), int(res.symbols),
                     '  [averaged weights, ema %g]' % args.ema if opt is not None and args.ema > 0 else ''))
            if args.align_eval:
                ali = model.align(xe, le, ile, lle)
                hits, total, share = layers.boundary_agreement(frames_to_samples(ali.starts), starts, lle, tolerance=int(round(0.02 * 16000)))
                print('step %5d  held-out boundary agreement within 20 ms %.4f (%d / %d)' % (step, float(share), int(hits), int(total)))
            if args.confusions > 0:
                confusion = torch.zeros((len(TIMIT_PHONES_39) + 1,) * 2, dtype=torch.int32, device=dev)
                parts = []
                for idx in held_out_all:                              # one matrix, accumulated on the device over the batches
                    xb, ilb, lb, llb = held_out_batch(idx)[:4]
                    parts.append(model.error_breakdown(xb, lb, ilb, llb, class_map=class_map, confusion=confusion))
                c, s, d, i = (sum(int(getattr(p, f)) for p in parts) for f in ('correct', 'substitutions', 'deletions', 'insertions'))
                n = max(c + s + d, 1)
                print('step %5d  held-out %%cor %.2f  %%sub %.2f  %%del %.2f  %%ins %.2f  (%d reference phones, %d batches)'
                      % (step, 100.0 * c / n, 100.0 * s / n, 100.0 * d / n, 100.0 * i / n, c + s + d, len(parts)))
                for r, h, count in layers.top_confusions(confusion, args.confusions, TIMIT_PHONES_39):
                    print('step %5d  confusion %-5s -> %-5s %d' % (step, r, h, count))
            if lm is not None:
                plain = model.evaluate(xe, le, ile, lle, greedy=False, beam_width=args.beam_width, class_map=class_map)
                fused = model.evaluate(xe, le, ile, lle, greedy=False, beam_width=args.beam_width, class_map=class_map, lm=lm,
                                       lm_weight=args.lm_weight, insertion_bonus=args.insertion_bonus)
                print('step %5d  held-out beam %d PER(39) without LM %.4f  with %d-gram LM %.4f'
                      % (step, args.beam_width, float(plain.per), args.lm_order, float(fused.per)))
        if plateau is not None:
            opt.set_lr_scale(plateau.update(float(res.per)))
            print('step %5d  learning-rate scale %g' % (step, plateau.scale))
        if args.checkpoint:
            state = rng.get_state()
            save_checkpoint(args.checkpoint, model, opt, policies,
                            extra=dict(step=step, plateau=plateau.state_dict() if plateau is not None else None,
                                       rng_keys=torch.from_numpy(state[1].astype(np.int64)), rng_pos=int(state[2])))


if __name__ == '__main__':
    main()
