"""Acoustic front end: waveforms -> the TIMIT model's channels_first quaternion input (B, 4, nfilt + 1, T).

The reference defines the input only by its shape, Input(shape=(4, 41, None)) (models/interspeech_model.py:81), and ships no feature
code.  The recipe here is python_speech_features' `logfbank` + `delta` with nfilt = 40: 25 ms frames every 10 ms, 40 log mel
filter-bank energies plus the log frame energy (the 41 rows), and the quaternion components r = static, i / j / k = first / second /
third time derivative.  Everything runs on the device in fp32 (csrc/qk_fbank.hip); semantics and limits: include/qk.h, "Acoustic front
end".  The input is data, so there is no autograd.
"""
import decimal
import math

import numpy as np
import torch

from . import _lib as L
from . import functional as F

WINDOWS = {'rect': L.QK_WINDOW_RECT, 'hamming': L.QK_WINDOW_HAMMING}
NORMALIZE = {None: L.QK_FBANK_NORM_NONE, 'utterance': L.QK_FBANK_NORM_UTTERANCE}


def _round_half_up(x):
    return int(decimal.Decimal(x).quantize(decimal.Decimal('1'), rounding=decimal.ROUND_HALF_UP))


def frame_geometry(sample_rate=16000, winlen=0.025, winstep=0.01):
    """(frame length, frame step) in samples: round-half-up of winlen / winstep times the rate (400 / 160 at 16 kHz)."""
    return _round_half_up(winlen * sample_rate), _round_half_up(winstep * sample_rate)


def num_frames(samples, sample_rate=16000, winlen=0.025, winstep=0.01):
    """Frames of an utterance of `samples` samples: 1 up to one frame length, else 1 + ceil((samples - L) / S)."""
    frame_len, frame_step = frame_geometry(sample_rate, winlen, winstep)
    if samples <= frame_len:
        return 1
    return 1 + int(math.ceil((1.0 * samples - frame_len) / frame_step))


def frames_to_samples(frames, sample_rate=16000, winlen=0.025, winstep=0.01, position='centre'):
    """Frame indices -> sample positions, in the geometry of frame_geometry: frame t starts at sample t * frame_step and covers
    frame_len samples, so its centre is t * frame_step + frame_len // 2.  position='centre' (the default) gives the centre -- the
    sample a frame-level boundary (functional.ctc_forced_align's starts / ends) stands for, and the inverse of samples_to_frames --
    position='start' the first sample.  A negative frame index (the alignment's -1 for "none") gives -1.  `frames` is an int, an
    integer numpy array or an integer torch tensor (device tensors stay on the device); the result has the same kind."""
    if position not in ('centre', 'start'):
        raise ValueError("frames_to_samples: position must be 'centre' or 'start', got %r" % (position,))
    frame_len, frame_step = frame_geometry(sample_rate, winlen, winstep)
    offset = frame_len // 2 if position == 'centre' else 0
    if torch.is_tensor(frames):
        f = frames.long()
        return torch.where(f < 0, torch.full_like(f, -1), f * frame_step + offset)
    if isinstance(frames, np.ndarray):
        f = frames.astype(np.int64)
        return np.where(f < 0, -1, f * frame_step + offset)
    return -1 if frames < 0 else int(frames) * frame_step + offset


def samples_to_frames(samples, sample_rate=16000, winlen=0.025, winstep=0.01):
    """Sample positions -> frame indices, in the geometry of frame_geometry: a sample maps to the frame whose CENTRE
    (t * frame_step + frame_len // 2) is nearest; a sample exactly half-way between two centres goes to the LOWER frame; the result
    is clamped to >= 0 (samples in front of the first centre belong to frame 0).  It is not clamped from above: the caller knows the
    utterance's frame count.  samples_to_frames(frames_to_samples(t)) == t for every t >= 0.  `samples` is an int, an integer numpy
    array or an integer torch tensor; the result has the same kind."""
    frame_len, frame_step = frame_geometry(sample_rate, winlen, winstep)
    # ceil((d - step / 2) / step) with d = sample - centre of frame 0, in integers: -floor((step - 2 d) / (2 step))
    if torch.is_tensor(samples):
        d = samples.long() - frame_len // 2
        return torch.clamp(-torch.div(frame_step - 2 * d, 2 * frame_step, rounding_mode='floor'), min=0)
    if isinstance(samples, np.ndarray):
        d = samples.astype(np.int64) - frame_len // 2
        return np.maximum(-((frame_step - 2 * d) // (2 * frame_step)), 0)
    d = int(samples) - frame_len // 2
    return max(-((frame_step - 2 * d) // (2 * frame_step)), 0)


def _mel_bins(nfilt, nfft, sample_rate, lowfreq, highfreq):
    lo, hi = (2595 * np.log10(1 + f / 700.) for f in (lowfreq, highfreq))
    mel = np.linspace(lo, hi, nfilt + 2)
    return np.floor((nfft + 1) * (700 * (10 ** (mel / 2595.0) - 1)) / sample_rate)


def mel_filterbank(nfilt=40, nfft=512, sample_rate=16000, lowfreq=0, highfreq=None):
    """(nfilt, nfft // 2 + 1) float64: python_speech_features' get_filterbanks.  nfilt + 2 points evenly spaced in mel
    (2595 log10(1 + f / 700)) from lowfreq to highfreq (default sample_rate / 2) are floored to FFT bins b; filter j rises from 0 at
    b[j] to 1 at b[j+1] and falls back to 0 at b[j+2].  The device kernel builds its tables from the same bins."""
    b = _mel_bins(nfilt, nfft, sample_rate, lowfreq, highfreq if highfreq is not None else sample_rate / 2)
    fb = np.zeros((nfilt, nfft // 2 + 1))
    for j in range(nfilt):
        lo, mid, hi = b[j], b[j + 1], b[j + 2]
        i = np.arange(int(lo), int(mid))
        fb[j, i] = (i - lo) / (mid - lo)
        i = np.arange(int(mid), int(hi))
        fb[j, i] = (hi - i) / (hi - mid)
    return fb


def quaternion_fbank(wave, lengths=None, sample_rate=16000, winlen=0.025, winstep=0.01, nfilt=40, nfft=512, lowfreq=0, highfreq=None,
                     preemph=0.97, window='rect', delta_n=2, append_energy=True, normalize=None, dtype=torch.float32, augment=None,
                     wave_augment=None):
    """Quaternion filter-bank features of a batch of waveforms, on the device.

    wave: (B, n_max) or (n_max,) int16 / float32 CUDA tensor; lengths: samples per utterance (B,) (default n_max each; clamped to
    [0, n_max]).  Per utterance: pre-emphasis, frames of winlen every winstep seconds (zero-padded), the window ('rect' or 'hamming'),
    |rfft(frame, nfft)|^2 / nfft, nfilt log mel energies (+ the log frame energy when append_energy), exact zeros floored to float64
    eps; then delta, delta^2, delta^3 over delta_n frames (python_speech_features.delta), edge-clamped at the utterance's own frames.
    normalize='utterance' standardises every (utterance, plane, row) over its valid frames.

    Returns (x, frame_lengths): x (B, 4, nfilt [+ 1], T) in `dtype` with T = num_frames(n_max) and frames t >= frame_lengths[b]
    zero; frame_lengths (B,) int32, ready to serve as the CTC input_length.  Limits: nfft a power of two in [256, 1024] and at least
    the frame length, nfilt <= 128, 1 <= delta_n <= 4.

    augment: a SpecAugment policy (training batches only).  The features are then computed in float32, after any normalisation,
    augmented with the frame lengths as the utterance lengths, and rounded once to `dtype`; after normalize='utterance' a fill of 0
    is the per-row mean.  None (the default): no augmentation, the calls are exactly those of the plain front end.

    wave_augment: a SpeedPerturb policy (training batches only).  The waveforms are perturbed first, and the front end runs on the
    perturbed float32 waveforms and THEIR lengths: T = num_frames of the perturbed batch's width (wider than n_max when the policy has
    a speed below 1), frame_lengths those of the perturbed utterances.  Labels are unchanged.  It combines with `augment`.  None (the
    default): the calls are exactly those of the plain front end.  Also a NoiseReverb policy (reverberation and additive noise; it
    keeps the lengths), or a tuple / list of policies applied in order -- the usual recipe is (SpeedPerturb, NoiseReverb)."""
    if wave_augment is None or isinstance(wave_augment, (SpeedPerturb, NoiseReverb)):
        wave_augments = () if wave_augment is None else (wave_augment,)
    elif isinstance(wave_augment, (tuple, list)) and all(isinstance(a, (SpeedPerturb, NoiseReverb)) for a in wave_augment):
        wave_augments = tuple(wave_augment)
    else:
        raise TypeError('quaternion_fbank: wave_augment must be a SpeedPerturb, a NoiseReverb, a tuple / list of them or None, got %r'
                        % (wave_augment,))
    if augment is not None and not isinstance(augment, SpecAugment):
        raise TypeError('quaternion_fbank: augment must be a SpecAugment or None, got %r' % (augment,))
    if window not in WINDOWS:
        raise ValueError('quaternion_fbank: window must be one of %s, got %r' % (sorted(WINDOWS), window))
    if normalize not in NORMALIZE:
        raise ValueError("quaternion_fbank: normalize must be None or 'utterance', got %r" % (normalize,))
    frame_len, frame_step = frame_geometry(sample_rate, winlen, winstep)
    if frame_len < 1 or frame_step < 1:
        raise ValueError('quaternion_fbank: winlen and winstep must give at least one sample (got %d / %d)' % (frame_len, frame_step))
    if nfft not in (256, 512, 1024) or nfft < frame_len:
        raise ValueError('quaternion_fbank: nfft %r must be 256, 512 or 1024 and at least the frame length (%d samples)'
                         % (nfft, frame_len))
    if not 1 <= nfilt <= L.QK_FBANK_MAX_FILT:
        raise ValueError('quaternion_fbank: nfilt %r outside 1 .. %d' % (nfilt, L.QK_FBANK_MAX_FILT))
    if not 1 <= delta_n <= 4:
        raise ValueError('quaternion_fbank: delta_n %r outside 1 .. 4' % (delta_n,))
    highfreq = sample_rate / 2 if highfreq is None else highfreq
    if not 0 <= lowfreq < highfreq <= sample_rate / 2:
        raise ValueError('quaternion_fbank: need 0 <= lowfreq < highfreq <= sample_rate / 2 (got %r, %r)' % (lowfreq, highfreq))
    if not math.isfinite(preemph):
        raise ValueError('quaternion_fbank: preemph must be finite')
    if not torch.is_tensor(wave) or not wave.is_cuda:
        raise RuntimeError('quaternion_fbank: got a CPU tensor. The acoustic front end runs only on the MI355X HIP path '
                           '(libqk_hip.so); there is no CPU fallback.')
    if wave.dtype not in (torch.int16, torch.float32):
        raise TypeError('quaternion_fbank: waveforms must be int16 or float32, got %s' % wave.dtype)
    if wave.dim() == 1:
        wave = wave[None]
    if wave.dim() != 2 or min(wave.shape) < 1:
        raise ValueError('quaternion_fbank: wave must be a non-empty (B, samples) tensor, got shape %s' % (tuple(wave.shape),))
    b, n_max = wave.shape
    if lengths is None:
        lengths = torch.full((b,), n_max, dtype=torch.int32, device=wave.device)
    else:
        lengths = torch.as_tensor(lengths)
        if lengths.numel() != b:
            raise ValueError('quaternion_fbank: lengths must have B = %d entries, got %d' % (b, lengths.numel()))
        lengths = lengths.reshape(-1).to(device=wave.device, dtype=torch.int32)
    for policy in wave_augments:
        wave, lengths = policy(wave, lengths)
        n_max = wave.shape[1]
    bins = _mel_bins(nfilt, nfft, sample_rate, lowfreq, highfreq).astype(np.int64).tolist()
    frames = num_frames(n_max, sample_rate, winlen, winstep)
    if augment is None:
        return F.fbank_quaternion(wave, lengths, frames, frame_len, frame_step, nfft, preemph, WINDOWS[window], bins, append_energy,
                                  delta_n, NORMALIZE[normalize], dtype)
    if dtype not in (torch.float32, torch.bfloat16, torch.float16):
        raise TypeError('quaternion_fbank: unsupported output dtype %s (float32, bfloat16, float16)' % dtype)
    x, flen = F.fbank_quaternion(wave, lengths, frames, frame_len, frame_step, nfft, preemph, WINDOWS[window], bins, append_energy,
                                 delta_n, NORMALIZE[normalize], torch.float32)
    return augment(x, flen, dtype=dtype), flen


class SpecAugment(object):
    """A SpecAugment policy (Park et al., 2019) for the quaternion filter-bank input, with its own device counter.

        aug = SpecAugment(seed=args.seed)
        x, il = quaternion_fbank(wave, lengths, normalize='utterance', dtype=torch.bfloat16, augment=aug)     # training batches only

    Per utterance: one time warp that moves a frame by up to time_warp frames, freq_masks masks of up to freq_width rows and
    time_masks masks of up to min(time_width, time_ratio * frames) frames, written as `fill` -- one launch (functional.spec_augment;
    semantics: include/qk.h, "SpecAugment").  A time-frequency cell is one quaternion, so all four planes get the same warp and the
    same masks; the derivative planes are warped like the static plane and NOT rescaled by the warp's local slope.

    The defaults are the paper's LibriSpeech policy scaled to 41 rows and TIMIT-length utterances (W 80 -> 5, F 27 of 80 -> 8 of
    41, T 100 -> 25, two masks of each kind, p = 0.2).  Nobody has measured a phone error rate with them: treat them as a starting
    point, not as tuned values.

    The draws are a hash of (seed, counter, utterance index): bit-repeatable from the seed.  __call__ advances the counter with a
    device op behind the kernel, so a captured graph draws new masks on every replay and nothing is read on the host.
    Data-parallel ranks must pass DIFFERENT seeds, or every rank masks its utterance b like every other's; seed and utterance index
    enter the hash as a sum, so keep the seeds at least a batch apart (e.g. seed + 65536 * rank).
    state_dict() / load_state_dict() carry the seed and the counter (reading the counter synchronises)."""

    def __init__(self, time_warp=5, freq_masks=2, freq_width=8, time_masks=2, time_width=25, time_ratio=0.2, fill=0.0, seed=0):
        F._specaug_policy('SpecAugment', time_warp, freq_masks, freq_width, time_masks, time_width, time_ratio, fill, seed)
        self.policy = dict(time_warp=time_warp, freq_masks=freq_masks, freq_width=freq_width, time_masks=time_masks,
                           time_width=time_width, time_ratio=float(time_ratio), fill=float(fill), seed=seed)
        self._counter = None            # one int32 on the device of the first call; the kernel reads its 32 bits as unsigned
        self._pending = 0               # counter value to start from (load_state_dict before the first call)
        self.last_plan = None

    @property
    def seed(self):
        return self.policy['seed']

    def _counter_on(self, device):
        if self._counter is None:
            v = self._pending - (1 << 32) if self._pending >= 1 << 31 else self._pending
            self._counter = torch.full((1,), v, dtype=torch.int32, device=device)
        elif self._counter.device != device:
            raise ValueError('SpecAugment: this policy\'s counter lives on %s, the input on %s' % (self._counter.device, device))
        return self._counter

    def __call__(self, x, lengths, dtype=None):
        """Augmented copy of x (B, planes, rows, T) in `dtype` (default x.dtype); the plan of the call is kept in .last_plan."""
        if not torch.is_tensor(x) or not x.is_cuda:
            raise RuntimeError('SpecAugment: got a CPU tensor. SpecAugment runs only on the MI355X HIP path (libqk_hip.so); there is '
                               'no CPU fallback.')
        counter = self._counter_on(x.device)
        out, self.last_plan = F.spec_augment(x, lengths, counter=counter, dtype=dtype, return_plan=True, **self.policy)
        counter.add_(1)                 # wraps mod 2^32, like the kernel's key
        return out

    def state_dict(self):
        counter = self._pending if self._counter is None else int(self._counter.item()) & 0xFFFFFFFF
        return {'seed': self.policy['seed'], 'counter': counter}

    def load_state_dict(self, d):
        """Takes what state_dict() gave; checked on the host before anything is written."""
        seed, counter = d['seed'], d['counter']
        for name, v in (('seed', seed), ('counter', counter)):
            if isinstance(v, bool) or not isinstance(v, int) or not 0 <= v <= 0xFFFFFFFF:
                raise ValueError('SpecAugment.load_state_dict: %s must be an integer in [0, 2^32), got %r' % (name, v))
        self.policy['seed'] = seed
        if self._counter is None:
            self._pending = counter
        else:
            self._counter.fill_(counter - (1 << 32) if counter >= 1 << 31 else counter)


class SpeedPerturb(object):
    """A speed and volume perturbation policy (Ko et al., 2015) for waveforms, with its own device counter.

        sp = SpeedPerturb(seed=args.seed)
        x, il = quaternion_fbank(wave, lengths, normalize='utterance', dtype=torch.bfloat16, wave_augment=sp)   # training batches only

    Per utterance: one of `speeds` ((num, den) pairs, default 0.9 / 1.0 / 1.1) is drawn and the utterance resampled by it, which
    changes tempo and pitch together as `sox speed` does, and a linear gain is drawn from [gain[0], gain[1]) -- one launch
    (functional.speed_perturb; semantics: include/qk.h, "Speed and volume perturbation").  The labels of an utterance are unchanged;
    a sped-up utterance has fewer frames for the same labels, so a batch that was just feasible for CTC may stop being so.
    Nobody has measured a phone error rate with this augmentation here.

    The draws are a hash of (seed, counter, utterance index): bit-repeatable from the seed.  __call__ advances the counter with a
    device op behind the kernel, so a captured graph draws anew on every replay and nothing is read on the host (call the policy once
    before capturing: the first call on a device creates the counter and copies the filter tables).
    Data-parallel ranks must pass DIFFERENT seeds, or every rank perturbs its utterance b like every other's; seed and utterance
    index enter the hash as a sum, so keep the seeds at least a batch apart (e.g. seed + 65536 * rank).
    state_dict() / load_state_dict() carry the seed and the counter (reading the counter synchronises)."""

    def __init__(self, speeds=F.DEFAULT_SPEEDS, gain=(1.0, 1.0), zeros=6, rolloff=0.99, seed=0):
        speeds, gain = F._speed_args('SpeedPerturb', speeds, gain, zeros, rolloff, seed)
        F.speed_perturb_tables(speeds, zeros, rolloff)          # (refuses a filter with too many taps)
        self.policy = dict(speeds=speeds, gain=gain, zeros=zeros, rolloff=float(rolloff), seed=seed)
        self._counter = None            # one int32 on the device of the first call; the kernel reads its 32 bits as unsigned
        self._pending = 0               # counter value to start from (load_state_dict before the first call)
        self.last_plan = None

    @property
    def seed(self):
        return self.policy['seed']

    def _counter_on(self, device):
        if self._counter is None:
            v = self._pending - (1 << 32) if self._pending >= 1 << 31 else self._pending
            self._counter = torch.full((1,), v, dtype=torch.int32, device=device)
        elif self._counter.device != device:
            raise ValueError('SpeedPerturb: this policy\'s counter lives on %s, the input on %s' % (self._counter.device, device))
        return self._counter

    def __call__(self, wave, lengths):
        """(out, out_lengths) of functional.speed_perturb for wave (B, n_max); the plan of the call is kept in .last_plan."""
        if not torch.is_tensor(wave) or not wave.is_cuda:
            raise RuntimeError('SpeedPerturb: got a CPU tensor. Speed perturbation runs only on the MI355X HIP path (libqk_hip.so); '
                               'there is no CPU fallback.')
        counter = self._counter_on(wave.device)
        out, out_lengths, self.last_plan = F.speed_perturb(wave, lengths, counter=counter, return_plan=True, **self.policy)
        counter.add_(1)                 # wraps mod 2^32, like the kernel's key
        return out, out_lengths

    def state_dict(self):
        counter = self._pending if self._counter is None else int(self._counter.item()) & 0xFFFFFFFF
        return {'seed': self.policy['seed'], 'counter': counter}

    def load_state_dict(self, d):
        """Takes what state_dict() gave; checked on the host before anything is written."""
        seed, counter = d['seed'], d['counter']
        for name, v in (('seed', seed), ('counter', counter)):
            if isinstance(v, bool) or not isinstance(v, int) or not 0 <= v <= 0xFFFFFFFF:
                raise ValueError('SpeedPerturb.load_state_dict: %s must be an integer in [0, 2^32), got %r' % (name, v))
        self.policy['seed'] = seed
        if self._counter is None:
            self._pending = counter
        else:
            self._counter.fill_(counter - (1 << 32) if counter >= 1 << 31 else counter)


class NoiseReverb(object):
    """A reverberation and additive-noise policy (Kaldi's wav-reverberate, Ko et al., 2017) for waveforms, with its own device
    counter.

        nr = NoiseReverb(rirs=F.prepare_rirs(synthetic_rirs(32)), noises=F.prepare_noises(synthetic_noises(8, 64000)), seed=args.seed)
        x, il = quaternion_fbank(wave, lengths, normalize='utterance', dtype=torch.bfloat16, wave_augment=(sp, nr))   # training only

    Per utterance: with probability rir_prob it is convolved with one room impulse response of the bank `rirs`
    (functional.prepare_rirs), aligned at the response's direct path so that labels and lengths are unchanged, and with probability
    noise_prob one recording of the bank `noises` (functional.prepare_noises) is added, from a drawn offset and wrapped around, at a
    signal-to-noise ratio drawn from [snr[0], snr[1]) dB -- two launches (functional.noise_reverb; semantics: include/qk.h,
    "Reverberation and additive noise").  A bank of None switches its half off.  It goes behind SpeedPerturb, as in Kaldi's recipes.
    Nobody has measured a phone error rate with this augmentation here.

    The draws are a hash of (seed, counter, utterance index): bit-repeatable from the seed.  __call__ advances the counter with a
    device op behind the kernels, so a captured graph draws anew on every replay and nothing is read on the host (call the policy
    once before capturing: the first call on a device creates the counter and copies the banks).
    Data-parallel ranks must pass DIFFERENT seeds; seed and utterance index enter the hash as a sum, so keep the seeds at least a
    batch apart (e.g. seed + 65536 * rank).
    state_dict() / load_state_dict() carry the seed and the counter (reading the counter synchronises); the banks are not state."""

    def __init__(self, rirs=None, noises=None, rir_prob=0.5, noise_prob=0.5, snr=(5.0, 20.0), seed=0):
        rirs, noises, _ = F._env_args('NoiseReverb', rirs, noises, rir_prob, noise_prob, snr, seed)
        self.policy = dict(rirs=rirs, noises=noises, rir_prob=float(rir_prob), noise_prob=float(noise_prob),
                           snr=(float(snr[0]), float(snr[1])), seed=seed)
        self._counter = None            # one int32 on the device of the first call; the kernel reads its 32 bits as unsigned
        self._pending = 0               # counter value to start from (load_state_dict before the first call)
        self.last_plan = None

    @property
    def seed(self):
        return self.policy['seed']

    def _counter_on(self, device):
        if self._counter is None:
            v = self._pending - (1 << 32) if self._pending >= 1 << 31 else self._pending
            self._counter = torch.full((1,), v, dtype=torch.int32, device=device)
            for name in ('rirs', 'noises'):                     # the banks move once, with the counter
                if self.policy[name] is not None:
                    self.policy[name] = tuple(t.to(device).contiguous() for t in self.policy[name])
        elif self._counter.device != device:
            raise ValueError('NoiseReverb: this policy\'s counter lives on %s, the input on %s' % (self._counter.device, device))
        return self._counter

    def __call__(self, wave, lengths):
        """(out, lengths) with out of functional.noise_reverb for wave (B, n_max); the plan of the call is kept in .last_plan."""
        if not torch.is_tensor(wave) or not wave.is_cuda:
            raise RuntimeError('NoiseReverb: got a CPU tensor. Reverberation and additive noise run only on the MI355X HIP path '
                               '(libqk_hip.so); there is no CPU fallback.')
        counter = self._counter_on(wave.device)
        out, self.last_plan = F.noise_reverb(wave, lengths, counter=counter, return_plan=True, **self.policy)
        counter.add_(1)                 # wraps mod 2^32, like the kernel's key
        return out, lengths

    def state_dict(self):
        counter = self._pending if self._counter is None else int(self._counter.item()) & 0xFFFFFFFF
        return {'seed': self.policy['seed'], 'counter': counter}

    def load_state_dict(self, d):
        """Takes what state_dict() gave; checked on the host before anything is written."""
        seed, counter = d['seed'], d['counter']
        for name, v in (('seed', seed), ('counter', counter)):
            if isinstance(v, bool) or not isinstance(v, int) or not 0 <= v <= 0xFFFFFFFF:
                raise ValueError('NoiseReverb.load_state_dict: %s must be an integer in [0, 2^32), got %r' % (name, v))
        self.policy['seed'] = seed
        if self._counter is None:
            self._pending = counter
        else:
            self._counter.fill_(counter - (1 << 32) if counter >= 1 << 31 else counter)


def synthetic_rirs(count, sample_rate=16000, rt60=(0.2, 0.8), seed=0):
    """`count` synthetic room impulse responses (a list of float64 arrays for functional.prepare_rirs), on the host: a unit direct
    path after 0 .. 2 ms, and behind it Gaussian noise under an exponential envelope that falls by 60 dB in a reverberation time
    drawn from rt60 (seconds), at a drawn direct-to-reverberant level; each response is cut where its envelope has fallen by 60 dB
    (and prepare_rirs cuts at its max_taps).  The classic Moorer / Polack model: enough to exercise and to use the augmentation
    without a corpus of measured rooms, not a substitute for one."""
    if isinstance(count, bool) or not isinstance(count, int) or count < 1:
        raise ValueError('synthetic_rirs: count must be a positive integer, got %r' % (count,))
    lo, hi = rt60
    if not 0.0 < lo <= hi or not math.isfinite(hi) or not sample_rate > 0:
        raise ValueError('synthetic_rirs: need 0 < rt60 low <= rt60 high and a positive sample rate')
    rng = np.random.RandomState(seed)
    out = []
    for _ in range(count):
        t60 = rng.uniform(lo, hi)
        onset = int(rng.randint(0, max(int(0.002 * sample_rate), 1) + 1))
        n = max(int(round(t60 * sample_rate)), 2)
        t = np.arange(n, dtype=np.float64) / sample_rate
        tail = rng.randn(n) * np.exp(-math.log(1000.0) * t / t60)
        tail *= 10.0 ** (-rng.uniform(0.0, 10.0) / 20.0) / math.sqrt(float(np.sum(tail[1:] ** 2)))       # reverberant energy 0 .. -10 dB
        tail[0] = 1.0
        out.append(np.concatenate([np.zeros(onset), tail]))
    return out


def synthetic_noises(count, samples, seed=0):
    """`count` synthetic noise recordings of `samples` samples (a list of float64 arrays for functional.prepare_noises), on the host:
    even ones white, odd ones 1/f-shaped (pink: white noise whose spectrum is divided by sqrt(f)), each at unit power."""
    for name, v in (('count', count), ('samples', samples)):
        if isinstance(v, bool) or not isinstance(v, int) or v < 1:
            raise ValueError('synthetic_noises: %s must be a positive integer, got %r' % (name, v))
    rng = np.random.RandomState(seed)
    out = []
    for i in range(count):
        v = rng.randn(samples)
        if i % 2 and samples > 1:
            spec = np.fft.rfft(v)
            spec[1:] /= np.sqrt(np.arange(1, spec.size, dtype=np.float64))
            spec[0] = 0.0
            v = np.fft.irfft(spec, samples)
        power = float(np.mean(v * v))
        out.append(v / math.sqrt(power) if power > 0 else v)
    return out
