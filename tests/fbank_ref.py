"""Float64 numpy restatement of the acoustic front end that qcnn_amd.features.quaternion_fbank computes on the device.

The recipe is python_speech_features' `logfbank` + `delta` (nfilt = 40 by default), stacked into the model's channels_first quaternion
input: r = static rows (40 log mel energies + log frame energy), i / j / k = first / second / third time derivative.  That library is
not a dependency, so its steps are restated here (sigproc.preemphasis / framesig / powspec, base.get_filterbanks / fbank / delta).
"""
import decimal
import math

import numpy as np

EPS = np.finfo(float).eps                   # what python_speech_features puts in place of exact zeros before the log


def round_half_up(x):
    return int(decimal.Decimal(x).quantize(decimal.Decimal('1'), rounding=decimal.ROUND_HALF_UP))


def frame_geometry(sample_rate=16000, winlen=0.025, winstep=0.01):
    return round_half_up(winlen * sample_rate), round_half_up(winstep * sample_rate)


def num_frames(n, frame_len, frame_step):
    if n <= frame_len:
        return 1
    return 1 + int(math.ceil((1.0 * n - frame_len) / frame_step))


def hz2mel(hz):
    return 2595 * np.log10(1 + hz / 700.)


def mel2hz(mel):
    return 700 * (10 ** (mel / 2595.0) - 1)


def mel_bins(nfilt=40, nfft=512, sample_rate=16000, lowfreq=0, highfreq=None):
    highfreq = highfreq or sample_rate / 2
    melpoints = np.linspace(hz2mel(lowfreq), hz2mel(highfreq), nfilt + 2)
    return np.floor((nfft + 1) * mel2hz(melpoints) / sample_rate)


def mel_filterbank(nfilt=40, nfft=512, sample_rate=16000, lowfreq=0, highfreq=None):
    """get_filterbanks: (nfilt, nfft // 2 + 1) triangles on integer bins."""
    b = mel_bins(nfilt, nfft, sample_rate, lowfreq, highfreq)
    fb = np.zeros([nfilt, nfft // 2 + 1])
    for j in range(nfilt):
        for i in range(int(b[j]), int(b[j + 1])):
            fb[j, i] = (i - b[j]) / (b[j + 1] - b[j])
        for i in range(int(b[j + 1]), int(b[j + 2])):
            fb[j, i] = (b[j + 2] - i) / (b[j + 2] - b[j + 1])
    return fb


def static_rows(sig, sample_rate=16000, winlen=0.025, winstep=0.01, nfilt=40, nfft=512, lowfreq=0, highfreq=None, preemph=0.97,
                window='rect', append_energy=True):
    """(n_frames, nfilt [+ 1]) float64: log mel energies (+ log frame energy) of one utterance."""
    sig = np.asarray(sig, dtype=np.float64)
    L, S = frame_geometry(sample_rate, winlen, winstep)
    sig = np.append(sig[:1], sig[1:] - preemph * sig[:-1])
    n = num_frames(len(sig), L, S)
    padded = np.concatenate((sig, np.zeros((n - 1) * S + L - len(sig))))
    idx = np.arange(L)[None, :] + S * np.arange(n)[:, None]
    frames = padded[idx]
    if window == 'hamming':
        frames = frames * np.hamming(L)[None, :]
    pspec = np.absolute(np.fft.rfft(frames, nfft)) ** 2 / nfft
    energy = np.sum(pspec, 1)
    energy = np.where(energy == 0, EPS, energy)
    feat = np.dot(pspec, mel_filterbank(nfilt, nfft, sample_rate, lowfreq, highfreq).T)
    feat = np.where(feat == 0, EPS, feat)
    feat = np.log(feat)
    if append_energy:
        feat = np.concatenate((feat, np.log(energy)[:, None]), axis=1)
    return feat


def delta(feat, N):
    """python_speech_features.delta along axis 0 (frames), edge padding at this utterance's own first and last frame."""
    n = len(feat)
    denom = 2 * sum(i ** 2 for i in range(1, N + 1))
    padded = np.pad(feat, ((N, N), (0, 0)), mode='edge')
    out = np.empty_like(feat)
    for t in range(n):
        out[t] = np.dot(np.arange(-N, N + 1), padded[t:t + 2 * N + 1]) / denom
    return out


def quaternion_fbank(waves, lengths, delta_n=2, normalize=None, **kw):
    """(B, 4, F, T_max) float64 and the frame counts, for a list / batch of waveforms cut to lengths[b] samples."""
    L, S = frame_geometry(kw.get('sample_rate', 16000), kw.get('winlen', 0.025), kw.get('winstep', 0.01))
    nf = [num_frames(int(n), L, S) for n in lengths]
    per = []
    for b, n in enumerate(lengths):
        s = static_rows(np.asarray(waves[b][:int(n)]), **kw)
        d1 = delta(s, delta_n)
        d2 = delta(d1, delta_n)
        d3 = delta(d2, delta_n)
        q = np.stack([s, d1, d2, d3]).transpose(0, 2, 1)          # (4, F, n_frames)
        if normalize == 'utterance':
            q = (q - q.mean(-1, keepdims=True)) / np.sqrt(q.var(-1, keepdims=True) + 1e-8)
        per.append(q)
    out = np.zeros((len(per), 4, per[0].shape[1], max(nf)))
    for b, q in enumerate(per):
        out[b, :, :, :q.shape[-1]] = q
    return out, np.array(nf, dtype=np.int32)
