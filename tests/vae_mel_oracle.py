"""fp64 restatement of the reference's training mel (``wav_to_mel``, train_apadapter_v2.py:253-336) for the tests.  TEST
INFRASTRUCTURE ONLY.

The STFT / mel core is audioldm's ``TacotronSTFT(1024, 160, 1024, 64, 16000, 0, 8000).mel_spectrogram``: reflect padding by
512, conv1d with the Fourier basis times a periodic Hann window (scipy ``get_window("hann", 1024, fftbins=True)``), magnitude,
``librosa.filters.mel`` (Slaney scale, Slaney norm), ``log(clamp(., 1e-5))``.  tests/test_vae_mel_oracle.py pins it to
``torch.stft`` and ``transformers.audio_utils``.

**PARITY UNPINNED** for the glue (audioldm 0.1.x is not installed; restated from its published source):
  read_wav_file   torchaudio.load -> resample to 16 kHz -> channel 0 -> normalize_wav (x - mean, / (max|x| + 1e-8), * 0.5)
                  -> pad_wav(segment = target * 160) -> / max|x| (or / 1e-6 when it is 0) -> * 0.5
  pad_wav         a shorter clip is zero-padded to ``segment``; a longer one is NOT truncated (``waveform[:segment]`` slices
                  axis 0 of a [1, N] array); <= 100 samples fails an assert
  get_mel_from_wav  clip to [-1, 1], mel_spectrogram, transpose to [frames, 64]
  _pad_spec       crop to / zero-fill up to ``target`` rows
In real arithmetic the two normalisations are y = 0.5 (x - m) / max|x - m| (0 for a constant clip); that is what this
module computes, in float64.
"""
import math

import numpy as np

SR, NFFT, HOP, NMEL, FMAX = 16000, 1024, 160, 64, 8000.0


def target_frames(duration):
    return int(duration * 102.4)


def hz_to_mel(f):
    f = np.asarray(f, np.float64)
    f_sp, min_log_hz = 200.0 / 3, 1000.0
    min_log_mel, logstep = min_log_hz / f_sp, math.log(6.4) / 27.0
    lin = f / f_sp
    return np.where(f >= min_log_hz, min_log_mel + np.log(np.maximum(f, min_log_hz) / min_log_hz) / logstep, lin)


def mel_to_hz(m):
    m = np.asarray(m, np.float64)
    f_sp, min_log_hz = 200.0 / 3, 1000.0
    min_log_mel, logstep = min_log_hz / f_sp, math.log(6.4) / 27.0
    return np.where(m >= min_log_mel, min_log_hz * np.exp(logstep * (m - min_log_mel)), f_sp * m)


def mel_filters(sr=SR, n_fft=NFFT, n_mels=NMEL, fmin=0.0, fmax=FMAX):
    """librosa.filters.mel(htk=False, norm="slaney") in float64: [n_mels, n_fft / 2 + 1]"""
    fft_f = np.linspace(0.0, sr / 2.0, n_fft // 2 + 1)
    pts = mel_to_hz(np.linspace(hz_to_mel(fmin), hz_to_mel(fmax), n_mels + 2))
    w = np.zeros((n_mels, fft_f.size))
    for i in range(n_mels):
        lo, c, hi = pts[i], pts[i + 1], pts[i + 2]
        up = (fft_f - lo) / (c - lo)
        down = (hi - fft_f) / (hi - c)
        w[i] = np.maximum(0.0, np.minimum(up, down)) * (2.0 / (hi - lo))
    return w


def hann_periodic(n=NFFT):
    return 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(n) / n)


def stft_magnitude(y):
    """|STFT| [frames, 513] of y (float64 [N]), frames = N // 160 + 1: reflect pad 512 (edge sample excluded), periodic Hann"""
    y = np.asarray(y, np.float64)
    p = np.pad(y, (NFFT // 2, NFFT // 2), mode="reflect")
    frames = y.shape[0] // HOP + 1
    idx = np.arange(frames)[:, None] * HOP + np.arange(NFFT)[None, :]
    return np.abs(np.fft.rfft(p[idx] * hann_periodic()[None, :], axis=1))


def log_mel(y):
    """mel_spectrogram(y) transposed: log(max(mel @ |STFT|, 1e-5)) [frames, 64]"""
    return np.log(np.maximum(stft_magnitude(y) @ mel_filters().T, 1e-5))


def normalize(x):
    """normalize_wav + pad_wav's zeros + the second peak normalisation, in real arithmetic (over the WHOLE clip)"""
    x = np.asarray(x, np.float64)
    d = x - x.mean()
    peak = np.abs(d).max()
    y = 0.5 * d / peak if peak > 0 else np.zeros_like(d)
    return np.clip(y, -1.0, 1.0)


def pad_wav(y, segment):
    n = y.shape[0]
    assert n > 100, n
    if n < segment:
        return np.concatenate([y, np.zeros(segment - n)])
    return y  # not truncated


def pad_spec(spec, target):
    p = target - spec.shape[0]
    if p > 0:
        return np.concatenate([spec, np.zeros((p, spec.shape[1]))])
    return spec[:target]


def mel_from_16k(x16, duration=10.0):
    """16 kHz samples of channel 0 -> [1, target, 64] float64"""
    target = target_frames(duration)
    y = pad_wav(normalize(x16), target * HOP)
    return pad_spec(log_mel(y), target)[None]


def wav_to_mel(waveform, sr, duration=10.0):
    """waveform float32 [channels, samples] (torchaudio.load convention) -> [1, target, 64] float64.  Resampling is the
    front-end oracle's (oracle/fbank.py, fp32 like torchaudio)."""
    from oracle.fbank import resample
    w = np.asarray(waveform, np.float32)
    x = w if w.ndim == 1 else w[0]
    if int(sr) != SR:
        x = resample(x, sr, SR)
    return mel_from_16k(x.astype(np.float64), duration)
