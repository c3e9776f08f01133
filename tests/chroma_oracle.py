"""Independent restatement of chroma features and chroma similarity for the tests: ``torch.stft`` for the transform, a filterbank
written bin by bin in numpy, and the similarity as plain tensor code.  float64 by default; ``dtype=torch.float32`` runs the same chain
in fp32 on the CPU (the yardstick the GPU tests scale their bounds by).  librosa is not installed here, so this file is the restated
formula of ``librosa.feature.chroma_stft`` (defaults, tuning fixed at 0), not a call into it."""
import math

import numpy as np
import torch

SR, N_FFT, HOP, N_CHROMA = 16000, 2048, 512, 12
TINY32 = 1.1754944e-38


def filterbank(sr=SR, n_fft=N_FFT, tuning=0.0, ctroct=5.0, octwidth=2.0):
    """[12][n_fft / 2 + 1] float64, row 0 = C: one FFT bin at a time"""
    a0 = 440.0 * 2.0 ** (tuning / 12.0) / 16.0  # A0 (27.5 Hz at tuning 0): octave 0
    pos = [0.0] * n_fft  # each bin's position in pitch classes above A0
    for k in range(1, n_fft):
        pos[k] = 12.0 * math.log2(k * sr / n_fft / a0)
    pos[0] = pos[1] - 18.0  # the 0 Hz bin: 1.5 octaves below bin 1
    fb = np.zeros((12, n_fft // 2 + 1))
    for k in range(n_fft // 2 + 1):
        width = max(pos[k + 1] - pos[k], 1.0) if k + 1 < n_fft else 1.0
        col = np.zeros(12)
        for c in range(12):  # class c counted from A; the wrapped distance lies in [-6, 6)
            d = (pos[k] - c + 6.0 + 120.0) % 12.0 - 6.0
            col[c] = math.exp(-0.5 * (2.0 * d / width) ** 2)
        nrm = math.sqrt(float((col * col).sum()))
        col = col / (nrm if nrm >= np.finfo(np.float64).tiny else 1.0)
        col = col * math.exp(-0.5 * ((pos[k] / 12.0 - ctroct) / octwidth) ** 2)
        for c in range(12):
            fb[(c - 3) % 12, k] = col[c]  # A is class 9 when row 0 is C
    return fb


_FB = {}


def frame_count(n):
    return 1 + n // HOP


def chroma(x, dtype=torch.float64):
    """x: 1-D samples (any float dtype; taken as they are) -> [frames, 12] in ``dtype`` on the CPU"""
    if "fb" not in _FB:
        _FB["fb"] = torch.from_numpy(filterbank())
    x = torch.as_tensor(x).detach().cpu().to(dtype)
    window = torch.hann_window(N_FFT, periodic=True, dtype=torch.float64).to(dtype)
    spec = torch.stft(x, N_FFT, hop_length=HOP, window=window, center=True, pad_mode="constant", return_complex=True)  # [1025, frames]
    power = spec.real ** 2 + spec.imag ** 2
    c = (_FB["fb"].to(dtype) @ power).T  # [frames, 12]
    m = c.abs().amax(dim=1, keepdim=True)
    m = torch.where(m < TINY32, torch.ones_like(m), m)
    return c / m


def chroma_batch(clips, target_frames, dtype=torch.float64):
    """ragged clips -> [B, target_frames, 12], zero rows past each clip's frames"""
    out = torch.zeros(len(clips), target_frames, N_CHROMA, dtype=dtype)
    for b, x in enumerate(clips):
        c = chroma(x, dtype)
        assert c.shape[0] == frame_count(len(x))
        out[b, : c.shape[0]] = c
    return out


def similarity(a, b, ref_index, frames, dtype=torch.float64):
    """a [n, T, 12], b [m, T, 12] -> (mean cosine over the first frames[i] frames [n], per-frame cosines [n, T] with 0 past frames[i])"""
    a, b = torch.as_tensor(a).detach().cpu().to(dtype), torch.as_tensor(b).detach().cpu().to(dtype)
    n, T = a.shape[:2]
    per = torch.zeros(n, T, dtype=dtype)
    out = torch.zeros(n, dtype=dtype)
    for i in range(n):
        f = int(frames[i])
        if f == 0:
            continue
        u, v = a[i, :f], b[int(ref_index[i]), :f]
        den = torch.clamp(u.norm(dim=1) * v.norm(dim=1), min=1e-8)
        per[i, :f] = (u * v).sum(dim=1) / den
        out[i] = per[i, :f].mean()
    return out, per


def waveform_similarity(edit, source, ref_index=None, dtype=torch.float64):
    """waveforms [n, samples], [m, samples] -> chroma similarity [n] (candidate i against source ref_index[i], default i // (n / m))"""
    n, m = len(edit), len(source)
    idx = [i // (n // m) for i in range(n)] if ref_index is None else list(ref_index)
    T = max(frame_count(len(x)) for x in list(edit) + list(source))
    a, b = chroma_batch(edit, T, dtype), chroma_batch(source, T, dtype)
    frames = [min(frame_count(len(edit[i])), frame_count(len(source[idx[i]]))) for i in range(n)]
    return similarity(a, b, idx, frames, dtype)[0]


def tone(freq, n=8192, sr=SR):
    return np.sin(2.0 * np.pi * freq * np.arange(n) / sr)


def signal(n, seed, sr=SR):
    """a sum of five sines between 100 and 4000 Hz plus 5 % noise, peak-normalised, float32 [n]"""
    g = np.random.RandomState(seed)
    t = np.arange(n, dtype=np.float64) / sr
    x = sum(g.uniform(0.3, 1.0) * np.sin(2.0 * np.pi * g.uniform(100.0, 4000.0) * t + g.uniform(0.0, 2.0 * np.pi)) for _ in range(5))
    x = x + 0.05 * g.standard_normal(n)
    return (x / np.abs(x).max()).astype(np.float32)
