"""Chroma features and chroma similarity on the GPU: how much of a source clip's melody and harmony an edit keeps.

``chroma_stft`` is ``librosa.feature.chroma_stft`` at its defaults (n_fft 2048, hop 512, periodic Hann, center=True with zero padding,
power spectrum, 12 classes, L-infinity normalisation per frame) with ONE stated deviation: librosa estimates a tuning per signal, here
it is an argument of the filterbank builder, fixed at 0.  ``chroma_similarity`` is the mean over the frames of the cosine between the
edit's and the source's chroma vectors (the fidelity metric of the AP-adapter paper).  **PARITY UNPINNED**: librosa is not a
dependency and was not available to compare against; the formula is restated here and in tests/chroma_oracle.py, and held to pitch
anchors (A4 -> row 9, C4 -> row 0, E4 -> row 4).

The STFT, the filterbank product, the normalisation (``apad_chroma``) and the similarity (``apad_chroma_similarity``) are one HIP launch
each; the host builds the constant tables and, for ranking, sorts a handful of scores.  ``resolve_rank_by`` / ``group_order`` are the
host half of ``AudioLDM2Pipeline.__call__(rank_by=)``.
"""
import numpy as np
import torch

from . import frontend, ops
from .derived import derived

SR, N_FFT, HOP, N_CHROMA = 16000, 2048, 512, 12


def chroma_filterbank(sr=SR, n_fft=N_FFT, n_chroma=N_CHROMA, tuning=0.0, ctroct=5.0, octwidth=2.0, base_c=True):
    """``librosa.filters.chroma(sr=, n_fft=, n_chroma=, tuning=, ctroct=, octwidth=, norm=2, base_c=)`` restated: float64
    [n_chroma][n_fft / 2 + 1].  Every FFT bin gets a Gaussian bump over its (wrapped) distance to each pitch class, measured in units of
    the bin's own width in classes; each column is L2-normalised over the classes, then weighted by a Gaussian of ``octwidth`` octaves
    around octave ``ctroct`` (A0 = 27.5 Hz is octave 0, so 5 is 880 Hz); the rows are rolled so that row 0 is C."""
    freqs = np.arange(1, n_fft, dtype=np.float64) * (float(sr) / n_fft)
    a440 = 440.0 * 2.0 ** (float(tuning) / n_chroma)
    bins = n_chroma * np.log2(freqs / (a440 / 16.0))
    bins = np.concatenate(([bins[0] - 1.5 * n_chroma], bins))  # the 0 Hz bin: 1.5 octaves below bin 1
    width = np.concatenate((np.maximum(bins[1:] - bins[:-1], 1.0), [1.0]))
    half = np.round(n_chroma / 2.0)
    d = bins[None, :] - np.arange(n_chroma, dtype=np.float64)[:, None]
    d = np.remainder(d + half + 10 * n_chroma, n_chroma) - half  # into [-n_chroma / 2, n_chroma / 2)
    w = np.exp(-0.5 * (2.0 * d / width[None, :]) ** 2)
    norm = np.sqrt((w * w).sum(axis=0, keepdims=True))
    w = w / np.where(norm < np.finfo(np.float64).tiny, 1.0, norm)
    if octwidth is not None:
        w = w * np.exp(-0.5 * ((bins / n_chroma - ctroct) / octwidth) ** 2)[None, :]
    if base_c:
        w = np.roll(w, -3 * (n_chroma // 12), axis=0)
    return np.ascontiguousarray(w[:, : n_fft // 2 + 1])


def frame_count(n):
    """frames of a clip of ``n`` samples (center=True): 1 + n // 512"""
    return 1 + int(n) // HOP


_FB64 = {}  # tuning -> the float64 filterbank on the host: the tensor the device tables derive from


def tables(dev, tuning=0.0):
    """(periodic Hann [2048], twiddles [1024][2], chroma filterbank [12][1025]) fp32 on ``dev``, from the derived-weight cache"""
    tuning = float(tuning)
    if tuning not in _FB64:
        _FB64[tuning] = torch.from_numpy(chroma_filterbank(tuning=tuning))
    fb64 = _FB64[tuning]

    def make():
        n = np.arange(N_FFT, dtype=np.float64)
        window = 0.5 - 0.5 * np.cos(2 * np.pi * n / N_FFT)
        k = np.arange(N_FFT // 2, dtype=np.float64)
        tw = np.stack([np.cos(2 * np.pi * k / N_FFT), -np.sin(2 * np.pi * k / N_FFT)], axis=1)
        return tuple(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev) for a in (window, tw)) + \
            (fb64.detach().to(torch.float32).to(dev).contiguous(),)

    return derived(fb64, ("chroma_tables", str(dev)), make)


def _clips(wav, sampling_rate, device=None):
    """wav -> list of 1-D fp32 GPU clips at 16 kHz: a tensor / array [b, samples] or [samples], or a ragged list of 1-D ones"""
    if torch.is_tensor(wav) or isinstance(wav, np.ndarray):
        t = torch.as_tensor(wav)
        if t.dim() not in (1, 2):
            raise ValueError(f"chroma: expected a waveform [samples] or [b, samples], got {tuple(t.shape)}")
        clips = [t] if t.dim() == 1 else list(t)
    else:
        clips = [torch.as_tensor(np.asarray(c, dtype=np.float32) if not torch.is_tensor(c) else c) for c in wav]
    if not clips or any(c.dim() != 1 or c.numel() == 0 for c in clips):
        raise ValueError("chroma: every clip must be a non-empty 1-D waveform")
    dev = device if device is not None else next((c.device for c in clips if c.is_cuda), None)
    if dev is None:
        if not torch.cuda.is_available():
            raise RuntimeError("chroma: expected GPU waveforms (or a GPU to upload them to); the HIP path has no CPU fallback")
        dev = torch.device("cuda", torch.cuda.current_device())
    clips = [c.to(device=dev, dtype=torch.float32) for c in clips]
    if int(sampling_rate) != SR:
        clips = [frontend.resample(c.reshape(1, -1).contiguous(), sampling_rate, SR)[0] for c in clips]
    return clips, dev


def chroma_stft(wav, sampling_rate=16000, target_frames=None, tuning=0.0, return_frames=False):
    """The chromagrams of a batch of clips in one launch: fp32 [b, target_frames, 12] on the GPU (time-major: librosa's [12, frames]
    transposed), ``target_frames`` = the longest clip's frame count unless given; rows after a clip's 1 + n // 512 frames are zero.
    ``wav``: a tensor / array [b, samples] or [samples] or a ragged list of 1-D clips; a rate other than 16 kHz goes through
    ``frontend.resample`` first.  ``return_frames`` adds the per-clip frame counts (a list)."""
    clips, dev = _clips(wav, sampling_rate)
    counts = [frame_count(c.numel()) for c in clips]
    T = max(counts) if target_frames is None else int(target_frames)
    offsets_host = torch.zeros(len(clips) + 1, dtype=torch.int64)
    offsets_host[1:] = torch.cumsum(torch.tensor([c.numel() for c in clips], dtype=torch.int64), 0)
    whole = torch.is_tensor(wav) and wav.is_cuda and wav.dtype == torch.float32 and wav.is_contiguous() and int(sampling_rate) == SR
    packed = wav.reshape(-1) if whole else torch.cat([c.contiguous() for c in clips])
    out = torch.empty(len(clips), T, N_CHROMA, dtype=torch.float32, device=dev)
    ops.chroma(packed, offsets_host.to(dev), offsets_host, *tables(dev, tuning), out)
    return (out, counts) if return_frames else out


def default_ref_index(n, m):
    """candidate i of n -> reference i // (n / m): each reference serves a run of n / m consecutive candidates"""
    if m <= 0 or n % m != 0:
        raise ValueError(f"chroma similarity: {m} references for {n} candidates (need a divisor)")
    return [i // (n // m) for i in range(n)]


def chroma_similarity(edit, source, sampling_rate=16000, ref_index=None, tuning=0.0, return_per_frame=False):
    """Per-candidate chroma similarity, fp32 [n] on the GPU: the mean over the frames both clips have of the cosine between the edit's
    and the source's chroma vectors (1 = same pitch-class content in every frame, 0 = nothing shared or silence).  ``edit`` n clips,
    ``source`` m clips (forms as in ``chroma_stft``); candidate i is compared with source ``ref_index[i]`` (default: i // (n / m)).
    Two launches of ``apad_chroma`` and one of ``apad_chroma_similarity``; nothing is read back.  ``return_per_frame`` adds the
    cosines, fp32 [n, T]."""
    e_clips, dev = _clips(edit, sampling_rate)
    s_clips, _ = _clips(source, sampling_rate, device=dev)
    n, m = len(e_clips), len(s_clips)
    idx = default_ref_index(n, m) if ref_index is None else [int(i) for i in ref_index]
    if len(idx) != n or any(not 0 <= i < m for i in idx):
        raise ValueError(f"chroma similarity: ref_index must hold {n} entries in [0, {m})")
    T = max(frame_count(c.numel()) for c in e_clips + s_clips)
    a, fa = chroma_stft(e_clips, SR, target_frames=T, tuning=tuning, return_frames=True)
    b, fb_ = chroma_stft(s_clips, SR, target_frames=T, tuning=tuning, return_frames=True)
    idx_host = torch.tensor(idx, dtype=torch.int32)
    frames_host = torch.tensor([min(fa[i], fb_[idx[i]]) for i in range(n)], dtype=torch.int32)
    per_frame = torch.empty(n, T, dtype=torch.float32, device=dev) if return_per_frame else None
    out = ops.chroma_similarity(a, b, idx_host.to(dev), idx_host, frames_host.to(dev), frames_host, per_frame=per_frame)
    return (out, per_frame) if return_per_frame else out


# ---- ranking: the host half of AudioLDM2Pipeline.__call__(rank_by=) ----
def resolve_rank_by(rank_by):
    """``rank_by`` -> None (today's path: CLAP ranking among all candidates where the call has text prompts and towers) or the weights
    (w_clap, w_chroma) of the score each prompt's own candidates are ordered by.  None and "clap" -> None; "chroma" -> (0, 1);
    {"clap": w_t, "chroma": w_f} -> (w_t, w_f); anything else raises ValueError."""
    if rank_by is None or (isinstance(rank_by, str) and rank_by == "clap"):
        return None
    if isinstance(rank_by, str) and rank_by == "chroma":
        return 0.0, 1.0
    if isinstance(rank_by, dict) and set(rank_by) == {"clap", "chroma"}:
        try:
            w = float(rank_by["clap"]), float(rank_by["chroma"])
        except (TypeError, ValueError):
            w = None
        if w is not None and all(np.isfinite(w)):
            return w
    raise ValueError(f"rank_by={rank_by!r}: None, 'clap', 'chroma' or {{'clap': w_t, 'chroma': w_f}} with two finite weights")


def mixed_scores(weights, chroma_sim, logits_per_text=None, logit_scale=1.0, group=1):
    """The score of each candidate, float64 [B] on the host: w_t * cos_clap + w_f * chroma, cos_clap[i] = logits_per_text[i // group, i]
    / logit_scale (candidate i against its OWN prompt; ``logits_per_text`` [P, B] is only read when w_t != 0)."""
    w_t, w_f = weights
    s = w_f * torch.as_tensor(chroma_sim).detach().to("cpu", torch.float64)
    if w_t != 0.0:
        lg = torch.as_tensor(logits_per_text).detach().to("cpu", torch.float64)
        own = lg[torch.arange(s.numel()) // group, torch.arange(s.numel())]
        s = s + w_t * (own / float(logit_scale))
    return s


def group_order(scores, group):
    """Indices [B] that re-order the candidates WITHIN each run of ``group`` consecutive ones (a prompt's own candidates) by descending
    score, ties in their original order; no candidate leaves its prompt's group"""
    s = torch.as_tensor(scores).detach().to("cpu").reshape(-1, group)
    order = torch.argsort(s, dim=1, descending=True, stable=True)
    return (order + torch.arange(s.shape[0])[:, None] * group).reshape(-1)
