"""The CLAP feature extractor's oracle, shared by tests/test_clap_features_host.py and tests/test_gpu_clap_features.py: the INSTALLED
transformers ``ClapFeatureExtractor`` (numpy, float64) with ``truncation="rand_trunc"`` on the same fp32 samples, the seeded
full-band test signals, and the two-tier comparison of a dB feature map against it."""
import numpy as np
import torch

SR = 48000


def installed(**kw):
    from transformers.models.clap.feature_extraction_clap import ClapFeatureExtractor
    kw.setdefault("truncation", "rand_trunc")
    return ClapFeatureExtractor(**kw)


def signal(n, seed, sr=SR):
    """fp32 [n]: Gaussian noise (sigma 0.1) plus two amplitude-modulated tones, generated at ``sr`` -- full band, so that every mel
    filter carries energy"""
    g = np.random.RandomState(seed)
    t = np.arange(n, dtype=np.float64) / sr
    f1, f2 = g.uniform(200.0, 2000.0), g.uniform(3000.0, 11000.0)
    x = 0.1 * g.standard_normal(n)
    x += 0.3 * (1.0 + 0.5 * np.sin(2 * np.pi * 3.0 * t)) * np.sin(2 * np.pi * f1 * t + g.uniform(0, 6.28))
    x += 0.2 * (1.0 + 0.8 * np.sin(2 * np.pi * 7.0 * t + 1.0)) * np.sin(2 * np.pi * f2 * t + g.uniform(0, 6.28))
    return x.astype(np.float32)


def reference(fe, clips, padding, max_length, crop_starts=None):
    """the installed extractor's input_features [B, 1, frames, feature_size] (fp32 tensor) for fp32 clips; a clip longer than
    ``max_length`` is cut at its crop start first (the installed class then frames exactly those samples, whatever it draws)"""
    cut = []
    for b, c in enumerate(clips):
        c = np.asarray(c, dtype=np.float32)
        if len(c) > max_length:
            s = int(crop_starts[b])
            assert 0 <= s <= len(c) - max_length
            c = c[s:s + max_length]
        cut.append(c)
    out = fe(cut, padding=padding, max_length=max_length, sampling_rate=fe.sampling_rate, return_tensors="pt")
    return out.input_features.float()


def silent_frames(ref):
    """[B, frames] bool: frames whose reference is the floor in every filter (an all-zero input)"""
    return (ref[:, 0] == -100.0).all(dim=-1)


def tier_a_mask(ref):
    """entries whose reference is within 60 dB of their frame's maximum"""
    return ref >= ref.amax(dim=-1, keepdim=True) - 60.0


def tier_a_coverage(ref):
    """share of tier A among the entries of the non-silent frames"""
    live = ~silent_frames(ref)
    return float(tier_a_mask(ref)[:, 0][live].float().mean())


def tier_errors(out, ref):
    """(tier A: max |out - ref| in dB over the entries within 60 dB of their frame's maximum; tier B: max over ALL entries of
    |10^(out/10) - 10^(ref/10)| relative to the frame's maximum mel power), in float64"""
    out, ref = out.detach().double().cpu(), ref.detach().double().cpu()
    a = float(((out - ref).abs() * tier_a_mask(ref)).max())
    p_out, p_ref = torch.pow(10.0, out / 10.0), torch.pow(10.0, ref / 10.0)
    b = float(((p_out - p_ref).abs() / p_ref.amax(dim=-1, keepdim=True)).max())
    return a, b
