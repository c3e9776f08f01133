"""-m gpu: the waveform front-ends of csrc/frontend.hip (apad_resample_fir, apad_wav_stats, apad_stft_logmel, apad_kaldi_fbank, apad_clap_logmel,
apad_chroma) held to impulses, bin-centred tones, dyadic samples and NaN neighbours.

The cases, their fp64 expectations, the derivation of the bound and the one measured term (the device logarithm, LOG_TOL) live in
tests/spectral_cases.py; tests/test_spectral_exact_host.py checks on the CPU that the expectations agree with the project's oracles, that the
fp32 restatement of each kernel stays inside the bound, that floors hold with room and that each case would see the mutation it exists for.

What is compared how:
  * the resampler of an impulse is 0.5 x its own table and +0.0 elsewhere: ``torch.equal`` (one product and exact zeros through every fma chain);
  * apad_wav_stats on dyadic samples: ``torch.equal`` with float32(float64 sum / n) and float32(0.5) / max(hi - mean, mean - lo) in fp32;
  * every entry expected at a floor (logf(1e-5f), -100 dB, a zero chroma row, the (0 - norm_mean) * inv_2std padding rows): every bit;
  * every other entry: |out - expected| <= its own derived bound (spectral_cases' docstring).
Every case runs with the clip between two all-NaN clips of its ragged batch, or as a view into a NaN-filled buffer, after ``nan_fill_free``: the
output must be finite, and for the batched kernels bit-equal to the same clip alone.

Every test records the largest error it saw over its bound and the device logarithm's error against the fp64 logarithm of the restatement's
argument; ``test_zz_figures`` prints them (-s)."""
import math

import numpy as np
import pytest
import torch

import spectral_cases as SC
from util import assert_bits_equal, nan_fill_free, nan_neighbours, nan_surrounded

pytestmark = pytest.mark.gpu

FIGURES = {}


@pytest.fixture(autouse=True)
def _stale_results_read_as_nan(dev):
    """every test starts with the allocator's free blocks NaN-filled (see tests/test_gpu_kernels.py)"""
    nan_fill_free(dev)


def _note(key, value):
    FIGURES[key] = max(FIGURES.get(key, 0.0), float(value))


def _compare(out, b, what):
    """out [rows, R] fp32 GPU against the built case: exact entries in every bit, the others within their bound"""
    sp = b.sp
    o = out.detach().cpu()
    assert o.dtype == torch.float32 and tuple(o.shape) == b.expect.shape, (what, o.dtype, tuple(o.shape), b.expect.shape)
    assert bool(torch.isfinite(o).all()), f"{what}: non-finite output"
    o64 = o.double().numpy()
    exact = b.exact
    want = torch.from_numpy(b.expect.astype(np.float32))
    if exact.any():
        m = torch.from_numpy(exact)
        assert_bits_equal(torch.where(m, o, torch.zeros_like(o)), torch.where(m, want, torch.zeros_like(o)), f"{what} (entries at the floor)")
    err = np.abs(o64 - b.expect)
    ratio = np.where(exact, 0.0, err / np.where(exact, 1.0, b.bound))
    _note(f"{sp.kind}: max error / bound", ratio.max())
    _note(f"{sp.kind}: max error", np.where(exact, 0.0, err).max())
    _note(f"{sp.kind}: max bound", b.bound.max())
    Fl = b.live_frames
    if sp.kind != "chroma" and Fl and b.e32 is not None:  # the measured term: the device logarithm against log64 of the restatement's argument
        # (on the well-conditioned entries: those whose derived part allows at most 3e-5 of relative error on the logarithm's argument)
        unit = 1.0 if sp.kind == "mel" else 10.0 / math.log(10.0) if sp.kind == "clap" else sp.inv_2std
        live = b.live[:Fl] & ~exact[:Fl] & (b.bound[:Fl] - SC.LOG_TOL[sp.kind] <= 3e-5 * unit)
        if live.any():
            _note(f"{sp.kind}: max |out - log64(restated argument)|", np.abs(o64[:Fl] - SC.post64(sp, b.e32.astype(np.float64)))[live].max())
    if ratio.max() > 1.0:
        r, c = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
        raise AssertionError(f"{what}: {int((ratio > 1).sum())} of {ratio.size} entries leave their bound; worst at (row {r}, column {c}): expected "
                             f"{b.expect[r, c]!r}, got {o64[r, c]!r}, error {err[r, c]:.3e}, bound {b.bound[r, c]:.3e}")


# ---- 1. apad_resample_fir ----
@pytest.mark.parametrize("name", [c.name for c in SC.RESAMPLE_CASES])
def test_resampler_of_an_impulse_is_its_table(dev, name):
    from ap_adapter_amd import frontend as FE
    c = SC.RESAMPLE_BY_NAME[name]
    kern, width, orig, new = SC.resample_table(*c.rates)
    x = SC.impulses(c.n, c.marks)
    want, hits = SC.resample_expect(x, kern, width, orig, new)
    assert hits.max() <= 1
    view = nan_surrounded(x, dev).view(1, -1)
    nan_fill_free(dev)
    out = FE.resample(view, *c.rates)
    assert tuple(out.shape) == (1, math.ceil(new * c.n / orig))
    assert_bits_equal(out[0], torch.from_numpy(want), name)
    assert not bool(torch.signbit(out[0][out[0] == 0]).any()), "a zero output is +0.0"


# ---- 2. apad_wav_stats ----
def _logmel(dev, clips, segment, target, fill=True):
    """frontend.logmel_launch on a ragged batch of fp32 GPU clips -> (stats [B, 2], out [B, target, 64])"""
    from ap_adapter_amd import frontend as FE
    offsets_host = torch.zeros(len(clips) + 1, dtype=torch.int64)
    offsets_host[1:] = torch.cumsum(torch.tensor([c.numel() for c in clips], dtype=torch.int64), 0)
    packed = torch.cat(clips)
    offsets = offsets_host.to(dev)
    if fill:
        nan_fill_free(dev)
    stats = torch.empty(len(clips), 2, dtype=torch.float32, device=dev)
    out = torch.empty(len(clips), target, 64, dtype=torch.float32, device=dev)
    FE.logmel_launch(packed, offsets, offsets_host, stats, out, segment, target)
    return stats, out


@pytest.mark.parametrize("n", SC.STATS_N)
def test_wav_stats_of_dyadic_samples(dev, n):
    """(fp32 division as hipcc compiles it by default: correctly rounded.  The MI355X agrees in every bit.)"""
    x = SC.dyadic_clip(n, n)
    mean, scale = SC.stats_expect(x)
    alone, _ = _logmel(dev, [torch.from_numpy(x).to(dev)], 800, 5)
    assert_bits_equal(alone[0], torch.tensor([mean, scale]), f"stats n={n}")
    batch, _ = _logmel(dev, nan_neighbours(x, dev), 800, 5)
    assert_bits_equal(batch[1], alone[0], f"stats n={n} between NaN clips")


def test_wav_stats_of_a_constant_clip(dev):
    x = np.full(1025, 0.25, np.float32)
    stats, out = _logmel(dev, nan_neighbours(x, dev), 800, 5)
    assert_bits_equal(stats[1], torch.tensor([0.25, 0.0]), "constant clip")
    floor = torch.full((5, 64), float(SC.floor_value(SC.spec("mel"))))
    assert_bits_equal(out[1], floor, "constant clip: every entry at the floor")


# ---- 3. apad_stft_logmel ----
def _mel_check(dev, c, fill=True):
    b = SC.mel_build(c)
    x = torch.from_numpy(b.x).to(dev)
    stats, alone = _logmel(dev, [x], c.segment, c.target, fill)
    assert_bits_equal(stats[0], torch.tensor([0.0, 1.0]), f"{c.name}: the normalisation is the identity")
    _compare(alone[0], b, c.name)
    stats3, batch = _logmel(dev, nan_neighbours(b.x, dev), c.segment, c.target, fill)
    assert_bits_equal(stats3[1], stats[0], f"{c.name}: stats between NaN clips")
    assert_bits_equal(batch[1], alone[0], f"{c.name}: between NaN clips")


@pytest.mark.parametrize("name", [c.name for c in SC.MEL_CASES])
def test_stft_logmel(dev, name):
    _mel_check(dev, SC.MEL_BY_NAME[name])


def test_stft_logmel_tone_at_every_filter_s_peak(dev):
    """every Slaney row live under its own tone and at logf(1e-5f), bit for bit, under the others' (the free blocks are NaN-filled once, by the
    fixture: 64 tones in one test)"""
    for c in SC.MEL_SWEEP:
        _mel_check(dev, c, fill=False)


# ---- 4. apad_kaldi_fbank ----
def _fbank_check(dev, c, fill=True):
    from ap_adapter_amd import frontend as FE
    b = SC.fbank_build(c)
    view = nan_surrounded(b.x, dev).view(1, -1)
    if fill:
        nan_fill_free(dev)
    out = FE.extract_kaldi_fbank_feature(view, 16000, torch.zeros(SC.FBANK_TARGET, 128), device=dev)
    _compare(out, b, c.name)


@pytest.mark.parametrize("name", [c.name for c in SC.FBANK_CASES])
def test_kaldi_fbank(dev, name):
    _fbank_check(dev, SC.FBANK_BY_NAME[name])


def test_kaldi_fbank_tone_under_every_filter(dev):
    for c in SC.FBANK_SWEEP:
        _fbank_check(dev, c, fill=False)


# ---- 5. apad_clap_logmel ----
_EXTRACTORS = {}


def _extractor(config):
    from ap_adapter_amd.clap_features import ClapFeatureExtractor
    if config not in _EXTRACTORS:
        _EXTRACTORS[config] = ClapFeatureExtractor(feature_size=config[0], frequency_max=config[1], truncation="rand_trunc")
    return _EXTRACTORS[config]


@pytest.mark.parametrize("name", [c.name for c in SC.CLAP_CASES])
def test_clap_logmel(dev, name):
    c = SC.CLAP_BY_NAME[name]
    for config in c.configs:
        b = SC.clap_build(c, config)
        fe = _extractor(config)
        kw = dict(padding=c.padding, max_length=SC.CLAP_MAX, sampling_rate=48000)
        nan_fill_free(dev)
        alone = fe([torch.from_numpy(b.x).to(dev)], crop_starts=[c.start], **kw).input_features
        assert tuple(alone.shape) == (1, 1, SC.CLAP_MAX // SC.CLAP_HOP + 1, config[0])
        _compare(alone[0, 0], b, f"{name} {config}")
        clips = nan_neighbours(b.x, dev)
        nan_fill_free(dev)
        batch = fe(clips, crop_starts=[0, c.start, 0], **kw).input_features
        assert_bits_equal(batch[1, 0], alone[0, 0], f"{name} {config}: between NaN clips")


# ---- 6. apad_chroma ----
def _chroma(dev, clips, T):
    from ap_adapter_amd import chroma as PC
    from ap_adapter_amd import ops
    offsets_host = torch.zeros(len(clips) + 1, dtype=torch.int64)
    offsets_host[1:] = torch.cumsum(torch.tensor([c.numel() for c in clips], dtype=torch.int64), 0)
    packed = torch.cat(clips)
    tables = PC.tables(dev)
    nan_fill_free(dev)
    out = torch.empty(len(clips), T, 12, dtype=torch.float32, device=dev)
    return ops.chroma(packed, offsets_host.to(dev), offsets_host, *tables, out)


@pytest.mark.parametrize("name", [c.name for c in SC.CHROMA_CASES])
def test_chroma(dev, name):
    c = SC.CHROMA_BY_NAME[name]
    b = SC.chroma_build(c)
    T = c.n // 512 + 1
    alone = _chroma(dev, [torch.from_numpy(b.x).to(dev)], T)
    _compare(alone[0], b, name)
    if c.family == "impulse":  # the same row in every frame that holds the impulse, whatever the window weight: to the bound, both ways
        held = sorted(SC.chroma_frames_holding(c.marks[0][0], c.n))
        rows = alone[0][held].double().cpu().numpy()
        assert (np.abs(rows - rows[:1]) <= 2 * b.bound[held].max(axis=0, keepdims=True)).all()
    batch = _chroma(dev, nan_neighbours(b.x, dev, before=700, after=513), max(T, 2))
    assert_bits_equal(batch[1, :T], alone[0], f"{name}: between NaN clips")
    assert not bool(batch[1, T:].any()), "rows past the clip's frames are zero"


def test_zz_figures():
    """the figures of the run (-s prints them); the logarithm's measured term must keep the factor of 4 that LOG_TOL was set with"""
    for k in sorted(FIGURES):
        print(f"FIGURE {k} = {FIGURES[k]:.4e}")
    for kind in ("mel", "clap", "fbank"):
        seen = FIGURES.get(f"{kind}: max |out - log64(restated argument)|")
        if seen is not None:
            assert 4.0 * seen <= SC.LOG_TOL[kind] * 1.05, (kind, seen, SC.LOG_TOL[kind])
