"""CPU: the conditions under which the cases of tests/spectral_cases.py determine what tests/test_gpu_exact_spectral.py asserts.

  * every expectation agrees with the oracle the project already trusts for that kernel, on the same samples: tests/vae_mel_oracle.py,
    tests/chroma_oracle.py to 1e-9.  The installed transformers ClapFeatureExtractor computes in complex64 / float32, so CLAP has two ties: to
    the installed extractor end to end (padding modes and crops included) within the fp32 rounding of its features, 100 x 2^-23 dB, and at
    1e-9 to an fp64 chain of trusted pieces (numpy's reflect pad and rfft, vae_mel_oracle's window, the installed fp64 Slaney bank).
    oracle/fbank.py computes in fp32 and is tied within twice the case's bound;
  * the closed forms: an impulse's log-mel is log(0.5 w[p] rowsum), a tone's log(A (128 W[k-1] + 256 W[k] + 128 W[k+1])), the resampler of an
    impulse is its table;
  * ``restate32`` (fp32 numpy in the kernels' order) stays inside every case's bound, and its leaked energy stays 8 x below the floor wherever
    the floor is expected; the frames a case is built for hold no entry within 8 x of the floor (fbank excepted: kaldi's pre-emphasis puts a
    spectral null under its lowest filters, see spectral_cases.fbank_edge_only and the bound's clamp);
  * every case carries a mutation of the REFERENCE that moves an entry by 64 x its bound (cases whose prescribed position cannot show one are
    named by the *_edge_only rules and say why), and every kind of mutation clears 64 x somewhere in each kernel it applies to;
  * coverage: every Slaney and HTK filter row is live under some tone, and every Slaney row floored under another.  HTK rows are floored only
    where the derived bound certifies it (five of the 128: fbank's 400-sample frame is not bin-centred, see spectral_cases' docstring), and the
    chroma bank is dense (every class weighs every bin, the output is divided by its maximum): its rows are never floored, so for chroma the
    condition is that tones at bins 1023 and 1024 and impulses move every row.  Every reflect branch of the 1024-point kernel holds a marked
    sample, every CLAP padding mode has a seam inside a frame, bin N/2 is weighed where the docstring says."""
import math

import numpy as np
import pytest

import chroma_oracle as CO
import spectral_cases as SC
import vae_mel_oracle as MO
from oracle import fbank as OF

U = SC.U


def _restatement_holds(b):
    sp, Fl = b.sp, b.live_frames
    if not Fl:
        return 0.0
    out32 = SC.post64(sp, b.e32.astype(np.float64))
    exact, expect, bound = b.exact[:Fl], b.expect[:Fl], b.bound[:Fl]
    if sp.kind == "chroma":
        assert (b.e32[exact] == 0).all()
    else:
        assert (b.e32[exact].astype(np.float64) <= sp.floor / SC.FLOOR_ROOM).all(), "the restatement leaks into a floored entry"
    err = np.abs(out32 - expect)[~exact]
    assert (err <= bound[~exact]).all(), float((err / bound[~exact]).max())
    return float((err / bound[~exact]).max()) if err.size else 0.0


def _no_band_in_clean_frames(b):
    band = ~(b.floor | b.live)
    assert not band[b.clean].any(), f"{int(band[b.clean].sum())} entries within {SC.FLOOR_ROOM} x of the floor"


def _mutants_clear(b, mutants, edge_only):
    ratios = {name: SC.mutation_ratio(b, m) for name, m in mutants}
    if not edge_only:
        assert ratios and max(ratios.values()) >= SC.MUTATION_FACTOR, ratios
    return {name.split("_", 1)[1] if name.startswith("row") else name for name, r in ratios.items() if r >= SC.MUTATION_FACTOR}


# ---- tables and the restated transform ----
@pytest.mark.parametrize("kind,args", [("mel", ()), ("clap", (64, 14000)), ("clap", (16, 26000)), ("chroma", ()), ("fbank", ())])
def test_fp32_operands_are_the_rounded_definition(kind, args):
    sp = SC.spec(kind, *args)
    assert np.abs(sp.window32 - sp.window64).max() <= U
    assert np.abs(sp.tw32 - sp.tw64).max() <= U
    assert (np.abs(sp.fb32 - sp.fb64) <= U * np.abs(sp.fb64) + 1e-15).all()
    y = np.random.RandomState(0).standard_normal((3, sp.N))
    re, im = SC.radix2(y, sp.log2n, sp.tw64)
    assert np.abs((re + 1j * im) - np.fft.fft(y, axis=1)).max() <= 1e-9
    assert SC.floor_value(sp).dtype == np.float32 and abs(float(SC.floor_value(sp)) - SC.exact_floor(sp)) <= SC.LOG_TOL[kind]


def test_nyquist_bin_is_weighed_where_the_cases_say():
    assert not SC.spec("mel").fb32[:, 512].any() and not SC.spec("clap", 64, 14000).fb32[:, 512].any()
    assert SC.spec("clap", 16, 26000).fb32[15, 512] > 5e-5 and SC.spec("chroma").fb32[:, 1024].max() > 0.1
    assert any(c.k == 512 for c in SC.CLAP_CASES if c.family == "tone") and any(c.k == 1024 for c in SC.CHROMA_CASES if c.family == "tone")


def test_tone_table_symmetries():
    for N in (512, 1024, 2048):
        t = SC.cos_table(N).astype(np.float64)
        assert t[0] == 1 and t[N // 4] == 0 and np.array_equal(t[1:], t[1:][::-1]) and np.array_equal(t[N // 2:], -t[:N // 2])
        assert np.abs(t - np.cos(2 * np.pi * np.arange(N) / N)).max() <= U
    for k in SC.mel_tone_bins() + tuple(SC.mel_sweep_bins()):
        x = SC.tone(k, 4096, 0.5, 1024).astype(np.float64)
        assert x.sum() == 0.0 and x.max() == 0.5 and x.min() == -0.5


# ---- 1. resampler ----
@pytest.mark.parametrize("name", [c.name for c in SC.RESAMPLE_CASES])
def test_resampler_expectation(name):
    c = SC.RESAMPLE_BY_NAME[name]
    kern, width, orig, new = SC.resample_table(*c.rates)
    x = SC.impulses(c.n, c.marks)
    out, hits = SC.resample_expect(x, kern, width, orig, new)
    assert hits.max() <= 1 and hits.sum() > 0, "every output's taps reach at most one impulse"
    assert out.shape[0] == math.ceil(new * c.n / orig)
    assert np.array_equal(out, OF.resample(x, *c.rates)), "the oracle's matrix product of one non-zero term per row is exact too"
    # one phase's taps shifted by one: among the two outputs that read the impulse through the largest taps (the peak of a symmetric
    # kernel can have an equal neighbour) one changes
    changed = []
    for i in np.argsort(-np.abs(out))[:2]:
        moved = kern.copy()
        moved[i % new] = np.roll(kern[i % new], 1)
        changed.append(not np.array_equal(SC.resample_expect(x, moved, width, orig, new)[0], out))
    assert any(changed)


# ---- 2. apad_wav_stats ----
@pytest.mark.parametrize("n", SC.STATS_N)
def test_stats_expectation(n):
    x = SC.dyadic_clip(n, n)
    assert np.array_equal(x * 1024, np.round(x * 1024)) and np.abs(x).max() <= 1
    mean, scale = SC.stats_expect(x)
    y = (x.astype(np.float64) - float(mean)) * float(scale)
    assert abs(np.abs(MO.normalize(x)).max() - 0.5) == 0 and np.abs(y - MO.normalize(x)).max() <= 4 * U
    assert SC.stats_expect(np.full(n, 0.25, np.float32)) == (np.float32(0.25), np.float32(0.0))


# ---- 3. apad_stft_logmel ----
def _mel_oracle(x, segment, target):
    return MO.pad_spec(MO.log_mel(MO.pad_wav(MO.normalize(x), segment)), target)


@pytest.mark.parametrize("name", [c.name for c in SC.MEL_CASES])
def test_mel_case(name):
    c = SC.MEL_BY_NAME[name]
    b = SC.mel_build(c)
    sp, x = b.sp, b.x.astype(np.float64)
    assert SC.stats_expect(b.x) == (np.float32(0.0), np.float32(1.0)) and np.array_equal(MO.normalize(x), x)
    ref = _mel_oracle(x, c.segment, c.target)
    assert np.abs(ref - b.expect)[~b.exact].max() <= 1e-9 and np.abs(ref - b.expect)[b.exact].max() <= SC.LOG_TOL["mel"]
    Fl = b.live_frames
    if c.family == "pair":  # the closed form: 0.5 w[p] in every bin (agrees with the oracle to 1e-15 relative)
        idx = SC.mel_index(c.n, c.segment, c.target)[0]
        for f in np.nonzero(b.clean)[0]:
            p = int(np.nonzero(SC.gather(b.x, idx[f:f + 1])[0])[0][0])
            closed = np.log(0.5 * sp.window64[p] * sp.fb64.sum(axis=1))
            assert np.abs(closed - b.expect[f]).max() <= 1e-12 and np.abs(closed - ref[f]).max() <= 1e-12
    if c.family == "tone":
        W, k = sp.fb64, c.k
        closed = 0.5 * (128 * W[:, k - 1] + 256 * W[:, k] + 128 * W[:, k + 1])
        touched = closed > 0
        assert b.clean.sum() >= 10
        for f in np.nonzero(b.clean)[0]:
            assert np.array_equal(b.floor[f], ~touched)
            assert np.abs(np.log(closed[touched]) - b.expect[f][touched]).max() <= 1e-6  # (the samples are the cosine rounded to fp32)
    _restatement_holds(b)
    _no_band_in_clean_frames(b)
    _mutants_clear(b, SC.mel_mutants(c), False)


def test_mel_mutations_and_branches_are_all_exercised():
    kinds, branches = set(), dict(left=False, right=False, both=False, cut=False)
    for c in SC.MEL_CASES:
        b = SC.mel_build(c)
        kinds |= _mutants_clear(b, SC.mel_mutants(c), False)
        if c.family == "pad":
            for name in branches:
                branches[name] |= b.branches[name]
    assert kinds >= {"impulse_-1", "impulse_+1", "reflect_repeats_edge", "first_bin_dropped", "last_bin_dropped", "neighbour_twiddle"}, kinds
    assert all(branches.values()), branches


def test_every_slaney_row_is_live_under_one_tone_and_floored_under_another():
    live, floored = np.zeros(64, bool), np.zeros(64, bool)
    for c in SC.MEL_SWEEP:
        b = SC.mel_build(c)
        _restatement_holds(b)
        _no_band_in_clean_frames(b)
        live |= b.live[b.clean].all(axis=0)
        floored |= b.floor[b.clean].all(axis=0)
    assert live.all() and floored.all()


# ---- 4. apad_kaldi_fbank ----
@pytest.mark.parametrize("name", [c.name for c in SC.FBANK_CASES])
def test_fbank_case(name):
    c = SC.FBANK_BY_NAME[name]
    b = SC.fbank_build(c)
    assert b.live_frames == (0 if c.n < 400 else min(SC.FBANK_TARGET, 1 + (c.n - 400) // 160))
    ref = OF.extract_kaldi_fbank_feature(b.x[None], 16000, target_len=SC.FBANK_TARGET).astype(np.float64)
    err = np.abs(ref - b.expect)
    assert (err[~b.exact] <= 2 * b.bound[~b.exact] + 1e-6).all() and (err[b.exact] <= 1e-6 + SC.LOG_TOL["fbank"]).all(), float(err.max())
    _restatement_holds(b)
    _mutants_clear(b, SC.fbank_mutants(c), SC.fbank_edge_only(c))


def test_fbank_mutations_and_rows_are_all_exercised():
    kinds = set()
    for c in SC.FBANK_CASES:
        kinds |= _mutants_clear(SC.fbank_build(c), SC.fbank_mutants(c), SC.fbank_edge_only(c))
    assert kinds >= {"impulse_-1", "impulse_+1", "first_bin_dropped", "last_bin_dropped", "neighbour_twiddle"}, kinds
    live, floored = np.zeros(128, bool), np.zeros(128, bool)
    for c in SC.FBANK_SWEEP:
        b = SC.fbank_build(c)
        _restatement_holds(b)
        live |= b.live.all(axis=0)
        floored |= b.floor.all(axis=0)
    empty = ~SC.spec("fbank").fb32.any(axis=1)  # kaldi's bank has one row between two bins of the 512-point transform: always at the floor
    assert list(np.nonzero(empty)[0]) == [3] and live[~empty].all()
    # floored under another tone: only what the derived bound certifies (a 400-sample frame leaks into every bin of the 512-point transform, and
    # the worst-case count of that leak exceeds eps / 8 under all but the narrowest low filters far from the tone): the empty row and a few more
    assert floored[3] and floored.sum() >= 3


# ---- 5. apad_clap_logmel ----
@pytest.mark.parametrize("name", [c.name for c in SC.CLAP_CASES])
def test_clap_case(name):
    import clap_feature_models as CF
    c = SC.CLAP_BY_NAME[name]
    for config in c.configs:
        b = SC.clap_build(c, config)
        sp = b.sp
        # the installed extractor end to end (fp32 features): its own padding, repeat and crop
        ref = CF.reference(sp.installed, [b.x], c.padding, SC.CLAP_MAX, [c.start])[0, 0].double().numpy()
        assert np.abs(ref - b.expect).max() <= 100 * 2.0 ** -23, float(np.abs(ref - b.expect).max())
        # its fp64 spectrogram of the max_length samples this file's index map selects
        j = np.arange(SC.CLAP_MAX)
        limit = SC.CLAP_MAX if c.n > SC.CLAP_MAX or c.padding == "repeat" else (c.n if c.padding == "pad" else (SC.CLAP_MAX // c.n) * c.n)
        framed = np.where(j < limit, b.x.astype(np.float64)[(c.start + j if c.n > SC.CLAP_MAX else j % c.n)], 0.0)
        # an fp64 chain from the pieces the project already trusts (the installed extractor itself computes in complex64 / float32):
        # numpy's reflect pad and rfft, vae_mel_oracle's periodic Hann window, the installed fp64 Slaney bank, power_to_db's formula
        padded = np.pad(framed, 512, mode="reflect")
        fr = padded[SC.CLAP_HOP * np.arange(SC.CLAP_MAX // SC.CLAP_HOP + 1)[:, None] + np.arange(1024)[None, :]]
        power = np.abs(np.fft.rfft(fr * MO.hann_periodic(1024)[None, :], axis=1)) ** 2
        ref64 = 10.0 * np.log10(np.maximum(power @ np.asarray(sp.installed.mel_filters_slaney, np.float64), 1e-10))
        assert np.abs(ref64 - b.expect).max() <= 1e-9, float(np.abs(ref64 - b.expect).max())
        _restatement_holds(b)
        _no_band_in_clean_frames(b)
        _mutants_clear(b, SC.clap_mutants(c, config), SC.clap_edge_only(c))
        if c.family == "tone":
            assert b.clean.any() and b.floor[b.clean].any() and b.live[b.clean].any()


def test_clap_mutations_and_seams_are_all_exercised():
    kinds, seams = set(), set()
    for c in SC.CLAP_CASES:
        for config in c.configs:
            b = SC.clap_build(c, config)
            kinds |= _mutants_clear(b, SC.clap_mutants(c, config), SC.clap_edge_only(c))
            if b.seam_in_frame:
                seams.add(c.padding)
    assert kinds >= {"impulse_-1", "impulse_+1", "reflect_repeats_edge", "seam_one_off", "first_bin_dropped", "last_bin_dropped",
                     "neighbour_twiddle", "nyquist_bin_dropped"}, kinds
    assert seams == {"repeatpad", "repeat", "pad"}


# ---- 6. apad_chroma ----
@pytest.mark.parametrize("name", [c.name for c in SC.CHROMA_CASES])
def test_chroma_case(name):
    c = SC.CHROMA_BY_NAME[name]
    b = SC.chroma_build(c)
    ref = CO.chroma(b.x).numpy()
    assert np.abs(ref - b.expect).max() <= 1e-9
    top = b.e.max(axis=1)
    assert ((top == 0) | (top > 1e-30)).all(), "no frame near the smallest normal number"
    if c.family == "impulse":  # a flat power spectrum: the same row wherever the impulse is read
        row = b.sp.fb64.sum(axis=1) / b.sp.fb64.sum(axis=1).max()
        held = sorted(SC.chroma_frames_holding(c.marks[0][0], c.n))
        assert held and np.array_equal(np.nonzero(top > 0)[0], np.array(held))
        assert np.abs(b.expect[held] - row[None]).max() <= 1e-12
    _restatement_holds(b)
    _mutants_clear(b, SC.chroma_mutants(c), SC.chroma_edge_only(c))


def test_chroma_mutations_are_all_exercised():
    kinds = set()
    for c in SC.CHROMA_CASES:
        kinds |= _mutants_clear(SC.chroma_build(c), SC.chroma_mutants(c), SC.chroma_edge_only(c))
    assert kinds >= {"impulse_-1", "impulse_+1", "nyquist_bin_dropped", "neighbour_twiddle"}, kinds


def test_the_bound_is_the_docstring_s_count():
    sp = SC.spec("mel")
    assert abs(sp.G - (2 + 8 * (math.sqrt(5) + 1) + 10)) < 1e-12 and 37 < sp.G < 38.5
    assert sp.steps.max() == math.ceil(int((sp.ranges[:, 1] - sp.ranges[:, 0]).max()) / 4) + 3
    # the derived part on the cases' own frames: every entry of an impulse pair stays below the 1e-5 the issue names for the mel kernels.  A
    # tone's does not quite: the transform's error is absolute (||dX||_2 <= Gn u sqrt N ||y||_2 = 5.0e-4 at A = 0.5), and the Slaney
    # normalisation makes the high filters weak (row 63: energy 0.68 under a tone at its peak), so the filter the tone sits on is bounded by 2e-6
    # (row 0) to 1.8e-5 (row 63).  The count was taken twice (bin-wise and in the 2-norm, spectral_cases' docstring); this is what it gives.
    pair = tone = 0.0
    for c in SC.MEL_CASES + SC.MEL_SWEEP:
        b = SC.mel_build(c)
        B = b.bound[:b.live_frames][b.clean] - SC.LOG_TOL["mel"]
        if c.family == "pair":
            pair = max(pair, float(B.max()))
        elif c in SC.MEL_SWEEP:  # (a tone at a filter's peak)
            tone = max(tone, float(B[np.arange(B.shape[0]), b.e[b.clean].argmax(axis=1)].max()))
    assert 1e-6 < pair <= 1e-5 and 1e-6 < tone <= 2e-5, (pair, tone)
