"""-m gpu: ap_adapter_amd.ClapFeatureExtractor (apad_clap_logmel) against the INSTALLED transformers ClapFeatureExtractor
(truncation="rand_trunc", numpy float64) on the same fp32 samples, the fused resampling against apad_resample_fir bit for bit, and the
ranking path of the pipeline on it.

Two tiers (tests/clap_feature_models.py): A = |ours - ref| in dB where the reference is within 60 dB of its frame's maximum, B =
|10^(ours/10) - 10^(ref/10)| relative to the frame's maximum mel power, everywhere.  TOL_A / TOL_B are 4 x the maxima of
test_parity_small measured on the MI355X, rounded up to one digit: 2.29e-5 dB (three fp32 steps of a value near
-70 dB) and 8.78e-7.  Every comparison prints its figures before it asserts."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import clap_audio_models as M
import clap_feature_models as F
from util import nan_fill_free, rel_err

pytestmark = pytest.mark.gpu

TOL_A = 1e-4   # dB (must stay below 1e-3 dB: more than that is wrong arithmetic, not rounding)
TOL_B = 4e-6   # of the frame's maximum mel power
ML = 4800
SMALL_N = (300, 1000, 4800, 6000, 6000)
SMALL_STARTS = [None, None, None, 0, 1200]
PADDINGS = ["repeatpad", "repeat", "pad"]


def small_clips():
    c = [F.signal(n, 100 + k) for k, n in enumerate(SMALL_N[:4])]
    return c + [c[3]]  # the 6000-sample clip twice: crop starts 0 and 1200


def check_parity(out, ref, what):
    assert out.shape == ref.shape and out.dtype == torch.float32 and torch.isfinite(out).all()
    a, b = F.tier_errors(out, ref)
    cov = F.tier_a_coverage(ref)
    print(f"{what}: tier A max |dB diff| {a:.3e} (covers {cov:.4f} of the live entries), tier B max power diff / frame max {b:.3e}")
    assert cov >= 0.95
    silent = F.silent_frames(ref)
    assert bool((out.cpu()[:, 0][silent] == -100.0).all())
    assert a <= TOL_A
    assert b <= TOL_B
    return int(silent.sum())


_ref_cache = {}


def small_reference(fs, padding):
    if (fs, padding) not in _ref_cache:
        _ref_cache[fs, padding] = F.reference(F.installed(feature_size=fs), small_clips(), padding, ML, SMALL_STARTS)
    return _ref_cache[fs, padding]


@pytest.mark.parametrize("padding", PADDINGS)
@pytest.mark.parametrize("fs", [64, 16])
def test_parity_small(dev, fs, padding):
    """max_length 4800 (11 frames), a ragged batch of 300 / 1000 / 4800 / 6000 / 6000 samples at 48 kHz (crop starts 0 and 1200): the
    300-sample clip's reflect pad reaches across repeat seams, the pad mode's tail frames are all zero and give exactly -100"""
    import ap_adapter_amd as A
    fe = A.ClapFeatureExtractor(feature_size=fs, truncation="rand_trunc")
    nan_fill_free(dev)
    got = fe([torch.from_numpy(c) for c in small_clips()], padding=padding, max_length=ML, sampling_rate=48000, crop_starts=SMALL_STARTS)
    assert got.is_longer == [[False], [False], [False], [True], [True]]
    out = got.input_features
    assert out.shape == (5, 1, 11, fs) and out.is_cuda
    ref = small_reference(fs, padding)
    nsilent = check_parity(out, ref, f"small feature_size={fs} {padding}")
    if padding == "pad":
        assert nsilent >= 9 + 7  # the 300-sample clip's frames 2.., the 1000-sample clip's frames 4..
    assert not torch.equal(out[3], out[4])  # the crop start is live


def test_parity_real_size(dev):
    """the default extractor (1001 frames): a 10.24 s clip cropped at the last valid start and a clip of exactly max_length"""
    import ap_adapter_amd as A
    clips = [F.signal(491520, 7), F.signal(480000, 8)]
    fe = A.ClapFeatureExtractor(truncation="rand_trunc")
    nan_fill_free(dev)
    got = fe([torch.from_numpy(c) for c in clips], sampling_rate=48000, crop_starts=[11520, None])
    assert got.is_longer == [[True], [False]] and got.input_features.shape == (2, 1, 1001, 64)
    ref = F.reference(F.installed(), clips, "repeatpad", 480000, [11520, None])
    check_parity(got.input_features, ref, "real size")
    with pytest.raises(ValueError, match="crop_starts"):
        fe([torch.from_numpy(clips[0])], sampling_rate=48000, crop_starts=[11521])


@pytest.mark.parametrize("padding", PADDINGS)
@pytest.mark.parametrize("rate,lengths,starts", [(16000, (101, 1601, 10240), [None, 3, 1234]), (44100, (4410, 1000, 4411), [None, None, 1])])
def test_fused_resampling_is_the_unfused_one(dev, rate, lengths, starts, padding):
    """source_sampling_rate=rate against frontend.resample(rate -> 48000) followed by the extractor with no resampling: bit-equal.
    Pins the zero-padded clip edges, the repeat seams and the ceil length (1601 samples at 16 kHz are 4803 at 48 kHz: 3 too long;
    4411 at 44.1 kHz are 4802) without a tolerance."""
    import ap_adapter_amd as A
    from ap_adapter_amd import frontend
    fe = A.ClapFeatureExtractor(truncation="rand_trunc")
    clips = [torch.from_numpy(F.signal(n, 200 + k, sr=rate)).to(dev) for k, n in enumerate(lengths)]
    resampled = [frontend.resample(c[None].contiguous(), rate, 48000)[0] for c in clips]
    assert [r.numel() for r in resampled] == [-(-n * 48000 // rate) for n in lengths]
    nan_fill_free(dev)
    fused = fe(clips, padding=padding, max_length=ML, sampling_rate=48000, source_sampling_rate=rate, crop_starts=starts)
    plain = fe(resampled, padding=padding, max_length=ML, sampling_rate=48000, crop_starts=starts)
    assert fused.is_longer == plain.is_longer == [[r.numel() > ML] for r in resampled]
    assert torch.isfinite(fused.input_features).all() and float(fused.input_features.max()) > -50.0
    assert torch.equal(fused.input_features, plain.input_features)


@pytest.mark.parametrize("padding", PADDINGS)
def test_batch_independence(dev, padding):
    """each clip of the ragged batch alone is bit-equal to its rows in the batch"""
    import ap_adapter_amd as A
    fe = A.ClapFeatureExtractor(truncation="rand_trunc")
    clips = [torch.from_numpy(c).to(dev) for c in small_clips()]
    whole = fe(clips, padding=padding, max_length=ML, sampling_rate=48000, crop_starts=SMALL_STARTS).input_features
    for b, c in enumerate(clips):
        nan_fill_free(dev)
        alone = fe([c], padding=padding, max_length=ML, sampling_rate=48000, crop_starts=[SMALL_STARTS[b]]).input_features
        assert torch.equal(alone[0], whole[b]), b
    # a rectangular GPU tensor is the same batch
    both = fe(torch.stack(clips[3:]), padding=padding, max_length=ML, sampling_rate=48000, crop_starts=SMALL_STARTS[3:]).input_features
    assert torch.equal(both, whole[3:])


def test_entry_point_refuses_bad_operands(dev):
    import ap_adapter_amd as A
    fe = A.ClapFeatureExtractor(truncation="rand_trunc")
    x = [torch.zeros(1000, device=dev)]
    with pytest.raises(RuntimeError, match="max_length"):
        A.clap_features.clap_logmel_launch(x[0], torch.tensor([0, 1000], device=dev), torch.tensor([0, 1000]), torch.zeros(1, dtype=torch.int64, device=dev),
                                           torch.zeros(1, dtype=torch.int64), (None, 0, 1, 1), fe.tables(dev), torch.empty(1, 1, 2, 64, device=dev), 512, 480,
                                           "repeatpad")
    with pytest.raises(RuntimeError, match="crop start"):
        A.clap_features.clap_logmel_launch(x[0], torch.tensor([0, 1000], device=dev), torch.tensor([0, 1000]), torch.zeros(1, dtype=torch.int64, device=dev),
                                           torch.tensor([201]), (None, 0, 1, 1), fe.tables(dev), torch.empty(1, 1, 2, 64, device=dev), 800, 480, "repeatpad")
    with pytest.raises(RuntimeError, match="staged samples"):  # 8 : 1 down-sampling: the frame's source window exceeds the LDS budget
        fe(x, sampling_rate=48000, source_sampling_rate=384000)
    out = fe(x, sampling_rate=48000, max_length=ML).input_features
    assert bool((out == -100.0).all())  # silence is the floor, exactly


# ---- through the tower and the pipeline: the small tower of tests/clap_audio_models.py (16 mel bins, 251 frames) ----
CLIP_SEEDS = (300, 301, 302, 303, 304, 305)
CLIP_LENGTHS = (120000, 120000, 90000, 60000, 33333, 120000)  # 2.5 s and shorter at 48 kHz
BAR = M.TOL  # features -> tower: the bar the tower itself is held to against transformers


def test_through_the_tower(dev):
    """get_audio_features of our features against get_audio_features of the installed extractor's features, same HIP tower"""
    import ap_adapter_amd as A
    clips = [F.signal(n, s) for n, s in zip(CLIP_LENGTHS, CLIP_SEEDS)]
    fe = A.ClapFeatureExtractor(feature_size=16, max_length_s=2.5, truncation="rand_trunc")
    tower = M.ours(M.SMALL_CFG, M.SMALL_SEED).to(dev)
    out = fe([torch.from_numpy(c) for c in clips], sampling_rate=48000).input_features
    assert out.shape == (6,) + M.SMALL_SHAPE[1:]
    ref = F.reference(F.installed(feature_size=16, max_length_s=2.5), clips, "repeatpad", 120000)
    a, b = F.tier_errors(out, ref)
    e = rel_err(tower.get_audio_features(out), tower.get_audio_features(ref.to(dev)).cpu())
    print(f"through the tower: rel_err of the audio features {e:.3e} (the features: tier A {a:.3e} dB, tier B {b:.3e})")
    assert e < BAR


@pytest.fixture(scope="module")
def text_parts(dev):
    import ap_adapter_amd as A
    from text_models import CLAP_CFG, T5_CFG, Tok, load_text_gold, ours_from_gold
    tg = load_text_gold()
    enc = A.PromptEncoder(ours_from_gold(tg, "clap2", "clap", dev, heads=2), ours_from_gold(tg, "t5", "t5", dev),
                          ours_from_gold(tg, "proj", "proj", dev), ours_from_gold(tg, "gpt2", "gpt2", dev))
    tok1 = Tok(CLAP_CFG(2)["vocab_size"], CLAP_CFG(2)["pad_token_id"], 24, bos=0, eos=2)
    tok2 = Tok(T5_CFG["vocab_size"], 0, 32, eos=1)
    return dict(prompt_encoder=enc, tokenizer=tok1, tokenizer_2=tok2)


def test_score_waveforms_ranks_like_the_installed_chain(dev, text_parts, monkeypatch):
    """six 2.5 s candidates at 16 kHz.  Reference on the CPU: our resampled audio -> installed extractor -> installed audio and
    text modules (clap_audio_models.oracle_pipe_logits on those features)"""
    import ap_adapter_amd as A
    from ap_adapter_amd import frontend
    from text_models import PROMPTS
    n, P = 3, len(PROMPTS)
    cand = torch.from_numpy(np.stack([F.signal(40000, s, sr=16000) for s in CLIP_SEEDS]))
    wav48 = frontend.resample(cand.to(dev), 16000, 48000).cpu().numpy()
    feats = F.reference(F.installed(feature_size=16, max_length_s=2.5), list(wav48), "repeatpad", 120000)
    monkeypatch.setattr(M, "pipe_features", lambda: feats)
    ref = M.oracle_pipe_logits()
    tol = BAR + M.TOL
    srt = torch.sort(ref, dim=1, descending=True).values
    gap = float((srt[:, :n] - srt[:, 1:n + 1]).min())
    print(f"reference logits: smallest deciding gap {gap:.3e}, 100 x tolerance x max|ref| = {100 * tol * float(ref.abs().max()):.3e}")
    assert gap >= 100 * tol * float(ref.abs().max())
    order = torch.argsort(ref, dim=1, descending=True)[:, :n].reshape(-1)
    assert order.tolist() != list(range(P * n))
    fe = A.ClapFeatureExtractor(feature_size=16, max_length_s=2.5, truncation="rand_trunc")
    pipe = A.AudioLDM2Pipeline(None, vocoder=SimpleNamespace(config=SimpleNamespace(sampling_rate=16000)),
                               audio_tower=M.ours(M.SMALL_CFG, M.SMALL_SEED).to(dev), feature_extractor=fe, **text_parts)

    def no_resample(*a, **k):
        raise AssertionError("frontend.resample on the fused route")

    monkeypatch.setattr(frontend, "resample", no_resample)
    out = pipe.score_waveforms(text=PROMPTS, audio=cand, num_waveforms_per_prompt=n, device=dev, dtype=torch.float32)
    e = rel_err(pipe.last_logits_per_text, ref)
    print(f"score_waveforms logits_per_text: rel_err {e:.3e}")
    assert e < tol
    assert torch.equal(out, cand[order])
    # the device copy is what gets scored when it is handed over
    again = pipe.score_waveforms(text=PROMPTS, audio=cand, num_waveforms_per_prompt=n, device=dev, dtype=torch.float32, audio_device=cand.to(dev))
    assert torch.equal(again, out)


class _StubFeatures:
    sampling_rate = 48000

    def __init__(self):
        self.calls = []

    def __call__(self, audio, return_tensors="pt", sampling_rate=None):
        self.calls.append((len(audio), len(audio[0]), sampling_rate))
        return SimpleNamespace(input_features=M.pipe_features())


def test_pipeline_plumbing(dev, text_parts, monkeypatch):
    """the tiny-UNet call of test_pipeline_ranks_candidates_like_the_installed_clap with the new extractor: the candidates come back
    in the order of the pipeline's own logits, latent output never reaches the extractor, a stub extractor keeps the host path"""
    import ap_adapter_amd as A
    from ap_adapter_amd import clap_features as CF, synthetic
    from text_models import PROMPTS
    R = lambda *shape, seed: torch.randn(*shape, generator=torch.Generator().manual_seed(seed))
    dtype = torch.float32
    unet = A.AudioLDM2UNet2DConditionModel(A.UNetConfig(block_out_channels=(64, 128, 192, 256), attention_head_dim=4, norm_num_groups=16))
    A.install_ap_adapter(unet, None, scale=0.5)
    synthetic.init_synthetic_(unet, 100, w_std=0.05, bias_std=0.02, norm_jitter=0.1)
    torch.manual_seed(3)
    vae = A.AutoencoderKL(A.VaeConfig(block_out_channels=(32, 64, 64), layers_per_block=1, norm_num_groups=8)).to(dev, dtype)
    voc = A.SpeechT5HifiGan(A.HifiGanConfig(upsample_initial_channel=256, upsample_rates=(5, 4, 2, 2, 2), upsample_kernel_sizes=(16, 16, 8, 4, 4))).to(dev, dtype)
    tower = M.ours(M.SMALL_CFG, M.SMALL_SEED).to(dev)
    fe = A.ClapFeatureExtractor(feature_size=16, max_length_s=2.5, truncation="rand_trunc")
    parts = dict(vocoder=voc, vae=vae, **text_parts)
    pipe = A.AudioLDM2Pipeline(unet.to(dev, dtype), audio_tower=tower, feature_extractor=fe, **parts)
    n, P = 3, len(PROMPTS)
    B, Lt = P * n, 8
    e = dict(prompt_embeds=R(P, 16, 1024, seed=20), negative_prompt_embeds=R(P, 16, 1024, seed=21),
             generated_prompt_embeds=R(P, Lt, 768, seed=22), negative_generated_prompt_embeds=R(P, Lt, 768, seed=23),
             attention_mask=torch.ones(P, 16, dtype=torch.long), negative_attention_mask=torch.ones(P, 16, dtype=torch.long))
    kw = dict(prompt=PROMPTS, num_waveforms_per_prompt=n, num_inference_steps=2, audio_length_in_s=0.64, latents=R(B, 8, 16, 16, seed=24),
              use_graph=False, **e)
    seen, launches = {}, []
    score, launch = pipe.score_waveforms, CF.clap_logmel_launch

    def spy(**k):
        seen["audio"], seen["device_copy"] = k["audio"].clone(), k.get("audio_device")
        return score(**k)

    def count(*a, **k):
        launches.append(a[0].numel())
        return launch(*a, **k)

    pipe.score_waveforms = spy
    monkeypatch.setattr(CF, "clap_logmel_launch", count)
    out = pipe(output_type="pt", **kw).audios
    cand = seen["audio"]
    assert cand.shape == (B, int(0.64 * 16000)) and not cand.is_cuda and len({float(c.abs().sum()) for c in cand}) == B
    assert seen["device_copy"] is not None and seen["device_copy"].is_cuda and torch.equal(seen["device_copy"].float().cpu(), cand)
    assert launches == [B * int(0.64 * 16000)]  # one launch, from the 16 kHz samples
    logits = pipe.last_logits_per_text
    assert logits.shape == (P, B)
    order = torch.argsort(logits, dim=1, descending=True)[:, :n].reshape(-1).cpu()
    assert out.shape == (B, cand.shape[1]) and not out.is_cuda and torch.equal(out, cand[order])
    assert isinstance(pipe(output_type="np", **kw).audios, np.ndarray)  # the public return types stay
    # latent output is the reference's early exit: no scoring, no features
    launches.clear()
    lat = pipe(output_type="latent", **kw).audios
    assert lat.shape == (B, 8, 16, 16) and not launches
    # any other extractor object keeps the host path
    stub = _StubFeatures()
    pipe2 = A.AudioLDM2Pipeline(pipe.unet, audio_tower=tower, feature_extractor=stub, **parts)
    pipe2(output_type="pt", **kw)
    assert stub.calls == [(B, int(0.64 * 48000), 48000)] and not launches
    with pytest.raises(NotImplementedError, match=r"audio_tower=.*feature_extractor="):
        A.AudioLDM2Pipeline(pipe.unet, **parts)(output_type="pt", **kw)
