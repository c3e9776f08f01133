"""-m gpu: the CLAP audio tower on the HIP path (fp32) -- apad_window_attention and apad_clap_mel2img alone against torch restatements
of the module's operators, the whole tower against the installed transformers module's outputs (committed fixture, re-derived on the CPU
by tests/test_clap_audio_host.py; transformers is not imported here), and the pipeline's candidate ranking.

Every comparison prints its rel_err before asserting it against the bar of 5e-5."""
from types import SimpleNamespace

import pytest
import torch

import clap_audio_models as M
from util import nan_fill_free, rel_err

pytestmark = pytest.mark.gpu


def R(*shape, seed=0, std=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * std


WIN_CASES = [(2, 16, 16, 2, 0), (2, 16, 16, 2, 4), (1, 8, 8, 4, 0), (1, 16, 24, 2, 4)]


@pytest.mark.parametrize("B,H,W,heads,shift", WIN_CASES)
def test_window_attention_vs_torch(dev, B, H, W, heads, shift):
    """roll + window_partition + ClapAudioSelfAttention (bias, -100 shift mask, softmax, P.V) + window_reverse + roll back in float64;
    scores of order +-5, so that the mask decides the result"""
    from ap_adapter_amd import ops
    C = heads * 24
    qkv = R(B, H, W, 3 * C, seed=H * W + shift, std=2.2)  # q.k / sqrt(24) has std 2.2^2 ~ 5
    bias = R(heads, 64, 64, seed=7 + heads)
    ref = M.ref_window_attention(qkv, bias, heads, shift)
    if shift > 0:  # the mask matters on these inputs: without it the oracle moves by far more than the tolerance
        assert rel_err(M.ref_window_attention(qkv, bias, heads, shift, masked=False), ref) > 1000 * M.TOL
        assert rel_err(M.ref_window_attention(qkv, bias, heads, 0), ref) > 1000 * M.TOL
    qd, bd = qkv.view(-1, 3 * C).to(dev), bias.to(dev)
    nan_fill_free(dev)
    out = ops.window_attention(qd, bd, B, H, W, heads, shift)
    assert out.shape == (B * H * W, C) and torch.isfinite(out).all()
    err = rel_err(out.view(B, H, W, C), ref)
    print(f"window_attention B={B} {H}x{W} heads={heads} shift={shift}: rel_err {err:.3e}")
    assert err < M.TOL
    # the fp32 matmul precision setting does not reach this entry point: same bits under "high"
    ops.set_float32_matmul_precision("high")
    try:
        nan_fill_free(dev)
        again = ops.window_attention(qd, bd, B, H, W, heads, shift)
    finally:
        ops.set_float32_matmul_precision("highest")
    assert torch.equal(again, out)


def test_window_attention_envelope_is_an_error_not_a_launch(dev):
    from ap_adapter_amd import _lib as L, ops
    bias = torch.zeros(2, 64, 64, device=dev)
    ok = torch.zeros(16 * 16, 3 * 48, device=dev)
    for kw, what in ((dict(H=12, W=16, n=12 * 16), "multiples of 8"), (dict(H=16, W=20, n=16 * 20), "multiples of 8")):
        with pytest.raises(RuntimeError, match=what):
            ops.window_attention(torch.zeros(kw["n"], 3 * 48, device=dev), bias, 1, kw["H"], kw["W"], 2, 0)
    with pytest.raises(RuntimeError, match="shift 2 not supported"):
        ops.window_attention(ok, bias, 1, 16, 16, 2, 2)
    with pytest.raises(RuntimeError, match="head_dim 32 not supported"):
        ops.window_attention(torch.zeros(16 * 16, 3 * 64, device=dev), bias, 1, 16, 16, 2, 0)
    out = torch.empty(16 * 16, 48, device=dev)
    args = lambda window, dtype: (ok.data_ptr(), bias.data_ptr(), out.data_ptr(), 1, 16, 16, 2, 24, window, 0, dtype, ops._stream())
    assert L.lib().apad_window_attention(*args(7, L.F32)) == -1 and b"window 7" in L.lib().apad_last_error()
    assert L.lib().apad_window_attention(*args(8, L.BF16)) == -1 and b"fp32 only" in L.lib().apad_last_error()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.window_attention(ok.cpu(), bias.cpu(), 1, 16, 16, 2, 0)


@pytest.mark.parametrize("T,Fb,S", [(251, 16, 64), (256, 16, 64), (1001, 64, 256), (1024, 64, 256)])
def test_clap_mel2img_vs_torch(dev, T, Fb, S):
    """BatchNorm2d (eval, randomised statistics) + reshape_mel2img (bicubic align_corners=True stretch when T is short) + 4 x 4 unfold;
    B = 2 with different content per sample"""
    from ap_adapter_amd import ops
    x = M.features((2, 1, T, Fb), seed=T)
    w, b, mean, var = 1 + 0.1 * R(Fb, seed=1), 0.2 * R(Fb, seed=2), 0.3 * R(Fb, seed=3), 0.5 + torch.rand(Fb, generator=torch.Generator().manual_seed(4))
    ref = M.ref_mel2img(x, w, b, mean, var, 1e-5, S)
    D = lambda t: t.to(dev)
    args = D(x), D(w), D(b), D(mean), D(var)
    nan_fill_free(dev)
    out = ops.clap_mel2img(*args, 1e-5, S)
    assert out.shape == ref.shape == (2 * (S // 4) ** 2, 16) and torch.isfinite(out).all()
    err = rel_err(out, ref)
    print(f"clap_mel2img T={T} F={Fb}: rel_err {err:.3e}")
    assert err < M.TOL
    half = out.shape[0] // 2
    assert not torch.equal(out[:half], out[half:])
    # without the BatchNorm statistics the result is far off: the randomised statistics are live
    assert rel_err(ops.clap_mel2img(D(x), D(w), D(b), torch.zeros_like(D(mean)), torch.ones_like(D(var)), 1e-5, S), ref) > 1000 * M.TOL


def test_clap_mel2img_too_long_is_the_modules_value_error(dev):
    from ap_adapter_amd import ops
    z = lambda n: torch.ones(n, device=dev)
    with pytest.raises(ValueError, match="less than or equal to the swin input size"):
        ops.clap_mel2img(torch.zeros(1, 1, 257, 16, device=dev), z(16), z(16), z(16), z(16), 1e-5, 64)


@pytest.fixture(scope="module")
def gold():
    return M.load_gold()


@pytest.mark.parametrize("which", ["small", "real"])
def test_tower_vs_installed_transformers(dev, gold, which):
    """audio_embeds and pooler_output of the whole tower: the small model (16 x 16 tokens in 4 windows with a shifted block, one
    patch merging, a last stage of one window) on [3, 1, 251, 16] and the real ClapAudioConfig() on [2, 1, 1001, 64]"""
    cfg, seed, shape = (M.SMALL_CFG, M.SMALL_SEED, M.SMALL_SHAPE) if which == "small" else (M.REAL_CFG, M.REAL_SEED, M.REAL_SHAPE)
    m = M.ours(cfg, seed).to(dev)
    x = M.features(shape, seed + 7).to(dev)
    out = m(x)
    e_emb, e_pool = rel_err(out.audio_embeds, gold[which + ".embeds"]), rel_err(out.pooler_output, gold[which + ".pooler"])
    print(f"tower {which}: rel_err audio_embeds {e_emb:.3e} pooler_output {e_pool:.3e}")
    assert out.audio_embeds.shape == gold[which + ".embeds"].shape and out.pooler_output.shape == gold[which + ".pooler"].shape
    assert e_emb < M.TOL and e_pool < M.TOL
    ref_n = torch.nn.functional.normalize(gold[which + ".embeds"], dim=-1)
    assert rel_err(m.get_audio_features(x), ref_n) < M.TOL
    if which == "small":  # the bias tables are live: zeroing one moves the result
        with torch.no_grad():
            m.audio_model.audio_encoder.layers[0].blocks[1].attention.self.relative_position_bias_table.zero_()
        assert rel_err(m(x).audio_embeds, gold["small.embeds"]) > 100 * M.TOL


class _StubFeatures:
    """a feature extractor that returns seeded features whatever the audio (ClapFeatureExtractor truncates clips above 10 s at a
    random offset; the ranking test must not depend on that)"""
    sampling_rate = 48000

    def __init__(self):
        self.calls = []

    def __call__(self, audio, return_tensors="pt", sampling_rate=None):
        self.calls.append((len(audio), len(audio[0]), sampling_rate))
        return SimpleNamespace(input_features=M.pipe_features())


def test_pipeline_ranks_candidates_like_the_installed_clap(dev, gold):
    """prompt=[2 texts], num_waveforms_per_prompt=3, waveform output: the six candidates come back in the order argsort of the installed
    modules' logits_per_text gives on the same features (fixture), best three per prompt among ALL six"""
    import ap_adapter_amd as A
    from ap_adapter_amd import synthetic
    from text_models import CLAP_CFG, PROMPTS, T5_CFG, Tok, load_text_gold, ours_from_gold
    tg = load_text_gold()
    enc = A.PromptEncoder(ours_from_gold(tg, "clap2", "clap", dev, heads=2), ours_from_gold(tg, "t5", "t5", dev),
                          ours_from_gold(tg, "proj", "proj", dev), ours_from_gold(tg, "gpt2", "gpt2", dev))
    tok1 = Tok(CLAP_CFG(2)["vocab_size"], CLAP_CFG(2)["pad_token_id"], 24, bos=0, eos=2)
    tok2 = Tok(T5_CFG["vocab_size"], 0, 32, eos=1)
    dtype = torch.float32
    unet = A.AudioLDM2UNet2DConditionModel(A.UNetConfig(block_out_channels=(64, 128, 192, 256), attention_head_dim=4, norm_num_groups=16))
    A.install_ap_adapter(unet, None, scale=0.5)
    synthetic.init_synthetic_(unet, 100, w_std=0.05, bias_std=0.02, norm_jitter=0.1)
    torch.manual_seed(3)
    vae = A.AutoencoderKL(A.VaeConfig(block_out_channels=(32, 64, 64), layers_per_block=1, norm_num_groups=8)).to(dev, dtype)
    voc = A.SpeechT5HifiGan(A.HifiGanConfig(upsample_initial_channel=256, upsample_rates=(5, 4, 2, 2, 2), upsample_kernel_sizes=(16, 16, 8, 4, 4))).to(dev, dtype)
    tower = M.ours(M.SMALL_CFG, M.SMALL_SEED).to(dev)
    fe = _StubFeatures()
    parts = dict(vocoder=voc, vae=vae, prompt_encoder=enc, tokenizer=tok1, tokenizer_2=tok2)
    pipe = A.AudioLDM2Pipeline(unet.to(dev, dtype), audio_tower=tower, feature_extractor=fe, **parts)
    n, P = 3, len(PROMPTS)
    B, Lt = P * n, 8
    # the text prompt decides the ranking; the UNet's conditions are the precomputed embeddings the reference accepts beside it
    e = dict(prompt_embeds=R(P, 16, 1024, seed=20), negative_prompt_embeds=R(P, 16, 1024, seed=21),
             generated_prompt_embeds=R(P, Lt, 768, seed=22), negative_generated_prompt_embeds=R(P, Lt, 768, seed=23),
             attention_mask=torch.ones(P, 16, dtype=torch.long), negative_attention_mask=torch.ones(P, 16, dtype=torch.long))
    kw = dict(prompt=PROMPTS, num_waveforms_per_prompt=n, num_inference_steps=2, audio_length_in_s=0.64, latents=R(B, 8, 16, 16, seed=24),
              use_graph=False, **e)
    # the oracle's decision is not a near-tie: every gap that decides the top 3 is at least 100 x the logits' tolerance
    ref = gold["pipe.logits"]
    assert ref.shape == (P, B)
    srt = torch.sort(ref, dim=1, descending=True).values
    assert float((srt[:, :n] - srt[:, 1:n + 1]).min()) >= 100 * M.TOL * float(ref.abs().max())
    order = torch.argsort(ref, dim=1, descending=True)[:, :n].reshape(-1)
    assert order.tolist() != list(range(B))
    seen = {}
    score = pipe.score_waveforms

    def spy(**k):
        seen["audio"] = k["audio"].clone()
        return score(**k)

    pipe.score_waveforms = spy
    out = pipe(output_type="pt", **kw).audios
    cand = seen["audio"]  # the un-ranked candidates, in generation order
    assert cand.shape == (B, int(0.64 * 16000)) and len({float(c.abs().sum()) for c in cand}) == B
    assert fe.calls == [(B, int(0.64 * 48000), 48000)]  # resampled 16 kHz -> 48 kHz on the way to the extractor
    e_log = rel_err(pipe.last_logits_per_text, ref)
    print(f"pipeline logits_per_text: rel_err {e_log:.3e}")
    assert e_log < M.TOL
    assert out.shape == (P * n, cand.shape[1]) and torch.equal(out, cand[order])
    # latent output is the reference's early exit: un-ranked latents, no scoring
    fe.calls.clear()
    lat = pipe(output_type="latent", **kw).audios
    assert lat.shape == (B, 8, 16, 16) and not fe.calls
    # a pipeline without the tower still refuses, and names the two arguments
    with pytest.raises(NotImplementedError, match=r"audio_tower=.*feature_extractor="):
        A.AudioLDM2Pipeline(unet, **parts)(output_type="pt", **kw)
