"""CPU: host logic of the CLAP audio tower -- parameter naming against the installed transformers module, the index arithmetic the two
kernels and the patch merging rely on (bias gather, merge index, shift-region formula) against the module's own code, the ABI
declarations, the ranking reorder, loud failure without a GPU, and the committed fixture against the installed module."""
import os
import re

import pytest
import torch

import clap_audio_models as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_installed_state_dict_loads_with_no_missing_or_unexpected_key():
    import ap_adapter_amd as A
    for cfg, seed in ((M.SMALL_CFG, M.SMALL_SEED), (M.REAL_CFG, M.REAL_SEED)):
        hf = M.installed(cfg, seed)
        o = A.ClapAudioModelWithProjection(A.ClapAudioConfig(**cfg))
        res = o.load_state_dict(hf.state_dict(), strict=True)
        assert not res.missing_keys and not res.unexpected_keys
        sd = hf.state_dict()
        assert any(k.endswith("relative_position_index") for k in sd)  # a buffer there: accepted
        for k, v in o.state_dict().items():
            assert torch.equal(sd[k], v), k
        # the helper's per-name stream fills both sides identically (the GPU tests seed the HIP module directly)
        for (k, v), (k2, v2) in zip(sorted(M.ours(cfg, seed).state_dict().items()), sorted(sd.items())):
            assert k == k2 and torch.equal(v, v2), k


def test_bias_gather_equals_the_modules():
    from ap_adapter_amd import clap_audio as CA
    hf = M.installed(M.SMALL_CFG, M.SMALL_SEED)
    for stage in hf.audio_model.audio_encoder.layers:
        att = stage.blocks[1].attention.self
        ref = att.relative_position_bias_table[att.relative_position_index.view(-1)].view(64, 64, -1).permute(2, 0, 1).contiguous()
        assert float(ref.detach().abs().max()) > 0.1  # randomised: a dropped bias would show
        assert torch.equal(CA.relative_position_index(), att.relative_position_index)
        assert torch.equal(CA.gather_relative_position_bias(att.relative_position_bias_table, att.relative_position_index), ref)


def test_merge_index_is_the_modules_interleave():
    from ap_adapter_amd import clap_audio as CA
    for B, H, W, C in ((2, 16, 16, 5), (1, 8, 12, 3)):
        x = torch.randn(B, H, W, C, generator=torch.Generator().manual_seed(H))
        ref = torch.cat([x[:, r::2, c::2] for c in range(2) for r in range(2)], -1).view(B, -1, 4 * C)
        got = x.view(-1, C)[CA.merge_index(B, H, W)].view(B, (H // 2) * (W // 2), 4 * C)
        assert torch.equal(got, ref)


@pytest.mark.parametrize("hw", [(16, 16), (32, 32), (64, 64), (16, 24)])
def test_region_formula_reproduces_get_attn_mask(hw):
    """the mask the kernel never materialises: region ids of the shifted coordinates, -100 where 3 * h_region + w_region differ --
    against the installed ClapAudioLayer.get_attn_mask and against its original slice-assignment form"""
    from ap_adapter_amd import clap_audio as CA
    H, W = hw
    reg = (3 * CA.shift_regions(H, 4)[:, None] + CA.shift_regions(W, 4)[None, :]).view(H // 8, 8, W // 8, 8).permute(0, 2, 1, 3).reshape(-1, 64)
    mine = torch.where(reg[:, None, :] != reg[:, :, None], -100.0, 0.0)
    assert torch.equal(mine.double(), M.ref_attn_mask(H, W, 4))
    layer = M.installed(M.SMALL_CFG, M.SMALL_SEED).audio_model.audio_encoder.layers[0].blocks[1]
    assert layer.shift_size == 4 and layer.window_size == 8
    assert torch.equal(mine, layer.get_attn_mask(H, W, torch.float32, "cpu"))
    assert int((mine != 0).sum()) > 0


def test_abi_declares_the_two_entry_points_additively():
    from ap_adapter_amd import _lib
    header = open(os.path.join(ROOT, "include", "apadapter_hip.h")).read()
    assert re.search(r"#define APAD_ABI_VERSION 12\b", header)  # additive: the version line stays
    for name in ("apad_window_attention", "apad_clap_mel2img"):
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in _lib.SYMBOLS
    # one ctypes argument per declared parameter
    for name in ("apad_window_attention", "apad_clap_mel2img"):
        decl = re.search(r"\bint %s\((.*?)\);" % name, header, re.S).group(1)
        assert len(decl.split(",")) == len(_lib.SYMBOLS[name][1]), name


def test_cpu_tensors_and_unsupported_configurations_raise():
    import ap_adapter_amd as A
    m = M.ours(M.SMALL_CFG, M.SMALL_SEED)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(M.features(M.SMALL_SHAPE, 1))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.get_audio_features(M.features(M.SMALL_SHAPE, 1))
    for kw, name in ((dict(enable_fusion=True), "enable_fusion"), (dict(window_size=4), "window_size"), (dict(patch_size=8), "patch_size"),
                     (dict(patch_stride=2), "patch_stride"), (dict(num_attention_heads=[3, 6, 12, 24]), "num_attention_heads")):
        with pytest.raises(NotImplementedError, match=name):
            A.ClapAudioModelWithProjection(A.ClapAudioConfig(**kw))


def test_rank_waveforms_reorders_over_all_candidates():
    """pipeline_audioldm2.py:610-613 on hand-written logits: per prompt the best n of ALL candidates, best first"""
    from ap_adapter_amd.clap_audio import rank_waveforms
    logits = torch.tensor([[0.1, 0.9, 0.3, 0.2, 0.8, 0.0],
                           [0.5, 0.4, 0.45, 0.9, 0.1, 0.95]])
    audio = torch.arange(6, dtype=torch.float32).view(6, 1).repeat(1, 4)
    out = rank_waveforms(logits, audio, 3)
    assert out.shape == (6, 4) and out[:, 0].tolist() == [1, 4, 2, 5, 3, 0]
    assert rank_waveforms(logits, audio, 1)[:, 0].tolist() == [1, 5]
    ref = torch.index_select(audio, 0, torch.argsort(logits, dim=1, descending=True)[:, :2].reshape(-1))
    assert torch.equal(rank_waveforms(logits, audio, 2), ref)


def test_pipeline_names_the_two_arguments_without_an_audio_tower():
    import ap_adapter_amd as A
    pipe = A.AudioLDM2Pipeline(None, vae=object(), vocoder=object())
    assert pipe.audio_tower is None and pipe.feature_extractor is None and abs(pipe.logit_scale_t - M.LOGIT_SCALE_T) < 1e-12
    with pytest.raises(NotImplementedError, match=r"audio_tower=.*feature_extractor="):
        pipe(prompt=["a"], num_waveforms_per_prompt=3)
    with pytest.raises(NotImplementedError, match=r"audio_tower=.*feature_extractor="):
        pipe.score_waveforms(["a"], torch.zeros(3, 8), 3, "cpu", torch.float32)


def test_fixture_is_the_installed_modules_output():
    """tests/golden/clap_audio.safetensors (what the GPU tests compare with) re-derived from the installed transformers module; and the
    module's pooler_output is the plain mean over the final tokens (its reshapes in front of avgpool are a permutation)"""
    gold = M.load_gold()
    for pre, cfg, seed, shape in (("small", M.SMALL_CFG, M.SMALL_SEED, M.SMALL_SHAPE), ("real", M.REAL_CFG, M.REAL_SEED, M.REAL_SHAPE)):
        emb, pooled = M.oracle_outputs(cfg, seed, shape)
        assert torch.allclose(emb, gold[pre + ".embeds"], rtol=0, atol=1e-5 * float(emb.abs().max()))
        assert torch.allclose(pooled, gold[pre + ".pooler"], rtol=0, atol=1e-5 * float(pooled.abs().max()))
    logits = M.oracle_pipe_logits()
    assert torch.allclose(logits, gold["pipe.logits"], rtol=0, atol=1e-5 * float(logits.abs().max()))
    with torch.no_grad():
        hf = M.installed(M.SMALL_CFG, M.SMALL_SEED)
        out = hf.audio_model(input_features=M.features(M.SMALL_SHAPE, M.SMALL_SEED + 7))
        tokens = out.last_hidden_state.flatten(2).transpose(1, 2)  # [B, 64 tokens (permuted), C]
        assert torch.allclose(tokens.mean(1), out.pooler_output, rtol=0, atol=1e-6)
