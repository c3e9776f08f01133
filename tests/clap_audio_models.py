"""The CLAP audio tower's oracle, shared by tests/test_clap_audio_host.py, tests/test_gpu_clap_audio.py and
tests/golden/make_clap_audio_golden.py: the INSTALLED transformers ``ClapAudioModelWithProjection`` in ``.eval()`` on the CPU in fp32
with seeded weights (the reference's own dependency, like tests/text_models.py for the prompt encoders), plus torch restatements of
the two new kernels' operators.

The weights are not stored: both sides fill them from a frozen per-parameter stream (``seeded_weights_``; the parameter names are the
same on both sides).  BatchNorm's running statistics and the relative-position bias tables are randomised too -- their defaults
(0 / 1 / zeros) would hide a missing BatchNorm or bias.  The GPU tests read the oracle's OUTPUTS from the committed fixture
tests/golden/clap_audio.safetensors (transformers is not imported on the GPU box: its import alone pages in for minutes there);
tests/test_clap_audio_host.py re-derives the fixture from the installed module on the CPU."""
import math
import os

import torch
import torch.nn.functional as F

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "clap_audio.safetensors")

# the small model: head size 24 and 64-token windows as in the real one; first stage 16 x 16 tokens (4 windows, a shifted odd block
# that exercises the mask), one patch-merging stage, last stage 8 x 8 (one window, shift forced to 0)
SMALL_CFG = dict(spec_size=64, num_mel_bins=16, patch_embeds_hidden_size=48, depths=[2, 2], num_attention_heads=[2, 4], hidden_size=96,
                 projection_dim=32)
REAL_CFG = dict()  # transformers.ClapAudioConfig() defaults = laion/clap-htsat-unfused
SMALL_SHAPE, REAL_SHAPE = (3, 1, 251, 16), (2, 1, 1001, 64)
SMALL_SEED, REAL_SEED = 41, 42
TOL = 5e-5  # the bar of the fp32 encoders against transformers (tests/test_gpu_text_encoders.py at real widths)


def seeded_weights_(module, seed):
    """fill every parameter of ``module`` (CPU) from a frozen per-parameter stream, in name order: matrices N(0, 0.05^2), the
    relative-position bias tables N(0, 0.5^2), normalisation gains 1 + 0.1 N(0, 1), other vectors N(0, 0.02^2); BatchNorm's running
    mean N(0, 0.3^2) and running variance U(0.5, 1.5)"""
    with torch.no_grad():
        for i, (name, p) in enumerate(sorted(module.named_parameters(), key=lambda kv: kv[0])):
            r = torch.randn(p.shape, generator=torch.Generator().manual_seed(seed * 1000 + i))
            if "relative_position_bias_table" in name:
                p.copy_(0.5 * r)
            elif p.dim() > 1:
                p.copy_(0.05 * r)
            elif name.endswith("weight"):  # LayerNorm / BatchNorm gains
                p.copy_(1.0 + 0.1 * r)
            else:
                p.copy_(0.02 * r)
        for i, (name, b) in enumerate(sorted(module.named_buffers(), key=lambda kv: kv[0])):
            g = torch.Generator().manual_seed(seed * 1000 + 500 + i)
            if name.endswith("running_mean"):
                b.copy_(0.3 * torch.randn(b.shape, generator=g))
            elif name.endswith("running_var"):
                b.copy_(0.5 + torch.rand(b.shape, generator=g))
    return module


def features(shape, seed):
    """stand-in log-mel features: per-sample offset and spread so that the samples differ by more than noise"""
    x = torch.randn(shape, generator=torch.Generator().manual_seed(seed))
    b = torch.arange(shape[0], dtype=torch.float32).view(-1, 1, 1, 1)
    return x * (1.0 + 0.5 * b) + 0.3 * b - 0.5


def ours(cfg, seed):
    """the HIP module (CPU, seeded)"""
    import ap_adapter_amd as A
    return seeded_weights_(A.ClapAudioModelWithProjection(A.ClapAudioConfig(**cfg)), seed)


def installed(cfg, seed):
    """the installed transformers module (CPU, eval, seeded)"""
    import transformers
    return seeded_weights_(transformers.ClapAudioModelWithProjection(transformers.ClapAudioConfig(**cfg)).eval(), seed)


@torch.no_grad()
def oracle_outputs(cfg, seed, shape):
    """(audio_embeds, pooler_output) of the installed module on the seeded features"""
    m = installed(cfg, seed)
    x = features(shape, seed + 7)
    pooled = m.audio_model(input_features=x).pooler_output
    return m(input_features=x).audio_embeds, pooled


# ---- the ranking case of the pipeline test: 2 prompts x 3 candidates, stub features, tiny CLAP text tower of tests/text_models.py ----
PIPE_FEATURE_SEED = 77
LOGIT_SCALE_T = math.log(1.0 / 0.07)


def pipe_features():
    return features((6,) + SMALL_SHAPE[1:], PIPE_FEATURE_SEED)


@torch.no_grad()
def oracle_pipe_logits():
    """logits_per_text of the installed modules (ClapModel.forward's arithmetic, :1596-1602) for text_models.PROMPTS under the stand-in
    tokenizer and the six stub feature maps"""
    from text_models import CLAP_CFG, PROMPTS, Tok, tiny_clap
    clap, _ = tiny_clap(heads=2)
    tok = Tok(CLAP_CFG(2)["vocab_size"], CLAP_CFG(2)["pad_token_id"], 24, bos=0, eos=2)(PROMPTS, padding=True)
    t = clap.text_projection(clap.text_model(input_ids=tok.input_ids, attention_mask=tok.attention_mask).pooler_output)
    a = installed(SMALL_CFG, SMALL_SEED)(input_features=pipe_features()).audio_embeds
    t, a = t / t.norm(p=2, dim=-1, keepdim=True), a / a.norm(p=2, dim=-1, keepdim=True)
    return torch.matmul(t, a.t()) * math.exp(LOGIT_SCALE_T)


def load_gold():
    from safetensors.torch import load_file
    return load_file(GOLD)


# ---- torch restatements of the two kernels' operators (no transformers) ----
def ref_attn_mask(H, W, shift, window=8):
    """ClapAudioLayer.get_attn_mask in its original slice-assignment form: [windows, 64, 64], -100 where the regions differ"""
    img = torch.zeros(1, H, W, 1, dtype=torch.float64)
    count = 0
    for hs in (slice(0, -window), slice(-window, -shift), slice(-shift, None)):
        for ws in (slice(0, -window), slice(-window, -shift), slice(-shift, None)):
            img[:, hs, ws, :] = count
            count += 1
    mw = img.view(1, H // window, window, W // window, window, 1).permute(0, 1, 3, 2, 4, 5).reshape(-1, window * window)
    am = mw.unsqueeze(1) - mw.unsqueeze(2)
    return am.masked_fill(am != 0, -100.0)


def ref_window_attention(qkv, bias, heads, shift, masked=True):
    """ClapAudioLayer's roll -> window_partition -> ClapAudioSelfAttention (scores / sqrt(d) + bias + mask, softmax, P.V) ->
    window_reverse -> roll back, in float64 from the fp32 operands.  qkv [B, H, W, 3C] (already projected), bias [heads, 64, 64]"""
    qkv, bias = qkv.double(), bias.double()
    B, H, W, C3 = qkv.shape
    C, d = C3 // 3, C3 // 3 // heads
    x = torch.roll(qkv, shifts=(-shift, -shift), dims=(1, 2)) if shift > 0 else qkv
    win = x.view(B, H // 8, 8, W // 8, 8, C3).permute(0, 1, 3, 2, 4, 5).reshape(-1, 64, C3)
    q, k, v = (t.reshape(-1, 64, heads, d).transpose(1, 2) for t in win.split(C, dim=-1))
    s = torch.matmul(q, k.transpose(-1, -2)) / math.sqrt(d) + bias.unsqueeze(0)
    if shift > 0 and masked:
        am = ref_attn_mask(H, W, shift)
        s = (s.view(B, am.shape[0], heads, 64, 64) + am.unsqueeze(1).unsqueeze(0)).view(-1, heads, 64, 64)
    o = torch.matmul(torch.softmax(s, dim=-1), v).permute(0, 2, 1, 3).reshape(-1, 8, 8, C)
    o = o.view(B, H // 8, W // 8, 8, 8, C).permute(0, 1, 3, 2, 4, 5).reshape(B, H, W, C)
    return torch.roll(o, shifts=(shift, shift), dims=(1, 2)) if shift > 0 else o


def ref_mel2img(x, bn_w, bn_b, bn_mean, bn_var, eps, spec_size):
    """BatchNorm2d (eval) over the mel bins -> ClapAudioEncoder.reshape_mel2img -> 4 x 4 / stride-4 unfold: [B * (S/4)^2, 16]"""
    B, _, T, Fb = x.shape
    r = spec_size // Fb
    y = F.batch_norm(x.transpose(1, 3), bn_mean, bn_var, bn_w, bn_b, False, 0.0, eps).transpose(1, 3)
    if T < spec_size * r:
        y = F.interpolate(y, (spec_size * r, Fb), mode="bicubic", align_corners=True)
    b, c, t, f = y.shape
    y = y.reshape(b, c * r, t // r, f).permute(0, 1, 3, 2).contiguous().reshape(b, c, f * r, t // r)
    return F.unfold(y, kernel_size=4, stride=4).transpose(1, 2).reshape(-1, 16)
