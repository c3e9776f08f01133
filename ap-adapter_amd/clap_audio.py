"""CLAP audio tower (transformers ``ClapAudioModelWithProjection``: HTSAT, a Swin transformer over the log-mel "image"), the half of
``AudioLDM2Pipeline.score_waveforms`` (pipeline/pipeline_audioldm2.py:592-614 of the reference) that the prompt encoders do not cover.

The classes keep the transformers parameter names, so the installed module's state dict loads with ``load_state_dict``, and run the
arithmetic through the C ABI in the fp32 precision mode, once per pipeline call: ``apad_clap_mel2img`` (BatchNorm + bicubic time stretch
+ reshape_mel2img + patch gather), ``apad_window_attention`` (one launch per Swin block: shift, window partition, relative-position
bias, shift mask, softmax, P.V) and existing entry points for everything else -- ``apad_gemm`` (patch embedding, fused q | k | v,
output dense + residual, the MLP with the erf-GELU epilogue, the patch-merging reduction, the token mean as a product with a constant
1 / n pooling matrix, the projection with the ReLU epilogue), ``apad_layernorm``, ``apad_gather_rows`` (the patch-merging interleave),
``apad_transpose_pad`` (the token-major -> channel-major turn in front of the mean) and ``apad_rmsnorm`` (F.normalize).
No PyTorch compute fallback: CPU tensors raise.  The fusion variant (``enable_fusion``, ``is_longer``) is outside this path.
"""
from dataclasses import dataclass, field
from types import SimpleNamespace

import torch
import torch.nn as nn

from . import ops
from .derived import derived
from .text_encoders import _ClapProjection, _need_gpu_f32

WINDOW = 8      # apad_window_attention's envelope: 8 x 8 windows of head size 24
HEAD_DIM = 24
POOL_CHUNK = 32  # samples per token-mean GEMM


@dataclass
class ClapAudioConfig:
    """defaults = transformers.ClapAudioConfig (laion/clap-htsat-unfused audio tower, the one cvssp/audioldm2 ships)"""
    window_size: int = 8
    num_mel_bins: int = 64
    spec_size: int = 256
    patch_size: int = 4
    patch_stride: int = 4
    hidden_size: int = 768
    projection_dim: int = 512
    depths: list = field(default_factory=lambda: [2, 2, 6, 2])
    num_attention_heads: list = field(default_factory=lambda: [4, 8, 16, 32])
    enable_fusion: bool = False
    patch_embeds_hidden_size: int = 96
    qkv_bias: bool = True
    mlp_ratio: float = 4.0
    layer_norm_eps: float = 1e-5
    model_type: str = "clap_audio_model"


def _check_config(cfg):
    """everything outside the kernels' envelope raises and names the argument"""
    if cfg.enable_fusion:
        raise NotImplementedError("enable_fusion=True: the fusion variant of the CLAP audio tower (AFF block, is_longer) is not on this path")
    if cfg.window_size != WINDOW:
        raise NotImplementedError(f"window_size={cfg.window_size}: apad_window_attention serves 8 x 8 windows")
    ps, st = cfg.patch_size, cfg.patch_stride
    if (tuple(ps) if isinstance(ps, (list, tuple)) else (ps, ps)) != (4, 4):
        raise NotImplementedError(f"patch_size={ps}: apad_clap_mel2img gathers 4 x 4 patches")
    if (tuple(st) if isinstance(st, (list, tuple)) else (st, st)) != (4, 4):
        raise NotImplementedError(f"patch_stride={st}: apad_clap_mel2img gathers 4 x 4 patches at stride 4")
    if len(cfg.depths) != len(cfg.num_attention_heads):
        raise ValueError(f"depths={cfg.depths} and num_attention_heads={cfg.num_attention_heads} differ in length")
    for i, h in enumerate(cfg.num_attention_heads):
        if cfg.patch_embeds_hidden_size * 2 ** i != h * HEAD_DIM:
            raise NotImplementedError(f"num_attention_heads={cfg.num_attention_heads} with patch_embeds_hidden_size={cfg.patch_embeds_hidden_size}: "
                                      f"stage {i} has head size {cfg.patch_embeds_hidden_size * 2 ** i / h:g}; apad_window_attention serves 24")
    if cfg.spec_size % cfg.num_mel_bins or cfg.spec_size % 4:
        raise ValueError(f"spec_size={cfg.spec_size} must be a multiple of num_mel_bins={cfg.num_mel_bins} and of the patch size")
    last = cfg.spec_size // 4 // 2 ** (len(cfg.depths) - 1)
    if last < WINDOW or (cfg.spec_size // 4) % (WINDOW * 2 ** (len(cfg.depths) - 1)):
        raise NotImplementedError(f"spec_size={cfg.spec_size} with depths={cfg.depths}: every stage must be a whole number of 8 x 8 windows")
    if not cfg.qkv_bias:
        raise NotImplementedError("qkv_bias=False is not on this path")


def relative_position_index(window=WINDOW):
    """ClapAudioSelfAttention.create_relative_position_index: [window^2, window^2] indices into the (2 window - 1)^2-row bias table"""
    c = torch.stack(torch.meshgrid([torch.arange(window), torch.arange(window)], indexing="ij")).flatten(1)
    rel = (c[:, :, None] - c[:, None, :]).permute(1, 2, 0).contiguous()
    rel[:, :, 0] += window - 1
    rel[:, :, 1] += window - 1
    rel[:, :, 0] *= 2 * window - 1
    return rel.sum(-1)


def gather_relative_position_bias(table, index):
    """relative_position_bias_table [(2w-1)^2, heads] + index [w^2, w^2] -> fp32 [heads, w^2, w^2] (head, query, key), the matrix
    apad_window_attention adds to the scores (a look-up: it moves values, no arithmetic)"""
    n = index.shape[0]
    return table.detach()[index.reshape(-1).to(table.device)].view(n, n, -1).permute(2, 0, 1).contiguous()


def merge_index(B, H, W, device=None):
    """int64 [B * H/2 * W/2 * 4]: the source token of each C-wide slot of the patch-merging rows, in the module's channel order
    (row 0, col 0), (row 1, col 0), (row 0, col 1), (row 1, col 1) -- ``torch.cat([x[:, r::2, c::2] for c in range(2) for r in range(2)], -1)``"""
    b = torch.arange(B).view(B, 1, 1, 1)
    i = torch.arange(H // 2).view(1, -1, 1, 1)
    j = torch.arange(W // 2).view(1, 1, -1, 1)
    q = torch.arange(4).view(1, 1, 1, 4)
    idx = b * (H * W) + (2 * i + q % 2) * W + (2 * j + q // 2)
    return idx.reshape(-1).to(device)


def shift_regions(n, shift, window=WINDOW):
    """region id of every SHIFTED coordinate along one axis of n tokens, the formula apad_window_attention evaluates: two tokens of
    a window attend each other iff 3 * h_region + w_region agree (ClapAudioLayer.get_attn_mask, -100 otherwise)"""
    i = torch.arange(n)
    return (i >= n - window).long() + (i >= n - shift).long()


def rank_waveforms(logits_per_text, audio, num_waveforms_per_prompt):
    """pipeline_audioldm2.py:610-613: per prompt, the ``num_waveforms_per_prompt`` best of ALL candidates of the batch by CLAP
    text-audio similarity; argsort / index_select move indices, not arithmetic"""
    indices = torch.argsort(logits_per_text, dim=1, descending=True)[:, :num_waveforms_per_prompt]
    return torch.index_select(audio, 0, indices.reshape(-1).cpu())


_index_cache = {}


def _cached_index(kind, key, device, make):
    k = (kind, key, str(device))
    if k not in _index_cache:
        _index_cache[k] = make().to(device)
    return _index_cache[k]


class _SelfAttention(nn.Module):
    def __init__(self, c, heads):
        super().__init__()
        self.relative_position_bias_table = nn.Parameter(torch.zeros((2 * WINDOW - 1) ** 2, heads))
        self.register_buffer("relative_position_index", relative_position_index())
        self.query, self.key, self.value = nn.Linear(c, c), nn.Linear(c, c), nn.Linear(c, c)

    def qkv(self):
        """rows q | k | v of the fused projection and its bias"""
        q, k, v = self.query, self.key, self.value
        w = derived(q.weight, "clap_qkv", lambda: torch.cat([q.weight.detach(), k.weight.detach(), v.weight.detach()], 0).contiguous(),
                    (k.weight, v.weight))
        b = derived(q.bias, "clap_qkv", lambda: torch.cat([q.bias.detach(), k.bias.detach(), v.bias.detach()], 0).contiguous(), (k.bias, v.bias))
        return w, b

    def bias_matrix(self):
        t = self.relative_position_bias_table
        return derived(t, "clap_rpb", lambda: gather_relative_position_bias(t, self.relative_position_index), (self.relative_position_index,))


class _Dense(nn.Module):
    def __init__(self, cin, cout):
        super().__init__()
        self.dense = nn.Linear(cin, cout)


class _Attention(nn.Module):
    def __init__(self, c, heads):
        super().__init__()
        self.self = _SelfAttention(c, heads)
        self.output = _Dense(c, c)


class ClapAudioLayer(nn.Module):
    """pre-LN Swin block: x + W-MSA(LN(x)), then x + MLP(LN(x))"""

    def __init__(self, cfg, c, heads, shift):
        super().__init__()
        self.heads, self.shift = heads, shift
        self.layernorm_before = nn.LayerNorm(c, eps=cfg.layer_norm_eps)
        self.attention = _Attention(c, heads)
        self.layernorm_after = nn.LayerNorm(c, eps=cfg.layer_norm_eps)
        self.intermediate = _Dense(c, int(c * cfg.mlp_ratio))
        self.output = _Dense(int(c * cfg.mlp_ratio), c)

    def forward(self, x, B, H, W):
        """x [B * H * W, C] in raster order"""
        shift = 0 if min(H, W) <= WINDOW else self.shift  # set_shift_and_window_size: one window = no shift
        ln, a = self.layernorm_before, self.attention
        w, b = a.self.qkv()
        qkv = ops.linear(ops.layer_norm(x, ln.weight, ln.bias, ln.eps), w, b)
        ctx = ops.window_attention(qkv, a.self.bias_matrix(), B, H, W, self.heads, shift)
        x = ops.linear(ctx, a.output.dense.weight, a.output.dense.bias, residual=x)
        ln = self.layernorm_after
        h = ops.linear(ops.layer_norm(x, ln.weight, ln.bias, ln.eps), self.intermediate.dense.weight, self.intermediate.dense.bias, act="gelu")
        return ops.linear(h, self.output.dense.weight, self.output.dense.bias, residual=x)


class ClapAudioPatchMerging(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.reduction = nn.Linear(4 * c, 2 * c, bias=False)
        self.norm = nn.LayerNorm(4 * c)

    def forward(self, x, B, H, W):
        C = x.shape[-1]
        idx = _cached_index("merge", (B, H, W), x.device, lambda: merge_index(B, H, W))
        y = ops.gather_rows(x, idx).view(B * (H // 2) * (W // 2), 4 * C)
        return ops.linear(ops.layer_norm(y, self.norm.weight, self.norm.bias, self.norm.eps), self.reduction.weight)


class ClapAudioStage(nn.Module):
    def __init__(self, cfg, c, depth, heads, downsample):
        super().__init__()
        self.blocks = nn.ModuleList([ClapAudioLayer(cfg, c, heads, 0 if i % 2 == 0 else cfg.window_size // 2) for i in range(depth)])
        if downsample:
            self.downsample = ClapAudioPatchMerging(c)
        else:
            self.downsample = None


class _PatchEmbed(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.proj = nn.Conv2d(1, cfg.patch_embeds_hidden_size, kernel_size=4, stride=4)
        self.norm = nn.LayerNorm(cfg.patch_embeds_hidden_size)


class ClapAudioEncoder(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        n = len(cfg.depths)
        self.batch_norm = nn.BatchNorm2d(cfg.num_mel_bins)
        self.patch_embed = _PatchEmbed(cfg)
        self.layers = nn.ModuleList([ClapAudioStage(cfg, cfg.patch_embeds_hidden_size * 2 ** i, cfg.depths[i], cfg.num_attention_heads[i], i < n - 1)
                                     for i in range(n)])
        self.norm = nn.LayerNorm(cfg.patch_embeds_hidden_size * 2 ** (n - 1))


class ClapAudioModel(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.audio_encoder = ClapAudioEncoder(cfg)


class ClapAudioModelWithProjection(nn.Module):
    """``forward(input_features).audio_embeds`` of transformers' ClapAudioModelWithProjection and ``get_audio_features`` of its
    ClapModel (the L2-normalised embeddings); a ClapModel state dict loads with strict=False (its ``audio_model.*`` /
    ``audio_projection.*`` parameters)"""

    def __init__(self, config: ClapAudioConfig = None):
        super().__init__()
        cfg = self.config = config or ClapAudioConfig()
        _check_config(cfg)
        self.audio_model = ClapAudioModel(cfg)
        self.audio_projection = _ClapProjection(cfg.hidden_size, cfg.projection_dim)

    def _pool_matrix(self, B, n_tok, device):
        """[B, B * n_tok]: row b holds 1 / n_tok over sample b's tokens -- the token mean as one GEMM (1 / 64 is exact)"""
        def make():
            m = torch.zeros(B, B * n_tok, dtype=torch.float32)
            for b in range(B):
                m[b, b * n_tok:(b + 1) * n_tok] = 1.0 / n_tok
            return m
        return _cached_index("pool", (B, n_tok), device, make)

    @torch.no_grad()
    def forward(self, input_features=None, is_longer=None):
        """input_features fp32 [B, 1, T <= spec_size^2 / num_mel_bins, num_mel_bins] -> .audio_embeds [B, projection_dim] (not
        normalised, as the module returns them) and .pooler_output [B, hidden_size] (the mean over the final tokens)"""
        _need_gpu_f32(self, "ClapAudioModelWithProjection")
        if is_longer is not None:
            raise NotImplementedError("is_longer: the fusion variant of the CLAP audio tower is not on this path")
        if not input_features.is_cuda:
            raise RuntimeError("ClapAudioModelWithProjection: expected GPU input_features; the HIP path has no CPU fallback")
        cfg, enc = self.config, self.audio_model.audio_encoder
        x = input_features.float().contiguous()
        if x.dim() != 4 or x.shape[1] != 1 or x.shape[3] != cfg.num_mel_bins:
            raise ValueError(f"input_features {tuple(x.shape)}: expected [B, 1, T, {cfg.num_mel_bins}]")
        B = x.shape[0]
        bn = enc.batch_norm
        patches = ops.clap_mel2img(x, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.eps, cfg.spec_size)
        pe = enc.patch_embed
        c0 = pe.proj.weight.shape[0]
        x = ops.linear(patches, pe.proj.weight.view(c0, 16), pe.proj.bias)
        x = ops.layer_norm(x, pe.norm.weight, pe.norm.bias, pe.norm.eps)
        H = W = cfg.spec_size // 4
        for stage in enc.layers:
            for blk in stage.blocks:
                x = blk(x, B, H, W)
            if stage.downsample is not None:
                x = stage.downsample(x, B, H, W)
                H, W = H // 2, W // 2
        x = ops.layer_norm(x, enc.norm.weight, enc.norm.bias, enc.norm.eps)
        # pooler_output: the module's reshapes in front of avgpool permute the final tokens, so it is their plain mean
        n_tok, C = H * W, x.shape[-1]
        pooled = torch.empty(B, C, dtype=torch.float32, device=x.device)
        for b0 in range(0, B, POOL_CHUNK):  # (the pooling matrix is block-diagonal: chunks keep it small; zeros add exactly)
            nb = min(POOL_CHUNK, B - b0)
            xt = ops.transpose_pad(x[b0 * n_tok:(b0 + nb) * n_tok], nb * n_tok)  # [C, nb * n_tok]
            ops.gemm(self._pool_matrix(nb, n_tok, x.device), xt, M=nb, N=C, K=nb * n_tok, lda=nb * n_tok, out=pooled[b0:b0 + nb], ldo=C, exact=True)
        p = self.audio_projection
        emb = ops.linear(ops.linear(pooled, p.linear1.weight, p.linear1.bias, act="relu"), p.linear2.weight, p.linear2.bias)
        return SimpleNamespace(audio_embeds=emb, pooler_output=pooled, last_hidden_state=x.view(B, n_tok, C))

    @torch.no_grad()
    def get_audio_features(self, input_features, is_longer=None):
        """ClapModel.get_audio_features: the L2-normalised audio embeddings [B, projection_dim]"""
        return ops.l2_normalize(self.forward(input_features, is_longer=is_longer).audio_embeds)
