"""The plug-in operators: MI355X-native counterparts of the reference's attention processors.

Same class names, constructor arguments, attributes and call signature as
/root/reference/APadapter/ap_adapter/attention_processor.py (``AttnProcessor2_0`` :199-294,
``IPAttnProcessor2_0`` :297-470) so that the reference wiring loop (inference.py:22-59) works unchanged:

    proc = IPAttnProcessor2_0(hidden_size=C, name=name, cross_attention_dim=768, scale=ap_scale, num_tokens=8)
    proc.to_k_ip.weight = torch.nn.Parameter(state_dict[name + ".to_k_ip.weight"].half())   # re-assignment is honoured
    unet.set_attn_processor({...})

The arithmetic runs in libapadapter_hip.so (apad_gemm + apad_attention); there is no PyTorch fallback.
Weights are read through the attributes at call time.  The timestep-invariant K/V projections can be hoisted
out of the denoise loop with ``kv_cache_enabled`` (the pipeline switches it on and clears it per call); with it
off every call recomputes them exactly like the reference.
"""
from typing import NamedTuple, Optional

import torch
import torch.nn as nn

from . import autograd as AG
from . import ops
from .derived import derived, signature

_vt_pool = {}

# The one-launch cross-attention kernels (apad_fused_cross_attention at C = 256, apad_cross_attention_rows at C = 384).  False selects the chain
# they replace (tests).
USE_FUSED_XATTN = True
USE_XATTN_ROWS = True  # the 384-wide level's kernel alone (follows USE_FUSED_XATTN)


def route(kind, attn, hidden_states, residual=None, ln=None, L1=0, L2=0, masked=False, same_batch=True, query_weighted=False, multi=False):
    """Which kernels run this attention sub-layer.  Decided ONCE per call, before the hoist, from shapes, dtypes, strides and module attributes
    only (CPU tensors do; nothing is launched); both the packing of the hoisted key / value sets and the dispatch read the answer.

    ``kind``: "self", "cross" (AttnProcessor2_0 over a condition) or "decoupled" (IPAttnProcessor2_0); ``residual`` / ``ln``: what the caller
    fuses (the block entry passes ``residual is hidden_states`` and its LayerNorm); ``L1`` / ``L2``: key counts of the one or two segments;
    ``masked``: a key bias will be passed; ``same_batch``: the condition has the batch of the hidden states; ``query_weighted``: the audio segment
    is weighed per query token (a bound ap_mask map): apad_fused_cross_attention has no such form, so what would be "fused" is "chain" -- every
    other answer is unchanged; ``multi``: the audio tokens are those of two or more prompts (bound audio prompts): the fused, rows and hs kernels
    have no such form, so every "decoupled" answer is "chain" (apad_attention_multi) -- every other answer is unchanged.

      "fused"  apad_fused_cross_attention: LayerNorm + to_q + attention + to_out + residual in one launch (C = 256)
      "rows"   apad_cross_attention_rows: the same sub-layer in one launch on row tiles (C = 384)
      "hs"     apad_hs_attention + apad_hs_out: the 64-token level's head-sliced pair (csrc/hsattn.hip), self or cross
      "sattn"  apad_self_attention_fused + to_out: LayerNorm + q | k | v + attention in one launch at the two large levels
      "chain"  projection(s) + apad_attention + to_out: every other geometry, every masked self-attention (the fused self-attention
               kernels carry no key bias; the reference applies attention_mask to attn1 too, attention_processor.py:245-249), all of fp32
    """
    x, heads, wq = hidden_states, attn.heads, attn.to_q.weight
    C_ = x.shape[-1]
    square_q = tuple(wq.shape) == (C_, C_)
    # [B, <= 64, 640], 8 heads, a bias-free square to_q; entered with or without the block's LayerNorm / residual
    hs = (ops.hs_ok(x, heads, wq.shape[0]) and attn.to_q.bias is None and attn.to_out[0].weight.shape[0] == ops.HS_C
          and (residual is None or (residual.shape == x.shape and residual.is_contiguous())))
    if kind == "self":
        if masked:
            return "chain"
        if hs:
            return "hs"
        if ln is not None and ops.sattn_ok(x, heads) and attn.to_q.bias is None and square_q:
            return "sattn"
        return "chain"
    if multi and kind == "decoupled":
        return "chain"
    # the one-launch kernels take the block entry only: they apply its LayerNorm and add x itself
    entry = USE_FUSED_XATTN and residual is x and ln is not None and square_q and x.is_contiguous() and x.dtype in ops.FUSED_DTYPES
    if entry and C_ == ops.XATTN_C and heads == ops.XATTN_HEADS and ops.xattn_lengths_ok(L1, L2, masked):
        return "chain" if query_weighted else "fused"
    if entry and USE_XATTN_ROWS and same_batch and ops.xrows_ok(C_, heads, L1, L2):
        return "rows"
    if hs and same_batch and ops.hs_cross_lengths_ok(L1, L2):
        return "hs"
    return "chain"


def _xrows_weights(attn):
    """fragment-packed to_q / to_out[0] of apad_cross_attention_rows, cached like _xattn_weights"""
    wq, wo = attn.to_q.weight, attn.to_out[0].weight
    return derived(wq, "xrows", lambda: (ops.xrows_pack_weight(wq), ops.xrows_pack_weight(wo)), (wo,))


def _xattn_weights(attn, ln):
    """(fragment-packed to_q with the block's LayerNorm folded in, its fold vectors, fragment-packed to_out[0]) of the fused kernel, cached on
    to_q and re-packed when a parameter (the LayerNorm's included) is re-assigned, moved, cast or updated in place"""
    wq, wo = attn.to_q.weight, attn.to_out[0].weight
    return derived(wq, "xattn", lambda: ops.xattn_pack_weight(wq.detach(), ln) + (ops.xattn_pack_weight(wo.detach()),),
                   (wo, ln[0], ln[1]), (float(ln[2]),))


def _rows_kv(pk, B, Lk, attn):
    return ops.RowsKV(pk, B, Lk, attn.heads, attn.to_out[0].weight.shape[0] // attn.heads)


def _hs_weights(attn, ln, self_attention):
    """(packed projection weights, their fp32 bias, packed to_out[0]) of apad_hs_attention / apad_hs_out, cached on to_q and re-packed when a
    parameter (the LayerNorm's included: it is folded into the projection) is re-assigned, moved, cast or updated in place"""
    wq, wk, wv, wo = attn.to_q.weight, attn.to_k.weight, attn.to_v.weight, attn.to_out[0].weight
    heads = attn.heads

    def make():
        if self_attention:  # (the to_q rows carry log2(e) / sqrt(d): q is the softmax's base-2 exponent operand as projected)
            d = wq.shape[0] // heads
            pk, bb = ops.hs_pack_qkv(wq, wk, wv, ln=ln, q_scale=ops.LOG2E / d ** 0.5)
        else:
            pk, bb = ops.hs_pack_rows(wq, ln=ln)
        return pk, bb, ops.hs_pack_rows(wo)[0]
    deps = (wo,) + ((wk, wv) if self_attention else ()) + (tuple(ln[:2]) if ln is not None else ())
    return derived(wq, "hs", make, deps, (self_attention, heads, None if ln is None else float(ln[2])))


def _hs_sublayer(attn, hidden_states, residual, ln, **kv):
    """LayerNorm? -> projections -> attention (apad_hs_attention), then to_out + bias (+ residual) (apad_hs_out)"""
    self_attention = "k1" not in kv
    pk, bb, wo = _hs_weights(attn, ln, self_attention)
    o = ops.hs_attention(hidden_states, pk, bb, self_attention=self_attention, normalize=ln is not None, ln_eps=(ln[2] if ln is not None else 0.0),
                         q_prescaled=self_attention, **kv)
    return ops.hs_out(o, wo, attn.to_out[0].bias, residual, rowstat=True)


def vt_buffer(slot, B, heads, d, Lk, dtype, device):
    """Zero-padded V^T scratch [B, heads, d, round_up(Lk,32)].  The pad columns are never written (apad_gemm
    APAD_OUT_VT stores l < Lk only), so buffers are shared by shape across attention sites.
    The pool is keyed by (slot, shape, dtype, device, stream) and is never evicted on purpose: a captured hipGraph holds the raw
    addresses of the buffers its kernels were recorded with, so freeing an entry behind a live graph would hand its memory to someone
    else.  Its size is bounded by the distinct attention geometries of the loaded models (a dozen entries, < 100 MB at batch 64);
    ``clear_vt_pool()`` drops it when no captured graph is alive (e.g. between pipelines in one process)."""
    Lpad = ops.round_up(Lk, 32)
    # per stream: the denoise step may run the two CFG halves concurrently on two streams
    key = (slot, B, heads, d, Lpad, dtype, device, torch.cuda.current_stream().cuda_stream)
    buf = _vt_pool.get(key)
    if buf is None:
        buf = torch.zeros(B, heads, d, Lpad, dtype=dtype, device=device)
        _vt_pool[key] = buf
    return buf


def clear_vt_pool():
    """Drop the V^T scratch pool.  Only when no captured hipGraph that used it is still going to be replayed."""
    _vt_pool.clear()


class _Hoist:
    """One hoisted (timestep-invariant) result: K / V^T / packed fragments of one (Attention site, condition tensor), or a
    mask's fp32 bias.  ``sig`` = what the result was computed from (condition version, weight identities / versions); when it
    no longer matches, ``make`` recomputes IN PLACE -- same buffers -- so that a captured hipGraph which reads them stays
    valid across pipeline calls (``refresh`` is what the pipeline runs before replaying a cached graph on new conditions)."""
    __slots__ = ("sig_fn", "make", "sig", "out", "owner")

    def __init__(self, sig_fn, make):
        self.sig_fn, self.make = sig_fn, make
        self.sig, self.out = sig_fn(), make()
        self.owner = HOIST_OWNER[0]  # who asked for it (a cached hipGraph, an eager pipeline call): dropped with its owner

    def get(self):
        sig = self.sig_fn()
        if sig != self.sig:
            new = self.make()
            same = len(new) == len(self.out) and all(
                (a is None and b is None) or (torch.is_tensor(a) and torch.is_tensor(b) and a.shape == b.shape and a.dtype == b.dtype)
                or (not torch.is_tensor(a) and a == b) for a, b in zip(self.out, new))
            if same:
                for a, b in zip(self.out, new):
                    if torch.is_tensor(a):
                        a.copy_(b)
            else:
                self.out = new
            self.sig = sig
        return self.out


HOIST_OWNER = [None]  # set by the pipeline around a call (see AudioLDM2Pipeline.denoise)


def _precision_of(w):
    """the fp32 matmul precision hoisted K/V of an fp32 module were projected in (part of their signature: K/V projected in one
    precision never serve the other); None for the 16-bit modes, which do not read it"""
    return ops.get_float32_matmul_precision() if w.dtype == torch.float32 else None


def _loose_key(attn, t):
    """which (site, condition BUFFER) a hoisted result belongs to; the content is tracked by _Hoist.sig"""
    return (id(attn), t.data_ptr(), tuple(t.shape), tuple(t.stride()), t.dtype)


def _key_bias(attention_mask, B, Lk):
    """The UNet hands processors an additive bias [B,1,L] (modeling_audioldm2.py:741-747); apad_attention takes it
    as fp32 [B,L]."""
    if attention_mask is None:
        return None
    m = attention_mask
    if m.shape[-1] != Lk:
        raise ValueError(f"attention_mask has {m.shape[-1]} key positions, expected {Lk}")
    if m.numel() != B * Lk:
        raise ValueError("attention_mask must broadcast as [batch, 1, keys] (per-head masks are not on this path)")
    return m.reshape(B, Lk).float().contiguous()


def _as_tokens(hidden_states, residual):
    """the 4-D entry of the reference's processors (attention_processor.py:232-236, :363-367): [B, C, H, W] -> [B, H*W, C] (a transposed copy:
    the kernels want channel-contiguous rows); returns (tokens, residual in the same layout, the 4-D shape or None)"""
    if hidden_states.ndim != 4:
        return hidden_states, residual, None
    Bc, Cc, H, W = hidden_states.shape
    tok = hidden_states.reshape(Bc, Cc, H * W).transpose(1, 2).contiguous()
    if residual is hidden_states:
        residual = tok
    elif residual is not None:
        residual = residual.reshape(Bc, Cc, H * W).transpose(1, 2).contiguous()
    return tok, residual, (Bc, Cc, H, W)


def _as_image(out, shape4):
    """... and back (:290-291, :461-462)"""
    return out if shape4 is None else out.transpose(-1, -2).reshape(*shape4)


class _KV(NamedTuple):
    """the hoisted key / value sets of one cross-attention call, per segment: k [B, L, C] row-major, vt [B, heads, d, Lpad] per-head transposed,
    pk = the fragment packing the call's route reads (ops.xattn_pack_kv for "fused", ops.rows_pack_kv for "rows" / "hs", None for "chain");
    a call without a second segment leaves its three fields None.  Segments 3 to 5 are audio prompts 1 to 3 of a call under bound audio
    prompts (the chain route: their pk stays None)"""
    k1: torch.Tensor
    vt1: torch.Tensor
    pk1: Optional[torch.Tensor] = None
    k2: Optional[torch.Tensor] = None
    vt2: Optional[torch.Tensor] = None
    pk2: Optional[torch.Tensor] = None
    k3: Optional[torch.Tensor] = None
    vt3: Optional[torch.Tensor] = None
    pk3: Optional[torch.Tensor] = None
    k4: Optional[torch.Tensor] = None
    vt4: Optional[torch.Tensor] = None
    pk4: Optional[torch.Tensor] = None
    k5: Optional[torch.Tensor] = None
    vt5: Optional[torch.Tensor] = None
    pk5: Optional[torch.Tensor] = None


def _pack_kv(r, k, vt):
    if r == "fused":
        return ops.xattn_pack_kv(k, vt, k.shape[1])
    if r in ("rows", "hs"):
        return ops.rows_pack_kv(k, vt).data
    return None


class _Processor(nn.Module):
    """What the two processors share: the entry of the reference's processors (guards, the 4-D form), the hoist of timestep-invariant results
    and the dispatch over ``route``.  Adds no parameter, buffer or sub-module.  A subclass describes its condition: ``_lengths`` (key counts of
    the one or two segments), ``_segments`` (source rows and projection weights of each), ``_kv_signature`` (what the hoisted sets were
    computed from), ``_bias`` (its mask rule), ``_scale2`` (the weight of the second segment) and ``_query_weight`` (its per-token map)."""

    fuses_residual = True
    kind = None

    def __init__(self):
        super().__init__()
        self.kv_cache_enabled = False
        self._kv_cache = None

    def clear_kv_cache(self):
        self._kv_cache = None

    def refresh_kv_cache(self):
        """recompute, in place, every hoisted result whose inputs changed (new condition content, re-assigned / stepped
        weights)"""
        for e in (self._kv_cache or {}).values():
            e.get()

    def drop_kv_owner(self, owner):
        if self._kv_cache:
            self._kv_cache = {k: e for k, e in self._kv_cache.items() if e.owner != owner}

    def _hoisted(self, key, sig_fn, make):
        if not self.kv_cache_enabled:
            return make()
        if self._kv_cache is None:
            self._kv_cache = {}
        e = self._kv_cache.get(key)
        if e is None:
            e = self._kv_cache[key] = _Hoist(sig_fn, make)
            return e.out
        return e.get()

    def _project_kv(self, attn, src, wk, wv, slot):
        """one key / value segment: k row-major, vt per-head transposed; slot None: a persistent (hoisted) value owns its buffer"""
        B, Lk, _ = src.shape
        d = attn.to_k.weight.shape[0] // attn.heads
        k = ops.linear(src, wk)
        if slot is None:
            vt = torch.zeros(B, attn.heads, d, ops.round_up(Lk, 32), dtype=src.dtype, device=src.device)
        else:
            vt = vt_buffer(slot, B, attn.heads, d, Lk, src.dtype, src.device)
        ops.linear_vt(src, wv, B, Lk, attn.heads, vt)
        return k, vt

    def _qkv_weight(self, attn, prescale=False):
        """to_q | to_k | to_v stacked for the one-launch projection.  prescale: the to_q rows carry log2(e) / sqrt(d) (scaled in
        fp32, rounded to the storage type once), so the projection writes q as the base-2 exponent operand of the softmax --
        rounded ONCE, like the reference's q -- and the attention kernel spends no instruction per score on the scale."""
        wq, wk, wv = attn.to_q.weight, attn.to_k.weight, attn.to_v.weight
        heads = attn.heads

        def make():
            q = wq.detach()
            if prescale:
                d = q.shape[0] // heads
                q = (q.float() * (ops.LOG2E / d ** 0.5)).to(q.dtype)
            return torch.cat([q, wk.detach(), wv.detach()], dim=0).contiguous()
        return derived(wq, "qkv", make, (wk, wv), (bool(prescale), heads))

    def _project_qkv(self, attn, x, ln):
        """LayerNorm? + q | k | v of a self-attention on the "chain" route -> (q, k, vt, q is pre-scaled)"""
        B, N, C_ = x.shape
        heads = attn.heads

        def outputs():
            q = torch.empty(B, N, C_, dtype=x.dtype, device=x.device)
            return q, torch.empty_like(q), vt_buffer("self", B, heads, C_ // heads, N, x.dtype, x.device)

        if ops.rp_ok(x) and attn.to_q.weight.shape[0] == C_:
            # LayerNorm + q|k|v in ONE launch: x is read once, V lands per-head transposed; the to_q rows carry log2(e) / sqrt(d), so
            # apad_attention takes q as the base-2 exponent operand
            q, k, vt = outputs()
            prescaled = attn.to_q.bias is None
            ops.rowpanel(x, self._qkv_weight(attn, prescaled), [(q, None, C_, "row"), (k, None, C_, "row"), (vt, None, C_, "vt")],
                         ln=ln, vt_geom=(heads, C_ // heads, N, vt.shape[-1]))
            return q, k, vt, prescaled
        if attn.to_q.weight.shape[0] == C_ and C_ % 128 == 0:  # (fp32 mode: every width whose C % 128 == 0)
            # widths outside the row-panel envelope (the 640-wide level): q|k|v in ONE tiled launch, the LayerNorm folded into
            # it when the GEMM that produced x left its row statistics, else a LayerNorm launch first
            qkv_w = self._qkv_weight(attn)
            fold = ln is not None and ops.ln_foldable(x, qkv_w)
            hs = x if (ln is None or fold) else ops.layer_norm(x, *ln)
            q, k, vt = outputs()
            ops.linear_qkv(hs, qkv_w, B, N, heads, q, k, vt, ln=ln if fold else None)
            return q, k, vt, False
        hs = x if ln is None else ops.layer_norm(x, *ln)
        return (ops.linear(hs, attn.to_q.weight),) + self._project_kv(attn, hs, attn.to_k.weight, attn.to_v.weight, "self") + (False,)

    def _sublayer(self, attn, hidden_states, encoder_hidden_states, attention_mask, _residual, _ln):
        """``_residual`` (added after to_out) and ``_ln`` = (gamma, beta, eps) (LayerNorm applied to hidden_states
        first) are private fusion hooks used by this package's BasicTransformerBlock; without them the call is the
        reference's."""
        if attn.spatial_norm is not None or attn.group_norm is not None or attn.norm_cross:
            raise NotImplementedError("spatial_norm / group_norm / norm_cross are not on the AudioLDM2 path")
        if hidden_states.ndim == 4:
            tok, res, shape4 = _as_tokens(hidden_states, _residual)
            return _as_image(self._sublayer(attn, tok, encoder_hidden_states, attention_mask, res, _ln), shape4)
        if hidden_states.ndim != 3:
            raise ValueError("hidden_states must be [batch, tokens, channels] or [batch, channels, height, width]")
        if encoder_hidden_states is None and self.kind == "decoupled":
            raise ValueError("IPAttnProcessor2_0 needs encoder_hidden_states = [text tokens | audio tokens]")
        if attn.residual_connection or attn.rescale_output_factor != 1.0:
            raise NotImplementedError("residual_connection / rescale_output_factor are not on the AudioLDM2 path")
        x, ehs, residual, ln = hidden_states, encoder_hidden_states, _residual, _ln
        if ehs is not None and ehs.dim() < 3:
            ehs = ehs.unsqueeze(0)
        if AG.on(x, ehs, *self.parameters()):
            return self._call_train(attn, x, ehs, attention_mask, residual, ln)
        B, N, _ = x.shape
        heads, wo, bo = attn.heads, attn.to_out[0].weight, attn.to_out[0].bias
        masked = attention_mask is not None
        if ehs is None:
            r = route("self", attn, x, residual, ln, masked=masked)
            if r == "hs":
                return _hs_sublayer(attn, x, residual, ln)
            if r == "sattn":  # workgroup = (sample, head), K / V^T in LDS; then to_out
                wq, wk, wv = attn.to_q.weight, attn.to_k.weight, attn.to_v.weight
                w_p, csbb = derived(wq, "sattn", lambda: ops.sattn_pack(wq, wk, wv, ln, heads), (wk, wv, ln[0], ln[1]), (float(ln[2]), heads))
                o = ops.self_attention_fused(x, w_p, csbb, heads, ln[2])
                return ops.fused_linear(o, wo, bo, residual=residual, rowstat=True)
            q, k, vt, prescaled = self._project_qkv(attn, x, ln)
            o = ops.attention(q, k, vt, N, heads, key_bias=self._bias(attention_mask, B, N), q_prescaled=prescaled)
            return ops.fused_linear(o, wo, bo, residual=residual, rowstat=True)
        L1, L2 = self._lengths(ehs)
        prompts = self._prompts(ehs, N)  # None, or one (length, scale2, query weight) per bound audio prompt; L2 is then prompt 0's length
        if prompts is not None:
            L2 = prompts[0][0]
        qw = (self._query_weight(N) if prompts is None else prompts[0][2]) if L2 > 0 else None
        multi = prompts is not None and len(prompts) > 1
        r = route(self.kind, attn, x, residual, ln, L1, L2, masked, ehs.shape[0] == B, query_weighted=qw is not None, multi=multi)
        persistent = self.kv_cache_enabled

        # (where each bound prompt's tokens end is fixed HERE, for the life of the hoisted set: a later refresh -- of every cached step's sets, under
        #  whatever is bound by then -- recomputes this one with the split it was made with)
        lengths = None if prompts is None else tuple(length for length, _, _ in prompts)

        def make():  # the projections, packed with them into what the route's kernel reads
            kv = [self._project_kv(attn, src, wk, wv, None if persistent else slot) for src, wk, wv, slot in self._segments(attn, ehs, lengths)]
            return _KV(*(t for k, vt in kv for t in (k, vt, _pack_kv(r, k, vt))))

        # hoisted K/V belong to ONE (Attention site, condition buffer) -- a processor instance may be shared by every site
        # (set_attn_processor(proc)) -- and are valid for one condition content and one set of projection weights (re-assigned or
        # stepped weights, an in-place update of the condition -> recomputed, in place); packed for one route
        kv = self._hoisted(_loose_key(attn, ehs) + (r, lengths), lambda: self._kv_signature(attn, ehs, lengths), make)
        bias = self._bias(attention_mask, B, L1)
        scale2 = self._scale2() if prompts is None else prompts[0][1]
        if L2 == 0 and isinstance(scale2, tuple):
            raise ValueError("ap_scale: the table weighs the audio branch, and encoder_hidden_states holds no audio tokens")
        if r == "fused":
            wq_p, q_fold, wo_p = _xattn_weights(attn, ln)
            return ops.fused_cross_attention(x, wq_p, wo_p, bo, kv.pk1, L1, heads, ln=ln, key_bias=bias, kv2_packed=kv.pk2, L2=L2, scale2=scale2,
                                             q_fold=q_fold)
        if r in ("rows", "hs"):
            k1 = _rows_kv(kv.pk1, B, L1, attn)
            k2 = _rows_kv(kv.pk2, B, L2, attn) if L2 > 0 else None
            if r == "hs":
                return _hs_sublayer(attn, x, residual, ln, k1=k1, vt1=None, key_bias=bias, k2=k2, vt2=None, scale2=scale2, query_weight=qw)
            wq_p, wo_p = _xrows_weights(attn)
            return ops.cross_attention_rows(x, wq_p, wo_p, bo, k1, None, heads, ln=ln, key_bias=bias, k2=k2, vt2=None, scale2=scale2,
                                            query_weight=qw)
        q = ops.fused_linear(x, attn.to_q.weight, ln=ln)
        extra = None
        if multi:  # prompts 1 to 3: segments 3 to 5 of the hoisted set, each under its own weight and map
            extra = [ops.AudioSegment(kv[6 + 3 * j], kv[7 + 3 * j], length, s2, w) for j, (length, s2, w) in enumerate(prompts[1:])]
        o = ops.attention(q, kv.k1, kv.vt1, L1, heads, key_bias=bias, k2=kv.k2, vt2=kv.vt2, L2=L2, scale2=scale2, query_weight=qw, extra=extra)
        return ops.fused_linear(o, wo, bo, residual=residual, rowstat=True)


class AttnProcessor2_0(_Processor):
    """Plain scaled-dot-product attention (reference :199-294).  Accepts dummy hidden_size / cross_attention_dim
    like the reference so it can live in AttnProcsLayers."""

    kind = "cross"

    def __init__(self, hidden_size=None, cross_attention_dim=None):
        super().__init__()

    def __call__(self, attn, hidden_states, encoder_hidden_states=None, attention_mask=None, temb=None,
                 _residual=None, _ln=None):
        return self._sublayer(attn, hidden_states, encoder_hidden_states, attention_mask, _residual, _ln)

    def _lengths(self, ehs):
        return ehs.shape[1], 0

    def _segments(self, attn, ehs, lengths=None):
        return [(ehs, attn.to_k.weight, attn.to_v.weight, "cross")]

    def _kv_signature(self, attn, ehs, lengths=None):
        return (ehs._version, signature(attn.to_k.weight, attn.to_v.weight), _precision_of(attn.to_k.weight))

    def _bias(self, attention_mask, B, Lk):
        """the whole mask as a key bias.  The mask -> fp32 bias conversion is timestep-invariant too: hoisted with the K/V (two tiny torch
        kernels per masked site per step otherwise)"""
        if attention_mask is None:
            return None
        m = attention_mask
        return self._hoisted(("bias",) + _loose_key(None, m) + (Lk,), lambda: m._version, lambda: (_key_bias(m, B, Lk),))[0]

    def _scale2(self):
        return 0.0

    def _query_weight(self, N):
        return None

    def _prompts(self, ehs, N):
        return None

    def _call_train(self, attn, hidden_states, ehs, attention_mask, _residual, _ln):
        """Training mode (gradients flow to hidden_states; autograd.py): the un-fused chain LayerNorm ->
        to_q / to_k / to_v -> attention -> to_out (+ residual), every node a HIP forward with a HIP backward."""
        B, N, _ = hidden_states.shape
        if _ln is not None and _residual is hidden_states:
            hs, _residual = AG.layer_norm_res(hidden_states, *_ln)  # (the residual gradient joins the LayerNorm backward launch)
        else:
            hs = hidden_states if _ln is None else AG.layer_norm(hidden_states, *_ln)
        if ehs is None:  # self-attention: one input-gradient GEMM for the three projections
            src = hs
            q, k, v, vt = AG.qkv(hs, attn.to_q.weight, attn.to_k.weight, attn.to_v.weight, attn.heads)
        else:
            src = ehs
            q = AG.linear(hs, attn.to_q.weight)
            k = AG.linear(src, attn.to_k.weight)
            v = AG.linear(src, attn.to_v.weight)
            vt = None
        o = AG.attention(q, k, v, attn.heads, _key_bias(attention_mask, B, src.shape[1]), vt=vt)
        return AG.linear(o, attn.to_out[0].weight, attn.to_out[0].bias, residual=_residual)


class IPAttnProcessor2_0(_Processor):
    """Decoupled cross-attention (reference :297-470): text branch over the first ``num_tokens`` tokens with the frozen
    ``attn.to_k/to_v``, audio branch over the remaining tokens with the trainable ``to_k_ip/to_v_ip``, blended
    ``text + scale * audio`` inside one fused kernel."""

    kind = "decoupled"

    def __init__(self, hidden_size, name, cross_attention_dim=None, num_tokens=4, scale=1.0, do_copy=False,
                 copy_dir=None):
        super().__init__()
        self.hidden_size = hidden_size
        self.cross_attention_dim = cross_attention_dim
        self.num_tokens = num_tokens
        self.scale = scale
        self.scale_table = None  # set_ap_scale_table: an ops.Scale2Binding read in place of ``scale``
        self.token_weights = None  # set_ap_token_weights: {token count N: ops.QueryWeight}, the map that multiplies the scale per query token
        self.audio_prompts = None  # set_audio_prompts: ((length, scale, token weights), ...) -- the audio tokens are those of several prompts
        self.name = name
        self.to_k_ip = nn.Linear(cross_attention_dim or hidden_size, hidden_size, bias=False)
        self.to_v_ip = nn.Linear(cross_attention_dim or hidden_size, hidden_size, bias=False)
        if do_copy:
            # reference :328-344 warm-starts from copied_cross_attention/{name}_{k,v}.bin
            from .wiring import load_copied_cross_attention
            load_copied_cross_attention(self, copy_dir)

    def __call__(self, attn, hidden_states, encoder_hidden_states=None, attention_mask=None, temb=None, scale=1.0,
                 _residual=None, _ln=None):
        if scale != 1.0:
            # the reference dereferences an undefined ``logger`` here (:356-357) -> NameError; reject loudly instead
            raise ValueError("`scale` of IPAttnProcessor2_0 is set through the `scale` attribute, not the call kwarg")
        return self._sublayer(attn, hidden_states, encoder_hidden_states, attention_mask, _residual, _ln)

    def _lengths(self, ehs):
        Lt = min(self.num_tokens, ehs.shape[1])
        return Lt, ehs.shape[1] - Lt

    def _segments(self, attn, ehs, lengths=None):
        # ``lengths``: the token counts of the bound audio prompts (None: one audio segment)
        # ragged views -> dense rows for the GEMM A operand (plumbing copies of <= 520 x 768 tokens)
        nt = self.num_tokens
        segs = [(ehs[:, :nt, :].contiguous(), attn.to_k.weight, attn.to_v.weight, "ip_txt")]
        if lengths is not None:  # one segment per prompt, all through the same to_k_ip / to_v_ip
            at = nt
            for j, length in enumerate(lengths):
                segs.append((ehs[:, at:at + length, :].contiguous(), self.to_k_ip.weight, self.to_v_ip.weight, "ip_aud" if j == 0 else f"ip_aud{j}"))
                at += length
            return segs
        if ehs.shape[1] > nt:
            segs.append((ehs[:, nt:, :].contiguous(), self.to_k_ip.weight, self.to_v_ip.weight, "ip_aud"))
        return segs

    def _kv_signature(self, attn, ehs, lengths=None):
        # all four projection weights: a re-assigned to_k_ip / to_v_ip (inference.py:56-57) or an optimizer step is never served stale K/V
        sig = (ehs._version, self.num_tokens, signature(attn.to_k.weight, attn.to_v.weight, self.to_k_ip.weight, self.to_v_ip.weight),
               _precision_of(attn.to_k.weight))
        if lengths is not None:  # where one prompt's tokens end and the next one's begin
            sig += (tuple(lengths),)
        return sig

    def _bias(self, attention_mask, B, Lt):
        """reference :424-428 keeps only mask column 0 (split by the singleton query dim) and broadcasts it over the text keys"""
        if attention_mask is None:
            return None
        return attention_mask.reshape(B, -1)[:, :1].float().expand(B, Lt).contiguous()

    def set_ap_scale_table(self, table, step_ptr, cols=None):
        """read the weight of the audio branch from a device table -- fp32 [steps, cols], row ``*step_ptr`` (an int32 on the device, None = row 0),
        column ``sample % cols`` -- instead of ``self.scale``, which is then neither read nor changed.  Inference only."""
        self.scale_table = ops.Scale2Binding(table, step_ptr, int(table.shape[1] if cols is None else cols))

    def clear_ap_scale_table(self):
        self.scale_table = None

    def _scale2(self):
        return self.scale if self.scale_table is None else self.scale_table

    def set_ap_token_weights(self, maps, cols):
        """weigh the audio branch per query token: ``maps`` = {N: fp32 [cols, N] device tensor}, one map per token count this processor is called
        with (the levels of ``UNet.attention_grids``, tokens in ``_as_tokens``' row-major order); query n of sample b uses (``scale`` or the
        bound table's entry) * maps[N][b % cols][n] (the apad_*_qw entry points).  While maps are bound the 256-wide sites run the chain
        instead of the fused kernel (``route(query_weighted=True)``).  Inference only."""
        self.token_weights = {int(n): ops.QueryWeight(w, int(cols)) for n, w in maps.items()}

    def clear_ap_token_weights(self):
        self.token_weights = None

    def _query_weight(self, N):
        if self.token_weights is None:
            return None
        if N not in self.token_weights:
            raise ValueError(f"ap_mask: no weight map is bound for a call of {N} tokens (bound: {sorted(self.token_weights)})")
        return self.token_weights[N]

    def set_audio_prompts(self, lengths, scales=None, token_weights=None):
        """read the audio tokens of the condition as those of SEVERAL prompts, [text | prompt 0 tokens | prompt 1 tokens | ...]: prompt j owns
        ``lengths[j]`` tokens (1 to 4 prompts; the lengths must sum to the audio tokens of every call), runs its own softmax over the
        ``to_k_ip`` / ``to_v_ip`` projections of its tokens and is added as scales[j] * token_weights[j][N][b % cols][n] * A(q, K_j, V_j).
        ``scales[j]``: None (this processor's ``scale``), a float or an ops.Scale2Binding; ``token_weights[j]``: None or {N: ops.QueryWeight}.
        While two or more prompts are bound every site runs the chain (``route(multi=True)``, apad_attention_multi); a bound ap_scale table
        and ap_mask maps are not read.  Inference only."""
        lengths = [int(n) for n in lengths]
        n = len(lengths)
        if not 1 <= n <= 4:
            raise ValueError(f"audio_prompts: 1 to 4 prompts, got {n}")
        if any(length <= 0 for length in lengths):
            raise ValueError(f"audio_prompts: every prompt needs at least one token, got lengths {lengths}")
        scales = [None] * n if scales is None else list(scales)
        token_weights = [None] * n if token_weights is None else list(token_weights)
        if len(scales) != n or len(token_weights) != n:
            raise ValueError(f"audio_prompts: {n} lengths, {len(scales)} scales and {len(token_weights)} token weights")
        bound = []
        for length, s, tw in zip(lengths, scales, token_weights):
            if s is not None and not isinstance(s, tuple):
                s = float(s)
            elif isinstance(s, tuple):
                s = ops.Scale2Binding(*s)
            if tw is not None:
                tw = {int(k): ops.QueryWeight(*w) for k, w in tw.items()}
            bound.append((length, s, tw))
        self.audio_prompts = tuple(bound)

    def clear_audio_prompts(self):
        self.audio_prompts = None

    def _prompts(self, ehs, N):
        if self.audio_prompts is None:
            return None
        have = ehs.shape[1] - min(self.num_tokens, ehs.shape[1])
        lengths = [length for length, _, _ in self.audio_prompts]
        if sum(lengths) != have:
            raise ValueError(f"audio_prompts: the bound prompts hold {lengths} = {sum(lengths)} tokens, encoder_hidden_states holds {have} audio tokens")
        out = []
        for j, (length, s, tw) in enumerate(self.audio_prompts):
            if tw is not None and N not in tw:
                raise ValueError(f"audio_prompts: prompt {j} has no weight map for a call of {N} tokens (bound: {sorted(tw)})")
            out.append((length, self.scale if s is None else s, None if tw is None else tw[N]))
        return out

    def _call_train(self, attn, hidden_states, ehs, attention_mask, _residual, _ln):
        """Training mode (reference :347-470 under autograd; train_apadapter_v2.py:941-957): gradients w.r.t.
        hidden_states, to_k_ip.weight and to_v_ip.weight (and the condition tokens if they require grad)."""
        if self.scale_table is not None:
            raise ValueError("ap_scale: the training path keeps the float `scale`; clear_ap_scale_table() before a forward under autograd")
        if self.token_weights is not None:
            raise ValueError("ap_mask: the training path has no per-token weight; clear_ap_token_weights() before a forward under autograd")
        if self.audio_prompts is not None:
            raise ValueError("audio_prompts: the training path has one audio prompt; clear_audio_prompts() before a forward under autograd")
        B = hidden_states.shape[0]
        nt = self.num_tokens
        txt, aud = ehs[:, :nt, :].contiguous(), ehs[:, nt:, :].contiguous()
        if _ln is not None and _residual is hidden_states:
            hs, _residual = AG.layer_norm_res(hidden_states, *_ln)  # (the residual gradient joins the LayerNorm backward launch)
        else:
            hs = hidden_states if _ln is None else AG.layer_norm(hidden_states, *_ln)
        q = AG.linear(hs, attn.to_q.weight)
        k_t, v_t = AG.linear(txt, attn.to_k.weight), AG.linear(txt, attn.to_v.weight)
        bias = self._bias(attention_mask, B, txt.shape[1])
        if aud.shape[1] == 0:  # no audio tokens: the text branch alone (reference :435-445 on an empty slice contributes 0)
            o = AG.attention(q, k_t, v_t, attn.heads, bias)
        else:
            k_a, v_a = AG.linear(aud, self.to_k_ip.weight), AG.linear(aud, self.to_v_ip.weight)
            o = AG.ip_attention(q, k_t, v_t, k_a, v_a, attn.heads, bias, float(self.scale))
        return AG.linear(o, attn.to_out[0].weight, attn.to_out[0].bias, residual=_residual)
