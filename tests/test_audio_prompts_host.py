"""CPU: the host side of ``audio_prompts=`` -- the additive C ABI of apad_attention_multi (header, ctypes mirror, the size check, what it rejects
before any launch), ``processors.route(multi=)``, the binding on the processors, ``AudioPrompt`` and the keyword's checks through ``__call__``,
``denoise`` and ``invert``, the condition layout, the graph key and the committed resource table.  No GPU compute."""
import ctypes as C
import os
import re

import pytest
import torch

import ap_adapter_amd as A
from ap_adapter_amd import _lib as L
from ap_adapter_amd import ops
from ap_adapter_amd import processors as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "apadapter_hip.h")).read()
NAME = "apad_attention_multi"


# ---- the header and the ctypes mirror ----
def test_abi_version_is_still_12_and_the_entry_is_declared_bound_and_exported():
    assert re.search(r"^#define APAD_ABI_VERSION 12$", HEADER, re.M) and A.lib().apad_abi_version() == 12
    declared = set(re.findall(r"\b(apad_[a-z0-9_]+)\s*\(", HEADER))
    h = C.CDLL(L.LIB_PATH)
    for name in (NAME, "apad_sizeof_attn_extra"):
        assert name in declared and name in L.SYMBOLS, name
        getattr(h, name)
    assert re.search(r"int apad_attention_multi\(const apad_attn_desc\* d, const apad_scale2_tab\* t, const apad_query_weight\* w,\s*"
                     r"const apad_attn_extra\* extra, int32_t n_extra, void\* stream\);", HEADER)
    assert NAME in HEADER[:HEADER.index("#ifndef APADAPTER_HIP_H")]  # documented in the header's "what it replaces" list
    doc = HEADER[HEADER.index("Several audio prompts in one launch"):HEADER.index("typedef struct apad_attn_extra")]
    assert "Kernel selection is per LAUNCH" in doc and "<= 64" in doc  # the documented selection rule


def test_the_extra_struct_matches_the_header_and_no_descriptor_changed_size():
    body = re.search(r"typedef struct apad_attn_extra \{(.*?)\} apad_attn_extra;", HEADER, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            fields += [re.sub(r"[\s\*]", "", x).split(" ")[-1] for x in re.sub(r"^(const\s+)?\w+\s*\*?\s*", "", decl).split(",")]
    want = ["k", "vt", "k_stride_b", "k_stride_l", "vt_stride_b", "L", "Lpad", "kv_batch_div", "reserved", "scale", "reserved_f", "tab", "qw"]
    assert fields == [f[0] for f in L.AttnExtra._fields_] == want
    h = A.lib()
    assert h.apad_sizeof_attn_extra() == C.sizeof(L.AttnExtra) == 120
    assert (h.apad_sizeof_attn_desc(), h.apad_sizeof_scale2_tab(), h.apad_sizeof_query_weight()) == (200, 32, 24)


def test_a_wrong_mirror_of_the_struct_fails_the_size_check(monkeypatch):
    """_lib.lib() compares apad_sizeof_attn_extra() with the ctypes struct: a mirror that lost a field is a RuntimeError at load"""
    class Short(C.Structure):
        _fields_ = L.AttnExtra._fields_[:-1]
    monkeypatch.setattr(L, "_lib", None)
    monkeypatch.setattr(L, "AttnExtra", Short)
    with pytest.raises(RuntimeError, match="descriptor layout mismatch"):
        L.lib()
    monkeypatch.undo()
    assert L.lib().apad_sizeof_attn_extra() == 120


def test_the_arguments_are_rejected_before_any_launch():
    """what needs no device: a negative code and a text naming the entry point"""
    h = A.lib()
    buf = (C.c_float * 256)()
    base = C.addressof(buf)

    def call(n_extra=1, null_extra=False, d_change=None, x_change=None, tab=None, qw=None, t=None, w=None):
        d = L.AttnDesc()
        d.L2, d.N = 32, 16
        for k, v in (d_change or {}).items():
            setattr(d, k, v)
        xs = (L.AttnExtra * 3)()
        for x in xs:
            x.k, x.vt, x.L, x.Lpad, x.kv_batch_div = base, base, 32, 32, 1
            x.k_stride_b = x.k_stride_l = x.vt_stride_b = 256
        for k, v in (x_change or {}).items():
            setattr(xs[max(n_extra, 1) - 1], k, v)
        for name, cls, val in (("tab", L.Scale2Tab, tab), ("qw", L.QueryWeight, qw)):
            if val is not None:
                s = cls()
                for k, v in val.items():
                    setattr(s, k, v)
                setattr(xs[max(n_extra, 1) - 1], name, s)
        ts, ws = L.Scale2Tab(), L.QueryWeight()
        for k, v in (t or {}).items():
            setattr(ts, k, v)
        for k, v in (w or {}).items():
            setattr(ws, k, v)
        rc = h.apad_attention_multi(C.byref(d), C.byref(ts) if t is not None else None, C.byref(ws) if w is not None else None,
                                    None if null_extra else xs, n_extra, None)
        return rc, h.apad_last_error().decode()

    good_t, good_w = dict(table=base, step=None, rows=2, cols=2, ld=2), dict(w=base, cols=2, ld=16)
    cases = [dict(n_extra=-1), dict(n_extra=4), dict(n_extra=2, null_extra=True), dict(d_change=dict(L2=0)), dict(d_change=dict(lse=base)),
             dict(n_extra=0, d_change=dict(L2=0)), dict(n_extra=0, d_change=dict(lse=base))]
    cases += [dict(n_extra=n, x_change=c) for n in (1, 3) for c in (dict(L=0), dict(L=-5), dict(Lpad=0), dict(L=40, Lpad=32), dict(L=30, Lpad=48),
                                                                     dict(kv_batch_div=0), dict(kv_batch_div=-1), dict(k=None), dict(vt=None))]
    for bad in (dict(rows=0), dict(cols=0), dict(ld=1), dict(table=base + 2), dict(step=base + 1)):
        cases += [dict(tab={**good_t, **bad}), dict(t={**good_t, **bad}), dict(n_extra=0, t={**good_t, **bad})]
    for bad in (dict(cols=0), dict(cols=-3), dict(ld=15), dict(w=base + 2)):
        cases += [dict(qw={**good_w, **bad}), dict(w={**good_w, **bad}), dict(n_extra=0, w={**good_w, **bad})]
    cases += [dict(t={**good_t, "table": None}), dict(w={**good_w, "w": None})]  # a given t / w must hold a table / a map
    for kw in cases:
        rc, text = call(**kw)
        assert rc < 0 and text.startswith(NAME + ":"), (kw, rc, text)
    assert h.apad_attention_multi(None, None, None, None, 0, None) < 0 and h.apad_last_error().decode().startswith(NAME + ":")


# ---- processors.route(multi=) ----
def _site(kind, C_, heads, dtype):
    from ap_adapter_amd.unet import Attention
    attn = Attention(C_, None if kind == "self" else 768, heads, C_ // heads)
    attn.set_processor(A.IPAttnProcessor2_0(hidden_size=C_, name="site", cross_attention_dim=768, num_tokens=8, scale=0.5)
                       if kind == "decoupled" else A.AttnProcessor2_0())
    return attn.to(dtype).requires_grad_(False)


def test_multi_route_answers_chain_for_decoupled_sites_and_leaves_the_others():
    """a grid of (kind, C, N, L1, L2, masked, block entry) cells: with multi=True every "decoupled" answer is "chain" -- at C = 256, 384 and 640
    the answer without it is "fused", "rows" and "hs" --, every "self" and "cross" answer is the answer without it, and the keyword's
    default is the old call"""
    seen, left = set(), set()
    for dtype in (torch.bfloat16, torch.float32):
        for kind in ("self", "cross", "decoupled"):
            for C_, heads, N in ((256, 8, 96), (256, 8, 1000), (384, 8, 40), (384, 8, 252), (640, 8, 40), (640, 8, 64), (128, 4, 40)):
                attn = _site(kind, C_, heads, dtype)
                x = torch.zeros(2, N, C_, dtype=dtype)
                ln = (torch.ones(C_, dtype=dtype), torch.zeros(C_, dtype=dtype), 1e-5)
                lengths = [(0, 0)] if kind == "self" else [(16, 0), (77, 0)] if kind == "cross" else [(8, 32), (8, 64), (8, 128)]
                for L1, L2 in lengths:
                    for masked in (False, True):
                        for residual, ln_ in ((x, ln), (None, None)):
                            for qw in (False, True):
                                old = P.route(kind, attn, x, residual, ln_, L1, L2, masked, True, query_weighted=qw)
                                assert old == P.route(kind, attn, x, residual, ln_, L1, L2, masked, True, query_weighted=qw, multi=False)
                                new = P.route(kind, attn, x, residual, ln_, L1, L2, masked, True, query_weighted=qw, multi=True)
                                if kind == "decoupled":
                                    assert new == "chain", (C_, N, L1, L2, masked, old, new)
                                    if dtype == torch.bfloat16:
                                        seen.add((C_, old))
                                else:
                                    assert new == old, (kind, C_, N, L1, L2, masked, old, new)
                                    left.add(old)
    assert {(256, "fused"), (384, "rows"), (640, "hs")} <= seen
    assert left == {"fused", "rows", "hs", "sattn", "chain"}  # (a "cross" site keeps its one-launch kernels: it has one segment)


# ---- the binding ----
@pytest.fixture(scope="module")
def small_unet():
    cfg = A.UNetConfig(block_out_channels=(64, 128, 192, 256), attention_head_dim=4, norm_num_groups=16, cross_attention_dim=(None, 768, 1024, None))
    u = A.AudioLDM2UNet2DConditionModel(cfg)
    A.install_ap_adapter(u, None, scale=0.5)
    return u


@pytest.fixture(scope="module")
def pipe(small_unet):
    return A.AudioLDM2Pipeline(small_unet)


def test_the_binding_reaches_every_decoupled_processor_and_the_training_path_refuses_it(small_unet):
    ip = [p for p in small_unet.attn_processors.values() if hasattr(p, "to_k_ip")]
    assert ip and all(p.audio_prompts is None for p in ip) and small_unet._ap_prompt_cols == ()
    ehs = torch.zeros(2, 8 + 32 + 40, 768)
    table, w = torch.ones(4, 3), torch.ones(3, 104)
    small_unet.set_audio_prompts([32, 40], [None, ops.Scale2Binding(table, None, 3)], [{104: ops.QueryWeight(w, 3)}, None])
    try:
        assert small_unet._ap_prompt_cols == (3, 3)  # every table's and map's column count: the batch-split rule reads them
        for p in ip:
            got = p._prompts(ehs, 104)
            assert [g[0] for g in got] == [32, 40] and got[0][1] == 0.5 and got[1][1].table is table and got[1][1].cols == 3
            assert got[0][2].w is w and got[0][2].cols == 3 and got[1][2] is None
            attn = _site("decoupled", 128, 4, torch.float32)
            segs = p._segments(attn, ehs, (32, 40))  # one (src, to_k_ip, to_v_ip) per prompt behind the text segment
            assert [tuple(s[0].shape) for s in segs] == [(2, 8, 768), (2, 32, 768), (2, 40, 768)]
            assert segs[1][1] is p.to_k_ip.weight and segs[2][1] is p.to_k_ip.weight and segs[2][2] is p.to_v_ip.weight
            assert p._kv_signature(attn, ehs, (32, 40))[-1] == (32, 40) and p._kv_signature(attn, ehs)[-1] != (32, 40)
            assert len(p._segments(attn, ehs)) == 2  # (a hoisted set keeps the split it was made with, whatever is bound when it is refreshed)
            with pytest.raises(ValueError, match=r"^audio_prompts: the bound prompts hold \[32, 40\] = 72 tokens"):
                p._prompts(torch.zeros(2, 8 + 64, 768), 104)
            with pytest.raises(ValueError, match="^audio_prompts: prompt 0 has no weight map for a call of 28 tokens"):
                p._prompts(ehs, 28)
            with pytest.raises(ValueError, match="^audio_prompts: the training path"):
                p._call_train(None, torch.zeros(1, 4, 64), ehs, None, None, None)
            assert p.scale == 0.5 and p.scale_table is None and p.token_weights is None
    finally:
        small_unet.clear_audio_prompts()
    assert small_unet._ap_prompt_cols == () and all(p.audio_prompts is None for p in ip)
    for bad in ([], [8] * 5, [8, 0]):
        with pytest.raises(ValueError, match="^audio_prompts"):
            ip[0].set_audio_prompts(bad)
    with pytest.raises(ValueError, match="^audio_prompts: 2 lengths, 1 scales"):
        ip[0].set_audio_prompts([8, 8], [0.5])
    assert ip[0].audio_prompts is None


def test_hoisted_kv_carries_a_segment_per_prompt():
    assert P._KV._fields == tuple(f"{n}{i}" for i in range(1, 6) for n in ("k", "vt", "pk"))
    assert P._KV(1, 2)[2:] == (None,) * 13


# ---- AudioPrompt and the keyword ----
def _embeds(tokens):
    return dict(prompt_embeds=torch.zeros(1, 16, 1024), negative_prompt_embeds=torch.zeros(1, 16, 1024),
                generated_prompt_embeds=torch.zeros(1, tokens, 768), negative_generated_prompt_embeds=torch.zeros(1, tokens, 768),
                attention_mask=torch.ones(1, 16), negative_attention_mask=torch.ones(1, 16), output_type="latent", num_inference_steps=4)


def test_every_value_error_of_the_keyword(pipe):
    """through ``__call__`` (10.24 s: a 256 x 16 latent grid), ``denoise`` and ``invert``, before any device work"""
    AP = A.AudioPrompt
    mel = torch.zeros(1, 1024, 128)
    with pytest.raises(ValueError, match="^AudioPrompt: mel and audio_file are both given"):
        AP(mel=mel, audio_file="a.wav")
    with pytest.raises(ValueError, match="^AudioPrompt: ap_mask and ap_region are both given"):
        AP(mel=mel, ap_region=(1.0, 2.0), ap_mask=torch.ones(1, 1, 256, 16))
    for bad in (0, -3, 2.5, True):
        with pytest.raises(ValueError, match="^AudioPrompt: length="):
            AP(length=bad)
    emb = _embeds(8)
    for bad, text in (([], ": expected 1 to 4 prompts, got 0"), ([AP(mel=mel)] * 5, ": expected 1 to 4 prompts, got 5"), (AP(mel=mel), ": expected a list"),
                      ([mel], r"\[0\]: expected an AudioPrompt"), ([AP(mel=mel), AP()], r"\[1\]: needs a recording, mel= or audio_file="),
                      ([AP(length=32), AP(mel=mel)], r"\[0\]: needs a recording")):
        with pytest.raises(ValueError, match="^audio_prompts" + text):
            pipe(audio_prompts=bad, **emb)
    both = AP(mel=mel)
    both.audio_file = "a.wav"  # (assigned behind the constructor's back: the list check repeats it)
    with pytest.raises(ValueError, match=r"^audio_prompts\[0\]: mel and audio_file are both given"):
        pipe(audio_prompts=[both], **emb)
    two = [AP(mel=mel), AP(mel=mel)]
    for kw in (dict(mel=mel), dict(audio_file="a.wav"), dict(ap_scale=0.5), dict(ap_region=(1.0, 2.0)), dict(ap_mask=torch.ones(1, 1, 256, 16))):
        with pytest.raises(ValueError, match="^audio_prompts is given together with %s" % next(iter(kw))):
            pipe(audio_prompts=two, **kw, **emb)
        with pytest.raises(ValueError, match="^audio_prompts is given together with %s" % next(iter(kw))):
            pipe(audio_prompts=two[:1], **kw, **emb)
    # every prompt's own schedule, region and mask, named by its index; one prompt is the keyword call and raises the keyword's own text
    for field, bad, text in (("ap_region", (10.0, 11.0), "ap_region="), ("ap_region", "4:7", r"ap_region=.*expected \(start_s, end_s\)"),
                             ("ap_region", (1.0, 1.01), "ap_region=.*at least one latent row"),
                             ("ap_mask", torch.ones(1, 1, 255, 16), r"ap_mask \(.*\) is not broadcastable to \[1, 1, 256, 16\]"),
                             ("ap_mask", torch.full((1, 1, 256, 16), float("nan")), "ap_mask values must be finite"),
                             ("ap_scale", [0.5] * 3, "ap_scale"), ("ap_scale", float("inf"), "ap_scale")):
        with pytest.raises(ValueError, match=r"^audio_prompts\[1\]\." + text):
            pipe(audio_prompts=[AP(mel=mel), AP(mel=mel, **{field: bad})], **emb)
        with pytest.raises(ValueError, match="^" + text):
            pipe(audio_prompts=[AP(mel=mel, **{field: bad})], **emb)
    # the embeddings path: length is required, a recording has no meaning, the lengths add up to the condition's audio tokens
    lat, ge, pe, am = torch.zeros(1, 8, 26, 16), torch.zeros(2, 8 + 72, 768), torch.zeros(2, 16, 1024), torch.ones(2, 16)
    src = A.EditSource(z0=torch.zeros(1, 8, 26, 16), x0=torch.zeros(1, 8, 26, 16))
    for run in (lambda **kw: pipe.denoise(lat, ge, pe, am, 4, 3.0, **kw), lambda **kw: pipe.invert(src, ge, pe, am, 4, 3.0, **kw)):
        with pytest.raises(ValueError, match=r"^audio_prompts\[1\]: length is required on the embeddings path"):
            run(audio_prompts=[AP(length=32), AP()])
        with pytest.raises(ValueError, match=r"^audio_prompts\[0\]: mel / audio_file have no meaning on the embeddings path"):
            run(audio_prompts=[AP(mel=mel, length=32), AP(length=40)])
        with pytest.raises(ValueError, match=r"^audio_prompts: the lengths \[32, 32\] add up to 64, the condition holds 72 audio tokens"):
            run(audio_prompts=[AP(length=32), AP(length=32)])
        with pytest.raises(ValueError, match="^audio_prompts is given together with ap_scale"):
            run(audio_prompts=[AP(length=32), AP(length=40)], ap_scale=0.5)
        with pytest.raises(ValueError, match="^audio_prompts: expected 1 to 4 prompts, got 0"):
            run(audio_prompts=[])
        with pytest.raises(ValueError, match=r"^audio_prompts\[0\]\.ap_region="):
            run(audio_prompts=[AP(length=32, ap_region=(5.0, 6.0)), AP(length=40)])
    plain = A.AudioLDM2Pipeline(A.AudioLDM2UNet2DConditionModel(pipe.unet.config))  # a UNet without the adapter has no audio branch
    with pytest.raises(ValueError, match="^audio_prompts needs the adapter's decoupled processors"):
        plain.denoise(lat, ge, pe, am, 4, 3.0, audio_prompts=[AP(length=32), AP(length=40)])


def test_condition_layout_of_two_prompts_of_different_token_counts():
    """[text | prompt 0 tokens | prompt 1 tokens]; the unconditional branch (and branch 0 of the three-branch form) gets the zero-mel tokens once
    per prompt"""
    g = torch.Generator().manual_seed(3)
    R = lambda *s: torch.randn(*s, generator=g)
    ge = R(4, 8, 768)  # [negative; positive] of two clips
    a0, a1, u0, u1 = R(1, 32, 768), R(1, 40, 768), R(1, 32, 768), R(1, 40, 768)
    asm = A.AudioLDM2Pipeline.assemble_condition
    neg, pos = ge.chunk(2)
    rep = lambda t: t.repeat(2, 1, 1)
    two = asm(ge, [a0, a1], [u0, u1], torch.float32)
    assert tuple(two.shape) == (4, 8 + 72, 768) and two.is_contiguous()
    assert torch.equal(two[:2], torch.cat([neg, rep(u0), rep(u1)], 1)) and torch.equal(two[2:], torch.cat([pos, rep(a0), rep(a1)], 1))
    three = asm(ge, [a0, a1], [u0, u1], torch.float32, branches=3)
    assert tuple(three.shape) == (6, 80, 768)
    assert torch.equal(three[:2], two[:2]) and torch.equal(three[2:4], torch.cat([neg, rep(a0), rep(a1)], 1)) and torch.equal(three[4:], two[2:])
    # one zero-mel tensor serves prompts of its token count, once per prompt; a list of one prompt is the plain call
    same = asm(ge, [a0, a0 + 1], u0, torch.float32)
    assert torch.equal(same[:2], torch.cat([neg, rep(u0), rep(u0)], 1))
    assert torch.equal(asm(ge, [a0], [u0], torch.bfloat16), asm(ge, a0, u0, torch.bfloat16))
    with pytest.raises(ValueError, match="^audio_prompts: every prompt needs zero-mel tokens of its own token count"):
        asm(ge, [a0, a1], u0, torch.float32)


class _Stop(Exception):
    pass


class _KeySpy(dict):
    """stands in for the pipeline's graph cache: the first look-up ends the call with the key it was made with"""
    def get(self, key, default=None):
        raise _Stop(key)


def _key_of(pipe, monkeypatch, **kw):
    monkeypatch.setattr(pipe, "_graphs", _KeySpy())
    lat, ge, pe, am = torch.zeros(2, 8, 26, 16), torch.zeros(4, 8 + 72, 768), torch.zeros(4, 16, 1024), torch.ones(4, 16)
    with pytest.raises(_Stop) as stop:
        pipe.denoise(lat, ge, pe, am, 4, 3.0, **kw)
    monkeypatch.undo()
    return stop.value.args[0]


def test_graph_key_gains_exactly_the_tuple_and_nothing_without_the_keyword(pipe, monkeypatch):
    AP = A.AudioPrompt
    base = _key_of(pipe, monkeypatch)
    assert not any(isinstance(x, tuple) and x and x[0] == "audio_prompts" for x in base)
    key = _key_of(pipe, monkeypatch, audio_prompts=[AP(length=32), AP(length=40)])
    assert key == base + (("audio_prompts", (32, 40), (None, None), (None, None)),)
    # tables and maps: their column counts only -- other weights, schedules and regions make the same key
    per_clip = torch.ones(2, 1, 26, 16)
    a = _key_of(pipe, monkeypatch, audio_prompts=[AP(length=32, ap_scale=0.3, ap_region=(0.2, 0.6)), AP(length=40, ap_scale=[[0.1, 0.2]], ap_mask=per_clip)])
    b = _key_of(pipe, monkeypatch, audio_prompts=[AP(length=32, ap_scale=[1.0, 0.7, 0.4, 0.1], ap_region=(0.4, 1.0)),
                                                  AP(length=40, ap_scale=[[0.9, -0.2]], ap_mask=per_clip * 0.5)])
    assert a == b == base + (("audio_prompts", (32, 40), (1, 2), (1, 2)),)
    assert [tuple(p["ap_scale"].shape) for p in pipe.last_audio_prompts] == [(4, 1), (4, 2)]
    assert [p["length"] for p in pipe.last_audio_prompts] == [32, 40] and sorted(pipe.last_audio_prompts[1]["ap_mask"]) == [8, 28, 104]
    assert torch.equal(pipe.last_audio_prompts[1]["ap_scale"], torch.tensor([[0.9, -0.2]]).expand(4, 2))
    assert _key_of(pipe, monkeypatch, audio_prompts=[AP(length=40), AP(length=32)]) == base + (("audio_prompts", (40, 32), (None, None), (None, None)),)
    three = _key_of(pipe, monkeypatch, audio_prompts=[AP(length=32), AP(length=8), AP(length=32, ap_scale=1.0)])
    assert three == base + (("audio_prompts", (32, 8, 32), (None, None, 1), (None, None, None)),)
    # a list of one prompt is the keyword call: the keyword's key
    assert _key_of(pipe, monkeypatch, audio_prompts=[AP(length=72)]) == base
    assert _key_of(pipe, monkeypatch, audio_prompts=[AP(length=72, ap_scale=0.3, ap_region=(0.2, 0.6))]) == \
        _key_of(pipe, monkeypatch, ap_scale=0.3, ap_region=(0.2, 0.6)) == base + (("ap_scale", 1), ("ap_mask", 1))
    assert all(p.audio_prompts is None for p in pipe.unet.attn_processors.values() if hasattr(p, "to_k_ip"))


def test_the_export_and_the_tool():
    assert A.AudioPrompt is __import__("ap_adapter_amd.pipeline", fromlist=["AudioPrompt"]).AudioPrompt
    assert ops.AudioSegment(1, 2, 3) == (1, 2, 3, 0.0, None, 1)
    src = open(os.path.join(ROOT, "tools", "run_sharded.py")).read()
    assert '"--audio-prompt"' in src and "audio_prompts" in src


def test_committed_resource_table_shows_no_register_moved_and_no_new_scratch():
    """profiles/audio_prompts_resources.txt holds the compiler's figures of every instantiation of attention.hip and f32_ops.hip at the parent
    commit and with apad_attention_multi.  Every kernel of the parent is there under its old name or as the <..., false> instantiation of a
    template that gained a trailing ``bool = false``: not a register moved.  The 42 new instantiations have no scratch and the LDS of their
    single-prompt twins (the map instantiations <..., true, true> / attn_f32*_qw_kernel); the runtime loop over the prompts costs registers,
    and with them at most ONE wave per SIMD against the twin (NOTES.md lists which) -- the long form keeps its twin's occupancy at d = 32 and
    d = 48, the head sizes of the two large levels."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("resource_table", os.path.join(ROOT, "tools", "resource_table.py"))
    rt = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(rt)
    path = os.path.join(ROOT, "profiles", "audio_prompts_resources.txt")
    before, raw = rt.parse(path, "parent commit"), rt.parse(path, "this commit")
    after = rt.under_old_names(before, raw)
    assert len(before) > 100 and set(before) <= set(after) and {k[0] for k in after} == {"attention.hip", "f32_ops.hip"}
    for k in before:
        assert after[k] == before[k], k
    new = {k: v for k, v in after.items() if k not in before}
    assert len(new) == 42 and all(r["scratch"] == 0 for r in new.values())
    twins = 0
    for (src, name), r in new.items():
        if src == "f32_ops.hip":
            assert "_multi_kernel" in name
            twin = re.sub(r"(\d+)(attn_f32(x3)?)_multi_kernel(.*)NS_5A32MPE", lambda m: "%d%s_qw_kernel%sNS_4A32PE" % (int(m.group(1)) - 3, m.group(2), m.group(4)), name)
        else:
            assert "ELb1ELb0ELb1EEEv" in name, name
            twin = name.split("ELb1ELb0ELb1EEEv")[0] + "ELb1ELb1EEEvNS_5AttnPE"
        t = before[(src, twin)]
        twins += 1
        assert t["waves"] - 1 <= r["waves"] <= t["waves"] and r["lds"] == t["lds"], (name, r, t)
        if "11attn_kernel" in name and ("ELi32E" in name or "ELi48E" in name):
            assert r["waves"] == t["waves"], (name, r, t)
    assert twins == 42
