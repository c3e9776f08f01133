"""CPU: the host side of ``ap_region=`` / ``ap_mask=`` -- the additive C ABI of the apad_*_qw entry points (header, ctypes mirror, exported
symbols, what they reject before any launch), ``processors.route(query_weighted=)``, ``scheduler.ap_mask_pyramid`` with
``UNet.attention_grids``, the keyword checks of the pipeline, the binding on the processors and the committed resource table.  No GPU compute."""
import ctypes as C
import os
import re

import pytest
import torch

import ap_adapter_amd as A
from ap_adapter_amd import _lib as L
from ap_adapter_amd import processors as P
from ap_adapter_amd.scheduler import ap_mask_pyramid

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "apadapter_hip.h")).read()
QW_ENTRIES = ("apad_attention_qw", "apad_cross_attention_rows_qw", "apad_hs_attention_qw")
QW_DESCS = ("apad_attn_desc", "apad_xrows_desc", "apad_hs_attn_desc")
NAN = float("nan")


# ---- the header and the ctypes mirror ----
def test_abi_version_is_still_12_and_the_entries_are_declared_bound_and_exported():
    assert re.search(r"^#define APAD_ABI_VERSION 12$", HEADER, re.M)
    assert A.lib().apad_abi_version() == 12
    declared = set(re.findall(r"\b(apad_[a-z0-9_]+)\s*\(", HEADER))
    h = C.CDLL(L.LIB_PATH)
    for name in QW_ENTRIES + ("apad_sizeof_query_weight",):
        assert name in declared and name in L.SYMBOLS, name
        getattr(h, name)  # AttributeError: declared but not exported
    for name, desc in zip(QW_ENTRIES, QW_DESCS):
        assert re.search(r"int %s\(const %s\* d, const apad_scale2_tab\* t[^,]*, const apad_query_weight\* w, void\* stream\);" % (name, desc),
                         HEADER), name
    assert "apad_fused_cross_attention_qw" not in HEADER  # the 256-wide kernel is deliberately left alone
    head = HEADER[:HEADER.index("#ifndef APADAPTER_HIP_H")]  # each is documented in the header's "what it replaces" list
    assert all(name in head for name in QW_ENTRIES)


def test_query_weight_layout_matches_the_header_and_no_descriptor_changed_size():
    body = re.search(r"typedef struct apad_query_weight \{(.*?)\} apad_query_weight;", HEADER, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            fields += [re.sub(r"[\s\*]", "", x).split(" ")[-1] for x in re.sub(r"^(const\s+)?\w+\s*\*?\s*", "", decl).split(",")]
    assert fields == [f[0] for f in L.QueryWeight._fields_] == ["w", "cols", "reserved", "ld"]
    h = A.lib()
    assert h.apad_sizeof_query_weight() == C.sizeof(L.QueryWeight) == 24
    assert (C.sizeof(L.AttnDesc), C.sizeof(L.XattnDesc), C.sizeof(L.XrowsDesc), C.sizeof(L.HsAttnDesc), C.sizeof(L.Scale2Tab)) == \
        (h.apad_sizeof_attn_desc(), h.apad_sizeof_xattn_desc(), h.apad_sizeof_xrows_desc(), h.apad_sizeof_hs_attn_desc(),
         h.apad_sizeof_scale2_tab()) == (200, 136, 152, 136, 32)


def test_the_map_arguments_are_rejected_before_any_launch():
    """what needs no device: a NULL struct or map, cols <= 0, ld < N, a map off 4-byte alignment, a single-segment call, and a bad table -- a
    negative code and a text naming the entry point, from every one of the three (the descriptor is not looked at before the two are)"""
    h = A.lib()
    buf = (C.c_float * 64)()
    base = C.addressof(buf)
    good_w, good_t = dict(w=base, cols=2, ld=16), dict(table=base, step=None, rows=2, cols=2, ld=2)
    bad_w = (dict(w=None), dict(cols=0), dict(cols=-3), dict(ld=15), dict(w=base + 2))
    bad_t = (dict(table=None), dict(rows=0), dict(cols=0), dict(ld=1), dict(table=base + 2), dict(step=base + 1))
    for name, desc in zip(QW_ENTRIES, (L.AttnDesc, L.XrowsDesc, L.HsAttnDesc)):
        fn = getattr(h, name)

        def call(L2=32, w_change=None, t_change=None, null_w=False, null_t=True):
            d, w, t = desc(), L.QueryWeight(), L.Scale2Tab()
            d.L2, d.N = L2, 16
            for k, v in {**good_w, **(w_change or {})}.items():
                setattr(w, k, v)
            for k, v in {**good_t, **(t_change or {})}.items():
                setattr(t, k, v)
            rc = fn(C.byref(d), None if null_t else C.byref(t), None if null_w else C.byref(w), None)
            return rc, h.apad_last_error().decode()

        cases = [dict(null_w=True), dict(L2=0), dict(L2=0, null_t=False)] + [dict(w_change=c) for c in bad_w] + \
                [dict(t_change=c, null_t=False) for c in bad_t]
        for kw in cases:
            rc, text = call(**kw)
            assert rc < 0 and text.startswith(name + ":"), (name, kw, rc, text)
        assert fn(None, None, None, None) < 0 and h.apad_last_error().decode().startswith(name + ":")


# ---- processors.route(query_weighted=) ----
def _site(kind, C_, heads, dtype):
    from ap_adapter_amd.unet import Attention
    attn = Attention(C_, None if kind == "self" else 768, heads, C_ // heads)
    attn.set_processor(A.IPAttnProcessor2_0(hidden_size=C_, name="site", cross_attention_dim=768, num_tokens=8, scale=0.5)
                       if kind == "decoupled" else A.AttnProcessor2_0())
    return attn.to(dtype).requires_grad_(False)


def test_query_weighted_route_turns_fused_into_chain_and_nothing_else():
    """a grid of (kind, C, N, L1, L2, masked, block entry) cells: the answer with query_weighted=True is the answer without it, except that
    "fused" becomes "chain"; the old positional call form and the keyword's default are the same call"""
    seen, changed = set(), 0
    for dtype in (torch.bfloat16, torch.float32):
        for kind in ("self", "cross", "decoupled"):
            for C_, heads, N in ((256, 8, 96), (256, 8, 1000), (384, 8, 40), (640, 8, 40), (640, 8, 100), (128, 4, 40)):
                attn = _site(kind, C_, heads, dtype)
                x = torch.zeros(2, N, C_, dtype=dtype)
                ln = (torch.ones(C_, dtype=dtype), torch.zeros(C_, dtype=dtype), 1e-5)
                lengths = [(0, 0)] if kind == "self" else [(16, 0), (77, 0)] if kind == "cross" else [(8, 0), (8, 32), (8, 128), (8, 512), (40, 40)]
                for L1, L2 in lengths:
                    for masked in (False, True):
                        for residual, ln_ in ((x, ln), (None, None)):
                            for same_batch in (True, False):
                                old = P.route(kind, attn, x, residual, ln_, L1, L2, masked, same_batch)
                                assert old == P.route(kind, attn, x, residual, ln_, L1, L2, masked, same_batch, query_weighted=False)
                                new = P.route(kind, attn, x, residual, ln_, L1, L2, masked, same_batch, query_weighted=True)
                                assert new == ("chain" if old == "fused" else old), (kind, C_, N, L1, L2, masked, old, new)
                                seen.add(old)
                                changed += old == "fused"
    assert seen == {"fused", "rows", "hs", "sattn", "chain"} and changed > 0


# ---- scheduler.ap_mask_pyramid and UNet.attention_grids ----
@pytest.fixture(scope="module")
def small_unet():
    cfg = A.UNetConfig(block_out_channels=(64, 128, 192, 256), attention_head_dim=4, norm_num_groups=16, cross_attention_dim=(None, 768, 1024, None))
    u = A.AudioLDM2UNet2DConditionModel(cfg)
    A.install_ap_adapter(u, None, scale=0.5)
    return u


@pytest.fixture(scope="module")
def pipe(small_unet):
    return A.AudioLDM2Pipeline(small_unet)


def test_attention_grids_follow_the_downsamplers(small_unet):
    """h -> (h + 1) // 2 per stride-2 downsampler; the first level (a plain DownBlock2D) holds no attention: one grid per level of the synthetic
    UNet's config that holds the adapter's sites (the GPU suite checks the same grids against the token counts of a forward: a binding without
    a level's count raises)"""
    assert small_unet.attention_grids(250, 16) == [(125, 8), (63, 4), (32, 2)]
    assert small_unet.attention_grids(26, 16) == [(13, 8), (7, 4), (4, 2)]
    assert small_unet.attention_grids(1, 1) == [(1, 1)] * 3
    # a UNet without the adapter holds no decoupled attn2
    assert A.AudioLDM2UNet2DConditionModel(small_unet.config).attention_grids(250, 16) == []
    # the channel widths of the levels that hold the adapter's sites: one grid per width
    widths = sorted({p.hidden_size for p in small_unet.attn_processors.values() if hasattr(p, "to_k_ip")})
    assert widths == [128, 192, 256] and len(widths) == len(small_unet.attention_grids(26, 16))


def test_region_pyramid_of_a_ten_second_clip(pipe, small_unet):
    """ap_region = (4.0, 7.0) on the 250 x 16 latent grid: rows 100 .. 174 (edit_region's rounding).  The latent-grid mask is exactly 0 / 1; each
    level equals adaptive_avg_pool2d, lies in [0, 1], is 1 well inside and 0 well outside, and is fractional only where a pooling window
    straddles an end of the region (row 175 is outside: the 125-row level's window 87 = rows 174, 175 weighs 0.5)"""
    mask = pipe.check_ap_mask((4.0, 7.0), None, 2, 250, 16, has_audio=True)
    assert tuple(mask.shape) == (1, 1, 250, 16) and mask.dtype == torch.float32
    want = torch.zeros(250)
    want[100:175] = 1.0
    assert torch.equal(mask[0, 0], want[:, None].expand(250, 16))
    grids = small_unet.attention_grids(250, 16)
    pyr = ap_mask_pyramid(mask, grids)
    assert sorted(pyr) == [32 * 2, 63 * 4, 125 * 8]
    for h, w in grids:
        level = pyr[h * w]
        assert tuple(level.shape) == (1, h * w) and level.dtype == torch.float32 and level.is_contiguous()
        pooled = torch.nn.functional.adaptive_avg_pool2d(mask, (h, w))
        assert torch.equal(level, pooled.reshape(1, h * w))  # row-major: token = row * w + column, the order of the processors' 4-D entry
        assert torch.equal(level.reshape(h, w)[:, 0], pooled[0, 0, :, 0])
        assert float(level.min()) >= 0.0 and float(level.max()) <= 1.0
        rows = level.reshape(h, w)[:, 0]
        frac = ((rows > 0) & (rows < 1)).nonzero().flatten().tolist()
        assert len(frac) <= 2 and bool((level.reshape(h, w) == rows[:, None]).all())
    r125 = pyr[1000].reshape(125, 8)[:, 0]
    assert bool((r125[50:87] == 1).all()) and float(r125[87]) == 0.5 and bool((r125[:50] == 0).all()) and bool((r125[88:] == 0).all())
    # an aligned region stays binary one level down
    aligned = ap_mask_pyramid(pipe.check_ap_mask((4.0, 7.04), None, 1, 250, 16, has_audio=True), grids)[1000]
    assert set(aligned.unique().tolist()) == {0.0, 1.0} and float(aligned.sum()) == 8 * 38


def test_pyramid_of_a_per_clip_mask_and_its_errors():
    mask = torch.zeros(3, 1, 26, 16)
    mask[0], mask[1, :, 5:15], mask[2, :, :, 4:12] = -1.5, 3.0, 0.25  # any finite value: negative, amplifying, a frequency band
    pyr = ap_mask_pyramid(mask, [(13, 8), (7, 4), (4, 2)])
    assert [tuple(pyr[n].shape) for n in (104, 28, 8)] == [(3, 104), (3, 28), (3, 8)]
    assert bool((pyr[104][0] == -1.5).all()) and float(pyr[104][1].max()) == 3.0
    assert torch.equal(pyr[104][2].reshape(13, 8)[0], torch.tensor([0, 0, 0.25, 0.25, 0.25, 0.25, 0, 0]))
    assert ap_mask_pyramid(mask, []) == {}
    for bad in (torch.zeros(26, 16), torch.zeros(1, 2, 26, 16), torch.full((1, 1, 26, 16), NAN), torch.full((1, 1, 26, 16), float("inf"))):
        with pytest.raises(ValueError, match="^ap_mask"):
            ap_mask_pyramid(bad, [(13, 8)])
    with pytest.raises(ValueError, match="^ap_mask: two attention levels"):
        ap_mask_pyramid(mask, [(4, 2), (2, 4)])


# ---- the keyword checks ----
def _embeds(tokens):
    return dict(prompt_embeds=torch.zeros(1, 16, 1024), negative_prompt_embeds=torch.zeros(1, 16, 1024),
                generated_prompt_embeds=torch.zeros(1, tokens, 768), negative_generated_prompt_embeds=torch.zeros(1, tokens, 768),
                attention_mask=torch.ones(1, 16), negative_attention_mask=torch.ones(1, 16), output_type="latent", num_inference_steps=4)


def test_every_value_error_of_the_keywords(pipe, small_unet):
    """through ``__call__`` (10.24 s: a 256 x 16 latent grid), before any device work"""
    nt = max(p.num_tokens for p in small_unet.attn_processors.values() if hasattr(p, "to_k_ip"))
    audio = _embeds(nt + 32)
    with pytest.raises(ValueError, match="^ap_mask and ap_region are both given"):
        pipe(ap_region=(1.0, 2.0), ap_mask=torch.ones(1, 1, 256, 16), **audio)
    for bad in (torch.ones(1, 1, 255, 16), torch.ones(3, 1, 256, 16), torch.ones(1, 2, 256, 16), torch.ones(1, 1, 1, 256, 16), torch.ones(256)):
        with pytest.raises(ValueError, match=r"^ap_mask \(.*\) is not broadcastable to \[1, 1, 256, 16\]"):
            pipe(ap_mask=bad, **audio)
    for bad in (NAN, float("inf")):
        m = torch.ones(1, 1, 256, 16)
        m[0, 0, 3, 3] = bad
        with pytest.raises(ValueError, match="^ap_mask values must be finite"):
            pipe(ap_mask=m, **audio)
    for kw in (dict(ap_region=(1.0, 2.0)), dict(ap_mask=torch.ones(1, 1, 256, 16))):  # text tokens only: no second segment
        with pytest.raises(ValueError, match="^%s needs an audio condition" % next(iter(kw))):
            pipe(**kw, **_embeds(nt))
    for region in ((10.0, 11.0), (-1.0, 2.0), (9.0, 10.5), (3.0, 2.0)):  # outside the 10.24 s clip, or reversed
        with pytest.raises(ValueError, match="^ap_region="):
            pipe(ap_region=region, **audio)
    for region in ((1.0, 1.01), (2.0, 2.0)):  # shorter than one 0.04 s latent row
        with pytest.raises(ValueError, match="^ap_region=.*at least one latent row"):
            pipe(ap_region=region, **audio)
    for region in ("4:7", (1.0,), (1.0, 2.0, 3.0), 4.0):
        with pytest.raises(ValueError, match="^ap_region=.*expected \\(start_s, end_s\\)"):
            pipe(ap_region=region, **audio)
    # what is accepted: lower-rank masks, a leading dimension of 1 or clips, any finite value; nothing given -> None
    assert pipe.check_ap_mask(None, None, 2, 26, 16) is None
    for ok, lead in ((torch.ones(26, 16), 1), (torch.full((1, 16), -2.0), 1), (torch.ones(2, 1, 1, 1).numpy(), 2), (3.0, 1), ([[0.5] * 16], 1)):
        assert tuple(pipe.check_ap_mask(None, ok, 2, 26, 16, has_audio=True).shape) == (lead, 1, 26, 16)
    # a UNet without the adapter has no audio branch to weigh
    plain = A.AudioLDM2Pipeline(A.AudioLDM2UNet2DConditionModel(small_unet.config))
    with pytest.raises(ValueError, match="^ap_region needs an audio condition"):
        plain.check_ap_mask((0.2, 0.6), None, 1, 26, 16, torch.zeros(2, nt + 32, 768))


def test_the_binding_reaches_every_decoupled_processor_and_the_training_path_refuses_it(small_unet):
    ip = [p for p in small_unet.attn_processors.values() if hasattr(p, "to_k_ip")]
    assert ip and all(p.token_weights is None and p._query_weight(104) is None for p in ip)
    maps = ap_mask_pyramid(torch.ones(2, 1, 26, 16), small_unet.attention_grids(26, 16))
    small_unet.set_ap_token_weights(maps, 2)
    try:
        assert small_unet._ap_mask_cols == 2
        for p in ip:
            for n in (104, 28, 8):
                b = p._query_weight(n)
                assert isinstance(b, tuple) and b.w is maps[n] and b.cols == 2
            with pytest.raises(ValueError, match="^ap_mask: no weight map is bound for a call of 416 tokens"):
                p._query_weight(416)
            with pytest.raises(ValueError, match="^ap_mask: the training path"):
                p._call_train(None, torch.zeros(1, 4, 64), torch.zeros(1, 40, 768), None, None, None)
            assert p.scale == 0.5 and p.scale_table is None
        assert all(p._query_weight(104) is None for p in small_unet.attn_processors.values() if not hasattr(p, "to_k_ip"))
    finally:
        small_unet.clear_ap_token_weights()
    assert small_unet._ap_mask_cols is None and all(p.token_weights is None for p in ip)


def test_run_sharded_takes_the_region():
    src = open(os.path.join(ROOT, "tools", "run_sharded.py")).read()
    assert '"--ap-region"' in src and 'aps["ap_region"]' in src


def test_committed_resource_table_shows_no_scratch_gained_and_no_occupancy_lost():
    """profiles/ap_region_resources.txt holds the compiler's figures of every instantiation of the four kernel files at the parent commit and
    with the map (tools/resource_table.py regenerates either half).  Every kernel of the parent is there under its old name or as the
    <..., false> instantiation of a template that gained a trailing ``bool = false``: none gained scratch, lost a wave or changed its LDS.
    The new instantiations keep the occupancy of their twins and none has scratch its twin does not have -- the chunked form of
    hs_attn_kernel (129 .. 512 audio keys) spills 84 bytes per lane at the parent already, 88 with the map (NOTES.md)."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("resource_table", os.path.join(ROOT, "tools", "resource_table.py"))
    rt = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(rt)
    path = os.path.join(ROOT, "profiles", "ap_region_resources.txt")
    before, raw = rt.parse(path, "parent commit"), rt.parse(path, "this commit")
    after = rt.under_old_names(before, raw)
    assert len(before) > 100 and set(before) <= set(after)
    assert {k[0] for k in after} == {"xattn.hip", "attention.hip", "hsattn.hip", "f32_ops.hip"}
    for k in before:
        assert after[k] == before[k], k  # not a register moved
    new = {k: v for k, v in after.items() if k not in before}
    assert len(new) == 60 and not any(k[0] == "xattn.hip" for k in new)
    twins = 0
    for (src, name), r in new.items():
        if "_qw_kernel" in name:  # attn_f32_qw_kernel<D> / attn_f32x3_qw_kernel<D>: the twin's name is three characters shorter
            twin = re.sub(r"(\d+)(attn_f32(x3)?)_qw_kernel", lambda m: "%d%s_kernel" % (int(m.group(1)) - 3, m.group(2)), name)
        else:
            assert "ELb1EEEv" in name, name
            twin = name.replace("ELb1EEEv", "EEEv", 1)
        t = before[(src, twin)]
        twins += 1
        assert r["waves"] == t["waves"] and r["lds"] == t["lds"], (name, r, t)
        if r["scratch"]:
            assert "hs_attn_kernel" in name and "Li16E" in name and (t["scratch"], r["scratch"]) == (84, 88), (name, r, t)
    assert twins == 60
