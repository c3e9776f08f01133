"""CPU: the host side of ``ap_scale=`` -- scheduler.ap_scale_table, the additive C ABI of the apad_*_tab entry points (header, ctypes mirror,
exported symbols, the echo) and the argument errors the pipeline and the processors raise before any device work.  No GPU compute."""
import ctypes as C
import math
import os
import re

import pytest
import torch

import ap_adapter_amd as A
from ap_adapter_amd import _lib as L
from ap_adapter_amd.scheduler import ap_scale_table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "apadapter_hip.h")).read()
TAB_ENTRIES = ("apad_attention_tab", "apad_fused_cross_attention_tab", "apad_cross_attention_rows_tab", "apad_hs_attention_tab")
NAN = float("nan")


# ---- scheduler.ap_scale_table ----
def test_table_shapes_of_the_three_forms():
    t = ap_scale_table(0.55, 5)
    assert t.dtype == torch.float32 and tuple(t.shape) == (5, 1) and t.is_contiguous() and bool((t == torch.tensor(0.55)).all())
    sched = [1.0, 0.75, 0.5, 0.25, -0.5]  # any finite value, negative included
    t = ap_scale_table(sched, 5)
    assert tuple(t.shape) == (5, 1) and t[:, 0].tolist() == sched
    assert torch.equal(ap_scale_table(torch.tensor(sched), 5), t) and torch.equal(ap_scale_table(tuple(sched), 5), t)
    grid = [[0.1 * i + j for j in range(3)] for i in range(5)]
    t = ap_scale_table(grid, 5, clips=3)
    assert tuple(t.shape) == (5, 3) and torch.equal(t, torch.tensor(grid, dtype=torch.float64).float())
    assert torch.equal(ap_scale_table(torch.tensor(grid), 5), t)  # clips not given: the columns are taken as they come


def test_a_single_row_is_broadcast_over_the_steps():
    t = ap_scale_table([[0.0, 0.5, 1.0, 2.0]], 3, clips=4)
    assert tuple(t.shape) == (3, 4) and all(t[i].tolist() == [0.0, 0.5, 1.0, 2.0] for i in range(3))
    assert torch.equal(ap_scale_table(torch.tensor([[0.0, 0.5, 1.0, 2.0]]), 3, clips=4), t)


def test_start_slices_and_tolerates_nan_before_it():
    t = ap_scale_table([NAN, NAN, 0.5, 0.25], 4, start=2)
    assert tuple(t.shape) == (2, 1) and t[:, 0].tolist() == [0.5, 0.25]
    t = ap_scale_table([[NAN, math.inf], [1.0, 2.0], [3.0, 4.0]], 3, start=1, clips=2)
    assert t.tolist() == [[1.0, 2.0], [3.0, 4.0]]
    assert tuple(ap_scale_table(0.3, 6, start=4).shape) == (2, 1)
    assert tuple(ap_scale_table([[0.3, 0.4]], 6, start=4).shape) == (2, 2)


@pytest.mark.parametrize("bad,kw", [
    ([1.0, NAN, 1.0], {}), (NAN, {}), (math.inf, {}), ([1.0, -math.inf, 0.0], {}), ([[1.0, NAN]], {}),
    ([NAN, 1.0, NAN], dict(start=1)),                       # a NaN inside the run
    ([1.0, 2.0], {}), ([1.0, 2.0, 3.0, 4.0], {}), ([], {}),  # wrong length: a 1-D sequence is always per step
    ([[1.0, 2.0], [3.0, 4.0]], {}),                        # 2 rows for 3 steps
    ([[1.0, 2.0, 3.0]], dict(clips=2)), ([[1.0]] * 3, dict(clips=2)), ([[1.0, 2.0], [1.0], [1.0, 2.0]], {}),  # wrong B / ragged rows
    ("loud", {}), ([["a"]], {}), (0.5, dict(start=3)), (0.5, dict(start=-1)),
])
def test_rejected_values_raise_value_errors_that_start_with_ap_scale(bad, kw):
    with pytest.raises(ValueError, match="^ap_scale"):
        ap_scale_table(bad, 3, **kw)


# ---- the header and the ctypes mirror ----
def test_abi_version_is_still_12_and_the_entries_are_declared_and_exported():
    assert re.search(r"^#define APAD_ABI_VERSION 12$", HEADER, re.M)
    assert A.lib().apad_abi_version() == 12
    declared = set(re.findall(r"\b(apad_[a-z0-9_]+)\s*\(", HEADER))
    h = C.CDLL(L.LIB_PATH)
    for name in TAB_ENTRIES + ("apad_sizeof_scale2_tab", "apad_echo_scale2_tab"):
        assert name in declared and name in L.SYMBOLS, name
        getattr(h, name)  # AttributeError: declared but not exported
    for name, desc in zip(TAB_ENTRIES, ("apad_attn_desc", "apad_xattn_desc", "apad_xrows_desc", "apad_hs_attn_desc")):
        assert re.search(r"int %s\(const %s\* d, const apad_scale2_tab\* t, void\* stream\);" % (name, desc), HEADER), name
    # each is documented in the header's "what it replaces" list
    head = HEADER[:HEADER.index("#ifndef APADAPTER_HIP_H")]
    assert all(name in head for name in TAB_ENTRIES) and "attention_processor.py:454" in head


def test_scale2_tab_layout_matches_the_header_and_round_trips():
    body = re.search(r"typedef struct apad_scale2_tab \{(.*?)\} apad_scale2_tab;", HEADER, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            fields += [re.sub(r"[\s\*]", "", x).split(" ")[-1] for x in re.sub(r"^(const\s+)?\w+\s*\*?\s*", "", decl).split(",")]
    assert fields == [f[0] for f in L.Scale2Tab._fields_] == ["table", "step", "rows", "cols", "ld"]
    h = A.lib()
    assert h.apad_sizeof_scale2_tab() == C.sizeof(L.Scale2Tab) == 32
    t = L.Scale2Tab()
    for i, n in enumerate(fields):
        setattr(t, n, i + 1)
    out = (C.c_double * 8)()
    assert h.apad_echo_scale2_tab(C.byref(t), out, 8) == 5 and list(out)[:5] == [1.0, 2.0, 3.0, 4.0, 5.0]


def test_existing_descriptors_did_not_change_size():
    h = A.lib()
    assert (C.sizeof(L.AttnDesc), C.sizeof(L.XattnDesc), C.sizeof(L.XrowsDesc), C.sizeof(L.HsAttnDesc)) == \
        (h.apad_sizeof_attn_desc(), h.apad_sizeof_xattn_desc(), h.apad_sizeof_xrows_desc(), h.apad_sizeof_hs_attn_desc()) == (200, 136, 152, 136)


def test_the_table_arguments_are_rejected_before_any_launch():
    """what needs no device: a NULL table, rows / cols <= 0, ld < cols, a pointer off 4-byte alignment, a single-segment call -- a negative code
    and a text naming the entry point, from every one of the four (the descriptor is not looked at before the table is)"""
    h = A.lib()
    descs = (L.AttnDesc, L.XattnDesc, L.XrowsDesc, L.HsAttnDesc)
    buf = (C.c_float * 16)()
    base = C.addressof(buf)
    good = dict(table=base, step=None, rows=2, cols=2, ld=2)
    cases = (dict(table=None), dict(rows=0), dict(rows=-1), dict(cols=0), dict(cols=-3), dict(ld=1), dict(table=base + 2), dict(step=base + 1))
    for name, desc in zip(TAB_ENTRIES, descs):
        fn = getattr(h, name)
        for L2 in (32, 0):
            for change in (cases if L2 else ({},)):
                d, t = desc(), L.Scale2Tab()
                d.L2 = L2
                for k, v in {**good, **change}.items():
                    setattr(t, k, v)
                assert fn(C.byref(d), C.byref(t), None) < 0, (name, change)
                text = h.apad_last_error().decode()
                assert text.startswith(name + ":") and ("scale2" in text), (name, change, text)
        d = desc()
        d.L2 = 32
        assert fn(C.byref(d), None, None) < 0 and h.apad_last_error().decode().startswith(name + ":")


# ---- argument errors of the pipeline and the processors ----
@pytest.fixture(scope="module")
def small_unet():
    cfg = A.UNetConfig(block_out_channels=(64, 128, 192, 256), attention_head_dim=4, norm_num_groups=16, cross_attention_dim=(None, 768, 1024, None))
    u = A.AudioLDM2UNet2DConditionModel(cfg)
    A.install_ap_adapter(u, None, scale=0.5)
    return u


def _embeds(tokens):
    return dict(prompt_embeds=torch.zeros(1, 16, 1024), negative_prompt_embeds=torch.zeros(1, 16, 1024),
                generated_prompt_embeds=torch.zeros(1, tokens, 768), negative_generated_prompt_embeds=torch.zeros(1, tokens, 768),
                attention_mask=torch.ones(1, 16), negative_attention_mask=torch.ones(1, 16), output_type="latent", num_inference_steps=4)


def test_ap_scale_without_an_audio_condition_raises(small_unet):
    pipe = A.AudioLDM2Pipeline(small_unet)
    nt = max(p.num_tokens for p in small_unet.attn_processors.values() if hasattr(p, "to_k_ip"))
    with pytest.raises(ValueError, match="^ap_scale needs an audio condition"):
        pipe(ap_scale=0.5, **_embeds(nt))  # text tokens only: no second segment
    with pytest.raises(ValueError, match="^ap_scale needs an audio condition"):
        pipe.check_ap_scale([0.5] * 4, 4, 0, 1, torch.zeros(2, nt, 768))
    # with audio tokens behind the text tokens the value is checked next, still on the host
    with pytest.raises(ValueError, match="^ap_scale holds 3 rows"):
        pipe(ap_scale=[0.5, 0.5, 0.5], **_embeds(nt + 32))
    with pytest.raises(ValueError, match="^ap_scale holds 2 per-clip values"):
        pipe(ap_scale=[[0.5, 0.25]], **_embeds(nt + 32))
    with pytest.raises(ValueError, match="^ap_scale: every value"):
        pipe(ap_scale=[0.5, NAN, 0.5, 0.5], **_embeds(nt + 32))
    t = pipe.check_ap_scale([[0.0, 1.0]], 4, 1, 2, torch.zeros(4, nt + 32, 768))
    assert tuple(t.shape) == (3, 2) and pipe.check_ap_scale(None, 4, 0, 2) is None
    # a UNet without the adapter has no audio branch to weigh
    plain = A.AudioLDM2Pipeline(A.AudioLDM2UNet2DConditionModel(small_unet.config))
    with pytest.raises(ValueError, match="^ap_scale needs an audio condition"):
        plain.check_ap_scale(0.5, 4, 0, 1, torch.zeros(2, nt + 32, 768))


def test_the_binding_reaches_every_decoupled_processor_and_the_training_path_refuses_it(small_unet):
    ip = [p for p in small_unet.attn_processors.values() if hasattr(p, "to_k_ip")]
    assert ip and all(p.scale_table is None and p._scale2() == 0.5 for p in ip)
    table, step = torch.zeros(3, 2), torch.zeros(1, dtype=torch.int32)
    small_unet.set_ap_scale_table(table, step)
    try:
        for p in ip:
            b = p._scale2()
            assert isinstance(b, tuple) and b.table is table and b.step_ptr is step and b.cols == 2 and p.scale == 0.5  # ``scale`` untouched
            with pytest.raises(ValueError, match="^ap_scale: the training path keeps the float"):
                p._call_train(None, torch.zeros(1, 4, 64), torch.zeros(1, 40, 768), None, None, None)
        assert all(p._scale2() == 0.0 for p in small_unet.attn_processors.values() if not hasattr(p, "to_k_ip"))
    finally:
        small_unet.clear_ap_scale_table()
    assert all(p.scale_table is None and p._scale2() == 0.5 for p in ip)


def test_committed_resource_table_shows_no_scratch_gained_and_no_occupancy_lost():
    """profiles/ap_scale_table_resources.txt holds the compiler's figures of every instantiation of the four kernel files at the parent commit
    and with the table (tools/resource_table.py regenerates either half): every kernel is in both, none gained scratch, none lost a wave"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("resource_table", os.path.join(ROOT, "tools", "resource_table.py"))
    rt = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(rt)
    path = os.path.join(ROOT, "profiles", "ap_scale_table_resources.txt")
    before, after = rt.parse(path, "parent commit"), rt.parse(path, "this commit")
    assert len(before) > 100 and set(before) == set(after)
    assert {k[0] for k in after} == {"xattn.hip", "attention.hip", "hsattn.hip", "f32_ops.hip"}
    for k in before:
        assert after[k]["scratch"] <= before[k]["scratch"] and after[k]["waves"] >= before[k]["waves"] and after[k]["lds"] == before[k]["lds"], k
