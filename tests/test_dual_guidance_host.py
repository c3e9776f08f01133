"""CPU: separate audio and text guidance as host arithmetic and public surface -- the C ABI line, the guidance table, the six-column
plan at eta = 0, the three-branch condition assembly, the argument checks of the pipeline call and the restatement's own identities.
No GPU compute.  PARITY UNPINNED (see guidance_oracle)."""
import inspect
import os
import re

import pytest
import torch

import ap_adapter_amd as A
from ap_adapter_amd import _lib as L
from ap_adapter_amd import scheduler as S

import guidance_oracle as GO
import sampler_oracle as SO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_abi_declares_the_dual_step_and_keeps_its_version():
    header = open(os.path.join(ROOT, "include", "apadapter_hip.h")).read()
    assert re.search(r"#define APAD_ABI_VERSION 12\b", header)  # additive: the version line stays
    index = header.split("#ifndef APADAPTER_HIP_H")[0]
    name, nargs = "apad_cfg_dual_step", 20
    assert re.search(r"\bint %s\s*\(" % name, header) and name in index
    decl = re.search(r"\bint %s\s*\(([^)]*)\)" % name, header).group(1)
    assert len(decl.split(",")) == nargs and "const float* guidance" in decl and "guidance_scale" not in decl
    assert name in L.SYMBOLS and len(L.SYMBOLS[name][1]) == nargs
    # the three existing entry points' rows are untouched
    assert [len(L.SYMBOLS[n][1]) for n in ("apad_cfg_ddim_step", "apad_cfg_sampler_step", "apad_cfg_edit_step")] == [11, 14, 20]
    if os.path.exists(L.LIB_PATH):
        assert A.lib().apad_abi_version() == 12 and hasattr(A.lib(), name)


def test_guidance_table_scalar_sequence_and_start():
    t = S.guidance_table(2.5, 7.5, 6)
    assert t.dtype == torch.float32 and t.shape == (6, 2) and t.is_contiguous()
    assert torch.equal(t, torch.tensor([[2.5, 7.5]] * 6))
    seq_a, seq_t = GO.ramp(1.0, 4.0, 6), GO.ramp(7.5, 3.0, 6)
    t = S.guidance_table(seq_a, seq_t, 6)
    assert torch.equal(t, torch.tensor([seq_a, seq_t], dtype=torch.float64).t().float())
    t = S.guidance_table(seq_a, 7.5, 6, start=2)  # an edit run entering the grid at index 2: rows 2: of the full grid
    assert t.shape == (4, 2) and torch.equal(t[:, 0], torch.tensor(seq_a[2:], dtype=torch.float64).float()) and bool((t[:, 1] == 7.5).all())
    assert torch.equal(S.guidance_table(torch.tensor(seq_a), tuple(seq_t), 6), S.guidance_table(seq_a, seq_t, 6))
    assert torch.equal(S.guidance_table(0, 0.0, 3), torch.zeros(3, 2))  # 0 is a legal scale: that branch does not guide
    # rows before ``start`` are never read, and may hold anything
    nan = float("nan")
    assert torch.equal(S.guidance_table([nan, nan, 1.0, 2.0], 3.0, 4, start=2), torch.tensor([[1.0, 3.0], [2.0, 3.0]]))


@pytest.mark.parametrize("arg", ["audio", "text"])
def test_guidance_table_rejections_name_the_argument(arg):
    other = "text" if arg == "audio" else "audio"
    call = lambda v, n=5, **kw: S.guidance_table(**{arg: v, other: 2.0}, num_inference_steps=n, **kw)
    for bad in ([1.0] * 4, [1.0] * 6, []):  # wrong length
        with pytest.raises(ValueError, match=rf"^{arg} holds {len(bad)} values"):
            call(bad)
    for bad in (-0.5, [1.0, 1.0, -1e-9, 1.0, 1.0], float("nan"), float("inf"), -float("inf"), [1.0, float("nan"), 1.0, 1.0, 1.0],
                [1.0, 1.0, 1.0, 1.0, float("inf")]):
        with pytest.raises(ValueError, match=rf"^{arg}=.*finite and >= 0"):
            call(bad)
    with pytest.raises(ValueError, match=rf"^{arg}="):
        call("loud")
    with pytest.raises(ValueError, match=rf"^{arg}=.*finite"):  # a bad value inside the slice
        call([1.0, 1.0, 1.0, float("nan"), 1.0], start=3)
    with pytest.raises(ValueError, match="start"):
        call(1.0, start=5)


def test_assemble_condition_three_branches_on_labelled_tensors():
    num, Lt, La, D = 2, 3, 2, 4
    neg = torch.arange(num).reshape(num, 1, 1).expand(num, Lt, D) + 100.0  # clip c's negative text: 100 + c
    pos = torch.arange(num).reshape(num, 1, 1).expand(num, Lt, D) + 200.0  # positive text: 200 + c
    ge = torch.cat([neg, pos])
    aud, unc = torch.full((1, La, D), 7.0), torch.full((1, La, D), -7.0)
    three = A.AudioLDM2Pipeline.assemble_condition(ge, aud, unc, torch.float32, branches=3)
    assert three.shape == (3 * num, Lt + La, D) and three.is_contiguous()
    for c in range(num):
        for branch, (text, audio) in enumerate(((100.0 + c, -7.0), (100.0 + c, 7.0), (200.0 + c, 7.0))):
            row = three[branch * num + c]
            assert bool((row[:Lt] == text).all()) and bool((row[Lt:] == audio).all()), (c, branch)  # text tokens first, audio after
    # the default is today's two halves, and they are branches 0 and 2
    two = A.AudioLDM2Pipeline.assemble_condition(ge, aud, unc, torch.float32)
    today = torch.cat([torch.cat([neg, unc.repeat(num, 1, 1)], 1), torch.cat([pos, aud.repeat(num, 1, 1)], 1)])
    assert torch.equal(two, today) and torch.equal(two, A.AudioLDM2Pipeline.assemble_condition(ge, aud, unc, torch.float32, branches=2))
    assert torch.equal(two, torch.cat([three[:num], three[2 * num:]]))
    assert A.AudioLDM2Pipeline.assemble_condition(ge, aud, unc, torch.bfloat16, branches=3).dtype == torch.bfloat16
    with pytest.raises(ValueError, match="branches"):
        A.AudioLDM2Pipeline.assemble_condition(ge, aud, unc, torch.float32, branches=4)


@pytest.mark.parametrize("n", [10, 50])
def test_dual_plan_is_six_column_and_the_default_plan_is_todays(n):
    d = A.DDIMScheduler()
    d.set_timesteps(n)
    p0 = d.sampler_plan()
    assert p0.legacy and p0.key == ("DDIMScheduler", 1, "leading", 1000, 1, (0.0015, 0.0195, False), 0.0) and torch.equal(p0.table, d.coef_table())
    p = d.sampler_plan(dual=True)
    assert not p.legacy and not p.needs_noise and not p.needs_history and p.keep is None and p.table.shape == (n, 6) and "dual" in p.key
    assert p.key != p0.key and p.key[:len(p0.key)] == p0.key
    assert torch.equal(p.table[:, :2], d.sampler_rows(0.0)[:, :2].float()) and bool((p.table[:, 2:] == 0).all())
    assert torch.equal(p.table, d.sampler_rows(0.0).float())
    pe = d.sampler_plan(0.5, dual=True)
    assert torch.equal(pe.table, d.sampler_plan(0.5).table) and pe.needs_noise and pe.key != d.sampler_plan(0.5).key
    pm = d.sampler_plan(0.0, start=3, masked=True, dual=True)
    assert torch.equal(pm.table, d.sampler_plan(0.0, start=3, masked=True).table) and torch.equal(pm.keep, d.keep_table(3)) and pm.start == 3
    m = A.DPMSolverMultistepScheduler()
    m.set_timesteps(n)
    q0, q = m.sampler_plan(), m.sampler_plan(dual=True)
    assert q0.key == ("DPMSolverMultistepScheduler", 2, "leading", True, 1000, 1, (0.0015, 0.0195))
    assert torch.equal(q.table, q0.table) and q.needs_history and q.key == q0.key + ("dual",)
    # the six-column rows at eta = 0 are the restatement's deterministic DDIM step
    acp, ts = SO.acp64(), SO.grid(n)
    x, e = torch.randn(64, generator=torch.Generator().manual_seed(1)).double(), torch.randn(64, generator=torch.Generator().manual_seed(2)).double()
    for i in (0, n // 2, n - 1):
        r = d.sampler_rows(0.0)[i]
        ref = SO.ddim_step(x, e, None, i, ts, acp)
        assert float((r[0] * x + r[1] * e - ref).abs().max()) < 1e-12


@pytest.fixture(scope="module")
def pipe_kw():
    u = A.AudioLDM2UNet2DConditionModel(A.UNetConfig(block_out_channels=(64, 128, 192, 256), attention_head_dim=4, norm_num_groups=16))
    B = 2
    e, ge = torch.zeros(B, 16, 1024), torch.zeros(B, 8, 768)
    kw = dict(prompt_embeds=e, negative_prompt_embeds=e, generated_prompt_embeds=ge, negative_generated_prompt_embeds=ge,
              attention_mask=e[..., 0], negative_attention_mask=e[..., 0], audio_length_in_s=1.04, num_inference_steps=10, output_type="latent")
    return u, kw


def test_call_needs_an_audio_condition_and_checks_the_scales_first(pipe_kw, monkeypatch):
    u, kw = pipe_kw
    pipe = A.AudioLDM2Pipeline(u)
    reached = []
    monkeypatch.setattr(pipe, "encode_prompt", lambda *a, **k: reached.append("encode_prompt"))
    monkeypatch.setattr(pipe, "denoise", lambda *a, **k: reached.append("denoise"))
    with pytest.raises(ValueError, match=r"audio_guidance_scale needs an audio condition \(mel= or audio_file=\)"):
        pipe(audio_guidance_scale=2.0, **kw)
    mel = torch.zeros(1, 1024, 128)
    with pytest.raises(ValueError, match=r"^audio=-1"):
        pipe(audio_guidance_scale=-1.0, mel=mel, **kw)
    with pytest.raises(ValueError, match=r"^text holds 3 values"):
        pipe(audio_guidance_scale=2.0, guidance_scale=[7.5, 7.5, 7.5], mel=mel, **kw)
    assert reached == []  # every check above ran before any encoder or device work
    assert inspect.signature(pipe.__call__).parameters["audio_guidance_scale"].default is None
    assert inspect.signature(A.AudioLDM2Pipeline.denoise).parameters["audio_guidance_scale"].default is None


def test_the_restatement_collapses_to_the_two_branch_expression():
    """with e_A == e_0, or e_AT == e_A, the rounded three-branch combine IS sampler_oracle.cfg_combine_rounded, value for value; at
    s_A = s_T = g it is the reference's formula up to fp32 rounding; and for f16 inputs at dyadic scales, rounding the exact fma once
    to f16 and rounding it through fp32 agree on every value (so the kernel-level identities do not depend on how a compiler folds the
    f16 rounding of the two-branch kernel)"""
    g = torch.Generator().manual_seed(3)
    for dtype in (torch.bfloat16, torch.float16, torch.float32):
        u, a, c = ((torch.randn(3, 4000, generator=g) * 0.5).to(dtype).float() for _ in range(3))
        for gs, s_other in ((7.5, 2.5), (2.5, 1.25), (1.25, 7.5)):
            two = SO.cfg_combine_rounded(torch.cat([u, c]), gs, dtype)
            assert torch.equal(GO.cfg3_combine_rounded(torch.cat([u, u, c]), s_other, gs, dtype), two)
            assert torch.equal(GO.cfg3_combine_rounded(torch.cat([u, c, c]), gs, s_other, dtype), two)
        e3 = torch.cat([u, a, c])
        both = GO.cfg3_combine_rounded(e3, 7.5, 7.5, torch.float32)
        two = SO.cfg_combine_rounded(torch.cat([u, c]), 7.5, torch.float32)
        err = float((both - two).abs().max() / two.abs().max())
        assert err < 1e-6, err
        assert float((GO.cfg3_combine_rounded(e3, 1.7, 6.1, torch.float32) - GO.cfg3_combine_exact(e3, 1.7, 6.1)).abs().max()) < 1e-5
    u, c = ((torch.randn(3, 64000, generator=g) * 0.5).to(torch.float16).float() for _ in range(2))
    for gs in (7.5, 2.5, 1.25):
        exact = gs * (c.double() - u.double()).float().double() + u.double()  # the fp32 difference, then the exact fma in float64
        # (float64 holds the product and the sum of these operands exactly enough for a single rounding to f16: 24 + 4 bits)
        assert torch.equal(exact.to(torch.float16), exact.float().to(torch.float16))
