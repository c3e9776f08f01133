"""CPU: editing from a source clip as host arithmetic -- the start index, the sliced coefficient tables and the keep table of
``sampler_plan(start=, masked=)`` against the independent fp64 restatement (tests/edit_oracle.py), every argument check of the
pipeline call, and the public surface.  No GPU compute.  PARITY UNPINNED (see edit_oracle)."""
import os
import re

import pytest
import torch

import ap_adapter_amd as A
from ap_adapter_amd import _lib as L
from ap_adapter_amd.scheduler import edit_start_index

import edit_oracle as EO
import sampler_oracle as SO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max())


@pytest.mark.parametrize("n", [4, 8, 10, 12, 50, 100, 200])
def test_edit_start_index_grid(n):
    for strength in (0.1, 0.25, 0.3, 0.5, 0.75, 0.99, 1.0):
        run = min(int(n * strength), n)
        if run == 0:
            with pytest.raises(ValueError, match="strength"):
                edit_start_index(n, strength)
            continue
        k = edit_start_index(n, strength)
        assert k == n - run == EO.start_index(n, strength) and 0 <= k < n
        assert A.DDIMScheduler.edit_start_index(n, strength) == k == A.DPMSolverMultistepScheduler.edit_start_index(n, strength)
    assert edit_start_index(n, 1.0) == 0
    # the one point tied to the reference: its unfinished loop starts at shallow_reverse_step = N // 4 * 2 (4 | N)
    if n % 4 == 0:
        assert edit_start_index(n, 0.5) == n // 4 * 2
    for bad in (0.0, -0.1, 1.0001, float("nan")):
        with pytest.raises(ValueError, match="strength"):
            edit_start_index(n, bad)


@pytest.mark.parametrize("n", [10, 50])
def test_default_plan_is_todays_plan_and_key(n):
    d = A.DDIMScheduler()
    d.set_timesteps(n)
    for eta in (0.0, 0.3):
        p, p0 = d.sampler_plan(eta), d.sampler_plan(eta, start=0, masked=False)
        assert p.key == p0.key == ("DDIMScheduler", 1, "leading", 1000, 1, (0.0015, 0.0195, False), eta)
        assert torch.equal(p.table, d.coef_table() if eta == 0.0 else d.sampler_rows(eta).float()) and torch.equal(p.table, p0.table)
        assert p.legacy == (eta == 0.0) and p.keep is None and p.start == 0 and p.needs_noise == (eta != 0.0)
    m = A.DPMSolverMultistepScheduler()
    m.set_timesteps(n)
    p = m.sampler_plan()
    assert p.key == ("DPMSolverMultistepScheduler", 2, "leading", True, 1000, 1, (0.0015, 0.0195))
    assert torch.equal(p.table, m.sampler_rows().float()) and p.keep is None and p.start == 0 and p.needs_history and not p.legacy
    # the key tells every edit form apart
    keys = {d.sampler_plan(0.0).key, d.sampler_plan(0.0, start=3).key, d.sampler_plan(0.0, start=3, masked=True).key,
            d.sampler_plan(0.0, masked=True).key, d.sampler_plan(0.0, start=4).key}
    assert len(keys) == 5
    assert len({m.sampler_plan().key, m.sampler_plan(start=3).key, m.sampler_plan(start=3, masked=True).key, m.sampler_plan(masked=True).key}) == 4
    for s in (d, m):
        for bad in (-1, n):
            with pytest.raises(ValueError, match="start"):
                s.sampler_plan(start=bad)


@pytest.mark.parametrize("n,k", [(10, 3), (12, 6), (50, 49), (200, 100)])
def test_sliced_ddim_tables_are_rows_of_the_full_table(n, k):
    d = A.DDIMScheduler()
    d.set_timesteps(n)
    p = d.sampler_plan(0.0, start=k)
    assert p.legacy and p.start == k and p.keep is None and torch.equal(p.table, d.coef_table()[k:]) and p.table.is_contiguous()
    p = d.sampler_plan(0.3, start=k)
    assert not p.legacy and p.needs_noise and torch.equal(p.table, d.sampler_rows(0.3).float()[k:]) and p.table.shape == (n - k, 6)
    # NOT what sampler_rows(timesteps=...) of the truncated grid gives: that would take the ratio from the truncated length
    if n - k > 1 and 1000 // (n - k) != 1000 // n:
        assert not torch.equal(p.table, d.sampler_rows(0.3, timesteps=d.timesteps.tolist()[k:]).float())
    # masked: six columns whatever eta, plus keep
    pm = d.sampler_plan(0.0, start=k, masked=True)
    assert not pm.legacy and not pm.needs_noise and not pm.needs_history and pm.keep.shape == (n - k, 2)
    assert torch.equal(pm.table, d.sampler_rows(0.0).float()[k:])


@pytest.mark.parametrize("n,k", [(10, 3), (12, 6), (14, 13), (20, 5), (200, 100)])
def test_dpm_slice_first_row_is_first_order(n, k):
    m = A.DPMSolverMultistepScheduler()
    m.set_timesteps(n)
    full, rows = m.sampler_rows(), m.sampler_rows(start=k)
    assert rows.shape == (n - k, 6) and torch.equal(rows[1:], full[k + 1:])
    assert float(rows[0, 2]) == 0.0
    assert (float(full[k, 2]) == 0.0) == (k == n - 1 and n < 15)  # the slice really changes that row (but for a first-order last row)
    # first order from t to the next grid entry is deterministic DDIM's step there (test_dpm_first_order_is_ddim's identity)
    m1 = A.DPMSolverMultistepScheduler(solver_order=1)
    m1.set_timesteps(n)
    assert torch.equal(rows[0], m1.sampler_rows()[k])
    # lower_order_final keeps judging by the full N
    assert (float(rows[-1, 2]) == 0.0) == (n < 15 or n - k == 1)
    p = m.sampler_plan(start=k, masked=True)
    assert torch.equal(p.table, rows.float()) and p.needs_history and p.keep.shape == (n - k, 2) and p.start == k


@pytest.mark.parametrize("n,k", [(10, 0), (10, 3), (12, 6), (50, 49), (200, 100)])
def test_keep_table_and_add_noise_coefs_match_the_restatement(n, k):
    """the exported fp32 table against the fp64 restatement: relative 1e-6 (one fp32 rounding is 6e-8)"""
    acp, ts = SO.acp64(), SO.grid(n)
    one, zero = torch.ones(1, dtype=torch.float64), torch.zeros(1, dtype=torch.float64)
    for s in (A.DDIMScheduler(), A.DPMSolverMultistepScheduler()):
        s.set_timesteps(n)
        keep = s.sampler_plan(start=k, masked=True).keep
        assert keep.dtype == torch.float32 and keep.shape == (n - k, 2)
        for i in range(n - k):
            kx = float(EO.known(one, zero, i, k, ts, acp))  # coefficient of x0
            kz = float(EO.known(zero, one, i, k, ts, acp))  # coefficient of z0
            assert abs(float(keep[i, 0]) - kx) <= 1e-6 * kx and abs(float(keep[i, 1]) - kz) <= 1e-6 * max(kz, 1e-30), (i, keep[i], kx, kz)
        assert keep[-1].tolist() == [1.0, 0.0]
        a, sg = s.add_noise_coefs(k)
        assert abs(a - float(EO.add_noise(one, zero, ts[k], acp))) <= 1e-12 and abs(sg - float(EO.add_noise(zero, one, ts[k], acp))) <= 1e-12


def _table_loop(plan_rows, keep, x0, z0, mask, eps, a, s, noise=None):
    """what apad_edit_start + apad_cfg_edit_step compute, in float64, from the tables"""
    x = a * x0 + s * z0
    m1 = torch.zeros_like(x)
    for i, r in enumerate(plan_rows.tolist()):
        e = eps[i]
        z = torch.zeros_like(x) if noise is None else noise[i]
        m0 = r[4] * x + r[5] * e
        g = r[0] * x + r[1] * e + r[2] * m1 + r[3] * z
        kn = float(keep[i, 0]) * x0 + float(keep[i, 1]) * z0
        x = mask * g + (1.0 - mask) * kn
        m1 = m0
    return x


@pytest.mark.parametrize("strength", [0.5, 0.75, 1.0])
def test_masked_12_step_loop_through_the_tables_equals_the_oracle_loop(strength):
    n = 12
    acp = SO.acp64()
    g = torch.Generator().manual_seed(21)
    R = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    x0, z0 = R(4, 64), R(4, 64)
    mask = torch.rand(4, 64, generator=g, dtype=torch.float64)
    mask[0], mask[1] = 1.0, 0.0
    mask[2] = (mask[2] > 0.5).double()
    eps, noise = [R(4, 64) for _ in range(n)], [R(4, 64) for _ in range(n)]
    k = EO.start_index(n, strength)
    fn = lambda i, t, x: eps[i]
    # the keep table in float64, from the scheduler's own arithmetic, so that the loop comparison is not limited by fp32 table rounding
    for sampler, eta, sched in (("dpm", 0.0, A.DPMSolverMultistepScheduler()), ("ddim", 0.0, A.DDIMScheduler()), ("ddim", 0.3, A.DDIMScheduler())):
        sched.set_timesteps(n)
        assert sched.edit_start_index(n, strength) == k
        rows = sched.sampler_rows(start=k) if sampler == "dpm" else sched.sampler_rows(eta)[k:]
        ts = sched.timesteps.tolist()
        keep64 = torch.tensor([[float(sched.alphas_cumprod.double()[t]) ** 0.5, (1.0 - float(sched.alphas_cumprod.double()[t])) ** 0.5] for t in ts[k + 1:]]
                              + [[1.0, 0.0]], dtype=torch.float64)
        assert _rel(sched.keep_table(k).double(), keep64) <= 1e-7
        a, s = sched.add_noise_coefs(k)
        out = _table_loop(rows, keep64, x0, z0, mask, eps, a, s, noise if eta else None)
        ref = EO.edit_loop(x0, z0, mask, fn, n, strength, acp, sampler=sampler, eta=eta, noise=noise if eta else None)
        err = _rel(out, ref)
        print(f"\n[masked loop through the tables vs oracle, {sampler} eta={eta} strength={strength}] rel err {err:.3e}")
        assert err <= 1e-9
        assert torch.equal(out[1], x0[1])  # the kept clip ends as the source, exactly
        # ... and the strength-only loop (mask of ones) against the unmasked oracle
        ones = torch.ones_like(mask)
        assert _rel(_table_loop(rows, keep64, x0, z0, ones, eps, a, s, noise if eta else None),
                    EO.edit_loop(x0, z0, None, fn, n, strength, acp, sampler=sampler, eta=eta, noise=noise if eta else None)) <= 1e-9


# ---- the pipeline's argument checks (host side, before any device work) ----
@pytest.fixture(scope="module")
def pipe_kw():
    u = A.AudioLDM2UNet2DConditionModel(A.UNetConfig(block_out_channels=(64, 128, 192, 256), attention_head_dim=4, norm_num_groups=16))
    B = 2
    e, ge = torch.zeros(B, 16, 1024), torch.zeros(B, 8, 768)
    kw = dict(prompt_embeds=e, negative_prompt_embeds=e, generated_prompt_embeds=ge, negative_generated_prompt_embeds=ge,
              attention_mask=e[..., 0], negative_attention_mask=e[..., 0], audio_length_in_s=1.04, num_inference_steps=10, output_type="latent")
    return u, kw


def test_every_edit_argument_check_names_its_argument(pipe_kw):
    u, kw = pipe_kw
    vae = A.AutoencoderKL(A.VaeConfig(block_out_channels=(32, 64, 64), layers_per_block=1, norm_num_groups=8))
    pipe = A.AudioLDM2Pipeline(u, vae=vae)
    B, H, W = 2, 26, 16
    lat, mel = torch.zeros(B, 8, H, W), torch.zeros(B, 1, 104, 64)
    ones = torch.ones(1, 1, H, W)
    cases = [
        (dict(source_latents=lat, strength=0.0), "strength"),
        (dict(source_latents=lat, strength=1.5), "strength"),
        (dict(source_latents=lat, strength=-0.5), "strength"),
        (dict(source_latents=lat, strength=0.05), "strength"),        # int(10 * 0.05) == 0
        (dict(strength=0.5), "strength needs a source"),
        (dict(edit_mask=ones), "edit_mask needs a source"),
        (dict(edit_region=(0.0, 0.5)), "edit_region needs a source"),
        (dict(source_latents=lat, source_mel=mel), "source_mel and source_latents"),
        (dict(source_audio="clip.wav", source_mel=mel), "source_audio and source_mel"),
        (dict(source_latents=lat, latents=lat), "latents="),
        (dict(source_latents=lat, edit_mask=torch.ones(H + 1, W)), "edit_mask .* not broadcastable"),
        (dict(source_latents=lat, edit_mask=torch.ones(3, 1, H, W)), "edit_mask .* not broadcastable"),
        (dict(source_latents=lat, edit_mask=torch.ones(B, 8, H, W)), "edit_mask .* not broadcastable"),
        (dict(source_latents=lat, edit_mask=ones * 1.5), r"edit_mask values must lie in \[0, 1\]"),
        (dict(source_latents=lat, edit_mask=ones * -0.1), r"edit_mask values must lie in \[0, 1\]"),
        (dict(source_latents=lat, edit_mask=ones * float("nan")), r"edit_mask values must lie in \[0, 1\]"),
        (dict(source_latents=torch.zeros(B, 8, H + 1, W)), "source_latents has 27 rows"),
        (dict(source_mel=torch.zeros(B, 1, 100, 64)), "source_mel has 100 frames"),
        (dict(source_latents=lat, edit_mask=ones, edit_region=(0.0, 0.5)), "edit_mask and edit_region"),
        (dict(source_latents=lat, edit_region=(0.5, 0.5)), "edit_region"),
        (dict(source_latents=lat, edit_region=(0.0, 2.0)), "edit_region"),   # the clip is 1.04 s
        (dict(source_latents=torch.zeros(3, 8, H, W)), "source_latents holds 3 clips"),
    ]
    for extra, match in cases:
        with pytest.raises(ValueError, match=match):
            pipe(**{**kw, **extra})
    # a source that has to be encoded needs the VAE; source_latents does not
    bare = A.AudioLDM2Pipeline(u)
    for extra in (dict(source_mel=mel), dict(source_audio="clip.wav")):
        with pytest.raises(ValueError, match="vae="):
            bare(**{**kw, **extra})
    k, m = bare.check_edit_arguments(B, 104, 10, 1.04, None, None, None, lat, 0.5, None, (0.2, 0.6))
    assert k == 5 and m.shape == (1, 1, H, W) and m.dtype == torch.float32
    assert torch.equal(m[0, 0, :, 0], torch.tensor([0.0] * 5 + [1.0] * 10 + [0.0] * 11))  # one latent row = 0.04 s
    k, m = bare.check_edit_arguments(B, 104, 10, 1.04, None, None, None, lat, 1.0, torch.rand(B, 1, H, W), None)
    assert k == 0 and m.shape == (B, 1, H, W)
    # no edit argument: nothing to check, nothing returned
    assert bare.check_edit_arguments(B, 104, 10, 1.04, lat, None, None, None, 1.0, None, None) == (0, None)


def test_a_three_dim_mask_is_per_row_not_per_clip(pipe_kw):
    """[H, W] and [1, H, W] are shared masks; a per-clip mask is [B, 1, H, W] (torch broadcasting against [B, 1, H, W])"""
    u, _ = pipe_kw
    pipe = A.AudioLDM2Pipeline(u)
    lat = torch.zeros(2, 8, 26, 16)
    for shape, mb in (((26, 16), 1), ((1, 26, 16), 1), ((1, 1, 26, 16), 1), ((2, 1, 26, 16), 2), ((26, 1), 1), ((2, 1, 1, 1), 2)):
        _, m = pipe.check_edit_arguments(2, 104, 10, 1.04, None, None, None, lat, 1.0, torch.ones(shape), None)
        assert m.shape == (mb, 1, 26, 16) and m.is_contiguous(), shape


def test_abi_declares_the_edit_entry_points():
    header = open(os.path.join(ROOT, "include", "apadapter_hip.h")).read()
    assert re.search(r"#define APAD_ABI_VERSION 12\b", header)  # additive: the version line stays
    index = header.split("#ifndef APADAPTER_HIP_H")[0]
    for name, nargs in (("apad_cfg_edit_step", 20), ("apad_edit_start", 13)):
        assert re.search(r"\bint %s\s*\(" % name, header) and name in index
        assert name in L.SYMBOLS and len(L.SYMBOLS[name][1]) == nargs
        decl = re.search(r"\bint %s\s*\(([^)]*)\)" % name, header).group(1)
        assert len(decl.split(",")) == nargs
    assert len(L.SYMBOLS["apad_cfg_sampler_step"][1]) == 14 and len(L.SYMBOLS["apad_cfg_ddim_step"][1]) == 11  # untouched
    if os.path.exists(L.LIB_PATH):
        assert A.lib().apad_abi_version() == 12
        assert hasattr(A.lib(), "apad_cfg_edit_step") and hasattr(A.lib(), "apad_edit_start")
