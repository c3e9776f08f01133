"""CPU: edit-friendly DDPM inversion as host arithmetic -- ``inversion_plan``'s rows and keep table against the independent fp64
restatement (tests/invert_oracle.py), the restatement's own round trip, every argument check, and the public surface.  No GPU compute.
PARITY UNPINNED (see invert_oracle)."""
import os
import re

import pytest
import torch

import ap_adapter_amd as A
from ap_adapter_amd import _lib as L

import invert_oracle as IO
import sampler_oracle as SO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("dual", [False, True])
@pytest.mark.parametrize("n", [4, 10, 200])
def test_inversion_plan_rows_and_keep_table_match_the_restatement(n, dual):
    """the exported fp32 tables against float64 closed forms: relative 1e-6 (one fp32 rounding is 6e-8; c_e is a difference of two O(1) terms,
    so its bound is absolute, 1e-6 of the larger term)"""
    acp, ts = SO.acp64(), SO.grid(n)
    d = A.DDIMScheduler()
    d.set_timesteps(n)
    for k in (0, n // 2):
        for eta in (1.0, 0.5):
            p = d.inversion_plan(eta, start=k, dual=dual)
            assert p.table.dtype == p.keep.dtype == torch.float32 and p.table.shape == (n - k, 6) and p.keep.shape == (n - k, 2)
            assert p.needs_noise and not p.needs_history and not p.legacy and p.start == k and p.table.is_contiguous()
            assert "invert" in p.key and ("dual" in p.key) == dual
            assert torch.equal(p.table, d.sampler_rows(eta)[k:].float()) and torch.equal(p.keep, d.keep_table(k))
            for i in range(n - k):
                c_x, c_e, std = IO.row(i, k, ts, acp, eta)
                r = p.table[i].tolist()
                assert abs(r[0] - c_x) <= 1e-6 * c_x and abs(r[1] - c_e) <= 1e-6 * c_x and abs(r[3] - std) <= 1e-6 * std and std > 0, (i, r)
                assert r[2] == r[4] == r[5] == 0.0
                kx, kz = IO.level(i, k, ts, acp)
                assert abs(float(p.keep[i, 0]) - kx) <= 1e-6 * kx and abs(float(p.keep[i, 1]) - kz) <= 1e-6 * max(kz, 1e-30)
            assert p.keep[-1].tolist() == [1.0, 0.0]
    # the key tells the inversion from every sampler plan, and one grid from another
    keys = {d.inversion_plan(1.0).key, d.inversion_plan(0.5).key, d.inversion_plan(1.0, start=1).key, d.inversion_plan(1.0, dual=True).key,
            d.sampler_plan(1.0).key, d.sampler_plan(1.0, start=1).key, d.sampler_plan(1.0, start=1, masked=True).key}
    assert len(keys) == 7


@pytest.mark.parametrize("n,k", [(4, 0), (6, 3), (10, 5), (50, 0), (200, 100)])
def test_the_restatement_round_trips_to_x0(n, k):
    """invert under one eps function, regenerate under the same: every x_(i+1) is retraced and the run ends on x0, to 1e-12 in float64 --
    for any eps function (here a smooth nonlinear one of x and t)"""
    acp = SO.acp64()
    g = torch.Generator().manual_seed(31)
    R = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    x0, z0 = R(3, 40) * 0.7, R(3, 40)
    draws = [R(3, 40) for _ in range(n - k)]
    fn = lambda i, t, x: torch.tanh(0.8 * x + 0.3) * (0.5 + t / 1000.0) + 0.1 * torch.sin(3.0 * x)
    xs, zs = IO.invert_chain(x0, z0, draws, fn, n, k, acp, 1.0)
    assert torch.equal(xs[-1], x0.double())
    ys = IO.regenerate_chain(xs[0], zs, fn, n, k, acp, 1.0)
    for a, b in zip(xs, ys):
        assert float((a - b).abs().max()) <= 1e-12 * float(a.abs().max())
    assert float((ys[-1] - x0).abs().max()) <= 1e-12 * float(x0.abs().max())
    # another condition (another eps function) does not retrace it
    other = IO.regenerate_chain(xs[0], zs, lambda i, t, x: 0.5 * fn(i, t, x), n, k, acp, 1.0)
    assert float((other[-1] - x0).abs().max()) > 1e-3


def test_inversion_plan_value_errors():
    d = A.DDIMScheduler()
    d.set_timesteps(10)
    for bad in (0.0, -0.5):
        with pytest.raises(ValueError, match="eta"):
            d.inversion_plan(bad)
    for bad in (-1, 10):
        with pytest.raises(ValueError, match="start"):
            d.inversion_plan(1.0, start=bad)
    m = A.DPMSolverMultistepScheduler()
    m.set_timesteps(10)
    with pytest.raises(ValueError, match="DPMSolverMultistepScheduler"):
        m.inversion_plan(1.0)


@pytest.fixture(scope="module")
def pipe_kw():
    u = A.AudioLDM2UNet2DConditionModel(A.UNetConfig(block_out_channels=(64, 128, 192, 256), attention_head_dim=4, norm_num_groups=16))
    B = 2
    e, ge = torch.zeros(B, 16, 1024), torch.zeros(B, 8, 768)
    kw = dict(prompt_embeds=e, negative_prompt_embeds=e, generated_prompt_embeds=ge, negative_generated_prompt_embeds=ge,
              attention_mask=e[..., 0], negative_attention_mask=e[..., 0], audio_length_in_s=1.04, num_inference_steps=10, output_type="latent")
    skw = dict(source_prompt_embeds=e, source_generated_prompt_embeds=ge, source_attention_mask=e[..., 0])
    return u, kw, skw


def test_every_inversion_argument_check_names_its_argument(pipe_kw):
    """each raises on the host, before any device work (the UNet lives on the CPU here: device work would fail otherwise)"""
    u, kw, skw = pipe_kw
    B, H, W = 2, 26, 16
    lat = torch.zeros(B, 8, H, W)
    pipe = A.AudioLDM2Pipeline(u)
    inv = dict(inversion="ddpm", source_latents=lat, eta=1.0, **skw)
    cases = [
        (dict(inversion="ddpm", eta=1.0, **skw), "needs a source clip"),
        ({**inv, "eta": 0.0}, r"eta=0\.0.*pass eta=1\.0"),
        (dict(inversion="ddpm", source_latents=lat, **skw), r"eta=0\.0.*pass eta=1\.0"),  # the call's default eta
        ({**inv, "inversion": "ddim"}, "inversion='ddim'"),
        ({**inv, "source_prompt": "a piano"}, "source_prompt needs text prompts"),
        ({k: v for k, v in inv.items() if k != "source_attention_mask"}, "source_attention_mask is required"),
        ({k: v for k, v in inv.items() if k != "source_prompt_embeds"}, "source_prompt_embeds is required"),
        ({**inv, "source_generated_prompt_embeds": torch.zeros(3, 8, 768)}, "source_generated_prompt_embeds holds 3 rows"),
        ({**inv, "source_guidance_scale": 1.0}, "source_guidance_scale"),
        ({**inv, "source_guidance_scale": -1.0, "audio_guidance_scale": 2.0, "mel": torch.zeros(1, 1024, 128)}, "text"),
        (dict(source_latents=lat, eta=1.0, **skw), "source_prompt_embeds is the source condition of inversion='ddpm'"),
        (dict(source_prompt="a piano"), "source_prompt is the source condition of inversion='ddpm'"),
    ]
    for extra, match in cases:
        with pytest.raises(ValueError, match=match):
            pipe(**{**kw, **extra})
    dpm = A.AudioLDM2Pipeline(u, scheduler=A.DPMSolverMultistepScheduler())
    with pytest.raises(ValueError, match="DDIM scheduler.*DPMSolverMultistepScheduler"):
        dpm(**{**kw, **inv})
    for p in (pipe, dpm):  # invert itself: eta and the scheduler, before any device work
        with pytest.raises(ValueError, match="eta" if p is pipe else "DPMSolverMultistepScheduler"):
            p.invert((lat, lat, None), None, None, None, 10, 3.0, eta=0.0 if p is pipe else 1.0)


def test_a_mismatched_inverted_source_is_refused(pipe_kw):
    u, kw, _ = pipe_kw
    B, C, H, W, N, k = 2, 8, 26, 16, 10, 5
    pipe = A.AudioLDM2Pipeline(u)
    pipe.scheduler.set_timesteps(N)
    lat = torch.zeros(B, C, H, W)
    ge, pe, am = torch.zeros(2 * B, 8, 768), torch.zeros(2 * B, 16, 1024), torch.ones(2 * B, 16)
    good = dict(z0=lat, x0=lat, z=torch.zeros(N - k, B, H * W, C), start=k, num_inference_steps=N, eta=1.0,
                scheduler_key=pipe.scheduler.inversion_plan(1.0, start=k).key)
    assert issubclass(A.InvertedSource, A.EditSource)
    run = lambda p, src, n=N, start=k, eta=1.0: p.denoise(None, ge, pe, am, n, 3.0, source=src, start=start, eta=eta)
    for field, value, call in (("num_inference_steps", 12, {}), ("start", 4, {}), ("eta", 0.5, {}), ("eta", 1.0, dict(eta=0.0)),
                               ("scheduler_key", ("other",), {}), ("z", torch.zeros(N - k, B, H * W, 4), {}), ("z", None, {})):
        with pytest.raises(ValueError, match=rf"InvertedSource\.{field}"):
            run(pipe, A.InvertedSource(**{**good, field: value}), **call)
    with pytest.raises(ValueError, match=r"InvertedSource\.scheduler_key.*DPMSolverMultistepScheduler"):
        run(A.AudioLDM2Pipeline(u, scheduler=A.DPMSolverMultistepScheduler()), A.InvertedSource(**good))
    # another beta schedule is another grid
    with pytest.raises(ValueError, match=r"InvertedSource\.scheduler_key"):
        run(A.AudioLDM2Pipeline(u, scheduler=A.DDIMScheduler(beta_end=0.02)), A.InvertedSource(**good))


def test_abi_declares_the_invert_entry_point():
    header = open(os.path.join(ROOT, "include", "apadapter_hip.h")).read()
    assert re.search(r"#define APAD_ABI_VERSION 12\b", header)  # additive: the version line stays
    index = header.split("#ifndef APADAPTER_HIP_H")[0]
    name, nargs = "apad_cfg_invert_step", 17
    assert re.search(r"\bint %s\s*\(" % name, header) and name in index
    assert name in L.SYMBOLS and len(L.SYMBOLS[name][1]) == nargs
    decl = re.search(r"\bint %s\s*\(([^)]*)\)" % name, header).group(1)
    assert len(decl.split(",")) == nargs
    assert len(L.SYMBOLS["apad_cfg_sampler_step"][1]) == 14 and len(L.SYMBOLS["apad_cfg_dual_step"][1]) == 20  # untouched
    if os.path.exists(L.LIB_PATH):
        assert A.lib().apad_abi_version() == 12 and hasattr(A.lib(), "apad_cfg_invert_step")
    import inspect
    sig = inspect.signature(A.AudioLDM2Pipeline.__call__).parameters
    assert [sig[n].default for n in ("inversion", "source_prompt", "source_guidance_scale")] == [None, None, 3.0]
    assert list(sig)[-6:] == ["inversion", "source_prompt", "source_guidance_scale", "source_prompt_embeds", "source_generated_prompt_embeds",
                              "source_attention_mask"]
    assert hasattr(A.AudioLDM2Pipeline, "invert") and callable(getattr(__import__("ap_adapter_amd.ops", fromlist=["x"]), "cfg_invert_step"))
