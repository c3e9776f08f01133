"""-m gpu: editing from a source clip -- apad_cfg_edit_step and apad_edit_start against the fp64 restatement (tests/edit_oracle.py), their
exactness properties (mask = 1 -> the bits of apad_cfg_sampler_step, mask = 0 -> the bits of the noised source, the last step -> the
bits of the source), and the pipeline: strength-only runs against hand-driven loops over the existing update kernels, masked runs
captured / eager / replayed, the untouched default path, bad operands, and the way in through the VAE encoder and a wav file.
PARITY UNPINNED (see edit_oracle)."""
import wave

import numpy as np
import pytest
import torch

from util import TOL, q, rel_err

import edit_oracle as EO
import sampler_oracle as SO
from test_gpu_samplers import _check_step, _count, _inputs
from test_gpu_unet import _small_unet

pytestmark = pytest.mark.gpu


def R(*shape, seed=0, std=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * std


def _mask(kind, B, npix, seed=3):
    """fp32 [1 or B, npix]: binary / fractional values, one per clip / shared by the batch"""
    g = torch.Generator().manual_seed(seed)
    m = torch.rand(B if "clip" in kind else 1, npix, generator=g)
    return (m > 0.5).float() if "binary" in kind else m


def _full(mask, B, C):
    """the mask per element of [B, n] (NHWC: element j of a clip belongs to pixel j // C)"""
    return mask.repeat_interleave(C, dim=1).expand(B, mask.shape[1] * C)


def _fma32(a, x, p):
    """fp32(a * x + p) -- one fused multiply-add -- for a Python float ``a`` holding an fp32 value and fp32 tensors x, p, on the host:
    the product is exact in float64; where the float64 sum was inexact AND sits exactly half way between two fp32 values, it is nudged
    towards the exact sum first, so that the second rounding cannot fall the wrong way"""
    prod = a * x.double()
    p = p.double()
    s = prod + p
    bb = s - prod
    err = (prod - (s - bb)) + (p - bb)  # TwoSum: prod + p = s + err exactly
    tie = (s.view(torch.int64) & 0x1FFFFFFF) == 0x10000000
    inf = torch.full_like(s, float("inf"))
    s = torch.where(tie & (err != 0), torch.nextafter(s, torch.where(err > 0, inf, -inf)), s)
    return s.float()


def _plan(sampler, eta, n, k, masked=True):
    import ap_adapter_amd as A
    s = A.DPMSolverMultistepScheduler() if sampler == "dpm" else A.DDIMScheduler()
    s.set_timesteps(n)
    return s, s.sampler_plan(eta, start=k, masked=masked)


GEOMS = [(4000, 8), (4001, 8), (4001, 4)]  # (pixels per clip, C): 16-byte form (B * n % 8 == 0, C == 8) twice, the scalar form (C == 4)


@pytest.mark.parametrize("kind", ["binary-clip", "fractional-clip", "binary-shared", "fractional-shared"])
@pytest.mark.parametrize("npix,C", GEOMS)
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32])
@pytest.mark.parametrize("sampler,eta", [("dpm", 0.0), ("ddim", 0.0), ("ddim", 0.5)])
def test_cfg_edit_step_matches_oracle(dev, sampler, eta, dtype, npix, C, kind):
    """every step of a 10-step edit loop -- the last 10 of a 14-step grid (strength 0.75: int(10.5) = 10, start index 4), so the slice,
    the multistep solver's first-order entry and its first-order last step (lower_order_final judged by N = 14) are all on the path --
    on random eps2.  Bounds: test_gpu_samplers._check_step's (eps 1e-6, latents 1e-5, unet_in TOL[dtype]) and 1e-5 for m0."""
    from ap_adapter_amd import ops
    B, N, strength, gs = 3, 14, 0.75, 7.5
    n = npix * C
    k = EO.start_index(N, strength)
    steps = N - k
    assert (k, steps) == (4, 10)
    sched, plan = _plan(sampler, eta, N, k)
    assert not plan.legacy and plan.table.shape == (steps, 6) and plan.keep.shape == (steps, 2)
    coef, keep = plan.table.to(dev), plan.keep.to(dev)
    acp, ts = SO.acp64(), SO.grid(N)
    x0, z0 = R(B, n, seed=60), R(B, n, seed=61)
    mask = _mask(kind, B, npix)
    mfull = _full(mask, B, C)
    noise = R(steps, B, n, seed=9) if eta else None
    lat = EO.add_noise(x0, z0, ts[k], acp)
    lat_d = lat.float().to(dev)
    x0_d, z0_d, mask_d = x0.to(dev), z0.to(dev), mask.to(dev)
    noise_d = None if noise is None else noise.to(dev)
    unet_in = torch.empty(B, n, dtype=dtype, device=dev)
    eps_out = torch.empty(B, n, dtype=torch.float32, device=dev)
    hist = torch.zeros(B, n, dtype=torch.float32, device=dev) if plan.needs_history else None
    step_ptr = torch.zeros(1, dtype=torch.int32, device=dev)
    m1, worst = None, [0.0, 0.0, 0.0, 0.0]
    for i in range(steps):
        eps2 = q(R(2 * B, n, seed=100 + i) * 0.5, dtype)
        e = SO.cfg_combine_rounded(eps2, gs, dtype)
        if sampler == "dpm":
            g, m1 = EO.dpm_edit_step(lat, e, m1, i, k, ts, acp)
        else:
            g = EO.ddim_edit_step(lat, e, None if noise is None else noise[i], i, k, ts, acp, eta)
        lat = EO.blend(g, mfull, x0, z0, i, k, ts, acp)
        ops.cfg_edit_step(eps2.to(dev, dtype), lat_d, unet_in, coef, keep, step_ptr, gs, x0_d, z0_d, mask_d, C, eps_out, hist, noise_d)
        ops.step_advance(step_ptr)
        errs = _check_step(dtype, lat_d, unet_in, eps_out, lat, e)
        if hist is not None:
            errs += (rel_err(hist, m1.float()),)
            assert errs[3] < 1e-5, errs
        worst = [max(a, b) for a, b in zip(worst, errs + (0.0,))]
    print(f"\n[apad_cfg_edit_step {sampler} eta={eta}, {dtype}, npix={npix} C={C}, {kind}] worst rel err: eps {worst[0]:.2e} latents {worst[1]:.2e} "
          f"unet_in {worst[2]:.2e} m0 {worst[3]:.2e}")
    assert int(step_ptr.item()) == steps
    if "binary" in kind:  # after the final step the kept pixels are the source latents, bit for bit; the others are not
        kept = mfull.to(dev) == 0
        assert torch.equal(lat_d[kept], x0_d[kept]) and not bool((lat_d[~kept] == x0_d[~kept]).all())
        assert bool(kept.any()) and bool((~kept).any())


@pytest.mark.parametrize("npix,C", GEOMS)
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32])
@pytest.mark.parametrize("sampler,eta", [("dpm", 0.0), ("ddim", 0.5)])
def test_mask_of_ones_is_cfg_sampler_step_bit_for_bit(dev, sampler, eta, dtype, npix, C):
    """mask = 1: fma(1, g, 0 * known) is g -- latents, unet_in, eps_out and history carry the bits apad_cfg_sampler_step writes from the
    same inputs, at every step of the slice; and so does a null mask"""
    from ap_adapter_amd import ops
    B, N, k, gs = 3, 14, 4, 7.5
    n = npix * C
    sched, plan = _plan(sampler, eta, N, k)
    coef, keep = plan.table.to(dev), plan.keep.to(dev)
    x0, z0 = R(B, n, seed=60).to(dev), R(B, n, seed=61).to(dev)
    noise = R(N - k, B, n, seed=9).to(dev) if eta else None
    ones = torch.ones(B, npix, device=dev)
    start = R(B, n, seed=44).to(dev)

    def state():
        return dict(lat=start.clone(), unet_in=torch.empty(B, n, dtype=dtype, device=dev), eps_out=torch.empty(B, n, device=dev),
                    hist=torch.zeros(B, n, device=dev) if plan.needs_history else None, ptr=torch.zeros(1, dtype=torch.int32, device=dev))

    a, b, c = state(), state(), state()
    for i in range(N - k):
        eps2 = q(R(2 * B, n, seed=100 + i) * 0.5, dtype).to(dev, dtype)
        ops.cfg_sampler_step(eps2, a["lat"], a["unet_in"], coef, a["ptr"], gs, a["eps_out"], a["hist"], noise)
        ops.cfg_edit_step(eps2, b["lat"], b["unet_in"], coef, keep, b["ptr"], gs, x0, z0, ones, C, b["eps_out"], b["hist"], noise)
        ops.cfg_edit_step(eps2, c["lat"], c["unet_in"], coef, None, c["ptr"], gs, None, None, None, C, c["eps_out"], c["hist"], noise)
        for s in (a, b, c):
            ops.step_advance(s["ptr"])
        for name in ("lat", "unet_in", "eps_out", "hist"):
            if a[name] is not None:
                assert torch.equal(a[name], b[name]) and torch.equal(a[name], c[name]), (i, name)


@pytest.mark.parametrize("npix,C", GEOMS)
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_mask_of_zeros_is_the_fp32_known_bit_for_bit(dev, dtype, npix, C):
    """mask = 0: fma(0, g, 1 * known) is known = fma(kx, x0, kz * z0) -- restated on the host (_fma32): p = fp32(kz z0),
    known = fp32(kx x0 + p); on the last step known is x0 itself"""
    from ap_adapter_amd import ops
    B, N, k, gs = 2, 10, 5, 7.5
    n = npix * C
    sched, plan = _plan("dpm", 0.0, N, k)
    coef, keep = plan.table.to(dev), plan.keep.to(dev)
    x0, z0 = R(B, n, seed=60), R(B, n, seed=61)
    x0_d, z0_d = x0.to(dev), z0.to(dev)
    zeros = torch.zeros(1, npix, device=dev)
    lat = R(B, n, seed=44).to(dev)
    unet_in = torch.empty(B, n, dtype=dtype, device=dev)
    hist = torch.zeros(B, n, device=dev)
    ptr = torch.zeros(1, dtype=torch.int32, device=dev)
    for i in range(N - k):
        eps2 = q(R(2 * B, n, seed=100 + i) * 0.5, dtype).to(dev, dtype)
        ops.cfg_edit_step(eps2, lat, unet_in, coef, keep, ptr, gs, x0_d, z0_d, zeros, C, None, hist)
        ops.step_advance(ptr)
        kx, kz = float(plan.keep[i, 0]), float(plan.keep[i, 1])
        known = _fma32(kx, x0, (kz * z0.double()).float())
        assert torch.equal(lat.cpu(), known), i
        assert torch.equal(unet_in.cpu(), known.to(dtype)), i
    assert torch.equal(lat, x0_d)
    assert bool(hist.abs().max() > 0)  # the history is still the pre-blend data prediction


@pytest.mark.parametrize("Lc", [8, 4])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32])
def test_edit_start_matches_fp64(dev, dtype, Lc):
    """x0 = (mean + exp(0.5 clamp(logvar)) post_noise) * scale and latents = a x0 + s z0 against float64: relative 1e-6 (fp32 arithmetic on
    O(1) operands); unet_in is the model-dtype copy.  Lc = 8 takes the 16-byte form, Lc = 4 the scalar one.  Against ops.gaussian_sample
    on the same (model-dtype) noise: that op returns the draw ROUNDED TO THE MODEL DTYPE, edit_start keeps it in fp32, so the two agree to
    one rounding of the model dtype -- half a unit in its last place, finfo(dtype).eps / 2 relative, per element -- plus one fp32 unit
    (2^-23) for the compiler's freedom to fuse the multiply-adds of the two kernels differently."""
    from ap_adapter_amd import ops
    rows, scale, a, s = 4000, 0.4110932946205139, 0.7310585786300049, 0.6823145491893791
    m = q(R(rows, 2 * Lc, seed=5) * 2, dtype)
    m[0, Lc:] = 50.0   # clamped to 20
    m[1, Lc:] = -50.0  # clamped to -30
    pn = q(R(rows, Lc, seed=6), dtype)  # exactly representable in the model dtype, so that gaussian_sample reads the same noise
    z0 = R(rows, Lc, seed=7)
    x0_ref = (m[:, :Lc].double() + torch.exp(0.5 * m[:, Lc:].double().clamp(-30, 20)) * pn.double()) * scale
    f32 = lambda v: float(torch.tensor(v, dtype=torch.float32))
    lat_ref = a * x0_ref + s * z0.double()
    x0 = torch.full((rows, Lc), float("nan"), device=dev)
    lat = torch.full((rows, Lc), float("nan"), device=dev)
    unet_in = torch.empty(rows, Lc, dtype=dtype, device=dev)
    ops.edit_start(z0.to(dev), x0, lat, unet_in, a, s, moments=m.to(dev, dtype), post_noise=pn.to(dev), scale=scale)
    # exclude the clamped-to-20 row from the max-normalised error (exp(10) = 22026 would hide everything else) and check it on its own
    errs = rel_err(x0[1:], x0_ref[1:].float()), rel_err(lat[1:], lat_ref[1:].float()), rel_err(x0[:1], x0_ref[:1].float()), rel_err(lat[:1], lat_ref[:1].float())
    print(f"\n[apad_edit_start moments, {dtype}, Lc={Lc}] rel err x0 {errs[0]:.2e} latents {errs[1]:.2e}; the logvar = 20 row: x0 {errs[2]:.2e} latents {errs[3]:.2e}")
    assert max(errs) < 1e-6, errs
    assert rel_err(unet_in, lat_ref.float()) < TOL[dtype] and torch.equal(unet_in, lat.to(dtype))
    gs_out = ops.gaussian_sample(m.to(dev, dtype), pn.to(dev, dtype), scale).float()
    bound = (torch.finfo(dtype).eps / 2 + 2.0 ** -23) * gs_out.abs() + torch.finfo(dtype).tiny * torch.finfo(dtype).eps  # (+ the smallest subnormal)
    assert bool(((x0 - gs_out).abs() <= bound).all())
    # the source_latents path: null moments, x0 is read, not written
    src = R(rows, Lc, seed=8).to(dev)
    x0b = src.clone()
    ops.edit_start(z0.to(dev), x0b, lat, unet_in, a, s)
    ref = a * src.double().cpu() + s * z0.double()
    assert torch.equal(x0b, src) and rel_err(lat, ref.float()) < 1e-6 and torch.equal(unet_in, lat.to(dtype))
    # ... and it is the fused multiply-add the step kernel's `known` uses
    assert torch.equal(lat.cpu(), _fma32(f32(a), src.cpu(), (f32(s) * z0.double()).float()))


def test_bad_operands_raise_from_the_status_code(dev):
    from ap_adapter_amd import _lib as L
    from ap_adapter_amd import ops
    B, npix, C = 2, 8, 8
    n = npix * C
    lat = torch.zeros(B, n, device=dev)
    eps2 = torch.zeros(2 * B, n, dtype=torch.bfloat16, device=dev)
    unet_in = torch.zeros(B, n, dtype=torch.bfloat16, device=dev)
    ptr = torch.zeros(1, dtype=torch.int32, device=dev)
    coef, keep = torch.zeros(5, 6, device=dev), torch.zeros(5, 2, device=dev)
    x0, z0, mask = torch.zeros(B, n, device=dev), torch.zeros(B, n, device=dev), torch.ones(B, npix, device=dev)
    with pytest.raises(RuntimeError, match=r"\[steps, 6\]"):
        ops.cfg_edit_step(eps2, lat, unet_in, torch.zeros(5, 2, device=dev), keep, ptr, 7.5, x0, z0, mask, C)
    with pytest.raises(RuntimeError, match=r"rc=-?\d+.*mask_batch 3 must be 1 or B = 2"):
        ops.cfg_edit_step(eps2, lat, unet_in, coef, keep, ptr, 7.5, x0, z0, torch.ones(3, npix, device=dev), C)
    with pytest.raises(RuntimeError, match=r"rc=-?\d+.*not a multiple of C = 7"):
        ops.cfg_edit_step(eps2, lat, unet_in, coef, keep, ptr, 7.5, x0, z0, mask, 7)
    with pytest.raises(RuntimeError, match=r"rc=-?\d+.*a mask needs the keep table, x0 and z0"):
        ops.cfg_edit_step(eps2, lat, unet_in, coef, keep, ptr, 7.5, None, z0, mask, C)
    with pytest.raises(RuntimeError, match="keep"):
        ops.cfg_edit_step(eps2, lat, unet_in, coef, torch.zeros(4, 2, device=dev), ptr, 7.5, x0, z0, mask, C)
    with pytest.raises(RuntimeError, match="mask"):
        ops.cfg_edit_step(eps2, lat, unet_in, coef, keep, ptr, 7.5, x0, z0, torch.ones(B, npix + 1, device=dev), C)
    # the entry point itself: a status code and a message, never an abort
    lib = L.lib()
    rc = lib.apad_cfg_edit_step(eps2.data_ptr(), lat.data_ptr(), unet_in.data_ptr(), None, None, None, coef.data_ptr(), keep.data_ptr(), None, None,
                                mask.data_ptr(), B, C, ptr.data_ptr(), 5, 7.5, B, n, L.BF16, None)
    assert rc != 0 and b"null operand" in lib.apad_last_error()
    rc = lib.apad_edit_start(x0.data_ptr(), None, z0.data_ptr(), x0.data_ptr(), lat.data_ptr(), unet_in.data_ptr(), 1.0, 0.0, 1.0, B * npix, C, L.BF16, None)
    assert rc != 0 and b"post_noise" in lib.apad_last_error()
    with pytest.raises(RuntimeError, match="moments"):
        ops.edit_start(z0, x0, lat, unet_in, 1.0, 0.0, moments=torch.zeros(B * npix, 2 * C, device=dev), post_noise=z0)  # fp32 moments, bf16 unet_in
    # a step counter beyond the tables reads their last rows, not past them
    ptr.fill_(1000)
    coef[4, 0], keep[4, 0] = 2.0, 1.0
    lat.fill_(1.5)
    x0.fill_(0.25)
    half = torch.full((1, npix), 0.5, device=dev)
    ops.cfg_edit_step(eps2, lat, unet_in, coef, keep, ptr, 7.5, x0, z0, half, C)
    assert bool((lat == 0.5 * 3.0 + 0.5 * 0.25).all())
    torch.cuda.synchronize()


# ---- the pipeline on the small synthetic UNet ----
def _source(dev, B, H=26, W=16, seed=70):
    """fp32 (x0, z0) [B, 8, H, W] on the device"""
    return R(B, 8, H, W, seed=seed, std=0.7).to(dev), R(B, 8, H, W, seed=seed + 1).to(dev)


def _nhwc(t):
    B, C, H, W = t.shape
    return t.float().permute(0, 2, 3, 1).reshape(B, H * W, C).contiguous()


@pytest.mark.parametrize("sampler", ["ddim", "dpm"])
def test_strength_only_is_a_hand_driven_loop_over_the_existing_step(dev, monkeypatch, sampler):
    """strength 0.5 at 12 steps: the start index is 6 (the reference's N // 4 * 2), the UNet is evaluated 6 times, neither update kernel
    of the full run is replaced -- deterministic DDIM stays on apad_cfg_ddim_step, DPM-Solver++ on apad_cfg_sampler_step -- and the latents
    are the bits of a loop driven by hand over that op from x_start, on the sliced table and the sliced time tables"""
    import ap_adapter_amd as A
    from ap_adapter_amd import ops
    dtype = torch.bfloat16
    u, cfg, sd, procs = _small_unet(dev, dtype)
    u.requires_grad_(False)
    B, H, W, N, gs = 2, 26, 16, 12, 7.5
    _, ehs, ehs1, m1 = _inputs(dev, dtype)
    x0, z0 = _source(dev, B)
    mk = (lambda: A.DPMSolverMultistepScheduler()) if sampler == "dpm" else (lambda: A.DDIMScheduler())
    pipe = A.AudioLDM2Pipeline(u, scheduler=mk())
    k = pipe.scheduler.edit_start_index(N, 0.5)
    assert k == 6 == N // 4 * 2
    calls = _count(monkeypatch, ("cfg_ddim_step", "cfg_sampler_step", "cfg_edit_step", "edit_start"))
    seen = []
    eager = pipe.denoise(None, ehs, ehs1, m1, N, gs, use_graph=False, source=(x0, z0, None), start=k, callback=lambda i, t, x: seen.append((i, t)))
    used, other = ("cfg_sampler_step", "cfg_ddim_step") if sampler == "dpm" else ("cfg_ddim_step", "cfg_sampler_step")
    assert (len(calls[used]), len(calls[other]), len(calls["cfg_edit_step"]), len(calls["edit_start"])) == (N - k, 0, 0, 1)
    assert seen == [(i, SO.grid(N)[k + i]) for i in range(N - k)]
    graph = pipe.denoise(None, ehs, ehs1, m1, N, gs, source=(x0, z0, None), start=k)
    again = pipe.denoise(None, ehs, ehs1, m1, N, gs, source=A.EditSource(x0=x0, z0=z0), start=k)
    assert (pipe.graph_captures, pipe.graph_hits) == (1, 1)
    monkeypatch.undo()
    # by hand
    sched = mk()
    sched.set_timesteps(N)
    a, s = sched.add_noise_coefs(k)
    x = torch.empty(B, H * W, 8, device=dev)
    unet_in = torch.empty(B, H * W, 8, dtype=dtype, device=dev)
    ops.edit_start(_nhwc(z0), _nhwc(x0), x, unet_in, a, s)
    acp_t = SO.acp64()[SO.grid(N)[k]]
    assert rel_err(x, EO.add_noise(_nhwc(x0).cpu(), _nhwc(z0).cpu(), SO.grid(N)[k], SO.acp64()).float()) < 1e-6 and abs(a * a - acp_t) < 1e-12
    hist = torch.zeros_like(x)
    coef = (sched.sampler_rows(start=k).float() if sampler == "dpm" else sched.coef_table()[k:].contiguous()).to(dev)
    step_ptr = torch.zeros(1, dtype=torch.int32, device=dev)
    with torch.no_grad():
        u.set_kv_cache(True)
        u.precompute_time_tables(sched.timesteps[k:].to(dev), step_ptr)
        try:
            for _ in range(N - k):
                eps2 = u.forward_nhwc(unet_in, H, W, None, ehs.to(dtype), ehs1.to(dtype), None, m1, batch_repeat=2)
                if sampler == "dpm":
                    ops.cfg_sampler_step(eps2, x, unet_in, coef, step_ptr, gs, None, hist)
                else:
                    ops.cfg_ddim_step(eps2, x, unet_in, coef, step_ptr, gs)
                ops.step_advance(step_ptr)
        finally:
            u.clear_time_tables()
            u.set_kv_cache(False)
    ref = x.reshape(B, H, W, 8).permute(0, 3, 1, 2)
    assert torch.equal(eager, ref) and torch.equal(graph, ref) and torch.equal(again, ref)
    # it is a different result from the full run's, and from another strength's
    assert not torch.equal(pipe.denoise(None, ehs, ehs1, m1, N, gs, source=(x0, z0, None), start=3, use_graph=False), ref)


@pytest.mark.parametrize("sampler,eta", [("ddim", 0.0), ("dpm", 0.0), ("ddim", 0.5)])
def test_masked_run_captured_eager_replayed(dev, monkeypatch, sampler, eta):
    import ap_adapter_amd as A
    dtype = torch.bfloat16
    u, cfg, sd, procs = _small_unet(dev, dtype)
    u.requires_grad_(False)
    B, H, W, N, k, gs = 2, 26, 16, 8, 3, 7.5
    mk = (lambda: A.DPMSolverMultistepScheduler()) if sampler == "dpm" else (lambda: A.DDIMScheduler())
    pipe = A.AudioLDM2Pipeline(u, scheduler=mk())
    in1, in2 = _inputs(dev, dtype, seed=2)[1:], _inputs(dev, dtype, seed=3)[1:]
    x0, z0 = _source(dev, B)
    x0b, z0b = _source(dev, B, seed=80)
    mask = torch.zeros(B, 1, H, W, device=dev)
    mask[0, :, 5:14], mask[1, :, :, 3:9] = 1.0, 0.5   # clip 0: rows 5..13 regenerated; clip 1: a half-blended band of frequencies
    maskb = torch.zeros(B, 1, H, W, device=dev)
    maskb[:, :, 10:20] = 1.0
    g = lambda seed: torch.Generator().manual_seed(seed)
    calls = _count(monkeypatch, ("cfg_ddim_step", "cfg_sampler_step", "cfg_edit_step"))
    a = pipe.denoise(None, *in1, N, gs, source=(x0, z0, mask), start=k, eta=eta, generator=g(5))
    assert (pipe.graph_captures, pipe.graph_hits) == (1, 0)
    n_graph = len(calls["cfg_edit_step"])
    eager = pipe.denoise(None, *in1, N, gs, source=(x0, z0, mask), start=k, eta=eta, generator=g(5), use_graph=False)
    assert len(calls["cfg_edit_step"]) - n_graph == N - k and len(calls["cfg_ddim_step"]) == len(calls["cfg_sampler_step"]) == 0
    monkeypatch.undo()
    assert torch.equal(a, eager) and bool(torch.isfinite(a).all())
    # kept pixels: the source's bits; regenerated ones differ; the half-blended band is neither
    kept, regen = (mask == 0).expand(B, 8, H, W), (mask == 1).expand(B, 8, H, W)
    assert torch.equal(a[kept], x0[kept]) and not bool((a[regen] == x0[regen]).any()) and bool(kept.any()) and bool(regen.any())
    assert not bool((a[1, :, :, 3:9] == x0[1, :, :, 3:9]).any())
    # a second call with another source, mask and conditions replays the captured step and equals that call run eagerly
    b = pipe.denoise(None, *in2, N, gs, source=(x0b, z0b, maskb), start=k, eta=eta, generator=g(6))
    assert (pipe.graph_captures, pipe.graph_hits) == (1, 1)
    fresh = A.AudioLDM2Pipeline(u, scheduler=mk())
    assert torch.equal(b, fresh.denoise(None, *in2, N, gs, source=(x0b, z0b, maskb), start=k, eta=eta, generator=g(6), use_graph=False))
    keptb = (maskb == 0).expand(B, 8, H, W)
    assert torch.equal(b[keptb], x0b[keptb]) and not torch.equal(b, a)
    assert torch.equal(pipe.denoise(None, *in1, N, gs, source=(x0, z0, mask), start=k, eta=eta, generator=g(5)), a) and pipe.graph_hits == 2
    # a shared mask is another captured step (the kernel indexes it differently); so are another start and the unmasked run
    shared = pipe.denoise(None, *in1, N, gs, source=(x0, z0, maskb[:1]), start=k, eta=eta, generator=g(5))
    assert pipe.graph_captures == 2
    assert torch.equal(shared, pipe.denoise(None, *in1, N, gs, source=(x0, z0, maskb), start=k, eta=eta, generator=g(5), use_graph=False))
    # an all-ones mask is the strength-only run, bit for bit -- where that run is on apad_cfg_sampler_step, whose bits apad_cfg_edit_step
    # reproduces at mask = 1.  Strength-only deterministic DDIM stays on apad_cfg_ddim_step (every earlier caller's kernel), whose compiled
    # multiply-adds already round differently from apad_cfg_sampler_step's in the last fp32 bit, so no bit equality exists to assert there.
    ones = pipe.denoise(None, *in1, N, gs, source=(x0, z0, torch.ones(1, 1, H, W, device=dev)), start=k, eta=eta, generator=g(5), use_graph=False)
    plain = pipe.denoise(None, *in1, N, gs, source=(x0, z0, None), start=k, eta=eta, generator=g(5), use_graph=False)
    if not (sampler == "ddim" and eta == 0.0):
        assert torch.equal(ones, plain)
    assert not torch.equal(plain, a) and not torch.equal(ones, a)


def test_masked_run_is_independent_of_the_batch(dev):
    """clip 0 of a batch of 3 (per-clip masks) equals the same clip run alone"""
    import ap_adapter_amd as A
    dtype = torch.bfloat16
    u, cfg, sd, procs = _small_unet(dev, dtype)
    u.requires_grad_(False)
    B, H, W, N, k, gs = 3, 26, 16, 6, 2, 7.5
    pipe = A.AudioLDM2Pipeline(u, scheduler=A.DPMSolverMultistepScheduler())
    _, ehs, ehs1, m1 = _inputs(dev, dtype, B=B)
    x0, z0 = _source(dev, B)
    mask = (torch.rand(B, 1, H, W, generator=torch.Generator().manual_seed(4)) > 0.5).float().to(dev)
    three = pipe.denoise(None, ehs, ehs1, m1, N, gs, source=(x0, z0, mask), start=k)
    pick = lambda t: torch.cat([t[0:1], t[B:B + 1]])  # clip 0 of the [negative; positive] halves
    one = pipe.denoise(None, pick(ehs), pick(ehs1), pick(m1), N, gs, source=(x0[:1], z0[:1], mask[:1]), start=k)
    assert torch.equal(three[:1], one)


def test_default_path_reaches_neither_new_op(dev, monkeypatch):
    import ap_adapter_amd as A
    dtype = torch.bfloat16
    u, cfg, sd, procs = _small_unet(dev, dtype)
    u.requires_grad_(False)
    lat, ehs, ehs1, m1 = _inputs(dev, dtype)
    B, steps, gs = 2, 3, 7.5
    calls = _count(monkeypatch, ("cfg_ddim_step", "cfg_sampler_step", "cfg_edit_step", "edit_start"))
    kw = dict(prompt_embeds=ehs1[B:], negative_prompt_embeds=ehs1[:B], generated_prompt_embeds=ehs[B:], negative_generated_prompt_embeds=ehs[:B],
              attention_mask=m1[B:], negative_attention_mask=m1[:B], audio_length_in_s=1.04, num_inference_steps=steps, guidance_scale=gs,
              output_type="latent")
    for sched, used in ((A.DDIMScheduler(), "cfg_ddim_step"), (A.DPMSolverMultistepScheduler(), "cfg_sampler_step")):
        pipe = A.AudioLDM2Pipeline(u, scheduler=sched)
        before = len(calls[used])
        out = pipe(latents=lat, use_graph=False, **kw).audios
        assert len(calls[used]) - before == steps and len(calls["cfg_edit_step"]) == 0 and len(calls["edit_start"]) == 0
        assert torch.equal(out, pipe.denoise(lat, ehs, ehs1, m1, steps, gs, use_graph=False))
        assert torch.equal(out, pipe(latents=lat, **kw).audios)  # captured
    assert len(calls["cfg_edit_step"]) == 0 and len(calls["edit_start"]) == 0


# ---- through the VAE encoder and a wav file ----
def _small_vae(dev, dtype):
    import ap_adapter_amd as A
    from ap_adapter_amd.synthetic import init_synthetic_
    vcfg = A.VaeConfig(block_out_channels=(32, 64, 64), layers_per_block=1, norm_num_groups=8)
    torch.manual_seed(13)
    vae = A.AutoencoderKL(vcfg)
    init_synthetic_(vae, 13, w_std=0.05, bias_std=0.02, norm_jitter=0.1)
    return vae.to(dev, dtype), vcfg


def _call_kw(ehs, ehs1, m1, B, N, gs):
    return dict(prompt_embeds=ehs1[B:], negative_prompt_embeds=ehs1[:B], generated_prompt_embeds=ehs[B:], negative_generated_prompt_embeds=ehs[:B],
                attention_mask=m1[B:], negative_attention_mask=m1[:B], audio_length_in_s=1.04, num_inference_steps=N, guidance_scale=gs,
                output_type="latent")


def test_source_mel_through_the_vae(dev, monkeypatch):
    """source_mel -> AutoencoderKL.encode -> apad_edit_start -> masked loop -> output_type='latent'.  The generator is drawn in the order
    posterior noise, z0; x0 equals latent_dist.sample(noise=the same draw) * scaling_factor to one rounding of the model dtype (that
    method returns the model dtype, see test_edit_start_matches_fp64)"""
    import ap_adapter_amd as A
    from ap_adapter_amd import ops
    dtype = torch.bfloat16
    u, cfg, sd, procs = _small_unet(dev, dtype)
    u.requires_grad_(False)
    vae, vcfg = _small_vae(dev, dtype)
    B, H, W, N, gs = 2, 26, 16, 8, 7.5
    _, ehs, ehs1, m1 = _inputs(dev, dtype)
    mel = (R(B, 1, 104, 64, seed=90) * 2.0 - 4.0).to(dev)
    pipe = A.AudioLDM2Pipeline(u, vae=vae)
    kw = _call_kw(ehs, ehs1, m1, B, N, gs)
    captured = {}
    real = ops.edit_start

    def spy(z0, x0, latents, unet_in, a, s, **k2):
        real(z0, x0, latents, unet_in, a, s, **k2)
        captured.update(x0=x0.clone(), z0=z0.clone(), lat=latents.clone(), a=a, s=s, moments=k2.get("moments"))

    monkeypatch.setattr(ops, "edit_start", spy)
    out = pipe(source_mel=mel, strength=0.5, edit_region=(0.2, 0.6), generator=torch.Generator().manual_seed(11), use_graph=False, **kw).audios
    monkeypatch.undo()
    assert out.shape == (B, 8, H, W) and captured["moments"] is not None
    g2 = torch.Generator().manual_seed(11)
    post = torch.randn(B, 8, H, W, generator=g2)
    z0 = torch.randn(B, 8, H, W, generator=g2)
    x0_nchw = captured["x0"].reshape(B, H, W, 8).permute(0, 3, 1, 2)
    assert torch.equal(captured["z0"].reshape(B, H, W, 8).permute(0, 3, 1, 2).cpu(), z0)
    ref = vae.encode(mel).latent_dist.sample(noise=post.to(dev), scale=vcfg.scaling_factor).float()
    # sample() reads the noise in the model dtype, edit_start in fp32: one more model-dtype rounding, of the noise, scaled by std -- bound
    # the difference by one unit in the last place of the model dtype relative to the largest latent
    assert rel_err(x0_nchw, ref) < torch.finfo(dtype).eps
    sched = A.DDIMScheduler()
    sched.set_timesteps(N)
    k = sched.edit_start_index(N, 0.5)
    assert (captured["a"], captured["s"]) == sched.add_noise_coefs(k) and k == 4
    # the kept region (outside 0.2 .. 0.6 s = latent rows 5 .. 14) is x0, bit for bit; the rest is not
    assert torch.equal(out[:, :, :5], x0_nchw[:, :, :5]) and torch.equal(out[:, :, 15:], x0_nchw[:, :, 15:])
    assert not bool((out[:, :, 5:15] == x0_nchw[:, :, 5:15]).any())
    # the same call captured, and through denoise with the EditSource spelled out
    assert torch.equal(out, pipe(source_mel=mel, strength=0.5, edit_region=(0.2, 0.6), generator=torch.Generator().manual_seed(11), **kw).audios)
    mask = torch.zeros(1, 1, H, W)
    mask[:, :, 5:15] = 1.0
    src = A.EditSource(z0=z0, moments=vae.encode(mel).latent_dist._m.reshape(B * H * W, 16), post_noise=post, scale=vcfg.scaling_factor, mask=mask)
    assert torch.equal(out, pipe.denoise(None, ehs, ehs1, m1, N, gs, source=src, start=k, use_graph=False))
    # source_latents = that x0: the same run without the posterior draw (z0 is then the generator's FIRST draw)
    g3 = torch.Generator().manual_seed(11)
    torch.randn(B, 8, H, W, generator=g3)
    assert torch.equal(out, pipe(source_latents=x0_nchw, strength=0.5, edit_region=(0.2, 0.6), generator=g3, **kw).audios)


def test_source_audio_from_a_wav_file(dev, tmp_path):
    import ap_adapter_amd as A
    from ap_adapter_amd import frontend as FE
    dtype = torch.bfloat16
    u, cfg, sd, procs = _small_unet(dev, dtype)
    u.requires_grad_(False)
    vae, vcfg = _small_vae(dev, dtype)
    B, H, W, N, gs = 2, 26, 16, 8, 7.5
    _, ehs, ehs1, m1 = _inputs(dev, dtype)
    sr = 16000
    t = np.arange(int(1.5 * sr)) / sr
    wav = 0.4 * np.sin(2 * np.pi * (200 + 900 * t) * t) + 0.02 * np.random.RandomState(0).randn(t.size)
    path = tmp_path / "clip.wav"
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(sr)
        w.writeframes(np.clip(np.round(wav * 32768.0), -32768, 32767).astype("<i2").tobytes())
    pipe = A.AudioLDM2Pipeline(u, vae=vae)
    kw = _call_kw(ehs, ehs1, m1, B, N, gs)
    g = lambda: torch.Generator().manual_seed(3)
    out = pipe(source_audio=str(path), strength=0.75, edit_region=(0.4, 0.8), generator=g(), **kw).audios
    mel = FE.wav_to_mel(str(path), (104 + 0.5) / 102.4, device=dev)
    assert mel.shape == (1, 104, 64)
    assert torch.equal(out, pipe(source_mel=mel, strength=0.75, edit_region=(0.4, 0.8), generator=g(), **kw).audios)   # one clip for the whole batch
    assert torch.equal(out, pipe(source_audio=[str(path), str(path)], strength=0.75, edit_region=(0.4, 0.8), generator=g(), **kw).audios)
    assert out.shape == (B, 8, H, W) and bool(torch.isfinite(out).all())
    assert not torch.equal(out[0], out[1])  # one source, but each clip has its own posterior draw and its own z0
