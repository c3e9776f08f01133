"""-m gpu: separate audio and text guidance -- apad_cfg_dual_step against the restatement (tests/guidance_oracle.py), its collapse onto
the two-branch entry points bit for bit, its rejections and bounds, the UNet at an odd effective batch (three sample-forwards per clip),
and the three-branch denoise loop captured / eager / hand-driven, swept without a re-capture, with editing, and isolated from the UNet's
rounding.  PARITY UNPINNED (see guidance_oracle)."""
import pytest
import torch

from util import TOL, guarded, q, rel_err

import guidance_oracle as GO
import sampler_oracle as SO
from test_gpu_edit import _fma32, _full, _mask
from test_gpu_samplers import _check_step, _count
from test_gpu_unet import _cond, _small_unet

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float16, torch.float32]
NS = [4000 * 8, 4001]  # 16-byte accesses / the scalar form (B * n not a multiple of 8)


def R(*shape, seed=0, std=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * std


def _sched(sampler):
    import ap_adapter_amd as A
    return A.DPMSolverMultistepScheduler() if sampler == "dpm" else A.DDIMScheduler()


# ---------------------------------------------------------------------------------------------------------------------
# kernel level
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("sampler,eta", [("dpm", 0.0), ("ddim", 1.0), ("ddim", 0.0)])
def test_cfg_dual_step_matches_restatement(dev, sampler, eta, dtype, n):
    """every step of a 10-step run on random eps3 with a guidance table that VARIES per step (s_A 1 -> 4, s_T 7.5 -> 3: the row is read at
    *step_ptr): guided noise, fp32 master latents, model-dtype copy and the data-prediction history.  Bounds: test_gpu_samplers._check_step's
    (eps 1e-6, latents 1e-5, unet_in TOL[dtype]) and 1e-5 for m0 -- the same arithmetic plus one fma."""
    from ap_adapter_amd import ops
    from ap_adapter_amd.scheduler import guidance_table
    B, steps = 3, 10
    s = _sched(sampler)
    s.set_timesteps(steps)
    plan = s.sampler_plan(eta, dual=True)
    assert not plan.legacy and plan.table.shape == (steps, 6)
    s_a, s_t = GO.ramp(1.0, 4.0, steps), GO.ramp(7.5, 3.0, steps)
    gtab = guidance_table(s_a, s_t, steps)
    coef, gtab_d = plan.table.to(dev), gtab.to(dev)
    acp, ts = SO.acp64(), SO.grid(steps)
    noise = R(steps, B, n, seed=9) if plan.needs_noise else None
    noise_d = None if noise is None else noise.to(dev)
    lat = R(B, n, seed=44).double()
    lat_d = lat.float().to(dev)
    unet_in = torch.empty(B, n, dtype=dtype, device=dev)
    eps_out = torch.empty(B, n, dtype=torch.float32, device=dev)
    hist = torch.zeros(B, n, dtype=torch.float32, device=dev) if plan.needs_history else None
    step_ptr = torch.zeros(1, dtype=torch.int32, device=dev)
    m1, worst = None, [0.0, 0.0, 0.0, 0.0]
    for i in range(steps):
        eps3 = q(R(3 * B, n, seed=100 + i) * 0.5, dtype)
        e = GO.cfg3_combine_rounded(eps3, float(gtab[i, 0]), float(gtab[i, 1]), dtype)
        if sampler == "dpm":
            lat, m1 = SO.dpm_step(lat, e, m1, i, ts, acp)
        else:
            lat = SO.ddim_step(lat, e, None if noise is None else noise[i], i, ts, acp, eta=eta)
        ops.cfg_dual_step(eps3.to(dev, dtype), lat_d, unet_in, coef, gtab_d, step_ptr, eps_out, hist, noise_d)
        ops.step_advance(step_ptr)
        errs = (rel_err(eps_out, e.float()), rel_err(lat_d, lat.float()), rel_err(unet_in, lat.float()),
                0.0 if hist is None else rel_err(hist, m1.float()))
        worst = [max(a, b) for a, b in zip(worst, errs)]
        print(f"[apad_cfg_dual_step {sampler} eta={eta}, {dtype}, n={n}] step {i}: eps {errs[0]:.2e} latents {errs[1]:.2e} unet_in {errs[2]:.2e} "
              f"m0 {errs[3]:.2e}")
        _check_step(dtype, lat_d, unet_in, eps_out, lat, e)
        assert errs[3] < 1e-5, errs
    print(f"\n[apad_cfg_dual_step {sampler} eta={eta}, {dtype}, n={n}] worst rel err: eps {worst[0]:.2e} latents {worst[1]:.2e} unet_in {worst[2]:.2e} "
          f"m0 {worst[3]:.2e}")
    assert int(step_ptr.item()) == steps
    # the guided noise really used row i: with row 0's scales the last step's noise is another one
    assert rel_err(eps_out, GO.cfg3_combine_rounded(eps3, s_a[0], s_t[0], dtype).float()) > 1e-2


def _two_vs_three(dev, dtype, n, eps2, eps3, g, s_a, s_t, step=2, steps=5, masked=None):
    """one launch of the two-branch entry point (guidance g) and one of apad_cfg_dual_step (row ``step`` = (s_a, s_t)) from the same
    latents / history / noise on a 2M-shaped random table; returns both sets of (latents, unet_in, eps_out, history)"""
    from ap_adapter_amd import ops
    B = eps2.shape[0] // 2
    coef = (R(steps, 6, seed=7) * 0.5 + 1.0).to(dev)  # every column non-zero: history and noise are both read
    gtab = torch.full((steps, 2), float("nan"))
    gtab[step] = torch.tensor([s_a, s_t])
    x, h, z = R(B, n, seed=44), R(B, n, seed=45) * 3.0, R(steps, B, n, seed=46)
    step_ptr = torch.full((1,), step, dtype=torch.int32, device=dev)
    outs = []
    for three in (False, True):
        lat, hist, noise = x.to(dev), h.to(dev), z.to(dev)
        unet_in = torch.empty(B, n, dtype=dtype, device=dev)
        eps_out = torch.empty(B, n, dtype=torch.float32, device=dev)
        if three:
            kw = {} if masked is None else dict(keep=masked["keep"], x0=masked["x0"], z0=masked["z0"], mask=masked["mask"], channels=masked["C"])
            ops.cfg_dual_step(eps3.to(dev, dtype), lat, unet_in, coef, gtab.to(dev), step_ptr, eps_out, hist, noise, **kw)
        elif masked is None:
            ops.cfg_sampler_step(eps2.to(dev, dtype), lat, unet_in, coef, step_ptr, g, eps_out, hist, noise)
        else:
            ops.cfg_edit_step(eps2.to(dev, dtype), lat, unet_in, coef, masked["keep"], step_ptr, g, masked["x0"], masked["z0"], masked["mask"],
                              masked["C"], eps_out, hist, noise)
        outs.append((lat, unet_in, eps_out, hist))
    return outs


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_collapse_identities_bit_for_bit(dev, dtype, n):
    """(a) eps3 = [u, u, c], any s_A, s_T = g   and   (b) eps3 = [u, a, a], s_A = g, any s_T   are apad_cfg_sampler_step([u, c] / [u, a], g) on
    latents, unet_in, eps_out and history, bit for bit, at dyadic scales (for f16 see
    test_dual_guidance_host.test_the_restatement_collapses_to_the_two_branch_expression)"""
    B = 3
    u, a = q(R(B, n, seed=100) * 0.5, dtype), q(R(B, n, seed=101) * 0.5, dtype)
    for g, other in ((7.5, 2.5), (2.5, 1.25), (1.25, 7.5)):
        for name, eps3, s_a, s_t in (("a", torch.cat([u, u, a]), other, g), ("b", torch.cat([u, a, a]), g, other)):
            two, three = _two_vs_three(dev, dtype, n, torch.cat([u, a]), eps3, g, s_a, s_t)
            for what, x2, x3 in zip(("latents", "unet_in", "eps_out", "history"), two, three):
                assert torch.equal(x2, x3), (name, g, what, rel_err(x3, x2))
            assert bool(torch.isfinite(three[0]).all())


@pytest.mark.parametrize("n", NS)
def test_equal_scales_are_the_two_branch_noise_to_fp32_rounding(dev, n):
    """s_A = s_T = g, fp32, one step: e_0 + g (e_A - e_0) + g (e_AT - e_A) against e_0 + g (e_AT - e_0): _check_step's eps bar (the host
    restatement gives 8.3e-8 on these inputs)"""
    B, g = 3, 7.5
    eps3 = R(3 * B, n, seed=100) * 0.5
    two, three = _two_vs_three(dev, torch.float32, n, torch.cat([eps3[:B], eps3[2 * B:]]), eps3, g, g, g)
    err = rel_err(three[2], two[2])
    print(f"\n[apad_cfg_dual_step s_A = s_T = {g}, fp32, n={n}] eps_out vs the two-branch eps_out: rel err {err:.2e}")
    assert err < 1e-6


@pytest.mark.parametrize("mask_kind", ["binary-clip", "binary-shared"])
@pytest.mark.parametrize("npix,C", [(4000, 8), (4001, 4)])  # the 16-byte form (C == 8) and the scalar form
@pytest.mark.parametrize("dtype", DTYPES)
def test_masked_form_is_cfg_edit_step_and_keeps_known_bits(dev, dtype, npix, C, mask_kind):
    """with mask / keep / x0 / z0 the launch equals apad_cfg_edit_step under identity (a), bit for bit; m = 0 pixels end as the bits of
    known = fma(kx, x0, kz * z0), m = 1 pixels as the bits of the unmasked launch"""
    B, g, step, steps = 3, 7.5, 2, 5
    n = npix * C
    u, c = q(R(B, n, seed=100) * 0.5, dtype), q(R(B, n, seed=101) * 0.5, dtype)
    keep = torch.rand(steps, 2, generator=torch.Generator().manual_seed(5)) + 0.25
    x0, z0, mask = R(B, n, seed=60), R(B, n, seed=61), _mask(mask_kind, B, npix)
    assert mask.shape[0] == (B if "clip" in mask_kind else 1)
    masked = dict(keep=keep.to(dev), x0=x0.to(dev), z0=z0.to(dev), mask=mask.to(dev), C=C)
    eps3 = torch.cat([u, u, c])
    two, three = _two_vs_three(dev, dtype, n, torch.cat([u, c]), eps3, g, 2.5, g, step, steps, masked)
    for what, x2, x3 in zip(("latents", "unet_in", "eps_out", "history"), two, three):
        assert torch.equal(x2, x3), (what, rel_err(x3, x2))
    _, plain = _two_vs_three(dev, dtype, n, torch.cat([u, c]), eps3, g, 2.5, g, step, steps, None)
    kept = (_full(mask, B, C) == 0).to(dev)
    known = _fma32(float(keep[step, 0]), x0, (keep[step, 1] * z0)).to(dev)  # fp32 product, one fma
    lat = three[0]
    assert torch.equal(lat[kept], known[kept]) and torch.equal(lat[~kept], plain[0][~kept]) and bool(kept.any()) and bool((~kept).any())
    assert torch.equal(three[1][~kept], plain[1][~kept]) and torch.equal(three[3], plain[3])  # m0 is formed before the blend


def test_cfg_dual_step_rejects_bad_operands(dev):
    """status + apad_last_error text from the entry point, RuntimeError from the wrapper; no operand is touched"""
    from ap_adapter_amd import _lib as L
    from ap_adapter_amd import ops
    B, npix, C, steps = 2, 24, 8, 5
    n = npix * C
    lat = torch.full((B, n), 1.5, device=dev)
    eps3 = torch.zeros(3 * B, n, dtype=torch.bfloat16, device=dev)
    unet_in = torch.full((B, n), 3.0, dtype=torch.bfloat16, device=dev)
    ptr = torch.zeros(1, dtype=torch.int32, device=dev)
    coef, gtab, keep = torch.ones(steps, 6, device=dev), torch.ones(steps, 2, device=dev), torch.ones(steps, 2, device=dev)
    x0, z0, mask = torch.zeros(B, n, device=dev), torch.zeros(B, n, device=dev), torch.ones(B, npix, device=dev)
    ed = dict(keep=keep, x0=x0, z0=z0, mask=mask, channels=C)
    with pytest.raises(RuntimeError, match=r"\[steps, 6\]"):
        ops.cfg_dual_step(eps3, lat, unet_in, torch.zeros(steps, 2, device=dev), gtab, ptr)
    for bad in (torch.ones(steps - 1, 2, device=dev), torch.ones(steps, 3, device=dev), torch.ones(2 * steps, device=dev),
                torch.ones(steps, 2, device=dev, dtype=torch.float64), torch.ones(steps, 4, device=dev)[:, ::2]):
        with pytest.raises(RuntimeError, match="guidance"):
            ops.cfg_dual_step(eps3, lat, unet_in, coef, bad, ptr)
    with pytest.raises(RuntimeError, match=r"eps3 must hold three branches"):
        ops.cfg_dual_step(eps3[: 2 * B], lat, unet_in, coef, gtab, ptr)
    with pytest.raises(RuntimeError, match=r"rc=-?\d+.*mask_batch 3 must be 1 or B = 2"):
        ops.cfg_dual_step(eps3, lat, unet_in, coef, gtab, ptr, **{**ed, "mask": torch.ones(3, npix, device=dev)})
    with pytest.raises(RuntimeError, match=r"rc=-?\d+.*not a multiple of C = 7"):
        ops.cfg_dual_step(eps3, lat, unet_in, coef, gtab, ptr, **{**ed, "channels": 7})
    with pytest.raises(RuntimeError, match=r"rc=-?\d+.*a mask needs the keep table, x0 and z0"):
        ops.cfg_dual_step(eps3, lat, unet_in, coef, gtab, ptr, **{**ed, "keep": None})
    with pytest.raises(RuntimeError, match=r"rc=-?\d+.*a mask needs the keep table, x0 and z0"):
        ops.cfg_dual_step(eps3, lat, unet_in, coef, gtab, ptr, **{**ed, "x0": None})
    with pytest.raises(RuntimeError, match="noise"):
        ops.cfg_dual_step(eps3, lat, unet_in, coef, gtab, ptr, noise=torch.zeros(steps - 1, B, n, device=dev))
    # the entry point itself: a status code and a message, never an abort
    lib = L.lib()
    args = lambda g, dt: (eps3.data_ptr(), lat.data_ptr(), unet_in.data_ptr(), None, None, None, coef.data_ptr(), g, None, None, None, None, 0, C,
                          ptr.data_ptr(), steps, B, n, dt, None)
    rc = lib.apad_cfg_dual_step(*args(None, L.BF16))
    assert rc != 0 and b"apad_cfg_dual_step: null guidance table" in lib.apad_last_error()
    rc = lib.apad_cfg_dual_step(*args(gtab.data_ptr(), 7))
    assert rc != 0 and b"apad_cfg_dual_step: dtype 7 not supported" in lib.apad_last_error()
    rc = lib.apad_cfg_dual_step(None, lat.data_ptr(), unet_in.data_ptr(), None, None, None, coef.data_ptr(), gtab.data_ptr(), None, None, None, None, 0,
                                C, ptr.data_ptr(), steps, B, n, L.BF16, None)
    assert rc != 0 and b"apad_cfg_dual_step: null operand" in lib.apad_last_error()
    torch.cuda.synchronize()
    assert bool((lat == 1.5).all()) and bool((unet_in == 3.0).all())  # nothing was launched
    # a step counter beyond the tables reads their last rows, not past them
    ptr.fill_(1000)
    coef.zero_()
    coef[steps - 1, 0] = 2.0
    gtab[:steps - 1] = float("nan")
    ops.cfg_dual_step(eps3, lat, unet_in, coef, gtab, ptr)
    assert bool((lat == 3.0).all())


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_guard_bands_and_nan_prefilled_outputs(dev, dtype, n):
    """every buffer the launch writes sits between NaN guard bands and starts as NaN: nothing outside its B * n elements changes, every
    element inside is written; a null history is not written (there is none to write) and the noise row of a step whose c_z is 0 is not
    read (it holds NaN)"""
    from ap_adapter_amd import ops
    B, steps, G = 3, 4, 2
    eps3 = q(R(3 * B, n, seed=100) * 0.5, dtype).to(dev, dtype)
    coef = (R(steps, 6, seed=7) * 0.5 + 1.0)
    coef[1, 3] = 0.0   # step 1 adds no noise
    coef[0, 2] = 0.0   # step 0 reads no history
    gtab = torch.tensor([[2.5, 7.5]] * steps).to(dev)
    noise = R(steps, B, n, seed=46)
    noise[1] = float("nan")
    noise_d, coef_d = noise.to(dev), coef.to(dev)
    x = R(B, n, seed=44)
    for step, with_hist in ((0, True), (1, True), (1, False), (3, True)):
        lat, lat_check = guarded(B, n, torch.float32, dev, guard_rows=G)
        lat.copy_(x)
        unet_in, ui_check = guarded(B, n, dtype, dev, guard_rows=G)
        eps_out, eo_check = guarded(B, n, torch.float32, dev, guard_rows=G)
        hist, h_check = guarded(B, n, torch.float32, dev, guard_rows=G)
        if step != 0:
            hist.copy_(R(B, n, seed=45))  # (step 0 leaves it NaN: c_m is 0, so it is written without being read)
        assert lat.is_contiguous() and unet_in.is_contiguous()
        ptr = torch.full((1,), step, dtype=torch.int32, device=dev)
        ops.cfg_dual_step(eps3, lat, unet_in, coef_d, gtab, ptr, eps_out, hist if with_hist else None, noise_d)
        for check, what in ((lat_check, "latents"), (ui_check, "unet_in"), (eo_check, "eps_out")) + (((h_check, "history"),) if with_hist else ()):
            check(f"apad_cfg_dual_step step {step} {what}")
        assert torch.equal(noise_d[0], noise[0].to(dev)) and torch.equal(coef_d, coef.to(dev))  # inputs untouched
        if not with_hist:  # without a history buffer the m1 term is 0
            lat2 = x.to(dev)
            ops.cfg_dual_step(eps3, lat2, torch.empty_like(unet_in), coef_d, gtab, ptr, None, torch.zeros(B, n, device=dev), noise_d)
            assert torch.equal(lat, lat2)


# ---------------------------------------------------------------------------------------------------------------------
# UNet and pipeline level (small synthetic UNet)
# ---------------------------------------------------------------------------------------------------------------------
def _inputs3(dev, dtype, B=2, H=26, W=16, seed=2):
    """latents [B, 8, H, W] and the conditions of 3B rows: [no condition ; audio ; audio + text] as assemble_condition(branches=3) lays them
    out -- branches 0 and A share the text tokens (the first 8) and the T5 states, A and AT share the audio tokens (the last 32)"""
    lat = torch.randn(B, 8, H, W, generator=torch.Generator().manual_seed(seed))
    ehs, ehs1, m1 = _cond(2 * B, 32, dtype, seed=seed)  # [negative | zero-mel ; positive | audio]
    neg, pos = ehs[:B], ehs[B:]
    ehs3 = torch.cat([neg, torch.cat([neg[:, :8], pos[:, 8:]], 1), pos])
    ehs1_3, m1_3 = torch.cat([ehs1[:B], ehs1]), torch.cat([m1[:B], m1])
    return lat.to(dev), ehs3.to(dev), ehs1_3.to(dev), m1_3.to(dev)


def _pick(t, B, branches):
    return torch.cat([t[b * B:(b + 1) * B] for b in branches])


def _forward(u, dev, dtype, x, cond, repeat, H=26, W=16, steps=3):
    import ap_adapter_amd as A
    sched = A.DDIMScheduler()
    sched.set_timesteps(steps)
    step_ptr = torch.ones(1, dtype=torch.int32, device=dev)
    ehs, ehs1, m1 = cond
    with torch.no_grad():
        u.set_kv_cache(True)
        u.precompute_time_tables(sched.timesteps.to(dev), step_ptr)
        try:
            return u.forward_nhwc(x, H, W, None, ehs.to(dtype), ehs1.to(dtype), None, m1, batch_repeat=repeat).clone()
        finally:
            u.clear_time_tables()
            u.set_kv_cache(False)


@pytest.mark.parametrize("B", [1, 2])
def test_odd_effective_batch_rows_equal_the_even_batches(dev, monkeypatch, B):
    """3 and 6 sample-forwards: the rows of ONE forward_nhwc(batch_repeat=3) are the bits of the same (latent, condition) pairs in two
    batch_repeat=2 forwards, [0, AT] and [0, A] (a row's arithmetic does not depend on the batch); and the fused routes
    agree with the chain within TOL at this batch too"""
    from ap_adapter_amd import ops
    from ap_adapter_amd import processors as P
    dtype = torch.bfloat16
    u, cfg, sd, procs = _small_unet(dev, dtype)
    u.requires_grad_(False)
    lat, ehs, ehs1, m1 = _inputs3(dev, dtype, B=B)
    x = lat.float().permute(0, 2, 3, 1).reshape(B, 26 * 16, 8).to(dtype).contiguous()
    three = _forward(u, dev, dtype, x, (ehs, ehs1, m1), 3)
    assert three.shape[0] == 3 * B and bool(torch.isfinite(three).all())
    two_at = _forward(u, dev, dtype, x, tuple(_pick(t, B, (0, 2)) for t in (ehs, ehs1, m1)), 2)
    two_a = _forward(u, dev, dtype, x, tuple(_pick(t, B, (0, 1)) for t in (ehs, ehs1, m1)), 2)
    r = lambda t, b: t[b * B:(b + 1) * B]
    pairs = (("0 vs [0, AT]", r(three, 0), r(two_at, 0)), ("AT vs [0, AT]", r(three, 2), r(two_at, 1)), ("0 vs [0, A]", r(three, 0), r(two_a, 0)),
             ("A vs [0, A]", r(three, 1), r(two_a, 1)))
    for name, a, b in pairs:
        print(f"[batch_repeat=3, B={B}] rows {name}: rel err {rel_err(a, b):.3e}")
    for name, a, b in pairs:
        assert torch.equal(a, b), name
    assert not torch.equal(r(three, 0), r(three, 1)) and not torch.equal(r(three, 1), r(three, 2))
    monkeypatch.setattr(P, "USE_FUSED_XATTN", False)
    for name in ("HS_ATTN", "SATTN_FUSED", "MLP_PACKED"):
        monkeypatch.setattr(ops, name, False)
    chain = _forward(u, dev, dtype, x, (ehs, ehs1, m1), 3)
    err = rel_err(three, chain)
    print(f"[batch_repeat=3, B={B}] fused routes vs the chain: rel err {err:.3e}")
    assert err < TOL[dtype]


def _hand_loop(u, dev, dtype, sched, lat, cond, steps, gtab, eta=0.0, H=26, W=16):
    """the three-branch loop written out over forward_nhwc(batch_repeat=3), ops.cfg_dual_step and ops.step_advance"""
    from ap_adapter_amd import ops
    B = lat.shape[0]
    ehs, ehs1, m1 = cond
    sched.set_timesteps(steps)
    plan = sched.sampler_plan(eta, dual=True)
    coef = plan.table.to(dev)
    step_ptr = torch.zeros(1, dtype=torch.int32, device=dev)
    x = lat.float().permute(0, 2, 3, 1).reshape(B, H * W, 8).contiguous()
    unet_in = x.to(dtype)
    hist = torch.zeros_like(x) if plan.needs_history else None
    with torch.no_grad():
        u.set_kv_cache(True)
        u.precompute_time_tables(sched.timesteps.to(dev), step_ptr)
        try:
            for _ in range(steps):
                eps3 = u.forward_nhwc(unet_in, H, W, None, ehs.to(dtype), ehs1.to(dtype), None, m1, batch_repeat=3)
                ops.cfg_dual_step(eps3, x, unet_in, coef, gtab.to(dev), step_ptr, None, hist)
                ops.step_advance(step_ptr)
        finally:
            u.clear_time_tables()
            u.set_kv_cache(False)
    return x.reshape(B, H, W, 8).permute(0, 3, 1, 2)


@pytest.mark.parametrize("sampler", ["ddim", "dpm"])
def test_captured_eager_and_hand_driven_loops_agree_bit_for_bit(dev, monkeypatch, sampler):
    """3 steps with audio_guidance_scale = 2.5: captured == eager == a loop driven by hand; only apad_cfg_dual_step runs, once per step;
    and with audio_guidance_scale = None the launches are today's, the new op never"""
    import ap_adapter_amd as A
    from ap_adapter_amd.scheduler import guidance_table
    dtype = torch.bfloat16
    u, cfg, sd, procs = _small_unet(dev, dtype)
    u.requires_grad_(False)
    B, steps, gs, ags = 2, 3, 7.5, 2.5
    lat, ehs, ehs1, m1 = _inputs3(dev, dtype, B=B)
    two = tuple(_pick(t, B, (0, 2)) for t in (ehs, ehs1, m1))
    pipe = A.AudioLDM2Pipeline(u, scheduler=_sched(sampler))
    calls = _count(monkeypatch, ("cfg_dual_step", "cfg_ddim_step", "cfg_sampler_step", "cfg_edit_step"))
    n = lambda: tuple(len(calls[k]) for k in ("cfg_dual_step", "cfg_ddim_step", "cfg_sampler_step", "cfg_edit_step"))
    eager = pipe.denoise(lat, ehs, ehs1, m1, steps, gs, use_graph=False, audio_guidance_scale=ags)
    assert n() == (steps, 0, 0, 0)
    seen = []
    cb = pipe.denoise(lat, ehs, ehs1, m1, steps, gs, audio_guidance_scale=ags, callback=lambda i, t, x: seen.append(i))  # a callback forces the eager loop
    assert n() == (2 * steps, 0, 0, 0) and seen == list(range(steps)) and pipe.graph_captures == 0
    graph = pipe.denoise(lat, ehs, ehs1, m1, steps, gs, audio_guidance_scale=ags)
    again = pipe.denoise(lat, ehs, ehs1, m1, steps, gs, audio_guidance_scale=ags)
    assert (pipe.graph_captures, pipe.graph_hits) == (1, 1) and n()[1:] == (0, 0, 0)
    before = n()
    default = pipe.denoise(lat, *two, steps, gs, use_graph=False)  # audio_guidance_scale=None: today's path
    want = (0, steps, 0, 0) if sampler == "ddim" else (0, 0, steps, 0)
    assert tuple(a - b for a, b in zip(n(), before)) == want
    default_graph = pipe.denoise(lat, *two, steps, gs)
    assert n()[0] == before[0] and pipe.graph_captures == 2 and torch.equal(default, default_graph)
    monkeypatch.undo()
    ref = _hand_loop(u, dev, dtype, _sched(sampler), lat, (ehs, ehs1, m1), steps, guidance_table(ags, gs, steps))
    assert torch.equal(eager, ref) and torch.equal(cb, ref) and torch.equal(graph, ref) and torch.equal(again, ref)
    assert bool(torch.isfinite(ref).all()) and not torch.equal(ref, default)
    # the default path's key is today's: the two-branch graph is keyed by its guidance value, the dual one by the marker
    assert sum(1 for k in pipe._graphs if "dual" in k) == 1 and sum(1 for k in pipe._graphs if gs in k) == 1
    with pytest.raises(NotImplementedError, match="classifier-free guidance"):
        pipe.denoise(lat, *two, steps, 1.0)
    assert bool(torch.isfinite(pipe.denoise(lat, ehs, ehs1, m1, steps, 1.0, audio_guidance_scale=0.0)).all())  # any scale >= 0 with three branches


def test_a_guidance_sweep_replays_one_captured_graph(dev):
    """other scale values, then a per-step sequence: graph_captures stays 1, each result is a fresh pipeline's bit for bit, and the first
    values reproduce the first latents"""
    import ap_adapter_amd as A
    dtype = torch.bfloat16
    u, cfg, sd, procs = _small_unet(dev, dtype)
    u.requires_grad_(False)
    B, steps = 2, 3
    inp = _inputs3(dev, dtype, B=B)
    pipe = A.AudioLDM2Pipeline(u, scheduler=A.DPMSolverMultistepScheduler())
    sweep = [(2.5, 7.5), (1.0, 9.5), (GO.ramp(1.0, 4.0, steps), GO.ramp(7.5, 3.0, steps)), (0.0, [3.0, 3.0, 0.0])]
    outs = []
    for ags, gs in sweep:
        outs.append(pipe.denoise(*inp, steps, gs, audio_guidance_scale=ags))
        assert pipe.graph_captures == 1
        fresh = A.AudioLDM2Pipeline(u, scheduler=A.DPMSolverMultistepScheduler())
        assert torch.equal(outs[-1], fresh.denoise(*inp, steps, gs, audio_guidance_scale=ags, use_graph=False)), (ags, gs)
    assert pipe.graph_hits == len(sweep) - 1
    assert all(not torch.equal(outs[0], o) for o in outs[1:])
    assert torch.equal(pipe.denoise(*inp, steps, sweep[0][1], audio_guidance_scale=sweep[0][0]), outs[0]) and pipe.graph_captures == 1
    with pytest.raises(ValueError, match="^audio"):
        pipe.denoise(*inp, steps, 7.5, audio_guidance_scale=-1.0)
    with pytest.raises(ValueError, match="^text holds 2"):
        pipe.denoise(*inp, steps, [7.5, 7.5], audio_guidance_scale=1.0)


def test_inert_audio_tokens_collapse_onto_the_two_branch_run(dev):
    """ap_scale = 0 on every processor: the audio tokens do nothing, e_A is e_0 bit for bit, so denoise(audio_guidance_scale=s,
    guidance_scale=g) is denoise(guidance_scale=g) on the [0, AT] conditions for every s (DPM-Solver++: both runs use the 16-byte form of
    the same sampler_update; deterministic DDIM's two-branch run is on apad_cfg_ddim_step, whose multiply-adds round differently)"""
    import ap_adapter_amd as A
    dtype = torch.bfloat16
    u, cfg, sd, procs = _small_unet(dev, dtype)
    u.requires_grad_(False)
    n_ip = 0
    for p in u.attn_processors.values():
        if hasattr(p, "to_k_ip"):
            p.scale = 0.0
            n_ip += 1
    assert n_ip > 0
    B, steps, gs = 2, 3, 7.5
    lat, ehs, ehs1, m1 = _inputs3(dev, dtype, B=B)
    two = tuple(_pick(t, B, (0, 2)) for t in (ehs, ehs1, m1))
    pipe = A.AudioLDM2Pipeline(u, scheduler=A.DPMSolverMultistepScheduler())
    ref = pipe.denoise(lat, *two, steps, gs)
    for s in (2.5, 0.75):
        out = pipe.denoise(lat, ehs, ehs1, m1, steps, gs, audio_guidance_scale=s)
        print(f"[ap_scale = 0, s_A = {s}] three-branch vs two-branch latents: rel err {rel_err(out, ref):.3e}")
        assert torch.equal(out, ref), s


def _stub_audio(pipe, dev, La=32, seed=21):
    """stand-in for the AudioMAE front end: fixed prompt tokens and zero-mel tokens [1, La, 768]"""
    tok, unc = R(1, La, 768, seed=seed).to(dev), R(1, La, 768, seed=seed + 1).to(dev)
    pipe.encode_audio = lambda mel, tp, fp: (tok, unc)
    return tok, unc


def _call_kw(ehs, ehs1, m1, B, N):
    """__call__'s precomputed-embedding arguments from [negative; positive] halves: 8 text tokens, T5 states, mask"""
    return dict(prompt_embeds=ehs1[B:], negative_prompt_embeds=ehs1[:B], generated_prompt_embeds=ehs[B:, :8], negative_generated_prompt_embeds=ehs[:B, :8],
                attention_mask=m1[B:], negative_attention_mask=m1[:B], audio_length_in_s=1.04, num_inference_steps=N, output_type="latent",
                mel=torch.zeros(1, 1024, 128))


def test_call_assembles_three_branches(dev):
    """__call__(mel=, audio_guidance_scale=): the T5 states and mask go in as [neg; neg; pos], the generated tokens as
    assemble_condition(branches=3), and the result is denoise's on those tensors"""
    import ap_adapter_amd as A
    dtype = torch.bfloat16
    u, cfg, sd, procs = _small_unet(dev, dtype)
    u.requires_grad_(False)
    B, N, gs, ags = 2, 3, 7.5, 2.5
    ehs, ehs1, m1 = (t.to(dev) for t in _cond(2 * B, 32, dtype, seed=2))
    lat = R(B, 8, 26, 16, seed=3).to(dev)
    pipe = A.AudioLDM2Pipeline(u)
    tok, unc = _stub_audio(pipe, dev)
    out = pipe(latents=lat, guidance_scale=gs, audio_guidance_scale=ags, **_call_kw(ehs, ehs1, m1, B, N)).audios
    ge3 = pipe.assemble_condition(torch.cat([ehs[:B, :8], ehs[B:, :8]]), tok, unc, dtype, branches=3)
    assert ge3.shape == (3 * B, 40, 768) and torch.equal(ge3[:B, 8:], unc.to(dtype).expand(B, 32, 768)) and torch.equal(ge3[B:2 * B, :8], ge3[:B, :8])
    pe3, am3 = torch.cat([ehs1[:B], ehs1]), torch.cat([m1[:B], m1])
    assert torch.equal(out, pipe.denoise(lat, ge3, pe3, am3, N, gs, audio_guidance_scale=ags, use_graph=False))
    two = pipe(latents=lat, guidance_scale=gs, **_call_kw(ehs, ehs1, m1, B, N)).audios  # without the keyword: today's call
    ge2 = pipe.assemble_condition(torch.cat([ehs[:B, :8], ehs[B:, :8]]), tok, unc, dtype)
    assert torch.equal(two, pipe.denoise(lat, ge2, ehs1, m1, N, gs, use_graph=False)) and not torch.equal(two, out)


@pytest.mark.parametrize("sampler,eta", [("ddim", 0.0), ("dpm", 0.0), ("ddim", 0.5)])
def test_editing_with_three_branches(dev, sampler, eta):
    """source_latents, strength 0.5 and an edit_region with audio_guidance_scale: the kept region is the source bit for bit, captured ==
    eager, and the guidance table starts at row k like the coefficient table (the first k entries of the per-step sequence are NaN)"""
    import ap_adapter_amd as A
    dtype = torch.bfloat16
    u, cfg, sd, procs = _small_unet(dev, dtype)
    u.requires_grad_(False)
    B, H, W, N = 2, 26, 16, 8
    ehs, ehs1, m1 = (t.to(dev) for t in _cond(2 * B, 32, dtype, seed=2))
    x0 = R(B, 8, H, W, seed=70, std=0.7).to(dev)
    pipe = A.AudioLDM2Pipeline(u, scheduler=_sched(sampler))
    _stub_audio(pipe, dev)
    k = pipe.scheduler.edit_start_index(N, 0.5)
    assert k == 4
    nan = float("nan")
    ags = [nan] * k + GO.ramp(1.0, 4.0, N - k)
    gs = [nan] * k + GO.ramp(7.5, 3.0, N - k)
    g = lambda: torch.Generator().manual_seed(11)
    kw = dict(source_latents=x0, strength=0.5, edit_region=(0.2, 0.6), guidance_scale=gs, audio_guidance_scale=ags, eta=eta,
              **_call_kw(ehs, ehs1, m1, B, N))
    a = pipe(generator=g(), **kw).audios
    assert (pipe.graph_captures, pipe.graph_hits) == (1, 0) and bool(torch.isfinite(a).all())
    eager = pipe(generator=g(), use_graph=False, **kw).audios
    assert torch.equal(a, eager)
    rows = slice(5, 15)  # 0.2 s .. 0.6 s at 0.04 s per latent row
    kept = torch.ones(B, 8, H, W, dtype=torch.bool, device=dev)
    kept[:, :, rows] = False
    assert torch.equal(a[kept], x0[kept]) and not bool((a[~kept] == x0[~kept]).any())
    # a NaN inside the slice is rejected on the host; another schedule replays the captured step
    with pytest.raises(ValueError, match="^audio"):
        pipe(generator=g(), **{**kw, "audio_guidance_scale": [1.0] * (N - 1) + [nan]})
    b = pipe(generator=g(), **{**kw, "audio_guidance_scale": 0.5}).audios
    assert (pipe.graph_captures, pipe.graph_hits) == (1, 1) and not torch.equal(b, a) and torch.equal(b[kept], x0[kept])
    assert torch.equal(b, pipe(generator=g(), use_graph=False, **{**kw, "audio_guidance_scale": 0.5}).audios)


def test_three_branch_2m_loop_tracks_the_restatement_on_its_own_noise(dev, monkeypatch):
    """8 steps of DPM-Solver++ (2M), f16: the eager latents against a host loop that feeds the GPU's OWN guided noise of every step
    through the fp64 restatement -- the sampler isolated from the UNet's rounding.  Bound: the 3e-2 of
    test_dpm_2m_loop_captured_eager_replayed_and_vs_restatement at this dtype."""
    import ap_adapter_amd as A
    from ap_adapter_amd import ops
    dtype = torch.float16
    u, cfg, sd, procs = _small_unet(dev, dtype)
    u.requires_grad_(False)
    B, H, W, steps, gs, ags = 2, 26, 16, 8, 7.5, 2.5
    inp = _inputs3(dev, dtype, B=B)
    pipe = A.AudioLDM2Pipeline(u, scheduler=A.DPMSolverMultistepScheduler())
    preds, branches = [], []
    real = ops.cfg_dual_step

    def spy(eps3, lat, unet_in, coef, guidance, step_ptr, eps_out=None, history=None, noise=None, **kw):
        assert history is not None and noise is None and eps_out is not None and eps3.shape[0] == 3 * B
        real(eps3, lat, unet_in, coef, guidance, step_ptr, eps_out, history, noise, **kw)
        preds.append(eps_out.double().cpu())
        branches.append(eps3.float().cpu().reshape(3 * B, -1))

    monkeypatch.setattr(ops, "cfg_dual_step", spy)
    b = pipe.denoise(*inp, steps, gs, use_graph=False, keep_noise_pred=True, audio_guidance_scale=ags)
    monkeypatch.undo()
    assert len(preds) == steps and torch.equal(pipe.denoise(*inp, steps, gs, audio_guidance_scale=ags), b)
    # the recorded noise is the restated combine of the recorded branches
    for e, eps3 in zip(preds, branches):
        assert rel_err(e.reshape(B, -1), GO.cfg3_combine_rounded(eps3, ags, gs, dtype).float()) < 1e-6
    acp, ts = SO.acp64(), SO.grid(steps)
    x = inp[0].float().cpu().permute(0, 2, 3, 1).reshape(B, H * W, 8).double()
    m1 = None
    for i in range(steps):
        x, m1 = SO.dpm_step(x, preds[i], m1, i, ts, acp)
    ref = x.reshape(B, H, W, 8).permute(0, 3, 1, 2)
    err = rel_err(b, ref.float())
    print(f"\n[three-branch 2M loop, 8 steps, f16 small UNet] eager latents vs fp64 restatement on the GPU's own noise_pred: rel err {err:.3e}")
    assert err < 3e-2
