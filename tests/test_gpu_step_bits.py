"""-m gpu: the bits of the step kernel behind apad_cfg_ddim_step / apad_cfg_sampler_step / apad_cfg_edit_step / apad_cfg_dual_step.

1. Against tests/golden/step_bits.safetensors: what the three separately compiled kernels of the commit before the merge wrote, recorded
   on the device by tests/golden/make_step_bits.py (whose CASES and run_case this module runs again).  torch.equal, every buffer, every case.
   Against tests/golden/step_bits_dual.safetensors (DUAL_CASES): what the three-branch kernel wrote while it was a copy of its own.
2. Against a host restatement of each rounding form spelled in csrc/elementwise.hip's sampler_update and guided_noise (fp32 instantiations):
   fp32 products and sums, each rounded once, from test_gpu_edit._fma32.  This pins the comment beside each form to what the kernel does."""
import os

import pytest
import torch
from safetensors.torch import load_file

import make_step_bits as MS
from test_gpu_edit import R, _fma32

pytestmark = pytest.mark.gpu

GOLD = load_file(MS.FIXTURE)
GOLD_DUAL = load_file(MS.FIXTURE_DUAL)


def test_fixture_covers_every_case_and_nothing_else():
    for cases, gold, path in ((MS.CASES, GOLD, MS.FIXTURE), (MS.DUAL_CASES, GOLD_DUAL, MS.FIXTURE_DUAL)):
        keys = {MS.fixture_key(c) + "." + b for c in cases for b in ("latents", "unet_in", "eps_out")}
        keys |= {MS.fixture_key(c) + ".history" for c in cases if c[1] == "dpm"}
        assert keys == set(gold) and os.path.getsize(path) < 1 << 20, path


def _assert_recorded(case, gold, dev):
    out = MS.run_case(case, dev)
    assert set(out) == {"latents", "unet_in", "eps_out"} | ({"history"} if case[1] == "dpm" else set())
    for name, t in out.items():
        g = gold[MS.fixture_key(case) + "." + name]
        assert t.dtype == g.dtype and torch.equal(t.cpu(), g), (case, name)


@pytest.mark.parametrize("case", MS.CASES, ids=lambda c: "-".join(c))
def test_step_bits_are_the_recorded_ones(dev, case):
    _assert_recorded(case, GOLD, dev)


@pytest.mark.parametrize("case", MS.DUAL_CASES, ids=lambda c: "-".join(c))
def test_dual_step_bits_are_the_recorded_ones(dev, case):
    _assert_recorded(case, GOLD_DUAL, dev)


# ---- the spelled forms, restated on the host ----
def _mul32(a, x):
    return (a * x.double()).float()  # the product of two fp32 values is exact in float64: one rounding


def _add32(x, y):
    return _fma32(1.0, x, y)


def _eps32(eps2, gs, B):
    """fp32: eps = fma(g, e_c - e_u, e_u), the difference rounded first"""
    eu, ec = eps2[:B], eps2[B:]
    return _fma32(gs, _fma32(-1.0, eu, ec), eu)


def _eps32_dual(eps3, s_a, s_t, B):
    """fp32: eps = fma(s_T, e_AT - e_A, fma(s_A, e_A - e_0, e_0)), each difference rounded first"""
    e0, ea, eat = eps3[:B], eps3[B:2 * B], eps3[2 * B:]
    return _fma32(s_t, _fma32(-1.0, ea, eat), _fma32(s_a, _fma32(-1.0, e0, ea), e0))


def _forms(form, r, x, e, m1, z):
    """(x', m0) of sampler_update's fp32 instantiations, as its comment states them"""
    c_x, c_e, c_m, c_z, d_x, d_e = r
    if form == "vec":
        return (_fma32(c_z, z, _fma32(c_m, m1, _fma32(c_x, x, _mul32(c_e, e)))), _fma32(d_x, x, _mul32(d_e, e)))
    return (_fma32(c_z, z, _fma32(c_m, m1, _fma32(c_e, e, _mul32(c_x, x)))), _add32(_mul32(d_x, x), _mul32(d_e, e)))


@pytest.mark.parametrize("form,npix,C", [("vec", 4000, 8), ("scalar", 4001, 4)])
@pytest.mark.parametrize("sampler,eta", [("dpm", 0.0), ("ddim", 0.5)])
def test_fp32_sampler_forms_match_their_host_restatement(dev, sampler, eta, form, npix, C):
    """apad_cfg_sampler_step, fp32, the 16-byte and the scalar form, every step of a 10-step slice.  A term whose coefficient is 0 is not read
    by the kernel and enters as fma(0, 0, .), which the restatement performs too (m1 = z = 0 there)."""
    from ap_adapter_amd import ops
    from test_gpu_edit import _plan
    B, N, k, gs = 3, 14, 4, 7.5
    n = npix * C
    assert (B * n % 8 == 0) == (form == "vec")
    sched, plan = _plan(sampler, eta, N, k)
    coef = plan.table.to(dev)
    noise = R(N - k, B, n, seed=9) if eta else None
    lat = R(B, n, seed=44)
    hist = torch.zeros(B, n) if plan.needs_history else None
    lat_d, unet_in, eps_out = lat.to(dev), torch.empty(B, n, device=dev), torch.empty(B, n, device=dev)
    hist_d = None if hist is None else hist.to(dev)
    noise_d = None if noise is None else noise.to(dev)
    ptr = torch.zeros(1, dtype=torch.int32, device=dev)
    zero = torch.zeros(B, n)
    for i in range(N - k):
        eps2 = R(2 * B, n, seed=100 + i) * 0.5
        r = [float(v) for v in plan.table[i]]
        e = _eps32(eps2, gs, B)
        m1 = hist if hist is not None and r[2] != 0.0 else zero
        z = noise[i] if noise is not None and r[3] != 0.0 else zero
        lat, m0 = _forms(form, r, lat, e, m1, z)
        if hist is not None:
            hist = m0
        ops.cfg_sampler_step(eps2.to(dev), lat_d, unet_in, coef, ptr, gs, eps_out, hist_d, noise_d)
        ops.step_advance(ptr)
        assert torch.equal(eps_out.cpu(), e) and torch.equal(lat_d.cpu(), lat) and torch.equal(unet_in.cpu(), lat), i
        assert hist is None or torch.equal(hist_d.cpu(), hist), i


def test_fp32_cfg_ddim_form_matches_its_host_restatement(dev):
    """apad_cfg_ddim_step, fp32: x' = fma(c_x, x, c_e * eps)"""
    import ap_adapter_amd as A
    from ap_adapter_amd import ops
    B, N, gs, n = 3, 10, 7.5, 4001 * 8
    sched = A.DDIMScheduler()
    sched.set_timesteps(N)
    table = sched.coef_table()
    coef = table.to(dev)
    lat = R(B, n, seed=44)
    lat_d, unet_in, eps_out = lat.to(dev), torch.empty(B, n, device=dev), torch.empty(B, n, device=dev)
    ptr = torch.zeros(1, dtype=torch.int32, device=dev)
    for i in range(N):
        eps2 = R(2 * B, n, seed=100 + i) * 0.5
        e = _eps32(eps2, gs, B)
        lat = _fma32(float(table[i, 0]), lat, _mul32(float(table[i, 1]), e))
        ops.cfg_ddim_step(eps2.to(dev), lat_d, unet_in, coef, ptr, gs, eps_out)
        ops.step_advance(ptr)
        assert torch.equal(eps_out.cpu(), e) and torch.equal(lat_d.cpu(), lat) and torch.equal(unet_in.cpu(), lat), i


@pytest.mark.parametrize("form,npix,C", [("vec", 17, 8), ("scalar", 17, 4)])
def test_fp32_dual_guided_noise_matches_its_host_restatement(dev, form, npix, C):
    """apad_cfg_dual_step, fp32, the 16-byte and the scalar form, every step of a 10-step slice with a guidance table that differs on every row:
    eps_out against guided_noise's three-branch formula"""
    from ap_adapter_amd import ops
    from ap_adapter_amd.scheduler import guidance_table
    from test_gpu_edit import _plan
    B, N, k = 3, 14, 4
    n = npix * C
    assert (B * n % 8 == 0) == (form == "vec")
    coef = _plan("dpm", 0.0, N, k)[1].table.to(dev)
    gtab = guidance_table(*MS.GUIDANCE, N, k)
    gtab_d = gtab.to(dev)
    lat, unet_in, eps_out, hist = R(B, n, seed=44).to(dev), torch.empty(B, n, device=dev), torch.empty(B, n, device=dev), torch.zeros(B, n, device=dev)
    ptr = torch.zeros(1, dtype=torch.int32, device=dev)
    for i in range(N - k):
        eps3 = R(3 * B, n, seed=100 + i) * 0.5
        ops.cfg_dual_step(eps3.to(dev), lat, unet_in, coef, gtab_d, ptr, eps_out, hist)
        ops.step_advance(ptr)
        assert torch.equal(eps_out.cpu(), _eps32_dual(eps3, float(gtab[i, 0]), float(gtab[i, 1]), B)), i
