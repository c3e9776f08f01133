"""CPU: the denoise loop's samplers -- DPMSolverMultistepScheduler (DPM-Solver++ 2M) and DDIMScheduler with eta > 0 -- as host
arithmetic: their device coefficient tables against the independent fp64 restatement (tests/sampler_oracle.py), the timestep grid,
an analytic ODE, the order of the pre-drawn noise, and the public surface.  No GPU compute."""
import os
import re

import pytest
import torch

import ap_adapter_amd as A
from ap_adapter_amd import _lib as L
from ap_adapter_amd.scheduler import SAMPLER_COLS

import sampler_oracle as SO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = [10, 14, 15, 20, 50, 200]  # 14 / 15 straddle the lower_order_final switch


def _apply_rows(rows, x, eps_seq, noise=None):
    """the update the kernel performs, in float64: x' = c_x x + c_eps eps + c_m1 m1 + c_z z;  m0 = d_x x + d_eps eps"""
    assert rows.dtype == torch.float64 and rows.shape[1] == len(SAMPLER_COLS) == 6
    x = x.double()
    m1 = torch.zeros_like(x)
    for i, r in enumerate(rows.tolist()):
        e = eps_seq[i].double()
        z = torch.zeros_like(x) if noise is None else noise[i].double()
        m0 = r[4] * x + r[5] * e
        x = r[0] * x + r[1] * e + r[2] * m1 + r[3] * z
        m1 = m0
    return x


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max())


def _seq(n, seed, shape=(64,)):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g, dtype=torch.float64), [torch.randn(shape, generator=g, dtype=torch.float64) for _ in range(n)]


@pytest.mark.parametrize("n", STEPS)
@pytest.mark.parametrize("order,lof", [(2, True), (2, False), (1, True)])
def test_dpm_table_matches_the_restatement(n, order, lof):
    s = A.DPMSolverMultistepScheduler(solver_order=order, lower_order_final=lof)
    s.set_timesteps(n)
    rows = s.sampler_rows()
    acp, ts = SO.acp64(), SO.grid(n)
    x, eps = _seq(n, 7 + n)
    ref = SO.dpm_loop(x, lambda i, t, x_: eps[i], ts, acp, solver_order=order, lower_order_final=lof)
    err = _rel(_apply_rows(rows, x, eps), ref)
    print(f"\n[2M table vs restatement, N={n}, order={order}, lower_order_final={lof}] rel err {err:.3e}")
    assert err <= 1e-12
    # both sides of the switch are really exercised: the last row is first order (no m1 term) exactly when it applies
    last_first_order = order == 1 or (lof and n < 15)
    assert (float(rows[-1, 2]) == 0.0) == last_first_order
    if order == 2:
        assert all(float(c) != 0.0 for c in rows[1:-1, 2]) and float(rows[0, 2]) == 0.0
    # the exported device table is these rows in fp32; no noise column
    plan = s.sampler_plan()
    assert plan.table.dtype == torch.float32 and torch.equal(plan.table, rows.float()) and not plan.legacy and not plan.needs_noise
    assert plan.needs_history == (order == 2) and float(rows[:, 3].abs().max()) == 0.0


@pytest.mark.parametrize("n", STEPS)
def test_dpm_first_order_is_ddim(n):
    """an identity of the two formulas: DPM-Solver++ of order 1 is deterministic DDIM"""
    s = A.DPMSolverMultistepScheduler(solver_order=1)
    s.set_timesteps(n)
    d = A.DDIMScheduler()
    d.set_timesteps(n)
    x, eps = _seq(n, 90 + n)
    acp, ts = SO.acp64(), SO.grid(n)
    ref = SO.ddim_loop(x, lambda i, t, x_: eps[i], ts, acp)
    assert _rel(_apply_rows(s.sampler_rows(), x, eps), ref) <= 1e-12
    assert _rel(_apply_rows(d.sampler_rows(0.0), x, eps), ref) <= 1e-12
    assert _rel(SO.dpm_loop(x, lambda i, t, x_: eps[i], ts, acp, solver_order=1), ref) <= 1e-12


def test_injected_grid():
    """the table builder takes the timestep list as an argument"""
    s = A.DPMSolverMultistepScheduler()
    ts = [901, 700, 420, 333, 100, 7]
    acp = SO.acp64()
    x, eps = _seq(len(ts), 3)
    ref = SO.dpm_loop(x, lambda i, t, x_: eps[i], ts, acp)
    assert _rel(_apply_rows(s.sampler_rows(timesteps=ts), x, eps), ref) <= 1e-12


@pytest.mark.parametrize("n", STEPS + [100])
def test_timesteps_are_ddims_grid(n):
    s, d = A.DPMSolverMultistepScheduler(), A.DDIMScheduler()
    s.set_timesteps(n)
    d.set_timesteps(n)
    assert torch.equal(s.timesteps, d.timesteps)
    ratio = 1000 // n
    assert s.timesteps.tolist() == [i * ratio + 1 for i in range(n - 1, -1, -1)]
    assert s.num_inference_steps == n and s.init_noise_sigma == 1.0 and s.order == 1 and s.solver_order == 2
    assert s.scale_model_input(x := torch.ones(2)) is x
    assert torch.equal(s.alphas_cumprod, d.alphas_cumprod)


def test_analytic_gaussian_problem_2m_beats_ddim():
    """data x0 ~ N(0, 0.5^2): the exact eps is linear in x and the probability-flow ODE has a closed form.  On DDIM's own grid, at every
    N the 2M sampler's end-point error at t = 0 is strictly below DDIM's (no convergence order is asserted: with leading spacing the
    last interval into t = 0 dominates)."""
    s_data, acp = 0.5, SO.acp64()
    x_T = torch.ones(1, dtype=torch.float64)
    for n in (10, 20, 50, 100, 200):
        ts = SO.grid(n)
        exact = SO.gaussian_ode_solution(1.0, ts[0], 0, acp, s_data)
        fn = SO.gaussian_eps(acp, s_data)
        e_ddim = abs(float(SO.ddim_loop(x_T, fn, ts, acp)) - exact)
        e_2m = abs(float(SO.dpm_loop(x_T, fn, ts, acp)) - exact)
        # ... and through the scheduler's own table
        sch = A.DPMSolverMultistepScheduler()
        sch.set_timesteps(n)
        x = x_T.clone()
        m1 = torch.zeros_like(x)
        for i, r in enumerate(sch.sampler_rows().tolist()):
            e = fn(i, ts[i], x)
            x, m1 = r[0] * x + r[1] * e + r[2] * m1, r[4] * x + r[5] * e
        e_tab = abs(float(x) - exact)
        print(f"\n[gaussian ODE, N={n}] |err| DDIM {e_ddim:.3e}  2M {e_2m:.3e} (table {e_tab:.3e})  ratio {e_ddim / e_2m:.2f}")
        assert e_2m < e_ddim and e_tab < e_ddim


@pytest.mark.parametrize("n", [10, 50, 200])
def test_ddim_eta_rows(n):
    d = A.DDIMScheduler()
    d.set_timesteps(n)
    # eta = 0 reproduces coef_table() exactly, and is the path that keeps apad_cfg_ddim_step
    r0 = d.sampler_rows(0.0)
    assert torch.equal(r0[:, :2].float(), d.coef_table()) and float(r0[:, 2:].abs().max()) == 0.0
    p0 = d.sampler_plan(0.0)
    assert p0.legacy and torch.equal(p0.table, d.coef_table()) and not p0.needs_noise and not p0.needs_history
    # eta = 1: the direction coefficient c_dir = sqrt(1 - a_prev - std^2) (recovered from c_eps = c_dir - c_x sqrt(1 - a_t))
    r1 = d.sampler_rows(1.0)
    acp, ts = SO.acp64(), SO.grid(n)
    for i, t in enumerate(ts):
        p = t - 1000 // n
        a_p = acp[p] if p >= 0 else acp[0]
        c_x, c_e, std = float(r1[i, 0]), float(r1[i, 1]), float(r1[i, 3])
        c_dir = c_e + c_x * (1.0 - acp[t]) ** 0.5
        assert std > 0.0
        assert abs(c_dir ** 2 + std ** 2 - (1.0 - a_p)) <= 1e-12 * (1.0 - a_p)
    p1 = d.sampler_plan(1.0)
    assert not p1.legacy and p1.needs_noise and not p1.needs_history and torch.equal(p1.table, r1.float()) and p1.key != p0.key
    # ... and the rows against the restatement, noise included
    for eta in (0.3, 1.0):
        x, eps = _seq(n, 11 + n)
        _, noise = _seq(n, 500 + n)
        ref = SO.ddim_loop(x, lambda i, t, x_: eps[i], ts, acp, eta=eta, noise=noise)
        assert _rel(_apply_rows(d.sampler_rows(eta), x, eps, noise), ref) <= 1e-12


def test_step_noise_is_drawn_in_the_references_order():
    """one randn of the latent shape per step from the caller's generator, after the initial latents"""
    pipe = A.AudioLDM2Pipeline(None)
    B, C, height, steps = 2, 8, 48, 5
    g = torch.Generator().manual_seed(1234)
    lat = pipe.prepare_latents(B, C, height, torch.float32, "cpu", g)
    H, W = lat.shape[2:]
    noise = pipe.prepare_step_noise(B, C, H, W, steps, g)
    g2 = torch.Generator().manual_seed(1234)
    assert torch.equal(lat, torch.randn(B, C, H, W, generator=g2))
    assert noise.shape == (steps, B, H * W, C) and noise.dtype == torch.float32
    for i in range(steps):
        z = torch.randn(B, C, H, W, generator=g2)
        assert torch.equal(noise[i].reshape(B, H, W, C).permute(0, 3, 1, 2), z), i
    # refilled in place for a replay
    again = pipe.prepare_step_noise(B, C, H, W, steps, torch.Generator().manual_seed(99), out=noise)
    assert again is noise and torch.equal(noise[0].reshape(B, H, W, C).permute(0, 3, 1, 2), torch.randn(B, C, H, W, generator=torch.Generator().manual_seed(99)))


def test_call_accepts_eta_and_either_scheduler():
    u = A.AudioLDM2UNet2DConditionModel(A.UNetConfig(block_out_channels=(64, 128, 192, 256), attention_head_dim=4, norm_num_groups=16))
    e = torch.zeros(1, 16, 1024)
    for sched in (None, A.DDIMScheduler(), A.DPMSolverMultistepScheduler()):
        pipe = A.AudioLDM2Pipeline(u, scheduler=sched)
        assert isinstance(pipe.scheduler, type(sched) if sched is not None else A.DDIMScheduler)
        # eta is no longer refused: the call gets as far as the next argument check
        with pytest.raises(ValueError, match="required"):
            pipe(prompt_embeds=e, output_type="latent", eta=0.5)
    # the multistep scheduler ignores eta (prepare_extra_step_kwargs), DDIM keys its captured step on it
    m = A.DPMSolverMultistepScheduler()
    m.set_timesteps(8)
    assert m.sampler_plan(0.0).key == m.sampler_plan(0.7).key and torch.equal(m.sampler_plan(0.7).table, m.sampler_plan(0.0).table)
    m1, d = A.DPMSolverMultistepScheduler(solver_order=1), A.DDIMScheduler()
    m1.set_timesteps(8)
    d.set_timesteps(8)
    assert len({m.sampler_plan().key, m1.sampler_plan().key, d.sampler_plan(0.0).key, d.sampler_plan(0.5).key}) == 4


@pytest.mark.parametrize("kw,name", [(dict(algorithm_type="dpmsolver"), "algorithm_type"), (dict(algorithm_type="sde-dpmsolver++"), "algorithm_type"),
                                     (dict(solver_type="heun"), "solver_type"), (dict(timestep_spacing="trailing"), "timestep_spacing"),
                                     (dict(timestep_spacing="linspace"), "timestep_spacing"), (dict(solver_order=3), "solver_order"),
                                     (dict(use_karras_sigmas=True), "use_karras_sigmas"), (dict(thresholding=True), "thresholding"),
                                     (dict(prediction_type="v_prediction"), "prediction_type")])
def test_unsupported_scheduler_options_raise_and_name_the_option(kw, name):
    with pytest.raises(NotImplementedError, match=name):
        A.DPMSolverMultistepScheduler(**kw)


def test_abi_declares_the_sampler_step():
    header = open(os.path.join(ROOT, "include", "apadapter_hip.h")).read()
    assert re.search(r"#define APAD_ABI_VERSION 12\b", header)
    assert re.search(r"\bint apad_cfg_sampler_step\s*\(", header)
    assert "apad_cfg_sampler_step" in header.split("#ifndef APADAPTER_HIP_H")[0]  # the index comment
    assert "apad_cfg_sampler_step" in L.SYMBOLS and len(L.SYMBOLS["apad_cfg_sampler_step"][1]) == 14
    assert re.search(r"\bint apad_cfg_ddim_step\s*\(", header) and len(L.SYMBOLS["apad_cfg_ddim_step"][1]) == 11  # untouched
    if os.path.exists(L.LIB_PATH):
        assert A.lib().apad_abi_version() == 12
        assert hasattr(A.lib(), "apad_cfg_sampler_step")
