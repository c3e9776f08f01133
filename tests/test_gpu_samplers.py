"""-m gpu: the samplers of the captured denoise step -- apad_cfg_sampler_step against the fp64 restatement (tests/sampler_oracle.py),
the untouched default path, the DPM-Solver++ (2M) loop captured / eager / replayed, and DDIM with eta > 0 from pre-drawn noise."""
import pytest
import torch

from util import TOL, q, rel_err

import sampler_oracle as SO
from test_gpu_unet import _cond, _small_unet

pytestmark = pytest.mark.gpu


def R(*shape, seed=0, std=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * std


def _check_step(dtype, lat_d, unet_in, eps_out, lat, e):
    """the bounds test_cfg_ddim_step_matches_oracle applies to apad_cfg_ddim_step (the same arithmetic plus one or two multiply-adds)"""
    errs = rel_err(eps_out, e.float()), rel_err(lat_d, lat.float()), rel_err(unet_in, lat.float())
    assert errs[0] < 1e-6 and errs[1] < 1e-5 and errs[2] < TOL[dtype], errs
    return errs


@pytest.mark.parametrize("n", [4000 * 8, 4001])  # 16-byte accesses / the scalar form (B * n not a multiple of 8)
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32])
def test_cfg_sampler_step_2m_matches_restatement(dev, dtype, n):
    """every step of a 10-step DPM-Solver++ (2M) run (first-order first and -- lower_order_final -- last step, second order between)
    on random eps2: guided noise, fp32 master latents, model-dtype copy and the data-prediction history, step by step"""
    from ap_adapter_amd import ops
    from ap_adapter_amd.scheduler import DPMSolverMultistepScheduler
    B, steps, gs = 3, 10, 7.5
    s = DPMSolverMultistepScheduler()
    s.set_timesteps(steps)
    plan = s.sampler_plan()
    assert plan.needs_history and not plan.legacy
    coef = plan.table.to(dev)
    acp, ts = SO.acp64(), SO.grid(steps)
    lat = R(B, n, seed=44).double()
    lat_d = lat.float().to(dev)
    unet_in = torch.empty(B, n, dtype=dtype, device=dev)
    eps_out = torch.empty(B, n, dtype=torch.float32, device=dev)
    hist = torch.zeros(B, n, dtype=torch.float32, device=dev)
    step_ptr = torch.zeros(1, dtype=torch.int32, device=dev)
    m1, worst = None, [0.0, 0.0, 0.0, 0.0]
    for i in range(steps):
        eps2 = q(R(2 * B, n, seed=100 + i) * 0.5, dtype)
        e = SO.cfg_combine_rounded(eps2, gs, dtype)
        lat, m1 = SO.dpm_step(lat, e, m1, i, ts, acp)
        ops.cfg_sampler_step(eps2.to(dev, dtype), lat_d, unet_in, coef, step_ptr, gs, eps_out, hist)
        ops.step_advance(step_ptr)
        errs = _check_step(dtype, lat_d, unet_in, eps_out, lat, e) + (rel_err(hist, m1.float()),)
        assert errs[3] < 1e-5, errs  # m0 = d_x x + d_eps eps: the same two-term fp32 form as the latent update
        worst = [max(a, b) for a, b in zip(worst, errs)]
    print(f"\n[apad_cfg_sampler_step 2M, {dtype}, n={n}] worst rel err: eps {worst[0]:.2e} latents {worst[1]:.2e} unet_in {worst[2]:.2e} m0 {worst[3]:.2e}")
    assert int(step_ptr.item()) == steps


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32])
def test_cfg_sampler_step_from_a_random_history(dev, dtype):
    """three consecutive second-order steps entered mid-run (step counter 3 of 20) from random latents AND a random history buffer;
    eps_out omitted"""
    from ap_adapter_amd import ops
    from ap_adapter_amd.scheduler import DPMSolverMultistepScheduler
    B, n, steps, gs, first = 2, 1000 * 8, 20, 7.5, 3
    s = DPMSolverMultistepScheduler()
    s.set_timesteps(steps)
    coef = s.sampler_plan().table.to(dev)
    acp, ts = SO.acp64(), SO.grid(steps)
    lat, m1 = R(B, n, seed=1).double(), (R(B, n, seed=2) * 3.0).double()
    lat_d, hist = lat.float().to(dev), m1.float().to(dev)
    unet_in = torch.empty(B, n, dtype=dtype, device=dev)
    step_ptr = torch.full((1,), first, dtype=torch.int32, device=dev)
    for i in range(first, first + 3):
        eps2 = q(R(2 * B, n, seed=200 + i) * 0.5, dtype)
        lat, m1 = SO.dpm_step(lat, SO.cfg_combine_rounded(eps2, gs, dtype), m1, i, ts, acp)
        ops.cfg_sampler_step(eps2.to(dev, dtype), lat_d, unet_in, coef, step_ptr, gs, None, hist)
        ops.step_advance(step_ptr)
        assert rel_err(lat_d, lat.float()) < 1e-5 and rel_err(unet_in, lat.float()) < TOL[dtype] and rel_err(hist, m1.float()) < 1e-5


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32])
def test_cfg_sampler_step_ddim_eta_matches_restatement(dev, dtype):
    """DDIM with eta = 1 over 10 steps: row *step_ptr of the noise buffer is the one added; no history buffer"""
    from ap_adapter_amd import ops
    from ap_adapter_amd.scheduler import DDIMScheduler
    B, n, steps, gs = 3, 2000 * 8, 10, 7.5
    s = DDIMScheduler()
    s.set_timesteps(steps)
    plan = s.sampler_plan(1.0)
    assert plan.needs_noise and not plan.needs_history and not plan.legacy
    coef = plan.table.to(dev)
    acp, ts = SO.acp64(), SO.grid(steps)
    noise = R(steps, B, n, seed=9)
    noise_d = noise.to(dev)
    lat = R(B, n, seed=44).double()
    lat_d = lat.float().to(dev)
    unet_in = torch.empty(B, n, dtype=dtype, device=dev)
    eps_out = torch.empty(B, n, dtype=torch.float32, device=dev)
    step_ptr = torch.zeros(1, dtype=torch.int32, device=dev)
    for i in range(steps):
        eps2 = q(R(2 * B, n, seed=100 + i) * 0.5, dtype)
        e = SO.cfg_combine_rounded(eps2, gs, dtype)
        lat = SO.ddim_step(lat, e, noise[i], i, ts, acp, eta=1.0)
        ops.cfg_sampler_step(eps2.to(dev, dtype), lat_d, unet_in, coef, step_ptr, gs, eps_out, None, noise_d)
        ops.step_advance(step_ptr)
        _check_step(dtype, lat_d, unet_in, eps_out, lat, e)
    # one step with eps = 0 from step counter 4: x' - c_x x is std_4 * z[4]
    step_ptr.fill_(4)
    x = R(B, n, seed=5)
    lat_d = x.to(dev)
    ops.cfg_sampler_step(torch.zeros(2 * B, n, dtype=dtype, device=dev), lat_d, unet_in, coef, step_ptr, gs, None, None, noise_d)
    c_x, std = float(plan.table[4, 0]), float(plan.table[4, 3])
    got = lat_d.cpu().double() - c_x * x.double()
    assert rel_err(got, (std * noise[4].double())) < 1e-5 and rel_err(got, std * noise[3].double()) > 0.5


def test_cfg_sampler_step_rejects_bad_operands(dev):
    from ap_adapter_amd import ops
    lat = torch.zeros(2, 64, device=dev)
    eps2 = torch.zeros(4, 64, dtype=torch.bfloat16, device=dev)
    unet_in = torch.zeros(2, 64, dtype=torch.bfloat16, device=dev)
    ptr = torch.zeros(1, dtype=torch.int32, device=dev)
    with pytest.raises(RuntimeError, match=r"\[steps, 6\]"):
        ops.cfg_sampler_step(eps2, lat, unet_in, torch.zeros(5, 2, device=dev), ptr, 7.5)
    with pytest.raises(RuntimeError, match="noise"):
        ops.cfg_sampler_step(eps2, lat, unet_in, torch.zeros(5, 6, device=dev), ptr, 7.5, noise=torch.zeros(4, 2, 64, device=dev))
    with pytest.raises(RuntimeError, match="history"):
        ops.cfg_sampler_step(eps2, lat, unet_in, torch.zeros(5, 6, device=dev), ptr, 7.5, history=torch.zeros(2, 32, device=dev))
    # a step counter beyond the table reads its last row, not past it
    ptr.fill_(1000)
    coef = torch.zeros(5, 6, device=dev)
    coef[4, 0] = 2.0
    lat.fill_(1.5)
    ops.cfg_sampler_step(eps2, lat, unet_in, coef, ptr, 7.5)
    assert bool((lat == 3.0).all())


def _inputs(dev, dtype, B=2, H=26, W=16, seed=2):
    lat = torch.randn(B, 8, H, W, generator=torch.Generator().manual_seed(seed))
    ehs, ehs1, m1 = _cond(2 * B, 32, dtype, seed=seed)
    return lat.to(dev), ehs.to(dev), ehs1.to(dev), m1.to(dev)


def _count(monkeypatch, names):
    from ap_adapter_amd import ops
    calls = {n: [] for n in names}
    for n in names:
        real = getattr(ops, n)
        monkeypatch.setattr(ops, n, (lambda real_, n_: lambda *a, **kw: (calls[n_].append(1), real_(*a, **kw))[1])(real, n))
    return calls


def test_default_path_still_launches_cfg_ddim_step_bit_for_bit(dev, monkeypatch):
    """DDIMScheduler, eta = 0 (every earlier caller): the loop launches apad_cfg_ddim_step from the two-column table, never the new entry
    point, and the latents after 3 steps are the bits of a hand-driven loop over ops.cfg_ddim_step"""
    import ap_adapter_amd as A
    from ap_adapter_amd import ops
    dtype = torch.bfloat16
    u, cfg, sd, procs = _small_unet(dev, dtype)
    u.requires_grad_(False)
    B, H, W, steps, gs = 2, 26, 16, 3, 7.5
    lat, ehs, ehs1, m1 = _inputs(dev, dtype)
    pipe = A.AudioLDM2Pipeline(u)
    calls = _count(monkeypatch, ("cfg_ddim_step", "cfg_sampler_step"))
    eager = pipe.denoise(lat, ehs, ehs1, m1, steps, gs, use_graph=False)
    assert (len(calls["cfg_ddim_step"]), len(calls["cfg_sampler_step"])) == (steps, 0)
    graph = pipe.denoise(lat, ehs, ehs1, m1, steps, gs)
    explicit = pipe.denoise(lat, ehs, ehs1, m1, steps, gs, eta=0.0, generator=torch.Generator().manual_seed(1))
    assert len(calls["cfg_sampler_step"]) == 0 and (pipe.graph_captures, pipe.graph_hits) == (1, 1)
    monkeypatch.undo()
    # by hand, as bench.py and tools/ drive the step
    sched = A.DDIMScheduler()
    sched.set_timesteps(steps)
    coef = sched.coef_table().to(dev)
    step_ptr = torch.zeros(1, dtype=torch.int32, device=dev)
    x = lat.float().permute(0, 2, 3, 1).reshape(B, H * W, 8).contiguous()
    unet_in = x.to(dtype)
    with torch.no_grad():
        u.set_kv_cache(True)
        u.precompute_time_tables(sched.timesteps.to(dev), step_ptr)
        try:
            for _ in range(steps):
                eps2 = u.forward_nhwc(unet_in, H, W, None, ehs.to(dtype), ehs1.to(dtype), None, m1, batch_repeat=2)
                ops.cfg_ddim_step(eps2, x, unet_in, coef, step_ptr, gs)
                ops.step_advance(step_ptr)
        finally:
            u.clear_time_tables()
            u.set_kv_cache(False)
    ref = x.reshape(B, H, W, 8).permute(0, 3, 1, 2)
    assert torch.equal(eager, ref) and torch.equal(graph, ref) and torch.equal(explicit, ref)


def test_dpm_2m_loop_captured_eager_replayed_and_vs_restatement(dev, monkeypatch):
    """8 steps of DPM-Solver++ (2M) on the small synthetic UNet (f16): the captured loop equals the eager loop bit for bit; a replay on
    new latents / conditions equals a fresh capture bit for bit (the history buffer is zeroed, nothing of the previous clip survives);
    and the eager latents track a host loop that feeds the GPU UNet's OWN guided noise_pred of every step through the fp64 restatement
    -- which isolates the sampler from UNet rounding.  Bound: the 3e-2 that test_small_unet_graph_loop_vs_oracle_loop applies to the DDIM
    loop at this dtype."""
    import ap_adapter_amd as A
    from ap_adapter_amd import ops
    dtype = torch.float16
    u, cfg, sd, procs = _small_unet(dev, dtype)
    u.requires_grad_(False)
    B, H, W, steps, gs = 2, 26, 16, 8, 7.5
    pipe = A.AudioLDM2Pipeline(u, scheduler=A.DPMSolverMultistepScheduler())
    in1, in2 = _inputs(dev, dtype, seed=2), _inputs(dev, dtype, seed=3)
    a = pipe.denoise(*in1, steps, gs)
    assert (pipe.graph_captures, pipe.graph_hits) == (1, 0)
    # eager, recording the guided noise the update kernel consumed at every step
    preds = []
    real = ops.cfg_sampler_step

    def spy(eps2, lat, unet_in, coef, step_ptr, g, eps_out=None, history=None, noise=None):
        assert history is not None and noise is None and eps_out is not None
        real(eps2, lat, unet_in, coef, step_ptr, g, eps_out, history, noise)
        preds.append(eps_out.double().cpu())

    monkeypatch.setattr(ops, "cfg_sampler_step", spy)
    b = pipe.denoise(*in1, steps, gs, use_graph=False, keep_noise_pred=True)
    monkeypatch.undo()
    assert len(preds) == steps and torch.equal(a, b)
    seen = []
    c = pipe.denoise(*in1, steps, gs, callback=lambda i, t, x: seen.append((i, t)), callback_steps=2)  # the callback (eager) path
    assert torch.equal(c, a) and seen == [(i, SO.grid(steps)[i]) for i in range(0, steps, 2)]
    # replay on another clip == fresh capture; and back
    a2 = pipe.denoise(*in2, steps, gs)
    assert (pipe.graph_captures, pipe.graph_hits) == (1, 1) and not torch.equal(a2, a)
    fresh = A.AudioLDM2Pipeline(u, scheduler=A.DPMSolverMultistepScheduler())
    assert torch.equal(fresh.denoise(*in2, steps, gs), a2)
    assert torch.equal(pipe.denoise(*in1, steps, gs), a) and pipe.graph_hits == 2
    # the sampler is part of the cache key: the same pipeline with DDIM captures again and gives DDIM's latents
    pipe.scheduler = A.DDIMScheduler()
    d = pipe.denoise(*in1, steps, gs)
    assert pipe.graph_captures == 2 and not torch.equal(d, a)
    assert torch.equal(d, A.AudioLDM2Pipeline(u).denoise(*in1, steps, gs, use_graph=False))
    # host loop through the restatement
    acp, ts = SO.acp64(), SO.grid(steps)
    x = in1[0].float().cpu().permute(0, 2, 3, 1).reshape(B, H * W, 8).double()
    m1 = None
    for i in range(steps):
        x, m1 = SO.dpm_step(x, preds[i], m1, i, ts, acp)
    ref = x.reshape(B, H, W, 8).permute(0, 3, 1, 2)
    err = rel_err(b, ref.float())
    print(f"\n[2M loop, 8 steps, f16 small UNet] eager latents vs fp64 restatement on the GPU's own noise_pred: rel err {err:.3e}")
    assert err < 3e-2


def test_stochastic_ddim_eta1_is_reproducible_from_a_cpu_generator(dev):
    """eta = 1: the same CPU seed gives the same bits, captured (first capture AND a replay, whose noise buffer is refilled in place) or
    eager; another seed and eta = 0 differ; __call__ draws the initial latents and then the per-step noise from the one generator"""
    import ap_adapter_amd as A
    dtype = torch.bfloat16
    u, cfg, sd, procs = _small_unet(dev, dtype)
    u.requires_grad_(False)
    steps, gs = 4, 7.5
    pipe = A.AudioLDM2Pipeline(u)
    inp = _inputs(dev, dtype)
    g = lambda seed: torch.Generator().manual_seed(seed)
    a = pipe.denoise(*inp, steps, gs, eta=1.0, generator=g(5))
    other = pipe.denoise(*inp, steps, gs, eta=1.0, generator=g(6))
    again = pipe.denoise(*inp, steps, gs, eta=1.0, generator=g(5))
    assert (pipe.graph_captures, pipe.graph_hits) == (1, 2)
    eager = pipe.denoise(*inp, steps, gs, eta=1.0, generator=g(5), use_graph=False)
    det = pipe.denoise(*inp, steps, gs)
    assert torch.equal(a, again) and torch.equal(a, eager) and not torch.equal(a, other) and not torch.equal(a, det)
    assert pipe.graph_captures == 2  # eta is part of the key
    assert bool(torch.isfinite(a).all())
    # the multistep scheduler ignores eta (and draws nothing from the generator)
    pm = A.AudioLDM2Pipeline(u, scheduler=A.DPMSolverMultistepScheduler())
    gen = g(7)
    state = gen.get_state()
    m_a = pm.denoise(*inp, steps, gs, eta=1.0, generator=gen)
    assert torch.equal(gen.get_state(), state) and torch.equal(m_a, pm.denoise(*inp, steps, gs)) and pm.graph_captures == 1
    # __call__: latents, then steps x noise, from one generator
    B = 2
    ge, pe, mask = inp[1], inp[2], inp[3]
    kw = dict(prompt_embeds=pe[B:], negative_prompt_embeds=pe[:B], generated_prompt_embeds=ge[B:], negative_generated_prompt_embeds=ge[:B],
              attention_mask=mask[B:], negative_attention_mask=mask[:B], audio_length_in_s=1.04, num_inference_steps=steps, guidance_scale=gs,
              output_type="latent")
    out = pipe(eta=1.0, generator=g(11), **kw).audios
    g2 = g(11)
    lat = pipe.prepare_latents(B, 8, 104, dtype, dev, g2)
    assert lat.shape == (B, 8, 26, 16)
    assert torch.equal(out, pipe.denoise(lat, ge, pe, mask, steps, gs, eta=1.0, generator=g2, use_graph=False))
