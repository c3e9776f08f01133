"""-m gpu: edit-friendly DDPM inversion -- apad_cfg_invert_step against the fp64 restatement (tests/invert_oracle.py) with derived bounds,
the two-kernel round trip the feature rests on (invert, then the sampler step with noise = z, retraces every x_(i+1)), the grid-stride wrap,
a zero-std row, bad operands, and the pipeline on the small synthetic UNet: invert + denoise returns the source, captured / eager / replayed,
another condition edits, a mask keeps, three branches, and a default call reaches none of it.  PARITY UNPINNED (see invert_oracle).

The measured round-trip errors are printed; with APAD_INVERT_PROFILE=<path> they are also written there as JSON (profiles/invert_roundtrip.json
is such a run)."""
import json
import os

import pytest
import torch

from util import nan_buffer, q, rel_err

import guidance_oracle as GO
import invert_oracle as IO
import sampler_oracle as SO
from test_gpu_dual_guidance import _inputs3
from test_gpu_edit import _fma32
from test_gpu_samplers import _count, _inputs
from test_gpu_unet import _small_unet

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float16, torch.float32]
# (B, pixels, C, offset in floats of every fp32 operand): the 16-byte form; the scalar form (8 does not divide 63); one vector; 8 | total but
# every fp32 base 4 bytes past a 16-byte boundary, so the scalar form is taken at a size the 16-byte form would accept
GEOMS = {"vec": (2, 5, 8, 0), "scalar": (3, 7, 3, 0), "one-vector": (1, 1, 8, 0), "offset": (2, 4, 8, 1)}
G = 64  # guard elements on either side of a buffer (a multiple of 16 bytes in every dtype: the guard does not move the alignment)
MEASURED = {}


def R(*shape, seed=0, std=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * std


def _f32(v):
    return float(torch.tensor(float(v), dtype=torch.float32))


def _band(values, dev, dtype=torch.float32, off=0):
    """(view, check): ``values`` (or, given a size, the NaN pattern) as a contiguous view ``off`` elements past a 16-byte boundary, inside one
    NaN-patterned allocation with G guard elements on either side; check() asserts that nothing outside the view changed and that every
    element inside is finite (an unwritten output element still reads NaN)"""
    n = values if isinstance(values, int) else values.numel()
    buf = nan_buffer(G + off + n + G, dtype, dev)
    idt = torch.int16 if buf.element_size() == 2 else torch.int32
    fill = buf.view(idt).clone()
    view = buf[G + off:G + off + n]
    assert view.data_ptr() % 16 == (off * buf.element_size()) % 16
    if not isinstance(values, int):
        view.copy_(values.reshape(-1).to(dtype))

    def check(what):
        bits = buf.view(idt)
        assert torch.equal(bits[:G + off], fill[:G + off]) and torch.equal(bits[G + off + n:], fill[G + off + n:]), f"{what}: stray write in a guard"
        assert bool(torch.isfinite(view.float()).all()), f"{what}: missing write or non-finite value"

    return view, check


def _plan(dev, n_steps, eta=1.0, dual=False):
    import ap_adapter_amd as A
    s = A.DDIMScheduler()
    s.set_timesteps(n_steps)
    p = s.inversion_plan(eta, dual=dual)
    return p, p.table.to(dev), p.keep.to(dev)


def _guided(eps, branches, gs, s_a, s_t, dtype):
    return SO.cfg_combine_rounded(eps, gs, dtype) if branches == 2 else GO.cfg3_combine_rounded(eps, s_a, s_t, dtype)


def _check_invert_launch(dev, dtype, branches, B, n, off, n_steps, step, x, x0, draws, eps, plan, coef_d, keep_d, gtab, gs, with_eps_out=True):
    """one launch of apad_cfg_invert_step at counter ``step`` (clamped to row i) on guarded, NaN-prefilled outputs, against the restatement.
    Bounds (derived, not tuned; u = 2^-24 is half an fp32 unit in the last place):
      latents == fma(kx, x0, kz n~) evaluated in fp32 on the host, bit for bit;  unet_in == latents.to(dtype), bit for bit;
      |z - z_ref| <= 2^-21 (|c_x x| + |c_e eps| + |kx x0| + |kz n~|) / std + 2^-23 |z_ref|: mu and the target take two roundings each, every
      one at most u of a partial result no larger than the sum S of the four magnitudes (4 u S), the subtraction one more (2 u S, its result
      is at most 2 S), the fp32 table entries against the restatement's float64 coefficients 4 u S -- 10 u S <= 2^-21 S -- all divided by
      std; the division itself rounds z once (u |z| <= 2^-23 |z_ref|)."""
    from ap_adapter_amd import ops
    acp, ts = SO.acp64(), SO.grid(n_steps)
    i = min(max(step, 0), n_steps - 1)
    lat, lat_check = _band(x, dev, off=off)
    noise, noise_check = _band(draws, dev, off=off)
    x0_d, _ = _band(x0, dev, off=off)
    unet_in, ui_check = _band(B * n, dev, dtype)
    eps_out, eo_check = _band(B * n, dev, off=off) if with_eps_out else (None, None)
    ptr = torch.full((1,), step, dtype=torch.int32, device=dev)
    ops.cfg_invert_step(eps.to(dev, dtype), lat.view(B, n), unet_in.view(B, n), coef_d, keep_d, x0_d.view(B, n), noise.view(n_steps, B, n), ptr,
                        guidance_scale=gs if branches == 2 else None, guidance=gtab.to(dev) if branches == 3 else None,
                        eps_out=None if eps_out is None else eps_out.view(B, n))
    for check, what in ((lat_check, "latents"), (noise_check, "noise"), (ui_check, "unet_in")) + (((eo_check, "eps_out"),) if with_eps_out else ()):
        check(f"apad_cfg_invert_step step {step} {what}")
    lat_h, z_h, ui_h = lat.cpu().view(B, n), noise.cpu().view(n_steps, B, n), unet_in.cpu().view(B, n)
    # rows of the noise table other than this step's are untouched
    for j in range(n_steps):
        if j != i:
            assert torch.equal(z_h[j], draws[j]), (step, j)
    kx, kz = float(plan.keep[i, 0]), float(plan.keep[i, 1])
    want = _fma32(kx, x0, (kz * draws[i].double()).float())
    assert torch.equal(lat_h, want), f"latents differ from fma(kx, x0, kz n~) at step {step}"
    assert torch.equal(ui_h, want.to(dtype)), f"unet_in is not the rounded copy of latents at step {step}"
    if i == n_steps - 1:
        assert torch.equal(lat_h, x0)  # the last row lands on x0 itself
    s_a, s_t = (float(gtab[i, 0]), float(gtab[i, 1])) if branches == 3 else (0.0, 0.0)
    e = _guided(eps, branches, gs, s_a, s_t, dtype)
    if with_eps_out:
        assert rel_err(eps_out.view(B, n), e.float()) < 1e-6  # (test_gpu_samplers._check_step's bound on the guided noise)
        e = eps_out.cpu().view(B, n).double()
    nxt, z_ref, _ = IO.invert_step(x, e, x0, draws[i], i, 0, ts, acp, 1.0)
    c_x, c_e, std = IO.row(i, 0, ts, acp, 1.0)
    lx, lz = IO.level(i, 0, ts, acp)
    S = (c_x * x.double()).abs() + (c_e * e).abs() + (lx * x0.double()).abs() + (lz * draws[i].double()).abs()
    bound = 2.0 ** -21 * S / std + 2.0 ** -23 * z_ref.abs()
    err = (z_h[i].double() - z_ref).abs()
    worst = float((err / bound).max())
    assert bool((err <= bound).all()), f"z exceeds its bound at step {step}: worst err / bound = {worst:.3f}"
    return lat_h, z_h[i], ui_h, worst


def _operands(B, n, n_steps, branches, dtype):
    x, x0 = R(B, n, seed=44), R(B, n, seed=60, std=0.7)
    draws = R(n_steps, B, n, seed=9)
    eps = q(R(branches * B, n, seed=100) * 0.5, dtype)
    gtab = torch.tensor([[2.5, 7.5], [1.0, 3.0], [0.5, 4.0], [3.0, 1.5]][:n_steps] + [[2.0, 2.0]] * max(0, n_steps - 4))
    return x, x0, draws, eps, gtab


@pytest.mark.parametrize("geom", list(GEOMS))
@pytest.mark.parametrize("branches", [2, 3])
@pytest.mark.parametrize("dtype", DTYPES)
def test_cfg_invert_step_matches_oracle(dev, dtype, branches, geom):
    """n_steps = 3; the counter at 0, 1, 2 and -1 / 5 (clamped to rows 0 / 2, like the step kernel); eps_out given and null (the same bits)"""
    B, npix, C, off = GEOMS[geom]
    n, n_steps, gs = npix * C, 3, 7.5
    plan, coef_d, keep_d = _plan(dev, n_steps, dual=branches == 3)
    x, x0, draws, eps, gtab = _operands(B, n, n_steps, branches, dtype)
    worst = 0.0
    for step in (0, 1, 2, -1, 5):
        args = (dev, dtype, branches, B, n, off, n_steps, step, x, x0, draws, eps, plan, coef_d, keep_d, gtab, gs)
        a = _check_invert_launch(*args)
        b = _check_invert_launch(*args, with_eps_out=False)
        assert all(torch.equal(u, v) for u, v in zip(a[:3], b[:3])), step
        worst = max(worst, a[3], b[3])
    print(f"\n[apad_cfg_invert_step {dtype}, {branches} branches, {geom}] worst |z - z_ref| / bound = {worst:.3f}")


@pytest.mark.parametrize("geom", list(GEOMS))
@pytest.mark.parametrize("branches", [2, 3])
@pytest.mark.parametrize("dtype", DTYPES)
def test_invert_then_sampler_step_retraces_the_trajectory(dev, dtype, branches, geom):
    """The property the feature rests on, on the two kernels alone: apad_cfg_invert_step over 4 steps with a fixed random eps per step, then
    the sampler step (apad_cfg_sampler_step; three branches: apad_cfg_dual_step) with the same eps, the same table and noise = z.  Both
    launches get the same buffers, hence the same form.

    Per step, from the inversion's own x_(i):  |x' - x_(i+1)| <= 2^-22 (|x_(i+1)| + |x_(i+1) - mu|), elementwise.  Derivation: the sampler
    forms mu with the inversion's operations (bit for bit the same mu), then x' = fl(mu + fl(std z)) with z = fl(fl(x_(i+1) - mu) / std):
    three roundings on x_(i+1) - mu and one on the sum in the unfused form (u (3 |x_(i+1) - mu| + |x_(i+1)|), u = 2^-24), fewer in the
    fused one.

    Chained from the same start (each sampler step from the sampler's own previous x'), the difference d_i = x'_(i) - x_(i) enters mu through
    c_x, so the bound that can be derived is the recurrence t_0 = 0, t_(i+1) = |c_x| t_i (1 + 2^-22) + 2^-22 (|x_(i+1)| + |x_(i+1) - mu| +
    |c_x| t_i): at step 0 it IS the per-step bound; c_x = sqrt(acp_prev / acp_t) > 1 carries it forward."""
    from ap_adapter_amd import ops
    B, npix, C, off = GEOMS[geom]
    n, n_steps, gs = npix * C, 4, 7.5
    plan, coef_d, keep_d = _plan(dev, n_steps, dual=branches == 3)
    x_start, x0, draws, _, gtab = _operands(B, n, n_steps, branches, dtype)
    gtab_d = gtab.to(dev) if branches == 3 else None
    eps = [q(R(branches * B, n, seed=100 + i) * 0.5, dtype).to(dev, dtype) for i in range(n_steps)]
    lat, _ = _band(x_start, dev, off=off)
    noise, _ = _band(draws, dev, off=off)
    x0_d, _ = _band(x0, dev, off=off)
    eps_out, _ = _band(B * n, dev, off=off)
    unet_in = torch.empty(B, n, dtype=dtype, device=dev)
    ptr = torch.zeros(1, dtype=torch.int32, device=dev)
    lat, noise, x0_d, eps_out = lat.view(B, n), noise.view(n_steps, B, n), x0_d.view(B, n), eps_out.view(B, n)
    xs, es = [lat.clone()], []
    for i in range(n_steps):
        ops.cfg_invert_step(eps[i], lat, unet_in, coef_d, keep_d, x0_d, noise, ptr, guidance_scale=gs if branches == 2 else None, guidance=gtab_d,
                            eps_out=eps_out)
        ops.step_advance(ptr)
        xs.append(lat.clone())
        es.append(eps_out.clone())
    assert torch.equal(xs[-1], x0_d)

    def sampler(i, x):
        ptr.fill_(i)
        if branches == 2:
            ops.cfg_sampler_step(eps[i], x, unet_in, coef_d, ptr, gs, eps_out, None, noise)
        else:
            ops.cfg_dual_step(eps[i], x, unet_in, coef_d, gtab_d, ptr, eps_out, None, noise)
        assert torch.equal(eps_out, es[i])  # the same guided noise in both kernels

    chained, _ = _band(x_start, dev, off=off)
    chained = chained.view(B, n)
    tol = torch.zeros(B, n, dtype=torch.float64)
    worst = [0.0, 0.0]
    for i in range(n_steps):
        c_x, c_e = float(plan.table[i, 0]), float(plan.table[i, 1])
        mu = c_x * xs[i].cpu().double() + c_e * es[i].cpu().double()
        nxt = xs[i + 1].cpu().double()
        bound = 2.0 ** -22 * (nxt.abs() + (nxt - mu).abs())
        lat.copy_(xs[i])  # per step: from the inversion's own x_(i)
        sampler(i, lat)
        err = (lat.cpu().double() - nxt).abs()
        worst[0] = max(worst[0], float((err / bound).max()))
        assert bool((err <= bound).all()), f"step {i}: worst err / bound = {float((err / bound).max()):.3f}"
        sampler(i, chained)  # chained: from the sampler's own previous result
        tol = abs(c_x) * tol * (1.0 + 2.0 ** -22) + bound + 2.0 ** -22 * abs(c_x) * tol
        err = (chained.cpu().double() - nxt).abs()
        worst[1] = max(worst[1], float((err / tol).max()))
        assert bool((err <= tol).all()), f"chained step {i}: worst err / bound = {float((err / tol).max()):.3f}"
    print(f"\n[invert -> sampler step, {dtype}, {branches} branches, {geom}] worst err / bound: per step {worst[0]:.3f}, chained {worst[1]:.3f}; "
          f"end vs x0: rel {rel_err(chained, x0):.2e}")


@pytest.mark.parametrize("total", [2048 * 256 + 37, 2048 * 256 * 8 + 8])
def test_grid_stride_wrap(dev, total):
    """more elements than the 2048-block grid covers in one pass: the scalar form (8 does not divide total) and the 16-byte form, fp32, both
    steps of a 2-step table, bounds as in test_cfg_invert_step_matches_oracle"""
    dtype, n_steps = torch.float32, 2
    plan, coef_d, keep_d = _plan(dev, n_steps)
    x, x0, draws, eps, gtab = _operands(1, total, n_steps, 2, dtype)
    for step in (0, 1):
        w = _check_invert_launch(dev, dtype, 2, 1, total, 0, n_steps, step, x, x0, draws, eps, plan, coef_d, keep_d, gtab, 7.5)[3]
        print(f"\n[apad_cfg_invert_step grid-stride wrap, total={total}, step {step}] worst |z - z_ref| / bound = {w:.3f}")


@pytest.mark.parametrize("geom", ["vec", "scalar"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_zero_std_row_writes_zero_noise(dev, dtype, geom):
    from ap_adapter_amd import ops
    B, npix, C, _ = GEOMS[geom]
    n, n_steps = npix * C, 3
    plan, coef_d, keep_d = _plan(dev, n_steps)
    coef_d = coef_d.clone()
    coef_d[1, 3] = 0.0
    x, x0, draws, eps, _ = _operands(B, n, n_steps, 2, dtype)
    lat, noise, x0_d = x.to(dev), draws.to(dev), x0.to(dev)
    unet_in = torch.full((B, n), float("nan"), dtype=dtype, device=dev)
    eps_out = torch.full((B, n), float("nan"), device=dev)
    ptr = torch.ones(1, dtype=torch.int32, device=dev)
    ops.cfg_invert_step(eps.to(dev, dtype), lat, unet_in, coef_d, keep_d, x0_d, noise, ptr, guidance_scale=7.5, eps_out=eps_out)
    assert bool((noise[1] == 0).all()) and torch.equal(noise[0].cpu(), draws[0]) and torch.equal(noise[2].cpu(), draws[2])
    want = _fma32(float(plan.keep[1, 0]), x0, (float(plan.keep[1, 1]) * draws[1].double()).float())
    assert torch.equal(lat.cpu(), want) and torch.equal(unet_in.cpu(), want.to(dtype))
    assert all(bool(torch.isfinite(t.float()).all()) for t in (lat, unet_in, eps_out, noise))


def test_bad_operands_raise_from_the_status_code(dev):
    """every refusal happens before a launch: nothing is provoked on the device"""
    from ap_adapter_amd import _lib as L
    from ap_adapter_amd import ops
    B, n, steps = 2, 64, 5
    lat, x0 = torch.zeros(B, n, device=dev), torch.zeros(B, n, device=dev)
    eps2 = torch.zeros(2 * B, n, dtype=torch.bfloat16, device=dev)
    eps3 = torch.zeros(3 * B, n, dtype=torch.bfloat16, device=dev)
    unet_in = torch.zeros(B, n, dtype=torch.bfloat16, device=dev)
    ptr = torch.zeros(1, dtype=torch.int32, device=dev)
    coef, keep, noise = torch.zeros(steps, 6, device=dev), torch.zeros(steps, 2, device=dev), torch.zeros(steps, B, n, device=dev)
    gtab = torch.ones(steps, 2, device=dev)
    ok = dict(eps=eps2, latents=lat, unet_in=unet_in, coef=coef, keep=keep, x0=x0, noise=noise, step_ptr=ptr, guidance_scale=7.5)
    for change, match in ((dict(coef=torch.zeros(steps, 2, device=dev)), r"\[steps, 6\]"),
                          (dict(keep=torch.zeros(steps - 1, 2, device=dev)), "keep"),
                          (dict(noise=torch.zeros(steps - 1, B, n, device=dev)), "noise"),
                          (dict(noise=torch.zeros(B, steps, n, device=dev)), "one row per step"),
                          (dict(x0=torch.zeros(B, n + 1, device=dev)), "x0"),
                          (dict(x0=None), "x0"),
                          (dict(keep=None), "keep"),
                          (dict(noise=noise.double()), "noise"),
                          (dict(latents=lat.cpu()), "GPU tensor"),
                          (dict(x0=x0.cpu()), "GPU tensor"),
                          (dict(unet_in=unet_in.float()), "share the model dtype"),
                          (dict(eps=eps3), "two branches"),
                          (dict(eps=eps2[:, ::2]), "contiguous"),
                          (dict(noise=torch.zeros(steps, B, 2 * n, device=dev)[:, :, ::2]), "contiguous"),
                          (dict(guidance=gtab), "not both"),
                          (dict(guidance_scale=None), "not both or neither"),
                          (dict(guidance_scale=None, guidance=gtab), "three branches"),
                          (dict(eps=eps3, guidance_scale=None, guidance=gtab[:3]), "guidance"),
                          (dict(eps_out=torch.zeros(B, n - 1, device=dev)), "eps_out")):
        with pytest.raises(RuntimeError, match=match):
            ops.cfg_invert_step(**{**ok, **change})
    # the entry point itself: a status code and a message, never an abort
    lib = L.lib()
    p = lambda t: t.data_ptr()
    call = lambda **kw: lib.apad_cfg_invert_step(*[{**dict(eps=p(eps2), lat=p(lat), ui=p(unet_in), eo=None, noise=p(noise), coef=p(coef), g=None,
                                                         keep=p(keep), x0=p(x0), ptr=p(ptr), steps=steps, gs=7.5, br=2, B=B, n=n, dt=L.BF16, st=None),
                                                    **kw}[k] for k in ("eps", "lat", "ui", "eo", "noise", "coef", "g", "keep", "x0", "ptr", "steps",
                                                                       "gs", "br", "B", "n", "dt", "st")])
    for kw, msg in ((dict(noise=None), b"null operand"), (dict(x0=None), b"null operand"), (dict(keep=None), b"null operand"),
                    (dict(br=4), b"branches = 4"), (dict(br=3), b"null guidance table"), (dict(dt=7), b"dtype 7"), (dict(B=0), b"empty problem"),
                    (dict(steps=0), b"empty problem")):
        assert call(**kw) != 0 and msg in lib.apad_last_error(), kw
    assert call() == 0 and call(ptr=None) == 0  # (a null counter is step 0)
    torch.cuda.synchronize()


# ---- the pipeline on the small synthetic UNet ----
N, GS = 6, 3.0


@pytest.fixture(scope="module", autouse=True)
def _profile():
    yield
    path = os.environ.get("APAD_INVERT_PROFILE")
    if path and MEASURED:
        with open(path, "w") as f:
            json.dump(MEASURED, f, indent=1, sort_keys=True)


def _pipe(dev, dtype):
    import ap_adapter_amd as A
    u = _small_unet(dev, dtype)[0]
    u.requires_grad_(False)
    return A.AudioLDM2Pipeline(u)


def _x0(dev, B=2, seed=70):
    return R(B, 8, 26, 16, seed=seed, std=0.7).to(dev)


def _round_trip(pipe, cond, x0, strength, seed=5, target=None, ags=None, mask=None, **kw):
    """invert under ``cond``, then the edit phase under ``target`` (default: the same condition and scale): (InvertedSource, result)"""
    import ap_adapter_amd as A
    k = pipe.scheduler.edit_start_index(N, strength)
    g = torch.Generator().manual_seed(seed)
    z0 = torch.randn(x0.shape, generator=g)
    inv = pipe.invert(A.EditSource(x0=x0, z0=z0, mask=mask), *cond, N, GS, start=k, eta=1.0, generator=g, audio_guidance_scale=ags, **kw)
    out = pipe.denoise(None, *(cond if target is None else target), N, GS, source=inv, start=k, eta=1.0, audio_guidance_scale=ags, **kw)
    return inv, out


@pytest.mark.parametrize("strength", [1.0, 0.5])
def test_fp32_round_trip_returns_the_source(dev, strength):
    """invert, then denoise under the SAME condition and scale: the run ends on the source latents.  Bar: the project's 1e-3 north-star
    bound; a float32 simulation of the chain with a smooth stand-in UNet puts the expectation near 1e-6 (the z_i are exact for the
    inversion's own trajectory, and the regeneration's differs from it by fp32 roundings the UNet passes on).  Measured on the MI355X, the
    same figure on every run: 8.5e-6 at strength 0.5 and 9.7e-4 at strength 1.0 -- the random-weight UNet amplifies a perturbation at the
    high-noise steps (the plain strength run from the same start ends 60 times the source's magnitude away), so the full schedule clears
    the bar by little."""
    pipe = _pipe(dev, torch.float32)
    x0 = _x0(dev)
    inv, out = _round_trip(pipe, _inputs(dev, torch.float32)[1:], x0, strength)
    k = pipe.scheduler.edit_start_index(N, strength)
    assert inv.z.shape == (N - k, 2, 26 * 16, 8) and inv.z.dtype == torch.float32 and inv.start == k and inv.eta == 1.0
    assert torch.equal(inv.x0, x0) and "invert" in inv.scheduler_key and bool(torch.isfinite(inv.z).all())
    err = rel_err(out, x0)
    MEASURED[f"fp32_strength_{strength}"] = err
    print(f"\n[invert -> denoise, fp32 small UNet, N={N}, strength={strength}] rel err to the source {err:.3e}")
    assert err < 1e-3


def test_bf16_round_trip_lands_closer_than_the_plain_strength_run(dev):
    """bf16: unet_in is the rounded copy of the fp32 master, and a rounding flip there moves one step's eps, so the bar is a relation: the
    round trip ends closer to the source than the plain ``strength`` run from the same source, seed, eta and conditions"""
    dtype = torch.bfloat16
    pipe = _pipe(dev, dtype)
    x0, cond = _x0(dev), _inputs(dev, dtype)[1:]
    for strength in (1.0, 0.5):
        k = pipe.scheduler.edit_start_index(N, strength)
        inv, out = _round_trip(pipe, cond, x0, strength)
        g = torch.Generator().manual_seed(5)
        z0 = torch.randn(x0.shape, generator=g)
        plain = pipe.denoise(None, *cond, N, GS, source=(x0, z0, None), start=k, eta=1.0, generator=g)
        err, err_plain = rel_err(out, x0), rel_err(plain, x0)
        MEASURED[f"bf16_strength_{strength}"] = err
        MEASURED[f"bf16_strength_{strength}_plain_sdedit"] = err_plain
        print(f"\n[invert -> denoise, bf16 small UNet, N={N}, strength={strength}] rel err to the source {err:.3e}; plain strength run {err_plain:.3e}")
        assert err < err_plain and bool(torch.isfinite(out).all())


def test_captured_eager_and_replayed_agree_bit_for_bit(dev):
    """both phases: the captured run, the eager run, and a replay (a cache hit with ANOTHER source, then the first source again)"""
    dtype = torch.bfloat16
    pipe = _pipe(dev, dtype)
    cond, cond_b = _inputs(dev, dtype)[1:], _inputs(dev, dtype, seed=3)[1:]
    x0, x0b = _x0(dev), _x0(dev, seed=80)
    inv, out = _round_trip(pipe, cond, x0, 0.5)
    assert (pipe.graph_captures, pipe.graph_hits) == (2, 0)  # one step captured per phase
    assert any("invert" in str(k) for k in pipe._graphs)
    z_first = inv.z.clone()
    inv_e, out_e = _round_trip(pipe, cond, x0, 0.5, use_graph=False)
    assert torch.equal(inv.z, inv_e.z) and torch.equal(inv.x0, inv_e.x0) and torch.equal(out, out_e)
    inv_b, out_b = _round_trip(pipe, cond_b, x0b, 0.5, seed=6)
    assert (pipe.graph_captures, pipe.graph_hits) == (2, 2)
    assert torch.equal(inv.z, z_first)  # the replay did not overwrite a result in use
    inv_be, out_be = _round_trip(pipe, cond_b, x0b, 0.5, seed=6, use_graph=False)
    assert torch.equal(inv_b.z, inv_be.z) and torch.equal(out_b, out_be) and not torch.equal(inv_b.z, inv.z)
    inv_2, out_2 = _round_trip(pipe, cond, x0, 0.5)
    assert (pipe.graph_captures, pipe.graph_hits) == (2, 4) and torch.equal(inv_2.z, inv.z) and torch.equal(out_2, out)


def test_another_condition_edits_and_a_mask_keeps(dev):
    dtype = torch.bfloat16
    pipe = _pipe(dev, dtype)
    cond, target = _inputs(dev, dtype)[1:], _inputs(dev, dtype, seed=3)[1:]
    x0 = _x0(dev)
    _, same = _round_trip(pipe, cond, x0, 1.0)
    _, edited = _round_trip(pipe, cond, x0, 1.0, target=target)
    assert rel_err(edited, x0) > rel_err(same, x0) and not torch.equal(edited, same) and bool(torch.isfinite(edited).all())
    mask = torch.zeros(1, 1, 26, 16, device=dev)
    mask[:, :, 5:15] = 1.0
    inv, masked = _round_trip(pipe, cond, x0, 1.0, target=target, mask=mask)
    assert inv.mask is mask
    assert torch.equal(masked[:, :, :5], x0[:, :, :5]) and torch.equal(masked[:, :, 15:], x0[:, :, 15:])
    assert not bool((masked[:, :, 5:15] == x0[:, :, 5:15]).all())


def test_three_branch_round_trip(dev):
    pipe = _pipe(dev, torch.float32)
    x0 = _x0(dev)
    cond3 = _inputs3(dev, torch.float32)[1:]
    inv, out = _round_trip(pipe, cond3, x0, 0.5, ags=2.0)
    assert "dual" in str([k for k in pipe._graphs if "invert" in str(k)][0])
    err = rel_err(out, x0)
    MEASURED["fp32_three_branch_strength_0.5"] = err
    print(f"\n[invert -> denoise, three branches, fp32 small UNet, N={N}, strength=0.5] rel err to the source {err:.3e}")
    assert err < 1e-3
    # an edit on three branches: another audio scale is another result, on the same captured steps
    k = pipe.scheduler.edit_start_index(N, 0.5)
    other = pipe.denoise(None, *cond3, N, GS, source=inv, start=k, eta=1.0, audio_guidance_scale=0.5)
    assert pipe.graph_captures == 2 and rel_err(other, x0) > 10 * err


def test_default_call_reaches_neither_the_new_op_nor_the_noise_copy(dev, monkeypatch):
    """calls without ``inversion=`` -- plain, eta > 0, a strength edit with eta > 0 -- launch no apad_cfg_invert_step and copy no noise table;
    ``inversion="ddpm"`` reaches both and is invert + denoise spelled out"""
    import ap_adapter_amd as A
    dtype = torch.bfloat16
    pipe = _pipe(dev, dtype)
    B = 2
    lat, ehs, ehs1, m1 = _inputs(dev, dtype)
    tgt = _inputs(dev, dtype, seed=3)
    calls = _count(monkeypatch, ("cfg_invert_step", "cfg_sampler_step", "cfg_ddim_step"))
    copies = []
    real_copy = A.AudioLDM2Pipeline._copy_step_noise
    monkeypatch.setattr(A.AudioLDM2Pipeline, "_copy_step_noise", staticmethod(lambda out, z: (copies.append(1), real_copy(out, z))[1]))
    kw = dict(prompt_embeds=tgt[2][B:], negative_prompt_embeds=ehs1[:B], generated_prompt_embeds=tgt[1][B:], negative_generated_prompt_embeds=ehs[:B],
              attention_mask=tgt[3][B:], negative_attention_mask=m1[:B], audio_length_in_s=1.04, num_inference_steps=N, guidance_scale=GS,
              output_type="latent", use_graph=False)
    g = lambda: torch.Generator().manual_seed(7)
    x0 = _x0(dev)
    pipe(latents=lat, **kw)
    pipe(latents=lat, eta=1.0, generator=g(), **kw)
    pipe(source_latents=x0, strength=0.5, eta=1.0, generator=g(), **kw)
    assert len(calls["cfg_invert_step"]) == 0 and not copies
    assert len(calls["cfg_ddim_step"]) == N and len(calls["cfg_sampler_step"]) == N + N // 2
    skw = dict(source_prompt_embeds=ehs1[B:], source_generated_prompt_embeds=ehs[B:], source_attention_mask=m1[B:])
    out = pipe(source_latents=x0, strength=0.5, eta=1.0, generator=g(), inversion="ddpm", **skw, **kw).audios
    assert len(calls["cfg_invert_step"]) == N // 2 and len(copies) == 1 and len(calls["cfg_sampler_step"]) == N + N
    monkeypatch.undo()
    gen = g()
    z0 = torch.randn(x0.shape, generator=gen)
    tgt_cond = (torch.cat([ehs[:B], tgt[1][B:]]), torch.cat([ehs1[:B], tgt[2][B:]]), torch.cat([m1[:B], tgt[3][B:]]))
    inv = pipe.invert(A.EditSource(x0=x0, z0=z0), ehs, ehs1, m1, N, 3.0, start=N // 2, eta=1.0, generator=gen, use_graph=False)
    assert torch.equal(out, pipe.denoise(None, *tgt_cond, N, GS, source=inv, start=N // 2, eta=1.0, use_graph=False))
    assert not torch.equal(out, x0) and bool(torch.isfinite(out).all())  # another text: an edit, not the source
