"""-m gpu: guidance rescale and adaptive projected guidance -- apad_cfg_shaped_step against the float64 restatement
(tests/shaped_guidance_oracle.py) within a bound derived from the rounding model (``_bounds``), its all-off row against the existing entry
points bit for bit, batch independence, three consecutive steps, and the denoise loop with the knobs on.  PARITY UNPINNED (see the oracle).

Shapes.  The kernel walks a clip with 1024 threads x 8 elements (16-byte form) or x 1 (scalar form), so:
  n = 8          one vector, every other lane idle            n = 8 * 65     crosses a wave
  n = 8192 + 24  a second, partial sweep                      n = 1001       scalar form, odd
  n = 2          the least n with a standard deviation        n = 32000      the product clip (once, bf16, B = 2)
each with B in {1, 3}, the three dtypes and two and three branches.

With APAD_SHAPED_PROFILE=<path> the largest observed error-to-bound ratios are merged into that JSON file (profiles/shaped_step.json)."""
import json
import math
import os

import pytest
import torch

from util import guarded, nan_buffer, q, rel_err

import sampler_oracle as SO
import shaped_guidance_oracle as SG
from test_gpu_edit import _fma32, _full, _mask
from test_gpu_samplers import _count
from test_gpu_unet import _cond, _small_unet

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float16, torch.float32]
NS = [8, 8 * 65, 8192 + 24, 1001, 2]
OFF = (0.0, 1.0, 0.0, 0.0)
U = 2.0 ** -24  # fp32 unit roundoff
MEASURED = {}


@pytest.fixture(scope="module", autouse=True)
def _profile():
    yield
    path = os.environ.get("APAD_SHAPED_PROFILE")
    if path and MEASURED:
        doc = {}
        if os.path.exists(path):
            with open(path) as f:
                doc = json.load(f)
        doc["error_to_bound"] = {"what": "largest observed |GPU - float64 restatement| / derived bound (tests/test_gpu_shaped_guidance.py, _bounds)",
                                 **{k: round(v, 4) for k, v in sorted(MEASURED.items())}}
        with open(path, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


def R(*shape, seed=0, std=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * std


def _weights(NB):
    return (7.5,) if NB == 2 else (2.5, 7.5)


def _branches(B, n, NB, dtype, seed=100):
    """[NB * B, n] fp32 holding ``dtype`` values: correlated branches (e_0 = c + 0.3 noise, e_A between them), c off-centre"""
    c = R(B, n, seed=seed) * 0.5 + 0.1
    if NB == 2:
        return q(torch.cat([c + 0.3 * R(B, n, seed=seed + 1), c]), dtype)
    e_a = c + 0.2 * R(B, n, seed=seed + 2)
    return q(torch.cat([e_a + 0.3 * R(B, n, seed=seed + 1), e_a, c]), dtype)


def _channels(n):
    return 8 if n % 8 == 0 else (7 if n % 7 == 0 else 2)


def _is_vec(n):
    return n % 8 == 0


def _knobs(n):
    r = 0.15 * math.sqrt(n)  # about half the norm of a difference of 0.3 sigma
    return {"phi": (0.7, 1.0, 0.0, 0.0), "eta": (0.0, 0.25, 0.0, 0.0), "r": (0.0, 1.0, r, 0.0), "beta": (0.0, 1.0, 0.0, -0.5),
            "all": (0.7, 0.25, r, -0.5)}


def _f32(v):
    return float(torch.tensor(float(v), dtype=torch.float32))


class Run:
    """the operands of one launch on the device, every written buffer between NaN guard bands (guard_rows = 2 keeps a 16-byte aligned start
    for 8 | n), and the host copies of what went in"""

    def __init__(self, dev, dtype, NB, B, n, coef, step, steps, row_table, masked, mom_prev, seed=100, eps=None, gtab=None):
        self.dev, self.dtype, self.NB, self.B, self.n, self.step, self.steps = dev, dtype, NB, B, n, step, steps
        K = NB - 1
        self.eps = _branches(B, n, NB, dtype, seed) if eps is None else eps
        self.x, self.h, self.z = R(B, n, seed=seed + 10), R(B, n, seed=seed + 11) * 3.0, R(steps, B, n, seed=seed + 12)
        self.coef, self.table = coef, row_table
        self.w = _weights(NB)
        self.gtab = gtab
        if NB == 3 and gtab is None:
            self.gtab = torch.full((steps, 2), float("nan"))
            self.gtab[step] = torch.tensor(self.w)
        G = 2
        self.lat, self.lat_check = guarded(B, n, torch.float32, dev, guard_rows=G)
        self.lat.copy_(self.x)
        self.unet_in, self.ui_check = guarded(B, n, dtype, dev, guard_rows=G)
        self.eps_out, self.eo_check = guarded(B, n, torch.float32, dev, guard_rows=G)
        self.hist, self.h_check = guarded(B, n, torch.float32, dev, guard_rows=G)
        self.hist.copy_(self.h)
        self.stats, self.st_check = guarded(B, 8, torch.float32, dev, guard_rows=G)
        self.mom_prev = mom_prev
        self.mom = self.m_check = None
        if mom_prev is not None:
            mom, self.m_check = guarded(K * B, n, torch.float32, dev, guard_rows=G)
            mom.copy_(mom_prev.reshape(K * B, n))
            self.mom = mom.view(K, B, n)
        self.masked = None
        if masked:
            C = _channels(n)
            self.C = C
            self.keep = torch.rand(steps, 2, generator=torch.Generator().manual_seed(5)) + 0.25
            self.x0, self.z0, self.mask = R(B, n, seed=seed + 20), R(B, n, seed=seed + 21), _mask("fraction-clip", B, n // C)
            self.masked = dict(keep=self.keep.to(dev), x0=self.x0.to(dev), z0=self.z0.to(dev), mask=self.mask.to(dev), channels=C)
        self.ptr = torch.full((1,), step, dtype=torch.int32, device=dev)

    def launch(self, stats=True, history=True, noise=True):
        from ap_adapter_amd import ops
        self.noise_d = self.z.to(self.dev) if noise else None
        self.used_history, self.used_noise = history, noise
        ops.cfg_shaped_step(self.eps.to(self.dev, self.dtype), self.lat, self.unet_in, self.coef.to(self.dev), self.table.to(self.dev), self.ptr,
                            self.w[0] if self.NB == 2 else None, None if self.NB == 2 else self.gtab.to(self.dev), self.mom,
                            self.stats if stats else None, self.eps_out, self.hist if history else None, self.noise_d, **(self.masked or {}))
        torch.cuda.synchronize()
        return self

    def check_guards(self, what, history=True):
        for check, name in ((self.lat_check, "latents"), (self.ui_check, "unet_in"), (self.eo_check, "eps_out"), (self.st_check, "stats")) + \
                (((self.h_check, "history"),) if history else ()):
            check(f"{what} {name}")
        if self.m_check is not None and float(self.table[min(self.step, self.steps - 1), 3]) != 0.0:
            self.m_check(f"{what} momentum")


def _depth(n, vec):
    """additions on the longest path of one of the kernel's sums: a thread's own elements in order, 6 butterfly levels, 15 wave partials"""
    V = 8 if vec else 1
    return V * math.ceil(n / (1024 * V)) + 6 + 15


def _half_ulp(dtype, a):
    if dtype == torch.bfloat16:
        return a * 2.0 ** -8
    if dtype == torch.float16:
        return torch.clamp(a * 2.0 ** -11, min=2.0 ** -25)
    return a * U


def _bounds(o, w, row, mom_prev, vec, dtype):
    """First-order rounding bounds of apad_cfg_shaped_step against the float64 restatement ``o`` on the same operands (and the same momentum
    state before the step), with u = 2^-24.

    Sums.  A sum of n terms is formed along a path of D = L + 6 + 15 additions (``_depth``; L = a thread's own elements), each an fp32 rounding,
    the products fused into the additions; so |sum^ - sum| <= D u sum|terms|.  The terms carry their own roundings: d_k = fl(e_(k+1) - e_k)
    (u |d|), after a momentum update m = fl(beta m' + d) (another u |m|): |delta d| <= 2 u a_d with a_d = |d_raw| + |beta m'| >= |d|.  A product
    of two such terms is off by at most 4 u a_d a_x.  Every sum therefore gets gamma = (D + 6) u times the sum of its terms' magnitudes, with
    a_d for |d|:   E<d,c> = gamma sum a_d |c|,  E<d,d> = gamma sum a_d^2,  E<c,c> = gamma <c,c>,  E(sum x) = gamma sum |x|.
    Scalars.   p = <d,c> / <c,c>:   E_p = (E<d,c> + |p| E<c,c>) / <c,c> + u |p|;      q = (1 - eta) p:   E_q = |1 - eta| E_p + 2 u |q|
               ||d|| = sqrt <d,d>:  relative rho = E<d,d> / <d,d> + u (sqrt(1 - x) >= 1 - x);   t = r / ||d||:   E_t = t (rho + u)
    (whichever side of ||d|| = r the kernel lands on, its t is within E_t of the restatement's).
    Elements.  v = d - q c, u_k = t v:   delta u = E_t |v| + t (delta d + E_q |c| + u |v|) + u t |v|;
               g = e_0 + sum w_k u_k (K fused multiply-adds):   delta g = sum |w_k| delta u_k + K u (|e_0| + sum |w_k u_k|).
    Rescale.   sum g = sum e_0 + sum_k w_k t_k (sum d_k - q_k sum c) from the pass-1 sums: the errors above propagated, plus 4 u of its terms;
               mean = sum / n (+ u).  a_i = g_i - mean g is off by eps_i = delta g_i + E_mean + u |a_i|, so
               S_g = sum a_i^2 is off by sum (2 |a_i| eps_i + eps_i^2) + gamma sum (|a_i| + eps_i)^2,  std = sqrt(S / (n - 1)): relative
               rho_g = E_S / S + 2 u;  likewise c.  f = phi std_c / std_g + 1 - phi:  E_f = phi (std_c / std_g) ((rho_c + rho_g) / (1 - rho_g) + u)
               + 2 u (|f| + phi std_c / std_g + |1 - phi|);   g <- f g:   delta g' = E_f |g| + |f| delta g + u |f g|.
    eps = (dtype) g':  half a ulp of dtype at |g'| + delta g' on top (2^-8 relative for bf16, 2^-11 and at least 2^-25 for f16, u for fp32).
    Returns dict(eps [B, n], t / q (lists of [B]), mean_g, std_g, std_c, f ([B]))."""
    phi, eta, r, beta = (float(v) for v in row)
    e0, c = o["e0"], o["c"]
    n, K = c.shape[-1], len(o["d"])
    gam = (_depth(n, vec) + 6) * U
    ac = c.abs()
    cc = (c * c).sum(-1)
    E_cc, E_sc, E_se0 = gam * cc, gam * ac.sum(-1), gam * e0.abs().sum(-1)
    col = lambda s: s[:, None]
    dg = K * U * e0.abs()
    E_t, E_q, E_sumg = [], [], E_se0 + 4 * U * e0.sum(-1).abs()
    for k in range(K):
        d, t, qk = o["d"][k], o["t"][k], o["q"][k]
        a_d = o["d_raw"][k].abs() + (abs(beta) * mom_prev[k].double().abs() if beta != 0.0 else 0.0)
        dd = (d * d).sum(-1)
        E_dc, E_dd, E_sd = gam * (a_d * ac).sum(-1), gam * (a_d * a_d).sum(-1), gam * a_d.sum(-1)
        p = torch.where(cc > 0, (d * c).sum(-1) / cc.clamp_min(1e-300), torch.zeros_like(cc))
        E_p = torch.where(cc > 0, (E_dc + p.abs() * E_cc) / cc.clamp_min(1e-300), torch.zeros_like(cc)) + U * p.abs()
        eq = abs(1.0 - eta) * E_p + 2 * U * qk.abs() if eta != 1.0 else torch.zeros_like(cc)
        et = t * (torch.where(dd > 0, E_dd / dd.clamp_min(1e-300), torch.zeros_like(dd)) + 2 * U) if r > 0.0 else torch.zeros_like(cc)
        v = d - col(qk) * c
        du = col(et) * v.abs() + col(t) * (2 * U * a_d + col(eq) * ac + U * v.abs()) + U * col(t) * v.abs()
        dg = dg + abs(w[k]) * du + K * U * abs(w[k]) * o["u"][k].abs()
        sd, sc = d.sum(-1), c.sum(-1)
        E_sumg = E_sumg + abs(w[k]) * (et * (sd - qk * sc).abs() + t * (E_sd + eq * sc.abs() + qk.abs() * E_sc)) \
            + 4 * U * abs(w[k]) * t * (sd.abs() + (qk * sc).abs())
        E_t.append(et)
        E_q.append(eq)
    g = o["g_pre"]
    zero = torch.zeros_like(cc)
    E_mg = E_sg = E_sdc = E_f = zero
    if phi > 0.0 and n > 1:
        mg, mc = g.mean(-1), c.mean(-1)
        E_mg = E_sumg / n + U * mg.abs()
        E_mc = E_sc / n + U * mc.abs()

        def rho(a, e):
            S = (a * a).sum(-1)
            E_S = (2 * a.abs() * e + e * e).sum(-1) + gam * ((a.abs() + e) ** 2).sum(-1)
            x = torch.where(S > 0, E_S / S.clamp_min(1e-300), torch.full_like(S, float("inf")))
            return torch.where(x < 1, x, torch.full_like(x, float("inf"))) + 2 * U

        a, b = g - col(mg), c - col(mc)
        rho_g, rho_c = rho(a, dg + col(E_mg) + U * a.abs()), rho(b, col(E_mc) + U * b.abs())
        ratio = o["std_c"] / o["std_g"].clamp_min(1e-300)
        E_f = phi * ratio * ((rho_c + rho_g) / (1 - rho_g).clamp_min(1e-300) + U) + 2 * U * (o["f"].abs() + phi * ratio + abs(1 - phi))
        E_f = torch.where(rho_g < 1, E_f, torch.full_like(E_f, float("inf")))
        E_sg, E_sdc = o["std_g"] * rho_g, o["std_c"] * rho_c
        dg = col(E_f) * g.abs() + col(o["f"].abs()) * dg + U * (col(o["f"]) * g).abs()
    eps = dg + _half_ulp(dtype, o["g"].abs() + dg)
    return dict(eps=eps, t=E_t, q=E_q, mean_g=E_mg, std_g=E_sg, std_c=E_sdc, f=E_f)


def _ratio(err, bound):
    """largest err / bound (0 / 0 = 0, x / 0 = inf)"""
    err, bound = err.double().reshape(-1), bound.double().reshape(-1)
    r = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    return float(r.max())


def _record(key, value):
    MEASURED[key] = max(MEASURED.get(key, 0.0), value)


def _check_against_oracle(run, row, tag):
    """every output of one launch against the restatement: stats and eps_out within ``_bounds``; the step after eps -- latents, unet_in,
    history -- against the float64 update of the kernel's OWN eps_out: a row of at most four products and a blend of two, every operation
    rounded once, so 8 u of the summed term magnitudes; unet_in is the rounded copy of the fp32 latents (half a ulp, plus u for a fold of the
    rounding into the last fma); momentum is fl(fma(beta, m', d)) bit for bit."""
    B, n, NB, dtype, s = run.B, run.n, run.NB, run.dtype, min(run.step, run.steps - 1)
    o = SG.shaped_guidance(run.eps, NB, [_f32(x) for x in run.w], row, None if run.mom_prev is None else run.mom_prev.double())
    bd = _bounds(o, [_f32(x) for x in run.w], row, run.mom_prev, _is_vec(n), dtype)
    st = run.stats.double().cpu()
    worst = {}
    # stats: (t_1, q_1, t_2, q_2, mean g, std g, std c, f), each stored as fp32 (+ u)
    ref = o["stats"]
    sb = torch.stack([bd["t"][0], bd["q"][0], bd["t"][-1] if NB == 3 else torch.zeros(B, dtype=torch.float64),
                      bd["q"][-1] if NB == 3 else torch.zeros(B, dtype=torch.float64), bd["mean_g"],
                      bd["std_g"], bd["std_c"], bd["f"]], dim=1).double() + U * ref.abs()
    worst["stats"] = _ratio((st - ref).abs(), sb)
    e_dev = run.eps_out.double().cpu()
    worst["eps"] = _ratio((e_dev - o["g"]).abs(), bd["eps"])
    # the step, from the kernel's own eps
    r6 = run.coef[s]
    use_h, use_z = run.used_history and float(r6[2]) != 0.0, run.used_noise and float(r6[3]) != 0.0
    xn, m0 = SG.sampler_row_update(r6, run.x, e_dev, run.h if use_h else None, run.z[s] if use_z else None)
    mag = (float(r6[0]) * run.x.double()).abs() + (float(r6[1]) * e_dev).abs() + (float(r6[2]) * run.h.double()).abs() * use_h \
        + (float(r6[3]) * run.z[s].double()).abs() * use_z
    if run.masked is not None:
        m = _full(run.mask, B, run.C)
        known = float(run.keep[s, 0]) * run.x0.double() + float(run.keep[s, 1]) * run.z0.double()
        mag = m * (mag + xn.abs()) + (1 - m) * ((float(run.keep[s, 0]) * run.x0.double()).abs() + (float(run.keep[s, 1]) * run.z0.double()).abs()
                                                   + known.abs())
        xn = SG.edit_blend(xn, m, run.keep[s], run.x0, run.z0)
    lat = run.lat.double().cpu()
    worst["latents"] = _ratio((lat - xn).abs(), 8 * U * mag)
    worst["unet_in"] = _ratio((run.unet_in.double().cpu() - lat).abs(), _half_ulp(dtype, lat.abs()) + U * lat.abs())
    if run.used_history:
        worst["history"] = _ratio((run.hist.double().cpu() - m0).abs(), 3 * U * ((float(r6[4]) * run.x.double()).abs() + (float(r6[5]) * e_dev).abs()))
    if run.mom is not None and float(row[3]) != 0.0:
        d32 = [(run.eps[(k + 1) * B:(k + 2) * B] - run.eps[k * B:(k + 1) * B]) for k in range(NB - 1)]  # fp32 subtraction, as the kernel's
        want = torch.stack([_fma32(_f32(row[3]), run.mom_prev[k], d32[k]) for k in range(NB - 1)])
        assert torch.equal(run.mom.cpu(), want), f"{tag}: momentum is not fl(fma(beta, m, d))"
    elif run.mom is not None:  # beta == 0: untouched, NaN included
        assert torch.equal(run.mom.cpu().view(torch.int32), run.mom_prev.view(torch.int32)), f"{tag}: momentum written on a beta == 0 row"
    print(f"[{tag}] err / bound: " + " ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    for k, v in worst.items():
        _record(f"{k}_{str(dtype).split('.')[-1]}", v)
        assert v <= 1.0, f"{tag}: {k} exceeds its bound, worst err / bound = {v:.3f}"
    return o


def _tables(kind, steps):
    """(coef fp32 [steps, 6], row to run): DPM-Solver++ 2M rows (an interior, second-order row: the history is read) or DDIM eta = 1 rows
    (the noise table is read)"""
    import ap_adapter_amd as A
    s = A.DPMSolverMultistepScheduler() if kind == "dpm" else A.DDIMScheduler()
    s.set_timesteps(steps)
    plan = s.sampler_plan(1.0, dual=True)
    assert plan.table.shape == (steps, 6) and (plan.needs_history if kind == "dpm" else plan.needs_noise)
    return plan.table


def _one_row_table(row, step, steps):
    t = torch.full((steps, 4), float("nan"))  # only row ``step`` may be read
    t[step] = torch.tensor(row)
    return t


@pytest.mark.parametrize("NB", [2, 3])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", NS)
def test_shaped_step_matches_the_restatement_within_the_derived_bound(dev, n, dtype, NB):
    """each knob alone, on DPM-Solver++ rows / DDIM eta = 1 rows and with / without a per-clip mask in turn, then all knobs together on all four
    combinations; B = 1 and 3.  Bound: ``_bounds`` (derivation in its docstring) for stats and eps_out, ``_check_against_oracle`` for the rest."""
    steps, step = 4, 2
    combos = [("dpm", False), ("ddim", True), ("dpm", True), ("ddim", False)]
    for B in (1, 3):
        cases = [(name, row, combos[i % 4]) for i, (name, row) in enumerate(list(_knobs(n).items())[:4])]
        cases += [("all", _knobs(n)["all"], cb) for cb in combos]
        for name, row, (kind, masked) in cases:
            mom_prev = R(NB - 1, B, n, seed=77) * 0.2 if row[3] != 0.0 else None
            run = Run(dev, dtype, NB, B, n, _tables(kind, steps), step, steps, _one_row_table(row, step, steps), masked, mom_prev)
            run.launch(history=kind == "dpm", noise=kind == "ddim")
            tag = f"apad_cfg_shaped_step {name} NB={NB} {dtype} B={B} n={n} {kind}{' mask' if masked else ''}"
            run.check_guards(tag, history=kind == "dpm")
            _check_against_oracle(run, [_f32(v) for v in row], tag)


def test_product_clip_bf16(dev):
    """B = 2 clips of 4000 pixels x 8 channels, bf16, three branches, all knobs, masked: the bench geometry's clip, once"""
    n, steps, step, NB, B, dtype = 32000, 4, 2, 3, 2, torch.bfloat16
    row = _knobs(n)["all"]
    run = Run(dev, dtype, NB, B, n, _tables("dpm", steps), step, steps, _one_row_table(row, step, steps), True, R(NB - 1, B, n, seed=77) * 0.2)
    run.launch(noise=False)
    run.check_guards("product clip")
    _check_against_oracle(run, [_f32(v) for v in row], "apad_cfg_shaped_step all NB=3 bf16 B=2 n=32000 dpm mask")


def _f16_ulp(v):
    _, e = torch.frexp(v.abs().double())
    return torch.clamp(torch.pow(2.0, (e - 11).double()), min=2.0 ** -24)


@pytest.mark.parametrize("NB", [2, 3])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", NS)
def test_all_off_row_is_the_existing_entry_points_bit_for_bit(dev, n, dtype, NB):
    """row (0, 1, 0, 0) against apad_cfg_sampler_step (no mask), apad_cfg_edit_step (mask) and apad_cfg_dual_step (three branches) from the same
    buffers on a table whose every column is non-zero: latents, unet_in, eps_out and history are the same bits.  B in {1, 3} keeps 8 | B n
    equivalent to 8 | n, so both kernels pick the same form.  The exception: two branches, f16, scalar form -- there the existing kernel leaves
    the fold of the f16 rounding into the fma to the compiler (guided_noise's comment) while this one rounds the fp32 value: eps may differ by
    one f16 ulp, and latents by |c_e| times that (times the mask, at most 1) plus 4 u of the summed term magnitudes."""
    from ap_adapter_amd import ops
    steps, step = 5, 2
    coef = R(steps, 6, seed=7) * 0.5 + 1.0
    for B in (1, 3):
        assert (B * n % 8 == 0) == (n % 8 == 0)
        for masked in (False, True):
            run = Run(dev, dtype, NB, B, n, coef, step, steps, _one_row_table(OFF, step, steps), masked, None)
            run.launch()
            run.check_guards(f"all-off NB={NB} {dtype} B={B} n={n} mask={masked}")
            lat, hist = run.x.to(dev), run.h.to(dev)
            unet_in, eps_out = torch.empty(B, n, dtype=dtype, device=dev), torch.empty(B, n, device=dev)
            eps_d, kw = run.eps.to(dev, dtype), run.masked or {}
            if NB == 3:
                ops.cfg_dual_step(eps_d, lat, unet_in, coef.to(dev), run.gtab.to(dev), run.ptr, eps_out, hist, run.noise_d, **kw)
            elif masked:
                ops.cfg_edit_step(eps_d, lat, unet_in, coef.to(dev), kw["keep"], run.ptr, run.w[0], kw["x0"], kw["z0"], kw["mask"], kw["channels"],
                                  eps_out, hist, run.noise_d)
            else:
                ops.cfg_sampler_step(eps_d, lat, unet_in, coef.to(dev), run.ptr, run.w[0], eps_out, hist, run.noise_d)
            assert torch.equal(run.stats.cpu(), torch.tensor([[1.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0]] * B))
            if NB == 2 and dtype == torch.float16 and not _is_vec(n):
                de = (run.eps_out - eps_out).abs().double().cpu()
                assert bool((de <= _f16_ulp(eps_out.cpu())).all())
                c_x, c_e, c_m, c_z, d_x, d_e = (abs(float(v)) for v in coef[step])
                mag = c_x * run.x.abs() + c_e * eps_out.cpu().abs() + c_m * run.h.abs() + c_z * run.z[step].abs()
                assert bool(((run.lat - lat).abs().double().cpu() <= c_e * de + 4 * U * mag.double()).all())
                assert bool(((run.hist - hist).abs().double().cpu() <= d_e * de + 4 * U * (d_x * run.x.abs() + d_e * eps_out.cpu().abs()).double()).all())
                continue
            for what, a, b in (("latents", run.lat, lat), ("unet_in", run.unet_in, unet_in), ("eps_out", run.eps_out, eps_out), ("history", run.hist, hist)):
                assert torch.equal(a, b), (what, B, masked, rel_err(a, b))


@pytest.mark.parametrize("NB", [2, 3])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", NS)
def test_a_clip_does_not_depend_on_its_batch(dev, n, dtype, NB):
    """all knobs on, per-clip mask: a clip alone and the same clip as the second of three give the same bits in latents, unet_in, eps_out,
    history, momentum and stats"""
    steps, step, K = 4, 2, NB - 1
    row = _knobs(n)["all"]
    coef = R(steps, 6, seed=7) * 0.5 + 1.0
    big = Run(dev, dtype, NB, 3, n, coef, step, steps, _one_row_table(row, step, steps), True, R(K, 3, n, seed=77) * 0.2).launch()
    one = Run(dev, dtype, NB, 1, n, coef, step, steps, _one_row_table(row, step, steps), True, big.mom_prev[:, 1:2].contiguous(),
              eps=big.eps.reshape(NB, 3, n)[:, 1].contiguous())
    for name in ("x", "h", "x0", "z0"):
        setattr(one, name, getattr(big, name)[1:2].contiguous())
    one.z, one.mask = big.z[:, 1:2].contiguous(), big.mask[1:2].contiguous()
    one.lat.copy_(one.x)
    one.hist.copy_(one.h)
    one.masked = dict(keep=big.masked["keep"], x0=one.x0.to(dev), z0=one.z0.to(dev), mask=one.mask.to(dev), channels=big.C)
    one.launch()
    for what, a, b in (("latents", one.lat, big.lat[1:2]), ("unet_in", one.unet_in, big.unet_in[1:2]), ("eps_out", one.eps_out, big.eps_out[1:2]),
                       ("history", one.hist, big.hist[1:2]), ("momentum", one.mom, big.mom[:, 1:2]), ("stats", one.stats, big.stats[1:2])):
        assert torch.equal(a, b), (what, rel_err(a, b))
    assert bool(torch.isfinite(big.lat).all()) and not torch.equal(big.stats[0], big.stats[1])


@pytest.mark.parametrize("NB", [2, 3])
@pytest.mark.parametrize("n", [8 * 65, 1001])
def test_three_consecutive_steps_select_rows_and_carry_the_momentum(dev, n, NB):
    """bf16, the counter advanced on the device: rows (phi, eta, r, beta) differ per step and each step matches the restatement fed with the
    momentum the previous launch left; then a counter past the table reads its last row; a beta == 0 row leaves a NaN-filled momentum buffer
    untouched; and a phi == 0, eta == 1, r == 0 row leaves stats at (1, 0, 1, 0, 0, 0, 0, 1)."""
    from ap_adapter_amd import ops
    dtype, B, steps, K = torch.bfloat16, 3, 3, NB - 1
    r = 0.15 * math.sqrt(n)
    rows = [(0.7, 0.25, r, -0.5), (0.0, 0.5, 0.0, 0.25), (1.0, 1.0, 2 * r, -0.75)]
    table = torch.tensor(rows)
    coef = _tables("dpm", steps)
    gtab = torch.tensor([[1.0, 4.0], [2.5, 7.5], [4.0, 3.0]]) if NB == 3 else None
    mom = torch.zeros(K, B, n)
    x, h = R(B, n, seed=110), torch.zeros(B, n)
    ptr = torch.zeros(1, dtype=torch.int32, device=dev)
    for s in range(steps + 1):
        srow = min(s, steps - 1)  # the fourth launch runs with the counter at 3: the clamp
        run = Run(dev, dtype, NB, B, n, coef, s, steps, table, False, mom, seed=200 + s, gtab=gtab)
        run.x, run.h = x, h
        run.lat.copy_(x)
        run.hist.copy_(h)
        run.ptr = ptr
        if NB == 3:
            run.w = tuple(float(v) for v in gtab[srow])
        assert int(ptr.item()) == s
        run.launch(noise=False)
        run.check_guards(f"step {s}")
        _check_against_oracle(run, [_f32(v) for v in rows[srow]], f"apad_cfg_shaped_step consecutive NB={NB} n={n} step {s}")
        mom, x, h = run.mom.cpu().clone(), run.lat.cpu().clone(), run.hist.cpu().clone()
        ops.step_advance(ptr)
    # beta == 0 with the other knobs on: the momentum buffer is neither read nor written
    nan = nan_buffer(K * B * n, torch.float32, dev).view(K, B, n).cpu()
    row = (0.7, 0.25, r, 0.0)
    run = Run(dev, dtype, NB, B, n, coef, 1, steps, _one_row_table(row, 1, steps), True, nan).launch(noise=False)
    run.check_guards("beta == 0")
    _check_against_oracle(run, [_f32(v) for v in row], f"apad_cfg_shaped_step beta=0 NB={NB} n={n}")
    assert bool(torch.isfinite(run.lat).all()) and bool(torch.isnan(run.mom).all())
    # momentum only: pass 1 runs for the state alone, and the stats stay at their defined values
    row = (0.0, 1.0, 0.0, -0.5)
    run = Run(dev, dtype, NB, B, n, coef, 1, steps, _one_row_table(row, 1, steps), False, R(K, B, n, seed=78)).launch(noise=False)
    assert torch.equal(run.stats.cpu(), torch.tensor([[1.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0]] * B))
    _check_against_oracle(run, [_f32(v) for v in row], f"apad_cfg_shaped_step beta only NB={NB} n={n}")


def test_shaped_step_rejects_bad_operands(dev):
    """RuntimeError from the wrapper, status + message from the entry point; nothing is launched"""
    from ap_adapter_amd import _lib as L
    from ap_adapter_amd import ops
    B, n, steps = 2, 64, 3
    lat = torch.full((B, n), 1.5, device=dev)
    eps2 = torch.zeros(2 * B, n, dtype=torch.bfloat16, device=dev)
    unet_in = torch.full((B, n), 3.0, dtype=torch.bfloat16, device=dev)
    ptr = torch.zeros(1, dtype=torch.int32, device=dev)
    coef, shape, gtab = torch.ones(steps, 6, device=dev), torch.tensor([list(OFF)] * steps, device=dev), torch.ones(steps, 2, device=dev)
    with pytest.raises(RuntimeError, match="guidance_scale .* or the guidance table"):
        ops.cfg_shaped_step(eps2, lat, unet_in, coef, shape, ptr)
    with pytest.raises(RuntimeError, match="guidance_scale .* or the guidance table"):
        ops.cfg_shaped_step(eps2, lat, unet_in, coef, shape, ptr, 7.5, gtab)
    for bad in (torch.ones(steps, 3, device=dev), torch.ones(steps - 1, 4, device=dev), torch.ones(steps, 4, device=dev, dtype=torch.float64),
                torch.ones(steps, 8, device=dev)[:, ::2]):
        with pytest.raises(RuntimeError, match="shape"):
            ops.cfg_shaped_step(eps2, lat, unet_in, coef, bad, ptr, 7.5)
    with pytest.raises(RuntimeError, match="shape: required"):
        ops.cfg_shaped_step(eps2, lat, unet_in, coef, None, ptr, 7.5)
    with pytest.raises(RuntimeError, match="momentum"):
        ops.cfg_shaped_step(eps2, lat, unet_in, coef, shape, ptr, 7.5, momentum=torch.zeros(2, B, n, device=dev))
    with pytest.raises(RuntimeError, match="stats"):
        ops.cfg_shaped_step(eps2, lat, unet_in, coef, shape, ptr, 7.5, stats=torch.zeros(B, 4, device=dev))
    with pytest.raises(RuntimeError, match="two branches"):
        ops.cfg_shaped_step(eps2[:B], lat, unet_in, coef, shape, ptr, 7.5)
    with pytest.raises(RuntimeError, match="three branches"):
        ops.cfg_shaped_step(eps2, lat, unet_in, coef, shape, ptr, None, gtab)
    lib = L.lib()
    args = lambda sh, br, dt: (eps2.data_ptr(), lat.data_ptr(), unet_in.data_ptr(), None, None, None, coef.data_ptr(), None, sh, None, None, None, None,
                               None, None, 0, 8, ptr.data_ptr(), steps, 7.5, br, B, n, dt, None)
    assert lib.apad_cfg_shaped_step(*args(None, 2, L.BF16)) != 0 and b"apad_cfg_shaped_step: null shape table" in lib.apad_last_error()
    assert lib.apad_cfg_shaped_step(*args(shape.data_ptr(), 4, L.BF16)) != 0 and b"branches = 4 must be 2 or 3" in lib.apad_last_error()
    assert lib.apad_cfg_shaped_step(*args(shape.data_ptr(), 3, L.BF16)) != 0 and b"apad_cfg_shaped_step: null guidance table" in lib.apad_last_error()
    assert lib.apad_cfg_shaped_step(*args(shape.data_ptr(), 2, 7)) != 0 and b"apad_cfg_shaped_step: dtype 7 not supported" in lib.apad_last_error()
    torch.cuda.synchronize()
    assert bool((lat == 1.5).all()) and bool((unet_in == 3.0).all())
    # a beta != 0 row without a momentum buffer reads as beta == 0 (never a null dereference)
    shape[:, 3] = -0.5
    a, b = lat.clone(), lat.clone()
    ops.cfg_shaped_step(eps2, a, unet_in, coef, shape, ptr, 7.5)
    shape[:, 3] = 0.0
    ops.cfg_shaped_step(eps2, b, unet_in, coef, shape, ptr, 7.5)
    assert torch.equal(a, b)


# ---------------------------------------------------------------------------------------------------------------------
# pipeline level (small synthetic UNet)
# ---------------------------------------------------------------------------------------------------------------------
KNOBS = dict(guidance_rescale=0.7, apg_eta=0.25, apg_norm_threshold=0.5, apg_momentum=-0.5)


def _inputs(dev, dtype, B=2, H=26, W=16, seed=2):
    lat = torch.randn(B, 8, H, W, generator=torch.Generator().manual_seed(seed))
    ehs, ehs1, m1 = _cond(2 * B, 32, dtype, seed=seed)
    return lat.to(dev), ehs.to(dev), ehs1.to(dev), m1.to(dev)


def _sched(sampler):
    import ap_adapter_amd as A
    return A.DPMSolverMultistepScheduler() if sampler == "dpm" else A.DDIMScheduler()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("sampler", ["ddim", "dpm"])
def test_captured_equals_eager_and_a_sweep_replays_one_graph(dev, monkeypatch, sampler, dtype):
    """5 steps with every knob on: captured == eager bit for bit and only apad_cfg_shaped_step runs; other values, then per-step schedules,
    replay the one captured graph and change the result; a call without the keywords takes today's path -- no call of the new op, the same
    bits as a hand-driven loop over the existing op, its own graph key -- and equals the all-neutral shaped call bit for bit (DPM-Solver++;
    deterministic DDIM's default path is apad_cfg_ddim_step, which rounds differently)."""
    import ap_adapter_amd as A
    from ap_adapter_amd import ops
    u, cfg, sd, procs = _small_unet(dev, dtype)
    u.requires_grad_(False)
    B, steps, gs = 2, 5, 7.5
    inp = _inputs(dev, dtype, B=B)
    pipe = A.AudioLDM2Pipeline(u, scheduler=_sched(sampler))
    names = ("cfg_shaped_step", "cfg_ddim_step", "cfg_sampler_step", "cfg_edit_step", "cfg_dual_step")
    calls = _count(monkeypatch, names)
    cnt = lambda: tuple(len(calls[k]) for k in names)
    eager = pipe.denoise(*inp, steps, gs, use_graph=False, **KNOBS)
    assert cnt() == (steps, 0, 0, 0, 0) and pipe.last_guidance_stats.shape == (B, 8)
    graph = pipe.denoise(*inp, steps, gs, **KNOBS)
    assert (pipe.graph_captures, pipe.graph_hits) == (1, 0) and torch.equal(graph, eager) and bool(torch.isfinite(eager).all())
    stats = pipe.last_guidance_stats.clone()
    assert bool((stats[:, 0] <= 1.0).all()) and bool((stats[:, 7] > 0).all()) and bool((stats[:, 5] > 0).all())
    outs = [graph]
    sweep = [dict(KNOBS, guidance_rescale=0.3), dict(KNOBS, apg_eta=0.0), dict(KNOBS, apg_norm_threshold=0.1), dict(KNOBS, apg_momentum=-0.25),
             dict(guidance_rescale=[0.0, 0.0, 0.5, 0.7, 1.0], apg_eta=[1.0, 1.0, 0.5, 0.0, 0.0], apg_norm_threshold=[0.0, 0.8, 0.6, 0.4, 0.2],
                  apg_momentum=[-0.5, 0.0, 0.0, -0.5, -0.5])]
    for kw in sweep:
        outs.append(pipe.denoise(*inp, steps, gs, **kw))
        assert pipe.graph_captures == 1
        assert torch.equal(outs[-1], pipe.denoise(*inp, steps, gs, use_graph=False, **kw)), kw
    assert pipe.graph_hits == len(sweep)
    assert all(not torch.equal(outs[i], outs[j]) for i in range(len(outs)) for j in range(i))
    assert torch.equal(pipe.denoise(*inp, steps, gs, **KNOBS), graph) and pipe.graph_captures == 1  # the momentum started from zero again
    # without momentum the key says so: another graph, no momentum buffer
    no_mom = pipe.denoise(*inp, steps, gs, guidance_rescale=0.7)
    assert pipe.graph_captures == 2 and [k for k in pipe._graphs if ("shaped", False) in k] and [k for k in pipe._graphs if ("shaped", True) in k]
    assert all(e["momentum"] is None for k, e in pipe._graphs.items() if ("shaped", False) in k)
    # the call without the keywords
    before = cnt()
    default = pipe.denoise(*inp, steps, gs, use_graph=False)
    want = (0, steps, 0, 0, 0) if sampler == "ddim" else (0, 0, steps, 0, 0)
    assert tuple(a - b for a, b in zip(cnt(), before)) == want
    default_graph = pipe.denoise(*inp, steps, gs)
    assert pipe.graph_captures == 3 and torch.equal(default, default_graph) and cnt()[0] == before[0]
    assert sum(1 for k in pipe._graphs if any(isinstance(x, tuple) and x and x[0] == "shaped" for x in k)) == 2
    monkeypatch.undo()
    # ... is a hand-driven loop over the existing op
    sched = _sched(sampler)
    sched.set_timesteps(steps)
    plan = sched.sampler_plan(0.0)
    H, W = 26, 16
    x = inp[0].float().permute(0, 2, 3, 1).reshape(B, H * W, 8).contiguous()
    unet_in, ptr = x.to(dtype), torch.zeros(1, dtype=torch.int32, device=dev)
    hist = torch.zeros_like(x) if plan.needs_history else None
    with torch.no_grad():
        u.set_kv_cache(True)
        u.precompute_time_tables(sched.timesteps.to(dev), ptr)
        try:
            for _ in range(steps):
                eps2 = u.forward_nhwc(unet_in, H, W, None, inp[1].to(dtype), inp[2].to(dtype), None, inp[3], batch_repeat=2)
                if plan.legacy:
                    ops.cfg_ddim_step(eps2, x, unet_in, plan.table.to(dev), ptr, gs)
                else:
                    ops.cfg_sampler_step(eps2, x, unet_in, plan.table.to(dev), ptr, gs, None, hist)
                ops.step_advance(ptr)
        finally:
            u.clear_time_tables()
            u.set_kv_cache(False)
    assert torch.equal(default, x.reshape(B, H, W, 8).permute(0, 3, 1, 2))
    neutral = pipe.denoise(*inp, steps, gs, apg_eta=1.0)  # on, every value neutral: the all-off rows
    if sampler == "dpm":
        assert torch.equal(neutral, default)
    assert not torch.equal(no_mom, default)


def test_fp32_loop_follows_the_restated_loop_and_full_rescale_matches_the_std(dev, monkeypatch):
    """fp32 small UNet, 4 DDIM steps, every knob on: the latents against a float64 loop that feeds the ORACLE UNet's outputs (oracle/unet.py, the
    same weights) through the restated stage and the restated DDIM step.  Bar: the project's fp32 loop bar, 1e-3 of max |ref| (the north-star
    bound; test_gpu_invert's fp32 round trip and test_gpu_unet's five-step fp32 loop are held to it).  Then guidance_rescale = 1: at every
    step std g * f equals std c to fp32 rounding (f = fl(std c / std g): one rounding, u; asserted at 2 u), read from the stats."""
    import ap_adapter_amd as A
    from ap_adapter_amd import ops
    from oracle import unet as OU
    dtype = torch.float32
    u, cfg, sd, procs = _small_unet(dev, dtype)
    u.requires_grad_(False)
    B, H, W, steps, gs = 2, 26, 16, 4, 7.5
    lat, ehs, ehs1, m1 = _inputs(dev, dtype, B=B)
    pipe = A.AudioLDM2Pipeline(u)
    out = pipe.denoise(lat, ehs, ehs1, m1, steps, gs, **KNOBS)
    acp, ts = SO.acp64(), SO.grid(steps)
    geo = cfg.geometry_dict()
    x = lat.cpu().double()
    mom = torch.zeros(1, B, H * W * 8, dtype=torch.float64)
    nhwc = lambda t: t.permute(0, 2, 3, 1).reshape(t.shape[0], -1)
    for i in range(steps):
        eps2 = OU.unet_forward(sd, geo, torch.cat([x, x]).float(), torch.tensor(ts[i]), ehs.cpu(), ehs1.cpu(), None, m1.cpu(), procs)
        o = SG.shaped_guidance(nhwc(eps2), 2, (gs,), tuple(KNOBS.values()), mom)
        mom = o["momentum"]
        e = o["g"].reshape(B, H, W, 8).permute(0, 3, 1, 2)
        x = SO.ddim_step(x, e, None, i, ts, acp)
    err = rel_err(out, x.float())
    print(f"\n[shaped loop, fp32 small UNet, {steps} DDIM steps, all knobs] latents vs the restated loop on the oracle UNet: rel err {err:.3e}")
    _record("fp32_loop_rel_err_over_1e-3", err / 1e-3)
    assert err < 1e-3
    # phi = 1, step by step
    seen, real = [], ops.cfg_shaped_step

    def spy(*a, **kw):
        real(*a, **kw)
        seen.append(a[9].double().cpu())  # stats

    monkeypatch.setattr(ops, "cfg_shaped_step", spy)
    pipe.denoise(lat, ehs, ehs1, m1, steps, gs, use_graph=False, guidance_rescale=1.0)
    monkeypatch.undo()
    assert len(seen) == steps
    for st in seen:
        assert bool((st[:, 5] > 0).all()) and bool(((st[:, 5] * st[:, 7] - st[:, 6]).abs() <= 2 * U * st[:, 6]).all()), st
        assert torch.equal(st[:, :4], torch.tensor([[1.0, 0.0, 1.0, 0.0]] * B, dtype=torch.float64))


def test_the_stage_works_with_a_mask_and_with_audio_guidance(dev, monkeypatch):
    """bf16, 6 steps.  (a) source latents, strength 0.5, a per-clip mask, DPM-Solver++: the kept region ends as the source bit for bit, captured ==
    eager, keep_noise_pred returns the shaped noise.  (b) audio_guidance_scale: three branches through the same op, captured == eager, one
    graph for two settings."""
    import ap_adapter_amd as A
    dtype = torch.bfloat16
    u, cfg, sd, procs = _small_unet(dev, dtype)
    u.requires_grad_(False)
    B, H, W, N, gs = 2, 26, 16, 6, 7.5
    lat, ehs, ehs1, m1 = _inputs(dev, dtype, B=B)
    calls = _count(monkeypatch, ("cfg_shaped_step", "cfg_edit_step", "cfg_dual_step", "cfg_sampler_step"))
    pipe = A.AudioLDM2Pipeline(u, scheduler=A.DPMSolverMultistepScheduler())
    x0, z0 = R(B, 8, H, W, seed=70, std=0.7).to(dev), R(B, 8, H, W, seed=71).to(dev)
    mask = torch.zeros(B, 1, H, W, device=dev)
    mask[0, :, 5:15] = 1.0
    mask[1, :, 10:20] = 1.0
    k = pipe.scheduler.edit_start_index(N, 0.5)
    a = pipe.denoise(None, ehs, ehs1, m1, N, gs, source=(x0, z0, mask), start=k, keep_noise_pred=True, **KNOBS)
    shaped_eps = pipe.last_noise_pred.clone()
    b = pipe.denoise(None, ehs, ehs1, m1, N, gs, source=(x0, z0, mask), start=k, use_graph=False, keep_noise_pred=True, **KNOBS)
    kept = (mask == 0).expand(B, 8, H, W)
    assert torch.equal(a, b) and torch.equal(a[kept], x0[kept]) and not bool((a[~kept] == x0[~kept]).any())
    assert torch.equal(shaped_eps, pipe.last_noise_pred) and bool(torch.isfinite(shaped_eps).all())
    plain = pipe.denoise(None, ehs, ehs1, m1, N, gs, source=(x0, z0, mask), start=k, use_graph=False, keep_noise_pred=True)
    assert not torch.equal(pipe.last_noise_pred, shaped_eps) and not torch.equal(plain, a)
    assert len(calls["cfg_shaped_step"]) == 2 + (N - k) and len(calls["cfg_edit_step"]) == N - k  # (2: the warm-up step and the capture)
    with pytest.raises(ValueError, match="^apg_norm_threshold.*needs apg_eta"):
        pipe.denoise(None, ehs, ehs1, m1, N, gs, source=(x0, z0, mask), start=k, apg_norm_threshold=2.0)
    with pytest.raises(ValueError, match="^guidance_rescale holds 3"):
        pipe.denoise(lat, ehs, ehs1, m1, N, gs, guidance_rescale=[0.5] * 3)
    # (b) three branches
    neg, pos = ehs[:B], ehs[B:]
    ehs3 = torch.cat([neg, torch.cat([neg[:, :8], pos[:, 8:]], 1), pos])
    pe3, am3 = torch.cat([ehs1[:B], ehs1]), torch.cat([m1[:B], m1])
    n0 = (len(calls["cfg_shaped_step"]), len(calls["cfg_dual_step"]))
    caps = pipe.graph_captures
    c = pipe.denoise(lat, ehs3, pe3, am3, N, gs, audio_guidance_scale=2.5, **KNOBS)
    d = pipe.denoise(lat, ehs3, pe3, am3, N, gs, audio_guidance_scale=2.5, use_graph=False, **KNOBS)
    e = pipe.denoise(lat, ehs3, pe3, am3, N, [gs] * N, audio_guidance_scale=1.0, **dict(KNOBS, guidance_rescale=0.2))
    assert torch.equal(c, d) and not torch.equal(c, e) and pipe.graph_captures == caps + 1 and bool(torch.isfinite(c).all())
    assert len(calls["cfg_dual_step"]) == n0[1] and len(calls["cfg_shaped_step"]) == n0[0] + 2 + N
    assert pipe.last_guidance_stats.shape == (B, 8) and bool((pipe.last_guidance_stats[:, 2] <= 1.0).all())
    assert not torch.equal(c, pipe.denoise(lat, ehs3, pe3, am3, N, gs, audio_guidance_scale=2.5))
