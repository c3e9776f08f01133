"""fp64 restatement of the denoise loop's two samplers for the tests.  TEST INFRASTRUCTURE ONLY.

**PARITY UNPINNED** (diffusers 0.21.2 is not installed; restated from the published formulas): written step by step from the
closed forms, with explicit m0 / m1 / h / r0 -- NOT from the linear-coefficient table of ``ap_adapter_amd/scheduler.py`` and sharing
no code with it, so that the table is checked against something other than itself.  The alphas_cumprod table and the timestep grid
come from ``oracle/ddim.py`` (fp32 cumprod of the scaled-linear betas; leading spacing, offset 1).

  alpha_t = sqrt(acp_t), sigma_t = sqrt(1 - acp_t), lambda_t = log alpha_t - log sigma_t   (integer timestep t)

DPM-Solver++ (2M), data prediction, midpoint (Lu et al. 2022): a step from t goes to the next grid entry, the last one to timestep 0;
  m0 = (x - sigma_t eps) / alpha_t,  h = lambda_prev - lambda_t
  first order   x' = (sigma_prev / sigma_t) x - alpha_prev (exp(-h) - 1) m0
                (step 0; solver_order 1; the final step when lower_order_final and fewer than 15 steps)
  second order  x' = (sigma_prev / sigma_t) x - alpha_prev (exp(-h) - 1) (m0 + 0.5 (m0 - m1) / r0),  r0 = (lambda_t - lambda_tprev) / h

DDIM with eta (Song et al. 2020; diffusers ``DDIMScheduler.step``): prev = t - 1000 // N (below 0: alphas_cumprod[0], the AudioLDM2
config's set_alpha_to_one = False),
  var = (1 - a_prev) / (1 - a_t) (1 - a_t / a_prev), std = eta sqrt(var), x0 = (x - sqrt(1 - a_t) eps) / sqrt(a_t)
  x' = sqrt(a_prev) x0 + sqrt(1 - a_prev - std^2) eps + std z
"""
import math

import torch

from oracle import ddim

T_TRAIN = ddim.SCHED["num_train_timesteps"]


def acp64():
    return [float(a) for a in ddim.alphas_cumprod().double()]


def grid(n):
    return [int(t) for t in ddim.timesteps(n)]


def _asl(acp, t):
    a, s = math.sqrt(acp[t]), math.sqrt(1.0 - acp[t])
    return a, s, math.log(a) - math.log(s)


def dpm_step(x, eps, m1, i, ts, acp, solver_order=2, lower_order_final=True):
    """step i of the grid ``ts``: (x' , m0), all float64; ``m1`` is the previous step's m0 (unused on a first-order step)"""
    x, eps = x.double(), eps.double()
    n = len(ts)
    a_t, s_t, lam_t = _asl(acp, ts[i])
    a_p, s_p, lam_p = _asl(acp, ts[i + 1] if i + 1 < n else 0)
    h = lam_p - lam_t
    m0 = (x - s_t * eps) / a_t
    first = i == 0 or solver_order == 1 or (lower_order_final and n < 15 and i == n - 1)
    if first:
        d = m0
    else:
        r0 = (lam_t - _asl(acp, ts[i - 1])[2]) / h
        d = m0 + 0.5 * (m0 - m1.double()) / r0
    return (s_p / s_t) * x - a_p * (math.exp(-h) - 1.0) * d, m0


def ddim_step(x, eps, z, i, ts, acp, eta=0.0):
    """step i of the grid ``ts`` (float64); ``z`` may be None when eta = 0"""
    x, eps = x.double(), eps.double()
    a_t = acp[ts[i]]
    p = ts[i] - T_TRAIN // len(ts)
    a_p = acp[p] if p >= 0 else acp[0]
    std = eta * math.sqrt((1.0 - a_p) / (1.0 - a_t) * (1.0 - a_t / a_p))
    x0 = (x - math.sqrt(1.0 - a_t) * eps) / math.sqrt(a_t)
    out = math.sqrt(a_p) * x0 + math.sqrt(1.0 - a_p - std * std) * eps
    return out if std == 0.0 else out + std * z.double()


def dpm_loop(x, eps_fn, ts, acp, **kw):
    """eps_fn(i, t, x) -> eps; returns the final x (float64)"""
    m1 = None
    x = x.double()
    for i, t in enumerate(ts):
        x, m1 = dpm_step(x, eps_fn(i, t, x), m1, i, ts, acp, **kw)
    return x


def ddim_loop(x, eps_fn, ts, acp, eta=0.0, noise=None):
    x = x.double()
    for i, t in enumerate(ts):
        x = ddim_step(x, eps_fn(i, t, x), None if noise is None else noise[i], i, ts, acp, eta)
    return x


def cfg_combine_rounded(eps2, guidance_scale, dtype):
    """the guided noise in the model dtype (eps2 holds storage-rounded values), with the kernels' fp32 arithmetic spelled out: the
    difference rounded to fp32, ONE fused multiply-add (the product of two fp32 values is exact in float64), one rounding to ``dtype``.
    torch's separate fp32 multiply and add differ from the fma in the last fp32 bit where an operand is ~2^13 times smaller than the
    other, and a 16-bit rounding tie then falls the other way -- a whole f16 ulp, seen once in 480 000 values."""
    u, c = eps2.float().chunk(2)
    d = c - u
    e32 = (float(torch.tensor(guidance_scale, dtype=torch.float32)) * d.double() + u.double()).float()
    return e32.to(dtype).double()


# ---- the analytic problem: data x0 ~ N(0, s^2) ----
def gaussian_eps(acp, s):
    """exact noise prediction eps*(x, t) = sigma_t x / (alpha_t^2 s^2 + sigma_t^2)"""
    def fn(i, t, x):
        a, sg, _ = _asl(acp, t)
        return sg * x / (a * a * s * s + sg * sg)
    return fn


def gaussian_ode_solution(x_T, t_from, t_to, acp, s):
    """x_t = x_T sqrt(alpha_t^2 s^2 + sigma_t^2) / sqrt(alpha_T^2 s^2 + sigma_T^2)"""
    v = lambda t: acp[t] * s * s + (1.0 - acp[t])
    return x_T * math.sqrt(v(t_to)) / math.sqrt(v(t_from))
