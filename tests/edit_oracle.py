"""fp64 restatement of editing from a source clip -- the strength start, the sliced loops and the region blend -- for the tests.
TEST INFRASTRUCTURE ONLY.

**PARITY UNPINNED** (diffusers is not installed, and the reference's own attempt, pipeline/style_transfer_pipeline.py:908-936, does not
import): diffusers' img2img / inpaint conventions written from their closed forms, step by step, on top of ``sampler_oracle.dpm_step``
/ ``ddim_step`` -- NOT from the coefficient or keep tables of ``ap_adapter_amd/scheduler.py`` and sharing no code with them.

  N steps on the grid ts (leading spacing, offset 1).  An edit of ``strength`` in (0, 1] runs the last min(int(N strength), N) steps:
  it enters the grid at k = N - that.
  start       x_k = sqrt(acp[ts[k]]) x0 + sqrt(1 - acp[ts[k]]) z0                                  (add_noise)
  step i      g = sampler step at grid index k + i, exactly as in the full run -- DDIM's previous timestep stays ts - 1000 // N, the
              multistep solver's lower_order_final keeps judging by N -- except that the solver's history is empty on entry, so its step
              i = 0 is first order
  blend       x' = m g + (1 - m) known_i ,  known_i = add_noise(x0, z0, ts[k + i + 1]), and known = x0 after the last step;
              m in [0, 1], 1 = regenerate, 0 = keep; z0 is the noise of the start (deterministic, no per-step draw)
  The data prediction handed to the next step is formed from the pre-blend x and eps.
"""
import math

import sampler_oracle as SO


def start_index(n, strength):
    run = min(int(n * strength), n)
    assert run > 0, (n, strength)
    return n - run


def add_noise(x0, z0, t, acp):
    return math.sqrt(acp[t]) * x0.double() + math.sqrt(1.0 - acp[t]) * z0.double()


def known(x0, z0, i, k, ts, acp):
    """the source at the noise level step i of the slice lands on"""
    j = k + i + 1
    return x0.double() if j >= len(ts) else add_noise(x0, z0, ts[j], acp)


def blend(g, m, x0, z0, i, k, ts, acp):
    m = m.double()
    return m * g.double() + (1.0 - m) * known(x0, z0, i, k, ts, acp)


def dpm_edit_step(x, eps, m1, i, k, ts, acp, solver_order=2, lower_order_final=True):
    """step i of the slice ts[k:]: (g, m0), before the blend"""
    if i == 0:  # empty history
        return SO.dpm_step(x, eps, None, k, ts, acp, solver_order=1)
    return SO.dpm_step(x, eps, m1, k + i, ts, acp, solver_order=solver_order, lower_order_final=lower_order_final)


def ddim_edit_step(x, eps, z, i, k, ts, acp, eta=0.0):
    return SO.ddim_step(x, eps, z, k + i, ts, acp, eta)


def edit_loop(x0, z0, mask, eps_fn, n, strength, acp, sampler="dpm", eta=0.0, noise=None, **kw):
    """the whole run: eps_fn(i, t, x) -> eps with i counting within the slice and t = ts[k + i]; ``noise[i]`` is DDIM's z of step i;
    ``mask`` None = strength only.  Returns the final x (float64)."""
    ts = SO.grid(n)
    k = start_index(n, strength)
    x = add_noise(x0, z0, ts[k], acp)
    m1 = None
    for i in range(n - k):
        eps = eps_fn(i, ts[k + i], x)
        if sampler == "dpm":
            x, m1 = dpm_edit_step(x, eps, m1, i, k, ts, acp, **kw)
        else:
            x = ddim_edit_step(x, eps, None if noise is None else noise[i], i, k, ts, acp, eta)
        if mask is not None:
            x = blend(x, mask, x0, z0, i, k, ts, acp)
    return x
