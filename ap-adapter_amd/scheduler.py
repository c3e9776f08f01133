"""Scheduler state for the denoise loop.

``DDIMScheduler``: diffusers==0.21.2 DDIMScheduler semantics with the AudioLDM2 scheduler_config: scaled_linear betas
0.0015..0.0195, 1000 train steps, leading spacing, steps_offset 1, set_alpha_to_one False, epsilon prediction; call sites
/root/reference/pipeline/pipeline_audioldm2.py:983-984, :1007, :1025.  ``eta`` is a per-call value as in the reference
(``prepare_extra_step_kwargs``, :617-632).

``DPMSolverMultistepScheduler``: DPM-Solver++ (2M), data-prediction form, midpoint (Lu et al. 2022), in diffusers'
conventions.  The reference pipeline accepts any ``KarrasDiffusionSchedulers`` member (:158); this is the second one here.

The per-step update itself runs on the device from a coefficient table (``apad_cfg_ddim_step`` for deterministic DDIM,
``apad_cfg_sampler_step`` for everything else, ``apad_cfg_edit_step`` with a region mask: ``apad_cfg_dual_step`` for the three-branch step
with separate audio and text guidance, ``sampler_plan(dual=True)`` + ``guidance_table``: four entry points onto one kernel, whose rounding
form per entry point is written out in csrc/elementwise.hip's ``guided_noise`` and ``sampler_update``), which removes the reference's per-step
host<->device sync inside ``scheduler.step``.  Every update here is LINEAR in (x, eps, previous data prediction m1, fresh noise z), so one row of six
coefficients per step describes it (``SAMPLER_COLS``); ``sampler_plan`` tells the loop which kernel, table and per-sampler buffers
a call needs.

An edit run (a source clip noised to an interior timestep, optionally with a region mask; ``edit_start_index``, ``_EditSchedule``,
``sampler_plan(start=, masked=)``) enters the same grid at index k and uses rows ``k:`` of the same tables.

Edit-friendly DDPM inversion (``DDIMScheduler.inversion_plan``, ``apad_cfg_invert_step``; Huberman-Spiegelglas et al. 2024) reads the
same ``eta`` > 0 rows and the same ``keep`` table on the same slice: it extracts the noise those rows would consume.

Guidance rescale and adaptive projected guidance (``shape_table``, ``apad_cfg_shaped_step``; Lin et al. 2024, Sadat et al. 2024) read the
same six-column tables; their own per-step values (phi, eta, r, beta) are one more device table on the same slice.

PARITY UNPINNED: the ``eta`` arithmetic and the multistep solver are restated from the published formulas (diffusers is not
vendored and not installable offline); ``tests/sampler_oracle.py`` restates them a second time, independently, in float64."""
import math
from dataclasses import dataclass

import numpy as np
import torch

# one table row: x' = c_x x + c_eps eps + c_m1 m1 + c_z z ;  m0 = d_x x + d_eps eps (the data prediction kept for the next step)
SAMPLER_COLS = ("c_x", "c_eps", "c_m1", "c_z", "d_x", "d_eps")


@dataclass
class SamplerPlan:
    """what one denoise call asks of the loop: ``table`` fp32 [steps, 2] for apad_cfg_ddim_step when ``legacy`` (the deterministic
    DDIM path every earlier caller takes), else fp32 [steps, 6] for apad_cfg_sampler_step; whether a data-prediction history buffer
    and a per-step noise buffer are needed; ``key`` is the scheduler's share of the captured graph's cache key.  An edit run
    (``sampler_plan(start=, masked=)``) visits ``timesteps[start:]``: ``table`` then holds the rows of those steps only, and with
    ``masked`` ``keep`` is the fp32 [steps - start, 2] table of apad_cfg_edit_step"""
    table: torch.Tensor
    legacy: bool
    needs_history: bool
    needs_noise: bool
    key: tuple
    keep: torch.Tensor = None
    start: int = 0


def edit_start_index(num_inference_steps, strength):
    """diffusers' img2img ``get_timesteps``: an edit of ``strength`` in (0, 1] runs the last ``min(int(N * strength), N)`` of the N steps,
    i.e. starts at index k = N - that.  strength 0.5 with 4 | N is the k = N // 4 * 2 of the reference's unfinished style-transfer loop
    (pipeline/style_transfer_pipeline.py:908-936)."""
    n = int(num_inference_steps)
    if not 0.0 < float(strength) <= 1.0:
        raise ValueError(f"strength={strength!r} must lie in (0, 1]")
    run = min(int(n * float(strength)), n)
    if run == 0:
        raise ValueError(f"strength={strength!r} leaves no step to run at num_inference_steps={n} (int(N * strength) == 0)")
    return n - run


def guidance_table(audio, text, num_inference_steps, start=0):
    """fp32 [N - start, 2], row i = (s_A, s_T) of step ``start + i``: the table apad_cfg_dual_step reads at ``*step_ptr``.  ``audio`` / ``text``:
    a float (every step) or a sequence of exactly N floats over the FULL grid -- a per-step guidance schedule -- of which rows ``start:`` are
    kept, like the coefficient table of an edit run.  Every value must be finite and >= 0 (rows before ``start`` are not used and not
    checked); a ValueError names the argument."""
    n, start = int(num_inference_steps), int(start)
    if not 0 <= start < n:
        raise ValueError(f"start={start!r} must lie in [0, {n})")
    cols = []
    for name, v in (("audio", audio), ("text", text)):
        if isinstance(v, torch.Tensor):
            v = v.detach().cpu().tolist()
        try:
            vals = [float(v)] * n if not hasattr(v, "__len__") else [float(x) for x in v]
        except (TypeError, ValueError):
            raise ValueError(f"{name}={v!r}: expected a float or a sequence of {n} floats") from None
        if len(vals) != n:
            raise ValueError(f"{name} holds {len(vals)} values; a per-step sequence needs exactly num_inference_steps = {n}")
        vals = vals[start:]
        if not all(math.isfinite(x) and x >= 0.0 for x in vals):
            raise ValueError(f"{name}={v!r}: every guidance value must be finite and >= 0")
        cols.append(vals)
    return torch.tensor(cols, dtype=torch.float64).t().float().contiguous()


SHAPE_COLS = ("guidance_rescale", "apg_eta", "apg_norm_threshold", "apg_momentum")  # one row of shape_table: (phi, eta, r, beta)


def shape_table(guidance_rescale, apg_eta, apg_norm_threshold, apg_momentum, num_inference_steps, start=0):
    """fp32 [N - start, 4], row i = (phi, eta, r, beta) of step ``start + i``: the table apad_cfg_shaped_step reads at ``*step_ptr`` (guidance
    rescale, Lin et al. 2024; adaptive projected guidance, Sadat et al. 2024: PAPERS.md).  Each argument is a float (every step) or a sequence
    of exactly N floats over the FULL grid, of which rows ``start:`` are kept, like ``guidance_table``.  phi in [0, 1] (0 = no rescale), eta any
    finite value (1 = no projection), r >= 0 (0 = no norm threshold), |beta| < 1 (0 = no momentum; APG uses negative values); a ValueError
    names the argument.  The row (0, 1, 0, 0) is plain classifier-free guidance."""
    n, start = int(num_inference_steps), int(start)
    if not 0 <= start < n:
        raise ValueError(f"start={start!r} must lie in [0, {n})")
    ok = {"guidance_rescale": (lambda x: 0.0 <= x <= 1.0, "must lie in [0, 1]"), "apg_eta": (lambda x: True, "must be finite"),
          "apg_norm_threshold": (lambda x: x >= 0.0, "must be >= 0"), "apg_momentum": (lambda x: abs(x) < 1.0, "must lie in (-1, 1)")}
    cols = []
    for name, v in zip(SHAPE_COLS, (guidance_rescale, apg_eta, apg_norm_threshold, apg_momentum)):
        if isinstance(v, torch.Tensor):
            v = v.detach().cpu().tolist()
        try:
            vals = [float(v)] * n if not hasattr(v, "__len__") else [float(x) for x in v]
        except (TypeError, ValueError):
            raise ValueError(f"{name}={v!r}: expected a float or a sequence of {n} floats") from None
        if len(vals) != n:
            raise ValueError(f"{name} holds {len(vals)} values; a per-step sequence needs exactly num_inference_steps = {n}")
        vals = vals[start:]
        if not all(math.isfinite(x) and ok[name][0](x) for x in vals):
            raise ValueError(f"{name}={v!r}: every value {ok[name][1]}")
        cols.append(vals)
    return torch.tensor(cols, dtype=torch.float64).t().float().contiguous()


def ap_scale_table(ap_scale, num_inference_steps, start=0, clips=None):
    """fp32 [N - start, cols], row i = the weight of the audio branch (``scale`` of attention_processor.py:454) at step ``start + i``: the table
    the decoupled cross-attention launches read at ``*step_ptr`` (apad_scale2_tab).  ``ap_scale``: a float (every step, every clip; cols = 1), a
    1-D sequence of exactly N floats over the FULL grid (a per-step schedule; a 1-D sequence is always per step; cols = 1), or a 2-D array-like
    / tensor [N, B] or [1, B] (per step and per clip, a single row broadcast over the steps; cols = B, which must equal ``clips`` = batch x
    num_waveforms_per_prompt, in generation order, when that is given).  Rows ``start:`` are kept, like ``guidance_table``; every kept value
    must be finite -- any finite value, negative included: the reference constrains nothing -- and entries before ``start`` are not read and may
    be NaN.  Errors are ValueErrors whose text starts with ``ap_scale``."""
    n, start = int(num_inference_steps), int(start)
    if not 0 <= start < n:
        raise ValueError(f"ap_scale: start={start!r} must lie in [0, {n})")
    v = ap_scale
    if isinstance(v, torch.Tensor):
        v = v.detach().cpu().tolist()
    try:
        two_d = hasattr(v, "__len__") and len(v) > 0 and all(hasattr(r, "__len__") for r in v)
        if not hasattr(v, "__len__"):
            rows = [[float(v)]] * n
        elif two_d:
            rows = [[float(x) for x in r] for r in v]
            if len(rows) == 1:
                rows = rows * n
        else:
            rows = [[float(x)] for x in v]
    except (TypeError, ValueError):
        raise ValueError(f"ap_scale={ap_scale!r}: expected a float, a sequence of {n} floats or a 2-D [{n} or 1, clips] array") from None
    if len(rows) != n:
        raise ValueError(f"ap_scale holds {len(rows)} rows; a per-step schedule needs exactly num_inference_steps = {n} (or ONE row of per-clip "
                         "values)")
    cols = len(rows[0])
    if cols < 1 or any(len(r) != cols for r in rows):
        raise ValueError("ap_scale: every row of a 2-D value must hold the same number (>= 1) of per-clip values")
    if two_d and clips is not None and cols != int(clips):
        raise ValueError(f"ap_scale holds {cols} per-clip values; the run generates {int(clips)} clips (batch x num_waveforms_per_prompt)")
    rows = rows[start:]
    if not all(math.isfinite(x) for r in rows for x in r):
        raise ValueError(f"ap_scale: every value from step {start} on must be finite")
    return torch.tensor(rows, dtype=torch.float64).float().contiguous()


def ap_mask_pyramid(mask, grids):
    """The per-token weight maps of the audio prompt for every attention level: ``mask`` fp32 [cols, 1, H, W] over the latent grid (the weight of
    the audio branch at each latent cell; any finite value), ``grids`` the (h, w) of the levels (``UNet.attention_grids(H, W)``).  Per level,
    ``adaptive_avg_pool2d`` of the mask to (h, w) -- a token's weight is the mean over the latent cells it covers -- flattened row-major to
    [cols, h * w], the token order of the processors' 4-D entry; computed on the host, once per call.  Returns {h * w: fp32 [cols, h * w]},
    what ``set_ap_token_weights`` takes (a processor picks its map by its token count).  The latent-grid mask of an ``ap_region`` is binary and
    so is a level whose pooling windows do not straddle the region's ends; a coarser level gets FRACTIONAL edge rows there (a window half
    inside weighs 0.5), and every pooled value of a mask in [0, 1] stays in [0, 1].  Errors are ValueErrors whose text starts with ``ap_mask``."""
    m = torch.as_tensor(mask).detach().to("cpu", torch.float32)
    if m.dim() != 4 or m.shape[1] != 1 or m.shape[0] < 1:
        raise ValueError(f"ap_mask: expected a [cols, 1, H, W] mask, got {tuple(m.shape)}")
    if not bool(torch.isfinite(m).all()):
        raise ValueError("ap_mask: every value must be finite")
    out = {}
    for h, w in grids:
        level = torch.nn.functional.adaptive_avg_pool2d(m, (int(h), int(w))).reshape(m.shape[0], int(h) * int(w)).contiguous()
        if int(h) * int(w) in out:
            raise ValueError(f"ap_mask: two attention levels hold {int(h) * int(w)} tokens; the maps are picked by the token count")
        out[int(h) * int(w)] = level
    return out


class _EditSchedule:
    """what an edit run needs of either scheduler (both share the timestep grid and alphas_cumprod): where it starts, the add_noise
    coefficients of the start and the per-step (kx, kz) of the kept region.  PARITY UNPINNED, like the samplers: diffusers' img2img /
    inpaint conventions restated from memory; tests/edit_oracle.py restates them a second time, independently, in float64."""
    edit_start_index = staticmethod(edit_start_index)

    def _check_start(self, start):
        n = len(self.timesteps)
        if not 0 <= int(start) < n:
            raise ValueError(f"start={start!r} must lie in [0, {n})")
        return int(start)

    def add_noise_coefs(self, start):
        """(a, s) of x_start = a x0 + s z0 at ``timesteps[start]``: (sqrt(acp_t), sqrt(1 - acp_t)), float64"""
        acp_t = float(self.alphas_cumprod.double()[int(self.timesteps[self._check_start(start)])])
        return math.sqrt(acp_t), math.sqrt(1.0 - acp_t)

    def keep_table(self, start=0):
        """fp32 [N - start, 2]: row i = (sqrt(acp_t), sqrt(1 - acp_t)) at t = timesteps[start + i + 1], the noise level step i lands
        on; the last row is (1, 0) -- the kept region ends as the source latents themselves"""
        acp = self.alphas_cumprod.double()
        ts = self.timesteps.tolist()[self._check_start(start) + 1:]
        rows = [[math.sqrt(float(acp[t])), math.sqrt(1.0 - float(acp[t]))] for t in ts] + [[1.0, 0.0]]
        return torch.tensor(rows, dtype=torch.float64).float()


def _scaled_linear_acp(num_train_timesteps, beta_start, beta_end):
    betas = torch.linspace(beta_start ** 0.5, beta_end ** 0.5, num_train_timesteps, dtype=torch.float32) ** 2
    return torch.cumprod(1.0 - betas, dim=0)


def _leading_timesteps(num_train_timesteps, num_inference_steps, steps_offset):
    ratio = num_train_timesteps // num_inference_steps
    return (np.arange(0, num_inference_steps) * ratio).round()[::-1].copy().astype(np.int64) + steps_offset


class DDIMScheduler(_EditSchedule):
    order = 1
    init_noise_sigma = 1.0

    def __init__(self, num_train_timesteps=1000, beta_start=0.0015, beta_end=0.0195, steps_offset=1,
                 set_alpha_to_one=False):
        self.num_train_timesteps = num_train_timesteps
        self.steps_offset = steps_offset
        self._betas = (beta_start, beta_end, bool(set_alpha_to_one))
        self.alphas_cumprod = _scaled_linear_acp(num_train_timesteps, beta_start, beta_end)
        self.final_alpha_cumprod = torch.tensor(1.0) if set_alpha_to_one else self.alphas_cumprod[0]
        self.timesteps = None
        self.num_inference_steps = None

    def set_timesteps(self, num_inference_steps, device=None):
        self.num_inference_steps = num_inference_steps
        ts = _leading_timesteps(self.num_train_timesteps, num_inference_steps, self.steps_offset)
        self.timesteps = torch.from_numpy(ts).to(device) if device is not None else torch.from_numpy(ts)

    def scale_model_input(self, sample, timestep=None):
        return sample

    def coef_table(self):
        """[steps, 2] fp32 (c_x, c_eps) with x_prev = c_x * x + c_eps * eps, i.e. DDIM eta=0:
        x0 = (x - sqrt(1-a_t) eps)/sqrt(a_t);  x_prev = sqrt(a_p) x0 + sqrt(1-a_p) eps.  Formed in float64."""
        acp = self.alphas_cumprod.double()
        ratio = self.num_train_timesteps // self.num_inference_steps
        rows = []
        for t in self.timesteps.tolist():
            a_t = acp[t]
            p = t - ratio
            a_p = acp[p] if p >= 0 else self.final_alpha_cumprod.double()
            c_x = (a_p / a_t).sqrt()
            c_e = (1 - a_p).sqrt() - (a_p / a_t).sqrt() * (1 - a_t).sqrt()
            rows.append([float(c_x), float(c_e)])
        return torch.tensor(rows, dtype=torch.float32)

    def sampler_rows(self, eta=0.0, timesteps=None):
        """[steps, 6] float64 rows (``SAMPLER_COLS``) of diffusers' ``DDIMScheduler.step`` with ``eta``:
        var = (1 - a_p) / (1 - a_t) * (1 - a_t / a_p), std = eta sqrt(var),
        x_prev = sqrt(a_p) x0 + sqrt(1 - a_p - std^2) eps + std z, x0 = (x - sqrt(1 - a_t) eps) / sqrt(a_t).
        The previous timestep is t - num_train_timesteps // steps (``final_alpha_cumprod`` below 0).  At eta = 0 the first two
        columns are the float64 values ``coef_table`` rounds.  ``timesteps`` (a list) replaces the scheduler's own grid."""
        acp = self.alphas_cumprod.double()
        ts = self.timesteps.tolist() if timesteps is None else [int(t) for t in timesteps]
        ratio = self.num_train_timesteps // len(ts)
        rows = []
        for t in ts:
            a_t = acp[t]
            p = t - ratio
            a_p = acp[p] if p >= 0 else self.final_alpha_cumprod.double()
            std = eta * ((1 - a_p) / (1 - a_t) * (1 - a_t / a_p)).sqrt()
            c_x = (a_p / a_t).sqrt()
            c_e = (1 - a_p - std ** 2).sqrt() - (a_p / a_t).sqrt() * (1 - a_t).sqrt()
            rows.append([float(c_x), float(c_e), 0.0, float(std), 0.0, 0.0])
        return torch.tensor(rows, dtype=torch.float64)

    def sampler_plan(self, eta=0.0, start=0, masked=False, dual=False):
        """eta = 0 keeps the two-column table and apad_cfg_ddim_step; eta > 0 needs one fresh noise tensor per step.  ``start`` > 0: rows
        ``start:`` of the FULL table (the previous timestep stays t - num_train_timesteps // N).  ``masked``: always the six-column
        table, plus ``keep``.  ``dual`` (the three-branch step, apad_cfg_dual_step): always the six-column table, ``sampler_rows(0.0)`` at
        eta = 0, and "dual" in ``key``."""
        eta = float(eta)
        start, masked = self._check_start(start), bool(masked)
        key = ("DDIMScheduler", self.order, "leading", self.num_train_timesteps, self.steps_offset, self._betas, eta)
        if start or masked:
            key += (start, masked)
        if dual:
            key += ("dual",)
        if eta == 0.0 and not masked and not dual:
            return SamplerPlan(self.coef_table()[start:].contiguous(), True, False, False, key, None, start)
        return SamplerPlan(self.sampler_rows(eta)[start:].float().contiguous(), False, False, eta != 0.0, key,
                           self.keep_table(start) if masked else None, start)

    def inversion_plan(self, eta, start=0, dual=False):
        """what edit-friendly DDPM inversion (apad_cfg_invert_step; Huberman-Spiegelglas et al. 2024) asks of the loop: rows
        ``start:`` of ``sampler_rows(eta)`` -- the table the edit phase's sampler step reads, whose std column the inversion divides by --
        ``keep_table(start)`` (the noise level each step lands on), one noise row per step, and "invert" in ``key``.  ``eta`` must be > 0:
        a deterministic step has no noise to invert into."""
        eta = float(eta)
        if not eta > 0.0:
            raise ValueError(f"eta={eta!r}: DDPM inversion extracts the per-step noise of a stochastic sampler and needs eta > 0 (pass eta=1.0)")
        start = self._check_start(start)
        key = ("DDIMScheduler", self.order, "leading", self.num_train_timesteps, self.steps_offset, self._betas, eta, start, "invert")
        if dual:
            key += ("dual",)
        return SamplerPlan(self.sampler_rows(eta)[start:].float().contiguous(), False, False, True, key, self.keep_table(start), start)


class DPMSolverMultistepScheduler(_EditSchedule):
    """DPM-Solver++ multistep (2M), epsilon prediction, data-prediction form, midpoint -- diffusers' class name, constructor keywords
    and attributes as far as they apply.  alpha_t = sqrt(acp_t), sigma_t = sqrt(1 - acp_t), lambda_t = log alpha_t - log sigma_t, all
    indexed by integer timestep; a step goes from ``timesteps[i]`` to ``timesteps[i + 1]`` and the last one to timestep 0 (the alpha of
    DDIMScheduler's ``final_alpha_cumprod``).

    Timestep grid -- a deliberate, UNPINNED choice: ``timesteps`` is DDIMScheduler's grid at the same step count (leading spacing,
    ratio ``num_train_timesteps // N``, ``steps_offset`` 1).  From memory diffusers 0.21.2 divides by ``N + 1`` for this class, which
    cannot be checked offline and would start a 200-step run at t = 801 instead of 996; sharing DDIM's grid makes both samplers visit the
    same timesteps and keeps the UNet's time tables identical.

    Not implemented (raise, name the argument): other ``algorithm_type`` / ``solver_type`` / ``timestep_spacing`` / ``prediction_type``,
    ``solver_order`` > 2, ``use_karras_sigmas``, ``thresholding``."""
    init_noise_sigma = 1.0

    def __init__(self, num_train_timesteps=1000, beta_start=0.0015, beta_end=0.0195, solver_order=2, prediction_type="epsilon",
                 thresholding=False, algorithm_type="dpmsolver++", solver_type="midpoint", lower_order_final=True,
                 use_karras_sigmas=False, timestep_spacing="leading", steps_offset=1):
        for name, value, ok in (("algorithm_type", algorithm_type, ("dpmsolver++",)), ("solver_type", solver_type, ("midpoint",)),
                                ("timestep_spacing", timestep_spacing, ("leading",)), ("solver_order", solver_order, (1, 2)),
                                ("prediction_type", prediction_type, ("epsilon",)), ("use_karras_sigmas", use_karras_sigmas, (False,)),
                                ("thresholding", thresholding, (False,))):
            if value not in ok:
                raise NotImplementedError(f"DPMSolverMultistepScheduler: {name}={value!r} is not implemented (supported: "
                                          f"{', '.join(repr(o) for o in ok)})")
        self.num_train_timesteps = num_train_timesteps
        self.steps_offset = steps_offset
        self.solver_order = int(solver_order)
        self.order = 1  # diffusers: ``order`` counts model evaluations per step, 1 for a multistep solver
        self.algorithm_type, self.solver_type, self.timestep_spacing = algorithm_type, solver_type, timestep_spacing
        self.lower_order_final = bool(lower_order_final)
        self.prediction_type = prediction_type
        self._betas = (beta_start, beta_end)
        self.alphas_cumprod = _scaled_linear_acp(num_train_timesteps, beta_start, beta_end)
        self.timesteps = None
        self.num_inference_steps = None

    def set_timesteps(self, num_inference_steps, device=None):
        self.num_inference_steps = num_inference_steps
        ts = _leading_timesteps(self.num_train_timesteps, num_inference_steps, self.steps_offset)
        self.timesteps = torch.from_numpy(ts).to(device) if device is not None else torch.from_numpy(ts)

    def scale_model_input(self, sample, timestep=None):
        return sample

    def sampler_rows(self, timesteps=None, start=0):
        """[steps - start, 6] float64 rows (``SAMPLER_COLS``).  With m0 = (x - sigma_t eps) / alpha_t = d_x x + d_eps eps, h = lambda_prev -
        lambda_t, A = sigma_prev / sigma_t and E = -alpha_prev (exp(-h) - 1):
          first order  (step 0, solver_order 1, the last step under lower_order_final with fewer than 15 steps):  x' = A x + E m0
          second order:  x' = A x + E (m0 + 0.5 (m0 - m1) / r0),  r0 = (lambda_t - lambda_tprev) / h
        expanded into c_x = A + E (1 + k) d_x, c_eps = E (1 + k) d_eps, c_m1 = -E k with k = 0.5 / r0 (0 on a first-order step).
        ``timesteps`` (a list) replaces the scheduler's own grid.  ``start`` > 0 (an edit run entering the grid at that index): rows
        ``start:`` of the same table, except that the history is empty on entry, so row ``start`` is first order; ``lower_order_final``
        keeps judging by the full step count."""
        acp = self.alphas_cumprod.double()
        ts = self.timesteps.tolist() if timesteps is None else [int(t) for t in timesteps]
        n = len(ts)
        al = lambda t: math.sqrt(float(acp[t]))
        sg = lambda t: math.sqrt(1.0 - float(acp[t]))
        lam = lambda t: math.log(al(t)) - math.log(sg(t))
        rows = []
        for i in range(start, n):
            t = ts[i]
            prev = ts[i + 1] if i + 1 < n else 0
            h = lam(prev) - lam(t)
            A = sg(prev) / sg(t)
            E = -al(prev) * math.expm1(-h)
            first = i == start or self.solver_order == 1 or (self.lower_order_final and n < 15 and i == n - 1)
            k = 0.0 if first else 0.5 * h / (lam(t) - lam(ts[i - 1]))
            d_x, d_e = 1.0 / al(t), -sg(t) / al(t)
            rows.append([A + E * (1.0 + k) * d_x, E * (1.0 + k) * d_e, -E * k, 0.0, d_x, d_e])
        return torch.tensor(rows, dtype=torch.float64)

    def sampler_plan(self, eta=0.0, start=0, masked=False, dual=False):
        """``eta`` is ignored, as the reference's ``prepare_extra_step_kwargs`` drops it for a scheduler whose ``step`` has none.
        ``start`` / ``masked`` / ``dual``: see ``sampler_rows`` and ``DDIMScheduler.sampler_plan`` (the table is six-column already; ``dual``
        only marks ``key``)."""
        start, masked = self._check_start(start), bool(masked)
        key = ("DPMSolverMultistepScheduler", self.solver_order, self.timestep_spacing, self.lower_order_final, self.num_train_timesteps,
               self.steps_offset, self._betas)
        if start or masked:
            key += (start, masked)
        if dual:
            key += ("dual",)
        return SamplerPlan(self.sampler_rows(start=start).float(), False, self.solver_order > 1, False, key,
                           self.keep_table(start) if masked else None, start)

    def inversion_plan(self, eta=0.0, start=0, dual=False):
        """not available: the multistep solver is deterministic -- it has no per-step noise to invert into (``DDIMScheduler.inversion_plan``)"""
        raise ValueError("scheduler: DDPM inversion needs DDIMScheduler with eta > 0; DPMSolverMultistepScheduler has no per-step noise to "
                         "invert into")
