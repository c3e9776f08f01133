"""Restatement of the three-branch guidance combine for the tests.  TEST INFRASTRUCTURE ONLY.

**PARITY UNPINNED**: the reference has no such path (its loop forms e_u + g (e_c - e_u) only).  The formula is InstructPix2Pix's
two-scale guidance (Brooks et al. 2023, section 3.2.1) with the image condition replaced by the audio prompt:

  eps = e_0 + s_A (e_A - e_0) + s_T (e_AT - e_A)

  e_0  : negative text, zero-mel audio tokens        e_A : negative text, prompt audio tokens        e_AT : positive text, prompt audio tokens

``cfg3_combine_rounded`` is the twin of ``sampler_oracle.cfg_combine_rounded``: the kernel's fp32 arithmetic spelled out on the host.
What follows the combine -- the sampler step, the edit blend -- is ``sampler_oracle.dpm_step`` / ``ddim_step`` and ``edit_oracle``,
unchanged.
"""
import torch

import sampler_oracle as SO  # noqa: F401  (re-exported: the steps that follow the combine)
import edit_oracle as EO  # noqa: F401


def _f32(s):
    return float(torch.tensor(float(s), dtype=torch.float32))


def cfg3_combine_rounded(eps3, s_A, s_T, dtype):
    """the guided noise in the model dtype (eps3 [3B, ...] holds storage-rounded values, branches 0 / A / AT along the batch): each
    difference rounded to fp32, two fused multiply-adds -- the product of two fp32 values is exact in float64, and each fma is
    (float32(s) * d.double() + base.double()).float() -- and one rounding to ``dtype``.  Returned as float64."""
    e0, ea, eat = eps3.float().chunk(3)
    d_a = ea - e0
    d_t = eat - ea
    inner = (_f32(s_A) * d_a.double() + e0.double()).float()
    e32 = (_f32(s_T) * d_t.double() + inner.double()).float()
    return e32.to(dtype).double()


def cfg3_combine_exact(eps3, s_A, s_T):
    """the same formula in float64, nothing rounded"""
    e0, ea, eat = eps3.double().chunk(3)
    return e0 + float(s_A) * (ea - e0) + float(s_T) * (eat - ea)


def ramp(a, b, steps):
    """``steps`` values from a to b inclusive, as Python floats: a per-step guidance schedule"""
    return [a + (b - a) * i / (steps - 1) for i in range(steps)]
