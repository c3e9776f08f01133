"""CPU: guidance rescale and adaptive projected guidance as host arithmetic -- the declared entry point, ``shape_table``, the pipeline's new
keywords and their checks, and the properties of the float64 restatement (tests/shaped_guidance_oracle.py).  No GPU compute.
PARITY UNPINNED (see shaped_guidance_oracle)."""
import inspect
import os
import re

import pytest
import torch

import ap_adapter_amd as A
from ap_adapter_amd import _lib as L
from ap_adapter_amd.scheduler import shape_table

import shaped_guidance_oracle as SG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OFF = (0.0, 1.0, 0.0, 0.0)


def R(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def _branches(B, n, branches, seed=0):
    """correlated branches, e_0 = c + 0.3 noise (and e_A between them), so that no denominator is near zero"""
    c = R(B, n, seed=seed) * 0.5 + 0.1
    if branches == 2:
        return torch.cat([c + 0.3 * R(B, n, seed=seed + 1), c])
    e_a = c + 0.2 * R(B, n, seed=seed + 2)
    return torch.cat([e_a + 0.3 * R(B, n, seed=seed + 1), e_a, c])


def test_header_declares_the_entry_point_and_the_abi_line_stays():
    h = open(os.path.join(ROOT, "include", "apadapter_hip.h")).read()
    assert re.search(r"^#define APAD_ABI_VERSION 12$", h, re.M)
    m = re.search(r"^int apad_cfg_shaped_step\(([^;]*)\);", h, re.M)
    assert m, "apad_cfg_shaped_step is not declared"
    args = [a.strip() for a in m.group(1).replace("\n", " ").split(",")]
    res, argtypes = L.SYMBOLS["apad_cfg_shaped_step"]
    assert len(args) == len(argtypes) == 25
    for name in ("const float* shape", "float* momentum", "float* stats", "int32_t branches", "float guidance_scale"):
        assert name in args, name
    # pointers where the header has pointers, scalars where it has scalars
    for a, t in zip(args, argtypes):
        assert ("*" in a) == (t is L._vp), (a, t)
    src = open(os.path.join(ROOT, "ap-adapter_amd", "csrc", "elementwise.hip")).read()
    assert "cfg_shaped_step_kernel" in src and 'extern "C" int apad_cfg_shaped_step(' in src


def test_shape_table_values_and_slicing():
    t = shape_table(0.7, 0.25, 2.5, -0.5, 4)
    assert t.dtype == torch.float32 and t.shape == (4, 4) and t.is_contiguous()
    assert torch.equal(t, torch.tensor([[0.7, 0.25, 2.5, -0.5]] * 4))
    assert torch.equal(shape_table(*OFF, 3), torch.tensor([list(OFF)] * 3))
    phi, eta = [0.0, 0.25, 0.5, 1.0], (1.0, 0.5, 0.0, -0.5)
    t = shape_table(phi, eta, torch.tensor([0.0, 1.0, 2.0, 3.0]), [0.0, 0.0, -0.75, 0.75], 4, start=1)
    assert t.shape == (3, 4)
    assert torch.equal(t, torch.tensor([[0.25, 0.5, 1.0, 0.0], [0.5, 0.0, 2.0, -0.75], [1.0, -0.5, 3.0, 0.75]]))
    # rows before ``start`` are neither used nor checked
    nan = float("nan")
    assert torch.equal(shape_table([nan, 0.5], [nan, 1.0], [-1.0, 0.0], [7.0, 0.0], 2, start=1), torch.tensor([[0.5, 1.0, 0.0, 0.0]]))


@pytest.mark.parametrize("kw,match", [
    (dict(guidance_rescale=-0.1), "^guidance_rescale"), (dict(guidance_rescale=1.5), "^guidance_rescale"),
    (dict(guidance_rescale=float("nan")), "^guidance_rescale"), (dict(guidance_rescale=[0.5, 0.5]), "^guidance_rescale holds 2"),
    (dict(guidance_rescale="x"), "^guidance_rescale"),
    (dict(apg_eta=float("inf")), "^apg_eta"), (dict(apg_eta=[1.0] * 5), "^apg_eta holds 5"), (dict(apg_eta=None), "^apg_eta"),
    (dict(apg_norm_threshold=-1.0), "^apg_norm_threshold"), (dict(apg_norm_threshold=float("nan")), "^apg_norm_threshold"),
    (dict(apg_norm_threshold=[1.0, 2.0, 3.0, -4.0]), "^apg_norm_threshold"),
    (dict(apg_momentum=1.0), "^apg_momentum"), (dict(apg_momentum=-1.0), "^apg_momentum"), (dict(apg_momentum=float("nan")), "^apg_momentum"),
    (dict(apg_momentum=[0.0, 0.0, 0.0]), "^apg_momentum holds 3"),
])
def test_shape_table_value_errors_name_the_argument(kw, match):
    args = dict(guidance_rescale=0.5, apg_eta=0.5, apg_norm_threshold=1.0, apg_momentum=-0.5)
    args.update(kw)
    with pytest.raises(ValueError, match=match):
        shape_table(num_inference_steps=4, **args)


def test_shape_table_start_is_checked():
    for start in (-1, 4):
        with pytest.raises(ValueError, match="^start"):
            shape_table(*OFF, 4, start=start)


def test_pipeline_keywords_defaults_and_validation():
    P = A.AudioLDM2Pipeline
    want = dict(guidance_rescale=0.0, apg_eta=None, apg_norm_threshold=0.0, apg_momentum=0.0)
    for fn in (P.__call__, P.denoise):
        params = inspect.signature(fn).parameters
        for name, default in want.items():
            assert name in params and params[name].default == default, (fn.__name__, name)
    assert not set(want) & set(inspect.signature(P.invert).parameters)  # the inversion pass is not shaped
    chk = P.check_shaping_arguments
    assert chk(0.0, None, 0.0, 0.0, 4) is None and chk(0, None, 0, 0, 4) is None  # the defaults: the stage is off
    assert torch.equal(chk(0.7, None, 0.0, 0.0, 3), torch.tensor([[0.7, 1.0, 0.0, 0.0]] * 3))  # a rescale alone: eta = 1
    assert torch.equal(chk(0.0, 0.0, 2.5, -0.5, 4, 2), torch.tensor([[0.0, 0.0, 2.5, -0.5]] * 2))
    assert torch.equal(chk(0.0, 1.0, 0.0, 0.0, 2), torch.tensor([list(OFF)] * 2))  # apg_eta given: on, even when every value is neutral
    assert chk([0.0, 0.0], None, 0.0, 0.0, 2) is not None  # a schedule is on, whatever it holds
    with pytest.raises(ValueError, match="^apg_norm_threshold.*needs apg_eta"):
        chk(0.0, None, 2.5, 0.0, 4)
    with pytest.raises(ValueError, match="^apg_momentum.*needs apg_eta"):
        chk(0.5, None, 0.0, -0.5, 4)
    with pytest.raises(ValueError, match="^apg_momentum.*needs apg_eta"):
        chk(0.0, None, 0.0, [0.0] * 4, 4)
    with pytest.raises(ValueError, match="^guidance_rescale"):
        chk(1.5, None, 0.0, 0.0, 4)
    with pytest.raises(ValueError, match="^apg_momentum"):
        chk(0.0, 0.5, 0.0, 1.0, 4)
    for doc in (P.__call__.__doc__, P.denoise.__doc__):
        assert "guidance_rescale" in doc and "apg_eta" in doc and "edit pass only" in doc.lower()


# ---- the restatement's own properties ----
@pytest.mark.parametrize("branches", [2, 3])
def test_all_off_row_and_eta_one_are_plain_guidance(branches):
    B, n = 3, 257
    eps = _branches(B, n, branches)
    w = (7.5,) if branches == 2 else (2.5, 7.5)
    plain = SG.plain_cfg(eps, branches, w)
    out = SG.shaped_guidance(eps, branches, w, OFF)
    assert torch.equal(out["g"], plain)
    assert torch.equal(out["stats"], torch.tensor([[1.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0]] * B, dtype=torch.float64))
    assert out["momentum"] is None
    # plain two-branch guidance written the usual way
    if branches == 2:
        e0, c = eps[:B], eps[B:]
        assert float((plain - (e0 + 7.5 * (c - e0))).abs().max()) == 0.0
    else:
        e0, ea, eat = eps[:B], eps[B:2 * B], eps[2 * B:]
        assert float((plain - (e0 + 2.5 * (ea - e0) + 7.5 * (eat - ea))).abs().max()) <= 1e-15 * float(plain.abs().max())


@pytest.mark.parametrize("branches", [2, 3])
def test_full_rescale_matches_the_conditioned_std(branches):
    B, n = 3, 1001
    eps = _branches(B, n, branches, seed=5)
    w = (7.5,) if branches == 2 else (2.5, 7.5)
    out = SG.shaped_guidance(eps, branches, w, (1.0, 1.0, 0.0, 0.0))
    c = eps[-B:]
    assert float((out["g"].std(-1) - c.std(-1)).abs().max()) <= 1e-12
    assert torch.allclose(out["std_c"], c.std(-1), rtol=1e-13) and torch.allclose(out["std_g"], SG.plain_cfg(eps, branches, w).std(-1), rtol=1e-13)
    assert bool((out["f"] < 1.0).all())  # guidance at these scales inflates the energy: the rescale pulls it back
    half = SG.shaped_guidance(eps, branches, w, (0.5, 1.0, 0.0, 0.0))
    assert torch.allclose(half["f"], 0.5 * out["f"] + 0.5, rtol=1e-13)
    one = SG.shaped_guidance(eps[:, :1], branches, w, (1.0, 1.0, 0.0, 0.0))  # n == 1: no standard deviation, f = 1
    assert torch.equal(one["f"], torch.ones(B, dtype=torch.float64)) and torch.equal(one["g"], SG.plain_cfg(eps[:, :1], branches, w))


@pytest.mark.parametrize("branches", [2, 3])
def test_eta_zero_leaves_the_orthogonal_part(branches):
    B, n = 3, 520
    eps = _branches(B, n, branches, seed=7)
    w = (7.5,) if branches == 2 else (2.5, 7.5)
    out = SG.shaped_guidance(eps, branches, w, (0.0, 0.0, 0.0, 0.0))
    c = out["c"]
    for u, d in zip(out["u"], out["d"]):
        cos = (u * c).sum(-1) / (u.norm(dim=-1) * c.norm(dim=-1))
        assert float(cos.abs().max()) <= 1e-13
        par = ((d * c).sum(-1) / (c * c).sum(-1))[:, None] * c
        assert float((u + par - d).abs().max()) <= 1e-14  # orthogonal + parallel = d
    # eta interpolates: u(eta) = orthogonal + eta * parallel
    mid = SG.shaped_guidance(eps, branches, w, (0.0, 0.25, 0.0, 0.0))
    for u0, um, d in zip(out["u"], mid["u"], out["d"]):
        assert float((um - (u0 + 0.25 * (d - u0))).abs().max()) <= 1e-14
    z = SG.shaped_guidance(torch.zeros_like(eps), branches, w, (0.0, 0.0, 2.0, 0.0))  # zero denominators: p = 0, t = 1
    assert torch.equal(z["g"], torch.zeros(B, n, dtype=torch.float64)) and torch.equal(z["stats"][:, :4], torch.tensor([[1.0, 0.0, 1.0, 0.0]] * B).double())


@pytest.mark.parametrize("branches", [2, 3])
def test_norm_threshold_bounds_the_difference(branches):
    B, n = 3, 520
    eps = _branches(B, n, branches, seed=9)
    w = (7.5,) if branches == 2 else (2.5, 7.5)
    norms = [d.norm(dim=-1) for d in SG.differences(eps, branches)[2]]
    r = float(min(float(x.min()) for x in norms)) * 0.5
    out = SG.shaped_guidance(eps, branches, w, (0.0, 1.0, r, 0.0))
    for t, d in zip(out["t"], out["d"]):
        assert bool((t < 1.0).all()) and float(((t[:, None] * d).norm(dim=-1) - r).abs().max()) <= 1e-12 * r
    big = SG.shaped_guidance(eps, branches, w, (0.0, 1.0, 1e6, 0.0))  # a threshold above every norm does nothing
    assert torch.equal(big["g"], SG.plain_cfg(eps, branches, w)) and all(bool((t == 1.0).all()) for t in big["t"])


@pytest.mark.parametrize("branches", [2, 3])
def test_momentum_recurrence_over_three_steps(branches):
    B, n, K = 2, 64, branches - 1
    w = (7.5,) if branches == 2 else (2.5, 7.5)
    betas = (-0.5, 0.25, -0.75)
    m = torch.zeros(K, B, n, dtype=torch.float64)
    ds = []
    for s, beta in enumerate(betas):
        eps = _branches(B, n, branches, seed=20 + 3 * s)
        out = SG.shaped_guidance(eps, branches, w, (0.0, 1.0, 0.0, beta), m)
        ds.append(out["d_raw"])
        m = out["momentum"]
        g = eps[:B].double()
        for k in range(K):
            g = g + w[k] * m[k]
        assert float((out["g"] - g).abs().max()) <= 1e-14  # the averaged difference is what guides
    for k in range(K):
        want = ds[2][k] + betas[2] * (ds[1][k] + betas[1] * ds[0][k])  # m_0 = d_0 (zero state), then d + beta m
        assert float((m[k] - want).abs().max()) <= 1e-14
    # beta == 0 passes the state through untouched and does not use it
    eps = _branches(B, n, branches, seed=40)
    nan = torch.full_like(m, float("nan"))
    out = SG.shaped_guidance(eps, branches, w, OFF, nan)
    assert out["momentum"] is nan and torch.equal(out["g"], SG.plain_cfg(eps, branches, w))
