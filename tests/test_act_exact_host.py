"""The operands of the saturated-activation tests (tests/act_exact_cases.py) checked on the CPU, on the fp64 reference alone.

Tier Z: every operand is representable in bf16, f16 and fp32; every gate lies in the activation's three classes; every value, hidden activation,
stage of the second GEMM and output is an integer of at most 256 (the backward's dgate at g = 0: a half-integer) and equals the fp64 activation
after rounding to each storage type; each hidden unit meets all three classes across its tokens (from 8 tokens up: the sign schedule of the first
eight; fewer: the case as a whole does); no 16-unit chunk of any token has a constant hidden activation; at least a third of the outputs are non-zero; every recipe and anchor
group is checked on all of its sign combinations.
Tier G: gates on the half-integer grid within 5.5, integer values within 8; the derivation of C_E is evaluated (its t term on a fine grid), an fp32
evaluation of gelu_erf_2's operation order with exactly rounded rcp and exp2 stays inside the bound (it reaches 0.23 of it in fp32, printed with
-s), and the bound separates the erf form from the tanh form in f16 and fp32.  tests/test_gpu_exact_activation.py runs the same cases on the GPU."""
import math

import pytest
import torch

import act_exact_cases as AC
from util import rne, ulp_of

_PARAMS = [(c.name, t) for c in AC.CASES for t in c.tiers]
_IDS = [f"{n}-{t}" for n, t in _PARAMS]
DTYPES = (torch.bfloat16, torch.float16, torch.float32)


def _is_int(t, unit=1.0):
    return t.dtype == torch.float64 and torch.equal(t / unit, (t / unit).round())


def _representable(t, dtypes=DTYPES):
    return all(torch.equal(t.to(d).float(), t) for d in dtypes)


@pytest.mark.parametrize("kind,bias", list(AC.RECIPES))
def test_every_recipe_and_anchor_group_stays_in_the_classes(kind, bias):
    act = "silu" if kind == "silu" else "geglu"
    for b, G in AC.RECIPES[(kind, bias)]:
        assert bias or b == 0
        cls = AC.class_of(AC.recipe_values(b, G), act)
        assert set(cls.tolist()) == {-1, 0, 1}, (kind, b, G, AC.recipe_values(b, G).tolist())
        assert bool((cls == 1).any())
    (b, G), sigmas = AC.ANCHOR[(kind, bias)]
    cls = torch.stack([AC.class_of(AC.recipe_values(b, G, s), act) for s in sigmas])  # [units, combinations]
    assert int((cls == 9).sum()) == 0
    assert bool((cls == 1).any(0).all()) and bool((cls != 1).any(0).all()), "a token could find the anchor units all positive or none positive"


@pytest.mark.parametrize("name,tier", _PARAMS, ids=_IDS)
def test_conditions_of_the_tier_hold_on_the_reference(name, tier):
    c, bt = AC.BY_NAME[name], AC.build(name, tier)
    for mode in c.modes:
        AC.route(c, mode)
    w, act = bt["w"], bt["act"]
    dts = tuple(dict.fromkeys(AC.MODES[m] for m in c.modes))
    for t in [w.x, w.w1, w.b1, bt.get("w2"), bt.get("b2"), bt.get("proj"), bt.get("dh"), bt.get("wp")] + list(w.ln[:2] if w.ln else []):
        if t is not None:
            assert t.dtype == torch.float32 and _representable(t, dts), "an operand is not representable in every storage type of the case"
            assert _representable(0.5 * t, dts)  # (the bf16 packers halve the value rows)
    g, v = bt["gates"], w.v
    if tier == "G":
        assert _is_int(g, 0.5) and float(g.abs().max()) <= 5.5 and (v is None or (_is_int(v) and float(v.abs().max()) <= 8))
        assert len(torch.unique(g)) >= 12, "the case sees too little of the grid"
        for mode in c.modes:
            ref, bound = AC.expected(name, tier, mode)
            assert bound.shape == ref.shape and bool((bound > 0).all()) and bool(torch.isfinite(bound).all())
        if w.w1 is not None and act in AC.GATED and w.ln is None:
            H = w.w1.shape[0] // 2
            assert bool((w.w1[:H] % 2 == 1).any()), "no odd value weight: the bf16 packers' halves would not be real"
        return
    # ---- tier Z
    cls = AC.class_of(g, act)
    assert int((cls == 9).sum()) == 0, f"{int((cls == 9).sum())} gates outside the three classes"
    for t in bt["inter"] + ([bt["hidden"]] if bt["hidden"] is not None else []):
        assert _is_int(t) and float(t.abs().max()) <= 256, "not an integer of at most 256"
    ref = bt["ref"]
    assert _is_int(ref, 0.5 if c.op == "geglu_bwd" else 1.0) and float(ref.abs().max()) <= 256
    if v is not None:
        assert float(v.abs().max()) <= 8
        if w.w1 is not None:
            assert bool((v % 2 == 1).all()), "a value pre-activation is even (zero is possible)"
            H = w.w1.shape[0] // 2
            if w.ln is None:
                assert bool((w.w1[:H] % 2 == 1).any()) and (w.b1 is None or bool((w.b1[:H] % 2 == 1).all()))
    # the fp64 activation agrees with the exact value after rounding to every storage type
    if c.op != "geglu_bwd":
        h64, hx = AC.hidden64(w, act), AC.hidden_exact(w, act)
        for d in DTYPES:
            assert torch.equal(h64.float().to(d).double() + 0.0, hx + 0.0), f"rne(act64) differs from the saturated value in {d}"
    else:
        dh = bt["dh"].double()
        full = torch.cat([dh * AC.gelu64(g), dh * v * AC.dgelu64(g)], 1)
        for d in DTYPES:
            assert torch.equal(full.float().to(d).double() + 0.0, ref + 0.0)
    # the three classes: per hidden unit across the tokens (the first eight tokens follow the sign schedule) -- so the token, not the unit, decides the
    # sign of a gate; below 8 tokens in the case as a whole
    M, matrix = g.shape[0], c.op not in ("geglu", "geglu_bwd")
    if matrix and M >= 8:
        first = cls if c.op == "conv1d" else cls[:8]  # (a convolution's taps read the schedule shifted and through the zero padding: all of its tokens)
        for k in (-1, 0, 1):
            assert bool((first == k).any(0).all()), f"{int((~(first == k).any(0)).sum())} hidden units do not meet class {k} in the first eight tokens"
    else:
        assert set(cls.unique().tolist()) == {-1, 0, 1} or (not matrix and g.numel() < 64)
    # no constant 16-unit chunk of the hidden activation
    h = bt["hidden"] if bt["hidden"] is not None else (ref if c.op not in ("geglu_bwd",) else None)
    if h is not None and w.w1 is not None and h.shape[1] % 16 == 0:
        ch = h.reshape(h.shape[0], -1, 16)
        assert bool((ch.amax(2) != ch.amin(2)).all()), "a 16-unit chunk of a token is constant"
    assert float((ref != 0).double().mean()) >= 1.0 / 3.0, f"only {float((ref != 0).double().mean()):.1%} of the outputs are non-zero"


def test_the_count_of_c_e():
    """the t term of C_E on a fine grid, and the sum of the derivation"""
    x = torch.linspace(0.0, 6.0, 60001, dtype=torch.float64) / math.sqrt(2.0)  # erf's argument for |g| <= 6
    t = 1.0 / (1.0 + AC.AS_P * x)
    sens = sum((k + 1) * a * t ** (k + 1) for k, a in enumerate(AC.AS_A)).abs() * torch.exp(-x * x)
    t_term = float((sens * (3.0 * (1.0 - t) + 3.0)).max())
    print(f"  t term {t_term:.2f} u; coefficients {sum(abs(a) for a in AC.AS_A):.2f} u")
    assert t_term <= 12.0 and sum(abs(a) for a in AC.AS_A) <= 4.5
    # Horner intermediates
    p1 = AC.AS_A[4] * t + AC.AS_A[3]
    p2 = p1 * t + AC.AS_A[2]
    p3 = p2 * t + AC.AS_A[1]
    p4 = p3 * t + AC.AS_A[0]
    horner = sum(float(p.abs().max()) for p in (p1, p2, p3, p4))
    assert horner <= 4.7
    q = x * x / math.log(2.0)
    e_term = float((5.0 * q * torch.exp2(-q) * math.log(2.0)).max()) + 2.0
    assert e_term <= 4.0
    assert t_term + horner + 4.5 + 1.0 + e_term + 1.0 <= AC.C_E <= 12.0 + 4.6 + 4.5 + 1.0 + 4.0 + 1.0 + 1.0 and AC.C_E_F == AC.C_E + 1.0
    # the A&S form itself: 1.5e-7
    as_erf = 1.0 - sum(a * t ** (k + 1) for k, a in enumerate(AC.AS_A)) * torch.exp(-x * x)
    assert float((as_erf - torch.erf(x)).abs().max()) <= 1.5e-7


def test_fp32_evaluation_of_gelu_erf_2_stays_inside_the_bound():
    """the kernel's operation order in fp32 on the grid (and on a fine grid), times every integer value, against the tier-G bound in fp32 storage"""
    worst = 0.0
    for g in (torch.arange(-11, 12, dtype=torch.float64) / 2.0, (torch.arange(-5632, 5633, dtype=torch.float64) / 1024.0)):
        ge = AC.emulate_gelu_erf_2(g)
        for vi in range(-8, 9):
            v = torch.full_like(g, float(vi))
            out = (v * ge).float().double()  # the fp32 product
            bound, ref = AC.gelu_bound(v, g, torch.float32)
            ratio = float(((out - ref).abs() / bound).max())
            worst = max(worst, ratio)
    print(f"  fp32 evaluation of gelu_erf_2's order: worst |error| / bound {worst:.3f}")
    assert worst <= 1.0
    # saturation: the same order returns g and 0 exactly from |g| = 6
    g = torch.tensor([6.0, 7.0, 8.0, 16.0, 32.0, 40.0, -6.0, -8.0, -16.0, -32.0, -40.0, 0.0], dtype=torch.float64)
    assert torch.equal(AC.emulate_gelu_erf_2(g) + 0.0, torch.where(g > 0, g, torch.zeros_like(g)))


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
def test_the_bound_separates_erf_gelu_from_tanh_gelu(dtype):
    g = (torch.arange(-11, 12, dtype=torch.float64) / 2.0).repeat(17)
    v = torch.arange(-8, 9, dtype=torch.float64).repeat_interleave(23)
    bound, ref = AC.gelu_bound(v, g, dtype)
    other = rne(v * AC.gelu_tanh64(g), dtype).double()
    n = int(((other - ref).abs() > bound).sum())
    print(f"  {n} of {g.numel()} (v, g) pairs of the tanh form leave the erf form's bound in {dtype}")
    assert n >= 20
    # and the erf form rounded to the type stays inside it
    assert bool(((rne(ref, dtype).double() - ref).abs() <= bound).all())


def test_backward_bound_holds_for_an_fp32_evaluation():
    """geglu_bwd_kernel's formulas in fp32 torch (erf, exp: within an ulp) against the dgate bound"""
    g = (torch.arange(-11, 12, dtype=torch.float64) / 2.0)
    gf = g.float()
    cdf = 0.5 * (1.0 + torch.erf(gf * 0.70710678118654752440))
    pdf = 0.3989422804014327 * torch.exp(-0.5 * gf * gf)
    for dhv in (1.0, -7.0, 64.0):
        out = (torch.tensor(dhv) * (cdf + gf * pdf)).double()
        bound, ref = AC.dgate_bound(torch.full_like(g, dhv), g, torch.float32, erff=True)
        assert bool(((out - ref).abs() <= bound).all())
