"""The operands of the exact-statistics normalisation tests (tests/norm_exact_cases.py) checked on the CPU, on the fp64 reference alone: every set's
sums are exact integers below 2^24, every set is centred (|mean| <= sigma), tier R's expected value is the dyadic +-gamma + beta with a tie margin of
2^-6 ulp, and a plain fp32 emulation of BOTH variance formulas (E[x^2] - mean^2 and the shifted form), each summed in two orders -- torch's blocked
sum, and threads that add strided elements in turn followed by a butterfly (64 lanes for a row: LayerNorm, RMS; the 256 threads of the fp32
GroupNorm for a slab: the only GroupNorm kernel with the shifted form) -- stays inside the tier-K bound 0.5 ulp_fp32 + 16 * 2^-24 * A for every case.
Worst |error| / bound of that emulation over all cases, as test_fp32_emulation_of_both_variance_formulas_stays_inside_the_bound prints it (-s):
0.21 for E[x^2] - mean^2 (exact sums: only the derived roundings remain), 0.91 for the shifted form (its sum of squared deviations is not exact; the
worst is the largest slab, 40000 elements, 157 additions per thread; 64 lanes on such a slab -- 625 additions per lane, no kernel's shape -- reach
2.6, which is why the emulation follows the kernels' shapes); the small-variance sets: 0.15 and 0.24.  tests/test_gpu_exact_norm.py runs the same
cases on the GPU."""
import pytest
import torch

import norm_exact_cases as NC
from util import ulp_of

_PARAMS = [(c.name, t) for c in NC.CASES for t in c.tiers]
_IDS = [f"{n}-{t}" for n, t in _PARAMS]
WORST = {}


def _unit(c):
    return 2.0 ** -6 if c.args.get("kind") == "small" else 1.0


@pytest.mark.parametrize("name,tier", _PARAMS, ids=_IDS)
def test_conditions_of_the_tier_hold_on_the_reference(name, tier):
    c, bt = NC.BY_NAME[name], NC.build(name, tier)
    kind = c.args.get("kind")
    for t in [bt.x, bt.gamma, bt.beta, bt.dy, bt.xa, bt.xb]:
        if t is not None:
            assert t.dtype == torch.float32
            for dt in (torch.bfloat16, torch.float16):
                assert torch.equal(t.to(dt).float(), t), "an operand is not representable in bf16 / f16 / fp32"
    # exact sums: integers (times the unit) whose absolute sums stay below 2^24, so every partial sum in any order is exact in fp32
    s = bt.sets.double() / _unit(c)
    assert torch.equal(s, s.round()), "not integers"
    assert float(s.abs().sum(1).max()) < 2 ** 24 and float((s * s).sum(1).max()) < 2 ** 24
    mean, var = bt.mean, bt.var
    if c.op in ("rms", "l2"):
        assert not bool(mean.any())
    elif kind == "flat":  # both formulas give exactly 0: n k / n = k and n k^2 / n - k^2 = 0 without a rounding
        assert bool((var == 0).all()) and set(mean.tolist()) == {1.0, 2.0}
    else:
        # (tier R reaches |m| = a, and var is an fp64 sum of squares: hence the 1e-12)
        assert bool((mean.abs() <= var.sqrt() * (1 + 1e-12)).all()), f"{name}: a set is off centre: |mean| / sigma up to {float((mean.abs() / var.sqrt()).max()):.2f}"
    if bt.gamma is not None:
        g8 = bt.gamma.double() * 8
        assert torch.equal(g8, g8.round()) and bool((g8 % 2 == 1).all()) and float(bt.gamma.abs().max()) <= 4
        pairs = {(float(a), float(b)) for a, b in zip(bt.gamma, bt.beta if bt.beta is not None else torch.zeros_like(bt.gamma))}
        C = bt.gamma.numel()
        assert len(pairs) == min(C, len(NC._pairs("R" if tier in "RS" else "K"))) or bt.beta is None, "(gamma, beta) repeat inside a window"
    if bt.beta is not None:
        b4 = bt.beta.double() * 4
        assert torch.equal(b4, b4.round()) and float(bt.beta.abs().max()) <= 4
    if tier in "RS":
        n = bt.sets.shape[1]
        hi, lo = bt.sets.max(1).values, bt.sets.min(1).values
        a, m = (hi - lo) / 2, (hi + lo) / 2
        assert bool(((bt.sets == hi[:, None]).sum(1) == n // 2).all()) and bool(((bt.sets == lo[:, None]).sum(1) == n // 2).all())
        assert bool(torch.isin(a, torch.tensor([1.0, 2.0, 4.0])).all()) and bool((m.abs() <= a).all()) and torch.equal(m, m.round())
        assert torch.equal(mean, m.double()) and torch.allclose(var, (a * a).double(), rtol=1e-13, atol=0)  # (var: an fp64 sum of squares)
        if c.op in ("ln", "ln_bwd", "rms", "l2", "rp_ln", "fold_ln"):
            ma = torch.stack([m, a], 1)
            assert bool((ma[1:] != ma[:-1]).any(1).all()), "neighbouring rows share (m, a)"
        elif c.op in ("gn", "gn_bwd"):
            ma = torch.stack([m, a], 1).reshape(c.args["B"], c.args["G"], 2)
            assert bool((ma[:, 1:] != ma[:, :-1]).any(-1).all()) and bool((ma[1:] != ma[:-1]).any(-1).all()), "neighbouring groups / samples share (m, a)"
        else:
            ma = torch.stack([m, a], 1).reshape(c.args["B"], c.args["G"], 2)
            assert bool((ma[:, 1:] != ma[:, :-1]).any(-1).all()) and bool((ma[1] != ma[0]).any(-1).all())
    if c.op == "fold_ln":
        assert set(bt.w.unique().tolist()) == {-1.0, 0.0, 1.0} and torch.equal(bt.wb, bt.wb.round())
        acc8 = (bt.x.double() @ (bt.w.double() * bt.gamma.double()).t()) * 8  # the accumulator and the column sums: multiples of 1/8 below 2^24 / 8
        assert torch.equal(acc8, acc8.round()) and float((bt.x.double().abs() @ (bt.w.double() * bt.gamma.double()).abs().t()).max()) * 8 < 2 ** 24
    if c.op == "rp_ln":  # the normalised operand is the dyadic value with tier R's margin; the product sums are multiples of 1/8 below 2^24 / 8
        y8 = bt.y * 8
        assert torch.equal(y8, y8.round()) and float((bt.absref * 8).max()) < 2 ** 24 and set(bt.w.unique().tolist()) == {-1.0, 0.0, 1.0}
        assert torch.equal(bt.wb, bt.wb.round()) and float(bt.wb.abs().max()) <= 8
    if bt.y is not None and tier == "R":
        y, ref = bt.y if c.op != "rp_ln" else bt.xn, NC.norm64(bt.x, bt.groups, bt.gamma, bt.beta, bt.eps, rms=c.op == "rms", l2=c.op == "l2")[0]
        assert bool((y != 0).all())
        for dt in (torch.bfloat16, torch.float16):
            assert torch.equal(y.float().to(dt).double(), y), "the dyadic value is not representable"
            assert torch.equal(ref.float().to(dt).double(), y), "the reference does not round to the dyadic value"
            assert bool(((ref - y).abs() <= 2.0 ** -6 * ulp_of(y, dt)).all()), f"{name}: the reference lies farther than 2^-6 ulp from the dyadic value ({dt})"
    if tier == "K" and kind is None:
        assert int((bt.x.abs() == NC.SPIKE).sum()) >= 2 and float(bt.x.abs().max()) == NC.SPIKE
        body = bt.x[bt.x.abs() != NC.SPIKE]
        assert float(body.abs().max()) <= 3
    if bt.dy is not None:
        assert torch.equal(bt.dy, bt.dy.round()) and float(bt.dy.abs().max()) == NC.SPIKE


def _sum_lanes(t, lanes=64):
    """[S, n] fp32 -> [S]: ``lanes`` threads add the elements lane, lane + lanes, ... in turn, then a butterfly: a wave per row (LayerNorm, RMS) or
    a 256-thread workgroup per slab (the fp32 GroupNorm, the only GroupNorm kernel with the shifted form)"""
    S, n = t.shape
    pad = (-n) % lanes
    if pad:
        t = torch.cat([t, torch.zeros(S, pad)], 1)
    t = t.reshape(S, -1, lanes)
    acc = torch.zeros(S, lanes)
    for i in range(t.shape[1]):
        acc = acc + t[:, i]
    w = lanes // 2
    while w:
        acc = acc[:, :w] + acc[:, w:2 * w]
        w //= 2
    return acc[:, 0]


def _emulate(bt, c, formula, summed):
    """the normalisation in plain fp32 torch: ((x - mean) * rstd) * gamma + beta"""
    s = bt.sets
    n = torch.tensor(float(s.shape[1]))
    if c.op in ("rms", "l2"):
        q = summed(s * s)
        r = 1.0 / torch.sqrt(q).clamp_min(bt.eps) if c.op == "l2" else 1.0 / torch.sqrt(q / n + bt.eps)
        out = NC.from_sets(s * r[:, None], bt.x.shape, None)
        return out * bt.gamma if bt.gamma is not None else out
    mean = summed(s) / n
    if formula == "raw":
        var = (summed(s * s) / n - mean * mean).clamp_min(0.0)
    else:
        d = s - mean[:, None]
        var = summed(d * d) / n
    rstd = 1.0 / torch.sqrt(var + bt.eps)
    xh = NC.from_sets((s - mean[:, None]) * rstd[:, None], bt.x.shape, bt.groups)
    return xh * bt.gamma + bt.beta


_FWD = [(n, t) for n, t in _PARAMS if t in "RK" and NC.BY_NAME[n].op not in ("ln_bwd", "gn_bwd", "rp_ln", "fold_ln")]


@pytest.mark.parametrize("name,tier", _FWD, ids=[f"{n}-{t}" for n, t in _FWD])
def test_fp32_emulation_of_both_variance_formulas_stays_inside_the_bound(name, tier):
    c, bt = NC.BY_NAME[name], NC.build(name, tier)
    assert all(t.dtype == torch.float32 for t in (bt.sets,))
    bound = 0.5 * ulp_of(bt.ref, torch.float32) + NC.COEFF * NC.U * bt.absref
    for formula in ("raw", "shifted"):
        for order, summed in (("blocked", lambda t: t.sum(1)), ("lanes", lambda t: _sum_lanes(t, 64 if bt.groups is None else 256))):
            out = _emulate(bt, c, formula, summed)
            assert out.dtype == torch.float32 and bool(torch.isfinite(out).all())
            ratio = float(((out.double() - bt.ref).abs() / bound).max())
            key = (formula, "small" if c.args.get("kind") == "small" else "other")
            WORST[key] = max(WORST.get(key, 0.0), ratio)
            assert ratio <= 1.0, f"{name} [{tier}] {formula} / {order}: error {ratio:.2f} of the bound"
    print(f"  {name} [{tier}]: worst so far {({k: round(v, 3) for k, v in WORST.items()})}")


def test_route_of_every_case_is_the_dispatchers():
    seen = set()
    for c in NC.CASES:
        for d in c.dtypes:
            seen.add(NC.check_route(c, NC.DTYPES[d]))
    assert seen == {"nv1", "nv2", "nv4", "f32", "f32_tail", "full8", "full4", "onepass256", "onepass1024", "twopass_fast", "twopass_generic",
                    "twopass_fast_65", "wave_row", "ln_bwd", "gn_bwd", "rowpanel", "folded"}
    # the thresholds the case names rely on, from gn_onepass_launch's arithmetic
    gn = lambda **a: NC.route_of("gn", a, True)
    assert gn(C=640, G=32, HW=600) == "onepass256" and gn(C=640, G=32, HW=601) == "onepass1024" and gn(C=640, G=32, HW=1025) == "twopass_generic"
    assert gn(C=64, G=8, HW=64) == "full8" and gn(C=64, G=4, HW=64) == "onepass256" and gn(C=1280, G=32, HW=64) == "onepass256"
    assert NC.route_of("gn2", dict(Ca=384, Cb=256, G=32, HW=64), True) == "onepass256"
    assert NC.route_of("gn2", dict(Ca=64, Cb=64, G=16, HW=64), True) == "onepass256"  # cg = 8: two sources never take the full-line form


def test_shifted_form_kernels_add_few_enough_terms_per_thread():
    """the 16 of the bound leaves the shifted form's inexact sum of squares about u sqrt(k) / 2 for k additions per thread (norm_exact_cases.py): the
    cases stay at k <= SHIFTED_ADDS_MAX, and the emulation above sums the GroupNorm slabs with the fp32 kernel's 256 threads"""
    worst = 0
    for c in NC.CASES:
        for d in c.dtypes:
            k = NC.shifted_adds(c, NC.DTYPES[d])
            worst = max(worst, k)
            assert k <= NC.SHIFTED_ADDS_MAX, (f"{c.name} [{d}]: {k} additions per thread in a shifted-form sum of squares: its rounding, about u sqrt(k) / 2 "
                                              f"of A, no longer fits the 16 (norm_exact_cases.py, 'variance, shifted form'); that kernel needs its own coefficient")
    assert worst == 157  # gn_twopass_C1280_HW1000 in fp32: 1000 pixels x 40 channels over 256 threads


def test_two_source_cases_straddle_the_boundary_and_read_each_source_modulo():
    for c in NC.CASES:
        if c.op != "gn2":
            continue
        a = c.args
        cg = (a["Ca"] + a["Cb"]) // a["G"]
        assert a["Ca"] % cg != 0 and a["B"] // min(a["Ba"], a["Bb"]) == 2
        for tier in c.tiers:
            bt = NC.build(c.name, tier)
            assert tuple(bt.xa.shape) == (a["Ba"], a["HW"], a["Ca"]) and tuple(bt.xb.shape) == (a["Bb"], a["HW"], a["Cb"])
            assert not torch.equal(bt.xa[0], bt.xa[1]) and not torch.equal(bt.xb[0], bt.xb[1])
            if tier == "K":
                assert bool((bt.xa[0, :, -1].abs() == NC.SPIKE).any()) and bool((bt.xb[0, :, 0].abs() == NC.SPIKE).any())
    assert {(c.args["Ba"], c.args["Bb"]) for c in NC.CASES if c.op == "gn2"} == {(4, 2), (2, 4)}


# ---- the LayerNorm inside the fused attention kernels (tests/norm_attn_cases.py)
import norm_attn_cases as NA  # noqa: E402


@pytest.mark.parametrize("name", [c.name for c in NA.CASES])
def test_fused_attention_rows_select_one_key_through_the_layernorm(name):
    c, bt = NA.BY_NAME[name], NA.build(name)
    B, N, C = bt.x.shape
    rows = bt.x.reshape(B * N, C)
    for t in (bt.x, bt.gamma, bt.beta, bt.wq, bt.wk, bt.wv, bt.k, bt.v):
        if t is not None:
            for dt in (torch.bfloat16, torch.float16):
                assert torch.equal(t.to(dt).float(), t), "an operand is not representable in bf16 / f16"
    hi, lo = rows.max(1).values, rows.min(1).values
    a, m = (hi - lo) / 2, (hi + lo) / 2
    assert bool(((rows == hi[:, None]).sum(1) == C // 2).all()) and bool(((rows == lo[:, None]).sum(1) == C // 2).all())
    assert bool(torch.isin(a, torch.tensor([1.0, 2.0, 4.0])).all()) and bool((m.abs() <= a).all())
    if B * N > 1:
        ma = torch.stack([m, a], 1)
        assert bool((ma[1:] != ma[:-1]).any(1).all()), "neighbouring rows share (m, a)"
    # the fp64 scores (base-2 exponent): the selected key within 0.1 of 0 (8 dims of w gamma eps / (2 a^2) each), every other key at most -150
    s = bt.scores  # [B, H, N, L]
    ssel = s.gather(-1, bt.sel[..., None])
    assert float(ssel.abs().max()) < 0.1, float(ssel.abs().max())
    if s.shape[-1] > 1:
        assert float(s.scatter(-1, bt.sel[..., None], -1.0e9).max()) <= -150.0
    assert len(set(bt.sel.reshape(-1).tolist())) == min(c.L, len(set(bt.sel.reshape(-1).tolist()))) and (0 in bt.sel and c.L - 1 in bt.sel or B * N * 8 < 3)
    # the fold vectors the test is about are large: column sums w gamma, W . beta = w beta
    assert float((bt.wq * bt.gamma).sum(1).abs().max()) >= 512 and float((bt.wq @ bt.beta).abs().max()) >= 512
    for dt in (torch.bfloat16, torch.float16):
        if c.route in NA.SELF:  # V = the normalised row: representable, and the fp64 LayerNorm within 2^-6 ulp of it wherever it is not 0
            assert torch.equal(bt.xn.float().to(dt).double(), bt.xn)
            x64 = rows.double()
            ln = (x64 - x64.mean(1, keepdim=True)) / (x64.var(1, unbiased=False, keepdim=True) + c.eps).sqrt() * bt.gamma.double() + bt.beta.double()
            nz = bt.xn != 0
            assert bool(((ln - bt.xn).abs()[nz] <= 2.0 ** -6 * ulp_of(bt.xn, dt)[nz]).all())
            assert float((ln - bt.xn).abs()[~nz].max()) < 2.0 ** -16  # gamma = beta channels: gamma eps / (2 a^2), where V is 0
        if c.route in ("hs_cross",) + NA.SELF:
            assert torch.equal(bt.ref.float().to(dt).double(), bt.ref)
