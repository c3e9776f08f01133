"""The operands of the exact attention-backward tests (tests/attn_bwd_exact_cases.py) checked on the CPU, on the fp64 reference alone: under these
conditions the gradients of a correct kernel are determined in every bit (or, for the fp32 kernels at a head size whose scale is no power of two,
to the bound the case file counts), and a dropped, doubled or misplaced key or query moves them.  tests/test_gpu_exact_attention_bwd.py runs the
same cases on the GPU.

The non-zero shares are asserted on the cases with N >= 32 and k >= 1: at k = 0 dQ = dK = 0 is the expectation (delta must cancel dP to the last
bit), and with a single query dV is dO's own density of 1/4."""
import math

import pytest
import torch

import attn_bwd_exact_cases as BC
from attn_exact_cases import MASK_BIAS, _code_key
from util import rne

LOG2E_F = float(torch.tensor(1.4426950408889634, dtype=torch.float32))
_PARAMS = BC.params()
_fl32 = BC._fl32


def _scale_log2(d):
    return float(torch.tensor(BC.scale32(d), dtype=torch.float32) * torch.tensor(LOG2E_F, dtype=torch.float32))


def _segments(name):
    o = BC.operands(name)
    return o, list(enumerate(o.segs))


@pytest.mark.parametrize("name", [c.name for c in BC.CASES])
def test_operands_make_the_softmax_exact(name):
    o, segs = _segments(name)
    B, N, H, d = o.q.shape
    for t in [o.q, o.do] + [x for _, s in segs for x in (s.k, s.v)]:
        assert t.dtype == torch.float32
        for dt in (torch.bfloat16, torch.float16):
            assert torch.equal(t.to(dt).float(), t), "an operand is not representable in bf16 / f16 / fp32"
    assert float(o.do.abs().max()) <= 2 and torch.equal(o.do, o.do.round())
    for si, sg in segs:
        L, k = sg.k.shape[1], sg.kexp
        # distinct codes per (sample, head): one code <-> one group or orphan; a decoy carries its twin's key row and other values
        for b in range(B):
            for h in range(H):
                keys = _code_key((sg.k[b, :, h, :16] != 0).float()).tolist()
                assert bool(((sg.k[b, :, h, :16] != 0).sum(-1) == 8).all())
                owner = {}
                for j in range(L):
                    g = int(sg.grp[b, h, j])
                    if g == -2:
                        continue
                    ident = g if g >= 0 else -10 - j
                    assert owner.setdefault(keys[j], ident) == ident, f"{name}: two groups of sample {b} head {h} share a code"
                for j in range(L):
                    if int(sg.grp[b, h, j]) == -2:
                        assert sg.bias[b, j] == MASK_BIAS and owner.get(keys[j], -1) >= 0
                        twins = [t for t in range(L) if sg.grp[b, h, t] >= 0 and torch.equal(sg.k[b, t, h], sg.k[b, j, h])]
                        assert twins and all(not torch.equal(sg.v[b, t, h], sg.v[b, j, h]) for t in twins)
                    elif sg.bias is not None:
                        assert sg.bias[b, j] == 0
        # every P is 0 or 2^-k, every row holds 2^k of them
        assert bool(((sg.P == 0) | (sg.P == 2.0 ** -k)).all()) and bool((sg.P.sum(-1) == 1).all())
        # exponents as the kernels form them: the group's keys exactly -k, every other key (masked ones included) at most -151
        sc = torch.einsum("bnhd,blhd->bhnl", o.q.double(), sg.k.double())
        assert torch.equal(sc, sc.round()) and float(sc.abs().max()) < 2 ** 24
        e = _fl32(sc * _scale_log2(d))
        if sg.bias is not None:
            e = _fl32(e + _fl32(sg.bias.double() * LOG2E_F)[:, None, None, :])
        e = _fl32(e - k)
        assert bool((e[sg.P > 0] == -k).all()), "a group key's exponent is not exactly -k"
        others = torch.where(sg.P == 0, e, torch.full_like(e, -1.0e9))
        assert float(others.max()) <= -151.0, f"{name}: a non-group exponent of {float(others.max())}"
        assert bool((torch.exp2(others.float()) == 0).all())
        # O is the integer c_group: the deviations cancel
        O = torch.einsum("bhnl,blhd->bnhd", sg.P, sg.v.double())
        assert torch.equal(O, sg.O) and torch.equal(O, O.round()) and float(O.abs().max()) <= 4
        # a masked key receives nothing, an orphan nothing
        dead = (sg.grp < 0)  # [B, H, L]
        assert not bool(sg.P.permute(0, 1, 3, 2)[dead].any())


def _share(t):
    return float((t != 0).double().mean())


@pytest.mark.parametrize("name,mode", _PARAMS, ids=[f"{n}-{m}" for n, m in _PARAMS])
def test_expected_gradients_are_determined(name, mode):
    dtype = BC.MODES[mode]
    bt = BC.build(name, mode)
    o, a = bt.ops, BC.BY_NAME[name].args
    B, N, H, d = o.q.shape
    sc = BC.scale32(d)
    for si, (sg, r) in enumerate(zip(o.segs, bt.refs)):
        L, k, s = sg.k.shape[1], sg.kexp, sg.s
        dS, unit = r["dS"], 2.0 ** -k * s
        ints = dS / unit
        assert torch.equal(ints, ints.round()), "dS 2^k / s is not an integer"
        if dtype != torch.float32:  # the 16-bit hand-over of P and dS to the second MFMA is exact
            m = torch.frexp(ints)[0].abs() * 2.0 ** BC.MANT[dtype]
            assert torch.equal(m, m.round()), f"{name}: a dS needs more than {BC.MANT[dtype]} significant bits"
            assert torch.equal(rne(dS, dtype).double(), dS) and torch.equal(rne(sg.P, dtype).double(), sg.P)
        # every sum, and the sum of the magnitudes of its terms, below 2^24 units of the common denominator: exact in fp32 in any order
        for A in (r["absq"], r["absk"]):
            assert float(A.max()) / unit < 2 ** 24
        assert float(torch.einsum("bhnl,bnhd->blhd", sg.P, o.do.double().abs()).max()) * 2.0 ** k < 2 ** 24
        assert float((o.do.double().abs().sum(-1) * 7).max()) < 2 ** 24 and float(r["delta"].abs().max()) / s < 2 ** 24
        for A in (r["Aq"], r["Ak"], r["Av"]):
            assert float((_fl32(A * sc)).abs().max()) < 65504.0
        # every 32-query tile and every 32-key tile that holds a group key holds non-zero dS (k = 0: dS = 0 by construction, P instead)
        w = dS if k > 0 else sg.P
        if k == 0:
            assert not bool(dS.any()) and not bool(r["Aq"].any()) and not bool(r["Ak"].any())
        for b in range(B):
            for h in range(H):
                for q0 in range(0, N, 32):
                    assert bool(w[b, h, q0:q0 + 32].any()), f"{name}: query tile {q0 // 32} of ({b}, {h}) holds no dS"
                for k0 in range(0, L, 32):
                    if bool((sg.grp[b, h, k0:k0 + 32] >= 0).any()):
                        assert bool(w[b, h, :, k0:k0 + 32].any()), f"{name}: key tile {k0 // 32} of ({b}, {h}) holds no dS"
        if k > 0 and N >= 32:
            live = (sg.grp >= 0).permute(0, 2, 1)  # [B, L, H]: masked and orphan keys are zero by construction and do not count
            shares = _share(r["Aq"]), _share(r["Ak"][live]), _share(r["Av"][live])
            assert shares[0] >= 0.25 and shares[1] >= 0.25 and shares[2] >= 0.50, f"{name}: non-zero shares dq {shares[0]:.0%} dk {shares[1]:.0%} dv {shares[2]:.0%}"
    for key, e in bt.exp.items():
        if e.bits is not None:
            assert e.bits.dtype == dtype and bool(torch.isfinite(e.bits.float()).all())
            assert not bool(((e.bits == 0) & torch.signbit(e.bits)).any()), "an expected -0.0"
    if a.get("acc"):  # the accumulate cases round: a fifth of the sums at least is not representable
        v = _fl32(bt.refs[0]["Aq"] * sc) + bt.dq0["acc_round"].double()
        off = float((rne(v, dtype).double() != v).double().mean())
        assert off >= 0.20, f"{name} [{mode}]: only {off:.1%} of the accumulated sums round"
        vi = _fl32(bt.refs[0]["Aq"] * sc) + bt.dq0["acc_int"].double()
        assert torch.equal(bt.dq0["acc_int"], bt.dq0["acc_int"].round()) and float(vi.abs().max()) < 65504
    if "L2" in a:  # the IP pair: the audio segment's dq lands on the text segment's stored dq
        assert bool(bt.dq0["ip"].any()) and bool(bt.refs[1]["Aq"].any())


@pytest.mark.parametrize("name", [c.name for c in BC.CASES])
def test_reference_agrees_with_autograd(name):
    """the analytic reference (P given) against torch autograd through softmax(Q K^T / sqrt(d) + bias) V in fp64, to 1e-12 of the largest element"""
    o, segs = _segments(name)
    B, N, H, d = o.q.shape
    for si, sg in segs:
        r = BC.backward64(o.q, o.do, sg)
        q, k, v = (t.double().requires_grad_(True) for t in (o.q, sg.k, sg.v))
        z = torch.einsum("bnhd,blhd->bhnl", q, k) / math.sqrt(d)
        if sg.bias is not None:
            z = z + sg.bias.double()[:, None, None, :]
        out = torch.einsum("bhnl,blhd->bnhd", torch.softmax(z, -1), v)
        assert float((out.detach() - sg.O).abs().max()) <= 1e-12 * max(1.0, float(sg.O.abs().max()))
        out.backward(o.do.double() * sg.s)
        top = max(float(t.abs().max()) for t in (q.grad, k.grad, v.grad))  # (k = 0: dq = dk = 0 against autograd's 1e-50)
        for got, want in ((r["Aq"] / math.sqrt(d), q.grad), (r["Ak"] / math.sqrt(d), k.grad), (r["Av"] * sg.s, v.grad)):
            assert float((got - want).abs().max()) <= 1e-12 * top


def _emulate_f32(ds, x):
    """csrc/f32_ops.hip's order in fp32: ds [B, H, R, M] (already fl32(ds * scale)), x [B, H, M, d] -> [B, H, R, d].  Lane l of the row's wave runs
    the FMA chain over the terms l, l + 64, ...; six butterfly adds follow.  (fp64 holds each product and each two-term sum exactly before the
    rounding, so fl32 of it is the fused operation's rounding.)"""
    B, H, R, M = ds.shape
    T = (M + 63) // 64
    pad = 64 * T - M
    ds = torch.cat([ds, ds.new_zeros(B, H, R, pad)], -1).reshape(B, H, R, T, 64)
    x = torch.cat([x, x.new_zeros(B, H, pad, x.shape[-1])], 2).reshape(B, H, T, 64, -1)
    acc = ds.new_zeros(B, H, R, 64, x.shape[-1])
    for t in range(T):
        acc = _fl32(acc + ds[:, :, :, t, :, None] * x[:, :, None, t])
    lane = torch.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        acc = _fl32(acc + acc[:, :, :, lane ^ off])
    assert bool((acc == acc[:, :, :, :1]).all())
    return acc[:, :, :, 0]


_F32_BOUND = [c.name for c in BC.CASES if "f32" in c.modes and not BC.pow2_scale(c.args["d"])]


@pytest.mark.parametrize("name", _F32_BOUND)
def test_f32_bound_constant_holds_for_the_kernels_order(name):
    """the fp32 kernels where the scale is no power of two: an emulation of their order stays inside c 2^-24 A with c = F32_COEFF (and is not
    bit-equal to the unrounded reference, or the bound would be idle)"""
    bt = BC.build(name, "f32")
    o = bt.ops
    B, N, H, d = o.q.shape
    sc = BC.scale32(d)
    moved = 0
    for si, (sg, r) in enumerate(zip(o.segs, bt.refs)):
        ds = _fl32(r["dS"] * sc)
        got_q = _emulate_f32(ds, sg.k.double().permute(0, 2, 1, 3)).permute(0, 2, 1, 3)
        got_k = _emulate_f32(ds.transpose(2, 3), o.q.double().permute(0, 2, 1, 3)).permute(0, 2, 1, 3)
        checks = [("dk" + ("" if si == 0 else "2"), got_k)]
        if si == 0:
            checks.append(("dq", got_q))
            for kind in bt.dq0:
                checks.append(("dq_" + kind, _fl32(bt.dq0[kind].double() + got_q)))
        for key, got in checks:
            e = bt.exp[key]
            assert e.bits is None and e.c == BC.F32_COEFF(sg.k.shape[1] if key.startswith("dq") else N)
            err = (got - e.ref).abs()
            assert bool((err <= e.c * 2.0 ** -24 * e.A).all()), f"{name} {key}: the emulation leaves the bound by {float((err / (2.0 ** -24 * e.A).clamp_min(1e-300)).max()):.2f} units (c = {e.c})"
            moved += int((err > 0).sum())
    assert moved > 0 or BC.BY_NAME[name].args["k"] == 0  # (k = 0: every dS is 0, A = 0 and the bound is an equality)


def test_table_covers_the_axes():
    args = [c.args for c in BC.CASES]
    assert {a["d"] for a in args} == {16, 32, 48, 64, 80, 128} and [c.modes for c in BC.CASES if c.args["d"] == 128] == [("f32",)]
    Ls = {a["L"] for a in args} | {a["L2"] for a in args if "L2" in a}
    assert {1, 8, 31, 32, 33, 64, 65, 96, 97, 160} <= Ls
    assert {a["N"] for a in args} == {1, 31, 32, 33, 97, 129, 160}
    assert {a["k"] for a in args} == {0, 1, 2, 3, 4} and {a.get("s", 1.0) for a in args} == {1.0, 0.5}
    odd = lambda n: ((n + 31) // 32) % 2 == 1 and n > 32
    for d in (16, 32, 48, 64, 80):  # every head size meets an odd tile count above one in both passes, at k >= 1
        assert any(a["d"] == d and odd(a["N"]) and (odd(a["L"]) and a["k"] > 0 or odd(a.get("L2", 0))) for a in args), d
    assert any(a["H"] == 3 and a["d"] == 16 for a in args) and any(a["B"] == 3 for a in args)
    assert {a.get("bias") for a in args} == {None, "edges", "tile0"}
    assert any(a.get("bias") == "edges" and a["L"] % 32 == 1 for a in args) and any(a.get("unmasked") is not None for a in args)
    assert sum(1 for a in args if a.get("acc")) >= 2 and any("L2" in a for a in args) and any(a["N"] == a["L"] for a in args)
    assert BC.BY_NAME[BC.CONTROL].args == dict(B=2, H=2, N=32, L=2, d=16, k=1) and set(BC.AUTOGRAD) <= set(BC.BY_NAME)
