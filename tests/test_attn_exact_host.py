"""The operands of the exact-softmax attention tests (tests/attn_exact_cases.py) checked on the CPU, on the fp64 reference alone: under these
conditions the result of a correct kernel is determined -- in every bit (tier S) or to half a storage ulp plus a few fp32 ulp (tiers U and P) -- and
a dropped, doubled or misplaced key moves it visibly.  tests/test_gpu_exact_attention.py runs the same cases on the GPU."""
import math

import pytest
import torch

import attn_exact_cases as AC
from util import ulp_of

_PARAMS = [(c.name, t) for c in AC.CASES for t in c.tiers]
LOG2E_F = float(torch.tensor(1.4426950408889634, dtype=torch.float32))


def _fl32(t):
    return t.float().double()


def _kernel_scale(args):
    """the fp32 factor the kernels multiply a raw score by: softmax_scale (a float) * log2(e) in fp32, or exactly 1 for a pre-scaled q"""
    if args.get("prescaled"):
        return 1.0
    return float(torch.tensor(1.0 / math.sqrt(args["d"]), dtype=torch.float32) * torch.tensor(1.4426950408889634, dtype=torch.float32))


def _d(case):
    return AC.FUSED[case.route]["d"] if case.route in AC.FUSED else case.args["d"]


def _dtypes(case):
    return [torch.float32] if case.modes == AC.F32 else [torch.bfloat16, torch.float16]


def _segments(case, bt):
    a = case.args
    return [(bt.segs[0], a.get("kvdiv", 1), 1.0)] + ([(bt.segs[1], a.get("kvdiv2", 1), a["scale2"])] if len(bt.segs) == 2 else [])


def _without_key(bt, seg, kvdiv, j, scale):
    """the segment's fp64 attention with key j removed"""
    keep = [i for i in range(seg.k.shape[1]) if i != j]
    bias = None if seg.bias is None else seg.bias[:, keep]
    return AC.attention64(bt.q, seg.k[:, keep], seg.v[:, keep], scale, bias, kvdiv)[0]


def _assert_sensitive(case, bt, dtype):
    """removing the first key, the last key or the last key of any 64-key tile moves more than half of the output columns (that carry values) of some
    query by more than 2 ulp of the storage type.  Two segments: 2 ulp of the segment's own branch w * A_seg, which the 16-bit kernels round on its own
    (in the blended sum a 512-key second segment beside 8 text keys of weight 1 / 8 can stay below the bf16 ulp of the text branch: what holds such a
    key loop to every key is tier S)"""
    a = case.args
    scale = AC.LN2 if a.get("prescaled") else 1.0 / math.sqrt(_d(case))
    for seg, kvdiv, w in _segments(case, bt):
        L = seg.k.shape[1]
        if L < 2:
            continue
        ulp = ulp_of(w * seg.ref, dtype)
        cols = (seg.v != 0).reshape(-1, seg.v.shape[-1]).any(0)
        for j in sorted({0, L - 1} | {min(AC.KT * t + AC.KT - 1, L - 1) for t in range((L + AC.KT - 1) // AC.KT)}):
            moved = (w * (_without_key(bt, seg, kvdiv, j, scale) - seg.ref)).abs() > 2.0 * ulp  # [B, N, H, d]
            frac = moved[..., cols].double().mean(-1)
            assert float(frac.max()) > 0.5, f"{case.name}: dropping key {j} of {L} moves at most {float(frac.max()):.0%} of a query's columns by 2 ulp ({dtype})"


@pytest.mark.parametrize("name,tier", _PARAMS, ids=[f"{n}-{t}" for n, t in _PARAMS])
def test_conditions_of_the_tier_hold_on_the_reference(name, tier):
    case, bt = AC.BY_NAME[name], AC.build(name, tier)
    a = case.args
    c = _kernel_scale(dict(a, d=_d(case)))
    for t in [bt.q] + [x for s in bt.segs for x in (s.k, s.v)] + ([bt.x] if bt.x is not None else []):
        assert t.dtype == torch.float32
        for dt in (torch.bfloat16, torch.float16):
            assert torch.equal(t.to(dt).float(), t), "an operand is not representable in bf16 / f16 / fp32"
    for seg, kvdiv, w in _segments(case, bt):
        s = seg.scores  # q . k, unscaled, [B, H, N, L]
        L = s.shape[-1]
        assert torch.equal(s, s.round()) and float(s.abs().max()) < 2 ** 24, "scores are not integers below 2^24"
        if tier == "S":
            z = _fl32(_fl32(s) * c)
            if seg.bias is not None:
                z = _fl32(z + _fl32(_fl32(seg.bias) * LOG2E_F)[:, None, None, :])
            zsel = z.gather(-1, seg.sel[..., None])
            assert bool((zsel == 0).all()), "a selected key's scaled score is not exactly 0"
            others = z.scatter(-1, seg.sel[..., None], -1.0e9)
            assert float(others.max()) <= -150.0, "an unselected key scores above -150"
            assert bool((torch.exp2(others.float()) == 0).all())  # fp32 exp2, with or without denormals
            B, H, N = seg.sel.shape
            vv = seg.v.double()[torch.arange(B) // kvdiv]  # [B, L, H, d]
            picked = vv.permute(0, 2, 1, 3)[torch.arange(B)[:, None, None], torch.arange(H)[None, :, None], seg.sel]  # [B, H, N, d]
            # (fp64 keeps weights like exp(-362) that fp32 does not: they show only where V[sel] is 0, and vanish in the reference's fp32 step)
            assert torch.equal(seg.ref.float(), picked.permute(0, 2, 1, 3).float()), "the softmax does not give weight 1 to the selected key and 0 to the rest"
            chosen = set(seg.sel.reshape(-1).tolist())
            tiles_with_real = {j // AC.KT for j in seg.real}
            if B * H * N >= len(tiles_with_real) + 3:
                assert {seg.real[0], seg.real[-1]} <= chosen and {j // AC.KT for j in chosen} == tiles_with_real
                if seg.bias is None:
                    assert 0 in chosen and L - 1 in chosen
            if seg is bt.segs[0] and N >= 32:  # ... by some query of EVERY full 32-query tile
                for q0 in range(0, N - 31, 32):
                    for b in range(B):
                        for h in range(H):
                            got = set(seg.sel[b, h, q0:q0 + 32].tolist())
                            assert {j // AC.KT for j in got} == tiles_with_real and {seg.real[0], seg.real[-1]} <= got
            if seg.bias is not None:  # every decoy is masked, carries its twin's key and other values
                for j, twin in AC._decoys(L).items():
                    assert bool((seg.bias[:, j] == AC.MASK_BIAS).all()) and torch.equal(seg.k[:, j], seg.k[:, twin]) and not torch.equal(seg.v[:, j], seg.v[:, twin])
                    assert twin in chosen
        elif tier == "U":
            nz = seg.v[seg.v != 0]  # (the fused entries with a residual keep V off the code dims)
            assert not bool(bt.q.any()) and torch.equal(seg.v, seg.v.round()) and 1 <= float(nz.abs().min()) and float(nz.abs().max()) <= 4
            assert bool((seg.v != 0).reshape(-1, seg.v.shape[-1]).all(0).sum() >= seg.v.shape[-1] - 32)
            assert 4 * L < 2 ** 24
            if seg.bias is not None:
                n = (seg.bias == 0).sum(1)
                assert int(n.min()) >= 1
                if L > 32:
                    assert any(bool((seg.bias[b, 32 * ((L - 1) // 32):] == AC.MASK_BIAS).all()) for b in range(seg.bias.shape[0])), "no sample masks the whole ragged sub-tile"
        else:
            assert float(s.max()) == 0 and float(s.min()) >= -3 and torch.equal(seg.v, seg.v.round())
            T = (L + AC.KT - 1) // AC.KT
            first = s[..., :AC.KT].amax(-1)
            assert bool((first == 0).any())
            if T >= 2:
                before_last = s[..., :AC.KT * (T - 1)].amax(-1)
                assert bool(((first == -3) & (before_last < 0) & (s.amax(-1) == 0)).any()), "no query's maximum rises from -3 in tile 0 to 0 in the last tile"
    for dtype in _dtypes(case):
        if tier in "UP":
            _assert_sensitive(case, bt, dtype)
        if tier == "U" and case.route == "xattn":
            # the normalised weights are rounded to the storage type (AC.xattn_weights): determined if an ulp of the reciprocal either way does not move them
            for si in range(len(bt.segs)):
                w = AC.xattn_weights(bt, si, dtype)
                for e in (-2.0 ** -22, 2.0 ** -22):
                    assert torch.equal(AC.xattn_weights(bt, si, dtype, rcp_err=e), w) or bt.segs[si].k.shape[1] > 128
        elif tier in "UP" and len(bt.segs) == 2 and dtype != torch.float32:
            # the 16-bit kernels round each branch before the blend: the roundings are determined if no branch value is nearer to a tie than the
            # fp32 error of the branch (an exact integer sum times a rounded reciprocal: a few fp32 ulp of the VALUE, so 0 stays 0)
            # (tier U: none -- S / L with an integer S cannot come that close; tier P: a few, and AC.expected admits both neighbours there)
            for seg in bt.segs:
                frac = float(AC.near_tie(seg.ref, dtype).mean())
                assert frac == 0 if tier == "U" else frac < 0.01, f"{name}: {frac:.2%} of a branch's values lie within the fp32 error of a rounding tie ({dtype})"


def test_route_of_every_case_is_the_dispatchers():
    for c in AC.CASES:
        assert AC.route_of(c.args, c.modes != AC.F32, route=c.route) == c.route, c.name
    assert {c.route for c in AC.CASES} == {"short", "generic", "2q", "2q_direct", "f32", "xattn", "xrows", "hs_cross", "hs_self"}


def test_fused_rows_carry_codes_and_values_apart():
    """the fused entries: x is the query operand (W_q = identity) and, where the entry adds its residual, zero on the value dims"""
    for c in AC.CASES:
        if c.route not in AC.FUSED:
            continue
        bt = AC.build(c.name, "S" if "S" in c.tiers else c.tiers[0])
        B, N, H, d = bt.q.shape
        x = bt.x.reshape(B, N, H, d)
        if c.route in ("xattn", "xrows"):
            assert not bool(x[..., 16:].any()) and all(not bool(s.v[..., :16].any()) for s in bt.segs)
        if c.route == "hs_self":
            wq, wk, wv = (w.double() for w in AC.hs_self_weights("S"))
            xf = bt.x.double()
            assert torch.equal((xf @ wq.t()).reshape(B, N, H, d), bt.q.double()) and torch.equal((xf @ wk.t()).reshape(B, N, H, d), bt.segs[0].k.double())
            assert torch.equal((xf @ wv.t()).reshape(B, N, H, d), bt.segs[0].v.double())
        else:
            assert torch.equal(x, bt.q)


def test_code_sets_are_distinct():
    cs = AC.code_sets(3, 1029, 5)
    assert cs.shape == (3, 1029, 16) and bool((cs.sum(-1) == 8).all())
    for g in range(3):
        assert len({tuple(r.tolist()) for r in cs[g]}) == 1029
