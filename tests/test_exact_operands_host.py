"""CPU: the integer-operand cases of tests/test_gpu_exact_linear.py stay inside their tier -- every reference value an integer, sums below
2^24, tier A at most 256 (what bf16 holds exactly), tier B far above the exactly-held range with enough rounded outputs and ties -- so a case
whose reference leaves its tier is found here, not on the GPU.  Plus: rne against hand-written ties, and synthetic wrong "kernels" that the
bit comparison must reject."""
import pytest
import torch
import torch.nn.functional as F

import exact_cases as EC
from util import assert_bits_equal, assert_exact_conditions, exact_case, int_operand, rne, unrepresentable_and_ties


@pytest.mark.parametrize("name,tier,mode", [p for p in EC.params() if p[2] in ("bf16", "f16")] +
                         [p for p in EC.params() if p[2] == "highest" and "bf16" not in EC.BY_NAME[p[0]].modes])
def test_case_reference_stays_in_its_tier(name, tier, mode):
    """(tier A operands do not depend on the mode: the 16-bit modes stand for the fp32 ones, whose bound is the same 256)"""
    bt = EC.build(name, tier, mode)
    dtype = EC.MODES[mode]
    for t in bt.t.values():
        if isinstance(t, torch.Tensor) and t.is_floating_point():
            assert torch.equal(t, t.round())
    for vname, v in bt.variants.items():
        side = list(v.get("side", {}).values())
        if tier == "B":
            assert not side
        assert_exact_conditions(list(v["out"].values()), v["inter"], dtype if dtype != torch.float32 else torch.bfloat16, tier, bt.K,
                                bt.amp_x, bt.amp_w, side=side)


def test_exact_case_amplitudes():
    """the amplitudes the rule gives at the reductions it was worked out for"""
    assert [exact_case(K, torch.bfloat16, "B")[0] for K in (72, 136, 2560, 11520)] == [15, 12, 6, 4]
    assert [exact_case(K, torch.float16, "B")[0] for K in (72, 136, 2560, 11520)] == [42, 36, 17, 12]
    assert exact_case(72, torch.float32, "A") == (2, 1, 1.0) and exact_case(2560, torch.bfloat16, "A") == (2, 1, 36.0 ** 2 / 5120)
    for K in (72, 136, 2560, 11520):
        for dt in (torch.bfloat16, torch.float16):
            a = exact_case(K, dt, "B")[0]
            assert K * a * a <= 1.7e6


def test_int_operand():
    t = int_operand(300, 70, amp=3, seed=5)
    assert t.dtype == torch.float32 and torch.equal(t, t.round()) and float(t.min()) == -3 and float(t.max()) == 3
    assert torch.equal(t, int_operand(300, 70, amp=3, seed=5)) and not torch.equal(t, int_operand(300, 70, amp=3, seed=6))
    s = int_operand(300, 70, amp=1, seed=5, density=0.25)
    assert 0.10 < float((s != 0).float().mean()) < 0.25  # 2/3 of the kept quarter is non-zero


def test_rne_on_hand_written_ties():
    t = lambda *v: torch.tensor(v, dtype=torch.float64)
    assert rne(t(257, 259, 258, 261, 263, -257, -259, 256, 255), torch.bfloat16).tolist() == [256, 260, 258, 260, 264, -256, -260, 256, 255]
    assert rne(t(2049, 2051, 2050, -2049, 4098, 4102, 2048), torch.float16).tolist() == [2048, 2052, 2050, -2048, 4096, 4104, 2048]
    assert rne(t(16777215, -3), torch.float32).tolist() == [16777215, -3]
    off, tie = unrepresentable_and_ties(t(257, 258, 513, 514, 1028, 7), torch.bfloat16)
    assert (off, tie) == (4 / 6, 3 / 6)  # 257, 514, 1028 are ties; 513 is rounded but no tie


def _synthetic(dtype=torch.bfloat16, K=136):
    ax, aw, _ = exact_case(K, dtype, "B")
    x, w = int_operand(70, K, amp=ax, seed=1).double(), int_operand(72, K, amp=aw, seed=2).double()
    b, r = int_operand(72, amp=100, seed=3).double(), int_operand(70, 72, amp=100, seed=4).double()
    return x, w, b, r


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_wrong_kernels_fail_the_comparison(dtype):
    """a right "kernel" passes; one that drops one k-term, truncates, or rounds once after the residual does not"""
    x, w, b, r = _synthetic(dtype)
    acc = F.linear(x, w)
    expected = rne(rne(acc + b, dtype).double() + r, dtype)
    assert_exact_conditions([rne(acc + b, dtype).double() + r], [acc, acc + b], dtype, "B", x.shape[1], *exact_case(x.shape[1], dtype, "B")[:2])
    assert_bits_equal(rne(rne(F.linear(x.float(), w.float()).double() + b, dtype).double() + r, dtype), expected)  # fp32 accumulation: exact
    # one k-term of one output dropped
    nz = int((x[5] * w[7]).abs().argmax())
    assert x[5, nz] * w[7, nz] != 0
    acc2 = acc.clone()
    acc2[5, 7] -= x[5, nz] * w[7, nz]
    with pytest.raises(AssertionError, match=r"first at \(row 5, column 7\)"):
        assert_bits_equal(rne(rne(acc2 + b, dtype).double() + r, dtype), expected, "dropped k-term")
    # truncation (round toward zero) in the epilogue
    def trunc(t64):
        rn = t64.float().to(dtype)
        over = rn.double().abs() > t64.abs()  # rounded away from zero: one step back in the sign-magnitude bit pattern
        return torch.where(over, (rn.view(torch.int16) - 1).view(dtype), rn)
    with pytest.raises(AssertionError, match="elements differ"):
        assert_bits_equal(trunc(trunc(acc + b).double() + r), expected, "truncating epilogue")
    # one rounding, after the residual
    with pytest.raises(AssertionError, match="elements differ"):
        assert_bits_equal(rne(acc + b + r, dtype), expected, "rounded once")


def test_tier_a_off_by_one_is_a_difference_of_one():
    x, w = int_operand(77, 72, amp=2, seed=1).double(), int_operand(8, 72, amp=1, seed=2).double()
    acc = F.linear(x, w)
    assert_exact_conditions(acc, [acc], torch.bfloat16, "A", 72, 2, 1)
    bad = acc.clone()
    bad[76, 7] += 1
    with pytest.raises(AssertionError, match=r"1 of 616 elements differ; first at \(row 76, column 7\).*difference 1\.0"):
        assert_bits_equal(rne(bad, torch.bfloat16), rne(acc, torch.bfloat16))
    with pytest.raises(AssertionError):  # and a reference that leaves the tier is refused
        assert_exact_conditions(acc + 300, [acc], torch.bfloat16, "A", 72, 2, 1)
