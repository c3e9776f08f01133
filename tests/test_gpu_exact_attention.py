"""-m gpu: the attention kernels held to selection, uniform and power-of-two softmaxes.

A softmax cannot be exact for arbitrary inputs, but it is where every probability is 0, 1 or a power of two -- and those inputs are the ones that
expose indexing, masking, tail and rescale errors, which the tolerance tests (N(0, 1) operands, 2e-2 of max|ref|, each of L weights about 1 / L)
cannot see.  The cases, their operands and fp64 references live in tests/attn_exact_cases.py (the three tiers are described there) and are checked
against the conditions of their tier on the CPU (tests/test_attn_exact_host.py).  Here every case goes through its public wrapper -- ops.attention /
ops.attention_lse (attn_short_kernel, attn_kernel, attn2q_kernel classic and direct, the fp32 attention "highest" and "high"),
ops.fused_cross_attention, ops.cross_attention_rows, ops.hs_attention (cross and self):
  tier S  the output is V[sel(i)] (two segments: rne(V1[sel1] + scale2 * V2[sel2])) in EVERY bit, in bf16, f16, fp32 "highest" and fp32 "high";
          the log-sum-exp is exactly 0.0 for every real query and 0.0 in the pad entries [N, round_up(N, 32)) (attn_kernel: "the pad entries ...
          are written too (0)").  Why: p_sel = exp2(0) = 1, every other p = exp2(<= -261) = 0 with or without denormals, the denominator is 1.
  tiers U, P  |out - ref| <= 0.5 ulp(ref) + 8 * 2^-24 * A(|V|): all sums are exact (integers, or multiples of 1/8, below 2^24), so the inexact
          steps are 1 / den, the multiply by it -- a few fp32 ulp of the magnitude A(|V|): the second term, which also absorbs a 1-ulp exp2 in tier
          P -- and the final rounding: the first.  lse = log2(unmasked keys) within 4 fp32 ulp.
Neither bound was tuned against a kernel's output; the two rounding models the references state (each branch of a two-segment launch rounded before
the blend; xattn_kernel's normalised weights rounded to the storage type) are quoted from the kernels' source in attn_exact_cases.py.  The output
buffer is a guarded one (util.guarded): stray and missing writes are named.  The raw and the rows_pack_kv forms of a key / value set must agree in
every bit.  The conditions that route a case to its kernel form (csrc/attention.hip launch_d, the wrappers' envelope functions, the key counts that
select a fused kernel's resident / split / chunked form) are asserted in ``AC.route_of``.

What the file sees -- one-line mutants of csrc/attention.hip / xattn.hip, each built apart from the tree and run once on the MI355X against every test
of test_gpu_kernels.py with "attention" in its name (252 tests: apad_attention's own 89 and the fused sub-layers, which compare against the
ops.attention chain), then against this file (280 tests).  "old": failures among the 252, in brackets among the 89 that call ops.attention directly.
  1. tile_compute's masked path, ``key < L`` -> ``key < L - 1``: old 61 [15: L = 100, 513, 70]; 58 fail here ("generic_L65 [S, bf16]:
     8320 of 16640 elements differ; first at (row 2, column 0): expected -0.8828125, got -0.0078125").
  2. ``bias[key]`` read as ``bias[key - 1]`` (clamped) in tile_compute: old 6 [0: every direct masked test passes; only three fused tests' comparison
     with the chain notices]; 8 fail here ("generic_masked_L257 [S, bf16]: 8342 of 38400 elements differ; first at (row 0, column 0): expected
     -0.8203125, got 0.79296875": the decoy at key 0 hands its mask to its twin).
  3. the last P.V step of a full tile skipped (``st < 3``) in tile_compute: old 57 [15]; 54 fail here ("generic_L65 [S, bf16]: 1792 of 16640 elements
     differ; first at (row 13, column 0): expected 0.050537109375, got 0.0").
  4. tile_compute2, classic form: the rescale skipped when the maximum moves (alpha = 1): old 70 [32]; 24 fail here ("2q_200x200_d32 [S, bf16]: 27555
     of 38400 elements differ"); tier U passes by construction (its maximum never moves), tiers S and P fail.
  4b. the same in the direct form's range-check branch: old 6 [6: the spike tests]; the 6 direct tier-S cases fail here ("direct_200x200 [S, bf16]:
     16778 of 38400 elements differ; first at (row 1, column 0): expected -1.484375, got -0.1123046875").
  5. the K/V group of segment 1: the issue's ``b / kvdiv`` -> ``b / kvdiv2`` reads past the key tensor wherever kvdiv > kvdiv2, so it was replaced by
     "group g > 0 reads group g - 1" (attn_kernel and attn_short_kernel): old 1 [1: test_attention_shared_kv_batch_div]; 12 fail here
     ("short_dual_kvdiv [S, bf16]: 7656 of 15360 elements differ; first at (row 160, column 0): expected -23.5, got 14.875").
  6. xattn.hip's chunked form: one half of the running sum not rescaled on chunk 1: old 8 [the 192 / 256 / 512-key cases]; the 4 chunked tier-S cases
     fail here ("xattn_8_192 [S, bf16]: 2499 of 25344 elements differ; first at (row 1, column 16): expected -107.0, got -79.0").
No mutant survived this file.  The tolerance tests are not blind to mutants 1, 3, 4 and 6 (random operands at L of a few hundred move by more than
2e-2 of max|ref| too); what they miss is mutant 2 in every test that calls ops.attention directly.

Out of scope: ``apad_self_attention_fused`` (its LayerNorm cannot be switched off, so q, k and v are never exact; its key loop ``tile_compute2`` is
the one attn2q_kernel runs here), ``window_attention`` and the text-encoder and CLAP towers.  The backward (``attention_bwd``) has its own exact suite,
tests/test_gpu_exact_attention_bwd.py."""
import pytest
import torch

import attn_exact_cases as AC
from util import assert_bits_equal, assert_within_half_ulp, guarded, nan_fill_free

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _stale_results_read_as_nan(dev):
    """every test starts with the allocator's free blocks NaN-filled (see tests/test_gpu_kernels.py)"""
    nan_fill_free(dev)


def _check(name, tier, mode, dev):
    from ap_adapter_amd import ops
    case, dtype = AC.BY_NAME[name], AC.MODES[mode]
    a = case.args
    assert AC.route_of(a, dtype in ops.FUSED_DTYPES, ops, case.route) == case.route, "not on the kernel form the case is named after"
    bt = AC.build(name, tier)
    B, N, H, d = bt.q.shape
    what = f"{name} [{tier}, {mode}]"
    view, check = (None, None) if a.get("lse") else guarded(B * N, H * d, dtype, dev)
    out, lse = AC.run(name, tier, mode, ops, dev, out=None if view is None else view.view(B, N, H * d))
    if check is not None:
        check(what)
    ref, absref = AC.expected(name, tier, dtype)
    if tier == "S":
        assert_bits_equal(out, (ref.float() + 0.0).to(dtype), what)
    else:
        assert_within_half_ulp(out, ref, absref, dtype, what)
    if a.get("lse"):
        Np = ops.round_up(N, 32)
        assert lse.dtype == torch.float32 and tuple(lse.shape) == (B, H, Np)
        bias = bt.segs[0].bias
        keys = torch.full((B,), float(bt.segs[0].k.shape[1])) if bias is None else (bias == 0).sum(1).float()
        want = torch.zeros(B, H, Np, dtype=torch.float64)
        if tier != "S":
            want[..., :N] = torch.log2(keys.double())[:, None, None]
        if tier == "S":
            assert_bits_equal(lse, want.float(), what + " lse")
        else:
            assert_bits_equal(lse[..., N:].contiguous(), want[..., N:].float().contiguous(), what + " lse pad entries")
            err = (lse[..., :N].cpu().double() - want[..., :N]).abs()
            tol = 4.0 * 2.0 ** -23 * torch.exp2(torch.floor(torch.log2(want[..., :N].clamp_min(2.0 ** -126))))
            assert bool((err <= tol).all()), f"{what} lse: worst error {float((err / tol.clamp_min(1e-300)).max()) * 4:.2f} fp32 ulp of log2(keys)"


_PARAMS = AC.params()


@pytest.mark.parametrize("name,tier,mode", [p for p in _PARAMS if p[1] == "S"], ids=[f"{n}-{m}" for n, t, m in _PARAMS if t == "S"])
def test_selection_softmax_bit_for_bit(dev, name, tier, mode):
    """tier S: one key scores 0, every other at most -261 in the exponent: the output is that key's value row in every bit"""
    _check(name, tier, mode, dev)


@pytest.mark.parametrize("name,tier,mode", [p for p in _PARAMS if p[1] == "U"], ids=[f"{n}-{m}" for n, t, m in _PARAMS if t == "U"])
def test_uniform_softmax_to_half_an_ulp(dev, name, tier, mode):
    """tier U: q = 0, every unmasked key weighs 1 / den; integer values, exact sums"""
    _check(name, tier, mode, dev)


@pytest.mark.parametrize("name,tier,mode", [p for p in _PARAMS if p[1] == "P"], ids=[f"{n}-{m}" for n, t, m in _PARAMS if t == "P"])
def test_power_of_two_softmax_to_half_an_ulp(dev, name, tier, mode):
    """tier P (q pre-scaled): weights 1, 1/2, 1/4, 1/8; the running maximum rises from -3 to 0 for some queries and never moves for others"""
    _check(name, tier, mode, dev)
