"""-m gpu: the normalisation kernels held to rows with exact statistics.

The tolerance tests (test_layernorm, test_groupnorm, test_groupnorm_two_sources, the backward tests: N(0, 1) operands, 2e-2 of max|ref|) cannot see one
pixel left out of a GroupNorm's sums at HW = 1000, a chunk partial that is never added, statistics taken from the neighbouring group, the wrong
source's batch modulo, the second half of a 16-byte vector normalised with the first half's group, or gamma / beta shifted by a lane.  Here every
set (LayerNorm row, GroupNorm slab) is built from small integers, so that its sums are exact in fp32 in any order; the cases, the two tiers, the
derivation of the bound and ``route_of`` live in tests/norm_exact_cases.py, the tier conditions are asserted on the CPU (tests/test_norm_exact_host.py):
  tier R   16-bit modes: the output is +-gamma + beta IN EVERY BIT (ops.layer_norm, ops.group_norm, ops.group_norm2, ops.rms_norm; ops.l2_normalize
           of a +-a row of 256 channels is +-1/16 in every bit, in fp32 too); with SiLU (tier "S") and in fp32: the bound below (SiLU in fp32: the
           normalised value is not rounded there, so A = 1.1 A_pre + |silu(y)| + |y|: NC.expected).
  tier K   spiked integers, small-variance and flat sets: |out - ref64| <= 0.5 ulp_dtype(ref64) + 16 * 2^-24 * A.
  backward ops.layer_norm_bwd (no dres), ops.group_norm_bwd (no SiLU): the same bound with A = rstd (|dy g| + |mean(dy g)| + |mean(dy g xhat)|).
Every output is a util.guarded buffer (stray and missing writes are named), the allocator's free blocks are NaN-filled before each test, and every case
asserts that it lands on the kernel form it is named after (NC.check_route).  ops.group_norm2 must equal ops.group_norm on the concatenation bit for bit.
The 16 is derived in norm_exact_cases.py, in fp32 roundings of A: the mean's quotient 1, x - mean 1, the variance under |mean| <= sigma with its eps add and
rsqrtf 5.5, the three multiplies / adds 3: 11 - 12, the rest left to the shifted form's inexact sum of squares.  The host's fp32 emulation of both
variance formulas, in two summation orders, reaches 0.21 (E[x^2] - mean^2) and 0.91 (shifted form, on the 40000-element slab) of the bound.
No tolerance in this file or its case file was chosen by looking at a kernel's output; every test prints its worst error / bound before asserting (on
the MI355X the fp32 modes stay below 0.25 of it forward and 0.56 backward; a 16-bit output whose reference lies next to a rounding tie reaches 1.00
of it, as it must).

What the file sees -- one-line mutants of norm.hip, train_ops.hip, rpgemm.hip, xattn.hip, hsattn.hip and attention.hip (all under
ap-adapter_amd/csrc/), each built apart from the tree, each IN BOUNDS (an
element dropped or an index swapped among valid ones), each run once on the MI355X against the existing normalisation tests ("old": test_layernorm,
test_groupnorm, test_groupnorm_two_sources, test_layer_norm_bwd, test_group_norm_bwd, test_layer_norm_bwd_entry, test_group_norm_bwd_entry: 202
tests; the row-panel mutant: the test_rowpanel_* tests) and once against this file ("new": its 429 tests outside the fused attention cases):
  1. gn_partial_kernel: ``p1 = min(p0 + GN_CHUNK, HW) - 1`` on the last chunk (the last pixel never summed): old 0 of 202; new 38 ("gn_twopass_C1280_HW1000
     [R, bf16]: 6512 of 3840000 elements differ; first at (row 0, column 419): expected 0.125, got 0.12451171875"; in bf16 tier R sees it only where
     the output is small -- every tier-K case of the two-pass form fails in both 16-bit types).
  2. ``g1 = c0 / cg`` in gn_apply_kernel (both loops) and gn_onepass_kernel: old 10 (groups of 4, 12, 20 and 28 channels, where a vector's second
     half lies in the next group); new 76 ("gn_full4_C128_HW1 [R, bf16]: 146 of 384 elements differ; first at (row 0, column 6): expected -1.625, got -0.875").
  3. gn_vec: ``bi % s.Bb`` -> 0: old 8; new 24: every gn2 case ("gn2_HW64_Ba4_Bb2 [R, bf16]: two sources against the concatenation: 17880 of
     163840 elements differ; first at (row 64, column 380)").
  4. gn_finalize_kernel's loop stopped at 64 chunks: old 0 of 202 (4000 pixels are 63 chunks); new 6: gn_twopass_66chunks in every tier and 16-bit type
     ("[R, bf16]: 81195 of 133152 elements differ; first at (row 0, column 0): expected 6.375, got 6.40625").
  5. layernorm_kernel: variance divided by C - 8: old 5 (f16 only); new 76 ("ln_C8_M1 [R, bf16]: 8 of 8 elements differ; ... expected 1.375, got 1.75").
  6. layernorm_kernel: gamma read one vector to the left (clamped at 0): old 10; new 64 ("ln_C256_M1 [R, bf16]: 236 of 256 elements differ; first at
     (row 0, column 8): expected -0.625, got -3.375"; C = 8 has one vector and cannot show it).
  7. gn_bwd_kernel: gamma read one 4-channel piece to the left (clamped): old 120; new 6: the 20-channel groups ("gn_bwd_C640_HW1 [R, bf16]: 1274 of 1280
     elements leave the half-ulp bound"; C = 32 has one piece per group).
  8. rp_gemm_kernel's LayerNorm: gamma of the 16-channel chunk to the left (clamped): old 20 of the 66 test_rowpanel_* tests; new 8: every
     rp_ln case ("rp_ln_K256_M130_N128 [R, bf16]: 16580 of 16640 elements differ; first at (row 0, column 0): expected -24.375, got -9.875").
No mutant survived this file; mutants 1 and 4 survive every older test.  The whole file (451 tests) takes 31 s on the MI355X, no test more than 0.3 s.

LayerNorm inside the linear kernels, tier R: ops.fused_linear(ln=) on the row-panel kernel (K = 256, 384; M = 5, 33, 130) gives rne(y W^T + b) in every bit
(bit equality: the normalised operand is rounded to the storage type before the matrix instruction, and it is exact); ops.linear(ln=) at K = 640 behind a
rowstat=True producer holds the bound form (rstd multiplies after the sum, so its rounding reaches the output).  Both kernel lines are quoted in
norm_exact_cases.py.

LayerNorm inside the fused attention kernels (tests/norm_attn_cases.py, 11 cases in bf16 and f16): ops.fused_cross_attention(ln=),
ops.cross_attention_rows(ln=), ops.hs_attention(normalize=True) cross and self, ops.self_attention_fused.  The signs of a tier-R row carry the selection
tier's codes through the LayerNorm; the output is V[sel] (rne(x + V[sel]) where the entry adds its residual) in every bit; self_attention_fused: the
elements whose exact value is 0 are held to |out| <= 2^-16 (the algebraic form leaves gamma eps / (2 a^2) there), every other element to bits.
Mutants of these kernels, run against the 252 tests of test_gpu_kernels.py with "attention" in their name ("old") and the 22 tests here ("new"):
  9. xattn.hip, fold_q: the column sums of the next 8 head dims (``8 * ((g + 1) & 3)``): old 35; new 4: every xattn_ln case.
  10. hsattn.hip: ``nm = -mean`` (the mean not scaled by rstd): old 2; new 10: every hs_cross_ln and hs_self_ln case.
  11. attention.hip, xattn_rows_kernel's LayerNorm: gamma read one vector to the left (clamped): old 36; new 4: every xrows_ln case.
  12. attention.hip, sattn_fused_kernel: ``mean = shift[n]`` (the mean's second term dropped): old 44; new 4: every sattn_ln case.

The GELU / GEGLU consumers (hs_geglu, geglu_mlp*, layernorm_geglu_packed) are held on tier-R rows by tests/test_gpu_exact_activation.py (the activation
is exact where it saturates).  Left out: ``dres`` and SiLU in the backward (both round to the storage type mid-way); off-centre sets (deliberate, see
norm_exact_cases.py).  A balanced two-valued row of 256 channels shows a reduction that is one vector short only in f16 (eight elements of 256 missing move
the mean by at most a / 32 and the output by a few 2^-8 of gamma: around half a bf16 ulp, many f16 ulp); tier K's spikes show it in every mode."""
import pytest
import torch

import norm_attn_cases as NA
import norm_exact_cases as NC
from util import assert_bits_equal, assert_within_half_ulp, guarded, nan_fill_free, ulp_of

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _stale_results_read_as_nan(dev):
    """every test starts with the allocator's free blocks NaN-filled (see tests/test_gpu_kernels.py)"""
    nan_fill_free(dev)


def _launch(c, bt, tier, dtype, ops, dev, out):
    D = lambda t: t.to(dev, dtype).contiguous()
    silu, op, eps = tier == "S", c.op, bt.eps
    if op == "ln":
        return ops.layer_norm(D(bt.x), D(bt.gamma), D(bt.beta), eps, out=out)
    if op == "gn":
        return ops.group_norm(D(bt.x), D(bt.gamma), D(bt.beta), bt.groups, eps, silu=silu, out=out)
    if op == "gn2":
        return ops.group_norm2(D(bt.xa), D(bt.xb), D(bt.gamma), D(bt.beta), bt.groups, eps, silu=silu, out=out)
    if op == "rms":
        return ops.rms_norm(D(bt.x), D(bt.gamma), eps, out=out)
    if op == "l2":
        return ops.l2_normalize(D(bt.x), out=out)
    if op == "fold_ln":
        K = c.args["C"]
        x = ops.linear(D(bt.x), torch.eye(K, dtype=dtype, device=dev), rowstat=True)  # the producer: stores the tier-R rows and their statistics
        assert_bits_equal(x, D(bt.x), "producer")
        rs = ops.rowstat_of(x)
        assert rs is not None and tuple(rs.shape) == (c.args["M"], K // 64, 2)
        xs = bt.x.double().reshape(-1, K // 64, 64)
        assert torch.equal(rs.cpu().double(), torch.stack([xs.sum(-1), (xs * xs).sum(-1)], -1)), "the producer's row statistics are not the exact sums"
        w = D(bt.w)
        assert ops.ln_foldable(x, w)
        return ops.linear(x, w, D(bt.wb), ln=(D(bt.gamma), D(bt.beta), eps), out=out)
    if op == "rp_ln":
        assert ops.rp_ok(D(bt.x)) and c.args["N"] % 64 == 0  # fused_linear's own condition for the row-panel launch
        return ops.fused_linear(D(bt.x), D(bt.w), D(bt.wb), ln=(D(bt.gamma), D(bt.beta), eps), out=out)
    if op == "ln_bwd":
        return ops.layer_norm_bwd(D(bt.x), D(bt.gamma), D(bt.dy), eps, out=out)
    assert op == "gn_bwd"
    return ops.group_norm_bwd(D(bt.x), D(bt.gamma), D(bt.beta), D(bt.dy), bt.groups, eps, False, out=out)


def _check(name, tier, mode, dev):
    from ap_adapter_amd import ops
    c, dtype = NC.BY_NAME[name], NC.DTYPES[mode]
    NC.check_route(c, dtype)
    bt = NC.build(name, tier)
    what = f"{name} [{tier}, {mode}]"
    shape = tuple(bt.ref.shape)
    view, check = guarded(bt.ref.numel() // shape[-1], shape[-1], dtype, dev)
    out = _launch(c, bt, tier, dtype, ops, dev, view.view(shape))
    check(what)
    assert out.data_ptr() == view.data_ptr() and tuple(out.shape) == shape
    if c.op == "gn2":
        single = ops.group_norm(bt.x.to(dev, dtype), bt.gamma.to(dev, dtype), bt.beta.to(dev, dtype), bt.groups, bt.eps, silu=tier == "S")
        assert_bits_equal(out, single, what + ": two sources against the concatenation")
    ref, absref = NC.expected(name, tier, dtype)
    bound = 0.5 * ulp_of(ref, dtype) + NC.COEFF * NC.U * absref
    print(f"  {what}: worst |out - ref64| / bound {float(((out.cpu().double() - ref).abs() / bound).max()):.3f}")
    if NC.expects_bits(c, tier, dtype):
        assert_bits_equal(out, bt.y.float().to(dtype), what)
    else:
        assert_within_half_ulp(out, ref, absref, dtype, what, coeff=NC.COEFF)


_PARAMS = NC.params()
_FWD = ("ln", "gn", "gn2", "rms", "l2")
_FUSED = ("rp_ln", "fold_ln")


def _sel(tiers, ops_):
    p = [(n, t, m) for n, t, m in _PARAMS if t in tiers and NC.BY_NAME[n].op in ops_]
    return dict(argvalues=p, ids=[f"{n}-{t}-{m}" for n, t, m in p])


@pytest.mark.parametrize("name,tier,mode", **_sel("RS", _FWD))
def test_two_valued_sets_give_gamma_plus_beta(dev, name, tier, mode):
    """tier R (S: with SiLU): mean = m, variance = a^2; 16-bit output +-gamma + beta in every bit"""
    _check(name, tier, mode, dev)


@pytest.mark.parametrize("name,tier,mode", **_sel("K", _FWD))
def test_spiked_integer_sets_to_half_an_ulp(dev, name, tier, mode):
    """tier K: integers in [-3, 3] with +-48 spikes on the edges of every loop; small-variance and flat sets"""
    _check(name, tier, mode, dev)


@pytest.mark.parametrize("name,tier,mode", **_sel("R", ("ln_bwd", "gn_bwd")))
def test_backward_of_two_valued_sets_to_half_an_ulp(dev, name, tier, mode):
    """ln_bwd_kernel / gn_bwd_kernel: tier R x, integer dy with spikes"""
    _check(name, tier, mode, dev)


@pytest.mark.parametrize("name,tier,mode", **_sel("R", _FUSED))
def test_layernorm_inside_the_linear_kernels(dev, name, tier, mode):
    """ops.fused_linear(ln=) at K = 256 / 384 (row-panel): the normalised operand is +-gamma + beta exactly, every product sum is exact: rne(y W^T + b)
    in every bit; ops.linear(ln=) at K = 640 (folded): rstd multiplies after the exact sum: the bound form"""
    _check(name, tier, mode, dev)


@pytest.mark.parametrize("name,mode", NA.params(), ids=[f"{n}-{m}" for n, m in NA.params()])
def test_layernorm_inside_the_fused_attention_kernels_bit_for_bit(dev, name, mode):
    """tests/norm_attn_cases.py: tier-R rows whose signs carry the selection tier's codes through the LayerNorm: V[sel] (+ x) in every bit"""
    from ap_adapter_amd import ops
    c, dtype, bt = NA.BY_NAME[name], NC.DTYPES[mode], NA.build(name)
    view, check = guarded(c.B * c.N, c.C, dtype, dev)
    out = NA.run(name, dtype, ops, dev, view.view(c.B, c.N, c.C))
    check(f"{name} [{mode}]")
    assert out.data_ptr() == view.data_ptr()
    if c.route == "sattn":  # v by algebra on the gamma = beta channels is gamma (1 - a rstd), not 0: below 2^-16, its bits not determined (NA docstring)
        zero = (bt.ref == 0).to(dev)
        assert float(out[zero].float().abs().max()) <= 2.0 ** -16, f"{name} [{mode}]: a value that should be gamma * eps / (2 a^2) is not"
        out = torch.where(zero, torch.zeros_like(out), out)
    assert_bits_equal(out, (bt.ref.float() + 0.0).to(dtype), f"{name} [{mode}]")
