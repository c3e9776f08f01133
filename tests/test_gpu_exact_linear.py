"""-m gpu: the linear kernels held to integer operands, bit for bit.

With small-integer operands every product and partial sum is an integer below 2^24, so fp32 accumulation is exact in any order and the result
of a linear kernel is a known integer: the output must equal it, correctly rounded to the storage type, in EVERY bit -- one dropped, doubled
or misplaced element moves an output by at least 1.  The reference is the same operation in fp64 torch on the CPU; the cases, their operands
and references live in tests/exact_cases.py and are checked against the conditions of their tier on the CPU
(tests/test_exact_operands_host.py).  Tier A: every value at most 256, the same expected bits in bf16, f16, fp32 "highest" and fp32 "high".
Tier B (16-bit): outputs far above the exactly-held range, so the epilogue's rounding is exercised: rne(acc + bias + row-group bias), then,
with a residual, rne(that + residual) (csrc/gemm_shared.h).

Every case goes through the public ``ops`` wrappers; the conditions of the dispatcher that route a case to its kernel form are asserted on the
shape in ``_route``.

What the bit comparison sees that the tolerance tests do not -- one-line mutants of csrc/gemm.hip / gemm_shared.h, each built apart from the
tree and run once on the MI355X against test_gpu_kernels.py's test_gemm_plain_bias_residual, test_gemm_rowgroup_bias_and_step,
test_gemm_ring_form_equals_the_tiled_kernel_bit_for_bit, test_conv3x3_implicit_gemm and test_patch_embed (41 tests), then against this file:
  * residual row ``(m + 1) % residual_row_mod``: the 41 pass; 28 fail here ("gemm_77x8x72 [A, bf16] residual_mod.out: 599 of 616 elements
    differ; first at (row 0, column 0): expected 1.0, got 3.0, difference 2.0").
  * the bf16 epilogue truncates where it should round to nearest even: the 41 pass; the 7 bf16 tier-B cases of the tiled and ring kernels fail
    ("gemm_513x640x2560 [B, bf16] bias.out: 81440 of 328320 elements differ; first at (row 0, column 0): expected 760.0, got 756.0").
  * the tiled kernel's K tail ends one 8-element vector early when K % 64 != 0 and K > 128: the 41 pass (their only ragged K is 72); 8 fail
    here ("gemm_130x72x136 [A, bf16] bias.out: 8184 of 9360 elements differ; first at (row 0, column 0): expected 1.0, got 10.0").
  * the same for every K % 64 != 0: of the 41 only (77, 8, 72) and the Cin = 8 convolution fail (4 tests); 30 fail here.
  * ``bias[n - 1]`` for the last valid column of a ragged N tile: of the 41 only (77, 8, 72) and the Cout = 96 convolution fail (4 tests); 46
    fail here ("gemm_tile128_40900x24x1024 [A, bf16] bias.out: 40900 of 981600 elements differ; first at (row 0, column 23)").
No mutant survived this file.

Forms not in the table: the big-tile kernel's up-sampled convolution form (>= 16000 output pixels), the 128-tile two-stage convolution, ring
mode 1.  The GEGLU / SiLU / GELU / tanh epilogues and the fused feed-forward are held to saturated gates in tests/test_gpu_exact_activation.py, the
LayerNorm inside the linear kernels in tests/test_gpu_exact_norm.py, attention to exact softmaxes in tests/test_gpu_exact_attention.py."""
import pytest
import torch

import exact_cases as EC
from util import assert_bits_equal, nan_fill_free, rne

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _stale_results_read_as_nan(dev):
    """every test starts with the allocator's free blocks NaN-filled (see tests/test_gpu_kernels.py)"""
    nan_fill_free(dev)


def _blocks128(M, N):
    return ((N + 127) // 128) * ((M + 127) // 128)


def _t128(M, N, K):
    b = _blocks128(M, N)
    return b >= 512 or (b >= 320 and K >= 1024)


def _big_tile_plain(M, N, K):
    """apad_cgemm_try on a plain A operand"""
    return M >= 16000 and N % 128 == 0 and K % 64 == 0 and not (K >= 384 and N >= 640)


def _route(case, ops, dtype):
    """the dispatcher's own conditions (csrc/gemm.hip launch / dispatch_amode, apad_cgemm_try, apad_hconv_try, apad_rowpanel_gemm,
    ops.conv_halo_eligible) for the kernel form the case is named after; -> the number of halo-kernel launches each variant makes"""
    a, name = case.args, case.name
    is16 = dtype in ops.FUSED_DTYPES
    if case.family == "linear" or case.family == "linear2":
        if case.family == "linear2":
            M, N, K = 2 * a["T"], a["N"], a["Ca"] + a["Cb"]
            assert a["Ca"] % 64 == 0
        else:
            M, N, K = a["M"], a["N"], a["K"]
        if name.startswith("big_") or name == "linear2_big":
            assert _big_tile_plain(M, N, K) and is16
            assert (N % 256 == 0) == ("256x256" in name)
        else:
            assert not _big_tile_plain(M, N, K)
            assert _t128(M, N, K) == ("tile128" in name)
            assert (K >= 384 and N >= 640) == ("kgroup" in name or name == "gemm_513x640x2560")  # K groups inside the workgroup
        if a.get("ring"):
            assert is16 and K >= 128 and M < 16000 and K % 64 == 0 and N % 64 == 0  # launch_ring's envelope
        if a.get("rowstat"):
            assert is16 and N % 64 == 0 and N not in ops.RP_K
    elif case.family == "conv":
        B, Cin, Cout, stride = a["B"], a["Cin"], a["Cout"], a.get("stride", 1)
        Hs, Ws = a.get("up") or (a["H"], a["W"])
        pad = 1 if a.get("asym_pad") else 2
        Ho, Wo = (Hs + pad - 3) // stride + 1, (Ws + pad - 3) // stride + 1
        M, K = B * Ho * Wo, 9 * Cin
        halo = is16 and Cin % 64 == 0 and stride == 1 and not a.get("asym_pad") and not a.get("src_batch_mod") and \
            ((Cout % 128 == 0 and Wo in (2, 4, 8, 16)) or (Cout in (8, 16) and Cin in (64, 128) and Wo in (4, 8, 16)))
        dma_ok = is16 and Cin % 64 == 0 and not a.get("asym_pad") and not a.get("src_batch_mod") and stride in (1, 2)
        small = dma_ok and M < 16000 and K >= 2304 and Cout % 64 == 0
        big = dma_ok and M >= 16000 and Cout % 128 == 0
        if a.get("hconv"):
            assert halo and ops.conv_halo_eligible(Cin, Cout, Wo, stride, dtype) == ops.HCONV
            assert ("narrow" in name) == (Cout <= 16) and ("kslices" in name) == (Wo == 2 and Cin // 64 >= 3)
            return 1
        assert small == ("small_ring" in name) and big == ("big_tile" in name)
        if big:
            assert M % 256 != 0
        if name == "conv_two_stage":
            assert K >= 2048 and _blocks128(M, Cout) <= 1024
    elif case.family == "fused":
        M, N, K = a["M"], a["N"], a["K"]
        ws = N <= 512 and N % (256 if K == 256 else 128) == 0  # apad_ws_dispatch: whole resident weight slices
        assert K in ops.RP_K and ws == name.startswith("ws_") and (M >= 32768) == ("8wave" in name)
    elif case.family == "rp3":
        C3 = 3 * EC.QKV_GEOM["heads"] * EC.QKV_GEOM["d"]
        assert C3 <= 512 and (C3 % (256 if a["K"] == 256 else 128) == 0) == (a["K"] == 384)  # K = 256: rpgemm, K = 384: wsgemm
    elif case.family == "hs":
        assert a["N"] <= 64 and is16
    return 0


def _check(name, tier, mode, dev):
    from ap_adapter_amd import ops, _lib as L
    case, dtype = EC.BY_NAME[name], EC.MODES[mode]
    halo_launches = _route(case, ops, dtype)
    bt = EC.build(name, tier, mode)
    n0 = L.lib().apad_hconv_launch_count()
    got = EC.run(name, bt, ops, dev, mode)
    assert L.lib().apad_hconv_launch_count() - n0 == halo_launches * len(bt.variants), "not on the kernel form the case is named after"
    assert set(got) == set(bt.variants)
    for vname, v in bt.variants.items():
        if got[vname] is None:  # (run() asserted that the wrapper refuses this variant in this mode)
            continue
        assert set(got[vname]) == set(v["out"]) | set(v.get("side", {}))
        for oname, ref in v["out"].items():
            assert_bits_equal(got[vname][oname].reshape(ref.shape), rne(ref + 0.0, dtype), f"{name} [{tier}, {mode}] {vname}.{oname}")
        for sname, ref in v.get("side", {}).items():
            out = got[vname][sname]
            assert out.dtype == torch.float32
            assert_bits_equal(out.reshape(ref.shape), (ref + 0.0).float(), f"{name} [{tier}, {mode}] {vname}.{sname} (fp32 side output)")


def test_control_fp32_highest_plain_gemm(dev):
    """the control: the fp32 "highest" plain GEMM (exact-f32 products, fp32 sums) on integer operands gives the integers"""
    _check("gemm_77x8x72", "A", "highest", dev)


@pytest.mark.parametrize("mode", EC.M16)
def test_control_16bit_64_tile_gemm(dev, mode):
    """the second control: integer sums below 2^24 come out of the 16-bit matrix instructions exactly (the 64-tile kernel at (77, 8, 72))"""
    _check("gemm_77x8x72", "A", mode, dev)


_A = [p for p in EC.params() if p[1] == "A"]
_B = [p for p in EC.params() if p[1] == "B"]


@pytest.mark.parametrize("name,tier,mode", _A, ids=[f"{n}-{m}" for n, _, m in _A])
def test_representable_integers_bit_for_bit(dev, name, tier, mode):
    """tier A: every accumulator, intermediate and output an integer of at most 256 -- the stored bits are the integer's in every mode"""
    _check(name, tier, mode, dev)


@pytest.mark.parametrize("name,tier,mode", _B, ids=[f"{n}-{m}" for n, _, m in _B])
def test_rounded_integers_bit_for_bit(dev, name, tier, mode):
    """tier B: the epilogue's rounding.  apad_gemm's kernels (tiled, ring, big tile, small ring, halo): bias only, and bias + residual as
    rne(rne(acc + bias + row-group bias) + residual).  The row-panel / weight-stationary launches: bias only (a single rounding).  The
    64-token kernels also with the residual, because their source states the order -- csrc/hsattn.hip, hs_out_kernel: "to_out + bias,
    rounded (the chain's first rounding)" and "+ residual (the second rounding)"; hs_ff2: "then bias, rounding, + residual and the row
    statistics exactly as in hs_out_kernel"."""
    _check(name, tier, mode, dev)
