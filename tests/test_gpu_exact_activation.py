"""-m gpu: the GELU, GEGLU, SiLU and tanh consumers held to saturated and integer gates.

The tolerance tests (test_rowpanel_geglu, test_geglu_mlp*, test_layernorm_geglu_packed*, test_hs_geglu, test_geglu_fwd_bwd, test_linear_geglu: N(0, 1)
operands, 2e-2 of max|ref|) pass with one wrong hidden unit, a value / gate pair taken from the neighbouring chunk or a truncated hidden activation;
the torch.equal checks between kernel forms prove that they agree, not that either is right.  Here the activation is exact because it saturates
(tests/act_exact_cases.py: the classes, the operands, the derivation of the bound, ``route``; the tier conditions are asserted on the CPU in
tests/test_act_exact_host.py):
  tier Z   every gate is 0 or saturated, its sign decided by the token; values odd integers; every hidden activation, stage and output an integer of
           at most 256: the output is util.rne of the fp64 reference IN EVERY BIT (a zero of either sign is a zero), in every storage type.
  tier G   gates on the half-integer grid within 5.5, integer values: |out - ref64| <= 0.5 ulp_T + |v| (|g| / 2 E + 3 * 2^-24 |gelu64(g)|), E = 1.5e-7 +
           28 * 2^-24 for gelu_erf_2's order (29 for gelu_erf_f's); the feed-forward adds 2^k 0.5 ulp_T(h) for the 16-bit hand-over of h and 0.5 ulp_T(h W2^T + b2) for its
           epilogue's first rounding.  Every test prints its worst |error| / bound before asserting.  No bound here was chosen by looking at a kernel's output.
  one function per pair: every forward kernel on gelu_erf_2's operation order gives the same output bits for the same (v, g), in bf16 and in f16.
Every output is a util.guarded buffer, the allocator's free blocks are NaN-filled before each test, every case asserts the dispatch conditions of the
kernel form it is named after (AC.route).

Forms: ops.linear(act=) tiled in bf16, f16, fp32 "highest" and "high" (geglu, gelu, silu) and the fp32-only epilogues (tanh, gelu_tanh, geglu_tanh);
the LDS-DMA ring form with the GEGLU epilogue; ops.linear(act="geglu", ln=) at K = 640 behind a rowstat producer; ops.conv1d(act="tanh") with a tap per output unit;
ops.fused_linear(act=) on rpgemm (K = 256, 384, with and without LayerNorm, the eight-wave form at 32805 rows) and wsgemm (GELU, SiLU, N <= 512);
ops.geglu_mlp and ops.geglu_mlp_packed (also out = x); ops.layernorm_geglu_packed; ops.hs_geglu and ops.hs_geglu + ops.hs_ff2; ops.geglu and
ops.geglu_bwd.

What the file sees -- one-line mutants of the kernels under ap-adapter_amd/csrc/, each built apart from the tree, each IN BOUNDS (a wrong element
inside the buffers and registers the launch already owns), each run once on the MI355X against the existing activation tests ("old": the 178 tests of
test_gpu_kernels.py, test_gpu_forward_bounds.py, test_gpu_train.py, test_gpu_backward_shapes.py and test_gpu_f32_split.py selected by "geglu or gelu or
mlp or silu") and against this file ("new", 363 tests):
  1. gemm_shared.h, epi_store: value and gate swapped for the second 8-column vector of a tile: old 14; new 50 ("linear_geglu_77x64x72 [Z, bf16]: 689 of
     4928 elements differ; first at (row 0, column 8): expected -80.0, got -2.384185791015625e-05").
  2. gemm_shared.h, epi_acc_to_lds: b1 not added to the gate half: old 14; new 42 ("... 1810 of 4928 elements differ; first at (row 0, column 0): expected
     -48.0, got -24.0").
  3. rpgemm.hip: the gate bias of a tile's second 16-unit chunk taken from the first: old 41; new 36 ("rp_geglu_K256_M1_ln0 [Z, bf16]: 262 of 1024
     elements differ; first at (row 0, column 22): expected 32.0, got 24.0").
  4. mlp.hip: the hidden activation truncated instead of rounded (one of each pair): old 31 (the bit-equalities between kernel forms); new 6: tier Z
     cannot see it (integers), tier G and the one-function test do ("mlp_M37 [G, bf16]: 39 of 9472 elements leave the half-ulp bound; first at (row 0,
     column 30): expected -0.9998733150326675, got -0.984375, error 3.968 ulp").
  5. mlp3.hip, apad_mlp_pack: one value row (unit 53) not halved in bf16: old 19; new 8 ("mlp_packed_M65 [Z, bf16]: 54 of 16640 elements differ; first
     at (row 2, column 48): expected 39.0, got 23.0").
  6. mlp3_shared.h, M3GegluT: hx of the even unit not halved in the f16 path: old 37; new 32 ("mlp_packed_M1 [Z, f16]: 125 of 256 elements differ;
     first at (row 0, column 2): expected 156.0, got 316.0").
  7. mlp3_shared.h: the A&S coefficient 1.421413741 of the even unit changed in its fourth digit: old 68 (bit-equalities); new 4: the packed C = 384
     kernel's tier-G cases in f16 ("lngeglu_M257_ln1_b1 [G, f16]: 2399 of 394752 elements leave the half-ulp bound ... error 0.610 ulp") and the
     one-function test in both types; the fused feed-forward's tier-G bound is too wide for it (the hand-over terms), its selection case enters
     through the one-function test.
  8. train_ops.hip, geglu_bwd_kernel: dgate written where dvalue belongs for the second 8-element chunk: old 12; new 12 ("geglu_bwd_37x1024 [Z, bf16]:
     195 of 75776 elements differ; first at (row 0, column 8): expected 0.0, got -15.0").
  9. hsattn.hip, hs_geglu: the gate takes the value half's bias: old 16; new 24 ("hs_geglu_B1_N1_norm1 [Z, bf16]: 1445 of 2560 elements differ").
  10. geglu3.hip, apad_geglu_pack: the gate biases of neighbouring units swapped: old 30; new 26 ("lngeglu_M1_ln1_b1 [Z, bf16]: 895 of 1536 elements differ").
  11. wsgemm.hip: the fourth element of each SiLU quad left unactivated: old 0 of 178; new 8: every ws_silu case ("ws_silu_K256_M37 [Z, bf16]: 755 of
      9472 elements differ; first at (row 0, column 7): expected 0.0, got -112.0").
  12. rpgemm.hip: the GELU epilogue activates element 1 of a quad twice, element 2 never: old 0 of 178; new 4: every rp_gelu case ("rp_gelu_K256_M37
      [Z, bf16]: 2879 of 21312 elements differ; first at (row 0, column 2): expected 16.0, got 0.0").
No mutant survived this file; mutants 11 and 12 survive every older test.  (A thirteenth, "the gate of the last 16-unit chunk of a tile from the
previous one" in rpgemm.hip, changes nothing: that kernel's tiles hold one chunk.)  The whole file (363 tests) takes 39 s on the MI355X with its
output printed, no test more than 0.4 s; tests/test_act_exact_host.py takes 11 s on the CPU.  In tier G the 16-bit kernels reach 1.00 of the bound
(a reference next to a rounding tie, as it must), the fp32 modes 0.20.

The fused feed-forward's epilogue rounds twice, rne(rne(h W2^T + b2) + x) (mlp.hip: ``y[0] = (typename E::elem)(yacc[ct][4 * g + 0] + b4.x);`` before
scratch_flush adds x; the same in mlp3.hip and hs_ff2), and the tier-G bound counts both roundings.  The route of a case is asserted on its shape only
(act_exact_cases.py, ``route``)."""
import pytest
import torch

import act_exact_cases as AC
from util import assert_bits_equal, assert_within_half_ulp, guarded, nan_fill_free, rne, ulp_of

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _stale_results_read_as_nan(dev):
    """every test starts with the allocator's free blocks NaN-filled (see tests/test_gpu_kernels.py)"""
    nan_fill_free(dev)


def _launch(name, tier, mode, dev):
    from ap_adapter_amd import ops
    c, dtype = AC.BY_NAME[name], AC.MODES[mode]
    AC.route(c, mode)
    shape = AC.out_shape(name, tier)
    view, check = guarded(AC.build(name, tier)["ref"].numel() // shape[-1], shape[-1], dtype, dev)
    out = AC.run(name, tier, mode, ops, dev, out=view.view(shape))
    what = f"{name} [{tier}, {mode}]"
    check(what)
    assert out.data_ptr() == view.data_ptr() and tuple(out.shape) == shape
    return out, what, dtype


def _check(name, tier, mode, dev):
    out, what, dtype = _launch(name, tier, mode, dev)
    ref, bound = AC.expected(name, tier, mode)
    o = out.cpu().reshape(ref.shape)
    if bound is None:
        assert_bits_equal(torch.where(o == 0, torch.zeros_like(o), o), rne(ref + 0.0, dtype), what)
    else:
        print(f"  {what}: worst |out - ref64| / bound {float(((o.double() - ref).abs() / bound).max()):.3f}")
        assert_within_half_ulp(o, ref, (bound - 0.5 * ulp_of(ref, dtype)) / AC.U, dtype, what, coeff=1.0)
    return out


def _sel(ops_, tiers):
    p = AC.params(ops_, tiers)
    return dict(argvalues=p, ids=[f"{n}-{t}-{m}" for n, t, m in p])


_GEMM = ("linear", "fold", "fused", "conv1d")
_FF = ("mlp", "mlp_packed", "lngeglu", "hs", "hs_ff")
_EW = ("geglu", "geglu_bwd")


@pytest.mark.parametrize("name,tier,mode", **_sel(_GEMM, "Z"))
def test_saturated_epilogues_of_the_linear_kernels_bit_for_bit(dev, name, tier, mode):
    """tier Z through ops.linear / ops.fused_linear / ops.conv1d: act(x W^T + b) (GEGLU: value * gelu(gate)) is a known integer"""
    _check(name, tier, mode, dev)


@pytest.mark.parametrize("name,tier,mode", **_sel(_FF, "Z"))
def test_saturated_feed_forward_kernels_bit_for_bit(dev, name, tier, mode):
    """tier Z through the fused feed-forward kernels: GEGLU, the 16-bit hand-over of h, the second GEMM, b2 and the residual"""
    out = _check(name, tier, mode, dev)
    c = AC.BY_NAME[name]
    if c.op in ("mlp", "mlp_packed"):  # out = x: the same bits
        from ap_adapter_amd import ops
        bt, dtype = AC.build(name, tier), AC.MODES[mode]
        view, check = guarded(c.args["M"], AC.MLP_C, dtype, dev)
        view.copy_(bt["w"].x.to(dev, dtype))
        D = lambda t: None if t is None else t.to(dev, dtype).contiguous()
        w = bt["w"]
        ln = None if w.ln is None else (D(w.ln[0]), D(w.ln[1]), w.ln[2])
        if c.op == "mlp":
            o2 = ops.geglu_mlp(view, D(w.w1), D(w.b1), D(bt["w2"]), D(bt["b2"]), ln=ln, out=view)
        else:
            wp, bp = ops.mlp_pack(D(w.w1), D(w.b1), D(bt["w2"]))
            o2 = ops.geglu_mlp_packed(view, wp, bp, D(bt["b2"]), ln=ln, out=view)
        check(f"{name} [{tier}, {mode}] out = x")
        assert_bits_equal(o2, out, f"{name} [{tier}, {mode}] out = x against out of place")


@pytest.mark.parametrize("name,tier,mode", **_sel(_EW, "Z"))
def test_saturated_stored_projection_geglu_forward_and_backward(dev, name, tier, mode):
    """ops.geglu / ops.geglu_bwd: h = v g or 0; dvalue = dh g or 0, dgate = dh v, dh v / 2 (g = 0) or 0"""
    _check(name, tier, mode, dev)


@pytest.mark.parametrize("name,tier,mode", **_sel(_GEMM + _FF + _EW, "G"))
def test_half_integer_gates_within_the_derived_bound(dev, name, tier, mode):
    """tier G: the unsaturated range, against fp64 within the bound act_exact_cases.py derives"""
    _check(name, tier, mode, dev)


_ONE_FUNCTION = ("linear_geglu_77x64x72", "linear_geglu_130x192x136", "linear_geglu_nobias_77x64x72", "ring_geglu_77x64x128", "ring_geglu_130x192x256",
                 "rp_geglu_K256_M37_ln0", "rp_geglu_K384_M37_ln0", "rp_geglu_K256_M37_ln1", "lngeglu_M257_ln1_b1", "hs_geglu_B3_N37_norm0",
                 "mlp_M130_select", "mlp_packed_M130_select")


@pytest.mark.parametrize("mode", AC.M16)
def test_one_function_of_value_and_gate_across_the_geglu_kernels(dev, mode):
    """common.h: "every GEGLU kernel of the library evaluates THIS operation order": the same (v, g) gives the same output bits on the tiled and ring
    GEMM epilogues, the row-panel kernel, the packed C = 384 kernel, the 64-token kernel and (through a +-2^k selection in W2, off the hot column of
    the one-hot x) both fused feed-forward kernels"""
    dtype = AC.MODES[mode]
    table = torch.full((17 * 23,), -1, dtype=torch.int64)
    owner = [""] * (17 * 23)
    for name in _ONE_FUNCTION:
        out, what, _ = _launch(name, "G", mode, dev)
        bt = AC.build(name, "G")
        w = bt["w"]
        o = out.cpu().reshape(bt["ref"].shape).float().double()
        v, g = w.v, w.g
        if "w2" in bt:  # out[t, j] = x[t, j] + w2[j, u] h[t, u]: where x is 0, h = out / w2 exactly (a power of two)
            w2 = bt["w2"].double()
            u = w2.abs().argmax(1)
            scale = w2[torch.arange(w2.shape[0]), u]
            keep = w.x.double() == 0
            o, v, g = (o / scale)[keep], v[:, u][keep], g[:, u][keep]
        bits = rne(o.reshape(-1), dtype).view(torch.int16).long() & 0xFFFF
        bits = torch.where(o.reshape(-1) == 0, torch.zeros_like(bits), bits)  # (a zero of either sign)
        key = ((v.reshape(-1) + 8) * 23 + (2 * g.reshape(-1) + 11)).long()
        first = torch.full_like(table, -1)
        first[key] = bits  # (any representative: the comparison below catches a pair with two outputs inside the case too)
        fresh = table < 0
        table = torch.where(fresh, first, table)
        for k in torch.nonzero(fresh & (first >= 0)).reshape(-1).tolist():
            owner[k] = name
        bad = table[key] != bits
        if bool(bad.any()):
            i = int(bad.to(torch.uint8).argmax())
            k = int(key[i])
            raise AssertionError(f"{what}: (v, g) = ({k // 23 - 8}, {(k % 23 - 11) / 2}) gives bits {int(bits[i]):#06x}, {owner[k]} gave {int(table[k]):#06x}; "
                                 f"{int(bad.sum())} of {bad.numel()} elements differ from the first kernel's function")
    assert int((table >= 0).sum()) >= 300, "the kernels together saw too little of the (v, g) table"
