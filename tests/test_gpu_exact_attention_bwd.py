"""-m gpu: the attention backward held to one-hot and 2^-k softmaxes, bit for bit.

A softmax backward is exact where the forward is.  The cases of tests/attn_bwd_exact_cases.py (construction, reference and expected bits are described
there; the conditions under which they are determined are checked on the CPU by tests/test_attn_bwd_exact_host.py) give every query weight 2^-k on the
2^k keys of its group and exactly 0 on every other key, with integer V, dO and K: delta, dP, dS and the three sums are dyadic numbers that fp32 holds
exactly in any order, so dq, dk and dv of ``ops.attention_bwd`` (dq_kernel, dkv_kernel, head_transpose_kernel of csrc/attention_bwd.hip; the fp32 twins
of csrc/f32_ops.hip) are each ONE known value -- compared in every bit, or, for the fp32 twins at a head size whose scale is no power of two, against
the bound counted in the case file.  The backward is fed the exact ``out`` and ``lse`` (NaN in the lse pad entries), so it is held on its own; one
chained variant per case and the autograd entry points take both from ``ops.attention_lse``.  Outputs, transposed copies and delta come from NaN-filled
memory (``_warm_then_fill``): what a launch does not write reads NaN.

Measured here, not assumed: the two controls (exp2 of -k is exactly 2^-k on __builtin_amdgcn_exp2f and on the fp32 kernels' exp2f, k = 0..4) pass, and
``ops.attention_lse`` returns exactly k for a denominator of 2^k in every case (attn_kernel and the fp32 attention; asserted exactly in ``_forward``).

What the file sees that the tolerance tests do not -- in-bounds one-line mutants of csrc/attention_bwd.hip (and the same line of the fp32 twin where it
has one), each built apart from the tree and run ONCE on the MI355X against the two old backward tests (test_gpu_backward_shapes.py::
test_attention_bwd_entry and test_gpu_train.py::test_attention_bwd, 54 tests: N(0, 1) operands, 1.5 x TOL of max|ref|) and against this file without
the transpose and refusal tests (119 tests).  No mutant removes a bound, a clamp or a validity guard that keeps an access inside its buffer.
  mutant                                                                    old tests (54)   this file (119)
  1. delta without dout_scale (both kernels)                                9 fail           39 fail
  2. dq pass: ``key < p.L`` -> ``key < p.Lpad`` (loads stay clamped)        all pass         all pass (equivalent)
  3. dkv pass: ``qq < p.N`` dropped from ``ok``                             all pass         24 fail
  4. dq pass: the middle ``break`` moved after the refill's ``compute``     all pass         all pass (equivalent)
  5. ``accumulate`` adds ``old`` after rounding the new value               all pass         3 fail
  6. dv stored with ``p.scale`` (both kernels)                              36 fail          119 fail
  7. dq pass: ``key < p.L`` -> ``key < p.L - 1`` (the last key dropped)      32 fail          60 fail
  8. dq pass: ``bias[key]`` read as ``bias[key - 1]`` (clamped at 0)        10 fail          22 fail
Four of the eight pass every old test (2, 3, 4, 5); two pass this file, and both are equivalent mutants, not blind spots: (2) the keys of [L, Lpad)
are then weighed like key L - 1, but their dS meets the K^T copy's pad columns, which head_transpose writes as zeros (held by the transpose test
below), so dq does not move in any bit; (4) the re-requested tile is computed a second time at key indices >= L, where ``key < p.L`` gives p = 0.
Messages: 1 "d32_N160_L96_k3 [bf16, plain] dq: 9552 of 20480 elements differ; first at (row 0, column 0): expected -0.1328125, got -0.419921875"
(the old tests see it only at dout_scale = 0.5); 3 "d16_N129_L65_k2_edges [bf16, plain] dk: 4160 of 4160 elements differ; ... expected 0.0, got nan"
(the NaN lse pad entries reach the sums; with the forward's zeros there the pad queries meet zero pad columns of Q^T and dO^T and the chained variant
passes -- "the padded tail of the stats arrays is never trusted" is held by the plain variant alone); 5 "d32_N160_L96_k3 [bf16, acc_int] dq: 467 of
20480 elements differ; first at (row 0, column 19): expected 1.2578125, got 1.25"; 7 "control_N32_L2_d16_k1 [bf16] dq: 968 of 2048 elements differ";
8 "d16_N129_L65_k2_edges [bf16, plain] dq: 248 of 8256 elements differ; first at (row 6, column 1): expected 0.0, got 0.9375" (the decoy at key 0
hands its mask to its twin).

The wrapper refuses what the kernels cannot hold (test_wrapper_refuses_what_the_kernels_cannot_hold): a ``dq=`` of another shape, dtype or stride,
``packed=True`` beside a ``dq=``, an ``lse`` whose rows are not round_up(N, 32) long -- all were accepted before."""
import pytest
import torch

import attn_bwd_exact_cases as BC
from util import assert_bits_equal, int_operand, nan_fill_free, rne

pytestmark = pytest.mark.gpu

@pytest.fixture(autouse=True)
def _stale_results_read_as_nan(dev):
    """every test starts with the allocator's free blocks NaN-filled (see tests/test_gpu_kernels.py)"""
    nan_fill_free(dev)


def _warm_then_fill(dev, run):
    """run once (so the allocator holds blocks of the launch's sizes), drop the outputs, fill the free blocks with NaN, run again: an element, a pad
    column or a delta entry the launch does not write reads NaN"""
    out = run()
    del out
    nan_fill_free(dev)
    return run()


def _hold(got, exp, what):
    """one gradient against its expectation: every bit, or the counted fp32 bound where the scale is no power of two"""
    if exp.bits is not None:
        assert_bits_equal(got, exp.bits, what)
        return
    assert got.dtype == torch.float32 and tuple(got.shape) == tuple(exp.ref.shape), (what, got.dtype, tuple(got.shape))
    err = (got.detach().cpu().double() - exp.ref).abs()
    tol = exp.c * 2.0 ** -24 * exp.A
    bad = ~(err <= tol)  # (a NaN is bad)
    units = float((err / (2.0 ** -24 * exp.A).clamp_min(1e-300))[exp.A > 0].max()) if bool((exp.A > 0).any()) else 0.0
    print(f"  {what}: worst error {units:.2f} x 2^-24 A (bound {exp.c})")
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} of {bad.numel()} elements leave the bound {exp.c} x 2^-24 A; worst {units:.2f}"


def _hold_all(res, bt, variant, what):
    exps = BC.expected_of(bt, variant)
    assert set(k for k, v in res.items() if v is not None) == set(exps), (what, sorted(res), sorted(exps))
    for key, exp in exps.items():
        _hold(res[key], exp, f"{what} {key}")
    for si, sg in enumerate(bt.ops.segs):  # masked keys (and the keys no query looks at) receive exactly 0, in every bit
        dead = (sg.grp < 0).permute(0, 2, 1)  # [B, L, H]
        for key in ("dk", "dv"):
            t = res.get(key + ("" if si == 0 else "2"))
            if t is not None and bool(dead.any()):
                rows = t.cpu()[dead]
                assert not bool(rows.view(torch.int16 if rows.element_size() == 2 else torch.int32).any()), f"{what} {key}: a masked key got a gradient"


def _run(dev, name, mode, variant, fwd=None):
    from ap_adapter_amd import ops
    bt = BC.build(name, mode)
    res = _warm_then_fill(dev, lambda: BC.run(name, bt, ops, dev, mode, variant, fwd))
    torch.cuda.synchronize(dev)
    return bt, res


@pytest.mark.parametrize("mode", BC.ALL)
def test_control_exp2_of_a_small_negative_integer_is_exact(dev, mode):
    """the premise of every k >= 1 case, on the smallest of them (N = 32, L = 2, d = 16, one group of two keys): exp2(-1) is exactly 1/2 on
    __builtin_amdgcn_exp2f (16-bit kernels) and on exp2f (fp32 kernels).  A failure here is a finding about the premise, not about the loops."""
    bt, res = _run(dev, BC.CONTROL, mode, "plain")
    _hold_all(res, bt, "plain", f"{BC.CONTROL} [{mode}]")


@pytest.mark.parametrize("mode", BC.ALL)
def test_control_exp2_is_exact_at_every_k(dev, mode):
    """the second control: one query per k = 0..4 against 2^k keys of one group (d = 16): dv = 2^-k dO for every key in every bit, which holds only
    if exp2(-k) is exactly 2^-k"""
    from ap_adapter_amd import ops
    dtype = BC.MODES[mode]
    for k in range(5):
        g, d = 1 << k, 16
        q = torch.zeros(1, 32, d)
        kk = torch.zeros(1, g, d)
        v = int_operand(1, g, d, amp=3, seed=k)
        if g > 1:
            v = torch.cat([v[:, :g // 2], -v[:, :g // 2]], 1)  # O = 0 (one key: O = v)
        do = int_operand(1, 32, d, amp=2, seed=10 + k)
        D = lambda t: t.to(dev, dtype).contiguous()
        out = torch.zeros(1, 32, d) if g > 1 else v.expand(1, 32, d)
        run = lambda: ops.attention_bwd(D(q), D(kk), D(v), D(out), D(do), BC.exact_lse(1, 1, 32, 32, k, dev), 1)
        dq, dk, dv = _warm_then_fill(dev, run)
        want = (do.double().sum(1, keepdim=True) * 2.0 ** -k).expand(1, g, d)
        assert_bits_equal(dv, rne(want + 0.0, dtype), f"k = {k} [{mode}] dv")
        assert not bool(dq.cpu().any()), f"k = {k} [{mode}]: q = 0 and K = 0, yet dq is not 0"


_PARAMS = BC.params()


@pytest.mark.parametrize("name,mode", _PARAMS, ids=[f"{n}-{m}" for n, m in _PARAMS])
def test_backward_bit_for_bit(dev, name, mode):
    """every variant of the case but the chained one: dq, dk and dv in every bit (fp32 at a scale that is no power of two: the counted bound), masked
    keys exactly 0, dq the same bits with and without the dk / dv pass, packed the same bits as unpacked; at k = 0, dq = 0 holds delta to the last bit"""
    plain = None
    for variant in BC.variants(name, mode):
        if variant.endswith("chained"):
            continue
        what = f"{name} [{mode}, {variant}]"
        bt, res = _run(dev, name, mode, variant)
        _hold_all(res, bt, variant, what)
        if variant == "plain":
            plain = res
        elif variant == "nodkv":
            assert res["dk"] is None and res["dv"] is None
            assert_bits_equal(res["dq"], plain["dq"], what + ": dq changes with need_dkv")
        elif variant == "packed":
            for key in ("dq", "dk", "dv"):
                assert_bits_equal(res[key].contiguous(), plain[key], what + f": packed {key} != unpacked")


def _forward(dev, name, mode):
    """ops.attention_lse of every segment, held: out = rne(O) in every bit, the lse pad entries 0, lse = k"""
    from ap_adapter_amd import ops
    dtype, bt = BC.MODES[mode], BC.build(name, mode)
    o = bt.ops
    B, N, H, d = o.q.shape
    fwd = []
    for si, sg in enumerate(o.segs):
        what = f"{name} [{mode}] segment {si}"
        out, lse = _warm_then_fill(dev, lambda: BC.forward(o, sg, ops, dev, dtype))
        assert_bits_equal(out.reshape(B, N, H, d), rne(sg.O + 0.0, dtype), what + " out")
        Np = ops.round_up(N, 32)
        assert lse.dtype == torch.float32 and tuple(lse.shape) == (B, H, Np)
        l = lse.cpu()
        assert not bool(l[..., N:].view(torch.int32).any()), what + ": lse pad entries are not 0"
        err = float((l[..., :N].double() - sg.kexp).abs().max())
        print(f"  {what}: attention_lse - k: worst {err:.3e} (k = {sg.kexp}, L = {sg.k.shape[1]})")
        # (measured on the MI355X: m + log2(den) is exactly k for den = 2^k in every case and mode, so it is asserted exactly)
        assert err == 0.0, f"{what}: lse differs from k = {sg.kexp} by {err:.3e}"
        fwd.append((out, lse))
    return bt, fwd


@pytest.mark.parametrize("name,mode", _PARAMS, ids=[f"{n}-{m}" for n, m in _PARAMS])
def test_chained_to_the_forward(dev, name, mode):
    """out and lse from ops.attention_lse (every case here reaches attn_kernel, the generic staged form -- a launch that asks for the lse never takes
    attn_short_kernel, and attn2q_kernel needs N and L of 200 at least --, or the fp32 attention): the same gradient bits"""
    from ap_adapter_amd import ops
    bt, fwd = _forward(dev, name, mode)
    variant = "ip_chained" if len(bt.ops.segs) == 2 else "chained"
    res = _warm_then_fill(dev, lambda: BC.run(name, bt, ops, dev, mode, variant, fwd))
    _hold_all(res, bt, variant, f"{name} [{mode}, {variant}]")


@pytest.mark.parametrize("mode", BC.ALL)
@pytest.mark.parametrize("name", BC.AUTOGRAD)
def test_autograd_entry_points_carry_the_same_bits(dev, name, mode):
    """autograd.attention / autograd.ip_attention with .backward(dO): the .grad tensors are the expected bits.  dO arrives non-contiguous (_c(do)); a
    second pass asks for q's gradient alone (need_kv off: the same dq) and hands over a ready V^T (vt=)"""
    from ap_adapter_amd import autograd as AG, ops
    dtype, bt = BC.MODES[mode], BC.build(name, mode)
    o = bt.ops
    B, N, H, d = o.q.shape
    C_ = H * d
    D = lambda t: t.reshape(t.shape[0], t.shape[1], C_).to(dev, dtype).contiguous()
    do = torch.empty(B, C_, N, dtype=dtype, device=dev).transpose(1, 2)
    do.copy_(D(o.do))
    assert not do.is_contiguous()
    sg = o.segs[0]
    bias = None if sg.bias is None else sg.bias.to(dev)
    what = f"{name} [{mode}] autograd"

    def leaves(*ts, grad=True):
        return [D(t).requires_grad_(grad) for t in ts]

    if len(o.segs) == 1:
        assert sg.s == 1.0
        def run(all_grads):
            q, = leaves(o.q)
            k, v = leaves(sg.k, sg.v, grad=all_grads)
            vt = None if all_grads else ops.head_transpose(v, H)
            AG.attention(q, k, v, H, key_bias=bias, vt=vt).backward(do)
            return q.grad, k.grad, v.grad
        dq, dk, dv = _warm_then_fill(dev, lambda: run(True))
        res = {"dq": dq, "dk": dk, "dv": dv}
        variant = "chained"
    else:
        s2 = o.segs[1]
        assert sg.s == 1.0
        def run(all_grads):
            q, = leaves(o.q)
            kt, vt_, ka, va = leaves(sg.k, sg.v, s2.k, s2.v, grad=all_grads)
            AG.ip_attention(q, kt, vt_, ka, va, H, bias, s2.s).backward(do)
            return q.grad, kt.grad, vt_.grad, ka.grad, va.grad
        dq, dk, dv, dk2, dv2 = _warm_then_fill(dev, lambda: run(True))
        res = {"dq": dq, "dk": dk, "dv": dv, "dk2": dk2, "dv2": dv2}
        variant = "ip_chained"
    _hold_all({k_: t.reshape(B, -1, H, d) for k_, t in res.items()}, bt, variant, what)
    only_q = _warm_then_fill(dev, lambda: run(False))
    assert all(t is None for t in only_q[1:])
    assert_bits_equal(only_q[0], res["dq"], what + ": dq changes when k and v take no gradient")


@pytest.mark.parametrize("mode", BC.ALL)
@pytest.mark.parametrize("ntensors", [1, 2, 3])
def test_head_transpose_against_permute(dev, mode, ntensors):
    """ops.head_transpose (one tensor) and ops.head_transpose_many (two and three per launch) against x.reshape(B, N, H, D).permute(0, 2, 3, 1), zero
    padded: integers, so torch.equal; the pad columns [N, pad) must read 0 on NaN-filled memory.  C = 48 and 16 leave a partial 32-channel tile."""
    from ap_adapter_amd import ops
    dtype = BC.MODES[mode]
    B = 2
    for N in (1, 31, 33, 97):
        for pad in (ops.round_up(N, 32), ops.round_up(N, 32) + 32):
            for H, d in ((1, 16), (3, 16), (2, 80)):
                xs = [int_operand(B, N, H * d, amp=100, seed=1000 * i + N + H).to(dev, dtype) for i in range(ntensors)]
                run = (lambda: [ops.head_transpose(xs[0], H, pad)]) if ntensors == 1 else (lambda: ops.head_transpose_many(xs, H, pad))
                outs = _warm_then_fill(dev, run)
                assert len(outs) == ntensors
                for x, y in zip(xs, outs):
                    want = torch.zeros(B, H, d, pad, dtype=dtype, device=dev)
                    want[..., :N] = x.reshape(B, N, H, d).permute(0, 2, 3, 1)
                    assert y.dtype == dtype and torch.equal(y, want) and not bool(torch.signbit(y[..., N:]).any()), (N, pad, H, d, mode)


def test_wrapper_refuses_what_the_kernels_cannot_hold(dev):
    """ops.attention_bwd: a dq= of another shape, dtype or stride, packed=True beside a dq=, an lse whose rows are not round_up(N, 32) long"""
    from ap_adapter_amd import ops
    B, N, L, H, d = 1, 33, 8, 2, 16
    C_ = H * d
    z = lambda *s, dt=torch.bfloat16: torch.zeros(*s, dtype=dt, device=dev)
    q, k, v, o, do = z(B, N, C_), z(B, L, C_), z(B, L, C_), z(B, N, C_), z(B, N, C_)
    lse = z(B, H, 64, dt=torch.float32)
    call = lambda **kw: ops.attention_bwd(q, k, v, o, do, kw.pop("lse", lse), H, **kw)
    for kw in (dict(dq=z(B, N + 1, C_)), dict(dq=z(B, N, C_, dt=torch.float16)), dict(dq=z(B, N, 2 * C_)[..., :C_]), dict(dq=z(B, C_, N).transpose(1, 2)),
               dict(lse=z(B, H, 33, dt=torch.float32)), dict(lse=z(B, H, 96, dt=torch.float32)), dict(lse=z(B, H, 64))):
        with pytest.raises(RuntimeError, match="attention_bwd"):
            call(**kw)
    q2, o2, do2, k2 = z(B, L, C_), z(B, L, C_), z(B, L, C_), z(B, L, C_)
    with pytest.raises(RuntimeError, match="packed"):
        ops.attention_bwd(q2, k2, v, o2, do2, z(B, H, 32, dt=torch.float32), H, dq=z(B, L, C_), packed=True)
    dq, dk, dv = call(dq=z(B, N, C_))  # (what is accepted still runs)
    assert tuple(dq.shape) == (B, N, C_) and tuple(dk.shape) == (B, L, C_)
