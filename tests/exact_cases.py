"""The case table of the integer-operand tests: tests/test_exact_operands_host.py builds every case's operands and fp64 reference on the CPU
and checks the conditions under which the expected bits are determined (util.assert_exact_conditions); tests/test_gpu_exact_linear.py runs
the same cases through the public ``ops`` wrappers and compares every bit.

A case is (family, arguments); ``build(case, tier, mode)`` returns its operands (fp32 CPU integers) and, per variant (bias only, + residual,
+ row-group bias ...), the fp64 values the kernel must store: ``out`` (what the final rounding sees), ``inter`` (accumulator and everything
a kernel may round on the way) and ``side`` (fp32 row statistics).  ``run(case, built, ops, dev, dtype)`` launches the variants.

The reference of a residual add is the one csrc/gemm_shared.h states -- rne(acc + bias + row-group bias), then rne(that + residual) -- which
in tier A (every value an integer of at most 256) is the plain sum."""
import functools
from collections import namedtuple

import torch
import torch.nn.functional as F

from util import exact_case, int_operand, rne

MODES = {"bf16": torch.bfloat16, "f16": torch.float16, "highest": torch.float32, "high": torch.float32}
M16 = ("bf16", "f16")
ALL = M16 + ("highest", "high")

Case = namedtuple("Case", "name family args modes tiers")
Built = namedtuple("Built", "K amp_x amp_w t variants")


def _side_amps(tier):
    """(bias / time-embedding rows, residual): tier A by the issue's rule; tier B large enough that the second rounding is a real one"""
    return (8, 16) if tier == "A" else (100, 100)


def _two_step(pre, res, dtype):
    return rne(pre, dtype).double() + res


def _stats(ref, dtype, width):
    """fp64 (sum, sum of squares) per ``width`` columns of the STORED rows"""
    s = rne(ref, dtype).double().reshape(ref.shape[0], -1, width)
    return torch.stack([s.sum(-1), (s * s).sum(-1)], -1)


def _seed(case, i):
    import zlib
    return (zlib.crc32(case.name.encode()) + 7919 * i) % (2 ** 31)


# ---------------------------------------------------------------- plain GEMM (tiled, ring, K groups, 128-tile, big tile)
def build_linear(case, tier, dtype):
    M, N, K = case.args["M"], case.args["N"], case.args["K"]
    ax, aw, dens = exact_case(K, dtype, tier)
    ab, ar = _side_amps(tier)
    rows = case.args.get("x_rows", M)  # the 128-tile case repeats a few random rows
    x = int_operand(rows, K, amp=ax, seed=_seed(case, 0))
    w = int_operand(N, K, amp=aw, seed=_seed(case, 1), density=dens)
    b = int_operand(N, amp=ab, seed=_seed(case, 2))
    Rm = case.args.get("res_mod", (M + 1) // 2)
    r = int_operand(Rm, N, amp=ar, seed=_seed(case, 3))
    rpg = (M + 1) // 2
    g2, g5 = int_operand(2, N, amp=ab, seed=_seed(case, 4)), int_operand(5, N, amp=ab, seed=_seed(case, 5))
    idx = torch.arange(M) % rows
    acc = F.linear(x.double(), w.double())[idx]
    pre = acc + b.double()
    v = {"bias": dict(out={"out": pre}, inter=[acc]),
         "residual_mod": dict(out={"out": _two_step(pre, r.double()[torch.arange(M) % Rm], dtype)}, inter=[acc, pre])}
    if tier == "A":
        pg = pre + g2.double()[torch.arange(M) // rpg]
        pt = pre + g5.double()[3]
        v["rg_group"] = dict(out={"out": pg}, inter=[acc])
        v["rg_table"] = dict(out={"out": pt}, inter=[acc])
    if case.args.get("rowstat"):
        full = int_operand(M, N, amp=ar, seed=_seed(case, 6))
        ref = _two_step(pre, full.double(), dtype)
        v = {"rowstat": dict(out={"out": ref}, inter=[acc, pre], side={"rowstat": _stats(ref, dtype, 64)})}
        r = full
    return Built(K, ax, aw, dict(x=x, w=w, b=b, r=r, g2=g2, g5=g5, idx=idx, rpg=rpg, Rm=Rm), v)


def run_linear(case, bt, ops, dev, dtype):
    D = lambda a: a.to(dev, dtype)
    t = bt.t
    x, w, b = D(t["x"])[t["idx"].to(dev)].contiguous(), D(t["w"]), D(t["b"])
    old = ops.set_gemm_ring(case.args.get("ring", 0))
    try:
        got = {}
        for name in bt.variants:
            if name == "bias":
                o = ops.linear(x, w, b)
            elif name == "residual_mod":
                o = ops.linear(x, w, b, residual=D(t["r"]), residual_row_mod=t["Rm"])
            elif name == "rg_group":
                o = ops.linear(x, w, b, rowgroup_bias=D(t["g2"]), rows_per_group=t["rpg"])
            elif name == "rg_table":
                step = torch.tensor([3], dtype=torch.int32, device=dev)
                o = ops.linear(x, w, b, rowgroup_bias=D(t["g5"]), rows_per_group=1 << 40, step_ptr=step)
            else:
                o = ops.linear(x, w, b, residual=D(t["r"]), rowstat=True)
                assert ops.rowstat_of(o) is not None
                got[name] = {"out": o, "rowstat": ops.rowstat_of(o)}
                continue
            got[name] = {"out": o}
        return got
    finally:
        ops.set_gemm_ring(old)


# ---------------------------------------------------------------- fp32-mode relu
def build_relu(case, tier, dtype):
    M, N, K = case.args["M"], case.args["N"], case.args["K"]
    ax, aw, dens = exact_case(K, dtype, tier)
    x, w = int_operand(M, K, amp=ax, seed=_seed(case, 0)), int_operand(N, K, amp=aw, seed=_seed(case, 1), density=dens)
    b = int_operand(N, amp=8, seed=_seed(case, 2))
    pre = F.linear(x.double(), w.double(), b.double())
    return Built(K, ax, aw, dict(x=x, w=w, b=b), {"relu": dict(out={"out": pre.clamp_min(0.0)}, inter=[pre - b.double(), pre])})


def run_relu(case, bt, ops, dev, dtype):
    D = lambda a: a.to(dev, dtype)
    return {"relu": {"out": ops.linear(D(bt.t["x"]), D(bt.t["w"]), D(bt.t["b"]), act="relu")}}


# ---------------------------------------------------------------- two-source GEMM (the second source's batch read modulo)
def build_linear2(case, tier, dtype):
    T, Ca, Cb, N = case.args["T"], case.args["Ca"], case.args["Cb"], case.args["N"]
    K = Ca + Cb
    ax, aw, dens = exact_case(K, dtype, tier)
    xa, xb = int_operand(2, T, Ca, amp=ax, seed=_seed(case, 0)), int_operand(1, T, Cb, amp=ax, seed=_seed(case, 1))
    w = int_operand(N, K, amp=aw, seed=_seed(case, 2), density=dens)
    b = int_operand(N, amp=_side_amps(tier)[0], seed=_seed(case, 3))
    acc = F.linear(torch.cat([xa, xb.expand(2, T, Cb)], -1).double(), w.double())
    return Built(K, ax, aw, dict(xa=xa, xb=xb, w=w, b=b), {"bias": dict(out={"out": acc + b.double()}, inter=[acc])})


def run_linear2(case, bt, ops, dev, dtype):
    D = lambda a: a.to(dev, dtype)
    old = ops.set_gemm_ring(case.args.get("ring", 0))
    try:
        return {"bias": {"out": ops.linear2(D(bt.t["xa"]), D(bt.t["xb"]), D(bt.t["w"]), D(bt.t["b"]))}}
    finally:
        ops.set_gemm_ring(old)


# ---------------------------------------------------------------- V^T and fused q | k | v outputs of the tiled kernel
QKV_GEOM = dict(B=2, L=35, heads=2, d=64, Lpad=40)


def _vt_ref(y, g):
    """[B*L, C] -> [B, heads, d, Lpad] with zero padding past L"""
    vt = torch.zeros(g["B"], g["heads"], g["d"], g["Lpad"], dtype=torch.float64)
    vt[..., :g["L"]] = y.reshape(g["B"], g["L"], g["heads"], g["d"]).permute(0, 2, 3, 1)
    return vt


def build_vt_qkv(case, tier, dtype):
    g, K = QKV_GEOM, case.args["K"]
    C, M = g["heads"] * g["d"], g["B"] * g["L"]
    ax, aw, dens = exact_case(K, dtype, tier)
    x = int_operand(M, K, amp=ax, seed=_seed(case, 0))
    w = int_operand(3 * C, K, amp=aw, seed=_seed(case, 1), density=dens)
    b = int_operand(3 * C, amp=8, seed=_seed(case, 2))
    acc = F.linear(x.double(), w.double())
    y = acc + b.double()
    qkv = {"q": y[:, :C], "k": y[:, C:2 * C], "vt": _vt_ref(y[:, 2 * C:], g)}
    v = {"vt": dict(out={"vt": _vt_ref(y[:, 2 * C:], g)}, inter=[acc]), "qkv": dict(out=dict(qkv), inter=[acc]),
         "qkv_v": dict(out=dict(qkv, v=y[:, 2 * C:]), inter=[acc])}
    return Built(K, ax, aw, dict(x=x, w=w, b=b), v)


def run_vt_qkv(case, bt, ops, dev, dtype):
    g = QKV_GEOM
    C, M = g["heads"] * g["d"], g["B"] * g["L"]
    D = lambda a: a.to(dev, dtype)
    x, w, b = D(bt.t["x"]), D(bt.t["w"]), D(bt.t["b"])
    zvt = lambda: torch.zeros(g["B"], g["heads"], g["d"], g["Lpad"], dtype=dtype, device=dev)
    old = ops.set_gemm_ring(case.args.get("ring", 0))
    try:
        got = {"vt": {"vt": ops.linear_vt(x, w[2 * C:], g["B"], g["L"], g["heads"], zvt(), bias=b[2 * C:])}}
        for name, with_v in (("qkv", False), ("qkv_v", True)):
            q, k = (torch.empty(M, C, dtype=dtype, device=dev) for _ in range(2))
            v = torch.empty(M, C, dtype=dtype, device=dev) if with_v else None
            vt = zvt()
            if with_v and dtype not in ops.FUSED_DTYPES:  # the fp32 kernels have no row-major v output: the wrapper must say so
                try:
                    ops.linear_qkv(x, w, g["B"], g["L"], g["heads"], q, k, vt, bias=b, v=v)
                except RuntimeError:
                    got[name] = None
                    continue
                raise AssertionError("linear_qkv(v=...) in an fp32 mode neither wrote v nor raised")
            ops.linear_qkv(x, w, g["B"], g["L"], g["heads"], q, k, vt, bias=b, v=v)
            got[name] = dict(q=q, k=k, vt=vt, **({"v": v} if with_v else {}))
        return got
    finally:
        ops.set_gemm_ring(old)


# ---------------------------------------------------------------- 3x3 convolution
def build_conv(case, tier, dtype):
    a = case.args
    B, H, W, Cin, Cout = a["B"], a["H"], a["W"], a["Cin"], a["Cout"]
    stride, up, asym, sbm = a.get("stride", 1), a.get("up"), a.get("asym_pad", False), a.get("src_batch_mod", 0)
    K = 9 * Cin
    ax, aw, dens = exact_case(K, dtype, tier)
    ab, ar = _side_amps(tier)
    Bs = sbm or B
    x = int_operand(Bs, Cin, H, W, amp=ax, seed=_seed(case, 0))
    w = int_operand(Cout, Cin, 3, 3, amp=aw, seed=_seed(case, 1), density=dens)
    b = int_operand(Cout, amp=ab, seed=_seed(case, 2))
    sample = a.get("temb") == "sample"  # one time-embedding row per sample (rows_per_group = Hout * Wout) instead of table row *step_ptr
    tt = int_operand(B if sample else 4, Cout, amp=ab, seed=_seed(case, 3))
    src = x.double()[torch.arange(B) % Bs]
    if up is not None:
        src = F.interpolate(src, size=up, mode="nearest")
    if asym:
        acc = F.conv2d(F.pad(src, (0, 1, 0, 1)), w.double(), None, stride=stride, padding=0)
    else:
        acc = F.conv2d(src, w.double(), None, stride=stride, padding=1)
    Ho, Wo = acc.shape[2:]
    r = int_operand(B, Cout, Ho, Wo, amp=ar, seed=_seed(case, 4))
    rows = lambda y: y.permute(0, 2, 3, 1).reshape(B, Ho * Wo, Cout)
    bias = acc + b.double()[None, :, None, None]
    v = {"bias": dict(out={"out": rows(bias)}, inter=[acc])}
    if not a.get("narrow"):  # (the narrow halo form takes no residual / row-group bias)
        pre = bias + (tt.double()[:, :, None, None] if sample else tt.double()[2][None, :, None, None])
        v["temb_residual"] = dict(out={"out": rows(_two_step(pre, r.double(), dtype))}, inter=[acc, bias, pre])
    return Built(K, ax, aw, dict(x=x, w=w, b=b, tt=tt, r=r, Ho=Ho, Wo=Wo), v)


def run_conv(case, bt, ops, dev, dtype):
    a, t = case.args, bt.t
    B, H, W = a["B"], a["H"], a["W"]
    D = lambda y: y.to(dev, dtype)
    nhwc = lambda y: D(y.permute(0, 2, 3, 1).reshape(y.shape[0], y.shape[2] * y.shape[3], -1).contiguous())
    wp = ops.conv3x3_pack(D(t["w"]))
    kw = dict(stride=a.get("stride", 1), up=a.get("up"), asym_pad=a.get("asym_pad", False), src_batch_mod=a.get("src_batch_mod", 0))
    old, ops.HCONV = ops.HCONV, bool(a.get("hconv", False))
    try:
        got = {}
        for name in bt.variants:
            if name == "bias":
                o, Ho, Wo = ops.conv3x3(nhwc(t["x"]), wp, D(t["b"]), B, H, W, **kw)
            else:
                sample = a.get("temb") == "sample"
                step = torch.tensor([0 if sample else 2], dtype=torch.int32, device=dev)
                o, Ho, Wo = ops.conv3x3(nhwc(t["x"]), wp, D(t["b"]), B, H, W, residual=nhwc(t["r"]), rowgroup_bias=D(t["tt"]),
                                        rows_per_group=(t["Ho"] * t["Wo"] if sample else 1 << 40), step_ptr=step, **kw)
            assert (Ho, Wo) == (t["Ho"], t["Wo"])
            got[name] = {"out": o}
        return got
    finally:
        ops.HCONV = old


# ---------------------------------------------------------------- 1-D convolutions (the vocoder's)
def build_conv1d(case, tier, dtype):
    a = case.args
    B, T, Cin, Cout, taps, dil, ts, slope = a["B"], a["T"], a["Cin"], a["Cout"], a["taps"], a.get("dil", 1), a.get("ts", 0), a.get("slope")
    K = taps * Cin
    ax, aw, dens = exact_case(K, dtype, tier)
    x = int_operand(B, T, Cin, amp=ax, seed=_seed(case, 0))
    if slope is not None:  # even values: a power-of-two slope keeps leaky-ReLU exact
        x = 2.0 * int_operand(B, T, Cin, amp=1, seed=_seed(case, 0))
    wp = int_operand(Cout, K, amp=aw, seed=_seed(case, 1), density=dens)
    b = int_operand(Cout, amp=8, seed=_seed(case, 2))
    xin = x.double().permute(0, 2, 1)
    if slope is not None:
        xin = F.leaky_relu(xin, slope)
    w3 = wp.double().reshape(Cout, taps, Cin)
    if ts:
        acc = F.conv_transpose1d(xin, w3.permute(2, 0, 1).contiguous(), None, stride=ts, padding=(taps - ts) // 2)
    else:
        acc = F.conv1d(xin, w3.permute(0, 2, 1).contiguous(), None, dilation=dil, padding=(taps * dil - dil) // 2)
    acc = acc.permute(0, 2, 1).contiguous()  # [B, Tout, Cout]
    r = int_operand(*acc.shape, amp=16, seed=_seed(case, 3))
    pre = acc + b.double()
    v = {"bias": dict(out={"out": pre}, inter=[acc, xin]), "residual": dict(out={"out": _two_step(pre, r.double(), dtype)}, inter=[acc, pre])}
    return Built(K, max(ax, 2), aw, dict(x=x, wp=wp, b=b, r=r), v)


def run_conv1d(case, bt, ops, dev, dtype):
    a, t = case.args, bt.t
    D = lambda y: y.to(dev, dtype)
    kw = dict(dilation=a.get("dil", 1), transposed_stride=a.get("ts", 0), pre_slope=a.get("slope"))
    return {"bias": {"out": ops.conv1d(D(t["x"]), D(t["wp"]), D(t["b"]), a["taps"], **kw)},
            "residual": {"out": ops.conv1d(D(t["x"]), D(t["wp"]), D(t["b"]), a["taps"], residual=D(t["r"]), **kw)}}


# ---------------------------------------------------------------- patch embedding from fp32 mel patches
def build_patch(case, tier, dtype):
    B, H, W, N = 2, 16, 32, case.args["N"]
    ax, aw, dens = exact_case(256, dtype, tier)
    mel = int_operand(B, H, W, amp=ax, seed=_seed(case, 0))
    w = int_operand(N, 256, amp=aw, seed=_seed(case, 1), density=dens)
    b = int_operand(N, amp=8, seed=_seed(case, 2))
    patches = mel.double().reshape(B, H // 16, 16, W // 16, 16).permute(0, 1, 3, 2, 4).reshape(B, -1, 256)
    acc = F.linear(patches, w.double())
    return Built(256, ax, aw, dict(mel=mel, w=w, b=b), {"bias": dict(out={"out": acc + b.double()}, inter=[acc])})


def run_patch(case, bt, ops, dev, dtype):
    t = bt.t
    return {"bias": {"out": ops.patch_embed(t["mel"].to(dev), t["w"].to(dev, dtype), t["b"].to(dev, dtype), dtype)}}


# ---------------------------------------------------------------- row-panel / weight-stationary projections without LayerNorm
def build_fused(case, tier, dtype):
    M, N, K = case.args["M"], case.args["N"], case.args["K"]
    ax, aw, dens = exact_case(K, dtype, tier)
    ab, ar = _side_amps(tier)
    x, w = int_operand(M, K, amp=ax, seed=_seed(case, 0)), int_operand(N, K, amp=aw, seed=_seed(case, 1), density=dens)
    b, r = int_operand(N, amp=ab, seed=_seed(case, 2)), int_operand(M, N, amp=ar, seed=_seed(case, 3))
    acc = F.linear(x.double(), w.double())
    pre = acc + b.double()
    v = {"bias": dict(out={"out": pre}, inter=[acc])}
    if tier == "A":
        v["residual"] = dict(out={"out": pre + r.double()}, inter=[acc, pre])
    return Built(K, ax, aw, dict(x=x, w=w, b=b, r=r), v)


def run_fused(case, bt, ops, dev, dtype):
    D = lambda a: a.to(dev, dtype)
    t = bt.t
    assert ops.rp_ok(D(t["x"])) and case.args["N"] % 64 == 0  # fused_linear's own condition for the row-panel launch
    got = {"bias": {"out": ops.fused_linear(D(t["x"]), D(t["w"]), D(t["b"]), ln=None)}}
    if "residual" in bt.variants:
        got["residual"] = {"out": ops.fused_linear(D(t["x"]), D(t["w"]), D(t["b"]), ln=None, residual=D(t["r"]))}
    return got


def build_rp3(case, tier, dtype):
    g, K = QKV_GEOM, case.args["K"]
    C, M = g["heads"] * g["d"], g["B"] * g["L"]
    ax, aw, dens = exact_case(K, dtype, tier)
    x = int_operand(M, K, amp=ax, seed=_seed(case, 0))
    w = int_operand(3 * C, K, amp=aw, seed=_seed(case, 1), density=dens)
    b = int_operand(3 * C, amp=8, seed=_seed(case, 2))
    acc = F.linear(x.double(), w.double())
    y = acc + b.double()
    return Built(K, ax, aw, dict(x=x, w=w, b=b), {"qkv": dict(out={"q": y[:, :C], "k": y[:, C:2 * C], "vt": _vt_ref(y[:, 2 * C:], g)}, inter=[acc])})


def run_rp3(case, bt, ops, dev, dtype):
    g = QKV_GEOM
    C, M = g["heads"] * g["d"], g["B"] * g["L"]
    D = lambda a: a.to(dev, dtype)
    b = D(bt.t["b"])
    q, k = (torch.empty(M, C, dtype=dtype, device=dev) for _ in range(2))
    vt = torch.zeros(g["B"], g["heads"], g["d"], g["Lpad"], dtype=dtype, device=dev)
    ops.rowpanel(D(bt.t["x"]), D(bt.t["w"]), [(q, b[:C], C, "row"), (k, b[C:2 * C], C, "row"), (vt, b[2 * C:], C, "vt")],
                 vt_geom=(g["heads"], g["d"], g["L"], g["Lpad"]))
    return {"qkv": dict(q=q, k=k, vt=vt)}


# ---------------------------------------------------------------- the 64-token level's to_out / FF2 kernels
def build_hs(case, tier, dtype):
    B, N, K = case.args["B"], case.args["N"], case.args["K"]
    ax, aw, dens = exact_case(K, dtype, tier)
    ab, ar = _side_amps(tier)
    o = int_operand(B, N, K, amp=ax, seed=_seed(case, 0))
    w = int_operand(640, K, amp=aw, seed=_seed(case, 1), density=dens)
    b, r = int_operand(640, amp=ab, seed=_seed(case, 2)), int_operand(B, N, 640, amp=ar, seed=_seed(case, 3))
    acc = F.linear(o.double(), w.double())
    pre = acc + b.double()
    ref = _two_step(pre, r.double(), dtype)
    v = {"bias": dict(out={"out": pre}, inter=[acc]), "residual": dict(out={"out": ref}, inter=[acc, pre])}
    if tier == "A":
        v["residual"]["side"] = {"rowstat": _stats(ref.reshape(B * N, 640), dtype, 32)}
    return Built(K, ax, aw, dict(o=o, w=w, b=b, r=r), v)


def run_hs(case, bt, ops, dev, dtype):
    D = lambda a: a.to(dev, dtype)
    t = bt.t
    if case.args["K"] == 640:
        fn, wp = ops.hs_out, ops.hs_pack_rows(D(t["w"]))[0]
    else:
        fn, wp = ops.hs_ff2, ops.hs_pack_ff2(D(t["w"]))
    got = {"bias": {"out": fn(D(t["o"]), wp, D(t["b"]), None)}}
    stat = "side" in bt.variants["residual"]
    o = fn(D(t["o"]), wp, D(t["b"]), D(t["r"]), rowstat=stat)
    got["residual"] = {"out": o}
    if stat:
        got["residual"]["rowstat"] = ops.rowstat_of(o)
    return got


# ---------------------------------------------------------------- weight gradients (reduction over the token rows)
def build_wgrad(case, tier, dtype):
    M, N, K = case.args["M"], 72, 40
    ax, aw, dens = exact_case(M, dtype, tier)
    dy, x = int_operand(M, N, amp=ax, seed=_seed(case, 0)), int_operand(M, K, amp=aw, seed=_seed(case, 1), density=dens)
    a0 = int_operand(N, K, amp=16, seed=_seed(case, 2))
    dw = dy.double().t() @ x.double()
    v = {"plain": dict(out={"out": dw}, inter=[]), "fp32": dict(out={}, inter=[dw], side={"out": dw}),
         "acc_twice": dict(out={}, inter=[dw, a0.double() + dw], side={"out": a0.double() + 2.0 * dw})}
    return Built(M, ax, aw, dict(dy=dy, x=x, a0=a0), v)


def run_wgrad(case, bt, ops, dev, dtype):
    D = lambda a: a.to(dev, dtype)
    dy, x = D(bt.t["dy"]), D(bt.t["x"])
    acc = bt.t["a0"].to(dev).contiguous()
    assert ops.weight_grad(dy, x, fp32=True, acc=acc) is None and ops.weight_grad(dy, x, fp32=True, acc=acc) is None
    return {"plain": {"out": ops.weight_grad(dy, x)}, "fp32": {"out": ops.weight_grad(dy, x, fp32=True)}, "acc_twice": {"out": acc}}


FAMILIES = {"linear": (build_linear, run_linear), "relu": (build_relu, run_relu), "linear2": (build_linear2, run_linear2),
            "vt_qkv": (build_vt_qkv, run_vt_qkv), "conv": (build_conv, run_conv), "conv1d": (build_conv1d, run_conv1d),
            "patch": (build_patch, run_patch), "fused": (build_fused, run_fused), "rp3": (build_rp3, run_rp3), "hs": (build_hs, run_hs),
            "wgrad": (build_wgrad, run_wgrad)}


def _c(name, family, modes=ALL, tiers="A", **args):
    return Case(name, family, args, modes, tiers)


# ring: ops.set_gemm_ring(2); hconv: ops.HCONV.  The shape conditions that route each case are asserted in test_gpu_exact_linear.py.
CASES = [
    # the two controls come first: the fp32 "highest" fmaf chain, then the 64-tile 16-bit kernel, at (77, 8, 72)
    _c("gemm_77x8x72", "linear", tiers="AB", M=77, N=8, K=72),
    _c("gemm_130x72x136", "linear", tiers="AB", M=130, N=72, K=136),
    _c("gemm_kgroup_70x640x384", "linear", tiers="AB", M=70, N=640, K=384),
    _c("gemm_513x640x2560", "linear", tiers="AB", M=513, N=640, K=2560),
    _c("gemm_tile128_40900x24x1024", "linear", tiers="AB", M=40900, N=24, K=1024, x_rows=257, res_mod=257),
    _c("gemm_rowstat_70x128x72", "linear", M16, M=70, N=128, K=72, rowstat=True),
    _c("ring_70x128x128", "linear", M16, tiers="AB", M=70, N=128, K=128, ring=2),
    _c("ring_kgroup_70x640x384", "linear", M16, M=70, N=640, K=384, ring=2),
    _c("ring_rowstat_70x128x128", "linear", M16, M=70, N=128, K=128, ring=2, rowstat=True),
    _c("big_256x128_16001x128x192", "linear", M16, tiers="AB", M=16001, N=128, K=192),
    _c("big_256x256_16385x256x64", "linear", M16, M=16385, N=256, K=64),
    _c("relu_37x36x36", "relu", ("highest", "high"), M=37, N=36, K=36),
    _c("linear2_tiled", "linear2", M16, T=35, Ca=64, Cb=72, N=72),  # (the fp32 kernels have no two-source operand)
    _c("linear2_ring", "linear2", M16, T=35, Ca=64, Cb=64, N=128, ring=2),
    _c("linear2_big", "linear2", M16, T=8001, Ca=64, Cb=64, N=128),
    _c("vt_qkv_k72", "vt_qkv", K=72),
    _c("vt_qkv_ring_k128", "vt_qkv", M16, K=128, ring=2),
    # 3x3 convolutions: the tiled form at the c_conv_* shapes of tests/golden/make_gemm_bits.py
    _c("conv_two_stage", "conv", B=2, H=4, W=4, Cin=256, Cout=72),
    _c("conv_s2", "conv", B=2, H=7, W=5, Cin=8, Cout=72, stride=2),
    _c("conv_up_odd", "conv", B=2, H=4, W=3, Cin=8, Cout=72, up=(9, 7)),
    _c("conv_asym", "conv", B=2, H=8, W=6, Cin=8, Cout=72, stride=2, asym_pad=True),
    _c("conv_fast", "conv", tiers="AB", B=2, H=7, W=5, Cin=64, Cout=72),
    _c("conv_fast_shared_src", "conv", B=2, H=7, W=5, Cin=64, Cout=72, src_batch_mod=1),
    _c("conv_small_ring_640", "conv", M16, tiers="AB", B=2, H=32, W=2, Cin=640, Cout=640),
    _c("conv_small_ring_1280", "conv", M16, B=2, H=32, W=2, Cin=1280, Cout=640),
    _c("conv_small_ring_s2", "conv", M16, B=2, H=8, W=4, Cin=256, Cout=64, stride=2),  # the ring's per-row source offsets (stride 2)
    _c("conv_halo_up_odd", "conv", M16, B=2, H=3, W=2, Cin=64, Cout=128, up=(5, 4), hconv=True),  # nearest up-sampling in the halo fill
    _c("conv_halo_kslices_640", "conv", M16, B=2, H=32, W=2, Cin=640, Cout=640, hconv=True),
    _c("conv_halo_kslices_1280", "conv", M16, B=2, H=32, W=2, Cin=1280, Cout=640, hconv=True),
    _c("conv_halo_5x4", "conv", M16, B=1, H=5, W=4, Cin=64, Cout=128, hconv=True),
    _c("conv_halo_32x2", "conv", M16, tiers="AB", B=2, H=32, W=2, Cin=128, Cout=128, hconv=True),
    _c("conv_halo_narrow", "conv", M16, B=5, H=63, W=4, Cin=64, Cout=16, hconv=True, narrow=True),
    _c("conv_big_tile", "conv", M16, tiers="AB", B=1, H=1001, W=16, Cin=64, Cout=128),
    _c("conv_big_tile_s2", "conv", M16, B=1, H=2001, W=32, Cin=64, Cout=128, stride=2),  # the big tile's per-row source offsets
    _c("conv_halo_sample_temb", "conv", M16, B=3, H=5, W=4, Cin=64, Cout=128, hconv=True, temb="sample"),
    _c("conv_tiled_sample_temb", "conv", B=3, H=5, W=4, Cin=8, Cout=72, temb="sample"),
    _c("conv_big_tile_on_halo", "conv", M16, B=1, H=1001, W=16, Cin=64, Cout=128, hconv=True),
    # 1-D convolutions
    _c("conv1d_k3_d1", "conv1d", B=2, T=37, Cin=16, Cout=24, taps=3, dil=1),
    _c("conv1d_k7_d3", "conv1d", B=2, T=37, Cin=16, Cout=24, taps=7, dil=3),
    _c("conv1d_k11_d5", "conv1d", B=2, T=37, Cin=16, Cout=24, taps=11, dil=5),
    _c("conv1d_k3_d3_slope", "conv1d", B=2, T=37, Cin=16, Cout=24, taps=3, dil=3, slope=0.5),
    _c("conv1d_tr_16_5", "conv1d", B=2, T=19, Cin=16, Cout=24, taps=16, ts=5),
    _c("conv1d_tr_4_2", "conv1d", B=2, T=19, Cin=16, Cout=24, taps=4, ts=2),
    _c("conv1d_tr_8_2_slope", "conv1d", B=2, T=19, Cin=16, Cout=24, taps=8, ts=2, slope=0.5),
    _c("patch_embed", "patch", N=72),
    # row-panel launches without LayerNorm (16-bit only): N % (256 at K = 256 | 128 at K = 384) == 0 is the weight-stationary kernel (wsgemm),
    # every other N the streamed row-panel kernel (rpgemm), whose 8-wave form starts at 32768 rows
    _c("ws_k256_m17", "fused", M16, M=17, N=256, K=256),
    _c("ws_k256_m257", "fused", M16, tiers="AB", M=257, N=256, K=256),
    _c("ws_k384_m257", "fused", M16, M=257, N=384, K=384),
    _c("rp_k256_m17", "fused", M16, M=17, N=64, K=256),
    _c("rp_k256_m257", "fused", M16, tiers="AB", M=257, N=64, K=256),
    _c("rp_k384_m257", "fused", M16, M=257, N=64, K=384),
    _c("rp_k256_8wave", "fused", M16, M=32768, N=64, K=256),
    _c("rp_k384_8wave", "fused", M16, M=32768, N=64, K=384),
    _c("rp3_k256", "rp3", M16, K=256),
    _c("rp3_k384", "rp3", M16, K=384),
    _c("hs_out_2x64", "hs", M16, B=2, N=64, K=640),
    _c("hs_out_3x16", "hs", M16, tiers="AB", B=3, N=16, K=640),
    _c("hs_out_1x1", "hs", M16, B=1, N=1, K=640),
    _c("hs_ff2_2x64", "hs", M16, B=2, N=64, K=2560),
    _c("hs_ff2_3x16", "hs", M16, tiers="AB", B=3, N=16, K=2560),
    _c("hs_ff2_1x1", "hs", M16, B=1, N=1, K=2560),
    _c("wgrad_m32", "wgrad", M16, M=32),
    _c("wgrad_m132", "wgrad", M16, M=132),
    _c("wgrad_m2048", "wgrad", M16, M=2048),
]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def params():
    """(case name, tier, mode), the modes of a case together so that build()'s cache serves them"""
    out = []
    for c in CASES:
        for tier in c.tiers:
            for mode in c.modes:
                if tier == "B" and mode not in M16:
                    continue
                out.append((c.name, tier, mode))
    return out


@functools.lru_cache(maxsize=3)
def _build(name, tier, dtype):
    return FAMILIES[BY_NAME[name].family][0](BY_NAME[name], tier, dtype)


def build(name, tier, mode):
    """tier A operands and references do not depend on the storage type: one build serves the four modes"""
    return _build(name, tier, torch.bfloat16 if tier == "A" else MODES[mode])


def run(name, built, ops, dev, mode):
    old = ops.get_float32_matmul_precision()
    try:
        if mode in ("highest", "high"):
            ops.set_float32_matmul_precision(mode)
        return FAMILIES[BY_NAME[name].family][1](BY_NAME[name], built, ops, dev, MODES[mode])
    finally:
        ops.set_float32_matmul_precision(old)
