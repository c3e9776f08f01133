"""The case table of the exact attention-backward tests: tests/test_attn_bwd_exact_host.py builds every case's operands and fp64 reference on the CPU
and checks the conditions under which the expected gradients are determined; tests/test_gpu_exact_attention_bwd.py runs the same cases through
``ops.attention_bwd``, ``ops.attention_lse`` and the autograd entry points.

A softmax backward is exact where the forward is.  The operands follow the selection codes of tests/attn_exact_cases.py, but g = 2^k keys share one
code: a query of group c gives weight 2^-k to each key of its group and exactly 0 to every other key.  Per (sample, head), dims 0..15 are code dims
and dims 16..d free dims:
  keys     group c owns an 8-of-16 code set S_c (distinct within the (sample, head)); key j of group c has k = -a_jd on S_c, a_jd in {1, 2, 3}, and 0
           on the other code dims; the members of a group are scattered over the key tiles by a seeded permutation.  Keys left over when L is not
           groups * 2^k are "orphans": a code of their own that no query carries (weight 0 from every query, dK = dV = 0).
  queries  a query of group c has q = Q0 = 1024 on the code dims outside S_c and 0 inside: its group's keys score exactly 0, every other key at most
           -Q0.
  free     on the first half of the free dims K holds integers in [-3, 3] and Q is 0, on the second half Q holds integers and K is 0: the scores
           are untouched, dQ and dK are non-zero on code dims and free dims alike.
  V        an integer c_group,d in [-4, 4] plus deviations in [-3, 3] that cancel in +- pairs inside the group: O = c_group, an integer.
  dO       integers in [-2, 2] at density 1/4.
  masked   a "decoy" is the twin of a group key (the same key row, other values) with key_bias = -10000: it must receive dK = dV = 0 in every bit.
With these every quantity the kernels form -- delta, dP, dS = 2^-k s dO.(V_j - c), the three sums -- is a dyadic number that fp32 holds exactly in
any order, provided exp2(-k) is exactly 2^-k (the GPU file's two controls measure that).  k = 0 is plain selection: dV = the scatter of dO and
dQ = dK = 0, which holds only if delta equals dO.V[sel] to the last bit.

The reference is the plain fp64 backward with P given as the 0 / 2^-k matrix (never autograd's result rounded: its non-group weights are 1e-100,
not 0, and an orphan key would then get -0.0):
  delta = s sum dO o O,  dS = P o (s dO V^T - delta),  Aq = dS K,  Ak = dS^T Q,  Av = P^T dO
and the expected bits are read off the kernels (csrc/attention_bwd.hip store_row; scale32 = float32(1 / sqrt(d)) as ops.attention_bwd passes it):
  16-bit   dq = rne_T(fl32(Aq scale32)),  dk = rne_T(fl32(Ak scale32)),  dv = rne_T(Av s);  with dq= given: rne_T(fl32(fl32(Aq scale32) + dq0)).
  fp32     csrc/f32_ops.hip multiplies the scale into every ds before the sum: the same values without rne_T where the scale is a power of two
           (d = 16, 64; dv at every d, its factor is dout_scale).  At the other d each ds is rounded once, so dq and dk are held to
           |out - ref| <= c 2^-24 A with A = scale32 sum_j |dS_ij K_jd| (+ |dq0|) and c = F32_COEFF(M) = ceil(M / 64) + 9, counted on the kernel's
           order for a sum over M terms: 1 for the rounding of ds * scale, ceil(M / 64) for a lane's FMA chain (each rounds a partial sum that is
           at most A), 6 for the wave's butterfly adds, 1 for the store (the add of the old dq), 1 for the second-order terms.  The host test runs an
           fp32 emulation in that order against it.

Variants of a case (``run``): "plain" (exact out and lse; the lse pad entries [N, round_up(N, 32)) are NaN: "the padded tail of the stats arrays is
never trusted"), "nodkv" (need_dkv=False: the same dq bits), "packed" (N == L, 16-bit: views of one [B, N, 3C] buffer, the same bits),
"acc_int" / "acc_round" (dq= prefilled with small integers / with integers at the top of the storage type's exact range, so that the sum rounds),
"chained" (out and lse from ops.attention_lse) and, for the IP pair, the step's order: the text segment, then the audio segment with s = 0.5
accumulating into the text segment's dq."""
import functools
import math
from collections import namedtuple

import torch

from attn_exact_cases import MASK_BIAS, _all_codes, _seed
from util import int_operand, rne

MODES = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}
ALL = ("bf16", "f16", "f32")
Q0 = 1024.0
MANT = {torch.bfloat16: 8, torch.float16: 11, torch.float32: 24}  # significant bits

Case = namedtuple("Case", "name args modes")
# one softmax segment: k, v [B, L, H, d] fp32; bias [B, L] or None; grp [B, H, L] (group of a key, -1 orphan, -2 decoy); P [B, H, N, L] fp64;
# O [B, N, H, d] fp64; kexp: the k of 2^-k; s: dout_scale
Seg = namedtuple("Seg", "k v bias grp P O kexp s")
Ops = namedtuple("Ops", "q do segs qgrp codes")
# an expectation: ``bits`` (a tensor of the storage type) or, where the fp32 scale is no power of two, the bound |out - ref| <= c 2^-24 A
Exp = namedtuple("Exp", "bits ref A c")
Built = namedtuple("Built", "ops out lse exp dq0 refs")


def F32_COEFF(M):
    return (M + 63) // 64 + 9


def _fl32(t):
    return t.float().double()


def scale32(d):
    return float(torch.tensor(1.0 / math.sqrt(d), dtype=torch.float32))


def pow2_scale(d):
    return math.frexp(scale32(d))[0] == 0.5


def spread_codes(count, gen, keep=None):
    """[count, 16] 0 / 1: 8-of-16 sets drawn in a seeded order (the table of attn_exact_cases.code_sets), a set taken only if it shares at most 6 dims
    with every set taken before and with ``keep``: two keys of different groups then differ on two code dims at least, so a foreign key scores at
    most -2 Q0 -- at d = 128 one dim (-1024 / sqrt(128) log2(e) = -131) would leave a denormal weight"""
    allc = _all_codes()
    n0 = 0 if keep is None else keep.shape[0]
    got = torch.zeros(n0 + count, 16)
    if n0:
        got[:n0] = keep
    n = n0
    for i in torch.randperm(allc.shape[0], generator=gen).tolist():
        if n == n0 + count:
            break
        if n == 0 or float((got[:n] @ allc[i]).max()) <= 6:
            got[n] = allc[i]
            n += 1
    assert n == n0 + count, "the code table ran out"
    return got[n0:]


def decoy_positions(mode, L):
    if mode is None:
        return []
    if mode == "edges":  # key 0 and key L - 1 (a one-key last tile where L % 32 == 1)
        return sorted({0, L - 1})
    assert mode == "tile0" and L > 64  # the whole first 32-key tile, and the last key
    return list(range(32)) + [L - 1]


def _segment(name, si, B, H, L, d, k, G, dec_mode, unmasked, s, given_codes=None):
    """-> (Seg without P / O, codes [B, H, Gmax, 16], Gs [B]): the keys, values and bias of one segment"""
    g = 1 << k
    gen = torch.Generator().manual_seed(_seed(name, 16 * si))
    K, V = torch.zeros(B, L, H, d), torch.zeros(B, L, H, d)
    grp = torch.full((B, H, L), -1, dtype=torch.long)
    bias = torch.zeros(B, L) if dec_mode else None
    cgen = torch.Generator().manual_seed(_seed(name, 16 * si + 1))
    Gmax = G if G else max(1, L // g)
    codes = torch.zeros(B, H, Gmax, 16)
    cval = torch.zeros(B, H, Gmax, d)
    Gs = []
    nf = d - 16
    for b in range(B):
        dec = [] if b == unmasked else decoy_positions(dec_mode, L)
        real = [j for j in range(L) if j not in dec]
        Gb = G if G else len(real) // g
        assert 1 <= Gb <= Gmax and Gb * g <= len(real), (name, Gb, g, len(real))
        Gs.append(Gb)
        if bias is not None:
            bias[b, dec] = MASK_BIAS
        for h in range(H):
            perm = torch.randperm(len(real), generator=gen).tolist()
            slots = [real[p] for p in perm]
            members, orphans = slots[:Gb * g], slots[Gb * g:]
            if given_codes is None:
                pool = spread_codes(Gb + len(orphans), cgen)
                gc, oc = pool[:Gb], pool[Gb:]
            else:  # the IP pair's second segment: the queries already carry the first segment's sets
                gc = given_codes[b, h, :Gb]
                oc = spread_codes(len(orphans), cgen, keep=gc)
            codes[b, h, :Gb] = gc
            cval[b, h, :Gb] = torch.randint(-4, 5, (Gb, d), generator=gen).float()
            for r, j in enumerate(members):
                c = r // g
                grp[b, h, j] = c
                K[b, j, h, :16] = -gc[c] * torch.randint(1, 4, (16,), generator=gen).float()
                if r % 2 == 0:  # deviations cancel in +- pairs (a group of one key: none)
                    dev = torch.randint(-3, 4, (d,), generator=gen).float() if g > 1 else torch.zeros(d)
                V[b, j, h] = cval[b, h, c] + (dev if r % 2 == 0 else -dev)
            for r, j in enumerate(orphans):
                K[b, j, h, :16] = -oc[r] * torch.randint(1, 4, (16,), generator=gen).float()
                V[b, j, h] = torch.randint(-7, 8, (d,), generator=gen).float()
            if nf:
                K[b, :, h, 16:16 + nf // 2] = torch.randint(-3, 4, (L, nf // 2), generator=gen).float()
            for j in dec:  # the twin: the group key nearest to the decoy (tile0: to its place in the next tile)
                target = j + 32 if (dec_mode == "tile0" and j < 32) else j
                twin = min(members, key=lambda m: (abs(m - target), m))
                grp[b, h, j] = -2
                K[b, j, h] = K[b, twin, h]
                V[b, j, h] = torch.randint(-7, 8, (d,), generator=gen).float()
    return Seg(K, V, bias, grp, None, cval, k, s), codes, Gs


@functools.lru_cache(maxsize=4)
def operands(name):
    """the operands of a case (the same in every mode) with the exact P and O of every segment"""
    a = BY_NAME[name].args
    B, H, N, L, d, k = a["B"], a["H"], a["N"], a["L"], a["d"], a["k"]
    seg1, codes, Gs = _segment(name, 0, B, H, L, d, k, a.get("G"), a.get("bias"), a.get("unmasked"), a.get("s", 1.0))
    segs = [seg1]
    if "L2" in a:
        seg2, _, Gs2 = _segment(name, 1, B, H, a["L2"], d, a["k2"], a["G"], None, None, a["s2"], given_codes=codes)
        assert Gs2 == Gs
        segs.append(seg2)
    gen = torch.Generator().manual_seed(_seed(name, 8))
    qgrp = torch.empty(B, H, N, dtype=torch.long)
    for b in range(B):
        for h in range(H):
            qgrp[b, h] = (torch.arange(N) + 3 * (b * H + h)) % Gs[b]
    q = torch.zeros(B, N, H, d)
    bb, hh = torch.arange(B)[:, None, None].expand(B, H, N), torch.arange(H)[None, :, None].expand(B, H, N)
    q[..., :16] = (Q0 * (1.0 - codes[bb, hh, qgrp])).permute(0, 2, 1, 3)
    nf = d - 16
    if nf:
        q[..., 16 + nf // 2:] = torch.randint(-3, 4, (B, N, H, nf - nf // 2), generator=gen).float()
    do = int_operand(B, N, H, d, amp=2, seed=_seed(name, 9), density=0.25)
    full = []
    for sg in segs:
        P = (sg.grp[:, :, None, :] == qgrp[:, :, :, None]).double() * 2.0 ** -sg.kexp  # (grp -1 / -2 match no query)
        O = sg.O[bb, hh, qgrp].permute(0, 2, 1, 3).double()  # c_group of the query's group
        full.append(sg._replace(P=P, O=O))
    return Ops(q, do, full, qgrp, codes)


def backward64(q, do, sg, s=None):
    """the plain fp64 backward of one segment with P given: -> dict(delta, dS, Aq, Ak, Av, absq, absk); Aq / Ak carry no softmax scale"""
    s = sg.s if s is None else s
    q64, do64, k64, v64 = q.double(), do.double(), sg.k.double(), sg.v.double()
    delta = s * (do64 * sg.O).sum(-1).permute(0, 2, 1)  # [B, H, N]
    dP = s * torch.einsum("bnhd,blhd->bhnl", do64, v64)
    dS = sg.P * (dP - delta[..., None])
    return dict(delta=delta, dS=dS, Aq=torch.einsum("bhnl,blhd->bnhd", dS, k64), Ak=torch.einsum("bhnl,bnhd->blhd", dS, q64),
                Av=torch.einsum("bhnl,bnhd->blhd", sg.P, do64), absq=torch.einsum("bhnl,blhd->bnhd", dS.abs(), k64.abs()),
                absk=torch.einsum("bhnl,bnhd->blhd", dS.abs(), q64.abs()))


def dq0_operand(name, kind, dtype, shape):
    """acc_int: integers in [-8, 8]; acc_round: integers m with 2^(p-1) <= |m| < 2^p, p the significant bits of the storage type: any fraction of
    the incoming gradient is then rounded away"""
    if kind == "acc_int":
        return int_operand(*shape, amp=8, seed=_seed(name, 10))
    g = torch.Generator().manual_seed(_seed(name, 11))
    p = MANT[dtype]
    m = torch.randint(2 ** (p - 1), 2 ** p, shape, generator=g).double() * (2 * torch.randint(0, 2, shape, generator=g) - 1).double()
    return m.float()


def _grad(A64, absA64, d, dtype, M, dq0=None):
    """the expectation of a gradient that carries the softmax scale: bits, or the fp32 bound where the scale is no power of two"""
    sc = scale32(d)
    if dtype == torch.float32 and not pow2_scale(d):
        ref, A = A64 * sc, absA64 * sc
        if dq0 is not None:
            ref, A = ref + dq0.double(), A + dq0.double().abs()
        return Exp(None, ref, A, F32_COEFF(M))
    v = _fl32(A64 * sc)
    if dq0 is not None:
        v = _fl32(v + dq0.double())
    return Exp(rne(v + 0.0, dtype), None, None, None)


@functools.lru_cache(maxsize=4)
def build(name, mode):
    """operands, the exact ``out`` [B, N, H, d] (fp64 integers) and ``lse`` (= k) per segment, and the expected dq / dk / dv of every variant"""
    c, dtype = BY_NAME[name], MODES[mode]
    a, o = c.args, operands(name)
    B, N, H, d = o.q.shape
    exp, dq0s, refs = {}, {}, []
    for si, sg in enumerate(o.segs):
        r = backward64(o.q, o.do, sg)
        refs.append(r)
        L = sg.k.shape[1]
        tag = "" if si == 0 else "2"
        exp["dk" + tag] = _grad(r["Ak"], r["absk"], d, dtype, N)
        exp["dv" + tag] = Exp(rne(r["Av"] * sg.s + 0.0, dtype), None, None, None)
        if si == 0:
            exp["dq"] = _grad(r["Aq"], r["absq"], d, dtype, L)
            for kind in (("acc_int", "acc_round") if a.get("acc") else ()):
                dq0s[kind] = dq0_operand(name, kind, dtype, (B, N, H, d))
                exp["dq_" + kind] = _grad(r["Aq"], r["absq"], d, dtype, L, dq0s[kind])
        else:  # the step's order: the audio segment accumulates into the text segment's (stored) dq
            assert exp["dq"].bits is not None, "the IP pair runs at a head size whose scale is a power of two"
            dq0s["ip"] = exp["dq"].bits.float()
            exp["dq_ip"] = _grad(r["Aq"], r["absq"], d, dtype, L, dq0s["ip"])
    out = [sg.O for sg in o.segs]
    lse = [float(sg.kexp) for sg in o.segs]
    return Built(o, out, lse, exp, dq0s, refs)


def variants(name, mode):
    a = BY_NAME[name].args
    if "L2" in a:
        return ["ip", "ip_chained"]
    v = ["plain", "nodkv", "chained"]
    if a["N"] == a["L"] and mode != "f32":
        v.append("packed")
    if a.get("acc"):
        v += ["acc_int", "acc_round"]
    return v


def exact_lse(B, H, N, Npad, k, dev):
    """[B, H, Npad] fp32: k for every query, NaN in the pad entries"""
    t = torch.full((B, H, Npad), float("nan"), dtype=torch.float32)
    t[..., :N] = float(k)
    return t.to(dev)


def forward(o, sg, ops, dev, dtype):
    """ops.attention_lse of a segment: -> (out [B, N, C], lse [B, H, Npad])"""
    from util import nan_padded_vt
    B, N, H, d = o.q.shape
    L = sg.k.shape[1]
    D = lambda t: t.reshape(t.shape[0], t.shape[1], H * d).to(dev, dtype).contiguous()
    vt = nan_padded_vt(sg.v, ops.round_up(L, 32), dtype, dev, poison=False)
    return ops.attention_lse(D(o.q), D(sg.k), vt, L, H, key_bias=None if sg.bias is None else sg.bias.to(dev))


def run(name, built, ops, dev, mode, variant="plain", fwd=None):
    """launch one variant of the case through ops.attention_bwd: -> dict of the gradients it returns ([B, rows, H, d] views).
    fwd: the (out, lse) pairs of ``forward`` per segment, for the chained variants"""
    dtype, o = MODES[mode], built.ops
    B, N, H, d = o.q.shape
    D = lambda t: t.reshape(t.shape[0], t.shape[1], H * d).to(dev, dtype).contiguous()
    U = lambda t: None if t is None else t.reshape(B, -1, H, d)
    Np = ops.round_up(N, 32)
    q, do = D(o.q), D(o.do)
    chained = variant in ("chained", "ip_chained")
    res = {}
    for si, sg in enumerate(o.segs):
        k, v = D(sg.k), D(sg.v)
        bias = None if sg.bias is None else sg.bias.to(dev)
        if chained:
            out, lse = fwd[si]
        else:
            out, lse = D(built.out[si].float()), exact_lse(B, H, N, Np, built.lse[si], dev)
        kw = dict(key_bias=bias, dout_scale=sg.s)
        if variant == "nodkv":
            kw["need_dkv"] = False
        elif variant == "packed":
            kw["packed"] = True
        elif variant in ("acc_int", "acc_round"):
            kw["dq"] = D(built.dq0[variant])
        elif si == 1:
            kw["dq"] = res["dq"].reshape(B, N, H * d)
        dq, dk, dv = ops.attention_bwd(q, k, v, out, do, lse, H, **kw)
        if variant == "packed":
            assert dq._base is not None and dq._base is dk._base is dv._base and tuple(dq._base.shape) == (B, N, 3 * H * d), "not one [B, N, 3C] buffer"
        if variant in ("acc_int", "acc_round"):
            assert dq.data_ptr() == kw["dq"].data_ptr(), "dq= is accumulated into in place"
        tag = "" if si == 0 else "2"
        res["dq"] = U(dq)
        res["dk" + tag], res["dv" + tag] = U(dk), U(dv)
    return res


def expected_of(built, variant):
    """{result name: Exp} of a variant's results"""
    e = built.exp
    if variant in ("ip", "ip_chained"):
        return {"dq": e["dq_ip"], "dk": e["dk"], "dv": e["dv"], "dk2": e["dk2"], "dv2": e["dv2"]}
    if variant == "nodkv":
        return {"dq": e["dq"]}
    if variant in ("acc_int", "acc_round"):
        return {"dq": e["dq_" + variant], "dk": e["dk"], "dv": e["dv"]}
    return {"dq": e["dq"], "dk": e["dk"], "dv": e["dv"]}


def _c(name, modes=ALL, B=2, H=2, **args):
    return Case(name, dict(args, B=B, H=H), modes)


CONTROL = "control_N32_L2_d16_k1"
CASES = [
    _c(CONTROL, N=32, L=2, d=16, k=1),  # the smallest k = 1 case: one group of two keys
    # ---- every head size at an odd tile count above one in both passes (L in 65 / 96 / 160: 3, 3, 5 key tiles; N in 129 / 160: 5 query tiles)
    _c("d16_N129_L65_k2_edges", N=129, L=65, d=16, k=2, bias="edges", unmasked=1, acc=True),  # decoys: key 0, key 64 alone in the last tile
    _c("d32_N160_L96_k3", N=160, L=96, d=32, k=3, s=0.5, acc=True),
    _c("d48_N129_L160_k4", N=129, L=160, d=48, k=4),
    _c("d64_N129_L65_k0", N=129, L=65, d=64, k=0, s=0.5),
    _c("d80_N160_L65_k1", N=160, L=65, d=80, k=1),
    _c("d128_N160_L65_k2", ("f32",), N=160, L=65, d=128, k=2),  # (one orphan key)
    # ---- the step's decoupled pair: text (masked) first, then audio with s = 0.5 accumulating into its dq; d = 64: bits in fp32 too
    _c("ip_N129_L33_L65_d64", N=129, L=33, d=64, k=1, G=15, bias="edges", unmasked=0, L2=65, k2=2, s2=0.5),
    # ---- self-shaped (N == L): packed, the one-launch three-tensor transpose
    _c("self_N97_d32_k2_tile0", N=97, L=97, d=32, k=2, bias="tile0", unmasked=0, s=0.5),  # a whole first key tile masked, and the last key
    _c("self_N31_d80_k0", N=31, L=31, d=80, k=0, s=0.5),
    _c("self_N32_d64_k4", N=32, L=32, d=64, k=4, acc=True),
    _c("self_N33_d48_k2_edges", N=33, L=33, d=48, k=2, bias="edges", unmasked=1),
    # ---- the small ends
    _c("N1_L8_d16_k3", N=1, L=8, d=16, k=3),
    _c("N1_L1_d48_k0", N=1, L=1, d=48, k=0),
    _c("N97_L64_d80_k3", N=97, L=64, d=80, k=3, s=0.5),
    _c("N31_L97_d64_k2", N=31, L=97, d=64, k=2),  # (one orphan key; four key tiles)
    _c("H3_N33_L8_d16_k2", H=3, N=33, L=8, d=16, k=2),  # C = 48: a partial 32-channel tile in head_transpose_kernel
    _c("B3_N32_L33_d32_k0", B=3, N=32, L=33, d=32, k=0),
]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
AUTOGRAD = ("d16_N129_L65_k2_edges", "self_N33_d48_k2_edges", "ip_N129_L33_L65_d64")  # the cases the autograd entry points run


def params():
    return [(c.name, m) for c in CASES for m in c.modes]
