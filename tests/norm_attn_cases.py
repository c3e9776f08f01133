"""The LayerNorm inside the fused attention kernels, held to the selection tier of tests/attn_exact_cases.py on tier-R rows of
tests/norm_exact_cases.py: ops.fused_cross_attention(ln=), ops.cross_attention_rows(ln=), ops.hs_attention(normalize=True) (cross and self) and
ops.self_attention_fused.  tests/test_norm_exact_host.py checks the conditions below on the CPU, tests/test_gpu_exact_norm.py runs the cases.

Every row of x holds m - a and m + a in equal numbers ((m, a) differs between neighbouring rows), so mean = m, variance = a^2 and the normalised
channel j is s_j gamma_j + beta_j up to 5e-6, with s_j = +-1 the side x_j lies on.  The signs carry the codes of the selection tier:
  q code  dims 0..15 of a head: s = -1 on the 8 dims of the set S_sel the query selects, +1 on the others.  On these channels gamma = beta (a power of
          two 1/8, 1/4, 1/2 by channel: the one place where the +-gamma + beta of tier R may be 0), and W_q has the single weight w = 4096 on the
          diagonal: q = w (s gamma + beta) is 0 on S_sel and 2 w gamma >= 1024 elsewhere (up to w gamma 5e-6 and the fp32 rounding of the fold).
  k code  (self-attention) dims 16..31 of a head: s = +1 on the token's own set S_n, gamma = beta as above, W_k = -1 / (2 gamma) from that channel to
          dim c: k = -1 on S_n, 0 elsewhere, as in tier S.  Cross-attention takes k = -codes from the key set, as attn_exact_cases does.
  values  self-attention: W_v = the identity, V = the normalised row itself, +-gamma + beta in every channel: exactly representable once rounded to the
          storage type (tier R's margin).  Cross-attention: V = util.exact_operand rows of the key set.
The selected key scores about 0, every other key at most -(2 w gamma_min) = -1024, at least -165 in the base-2 exponent at d = 80 (-261 at d = 32):
p_sel = exp2(0) = 1, every other p = 0 in fp32, the denominator is 1 -- WHATEVER the last bits of q are, which is why the folded forms (the
LayerNorm applied by algebra on the accumulators, a weight rounded after gamma and the softmax scale went in) are held to bits too.  What moves the
result is a wrong statistic, row, channel or fold vector: q = rstd (acc - mean * colsum) + W beta with colsum = w gamma and W beta = w beta in the
thousands, so a mean, a column sum or a beta taken from a neighbour shifts q by hundreds to thousands and hands the query to another key.
No "difference of two channels" weight is used: it would make colsum and W beta vanish and blind the case to exactly those errors.

Expected, IN EVERY BIT in bf16 and f16:
  fused_cross_attention, cross_attention_rows   rne(x + V[sel]): W_o = the identity, b_o = 0; the attention result V[sel] is representable, so the two
      stated roundings (xattn_kernel: "out^T = Wo_slice . O^T + bias, rounded, ADDED IN PLACE to" the x tile) collapse into the one of the sum, which
      is exact in fp32 (an integer plus a bf16 value)
  hs_attention cross                            V[sel]
  hs_attention self, self_attention_fused       V[sel] = the normalised row of the selected token, s gamma + beta.  One exception, decided on the
      reference alone: sattn_fused_kernel applies the LayerNorm to v by algebra (ap-adapter_amd/csrc/attention.hip, ``rstd * (acc - mean * cs) +
      bb``), so where s gamma + beta = 0 (the gamma = beta code channels) it holds gamma (1 - a rstd) = gamma eps / (2 a^2) <= 2.5e-6, a value whose
      16-bit rounding the fp32 error of rstd can move: there the test asserts |out| <= 2^-16 and compares the other elements bit for bit.
      hs_attn_kernel rounds the normalised row to the storage type first (ap-adapter_amd/csrc/hsattn.hip: ``v[e] = __builtin_fmaf(v[e], rstd, nm)``
      then ``pack8<DT>(v)``: +-1 exactly), so its 0 is an exact 0 and every element is compared.
The rounding steps relied on: the normalised value that becomes V is rounded to the storage type before the P.V product (every kernel feeds 16-bit
MFMA operands), and it lies within 2^-6 ulp of the dyadic value (tier R's pairs)."""
import functools
import math
import zlib
from collections import namedtuple

import torch

import attn_exact_cases as AC
import norm_exact_cases as NC
from util import exact_operand

W_CODE = 4096.0
H = 8
ACase = namedtuple("ACase", "name route C B N L eps")
ABuilt = namedtuple("ABuilt", "x gamma beta wq wk wv k v sel xn ref scores")

CASES = [
    ACase("xattn_ln_33", "xattn", 256, 3, 33, 8, 1e-5), ACase("xattn_ln_130", "xattn", 256, 3, 130, 40, 1e-6),
    ACase("xrows_ln_33", "xrows", 384, 3, 33, 8, 1e-5), ACase("xrows_ln_100", "xrows", 384, 3, 100, 40, 1e-6),
    ACase("hs_cross_ln_33", "hs_cross", 640, 3, 33, 40, 1e-5), ACase("hs_cross_ln_64", "hs_cross", 640, 3, 64, 8, 1e-6),
    ACase("hs_self_ln_33", "hs_self", 640, 3, 33, 33, 1e-5), ACase("hs_self_ln_64", "hs_self", 640, 3, 64, 64, 1e-6), ACase("hs_self_ln_1", "hs_self", 640, 3, 1, 1, 1e-5),
    ACase("sattn_ln_C256_N513", "sattn", 256, 2, 513, 513, 1e-5), ACase("sattn_ln_C384_N130", "sattn", 384, 2, 130, 130, 1e-6),
]
BY_NAME = {c.name: c for c in CASES}
SELF = ("hs_self", "sattn")


def _seed(name, i):
    return (zlib.crc32(name.encode()) + 7919 * i) % (2 ** 31)


@functools.lru_cache(maxsize=2)
def build(name):
    c = BY_NAME[name]
    C, B, N, L, d = c.C, c.B, c.N, c.L, c.C // H
    self_ = c.route in SELF
    assert L == N or not self_
    codes = AC.code_sets(B * H, L, _seed(name, 0)).reshape(B, H, L, 16)  # the key sets S_j, distinct per (sample, head)
    sel = AC.select(B, H, N, L, list(range(L)), {}, _seed(name, 1))  # [B, H, N]
    bi, hi = torch.arange(B)[:, None, None], torch.arange(H)[None, :, None]
    selcode = codes[bi, hi, sel].permute(0, 2, 1, 3)  # [B, N, H, 16]: 1 on S_sel
    g = torch.Generator().manual_seed(_seed(name, 2))
    ncode = 32 if self_ else 16
    s = torch.empty(B, N, H, d)
    s[..., :16] = 1.0 - 2.0 * selcode
    if self_:
        s[..., 16:32] = 2.0 * codes.permute(0, 2, 1, 3) - 1.0  # token n is key n: +1 on its own set
    if d > ncode:
        s[..., ncode:] = NC._balanced_signs(B * N * H, d - ncode, g).reshape(B, N, H, d - ncode)
    s = s.reshape(B * N, C)
    assert bool((s.sum(1) == 0).all())
    ma = torch.tensor(NC.MA, dtype=torch.float32)[NC._ma_index(B * N, 1).reshape(-1)]
    x = ma[:, :1] + s * ma[:, 1:]
    gamma, beta = NC.gamma_beta(C, "R", _seed(name, 3))
    ch = torch.arange(C) % d
    pow2 = torch.tensor([0.125, 0.25, 0.5])[(torch.arange(C) + torch.arange(C) // d) % 3]
    code = ch < ncode
    gamma, beta = torch.where(code, pow2, gamma), torch.where(code, pow2, beta)
    wq = torch.diag(torch.where(ch < 16, torch.tensor(W_CODE), torch.tensor(0.0)))
    wk = wv = None
    if self_:
        wk = torch.zeros(C, C)
        cols = torch.arange(C)[(ch >= 16) & (ch < 32)]
        wk[cols - 16, cols] = -1.0 / (2.0 * gamma[cols])
        wv = torch.eye(C)
    xn = s.double() * gamma.double() + beta.double()  # the normalised row, eps apart
    if self_:
        k = v = None
        vv = xn.reshape(B, N, H, d)
    else:
        k = torch.zeros(B, L, H, d)
        k[..., :16] = -codes.permute(0, 2, 1, 3)
        v = exact_operand(B, L, H, d, seed=_seed(name, 4))
        vv = v.double()
    picked = vv.permute(0, 2, 1, 3)[bi, hi, sel].permute(0, 2, 1, 3).reshape(B * N, C)  # V[sel] [B, N, H, d]
    ref = picked + x.double() if c.route in ("xattn", "xrows") else picked
    # the fp64 scores in the base-2 exponent, for the host test: q from the fp64 LayerNorm of x
    mean, var = x.double().mean(1, keepdim=True), x.double().var(1, unbiased=False, keepdim=True)
    ln = (x.double() - mean) / (var + c.eps).sqrt() * gamma.double() + beta.double()
    q = (ln @ wq.double().t()).reshape(B, N, H, d)
    kk = (ln @ wk.double().t()).reshape(B, N, H, d) if self_ else k.double()
    scores = torch.einsum("bnhd,blhd->bhnl", q, kk) * (math.log2(math.e) / math.sqrt(d))
    return ABuilt(x.reshape(B, N, C), gamma, beta, wq, wk, wv, k, v, sel, xn, ref.reshape(B, N, C), scores)


def run(name, dtype, ops, dev, out):
    from util import nan_padded_vt
    c, bt = BY_NAME[name], build(name)
    C, B, N, L, d = c.C, c.B, c.N, c.L, c.C // H
    D = lambda t: t.to(dev, dtype).contiguous()
    x, ln = D(bt.x), (D(bt.gamma), D(bt.beta), c.eps)
    eye, zero = torch.eye(C), torch.zeros(C, dtype=dtype, device=dev)
    if c.route == "xattn":
        assert ops.xattn_lengths_ok(L, 0, False)
        wq_p, q_fold = ops.xattn_pack_weight(D(bt.wq), ln=ln)
        kv = ops.xattn_pack_kv(D(bt.k.reshape(B, L, C)), nan_padded_vt(bt.v, ops.round_up(L, 32) + 32, dtype, dev, poison=True), L)
        return ops.fused_cross_attention(x, wq_p, ops.xattn_pack_weight(D(eye)), zero, kv, L, H, ln=ln, q_fold=q_fold, out=out)
    if c.route == "xrows":
        assert ops.xrows_ok(C, H, L, 0)
        vt = nan_padded_vt(bt.v, ops.round_up(L, 32), dtype, dev, poison=False)
        return ops.cross_attention_rows(x, ops.xrows_pack_weight(D(bt.wq)), ops.xrows_pack_weight(D(eye)), zero, D(bt.k.reshape(B, L, C)), vt, H, ln=ln, out=out)
    if c.route == "hs_cross":
        assert ops.hs_cross_lengths_ok(L, 0)
        pk, bb = ops.hs_pack_rows(D(bt.wq), ln=ln)
        vt = nan_padded_vt(bt.v, ops.round_up(L, 32), dtype, dev, poison=False)
        return ops.hs_attention(x, pk, bb, self_attention=False, normalize=True, ln_eps=c.eps, k1=D(bt.k.reshape(B, L, C)), vt1=vt, out=out)
    if c.route == "hs_self":
        pk, bb = ops.hs_pack_qkv(D(bt.wq), D(bt.wk), D(bt.wv), ln=ln)
        return ops.hs_attention(x, pk, bb, self_attention=True, normalize=True, ln_eps=c.eps, out=out)
    assert c.route == "sattn" and ops.sattn_ok(x, H), "outside the token counts routed to apad_self_attention_fused"
    w, csbb = ops.sattn_pack(D(bt.wq), D(bt.wk), D(bt.wv), ln, H)
    return ops.self_attention_fused(x, w, csbb, H, c.eps, out=out)


def params():
    return [(c.name, m) for c in CASES for m in ("bf16", "f16")]
