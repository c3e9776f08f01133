"""The case table of the exact-statistics normalisation tests: tests/test_norm_exact_host.py builds every case's operands and fp64 reference on the
CPU and checks the conditions of its tier; tests/test_gpu_exact_norm.py runs the same cases through the public ``ops`` wrappers.

A **set** is what one normalisation reduces over: a LayerNorm / RMS row, or the (sample, group) slab [HW][C / G] of a GroupNorm.  Every set is built
from small integers (the small-variance kind: integers times 2^-6), so every partial sum of x and of x^2 is an integer (times 2^-6, 2^-12) below
2^24: both sums are exact in fp32 in ANY order -- vector width, pixel lanes, chunk partials, butterflies.  Every set keeps |mean| <= sigma (the host
test asserts it; flat sets, whose variance is exactly 0 under both formulas, apart), so ``E[x^2] - mean^2`` (norm.hip's GroupNorm, train_ops.hip) and
the shifted form (LayerNorm, f32_ops.hip) are both accurate to a few fp32 ulp.  The centring is deliberate: the suite does not judge either formula
on off-centre sets.

Tier R (representable).  A set holds the two values m - a and m + a in equal numbers, placed by a seeded permutation; a in {1, 2, 4}, integer
  |m| <= a, (m, a) different in neighbouring rows, groups and samples (MA, _ma_index).  mean = m and variance = a^2 exactly, so the normalised value is
  +-a / sqrt(a^2 + eps) = +-(1 - eps / (2 a^2) + ...), at most 5.0e-6 off +-1, and the output +-gamma + beta up to |gamma| * 5e-6.  gamma is an odd
  multiple of 1/8, beta a multiple of 1/4, |gamma|, |beta| <= 4: +-gamma + beta is a non-zero multiple of 1/8 below 8, exact in bf16 and f16.  Of
  those pairs tier R keeps the ones whose perturbation at a = 1, eps = 1e-5 stays below 2^-6 f16 ulp of the smaller of |gamma + beta|, |beta - gamma|
  (``_pairs``: 2^-6 of a f16 ulp is far from the tie at 1/2, and a bf16 ulp is 8 times wider), so IN THE 16-BIT MODES THE OUTPUT IS +-gamma + beta
  IN EVERY BIT.  (gamma, beta) pairs are dealt by a seeded permutation of the list: any window of len(list) channels holds distinct pairs.
  With SiLU (tier "S" in the tables: tier R operands, silu=True, 16-bit modes) the kernels round the normalised value to the storage type first ("storage rounding before SiLU", gn_apply_kernel): that value is the
  exact dyadic y, and only silu_f and the last rounding are inexact: the tier-K bound with A = |silu(y)| + |y|.
Tier K (spiked integers).  Integers in [-3, 3] from a seeded generator plus spikes of +-48 at the positions the case lists (last pixel, the single
  pixel of a tail chunk, either side of a chunk boundary, first / last channel of a group, both sides of the source boundary, the last row): an
  element dropped, doubled or taken from a neighbour moves mean and sigma by far more than a 16-bit ulp.  Kinds of tier K: "small" -- values +-2^-6
  with random signs, eps = 1e-5 is 4 % of the variance 2^-12; "flat" -- every element of a set is 1 (or 2): the output is beta.
  Bound: |out - ref64| <= 0.5 ulp_dtype(ref64) + 16 * 2^-24 * A,  A = (|x| + |mean|) * rstd * |gamma| + |beta| per element.

The 16, in units of u = 2^-24 (the relative error of one fp32 rounding), for out = ((x - mean) * rstd) * gamma + beta with exact sums S, Q:
    mean = S / n                              1 u of |mean|                      -> 1 u of A
    x - mean                                  1 u of |x - mean| <= |x| + |mean|  -> 1 u of A
    variance, E[x^2] - mean^2 form: Q / n (1 u of E[x^2] <= 2 sigma^2 under |mean| <= sigma), mean * mean (3 u of mean^2 <= sigma^2), the difference
      (1 u): <= 6 u of sigma^2; + eps 1 u; rstd takes half: 3.5 u; rsqrtf / 1 / sqrtf: 1 ulp = 2 u          -> 5.5 u of A
    variance, shifted form: each d = x - mean carries 2 u (|x| + |mean|), so d^2 carries <= 4 u * 2 sigma * |d| ... summed and halved the same
      3 - 4 u, plus the rounding of the sum of squares itself (not exact: d is no integer).  A thread that adds k positive terms of about sigma^2 in
      turn rounds its j-th partial sum, about j sigma^2, by a uniform error within +-u j sigma^2: variance u^2 sigma^4 j^2 / 3, summed over j
      k^3 u^2 sigma^4 / 9, i.e. a relative error of the sum of u sqrt(k) / 3 (one sigma; the butterfly adds log2(threads) roundings, below 1 u
      together), of which rstd takes half: at three sigma u sqrt(k) / 2.  (Worst case, every rounding the same way: k u / 4.)  k is
      SHIFTED_ADDS: C / 64 <= 32 for a LayerNorm row (2.8 u), HW cg / 256 for the fp32 GroupNorm's 256 threads, 157 on the largest slab here
      (6.3 u).  The bound therefore rests on k: tests/test_norm_exact_host.py asserts k <= SHIFTED_ADDS_MAX = 160 for every case a shifted-form kernel
      runs (shifted_adds), so that a larger fp32 shape fails there, pointing here, and not on the GPU; such a shape needs a coefficient that grows
      with sqrt(k) / 2 for that kernel, not a wider 16 for all
    * rstd, * gamma, + beta                   3 u of A
  11 - 12 u derived as the sum of worst cases, 16 allowed.  For the E[x^2] - mean^2 kernels that is the whole of it.  For the shifted-form kernels
  the sum-of-squares term comes on top: 2.8 u for LayerNorm, inside the 4 u left; 6.3 u at k = 157, inside 16 only because a dozen independent
  roundings do not all reach their worst case together (added in quadrature, the 11 - 12 u are below 5 u).  tests/test_norm_exact_host.py emulates
  both formulas in fp32, each summed in two orders, and asserts the worst |error| / (16 u A) over every case (its docstring records it: 0.91 at k = 157).
  The half ulp is the final rounding to the storage type.  Nothing here was read off a kernel's output.

Backward (ln_bwd / gn_bwd, tier R operands, integer dy in [-3, 3] with +-48 spikes): dx = rstd * (dy gamma - mean(dy gamma) - xhat * mean(dy gamma
  xhat)); bound 0.5 ulp + 16 u A with A = rstd * (|dy gamma| + |mean(dy gamma)| + |mean(dy gamma xhat)|) -- the three terms cancel, so the bound is
  on their magnitudes, never relative to |dx|.  ``dres`` and SiLU are left out: both round to the storage type mid-way.

LayerNorm inside a fused kernel (op "rp_ln": ops.fused_linear(ln=) on the row-panel kernel, K = 256 / 384), tier R only.  rp_gemm_kernel normalises the
  x panel in registers and rounds it to the storage type before the matrix instruction (ap-adapter_amd/csrc/rpgemm.hip:
  ``xf[c][j] = (typename E::elem)(((float)xf[c][j] * rstd + nmr) * (float)g[j] + (float)b[j]);`` with nmr = -mean * rstd): x * rstd and nmr carry one
  rounding each, 3 u of (|x| + |mean|) rstd <= 9 u next to the 5e-6 of eps, still far inside tier R's tie margin, so the operand is +-gamma + beta
  exactly.  With weights in {-1, 0, 1} and an integer bias every product sum is a multiple of 1/8 below 2^21: exact in fp32 in any order, and the
  output is rne(y W^T + b) IN EVERY BIT, representable or not.  This holds row, channel and gamma / beta indexing and the M tail of the row tile.

LayerNorm folded into apad_gemm (op "fold_ln": ops.linear(ln=) at K = 640, x from a producer launched with rowstat=True -- the identity weight over
  tier-R rows, so that the stored rows ARE tier-R rows and the 64-column partial sums exact integers).  The kernel applies the LayerNorm by algebra
  (ap-adapter_amd/csrc/gemm_shared.h, epi_acc_to_lds: ``v = rstat[ml][1] * (acc[r] - rstat[ml][0] * c.lcs) + c.lbb``): acc = x . (W gamma), the column sums, mean = m and
  acc - mean * colsum are exact multiples of 1/8; rstd multiplies AFTER the sum, so its (1 + delta) -- the eps add, rsqrtf: <= 3 u -- reaches the output,
  followed by one multiply, one add and the storage rounding: the bound form, 0.5 ulp + 16 u A with A = |xhat gamma| . |W|^T + |beta| . |W|^T + |b|.

``route_of`` restates the dispatch of ln_launch / gn_onepass_launch / gn_launch (ap-adapter_amd/csrc/norm.hip) and of the fp32 entries; every case names the form
it is meant for, and both test files assert that it lands there."""
import functools
import math
import zlib
from collections import namedtuple

import torch

DTYPES = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}
D16 = ("bf16", "f16")
DALL = ("bf16", "f16", "f32")
U = 2.0 ** -24
COEFF = 16.0
SPIKE = 48.0
GN_CHUNK, GN_APPLY_CHUNK = 64, 256  # csrc/norm.hip

Case = namedtuple("Case", "name op form args tiers dtypes")
Built = namedtuple("Built", "x xa xb gamma beta dy eps groups ref absref y sets mean var w wb xn", defaults=(None, None, None))


def _seed(name, i=0):
    return (zlib.crc32(name.encode()) + 7919 * i) % (2 ** 31)


# ---- (m, a) of tier R: a in {1, 2, 4}, integer |m| <= a
MA = [(m, a) for a in (1, 2, 4) for m in range(-a, a + 1)]
assert len(MA) == 17


def _ma_index(outer, inner):
    """[outer, inner] indices into MA: neighbours differ along both axes (steps 7 and 5 modulo 17)"""
    return (7 * torch.arange(outer)[:, None] + 5 * torch.arange(inner)[None, :] + 1) % len(MA)


@functools.lru_cache(maxsize=None)
def _pairs(tier):
    """the (gamma, beta) pairs of a tier: gamma odd / 8, beta k / 4, both within [-4, 4].  Tier R keeps the pairs whose perturbation |gamma| * (1 -
    1 / sqrt(1 + 1e-5)) (a = 1, eps = 1e-5: the largest of all tier-R sets) is at most 2^-6 of the f16 spacing at min(|beta + gamma|, |beta - gamma|)"""
    out = []
    delta = 1.0 - 1.0 / math.sqrt(1.0 + 1e-5)
    for gi in range(-31, 32, 2):
        for bi in range(-16, 17):
            g, b = gi / 8.0, bi / 4.0
            lo = min(abs(b + g), abs(b - g))
            if tier == "R" and abs(g) * delta > 2.0 ** -6 * 2.0 ** (math.floor(math.log2(lo)) - 10):
                continue
            out.append((g, b))
    return out


def gamma_beta(C, tier, seed):
    """[C] fp32 gamma, beta: the tier's pairs in a seeded order, repeated: any window of len(pairs) channels holds distinct pairs"""
    p = torch.tensor(_pairs("R" if tier == "R" else "K"))
    p = p[torch.randperm(p.shape[0], generator=torch.Generator().manual_seed(seed))]
    idx = torch.arange(C) % p.shape[0]
    return p[idx, 0].float().contiguous(), p[idx, 1].float().contiguous()


# ---- sets <-> tensors
def to_sets(x, G):
    """x [M, C] (G None: a set per row) or [B, HW, C] -> [sets, n]"""
    if G is None:
        return x.reshape(-1, x.shape[-1])
    B, HW, C = x.shape
    return x.reshape(B, HW, G, C // G).permute(0, 2, 1, 3).reshape(B * G, HW * (C // G))


def from_sets(s, shape, G):
    if G is None:
        return s.reshape(shape)
    B, HW, C = shape
    return s.reshape(B, G, HW, C // G).permute(0, 2, 1, 3).reshape(B, HW, C).contiguous()


def _balanced_signs(S, n, g):
    """[S, n] +-1 with n / 2 of each per row, placed by a seeded permutation"""
    assert n % 2 == 0
    return torch.where(torch.rand(S, n, generator=g).argsort(1) < n // 2, 1.0, -1.0)


def tier_r_sets(ma_idx, n, seed):
    """ma_idx [S] -> [S, n] fp32: row s holds MA[ma_idx[s]] = (m, a) as m - a and m + a, n / 2 each"""
    ma = torch.tensor(MA, dtype=torch.float32)[ma_idx.reshape(-1)]
    sg = _balanced_signs(ma.shape[0], n, torch.Generator().manual_seed(seed))
    return ma[:, :1] + sg * ma[:, 1:]


def _spiked(shape, spikes, seed, G):
    """integers in [-3, 3] + spikes (index tuple -> +-48, alternating); sets that leave |mean| <= sigma (tiny ones only) are drawn again"""
    g = torch.Generator().manual_seed(seed)
    mask = torch.zeros(shape, dtype=torch.bool)
    val = torch.zeros(shape)
    for i, idx in enumerate(spikes):
        mask[idx] = True
        val[idx] = SPIKE if i % 2 == 0 else -SPIKE
    draw = lambda: torch.where(mask, val, torch.randint(-3, 4, shape, generator=g).float())
    x = draw()
    for _ in range(64):
        s = to_sets(x, G).double()
        bad = s.mean(1).abs() > s.var(1, unbiased=False).sqrt()
        if not bool(bad.any()):
            return x
        s2 = to_sets(draw(), G)
        x = from_sets(torch.where(bad[:, None], s2, to_sets(x, G)), shape, G)
    raise AssertionError("could not centre every set")


def norm64(x, G, gamma, beta, eps, rms=False, l2=False):
    """fp64 reference -> (ref, A, mean [sets], var [sets]); A = (|x| + |mean|) rstd |gamma| + |beta|"""
    shape = x.shape
    s = to_sets(x.double(), G)
    if rms or l2:
        mean = torch.zeros(s.shape[0], dtype=torch.float64)
        var = (s * s).mean(1)
        rstd = 1.0 / (s * s).sum(1).sqrt().clamp_min(eps) if l2 else 1.0 / (var + eps).sqrt()
    else:
        mean = s.mean(1)
        var = s.var(1, unbiased=False)
        rstd = 1.0 / (var + eps).sqrt()
    xh = from_sets((s - mean[:, None]) * rstd[:, None], shape, G)
    ab = from_sets((s.abs() + mean.abs()[:, None]) * rstd[:, None], shape, G)
    g = torch.ones(shape[-1], dtype=torch.float64) if gamma is None else gamma.double()
    b = torch.zeros(shape[-1], dtype=torch.float64) if beta is None else beta.double()
    return xh * g + b, ab * g.abs() + b.abs(), mean, var


def silu64(y):
    return y * torch.sigmoid(y)


# ---- the dispatch restated (csrc/norm.hip: ln_launch, gn_onepass_launch, gn_launch; apad_layernorm / apad_groupnorm2 for the fp32 entries)
def route_of(op, a, is16):
    if op in ("rms", "l2"):
        return "wave_row"
    if op == "fold_ln":  # ops.ln_foldable: 16-bit, row statistics, a width the row-panel kernel does not cover; the producer: N % 64 == 0, not in RP_K
        return "folded" if a["C"] not in (256, 384) and a["C"] % 64 == 0 and is16 else None
    if op == "rp_ln":  # ops.fused_linear: rp_ok(x, K) and N % 64 == 0
        return "rowpanel" if a["C"] in (256, 384) and a["N"] % 64 == 0 and is16 else None
    if op in ("ln_bwd", "gn_bwd"):
        return op
    if op == "ln":
        C = a["C"]
        if not is16:
            return "f32_tail" if C % 256 else "f32"
        assert C % 8 == 0 and C <= 2048
        nvec = C // 8
        return "nv1" if nvec <= 64 else "nv2" if nvec <= 128 else "nv4"
    assert op in ("gn", "gn2")
    HW, G = a["HW"], a["G"]
    C = a["C"] if op == "gn" else a["Ca"] + a["Cb"]
    two = op == "gn2"
    if not is16:
        assert not two
        return "f32"
    cg = C // G
    assert G <= 64 and C % G == 0 and cg % 4 == 0 and C % 8 == 0 and C <= 1280
    if HW <= 1024 and cg in (8, 4) and G % (64 // cg) == 0 and not two:
        return "full8" if cg == 8 else "full4"
    if not (HW > 1024 or G % 4 != 0 or cg % 4 != 0 or cg > 40):
        vps = 4 * cg // 8
        if (HW + 256 // vps - 1) // (256 // vps) <= 24:
            return "onepass256"
        if (HW + 1024 // vps - 1) // (1024 // vps) <= 12:
            return "onepass1024"
    nchunk = (HW + GN_CHUNK - 1) // GN_CHUNK
    return ("twopass_fast" if 256 % (C // 8) == 0 else "twopass_generic") + ("_65" if nchunk > 64 else "")


# ---- builders
def _ln_like(c, tier):
    a = c.args
    M, C = a["M"], a["C"]
    kind = a.get("kind")
    if tier == "R" and c.op in ("rms", "l2"):  # rows +-a: a = 1, 2, 4 by row (MA's m = 0 entries)
        x = tier_r_sets(torch.tensor([1, 5, 12])[torch.arange(M) % 3], C, _seed(c.name, 1)).reshape(M, C)
    elif tier == "R":
        x = tier_r_sets(_ma_index(M, 1).reshape(-1), C, _seed(c.name, 1)).reshape(M, C)
    elif kind == "small":
        x = torch.where(torch.rand(M, C, generator=torch.Generator().manual_seed(_seed(c.name, 1))) < 0.5, -1.0, 1.0) * 2.0 ** -6
    elif kind == "flat":
        x = (1.0 + (torch.arange(M) % 2).float())[:, None].expand(M, C).contiguous()
    else:
        x = _spiked((M, C), [(M - 1, C - 1), (0, 0), (M - 1, 0), (M // 2, C - 8), (M - 1, min(C - 1, 511)), (M - 1, min(C - 1, 512))], _seed(c.name, 1), None)
    return x


def _gn_spikes(B, HW, C, G, Ca=None):
    """last pixel; the single pixel of a tail chunk (= the last pixel where HW % 64 == 1); either side of the partial and the apply chunk boundaries;
    first and last channel of a group; both sides of the source boundary; chunk 64 of a launch with more than 64 chunks"""
    cg = C // G
    pts = [(B - 1, HW - 1, C - 1), (0, HW - 1, 0), (B - 1, 0, cg - 1), (0, 0, cg), (B - 1, HW - 1, (G - 1) * cg), (0, HW // 2, cg * (G // 2) + 4 * (cg > 4))]
    for edge in (GN_CHUNK, GN_APPLY_CHUNK, 1024):
        if HW > edge:
            pts += [(0, edge - 1, 3), (B - 1, edge, C - 2)]
    if HW > 64 * GN_CHUNK:
        pts += [(0, 64 * GN_CHUNK, 1), (0, 64 * GN_CHUNK + GN_CHUNK - 1, C - 1)]
    if Ca is not None:
        pts += [(b, p, ch) for b in (0, B - 1) for p in (0, HW - 1) for ch in (Ca - 1, Ca)]
    return list(dict.fromkeys(pts))


def _gn_like(c, tier, B, HW, C, G, seed, bmod=None, Ca=None):
    kind = c.args.get("kind")
    cg = C // G
    if tier == "R":
        idx = _ma_index(B, G)
        if bmod:  # two sources: a set's (m, a) must be the same wherever a modulo-read sample is shared
            idx = idx[torch.arange(B) % bmod]
        return idx
    if kind == "small":
        return torch.where(torch.rand(B, HW, C, generator=torch.Generator().manual_seed(seed)) < 0.5, -1.0, 1.0) * 2.0 ** -6
    if kind == "flat":
        lvl = 1.0 + ((torch.arange(B)[:, None] + torch.arange(G)[None, :]) % 2).float()  # [B, G]
        return lvl[:, None, :, None].expand(B, HW, G, cg).reshape(B, HW, C).contiguous()
    return _spiked((B, HW, C), _gn_spikes(B, HW, C, G, Ca), seed, G)


def _dy(shape, seed, spikes):
    g = torch.Generator().manual_seed(seed)
    dy = torch.randint(-3, 4, shape, generator=g).float()
    for i, idx in enumerate(spikes):
        dy[idx] = SPIKE if i % 2 == 0 else -SPIKE
    return dy


@functools.lru_cache(maxsize=2)
def build(name, tier):
    """operands and fp64 reference of a case: the same for every storage type.  Tier "S" = tier R run with SiLU."""
    c = BY_NAME[name]
    a, op = c.args, c.op
    silu = tier == "S"
    t = "R" if silu else tier
    eps = a.get("eps", 1e-5)
    xa = xb = dy = y = None
    if op in ("ln", "rms", "l2", "ln_bwd", "rp_ln", "fold_ln"):
        G, C = None, a["C"]
        x = _ln_like(c, t)
    elif op in ("gn", "gn_bwd"):
        B, HW, C, G = a["B"], a["HW"], a["C"], a["G"]
        r = _gn_like(c, t, B, HW, C, G, _seed(name, 1))
        x = from_sets(tier_r_sets(r.reshape(-1), HW * (C // G), _seed(name, 2)), (B, HW, C), G) if t == "R" else r
    else:
        assert op == "gn2"
        B, Ba, Bb, HW, Ca, Cb, G = a["B"], a["Ba"], a["Bb"], a["HW"], a["Ca"], a["Cb"], a["G"]
        C, cg = Ca + Cb, (Ca + Cb) // G
        if t == "R":
            # every 4-channel column block of a sample is balanced on its own, so a set is balanced however the sources' samples are paired
            idx = _gn_like(c, t, B, HW, C, G, 0, bmod=min(Ba, Bb))  # [B, G]
            per4 = idx[:, :, None].expand(B, G, cg // 4).reshape(B, C // 4)  # the (m, a) of every 4-channel block
            blocks = tier_r_sets(per4.reshape(-1), HW * 4, _seed(name, 2)).reshape(B, C // 4, HW, 4)
            full = blocks.permute(0, 2, 1, 3).reshape(B, HW, C)
            xa, xb = full[:Ba, :, :Ca].contiguous(), full[:Bb, :, Ca:].contiguous()
        else:
            full = _gn_like(c, t, max(Ba, Bb), HW, C, G, _seed(name, 1), Ca=Ca)
            xa, xb = full[:Ba, :, :Ca].contiguous(), full[:Bb, :, Ca:].contiguous()
        x = torch.cat([xa.repeat(B // Ba, 1, 1), xb.repeat(B // Bb, 1, 1)], -1)
    if op == "l2":
        gamma = beta = None
        eps = 1e-12
    else:
        gamma, beta = gamma_beta(C, t, _seed(name, 3))
        if op == "rms":
            beta = None
    shape = x.shape
    if op in ("ln_bwd", "gn_bwd"):
        lead = tuple(s - 1 for s in shape)
        dy = _dy(shape, _seed(name, 4), [lead, tuple(0 for _ in shape), lead[:-1] + (0,), (0,) * (len(shape) - 1) + (shape[-1] - 1,)])
        s = to_sets(x.double(), G)
        mean, var = s.mean(1), s.var(1, unbiased=False)
        rstd = 1.0 / (var + eps).sqrt()
        xh = (s - mean[:, None]) * rstd[:, None]
        gg = to_sets(dy.double() * gamma.double(), G)
        sg, sgx = gg.mean(1, keepdim=True), (gg * xh).mean(1, keepdim=True)
        ref = from_sets(rstd[:, None] * (gg - sg - xh * sgx), shape, G)
        absref = from_sets(rstd[:, None] * (gg.abs() + sg.abs() + sgx.abs()), shape, G)
    elif op == "fold_ln":
        from util import int_operand
        ref, absref, mean, var = norm64(x, G, gamma, beta, eps)
        w, wb = int_operand(a["N"], C, amp=1, seed=_seed(name, 5)), int_operand(a["N"], amp=8, seed=_seed(name, 6))
        return Built(x, None, None, gamma, beta, None, eps, G, ref @ w.double().t() + wb.double(),
                     (ref - beta.double()).abs() @ w.double().abs().t() + beta.double().abs() @ w.double().abs().t() + wb.double().abs(), None,
                     to_sets(x, G), mean, var, w, wb, None)
    elif op == "rp_ln":
        from util import int_operand
        _, _, mean, var = norm64(x, G, gamma, beta, eps)
        xn = torch.sign(x.double() - mean[:, None]) * gamma.double() + beta.double()
        w, wb = int_operand(a["N"], C, amp=1, seed=_seed(name, 5)), int_operand(a["N"], amp=8, seed=_seed(name, 6))
        y = xn @ w.double().t() + wb.double()
        return Built(x, None, None, gamma, beta, None, eps, G, y, xn.abs() @ w.double().abs().t() + wb.double().abs(), y, to_sets(x, G), mean, var, w, wb, xn)
    else:
        ref, absref, mean, var = norm64(x, G, gamma, beta, eps, rms=op == "rms", l2=op == "l2")
        if t == "R" and not (op == "l2" and C != 256):
            sg = from_sets(torch.sign(to_sets(x, G) - mean.float()[:, None]), shape, G).double()
            y = sg / 16.0 if op == "l2" else sg * gamma.double() + (0.0 if beta is None else beta.double())
        if silu:
            ref, absref = silu64(y), silu64(y).abs() + y.abs()
    return Built(x, xa, xb, gamma, beta, dy, eps, G, ref, absref, y, to_sets(x, G), mean, var)


def _c(name, op, form, tiers="RK", dtypes=DALL, **args):
    return Case(name, op, form, args, tiers, dtypes)


def _ln_cases():
    out = []
    for C in (8, 256, 520, 1024, 1032, 2048):
        form = "nv1" if C <= 512 else "nv2" if C <= 1024 else "nv4"
        for M in (1, 5, 130):
            out.append(_c(f"ln_C{C}_M{M}", "ln", form, C=C, M=M, eps=1e-5 if M != 5 else 1e-6))
    out += [_c(f"ln_f32tail_C260_M{M}", "ln", "f32_tail", dtypes=("f32",), C=260, M=M) for M in (1, 5, 130)]
    out += [_c("ln_small_C520", "ln", "nv2", "K", C=520, M=5, kind="small"), _c("ln_flat_C520", "ln", "nv2", "K", C=520, M=5, kind="flat"),
            _c("ln_small_C264", "ln", "nv1", "K", C=264, M=5, kind="small")]
    return out


def _gn(name, form, tiers="RSK", dtypes=DALL, B=3, **args):
    return _c(name, "gn", form, tiers, dtypes, B=B, **args)


CASES = _ln_cases() + [
    # ---- one-pass, full-line form for 8-channel groups (C = 64, G = 8 has cg = 8 and G % 8 == 0: gn_onepass_launch takes the full-line form first)
    *[_gn(f"gn_full8_C64_HW{HW}", "full8", C=64, G=8, HW=HW) for HW in (1, 63, 64)],
    *[_gn(f"gn_full8_C256_HW{HW}", "full8", C=256, G=32, HW=HW, eps=1e-6) for HW in (1, 1000, 1024)],
    *[_gn(f"gn_full4_C128_HW{HW}", "full4", C=128, G=32, HW=HW) for HW in (1, 1000)],
    # ---- one-pass, default form, 256 threads: 16-channel groups, and 8-channel groups whose count is no multiple of 8
    *[_gn(f"gn_onepass256_C64G4_HW{HW}", "onepass256", C=64, G=4, HW=HW) for HW in (1, 63, 64)],
    _gn("gn_onepass256_C96G12_HW65", "onepass256", C=96, G=12, HW=65, eps=1e-6),
    _gn("gn_onepass256_C640_HW600", "onepass256", C=640, G=32, HW=600),  # the last HW the 256-thread form accepts at cg = 20 (25 pixel lanes x 24)
    # ---- one-pass, 1024 threads: cg = 20 -> vps = 10: ceil(HW / 25) > 24 from HW = 601, ceil(HW / 102) <= 12 up to 1024
    _gn("gn_onepass1024_C640_HW601", "onepass1024", C=640, G=32, HW=601),
    _gn("gn_onepass1024_C640_HW1024", "onepass1024", C=640, G=32, HW=1024, eps=1e-6),
    # ---- HW <= 1024 that neither one-pass form accepts (cg = 40: 12 and 51 pixel lanes) -> two passes, generic apply loop
    _gn("gn_twopass_C1280_HW1000", "twopass_generic", C=1280, G=32, HW=1000),
    # ---- two passes, HW = 1025: 17 partial chunks, a one-pixel tail in gn_partial_kernel and in the 256-pixel apply chunk
    _gn("gn_twopass_C128_HW1025", "twopass_fast", C=128, G=32, HW=1025),
    _gn("gn_twopass_C384_HW1025", "twopass_generic", C=384, G=32, HW=1025, eps=1e-6),
    # ---- more than 64 chunks: gn_finalize_kernel's k += 64 loop takes a second trip (66 chunks; spikes in chunk 64 and in the last pixel)
    _gn("gn_twopass_66chunks", "twopass_fast_65", B=1, C=32, G=8, HW=4161),
    # ---- small variance and flat, one-pass and two-pass
    _gn("gn_small_onepass", "onepass256", "K", C=64, G=4, HW=63, kind="small"), _gn("gn_flat_onepass", "onepass256", "K", C=64, G=4, HW=63, kind="flat"),
    _gn("gn_small_full8", "full8", "K", C=256, G=32, HW=100, kind="small"), _gn("gn_flat_full8", "full8", "K", C=256, G=32, HW=100, kind="flat"),
    _gn("gn_small_twopass", "twopass_fast", "K", C=128, G=32, HW=1025, kind="small"), _gn("gn_flat_twopass", "twopass_fast", "K", C=128, G=32, HW=1025, kind="flat"),
    # ---- two sources: 640 = 384 + 256 channels in 32 groups of 20: group 19 straddles the boundary; each source read modulo once
    *[_c(f"gn2_HW{HW}_Ba{Ba}_Bb{Bb}", "gn2", form, "RSK", D16, B=4, Ba=Ba, Bb=Bb, HW=HW, Ca=384, Cb=256, G=32)
      for HW, form in ((64, "onepass256"), (1025, "twopass_generic")) for Ba, Bb in ((4, 2), (2, 4))],
    # ---- T5LayerNorm and F.normalize: one wave per row, c += 64
    *[_c(f"rms_C{C}_M{M}", "rms", "wave_row", C=C, M=M, eps=1e-6 if M == 1 else 1e-5) for C in (256, 264) for M in (1, 5)],
    _c("rms_small_C264", "rms", "wave_row", "K", C=264, M=5, kind="small"),
    _c("rms_flat_C264", "rms", "wave_row", "K", C=264, M=5, kind="flat"),  # rows of 1 or 2: gamma k / sqrt(k^2 + eps)
    _c("l2_small_C264", "l2", "wave_row", "K", C=264, M=5, kind="small"), _c("l2_flat_C264", "l2", "wave_row", "K", C=264, M=5, kind="flat"),
    *[_c(f"l2_C{C}_M{M}", "l2", "wave_row", C=C, M=M) for C in (256, 264) for M in (1, 5)],
    # ---- LayerNorm inside the row-panel GEMM: M = 5, 33 and 130 end inside a row tile
    *[_c(f"rp_ln_K{K}_M{M}_N{N}", "rp_ln", "rowpanel", "R", D16, C=K, M=M, N=N, eps=eps)
      for K, M, N, eps in ((256, 130, 128, 1e-5), (256, 5, 64, 1e-6), (384, 33, 192, 1e-5), (384, 130, 64, 1e-6))],
    # ---- LayerNorm folded into apad_gemm at K = 640, behind a producer that emits the row statistics
    *[_c(f"fold_ln_K640_M{M}_N{N}", "fold_ln", "folded", "R", D16, C=640, M=M, N=N, eps=eps) for M, N, eps in ((130, 128, 1e-5), (5, 640, 1e-6))],
    # ---- backward: tier R x, integer dy with spikes
    *[_c(f"ln_bwd_C{C}", "ln_bwd", "ln_bwd", "R", C=C, M=5) for C in (8, 520, 1280)],
    *[_c(f"gn_bwd_C{C}_HW{HW}", "gn_bwd", "gn_bwd", "R", B=2, C=C, G=G, HW=HW) for C, G in ((32, 8), (640, 32)) for HW in (1, 65)],
]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def params():
    """(case name, tier, dtype name): the dtypes of a (case, tier) together, so that build()'s cache serves them"""
    return [(c.name, t, d) for c in CASES for t in c.tiers for d in c.dtypes]


def expected(name, tier, dtype):
    """(fp64 value the final rounding sees, fp64 magnitude A) of a case in ``dtype``.  Tier "S" in fp32: the kernel does not round the normalised value
    (csrc/f32_ops.hip, groupnorm_f32_kernel: ``f4 y = (v - mean) * rstd * gm + bt;`` then ``y[e] = silu_p(y[e])``), so the reference is silu64 of the
    fp64 normalisation y.  The pre-activation error, at most 16 u A_pre, passes through silu, whose derivative lies in [-0.1, 1.1]; silu_p itself
    (``x / (1.0f + expf(-x))``: expf 1 - 2 ulp, an add, a divide) is a few u of |silu(y)| + |y| as in the 16-bit modes.  Hence the same 16 with
    A = 1.1 A_pre + |silu(y)| + |y|."""
    bt = build(name, tier)
    if tier == "S" and dtype == torch.float32:
        y, a_pre, _, _ = norm64(bt.x, bt.groups, bt.gamma, bt.beta, bt.eps)
        return silu64(y), 1.1 * a_pre + silu64(y).abs() + y.abs()
    return bt.ref, bt.absref


SHIFTED_ADDS_MAX = 160


def shifted_adds(c, dtype):
    """additions per thread in the sum of squared deviations of the shifted-form kernel the case runs in ``dtype`` (module docstring), or 0 where the
    kernel uses E[x^2] - mean^2 with exact sums.  LayerNorm: a wave per row in every mode (8-element vectors, 16-bit: C / 64; fp32: 4-element vectors,
    the same count); GroupNorm: only the fp32 kernel, 256 threads per slab"""
    a = c.args
    if c.op == "ln":
        return -(-a["C"] // 64)
    if c.op == "gn" and dtype == torch.float32:
        return -(-(a["HW"] * (a["C"] // a["G"])) // 256)
    return 0


def expects_bits(c, tier, dtype):
    """tier R in a 16-bit mode: the output is the dyadic value in every bit; F.normalize of a +-a row of 256 channels also in fp32 (every step exact)"""
    if tier != "R" or c.op in ("ln_bwd", "gn_bwd", "fold_ln"):
        return False
    if c.op == "l2":
        return c.args["C"] == 256
    return dtype != torch.float32


def check_route(c, dtype):
    """the case lands on the kernel form it is named after (``form`` names the 16-bit form; the fp32 entries have one kernel per operation)"""
    r = route_of(c.op, c.args, dtype != torch.float32)
    if dtype == torch.float32 and c.op in ("ln", "gn"):
        assert r == (c.form if c.form.startswith("f32") else "f32_tail" if c.op == "ln" and c.args["C"] % 256 else "f32"), (c.name, r)
    else:
        assert r == c.form, f"{c.name}: dispatched to {r}, named after {c.form}"
    return r
