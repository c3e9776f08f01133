"""The case table of the saturated-activation tests: tests/test_act_exact_host.py builds every case's operands and fp64 reference on the CPU and
asserts the conditions of its tier; tests/test_gpu_exact_activation.py runs the same cases through the public ``ops`` wrappers.

The activations of the library are exact where they saturate (the code: csrc/common.h gelu_erf_2 / erf_as / silu_f, csrc/mlp3_shared.h M3GegluT,
csrc/f32_ops.hip gelu_p / gelu_tanh_p / silu_p, csrc/train_ops.hip geglu_bwd_kernel):
  GELU   r = fma(p t, -e, 1) with e = exp2(-0.7213 g^2): for |g| >= 6 p t e < 2^-25 and r == 1.0f, so hx + |hx| r is g (g > 0) or +-0 (g < 0), and
         fma(0, r, 0) = 0 at g = 0; 0.5 x (1 + erf) of gelu_erf_f / gelu_p and the tanh form saturate the same way.  Gate classes: {0} u +-[16, 32].
  SiLU   1 + exp2(-1.44 x) == 1 from x = 32 (the result is x); the exponential overflows to inf from x = -112 down (the result is -0).  Classes
         {0} u [32, 256] u [-256, -112]  (at -104 the fp32 result is still a non-zero subnormal).
  tanh   +-1 from |x| = 16; classes as GELU.
  GEGLU backward: for |g| >= 16 cdf is 1 or 0 and pdf underflows to 0: dvalue = dh g or 0, dgate = dh v or 0; at g = 0 (cdf 1/2) dgate = dh v / 2.

Tier Z (bits).  The operand of the first GEMM is a TWO-VALUED matrix: y[t, c] = beta_c + s[t, c] gamma_c with random signs s.  Without a LayerNorm
  x = y with gamma_c in {1, 3}, beta = 0 (odd integers).  With one, x holds tier-R rows of norm_exact_cases.py (m - a, m + a in equal numbers: mean m,
  variance a^2) whose 16-bit normalised value is s gamma + beta in every bit; (gamma, beta) from tier R's own pair list, restricted to 8 |gamma| in
  {1, 3}, |gamma| + |beta| <= 3/8 (LN_PAIRS), weights multiples of 8: Y = 8 y = 8 beta + s o is an integer with o = 8 gamma odd, |Y| <= 3.
  gate rows: a recipe (b, (G_1 .. G_k)) on k columns with |o| = 1 gives gate = b + sum_i G_i s_i: every sign combination lies in the activation's
    classes and all three classes occur (RECIPES; b = 0 recipes where b1 is absent and behind the LayerNorm the 640-wide GEMM applies by algebra,
    whose rstd multiplies after the sum: only an exact 0 stays 0).  The sign of a unit's gate therefore depends on the token.
  value rows: +-1 (times 8 behind a LayerNorm) on two columns and a bias of +-1 (one column where b1 is absent): v is ODD, |v| <= 7 -- never zero, and
    the bf16 packers' halved value rows (apad_mlp_pack, apad_geglu_pack) hold real halves.
  anchors: in every 16-unit chunk a group of units shares its columns with the sign patterns of the recipe arranged so that for every token at least
    one of them is positive and one is not: no 16-unit chunk of any token has a constant hidden activation.
  second GEMM: W2 has up to three +-1 per output row (thinned per row until every stage below stays within 256), b2 in [-8, 8], residual x.
  Every value, hidden activation (|v g| <= 7 * 32), stage (h W2^T, + b2, + x) and output is an integer of at most 256: exact in bf16, f16 and fp32,
  not a rounding tie, so the hand-over rounding of h and the epilogue's order cannot matter.  Expected: util.rne of the fp64 reference; a zero of
  either sign equals zero (the launch adds +0.0), every other element is compared with util.assert_bits_equal.
  The first eight tokens follow a sign schedule (two_valued) under which the columns of a gate row run through all 2^k sign combinations, so from
  8 tokens up each hidden unit meets all three gate classes across the tokens of its case (asserted per unit); a case of fewer tokens (M = 1, 5)
  must show all three classes across its units.  The later tokens keep random signs.

Tier G (bound).  Gates on the half-integer grid in [-5.5, 5.5], integer |v| <= 8, pre-activations exact: x rows are +-one-hot (they select a column of
  W1; behind a LayerNorm tier-R rows, gate and value rows non-zero in one column).  For out = v gelu(g):
      |out - ref64| <= 0.5 ulp_T(ref64) + |v| (|g| / 2 E + C_G 2^-24 |gelu64(g)|),     E = 1.5e-7 + C_E 2^-24 (A&S 7.1.26), 6 * 2^-24 (erff: 2 ulp of libm = 4 u, the
      rounded 1 / sqrt 2 and the product through erf' x <= 0.48: 1 u), 8 * 2^-24 (the tanh form: tanhf 4 u, its argument's five roundings through tanh' x <= 0.45: 2.3 u).
  C_E, in u = 2^-24 (one fp32 rounding; v_rcp_f32 and v_exp_f32 at 1 ulp = 2 u), counted on gelu_erf_2's order for the absolute error of
  r = fma(p t, -e, 1) beyond the 1.5e-7 of the approximation (common.h cites it):
      t = rcp(fma(|z|, P1, 1)), z = x K1:  K1 and P1 rounded (1 u each), the product (1 u), the fma (1 u), rcp (2 u): relative error of t at most
          (3 (1 - t) + 3) u; it reaches r through |d(P(t) t)/dt t| e = |sum_k k a_k t^k| e, whose product with (3 (1 - t) + 3) stays below 12 over
          x >= 0 (test_act_exact_host.py evaluates it on a fine grid)                                                             12 u
      the four Horner fmas, intermediates at most 1.46, 1.43, 0.75, 1.0                                                           4.6 u
      the five rounded coefficients (sum of magnitudes 4.47)                                                                      4.5 u
      p * t                                                                                                                       1 u
      e = exp2(-z z): z z carries 5 u relative, times q e ln 2 <= 0.37: 1.9 u, exp2 itself 2 u                                      4 u
      the last fma                                                                                                                1 u
  27.1 u derived: C_E = 28.  erf_as / gelu_erf_f (ops.geglu, ops.geglu_bwd, the GELU epilogues) scale the argument in two steps (x / sqrt 2, then
  -log2(e) ax ax: 7 u on the exponent where gelu_erf_2 has 5, times 0.37): C_E_F = 29.  C_G = 3: hx = x / 2 is exact; gelu_erf_2: the fma hx + |hx| r (1 u) and the product with v (1 u); gelu_erf_f: (1 + erf) (1 u),
  the product with 0.5 x (1 u), the product with v (1 u).  The half ulp is the store's rounding.  Nothing here was read off a kernel's output; the
  host test evaluates gelu_erf_2's order in fp32 with exactly rounded rcp and exp2 against the bound and asserts that the bound separates the erf
  form from the tanh form on the grid in f16 and fp32.
  The fused feed-forward in tier G: W2 is a signed selection (one +-2^k per output row), out = x + 2^k s h + b2.  The kernels hand h to the second
  GEMM through LDS ROUNDED TO THE STORAGE TYPE (mlp.hip / mlp3.hip; hs_geglu stores it): the reference keeps h in fp64 and the bound gains
  2^k (0.5 ulp_T(h) + the GEGLU term).  The epilogue of these kernels is the library's two-step one (mlp.hip: ``y[0] = (typename E::elem)(yacc[ct][4 * g + 0]
  + b4.x);`` then scratch_flush adds x; hsattn.hip, hs_ff2: "bias, rounding, + residual"): out = rne(rne(h W2^T + b2) + x), so the first rounding's
  0.5 ulp_T(h W2^T + b2) is part of the bound as well (where x cancels most of it, it is the larger term).
  Backward (ops.geglu_bwd): dvalue = dh gelu(g): the forward bound with dh for v; dgate = dh v D(g), D = cdf + g pdf:
      |dgate - ref64| <= 0.5 ulp_T(ref64) + |dh v| (E / 2 + C_D 2^-24 (D64(g) + 1)),  C_D = 8: cdf = 0.5 (1 + erf) carries E / 2; pdf: the constant,
      two products in the exponent (3 u of q <= 22 where pdf q |g| <= 0.6: 2 u absolute), exp 2 u, the product with g and the sum 2 u, two products
      with dh and v 2 u: 8 u of D + 1.

``route`` restates the dispatch conditions of each kernel form ON THE SHAPE; both test files assert it for every case.  It does not observe which
kernel ran: launch_ring, for one, falls back to the tiled kernel where it declines a launch, and the two are bit-equal by construction (the same
limitation as the route check of test_gpu_exact_linear.py)."""
import functools
import math
import zlib
from collections import namedtuple

import torch

import norm_exact_cases as NC
from util import int_operand, ulp_of

MODES = {"bf16": torch.bfloat16, "f16": torch.float16, "highest": torch.float32, "high": torch.float32}
M16 = ("bf16", "f16")
ALL = M16 + ("highest", "high")
U = 2.0 ** -24
C_E, C_E_F, C_G, C_D = 28.0, 29.0, 3.0, 8.0
E_AS = 1.5e-7 + C_E * U      # gelu_erf_2 / M3GegluT
E_AS_F = 1.5e-7 + C_E_F * U  # erf_as / gelu_erf_f
E_ERFF = 6.0 * U
E_TANH = 8.0 * U
AS_P, AS_A = 0.3275911, (0.254829592, -0.284496736, 1.421413741, -1.453152027, 1.061405429)

Case = namedtuple("Case", "name op args tiers modes")
W1 = namedtuple("W1", "x ln w1 b1 y v g S")  # operands (fp32 CPU) and fp64 pre-activations: v [M, H] (None: no value half), g [M, H]


def _seed(name, i=0):
    return (zlib.crc32(name.encode()) + 7919 * i) % (2 ** 31)


# ---- activations in fp64 and their classes
def gelu64(g):
    return 0.5 * g * (1.0 + torch.erf(g / math.sqrt(2.0)))


def gelu_tanh64(g):
    return 0.5 * g * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (g + 0.044715 * g ** 3)))


def silu64(x):
    return x * torch.sigmoid(x)


def dgelu64(g):
    """cdf + g pdf"""
    return 0.5 * (1.0 + torch.erf(g / math.sqrt(2.0))) + g * torch.exp(-0.5 * g * g) / math.sqrt(2.0 * math.pi)


ACT64 = {"gelu": gelu64, "geglu": gelu64, "gelu_tanh": gelu_tanh64, "geglu_tanh": gelu_tanh64, "silu": silu64, "tanh": torch.tanh}
GATED = ("geglu", "geglu_tanh")


def classes(act):
    """(lo, hi) of the positive class and of the negative class (as magnitudes); 0 is the third"""
    return ((32, 256), (112, 256)) if act == "silu" else ((16, 32), (16, 32))


def class_of(g, act):
    """fp64 gates -> 0 (zero), 1 (positive class), -1 (negative class), 9 (outside every class)"""
    (pl, ph), (nl, nh) = classes(act)
    out = torch.full(g.shape, 9, dtype=torch.int64)
    out[g == 0] = 0
    out[(g >= pl) & (g <= ph)] = 1
    out[(g <= -nl) & (g >= -nh)] = -1
    return out


def saturated(g, act):
    """what the activation is on a saturated gate, exactly: g (tanh: 1) on the positive class, 0 on zero, 0 (tanh: -1) on the negative class"""
    c = class_of(g, act)
    assert int((c == 9).sum()) == 0
    if act == "tanh":
        return c.double()
    return torch.where(c == 1, g, torch.zeros_like(g))


# ---- recipes: (b, (G_1 .. G_k)); a unit's gate is b + sum_i sigma_i G_i s_i over its k columns.  ANCHORS: the sign patterns sigma of the units that
# share a column set, chosen so that every token finds one of them positive and one of them not (asserted by the host test on every combination)
RECIPES = {
    ("gelu", True): [(8, (8, 8, 8)), (8, (16, 8)), (-8, (8, 8, 8)), (0, (16, 8, 8))],
    ("gelu", False): [(0, (16, 8, 8))],
    ("silu", True): [(16, (56, 72)), (0, (112, 56, 56))],
    ("silu", False): [(0, (112, 56, 56))],
}
ANCHOR = {
    ("gelu", True): ((8, (8, 8, 8)), ((1, 1, 1), (-1, -1, -1))),  # gate and 16 - gate
    ("gelu", False): ((0, (16, 8, 8)), ((1, 1, 1), (-1, 1, 1), (1, -1, -1), (-1, -1, -1))),
    ("silu", True): ((0, (112, 56, 56)), ((1, 1, 1), (-1, 1, 1), (1, -1, -1), (-1, -1, -1))),
    ("silu", False): ((0, (112, 56, 56)), ((1, 1, 1), (-1, 1, 1), (1, -1, -1), (-1, -1, -1))),
}


def _kind(act):
    return "silu" if act == "silu" else "gelu"


def recipe_values(b, G, sigma=None):
    """the gate of every sign combination of the columns: [2^k]"""
    k = len(G)
    sg = torch.tensor([[1.0 if (i >> j) & 1 else -1.0 for j in range(k)] for i in range(2 ** k)], dtype=torch.float64)
    Gs = torch.tensor(G, dtype=torch.float64) * (1.0 if sigma is None else torch.tensor(sigma, dtype=torch.float64))
    return b + sg @ Gs


# ---- the two-valued operand
@functools.lru_cache(maxsize=None)
def ln_pairs(beta_zero):
    """tier R's (gamma, beta) pairs with 8 |gamma| in {1, 3} and |gamma| + |beta| <= 3 / 8 (beta_zero: beta = 0 only)"""
    out = [(g, b) for g, b in NC._pairs("R") if abs(8 * g) in (1.0, 3.0) and abs(g) + abs(b) <= 0.375 and not (beta_zero and b != 0)]
    assert {abs(8 * g) for g, _ in out} == {1.0, 3.0} and len(out) == (4 if beta_zero else 8), out
    return out


def sched_bit(c, K):
    """the bit of the token schedule a column carries (columns c and c + K / 2 the same)"""
    return (c % (K // 2 if K % 2 == 0 else K)) % 3


def two_valued(M, K, ln, seed, beta_zero=False, onehot=False):
    """-> (x [M, K] fp32, ln = (gamma, beta, eps) | None, Y [M, K] fp64 = S y (integers), S, o [K] = S gamma (odd), sb [K] = S beta).
    onehot (tier G without a LayerNorm): x rows are +-one-hot instead (Y = x, S = 1; o, sb unused)"""
    g = torch.Generator().manual_seed(seed)
    # the first eight tokens follow a schedule: column c carries bit sched_bit(c, K) of (t + phase_c), so any three columns of different bits run through
    # all eight sign combinations there (bit 0 alternates, bit 1 has period 4, bit 2 period 8), whatever the phases; column c + K / 2 carries the
    # opposite of column c, which keeps a LayerNorm row balanced.  The later tokens keep random signs.
    half = K // 2 if K % 2 == 0 else K
    phase, r = torch.randint(0, 8, (half,), generator=g), torch.where(torch.rand(half, generator=g) < 0.5, -1.0, 1.0)
    cc = torch.arange(K)
    sched = 1.0 - 2.0 * (((torch.arange(8)[:, None] + phase[cc % half][None, :]) >> sched_bit(cc, K)[None, :]) & 1).float()
    sched = sched * (r[cc % half] * torch.where(cc >= half, -1.0, 1.0))[None, :]  # [8, K]
    if onehot:
        assert not ln
        col = torch.randint(0, K, (M,), generator=g)
        col[:min(M, K)] = torch.randperm(K, generator=g)[:min(M, K)]  # every column once where there are tokens enough
        col[-1] = K - 1  # the last token selects the last column (the K tail)
        sg = torch.where(torch.rand(M, generator=g) < 0.5, -1.0, 1.0)
        x = torch.zeros(M, K)
        x[torch.arange(M), col] = sg
        return x, None, x.double(), 1.0, None, None
    if not ln:
        o = torch.where(torch.rand(K, generator=g) < 0.34, 3.0, 1.0)
        s = torch.where(torch.rand(M, K, generator=g) < 0.5, -1.0, 1.0)
        s[:8] = sched[:M]
        x = s * o
        return x, None, x.double(), 1.0, o.double(), torch.zeros(K, dtype=torch.float64)
    assert K % 2 == 0
    p = torch.tensor(ln_pairs(beta_zero))
    p = p[torch.randint(0, p.shape[0], (K,), generator=g)]
    gamma, beta = p[:, 0].float().contiguous(), p[:, 1].float().contiguous()
    x = NC.tier_r_sets(NC._ma_index(M, 1).reshape(-1), K, seed + 1).reshape(M, K)
    m = x.mean(1, keepdim=True)  # (exact: m - a and m + a in equal numbers)
    a, s = (x - m).abs(), torch.sign(x - m)
    s[:8] = sched[:M]
    x = m + s * a
    s = s.double()
    o, sb = 8.0 * gamma.double(), 8.0 * beta.double()
    return x, (gamma, beta, 1e-5 if seed % 2 else 1e-6), sb + s * o, 8.0, o, sb


def build_w1(M, K, H, act, tier, ln, bias, seed, gate_b0=False, ln_fold=False):
    """the first GEMM of a case: x [M, K], W1 [(2) H, K] (value rows, then gate rows, where ``act`` is gated), b1 | None, and the fp64
    pre-activations.  gate_b0: only recipes with b = 0.  Tier Z and tier G as the module docstring describes."""
    gated = act in GATED
    g = torch.Generator().manual_seed(seed + 11)
    if tier == "G":
        x, lnp, Y, S, o, sb = two_valued(M, K, ln, seed, onehot=not ln)
        if not ln:  # dense grids: a +-one-hot row selects +-column + bias
            wg = torch.randint(-6, 7, (H, K), generator=g).double() / 2.0
            bg = torch.randint(-5, 6, (H,), generator=g).double() / 2.0 if bias else torch.zeros(H, dtype=torch.float64)
            if not bias:
                wg = torch.randint(-11, 12, (H, K), generator=g).double() / 2.0
            wv = torch.randint(-5, 6, (H, K), generator=g).double()
            bv = torch.randint(-3, 4, (H,), generator=g).double() if bias else torch.zeros(H, dtype=torch.float64)
            if not bias:
                wv = torch.randint(-8, 9, (H, K), generator=g).double()
        else:  # one column per row: gate j Y / 2 (+ half-integer bias), value omega Y (+ bias)
            cg, cv = torch.randint(0, K, (H,), generator=g), torch.randint(0, K, (H,), generator=g)
            j = torch.randint(1, 4, (H,), generator=g).double() * torch.where(torch.rand(H, generator=g) < 0.5, -1.0, 1.0)
            om = torch.randint(1, 3, (H,), generator=g).double() * torch.where(torch.rand(H, generator=g) < 0.5, -1.0, 1.0)
            wg, wv = torch.zeros(H, K, dtype=torch.float64), torch.zeros(H, K, dtype=torch.float64)
            wg[torch.arange(H), cg] = 4.0 * j   # 4 j y = j Y / 2
            wv[torch.arange(H), cv] = 8.0 * om  # 8 omega y = omega Y
            bg = torch.randint(-2, 3, (H,), generator=g).double() / 2.0 if bias else torch.zeros(H, dtype=torch.float64)
            bv = torch.randint(-2, 3, (H,), generator=g).double() if bias else torch.zeros(H, dtype=torch.float64)
        y = Y / S
        gate = y @ wg.t() + bg
        val = y @ wv.t() + bv if gated else None
        w1 = torch.cat([wv, wg], 0) if gated else wg
        b1 = (torch.cat([bv, bg]) if gated else bg) if bias else None
        return W1(x, lnp, w1.float(), None if b1 is None else b1.float(), y, val, gate, S)
    assert tier == "Z"
    b0 = gate_b0 or not bias
    x, lnp, Y, S, o, sb = two_valued(M, K, ln, seed, beta_zero=ln and not bias)
    kind = _kind(act)
    recipes = [r for r in RECIPES[(kind, bias)] if not (b0 and r[0] != 0)]
    (ab, aG), asig = ANCHOR[(kind, bias and not b0)]
    unit = torch.nonzero(o.abs() == 1).reshape(-1)  # the columns a gate row may use
    if not bias and ln:
        assert bool((sb == 0).all())
    Og = torch.zeros(H, K, dtype=torch.float64)
    bgt = torch.zeros(H, dtype=torch.float64)  # the recipe's b per unit

    def put(u, cols, b, G, sigma):
        for c, Gi, si in zip(cols, G, sigma):
            Og[u, c] = si * Gi * o[c]  # (o = +-1: its contribution is si Gi (o sb + s))
        bgt[u] = b

    by_bit = [unit[sched_bit(unit, K) == j] for j in range(3)]
    assert all(b.numel() > 0 for b in by_bit)

    def pick(k):  # k columns of different schedule bits
        return [int(by_bit[j][int(torch.randint(0, by_bit[j].numel(), (1,), generator=g))]) for j in torch.randperm(3, generator=g)[:k].tolist()]

    for c0 in range(0, H, 16):
        n = min(16, H - c0)
        pos = (torch.randperm(n, generator=g) + c0).tolist()
        cols = pick(len(aG))
        na = min(len(asig), n)
        for u, sigma in zip(pos[:na], asig[:na]):
            put(u, cols, ab, aG, sigma)
        for u in pos[na:]:
            b, G = recipes[int(torch.randint(0, len(recipes), (1,), generator=g))]
            put(u, pick(len(G)), b, G, torch.where(torch.rand(len(G), generator=g) < 0.5, -1.0, 1.0).tolist())
    # gate = Y Og^T + (b - Og sb): the second term is the gate half of b1 (zero where b1 is absent: b = 0 and sb = 0 on the columns used)
    bg = bgt - Og @ sb
    gate = Y @ Og.t() + bg
    if not bias:
        assert bool((bg == 0).all())
    val = bv = Ov = None
    if gated:
        Ov = torch.zeros(H, K, dtype=torch.float64)
        ncol = 2 if bias else 1
        vc = torch.rand(H, K, generator=g).argsort(1)[:, :ncol]  # ncol different columns per unit
        Ov.scatter_(1, vc, torch.where(torch.rand(H, ncol, generator=g) < 0.5, -1.0, 1.0).double())
        bv = torch.where(torch.rand(H, generator=g) < 0.5, -1.0, 1.0).double() if bias else torch.zeros(H, dtype=torch.float64)
        val = Y @ Ov.t() + bv
    w1 = S * (torch.cat([Ov, Og], 0) if gated else Og)
    b1 = (torch.cat([bv, bg]) if gated else bg) if bias else None
    return W1(x, lnp, w1.float(), None if b1 is None else b1.float(), Y / S, val, gate, S)


def hidden64(w, act):
    """fp64 hidden activation (or plain activation output) of a W1"""
    a = ACT64[act](w.g)
    return a if w.v is None else w.v * a


def hidden_exact(w, act):
    """tier Z: the same, from the classes alone (an integer)"""
    a = saturated(w.g, act)
    return a if w.v is None else w.v * a


def build_w2(h, Cout, res, bias, tier, seed):
    """the second GEMM over h [M, Hh] (fp64): tier Z: up to three +-1 per output row, thinned until h W2^T, + b2, + res stay within 256; tier G: one
    +-2^k per row.  -> (w2 [Cout, Hh] fp32, b2 | None, stages [acc, acc + b2, acc + b2 + res] fp64)"""
    g = torch.Generator().manual_seed(seed + 23)
    M, Hh = h.shape
    b2 = int_operand(Cout, amp=8 if tier == "Z" else 4, seed=seed + 29).double() if bias else torch.zeros(Cout, dtype=torch.float64)
    r = torch.zeros(M, Cout, dtype=torch.float64) if res is None else res.double()
    w2 = torch.zeros(Cout, Hh, dtype=torch.float64)
    cols = torch.stack([torch.randperm(Hh, generator=g)[:3] for _ in range(Cout)])
    cols[-1, 0], cols[0, 0] = Hh - 1, 0
    sg = torch.where(torch.rand(Cout, 3, generator=g) < 0.5, -1.0, 1.0).double()
    if tier == "G":
        k = torch.randint(0, 3, (Cout,), generator=g).double()
        w2[torch.arange(Cout), cols[:, 0]] = sg[:, 0] * torch.exp2(k)
    else:
        keep = torch.full((Cout,), 3)
        for _ in range(3):
            w2.zero_()
            for i in range(3):
                w2[torch.arange(Cout), cols[:, i]] = torch.where(keep > i, sg[:, i], torch.zeros(Cout, dtype=torch.float64))
            acc = h @ w2.t()
            over = torch.stack([acc.abs(), (acc + b2).abs(), (acc + b2 + r).abs(), (acc + r).abs()]).amax((0, 1)) > 256
            if not bool(over.any()):
                break
            keep = torch.where(over, keep - 1, keep)
        assert int(keep.min()) >= 1 and not bool(over.any())
    acc = h @ w2.t()
    return w2.float(), (b2.float() if bias else None), [acc, acc + b2, acc + b2 + r]


# ---- bounds of tier G
def gelu_bound(v, g, dtype, ref=None, erff=False, tanh_form=False, erf_as=False):
    """0.5 ulp_T(ref) + |v| (|g| / 2 E + C_G u |act64(g)|); v None: a plain GELU"""
    v = torch.ones_like(g) if v is None else v
    a = (gelu_tanh64 if tanh_form else gelu64)(g)
    ref = v * a if ref is None else ref
    E = E_TANH if tanh_form else E_ERFF if erff else E_AS_F if erf_as else E_AS
    return 0.5 * ulp_of(ref, dtype) + v.abs() * (g.abs() / 2.0 * E + C_G * U * a.abs()), ref


def dgate_bound(dhv, g, dtype, erff=False):
    ref = dhv * dgelu64(g)
    return 0.5 * ulp_of(ref, dtype) + dhv.abs() * ((E_ERFF if erff else E_AS_F) / 2.0 + C_D * U * (dgelu64(g).abs() + 1.0)), ref


def emulate_gelu_erf_2(g64):
    """gelu_erf_2's operation order in fp32 (every product, fma and sum rounded once; rcp and exp2 exactly rounded) -> fp64 of the fp32 result"""
    f = lambda t: t.float().double()  # one fp32 rounding of an fp64 value (products of two fp32 are exact in fp64)
    K1, P1 = f(torch.tensor(0.84932180028801904272, dtype=torch.float64)), f(torch.tensor(0.2727374808792225, dtype=torch.float64))
    a = [f(torch.tensor(c, dtype=torch.float64)) for c in AS_A]
    x = f(g64)
    z = f(x * K1)
    d = f(z.abs() * P1 + 1.0)
    t = f(1.0 / d)
    p = f(t * a[4] + a[3])
    p = f(p * t + a[2])
    p = f(p * t + a[1])
    p = f(p * t + a[0])
    q = f(z * z)
    e = f(torch.exp2(-q))
    r = f(f(p * t) * -e + 1.0)
    hx = x * 0.5
    return f(hx.abs() * r + hx)


# ---- the cases
def _c(name, op, tiers="Z", modes=M16, **args):
    return Case(name, op, args, tiers, modes)


def _cases():
    out = []
    # ops.linear(act=) on the tiled kernel: the ragged K and N tails; every storage type and both fp32 precisions
    for M, N, K in ((77, 64, 72), (130, 192, 136), (77, 192, 256), (130, 64, 136)):
        for act in ("geglu", "gelu", "silu"):
            out.append(_c(f"linear_{act}_{M}x{N}x{K}", "linear", "ZG" if act != "silu" else "Z", ALL, M=M, N=N, K=K, act=act, bias=True))
    for M in (77, 130):  # the rest of the (M, N, K) grid: GEGLU, tier Z
        for N in (64, 192):
            for K in (72, 136, 256):
                if f"linear_geglu_{M}x{N}x{K}" not in {c.name for c in out}:
                    out.append(_c(f"linear_geglu_{M}x{N}x{K}", "linear", "Z", ALL, M=M, N=N, K=K, act="geglu", bias=True))
    out.append(_c("linear_geglu_nobias_77x64x72", "linear", "ZG", ALL, M=77, N=64, K=72, act="geglu", bias=False))
    # the fp32-only epilogues
    for act in ("tanh", "gelu_tanh", "geglu_tanh"):
        out.append(_c(f"linear_{act}_77x64x72", "linear", "ZG" if act != "tanh" else "Z", ("highest", "high"), M=77, N=64, K=72, act=act, bias=True))
        out.append(_c(f"linear_{act}_130x192x136", "linear", "Z", ("highest",), M=130, N=192, K=136, act=act, bias=True))
    # the LDS-DMA ring form with the GEGLU epilogue
    for M, N, K in ((77, 64, 128), (130, 192, 256)):
        out.append(_c(f"ring_geglu_{M}x{N}x{K}", "linear", "ZG", M16, M=M, N=N, K=K, act="geglu", bias=True, ring=2))
    # LayerNorm by algebra at K = 640 behind a rowstat producer
    out += [_c(f"fold_geglu_M{M}_N{N}", "fold", "Z", M16, M=M, N=N, K=640) for M, N in ((130, 128), (5, 640))]
    # row-panel kernels (rpgemm; wsgemm for GELU / SiLU with N <= 512)
    for K in (256, 384):
        for M in (1, 37, 300):
            for ln in (False, True):
                out.append(_c(f"rp_geglu_K{K}_M{M}_ln{int(ln)}", "fused", "ZG" if M == 37 else "Z", M16, M=M, N=4 * K if M != 300 else 192, K=K, act="geglu", ln=ln, bias=True))
        for act in ("gelu", "silu"):
            out.append(_c(f"rp_{act}_K{K}_M37", "fused", "Z", M16, M=37, N=576, K=K, act=act, ln=True, bias=True))
            out.append(_c(f"ws_{act}_K{K}_M37", "fused", "ZG" if act == "gelu" else "Z", M16, M=37, N=256, K=K, act=act, ln=False, bias=True))
            out.append(_c(f"ws_{act}_K{K}_M300_ln", "fused", "Z", M16, M=300, N=512 if K == 256 else 384, K=K, act=act, ln=True, bias=True))
    out.append(_c("rp_geglu_8wave_K256", "fused", "Z", M16, M=32768 + 37, N=128, K=256, act="geglu", ln=True, bias=True))
    out.append(_c("rp_geglu_nobias_K384_M37", "fused", "Z", M16, M=37, N=192, K=384, act="geglu", ln=True, bias=False))
    # the fused feed-forward at C = 256: 128-token workgroups (geglu_mlp) and 256-token workgroups of 64-token blocks (geglu_mlp_packed)
    for op in ("mlp", "mlp_packed"):
        for M in (1, 37, 63, 65, 127, 129, 255, 257, 300):
            ln, b1, b2 = M % 2 == 1 and M != 63, M not in (65, 255), M not in (127, 255)
            out.append(_c(f"{op}_M{M}", op, "ZG" if M in (37, 257) else "Z", M16, M=M, ln=ln, b1=b1, b2=b2))
        out.append(_c(f"{op}_M130_select", op, "G", M16, M=130, ln=False, b1=True, b2=False))  # x one-hot, no b2: out = +-2^k h off the hot column
        out += [_c(f"{op}_M300_noln", op, "Z", M16, M=300, ln=False, b1=True, b2=True), _c(f"{op}_M63_ln_nob1", op, "Z", M16, M=63, ln=True, b1=False, b2=True)]
    # LayerNorm + GEGLU from packed weights at C = 384
    for M in (1, 63, 255, 257, 300):
        for ln, bias in ((True, True), (False, True), (True, False)):
            out.append(_c(f"lngeglu_M{M}_ln{int(ln)}_b{int(bias)}", "lngeglu", "ZG" if M == 257 and bias else "Z", M16, M=M, ln=ln, bias=bias))
    # the 64-token level: hs_geglu, and hs_geglu + hs_ff2
    for B, N in ((1, 1), (3, 37), (2, 64)):
        for norm in (True, False):
            out.append(_c(f"hs_geglu_B{B}_N{N}_norm{int(norm)}", "hs", "ZG" if (B, N) == (3, 37) and not norm else "Z", M16, B=B, N=N, norm=norm))
        out.append(_c(f"hs_ff_B{B}_N{N}", "hs_ff", "ZG" if N == 37 else "Z", M16, B=B, N=N, norm=True))
    # the stored-projection GEGLU of the training step, forward and backward
    for M, N in ((3, 8), (37, 1024), (257, 2560)):
        out.append(_c(f"geglu_{M}x{N}", "geglu", "ZG", ("bf16", "f16", "highest"), M=M, N=N))
        out.append(_c(f"geglu_bwd_{M}x{N}", "geglu_bwd", "ZG", ("bf16", "f16", "highest"), M=M, N=N))
    # the vocoder's tanh epilogue (16-bit: conv1d only), at the conv1d shapes of exact_cases.py
    out += [_c("conv1d_tanh_k3", "conv1d", "Z", M16, B=2, T=37, Cin=16, Cout=24, taps=3, dil=1), _c("conv1d_tanh_k7_d3", "conv1d", "Z", M16, B=2, T=37, Cin=16, Cout=24, taps=7, dil=3)]
    return out


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
RP_K, HS_C, MLP_C, GEGLU_C = (256, 384), 640, 256, 384


def params(ops_=None, tiers="ZG"):
    return [(c.name, t, m) for c in CASES if ops_ is None or c.op in ops_ for t in c.tiers if t in tiers for m in c.modes]


def route(c, mode):
    """the dispatcher's conditions for the kernel form the case is named after (csrc/gemm.hip launch / launch_ring, apad_rowpanel_gemm and
    apad_ws_dispatch, ops.fused_linear, ops.ln_foldable, the envelopes of the fused kernels), asserted on the shape"""
    a, is16 = c.args, mode in M16
    if c.op == "linear":
        M, N, K = a["M"], a["N"], a["K"]
        assert M < 16000 and ((N + 127) // 128) * ((M + 127) // 128) < 320 and not (K >= 384 and N >= 640)  # the 64-tile kernel, one K group
        if a.get("ring"):
            assert is16 and K >= 128 and K % 64 == 0 and N % 64 == 0  # launch_ring's envelope
        if a["act"] in ("tanh", "gelu_tanh", "geglu_tanh"):
            assert not is16  # fp32-mode epilogues
        return "ring" if a.get("ring") else "tiled" if is16 else "f32"
    if c.op == "fold":
        assert is16 and a["K"] % 64 == 0 and a["K"] not in RP_K and a["N"] % 64 == 0
        return "folded"
    if c.op == "fused":
        assert is16 and a["K"] in RP_K and a["N"] % 64 == 0  # ops.fused_linear's condition for the row-panel launch
        ws = a["act"] not in GATED and a["N"] <= 512 and a["N"] % (256 if a["K"] == 256 else 128) == 0
        assert ws == c.name.startswith("ws_") and (a["M"] >= 32768) == ("8wave" in c.name)
        return "ws" if ws else "rp8" if a["M"] >= 32768 else "rp"
    if c.op in ("mlp", "mlp_packed", "lngeglu", "hs", "hs_ff"):
        assert is16 and (c.op not in ("hs", "hs_ff") or a["N"] <= 64)
        return c.op
    if c.op == "conv1d":
        assert is16
        return "conv1d"
    assert c.op in ("geglu", "geglu_bwd") and a["N"] % 8 == 0
    return c.op


# ---- builders: -> dict(t = operands, ref = fp64 value the final rounding sees, bound = fp64 | None, inter = exact integers (tier Z), gates, hidden)
def _ff(name, tier, C, M, ln, b1, b2, norm_fold=False):
    w = build_w1(M, C, 4 * C, "geglu", tier, ln, b1, _seed(name, 1))
    h = hidden_exact(w, "geglu") if tier == "Z" else hidden64(w, "geglu")
    w2, bb2, st = build_w2(h, C, w.x, b2, tier, _seed(name, 2))
    return w, h, w2, bb2, st


def _g_terms(w, act, dtype, erff, erf_as):
    """tier G: (bound of the hidden activation without its half ulp, h64)"""
    tanh_form = act in ("gelu_tanh", "geglu_tanh")
    b, ref = gelu_bound(w.v, w.g, dtype, erff=erff, tanh_form=tanh_form, erf_as=erf_as)
    return b - 0.5 * ulp_of(ref, dtype), ref


@functools.lru_cache(maxsize=4)
def build(name, tier):
    """operands and fp64 reference of (case, tier): the same for every storage type (the bound is per type: ``expected``)"""
    c = BY_NAME[name]
    a, op = c.args, c.op
    if op in ("linear", "fused", "fold"):
        act = a.get("act", "geglu")
        w = build_w1(a["M"], a["K"], a["N"], act, tier, a.get("ln", op == "fold"), a.get("bias", True), _seed(name, 1), gate_b0=op == "fold")
        return dict(w=w, act=act, ref=hidden_exact(w, act) if tier == "Z" else hidden64(w, act), gates=w.g, hidden=None, inter=[t for t in (w.v, w.g) if t is not None])
    if op in ("mlp", "mlp_packed"):
        w, h, w2, b2, st = _ff(name, tier, MLP_C, a["M"], a["ln"], a["b1"], a["b2"])
        return dict(w=w, act="geglu", w2=w2, b2=b2, ref=st[2], mid=st[1], gates=w.g, hidden=h, inter=[w.v, w.g, h] + st)
    if op == "lngeglu":
        w = build_w1(a["M"], GEGLU_C, 4 * GEGLU_C, "geglu", tier, a["ln"], a["bias"], _seed(name, 1))
        return dict(w=w, act="geglu", ref=hidden_exact(w, "geglu") if tier == "Z" else hidden64(w, "geglu"), gates=w.g, hidden=None, inter=[w.v, w.g])
    if op in ("hs", "hs_ff"):
        M = a["B"] * a["N"]
        if op == "hs":
            w = build_w1(M, HS_C, 4 * HS_C, "geglu", tier, a["norm"], True, _seed(name, 1))
            return dict(w=w, act="geglu", ref=hidden_exact(w, "geglu") if tier == "Z" else hidden64(w, "geglu"), gates=w.g, hidden=None, inter=[w.v, w.g])
        w, h, w2, b2, st = _ff(name, tier, HS_C, M, tier == "Z", True, True)
        return dict(w=w, act="geglu", w2=w2, b2=b2, ref=st[2], mid=st[1], gates=w.g, hidden=h, inter=[w.v, w.g, h] + st)
    if op == "conv1d":
        # unit u reads tap u % taps: its recipe's columns all sit on that tap, so a token whose tap falls into the zero padding has the gate b.  Units
        # on the centre tap (always inside) take any recipe, the others the b = 0 recipes (their edge tokens are the zero class) and a zero bias.
        B, T, Cin, Cout, taps, dil = a["B"], a["T"], a["Cin"], a["Cout"], a["taps"], a["dil"]
        wc = build_w1(B * T, Cin, Cout, "tanh", "Z", False, True, _seed(name, 1))
        w0 = build_w1(B * T, Cin, Cout, "tanh", "Z", False, True, _seed(name, 1), gate_b0=True)  # (the same x: the same seed)
        assert torch.equal(wc.x, w0.x)
        tap = torch.arange(Cout) % taps
        ctr = tap == taps // 2
        wp = torch.zeros(Cout, taps, Cin)
        wp[torch.arange(Cout), tap] = torch.where(ctr[:, None], wc.w1, w0.w1)
        b1 = torch.where(ctr, wc.b1, w0.b1)
        xp = torch.zeros(B, T + 2 * (taps // 2) * dil, Cin, dtype=torch.float64)
        xp[:, (taps // 2) * dil:(taps // 2) * dil + T] = wc.x.double().reshape(B, T, Cin)
        win = torch.stack([xp[:, k * dil:k * dil + T] for k in range(taps)], 2)  # [B, T, taps, Cin]: tap k reads position t + (k - taps // 2) dil
        gate = (torch.einsum("btkc,okc->bto", win, wp.double()) + b1.double()).reshape(B * T, Cout)
        w = W1(wc.x, None, None, b1, None, None, gate, 1.0)
        return dict(w=w, act="tanh", wp=wp.reshape(Cout, taps * Cin), ref=hidden_exact(w, "tanh"), gates=gate, hidden=None, inter=[gate])
    M, N = a["M"], a["N"]
    g = torch.Generator().manual_seed(_seed(name, 1))
    v = torch.randint(-8, 9, (M, N), generator=g).double()
    dh = torch.randint(-8, 9, (M, N), generator=g).double()
    if tier == "Z":
        cls = torch.randint(0, 4, (M, N), generator=g)  # a quarter zero, a quarter negative, half positive
        mag = torch.randint(16, 33, (M, N), generator=g).double()
        gt = torch.where(cls == 0, torch.zeros(M, N, dtype=torch.float64), torch.where(cls == 1, -mag, mag))
    else:
        gt = torch.randint(-11, 12, (M, N), generator=g).double() / 2.0
    w = W1(None, None, None, None, None, v, gt, 1.0)
    proj = torch.cat([v, gt], 1).float()
    if op == "geglu":
        return dict(w=w, act="geglu", proj=proj, ref=hidden_exact(w, "geglu") if tier == "Z" else hidden64(w, "geglu"), gates=gt, hidden=None, inter=[v, gt])
    if tier == "Z":
        c3 = class_of(gt, "geglu")
        dv = torch.where(c3 == 1, dh * gt, torch.zeros_like(gt))
        dg = torch.where(c3 == 1, dh * v, torch.where(c3 == 0, dh * v / 2.0, torch.zeros_like(gt)))
    else:
        dv, dg = dh * gelu64(gt), dh * v * dgelu64(gt)
    return dict(w=w, act="geglu", proj=proj, dh=dh.float(), ref=torch.cat([dv, dg], 1), gates=gt, hidden=None, inter=[v, gt, dh * gt, dh * v])


def expected(name, tier, mode):
    """(fp64 reference, fp64 bound | None (tier Z: bits)) of a case in a mode"""
    bt, c, dtype = build(name, tier), BY_NAME[name], MODES[mode]
    if tier == "Z":
        return bt["ref"], None
    w, act, erff = bt["w"], bt["act"], dtype == torch.float32
    if c.op == "geglu_bwd":
        bv, _ = gelu_bound(bt["dh"].double(), w.g, dtype, erff=erff, erf_as=True)
        bg, _ = dgate_bound(bt["dh"].double() * w.v, w.g, dtype, erff=erff)
        return bt["ref"], torch.cat([bv, bg], 1)
    term, h64 = _g_terms(w, act, dtype, erff, erf_as=act == "gelu" or c.op == "geglu")  # the GELU epilogues and ops.geglu: gelu_erf_f
    if "w2" in bt:  # out = rne(rne(h W2^T + b2) + x), W2 a signed selection: the hand-over rounding of h and the GEGLU term, scaled by |W2|, then
        # the epilogue's two roundings (each half an ulp of the largest value it can see)
        a2 = bt["w2"].double().abs()
        e_h = (0.5 * ulp_of(h64, dtype) + term) @ a2.t()
        e_mid = e_h + 0.5 * ulp_of(bt["mid"].abs() + e_h, dtype)
        return bt["ref"], e_mid + 0.5 * ulp_of(bt["ref"].abs() + e_mid, dtype)
    return bt["ref"], 0.5 * ulp_of(bt["ref"], dtype) + term


# ---- launches (shared by the GPU tests; ``out``: a caller's buffer of the result's shape)
def run(name, tier, mode, ops, dev, out=None):
    c, bt, dtype = BY_NAME[name], build(name, tier), MODES[mode]
    a, op, w = c.args, c.op, bt["w"]
    D = lambda t: None if t is None else t.to(dev, dtype).contiguous()
    ln = None if w.ln is None else (D(w.ln[0]), D(w.ln[1]), w.ln[2])
    if op == "linear":
        old_ring, old_prec = ops.set_gemm_ring(a.get("ring", 0)), ops.get_float32_matmul_precision()
        ops.set_float32_matmul_precision("high" if mode == "high" else "highest")
        try:
            return ops.linear(D(w.x), D(w.w1), D(w.b1), act=bt["act"], out=out)
        finally:
            ops.set_gemm_ring(old_ring)
            ops.set_float32_matmul_precision(old_prec)
    if op == "fold":
        from util import assert_bits_equal
        K = a["K"]
        x = ops.linear(D(w.x), torch.eye(K, dtype=dtype, device=dev), rowstat=True)  # the producer: stores the tier-R rows and their statistics
        assert_bits_equal(x, D(w.x), "producer")
        assert ops.rowstat_of(x) is not None and ops.ln_foldable(x, D(w.w1))
        return ops.linear(x, D(w.w1), D(w.b1), act="geglu", ln=ln, out=out)
    if op == "fused":
        assert ops.rp_ok(D(w.x)) and a["N"] % 64 == 0
        return ops.fused_linear(D(w.x), D(w.w1), D(w.b1), ln=ln, act=bt["act"], out=out)
    if op == "mlp":
        return ops.geglu_mlp(D(w.x), D(w.w1), D(w.b1), D(bt["w2"]), D(bt["b2"]), ln=ln, out=out)
    if op == "mlp_packed":
        wp, bp = ops.mlp_pack(D(w.w1), D(w.b1), D(bt["w2"]))
        return ops.geglu_mlp_packed(D(w.x), wp, bp, D(bt["b2"]), ln=ln, out=out)
    if op == "lngeglu":
        wp, bp = ops.geglu_pack(D(w.w1), D(w.b1))
        return ops.layernorm_geglu_packed(D(w.x), wp, bp, ln=ln, out=out)
    if op in ("hs", "hs_ff"):
        B, N = a["B"], a["N"]
        pk, bb = ops.hs_pack_geglu(D(w.w1), D(w.b1), ln=ln)  # the affine part (dyadic gamma, beta) folded by the packer
        x = D(w.x).view(B, N, HS_C)
        if op == "hs":
            return ops.hs_geglu(x, pk, bb, normalize=ln is not None, ln_eps=1e-5 if ln is None else ln[2], out=out)
        h = ops.hs_geglu(x, pk, bb, normalize=ln is not None, ln_eps=1e-5 if ln is None else ln[2])
        return ops.hs_ff2(h, ops.hs_pack_ff2(D(bt["w2"])), D(bt["b2"]), x, out=out)
    if op == "conv1d":
        return ops.conv1d(D(w.x).view(a["B"], a["T"], a["Cin"]), D(bt["wp"]), D(w.b1), a["taps"], dilation=a["dil"], act="tanh", out=out)
    if op == "geglu":
        return ops.geglu(D(bt["proj"]), out=out)
    assert op == "geglu_bwd"
    return ops.geglu_bwd(D(bt["proj"]), D(bt["dh"]), out=out)


def out_shape(name, tier):
    c, bt = BY_NAME[name], build(name, tier)
    if c.op in ("hs", "hs_ff"):
        return (c.args["B"], c.args["N"], bt["ref"].shape[-1])
    if c.op == "conv1d":
        return (c.args["B"], c.args["T"], c.args["Cout"])
    return tuple(bt["ref"].shape)
