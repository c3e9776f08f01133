"""The case table of the exact-softmax attention tests: tests/test_attn_exact_host.py builds every case's operands and fp64 reference on the CPU and
checks the conditions under which the expected result is determined; tests/test_gpu_exact_attention.py runs the same cases through the public ``ops``
wrappers.

A softmax is exact where every probability is 0, 1 or a power of two.  Three operand families ("tiers"), each with a plain fp64 softmax attention of
the same operands as its reference:
  S  selection: dims 0..15 of a head carry codes.  Key j has k = -1 on a set S_j of 8 of the 16 code dims (all S_j of a (K/V set, head) distinct), query
     i has q = 2048 on the code dims outside S_sel(i): the selected key scores exactly 0, every other key at most -2048 (at most -261 after the scale
     log2(e) / sqrt(128)), so p_sel = 1, every other p = 0 in fp32 and the output is V[sel(i)] in every bit, in every storage type and precision mode.
  U  uniform: q = 0, every p = 1, the denominator is the number of unmasked keys; V holds integers +-1..+-4, so every sum is an exact integer.  The
     inexact steps are 1 / den, the multiply by it and the final rounding: |out - ref| <= 0.5 ulp(ref) + 8 * 2^-24 * A(|V|).
  P  power-of-two weights (q_prescaled entries): q' one-hot, k integers 0..-3, so the base-2 scores are the integers 0..-3 and p is 1, 1/2, 1/4, 1/8;
     every rescale factor is a power of two.  The same bound as U.

Operands are built per head ([.., heads, d]) and flattened to the wrappers' [.., C] layout.  Poison: V^T of ops.attention's layout keeps ZERO pad
columns [L, Lpad) -- csrc/attention.hip documents that it needs them ("V must be supplied transposed per head ... with zero padding": a masked key's
probability 0 times a NaN pad would be NaN), and the raw (k, vt) pairs of cross_attention_rows / hs_attention are that layout.  Where a packer stands
between the layout and the kernel the pad is NaN (util.NAN_WORD): all of [L, Lpad) for xattn_pack_kv ("rows >= L: 0"), the columns from
round_up(L, 32) on for rows_pack_kv (it copies whole 32-key sub-tiles and reads nothing behind them).  K has no rows past L in any layout.

The fused entries (FUSED below) run with W_q = the identity (q = x; the zero matrix in tier U), W_o = the identity, b_o = 0 and ln = None; where the
entry adds its residual, x lives on the code dims 0..15 of every head and V on the others, so out = x there and A(V) here without a double rounding.
The self-attention of the 64-token level carries q code | k code | V side by side in x behind 0 / 1 selection matrices (hs_self_weights).

Two key segments blend as out = A1 + scale2 * A2.  The 16-bit kernels state their model in the source (attn_kernel / attn_short_kernel: "the un-fused
reference rounds each branch, and scale * audio, to the storage type before the add"): the 16-bit reference of a two-segment case is therefore
rne(A1) + rne(scale2 * rne(A2)), each branch from fp64, and the host test asserts that no branch value lies closer to a rounding tie than the fp32
error term (so the branch roundings are determined; tier P: where one does, both neighbours are admitted -- near_tie); the fp32 kernels add the
branches unrounded and keep the plain reference.  apad_fused_cross_attention states another model for segments of up to 128 keys: the NORMALISED
probabilities are rounded to the storage type (xattn_weights)."""
import functools
import itertools
import math
import zlib
from collections import namedtuple

import torch

from util import exact_operand, int_operand, ulp_of

MODES = {"bf16": torch.bfloat16, "f16": torch.float16, "highest": torch.float32, "high": torch.float32}
M16 = ("bf16", "f16")
F32 = ("highest", "high")
MASK_BIAS = -10000.0
KT = 64  # keys per tile of the staged kernels

Case = namedtuple("Case", "name route args tiers modes")
Seg = namedtuple("Seg", "k v bias sel real ref absref scores")  # one softmax segment; k, v [Bk, L, H, d] fp32; ref / absref [B, N, H, d] fp64
Built = namedtuple("Built", "q segs scale2 ref absref x")  # x: the fused entries' input rows [B, N, C]


def _seed(name, i):
    return (zlib.crc32(name.encode()) + 7919 * i) % (2 ** 31)


@functools.lru_cache(maxsize=1)
def _all_codes():
    """[12870, 16] 0 / 1: every 8-element subset of the 16 code dims"""
    t = torch.zeros(12870, 16)
    for r, c in enumerate(itertools.combinations(range(16), 8)):
        t[r, list(c)] = 1.0
    return t


def code_sets(groups, L, seed):
    """[groups, L, 16] 0 / 1: per group L DISTINCT 8-of-16 sets from a seeded generator"""
    g = torch.Generator().manual_seed(seed)
    allc = _all_codes()
    assert L <= allc.shape[0]
    return torch.stack([allc[torch.randperm(allc.shape[0], generator=g)[:L]] for _ in range(groups)], 0)


def attention64(q, k, v, scale, bias=None, kvdiv=1):
    """plain fp64 softmax attention: q [B, N, H, d], k / v [Bk, L, H, d], bias [B, L] additive -> (out [B, N, H, d], scores q.k [B, H, N, L] unscaled)"""
    B = q.shape[0]
    idx = torch.arange(B) // kvdiv
    kk, vv = k.double()[idx], v.double()[idx]
    s = torch.einsum("bnhd,blhd->bhnl", q.double(), kk)
    z = s * scale
    if bias is not None:
        z = z + bias.double()[:, None, None, :]
    p = torch.softmax(z, -1)
    return torch.einsum("bhnl,blhd->bnhd", p, vv), s


def _decoys(L):
    """masked form of tier S: {decoy key: its twin}: key 0, key L - 1 and one key beside its twin in every tile"""
    dec = {0: 1, L - 1: L - 2}
    for t in range((L + KT - 1) // KT):
        if KT * t + 5 < L - 2:
            dec[KT * t + 5] = KT * t + 4
    return dec


def select(B, H, N, L, real, prefer, seed):
    """sel [B, H, N]: within every 32-query tile the queries select the first real key, the last one, the first of the last key tile and then walk the
    key tiles (a random real key of each; ``prefer``: {tile: key} taken at the first visit), rotated per (sample, head): some queries of a tile find
    their key in tile 0 (the running maximum never moves again), others in the last tile (it rises late)"""
    g = torch.Generator().manual_seed(seed)
    T = (L + KT - 1) // KT
    tiles = [t for t in ([j for j in real if j // KT == t] for t in range(T)) if t]  # (masked form: a last tile of one key holds only a decoy)
    prefer = {i: prefer[t[0] // KT] for i, t in enumerate(tiles) if t[0] // KT in prefer}
    T = len(tiles)
    sel = torch.empty(B, H, N, dtype=torch.long)
    for b in range(B):
        for h in range(H):
            for i in range(N):
                r = (i + 5 * (b * H + h)) % 32
                if r == 0:
                    j = real[0]
                elif r == 1:
                    j = real[-1]
                elif r == 2:
                    j = tiles[-1][0]
                else:
                    t = (r - 3) % T
                    cand = tiles[t]
                    j = prefer[t] if (r - 3 < T and t in prefer) else cand[int(torch.randint(len(cand), (1,), generator=g))]
                sel[b, h, i] = j
    return sel


def _v_operand(tier, shape, seed, integer):
    if tier == "S" and not integer:
        return exact_operand(*shape, seed=seed)
    if tier == "S":  # two segments: integers large enough that V1 + scale2 * V2 needs a real rounding in bf16
        return int_operand(*shape, amp=100, seed=seed)
    g = torch.Generator().manual_seed(seed)
    return (torch.randint(1, 5, shape, generator=g) * (2 * torch.randint(0, 2, shape, generator=g) - 1)).float()


def build_segment(tier, name, si, B, N, H, d, L, kvdiv=1, masked=False, integer_v=False, scale=None, vcols=None):
    """one softmax segment of a case: -> (q [B, N, H, d] fp32, Seg).  ``scale``: what multiplies q.k in the reference's exponent (natural log units);
    vcols = (lo, hi): V is zero outside these head dims (the fused entries keep the code dims free of values)"""
    Bk = (B + kvdiv - 1) // kvdiv
    scale = 1.0 / math.sqrt(d) if scale is None else scale
    sd = lambda i: _seed(name, 16 * si + i)
    v = _v_operand(tier, (Bk, L, H, d), sd(0), integer_v)
    if vcols is not None:  # (assignment, not a product: -x * 0 would leave -0.0)
        v[..., :vcols[0]] = 0.0
        v[..., vcols[1]:] = 0.0
    q = torch.zeros(B, N, H, d)
    k = torch.zeros(Bk, L, H, d)
    bias, sel, real = None, None, list(range(L))
    g = torch.Generator().manual_seed(sd(1))
    if tier == "S":
        codes = code_sets(Bk * H, L, sd(2)).reshape(Bk, H, L, 16)
        dec = _decoys(L) if masked else {}
        for j, twin in dec.items():
            codes[:, :, j] = codes[:, :, twin]
        real = [j for j in range(L) if j not in dec]
        sel = select(B, H, N, L, real, {twin // KT: twin for j, twin in dec.items() if j not in (0, L - 1)}, sd(3))
        k[..., :16] = -codes.permute(0, 2, 1, 3)
        bk = (torch.arange(B) // kvdiv)[:, None, None].expand(B, H, N)
        hh = torch.arange(H)[None, :, None].expand(B, H, N)
        q[..., :16] = (2048.0 * (1.0 - codes[bk, hh, sel])).permute(0, 2, 1, 3)  # [B, H, N, 16] -> [B, N, H, 16]
        if masked:
            bias = torch.zeros(B, L)
            bias[:, list(dec)] = MASK_BIAS
    elif tier == "U":
        k = int_operand(Bk, L, H, d, amp=3, seed=sd(2))  # q = 0: the keys cannot matter
        if masked:
            bias = torch.zeros(B, L)
            for b in range(B):
                if b % 2 == 1:  # the whole ragged (last) 32-key sub-tile; a segment of one sub-tile: its last 4 keys
                    bias[b, (32 * ((L - 1) // 32) or L - 4):] = MASK_BIAS
                else:
                    drop = torch.rand(L, generator=g) < 0.25
                    drop[L - 1] = False
                    bias[b, drop] = MASK_BIAS
            real = None  # (per sample: see the bias)
    else:
        assert tier == "P" and not masked
        T = (L + KT - 1) // KT
        k = -torch.randint(0, 4, (Bk, L, H, d), generator=g).float()
        # even dims: the tile maximum is -3 in tile 0, at most -1 in the middle tiles and reaches 0 only in the last tile; odd dims: 0 from tile 0
        if T >= 2:
            mid = -torch.randint(1, 4, (Bk, L, H, d), generator=g).float()
            k[:, :KT * (T - 1), :, 0::2] = mid[:, :KT * (T - 1), :, 0::2]
            k[:, :KT, :, 0::2] = -3.0
            k[:, KT * (T - 1), :, 0::2] = 0.0
        k[:, 1, :, 1::2] = 0.0
        cdim = (torch.arange(N)[None, :, None] + 3 * torch.arange(H)[None, None, :] + torch.arange(B)[:, None, None]) % d
        q.scatter_(3, cdim[..., None], 1.0)
    ref, scores = attention64(q, k, v, scale, bias, kvdiv)
    absref, _ = attention64(q, k, v.abs(), scale, bias, kvdiv)
    return q, Seg(k, v, bias, sel, real, ref, absref, scores)


LN2 = math.log(2.0)


@functools.lru_cache(maxsize=4)
def build(name, tier):
    """operands and fp64 references of a case: the same for every storage type and precision mode"""
    c = BY_NAME[name]
    a = c.args
    fused = FUSED.get(c.route)
    B, N, H, d, L = a["B"], a["N"], (8 if fused else a.get("H", 2)), (fused["d"] if fused else a["d"]), a.get("L", a["N"])
    scale = LN2 if a.get("prescaled") else None  # a pre-scaled q is the base-2 exponent operand
    L2 = a.get("L2", 0)
    q, s1 = build_segment(tier, name, 0, B, N, H, d, L, a.get("kvdiv", 1), a.get("masked", False), L2 > 0, scale, fused["vcols"] if fused else None)
    segs, ref, absref = [s1], s1.ref, s1.absref
    if L2 > 0:
        if tier == "S":  # ONE q selects in both segments: segment 2 is built around the sets the queries already carry
            s2 = _second_selection(q, s1, name, B, N, H, d, L2, a.get("kvdiv", 1), a.get("kvdiv2", 1), scale, fused["vcols"] if fused else None)
        else:
            _, s2 = build_segment(tier, name, 1, B, N, H, d, L2, a.get("kvdiv2", 1), False, True, scale, fused["vcols"] if fused else None)
        segs.append(s2)
        ref = s1.ref + a["scale2"] * s2.ref
        absref = s1.absref + abs(a["scale2"]) * s2.absref
    return Built(q, segs, a.get("scale2", 0.0), ref, absref, _fused_rows(c, tier, q, s1) if fused else None)


# the fused sub-layer entries: 8 heads; V lives on the head dims ``vcols`` (the entries with a residual keep the code dims 0..15 free of values: out = x
# there and V[sel] on the value dims, with no double rounding to argue about; the self-attention carries q codes, k codes and V side by side in x)
FUSED = {"xattn": dict(d=32, vcols=(16, 32)), "xrows": dict(d=48, vcols=(16, 48)), "hs_cross": dict(d=80, vcols=None), "hs_self": dict(d=80, vcols=(32, 80))}


def _fused_rows(c, tier, q, s1):
    """x [B, N, C]: the query operand on the code dims (W_q is the identity; in tier U, where W_q = 0, small integers that a non-zero W_q would turn into
    scores); hs_self: per head [q code | k code | V dims 32..79] of the token"""
    B, N, H, d = q.shape
    x = q.clone()
    if tier == "U":
        x[..., :16] = int_operand(B, N, H, 16, amp=8, seed=_seed(c.name, 40))
    if c.route == "hs_self":
        x[..., 16:32] = s1.k[..., :16]
        x[..., 32:] = s1.v[..., 32:]
    return x.reshape(B, N, H * d)


def _code_key(rows):
    return (rows * (2.0 ** torch.arange(16.0))).sum(-1).long()


def _second_selection(q, s1, name, B, N, H, d, L2, kvdiv, kvdiv2, scale, vcols=None):
    """tier S, second segment: the query's code is fixed by segment 1 (q = 2048 outside S_sel1(i)), so the key of segment 2 that query i selects must
    carry the SAME set S_sel1(i) and every other key of segment 2 another one.  Per (K/V-2 sample, head): the sets its queries use go to the first,
    the last and evenly spread keys of segment 2, the remaining keys take sets no query uses."""
    Bk2 = (B + kvdiv2 - 1) // kvdiv2
    v2 = _v_operand("S", (Bk2, L2, H, d), _seed(name, 16), True)
    if vcols is not None:
        v2[..., :vcols[0]] = 0.0
        v2[..., vcols[1]:] = 0.0
    codes1 = -s1.k[..., :16].permute(0, 2, 1, 3)  # [Bk1, H, L1, 16]
    keys1 = _code_key(codes1)
    allc = _all_codes()
    allk = _code_key(allc)
    order = torch.argsort(allk)
    g = torch.Generator().manual_seed(_seed(name, 17))
    k2 = torch.zeros(Bk2, L2, H, d)
    sel2 = torch.empty(B, H, N, dtype=torch.long)
    for b2 in range(Bk2):
        samples = [b for b in range(B) if b // kvdiv2 == b2]
        for h in range(H):
            qkeys = {b: keys1[b // kvdiv, h][s1.sel[b, h]] for b in samples}  # the code of every query [N]
            used = torch.unique(torch.cat(list(qkeys.values())))
            n = used.numel()
            assert n <= L2, "segment 2 has fewer keys than its queries have distinct codes"
            slots = torch.unique(torch.round(torch.arange(n) * ((L2 - 1) / max(n - 1, 1))).long())
            assert slots.numel() == n
            perm = torch.randperm(allc.shape[0], generator=g)
            fresh = perm[~torch.isin(allk[perm], used)][:L2 - n]
            rows = torch.empty(L2, 16)
            rest = torch.ones(L2, dtype=torch.bool)
            rest[slots] = False
            rows[slots] = allc[order[torch.searchsorted(allk[order], used)]]
            rows[rest] = allc[fresh]
            k2[b2, :, h, :16] = -rows
            for b in samples:
                sel2[b, h] = slots[torch.searchsorted(used, qkeys[b])]
    sc = 1.0 / math.sqrt(d) if scale is None else scale
    ref, scores = attention64(q, k2, v2, sc, None, kvdiv2)
    absref, _ = attention64(q, k2, v2.abs(), sc, None, kvdiv2)
    return Seg(k2, v2, None, sel2, list(range(L2)), ref, absref, scores)


def _r16(t, dtype):
    return t.float().to(dtype).double()


def near_tie(x, dtype):
    """fp64 0 / 1: the branch values whose rounding to ``dtype`` the fp32 error of the branch (an exact sum times a rounded reciprocal: a few fp32 ulp
    of the value) can turn either way.  The two-segment model rounds each branch; where a branch value is this close to a tie the model admits both
    neighbours, and the bound grows by one ulp of the branch THERE (decided on the reference alone)."""
    margin = 0.5 * ulp_of(x, dtype) - (x - _r16(x, dtype)).abs()
    return (margin <= 8.0 * 2.0 ** -24 * x.abs()).double()


def _keys_per_sample(seg, B):
    """[B] fp64: the unmasked keys of every sample (tiers U: the softmax denominator)"""
    return torch.full((B,), float(seg.k.shape[1]), dtype=torch.float64) if seg.bias is None else (seg.bias == 0).sum(1).double()


def xattn_weights(bt, si, dtype, rcp_err=0.0):
    """tier U through apad_fused_cross_attention: the weight every key of segment ``si`` carries into the P.V product, [B] fp64.  A segment of up to 128
    keys follows xa_segment's stated model -- "the probabilities, normalised and scaled by pscale, are rounded to the storage type": rne(pscale *
    fl32(1 / den)) --, a longer second segment the chunked form's: un-normalised probabilities (1), one multiply by scale2 / den at the end (exact
    here up to the bound's fp32 term).  ``rcp_err``: relative error given to the reciprocal (the host test moves it by an ulp either way)."""
    seg = bt.segs[si]
    den = _keys_per_sample(seg, bt.q.shape[0])
    pscale = 1.0 if si == 0 else bt.scale2
    if si == 1 and seg.k.shape[1] > 128:
        return pscale / den
    return _r16((pscale * ((1.0 / den).float().double() * (1.0 + rcp_err))).float().double(), dtype)


def expected(name, tier, dtype):
    """(fp64 value the final rounding sees, fp64 magnitude A(|V|)) under the kernels' documented model for ``dtype`` (module docstring)"""
    c, bt = BY_NAME[name], build(name, tier)
    B, absref = bt.q.shape[0], bt.absref
    if c.route == "xattn" and tier == "U":
        ref = 0.0
        for si, seg in enumerate(bt.segs):
            den = _keys_per_sample(seg, B)[:, None, None, None]
            ref = ref + (seg.ref * den).round() * xattn_weights(bt, si, dtype)[:, None, None, None]  # (the integer sums) x (the weight)
    elif len(bt.segs) == 1 or dtype == torch.float32:
        ref = bt.ref
    else:
        ref = _r16(bt.segs[0].ref, dtype) + _r16(bt.scale2 * _r16(bt.segs[1].ref, dtype), dtype)
        if tier == "P":  # (tier U has no such element: asserted by the host test)
            absref = absref + sum(near_tie(seg.ref, dtype) * ulp_of(seg.ref, dtype) * w for seg, w in zip(bt.segs, (1.0, abs(bt.scale2)))) / (8.0 * 2.0 ** -24)
    if c.route in ("xattn", "xrows"):  # the sub-layer's residual: x lives on the code dims, the values on the others
        ref = ref + bt.x.double().reshape(ref.shape)
    return ref, absref


def _attention_run(c, bt, mode, ops, dev, out):
    from util import nan_padded_vt
    a, dtype = c.args, MODES[mode]
    B, N, H, d = bt.q.shape
    D = lambda t: t.reshape(t.shape[0], t.shape[1], H * d).to(dev, dtype).contiguous()
    old = ops.get_float32_matmul_precision()
    try:
        if mode in F32:
            ops.set_float32_matmul_precision(mode)
        s1 = bt.segs[0]
        L = s1.k.shape[1]
        vt = nan_padded_vt(s1.v, ops.round_up(L, 32) + a.get("lpad_extra", 0), dtype, dev, poison=False)
        bias = None if s1.bias is None else s1.bias.to(dev)
        if a.get("lse"):
            o, lse = ops.attention_lse(D(bt.q), D(s1.k), vt, L, H, key_bias=bias)
            return o.reshape(B, N, H, d), lse
        kw = {}
        if len(bt.segs) == 2:
            s2 = bt.segs[1]
            L2 = s2.k.shape[1]
            kw = dict(k2=D(s2.k), vt2=nan_padded_vt(s2.v, ops.round_up(L2, 32), dtype, dev, poison=False), L2=L2, scale2=bt.scale2,
                      kv2_batch_div=a.get("kvdiv2", 1))
        o = ops.attention(D(bt.q), D(s1.k), vt, L, H, key_bias=bias, kv_batch_div=a.get("kvdiv", 1), q_prescaled=bool(a.get("prescaled")), out=out, **kw)
        return o.reshape(B, N, H, d), None
    finally:
        ops.set_float32_matmul_precision(old)


def hs_self_weights(tier):
    """0 / 1 selection matrices [640, 640] of the self-attention case: per head q = x[0:16] (zero matrix in tier U), k = x[16:32] -> dims 0..15, v = x[32:80]"""
    C, d = 640, 80
    j = torch.arange(C) % d
    wq = torch.diag((j < 16).float()) if tier != "U" else torch.zeros(C, C)
    wk = torch.zeros(C, C)
    rows = torch.arange(C)[j < 16]
    wk[rows, rows + 16] = 1.0
    return wq, wk, torch.diag((j >= 32).float())


def _fused_run(c, bt, tier, mode, ops, dev, out):
    """the fused sub-layer entries: W_q the identity (the zero matrix in tier U), W_o the identity, b_o = 0, ln = None.  V^T pad columns are NaN where
    the entry's packer documents that it masks them (apad_xattn_pack_kv: "rows >= L: 0"; apad_rows_pack_kv never reads past round_up(L, 32), the
    columns [L, round_up(L, 32)) stay zero as in ops.attention's layout), zero in the raw layout."""
    from util import nan_padded_vt
    a, dtype, route = c.args, MODES[mode], c.route
    B, N, H, d = bt.q.shape
    C = H * d
    D = lambda t: t.reshape(t.shape[0], t.shape[1], C).to(dev, dtype).contiguous()
    W = lambda t: t.to(dev, dtype).contiguous()
    x = bt.x.to(dev, dtype).contiguous()
    eye = torch.eye(C)
    wq = torch.zeros(C, C) if tier == "U" else eye
    bias = None if bt.segs[0].bias is None else bt.segs[0].bias.to(dev)
    Ls = [seg.k.shape[1] for seg in bt.segs]
    if route == "hs_self":
        pk, bb = ops.hs_pack_qkv(*(W(w) for w in hs_self_weights(tier)))
        assert bb is None
        return ops.hs_attention(x, pk, None, self_attention=True, normalize=False, out=out).reshape(B, N, H, d), None
    if route == "xattn":
        pks = [ops.xattn_pack_kv(D(seg.k), nan_padded_vt(seg.v, ops.round_up(L, 32) + 32 * (si == 0), dtype, dev, poison=True), L) for si, (seg, L) in enumerate(zip(bt.segs, Ls))]
        o = ops.fused_cross_attention(x, ops.xattn_pack_weight(W(wq)), ops.xattn_pack_weight(W(eye)), torch.zeros(C, dtype=dtype, device=dev), pks[0], Ls[0], H,
                                      ln=None, key_bias=bias, kv2_packed=pks[1] if len(pks) == 2 else None, L2=Ls[1] if len(pks) == 2 else 0, scale2=bt.scale2, out=out)
        return o.reshape(B, N, H, d), None
    raw = [(D(seg.k), nan_padded_vt(seg.v, ops.round_up(L, 32), dtype, dev, poison=False)) for seg, L in zip(bt.segs, Ls)]
    packed = [(ops.rows_pack_kv(D(seg.k), nan_padded_vt(seg.v, ops.round_up(L, 32) + 32, dtype, dev, poison=True, zero_to=ops.round_up(L, 32))), None)
              for seg, L in zip(bt.segs, Ls)]
    if route == "xrows":
        wq_p, wo_p, bo = ops.xrows_pack_weight(W(wq)), ops.xrows_pack_weight(W(eye)), torch.zeros(C, dtype=dtype, device=dev)
        call = lambda kv, o_: ops.cross_attention_rows(x, wq_p, wo_p, bo, kv[0][0], kv[0][1], H, ln=None, key_bias=bias, k2=kv[1][0] if len(kv) == 2 else None,
                                                       vt2=kv[1][1] if len(kv) == 2 else None, scale2=bt.scale2, out=o_)
    else:
        assert route == "hs_cross"
        wq_p, qb = ops.hs_pack_rows(W(wq))
        assert qb is None
        call = lambda kv, o_: ops.hs_attention(x, wq_p, None, self_attention=False, normalize=False, k1=kv[0][0], vt1=kv[0][1], key_bias=bias,
                                               k2=kv[1][0] if len(kv) == 2 else None, vt2=kv[1][1] if len(kv) == 2 else None, scale2=bt.scale2,
                                               q_prescaled=bool(a.get("prescaled")), out=o_)
    o = call(raw, out)
    o_packed = call(packed, None)
    assert torch.equal(o.view(torch.int16), o_packed.view(torch.int16)), f"{c.name}: the raw and the packed key / value sets give different bits"
    return o.reshape(B, N, H, d), None


def run(name, tier, mode, ops, dev, out=None):
    """launch the case through its public ``ops`` wrapper; -> (out [B, N, H, d], lse or None)"""
    c, bt = BY_NAME[name], build(name, tier)
    if c.route in FUSED:
        return _fused_run(c, bt, tier, mode, ops, dev, out)
    return _attention_run(c, bt, mode, ops, dev, out)


def route_of(a, is16, ops=None, route=None):
    """csrc/attention.hip, launch_d: the kernel form a launch of ops.attention / attention_lse takes.  The fused entries: the envelope function of
    their wrapper and the kernel form the key counts select (xattn_kernel's template arguments in apad_fused_cross_attention, xattn_rows_launch,
    hs_attn_go), named in the case's ``form``"""
    if route in FUSED:
        L1, L2, masked = a.get("L", a["N"]), a.get("L2", 0), bool(a.get("masked"))
        if route == "xattn":
            ok = ops is None or ops.xattn_lengths_ok(L1, L2, masked)
            form = "chunk" if L2 > 128 else "split" if L2 > 64 else "resident"
        elif route == "hs_self":
            ok, form = a["N"] <= 64, "resident"
        else:
            ok = ops is None or (ops.xrows_ok(384, 8, L1, L2) if route == "xrows" else ops.hs_cross_lengths_ok(L1, L2))
            form = "chunk" if L2 > (64 if route == "xrows" else 128) else "split" if L2 > 64 else "two_sub" if max(L1, L2) > 32 else "resident"
        return route if ok and is16 and form == a["form"] else None
    if not is16:
        return "f32"
    dual, lse, bias = a.get("L2", 0) > 0, bool(a.get("lse")), bool(a.get("masked"))
    if a["L"] <= 64 and (not dual or a["L2"] <= 64) and not lse:
        return "short"
    if a["d"] in (32, 48) and not dual and not bias and a["N"] >= 200 and a["L"] >= 200:
        return "2q_direct" if a["d"] == 32 and a.get("prescaled") else "2q"
    return "generic"


def _c(name, route, tiers="SU", modes=M16, **args):
    return Case(name, route, args, tiers, modes)


CASES = [
    # ---- attn_short_kernel: L <= 64, L2 <= 64, no lse; one and two 32-key sub-tiles, every head size
    _c("short_L7_d16", "short", B=2, N=40, L=7, d=16),
    _c("short_L32_d32", "short", B=2, N=130, L=32, d=32),
    _c("short_L33_d48", "short", B=2, N=40, L=33, d=48),
    _c("short_L64_d64", "short", B=2, N=130, L=64, d=64, lpad_extra=32),
    _c("short_L33_d80", "short", B=2, N=130, L=33, d=80),
    _c("short_L64_d96", "short", B=2, N=40, L=64, d=96),
    _c("short_L7_d128", "short", B=2, N=130, L=7, d=128),
    _c("short_L32_d128", "short", B=1, N=40, L=32, d=128, lpad_extra=32),
    _c("short_dual_8_32", "short", B=2, N=130, L=8, L2=32, d=32, scale2=0.5),
    _c("short_dual_8_64", "short", B=2, N=40, L=8, L2=64, d=80, scale2=2.0),
    _c("short_dual_kvdiv", "short", B=4, N=40, L=8, L2=33, d=48, scale2=0.5, kvdiv=2, kvdiv2=1),
    _c("short_masked_L16", "short", B=2, N=130, L=16, d=80, masked=True),
    _c("short_prescaled_L64", "short", "P", B=2, N=40, L=64, d=32, prescaled=True),
    # ---- attn_kernel: the staged generic form
    _c("generic_L65", "generic", B=2, N=130, L=65, d=32),
    _c("generic_L130", "generic", B=2, N=40, L=130, d=48),
    _c("generic_L257", "generic", B=1, N=199, L=257, d=16),
    _c("generic_masked_L257", "generic", B=2, N=300, L=257, d=32, masked=True),  # (the bias forces the generic kernel)
    _c("generic_dual_8_128", "generic", B=2, N=130, L=8, L2=128, d=64, scale2=0.5),
    _c("generic_dual_70_513", "generic", B=2, N=40, L=70, L2=513, d=32, scale2=2.0),
    _c("generic_kvdiv2", "generic", B=4, N=130, L=130, d=32, kvdiv=2),
    _c("generic_dual_kvdiv", "generic", B=4, N=40, L=70, L2=130, d=32, scale2=0.5, kvdiv=2, kvdiv2=1),
    _c("generic_dual_kvdiv2", "generic", B=4, N=40, L=40, L2=130, d=32, scale2=0.5, kvdiv=1, kvdiv2=2),
    _c("generic_L200_d64", "generic", B=1, N=130, L=200, d=64),
    _c("generic_L200_d80", "generic", B=1, N=130, L=200, d=80),
    _c("generic_L200_d96", "generic", B=1, N=130, L=200, d=96, lpad_extra=32),
    _c("generic_L200_d128", "generic", B=1, N=130, L=200, d=128),
    _c("generic_lse_L130", "generic", B=2, N=130, L=130, d=32, lse=True),
    _c("generic_lse_masked_L40", "generic", B=2, N=70, L=40, d=64, lse=True, masked=True),
    _c("generic_prescaled_L257_d48", "generic", "P", B=2, N=130, L=257, d=48, prescaled=True),
    # ---- attn2q_kernel, classic form: B = 3 leaves idle slots in the grid's batch round-up to 8
    _c("2q_200x200_d32", "2q", B=3, N=200, L=200, d=32),
    _c("2q_257x321_d48", "2q", B=3, N=257, L=321, d=48),
    _c("2q_513x1029_d32", "2q", B=3, N=513, L=1029, d=32),
    _c("2q_513x1029_d48", "2q", B=3, N=513, L=1029, d=48),
    _c("2q_lse_257x321_d32", "2q", B=3, N=257, L=321, d=32, lse=True),
    _c("2q_prescaled_257x321_d48", "2q", "P", B=3, N=257, L=321, d=48, prescaled=True),
    # ---- attn2q_kernel, direct form (d = 32, q pre-scaled)
    _c("direct_200x200", "2q_direct", "SUP", B=3, N=200, L=200, d=32, prescaled=True),
    _c("direct_257x321", "2q_direct", "SUP", B=3, N=257, L=321, d=32, prescaled=True),
    _c("direct_513x1029", "2q_direct", "SUP", B=3, N=513, L=1029, d=32, prescaled=True),
    # ---- apad_f32_attention, "highest" and "high" (bf16x3: the operands split as hi = x, lo = 0)
    _c("f32_130x70_d32", "f32", modes=F32, B=2, N=130, L=70, d=32),
    _c("f32_257x321_d48", "f32", modes=F32, B=2, N=257, L=321, d=48),
    _c("f32_dual_8_33", "f32", modes=F32, B=2, N=130, L=8, L2=33, d=32, scale2=0.5),
    _c("f32_masked_lse_L70", "f32", modes=F32, B=2, N=40, L=70, d=32, lse=True, masked=True),
    # ---- ops.fused_cross_attention (C = 256, 8 heads of 32): B = 3 with N = 33 / 130, so 32-token panels and 128-token tiles end inside a sample
    _c("xattn_8_0", "xattn", B=3, N=33, L=8, form="resident"),
    _c("xattn_40_0", "xattn", B=3, N=130, L=40, form="resident"),
    _c("xattn_8_32", "xattn", B=3, N=130, L=8, L2=32, scale2=0.5, form="resident"),
    _c("xattn_8_33", "xattn", B=3, N=33, L=8, L2=33, scale2=2.0, form="resident"),
    _c("xattn_8_128", "xattn", B=3, N=130, L=8, L2=128, scale2=0.5, form="split"),
    _c("xattn_8_192", "xattn", B=3, N=33, L=8, L2=192, scale2=2.0, form="chunk"),
    _c("xattn_8_512", "xattn", B=3, N=130, L=8, L2=512, scale2=0.5, form="chunk"),
    _c("xattn_masked_16", "xattn", B=3, N=130, L=16, masked=True, form="resident"),
    # ---- ops.cross_attention_rows (C = 384, 8 heads of 48): every case runs the raw (k, vt) pair and the rows_pack_kv form, which must agree in every bit
    _c("xrows_8_0", "xrows", B=3, N=33, L=8, form="resident"),
    _c("xrows_64_64", "xrows", B=3, N=100, L=64, L2=64, scale2=0.5, form="two_sub"),
    _c("xrows_8_128", "xrows", B=3, N=33, L=8, L2=128, scale2=2.0, form="chunk"),
    _c("xrows_32_512", "xrows", B=3, N=100, L=32, L2=512, scale2=0.5, form="chunk"),
    _c("xrows_masked_16", "xrows", B=3, N=100, L=16, masked=True, form="resident"),
    _c("xrows_masked_40_33", "xrows", B=3, N=33, L=40, L2=33, scale2=0.5, masked=True, form="two_sub"),
    # ---- ops.hs_attention, cross (C = 640, 8 heads of 80, normalize=False): raw and packed sets; tier P with q_prescaled=True
    _c("hs_cross_8_0", "hs_cross", B=3, N=1, L=8, form="resident"),
    _c("hs_cross_40_0", "hs_cross", B=3, N=33, L=40, form="two_sub"),
    _c("hs_cross_8_32", "hs_cross", B=3, N=64, L=8, L2=32, scale2=0.5, form="resident"),
    _c("hs_cross_8_128", "hs_cross", B=3, N=33, L=8, L2=128, scale2=2.0, form="split"),
    _c("hs_cross_8_129", "hs_cross", B=3, N=64, L=8, L2=129, scale2=0.5, form="chunk"),
    _c("hs_cross_32_200", "hs_cross", B=3, N=33, L=32, L2=200, scale2=2.0, form="chunk"),
    _c("hs_cross_8_512", "hs_cross", B=3, N=64, L=8, L2=512, scale2=0.5, form="chunk"),
    _c("hs_cross_masked_40", "hs_cross", B=3, N=64, L=40, masked=True, form="two_sub"),
    _c("hs_cross_p_40_0", "hs_cross", "P", B=3, N=33, L=40, prescaled=True, form="two_sub"),
    _c("hs_cross_p_8_129", "hs_cross", "P", B=3, N=64, L=8, L2=129, scale2=0.5, prescaled=True, form="chunk"),
    _c("hs_cross_p_32_200", "hs_cross", "P", B=3, N=1, L=32, L2=200, scale2=2.0, prescaled=True, form="chunk"),
    _c("hs_cross_p_8_512", "hs_cross", "P", B=3, N=64, L=8, L2=512, scale2=0.5, prescaled=True, form="chunk"),
    # ---- ops.hs_attention, self (normalize=False): q code | k code | V side by side in x, 0 / 1 selection matrices through hs_pack_qkv
    _c("hs_self_1", "hs_self", B=3, N=1, form="resident"),
    _c("hs_self_33", "hs_self", B=3, N=33, form="resident"),
    _c("hs_self_40", "hs_self", B=3, N=40, form="resident"),
    _c("hs_self_64", "hs_self", B=3, N=64, form="resident"),
]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def params():
    """(case name, tier, mode), the modes of a (case, tier) together so that build()'s cache serves them"""
    return [(c.name, t, m) for c in CASES for t in c.tiers for m in c.modes]
