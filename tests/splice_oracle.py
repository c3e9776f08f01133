"""The splice of a region edit into its reference recording, restated in fp64 numpy, independent of ap_adapter_amd/splice.py and of the
kernel: the host plan (merge, seams, kept set), the gain over the kept set, each seam's least-squares window with its tie rule and
correlation, the power-complementary crossfade, and the copy everywhere else.

The one fp32 operation of the definition is kept as one: ge[i] = fp32(fp32(g) * e[i]).  Everything after it (differences, costs,
correlations, crossfades) is fp64 on those fp32 values.
"""
import collections
import math

import numpy as np

U = 2.0 ** -24  # the unit roundoff of fp32

Plan = collections.namedtuple("Plan", "regions seams kept")  # seams: per region (left, right), each (lo, hi) or None
Result = collections.namedtuple("Result", "out g starts cost rho costs plan")


def plan(n, regions, W, M):
    """step 1: sorted, merged (gap < 2 M) regions; per region the search spans [lo, hi) of its seams (window starts in [lo, hi - W]); kept"""
    if W < 2 or M < W or M > 8192:
        raise ValueError(f"W={W}, M={M}: need 2 <= W <= M <= 8192")
    regs = sorted((int(a), int(b)) for a, b in regions)
    if not regs:
        raise ValueError("no region")
    if any(not 0 <= a < b <= n for a, b in regs):
        raise ValueError("a region is empty or outside the clip")
    merged = []
    for a, b in regs:
        if merged and a - merged[-1][1] < 2 * M:
            merged[-1][1] = max(merged[-1][1], b)
        else:
            merged.append([a, b])
    if len(merged) > 4:
        raise ValueError("more than 4 regions (8 seams)")
    seams, inside = [], np.zeros(n, bool)
    for a, b in merged:
        left = (max(0, a - M), a) if a >= W else None
        right = (b, min(n, b + M)) if n - b >= W else None
        seams.append((left, right))
        inside[(left[0] if left else 0):(right[1] if right else n)] = True
    if inside.all():
        raise ValueError("no kept sample")
    edges = np.flatnonzero(np.diff(np.concatenate([[True], inside, [True]]).astype(np.int8)))
    return Plan([tuple(m) for m in merged], seams, [(int(lo), int(hi)) for lo, hi in zip(edges[0::2], edges[1::2])])


def kept_gain(e, r, kept):
    """step 2, in fp64: sqrt(sum r^2 / sum e^2) over the kept intervals; 1 if either sum is 0 or not finite"""
    idx = np.concatenate([np.arange(lo, hi) for lo, hi in kept])
    sr, se = float((r[idx].astype(np.float64) ** 2).sum()), float((e[idx].astype(np.float64) ** 2).sum())
    return math.sqrt(sr / se) if sr > 0 and se > 0 and math.isfinite(sr) and math.isfinite(se) else 1.0


def window_costs(d, W):
    """cost(s) for every window start of a span's differences d (fp64): the sum of d^2 over W consecutive samples"""
    return np.lib.stride_tricks.sliding_window_view(d * d, W).sum(axis=1)


def splice(e, r, regions, W, M, shape="matched", gain="kept", starts_in=None):
    """e, r: fp32 arrays of one length -> Result: out fp64 [n], g (fp64: the measured or the given one), starts [8] (-1 = no seam), cost
    [8], rho [8] (the measured correlation, whatever the shape), costs (per seam the fp64 cost of every candidate, or None), plan.
    ``starts_in`` [8]: take these window starts instead of the minimisers (what follows a seam search, for starts found elsewhere)"""
    e, r = np.asarray(e, np.float32), np.asarray(r, np.float32)
    n = len(e)
    assert len(r) == n
    p = plan(n, regions, W, M)
    g = kept_gain(e, r, p.kept) if isinstance(gain, str) and gain == "kept" else 1.0 if gain is None else float(gain)
    ge = (np.float32(g) * e).astype(np.float32).astype(np.float64)  # ONE fp32 multiply
    r64 = r.astype(np.float64)
    out = r64.copy()
    starts, cost, rho, costs = [-1] * 8, [0.0] * 8, [0.0] * 8, [None] * 8
    for q, ((a, b), sides) in enumerate(zip(p.regions, p.seams)):
        for side, span in enumerate(sides):
            if span is None:
                continue
            lo, hi = span
            c = window_costs(r64[lo:hi] - ge[lo:hi], W)
            best = np.flatnonzero(c == c.min())
            s = lo + int(best[-1] if side == 0 else best[0])  # the tie goes to the start nearest the region
            if starts_in is not None:
                s = int(starts_in[2 * q + side])
                assert lo <= s <= hi - W
            rw, gw = r64[s:s + W], ge[s:s + W]
            err, erg = float((rw * rw).sum()), float((gw * gw).sum())
            k = 2 * q + side
            starts[k], cost[k], costs[k] = s, float(c[s - lo]), c
            rho[k] = min(max(float((rw * gw).sum()) / math.sqrt(err * erg), 0.0), 1.0) if err > 0 and erg > 0 else 0.0
        sl, sr = starts[2 * q], starts[2 * q + 1]
        lo, hi = (sl + W if sl >= 0 else 0), (sr if sr >= 0 else n)
        out[lo:hi] = ge[lo:hi]
        for side, s in ((0, sl), (1, sr)):
            if s < 0:
                continue
            c = {"matched": rho[2 * q + side], "linear": 1.0, "equal_power": 0.0}[shape]
            t = (np.arange(W) + 0.5) / W
            we = t if side == 0 else 1.0 - t
            wr = 1.0 - we
            out[s:s + W] = (wr * r64[s:s + W] + we * ge[s:s + W]) / np.sqrt(wr * wr + we * we + 2.0 * c * wr * we)
    return Result(out, g, starts, cost, rho, costs, p)


def window_mask(res, W, n):
    """True inside the chosen crossfade windows"""
    m = np.zeros(n, bool)
    for s in res.starts:
        if s >= 0:
            m[s:s + W] = True
    return m


def edit_mask(res, W, n):
    """True between each region's two windows (from the clip's edge where a seam is absent)"""
    m = np.zeros(n, bool)
    for q in range(len(res.plan.regions)):
        sl, sr = res.starts[2 * q], res.starts[2 * q + 1]
        m[(sl + W if sl >= 0 else 0):(sr if sr >= 0 else n)] = True
    return m


def gamma(k):
    """Higham's gamma_k for fp32: the relative error bound of k successive roundings"""
    return k * U / (1.0 - k * U)


def signal(n, seed=0, sr=16000):
    """seeded sines plus noise, fp32, peak below 1"""
    g = np.random.default_rng(seed)
    t = np.arange(n) / sr
    x = sum(a * np.sin(2 * np.pi * f * t + ph) for a, f, ph in zip((0.3, 0.2, 0.1), g.uniform(100, 2000, 3), g.uniform(0, 6.28, 3)))
    return (x + 0.02 * g.standard_normal(n)).astype(np.float32)


def planted(n, regions, W, M, seed=0):
    """(e, r, planted starts [8]): r = sines plus noise; e = (r + noise * env) / 1.7 with env = 0 on the kept set and on one planted
    window inside each search span, 1 elsewhere (the rest of the spans, and the regions)"""
    g = np.random.default_rng(seed + 1000)
    r = signal(n, seed)
    p = plan(n, regions, W, M)
    env = np.ones(n)
    for lo, hi in p.kept:
        env[lo:hi] = 0.0
    want = [-1] * 8
    for q, sides in enumerate(p.seams):
        for side, span in enumerate(sides):
            if span is not None:
                s = int(g.integers(span[0], span[1] - W + 1))
                env[s:s + W] = 0.0
                want[2 * q + side] = s
    noise = 0.1 * g.standard_normal(n)
    e = ((r.astype(np.float64) + noise * env) / 1.7).astype(np.float32)
    return e, r, want
