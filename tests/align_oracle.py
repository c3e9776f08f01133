"""The time alignment of an edit to its reference recording, restated in fp64 (and int64) numpy, independent of ap_adapter_amd/align.py
and of the kernels: the kept set, the correlation table over [-L, L], the winner with its tie order, the normalised correlation, the gate
and the shift.

A lag l means e[i + l] ~ r[i]: positive = the edit is late.  K = the kept intervals of the splice plan (splice_oracle.plan), each shrunk by
L on both sides.  c(l) = sum over K of r[i] e[i + l]; the winner is the largest c, ties to the smaller |l|, then to l >= 0;
ncc(l) = c(l) / sqrt(sum_K r[i]^2 sum_K e[i + l]^2), 0 when either energy is 0; the applied lag is the winner if c > 0 and ncc >= min_corr,
else 0; a[i] = e[i + lag] where that lies in the clip, +0.0 elsewhere.
"""
import collections
import math

import numpy as np

import splice_oracle as S

Result = collections.namedtuple("Result", "out found applied c mag ncc ncc0 er kept")
Result.__doc__ = """out: the shifted edit (fp32, the edit's bits); found / applied: the lags; c: the table [2 L + 1] (fp64, or int64 from
integer signals); mag: sum |r e| per lag (what a rounding bound multiplies); ncc / ncc0 at the found lag and at 0; er = sum_K r^2"""


def kept_set(n, regions, W, M, L):
    """the splice plan's kept intervals, or the whole clip without regions, shrunk by L on both sides; the empty ones dropped"""
    kept = S.plan(n, regions, W, M).kept if regions else [(0, n)]
    out = [(lo + L, hi - L) for lo, hi in kept if lo + L < hi - L]
    if not out:
        raise ValueError("no kept sample")
    return out


def index(kept):
    return np.concatenate([np.arange(lo, hi) for lo, hi in kept])


def table(e, r, kept, L, dtype=np.float64):
    """(c, mag) over l = -L .. L, entry l + L"""
    idx = index(kept)
    rk, ee = np.asarray(r)[idx].astype(dtype), np.asarray(e).astype(dtype)
    c, mag = np.zeros(2 * L + 1, dtype), np.zeros(2 * L + 1, dtype)
    for j in range(2 * L + 1):
        prod = rk * ee[idx + (j - L)]
        c[j], mag[j] = prod.sum(), np.abs(prod).sum()
    return c, mag


def winner(c, L):
    """the search from (c(0), 0): a candidate replaces the holder if its c is larger, or equal with a smaller |l|, or with the same |l| and
    l > 0"""
    best, bl = c[L], 0
    for j in range(2 * L + 1):
        l = j - L
        if c[j] > best or (c[j] == best and (abs(l) < abs(bl) or (abs(l) == abs(bl) and l > bl))):
            best, bl = c[j], l
    return bl


def energy(x, kept, lag=0):
    v = np.asarray(x)[index(kept) + lag].astype(np.float64)
    return float((v * v).sum())


def ncc(c, er, ee):
    return 0.0 if er == 0.0 or ee == 0.0 else float(c) / math.sqrt(er * ee)


def shift(e, lag):
    """a[i] = e[i + lag], the same bits, +0.0 where i + lag leaves the clip"""
    e = np.asarray(e, np.float32)
    n = len(e)
    out = np.zeros(n, np.float32)
    i = np.arange(n)
    ok = (i + lag >= 0) & (i + lag < n)
    out[ok] = e[i[ok] + lag]
    return out


def align(e, r, kept, L, min_corr=0.5, integer=False):
    e, r = np.asarray(e, np.float32), np.asarray(r, np.float32)
    assert len(e) == len(r) and all(L <= lo < hi <= len(e) - L for lo, hi in kept)
    c, mag = table(e, r, kept, L, np.int64 if integer else np.float64)
    found = winner(c, L)
    er = energy(r, kept)
    n_star, n_zero = ncc(c[found + L], er, energy(e, kept, found)), ncc(c[L], er, energy(e, kept))
    applied = found if c[found + L] > 0 and n_star >= min_corr else 0
    return Result(shift(e, applied), found, applied, c, mag, n_star, n_zero, er, kept)


def planted(n, regions, W, M, L, lag, seed=0, integer=False):
    """(e, r, kept): r = a cut of splice_oracle.signal of length n + 2 L, e[i + lag] = r[i] for every i where both exist -- exactly, then
    divided by 1.7 with white noise of 0.03 added; inside the regions e is independent noise.  ``integer``: both hold integers in [-4, 4],
    e the exact shift (no gain, no noise) outside the regions."""
    assert abs(lag) <= L
    g = np.random.default_rng(seed + 2000)
    if integer:
        x = g.integers(-4, 5, n + 2 * L).astype(np.float64)
    else:
        x = S.signal(n + 2 * L, seed).astype(np.float64)
    r = x[L:L + n]
    e = x[L - lag:L - lag + n].copy()  # e[j] = x[L + j - lag]: e[i + lag] = x[L + i] = r[i]
    if not integer:
        e = (e + 0.03 * g.standard_normal(n)) / 1.7
    for a, b in regions:
        e[a:b] = g.integers(-4, 5, b - a) if integer else 0.2 * g.standard_normal(b - a)
    return e.astype(np.float32), r.astype(np.float32), kept_set(n, regions, W, M, L)


def periodic(n, L, lag, period=8):
    """integer signals of that period, e the exact shift of r by ``lag`` everywhere: c(l) ties at every l = lag + m period"""
    base = np.array([3, -1, 4, 1, -4, 2, -2, 0])[:period]
    x = np.tile(base, (n + 2 * L) // period + 2)
    r = x[L:L + n]
    e = x[L - lag:L - lag + n]
    return e.astype(np.float32), r.astype(np.float32)
