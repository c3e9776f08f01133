"""Align a re-rendered edit to the recording it is spliced into: one integer lag per clip, found by cross-correlation over the kept part.

The splice (splice.py) joins the recording ``r`` and the vocoder's rendering ``e`` of the edit sample by sample; a decoder path with a
constant latency of a few samples puts every partial out of phase across the crossfades.  This stage measures that latency and removes it.

  lag        l means e[i + l] ~ r[i]: positive = the edit is late.
  plan       (host) the kept intervals [lo, hi) -- where edit and recording hold the same material -- are shrunk by L samples on both
             sides, so that no e[i + l] touches a region or a seam's search span; intervals that become empty are dropped.  K = the rest,
             at most 5 intervals.
  table      c(l) = sum over K of r[i] e[i + l] for l in [-L, L] (``apad_align_corr``, a (chunk of 4096 samples, clip) grid).
  winner     the lag of the largest c; ties go to the smaller |l|, then to l >= 0.
  confidence ncc(l) = c(l) / sqrt(sum_K r[i]^2 sum_K e[i + l]^2) for the winner and for l = 0.
  gate       the lag is applied if c > 0 and ncc >= min_corr, else 0 is.
  output     a[i] = e[i + lag], the same bits; +0.0 where the edit does not reach (``apad_align_apply``).

Two HIP launches for a ragged batch, nothing read back.  **PARITY UNPINNED**: no other implementation was available; the stage is held to the
fp64 restatement in tests/align_oracle.py and to its identities (an exact table on integer signals, the shifted edit's bits).  The
estimator is the plain cross-correlation of Knapp & Carter's family, without a frequency weighting.  Not here: fractional
(sub-sample) lags, a lag per seam or any time-stretching, polarity inversion, alignment in the mel domain.  The defaults
``search_s = 0.02`` and ``min_corr = 0.5`` are NOT calibrated on real decoders (no real weights were available).
"""
import collections
import math

import numpy as np
import torch

MAX_LAG, MAX_INTERVALS, PLAN_INTS, CHUNK = 1024, 5, 16, 4096

Plan = collections.namedtuple("Plan", "n L kept")
Plan.__doc__ = """What ``plan`` returns: ``kept`` [(lo, hi)] the intervals the correlation is summed over, L <= lo < hi <= n - L."""


def plan(n, kept, L):
    """``kept`` [(lo, hi)] in samples of a clip of ``n`` (``splice.plan(...).kept``, or [(0, n)]) and the search half-width ``L`` -> Plan:
    every interval shrunk by L on both sides, the empty ones dropped.  ValueError if L is outside [1, 1024], an interval is outside the
    clip or out of order, none is left or more than 5 are."""
    n, L = int(n), int(L)
    if not 1 <= L <= MAX_LAG:
        raise ValueError(f"align: the search half-width L={L} samples is outside [1, {MAX_LAG}]")
    out, cur = [], 0
    for lo, hi in kept:
        lo, hi = int(lo), int(hi)
        if not cur <= lo < hi <= n:
            raise ValueError(f"align: the kept interval [{lo}, {hi}) is empty, out of order or outside the clip's {n} samples")
        cur = hi
        if lo + L < hi - L:
            out.append((lo + L, hi - L))
    if not out:
        raise ValueError(f"align: no kept sample is left {L} samples away from the regions and the clip's ends: nothing to measure the lag on")
    if len(out) > MAX_INTERVALS:
        raise ValueError(f"align: {len(out)} kept intervals, at most {MAX_INTERVALS}")
    return Plan(n, L, out)


def plan_row(p=None):
    """a Plan as the 16 int32 of the apad_align_* table (include/apadapter_hip.h); None = a given lag"""
    row = [0, 1, 1, 0] if p is None else [len(p.kept), p.L, 0, 0] + [v for iv in p.kept for v in iv]
    return row + [0] * (PLAN_INTS - len(row))


def check_arguments(sampling_rate, align, align_search_s=0.02, align_min_corr=0.5):
    """None -> None; "kept" -> (L in samples, min_corr, None); an int -> (None, None, lag).  ValueError otherwise."""
    if align is None:
        return None
    if isinstance(align, (int, np.integer)) and not isinstance(align, bool):
        if abs(int(align)) >= 2 ** 24:
            raise ValueError(f"align={align!r}: a given lag is below 2^24 samples")
        return None, None, int(align)
    if not (isinstance(align, str) and align == "kept"):
        raise ValueError(f"align={align!r}: None, 'kept' (the lag is measured on the kept part) or an int (a given lag in samples)")

    def number(v):
        try:
            return float(v)
        except (TypeError, ValueError):
            return float("nan")

    sr, s, c = number(sampling_rate), number(align_search_s), number(align_min_corr)
    if not (math.isfinite(sr) and sr > 0):
        raise ValueError(f"align: sampling_rate={sampling_rate!r} must be a positive rate in Hz")
    if not (math.isfinite(s) and 1 <= int(round(s * sr)) <= MAX_LAG):
        raise ValueError(f"align: align_search_s={align_search_s!r} must cover 1 to {MAX_LAG} samples at {sampling_rate} Hz")
    if not -1.0 <= c <= 1.0:
        raise ValueError(f"align: align_min_corr={align_min_corr!r} must lie in [-1, 1]")
    return int(round(s * sr)), c, None


def run(edit, offsets_host, ref, ref_offsets_host, ref_index, plans, min_corr=0.5, lag=None, return_table=False):
    """Both launches on packed fp32 GPU clips: ``plans`` one Plan per clip (measured), or ``lag`` an int or one per clip (given; ``plans``
    is then ignored) -> (aligned packed as edit, lags int32 [b, 2] = (found, applied), stats fp32 [b, 4] = (ncc(l*), ncc(0), c(l*), E_r));
    ``return_table`` adds the table fp32 [b, 2 max L + 1]."""
    from . import ops
    dev, B = edit.device, offsets_host.numel() - 1
    given = lag is not None
    plan_host = torch.tensor([plan_row(None if given else p) for p in (range(B) if given else plans)], dtype=torch.int32)
    idx_host = torch.tensor(list(ref_index), dtype=torch.int32)
    offsets, roffsets, idx, plan_dev = offsets_host.to(dev), ref_offsets_host.to(dev), idx_host.to(dev), plan_host.to(dev)
    out = torch.empty_like(edit)
    lags_out, stats = torch.empty(B, 2, dtype=torch.int32, device=dev), torch.empty(B, 4, dtype=torch.float32, device=dev)
    partial = lag_in = table = None
    if given:
        lag_in = torch.tensor([int(lag)] * B if isinstance(lag, (int, np.integer)) else [int(v) for v in lag], dtype=torch.int32).to(dev)
    else:
        chunks = max(-(-p.n // CHUNK) for p in plans)
        nl = 2 * max(p.L for p in plans) + 1
        partial = torch.empty(B, chunks, nl, dtype=torch.float32, device=dev)
        table = torch.zeros(B, nl, dtype=torch.float32, device=dev) if return_table else None
        ops.align_corr(edit, offsets, offsets_host, ref, roffsets, ref_offsets_host, idx, idx_host, plan_dev, plan_host, partial)
    ops.align_apply(edit, offsets, offsets_host, ref, roffsets, ref_offsets_host, idx, idx_host, plan_dev, plan_host, out, lags_out, stats,
                    0.0 if min_corr is None else float(min_corr), partial=partial, lag_in=lag_in, corr_out=table)
    return (out, lags_out, stats, table) if return_table else (out, lags_out, stats)


def align_edit(edit, reference, regions=None, sampling_rate=16000, search_s=0.02, min_corr=0.5, lag=None, splice_margins=None):
    """Shift each edit by the lag that aligns it to its reference: ``(aligned, lags, stats)`` -- the shifted clips in the form ``edit`` came
    in (a tensor of the same shape, or a list of 1-D clips; fp32 on the GPU; +0.0 where the shifted edit does not reach), lags int32
    [b, 2] = (found, applied) in samples, positive = the edit was late, and stats fp32 [b, 4] = (ncc at the found lag, ncc at lag 0,
    c at the found lag, the reference's energy over the kept set).

    ``edit``, ``reference``: the waveform forms of ``splice_edit``.  ``regions``: None (the whole clip is kept material), or the forms of
    ``splice_edit`` in seconds: the lag is measured outside them.  ``splice_margins`` = (crossfade_s, seam_search_s): the kept set is the
    one ``splice_edit`` would use for these regions; without it, the complement of the regions widened by ``search_s`` on both sides.
    ``search_s``: lags up to +- that many seconds are searched (at most 1024 samples).  ``min_corr``: the found lag is applied only if
    its normalised correlation reaches this, else the edit comes back as it was.  ``lag`` (an int, or one per clip): shift by that many
    samples and measure nothing (stats 0).  Neither default is calibrated on a real decoder."""
    from . import loudness, splice as S
    if lag is None:
        L, min_corr, _ = check_arguments(sampling_rate, "kept", search_s, min_corr)
    try:
        lens = loudness._shapes(edit, "edit")
        rlens = loudness._shapes(reference, "reference")
        ridx = loudness.default_ref_index(len(lens), len(rlens))
    except ValueError as err:
        raise ValueError(str(err).replace("loudness:", "align:", 1)) from None
    for i, n in enumerate(lens):
        if rlens[ridx[i]] != n:
            raise ValueError(f"align: clip {i} has {n} samples, its reference {ridx[i]} has {rlens[ridx[i]]}")
    plans = None
    if lag is not None:
        given = list(lag) if isinstance(lag, (list, tuple)) else [lag] * len(lens)
        if len(given) != len(lens) or any(isinstance(v, bool) or not isinstance(v, (int, np.integer)) for v in given):
            raise ValueError(f"align: lag={lag!r}: an int, or one int per clip ({len(lens)})")
        for v, n in zip(given, lens):
            if abs(int(v)) >= n:
                raise ValueError(f"align: lag={int(v)} shifts a clip of {n} samples out of itself")
        lag = given
    elif regions is None:
        if splice_margins is not None:
            raise ValueError("align: splice_margins describes the seams of regions; without regions= it has no use")
        plans = [plan(n, [(0, n)], L) for n in lens]
    else:
        per_clip = S._region_lists(regions, len(lens), float(sampling_rate))
        if splice_margins is not None:
            W, M = S.check_lengths(sampling_rate, *splice_margins)
            plans = [plan(n, S.plan(n, [(a, min(b, n)) for a, b in regs if a < n], W, M).kept, L) for n, regs in zip(lens, per_clip)]
        else:
            plans = [plan(n, _complement(n, regs, L), L) for n, regs in zip(lens, per_clip)]
    packed, offsets_host, dev = loudness._pack(edit)
    rp, roh, _ = loudness._pack(reference, dev)
    out, lags, stats = run(packed, offsets_host, rp, roh, ridx, plans, min_corr, lag)
    if torch.is_tensor(edit) or isinstance(edit, np.ndarray):
        res = out.reshape(tuple(edit.shape))
    else:
        res = [out[int(offsets_host[i]): int(offsets_host[i + 1])] for i in range(len(lens))]
    return res, lags, stats


def _complement(n, regions, widen):
    """the intervals of [0, n) outside every region widened by ``widen`` samples on both sides"""
    kept, cur = [], 0
    for a, b in sorted((max(0, a - widen), min(n, b + widen)) for a, b in regions if a < n):
        if a > cur:
            kept.append((cur, a))
        cur = max(cur, b)
    if cur < n:
        kept.append((cur, n))
    return kept
