"""Splice a region edit back into the recording it was made from: outside the edited regions the returned samples are the recording's own,
bit for bit; inside they are the edit, brought to the recording's level; the two are joined where they agree best, by a short crossfade.

What every audio editor does when it replaces a region.  The edit ``e`` and the reference ``r`` are mono clips of the same length and rate.

  plan       (host) the regions are sorted and merged where their gap is below 2 M samples.  A region [a, b) has a left seam iff a >= W, with
             its crossfade window starting somewhere in [max(0, a - M), a - W], and a right seam iff n - b >= W, starting in
             [b, min(n, b + M) - W]; where a side has no seam the edit runs to the clip's edge.  At most 4 regions (8 seams).  The kept set is
             every sample outside all [max(0, a - M), min(n, b + M)) spans (each runs to the clip's edge on a side without a seam).
  gain       g = sqrt(sum r^2 / sum e^2) over the kept set (1 if either sum is 0 or not finite), or 1, or a given number; ge = g e.
  seams      the window start of least sum (r - ge)^2 over W samples; ties go to the start nearest the region.  rho = the correlation of r
             and ge over that window, clamped to [0, 1].
  crossfade  with t = (i - s + 0.5) / W, w_e = t (left) or 1 - t (right), w_r = 1 - w_e:
             out = (w_r r + w_e ge) / sqrt(w_r^2 + w_e^2 + 2 rho w_r w_e): the mix keeps the power of two signals of correlation rho
             (Fink, Holters, Zoelzer, DAFx-16).  "linear" is rho = 1, "equal_power" rho = 0.

``plan`` is host code; everything else is ONE HIP launch (``apad_splice``) for a ragged batch, with nothing read back.  **PARITY UNPINNED**:
no other implementation was available; the stage is held to the fp64 restatement in tests/splice_oracle.py and to its identities (the
reference's bits outside the windows, one multiply inside).  A time alignment of edit and reference by one integer lag per clip is the
stage before this one (align.py; ``splice_edit(align=)``).  Not here: a lag per seam or a fractional one, splices in the mel domain or per
frequency band, true peak or limiting.
"""
import collections
import math

import numpy as np
import torch

MAX_REGIONS, MAX_SEAMS, MAX_SPAN, PLAN_INTS = 4, 8, 8192, 32
SHAPES = {"matched": 0, "linear": 1, "equal_power": 2}

Plan = collections.namedtuple("Plan", "n W M regions seams kept")
Plan.__doc__ = """What ``plan`` returns: ``regions`` [(a, b)] merged and sorted, ``seams`` [(left, right)] per region with each side a search
span (lo, hi) in samples -- window starts lie in [lo, hi - W] -- or None, ``kept`` [(lo, hi)] the non-empty intervals the gain is measured on."""


def plan(n, regions, W, M):
    """Step 1 of the module's docstring for a clip of ``n`` samples: ``regions`` [(a, b)] in samples, crossfade length ``W``, search margin
    ``M`` -> Plan.  Pure host code.  ValueError on W < 2, M < W, M > 8192, a region outside 0 <= a < b <= n, no region, more than 4 regions
    after merging, or no kept sample."""
    n, W, M = int(n), int(W), int(M)
    if W < 2:
        raise ValueError(f"splice: a crossfade of W={W} samples is too short (need W >= 2)")
    if M < W:
        raise ValueError(f"splice: the search margin M={M} is shorter than the crossfade W={W}")
    if M > MAX_SPAN:
        raise ValueError(f"splice: the search margin M={M} samples exceeds {MAX_SPAN}")
    regs = sorted((int(a), int(b)) for a, b in regions)
    if not regs:
        raise ValueError("splice: no region: there is nothing to splice in")
    for a, b in regs:
        if not 0 <= a < b <= n:
            raise ValueError(f"splice: region [{a}, {b}) is empty or outside the clip's {n} samples")
    merged = [regs[0]]
    for a, b in regs[1:]:
        if a - merged[-1][1] < 2 * M:
            merged[-1] = (merged[-1][0], max(merged[-1][1], b))
        else:
            merged.append((a, b))
    if len(merged) > MAX_REGIONS:
        raise ValueError(f"splice: {len(merged)} regions ({2 * len(merged)} seams) after merging; at most {MAX_REGIONS} regions ({MAX_SEAMS} seams)")
    seams, kept, cur = [], [], 0
    for a, b in merged:
        left = (max(0, a - M), a) if a >= W else None
        right = (b, min(n, b + M)) if n - b >= W else None
        seams.append((left, right))
        start = left[0] if left else 0
        if start > cur:
            kept.append((cur, start))
        cur = right[1] if right else n
    if cur < n:
        kept.append((cur, n))
    if not kept:
        raise ValueError("splice: no kept sample: the regions and their seams cover the whole clip, there is nothing to splice into")
    return Plan(n, W, M, merged, seams, kept)


def plan_row(p, shape=0, given_gain=False):
    """a Plan as the 32 int32 of apad_splice's table (include/apadapter_hip.h)"""
    row = [len(p.regions), p.W, int(shape), int(bool(given_gain)), p.M, 0, 0, 0]
    for (a, b), (left, right) in zip(p.regions, p.seams):
        row += [a, b, *(left or (-1, -1)), *(right or (-1, -1))]
    return row + [0] * (PLAN_INTS - len(row))


def mask_regions(mask, row_samples, n):
    """An edit mask [rows, columns] (or [b, 1, rows, columns]: one list per clip) -> sample ranges: a latent row is inside a region if any
    of its columns is > 0, and each run of inside rows [r0, r1) becomes [r0 * row_samples, min(r1 * row_samples, n)).  A frequency-band
    mask therefore counts as its rows."""
    m = torch.as_tensor(mask)
    if m.dim() == 4:
        return [mask_regions(c[0], row_samples, n) for c in m]
    inside = (m > 0).any(dim=-1).tolist()
    out, r0 = [], None
    for i, v in enumerate(inside + [False]):
        if v and r0 is None:
            r0 = i
        elif not v and r0 is not None:
            if r0 * row_samples < n:
                out.append((r0 * row_samples, min(i * row_samples, n)))
            r0 = None
    return out


def check_shape(crossfade_shape):
    if not isinstance(crossfade_shape, str) or crossfade_shape not in SHAPES:
        raise ValueError(f"splice: crossfade_shape={crossfade_shape!r}: one of {', '.join(repr(s) for s in SHAPES)}")
    return SHAPES[crossfade_shape]


def check_gain(gain, what="gain"):
    """"kept" -> None (measured on the kept set); None -> 1.0; a positive finite float -> itself"""
    if isinstance(gain, str):
        if gain != "kept":
            raise ValueError(f"splice: {what}={gain!r}: 'kept' (matched on the kept part), None (1) or a positive number")
        return None
    if gain is None:
        return 1.0
    try:
        g = float(gain)
    except (TypeError, ValueError):
        g = float("nan")
    if not (math.isfinite(g) and g > 0.0):
        raise ValueError(f"splice: {what}={gain!r}: 'kept' (matched on the kept part), None (1) or a positive number")
    return g


def check_lengths(sampling_rate, crossfade_s, seam_search_s):
    """seconds -> (W, M) in samples, checked"""
    def number(v):
        try:
            return float(v)
        except (TypeError, ValueError):
            return float("nan")

    sr, c, s = number(sampling_rate), number(crossfade_s), number(seam_search_s)
    if not (math.isfinite(sr) and sr > 0):
        raise ValueError(f"splice: sampling_rate={sampling_rate!r} must be a positive rate in Hz")
    if not (math.isfinite(c) and c > 0) or int(round(c * sr)) < 2:
        raise ValueError(f"splice: crossfade_s={crossfade_s!r} must cover at least 2 samples at {sampling_rate} Hz")
    W = int(round(c * sr))
    if not (math.isfinite(s) and int(round(s * sr)) >= W):
        raise ValueError(f"splice: seam_search_s={seam_search_s!r} must be at least crossfade_s={crossfade_s!r}")
    M = int(round(s * sr))
    if M > MAX_SPAN:
        raise ValueError(f"splice: seam_search_s={seam_search_s!r} is {M} samples at {sampling_rate} Hz, above the {MAX_SPAN} a seam is searched over")
    return W, M


def _region_lists(regions, count, sampling_rate):
    """``regions`` = (t0, t1), a list of them, or one list per clip, in seconds -> per clip a list of (a, b) in samples"""
    def pair(v):
        try:
            t0, t1 = (float(x) for x in v)
        except (TypeError, ValueError):
            raise ValueError(f"splice: regions: {v!r} is not (start_s, end_s)") from None
        if not (math.isfinite(t0) and math.isfinite(t1) and 0.0 <= t0 < t1):
            raise ValueError(f"splice: regions: {v!r}: expected 0 <= start_s < end_s")
        return int(round(t0 * sampling_rate)), int(round(t1 * sampling_rate))

    def scalar(x):
        return isinstance(x, (int, float)) or (hasattr(x, "ndim") and getattr(x, "ndim") == 0)

    if regions is None or isinstance(regions, str) or not hasattr(regions, "__len__") or len(regions) == 0:
        raise ValueError(f"splice: regions={regions!r}: expected (start_s, end_s), a list of them, or one list per clip")
    if scalar(regions[0]):
        return [[pair(regions)]] * count
    if all(hasattr(v, "__len__") and len(v) and scalar(v[0]) for v in regions):
        return [[pair(v) for v in regions]] * count
    if len(regions) != count:
        raise ValueError(f"splice: regions holds {len(regions)} lists for {count} clips")
    return [[pair(v) for v in per] for per in regions]


def run(edit, offsets_host, ref, ref_offsets_host, ref_index, plans, shape=0, gain=None):
    """One apad_splice launch on packed fp32 GPU clips: ``plans`` one Plan per clip, ``ref_index`` clip -> reference (a list), ``gain``
    None = measured on the kept set, or a float -> (out packed as edit, gains fp32 [b], seam starts int32 [b, 8], seam stats fp32 [b, 8, 2])"""
    from . import ops
    dev, B = edit.device, len(plans)
    plan_host = torch.tensor([plan_row(p, shape, gain is not None) for p in plans], dtype=torch.int32)
    idx_host = torch.tensor(list(ref_index), dtype=torch.int32)
    out, gains = torch.empty_like(edit), torch.empty(B, dtype=torch.float32, device=dev)
    starts = torch.empty(B, MAX_SEAMS, dtype=torch.int32, device=dev)
    stats = torch.empty(B, MAX_SEAMS, 2, dtype=torch.float32, device=dev)
    gain_in = None if gain is None else torch.full((B,), float(gain), dtype=torch.float32).to(dev)
    ops.splice(edit, offsets_host.to(dev), offsets_host, ref, ref_offsets_host.to(dev), ref_offsets_host, idx_host.to(dev), idx_host,
               plan_host.to(dev), plan_host, out, gains, starts, stats, gain_in=gain_in)
    return out, gains, starts, stats


def splice_edit(edit, reference, regions, sampling_rate=16000, crossfade_s=0.03, seam_search_s=0.08, crossfade_shape="matched", gain="kept",
                return_plan=False):
    """Splice each edit into its reference: ``(out, gains)``, the spliced clips in the form ``edit`` came in (a tensor of the same shape, or
    a list of 1-D clips) as fp32 on the GPU, and the gains fp32 [b] applied to the edits.

    ``edit``, ``reference``: a tensor / array [samples] or [b, samples], or a ragged list of 1-D clips, mono, both at ``sampling_rate``;
    m references with m dividing b: clip i is spliced into reference i // (b / m), which must have its length.  ``regions``: (start_s,
    end_s), a list of them (shared by all clips), or one list per clip, in seconds; a region's end is cut at the clip's.  ``crossfade_s``:
    the length of each crossfade; ``seam_search_s``: how far outside a region its seams may move (at most 8192 samples).
    ``crossfade_shape``: "matched" (power-complementary for the measured correlation of the two signals in the window), "linear" or
    "equal_power".  ``gain``: "kept" (the edit is brought to the reference's level, measured where both are the kept material), None
    (1), or a number.  Outside the regions and crossfade windows ``out`` holds the reference's samples, bit for bit.
    ``return_plan`` adds the chosen window starts int32 [b, 8] (entry 2 q / 2 q + 1: left / right seam of region q; -1 = no seam), their
    (cost, correlation) fp32 [b, 8, 2] and the host Plans.  One ``apad_splice`` launch; nothing is read back.  The edit is taken as it
    is, sample i against the reference's sample i: ``splice_edit_aligned`` shifts it first."""
    return _splice_edit(edit, reference, regions, sampling_rate, crossfade_s, seam_search_s, crossfade_shape, gain, return_plan)


def splice_edit_aligned(edit, reference, regions, sampling_rate=16000, crossfade_s=0.03, seam_search_s=0.08, crossfade_shape="matched", gain="kept",
                        return_plan=False, align="kept", align_search_s=0.02, align_min_corr=0.5):
    """``splice_edit`` behind a time alignment (align.py), every other argument as there.  ``align``: None = ``splice_edit``; "kept" = each
    edit is first shifted by the integer lag, within +- ``align_search_s`` seconds, that correlates it best with its reference over the
    splice plan's own kept set (shrunk by the search width), provided the normalised correlation reaches ``align_min_corr`` (neither default
    is calibrated on a real decoder); an int = a given lag in samples, positive = the edit is late.  With ``return_plan`` and ``align`` set
    the tuple ends in (lags int32 [b, 2] = (found, applied), align stats fp32 [b, 4]).  Two more launches (``apad_align_corr``,
    ``apad_align_apply``); nothing is read back."""
    return _splice_edit(edit, reference, regions, sampling_rate, crossfade_s, seam_search_s, crossfade_shape, gain, return_plan, align,
                        align_search_s, align_min_corr)


def _splice_edit(edit, reference, regions, sampling_rate, crossfade_s, seam_search_s, crossfade_shape, gain, return_plan, align=None,
                 align_search_s=0.02, align_min_corr=0.5):
    from . import loudness
    if align is not None:
        from . import align as A
        al = A.check_arguments(sampling_rate, align, align_search_s, align_min_corr)
    W, M = check_lengths(sampling_rate, crossfade_s, seam_search_s)
    shape, g = check_shape(crossfade_shape), check_gain(gain)
    try:  # the waveform forms of normalize_loudness, checked by its own code
        lens = loudness._shapes(edit, "edit")
        rlens = loudness._shapes(reference, "reference")
        ridx = loudness.default_ref_index(len(lens), len(rlens))
    except ValueError as err:
        raise ValueError(str(err).replace("loudness:", "splice:", 1)) from None
    for i, n in enumerate(lens):
        if rlens[ridx[i]] != n:
            raise ValueError(f"splice: clip {i} has {n} samples, its reference {ridx[i]} has {rlens[ridx[i]]}")
    per_clip = _region_lists(regions, len(lens), float(sampling_rate))
    plans = [plan(n, [(a, min(b, n)) for a, b in regs if a < n], W, M) for n, regs in zip(lens, per_clip)]
    if align is not None:  # (nothing kept after the search width is taken off: a ValueError before anything is uploaded)
        L, min_corr, lag = al
        if lag is not None and any(abs(lag) >= n for n in lens):
            raise ValueError(f"splice: align={lag} shifts a clip of {min(lens)} samples out of itself")
        aplans = None if lag is not None else [A.plan(p.n, p.kept, L) for p in plans]
    packed, offsets_host, dev = loudness._pack(edit)
    rp, roh, _ = loudness._pack(reference, dev)
    if align is not None:
        packed, lags, astats = A.run(packed, offsets_host, rp, roh, ridx, aplans, min_corr, lag)
    out, gains, starts, stats = run(packed, offsets_host, rp, roh, ridx, plans, shape, g)
    if torch.is_tensor(edit) or isinstance(edit, np.ndarray):
        res = out.reshape(tuple(edit.shape))
    else:
        res = [out[int(offsets_host[i]): int(offsets_host[i + 1])] for i in range(len(lens))]
    if return_plan:
        return (res, gains, starts, stats, plans) + ((lags, astats) if align is not None else ())
    return res, gains
