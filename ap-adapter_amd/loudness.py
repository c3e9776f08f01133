"""Loudness on the GPU: ITU-R BS.1770-4 integrated loudness (LUFS) of mono clips with the EBU R 128 gates, and the gain that takes a clip
to a target loudness -- a number, or the loudness of another clip (an edit matched to its source) -- under a sample-peak guard.

``integrated_loudness`` is the standard's measure for one channel: the K-weighting (a high-shelf and a 38 Hz high-pass biquad, designed
here for the clip's own rate from the analog prototypes that reproduce the standard's 48 kHz table), the mean square of 400 ms blocks every
100 ms, the absolute gate at -70 LUFS and the relative gate 10 LU below the loudness of what passed it.  **PARITY UNPINNED** against
libebur128 / pyloudnorm (neither is a dependency, neither was available): the feature is pinned to the standard's coefficient table, to
its calibration statement (a full-scale 997 Hz sine reads -3.01 LKFS) and to fp64 ``scipy.signal.sosfilt`` in tests/loudness_oracle.py.
Not here: true peak (the oversampled peak; the guard is on the SAMPLE peak), loudness range, multichannel weighting, any limiter.

The measurement (``apad_loudness``) and the gain (``apad_loudness_gain``) are one HIP launch each for a ragged batch; the host designs the
filter, takes the powers of its transition matrix the kernel scans the recursion with, and checks arguments.
"""
import math

import numpy as np
import torch

from . import ops
from .derived import derived

SR = 16000
RUN, N_POWERS = 8, 65            # samples per lane of the kernel's scan; M^0 .. M^64, M = A^RUN
MAX_HOP, MAX_HOPS = 8192, 3072   # what apad_loudness takes: samples per hop, whole hops per clip
MIN_RATE, MAX_RATE = 4000, 81920


def _check_rate(sampling_rate):
    sr = float(sampling_rate)
    if not (math.isfinite(sr) and MIN_RATE <= sr <= MAX_RATE):
        raise ValueError(f"loudness: sampling_rate={sampling_rate!r} is outside [{MIN_RATE}, {MAX_RATE}] Hz")
    return sr


def k_weighting(sampling_rate):
    """The K-weighting of BS.1770-4 at ``sampling_rate``: float64 sos [2, 6] = (b0 b1 b2 1 a1 a2) of the high-shelf, then of the high-pass
    (scipy's layout).  The bilinear designs whose 48 kHz values are the standard's table to every printed digit."""
    fs = _check_rate(sampling_rate)

    def den(K, Q):
        a0 = 1.0 + K / Q + K * K
        return a0, [1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0]

    K, Q = math.tan(math.pi * 1681.974450955533 / fs), 0.7071752369554196
    Vh = 10.0 ** (3.999843853973347 / 20.0)
    Vb = Vh ** 0.4996667741545416
    a0, a = den(K, Q)
    shelf = [(Vh + Vb * K / Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / Q + K * K) / a0] + a
    _, a = den(math.tan(math.pi * 38.13547087602444 / fs), 0.5003270373238773)
    return np.array([shelf, [1.0, -2.0, 1.0] + a], dtype=np.float64)


def hop_block(sampling_rate):
    """(hop, block) in samples: 100 ms rounded to an integer, and four hops (400 ms)"""
    hop = int(round(0.1 * _check_rate(sampling_rate)))
    return hop, 4 * hop


def block_count(n, sampling_rate=SR):
    """400 ms blocks at 100 ms steps in a clip of ``n`` samples: max(0, (n - block) // hop + 1)"""
    hop, block = hop_block(sampling_rate)
    return max(0, (int(n) - block) // hop + 1)


def transition_powers(sos, run=RUN, count=N_POWERS):
    """float64 [2, count, 2, 2]: per section M^j, M = A^run, A the zero-input transition of what the kernel scans -- the shelf in the
    transposed direct form II (state: its two delay registers), and the high-pass's all-pole half y[n] = w[n] - a1 y[n-1] - a2 y[n-2]
    in the coordinates (y[n-1], y[n-1] - y[n-2]), value and difference (its numerator is applied to the shelf's output beforehand and
    needs no scan).  In (y[n-1], y[n-2]) the 38 Hz mode's powers hold entries near +50 and -50 that multiply two nearly equal numbers, and
    every fp32 product rounds at 50 times the size of the result; in value and difference the large entry multiplies the small
    difference.  ``sos`` are the coefficients the kernel runs (the fp32-rounded ones), as float64."""
    (_, _, _, _, a1, a2), (_, _, _, _, c1, c2) = np.asarray(sos, dtype=np.float64)
    out = np.empty((2, count, 2, 2))
    T = np.array([[1.0, 0.0], [1.0, -1.0]])  # (a, b) <-> (a, a - b): its own inverse
    for sec, A in enumerate((np.array([[-a1, 1.0], [-a2, 0.0]]), T @ np.array([[-c1, -c2], [1.0, 0.0]]) @ T)):
        M = np.linalg.matrix_power(A, run)
        out[sec, 0] = np.eye(2)
        for j in range(1, count):
            out[sec, j] = out[sec, j - 1] @ M
    return out


_SOS64 = {}  # rate -> the float64 design on the host: the tensor the device tables derive from


def tables(dev, sampling_rate=SR):
    """(coef fp32 [10] = (b0 b1 b2 a1 a2) x 2, powers fp32 [2, 65, 2, 2, 2]) on ``dev``, from the derived-weight cache: the fp64 design
    rounded to fp32, and the powers of the ROUNDED recursions' transition matrices, taken in fp64 and split once into hi + lo fp32 pairs
    ([section, j, hi / lo, row, column])"""
    sr = _check_rate(sampling_rate)
    if sr not in _SOS64:
        _SOS64[sr] = torch.from_numpy(k_weighting(sr))
    sos64 = _SOS64[sr]

    def make():
        sos32 = sos64.numpy().astype(np.float32)
        coef = np.ascontiguousarray(sos32[:, [0, 1, 2, 4, 5]].reshape(10))
        p64 = transition_powers(sos32.astype(np.float64))
        hi = p64.astype(np.float32)
        powers = np.stack([hi, (p64 - hi.astype(np.float64)).astype(np.float32)], axis=2)
        return torch.from_numpy(coef).to(dev), torch.from_numpy(np.ascontiguousarray(powers)).to(dev)

    return derived(sos64, ("loudness_tables", str(dev)), make)


def check_target(target, count=None, what="target"):
    """a finite float, or ``count`` of them -> list of floats (ValueError otherwise)"""
    try:
        vals = [float(target)] if not hasattr(target, "__len__") else [float(v) for v in target]
    except (TypeError, ValueError):
        raise ValueError(f"loudness: {what}={target!r} is not a loudness in LUFS (a float, or one per clip)") from None
    if isinstance(target, str) or not all(math.isfinite(v) for v in vals):
        raise ValueError(f"loudness: {what}={target!r} must be finite (LUFS)")
    if hasattr(target, "__len__") and count is not None and len(vals) != count:
        raise ValueError(f"loudness: {what} holds {len(vals)} values for {count} clips")
    return vals


def peak_limit(peak_limit_db):
    """dB relative to full scale (<= 0) -> the linear sample-peak limit; None -> 0 = no guard"""
    if peak_limit_db is None:
        return 0.0
    try:
        p = float(peak_limit_db)
    except (TypeError, ValueError):
        p = float("nan")
    if not p <= 0.0:
        raise ValueError(f"loudness: peak_limit_db={peak_limit_db!r} must be <= 0 dB relative to full scale (None = no guard)")
    return 10.0 ** (p / 20.0)


def _shapes(wav, what="wav"):
    """the clip lengths of a tensor / array [n] or [b, n] or of a list of 1-D clips, checked on the host"""
    if torch.is_tensor(wav) or isinstance(wav, np.ndarray):
        shp = tuple(wav.shape)
        if len(shp) not in (1, 2) or 0 in shp:
            raise ValueError(f"loudness: {what} {shp}: expected a non-empty waveform [samples] or [b, samples]")
        return [shp[-1]] * (1 if len(shp) == 1 else shp[0])
    lens = [tuple(np.shape(c)) for c in wav]
    if not lens or any(len(s) != 1 or s[0] == 0 for s in lens):
        raise ValueError(f"loudness: {what}: every clip must be a non-empty 1-D waveform")
    return [s[0] for s in lens]


def _pack(wav, device=None):
    """wav -> (packed fp32 [sum n] on the GPU, offsets_host int64 [b + 1], device)"""
    if torch.is_tensor(wav) or isinstance(wav, np.ndarray):
        t = torch.as_tensor(wav)
        clips = [t] if t.dim() == 1 else list(t)
    else:
        clips = [c if torch.is_tensor(c) else torch.as_tensor(np.asarray(c, dtype=np.float32)) for c in wav]
    dev = device if device is not None else next((c.device for c in clips if c.is_cuda), None)
    if dev is None:
        if not torch.cuda.is_available():
            raise RuntimeError("loudness: expected GPU waveforms (or a GPU to upload them to); the HIP path has no CPU fallback")
        dev = torch.device("cuda", torch.cuda.current_device())
    offsets_host = torch.zeros(len(clips) + 1, dtype=torch.int64)
    offsets_host[1:] = torch.cumsum(torch.tensor([c.numel() for c in clips], dtype=torch.int64), 0)
    whole = torch.is_tensor(wav) and wav.device == dev and wav.dtype == torch.float32 and wav.is_contiguous()
    packed = wav.reshape(-1) if whole else torch.cat([c.to(device=dev, dtype=torch.float32).reshape(-1) for c in clips])
    return packed, offsets_host, dev


def measure(packed, offsets, offsets_host, sampling_rate=SR, hop_energy=False):
    """stats fp32 [b, 4] = (LUFS, sample peak, blocks above the absolute gate, blocks above both) of packed clips, one launch; with
    ``hop_energy`` also fp32 [b, longest clip's whole hops (at least 1)]: the K-weighted energy of every whole 100 ms hop"""
    hop, _ = hop_block(sampling_rate)
    lens = (offsets_host[1:] - offsets_host[:-1])
    if int(lens.max()) // hop > MAX_HOPS:
        raise ValueError(f"loudness: a clip of {int(lens.max())} samples has more than {MAX_HOPS} hops of {hop}")
    b = lens.numel()
    stats = torch.empty(b, 4, dtype=torch.float32, device=packed.device)
    he = torch.empty(b, max(1, int(lens.max()) // hop), dtype=torch.float32, device=packed.device) if hop_energy else None
    ops.loudness(packed, offsets, offsets_host, *tables(packed.device, sampling_rate), stats, hop, hop_energy=he)
    return (stats, he) if hop_energy else stats


def integrated_loudness(wav, sampling_rate=16000, return_stats=False):
    """BS.1770-4 integrated loudness of each clip, fp32 [b] in LUFS on the GPU (-inf for a clip shorter than 400 ms or silent throughout);
    ``return_stats`` gives fp32 [b, 4] = (LUFS, sample peak, blocks above the absolute gate, blocks above both gates) instead.  ``wav``: a
    tensor / array [samples] or [b, samples], or a ragged list of 1-D clips, mono, at ``sampling_rate`` (measured at that rate: the
    filter is designed for it, nothing is resampled).  One ``apad_loudness`` launch; nothing is read back."""
    hop_block(sampling_rate)
    _shapes(wav)
    packed, offsets_host, dev = _pack(wav)
    stats = measure(packed, offsets_host.to(dev), offsets_host, sampling_rate)
    return stats if return_stats else stats[:, 0]


def default_ref_index(n, m):
    """clip i of n -> reference i // (n / m): each reference serves a run of n / m consecutive clips"""
    if m <= 0 or n % m != 0:
        raise ValueError(f"loudness: {m} references for {n} clips (need a divisor)")
    return [i // (n // m) for i in range(n)]


def normalize_loudness(wav, target=None, reference=None, peak_limit_db=-1.0, sampling_rate=16000, return_stats=False):
    """Bring every clip to a target loudness: ``(wav, gains)``, the clips times one gain each, in the form they came in (a tensor of the
    same shape, or a list of 1-D clips) as fp32 on the GPU, and the linear gains fp32 [b].

    ``target``: LUFS, a float or one per clip (default -14.0, the common streaming level).  ``reference`` instead: waveforms of the same
    forms, m of them with m dividing b; clip i is matched to the loudness of reference i // (b / m) -- an edit to its source.  Giving
    both is an error.  ``peak_limit_db`` (<= 0 dBFS, None = off): a gain that would take the clip's largest sample over the limit is cut to
    the one that puts it on the limit, so the clip ends below its target, never clipped.  This is a sample-peak guard, not the
    standard's true peak.  A clip with no loudness (-inf: shorter than 400 ms, or silent) and a reference without one keep gain 1.
    ``return_stats`` adds the fp32 [b, 4] measurement of the INPUT clips.  Two launches (three with a reference); nothing is read back."""
    if target is not None and reference is not None:
        raise ValueError("loudness: give target= or reference=, not both")
    lens = _shapes(wav)
    limit = peak_limit(peak_limit_db)
    hop_block(sampling_rate)
    if reference is None:
        tvals = check_target(-14.0 if target is None else target, len(lens))
        tvals = tvals * len(lens) if len(tvals) == 1 else tvals
    else:
        ridx = default_ref_index(len(lens), len(_shapes(reference, "reference")))
    packed, offsets_host, dev = _pack(wav)
    offsets = offsets_host.to(dev)
    stats = measure(packed, offsets, offsets_host, sampling_rate)
    out, gains = torch.empty_like(packed), torch.empty(len(lens), dtype=torch.float32, device=dev)
    if reference is None:
        ops.loudness_gain(packed, offsets, offsets_host, stats, out, gains, limit, target=torch.tensor(tvals, dtype=torch.float32).to(dev))
    else:
        rp, roh, _ = _pack(reference, dev)
        ref_stats = measure(rp, roh.to(dev), roh, sampling_rate)
        idx_host = torch.tensor(ridx, dtype=torch.int32)
        ops.loudness_gain(packed, offsets, offsets_host, stats, out, gains, limit, ref_stats=ref_stats, ref_index=idx_host.to(dev),
                          ref_index_host=idx_host)
    if torch.is_tensor(wav) or isinstance(wav, np.ndarray):
        res = out.reshape(tuple(wav.shape))
    else:
        res = [out[int(offsets_host[i]): int(offsets_host[i + 1])] for i in range(len(lens))]
    return (res, gains, stats) if return_stats else (res, gains)
