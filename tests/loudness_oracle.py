"""Independent restatement of ITU-R BS.1770-4 integrated loudness (mono, EBU R 128 gating) for the tests: ``scipy.signal.sosfilt`` for
the K-weighting, with coefficients computed HERE (not imported from the package), and plain numpy for the blocks and gates.  float64 by
default; ``dtype=np.float32`` runs the same chain in fp32 on the CPU (coefficients, filter state and every sum in fp32): the yardstick
the GPU tests scale their bounds by.  Neither libebur128 nor pyloudnorm is installed, so this file is the standard restated, anchored
to its own calibration statement (a 0 dBFS 997 Hz sine reads -3.01 LKFS)."""
import math
from collections import namedtuple

import numpy as np
from scipy.signal import sosfilt

SR = 16000
Result = namedtuple("Result", "L block_loudness rel_threshold n_abs n_rel hop_energy")


def _biquad_den(f0, Q, fs):
    K = math.tan(math.pi * f0 / fs)
    a0 = 1.0 + K / Q + K * K
    return K, a0, [1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0]


def sos(fs):
    """[2, 6] float64: the high-shelf (pre-filter) and the RLB high-pass, bilinear designs from the analog prototypes behind the
    standard's 48 kHz table"""
    Q = 0.7071752369554196
    K, a0, a = _biquad_den(1681.974450955533, Q, fs)
    Vh = 10.0 ** (3.999843853973347 / 20.0)
    Vb = Vh ** 0.4996667741545416
    shelf = [(Vh + Vb * K / Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / Q + K * K) / a0] + a
    _, _, a = _biquad_den(38.13547087602444, 0.5003270373238773, fs)
    return np.array([shelf, [1.0, -2.0, 1.0] + a])


def hop_block(fs):
    hop = int(round(0.1 * fs))
    return hop, 4 * hop


def block_count(n, fs=SR):
    hop, block = hop_block(fs)
    return max(0, (n - block) // hop + 1)


def k_weight(x, fs=SR, dtype=np.float64):
    """the K-weighted signal in ``dtype`` (the samples are taken as they are, zero initial state)"""
    return sosfilt(sos(fs).astype(dtype), np.asarray(x).astype(dtype)).astype(dtype)


def loudness(x, fs=SR, dtype=np.float64):
    """x: 1-D samples -> Result(L in LUFS (-inf when no block survives), per-block loudness, the relative threshold in LUFS (nan when no
    block passes the absolute gate), blocks above the absolute gate, blocks above both, the energy of every whole hop)"""
    hop, block = hop_block(fs)
    y = k_weight(x, fs, dtype)
    nh = len(y) // hop
    e = (y[: nh * hop].reshape(nh, hop) ** 2).sum(axis=1, dtype=dtype) if nh else np.zeros(0, dtype)
    nb = block_count(len(y), fs)
    z = np.array([e[j: j + 4].sum(dtype=dtype) / dtype(block) for j in range(nb)], dtype=dtype)
    with np.errstate(divide="ignore"):
        l = dtype(-0.691) + dtype(10) * np.log10(z)
    keep = l > -70.0
    if not keep.any():
        return Result(-math.inf, l, math.nan, 0, 0, e)
    rel = dtype(-0.691) + dtype(10) * np.log10(z[keep].mean(dtype=dtype)) - dtype(10)
    both = keep & (l > rel)
    L = dtype(-0.691) + dtype(10) * np.log10(z[both].mean(dtype=dtype))
    return Result(float(L), l, float(rel), int(keep.sum()), int(both.sum()), e)


def gate_margin(r):
    """the smallest distance in LU of any block from the absolute and from the relative threshold: (abs, rel); inf where there is none"""
    if len(r.block_loudness) == 0:
        return math.inf, math.inf
    a = float(np.abs(r.block_loudness - (-70.0)).min())
    b = float(np.abs(r.block_loudness - r.rel_threshold).min()) if r.n_abs else math.inf
    return a, b


def gain(L, target, peak, peak_limit):
    """the fp64 gain rule: 10^((target - L) / 20), cut to peak_limit / peak when it would take the peak over a positive limit; 1 when L or
    the target is not finite or the peak is 0"""
    if not (math.isfinite(L) and math.isfinite(target)) or peak == 0:
        return 1.0
    g = 10.0 ** ((target - L) / 20.0)
    if peak_limit > 0 and g * peak > peak_limit:
        g = peak_limit / peak
    return g


def signal(n, fs=SR):
    """the tests' clip of n samples: two sines and noise under a three-level envelope (full, -30 dB, 1e-5), float32 -- loud, quiet and
    sub-gate stretches, so both gates have blocks on either side"""
    rng = np.random.default_rng(n)
    t = np.arange(n, dtype=np.float64) / fs
    x = 0.1 * np.sin(2 * np.pi * 220 * t) + 0.05 * np.sin(2 * np.pi * 1760 * t + 1) + 0.02 * rng.standard_normal(n)
    env = np.full(n, 1e-5)
    env[: int(0.45 * n)] = 1.0
    env[int(0.45 * n): int(0.75 * n)] = 10.0 ** (-30 / 20)
    return (x * env).astype(np.float32)
