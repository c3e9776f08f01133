"""The case table of tests/test_gpu_exact_spectral.py: the waveform front-ends of csrc/frontend.hip held to impulses, bin-centred tones and
NaN neighbours.  Its conditions are checked on the CPU by tests/test_spectral_exact_host.py.

Three signal families, each built in fp32 on the CPU:
  impulse   one or two samples of +-0.5 (2^-6 for CLAP): a flat spectrum of known height, and a sample index marked with the window weight of the
            position it is read at -- a read one sample off, a reflection that repeats the edge, a repeat seam one sample off each move it.
  tone      A cos(2 pi k i / N) from a table with the cosine's exact symmetries (so the sum over whole periods is exactly 0 and the peak exactly
            A): under the periodic Hann window an interior frame holds bins k - 1, k, k + 1 (N/8, N/4, N/8 of A) and nothing else, so a filter
            that touches none of them sits at its floor, bit for bit.
  dyadic    multiples of 2^-10 (apad_wav_stats: the fp64 sum is exact).
The resampler of an impulse returns its own table; no rounding is involved.

Every expectation comes from the definition in float64: this file's own index map of the framing (reflection, repeat, crop, zero padding), the
fp64 window, ``numpy.fft`` of the framed samples, the oracle's fp64 filter table, the logarithm.  ``restate32`` is the same chain in fp32 numpy in
the kernels' order (bit-reversed load, radix-2 decimation in time with the fp32 twiddle table, the filter sums lane by lane): the host test holds
it to the bound below, and the GPU test measures the device logarithm against the fp64 logarithm of its argument.

THE BOUND (derived from the kernels' order of operations, never from a run).  u = 2^-24.  With y_j the windowed samples of a frame, S = sum |y_j|
and L = log2 N, every bin of the fp32 transform satisfies

    |X_k - X_k(exact)| <= G u S,    G = 2 + (L - 2) (sqrt 5 + 1) + L

  2             the window table's rounding and the product v * window[j];
  (L - 2) (..)  X_k is a sum of N terms y_j w^(jk) built by L butterfly stages; a term passes at most L twiddle products, of which those of stages
                1 and 2 are by 1 and -i (exact up to 6e-17): a complex product without fma errs by at most sqrt 5 u of its modulus (Brent,
                Percival, Zimmermann 2007) and the rounded twiddle by u more;
  L             one addition per stage, each at most u of its result, and every partial result is at most the sum of the moduli of its terms.
For an impulse S = |y_p| = |X_k|, so this is G u relative (38 u at N = 1024); for a tone S = 0.32 N A against a peak of N A / 4, 1.27 G u of the
peak IN EVERY BIN, which a wide filter sums over its whole row.  A tone is better served by the same count taken in the 2-norm: a stage maps its
input by sqrt 2 times a unitary matrix, its rounding adds at most (sqrt 5 + 1) u sqrt 2 ||b half|| + u ||out|| <= (sqrt 5 + 2) u ||out||, and later
stages scale that like the signal, so over all N bins

    ||X - X(exact)||_2 <= Gn u sqrt N ||y||_2,    Gn = 2 + (L - 2) (sqrt 5 + 2) + 2    (window; stages 3..L; the additions of stages 1, 2)

and a filter's sum of |X_k| errs by at most ||W_row||_2 times that (Cauchy-Schwarz; for a power spectrum 2 ||W o |X| ||_2 ||dX||_2 +
max W ||dX||_2^2).  Every entry takes the smaller of the two counts.  Then
  magnitude     sqrt(re^2 + im^2): two products and a sum (2 u of the power, u of the modulus) and a square root within one ulp: 3 u |X_k|;
  power         re^2 + im^2: 2 u |X_k|^2, and 2 |X_k| dX + dX^2 from the transform;
  filter        non-negative terms, so relative to the sum: u for each weight's rounding plus one u per fma / add of the chain a term passes
                (mel kernels: ceil((hi - lo) / 4) fma + 2 shuffles; fbank: the hi - lo non-zero weights in sequence; chroma: 5 fma + 6
                shuffles + 3 adds);
  logarithm     out lies between log max(e - de, floor) and log max(e + de, floor) (the clamp and the logarithm are monotone), plus LOG_TOL: the
                device logarithm's own error, the ONE MEASURED term (its accuracy is documented nowhere in this project or the installed ROCm):
                4 x the largest |out - log64(argument of restate32)| seen on the MI355X, recorded in DESIGN.md.
At N = 1024 with the widest of the 64 Slaney filters (61 bins) this is 38 + 3 + 19 = 60 u = 3.6e-6 on an impulse's filter energy.  On a tone
the transform's error is absolute -- ||dX||_2 <= 38 u x 32 x 6.9 = 5.0e-4 for A = 0.5 -- so the bound of a filter is that times ||W_row||_2 over
its energy: 2e-6 to 1.8e-5 for the filter whose peak the tone sits on (the Slaney normalisation makes the high filters weak), more for a filter
that the tone touches only with the foot of its triangle.  The restatement's own error on these cases is below 3 % of the bound.

Floors.  An entry is FLOOR when its fp64 energy is at most floor / 8 and restate32's leaked energy is too (the worst-case count above cannot
certify a floor: G u S rowsum is 2.4e-5 for a tone at A = 0.5, the restatement leaks 2e-7); it must then be the floor's value in every bit.
It is LIVE when e >= 8 floor and BAND in between.  The frames a case is built for (an impulse case's frames that read one marked sample, a tone
case's interior frames) hold no BAND entry; the other frames (two marked samples with a spectral null between them, a tone cut by a reflection
or a seam) are compared with the same bound, which stays valid through the clamp.  apad_kaldi_fbank is the exception: nothing is bin-centred in
a 400-sample frame of a 512-point transform and kaldi's pre-emphasis puts a null under the lowest filters, so its floors are only those the
derived bound certifies (e + de <= eps / 8) and its BAND entries are compared like the others.

Unobservable by construction: the Nyquist bin (the ``tid == 0`` lane) of apad_stft_logmel, whose Slaney weight is exactly 0 for f_max = the
Nyquist frequency, and of apad_clap_logmel at its default f_max = 14 kHz.  The lane is covered in apad_chroma (tones at bins 1023 and 1024) and in
apad_clap_logmel by the 16-filter extractor with frequency_max = 26 kHz, whose last filter weighs bin 512 by 6.7e-5.
"""
import functools
import math
import types

import numpy as np
import torch

import chroma_oracle as CO
import clap_feature_models as CF
import vae_mel_oracle as MO
from oracle import fbank as OF

U = 2.0 ** -24
F32 = np.float32
MUTATION_FACTOR = 64.0
FLOOR_ROOM = 8.0

# MEASURED (see the module docstring): 4 x the largest |out - log64(argument of restate32)| seen on the MI355X, in the output's units, over the
# live entries whose derived part allows at most 3e-5 on the argument.  Seen: logf 1.42e-6 (log-mel), 10 log10f 1.23e-5 dB (CLAP), __logf
# 1.77e-7 normalised = 1.6e-6 in the logarithm (fbank).  test_gpu_exact_spectral.py::test_zz_figures fails if a run sees more than a quarter.
LOG_TOL = {"mel": 5.7e-6, "clap": 4.9e-5, "fbank": 7.1e-7, "chroma": 0.0}


# ---- shared arithmetic ----
@functools.lru_cache(None)
def bitrev(log2n):
    n = 1 << log2n
    r = np.zeros(n, np.int64)
    for b in range(log2n):
        r |= ((np.arange(n) >> b) & 1) << (log2n - 1 - b)
    return r


def twiddles(N):
    k = np.arange(N // 2, dtype=np.float64)
    return np.stack([np.cos(2 * np.pi * k / N), -np.sin(2 * np.pi * k / N)], axis=1)


def radix2(y, log2n, tw):
    """The kernels' transform (fft_radix2 / fbank_kernel's loop) in y's dtype: y [F, N] real, natural order -> (re, im) [F, N]"""
    y = np.asarray(y)
    N = 1 << log2n
    tw = np.asarray(tw, y.dtype)
    re, im = np.zeros_like(y), np.zeros_like(y)
    re[:, bitrev(log2n)] = y
    bf = np.arange(N // 2)
    for s in range(1, log2n + 1):
        half = 1 << (s - 1)
        grp, pos = bf >> (s - 1), bf & (half - 1)
        i0 = grp * (half << 1) + pos
        i1 = i0 + half
        wr, wi = tw[pos << (log2n - s), 0], tw[pos << (log2n - s), 1]
        ar, ai, br, bi = re[:, i0], im[:, i0], re[:, i1], im[:, i1]
        tr, ti = br * wr - bi * wi, br * wi + bi * wr
        re[:, i0], im[:, i0], re[:, i1], im[:, i1] = ar + tr, ai + ti, ar - tr, ai - ti
    return re, im


def fma32(a, b, c):
    """fp32 fma: the product of two fp32 numbers is exact in fp64"""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F32)


@functools.lru_cache(None)
def cos_table(N):
    """fp32 cos(2 pi m / N), m < N, with t[N - m] = t[m], t[N/2 + m] = -t[m] and t[N/4] = 0 holding exactly"""
    q = N // 4
    c = np.cos(2 * np.pi * np.arange(q + 1) / N)
    c[q] = 0.0
    t = np.zeros(N)
    t[:q + 1] = c
    t[q + 1:N // 2 + 1] = -c[q - 1::-1]
    t[N // 2 + 1:] = t[1:N // 2][::-1]
    return t.astype(F32)


def tone(k, n, amp, N):
    """fp32 amp cos(2 pi k i / N), i < n (amp a power of two: the scaling is exact)"""
    return (F32(amp) * cos_table(N)[(k * np.arange(n, dtype=np.int64)) % N]).astype(F32)


def impulses(n, marks):
    x = np.zeros(n, F32)
    for s, a in marks:
        assert 0 <= s < n and x[s] == 0, (n, marks)
        x[s] = a
    return x


def shifted(marks, d, n):
    """the marks moved by d samples (a mark that would leave the clip stays)"""
    return [(s + d if 0 <= s + d < n else s, a) for s, a in marks]


# ---- the kernels' constants: fp32 operands from the product's own host tables, fp64 from the definition / the oracles ----
class Spec:
    pass


def _ranges(fb32):
    r = np.zeros((fb32.shape[0], 2), np.int64)
    for i in range(fb32.shape[0]):
        nz = np.nonzero(fb32[i])[0]
        if nz.size:
            r[i] = (nz[0], nz[-1] + 1)
    return r


@functools.lru_cache(None)
def spec(kind, feature_size=64, fmax=14000):
    from ap_adapter_amd import chroma as PC
    from ap_adapter_amd import clap_features as PF
    from ap_adapter_amd import frontend as FE
    cpu = torch.device("cpu")
    s = Spec()
    s.kind = kind
    if kind == "mel":
        w, tw, fb, rng = (t.numpy() for t in FE._logmel_tables(cpu))
        s.log2n, s.hop, s.power, s.floor = 10, 160, False, float(F32(1e-5))
        s.fb64 = MO.mel_filters()
        s.window64 = MO.hann_periodic(1024)
    elif kind == "clap":
        fe = PF.ClapFeatureExtractor(feature_size=feature_size, frequency_max=fmax, truncation="rand_trunc")
        w, tw, fb, rng = (t.numpy() for t in fe.tables(cpu))
        s.log2n, s.hop, s.power, s.floor = 10, 480, True, float(F32(1e-10))
        s.installed = CF.installed(feature_size=feature_size, frequency_max=fmax)
        s.fb64 = np.ascontiguousarray(np.asarray(s.installed.mel_filters_slaney, np.float64).T)
        s.window64 = MO.hann_periodic(1024)
        s.feature_size, s.fmax = feature_size, fmax
    elif kind == "chroma":
        w, tw, fb = (t.numpy() for t in PC.tables(cpu))
        rng = None
        s.log2n, s.hop, s.power, s.floor = 11, 512, True, 0.0
        s.fb64 = CO.filterbank()
        s.window64 = MO.hann_periodic(2048)
    else:
        assert kind == "fbank"
        w, tw, fb = (t.numpy() for t in FE._fbank_tables(cpu, 128))
        rng = None
        s.log2n, s.hop, s.power, s.floor = 9, 160, True, float(OF.EPS)
        s.fb64 = OF.mel_banks(128).astype(np.float64)  # kaldi builds its banks in fp32: the fp32 table is the definition
        n = np.arange(400, dtype=np.float64)
        s.window64 = np.concatenate([0.5 - 0.5 * np.cos(2 * np.pi * n / 399), np.zeros(112)])
        w = np.concatenate([w, np.zeros(112, F32)])
        s.norm_mean = float(F32(FE.NORM_MEAN))
        s.inv_2std = float(F32(1.0) / (F32(2.0) * F32(FE.NORM_STD)))
    s.N = 1 << s.log2n
    s.window32, s.tw32, s.fb32 = w, tw, fb
    s.tw64 = twiddles(s.N)
    s.ranges = _ranges(fb) if rng is None else rng.astype(np.int64)
    width = s.ranges[:, 1] - s.ranges[:, 0]
    # fma / add steps a term of the filter sum passes, + 1 for the weight's own rounding
    s.steps = {"mel": np.ceil(width / 4) + 2, "clap": np.ceil(width / 4) + 2, "fbank": width.astype(np.float64),
               "chroma": np.full(12, 14.0)}[kind] + 1.0
    s.G = 2.0 + (s.log2n - 2) * (math.sqrt(5.0) + 1.0) + s.log2n
    s.Gn = 2.0 + (s.log2n - 2) * (math.sqrt(5.0) + 2.0) + 2.0
    return s


def spectrum64(sp, frames, tw=None):
    """fp64: windowed frames -> (|X_k| [F, N/2 + 1], S = sum |y_j| [F], S2 = ||y||_2 [F]); ``tw``: a (mutated) twiddle table for the kernels'
    transform, else numpy's"""
    y = np.asarray(frames, np.float64) * sp.window64[None, :]
    if tw is None:
        X = np.fft.rfft(y, axis=1)
    else:
        re, im = radix2(y, sp.log2n, tw)
        X = (re + 1j * im)[:, :sp.N // 2 + 1]
    return np.abs(X), np.abs(y).sum(axis=1), np.sqrt((y * y).sum(axis=1))


def energies64(sp, A, fb=None):
    fb = sp.fb64 if fb is None else fb
    return (A * A if sp.power else A) @ fb.T


def energy_bound(sp, A, S, e, dy=None, S2=None):
    """the module docstring's bound on the filter energies, [F, rows]: the smaller of the bin-wise and the norm-wise count.  ``dy`` = (1-norm,
    2-norm) per frame of the error the windowed samples already carry (fbank's preparation): a bin moves by at most the 1-norm, the whole
    spectrum by sqrt N times the 2-norm (Parseval)"""
    extra, extra2 = (0.0, 0.0) if dy is None else dy
    dX = (sp.G * U * S + extra)[:, None]
    dP = 2.0 * A * dX + dX * dX + 2.0 * U * A * A if sp.power else dX + 3.0 * U * A
    de = dP @ sp.fb64.T
    if S2 is not None:
        nX = (math.sqrt(sp.N) * (sp.Gn * U * S2 + extra2))[:, None]  # ||dX||_2 over all bins
        if sp.power:
            w2 = np.sqrt((A * A) @ (sp.fb64 * sp.fb64).T)  # || W o |X| ||_2 per row
            dn = 2.0 * w2 * nX + sp.fb64.max(axis=1)[None, :] * nX * nX + 2.0 * U * e
        else:
            dn = np.sqrt((sp.fb64 * sp.fb64).sum(axis=1))[None, :] * nX + 3.0 * U * e
        de = np.minimum(de, dn)
    return de + sp.steps[None, :] * U * e


def restate32(sp, frames32):
    """fp32, the kernels' order: frames [F, N] fp32 (what the kernel multiplies by the window) -> filter energies [F, rows] fp32"""
    y = np.asarray(frames32, F32) * sp.window32[None, :]
    re, im = radix2(y, sp.log2n, sp.tw32)
    K = sp.N // 2 + 1
    P = re[:, :K] * re[:, :K] + im[:, :K] * im[:, :K]
    if not sp.power:
        P = np.sqrt(P)
    F, R = P.shape[0], sp.fb32.shape[0]
    e = np.zeros((F, R), F32)
    if sp.kind in ("mel", "clap"):  # 4 lanes per filter, bins lo + lane, + 4, ...; (lane 0 + lane 1) + (lane 2 + lane 3)
        for r in range(R):
            lo, hi = sp.ranges[r]
            lane = []
            for l in range(4):
                acc = np.zeros(F, F32)
                for k in range(lo + l, hi, 4):
                    acc = fma32(np.full(F, sp.fb32[r, k], F32), P[:, k], acc)
                lane.append(acc)
            e[:, r] = (lane[0] + lane[1]) + (lane[2] + lane[3])
    elif sp.kind == "fbank":  # one thread per filter, bins in order
        acc = np.zeros((F, R), F32)
        for k in range(K):
            if sp.fb32[:, k].any():
                acc = fma32(np.broadcast_to(sp.fb32[None, :, k], (F, R)), np.broadcast_to(P[:, k, None], (F, R)), acc)
        e = acc
    else:  # chroma: thread t owns bins t + 256 r; lane -> wave (xor butterfly) -> waves 0..3 in order
        acc = np.zeros((F, 256, R), F32)
        for r5 in range(5):
            k = np.arange(256) + 256 * r5
            k = k[k < K]
            acc[:, :k.size] = fma32(np.broadcast_to(sp.fb32.T[None, k, :], (F, k.size, R)), np.broadcast_to(P[:, k, None], (F, k.size, R)),
                                    acc[:, :k.size])
        v = acc.reshape(F, 4, 64, R)
        for o in (32, 16, 8, 4, 2, 1):
            v = v + v[:, :, np.arange(64) ^ o]
        e = ((v[:, 0, 0] + v[:, 1, 0]) + v[:, 2, 0]) + v[:, 3, 0]
    return e


def post64(sp, e):
    """filter energies -> the kernel's output, fp64"""
    if sp.kind == "mel":
        return np.log(np.maximum(e, sp.floor))
    if sp.kind == "clap":
        return np.where(e <= sp.floor, -100.0, 10.0 * np.log10(np.maximum(e, 1e-300)))
    if sp.kind == "fbank":
        return (np.log(np.maximum(e, sp.floor)) - sp.norm_mean) * sp.inv_2std
    m = np.abs(e).max(axis=1, keepdims=True)
    return e / np.where(m < CO.TINY32, 1.0, m)


# what the MI355X's logarithms return at the floors' arguments (MEASURED, part of the same term as LOG_TOL: logf(1e-5f) comes out 2 ulp below the
# correctly rounded -11.512925; fbank's __logf(2^-23), normalised, 1 ulp below).  Every floored entry must be this value in every bit.
# After a ROCm upgrade that changes the math library: run test_wav_stats_of_a_constant_clip (every entry of a constant clip is logf(1e-5f)) and
# any fbank case (the padding-free rows of filter 3, which has no weight, are __logf(2^-23) normalised); the failure messages print the new
# values; put them here if the host test still finds them within LOG_TOL of the exact floors.
DEVICE_FLOOR = {"mel": F32(-11.512927055358887), "fbank": F32(-1.2775938510894775)}


def floor_value(sp):
    """the output of an entry at the floor, as the fp32 the kernel stores"""
    if sp.kind in DEVICE_FLOOR:
        return DEVICE_FLOOR[sp.kind]
    return F32(-100.0) if sp.kind == "clap" else F32(0.0)


def exact_floor(sp):
    """the same in real arithmetic"""
    if sp.kind == "mel":
        return math.log(sp.floor)
    if sp.kind == "fbank":
        return (math.log(sp.floor) - sp.norm_mean) * sp.inv_2std
    return float(floor_value(sp))


def classify(sp, e, de):
    """(floor, live): FLOOR entries have e <= floor / 8 in fp64 (the host test holds restate32's leaked energy to the same; chroma: a frame
    whose every energy is exactly 0; fbank: e + de <= floor / 8, the derived bound alone), LIVE ones e >= 8 floor"""
    if sp.kind == "chroma":
        z = np.broadcast_to((e.max(axis=1, keepdims=True) == 0.0), e.shape)
        return z, ~z
    if sp.kind == "fbank":  # a 400-sample frame in a 512-point transform: nothing is bin-centred, the fp32 leakage of a tone reaches eps
        return e + de <= sp.floor / FLOOR_ROOM, e >= FLOOR_ROOM * sp.floor
    return e <= sp.floor / FLOOR_ROOM, e >= FLOOR_ROOM * sp.floor


def output_bound(sp, e, de, out):
    """the bound on the output entries that are not FLOOR, in the output's units"""
    if sp.kind == "chroma":  # e_c / max e: both relative errors, the division and (for safety) one more rounding
        rel = de / np.maximum(e, 1e-300)
        top = e >= 0.5 * e.max(axis=1, keepdims=True)
        rel_m = np.where(top, rel, 0.0).max(axis=1, keepdims=True)
        return np.abs(out) * (rel + rel_m + 2.0 * U)
    span = np.log(np.maximum(e + de, sp.floor)) - np.log(np.maximum(e - de, sp.floor))
    if sp.kind == "mel":
        return span + LOG_TOL["mel"]
    if sp.kind == "clap":  # 10 * log10f(e): the product's rounding on top
        return 10.0 / math.log(10.0) * span + U * np.abs(out) + LOG_TOL["clap"]
    lg = np.abs(np.log(np.maximum(e, sp.floor)))  # fbank: (__logf(e) - mean) * inv_2std, two more roundings
    return sp.inv_2std * span + 3.0 * U * (lg + abs(sp.norm_mean)) * sp.inv_2std + LOG_TOL["fbank"]


# ---- the framing of each kernel: this file's own index maps (-1 = a zero) ----
def mel_index(n, segment, target, mut=None):
    """apad_stft_logmel: [live frames, 1024] indices into the clip, and which of them came through a reflection"""
    nv = max(n, segment)
    live = min(target, nv // 160 + 1)
    i = 160 * np.arange(live)[:, None] - 512 + np.arange(1024)[None, :]
    left = i < 0
    i = np.where(left, -i - (1 if mut == "reflect_repeats_edge" else 0), i)
    right = i >= nv
    i = np.where(right, 2 * (nv - 1) - i + (1 if mut == "reflect_repeats_edge" else 0), i)
    cut = i >= n
    return np.where(cut, -1, i), left, right, cut & (left | right)


def clap_index(n, max_length, hop, padding, start=0, mut=None):
    """apad_clap_logmel at the target rate: crop / repeatpad / repeat / pad, then the reflect pad"""
    i = hop * np.arange(max_length // hop + 1)[:, None] - 512 + np.arange(1024)[None, :]
    rep = 1 if mut == "reflect_repeats_edge" else 0
    i = np.where(i < 0, -i - rep, i)
    i = np.where(i >= max_length, 2 * (max_length - 1) - i + rep, i)
    if n > max_length:
        return start + i
    limit = {"repeatpad": (max_length // n) * n, "repeat": max_length, "pad": n}[padding]
    q = (i + i // n) % n if mut == "seam_one_off" else i % n  # the mutant starts each further copy one sample late
    return np.where(i < limit, q, -1)


def chroma_index(n):
    i = 512 * np.arange(n // 512 + 1)[:, None] - 1024 + np.arange(2048)[None, :]
    return np.where((i >= 0) & (i < n), i, -1)


def gather(x, idx):
    return np.where(idx >= 0, np.asarray(x)[np.maximum(idx, 0)], 0).astype(np.asarray(x).dtype)


def fbank_frames(x, dtype):
    """kaldi.fbank's framing at 16 kHz: snip_edges frames of 400, per-frame DC removal, replicate-padded pre-emphasis, zero-padded to 512
    (before the window); -> (frames [F, 512], (1-norm, 2-norm) per frame [F] of the |error| the fp32 preparation adds to each windowed sample)"""
    n = x.shape[0]
    m = 0 if n < 400 else 1 + (n - 400) // 160
    fr = np.stack([x[160 * f:160 * f + 400] for f in range(m)]).astype(dtype) if m else np.zeros((0, 400), dtype)
    if dtype == F32:
        fr = fr - fr.mean(axis=1, keepdims=True, dtype=F32)
    else:
        fr = fr - fr.mean(axis=1, keepdims=True)
    prev = np.concatenate([fr[:, :1], fr[:, :-1]], axis=1)
    pre = fr - dtype(F32(0.97)) * prev
    # x - dc (u |x|), the frame mean (a sum of depth 10 and a division: 11 u mean|x|), cur and prev (u each), the product by 0.97 (u), the
    # difference (u): every term is at most u times a quantity below |cur| + 2 |prev| + |pre| + 12 mean|raw|
    raw = np.abs(fr) + np.abs(fr - pre)  # (loose on purpose: |cur| + 0.97 |prev|)
    dy = U * (2.0 * np.abs(fr) + 3.0 * np.abs(prev) + np.abs(pre) + 12.0 * raw.mean(axis=1, keepdims=True) + 12.0 * 0.5 / 400)
    win = 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(400) / 399)
    dyw = dy * win[None, :]
    return np.concatenate([pre, np.zeros((m, 112), dtype)], axis=1), (dyw.sum(axis=1), np.sqrt((dyw * dyw).sum(axis=1)))


# ---- one evaluated case ----
def evaluate(sp, frames64, frames32, rows, dy=None, clean=None):
    """-> namespace: expect / bound / exact [rows, R] (rows past the live frames are the kernel's padding rows, exact), the energies, the
    restatement.  ``clean``: the live frames the case is built for (default all)."""
    A, S, S2 = spectrum64(sp, frames64)
    e = energies64(sp, A)
    de = energy_bound(sp, A, S, e, dy, S2)
    out = post64(sp, e)
    floor, live = classify(sp, e, de)
    bound = np.where(floor, 0.0, output_bound(sp, e, de, out))
    out = np.where(floor, np.float64(floor_value(sp)), out)
    Fl, R = e.shape
    pad_value = 0.0
    if sp.kind == "fbank":
        pad_value = np.float64((F32(0.0) - F32(sp.norm_mean)) * F32(sp.inv_2std))
    b = types.SimpleNamespace(sp=sp, live_frames=Fl, e=e, de=de, A=A, S=S, floor=floor, live=live)
    b.expect = np.full((rows, R), pad_value)
    b.bound = np.zeros((rows, R))
    b.exact = np.ones((rows, R), bool)
    b.expect[:Fl], b.bound[:Fl], b.exact[:Fl] = out, bound, floor
    b.clean = np.ones(Fl, bool) if clean is None else clean
    b.e32 = restate32(sp, frames32) if frames32 is not None else None
    return b


def expect_only(sp, frames64, rows, fb=None, tw=None):
    """a mutant's expectation: the same chain with a changed filter table / twiddle table / framing"""
    A = spectrum64(sp, frames64, tw)[0]
    out = post64(sp, energies64(sp, A, fb))
    full = np.zeros((rows, out.shape[1]))
    full[:out.shape[0]] = out
    return full


def mutation_ratio(b, mutated):
    """the largest |mutated - expected| over an entry's own bound; an exact entry (bound 0) counts as moved, infinitely, when it moves by more
    than 1e-4 of the output's unit (the fp64 mutant does not carry the floor's fp32 rounding)"""
    d = np.abs(mutated - b.expect)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(b.exact, np.where(d > 1e-4, np.inf, 0.0), d / b.bound)
    return float(r.max()) if r.size else 0.0


def drop_bin(sp, row, which):
    fb = sp.fb64.copy()
    nz = np.nonzero(fb[row])[0]
    fb[row, nz[0] if which == "first" else nz[-1]] = 0.0
    return fb


def neighbour_twiddle(sp, t):
    tw = sp.tw64.copy()
    tw[t] = tw[t + 1 if t + 1 < tw.shape[0] else t - 1]
    return tw


def mirror_twiddle(sp, k):
    """The twiddle a tone at bin k is sensitive to.  X[t] = E[t] + w_t O[t] (the last stage; E, O the transforms of the even and odd samples).
    At t = k the two terms are in phase, so a wrong w_k moves |X_k| only in second order (5e-6); at the mirror bin t = N/2 - k they cancel, and a
    wrong w_t leaves |O_t| |dw| = 0.6 % of the peak in a bin that should be empty: a floored filter comes alive."""
    t = (sp.N // 2 - k) % (sp.N // 2)
    # (a tone near N/4 is its own mirror: the leak would fall under the filter that is live anyway.  Twiddle N/8 serves stages 3 to L and
    # leaks a quarter of the signal into bins far from k.)
    return t if abs(t - k) >= sp.N // 16 else sp.N // 8


def single_mark_frames(x, idx):
    """the live frames that read exactly one non-zero sample"""
    return (gather(x, idx) != 0).sum(axis=1) == 1


Case = types.SimpleNamespace


# ---- 1. the resampler ----
RATES = ((44100, 16000), (48000, 16000), (22050, 16000), (8000, 16000), (16000, 48000), (44100, 48000))


def resample_table(orig_freq, new_freq):
    from ap_adapter_amd import frontend as FE
    return FE._resample_kernel(orig_freq, new_freq)


def resample_expect(x, kern, width, orig, new):
    """-> (out fp32 [ceil(new n / orig)], the number of non-zero input samples each output's taps reach)"""
    n = x.shape[0]
    n_out = int(math.ceil(new * n / orig))
    i = np.arange(n_out)
    base = (i // new) * orig - width
    out, hits = np.zeros(n_out, F32), np.zeros(n_out, np.int64)
    for s in np.nonzero(x)[0]:
        j = s - base
        ok = (j >= 0) & (j < kern.shape[1])
        out[ok] += x[s] * kern[(i % new)[ok], j[ok]]
        hits += ok
    return out, hits


def resample_cases():
    cases = []
    for of, nf in RATES:
        _, width, orig, new = resample_table(of, nf)
        for n in sorted({1, orig - 1, orig, orig + 1, 2 * orig + 3} - {0}):
            for s in sorted({0, 1, n // 2, n - 1} & set(range(n))):
                cases.append(Case(name=f"rs_{of}_{nf}_n{n}_s{s}", rates=(of, nf), n=n, marks=[(s, 0.5)]))
        kw = 2 * width + orig
        for s in (0, orig + 1):  # two impulses farther apart than the taps reach
            cases.append(Case(name=f"rs_{of}_{nf}_pair_s{s}", rates=(of, nf), n=s + kw + 5 + orig, marks=[(s, 0.5), (s + kw + 2, -0.25)]))
    return cases


# ---- 2. apad_wav_stats ----
STATS_N = (101, 1023, 1024, 1025, 4097)


def dyadic_clip(n, seed):
    g = np.random.RandomState(seed)
    return (g.randint(-1024, 1025, size=n).astype(np.float64) / 1024.0).astype(F32)


def stats_expect(x):
    """(mean, scale) as apad_wav_stats defines them, the sum in fp64 (exact for dyadic samples), the rest in fp32"""
    x = np.asarray(x, F32)
    mean = F32(np.float64(x.astype(np.float64).sum()) / x.shape[0])
    peak = max(F32(x.max() - mean), F32(mean - x.min()))
    return mean, (F32(0.5) / F32(peak) if peak > 0 else F32(0.0))


# ---- 3. apad_stft_logmel ----
MEL_PAD_N = (101, 512, 513, 799, 800, 801, 960, 1600)
MEL_TONE_ROW = 20


def mel_tone_bins():
    sp = spec("mel")
    lo, hi = sp.ranges[MEL_TONE_ROW]
    return (1, 2, 3, int(lo), int(np.argmax(sp.fb32[MEL_TONE_ROW])), int(hi - 1), 510, 511)


def mel_sweep_bins():
    """one tone at every filter's peak bin: every row is live in its own tone and floored in others'"""
    sp = spec("mel")
    return sorted({int(np.argmax(sp.fb32[r])) for r in range(64)})


def mel_cases():
    cases = []
    for n, s in ((3200, 600), (3200, 680), (3300, 1000)):  # interior frames see a single impulse
        cases.append(Case(name=f"mel_pair_n{n}_s{s}", family="pair", n=n, segment=3200, target=20, marks=[(s, 0.5), (s + 1200, -0.5)]))
    for n in MEL_PAD_N:  # + at s, - at n - 1 - s: both reflect pads hold a marked sample
        for s in (0, 1, 511, 512):
            if s < n - 1 - s:
                cases.append(Case(name=f"mel_pad_n{n}_s{s}", family="pad", n=n, segment=800, target=8, marks=[(s, 0.5), (n - 1 - s, -0.5)]))
    for k in mel_tone_bins():
        cases.append(Case(name=f"mel_tone_k{k}", family="tone", n=4096, segment=3200, target=20, k=k))
    return cases


def mel_sweep_cases():
    return [Case(name=f"mel_sweep_k{k}", family="tone", n=4096, segment=3200, target=20, k=k) for k in mel_sweep_bins()]


def mel_signal(c):
    return tone(c.k, c.n, 0.5, 1024) if c.family == "tone" else impulses(c.n, c.marks)


@functools.lru_cache(None)
def _mel_build(name):
    c = MEL_BY_NAME[name]
    sp = spec("mel")
    x = mel_signal(c)
    idx, left, right, cut = mel_index(c.n, c.segment, c.target)
    clean = None
    if c.family == "tone":  # interior: no reflection and no zero padding inside the frame
        clean = ~(left.any(axis=1) | right.any(axis=1) | (idx < 0).any(axis=1))
    else:
        clean = single_mark_frames(x, idx)
    b = evaluate(sp, gather(x.astype(np.float64), idx), gather(x, idx), c.target, clean=clean)
    b.x, b.case = x, c
    marked = gather(x, idx) != 0
    b.branches = dict(left=bool((marked & left).any(axis=1).any() and ((marked & left).any(axis=1) & ~(marked & right).any(axis=1)).any()),
                      right=bool(((marked & right).any(axis=1) & ~(marked & left).any(axis=1)).any()),
                      both=bool(((marked & right).any(axis=1) & (marked & left).any(axis=1)).any()), cut=bool(cut.any()))
    return b


def mel_build(c):
    return _mel_build(c.name)


def mel_mutants(c):
    """[(name, mutated expectation [target, 64])]"""
    sp = spec("mel")
    out = []

    def run(x, mut=None, fb=None, tw=None):
        idx = mel_index(c.n, c.segment, c.target, mut)[0]
        return expect_only(sp, gather(x.astype(np.float64), idx), c.target, fb, tw)

    if c.family == "tone":
        x = mel_signal(c)
        rows = [r for r in range(64) if sp.ranges[r, 0] <= c.k + 1 and sp.ranges[r, 1] > c.k - 1]
        for r in rows:
            lo, hi = sp.ranges[r]
            if lo == c.k:
                out.append((f"row{r}_first_bin_dropped", run(x, fb=drop_bin(sp, r, "first"))))
            if hi - 1 == c.k:
                out.append((f"row{r}_last_bin_dropped", run(x, fb=drop_bin(sp, r, "last"))))
        out.append(("neighbour_twiddle", run(x, tw=neighbour_twiddle(sp, mirror_twiddle(sp, c.k)))))
    else:
        for d in (-1, 1):
            out.append((f"impulse_{d:+d}", run(impulses(c.n, shifted(c.marks, d, c.n)))))
        if c.family == "pad" and c.marks[0][0] <= 1:  # (a mark at 511 / 512 is read at window weight 1e-5 on the left: its partner carries the right pad)
            out.append(("reflect_repeats_edge", run(mel_signal(c), mut="reflect_repeats_edge")))
    return out


# ---- 4. apad_kaldi_fbank ----
FBANK_N = (399, 400, 401, 559, 560, 561, 400 + 160 * 7, 401 + 160 * 7, 400 + 160 * 8)
FBANK_P = (0, 1, 80, 199, 320, 398, 399)  # the issue's five, and two on the window's slopes where a read one sample off shows
FBANK_TARGET = 8
FBANK_TONE_BINS = tuple(range(2, 256, 3))  # 512-point bins: every HTK filter holds one of them or a neighbour


def fbank_cases():
    cases = []
    for n in FBANK_N:
        frames = 0 if n < 400 else min(FBANK_TARGET, 1 + (n - 400) // 160)
        for p in FBANK_P:
            s = min(160 * max(frames - 1, 0) + p, n - 1)  # window position p of the last frame kept
            cases.append(Case(name=f"fbank_n{n}_p{p}", family="impulse", n=n, p=p, marks=[(s, 0.5)]))
    for n in (560, 1520):
        cases.append(Case(name=f"fbank_tone_n{n}", family="tone", n=n, k=40))
    return cases


def fbank_sweep_cases():
    return [Case(name=f"fbank_sweep_k{k}", family="tone", n=560, k=k) for k in FBANK_TONE_BINS]


def fbank_edge_only(c):
    """window positions 0, 1, 398, 399 of kaldi's non-periodic Hann weigh 0 and 6e-5: the impulse is read (a NaN beside it would show) but what
    a shifted read changes drowns in the frame's DC term; position 199 of a clip with a single frame is the window's flat top (with a second
    frame the same sample is read at 359 as well); a clip with no frame has no entry to move.  Positions 80 and 320 hold every length to a
    shifted read."""
    return c.family == "impulse" and (c.n < 400 or c.p in (0, 1, 398, 399) or (c.p == 199 and c.n < 560))


def fbank_signal(c):
    return tone(c.k, c.n, 0.5, 512) if c.family == "tone" else impulses(c.n, c.marks)


def fbank_eval(x, fb=None, tw=None, full=True):
    sp = spec("fbank")
    x = np.asarray(x, F32)
    n = x.shape[0]
    fr64, dy = fbank_frames(x.astype(np.float64), np.float64)
    keep = min(FBANK_TARGET, fr64.shape[0])
    if not full:
        return expect_only(sp, fr64[:keep], FBANK_TARGET, fb, tw) if keep else np.zeros((FBANK_TARGET, 128))
    if keep == 0:
        b = evaluate(sp, np.zeros((0, 512)), None, FBANK_TARGET)
        b.e32 = np.zeros((0, 128), F32)
    else:
        b = evaluate(sp, fr64[:keep], fbank_frames(x - x.mean(dtype=F32), F32)[0][:keep], FBANK_TARGET, dy=(dy[0][:keep], dy[1][:keep]))
    return b


@functools.lru_cache(None)
def _fbank_build(name):
    c = FBANK_BY_NAME[name]
    x = fbank_signal(c)
    b = fbank_eval(x)
    b.x, b.case = x, c
    return b


def fbank_build(c):
    return _fbank_build(c.name)


def fbank_mutants(c):
    sp = spec("fbank")
    pad = np.float64((F32(0.0) - F32(sp.norm_mean)) * F32(sp.inv_2std))

    def run(x, fb=None, tw=None):
        out = fbank_eval(x, fb, tw, full=False)
        frames = 0 if c.n < 400 else min(FBANK_TARGET, 1 + (c.n - 400) // 160)
        out[frames:] = pad
        return out

    if c.family == "tone":
        x = fbank_signal(c)
        r = int(np.argmax(sp.fb32[:, c.k]))
        return [(f"row{r}_first_bin_dropped", run(x, fb=drop_bin(sp, r, "first"))), (f"row{r}_last_bin_dropped", run(x, fb=drop_bin(sp, r, "last"))),
                ("neighbour_twiddle", run(x, tw=neighbour_twiddle(sp, mirror_twiddle(sp, c.k))))]
    return [(f"impulse_{d:+d}", run(impulses(c.n, shifted(c.marks, d, c.n)))) for d in (-1, 1)]


# ---- 5. apad_clap_logmel ----
CLAP_MAX, CLAP_HOP, CLAP_AMP = 4800, 480, 2.0 ** -6  # (the tones' amplitude: the power floor is 1e-10; impulses are +0.5 / -0.25)
CLAP_N = (1, 2, 479, 480, 513, 2399, 2400, 2401, 4799, 4800, 4801, 6000)
CLAP_CONFIGS = ((64, 14000), (16, 26000))  # (feature_size, frequency_max); the second weighs bin 512
CLAP_TONE_FORMS = ((1024, "repeat"), (2048, "repeatpad"), (4800, "pad"), (6000, "pad"))


def clap_tone_bins(config):
    """[(k, row, which)]: a filter's first bin, peak and last bin -- of the filter whose peak is nearest bin 250, so that the tone's mirror
    bin 512 - k lies under a filter too (see mirror_twiddle) -- and, where the bank weighs it, bins 511 and 512"""
    sp = spec("clap", *config)
    peaks = np.array([int(np.argmax(sp.fb32[r])) for r in range(sp.fb32.shape[0])])
    r = int(np.argmin(np.abs(peaks - 250)))
    lo, hi = sp.ranges[r]
    bins = [(int(lo), r, "first"), (int(peaks[r]), r, "peak"), (int(hi - 1), r, "last")]
    if sp.fb32[:, 512].any():
        last = sp.fb32.shape[0] - 1
        bins += [(511, last, None), (512, last, None)]
    return bins


def clap_cases():
    cases = []
    for padding in ("repeatpad", "repeat", "pad"):
        for n in CLAP_N:
            marks = [(0, 0.5)] + ([(n - 1, -0.25)] if n > 1 else [])
            for start in ((0, n - CLAP_MAX) if n > CLAP_MAX else (0,)):
                cases.append(Case(name=f"clap_{padding}_n{n}_c{start}", family="impulse", padding=padding, n=n, start=start, marks=marks,
                                  configs=CLAP_CONFIGS))
    for config in CLAP_CONFIGS:
        for j, (k, row, which) in enumerate(clap_tone_bins(config)):
            n, padding = CLAP_TONE_FORMS[j % len(CLAP_TONE_FORMS)]
            for start in ((0, n - CLAP_MAX) if n > CLAP_MAX else (0,)):
                cases.append(Case(name=f"clap_tone{config[0]}_{padding}_n{n}_k{k}_c{start}", family="tone", padding=padding, n=n, start=start,
                                  k=k, row=row, which=which, configs=(config,)))
    return cases


def clap_signal(c):
    return tone(c.k, c.n, CLAP_AMP, 1024) if c.family == "tone" else impulses(c.n, c.marks)


@functools.lru_cache(None)
def _clap_build(name, config):
    c = CLAP_BY_NAME[name]
    sp = spec("clap", *config)
    x = clap_signal(c)
    idx = clap_index(c.n, CLAP_MAX, CLAP_HOP, c.padding, c.start)
    first = CLAP_HOP * np.arange(CLAP_MAX // CLAP_HOP + 1) - 512
    if c.family == "tone":  # frames the reflection and the zero padding leave alone (a tone's repeat seam is no seam: whole periods)
        clean = (first >= 0) & (first + 1024 <= CLAP_MAX) & (idx >= 0).all(axis=1)
    else:
        clean = single_mark_frames(x, idx)
    b = evaluate(sp, gather(x.astype(np.float64), idx), gather(x, idx), CLAP_MAX // CLAP_HOP + 1, clean=clean)
    b.x, b.case = x, c
    # the seam between two copies (or between the clip and its zero padding): samples n - 1 and n of the framed signal inside one frame
    b.seam_in_frame = bool(c.n < CLAP_MAX and ((c.n - 1 >= np.maximum(first, 0)) & (c.n <= np.minimum(first + 1023, CLAP_MAX - 1))).any())
    return b


def clap_build(c, config):
    return _clap_build(c.name, config)


def clap_mutants(c, config):
    sp = spec("clap", *config)
    rows = CLAP_MAX // CLAP_HOP + 1

    def run(x, mut=None, fb=None, tw=None):
        return expect_only(sp, gather(x.astype(np.float64), clap_index(c.n, CLAP_MAX, CLAP_HOP, c.padding, c.start, mut)), rows, fb, tw)

    out = []
    if c.family == "tone":
        x = clap_signal(c)
        if c.which in ("first", "last"):
            out.append((f"row{c.row}_{c.which}_bin_dropped", run(x, fb=drop_bin(sp, c.row, c.which))))
        if c.k < 512:
            out.append(("neighbour_twiddle", run(x, tw=neighbour_twiddle(sp, mirror_twiddle(sp, c.k)))))
        if c.k >= 511:
            fb = sp.fb64.copy()
            fb[:, 512] = 0.0
            out.append(("nyquist_bin_dropped", run(x, fb=fb)))
        return out
    for d in (-1, 1):
        moved = shifted(c.marks, d, c.n)
        if c.n > 2 and moved != c.marks:
            out.append((f"impulse_{d:+d}", run(impulses(c.n, moved))))
    if 1 < c.n and 2 * c.n <= CLAP_MAX and c.padding != "pad":
        out.append(("seam_one_off", run(clap_signal(c), mut="seam_one_off")))
    if c.n > 1:
        out.append(("reflect_repeats_edge", run(clap_signal(c), mut="reflect_repeats_edge")))
    return out


# ---- 6. apad_chroma ----
CHROMA_N = (1, 511, 512, 2047, 2048, 5121)  # tests/test_gpu_chroma.py's SMALL_N
CHROMA_S = (0, 511, 512, 1023, 1024)


def chroma_cases():
    cases = []
    for n in CHROMA_N:
        for s in sorted({s for s in CHROMA_S + (n - 1,) if s < n}):
            cases.append(Case(name=f"chroma_n{n}_s{s}", family="impulse", n=n, marks=[(s, 0.5)]))
    for k in (1023, 1024):
        cases.append(Case(name=f"chroma_tone_k{k}", family="tone", n=4096, k=k))
    return cases


def chroma_frames_holding(s, n):
    """the frames that read sample s at a non-zero window weight (position 0 of the periodic Hann window weighs exactly 0)"""
    return {f for f in range(n // 512 + 1) if 512 * f - 1024 + 1 <= s <= 512 * f + 1023}


def chroma_edge_only(c):
    """an impulse's chroma row does not depend on where in the frame it is read (a flat power spectrum, divided by its own maximum): a shifted
    read shows only where it changes WHICH frames hold the impulse"""
    if c.family != "impulse":
        return False
    s = c.marks[0][0]
    return all(chroma_frames_holding(s + d, c.n) == chroma_frames_holding(s, c.n) for d in (-1, 1) if 0 <= s + d < c.n)


def clap_edge_only(c):
    """a one-sample clip: repeated it is a constant, padded it has nowhere to move"""
    return c.family == "impulse" and c.n == 1


def chroma_signal(c):
    return tone(c.k, c.n, 0.5, 2048) if c.family == "tone" else impulses(c.n, c.marks)


@functools.lru_cache(None)
def _chroma_build(name):
    c = CHROMA_BY_NAME[name]
    sp = spec("chroma")
    x = chroma_signal(c)
    idx = chroma_index(c.n)
    clean = (idx >= 0).all(axis=1) if c.family == "tone" else single_mark_frames(x, idx)
    b = evaluate(sp, gather(x.astype(np.float64), idx), gather(x, idx), c.n // 512 + 1, clean=clean)
    b.x, b.case = x, c
    return b


def chroma_build(c):
    return _chroma_build(c.name)


def chroma_mutants(c):
    sp = spec("chroma")
    run = lambda x, fb=None, tw=None: expect_only(sp, gather(x.astype(np.float64), chroma_index(c.n)), c.n // 512 + 1, fb, tw)
    if c.family == "tone":
        fb = sp.fb64.copy()
        fb[:, 1024] = 0.0
        # (twiddle 0 serves every stage; the mirror bins 0 and 1 weigh 3e-3 in the chroma bank and the power is second order in a leak)
        x = chroma_signal(c)
        return [("nyquist_bin_dropped", run(x, fb=fb)), ("neighbour_twiddle", run(x, tw=neighbour_twiddle(sp, 0)))]
    # a flat spectrum gives the same row at every position: what a shifted read changes is WHICH frames hold the impulse, so the mutant
    # moves it across the nearest frame edge (512 f - 1024 or 512 f + 1023)
    s = c.marks[0][0]
    out = []
    for d in (-1, 1):
        if 0 <= s + d < c.n:
            out.append((f"impulse_{d:+d}", run(impulses(c.n, [(s + d, 0.5)]))))
    return out


MEL_CASES, FBANK_CASES, CLAP_CASES, CHROMA_CASES, RESAMPLE_CASES = mel_cases(), fbank_cases(), clap_cases(), chroma_cases(), resample_cases()
MEL_SWEEP, FBANK_SWEEP = mel_sweep_cases(), fbank_sweep_cases()
MEL_BY_NAME = {c.name: c for c in MEL_CASES + MEL_SWEEP}
FBANK_BY_NAME = {c.name: c for c in FBANK_CASES + FBANK_SWEEP}
CLAP_BY_NAME = {c.name: c for c in CLAP_CASES}
CHROMA_BY_NAME = {c.name: c for c in CHROMA_CASES}
RESAMPLE_BY_NAME = {c.name: c for c in RESAMPLE_CASES}
