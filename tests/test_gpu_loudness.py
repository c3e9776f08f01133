"""-m gpu: BS.1770 loudness (apad_loudness) and the gain towards a target (apad_loudness_gain) against the independent fp64 restatement
in tests/loudness_oracle.py (scipy's sosfilt, numpy blocks and gates), and ``target_loudness=`` through the pipeline.

Yardstick: the SAME oracle run in fp32 on the CPU (fp32 coefficients, state and sums: the plain serial recursion) against its fp64 self
on the same fp32 samples, measured inside each test.  Bounds:

  hop energies   |error| / the clip's largest hop energy <= max(8 x yardstick, 1e-6)
  loudness       |dL| <= max(8 x yardstick, 2e-5 LU), and below 0.1 LU (the EBU Tech 3341 meter tolerance: a condition, not the expectation)

The factor 8 = 2 x 4.  2, from the operation count: the serial fp32 recursion's state carries the roundings of about 1 / (1 - 0.985) = 66
samples (the 38 Hz pole pair's memory at 16 kHz).  A state in the kernel carries, in place of those, its lane's forced response (8
steps), six scan levels, at most 15 wave carries, one tile carry and one entry product -- 31 more roundings of the same size, each sample
is filtered twice (from a zero state, then from the true one), and the shelf and the high-pass's all-pole half are scanned one after the
other: (66 + 31 + 8) / 66 = 1.6 in the worst case where everything adds up, below 2.  4, because both figures are the MAXIMUM of a rounding
walk over up to 102 hops, of which the yardstick is one draw: a second draw from the same distribution exceeds the first by more than 4 x
with negligible probability.  The floors cover clips where the yardstick is a handful of ulps (log10f and the last rounding of a value
near -23: 2e-6 LU each).  Measured on the MI355X (each figure is printed before it is asserted): hop energies 8.3e-6 .. 1.05e-5 on the
three-level clips of 6399 .. 163840 samples against yardsticks of 7.5e-6 .. 8.5e-6 (1.0 .. 1.25 x), 4.2e-5 against 5.6e-5 on the 50 Hz sine,
2.0e-7 against 2.5e-5 on the step, 4.7e-5 against 4.3e-5 at 44.1 kHz; loudness 3.0e-5 .. 3.8e-5 LU against 3.0e-5 .. 3.3e-5, 1.8e-4 against
2.0e-4 on the sine.  (With the all-pole state scanned as (y[n-1], y[n-2]) instead of value and difference the same clips read 4e-5 .. 1.5e-4:
that version failed these bounds, which is how the coordinates were found.)

Gain bound, from the kernel's operations (u = 2^-24; the reference is the fp64 formula on the kernel's own fp32 L, target and peak):
d = target - L (u), e = d * 0.05f (u, and 0.05f's own 0.6 u), so the exponent is off by at most 3 u |e| and 10^e by ln(10) 3 u |e|;
exp10f itself within 3 ulp = 6 u: |g - ref| / ref <= (6 + 6.91 |e|) u.  Where the guard binds g = peak_limit / peak, one correctly
rounded division: bit-equal to the same division in numpy.
"""
import functools
import math

import numpy as np
import pytest
import torch

import loudness_oracle as O
from util import nan_fill_free

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
LENGTHS = (6399, 6400, 6401, 7999, 8000, 20000, 51200)
CAP = 0.1


def nan(*shape, dev):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=dev)


@functools.lru_cache(maxsize=None)
def clip(name):
    """the tests' clips by name: an integer length (the issue's three-level signal), or a carry clip of 20000 samples"""
    if name == "sine50":
        return (0.5 * np.sin(2 * np.pi * 50 * np.arange(20000) / O.SR)).astype(np.float32)
    if name == "step":
        return np.full(20000, 0.5, np.float32)
    return O.signal(int(name))


@functools.lru_cache(maxsize=None)
def oracle(name, fs=O.SR):
    """(fp64 result, fp32 yardstick result) of a clip, computed once; the gate condition is asserted here, on the oracle, for every user"""
    r64, r32 = O.loudness(clip(name), fs), O.loudness(clip(name), fs, dtype=np.float32)
    margin = O.gate_margin(r64)
    assert min(margin) >= 1.0, (name, margin)  # no block within 1 LU of a gate: a flipped decision cannot hide in the tolerance
    assert (r32.n_abs, r32.n_rel) == (r64.n_abs, r64.n_rel)
    return r64, r32


def bounds(r64, r32):
    big = float(r64.hop_energy.max()) if len(r64.hop_energy) else 1.0
    yard_hop = float(np.abs(r32.hop_energy.astype(np.float64) - r64.hop_energy).max()) / big if len(r64.hop_energy) else 0.0
    yard_L = abs(r32.L - r64.L) if math.isfinite(r64.L) else 0.0
    return yard_hop, max(8.0 * yard_hop, 1e-6), yard_L, max(8.0 * yard_L, 2e-5)


def launch(clips, dev, fs=O.SR, target_hops=None, hop_energy=True):
    """ops.loudness on NaN-filled outputs: every element must be written"""
    from ap_adapter_amd import loudness, ops
    hop = O.hop_block(fs)[0]
    oh = torch.zeros(len(clips) + 1, dtype=torch.int64)
    oh[1:] = torch.cumsum(torch.tensor([len(c) for c in clips]), 0)
    packed = torch.from_numpy(np.concatenate(clips).astype(np.float32)).to(dev)
    T = max(1, max(len(c) for c in clips) // hop) if target_hops is None else target_hops
    stats, he = nan(len(clips), 4, dev=dev), (nan(len(clips), T, dev=dev) if hop_energy else None)
    ops.loudness(packed, oh.to(dev), oh, *loudness.tables(dev, fs), stats, hop, hop_energy=he)
    assert not torch.isnan(stats).any() and (he is None or not torch.isnan(he).any())
    return stats, he, (packed, oh)


def check_clip(name, stats, he, what, fs=O.SR):
    """one clip's kernel outputs (stats [4], hop energies [T], on the host) against the oracle, within the docstring's bounds"""
    r64, r32 = oracle(name, fs)
    yard_hop, bound_hop, yard_L, bound_L = bounds(r64, r32)
    nh = len(r64.hop_energy)
    big = float(r64.hop_energy.max()) if nh else 1.0
    err_hop = float(np.abs(he[:nh].double().numpy() - r64.hop_energy).max()) / big if nh else 0.0
    L = float(stats[0])
    err_L = abs(L - r64.L) if math.isfinite(r64.L) else (0.0 if L == r64.L else math.inf)
    print(f"{what}: L {L:.6f} (oracle {r64.L:.6f}), blocks {len(r64.block_loudness)} -> {r64.n_abs} -> {r64.n_rel}; hop energies: yardstick "
          f"{yard_hop:.3e}, bound {bound_hop:.3e}, kernel {err_hop:.3e}; loudness: yardstick {yard_L:.3e} LU, bound {bound_L:.3e}, kernel {err_L:.3e}")
    assert bool((he[nh:] == 0).all())  # only whole hops are written; zeros after them
    assert float(stats[1]) == float(np.abs(clip(name)).max())  # the sample peak, bit for bit
    assert (float(stats[2]), float(stats[3])) == (float(r64.n_abs), float(r64.n_rel))
    assert bound_L < CAP
    assert err_hop <= bound_hop and err_L <= bound_L
    return err_hop, err_L


@pytest.mark.parametrize("n", LENGTHS)
def test_parity(dev, n):
    assert O.block_count(n) == {6399: 0, 6400: 1, 6401: 1, 7999: 1, 8000: 2, 20000: 9, 51200: 29}[n]
    stats, he, _ = launch([clip(n)], dev)
    if n == 6399:
        assert float(stats[0, 0]) == -math.inf and float(stats[0, 2]) == 0 and float(stats[0, 3]) == 0
    if n == 51200:
        r64, _ = oracle(n)
        assert (len(r64.block_loudness), r64.n_abs, r64.n_rel) == (29, 24, 15)  # both gates keep some blocks and drop others
    check_clip(n, stats[0].cpu(), he[0].cpu(), f"n = {n}")


def test_parity_product_shape(dev):
    r64, _ = oracle(163840)
    assert (len(r64.block_loudness), r64.n_abs, r64.n_rel) == (99, 77, 46)
    stats, he, _ = launch([clip(163840)], dev)
    check_clip(163840, stats[0].cpu(), he[0].cpu(), "n = 163840")


@pytest.mark.parametrize("name", ["sine50", "step"])
def test_carry_clips(dev, name):
    """what a wrong lane, wave or tile carry shows in: a 50 Hz sine (inside the high-pass's transition band), and a constant, whose
    output after the first samples is all zero-input decay handed across three tile boundaries"""
    stats, he, _ = launch([clip(name)], dev)
    check_clip(name, stats[0].cpu(), he[0].cpu(), name)


def test_other_rates(dev):
    """48 kHz: one hop per tile, and the standard's calibration statement on the device (a 0 dBFS 997 Hz sine reads -3.01 LKFS).
    44.1 kHz: a tile of 4410 samples is no multiple of a lane's 8, so the tile's carry leaves from the middle of a lane's run."""
    from ap_adapter_amd import loudness
    t = np.arange(48000 * 2) / 48000.0
    sine = np.sin(2 * np.pi * 997 * t).astype(np.float32)
    L = float(loudness.integrated_loudness(torch.from_numpy(sine).to(dev), sampling_rate=48000)[0])
    ref = O.loudness(sine, 48000)
    yard = abs(O.loudness(sine, 48000, dtype=np.float32).L - ref.L)
    print(f"997 Hz, 0 dBFS, 48 kHz: {L:.5f} LKFS (oracle {ref.L:.5f}; yardstick {yard:.3e})")
    assert abs(L - (-3.01)) <= 0.01 and abs(L - ref.L) <= max(8 * yard, 2e-5)
    x = O.signal(4410 * 7 + 999, 44100)
    r64, r32 = O.loudness(x, 44100), O.loudness(x, 44100, dtype=np.float32)
    assert min(O.gate_margin(r64)) >= 1.0
    yard_hop, bound_hop, yard_L, bound_L = bounds(r64, r32)
    stats, he, _ = launch([x], dev, fs=44100)
    err_hop = float(np.abs(he[0].cpu().double().numpy() - r64.hop_energy).max()) / float(r64.hop_energy.max())
    err_L = abs(float(stats[0, 0]) - r64.L)
    print(f"44.1 kHz, {len(x)} samples: hop energies yardstick {yard_hop:.3e}, bound {bound_hop:.3e}, kernel {err_hop:.3e}; loudness yardstick "
          f"{yard_L:.3e}, bound {bound_L:.3e}, kernel {err_L:.3e}")
    assert he.shape[1] == 7 and err_hop <= bound_hop and err_L <= bound_L
    assert (float(stats[0, 2]), float(stats[0, 3])) == (float(r64.n_abs), float(r64.n_rel))


def test_silence(dev):
    stats, he, _ = launch([np.zeros(20000, np.float32), clip(6399)], dev, target_hops=14)
    s = stats.cpu()
    assert float(s[0, 0]) == -math.inf and s[0, 1:].tolist() == [0.0, 0.0, 0.0] and bool((he[0] == 0).all())
    assert float(s[1, 0]) == -math.inf and s[1, 2:].tolist() == [0.0, 0.0] and float(s[1, 1]) > 0
    assert bool((he[1, 3:] == 0).all()) and bool((he[1, :3] > 0).all())  # 6399 samples: three whole hops, no block


def test_batch_independence(dev):
    names = (51200, "step", 6399, 8000, "sine50", 20000, 6401)
    alone = [launch([clip(n)], dev, target_hops=32)[:2] for n in names]
    for order in (list(range(len(names))), [4, 0, 6, 2, 5, 1, 3]):
        stats, he, _ = launch([clip(names[i]) for i in order], dev, target_hops=32)
        for row, i in enumerate(order):
            assert torch.equal(stats[row], alone[i][0][0]) and torch.equal(he[row], alone[i][1][0]), (order, row)
    # without the hop energies the statistics are the same numbers
    assert torch.equal(launch([clip(n) for n in names], dev, hop_energy=False)[0], torch.cat([a[0] for a in alone]))


def run_gain(packed, oh, stats, dev, limit, target=None, ref_stats=None, ref_index=None, alias=False):
    from ap_adapter_amd import ops
    B = oh.numel() - 1
    x = packed.clone()
    out, gains = (x if alias else nan(packed.numel(), dev=dev)), nan(B, dev=dev)
    kw = {}
    if target is not None:
        kw["target"] = torch.tensor(target, dtype=torch.float32).to(dev)
    else:
        ih = torch.tensor(ref_index, dtype=torch.int32)
        kw.update(ref_stats=ref_stats, ref_index=ih.to(dev), ref_index_host=ih)
    ops.loudness_gain(x, oh.to(dev), oh, stats, out, gains, limit, **kw)
    assert not torch.isnan(gains).any() and not torch.isnan(out).any()
    return out, gains


def check_gains(gains, stats, targets, limit, what):
    """the fp64 rule on the kernel's own fp32 inputs, within the docstring's bound; returns which clips the guard bound"""
    bound_by_guard = []
    for b, t in enumerate(targets):
        L, peak = float(stats[b, 0]), float(stats[b, 1])
        t32 = float(np.float32(t))
        ref = O.gain(L, t32, peak, float(np.float32(limit)))
        g = float(gains[b])
        free = O.gain(L, t32, peak, 0.0)
        guarded = limit > 0 and ref != free
        bound_by_guard.append(guarded)
        if guarded:
            assert g == float(np.float32(limit) / np.float32(peak)), (what, b)
        elif ref == 1.0 and not (math.isfinite(L) and math.isfinite(t32) and peak > 0):
            assert g == 1.0, (what, b)
        else:
            e = abs(t32 - L) / 20.0
            bound = (6.0 + 6.91 * e) * U
            print(f"{what}: clip {b}: gain {g:.7g}, fp64 rule {ref:.7g}, relative error {abs(g - ref) / ref:.3e}, bound {bound:.3e}")
            assert abs(g - ref) / ref <= bound, (what, b)
    return bound_by_guard


def test_gain(dev):
    names = (51200, 20000, "sine50", 6399, 8000)
    clips = [clip(n) for n in names] + [np.zeros(7000, np.float32)]
    stats, _, (packed, oh) = launch(clips, dev, hop_energy=False)
    s = stats.cpu()
    limit = 10.0 ** (-1.0 / 20.0)
    # -14 LUFS lifts the first clip (-22.3 LUFS, peak 0.23) by 8.3 dB: under the limit; +3 LUFS would lift the second by 26 dB: the guard binds
    targets = [-14.0, 3.0, -30.0, -20.0, float("nan"), -20.0]
    out, gains = run_gain(packed, oh, stats, dev, limit, target=targets)
    guarded = check_gains(gains.cpu(), s, targets, limit, "targets")
    assert guarded[1] and not guarded[0] and not guarded[2]
    g, o, x = gains.cpu(), out.cpu(), packed.cpu()
    assert g[3] == 1.0 and g[4] == 1.0 and g[5] == 1.0  # no loudness (no block), a NaN target, a silent clip
    for b in range(len(clips)):
        lo, hi = int(oh[b]), int(oh[b + 1])
        assert torch.equal(o[lo:hi], g[b] * x[lo:hi]), b  # one fp32 multiply per sample: the host reproduces the bits
    lo, hi = int(oh[1]), int(oh[2])
    peak_out = float(o[lo:hi].abs().max())
    print(f"guarded clip: gain {float(g[1]):.6f}, peak {peak_out:.7f}, limit {limit:.7f}")
    assert peak_out <= float(np.float32(limit)) * (1 + 2.0 ** -23)
    # in place: the same bits
    out2, gains2 = run_gain(packed, oh, stats, dev, limit, target=targets, alias=True)
    assert torch.equal(out2, out) and torch.equal(gains2, gains)
    # a target of -inf, and no guard at all
    out3, gains3 = run_gain(packed, oh, stats, dev, 0.0, target=[-math.inf, 3.0, -30.0, -20.0, -20.0, -20.0])
    assert float(gains3[0]) == 1.0
    assert not any(check_gains(gains3.cpu(), s, [-math.inf, 3.0, -30.0, -20.0, -20.0, -20.0], 0.0, "no guard"))
    assert float(out3[int(oh[1]): int(oh[2])].abs().max()) > 1.0  # (what the guard is for)
    # source matching: two candidates mapped to different references each get their own reference's loudness as the target
    ref_stats, _, _ = launch([clip("sine50"), clip(51200), clip(6399)], dev, hop_energy=False)
    idx = [0, 1, 0, 1, 2, 0]
    out4, gains4 = run_gain(packed, oh, stats, dev, limit, ref_stats=ref_stats, ref_index=idx)
    r = ref_stats.cpu()
    check_gains(gains4.cpu(), s, [float(r[i, 0]) for i in idx], limit, "references")
    assert float(gains4[0]) > 2.0 and 1.0 < float(gains4[1]) < 1.5  # -22.3 -> -13.6 (the sine's), -23.2 -> -22.3 (the long clip's)
    assert float(gains4[2]) == 1.0  # matched to itself: 10^0, exactly
    assert float(gains4[3]) == 1.0 and float(gains4[4]) == 1.0  # no loudness of its own; a reference without one (-inf)


def test_refusals(dev):
    from ap_adapter_amd import loudness, ops
    tabs = loudness.tables(dev)
    x = torch.zeros(70000, device=dev)

    def run(offsets, T=None, hop=1600):
        oh = torch.tensor(offsets, dtype=torch.int64)
        return ops.loudness(x, oh.to(dev), oh, *tabs, nan(oh.numel() - 1, 4, dev=dev), hop,
                            hop_energy=None if T is None else nan(oh.numel() - 1, T, dev=dev))

    with pytest.raises(RuntimeError, match="clip 1 is empty"):
        run([0, 600, 600, 900])
    with pytest.raises(RuntimeError, match=r"offsets\[0\] must be 0"):
        run([4, 600])
    with pytest.raises(RuntimeError, match="clip 1 has 3 whole hops, target_hops is 2"):
        run([0, 600, 5500], 2)
    with pytest.raises(RuntimeError, match="a hop of 8193 samples"):
        run([0, 600], hop=8193)
    with pytest.raises(RuntimeError, match="clip 0 has 7000 hops"):
        run([0, 70000], hop=10)
    with pytest.raises(RuntimeError, match="batch 65536 exceeds 65535"):
        run(list(range(65537)))
    s = run([0, 600, 5500], 3).cpu()
    assert bool((s[:, 0] == -math.inf).all()) and bool((s[:, 1:] == 0).all())  # the same operands, valid: silence
    oh = torch.tensor([0, 600, 5500], dtype=torch.int64)
    st, g, ih = torch.zeros(2, 4, device=dev), nan(2, dev=dev), torch.tensor([0, 2], dtype=torch.int32)
    with pytest.raises(RuntimeError, match=r"ref_index\[1\] = 2 outside \[0, 2\)"):
        ops.loudness_gain(x, oh.to(dev), oh, st, x.clone(), g, 0.5, ref_stats=st, ref_index=ih.to(dev), ref_index_host=ih)
    with pytest.raises(RuntimeError, match="either target, or ref_stats"):
        ops.loudness_gain(x, oh.to(dev), oh, st, x.clone(), g, 0.5)
    with pytest.raises(RuntimeError, match="either target, or ref_stats"):
        ops.loudness_gain(x, oh.to(dev), oh, st, x.clone(), g, 0.5, target=g, ref_stats=st, ref_index=ih.to(dev), ref_index_host=ih)


def test_graph_capture(dev):
    """both launches recorded in one hipGraph on one stream and replayed twice on new contents of the same buffers equal eager, bit for bit"""
    from ap_adapter_amd import loudness, ops
    tabs = loudness.tables(dev)
    names = (20000, 8000, 6399)
    oh = torch.zeros(4, dtype=torch.int64)
    oh[1:] = torch.cumsum(torch.tensor([len(clip(n)) for n in names]), 0)
    od = oh.to(dev)
    first = torch.from_numpy(np.concatenate([clip(n) for n in names])).to(dev)
    second = (first * 0.37).contiguous()
    x = first.clone()
    target = torch.tensor([-23.0, 0.0, -23.0], device=dev)
    stats, he, out, gains = nan(3, 4, dev=dev), nan(3, 12, dev=dev), nan(x.numel(), dev=dev), nan(3, dev=dev)
    bufs = (stats, he, out, gains)

    def both():
        ops.loudness(x, od, oh, *tabs, stats, 1600, hop_energy=he)
        ops.loudness_gain(x, od, oh, stats, out, gains, 0.5, target=target)

    both()  # (loads the library and the tables outside the capture)
    stats_first = stats.clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        both()
    x.copy_(second)
    got = []
    for _ in range(2):
        for t in bufs:
            t.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        got.append([t.clone() for t in bufs])
    for t in bufs:
        t.fill_(float("nan"))
    both()
    torch.cuda.synchronize()
    for rep in got:
        for a, b in zip(rep, bufs):
            assert not torch.isnan(a).any() and torch.equal(a, b)
    assert not torch.equal(got[0][0], stats_first)  # the replay read the buffers' new contents


def test_public_surface(dev):
    """integrated_loudness / normalize_loudness: ragged lists, a rectangular GPU tensor, a single clip; targets and a reference"""
    import ap_adapter_amd as A
    names = (20000, 8000, 51200)
    clips = [clip(n) for n in names]
    nan_fill_free(dev)
    rag = A.integrated_loudness([torch.from_numpy(c) for c in clips], return_stats=True)
    assert rag.shape == (3, 4) and torch.equal(rag, launch(clips, dev, hop_energy=False)[0])
    rect = torch.from_numpy(np.stack([clips[0], 0.5 * clips[0]])).to(dev)  # (an exact scaling: the same gate margins, 6.02 LU lower)
    L = A.integrated_loudness(rect)
    assert L.shape == (2,) and torch.equal(L[0], rag[0, 0]) and torch.equal(A.integrated_loudness(rect[0])[0], L[0])
    nan_fill_free(dev)
    out, gains = A.normalize_loudness(clips, target=[-23.0, -16.0, -30.0], peak_limit_db=None)
    assert isinstance(out, list) and [o.numel() for o in out] == list(names) and gains.shape == (3,)
    for b, n in enumerate(names):
        r64, r32 = oracle(n)
        after = O.loudness(out[b].cpu().numpy())
        bound = bounds(r64, r32)[3] + 2e-5  # the measurement's bound, and the gain's (11 u of 8.7 dB: 6e-6 LU) with the multiply's rounding
        print(f"normalize_loudness: clip {n} to {(-23.0, -16.0, -30.0)[b]}: oracle reads {after.L:.6f} (bound {bound:.3e})")
        assert abs(after.L - (-23.0, -16.0, -30.0)[b]) <= bound
    out2, gains2 = A.normalize_loudness(rect, reference=torch.from_numpy(clips[2]))  # both clips to the third's loudness
    assert out2.shape == rect.shape and out2.is_cuda
    for b in range(2):
        assert abs(O.loudness(out2[b].cpu().numpy()).L - oracle(51200)[0].L) <= bounds(*oracle(20000))[3] + bounds(*oracle(51200))[3] + 2e-5
    out3, gains3 = A.normalize_loudness(rect[0], target=0.0)  # default guard -1 dBFS: binds
    assert out3.shape == (20000,) and float(out3.abs().max()) <= float(np.float32(10.0 ** (-1 / 20))) * (1 + 2.0 ** -23)


# ---- through the pipeline: the small synthetic UNet, VAE and vocoder of the chroma tests ----
@pytest.fixture(scope="module")
def small(dev):
    import test_gpu_chroma as C
    return C.build_small(dev)


def check_returned(out, targets, limit, pipe, what, extra=0.0):
    """each returned clip against its target: within the bound (+ ``extra``: the error of a measured target) where the guard did not bind,
    at most on the limit where it did"""
    stats, gains = pipe.last_loudness
    assert stats.is_cuda and tuple(stats.shape) == (out.shape[0], 4) and tuple(gains.shape) == (out.shape[0],)
    for b in range(out.shape[0]):
        x = out[b].numpy()
        r64, r32 = O.loudness(x), O.loudness(x, dtype=np.float32)
        assert min(O.gate_margin(r64)) >= 1.0, (what, b, O.gate_margin(r64))
        bound = max(8.0 * abs(r32.L - r64.L), 2e-5) + 2e-5  # the measurement's bound on a clip of this kind, and the gain's (as above)
        peak = float(np.abs(x).max())
        on_limit = limit > 0 and peak >= limit * (1 - 1e-6)
        print(f"{what}: clip {b}: oracle reads {r64.L:.6f} LUFS, target {targets[b]:.6f}, bound {bound:.3e}, peak {peak:.6f}"
              f"{' (guard bound)' if on_limit else ''}; last_loudness {float(stats[b, 0]):.6f}, gain {float(gains[b]):.6f}")
        assert bound < CAP
        if on_limit:
            assert peak <= float(np.float32(limit)) * (1 + 2.0 ** -23) and r64.L <= targets[b] + bound + extra
        else:
            assert abs(r64.L - targets[b]) <= bound + extra
        # last_loudness holds the statistics of what was returned
        assert abs(float(stats[b, 0]) - r64.L) <= bound and float(stats[b, 1]) == peak
        assert (float(stats[b, 2]), float(stats[b, 3])) == (float(r64.n_abs), float(r64.n_rel))


def test_pipeline_target_and_source(dev, small):
    import ap_adapter_amd as A
    import test_gpu_chroma as C
    pipe = A.AudioLDM2Pipeline(small.unet, vae=small.vae, vocoder=small.voc)
    kw = dict(source_latents=small.source, **small.kw)
    gen = lambda: torch.Generator().manual_seed(C.SEED)
    B = small.P * C.N
    plain = pipe(generator=gen(), **kw).audios
    assert pipe.last_loudness is None
    assert torch.equal(pipe(generator=gen(), target_loudness=None, **kw).audios, plain) and pipe.last_loudness is None
    limit = 10.0 ** (-1.0 / 20.0)
    nan_fill_free(dev)
    out = pipe(generator=gen(), target_loudness=-23.0, **kw).audios
    assert out.shape == plain.shape and not out.is_cuda
    check_returned(out, [-23.0] * B, limit, pipe, "target -23")
    g = pipe.last_loudness[1].cpu()
    for b in range(B):
        assert torch.equal(out[b], g[b] * plain[b])  # the candidates as generated, times one gain each
    # one target per returned clip
    per_clip = [-20.0 - b for b in range(B)]
    out = pipe(generator=gen(), target_loudness=per_clip, **kw).audios
    check_returned(out, per_clip, limit, pipe, "per-clip targets")
    # matched to the source as the same VAE and vocoder render it
    src = C.decoded_source(small)
    src_L = [O.loudness(s.numpy()).L for s in src]
    for s in src:
        assert min(O.gate_margin(O.loudness(s.numpy()))) >= 1.0
    nan_fill_free(dev)
    out = pipe(generator=gen(), target_loudness="source", **kw).audios
    # (the kernel's measurement of the reference carries its own error: the same bound, taken on the sources)
    extra = max(max(8.0 * abs(O.loudness(x.numpy(), dtype=np.float32).L - L), 2e-5) for x, L in zip(src, src_L))
    check_returned(out, [src_L[b // C.N] for b in range(B)], limit, pipe, "source", extra=extra)
    # (this vocoder ends in a tanh that saturates: the candidates peak at 1.0, so under the default guard every clip above ends ON the limit,
    # below its source.  Without the guard each edit reads its source's loudness.)
    out = pipe(generator=gen(), target_loudness="source", peak_limit_db=None, **kw).audios
    check_returned(out, [src_L[b // C.N] for b in range(B)], 0.0, pipe, "source, no guard", extra=extra)
    # a given reference overrides the decoded source
    given = plain[:1] * 0.25
    out = pipe(generator=gen(), target_loudness="source", loudness_reference=given[0], peak_limit_db=None, **kw).audios
    given_L = O.loudness(given[0].numpy())
    assert min(O.gate_margin(given_L)) >= 1.0
    check_returned(out, [given_L.L] * B, 0.0, pipe, "given reference", extra=max(8.0 * abs(O.loudness(given[0].numpy(), dtype=np.float32).L - given_L.L), 2e-5))
    assert isinstance(pipe(generator=gen(), target_loudness=-23.0, **dict(kw, output_type="np")).audios, np.ndarray)
    lat = pipe(generator=gen(), target_loudness=-23.0, **dict(kw, output_type="latent")).audios
    assert lat.shape[1:] == small.source.shape[1:]  # the latent exit comes before the stage


def test_ranking_sees_the_normalised_candidates(dev, small):
    """rank_by="chroma" with a target: chroma similarity is level-invariant, so the order is the un-normalised call's and every returned
    clip is at the target"""
    import ap_adapter_amd as A
    import test_gpu_chroma as C
    pipe = A.AudioLDM2Pipeline(small.unet, vae=small.vae, vocoder=small.voc)
    kw = dict(source_latents=small.source, **small.kw)
    gen = lambda: torch.Generator().manual_seed(C.SEED)
    cand = pipe(generator=gen(), **kw).audios
    ranked = pipe(generator=gen(), rank_by="chroma", **kw).audios
    both = pipe(generator=gen(), rank_by="chroma", target_loudness=-23.0, peak_limit_db=None, **kw).audios
    gains = pipe.last_loudness[1].cpu()  # generation order; the returned clips are re-ordered within their groups
    assert ranked.tolist() != cand.tolist()
    for b in range(both.shape[0]):
        j = [i for i in range(cand.shape[0]) if torch.equal(ranked[b], cand[i])]
        assert len(j) == 1 and torch.equal(both[b], gains[j[0]] * cand[j[0]]), b  # the same order; each clip times its own gain


def test_no_reach(dev, small, monkeypatch):
    """with ops.loudness out of order, calls without target_loudness run as before"""
    import ap_adapter_amd as A
    import test_gpu_chroma as C
    from ap_adapter_amd import ops

    def broken(*a, **k):
        raise AssertionError("ops.loudness reached without target_loudness")

    pipe = A.AudioLDM2Pipeline(small.unet, vae=small.vae, vocoder=small.voc)
    kw = dict(source_latents=small.source, **small.kw)
    before = pipe(generator=torch.Generator().manual_seed(C.SEED), **kw).audios
    monkeypatch.setattr(ops, "loudness", broken)
    monkeypatch.setattr(ops, "loudness_gain", broken)
    assert torch.equal(pipe(generator=torch.Generator().manual_seed(C.SEED), **kw).audios, before)
    assert pipe(generator=torch.Generator().manual_seed(C.SEED), rank_by="chroma", **kw).audios.shape == before.shape
    with pytest.raises(AssertionError, match="reached"):
        pipe(generator=torch.Generator().manual_seed(C.SEED), target_loudness=-23.0, **kw)
