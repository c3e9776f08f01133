"""-m gpu: the time alignment of an edit to its reference (apad_align_corr, apad_align_apply) against the restatement in
tests/align_oracle.py and against its identities, ahead of the splice and through the pipeline.

Identities (no tolerance): on integer-valued clips every partial sum is an integer below 2^24, so the table equals the int64 oracle at
every lag whatever the order of the sums, and with it the found lag, the tie order, the applied lag; the output is the edit's bits,
shifted, with +0.0 where the edit does not reach.

Bounds on float clips, from the order csrc/align.hip states (u = 2^-24, gamma_k = k u / (1 - k u)):

  c      a term r[i] e[i + l] enters a chain of fused multiply-adds over the kept samples of its sub-chunk (4096 / G samples; G = 256 / P
         lane groups, P the power of two >= max(8, ceil((2 L + 1) / 8)), G = 1 from 129 octets on), at most 4096 / G roundings; the G
         sub-chunk sums are added in order, G - 1 roundings; the chunk sums in order, ceil(n / 4096) - 1 roundings:
         k = 4096 / G + G - 1 + ceil(n / 4096) - 1 <= 4096 + ceil(n / 4096), and |c - c64| <= gamma_k sum |r e|  (``k_table``).
  E      the three energies: a thread's chain takes at most ceil(len / 1024) fused multiply-adds per kept interval, then 6 butterfly and
         15 serial additions, all terms non-negative: relative error gamma_(k_e), k_e = sum ceil(len / 1024) + 21  (``k_energy``).
  ncc    D = sqrt(E_r E_e): relative error gamma_(k_e) from the energies (two of them under a square root) + 2 u (product, root); the
         quotient adds u; sum |r e| <= D64.  |ncc - ncc64| <= gamma_k (sum |r e| / D64) + gamma_(k_e + 4) (|ncc64| + gamma_k)
         (``bound_ncc``).
  lag    the condition, asserted on the oracle first: the winner leads the runner-up by more than twice the largest bound of a c; then the
         device's found lag must be the planted one.

Every figure is printed before it is asserted.  Measured on the MI355X: the integer tables equal the int64 oracle at every lag (largest |c|
759150); on the float clips the winner leads by 9.4e-3 .. 1.2e-1 of c against bounds of 9.5e-6 .. 2.5e-4 of it, the table is within 0.3 % ..
2.4 % of its bound, ncc within 5e-8 .. 3.9e-7 (bounds 1.1e-5 .. 2.5e-4), E_r within 7e-8 relative (bounds from 1.5e-6).
"""
import functools

import numpy as np
import pytest
import torch

import align_oracle as O
import splice_oracle as SO
from util import nan_fill_free

pytestmark = pytest.mark.gpu

U = SO.U
CASES = {  # (n, regions, W, M, L, planted lag)
    "small": (6399, [(2560, 3840)], 64, 192, 16, 5),             # more than one chunk, far fewer lags than threads
    "neg_extreme": (6399, [(2560, 3840)], 64, 192, 16, -16),     # the winner at the table's edge
    "at_start": (6400, [(0, 1280)], 64, 192, 100, 100),          # one kept interval, lag = +L
    "straddle": (12000, [(3900, 4500), (8000, 8640)], 64, 192, 100, -37),  # intervals across both chunk boundaries
    "max_L": (20000, [(9000, 10000)], 64, 192, 1024, 777),       # 2049 lags: more than one octet per lane, the largest LDS window
    "product": (163840, [(48000, 80000), (120000, 131072)], 480, 1280, 320, -123),  # the workload's own shape
}
FILL = -7777


def k_table(n, L):
    octets = -(-(2 * L + 1) // 8)
    P = 8
    while P < octets and P < 256:
        P *= 2
    G = 256 // P
    return 4096 // G + G - 1 + -(-n // 4096) - 1


def k_energy(kept):
    return sum(-(-(hi - lo) // 1024) for lo, hi in kept) + 21


def bound_ncc(k, ke, mag, d64, ncc64):
    return SO.gamma(k) * mag / d64 + SO.gamma(ke + 4) * (abs(ncc64) + SO.gamma(k))


def nan(*shape, dev):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=dev)


@functools.lru_cache(maxsize=None)
def planted(name, integer=False):
    n, regions, W, M, L, lag = CASES[name]
    e, r, kept = O.planted(n, regions, W, M, L, lag, seed=len(name), integer=integer)
    e.setflags(write=False), r.setflags(write=False)
    return e, r, kept, L


@functools.lru_cache(maxsize=None)
def oracle(name, integer=False):
    e, r, kept, L = planted(name, integer)
    return O.align(e, r, kept, L, integer=integer)


def rows(clips, given=False):
    from ap_adapter_amd import align
    return torch.tensor([align.plan_row(None if given else align.Plan(len(c[0]), c[3], list(c[2]))) for c in clips], dtype=torch.int32)


def launch(clips, dev, min_corr=0.5, lag=None, ref_index=None, refs=None, mutate=None, raw=False, chunks=None, lags=None):
    """both launches on NaN-filled float outputs and sentinel-filled integer ones.  clips: [(e, r, kept, L)]; ``lag`` a list: the given-lag
    mode (no partial).  ``mutate(plan_host)`` edits the table first; ``raw`` calls the C entry points and returns their statuses."""
    from ap_adapter_amd import _lib, ops
    B = len(clips)
    refs = [c[1] for c in clips] if refs is None else refs
    ref_index = list(range(B)) if ref_index is None else ref_index
    oh = torch.zeros(B + 1, dtype=torch.int64)
    oh[1:] = torch.cumsum(torch.tensor([len(c[0]) for c in clips]), 0)
    roh = torch.zeros(len(refs) + 1, dtype=torch.int64)
    roh[1:] = torch.cumsum(torch.tensor([len(r) for r in refs]), 0)
    e = torch.from_numpy(np.concatenate([c[0] for c in clips]).astype(np.float32)).to(dev)
    r = torch.from_numpy(np.concatenate(refs).astype(np.float32)).to(dev)
    ph = rows(clips, lag is not None)
    if mutate is not None:
        mutate(ph)
    ih = torch.tensor(ref_index, dtype=torch.int32)
    chunks = max(-(-len(c[0]) // 4096) for c in clips) if chunks is None else chunks
    lags = 2 * max(c[3] for c in clips) + 1 if lags is None else lags
    partial = None if lag is not None else nan(B, chunks, lags, dev=dev)
    lag_in = None if lag is None else torch.tensor(lag, dtype=torch.int32).to(dev)
    out, stats, corr = nan(e.numel(), dev=dev), nan(B, 4, dev=dev), nan(B, lags, dev=dev)
    lo = torch.full((B, 2), FILL, dtype=torch.int32, device=dev)
    common = (e, oh.to(dev), oh, r, roh.to(dev), roh, ih.to(dev), ih, ph.to(dev), ph)
    if raw:
        p = lambda t: None if t is None else t.data_ptr()
        lib, st = _lib.lib(), torch.cuda.current_stream().cuda_stream
        rc_corr = lib.apad_align_corr(*(p(t) for t in common), p(partial if partial is not None else corr), B, len(refs), chunks, lags, st)
        rc_apply = lib.apad_align_apply(*(p(t) for t in common), p(partial), p(lag_in), p(out), p(lo), p(stats), p(corr), B, len(refs), chunks, lags,
                                        float(min_corr), st)
        torch.cuda.synchronize()
        return rc_corr, rc_apply, out, lo, stats, corr, partial
    if partial is not None:
        ops.align_corr(*common, partial)
    ops.align_apply(*common, out, lo, stats, min_corr, partial=partial, lag_in=lag_in, corr_out=corr)
    assert not torch.isnan(stats).any() and bool((lo != FILL).all())
    outs = [out[int(oh[b]): int(oh[b + 1])] for b in range(B)]
    return outs, lo.cpu(), stats.cpu(), corr.cpu()


def same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


def check_exact(name, out, lo, corr, res, L):
    got = corr[:2 * L + 1].double().numpy()
    worst = int(np.abs(got - res.c).max())
    print(f"{name}: {2 * L + 1} lags, largest |c| {int(np.abs(res.c).max())}, largest deviation from the int64 table {worst}; found "
          f"{lo.tolist()} (oracle {res.found}, {res.applied})")
    assert int(np.abs(res.c).max()) < 2 ** 24 and np.array_equal(got, res.c.astype(np.float64))
    assert bool(torch.isnan(corr[2 * L + 1:]).all())  # entries past the clip's own 2 L + 1 are not written
    assert lo.tolist() == [res.found, res.applied]
    assert same_bits(out.cpu().numpy(), res.out)


@pytest.mark.parametrize("name", list(CASES))
def test_exact_table(dev, name):
    e, r, kept, L = planted(name, True)
    res = oracle(name, True)
    assert res.found == CASES[name][5] == res.applied
    (out,), lo, stats, corr = launch([(e, r, kept, L)], dev)
    check_exact(name, out, lo[0], corr[0], res, L)
    assert float(stats[0, 2]) == float(res.c[res.found + L]) and float(stats[0, 3]) == res.er


def test_exact_table_ragged_batch(dev):
    """all six in one batch, each with its own L: the row stride of partial and corr_out is the largest clip's"""
    clips = [planted(k, True) for k in CASES]
    outs, lo, stats, corr = launch(clips, dev)
    for b, name in enumerate(CASES):
        check_exact(name, outs[b], lo[b], corr[b], oracle(name, True), clips[b][3])


@pytest.mark.parametrize("lag,rivals", [(3, (-13, -5, 11)), (4, (-4, -12, 12))])
def test_tie_order(dev, lag, rivals):
    """a signal of period 8: the table ties exactly at lag + 8 m; the smaller |l| wins, then l >= 0"""
    n, L = 6399, 16
    e, r = O.periodic(n, L, lag)
    kept = O.kept_set(n, [(2560, 3840)], 64, 192, L)
    res = O.align(e, r, kept, L, integer=True)
    assert res.found == lag and all(res.c[v + L] == res.c[lag + L] for v in rivals)
    (out,), lo, stats, corr = launch([(e, r, kept, L)], dev)
    check_exact(f"period 8, lag {lag}", out, lo[0], corr[0], res, L)
    assert all(float(corr[0, v + L]) == float(corr[0, lag + L]) for v in rivals)
    assert float(stats[0, 0]) == 1.0  # the energies are integers too, and equal: c / sqrt(c c)


@pytest.mark.parametrize("name", list(CASES))
def test_planted_lag_against_fp64(dev, name):
    n, regions, W, M, L, lag = CASES[name]
    e, r, kept, _ = planted(name)
    res = oracle(name)
    k, ke = k_table(n, L), k_energy(kept)
    bound_c = SO.gamma(k) * res.mag
    two = np.sort(res.c)[-2:]
    print(f"{name}: k = {k}, k_e = {ke}; winner c = {two[1]:.6e} at {res.found}, runner-up {two[0]:.6e} (lead {(two[1] - two[0]) / two[1]:.2e} of it), "
          f"largest bound of a c {bound_c.max():.3e} ({bound_c.max() / two[1]:.2e} of it); ncc {res.ncc:.6f}, ncc(0) {res.ncc0:.6f}")
    assert res.found == lag == res.applied and two[1] - two[0] > 2 * bound_c.max()  # the condition, on the oracle alone
    (out,), lo, stats, corr = launch([(e, r, kept, L)], dev)
    err = np.abs(corr[0, :2 * L + 1].double().numpy() - res.c)
    print(f"{name}: table: largest error / bound {float((err / bound_c).max()):.4f} (largest error {err.max():.3e})")
    assert (err <= bound_c).all()
    assert lo[0].tolist() == [lag, lag]
    assert same_bits(out.cpu().numpy(), O.shift(e, lag))
    edge = out[n - lag:] if lag > 0 else out[:-lag]
    assert lag == 0 or (edge.numel() == abs(lag) and bool((edge.cpu().view(torch.int32) == 0).all()))  # +0.0, not -0.0
    d_star = np.sqrt(res.er * O.energy(e, kept, lag))
    d_zero = np.sqrt(res.er * O.energy(e, kept))
    b_star, b_zero = bound_ncc(k, ke, res.mag[lag + L], d_star, res.ncc), bound_ncc(k, ke, res.mag[L], d_zero, res.ncc0)
    got = stats[0].double().numpy()
    print(f"{name}: ncc {got[0]:.7f} (oracle {res.ncc:.7f}, error {abs(got[0] - res.ncc):.2e}, bound {b_star:.2e}); ncc(0) {got[1]:.7f} (oracle "
          f"{res.ncc0:.7f}, error {abs(got[1] - res.ncc0):.2e}, bound {b_zero:.2e}); E_r relative error {abs(got[3] - res.er) / res.er:.2e} "
          f"(bound {SO.gamma(ke):.2e})")
    assert abs(got[0] - res.ncc) <= b_star and abs(got[1] - res.ncc0) <= b_zero
    assert got[2] == float(corr[0, lag + L]) and abs(got[3] - res.er) <= SO.gamma(ke) * res.er
    assert got[0] > 0.98 and got[1] < 0.9


def test_gate(dev):
    """an edit of independent white noise: the found lag and the stats are reported, nothing is applied"""
    n, regions, W, M, L, _ = CASES["small"]
    _, r, kept, _ = planted("small")
    e = (0.2 * np.random.default_rng(5).standard_normal(n)).astype(np.float32)
    res = O.align(e, r, kept, L)
    k, ke = k_table(n, L), k_energy(kept)
    b = bound_ncc(k, ke, res.mag[res.found + L], np.sqrt(res.er * O.energy(e, kept, res.found)), res.ncc)
    two = np.sort(res.c)[-2:]
    decided = two[1] - two[0] > 2 * (SO.gamma(k) * res.mag).max()
    print(f"white noise: oracle lag {res.found}, ncc {res.ncc:.4f} (bound {b:.2e}), c {two[1]:.4e}, runner-up {two[0]:.4e}: "
          f"{'decided' if decided else 'a tie within the bound'}")
    assert res.ncc < 0.5 - b and res.applied == 0 and res.c[res.found + L] > 0  # the condition, on the oracle alone
    (out,), lo, stats, corr = launch([(e, r, kept, L)], dev)
    found = int(lo[0, 0])
    print(f"white noise: device lag {lo[0].tolist()}, stats {stats[0].tolist()}")
    assert -L <= found <= L and (not decided or found == res.found) and int(lo[0, 1]) == 0
    assert abs(float(stats[0, 0]) - O.ncc(res.c[found + L], res.er, O.energy(e, kept, found))) <= b and float(stats[0, 2]) == float(corr[0, found + L])
    assert torch.equal(out.cpu(), torch.from_numpy(e)) and same_bits(out.cpu().numpy(), e)
    # no floor: the found lag is applied iff its c is positive
    (out2,), lo2, stats2, corr2 = launch([(e, r, kept, L)], dev, min_corr=-1.0)
    assert torch.equal(corr2, corr) and torch.equal(stats2, stats) and int(lo2[0, 0]) == found
    assert int(lo2[0, 1]) == (found if float(stats[0, 2]) > 0 else 0) and same_bits(out2.cpu().numpy(), O.shift(e, int(lo2[0, 1])))
    pos = (np.abs(r) + 1.0).astype(np.float32)  # every product negative: c < 0 at every lag, nothing is applied even without a floor
    (out3,), lo3, stats3, _ = launch([(-pos, pos, kept, L)], dev, min_corr=-1.0)
    print(f"anti-correlated: lags {lo3[0].tolist()}, stats {stats3[0].tolist()}")
    assert float(stats3[0, 2]) < 0 and float(stats3[0, 0]) < 0 and int(lo3[0, 1]) == 0 and same_bits(out3.cpu().numpy(), -pos)


def test_given_lag(dev):
    """nothing is measured and partial is not read (there is none); whatever the lag, nothing outside the clip is read"""
    e, r, kept, L = planted("small")
    n = len(e)
    given = [0, 7, -n + 1, n - 1, 2 ** 31 - 1, -2 ** 31]
    outs, lo, stats, corr = launch([(e, r, (), L)] * len(given), dev, lag=given)
    assert bool(torch.isnan(corr).all()) and bool((stats == 0).all())
    for b, lag in enumerate(given):
        assert lo[b].tolist() == [lag, lag] and same_bits(outs[b].cpu().numpy(), O.shift(e, lag) if abs(lag) < n else np.zeros(n, np.float32)), lag
    assert same_bits(outs[2].cpu().numpy()[-1:], e[:1]) and not outs[2][:-1].any() and same_bits(outs[0].cpu().numpy(), e)


def test_reach(dev):
    """NaN in e and r inside the region, more than L from every kept interval: no bit of any result moves"""
    e, r, kept, L = planted("small")
    clean = launch([(e, r, kept, L)], dev)
    e2, r2 = e.copy(), r.copy()
    e2[2600:3800], r2[2600:3800] = np.nan, np.nan
    r2[:L], r2[-L:] = np.nan, np.nan  # r is read on K alone
    assert all(hi + L <= 2600 or lo - L >= 3800 for lo, hi in kept)
    dirty = launch([(e2, r2, kept, L)], dev)
    for a, b in zip(clean[1:], dirty[1:]):
        assert torch.equal(a[~torch.isnan(a)], b[~torch.isnan(b)]) and torch.equal(torch.isnan(a), torch.isnan(b))
    assert same_bits(dirty[0][0].cpu().numpy(), O.shift(e2, int(clean[1][0, 1])))
    assert int(torch.isnan(dirty[0][0]).sum()) == 1200 and int(clean[1][0, 1]) == 5


def test_batch_independence(dev):
    """a clip alone against the same clip inside a ragged batch of three with larger L beside it: every output, bit for bit"""
    clips = [planted(k) for k in ("straddle", "small", "max_L")]
    alone = launch([clips[1]], dev)
    outs, lo, stats, corr = launch(clips, dev)
    nl = 2 * clips[1][3] + 1
    assert torch.equal(outs[1], alone[0][0]) and torch.equal(lo[1], alone[1][0]) and torch.equal(stats[1], alone[2][0])
    assert torch.equal(corr[1, :nl], alone[3][0, :nl]) and bool(torch.isnan(corr[1, nl:]).all())
    # shared references stored in another order
    outs2, lo2, stats2, corr2 = launch([clips[1], clips[0], clips[1]], dev, refs=[clips[0][1], clips[1][1]], ref_index=[1, 0, 1])
    for b in (0, 2):
        assert torch.equal(outs2[b], alone[0][0]) and torch.equal(stats2[b], alone[2][0]) and torch.equal(corr2[b, :nl], alone[3][0, :nl])
    assert torch.equal(outs2[1], outs[0]) and torch.equal(corr2[1, :201], corr[0, :201])  # (straddle: 2 L + 1 = 201)


def test_refusals(dev):
    from ap_adapter_amd import _lib, ops
    e, r, kept, L = planted("small")  # n = 6399, K = [16, 2352) and [4048, 6383)
    clip = (e, r, kept, L)
    n = len(e)

    def untouched(res, both=True):
        rc_corr, rc_apply, out, lo, stats, corr, partial = res
        assert rc_apply < 0 and (rc_corr < 0 or not both)
        assert bool(torch.isnan(out).all()) and bool((lo == FILL).all()) and bool(torch.isnan(stats).all()) and bool(torch.isnan(corr).all())
        assert partial is None or rc_corr == 0 or bool(torch.isnan(partial).all())

    def set_(i, v):
        def f(ph):
            ph[0, i] = v
        return f

    bad = [(set_(1, 0), "L = 0 outside"), (set_(1, 1025), "L = 1025 outside"), (set_(1, 17), "lags = 33 is below 2 L \\+ 1 = 35"),
           (set_(0, 6), "6 intervals, at most 5"), (set_(0, 0), "needs an interval"), (set_(0, -1), "-1 intervals"),
           (set_(2, 2), "mode 2 outside"), (set_(2, -1), "mode -1 outside"), (set_(2, 1), "a given lag"),
           (set_(5, 16), "interval 0 = \\[16, 16\\) is empty"), (set_(4, 15), "not inside \\[L, n - L\\) = \\[16, 6383\\)"),
           (set_(7, 6384), "interval 1 = \\[4048, 6384\\)"), (set_(6, 2351), "interval 1 = \\[2351, 6383\\) is empty, not behind"),
           (set_(6, 1000), "not behind the one before it")]
    for mutate, msg in bad:
        with pytest.raises(RuntimeError, match=msg):
            launch([clip], dev, mutate=mutate)
        untouched(launch([clip], dev, mutate=mutate, raw=True))
    assert b"not behind the one before it" in _lib.lib().apad_last_error()
    with pytest.raises(RuntimeError, match="1 chunks of 4096 do not cover 6399 samples"):
        launch([clip], dev, chunks=1)
    untouched(launch([clip], dev, chunks=1, raw=True))
    untouched(launch([clip], dev, lags=2 * L, raw=True))
    with pytest.raises(RuntimeError, match="its reference 0 has 6400"):
        launch([clip], dev, refs=[np.zeros(6400, np.float32)])
    untouched(launch([clip], dev, refs=[np.zeros(6400, np.float32)], raw=True))
    with pytest.raises(RuntimeError, match=r"ref_index\[0\] = 1 outside \[0, 1\)"):
        launch([clip], dev, ref_index=[1])
    untouched(launch([clip], dev, ref_index=[-1], raw=True))
    # a given-lag row: an interval is refused
    with pytest.raises(RuntimeError, match="a given lag takes no interval"):
        launch([(e, r, (), L)], dev, lag=[3], mutate=set_(0, 1))
    # null pointers, sizes and aliasing, through the C entry points
    lib, x = _lib.lib(), torch.zeros(n, device=dev)
    oh, ih, ph = torch.tensor([0, n]), torch.zeros(1, dtype=torch.int32), rows([clip])
    od, idd, pd = oh.to(dev), ih.to(dev), ph.to(dev)
    part, out, stats = nan(1, 2, 33, dev=dev), nan(n, dev=dev), nan(1, 4, dev=dev)
    lo = torch.full((1, 2), FILL, dtype=torch.int32, device=dev)
    p = lambda t: None if t is None else t.data_ptr()
    common = [x, od, oh, x, od, oh, idd, ih, pd, ph]

    def corr_rc(args=common, partial=part, batch=1, n_ref=1):
        return lib.apad_align_corr(*(p(t) for t in args), p(partial), batch, n_ref, 2, 33, None)

    def apply_rc(args=common, partial=part, lag_in=None, o=out, l=lo, s=stats, batch=1):
        return lib.apad_align_apply(*(p(t) for t in args), p(partial), p(lag_in), p(o), p(l), p(s), None, batch, 1, 2, 33, 0.5, None)

    for i in range(10):
        args = list(common)
        args[i] = None
        assert corr_rc(args) < 0 and b"null pointer" in lib.apad_last_error() and apply_rc(args) < 0 and b"null pointer" in lib.apad_last_error()
    assert corr_rc(partial=None) < 0 and apply_rc(o=None) < 0 and apply_rc(l=None) < 0 and apply_rc(s=None) < 0
    assert apply_rc(partial=None) < 0 and b"needs partial" in lib.apad_last_error()
    assert apply_rc(o=x) < 0 and b"out must not be edit or ref" in lib.apad_last_error()
    for batch in (0, -1, 65536):
        assert corr_rc(batch=batch) < 0 and apply_rc(batch=batch) < 0 and b"outside [1, 65535]" in lib.apad_last_error()
    off1 = torch.tensor([1, n + 1])
    assert corr_rc([x, od, off1] + common[3:]) < 0 and b"offsets[0]" in lib.apad_last_error()
    empty = torch.tensor([0, 0])
    assert corr_rc([x, od, empty] + common[3:]) < 0 and apply_rc([x, od, empty] + common[3:]) < 0 and b"outside [1, 2^24]" in lib.apad_last_error()
    big = torch.tensor([0, 2 ** 24 + 1])
    assert corr_rc([x, od, big, x, od, big] + common[6:]) < 0 and b"outside [1, 2^24]" in lib.apad_last_error()
    torch.cuda.synchronize()
    assert bool(torch.isnan(part).all()) and bool(torch.isnan(out).all()) and bool((lo == FILL).all()) and bool(torch.isnan(stats).all())
    with pytest.raises(RuntimeError, match="expected a GPU tensor"):
        ops.align_corr(x.cpu(), *[None] * 10)
    rc = launch([clip], dev, raw=True)  # the same operands, valid
    assert rc[0] == 0 and rc[1] == 0 and not torch.isnan(rc[2]).any() and rc[3][0].tolist() == [5, 5]


def test_graph_capture(dev):
    """both launches recorded in a hipGraph and replayed twice on new contents of the same buffers equal eager, bit for bit"""
    from ap_adapter_amd import ops
    names = ("small", "straddle")
    clips = [planted(k) for k in names]
    oh = torch.zeros(3, dtype=torch.int64)
    oh[1:] = torch.cumsum(torch.tensor([len(c[0]) for c in clips]), 0)
    od = oh.to(dev)
    first = torch.from_numpy(np.concatenate([c[0] for c in clips])).to(dev)
    first_r = torch.from_numpy(np.concatenate([c[1] for c in clips])).to(dev)
    other = [O.planted(*CASES[k][:5], lag, seed=77) for k, lag in zip(names, (-9, 64))]
    second, second_r = (torch.from_numpy(np.concatenate([c[i] for c in other])).to(dev) for i in (0, 1))
    ph = rows(clips)
    pd, ih = ph.to(dev), torch.tensor([0, 1], dtype=torch.int32)
    idd = ih.to(dev)
    e, r = first.clone(), first_r.clone()
    partial, out, stats, corr = nan(2, 3, 201, dev=dev), nan(e.numel(), dev=dev), nan(2, 4, dev=dev), nan(2, 201, dev=dev)
    lo = torch.full((2, 2), FILL, dtype=torch.int32, device=dev)
    bufs = (partial, out, lo, stats, corr)

    def run():
        ops.align_corr(e, od, oh, r, od, oh, idd, ih, pd, ph, partial)
        ops.align_apply(e, od, oh, r, od, oh, idd, ih, pd, ph, out, lo, stats, 0.5, partial=partial, corr_out=corr)

    def fill():
        for t in bufs:
            t.fill_(float("nan") if t.is_floating_point() else FILL)

    run()  # (loads the library outside the capture)
    lo_first = lo.clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        run()
    e.copy_(second), r.copy_(second_r)
    got = []
    for _ in range(2):
        fill()
        g.replay()
        torch.cuda.synchronize()
        got.append([t.clone() for t in bufs])
    fill()
    run()
    torch.cuda.synchronize()
    same = lambda a, b: torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.nan_to_num(a), torch.nan_to_num(b))
    for rep in got:
        assert all(same(a.float(), b.float()) for a, b in zip(rep, bufs)) and not torch.isnan(rep[1]).any()
    print(f"graph: first contents {lo_first.tolist()}, replay on the second {got[0][2].tolist()}")
    assert got[0][2].tolist() == [[-9, -9], [64, 64]] and lo_first.tolist() == [[5, 5], [-37, -37]]  # the replay read the new contents


def halves(n=4160, lag=37):
    """r on a grid of 2^-12 (so that every product of the crossfade with a weight k / 128 is exact), e[i + lag] = r[i] / 2 exactly"""
    x = np.round(SO.signal(n + 2 * lag, seed=8).astype(np.float64) * 4096.0) / 4096.0
    return (0.5 * x[:n]).astype(np.float32), x[lag:lag + n].astype(np.float32)


def test_with_the_splice(dev):
    """an edit that is the recording at half the level, 37 samples late: aligned first, the splice finds identical signals -- every seam
    cost 0, and the whole clip comes back as the recording (W = 64: the weights are k / 128, the products exact on r's grid, rho == 1);
    spliced as it is, the seams see two different signals"""
    import ap_adapter_amd as A
    n, lag = 4160, 37
    e, r = halves(n, lag)
    assert np.array_equal(e[lag:], 0.5 * r[:n - lag])
    kw = dict(regions=(1920 / 16000.0, 2560 / 16000.0), crossfade_s=64 / 16000.0, seam_search_s=192 / 16000.0, gain=2.0, return_plan=True)
    nan_fill_free(dev)
    et, rt = torch.from_numpy(e).to(dev), torch.from_numpy(r).to(dev)
    out, gains, starts, stats, plans, lags, astats = A.splice_edit_aligned(et, rt, align="kept", **kw)
    print(f"aligned: lags {lags.tolist()}, align stats {astats.tolist()}, seam costs {stats[0, :2, 0].tolist()}, starts {starts[0, :2].tolist()}")
    assert lags.tolist() == [[lag, lag]] and float(gains[0]) == 2.0 and plans[0].kept == [(0, 1728), (2752, 4160)]
    assert float(stats[0, :, 0].max()) == 0.0 and starts[0, :2].tolist() == [1920 - 64, 2560]
    assert torch.equal(out, rt) and same_bits(out.cpu().numpy(), r)
    assert float(astats[0, 0]) > 0.999 and float(astats[0, 0]) > float(astats[0, 1])
    plain = A.splice_edit(et, rt, **kw)
    print(f"as it is: seam costs {plain[3][0, :2, 0].tolist()}")
    assert float(plain[3][0, :2, 0].min()) > 0.0 and not torch.equal(plain[0], rt)
    assert len(plain) == 5 and torch.equal(A.splice_edit_aligned(et, rt, align=None, **kw)[0], plain[0])
    # the same as splicing the edit shifted beforehand; a given lag; align_edit alone
    shifted = torch.from_numpy(O.shift(e, lag)).to(dev)
    pre = A.splice_edit(shifted, rt, **kw)
    assert torch.equal(pre[0], out) and torch.equal(pre[2], starts) and torch.equal(pre[3], stats)
    given = A.splice_edit_aligned(et, rt, align=lag, **kw)
    assert torch.equal(given[0], out) and given[5].tolist() == [[lag, lag]] and not given[6].any()
    al, l2, s2 = A.align_edit(et, rt, regions=kw["regions"], splice_margins=(kw["crossfade_s"], kw["seam_search_s"]))
    assert torch.equal(al, shifted) and torch.equal(l2, lags) and torch.equal(s2, astats)
    whole, l3, _ = A.align_edit([e, e[:3000]], [r, r[:3000]], search_s=0.004)
    assert isinstance(whole, list) and l3.tolist() == [[lag, lag]] * 2 and same_bits(whole[1].cpu().numpy(), O.shift(e[:3000], lag))
    back, l4, s4 = A.align_edit(torch.from_numpy(np.stack([e, e])), r, lag=[0, -5])
    assert back.shape == (2, n) and l4.tolist() == [[0, 0], [-5, -5]] and not s4.any() and same_bits(back[1].cpu().numpy(), O.shift(e, -5))


# ---- through the pipeline: the small synthetic UNet, VAE and vocoder of the chroma tests ----
@pytest.fixture(scope="module")
def small(dev):
    import test_gpu_chroma as C
    return C.build_small(dev)


REGION = (0.2, 0.36)  # latent rows 5 .. 8: samples [3200, 5760) of 10240; the splice keeps [0, 1920) and [7040, 10240)
LAG = 23


def test_pipeline_aligns_before_the_splice(dev, small):
    import ap_adapter_amd as A
    import test_gpu_chroma as C
    pipe = A.AudioLDM2Pipeline(small.unet, vae=small.vae, vocoder=small.voc)
    kw = dict(source_latents=small.source, edit_region=REGION, **small.kw)
    gen = lambda: torch.Generator().manual_seed(C.SEED)
    plain = pipe(generator=gen(), **kw).audios
    assert pipe.last_align is None
    ref = torch.roll(plain, -LAG, dims=1)  # ref[i] = plain[i + LAG]: the rendering is LAG samples late
    nan_fill_free(dev)
    out = pipe(generator=gen(), splice="source", splice_reference=ref, align="kept", **kw).audios
    lags, stats = (t.cpu() for t in pipe.last_align)
    B, n = plain.shape
    print(f"pipeline: lags {lags.tolist()}, ncc {stats[:, 0].tolist()}, ncc(0) {stats[:, 1].tolist()}, gains {pipe.last_splice[0].tolist()}")
    assert pipe.last_align[0].is_cuda and tuple(lags.shape) == (B, 2) and tuple(stats.shape) == (B, 4) and out.shape == plain.shape
    assert lags.tolist() == [[LAG, LAG]] * B and bool((stats[:, 0] > stats[:, 1]).all()) and bool((stats[:, 0] > 0.999).all())
    starts = pipe.last_splice[1].cpu()
    keep = torch.ones(n, dtype=torch.bool)
    for b in range(B):
        keep[:] = True
        keep[int(starts[b, 0]): int(starts[b, 1]) + 480] = False  # from the left window's start to the right window's end
        assert int(keep.sum()) >= 1920 + 3200 and torch.equal(out[b][keep], ref[b][keep]), b
    cost_aligned = float(pipe.last_splice[2][:, :2, 0].max())  # (not 0: the last LAG samples of the shifted edit are zeros, and the gain sees them)
    # a given lag: the same shift, nothing measured
    given = pipe(generator=gen(), splice="source", splice_reference=ref, align=LAG, **kw).audios
    assert torch.equal(given, out) and pipe.last_align[0].tolist() == [[LAG, LAG]] * B and not pipe.last_align[1].any()
    # without align the seams see two different signals, and last_align is reset
    none = pipe(generator=gen(), splice="source", splice_reference=ref, **kw).audios
    cost_plain = float(pipe.last_splice[2][:, :2, 0].min())
    print(f"pipeline: largest seam cost aligned {cost_aligned:.3e}, smallest seam cost spliced as it is {cost_plain:.3e}")
    assert pipe.last_align is None and cost_aligned < 0.01 * cost_plain and not torch.equal(none, out)
    with pytest.raises(ValueError, match="align_search_s"):
        pipe(generator=gen(), splice="source", splice_reference=ref, align="kept", align_search_s=0.1, **kw)
    with pytest.raises(ValueError, match="without splice= it has no use"):
        pipe(generator=gen(), align="kept", **kw)


def test_no_reach(dev, small, monkeypatch):
    """with ops.align_corr and ops.align_apply out of order, calls without align= run as before"""
    import ap_adapter_amd as A
    import test_gpu_chroma as C
    from ap_adapter_amd import ops

    def broken(*a, **k):
        raise AssertionError("the alignment reached without align=")

    pipe = A.AudioLDM2Pipeline(small.unet, vae=small.vae, vocoder=small.voc)
    kw = dict(source_latents=small.source, edit_region=REGION, **small.kw)
    gen = lambda: torch.Generator().manual_seed(C.SEED)
    ref = torch.from_numpy(SO.signal(C.LEN, seed=41))
    before = pipe(generator=gen(), **kw).audios
    spliced = pipe(generator=gen(), splice="source", splice_reference=ref, **kw).audios
    monkeypatch.setattr(ops, "align_corr", broken)
    monkeypatch.setattr(ops, "align_apply", broken)
    assert torch.equal(pipe(generator=gen(), **kw).audios, before)
    assert torch.equal(pipe(generator=gen(), splice="source", splice_reference=ref, align=None, **kw).audios, spliced) and pipe.last_align is None
    e, r = halves()
    assert A.splice_edit(torch.from_numpy(e).to(dev), torch.from_numpy(r).to(dev), (0.12, 0.16))[0].shape == (4160,)
    with pytest.raises(AssertionError, match="reached"):
        pipe(generator=gen(), splice="source", splice_reference=ref, align="kept", **kw)
    with pytest.raises(AssertionError, match="reached"):
        pipe(generator=gen(), splice="source", splice_reference=ref, align=3, **kw)
