"""-m gpu: the splice of a region edit into its reference recording (apad_splice) against the fp64 restatement in tests/splice_oracle.py
and against its identities, and ``splice="source"`` through the pipeline.

Identities (no tolerance): outside regions and crossfade windows the output is the reference's bits; between a region's two windows it is
fp32(g) * e, one multiply, with g read back; e = r / 2 gives g == 2 and e = r gives g == 1 with every cost 0.

Bounds, from the kernel's operations (u = 2^-24, gamma_k = k u / (1 - k u); the oracle is given the kernel's own g, so ge holds the same
fp32 values on both sides):

  g      each of the two sums is one fused multiply-add per kept sample in the lane (at most k_l = the sum over the kept intervals of
         ceil(length / 1024) of them), 6 butterfly additions and 15 serial ones, all terms non-negative: relative error gamma_(k_l + 22).
         The quotient of the two, a correctly rounded division and square root: |g - g64| / g64 <= (k_l + 22) u + 1.5 u; asserted with
         (k_l + 24) u.
  cost   d = fl(r - ge) carries one rounding and enters squared, the sum is W fused multiply-adds in index order on non-negative terms:
         |cost - cost64| <= gamma_(W + 2) cost64.  This is "the rounding bound of a cost" of the planted-seam condition.
  rho    the three sums over the window take k_w = ceil(W / 1024) + 22 roundings each; sum |r ge| <= sqrt(sum r^2 sum ge^2), so the
         numerator is off by at most gamma_(k_w) of the denominator; the denominator by gamma_(k_w) (two sums under a square root)
         + 2 u (product, root); the quotient by u: |rho - rho64| <= (2 k_w + 4) u (the clamp does not widen it).
  window with A = |r| + |ge|: each weight is off by at most 2 u (t: one division; w_r: one subtraction), the numerator by 2 u A from the
         weights and 2 u A from its product and fused multiply-add; the denominator's square, in [1/2, 1], by 8 u from the weights,
         5 u from its five operations and 2 w_r w_e |d rho| <= |d rho| / 2, the root halves that relative to a square >= 1/2 and adds u:
         relative 14 u + |d rho| / 2; the division adds u.  With |out| <= A sqrt 2 and 1 / den <= sqrt 2:
         |out - out64| <= A (27 u + 0.71 |d rho|), |d rho| the bound above (0 for the fixed shapes).
  e = r  rho is exactly 1 (sqrt(fl(x x)) == x) and the output is r (w_r + w_e (1 + d1)) (1 + d2) / ((w_r + w_e) (1 + 2.5 u)) (1 + d3):
         |out - r| <= 5.5 u |r| + O(u^2); asserted with 6 u |r|, three units in the last place at the most.

  starts on the planted seams and on the partly correlated clips the oracle's runner-up is further from its minimum than twice the rounding
         bound of a cost (asserted on the oracle first), and the starts must be the oracle's.  Through the pipeline nothing plants a window
         and two candidates may tie within that bound; what holds of any fp32 search with the cost bound above: it picks s with
         cost32(s) <= cost32(s*), so cost64(s) (1 - gamma) <= cost64(s*) (1 + gamma) and cost64(s) - cost64(s*) <= 2 gamma_(W + 2) cost64(s).
         That is asserted, and equality of the starts wherever the oracle's minimum is decided beyond it.

Every figure is printed before it is asserted.  Measured on the MI355X: g within 4e-8 .. 1e-7 of fp64 (bounds 1.9e-6 .. 8.2e-6), costs within
2.7e-20 (bounds from 4e-20), rho within 1.2e-7 (bound 3.0e-6), window samples within 5 % of their bound, |out - r| = 0 for e = r.
"""
import functools

import numpy as np
import pytest
import torch

import splice_oracle as O
from util import nan_fill_free

pytestmark = pytest.mark.gpu

U = O.U
SMALL = (4160, [(1920, 2560)], 64, 192)
CASES = {
    "small": SMALL,
    "odd": (4161, [(1920, 2561)], 63, 191),         # an odd length, an odd W, an odd M
    "m_is_w": (4160, [(1920, 2560)], 64, 64),        # one candidate per seam
    "at_start": (4160, [(0, 640)], 64, 192),         # no left seam
    "to_the_end": (4160, [(3000, 4120)], 64, 192),   # fewer than W samples to the end: no right seam
    "two": (9000, [(1500, 2500), (5000, 6000)], 64, 192),
    "wide": (40000, [(20000, 21000)], 100, 8192),    # the largest span: every LDS word, eight candidates per lane
    "product": (163840, [(48000, 80000), (120000, 131072)], 480, 1280),
}


def nan(*shape, dev):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=dev)


@functools.lru_cache(maxsize=None)
def planted(name):
    n, regions, W, M = CASES[name]
    return O.planted(n, regions, W, M, seed=len(name))


def launch(clips, dev, shape=0, gain=None, ref_index=None, refs=None, mutate=None, raw=False):
    """ops.splice on NaN-filled outputs.  clips: [(e, r, regions, W, M)]; refs / ref_index override the references (default: each clip's
    own).  ``mutate(plan_host)`` edits the table before the launch; ``raw`` calls the C entry point and returns its status."""
    from ap_adapter_amd import _lib, ops, splice
    B = len(clips)
    refs = [c[1] for c in clips] if refs is None else refs
    ref_index = list(range(B)) if ref_index is None else ref_index
    oh = torch.zeros(B + 1, dtype=torch.int64)
    oh[1:] = torch.cumsum(torch.tensor([len(c[0]) for c in clips]), 0)
    roh = torch.zeros(len(refs) + 1, dtype=torch.int64)
    roh[1:] = torch.cumsum(torch.tensor([len(r) for r in refs]), 0)
    e = torch.from_numpy(np.concatenate([c[0] for c in clips]).astype(np.float32)).to(dev)
    r = torch.from_numpy(np.concatenate(refs).astype(np.float32)).to(dev)
    plans = [splice.plan(len(c[0]), c[2], c[3], c[4]) for c in clips]
    ph = torch.tensor([splice.plan_row(p, shape, gain is not None) for p in plans], dtype=torch.int32)
    if mutate is not None:
        mutate(ph)
    ih = torch.tensor(ref_index, dtype=torch.int32)
    out, gains, stats = nan(e.numel(), dev=dev), nan(B, dev=dev), nan(B, 8, 2, dev=dev)
    starts = torch.full((B, 8), -7, dtype=torch.int32, device=dev)
    gin = None if gain is None else torch.full((B,), float(gain), dtype=torch.float32).to(dev)
    args = (e, oh.to(dev), oh, r, roh.to(dev), roh, ih.to(dev), ih, ph.to(dev), ph, out, gains, starts, stats)
    if raw:
        p = lambda t: None if t is None else t.data_ptr()
        rc = _lib.lib().apad_splice(*(p(t) for t in args[:10]), p(gin), *(p(t) for t in args[10:]), B, len(refs),
                                    torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return rc, out, gains, starts, stats
    ops.splice(*args, gain_in=gin)
    assert not torch.isnan(out).any() and not torch.isnan(gains).any() and not torch.isnan(stats).any() and int(starts.min()) >= -1
    outs = [out[int(oh[b]): int(oh[b + 1])] for b in range(B)]
    return outs, gains, starts, stats


def check_bits(e, r, regions, W, M, out, g, starts):
    """the identities: r's bits outside regions and windows, fp32(g) * e between a region's windows.  out / g / starts: one clip's, on the host"""
    n = len(e)
    res = O.Result(None, None, [int(s) for s in starts], None, None, None, O.plan(n, regions, W, M))
    win, edit = O.window_mask(res, W, n), O.edit_mask(res, W, n)
    for (a, b), (sl, sr) in zip(res.plan.regions, zip(res.starts[0::2], res.starts[1::2])):  # the windows lie where the plan allows
        assert (sl == -1 and a < W) or max(0, a - M) <= sl <= a - W
        assert (sr == -1 and n - b < W) or b <= sr <= min(n, b + M) - W
    o, rt, et = out.numpy(), np.asarray(r, np.float32), np.asarray(e, np.float32)
    keep = ~win & ~edit
    assert keep.any() and edit.any()
    assert np.array_equal(o[keep].view(np.uint32), rt[keep].view(np.uint32))
    assert np.array_equal(o[edit].view(np.uint32), (np.float32(g) * et)[edit].view(np.uint32))
    return win, edit


@pytest.mark.parametrize("name", list(CASES))
def test_planted_seams_and_bits(dev, name):
    n, regions, W, M = CASES[name]
    e, r, want = planted(name)
    # the condition, on the oracle alone: every seam's runner-up is further from the minimum than twice the rounding bound of a cost
    ref = O.splice(e, r, regions, W, M)
    assert ref.starts == want
    for k, c in enumerate(ref.costs):
        if c is not None and len(c) > 1:
            two = np.partition(c, 1)[:2]
            bound = O.gamma(W + 2) * two[1]
            print(f"{name}: seam {k}: {len(c)} candidates, minimum {two[0]:.4e}, runner-up {two[1]:.4e} (gap {(two[1] - two[0]) / two[1]:.2%} of it), "
                  f"rounding bound of a cost {bound:.3e} ({O.gamma(W + 2):.2e} relative)")
            assert two[1] - two[0] > 2 * bound
    (out,), gains, starts, stats = launch([(e, r, regions, W, M)], dev)
    out, g, starts, stats = out.cpu(), float(gains[0]), starts[0].cpu().tolist(), stats[0].cpu().double().numpy()
    assert starts == ref.starts
    win, _ = check_bits(e, r, regions, W, M, out, g, starts)
    p = ref.plan
    k_l = sum(-(-(hi - lo) // 1024) for lo, hi in p.kept)
    bound_g = (k_l + 24) * U
    print(f"{name}: g {g:.8f}, oracle {ref.g:.8f}, relative error {abs(g - ref.g) / ref.g:.3e}, bound {bound_g:.3e}")
    assert abs(g - ref.g) / ref.g <= bound_g
    same_g = O.splice(e, r, regions, W, M, gain=g)  # the kernel's own g: ge holds the same fp32 values on both sides
    assert same_g.starts == starts
    k_w = -(-W // 1024) + 22
    bound_rho = (2 * k_w + 4) * U
    for k, s in enumerate(starts):
        if s < 0:
            assert stats[k].tolist() == [0.0, 0.0]
            continue
        err_c, bound_c = abs(stats[k, 0] - same_g.cost[k]), O.gamma(W + 2) * same_g.cost[k]
        err_r = abs(stats[k, 1] - same_g.rho[k])
        print(f"{name}: seam {k} at {s}: cost {stats[k, 0]:.6e} (oracle {same_g.cost[k]:.6e}, error {err_c:.2e}, bound {bound_c:.2e}); rho "
              f"{stats[k, 1]:.7f} (oracle {same_g.rho[k]:.7f}, error {err_r:.2e}, bound {bound_rho:.2e})")
        assert err_c <= bound_c and err_r <= bound_rho
    A = np.abs(r.astype(np.float64)) + np.abs((np.float32(g) * e).astype(np.float64))
    err = np.abs(out.double().numpy() - same_g.out)
    bound_w = A * (27 * U + 0.71 * bound_rho)
    print(f"{name}: window samples: largest error / bound {float((err[win] / bound_w[win]).max()):.3f}")
    assert (err[win] <= bound_w[win]).all()


def decorrelated(n, seed):
    """an edit that shares only part of the reference: e = 0.6 r + noise of r's size, everywhere -- the windows' correlation is near 0.5"""
    r = O.signal(n, seed)
    noise = np.random.default_rng(seed + 500).standard_normal(n) * float(r.std())
    return (0.6 * r + 0.9 * noise).astype(np.float32), r


@pytest.mark.parametrize("name", ["small", "odd", "two"])
def test_matched_crossfade_of_partly_correlated_signals(dev, name):
    """no planted window: the minimum is whatever the signals give (the same condition is asserted on the oracle first), rho is well inside
    (0, 1) and the matched crossfade differs from both fixed shapes"""
    n, regions, W, M = CASES[name]
    e, r = decorrelated(n, 11 + len(name))
    (out,), gains, starts, stats = launch([(e, r, regions, W, M)], dev)
    out, g, starts, stats = out.cpu(), float(gains[0]), starts[0].cpu().tolist(), stats[0].cpu().double().numpy()
    ref = O.splice(e, r, regions, W, M, gain=g)
    for k, c in enumerate(ref.costs):
        if c is not None:
            two = np.partition(c, 1)[:2]
            print(f"{name}: seam {k}: minimum {two[0]:.6e}, runner-up {two[1]:.6e} (gap {(two[1] - two[0]) / two[1]:.3%}), rounding bound of a "
                  f"cost {O.gamma(W + 2) * two[1]:.3e}; rho {ref.rho[k]:.4f}")
            assert two[1] - two[0] > 2 * O.gamma(W + 2) * two[1]
            assert 0.2 < ref.rho[k] < 0.8
    assert starts == ref.starts
    win, _ = check_bits(e, r, regions, W, M, out, g, starts)
    bound_rho = (2 * (-(-W // 1024) + 22) + 4) * U
    for k, s in enumerate(starts):
        if s >= 0:
            assert abs(stats[k, 0] - ref.cost[k]) <= O.gamma(W + 2) * ref.cost[k] and abs(stats[k, 1] - ref.rho[k]) <= bound_rho
    A = np.abs(r.astype(np.float64)) + np.abs((np.float32(g) * e).astype(np.float64))
    err = np.abs(out.double().numpy() - ref.out)
    bound_w = A * (27 * U + 0.71 * bound_rho)
    print(f"{name}: window samples: largest error / bound {float((err[win] / bound_w[win]).max()):.3f}")
    assert (err[win] <= bound_w[win]).all()
    for shape in ("linear", "equal_power"):
        assert np.abs(O.splice(e, r, regions, W, M, shape=shape, gain=g).out - ref.out)[win].max() > 1e-3


def test_exact_half(dev):
    n, regions, W, M = SMALL
    r = O.signal(n, seed=5)
    e = (0.5 * r.astype(np.float64)).astype(np.float32)
    (out,), gains, starts, stats = launch([(e, r, regions, W, M)], dev)
    assert float(gains[0]) == 2.0 and float(stats[0, :, 0].max()) == 0.0
    win, _ = check_bits(e, r, regions, W, M, out.cpu(), 2.0, starts[0].cpu())
    assert np.array_equal(out.cpu().numpy()[~win].view(np.uint32), r[~win].view(np.uint32))  # 2 (r / 2) is r: the whole clip outside the windows


def test_exact_same(dev):
    n, regions, W, M = SMALL
    r = O.signal(n, seed=6)
    (out,), gains, starts, stats = launch([(r, r, regions, W, M)], dev)
    assert float(gains[0]) == 1.0 and bool((stats[0, :, 0] == 0).all())
    assert starts[0].cpu().tolist() == [1920 - W, 2560] + [-1] * 6  # every cost ties at 0: the windows nearest the region
    assert stats[0, :2, 1].cpu().tolist() == [1.0, 1.0]
    o = out.cpu().numpy()
    win, _ = check_bits(r, r, regions, W, M, out.cpu(), 1.0, starts[0].cpu())
    rel = np.abs(o.astype(np.float64) - r)[win] / np.abs(r.astype(np.float64))[win]
    print(f"e = r: largest |out - r| / |r| inside the windows {rel.max() / U:.2f} u (bound 6 u)")
    assert rel.max() <= 6 * U
    assert np.array_equal(o[~win].view(np.uint32), r[~win].view(np.uint32))


@pytest.mark.parametrize("shape", ["linear", "equal_power"])
def test_fixed_shapes(dev, shape):
    from ap_adapter_amd import splice
    n, regions, W, M = CASES["two"]
    e, r, want = planted("two")
    (out,), gains, starts, stats = launch([(e, r, regions, W, M)], dev, shape=splice.SHAPES[shape])
    g = float(gains[0])
    ref = O.splice(e, r, regions, W, M, shape=shape, gain=g)
    assert starts[0].cpu().tolist() == ref.starts == want
    win, _ = check_bits(e, r, regions, W, M, out.cpu(), g, starts[0].cpu())
    A = np.abs(r.astype(np.float64)) + np.abs((np.float32(g) * e).astype(np.float64))
    err = np.abs(out.cpu().double().numpy() - ref.out)
    print(f"{shape}: window samples: largest error / bound {float((err[win] / (27 * U * A[win])).max()):.3f}")
    assert (err[win] <= 27 * U * A[win]).all()
    # the measured correlation is reported whatever the shape; the two shapes differ where it matters
    assert abs(float(stats[0, 0, 1]) - ref.rho[0]) <= (2 * 23 + 4) * U
    other = O.splice(e, r, regions, W, M, shape="linear" if shape == "equal_power" else "equal_power", gain=g)
    assert np.abs(other.out - ref.out)[win].max() > 1e-3


@pytest.mark.parametrize("gain", [1.0, 0.75, 1.7])
def test_given_gain(dev, gain):
    """a forced gain (``splice_gain=None`` is 1.0): read back as given, used as one multiply, and the seams are searched under it"""
    n, regions, W, M = SMALL
    e, r, _ = planted("small")
    (out,), gains, starts, stats = launch([(e, r, regions, W, M)], dev, gain=gain)
    g = float(gains[0])
    assert g == float(np.float32(gain))
    ref = O.splice(e, r, regions, W, M, gain=g)
    assert starts[0].cpu().tolist() == ref.starts
    for k in range(2):
        assert abs(float(stats[0, k, 0]) - ref.cost[k]) <= O.gamma(W + 2) * ref.cost[k]
    check_bits(e, r, regions, W, M, out.cpu(), g, starts[0].cpu())


def test_batch_independence(dev):
    """a clip alone against the same clip in ragged batches, with shared and permuted references: every output, bit for bit"""
    names = ("small", "odd", "two")
    clips = [planted(k)[:2] + CASES[k][1:] for k in names]
    alone = [launch([c], dev) for c in clips]
    for order in ([0, 1, 2], [2, 0, 1]):
        batch = [clips[i] for i in order]
        outs, gains, starts, stats = launch(batch, dev)
        for row, i in enumerate(order):
            a_out, a_g, a_s, a_t = alone[i]
            assert torch.equal(outs[row], a_out[0]) and torch.equal(gains[row], a_g[0]) and torch.equal(starts[row], a_s[0]) \
                and torch.equal(stats[row], a_t[0]), (order, row)
    # the references stored in another order and shared: two candidates of one recording
    outs, gains, starts, stats = launch([clips[0], clips[2], clips[0]], dev, refs=[clips[2][1], clips[0][1]], ref_index=[1, 0, 1])
    for row, i in enumerate((0, 2, 0)):
        assert torch.equal(outs[row], alone[i][0][0]) and torch.equal(stats[row], alone[i][3][0])


def test_refusals(dev):
    e, r, _ = planted("small")
    clip = (e, r) + SMALL[1:]

    def set_(i, v):
        def f(ph):
            ph[0, i] = v
        return f

    bad = [(set_(1, 1), "W = 1"), (set_(4, 63), "M = 63 is below W = 64"), (set_(4, 8193), "M = 8193 exceeds 8192"),
           (set_(0, 5), r"5 regions \(10 seams\)"), (set_(0, 0), "no region"), (set_(13, 4161), "right seam span"),
           (set_(12, 2500), "right seam span"), (set_(10, 1900), "left seam span"), (set_(9, 4161), "region 0"),
           (set_(2, 3), "shape 3"), (set_(3, 1), "gain mode 1")]
    for mutate, msg in bad:
        with pytest.raises(RuntimeError, match=msg):
            launch([clip], dev, mutate=mutate)
        rc, out, gains, starts, stats = launch([clip], dev, mutate=mutate, raw=True)
        assert rc < 0 and bool(torch.isnan(out).all()) and bool(torch.isnan(gains).all()) and bool((starts == -7).all())
    from ap_adapter_amd import _lib, ops
    assert b"gain mode 1" in _lib.lib().apad_last_error()
    with pytest.raises(RuntimeError, match="its reference 0 has 4161"):
        launch([clip], dev, refs=[np.zeros(4161, np.float32)])
    with pytest.raises(RuntimeError, match=r"ref_index\[0\] = 1 outside \[0, 1\)"):
        launch([clip], dev, ref_index=[1])
    # null pointers, and out aliasing an input
    x = torch.zeros(4160, device=dev)
    oh, ih = torch.tensor([0, 4160]), torch.zeros(1, dtype=torch.int32)
    assert _lib.lib().apad_splice(x.data_ptr(), oh.to(dev).data_ptr(), oh.data_ptr(), x.data_ptr(), oh.to(dev).data_ptr(), oh.data_ptr(), None, None,
                                  None, None, None, None, None, None, None, 1, 1, None) < 0
    assert b"null pointer" in _lib.lib().apad_last_error()
    with pytest.raises(RuntimeError, match="expected a GPU tensor"):
        ops.splice(x.cpu(), *[None] * 13)
    rc, out, *_ = launch([clip], dev, raw=True)  # the same operands, valid
    assert rc == 0 and not torch.isnan(out).any()


def test_graph_capture(dev):
    """the launch recorded in a hipGraph and replayed twice on new contents of the same buffers equals eager, bit for bit"""
    from ap_adapter_amd import ops, splice
    names = ("small", "two")
    clips = [planted(k)[:2] + CASES[k][1:] for k in names]
    oh = torch.zeros(3, dtype=torch.int64)
    oh[1:] = torch.cumsum(torch.tensor([len(c[0]) for c in clips]), 0)
    od = oh.to(dev)
    first = torch.from_numpy(np.concatenate([c[0] for c in clips])).to(dev)
    second = torch.from_numpy(np.concatenate([O.planted(*CASES[k], seed=77)[0] for k in names])).to(dev)
    r = torch.from_numpy(np.concatenate([c[1] for c in clips])).to(dev)
    ph = torch.tensor([splice.plan_row(splice.plan(len(c[0]), *c[2:])) for c in clips], dtype=torch.int32)
    pd, ih = ph.to(dev), torch.tensor([0, 1], dtype=torch.int32)
    idd = ih.to(dev)
    e = first.clone()
    out, gains, stats = nan(e.numel(), dev=dev), nan(2, dev=dev), nan(2, 8, 2, dev=dev)
    starts = torch.full((2, 8), -7, dtype=torch.int32, device=dev)
    bufs = (out, gains, starts, stats)

    def run():
        ops.splice(e, od, oh, r, od, oh, idd, ih, pd, ph, out, gains, starts, stats)

    run()  # (loads the library outside the capture)
    out_first = out.clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        run()
    e.copy_(second)
    got = []
    for _ in range(2):
        for t in bufs:
            t.fill_(float("nan") if t.is_floating_point() else -7)
        g.replay()
        torch.cuda.synchronize()
        got.append([t.clone() for t in bufs])
    for t in bufs:
        t.fill_(float("nan") if t.is_floating_point() else -7)
    run()
    torch.cuda.synchronize()
    for rep in got:
        for a, b in zip(rep, bufs):
            assert not torch.isnan(a.float()).any() and torch.equal(a, b)
    assert not torch.equal(got[0][0], out_first)  # the replay read the buffers' new contents


def test_public_surface(dev):
    """splice_edit: a rectangular GPU tensor with one shared reference, a ragged list with per-clip regions, a single clip"""
    import ap_adapter_amd as A
    n, regions, W, M = SMALL
    e, r, want = planted("small")
    sec = lambda a, b: (a / 16000.0, b / 16000.0)
    kw = dict(crossfade_s=W / 16000.0, seam_search_s=M / 16000.0)
    nan_fill_free(dev)
    rect = torch.from_numpy(np.stack([e, 0.5 * e])).to(dev)
    out, gains, starts, stats, plans = A.splice_edit(rect, torch.from_numpy(r), sec(1920, 2560), return_plan=True, **kw)
    assert out.shape == rect.shape and out.is_cuda and gains.shape == (2,) and starts.shape == (2, 8) and stats.shape == (2, 8, 2)
    (alone,), g_alone, s_alone, _ = launch([(e, r, regions, W, M)], dev)
    assert torch.equal(out[0], alone) and torch.equal(gains[0], g_alone[0]) and starts[0].cpu().tolist() == want
    assert float(gains[1]) == 2.0 * float(gains[0]) and plans[0].regions == [(1920, 2560)]
    e2, r2, want2 = planted("two")
    outs, gains2 = A.splice_edit([e, e2], [r, r2], [[sec(1920, 2560)], [sec(*ab) for ab in CASES["two"][1]]], **kw)
    assert isinstance(outs, list) and [o.numel() for o in outs] == [n, 9000] and torch.equal(outs[0], alone)
    assert torch.equal(outs[1], launch([(e2, r2) + CASES["two"][1:]], dev)[0][0])
    one, g1 = A.splice_edit(torch.from_numpy(e), r, sec(1920, 2560), gain=None, crossfade_shape="linear", **kw)
    assert one.shape == (n,) and float(g1[0]) == 1.0


# ---- through the pipeline: the small synthetic UNet, VAE and vocoder of the chroma tests ----
@pytest.fixture(scope="module")
def small(dev):
    import test_gpu_chroma as C
    return C.build_small(dev)


REGION = (0.2, 0.36)  # latent rows 5 .. 8: samples [3200, 5760) of 10240
W_S, M_S = 480, 1280


def check_against_reference(out, plain, ref, pipe, what, scale=None, measured=True):
    """each returned clip: the reference's bits (times ``scale[b]``, one fp32 multiply) outside the reported windows and the region;
    ``last_splice`` against the oracle on the decoded edit"""
    gains, starts, stats = (t.cpu() for t in pipe.last_splice)
    B, n = out.shape
    per = B // ref.shape[0]
    assert tuple(gains.shape) == (B,) and tuple(starts.shape) == (B, 8) and tuple(stats.shape) == (B, 8, 2) and pipe.last_splice[1].is_cuda
    for b in range(B):
        e, r = plain[b].numpy(), ref[b // per].numpy()
        g = float(gains[b])
        res = O.splice(e, r, [(3200, 5760)], W_S, M_S, gain=g)
        # The decoded edit is whatever the synthetic decoders give: nothing plants a window, and two candidates may tie within the rounding of a
        # cost.  What holds of any fp32 search: the chosen start's fp64 cost is within twice the cost's rounding bound of the minimum; where the
        # oracle's runner-up is further away than that, the start is the oracle's.
        for k, c in enumerate(res.costs[:2]):
            lo = res.plan.seams[0][k][0]
            mine, two = c[int(starts[b, k]) - lo], np.partition(c, 1)[:2]
            bound = O.gamma(W_S + 2) * mine
            decided = two[1] - two[0] > 2 * O.gamma(W_S + 2) * two[1]
            print(f"{what}: clip {b}: seam {k}: minimum {two[0]:.7e}, runner-up {two[1]:.7e}, the device's window {mine:.7e}, rounding bound of a "
                  f"cost {bound:.2e}: {'decided' if decided else 'a tie within the bound'}")
            assert mine - two[0] <= 2 * bound, (what, b, k)
            assert not decided or int(starts[b, k]) == res.starts[k], (what, b, k)
        res = O.splice(e, r, [(3200, 5760)], W_S, M_S, gain=g, starts_in=starts[b].tolist())
        assert starts[b].tolist() == res.starts, (what, b)
        k_l = sum(-(-(hi - lo) // 1024) for lo, hi in res.plan.kept)
        g64 = O.splice(e, r, [(3200, 5760)], W_S, M_S).g
        print(f"{what}: clip {b}: g {g:.7f} (oracle {g64:.7f}), windows at {res.starts[:2]}, rho {stats[b, :2, 1].tolist()} (oracle {res.rho[:2]})")
        assert abs(g - g64) / g64 <= (k_l + 24) * U if measured else g == 1.0
        for k in range(2):
            assert abs(float(stats[b, k, 0]) - res.cost[k]) <= O.gamma(W_S + 2) * res.cost[k]
            assert abs(float(stats[b, k, 1]) - res.rho[k]) <= (2 * 23 + 4) * U
        keep = ~O.window_mask(res, W_S, n) & ~O.edit_mask(res, W_S, n)
        assert keep.sum() >= 1920 + 3200
        want = torch.from_numpy(r) if scale is None else scale[b] * torch.from_numpy(r)
        assert torch.equal(out[b][torch.from_numpy(keep)], want[torch.from_numpy(keep)]), (what, b)
        if scale is None:
            edit = torch.from_numpy(O.edit_mask(res, W_S, n))
            assert torch.equal(out[b][edit], (gains[b] * plain[b])[edit]), (what, b)


def test_pipeline_splices_into_the_reference(dev, small):
    import ap_adapter_amd as A
    import test_gpu_chroma as C
    pipe = A.AudioLDM2Pipeline(small.unet, vae=small.vae, vocoder=small.voc)
    kw = dict(source_latents=small.source, edit_region=REGION, **small.kw)
    gen = lambda: torch.Generator().manual_seed(C.SEED)
    ref = torch.from_numpy(np.stack([O.signal(C.LEN, seed=40 + i) for i in range(small.P)]))
    plain = pipe(generator=gen(), **kw).audios
    assert pipe.last_splice is None
    assert torch.equal(pipe(generator=gen(), splice=None, **kw).audios, plain) and pipe.last_splice is None
    nan_fill_free(dev)
    out = pipe(generator=gen(), splice="source", splice_reference=ref, **kw).audios
    assert out.shape == plain.shape and not out.is_cuda and pipe.last_loudness is None
    check_against_reference(out, plain, ref, pipe, "splice")
    # the loudness stage scales the spliced clip as a whole: the kept part is the reference times the one gain
    loud = pipe(generator=gen(), splice="source", splice_reference=ref, target_loudness=-23.0, peak_limit_db=None, **kw).audios
    gl = pipe.last_loudness[1].cpu()
    for b in range(out.shape[0]):
        assert torch.equal(loud[b], gl[b] * out[b])
    check_against_reference(loud, plain, ref, pipe, "splice + target_loudness", scale=gl)
    # one source for every candidate: a 1-D reference, num_waveforms_per_prompt = 3 per prompt
    one = dict(kw, source_latents=small.source[:1])
    plain1 = pipe(generator=gen(), **one).audios
    out1 = pipe(generator=gen(), splice="source", splice_reference=ref[0], crossfade_shape="linear", splice_gain=None, **one).audios
    assert out1.shape[0] == small.P * C.N and bool((pipe.last_splice[0] == 1.0).all())
    check_against_reference(out1, plain1, ref[:1], pipe, "one source", measured=False)
    assert isinstance(pipe(generator=gen(), splice="source", splice_reference=ref, **dict(kw, output_type="np")).audios, np.ndarray)
    # a per-clip mask; ranking sees the spliced candidates and returns them re-ordered
    ranked = pipe(generator=gen(), splice="source", splice_reference=ref, rank_by="chroma", **kw).audios
    assert sorted(map(tuple, ranked[:C.N].tolist())) == sorted(map(tuple, out[:C.N].tolist()))


def test_pipeline_source_audio_is_the_raw_recording(dev, small, tmp_path):
    """``source_audio=``: the reference is the file's channel 0 at the vocoder's rate -- the samples as recorded, not the level-normalised
    ones the encoder sees -- zero-padded to the clip; two candidates per file"""
    import wave
    import ap_adapter_amd as A
    import test_gpu_chroma as C
    from ap_adapter_amd import frontend as FE
    sr = 44100
    n = int(0.6 * sr)  # shorter than the 0.64 s clip: the tail of the reference is zeros
    left = 0.2 * O.signal(n, seed=60, sr=sr)
    stereo = np.stack([left, -0.5 * left], axis=1)
    path = tmp_path / "recording.wav"
    with wave.open(str(path), "wb") as w:
        w.setnchannels(2)
        w.setsampwidth(2)
        w.setframerate(sr)
        w.writeframes(np.clip(np.round(stereo * 32768.0), -32768, 32767).astype("<i2").tobytes())
    data, rate = FE.load_wav(str(path))
    rec = FE.resample(torch.from_numpy(data[:1]).to(dev), rate, 16000)[0].cpu()
    assert rate == sr and 9000 < rec.numel() < C.LEN and 0.05 < float(rec.abs().max()) < 0.5
    ref = torch.zeros(1, C.LEN)
    ref[0, :rec.numel()] = rec
    pipe = A.AudioLDM2Pipeline(small.unet, vae=small.vae, vocoder=small.voc)
    kw = dict(source_audio=str(path), edit_region=REGION, strength=0.75, **small.kw)
    gen = lambda: torch.Generator().manual_seed(C.SEED)
    plain = pipe(generator=gen(), **kw).audios
    out = pipe(generator=gen(), splice="source", **kw).audios
    check_against_reference(out, plain, ref, pipe, "source_audio")
    assert bool((out[:, C.LEN - 100:] == 0).all())  # past the file's end the kept part is the padding


def test_no_reach(dev, small, monkeypatch):
    """with ops.splice out of order, calls without splice= run as before"""
    import ap_adapter_amd as A
    import test_gpu_chroma as C
    from ap_adapter_amd import ops

    def broken(*a, **k):
        raise AssertionError("ops.splice reached without splice=")

    pipe = A.AudioLDM2Pipeline(small.unet, vae=small.vae, vocoder=small.voc)
    kw = dict(source_latents=small.source, edit_region=REGION, **small.kw)
    before = pipe(generator=torch.Generator().manual_seed(C.SEED), **kw).audios
    monkeypatch.setattr(ops, "splice", broken)
    assert torch.equal(pipe(generator=torch.Generator().manual_seed(C.SEED), **kw).audios, before)
    assert pipe(generator=torch.Generator().manual_seed(C.SEED), target_loudness=-23.0, **kw).audios.shape == before.shape
    with pytest.raises(AssertionError, match="reached"):
        pipe(generator=torch.Generator().manual_seed(C.SEED), splice="source", splice_reference=torch.zeros(C.LEN), **kw)
