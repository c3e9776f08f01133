"""CPU: the host half of the splice stage -- ``splice.plan`` on hand cases (and against the oracle's own plan), every ValueError of
``splice_edit`` and of the pipeline's keywords, mask -> regions, the ABI addition, and the fp64 oracle against closed forms."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

import splice_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, W, M = 4160, 64, 192


def both_plans(n, regions, w=W, m=M):
    from ap_adapter_amd import splice
    p, o = splice.plan(n, regions, w, m), O.plan(n, regions, w, m)
    assert p.regions == o.regions and [tuple(s) for s in p.seams] == o.seams and p.kept == o.kept
    return p


def test_plan_hand_cases():
    p = both_plans(N, [(1920, 2560)])
    assert p.regions == [(1920, 2560)] and p.seams == [((1728, 1920), (2560, 2752))] and p.kept == [(0, 1728), (2752, 4160)]
    # a region at the clip's start: no left seam, the edit runs from sample 0
    p = both_plans(N, [(0, 640)])
    assert p.seams == [(None, (640, 832))] and p.kept == [(832, 4160)]
    # a < W: no room for a left window either; a == W: exactly one candidate
    assert both_plans(N, [(63, 640)]).seams[0][0] is None
    assert both_plans(N, [(64, 640)]).seams[0][0] == (0, 64)
    # fewer than W samples to the end: the edit runs to the edge
    p = both_plans(N, [(3000, N - 63)])
    assert p.seams == [((2808, 3000), None)] and p.kept == [(0, 2808)]
    assert both_plans(N, [(3000, N - 64)]).seams[0][1] == (N - 64, N)
    # the search span is cut at the clip's edges
    assert both_plans(N, [(100, 2000)], 32, 192).seams == [((0, 100), (2000, 2192))]
    assert both_plans(N, [(2000, 4100)], 32, 192).seams == [((1808, 2000), (4100, 4160))]
    # unsorted and overlapping input
    assert both_plans(N, [(2000, 2100), (1000, 1100), (1050, 1200)], 16, 32).regions == [(1000, 1200), (2000, 2100)]


def test_plan_merges_below_twice_the_margin():
    n = 20000
    assert both_plans(n, [(1000, 2000), (2000 + 2 * M - 1, 4000)]).regions == [(1000, 4000)]
    p = both_plans(n, [(1000, 2000), (2000 + 2 * M, 4000)])
    assert p.regions == [(1000, 2000), (2384, 4000)]
    assert p.seams[0][1] == (2000, 2192) and p.seams[1][0] == (2192, 2384)  # the two spans touch, nothing is kept between them
    assert p.kept == [(0, 808), (4192, n)]


def test_plan_refusals():
    from ap_adapter_amd import splice
    four = [(2000 * k + 500, 2000 * k + 900) for k in range(4)]
    assert len(both_plans(20000, four).regions) == 4
    for fn in (splice.plan, O.plan):
        with pytest.raises(ValueError, match="4 regions"):
            fn(20000, four + [(8500, 8900)], W, M)
        with pytest.raises(ValueError, match="no region"):
            fn(N, [], W, M)
        with pytest.raises(ValueError, match="no kept sample"):
            fn(N, [(100, 4100)], W, M)
        with pytest.raises(ValueError):
            fn(N, [(100, 4161)], W, M)
        with pytest.raises(ValueError):
            fn(N, [(200, 200)], W, M)
        for w, m in ((1, 192), (64, 63), (64, 8193)):
            with pytest.raises(ValueError):
                fn(20000, [(9000, 9500)], w, m)
    assert splice.plan(200000, [(90000, 95000)], 480, 8192).seams == [((81808, 90000), (95000, 103192))]


def test_plan_row_layout():
    from ap_adapter_amd import splice
    row = splice.plan_row(splice.plan(N, [(0, 640), (2000, 2100)], 16, 32), shape=2, given_gain=True)
    assert len(row) == splice.PLAN_INTS == 32
    assert row[:8] == [2, 16, 2, 1, 32, 0, 0, 0]
    assert row[8:14] == [0, 640, -1, -1, 640, 672] and row[14:20] == [2000, 2100, 1968, 2000, 2100, 2132] and row[20:] == [0] * 12


def test_splice_edit_refusals():
    """on the host, before any device work: none of these needs a GPU to fail"""
    import ap_adapter_amd as A
    from ap_adapter_amd import splice
    assert A.splice_edit is splice.splice_edit
    x, r = torch.zeros(2, 16000), torch.zeros(16000)
    ok = dict(regions=(0.3, 0.6))
    for bad in ("cosine", None, 1):
        with pytest.raises(ValueError, match="crossfade_shape"):
            A.splice_edit(x, r, crossfade_shape=bad, **ok)
    for bad in ("source", 0.0, -1.0, float("nan"), float("inf"), object()):
        with pytest.raises(ValueError, match="gain"):
            A.splice_edit(x, r, gain=bad, **ok)
    for bad in (0.0, -1.0, 0.00005, float("nan"), "long"):
        with pytest.raises(ValueError, match="crossfade_s"):
            A.splice_edit(x, r, crossfade_s=bad, **ok)
    with pytest.raises(ValueError, match="seam_search_s"):
        A.splice_edit(x, r, crossfade_s=0.03, seam_search_s=0.02, **ok)
    with pytest.raises(ValueError, match="seam_search_s=0.6 is 9600 samples"):
        A.splice_edit(x, r, seam_search_s=0.6, **ok)
    with pytest.raises(ValueError, match="sampling_rate"):
        A.splice_edit(x, r, sampling_rate=0, **ok)
    for bad in (None, [], "all", (0.5, 0.2), (-0.1, 0.2), (0.1, float("nan")), [(0.1, 0.2, 0.3)], [[(0.1, 0.2)]] * 3):
        with pytest.raises(ValueError, match="regions"):
            A.splice_edit(x, r, regions=bad)
    with pytest.raises(ValueError, match="3 references for 2 clips"):
        A.splice_edit(x, torch.zeros(3, 16000), **ok)
    with pytest.raises(ValueError, match="clip 0 has 16000 samples, its reference 0 has 15999"):
        A.splice_edit(x, torch.zeros(15999), **ok)
    for bad in (torch.zeros(2, 3, 100), torch.zeros(0), []):
        with pytest.raises(ValueError, match="edit"):
            A.splice_edit(bad, r, **ok)
    with pytest.raises(ValueError, match="reference"):
        A.splice_edit(x, torch.zeros(2, 0), **ok)
    with pytest.raises(ValueError, match="no kept sample"):
        A.splice_edit(x, r, regions=(0.05, 0.95))
    with pytest.raises(ValueError, match="no region"):
        A.splice_edit(x, r, regions=(1.5, 1.6))  # past the clip's end
    with pytest.raises(ValueError, match="5 regions"):
        A.splice_edit(torch.zeros(160000), torch.zeros(160000), regions=[(k + 0.2, k + 0.5) for k in range(5)])
    sig = inspect.signature(A.splice_edit).parameters
    assert [(k, v.default) for k, v in sig.items()][2:] == [("regions", inspect.Parameter.empty), ("sampling_rate", 16000), ("crossfade_s", 0.03),
                                                            ("seam_search_s", 0.08), ("crossfade_shape", "matched"), ("gain", "kept"),
                                                            ("return_plan", False)]


def test_mask_regions():
    from ap_adapter_amd import splice
    m = torch.zeros(16, 16)
    m[3:5] = 1.0
    assert splice.mask_regions(m, 640, 10240) == [(1920, 3200)]
    # a frequency-band mask counts as its rows; a fractional entry counts; the last run is cut at the clip's end
    m = torch.zeros(16, 16)
    m[3:5, 2:4], m[9, 15], m[15, 0] = 1.0, 0.25, 1.0
    assert splice.mask_regions(m, 640, 10000) == [(1920, 3200), (5760, 6400), (9600, 10000)]
    assert splice.mask_regions(torch.zeros(16, 16), 640, 10240) == []
    per_clip = torch.zeros(2, 1, 16, 16)
    per_clip[0, 0, 0], per_clip[1, 0, 4:6] = 1.0, 1.0
    assert splice.mask_regions(per_clip, 640, 10240) == [[(0, 640)], [(2560, 3840)]]


def _pipe(**parts):
    import ap_adapter_amd as A
    return A.AudioLDM2Pipeline(None, **parts)


def _check(pipe, **over):
    mask = torch.zeros(1, 1, 16, 16)
    mask[:, :, 5:8] = 1.0
    kw = dict(splice="source", splice_reference=torch.zeros(10240), crossfade_s=0.03, seam_search_s=0.08, crossfade_shape="matched",
              splice_gain="kept", source_audio=None, source_mel=None, source_latents=torch.zeros(1, 8, 16, 16), mask=mask, output_type="pt",
              batch=4, samples=10240)
    kw.update(over)
    return pipe.check_splice_arguments(**kw)


def test_pipeline_keyword_resolution_and_refusals():
    pipe = _pipe()
    assert _check(pipe, splice=None, splice_reference=None) is None
    regions, w, m, shape, gain = _check(pipe)
    assert regions == [[(3200, 5120)]] * 4 and (w, m, shape, gain) == (480, 1280, 0, None)
    assert _check(pipe, splice_gain=None, crossfade_shape="linear")[3:] == (1, 1.0)
    assert _check(pipe, splice_gain=0.5, crossfade_shape="equal_power", splice_reference=torch.zeros(2, 10240))[3:] == (2, 0.5)
    assert _check(pipe, source_latents=None, source_audio="a.wav", splice_reference=None)[0] == [[(3200, 5120)]] * 4
    per_clip = torch.zeros(4, 1, 16, 16)
    for b in range(4):
        per_clip[b, 0, 4 + b] = 1.0
    assert _check(pipe, mask=per_clip)[0] == [[(640 * (4 + b), 640 * (5 + b))] for b in range(4)]
    with pytest.raises(ValueError, match="splice='other'"):
        _check(pipe, splice="other")
    with pytest.raises(ValueError, match="needs a source clip"):
        _check(pipe, source_latents=None)
    with pytest.raises(ValueError, match="needs a region"):
        _check(pipe, mask=None)
    with pytest.raises(ValueError, match="output_type='latent'"):
        _check(pipe, output_type="latent")
    with pytest.raises(ValueError, match="needs the recording itself: splice_reference="):
        _check(pipe, splice_reference=None)
    with pytest.raises(ValueError, match="splice_reference and source_audio are both given"):
        _check(pipe, source_latents=None, source_audio="a.wav")
    with pytest.raises(ValueError, match="splice_reference .* has no use"):
        _check(pipe, splice=None)
    for ref in (torch.zeros(3, 10240), torch.zeros(2, 2, 100), torch.zeros(0)):
        with pytest.raises(ValueError, match="splice_reference"):
            _check(pipe, splice_reference=ref)
    with pytest.raises(ValueError, match="crossfade_s"):
        _check(pipe, crossfade_s=0.0)
    with pytest.raises(ValueError, match="seam_search_s"):
        _check(pipe, seam_search_s=0.01)
    with pytest.raises(ValueError, match="seam_search_s"):
        _check(pipe, seam_search_s=1.0)
    with pytest.raises(ValueError, match="crossfade_shape"):
        _check(pipe, crossfade_shape="cosine")
    with pytest.raises(ValueError, match="splice_gain"):
        _check(pipe, splice_gain="source")
    with pytest.raises(ValueError, match="no region"):
        _check(pipe, mask=torch.zeros(1, 1, 16, 16))
    with pytest.raises(ValueError, match="no kept sample"):
        _check(pipe, mask=torch.ones(1, 1, 16, 16))


def test_call_checks_splice_before_any_device_work():
    """a pipeline without a UNet: the call fails on the argument, not on the missing model"""
    pipe = _pipe()
    e = dict(prompt_embeds=torch.zeros(2, 4, 8), negative_prompt_embeds=torch.zeros(2, 4, 8), generated_prompt_embeds=torch.zeros(2, 2, 8),
             negative_generated_prompt_embeds=torch.zeros(2, 2, 8), attention_mask=torch.ones(2, 4, dtype=torch.long),
             negative_attention_mask=torch.ones(2, 4, dtype=torch.long), output_type="latent", audio_length_in_s=0.64)
    with pytest.raises(ValueError, match="needs a source clip"):
        pipe(splice="source", **e)
    with pytest.raises(ValueError, match="splice='both'"):
        pipe(splice="both", **e)
    with pytest.raises(ValueError, match="splice_reference .* has no use"):
        pipe(splice_reference=torch.zeros(100), **e)
    sig = inspect.signature(type(pipe).__call__).parameters
    names = ["splice", "splice_reference", "crossfade_s", "seam_search_s", "crossfade_shape", "splice_gain"]
    assert [sig[k].default for k in names] == [None, None, 0.03, 0.08, "matched", "kept"]
    assert pipe.last_splice is None
    assert "frequency-band" in type(pipe).__call__.__doc__  # the docstring states how such a mask is read


def test_abi_addition():
    from ap_adapter_amd import _lib
    header = open(os.path.join(ROOT, "include", "apadapter_hip.h")).read()
    source = open(os.path.join(ROOT, "ap-adapter_amd", "csrc", "splice.hip")).read()
    decl = re.search(r"\bint apad_splice\((.*?)\);", header, re.S).group(1)
    defn = re.search(r'extern "C" int apad_splice\((.*?)\) \{', source, re.S).group(1)
    assert len(decl.split(",")) == len(defn.split(",")) == len(_lib.SYMBOLS["apad_splice"][1]) == 18
    assert [" ".join(a.split()) for a in decl.split(",")] == [" ".join(a.split()) for a in defn.split(",")]  # the same parameters, by name
    assert "splice.hip" in open(os.path.join(ROOT, "ap-adapter_amd", "csrc", "Makefile")).read()
    assert "#define APAD_ABI_VERSION 12\n" in header  # additive: the ABI version stays
    for word in ("printf", "assert(", "atomicAdd", "_atomic"):  # the kernel prints nothing, aborts on nothing and has no atomics
        assert word not in source
    import ctypes
    h = ctypes.CDLL(_lib.LIB_PATH)  # the built library exports the symbol (an AttributeError otherwise) and still reports version 12
    assert h.apad_splice is not None and h.apad_abi_version() == 12 and _lib.lib().apad_abi_version() == 12


def test_oracle_closed_forms():
    r = O.signal(N, seed=3)
    half = (0.5 * r.astype(np.float64)).astype(np.float32)  # exact halves
    res = O.splice(half, r, [(1920, 2560)], W, M)
    assert res.g == 2.0 and max(res.cost) == 0.0
    assert np.array_equal(res.out[~O.window_mask(res, W, N)], r.astype(np.float64)[~O.window_mask(res, W, N)])
    same = O.splice(r, r, [(1920, 2560)], W, M)
    assert same.g == 1.0 and same.starts[:2] == [1920 - W, 2560] and same.rho[:2] == [1.0, 1.0] and same.starts[2:] == [-1] * 6
    assert np.abs(same.out - r).max() <= 4 * 2.0 ** -53 * np.abs(r).max()
    # sine against cosine over whole periods: orthogonal, rho = 0 up to fp32's rounding of the samples
    n, w = 8000, 800
    t = np.arange(n)
    s, c = np.sin(2 * np.pi * t / 100).astype(np.float32), np.cos(2 * np.pi * t / 100).astype(np.float32)
    oc = O.splice(c, s, [(4000, 4400)], w, w, gain=None)
    print(f"sine against cosine over 8 periods: rho = {oc.rho[:2]}")
    assert oc.starts[:2] == [3200, 4400] and max(oc.rho) < 1e-6
    # with rho = 0 the crossfade is the equal-power one; with e = r and rho = 1 it is the identity, with rho = 0 it lifts the middle by sqrt 2
    eq = O.splice(r, r, [(1920, 2560)], W, M, shape="equal_power")
    mid = 1920 - W + W // 2
    assert abs(eq.out[mid] / r[mid] - 1 / np.sqrt(2 * 0.5 ** 2 + 2 * (0.5 / W) ** 2)) < 1e-12
    # the gain is measured on the kept set alone: what happens inside the spans does not move it
    e2 = half.copy()
    e2[1728:2752] = 0.3
    assert O.splice(e2, r, [(1920, 2560)], W, M).g == 2.0
    assert O.splice(e2, r, [(1920, 2560)], W, M, gain=None).g == 1.0 and O.splice(e2, r, [(1920, 2560)], W, M, gain=1.25).g == 1.25
    assert O.splice(np.zeros(N, np.float32), r, [(1920, 2560)], W, M).g == 1.0


def test_planted_windows_are_found_by_the_oracle():
    e, r, want = O.planted(N, [(1920, 2560)], W, M)
    res = O.splice(e, r, [(1920, 2560)], W, M)
    assert res.starts == want and abs(res.g - 1.7) < 1e-6
