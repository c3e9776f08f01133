"""CPU: the host half of the alignment stage -- ``align.plan`` on hand cases (and against the oracle's own kept set), the plan row, every
ValueError of ``align_edit``, ``splice_edit_aligned`` and the pipeline's keywords before any device work, the ABI addition, and the fp64
oracle against closed forms."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

import align_oracle as O
import splice_oracle as SO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, W, M = 4160, 64, 192


def test_plan_hand_cases():
    from ap_adapter_amd import align, splice
    assert align.plan(N, [(0, N)], 16).kept == [(16, N - 16)]
    p = align.plan(N, splice.plan(N, [(1920, 2560)], W, M).kept, 100)
    assert p == align.Plan(N, 100, [(100, 1628), (2852, 4060)]) and p.kept == O.kept_set(N, [(1920, 2560)], W, M, 100)
    # an interval that vanishes is dropped; one sample is enough to keep one
    assert align.plan(N, [(0, 200), (1000, N)], 100).kept == [(1100, N - 100)]
    assert align.plan(N, [(0, 201), (1000, N)], 100).kept == [(100, 101), (1100, N - 100)]
    assert align.plan(N, [(0, 3)], 1).kept == [(1, 2)]
    for name, (n, regions, w, m, L, _) in CASES.items():
        assert align.plan(n, splice.plan(n, regions, w, m).kept, L).kept == O.kept_set(n, regions, w, m, L), name
    for L in (0, -1, 1025):
        with pytest.raises(ValueError, match="outside \\[1, 1024\\]"):
            align.plan(N, [(0, N)], L)
    with pytest.raises(ValueError, match="no kept sample is left 1024 samples away"):
        align.plan(2048, [(0, 2048)], 1024)
    with pytest.raises(ValueError, match="no kept sample"):
        align.plan(N, [], 16)
    for bad in ([(0, N + 1)], [(5, 5)], [(100, 200), (150, 300)], [(-1, 5)]):
        with pytest.raises(ValueError, match="empty, out of order or outside"):
            align.plan(N, bad, 1)
    with pytest.raises(ValueError, match="6 kept intervals, at most 5"):
        align.plan(N, [(k * 100, k * 100 + 50) for k in range(6)], 1)


CASES = {  # the shapes of tests/test_gpu_align.py
    "small": (6399, [(2560, 3840)], 64, 192, 16, 5),
    "neg_extreme": (6399, [(2560, 3840)], 64, 192, 16, -16),
    "at_start": (6400, [(0, 1280)], 64, 192, 100, 100),
    "straddle": (12000, [(3900, 4500), (8000, 8640)], 64, 192, 100, -37),
    "max_L": (20000, [(9000, 10000)], 64, 192, 1024, 777),
    "product": (163840, [(48000, 80000), (120000, 131072)], 480, 1280, 320, -123),
}


def test_plan_row_layout():
    from ap_adapter_amd import align
    p = align.Plan(N, 100, [(100, 1628), (2852, 4060)])
    assert align.plan_row(p) == [2, 100, 0, 0, 100, 1628, 2852, 4060] + [0] * 8
    assert align.plan_row(align.Plan(N, 7, [(k * 10 + 7, k * 10 + 9) for k in range(5)])) == [5, 7, 0, 0] + \
        [v for k in range(5) for v in (k * 10 + 7, k * 10 + 9)] + [0, 0]
    assert align.plan_row(None) == [0, 1, 1, 0] + [0] * 12 and len(align.plan_row(p)) == align.PLAN_INTS == 16
    header = open(os.path.join(ROOT, "include", "apadapter_hip.h")).read()
    for name, value in (("PLAN_INTS", align.PLAN_INTS), ("MAX_INTERVALS", align.MAX_INTERVALS), ("MAX_LAG", align.MAX_LAG), ("CHUNK", align.CHUNK)):
        assert f"#define APAD_ALIGN_{name} {value}\n" in header


def test_check_arguments():
    from ap_adapter_amd import align
    assert align.check_arguments(16000, None, "nonsense", "nonsense") is None
    assert align.check_arguments(16000, "kept", 0.02, 0.5) == (320, 0.5, None)
    assert align.check_arguments(16000, "kept", 0.064, -1) == (1024, -1.0, None)
    assert align.check_arguments(16000, 37) == (None, None, 37) and align.check_arguments(16000, np.int64(-5)) == (None, None, -5)
    for bad in ("source", True, 1.5, [3]):
        with pytest.raises(ValueError, match="align="):
            align.check_arguments(16000, bad)
    for bad in (0.0, 0.00001, 0.07, -0.02, float("nan"), "wide", None):
        with pytest.raises(ValueError, match="align_search_s"):
            align.check_arguments(16000, "kept", bad, 0.5)
    for bad in (1.5, -1.01, float("nan"), "high", None):
        with pytest.raises(ValueError, match="align_min_corr"):
            align.check_arguments(16000, "kept", 0.02, bad)
    with pytest.raises(ValueError, match="sampling_rate"):
        align.check_arguments(0, "kept")
    with pytest.raises(ValueError, match="below 2\\^24"):
        align.check_arguments(16000, 2 ** 24)


def test_align_edit_refusals():
    """each ValueError is raised before anything touches the GPU (there is none here)"""
    import ap_adapter_amd as A
    x, r = torch.zeros(2, 16000), torch.zeros(16000)
    with pytest.raises(ValueError, match="search_s"):
        A.align_edit(x, r, search_s=0.1)
    with pytest.raises(ValueError, match="min_corr"):
        A.align_edit(x, r, min_corr=2.0)
    with pytest.raises(ValueError, match="3 references for 2 clips"):
        A.align_edit(x, torch.zeros(3, 16000))
    with pytest.raises(ValueError, match="clip 0 has 16000 samples, its reference 0 has 15999"):
        A.align_edit(x, torch.zeros(15999))
    with pytest.raises(ValueError, match="edit"):
        A.align_edit(torch.zeros(0), r)
    with pytest.raises(ValueError, match="regions"):
        A.align_edit(x, r, regions="all")
    with pytest.raises(ValueError, match="no kept sample is left"):
        A.align_edit(x, r, regions=(0.01, 0.99))
    with pytest.raises(ValueError, match="no kept sample is left"):
        A.align_edit(torch.zeros(600), torch.zeros(600))  # shorter than twice the search width
    with pytest.raises(ValueError, match="splice_margins"):
        A.align_edit(x, r, splice_margins=(0.03, 0.08))
    with pytest.raises(ValueError, match="crossfade_s"):
        A.align_edit(x, r, regions=(0.4, 0.6), splice_margins=(0.0, 0.08))
    for bad in (1.5, "kept", [1], [1, 2, 3], True):
        with pytest.raises(ValueError, match="lag="):
            A.align_edit(x, r, lag=bad)
    with pytest.raises(ValueError, match="out of itself"):
        A.align_edit(x, r, lag=16000)
    sig = inspect.signature(A.align_edit).parameters
    assert [(k, v.default) for k, v in sig.items()][2:] == [("regions", None), ("sampling_rate", 16000), ("search_s", 0.02), ("min_corr", 0.5),
                                                            ("lag", None), ("splice_margins", None)]
    assert A.align.align_edit is A.align_edit


def test_splice_edit_aligned_refusals():
    import ap_adapter_amd as A
    x, r = torch.zeros(2, 16000), torch.zeros(16000)
    ok = dict(regions=(0.4, 0.6))
    with pytest.raises(ValueError, match="align='source'"):
        A.splice_edit_aligned(x, r, align="source", **ok)
    with pytest.raises(ValueError, match="align_search_s"):
        A.splice_edit_aligned(x, r, align_search_s=0.1, **ok)
    with pytest.raises(ValueError, match="align_min_corr"):
        A.splice_edit_aligned(x, r, align_min_corr=float("nan"), **ok)
    with pytest.raises(ValueError, match="crossfade_s"):
        A.splice_edit_aligned(x, r, crossfade_s=0.0, **ok)
    with pytest.raises(ValueError, match="out of itself"):
        A.splice_edit_aligned(x, r, align=-16000, **ok)
    with pytest.raises(ValueError, match="no kept sample is left"):  # the splice keeps 0.005 s at either end, the search width eats them
        A.splice_edit_aligned(x, r, regions=(0.085, 0.915), align_search_s=0.0025)
    sig = inspect.signature(A.splice_edit_aligned).parameters
    assert [sig[k].default for k in ("align", "align_search_s", "align_min_corr")] == ["kept", 0.02, 0.5]
    plain = inspect.signature(A.splice_edit).parameters
    assert list(sig)[:len(plain)] == list(plain) and all(sig[k].default == plain[k].default for k in plain)


def _pipe(**parts):
    import ap_adapter_amd as A
    return A.AudioLDM2Pipeline(None, **parts)


def _spl(pipe, mask=None):
    if mask is None:
        mask = torch.zeros(1, 1, 16, 16)
        mask[:, :, 5:8] = 1.0
    return pipe.check_splice_arguments("source", torch.zeros(10240), 0.03, 0.08, "matched", "kept", None, None, torch.zeros(1, 8, 16, 16), mask, "pt",
                                       4, 10240)


def test_pipeline_keyword_resolution_and_refusals():
    pipe = _pipe()
    spl = _spl(pipe)
    assert pipe.check_align_arguments(None, 0.02, 0.5, spl, 10240) is None
    assert pipe.check_align_arguments("kept", 0.02, 0.5, spl, 10240) == (320, 0.5, None)
    assert pipe.check_align_arguments(23, "unused", "unused", spl, 10240) == (None, None, 23)
    with pytest.raises(ValueError, match="without splice= it has no use"):
        pipe.check_align_arguments("kept", 0.02, 0.5, None, 10240)
    with pytest.raises(ValueError, match="align='both'"):
        pipe.check_align_arguments("both", 0.02, 0.5, spl, 10240)
    with pytest.raises(ValueError, match="align_search_s"):
        pipe.check_align_arguments("kept", 0.1, 0.5, spl, 10240)
    with pytest.raises(ValueError, match="align_min_corr"):
        pipe.check_align_arguments("kept", 0.02, 1.1, spl, 10240)
    with pytest.raises(ValueError, match="out of itself"):
        pipe.check_align_arguments(10240, 0.02, 0.5, spl, 10240)
    # a kept set that vanishes after shrinking: rows 1 .. 14 edited, 1280 samples of seam span each side: nothing is kept beyond 640 - 1280
    wide = torch.zeros(1, 1, 16, 16)
    wide[:, :, 3:13] = 1.0  # samples [1920, 8320): spans [640, 9600), kept [0, 640) and [9600, 10240): both vanish at L = 320
    assert _spl(pipe, wide) is not None
    with pytest.raises(ValueError, match="no kept sample is left 320 samples away"):
        pipe.check_align_arguments("kept", 0.02, 0.5, _spl(pipe, wide), 10240)
    assert pipe.check_align_arguments("kept", 0.01, 0.5, _spl(pipe, wide), 10240) == (160, 0.5, None)


def test_call_checks_align_before_any_device_work():
    """a pipeline without a UNet: the call fails on the argument, not on the missing model"""
    import types
    pipe = _pipe(vae=object(), vocoder=types.SimpleNamespace(config=types.SimpleNamespace(sampling_rate=16000)))  # (never run)
    e = dict(prompt_embeds=torch.zeros(2, 4, 8), negative_prompt_embeds=torch.zeros(2, 4, 8), generated_prompt_embeds=torch.zeros(2, 2, 8),
             negative_generated_prompt_embeds=torch.zeros(2, 2, 8), attention_mask=torch.ones(2, 4, dtype=torch.long),
             negative_attention_mask=torch.ones(2, 4, dtype=torch.long), output_type="latent", audio_length_in_s=0.64)
    with pytest.raises(ValueError, match="align= shifts the edit ahead of splice='source'"):
        pipe(align="kept", **e)
    with pytest.raises(ValueError, match="align= shifts the edit ahead of splice='source'"):
        pipe(align=3, **e)
    sig = inspect.signature(type(pipe).__call__).parameters
    assert [sig[k].default for k in ("align", "align_search_s", "align_min_corr")] == [None, 0.02, 0.5]
    assert pipe.last_align is None
    doc = type(pipe).__call__.__doc__
    assert "last_align" in doc and "fractional lags" in doc and "No global time alignment" not in doc


def test_abi_addition():
    from ap_adapter_amd import _lib
    header = open(os.path.join(ROOT, "include", "apadapter_hip.h")).read()
    source = open(os.path.join(ROOT, "ap-adapter_amd", "csrc", "align.hip")).read()
    for name, arity in (("apad_align_corr", 16), ("apad_align_apply", 22)):
        decl = re.search(r"\bint %s\((.*?)\);" % name, header, re.S).group(1)
        defn = re.search(r'extern "C" int %s\((.*?)\) \{' % name, source, re.S).group(1)
        assert len(decl.split(",")) == len(defn.split(",")) == len(_lib.SYMBOLS[name][1]) == arity
        assert [" ".join(a.split()) for a in decl.split(",")] == [" ".join(a.split()) for a in defn.split(",")]  # the same parameters, by name
    assert "align.hip" in open(os.path.join(ROOT, "ap-adapter_amd", "csrc", "Makefile")).read()
    assert "#define APAD_ABI_VERSION 12\n" in header  # additive: the ABI version stays
    import ctypes
    h = ctypes.CDLL(_lib.LIB_PATH)  # the built library exports the symbols (an AttributeError otherwise) and still reports version 12
    assert h.apad_align_corr is not None and h.apad_align_apply is not None and h.apad_abi_version() == 12 and _lib.lib().apad_abi_version() == 12


def test_oracle_closed_forms():
    n, L = 3000, 32
    x = SO.signal(n + 2 * L, seed=4)
    r = x[L:L + n]
    kept = [(L, 1000), (1500, n - L)]
    for lag in (0, 1, -7, L, -L):
        e = x[L - lag:L - lag + n]  # e[i + lag] = r[i], exactly
        res = O.align(e, r, kept, L)
        assert (res.found, res.applied) == (lag, lag) and abs(res.ncc - 1.0) <= 1e-12 and (res.ncc0 < 1.0 - 1e-4 or lag == 0)
        assert np.array_equal(res.out.view(np.uint32), O.shift(e, lag).view(np.uint32))
        assert abs(res.c[lag + L] - res.er) <= 1e-12 * res.er
    # the shift: the same bits, +0.0 at the uncovered edge (also for a NaN and a -0.0 inside)
    e = np.arange(1, 9, dtype=np.float32)
    e[3], e[4] = np.nan, -0.0
    assert O.shift(e, 2).view(np.uint32).tolist() == e[2:].view(np.uint32).tolist() + [0, 0]
    assert O.shift(e, -3).view(np.uint32).tolist() == [0, 0, 0] + e[:5].view(np.uint32).tolist()
    assert O.shift(e, -7).tolist()[:7] == [0.0] * 7 and O.shift(e, 0).view(np.uint32).tolist() == e.view(np.uint32).tolist()
    # the gate: anti-correlated (c <= 0 everywhere but the found lag is reported), and a floor above the measured ncc
    pos = (np.abs(r) + 1.0).astype(np.float32)
    neg = O.align(-pos, pos, kept, L, min_corr=-1.0)
    assert neg.c.max() < 0 and neg.applied == 0 and neg.ncc < 0
    half = O.align((0.5 * r + 0.5 * SO.signal(n, seed=9)).astype(np.float32), r, kept, L, min_corr=0.99)
    assert half.found == 0 and 0.3 < half.ncc < 0.99 and half.applied == 0
    assert O.align(np.zeros(n, np.float32), r, kept, L).ncc == 0.0  # an energy of 0


def test_oracle_tie_order():
    """a signal of period 8 ties at every lag = planted + 8 m: the smaller |l| wins, then l >= 0 -- exactly, on integers"""
    n, L = 2000, 16
    kept = [(L, n - L)]
    for lag, ties in ((3, [-13, -5, 3, 11]), (4, [-12, -4, 4, 12]), (-3, [-11, -3, 5, 13]), (0, [-16, -8, 0, 8, 16]), (-4, [-12, -4, 4, 12])):
        e, r = O.periodic(n, L, lag)
        res = O.align(e, r, kept, L, integer=True)
        assert np.flatnonzero(res.c == res.c.max()).tolist() == [t + L for t in ties]
        want = min(ties, key=lambda l: (abs(l), l < 0))
        assert res.found == want == (4 if abs(lag) == 4 else lag), (lag, res.found)
    # the order is total: the winner does not depend on where the search starts or which way it runs
    e, r = O.periodic(n, L, 4)
    c, _ = O.table(e, r, kept, L, np.int64)
    assert O.winner(c, L) == 4 and -O.winner(c[::-1].copy(), L) == -4


def test_planted_lags_are_found_by_the_oracle():
    for name in ("small", "neg_extreme", "at_start", "straddle"):
        n, regions, w, m, L, lag = CASES[name]
        for integer in (False, True):
            e, r, kept = O.planted(n, regions, w, m, L, lag, seed=len(name), integer=integer)
            res = O.align(e, r, kept, L, integer=integer)
            assert (res.found, res.applied) == (lag, lag), (name, integer)
            assert res.ncc > 0.98 and res.ncc0 < 0.9
