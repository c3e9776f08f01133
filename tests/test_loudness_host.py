"""CPU: the host half of loudness -- the product's K-weighting design against the standard's 48 kHz table and against the oracle's own
constants, the oracle against the standard's calibration statement, the block-count rule, the powers the kernel scans with, the argument
checks of ``__call__`` and of the two public functions, and the ABI additions."""
import inspect
import math
import os
import re

import numpy as np
import pytest
import torch
from scipy.signal import sosfilt

import loudness_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_k_weighting_is_the_standards_table_at_48_khz():
    from ap_adapter_amd import loudness
    sos = loudness.k_weighting(48000)
    assert sos.dtype == np.float64 and sos.shape == (2, 6)
    table = {(0, 0): 1.53512485958697, (0, 1): -2.69169618940638, (0, 2): 1.19839281085285, (0, 4): -1.69065929318241,
             (0, 5): 0.73248077421585, (1, 4): -1.99004745483398, (1, 5): 0.99007225036621}
    for (i, j), v in table.items():
        assert abs(sos[i, j] - v) < 1e-12, (i, j, sos[i, j], v)
    assert sos[0, 3] == 1.0 and sos[1].tolist()[:4] == [1.0, -2.0, 1.0, 1.0]


@pytest.mark.parametrize("fs", [16000, 44100, 8000])
def test_k_weighting_matches_the_oracles_own_design(fs):
    from ap_adapter_amd import loudness
    err = float(np.abs(loudness.k_weighting(fs) - O.sos(fs)).max())
    print(f"{fs} Hz: max-abs difference of the two designs {err:.3e}")
    assert err < 1e-12


def test_oracle_reads_the_calibration_sine():
    """BS.1770: a 0 dBFS 997 Hz sine in one front channel reads -3.01 LKFS"""
    t = np.arange(48000 * 5) / 48000.0
    r = O.loudness(np.sin(2 * np.pi * 997 * t), 48000)
    print(f"997 Hz, 0 dBFS, 48 kHz: {r.L:.4f} LKFS")
    assert abs(r.L - (-3.01)) <= 0.01 and r.n_abs == r.n_rel == len(r.block_loudness) == 47


@pytest.mark.parametrize("n,blocks", [(6399, 0), (6400, 1), (7999, 1), (8000, 2), (1, 0), (163840, 99)])
def test_block_count_rule(n, blocks):
    from ap_adapter_amd import loudness
    assert loudness.block_count(n) == O.block_count(n) == blocks
    assert loudness.hop_block(16000) == (1600, 6400) and loudness.hop_block(48000) == (4800, 19200) and loudness.hop_block(44100) == (4410, 17640)
    if n <= 8000:
        r = O.loudness(O.signal(n))
        assert len(r.block_loudness) == blocks and len(r.hop_energy) == n // 1600
        if blocks == 0:
            assert r.L == -math.inf and (r.n_abs, r.n_rel) == (0, 0)


def test_oracle_gates_and_silence():
    r = O.loudness(np.zeros(20000))
    assert r.L == -math.inf and (r.n_abs, r.n_rel) == (0, 0) and len(r.block_loudness) == 9
    r = O.loudness(O.signal(51200))
    assert (len(r.block_loudness), r.n_abs, r.n_rel) == (29, 24, 15) and min(O.gate_margin(r)) >= 1.0
    # a gain of g moves the loudness by 20 log10 g
    assert abs(O.loudness(0.5 * O.signal(20000).astype(np.float64)).L - (O.loudness(O.signal(20000)).L + 20 * math.log10(0.5))) < 1e-9
    assert O.gain(-20.0, -14.0, 0.1, 0.0) == pytest.approx(10 ** 0.3) and O.gain(-20.0, -14.0, 0.8, 0.5) == 0.5 / 0.8
    assert O.gain(-math.inf, -14.0, 0.8, 0.5) == 1.0 and O.gain(-20.0, math.nan, 0.8, 0.5) == 1.0 and O.gain(-20.0, -14.0, 0.0, 0.5) == 1.0


@pytest.mark.parametrize("fs", [16000, 44100])
def test_transition_powers_carry_the_recursion(fs):
    """what the kernel's scan relies on: the state after 8 j samples of zero input is M^j times the state before them -- for the shelf in
    the transposed direct form II (scipy's own state) and for the high-pass's all-pole half in value and difference coordinates"""
    from ap_adapter_amd import loudness
    sos = loudness.k_weighting(fs)
    P = loudness.transition_powers(sos)
    assert P.shape == (2, 65, 2, 2) and np.array_equal(P[:, 0], np.stack([np.eye(2)] * 2))
    g = np.random.default_rng(0)
    for j in (1, 2, 7, 64):
        zi = g.standard_normal((1, 2))
        _, zf = sosfilt(sos[:1], np.zeros(8 * j), zi=zi)
        assert np.allclose(P[0, j] @ zi[0], zf[0], rtol=0, atol=1e-12)
        p = g.standard_normal(2)  # (y[n-1], y[n-2]); the powers act on (y[n-1], y[n-1] - y[n-2])
        y = list(p[::-1])
        for _ in range(8 * j):
            y.append(-sos[1, 4] * y[-1] - sos[1, 5] * y[-2])
        assert np.allclose(P[1, j] @ [p[0], p[0] - p[1]], [y[-1], y[-1] - y[-2]], rtol=0, atol=1e-9 * max(1.0, np.abs(P[1, j]).max()))


def _pipe(**parts):
    import ap_adapter_amd as A
    return A.AudioLDM2Pipeline(None, **parts)


def test_loudness_argument_resolution():
    pipe = _pipe()
    assert pipe.check_loudness_arguments(None, -1.0, None, False, 4) is None
    t, limit = pipe.check_loudness_arguments(-23.0, -1.0, None, False, 4)
    assert t == [-23.0] * 4 and limit == pytest.approx(10 ** (-1 / 20))
    assert pipe.check_loudness_arguments([-20, -21.5], 0.0, None, False, 2) == ([-20.0, -21.5], 1.0)
    assert pipe.check_loudness_arguments(torch.tensor([-20.0, -21.5]), None, None, False, 2) == ([-20.0, -21.5], 0.0)  # None: no guard
    assert pipe.check_loudness_arguments("source", -1.0, None, True, 6)[0] == "source"
    assert pipe.check_loudness_arguments("source", -1.0, torch.zeros(2, 100), False, 6)[0] == "source"
    assert pipe.check_loudness_arguments("source", -1.0, torch.zeros(100), True, 6)[0] == "source"


BAD_TARGETS = [float("nan"), float("inf"), -float("inf"), "loud", "", [-23.0, float("nan")], [-23.0], [-23.0] * 5, [], object()]


@pytest.mark.parametrize("bad", BAD_TARGETS, ids=["object()" if type(b) is object else repr(b)[:24] for b in BAD_TARGETS])  # (an object's repr holds its address: no stable id)
def test_target_loudness_refuses_anything_else(bad):
    with pytest.raises(ValueError, match="target_loudness"):
        _pipe().check_loudness_arguments(bad, -1.0, None, True, 4)


def test_loudness_argument_refusals():
    pipe = _pipe()
    for p in (0.5, 1e-9, float("nan"), float("inf"), "loud"):
        with pytest.raises(ValueError, match="peak_limit_db"):
            pipe.check_loudness_arguments(-23.0, p, None, False, 4)
    with pytest.raises(ValueError, match="needs one \\(source_audio="):
        pipe.check_loudness_arguments("source", -1.0, None, False, 4)
    with pytest.raises(ValueError, match="loudness_reference"):
        pipe.check_loudness_arguments(None, -1.0, torch.zeros(100), True, 4)
    with pytest.raises(ValueError, match="loudness_reference"):
        pipe.check_loudness_arguments(-23.0, -1.0, torch.zeros(100), True, 4)
    for ref in (torch.zeros(4, 2, 100), torch.zeros(3, 100), torch.zeros(2, 0), torch.zeros(0)):
        with pytest.raises(ValueError, match="loudness_reference"):
            pipe.check_loudness_arguments("source", -1.0, ref, True, 4)


def test_call_checks_loudness_before_any_device_work():
    """a pipeline without a UNet: the call fails on the argument, not on the missing model"""
    pipe = _pipe()
    e = dict(prompt_embeds=torch.zeros(2, 4, 8), negative_prompt_embeds=torch.zeros(2, 4, 8), generated_prompt_embeds=torch.zeros(2, 2, 8),
             negative_generated_prompt_embeds=torch.zeros(2, 2, 8), attention_mask=torch.ones(2, 4, dtype=torch.long),
             negative_attention_mask=torch.ones(2, 4, dtype=torch.long), output_type="latent", audio_length_in_s=0.64)
    with pytest.raises(ValueError, match="must be finite"):
        pipe(target_loudness=float("nan"), **e)
    with pytest.raises(ValueError, match="peak_limit_db=3.0"):
        pipe(target_loudness=-23.0, peak_limit_db=3.0, **e)
    with pytest.raises(ValueError, match="needs one \\(source_audio="):
        pipe(target_loudness="source", **e)
    with pytest.raises(ValueError, match="holds 3 values for 2 clips"):
        pipe(target_loudness=[-23.0, -23.0, -23.0], **e)
    with pytest.raises(ValueError, match="holds 2 values for 4 clips"):
        pipe(target_loudness=[-23.0, -23.0], num_waveforms_per_prompt=2, **e)
    with pytest.raises(ValueError, match="loudness_reference"):
        pipe(loudness_reference=torch.zeros(100), **e)
    sig = inspect.signature(type(pipe).__call__).parameters
    assert sig["target_loudness"].default is None and sig["peak_limit_db"].default == -1.0 and sig["loudness_reference"].default is None
    # (in front of rank_by: tests/test_chroma_host.py and tests/test_invert_host.py pin the names after them)
    assert list(sig)[-11:-8] == ["target_loudness", "peak_limit_db", "loudness_reference"] and list(sig)[-8] == "rank_by"
    assert pipe.last_loudness is None


def test_public_functions_check_their_arguments():
    """on the host, before any device work: none of these needs a GPU to fail"""
    import ap_adapter_amd as A
    from ap_adapter_amd import loudness
    assert A.integrated_loudness is loudness.integrated_loudness and A.normalize_loudness is loudness.normalize_loudness
    x = torch.zeros(2, 8000)
    for bad in (float("nan"), float("inf"), [-14.0], [-14.0, float("nan")], "source"):
        with pytest.raises(ValueError, match="loudness: target"):
            A.normalize_loudness(x, target=bad)
    with pytest.raises(ValueError, match="peak_limit_db"):
        A.normalize_loudness(x, peak_limit_db=0.1)
    with pytest.raises(ValueError, match="not both"):
        A.normalize_loudness(x, target=-14.0, reference=x)
    with pytest.raises(ValueError, match="3 references for 2 clips"):
        A.normalize_loudness(x, reference=torch.zeros(3, 100))
    for bad in (torch.zeros(2, 3, 100), torch.zeros(0), torch.zeros(2, 0), [], [np.zeros(0)], [np.zeros((2, 2))]):
        with pytest.raises(ValueError, match="loudness:"):
            A.integrated_loudness(bad)
        with pytest.raises(ValueError, match="loudness:"):
            A.normalize_loudness(bad)
    for sr in (0, 3999, 96000, float("nan")):
        with pytest.raises(ValueError, match="sampling_rate"):
            A.integrated_loudness(x, sampling_rate=sr)
        with pytest.raises(ValueError, match="sampling_rate"):
            loudness.k_weighting(sr)
    assert loudness.peak_limit(None) == 0.0 and loudness.peak_limit(0) == 1.0 and loudness.peak_limit(-20) == pytest.approx(0.1)
    assert loudness.default_ref_index(6, 2) == [0, 0, 0, 1, 1, 1]


def test_abi_additions():
    from ap_adapter_amd import _lib
    header = open(os.path.join(ROOT, "include", "apadapter_hip.h")).read()
    source = open(os.path.join(ROOT, "ap-adapter_amd", "csrc", "loudness.hip")).read()
    for name, nargs in (("apad_loudness", 11), ("apad_loudness_gain", 14)):
        decl = re.search(r"\bint %s\((.*?)\);" % name, header, re.S).group(1)
        defn = re.search(r'extern "C" int %s\((.*?)\) \{' % name, source, re.S).group(1)
        assert len(decl.split(",")) == len(defn.split(",")) == len(_lib.SYMBOLS[name][1]) == nargs
    assert "loudness.hip" in open(os.path.join(ROOT, "ap-adapter_amd", "csrc", "Makefile")).read()
    assert "#define APAD_ABI_VERSION 12\n" in header  # additive: the ABI version stays
    for word in ("printf", "assert("):  # the kernels print nothing and abort on nothing
        assert word not in source
