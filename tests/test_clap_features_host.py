"""CPU: ap_adapter_amd.ClapFeatureExtractor against the installed transformers class -- constructor, attributes, mel filters, the
index map ``apad_clap_logmel`` implements (against np.tile / np.pad / slicing), the crop starts under a seeded numpy, the ABI and
what raises."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

import clap_feature_models as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ML = 4800
N48 = (300, 1000, 2400, 4799, 4800, 4801, 6000)


def _params(cls):
    return [(n, p.default) for n, p in inspect.signature(cls.__init__).parameters.items()
            if n != "self" and p.kind is not inspect.Parameter.VAR_KEYWORD]


def test_constructor_names_and_defaults_are_the_installed_ones():
    import ap_adapter_amd as A
    assert _params(A.ClapFeatureExtractor) == _params(type(F.installed()))
    mine = list(inspect.signature(A.ClapFeatureExtractor.__call__).parameters)
    theirs = [n for n in inspect.signature(type(F.installed()).__call__).parameters if n != "kwargs"]
    assert mine == theirs + ["source_sampling_rate", "crop_starts"]


@pytest.mark.parametrize("kw", [dict(), dict(feature_size=16, max_length_s=2.5)], ids=["default", "small"])
def test_attributes_and_mel_filters(kw):
    import ap_adapter_amd as A
    a, b = A.ClapFeatureExtractor(**kw), type(F.installed())(**kw)
    assert a.model_input_names == b.model_input_names
    for name, v in b.__dict__.items():
        w = getattr(a, name)
        if isinstance(v, np.ndarray):
            assert w.shape == v.shape
            err = float(np.abs(w - v).max())
            print(f"{name} {v.shape}: max abs diff {err:.2e}")
            assert err <= 1e-7
        else:
            assert w == v and type(w) is type(v), name
    assert a.top_db is None  # stored, unused


def _installed_padded(w, padding, start):
    """the samples the installed extractor frames, np.pad(mode="reflect") included: _get_input_mel's own lines + spectrogram's pad"""
    if len(w) > ML:
        w = w[start:start + ML]
    elif len(w) < ML:
        if padding == "repeat":
            w = np.tile(w, int(ML / len(w)) + 1)[:ML]
        if padding == "repeatpad":
            w = np.tile(w, int(ML / len(w)))
        w = np.pad(w, (0, ML - w.shape[0]), mode="constant", constant_values=0)
    return np.pad(w, (512, 512), mode="reflect")


@pytest.mark.parametrize("n48", N48)
@pytest.mark.parametrize("padding", ["repeatpad", "repeat", "pad"])
def test_index_map_vs_numpy(n48, padding):
    """ramp waveforms w[i] = i + 1 (0 means padding): reflect_index then source_index reproduce the installed path's padded signal"""
    from ap_adapter_amd.clap_features import reflect_index, source_index
    w = np.arange(1, n48 + 1, dtype=np.float64)
    for start in (sorted({0, min(7, n48 - ML), n48 - ML}) if n48 > ML else (0,)):  # 0, 7 where it is a valid start, overflow
        ref = _installed_padded(w, padding, start)
        assert ref.shape == (ML + 1024,)
        mine = np.zeros_like(ref)
        for k in range(ML + 1024):
            q = source_index(reflect_index(k - 512, ML), n48, ML, padding, start)
            mine[k] = 0.0 if q is None else w[q]
        assert np.array_equal(mine, ref), (n48, padding, start)


def test_installed_path_is_what_the_helper_restates(monkeypatch):
    """_installed_padded above against the installed class itself: the waveform it hands to _np_extract_fbank_features"""
    fe = F.installed()
    seen = []
    monkeypatch.setattr(type(fe), "_np_extract_fbank_features", lambda self, waveform, mel_filters=None: seen.append(waveform.copy()) or np.zeros((11, 64)))
    for n48 in N48:
        for padding in ("repeatpad", "repeat", "pad"):
            w = np.arange(1, n48 + 1, dtype=np.float64)
            seen.clear()
            np.random.seed(n48)
            fe([w], padding=padding, max_length=ML, sampling_rate=48000)
            np.random.seed(n48)
            start = np.random.randint(0, n48 - ML + 1) if n48 > ML else 0
            assert np.array_equal(np.pad(seen[0], (512, 512), mode="reflect"), _installed_padded(w, padding, start))


class _Recorded(Exception):
    pass


@pytest.mark.parametrize("seed", [0, 1, 12345])
def test_crop_starts_under_a_seeded_numpy_are_the_installed_ones(monkeypatch, seed):
    """two long clips and a short one: the installed extractor's crops (recovered from the waveform it frames) and ours (the
    ``starts`` operand of the launch) under the same numpy seed"""
    import ap_adapter_amd as A
    from ap_adapter_amd import clap_features as CF
    clips = [np.arange(1, 9001, dtype=np.float32), np.arange(1, 1001, dtype=np.float32), np.arange(1, 6001, dtype=np.float32)]
    fe = F.installed()
    seen = []
    monkeypatch.setattr(type(fe), "_np_extract_fbank_features", lambda self, waveform, mel_filters=None: seen.append(waveform.copy()) or np.zeros((11, 64)))
    np.random.seed(seed)
    longer = fe(clips, max_length=ML, sampling_rate=48000)["is_longer"]
    theirs = [int(seen[0][0]) - 1, 0, int(seen[2][0]) - 1]
    got = {}

    def record(packed, offsets, offsets_host, starts, starts_host, *rest):
        got["starts"] = starts_host.tolist()
        raise _Recorded

    monkeypatch.setattr(CF, "clap_logmel_launch", record)
    monkeypatch.setattr(CF.ClapFeatureExtractor, "_clips", staticmethod(lambda raw: ([torch.as_tensor(c) for c in raw], torch.device("cpu"))))
    monkeypatch.setattr(CF.ClapFeatureExtractor, "tables", lambda self, dev: None)
    np.random.seed(seed)
    with pytest.raises(_Recorded):
        A.ClapFeatureExtractor(truncation="rand_trunc")(clips, max_length=ML, sampling_rate=48000)
    assert got["starts"] == theirs and longer == [[True], [False], [True]]
    assert theirs[0] <= 9000 - ML and theirs[2] <= 6000 - ML


def test_abi_declares_the_entry_point_additively():
    from ap_adapter_amd import _lib
    header = open(os.path.join(ROOT, "include", "apadapter_hip.h")).read()
    assert re.search(r"#define APAD_ABI_VERSION 12\b", header)  # additive: the version line stays
    assert re.search(r"\bint apad_clap_logmel\(", header) and "apad_clap_logmel" in _lib.SYMBOLS
    decl = re.search(r"\bint apad_clap_logmel\((.*?)\);", header, re.S).group(1)
    assert len(decl.split(",")) == len(_lib.SYMBOLS["apad_clap_logmel"][1]) == 20
    source = open(os.path.join(ROOT, "ap-adapter_amd", "csrc", "frontend.hip")).read()
    defn = re.search(r'extern "C" int apad_clap_logmel\((.*?)\) \{', source, re.S).group(1)
    assert [p.split()[-1] for p in defn.split(",")] == [p.split()[-1] for p in decl.split(",")]


def test_unsupported_arguments_raise_and_are_named():
    import ap_adapter_amd as A
    for kw, name in ((dict(fft_window_size=512), "fft_window_size"), (dict(feature_size=128), "feature_size"),
                     (dict(return_attention_mask=True), "return_attention_mask"), (dict(padding_value=1.0), "padding_value")):
        with pytest.raises(NotImplementedError, match=name):
            A.ClapFeatureExtractor(**kw)
    x = [np.zeros(1000, np.float32)]
    with pytest.raises(NotImplementedError, match="truncation"):  # the default, resolved at the call as in the installed class
        A.ClapFeatureExtractor()(x, sampling_rate=48000)
    fe = A.ClapFeatureExtractor(truncation="rand_trunc")
    with pytest.raises(NotImplementedError, match="truncation"):
        fe(x, truncation="fusion", sampling_rate=48000)
    with pytest.raises(NotImplementedError, match="padding"):
        fe(x, padding="wrap", sampling_rate=48000)
    with pytest.raises(ValueError, match="sampling rate of 48000"):
        fe(x, sampling_rate=16000)
    with pytest.raises(ValueError, match="sampling rate of 48000"):
        F.installed()(x, sampling_rate=16000)


def test_cpu_waveforms_without_a_gpu_raise(monkeypatch):
    import ap_adapter_amd as A
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    fe = A.ClapFeatureExtractor(truncation="rand_trunc")
    for x in (torch.zeros(2, 1000), [torch.zeros(1000), np.zeros(700, np.float32)]):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fe(x, sampling_rate=48000)


def test_tier_a_covers_the_live_frames_of_the_gpu_tests_signals():
    """from the reference alone, for the seeds tests/test_gpu_clap_features.py uses: at least 95 % of the entries of the non-silent
    frames are within 60 dB of their frame's maximum"""
    for fs in (64, 16):
        fe = F.installed(feature_size=fs)
        clips = [F.signal(n, 100 + k) for k, n in enumerate((300, 1000, 4800, 6000))]
        for padding in ("repeatpad", "repeat", "pad"):
            ref = F.reference(fe, clips, padding, ML, [None, None, None, 1200])
            cov = F.tier_a_coverage(ref)
            print(f"feature_size {fs} {padding}: tier A covers {cov:.4f} of the live entries")
            assert cov >= 0.95
