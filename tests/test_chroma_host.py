"""CPU: the host half of chroma similarity -- the product's filterbank against the oracle's independent one, the pitch anchors and the
frame-count rule on the fp64 oracle, ``rank_by`` validation, the group-restricted ordering and the ABI additions."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

import chroma_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_filterbank_matches_the_independent_restatement():
    from ap_adapter_amd import chroma
    ours, ref = chroma.chroma_filterbank(), O.filterbank()
    assert ours.dtype == np.float64 and ours.shape == ref.shape == (12, 1025)
    err = float(np.abs(ours - ref).max())
    print(f"filterbank: max-abs difference {err:.3e} (max weight {ref.max():.3f})")
    assert err < 1e-12
    # the L2-normalised columns carry the octave weight alone, and every weight is a non-negative number
    assert np.isfinite(ours).all() and (ours >= 0).all() and 0.9 < ours.max() <= 1.0
    # another tuning moves the bumps: with A half a class higher, the bin just below 440 Hz (437.5 Hz) is nearer to G sharp than to A
    k = 440 * 2048 // 16000
    assert np.argmax(ours[:, k]) == 9
    shifted = chroma.chroma_filterbank(tuning=0.5)
    assert np.argmax(shifted[:, k]) == 8 and shifted[9, k] < ours[9, k]


@pytest.mark.parametrize("freq,row", [(440.0, 9), (261.63, 0), (329.63, 4)])
def test_pitch_anchors(freq, row):
    c = O.chroma(O.tone(freq))
    assert c.shape == (17, 12)
    assert (c.argmax(dim=1) == row).all(), c.argmax(dim=1).tolist()
    assert float(c[:, row].min()) == 1.0  # L-infinity normalisation: the peak class is exactly 1


@pytest.mark.parametrize("n,frames", [(1, 1), (511, 1), (512, 2), (2047, 4), (2048, 5), (5121, 11), (163840, 321)])
def test_frame_count_rule(n, frames):
    from ap_adapter_amd import chroma
    assert chroma.frame_count(n) == O.frame_count(n) == frames
    if n <= 5121:
        assert O.chroma(O.signal(n, 1)).shape == (frames, 12)


def test_oracle_silence_and_similarity():
    assert bool((O.chroma(np.zeros(3000)) == 0).all())
    a = torch.rand(2, 5, 12, dtype=torch.float64)
    s, per = O.similarity(a, a, [0, 1], [5, 0])
    assert abs(float(s[0]) - 1.0) < 1e-12 and float(s[1]) == 0.0 and bool((per[1] == 0).all())
    x = [O.signal(4096, 3), O.signal(4096, 4)]
    s = O.waveform_similarity(x, x[:1])
    assert abs(float(s[0]) - 1.0) < 1e-12 and 0.0 < float(s[1]) < 0.999


def _pipe(**parts):
    import ap_adapter_amd as A
    return A.AudioLDM2Pipeline(None, **parts)


BAD_RANK_BY = ["chromagram", "CLAP", "", 3, 1.0, ("clap", "chroma"), ["chroma"], {}, {"clap": 1.0}, {"chroma": 1.0},
               {"clap": 1.0, "chroma": 1.0, "fad": 1.0}, {"clap": "a", "chroma": 1.0}, {"clap": 1.0, "chroma": None},
               {"clap": float("nan"), "chroma": 1.0}, {"clap": 1.0, "chroma": float("inf")}]


@pytest.mark.parametrize("bad", BAD_RANK_BY, ids=[repr(b) for b in BAD_RANK_BY])
def test_rank_by_refuses_anything_else(bad):
    from ap_adapter_amd import chroma
    with pytest.raises(ValueError, match="rank_by="):
        chroma.resolve_rank_by(bad)
    with pytest.raises(ValueError, match="rank_by="):
        _pipe().check_rank_arguments(bad, None, True, ["a prompt"], 4)


def test_rank_by_resolution():
    from ap_adapter_amd import chroma
    assert chroma.resolve_rank_by(None) is None and chroma.resolve_rank_by("clap") is None  # today's path
    assert chroma.resolve_rank_by("chroma") == (0.0, 1.0)
    assert chroma.resolve_rank_by({"clap": 2, "chroma": 0.5}) == (2.0, 0.5)
    pipe = _pipe()
    assert pipe.check_rank_arguments(None, None, False, None, 4) is None and pipe.check_rank_arguments("clap", None, False, None, 4) is None
    assert pipe.check_rank_arguments("chroma", None, True, None, 6) == (0.0, 1.0)  # neither text prompts nor towers
    assert pipe.check_rank_arguments({"clap": 0.0, "chroma": 1.0}, None, True, None, 6) == (0.0, 1.0)  # a zero weight needs nothing
    assert pipe.check_rank_arguments("chroma", torch.zeros(2, 100), True, None, 6) == (0.0, 1.0)
    assert pipe.check_rank_arguments("chroma", torch.zeros(100), True, None, 6) == (0.0, 1.0)


def test_rank_by_needs_a_source_and_what_clap_needs():
    pipe = _pipe()
    mixed = {"clap": 1.0, "chroma": 1.0}
    for rb in ("chroma", mixed):
        with pytest.raises(ValueError, match="needs one \\(source_audio="):
            pipe.check_rank_arguments(rb, None, False, ["a prompt"], 4)
    with pytest.raises(ValueError, match="text prompts"):
        pipe.check_rank_arguments(mixed, None, True, None, 4)
    with pytest.raises(NotImplementedError, match="audio_tower="):
        pipe.check_rank_arguments(mixed, None, True, ["a prompt"], 4)
    for rb in (None, "clap"):
        with pytest.raises(ValueError, match="fidelity_reference"):
            pipe.check_rank_arguments(rb, torch.zeros(100), True, ["a prompt"], 4)
    for ref in (torch.zeros(4, 2, 100), torch.zeros(3, 100), torch.zeros(2, 0), torch.zeros(0)):
        with pytest.raises(ValueError, match="fidelity_reference"):
            pipe.check_rank_arguments("chroma", ref, True, None, 4)


def test_call_checks_rank_by_before_any_device_work():
    """a pipeline without a UNet: the call fails on the argument, not on the missing model"""
    pipe = _pipe()
    e = dict(prompt_embeds=torch.zeros(2, 4, 8), negative_prompt_embeds=torch.zeros(2, 4, 8), generated_prompt_embeds=torch.zeros(2, 2, 8),
             negative_generated_prompt_embeds=torch.zeros(2, 2, 8), attention_mask=torch.ones(2, 4, dtype=torch.long),
             negative_attention_mask=torch.ones(2, 4, dtype=torch.long), output_type="latent", audio_length_in_s=0.64)
    with pytest.raises(ValueError, match="needs one \\(source_audio="):
        pipe(rank_by="chroma", **e)
    with pytest.raises(ValueError, match="rank_by='chromagram'"):
        pipe(rank_by="chromagram", **e)
    with pytest.raises(ValueError, match="fidelity_reference"):
        pipe(fidelity_reference=torch.zeros(100), **e)
    sig = inspect.signature(type(pipe).__call__).parameters
    assert sig["rank_by"].default is None and sig["fidelity_reference"].default is None
    # (they sit in front of the inversion keywords: tests/test_invert_host.py pins those as the signature's last six)
    assert list(sig)[-8:-6] == ["rank_by", "fidelity_reference"] and list(sig)[-6] == "inversion"
    assert pipe.last_chroma_similarity is None


def test_group_restricted_ordering():
    from ap_adapter_amd import chroma
    # two prompts x three candidates: the best of the batch sits in group 1 and must stay there
    sim = torch.tensor([0.2, 0.5, 0.3, 0.9, 0.7, 0.8])
    assert chroma.group_order(sim, 3).tolist() == [1, 2, 0, 3, 5, 4]
    assert chroma.group_order(sim, 1).tolist() == [0, 1, 2, 3, 4, 5]
    assert chroma.group_order(sim, 6).tolist() == [3, 5, 4, 1, 2, 0]
    assert chroma.group_order(torch.tensor([0.5, 0.5, 0.1, 0.5]), 2).tolist() == [0, 1, 3, 2]  # ties keep their order
    # the mixed form: w_t cos_clap + w_f chroma, cos_clap[i] = logits[i // n, i] / logit_scale -- candidate against its OWN prompt
    logits = torch.tensor([[10.0, 2.0, 4.0, 99.0, 99.0, 99.0], [99.0, 99.0, 99.0, 1.0, 8.0, 2.0]])
    s = chroma.mixed_scores((1.0, 2.0), sim, logits, 10.0, 3)
    want = [1.0 + 0.4, 0.2 + 1.0, 0.4 + 0.6, 0.1 + 1.8, 0.8 + 1.4, 0.2 + 1.6]
    assert s.dtype == torch.float64 and np.allclose(s.numpy(), want, rtol=0, atol=1e-6)
    assert chroma.group_order(s, 3).tolist() == [0, 1, 2, 4, 3, 5]
    assert chroma.group_order(chroma.mixed_scores((0.0, 1.0), sim, None, 10.0, 3), 3).tolist() == [1, 2, 0, 3, 5, 4]  # no logits read
    assert chroma.group_order(chroma.mixed_scores((1.0, 0.0), sim, logits, 10.0, 3), 3).tolist() == [0, 2, 1, 4, 5, 3]


def test_abi_additions():
    from ap_adapter_amd import _lib
    header = open(os.path.join(ROOT, "include", "apadapter_hip.h")).read()
    source = open(os.path.join(ROOT, "ap-adapter_amd", "csrc", "frontend.hip")).read()
    for name, nargs in (("apad_chroma", 10), ("apad_chroma_similarity", 12)):
        decl = re.search(r"\bint %s\((.*?)\);" % name, header, re.S).group(1)
        defn = re.search(r'extern "C" int %s\((.*?)\) \{' % name, source, re.S).group(1)
        assert len(decl.split(",")) == len(defn.split(",")) == len(_lib.SYMBOLS[name][1]) == nargs
    assert "fft_radix2<11, 256>" in source
    assert "#define APAD_ABI_VERSION 12\n" in header  # additive: the ABI version stays


def test_evaluate_edits_pairs_files_by_name(tmp_path):
    import importlib.util
    spec = importlib.util.spec_from_file_location("evaluate_edits", os.path.join(ROOT, "tools", "evaluate_edits.py"))
    E = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(E)
    src, edits = tmp_path / "src", tmp_path / "edits"
    src.mkdir(), edits.mkdir()
    for d, names in ((src, ("a.wav", "b.wav", "c.wav")), (edits, ("b.wav", "a.wav", "notes.txt"))):
        for n in names:
            (d / n).write_bytes(b"")
    assert [(n, os.path.basename(s), os.path.basename(e)) for n, s, e in E.pair_files(str(src), str(edits))] == [("a.wav", "a.wav", "a.wav"), ("b.wav", "b.wav", "b.wav")]
    assert [os.path.basename(s) for _, s, _ in E.pair_files(str(src), str(edits), {"a.wav": "c.wav", "b.wav": "a.wav"})] == ["c.wav", "a.wav"]
    (edits / "d.wav").write_bytes(b"")
    with pytest.raises(SystemExit, match="d.wav has no source"):
        E.pair_files(str(src), str(edits))
    with pytest.raises(SystemExit, match="not in --pairs"):
        E.pair_files(str(src), str(edits), {"a.wav": "c.wav", "b.wav": "a.wav"})
    (tmp_path / "p.json").write_text('{"a.wav": "a jazz band"}')
    (tmp_path / "p.tsv").write_text("a.wav\ta jazz band\nb.wav\tdrums, then strings\n")
    assert E.read_prompts(str(tmp_path / "p.json")) == {"a.wav": "a jazz band"}
    assert E.read_prompts(str(tmp_path / "p.tsv")) == {"a.wav": "a jazz band", "b.wav": "drums, then strings"}
