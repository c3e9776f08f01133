"""Score a directory of edits against the directory of their sources: chroma similarity per (source, edit) pair -- did the edit keep
the recording's melody and harmony -- and, when a CLAP checkpoint and a prompt file are given, the CLAP text-audio cosine -- did it
follow the text.  Files are paired by name: edits/NAME.wav with sources/NAME.wav; an edit named as run_sharded.py --wav-dir names them
("PROMPT_INDEX_ip..._t..._f....wav") cannot be paired by name and needs --pairs.

    python tools/evaluate_edits.py --sources DIR --edits DIR [--out scores.json]
    python tools/evaluate_edits.py --sources DIR --edits DIR --pairs pairs.json          ({"edit file name": "source file name", ...})
    python tools/evaluate_edits.py --sources DIR --edits DIR --prompts prompts.json --clap CLAP_DIR
                                    (prompts.json: {"edit file name": "text", ...}, or a text file with one "name<TAB>text" per line;
                                     CLAP_DIR: a local transformers ClapModel checkpoint with its tokenizer files)

Every wav is read on the host, resampled to 16 kHz on the GPU (apad_resample_fir) and scored in batches of --batch pairs: two
apad_chroma launches and one apad_chroma_similarity launch per batch; the CLAP leg is score_waveforms' (apad_clap_logmel, the HIP
audio and text towers).  Chroma similarity is librosa's chroma_stft restated with the tuning fixed at 0 (ap_adapter_amd/chroma.py):
compare its numbers with each other, not with a librosa-based evaluation.

Every pair also gets the source's and the edit's integrated loudness (ITU-R BS.1770-4, mono, measured on the 16 kHz signal:
ap_adapter_amd/loudness.py, one apad_loudness launch per side and batch) and their difference in LU -- "this edit came out 5 LU hotter
than its source".  A clip shorter than 400 ms or silent has no loudness: null.  Not compared against libebur128 / pyloudnorm.

Every pair also gets the integer lag, within +- --align-search-s seconds, at which the edit correlates best with its source over the
length both have (ap_adapter_amd/align.py: apad_align_corr and apad_align_apply; positive = the edit is late), in samples and in ms, with the
normalised correlation there and at lag 0 -- whether a decoder's output sits on its recording closely enough for a sample-domain splice,
the measurement ``splice="source", align="kept"`` acts on.  The whole clip counts as kept material here (no region is known); a pair too
short for the search width has no lag: null.
"""
import argparse
import glob
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402


def pair_files(sources, edits, pairs=None):
    """[(name, source path, edit path)] in name order; raises when an edit has no source"""
    out = []
    for e in sorted(glob.glob(os.path.join(edits, "*.wav"))):
        name = os.path.basename(e)
        if pairs is not None and name not in pairs:
            raise SystemExit(f"evaluate_edits: {name} is not in --pairs")
        s = os.path.join(sources, pairs[name] if pairs is not None else name)
        if not os.path.exists(s):
            raise SystemExit(f"evaluate_edits: {name} has no source {s}" + ("" if pairs is not None else " (pair by name, or pass --pairs)"))
        out.append((name, s, e))
    if not out:
        raise SystemExit(f"evaluate_edits: no wav files in {edits}")
    return out


def read_prompts(path):
    with open(path) as f:
        text = f.read()
    try:
        return {str(k): str(v) for k, v in json.loads(text).items()}
    except ValueError:
        return dict(line.split("\t", 1) for line in text.splitlines() if "\t" in line)


def load_16k(path, dev):
    """channel 0 of a wav file at 16 kHz, fp32 on the device"""
    from ap_adapter_amd import frontend
    w, sr = frontend.load_wav(path)
    return frontend.resample(torch.from_numpy(w[:1]).to(dev), sr, 16000)[0]


def lufs(values):
    """fp32 loudness values -> JSON numbers, None where a clip has no loudness (-inf)"""
    import math
    return [round(float(v), 3) if math.isfinite(float(v)) else None for v in values]


def build_clap(clap_dir, dev):
    """(audio tower, text tower, tokenizer, feature extractor, logit_scale_t) from a local transformers ClapModel checkpoint"""
    import transformers
    import ap_adapter_amd as A
    from ap_adapter_amd import text_encoders as TE
    model = transformers.ClapModel.from_pretrained(clap_dir, local_files_only=True)
    tok = transformers.AutoTokenizer.from_pretrained(clap_dir, local_files_only=True)
    fields = lambda cls, cfg: {k: getattr(cfg, k) for k in cls.__dataclass_fields__ if hasattr(cfg, k) and k != "model_type"}
    audio = A.ClapAudioModelWithProjection(A.ClapAudioConfig(**fields(A.ClapAudioConfig, model.config.audio_config)))
    text = TE.ClapTextModelWithProjection(TE.ClapTextConfig(**fields(TE.ClapTextConfig, model.config.text_config)))
    sd = model.state_dict()
    for ours in (audio, text):
        missing = [k for k in ours.load_state_dict(sd, strict=False).missing_keys if not k.endswith("relative_position_index")]
        if missing:
            raise SystemExit(f"evaluate_edits: {clap_dir} lacks {missing[:4]} ...")
    fe = A.ClapFeatureExtractor(truncation="rand_trunc", padding="repeatpad")
    return audio.to(dev), text.to(dev), tok, fe, float(model.logit_scale_t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sources", required=True, help="directory of source wavs")
    ap.add_argument("--edits", required=True, help="directory of edited wavs, named like their sources (or see --pairs)")
    ap.add_argument("--pairs", default=None, help="JSON {edit file name: source file name} when the names differ")
    ap.add_argument("--prompts", default=None, help="JSON {edit file name: text}, or lines of name<TAB>text: the edit prompts, for the CLAP cosine")
    ap.add_argument("--clap", default=None, metavar="DIR", help="local transformers ClapModel checkpoint (weights + tokenizer): adds the CLAP cosine")
    ap.add_argument("--batch", type=int, default=32, help="pairs per launch")
    ap.add_argument("--align-search-s", type=float, default=0.02, metavar="S", help="the lag of each edit to its source is searched within +-S "
                    "seconds (at most 1024 samples at 16 kHz)")
    ap.add_argument("--out", default=None, help="write the JSON here (default: print only)")
    args = ap.parse_args()
    if (args.prompts is None) != (args.clap is None):
        ap.error("the CLAP cosine needs both --prompts and --clap")
    if not torch.cuda.is_available():
        raise SystemExit("evaluate_edits: needs the GPU (the HIP path has no CPU fallback)")
    import ap_adapter_amd as A
    from types import SimpleNamespace
    dev = torch.device("cuda:0")
    pairs = pair_files(args.sources, args.edits, None if args.pairs is None else json.load(open(args.pairs)))
    prompts = pipe = None
    if args.clap is not None:
        prompts = read_prompts(args.prompts)
        lacking = [n for n, _, _ in pairs if n not in prompts]
        if lacking:
            raise SystemExit(f"evaluate_edits: no prompt for {lacking[:4]} ...")
        audio, text, tok, fe, scale_t = build_clap(args.clap, dev)
        pipe = A.AudioLDM2Pipeline(None, vocoder=SimpleNamespace(config=SimpleNamespace(sampling_rate=16000)), audio_tower=audio,
                                   feature_extractor=fe, prompt_encoder=SimpleNamespace(text_encoder=text), tokenizer=tok)
        pipe.logit_scale_t = scale_t
    rows = []
    for i in range(0, len(pairs), args.batch):
        chunk = pairs[i:i + args.batch]
        src, edit = [load_16k(s, dev) for _, s, _ in chunk], [load_16k(e, dev) for _, _, e in chunk]
        sim = A.chroma_similarity(edit, src, ref_index=range(len(chunk))).cpu().tolist()
        l_src, l_edit = lufs(A.integrated_loudness(src).cpu()), lufs(A.integrated_loudness(edit).cpu())
        lagged = []
        for sw, ew in zip(src, edit):  # pair by pair: each over the length both have
            m = min(sw.numel(), ew.numel())
            try:
                _, lg, st = A.align_edit([ew[:m]], [sw[:m]], search_s=args.align_search_s, min_corr=-1.0)
                lagged.append({"lag_samples": int(lg[0, 0]), "lag_ms": round(int(lg[0, 0]) / 16.0, 4), "ncc_at_lag": round(float(st[0, 0]), 6),
                               "ncc_at_0": round(float(st[0, 1]), 6)})
            except ValueError:
                lagged.append({"lag_samples": None, "lag_ms": None, "ncc_at_lag": None, "ncc_at_0": None})
        cos = [None] * len(chunk)
        if pipe is not None:  # one clip at a time: the extractor crops at random past 10 s, the towers batch per call anyway
            import math
            for j, (name, _, _) in enumerate(chunk):
                pipe.score_waveforms(text=[prompts[name]], audio=edit[j][None].cpu(), num_waveforms_per_prompt=1, device=dev, dtype=torch.float32,
                                     audio_device=edit[j][None])
                cos[j] = float(pipe.last_logits_per_text[0, 0]) / math.exp(pipe.logit_scale_t)
        for (name, s, _), c, t, ls, le, lg in zip(chunk, sim, cos, l_src, l_edit, lagged):
            rows.append({"edit": name, "source": os.path.basename(s), "chroma_similarity": round(c, 6), "source_lufs": ls, "edit_lufs": le,
                         "loudness_difference_lu": None if ls is None or le is None else round(le - ls, 3), **lg,
                         **({} if t is None else {"prompt": prompts[name], "clap_cosine": round(t, 6)})})
    res = {"pairs": rows, "n": len(rows), "chroma_similarity_mean": round(sum(r["chroma_similarity"] for r in rows) / len(rows), 6),
           "chroma": "librosa.feature.chroma_stft restated (n_fft 2048, hop 512, 16 kHz, tuning fixed at 0); mean per-frame cosine over the "
                     "frames both clips have",
           "loudness": "ITU-R BS.1770-4 integrated loudness, mono, at 16 kHz (LUFS; null = no 400 ms block above the gates); difference = edit "
                       "- source in LU",
           "lag": f"the integer lag within +-{args.align_search_s} s of the largest cross-correlation of edit and source over their common "
                  "length at 16 kHz (positive = the edit is late), with the normalised correlation there and at lag 0; null = too short"}
    diffs = [r["loudness_difference_lu"] for r in rows if r["loudness_difference_lu"] is not None]
    if diffs:
        res["loudness_difference_lu_mean"] = round(sum(diffs) / len(diffs), 3)
    if pipe is not None:
        res["clap_cosine_mean"] = round(sum(r["clap_cosine"] for r in rows) / len(rows), 6)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
