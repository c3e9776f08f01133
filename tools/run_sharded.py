"""BASELINE cfg 4 end to end: the clips of a directory of wavs (default: seeded synthetic 10 s tones, the evaluation audio is
not redistributable) x the task's prompts, sharded over the GPUs of the node, each rank running
wav -> Kaldi fbank -> AudioMAE (fp32) -> per-clip condition -> 200-step CFG + DDIM (hipGraph captured once per rank), latents
gathered in clip order on every rank; rank 0 writes them.

    python tools/run_sharded.py --task style_transfer --clips 256 --batch 32 --steps 200 [--audio-dir DIR] [--out latents.pt]
    python tools/run_sharded.py --gpus 8 --clips 256 ...        (starts its 8 ranks itself; equivalent to the line below)
    python -m torch.distributed.run --nnodes=1 --nproc-per-node 8 --master-addr 127.0.0.1 tools/run_sharded.py --clips 256 ...

Editing instead of generating (--strength S and / or --edit-region A:B, optionally --source-dir DIR): every clip starts from its source
wav -- the file of the same name in DIR, by default the audio prompt itself -- encoded by the VAE (random-init weights here), noised to
the interior timestep S selects, and only seconds A..B are regenerated.  Each clip's noise is seeded by its index, so a clip's result
does not depend on the batch or rank it lands in.
    python tools/run_sharded.py --clips 64 --steps 50 --strength 0.6 --edit-region 4:7

Edit-friendly DDPM inversion (--inversion ddpm, with --source-prompt TEXT and --source-guidance S; an edit run, DDIM only, eta = 1): each
batch first extracts its sources' per-step noise maps under the source prompt (``pipeline.invert``), then runs the edit on those maps under
the task's prompt.  The inversion's per-step draws are seeded by the batch's first clip, so here a clip's result does depend on its batch.
    python tools/run_sharded.py --clips 64 --steps 50 --strength 0.6 --inversion ddpm --source-prompt "a recording of a piano"

Fidelity of the edits (--rank-by chroma, an edit run with --wav-dir): every written clip is scored by chroma similarity (``score_fidelity``)
against its source as the same VAE and vocoder render it (the mean of the source's posterior, decoded), and each rank lists its clips best
first in WAV_DIR/fidelity_rank<R>.json.
    python tools/run_sharded.py --clips 64 --steps 50 --strength 0.6 --wav-dir out --rank-by chroma

Loudness of the written clips (--target-loudness L|source, --peak-limit-db P, with --wav-dir): before a clip is written it is brought to L
LUFS (ITU-R BS.1770-4 integrated loudness, ``normalize_loudness``), or -- "source", an edit run -- to the loudness of its source as the same
VAE and vocoder render it; a gain that would take its largest sample over P dBFS (default -1) is cut to the one that puts it there, so
nothing is clipped on disk.  Each rank lists file, LUFS before and after and gain in WAV_DIR/loudness_rank<R>.json.
    python tools/run_sharded.py --clips 64 --steps 50 --wav-dir out --target-loudness -14

Splicing a region edit back into its recording (--splice, with --edit-region and --wav-dir; --crossfade-s C, --seam-search-s S): before a clip
is written (and before --target-loudness) the decoded edit is joined to its source wav itself (``splice_edit``: channel 0, resampled to 16
kHz), so that outside the region and its two crossfades the file holds the recording's samples, not their re-rendering through the VAE and the
vocoder.  Each rank lists file, gain and window starts in WAV_DIR/splice_rank<R>.json.  With --align (--align-search-s S, --align-min-corr
C) the decoded edit is first shifted by the integer lag that correlates it best with the recording over the kept part
(``splice_edit_aligned``); the list then holds each clip's found lag, applied lag and normalised correlation.  Neither default is calibrated
on a real decoder.
    python tools/run_sharded.py --clips 64 --steps 50 --strength 0.6 --edit-region 4:7 --wav-dir out --splice

The weight of the audio prompt (--ap-scale V, or V0,V1,... with one value per step): ``text + ap_scale * audio`` in every decoupled attn2, read by
the captured step from a device table (``pipeline.denoise(ap_scale=)``) instead of the task preset's value baked into the processors; a
comma-separated list is a per-step schedule over the full grid.  Both passes of --inversion run under it.  The written wavs carry it in their
names (a schedule as "sched") and the summary line holds the values.
    python tools/run_sharded.py --clips 64 --steps 4 --ap-scale 1.0,0.7,0.4,0.1

The audio prompt by region (--ap-region A:B, seconds): the weight above is kept between A and B and is zero elsewhere, per query token of every
decoupled attn2 (``pipeline.denoise(ap_region=)``; the 256-wide sites then run the un-fused chain).  It composes with --ap-scale, and both
passes of --inversion run under it.
    python tools/run_sharded.py --clips 64 --steps 50 --ap-region 4:7

Several audio prompts per clip (--audio-prompt FILE[:START:END[:SCALE]], up to four times): every clip is conditioned on THESE recordings instead
of its own -- each with its own softmax in every decoupled attn2, its own region in seconds and its own weight (default: the whole clip, the
task preset's weight) -- ``pipeline.denoise(audio_prompts=)``.  One --audio-prompt is --ap-region / --ap-scale on that file; with two or more
every decoupled site runs the un-fused chain.  Not together with --ap-scale / --ap-region:
    python tools/run_sharded.py --clips 64 --steps 50 --audio-prompt cello.wav:0:5 --audio-prompt flute.wav:5:10:0.8
"""
import argparse
import glob
import json
import math
import os
import struct
import sys
import tempfile
import time
import wave

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402


EVAL_RATE_MIX = ((44100, 45), (48000, 5), (16000, 2))  # sample rates of the reference's eval_audio_* wavs: 45 + 5 + 2 files


def write_synthetic_wavs(out_dir, n=8, seconds=10.0, sr=16000, rate_mix=None):
    """seeded two-partial tones with a slow envelope, 16-bit PCM: stand-ins for eval_audio_in_domain/*.wav.  rate_mix = ((rate, weight), ...):
    file i takes the sample rate of its slot in the weighted cycle (EVAL_RATE_MIX: the evaluation set's 44.1 k / 48 k / 16 k proportions),
    so the front-end's resampler is on the path as it is for the real set"""
    os.makedirs(out_dir, exist_ok=True)
    paths = []
    # (each rate's slots spread evenly over the cycle: 16 files of EVAL_RATE_MIX already hold all three rates)
    cycle = [r for _, r in sorted(((k + 0.5) / w_, r) for r, w_ in (rate_mix or ((sr, 1),)) for k in range(w_))]
    for i in range(n):
        sr = cycle[i % len(cycle)] if rate_mix else sr
        g = torch.Generator().manual_seed(i)
        f0 = 110.0 * 2 ** (float(torch.rand(1, generator=g)) * 3)
        t = torch.arange(int(seconds * sr)) / sr
        x = 0.4 * torch.sin(2 * math.pi * f0 * t) + 0.2 * torch.sin(2 * math.pi * 2.01 * f0 * t + 0.3)
        x = x * (0.6 + 0.4 * torch.sin(2 * math.pi * 0.5 * t)) + 0.01 * torch.randn(t.shape, generator=g)
        p = os.path.join(out_dir, f"tone_{i}.wav")
        with wave.open(p, "wb") as w:
            w.setnchannels(1); w.setsampwidth(2); w.setframerate(sr)
            w.writeframes(struct.pack("<%dh" % x.numel(), *(x.clamp(-1, 1) * 32767).to(torch.int16).tolist()))
        paths.append(p)
    return paths


def write_wav16(path, x, sr=16000):
    """mono float waveform in [-1, 1] -> 16-bit PCM (the reference writes float32 through scipy.io.wavfile, inference.py:79-81)"""
    with wave.open(path, "wb") as w:
        w.setnchannels(1); w.setsampwidth(2); w.setframerate(sr)
        w.writeframes((x.clamp(-1, 1) * 32767).to(torch.int16).cpu().numpy().tobytes())


def build_decoder(dev, dtype, small=False, seed=300):
    """latents -> mel -> waveform stages (f-4): AutoencoderKL + SpeechT5HifiGan on the HIP path, random-init weights of the real shapes"""
    import ap_adapter_amd as A
    torch.manual_seed(seed)
    vae = A.AutoencoderKL(A.VaeConfig(block_out_channels=(32, 64, 64), layers_per_block=1, norm_num_groups=8) if small else A.VaeConfig())
    voc = A.SpeechT5HifiGan(A.HifiGanConfig(upsample_initial_channel=256) if small else A.HifiGanConfig())
    return vae.to(dev, dtype).requires_grad_(False), voc.to(dev, dtype).requires_grad_(False)


SAMPLERS = {"ddim": "DDIMScheduler", "dpmsolver++": "DPMSolverMultistepScheduler"}  # --sampler -> scheduler class of ap_adapter_amd


def build_job(dev, dtype, task_cfg, small=False, seed=100, adapter_ckpt=None, sampler="ddim"):
    """UNet + adapter + AudioMAE (fp32, the reference's type) on ``dev``; random-init weights of the real shapes unless an adapter
    checkpoint (reference key scheme) is given"""
    import ap_adapter_amd as A
    from ap_adapter_amd.synthetic import init_synthetic_
    cfg = A.UNetConfig(block_out_channels=(64, 128, 192, 256), attention_head_dim=4, norm_num_groups=16) if small else A.UNetConfig()
    with torch.device(dev):
        unet = A.AudioLDM2UNet2DConditionModel(cfg)
        sd = A.load_adapter(adapter_ckpt) if adapter_ckpt else None
        A.install_ap_adapter(unet, sd, scale=task_cfg["ap_scale"], num_tokens=8)
        mae = A.AudioMAEConditionCTPoolRand(**({"depth": 2} if small else {}))
    init_synthetic_(unet, seed, on_device=True)
    init_synthetic_(mae, seed + 1, w_std=0.02, on_device=True)
    if sd is not None:  # the checkpoint's adapter weights survive the synthetic init of the frozen part
        for n, p in unet.attn_processors.items():
            if hasattr(p, "to_k_ip"):
                p.to_k_ip.weight = torch.nn.Parameter(sd[n + ".to_k_ip.weight"].to(dev))
                p.to_v_ip.weight = torch.nn.Parameter(sd[n + ".to_v_ip.weight"].to(dev))
    unet = unet.to(dev, dtype).requires_grad_(False)
    return A.AudioLDM2Pipeline(unet, scheduler=getattr(A, SAMPLERS[sampler])(), audiomae=mae.to(dev, torch.float32))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--task", default="style_transfer")
    ap.add_argument("--audio-dir", default=None)
    ap.add_argument("--clips", type=int, default=None, help="number of clips (default: files x prompts)")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--sampler", choices=sorted(SAMPLERS), default="ddim", help="ddim: the reference's scheduler; dpmsolver++: DPM-Solver++ (2M), "
                                                                                "meant for 20 - 25 steps")
    ap.add_argument("--small", action="store_true", help="small UNet / 2-block AudioMAE (smoke runs)")
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--adapter-ckpt", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--wav-dir", default=None, help="decode every clip (VAE + vocoder on the HIP path) and write 16 kHz wavs named as "
                                                     "inference.py:79 names them")
    ap.add_argument("--source-dir", default=None, help="edit: directory holding each clip's source wav under the audio prompt's file name "
                                                        "(default: the audio prompt itself)")
    ap.add_argument("--strength", type=float, default=None, help="edit: in (0, 1], the share of the schedule that is run from the noised source")
    ap.add_argument("--edit-region", default=None, metavar="A:B", help="edit: regenerate seconds A..B only, keep the rest of the source")
    ap.add_argument("--audio-guidance", type=float, default=None, metavar="S", help="separate audio and text guidance: three branches per clip, "
                    "eps_0 + S (eps_A - eps_0) + guidance_scale (eps_AT - eps_A); without it the job is the two-branch one")
    ap.add_argument("--guidance-rescale", type=float, default=0.0, metavar="PHI", help="guidance rescale in [0, 1]: pulls the guided noise's "
                    "per-clip standard deviation back towards the conditioned branch's (0 = off)")
    ap.add_argument("--apg-eta", type=float, default=None, metavar="ETA", help="adaptive projected guidance: the weight of the guidance component "
                    "parallel to the conditioned prediction (1 = plain guidance, 0 = orthogonal part only; default: APG off)")
    ap.add_argument("--apg-norm-threshold", type=float, default=0.0, metavar="R", help="--apg-eta: clip the guidance difference's norm at R (0 = off)")
    ap.add_argument("--apg-momentum", type=float, default=0.0, metavar="BETA", help="--apg-eta: running average of the guidance differences over the "
                    "steps, |BETA| < 1 (APG uses negative values; 0 = off)")
    ap.add_argument("--inversion", choices=["ddpm"], default=None, help="edit from the source's own per-step noise (edit-friendly DDPM inversion) "
                    "instead of fresh noise: one more pass of the run's UNet steps; needs --sampler ddim, runs at eta = 1")
    ap.add_argument("--source-prompt", default="", metavar="TEXT", help="--inversion: the text describing the SOURCE clip (default: the empty prompt)")
    ap.add_argument("--source-guidance", type=float, default=3.0, metavar="S", help="--inversion: the text guidance scale of the inversion pass")
    ap.add_argument("--rank-by", choices=["chroma"], default=None, help="edit + --wav-dir: score every written clip by chroma similarity to its "
                    "source and list each rank's clips best first in WAV_DIR/fidelity_rank<R>.json")
    ap.add_argument("--target-loudness", default=None, metavar="L|source", help="--wav-dir: bring every written clip to L LUFS (BS.1770-4), or "
                    "'source' (an edit run): to the loudness of its source as the same VAE and vocoder render it")
    ap.add_argument("--peak-limit-db", type=float, default=-1.0, metavar="P", help="--target-loudness: no gain takes a clip's largest sample over "
                    "P dBFS (<= 0)")
    ap.add_argument("--splice", action="store_true", help="--edit-region + --wav-dir: splice every written edit back into its source recording "
                    "(outside the region and its crossfades the file holds the recording's own samples)")
    ap.add_argument("--crossfade-s", type=float, default=0.03, metavar="C", help="--splice: the length of each crossfade in seconds")
    ap.add_argument("--seam-search-s", type=float, default=0.08, metavar="S", help="--splice: how far outside the region a seam may move, in seconds")
    ap.add_argument("--align", action="store_true", help="--splice: shift every decoded edit by the integer lag that aligns it to its recording, "
                    "measured on the kept part, before it is spliced")
    ap.add_argument("--align-search-s", type=float, default=0.02, metavar="S", help="--align: lags up to +-S seconds are searched (at most 1024 "
                    "samples); not calibrated on a real decoder")
    ap.add_argument("--align-min-corr", type=float, default=0.5, metavar="C", help="--align: the found lag is applied only if its normalised "
                    "correlation reaches C; not calibrated on a real decoder")
    ap.add_argument("--ap-scale", default=None, metavar="V|V0,V1,...", help="the weight of the audio prompt in the decoupled cross-attention: one "
                    "float, or one per step (a schedule over the full grid); default: the task preset's value, set on the processors")
    ap.add_argument("--ap-region", default=None, metavar="A:B", help="seconds: the audio prompt weighs the tokens between A and B only "
                    "(ap_region=(A, B)); default: the whole clip")
    ap.add_argument("--audio-prompt", action="append", default=None, metavar="FILE[:START:END[:SCALE]]", help="repeatable (1 to 4): condition every "
                    "clip on these recordings, each weighing the tokens between START and END seconds only, by SCALE (audio_prompts=)")
    ap.add_argument("--gpus", type=int, default=1, help="N > 1 without a launcher: this script starts its N ranks itself (one per GPU)")
    args = ap.parse_args()
    if args.inversion and args.sampler != "ddim":
        ap.error("--inversion ddpm needs --sampler ddim: the multistep solver has no per-step noise to invert into")
    if args.rank_by and not (args.wav_dir and (args.strength is not None or args.edit_region is not None or args.source_dir is not None
                                               or args.inversion is not None)):
        ap.error("--rank-by chroma scores decoded edits against their sources: it needs an edit run (--strength / --edit-region / --source-dir / "
                 "--inversion) and --wav-dir")
    is_edit = args.strength is not None or args.edit_region is not None or args.source_dir is not None or args.inversion is not None
    if args.target_loudness is not None:
        if not args.wav_dir:
            ap.error("--target-loudness acts on the written waveforms: it needs --wav-dir")
        if args.target_loudness == "source":
            if not is_edit:
                ap.error("--target-loudness source matches an edit to its source: it needs an edit run (--strength / --edit-region / --source-dir / "
                         "--inversion)")
        else:
            try:
                args.target_loudness = float(args.target_loudness)
            except ValueError:
                args.target_loudness = float("nan")
            if not math.isfinite(args.target_loudness):
                ap.error("--target-loudness: a finite loudness in LUFS, or 'source'")
        if not args.peak_limit_db <= 0.0:
            ap.error("--peak-limit-db must be <= 0 dB relative to full scale")

    if args.splice:
        if not (args.wav_dir and args.edit_region):
            ap.error("--splice joins a region edit to its recording: it needs --edit-region and --wav-dir")
        try:
            from ap_adapter_amd.splice import check_lengths
            check_lengths(16000, args.crossfade_s, args.seam_search_s)
        except ValueError as err:
            ap.error(str(err))
    if args.align:
        if not args.splice:
            ap.error("--align shifts an edit ahead of its splice: it needs --splice")
        try:
            from ap_adapter_amd.align import check_arguments
            check_arguments(16000, "kept", args.align_search_s, args.align_min_corr)
        except ValueError as err:
            ap.error(str(err))

    if args.ap_scale is not None:
        try:
            vals = [float(v) for v in args.ap_scale.split(",")]
        except ValueError:
            ap.error("--ap-scale: one float, or a comma-separated list with one float per step")
        args.ap_scale = vals[0] if len(vals) == 1 else vals

    if args.ap_region is not None:
        try:
            a0, a1 = (float(v) for v in args.ap_region.split(":"))
        except ValueError:
            ap.error("--ap-region: A:B in seconds")
        args.ap_region = (a0, a1)

    if args.audio_prompt is not None:
        if args.ap_scale is not None or args.ap_region is not None:
            ap.error("--audio-prompt carries its own START:END and SCALE: not together with --ap-scale / --ap-region")
        if not 1 <= len(args.audio_prompt) <= 4:
            ap.error("--audio-prompt: 1 to 4 recordings")
        parsed = []
        for spec in args.audio_prompt:
            f = spec.rsplit(":", 3) if spec.count(":") >= 3 else spec.rsplit(":", 2) if spec.count(":") == 2 else [spec]
            try:
                if len(f) not in (1, 3, 4):
                    raise ValueError(spec)
                parsed.append((f[0], (float(f[1]), float(f[2])) if len(f) >= 3 else None, float(f[3]) if len(f) == 4 else None))
            except ValueError:
                ap.error(f"--audio-prompt {spec!r}: FILE, FILE:START:END or FILE:START:END:SCALE (seconds, a float)")
        args.audio_prompt = parsed

    from ap_adapter_amd import distributed as D
    if args.gpus > 1 and not D.launched_by_torchrun():
        sys.exit(D.spawn_ranks(args.gpus, os.path.abspath(__file__), sys.argv[1:]))

    import ap_adapter_amd as A
    from ap_adapter_amd import sharded as S
    from ap_adapter_amd.frontend import load_mel
    rank, world, local = A.distributed.init_from_env()
    torch.cuda.set_device(local)
    dev, dtype = torch.device("cuda", local), torch.bfloat16
    cfg = A.get_config(args.task)
    if args.audio_dir:
        files = sorted(glob.glob(os.path.join(args.audio_dir, "*.wav")))
    else:
        files = write_synthetic_wavs(os.path.join(tempfile.gettempdir(), "apad_synth_wavs"), seconds=args.seconds)
    clips = S.list_clips(files, cfg, args.clips)
    pipe = build_job(dev, dtype, cfg, small=args.small, adapter_ckpt=args.adapter_ckpt, sampler=args.sampler)
    H = int(args.seconds / pipe.vocoder_upsample_factor) // pipe.vae_scale_factor  # latent frames: 10 s -> 250 (pipeline_audioldm2.py:872-880)

    prompt_lengths = []

    def encode_audio(path, tp, fp):
        if args.audio_prompt is not None:  # the job's recordings instead of the clip's own: their tokens one after the other
            enc = [pipe.encode_audio(load_mel(f, device=dev), tp, fp) for f, _, _ in args.audio_prompt]
            prompt_lengths[:] = [tok.shape[1] for tok, _ in enc]
            return torch.cat([tok[0] for tok, _ in enc]), torch.cat([unc[0] for _, unc in enc])
        tok, unc = pipe.encode_audio(load_mel(path, device=dev), tp, fp)
        return tok[0], unc[0]

    editing = args.strength is not None or args.edit_region is not None or args.source_dir is not None or args.inversion is not None
    if editing:
        height = H * pipe.vae_scale_factor
        pipe.vae = build_decoder(dev, dtype, small=args.small)[0]
        region = tuple(float(v) for v in args.edit_region.split(":")) if args.edit_region else None
        # the pipeline's own argument checks, once, on a stand-in source of the right shape
        start, region_mask = pipe.check_edit_arguments(args.batch, height, args.steps, args.seconds, None, None, None, torch.empty(1, 8, H, 16),
                                                       1.0 if args.strength is None else args.strength, None, region)
        moments = {}

        def source_moments(path):
            from ap_adapter_amd.frontend import wav_to_mel
            src = os.path.join(args.source_dir, os.path.basename(path)) if args.source_dir else path
            if src not in moments:
                mel = wav_to_mel(src, (height + 0.5) / 102.4, device=dev)
                moments[src] = pipe.vae.encode(mel[None]).latent_dist._m.reshape(H * 16, 16)
            return moments[src]

    dual = {} if args.audio_guidance is None else {"audio_guidance_scale": args.audio_guidance}
    # guidance rescale / projected guidance (the edit pass only under --inversion); checked once, before any clip is touched
    shaping = dict(guidance_rescale=args.guidance_rescale, apg_eta=args.apg_eta, apg_norm_threshold=args.apg_norm_threshold,
                   apg_momentum=args.apg_momentum)
    try:
        shaped = pipe.check_shaping_arguments(*shaping.values(), args.steps) is not None
    except ValueError as err:
        ap.error(str(err))
    shaping = shaping if shaped else {}
    aps = {}
    if args.ap_scale is not None:  # the values of the steps the job runs, checked once; both passes of an inversion run take the keyword
        try:
            A.scheduler.ap_scale_table(args.ap_scale, args.steps, start if editing else 0)
        except ValueError as err:
            ap.error(str(err))
        aps = {"ap_scale": args.ap_scale}
    if args.ap_region is not None:  # the rows of the region, checked once against the job's latent height
        try:
            pipe.check_ap_mask(args.ap_region, None, 1, H, 16, has_audio=True)
        except ValueError as err:
            ap.error(str(err))
        aps["ap_region"] = args.ap_region

    if args.audio_prompt is not None:  # every prompt's region and weight, checked once against the job's latent height and steps
        try:
            pipe._host_audio_prompts([A.AudioPrompt(length=1, ap_scale=sc, ap_region=reg) for _, reg, sc in args.audio_prompt], args.steps,
                                     start if editing else 0, 1, H, 16)
        except ValueError as err:
            ap.error(str(err))

    def aps_now():  # (the prompts' token counts are known once the first batch has been encoded)
        if args.audio_prompt is None:
            return aps
        return {"audio_prompts": [A.AudioPrompt(length=n, ap_scale=sc, ap_region=reg) for n, (_, reg, sc) in zip(prompt_lengths, args.audio_prompt)]}

    def denoise(lat, gen, t5, mask, gs, clips=None):
        if not editing:
            return pipe.denoise(lat, gen, t5, mask, args.steps, gs, **dual, **shaping, **aps_now())
        # z0 = the clip's seeded latents (what a generation run would start from); the posterior draw is seeded by the clip index too
        post = torch.stack([torch.randn(8, H, 16, generator=torch.Generator().manual_seed(7919 * c["index"] + 1)) for c in clips])
        src = A.EditSource(z0=lat, moments=torch.cat([source_moments(c["audio"]) for c in clips]), post_noise=post,
                           scale=pipe.vae.config.scaling_factor, mask=region_mask)
        if args.inversion is None:
            return pipe.denoise(None, gen, t5, mask, args.steps, gs, source=src, start=start, **dual, **shaping, **aps_now())
        # the source condition: the batch's own, with the positive branch's text (the last b rows; 8 generated tokens) replaced
        b = lat.shape[0]
        sg, st, sm = S.synthetic_text_embeddings(args.source_prompt, t5_len=t5.shape[1])
        sgen, st5, smask = gen.clone(), t5.clone(), mask.clone()
        sgen[-b:, :8], st5[-b:], smask[-b:] = sg.to(gen), st.to(t5), sm.to(mask)
        inv = pipe.invert(src, sgen, st5, smask, args.steps, args.source_guidance, start=start, eta=1.0,
                          generator=torch.Generator().manual_seed(104729 * clips[0]["index"] + 2), **dual, **aps_now())
        return pipe.denoise(None, gen, t5, mask, args.steps, gs, source=inv, start=start, eta=1.0, **dual, **shaping, **aps_now())

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    local_out = S.run_sharded(clips, cfg, encode_audio, denoise, args.batch, rank, world, latent_shape=(8, H, 16), device=dev, pass_clips=True,
                              **({"branches": 3} if dual else {}))
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    n_wavs = 0
    if args.wav_dir:  # each rank decodes and writes its own clips (no collective): latents / scaling_factor -> mel -> waveform
        os.makedirs(args.wav_dir, exist_ok=True)
        vae, voc = build_decoder(dev, dtype, small=args.small)
        pipe.vae, pipe.vocoder = vae, voc
        scored, rendered, levels, seams, recordings = [], {}, [], [], {}
        if args.splice:  # the region as the mask's rows give it, and the whole plan, checked before the first clip is decoded
            n16 = int(args.seconds * 16000)
            spliced = [(a / 16000.0, b / 16000.0) for a, b in A.splice.mask_regions(region_mask, 640, n16)[0]]
            whole = A.splice.plan(n16, A.splice.mask_regions(region_mask, 640, n16)[0], *A.splice.check_lengths(16000, args.crossfade_s, args.seam_search_s))
            if args.align:
                A.align.plan(n16, whole.kept, A.align.check_arguments(16000, "kept", args.align_search_s, args.align_min_corr)[0])

        def recording(path):
            """the source wav itself at 16 kHz (channel 0), cropped or zero-padded to the clip"""
            src = os.path.join(args.source_dir, os.path.basename(path)) if args.source_dir else path
            if src not in recordings:
                recordings[src] = pipe._splice_reference(src, None, int(args.seconds * 16000), dev)[0]
            return recordings[src]

        def rendered_source(path):
            """the source as this VAE and vocoder render it: the mean of its posterior, decoded"""
            if path not in rendered:
                mean = source_moments(path)[:, :8].reshape(1, H, 16, 8).permute(0, 3, 1, 2).contiguous()
                rendered[path] = voc(vae.decode(mean.to(dev, dtype)).sample.squeeze(1))[:, : int(args.seconds * 16000)].float()
            return rendered[path]

        for idx in sorted(local_out):
            mel = vae.decode(local_out[idx][None].to(dev, dtype) / vae.config.scaling_factor).sample
            wav = pipe.mel_spectrogram_to_waveform(mel)[0, : int(args.seconds * 16000)]
            c = clips[idx]
            ip = cfg["ap_scale"] if args.ap_scale is None else "sched" if isinstance(args.ap_scale, list) else args.ap_scale
            name = f"{c['prompt']}_{idx}_ip{ip}_t{cfg['time_pooling']}_f{cfg['freq_pooling']}.wav".replace("/", "_")
            if args.splice:  # on the device, before the loudness stage: the kept part of the file is the recording itself
                aligned = {}
                if args.align:
                    wav, sg, starts, _, _, lags, ast = A.splice_edit_aligned(wav.to(dev).float(), recording(c["audio"]), spliced,
                                                                             crossfade_s=args.crossfade_s, seam_search_s=args.seam_search_s,
                                                                             return_plan=True, align="kept", align_search_s=args.align_search_s,
                                                                             align_min_corr=args.align_min_corr)
                    aligned = {"lag_found": int(lags[0, 0]), "lag_applied": int(lags[0, 1]), "ncc": round(float(ast[0, 0]), 6),
                               "ncc_lag0": round(float(ast[0, 1]), 6)}
                else:
                    wav, sg, starts, _, _ = A.splice_edit(wav.to(dev).float(), recording(c["audio"]), spliced, crossfade_s=args.crossfade_s,
                                                          seam_search_s=args.seam_search_s, return_plan=True)
                seams.append({"file": name, "gain": round(float(sg[0]), 6), "window_starts": [int(v) for v in starts[0] if int(v) >= 0], **aligned})
            if args.target_loudness is not None:  # on the device, before the write: a hot clip is turned down instead of clipped on disk
                to = dict(reference=rendered_source(c["audio"])) if args.target_loudness == "source" else dict(target=args.target_loudness)
                wav, gain, before = A.normalize_loudness(wav.to(dev), peak_limit_db=args.peak_limit_db, return_stats=True, **to)
                lufs = lambda v: round(float(v), 3) if math.isfinite(float(v)) else None
                levels.append({"file": name, "lufs_before": lufs(before[0, 0]), "lufs_after": lufs(A.integrated_loudness(wav)[0]),
                               "gain": round(float(gain[0]), 6)})
            write_wav16(os.path.join(args.wav_dir, name), wav)
            n_wavs += 1
            if args.rank_by:
                scored.append({"file": name, "source": os.path.basename(c["audio"]),
                               "chroma_similarity": round(float(pipe.score_fidelity(wav[None].to(dev), rendered_source(c["audio"]))[0]), 6)})
        if args.splice:
            with open(os.path.join(args.wav_dir, f"splice_rank{rank}.json"), "w") as f:
                json.dump(seams, f, indent=1)
                f.write("\n")
        if args.target_loudness is not None:
            with open(os.path.join(args.wav_dir, f"loudness_rank{rank}.json"), "w") as f:
                json.dump(levels, f, indent=1)
                f.write("\n")
        if args.rank_by:
            scored.sort(key=lambda r: -r["chroma_similarity"])
            with open(os.path.join(args.wav_dir, f"fidelity_rank{rank}.json"), "w") as f:
                json.dump(scored, f, indent=1)
                f.write("\n")
    allc = S.gather_clips(local_out, len(clips), rank, world)
    if rank == 0:
        finite = all(bool(torch.isfinite(x).all()) for x in allc)
        print(json.dumps({"task": args.task, "clips": len(clips), "world": world, "batch": args.batch, "steps": args.steps,
                          "sampler": args.sampler, "strength": args.strength, "edit_region": args.edit_region, "La": A.config.audio_tokens(cfg), "seconds_rank0": round(dt, 2), "clips_per_s": round(len(clips) / dt, 4),
                          "graph_captures": pipe.graph_captures, "graph_hits": pipe.graph_hits, "finite": finite,
                          "wavs_written_rank0": n_wavs, **({"audio_guidance": args.audio_guidance} if dual else {}), **shaping, **({"audio_prompts": [list(p) for p in args.audio_prompt]} if args.audio_prompt is not None else aps),
                          **({"inversion": args.inversion, "source_prompt": args.source_prompt, "source_guidance": args.source_guidance}
                             if args.inversion else {}),
                          **({"rank_by": args.rank_by, "chroma_similarity_mean_rank0": round(sum(r["chroma_similarity"] for r in scored) / max(len(scored), 1), 6)}
                             if args.rank_by else {}),
                          **({"target_loudness": args.target_loudness, "peak_limit_db": args.peak_limit_db} if args.target_loudness is not None else {}),
                          **({"splice": True, "crossfade_s": args.crossfade_s, "seam_search_s": args.seam_search_s} if args.splice else {}),
                          **({"align": True, "align_search_s": args.align_search_s, "align_min_corr": args.align_min_corr} if args.align else {})}))
        if args.out:
            torch.save({"latents": torch.stack([x.cpu() for x in allc]), "clips": clips}, args.out)
    if world > 1:
        torch.distributed.barrier()
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
