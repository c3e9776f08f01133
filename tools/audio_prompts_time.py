"""Time apad_attention_multi (several audio prompts per launch) against apad_attention_qw of the same build, and the captured batch-32 step
under one, two and three audio prompts, in ONE process, alternating; write the medians to profiles/audio_prompts.json.

    python tools/audio_prompts_time.py [--out profiles/audio_prompts.json] [--rounds 15] [--launches 200] [--step-rounds 7]

  (i)  per launch (64 sample-forwards = batch 32 x 2 guidance branches, 8 text keys + 32 keys per prompt, bf16, every prompt under a table and
       a [32, tokens] region map): apad_attention_qw, and apad_attention_multi with 1, 2 and 3 prompts, at d = 32 / 1000 tokens, d = 48 / 252
       tokens and d = 80 / 64 tokens; back-to-back launches timed with device events, medians over rounds, the entry points alternated
       within every round;
  (ii) the captured step of the full UNet at batch 32 (the bench geometry), four configurations alternated: one prompt on today's routes
       (``denoise`` without the keyword), one prompt with every decoupled site forced to the un-fused chain (``processors.route`` patched while
       that step is captured), two prompts and three prompts (``audio_prompts=``, each under its own ``ap_scale`` table).  Wall time of
       replayed calls of 10 and of 30 steps; (30-step wall - 10-step wall) / 20 is the step without the per-call refill.  chain - routes is
       the price of leaving the one-launch kernels, two - chain and three - two the price of each further prompt's segment.

Neither says anything about audio quality or about which weights or regions are musically useful: the weights are synthetic.  The GPU work
runs in a child process under a time limit; a run without a GPU fails."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, CLIPS, LT, LA, STEPS = 64, 32, 8, 32, 200
GEOMETRY = {"d32": (256, 1000), "d48": (384, 252), "d80": (640, 64)}


def launch_times(args, torch, ops, dev, dtype):
    g = torch.Generator().manual_seed(0)
    R = lambda *s, std=1.0: (torch.randn(*s, generator=g) * std).to(dev, dtype).contiguous()
    step = torch.full((1,), STEPS // 2, dtype=torch.int32, device=dev)
    res = {}
    for name, (C_, N) in GEOMETRY.items():
        H, d = 8, C_ // 8
        x, o = R(B, N, C_), torch.empty(B, N, C_, device=dev, dtype=dtype)

        def kv(L):
            vt = torch.zeros(B, H, d, ops.round_up(L, 32), device=dev, dtype=dtype)
            vt[..., :L] = R(B, H, d, L)
            return R(B, L, C_, std=0.5), vt

        k1, v1 = kv(LT)
        prompts = []
        for j in range(3):  # each prompt: its own K / V, table and region map (a third of the clip each)
            region = torch.zeros(CLIPS, N, device=dev)
            region[:, j * N // 3:(j + 1) * N // 3] = 1.0
            prompts.append(kv(LA) + (ops.Scale2Binding(torch.full((STEPS, CLIPS), 0.55 + 0.1 * j, device=dev), step, CLIPS), ops.QueryWeight(region, CLIPS)))

        def launch(n, multi=True):
            (k2, v2, s, w), rest = prompts[0], prompts[1:n]
            extra = [ops.AudioSegment(k, v, LA, s_, w_) for k, v, s_, w_ in rest] if multi else None
            return ops.attention(x, k1, v1, LT, H, k2=k2, vt2=v2, L2=LA, scale2=s, query_weight=w, out=o, extra=extra)

        forms = {"qw": lambda: launch(1, False), "multi_1": lambda: launch(1), "multi_2": lambda: launch(2), "multi_3": lambda: launch(3)}

        def run(fn, launches):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(launches):
                fn()
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) * 1e3 / launches  # us per launch

        equal = bool(torch.equal(forms["qw"]().clone(), forms["multi_1"]()))  # no extra segment: the twin's launch
        for fn in forms.values():  # warm-up: code objects loaded, buffers touched
            run(fn, 20)
        times = {k: [] for k in forms}
        for _ in range(args.rounds):  # alternate the entry points within every round
            for k, fn in forms.items():
                times[k].append(run(fn, args.launches))
        r = {k: {"median_us": round(statistics.median(ts), 3), "min_us": round(min(ts), 3), "max_us": round(max(ts), 3)} for k, ts in times.items()}
        for k in ("multi_1", "multi_2", "multi_3"):
            r[k + "_minus_qw_us"] = round(r[k]["median_us"] - r["qw"]["median_us"], 3)
        r["multi_1_bit_equal_to_qw"] = equal
        r["C"], r["tokens"], r["head_dim"] = C_, N, d
        res[name] = r
    return res


def step_times(args, torch, A, dev, dtype):
    from ap_adapter_amd import processors as P
    from ap_adapter_amd.synthetic import init_synthetic_, synthetic_inputs
    with torch.device(dev):  # parameters are created and initialised ON the device, as bench.py does
        unet = A.AudioLDM2UNet2DConditionModel()
        A.install_ap_adapter(unet, None, scale=0.55)
    init_synthetic_(unet, 100, on_device=True)
    unet = unet.to(dev, dtype)
    unet.requires_grad_(False)
    inp = synthetic_inputs(CLIPS, LA, seed=0)
    asm = A.AudioLDM2Pipeline.assemble_condition
    gen, tok, unc = (inp[k].to(dev) for k in ("generated_prompt_embeds", "audio_tokens", "uncond_audio_tokens"))
    more = [torch.randn(tok.shape, generator=torch.Generator().manual_seed(50 + j)).to(tok) for j in range(2)]
    conds = {1: asm(gen, tok, unc, dtype), 2: asm(gen, [tok, more[0]], unc, dtype), 3: asm(gen, [tok, more[0], more[1]], unc, dtype)}
    pe, am, lat = inp["prompt_embeds"].to(dev, dtype), inp["attention_mask"].to(dev), inp["latents"].to(dev)
    AP = A.AudioPrompt
    # name: (prompts, keywords, decoupled sites forced to the chain); one pipeline each: the first two share a graph key
    forms = {"one_prompt_routes": (1, {}, False), "one_prompt_chain": (1, {}, True),
             "two_prompts": (2, dict(audio_prompts=[AP(length=LA, ap_scale=0.55), AP(length=LA, ap_scale=0.45)]), False),
             "three_prompts": (3, dict(audio_prompts=[AP(length=LA, ap_scale=0.55), AP(length=LA, ap_scale=0.45), AP(length=LA, ap_scale=0.35)]), False)}
    pipes = {k: A.AudioLDM2Pipeline(unet) for k in forms}
    short, long_ = 10, 30
    real_route = P.route

    def call(k, steps):
        n, kw, chain = forms[k]
        if chain:  # (read while a step is captured; a replay calls no route)
            P.route = lambda kind, *a, **kw_: "chain" if kind == "decoupled" else real_route(kind, *a, **kw_)
        try:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = pipes[k].denoise(lat, conds[n], pe, am, steps, 7.5, **kw)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3, out
        finally:
            P.route = real_route

    finite = True
    for k in forms:  # the eight captures (four forms x two step counts)
        for steps in (short, long_):
            finite &= bool(torch.isfinite(call(k, steps)[1]).all())
    captures = sum(p.graph_captures for p in pipes.values())
    walls = {k: {short: [], long_: []} for k in forms}
    for _ in range(args.step_rounds):  # alternate the forms within every round
        for steps in (short, long_):
            for k in forms:
                walls[k][steps].append(call(k, steps)[0])
    res = {"batch": CLIPS, "graph_captures": captures, "recaptured_while_timing": sum(p.graph_captures for p in pipes.values()) != captures,
           "finite": finite, "rounds": args.step_rounds}
    for k in forms:
        w10, w30 = statistics.median(walls[k][short]), statistics.median(walls[k][long_])
        res[k] = {"wall_ms_%d_steps" % short: round(w10, 2), "wall_ms_%d_steps" % long_: round(w30, 2), "step_ms": round((w30 - w10) / (long_ - short), 3)}
    base = res["one_prompt_routes"]["step_ms"]
    for k in ("one_prompt_chain", "two_prompts", "three_prompts"):
        res[k]["minus_routes_step_ms"] = round(res[k]["step_ms"] - base, 3)
    res["chain_share_of_two_prompts_cost"] = round(res["one_prompt_chain"]["minus_routes_step_ms"] / res["two_prompts"]["minus_routes_step_ms"], 3) \
        if res["two_prompts"]["minus_routes_step_ms"] > 0 else None
    return res


def child(args):
    import torch
    import ap_adapter_amd as A
    from ap_adapter_amd import ops
    if not torch.cuda.is_available():
        raise SystemExit("audio_prompts_time: no GPU visible; nothing is measured without one")
    dev, dtype = torch.device("cuda:0"), torch.bfloat16
    out = {"what": "(i) apad_attention_multi with 1, 2 and 3 prompts vs apad_attention_qw at three head sizes, back-to-back launches timed with device "
                   "events, medians over rounds, the entry points alternated within each round (the working set stays cache-resident across "
                   "launches); (ii) the captured batch-32 step of the full UNet: one prompt on today's routes, one prompt with every decoupled "
                   "site on the un-fused chain, two prompts, three prompts, alternated in one process: (wall of a replayed 30-step call - wall of "
                   "a replayed 10-step call) / 20",
           "not_measured": ["audio quality", "which weights or regions are musically useful (no real weights)",
                            "a run on another box: compare only the figures of one run with each other"],
           "device": torch.cuda.get_device_name(0), "sample_forwards": B, "clips": CLIPS, "text_keys": LT, "audio_keys_per_prompt": LA,
           "dtype": "bfloat16", "rounds": args.rounds, "launches_per_round": args.launches}
    out["launch"] = launch_times(args, torch, ops, dev, dtype)
    if not args.launch_only:
        out["step"] = step_times(args, torch, A, dev, dtype)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "audio_prompts.json"))
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--step-rounds", type=int, default=7)
    ap.add_argument("--launch-only", action="store_true", help="skip (ii): no full UNet is built")
    ap.add_argument("--timeout", type=int, default=540, help="seconds the GPU step may take")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    # the GPU step: a fresh child process under its own time limit
    cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--child", "--out", args.out, "--rounds", str(args.rounds),
           "--launches", str(args.launches), "--step-rounds", str(args.step_rounds)] + (["--launch-only"] if args.launch_only else [])
    sys.exit(subprocess.run(cmd).returncode)


if __name__ == "__main__":
    main()
