"""Time the three apad_*_qw entry points (the audio prompt weighed per query token) against their apad_*_tab twins of the same build, and the
captured batch-32 step with an ``ap_scale`` table only against the same step with table + map, in ONE process, alternating; write the medians
to profiles/ap_region.json.

    python tools/ap_region_time.py [--out profiles/ap_region.json] [--rounds 15] [--launches 200] [--step-rounds 7]

  (i)  per launch, at the bench geometry (64 sample-forwards = batch 32 x 2 guidance branches, 8 text + 32 audio keys, bf16): apad_attention
       (C = 256, 1000 tokens), apad_cross_attention_rows (C = 384, 252 tokens) and apad_hs_attention (C = 640, 64 tokens), each through its
       _tab entry point and through its _qw entry point with the same table and a [32, tokens] region map; back-to-back launches timed with
       device events, medians over rounds, the two entry points alternated within every round;
  (ii) the captured step of the full UNet at batch 32, ``pipeline.denoise(..., ap_scale=0.55)`` against ``..., ap_scale=0.55,
       ap_region=(4, 7))``: wall time of replayed calls of 10 and of 30 steps, alternated; (30-step wall - 10-step wall) / 20 is the step without
       the per-call refill.  The difference between the two forms is the price of the C = 256 sites running the un-fused chain
       (apad_attention_qw between two GEMM launches) instead of apad_fused_cross_attention, plus the map loads of the other sites.

Neither says anything about audio quality or about which regions or weights are musically useful: the weights are synthetic.  The GPU work
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
GEOMETRY = {"attention": (256, 1000), "cross_attention_rows": (384, 252), "hs_attention": (640, 64)}
REGION = (4.0, 7.0)


def launchers(torch, ops, dev, dtype):
    """entry point -> launch(scale2, query_weight) on random operands of its bench geometry (the operands of tools/ap_scale_time.py)"""
    g = torch.Generator().manual_seed(0)
    R = lambda *s, std=1.0: (torch.randn(*s, generator=g) * std).to(dev, dtype).contiguous()
    out = {}
    for name, (C_, N) in GEOMETRY.items():
        H, d = 8, C_ // 8
        x, o = R(B, N, C_), torch.empty(B, N, C_, device=dev, dtype=dtype)
        ln = (1 + 0.1 * R(C_), 0.1 * R(C_), 1e-5)
        wq, wo, bo = R(C_, C_, std=0.05), R(C_, C_, std=0.05), R(C_, std=0.3)

        def kv(L):
            vt = torch.zeros(B, H, d, ops.round_up(L, 32), device=dev, dtype=dtype)
            vt[..., :L] = R(B, H, d, L)
            return R(B, L, C_, std=0.5), vt

        (k1, v1), (k2, v2) = kv(LT), kv(LA)
        if name == "attention":
            out[name] = lambda s, w, a=(x, k1, v1, k2, v2, o): ops.attention(a[0], a[1], a[2], LT, 8, k2=a[3], vt2=a[4], L2=LA, scale2=s, out=a[5],
                                                                             query_weight=w)
        elif name == "cross_attention_rows":
            wq_p, wo_p = ops.xrows_pack_weight(wq), ops.xrows_pack_weight(wo)
            p1, p2 = ops.rows_pack_kv(k1, v1), ops.rows_pack_kv(k2, v2)
            out[name] = lambda s, w, a=(x, wq_p, wo_p, bo, p1, ln, p2, o): ops.cross_attention_rows(a[0], a[1], a[2], a[3], a[4], None, 8, ln=a[5],
                                                                                                     k2=a[6], scale2=s, out=a[7], query_weight=w)
        else:
            wq_p, qb = ops.hs_pack_rows(wq, ln=ln)
            p1, p2 = ops.rows_pack_kv(k1, v1), ops.rows_pack_kv(k2, v2)
            out[name] = lambda s, w, a=(x, wq_p, qb, p1, p2, o): ops.hs_attention(a[0], a[1], a[2], self_attention=False, ln_eps=1e-5, k1=a[3],
                                                                                 k2=a[4], scale2=s, out=a[5], query_weight=w)
    return out


def launch_times(args, torch, ops, dev, dtype):
    table = torch.full((STEPS, CLIPS), 0.55, device=dev)
    step = torch.full((1,), STEPS // 2, dtype=torch.int32, device=dev)
    tab = ops.Scale2Binding(table, step, CLIPS)

    def run(fn, w, launches):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(launches):
            fn(tab, w)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / launches  # us per launch

    res = {}
    for name, fn in launchers(torch, ops, dev, dtype).items():
        N = GEOMETRY[name][1]
        ones = ops.QueryWeight(torch.ones(CLIPS, N, device=dev), CLIPS)
        region = torch.zeros(CLIPS, N, device=dev)
        region[:, 2 * N // 5: 7 * N // 10] = 1.0  # seconds 4 to 7 of 10
        forms = {"tab": None, "qw": ops.QueryWeight(region, CLIPS)}
        equal = bool(torch.equal(fn(tab, None).clone(), fn(tab, ones)))  # an all-ones map: the twin's bits
        for w in forms.values():  # warm-up: code objects loaded, buffers touched
            run(fn, w, 20)
        times = {k: [] for k in forms}
        for _ in range(args.rounds):  # alternate the two entry points within every round
            for k, w in forms.items():
                times[k].append(run(fn, w, args.launches))
        r = {k: {"median_us": round(statistics.median(ts), 3), "min_us": round(min(ts), 3), "max_us": round(max(ts), 3)} for k, ts in times.items()}
        r["qw_minus_tab_us"] = round(r["qw"]["median_us"] - r["tab"]["median_us"], 3)
        r["ones_map_bit_equal"] = equal
        r["C"], r["tokens"] = GEOMETRY[name]
        res["apad_" + name] = r
    return res


def step_times(args, torch, A, dev, dtype):
    from ap_adapter_amd.synthetic import init_synthetic_, synthetic_inputs
    with torch.device(dev):  # parameters are created and initialised ON the device, as bench.py does
        unet = A.AudioLDM2UNet2DConditionModel()
        A.install_ap_adapter(unet, None, scale=0.55)
    init_synthetic_(unet, 100, on_device=True)
    unet = unet.to(dev, dtype)
    unet.requires_grad_(False)
    inp = synthetic_inputs(CLIPS, LA, seed=0)
    pipe = A.AudioLDM2Pipeline(unet)
    ge = pipe.assemble_condition(inp["generated_prompt_embeds"].to(dev), inp["audio_tokens"].to(dev), inp["uncond_audio_tokens"].to(dev), dtype)
    pe, am, lat = inp["prompt_embeds"].to(dev, dtype), inp["attention_mask"].to(dev), inp["latents"].to(dev)
    forms = {"table": dict(ap_scale=0.55), "table_and_map": dict(ap_scale=0.55, ap_region=REGION)}
    short, long_ = 10, 30

    def call(kw, steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = pipe.denoise(lat, ge, pe, am, steps, 7.5, **kw)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    finite = True
    for kw in forms.values():  # the four captures (two forms x two step counts: MAX_CACHED_GRAPHS holds them)
        for steps in (short, long_):
            finite &= bool(torch.isfinite(call(kw, steps)[1]).all())
    captures = pipe.graph_captures
    walls = {k: {short: [], long_: []} for k in forms}
    for _ in range(args.step_rounds):  # alternate the two forms within every round
        for steps in (short, long_):
            for k, kw in forms.items():
                walls[k][steps].append(call(kw, steps)[0])
    res = {"batch": CLIPS, "region_s": list(REGION), "graph_captures": captures, "recaptured_while_timing": pipe.graph_captures != captures,
           "finite": finite, "rounds": args.step_rounds}
    for k in forms:
        w10, w30 = statistics.median(walls[k][short]), statistics.median(walls[k][long_])
        res[k] = {"wall_ms_%d_steps" % short: round(w10, 2), "wall_ms_%d_steps" % long_: round(w30, 2),
                  "step_ms": round((w30 - w10) / (long_ - short), 3)}
    res["map_minus_table_step_ms"] = round(res["table_and_map"]["step_ms"] - res["table"]["step_ms"], 3)
    return res


def child(args):
    import torch
    import ap_adapter_amd as A
    from ap_adapter_amd import ops
    if not torch.cuda.is_available():
        raise SystemExit("ap_region_time: no GPU visible; nothing is measured without one")
    dev, dtype = torch.device("cuda:0"), torch.bfloat16
    out = {"what": "(i) the three apad_*_qw entry points vs their apad_*_tab twins at the bench geometry, back-to-back launches timed with device "
                   "events, medians over rounds, the two entry points alternated within each round (the working set stays cache-resident across "
                   "launches); (ii) the captured batch-32 step of the full UNet with an ap_scale table only vs table + region map, alternated in "
                   "one process: (wall of a replayed 30-step call - wall of a replayed 10-step call) / 20",
           "not_measured": ["audio quality", "which regions or weights are musically useful (no real weights)",
                            "a run on another box: compare only the figures of one run with each other"],
           "device": torch.cuda.get_device_name(0), "sample_forwards": B, "clips": CLIPS, "text_keys": LT, "audio_keys": LA, "dtype": "bfloat16",
           "rounds": args.rounds, "launches_per_round": args.launches}
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ap_region.json"))
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--step-rounds", type=int, default=7)
    ap.add_argument("--launch-only", action="store_true", help="skip (ii): no full UNet is built")
    ap.add_argument("--timeout", type=int, default=420, help="seconds the GPU step may take")
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
