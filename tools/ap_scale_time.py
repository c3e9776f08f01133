"""Time the four apad_*_tab entry points (ap_scale read from a device table) against their scalar twins of the same build, in ONE process,
alternating, and the first call against the later calls of an ``ap_scale=`` sweep; write the medians to profiles/ap_scale.json.

    python tools/ap_scale_time.py [--out profiles/ap_scale.json] [--rounds 15] [--launches 200] [--sweep-steps 10]

  (i)  per launch, at the bench geometry (64 sample-forwards = batch 32 x 2 guidance branches, 8 text + 32 audio keys, bf16): apad_attention
       (C = 256, 1000 tokens), apad_fused_cross_attention (C = 256, 1000 tokens), apad_cross_attention_rows (C = 384, 252 tokens) and
       apad_hs_attention (C = 640, 64 tokens), each with the float and with a [200, 32] table read at an interior row; back-to-back launches
       timed with device events, medians over rounds, the two entry points alternated within every round;
  (ii) wall time of ``pipeline.denoise(..., ap_scale=v)`` over a five-value sweep on the full UNet at batch 32: the first call warms up and
       captures the step, the others refill the table and replay it.

Neither says anything about audio quality or about which values or schedules are musically useful: the weights are synthetic.  The GPU work
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
GEOMETRY = {"attention": (256, 1000), "fused_cross_attention": (256, 1000), "cross_attention_rows": (384, 252), "hs_attention": (640, 64)}


def launchers(torch, ops, dev, dtype):
    """entry point -> launch(scale2) on random operands of its bench geometry"""
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
            out[name] = lambda s, a=(x, k1, v1, k2, v2, o): ops.attention(a[0], a[1], a[2], LT, 8, k2=a[3], vt2=a[4], L2=LA, scale2=s, out=a[5])
        elif name == "fused_cross_attention":
            (wq_p, q_fold), wo_p = ops.xattn_pack_weight(wq, ln), ops.xattn_pack_weight(wo)
            pk1, pk2 = ops.xattn_pack_kv(k1, v1, LT), ops.xattn_pack_kv(k2, v2, LA)
            out[name] = lambda s, a=(x, wq_p, wo_p, bo, pk1, ln, pk2, q_fold, o): ops.fused_cross_attention(
                a[0], a[1], a[2], a[3], a[4], LT, 8, ln=a[5], kv2_packed=a[6], L2=LA, scale2=s, q_fold=a[7], out=a[8])
        elif name == "cross_attention_rows":
            wq_p, wo_p = ops.xrows_pack_weight(wq), ops.xrows_pack_weight(wo)
            p1, p2 = ops.rows_pack_kv(k1, v1), ops.rows_pack_kv(k2, v2)
            out[name] = lambda s, a=(x, wq_p, wo_p, bo, p1, ln, p2, o): ops.cross_attention_rows(a[0], a[1], a[2], a[3], a[4], None, 8, ln=a[5], k2=a[6],
                                                                                                  scale2=s, out=a[7])
        else:
            wq_p, qb = ops.hs_pack_rows(wq, ln=ln)
            p1, p2 = ops.rows_pack_kv(k1, v1), ops.rows_pack_kv(k2, v2)
            out[name] = lambda s, a=(x, wq_p, qb, p1, p2, o): ops.hs_attention(a[0], a[1], a[2], self_attention=False, ln_eps=1e-5, k1=a[3], k2=a[4],
                                                                              scale2=s, out=a[5])
    return out


def launch_times(args, torch, ops, dev, dtype):
    table = torch.full((STEPS, CLIPS), 0.55, device=dev)
    step = torch.full((1,), STEPS // 2, dtype=torch.int32, device=dev)
    forms = {"scalar": 0.55, "tab": ops.Scale2Binding(table, step, CLIPS)}

    def run(fn, scale2, launches):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(launches):
            fn(scale2)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / launches  # us per launch

    res = {}
    for name, fn in launchers(torch, ops, dev, dtype).items():
        ref = fn(forms["scalar"]).clone()
        equal = bool(torch.equal(fn(forms["tab"]), ref))
        for s in forms.values():  # warm-up: code objects loaded, buffers touched
            run(fn, s, 20)
        times = {k: [] for k in forms}
        for _ in range(args.rounds):  # alternate the two entry points within every round
            for k, s in forms.items():
                times[k].append(run(fn, s, args.launches))
        r = {k: {"median_us": round(statistics.median(ts), 3), "min_us": round(min(ts), 3), "max_us": round(max(ts), 3)} for k, ts in times.items()}
        r["tab_minus_scalar_us"] = round(r["tab"]["median_us"] - r["scalar"]["median_us"], 3)
        r["bit_equal"] = equal
        r["C"], r["tokens"] = GEOMETRY[name]
        res["apad_" + name] = r
    return res


def sweep_times(args, torch, A, dev, dtype):
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
    walls = []
    for v in (0.3, 0.45, 0.55, 0.7, 1.0):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = pipe.denoise(lat, ge, pe, am, args.sweep_steps, 7.5, ap_scale=v)
        torch.cuda.synchronize()
        walls.append(round((time.perf_counter() - t0) * 1e3, 1))
    return {"values": [0.3, 0.45, 0.55, 0.7, 1.0], "steps": args.sweep_steps, "batch": CLIPS, "wall_ms_per_call": walls, "first_call_ms": walls[0],
            "later_call_median_ms": statistics.median(walls[1:]), "graph_captures": pipe.graph_captures, "graph_hits": pipe.graph_hits,
            "finite": bool(torch.isfinite(out).all())}


def child(args):
    import torch
    import ap_adapter_amd as A
    from ap_adapter_amd import ops
    if not torch.cuda.is_available():
        raise SystemExit("ap_scale_time: no GPU visible; nothing is measured without one")
    dev, dtype = torch.device("cuda:0"), torch.bfloat16
    out = {"what": "(i) the four apad_*_tab entry points vs their scalar twins at the bench geometry, back-to-back launches timed with device events, "
                   "medians over rounds, the two entry points alternated within each round (the working set stays cache-resident across launches); "
                   "(ii) wall time per pipeline.denoise call over a five-value ap_scale sweep on the full UNet: the first call captures, the others "
                   "replay",
           "not_measured": ["audio quality", "which ap_scale values or schedules are musically useful (no real weights)",
                            "a run on another box: compare only the figures of one run with each other"],
           "device": torch.cuda.get_device_name(0), "sample_forwards": B, "clips": CLIPS, "text_keys": LT, "audio_keys": LA, "dtype": "bfloat16",
           "rounds": args.rounds, "launches_per_round": args.launches}
    out["launch"] = launch_times(args, torch, ops, dev, dtype)
    if not args.launch_only:
        out["sweep"] = sweep_times(args, torch, A, dev, dtype)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ap_scale.json"))
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--sweep-steps", type=int, default=10)
    ap.add_argument("--launch-only", action="store_true", help="skip (ii): no full UNet is built")
    ap.add_argument("--timeout", type=int, default=420, help="seconds the GPU step may take")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    # the GPU step: a fresh child process under its own time limit
    cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--child", "--out", args.out, "--rounds", str(args.rounds),
           "--launches", str(args.launches), "--sweep-steps", str(args.sweep_steps)] + (["--launch-only"] if args.launch_only else [])
    sys.exit(subprocess.run(cmd).returncode)


if __name__ == "__main__":
    main()
