"""Time the three-branch step (separate audio and text guidance) against the two-branch step of the same build, in ONE process, alternating,
and write the medians to profiles/dual_guidance.json.

    python tools/dual_guidance_time.py [--out profiles/dual_guidance.json] [--rounds 15] [--launches 200] [--windows 9] [--replays 10]

  (i)  the update kernel alone: apad_cfg_dual_step against apad_cfg_sampler_step per launch, B = 32 clips of 4000 latent pixels x 8
       channels, bf16, DPM-Solver++ 2M interior row, back-to-back launches timed with device events;
  (ii) the captured step at the bench geometry (the full UNet, batch 32, La = 32, ap_scale 0.55): ``pipeline.denoise`` captures the
       three-branch and the two-branch step once each, then windows of ``--replays`` graph replays are timed with device events, the two
       graphs alternated; median over ``--windows`` windows, ms per replayed step.

Neither says anything about audio quality or about which scale values are useful: the weights are synthetic.  The GPU work runs in a child
process under a time limit; a run without a GPU fails."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, NPIX, C, STEPS = 32, 4000, 8, 200


def bytes_per_element(kernel):
    """what the algorithm moves per latent element, bf16 model dtype, DPM-Solver++ 2M interior step (history read and written): eps 2 bytes
    per branch read, latents 4 read + 4 written, unet_in 2 written, history 4 read + 4 written: 22 with two branches, 24 with three"""
    return {"sampler": 22.0, "dual": 24.0}[kernel]


def kernel_times(args, torch, A, ops, dev, dtype):
    n = NPIX * C
    g = torch.Generator().manual_seed(0)
    R = lambda *s: torch.randn(*s, generator=g)
    sched = A.DPMSolverMultistepScheduler()
    sched.set_timesteps(STEPS)
    plan = sched.sampler_plan(dual=True)
    coef = plan.table.to(dev)
    gtab = A.scheduler.guidance_table(2.5, 7.5, STEPS).to(dev)
    eps3 = (R(3 * B, n) * 0.5).to(dev, dtype)
    eps2 = eps3[: 2 * B]
    lat0 = R(B, n).to(dev)
    lat, unet_in, hist = lat0.clone(), torch.empty(B, n, dtype=dtype, device=dev), torch.zeros(B, n, device=dev)
    ptr = torch.full((1,), STEPS // 2, dtype=torch.int32, device=dev)  # an interior (second-order) row

    def run(kernel, launches):
        lat.copy_(lat0)
        hist.zero_()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(launches):
            if kernel == "sampler":
                ops.cfg_sampler_step(eps2, lat, unet_in, coef, ptr, 7.5, None, hist)
            else:
                ops.cfg_dual_step(eps3, lat, unet_in, coef, gtab, ptr, None, hist)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / launches  # us per launch

    kernels = ("sampler", "dual")
    for kernel in kernels:  # warm-up: code objects loaded, buffers touched
        run(kernel, 20)
    times = {kernel: [] for kernel in kernels}
    for _ in range(args.rounds):  # alternate the kernels within every round
        for kernel in kernels:
            times[kernel].append(run(kernel, args.launches))
    res = {}
    for kernel, ts in times.items():
        med = statistics.median(ts)
        res[kernel] = {"median_us": round(med, 3), "min_us": round(min(ts), 3), "max_us": round(max(ts), 3),
                       "bytes_per_element_by_shape": bytes_per_element(kernel),
                       "GB_per_s_at_median": round(bytes_per_element(kernel) * B * n / med / 1e3, 1)}
    res["dual_minus_sampler_us"] = round(res["dual"]["median_us"] - res["sampler"]["median_us"], 3)
    return res


def step_times(args, torch, A, dev, dtype):
    from ap_adapter_amd.synthetic import init_synthetic_, synthetic_inputs
    with torch.device(dev):  # parameters are created and initialised ON the device, as bench.py does
        unet = A.AudioLDM2UNet2DConditionModel()
        A.install_ap_adapter(unet, None, scale=0.55)
    init_synthetic_(unet, 100, on_device=True)
    unet = unet.to(dev, dtype)
    unet.requires_grad_(False)
    inp = synthetic_inputs(B, 32, seed=0)
    pipe = A.AudioLDM2Pipeline(unet, scheduler=A.DPMSolverMultistepScheduler())
    cond = lambda br: pipe.assemble_condition(inp["generated_prompt_embeds"].to(dev), inp["audio_tokens"].to(dev), inp["uncond_audio_tokens"].to(dev),
                                              dtype, branches=br)
    pe, am, lat = inp["prompt_embeds"].to(dev, dtype), inp["attention_mask"].to(dev), inp["latents"].to(dev)
    n_steps = 2 * args.replays  # the capture call itself runs this many steps
    pipe.denoise(lat, cond(2), pe, am, n_steps, 7.5)
    pipe.denoise(lat, cond(3), torch.cat([pe[:B], pe]), torch.cat([am[:B], am]), n_steps, 7.5, audio_guidance_scale=2.5)
    assert pipe.graph_captures == 2
    entries = {("three" if "dual" in key else "two"): e for key, e in pipe._graphs.items()}
    lat0 = lat.float().permute(0, 2, 3, 1).reshape(B, -1, 8).contiguous()

    def window(e):
        e["lat"].copy_(lat0)
        e["unet_in"].copy_(lat0)
        e["step_ptr"].zero_()
        e["hist"].zero_()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.replays):
            e["graph"].replay()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / args.replays  # ms per step

    for name in ("two", "three"):  # one untimed window each
        window(entries[name])
    times = {"two": [], "three": []}
    for _ in range(args.windows):
        for name in ("two", "three"):
            times[name].append(window(entries[name]))
    res = {name: {"median_ms_per_step": round(statistics.median(ts), 3), "min_ms": round(min(ts), 3), "max_ms": round(max(ts), 3),
                  "sample_forwards_per_step": B * (3 if name == "three" else 2)} for name, ts in times.items()}
    res["three_over_two"] = round(res["three"]["median_ms_per_step"] / res["two"]["median_ms_per_step"], 4)
    res["finite"] = all(bool(torch.isfinite(e["lat"]).all()) for e in entries.values())
    return res


def child(args):
    import torch
    import ap_adapter_amd as A
    from ap_adapter_amd import ops
    if not torch.cuda.is_available():
        raise SystemExit("dual_guidance_time: no GPU visible; nothing is measured without one")
    dev, dtype = torch.device("cuda:0"), torch.bfloat16
    out = {"what": "(i) apad_cfg_dual_step vs apad_cfg_sampler_step, back-to-back launches timed with device events, medians over rounds, the two "
                   "kernels alternated within each round (the working set stays cache-resident across launches, so the rates are not HBM rates); "
                   "(ii) the captured denoise step of the full UNet at batch 32 with three branches vs two, windows of graph replays timed with "
                   "device events, the two graphs alternated, median over windows",
           "not_measured": ["audio quality", "which (audio, text) scale values are musically useful (no real weights)",
                            "a run on another box: compare only the two figures of one run with each other"],
           "device": torch.cuda.get_device_name(0), "B": B, "n": NPIX * C, "C": C, "dtype": "bfloat16", "sampler": "dpmsolver++ (2M)",
           "rounds": args.rounds, "launches_per_round": args.launches, "windows": args.windows, "replays_per_window": args.replays}
    out["kernel"] = kernel_times(args, torch, A, ops, dev, dtype)
    if not args.kernel_only:
        out["captured_step"] = step_times(args, torch, A, dev, dtype)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dual_guidance.json"))
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--replays", type=int, default=10)
    ap.add_argument("--kernel-only", action="store_true", help="skip (ii): no full UNet is built")
    ap.add_argument("--timeout", type=int, default=420, help="seconds the GPU step may take")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    # the GPU step: a fresh child process under its own time limit
    cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--child", "--out", args.out, "--rounds", str(args.rounds),
           "--launches", str(args.launches), "--windows", str(args.windows), "--replays", str(args.replays)] + (["--kernel-only"] if args.kernel_only else [])
    sys.exit(subprocess.run(cmd).returncode)


if __name__ == "__main__":
    main()
