"""Time apad_cfg_shaped_step -- all knobs on, guidance rescale only, and the all-off row -- against apad_cfg_sampler_step and
apad_cfg_dual_step at the bench geometry (B = 32 clips of 4000 latent pixels x 8 channels, bf16, DPM-Solver++ 2M interior row), all in ONE
process, alternating, and write the medians to profiles/shaped_step.json.

    python tools/shaped_step_time.py [--out profiles/shaped_step.json] [--rounds 15] [--launches 200]

This is the ONLY measurement of the feature: the update kernel alone, one workgroup per clip (32 workgroups on a 256-CU chip), each walking
its clip up to three times.  The buffers (tens of MB) stay cache-resident between the back-to-back launches, so nothing here is an HBM rate,
and no end-to-end time of a shaped run has been measured.  An existing "error_to_bound" entry of the output file (written by
tests/test_gpu_shaped_guidance.py under APAD_SHAPED_PROFILE) is kept.  The GPU work runs in a child process under a time limit; a run
without a GPU fails."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, NPIX, C, STEPS = 32, 4000, 8, 200
STEP_MS = 32.5  # the denoise step the README records for this geometry; the condition on the added time is 1 % of it


def child(args):
    import torch
    import ap_adapter_amd as A
    from ap_adapter_amd import ops
    from ap_adapter_amd.scheduler import guidance_table, shape_table
    if not torch.cuda.is_available():
        raise SystemExit("shaped_step_time: no GPU visible; nothing is measured without one")
    dev, dtype = torch.device("cuda:0"), torch.bfloat16
    n = NPIX * C
    g = torch.Generator().manual_seed(0)
    R = lambda *s: torch.randn(*s, generator=g)
    sched = A.DPMSolverMultistepScheduler()
    sched.set_timesteps(STEPS)
    coef = sched.sampler_plan(0.0, dual=True).table.to(dev)
    c = R(B, n) * 0.5 + 0.1
    e_a = c + 0.2 * R(B, n)
    eps3 = torch.cat([e_a + 0.3 * R(B, n), e_a, c]).to(dev, dtype)
    eps2 = torch.cat([eps3[:B], eps3[2 * B:]]).contiguous()
    lat0 = R(B, n).to(dev)
    lat, unet_in, hist = lat0.clone(), torch.empty(B, n, dtype=dtype, device=dev), torch.zeros(B, n, device=dev)
    gtab = guidance_table(2.5, 7.5, STEPS).to(dev)
    ptr = torch.full((1,), STEPS // 2, dtype=torch.int32, device=dev)  # an interior (second-order) row
    r = 0.15 * n ** 0.5
    tables = {"all": shape_table(0.7, 0.25, r, -0.5, STEPS), "rescale": shape_table(0.7, 1.0, 0.0, 0.0, STEPS), "off": shape_table(0.0, 1.0, 0.0, 0.0, STEPS)}
    tables = {k: v.to(dev) for k, v in tables.items()}
    mom = {2: torch.zeros(1, B, n, device=dev), 3: torch.zeros(2, B, n, device=dev)}
    kernels = ["sampler", "dual"] + [f"shaped{nb}_{k}" for nb in (2, 3) for k in tables]

    def run(kernel, launches):
        lat.copy_(lat0)
        hist.zero_()
        for m in mom.values():
            m.zero_()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(launches):
            if kernel == "sampler":
                ops.cfg_sampler_step(eps2, lat, unet_in, coef, ptr, 7.5, None, hist)
            elif kernel == "dual":
                ops.cfg_dual_step(eps3, lat, unet_in, coef, gtab, ptr, None, hist)
            else:
                nb, knobs = int(kernel[6]), kernel[8:]
                ops.cfg_shaped_step(eps2 if nb == 2 else eps3, lat, unet_in, coef, tables[knobs], ptr, 7.5 if nb == 2 else None,
                                    None if nb == 2 else gtab, mom[nb] if knobs == "all" else None, None, None, hist)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / launches  # us per launch

    for kernel in kernels:  # warm-up: code objects loaded, buffers touched
        run(kernel, 20)
    times = {kernel: [] for kernel in kernels}
    for _ in range(args.rounds):  # alternate the entry points within every round
        for kernel in kernels:
            times[kernel].append(run(kernel, args.launches))
    results = {k: {"median_us": round(statistics.median(ts), 3), "min_us": round(min(ts), 3), "max_us": round(max(ts), 3)} for k, ts in times.items()}
    added = {k: round(results[k]["median_us"] - results["sampler" if k[6] == "2" else "dual"]["median_us"], 3) for k in kernels if k.startswith("shaped")}
    out = {}
    if os.path.exists(args.out):
        with open(args.out) as f:
            out = {k: v for k, v in json.load(f).items() if k == "error_to_bound"}
    out.update({"what": "apad_cfg_shaped_step (two and three branches; all knobs on / guidance rescale only / the all-off row) vs apad_cfg_sampler_step and "
                        "apad_cfg_dual_step, back-to-back launches timed with device events; medians over rounds, the entry points alternated within "
                        "each round; the working set (tens of MB) stays cache-resident across launches, so no figure here is an HBM rate",
                "not_measured": ["end-to-end time of a shaped run", "audio quality (no real weights)"],
                "device": torch.cuda.get_device_name(0), "B": B, "n": n, "C": C, "dtype": "bfloat16", "rounds": args.rounds,
                "launches_per_round": args.launches, "results": results, "added_us_over_the_plain_step": added,
                "condition": {"what": f"added time under 1 % of the {STEP_MS} ms denoise step", "limit_us": STEP_MS * 10.0,
                              "worst_added_us": max(added.values()), "holds": max(added.values()) < STEP_MS * 10.0}})
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "shaped_step.json"))
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--timeout", type=int, default=240, help="seconds the GPU step may take")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    # the GPU step: a fresh child process under its own time limit
    cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--child", "--out", args.out, "--rounds", str(args.rounds),
           "--launches", str(args.launches)]
    sys.exit(subprocess.run(cmd).returncode)


if __name__ == "__main__":
    main()
