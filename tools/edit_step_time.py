"""Time apad_cfg_edit_step against apad_cfg_sampler_step, and apad_cfg_ddim_step on its two-column table, at the bench geometry (B = 32
clips of 4000 latent pixels x 8 channels, bf16), all in ONE process, alternating, and write the medians to profiles/edit_step.json.

    python tools/edit_step_time.py [--out profiles/edit_step.json] [--rounds 15] [--launches 200]

This is the ONLY measurement of the edit feature: the update kernel alone.  The edit kernel also reads x0, z0 and the mask (about 22
bytes per element against about 14), over about one million elements, beside a UNet step of tens of milliseconds; no end-to-end edit
time has been measured.  The GPU work runs in a child process under a time limit; a run without a GPU fails."""
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
    """what the algorithm moves per latent element, bf16 model dtype, DPM-Solver++ 2M interior step (history read and written):
    eps2 2 x 2 read, latents 4 read + 4 written, unet_in 2 written, history 4 read + 4 written = 22; the edit step adds x0 and z0
    (4 + 4 read) and one mask value per 8 elements (0.5);
    the deterministic DDIM entry reads and writes no history: 14"""
    return {"sampler": 22.0, "edit": 30.5, "cfg_ddim": 14.0}[kernel]


def child(args):
    import torch
    import ap_adapter_amd as A
    from ap_adapter_amd import ops
    if not torch.cuda.is_available():
        raise SystemExit("edit_step_time: no GPU visible; nothing is measured without one")
    dev, dtype = torch.device("cuda:0"), torch.bfloat16
    n = NPIX * C
    g = torch.Generator().manual_seed(0)
    R = lambda *s: torch.randn(*s, generator=g)
    results = {}
    for name, sched in (("dpmsolver++", A.DPMSolverMultistepScheduler()), ("ddim", A.DDIMScheduler())):
        sched.set_timesteps(STEPS)
        plan = sched.sampler_plan(0.0, start=0, masked=True)
        coef, keep = plan.table.to(dev), plan.keep.to(dev)
        eps2 = (R(2 * B, n) * 0.5).to(dev, dtype)
        lat0 = R(B, n).to(dev)
        lat, unet_in = lat0.clone(), torch.empty(B, n, dtype=dtype, device=dev)
        hist = torch.zeros(B, n, device=dev) if plan.needs_history else None
        x0, z0 = R(B, n).to(dev), R(B, n).to(dev)
        mask = (torch.rand(B, NPIX, generator=g) > 0.5).float().to(dev)
        ptr = torch.full((1,), STEPS // 2, dtype=torch.int32, device=dev)  # an interior (second-order) row
        kernels = ("sampler", "edit") + (("cfg_ddim",) if name == "ddim" else ())
        coef2 = sched.coef_table().to(dev) if name == "ddim" else None  # apad_cfg_ddim_step's two-column table

        def run(kernel, launches):
            lat.copy_(lat0)
            if hist is not None:
                hist.zero_()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(launches):
                if kernel == "cfg_ddim":
                    ops.cfg_ddim_step(eps2, lat, unet_in, coef2, ptr, 7.5)
                elif kernel == "sampler":
                    ops.cfg_sampler_step(eps2, lat, unet_in, coef, ptr, 7.5, None, hist)
                else:
                    ops.cfg_edit_step(eps2, lat, unet_in, coef, keep, ptr, 7.5, x0, z0, mask, C, None, hist)
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) * 1e3 / launches  # us per launch

        for kernel in kernels:  # warm-up: code objects loaded, buffers touched
            run(kernel, 20)
        times = {kernel: [] for kernel in kernels}
        for _ in range(args.rounds):  # alternate the kernels within every round
            for kernel in kernels:
                times[kernel].append(run(kernel, args.launches))
        results[name] = {}
        for kernel, ts in times.items():
            med = statistics.median(ts)
            no_hist = 8.0 if hist is None and kernel != "cfg_ddim" else 0.0
            results[name][kernel] = {"median_us": round(med, 3), "min_us": round(min(ts), 3), "max_us": round(max(ts), 3),
                                     "bytes_per_element_by_shape": bytes_per_element(kernel) - no_hist,
                                     "GB_per_s_at_median": round((bytes_per_element(kernel) - no_hist) * B * n / med / 1e3, 1)}
        results[name]["edit_minus_sampler_us"] = round(results[name]["edit"]["median_us"] - results[name]["sampler"]["median_us"], 3)
    out = {"what": "apad_cfg_edit_step vs apad_cfg_sampler_step (and apad_cfg_ddim_step under \"ddim\"), back-to-back launches timed with device events; medians over rounds, the "
                   "kernels alternated within each round; the working set (tens of MB) stays cache-resident across launches, so the rates are "
                   "not HBM rates",
           "not_measured": ["end-to-end edit time", "audio quality (no real weights)"],
           "device": torch.cuda.get_device_name(0), "B": B, "n": n, "C": C, "dtype": "bfloat16", "rounds": args.rounds,
           "launches_per_round": args.launches, "results": results}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "edit_step.json"))
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
