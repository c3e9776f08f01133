"""Time apad_cfg_invert_step beside apad_cfg_sampler_step with a noise table (DDIM, eta = 1) at the bench geometry (B = 32 clips of 4000
latent pixels x 8 channels, bf16), in ONE process, and write the medians to profiles/invert_step.json.

    python tools/invert_step_time.py [--out profiles/invert_step.json] [--rounds 15] [--launches 200]

Two ways, both medians over the rounds: "alternating" -- the two kernels alternate launch by launch, each launch between its own pair of
device events (the event pair's own cost is in both figures) -- and "back_to_back" -- tools/edit_step_time.py's way, ``launches`` launches
of one kernel between one pair of events, the kernels alternating round by round.

This is the ONLY measurement of the inversion feature's speed: the update kernel alone, a record, not a gate.  The invert step reads one
more fp32 stream than the sampler step (x0) and writes one more (z, over the draw it read).  End to end an inversion edit costs one more
pass of the run's UNet steps -- arithmetic, not a measurement.  The timed row's kz is set to 0 so that repeated launches on one row stay
finite (z is written over the draw the next launch reads; the memory traffic is unchanged).  The GPU work runs in a child process under a
time limit; a run without a GPU fails."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, NPIX, C, STEPS, ROWS = 32, 4000, 8, 200, 4

# per latent element, bf16: eps2 2 x 2 read, latents 4 read + 4 written, unet_in 2 written, noise 4 read = 18; the invert step also reads x0
# (4) and writes z (4)
BYTES = {"sampler": 18.0, "invert": 26.0}


def child(args):
    import torch
    import ap_adapter_amd as A
    from ap_adapter_amd import ops
    if not torch.cuda.is_available():
        raise SystemExit("invert_step_time: no GPU visible; nothing is measured without one")
    dev, dtype = torch.device("cuda:0"), torch.bfloat16
    n = NPIX * C
    g = torch.Generator().manual_seed(0)
    R = lambda *s: torch.randn(*s, generator=g)
    sched = A.DDIMScheduler()
    sched.set_timesteps(STEPS)
    plan = sched.inversion_plan(1.0, start=STEPS - ROWS)  # the last ROWS rows: the noise table stays small; the kernels index one row
    coef, keep = plan.table.to(dev), plan.keep.clone()
    row = 1
    keep[row, 1] = 0.0
    keep = keep.to(dev)
    eps2 = (R(2 * B, n) * 0.5).to(dev, dtype)
    lat0, x0 = R(B, n).to(dev), R(B, n).to(dev)
    noise0 = R(ROWS, B, n).to(dev)
    lat, noise, unet_in = lat0.clone(), noise0.clone(), torch.empty(B, n, dtype=dtype, device=dev)
    ptr = torch.full((1,), row, dtype=torch.int32, device=dev)
    launch = {"sampler": lambda: ops.cfg_sampler_step(eps2, lat, unet_in, coef, ptr, 7.5, None, None, noise),
              "invert": lambda: ops.cfg_invert_step(eps2, lat, unet_in, coef, keep, x0, noise, ptr, guidance_scale=7.5)}
    kernels = ("sampler", "invert")
    ev = lambda: torch.cuda.Event(enable_timing=True)

    def reset():
        lat.copy_(lat0)
        noise.copy_(noise0)

    def back_to_back(kernel, launches):
        reset()
        e0, e1 = ev(), ev()
        e0.record()
        for _ in range(launches):
            launch[kernel]()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / launches  # us per launch

    def alternating(launches):
        reset()
        marks = [ev() for _ in range(2 * launches + 1)]
        marks[0].record()
        for i in range(launches):
            launch["sampler"]()
            marks[2 * i + 1].record()
            launch["invert"]()
            marks[2 * i + 2].record()
        torch.cuda.synchronize()
        t = [marks[j].elapsed_time(marks[j + 1]) * 1e3 for j in range(2 * launches)]
        return {"sampler": statistics.median(t[0::2]), "invert": statistics.median(t[1::2])}

    for kernel in kernels:  # warm-up: code objects loaded, buffers touched
        back_to_back(kernel, 20)
    alternating(20)
    b2b, alt = {k: [] for k in kernels}, {k: [] for k in kernels}
    for _ in range(args.rounds):
        for kernel in kernels:
            b2b[kernel].append(back_to_back(kernel, args.launches))
        a = alternating(args.launches)
        for kernel in kernels:
            alt[kernel].append(a[kernel])
    finite = bool(torch.isfinite(lat).all()) and bool(torch.isfinite(noise).all())

    def stats(ts, kernel):
        med = statistics.median(ts)
        return {"median_us": round(med, 3), "min_us": round(min(ts), 3), "max_us": round(max(ts), 3), "bytes_per_element_by_shape": BYTES[kernel],
                "GB_per_s_at_median": round(BYTES[kernel] * B * n / med / 1e3, 1)}

    results = {"back_to_back": {k: stats(b2b[k], k) for k in kernels}, "alternating": {k: stats(alt[k], k) for k in kernels}}
    for way in results:
        results[way]["invert_minus_sampler_us"] = round(results[way]["invert"]["median_us"] - results[way]["sampler"]["median_us"], 3)
    out = {"what": "apad_cfg_invert_step vs apad_cfg_sampler_step with a noise table (DDIM, eta = 1), timed with device events; medians over rounds; "
                   "back_to_back: `launches_per_round` launches of one kernel between one event pair; alternating: the kernels alternate launch by "
                   "launch, one event pair per launch (its cost included; the per-round figure is the median launch).  The working set (tens of "
                   "MB) stays cache-resident across launches, so the rates are not HBM rates",
           "not_measured": ["end-to-end inversion edit time (one extra pass of the run's UNet steps: arithmetic)", "audio quality (no real weights)",
                            "structure preservation on real music", "useful source_guidance_scale values"],
           "device": torch.cuda.get_device_name(0), "B": B, "n": n, "C": C, "dtype": "bfloat16", "rounds": args.rounds,
           "launches_per_round": args.launches, "outputs_finite": finite, "results": results}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "invert_step.json"))
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
