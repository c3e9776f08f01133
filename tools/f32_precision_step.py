"""The fp32-storage denoise step at the bench geometry (batch 32, La 32, 10 s clip: latents 8 x 250 x 16, CFG), hipGraph-replayed, in both
fp32 matmul precisions: "highest" (exact-f32 MFMA) and "high" (bf16x3 split, APAD_F32_BF16X3).  Prints one JSON line: ms per step of each,
and the max-abs difference of the guided noise_pred of the first step between the two.  Model and inputs are bench.py's (synthetic weights,
bf16-rounded, so every mode sees the same numbers); bench.py's own line is not affected.

    python tools/f32_precision_step.py [--batch 32] [--steps 5] [--out FILE] [--only-high]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--la", type=int, default=32)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--guidance", type=float, default=9.5)
    ap.add_argument("--out", default=None, help="also append the JSON line to this file")
    ap.add_argument("--only-high", action="store_true", help="time the \"high\" step alone (a kernel-trace run of its launches)")
    args = ap.parse_args()

    import bench
    import ap_adapter_amd as A
    from ap_adapter_amd.synthetic import init_synthetic_, synthetic_inputs

    dev = torch.device("cuda:0")
    with torch.device(dev):
        unet = A.AudioLDM2UNet2DConditionModel()
        A.install_ap_adapter(unet, None, scale=0.55)
    init_synthetic_(unet, 100, on_device=True)
    unet = unet.to(dev, torch.bfloat16).to(torch.float32)  # bench.py's weights: bf16-rounded, exact in fp32
    unet.requires_grad_(False)
    inp = synthetic_inputs(args.batch, args.la, seed=0)

    legs = {}
    try:
        for prec in (("high",) if args.only_high else ("highest", "high")):
            A.set_float32_matmul_precision(prec)
            t0 = time.perf_counter()
            leg, noise_pred = bench.precision_leg(A, unet, inp, args, dev, torch.float32, steps=args.steps, graph=True)
            leg["setup_s"] = round(time.perf_counter() - t0, 1)
            legs[prec] = (leg, noise_pred)
            torch.cuda.synchronize()
    finally:
        A.set_float32_matmul_precision("highest")
    if args.only_high:
        print(json.dumps({"tool": "f32_precision_step", "device": torch.cuda.get_device_name(0), "high": legs["high"][0]}))
        return
    (hi_leg, np_highest), (x3_leg, np_high) = legs["highest"], legs["high"]
    line = {
        "tool": "f32_precision_step", "device": torch.cuda.get_device_name(0),
        "geometry": f"batch {args.batch}, La {args.la}, latents 8x250x16, CFG {args.guidance}, fp32 storage, hipGraph replay",
        "highest": hi_leg, "high": x3_leg,
        "speedup_high_vs_highest": round(hi_leg["ms_per_step"] / x3_leg["ms_per_step"], 2),
        "noise_pred_max_abs_high_vs_highest": float((np_high - np_highest).abs().max()),
        "noise_pred_max_abs": round(float(np_highest.abs().max()), 4),
        "tensor": f"guided noise_pred of the first DDIM step, batch {args.batch}",
    }
    s = json.dumps(line)
    print(s)
    if args.out:
        with open(args.out, "a") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
