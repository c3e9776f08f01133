"""Record the bits the step entry points (apad_cfg_ddim_step / apad_cfg_sampler_step / apad_cfg_edit_step, and apad_cfg_dual_step) write,
on the GPU, BY RUNNING THE LIBRARY AS BUILT FROM THE COMMIT THAT IS TO BE PRESERVED:

    python tests/golden/make_step_bits.py [OUT [REVISION]]          # CASES -> tests/golden/step_bits.safetensors, or OUT
    python tests/golden/make_step_bits.py --dual [OUT [REVISION]]   # DUAL_CASES -> tests/golden/step_bits_dual.safetensors, or OUT

REVISION, the git revision the running library was built from, goes into the file's metadata ("library_revision").  The two files were
recorded from different commits, each the last one before a merge of kernels: step_bits from the three separately compiled two-branch
kernels, step_bits_dual from the three-branch kernel while it was still a copy of its own.

tests/test_gpu_step_bits.py imports CASES and run_case from here and asserts torch.equal against the file, so a later change of the
kernels (or of the compiler under them) is compared with what that commit computed, not with another kernel of the same build.  Inputs
are not stored: they come from the seeded generator R.  Every case runs STEPS steps from step 0 of a 14-step grid entered at index 4
(the multistep solver's first-order entry, then two second-order steps) at B = 3; stored are all output buffers after the last step --
the latents and the history carry every earlier step's rounding forward.

Geometries (pixels per clip, C, offset): the 16-byte form twice (B * n % 8 == 0), the scalar form by size (B * n % 8 == 4), and the scalar
form by alignment alone (the latents start one element past a 16-byte boundary).  A null mask and a mask of ones are
apad_cfg_sampler_step's bits: main() checks that at recording time and stores those bits once, under the "sampler" entry.

DUAL_CASES (entry "dual", ops.cfg_dual_step) run the same grid and geometries with three branches and a guidance table that differs on every
row and is not dyadic (the f16 rounding of the guided noise and the per-row read both show in the bits), on the multistep solver, DDIM
eta = 0.5 and DDIM eta = 0 on the six-column table (sampler_plan(0.0, dual=True)), without a mask and with a fractional one.
"""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "step_bits.safetensors")
FIXTURE_DUAL = os.path.join(HERE, "step_bits_dual.safetensors")

B, N, K, STEPS, GS = 3, 14, 4, 3, 7.5
GEOMS = {"vec": (16, 8, 0), "vec17": (17, 8, 0), "scalar": (17, 4, 0), "offset": (16, 8, 1)}
DTYPES = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}
SAMPLERS = {"dpm": ("dpm", 0.0), "ddim_eta": ("ddim", 0.5)}
MASKS = ("null", "ones", "frac-shared", "frac-clip")
# (entry, sampler, dtype, geometry, mask)
CASES = [("ddim", "ddim", d, g, "-") for d in DTYPES for g in GEOMS]
CASES += [("sampler", s, d, g, "-") for s in SAMPLERS for d in DTYPES for g in GEOMS]
CASES += [("edit", s, d, g, m) for s in SAMPLERS for d in DTYPES for g in GEOMS for m in MASKS]
DUAL_SAMPLERS = dict(SAMPLERS, ddim0=("ddim", 0.0))
DUAL_CASES = [("dual", s, d, g, m) for s in DUAL_SAMPLERS for d in DTYPES for g in GEOMS for m in ("-", "frac-shared", "frac-clip")]
# (s_A, s_T) over the full grid: two ramps, every row different, none a dyadic value
GUIDANCE = ([1.0 + 3.0 * i / (N - 1) for i in range(N)], [7.5 - 4.5 * i / (N - 1) for i in range(N)])


def R(*shape, seed=0, std=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * std


def fixture_key(case):
    """null and ones masks are stored once, as the sampler entry's bits"""
    entry, sampler, dtype, geom, mask = case
    if entry == "edit" and mask in ("null", "ones"):
        entry, mask = "sampler", "-"
    return ".".join((entry, sampler, dtype, geom, mask))


def run_case(case, dev):
    """-> {buffer name: tensor on the device} after STEPS steps"""
    import ap_adapter_amd as A
    from ap_adapter_amd import ops
    entry, sampler, dname, geom, mkind = case
    dtype = DTYPES[dname]
    npix, C, off = GEOMS[geom]
    n = npix * C
    lat = torch.empty(B * n + off, device=dev)[off:].view(B, n)  # off = 1: four bytes past the allocation's alignment
    lat.copy_(R(B, n, seed=44))
    unet_in = torch.empty(B, n, dtype=dtype, device=dev)
    eps_out = torch.empty(B, n, device=dev)
    ptr = torch.zeros(1, dtype=torch.int32, device=dev)
    hist = noise = None
    if entry == "ddim":
        sched = A.DDIMScheduler()
        sched.set_timesteps(N)
        coef = sched.coef_table()[K:].contiguous().to(dev)
    else:
        kind, eta = DUAL_SAMPLERS[sampler]
        sched = A.DPMSolverMultistepScheduler() if kind == "dpm" else A.DDIMScheduler()
        sched.set_timesteps(N)
        plan = sched.sampler_plan(eta, start=K, masked=True, dual=entry == "dual")
        coef, keep = plan.table.to(dev), plan.keep.to(dev)
        hist = torch.zeros(B, n, device=dev) if plan.needs_history else None
        noise = R(N - K, B, n, seed=9).to(dev) if eta else None
        x0, z0 = R(B, n, seed=60).to(dev), R(B, n, seed=61).to(dev)
        mask = {"-": None, "null": None, "ones": torch.ones(B, npix),
                "frac-shared": torch.rand(1, npix, generator=torch.Generator().manual_seed(3)),
                "frac-clip": torch.rand(B, npix, generator=torch.Generator().manual_seed(3))}[mkind]
        mask = None if mask is None else mask.to(dev)
        if entry == "dual":
            from ap_adapter_amd.scheduler import guidance_table
            gtab = guidance_table(*GUIDANCE, N, K).to(dev)
    for i in range(STEPS):
        eps2 = (R((3 if entry == "dual" else 2) * B, n, seed=100 + i) * 0.5).to(dev, dtype)
        if entry == "dual":
            edit = () if mask is None else (keep, x0, z0, mask, C)
            ops.cfg_dual_step(eps2, lat, unet_in, coef, gtab, ptr, eps_out, hist, noise, *edit)
        elif entry == "ddim":
            ops.cfg_ddim_step(eps2, lat, unet_in, coef, ptr, GS, eps_out)
        elif entry == "sampler":
            ops.cfg_sampler_step(eps2, lat, unet_in, coef, ptr, GS, eps_out, hist, noise)
        elif mask is None:
            ops.cfg_edit_step(eps2, lat, unet_in, coef, None, ptr, GS, None, None, None, C, eps_out, hist, noise)
        else:
            ops.cfg_edit_step(eps2, lat, unet_in, coef, keep, ptr, GS, x0, z0, mask, C, eps_out, hist, noise)
        ops.step_advance(ptr)
    out = {"latents": lat, "unet_in": unet_in, "eps_out": eps_out}
    if hist is not None:
        out["history"] = hist
    return out


def main(cases, path, revision="unknown"):
    from safetensors.torch import save_file
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    from ap_adapter_amd import _lib as L
    dev = torch.device("cuda:0")
    tensors = {}
    for case in cases:
        key = fixture_key(case)
        for name, t in run_case(case, dev).items():
            t = t.cpu().contiguous().clone()
            if key + "." + name in tensors:  # a null / ones mask: must be the sampler entry's bits already recorded
                assert torch.equal(tensors[key + "." + name], t), (case, name)
            tensors[key + "." + name] = t
    save_file(tensors, path, metadata={"generator": "tests/golden/make_step_bits.py", "device": torch.cuda.get_device_name(0),
                                          "torch": torch.__version__, "cases": str(len(cases)), "library_revision": revision,
                                          "library": os.path.basename(os.path.dirname(L.LIB_PATH)) + "/" + os.path.basename(L.LIB_PATH)})
    print("wrote", path, os.path.getsize(path), "bytes,", len(tensors), "tensors,", len(cases), "cases")


if __name__ == "__main__":
    dual = sys.argv[1:2] == ["--dual"]
    args = sys.argv[2:4] if dual else sys.argv[1:3]
    main(DUAL_CASES if dual else CASES, *(args or [FIXTURE_DUAL if dual else FIXTURE])[:2])
