"""What ranking num_waveforms_per_prompt candidates costs on the GPU (profiles/clap_rank.json):

  * one pass of the CLAP audio tower at the real configuration (transformers ClapAudioConfig() widths, seeded weights) for 3 and for 96
    candidates (32 prompts x 3), with the split per launch family (device events around every C-ABI call of the pass, summed per family;
    the families' sum is below the pass time by the gaps between launches);
  * apad_window_attention at the first-stage shape (64 x 64 tokens, 4 heads) beside the per-(window, head) chain apad_gemm (Q.K^T) ->
    apad_softmax_rows (+ bias) -> apad_gemm (P.V) on the same data.  The chain is RUN for one window-row (8 windows x 4 heads of one
    sample), reported per window as measured, and EXTRAPOLATED linearly to the 64 windows x candidates of the launch it replaces -- the
    file says which number is which.  The chain here omits the shift mask and the window gather, so it is a lower bound of that route.

  * the feature extractor in front of the tower, for 3 and for 96 candidates of 10.24 s at 16 kHz: the INSTALLED transformers
    ClapFeatureExtractor (truncation="rand_trunc") on this host's CPU, on audio already resampled to 48 kHz (wall clock, one run
    for 96 candidates; the resampling, the download and the upload of the features around it are not in the figure), beside
    ap_adapter_amd.ClapFeatureExtractor on the device from the 16 kHz samples (resampling inside the launch; device events, and
    the wall clock of the whole call with its host side).  A measurement on one host, not a pass / fail.

Times are medians of ``--repeats`` timed runs after ``--warmup`` runs of the same shapes, device events around work ending in a
synchronise.  Audio quality and ranking quality are not measured (no real weights).

    python tools/clap_rank_time.py [--out profiles/clap_rank.json]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402


def seeded_(module, seed):
    with torch.no_grad():
        for i, (name, p) in enumerate(sorted(module.named_parameters(), key=lambda kv: kv[0])):
            r = torch.randn(p.shape, generator=torch.Generator().manual_seed(seed * 1000 + i))
            p.copy_(0.5 * r if "relative_position_bias_table" in name else 0.05 * r if p.dim() > 1 else 1.0 + 0.1 * r if name.endswith("weight") else 0.02 * r)
    return module


def timed(fn, warmup, repeats):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms)


FAMILIES = {"linear": "apad_gemm", "gemm": "apad_gemm", "layer_norm": "apad_layernorm", "window_attention": "apad_window_attention",
            "clap_mel2img": "apad_clap_mel2img", "gather_rows": "apad_gather_rows", "transpose_pad": "apad_transpose_pad"}


def family_split(ops, fn):
    """per-family device time and launch count of one pass: events around every wrapped ops call (linear calls gemm: counted once)"""
    events, saved, depth = [], {}, [0]
    for name, fam in FAMILIES.items():
        orig = saved[name] = getattr(ops, name)

        def wrap(*a, _orig=orig, _fam=fam, **k):
            if depth[0]:
                return _orig(*a, **k)
            depth[0] += 1
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            try:
                return _orig(*a, **k)
            finally:
                e1.record()
                events.append((_fam, e0, e1))
                depth[0] -= 1
        setattr(ops, name, wrap)
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        for name, orig in saved.items():
            setattr(ops, name, orig)
    out = {}
    for fam, e0, e1 in events:
        d = out.setdefault(fam, {"launches": 0, "ms": 0.0})
        d["launches"] += 1
        d["ms"] += e0.elapsed_time(e1)
    return {k: {"launches": v["launches"], "ms": round(v["ms"], 4)} for k, v in sorted(out.items())}


def extractor_leg(A, dev, warmup, repeats):
    """the host extractor against the device one, per candidate count"""
    import time
    from transformers.models.clap.feature_extraction_clap import ClapFeatureExtractor as Installed
    from ap_adapter_amd import frontend
    host, ours = Installed(truncation="rand_trunc"), A.ClapFeatureExtractor(truncation="rand_trunc")
    n16 = int(10.24 * 16000)
    leg = {"clip": "10.24 s: 163840 samples at 16 kHz, 491520 at 48 kHz, cropped to 480000; output [n, 1, 1001, 64]",
           "host": "transformers.ClapFeatureExtractor(truncation='rand_trunc') on 48 kHz numpy audio, wall clock",
           "device": "ap_adapter_amd.ClapFeatureExtractor on the 16 kHz device tensor (source_sampling_rate=16000), one apad_clap_logmel launch"}
    for n in (3, 96):
        wav = (0.1 * torch.randn(n, n16, generator=torch.Generator().manual_seed(n))).to(dev)
        run = lambda: ours(wav, sampling_rate=48000, source_sampling_rate=16000)
        med, best = timed(run, warmup, repeats)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run()
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        wav48 = list(frontend.resample(wav, 16000, 48000).cpu().numpy())
        host_runs = 3 if n <= 3 else 1
        secs = []
        for _ in range(host_runs):
            t0 = time.perf_counter()
            host(wav48, sampling_rate=48000, return_tensors="pt")
            secs.append(time.perf_counter() - t0)
        leg[str(n)] = {"candidates": n, "device_ms_median": round(med, 3), "device_ms_min": round(best, 3), "device_call_wall_ms": round(1e3 * wall, 3),
                       "host_s": round(statistics.median(secs), 3), "host_runs": host_runs,
                       "host_over_device": round(1e3 * statistics.median(secs) / med, 1)}
    leg["host_torch_threads"] = torch.get_num_threads()
    return leg


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "clap_rank.json"))
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=9)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("clap_rank_time: needs the GPU (a CPU run measures nothing)")
    import ap_adapter_amd as A
    from ap_adapter_amd import ops
    dev = torch.device("cuda:0")
    tower = seeded_(A.ClapAudioModelWithProjection(), 42).to(dev)
    res = {"device": torch.cuda.get_device_name(0), "config": "transformers.ClapAudioConfig() defaults, seeded weights, fp32, input [n, 1, 1001, 64]",
           "warmup": args.warmup, "repeats": args.repeats, "tower": {}}
    for n in (3, 96):
        x = torch.randn(n, 1, 1001, 64, generator=torch.Generator().manual_seed(n)).to(dev)
        run = lambda: tower.get_audio_features(x)
        med, best = timed(run, args.warmup, args.repeats)
        res["tower"][str(n)] = {"candidates": n, "pass_ms_median": round(med, 3), "pass_ms_min": round(best, 3), "families": family_split(ops, run)}

    # the first-stage shape: 64 x 64 tokens, 4 heads of 24, for 3 candidates
    B, H, W, heads, C = 3, 64, 64, 4, 96
    g = torch.Generator().manual_seed(5)
    qkv = (torch.randn(B * H * W, 3 * C, generator=g) * 2.2).to(dev)
    bias = torch.randn(heads, 64, 64, generator=g).to(dev)
    out = torch.empty(B * H * W, C, device=dev)
    wa = {}
    for shift in (0, 4):
        med, best = timed(lambda: ops.window_attention(qkv, bias, B, H, W, heads, shift, out=out), args.warmup, args.repeats)
        wa[f"shift{shift}_ms_median"], wa[f"shift{shift}_ms_min"] = round(med, 4), round(best, 4)
    n_win = B * (H // 8) * (W // 8)
    wa["windows"], wa["per_window_us_shift0"] = n_win, round(1e3 * wa["shift0_ms_median"] / n_win, 4)
    # the chain on one window-row: 8 windows x 4 heads; rows of a window contiguous (the gather is not part of what is timed)
    rows = qkv[: 8 * 64].view(8, 64, 3 * C)
    vt = rows[:, :, 2 * C:].reshape(8, 64, heads, 24).permute(0, 2, 3, 1).contiguous()  # [window, head, 24, 64]
    s = torch.empty(64, 64, device=dev)
    o = torch.empty(8 * 64, C, device=dev)

    def chain():
        for w in range(8):
            r = rows[w]
            for h in range(heads):
                ops.gemm(r[:, h * 24:], r[:, C + h * 24:], M=64, N=64, K=24, lda=3 * C, ldw=3 * C, out=s, ldo=64, exact=True)
                ops.softmax_rows(s, 1.0 / 24 ** 0.5, out=s, bias=bias[h])
                ops.gemm(s, vt[w, h], M=64, N=24, K=64, lda=64, ldw=64, out=o[w * 64:, h * 24:], ldo=C, exact=True)

    med, best = timed(chain, args.warmup, args.repeats)
    ref = torch.empty(8 * 64, C, device=dev)
    per_win = med / 8
    res["window_attention"] = dict(shape=f"B={B} {H}x{W} tokens, {heads} heads of 24, fp32", **wa)
    res["chain"] = {"what": "apad_gemm -> apad_softmax_rows(+bias) -> apad_gemm per (window, head), no shift mask, no window gather",
                    "measured": {"windows": 8, "heads": heads, "launches": 8 * heads * 3, "ms_median": round(med, 4), "ms_min": round(best, 4),
                                 "per_window_us": round(1e3 * per_win, 3)},
                    "extrapolated": {"windows": n_win, "launches": n_win * heads * 3, "ms": round(per_win * n_win, 2),
                                     "note": "per-window time of the measured window-row x the windows of the launch above (linear; not run)"}}
    res["ratio_chain_extrapolated_over_kernel"] = round(per_win * n_win / wa["shift0_ms_median"], 1)
    # same arithmetic: the chain's output equals the kernel's on the same windows (window-major data as a 64 x 8 strip is one window per 8 rows)
    strip = rows.reshape(8, 8, 8, 3 * C).permute(1, 0, 2, 3).reshape(8 * 64, 3 * C).contiguous()  # windows side by side: [8 rows][8 windows * 8][3C]
    ops.window_attention(strip, bias, 1, 8, 64, heads, 0, out=ref)
    back = ref.view(8, 8, 8, C).permute(1, 0, 2, 3).reshape(8 * 64, C)
    res["chain"]["max_abs_diff_vs_kernel"] = float((back - o).abs().max())
    res["feature_extractor"] = extractor_leg(A, dev, args.warmup, args.repeats)
    res["not_measured"] = "audio quality and ranking quality (no real weights)"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
