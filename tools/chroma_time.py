"""What scoring edit candidates by chroma similarity costs on the GPU (profiles/chroma.json): for 3 and for 96 candidates of 10.24 s at
16 kHz (163840 samples, 321 frames), each of the two launches -- apad_chroma on the candidates, apad_chroma_similarity against one
reference per three candidates -- beside the same arithmetic restated in fp32 on this host's CPU (torch.stft + the filterbank product +
the normalisation; the cosine and the mean), torch on --threads threads.

Times are medians of ``--repeats`` timed runs after ``--warmup`` runs of the same shapes: device events around work ending in a
synchronise on the GPU, wall clock on the CPU.  A measurement on one host, not a pass / fail; audio quality is not measured.

    python tools/chroma_time.py [--out profiles/chroma.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402


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


def timed_host(fn, warmup, repeats):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        ms.append(1e3 * (time.perf_counter() - t0))
    return statistics.median(ms), min(ms)


def cpu_chroma(wav, fb, window):
    spec = torch.stft(wav, 2048, hop_length=512, window=window, center=True, pad_mode="constant", return_complex=True)  # [n, 1025, frames]
    c = torch.matmul(fb, spec.real ** 2 + spec.imag ** 2).transpose(1, 2)
    m = c.amax(dim=2, keepdim=True)
    return c / torch.where(m < 1.1754944e-38, torch.ones_like(m), m)


def cpu_similarity(a, b, idx):
    r = b[idx]
    den = torch.clamp(a.norm(dim=2) * r.norm(dim=2), min=1e-8)
    return ((a * r).sum(dim=2) / den).mean(dim=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "chroma.json"))
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--threads", type=int, default=16)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("chroma_time: needs the GPU (a CPU run measures nothing)")
    from ap_adapter_amd import chroma, ops
    torch.set_num_threads(args.threads)
    dev = torch.device("cuda:0")
    n16, T = int(10.24 * 16000), chroma.frame_count(int(10.24 * 16000))
    tabs = chroma.tables(dev)
    fb_cpu, win_cpu = tabs[2].cpu(), tabs[0].cpu()
    res = {"device": torch.cuda.get_device_name(0), "clip": f"10.24 s: {n16} samples at 16 kHz, {T} frames of 12 classes",
           "warmup": args.warmup, "repeats": args.repeats, "host_torch_threads": torch.get_num_threads(),
           "device_times": "apad_chroma on n candidates; apad_chroma_similarity of n candidates against n / 3 references (device events)",
           "host_times": "the same arithmetic in fp32 torch on the CPU (wall clock)"}
    for n in (3, 96):
        wav = 0.1 * torch.randn(n, n16, generator=torch.Generator().manual_seed(n))
        ref = 0.1 * torch.randn(n // 3, n16, generator=torch.Generator().manual_seed(1000 + n))
        x, oh = wav.reshape(-1).to(dev), torch.arange(n + 1, dtype=torch.int64) * n16
        od = oh.to(dev)
        a = torch.empty(n, T, 12, device=dev)
        b = chroma.chroma_stft(ref.to(dev))
        ih, fh = torch.arange(n, dtype=torch.int32) // 3, torch.full((n,), T, dtype=torch.int32)
        idd, fd = ih.to(dev), fh.to(dev)
        out = torch.empty(n, device=dev)
        c_med, c_min = timed(lambda: ops.chroma(x, od, oh, *tabs, a), args.warmup, args.repeats)
        s_med, s_min = timed(lambda: ops.chroma_similarity(a, b, idd, ih, fd, fh, out=out), args.warmup, args.repeats)
        hc_med, hc_min = timed_host(lambda: cpu_chroma(wav, fb_cpu, win_cpu), 1, args.repeats)
        ca, cb = cpu_chroma(wav, fb_cpu, win_cpu), cpu_chroma(ref, fb_cpu, win_cpu)
        hs_med, hs_min = timed_host(lambda: cpu_similarity(ca, cb, ih.long()), 1, args.repeats)
        res[str(n)] = {"candidates": n, "references": n // 3,
                       "chroma_ms_median": round(c_med, 4), "chroma_ms_min": round(c_min, 4),
                       "similarity_ms_median": round(s_med, 4), "similarity_ms_min": round(s_min, 4),
                       "host_chroma_ms_median": round(hc_med, 3), "host_chroma_ms_min": round(hc_min, 3),
                       "host_similarity_ms_median": round(hs_med, 3), "host_similarity_ms_min": round(hs_min, 3),
                       "max_abs_diff_chroma_vs_host": float((a.cpu() - ca).abs().max()),
                       "max_abs_diff_similarity_vs_host": float((out.cpu() - cpu_similarity(ca, cb, ih.long())).abs().max())}
    res["not_measured"] = "audio quality, structure preservation on real music (no real weights, no real recordings)"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
