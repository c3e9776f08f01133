"""What the loudness stage costs on the GPU (profiles/loudness.json): for 3 and for 96 candidates of 10.24 s at 16 kHz (163840 samples,
102 hops, 99 blocks), each of the two launches -- apad_loudness (K-weighting scan, hop energies, blocks and gates) and apad_loudness_gain
(the gain and its application) -- beside the vocoder call that produces such a batch (the full-size SpeechT5HifiGan, random weights, bf16:
the stage's time is to be read as a fraction of it), and beside the filter alone on this host's CPU: scipy.signal.sosfilt in fp64 and in
fp32, the clips spread over --threads threads (sosfilt is serial per clip and releases the GIL).

Times are medians of ``--repeats`` timed runs after ``--warmup`` runs of the same shapes: device events around work ending in a
synchronise on the GPU, wall clock on the CPU.  A measurement on one host, not a pass / fail.  Not measured: agreement with libebur128 /
pyloudnorm, true peak, anything on real music.

    python tools/loudness_time.py [--out profiles/loudness.json]
"""
import argparse
import json
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "loudness.json"))
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--threads", type=int, default=16)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("loudness_time: needs the GPU (a CPU run measures nothing)")
    from scipy.signal import sosfilt
    import ap_adapter_amd as A
    from ap_adapter_amd import loudness, ops
    dev = torch.device("cuda:0")
    n16 = int(10.24 * 16000)
    hop, _ = loudness.hop_block(16000)
    tabs = loudness.tables(dev)
    sos64 = loudness.k_weighting(16000)
    sos32 = sos64.astype(np.float32)
    torch.manual_seed(0)
    voc = A.SpeechT5HifiGan(A.HifiGanConfig()).to(dev, torch.bfloat16)
    frames = n16 // 160
    pool = ThreadPoolExecutor(args.threads)
    res = {"device": torch.cuda.get_device_name(0), "clip": f"10.24 s: {n16} samples at 16 kHz, {n16 // hop} hops, {loudness.block_count(n16)} blocks",
           "warmup": args.warmup, "repeats": args.repeats, "host_threads": args.threads,
           "device_times": "apad_loudness and apad_loudness_gain on n candidates; the vocoder call that renders n candidates (bf16, random weights), "
                           "all by device events",
           "host_times": "scipy.signal.sosfilt (the K-weighting alone, no blocks or gates) over n clips on host_threads threads, wall clock"}
    for n in (3, 96):
        wav = 0.1 * torch.randn(n, n16, generator=torch.Generator().manual_seed(n))
        x, oh = wav.reshape(-1).to(dev), torch.arange(n + 1, dtype=torch.int64) * n16
        od = oh.to(dev)
        stats, out, gains = torch.empty(n, 4, device=dev), torch.empty(n * n16, device=dev), torch.empty(n, device=dev)
        target = torch.full((n,), -14.0, device=dev)
        l_med, l_min = timed(lambda: ops.loudness(x, od, oh, *tabs, stats, hop), args.warmup, args.repeats)
        g_med, g_min = timed(lambda: ops.loudness_gain(x, od, oh, stats, out, gains, 0.891, target=target), args.warmup, args.repeats)
        mel = torch.randn(n, frames, voc.config.model_in_dim, generator=torch.Generator().manual_seed(7)).to(dev, torch.bfloat16)
        with torch.no_grad():
            v_med, v_min = timed(lambda: voc(mel), 2, args.repeats)
        clips64, clips32 = [c.numpy().astype(np.float64) for c in wav], [c.numpy() for c in wav]
        h64_med, h64_min = timed_host(lambda: list(pool.map(lambda c: sosfilt(sos64, c), clips64)), 1, args.repeats)
        h32_med, h32_min = timed_host(lambda: list(pool.map(lambda c: sosfilt(sos32, c), clips32)), 1, args.repeats)
        y = sosfilt(sos64, clips64[0])
        e = (y[: (n16 // hop) * hop].reshape(-1, hop) ** 2).sum(axis=1)
        z = np.array([e[j: j + 4].sum() / (4 * hop) for j in range(len(e) - 3)])
        L64 = -0.691 + 10 * np.log10(z[z > 0.1 * z.mean()].mean())  # (white noise at -20 dBFS: every block passes the absolute gate)
        res[str(n)] = {"candidates": n,
                       "loudness_ms_median": round(l_med, 4), "loudness_ms_min": round(l_min, 4),
                       "gain_ms_median": round(g_med, 4), "gain_ms_min": round(g_min, 4),
                       "vocoder_ms_median": round(v_med, 3), "vocoder_ms_min": round(v_min, 3),
                       "stage_fraction_of_vocoder": round((l_med + g_med) / v_med, 5),
                       "host_sosfilt_fp64_ms_median": round(h64_med, 3), "host_sosfilt_fp64_ms_min": round(h64_min, 3),
                       "host_sosfilt_fp32_ms_median": round(h32_med, 3), "host_sosfilt_fp32_ms_min": round(h32_min, 3),
                       "clip0_lufs": round(float(stats[0, 0]), 5), "clip0_lufs_host_fp64": round(float(L64), 5)}
    res["not_measured"] = "agreement with libebur128 / pyloudnorm (not installed), true peak (not implemented), anything on real music (no real " \
                          "weights, no real recordings)"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
