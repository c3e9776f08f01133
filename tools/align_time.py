"""What the alignment stage costs on the GPU (profiles/align.json): for 3 and for 96 candidates of 10.24 s at 16 kHz (163840 samples), one
region of 3 s with the pipeline's defaults (the splice's kept set, a search of +-20 ms: L = 320, 641 lags), the two launches --
apad_align_corr, the (chunk, clip) grid of the correlation table, and apad_align_apply, the fold, the winner, the energies and the shifted
copy -- each alone, beside the vocoder call that produces such a batch (the full-size SpeechT5HifiGan, random weights, bf16: the stage's
time is to be read as a fraction of it), and beside the same correlation through torch's FFT in fp32 on this host's CPU (--threads
threads).  As arithmetic, not a measurement: the 112000 kept samples times 641 lags are 72 M multiply-adds per clip, 6.9 G for 96 (105 M and
10 G were the whole clip kept).

Times are medians of ``--repeats`` timed runs after ``--warmup`` runs of the same shapes: device events around work ending in a
synchronise on the GPU, wall clock on the CPU.  A measurement on one host, not a pass / fail.  Not measured: the lag real AudioLDM2
weights produce, whether it is constant over a clip, useful values of the two defaults (no real weights, no real recordings).

    python tools/align_time.py [--out profiles/align.json]
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


def host_lags(e, r, kept, L):
    """the table through torch's FFT in fp32 on the CPU for a rectangular batch [b, n] sharing one kept set -> the arg-max lag per clip.
    c(l) = sum_K r[i] e[i + l]: the cross-correlation of r masked to K with e"""
    n = e.shape[1]
    rk = torch.zeros_like(r)
    for lo, hi in kept:
        rk[:, lo:hi] = r[:, lo:hi]
    size = 1 << (2 * n - 1).bit_length()
    c = torch.fft.irfft(torch.fft.rfft(e, size) * torch.fft.rfft(rk, size).conj(), size)
    table = torch.cat([c[:, size - L:], c[:, :L + 1]], 1)  # lags -L .. L
    return table.argmax(1) - L


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "align.json"))
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--threads", type=int, default=16)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("align_time: needs the GPU (a CPU run measures nothing)")
    import ap_adapter_amd as A
    from ap_adapter_amd import align, ops, splice
    torch.set_num_threads(args.threads)
    dev = torch.device("cuda:0")
    n16 = int(10.24 * 16000)
    W, M = splice.check_lengths(16000, 0.03, 0.08)
    L, min_corr, _ = align.check_arguments(16000, "kept", 0.02, 0.5)
    plan = align.plan(n16, splice.plan(n16, [(4 * 16000, 7 * 16000)], W, M).kept, L)
    kept_samples = sum(hi - lo for lo, hi in plan.kept)
    chunks, nl, lag = -(-n16 // align.CHUNK), 2 * L + 1, 57
    torch.manual_seed(0)
    voc = A.SpeechT5HifiGan(A.HifiGanConfig()).to(dev, torch.bfloat16)
    frames = n16 // 160
    res = {"device": torch.cuda.get_device_name(0),
           "clip": f"10.24 s: {n16} samples at 16 kHz, one region [4 s, 7 s), the splice's kept set shrunk by L = {L}: {kept_samples} samples in "
                   f"{len(plan.kept)} intervals, {nl} lags, {chunks} chunks; every edit is its recording {lag} samples late plus noise",
           "multiply_adds_per_clip": kept_samples * nl,
           "warmup": args.warmup, "repeats": args.repeats, "host_threads": args.threads,
           "device_times": "apad_align_corr and apad_align_apply on n candidates of one recording, each alone and back to back; the vocoder call "
                           "that renders n candidates (bf16, random weights); all by device events",
           "host_times": "the same table through torch.fft in fp32 on the CPU with host_threads threads and its arg-max, wall clock"}
    for n in (3, 96):
        g = torch.Generator().manual_seed(n)
        long = 0.1 * torch.randn(1, n16 + lag, generator=g)
        ref = long[:, lag:].contiguous()
        wav = 0.6 * long[:, :n16] + 0.02 * torch.randn(n, n16, generator=g)  # wav[i + lag] ~ 0.6 ref[i]
        e, r = wav.reshape(-1).to(dev), ref.reshape(-1).to(dev)
        oh, roh = torch.arange(n + 1, dtype=torch.int64) * n16, torch.tensor([0, n16], dtype=torch.int64)
        od, rod = oh.to(dev), roh.to(dev)
        ih = torch.zeros(n, dtype=torch.int32)
        ph = torch.tensor([align.plan_row(plan)] * n, dtype=torch.int32)
        idd, pd = ih.to(dev), ph.to(dev)
        partial, out = torch.empty(n, chunks, nl, device=dev), torch.empty(n * n16, device=dev)
        lags, stats = torch.empty(n, 2, dtype=torch.int32, device=dev), torch.empty(n, 4, device=dev)
        corr = lambda: ops.align_corr(e, od, oh, r, rod, roh, idd, ih, pd, ph, partial)
        apply = lambda: ops.align_apply(e, od, oh, r, rod, roh, idd, ih, pd, ph, out, lags, stats, min_corr, partial=partial)
        c_med, c_min = timed(corr, args.warmup, args.repeats)
        a_med, a_min = timed(apply, args.warmup, args.repeats)
        b_med, b_min = timed(lambda: (corr(), apply()), args.warmup, args.repeats)
        mel = torch.randn(n, frames, voc.config.model_in_dim, generator=torch.Generator().manual_seed(7)).to(dev, torch.bfloat16)
        with torch.no_grad():
            v_med, v_min = timed(lambda: voc(mel), 2, args.repeats)
        rb = ref.expand(n, n16).contiguous()
        h_med, h_min = timed_host(lambda: host_lags(wav, rb, plan.kept, L), 1, args.repeats)
        hl = host_lags(wav, rb, plan.kept, L)
        res[str(n)] = {"candidates": n,
                       "align_corr_ms_median": round(c_med, 4), "align_corr_ms_min": round(c_min, 4),
                       "align_apply_ms_median": round(a_med, 4), "align_apply_ms_min": round(a_min, 4),
                       "both_ms_median": round(b_med, 4), "both_ms_min": round(b_min, 4),
                       "align_corr_gflops": round(2e-6 * n * kept_samples * nl / c_med, 1),
                       "vocoder_ms_median": round(v_med, 3), "vocoder_ms_min": round(v_min, 3),
                       "stage_fraction_of_vocoder": round(b_med / v_med, 5),
                       "host_fft_fp32_torch_ms_median": round(h_med, 3), "host_fft_fp32_torch_ms_min": round(h_min, 3),
                       "clip0_lags": lags[0].tolist(), "clip0_ncc": [round(float(v), 6) for v in stats[0, :2]], "clip0_lag_host": int(hl[0])}
    res["not_measured"] = "the lag real AudioLDM2 weights produce, whether it is constant over a clip, useful values of align_search_s and " \
                          "align_min_corr, audibility of seams on real music (no real weights, no real recordings)"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
