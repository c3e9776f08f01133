"""What the splice stage costs on the GPU (profiles/splice.json): for 3 and for 96 candidates of 10.24 s at 16 kHz (163840 samples), one
region of 3 s with the pipeline's defaults (a 30 ms crossfade, W = 480; an 80 ms search margin, M = 1280: 801 candidates per seam), the
one launch -- apad_splice: the gain over the kept part, two seam searches, the output -- beside the vocoder call that produces such a batch
(the full-size SpeechT5HifiGan, random weights, bf16: the stage's time is to be read as a fraction of it), and beside the same arithmetic
in fp32 torch on this host's CPU (--threads threads: the gain, each seam's costs as a sliding sum of squared differences and their
arg-min, the correlation, the crossfade and the copy).

Times are medians of ``--repeats`` timed runs after ``--warmup`` runs of the same shapes: device events around work ending in a
synchronise on the GPU, wall clock on the CPU.  A measurement on one host, not a pass / fail.  Not measured: audio quality, whether a
seam is audible on real music, whether the vocoder's output is time-aligned with a recording closely enough (no real weights, no real
recordings).

    python tools/splice_time.py [--out profiles/splice.json]
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


def host_splice(e, r, plan):
    """the stage's arithmetic in fp32 torch on the CPU for a rectangular batch [b, n] sharing one plan (one region): not bit-equal to the
    kernel (torch's own summation order), the same work"""
    W = plan.W
    (a, b), (left, right) = plan.regions[0], plan.seams[0]
    kept = torch.cat([torch.arange(lo, hi) for lo, hi in plan.kept])
    g = torch.sqrt((r[:, kept] ** 2).sum(1) / (e[:, kept] ** 2).sum(1))
    ge = g[:, None] * e
    out = r.clone()
    starts = []
    for side, (lo, hi) in enumerate((left, right)):
        d2 = (r[:, lo:hi] - ge[:, lo:hi]) ** 2
        cost = d2.unfold(1, W, 1).sum(2)
        starts.append(lo + (cost.flip(1).argmin(1).neg() + cost.shape[1] - 1 if side == 0 else cost.argmin(1)))
    t = (torch.arange(W, dtype=torch.float32) + 0.5) / W
    for i in range(e.shape[0]):
        sl, sr = int(starts[0][i]), int(starts[1][i])
        out[i, sl + W:sr] = ge[i, sl + W:sr]
        for s, we in ((sl, t), (sr, 1 - t)):
            rw, gw = r[i, s:s + W], ge[i, s:s + W]
            rho = ((rw * gw).sum() / torch.sqrt((rw * rw).sum() * (gw * gw).sum())).clamp(0, 1)
            wr = 1 - we
            out[i, s:s + W] = (wr * rw + we * gw) / torch.sqrt(wr * wr + we * we + 2 * rho * wr * we)
    return out, g, starts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "splice.json"))
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--threads", type=int, default=16)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("splice_time: needs the GPU (a CPU run measures nothing)")
    import ap_adapter_amd as A
    from ap_adapter_amd import ops, splice
    torch.set_num_threads(args.threads)
    dev = torch.device("cuda:0")
    n16 = int(10.24 * 16000)
    W, M = splice.check_lengths(16000, 0.03, 0.08)
    plan = splice.plan(n16, [(4 * 16000, 7 * 16000)], W, M)
    torch.manual_seed(0)
    voc = A.SpeechT5HifiGan(A.HifiGanConfig()).to(dev, torch.bfloat16)
    frames = n16 // 160
    res = {"device": torch.cuda.get_device_name(0),
           "clip": f"10.24 s: {n16} samples at 16 kHz, one region [4 s, 7 s), W = {W}, M = {M}: {M - W + 1} candidates per seam, 2 seams",
           "warmup": args.warmup, "repeats": args.repeats, "host_threads": args.threads,
           "device_times": "apad_splice on n candidates of one recording; the vocoder call that renders n candidates (bf16, random weights), "
                           "all by device events",
           "host_times": "the same arithmetic in fp32 torch on the CPU with host_threads threads, wall clock"}
    for n in (3, 96):
        g = torch.Generator().manual_seed(n)
        ref = 0.1 * torch.randn(1, n16, generator=g)
        wav = 0.6 * ref + 0.05 * torch.randn(n, n16, generator=g)
        e, r = wav.reshape(-1).to(dev), ref.reshape(-1).to(dev)
        oh, roh = torch.arange(n + 1, dtype=torch.int64) * n16, torch.tensor([0, n16], dtype=torch.int64)
        od, rod = oh.to(dev), roh.to(dev)
        ih = torch.zeros(n, dtype=torch.int32)
        ph = torch.tensor([splice.plan_row(plan)] * n, dtype=torch.int32)
        idd, pd = ih.to(dev), ph.to(dev)
        out, gains = torch.empty(n * n16, device=dev), torch.empty(n, device=dev)
        starts, stats = torch.empty(n, 8, dtype=torch.int32, device=dev), torch.empty(n, 8, 2, device=dev)
        s_med, s_min = timed(lambda: ops.splice(e, od, oh, r, rod, roh, idd, ih, pd, ph, out, gains, starts, stats), args.warmup, args.repeats)
        mel = torch.randn(n, frames, voc.config.model_in_dim, generator=torch.Generator().manual_seed(7)).to(dev, torch.bfloat16)
        with torch.no_grad():
            v_med, v_min = timed(lambda: voc(mel), 2, args.repeats)
        rb = ref.expand(n, n16).contiguous()
        h_med, h_min = timed_host(lambda: host_splice(wav, rb, plan), 1, args.repeats)
        _, hg, hs = host_splice(wav, rb, plan)
        res[str(n)] = {"candidates": n,
                       "splice_ms_median": round(s_med, 4), "splice_ms_min": round(s_min, 4),
                       "vocoder_ms_median": round(v_med, 3), "vocoder_ms_min": round(v_min, 3),
                       "stage_fraction_of_vocoder": round(s_med / v_med, 5),
                       "host_fp32_torch_ms_median": round(h_med, 3), "host_fp32_torch_ms_min": round(h_min, 3),
                       "clip0_gain": round(float(gains[0]), 6), "clip0_gain_host": round(float(hg[0]), 6),
                       "clip0_starts": starts[0, :2].tolist(), "clip0_starts_host": [int(hs[0][0]), int(hs[1][0])]}
    res["not_measured"] = "audio quality, whether a seam is audible on real music, whether the vocoder's output is time-aligned with a recording " \
                          "closely enough for a sample-domain splice (no real weights, no real recordings)"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
