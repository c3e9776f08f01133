// Splice of a region edit back into its reference recording, after the vocoder, for gfx950.
//
//   apad_splice   per clip: the gain that matches the edit to the reference on the kept part, each seam's best window (least squared
//                 difference between reference and gained edit over W samples, searched over the seam's span), the windows' correlation, and
//                 the output: the reference's own bits outside regions and windows, the gained edit inside a region, a power-complementary
//                 crossfade for signals of that correlation in each window.  One launch for a ragged batch.
//
// One workgroup owns a clip and runs three phases in order.  (1) sum r^2 and sum e^2 over the kept intervals: thread t takes samples t, t + 1024, ..
// of each interval in increasing order, then lane -> wave -> workgroup.  (2) per seam: d = r - g e of the search span goes to LDS (8192 floats
// at the most); lane c sums d^2 over the W consecutive entries of candidate c in index order -- neighbouring lanes read neighbouring words,
// no bank conflict -- and the (cost, start) pairs are reduced by a total order (smaller cost, then the start nearer the region), so the
// minimum does not depend on the order of the reduction.  (3) every sample of the clip is written once.  No atomics, no allocation, nothing
// read by the host: a clip's numbers depend on the clip, its reference and its plan alone.
//
// Every product that the interface states as one rounding is one: the file is compiled without floating-point contraction and the fused
// multiply-adds are written out.
#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int STHREADS = 1024, SWAVES = STHREADS / 64;
constexpr int SMAXSPAN = APAD_SPLICE_MAX_SPAN;  // samples of one seam's search span held in LDS
constexpr int SPLAN = APAD_SPLICE_PLAN_INTS, SREG = APAD_SPLICE_MAX_REGIONS;

// wave (xor butterfly) -> workgroup (waves 0..15 in order); both barriers are reached by every thread
__device__ __forceinline__ float block_sum16(float v, float* sh) {
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    float s = sh[0];
#pragma unroll
    for (int w = 1; w < SWAVES; ++w) s += sh[w];
    return s;
}

// a total order on (cost, start): the smaller cost, then the start nearer the region (the larger one on a left seam)
__device__ __forceinline__ bool better(float c1, int s1, float c2, int s2, bool left) {
    return c1 < c2 || (c1 == c2 && (left ? s1 > s2 : s1 < s2));
}

// grid (B), 1024 threads.  plan [B][32] as include/apadapter_hip.h lays it out, checked by the host.
__global__ __launch_bounds__(STHREADS) void splice_kernel(const float* __restrict__ edit, const int64_t* __restrict__ offsets,
                                                          const float* __restrict__ ref, const int64_t* __restrict__ ref_offsets,
                                                          const int32_t* __restrict__ ref_index, const int32_t* __restrict__ plan,
                                                          const float* __restrict__ gain_in, float* __restrict__ out,
                                                          float* __restrict__ gains, int32_t* __restrict__ seam_start,
                                                          float* __restrict__ seam_stats) {
    __shared__ float d[SMAXSPAN];
    __shared__ float red[SWAVES];
    __shared__ int reds[SWAVES];
    __shared__ int win[2 * SREG];    // the chosen window starts, -1 = no seam
    __shared__ float rho[2 * SREG];  // the correlation each crossfade uses
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t o0 = offsets[b];
    const int n = (int)(offsets[b + 1] - o0);
    const float* e = edit + o0;
    const float* r = ref + ref_offsets[ref_index[b]];
    float* o = out + o0;
    const int32_t* p = plan + (int64_t)b * SPLAN;
    const int nreg = p[0], W = p[1], shape = p[2];

    // (1) the gain over the kept intervals: before the first span, between spans, after the last
    float g = 1.f;
    if (p[3] == 0) {
        float sr = 0.f, se = 0.f;
        int cur = 0;
        for (int q = 0; q <= nreg; ++q) {
            const int32_t* pr = p + 8 + 6 * q;
            const int end = q < nreg ? (pr[2] >= 0 ? pr[2] : 0) : n;
            for (int i = cur + tid; i < end; i += STHREADS) {
                const float rv = r[i], ev = e[i];
                sr = fmaf(rv, rv, sr), se = fmaf(ev, ev, se);
            }
            if (q < nreg) cur = pr[4] >= 0 ? pr[5] : n;
        }
        sr = block_sum16(sr, red);
        se = block_sum16(se, red);
        if (sr > 0.f && se > 0.f && isfinite(sr) && isfinite(se)) g = sqrtf(sr / se);
    } else {
        g = gain_in[b];
    }

    // (2) the seams: 2 q = the left seam of region q, 2 q + 1 its right seam
    for (int k = 0; k < 2 * SREG; ++k) {
        const int q = k >> 1;
        const bool left = !(k & 1);
        const int lo = q < nreg ? p[8 + 6 * q + (left ? 2 : 4)] : -1;
        float cost = 0.f, corr = 0.f;
        int s = -1;
        if (lo >= 0) {  // (uniform over the workgroup)
            const int hi = p[8 + 6 * q + (left ? 3 : 5)], C = hi - lo - W + 1;
            __syncthreads();  // the seam before this one has read d
            for (int j = tid; j < hi - lo; j += STHREADS) d[j] = r[lo + j] - g * e[lo + j];
            __syncthreads();
            cost = INFINITY, s = left ? hi - W : lo;
            for (int c = tid; c < C; c += STHREADS) {
                float acc = 0.f;
                for (int j = 0; j < W; ++j) acc = fmaf(d[c + j], d[c + j], acc);
                if (better(acc, lo + c, cost, s, left)) cost = acc, s = lo + c;
            }
#pragma unroll
            for (int m = 32; m > 0; m >>= 1) {
                const float oc = __shfl_xor(cost, m, 64);
                const int os = __shfl_xor(s, m, 64);
                if (better(oc, os, cost, s, left)) cost = oc, s = os;
            }
            if (lane == 0) red[wave] = cost, reds[wave] = s;
            __syncthreads();
            cost = red[0], s = reds[0];
#pragma unroll
            for (int w = 1; w < SWAVES; ++w)
                if (better(red[w], reds[w], cost, s, left)) cost = red[w], s = reds[w];
            // the correlation of reference and gained edit over the chosen window
            float a = 0.f, rr = 0.f, gg = 0.f;
            for (int j = tid; j < W; j += STHREADS) {
                const float rv = r[s + j], gv = g * e[s + j];
                a = fmaf(rv, gv, a), rr = fmaf(rv, rv, rr), gg = fmaf(gv, gv, gg);
            }
            a = block_sum16(a, red);
            rr = block_sum16(rr, red);
            gg = block_sum16(gg, red);
            if (rr > 0.f && gg > 0.f) corr = fminf(fmaxf(a / sqrtf(rr * gg), 0.f), 1.f);
        }
        if (tid == 0) {
            win[k] = s;
            rho[k] = shape == 1 ? 1.f : shape == 2 ? 0.f : corr;
            seam_start[(int64_t)b * 2 * SREG + k] = s;
            seam_stats[((int64_t)b * 2 * SREG + k) * 2] = cost;
            seam_stats[((int64_t)b * 2 * SREG + k) * 2 + 1] = corr;
        }
    }
    if (tid == 0) gains[b] = g;
    __syncthreads();

    // (3) the output: the reference's bits, the gained edit between a region's windows, the crossfade inside a window
    const float fw = (float)W;
    for (int i = tid; i < n; i += STHREADS) {
        const float rv = r[i];
        float v = rv;
        for (int q = 0; q < nreg; ++q) {
            const int sl = win[2 * q], sr = win[2 * q + 1];
            const int from = sl >= 0 ? sl + W : 0, to = sr >= 0 ? sr : n;
            if (i >= from && i < to) {
                v = g * e[i];
            } else if ((sl >= 0 && i >= sl && i < from) || (sr >= 0 && i >= to && i < to + W)) {
                const bool lft = i < from;
                const float t = ((float)(i - (lft ? sl : sr)) + 0.5f) / fw;
                const float we = lft ? t : 1.f - t, wr = 1.f - we, c = rho[2 * q + (lft ? 0 : 1)];
                const float num = fmaf(wr, rv, we * (g * e[i]));
                const float den = sqrtf(fmaf(2.f * c * wr, we, fmaf(wr, wr, we * we)));
                v = num / den;
            }
        }
        o[i] = v;
    }
}

}  // namespace

extern "C" int apad_splice(const float* edit, const int64_t* offsets, const int64_t* offsets_host, const float* ref, const int64_t* ref_offsets,
                           const int64_t* ref_offsets_host, const int32_t* ref_index, const int32_t* ref_index_host, const int32_t* plan,
                           const int32_t* plan_host, const float* gain_in, float* out, float* gains, int32_t* seam_start, float* seam_stats,
                           int32_t batch, int32_t n_ref, void* stream) {
    APAD_CHECK(edit && offsets && offsets_host && ref && ref_offsets && ref_offsets_host && ref_index && ref_index_host && plan && plan_host &&
                   out && gains && seam_start && seam_stats,
               "apad_splice: bad operands (a null pointer)");
    APAD_CHECK(batch > 0 && batch <= 65535 && n_ref > 0, "apad_splice: batch %d outside [1, 65535] or n_ref %d < 1", batch, n_ref);
    APAD_CHECK(out != edit && out != ref, "apad_splice: out must not be edit or ref");
    APAD_CHECK(offsets_host[0] == 0 && ref_offsets_host[0] == 0, "apad_splice: offsets[0] and ref_offsets[0] must be 0");
    for (int i = 0; i < batch; ++i) {
        const int64_t n = offsets_host[i + 1] - offsets_host[i];
        APAD_CHECK(n > 0 && n <= (1 << 30), "apad_splice: clip %d has %lld samples, outside [1, 2^30]", i, (long long)n);
        const int ri = ref_index_host[i];
        APAD_CHECK(ri >= 0 && ri < n_ref, "apad_splice: ref_index[%d] = %d outside [0, %d)", i, ri, n_ref);
        APAD_CHECK(ref_offsets_host[ri + 1] - ref_offsets_host[ri] == n, "apad_splice: clip %d has %lld samples, its reference %d has %lld", i,
                   (long long)n, ri, (long long)(ref_offsets_host[ri + 1] - ref_offsets_host[ri]));
        const int32_t* p = plan_host + (int64_t)i * SPLAN;
        const int nreg = p[0], W = p[1], shape = p[2], M = p[4];
        APAD_CHECK(nreg >= 1, "apad_splice: clip %d has no region", i);
        APAD_CHECK(nreg <= SREG, "apad_splice: clip %d has %d regions (%d seams), at most %d regions (%d seams)", i, nreg, 2 * nreg, SREG, 2 * SREG);
        APAD_CHECK(W >= 2, "apad_splice: clip %d: W = %d, a crossfade needs W >= 2", i, W);
        APAD_CHECK(M >= W, "apad_splice: clip %d: M = %d is below W = %d", i, M, W);
        APAD_CHECK(M <= SMAXSPAN, "apad_splice: clip %d: M = %d exceeds %d", i, M, SMAXSPAN);
        APAD_CHECK(shape >= 0 && shape <= 2, "apad_splice: clip %d: shape %d outside 0 (matched), 1 (linear), 2 (equal power)", i, shape);
        APAD_CHECK(p[3] == 0 || (p[3] == 1 && gain_in), "apad_splice: clip %d: gain mode %d needs 0 (measured), or 1 with gain_in", i, p[3]);
        int64_t cur = 0;  // where the span before this region ends
        for (int q = 0; q < nreg; ++q) {
            const int32_t* pr = p + 8 + 6 * q;
            const int64_t a = pr[0], bb = pr[1];
            APAD_CHECK(a >= cur && a < bb && bb <= n, "apad_splice: clip %d: region %d = [%d, %d) is empty, outside the clip's %lld samples or not "
                       "behind the region before it", i, q, pr[0], pr[1], (long long)n);
            if (pr[2] >= 0) {
                APAD_CHECK(pr[2] >= cur && pr[3] <= a && pr[3] - pr[2] >= W && pr[3] - pr[2] <= M, "apad_splice: clip %d: the left seam span "
                           "[%d, %d) of region %d must lie in [%lld, %d) and hold W = %d to M = %d samples", i, pr[2], pr[3], q, (long long)cur,
                           pr[0], W, M);
            } else {
                APAD_CHECK(q == 0, "apad_splice: clip %d: only the first region may go without a left seam (region %d)", i, q);
            }
            if (pr[4] >= 0) {
                APAD_CHECK(pr[4] >= bb && pr[5] <= n && pr[5] - pr[4] >= W && pr[5] - pr[4] <= M, "apad_splice: clip %d: the right seam span "
                           "[%d, %d) of region %d must lie in [%d, %lld) and hold W = %d to M = %d samples", i, pr[4], pr[5], q, pr[1],
                           (long long)n, W, M);
                cur = pr[5];
            } else {
                APAD_CHECK(q == nreg - 1, "apad_splice: clip %d: only the last region may go without a right seam (region %d)", i, q);
                cur = n;
            }
        }
    }
    hipLaunchKernelGGL(splice_kernel, dim3((unsigned)batch), dim3(STHREADS), 0, (hipStream_t)stream, edit, offsets, ref, ref_offsets, ref_index,
                       plan, gain_in, out, gains, seam_start, seam_stats);
    return apad_check_launch("apad_splice");
}
