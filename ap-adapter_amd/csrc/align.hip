// Time alignment of an edit to its reference recording by an integer lag, after the vocoder and before the splice, for gfx950.
//
//   apad_align_corr    the table's hot loop: c(l) = sum over the kept samples i of r[i] e[i + l] for every lag l in [-L, L], as one partial
//                      table per (clip, chunk of 4096 samples).  Grid (chunk, clip), 256 threads.
//   apad_align_apply   per clip: the partial tables folded, the winning lag, its normalised correlation and the one of lag 0, the gate, and the
//                      shifted edit.  One 1024-thread workgroup per clip.
//
// apad_align_corr.  A workgroup stages its chunk of r (4096 floats) and the chunk's window of e (4096 + 2 L floats, zero outside the clip) in
// LDS once.  A lane owns 8 consecutive lag entries j = 8 o .. 8 o + 7 (entry j is the lag j - L) in registers; with O = ceil((2 L + 1) / 8)
// octets and P the power of two >= O, G = max(1, 256 / P) lane groups cut the chunk into G sub-chunks of 4096 / G samples, group g takes
// sub-chunk g; when O > 256 a lane takes the octets o, o + 256, .. one after the other (G = 1).  r[i] is one LDS word read by all the lanes of a
// group (a broadcast), e comes as 16-byte LDS reads of consecutive words (neighbouring lanes 32 bytes apart), and the 12-word window of e a
// lane works on slides by 4 samples per step: 2 LDS reads for 32 multiply-adds.
//
// THE SUMMATION ORDER of c(l), a function of the clip's length, its plan row alone (G follows from L):
//   1. per (chunk, sub-chunk, lag) one chain of fused multiply-adds acc = fma(r[i], e[i + l], acc) from acc = 0, over the kept samples of the
//      sub-chunk in increasing i (interval after interval): at most 4096 / G roundings;
//   2. the G sub-chunk sums of a chunk added in increasing g, starting from sub-chunk 0's: G - 1 <= 31 roundings (apad_align_corr);
//   3. the chunk sums added in increasing chunk order, starting from chunk 0's: ceil(n / 4096) - 1 roundings (apad_align_apply).
// So a term passes through at most 4096 / G + (G - 1) + ceil(n / 4096) - 1 <= 4096 + ceil(n / 4096) roundings.
// The energies of apad_align_apply: thread t of 1024 takes the samples lo + t, lo + t + 1024, .. of each kept interval in increasing order in
// one fma chain (at most ceil(|K| / 1024) + 4 roundings: an interval's last stride may be partial), then the wave's xor butterfly (6) and waves
// 0 .. 15 in order (15).
//
// No atomics, no allocation, nothing read by the host; a clip's numbers depend on the clip, its reference and its plan row alone.  The file is
// compiled without floating-point contraction and the fused multiply-adds are written out.
#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int APLAN = APAD_ALIGN_PLAN_INTS, ACHUNK = APAD_ALIGN_CHUNK, AMAXL = APAD_ALIGN_MAX_LAG, AINT = APAD_ALIGN_MAX_INTERVALS;
constexpr int CTHREADS = 256;
constexpr int EWIN = ACHUNK + 2 * AMAXL + 16;  // the window of e, and the words a lane's last octet and its read-ahead reach past it
constexpr int ATHREADS = 1024, AWAVES = ATHREADS / 64;

__device__ __forceinline__ float4 lds4(const float* p) { return *reinterpret_cast<const float4*>(p); }

// 4 samples x 8 lags: acc[t] += r[s] * w[s + t], s ascending, for the 12-word window (w0, w1, w2)
__device__ __forceinline__ void step4(float (&acc)[8], const float4 rv, const float4 w0, const float4 w1, const float4 w2) {
    const float w[12] = {w0.x, w0.y, w0.z, w0.w, w1.x, w1.y, w1.z, w1.w, w2.x, w2.y, w2.z, w2.w};
    const float r4[4] = {rv.x, rv.y, rv.z, rv.w};
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int t = 0; t < 8; ++t) acc[t] = fmaf(r4[s], w[s + t], acc[t]);
}

// One lane's 8 lags over the kept samples of [s0, s1) (chunk coordinates: sample 0 is the clip's c0), in increasing order.  Eo[i + t] is
// e[c0 + i + l_t] for the lane's lag t, Rc[i] is r[c0 + i]; both are 16-byte aligned.
__device__ __forceinline__ void accumulate(float (&acc)[8], const float* Eo, const float* Rc, const int32_t* p, int nk, int c0, int s0, int s1) {
    for (int q = 0; q < nk; ++q) {
        int i = max(p[4 + 2 * q] - c0, s0);
        const int hi = min(p[5 + 2 * q] - c0, s1);
        for (; i < hi && (i & 3); ++i) {  // up to the next multiple of 4
            const float rv = Rc[i];
#pragma unroll
            for (int t = 0; t < 8; ++t) acc[t] = fmaf(rv, Eo[i + t], acc[t]);
        }
        if (i + 4 <= hi) {
            float4 wa = lds4(Eo + i), wb = lds4(Eo + i + 4), wc;
            for (; i + 12 <= hi; i += 12) {  // the window's three registers take turns: no moves
                wc = lds4(Eo + i + 8);
                step4(acc, lds4(Rc + i), wa, wb, wc);
                wa = lds4(Eo + i + 12);
                step4(acc, lds4(Rc + i + 4), wb, wc, wa);
                wb = lds4(Eo + i + 16);
                step4(acc, lds4(Rc + i + 8), wc, wa, wb);
            }
            for (; i + 4 <= hi; i += 4) {
                wc = lds4(Eo + i + 8);
                step4(acc, lds4(Rc + i), wa, wb, wc);
                wa = wb, wb = wc;
            }
        }
        for (; i < hi; ++i) {
            const float rv = Rc[i];
#pragma unroll
            for (int t = 0; t < 8; ++t) acc[t] = fmaf(rv, Eo[i + t], acc[t]);
        }
    }
}

// grid (chunks, B), 256 threads.  plan [B][16] as include/apadapter_hip.h lays it out, checked by the host.
__global__ __launch_bounds__(CTHREADS) void align_corr_kernel(const float* __restrict__ edit, const int64_t* __restrict__ offsets,
                                                              const float* __restrict__ ref, const int64_t* __restrict__ ref_offsets,
                                                              const int32_t* __restrict__ ref_index, const int32_t* __restrict__ plan,
                                                              float* __restrict__ partial, int chunks, int lags) {
    __shared__ __attribute__((aligned(16))) float E[EWIN];
    __shared__ __attribute__((aligned(16))) float R[ACHUNK];  // the chunk of r; afterwards the sub-chunk sums [G][8 P]
    const int b = blockIdx.y, chunk = blockIdx.x, tid = threadIdx.x;
    const int32_t* p = plan + (int64_t)b * APLAN;
    const int nk = p[0], L = p[1];
    if (p[2] != 0) return;  // a given lag: nothing to measure
    const int64_t o0 = offsets[b];
    const int n = (int)(offsets[b + 1] - o0);
    const int c0 = chunk * ACHUNK;
    if (c0 >= n) return;
    const int c1 = min(c0 + ACHUNK, n), nl = 2 * L + 1;
    float* dst = partial + ((int64_t)b * chunks + chunk) * lags;
    bool any = false;
    for (int q = 0; q < nk; ++q) any |= max(p[4 + 2 * q], c0) < min(p[5 + 2 * q], c1);
    if (!any) {  // (uniform) no kept sample here
        for (int j = tid; j < nl; j += CTHREADS) dst[j] = 0.f;
        return;
    }
    const float* e = edit + o0;
    const float* r = ref + ref_offsets[ref_index[b]];
    for (int j = tid; j < ACHUNK; j += CTHREADS) R[j] = c0 + j < n ? r[c0 + j] : 0.f;
    for (int j = tid; j < EWIN; j += CTHREADS) {  // E[j] = e[c0 - L + j]
        const int i = c0 - L + j;
        E[j] = (j < ACHUNK + 2 * L && i >= 0 && i < n) ? e[i] : 0.f;
    }
    __syncthreads();

    const int O = (nl + 7) >> 3;
    int P = 8;
    while (P < O && P < CTHREADS) P <<= 1;
    const int G = CTHREADS / P, sub = ACHUNK / G;
    if (G == 1) {
        for (int o = tid; o < O; o += CTHREADS) {  // (more than one turn only when O > 256)
            float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            accumulate(acc, E + 8 * o, R, p, nk, c0, 0, c1 - c0);
#pragma unroll
            for (int t = 0; t < 8; ++t)
                if (8 * o + t < nl) dst[8 * o + t] = acc[t];
        }
        return;
    }
    const int g = tid / P, lane = tid - g * P;
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (lane < O) accumulate(acc, E + 8 * lane, R, p, nk, c0, g * sub, min(g * sub + sub, c1 - c0));
    __syncthreads();  // every group has read R
#pragma unroll
    for (int t = 0; t < 8; ++t) R[g * 8 * P + 8 * lane + t] = acc[t];
    __syncthreads();
    for (int j = tid; j < nl; j += CTHREADS) {
        float s = R[j];
        for (int k = 1; k < G; ++k) s += R[k * 8 * P + j];
        dst[j] = s;
    }
}

// a total order on (c, lag): the larger c, then the smaller |lag|, then lag >= 0
__device__ __forceinline__ bool better(float c1, int l1, float c2, int l2) {
    const int a1 = l1 < 0 ? -l1 : l1, a2 = l2 < 0 ? -l2 : l2;
    return c1 > c2 || (c1 == c2 && (a1 < a2 || (a1 == a2 && l1 > l2)));
}

// wave (xor butterfly) -> workgroup (waves 0..15 in order); both barriers are reached by every thread
__device__ __forceinline__ float block_sum16(float v, float* sh) {
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    float s = sh[0];
#pragma unroll
    for (int w = 1; w < AWAVES; ++w) s += sh[w];
    return s;
}

// grid (B), 1024 threads
__global__ __launch_bounds__(ATHREADS) void align_apply_kernel(const float* __restrict__ edit, const int64_t* __restrict__ offsets,
                                                               const float* __restrict__ ref, const int64_t* __restrict__ ref_offsets,
                                                               const int32_t* __restrict__ ref_index, const int32_t* __restrict__ plan,
                                                               const float* __restrict__ partial, const int32_t* __restrict__ lag_in,
                                                               float* __restrict__ out, int32_t* __restrict__ lags_out,
                                                               float* __restrict__ stats, float* __restrict__ corr_out, int chunks, int lags,
                                                               float min_corr) {
    __shared__ float tab[2 * AMAXL + 1];
    __shared__ float red[AWAVES];
    __shared__ int redl[AWAVES];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t o0 = offsets[b];
    const int n = (int)(offsets[b + 1] - o0);
    const float* e = edit + o0;
    float* o = out + o0;
    const int32_t* p = plan + (int64_t)b * APLAN;
    const int nk = p[0], L = p[1];
    int found, applied;
    float st[4] = {0.f, 0.f, 0.f, 0.f};
    if (p[2] == 0) {  // (uniform)
        const float* r = ref + ref_offsets[ref_index[b]];
        const int nl = 2 * L + 1, nch = (n + ACHUNK - 1) / ACHUNK;
        // (1) the chunks' tables, in increasing chunk order
        const float* pb = partial + (int64_t)b * chunks * lags;
        for (int j = tid; j < nl; j += ATHREADS) {
            float s = pb[j];
            for (int c = 1; c < nch; ++c) s += pb[(int64_t)c * lags + j];
            tab[j] = s;
            if (corr_out) corr_out[(int64_t)b * lags + j] = s;
        }
        __syncthreads();
        // (2) the winner, from (c(0), 0)
        float best = tab[L];
        int bl = 0;
        for (int j = tid; j < nl; j += ATHREADS)
            if (better(tab[j], j - L, best, bl)) best = tab[j], bl = j - L;
#pragma unroll
        for (int m = 32; m > 0; m >>= 1) {
            const float oc = __shfl_xor(best, m, 64);
            const int ol = __shfl_xor(bl, m, 64);
            if (better(oc, ol, best, bl)) best = oc, bl = ol;
        }
        if (lane == 0) red[wave] = best, redl[wave] = bl;
        __syncthreads();
        best = red[0], bl = redl[0];
#pragma unroll
        for (int w = 1; w < AWAVES; ++w)
            if (better(red[w], redl[w], best, bl)) best = red[w], bl = redl[w];
        const float c0v = tab[L];
        // (3) the energies over the kept set: reads stay inside [lo - L, hi + L), inside the clip
        float er = 0.f, ew = 0.f, ez = 0.f;
        for (int q = 0; q < nk; ++q) {
            const int lo = p[4 + 2 * q], hi = p[5 + 2 * q];
            for (int i = lo + tid; i < hi; i += ATHREADS) {
                const float rv = r[i], wv = e[i + bl], zv = e[i];
                er = fmaf(rv, rv, er), ew = fmaf(wv, wv, ew), ez = fmaf(zv, zv, ez);
            }
        }
        er = block_sum16(er, red);
        ew = block_sum16(ew, red);
        ez = block_sum16(ez, red);
        st[0] = (er == 0.f || ew == 0.f) ? 0.f : best / sqrtf(er * ew);
        st[1] = (er == 0.f || ez == 0.f) ? 0.f : c0v / sqrtf(er * ez);
        st[2] = best, st[3] = er;
        // (4) the gate
        found = bl;
        applied = (best > 0.f && st[0] >= min_corr) ? bl : 0;
    } else {
        found = applied = lag_in[b];
    }
    if (tid == 0) {
        lags_out[2 * b] = found, lags_out[2 * b + 1] = applied;
#pragma unroll
        for (int k = 0; k < 4; ++k) stats[4 * b + k] = st[k];
    }
    // (5) the shifted edit: the same bits, +0.0 where the edit does not reach
    for (int i = tid; i < n; i += ATHREADS) {
        const int64_t k = (int64_t)i + applied;
        o[i] = (k >= 0 && k < n) ? e[k] : 0.f;
    }
}

// what both entry points refuse, past their own pointers
int check(const char* who, const int64_t* offsets_host, const int64_t* ref_offsets_host, const int32_t* ref_index_host, const int32_t* plan_host,
          bool has_partial, bool has_lag_in, int batch, int n_ref, int chunks, int lags, bool* any_measured) {
    APAD_CHECK(batch > 0 && batch <= 65535 && n_ref > 0, "%s: batch %d outside [1, 65535] or n_ref %d < 1", who, batch, n_ref);
    APAD_CHECK(offsets_host[0] == 0 && ref_offsets_host[0] == 0, "%s: offsets[0] and ref_offsets[0] must be 0", who);
    *any_measured = false;
    for (int i = 0; i < batch; ++i) {
        const int64_t n = offsets_host[i + 1] - offsets_host[i];
        APAD_CHECK(n > 0 && n <= (1 << 24), "%s: clip %d has %lld samples, outside [1, 2^24]", who, i, (long long)n);
        const int ri = ref_index_host[i];
        APAD_CHECK(ri >= 0 && ri < n_ref, "%s: ref_index[%d] = %d outside [0, %d)", who, i, ri, n_ref);
        APAD_CHECK(ref_offsets_host[ri + 1] - ref_offsets_host[ri] == n, "%s: clip %d has %lld samples, its reference %d has %lld", who, i,
                   (long long)n, ri, (long long)(ref_offsets_host[ri + 1] - ref_offsets_host[ri]));
        const int32_t* p = plan_host + (int64_t)i * APLAN;
        const int nk = p[0], L = p[1], mode = p[2];
        APAD_CHECK(mode == 0 || mode == 1, "%s: clip %d: mode %d outside 0 (measured), 1 (given)", who, i, mode);
        APAD_CHECK(L >= 1 && L <= AMAXL, "%s: clip %d: L = %d outside [1, %d]", who, i, L, AMAXL);
        APAD_CHECK(nk >= 0 && nk <= AINT, "%s: clip %d has %d intervals, at most %d", who, i, nk, AINT);
        if (mode == 1) {
            APAD_CHECK(has_lag_in, "%s: clip %d: a given lag needs lag_in", who, i);
            APAD_CHECK(nk == 0, "%s: clip %d: a given lag takes no interval (%d)", who, i, nk);
            continue;
        }
        *any_measured = true;
        APAD_CHECK(nk >= 1, "%s: clip %d: a measured lag needs an interval", who, i);
        APAD_CHECK(has_partial, "%s: clip %d: a measured lag needs partial", who, i);
        APAD_CHECK(lags >= 2 * L + 1, "%s: clip %d: lags = %d is below 2 L + 1 = %d", who, i, lags, 2 * L + 1);
        APAD_CHECK((int64_t)chunks * ACHUNK >= n, "%s: clip %d: %d chunks of %d do not cover %lld samples", who, i, chunks, ACHUNK, (long long)n);
        int64_t cur = L;
        for (int q = 0; q < nk; ++q) {
            const int64_t lo = p[4 + 2 * q], hi = p[5 + 2 * q];
            APAD_CHECK(lo >= cur && lo < hi && hi <= n - L, "%s: clip %d: interval %d = [%d, %d) is empty, not behind the one before it or not "
                       "inside [L, n - L) = [%d, %lld)", who, i, q, p[4 + 2 * q], p[5 + 2 * q], L, (long long)(n - L));
            cur = hi;
        }
    }
    return 0;
}

}  // namespace

extern "C" int apad_align_corr(const float* edit, const int64_t* offsets, const int64_t* offsets_host, const float* ref, const int64_t* ref_offsets,
                               const int64_t* ref_offsets_host, const int32_t* ref_index, const int32_t* ref_index_host, const int32_t* plan,
                               const int32_t* plan_host, float* partial, int32_t batch, int32_t n_ref, int32_t chunks, int32_t lags,
                               void* stream) {
    APAD_CHECK(edit && offsets && offsets_host && ref && ref_offsets && ref_offsets_host && ref_index && ref_index_host && plan && plan_host &&
                   partial,
               "apad_align_corr: bad operands (a null pointer)");
    APAD_CHECK(chunks >= 1 && chunks <= 65535 && lags >= 1, "apad_align_corr: chunks %d outside [1, 65535] or lags %d < 1", chunks, lags);
    bool any;
    if (check("apad_align_corr", offsets_host, ref_offsets_host, ref_index_host, plan_host, true, true, batch, n_ref, chunks, lags, &any)) return -1;
    hipLaunchKernelGGL(align_corr_kernel, dim3((unsigned)chunks, (unsigned)batch), dim3(CTHREADS), 0, (hipStream_t)stream, edit, offsets, ref,
                       ref_offsets, ref_index, plan, partial, chunks, lags);
    return apad_check_launch("apad_align_corr");
}

extern "C" int apad_align_apply(const float* edit, const int64_t* offsets, const int64_t* offsets_host, const float* ref, const int64_t* ref_offsets,
                                const int64_t* ref_offsets_host, const int32_t* ref_index, const int32_t* ref_index_host, const int32_t* plan,
                                const int32_t* plan_host, const float* partial, const int32_t* lag_in, float* out, int32_t* lags_out, float* stats,
                                float* corr_out, int32_t batch, int32_t n_ref, int32_t chunks, int32_t lags, float min_corr, void* stream) {
    APAD_CHECK(edit && offsets && offsets_host && ref && ref_offsets && ref_offsets_host && ref_index && ref_index_host && plan && plan_host &&
                   out && lags_out && stats,
               "apad_align_apply: bad operands (a null pointer)");
    APAD_CHECK(out != edit && out != ref, "apad_align_apply: out must not be edit or ref");
    APAD_CHECK(chunks >= 1 && chunks <= 65535 && lags >= 1, "apad_align_apply: chunks %d outside [1, 65535] or lags %d < 1", chunks, lags);
    bool any;
    if (check("apad_align_apply", offsets_host, ref_offsets_host, ref_index_host, plan_host, partial != nullptr, lag_in != nullptr, batch, n_ref,
              chunks, lags, &any))
        return -1;
    hipLaunchKernelGGL(align_apply_kernel, dim3((unsigned)batch), dim3(ATHREADS), 0, (hipStream_t)stream, edit, offsets, ref, ref_offsets, ref_index,
                       plan, partial, lag_in, out, lags_out, stats, corr_out, chunks, lags, min_corr);
    return apad_check_launch("apad_align_apply");
}
