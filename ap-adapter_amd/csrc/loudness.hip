// Loudness after the vocoder (ITU-R BS.1770-4 integrated loudness, mono; EBU R 128 gating), for gfx950.
//
//   apad_loudness        K-weighting (high-shelf then high-pass biquad, zero initial state) -> y^2 per 100 ms hop -> 400 ms blocks ->
//                        absolute (-70 LUFS) and relative (-10 LU) gates -> LUFS, sample peak and the two block counts, one launch for a
//                        ragged batch
//   apad_loudness_gain   per-clip gain towards a target (a table, or another clip's loudness) with a sample-peak guard, out = g x
//
// The filter is a 4th-order recursion whose 38 Hz pole pair (radius 0.985 at 16 kHz) remembers for thousands of samples, so it is not cut
// into independently warmed-up pieces: each biquad is a linear recurrence s' = A s + (input terms), and the kernel scans it.  One workgroup
// owns a clip and walks it in tiles of whole hops staged through LDS.  In a tile each lane owns LRUN consecutive samples.  Per section the
// lane runs them from a ZERO state (the run's forced response z), the lanes' z are combined into every lane's true entry state with the
// host's powers of M = A^LRUN (s_(l+1) = M s_l + z_l: a Kogge-Stone scan inside the wave, a short serial carry over the 16 waves, the
// tile's carry from the one before), and the lane runs its samples again from that state.  The result is the recursion's own, up to fp32
// rounding.  Two things keep that rounding at the level of the plain serial fp32 recursion (measured against it in the tests):
//   * the high-pass runs as its numerator on the shelf's true output (w = y1[n] - 2 y1[n-1] + y1[n-2]: small for the low frequencies the
//     section removes) followed by its all-pole recursion, and only the latter is scanned.  Scanning the section in the transposed form
//     would add forced responses thousands of times larger than the state they cancel to;
//   * that all-pole state is scanned as (y[n-1], y[n-1] - y[n-2]), value and difference, with the powers in those coordinates: in
//     (y[n-1], y[n-2]) the 38 Hz mode's powers have entries near +50 and -50 that multiply two nearly equal numbers, and every product
//     rounds at 50 times the size of the result (measured: 1.2e-4 of a hop's energy against 1e-5 in these coordinates);
//   * the powers come as hi + lo fp32 pairs, so their own rounding does not enter.
// Every sum has a fixed order that depends on the clip's length and the hop alone: no atomics, nothing depends on the batch or the grid.
#include "common.h"

namespace {

constexpr int LTHREADS = 1024, LWAVES = LTHREADS / 64;
constexpr int LRUN = 8;                  // consecutive samples per lane and tile
constexpr int LSTRIDE = LRUN + 4;        // a lane's samples start 12 floats apart: its two 16-byte reads hit distinct banks in a 16-lane group;
                                         // the first two of the four spare floats carry the lane's last two shelf outputs to its neighbour
constexpr int LTILE = LTHREADS * LRUN;   // samples per tile at the most (a tile is the whole hops that fit, 16 of them at the most)
constexpr int LMAXHOPS = 3072;           // whole hops per clip the workgroup keeps in LDS (307 s at any rate)
constexpr int LPOW = 65 * 8;             // one section's powers: M^0 .. M^64, each hi[2][2] then lo[2][2]
constexpr float LABS_GATE = 1.1724653e-07f;  // 10^((-70 + 0.691) / 10): the mean square of a block at -70 LUFS

// o = (hi + lo) v for m = hi[2][2], lo[2][2] row-major: the small terms first
__device__ __forceinline__ void matvec2(const float* __restrict__ m, const float* v, float* o) {
#pragma unroll
    for (int i = 0; i < 2; ++i) o[i] = fmaf(m[2 * i + 1], v[1], fmaf(m[2 * i], v[0], fmaf(m[4 + 2 * i + 1], v[1], m[4 + 2 * i] * v[0])));
}

// the high-shelf in the transposed direct form II: c = (b0 b1 b2 a1 a2), s its two delay registers
__device__ __forceinline__ float shelf_step(float x, float* s, const float* c) {
    const float y = fmaf(c[0], x, s[0]);
    s[0] = fmaf(-c[3], y, fmaf(c[1], x, s[1]));
    s[1] = fmaf(-c[4], y, c[2] * x);
    return y;
}
// the high-pass's recursive half: y[n] = w[n] - a1 y[n-1] - a2 y[n-2], p = (y[n-1], y[n-2])
__device__ __forceinline__ float allpole_step(float w, float* p, const float* c) {
    const float y = fmaf(-c[4], p[1], fmaf(-c[3], p[0], w));
    p[1] = p[0];
    p[0] = y;
    return y;
}

__device__ __forceinline__ int lds_slot(int i) { return (i >> 3) * LSTRIDE + (i & 7); }

// v = the lane's forced response (its run from a zero state) -> the state at the lane's entry.  pw = the section's powers, pl = this
// lane's own M^(lane), zw = the waves' totals in LDS, cin = the state at the tile's entry.  Holds one barrier every thread reaches.
// DIFF: v and cin are (a, b) and the powers act on (a, a - b); the result is (a, b) again.
template <bool DIFF>
__device__ __forceinline__ void scan_entry_state(float* v, const float* __restrict__ pw, const float* pl, float (*zw)[2], const float* cin,
                                                 int lane, int wave) {
    float u[2], w[2];
    if (DIFF) v[1] = v[0] - v[1];
    // inclusive scan over the wave: v_l <- v_l + M^d v_(l - d), d = 1, 2, .., 32
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        u[0] = __shfl_up(v[0], d, 64), u[1] = __shfl_up(v[1], d, 64);
        matvec2(pw + d * 8, u, w);
        if (lane >= d) v[0] += w[0], v[1] += w[1];
    }
    if (lane == 63) zw[wave][0] = v[0], zw[wave][1] = v[1];
    // exclusive: what the lanes before this one in the wave leave, from a zero state at the wave's entry
    u[0] = __shfl_up(v[0], 1, 64), u[1] = __shfl_up(v[1], 1, 64);
    if (lane == 0) u[0] = 0.f, u[1] = 0.f;
    __syncthreads();
    float s[2] = {cin[0], DIFF ? cin[0] - cin[1] : cin[1]};  // the state at this wave's entry: the tile's carry through the waves before it
    for (int q = 0; q < wave; ++q) {
        matvec2(pw + 64 * 8, s, w);
        s[0] = w[0] + zw[q][0], s[1] = w[1] + zw[q][1];
    }
    matvec2(pl, s, w);
    v[0] = u[0] + w[0], v[1] = u[1] + w[1];
    if (DIFF) v[1] = v[0] - v[1];
}

// wave (xor butterfly) -> workgroup (waves 0..15 in order); both barriers are reached by every thread
__device__ __forceinline__ float block_sum16(float v, float* sh) {
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    float s = sh[0];
#pragma unroll
    for (int w = 1; w < LWAVES; ++w) s += sh[w];
    return s;
}

// grid (B), 1024 threads.  hpt = whole hops per tile (hpt * hop <= LTILE, hpt <= 16: wave w sums the tile's hop w).
// coef [10] = (b0 b1 b2 a1 a2) of the shelf, then of the high-pass; powers [2][65][2][2][2]: per section (the shelf's transposed-form
// transition; the high-pass's all-pole transition in (value, difference) coordinates) M^j, j = 0..64, M = A^LRUN, as hi then lo.
__global__ __launch_bounds__(LTHREADS) void loudness_kernel(const float* __restrict__ x, const int64_t* __restrict__ offsets,
                                                            const float* __restrict__ coef, const float* __restrict__ powers,
                                                            float* __restrict__ stats, float* __restrict__ hop_energy, int hop, int hpt,
                                                            int target_hops) {
    __shared__ __attribute__((aligned(16))) float tile[LTHREADS * LSTRIDE];
    __shared__ float energy[LMAXHOPS];
    __shared__ float zws[LWAVES][2], zwp[LWAVES][2], carry[2][6], red[LWAVES];  // carry: shelf state, last two shelf outputs, all-pole state
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t o0 = offsets[b], n = offsets[b + 1] - o0;
    const float* xc = x + o0;
    const int tlen = hpt * hop;
    const int64_t ntiles = (n + tlen - 1) / tlen, whole = n / hop;

    float c[10], pls[8], plp[8];
#pragma unroll
    for (int i = 0; i < 10; ++i) c[i] = coef[i];
#pragma unroll
    for (int i = 0; i < 8; ++i) pls[i] = powers[lane * 8 + i], plp[i] = powers[LPOW + lane * 8 + i];
    if (tid < 6) carry[0][tid] = 0.f;  // zero initial state; the first read comes after the tile's first barrier

    float peak = 0.f, r[LRUN];
#pragma unroll
    for (int k = 0; k < LRUN; ++k) {
        const int i = tid + k * LTHREADS;
        r[k] = (i < tlen && (int64_t)i < n) ? xc[i] : 0.f;
    }
    for (int64_t t = 0; t < ntiles; ++t) {
        const int64_t t0 = t * tlen;
        const int valid = (int)(n - t0 < (int64_t)tlen ? n - t0 : (int64_t)tlen);
        const float* cin = carry[t & 1];
        float* cout = carry[(t + 1) & 1];
#pragma unroll
        for (int k = 0; k < LRUN; ++k) {  // coalesced: thread tid holds samples tid, tid + 1024, ..; zeros past the tile or the clip
            tile[lds_slot(tid + k * LTHREADS)] = r[k];
            peak = fmaxf(peak, fabsf(r[k]));
        }
        __syncthreads();
        if (t + 1 < ntiles) {  // the next tile's samples travel while this one is filtered
#pragma unroll
            for (int k = 0; k < LRUN; ++k) {
                const int i = tid + k * LTHREADS;
                const int64_t g = t0 + tlen + i;
                r[k] = (i < tlen && g < n) ? xc[g] : 0.f;
            }
        }
        float* mine = tile + tid * LSTRIDE;
        float v[LRUN];
        {
            const f32x4 lo = *reinterpret_cast<const f32x4*>(mine), hi = *reinterpret_cast<const f32x4*>(mine + 4);
#pragma unroll
            for (int k = 0; k < 4; ++k) v[k] = lo[k], v[4 + k] = hi[k];
        }
        // the lane that holds the tile's last sample hands every state on as it is after exactly that sample
        const int cnt = valid - tid * LRUN;
        const bool last = cnt >= 1 && cnt <= LRUN;
        // shelf: the run from a zero state, the scan, the run from the true state; v becomes the shelf's output
        float s[2] = {0.f, 0.f};
#pragma unroll
        for (int k = 0; k < LRUN; ++k) shelf_step(v[k], s, c);
        scan_entry_state<false>(s, powers, pls, zws, cin, lane, wave);
#pragma unroll
        for (int k = 0; k < LRUN; ++k) {
            v[k] = shelf_step(v[k], s, c);
            if (last && k + 1 == cnt) cout[0] = s[0], cout[1] = s[1];
        }
        mine[LRUN] = v[LRUN - 1], mine[LRUN + 1] = v[LRUN - 2];
        __syncthreads();
        // high-pass numerator on the true shelf output (the two samples before the lane's first: its neighbour's last, or the carry)
        float q1 = tid ? mine[LRUN - LSTRIDE] : cin[2], q2 = tid ? mine[LRUN + 1 - LSTRIDE] : cin[3];
        float p[2] = {0.f, 0.f};
#pragma unroll
        for (int k = 0; k < LRUN; ++k) {
            const float w = fmaf(c[5], v[k], fmaf(c[6], q1, c[7] * q2));
            q2 = q1, q1 = v[k];
            if (last && k + 1 == cnt) cout[2] = q1, cout[3] = q2;
            v[k] = w;
            allpole_step(w, p, c + 5);
        }
        scan_entry_state<true>(p, powers + LPOW, plp, zwp, cin + 4, lane, wave);
#pragma unroll
        for (int k = 0; k < LRUN; ++k) {
            const float y = allpole_step(v[k], p, c + 5);
            if (last && k + 1 == cnt) cout[4] = p[0], cout[5] = p[1];
            v[k] = y * y;
        }
        *reinterpret_cast<f32x4*>(mine) = (f32x4){v[0], v[1], v[2], v[3]};
        *reinterpret_cast<f32x4*>(mine + 4) = (f32x4){v[4], v[5], v[6], v[7]};
        __syncthreads();
        // wave w sums the tile's hop w: lane j takes samples j, j + 64, .. in increasing order, then the butterfly
        const int64_t gh = t * hpt + wave;
        if (wave < hpt && gh < whole) {
            float acc = 0.f;
            for (int j = lane; j < hop; j += 64) acc += tile[lds_slot(wave * hop + j)];
            acc = wave_sum(acc);
            if (lane == 0) {
                energy[gh] = acc;
                if (hop_energy) hop_energy[(int64_t)b * target_hops + gh] = acc;
            }
        }
        __syncthreads();
    }
    if (hop_energy) {
        for (int64_t h = whole + tid; h < target_hops; h += LTHREADS) hop_energy[(int64_t)b * target_hops + h] = 0.f;
    }
    // sample peak: exact, so the order does not matter
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) peak = fmaxf(peak, __shfl_xor(peak, o, 64));
    if (lane == 0) red[wave] = peak;
    __syncthreads();
    peak = red[0];
#pragma unroll
    for (int q = 1; q < LWAVES; ++q) peak = fmaxf(peak, red[q]);
    // blocks of four hops and the two gates, in the linear domain: thread tid takes blocks tid, tid + 1024, ..
    const int nb = whole >= 4 ? (int)(whole - 3) : 0;
    const float blk = (float)(4 * hop);
    float sum = 0.f, cntf = 0.f;
    for (int j = tid; j < nb; j += LTHREADS) {
        const float z = (((energy[j] + energy[j + 1]) + energy[j + 2]) + energy[j + 3]) / blk;
        if (z > LABS_GATE) sum += z, cntf += 1.f;
    }
    sum = block_sum16(sum, red);
    const float n_abs = block_sum16(cntf, red);
    const float rel = n_abs > 0.f ? 0.1f * (sum / n_abs) : 0.f;  // 10 LU below the loudness of the kept blocks' mean
    sum = 0.f, cntf = 0.f;
    for (int j = tid; j < nb; j += LTHREADS) {
        const float z = (((energy[j] + energy[j + 1]) + energy[j + 2]) + energy[j + 3]) / blk;
        if (z > LABS_GATE && z > rel) sum += z, cntf += 1.f;
    }
    sum = block_sum16(sum, red);
    const float n_rel = block_sum16(cntf, red);
    if (tid == 0) {
        float* o = stats + (int64_t)b * 4;
        o[0] = n_rel > 0.f ? -0.691f + 10.f * log10f(sum / n_rel) : -INFINITY;
        o[1] = peak;
        o[2] = n_rel > 0.f ? n_abs : 0.f;
        o[3] = n_rel;
    }
}

// grid (chunks, B), 256 threads: every thread derives the clip's gain from the same inputs by the same operations
__global__ __launch_bounds__(256) void loudness_gain_kernel(const float* x, const int64_t* __restrict__ offsets, const float* __restrict__ stats,
                                                            const float* __restrict__ target, const float* __restrict__ ref_stats,
                                                            const int32_t* __restrict__ ref_index, float* out, float* __restrict__ gains,
                                                            float peak_limit) {
    const int b = blockIdx.y;
    const int64_t o0 = offsets[b], n = offsets[b + 1] - o0;
    const float L = stats[(int64_t)b * 4], peak = stats[(int64_t)b * 4 + 1];
    const float tgt = target ? target[b] : ref_stats[(int64_t)ref_index[b] * 4];
    float g = 1.f;
    if (isfinite(L) && isfinite(tgt) && peak > 0.f) {
        g = exp10f((tgt - L) * 0.05f);
        if (peak_limit > 0.f && g * peak > peak_limit) g = peak_limit / peak;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) gains[b] = g;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) out[o0 + i] = g * x[o0 + i];
}

}  // namespace

extern "C" int apad_loudness(const float* x, const int64_t* offsets, const int64_t* offsets_host, const float* coef, const float* powers,
                             float* stats, float* hop_energy, int32_t batch, int32_t hop, int32_t target_hops, void* stream) {
    APAD_CHECK(x && offsets && offsets_host && coef && powers && stats && batch > 0, "apad_loudness: bad operands");
    APAD_CHECK(batch <= 65535, "apad_loudness: batch %d exceeds 65535", batch);
    APAD_CHECK(hop >= 1 && hop <= LTILE, "apad_loudness: a hop of %d samples is outside [1, %d]", hop, LTILE);
    APAD_CHECK(!hop_energy || target_hops > 0, "apad_loudness: hop_energy needs target_hops > 0");
    APAD_CHECK(offsets_host[0] == 0, "apad_loudness: offsets[0] must be 0");
    for (int i = 0; i < batch; ++i) {
        const int64_t n = offsets_host[i + 1] - offsets_host[i];
        APAD_CHECK(n > 0, "apad_loudness: clip %d is empty", i);
        APAD_CHECK(n / hop <= LMAXHOPS, "apad_loudness: clip %d has %lld hops, at most %d are kept", i, (long long)(n / hop), LMAXHOPS);
        APAD_CHECK(!hop_energy || n / hop <= target_hops, "apad_loudness: clip %d has %lld whole hops, target_hops is %d", i, (long long)(n / hop),
                   target_hops);
    }
    const int hpt = LTILE / hop < LWAVES ? LTILE / hop : LWAVES;
    hipLaunchKernelGGL(loudness_kernel, dim3((unsigned)batch), dim3(LTHREADS), 0, (hipStream_t)stream, x, offsets, coef, powers, stats,
                       hop_energy, (int)hop, hpt, (int)target_hops);
    return apad_check_launch("apad_loudness");
}

extern "C" int apad_loudness_gain(const float* x, const int64_t* offsets, const int64_t* offsets_host, const float* stats, const float* target,
                                  const float* ref_stats, const int32_t* ref_index, const int32_t* ref_index_host, float* out, float* gains,
                                  int32_t batch, int32_t n_ref, float peak_limit, void* stream) {
    APAD_CHECK(x && offsets && offsets_host && stats && out && gains && batch > 0, "apad_loudness_gain: bad operands");
    APAD_CHECK(batch <= 65535, "apad_loudness_gain: batch %d exceeds 65535", batch);
    const bool by_ref = ref_stats || ref_index || ref_index_host;
    APAD_CHECK(by_ref ? (!target && ref_stats && ref_index && ref_index_host && n_ref > 0) : target != nullptr,
               "apad_loudness_gain: give either target, or ref_stats with ref_index, ref_index_host and n_ref > 0");
    APAD_CHECK(peak_limit == peak_limit, "apad_loudness_gain: peak_limit is NaN");
    APAD_CHECK(offsets_host[0] == 0, "apad_loudness_gain: offsets[0] must be 0");
    int64_t longest = 0;
    for (int i = 0; i < batch; ++i) {
        const int64_t n = offsets_host[i + 1] - offsets_host[i];
        APAD_CHECK(n > 0, "apad_loudness_gain: clip %d is empty", i);
        APAD_CHECK(!by_ref || (ref_index_host[i] >= 0 && ref_index_host[i] < n_ref), "apad_loudness_gain: ref_index[%d] = %d outside [0, %d)", i,
                   by_ref ? ref_index_host[i] : 0, n_ref);
        longest = n > longest ? n : longest;
    }
    const int64_t chunks = (longest + 2047) / 2048;  // 8 samples per thread unless the clip is very long
    hipLaunchKernelGGL(loudness_gain_kernel, dim3((unsigned)(chunks < 4096 ? chunks : 4096), (unsigned)batch), dim3(256), 0, (hipStream_t)stream,
                       x, offsets, stats, target, ref_stats, ref_index, out, gains, peak_limit);
    return apad_check_launch("apad_loudness_gain");
}
