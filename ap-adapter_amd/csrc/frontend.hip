// Audio front-end ("next" row f-2): the steps immediately upstream of AudioMAE,
// reference audio_encoder/AudioMAE.py:356-394 (extract_kaldi_fbank_feature):
//   apad_resample_fir   torchaudio.functional.resample as a polyphase FIR (kernel table from the host)
//   apad_kaldi_fbank    Kaldi-compatible 128-bin log-mel filterbank of 25 ms / 10 ms frames, zero-padded or cropped to
//                       `target_frames` rows BEFORE the (x - mean) / (2 std) normalisation, like the reference
// fp32 throughout (the reference computes the mel in fp32 and feeds AudioMAE fp32).  HBM/latency-bound byte-sized work:
// one workgroup per frame, the whole frame lives in LDS (DC removal, pre-emphasis, window, 512-point radix-2 FFT, power,
// mel projection, log); nothing here is shaped for MFMA.
//
// VAE front-end ("next" rows f-2 / f-3): the log-mel the mel VAE encodes into training latents, reference
// train_apadapter_v2.py:253-336 (wav_to_mel -> audioldm TacotronSTFT.mel_spectrogram):
//   apad_wav_stats      per-clip {mean, 0.5 / max|x - mean|} of a ragged batch (normalize_wav + pad_wav + the second peak
//                       normalisation, folded into one affine map)
//   apad_stft_logmel    1024-point periodic-Hann STFT (hop 160, reflect-padded by 512) -> |X| -> 64 Slaney mel filters ->
//                       log(max(., 1e-5)), the first `target_frames` frames of each clip
//
// CLAP front-end (score_waveforms; transformers ClapFeatureExtractor with truncation="rand_trunc"):
//   apad_clap_logmel    resample (the polyphase sum of apad_resample_fir, on the fly) -> crop / repeatpad / repeat / pad to
//                       max_length -> 1024-point periodic-Hann STFT (run-time hop, reflect-padded by 512) -> |X|^2 -> Slaney
//                       mel filters -> 10 log10(max(., 1e-10)), one launch for a ragged batch
//
// Edit fidelity (score_fidelity; librosa.feature.chroma_stft at its defaults with the tuning fixed, restated: PARITY UNPINNED):
//   apad_chroma              2048-point periodic-Hann STFT (hop 512, zero-padded by 1024) -> |X|^2 -> 12 chroma filters -> each frame
//                            divided by its maximum, one launch for a ragged batch
//   apad_chroma_similarity   mean over the frames of the cosine between a candidate's and its reference's chroma vectors
#include "common.h"

namespace {

constexpr int WIN = 400, SHIFT = 160, NFFT = 512, NBIN = 257;

__global__ __launch_bounds__(256) void resample_kernel(const float* x, const float* kern, float* out, int64_t n_in, int64_t n_out,
                                                       int orig, int newf, int width, int kw) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_out) return;
    const int64_t blk = i / newf;
    const int phase = (int)(i - blk * newf);
    const float* kp = kern + (int64_t)phase * kw;
    const int64_t base = blk * orig - width;  // index into the un-padded input
    float acc = 0.f;
    for (int j = 0; j < kw; ++j) {
        const int64_t s = base + j;
        const float v = (s >= 0 && s < n_in) ? x[s] : 0.f;
        acc = fmaf(kp[j], v, acc);
    }
    out[i] = acc;
}

// sum over the workgroup in a fixed order
__device__ __forceinline__ float block_sum(float v, float* sh) {
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    return sh[0] + sh[1] + sh[2] + sh[3];
}

__global__ __launch_bounds__(256) void fbank_kernel(const float* x, float dc, const float* window, const float* twiddle /* [256][2] */,
                                                    const float* mel /* [nmel][257] */, float* out, int n_frames, int nmel,
                                                    float preemph, float norm_mean, float inv_2std) {
    __shared__ float re[NFFT], im[NFFT], raw[WIN], sh[4];
    const int f = blockIdx.x, tid = threadIdx.x;
    if (f >= n_frames) {  // rows past the last frame: zero-padded BEFORE normalisation (AudioMAE.py:384-387, :393)
        for (int b = tid; b < nmel; b += 256) out[(int64_t)f * nmel + b] = (0.f - norm_mean) * inv_2std;
        return;
    }
    const float* xf = x + (int64_t)f * SHIFT;
    float part = 0.f;
    for (int j = tid; j < WIN; j += 256) {
        const float v = xf[j] - dc;  // waveform - waveform.mean() (:368)
        raw[j] = v;
        part += v;
    }
    const float mean = block_sum(part, sh) / (float)WIN;  // remove_dc_offset, per frame
    // bit-reversed load for the in-place decimation-in-time FFT; samples >= WIN are the zero padding to 512
    for (int j = tid; j < NFFT; j += 256) {
        float v = 0.f;
        if (j < WIN) {
            const float cur = raw[j] - mean, prev = raw[j > 0 ? j - 1 : 0] - mean;  // replicate-padded pre-emphasis
            v = (cur - preemph * prev) * window[j];
        }
        const int r = (int)(__brev((unsigned)j) >> 23);  // 9-bit reversal
        re[r] = v;
        im[r] = 0.f;
    }
    __syncthreads();
#pragma unroll 1
    for (int s = 1; s <= 9; ++s) {
        const int half = 1 << (s - 1);
        const int grp = tid >> (s - 1), pos = tid & (half - 1);
        const int i0 = grp * (half << 1) + pos, i1 = i0 + half;
        const int tw = pos << (9 - s);  // twiddle index k * (512 / 2^s)
        const float wr = twiddle[2 * tw], wi = twiddle[2 * tw + 1];
        const float ar = re[i0], ai = im[i0], br = re[i1], bi = im[i1];
        const float tr = br * wr - bi * wi, ti = br * wi + bi * wr;
        re[i0] = ar + tr; im[i0] = ai + ti;
        re[i1] = ar - tr; im[i1] = ai - ti;
        __syncthreads();
    }
    // power spectrum, bins 0..256 (reuse re[] for the power; bin 256 lives in re[256])
    float p0 = re[tid] * re[tid] + im[tid] * im[tid];
    float p256 = 0.f;
    if (tid == 0) p256 = re[256] * re[256] + im[256] * im[256];
    __syncthreads();
    re[tid] = p0;
    if (tid == 0) re[256] = p256;
    __syncthreads();
    for (int b = tid; b < nmel; b += 256) {
        const float* w = mel + (int64_t)b * NBIN;
        float e = 0.f;
        for (int k = 0; k < NBIN; ++k) e = fmaf(w[k], re[k], e);
        e = fmaxf(e, 1.1920928955078125e-07f);  // use_log_fbank: max(eps).log()
        out[(int64_t)f * nmel + b] = (__logf(e) - norm_mean) * inv_2std;
    }
}

}  // namespace

extern "C" int apad_resample_fir(const float* x, const float* kernel, float* out, int64_t n_in, int64_t n_out, int32_t orig,
                                 int32_t newf, int32_t width, void* stream) {
    APAD_CHECK(x && kernel && out && n_in > 0 && n_out > 0 && orig > 0 && newf > 0 && width >= 0, "apad_resample_fir: bad operands");
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(resample_kernel, dim3((unsigned)((n_out + 255) / 256)), dim3(256), 0, s, x, kernel, out, n_in, n_out, orig, newf,
                       width, 2 * width + orig);
    return apad_check_launch("apad_resample_fir");
}

extern "C" int apad_kaldi_fbank(const float* x, int64_t n_samples, float dc, const float* window, const float* twiddle, const float* mel,
                                float* out, int32_t target_frames, int32_t num_mel_bins, float preemphasis, float norm_mean,
                                float norm_std, void* stream) {
    APAD_CHECK(x && window && twiddle && mel && out && target_frames > 0 && num_mel_bins > 0, "apad_kaldi_fbank: bad operands");
    int64_t frames = n_samples < WIN ? 0 : 1 + (n_samples - WIN) / SHIFT;  // snip_edges
    if (frames > target_frames) frames = target_frames;                     // crop (:388-389)
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(fbank_kernel, dim3((unsigned)target_frames), dim3(256), 0, s, x, dc, window, twiddle, mel, out, (int)frames,
                       num_mel_bins, preemphasis, norm_mean, 1.0f / (2.0f * norm_std));
    return apad_check_launch("apad_kaldi_fbank");
}

// ---------------------------------------------------------------------------------------------------------------------
// VAE log-mel front-end
// ---------------------------------------------------------------------------------------------------------------------
namespace {

constexpr int SNFFT = 1024, SHOP = 160, SPAD = SNFFT / 2, SBIN = SNFFT / 2 + 1, SMEL = 64, STATS_NT = 1024;

// In-place decimation-in-time radix-2 FFT of 2^LOG2N points in LDS (input in bit-reversed order, output in natural
// order).  twiddle [2^(LOG2N-1)][2] = (cos, -sin)(2 pi k / 2^LOG2N); NT threads own 2^(LOG2N-1) / NT butterflies each
// per stage.  (fbank_kernel keeps its own copy of the 512-point loop: routing it through this template changes its
// device code.)
template <int LOG2N, int NT>
__device__ __forceinline__ void fft_radix2(float* re, float* im, const float* twiddle, int tid) {
    constexpr int PER = (1 << (LOG2N - 1)) / NT;
    static_assert(PER * NT == (1 << (LOG2N - 1)), "whole butterflies per thread");
#pragma unroll 1
    for (int s = 1; s <= LOG2N; ++s) {
        const int half = 1 << (s - 1);
#pragma unroll
        for (int r = 0; r < PER; ++r) {
            const int bf = tid + r * NT;
            const int grp = bf >> (s - 1), pos = bf & (half - 1);
            const int i0 = grp * (half << 1) + pos, i1 = i0 + half;
            const int tw = pos << (LOG2N - s);  // twiddle index k * (2^LOG2N / 2^s)
            const float wr = twiddle[2 * tw], wi = twiddle[2 * tw + 1];
            const float ar = re[i0], ai = im[i0], br = re[i1], bi = im[i1];
            const float tr = br * wr - bi * wi, ti = br * wi + bi * wr;
            re[i0] = ar + tr; im[i0] = ai + ti;
            re[i1] = ar - tr; im[i1] = ai - ti;
        }
        __syncthreads();
    }
}

// One workgroup per clip: a one-pass sum (fp64 per lane), min and max, reduced lane -> wave -> workgroup in a fixed
// order (no atomics), so a clip's result does not depend on the batch around it.
// stats[2b] = mean, stats[2b+1] = 0.5 / max(xmax - mean, mean - xmin), or 0 for a constant / silent clip.
__global__ __launch_bounds__(STATS_NT) void wav_stats_kernel(const float* x, const int64_t* offsets, float* stats) {
    __shared__ double ssum[STATS_NT / 64];
    __shared__ float smin[STATS_NT / 64], smax[STATS_NT / 64];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int64_t o0 = offsets[b], n = offsets[b + 1] - o0;
    const float* xc = x + o0;
    double sum = 0.0;
    float lo = INFINITY, hi = -INFINITY;
    for (int64_t i = tid; i < n; i += STATS_NT) {
        const float v = xc[i];
        sum += (double)v;
        lo = fminf(lo, v);
        hi = fmaxf(hi, v);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        sum += __shfl_xor(sum, o, 64);
        lo = fminf(lo, __shfl_xor(lo, o, 64));
        hi = fmaxf(hi, __shfl_xor(hi, o, 64));
    }
    if ((tid & 63) == 0) {
        ssum[tid >> 6] = sum;
        smin[tid >> 6] = lo;
        smax[tid >> 6] = hi;
    }
    __syncthreads();
    if (tid == 0) {
        double s = 0.0;
        for (int w = 0; w < STATS_NT / 64; ++w) {
            s += ssum[w];
            lo = fminf(lo, smin[w]);
            hi = fmaxf(hi, smax[w]);
        }
        const float mean = (float)(s / (double)n);
        const float peak = fmaxf(hi - mean, mean - lo);  // max|x - mean|
        stats[2 * b] = mean;
        stats[2 * b + 1] = peak > 0.f ? 0.5f / peak : 0.f;
    }
}

// grid (target_frames, B), 256 threads: frame f of clip b.  The clip's virtual signal is y[i] = clip((x[i] - mean) * scale,
// -1, 1) for i < n, 0 for n <= i < nv = max(n, segment) (pad_wav's zeros come after the normalisation); the STFT reads it
// reflect-padded by 512 (edge sample not repeated).  Frames past nv / 160 + 1 (none when nv >= target * 160) are zero rows.
__global__ __launch_bounds__(256) void stft_logmel_kernel(const float* x, const int64_t* offsets, const float* stats,
                                                          const float* window, const float* twiddle /* [512][2] */,
                                                          const float* mel /* [64][513] */, const int32_t* mel_range /* [64][2] */,
                                                          float* out, int64_t segment, int target) {
    __shared__ float re[SNFFT], im[SNFFT];
    const int f = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    float* o = out + ((int64_t)b * target + f) * SMEL;
    const int64_t o0 = offsets[b], n = offsets[b + 1] - o0;
    const int64_t nv = n > segment ? n : segment;
    if ((int64_t)f >= nv / SHOP + 1) {
        if (tid < SMEL) o[tid] = 0.f;
        return;
    }
    const float mean = stats[2 * b], scale = stats[2 * b + 1];
    const float* xc = x + o0;
    const int64_t start = (int64_t)f * SHOP - SPAD;
    for (int j = tid; j < SNFFT; j += 256) {
        int64_t i = start + j;
        if (i < 0) i = -i;                   // left reflection: i in [1, 512]
        if (i >= nv) i = 2 * (nv - 1) - i;   // right reflection: nv > 512 keeps i >= 0
        float v = 0.f;
        if (i < n) v = fminf(fmaxf((xc[i] - mean) * scale, -1.f), 1.f);
        const int r = (int)(__brev((unsigned)j) >> 22);  // 10-bit reversal
        re[r] = v * window[j];
        im[r] = 0.f;
    }
    __syncthreads();
    fft_radix2<10, 256>(re, im, twiddle, tid);
    // magnitudes of bins 0..512 into re[] (every read before any write)
    const float m0 = sqrtf(re[tid] * re[tid] + im[tid] * im[tid]);
    const float m1 = sqrtf(re[tid + 256] * re[tid + 256] + im[tid + 256] * im[tid + 256]);
    const float m2 = tid == 0 ? sqrtf(re[512] * re[512] + im[512] * im[512]) : 0.f;
    __syncthreads();
    re[tid] = m0;
    re[tid + 256] = m1;
    if (tid == 0) re[512] = m2;
    __syncthreads();
    // 4 lanes per mel filter over its non-zero bins [lo, hi), combined in a fixed order
    const int filt = tid >> 2, lane = tid & 3;
    const int lo = mel_range[2 * filt], hi = mel_range[2 * filt + 1];
    const float* w = mel + (int64_t)filt * SBIN;
    float e = 0.f;
    for (int k = lo + lane; k < hi; k += 4) e = fmaf(w[k], re[k], e);
    e += __shfl_xor(e, 1, 64);
    e += __shfl_xor(e, 2, 64);
    if (lane == 0) o[filt] = logf(fmaxf(e, 1e-5f));
}

}  // namespace

extern "C" int apad_wav_stats(const float* x, const int64_t* offsets, const int64_t* offsets_host, float* stats, int32_t batch,
                              void* stream) {
    APAD_CHECK(x && offsets && offsets_host && stats && batch > 0, "apad_wav_stats: bad operands");
    APAD_CHECK(offsets_host[0] == 0, "apad_wav_stats: offsets[0] must be 0");
    for (int i = 0; i < batch; ++i)
        APAD_CHECK(offsets_host[i + 1] - offsets_host[i] > 100, "apad_wav_stats: clip %d has %lld samples (needs > 100)", i,
                   (long long)(offsets_host[i + 1] - offsets_host[i]));
    hipLaunchKernelGGL(wav_stats_kernel, dim3((unsigned)batch), dim3(STATS_NT), 0, (hipStream_t)stream, x, offsets, stats);
    return apad_check_launch("apad_wav_stats");
}

extern "C" int apad_stft_logmel(const float* x, const int64_t* offsets, const int64_t* offsets_host, const float* stats,
                                const float* window, const float* twiddle, const float* mel, const int32_t* mel_range, float* out,
                                int32_t batch, int64_t segment, int32_t target_frames, void* stream) {
    APAD_CHECK(x && offsets && offsets_host && stats && window && twiddle && mel && mel_range && out && batch > 0,
               "apad_stft_logmel: bad operands");
    APAD_CHECK(segment > SPAD, "apad_stft_logmel: segment %lld must exceed the 512-sample reflect pad", (long long)segment);
    APAD_CHECK(target_frames > 0 && batch <= 65535, "apad_stft_logmel: target_frames %d / batch %d out of range", target_frames, batch);
    APAD_CHECK(offsets_host[0] == 0, "apad_stft_logmel: offsets[0] must be 0");
    for (int i = 0; i < batch; ++i)
        APAD_CHECK(offsets_host[i + 1] - offsets_host[i] > 100, "apad_stft_logmel: clip %d has %lld samples (needs > 100)", i,
                   (long long)(offsets_host[i + 1] - offsets_host[i]));
    hipLaunchKernelGGL(stft_logmel_kernel, dim3((unsigned)target_frames, (unsigned)batch), dim3(256), 0, (hipStream_t)stream, x, offsets,
                       stats, window, twiddle, mel, mel_range, out, segment, (int)target_frames);
    return apad_check_launch("apad_stft_logmel");
}

// ---------------------------------------------------------------------------------------------------------------------
// CLAP log-mel front-end
// ---------------------------------------------------------------------------------------------------------------------
namespace {

constexpr int CLAP_SRC_CAP = 4096;  // floats of LDS for a frame's source window (two segments when a repeat seam cuts it)
enum { CLAP_REPEATPAD = 0, CLAP_REPEAT = 1, CLAP_PAD = 2 };

// One output sample of the polyphase resampler, resample_kernel's arithmetic on a staged window: the same taps, acc = 0 then
// acc = fmaf(kp[j], v, acc) in tap order, v = 0 outside the clip (the staging wrote those zeros).  resample_kernel keeps its
// own copy of the loop: routing it through this function flips a branch in its device code.
__device__ __forceinline__ float polyphase_sum(const float* kp, int kw, const float* v) {
    float acc = 0.f;
    for (int j = 0; j < kw; ++j) acc = fmaf(kp[j], v[j], acc);
    return acc;
}

// grid (frames, B), 256 threads: frame f of clip b.  The clip of n source samples is r[0 .. n48) after resampling (n48 =
// ceil(n * newf / orig), r[q] = the polyphase sum resample_kernel computes; never stored).  The max_length samples the STFT
// frames are v[i] = r[shift + i mod n48] for i < limit, else 0, with (shift, limit) = (starts[b], max_length) for a clip longer
// than max_length, else shift = 0 and limit = max_length (repeat), n48 (pad) or (max_length / n48) n48 (repeatpad).  Frame f
// reads v reflect-padded by 512 (edge sample not repeated) from f * hop - 512.
// The frame's indices i cover one range [imin, imax]; modulo n48 that is one range of q or two (a seam), each staged into LDS
// as the source samples its taps reach, zeros outside [0, n).
__global__ __launch_bounds__(256) void clap_logmel_kernel(const float* x, const int64_t* offsets, const int64_t* starts, const float* kern,
                                                          int orig, int newf, int width, const float* window,
                                                          const float* twiddle /* [512][2] */, const float* mel /* [n_mels][513] */,
                                                          const int32_t* mel_range /* [n_mels][2] */, float* out, int64_t max_length,
                                                          int hop, int n_mels, int mode) {
    __shared__ float re[SNFFT], im[SNFFT], src[CLAP_SRC_CAP];
    const int f = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const int64_t o0 = offsets[b], n = offsets[b + 1] - o0;
    const float* xc = x + o0;
    const int64_t n48 = (n * newf + orig - 1) / orig;
    const bool longer = n48 > max_length;
    const int64_t shift = longer ? starts[b] : 0;
    const int64_t limit = (longer || mode == CLAP_REPEAT) ? max_length : mode == CLAP_PAD ? n48 : (max_length / n48) * n48;
    const int kw = 2 * width + orig;
    const int64_t first = (int64_t)f * hop - SPAD;
    // the range of i the frame reads, after both reflections and the cut at `limit`
    int64_t imin = first < 0 ? 0 : first, imax = first + SNFFT - 1;
    if (first < 0 && -first > imax) imax = -first;
    if (imax >= max_length) {
        const int64_t refl = 2 * (max_length - 1) - imax;
        if (refl < imin) imin = refl;
        imax = max_length - 1;
    }
    if (imax >= limit) imax = limit - 1;
    // its image under q = shift + i mod n48: segment A = [qa0, qa1], segment B = [qb0, qb1] (empty: q1 < q0)
    int64_t qa0 = 0, qa1 = -1, qb0 = 0, qb1 = -1;
    if (imin <= imax) {
        if (imax - imin + 1 >= n48) {
            qa1 = n48 - 1;
        } else {
            qa0 = imin % n48;
            qa1 = imax % n48;
            if (qa0 > qa1) {
                qb1 = qa1;
                qa1 = n48 - 1;
            }
        }
        qa0 += shift; qa1 += shift; qb0 += shift; qb1 += shift;
    }
    // source samples the segments' taps reach: [sa0, sa0 + la) and [sb0, sb0 + lb)
    const int64_t sa0 = (qa0 / newf) * orig - width, sb0 = (qb0 / newf) * orig - width;
    int la = qa1 >= qa0 ? (int)((qa1 / newf - qa0 / newf) * orig) + kw : 0;
    int lb = qb1 >= qb0 ? (int)((qb1 / newf - qb0 / newf) * orig) + kw : 0;
    if (la > CLAP_SRC_CAP) la = CLAP_SRC_CAP;  // (the host checked la + lb <= CLAP_SRC_CAP for every frame)
    if (lb > CLAP_SRC_CAP - la) lb = CLAP_SRC_CAP - la;
    for (int t = tid; t < la + lb; t += 256) {
        const int64_t s = t < la ? sa0 + t : sb0 + (t - la);
        src[t] = (s >= 0 && s < n) ? xc[s] : 0.f;
    }
    __syncthreads();
    for (int j = tid; j < SNFFT; j += 256) {
        int64_t i = first + j;
        if (i < 0) i = -i;                                   // left reflection: i in [1, 512], max_length > 512
        if (i >= max_length) i = 2 * (max_length - 1) - i;   // right reflection
        float v = 0.f;
        if (i < limit) {
            const int64_t q = shift + i % n48;
            const bool in_a = q >= qa0 && q <= qa1;
            const int64_t blk = q / newf;
            const int phase = (int)(q - blk * newf);
            const int at = (int)(blk * orig - width - (in_a ? sa0 : sb0)) + (in_a ? 0 : la);
            if (at >= 0 && at + kw <= la + lb)  // (always: the segments cover the frame)
                v = kern ? polyphase_sum(kern + (int64_t)phase * kw, kw, src + at) : src[at];
        }
        const int r = (int)(__brev((unsigned)j) >> 22);  // 10-bit reversal
        re[r] = v * window[j];
        im[r] = 0.f;
    }
    __syncthreads();
    fft_radix2<10, 256>(re, im, twiddle, tid);
    // power of bins 0..512 into re[] (every read before any write)
    const float p0 = re[tid] * re[tid] + im[tid] * im[tid];
    const float p1 = re[tid + 256] * re[tid + 256] + im[tid + 256] * im[tid + 256];
    const float p2 = tid == 0 ? re[512] * re[512] + im[512] * im[512] : 0.f;
    __syncthreads();
    re[tid] = p0;
    re[tid + 256] = p1;
    if (tid == 0) re[512] = p2;
    __syncthreads();
    // 4 lanes per mel filter over its non-zero bins [lo, hi), combined in a fixed order
    const int filt = tid >> 2, lane = tid & 3;
    const bool live = filt < n_mels;
    const int lo = live ? mel_range[2 * filt] : 0, hi = live ? mel_range[2 * filt + 1] : 0;
    const float* w = mel + (int64_t)filt * SBIN;
    float e = 0.f;
    for (int k = lo + lane; k < hi; k += 4) e = fmaf(w[k], re[k], e);
    e += __shfl_xor(e, 1, 64);
    e += __shfl_xor(e, 2, 64);
    // power_to_db: 10 log10(max(e, 1e-10)); the floor itself is -100 exactly
    if (live && lane == 0)
        out[((int64_t)b * gridDim.x + f) * n_mels + filt] = e <= 1e-10f ? -100.f : 10.f * log10f(e);
}

}  // namespace

extern "C" int apad_clap_logmel(const float* x, const int64_t* offsets, const int64_t* offsets_host, const int64_t* starts,
                                const int64_t* starts_host, const float* kernel, int32_t orig, int32_t newf, int32_t width,
                                const float* window, const float* twiddle, const float* mel, const int32_t* mel_range, float* out,
                                int32_t batch, int64_t max_length, int32_t hop, int32_t n_mels, int32_t padding, void* stream) {
    APAD_CHECK(x && offsets && offsets_host && starts && starts_host && window && twiddle && mel && mel_range && out && batch > 0,
               "apad_clap_logmel: bad operands");
    APAD_CHECK(orig >= 1 && newf >= 1 && width >= 0, "apad_clap_logmel: resampling ratio %d : %d (width %d) out of range", orig, newf, width);
    APAD_CHECK(kernel || (orig == 1 && newf == 1 && width == 0), "apad_clap_logmel: a null kernel table means orig = new = 1, width = 0");
    APAD_CHECK(max_length > SPAD, "apad_clap_logmel: max_length %lld must exceed the 512-sample reflect pad", (long long)max_length);
    APAD_CHECK(n_mels >= 1 && n_mels <= SMEL, "apad_clap_logmel: n_mels %d outside [1, 64]", n_mels);
    APAD_CHECK(hop >= 1, "apad_clap_logmel: hop %d must be at least 1", hop);
    APAD_CHECK(batch <= 65535, "apad_clap_logmel: batch %d exceeds 65535", batch);
    APAD_CHECK(padding == CLAP_REPEATPAD || padding == CLAP_REPEAT || padding == CLAP_PAD, "apad_clap_logmel: padding mode %d unknown", padding);
    const int64_t frames = max_length / hop + 1;
    APAD_CHECK(frames <= 0x7fffffffLL, "apad_clap_logmel: %lld frames exceed the grid", (long long)frames);
    // a frame's source window: at most 1024 resampled samples in two segments, each with the taps' reach
    const int64_t need = ((int64_t)(SNFFT - 1) / newf + 2) * orig + 2 * (2 * (int64_t)width + orig);
    APAD_CHECK(need <= CLAP_SRC_CAP, "apad_clap_logmel: ratio %d : %d needs %lld staged samples per frame (limit %d)", orig, newf,
               (long long)need, CLAP_SRC_CAP);
    APAD_CHECK(offsets_host[0] == 0, "apad_clap_logmel: offsets[0] must be 0");
    for (int i = 0; i < batch; ++i) {
        const int64_t n = offsets_host[i + 1] - offsets_host[i];
        APAD_CHECK(n > 0, "apad_clap_logmel: clip %d is empty", i);
        const int64_t n48 = (n * newf + orig - 1) / orig;
        if (n48 > max_length)
            APAD_CHECK(starts_host[i] >= 0 && starts_host[i] <= n48 - max_length, "apad_clap_logmel: clip %d: crop start %lld outside [0, %lld]",
                       i, (long long)starts_host[i], (long long)(n48 - max_length));
    }
    hipLaunchKernelGGL(clap_logmel_kernel, dim3((unsigned)frames, (unsigned)batch), dim3(256), 0, (hipStream_t)stream, x, offsets, starts,
                       kernel, (int)orig, (int)newf, (int)width, window, twiddle, mel, mel_range, out, max_length, (int)hop, (int)n_mels,
                       (int)padding);
    return apad_check_launch("apad_clap_logmel");
}

// ---------------------------------------------------------------------------------------------------------------------
// Chroma features and chroma similarity (librosa.feature.chroma_stft at its defaults, tuning fixed by the host's filterbank)
// ---------------------------------------------------------------------------------------------------------------------
namespace {

constexpr int CNFFT = 2048, CHOP = 512, CPAD = CNFFT / 2, CBIN = CNFFT / 2 + 1, NCHROMA = 12;

// grid (target_frames, B), 256 threads: frame f of clip b covers samples [512 f - 1024, 512 f + 1024) of the clip, zeros outside
// it (center=True, pad_mode="constant"); a clip of n samples has 1 + n / 512 frames, later rows are 0.  Thread t owns bins t,
// t + 256, t + 512, t + 768 (thread 0 also bin 1024): their powers never go back to LDS.  Each of the 12 filter sums goes lane (bins
// in increasing order) -> wave (xor butterfly) -> workgroup (waves 0..3 in order): no atomics, nothing depends on the grid.
__global__ __launch_bounds__(256) void chroma_kernel(const float* x, const int64_t* offsets, const float* window,
                                                     const float* twiddle /* [1024][2] */, const float* fb /* [12][1025] */, float* out,
                                                     int target) {
    __shared__ float re[CNFFT], im[CNFFT], part[4][NCHROMA];
    const int f = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    float* o = out + ((int64_t)b * target + f) * NCHROMA;
    const int64_t o0 = offsets[b], n = offsets[b + 1] - o0;
    if ((int64_t)f >= n / CHOP + 1) {
        if (tid < NCHROMA) o[tid] = 0.f;
        return;
    }
    const float* xc = x + o0;
    const int64_t start = (int64_t)f * CHOP - CPAD;
    for (int j = tid; j < CNFFT; j += 256) {
        const int64_t i = start + j;
        const float v = (i >= 0 && i < n) ? xc[i] : 0.f;
        const int r = (int)(__brev((unsigned)j) >> 21);  // 11-bit reversal
        re[r] = v * window[j];
        im[r] = 0.f;
    }
    __syncthreads();
    fft_radix2<11, 256>(re, im, twiddle, tid);
    float acc[NCHROMA];
#pragma unroll
    for (int c = 0; c < NCHROMA; ++c) acc[c] = 0.f;
#pragma unroll
    for (int r = 0; r < 5; ++r) {
        const int k = tid + r * 256;
        if (k < CBIN) {  // r = 4: bin 1024, thread 0 only
            const float p = re[k] * re[k] + im[k] * im[k];
#pragma unroll
            for (int c = 0; c < NCHROMA; ++c) acc[c] = fmaf(fb[c * CBIN + k], p, acc[c]);
        }
    }
#pragma unroll
    for (int c = 0; c < NCHROMA; ++c) acc[c] = wave_sum(acc[c]);
    if ((tid & 63) == 0) {
#pragma unroll
        for (int c = 0; c < NCHROMA; ++c) part[tid >> 6][c] = acc[c];
    }
    __syncthreads();
    if (tid < 64) {  // lanes 0..11 hold the classes; the maximum goes over the first 16 lanes (lanes 12..15 carry 0 <= every sum)
        float v = tid < NCHROMA ? ((part[0][tid] + part[1][tid]) + part[2][tid]) + part[3][tid] : 0.f;
        float m = fabsf(v);
#pragma unroll
        for (int s = 8; s > 0; s >>= 1) m = fmaxf(m, __shfl_xor(m, s, 64));
        if (m < 1.1754944e-38f) m = 1.f;  // util.normalize: a frame below the smallest normal is left as it is (silence: exactly 0)
        if (tid < NCHROMA) o[tid] = v / m;
    }
}

// One workgroup per candidate i: cosine of a[i][f] and b[ref_index[i]][f] over the 12 classes for f < frames[i], each thread its
// frames f = t, t + 256, ... in increasing order, then lane -> wave -> workgroup in a fixed order and one division by frames[i].
__global__ __launch_bounds__(256) void chroma_similarity_kernel(const float* a, const float* b, const int32_t* ref_index,
                                                                const int32_t* frames, float* out, float* per_frame, int T) {
    __shared__ float sh[4];
    const int i = blockIdx.x, tid = threadIdx.x;
    const int nf = frames[i];
    const float* ai = a + (int64_t)i * T * NCHROMA;
    const float* bi = b + (int64_t)ref_index[i] * T * NCHROMA;
    float sum = 0.f;
    for (int f = tid; f < T; f += 256) {
        float c = 0.f;
        if (f < nf) {
            float dot = 0.f, na = 0.f, nb = 0.f;
#pragma unroll
            for (int k = 0; k < NCHROMA; ++k) {
                const float u = ai[(int64_t)f * NCHROMA + k], v = bi[(int64_t)f * NCHROMA + k];
                dot = fmaf(u, v, dot);
                na = fmaf(u, u, na);
                nb = fmaf(v, v, nb);
            }
            c = dot / fmaxf(sqrtf(na) * sqrtf(nb), 1e-8f);
            sum += c;
        }
        if (per_frame) per_frame[(int64_t)i * T + f] = c;
    }
    sum = block_sum(sum, sh);
    if (tid == 0) out[i] = nf > 0 ? sum / (float)nf : 0.f;
}

}  // namespace

extern "C" int apad_chroma(const float* x, const int64_t* offsets, const int64_t* offsets_host, const float* window, const float* twiddle,
                           const float* fb, float* out, int32_t batch, int32_t target_frames, void* stream) {
    APAD_CHECK(x && offsets && offsets_host && window && twiddle && fb && out && batch > 0 && target_frames > 0, "apad_chroma: bad operands");
    APAD_CHECK(batch <= 65535, "apad_chroma: batch %d exceeds 65535", batch);
    APAD_CHECK(offsets_host[0] == 0, "apad_chroma: offsets[0] must be 0");
    for (int i = 0; i < batch; ++i) {
        const int64_t n = offsets_host[i + 1] - offsets_host[i];
        APAD_CHECK(n > 0, "apad_chroma: clip %d is empty", i);
        APAD_CHECK(n / CHOP + 1 <= target_frames, "apad_chroma: clip %d has %lld frames, target_frames is %d", i, (long long)(n / CHOP + 1),
                   target_frames);
    }
    hipLaunchKernelGGL(chroma_kernel, dim3((unsigned)target_frames, (unsigned)batch), dim3(256), 0, (hipStream_t)stream, x, offsets, window,
                       twiddle, fb, out, (int)target_frames);
    return apad_check_launch("apad_chroma");
}

extern "C" int apad_chroma_similarity(const float* a, const float* b, const int32_t* ref_index, const int32_t* ref_index_host,
                                      const int32_t* frames, const int32_t* frames_host, float* out, float* per_frame, int32_t n, int32_t m,
                                      int32_t T, void* stream) {
    APAD_CHECK(a && b && ref_index && ref_index_host && frames && frames_host && out && n > 0 && m > 0 && T > 0,
               "apad_chroma_similarity: bad operands");
    for (int i = 0; i < n; ++i) {
        APAD_CHECK(ref_index_host[i] >= 0 && ref_index_host[i] < m, "apad_chroma_similarity: ref_index[%d] = %d outside [0, %d)", i,
                   ref_index_host[i], m);
        APAD_CHECK(frames_host[i] >= 0 && frames_host[i] <= T, "apad_chroma_similarity: frames[%d] = %d outside [0, %d]", i, frames_host[i], T);
    }
    hipLaunchKernelGGL(chroma_similarity_kernel, dim3((unsigned)n), dim3(256), 0, (hipStream_t)stream, a, b, ref_index, frames, out, per_frame,
                       (int)T);
    return apad_check_launch("apad_chroma_similarity");
}
