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
