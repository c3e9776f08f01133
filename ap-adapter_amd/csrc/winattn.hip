// CLAP audio tower (HTSAT, a Swin transformer over the log-mel "image"; transformers ClapAudioModelWithProjection), fp32:
//   apad_window_attention  the shifted-window attention of one Swin block in ONE launch
//   apad_clap_mel2img      BatchNorm (eval) + bicubic time stretch + reshape_mel2img fold + 4x4 patch gather, one launch
//
// Window attention.  Input: the fused q | k | v projection of the LayerNormed tokens in RASTER order [B][H][W][3C]; output
// [B][H][W][C] in raster order.  torch.roll(-shift), window_partition, window_reverse and torch.roll(+shift) are index arithmetic:
// token t = 8 ty + tx of window (wy, wx) has the shifted coordinate (8 wy + ty, 8 wx + tx) and lives -- on the way in and on the
// way out -- at the raster position ((8 wy + ty + shift) % H, (8 wx + tx + shift) % W).  The shift mask (ClapAudioLayer.get_attn_mask)
// is not materialised either: per axis a shifted coordinate i has the region id (i >= n - 8) + (i >= n - shift), and a score gets
// -100 exactly where 3 * h_region + w_region of the two tokens differ.
//
// One workgroup = one (sample, window); its 4 waves walk the 2 * heads units (head, 32-query half).  House form of attention.hip /
// f32_ops.hip: TRANSPOSED scores S^T (keys x queries) = K . Q^T on v_mfma_f32_32x32x2_f32 (exact f32, bitwise an fmaf chain; d = 24
// is 12 k-steps, no padding), so a lane owns one query and its 64 scores sit in the 2 x 16 accumulator registers of the two key
// tiles: the softmax needs the half-wave exchange only.  O^T (channels x queries) = V^T . P^T re-uses the score registers as the B
// operand (register r of key tile kt is k-step r; V is read at the same key permutation).  Every reduction order is fixed.
#include <math.h>
#include "common.h"

namespace {

typedef float f4 __attribute__((ext_vector_type(4)));

constexpr int WIN = 8;          // window edge
constexpr int WT = WIN * WIN;   // tokens per window
constexpr int HD = 24;          // head size of every HTSAT stage
constexpr float LOG2E_W = 1.4426950408889634f;

__device__ __forceinline__ f32x16 mfma2(float a, float b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
}

struct WinP {
    const float* qkv;   // [B][H][W][3C]
    const float* bias;  // [heads][64][64] (query, key)
    float* out;         // [B][H][W][C]
    int32_t H, W, C, heads, shift;
    float scale;        // 1 / sqrt(24)
};

// region id of a shifted coordinate (get_attn_mask; only read when shift > 0)
__device__ __forceinline__ int region(int i, int n, int shift) { return (i >= n - WIN) + (i >= n - shift); }

__global__ __launch_bounds__(256) void window_attention_kernel(WinP p) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int half = lane >> 5, l31 = lane & 31;
    const int nwx = p.W / WIN, nwy = p.H / WIN;
    const int win = blockIdx.x % (nwx * nwy), b = blockIdx.x / (nwx * nwy);
    const int y0 = (win / nwx) * WIN, x0 = (win % nwx) * WIN;  // shifted coordinates of the window's first token
    const int64_t C3 = 3 * (int64_t)p.C;
    const int64_t img = (int64_t)b * p.H * p.W;
    // raster pixel of window token t
    auto pixel = [&](int t) -> int64_t {
        const int y = (y0 + (t >> 3) + p.shift) % p.H, x = (x0 + (t & 7) + p.shift) % p.W;
        return img + (int64_t)y * p.W + x;
    };
    auto region_of = [&](int t) -> int { return 3 * region(y0 + (t >> 3), p.H, p.shift) + region(x0 + (t & 7), p.W, p.shift); };

    for (int unit = wave; unit < 2 * p.heads; unit += 4) {  // wave-uniform: no barrier in the kernel
        const int h = unit >> 1, qt = unit & 1;
        const int tq = qt * 32 + l31;  // this lane's query
        const int64_t pq = pixel(tq);
        const int rq = region_of(tq);
        // Q^T B operand: lane holds Q[tq][cc * 8 + half * 4 .. + 4)
        f4 qf[3];
        {
            const float* qp = p.qkv + pq * C3 + h * HD + half * 4;
#pragma unroll
            for (int cc = 0; cc < 3; ++cc) qf[cc] = *reinterpret_cast<const f4*>(qp + cc * 8);
        }
        // S^T tiles: keys kt * 32 + (C layout rows), this lane's query
        f32x16 s[2];
#pragma unroll
        for (int kt = 0; kt < 2; ++kt) {
#pragma unroll
            for (int r = 0; r < 16; ++r) s[kt][r] = 0.f;
            const float* kp = p.qkv + pixel(kt * 32 + l31) * C3 + p.C + h * HD + half * 4;  // A operand row = key kt * 32 + l31
#pragma unroll
            for (int cc = 0; cc < 3; ++cc) {
                const f4 kf = *reinterpret_cast<const f4*>(kp + cc * 8);
#pragma unroll
                for (int j = 0; j < 4; ++j) s[kt] = mfma2(kf[j], qf[cc][j], s[kt]);  // d = cc * 8 + half * 4 + j in both operands
            }
        }
        // scores (base-2 exponent domain): (q.k / sqrt(24) + bias + mask) * log2(e)
        const float* bp = p.bias + ((int64_t)h * WT + tq) * WT + half * 4;
        float m = -3.0e38f;
#pragma unroll
        for (int kt = 0; kt < 2; ++kt)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const f4 bv = *reinterpret_cast<const f4*>(bp + kt * 32 + g * 8);  // keys kt * 32 + 8 g + 4 half + j
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    float v = s[kt][g * 4 + j] * p.scale + bv[j];
                    if (p.shift > 0 && region_of(kt * 32 + g * 8 + half * 4 + j) != rq) v += -100.0f;
                    v *= LOG2E_W;
                    s[kt][g * 4 + j] = v;
                    m = fmaxf(m, v);
                }
            }
        m = half_max(m);
        float sum = 0.f;
#pragma unroll
        for (int kt = 0; kt < 2; ++kt)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                s[kt][r] = exp2f(s[kt][r] - m);
                sum += s[kt][r];
            }
        const float inv = 1.0f / half_sum(sum);
        // O^T (channels x queries) += V^T . P^T: A operand row = channel l31 (rows 24..31 are zero), k = key
        f32x16 o;
#pragma unroll
        for (int r = 0; r < 16; ++r) o[r] = 0.f;
        const bool dvalid = l31 < HD;
        const float* vbase = p.qkv + 2 * p.C + h * HD + (dvalid ? l31 : 0);
#pragma unroll
        for (int kt = 0; kt < 2; ++kt)
#pragma unroll
            for (int g = 0; g < 4; ++g)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float vv = vbase[pixel(kt * 32 + g * 8 + half * 4 + j) * C3];
                    o = mfma2(dvalid ? vv : 0.f, s[kt][g * 4 + j], o);
                }
        // register r = channel 8 (r / 4) + 4 half + r % 4 of query tq: channels < 24 are g = 0..2
        float* op = p.out + pq * p.C + h * HD + half * 4;
#pragma unroll
        for (int g = 0; g < 3; ++g) {
            const f4 v = {o[g * 4] * inv, o[g * 4 + 1] * inv, o[g * 4 + 2] * inv, o[g * 4 + 3] * inv};
            *reinterpret_cast<f4*>(op + g * 8) = v;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// input_features [B][1][T][F] -> patch matrix [B * G * G][16] (G = S / 4), the A operand of the patch-embedding GEMM:
//   BatchNorm2d over the mel bins (eval: (x - mean) / sqrt(var + eps) * weight + bias per bin),
//   F.interpolate(mode="bicubic", align_corners=True) of the time axis to S * r frames (r = S / F) when T is shorter (torch's
//   cubic-convolution coefficients, A = -0.75, taps clamped to the border; the mel axis keeps its size, where the same
//   interpolation is the identity),
//   reshape_mel2img: img[c * F + f][tt] = x[c * S + tt][f] (r time chunks stacked along the image rows),
//   the 4 x 4 / stride-4 patch gather: row = py * G + px, column = ky * 4 + kx.
// ---------------------------------------------------------------------------------------------------------------------
struct MelP {
    const float* x;
    const float *bn_w, *bn_b, *bn_mean, *bn_var;
    float* out;
    int32_t B, T, F, S;
    float eps, tscale;  // tscale = (T - 1) / (S * r - 1) in fp32
};

__device__ __forceinline__ float cubic1(float x, float A) { return ((A + 2.f) * x - (A + 3.f)) * x * x + 1.f; }
__device__ __forceinline__ float cubic2(float x, float A) { return ((A * x - 5.f * A) * x + 8.f * A) * x - 4.f * A; }

__global__ __launch_bounds__(256) void clap_mel2img_kernel(MelP p) {
    const int G = p.S / 4;
    const int64_t total = (int64_t)p.B * G * G * 16;
    const int Tfull = p.S * (p.S / p.F);
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
        const int k = (int)(idx & 15);
        const int64_t tok = idx >> 4;
        const int px = (int)(tok % G), py = (int)((tok / G) % G), b = (int)(tok / ((int64_t)G * G));
        const int row = py * 4 + (k >> 2), col = px * 4 + (k & 3);
        const int c = row / p.F, f = row - c * p.F;
        const int t = c * p.S + col;  // frame of the stretched spectrogram
        const float* xb = p.x + (int64_t)b * p.T * p.F + f;
        const float alpha = p.bn_w[f] / sqrtf(p.bn_var[f] + p.eps), mean = p.bn_mean[f], beta = p.bn_b[f];
        float v;
        if (p.T == Tfull) {
            v = (xb[(int64_t)t * p.F] - mean) * alpha + beta;
        } else {
            const float real = p.tscale * (float)t;
            int i0 = (int)floorf(real);
            i0 = i0 < p.T - 1 ? i0 : p.T - 1;
            float lam = real - (float)i0;
            lam = fminf(fmaxf(lam, 0.f), 1.f);
            const float A = -0.75f;
            const float w[4] = {cubic2(lam + 1.f, A), cubic1(lam, A), cubic1(1.f - lam, A), cubic2(2.f - lam, A)};
            v = 0.f;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                int ti = i0 - 1 + j;
                ti = ti < 0 ? 0 : (ti > p.T - 1 ? p.T - 1 : ti);
                const float xv = (xb[(int64_t)ti * p.F] - mean) * alpha + beta;
                v = j == 0 ? w[0] * xv : v + w[j] * xv;
            }
        }
        p.out[idx] = v;
    }
}

}  // namespace

extern "C" int apad_window_attention(const void* qkv, const float* bias, void* out, int32_t B, int32_t H, int32_t W, int32_t heads,
                                     int32_t head_dim, int32_t window, int32_t shift, int32_t dtype, void* stream) {
    APAD_CHECK(qkv && bias && out, "apad_window_attention: null operand");
    APAD_CHECK(dtype == APAD_F32, "apad_window_attention: dtype %d not supported (fp32 only)", dtype);
    APAD_CHECK(window == WIN, "apad_window_attention: window %d not supported (8)", window);
    APAD_CHECK(head_dim == HD, "apad_window_attention: head_dim %d not supported (24)", head_dim);
    APAD_CHECK(shift == 0 || shift == WIN / 2, "apad_window_attention: shift %d not supported (0 or 4)", shift);
    APAD_CHECK(B > 0 && heads > 0 && H > 0 && W > 0 && H % WIN == 0 && W % WIN == 0,
               "apad_window_attention: need B, heads > 0 and H, W positive multiples of 8 (B=%d heads=%d H=%d W=%d)", B, heads, H, W);
    APAD_CHECK((int64_t)B * (H / WIN) * (W / WIN) < (int64_t)1 << 31, "apad_window_attention: too many windows");
    APAD_CHECK(((uintptr_t)qkv & 15) == 0 && ((uintptr_t)bias & 15) == 0 && ((uintptr_t)out & 15) == 0,
               "apad_window_attention: pointers must be 16-byte aligned");
    WinP p;
    p.qkv = (const float*)qkv; p.bias = bias; p.out = (float*)out;
    p.H = H; p.W = W; p.C = heads * HD; p.heads = heads; p.shift = shift;
    p.scale = 1.0f / sqrtf((float)HD);
    hipLaunchKernelGGL(window_attention_kernel, dim3((unsigned)(B * (H / WIN) * (W / WIN))), dim3(256), 0, (hipStream_t)stream, p);
    return apad_check_launch("apad_window_attention");
}

extern "C" int apad_clap_mel2img(const float* x, const float* bn_weight, const float* bn_bias, const float* bn_mean, const float* bn_var,
                                 float bn_eps, float* out, int32_t B, int32_t T, int32_t F, int32_t spec_size, void* stream) {
    APAD_CHECK(x && bn_weight && bn_bias && bn_mean && bn_var && out, "apad_clap_mel2img: null operand");
    APAD_CHECK(B > 0 && T > 0 && F > 0 && spec_size > 0 && spec_size % 4 == 0 && spec_size % F == 0,
               "apad_clap_mel2img: need B, T, F > 0, spec_size %% 4 == 0 and spec_size %% F == 0 (B=%d T=%d F=%d spec_size=%d)", B, T, F, spec_size);
    const int64_t Tfull = (int64_t)spec_size * (spec_size / F);
    APAD_CHECK(T <= Tfull, "apad_clap_mel2img: T=%d exceeds the swin input size (%lld frames)", T, (long long)Tfull);
    APAD_CHECK(T >= 2 || T == Tfull, "apad_clap_mel2img: a stretched input needs T >= 2 (T=%d)", T);
    MelP p;
    p.x = x; p.bn_w = bn_weight; p.bn_b = bn_bias; p.bn_mean = bn_mean; p.bn_var = bn_var; p.out = out;
    p.B = B; p.T = T; p.F = F; p.S = spec_size; p.eps = bn_eps;
    p.tscale = Tfull > 1 ? (float)(T - 1) / (float)(Tfull - 1) : 0.f;
    const int64_t total = (int64_t)B * (spec_size / 4) * (spec_size / 4) * 16;
    int64_t blocks = (total + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(clap_mel2img_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, p);
    return apad_check_launch("apad_clap_mel2img");
}
