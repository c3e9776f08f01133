// Small HBM-bound kernels of the path: AudioMAE token pooling, sinusoidal timestep embedding, fused
// classifier-free-guidance + sampler update (one kernel of two or three guidance branches and one host launch path behind apad_cfg_ddim_step /
// apad_cfg_sampler_step / apad_cfg_edit_step / apad_cfg_dual_step), the noise-extracting step of DDPM inversion beside it (apad_cfg_invert_step),
// the same step with guidance rescale / projected guidance, which sums over each clip (apad_cfg_shaped_step), the edit run's start, device-side
// step counter.
#include "common.h"
#include "f32_ops.h"

namespace {

// rep [B][513][768] -> out [B][(64/tp)*(8/fp)][768]; token (t,f) of the 64x8 grid is row 1 + 8*t + f.
// (avg + max) / 2 over (tp x fp) windows (reference AudioMAE.py:148-182).
template <int DT, int ODT>
__global__ __launch_bounds__(256) void pool_kernel(const uint8_t* rep, uint8_t* out, int B, int tp, int fp) {
    const int nt = 64 / tp, nf = 8 / fp, La = nt * nf;
    const int64_t total = (int64_t)B * La * 96;  // 96 vectors of 8 channels
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
        const int vc = (int)(idx % 96);
        const int64_t tok = idx / 96;
        const int b = (int)(tok / La), o = (int)(tok % La);
        const int ot = o / nf, of = o % nf;
        float s[8], mx[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            s[e] = 0.f;
            mx[e] = -3.0e38f;
        }
        for (int dt = 0; dt < tp; ++dt)
            for (int df = 0; df < fp; ++df) {
                const int row = 1 + 8 * (ot * tp + dt) + (of * fp + df);
                float v[8];
                unpack8<DT>(*reinterpret_cast<const uint4*>(rep + (((int64_t)b * 513 + row) * 768 + vc * 8) * 2), v);
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    s[e] += v[e];
                    mx[e] = fmaxf(mx[e], v[e]);
                }
            }
        const float inv = 1.0f / (float)(tp * fp);
        float y[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) y[e] = (s[e] * inv + mx[e]) * 0.5f;
        if (ODT == APAD_F32) {
            float4* op = reinterpret_cast<float4*>(out + (tok * 768 + vc * 8) * 4);
            op[0] = make_float4(y[0], y[1], y[2], y[3]);
            op[1] = make_float4(y[4], y[5], y[6], y[7]);
        } else {
            constexpr int PD = (ODT == APAD_F32) ? APAD_BF16 : ODT;
            *reinterpret_cast<uint4*>(out + (tok * 768 + vc * 8) * 2) = pack8<PD>(y);
        }
    }
}

// diffusers get_timestep_embedding: exponent = -ln(10000) * i / (half - freq_shift); [sin | cos], flipped to
// [cos | sin] when flip_sin_to_cos.
template <int DT>
__global__ void timestep_kernel(const float* t, uint8_t* out, int n, int dim, int flip, float freq_shift) {
    const int half = dim >> 1;
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n * half) return;
    const int r = idx / half, i = idx - r * half;
    // fp32 mode: the exponent in f32 exactly as torch forms it, exp correctly rounded (via f64) -- at t ~ 1000 one ulp of the
    // frequency is 6e-5 in the sin / cos argument
    const float ex = (-9.210340371976184f * (float)i) / ((float)half - freq_shift);
    const float freq = DT == APAD_F32 ? (float)exp((double)ex) : expf(ex);
    const float a = t[r] * freq;
    const float sv = sinf(a), cv = cosf(a);
    const int64_t base = (int64_t)r * dim;
    if (flip) {
        st_elem<DT>(out, base + i, cv);
        st_elem<DT>(out, base + half + i, sv);
    } else {
        st_elem<DT>(out, base + i, sv);
        st_elem<DT>(out, base + half + i, cv);
    }
}

// V consecutive elements <-> registers: V = 8 moves 16 bytes per access (two for fp32), V = 1 is the scalar form
template <int V> __device__ __forceinline__ void ld_f32v(const float* p, int64_t i, float* v) {
    if constexpr (V == 8) {
        const float4 a = *reinterpret_cast<const float4*>(p + i), b = *reinterpret_cast<const float4*>(p + i + 4);
        v[0] = a.x, v[1] = a.y, v[2] = a.z, v[3] = a.w, v[4] = b.x, v[5] = b.y, v[6] = b.z, v[7] = b.w;
    } else {
        v[0] = p[i];
    }
}
template <int V> __device__ __forceinline__ void st_f32v(float* p, int64_t i, const float* v) {
    if constexpr (V == 8) {
        *reinterpret_cast<float4*>(p + i) = make_float4(v[0], v[1], v[2], v[3]);
        *reinterpret_cast<float4*>(p + i + 4) = make_float4(v[4], v[5], v[6], v[7]);
    } else {
        p[i] = v[0];
    }
}
template <int DT, int V> __device__ __forceinline__ void ld_elemv(const uint8_t* p, int64_t i, float* v) {
    if constexpr (DT == APAD_F32) ld_f32v<V>(reinterpret_cast<const float*>(p), i, v);
    else if constexpr (V == 8) unpack8<DT>(*reinterpret_cast<const uint4*>(p + i * 2), v);
    else v[0] = ld_elem<DT>(p, i);
}
template <int DT, int V> __device__ __forceinline__ void st_elemv(uint8_t* p, int64_t i, const float* v) {
    if constexpr (DT == APAD_F32) st_f32v<V>(reinterpret_cast<float*>(p), i, v);
    else if constexpr (V == 8) *reinterpret_cast<uint4*>(p + i * 2) = pack8<DT>(v);
    else st_elem<DT>(p, i, v[0]);
}

// The forms of the step kernel: the 16-byte form (8 elements per access), the scalar form, and apad_cfg_ddim_step's (scalar, two-column table)
enum { STEP_DDIM = 0, STEP_SCALAR = 1, STEP_VEC = 8 };

// The sampler's update, linear in (x, eps, m1, z), with every rounding spelled out: contraction is off and each fused multiply-add is written
// as one.  The forms are the ones hipcc once chose for three separately compiled kernels, read off their gfx950 code (v_fma / v_fmac = fused,
// v_mul / v_pk_mul + v_add = not) and kept bit for bit: tests/golden/step_bits.safetensors holds what those kernels wrote, and
// tests/test_gpu_step_bits.py compares with it and restates each fp32 form on the host.
//   STEP_VEC, every dtype:   x' = fma(c_z, z, fma(c_m, m1, fma(c_x, x, c_e * e))),   m0 = fma(d_x, x, d_e * e)
//   STEP_SCALAR, fp32:       x' = fma(c_z, z, fma(c_m, m1, fma(c_e, e, c_x * x))),   m0 = d_x * x + d_e * e
//   STEP_SCALAR, 16-bit:     x' = ((c_x * x + c_e * e) + c_m * m1) + c_z * z,        m0 = d_x * x + d_e * e
//   STEP_DDIM, fp32:         x' = fma(c_x, x, c_e * e)      (v_mul_f32 c_e e; v_fmac_f32 c_x x)
//   STEP_DDIM, 16-bit:       x' = c_x * x + c_e * e         (v_pk_mul_f32 (c_x, c_e) (x, e); v_add_f32)
// STEP_DDIM has no m1 / z terms and no m0: it performs the two-column update's operations and no others.
template <int DT, int FORM>
__device__ __forceinline__ void sampler_update(float c_x, float c_e, float c_m, float c_z, float d_x, float d_e, float x, float e, float m1, float zz,
                                               float& xn, float& m0) {
#pragma clang fp contract(off)
    if constexpr (FORM == STEP_DDIM) {
        if constexpr (DT == APAD_F32) xn = fmaf(c_x, x, c_e * e);
        else xn = c_x * x + c_e * e;
        m0 = 0.f;  // not stored
    } else if constexpr (FORM == STEP_VEC) {
        xn = fmaf(c_z, zz, fmaf(c_m, m1, fmaf(c_x, x, c_e * e)));
        m0 = fmaf(d_x, x, d_e * e);
    } else if constexpr (DT == APAD_F32) {
        xn = fmaf(c_z, zz, fmaf(c_m, m1, fmaf(c_e, e, c_x * x)));
        m0 = d_x * x + d_e * e;
    } else {
        xn = ((c_x * x + c_e * e) + c_m * m1) + c_z * zz;
        m0 = d_x * x + d_e * e;
    }
}

// known = fma(kx, x0, kz * z0);  x' = fma(m, g, (1 - m) * known): m = 1 leaves the bits of g, m = 0 those of known, (kx, kz) = (1, 0) makes known x0
__device__ __forceinline__ float edit_known(float kx, float kz, float x0, float z0) {
#pragma clang fp contract(off)
    return fmaf(kx, x0, kz * z0);
}
__device__ __forceinline__ float edit_blend(float m, float g, float kx, float kz, float x0, float z0) {
#pragma clang fp contract(off)
    return fmaf(m, g, (1.0f - m) * edit_known(kx, kz, x0, z0));
}

// The guided noise, formed in the model dtype as the reference does, one device function per branch count.
// Two branches (eps = [e_u ; e_c], one scale, a kernel argument):
//   eps = (elem)fma(g, e_c - e_u, e_u)   (pipeline_audioldm2.py:1020-1025; one fp32 fma, one rounding to the model dtype)
// (f16 only, and the one fold still the compiler's: the scalar forms round the exact fma to f16 once, v_fma_mixlo_f16, the 16-byte form rounds
// it to fp32 first, v_cvt_pk_f16_f32 -- as before the kernels were merged, and pinned by the recorded bits)
template <int DT> __device__ __forceinline__ float guided_noise(float gs, float, const float (&e)[2]) {
    return (float)(typename ET<DT>::elem)fmaf(gs, e[1] - e[0], e[0]);
}
// Three branches (eps = [e_0 ; e_A ; e_AT]: no condition / audio prompt / audio prompt + text; InstructPix2Pix's two scales):
//   eps = (elem)fma(s_T, e_AT - e_A, fma(s_A, e_A - e_0, e_0))
// -- each difference and each fma rounded to fp32, one rounding to the model dtype.  The f16 rounding is pinned here (the fp32 fma first, in
// every form): the guidance values are arbitrary floats, and folding the store's rounding into the fma would move a rounding tie by a whole f16
// ulp against the written formula.
template <int DT> __device__ __forceinline__ float guided_noise(float s_a, float s_t, const float (&e)[3]) {
#pragma clang fp contract(off)
    float g = fmaf(s_t, e[2] - e[1], fmaf(s_a, e[1] - e[0], e[0]));
    if constexpr (DT == APAD_F16) asm volatile("" : "+v"(g));  // (the fp32 value exists before the f16 rounding: see above)
    return (float)(typename ET<DT>::elem)g;
}

// The denoise step's last kernel, behind all four entry points: the guided noise of NB = 2 or 3 branches (guided_noise; NB = 2 guides by the
// argument gs, NB = 3 by (s_A, s_T) = guidance[2 * step], apad_cfg_dual_step),
// then a sampler whose update is linear in (x, eps, m1, z) -- row r = coef + 6 * step (scheduler.py SAMPLER_COLS),
//   x' = r0 x + r1 eps + r2 m1 + r3 z[step],   m0 = r4 x + r5 eps -> hist (the next step's m1),   roundings as in sampler_update;
// DPM-Solver++ 2M: r3 = 0;  DDIM eta > 0: r2 = 0, no hist.  m1 / z are not read on a step whose coefficient is 0 (wave-uniform) -- then the
// edit blend (scheduler.py ``keep`` table, row s = (kx, kz)): with g the sampler's update,
//   known = fma(kx, x0, kz * z0)   -- the source at the noise level the step lands on ((1, 0) on the last step: the bits of x0)
//   x'    = fma(m, g, (1 - m) * known),  m = mask[pixel] in [0, 1]  -- m = 1 leaves the bits of g, m = 0 those of known
// mask fp32 [mask_batch][n / C], element j of a clip belongs to pixel j / C (NHWC, channel fastest).  STEP_VEC requires C == 8: one vector is
// one pixel and takes one mask value.  The data prediction m0 is formed from the pre-blend x and eps.  A null mask is m = 1 everywhere: the
// plain sampler step (apad_cfg_sampler_step).  STEP_DDIM (apad_cfg_ddim_step, deterministic DDIM) reads row coef + 2 * step = (c_x, c_e) of a
// table whose length the entry point is not told (no clamp), and has neither hist, noise nor mask.
template <int DT, int FORM, int NB>
__global__ __launch_bounds__(256) void cfg_step_kernel(const uint8_t* eps, float* latents, uint8_t* unet_in, float* eps_out, float* hist,
                                                       const float* noise, const float* coef, const float* keep, const float* x0, const float* z0,
                                                       const float* mask, int mask_per_clip, int C, int64_t n, const int32_t* step_ptr, int n_steps,
                                                       float gs, int64_t total, const float* guidance) {
    static_assert(NB == 2 || (NB == 3 && FORM != STEP_DDIM), "the two-column table has no three-branch form");
    constexpr int V = FORM == STEP_VEC ? 8 : 1;
    constexpr bool ddim = FORM == STEP_DDIM;
    if constexpr (ddim) hist = nullptr, noise = nullptr, mask = nullptr;
    int step = step_ptr ? *step_ptr : 0;
    if constexpr (!ddim) step = step < 0 ? 0 : (step >= n_steps ? n_steps - 1 : step);  // the tables and the noise buffer have n_steps rows
    const float* r = coef + (ddim ? 2 : 6) * step;
    const float c_x = r[0], c_e = r[1], c_m = ddim ? 0.f : r[2], c_z = ddim ? 0.f : r[3], d_x = ddim ? 0.f : r[4], d_e = ddim ? 0.f : r[5];
    const float s_a = NB == 3 ? guidance[2 * step] : gs, s_t = NB == 3 ? guidance[2 * step + 1] : 0.f;
    const float kx = mask ? keep[2 * step] : 0.f, kz = mask ? keep[2 * step + 1] : 0.f;
    const bool use_m1 = hist && c_m != 0.f, use_z = noise && c_z != 0.f;
    const float* z = noise + (use_z ? (int64_t)step * total : 0);
    const int64_t npix = n / C;  // pixels per clip
    for (int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * V; i < total; i += (int64_t)gridDim.x * 256 * V) {
        float eb[NB][V], x[V], m1[V], zz[V], e[V], m0[V];
#pragma unroll
        for (int b = 0; b < NB; ++b) ld_elemv<DT, V>(eps, b * total + i, eb[b]);
        ld_f32v<V>(latents, i, x);
#pragma unroll
        for (int j = 0; j < V; ++j) m1[j] = zz[j] = 0.f;
        if (use_m1) ld_f32v<V>(hist, i, m1);
        if (use_z) ld_f32v<V>(z, i, zz);
#pragma unroll
        for (int j = 0; j < V; ++j) {
            float ej[NB];
#pragma unroll
            for (int b = 0; b < NB; ++b) ej[b] = eb[b][j];
            e[j] = guided_noise<DT>(s_a, s_t, ej);
            float xn;
            sampler_update<DT, FORM>(c_x, c_e, c_m, c_z, d_x, d_e, x[j], e[j], m1[j], zz[j], xn, m0[j]);
            x[j] = xn;
        }
        if (mask) {
            const int64_t pix = V == 8 ? (i >> 3) : i / C;  // over the whole batch: clip * npix + pixel
            const float m = mask[mask_per_clip ? pix : pix % npix];
            float a[V], b[V];
            ld_f32v<V>(x0, i, a);
            ld_f32v<V>(z0, i, b);
#pragma unroll
            for (int j = 0; j < V; ++j) x[j] = edit_blend(m, x[j], kx, kz, a[j], b[j]);
        }
        st_f32v<V>(latents, i, x);
        st_elemv<DT, V>(unet_in, i, x);
        if (hist) st_f32v<V>(hist, i, m0);
        if (eps_out) st_f32v<V>(eps_out, i, e);
    }
}

// ---- shaped guidance: guidance rescale and adaptive projected guidance, the per-clip sums inside the step (apad_cfg_shaped_step) ----
//
// cfg_step_kernel with another guided-noise stage; everything after eps -- sampler_update, history, noise table, edit_blend, mask indexing,
// eps_out -- is that kernel's, statement for statement.  The stage needs sums over a whole clip (n = h * w * C values), so ONE workgroup of 1024
// threads owns a clip (gridDim.x = B) and walks it up to three times; a clip is at most a few hundred KB and stays in L2 between the passes.
//
// Per clip b and step s = *step_ptr clamped to [0, n_steps), operands widened to fp32, every sum over the clip's n elements.  Branches as in
// guided_noise: NB = 2: e_0, c = e_1, one difference d_1 = c - e_0 with weight w_1 = gs;  NB = 3: e_0, e_A, c = e_AT, d_1 = e_A - e_0 (w_1 = s_A),
// d_2 = e_AT - e_A (w_2 = s_T), the weights from the guidance table.  Row s of shape [n_steps][4] fp32 is (phi, eta, r, beta):
//   1. momentum      beta != 0:  m_k <- fma(beta, m_k, d_k) -> momentum [NB - 1][B][n] fp32, and d_k := m_k.  beta == 0: neither read nor written.
//   2. norm          r > 0:  t_k = min(1, r / ||d_k||_2), a zero norm gives 1;  otherwise t_k = 1.
//   3. projection    p_k = <d_k, c> / <c, c>, a zero denominator gives 0;  q_k = (1 - eta) p_k (eta == 1: q_k = 0, nothing divided);
//                    u_k = t_k * fma(-q_k, c, d_k)  -- orthogonal + eta * parallel = d - (1 - eta) * parallel (Sadat et al. 2024)
//   4. guided noise  g = fma(w_2, u_2, fma(w_1, u_1, e_0))  (NB = 2: fma(w_1, u_1, e_0)) -- diffusers' non-original APG form, plain CFG at eta = 1
//   5. rescale       phi > 0:  f = fma(phi, std(c) / std(g), 1 - phi), std(g) == 0 or n == 1 gives f = 1;  g <- f * g.  std is the unbiased one
//                    (n - 1), from centred values: sqrt(sum (x - mean)^2 / (n - 1))  (Lin et al. 2024)
//   6. eps = (dtype) g, the fp32 value rounded once, in every form and dtype (asm barrier for f16, as the three-branch guided_noise)
// A factor that is off is not applied at all: q_k == 0 skips the fma, t_k == 1 and phi == 0 skip the multiplies.  So the row (0, 1, 0, 0) leaves
// u_k the bits of d_k and g the very fma chain of guided_noise: the kernel then writes cfg_step_kernel's bits (except where that kernel leaves
// the f16 rounding to the compiler: two branches, f16, scalar form), and a schedule may switch the stage on for part of a run.
//
// Passes, each thread visiting the same elements in each (thread t: vectors t, t + 1024, ...), so what pass 1 stores pass 3 re-reads itself:
//   pass 1 (any of beta != 0, r > 0, eta != 1, phi > 0)   momentum update;  <d_k, c>, <d_k, d_k>, sum d_k, <c, c>, sum c, sum e_0.
//          mean(g) follows from these: g is linear in the vectors once t_k, q_k are known.
//   pass 2 (phi > 0 and n > 1)                            sum (g - mean g)^2, sum (c - mean c)^2
//   pass 3                                                g, f, eps, then the step
// Sums: each thread adds its elements in index order (fma for the products), a xor butterfly inside the wave (a + b == b + a: every lane holds the
// same bits), the 16 wave sums through LDS, added in order 0 .. 15 by one thread per sum and read back by all.  The order depends on n and the form only, so a clip's
// outputs are the same bits whatever B is and wherever the clip sits in the batch.  No atomics, no host reads.
// stats (optional) [B][8] fp32 = (t_1, q_1, t_2, q_2, mean g, std g, std c, f) per clip; NB = 2: (t_2, q_2) = (1, 0); phi == 0: (0, 0, 0, 1) in
// the last four (not computed).  STEP_VEC additionally needs 8 | n: a clip must start on a 16-byte boundary.
constexpr int SHAPED_THREADS = 1024, SHAPED_WAVES = SHAPED_THREADS / 64;

template <int NS> __device__ __forceinline__ void shaped_block_sum(float (&v)[NS], float (*part)[SHAPED_WAVES]) {
#pragma unroll
    for (int k = 0; k < NS; ++k) v[k] = wave_sum(v[k]);
    __syncthreads();  // (the previous sum's partials have been read by everyone)
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < NS; ++k) part[k][threadIdx.x >> 6] = v[k];
    }
    __syncthreads();
    if (threadIdx.x < NS) {  // thread k adds sum k's wave partials in order 0 .. 15
        float s = part[threadIdx.x][0];
#pragma unroll
        for (int w = 1; w < SHAPED_WAVES; ++w) s += part[threadIdx.x][w];
        part[threadIdx.x][0] = s;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < NS; ++k) v[k] = part[k][0];
}

// e_0, c and the NB - 1 differences of elements i .. i + V of the batch; with ``m`` (a momentum row, after pass 1) the running averages instead
template <int DT, int V, int NB>
__device__ __forceinline__ void shaped_load(const uint8_t* eps, const float* m, int64_t total, int64_t i, float (&e0)[V], float (&c)[V],
                                            float (&d)[NB - 1][V]) {
    float eb[NB][V];
#pragma unroll
    for (int b = 0; b < NB; ++b) ld_elemv<DT, V>(eps, b * total + i, eb[b]);
#pragma unroll
    for (int j = 0; j < V; ++j) e0[j] = eb[0][j], c[j] = eb[NB - 1][j];
#pragma unroll
    for (int k = 0; k < NB - 1; ++k) {
        if (m) {
            ld_f32v<V>(m, k * total + i, d[k]);
        } else {
#pragma unroll
            for (int j = 0; j < V; ++j) d[k][j] = eb[k + 1][j] - eb[k][j];
        }
    }
}

// steps 3 and 4 for one element: g before the rescale
template <int K> __device__ __forceinline__ float shaped_guided(float e0, float c, const float (&d)[K], const float (&w)[K], const float (&t)[K],
                                                                const float (&q)[K]) {
#pragma clang fp contract(off)
    float g = e0;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        float u = d[k];
        if (q[k] != 0.f) u = fmaf(-q[k], c, u);
        if (t[k] != 1.f) u = t[k] * u;
        g = fmaf(w[k], u, g);
    }
    return g;
}

template <int DT, int FORM, int NB>
__global__ __launch_bounds__(SHAPED_THREADS) void cfg_shaped_step_kernel(const uint8_t* eps, float* latents, uint8_t* unet_in, float* eps_out, float* hist,
                                                                         const float* noise, const float* coef, const float* keep, const float* x0,
                                                                         const float* z0, const float* mask, int mask_per_clip, int C, int64_t n,
                                                                         const int32_t* step_ptr, int n_steps, float gs, int64_t total,
                                                                         const float* guidance, const float* shape, float* momentum, float* stats) {
#pragma clang fp contract(off)
    static_assert(FORM == STEP_VEC || FORM == STEP_SCALAR, "the shaped step reads the six-column table");
    constexpr int V = FORM == STEP_VEC ? 8 : 1, K = NB - 1, NS = 3 * K + 3;
    __shared__ float part[NS][SHAPED_WAVES];
    int step = step_ptr ? *step_ptr : 0;
    step = step < 0 ? 0 : (step >= n_steps ? n_steps - 1 : step);
    const float* r = coef + 6 * step;
    const float c_x = r[0], c_e = r[1], c_m = r[2], c_z = r[3], d_x = r[4], d_e = r[5];
    float w[K], t[K], q[K];
    w[0] = NB == 3 ? guidance[2 * step] : gs;
    if constexpr (NB == 3) w[1] = guidance[2 * step + 1];
#pragma unroll
    for (int k = 0; k < K; ++k) t[k] = 1.f, q[k] = 0.f;
    const float phi = shape[4 * step], eta = shape[4 * step + 1], rr = shape[4 * step + 2], beta = momentum ? shape[4 * step + 3] : 0.f;
    const float kx = mask ? keep[2 * step] : 0.f, kz = mask ? keep[2 * step + 1] : 0.f;
    const bool use_m1 = hist && c_m != 0.f, use_z = noise && c_z != 0.f;
    const float* z = noise + (use_z ? (int64_t)step * total : 0);
    const int64_t npix = n / C;                  // pixels per clip
    const int64_t base = (int64_t)blockIdx.x * n;  // this workgroup's clip
    const int64_t first = (int64_t)threadIdx.x * V, stride = (int64_t)SHAPED_THREADS * V;
    const float* mom = beta != 0.f ? momentum : nullptr;  // where passes 2 and 3 find d_k
    float f = 1.f, mean_g = 0.f, mean_c = 0.f, std_g = 0.f, std_c = 0.f;

    if (beta != 0.f || rr > 0.f || eta != 1.f || phi > 0.f) {  // pass 1
        float s[NS];  // per k: <d_k, c>, <d_k, d_k>, sum d_k;  then <c, c>, sum c, sum e_0
#pragma unroll
        for (int k = 0; k < NS; ++k) s[k] = 0.f;
        for (int64_t j = first; j < n; j += stride) {
            const int64_t i = base + j;
            float e0[V], c[V], d[K][V];
            shaped_load<DT, V, NB>(eps, nullptr, total, i, e0, c, d);
            if (mom) {
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    float m[V];
                    ld_f32v<V>(momentum, k * total + i, m);
#pragma unroll
                    for (int l = 0; l < V; ++l) d[k][l] = fmaf(beta, m[l], d[k][l]);
                    st_f32v<V>(momentum, k * total + i, d[k]);
                }
            }
#pragma unroll
            for (int l = 0; l < V; ++l) {
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    s[3 * k] = fmaf(d[k][l], c[l], s[3 * k]);
                    s[3 * k + 1] = fmaf(d[k][l], d[k][l], s[3 * k + 1]);
                    s[3 * k + 2] += d[k][l];
                }
                s[3 * K] = fmaf(c[l], c[l], s[3 * K]);
                s[3 * K + 1] += c[l];
                s[3 * K + 2] += e0[l];
            }
        }
        shaped_block_sum<NS>(s, part);
        float sum_g = s[3 * K + 2];
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const float nrm = sqrtf(s[3 * k + 1]);
            if (rr > 0.f && nrm > rr) t[k] = rr / nrm;
            if (eta != 1.f && s[3 * K] != 0.f) q[k] = (1.f - eta) * (s[3 * k] / s[3 * K]);
            sum_g = fmaf(w[k] * t[k], fmaf(-q[k], s[3 * K + 1], s[3 * k + 2]), sum_g);
        }
        if (phi > 0.f) mean_g = sum_g / (float)n, mean_c = s[3 * K + 1] / (float)n;
    }

    if (phi > 0.f && n > 1) {  // pass 2
        float s[2] = {0.f, 0.f};
        for (int64_t j = first; j < n; j += stride) {
            float e0[V], c[V], d[K][V];
            shaped_load<DT, V, NB>(eps, mom, total, base + j, e0, c, d);
#pragma unroll
            for (int l = 0; l < V; ++l) {
                float dl[K];
#pragma unroll
                for (int k = 0; k < K; ++k) dl[k] = d[k][l];
                const float a = shaped_guided<K>(e0[l], c[l], dl, w, t, q) - mean_g, b = c[l] - mean_c;
                s[0] = fmaf(a, a, s[0]);
                s[1] = fmaf(b, b, s[1]);
            }
        }
        shaped_block_sum<2>(s, part);
        std_g = sqrtf(s[0] / (float)(n - 1)), std_c = sqrtf(s[1] / (float)(n - 1));
        if (std_g != 0.f) f = fmaf(phi, std_c / std_g, 1.f - phi);
    }
    if (stats && threadIdx.x == 0) {
        float* o = stats + 8 * (int64_t)blockIdx.x;
        o[0] = t[0], o[1] = q[0], o[2] = t[K - 1], o[3] = q[K - 1];
        if constexpr (NB == 2) o[2] = 1.f, o[3] = 0.f;
        o[4] = mean_g, o[5] = std_g, o[6] = std_c, o[7] = f;
    }

    for (int64_t j = first; j < n; j += stride) {  // pass 3: cfg_step_kernel's body on the shaped noise
        const int64_t i = base + j;
        float e0[V], c[V], d[K][V], x[V], m1[V], zz[V], e[V], m0[V];
        shaped_load<DT, V, NB>(eps, mom, total, i, e0, c, d);
        ld_f32v<V>(latents, i, x);
#pragma unroll
        for (int l = 0; l < V; ++l) m1[l] = zz[l] = 0.f;
        if (use_m1) ld_f32v<V>(hist, i, m1);
        if (use_z) ld_f32v<V>(z, i, zz);
#pragma unroll
        for (int l = 0; l < V; ++l) {
            float dl[K];
#pragma unroll
            for (int k = 0; k < K; ++k) dl[k] = d[k][l];
            float g = shaped_guided<K>(e0[l], c[l], dl, w, t, q);
            if (phi > 0.f) g = f * g;
            if constexpr (DT == APAD_F16) asm volatile("" : "+v"(g));  // (the fp32 value exists before the f16 rounding)
            e[l] = (float)(typename ET<DT>::elem)g;
            float xn;
            sampler_update<DT, FORM>(c_x, c_e, c_m, c_z, d_x, d_e, x[l], e[l], m1[l], zz[l], xn, m0[l]);
            x[l] = xn;
        }
        if (mask) {
            const int64_t pix = V == 8 ? (i >> 3) : i / C;  // over the whole batch: clip * npix + pixel
            const float m = mask[mask_per_clip ? pix : pix % npix];
            float a[V], b[V];
            ld_f32v<V>(x0, i, a);
            ld_f32v<V>(z0, i, b);
#pragma unroll
            for (int l = 0; l < V; ++l) x[l] = edit_blend(m, x[l], kx, kz, a[l], b[l]);
        }
        st_f32v<V>(latents, i, x);
        st_elemv<DT, V>(unet_in, i, x);
        if (hist) st_f32v<V>(hist, i, m0);
        if (eps_out) st_f32v<V>(eps_out, i, e);
    }
}

// The three buffers an edit run starts from, in the loop's layout (NHWC, [rows = B * h * w][Lc]), in one pass:
//   x0 = (mean + exp(0.5 * clamp(logvar, -30, 20)) * post_noise) * scale   (gaussian_sample_kernel's draw, kept in fp32; or, with null moments,
//        the x0 already there),   latents = fma(a, x0, s * z0)   (add_noise at the start timestep),   unet_in = latents in the model dtype.
// V = 8 requires Lc == 8: one vector is one latent pixel, its mean at moments + 16 * row and its logvar 8 elements further.
template <int DT, int V>
__global__ __launch_bounds__(256) void edit_start_kernel(const uint8_t* moments, const float* post_noise, const float* z0, float* x0, float* latents,
                                                         uint8_t* unet_in, float a, float s, float scale, int64_t total, int Lc) {
    for (int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * V; i < total; i += (int64_t)gridDim.x * 256 * V) {
        float x[V], zz[V];
        if (moments) {
            const int64_t row = V == 8 ? (i >> 3) : i / Lc;
            const int64_t mo = row * 2 * Lc + (i - row * Lc);
            float mean[V], lv[V], pn[V];
            ld_elemv<DT, V>(moments, mo, mean);
            ld_elemv<DT, V>(moments, mo + Lc, lv);
            ld_f32v<V>(post_noise, i, pn);
#pragma unroll
            for (int j = 0; j < V; ++j) x[j] = (mean[j] + expf(0.5f * fminf(fmaxf(lv[j], -30.0f), 20.0f)) * pn[j]) * scale;
            st_f32v<V>(x0, i, x);
        } else {
            ld_f32v<V>(x0, i, x);
        }
        ld_f32v<V>(z0, i, zz);
#pragma unroll
        for (int j = 0; j < V; ++j) {
            x[j] = edit_known(a, s, x[j], zz[j]);  // the source at the start timestep's noise level
            // unet_in is the copy of the fp32 master: keep the compiler from folding the f16 store into the multiply-add (v_fma_mixlo_f16
            // rounds the exact sum once, and the copy would differ from the rounded master in the last f16 bit)
            asm volatile("" : "+v"(x[j]));
        }
        st_f32v<V>(latents, i, x);
        st_elemv<DT, V>(unet_in, i, x);
    }
}

// z = (x' - mu) / std: one fp32 subtraction and one IEEE fp32 division (correctly rounded, v_div_scale / v_div_fmas / v_div_fixup), nothing
// fused into either.  std == 0 (a deterministic row: the step adds no noise, so there is none to extract) gives z = 0, never inf or NaN.
__device__ __forceinline__ float invert_noise(float xn, float mu, float sd) {
#pragma clang fp contract(off)
    const float d = xn - mu;
    return sd != 0.f ? d / sd : 0.f;
}

// The guided noise as cfg_step_kernel<DT, FORM, NB> forms it, so that the inversion and the sampler step that consumes its z see the same eps
// bits: guided_noise, except for the one fold that function leaves to the compiler (f16, two branches).  The step kernel's 16-byte form
// rounds the fma to fp32 and then to f16 (v_cvt_pk_f16_f32), its scalar form rounds the exact fma once (v_fma_mixlo_f16); here the compiler
// chooses the single rounding in both forms, so the 16-byte form is pinned to the step kernel's two roundings.
template <int DT, int FORM> __device__ __forceinline__ float invert_guided_noise(float gs, float, const float (&e)[2]) {
    if constexpr (DT == APAD_F16 && FORM == STEP_VEC) {
        float g = fmaf(gs, e[1] - e[0], e[0]);
        asm volatile("" : "+v"(g));
        return (float)(typename ET<DT>::elem)g;
    } else {
        return guided_noise<DT>(gs, 0.f, e);
    }
}
template <int DT, int FORM> __device__ __forceinline__ float invert_guided_noise(float s_a, float s_t, const float (&e)[3]) {
    return guided_noise<DT>(s_a, s_t, e);
}

// Edit-friendly DDPM inversion (Huberman-Spiegelglas et al. 2024), the step that EXTRACTS a stochastic sampler's noise instead of
// consuming it -- cfg_step_kernel's layout, grid, step clamp, guided noise and forms (STEP_VEC / STEP_SCALAR), at the end of the same captured
// UNet step.  With row r = coef + 6 * step = (c_x, c_e, -, std, -, -), (kx, kz) = keep[2 * step] and n~ = noise[step] (an independent draw):
//   eps = guided_noise<DT>(branches at x)                            the source condition's guided noise, as the sampler forms it
//                                                                     (invert_guided_noise)
//   mu  = sampler_update<DT, FORM>'s c_x x + c_e eps                 (c_m = c_z = 0, m1 = z = 0: the same operations in the same order, so
//                                                                     STEP_VEC: fma(c_x, x, c_e * e);  STEP_SCALAR fp32: fma(c_e, e, c_x * x);
//                                                                     STEP_SCALAR 16-bit: c_x * x + c_e * e -- the added zeros change no bit
//                                                                     of a nonzero mu)
//   x'  = edit_known(kx, kz, x0, n~) = fma(kx, x0, kz * n~)          the source at the noise level the step lands on; (1, 0) on the last row:
//                                                                     the bits of x0
//   z   = (x' - mu) / std   (invert_noise)                           -> written over n~, row ``step`` of the noise table
//   latents = x',  unet_in = (model dtype) x'
// so that the sampler's own step from x with the same eps and noise = z gives fma(std, z, mu) = x' up to the roundings of z.  x is only read to
// form mu: the trajectory x_(i) is independent of the UNet, the z_i are not.
template <int DT, int FORM, int NB>
__global__ __launch_bounds__(256) void cfg_invert_step_kernel(const uint8_t* eps, float* latents, uint8_t* unet_in, float* eps_out, float* noise,
                                                              const float* coef, const float* keep, const float* x0, const int32_t* step_ptr,
                                                              int n_steps, float gs, int64_t total, const float* guidance) {
    static_assert(FORM == STEP_VEC || FORM == STEP_SCALAR, "the two-column table has no noise column to invert into");
    constexpr int V = FORM == STEP_VEC ? 8 : 1;
    int step = step_ptr ? *step_ptr : 0;
    step = step < 0 ? 0 : (step >= n_steps ? n_steps - 1 : step);  // the tables and the noise buffer have n_steps rows
    const float* r = coef + 6 * step;
    const float c_x = r[0], c_e = r[1], sd = r[3];
    const float s_a = NB == 3 ? guidance[2 * step] : gs, s_t = NB == 3 ? guidance[2 * step + 1] : 0.f;
    const float kx = keep[2 * step], kz = keep[2 * step + 1];
    float* z = noise + (int64_t)step * total;
    for (int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * V; i < total; i += (int64_t)gridDim.x * 256 * V) {
        float eb[NB][V], x[V], a[V], zz[V], e[V];
#pragma unroll
        for (int b = 0; b < NB; ++b) ld_elemv<DT, V>(eps, b * total + i, eb[b]);
        ld_f32v<V>(latents, i, x);
        ld_f32v<V>(x0, i, a);
        ld_f32v<V>(z, i, zz);
#pragma unroll
        for (int j = 0; j < V; ++j) {
            float ej[NB];
#pragma unroll
            for (int b = 0; b < NB; ++b) ej[b] = eb[b][j];
            e[j] = invert_guided_noise<DT, FORM>(s_a, s_t, ej);
            float mu, m0;
            sampler_update<DT, FORM>(c_x, c_e, 0.f, 0.f, 0.f, 0.f, x[j], e[j], 0.f, 0.f, mu, m0);
            x[j] = edit_known(kx, kz, a[j], zz[j]);
            asm volatile("" : "+v"(x[j]));  // unet_in is the rounded copy of the fp32 master (see edit_start_kernel)
            zz[j] = invert_noise(x[j], mu, sd);
        }
        st_f32v<V>(latents, i, x);
        st_elemv<DT, V>(unet_in, i, x);
        st_f32v<V>(z, i, zz);
        if (eps_out) st_f32v<V>(eps_out, i, e);
    }
}

__global__ void step_advance_kernel(int32_t* p) { *p = *p + 1; }

template <int DT> __global__ __launch_bounds__(256) void mix3_kernel(const uint8_t* a, const uint8_t* b, const uint8_t* c, uint8_t* out, int64_t n,
                                                                     float scale) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
        st_elem<DT>(out, i, (ld_elem<DT>(a, i) + ld_elem<DT>(b, i) + ld_elem<DT>(c, i)) * scale);
}

// out[m][n] = softmax_n(scale * x[m][n]); one wave per row, statistics and exponentials in fp32 (libm expf: the op runs once per
// decoded clip, not per denoise step).  Serves the VAE mid-block's single-head d = 512 attention, which lies outside
// apad_attention's head-dim envelope and runs as apad_gemm (Q.K^T) -> this -> apad_gemm (P.V).
template <int DT> __global__ __launch_bounds__(256) void softmax_rows_kernel(const uint8_t* x, const float* bias, uint8_t* out, int64_t M, int N,
                                                                             int64_t ldx, int64_t ldb, int64_t ldo, float scale) {
    const int lane = threadIdx.x & 63;
    const int64_t m = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (m >= M) return;
    const int64_t xo = m * ldx, oo = m * ldo;
    const float* bm = bias ? bias + m * ldb : nullptr;
    auto at = [&](int n) { return ld_elem<DT>(x, xo + n) * scale + (bm ? bm[n] : 0.f); };
    float mx = -INFINITY;
    for (int n = lane; n < N; n += 64) mx = fmaxf(mx, at(n));
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
    if (mx == -INFINITY) mx = 0.f;  // a fully masked row: exp(-inf) = 0 everywhere, written as zeros below
    float sum = 0.f;
    for (int n = lane; n < N; n += 64) sum += expf(at(n) - mx);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
    const float inv = sum > 0.f ? 1.0f / sum : 0.f;
    for (int n = lane; n < N; n += 64) st_elem<DT>(out, oo + n, expf(at(n) - mx) * inv);
}

// T5LayerNorm (mode 0: x * rsqrt(mean(x^2) + eps) * gamma) and F.normalize (mode 1: x / max(||x||, eps)); one wave per row
template <int DT> __global__ __launch_bounds__(256) void rmsnorm_kernel(const uint8_t* x, const uint8_t* gamma, uint8_t* out, int64_t M, int C,
                                                                        int64_t ldx, int64_t ldo, float eps, int mode) {
    const int lane = threadIdx.x & 63;
    const int64_t m = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (m >= M) return;
    float ss = 0.f;
    for (int c = lane; c < C; c += 64) {
        const float v = ld_elem<DT>(x, m * ldx + c);
        ss = fmaf(v, v, ss);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) ss += __shfl_xor(ss, o);
    const float r = mode == 0 ? 1.0f / sqrtf(ss / (float)C + eps) : 1.0f / fmaxf(sqrtf(ss), eps);
    for (int c = lane; c < C; c += 64) st_elem<DT>(out, m * ldo + c, ld_elem<DT>(x, m * ldx + c) * r * (mode == 0 ? ld_elem<DT>(gamma, c) : 1.0f));
}

// nn.Embedding: one wave per output row
template <int DT> __global__ __launch_bounds__(256) void gather_rows_kernel(const uint8_t* table, const int64_t* ids, uint8_t* out, int64_t n,
                                                                            int64_t rows, int C) {
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= n) return;
    const int64_t id = ids[i];
    const bool ok = id >= 0 && id < rows;
    for (int c = lane; c < C; c += 64) st_elem<DT>(out, i * C + c, ok ? ld_elem<DT>(table, id * C + c) : 0.f);
}

// DiagonalGaussianDistribution.sample() of the VAE encoder: moments [rows][2L] = (mean | logvar) per latent pixel ->
// out [rows][L] = (mean + exp(0.5 * clamp(logvar, -30, 20)) * noise) * scale  (scale = the pipeline's scaling_factor, or 1)
template <int DT> __global__ __launch_bounds__(256) void gaussian_sample_kernel(const uint8_t* moments, const uint8_t* noise, uint8_t* out,
                                                                                int64_t rows, int L, float scale) {
    const int64_t n = rows * L;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int64_t r = i / L;
        const int c = (int)(i - r * L);
        const float mean = ld_elem<DT>(moments, r * 2 * L + c);
        const float logvar = fminf(fmaxf(ld_elem<DT>(moments, r * 2 * L + L + c), -30.0f), 20.0f);
        st_elem<DT>(out, i, (mean + expf(0.5f * logvar) * ld_elem<DT>(noise, i)) * scale);
    }
}

}  // namespace

extern "C" int apad_audiomae_pool(const void* rep, void* out, int32_t B, int32_t tp, int32_t fp, int32_t dtype,
                                  int32_t out_dtype, void* stream) {
    APAD_CHECK(rep && out && B > 0, "apad_audiomae_pool: null operand / empty batch");
    if (dtype == APAD_F32) {
        APAD_CHECK(out_dtype == APAD_F32, "apad_audiomae_pool: f32 input needs f32 output");
        APAD_CHECK(tp > 0 && fp > 0 && 64 % tp == 0 && 8 % fp == 0, "apad_audiomae_pool: pooling (%d,%d) must divide (64,8)", tp, fp);
        return apad_f32_audiomae_pool(rep, out, B, tp, fp, (hipStream_t)stream);
    }
    APAD_CHECK(dtype == APAD_BF16 || dtype == APAD_F16, "apad_audiomae_pool: dtype %d not supported", dtype);
    APAD_CHECK(out_dtype == dtype || out_dtype == APAD_F32, "apad_audiomae_pool: out_dtype must equal dtype or be f32");
    APAD_CHECK(tp > 0 && fp > 0 && 64 % tp == 0 && 8 % fp == 0, "apad_audiomae_pool: pooling (%d,%d) must divide (64,8)", tp, fp);
    const int64_t total = (int64_t)B * (64 / tp) * (8 / fp) * 96;
    int64_t blocks = (total + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    hipStream_t s = (hipStream_t)stream;
    const uint8_t* r = (const uint8_t*)rep;
    uint8_t* o = (uint8_t*)out;
    if (dtype == APAD_BF16) {
        if (out_dtype == APAD_F32)
            hipLaunchKernelGGL((pool_kernel<APAD_BF16, APAD_F32>), dim3((unsigned)blocks), dim3(256), 0, s, r, o, B, tp, fp);
        else
            hipLaunchKernelGGL((pool_kernel<APAD_BF16, APAD_BF16>), dim3((unsigned)blocks), dim3(256), 0, s, r, o, B, tp, fp);
    } else {
        if (out_dtype == APAD_F32)
            hipLaunchKernelGGL((pool_kernel<APAD_F16, APAD_F32>), dim3((unsigned)blocks), dim3(256), 0, s, r, o, B, tp, fp);
        else
            hipLaunchKernelGGL((pool_kernel<APAD_F16, APAD_F16>), dim3((unsigned)blocks), dim3(256), 0, s, r, o, B, tp, fp);
    }
    return apad_check_launch("apad_audiomae_pool");
}

extern "C" int apad_timestep_embedding(const float* t, void* out, int32_t n, int32_t dim, int32_t flip_sin_to_cos,
                                       float freq_shift, int32_t dtype, void* stream) {
    APAD_CHECK(t && out && n > 0 && dim > 0 && dim % 2 == 0, "apad_timestep_embedding: bad arguments");
    APAD_CHECK(dtype == APAD_BF16 || dtype == APAD_F16 || dtype == APAD_F32, "apad_timestep_embedding: dtype %d not supported", dtype);
    const int total = n * (dim / 2);
    dim3 grid((total + 255) / 256);
    hipStream_t s = (hipStream_t)stream;
    LAUNCH_DT(timestep_kernel, grid, t, (uint8_t*)out, n, dim, flip_sin_to_cos, freq_shift);
    return apad_check_launch("apad_timestep_embedding");
}

namespace {

// what a step entry point hands to step_launch: its own arguments, null / 0 where it has none
struct StepOperands {
    const void* eps;  // [branches * B][n] in the model dtype
    float* latents;
    void* unet_in;
    float *eps_out, *history;
    const float *noise, *coef, *guidance, *keep, *x0, *z0, *mask;
    int mask_batch, C;
    const int32_t* step_ptr;
    int n_steps;
    float gs;
    int B;
    int64_t n;
    int dtype;
    void* stream;
    int branches;  // 2, or 3: the guidance table instead of gs
    bool ddim;     // apad_cfg_ddim_step: two-column table of a length it is not told, scalar form only
    // apad_cfg_shaped_step (cfg_shaped_step_kernel, one workgroup per clip): the (phi, eta, r, beta) table, and null or its optional buffers
    const float* shape;
    float *momentum, *stats;
};

using step_kernel_t = decltype(&cfg_step_kernel<APAD_BF16, STEP_VEC, 2>);
template <int DT> step_kernel_t step_kernel(int form, int branches) {
    if (branches == 3) return form == STEP_VEC ? cfg_step_kernel<DT, STEP_VEC, 3> : cfg_step_kernel<DT, STEP_SCALAR, 3>;
    return form == STEP_VEC ? cfg_step_kernel<DT, STEP_VEC, 2> : form == STEP_SCALAR ? cfg_step_kernel<DT, STEP_SCALAR, 2> : cfg_step_kernel<DT, STEP_DDIM, 2>;
}

using shaped_kernel_t = decltype(&cfg_shaped_step_kernel<APAD_BF16, STEP_VEC, 2>);
template <int DT> shaped_kernel_t shaped_kernel(bool vec, int branches) {
    if (branches == 3) return vec ? cfg_shaped_step_kernel<DT, STEP_VEC, 3> : cfg_shaped_step_kernel<DT, STEP_SCALAR, 3>;
    return vec ? cfg_shaped_step_kernel<DT, STEP_VEC, 2> : cfg_shaped_step_kernel<DT, STEP_SCALAR, 2>;
}

// Every check, the choice of form, the grid and the launch of the step entry points; ``fn`` prefixes the messages.
int step_launch(const char* fn, const StepOperands& a) {
    APAD_CHECK(a.eps && a.latents && a.unet_in && a.coef, "%s: null operand", fn);
    APAD_CHECK(a.branches == 2 || a.guidance, "%s: null guidance table", fn);
    APAD_CHECK(a.dtype == APAD_BF16 || a.dtype == APAD_F16 || a.dtype == APAD_F32, "%s: dtype %d not supported", fn, a.dtype);
    APAD_CHECK(a.B > 0 && a.n > 0 && (a.ddim || a.n_steps > 0), "%s: empty problem", fn);
    if (a.mask) {
        APAD_CHECK(a.keep && a.x0 && a.z0, "%s: a mask needs the keep table, x0 and z0 (null operand)", fn);
        APAD_CHECK(a.mask_batch == 1 || a.mask_batch == a.B, "%s: mask_batch %d must be 1 or B = %d", fn, a.mask_batch, a.B);
        APAD_CHECK(a.C > 0 && a.n % a.C == 0, "%s: n = %lld is not a multiple of C = %d", fn, (long long)a.n, a.C);
    }
    const int64_t total = (int64_t)a.B * a.n;
    // 16-byte accesses need every non-null base 16-byte aligned and 8 | total (then every further branch and every noise row is aligned too), and
    // with a mask C == 8, which makes one 8-element vector one pixel.  apad_cfg_ddim_step launches the scalar form only: the 16-byte form rounds
    // differently (sampler_update)
    const uintptr_t bases = (uintptr_t)a.eps | (uintptr_t)a.latents | (uintptr_t)a.unet_in | (uintptr_t)a.eps_out | (uintptr_t)a.history |
                            (uintptr_t)a.noise | (uintptr_t)a.x0 | (uintptr_t)a.z0 | (uintptr_t)a.momentum;
    const bool vec = !a.ddim && total % 8 == 0 && bases % 16 == 0 && (!a.mask || a.C == 8);
    const int per_clip = a.mask_batch == a.B && a.B > 1;
    if (a.shape) {  // one workgroup per clip, which must then start on a 16-byte boundary for the 16-byte form: 8 | n
        const bool svec = vec && a.n % 8 == 0;
        const shaped_kernel_t kern = a.dtype == APAD_BF16  ? shaped_kernel<APAD_BF16>(svec, a.branches)
                                     : a.dtype == APAD_F32 ? shaped_kernel<APAD_F32>(svec, a.branches)
                                                           : shaped_kernel<APAD_F16>(svec, a.branches);
        hipLaunchKernelGGL(kern, dim3((unsigned)a.B), dim3(SHAPED_THREADS), 0, (hipStream_t)a.stream, (const uint8_t*)a.eps, a.latents,
                           (uint8_t*)a.unet_in, a.eps_out, a.history, a.noise, a.coef, a.keep, a.x0, a.z0, a.mask, per_clip, a.mask ? a.C : 1, a.n,
                           a.step_ptr, a.n_steps, a.gs, total, a.guidance, a.shape, a.momentum, a.stats);
        return apad_check_launch(fn);
    }
    int64_t blocks = ((vec ? total / 8 : total) + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    const int form = a.ddim ? STEP_DDIM : vec ? STEP_VEC : STEP_SCALAR;
    const step_kernel_t kern = a.dtype == APAD_BF16  ? step_kernel<APAD_BF16>(form, a.branches)
                               : a.dtype == APAD_F32 ? step_kernel<APAD_F32>(form, a.branches)
                                                     : step_kernel<APAD_F16>(form, a.branches);
    hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)a.stream, (const uint8_t*)a.eps, a.latents, (uint8_t*)a.unet_in, a.eps_out,
                       a.history, a.noise, a.coef, a.keep, a.x0, a.z0, a.mask, per_clip, a.mask ? a.C : 1, a.n, a.step_ptr, a.n_steps, a.gs, total,
                       a.guidance);
    return apad_check_launch(fn);
}

}  // namespace

extern "C" int apad_cfg_ddim_step(const void* eps2, float* latents, void* unet_in, float* eps_out, const float* coef,
                                  const int32_t* step_ptr, float guidance_scale, int32_t B, int64_t n, int32_t dtype,
                                  void* stream) {
    StepOperands a = {};
    a.eps = eps2, a.latents = latents, a.unet_in = unet_in, a.eps_out = eps_out, a.coef = coef, a.step_ptr = step_ptr, a.gs = guidance_scale;
    a.B = B, a.n = n, a.dtype = dtype, a.stream = stream, a.branches = 2, a.ddim = true;
    return step_launch("apad_cfg_ddim_step", a);
}

extern "C" int apad_cfg_sampler_step(const void* eps2, float* latents, void* unet_in, float* eps_out, float* history, const float* noise,
                                     const float* coef, const int32_t* step_ptr, int32_t n_steps, float guidance_scale, int32_t B, int64_t n,
                                     int32_t dtype, void* stream) {
    StepOperands a = {};
    a.eps = eps2, a.latents = latents, a.unet_in = unet_in, a.eps_out = eps_out, a.history = history, a.noise = noise, a.coef = coef;
    a.step_ptr = step_ptr, a.n_steps = n_steps, a.gs = guidance_scale, a.B = B, a.n = n, a.dtype = dtype, a.stream = stream, a.branches = 2;
    return step_launch("apad_cfg_sampler_step", a);
}

extern "C" int apad_cfg_edit_step(const void* eps2, float* latents, void* unet_in, float* eps_out, float* history, const float* noise,
                                  const float* coef, const float* keep, const float* x0, const float* z0, const float* mask, int32_t mask_batch,
                                  int32_t C, const int32_t* step_ptr, int32_t n_steps, float guidance_scale, int32_t B, int64_t n, int32_t dtype,
                                  void* stream) {
    StepOperands a = {};
    a.eps = eps2, a.latents = latents, a.unet_in = unet_in, a.eps_out = eps_out, a.history = history, a.noise = noise, a.coef = coef;
    a.keep = keep, a.x0 = x0, a.z0 = z0, a.mask = mask, a.mask_batch = mask_batch, a.C = C;
    a.step_ptr = step_ptr, a.n_steps = n_steps, a.gs = guidance_scale, a.B = B, a.n = n, a.dtype = dtype, a.stream = stream, a.branches = 2;
    return step_launch("apad_cfg_edit_step", a);
}

extern "C" int apad_cfg_dual_step(const void* eps3, float* latents, void* unet_in, float* eps_out, float* history, const float* noise,
                                  const float* coef, const float* guidance, const float* keep, const float* x0, const float* z0, const float* mask,
                                  int32_t mask_batch, int32_t C, const int32_t* step_ptr, int32_t n_steps, int32_t B, int64_t n, int32_t dtype,
                                  void* stream) {
    StepOperands a = {};
    a.eps = eps3, a.latents = latents, a.unet_in = unet_in, a.eps_out = eps_out, a.history = history, a.noise = noise, a.coef = coef;
    a.guidance = guidance, a.keep = keep, a.x0 = x0, a.z0 = z0, a.mask = mask, a.mask_batch = mask_batch, a.C = C;
    a.step_ptr = step_ptr, a.n_steps = n_steps, a.B = B, a.n = n, a.dtype = dtype, a.stream = stream, a.branches = 3;
    return step_launch("apad_cfg_dual_step", a);
}

extern "C" int apad_cfg_shaped_step(const void* eps, float* latents, void* unet_in, float* eps_out, float* history, const float* noise,
                                    const float* coef, const float* guidance, const float* shape, float* momentum, float* stats, const float* keep,
                                    const float* x0, const float* z0, const float* mask, int32_t mask_batch, int32_t C, const int32_t* step_ptr,
                                    int32_t n_steps, float guidance_scale, int32_t branches, int32_t B, int64_t n, int32_t dtype, void* stream) {
    const char* fn = "apad_cfg_shaped_step";
    APAD_CHECK(branches == 2 || branches == 3, "%s: branches = %d must be 2 or 3", fn, branches);
    APAD_CHECK(shape, "%s: null shape table", fn);
    StepOperands a = {};
    a.eps = eps, a.latents = latents, a.unet_in = unet_in, a.eps_out = eps_out, a.history = history, a.noise = noise, a.coef = coef;
    a.guidance = guidance, a.keep = keep, a.x0 = x0, a.z0 = z0, a.mask = mask, a.mask_batch = mask_batch, a.C = C;
    a.step_ptr = step_ptr, a.n_steps = n_steps, a.gs = branches == 3 ? 0.f : guidance_scale, a.B = B, a.n = n, a.dtype = dtype, a.stream = stream;
    a.branches = branches, a.shape = shape, a.momentum = momentum, a.stats = stats;
    return step_launch(fn, a);
}

namespace {
using invert_kernel_t = decltype(&cfg_invert_step_kernel<APAD_BF16, STEP_VEC, 2>);
template <int DT> invert_kernel_t invert_kernel(bool vec, int branches) {
    if (branches == 3) return vec ? cfg_invert_step_kernel<DT, STEP_VEC, 3> : cfg_invert_step_kernel<DT, STEP_SCALAR, 3>;
    return vec ? cfg_invert_step_kernel<DT, STEP_VEC, 2> : cfg_invert_step_kernel<DT, STEP_SCALAR, 2>;
}
}  // namespace

extern "C" int apad_cfg_invert_step(const void* eps, float* latents, void* unet_in, float* eps_out, float* noise, const float* coef,
                                    const float* guidance, const float* keep, const float* x0, const int32_t* step_ptr, int32_t n_steps,
                                    float guidance_scale, int32_t branches, int32_t B, int64_t n, int32_t dtype, void* stream) {
    const char* fn = "apad_cfg_invert_step";
    APAD_CHECK(eps && latents && unet_in && noise && coef && keep && x0, "%s: null operand", fn);
    APAD_CHECK(branches == 2 || branches == 3, "%s: branches = %d must be 2 or 3", fn, branches);
    APAD_CHECK(branches == 2 || guidance, "%s: null guidance table", fn);
    APAD_CHECK(dtype == APAD_BF16 || dtype == APAD_F16 || dtype == APAD_F32, "%s: dtype %d not supported", fn, dtype);
    APAD_CHECK(B > 0 && n > 0 && n_steps > 0, "%s: empty problem", fn);
    const int64_t total = (int64_t)B * n;
    // the step kernel's rule (step_launch): 16-byte accesses need every non-null base 16-byte aligned and 8 | total
    const uintptr_t bases = (uintptr_t)eps | (uintptr_t)latents | (uintptr_t)unet_in | (uintptr_t)eps_out | (uintptr_t)noise | (uintptr_t)x0;
    const bool vec = total % 8 == 0 && bases % 16 == 0;
    int64_t blocks = ((vec ? total / 8 : total) + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    const invert_kernel_t kern = dtype == APAD_BF16  ? invert_kernel<APAD_BF16>(vec, branches)
                                 : dtype == APAD_F32 ? invert_kernel<APAD_F32>(vec, branches)
                                                     : invert_kernel<APAD_F16>(vec, branches);
    hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (const uint8_t*)eps, latents, (uint8_t*)unet_in, eps_out, noise, coef,
                       keep, x0, step_ptr, n_steps, branches == 3 ? 0.f : guidance_scale, total, guidance);
    return apad_check_launch(fn);
}

extern "C" int apad_edit_start(const void* moments, const float* post_noise, const float* z0, float* x0_out, float* latents, void* unet_in, float a,
                               float sg, float scale, int64_t rows, int32_t Lc, int32_t dtype, void* stream) {
    APAD_CHECK(z0 && x0_out && latents && unet_in, "apad_edit_start: null operand");
    APAD_CHECK(!moments || post_noise, "apad_edit_start: moments need post_noise (null operand)");
    APAD_CHECK(dtype == APAD_BF16 || dtype == APAD_F16 || dtype == APAD_F32, "apad_edit_start: dtype %d not supported", dtype);
    APAD_CHECK(rows > 0 && Lc > 0, "apad_edit_start: empty problem (rows=%lld Lc=%d)", (long long)rows, Lc);
    const int64_t total = rows * Lc;
    const uintptr_t bases = (uintptr_t)moments | (uintptr_t)post_noise | (uintptr_t)z0 | (uintptr_t)x0_out | (uintptr_t)latents | (uintptr_t)unet_in;
    const bool vec = Lc == 8 && bases % 16 == 0;
    int64_t blocks = ((vec ? total / 8 : total) + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    hipStream_t s = (hipStream_t)stream;
    LAUNCH_DT_V(edit_start_kernel, vec, dim3((unsigned)blocks), (const uint8_t*)moments, post_noise, z0, x0_out, latents, (uint8_t*)unet_in, a, sg, scale,
                total, Lc);
    return apad_check_launch("apad_edit_start");
}

extern "C" int apad_mix3(const void* a, const void* b, const void* c, void* out, int64_t n, float scale, int32_t dtype, void* stream) {
    APAD_CHECK(a && b && c && out && n > 0, "apad_mix3: bad operands");
    APAD_CHECK(dtype == APAD_BF16 || dtype == APAD_F16 || dtype == APAD_F32, "apad_mix3: dtype %d not supported", dtype);
    int64_t blocks = (n + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    hipStream_t s = (hipStream_t)stream;
    const uint8_t *pa = (const uint8_t*)a, *pb = (const uint8_t*)b, *pc = (const uint8_t*)c;
    LAUNCH_DT(mix3_kernel, dim3((unsigned)blocks), pa, pb, pc, (uint8_t*)out, n, scale);
    return apad_check_launch("apad_mix3");
}

extern "C" int apad_softmax_rows(const void* x, const float* bias, void* out, int64_t M, int32_t N, int64_t ldx, int64_t ldb, int64_t ldo,
                                 float scale, int32_t dtype, void* stream) {
    APAD_CHECK(x && out && M > 0 && N > 0 && ldx >= N && ldo >= N && (!bias || ldb >= N),
               "apad_softmax_rows: bad operands (M=%lld N=%d ldx=%lld ldb=%lld ldo=%lld)", (long long)M, N, (long long)ldx, (long long)ldb, (long long)ldo);
    APAD_CHECK(dtype == APAD_BF16 || dtype == APAD_F16 || dtype == APAD_F32, "apad_softmax_rows: dtype %d not supported", dtype);
    const dim3 grid((unsigned)((M + 3) / 4));
    hipStream_t s = (hipStream_t)stream;
    const uint8_t* px = (const uint8_t*)x;
    LAUNCH_DT(softmax_rows_kernel, grid, px, bias, (uint8_t*)out, M, N, ldx, ldb, ldo, scale);
    return apad_check_launch("apad_softmax_rows");
}

extern "C" int apad_rmsnorm(const void* x, const void* gamma, void* out, int64_t M, int32_t C, int64_t ldx, int64_t ldo, float eps, int32_t mode,
                            int32_t dtype, void* stream) {
    APAD_CHECK(x && out && M > 0 && C > 0 && ldx >= C && ldo >= C && (mode == 0 || mode == 1) && (mode == 1 || gamma), "apad_rmsnorm: bad operands");
    APAD_CHECK(dtype == APAD_BF16 || dtype == APAD_F16 || dtype == APAD_F32, "apad_rmsnorm: dtype %d not supported", dtype);
    const dim3 grid((unsigned)((M + 3) / 4));
    hipStream_t s = (hipStream_t)stream;
    const uint8_t *px = (const uint8_t*)x, *pg = (const uint8_t*)gamma;
    LAUNCH_DT(rmsnorm_kernel, grid, px, pg, (uint8_t*)out, M, C, ldx, ldo, eps, mode);
    return apad_check_launch("apad_rmsnorm");
}

extern "C" int apad_gather_rows(const void* table, const int64_t* ids, void* out, int64_t n, int64_t rows, int32_t C, int32_t dtype, void* stream) {
    APAD_CHECK(table && ids && out && n > 0 && rows > 0 && C > 0, "apad_gather_rows: bad operands");
    APAD_CHECK(dtype == APAD_BF16 || dtype == APAD_F16 || dtype == APAD_F32, "apad_gather_rows: dtype %d not supported", dtype);
    const dim3 grid((unsigned)((n + 3) / 4));
    hipStream_t s = (hipStream_t)stream;
    const uint8_t* pt = (const uint8_t*)table;
    LAUNCH_DT(gather_rows_kernel, grid, pt, ids, (uint8_t*)out, n, rows, C);
    return apad_check_launch("apad_gather_rows");
}

extern "C" int apad_gaussian_sample(const void* moments, const void* noise, void* out, int64_t rows, int32_t latent, float scale,
                                    int32_t dtype, void* stream) {
    APAD_CHECK(moments && noise && out && rows > 0 && latent > 0, "apad_gaussian_sample: bad operands");
    APAD_CHECK(dtype == APAD_BF16 || dtype == APAD_F16 || dtype == APAD_F32, "apad_gaussian_sample: dtype %d not supported", dtype);
    int64_t blocks = (rows * latent + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    hipStream_t s = (hipStream_t)stream;
    const uint8_t *pm = (const uint8_t*)moments, *pn = (const uint8_t*)noise;
    LAUNCH_DT(gaussian_sample_kernel, dim3((unsigned)blocks), pm, pn, (uint8_t*)out, rows, latent, scale);
    return apad_check_launch("apad_gaussian_sample");
}

extern "C" int apad_step_advance(int32_t* step_ptr, void* stream) {
    APAD_CHECK(step_ptr, "apad_step_advance: null pointer");
    hipLaunchKernelGGL(step_advance_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, step_ptr);
    return apad_check_launch("apad_step_advance");
}

// ---- measurement probe (bench.py's `mfma_ceiling`): four independent v_mfma_f32_32x32x16_bf16 chains per wave, two waves per SIMD, no memory
//      traffic; operands zero (mode 0) or eight rotating register sets of pseudo-random bf16 in [-1, 1) (mode 1).  The dense rate this chip delivers
//      depends on the operand data (power management: tools/ubench/mfma_data.hip); the bench line states it next to the nominal peak. ----
namespace {
__device__ __forceinline__ uint32_t probe_hash32(uint32_t x) {
    x ^= x >> 16; x *= 0x7feb352dU; x ^= x >> 15; x *= 0x846ca68bU; x ^= x >> 16;
    return x;
}
__global__ __launch_bounds__(256) void mfma_probe_kernel(float* sink, int mode, int iters) {
    bf16x8_t a[8], b[8];
    for (int s = 0; s < 8; ++s)
        for (int i = 0; i < 8; ++i) {
            float va = 0.f, vb = 0.f;
            if (mode == 1) {
                va = (float)(probe_hash32(threadIdx.x * 131u + s * 17u + i) & 0xffff) / 32768.f - 1.f;
                vb = (float)(probe_hash32(threadIdx.x * 977u + s * 29u + i + 7u) & 0xffff) / 32768.f - 1.f;
            }
            a[s][i] = (__bf16)va;
            b[s][i] = (__bf16)vb;
        }
    f32x16 acc[4];
    for (int c = 0; c < 4; ++c)
        for (int r = 0; r < 16; ++r) acc[c][r] = 0.f;
    for (int it = 0; it < iters; ++it) {
#pragma unroll
        for (int s = 0; s < 8; ++s)
#pragma unroll
            for (int c = 0; c < 4; ++c) acc[c] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[s], b[(s + c) & 7], acc[c], 0, 0, 0);
    }
    float t = 0.f;
    for (int c = 0; c < 4; ++c)
        for (int r = 0; r < 16; ++r) t += acc[c][r];
    if (t == 12345.678f) sink[0] = t;
}
}  // namespace

// launches the probe on 512 workgroups of 256 threads; returns the FLOPs of the launch through *flops (2 x 32 x 32 x 16 per MFMA)
extern "C" int apad_probe_mfma(void* sink, int32_t mode, int32_t iters, double* flops, void* stream) {
    APAD_CHECK(sink && iters > 0 && (mode == 0 || mode == 1), "apad_probe_mfma: bad arguments");
    hipLaunchKernelGGL(mfma_probe_kernel, dim3(512), dim3(256), 0, (hipStream_t)stream, (float*)sink, mode, iters);
    if (flops) *flops = 512.0 * 4 * iters * 32 * 2.0 * 32 * 32 * 16;
    return apad_check_launch("apad_probe_mfma");
}
