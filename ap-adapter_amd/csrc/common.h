// Shared device helpers for the gfx950 kernels (wave64, MFMA 32x32x16, bf16/f16 with fp32 accumulate).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/apadapter_hip.h"

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8_t;
typedef __attribute__((ext_vector_type(8))) _Float16 f16x8_t;
typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4_t;
typedef __attribute__((ext_vector_type(4))) _Float16 f16x4_t;
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

#define APAD_WAVE 64

// Element-type traits: DT is APAD_BF16 or APAD_F16.
template <int DT> struct ET;
template <> struct ET<APAD_BF16> {
    using elem = __bf16;
    using v8 = bf16x8_t;
    using v4 = bf16x4_t;
    static __device__ __forceinline__ f32x16 mfma32(v8 a, v8 b, f32x16 c) {
        return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
    }
};
template <> struct ET<APAD_F16> {
    using elem = _Float16;
    using v8 = f16x8_t;
    using v4 = f16x4_t;
    static __device__ __forceinline__ f32x16 mfma32(v8 a, v8 b, f32x16 c) {
        return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0);
    }
};

// fp32 precision mode: only the element type (the element-wise kernels are templated on it); the MFMA kernels of this
// mode live in f32_ops.hip
template <> struct ET<APAD_F32> {
    using elem = float;
};

template <int DT> __device__ __forceinline__ typename ET<DT>::v8 as_v8(uint4 u) {
    return __builtin_bit_cast(typename ET<DT>::v8, u);
}
template <int DT> __device__ __forceinline__ uint4 as_u4(typename ET<DT>::v8 v) {
    return __builtin_bit_cast(uint4, v);
}
template <int DT> __device__ __forceinline__ float ld_elem(const void* p, int64_t i) {
    return (float)reinterpret_cast<const typename ET<DT>::elem*>(p)[i];
}
template <int DT> __device__ __forceinline__ void st_elem(void* p, int64_t i, float v) {
    reinterpret_cast<typename ET<DT>::elem*>(p)[i] = (typename ET<DT>::elem)v;
}
// 8 floats <-> one 16-byte vector of elements
template <int DT> __device__ __forceinline__ void unpack8(uint4 u, float* f) {
    typename ET<DT>::v8 v = as_v8<DT>(u);
#pragma unroll
    for (int i = 0; i < 8; ++i) f[i] = (float)v[i];
}
template <int DT> __device__ __forceinline__ uint4 pack8(const float* f) {
    typename ET<DT>::v8 v;
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = (typename ET<DT>::elem)f[i];
    return as_u4<DT>(v);
}

// Exchange between the two 32-lane halves of a wave (lane l <-> lane l ^ 32), the only cross-lane traffic of the
// transposed-score kernels.  gfx950's v_permlane32_swap does it in one VALU instruction; __shfl_xor(v, 32) lowers to
// ds_bpermute_b32, i.e. an LDS round trip plus an lgkmcnt wait in the middle of the softmax.
__device__ __forceinline__ void half_pair(float v, float& lo, float& hi) {
    const unsigned a = __float_as_uint(v);
    const auto r = __builtin_amdgcn_permlane32_swap(a, a, false, false);
    lo = __uint_as_float(r[0]);  // the lower half's value, in every lane
    hi = __uint_as_float(r[1]);  // the upper half's value, in every lane
}
__device__ __forceinline__ float half_max(float v) { float lo, hi; half_pair(v, lo, hi); return fmaxf(lo, hi); }
__device__ __forceinline__ float half_sum(float v) { float lo, hi; half_pair(v, lo, hi); return lo + hi; }
__device__ __forceinline__ float half_lo(float v) { float lo, hi; half_pair(v, lo, hi); return lo; }

__device__ __forceinline__ float silu_f(float x) { return x * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-1.4426950408889634f * x)); }
// erf via Abramowitz & Stegun 7.1.26 (|error| <= 1.5e-7, i.e. fp32-exact for a bf16/f16 result): one rcp, one exp2 and
// five FMAs instead of libm's erff (~40 VALU instructions) -- the GEGLU epilogue evaluates this for every element of the
// 4C-wide feed-forward activation, where erff made the epilogue cost more than the MFMAs feeding it.
__device__ __forceinline__ float erf_as(float x) {
    const float ax = fabsf(x);
    const float t = __builtin_amdgcn_rcpf(fmaf(0.3275911f, ax, 1.0f));
    float p = fmaf(1.061405429f, t, -1.453152027f);
    p = fmaf(p, t, 1.421413741f);
    p = fmaf(p, t, -0.284496736f);
    p = fmaf(p, t, 0.254829592f);
    const float e = __builtin_amdgcn_exp2f(-1.4426950408889634f * ax * ax);
    const float r = fmaf(-p * t, e, 1.0f);
    return copysignf(r, x);
}
__device__ __forceinline__ float gelu_erf_f(float x) { return 0.5f * x * (1.0f + erf_as(x * 0.70710678118654752440f)); }

// Two GELUs at once on packed fp32 math (v_pk_mul/fma_f32 process two lanes-worth per instruction; only rcp / exp2 stay
// scalar).  A&S 7.1.26 with the argument scaled ONCE: z' = x sqrt(log2(e) / 2), so that exp(-x^2 / 2) = exp2(-z'^2) (the negation is a source
// modifier) and the rational argument is |z'| p' with p' = p / sqrt(log2 e) -- two multiplies per value fewer than scaling x / sqrt 2 and
// z^2 log2(e) separately.  Every GEGLU kernel of the library evaluates THIS operation order (the phased form: M3Geglu, mlp3_shared.h), which
// is what makes a row's result independent of the kernel its batch size selects.
typedef float apad_f32x2 __attribute__((ext_vector_type(2)));
constexpr float APAD_GELU_K1 = 0.84932180028801904272f;  // sqrt(log2(e) / 2)
constexpr float APAD_GELU_P1 = 0.2727374808792225f;       // 0.3275911 / sqrt(log2(e))
__device__ __forceinline__ apad_f32x2 gelu_erf_2(apad_f32x2 x) {
    const apad_f32x2 z = x * APAD_GELU_K1;
    const apad_f32x2 az = {fabsf(z[0]), fabsf(z[1])};
    const apad_f32x2 d = __builtin_elementwise_fma(az, (apad_f32x2){APAD_GELU_P1, APAD_GELU_P1}, (apad_f32x2){1.0f, 1.0f});
    const apad_f32x2 t = {__builtin_amdgcn_rcpf(d[0]), __builtin_amdgcn_rcpf(d[1])};
    apad_f32x2 p = __builtin_elementwise_fma(t, (apad_f32x2){1.061405429f, 1.061405429f}, (apad_f32x2){-1.453152027f, -1.453152027f});
    p = __builtin_elementwise_fma(p, t, (apad_f32x2){1.421413741f, 1.421413741f});
    p = __builtin_elementwise_fma(p, t, (apad_f32x2){-0.284496736f, -0.284496736f});
    p = __builtin_elementwise_fma(p, t, (apad_f32x2){0.254829592f, 0.254829592f});
    const apad_f32x2 q = z * z;
    const apad_f32x2 e = {__builtin_amdgcn_exp2f(-q[0]), __builtin_amdgcn_exp2f(-q[1])};
    const apad_f32x2 r = __builtin_elementwise_fma(p * t, -e, (apad_f32x2){1.0f, 1.0f});  // erf(|x| / sqrt 2)
    const apad_f32x2 hx = x * 0.5f;
    // 0.5 x (1 + sign(x) erf|z|) = hx + |hx| * erf|z|
    const apad_f32x2 ahx = {fabsf(hx[0]), fabsf(hx[1])};
    return __builtin_elementwise_fma(ahx, r, hx);
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// apad_scale2_tab as the two-segment attention kernels carry it in their parameter block: table == nullptr selects the descriptor's scalar.
struct Scale2Tab {
    const float* table;
    const int32_t* step;
    int64_t ld;
    int32_t rows, cols;
};
// The weight of segment 2 for sample b: table[min(*step, rows - 1) * ld + b % cols], or `scalar` without a table.  Read once per workgroup (per
// panel group where a tile spans samples), before the key loop: the address is formed from kernel arguments, *step and the workgroup's sample
// index only -- readfirstlane states that to the compiler -- so it is one scalar load on the uniform path and the value lives in an SGPR.
__device__ __forceinline__ float scale2_of(const Scale2Tab& t, float scalar, int b) {
    if (t.table == nullptr) return scalar;
    int r = t.step ? *t.step : 0;
    r = r < t.rows - 1 ? r : t.rows - 1;
    r = r > 0 ? r : 0;
    const int c = __builtin_amdgcn_readfirstlane(b) % t.cols;
    return t.table[(int64_t)r * t.ld + c];
}
// The same for a persistent kernel that reads the table after it has stored a tile: there the compiler cannot show the table unwritten and
// would fetch the uniform value through the vector port into a VGPR, one register too many for the 256-register kernels.  Both reads are
// scalar loads by hand (the scalar cache is clean: nothing in the launch writes the table or the counter).
__device__ __forceinline__ float scale2_of_sload(const Scale2Tab& t, float scalar, int b) {
    if (t.table == nullptr) return scalar;
    int r = 0;
    if (t.step) asm volatile("s_load_dword %0, %1, 0x0\n\ts_waitcnt lgkmcnt(0)" : "=s"(r) : "s"(t.step) : "memory");
    r = r < t.rows - 1 ? r : t.rows - 1;
    r = r > 0 ? r : 0;
    const int c = __builtin_amdgcn_readfirstlane(b) % t.cols;
    const float* src = t.table + ((int64_t)r * t.ld + c);
    float v;
    asm volatile("s_load_dword %0, %1, 0x0\n\ts_waitcnt lgkmcnt(0)" : "=s"(v) : "s"(src) : "memory");
    return v;
}

// apad_query_weight as the kernels' QW instantiations carry it (the other instantiations never read it: w == nullptr).
struct QueryW {
    const float* w;
    int64_t ld;
    int32_t cols, pad;
};
// The weight of segment 2 for query n of sample b (n < N: the caller clamps a tail lane as it clamps its q load): s * w[(b % cols) * ld + n], ONE
// fp32 multiply of the workgroup's scalar by the lane's own map entry -- one vector load per lane, its row base formed on the scalar path.
// The product stands where the scalar stands in the blend, so a map entry v is bit-equal to the scalar launch with (float)s * v.
template <bool QW> __device__ __forceinline__ float query_weight(const QueryW& q, int b, int n) {
    if constexpr (!QW) return 1.0f;
    else {
        const float* const row = q.w + (int64_t)(__builtin_amdgcn_readfirstlane(b) % q.cols) * q.ld;  // uniform: a scalar base
        return row[(uint32_t)n];                                                                      // + the lane's 32-bit offset
    }
}
template <bool QW> __device__ __forceinline__ float weighted_scale2(float s, float w) {
    if constexpr (!QW) return s;
    else return s * w;
}

// apad_attention_multi: one more audio segment (apad_attn_extra) as the multi-prompt kernels carry it, and the block of up to three of them that
// travels beside AttnP / A32P.  Strides in elements of the launch's type.  The kernels index x[] with a runtime j: the block lives in the kernel
// argument segment, so an entry is a handful of scalar loads.
struct AttnSeg {
    const void* k;
    const void* vt;
    int64_t k_sb, k_sl, vt_sb;
    int32_t L, Lpad, kvdiv, pad;
    float scale, padf;  // read when s2.table == nullptr
    Scale2Tab s2;
    QueryW qw;          // w == nullptr: no map
};
constexpr int APAD_MAX_EXTRA = 3;
struct AttnExtras {
    AttnSeg x[APAD_MAX_EXTRA];
    int32_t n, pad;
};
// The map entry of a multi-prompt launch, where a prompt has a map or not at run time: no map reads as 1.0f, and s * 1.0f is s bit for bit, so
// both sides are the expressions of query_weight<> / weighted_scale2<>.
__device__ __forceinline__ float query_weight_rt(const QueryW& q, int b, int n) {
    if (q.w == nullptr) return 1.0f;  // (wave-uniform)
    const float* const row = q.w + (int64_t)(__builtin_amdgcn_readfirstlane(b) % q.cols) * q.ld;
    return row[(uint32_t)n];
}

// host-side error plumbing (capi.cpp)
void apad_set_error(const char* fmt, ...);
#define APAD_CHECK(cond, ...)            \
    do {                                 \
        if (!(cond)) {                   \
            apad_set_error(__VA_ARGS__); \
            return -1;                   \
        }                                \
    } while (0)
int apad_check_launch(const char* what);
// The table of an apad_*_tab entry point `who`, checked (null table, rows / cols <= 0, ld < cols, a pointer off 4 bytes, or a single-segment call
// L2 == 0: an error naming `who`, -1) and copied into the kernels' form.  t == nullptr (the scalar entry points): *out = no table, 0.
int apad_scale2_tab_arg(const char* who, const apad_scale2_tab* t, bool has_tab, int L2, Scale2Tab* out);
// The map of an apad_*_qw entry point `who`, checked (a null struct or map, cols <= 0, ld < N, a map off 4 bytes, or a single-segment call: an
// error naming `who`, -1) and copied into the kernels' form.  has_qw false (every other entry point): *out = no map, 0.
int apad_query_weight_arg(const char* who, const apad_query_weight* w, bool has_qw, int N, int L2, QueryW* out);
// The extra segments of apad_attention_multi (`who`), checked (what include/apadapter_hip.h lists: an error naming `who`, -1) and copied into
// the kernels' form; entries at and past n_extra are zeroed.  N: the launch's queries (a map's row stride); elem_bytes: 2 or 4.
int apad_attn_extras_arg(const char* who, const apad_attn_extra* extra, int n_extra, int N, int elem_bytes, AttnExtras* out);
// The dtype ladder of the 256-thread element-wise launches, for the `dtype` (APAD_BF16 / APAD_F16 / APAD_F32, checked by the caller) and the
// stream `s` of the calling scope: kern<DT> (LAUNCH_DT), kern<DT, F> (LAUNCH_DT_F), kern<DT, vec ? 8 : 1> (LAUNCH_DT_V)
#define LAUNCH_DT(kern, grid, ...)                                                                                \
    do {                                                                                                          \
        if (dtype == APAD_BF16) hipLaunchKernelGGL((kern<APAD_BF16>), grid, dim3(256), 0, s, __VA_ARGS__);        \
        else if (dtype == APAD_F32) hipLaunchKernelGGL((kern<APAD_F32>), grid, dim3(256), 0, s, __VA_ARGS__);     \
        else hipLaunchKernelGGL((kern<APAD_F16>), grid, dim3(256), 0, s, __VA_ARGS__);                            \
    } while (0)
#define LAUNCH_DT_F(kern, F, grid, ...)                                                                           \
    do {                                                                                                          \
        if (dtype == APAD_BF16) hipLaunchKernelGGL((kern<APAD_BF16, F>), grid, dim3(256), 0, s, __VA_ARGS__);     \
        else if (dtype == APAD_F32) hipLaunchKernelGGL((kern<APAD_F32, F>), grid, dim3(256), 0, s, __VA_ARGS__);  \
        else hipLaunchKernelGGL((kern<APAD_F16, F>), grid, dim3(256), 0, s, __VA_ARGS__);                         \
    } while (0)
#define LAUNCH_DT_V(kern, vec, grid, ...)                          \
    do {                                                           \
        if (vec) LAUNCH_DT_F(kern, 8, grid, __VA_ARGS__);          \
        else LAUNCH_DT_F(kern, 1, grid, __VA_ARGS__);              \
    } while (0)
// dynamic LDS above 64 KB needs hipFuncAttributeMaxDynamicSharedMemorySize once per (kernel, DEVICE): *devmask = the devices it has been set on
// (one static word per kernel at the call site); thread-safe, the return code of hipFuncSetAttribute is checked.  0 = ok, -1 = error set
int apad_ensure_dyn_lds(const void* kern, int bytes, unsigned* devmask);
// big-tile GEMM / implicit convolution (cgemm.hip): 1 = not applicable, 0 = launched, < 0 = error
int apad_cgemm_try(const apad_gemm_desc* d, hipStream_t s);
// halo-resident 3x3 convolution (hconv.hip), same convention; needs apad_gemm_desc::w_halo
int apad_hconv_try(const apad_gemm_desc* d, hipStream_t s);
