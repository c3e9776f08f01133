// Internal entry points of the fp32 precision mode (f32_ops.hip).  The C-ABI functions dispatch here when the
// descriptor's dtype is APAD_F32 (or APAD_F32_BF16X3 for apad_gemm / apad_attention); arguments are validated inside.
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/apadapter_hip.h"
#include "common.h"

int apad_f32_gemm(const apad_gemm_desc* d, hipStream_t s);
int apad_f32_attention(const apad_attn_desc* d, const Scale2Tab& s2, const QueryW& qw, hipStream_t s);  // s2 / qw: apad_attention_tab's table, apad_attention_qw's map, or none
int apad_f32_attention_multi(const apad_attn_desc* d, const Scale2Tab& s2, const QueryW& qw, const AttnExtras& xs, hipStream_t s);  // xs.n > 0 extra audio segments
int apad_f32_layernorm(const void* x, const void* gamma, const void* beta, void* out, int64_t M, int32_t C, int64_t ldx,
                       int64_t ldo, float eps, hipStream_t s);
int apad_f32_groupnorm(const void* x, const void* gamma, const void* beta, void* out, int32_t B, int32_t HW, int32_t C,
                       int32_t G, float eps, int32_t silu, hipStream_t s);
int apad_f32_audiomae_pool(const void* rep, void* out, int32_t B, int32_t tp, int32_t fp, hipStream_t s);
int apad_f32_attention_bwd(const apad_attn_bwd_desc* d, hipStream_t s);
