// The hand-scheduling layer of the LDS-DMA kernels, written once: LDS-DMA with hand-kept vmcnt waits, raw barriers,
// inline-asm fragment reads, VGPR-form MFMAs in inline asm.  The compiler's wait-count pass orders every LDS access it can see behind
// ALL outstanding LDS-DMA (it inserts s_waitcnt vmcnt(0), which drains the tiles in flight), so next to a DMA ring the ordering that
// is actually needed is kept by hand with these.
// The exact form of each one is part of the schedules around it: an operand constraint, a fence or a sched_barrier changed here changes
// the device assembly of every kernel that uses it.
#pragma once
#include "common.h"

// an LDS pointer: what the LDS-DMA builtins take; (uint32_t)(size_t)(lds_ptr)p is the LDS byte address inline asm wants
typedef __attribute__((address_space(3))) void* lds_ptr;

// a wave-uniform pointer, pinned to SGPRs: loads through it take the (scalar base + 32-bit lane offset) form instead of a
// 64-bit per-lane address -- the compiler otherwise hoists one such address per weight fragment out of the tile loop (24
// registers per weight), which is what spilled in the 256-register kernels
// (typed as a GLOBAL-address-space pointer: after the integer round trip the compiler no longer infers that, and a generic
//  pointer turns the loads into flat_load, which also ticks lgkmcnt and makes every later wait a vmcnt(0))
typedef const __attribute__((address_space(1))) uint8_t* gptr;
typedef const __attribute__((address_space(1))) u32x4* gptr16;
__device__ __forceinline__ gptr sgpr_ptr(const uint8_t* p) {
    const uint64_t a = reinterpret_cast<uint64_t>(p);
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)a), hi = __builtin_amdgcn_readfirstlane((uint32_t)(a >> 32));  // (unsigned: no sign extension)
    return (gptr)(((uint64_t)hi << 32) | lo);
}
__device__ __forceinline__ u32x4 ld16(gptr base, uint32_t off) { return *(gptr16)(base + off); }

// buffer resource over [p, p + bytes): a load past the end returns 0 (the convolutions' zero padding, ragged last tiles), a store past it is dropped
__device__ __forceinline__ __amdgpu_buffer_rsrc_t buf_rsrc(const void* p, uint32_t bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), 0, (int)bytes, 0x00020000);
}

// Piece q (0 .. N - 1; a constant once inlined) of a group of 1 KB LDS-DMA pieces (16 bytes per lane) that share one M0 / scalar offset:
// the instruction's immediate offset Q KB moves the memory address AND the LDS address.  The builtin wants the offset as a literal.
template <int N, int Q = 0>
__device__ __forceinline__ void dma_piece(__amdgpu_buffer_rsrc_t r, lds_ptr lp, uint32_t voff, int soff, int q) {
    if constexpr (Q + 1 < N) {
        if (q != Q) return dma_piece<N, Q + 1>(r, lp, voff, soff, q);
    }
    __builtin_amdgcn_raw_ptr_buffer_load_lds(r, lp, 16, voff, soff, Q * 1024, 0);
}

// SCHED_PIN: nothing is scheduled across it.  ASM_FENCE: a compiler-only memory fence.  RAW_BARRIER: s_barrier without the
// s_waitcnt vmcnt(0) a __syncthreads() carries, so the DMA in flight stays in flight across it; fenced and pinned on both sides.
#define SCHED_PIN() __builtin_amdgcn_sched_barrier(0)
#define ASM_FENCE() asm volatile("" ::: "memory")
#define RAW_BARRIER()                  \
    do {                               \
        SCHED_PIN();                   \
        ASM_FENCE();                   \
        __builtin_amdgcn_s_barrier();  \
        ASM_FENCE();                   \
        SCHED_PIN();                   \
    } while (0)

// counted waits: at most N of this wave's vector-memory (LDS-DMA, global, buffer) / LDS requests still outstanding.  Neither pins: the
// compiler does not know the inline-asm reads are outstanding, so a wait_lgkm whose values are consumed next is followed by SCHED_PIN()
// or RAW_BARRIER() (which starts with one; a second sched_barrier there changes the schedule).
template <int N> __device__ __forceinline__ void wait_vm() {
    static_assert(N >= 0 && N < 64, "vmcnt is 6 bits");
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}
template <int N> __device__ __forceinline__ void wait_lgkm() {
    static_assert(N >= 0 && N < 16, "lgkmcnt is 4 bits");
    asm volatile("s_waitcnt lgkmcnt(%0)" ::"n"(N) : "memory");
}

// one 16-byte LDS fragment read at immediate offset OFF, in inline asm (see the top).  IMM: the constraint letter of the offset
// operand, 'n' or 'i'.  The two are not neutral -- each caller keeps the one its schedule was made with (hconv.hip: 'i').
template <int OFF, char IMM = 'n'> __device__ __forceinline__ void lds_read16(u32x4& d, uint32_t a) {
    static_assert(IMM == 'n' || IMM == 'i', "offset constraint");
    if constexpr (IMM == 'n') asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(d) : "v"(a), "n"(OFF));
    else asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(d) : "v"(a), "i"(OFF));
}

// 32x32x16 MFMA in inline asm with VGPR accumulators, for functions whose compiler MFMAs are the AGPR form.  mlp3.hip: the 256 output
// accumulators fill the AGPR file, and an AGPR-form accumulator for gemm1 would have to be copied out through v_accvgpr_read for the GEGLU
// arithmetic (and, with 320 accumulator registers asked of a 256-entry file, shuffled between AGPR ranges: measured in the ISA, 8 copies per MFMA).
// B: the register class of the B operand, 'v' or 'a' (geglu3.hip keeps x in AGPRs for the whole kernel).  The hazards the compiler would
// have covered are the caller's: first()'s C operand (b1, straight from ds_read_b128) sits behind an explicit wait + the s_nop 1 here, and
// its registers are not rewritten within 13 wait states of the MFMA; vector code reads the accumulators only an LDS round trip (the next
// fragment wait) after the last MFMA that writes them.
template <int DT, char B> struct AsmMfma;
template <char B> struct AsmMfma<APAD_BF16, B> {
    static_assert(B == 'v' || B == 'a', "B operand register class");
    template <typename V8> static __device__ __forceinline__ void first(f32x16& d, const V8& a, const V8& b, const f32x16& c) {
        if constexpr (B == 'v') asm volatile("s_nop 1\n\tv_mfma_f32_32x32x16_bf16 %0, %1, %2, %3" : "=&v"(d) : "v"(a), "v"(b), "v"(c));
        else asm volatile("s_nop 1\n\tv_mfma_f32_32x32x16_bf16 %0, %1, %2, %3" : "=&v"(d) : "v"(a), "a"(b), "v"(c));
    }
    template <typename V8> static __device__ __forceinline__ void acc(f32x16& d, const V8& a, const V8& b) {
        if constexpr (B == 'v') asm volatile("v_mfma_f32_32x32x16_bf16 %0, %1, %2, %0" : "+v"(d) : "v"(a), "v"(b));
        else asm volatile("v_mfma_f32_32x32x16_bf16 %0, %1, %2, %0" : "+v"(d) : "v"(a), "a"(b));
    }
};
template <char B> struct AsmMfma<APAD_F16, B> {
    static_assert(B == 'v' || B == 'a', "B operand register class");
    template <typename V8> static __device__ __forceinline__ void first(f32x16& d, const V8& a, const V8& b, const f32x16& c) {
        if constexpr (B == 'v') asm volatile("s_nop 1\n\tv_mfma_f32_32x32x16_f16 %0, %1, %2, %3" : "=&v"(d) : "v"(a), "v"(b), "v"(c));
        else asm volatile("s_nop 1\n\tv_mfma_f32_32x32x16_f16 %0, %1, %2, %3" : "=&v"(d) : "v"(a), "a"(b), "v"(c));
    }
    template <typename V8> static __device__ __forceinline__ void acc(f32x16& d, const V8& a, const V8& b) {
        if constexpr (B == 'v') asm volatile("v_mfma_f32_32x32x16_f16 %0, %1, %2, %0" : "+v"(d) : "v"(a), "v"(b));
        else asm volatile("v_mfma_f32_32x32x16_f16 %0, %1, %2, %0" : "+v"(d) : "v"(a), "a"(b));
    }
};
