// Pieces shared by the GEMM kernels behind apad_gemm: the XCD-aware tile order (gemm.hip, cgemm.hip, hconv.hip), the A-operand geometry,
// row decode and gather arithmetic of the implicit convolutions (gemm.hip and f32_ops.hip: identical up to the element width), the
// 16-bit epilogue of the tiled and the ring kernel (gemm.hip: ONE text, so the two forms stay bit-equal by construction) and the
// descriptor checks apad_gemm and apad_f32_gemm state alike.  Plain forceinline templates; what a kernel does differently stays in it.
#pragma once
#include "common.h"

namespace {

// XCD-aware tile order: workgroup id b runs on XCD b % 8 (observed dispatch order, speed only).  Tiles are numbered so that all
// N-tiles of one M-tile share b % 8, i.e. one XCD's L2 fetches each A row-panel (hconv: each halo) once.
__device__ __forceinline__ void xcd_tile_order(int b, int nM, int nN, int& mt, int& nt) {
    const int full = (nM / 8) * 8 * nN;  // blocks covered by complete groups of 8 M-tiles
    if (b < full) {
        const int grp = b / (8 * nN), rem = b - grp * 8 * nN;
        nt = rem >> 3;
        mt = grp * 8 + (rem & 7);
    } else {
        const int rem = b - full, tail = nM - (nM / 8) * 8;  // < 8 leftover M-tiles
        nt = rem / tail;
        mt = (nM / 8) * 8 + rem - nt * tail;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// A operand of the implicit GEMMs: what apad_gemm_desc says about the source, the decode of an output row and the source offset of
// one staging vector.  The element width (and with it the vector length, the load and the pre-activation) is the caller's.
// ---------------------------------------------------------------------------------------------------------------------------------
struct AGeom {
    int32_t Hin, Win, Cin, Hout, Wout, stride, Hup, Wup, src_batch_mod;
    int32_t taps, dilation, pad, transposed, pre_act;  // APAD_A_CONV1D
    float pre_slope;
    int32_t lead;  // conv3x3: zero rows / columns before the first source row / column (1, or 0 with conv_asym_pad)
};

inline AGeom a_geom(const apad_gemm_desc* d) {
    AGeom g;
    g.Hin = d->Hin; g.Win = d->Win; g.Cin = d->Cin; g.Hout = d->Hout; g.Wout = d->Wout;
    g.stride = d->stride; g.Hup = d->Hup; g.Wup = d->Wup; g.src_batch_mod = d->src_batch_mod;
    g.taps = d->taps; g.dilation = d->dilation; g.pad = d->pad; g.transposed = d->transposed; g.pre_act = d->a_pre_act;
    g.pre_slope = d->a_pre_slope;
    g.lead = d->conv_asym_pad ? 0 : 1;
    return g;
}

struct ARow {
    int64_t base;  // PLAIN: element offset of the row; CONV / PATCH: source batch index
    int oy, ox;
    bool valid;
};

// output row m of a CONV3X3 / CONV1D / PATCH16 launch -> (source batch, oy, ox); a plain row is the kernel's own
template <int AMODE> __device__ __forceinline__ void decode_row(const AGeom& g, int64_t m, ARow& r) {
    if (AMODE == APAD_A_CONV3X3) {
        const int64_t hw = (int64_t)g.Hout * g.Wout;
        const int64_t b = m / hw;
        const int rem = (int)(m - b * hw);
        r.oy = rem / g.Wout;
        r.ox = rem - r.oy * g.Wout;
        r.base = g.src_batch_mod > 0 ? b % g.src_batch_mod : b;
    } else if (AMODE == APAD_A_CONV1D) {
        const int64_t b = m / g.Hout;
        r.oy = (int)(m - b * g.Hout);
        r.base = b;
    } else {
        const int wp = g.Win >> 4, hp = g.Hin >> 4;
        const int64_t b = m / (hp * wp);
        const int rem = (int)(m - b * hp * wp);
        r.oy = rem / wp;
        r.ox = rem - r.oy * wp;
        r.base = b;
    }
}

// element offset of the staging vector at reduction index k of a decoded row, or A_ZERO: the vector lies in the padding
constexpr int64_t A_ZERO = -1;
template <int AMODE> __device__ __forceinline__ int64_t a_src_offset(const AGeom& g, const ARow& r, int k) {
    if (AMODE == APAD_A_CONV3X3) {
        const int tap = k / g.Cin, c = k - tap * g.Cin;
        const int ky = tap / 3, kx = tap - ky * 3;
        int iy = r.oy * g.stride + ky - g.lead, ix = r.ox * g.stride + kx - g.lead;
        const int H = g.Hup > 0 ? g.Hup : g.Hin, W = g.Hup > 0 ? g.Wup : g.Win;
        if (iy < 0 || iy >= H || ix < 0 || ix >= W) return A_ZERO;
        if (g.Hup > 0) {  // nearest-neighbour source index, floor(dst * in / out)
            iy = (int)(((int64_t)iy * g.Hin) / g.Hup);
            ix = (int)(((int64_t)ix * g.Win) / g.Wup);
        }
        return ((r.base * g.Hin + iy) * g.Win + ix) * g.Cin + c;
    } else if (AMODE == APAD_A_CONV1D) {  // channels-last [B][Hin][Cin]; r.base = b, r.oy = t; k = (tap, c)
        const int tap = k / g.Cin, c = k - tap * g.Cin;
        int ti;
        if (g.transposed) {
            const int num = r.oy + g.pad - tap;
            ti = num / g.stride;
            if (num < 0 || ti * g.stride != num) return A_ZERO;
        } else {
            ti = r.oy + tap * g.dilation - g.pad;
        }
        if (ti < 0 || ti >= g.Hin) return A_ZERO;
        return (r.base * g.Hin + ti) * g.Cin + c;
    } else {  // PATCH16: fp32 mel [B][Hin][Win]; k = py * 16 + px
        const int py = k >> 4, px = k & 15;
        return (r.base * g.Hin + r.oy * 16 + py) * g.Win + r.ox * 16 + px;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// The descriptor checks of apad_gemm (vec = 8 elements per 16 bytes) and apad_f32_gemm (vec = 4) that both state, in apad_gemm's
// order.  geglu: the epilogue interleaves value | gate rows; out4: the path writes APAD_OUT_QKV's row-major v.
// ---------------------------------------------------------------------------------------------------------------------------------
inline bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

inline int gemm_desc_check(const apad_gemm_desc* d, int vec, const char* tag, bool geglu, bool out4) {
    APAD_CHECK(d->a && d->w && d->out, "%s: null operand", tag);
    APAD_CHECK(d->M > 0 && d->N > 0 && d->K > 0, "%s: empty problem M=%lld N=%lld K=%lld", tag, (long long)d->M, (long long)d->N, (long long)d->K);
    APAD_CHECK(d->K % vec == 0 && d->ldw % vec == 0, "%s: K and ldw must be multiples of %d (K=%lld ldw=%lld)", tag, vec, (long long)d->K,
               (long long)d->ldw);
    APAD_CHECK(al16(d->a) && al16(d->w) && al16(d->out) && al16(d->residual), "%s: pointers must be 16-byte aligned", tag);
    if (d->a_mode == APAD_A_PLAIN) {
        APAD_CHECK(d->lda % vec == 0, "%s: lda must be a multiple of %d", tag, vec);
    } else if (d->a_mode == APAD_A_CONV3X3) {
        APAD_CHECK(d->Cin > 0 && d->Cin % vec == 0 && d->K == 9LL * d->Cin, "%s: conv3x3 needs Cin%%%d==0 and K==9*Cin", tag, vec);
        APAD_CHECK(d->stride == 1 || d->stride == 2, "%s: conv stride must be 1 or 2", tag);
        APAD_CHECK(d->Hin > 0 && d->Win > 0 && d->Hout > 0 && d->Wout > 0 && d->M % ((int64_t)d->Hout * d->Wout) == 0,
                   "%s: conv geometry inconsistent with M", tag);
        APAD_CHECK((d->Hup > 0) == (d->Wup > 0), "%s: Hup/Wup must both be set or both 0", tag);
    } else if (d->a_mode == APAD_A_PATCH16) {
        APAD_CHECK(d->K == 256 && d->Hin % 16 == 0 && d->Win % 16 == 0, "%s: patch16 needs K==256 and H,W %% 16 == 0", tag);
        APAD_CHECK(d->M % ((int64_t)(d->Hin / 16) * (d->Win / 16)) == 0, "%s: patch16 M inconsistent", tag);
    } else if (d->a_mode == APAD_A_CONV1D) {
        APAD_CHECK(d->Cin > 0 && d->Cin % vec == 0 && d->taps > 0 && d->K == (int64_t)d->taps * d->Cin, "%s: conv1d needs Cin%%%d==0 and K==taps*Cin",
                   tag, vec);
        APAD_CHECK(d->Hin > 0 && d->Hout > 0 && d->M % d->Hout == 0 && d->pad >= 0, "%s: conv1d geometry inconsistent with M", tag);
        APAD_CHECK(d->transposed ? d->stride >= 1 : d->dilation >= 1, "%s: conv1d needs dilation >= 1 (stride >= 1 when transposed)", tag);
    }
    if (d->out_mode == APAD_OUT_ROWMAJOR) {
        APAD_CHECK(d->N % vec == 0 && d->ldo % vec == 0, "%s: N and ldo must be multiples of %d", tag, vec);
        if (d->residual) APAD_CHECK(d->ldr % vec == 0, "%s: ldr must be a multiple of %d", tag, vec);
        if (geglu) APAD_CHECK(d->N % (8 * vec) == 0, "%s: GEGLU needs N %% %d == 0", tag, 8 * vec);  // half a 64-element (16-bit) / 32-float tile row
    } else if (d->out_mode == APAD_OUT_QKV) {
        APAD_CHECK(d->out2 && d->out3 && al16(d->out2) && al16(d->out3), "%s: APAD_OUT_QKV needs 16-byte aligned out2 / out3", tag);
        if (out4) APAD_CHECK(al16(d->out4), "%s: out4 must be 16-byte aligned", tag);
        APAD_CHECK(d->heads > 0 && d->head_dim > 0 && d->L > 0 && d->Lpad >= d->L && d->N == 3LL * d->heads * d->head_dim &&
                       d->M % d->L == 0 && (d->N / 3) % (16 * vec) == 0 && d->ldo % vec == 0,
                   "%s: fused q|k|v geometry inconsistent (needs C %% %d == 0)", tag, 16 * vec);  // a tile lies in one third of the columns
        APAD_CHECK(!d->residual, "%s: fused q|k|v takes no residual", tag);
    } else if (d->out_mode == APAD_OUT_VT) {
        APAD_CHECK(d->heads > 0 && d->head_dim > 0 && d->L > 0 && d->Lpad >= d->L && d->N == (int64_t)d->heads * d->head_dim &&
                       d->M % d->L == 0,
                   "%s: V^T output geometry inconsistent", tag);
        APAD_CHECK(!d->residual, "%s: V^T output takes no residual", tag);
    } else {
        apad_set_error("%s: unknown out_mode %d", tag, d->out_mode);
        return -1;
    }
    if (d->rowgroup_bias) APAD_CHECK(d->ld_rg > 0, "%s: rowgroup_bias needs ld_rg", tag);
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// The 16-bit kernels' parameter block and their epilogue: accumulators (+ bias, + rowgroup bias / time-embedding row, folded
// LayerNorm, activation) -> LDS tile -> full-row 16-byte stores (GEGLU, residual, row statistics, q | k | v split, V^T).
// ---------------------------------------------------------------------------------------------------------------------------------
struct GemmP {
    const uint8_t* a;
    const uint8_t* w;
    uint8_t* out;
    uint8_t* out2;
    uint8_t* out3;
    uint8_t* out4;  // APAD_OUT_QKV: optional row-major v
    const uint8_t* bias;
    const uint8_t* residual;
    const uint8_t* rg;
    const int32_t* step_ptr;
    int64_t M, N, K, lda, ldw, ldo, ldr, ld_rg, rows_per_group;
    AGeom g;
    int32_t res_mod;
    int32_t heads, head_dim, L, Lpad;
    int32_t wrows;  // rows of w (N, or 2N for GEGLU)
    int32_t m_tiles, n_tiles;
    // LayerNorm folded into the contraction (apad_gemm_desc::rowstat_in): a = RAW rows, w = gamma-scaled weights,
    // out = rstd_m * (acc - mean_m * ln_cs[n]) + ln_bb[n]; the row statistics are summed from the producing kernel's partials
    float* rs_out;        // [M][rs_out_tiles][2]: per 64-column block (sum, sum of squares) of the stored output row
    const float* rs_in;   // [M][rs_in_tiles][2]
    const float* ln_cs;   // [w rows]
    const float* ln_bb;   // [w rows]
    int32_t rs_in_tiles, rs_out_tiles;
    float ln_eps;
    // two-source plain A (apad_gemm_desc::a2): columns >= ksplit of row m come from a2[(m % a2_mod) * lda2 + k - ksplit]
    const uint8_t* a2;
    int64_t lda2;
    int32_t ksplit, a_mod, a2_mod;
};

// LayerNorm-by-algebra: mean / rstd of the BM rows from m0 into rstat, summed in a fixed order from the producer's 64-column partials
template <int BM>
__device__ __forceinline__ void ln_row_stats(const float* rs_in, int rs_in_tiles, int64_t K, float ln_eps, int64_t m0, int64_t M, float (*rstat)[2]) {
    if (rs_in == nullptr || threadIdx.x >= BM) return;
    const int64_t m = m0 + threadIdx.x;
    float s1 = 0.f, s2 = 0.f;
    if (m < M) {
        const float* src = rs_in + m * rs_in_tiles * 2;
        for (int t_ = 0; t_ < rs_in_tiles; ++t_) {
            s1 += src[2 * t_];
            s2 += src[2 * t_ + 1];
        }
    }
    const float mean = s1 / (float)K;
    const float var = fmaxf(s2 / (float)K - mean * mean, 0.f);
    rstat[threadIdx.x][0] = mean;
    rstat[threadIdx.x][1] = rsqrtf(var + ln_eps);
}

// W row feeding local tile column nl (GEGLU: first half of the BN tile columns = value rows, second half = gate rows), and whether it exists
template <int EPI, int BN> __device__ __forceinline__ int64_t w_row(int64_t N, int64_t n0, int nl) {
    if (EPI == APAD_EPI_GEGLU) return nl < BN / 2 ? n0 + nl : N + n0 + (nl - BN / 2);
    return n0 + nl;
}
template <int EPI, int BN> __device__ __forceinline__ bool w_row_valid(int64_t N, int64_t n0, int nl) {
    if (EPI == APAD_EPI_GEGLU) return (nl < BN / 2 ? n0 + nl : n0 + nl - BN / 2) < N;
    return n0 + nl < N;
}

// what the epilogue adds along one tile column
struct EpiCol {
    bool nvalid;
    int64_t wr;
    float bv, rg0, lcs, lbb;
};
// nvalid: the column's W row exists (a kernel whose envelope has whole N tiles passes `true` and the guards fold away)
template <int DT> __device__ __forceinline__ EpiCol epi_column(const GemmP& p, bool nvalid, int64_t wrow, int64_t step, bool one_group) {
    EpiCol c;
    c.nvalid = nvalid;
    c.wr = nvalid ? wrow : 0;
    c.bv = (p.bias && nvalid) ? ld_elem<DT>(p.bias, c.wr) : 0.f;
    c.rg0 = (p.rg && one_group && nvalid) ? ld_elem<DT>(p.rg, step * p.ld_rg + c.wr) : 0.f;
    const bool lnf = p.rs_in != nullptr;
    c.lcs = (lnf && nvalid) ? p.ln_cs[c.wr] : 0.f;
    c.lbb = (lnf && nvalid) ? p.ln_bb[c.wr] : 0.f;
    return c;
}

// ONE 32x32 MFMA tile (a named f32x16, by value: accumulator arrays handed to a helper went to scratch) -> LDS tile ct, at local rows
// ml0 .. ml0 + 31, local column nl of this lane
template <int DT, int EPI, int C_LD>
__device__ __forceinline__ void epi_acc_to_lds(const GemmP& p, f32x16 acc, typename ET<DT>::elem* ct, const float (*rstat)[2], int ml0, int nl,
                                               int half, int64_t m0, const EpiCol& c, int64_t step, bool one_group) {
    const bool lnf = p.rs_in != nullptr;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int ml = ml0 + (r & 3) + 8 * (r >> 2) + 4 * half;
        float v = acc[r] + c.bv + c.rg0;
        if (lnf) v = rstat[ml][1] * (acc[r] - rstat[ml][0] * c.lcs) + c.lbb + c.rg0;
        if (p.rg && !one_group) {
            const int64_t m = m0 + ml;
            if (m < p.M && c.nvalid) v += ld_elem<DT>(p.rg, (m / p.rows_per_group + step) * p.ld_rg + c.wr);
        }
        if (EPI == APAD_EPI_SILU) v = silu_f(v);
        if (EPI == APAD_EPI_GELU) v = gelu_erf_f(v);
        if (EPI == APAD_EPI_TANH) v = tanhf(v);
        ct[ml * C_LD + nl] = (typename ET<DT>::elem)v;
    }
}

// LDS tile ct (BM x BN, row stride BN + 8) -> global, by all NT threads of the workgroup
template <int DT, int EPI, int OUTMODE, int BM, int BN, int NT>
__device__ __forceinline__ void epi_store(const GemmP& p, const typename ET<DT>::elem* ct, int64_t m0, int64_t n0) {
    using E = ET<DT>;
    constexpr int C_LD = BN + 8, GH = BN / 2;
    constexpr int BN_OUT = (EPI == APAD_EPI_GEGLU) ? BN / 2 : BN;
    // fused q|k|v: the tile lies in exactly one third of the columns (C % tile == 0, checked on the host)
    const int Cq = (int)(p.N / 3);
    const int qseg = (OUTMODE == APAD_OUT_QKV) ? (int)(n0 / Cq) : 0;
    if (OUTMODE == APAD_OUT_ROWMAJOR || (OUTMODE == APAD_OUT_QKV && qseg < 2)) {
        uint8_t* const obase = (OUTMODE == APAD_OUT_QKV && qseg == 1) ? p.out2 : p.out;
        const int64_t ncol0 = (OUTMODE == APAD_OUT_QKV) ? (int64_t)qseg * Cq : 0;
        constexpr int VPR = BN_OUT / 8;  // 16-byte vectors per output row
        if (p.rs_out != nullptr && VPR >= 8 && OUTMODE == APAD_OUT_ROWMAJOR) {
            // the same store loop, plus the row statistics of what is stored: 8 consecutive lanes own 64 consecutive columns of one
            // row (BM * VPR is a multiple of the thread count, so a group is never split and every lane takes part in the shuffles)
            for (int idx = threadIdx.x; idx < BM * VPR; idx += NT) {
                const int rl = idx / VPR, vc = idx - rl * VPR;
                const int64_t m = m0 + rl, n = n0 + vc * 8;
                const bool ok = m < p.M && n < p.N;
                float f[8];
                unpack8<DT>(*reinterpret_cast<const uint4*>(&ct[rl * C_LD + vc * 8]), f);
                if (p.residual && ok) {
                    float rr[8];
                    const int64_t rm = p.res_mod > 0 ? m % p.res_mod : m;
                    unpack8<DT>(*reinterpret_cast<const uint4*>(p.residual + (rm * p.ldr + n) * 2), rr);
#pragma unroll
                    for (int e = 0; e < 8; ++e) f[e] = (float)(typename E::elem)f[e] + rr[e];
                }
                const uint4 pk = pack8<DT>(f);
                float s1 = 0.f, s2 = 0.f;
                if (ok) {
                    *reinterpret_cast<uint4*>(obase + (m * p.ldo + (n - ncol0)) * 2) = pk;
                    float g[8];
                    unpack8<DT>(pk, g);  // statistics of the ROUNDED values: what the consumer will read
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        s1 += g[e];
                        s2 = __builtin_fmaf(g[e], g[e], s2);
                    }
                }
#pragma unroll
                for (int o_ = 1; o_ < 8; o_ <<= 1) {
                    s1 += __shfl_xor(s1, o_);
                    s2 += __shfl_xor(s2, o_);
                }
                if (ok && (vc & 7) == 0) {
                    float* dst = p.rs_out + (m * p.rs_out_tiles + (n >> 6)) * 2;
                    dst[0] = s1;
                    dst[1] = s2;
                }
            }
        } else
        for (int idx = threadIdx.x; idx < BM * VPR; idx += NT) {
            const int rl = idx / VPR, vc = idx - rl * VPR;
            const int64_t m = m0 + rl, n = n0 + vc * 8;
            if (m >= p.M || n >= p.N) continue;
            float f[8];
            unpack8<DT>(*reinterpret_cast<const uint4*>(&ct[rl * C_LD + vc * 8]), f);
            if (EPI == APAD_EPI_GEGLU) {
                float g[8];
                unpack8<DT>(*reinterpret_cast<const uint4*>(&ct[rl * C_LD + GH + vc * 8]), g);
#pragma unroll
                for (int e = 0; e < 8; e += 2) {
                    const apad_f32x2 ge = gelu_erf_2((apad_f32x2){g[e], g[e + 1]});
                    f[e] *= ge[0];
                    f[e + 1] *= ge[1];
                }
            }
            if (p.residual) {
                float rr[8];
                const int64_t rm = p.res_mod > 0 ? m % p.res_mod : m;
                unpack8<DT>(*reinterpret_cast<const uint4*>(p.residual + (rm * p.ldr + n) * 2), rr);
                // the un-fused reference rounds the linear output to the storage type before the add
#pragma unroll
                for (int e = 0; e < 8; ++e) f[e] = (float)(typename E::elem)f[e] + rr[e];
            }
            *reinterpret_cast<uint4*>(obase + (m * p.ldo + (n - ncol0)) * 2) = pack8<DT>(f);
        }
    } else {  // APAD_OUT_VT (or the v third of APAD_OUT_QKV): consecutive lanes -> consecutive tokens of one (head, dd) row
        typename E::elem* o = reinterpret_cast<typename E::elem*>(OUTMODE == APAD_OUT_QKV ? p.out3 : p.out);
        const int64_t nsub = (OUTMODE == APAD_OUT_QKV) ? 2 * (int64_t)Cq : 0;
        if (OUTMODE == APAD_OUT_QKV && p.out4 != nullptr) {  // v row-major as well (the training step keeps both forms)
            for (int idx = threadIdx.x; idx < BM * (BN / 8); idx += NT) {
                const int rl = idx / (BN / 8), vc = idx - rl * (BN / 8);
                const int64_t m = m0 + rl, n = n0 + vc * 8;
                if (m < p.M && n < p.N) *reinterpret_cast<uint4*>(p.out4 + (m * p.ldo + (n - nsub)) * 2) = *reinterpret_cast<const uint4*>(&ct[rl * C_LD + vc * 8]);
            }
        }
        for (int idx = threadIdx.x; idx < BM * BN; idx += NT) {
            const int nl = idx / BM, rl = idx % BM;
            const int64_t m = m0 + rl;
            int64_t n = n0 + nl;
            if (m >= p.M || n >= p.N) continue;
            n -= nsub;
            const int64_t b = m / p.L;
            const int l = (int)(m - b * p.L);
            const int h = (int)(n / p.head_dim), dd = (int)(n - (int64_t)h * p.head_dim);
            o[((b * p.heads + h) * p.head_dim + dd) * p.Lpad + l] = ct[rl * C_LD + nl];
        }
    }
}

}  // namespace
