// K pipeline of the decode GEMVs, shared by gemv.hip and head_argmax.hip
// (piece geometry: gemv_tile.h).
//
// A row is walked in pieces of D unit-rows (D * 64 16-B units): KU deep while
// that many whole unit-rows are left, then 4, 2, 1 as they fit, so every such piece is
// free of per-load predicates and its slots sit at immediate offsets from one
// address. Only the partial unit-row of a K % 512 != 0 shape is predicated
// (depth 1): a dead lane loads nothing and feeds zeros — fmaf(0, 0, acc)
// leaves acc untouched. All arrays are indexed by unrolled constants only, so
// they live in VGPRs.
#pragma once

#include "common.h"
#include "gemv_tile.h"

typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;

__device__ __forceinline__ u32x4 nt_load4(const uint32_t* p) {
    return __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(p));
}

// Keeps the scheduler from hoisting every slot's bf16 unpacking above the
// first FMA: unfenced, the consume of a deep piece holds all its unpacked
// floats at once and the VGPR count (hence resident waves) suffers.
#define GEMV_SLOT_FENCE() __builtin_amdgcn_sched_barrier(0)

__device__ __forceinline__ u32x4 ld4(const uint32_t* p) {
    return *reinterpret_cast<const u32x4*>(p);
}

// one rstd piece: D x loads in flight, then the single ss chain in K order
template <int D, bool PARTIAL>
__device__ __forceinline__ float rstd_piece(const uint32_t* xrow, int k2, int r,
                                            int lane, float ss) {
    const uint32_t* p = xrow + gemv_slot_word(r, 0, lane);  // slot s: + s * 256
    u32x4 xv[D];
#pragma unroll
    for (int s = 0; s < D; ++s) {
        if (PARTIAL) xv[s] = u32x4{0u, 0u, 0u, 0u};
        if (!PARTIAL || gemv_partial_live(k2, lane)) xv[s] = ld4(p + s * 256);
    }
#pragma unroll
    for (int s = 0; s < D; ++s) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float lo = bf16_lo(xv[s][j]), hi = bf16_hi(xv[s][j]);
            ss = fmaf(lo, lo, ss);
            ss = fmaf(hi, hi, ss);
        }
        GEMV_SLOT_FENCE();
    }
    return ss;
}

// row_rstd for the fused-norm VALU GEMVs: the same single `ss` chain in
// ascending K, but XD 16-B x loads are in flight before the first is consumed
// (K = 4096 is ONE trip at XD = 8) instead of one L2 round trip per load.
template <int XD>
__device__ __forceinline__ float row_rstd_pipe(const uint32_t* xrow, int k2,
                                               int lane, float eps) {
    float ss = 0.0f;
    int r = 0;
    for (int d; (d = gemv_piece_depth(k2, XD, r)) > 0; r += d) {
        if (d == XD) ss = rstd_piece<XD, false>(xrow, k2, r, lane, ss);
        else if (XD > 4 && d == 4) ss = rstd_piece<4, false>(xrow, k2, r, lane, ss);
        else if (XD > 2 && d == 2) ss = rstd_piece<2, false>(xrow, k2, r, lane, ss);
        else ss = rstd_piece<1, false>(xrow, k2, r, lane, ss);
    }
    if (gemv_slot_word(r, 0, 0) < k2) ss = rstd_piece<1, true>(xrow, k2, r, lane, ss);
    ss = wave_reduce_sum(ss);
    return rsqrtf(ss / (float)(k2 * 2) + eps);
}

// One piece of one row group: issue D W loads per row and the matching x
// (and norm-weight) loads back to back, then consume the slots in order —
// one accumulator per (row, m), ascending K, low half before high half, i.e.
// the order of the one-load-per-trip loop.
//
// NORM: W does not depend on rstd, so on a wave's first piece the W loads go
// out FIRST and the whole rstd prologue (x loads, ss chain, wave reduction)
// runs under their HBM latency; `need_rstd` is wave-uniform.
//
// M > 2 (depth 1, not on the hot path) reads x inside the consume loop as the
// original kernel did, to keep its register footprint.
template <int M, bool NORM, int RW, int D, int XD, bool PARTIAL>
__device__ __forceinline__ void gemv_piece_step(
    float (&acc)[RW][M], float (&rstd)[M], bool& need_rstd,
    const uint32_t* (&wr)[RW], const uint32_t* x, const uint32_t* wn, int k2,
    int r, int lane, float eps) {
    constexpr bool XPRE = M == 1;
    const u32x4 zero = {0u, 0u, 0u, 0u};
    const bool on = !PARTIAL || gemv_partial_live(k2, lane);
    const int i0 = gemv_slot_word(r, 0, lane);  // slot s: + s * 256 words

    u32x4 wv[D][RW], xv[D][M], nv[D];
    if (XPRE && !NORM) {
#pragma unroll
        for (int s = 0; s < D; ++s)
#pragma unroll
            for (int m = 0; m < M; ++m) {
                if (PARTIAL) xv[s][m] = zero;
                if (on) xv[s][m] = ld4(x + (size_t)m * k2 + i0 + s * 256);
            }
    }
    // stream W non-temporally: each byte is read exactly once per step; keep
    // L2 for the KV cache and activations
#pragma unroll
    for (int s = 0; s < D; ++s)
#pragma unroll
        for (int rr_ = 0; rr_ < RW; ++rr_) {
            if (PARTIAL) wv[s][rr_] = zero;
            if (on) wv[s][rr_] = nt_load4(wr[rr_] + i0 + s * 256);
        }
    if (NORM) {
        if (need_rstd) {
#pragma unroll
            for (int m = 0; m < M; ++m)
                rstd[m] = row_rstd_pipe<XD>(x + (size_t)m * k2, k2, lane, eps);
            need_rstd = false;
        }
        if (XPRE) {
#pragma unroll
            for (int s = 0; s < D; ++s) {
#pragma unroll
                for (int m = 0; m < M; ++m) {
                    if (PARTIAL) xv[s][m] = zero;
                    if (on) xv[s][m] = ld4(x + (size_t)m * k2 + i0 + s * 256);
                }
                if (PARTIAL) nv[s] = zero;
                if (on) nv[s] = ld4(wn + i0 + s * 256);
            }
        }
    }

#pragma unroll
    for (int s = 0; s < D; ++s) {
        u32x4 nq = zero;
        if (NORM) {
            if (XPRE) nq = nv[s];
            else if (on) nq = ld4(wn + i0 + s * 256);
        }
#pragma unroll
        for (int m = 0; m < M; ++m) {
            u32x4 xq = zero;
            if (XPRE) xq = xv[s][m];
            else if (on) xq = ld4(x + (size_t)m * k2 + i0 + s * 256);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float xl = bf16_lo(xq[j]), xh = bf16_hi(xq[j]);
                if (NORM) {
                    const uint32_t wnw = nq[j];
                    xl *= rstd[m] * bf16_lo(wnw);
                    xh *= rstd[m] * bf16_hi(wnw);
                }
#pragma unroll
                for (int rr_ = 0; rr_ < RW; ++rr_) {
                    acc[rr_][m] = fmaf(xl, bf16_lo(wv[s][rr_][j]), acc[rr_][m]);
                    acc[rr_][m] = fmaf(xh, bf16_hi(wv[s][rr_][j]), acc[rr_][m]);
                }
            }
        }
        GEMV_SLOT_FENCE();
    }
}

// all pieces of one row group: KU deep, then the 4/2/1-deep tail, then the
// partial unit-row if K % 512 != 0
template <int M, bool NORM, int RW, int KU, int XD>
__device__ __forceinline__ void gemv_row_pieces(
    float (&acc)[RW][M], float (&rstd)[M], bool& need_rstd,
    const uint32_t* (&wr)[RW], const uint32_t* x, const uint32_t* wn, int k2,
    int lane, float eps) {
#define GEMV_STEP(DV, PV)                                                      \
    gemv_piece_step<M, NORM, RW, DV, XD, PV>(acc, rstd, need_rstd, wr, x, wn,  \
                                             k2, r, lane, eps)
    int r = 0;
    for (int d; (d = gemv_piece_depth(k2, KU, r)) > 0; r += d) {
        if (d == KU) GEMV_STEP(KU, false);
        else if (KU > 4 && d == 4) GEMV_STEP(4, false);
        else if (KU > 2 && d == 2) GEMV_STEP(2, false);
        else GEMV_STEP(1, false);
    }
    if (gemv_slot_word(r, 0, 0) < k2) GEMV_STEP(1, true);
#undef GEMV_STEP
}
