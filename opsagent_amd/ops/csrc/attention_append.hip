// Paged APPEND attention for MI355X (gfx950): B sequences, each with
// L_b in [1, 16] new query tokens, attend causally over the paged KV cache in
// place — the case between decode (1 token/sequence, VALU dot products) and
// prefill (many tokens, contiguous K/V). Jump-ahead catch-up, speculative
// verify and mixed decode steps use it instead of gathering the whole past
// out of the cache for the prefill kernel.
//
// Layouts:
//   q        [T, Hq, 128] bf16, token stride qs (a head-slice view)
//   kc/vc    flat [num_slots, Hk, 128] bf16 (slot = block_id*block_size + off)
//   block_table [B, max_blocks] int32, seq_lens [B] int32 (keys INCLUDING the
//   new ones, already written by rope_kv), cu_q [B+1] int32
//   o_part   [(B*Hk*nsplit) * rmax, 128] f32   (rmax = max_q * G rows)
//   ml_part  [(B*Hk*nsplit) * rmax, 2]   f32   (m in the exp2 domain, l)
//   out      [T, Hq, 128] bf16
//
// Rows: the R = L*G (token, q-head) pairs that share kv-head h form the
// q-rows of a block, row = j*G + gh, causal limit p = n - L + j.
//
// MFMA form (v_mfma_f32_16x16x32_bf16, swapped as in the prefill kernel):
//   S^T[key][row] = K · Q^T. With the A-operand map (lane l holds
//   A[row l&15][k = 8(l>>4)+j]) a 16-key x 128-dim K tile is four 16-B global
//   loads per lane straight into the A fragments — K never touches LDS. The
//   lane's q-row is l&15, so the softmax statistics are per-lane scalars
//   merged over the four 16-lane groups.
//   O^T[dim][row] = V^T · P^T. Lane group g holds P for keys 4g..4g+3 of each
//   16-key tile; the MFMA k index is free to permute as long as A and B
//   agree, so one 32-key step takes k = 8g+j -> key (j<4 ? 4g+j : 16+4g+j-4)
//   and the P fragment is the lane's own registers, no exchange. The V^T
//   fragment under the same permutation is two ds_read_b64_tr_b16 of a
//   wave-private row-major LDS image (guide T10 image (b)).
//
// Work split: a block owns (b, h, split); its four waves either split the
// split's keys (R <= 16*NRT: every wave carries all row tiles) or split the
// row tiles (wave w owns tiles w, w+4; all waves walk every key, so K/V come
// from HBM once and from L2 after). Wave-private V images mean the main loop
// has no block barrier.
//
// fp8 cache (FP8 = true, the layout of kv_fp8.hip): kc/vc are e4m3 codes
// uint8 [num_slots, Hk, 128] with one f32 scale per (slot, kv-head) row. The
// codes become bf16 EXACTLY (every e4m3 value is a bf16 value) and feed the
// MFMAs unscaled; the scales fold in fp32 on the other side of each product:
//   score = (K_codes · q) * k_scale[key]          before the scale*log2e fold
//   O    += V_codes^T · bf16(p * v_scale[key])    one rounding; l keeps p
// A lane's eight scores and eight P values of a step belong to the same keys
// kb0 + 16t + 4fs + r, so one 4-B load per lane per step (k_scale of key
// kb0 + lane in the lower half-wave, v_scale of key kb0 + lane - 32 in the
// upper) fetches every scale the wave needs; a 256-B wave-private LDS strip
// hands them out as four b128 reads. Everything else — partition, masks,
// softmax, P·V, merges, combine — is the one code path.

#include "common.h"

#define DHEAD 128
#define APPEND_MAX_Q 16

typedef __attribute__((ext_vector_type(8))) short bf16x8_t;
typedef __attribute__((ext_vector_type(4))) float f32x4_t;
typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4v;
typedef __attribute__((ext_vector_type(4))) uint32_t u32x4_t;
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2v_t;

// byte offset of 16-byte chunk ch (0..15) of row `row` in a [32][128] bf16
// image with 256-B rows; the XOR serves the b128 writes and the tr reads
__device__ __forceinline__ uint32_t v_img_off(int row, int ch) {
    return 256u * row + 16u * (ch ^ (((row & 3) << 2) | ((row >> 2) & 3)));
}

// flat cache slot of `key`, clamped into [0, last_key]; (b0, e0..e2) are the
// block-table entries of the step's first block and the two after it
template <bool SMALLBS>
__device__ __forceinline__ size_t append_slot(int key, int last_key, int block_shift,
                                              int bmask, const int* __restrict__ btrow,
                                              int max_blocks, int b0, int e0, int e1,
                                              int e2) {
    const int kk = max(min(key, last_key), 0);
    const int blk = kk >> block_shift;
    int entry;
    if (SMALLBS)
        entry = btrow[min(blk, max_blocks - 1)];
    else
        entry = (blk == b0) ? e0 : ((blk == b0 + 1) ? e1 : e2);
    return ((size_t)entry << block_shift) | (size_t)(kk & bmask);
}

// two e4m3 codes (byte pair `HI` of w) -> two bf16, exact (every e4m3 value
// is a bf16 value): one v_cvt_scalef32_pk_bf16_fp8 with the scale 1.0. It
// gives the bits of v_cvt_pk_f32_fp8 followed by the high halves of the two
// f32 (three instructions; measured 5-10 % slower on the row-tile shapes);
// the `codes_all` parity case covers every non-NaN code.
template <bool HI>
__device__ __forceinline__ uint32_t fp8x2_to_bf16x2(uint32_t w) {
    const bf16x2v_t b = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w, 1.0f, HI);
    return __builtin_bit_cast(uint32_t, b);
}

// 8 e4m3 codes (element-linear bytes) -> 8 bf16 in element order
__device__ __forceinline__ u32x4_t fp8x8_to_bf16x8(const uint2& w) {
    u32x4_t o;
    o[0] = fp8x2_to_bf16x2<false>(w.x);
    o[1] = fp8x2_to_bf16x2<true>(w.x);
    o[2] = fp8x2_to_bf16x2<false>(w.y);
    o[3] = fp8x2_to_bf16x2<true>(w.y);
    return o;
}

// what a lane holds of the step ahead: K fragments and V image rows as loaded
template <bool FP8> struct AppendRaw {
    typedef bf16x8_t k_t;
    typedef u32x4_t v_t;
};
template <> struct AppendRaw<true> {
    typedef uint2 k_t;
    typedef uint2 v_t;
};

template <int NRT, bool SMALLBS, bool FP8>
__global__ __launch_bounds__(256) void append_attn_kernel(
    const uint16_t* __restrict__ q, const void* __restrict__ kcv,
    const void* __restrict__ vcv, const float* __restrict__ kscl,
    const float* __restrict__ vscl, const int* __restrict__ block_table,
    const int* __restrict__ seq_lens, const int* __restrict__ cu_q,
    float* __restrict__ o_part, float* __restrict__ ml_part, int Hk,
    int gshift /* log2(G) */, int max_blocks, int block_shift, int nsplit,
    float scale2 /* scale * log2(e) */, int qs, int rmax) {
    constexpr int ROWS = 16 * NRT;         // rows a key-splitting wave carries
    constexpr int V_BYTES = 32 * DHEAD * 2;  // one wave's 32-key V image
    constexpr int MO_BYTES = 4 * ROWS * DHEAD * 4;
    constexpr int SMEM = MO_BYTES > 4 * V_BYTES ? MO_BYTES : 4 * V_BYTES;
    __shared__ __attribute__((aligned(16))) char smem[SMEM];
    __shared__ float s_ml[4][ROWS][2];
    // fp8 only: per wave, k_scale of the step's 32 keys then their v_scale
    __shared__ __attribute__((aligned(16))) float s_scl[FP8 ? 4 * 64 : 1];
    typedef typename AppendRaw<FP8>::k_t kraw_t;
    typedef typename AppendRaw<FP8>::v_t vraw_t;
    const uint16_t* kc = reinterpret_cast<const uint16_t*>(kcv);
    const uint16_t* vc = reinterpret_cast<const uint16_t*>(vcv);
    const uint8_t* kc8 = reinterpret_cast<const uint8_t*>(kcv);
    const uint8_t* vc8 = reinterpret_cast<const uint8_t*>(vcv);

    const int bh = blockIdx.x;
    const int b = bh / Hk;
    const int h = bh % Hk;
    const int split = blockIdx.y;
    const int G = 1 << gshift;

    const int lane = threadIdx.x & (WAVE - 1);
    const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x / WAVE);
    const int fr = lane & 15;  // q-row within a tile / key within a K tile
    const int fs = lane >> 4;  // 16-lane group

    const int n = seq_lens[b];
    const int t0 = cu_q[b];
    const int L = min(cu_q[b + 1] - t0, APPEND_MAX_Q);
    const int R = min(L << gshift, rmax);
    const int ntile = (R + 15) >> 4;

    const int chunk = CEIL_DIV(max(n, 0), nsplit);
    const int kstart = split * chunk;
    const int kend = min(n, kstart + chunk);

    // block-uniform mode: split keys over the waves, or split row tiles
    const bool ksplit = ntile <= NRT;
    int wstart, wend, tile0, tstep;
    if (ksplit) {
        const int span = max(kend - kstart, 0);
        const int wchunk = CEIL_DIV(CEIL_DIV(span, 4), 32) * 32;
        wstart = kstart + wid * wchunk;
        wend = min(kend, wstart + wchunk);
        tile0 = 0;
        tstep = 1;
    } else {
        wstart = kstart;
        wend = kend;
        tile0 = wid;
        tstep = 4;
    }
    if (tile0 >= ntile) wend = wstart;  // wave owns no row tile

    // ---- Q B-fragments: bq[rt][s] = Q[row][d = 32s + 8fs .. +7] -----------
    uint4 bq[NRT][4];
    int plim[NRT];
    int rowi[NRT];
#pragma unroll
    for (int rt = 0; rt < NRT; ++rt) {
        const int row = (tile0 + rt * tstep) * 16 + fr;
        rowi[rt] = row;
        if (row < R) {
            const int j = row >> gshift;
            const int gh = row & (G - 1);
            plim[rt] = n - L + j;
            const uint16_t* qp = q + (size_t)(t0 + j) * qs +
                                 (size_t)(h * G + gh) * DHEAD + fs * 8;
#pragma unroll
            for (int s = 0; s < 4; ++s)
                bq[rt][s] = *reinterpret_cast<const uint4*>(qp + s * 32);
        } else {
            plim[rt] = -1;  // padded row: every key masked, never stored
#pragma unroll
            for (int s = 0; s < 4; ++s) bq[rt][s] = make_uint4(0, 0, 0, 0);
        }
    }

    float m[NRT], lsum[NRT];
    f32x4_t acc[NRT][8];
#pragma unroll
    for (int rt = 0; rt < NRT; ++rt) {
        m[rt] = -INFINITY;
        lsum[rt] = 0.0f;
#pragma unroll
        for (int db = 0; db < 8; ++db) acc[rt][db] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
    }

    const int bmask = (1 << block_shift) - 1;
    const int* btrow = block_table + (size_t)b * max_blocks;
    const int last_key = n - 1;
    char* vbuf = smem + wid * V_BYTES;
    // keys <= n - L are visible to every row; the mask costs only past them
    const int all_visible_end = n - L + 1;

    // A 32-key step touches at most three blocks when block_size >= 16:
    // their table entries come by SCALAR loads, one step ahead, so the
    // per-lane slot is a select and the K/V loads do not queue behind a
    // block-table load on the same counter (which would drain the loads in
    // flight at every step). Smaller blocks take a per-lane table load.
    // Tail keys clamp to the last valid key and table reads clamp to the
    // row, so every load is in bounds whatever n, L and the split are.
    int e_b0, e_e0, e_e1, e_e2;
#define LOAD_ENT(KB0)                                                             \
    do {                                                                          \
        e_b0 = __builtin_amdgcn_readfirstlane(min((KB0), max(last_key, 0)) >>     \
                                              block_shift);                       \
        e_e0 = btrow[min(e_b0, max_blocks - 1)];                                  \
        e_e1 = btrow[min(e_b0 + 1, max_blocks - 1)];                              \
        e_e2 = btrow[min(e_b0 + 2, max_blocks - 1)];                              \
    } while (0)
#define SLOT_OF(KEY)                                                              \
    append_slot<SMALLBS>((KEY), last_key, block_shift, bmask, btrow, max_blocks,  \
                         e_b0, e_e0, e_e1, e_e2)
    // K A-fragments: key kb0 + 16t + fr, dims 32s + 8fs .. +7 (fp8: the
    // same elements as 8 B of codes)
#define LOAD_K(KB0)                                                               \
    _Pragma("unroll") for (int t = 0; t < 2; ++t) {                               \
        const size_t ke =                                                         \
            (SLOT_OF((KB0) + 16 * t + fr) * Hk + h) * DHEAD + fs * 8;             \
        _Pragma("unroll") for (int s = 0; s < 4; ++s) {                           \
            if constexpr (FP8)                                                    \
                ak[t][s] = *reinterpret_cast<const kraw_t*>(kc8 + ke + s * 32);   \
            else                                                                  \
                ak[t][s] = *reinterpret_cast<const kraw_t*>(kc + ke + s * 32);    \
        }                                                                         \
    }
    // V rows for the LDS image: key kb0 + 4i + fs, chunk fr
#define LOAD_V(KB0)                                                               \
    _Pragma("unroll") for (int i = 0; i < 8; ++i) {                               \
        const size_t ve =                                                         \
            (SLOT_OF((KB0) + 4 * i + fs) * Hk + h) * DHEAD + fr * 8;              \
        if constexpr (FP8)                                                        \
            vv[i] = *reinterpret_cast<const vraw_t*>(vc8 + ve);                   \
        else                                                                      \
            vv[i] = *reinterpret_cast<const vraw_t*>(vc + ve);                    \
    }
    // fp8 scales of the step: lane l < 32 takes k_scale of key kb0 + l, lane
    // l >= 32 v_scale of key kb0 + l - 32, clamped like every other load
#define LOAD_SC(KB0)                                                              \
    if constexpr (FP8)                                                            \
        sraw = (lane < 32 ? kscl : vscl)[SLOT_OF((KB0) + (lane & 31)) * Hk + h];

    // One step ahead: step i's K and V are in registers when it starts.
    // V(i) goes to the LDS image and V(i+1) is requested at once; K(i+1)
    // is requested as soon as the S^T MFMAs have read K(i), so both stream
    // under the softmax and P·V of step i. The look-ahead loads are
    // unconditional: past the range they clamp to the last valid key.
    kraw_t ak[2][4] = {};
    vraw_t vv[8] = {};
    float sraw = 0.0f;
    float* sstrip = s_scl + (FP8 ? wid * 64 : 0);
    LOAD_ENT(wstart);
    LOAD_V(wstart)
    LOAD_SC(wstart)
    LOAD_K(wstart)
    LOAD_ENT(wstart + 32);

    for (int kb0 = wstart; kb0 < wend; kb0 += 32) {
        // ---- V image. A wave's LDS operations execute in issue order, so
        // these writes land after the previous step's tr reads and before
        // this step's; the image is wave-private, no barrier is needed.
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            u32x4_t vrow;
            if constexpr (FP8) vrow = fp8x8_to_bf16x8(vv[i]);
            else vrow = vv[i];
            *reinterpret_cast<u32x4_t*>(vbuf + v_img_off(4 * i + fs, fr)) = vrow;
        }
        // the scale strip follows the same rule: this write lands after the
        // previous step's reads of it and before this step's
        if constexpr (FP8) sstrip[lane] = sraw;
        LOAD_V(kb0 + 32)
        LOAD_SC(kb0 + 32)

        const bool need_mask = (kb0 + 32 > wend) || (kb0 + 32 > all_visible_end);

        // ---- S^T = K · Q^T ------------------------------------------------
        f32x4_t sall[NRT][2];
        if constexpr (FP8) {
            // codes -> exact bf16 once per step, shared by the row tiles
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                bf16x8_t akb[4];
#pragma unroll
                for (int s = 0; s < 4; ++s)
                    akb[s] = __builtin_bit_cast(bf16x8_t, fp8x8_to_bf16x8(ak[t][s]));
#pragma unroll
                for (int rt = 0; rt < NRT; ++rt) {
                    if (tile0 + rt * tstep >= ntile) continue;  // wave-uniform
                    f32x4_t a = (f32x4_t){0.f, 0.f, 0.f, 0.f};
#pragma unroll
                    for (int s = 0; s < 4; ++s)
                        a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                            akb[s], *reinterpret_cast<bf16x8_t*>(&bq[rt][s]), a, 0, 0, 0);
                    sall[rt][t] = a;
                }
            }
        } else {
#pragma unroll
            for (int rt = 0; rt < NRT; ++rt) {
                if (tile0 + rt * tstep >= ntile) continue;  // wave-uniform
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    f32x4_t a = (f32x4_t){0.f, 0.f, 0.f, 0.f};
#pragma unroll
                    for (int s = 0; s < 4; ++s)
                        a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                            ak[t][s], *reinterpret_cast<bf16x8_t*>(&bq[rt][s]), a, 0, 0, 0);
                    sall[rt][t] = a;
                }
            }
        }
        LOAD_K(kb0 + 32)
        LOAD_ENT(kb0 + 64);

        // fp8: k_scale / v_scale of the lane's keys kb0 + 16t + 4fs + r
        f32x4_t ksc[2], vsc[2];
        if constexpr (FP8) {
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                ksc[t] = *reinterpret_cast<const f32x4_t*>(sstrip + 16 * t + 4 * fs);
                vsc[t] = *reinterpret_cast<const f32x4_t*>(sstrip + 32 + 16 * t + 4 * fs);
            }
        }

        // ---- mask, online softmax -----------------------------------------
        union PF {
            uint32_t u[4];
            bf16x8_t v8;
        } pf[NRT];
#pragma unroll
        for (int rt = 0; rt < NRT; ++rt) {
            if (tile0 + rt * tstep >= ntile) continue;  // wave-uniform
            f32x4_t st[2] = {sall[rt][0], sall[rt][1]};
            if constexpr (FP8) {
                st[0] *= ksc[0];
                st[1] *= ksc[1];
            }
            // lane's score st[t][r] is key kb0 + 16t + 4fs + r of its row
            if (need_mask) {
                const int lim = min(wend - 1, plim[rt]);
#pragma unroll
                for (int t = 0; t < 2; ++t)
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        if (kb0 + 16 * t + 4 * fs + r > lim) st[t][r] = -INFINITY;
            }
            float rowmax = fmaxf(fmaxf(fmaxf(st[0][0], st[0][1]), fmaxf(st[0][2], st[0][3])),
                                 fmaxf(fmaxf(st[1][0], st[1][1]), fmaxf(st[1][2], st[1][3])));
            rowmax = fmaxf(rowmax, __shfl_xor(rowmax, 16, WAVE));
            rowmax = fmaxf(rowmax, __shfl_xor(rowmax, 32, WAVE));
            const float mn = fmaxf(m[rt], rowmax);
            // a row with no visible key yet keeps m = -inf: exponent base 0
            const float mnb = (mn == -INFINITY) ? 0.0f : mn * scale2;
            const float alpha =
                __builtin_amdgcn_exp2f(__builtin_fmaf(m[rt], scale2, -mnb));
            m[rt] = mn;
            float p[2][4];
            float psum = 0.0f;
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    p[t][r] = __builtin_amdgcn_exp2f(
                        __builtin_fmaf(st[t][r], scale2, -mnb));
                    psum += p[t][r];
                }
            lsum[rt] = lsum[rt] * alpha + psum;  // per-group partial sum
#pragma unroll
            for (int db = 0; db < 8; ++db)
#pragma unroll
                for (int r = 0; r < 4; ++r) acc[rt][db][r] *= alpha;
            // fp8: v_scale rides on P in fp32, one rounding; l kept p itself
            if constexpr (FP8) {
#pragma unroll
                for (int t = 0; t < 2; ++t)
#pragma unroll
                    for (int r = 0; r < 4; ++r) p[t][r] *= vsc[t][r];
            }
            // P^T B-fragment: k = 8fs + j <-> key (j<4 ? 4fs+j : 16+4fs+j-4)
            pf[rt].u[0] = pack_bf16x2(p[0][0], p[0][1]);
            pf[rt].u[1] = pack_bf16x2(p[0][2], p[0][3]);
            pf[rt].u[2] = pack_bf16x2(p[1][0], p[1][1]);
            pf[rt].u[3] = pack_bf16x2(p[1][2], p[1][3]);
        }

        // ---- O^T += V^T · P^T; lane 4q+p supplies row r0+q, dims 4p..4p+3 --
        const int tq = fr >> 2, tp = fr & 3;
#pragma unroll
        for (int db = 0; db < 8; ++db) {
            const bf16x4v r0 = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(
                (__attribute__((address_space(3))) bf16x4v*)(
                    vbuf + v_img_off(4 * fs + tq, 2 * db + (tp >> 1)) +
                    8 * (tp & 1)));
            const bf16x4v r1 = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(
                (__attribute__((address_space(3))) bf16x4v*)(
                    vbuf + v_img_off(16 + 4 * fs + tq, 2 * db + (tp >> 1)) +
                    8 * (tp & 1)));
            union {
                struct { bf16x4v lo, hi; } p;
                bf16x8_t v8;
            } av;
            av.p.lo = r0;
            av.p.hi = r1;
#pragma unroll
            for (int rt = 0; rt < NRT; ++rt) {
                if (tile0 + rt * tstep >= ntile) continue;  // wave-uniform
                acc[rt][db] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                    av.v8, pf[rt].v8, acc[rt][db], 0, 0, 0);
            }
        }
    }

#undef LOAD_ENT
#undef SLOT_OF
#undef LOAD_K
#undef LOAD_V
#undef LOAD_SC

    // the four groups hold the same m and disjoint key sums
#pragma unroll
    for (int rt = 0; rt < NRT; ++rt) {
        lsum[rt] += __shfl_xor(lsum[rt], 16, WAVE);
        lsum[rt] += __shfl_xor(lsum[rt], 32, WAVE);
    }

    const size_t part_row0 = ((size_t)bh * nsplit + split) * rmax;

    if (!ksplit) {
        // each wave owns whole rows: publish (m, l, o) straight to the slab.
        // lane holds O[row][dims 16db + 4fs .. +3]
#pragma unroll
        for (int rt = 0; rt < NRT; ++rt) {
            const int row = rowi[rt];
            if (row >= R) continue;
            float* op = o_part + (part_row0 + row) * DHEAD + 4 * fs;
#pragma unroll
            for (int db = 0; db < 8; ++db)
                *reinterpret_cast<float4*>(op + db * 16) = make_float4(
                    acc[rt][db][0], acc[rt][db][1], acc[rt][db][2], acc[rt][db][3]);
            if (fs == 0) {
                float* mp = ml_part + (part_row0 + row) * 2;
                mp[0] = m[rt] * scale2;
                mp[1] = lsum[rt];
            }
        }
        return;
    }

    // key-split: merge the four waves' partials through LDS (the V images
    // are dead once every wave is past its loop)
    __syncthreads();
    float* mo = reinterpret_cast<float*>(smem);
#pragma unroll
    for (int rt = 0; rt < NRT; ++rt) {
        const int row = rowi[rt];  // < ROWS in this mode
        float* op = mo + ((size_t)(wid * ROWS + row)) * DHEAD + 4 * fs;
#pragma unroll
        for (int db = 0; db < 8; ++db)
            *reinterpret_cast<float4*>(op + db * 16) = make_float4(
                acc[rt][db][0], acc[rt][db][1], acc[rt][db][2], acc[rt][db][3]);
        if (fs == 0) {
            s_ml[wid][row][0] = m[rt] * scale2;
            s_ml[wid][row][1] = lsum[rt];
        }
    }
    __syncthreads();
    for (int idx = threadIdx.x; idx < R * DHEAD; idx += blockDim.x) {
        const int row = idx >> 7;
        const int d = idx & (DHEAD - 1);
        float mt = -INFINITY;
#pragma unroll
        for (int w = 0; w < 4; ++w)
            if (s_ml[w][row][1] > 0.0f) mt = fmaxf(mt, s_ml[w][row][0]);
        float lt = 0.0f, ot = 0.0f;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const float lw = s_ml[w][row][1];
            if (lw > 0.0f) {
                const float sc = __builtin_amdgcn_exp2f(s_ml[w][row][0] - mt);
                lt += lw * sc;
                ot += mo[(size_t)(w * ROWS + row) * DHEAD + d] * sc;
            }
        }
        o_part[(part_row0 + row) * DHEAD + d] = ot;
        if (d == 0) {
            ml_part[(part_row0 + row) * 2 + 0] = mt;
            ml_part[(part_row0 + row) * 2 + 1] = lt;
        }
    }
}

// Combine the split partials of one (token, q-head): a row whose causal limit
// lies before a split's first key has l == 0 there and is ignored, as in the
// decode combine. m is in the exp2 domain.
__global__ __launch_bounds__(128) void append_combine_kernel(
    const float* __restrict__ o_part, const float* __restrict__ ml_part,
    const int* __restrict__ cu_q, uint16_t* __restrict__ out, int B, int Hk,
    int gshift, int nsplit, int rmax) {
    const int Hq = Hk << gshift;
    const int tok = blockIdx.x / Hq;
    const int qh = blockIdx.x % Hq;
    const int d = threadIdx.x;
    int b = 0;
    while (b + 1 < B && cu_q[b + 1] <= tok) ++b;
    const int j = tok - cu_q[b];
    const int h = qh >> gshift;
    const int row = (j << gshift) + (qh & ((1 << gshift) - 1));
    if (j < 0 || row >= rmax) return;
    const size_t base = ((size_t)(b * Hk + h) * nsplit) * rmax + row;
    float mt = -INFINITY;
    for (int s = 0; s < nsplit; ++s) {
        const float2 ml = *reinterpret_cast<const float2*>(
            ml_part + (base + (size_t)s * rmax) * 2);
        if (ml.y > 0.0f) mt = fmaxf(mt, ml.x);
    }
    float lt = 0.0f, ot = 0.0f;
    for (int s = 0; s < nsplit; ++s) {
        const float2 ml = *reinterpret_cast<const float2*>(
            ml_part + (base + (size_t)s * rmax) * 2);
        if (ml.y > 0.0f) {
            const float sc = __builtin_amdgcn_exp2f(ml.x - mt);
            lt += ml.y * sc;
            ot += o_part[(base + (size_t)s * rmax) * DHEAD + d] * sc;
        }
    }
    const float res = (lt > 0.0f) ? ot / lt : 0.0f;
    out[((size_t)tok * Hq + qh) * DHEAD + d] = f32_to_bf16(res);
}

// Largest L the kernel serves at group size G (0: unsupported G).
extern "C" int oa_attention_append_max_q(int G) {
    return (G == 1 || G == 2 || G == 4 || G == 8) ? APPEND_MAX_Q : 0;
}

// One launcher for both cache formats; the bf16 entry passes no scales.
static int append_launch(void* stream, const void* q, const void* kc,
                         const void* vc, const void* kscl, const void* vscl,
                         const void* block_table, const void* seq_lens,
                         const void* cu_q, void* o_part, void* ml_part, void* out,
                         int B, int T, int Hq, int Hk, int D, int max_blocks,
                         int block_size, int nsplit, float scale, int q_stride,
                         int max_q, bool fp8) {
    if (q_stride % 8 != 0) return -103;
    if (D != DHEAD) return -100;
    if ((block_size & (block_size - 1)) != 0) return -101;
    if (Hk <= 0 || Hq % Hk != 0) return -102;
    const int G = Hq / Hk;
    if (oa_attention_append_max_q(G) == 0) return -102;
    if (max_q < 1 || max_q > oa_attention_append_max_q(G)) return -104;
    if (B < 1 || T < B || nsplit < 1 || max_blocks < 1) return -105;
    int block_shift = 0;
    while ((1 << block_shift) < block_size) ++block_shift;
    int gshift = 0;
    while ((1 << gshift) < G) ++gshift;
    const int rmax = max_q * G;
    const float scale2 = scale * 1.4426950408889634f;
    dim3 grid(B * Hk, nsplit), block(256);
#define LAUNCH_A(NRTV, SB, F8)                                                  \
    hipLaunchKernelGGL((append_attn_kernel<NRTV, SB, F8>), grid, block, 0,      \
                       (hipStream_t)stream, (const uint16_t*)q, kc, vc,         \
                       (const float*)kscl, (const float*)vscl,                  \
                       (const int*)block_table, (const int*)seq_lens,           \
                       (const int*)cu_q, (float*)o_part, (float*)ml_part, Hk,   \
                       gshift, max_blocks, block_shift, nsplit, scale2,         \
                       q_stride, rmax)
#define LAUNCH_F(NRTV, SB)                                                      \
    do {                                                                        \
        if (fp8) LAUNCH_A(NRTV, SB, true); else LAUNCH_A(NRTV, SB, false);      \
    } while (0)
    const bool smallbs = block_size < 16;  // per-lane block-table loads
    if (rmax <= 16) {
        if (smallbs) LAUNCH_F(1, true); else LAUNCH_F(1, false);
    } else {
        if (smallbs) LAUNCH_F(2, true); else LAUNCH_F(2, false);
    }
#undef LAUNCH_F
#undef LAUNCH_A
    HIP_CHECK_LAUNCH();
    hipLaunchKernelGGL(append_combine_kernel, dim3(T * Hq), dim3(128), 0,
                       (hipStream_t)stream, (const float*)o_part,
                       (const float*)ml_part, (const int*)cu_q, (uint16_t*)out,
                       B, Hk, gshift, nsplit, rmax);
    HIP_CHECK_LAUNCH();
    return 0;
}

extern "C" int oa_attention_append(void* stream, const void* q, const void* kc,
                                   const void* vc, const void* block_table,
                                   const void* seq_lens, const void* cu_q,
                                   void* o_part, void* ml_part, void* out, int B,
                                   int T, int Hq, int Hk, int D, int max_blocks,
                                   int block_size, int nsplit, float scale,
                                   int q_stride, int max_q) {
    return append_launch(stream, q, kc, vc, nullptr, nullptr, block_table,
                         seq_lens, cu_q, o_part, ml_part, out, B, T, Hq, Hk, D,
                         max_blocks, block_size, nsplit, scale, q_stride, max_q,
                         false);
}

// The same kernel over the fp8 paged cache: kc/vc are e4m3 codes uint8
// [blocks, block_size, Hk, 128], k_scale/v_scale f32 [blocks, block_size, Hk].
extern "C" int oa_attention_append_fp8(
    void* stream, const void* q, const void* kc, const void* vc,
    const void* k_scale, const void* v_scale, const void* block_table,
    const void* seq_lens, const void* cu_q, void* o_part, void* ml_part,
    void* out, int B, int T, int Hq, int Hk, int D, int max_blocks,
    int block_size, int nsplit, float scale, int q_stride, int max_q) {
    return append_launch(stream, q, kc, vc, k_scale, v_scale, block_table,
                         seq_lens, cu_q, o_part, ml_part, out, B, T, Hq, Hk, D,
                         max_blocks, block_size, nsplit, scale, q_stride, max_q,
                         true);
}
