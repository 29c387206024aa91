// Paged decode attention for MI355X (gfx950) — SURVEY.md §2b "Decode (paged
// KV) attention kernel".
//
// Single new token per sequence attends to the whole paged KV cache. The op
// is HBM-bound (reads n_tokens * 2 * Hk * D * 2 bytes); the design follows
// the CDNA guide Appendix B "Attention decode": vectorized bf16 KV loads
// (16 B/lane), shuffle-reduce dot products, online softmax in registers, and
// sequence-split ("split-K over keys") so the grid covers the chip even at
// batch 1 (B*Hk workgroups alone would leave 256 CUs mostly idle).
//
// Layouts:
//   q        [B, Hq, 128] bf16
//   kc/vc    flat [num_slots, Hk, 128] bf16 (slot = block_id*block_size + off)
//   block_table [B, max_blocks] int32
//   seq_lens [B] int32 (tokens in cache, incl. the current token)
//   o_part   [B*Hk*NSPLIT, G, 128] f32, ml_part [B*Hk*NSPLIT, G, 2] f32
//   out      [B, Hq, 128] bf16
//
// Wave layout: 16 lanes per key row (16 x 8 dims = 128), 4 keys in flight per
// wave, 4 waves per workgroup each owning a quarter of the split's key range.

#include "common.h"

#define DHEAD 128
// o_part loads every combine / reducer task keeps in flight
#define RED_U 8

// The split reduction of one (b, h), run by the LAST split block of a FUSED
// launch (256 threads). It reproduces decode_combine_kernel's arithmetic
// exactly — split s belongs to group s & 3; within a group the max over the
// live splits, then lt / ot accumulated in ascending s; the four groups merged
// in order 1, 2, 3 with the online formula; the same divide and bf16 rounding
// — so the output is bit-identical to the two-kernel path. Both spell their
// multiply-adds as explicit fmas, in the form the stand-alone combine has
// always compiled to (x += a * b is fma(a, b, x); the merge x * a1 + y * a2 is
// fma(x, a1, y * a2)): left to the compiler, which product of the merge is
// fused depends on how it vectorises the surrounding code, and the two
// kernels would differ in the last bit.
// A task is (gh, group, 4 consecutive dims): 16-B o_part loads, issued
// unconditionally (a split index past the end is clamped and its value
// dropped by a select, never a branch) and at least RED_U per lane in flight, beside
// the (m, l) table's trip to LDS. An empty split's slab (l == 0) may hold
// anything, NaN included: `live` selects it away.
// sml: dynamic LDS [nsplit][G][2]; red_o / red_ml: the block's static LDS,
// free once the partials are published.
template <int G>
__device__ __forceinline__ void decode_reduce_splits(
    const float* __restrict__ o_part, const float* __restrict__ ml_part,
    uint32_t* __restrict__ out, int bh, int b, int h, int Hk, int nsplit,
    float* sml, float (&red_o)[4][G][DHEAD], float (&red_ml)[4][G][2]) {
    constexpr int NT = (G * 128 + 255) / 256;  // tasks per thread
    // loads in flight per task: NT * U >= 8 per lane, capped for registers
    constexpr int U = NT > 2 ? RED_U / 2 : RED_U;
    const int base = bh * nsplit;
    const int d4 = threadIdx.x & 31;
    const int sh = (threadIdx.x >> 5) & 3;
    const int gh0 = threadIdx.x >> 7;  // task i serves head gh0 + 2 * i

    float4 v[NT][U];
    auto load_chunk = [&](int c0) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < NT; ++i) {
            const int gh = min(gh0 + 2 * i, G - 1);
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int s = min(c0 + sh + 4 * u, nsplit - 1);
                v[i][u] = *reinterpret_cast<const float4*>(
                    o_part + ((size_t)(base + s) * G + gh) * DHEAD + d4 * 4);
            }
        }
    };
    load_chunk(0);
    for (int i = threadIdx.x; i < nsplit * G; i += blockDim.x) {
        const float2 ml =
            *reinterpret_cast<const float2*>(ml_part + ((size_t)base * G + i) * 2);
        sml[i * 2] = ml.x;
        sml[i * 2 + 1] = ml.y;
    }
    __syncthreads();

    float mt[NT], lt[NT], ot[NT][4];
#pragma unroll
    for (int i = 0; i < NT; ++i) {
        const int gh = min(gh0 + 2 * i, G - 1);
        mt[i] = -INFINITY;
        for (int s = sh; s < nsplit; s += 4)
            if (sml[(s * G + gh) * 2 + 1] > 0.0f) mt[i] = fmaxf(mt[i], sml[(s * G + gh) * 2]);
        lt[i] = 0.0f;
#pragma unroll
        for (int j = 0; j < 4; ++j) ot[i][j] = 0.0f;
    }
    for (int c0 = 0; c0 < nsplit; c0 += 4 * U) {
        if (c0 > 0) load_chunk(c0);
#pragma unroll
        for (int i = 0; i < NT; ++i) {
            const int gh = min(gh0 + 2 * i, G - 1);
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int s = c0 + sh + 4 * u;
                const int sc_ = min(s, nsplit - 1);
                const float lw = sml[(sc_ * G + gh) * 2 + 1];
                const bool live = (s < nsplit) && (lw > 0.0f);
                const float sc = __expf(sml[(sc_ * G + gh) * 2] - mt[i]);
                lt[i] = live ? __fmaf_rn(lw, sc, lt[i]) : lt[i];
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    ot[i][j] = live ? __fmaf_rn((&v[i][u].x)[j], sc, ot[i][j]) : ot[i][j];
            }
        }
    }
#pragma unroll
    for (int i = 0; i < NT; ++i) {
        const int gh = gh0 + 2 * i;
        if (gh < G) {
#pragma unroll
            for (int j = 0; j < 4; ++j) red_o[sh][gh][d4 * 4 + j] = ot[i][j];
            if (d4 == 0) {
                red_ml[sh][gh][0] = mt[i];
                red_ml[sh][gh][1] = lt[i];
            }
        }
    }
    __syncthreads();
    if (sh != 0) return;
    const int Hq = Hk * G;
#pragma unroll
    for (int i = 0; i < NT; ++i) {
        const int gh = gh0 + 2 * i;
        if (gh >= G) continue;
        float res[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float mj = mt[i], lj = lt[i], oj = ot[i][j];
#pragma unroll
            for (int g2 = 1; g2 < 4; ++g2) {
                const float m2 = red_ml[g2][gh][0], l2 = red_ml[g2][gh][1];
                const float o2 = red_o[g2][gh][d4 * 4 + j];
                const float mn = fmaxf(mj, m2);
                const float a1 = (lj > 0.0f) ? __expf(mj - mn) : 0.0f;
                const float a2 = (l2 > 0.0f) ? __expf(m2 - mn) : 0.0f;
                oj = __fmaf_rn(oj, a1, o2 * a2);
                lj = __fmaf_rn(lj, a1, l2 * a2);
                mj = (lj > 0.0f) ? mn : -INFINITY;
            }
            res[j] = (lj > 0.0f) ? oj / lj : 0.0f;
        }
        uint2 w;
        w.x = pack_bf16x2(res[0], res[1]);
        w.y = pack_bf16x2(res[2], res[3]);
        *reinterpret_cast<uint2*>(
            out + ((size_t)(b * Hq + h * G + gh) * DHEAD + d4 * 4) / 2) = w;
    }
}

// FUSED = true folds the split-combine into this launch with the CDNA guide's
// in-launch split-K hand-off (plain-store form): each split block publishes
// its partial with an agent-scope release and draws a ticket from cnt[b, h];
// the block that draws nsplit-1 acquires and runs decode_reduce_splits —
// saving the second kernel launch per layer. No block ever waits on another:
// there is no poll and no spin. The reducer re-arms its ticket word (stores
// 0) before it exits, so `cnt` needs zeroing only once, where it is
// allocated: launches that share one workspace (the layers of a step, the
// replays of a graph) are ordered by the stream, and a launch ends with every
// word it touched back at zero. FUSED launches take nsplit * G * 8 bytes of
// dynamic LDS for the reducer's (m, l) table.
// ROPE = true additionally fuses the per-token RoPE + paged-KV scatter that
// the separate rope_kv kernel did (4.7 us/layer of pure launch latency at
// decode): every block ropes its G q heads IN REGISTERS (rotate-half partner
// dims live in lane dl^8 — one __shfl_xor), the main loop covers only the
// CACHED keys [0, n-1), and the split that owns key n-1 ropes the new k from
// the raw GEMV output, scatters roped-k and v to the cache slot, and folds
// the new key into its online softmax. kin/vin/cs/sn/slots/kcw/vcw are only
// read when ROPE.
//
// Load order. At small batch the kernel is a chain of dependent memory round
// trips and nothing else, so the chain is kept as short as the data allows:
//   1. at the top, everything that depends only on (b, h, split): seq_lens[b]
//      and slots[b] (scalar), the raw q words, and on wave 3 (the wave that
//      folds the new key in) the kin / vin rows;
//   2. once n is known: the cos/sin row and the block-table entries of the
//      wave's key range — by SCALAR loads when block_size >= 16 (a key quad
//      then touches at most two blocks, both at wave-uniform addresses), per
//      lane otherwise;
//   3. in the 4-deep form, the first K/V burst (every ring slot the loop
//      does not issue itself) BEFORE any math on q: the bf16 -> f32 unpack and
//      the rope of q run under the K/V latency. (As compiled, two of the
//      burst's three quads stay there; the third, used only inside the loop,
//      is sunk to the loop's preheader — profiles/README.md, v10.)
// Every K/V load is unconditional: a key index at or past the wave's end is
// clamped to the wave's last key (the duplicate hits the cache), a wave with
// no key reads slot 0, and `valid` gates only the math, exactly as before. A
// load under `if (valid)`, or behind a per-lane table load on the same
// counter, proves nothing to the compiler about issue order: its waits become
// vmcnt(0) and every wait drains the ring.
// The ARITHMETIC — the rope of q and of the new key, the key loop's four
// process() copies and their order, the wave and block merges — is the text
// and the structure it has always been, on purpose: which product of a
// x * a + y * b the compiler fuses follows its vectorisation of that text, so
// moving the math moves last bits. Only loads moved, and the empty asm
// statements below exist to keep two branches branches. Nothing pins the
// compiler's choice, so a compiler update or an edit nearby can move last
// bits: tests/test_decode_fused_gpu.py holds the two-kernel output to a
// re-computation from the kernel's own partials and the fused forms to the
// two-kernel one, tests/test_attention_edges_gpu.py holds the result to the
// fp64 oracle, and `bench.py --dump-outputs` against the parent commit is
// the check that the partials themselves did not move.
template <int G, bool FUSED, bool ROPE, bool DEEP = true>
__global__ __launch_bounds__(256) void decode_attn_kernel(
    const uint32_t* __restrict__ q, const uint32_t* __restrict__ kc,
    const uint32_t* __restrict__ vc, const int* __restrict__ block_table,
    const int* __restrict__ seq_lens, float* __restrict__ o_part,
    float* __restrict__ ml_part, unsigned* __restrict__ cnt,
    uint32_t* __restrict__ out, int B, int Hk, int max_blocks,
    int block_shift /* log2(block_size) */, int nsplit, float scale,
    int qs2 /* q batch-row stride in words */,
    const uint32_t* __restrict__ kin, const uint32_t* __restrict__ vin,
    const float* __restrict__ cs, const float* __restrict__ sn,
    const int* __restrict__ slots, uint32_t* __restrict__ kcw,
    uint32_t* __restrict__ vcw, int ks2, int vs2) {
    const int bh = blockIdx.x;
    const int b = bh / Hk;
    const int h = bh % Hk;
    const int split = blockIdx.y;

    const int lane = threadIdx.x & (WAVE - 1);
    // wave-uniform on purpose (an SGPR): the wave's key range, and with it the
    // block-table addresses below, must be scalar
    const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x / WAVE);
    const int g16 = lane >> 4;   // key slot within the wave's 4-key window
    const int dl = lane & 15;    // owns dims dl*8 .. dl*8+7

    // ---- 1. loads that need nothing but (b, h, split) ----------------------
    const int n = seq_lens[b];
    int new_slot = 0;
    if (ROPE) new_slot = slots[b];
    // q fragments: [G] x 8 bf16 per lane (all lane groups redundant)
    uint4 qw[G];
#pragma unroll
    for (int gh = 0; gh < G; ++gh)
        qw[gh] = *reinterpret_cast<const uint4*>(
            q + (size_t)b * qs2 + ((size_t)(h * G + gh) * DHEAD + dl * 8) / 2);
    // the new key's raw k / v rows: wave 3 folds it in, in whichever split
    // owns key n-1 — not known yet, and not worth waiting for
    // (4-deep form only: two live rows across the loop cost the 2-deep forms
    // a resident wave, so they load them where they use them)
    constexpr bool DEEP4 = G <= 4 && DEEP;
    uint4 knw{}, vnw{};
    if (ROPE && DEEP4 && wid == 3) {
        knw = *reinterpret_cast<const uint4*>(
            kin + (size_t)b * ks2 + ((size_t)h * DHEAD + dl * 8) / 2);
        vnw = *reinterpret_cast<const uint4*>(
            vin + (size_t)b * vs2 + ((size_t)h * DHEAD + dl * 8) / 2);
    }

    const int chunk = CEIL_DIV(n, nsplit);
    const int kstart = split * chunk;
    const int kend = min(n, kstart + chunk);
    // ROPE: the new key (index n-1) is handled from registers, not cache
    const int n_cached = ROPE ? (n - 1) : n;
    const int kend_c = min(kend, n_cached);

    const int part_idx = (bh * nsplit + split);
    float* opart_row = o_part + ((size_t)part_idx * G) * DHEAD;
    float* mlpart_row = ml_part + ((size_t)part_idx * G) * 2;

    // per-wave sub-range (over CACHED keys only)
    const int span = kend_c - kstart;
    const int wchunk = CEIL_DIV(max(span, 0), 4);
    const int wstart = kstart + wid * wchunk;
    const int wend = min(kend_c, wstart + wchunk);
    const bool has_keys = wstart < wend;  // wave-uniform

    // ---- 2. loads that need n ----------------------------------------------
    // ROPE: the cos/sin row of position n-1. Lane dl owns dims dl*8..dl*8+7;
    // the partner half (d +/- 64) lives in lane dl^8 of the same 16-lane group.
    float c8[8], s8[8];
    if (ROPE) {
        const int pos = max(n - 1, 0);
        const float* crow = cs + (size_t)pos * (DHEAD / 2) + (dl & 7) * 8;
        const float* srow = sn + (size_t)pos * (DHEAD / 2) + (dl & 7) * 8;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            c8[j] = crow[j];
            s8[j] = srow[j];
        }
    }

    const int bmask = (1 << block_shift) - 1;
    const int* btrow = block_table + (size_t)b * max_blocks;
    // A wave without a key reads slot 0, whatever the table holds: `keep`
    // masks its table entry and key offset to zero. It passes through
    // readfirstlane (it is wave-uniform anyway) so that the compiler cannot
    // turn the mask into a branch around the table loads — they are to stay
    // unconditional.
    const int keep = __builtin_amdgcn_readfirstlane(has_keys ? -1 : 0);
    const int last = max(wend - 1, 0);
    const bool sbt = block_shift >= 4;  // table entries by scalar loads

    // The K and V rows of key quad kk0. sbt: the quad's keys lie in the block
    // of its first key or in the one after it, both at wave-uniform table
    // addresses. Otherwise the entry is loaded per lane, and waited for
    // inside its branch (the empty asm), so that the scalar form never meets
    // that load on its wait counter.
    auto issue_loads = [&](int kk0, uint4& kw, uint4& vw, bool& valid)
                           __attribute__((always_inline)) {
        valid = kk0 + g16 < wend;
        const int kk = min(kk0 + g16, last);
        int bte;
        if (sbt) {
            const int blk0 = min(kk0, last) >> block_shift;
            const int bt0 = btrow[blk0];
            const int bt1 = btrow[min(kk0 + 3, last) >> block_shift];
            bte = (kk >> block_shift) == blk0 ? bt0 : bt1;
        } else {
            bte = btrow[kk >> block_shift];
            asm volatile("" : "+v"(bte));
        }
        const int64_t slot = (int64_t)(bte & keep) << block_shift | (kk & bmask & keep);
        kw = *reinterpret_cast<const uint4*>(
            kc + ((size_t)slot * Hk + h) * (DHEAD / 2) + dl * 4);
        vw = *reinterpret_cast<const uint4*>(
            vc + ((size_t)slot * Hk + h) * (DHEAD / 2) + dl * 4);
    };

    // ---- 3. first K/V burst ------------------------------------------------
    // The 4-deep form (B <= 4, latency-bound) issues it before any math on q.
    // The 2-deep forms (B > 4, occupancy-bound; G = 8, at the register limit)
    // unpack and rope q first: holding the raw q words across the first load
    // costs them a resident wave per SIMD.
    uint4 kA{}, vA4{}, kB{}, vB4{}, kC{}, vC4{}, kD{}, vD4{};
    bool va = false, vb = false, vc2 = false, vd = false;
    if (DEEP4) {
        issue_loads(wstart, kA, vA4, va);
        issue_loads(wstart + 4, kB, vB4, vb);
        issue_loads(wstart + 8, kC, vC4, vc2);
    }

    // load q fragments: [G][8] floats per lane
    float qreg[G][8];
#pragma unroll
    for (int gh = 0; gh < G; ++gh) {
        const uint4 w = qw[gh];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            qreg[gh][j * 2] = bf16_lo((&w.x)[j]);
            qreg[gh][j * 2 + 1] = bf16_hi((&w.x)[j]);
        }
    }

    // ROPE: rotate-half q in registers
    if (ROPE) {
#pragma unroll
        for (int gh = 0; gh < G; ++gh) {
            float part[8];
#pragma unroll
            for (int j = 0; j < 8; ++j)
                part[j] = __shfl_xor(qreg[gh][j], 8, WAVE);
#pragma unroll
            for (int j = 0; j < 8; ++j)
                qreg[gh][j] = (dl < 8)
                                  ? qreg[gh][j] * c8[j] - part[j] * s8[j]
                                  : qreg[gh][j] * c8[j] + part[j] * s8[j];
        }
    }

    if (!DEEP4) issue_loads(wstart, kA, vA4, va);

    float m[G], lsum[G], o[G][8];
#pragma unroll
    for (int gh = 0; gh < G; ++gh) {
        m[gh] = -INFINITY;
        lsum[gh] = 0.0f;
#pragma unroll
        for (int j = 0; j < 8; ++j) o[gh][j] = 0.0f;
    }

    auto process = [&](const uint4& kw, const uint4& vw, bool valid) {
        float kv_k[8], kv_v[8];
        if (valid) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                kv_k[j * 2] = bf16_lo((&kw.x)[j]);
                kv_k[j * 2 + 1] = bf16_hi((&kw.x)[j]);
                kv_v[j * 2] = bf16_lo((&vw.x)[j]);
                kv_v[j * 2 + 1] = bf16_hi((&vw.x)[j]);
            }
        }
#pragma unroll
        for (int gh = 0; gh < G; ++gh) {
            float s = 0.0f;
            if (valid) {
#pragma unroll
                for (int j = 0; j < 8; ++j) s += qreg[gh][j] * kv_k[j];
            }
            s = group16_reduce_sum(s);  // all 16 lanes of the group get the dot
            if (valid) {
                s *= scale;
                const float mn = fmaxf(m[gh], s);
                const float alpha = __expf(m[gh] - mn);
                const float p = __expf(s - mn);
#pragma unroll
                for (int j = 0; j < 8; ++j) o[gh][j] = o[gh][j] * alpha + p * kv_v[j];
                lsum[gh] = lsum[gh] * alpha + p;
                m[gh] = mn;
            }
        }
    };
    {
        // 4-deep key-quad pipeline (modulo-scheduled with NAMED slots —
        // a runtime-indexed ring would go to scratch, guide rule 20):
        // 2-deep left most of the ~900-cycle HBM latency exposed at small
        // batch, where one quad is only 32 B/lane in flight. DEEP is
        // dispatched for B<=4 only: the extra slots cost VGPRs — right when
        // latency-bound, an occupancy tax once a big batch saturates HBM.
        // G8 keeps depth 2 (qreg+o already hold 128 VGPRs).
        if (DEEP4) {
            for (int kk0 = wstart; kk0 < wend; kk0 += 16) {
                issue_loads(kk0 + 12, kD, vD4, vd);
                process(kA, vA4, va);
                issue_loads(kk0 + 16, kA, vA4, va);
                process(kB, vB4, vb);
                issue_loads(kk0 + 20, kB, vB4, vb);
                process(kC, vC4, vc2);
                issue_loads(kk0 + 24, kC, vC4, vc2);
                process(kD, vD4, vd);
            }
        } else {
            for (int kk0 = wstart; kk0 < wend; kk0 += 4) {
                issue_loads(kk0 + 4, kB, vB4, vb);
                process(kA, vA4, va);
                kA = kB; vA4 = vB4; va = vb;
            }
        }
    }

    // ROPE: the owning split ropes the NEW key from the raw GEMV output,
    // scatters roped-k and v to the cache slot, and folds it into wave 3's
    // online softmax (the cross-wave LDS merge below absorbs it).
    if (ROPE) {
        const int pos = n - 1;
        if (pos >= kstart && pos < kend && wid == 3) {
            const bool nv = (g16 == 0);
            uint4 kw{}, vw{};
            if (nv) {
                if (DEEP4) {
                    // the rows came in at the top of the kernel; the empty asm
                    // keeps this a branch, as the load it replaces was
                    kw = knw;
                    vw = vnw;
                    asm volatile("" : "+v"(kw.x), "+v"(kw.y), "+v"(kw.z), "+v"(kw.w));
                    asm volatile("" : "+v"(vw.x), "+v"(vw.y), "+v"(vw.z), "+v"(vw.w));
                } else {
                    kw = *reinterpret_cast<const uint4*>(
                        kin + (size_t)b * ks2 + ((size_t)h * DHEAD + dl * 8) / 2);
                    vw = *reinterpret_cast<const uint4*>(
                        vin + (size_t)b * vs2 + ((size_t)h * DHEAD + dl * 8) / 2);
                }
            }
            float kf[8], vf[8];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                kf[j * 2] = bf16_lo((&kw.x)[j]);
                kf[j * 2 + 1] = bf16_hi((&kw.x)[j]);
                vf[j * 2] = bf16_lo((&vw.x)[j]);
                vf[j * 2 + 1] = bf16_hi((&vw.x)[j]);
            }
            float kp[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) kp[j] = __shfl_xor(kf[j], 8, WAVE);
            float kr[8];
#pragma unroll
            for (int j = 0; j < 8; ++j)
                kr[j] = (dl < 8) ? kf[j] * c8[j] - kp[j] * s8[j]
                                 : kf[j] * c8[j] + kp[j] * s8[j];
            if (nv) {
                const int64_t slot = new_slot;
                uint4 kout;
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    (&kout.x)[j] = pack_bf16x2(kr[j * 2], kr[j * 2 + 1]);
                *reinterpret_cast<uint4*>(
                    kcw + ((size_t)slot * Hk + h) * (DHEAD / 2) + dl * 4) = kout;
                *reinterpret_cast<uint4*>(
                    vcw + ((size_t)slot * Hk + h) * (DHEAD / 2) + dl * 4) = vw;
            }
#pragma unroll
            for (int gh = 0; gh < G; ++gh) {
                float s = 0.0f;
                if (nv) {
#pragma unroll
                    for (int j = 0; j < 8; ++j) s += qreg[gh][j] * kr[j];
                }
                s = group16_reduce_sum(s);
                if (nv) {
                    s *= scale;
                    const float mn = fmaxf(m[gh], s);
                    const float alpha = __expf(m[gh] - mn);
                    const float p = __expf(s - mn);
#pragma unroll
                    for (int j = 0; j < 8; ++j)
                        o[gh][j] = o[gh][j] * alpha + p * vf[j];
                    lsum[gh] = lsum[gh] * alpha + p;
                    m[gh] = mn;
                }
            }
        }
    }

    // merge the wave's 4 key-groups (lanes l, l^16, l^32 hold same dims)
#pragma unroll
    for (int off = 16; off <= 32; off <<= 1) {
#pragma unroll
        for (int gh = 0; gh < G; ++gh) {
            const float m2 = __shfl_xor(m[gh], off, WAVE);
            const float l2 = __shfl_xor(lsum[gh], off, WAVE);
            float o2[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) o2[j] = __shfl_xor(o[gh][j], off, WAVE);
            const float mn = fmaxf(m[gh], m2);
            // guard: empty partial (l == 0, m == -inf) must not produce NaN
            const float a1 = (lsum[gh] > 0.0f) ? __expf(m[gh] - mn) : 0.0f;
            const float a2 = (l2 > 0.0f) ? __expf(m2 - mn) : 0.0f;
#pragma unroll
            for (int j = 0; j < 8; ++j) o[gh][j] = o[gh][j] * a1 + o2[j] * a2;
            lsum[gh] = lsum[gh] * a1 + l2 * a2;
            m[gh] = (lsum[gh] > 0.0f) ? mn : -INFINITY;
        }
    }

    // cross-wave combine through LDS
    __shared__ float lds_o[4][G][DHEAD];
    __shared__ float lds_ml[4][G][2];
    if (lane < 16) {
#pragma unroll
        for (int gh = 0; gh < G; ++gh) {
#pragma unroll
            for (int j = 0; j < 8; ++j) lds_o[wid][gh][dl * 8 + j] = o[gh][j];
            if (dl == 0) {
                lds_ml[wid][gh][0] = m[gh];
                lds_ml[wid][gh][1] = lsum[gh];
            }
        }
    }
    __syncthreads();

    // 256 threads cover G*128 outputs
    for (int idx = threadIdx.x; idx < G * DHEAD; idx += blockDim.x) {
        const int gh = idx / DHEAD;
        const int d = idx % DHEAD;
        float mt = -INFINITY;
#pragma unroll
        for (int w = 0; w < 4; ++w)
            if (lds_ml[w][gh][1] > 0.0f) mt = fmaxf(mt, lds_ml[w][gh][0]);
        float lt = 0.0f, ot = 0.0f;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const float lw = lds_ml[w][gh][1];
            if (lw > 0.0f) {
                const float sc = __expf(lds_ml[w][gh][0] - mt);
                lt += lw * sc;
                ot += lds_o[w][gh][d] * sc;
            }
        }
        opart_row[gh * DHEAD + d] = ot;
        if (d == 0) {
            mlpart_row[gh * 2 + 0] = mt;
            mlpart_row[gh * 2 + 1] = lt;
        }
    }

    if (!FUSED) return;

    // ---- publish + reducer election (plain-store recipe) -------------------
    // every wave drains its slab stores, then one lane releases and takes a
    // ticket; the block that draws nsplit-1 becomes the reducer
    __shared__ int s_last;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // EVERY wave
    __syncthreads();
    if (threadIdx.x == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        // restate the post-wbl2 wait the compiler may drop (guide pitfall 12)
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const unsigned prev = __hip_atomic_fetch_add(
            &cnt[bh], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const int last = (prev == (unsigned)(nsplit - 1));
        // re-arm: every ticket of this launch is drawn, and the next launch
        // on this word is behind this one on the stream
        if (last)
            __hip_atomic_store(&cnt[bh], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        s_last = last;
    }
    __syncthreads();
    if (!s_last) return;
    if (threadIdx.x == 0) {
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");  // drop stale L1
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __syncthreads();

    extern __shared__ __attribute__((aligned(16))) float red_sml[];  // [nsplit][G][2]
    decode_reduce_splits<G>(o_part, ml_part, out, bh, b, h, Hk, nsplit, red_sml,
                            lds_o, lds_ml);
}

// Combine split partials -> final output. Grid: B*Hq blocks, 512 threads:
// thread (d = tid & 127, sh = tid >> 7) accumulates splits sh, sh+4, ... so
// the split loop runs nsplit/4 iterations with 4-way ILP, then the 4 partial
// (m, l, o_d) triples merge through LDS. The (m, l) table is staged into LDS
// once by the first wave (the naive one-thread-one-d loop over 64 splits was
// 32 us/launch — 3x the attention kernel itself). The o_part loads go out
// first, RED_U per thread and unconditional (a split index past the end is
// clamped), beside the table's loads and not behind its barrier; `l > 0` is
// a select on the math, so an empty split's slab cannot leak.
template <int G>
__global__ __launch_bounds__(512) void decode_combine_kernel(
    const float* __restrict__ o_part, const float* __restrict__ ml_part,
    uint32_t* __restrict__ out, int B, int Hk, int nsplit) {
    const int bq = blockIdx.x;
    const int Hq = Hk * G;
    const int b = bq / Hq;
    const int qh = bq % Hq;
    const int h = qh / G;
    const int gh = qh % G;
    const int d = threadIdx.x & (DHEAD - 1);
    const int sh = threadIdx.x >> 7;  // 0..3

    extern __shared__ __attribute__((aligned(16))) float sml[];  // [nsplit][2]
    const int base = (b * Hk + h) * nsplit;
    float v[RED_U];
    auto load_chunk = [&](int c0) __attribute__((always_inline)) {
#pragma unroll
        for (int u = 0; u < RED_U; ++u) {
            const int s = min(c0 + sh + 4 * u, nsplit - 1);
            v[u] = o_part[((size_t)(base + s) * G + gh) * DHEAD + d];
        }
    };
    load_chunk(0);
    for (int s = threadIdx.x; s < nsplit; s += blockDim.x) {
        const float2 ml = *reinterpret_cast<const float2*>(
            ml_part + ((size_t)(base + s) * G + gh) * 2);
        sml[s * 2] = ml.x;
        sml[s * 2 + 1] = ml.y;
    }
    __syncthreads();

    float mt = -INFINITY;
    for (int s = sh; s < nsplit; s += 4)
        if (sml[s * 2 + 1] > 0.0f) mt = fmaxf(mt, sml[s * 2]);
    float lt = 0.0f, ot = 0.0f;
    for (int c0 = 0; c0 < nsplit; c0 += 4 * RED_U) {
        if (c0 > 0) load_chunk(c0);
#pragma unroll
        for (int u = 0; u < RED_U; ++u) {
            const int s = c0 + sh + 4 * u;
            const int sc_ = min(s, nsplit - 1);
            const float lw = sml[sc_ * 2 + 1];
            const bool live = (s < nsplit) && (lw > 0.0f);
            const float sc = __expf(sml[sc_ * 2] - mt);
            lt = live ? __fmaf_rn(lw, sc, lt) : lt;
            ot = live ? __fmaf_rn(v[u], sc, ot) : ot;
        }
    }
    // merge the 4 split-groups via LDS (per d): (m, l, o) online combine
    __shared__ float red_m[4][DHEAD], red_l[4][DHEAD], red_o[4][DHEAD];
    red_m[sh][d] = mt;
    red_l[sh][d] = lt;
    red_o[sh][d] = ot;
    __syncthreads();
    if (sh == 0) {
#pragma unroll
        for (int g2 = 1; g2 < 4; ++g2) {
            const float m2 = red_m[g2][d], l2 = red_l[g2][d], o2 = red_o[g2][d];
            const float mn = fmaxf(mt, m2);
            const float a1 = (lt > 0.0f) ? __expf(mt - mn) : 0.0f;
            const float a2 = (l2 > 0.0f) ? __expf(m2 - mn) : 0.0f;
            ot = __fmaf_rn(ot, a1, o2 * a2);
            lt = __fmaf_rn(lt, a1, l2 * a2);
            mt = (lt > 0.0f) ? mn : -INFINITY;
        }
        const float res = (lt > 0.0f) ? ot / lt : 0.0f;
        reinterpret_cast<uint16_t*>(out)[(size_t)(b * Hq + qh) * DHEAD + d] =
            f32_to_bf16(res);
    }
}

// ---- host side --------------------------------------------------------------
namespace {

struct DecodeArgs {
    hipStream_t stream;
    const void *q, *kc, *vc, *block_table, *seq_lens;
    void *o_part, *ml_part, *cnt, *out;
    int B, Hq, Hk, max_blocks, block_size, nsplit;
    float scale;
    int q_stride;
    // ROPE only
    const void *kin, *vin, *cos_t, *sin_t, *slots;
    int k_stride, v_stride;
};

template <int G>
int launch_combine(hipStream_t stream, const void* o_part, const void* ml_part,
                   void* out, int B, int Hk, int nsplit) {
    dim3 cgrid(B * Hk * G), cblock(512);
    const int clds = nsplit * 2 * (int)sizeof(float);
    hipLaunchKernelGGL((decode_combine_kernel<G>), cgrid, cblock, clds, stream,
                       (const float*)o_part, (const float*)ml_part, (uint32_t*)out,
                       B, Hk, nsplit);
    HIP_CHECK_LAUNCH();
    return 0;
}

// One attention launch (+ the stand-alone combine unless fused). DEEP (the
// 4-deep ring) is dispatched for B <= 4.
template <int G, bool ROPE>
int launch_decode(const DecodeArgs& a, bool fused) {
    int block_shift = 0;
    while ((1 << block_shift) < a.block_size) ++block_shift;
    dim3 grid(a.B * a.Hk, a.nsplit), block(256);
    const bool deep = a.B <= 4;
    // reducer's (m, l) table; the block's static LDS is at most 16.6 KB
    const int rlds = fused ? a.nsplit * G * 2 * (int)sizeof(float) : 0;
    if (rlds > 32768) return -105;
    auto k = fused ? (deep ? decode_attn_kernel<G, true, ROPE, true>
                           : decode_attn_kernel<G, true, ROPE, false>)
                   : (deep ? decode_attn_kernel<G, false, ROPE, true>
                           : decode_attn_kernel<G, false, ROPE, false>);
    hipLaunchKernelGGL(k, grid, block, rlds, a.stream, (const uint32_t*)a.q,
                       (const uint32_t*)a.kc, (const uint32_t*)a.vc,
                       (const int*)a.block_table, (const int*)a.seq_lens,
                       (float*)a.o_part, (float*)a.ml_part, (unsigned*)a.cnt,
                       (uint32_t*)a.out, a.B, a.Hk, a.max_blocks, block_shift,
                       a.nsplit, a.scale, a.q_stride / 2, (const uint32_t*)a.kin,
                       (const uint32_t*)a.vin, (const float*)a.cos_t,
                       (const float*)a.sin_t, (const int*)a.slots,
                       ROPE ? (uint32_t*)a.kc : (uint32_t*)nullptr,
                       ROPE ? (uint32_t*)a.vc : (uint32_t*)nullptr,
                       a.k_stride / 2, a.v_stride / 2);
    HIP_CHECK_LAUNCH();
    if (fused) return 0;
    return launch_combine<G>(a.stream, a.o_part, a.ml_part, a.out, a.B, a.Hk, a.nsplit);
}

template <bool ROPE>
int dispatch_decode(const DecodeArgs& a, int D, bool fused) {
    if (D != DHEAD) return -100;
    if ((a.block_size & (a.block_size - 1)) != 0) return -101;
    switch (a.Hq / a.Hk) {
        case 1: return launch_decode<1, ROPE>(a, fused);
        case 2: return launch_decode<2, ROPE>(a, fused);
        case 4: return launch_decode<4, ROPE>(a, fused);
        case 8: return launch_decode<8, ROPE>(a, fused);
        default: return -102;
    }
}

int decode_rope(void* stream, const void* q, const void* kin, const void* vin,
                void* kc, void* vc, const void* block_table, const void* seq_lens,
                const void* cos_t, const void* sin_t, const void* slots,
                void* o_part, void* ml_part, void* cnt_ws, void* out, int B, int Hq,
                int Hk, int D, int max_blocks, int block_size, int nsplit,
                float scale, int q_stride, int k_stride, int v_stride, bool fused) {
    if ((q_stride | k_stride | v_stride) % 8 != 0) return -103;
    DecodeArgs a{(hipStream_t)stream, q, kc, vc, block_table, seq_lens,
                 o_part, ml_part, cnt_ws, out,
                 B, Hq, Hk, max_blocks, block_size, nsplit, scale, q_stride,
                 kin, vin, cos_t, sin_t, slots, k_stride, v_stride};
    return dispatch_decode<true>(a, D, fused);
}

}  // namespace

// fused=1 folds the combine into the attention launch; this entry zeroes the
// ticket words itself on every call (a memset node under graph capture), so
// cnt_ws may hold anything. fused=0 is the two-kernel path.
extern "C" int oa_attention_decode(void* stream, const void* q, const void* kc,
                                   const void* vc, const void* block_table,
                                   const void* seq_lens, void* o_part,
                                   void* ml_part, void* cnt_ws, void* out, int B,
                                   int Hq, int Hk, int D, int max_blocks,
                                   int block_size, int nsplit, float scale,
                                   int q_stride, int fused) {
    if (q_stride % 8 != 0) return -103;
    if (fused) {
        hipError_t e = hipMemsetAsync(cnt_ws, 0, B * Hk * 4, (hipStream_t)stream);
        if (e != hipSuccess) return (int)e;
    }
    DecodeArgs a{(hipStream_t)stream, q, kc, vc, block_table, seq_lens,
                 o_part, ml_part, cnt_ws, out,
                 B, Hq, Hk, max_blocks, block_size, nsplit, scale, q_stride,
                 nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0};
    return dispatch_decode<false>(a, D, fused != 0);
}

// The combine alone, for kernels in other files that publish partials in the
// same (o_part, ml_part) layout — see decode_combine.h.
extern "C" int oa_decode_combine(void* stream, const void* o_part,
                                 const void* ml_part, void* out, int B, int Hq,
                                 int Hk, int nsplit) {
    hipStream_t st = (hipStream_t)stream;
    switch (Hq / Hk) {
        case 1: return launch_combine<1>(st, o_part, ml_part, out, B, Hk, nsplit);
        case 2: return launch_combine<2>(st, o_part, ml_part, out, B, Hk, nsplit);
        case 4: return launch_combine<4>(st, o_part, ml_part, out, B, Hk, nsplit);
        case 8: return launch_combine<8>(st, o_part, ml_part, out, B, Hk, nsplit);
        default: return -102;
    }
}

// Fully-fused decode attention: RoPE(q, k) + paged-KV scatter of (k, v) +
// split-K attention in ONE launch (+ the combine kernel) — replaces the
// separate rope_kv launch per layer. q/kin/vin are the RAW (un-roped) GEMV
// outputs; kc/vc are read for cached keys and written at slots[b].
extern "C" int oa_attention_decode_rope(
    void* stream, const void* q, const void* kin, const void* vin, void* kc,
    void* vc, const void* block_table, const void* seq_lens, const void* cos_t,
    const void* sin_t, const void* slots, void* o_part, void* ml_part,
    void* out, int B, int Hq, int Hk, int D, int max_blocks, int block_size,
    int nsplit, float scale, int q_stride, int k_stride, int v_stride) {
    return decode_rope(stream, q, kin, vin, kc, vc, block_table, seq_lens, cos_t,
                       sin_t, slots, o_part, ml_part, nullptr, out, B, Hq, Hk, D,
                       max_blocks, block_size, nsplit, scale, q_stride, k_stride,
                       v_stride, false);
}

// oa_attention_decode_rope with the combine folded into the launch: no
// combine kernel and no memset node. cnt_ws holds B*Hk ticket words that the
// CALLER zeroed once, when it allocated them; every launch leaves them zero.
extern "C" int oa_attention_decode_rope_fused(
    void* stream, const void* q, const void* kin, const void* vin, void* kc,
    void* vc, const void* block_table, const void* seq_lens, const void* cos_t,
    const void* sin_t, const void* slots, void* o_part, void* ml_part,
    void* cnt_ws, void* out, int B, int Hq, int Hk, int D, int max_blocks,
    int block_size, int nsplit, float scale, int q_stride, int k_stride,
    int v_stride) {
    if (cnt_ws == nullptr) return -106;
    return decode_rope(stream, q, kin, vin, kc, vc, block_table, seq_lens, cos_t,
                       sin_t, slots, o_part, ml_part, cnt_ws, out, B, Hq, Hk, D,
                       max_blocks, block_size, nsplit, scale, q_stride, k_stride,
                       v_stride, true);
}
