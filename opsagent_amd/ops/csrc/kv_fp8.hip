// fp8 paged KV cache for MI355X (gfx950): quantising write, gather-dequant
// and split-K paged decode attention.
//
// Format, per layer, for K and V each:
//   codes  uint8 [num_slots, Hk, 128]  OCP e4m3fn (slot = block*block_size+off)
//   scales f32   [num_slots, Hk]       one per (slot, kv-head) row
// Same convention as quant_fp8_kernel (fp8_moe.hip): scale = max(absmax,
// 1e-8) / 448, code = HW convert of x * (448 / absmax). A slot costs 132 B
// per head against 256 B for bf16.
//
// All three kernels map one 16-lane group to one 128-dim row, lane dl owning
// dims dl*8 .. dl*8+7 (8 code bytes = one 8-B load/store per lane).

#include "common.h"
#include "decode_combine.h"

#define DHEAD 128
#define FP8_MAX 448.0f

typedef __attribute__((ext_vector_type(2))) float f32x2;

// 8 e4m3 codes -> 4 float pairs, the form v_pk_fma_f32 / v_pk_mul_f32 take
__device__ __forceinline__ void fp8x8_to_f32x2(const uint2& w, f32x2* f) {
    f[0] = __builtin_amdgcn_cvt_pk_f32_fp8(w.x, false);
    f[1] = __builtin_amdgcn_cvt_pk_f32_fp8(w.x, true);
    f[2] = __builtin_amdgcn_cvt_pk_f32_fp8(w.y, false);
    f[3] = __builtin_amdgcn_cvt_pk_f32_fp8(w.y, true);
}

// 8 e4m3 codes (two words, element-linear bytes) -> 8 floats
__device__ __forceinline__ void fp8x8_to_f32(const uint2& w, float* f) {
    const f32x2 a = __builtin_amdgcn_cvt_pk_f32_fp8(w.x, false);
    const f32x2 b = __builtin_amdgcn_cvt_pk_f32_fp8(w.x, true);
    const f32x2 c = __builtin_amdgcn_cvt_pk_f32_fp8(w.y, false);
    const f32x2 d = __builtin_amdgcn_cvt_pk_f32_fp8(w.y, true);
    f[0] = a[0]; f[1] = a[1]; f[2] = b[0]; f[3] = b[1];
    f[4] = c[0]; f[5] = c[1]; f[6] = d[0]; f[7] = d[1];
}

// 8 floats (already multiplied by 448/absmax) -> 8 e4m3 codes
__device__ __forceinline__ uint2 f32x8_to_fp8(const float* f) {
    uint2 o;
    unsigned int p = 0;
    p = __builtin_amdgcn_cvt_pk_fp8_f32(f[0], f[1], p, false);
    p = __builtin_amdgcn_cvt_pk_fp8_f32(f[2], f[3], p, true);
    o.x = p;
    p = 0;
    p = __builtin_amdgcn_cvt_pk_fp8_f32(f[4], f[5], p, false);
    p = __builtin_amdgcn_cvt_pk_fp8_f32(f[6], f[7], p, true);
    o.y = p;
    return o;
}

// Sum over the 16 lanes of a DPP row (= the 16-lane group of one key row) in
// four VALU ops: xor-1 and xor-2 quad permutes, then the half-row and row
// mirrors. Every lane of the row ends with the total. Unlike __shfl_xor
// (ds_bpermute + an lgkmcnt wait per step) it never leaves the VALU — the
// reduce sits on the loop-carried softmax chain of every key. Must run with
// the whole row active.
template <int CTRL>
__device__ __forceinline__ float dpp_f32(float v) {
    return __builtin_bit_cast(
        float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL,
                                           0xf, 0xf, true));
}
__device__ __forceinline__ float row16_sum_dpp(float v) {
    v += dpp_f32<0xB1>(v);   // quad_perm [1,0,3,2]
    v += dpp_f32<0x4E>(v);   // quad_perm [2,3,0,1]
    v += dpp_f32<0x141>(v);  // row_half_mirror
    v += dpp_f32<0x140>(v);  // row_mirror
    return v;
}

// ---- write path: RoPE(q, k in place) + per-row quantise + paged scatter ----
// One 16-lane group per (token, head) row; rows of a token are ordered
// [q heads | k heads | v heads]. The rotate-half partner of dim d (d +/- 64)
// lives in lane dl^8 of the same group. k is quantised from the roped value
// AS ROUNDED TO bf16 (what the in-place k holds), so the cache and the
// in-place tensor describe the same numbers. Every shuffle runs in uniform
// control flow; dead tail groups compute on row 0 and store nothing.
__global__ __launch_bounds__(256) void rope_kv_fp8_kernel(
    uint32_t* __restrict__ q,        // [T, Hq, 64] words, token stride qts2
    uint32_t* __restrict__ k,        // [T, Hk, 64]
    const uint32_t* __restrict__ v,  // [T, Hk, 64]
    uint2* __restrict__ kc,          // codes, flat [num_slots, Hk, 16] x 8 B
    uint2* __restrict__ vc,
    float* __restrict__ ks,          // scales, flat [num_slots, Hk]
    float* __restrict__ vs,
    const float* __restrict__ cs, const float* __restrict__ sn,
    const int* __restrict__ positions, const int* __restrict__ slots,
    int T, int Hq, int Hk, int qts2, int kts2, int vts2) {
    const int dl = threadIdx.x & 15;
    const int rows_per_tok = Hq + 2 * Hk;
    const int64_t total = (int64_t)T * rows_per_tok;
    const int64_t gid = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 4;
    const bool live = gid < total;
    const int64_t row = live ? gid : 0;
    const int it = (int)(row / rows_per_tok);
    const int r = (int)(row % rows_per_tok);
    const bool is_q = r < Hq;
    const bool is_v = r >= Hq + Hk;
    const int h = is_q ? r : (is_v ? r - Hq - Hk : r - Hq);

    uint32_t* rowp = is_q ? q + (size_t)it * qts2 + (size_t)h * (DHEAD / 2)
                   : is_v ? const_cast<uint32_t*>(v) + (size_t)it * vts2 +
                                (size_t)h * (DHEAD / 2)
                          : k + (size_t)it * kts2 + (size_t)h * (DHEAD / 2);
    const uint4 w = *reinterpret_cast<const uint4*>(rowp + dl * 4);
    float x[8];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        x[j * 2] = bf16_lo((&w.x)[j]);
        x[j * 2 + 1] = bf16_hi((&w.x)[j]);
    }

    // rotate-half RoPE (q and k rows); v rows keep x
    const int pos = positions[it];
    const float* crow = cs + (size_t)pos * (DHEAD / 2) + (dl & 7) * 8;
    const float* srow = sn + (size_t)pos * (DHEAD / 2) + (dl & 7) * 8;
    const float4 c0 = *reinterpret_cast<const float4*>(crow);
    const float4 c1 = *reinterpret_cast<const float4*>(crow + 4);
    const float4 s0 = *reinterpret_cast<const float4*>(srow);
    const float4 s1 = *reinterpret_cast<const float4*>(srow + 4);
    const float c8[8] = {c0.x, c0.y, c0.z, c0.w, c1.x, c1.y, c1.z, c1.w};
    const float s8[8] = {s0.x, s0.y, s0.z, s0.w, s1.x, s1.y, s1.z, s1.w};
    float part[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) part[j] = __shfl_xor(x[j], 8, WAVE);
    uint4 roped;
    if (!is_v) {
        float rr[8];
#pragma unroll
        for (int j = 0; j < 8; ++j)
            rr[j] = (dl < 8) ? x[j] * c8[j] - part[j] * s8[j]
                             : x[j] * c8[j] + part[j] * s8[j];
#pragma unroll
        for (int j = 0; j < 4; ++j)
            (&roped.x)[j] = pack_bf16x2(rr[j * 2], rr[j * 2 + 1]);
        // quantise what the in-place tensor holds: the bf16-rounded value
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            x[j * 2] = bf16_lo((&roped.x)[j]);
            x[j * 2 + 1] = bf16_hi((&roped.x)[j]);
        }
        if (live) *reinterpret_cast<uint4*>(rowp + dl * 4) = roped;
    }

    // per-row absmax -> scale, codes (all lanes take part in the reduction)
    float amax = 0.0f;
#pragma unroll
    for (int j = 0; j < 8; ++j) amax = fmaxf(amax, fabsf(x[j]));
    amax = fmaxf(group16_reduce_max(amax), 1e-8f);
    if (!live || is_q) return;
    const float inv = FP8_MAX / amax;
    float y[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) y[j] = x[j] * inv;
    const uint2 codes = f32x8_to_fp8(y);
    const size_t crow_idx = (size_t)slots[it] * Hk + h;
    (is_v ? vc : kc)[crow_idx * (DHEAD / 8) + dl] = codes;
    if (dl == 0) (is_v ? vs : ks)[crow_idx] = amax / FP8_MAX;
}

extern "C" int oa_rope_kv_fp8(void* stream, void* q, void* k, const void* v,
                              void* k_cache, void* v_cache, void* k_scale,
                              void* v_scale, const void* cos_t,
                              const void* sin_t, const void* positions,
                              const void* slots, int T, int Hq, int Hk, int D,
                              int q_stride, int k_stride, int v_stride) {
    if (D != DHEAD) return -100;
    if ((q_stride | k_stride | v_stride) % 8 != 0) return -101;
    if (T <= 0) return 0;
    const int64_t groups = (int64_t)T * (Hq + 2 * Hk);
    const int64_t grid = CEIL_DIV(groups, 16);
    if (grid > 0x7fffffff) return -102;
    hipLaunchKernelGGL(rope_kv_fp8_kernel, dim3((unsigned)grid), dim3(256), 0,
                       (hipStream_t)stream, (uint32_t*)q, (uint32_t*)k,
                       (const uint32_t*)v, (uint2*)k_cache, (uint2*)v_cache,
                       (float*)k_scale, (float*)v_scale, (const float*)cos_t,
                       (const float*)sin_t, (const int*)positions,
                       (const int*)slots, T, Hq, Hk, q_stride / 2,
                       k_stride / 2, v_stride / 2);
    HIP_CHECK_LAUNCH();
    return 0;
}

// ---- read path for prefill: gather + dequantise to contiguous bf16 ---------
// One 16-lane group per (key, head) row of K and of V (rows [0, Skv*Hk) are
// K, the rest V); value = bf16_rne(float(code) * scale).
__global__ __launch_bounds__(256) void kv_gather_fp8_kernel(
    const uint2* __restrict__ kc, const uint2* __restrict__ vc,
    const float* __restrict__ ks, const float* __restrict__ vs,
    const int* __restrict__ slots,  // [Skv]
    uint4* __restrict__ k_out,      // [Skv, Hk, 16] x 16 B
    uint4* __restrict__ v_out, int Skv, int Hk) {
    const int dl = threadIdx.x & 15;
    const int64_t per = (int64_t)Skv * Hk;
    const int64_t gid = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 4;
    if (gid >= 2 * per) return;
    const bool is_v = gid >= per;
    const int64_t row = is_v ? gid - per : gid;
    const int t = (int)(row / Hk);
    const int h = (int)(row % Hk);
    const size_t src = (size_t)slots[t] * Hk + h;
    const uint2 codes = (is_v ? vc : kc)[src * (DHEAD / 8) + dl];
    const float sc = (is_v ? vs : ks)[src];
    float f[8];
    fp8x8_to_f32(codes, f);
    uint4 o;
#pragma unroll
    for (int j = 0; j < 4; ++j)
        (&o.x)[j] = pack_bf16x2(f[j * 2] * sc, f[j * 2 + 1] * sc);
    (is_v ? v_out : k_out)[(size_t)row * (DHEAD / 8) + dl] = o;
}

extern "C" int oa_kv_gather_fp8(void* stream, const void* k_cache,
                                const void* v_cache, const void* k_scale,
                                const void* v_scale, const void* slots,
                                void* k_out, void* v_out, int Skv, int Hk,
                                int D) {
    if (D != DHEAD) return -100;
    if (Skv <= 0) return 0;
    const int64_t grid = CEIL_DIV((int64_t)2 * Skv * Hk, 16);
    if (grid > 0x7fffffff) return -102;
    hipLaunchKernelGGL(kv_gather_fp8_kernel, dim3((unsigned)grid), dim3(256), 0,
                       (hipStream_t)stream, (const uint2*)k_cache,
                       (const uint2*)v_cache, (const float*)k_scale,
                       (const float*)v_scale, (const int*)slots,
                       (uint4*)k_out, (uint4*)v_out, Skv, Hk);
    HIP_CHECK_LAUNCH();
    return 0;
}

// ---- split-K paged decode attention over the fp8 cache ---------------------
// Same key partition and partial layout as decode_attn_kernel
// (attention_decode.hip): grid (B*Hk, nsplit), chunk = ceil(n / nsplit), four
// waves each taking ceil(span / 4), 16 lanes per key row and 4 keys per wave
// window; o_part / ml_part feed the shared combine kernel.
//
// A key quad is 2 x 8 B of codes per lane (half the bf16 kernel's 2 x 16 B),
// so the quad pipeline is DEPTH = 8 where the bf16 kernel runs 4 (B <= 4,
// G <= 4) and 4 where it runs 2: bytes in flight per wave stay the same.
// Slots are compile-time indexed after full unrolling (a runtime-indexed
// ring would go to scratch).
//
// Scales fold into one multiply per key, not per element:
//   score = dot(q, k_codes) * (k_scale * scale),  o += (p * v_scale) * v_codes
// G4 at depth 4 lands 3 VGPRs over the 128 that four waves per SIMD allow;
// the occupancy request makes the allocator fit (0 B scratch), matching the
// bf16 kernel's residency at batch.
template <int G, int DEPTH>
__global__ __launch_bounds__(256)
__attribute__((amdgpu_waves_per_eu((G == 4 && DEPTH == 4) ? 4 : 1)))
void decode_attn_fp8_kernel(
    const uint32_t* __restrict__ q, const uint2* __restrict__ kc,
    const uint2* __restrict__ vc, const float* __restrict__ ks,
    const float* __restrict__ vs, const int* __restrict__ block_table,
    const int* __restrict__ seq_lens, float* __restrict__ o_part,
    float* __restrict__ ml_part, int B, int Hk, int max_blocks,
    int block_shift /* log2(block_size) */, int nsplit, float scale,
    int qs2 /* q batch-row stride in words */) {
    const int bh = blockIdx.x;
    const int b = bh / Hk;
    const int h = bh % Hk;
    const int split = blockIdx.y;

    const int n = seq_lens[b];
    const int chunk = CEIL_DIV(n, nsplit);
    const int kstart = split * chunk;
    const int kend = min(n, kstart + chunk);

    const int lane = threadIdx.x & (WAVE - 1);
    // wave-uniform on purpose (an SGPR): the wave's key range, and with it the
    // block-table addresses below, must be scalar
    const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x / WAVE);
    const int g16 = lane >> 4;   // key slot within the wave's 4-key window
    const int dl = lane & 15;    // owns dims dl*8 .. dl*8+7

    const int part_idx = (bh * nsplit + split);
    float* opart_row = o_part + ((size_t)part_idx * G) * DHEAD;
    float* mlpart_row = ml_part + ((size_t)part_idx * G) * 2;

    const int span = kend - kstart;
    const int wchunk = CEIL_DIV(max(span, 0), 4);
    const int wstart = kstart + wid * wchunk;
    const int wend = min(kend, wstart + wchunk);

    // q and the output accumulator live as float PAIRS: the converts deliver
    // pairs, and the dot and the accumulate run on packed-f32 VALU ops (half
    // the instructions of the scalar form; at G >= 4 this loop is VALU-bound,
    // not HBM-bound)
    f32x2 qreg[G][4];
#pragma unroll
    for (int gh = 0; gh < G; ++gh) {
        const uint32_t* qp = q + (size_t)b * qs2 + ((size_t)(h * G + gh) * DHEAD + dl * 8) / 2;
        uint4 w = *reinterpret_cast<const uint4*>(qp);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            qreg[gh][j] = f32x2{bf16_lo((&w.x)[j]), bf16_hi((&w.x)[j])};
        }
    }

    float m[G], lsum[G];
    f32x2 o[G][4];
#define O_AT(gh, j) o[gh][(j) >> 1][(j) & 1]
#pragma unroll
    for (int gh = 0; gh < G; ++gh) {
        m[gh] = -INFINITY;
        lsum[gh] = 0.0f;
#pragma unroll
        for (int j = 0; j < 4; ++j) o[gh][j] = f32x2{0.0f, 0.0f};
    }

    const int bmask = (1 << block_shift) - 1;
    const int* btrow = block_table + (size_t)b * max_blocks;

    struct Quad {
        uint2 kw, vw;
        float ksc, vsc;
        bool valid;
    };
    // Every load of the pipeline is UNCONDITIONAL: a key index at or past
    // wend is clamped to the wave's last key (so keys at or past seq_len are
    // never read; the duplicate hits the cache) and `valid` only gates the
    // softmax update. The compiler sizes each s_waitcnt vmcnt(N) from the
    // loads it can PROVE were issued after the one it waits for; loads inside
    // an `if (valid)` prove nothing, N collapses to 0 and every wait drains
    // the whole pipeline.
    // The block-table entries come through SCALAR loads for the same reason:
    // with block_size >= 4 (the launcher rejects smaller) a quad's four keys
    // touch at most two blocks (that of its first and of its last key), both
    // at wave-uniform addresses; a per-lane table load
    // would sit on the vector-memory counter in front of the K/V loads that
    // depend on it. Only called when the wave has a key (wstart < wend).
    auto issue_loads = [&](int kk0, Quad& s) {
        s.valid = kk0 + g16 < wend;
        const int last = wend - 1;
        const int kk = min(kk0 + g16, last);
        const int blk0 = min(kk0, last) >> block_shift;
        const int bt0 = btrow[blk0];
        const int bt1 = btrow[min(kk0 + 3, last) >> block_shift];
        const int64_t slot =
            (int64_t)((kk >> block_shift) == blk0 ? bt0 : bt1) << block_shift |
            (kk & bmask);
        const size_t row = (size_t)slot * Hk + h;
        s.kw = kc[row * (DHEAD / 8) + dl];
        s.vw = vc[row * (DHEAD / 8) + dl];
        s.ksc = ks[row];
        s.vsc = vs[row];
    };
    // Converts, dots and the row reduce run unconditionally (a dead slot
    // holds zero or stale codes whose result is dropped), so one exec-masked
    // region per key quad holds all G softmax updates.
    auto process = [&](const Quad& s) {
        f32x2 kf[4], vf[4];
        float d[G];
        fp8x8_to_f32x2(s.kw, kf);
        fp8x8_to_f32x2(s.vw, vf);
#pragma unroll
        for (int gh = 0; gh < G; ++gh) {
            f32x2 a = qreg[gh][0] * kf[0];
#pragma unroll
            for (int j = 1; j < 4; ++j) a += qreg[gh][j] * kf[j];
            d[gh] = row16_sum_dpp(a[0] + a[1]);  // all 16 lanes of the group get the dot
        }
        if (s.valid) {
            const float sk = s.ksc * scale;
#pragma unroll
            for (int gh = 0; gh < G; ++gh) {
                const float sc = d[gh] * sk;
                const float mn = fmaxf(m[gh], sc);
                const float alpha = __expf(m[gh] - mn);
                const float p = __expf(sc - mn);
                const float pv = p * s.vsc;
                const f32x2 alpha2{alpha, alpha}, pv2{pv, pv};
#pragma unroll
                for (int j = 0; j < 4; ++j) o[gh][j] = o[gh][j] * alpha2 + pv2 * vf[j];
                lsum[gh] = lsum[gh] * alpha + p;
                m[gh] = mn;
            }
        }
    };
    if (wstart < wend) {  // wave-uniform
        Quad ring[DEPTH];
#pragma unroll
        for (int i = 0; i < DEPTH; ++i) {
            ring[i].kw = uint2{0, 0};
            ring[i].vw = uint2{0, 0};
            ring[i].ksc = ring[i].vsc = 0.0f;
            ring[i].valid = false;
        }
#pragma unroll
        for (int i = 0; i < DEPTH - 1; ++i) issue_loads(wstart + 4 * i, ring[i]);
        for (int kk0 = wstart; kk0 < wend; kk0 += 4 * DEPTH) {
#pragma unroll
            for (int i = 0; i < DEPTH; ++i) {
                issue_loads(kk0 + 4 * (i + DEPTH - 1), ring[(i + DEPTH - 1) % DEPTH]);
                process(ring[i]);
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
            for (int j = 0; j < 8; ++j) o2[j] = __shfl_xor(O_AT(gh, j), off, WAVE);
            const float mn = fmaxf(m[gh], m2);
            // guard: empty partial (l == 0, m == -inf) must not produce NaN
            const float a1 = (lsum[gh] > 0.0f) ? __expf(m[gh] - mn) : 0.0f;
            const float a2 = (l2 > 0.0f) ? __expf(m2 - mn) : 0.0f;
#pragma unroll
            for (int j = 0; j < 8; ++j) O_AT(gh, j) = O_AT(gh, j) * a1 + o2[j] * a2;
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
            for (int j = 0; j < 8; ++j) lds_o[wid][gh][dl * 8 + j] = O_AT(gh, j);
            if (dl == 0) {
                lds_ml[wid][gh][0] = m[gh];
                lds_ml[wid][gh][1] = lsum[gh];
            }
        }
    }
    __syncthreads();

    // 256 threads cover G*128 outputs; an empty split publishes l = 0
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
}

#undef O_AT

extern "C" int oa_attention_decode_fp8(
    void* stream, const void* q, const void* kc, const void* vc,
    const void* k_scale, const void* v_scale, const void* block_table,
    const void* seq_lens, void* o_part, void* ml_part, void* out, int B,
    int Hq, int Hk, int D, int max_blocks, int block_size, int nsplit,
    float scale, int q_stride) {
    if (q_stride % 8 != 0) return -103;
    if (D != DHEAD) return -100;
    // block_size >= 4: a key quad may then touch at most two blocks, which
    // is what the scalar block-table loads rely on
    if ((block_size & (block_size - 1)) != 0 || block_size < 4) return -101;
    if (B <= 0 || nsplit <= 0) return -104;
    const int G = Hq / Hk;
    int block_shift = 0;
    while ((1 << block_shift) < block_size) ++block_shift;
    dim3 grid(B * Hk, nsplit), block(256);
    const bool deep = B <= 4;

#define LAUNCH_F8(GV, DV)                                                       \
    hipLaunchKernelGGL((decode_attn_fp8_kernel<GV, DV>), grid, block, 0,        \
                       (hipStream_t)stream, (const uint32_t*)q,                 \
                       (const uint2*)kc, (const uint2*)vc,                      \
                       (const float*)k_scale, (const float*)v_scale,            \
                       (const int*)block_table, (const int*)seq_lens,           \
                       (float*)o_part, (float*)ml_part, B, Hk, max_blocks,      \
                       block_shift, nsplit, scale, q_stride / 2)
#define LAUNCH_G(GV)                                                            \
    do {                                                                        \
        if (deep) LAUNCH_F8(GV, 8);                                             \
        else LAUNCH_F8(GV, 4);                                                  \
    } while (0)
    switch (G) {
        case 1: LAUNCH_G(1); break;
        case 2: LAUNCH_G(2); break;
        case 4: LAUNCH_G(4); break;
        case 8: LAUNCH_F8(8, 4); break;  // qreg + o already hold 128 VGPRs
        default: return -102;
    }
#undef LAUNCH_G
#undef LAUNCH_F8
    HIP_CHECK_LAUNCH();
    return oa_decode_combine(stream, o_part, ml_part, out, B, Hq, Hk, nsplit);
}
