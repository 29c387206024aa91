// Seeded sampler: grammar mask, sparse logit adjustments, top-k, top-p and a
// Gumbel-max draw in one launch.
//
// Semantics (docs/DESIGN.md "Sampling", tests/sampling_cases.py is the oracle):
//   candidates  = mask-allowed tokens with finite z = fl32(float(logit) + delta)
//   greedy      (inv_temp == 0): argmax z, lowest index on ties
//   top-k       keep z >= tau_k, tau_k the k-th largest candidate (ties whole)
//   top-p       s = fl32(z * inv_temp), w = exp(s - s_max) over what top-k
//               kept; keep a token iff the mass strictly above its value is
//               <= top_p * Z
//   draw        argmax of s + g over what is kept, g = -log(-log u), u from
//               word t&3 of Philox4x32-10(key = seed, ctr = (t>>2, step, 0))
//
// Shape: three launches in one linear chain, no atomics on global memory, no
// memset. A whole-row pass costs one CU about 17 us at a 128k vocabulary (it is
// bound by that CU's VALU, not by the 256 KB read), so the two passes that
// must visit every token run on a (chunks, B) grid of 256-thread blocks:
//   1. sample_chunk_first: temperature-only rows draw; every other row counts
//      candidates and finds its maximum. One partial per (row, chunk).
//   2. sample_chunk_hist: the first histogram of the row's first filter over
//      the chunk (top-k adds 1 per token, top-p adds w * 2^40 rounded to an
//      integer), stored whole.
//   3. sample_row_finish: one 1024-thread block per row merges the partials in
//      chunk order, refines the radix selects (11/11/10 bits over the
//      order-preserving u32 image of z; the later passes add few tokens) and
//      draws over what is kept.
// Every merged quantity is an integer sum, min or max, so the bits do not
// depend on the order of the adds, on B or on where the row sits. A row runs
// only the work its parameters need.
//
// Adjustments (logit_bias, penalties) arrive as a per-row sorted (token,
// delta) list. A one-byte-per-granule "adjusted" bitmap in LDS tells the
// stream which tokens have one; only those search the list.
//
// logits bf16 [B, V], V % 8 == 0; mask u32 [B, ceil(V/32)] or null;
// inv_temp f32 [B]; top_k i32 [B]; top_p f32 [B]; seed, step u64 [B];
// adj_ptr i32 [B+1], adj_tok i32 [nnz], adj_val f32 [nnz] or null;
// info i32 [B, 2] or null; out i32 [B]; ws oa_sample_ws_bytes(B, V) bytes, 16-byte
// aligned, need not be initialised.

#include "common.h"

#define SAMPLE_THREADS 1024
#define SAMPLE_WAVES (SAMPLE_THREADS / WAVE)
#define SAMPLE_UNROLL 4
#define SAMPLE_BINS 2048
#define SAMPLE_CHUNKS 16          // chunk blocks per row at most
#define SAMPLE_CHUNK_THREADS 256
#define SAMPLE_MAX_GRANULES 32768  // LDS bitmap bytes; V <= 262144

namespace {

typedef unsigned long long u64;

// the same map as ordered_f32 in sampling.hip: greedy rows must agree with
// masked_argmax bit for bit, tests/test_sampling_gpu.py holds them to it
__device__ __forceinline__ uint32_t sample_ord(float f) {
    const uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ float sample_unord(uint32_t o) {
    return __uint_as_float((o & 0x80000000u) ? (o & 0x7fffffffu) : ~o);
}

struct Philox4 {
    uint32_t r0, r1, r2, r3;
};

__device__ __forceinline__ Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2,
                                                 uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int i = 0; i < 10; ++i) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    Philox4 o;
    o.r0 = c0;
    o.r1 = c1;
    o.r2 = c2;
    o.r3 = c3;
    return o;
}

// u = (2 (r >> 9) + 1) 2^-24, exact and strictly inside (0, 1)
__device__ __forceinline__ float gumbel(uint32_t r) {
    const float u = (float)(2u * (r >> 9) + 1u) * 5.9604644775390625e-08f;
    return -logf(-logf(u));
}

struct Row {
    const uint4* row;       // granules of 8 bf16
    const uint32_t* mrow;   // mask words or null
    const uint8_t* abits;   // LDS: bit j of byte g = token 8g+j is adjusted; null = none
    const int* atok;        // this row's adjustment tokens
    const float* aval;
    int na;
    int g0, g1;             // granules this block streams
};

__device__ __forceinline__ float adj_delta(const Row& r, int t) {
    int lo = 0, hi = r.na - 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (r.atok[mid] < t) lo = mid + 1;
        else hi = mid;
    }
    return r.aval[lo];
}

// Row pointers, this block's granule range and, when the row has adjustments,
// the LDS bitmap. Called by every thread of the block.
__device__ __forceinline__ Row setup_row(const uint4* logits, const uint32_t* mask,
                                         const int* adj_ptr, const int* adj_tok,
                                         const float* adj_val, uint32_t* abits_w, int b, int V,
                                         int mask_words, int g0, int g1) {
    Row r;
    const int G = V / 8;
    r.g0 = g0;
    r.g1 = g1;
    r.row = logits + (size_t)b * G;
    r.mrow = mask ? mask + (size_t)b * mask_words : nullptr;
    r.abits = nullptr;
    r.atok = nullptr;
    r.aval = nullptr;
    r.na = 0;
    if (adj_ptr) {
        const int a0 = adj_ptr[b], a1 = adj_ptr[b + 1];
        if (a1 > a0) {
            r.atok = adj_tok + a0;
            r.aval = adj_val + a0;
            r.na = a1 - a0;
            const int words = (G + 3) / 4;
            for (int i = threadIdx.x; i < words; i += blockDim.x) abits_w[i] = 0;
            __syncthreads();
            for (int i = threadIdx.x; i < r.na; i += blockDim.x) {
                const int t = r.atok[i];
                if (t >= 0 && t < V) atomicOr(&abits_w[t >> 5], 1u << (t & 31));
            }
            __syncthreads();
            r.abits = reinterpret_cast<const uint8_t*>(abits_w);
        }
    }
    return r;
}

// Stream granules [g0, g1) once. f(t0, z0..z3, live) sees four tokens that
// share one Philox block (t0 % 4 == 0): zj is the adjusted fp32 logit of token
// t0+j, live bit j says it is a candidate. Loads are clamped at the range end,
// never predicated.
template <class F>
__device__ __forceinline__ void scan_row(const Row& r, F&& f) {
    const int nthr = blockDim.x;
    for (int g0 = r.g0 + threadIdx.x; g0 < r.g1; g0 += nthr * SAMPLE_UNROLL) {
        // named registers, not arrays: selecting among array elements by a
        // run-time index would put the array in scratch
        uint4 w0, w1, w2, w3;
        uint32_t m0, m1, m2, m3;
#define SAMPLE_LOAD(U, W, M)                                                          \
    {                                                                                 \
        const int g = g0 + U * nthr;                                                  \
        const int gc = min(g, r.g1 - 1);                                              \
        W = r.row[gc];                                                                \
        /* one word fetch per granule: 8 | 32, so a granule never straddles */        \
        const uint32_t mw = r.mrow ? (r.mrow[gc >> 2] >> ((gc & 3) * 8)) & 0xffu : 0xffu; \
        M = g < r.g1 ? mw : 0u;                                                       \
    }
        SAMPLE_LOAD(0, w0, m0)
        SAMPLE_LOAD(1, w1, m1)
        SAMPLE_LOAD(2, w2, m2)
        SAMPLE_LOAD(3, w3, m3)
#undef SAMPLE_LOAD
#pragma unroll 1
        for (int u = 0; u < SAMPLE_UNROLL; ++u) {
            const uint32_t m = u == 0 ? m0 : u == 1 ? m1 : u == 2 ? m2 : m3;
            if (m == 0) continue;
            uint4 q;
            q.x = u == 0 ? w0.x : u == 1 ? w1.x : u == 2 ? w2.x : w3.x;
            q.y = u == 0 ? w0.y : u == 1 ? w1.y : u == 2 ? w2.y : w3.y;
            q.z = u == 0 ? w0.z : u == 1 ? w1.z : u == 2 ? w2.z : w3.z;
            q.w = u == 0 ? w0.w : u == 1 ? w1.w : u == 2 ? w2.w : w3.w;
            const int g = g0 + u * nthr;
            const uint32_t ab = r.abits ? (uint32_t)r.abits[g] & m : 0u;
#pragma unroll 1
            for (int h = 0; h < 2; ++h) {
                const uint32_t mq = (m >> (4 * h)) & 0xfu;
                if (mq == 0) continue;
                const int t0 = g * 8 + h * 4;
                const uint32_t lo = h ? q.z : q.x, hi = h ? q.w : q.y;
                float z0 = bf16_lo(lo), z1 = bf16_hi(lo), z2 = bf16_lo(hi), z3 = bf16_hi(hi);
                uint32_t aq = (ab >> (4 * h)) & 0xfu;
                while (aq) {  // rare: one search per adjusted, allowed token
                    const int ja = __ffs(aq) - 1;
                    aq &= aq - 1;
                    const float d = adj_delta(r, t0 + ja);
                    z0 = ja == 0 ? z0 + d : z0;
                    z1 = ja == 1 ? z1 + d : z1;
                    z2 = ja == 2 ? z2 + d : z2;
                    z3 = ja == 3 ? z3 + d : z3;
                }
                // a candidate is allowed and neither -inf nor NaN
                const uint32_t live = ((mq & 1u) && z0 > -INFINITY ? 1u : 0u) |
                                      ((mq & 2u) && z1 > -INFINITY ? 2u : 0u) |
                                      ((mq & 4u) && z2 > -INFINITY ? 4u : 0u) |
                                      ((mq & 8u) && z3 > -INFINITY ? 8u : 0u);
                if (live) f(t0, z0, z1, z2, z3, live);
            }
        }
    }
}

// A partial of a pass: candidate (or kept) count, smallest kept ord(z), best
// packed key. All three merge by integer sum / min / max, so any order of
// merging gives the same bits.
struct alignas(16) Red {
    uint32_t cnt;   // sum
    uint32_t omin;  // min
    u64 best;       // max
};

__device__ __forceinline__ Red red_merge(Red a, Red b) {
    a.cnt += b.cnt;
    a.omin = min(a.omin, b.omin);
    a.best = b.best > a.best ? b.best : a.best;
    return a;
}

// Block reduction; every thread returns the result. Integer only.
__device__ __forceinline__ Red block_reduce(Red v, uint32_t* s_cnt, uint32_t* s_min,
                                            u64* s_best) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        Red o;
        o.cnt = __shfl_xor(v.cnt, off, WAVE);
        o.omin = __shfl_xor(v.omin, off, WAVE);
        o.best = __shfl_xor(v.best, off, WAVE);
        v = red_merge(v, o);
    }
    const int wid = threadIdx.x / WAVE;
    const int nwaves = blockDim.x / WAVE;
    __syncthreads();  // the arrays may still be read from an earlier call
    if ((threadIdx.x & (WAVE - 1)) == 0) {
        s_cnt[wid] = v.cnt;
        s_min[wid] = v.omin;
        s_best[wid] = v.best;
    }
    __syncthreads();
    Red r = {0u, 0xffffffffu, 0ull};
#pragma unroll 4
    for (int i = 0; i < nwaves; ++i) {
        Red o = {s_cnt[i], s_min[i], s_best[i]};
        r = red_merge(r, o);
    }
    return r;
}

// The chunk partials of one row, merged in chunk order.
__device__ __forceinline__ Red merge_parts(const Red* part, int chunks) {
    Red r = {0u, 0xffffffffu, 0ull};
    for (int c = 0; c < chunks; ++c) r = red_merge(r, part[c]);
    return r;
}

// candidate count and best {ord(z), lowest index} of this thread's tokens
__device__ __forceinline__ Red pass0_scan(const Row& r) {
    Red v = {0u, 0xffffffffu, 0ull};
    scan_row(r, [&](int t0, float z0, float z1, float z2, float z3, uint32_t live) {
        const float z[4] = {z0, z1, z2, z3};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if ((live >> j) & 1u) {
                v.cnt++;
                // z + 0.0f: -0 ties with +0 and the lowest index wins, as in masked_argmax
                const u64 key =
                    ((u64)sample_ord(z[j] + 0.0f) << 32) | (uint32_t)(0x7fffffff - (t0 + j));
                v.best = key > v.best ? key : v.best;
            }
        }
    });
    return v;
}

// Gumbel-max draw over this thread's tokens with ord(z) >= thr
__device__ __forceinline__ Red draw_scan(const Row& r, uint32_t thr, float it, u64 sd, u64 st) {
    const uint32_t k0 = (uint32_t)sd, k1 = (uint32_t)(sd >> 32);
    const uint32_t c1 = (uint32_t)st, c2 = (uint32_t)(st >> 32);
    Red v = {0u, 0xffffffffu, 0ull};
    scan_row(r, [&](int t0, float z0, float z1, float z2, float z3, uint32_t live) {
        const uint32_t kept = live & ((sample_ord(z0) >= thr ? 1u : 0u) |
                                      (sample_ord(z1) >= thr ? 2u : 0u) |
                                      (sample_ord(z2) >= thr ? 4u : 0u) |
                                      (sample_ord(z3) >= thr ? 8u : 0u));
        if (kept == 0) return;
        const Philox4 x = philox4x32_10((uint32_t)(t0 >> 2), c1, c2, 0u, k0, k1);
#pragma unroll 1
        for (int j = 0; j < 4; ++j) {
            if ((kept >> j) & 1u) {
                const float zj = j == 0 ? z0 : j == 1 ? z1 : j == 2 ? z2 : z3;
                const uint32_t rj = j == 0 ? x.r0 : j == 1 ? x.r1 : j == 2 ? x.r2 : x.r3;
                v.cnt++;
                v.omin = min(v.omin, sample_ord(zj));
                const float key = __fadd_rn(__fmul_rn(zj, it), gumbel(rj));
                const u64 pk = ((u64)sample_ord(key) << 32) | (uint32_t)(0x7fffffff - (t0 + j));
                v.best = pk > v.best ? pk : v.best;
            }
        }
    });
    return v;
}

// One histogram pass of the radix select into LDS `hist` (zeroed by the
// caller): MASS = false adds 1 per token, MASS = true adds w * 2^40 rounded.
template <bool MASS>
__device__ __forceinline__ void hist_scan(const Row& r, u64* hist, int pass, uint32_t prefix,
                                          uint32_t floor_ord, float inv_temp, float smax) {
    const int shift = pass == 0 ? 21 : pass == 1 ? 10 : 0;
    const int nbits = pass == 2 ? 10 : 11;
    const int hshift = shift + nbits;  // bits above this pass: 32, 21, 10
    scan_row(r, [&](int t0, float z0, float z1, float z2, float z3, uint32_t live) {
        (void)t0;
        const float z[4] = {z0, z1, z2, z3};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t o = sample_ord(z[j]);
            bool in = ((live >> j) & 1u) && o >= floor_ord;
            if (pass > 0) in = in && ((o >> hshift) == (prefix >> hshift));
            if (in) {
                u64 wgt = 1;
                if (MASS)
                    wgt = __float2ull_rn(expf(__fsub_rn(__fmul_rn(z[j], inv_temp), smax)) *
                                         1099511627776.0f);
                if (wgt) atomicAdd(&hist[(o >> shift) & ((1u << nbits) - 1u)], wgt);
            }
        }
    });
}

// Radix select over ord(z) of the candidates with ord(z) >= floor_ord.
// MASS = false: weight 1, limit = k - 1       -> the k-th largest value
// MASS = true:  weight w * 2^40, limit = floor(top_p * Z), Z from the first
//               histogram                      -> the lowest value whose mass
//                                                 strictly above is <= limit
// Either way the answer is the lowest non-empty bin whose weight above it is
// <= limit, refined over three passes. With `first` given, the first pass's
// histogram is the sum, in chunk order, of the chunk histograms found there.
template <bool MASS>
__device__ __forceinline__ uint32_t radix_select(const Row& r, u64* hist, u64* s_sel,
                                                 const u64* first, int chunks,
                                                 uint32_t floor_ord, u64 limit, float top_p,
                                                 float inv_temp, float smax) {
    uint32_t prefix = 0;
#pragma unroll 1
    for (int pass = 0; pass < 3; ++pass) {
        const int shift = pass == 0 ? 21 : pass == 1 ? 10 : 0;
        if (pass == 0 && first) {
            for (int i = threadIdx.x; i < SAMPLE_BINS; i += blockDim.x) {
                u64 a = 0;
                for (int c = 0; c < chunks; ++c) a += first[(size_t)c * SAMPLE_BINS + i];
                hist[i] = a;
            }
        } else {
            for (int i = threadIdx.x; i < SAMPLE_BINS; i += blockDim.x) hist[i] = 0;
            __syncthreads();
            hist_scan<MASS>(r, hist, pass, prefix, floor_ord, inv_temp, smax);
        }
        __syncthreads();
        if (threadIdx.x < WAVE) {
            // lane l owns bins [32 l, 32 l + 32); above = weight in higher lanes
            const int lane = threadIdx.x;
            const int per = SAMPLE_BINS / WAVE;
            u64 mine = 0;
#pragma unroll 4
            for (int i = 0; i < per; ++i) mine += hist[lane * per + i];
            u64 incl = mine;  // inclusive suffix sum over lanes
#pragma unroll
            for (int off = 1; off < WAVE; off <<= 1) {
                const u64 o = __shfl_down(incl, off, WAVE);
                if (lane + off < WAVE) incl += o;
            }
            if (MASS && pass == 0) {
                const u64 Z = __shfl(incl, 0, WAVE);
                limit = top_p > 0.0f ? (u64)((double)top_p * (double)Z) : 0ull;
            }
            u64 above = incl - mine;
            int sel = 0x7fffffff;
            u64 sel_above = 0;
#pragma unroll 4
            for (int i = per - 1; i >= 0; --i) {
                const u64 h = hist[lane * per + i];
                if (h > 0 && above <= limit) {
                    sel = lane * per + i;
                    sel_above = above;
                }
                above += h;
            }
            int lowest = sel;
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) lowest = min(lowest, __shfl_xor(lowest, off, WAVE));
            if (sel == lowest && sel != 0x7fffffff) {
                s_sel[0] = (u64)(uint32_t)sel;
                s_sel[1] = limit - sel_above;
            }
        }
        __syncthreads();
        prefix |= (uint32_t)s_sel[0] << shift;
        limit = s_sel[1];
    }
    return prefix;
}

struct Mode {
    float it, p;
    int k;
    bool greedy, use_k, use_p;
};

__device__ __forceinline__ Mode row_mode(const float* inv_temp, const int* top_k,
                                         const float* top_p, int b) {
    Mode m;
    m.it = inv_temp[b];
    m.k = top_k[b];
    m.p = top_p[b];
    m.greedy = !(m.it > 0.0f);
    m.use_k = !m.greedy && m.k > 0;
    m.use_p = !m.greedy && m.p < 1.0f;
    return m;
}

__device__ __forceinline__ void chunk_range(int V, int& g0, int& g1) {
    const int G = V / 8;
    const int per = CEIL_DIV(G, (int)gridDim.x);
    g0 = min(G, (int)blockIdx.x * per);
    g1 = min(G, g0 + per);
}

}  // namespace

// Launch 1, grid (chunks, B): the one pass a row can start without knowing
// anything about itself, over this block's chunk. A temperature-only row
// draws; every other row counts its candidates and finds its maximum.
__global__ __launch_bounds__(SAMPLE_CHUNK_THREADS) void sample_chunk_first(
    const uint4* __restrict__ logits, const uint32_t* __restrict__ mask,
    const float* __restrict__ inv_temp, const int* __restrict__ top_k,
    const float* __restrict__ top_p, const u64* __restrict__ seed,
    const u64* __restrict__ step, const int* __restrict__ adj_ptr,
    const int* __restrict__ adj_tok, const float* __restrict__ adj_val,
    Red* __restrict__ part, int V, int mask_words) {
    extern __shared__ u64 smem[];
    uint32_t* abits_w = reinterpret_cast<uint32_t*>(smem + SAMPLE_BINS);
    __shared__ uint32_t s_cnt[SAMPLE_WAVES], s_min[SAMPLE_WAVES];
    __shared__ u64 s_best[SAMPLE_WAVES];
    const int b = blockIdx.y;
    int g0, g1;
    chunk_range(V, g0, g1);
    const Row r = setup_row(logits, mask, adj_ptr, adj_tok, adj_val, abits_w, b, V, mask_words,
                            g0, g1);
    const Mode m = row_mode(inv_temp, top_k, top_p, b);
    Red v = (m.greedy || m.use_k || m.use_p) ? pass0_scan(r)
                                             : draw_scan(r, 0u, m.it, seed[b], step[b]);
    v = block_reduce(v, s_cnt, s_min, s_best);
    if (threadIdx.x == 0) part[(size_t)b * gridDim.x + blockIdx.x] = v;
}

// Launch 2, grid (chunks, B): the first histogram of the row's first filter
// over this block's chunk, written out whole with plain stores. Rows without
// a filter, and rows whose k covers every candidate and have no top-p, leave.
__global__ __launch_bounds__(SAMPLE_CHUNK_THREADS) void sample_chunk_hist(
    const uint4* __restrict__ logits, const uint32_t* __restrict__ mask,
    const float* __restrict__ inv_temp, const int* __restrict__ top_k,
    const float* __restrict__ top_p, const int* __restrict__ adj_ptr,
    const int* __restrict__ adj_tok, const float* __restrict__ adj_val,
    const Red* __restrict__ part, u64* __restrict__ hist_out, int V, int mask_words) {
    extern __shared__ u64 smem[];
    u64* hist = smem;
    uint32_t* abits_w = reinterpret_cast<uint32_t*>(smem + SAMPLE_BINS);
    const int b = blockIdx.y;
    const Mode m = row_mode(inv_temp, top_k, top_p, b);
    if (!(m.use_k || m.use_p)) return;
    const Red t = merge_parts(part + (size_t)b * gridDim.x, gridDim.x);
    if (t.cnt == 0) return;
    const bool by_count = m.use_k && (uint32_t)m.k < t.cnt;
    if (!by_count && !m.use_p) return;
    int g0, g1;
    chunk_range(V, g0, g1);
    const Row r = setup_row(logits, mask, adj_ptr, adj_tok, adj_val, abits_w, b, V, mask_words,
                            g0, g1);
    for (int i = threadIdx.x; i < SAMPLE_BINS; i += blockDim.x) hist[i] = 0;
    __syncthreads();
    if (by_count) {
        hist_scan<false>(r, hist, 0, 0u, 0u, 0.0f, 0.0f);
    } else {
        const float zmax = sample_unord((uint32_t)(t.best >> 32));
        hist_scan<true>(r, hist, 0, 0u, 0u, m.it, __fmul_rn(zmax, m.it));
    }
    __syncthreads();
    u64* dst = hist_out + ((size_t)b * gridDim.x + blockIdx.x) * SAMPLE_BINS;
    for (int i = threadIdx.x; i < SAMPLE_BINS; i += blockDim.x) dst[i] = hist[i];
}

// Launch 3, one block per row: merges the chunk partials in chunk order,
// finishes the selects (their later passes touch few tokens) and draws.
__global__ __launch_bounds__(SAMPLE_THREADS) void sample_row_finish(
    const uint4* __restrict__ logits, const uint32_t* __restrict__ mask,
    const float* __restrict__ inv_temp, const int* __restrict__ top_k,
    const float* __restrict__ top_p, const u64* __restrict__ seed,
    const u64* __restrict__ step, const int* __restrict__ adj_ptr,
    const int* __restrict__ adj_tok, const float* __restrict__ adj_val,
    const Red* __restrict__ part, const u64* __restrict__ hist_in, int chunks,
    int* __restrict__ info, int* __restrict__ out, int V, int mask_words) {
    extern __shared__ u64 smem[];
    u64* hist = smem;                                                     // SAMPLE_BINS
    uint32_t* abits_w = reinterpret_cast<uint32_t*>(smem + SAMPLE_BINS);  // G bytes
    __shared__ uint32_t s_cnt[SAMPLE_WAVES], s_min[SAMPLE_WAVES];
    __shared__ u64 s_best[SAMPLE_WAVES];
    __shared__ u64 s_sel[2];

    const int b = blockIdx.x;
    const Mode m = row_mode(inv_temp, top_k, top_p, b);
    Red v = merge_parts(part + (size_t)b * chunks, chunks);
    const bool filtered = m.use_k || m.use_p;
    if (filtered && v.cnt != 0) {
        const Row r = setup_row(logits, mask, adj_ptr, adj_tok, adj_val, abits_w, b, V,
                                mask_words, 0, V / 8);
        const u64* first = hist_in + (size_t)b * chunks * SAMPLE_BINS;
        const float zmax = sample_unord((uint32_t)(v.best >> 32));
        uint32_t thr = 0;  // keep ord(z) >= thr
        if (m.use_k && (uint32_t)m.k < v.cnt) {
            thr = radix_select<false>(r, hist, s_sel, first, chunks, 0u, (u64)(m.k - 1), 0.0f,
                                      0.0f, 0.0f);
            first = nullptr;
        }
        if (m.use_p) {
            const uint32_t tp = radix_select<true>(r, hist, s_sel, first, chunks, thr, 0ull, m.p,
                                                   m.it, __fmul_rn(zmax, m.it));
            thr = max(thr, tp);
        }
        v = draw_scan(r, thr, m.it, seed[b], step[b]);
        v = block_reduce(v, s_cnt, s_min, s_best);
    }
    if (threadIdx.x == 0) {
        out[b] = v.cnt ? 0x7fffffff - (int)(uint32_t)(v.best & 0xffffffffu) : -1;
        if (info) {
            // greedy: candidate count and the winner's z; else kept count and smallest kept z
            const uint32_t zo = m.greedy ? (uint32_t)(v.best >> 32) : v.omin;
            info[2 * b] = (int)v.cnt;
            info[2 * b + 1] = v.cnt ? (int)__float_as_uint(sample_unord(zo)) : 0x7f800000;
        }
    }
}

static int sample_chunks(int V) {
    // one sweep of a chunk block covers SAMPLE_CHUNK_THREADS * SAMPLE_UNROLL granules
    const int c = CEIL_DIV(V / 8, SAMPLE_CHUNK_THREADS * SAMPLE_UNROLL);
    return c < 1 ? 1 : (c > SAMPLE_CHUNKS ? SAMPLE_CHUNKS : c);
}

extern "C" long long oa_sample_ws_bytes(int B, int V) {
    if (B <= 0 || V <= 0) return 0;
    const long long per = sizeof(Red) + (long long)SAMPLE_BINS * sizeof(u64);
    return (long long)B * sample_chunks(V) * per;
}

extern "C" int oa_sample(void* stream, const void* logits, const void* mask,
                         const void* inv_temp, const void* top_k, const void* top_p,
                         const void* seed, const void* step, const void* adj_ptr,
                         const void* adj_tok, const void* adj_val, void* ws, void* info,
                         void* out, int B, int V) {
    if (V % 8 != 0) return -100;
    if (V <= 0 || V / 8 > SAMPLE_MAX_GRANULES) return -101;
    if (B <= 0) return 0;
    if (!ws) return -102;
    const bool adj = adj_ptr && adj_tok && adj_val;
    const int* ap = adj ? (const int*)adj_ptr : nullptr;
    const int mask_words = CEIL_DIV(V, 32);
    const int chunks = sample_chunks(V);
    const size_t lds = SAMPLE_BINS * sizeof(u64) + (size_t)CEIL_DIV(V / 8, 4) * 4;
    Red* part = (Red*)ws;
    u64* hist = (u64*)((char*)ws + (size_t)B * chunks * sizeof(Red));
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(sample_chunk_first, dim3(chunks, B), dim3(SAMPLE_CHUNK_THREADS), lds, s,
                       (const uint4*)logits, (const uint32_t*)mask, (const float*)inv_temp,
                       (const int*)top_k, (const float*)top_p, (const u64*)seed,
                       (const u64*)step, ap, (const int*)adj_tok, (const float*)adj_val, part, V,
                       mask_words);
    HIP_CHECK_LAUNCH();
    hipLaunchKernelGGL(sample_chunk_hist, dim3(chunks, B), dim3(SAMPLE_CHUNK_THREADS), lds, s,
                       (const uint4*)logits, (const uint32_t*)mask, (const float*)inv_temp,
                       (const int*)top_k, (const float*)top_p, ap, (const int*)adj_tok,
                       (const float*)adj_val, (const Red*)part, hist, V, mask_words);
    HIP_CHECK_LAUNCH();
    hipLaunchKernelGGL(sample_row_finish, dim3(B), dim3(SAMPLE_THREADS), lds, s,
                       (const uint4*)logits, (const uint32_t*)mask, (const float*)inv_temp,
                       (const int*)top_k, (const float*)top_p, (const u64*)seed,
                       (const u64*)step, ap, (const int*)adj_tok, (const float*)adj_val,
                       (const Red*)part, (const u64*)hist, chunks, (int*)info, (int*)out, V,
                       mask_words);
    HIP_CHECK_LAUNCH();
    return 0;
}
