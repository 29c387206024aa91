// Masked lm_head GEMV with an argmax epilogue — the greedy decode head.
//
//   out[m] = argmax over allowed t of bf16(x[m, :] . W[t, :])     (M <= 2)
//
// A greedy decode step with no logit transform and no logprobs reads nothing
// of the logits row but its masked argmax, and a token whose mask bit is 0 can
// never be chosen. So this kernel streams only the W rows some batch row
// allows and keeps the running best in registers: no logits row is written,
// and the memset / scan / finish tail of oa_masked_argmax shrinks to one tiny
// finish kernel.
//
// Arithmetic is that of the unfused head. The row pipeline is the two-row
// gemv_kernel<M, false, false, 2, KU> one (gemv_pipe.h): two adjacent rows per
// wave, one accumulator per (row, m) fed in ascending K, wave_reduce_sum — a
// live row's fp32 value is bit-identical to the logit oa_gemv computes. It is
// rounded with f32_to_bf16 before it is compared, because the unfused path
// takes its argmax over the bf16 logits row; keys are packed as sampling.hip
// packs them, {ordered_f32(value), 0x7fffffff - idx}, so the lowest index wins
// a tie. (-inf and NaN never enter, as in masked_argmax_scan.)
//
// Row skip without a load chain: a wave's trips are p0 + t * nwaves row pairs.
// Lane t fetches the mask word of trip t — ONE vector load per batch row covers
// 64 trips — and four ballots turn the bits into wave-uniform 64-bit trip
// masks. The trip loop then walks the set bits of their OR: a dead pair costs
// nothing, and no mask load sits in front of any W load. V % 8 == 0 makes
// every pair whole, and lanes whose trip lies past V contribute no bit, so
// mask bits at positions >= V are ignored.
//
// Reduction: running best per (wave, m) in registers, the block's four waves
// meet in LDS, every block stores one key per m to ws[m][blockIdx.x] with a
// plain store (0 = nothing live; no memset, no atomics); head_argmax_finish
// (one block) takes the maximum over the grid's keys.

#include "common.h"
#include "gemv_pipe.h"

// K depth of the row pipeline per M. Depth 1 is what the two-row GEMV ships
// for lm_head. tests/test_head_resources.py holds the shipped depths to the
// register budget of HEAD_WAVES: M = 1 fits 8 waves per SIMD at depth 1 and 2
// (depth 4 spills there); M = 2 carries two activation rows and four
// accumulators and fits 7 at depth 1, so its grid is sized for 7.
#define HEAD_ARGMAX_KU_M1 2
#define HEAD_ARGMAX_KU_M2 1
#define HEAD_WAVES(M) ((M) == 1 ? 8 : 7)  // resident waves per SIMD

typedef unsigned long long u64;

__device__ __forceinline__ uint32_t head_ordered_f32(float f) {
    union {
        uint32_t u;
        float f;
    } v;
    v.f = f;
    return (v.u & 0x80000000u) ? ~v.u : (v.u | 0x80000000u);
}

// best + 0.0f turns -0 into +0: the wave compared floats, where -0 == +0 and
// the lowest index wins; the packed key alone would order -0 below +0
__device__ __forceinline__ u64 head_key(float best, int besti) {
    return besti < 0 ? 0ull
                     : ((u64)head_ordered_f32(best + 0.0f) << 32) |
                           (unsigned)(0x7fffffff - besti);
}

template <int M, int KU>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(HEAD_WAVES(M))))
void head_argmax_kernel(
    const uint32_t* __restrict__ x,     // [M, K/2]
    const uint32_t* __restrict__ w,     // [V, K/2]
    const uint32_t* __restrict__ mask,  // [M, mask_words] or nullptr
    u64* __restrict__ ws,               // [M, gridDim.x]
    int V, int k2, int mask_words) {
    const int lane = threadIdx.x & (WAVE - 1);
    // wave-uniform on purpose: row addresses and the trip loop stay scalar
    const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x / WAVE);
    const int wave = blockIdx.x * 4 + wid;
    const int nwaves = gridDim.x * 4;
    const int pairs = V >> 1;  // V % 8 == 0: every pair is whole

    float best[M];
    int besti[M];
    float rstd[M];
#pragma unroll
    for (int m = 0; m < M; ++m) {
        best[m] = -INFINITY;
        besti[m] = -1;
        rstd[m] = 1.0f;
    }
    bool need_rstd = false;

    // 64 trips per chunk; V = 128256 on the 2048-block grid is 8 trips
    for (int p0 = wave; p0 < pairs; p0 += nwaves * WAVE) {
        const int pl = p0 + lane * nwaves;  // lane t: row pair of trip t
        u64 allow[M][2], live = 0;
#pragma unroll
        for (int m = 0; m < M; ++m) {
            uint32_t bits = 0;
            if (pl < pairs)
                bits = mask ? (mask[(size_t)m * mask_words + (pl >> 4)] >>
                               ((pl & 15) * 2)) & 3u
                            : 3u;
            allow[m][0] = __ballot(bits & 1u);
            allow[m][1] = __ballot(bits & 2u);
            live |= allow[m][0] | allow[m][1];
        }
        while (live) {
            const int t = __builtin_ctzll(live);
            live &= live - 1;
            const int row0 = (p0 + t * nwaves) * 2;
            const uint32_t* wr[2];
            wr[0] = w + (size_t)row0 * k2;
            wr[1] = wr[0] + k2;
            float acc[2][M];
#pragma unroll
            for (int m = 0; m < M; ++m) acc[0][m] = acc[1][m] = 0.0f;
            gemv_row_pieces<M, false, 2, KU, 4>(acc, rstd, need_rstd, wr, x,
                                                nullptr, k2, lane, 0.0f);
#pragma unroll
            for (int m = 0; m < M; ++m) {
#pragma unroll
                for (int rr_ = 0; rr_ < 2; ++rr_) {
                    const float v = wave_reduce_sum(acc[rr_][m]);
                    const float q = bf16_to_f32(f32_to_bf16(v));
                    // rows ascend within a wave: strict > keeps the lowest
                    if (((allow[m][rr_] >> t) & 1ull) && q > best[m]) {
                        best[m] = q;
                        besti[m] = row0 + rr_;
                    }
                }
            }
        }
    }

    __shared__ u64 sk[M][4];
    if (lane == 0) {
#pragma unroll
        for (int m = 0; m < M; ++m) sk[m][wid] = head_key(best[m], besti[m]);
    }
    __syncthreads();
    if (threadIdx.x < M) {
        const int m = threadIdx.x;
        u64 k = sk[m][0];
#pragma unroll
        for (int i = 1; i < 4; ++i) k = max(k, sk[m][i]);
        ws[(size_t)m * gridDim.x + blockIdx.x] = k;
    }
}

__global__ __launch_bounds__(256) void head_argmax_finish(
    const u64* __restrict__ ws, int* __restrict__ out, int M, int n) {
    __shared__ u64 sk[4];
    const int lane = threadIdx.x & (WAVE - 1);
    const int wid = threadIdx.x / WAVE;
    for (int m = 0; m < M; ++m) {
        u64 k = 0;
        for (int i = threadIdx.x; i < n; i += blockDim.x)
            k = max(k, ws[(size_t)m * n + i]);
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) k = max(k, __shfl_xor(k, off, WAVE));
        if (lane == 0) sk[wid] = k;
        __syncthreads();
        if (threadIdx.x == 0) {
            k = max(max(sk[0], sk[1]), max(sk[2], sk[3]));
            out[m] = k ? (int)(0x7fffffff - (unsigned)(k & 0xffffffffu)) : -1;
        }
        __syncthreads();
    }
}

// Blocks of the head kernel (= keys per batch row in ws): four waves of one
// row pair each per block, capped at the blocks that are resident at once —
// 256 CUs x HEAD_WAVES(M) waves per SIMD. The rest goes by grid stride, so
// dead rows spread over all waves and the key array stays small.
extern "C" int oa_head_argmax_grid(int V, int M) {
    const int cap = 256 * (M == 1 ? HEAD_WAVES(1) : HEAD_WAVES(2));
    return V < 8 ? 1 : min(cap, CEIL_DIV(V, 8));
}

template <int M, int KU>
static void head_argmax_launch(hipStream_t s, int grid, const void* x,
                               const void* w, const void* mask, void* ws, int V,
                               int K) {
    hipLaunchKernelGGL((head_argmax_kernel<M, KU>), dim3(grid), dim3(256), 0, s,
                       (const uint32_t*)x, (const uint32_t*)w,
                       (const uint32_t*)mask, (u64*)ws, V, K / 2,
                       CEIL_DIV(V, 32));
}

// probe/test entry: the head at an explicit K depth (M = 2: depth 1 only)
extern "C" int oa_head_argmax_ku(void* stream, const void* x, const void* w,
                                 const void* mask, void* ws, void* out, int M,
                                 int V, int K, int ku) {
    if (V % 8 != 0 || V < 8) return -100;
    if (M < 1 || M > 2) return -101;
    if (K % 8 != 0 || K < 8) return -102;
    const int grid = oa_head_argmax_grid(V, M);
    hipStream_t s = (hipStream_t)stream;
    if (M == 1 && ku == 1) head_argmax_launch<1, 1>(s, grid, x, w, mask, ws, V, K);
    else if (M == 1 && ku == 2) head_argmax_launch<1, 2>(s, grid, x, w, mask, ws, V, K);
    else if (M == 2 && ku == 1) head_argmax_launch<2, 1>(s, grid, x, w, mask, ws, V, K);
    else return -103;
    HIP_CHECK_LAUNCH();
    hipLaunchKernelGGL(head_argmax_finish, dim3(1), dim3(256), 0, s,
                       (const u64*)ws, (int*)out, M, grid);
    HIP_CHECK_LAUNCH();
    return 0;
}

// x bf16 [M, K]; w bf16 [V, K]; mask uint32 [M, ceil(V/32)] (bit t set =
// allowed) or nullptr; ws u64 [M, oa_head_argmax_grid(V, M)]; out int32 [M]
// (-1: no token allowed). M in {1, 2}, V % 8 == 0, K % 8 == 0.
extern "C" int oa_head_argmax(void* stream, const void* x, const void* w,
                              const void* mask, void* ws, void* out, int M,
                              int V, int K) {
    return oa_head_argmax_ku(stream, x, w, mask, ws, out, M, V, K,
                             M == 1 ? HEAD_ARGMAX_KU_M1 : HEAD_ARGMAX_KU_M2);
}

