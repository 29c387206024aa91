// Skinny-M GEMM ("GEMV") for decode projections on MI355X:
//   out[M, N] = x[M, K] @ W[N, K]^T      (torch F.linear layout, bf16)
//
// Decode at small batch is weight-streaming-bound: each step reads every
// weight byte once. hipBLASLt's skinny kernels measure ~2.5x off the HBM
// roofline at M=1 (19.9us for a 50 MB qkv read, ~8us at 6.3 TB/s); this
// kernel follows the CDNA guide's GEMV row ("M <= 16 decode weights: operand
// streamed once per block, not shared across waves -> load straight to
// VGPRs, deep unroll, late vmcnt"): W rows stream through 16-B vector loads
// per lane, fp32 accumulate, one wave-reduction per (row, m). The activation
// x is tiny (8-56 KB) and L1-resident after the first pass — each lane
// re-reads only its own 16-B slices, so no LDS staging is needed.
//
// K pipeline: one 16-B load per lane and trip keeps RW KiB per wave in
// flight, and a row then costs K/512 serial HBM round trips. The K loop
// instead walks pieces of KU * 64 16-B units (geometry: gemv_tile.h; the piece
// loop itself: gemv_pipe.h, shared with head_argmax.hip): a wave issues the
// piece's x (and norm-weight) loads and its KU W loads per row back to back,
// then consumes the slots in order — KU * RW KiB in flight per wave, K/(512
// KU) round trips per row. Each (row, m) keeps ONE accumulator fed in
// ascending K, low half before high half, so every depth is bit-identical to
// depth 1.
//
// Requires K % 8 == 0 (16-B units); callers fall back to hipBLASLt otherwise
// (and for M > 8, where the MFMA path wins).

#include "common.h"
#include "gemv_pipe.h"
#include <cstdlib>

// fp32 rstd of x row m: one extra pass over the (L1-resident) activation
__device__ __forceinline__ float row_rstd(const uint32_t* xrow, int k2, int lane,
                                          float eps) {
    float ss = 0.0f;
    for (int i = lane * 4; i < k2; i += WAVE * 4) {
        uint4 xv = *reinterpret_cast<const uint4*>(xrow + i);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float lo = bf16_lo((&xv.x)[j]), hi = bf16_hi((&xv.x)[j]);
            ss = fmaf(lo, lo, ss);
            ss = fmaf(hi, hi, ss);
        }
    }
    ss = wave_reduce_sum(ss);
    return rsqrtf(ss / (float)(k2 * 2) + eps);
}

// NORM: x is normalized on the fly (rstd prologue + norm-weight multiply) —
// the separate rmsnorm kernel and its output round-trip disappear.
// ADDRES: the epilogue adds a residual row — out = x @ W^T + residual, i.e.
// the new residual stream is produced directly by the projection.
// KU: 16-B W loads per row in flight per K tile (1 = one load per trip).
template <int M, bool NORM, bool ADDRES, int RW = 2, int KU = 1>
__global__ __launch_bounds__(256) void gemv_kernel(
    const uint32_t* __restrict__ x,  // [M, K/2]
    const uint32_t* __restrict__ w,  // [N, K/2]
    uint32_t* __restrict__ out,      // [M, N] bf16 (u16 scalar writes)
    const uint32_t* __restrict__ wn, // [K/2] rmsnorm weight (NORM only)
    const uint32_t* __restrict__ res,// [M, N] residual (ADDRES only)
    int N, int k2 /* K/2 */, float eps) {
    // rstd prologue depth: K = 4096 in one trip where the registers allow
    constexpr int XD = (RW == 1 && KU <= 4 && M == 1) ? 8 : 4;
    const int lane = threadIdx.x & (WAVE - 1);
    const int wid = threadIdx.x / WAVE;

    float rstd[M];
#pragma unroll
    for (int m = 0; m < M; ++m) rstd[m] = 1.0f;
    bool need_rstd = NORM;
    if (NORM && M > 2) {  // depth-1 forms: the plain prologue, up front
#pragma unroll
        for (int m = 0; m < M; ++m) rstd[m] = row_rstd(x + (size_t)m * k2, k2, lane, eps);
        need_rstd = false;
    }

    // RW adjacent W rows per wave: multiplies the outstanding 16-B streams
    // per wave (the 1-row form measured 5.1 TB/s vs the 2-row gateup's 6.4)
    for (int row0 = (blockIdx.x * 4 + wid) * RW; row0 < N;
         row0 += gridDim.x * 4 * RW) {
        const uint32_t* wr[RW];
        bool live[RW];
#pragma unroll
        for (int rr_ = 0; rr_ < RW; ++rr_) {
            live[rr_] = row0 + rr_ < N;
            wr[rr_] = w + (size_t)(live[rr_] ? row0 + rr_ : row0) * k2;
        }
        float acc[RW][M];
#pragma unroll
        for (int rr_ = 0; rr_ < RW; ++rr_)
#pragma unroll
            for (int m = 0; m < M; ++m) acc[rr_][m] = 0.0f;
        gemv_row_pieces<M, NORM, RW, KU, XD>(acc, rstd, need_rstd, wr, x, wn, k2,
                                            lane, eps);
#pragma unroll
        for (int m = 0; m < M; ++m) {
#pragma unroll
            for (int rr_ = 0; rr_ < RW; ++rr_) {
                float v = wave_reduce_sum(acc[rr_][m]);
                if (lane == 0 && live[rr_]) {
                    if (ADDRES) {
                        v += bf16_to_f32(reinterpret_cast<const uint16_t*>(
                            res)[(size_t)m * N + row0 + rr_]);
                    }
                    reinterpret_cast<uint16_t*>(out)[(size_t)m * N + row0 + rr_] =
                        f32_to_bf16(v);
                }
            }
        }
    }
}

// Fused gate-up + SiLU GEMV for the MLP up-projection: the fused weight
// holds gate rows [0, I) and up rows [I, 2I); each wave computes BOTH rows
// r and I + r and writes act[m][r] = silu(gate) * up directly — the separate
// [1, 2I] intermediate and the silu_mul pass never materialize. The K
// pipeline is the two-row one above with (gate, up) as the row pair.
// (the M = 2 fused-norm form is held to the 6 waves per SIMD of its M = 2
// siblings; left alone the compiler spends 88 VGPRs on it)
template <int M, bool NORM, int KU = 1>
__global__ __launch_bounds__(256)
__attribute__((amdgpu_waves_per_eu(M == 2 && NORM && KU == 1 ? 6 : 1)))
void gemv_gateup_kernel(
    const uint32_t* __restrict__ x,  // [M, K/2]
    const uint32_t* __restrict__ w,  // [2I, K/2] (gate; up)
    uint32_t* __restrict__ out,      // [M, I] bf16
    const uint32_t* __restrict__ wn, // [K/2] rmsnorm weight (NORM only)
    int I, int k2, float eps) {
    constexpr int XD = M == 1 ? 4 : 2;
    const int lane = threadIdx.x & (WAVE - 1);
    const int wid = threadIdx.x / WAVE;

    float rstd[M];
#pragma unroll
    for (int m = 0; m < M; ++m) rstd[m] = 1.0f;
    bool need_rstd = NORM;
    if (NORM && M > 2) {  // depth-1 forms: the plain prologue, up front
#pragma unroll
        for (int m = 0; m < M; ++m) rstd[m] = row_rstd(x + (size_t)m * k2, k2, lane, eps);
        need_rstd = false;
    }

    for (int row = blockIdx.x * 4 + wid; row < I; row += gridDim.x * 4) {
        const uint32_t* wr[2];
        wr[0] = w + (size_t)row * k2;
        wr[1] = w + (size_t)(I + row) * k2;
        float acc[2][M];  // [0] gate, [1] up
#pragma unroll
        for (int m = 0; m < M; ++m) acc[0][m] = acc[1][m] = 0.0f;
        gemv_row_pieces<M, NORM, 2, KU, XD>(acc, rstd, need_rstd, wr, x, wn, k2,
                                           lane, eps);
#pragma unroll
        for (int m = 0; m < M; ++m) {
            const float g = wave_reduce_sum(acc[0][m]);
            const float u = wave_reduce_sum(acc[1][m]);
            if (lane == 0) {
                const float act = g / (1.0f + __expf(-g)) * u;
                reinterpret_cast<uint16_t*>(out)[(size_t)m * I + row] = f32_to_bf16(act);
            }
        }
    }
}

static bool gemv_bf16_use_mfma(int M, int K, int gateup);
extern "C" int oa_gemv_bf16_mfma(void* stream, const void* x, const void* w,
                                 void* out, const void* wn, const void* res,
                                 int M, int N, int K, float eps, int mode,
                                 int gateup);

// ---- K-depth dispatch (M <= 2, the decode hot path) -------------------------
// Depth per dispatch class and M, chosen by measurement at M = 1
// (scripts/gemv_depth_ab.py, then the in-model A/B; profiles/README.md
// "K-depth pipeline") under the register budget tests/test_gemv_resources.py
// gates: a depth must leave as many waves resident as the class's grid
// supplies. M = 2 takes the deepest form that fits the same budget. The
// M = 3..16 instantiations stay at depth 1: they exist for tests, not for the
// hot path. OPSAGENT_GEMV_KU_<CLASS> overrides a class for both M.
#define GEMV_KU_RW1_M1 8       // one row per wave, small N: o_proj, down
#define GEMV_KU_RW1_M2 8
#define GEMV_KU_RW1_NORM_M1 2  // the same with the fused norm: qkv
#define GEMV_KU_RW1_NORM_M2 2
#define GEMV_KU_RW2_M1 1       // two rows per wave: lm_head, 70B shapes
#define GEMV_KU_RW2_M2 1
#define GEMV_KU_RW2_NORM_M1 1
#define GEMV_KU_RW2_NORM_M2 1
#define GEMV_KU_GATEUP_M1 1    // (gate, up) row pair per wave
#define GEMV_KU_GATEUP_M2 1

// env override of a class's depth, 0 when unset or not one of 1/2/4/8
static int gemv_env_ku(const char* name) {
    const char* e = getenv(name);
    if (!e) return 0;
    const int v = atoi(e);
    return (v == 1 || v == 2 || v == 4 || v == 8) ? v : 0;
}

struct GemvArgs {
    hipStream_t stream;
    const uint32_t *x, *w;
    uint32_t* out;
    const uint32_t *wn, *res;
    int N, k2;  // gate-up: N holds I
    float eps;
    int grid;
};

template <int M, int RW, int KU>
static int gemv_launch_mode(const GemvArgs& a, int mode) {
#define LAUNCH_KU(NORMV, RESV)                                                 \
    hipLaunchKernelGGL((gemv_kernel<M, NORMV, RESV, RW, KU>), dim3(a.grid),    \
                       dim3(256), 0, a.stream, a.x, a.w, a.out, a.wn, a.res,   \
                       a.N, a.k2, a.eps)
    switch (mode) {
        case 0: LAUNCH_KU(false, false); break;
        case 1: LAUNCH_KU(true, false); break;
        case 2: LAUNCH_KU(false, true); break;
        case 3: LAUNCH_KU(true, true); break;
        default: return -102;
    }
#undef LAUNCH_KU
    return 0;
}

template <int M, int RW>
static int gemv_launch_ku(const GemvArgs& a, int mode, int ku) {
    switch (ku) {
        case 1: return gemv_launch_mode<M, RW, 1>(a, mode);
        case 2: return gemv_launch_mode<M, RW, 2>(a, mode);
        case 4: return gemv_launch_mode<M, RW, 4>(a, mode);
        case 8: return gemv_launch_mode<M, RW, 8>(a, mode);
        default: return -103;
    }
}

// M in {1, 2}, rw in {1, 2}, ku in {1, 2, 4, 8}
static int gemv_launch_m12(const GemvArgs& a, int M, int mode, int rw, int ku) {
    if (M == 1) return rw == 1 ? gemv_launch_ku<1, 1>(a, mode, ku)
                               : gemv_launch_ku<1, 2>(a, mode, ku);
    return rw == 1 ? gemv_launch_ku<2, 1>(a, mode, ku)
                   : gemv_launch_ku<2, 2>(a, mode, ku);
}

template <int M, int KU>
static void gemv_gateup_launch(const GemvArgs& a, int norm) {
    if (norm)
        hipLaunchKernelGGL((gemv_gateup_kernel<M, true, KU>), dim3(a.grid),
                           dim3(256), 0, a.stream, a.x, a.w, a.out, a.wn, a.N,
                           a.k2, a.eps);
    else
        hipLaunchKernelGGL((gemv_gateup_kernel<M, false, KU>), dim3(a.grid),
                           dim3(256), 0, a.stream, a.x, a.w, a.out, a.wn, a.N,
                           a.k2, a.eps);
}

template <int M>
static int gemv_gateup_launch_ku(const GemvArgs& a, int norm, int ku) {
    switch (ku) {
        case 1: gemv_gateup_launch<M, 1>(a, norm); break;
        case 2: gemv_gateup_launch<M, 2>(a, norm); break;
        case 4: gemv_gateup_launch<M, 4>(a, norm); break;
        case 8: gemv_gateup_launch<M, 8>(a, norm); break;
        default: return -103;
    }
    return 0;
}

// probe/test entry: gate-up at an explicit K depth (M <= 2, VALU kernel only)
extern "C" int oa_gemv_gateup_ku(void* stream, const void* x, const void* w,
                                 void* out, const void* wn, int M, int I, int K,
                                 float eps, int norm, int ku) {
    if (K % 8 != 0 || K < 8) return -100;
    if (M < 1 || M > 2 || I < 1) return -101;
    const GemvArgs a = {(hipStream_t)stream, (const uint32_t*)x, (const uint32_t*)w,
                        (uint32_t*)out, (const uint32_t*)wn, nullptr, I, K / 2, eps,
                        min(2048, CEIL_DIV(I, 4))};
    const int rc = M == 1 ? gemv_gateup_launch_ku<1>(a, norm, ku)
                          : gemv_gateup_launch_ku<2>(a, norm, ku);
    if (rc != 0) return rc;
    HIP_CHECK_LAUNCH();
    return 0;
}

extern "C" int oa_gemv_gateup_ex(void* stream, const void* x, const void* w,
                                 void* out, const void* wn, int M, int I, int K,
                                 float eps, int norm) {
    if (K % 8 != 0) return -100;
    if (gemv_bf16_use_mfma(M, K, 1))
        return oa_gemv_bf16_mfma(stream, x, w, out, wn, nullptr, M, 2 * I, K,
                                 eps, norm ? 1 : 0, 1);
    if (M <= 2) {
        static const int env_ku = gemv_env_ku("OPSAGENT_GEMV_KU_GATEUP");
        const int ku = env_ku ? env_ku
                              : (M == 1 ? GEMV_KU_GATEUP_M1 : GEMV_KU_GATEUP_M2);
        return oa_gemv_gateup_ku(stream, x, w, out, wn, M, I, K, eps, norm, ku);
    }
    const int k2 = K / 2;
    const int grid = min(2048, CEIL_DIV(I, 4));
#define LAUNCH_GU(MV)                                                          \
    do {                                                                       \
        if (norm)                                                              \
            hipLaunchKernelGGL((gemv_gateup_kernel<MV, true>), dim3(grid),     \
                               dim3(256), 0, (hipStream_t)stream,              \
                               (const uint32_t*)x, (const uint32_t*)w,         \
                               (uint32_t*)out, (const uint32_t*)wn, I, k2, eps);\
        else                                                                   \
            hipLaunchKernelGGL((gemv_gateup_kernel<MV, false>), dim3(grid),    \
                               dim3(256), 0, (hipStream_t)stream,              \
                               (const uint32_t*)x, (const uint32_t*)w,         \
                               (uint32_t*)out, (const uint32_t*)wn, I, k2, eps);\
    } while (0)
    switch (M) {
        case 3: LAUNCH_GU(3); break;
        case 4: LAUNCH_GU(4); break;
        case 5: LAUNCH_GU(5); break;
        case 6: LAUNCH_GU(6); break;
        case 7: LAUNCH_GU(7); break;
        case 8: LAUNCH_GU(8); break;
        case 12: LAUNCH_GU(12); break;
        case 16: LAUNCH_GU(16); break;
        default: return -101;
    }
#undef LAUNCH_GU
    HIP_CHECK_LAUNCH();
    return 0;
}

extern "C" int oa_gemv_gateup(void* stream, const void* x, const void* w,
                              void* out, int M, int I, int K) {
    return oa_gemv_gateup_ex(stream, x, w, out, nullptr, M, I, K, 0.0f, 0);
}

// probe/test entry: plain/norm/residual GEMV at an explicit rows-per-wave and
// K depth (M <= 2, VALU kernel only; same grids as the dispatcher)
extern "C" int oa_gemv_ku(void* stream, const void* x, const void* w, void* out,
                          const void* wn, const void* res, int M, int N, int K,
                          float eps, int mode, int rw, int ku) {
    if (K % 8 != 0 || K < 8) return -100;
    if (M < 1 || M > 2 || N < 1) return -101;
    if (rw != 1 && rw != 2) return -104;
    const GemvArgs a = {(hipStream_t)stream, (const uint32_t*)x, (const uint32_t*)w,
                        (uint32_t*)out, (const uint32_t*)wn, (const uint32_t*)res,
                        N, K / 2, eps, min(2048, CEIL_DIV(N, 4 * rw))};
    const int rc = gemv_launch_m12(a, M, mode, rw, ku);
    if (rc != 0) return rc;
    HIP_CHECK_LAUNCH();
    return 0;
}

// mode: 0 plain, 1 norm-prologue, 2 residual-add epilogue, 3 both
extern "C" int oa_gemv_ex(void* stream, const void* x, const void* w, void* out,
                          const void* wn, const void* res, int M, int N, int K,
                          float eps, int mode) {
    if (K % 8 != 0) return -100;
    if (gemv_bf16_use_mfma(M, K, 0))
        return oa_gemv_bf16_mfma(stream, x, w, out, wn, res, M, N, K, eps,
                                 mode, 0);
    const int k2 = K / 2;
    // 4 rows/wave won +3-6% in the ISOLATED probe on wide outputs
    // (scripts/gemv_ab.py) but lost 3% in-model (decode step 3.63 -> 3.75 ms,
    // within-box A/B) — real decode interleaves the W stream with KV/L2
    // traffic the probe does not. Default OFF; OPSAGENT_GEMV_RW4_MIN_N
    // re-enables for experiments.
    static int rw4_min_n = -1;
    static int rw1_max_n = -1;
    static int env_rw1 = 0, env_rw1n = 0, env_rw2 = 0, env_rw2n = 0;
    if (rw4_min_n < 0) {
        // K depth per class (see GEMV_KU_*); env overrides for experiments
        env_rw1 = gemv_env_ku("OPSAGENT_GEMV_KU_RW1");
        env_rw1n = gemv_env_ku("OPSAGENT_GEMV_KU_RW1_NORM");
        env_rw2 = gemv_env_ku("OPSAGENT_GEMV_KU_RW2");
        env_rw2n = gemv_env_ku("OPSAGENT_GEMV_KU_RW2_NORM");
        // RW=1 for small-N outputs: at N=4096 the RW=2 grid is only 512
        // workgroups (2 per CU — half the SIMD slots idle); one row per wave
        // doubles the wave count and the streams in flight. In-model A/B
        // (8B turn, same box): off 438.1 ms, N<=6144 431.0 ms, N<=4096
        // 431.9 ms — default N<=6144 (covers o_proj and the fused-norm qkv).
        const char* e1 = getenv("OPSAGENT_GEMV_RW1_MAX_N");
        rw1_max_n = e1 ? atoi(e1) : 6144;
        const char* e = getenv("OPSAGENT_GEMV_RW4_MIN_N");
        rw4_min_n = e ? atoi(e) : (1 << 30);
    }
    const bool rw4 = N >= rw4_min_n;
    const bool rw1 = !rw4 && N <= rw1_max_n;
    if (M <= 2 && !rw4) {
        const bool norm = mode & 1, m1 = M == 1;
        int ku;
        if (rw1 && !norm) ku = env_rw1 ? env_rw1 : (m1 ? GEMV_KU_RW1_M1 : GEMV_KU_RW1_M2);
        else if (rw1) ku = env_rw1n ? env_rw1n : (m1 ? GEMV_KU_RW1_NORM_M1 : GEMV_KU_RW1_NORM_M2);
        else if (!norm) ku = env_rw2 ? env_rw2 : (m1 ? GEMV_KU_RW2_M1 : GEMV_KU_RW2_M2);
        else ku = env_rw2n ? env_rw2n : (m1 ? GEMV_KU_RW2_NORM_M1 : GEMV_KU_RW2_NORM_M2);
        return oa_gemv_ku(stream, x, w, out, wn, res, M, N, K, eps, mode,
                          rw1 ? 1 : 2, ku);
    }
    const int grid = min(2048, CEIL_DIV(N, rw4 ? 16 : (rw1 ? 4 : 8)));
#define LAUNCH_NM(MV, NORMV, RESV)                                            \
    do {                                                                       \
        if (rw4)                                                               \
            hipLaunchKernelGGL((gemv_kernel<MV, NORMV, RESV, 4>), dim3(grid),  \
                               dim3(256), 0, (hipStream_t)stream,              \
                               (const uint32_t*)x, (const uint32_t*)w,         \
                               (uint32_t*)out, (const uint32_t*)wn,            \
                               (const uint32_t*)res, N, k2, eps);              \
        else if (rw1)                                                          \
            hipLaunchKernelGGL((gemv_kernel<MV, NORMV, RESV, 1>), dim3(grid),  \
                               dim3(256), 0, (hipStream_t)stream,              \
                               (const uint32_t*)x, (const uint32_t*)w,         \
                               (uint32_t*)out, (const uint32_t*)wn,            \
                               (const uint32_t*)res, N, k2, eps);              \
        else                                                                   \
            hipLaunchKernelGGL((gemv_kernel<MV, NORMV, RESV, 2>), dim3(grid),  \
                               dim3(256), 0, (hipStream_t)stream,              \
                               (const uint32_t*)x, (const uint32_t*)w,         \
                               (uint32_t*)out, (const uint32_t*)wn,            \
                               (const uint32_t*)res, N, k2, eps);              \
    } while (0)
#define LAUNCH_MODE(MV)                                                        \
    do {                                                                       \
        switch (mode) {                                                        \
            case 0: LAUNCH_NM(MV, false, false); break;                        \
            case 1: LAUNCH_NM(MV, true, false); break;                         \
            case 2: LAUNCH_NM(MV, false, true); break;                         \
            case 3: LAUNCH_NM(MV, true, true); break;                          \
            default: return -102;                                              \
        }                                                                      \
    } while (0)
    switch (M) {
        case 1: LAUNCH_MODE(1); break;
        case 2: LAUNCH_MODE(2); break;
        case 3: LAUNCH_MODE(3); break;
        case 4: LAUNCH_MODE(4); break;
        case 5: LAUNCH_MODE(5); break;
        case 6: LAUNCH_MODE(6); break;
        case 7: LAUNCH_MODE(7); break;
        case 8: LAUNCH_MODE(8); break;
        case 12: LAUNCH_MODE(12); break;
        case 16: LAUNCH_MODE(16); break;
        default: return -101;
    }
#undef LAUNCH_MODE
#undef LAUNCH_NM
    HIP_CHECK_LAUNCH();
    return 0;
}

extern "C" int oa_gemv(void* stream, const void* x, const void* w, void* out,
                       int M, int N, int K) {
    return oa_gemv_ex(stream, x, w, out, nullptr, nullptr, M, N, K, 0.0f, 0);
}

// RW=4 probe variant (within-probe A/B only — guide rule 24)
extern "C" int oa_gemv_rw4(void* stream, const void* x, const void* w, void* out,
                           int M, int N, int K) {
    if (K % 8 != 0) return -100;
    const int k2 = K / 2;
    const int grid = min(2048, CEIL_DIV(N, 16));
    switch (M) {
        case 1:
            hipLaunchKernelGGL((gemv_kernel<1, false, false, 4>), dim3(grid),
                               dim3(256), 0, (hipStream_t)stream,
                               (const uint32_t*)x, (const uint32_t*)w,
                               (uint32_t*)out, nullptr, nullptr, N, k2, 0.0f);
            break;
        default:
            return -101;
    }
    HIP_CHECK_LAUNCH();
    return 0;
}

// ---- MFMA bf16 GEMV (batched decode, M 2..16) ------------------------------
// The VALU kernels win at M <= 2 but their per-element M-loop turns
// compute-bound as the batch grows, and hipBLASLt's skinny kernels (the old
// M > 2 fallback) run ~2.5x off the stream roofline — concurrent decode
// (c=8/16) measured ~2 TB/s effective. Same architecture as the fp8 MFMA
// GEMV (fp8_moe.hip): x staged ONCE into LDS (norm applied in fp32 at stage
// time), each of the block's four waves streams 16 W rows over a quarter of
// K straight into v_mfma_f32_16x16x32_bf16 A-fragments with a PF-deep
// register prefetch ring, partial D tiles meet in LDS. The 16 B columns
// carry the batch — M up to 16 rides one weight stream.
typedef __attribute__((ext_vector_type(8))) short bf16x8g;
typedef __attribute__((ext_vector_type(4))) float f32x4g;

template <bool NORM, bool ADDRES, bool GATEUP>
__global__ __launch_bounds__(256, 1) void gemv_bf16_mfma_kernel(
    const uint32_t* __restrict__ x,   // [M, K/2] bf16x2
    const uint32_t* __restrict__ w,   // [N, K/2] (gateup: [2I, K/2])
    uint32_t* __restrict__ out,       // [M, N] bf16 (gateup: [M, I])
    const uint32_t* __restrict__ wn,  // [K/2] rmsnorm weight (NORM)
    const uint32_t* __restrict__ res, // [M, N] residual (ADDRES)
    int M, int N, int K, float eps) {
    constexpr int PF = GATEUP ? 4 : 8;
    const int tid = threadIdx.x;
    const int lane = tid & (WAVE - 1);
    const int wid = tid / WAVE;
    const int fr = lane & 15;   // A row / B,D col
    const int fs = lane >> 4;   // 8-element k-slice; D rows fs*4..+3
    const int rows = GATEUP ? N / 2 : N;
    const int I = rows;
    const int row0 = blockIdx.x * 16;
    const int wrow = min(row0 + fr, rows - 1);
    const int k2 = K / 2;

    extern __shared__ __attribute__((aligned(16))) char xls[];
    const int pitch = K * 2 + 16;  // bytes; pad de-banks the batch rows

    // stage x (wave w handles batch rows m ≡ w mod 4), norm folded in fp32
    for (int m = wid; m < M; m += 4) {
        const uint32_t* xr = x + (size_t)m * k2;
        uint32_t* dst = reinterpret_cast<uint32_t*>(xls + (size_t)m * pitch);
        float rstd = 1.0f;
        if (NORM) rstd = row_rstd(xr, k2, lane, eps);
        for (int i = lane * 4; i < k2; i += WAVE * 4) {
            uint4 v = *reinterpret_cast<const uint4*>(xr + i);
            if (NORM) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const uint32_t g = wn[i + j];
                    const float lo = bf16_lo((&v.x)[j]) * rstd * bf16_lo(g);
                    const float hi = bf16_hi((&v.x)[j]) * rstd * bf16_hi(g);
                    (&v.x)[j] = (uint32_t)f32_to_bf16(lo) |
                                ((uint32_t)f32_to_bf16(hi) << 16);
                }
            }
            *reinterpret_cast<uint4*>(dst + i) = v;
        }
    }
    __syncthreads();

    const int ke = K / 4;               // elements per wave
    const int k0b = wid * ke * 2;       // byte offset of this wave's range
    const int nk = ke / 32;             // 32-element MFMA steps
    const char* wp = reinterpret_cast<const char*>(w);
    const uint32_t* wr0 = reinterpret_cast<const uint32_t*>(
        wp + (size_t)wrow * K * 2 + k0b) + fs * 4;
    const uint32_t* wr1 = reinterpret_cast<const uint32_t*>(
        wp + (size_t)(wrow + (GATEUP ? I : 0)) * K * 2 + k0b) + fs * 4;
    const int mrow = fr < M ? fr : 0;
    const char* xrw = xls + (size_t)mrow * pitch + k0b + fs * 16;

    f32x4g acc0 = {}, acc1 = {};
    uint4 abuf[PF], ubuf[GATEUP ? PF : 1];
    auto load_a = [&](int p, int kb) {
        u32x4 t = nt_load4(wr0 + kb * 16);
        abuf[p] = *reinterpret_cast<uint4*>(&t);
        if (GATEUP) {
            u32x4 t2 = nt_load4(wr1 + kb * 16);
            ubuf[p] = *reinterpret_cast<uint4*>(&t2);
        }
    };
#pragma unroll
    for (int p = 0; p < PF; ++p) load_a(p, p);
    // x fragment double-buffered ONE step ahead: an inline ds_read feeding
    // its own MFMA serializes on lgkmcnt(0) every step (measured in the .s)
    uint4 bcur = *reinterpret_cast<const uint4*>(xrw);
    for (int kb0 = 0; kb0 < nk; kb0 += PF) {
        const bool more = kb0 + PF < nk;
#pragma unroll
        for (int p = 0; p < PF; ++p) {
            const int kb = kb0 + p;
            uint4 bnext;
            if (kb + 1 < nk)
                bnext = *reinterpret_cast<const uint4*>(xrw + (kb + 1) * 64);
            acc0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                *reinterpret_cast<bf16x8g*>(&abuf[p]),
                *reinterpret_cast<bf16x8g*>(&bcur), acc0, 0, 0, 0);
            if (GATEUP)
                acc1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                    *reinterpret_cast<bf16x8g*>(&ubuf[p]),
                    *reinterpret_cast<bf16x8g*>(&bcur), acc1, 0, 0, 0);
            if (more) load_a(p, kb0 + PF + p);
            if (kb + 1 < nk) bcur = bnext;
        }
    }

    // intra-block reduction: [wave][plane][col fr][row fs*4+i] f32 in LDS
    __syncthreads();  // x reads done before the tiles overwrite the image
    float* red = reinterpret_cast<float*>(xls);
    const int planes = GATEUP ? 2 : 1;
    {
        float* t = red + ((wid * planes) * 16 + fr) * 16 + fs * 4;
        *reinterpret_cast<f32x4g*>(t) = acc0;
        if (GATEUP) *reinterpret_cast<f32x4g*>(t + 16 * 16) = acc1;
    }
    __syncthreads();
    if (wid != 0 || fr >= M) return;
    const int m = fr;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int row = row0 + fs * 4 + i;
        if (row >= rows) continue;
        float sg = 0.0f, su = 0.0f;
#pragma unroll
        for (int wv = 0; wv < 4; ++wv) {
            sg += red[((wv * planes) * 16 + m) * 16 + fs * 4 + i];
            if (GATEUP)
                su += red[((wv * planes + 1) * 16 + m) * 16 + fs * 4 + i];
        }
        float v;
        if (GATEUP) {
            v = sg / (1.0f + __expf(-sg)) * su;
        } else {
            v = sg;
            if (ADDRES)
                v += bf16_to_f32(reinterpret_cast<const uint16_t*>(
                    res)[(size_t)m * rows + row]);
        }
        reinterpret_cast<uint16_t*>(out)[(size_t)m * rows + row] =
            f32_to_bf16(v);
    }
}

// eligibility shared by the C dispatch and its callers; must mirror the
// kernel's constraints so ineligible shapes FALL BACK, never error
static bool gemv_bf16_use_mfma(int M, int K, int gateup) {
    const char* e = getenv("OPSAGENT_BF16_GEMV_MFMA");
    if (e && e[0] == '0') return false;
    int min_m = 3;  // VALU kernels keep the measured M<=2 regime
    if (e && e[0] == 'm') min_m = atoi(e + 1);
    if (M < min_m || M > 16) return false;
    if (K % (gateup ? 512 : 1024) != 0) return false;
    // A/B-measured win region (scripts/gemv_bf16_mfma_ab.py): +29..+83%
    // at the 8B-class K<=6144 shapes; hipBLASLt keeps deep-K (70B qkv
    // K=8192 5.56 TB/s vs 3.21; 8B down K=14336 a wash) and the M=16
    // gateup (131 KiB x-image halves block occupancy). Env 'm<N>' widens
    // for experiments.
    if (!(e && e[0] == 'm')) {
        // engine A/B at c16 (same box): the M 9..16 forms LOSE ~7% end to
        // end even though the M16 microbench won — cap at the regime both
        // agree on (M <= 8, K <= 6144)
        if (K > 6144 || M > 8) return false;
    }
    const size_t img = (size_t)M * (K * 2 + 16);
    return img <= 147456;
}

extern "C" int oa_gemv_bf16_mfma(void* stream, const void* x, const void* w,
                                 void* out, const void* wn, const void* res,
                                 int M, int N, int K, float eps, int mode,
                                 int gateup) {
    const int rows = gateup ? N / 2 : N;
    const size_t img = (size_t)M * (K * 2 + 16);
    const size_t red = (size_t)(gateup ? 2 : 1) * 4 * 16 * 16 * 4;
    const size_t shmem = img > red ? img : red;
    dim3 grid(CEIL_DIV(rows, 16)), block(256);
#define LAUNCH_BMF(NORMV, RESV, GUV)                                           \
    hipLaunchKernelGGL((gemv_bf16_mfma_kernel<NORMV, RESV, GUV>), grid, block, \
                       shmem, (hipStream_t)stream, (const uint32_t*)x,         \
                       (const uint32_t*)w, (uint32_t*)out,                     \
                       (const uint32_t*)wn, (const uint32_t*)res, M, N, K, eps)
    if (gateup) {
        if (mode & 1) LAUNCH_BMF(true, false, true);
        else LAUNCH_BMF(false, false, true);
    } else {
        switch (mode) {
            case 0: LAUNCH_BMF(false, false, false); break;
            case 1: LAUNCH_BMF(true, false, false); break;
            case 2: LAUNCH_BMF(false, true, false); break;
            case 3: LAUNCH_BMF(true, true, false); break;
            default: return -102;
        }
    }
#undef LAUNCH_BMF
    HIP_CHECK_LAUNCH();
    return 0;
}
