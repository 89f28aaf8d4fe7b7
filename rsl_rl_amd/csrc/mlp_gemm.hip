// fp32 MFMA GEMMs with fused epilogues for the actor/critic MLP.
//
// Replaces, for the hidden layers of rsl_rl/networks/mlp.py:106-114 (nn.Linear + ELU), the three
// kernels torch runs per layer and direction -- GEMM, ELU, and in backward ELU' plus the bias-grad
// reduction -- with one kernel each:
//   linear_fwd   Y = act(X W^T + b)                 (act = identity | ELU, alpha 1)
//   linear_dgrad dZp = (dZ W) * ELU'(H)             (H = this layer's input = previous ELU output)
//                + per-tile column sums of dZp      (bias gradient of the previous layer)
// The pre-activation never reaches HBM in forward, dH never reaches HBM in backward.  The weight
// gradients stay split-K batched GEMMs (networks/linear.py).
//
// Exact fp32 arithmetic on v_mfma_f32_32x32x2_f32 (a k-ordered f32 fma chain, MI355X_MICROARCH.md);
// the k order inside a 4-deep group differs from a plain GEMM, i.e. rounding differs at fp32 epsilon.
//
// Tile: 128 rows x 256 columns per 512-thread workgroup (8 waves as 2 (M) x 4 (N), each wave 64 x 64 =
// 2 x 2 MFMA tiles), K staged in 16-deep chunks through double-buffered LDS (rows padded to 18 floats:
// the 8-byte operand reads of 32 lanes hit 32 distinct bank pairs).  For a k-group of 4 each lane reads
// A[i][4t + 2h .. +1] and B[j][4t + 2h .. +1] with one ds_read_b64 each and feeds two MFMA k-steps
// (step 2t uses k = 4t + 2h, step 2t+1 uses k = 4t + 2h + 1 -- the same mapping for A and B).
//
// This unit: the f32 kernel, the x6 / h3 kernels instantiated from mlp_gemm_x6.h with their pair forms, the opt-in
// 16x16x32 ("x6s"), "w4" and "w8" forms, and the two entry points rslrl_linear_gemm / rslrl_linear_gemm_pair with the
// validator.  The fused last hidden + output layer (RSLRL_LINEAR_FWD_OUT, the value and actor heads) is mlp_heads.hip,
// the output-layer backward mlp_out_bwd.hip, the images mlp_image.hip.  The fp32 kernel above is the f32 arithmetic of
// the same ops; x6 (the default) and h3 are described in mlp_gemm_x6.h.

#include <cstdlib>
#include <string>
#include <type_traits>

#include "common.h"
#include "fwd_stream.h"
#include "mlp_gemm_x6.h"

namespace rslrl {
namespace {

constexpr int kPad = 2;
constexpr int kLd = kKC + kPad;  // LDS row stride (floats)

// global -> registers for one K chunk: A: 128 x 16 floats = 512 float4 (1 per thread); B: 256 x 16 = 1024
// float4 (2 per thread, only the first N rows real).  Rows >= M / N and k >= K read as zero.
struct Stage {
    float4 a, b0, b1;
};

__device__ __forceinline__ Stage load_chunk(const GemmParams& p, int64_t row0, int k0) {
    const int t = threadIdx.x;
    const int k = k0 + 4 * (t & 3);
    const bool k_ok = k < p.K;
    Stage s;
    const int r = t >> 2;  // 0..127
    const int64_t row = row0 + r;
    const bool row_ok = row < p.M;
    s.a = load4_masked(p.a + (row_ok ? row : row0) * p.K, row_ok && k_ok, k);
    const int n0 = r, n1 = r + 128;
    s.b0 = load4_masked(p.bw + static_cast<int64_t>(n0 < p.N ? n0 : 0) * p.K, n0 < p.N && k_ok, k);
    s.b1 = load4_masked(p.bw + static_cast<int64_t>(n1 < p.N ? n1 : 0) * p.K, n1 < p.N && k_ok, k);
    return s;
}

__device__ __forceinline__ void store_chunk(const Stage& s, float* __restrict__ a_lds, float* __restrict__ b_lds) {
    const int t = threadIdx.x;
    const int q = t & 3;
    const int r = t >> 2;
    float2* pa = reinterpret_cast<float2*>(a_lds + r * kLd + 4 * q);
    pa[0] = make_float2(s.a.x, s.a.y);
    pa[1] = make_float2(s.a.z, s.a.w);
    float2* pb0 = reinterpret_cast<float2*>(b_lds + r * kLd + 4 * q);
    pb0[0] = make_float2(s.b0.x, s.b0.y);
    pb0[1] = make_float2(s.b0.z, s.b0.w);
    float2* pb1 = reinterpret_cast<float2*>(b_lds + (r + 128) * kLd + 4 * q);
    pb1[0] = make_float2(s.b1.x, s.b1.y);
    pb1[1] = make_float2(s.b1.z, s.b1.w);
}

// f32 kernel epilogue: 128-row tile, waves 2 (m) x 4 (n) of 64 x 64; column sums over the tile's 128 rows
// (lanes l and l+32 hold the two row halves, the two wm waves the two 64-row halves; fixed combine order)
// -> colsum[col][blockIdx.x].  colred: 2 x kBN floats of LDS the caller no longer reads.
template <int EPI>
__device__ __forceinline__ void epilogue(const GemmParams& p, f32x16 (&acc)[2][2], int64_t row0, float* colred) {
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int wm = wave >> 2;
    const int wn = wave & 3;
    const int h = lane >> 5;
    const int l32 = lane & 31;
    const bool full = (row0 + kBM <= p.M) && (p.N == kBN);  // wave-uniform: no per-element bounds checks
    float colpart[2];
    float amx = 0.f;
    epilogue_tiles<EPI, 2, 2>(p, acc, row0 + wm * 64, wn * 64, full, colpart, amx);
    if constexpr (EPI == kEpiEluGrad) {
        __syncthreads();  // the LDS tiles are no longer read
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const float s = colpart[j] + __shfl_xor(colpart[j], 32, 64);
            if (h == 0) colred[wm * kBN + wn * 64 + j * 32 + l32] = s;
        }
        __syncthreads();
        // tile-major partials [tiles][N]: one contiguous row per workgroup (column-major rows of 4-byte
        // pieces scattered over the whole buffer cost a read-modify-write of a line each)
        for (int col = threadIdx.x; col < p.N && col < kBN; col += kThreads)
            p.colsum[static_cast<int64_t>(blockIdx.x) * p.N + col] = colred[col] + colred[kBN + col];
    }
}

// MINW = minimum waves per SIMD the register allocation must allow (4: two workgroups per CU, <= 128
// VGPRs; 2: one workgroup per CU, <= 256 VGPRs).
template <int EPI, int MINW>
__global__ __launch_bounds__(kThreads, MINW) void mlp_gemm_kernel(GemmParams p) {
    __shared__ __attribute__((aligned(16))) float lds[2][(kBM + kBN) * kLd];
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int wm = wave >> 2;  // 0..1 -> rows wm*64
    const int wn = wave & 3;   // 0..3 -> cols wn*64
    const int h = lane >> 5;
    const int l32 = lane & 31;
    const int64_t row0 = static_cast<int64_t>(blockIdx.x) * kBM;

    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = f32x16{};

    const int nchunks = (p.K + kKC - 1) / kKC;
    Stage st = load_chunk(p, row0, 0);
    store_chunk(st, lds[0], lds[0] + kBM * kLd);
    __syncthreads();
    for (int c = 0; c < nchunks; ++c) {
        const int buf = c & 1;
        const bool more = c + 1 < nchunks;
        if (more) st = load_chunk(p, row0, (c + 1) * kKC);  // in flight during this chunk's MFMAs
        const float* a_lds = lds[buf];
        const float* b_lds = lds[buf] + kBM * kLd;
#pragma unroll
        for (int t = 0; t < kKC / 4; ++t) {
            float2 av[2], bv[2];
#pragma unroll
            for (int i = 0; i < 2; ++i)
                av[i] = *reinterpret_cast<const float2*>(a_lds + (wm * 64 + i * 32 + l32) * kLd + 4 * t + 2 * h);
#pragma unroll
            for (int j = 0; j < 2; ++j)
                bv[j] = *reinterpret_cast<const float2*>(b_lds + (wn * 64 + j * 32 + l32) * kLd + 4 * t + 2 * h);
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[i].x, bv[j].x, acc[i][j], 0, 0, 0);
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[i].y, bv[j].y, acc[i][j], 0, 0, 0);
                }
        }
        if (more) {
            // the other buffer was last read in chunk c-1, and every wave passed the barrier after it
            store_chunk(st, lds[buf ^ 1], lds[buf ^ 1] + kBM * kLd);
        }
        __syncthreads();
    }
    epilogue<EPI>(p, acc, row0, lds[0]);
}

// the K = 48 kernel applies to full tiles of a forward on x6 operands with the deep loop enabled
template <int EPI>
bool k48_deep(const GemmParams& p, bool fullm, int pl) {
    return (EPI == kEpiBias || EPI == kEpiBiasElu) && pl == 3 && fullm && p.K == 3 * kKC && p.deep;
}

template <int EPI, bool FULL, int PL, int KCH = 0, bool STAGE = false>
__global__ __launch_bounds__(kThreads, 4) void mlp_gemm_x6_pair_kernel(GemmPair b) {
    __shared__ __attribute__((aligned(16))) char lds_b0[x6_buf_bytes<EPI, PL>()];
    __shared__ __attribute__((aligned(16))) char lds_b1[x6_buf_bytes<EPI, PL>()];
    const int y = blockIdx.y;
    mlp_gemm_x6_body<EPI, FULL, 4, PL, STAGE, KCH>(b.p[y], b.img[y], lds_b0, lds_b1);
}

// ---- the same x6 GEMM on v_mfma_f32_16x16x32_bf16 ("paired" x6).  Under load the chip holds a higher
// clock on the 16x16x32 shape than on 32x32x16 at equal cycles per FLOP (MI355X_MICROARCH.md, DVFS
// give-back item 7).  Its k = 32 is spent on two plane products of the same 16-deep chunk: lanes 0-31
// carry the first product of a pair, lanes 32-63 the second (a dot product does not care which lanes
// hold which k), so three MFMAs per 16x16 tile and chunk accumulate, smallest terms first,
//   P1 = a0b2 + a2b0,  P2 = a1b1 + a0b1,  P3 = a1b0 + a0b0.
// A fragments: P1 reads plane (0 | 2), P2 and P3 share plane (1 | 0); B fragments: (2 | 0), 1, 0.  Lane l
// reads row (l & 15) of its 16-row block, k half (l >> 4) & 1 -- each 16-lane group covers all 64 banks
// through the same row-half swizzle, so the LDS image and its staging are the 32x32x16 kernel's.
// The MFMAs take the weight fragment as their A operand and the activation fragment as B, so they
// produce C^T tiles: lane l holds row (l & 15) of its 16-row block and the four consecutive columns
// 4 (l >> 4) .. +3 of its 16-column block -> 16-byte stores and h loads in the epilogue.  Wave tile 64 x 64.
__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }

template <int EPI, bool FULLT, bool NT>
__device__ __forceinline__ void epilogue16_impl(const GemmParams& p, f32x4 (&acc)[4][4], int64_t wrow0, int wcol0,
                                                f32x4 (&colpart)[4]) {
    constexpr bool full = FULLT;
    constexpr bool GRAD = EPI == kEpiEluGrad;
    const int lane = threadIdx.x & 63;
    const int l16 = lane & 15;
    const int cq = 4 * (lane >> 4);
#pragma unroll
    for (int j = 0; j < 4; ++j) colpart[j] = f32x4{};
    f32x4 bias[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int col = wcol0 + 16 * j + cq;  // N % 4 == 0 (launch)
        bias[j] = f32x4{};
        if constexpr (!GRAD) {
            if (col < p.N) {
                const float4 b = ld4(p.bias + col);
                bias[j] = f32x4{b.x, b.y, b.z, b.w};
            }
        }
    }
    // h of row block i (4 column quads), loaded at the block's start: a prefetch of block i + 1 would
    // push the 128-register allocation into scratch
    f32x4 hcur[4];
    auto load_h = [&](int i, f32x4 (&dst)[4]) {
        const int64_t row = wrow0 + 16 * i + l16;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int col = wcol0 + 16 * j + cq;
            dst[j] = f32x4{};
            if (full || (row < p.M && col < p.N)) {
                const float4 v = ld4(p.h + row * p.N + col);
                dst[j] = f32x4{v.x, v.y, v.z, v.w};
            }
        }
    };
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if constexpr (GRAD) load_h(i, hcur);
        const int64_t row = wrow0 + 16 * i + l16;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int col = wcol0 + 16 * j + cq;
            f32x4 v = acc[i][j];
            if constexpr (EPI == kEpiBias) {
                v = v + bias[j];
            } else if constexpr (EPI == kEpiBiasElu) {
                v = v + bias[j];
#pragma unroll
                for (int r = 0; r < 4; ++r) v[r] = v[r] > 0.f ? v[r] : elu_neg(v[r]);
            } else {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float hv = hcur[j][r];
                    v[r] = hv > 0.f ? v[r] : v[r] * (hv + 1.f);
                }
            }
            if (full || (row < p.M && col < p.N)) {
                if constexpr (GRAD) colpart[j] = colpart[j] + v;
                f32x4* dst = reinterpret_cast<f32x4*>(p.c + row * p.N + col);
                if constexpr (NT) __builtin_nontemporal_store(v, dst);
                else *dst = v;
            }
        }
    }
}

template <int EPI, bool FULL, int MINW, bool NT>
__global__ __launch_bounds__(kThreads, MINW) void mlp_gemm_x6s_kernel(GemmParams p, const uint4* __restrict__ bimg) {
    constexpr int BM = kBM;
    constexpr int planeA = BM * kX6RowB;
    constexpr int bufBytes = 3 * planeA + kX6ChunkB;
    static_assert(EPI == kEpiBias || EPI == kEpiBiasElu || EPI == kEpiEluGrad, "no fused weight gradient here");
    __shared__ __attribute__((aligned(16))) char lds[2][bufBytes];
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int wm = wave >> 2;  // rows wm * 64
    const int wn = wave & 3;   // cols wn * 64
    const int hs = lane >> 5;          // which product of a pair
    const int hk = (lane >> 4) & 1;    // k half of the chunk
    const int l16 = lane & 15;
    const int64_t row0 = static_cast<int64_t>(blockIdx.x) * BM;
    const int offA0 = (hs ? 2 : 0) * planeA;     // P1: a0 | a2
    const int offA1 = (hs ? 0 : 1) * planeA;     // P2, P3: a1 | a0
    const int offB0 = (hs ? 0 : 2) * kX6PlaneB;  // P1: b2 | b0

    f32x4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{};

    // one chunk's fragments and MFMAs (a_lds / b_lds: the chunk's A planes and B image in LDS)
    auto compute = [&](const char* a_lds, const char* b_lds) {
        bf16x8 af[4][2];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int row = wm * 64 + 16 * i + l16;
            af[i][0] = read_frag(a_lds + offA0, row, hk);
            af[i][1] = read_frag(a_lds + offA1, row, hk);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int col = wn * 64 + 16 * j + l16;
            const bf16x8 b0 = read_frag(b_lds + offB0, col, hk);
            const bf16x8 b1 = read_frag(b_lds + kX6PlaneB, col, hk);
            const bf16x8 b2 = read_frag(b_lds, col, hk);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(b0, af[i][0], acc[i][j], 0, 0, 0);
                acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(b1, af[i][1], acc[i][j], 0, 0, 0);
                acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(b2, af[i][1], acc[i][j], 0, 0, 0);
            }
        }
    };
    bool deep = false;
    if constexpr (FULL) {
        if (p.K == 16 * kKC && p.deep) {  // the unrolled look-ahead pipeline (K = 256)
            char* ldsp[2] = {lds[0], lds[1]};
            deep_pipeline<BM, 3, 16, kX6Depth>(p, row0, bimg, ldsp, 1.f, compute);
            deep = true;
        }
    }
    const int nchunks = deep ? 0 : (p.K + kKC - 1) / kKC;
    if (!deep) {
    load_b_lds<3>(bimg, 0, lds[0] + 3 * planeA);
    store_a_split<BM, 3>(load_a<BM, FULL>(p, row0, 0), lds[0], 1.f);
    __syncthreads();
    for (int c = 0; c < nchunks; ++c) {
        const int buf = c & 1;
        const bool more = c + 1 < nchunks;
        AStage<BM> an;
        if (more) {
            load_b_lds<3>(bimg, c + 1, lds[buf ^ 1] + 3 * planeA);
            an = load_a<BM, FULL>(p, row0, (c + 1) * kKC);
        }
        compute(lds[buf], lds[buf] + 3 * planeA);
        if (more) store_a_split<BM, 3>(an, lds[buf ^ 1], 1.f);
        __syncthreads();
    }
    }  // !deep

    const bool full = (row0 + BM <= p.M) && (p.N == kBN);
    f32x4 colpart[4];
    if (full)
        epilogue16_impl<EPI, true, NT>(p, acc, row0 + wm * 64, wn * 64, colpart);
    else
        epilogue16_impl<EPI, false, NT>(p, acc, row0 + wm * 64, wn * 64, colpart);
    if constexpr (EPI == kEpiEluGrad) {
        // column sums over the tile's 128 rows: the 16 lanes of a group hold 16 rows of the same columns
        // (butterfly over lane bits 0-3, a fixed order), the two wave rows (wm) are combined through LDS
#pragma unroll
        for (int m = 1; m < 16; m <<= 1)
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r) colpart[j][r] += __shfl_xor(colpart[j][r], m, 64);
        float* colred = reinterpret_cast<float*>(lds[0]);
        __syncthreads();  // the LDS tiles are no longer read
        if ((lane & 15) == 0) {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                *reinterpret_cast<f32x4*>(colred + wm * kBN + wn * 64 + 16 * j + 4 * (lane >> 4)) = colpart[j];
        }
        __syncthreads();
        for (int col = threadIdx.x; col < p.N && col < kBN; col += kThreads)
            p.colsum[static_cast<int64_t>(blockIdx.x) * p.N + col] = colred[col] + colred[kBN + col];
    }
}

// tuning knob: RSLRL_X6S_NT=0|1 (default 0): streaming stores in the 16x16 epilogue.  Its 64-byte row
// pieces are better served by ordinary stores (K=48 forward 126 vs 159 us; the 32x32 epilogue writes whole
// 128-byte lines per instruction and gains from streaming stores instead)
bool x6s_nontemporal() {
    static const bool v = [] {
        const char* e = std::getenv("RSLRL_X6S_NT");
        return e && std::atoi(e) == 1;
    }();
    return v;
}

// tuning knob: RSLRL_X6_SHAPE=16|32 (default 32): MFMA shape of the long-K x6 forward GEMMs.  Measured at
// C3 (bench.py, 3 x 20 iterations each): 16x16x32 13.10 M vs 32x32x16 13.05 M env-steps/s -- on par; the
// forward kernels gain 2-7 % per launch, the dgrad epilogue does not fit 128 registers on the 16x16 tiling
// (acc spills in the main loop: 1.2 ms per launch) and stays on 32x32x16.
int x6_shape() {  // read per call (A/B measurements in one process)
    const char* e = std::getenv("RSLRL_X6_SHAPE");
    return (e && std::atoi(e) == 16) ? 16 : 32;
}

int dgrad_occupancy() {  // tuning knob: RSLRL_DGRAD_OCC=2|4 (default 4)
    static const int v = [] {
        const char* e = std::getenv("RSLRL_DGRAD_OCC");
        return (e && std::atoi(e) == 2) ? 2 : 4;
    }();
    return v;
}

// the opt-in 16x16x32 forward (RSLRL_X6_SHAPE=16); false: not taken
template <int EPI>
bool launch_x6s(const GemmParams& p, const uint4* img, bool fullm, dim3 g, hipStream_t st) {
    if constexpr (EPI == kEpiBias || EPI == kEpiBiasElu) {
        if (x6_shape() != 16 || (p.N & 3) || !aligned16(p.c) || !aligned16(p.bias) || p.amax_out)
            return false;  // 16-B epilogue, no amax
        const dim3 b(kThreads);
        const char* mw = std::getenv("RSLRL_X6S_MINW");  // tuning knob, read per call: 2 = one workgroup per CU
        if (mw && std::atoi(mw) == 2) {
            if (fullm) hipLaunchKernelGGL((mlp_gemm_x6s_kernel<EPI, true, 2, false>), g, b, 0, st, p, img);
            else hipLaunchKernelGGL((mlp_gemm_x6s_kernel<EPI, false, 2, false>), g, b, 0, st, p, img);
        } else if (x6s_nontemporal()) {
            if (fullm) hipLaunchKernelGGL((mlp_gemm_x6s_kernel<EPI, true, 4, true>), g, b, 0, st, p, img);
            else hipLaunchKernelGGL((mlp_gemm_x6s_kernel<EPI, false, 4, true>), g, b, 0, st, p, img);
        } else {
            if (fullm) hipLaunchKernelGGL((mlp_gemm_x6s_kernel<EPI, true, 4, false>), g, b, 0, st, p, img);
            else hipLaunchKernelGGL((mlp_gemm_x6s_kernel<EPI, false, 4, false>), g, b, 0, st, p, img);
        }
        return true;
    } else {
        return false;
    }
}

int out_fwd_nt() {  // tuning knob: RSLRL_OUT_FWD_NT=0|1
    static const int v = [] {
        const char* e = std::getenv("RSLRL_OUT_FWD_NT");
        return (e && std::atoi(e) == 1) ? 1 : 0;
    }();
    return v;
}

int cu_count() {  // compute units of the current device (cached per device)
    static int cache[64] = {};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 256;
    if (cache[dev] <= 0) {
        int n = 0;
        if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
        cache[dev] = n;
    }
    return cache[dev];
}

int out_bwd_mode() {  // tuning knob: RSLRL_OUT_BWD=mfma selects the MFMA kernel (default: VALU)
    static const int v = [] {
        const char* e = std::getenv("RSLRL_OUT_BWD");
        return (e && std::string(e) == "mfma") ? 1 : 0;
    }();
    return v;
}

// bimage == nullptr: exact f32 MFMA main loop on p.bw; otherwise the split main loop on the image (PL = 3: x6
// bf16 planes, layout-0 image; PL = 2: h3 fp16 planes, layout-2 image, A scaled from *p.a_amax).
template <int EPI, int PL = 3>
int launch(const GemmParams& p, const void* bimage, hipStream_t st) {
    const int64_t tiles = ceil_div(p.M, kBM);
    if (tiles > INT32_MAX) return RSLRL_E_INVALID_ARGUMENT;
    const dim3 g(static_cast<unsigned>(tiles)), b(kThreads);
    if (bimage) {
        const uint4* img = static_cast<const uint4*>(bimage);
        // a short reduction (the dgrad of the 12- / 1-wide output layer: one chunk) is bound by the
        // epilogue's h loads, which want the registers of the 2-waves-per-SIMD allocation
        const bool short_k = EPI != kEpiBias && EPI != kEpiBiasElu && p.K <= 2 * kKC;
        const bool fullm = p.M % kBM == 0 && p.K % kKC == 0;
        if constexpr (EPI == kEpiEluGradWgrad) {  // K = Nred in {4, 8, 12, 16}
            if constexpr (PL != 3) {
                return RSLRL_E_UNSUPPORTED;
            } else if (out_bwd_mode() == 0) {
                out_bwd_valu_launch(p, img, g, st);
            } else if (p.K & 3) {
                return RSLRL_E_UNSUPPORTED;  // the MFMA variant reads whole float4 rows of dZ
            } else {
                auto go = [&](auto nr) {
                    constexpr int NR = decltype(nr)::value;
                    if (fullm) hipLaunchKernelGGL((mlp_gemm_x6_kernel<EPI, true, 2, NR>), g, b, 0, st, p, img);
                    else hipLaunchKernelGGL((mlp_gemm_x6_kernel<EPI, false, 2, NR>), g, b, 0, st, p, img);
                };
                switch (p.K) {
                    case 4: go(std::integral_constant<int, 4>{}); break;
                    case 8: go(std::integral_constant<int, 8>{}); break;
                    case 12: go(std::integral_constant<int, 12>{}); break;
                    default: go(std::integral_constant<int, 16>{}); break;
                }
            }
        } else if (short_k) {
            if (fullm) hipLaunchKernelGGL((mlp_gemm_x6_kernel<EPI, true, 2, 4, PL>), g, b, 0, st, p, img);
            else hipLaunchKernelGGL((mlp_gemm_x6_kernel<EPI, false, 2, 4, PL>), g, b, 0, st, p, img);
        } else if (k48_deep<EPI>(p, fullm, PL)) {
            if constexpr (PL == 3 && (EPI == kEpiBias || EPI == kEpiBiasElu))
                hipLaunchKernelGGL((mlp_gemm_x6_kernel<EPI, true, 4, 4, PL, 3>), g, b, 0, st, p, img);
        } else if (PL != 3 || !launch_x6s<EPI>(p, img, fullm, g, st)) {
            if (fullm) hipLaunchKernelGGL((mlp_gemm_x6_kernel<EPI, true, 4, 4, PL>), g, b, 0, st, p, img);
            else hipLaunchKernelGGL((mlp_gemm_x6_kernel<EPI, false, 4, 4, PL>), g, b, 0, st, p, img);
        }
    } else if constexpr (EPI == kEpiEluGradWgrad) {
        return RSLRL_E_UNSUPPORTED;  // x6 path only
    } else if (EPI == kEpiEluGrad && dgrad_occupancy() == 2) {
        hipLaunchKernelGGL((mlp_gemm_kernel<EPI, 2>), g, b, 0, st, p);
    } else {
        hipLaunchKernelGGL((mlp_gemm_kernel<EPI, 4>), g, b, 0, st, p);
    }
    return launch_status();
}

}  // namespace
}  // namespace rslrl

using namespace rslrl;

extern "C" int64_t rslrl_linear_tiles(int64_t M) { return ceil_div(M, kBM); }

extern "C" size_t rslrl_amax_workspace_bytes(void) { return 1024; }

namespace {
// RSLRL_H3_DEEP = bit mask over ops (1 << RSLRL_LINEAR_*) taking the look-ahead main loop; read per call
// (A/B measurements in one process)
int h3_deep(int op) {
    const char* e = std::getenv("RSLRL_H3_DEEP");
    const int mask = e ? std::atoi(e) : kH3DeepDefault;
    return (mask >> op) & 1;
}

}  // namespace

// The one validator of the fused linear ops (include/rslrl_amd.h, the op x arith table): checks `a` for its op and
// arithmetic and fills p by name; nothing is launched.  An empty batch (M == 0) is RSLRL_OK once the shape is checked,
// before any pointer is looked at: the caller then launches nothing.
int rslrl::gemm_params(const rslrl_linear_args_t* a, GemmParams& p) {
    p = GemmParams{};
    const int op = a->op;
    const bool f32 = a->arith == RSLRL_ARITH_F32, h3 = a->arith == RSLRL_ARITH_H3;
    if (!f32 && !h3 && a->arith != RSLRL_ARITH_X6) return RSLRL_E_INVALID_ARGUMENT;
    // K % 4 == 0, except the output-layer backward's reduction width (Nred 1..16, dZ rows read as they are)
    if (a->M < 0 || a->K < 1 || a->N < 1 || a->N > kBN || ((a->K & 3) && op != RSLRL_LINEAR_DGRAD_ELU_WGRAD) ||
        a->K > INT32_MAX / 2)
        return RSLRL_E_INVALID_ARGUMENT;
    p.M = a->M;
    p.K = a->K;
    p.N = a->N;
    p.deep = h3_deep(op);
    if (a->M == 0) return RSLRL_OK;
    if (!a->a || !a->bimage || (h3 && !a->a_amax)) return RSLRL_E_INVALID_ARGUMENT;
    if (a->amax_out && !a->amax_workspace) return RSLRL_E_INVALID_ARGUMENT;
    if (!aligned16(a->a) || !aligned16(a->bimage)) return RSLRL_E_MISALIGNED;
    if (a->amax_out && (op == RSLRL_LINEAR_FWD_OUT || f32)) return RSLRL_E_UNSUPPORTED;
    p.a = a->a;
    p.bw = f32 ? static_cast<const float*>(a->bimage) : nullptr;  // f32: the B operand itself, no image
    p.a_amax = a->a_amax;
    p.amax_out = a->amax_out;
    p.amax_ws = static_cast<unsigned*>(a->amax_workspace);
    switch (op) {
        case RSLRL_LINEAR_FWD:
        case RSLRL_LINEAR_FWD_ELU:
            if (!a->bias || !a->c) return RSLRL_E_INVALID_ARGUMENT;
            p.bias = a->bias;
            p.c = a->c;
            return RSLRL_OK;
        case RSLRL_LINEAR_DGRAD_ELU_WGRAD:
            if (f32 || h3) return RSLRL_E_UNSUPPORTED;
            if (a->K > kMaxWgradRows || !a->wgrad_partials) return RSLRL_E_INVALID_ARGUMENT;
            p.wpart = a->wgrad_partials;
            [[fallthrough]];
        case RSLRL_LINEAR_DGRAD_ELU:  // colsum_partials optional, except for the f32 kernel (it always writes them)
            if (!a->h || !a->c || (f32 && !a->colsum_partials)) return RSLRL_E_INVALID_ARGUMENT;
            p.h = a->h;
            p.c = a->c;
            p.colsum = a->colsum_partials;
            p.ctiles = ceil_div(a->M, kBM);
            return RSLRL_OK;
        case RSLRL_LINEAR_FWD_OUT:
            if (f32) return RSLRL_E_UNSUPPORTED;
            if ((a->N & 3) || a->nout < 1 || a->nout > kMaxOutWidth || !a->bias || !a->out_bias || !a->out_image ||
                !a->y)
                return RSLRL_E_INVALID_ARGUMENT;
            if (!aligned16(a->bias) || !aligned16(a->out_image) || (a->c && !aligned16(a->c))) return RSLRL_E_MISALIGNED;
            p.bias = a->bias;
            p.c = a->c;
            p.oimg = static_cast<const uint4*>(a->out_image);
            p.obias = a->out_bias;
            p.y = a->y;
            p.nout = a->nout;
            p.nt = out_fwd_nt();
            return RSLRL_OK;
        default:
            return RSLRL_E_INVALID_ARGUMENT;
    }
}

namespace {
// The single launch of validated params.  x6 and f32 share launch<EPI, 3>: f32 passes no image and the kernel reads
// p.bw.  RSLRL_LINEAR_FWD_OUT (x6 or h3; gemm_params refuses f32) is mlp_heads.hip's.
int launch_op(const rslrl_linear_args_t* a, const GemmParams& p, hipStream_t st) {
    const void* img = a->arith == RSLRL_ARITH_F32 ? nullptr : a->bimage;
    if (a->arith != RSLRL_ARITH_H3) {
        switch (a->op) {
            case RSLRL_LINEAR_FWD_ELU: return launch<kEpiBiasElu, 3>(p, img, st);
            case RSLRL_LINEAR_FWD: return launch<kEpiBias, 3>(p, img, st);
            case RSLRL_LINEAR_DGRAD_ELU: return launch<kEpiEluGrad, 3>(p, img, st);
            case RSLRL_LINEAR_DGRAD_ELU_WGRAD: return launch<kEpiEluGradWgrad, 3>(p, img, st);
            default: return fwd_out_launch(p, img, 3, st);
        }
    }
    switch (a->op) {
        case RSLRL_LINEAR_FWD_ELU: return launch<kEpiBiasElu, 2>(p, img, st);
        case RSLRL_LINEAR_FWD: return launch<kEpiBias, 2>(p, img, st);
        case RSLRL_LINEAR_DGRAD_ELU: return launch<kEpiEluGrad, 2>(p, img, st);
        default: return fwd_out_launch(p, img, 2, st);
    }
}
}  // namespace

// One entry point for every fused linear op in every arithmetic (include/rslrl_amd.h rslrl_linear_args_t).
extern "C" int rslrl_linear_gemm(const rslrl_linear_args_t* a, rslrl_stream_t stream) {
    if (!a) return RSLRL_E_INVALID_ARGUMENT;
    GemmParams p;
    const int rc = gemm_params(a, p);
    if (rc || a->M == 0) return rc;
    return launch_op(a, p, reinterpret_cast<hipStream_t>(stream));
}

namespace {
// ---- "w4": the same x6 GEMM with 4 waves per workgroup side by side (1 x 4), each 128 x 64 = 4 x 2 MFMA tiles, on
// the 128 x 256 tile: a B fragment feeds 4 MFMAs and an A fragment 2 (0.375 ds_read_b128 per MFMA instead of 0.5),
// two workgroups per CU at <= 256 registers (2 waves per SIMD).  Full tiles, x6, K = 256, no column sums or amax
// (the paired update's hidden forward and input gradient); RSLRL_W4 selects it (A/B).
constexpr int kThreadsW4 = 256;
#ifndef RSLRL_W4_DEPTH
#define RSLRL_W4_DEPTH 2
#endif
constexpr int kW4Depth = RSLRL_W4_DEPTH;  // A look-ahead (chunks): the 256-register budget has room for 2

template <int EPI>
__device__ __forceinline__ void mlp_gemm_x6_w4_body(const GemmParams& p, const uint4* __restrict__ bimg, char* lds_b0,
                                                    char* lds_b1) {
    constexpr int BM = kBM, PL = 3, I = 4;
    constexpr int planeA = BM * kX6RowB;
    using Frag = typename Arith<PL>::frag;
    char* lds[2];
    lds[0] = lds_b0;
    lds[1] = lds_b1;
    const int lane = threadIdx.x & 63;
    const int wn = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // cols wn * 64
    const int h = lane >> 5;
    const int l32 = lane & 31;
    const int64_t row0 = static_cast<int64_t>(blockIdx.x) * BM;
    f32x16 acc[I][2];
#pragma unroll
    for (int i = 0; i < I; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = f32x16{};
    auto compute = [&](const char* a_lds, const char* b_lds) {
        Frag bf[2][PL];
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int q = 0; q < PL; ++q) bf[j][q] = read_frag<Frag>(b_lds + q * kX6PlaneB, wn * 64 + j * 32 + l32, h);
#pragma unroll
        for (int i = 0; i < I; ++i) {
            Frag af[PL];
#pragma unroll
            for (int q = 0; q < PL; ++q) af[q] = read_frag<Frag>(a_lds + q * planeA, i * 32 + l32, h);
#pragma unroll
            for (int j = 0; j < 2; ++j) acc[i][j] = Arith<PL>::mfma(af, bf[j], acc[i][j]);
        }
    };
    deep_pipeline<BM, PL, 16, kW4Depth, decltype(compute)&, NoHook, kThreadsW4>(p, row0, bimg, lds, 1.f, compute);
    float colpart[2];
    float amx = 0.f;
    epilogue_tiles<EPI, I, 2>(p, acc, row0, wn * 64, true, colpart, amx);
}

template <int EPI>
__global__ __launch_bounds__(kThreadsW4, 2) void mlp_gemm_x6_w4_pair_kernel(GemmPair b) {
    __shared__ __attribute__((aligned(16))) char lds_b0[x6_buf_bytes<EPI, 3>()];
    __shared__ __attribute__((aligned(16))) char lds_b1[x6_buf_bytes<EPI, 3>()];
    mlp_gemm_x6_w4_body<EPI>(b.p[blockIdx.y], b.img[blockIdx.y], lds_b0, lds_b1);
}

// ---- "w8": 256 x 256 tiles, 8 waves as 2 (M) x 4 (N) of the w4 wave tile (128 x 64), one workgroup per CU at <= 256
// registers.  Each B-image chunk is staged once per 256 rows instead of once per 128: the image (384 KiB per tile, from
// L2) is the kernels' largest stream -- at 128-row tiles 2.36 GB per input-gradient pair launch against 2.4 GB of HBM
// traffic, 2.4 M of the launch's 6.3 M vector-memory instructions (SQ counters, profiles/r4_mlp_pmc_base.json).
constexpr int kBMW8 = 256;
#ifndef RSLRL_W8_DEPTH
#define RSLRL_W8_DEPTH 2
#endif
constexpr int kW8Depth = RSLRL_W8_DEPTH;  // A look-ahead (chunks)

template <int EPI>
__device__ __forceinline__ void mlp_gemm_x6_w8_body(const GemmParams& p, const uint4* __restrict__ bimg, char* lds_b0,
                                                    char* lds_b1) {
    constexpr int BM = kBMW8, PL = 3, I = 4;
    constexpr int planeA = BM * kX6RowB;
    using Frag = typename Arith<PL>::frag;
    char* lds[2];
    lds[0] = lds_b0;
    lds[1] = lds_b1;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int wm = wave >> 2;  // rows wm * 128
    const int wn = wave & 3;   // cols wn * 64
    const int h = lane >> 5;
    const int l32 = lane & 31;
    const int64_t row0 = static_cast<int64_t>(blockIdx.x) * BM;
    f32x16 acc[I][2];
#pragma unroll
    for (int i = 0; i < I; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = f32x16{};
    auto compute = [&](const char* a_lds, const char* b_lds) {
        Frag bf[2][PL];
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int q = 0; q < PL; ++q) bf[j][q] = read_frag<Frag>(b_lds + q * kX6PlaneB, wn * 64 + j * 32 + l32, h);
#pragma unroll
        for (int i = 0; i < I; ++i) {
            Frag af[PL];
#pragma unroll
            for (int q = 0; q < PL; ++q) af[q] = read_frag<Frag>(a_lds + q * planeA, wm * 128 + i * 32 + l32, h);
#pragma unroll
            for (int j = 0; j < 2; ++j) acc[i][j] = Arith<PL>::mfma(af, bf[j], acc[i][j]);
        }
    };
    deep_pipeline<BM, PL, 16, kW8Depth, decltype(compute)&, NoHook, kThreads>(p, row0, bimg, lds, 1.f, compute);
    float colpart[2];
    float amx = 0.f;
    epilogue_tiles<EPI, I, 2>(p, acc, row0 + wm * 128, wn * 64, true, colpart, amx);
}

template <int EPI>
__global__ __launch_bounds__(kThreads, 2) void mlp_gemm_x6_w8_pair_kernel(GemmPair b) {
    constexpr int bytes = 3 * kBMW8 * kX6RowB + 3 * kX6PlaneB;
    __shared__ __attribute__((aligned(16))) char lds_b0[bytes];
    __shared__ __attribute__((aligned(16))) char lds_b1[bytes];
    mlp_gemm_x6_w8_body<EPI>(b.p[blockIdx.y], b.img[blockIdx.y], lds_b0, lds_b1);
}

// RSLRL_W4 (read per call: A/B in one process): 1 = every eligible launch, 0 = none; unset = the input gradient at
// >= 2048 tiles per problem (measured, scripts/w4_probe.py: dgrad pair at 393,216 rows 669 -> 642 us; the hidden
// forward 607 -> 617 us and both equal within noise at 98,304 rows)
bool w4_enabled(int epi, int64_t tiles) {
    const char* e = std::getenv("RSLRL_W4");
    if (e && e[0] == '1') return true;
    if (e && e[0] == '0') return false;
    return epi == kEpiEluGrad && tiles >= 2048;
}

// RSLRL_W8 (read per call): 1 = the 256-row tiles for every eligible launch (M % 256 == 0), 0 = none (default)
bool w8_enabled(int epi, int64_t M) {
    (void)epi;
    const char* e = std::getenv("RSLRL_W8");
    return e && e[0] == '1' && M % kBMW8 == 0;
}

template <int EPI, int PL>
int launch_pair(const GemmPair& b, bool fullm, hipStream_t st) {
    const int64_t tiles = ceil_div(b.p[0].M, kBM);
    if (tiles > INT32_MAX) return RSLRL_E_INVALID_ARGUMENT;
    const dim3 g(static_cast<unsigned>(tiles), 2), blk(kThreads);
    if constexpr (PL == 3 && (EPI == kEpiBias || EPI == kEpiBiasElu)) {
        if (k48_deep<EPI>(b.p[0], fullm, PL)) {  // both problems share the shape and the op
            hipLaunchKernelGGL((mlp_gemm_x6_pair_kernel<EPI, true, PL, 3>), g, blk, 0, st, b);
            return launch_status();
        }
    }
    if constexpr (PL == 3 && (EPI == kEpiBiasElu || EPI == kEpiEluGrad)) {
        const bool plain = b.p[0].colsum == nullptr && b.p[1].colsum == nullptr && b.p[0].amax_out == nullptr &&
                           b.p[1].amax_out == nullptr;
        if (w8_enabled(EPI, b.p[0].M) && plain && b.p[0].K == 16 * kKC && b.p[0].N == kBN && b.p[0].deep) {
            hipLaunchKernelGGL((mlp_gemm_x6_w8_pair_kernel<EPI>), dim3(static_cast<unsigned>(b.p[0].M / kBMW8), 2),
                               dim3(kThreads), 0, st, b);
            return launch_status();
        }
        if (w4_enabled(EPI, tiles) && fullm && plain && b.p[0].K == 16 * kKC && b.p[0].N == kBN && b.p[0].deep) {
            hipLaunchKernelGGL((mlp_gemm_x6_w4_pair_kernel<EPI>), g, dim3(kThreadsW4), 0, st, b);
            return launch_status();
        }
    }
    if constexpr (EPI == kEpiEluGrad) {  // the input gradient stages its first H block like the single launch
        if (fullm) hipLaunchKernelGGL((mlp_gemm_x6_pair_kernel<EPI, true, PL, 0, true>), g, blk, 0, st, b);
        else hipLaunchKernelGGL((mlp_gemm_x6_pair_kernel<EPI, false, PL, 0, true>), g, blk, 0, st, b);
        return launch_status();
    }
    if (fullm) hipLaunchKernelGGL((mlp_gemm_x6_pair_kernel<EPI, true, PL>), g, blk, 0, st, b);
    else hipLaunchKernelGGL((mlp_gemm_x6_pair_kernel<EPI, false, PL>), g, blk, 0, st, b);
    return launch_status();
}

}  // namespace

// Two problems of one op, arithmetic, M and N (and K, except the output-layer backward's reduction widths) in one
// launch -- e.g. the actor's and the critic's layer l.  Each keeps its own operands, bias, output, amax and amax
// workspace.  Both are validated before anything is launched.
extern "C" int rslrl_linear_gemm_pair(const rslrl_linear_args_t* a0, const rslrl_linear_args_t* a1,
                                      rslrl_stream_t stream) {
    if (!a0 || !a1) return RSLRL_E_INVALID_ARGUMENT;
    const int op = a0->op;
    if (a1->op != op || (op != RSLRL_LINEAR_FWD && op != RSLRL_LINEAR_FWD_ELU && op != RSLRL_LINEAR_DGRAD_ELU &&
                         op != RSLRL_LINEAR_FWD_OUT && op != RSLRL_LINEAR_DGRAD_ELU_WGRAD))
        return RSLRL_E_UNSUPPORTED;
    if (a0->arith != a1->arith || a0->M != a1->M || a0->N != a1->N ||
        (a0->K != a1->K && op != RSLRL_LINEAR_DGRAD_ELU_WGRAD))
        return RSLRL_E_INVALID_ARGUMENT;
    if (a0->arith == RSLRL_ARITH_F32) return RSLRL_E_UNSUPPORTED;  // the f32 kernel has no pair form
    if (a0->amax_out && a1->amax_out && a0->amax_workspace == a1->amax_workspace) return RSLRL_E_INVALID_ARGUMENT;
    GemmPair b{};
    for (int i = 0; i < 2; ++i) {
        const int rc = gemm_params(i ? a1 : a0, b.p[i]);
        if (rc) return rc;
        b.img[i] = static_cast<const uint4*>((i ? a1 : a0)->bimage);
    }
    if (a0->M == 0) return RSLRL_OK;
    const int64_t tiles = ceil_div(a0->M, kBM);
    if (tiles > INT32_MAX) return RSLRL_E_INVALID_ARGUMENT;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const auto two_launches = [&] {  // where no pair kernel covers the problems: identical results
        const int rc = launch_op(a0, b.p[0], st);
        return rc ? rc : launch_op(a1, b.p[1], st);
    };
    const dim3 g(static_cast<unsigned>(tiles), 2);
    const bool h3 = a0->arith == RSLRL_ARITH_H3;
    const bool fullm = a0->M % kBM == 0 && a0->K % kKC == 0;
    if (op == RSLRL_LINEAR_DGRAD_ELU_WGRAD) {  // VALU kernels only
        if (out_bwd_mode() != 0 || !out_bwd_pair_dispatch(b, (a0->K + 3) / 4 * 4, (a1->K + 3) / 4 * 4, g, st))
            return two_launches();
        return launch_status();
    }
    if (op == RSLRL_LINEAR_FWD_OUT) {  // output widths may differ; x6 at the default occupancy, at most a tile per CU
        if (h3 || x6_shape() == 16 || 2 * tiles > cu_count()) return two_launches();
        fwd_out_pair_launch(b, fullm, g, st);
        return launch_status();
    }
    if (!h3 && x6_shape() == 16) return two_launches();  // the opt-in 16x16x32 x6 forward has no pair kernel
    if (op == RSLRL_LINEAR_DGRAD_ELU)
        return h3 ? launch_pair<kEpiEluGrad, 2>(b, fullm, st) : launch_pair<kEpiEluGrad, 3>(b, fullm, st);
    // streaming only where it measured faster (profiles/r5_fs_ab.json, medians of two processes each): M >= 196,608
    // (393,216: 688-695 vs 706-708 us; 196,608: 307 vs 325-327) and M <= 16,384 (37 vs 40 us; one tile per
    // workgroup); 65,536 and 98,304 rows stay tiled (106-108 vs 105-106, 155-157 vs 151-152)
    const int64_t ftiles = a0->M / kBM;
    const bool stream_m = ftiles >= 1536 || ftiles <= 128 || fwd_stream_forced();
    if (op == RSLRL_LINEAR_FWD_ELU && !h3 && fwd_stream_enabled() && stream_m &&
        (a0->K == kBN || (a0->K == 48 && fwd_stream48())) && a0->N == kBN && a0->M % kBM == 0 && !a0->amax_out &&
        !a1->amax_out) {
        // the square hidden layers: the streaming forward (mlp_fwd_stream.hip, same bits); the 48-wide first layer only
        // on request (RSLRL_FWD_STREAM=48): HBM-bound, it measured 222 vs 190-201 us on the tiled kernel's two
        // workgroups per CU (profiles/r5_fs_ab.json)
        const FwdStreamProblem fp[2] = {{b.p[0].a, b.img[0], b.p[0].bias, b.p[0].c},
                                        {b.p[1].a, b.img[1], b.p[1].bias, b.p[1].c}};
        return fwd_stream_pair(fp, 2, a0->M, a0->K, st);
    }
    if (op == RSLRL_LINEAR_FWD_ELU)
        return h3 ? launch_pair<kEpiBiasElu, 2>(b, fullm, st) : launch_pair<kEpiBiasElu, 3>(b, fullm, st);
    return h3 ? launch_pair<kEpiBias, 2>(b, fullm, st) : launch_pair<kEpiBias, 3>(b, fullm, st);
}
