// A first layer whose input width K is no multiple of 4 (the 235-float observation of the rough-terrain locomotion
// tasks), x6 arithmetic: the operand rows are read as they lie in memory, row stride K floats, no padded copy.
//   rslrl_linear_gemm_ragged        RSLRL_LINEAR_FWD / FWD_ELU for 1 <= K <= 1024, K % 4 != 0, N % 4 == 0, N <= 1024:
//                                   mlp_wide.hip's kernel (one 256-column block per blockIdx.y; a layer of N <= 256 is
//                                   one block, the tiled kernel's problem) with the ragged A-stage loader
//   rslrl_linear_wgrad_bias_ragged  dW [N, K] = dz^T x (+ the column sums of dz) straight in W's layout: the form, tile
//                                   and slices the zero-padded problem takes today -- (x^T dz)^T on the 32 / 64-row
//                                   tiles for K <= 64 < N, dz^T x on 64 / 256-row tiles above, the dense entry's
//                                   geometry while N and the padded K are <= 256, the wide entry's blocks beyond --
//                                   with the ragged load_tile on the x side; the partials have no pad column (their
//                                   rows are K, or N, floats apart), the fold sums in the padded problem's order
// The device code is mlp_gemm_x6.h's and mlp_wgrad_x6.h's; ragged_load.h holds the loads.  Each masked element enters
// its MFMA k step as a zero, so every output equals, bit for bit, today's entry point on the problem padded with zero
// columns to the next multiple of 4 (tests/test_gpu_ragged_linear.py).  No atomics: one lane writes each output.
#include <algorithm>
#include <type_traits>

#include "common.h"
#include "fold_as.h"
#include "mlp_gemm.h"
#define RSLRL_GEMM_WIDE
#define RSLRL_GEMM_RAGGED
#define RSLRL_WGRAD_WIDE
#define RSLRL_WGRAD_RAGGED
#include "mlp_gemm_x6.h"
#include "mlp_wgrad_x6.h"

namespace rslrl {
namespace {

constexpr int kRaggedMax = 1024;  // widest layer side (mlp_wide.hip's)

struct RaggedGemmArgs {
    WideGemmParams p;   // the whole layer, as mlp_wide.hip's WideGemmArgs
    const uint4* img;   // ceil(N / 256) block images
    int64_t img_units;  // 16-byte units per block image
};

// FULL = false: the masked loader (ragged here) and the generic main loop; a tile whose rows and columns all exist
// still takes the full-tile epilogue (a run-time choice of the body)
template <int EPI>
__global__ __launch_bounds__(kThreads, 4) void mlp_gemm_x6_ragged_kernel(RaggedGemmArgs w) {
    __shared__ __attribute__((aligned(16))) char lds_b0[x6_buf_bytes<EPI, 3>()];
    __shared__ __attribute__((aligned(16))) char lds_b1[x6_buf_bytes<EPI, 3>()];
    const int j = blockIdx.y;
    const int c0 = j * kBN;
    WideGemmParams p = w.p;
    p.N = min(kBN, w.p.N - c0);
    p.c += c0;
    p.bias += c0;
    mlp_gemm_x6_body<EPI, false, 4, 3, false, 0, 0>(p, w.img + j * w.img_units, lds_b0, lds_b1);
}

bool ragged_k(int32_t k) { return k >= 1 && k <= kRaggedMax && (k & 3) != 0; }
bool aligned_n(int32_t n) { return n >= 4 && n <= kRaggedMax && (n & 3) == 0; }

// ---- weight gradient
struct RaggedWgradArgs {
    RaggedWgradParams p;  // the whole layer, as mlp_wide.hip's WideWgradArgs
};

template <int TN, bool FULL, bool MASKN, int CS, int RAG>
__global__ __launch_bounds__(kThreadsW, TN <= 64 ? 4 : 2) void wgrad_x6_ragged_kernel(RaggedWgradArgs w) {
    const int n0 = blockIdx.y * TN, k0 = blockIdx.z * kTK;
    RaggedWgradParams p = w.p;
    p.N = min(TN, w.p.N - n0);
    p.K = min(kTK, w.p.K - k0);
    p.dz += n0;
    p.x += k0;
    p.part += static_cast<int64_t>(n0) * p.ldx + k0;
    p.back = RAG == 1 ? n0 : k0;
    float* cs = w.p.part + static_cast<int64_t>(w.p.N) * w.p.K;
    if constexpr (CS == 1) p.cs = blockIdx.z == 0 ? cs + n0 : nullptr;
    else if constexpr (CS == 2) p.cs = blockIdx.y == 0 ? cs + k0 : nullptr;
    else p.cs = nullptr;
    wgrad_x6_body<TN, FULL, 3, MASKN, CS, RAG>(p);
}

// What the zero-padded problem (K rounded up to Kp) takes today, and the ragged launch in that geometry.  The kernel
// computes (its N) x (its K) = rows of its first operand x columns of its second.
struct RaggedPlan {
    bool first;         // (x^T dz)^T: the kernel's first operand is x (ragged), its second dz
    int Nk, Kk;         // the kernel's N and K, unpadded; Nkp, Kkp: padded
    int Nkp, Kkp;
    int tn, cs;
    dim3 grid;
    int64_t rows_per, S;
    int64_t NKE;        // floats per partial slice: Nk * Kk + column sums
    int64_t order_NKE;  // the padded problem's: its fold's order
    bool full;
};

int ragged_plan(int64_t M, int32_t N, int32_t K, int32_t with_bias, RaggedPlan& pl) {
    if (!ragged_k(K) || !aligned_n(N) || (with_bias != 0 && with_bias != 1)) return RSLRL_E_UNSUPPORTED;
    const int Kp = (K + 3) & ~3;
    const bool wide = N > kTK || Kp > kTK;
    pl.first = K <= 64 && N > 64;
    // below, the layer-by-layer path has no split-kernel form today either (fused_mlp._wgrad_form)
    if (!pl.first && !wide && (K <= 64 || N <= 32)) return RSLRL_E_UNSUPPORTED;
    if (with_bias && !pl.first && N <= 64) return RSLRL_E_UNSUPPORTED;  // the column sums of dz need the 256-row tiles
    pl.cs = with_bias ? (pl.first ? 2 : 1) : 0;
    pl.Nk = pl.first ? K : N;
    pl.Kk = pl.first ? N : K;
    pl.Nkp = pl.first ? Kp : N;
    pl.Kkp = pl.first ? N : Kp;
    const int64_t m = std::max<int64_t>(M, 1);
    bool full;
    if (wide) {
        pl.tn = wide_tn(pl.Nkp);
        pl.rows_per = wide_rows_per(m, pl.Nkp, pl.Kkp);
        full = (m % pl.rows_per == 0) && (pl.rows_per / kMC) % kWgradDepth == 0 && pl.Kkp % kTK == 0 &&
               (pl.tn == 64 || pl.Nkp % kTK == 0);
        pl.grid = dim3(1, static_cast<unsigned>(ceil_div(pl.Nkp, pl.tn)), static_cast<unsigned>(ceil_div(pl.Kkp, kTK)));
    } else {
        pl.tn = pl.Nkp <= 32 ? 32 : (pl.Nkp <= 64 ? 64 : 256);
        pl.rows_per = wgrad_rows_per(m, pl.Nkp);
        full = (m % pl.rows_per == 0) && pl.Kkp == kTK && (pl.rows_per / kMC) % kWgradDepth == 0;
        pl.grid = dim3(1, 1, 1);
    }
    pl.S = ceil_div(m, pl.rows_per);
    pl.grid.x = static_cast<unsigned>(pl.S);
    pl.full = full && K >= 4;  // the look-ahead loop's loader reads whole quads (ragged_load.h)
    const int64_t E = pl.cs == 1 ? pl.Nk : (pl.cs == 2 ? pl.Kk : 0);
    pl.NKE = static_cast<int64_t>(pl.Nk) * pl.Kk + E;  // a multiple of 4: N is
    pl.order_NKE = static_cast<int64_t>(pl.Nkp) * pl.Kkp + E;
    return RSLRL_OK;
}

template <int TN, bool FULL, bool MASKN, int CS, int RAG>
void go(const RaggedPlan& pl, const RaggedWgradArgs& w, hipStream_t st) {
    hipLaunchKernelGGL((wgrad_x6_ragged_kernel<TN, FULL, MASKN, CS, RAG>), pl.grid, dim3(kThreadsW), 0, st, w);
}

// x (the ragged operand) is the kernel's first operand: 32 / 64-row tiles, column sums (of dz) on its K side
template <int TN>
void launch_first(const RaggedPlan& pl, const RaggedWgradArgs& w, hipStream_t st) {
    if (pl.cs == 2) pl.full ? go<TN, true, false, 2, 1>(pl, w, st) : go<TN, false, false, 2, 1>(pl, w, st);
    else pl.full ? go<TN, true, false, 0, 1>(pl, w, st) : go<TN, false, false, 0, 1>(pl, w, st);
}

// x is the kernel's second operand; dz (aligned) the first: masked on a full tile with fewer than TN rows
template <int TN, int CS>
void launch_second(const RaggedPlan& pl, const RaggedWgradArgs& w, hipStream_t st) {
    if (!pl.full) go<TN, false, false, CS, 2>(pl, w, st);
    else if (pl.Nk % TN == 0) go<TN, true, false, CS, 2>(pl, w, st);
    else go<TN, true, true, CS, 2>(pl, w, st);
}

}  // namespace
}  // namespace rslrl

using namespace rslrl;

extern "C" int rslrl_linear_gemm_ragged(const rslrl_linear_args_t* a, rslrl_stream_t stream) {
    if (!a) return RSLRL_E_INVALID_ARGUMENT;
    if (a->op != RSLRL_LINEAR_FWD && a->op != RSLRL_LINEAR_FWD_ELU) return RSLRL_E_UNSUPPORTED;
    if (a->arith != RSLRL_ARITH_X6 || a->amax_out) return RSLRL_E_UNSUPPORTED;
    if (!ragged_k(a->K) || !aligned_n(a->N)) return RSLRL_E_UNSUPPORTED;
    if (a->M < 0) return RSLRL_E_INVALID_ARGUMENT;
    if (a->M == 0) return RSLRL_OK;
    if (!a->a || !a->bimage || !a->c || !a->bias) return RSLRL_E_INVALID_ARGUMENT;
    if (!aligned16(a->a) || !aligned16(a->bimage) || !aligned16(a->c)) return RSLRL_E_MISALIGNED;
    const int64_t tiles = ceil_div(a->M, kBM);
    if (tiles > INT32_MAX) return RSLRL_E_UNSUPPORTED;
    RaggedGemmArgs w{};
    WideGemmParams& p = w.p;
    p.a = a->a;
    p.M = a->M;
    p.K = a->K;
    p.N = a->N;
    p.ld = a->N;
    p.c = a->c;
    p.bias = a->bias;
    w.img = static_cast<const uint4*>(a->bimage);
    w.img_units = static_cast<int64_t>(rslrl_linear_bimage_bytes(a->K) / 16);
    const dim3 g(static_cast<unsigned>(tiles), static_cast<unsigned>(ceil_div(a->N, kBN))), b(kThreads);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (a->op == RSLRL_LINEAR_FWD_ELU) hipLaunchKernelGGL((mlp_gemm_x6_ragged_kernel<kEpiBiasElu>), g, b, 0, st, w);
    else hipLaunchKernelGGL((mlp_gemm_x6_ragged_kernel<kEpiBias>), g, b, 0, st, w);
    return launch_status();
}

extern "C" size_t rslrl_linear_wgrad_bias_ragged_workspace_bytes(int64_t M, int32_t N, int32_t K, int32_t with_bias) {
    RaggedPlan pl;
    if (M < 1 || ragged_plan(M, N, K, with_bias, pl)) return 0;
    return static_cast<size_t>(pl.S) * pl.NKE * sizeof(float) + fold_partials_as_workspace_bytes(pl.S, pl.NKE, pl.order_NKE);
}

extern "C" int rslrl_linear_wgrad_bias_ragged(const float* dz, const float* x, int64_t M, int32_t N, int32_t K,
                                              int32_t with_bias, float* dw_db, void* workspace, size_t workspace_bytes,
                                              rslrl_stream_t stream) {
    RaggedPlan pl;
    const int rc = ragged_plan(M, N, K, with_bias, pl);
    if (rc) return rc;
    if (M < 0) return RSLRL_E_INVALID_ARGUMENT;
    if (M == 0) return RSLRL_OK;
    if (!dz || !x || !dw_db || !workspace) return RSLRL_E_INVALID_ARGUMENT;
    if (!aligned16(dz) || !aligned16(x) || !aligned16(workspace)) return RSLRL_E_MISALIGNED;
    if (workspace_bytes < rslrl_linear_wgrad_bias_ragged_workspace_bytes(M, N, K, with_bias))
        return RSLRL_E_WORKSPACE_TOO_SMALL;
    const size_t part_bytes = static_cast<size_t>(pl.S) * pl.NKE * sizeof(float);  // a 16-byte multiple
    RaggedWgradArgs w{};
    w.p.dz = pl.first ? x : dz;  // the kernel's first operand [M, Nk]
    w.p.x = pl.first ? dz : x;   // its second [M, Kk]
    w.p.part = static_cast<float*>(workspace);
    w.p.M = M;
    w.p.rows_per = pl.rows_per;
    w.p.N = pl.Nk;
    w.p.K = pl.Kk;
    w.p.ldz = pl.Nk;
    w.p.ldx = pl.Kk;
    w.p.slice_floats = pl.NKE;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (pl.first) {
        if (pl.tn == 32) launch_first<32>(pl, w, st);
        else launch_first<64>(pl, w, st);
    } else if (pl.tn == 64) {
        launch_second<64, 0>(pl, w, st);
    } else if (pl.cs == 1) {
        launch_second<256, 1>(pl, w, st);
    } else {
        launch_second<256, 0>(pl, w, st);
    }
    const int lrc = launch_status();
    if (lrc) return lrc;
    // (x^T dz)^T: the fold writes the transpose, dW in W's layout; then the column sums
    return fold_partials_as(static_cast<const float*>(workspace), pl.S, pl.NKE, pl.order_NKE, dw_db, pl.NKE,
                            pl.first ? pl.Nk : 0, pl.first ? pl.Kk : 0, static_cast<char*>(workspace) + part_bytes,
                            workspace_bytes - part_bytes, stream);
}
