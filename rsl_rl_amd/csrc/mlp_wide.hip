// Linear + ELU layers wider than the 256-column tile (hidden widths up to 1024), x6 arithmetic: the default actor /
// critic of Legged-Gym and Isaac Lab is [512, 256, 128].  A layer with N > 256 outputs or K > 256 inputs goes through
// the three entry points of this unit:
//   rslrl_linear_gemm_wide          RSLRL_LINEAR_FWD / FWD_ELU / DGRAD_ELU: one launch, the ceil(N / 256) column blocks
//                                   of the output on gridDim.y.  Block j is the dense 256-column problem of
//                                   mlp_gemm_x6_kernel on the j-th block image and its slice of bias / h / c / colsum,
//                                   with the layer's N as row stride (WideGemmParams::ld): the device code is
//                                   mlp_gemm_x6.h's, so a block's bits are the dense kernel's.
//   rslrl_linear_prepare_bimage_wide  the ceil(rows / 256) consecutive layout-GEMM block images of a weight, one launch
//   rslrl_linear_wgrad_bias_wide    dW [N, K] = dz^T x in TN x 256 blocks (TN = 256, or 64 when N <= 64) of
//                                   mlp_wgrad_x6.h's split-K body: grid (row slices, N blocks, K blocks), one launch,
//                                   then the fp64 fold of the slices (rslrl_fold_partials): deterministic
// No atomics: every output element is written by one lane.
#include <algorithm>
#include <type_traits>

#include "common.h"
#include "mlp_gemm.h"
// the two device headers are instantiated here on the strided parameter blocks
#define RSLRL_GEMM_WIDE
#define RSLRL_WGRAD_WIDE
#include "mlp_gemm_x6.h"
#include "mlp_wgrad_x6.h"

namespace rslrl {
namespace {

constexpr int kWideMax = 1024;  // widest layer side

// ---- GEMM: the kernel argument of a wide layer.  p describes the whole layer (N = ld = its width, the pointers its
// first column); the workgroup of column block blockIdx.y narrows a copy to its block.
struct WideGemmArgs {
    WideGemmParams p;
    const uint4* img;   // ceil(N / 256) block images
    int64_t img_units;  // 16-byte units per block image
};

template <int EPI, bool FULL, int MINW>
__global__ __launch_bounds__(kThreads, MINW) void mlp_gemm_x6_wide_kernel(WideGemmArgs w) {
    __shared__ __attribute__((aligned(16))) char lds_b0[x6_buf_bytes<EPI, 3>()];
    __shared__ __attribute__((aligned(16))) char lds_b1[x6_buf_bytes<EPI, 3>()];
    const int j = blockIdx.y;
    const int c0 = j * kBN;
    WideGemmParams p = w.p;
    p.N = min(kBN, w.p.N - c0);
    p.c += c0;
    if (p.bias) p.bias += c0;
    if (p.h) p.h += c0;
    if (p.colsum) p.colsum += c0;
    // STAGE = false: the LDS stage of the first H block assumes the dense row stride
    mlp_gemm_x6_body<EPI, FULL, 4, 3, false, 0, 0>(p, w.img + j * w.img_units, lds_b0, lds_b1);
}

template <int EPI>
int launch_wide(const WideGemmArgs& w, hipStream_t st) {
    const WideGemmParams& p = w.p;
    const int64_t tiles = ceil_div(p.M, kBM);
    if (tiles > INT32_MAX) return RSLRL_E_UNSUPPORTED;
    const dim3 g(static_cast<unsigned>(tiles), static_cast<unsigned>(ceil_div(p.N, kBN))), b(kThreads);
    const bool fullm = p.M % kBM == 0 && p.K % kKC == 0;
    // as the dense launch: a short reduction's input gradient is bound by the epilogue's h loads and takes the
    // registers of one workgroup per CU (the forward epilogues have no such form: not instantiated)
    if constexpr (EPI == kEpiEluGrad) {
        if (p.K <= 2 * kKC) {
            if (fullm) hipLaunchKernelGGL((mlp_gemm_x6_wide_kernel<EPI, true, 2>), g, b, 0, st, w);
            else hipLaunchKernelGGL((mlp_gemm_x6_wide_kernel<EPI, false, 2>), g, b, 0, st, w);
            return launch_status();
        }
    }
    if (fullm) hipLaunchKernelGGL((mlp_gemm_x6_wide_kernel<EPI, true, 4>), g, b, 0, st, w);
    else hipLaunchKernelGGL((mlp_gemm_x6_wide_kernel<EPI, false, 4>), g, b, 0, st, w);
    return launch_status();
}

bool wide_side(int32_t n) { return n >= 4 && n <= kWideMax && (n & 3) == 0; }

// ---- images: block image blockIdx.y holds rows 256 blockIdx.y .. of B in the layout-GEMM form of mlp_tile.h
// ([chunk][3 bf16 planes][256 rows][32 B swizzled]); one thread per (chunk, image row n, physical 16-byte half), as
// bimage_kernel (mlp_image.hip) builds a single image.  B[r][k] = transposed ? src[k * rows + r] : src[r * depth + k],
// zero for r >= rows or k >= depth.
__global__ __launch_bounds__(kBlock) void bimage_wide_kernel(const float* __restrict__ src, int rows, int depth,
                                                             int transposed, uint4* image, int64_t img_units) {
    const int nchunks = (depth + kKC - 1) / kKC;
    const int id = blockIdx.x * kBlock + threadIdx.x;
    if (id >= nchunks * kBN * 2) return;
    const int c = id / (kBN * 2);
    const int n = (id >> 1) % kBN;
    const int ph = id & 1;
    const int lh = ph ^ ((n >> 3) & 1);
    const int r = blockIdx.y * kBN + n;
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int k = 16 * c + 8 * lh + j;
        v[j] = (r < rows && k < depth) ? src[transposed ? static_cast<int64_t>(k) * rows + r
                                                        : static_cast<int64_t>(r) * depth + k]
                                       : 0.f;
    }
    uint2 lo[3], hi[3];
    split4(make_float4(v[0], v[1], v[2], v[3]), lo[0], lo[1], lo[2]);
    split4(make_float4(v[4], v[5], v[6], v[7]), hi[0], hi[1], hi[2]);
    uint4* base = image + blockIdx.y * img_units + static_cast<int64_t>(c) * (kX6ChunkB / 16) +
                  (n * kX6RowB + 16 * ph) / 16;
#pragma unroll
    for (int q = 0; q < 3; ++q) base[q * (kX6PlaneB / 16)] = make_uint4(lo[q].x, lo[q].y, hi[q].x, hi[q].y);
}

// ---- weight gradient: block (blockIdx.y, blockIdx.z) of dW, rows of slice blockIdx.x
struct WideWgradArgs {
    WideWgradParams p;  // the whole layer: N, K = ldz, ldx = its widths, the pointers its first columns
};

template <int TN, bool FULL, bool MASKN, int CS>
__global__ __launch_bounds__(kThreadsW, TN <= 64 ? 4 : 2) void wgrad_x6_wide_kernel(WideWgradArgs w) {
    const int n0 = blockIdx.y * TN, k0 = blockIdx.z * kTK;
    WideWgradParams p = w.p;
    p.N = min(TN, w.p.N - n0);
    p.K = min(kTK, w.p.K - k0);
    p.dz += n0;
    p.x += k0;
    p.part += static_cast<int64_t>(n0) * p.ldx + k0;
    // the column sums of a block of dz (x) columns come from the workgroups of the first K (N) block
    float* cs = w.p.part + static_cast<int64_t>(w.p.N) * w.p.K;
    if constexpr (CS == 1) p.cs = blockIdx.z == 0 ? cs + n0 : nullptr;
    else if constexpr (CS == 2) p.cs = blockIdx.y == 0 ? cs + k0 : nullptr;
    else p.cs = nullptr;
    wgrad_x6_body<TN, FULL, 3, MASKN, CS>(p);
}

int64_t colsum_len(int side, int32_t N, int32_t K) { return side == 1 ? N : (side == 2 ? K : 0); }

bool wgrad_shape_ok(int32_t N, int32_t K, int32_t bias_side) {
    return wide_side(N) && wide_side(K) && bias_side >= 0 && bias_side <= 2 && !(bias_side == 1 && N <= 64);
}

}  // namespace
}  // namespace rslrl

using namespace rslrl;

extern "C" int rslrl_linear_gemm_wide(const rslrl_linear_args_t* a, rslrl_stream_t stream) {
    if (!a) return RSLRL_E_INVALID_ARGUMENT;
    const int op = a->op;
    if (op != RSLRL_LINEAR_FWD && op != RSLRL_LINEAR_FWD_ELU && op != RSLRL_LINEAR_DGRAD_ELU) return RSLRL_E_UNSUPPORTED;
    if (a->arith != RSLRL_ARITH_X6 || a->amax_out) return RSLRL_E_UNSUPPORTED;
    if (a->N < 1 || a->N > kWideMax || (a->N & 3) || !wide_side(a->K)) return RSLRL_E_UNSUPPORTED;
    if (a->M < 0) return RSLRL_E_INVALID_ARGUMENT;
    if (a->M == 0) return RSLRL_OK;
    const bool grad = op == RSLRL_LINEAR_DGRAD_ELU;
    if (!a->a || !a->bimage || !a->c || (grad ? !a->h : !a->bias)) return RSLRL_E_INVALID_ARGUMENT;
    if (!aligned16(a->a) || !aligned16(a->bimage) || !aligned16(a->c) || (grad && !aligned16(a->h)))
        return RSLRL_E_MISALIGNED;
    WideGemmArgs w{};
    WideGemmParams& p = w.p;
    p.a = a->a;
    p.M = a->M;
    p.K = a->K;
    p.N = a->N;
    p.ld = a->N;
    p.c = a->c;
    p.deep = a->K == 16 * kKC;  // the unrolled look-ahead main loop of the K = 256 full tiles
    if (grad) {
        p.h = a->h;
        p.colsum = a->colsum_partials;
        p.ctiles = ceil_div(a->M, kBM);
    } else {
        p.bias = a->bias;
    }
    w.img = static_cast<const uint4*>(a->bimage);
    w.img_units = static_cast<int64_t>(rslrl_linear_bimage_bytes(a->K) / 16);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (grad) return launch_wide<kEpiEluGrad>(w, st);
    return op == RSLRL_LINEAR_FWD_ELU ? launch_wide<kEpiBiasElu>(w, st) : launch_wide<kEpiBias>(w, st);
}

extern "C" size_t rslrl_linear_bimage_wide_bytes(int32_t rows, int32_t depth) {
    if (rows < 1 || rows > kWideMax || depth < 1 || depth > kWideMax) return 0;
    return static_cast<size_t>(ceil_div(rows, kBN)) * rslrl_linear_bimage_bytes(depth);
}

extern "C" int rslrl_linear_prepare_bimage_wide(const float* src, int32_t rows, int32_t depth, int32_t transposed,
                                                void* image, rslrl_stream_t stream) {
    if (rows < 1 || rows > kWideMax || depth < 1 || depth > kWideMax) return RSLRL_E_UNSUPPORTED;
    if (!src || !image) return RSLRL_E_INVALID_ARGUMENT;
    if (!aligned16(image)) return RSLRL_E_MISALIGNED;
    const int64_t threads = ceil_div(depth, kKC) * kBN * 2;
    const dim3 grid(static_cast<unsigned>(ceil_div(threads, kBlock)), static_cast<unsigned>(ceil_div(rows, kBN)));
    hipLaunchKernelGGL(bimage_wide_kernel, grid, dim3(kBlock), 0, reinterpret_cast<hipStream_t>(stream), src, rows,
                       depth, transposed ? 1 : 0, static_cast<uint4*>(image),
                       static_cast<int64_t>(rslrl_linear_bimage_bytes(depth) / 16));
    return launch_status();
}

extern "C" size_t rslrl_linear_wgrad_bias_wide_workspace_bytes(int64_t M, int32_t N, int32_t K, int32_t bias_side) {
    if (M < 1 || !wgrad_shape_ok(N, K, bias_side)) return 0;
    const int64_t S = ceil_div(M, wide_rows_per(M, N, K));
    const int64_t NKE = static_cast<int64_t>(N) * K + colsum_len(bias_side, N, K);
    return static_cast<size_t>(S) * NKE * sizeof(float) + rslrl_fold_partials_workspace_bytes(S, NKE);
}

extern "C" int rslrl_linear_wgrad_bias_wide(const float* dz, const float* x, int64_t M, int32_t N, int32_t K,
                                            int32_t bias_side, float* dw_db, void* workspace, size_t workspace_bytes,
                                            rslrl_stream_t stream) {
    if (!wgrad_shape_ok(N, K, bias_side)) return RSLRL_E_UNSUPPORTED;
    if (M < 0) return RSLRL_E_INVALID_ARGUMENT;
    if (M == 0) return RSLRL_OK;
    if (!dz || !x || !dw_db || !workspace) return RSLRL_E_INVALID_ARGUMENT;
    if (!aligned16(dz) || !aligned16(x) || !aligned16(workspace)) return RSLRL_E_MISALIGNED;
    if (workspace_bytes < rslrl_linear_wgrad_bias_wide_workspace_bytes(M, N, K, bias_side))
        return RSLRL_E_WORKSPACE_TOO_SMALL;
    const int64_t rows_per = wide_rows_per(M, N, K);
    const int64_t S = ceil_div(M, rows_per);
    const int64_t NKE = static_cast<int64_t>(N) * K + colsum_len(bias_side, N, K);
    const size_t part_bytes = static_cast<size_t>(S) * NKE * sizeof(float);  // 16-byte multiple (N, K % 4)
    WideWgradArgs w{};
    w.p.dz = dz;
    w.p.x = x;
    w.p.part = static_cast<float*>(workspace);
    w.p.M = M;
    w.p.rows_per = rows_per;
    w.p.N = N;
    w.p.K = K;
    w.p.ldz = N;
    w.p.ldx = K;
    w.p.slice_floats = NKE;
    const int tn = wide_tn(N);
    // full tiles: whole chunks, a multiple of the look-ahead depth of them, every block 256 columns of x and TN (or,
    // on the 64-row tiles, fewer: masked) of dz
    const bool full = (M % rows_per == 0) && (rows_per / kMC) % kWgradDepth == 0 && K % kTK == 0 &&
                      (tn == 64 || N % kTK == 0);
    const dim3 g(static_cast<unsigned>(S), static_cast<unsigned>(ceil_div(N, tn)), static_cast<unsigned>(ceil_div(K, kTK)));
    const dim3 b(kThreadsW);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    auto go = [&](auto tnc, auto cs) {
        constexpr int TN = decltype(tnc)::value, CS = decltype(cs)::value;
        if constexpr (CS == 1 && TN != kTK) {
            return;  // excluded above (bias_side 1 needs N > 64: the 256-row tiles)
        } else {
            if (full && (TN == kTK || N == TN)) hipLaunchKernelGGL((wgrad_x6_wide_kernel<TN, true, false, CS>), g, b, 0, st, w);
            else if (full) hipLaunchKernelGGL((wgrad_x6_wide_kernel<TN, true, true, CS>), g, b, 0, st, w);
            else hipLaunchKernelGGL((wgrad_x6_wide_kernel<TN, false, false, CS>), g, b, 0, st, w);
        }
    };
    auto by_side = [&](auto tnc) {
        if (bias_side == 1) go(tnc, std::integral_constant<int, 1>{});
        else if (bias_side == 2) go(tnc, std::integral_constant<int, 2>{});
        else go(tnc, std::integral_constant<int, 0>{});
    };
    if (tn == 64) by_side(std::integral_constant<int, 64>{});
    else by_side(std::integral_constant<int, 256>{});
    const int rc = launch_status();
    if (rc) return rc;
    return rslrl_fold_partials(static_cast<const float*>(workspace), S, NKE, dw_db,
                               static_cast<char*>(workspace) + part_bytes, workspace_bytes - part_bytes, stream);
}
