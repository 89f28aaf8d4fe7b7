// Internal interface between the units of the fused linear ops: the kernel parameter blocks (filled by the one
// validator, gemm_params), and the launchers one unit offers another.  No C ABI of its own (include/rslrl_amd.h).
//   mlp_gemm.hip     the f32 / x6 / h3 GEMM kernels, rslrl_linear_gemm, rslrl_linear_gemm_pair, gemm_params
//   mlp_heads.hip    everything on the fused last hidden + output layer epilogue (kEpiBiasEluOut): RSLRL_LINEAR_FWD_OUT
//                    and its pair, the critic's and the actor's fused heads (rslrl_value_head_*, rslrl_actor_head_*)
//   mlp_out_bwd.hip  the output-layer backward on the VALU
//   mlp_image.hip    the weight images and the column-sum fold
//   mlp_wide.hip     layers wider than kBN: the x6 kernels above per 256-column block (its own parameter blocks)
#pragma once

#include "common.h"
#include "mlp_tile.h"

namespace rslrl {

// kEpiEluGradWgrad: kEpiEluGrad for a short reduction (Nred <= 16, one chunk: the output layer) that also
// accumulates that layer's weight gradient dZ^T H from the same H tile (x6 path only)
// kEpiBiasEluOut: kEpiBiasElu for the last hidden layer that also applies the (<= 32 wide) output layer to
// the activation tile while it is in registers (x6 path only; the main loop computes C^T tiles)
enum Epilogue { kEpiBias = 0, kEpiBiasElu = 1, kEpiEluGrad = 2, kEpiEluGradWgrad = 3, kEpiBiasEluOut = 4 };
constexpr int kH0StageBytes = 4096;  // kEpiEluGrad: one wave's first H block staged in LDS (stage_h_block0)
constexpr int kMaxWgradRows = 16;
constexpr int kStagedOutWidth = 20;  // kEpiBiasEluOut: widths whose reduction tiles fit beside the h stage

struct GemmParams {
    const float* a;    // [M, K] row-major (lda = K)
    const float* bw;   // [N, K] row-major (the nn.Linear weight layout; for dgrad: W^T)
    const float* bias; // [N] (fwd)
    const float* h;    // [M, N] (dgrad: the activation whose ELU' gates the output)
    float* c;          // [M, N] row-major
    float* colsum;     // [gridDim.x, N] (dgrad)
    int64_t M;
    int K;
    int N;
    int64_t ctiles;    // dgrad: columns of colsum (= rslrl_linear_tiles(M), 128-row tiles)
    float* wpart;      // kEpiEluGradWgrad: per-tile weight-gradient partials [tiles][K][N]
    const uint4* oimg;   // kEpiBiasEluOut: output-layer image (layout 1, mlp_tile.h)
    const float* obias;  // kEpiBiasEluOut: output bias [nout]
    float* y;            // kEpiBiasEluOut: output [M, nout]
    int nout;            // kEpiBiasEluOut: output width <= 32
    int nt;              // kEpiBiasEluOut: streaming stores for h
    const float* a_amax;  // h3: max |A| (device scalar written by A's producer) -> A's power-of-two scale
    float* amax_out;      // optional: max |C| over the stored output (device scalar, for an h3 consumer)
    unsigned* amax_ws;    // with amax_out: {running max bits, arrival ticket}, zero before and after the launch
    int deep;             // K = 256: the unrolled look-ahead main loop (h3_deep_loop; x6 and h3)
    // value head with its backward (mlp_gemm_x6_value_head_kernel, rslrl_value_head_fwd_bwd)
    const float* vh_tv;   // [M] target values (the rollout's values)
    const float* vh_ret;  // [M] returns
    const float* vh_w;    // [N] the value head's fp32 weight row
    float vh_clip;        // clip_param
    float vh_g;           // value_loss_coef / M
    int vh_clipped;       // use_clipped_value_loss
};

// One 256-column block of a layer wider than kBN (mlp_wide.hip): N is the block's width, a / bias / h / c / colsum
// point at the block's first column, and ld is the row stride of h, c and colsum (the layer's whole width).  A struct
// of its own: the dense kernels keep GemmParams as their kernel argument.
struct WideGemmParams : GemmParams {
    int ld;
};

// Two independent problems of one shape in one launch (blockIdx.y picks the problem): the rollout's actor and
// critic layers, whose 512-tile launches (M = 65536) leave half of the 2-per-CU workgroup slots idle.  Each
// problem keeps its own amax output and workspace (the protocol counts gridDim.x workgroups per problem).
struct GemmPair {
    GemmParams p[2];
    const uint4* img[2];
};

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// mlp_gemm.hip.  The one validator of the fused linear ops: checks `a` for its op and arithmetic and fills p by name;
// nothing is launched.
int gemm_params(const rslrl_linear_args_t* a, GemmParams& p);

// mlp_heads.hip.  RSLRL_LINEAR_FWD_OUT of validated params on the image (pl = 3: x6, 2: h3); the pair form (x6: the
// two output widths may differ) on grid g = (tiles, 2).
int fwd_out_launch(const GemmParams& p, const void* bimage, int pl, hipStream_t st);
void fwd_out_pair_launch(const GemmPair& b, bool fullm, dim3 g, hipStream_t st);

// mlp_out_bwd.hip.  RSLRL_LINEAR_DGRAD_ELU_WGRAD on the VALU kernels (validated params; p.K = Nred in 1..16, img the
// x6 image of W^T; g: one workgroup per 128-row tile, y = 2 for a pair).  The pair form covers one reduction <= 4 wide
// beside any of 4 / 8 / 12 / 16 (nr: Nred rounded up to 4) and returns false, nothing launched, for the rest.
void out_bwd_valu_launch(const GemmParams& p, const uint4* img, dim3 g, hipStream_t st);
bool out_bwd_pair_dispatch(const GemmPair& b, int nr0, int nr1, dim3 g, hipStream_t st);

}  // namespace rslrl
