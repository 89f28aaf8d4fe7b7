// Tile and weight-image geometry of the split-precision MLP kernels, and the ELU's negative branch: the one definition
// of what the tiled GEMMs (mlp_gemm.hip, mlp_heads.hip), the image builder (mlp_image.hip), the output-layer backward
// (mlp_out_bwd.hip), the streaming forward (mlp_fwd_stream.hip) and the rollout's fused MLP (rollout_mlp.hip) must agree
// on bit for bit.
#pragma once

#include "common.h"

namespace rslrl {

constexpr int kBM = 128;       // rows of a workgroup tile
constexpr int kBN = 256;       // columns of a workgroup tile (the widest layer)
constexpr int kKC = 16;        // k depth of a staged chunk
constexpr int kThreads = 512;  // 8 waves

// ---- B image, layout 0 (RSLRL_BIMAGE_LAYOUT_GEMM): [chunk][3 bf16 planes][256 rows][32 B] -- byte for byte the LDS
// image of a chunk.  A row is 16 bf16 = 32 B; its two 16-B halves are swapped on rows with (row >> 3) & 1, which makes
// both the staging stores (ds_write_b64, 16-lane groups) and the fragment reads (ds_read_b128: lane l reads row l & 31,
// half l >> 5) bank-conflict free.
constexpr int kX6RowB = 32;
constexpr int kX6PlaneB = kBN * kX6RowB;  // 8 KiB
constexpr int kX6ChunkB = 3 * kX6PlaneB;  // 24 KiB: one chunk of the B image
// h3 B image (RSLRL_BIMAGE_LAYOUT_H3): [chunk][2 fp16 planes][256 rows][32 B swizzled] of t_n B[n][k] (t_n a
// power of two per row n from max_k |B[n][k]|), then 1 / t_n for the 256 rows (fp32).
constexpr int kH3ChunkB = 2 * kX6PlaneB;
__host__ __device__ inline int64_t h3_image_scales_offset(int depth) { return ((depth + kKC - 1) / kKC) * int64_t{kH3ChunkB}; }

__device__ __forceinline__ int swz(int row, int half) { return row * kX6RowB + 16 * (half ^ ((row >> 3) & 1)); }

// Output-layer image (layout 1, RSLRL_LINEAR_FWD_OUT): for wave column group wn (64 columns), column tile j,
// k step s, plane q, lane half h and output o: 8 bf16 of W_out[o][c], c = 64 wn + 32 j + 4 h + (t & 3) +
// 8 (2 s + (t >> 2)), t < 8 -- the columns lane half h of the C^T epilogue holds in registers 8 s .. 8 s + 7.
// Unit (16 B) index ((((wn * 2 + j) * 2 + s) * 3 + q) * 2 + h) * 32 + o; zero for o >= rows, c >= depth.
// Followed by the same weights in fp32 for the VALU path (<= 4 outputs): 8 floats per (wn, j, s, h, o) at
// unit kOutImagePlaneUnits + 2 ((((wn * 2 + j) * 2 + s) * 2 + h) * 32 + o).
constexpr int kMaxOutWidth = 32;  // outputs of an out image (the o index)
constexpr int kOutImagePlaneUnits = 4 * 2 * 2 * 3 * 2 * 32;
constexpr int kOutImageThreads = 4 * 2 * 2 * 2 * 32;
constexpr int kOutImageUnits = kOutImagePlaneUnits + 2 * kOutImageThreads;
__host__ __device__ constexpr int out_image_unit(int wn, int j, int s, int q, int h, int o) {
    return ((((wn * 2 + j) * 2 + s) * 3 + q) * 2 + h) * 32 + o;
}
// fp32 section: index of the float4 pair (8 floats) of (wn, j, s, h, o), counted from unit kOutImagePlaneUnits
__host__ __device__ constexpr int out_image_f32_pair(int wn, int j, int s, int h, int o) {
    return (((wn * 2 + j) * 2 + s) * 2 + h) * 32 + o;
}

// expm1(v) for v <= 0 (the ELU's negative branch) in ~9 VALU instead of libm expm1f's ~27: a degree-5 polynomial
// (Horner, explicit fma) on [-0.5, 0], exp(v) - 1 below (the subtraction is exact there, error = exp's ~1 ulp of a
// value <= 0.61 -> <= 2 ulp of the result).
__device__ __forceinline__ float elu_neg(float v) {
    // minimax fit of expm1(v) / v on [-0.5, 0] (degree 5, Horner with explicit fma; round 6): 1.26 ulp at most against
    // expm1 over every 7th fp32 in [-0.5, 0) (the degree-9 Taylor form it replaced: 1.14 ulp) in 3 fewer FMAs
    float t = __fmaf_rn(v, 0.0011216326f, 0.008187376f);
    t = __fmaf_rn(v, t, 0.04162908f);
    t = __fmaf_rn(v, t, 0.16666223f);
    t = __fmaf_rn(v, t, 0.49999982f);
    t = __fmaf_rn(v, t, 1.0f);
    const float poly = v * t;
    const float e = __expf(v) - 1.0f;
    return v > -0.5f ? poly : e;
}

}  // namespace rslrl
