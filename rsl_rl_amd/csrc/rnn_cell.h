// What the fused recurrent cells (lstm_cell.hip, gru_cell.hip) share: the tile constants and the three device helpers
// of their main loop and pointwise part.  One definition, so the two cells' arithmetic cannot drift apart.
//
// Tile: a workgroup of 4 waves owns 64 rows and 128 hidden columns (grid: M / 64 x 2 x problems); wave w owns the 32
// columns n0 = 128 y + 32 w of every gate for the 64 rows, as 32 x 32 C^T accumulators: lane (l32, h) of row block i
// holds row 32 i + l32 and columns n0 + (r & 3) + 8 (r >> 2) + 4 h.  Weight images are layout-0 (GEMM) images of 256
// rows, read in 16-deep chunks of three bf16 planes.
//
// The `_h` forms (hidden size 512) keep the tile and take four column slabs (grid.y = 4): a gate is two consecutive
// 256-row images, and the wave reads the one that holds its columns, n0 / 256.
#pragma once

#include "common.h"
#include "x6_split.h"

namespace rslrl {

constexpr int kLcRows = 64;
constexpr int kLcH = 256;
constexpr int kLcBlockRows = 256;           // rows of one layout-0 image: a gate of the 512 forms is two of them
constexpr int kLcHWide = 512;               // the `_h` forms' hidden size
constexpr int kLcPlaneU = 256 * 2;          // 16-byte units of one plane of one image chunk (layout 0)
constexpr int kLcChunkU = 3 * kLcPlaneU;

__device__ __forceinline__ void lc_split8(const float4& lo4, const float4& hi4, bf16x8 (&f)[3]) {
    uint2 lo[3], hi[3];
    split4(lo4, lo[0], lo[1], lo[2]);
    split4(hi4, hi[0], hi[1], hi[2]);
#pragma unroll
    for (int q = 0; q < 3; ++q) f[q] = __builtin_bit_cast(bf16x8, make_uint4(lo[q].x, lo[q].y, hi[q].x, hi[q].y));
}

// C^T tile: MFMA(w_q, x_p).  One chunk's six products are summed from zero, smallest terms first, and the chunk's
// sum is added to the running accumulator once: the accumulator (the size of a whole gate) is rounded once per chunk
// instead of six times.  With K up to 512 the per-MFMA roundings of a full-size accumulator were the cell's largest
// error against the RNN library's GEMMs.
__device__ __forceinline__ f32x16 lc_mfma(const bf16x8 (&x)[3], const bf16x8 (&w)[3], f32x16 acc) {
    f32x16 t = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w[0], x[2], f32x16{}, 0, 0, 0);
    t = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w[2], x[0], t, 0, 0, 0);
    t = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w[1], x[1], t, 0, 0, 0);
    t = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w[0], x[1], t, 0, 0, 0);
    t = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w[1], x[0], t, 0, 0, 0);
    t = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w[0], x[0], t, 0, 0, 0);
    return acc + t;
}

// The pointwise update runs in fp64 and rounds once per stored value (fp32 expf / tanhf are 1-2 ulp each, which shows
// on sigmoid(f) c once the states are small).
__device__ __forceinline__ double lc_sigmoid(double v) { return 1.0 / (1.0 + exp(-v)); }

}  // namespace rslrl
