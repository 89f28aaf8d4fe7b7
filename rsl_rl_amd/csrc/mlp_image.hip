// Weight images of the split-precision MLP kernels and the bias-gradient fold.
//   rslrl_linear_prepare_bimage(s)  fp32 weights -> the operand images the GEMMs read (layouts in mlp_tile.h): layout 0
//                                   (x6, three bf16 planes), layout 2 (h3, two scaled fp16 planes + row scales) and the
//                                   output layer's image (layout 1); one launch builds every image of an MLP pass
//   rslrl_column_sum_fold           per-tile column sums -> the bias gradient, in a fixed order
#include <algorithm>

#include "common.h"
#include "mlp_tile.h"
#include "x6_split.h"

namespace rslrl {
namespace {

// B image: [chunk][plane][256 rows][32 B swizzled]; element (row n, k) = transposed ? src[k * rows + n] :
// src[n * depth + k], zero for n >= rows or k >= depth.  One thread per (chunk, row, physical half);
// blockIdx.y selects the image of a batch (one launch builds every image an MLP pass needs).
constexpr int kMaxImages = 16;
struct BImageBatch {
    rslrl_bimage_desc_t d[kMaxImages];
};

__device__ __forceinline__ void out_image_thread(const rslrl_bimage_desc_t& dsc, int id) {
    if (id >= kOutImageThreads) return;
    const int o = id & 31, h = (id >> 5) & 1, s = (id >> 6) & 1, j = (id >> 7) & 1, wn = id >> 8;
    float v[8];
#pragma unroll
    for (int t = 0; t < 8; ++t) {
        const int c = wn * 64 + j * 32 + 4 * h + (t & 3) + 8 * (2 * s + (t >> 2));
        v[t] = (o < dsc.rows && c < dsc.depth) ? dsc.src[static_cast<int64_t>(o) * dsc.depth + c] : 0.f;
    }
    uint2 lo[3], hi[3];
    split4(make_float4(v[0], v[1], v[2], v[3]), lo[0], lo[1], lo[2]);
    split4(make_float4(v[4], v[5], v[6], v[7]), hi[0], hi[1], hi[2]);
    uint4* img = static_cast<uint4*>(dsc.image);
#pragma unroll
    for (int q = 0; q < 3; ++q)
        img[out_image_unit(wn, j, s, q, h, o)] = make_uint4(lo[q].x, lo[q].y, hi[q].x, hi[q].y);
    float4* f = reinterpret_cast<float4*>(img + kOutImagePlaneUnits) + 2 * id;  // id = out_image_f32_pair(wn, j, s, h, o)
    f[0] = make_float4(v[0], v[1], v[2], v[3]);
    f[1] = make_float4(v[4], v[5], v[6], v[7]);
}

__global__ __launch_bounds__(kBlock) void bimage_kernel(BImageBatch batch) {
    const rslrl_bimage_desc_t& dsc = batch.d[blockIdx.y];
    if (dsc.layout == RSLRL_BIMAGE_LAYOUT_OUT) {
        out_image_thread(dsc, blockIdx.x * kBlock + threadIdx.x);
        return;
    }
    const int rows = dsc.rows, depth = dsc.depth;
    const float* __restrict__ src = dsc.src;
    const int nchunks = (depth + kKC - 1) / kKC;
    const int id = blockIdx.x * kBlock + threadIdx.x;
    if (dsc.layout == RSLRL_BIMAGE_LAYOUT_H3) {
        // depth <= 256: the 16 chunks x 2 halves of row n are the 32 lanes of a half wave, so the row's max
        // (-> its scale t_n) is a 32-lane shuffle reduction of the lanes' own 8 values
        if (id >= kBN * 32) return;  // whole half waves exit together
        const int n = id >> 5;
        const int c = (id >> 1) & 15;
        const int ph = id & 1;
        const int lh = ph ^ ((n >> 3) & 1);
        float v[8];
        float m = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int k = 16 * c + 8 * lh + j;
            v[j] = (n < rows && k < depth) ? src[dsc.transposed ? static_cast<int64_t>(k) * rows + n
                                                                : static_cast<int64_t>(n) * depth + k]
                                           : 0.f;
            m = fmaxf(m, fabsf(v[j]));
        }
#pragma unroll
        for (int off = 16; off >= 1; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, 32));
        const float t = h3_scale(m);
        if (c < nchunks) {
            uint2 lo[2], hi[2];
            split4_h(make_float4(v[0] * t, v[1] * t, v[2] * t, v[3] * t), lo[0], lo[1]);
            split4_h(make_float4(v[4] * t, v[5] * t, v[6] * t, v[7] * t), hi[0], hi[1]);
            uint4* base = static_cast<uint4*>(dsc.image) + static_cast<int64_t>(c) * (kH3ChunkB / 16) +
                          (n * kX6RowB + 16 * ph) / 16;
#pragma unroll
            for (int q = 0; q < 2; ++q) base[q * (kX6PlaneB / 16)] = make_uint4(lo[q].x, lo[q].y, hi[q].x, hi[q].y);
        }
        if (c == 0 && ph == 0)
            reinterpret_cast<float*>(static_cast<char*>(dsc.image) + h3_image_scales_offset(depth))[n] = 1.f / t;
        return;
    }
    if (id >= nchunks * kBN * 2) return;
    const int c = id / (kBN * 2);
    const int n = (id >> 1) % kBN;
    const int ph = id & 1;
    const int lh = ph ^ ((n >> 3) & 1);
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int k = 16 * c + 8 * lh + j;
        v[j] = (n < rows && k < depth) ? src[dsc.transposed ? static_cast<int64_t>(k) * rows + n
                                                            : static_cast<int64_t>(n) * depth + k]
                                       : 0.f;
    }
    uint2 lo[3], hi[3];
    split4(make_float4(v[0], v[1], v[2], v[3]), lo[0], lo[1], lo[2]);
    split4(make_float4(v[4], v[5], v[6], v[7]), hi[0], hi[1], hi[2]);
    uint4* base = static_cast<uint4*>(dsc.image) + static_cast<int64_t>(c) * (kX6ChunkB / 16) +
                  (n * kX6RowB + 16 * ph) / 16;
#pragma unroll
    for (int q = 0; q < 3; ++q) base[q * (kX6PlaneB / 16)] = make_uint4(lo[q].x, lo[q].y, hi[q].x, hi[q].y);
}

// Bias gradient: out[col] = sum over tiles of part[tiles][N], in two launches and a fixed order.  Pass 1:
// workgroup (column group of 64, slice s) sums the slice's tiles (4 phases of 64 columns, fp64, phases
// folded in order) and leaves the slice sum in the slice's first row (that element was read by the same
// thread); pass 2 adds the slice sums in order.  The partials are scratch: pass 1 overwrites them.
constexpr int kFoldCols = 64;
constexpr int kFoldPhases = kBlock / kFoldCols;
constexpr int kFoldSlices = 64;
__global__ __launch_bounds__(kBlock) void colsum_slice_kernel(float* __restrict__ part, int tiles, int n, int per) {
    __shared__ double scratch[kFoldPhases][kFoldCols];
    const int c = threadIdx.x % kFoldCols, ph = threadIdx.x / kFoldCols;
    const int col = blockIdx.x * kFoldCols + c;
    const int t0 = blockIdx.y * per;
    const int t1 = t0 + per < tiles ? t0 + per : tiles;
    double s = 0.0;
    if (col < n) {
#pragma unroll 4
        for (int t = t0 + ph; t < t1; t += kFoldPhases) s += static_cast<double>(part[static_cast<int64_t>(t) * n + col]);
    }
    scratch[ph][c] = s;
    __syncthreads();
    if (ph == 0 && col < n) {
        double tot = 0.0;
        for (int q = 0; q < kFoldPhases; ++q) tot += scratch[q][c];
        part[static_cast<int64_t>(t0) * n + col] = static_cast<float>(tot);
    }
}

// pass 2: thread (group g, column c) loads slices g, g + 4, ... (<= 16, all loads issued before the adds) and the
// four group sums are added in g order
__global__ __launch_bounds__(kBlock) void colsum_fold_kernel(const float* __restrict__ part, int slices, int n,
                                                             int per, float* __restrict__ out) {
    __shared__ double scratch[kFoldPhases][kFoldCols];
    const int c = threadIdx.x % kFoldCols, g = threadIdx.x / kFoldCols;
    const int col = blockIdx.x * kFoldCols + c;
    constexpr int kMaxPer = kFoldSlices / kFoldPhases;
    float v[kMaxPer];
#pragma unroll
    for (int i = 0; i < kMaxPer; ++i) {
        const int s = g + kFoldPhases * i;
        v[i] = (col < n && s < slices) ? part[static_cast<int64_t>(s) * per * n + col] : 0.f;
    }
    double tot = 0.0;
#pragma unroll
    for (int i = 0; i < kMaxPer; ++i) tot += static_cast<double>(v[i]);
    scratch[g][c] = tot;
    __syncthreads();
    if (g == 0 && col < n) {
        double t = 0.0;
        for (int q = 0; q < kFoldPhases; ++q) t += scratch[q][c];
        out[col] = static_cast<float>(t);
    }
}

}  // namespace
}  // namespace rslrl

using namespace rslrl;

extern "C" size_t rslrl_linear_bimage_bytes(int32_t depth) {
    return depth < 1 ? 0 : static_cast<size_t>(ceil_div(static_cast<int64_t>(depth), kKC)) * kX6ChunkB;
}

extern "C" size_t rslrl_linear_bimage_h3_bytes(int32_t depth) {
    return depth < 1 ? 0 : static_cast<size_t>(h3_image_scales_offset(depth)) + kBN * sizeof(float);
}

extern "C" int rslrl_linear_prepare_bimages(const rslrl_bimage_desc_t* descs, int32_t n, rslrl_stream_t stream) {
    if (!descs || n < 1 || n > kMaxImages) return RSLRL_E_INVALID_ARGUMENT;
    BImageBatch batch{};
    int max_chunks = 0;
    int max_threads = 0;
    for (int i = 0; i < n; ++i) {
        const rslrl_bimage_desc_t& d = descs[i];
        if (!d.src || !d.image || d.rows < 1 || d.rows > kBN || d.depth < 1 || d.depth > (1 << 24))
            return RSLRL_E_INVALID_ARGUMENT;
        if (reinterpret_cast<uintptr_t>(d.image) & 15) return RSLRL_E_MISALIGNED;
        if (d.layout == RSLRL_BIMAGE_LAYOUT_OUT) {
            if (d.rows > kMaxOutWidth || d.depth > kBN || d.transposed) return RSLRL_E_INVALID_ARGUMENT;
            max_threads = std::max(max_threads, kOutImageThreads);
        } else if (d.layout == RSLRL_BIMAGE_LAYOUT_H3) {
            if (d.depth > kBN) return RSLRL_E_INVALID_ARGUMENT;
            max_threads = std::max(max_threads, kBN * 32);
        } else if (d.layout == RSLRL_BIMAGE_LAYOUT_GEMM) {
            max_chunks = std::max(max_chunks, static_cast<int>(ceil_div(static_cast<int64_t>(d.depth), kKC)));
        } else {
            return RSLRL_E_INVALID_ARGUMENT;
        }
        batch.d[i] = d;
    }
    max_threads = std::max(max_threads, max_chunks * kBN * 2);
    const dim3 grid(static_cast<unsigned>(ceil_div(max_threads, kBlock)), static_cast<unsigned>(n));
    hipLaunchKernelGGL(bimage_kernel, grid, dim3(kBlock), 0, reinterpret_cast<hipStream_t>(stream), batch);
    return launch_status();
}

extern "C" int rslrl_linear_prepare_bimage(const float* src, int32_t rows, int32_t depth, int32_t transposed,
                                           void* image, rslrl_stream_t stream) {
    const rslrl_bimage_desc_t d{src, image, rows, depth, transposed ? 1 : 0, RSLRL_BIMAGE_LAYOUT_GEMM};
    return rslrl_linear_prepare_bimages(&d, 1, stream);
}

extern "C" size_t rslrl_linear_out_image_bytes(void) { return static_cast<size_t>(kOutImageUnits) * 16; }

extern "C" int rslrl_column_sum_fold(float* partials, int64_t tiles, int32_t N, float* out,
                                     rslrl_stream_t stream) {
    if (tiles < 1 || tiles > INT32_MAX || N < 1 || !partials || !out) return RSLRL_E_INVALID_ARGUMENT;
    const int per = static_cast<int>(ceil_div(tiles, kFoldSlices));
    const int slices = static_cast<int>(ceil_div(tiles, per));
    const unsigned cg = static_cast<unsigned>(ceil_div(N, kFoldCols));
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(colsum_slice_kernel, dim3(cg, static_cast<unsigned>(slices)), dim3(kBlock), 0, st, partials,
                       static_cast<int>(tiles), N, per);
    hipLaunchKernelGGL(colsum_fold_kernel, dim3(cg), dim3(kBlock), 0, st, partials, slices, N, per, out);
    return launch_status();
}
