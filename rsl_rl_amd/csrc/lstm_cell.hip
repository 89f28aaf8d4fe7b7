// One LSTM time step for M rows in one launch on gfx950 (rslrl_lstm_cell / rslrl_lstm_cell_pair, ABI 25): the rollout's
// Memory.forward of rsl_rl/networks/memory.py:37 for one layer of hidden size 256 -- what the RNN library runs as two
// GEMMs and a pointwise launch, and what the storage's pre-step states are copied around.
//
//   gates = x W_ih^T + b_ih + h W_hh^T + b_hh   (torch's order i, f, g, o; four blocks of 256 rows)
//   c' = sigmoid(f) c + sigmoid(i) tanh(g),  h' = sigmoid(o) tanh(c')       h / c NULL: zeros (the step after reset())
//
// Arithmetic: the project's fp32-faithful x6 split-bf16 MFMA (x6_split.h), fp32 accumulation, over K = D + 256 in
// 16-deep chunks of [x | h]; the pointwise update in fp64, rounded once per stored value.
// Weights: per gate one layout-0 image of the 256 rows of
// [W_ih | W_hh] (rslrl_lstm_prepare_image: the chunks of W_ih, then those of W_hh -- D is a multiple of 16, so no
// chunk straddles the two -- built by rslrl_linear_prepare_bimages in one launch).
//
// Tile: a workgroup of 4 waves owns 64 rows and 128 hidden columns (grid: M / 64 x 2 x problems); wave w owns the 32
// columns n0 = 128 y + 32 w of ALL FOUR gates for the 64 rows: 4 gates x 2 row blocks of 32 x 32 C^T accumulators
// (128 registers), so that a lane holds i, f, g and o of the same (row, column) and the whole cell update is
// register-local: lane (l32, h) of row block i holds row 32 i + l32 and columns n0 + (r & 3) + 8 (r >> 2) + 4 h.
// The [x | h] fragments (row 32 i + l32, k = 16 c + 8 h .. + 7) are read from global memory as fp32 and split on read;
// weight fragments come straight from the images (L2-resident).  No LDS, no barrier, deterministic.

#include "common.h"
#include "x6_split.h"

namespace rslrl {
namespace {

constexpr int kLcRows = 64;
constexpr int kLcH = 256;
constexpr int kLcPlaneU = 256 * 2;          // 16-byte units of one plane of one image chunk (layout 0)
constexpr int kLcChunkU = 3 * kLcPlaneU;

struct LcProblem {
    const float* x;     // [M, D]
    const float* h;     // [M, 256] or null
    const float* c;     // [M, 256] or null
    const uint4* image; // 4 gate images of depth D + 256
    const float* b_ih;  // [1024]
    const float* b_hh;  // [1024]
    float* h_out;       // [M, 256]
    float* c_out;       // [M, 256]
    int D;
};

struct LcArgs {
    LcProblem p[2];
};

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

__global__ __launch_bounds__(kBlock) void lstm_cell_kernel(LcArgs args) {
    const LcProblem& P = args.p[blockIdx.z];
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int hh = lane >> 5;
    const int l32 = lane & 31;
    const int64_t row0 = static_cast<int64_t>(blockIdx.x) * kLcRows;
    const int n0 = 128 * blockIdx.y + 32 * wave;
    const int kc_x = P.D / 16;
    const int kc = kc_x + (P.h ? kLcH / 16 : 0);  // h == null: its chunks contribute nothing
    const int gate_units = (kc_x + kLcH / 16) * kLcChunkU;
    // weight fragment of image row n = n0 + l32, logical half hh (physical half swapped when (n >> 3) & 1)
    const int wunit = (n0 + l32) * 2 + (hh ^ ((l32 >> 3) & 1));

    f32x16 acc[4][2];
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
        for (int i = 0; i < 2; ++i) acc[g][i] = f32x16{};

    for (int c = 0; c < kc; ++c) {
        bf16x8 xf[2][3];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int64_t r = row0 + 32 * i + l32;
            const float* src = c < kc_x ? P.x + r * P.D + 16 * c + 8 * hh : P.h + r * kLcH + 16 * (c - kc_x) + 8 * hh;
            const float4 lo = *reinterpret_cast<const float4*>(src);
            const float4 hi = *reinterpret_cast<const float4*>(src + 4);
            lc_split8(lo, hi, xf[i]);
        }
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            bf16x8 wf[3];
            const uint4* img = P.image + static_cast<int64_t>(g) * gate_units + c * kLcChunkU + wunit;
#pragma unroll
            for (int q = 0; q < 3; ++q) wf[q] = __builtin_bit_cast(bf16x8, img[q * kLcPlaneU]);
#pragma unroll
            for (int i = 0; i < 2; ++i) acc[g][i] = lc_mfma(xf[i], wf, acc[g][i]);
        }
    }

    // the cell update, register-local: 4 column quads per row block
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int64_t r = row0 + 32 * i + l32;
#pragma unroll
        for (int qd = 0; qd < 4; ++qd) {
            const int n = n0 + 8 * qd + 4 * hh;
            float gate[4][4];
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const float4 bi = *reinterpret_cast<const float4*>(P.b_ih + g * kLcH + n);
                const float4 bh = *reinterpret_cast<const float4*>(P.b_hh + g * kLcH + n);
                const float bia[4] = {bi.x, bi.y, bi.z, bi.w}, bha[4] = {bh.x, bh.y, bh.z, bh.w};
#pragma unroll
                for (int e = 0; e < 4; ++e) gate[g][e] = (acc[g][i][4 * qd + e] + bia[e]) + bha[e];
            }
            float4 cp = make_float4(0.f, 0.f, 0.f, 0.f);
            if (P.c) cp = *reinterpret_cast<const float4*>(P.c + r * kLcH + n);
            const float cpa[4] = {cp.x, cp.y, cp.z, cp.w};
            float cn[4], hn[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const double cd = lc_sigmoid(static_cast<double>(gate[1][e])) * static_cast<double>(cpa[e]) +
                                  lc_sigmoid(static_cast<double>(gate[0][e])) * tanh(static_cast<double>(gate[2][e]));
                cn[e] = static_cast<float>(cd);
                hn[e] = static_cast<float>(lc_sigmoid(static_cast<double>(gate[3][e])) *
                                           tanh(static_cast<double>(cn[e])));  // of the stored c'
            }
            *reinterpret_cast<float4*>(P.c_out + r * kLcH + n) = make_float4(cn[0], cn[1], cn[2], cn[3]);
            *reinterpret_cast<float4*>(P.h_out + r * kLcH + n) = make_float4(hn[0], hn[1], hn[2], hn[3]);
        }
    }
}

int lc_check(const rslrl_lstm_cell_t* a, int64_t M) {
    if (!a) return RSLRL_E_INVALID_ARGUMENT;
    if (a->hidden != kLcH || a->layers != 1 || a->D < 16 || a->D > 256 || a->D % 16 || M < kLcRows || M % kLcRows ||
        M > (INT64_C(1) << 31))
        return RSLRL_E_UNSUPPORTED;
    if (!a->x || !a->image || !a->b_ih || !a->b_hh || !a->h_out || !a->c_out) return RSLRL_E_INVALID_ARGUMENT;
    // every block reads whole rows of h while others write h_out: they must not be one buffer (c_out may be c)
    if (a->h_out == a->h || a->h_out == a->c_out) return RSLRL_E_INVALID_ARGUMENT;
    const uintptr_t ptrs[] = {reinterpret_cast<uintptr_t>(a->x),     reinterpret_cast<uintptr_t>(a->h),
                              reinterpret_cast<uintptr_t>(a->c),     reinterpret_cast<uintptr_t>(a->image),
                              reinterpret_cast<uintptr_t>(a->b_ih),  reinterpret_cast<uintptr_t>(a->b_hh),
                              reinterpret_cast<uintptr_t>(a->h_out), reinterpret_cast<uintptr_t>(a->c_out)};
    for (uintptr_t p : ptrs)
        if (p & 15) return RSLRL_E_MISALIGNED;
    return RSLRL_OK;
}

LcProblem lc_problem(const rslrl_lstm_cell_t* a) {
    return LcProblem{a->x, a->h, a->c, static_cast<const uint4*>(a->image), a->b_ih, a->b_hh, a->h_out, a->c_out, a->D};
}

}  // namespace
}  // namespace rslrl

using namespace rslrl;

extern "C" size_t rslrl_lstm_image_bytes(int32_t D) {
    if (D < 16 || D > 256 || D % 16) return 0;
    return 4 * rslrl_linear_bimage_bytes(D + kLcH);
}

extern "C" int rslrl_lstm_prepare_image(const float* w_ih, const float* w_hh, int32_t D, int32_t hidden, void* image,
                                        rslrl_stream_t stream) {
    if (hidden != kLcH || D < 16 || D > 256 || D % 16) return RSLRL_E_UNSUPPORTED;
    if (!w_ih || !w_hh || !image) return RSLRL_E_INVALID_ARGUMENT;
    if (reinterpret_cast<uintptr_t>(image) & 15) return RSLRL_E_MISALIGNED;
    const size_t gate_bytes = rslrl_linear_bimage_bytes(D + kLcH);
    const size_t x_bytes = rslrl_linear_bimage_bytes(D);
    rslrl_bimage_desc_t d[8];
    for (int g = 0; g < 4; ++g) {
        char* base = static_cast<char*>(image) + g * gate_bytes;
        d[2 * g] = rslrl_bimage_desc_t{w_ih + static_cast<int64_t>(g) * kLcH * D, base, kLcH, D, 0,
                                       RSLRL_BIMAGE_LAYOUT_GEMM};
        d[2 * g + 1] = rslrl_bimage_desc_t{w_hh + static_cast<int64_t>(g) * kLcH * kLcH, base + x_bytes, kLcH, kLcH, 0,
                                           RSLRL_BIMAGE_LAYOUT_GEMM};
    }
    return rslrl_linear_prepare_bimages(d, 8, stream);
}

extern "C" int rslrl_lstm_cell_pair(const rslrl_lstm_cell_t* a0, const rslrl_lstm_cell_t* a1, int64_t M,
                                    rslrl_stream_t stream) {
    int rc = lc_check(a0, M);
    if (rc != RSLRL_OK) return rc;
    LcArgs args{};
    args.p[0] = lc_problem(a0);
    unsigned np = 1;
    if (a1) {
        rc = lc_check(a1, M);
        if (rc != RSLRL_OK) return rc;
        args.p[1] = lc_problem(a1);
        np = 2;
    }
    hipLaunchKernelGGL(lstm_cell_kernel, dim3(static_cast<unsigned>(M / kLcRows), 2, np), dim3(kBlock), 0,
                       reinterpret_cast<hipStream_t>(stream), args);
    return launch_status();
}

extern "C" int rslrl_lstm_cell(const rslrl_lstm_cell_t* a, int64_t M, rslrl_stream_t stream) {
    return rslrl_lstm_cell_pair(a, nullptr, M, stream);
}
