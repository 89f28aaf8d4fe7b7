// The tile of the heads for a last hidden layer with 128 inputs, shared by the units that launch them
// (mlp_heads_k128.hip: the critic and 5 to 16 actions; mlp_heads_wide_k128.hip: 17 to 32 actions): the x planes and
// their staging, the main loop on weight fragments from L2, H = ELU(acc + b), the H stage and the dZ store, and the
// host's slice rule.  The geometry and the LDS images are described at the top of mlp_heads_k128.hip.
#pragma once

#include <algorithm>

#include "common.h"
#include "mlp_gemm_x6.h"

namespace rslrl {
namespace {

constexpr int kKhT = 64;                      // rows per tile
constexpr int kKhK = 128;                     // the layer's input width
constexpr int kKhThreads = 256;               // 4 waves
constexpr int kKhPlane = kKhT * kKhK * 2;     // one bf16 plane of the x tile: 16 KiB
constexpr int kKhXBytes = 3 * kKhPlane;       // 48 KiB
constexpr int kKhChunks = kKhK / kKC;         // 8
constexpr int kKhMaxSlices = 512;             // two workgroups on each of the 256 CUs

struct KhArgs {
    GemmParams p;
    const uint4* img;  // layout-0 image of W [N, 128]: 8 chunks
    int tiles;         // M / 64
    int tiles_per;     // tiles per slice
};

__host__ __device__ constexpr int kh_f(int c) { return (c & 3) | (((c & 1) ^ (c >> 2)) << 2); }

// byte offset of (row m, column col % 4 == 0) in an x plane
__device__ __forceinline__ int kh_x_off(int m, int col) {
    const int c = col >> 4;
    return c * (kKhT * 32) + (m ^ kh_f(c)) * 32 + 16 * (((col >> 3) & 1) ^ ((m >> 3) & 1)) + 8 * ((col >> 2) & 1);
}

constexpr uint32_t kKhRsrcFlags = 0x00020000;

// the tile's x, 8 float4 per thread: row (t >> 5) + 8 i, columns 4 (t & 31) .. + 3, through a buffer resource over the
// tile's 32 KiB (nontemporal: read once)
__device__ __forceinline__ void kh_load_x(const float* x, int64_t row0, float4 (&v)[8]) {
    const __amdgpu_buffer_rsrc_t r =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(x + row0 * kKhK), 0, kKhT * kKhK * 4, kKhRsrcFlags);
    const int off = ((threadIdx.x >> 5) * kKhK + 4 * (threadIdx.x & 31)) * 4;
#pragma unroll
    for (int i = 0; i < 8; ++i)
        v[i] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(r, off, i * 8 * kKhK * 4, 2));
}

__device__ __forceinline__ void kh_store_x(const float4 (&v)[8], char* __restrict__ lds) {
    const int col = 4 * (threadIdx.x & 31);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        uint2 w[3];
        split4(v[i], w[0], w[1], w[2]);
        const int off = kh_x_off((threadIdx.x >> 5) + 8 * i, col);
#pragma unroll
        for (int q = 0; q < 3; ++q) *reinterpret_cast<uint2*>(lds + q * kKhPlane + off) = w[q];
    }
}

__device__ __forceinline__ bf16x8 kh_read16(int addr) {
    typedef __attribute__((address_space(3))) uint4 lds_u4;
    return __builtin_bit_cast(bf16x8, *reinterpret_cast<const lds_u4*>(addr));
}

// LDS writes retired, then the barrier: __syncthreads would also wait out the next tile's x loads
__device__ __forceinline__ void kh_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// float index of (row r, float4 quad) in the H stage of row length N
template <int N>
__device__ __forceinline__ int kh_stage_idx(int r, int quad) { return r * N + 4 * (quad ^ (r & 15)); }

// What both heads share around their loss: the wave's place in the tile, the main loop, H, the stage and the dZ store
template <int NW>
struct KhTile {
    static constexpr int kN = 64 * NW;    // the layer's width
    static constexpr int kRG = 4 / NW;    // row groups of the column walk
    static constexpr int kRPG = 16 * NW;  // rows per group
    int lane, wave, ib, wn, l32, h;
    bool live;   // this wave holds H columns (wave-uniform)
    int la[kKhChunks];  // LDS addresses of the x fragments: row 32 ib + l32, columns 16 c + 8 h ..
    int boff;           // image row 64 wn + l32, half h (the j = 1 block: + 1 KiB)
    __amdgpu_buffer_rsrc_t rimg;
    int c, rg;   // the column walk: column c of rows [kRPG rg, kRPG rg + kRPG)

    __device__ __forceinline__ void init(const char* lds, const uint4* img) {
        lane = threadIdx.x & 63;
        wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
        ib = wave >> 1;
        wn = wave & 1;
        l32 = lane & 31;
        h = lane >> 5;
        live = wn < NW;
        const int lbase = static_cast<int>(reinterpret_cast<uintptr_t>(lds));
#pragma unroll
        for (int c2 = 0; c2 < kKhChunks; ++c2) la[c2] = lbase + kh_x_off(32 * ib + l32, 16 * c2 + 8 * h);
        boff = swz(64 * wn + l32, h);
        rimg = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint4*>(img), 0,
                                                 static_cast<uint32_t>(kKhChunks * kX6ChunkB), kKhRsrcFlags);
        c = 64 * (wave % NW) + lane;
        rg = wave / NW;
    }

    // acc[j]: lane (l32, h) holds row 32 ib + l32, columns 64 wn + 32 j + (r & 3) + 8 (r >> 2) + 4 h
    __device__ __forceinline__ void main_loop(f32x16 (&acc)[2]) const {
        acc[0] = f32x16{};
        acc[1] = f32x16{};
        if (!live) return;
        auto bload = [&](int ch, int j, int q) {
            return __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(
                                                 rimg, boff, ch * kX6ChunkB + q * kX6PlaneB + j * 32 * kX6RowB, 0));
        };
        uint4 bq[2][2][3];  // ring of image chunks
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int q = 0; q < 3; ++q) bq[0][j][q] = bload(0, j, q);
#pragma unroll
        for (int ch = 0; ch < kKhChunks; ++ch) {
            if (ch + 1 < kKhChunks) {
#pragma unroll
                for (int j = 0; j < 2; ++j)
#pragma unroll
                    for (int q = 0; q < 3; ++q) bq[(ch + 1) & 1][j][q] = bload(ch + 1, j, q);
            }
            bf16x8 af[3];
#pragma unroll
            for (int q = 0; q < 3; ++q) af[q] = kh_read16(la[ch] + q * kKhPlane);
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                bf16x8 bf[3];
#pragma unroll
                for (int q = 0; q < 3; ++q) bf[q] = __builtin_bit_cast(bf16x8, bq[ch & 1][j][q]);
                acc[j] = Arith<3>::mfma(bf, af, acc[j]);  // C^T tile: the weight fragment is the MFMA's A operand
            }
            __builtin_amdgcn_sched_barrier(0);  // one chunk's fragments ahead, no more
        }
    }

    // H = ELU(acc + b) in place (the forward epilogue's expression), bias [N] in LDS
    __device__ __forceinline__ void elu_bias(f32x16 (&acc)[2], const float* bias) const {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int cb = wn * 64 + j * 32 + 4 * h;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const float4 b4 = *reinterpret_cast<const float4*>(bias + cb + 8 * g);
                float tt[4] = {acc[j][4 * g], acc[j][4 * g + 1], acc[j][4 * g + 2], acc[j][4 * g + 3]};
                tt[0] += b4.x;
                tt[1] += b4.y;
                tt[2] += b4.z;
                tt[3] += b4.w;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float n = elu_neg(fminf(tt[e], 0.f));
                    acc[j][4 * g + e] = tt[e] > 0.f ? tt[e] : n;
                }
            }
        }
    }

    __device__ __forceinline__ void stage_h(const f32x16 (&acc)[2], float* stg) const {
        const int r = 32 * ib + l32;
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const f32x4 hv = {acc[j][4 * g], acc[j][4 * g + 1], acc[j][4 * g + 2], acc[j][4 * g + 3]};
                *reinterpret_cast<f32x4*>(stg + kh_stage_idx<kN>(r, wn * 16 + j * 8 + 2 * g + h)) = hv;
            }
    }

    // the wave's kRPG x 64 region of dZ out of the stage: 4 rows of 256 bytes per instruction
    __device__ __forceinline__ void store_dz(const float* stg, float* dz, int64_t row0, int nt) const {
        __builtin_amdgcn_wave_barrier();  // one wave's LDS accesses execute in order
        const int cw = 64 * (wave % NW);
        float* ct = dz + (row0 + kRPG * rg) * kN + cw;
#pragma unroll
        for (int k = 0; k < kRPG / 4; ++k) {
            const int sr = 4 * k + (lane >> 4), cq = lane & 15;
            const f32x4 v = *reinterpret_cast<const f32x4*>(stg + kh_stage_idx<kN>(kRPG * rg + sr, (cw >> 2) + cq));
            f32x4* dst = reinterpret_cast<f32x4*>(ct + sr * kN + 4 * cq);
            if (nt) __builtin_nontemporal_store(v, dst);
            else *dst = v;
        }
        __builtin_amdgcn_wave_barrier();
    }
};

bool kh_shape_ok(const rslrl_linear_args_t* a) {
    return a->arith == RSLRL_ARITH_X6 && a->K == kKhK && (a->N == 64 || a->N == 128) && a->M >= kKhT &&
           a->M % kKhT == 0 && a->M / kKhT <= INT32_MAX;
}

// Tiles per slice: one while the tiles fit two workgroups per CU, above that as few as keep the slices within that.  A
// slice's partial row is at most 8 KiB against the 64 KiB a tile streams, so no minimum (the 128-wide hidden
// backward's 64.5 KiB row needs two).  24,576 rows: 384 slices of 1; 393,216 rows: 512 slices of 12.
int64_t kh_tiles_per(int64_t tiles) { return std::max<int64_t>(1, ceil_div(tiles, kKhMaxSlices)); }

int64_t kh_slices(int64_t M) {
    const int64_t tiles = M / kKhT;
    return ceil_div(tiles, kh_tiles_per(tiles));
}

KhArgs kh_args(const rslrl_linear_args_t* a, const GemmParams& p) {
    const int64_t tiles = a->M / kKhT;
    return KhArgs{p, static_cast<const uint4*>(a->bimage), static_cast<int>(tiles),
                  static_cast<int>(kh_tiles_per(tiles))};
}

}  // namespace
}  // namespace rslrl
