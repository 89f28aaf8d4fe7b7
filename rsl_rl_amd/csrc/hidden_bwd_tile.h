// The 64-row tile of the fused hidden-layer backward kernels whose dZ is 128 columns wide (mlp_bwd_fused_n.hip:
// Linear(128, 128); mlp_bwd_fused_kn.hip: Linear(256, 128)): the dZ tile as three resident bf16 planes, a wave's 8 KiB
// H region, and the loads, DMAs and LDS reads of both.  The layer input H and the input gradient dZp are addressed at
// a row stride of their own (kStride: 128 or 256 floats).
//
// LDS image of a dZ plane: [8 chunks of 16 columns][64 row slots][32 bytes]; row m of chunk c in slot m ^ f(c),
// f(c) = (c & 3) | 4 ((c & 1) ^ (c >> 2)) = 0 5 2 7 4 1 6 3, its two 16-byte halves swapped when (m >> 3) & 1.
// Bank-conflict free (64 banks of 4 bytes) for all three accesses:
//  - staging stores (ds_write_b64; 32 lanes = one row of all 8 chunks, 4 lanes per chunk): f(c) mod 8 is a permutation
//    of 0..7, so every chunk's 32 bytes take their own 8 banks;
//  - row-fragment reads (ds_read_b128, one chunk per instruction, 16 lanes = rows m .. m + 15 of one half): rows m and
//    m + 8 share slot mod 8 and are separated by the half swap;
//  - transposed reads (ds_read_b64_tr_b16, 32 lanes = 4 consecutive rows of chunks 2 nb and 2 nb + 1, 32 bytes each):
//    the rows of one chunk take four slots mod 8 of one 4-aligned group, and bit 2 of f differs between an even chunk
//    and its successor, which puts the odd chunk's rows on the other 32 banks.
// f < 8 and the row steps of the fragments are multiples of 16, so every chunk, plane and row-step offset lands in the
// instructions' immediate fields: 8 + 8 address registers for the whole slice.
// H stage: wave w's region is [64 row slots][32 columns] fp32, row r in slot r ^ ((r >> 2) & 1) (rows r and r + 4, the
// two lane halves of one accumulator-layout read, on opposite bank halves), as in the 256-wide kernel.
#pragma once

#include "common.h"
#include "x6_split.h"

namespace rslrl {

constexpr int kHnT = 64;                        // rows per tile
constexpr int kHnW = 128;                       // columns of dZ (the reduction of the input gradient)
constexpr int kHnThreads = 256;                 // 4 waves
constexpr int kHnPlane = kHnT * kHnW * 2;       // one bf16 plane of the dZ tile: 16 KiB
constexpr int kHnDzBytes = 3 * kHnPlane;        // 48 KiB
constexpr int kHnHRegion = kHnT * 32 * 4;       // a wave's H region: 8 KiB
constexpr int kHnHBytes = 4 * kHnHRegion;       // the H stage: 32 KiB
constexpr int kHnLds = kHnDzBytes + kHnHBytes;  // 80 KiB: two workgroups per CU
constexpr int kHnChunks = kHnW / 16;            // k-chunks of the input gradient
constexpr int kHnChunkB = kHnT * 32;            // one chunk of one plane: 2 KiB
constexpr int kHnImgPlaneU = 256 * 32 / 16;     // 16-byte units of one (256-row) plane of an image chunk
constexpr int kHnImgChunkU = 3 * kHnImgPlaneU;

using s16x4 = __attribute__((ext_vector_type(4))) short;
using u32x4 = __attribute__((ext_vector_type(4))) unsigned int;

__host__ __device__ constexpr int hn_f(int c) { return (c & 3) | (((c & 1) ^ (c >> 2)) << 2); }

// byte offset of (row m, column col % 4 == 0) in a plane
__device__ __forceinline__ int hn_dz_off(int m, int col) {
    const int c = col >> 4;
    return c * kHnChunkB + (m ^ hn_f(c)) * 32 + 16 * (((col >> 3) & 1) ^ ((m >> 3) & 1)) + 8 * ((col >> 2) & 1);
}

constexpr uint32_t kHnRsrcFlags = 0x00020000;
constexpr uint32_t kHnTileBytes = kHnT * kHnW * 4;  // 32 KiB: one tile of an [M, 128] array

// a buffer resource over the tile's rows of an [M, kStride] fp32 array: loads past the tile return 0, stores are
// dropped
template <int kStride = kHnW>
__device__ __forceinline__ __amdgpu_buffer_rsrc_t hn_tile_rsrc(const float* base, int64_t row0) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(base + row0 * kStride), 0, kHnT * kStride * 4,
                                             kHnRsrcFlags);
}

// the tile's dZ, 8 float4 per thread: row (t >> 5) + 8 i, columns 4 (t & 31) .. + 3; nontemporal (read once: it
// should not push the W^T image out of L2)
__device__ __forceinline__ void hn_load_dz(__amdgpu_buffer_rsrc_t r, float4 (&v)[8]) {
    const int off = ((threadIdx.x >> 5) * kHnW + 4 * (threadIdx.x & 31)) * 4;
#pragma unroll
    for (int i = 0; i < 8; ++i)
        v[i] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(r, off, i * 8 * kHnW * 4, 2));
}

__device__ __forceinline__ void hn_store_dz(const float4 (&v)[8], char* __restrict__ lds, float4& csum) {
    const int col = 4 * (threadIdx.x & 31);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int m = (threadIdx.x >> 5) + 8 * i;
        csum.x += v[i].x;
        csum.y += v[i].y;
        csum.z += v[i].z;
        csum.w += v[i].w;
        uint2 w[3];
        split4(v[i], w[0], w[1], w[2]);
        const int off = hn_dz_off(m, col);
#pragma unroll
        for (int q = 0; q < 3; ++q) *reinterpret_cast<uint2*>(lds + q * kHnPlane + off) = w[q];
    }
}

__device__ __forceinline__ int hn_hslot(int r) { return r ^ ((r >> 2) & 1); }

// the tile's H columns [col0 + 32 w, col0 + 32 w + 32) into wave w's region: instruction i fills slots 8 i .. 8 i + 7
// (lane l: slot 8 i + l / 8, 16 bytes of column quad l % 8).  Issued as asm statements: the compiler orders every later
// LDS read behind a DMA it knows of with vmcnt(0) -- an HBM round trip in the middle of the weight gradient -- while
// nothing reads the region before the wave's own vmcnt(0) ahead of the next epilogue.  M0 (the LDS destination) is set
// and restored in the statement.
template <int kStride = kHnW>
__device__ __forceinline__ void hn_dma_h(__amdgpu_buffer_rsrc_t r, char* stage, int col0 = 0) {
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    // slot ^ row differ in bit 0 only
    const int off = (hn_hslot(lane >> 3) * kStride + col0 + 32 * wave + 4 * (lane & 7)) * 4;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const uint32_t dst = static_cast<uint32_t>(reinterpret_cast<uintptr_t>(stage)) + wave * kHnHRegion + i * 1024;
        const int soff = i * 8 * kStride * 4;
        uint32_t keep;
        asm volatile(
            "s_mov_b32 %0, m0\n\ts_mov_b32 m0, %1\n\ts_nop 0\n\tbuffer_load_dwordx4 %2, %3, %4 offen nt lds\n\t"
            "s_mov_b32 m0, %0"
            : "=&s"(keep)
            : "s"(dst), "v"(off), "s"(r), "s"(soff)
            : "memory");
    }
}

// one 4-row transposed read (ds_read_b64_tr_b16) at byte address addr of the LDS
__device__ __forceinline__ s16x4 hn_tr(int addr) {
    typedef __attribute__((address_space(3))) s16x4 lds_s16x4;
    return __builtin_amdgcn_ds_read_tr16_b64_v4i16(reinterpret_cast<lds_s16x4*>(addr));
}

__device__ __forceinline__ bf16x8 hn_cat(s16x4 lo, s16x4 hi) {
    const __attribute__((ext_vector_type(8))) short v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    return __builtin_bit_cast(bf16x8, v);
}

__device__ __forceinline__ bf16x8 hn_read16(int addr) {
    typedef __attribute__((address_space(3))) uint4 lds_u4;
    return __builtin_bit_cast(bf16x8, *reinterpret_cast<const lds_u4*>(addr));
}

}  // namespace rslrl
