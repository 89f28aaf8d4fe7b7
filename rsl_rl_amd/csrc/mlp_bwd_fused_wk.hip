// Backward of a 512 -> 256 hidden layer (Linear(512, 256) + ELU of rsl_rl/networks/mlp.py:106-114, reached from
// ppo.py:367's loss.backward(): the second layer of [512, 256, 128], the default actor and critic of Legged-Gym and
// Isaac Lab rough terrain, which holds about 70 % of that stack's MACs) in ONE pass over the mini-batch rows, on the x6
// split-bf16 MFMA path:
//   input gradient   dZp = (dZ W) * ELU'(H)   [M, 512]   (rslrl_linear_gemm_wide RSLRL_LINEAR_DGRAD_ELU: the same bits)
//   weight gradient  dW  = dZ^T H  [256, 512],  bias gradient db = sum_m dZ[m]  (rslrl_linear_wgrad_bias_wide, side 1)
// with dZ [M, 256] the gradient at this layer's pre-activation, H [M, 512] this layer's input and W [256, 512].  The two
// separate launches move 10 KiB per row (dZ and H read once per launch, dZp written); this pass moves 6 KiB (H once,
// dZ once per block, dZp written).
//
// Both GEMMs have their 512 output columns on the H side (dZp[m][k] and dW[n][k] for all 256 n), and a slice's dW is
// 256 x 512 fp32 = 512 KiB, the whole register file of a CU: no single workgroup can hold it, so the columns are split
// into two blocks of 256.  Block q of a slice is one workgroup of the 4-wave form of mlp_bwd_fused.hip -- one wave per
// SIMD, 512 registers per lane, the block's 256 x 256 dW in 256 accumulator registers for the whole slice, the dZ tile
// resident as three bf16 planes (96 KiB, that file's swizzled layout), a 64 KiB H stage in per-wave regions, dZ^T read
// by ds_read_b64_tr_b16 from the planes, H taken from the epilogue's registers, the B fragments of the input gradient
// read from global memory ahead of their MFMAs, one workgroup per CU -- and everything that is not an MFMA is woven
// between the weight gradient's MFMAs exactly as there (the table above hidden_bwd4_kernel).  What differs:
//  - H and dZp are addressed at a row stride of 512 floats with the block's column offset 256 q (128 KiB tiles); the
//    buffer resources cover the tile's rows at that stride, so block 1's last access ends at the tile's end;
//  - the B fragments come from the q-th of the two consecutive 256-row layout-0 block images of W^T that the tape
//    already holds for the wide input-gradient GEMM (bimage_wide(W, True)): no image of its own;
//  - each block stages the dZ tile itself (dZ is read twice: 6 KiB per row instead of 5);
//  - the blocks of a slice are the workgroups x and x + 8 of the grid, so that under round-robin dispatch over the 8
//    XCDs they share an L2 and the second read of the dZ tile tends to hit there.  Locality only: each workgroup is
//    complete in itself and nothing orders the two;
//  - each block writes its 256 columns of the slice's 256 rows of dW at row stride 512; block 0 also writes db.
// The input gradient takes the 16 k-chunks of 16 in ascending order with Arith<3>::mfma per chunk and the ELU'
// expression of epilogue_tiles_impl, which is what makes dZp the wide GEMM's bits on the dense block.  Each slice
// writes one partial row [dW | db] of 256 * 512 + 256 floats; rslrl_fold_partials* folds the rows in fp64 in slice
// order.  No atomics: the summation order depends on M alone.
//
// The tile helpers below are this unit's own copies of mlp_bwd_fused.hip's (hb_* there, wk_* here, with the row
// stride and the column offset added): that file is left untouched, so every kernel it builds keeps its instructions.
#include <algorithm>
#include <utility>

#include "common.h"
#include "x6_split.h"

namespace rslrl {
namespace {

constexpr int kWkT = 64;                           // rows per tile
constexpr int kWkN = 256;                          // columns of dZ (the reduction of the input gradient)
constexpr int kWkK = 512;                          // the layer's input width: columns of H, dZp and dW
constexpr int kWkBlock = 256;                      // columns per workgroup
constexpr int kWkThreads = 256;                    // 4 waves: one per SIMD
constexpr int kWkPlane = kWkT * kWkN * 2;          // one bf16 plane of the dZ tile: 32 KiB
constexpr int kWkDzBytes = 3 * kWkPlane;           // 96 KiB
constexpr int kWkHRegion = kWkT * 32 * 4;          // 32 columns of H: 8 KiB (a wave owns two regions)
constexpr int kWkHBytes = 8 * kWkHRegion;          // the H stage: 64 KiB
constexpr int kWkLds = kWkDzBytes + kWkHBytes;     // 160 KiB: the whole LDS of a CU
constexpr int kWkChunks = kWkN / 16;               // k-chunks of the input gradient
constexpr int kWkChunkB = kWkT * 32;               // one chunk of one plane: 2 KiB
constexpr int kWkImgPlaneU = 256 * 32 / 16;        // 16-byte units of one plane of one image chunk (bimage layout 0)
constexpr int kWkImgChunkU = 3 * kWkImgPlaneU;
constexpr int kWkImgBlockU = kWkChunks * kWkImgChunkU;  // one 256-row block image: 384 KiB
constexpr int kWkBDepth = 2;                       // image chunks in flight ahead of the input gradient's MFMAs
constexpr int kWkPartFloats = kWkN * kWkK + kWkN;  // a slice's partial row: [dW (256 x 512) | db (256)]
constexpr uint32_t kWkRsrcFlags = 0x00020000;
constexpr uint32_t kWkDzTileBytes = kWkT * kWkN * 4;  // 64 KiB: one tile of dZ
constexpr uint32_t kWkHTileBytes = kWkT * kWkK * 4;   // 128 KiB: one tile of H or dZp
// Slices per problem.  A slice is two workgroups and a workgroup takes a CU, so 128 slices of one problem fill the 256
// CUs of an MI355X with one workgroup each; and a slice runs at least two tiles, because its partial row costs
// 2 x 513 KiB (written here, read by the fold) against the 384 KiB a tile streams.  24,576 rows: 384 tiles -> 128
// slices of 3; 393,216 rows: 6,144 tiles -> 128 slices of 48.
constexpr int kWkMaxSlices = 128;
constexpr int kWkMinTilesPer = 2;
constexpr int kWkXcds = 8;

using s16x4 = __attribute__((ext_vector_type(4))) short;
using u32x4 = __attribute__((ext_vector_type(4))) unsigned int;

struct WkProblem {
    const float* dz;   // [M, 256]
    const float* h;    // [M, 512]
    const uint4* img;  // two consecutive x6 block images of W^T (layout 0, 16 chunks, 256 rows each)
    float* dz_prev;    // [M, 512]
    float* part;       // [S][kWkPartFloats]
};

struct WkArgs {
    WkProblem p[2];
    int tiles;      // M / 64
    int tiles_per;  // tiles per slice
};

// LDS image of a dZ plane: [16 chunks of 16 columns][64 row slots][32 bytes], row m of chunk c in slot m ^ f(c),
// f(c) = (c & 3) | 4 (c & 1), its two 16-byte halves swapped when (m >> 3) & 1: bank-conflict free for the row
// fragments, the transposed reads and the staging stores (mlp_bwd_fused.hip's header has the argument)
__host__ __device__ constexpr int wk_f(int c) { return (c & 3) | ((c & 1) << 2); }

// byte offset of (row m, column col % 4 == 0) in a plane
__device__ __forceinline__ int wk_dz_off(int m, int col) {
    const int c = col >> 4;
    return c * kWkChunkB + (m ^ wk_f(c)) * 32 + 16 * (((col >> 3) & 1) ^ ((m >> 3) & 1)) + 8 * ((col >> 2) & 1);
}

// buffer resources over the tile's rows of dZ [M, 256] and of H [M, 512]: wave-uniform base, every offset in the
// instructions' voffset / soffset fields; a load past the tile returns 0
__device__ __forceinline__ __amdgpu_buffer_rsrc_t wk_dz_rsrc(const float* base, int64_t row0) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(base + row0 * kWkN), 0, kWkDzTileBytes, kWkRsrcFlags);
}
__device__ __forceinline__ __amdgpu_buffer_rsrc_t wk_h_rsrc(const float* base, int64_t row0) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(base + row0 * kWkK), 0, kWkHTileBytes, kWkRsrcFlags);
}

__device__ __forceinline__ int wk_hslot(int r) { return r ^ ((r >> 2) & 1); }

__device__ __forceinline__ s16x4 wk_tr(int addr) {  // one 4-row transposed read (ds_read_b64_tr_b16)
    typedef __attribute__((address_space(3))) s16x4 lds_s16x4;
    return __builtin_amdgcn_ds_read_tr16_b64_v4i16(reinterpret_cast<lds_s16x4*>(addr));
}

__device__ __forceinline__ bf16x8 wk_cat(s16x4 lo, s16x4 hi) {
    const __attribute__((ext_vector_type(8))) short v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    return __builtin_bit_cast(bf16x8, v);
}

__device__ __forceinline__ bf16x8 wk_read16(int addr) {
    typedef __attribute__((address_space(3))) uint4 lds_u4;
    return __builtin_bit_cast(bf16x8, *reinterpret_cast<const lds_u4*>(addr));
}

// f(integral_constant<int, 0>) ... f(integral_constant<int, N - 1>): a loop whose index is a constant in its body
template <class F, int... I>
__device__ __forceinline__ void wk_static_for_impl(F&& f, std::integer_sequence<int, I...>) {
    (f(std::integral_constant<int, I>{}), ...);
}
template <int N, class F>
__device__ __forceinline__ void wk_static_for(F&& f) {
    wk_static_for_impl(f, std::make_integer_sequence<int, N>{});
}

// split_pair / split4 of x6_split.h with the residuals kept scalar: left alone, the optimizer packs each pair's two
// subtractions into one v_pk_add_f32, which costs a lone wave more issue time beside MFMAs than the two v_sub_f32
__device__ __forceinline__ uint32_t wk_split_pair(float& x, float& y) {
    const uint32_t pk = split_pair(x, y);
    asm("" : "+v"(x));
    asm("" : "+v"(y));
    return pk;
}
__device__ __forceinline__ void wk_split4(float4 v, uint2& p0, uint2& p1, uint2& p2) {
    p0.x = wk_split_pair(v.x, v.y);
    p0.y = wk_split_pair(v.z, v.w);
    p1.x = wk_split_pair(v.x, v.y);
    p1.y = wk_split_pair(v.z, v.w);
    p2.x = pack_pair(v.x, v.y);
    p2.y = pack_pair(v.z, v.w);
}

// N MFMA gaps, each offered one LDS read, one global load and a few vector instructions of the same block
template <int N>
__device__ __forceinline__ void wk_weave() {
#pragma unroll
    for (int n = 0; n < N; ++n) {
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);  // MFMA
        __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);  // DS read
        __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);  // VMEM read
        __builtin_amdgcn_sched_group_barrier(0x002, 4, 0);  // VALU
        __builtin_amdgcn_sched_group_barrier(0x200, 2, 0);  // DS write
    }
}

// the tile's dZ, 16 float4 per thread: row (t >> 6) + 4 i, columns 4 (t & 63) .. + 3; nontemporal (the second block's
// read is meant to hit L2, the W^T image should stay there)
__device__ __forceinline__ void wk_load_dz(__amdgpu_buffer_rsrc_t r, float4 (&v)[16], int i0, int i1) {
    const int off = ((threadIdx.x >> 6) * kWkN + 4 * (threadIdx.x & 63)) * 4;
#pragma unroll
    for (int i = i0; i < i1; ++i)
        v[i] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(r, off, i * 4 * kWkN * 4, 2));
}

__device__ __forceinline__ void wk_store_planes(const uint2 (&sp)[16][3], char* __restrict__ lds) {
    const int col = 4 * (threadIdx.x & 63);
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int off = wk_dz_off(static_cast<int>(threadIdx.x >> 6) + 4 * i, col);
#pragma unroll
        for (int q = 0; q < 3; ++q) *reinterpret_cast<uint2*>(lds + q * kWkPlane + off) = sp[i][q];
    }
}

// H stage: wave w owns the regions 2 w and 2 w + 1, [64 row slots][32 columns] of its columns [col0 + 64 w + 32 j,
// + 32), row r in slot r ^ ((r >> 2) & 1).  Instructions i0 .. i1 - 1 of region j: instruction i fills slots 8 i ..
// 8 i + 7 (lane l: slot 8 i + l / 8, 16 bytes of column quad l % 8); the largest byte read is row 63, columns
// col0 + 64 w + 32 j + 28 .. 31 <= 511: inside the tile.  Issued as asm statements: the compiler orders every later
// LDS read behind a DMA it knows of with vmcnt(0) -- a full HBM round trip in the middle of the weight gradient --
// while nothing here reads the region before the wave's own vmcnt(0) beside the next input gradient's last blocks.
// M0 (the LDS destination) is set and restored in the statement.
__device__ __forceinline__ void wk_dma_h(__amdgpu_buffer_rsrc_t r, char* stage, int col0, int j, int i0, int i1) {
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    const int off = (wk_hslot(lane >> 3) * kWkK + col0 + 64 * wave + 4 * (lane & 7)) * 4;
#pragma unroll
    for (int i = i0; i < i1; ++i) {
        const uint32_t dst = static_cast<uint32_t>(reinterpret_cast<uintptr_t>(stage)) +
                             (2 * wave + j) * kWkHRegion + i * 1024;
        const int soff = i * 8 * kWkK * 4 + j * 128;
        uint32_t keep;
        asm volatile(
            "s_mov_b32 %0, m0\n\ts_mov_b32 m0, %1\n\ts_nop 0\n\tbuffer_load_dwordx4 %2, %3, %4 offen nt lds\n\t"
            "s_mov_b32 m0, %0"
            : "=&s"(keep)
            : "s"(dst), "v"(off), "s"(r), "s"(soff)
            : "memory");
    }
}

// Wave w of block q owns the columns [256 q + 64 w, + 64) of H, dZp and dW as two column blocks j of 32: 4 MFMA blocks
// of dZp per tile and 16 blocks of dW (256 accumulator registers).  Beside the MFMAs of the weight gradient (a block =
// one dZ^T fragment x the wave's two column blocks = 12 MFMAs):
//   block  0 ..  7   the epilogue's first halves: ELU', dZp over the H words of the stage (8 accumulator rows per block)
//   block  1 .. 17   its second halves: one 16-byte unit per lane read back per block and stored in the next
//   block  9 .. 24   the next tile's H DMA into the two regions as they are read out, one instruction per block
//   block  8 .. 23   the next tile's dZ into registers (the input gradient's accumulators are dead by then)
//   block 16 .. 31   its split into the three bf16 planes, one float4 per block (written to LDS after the barrier)
//   every block      one pair of the next row step's H planes; the next block's dZ^T fragments
__global__ __launch_bounds__(kWkThreads, 1) void hidden_bwd_wk_kernel(WkArgs args) {
    __shared__ __attribute__((aligned(16))) char lds[kWkLds];
    char* const dzl = lds;
    char* const stage = lds + kWkDzBytes;
    const WkProblem& P = args.p[blockIdx.y];
    // workgroups 16 g .. 16 g + 15 are the slices 8 g .. 8 g + 7, block 0 then block 1 (gridDim.x is a multiple of 16, so
    // the second problem's ids keep the residues); the last group may hold slices past the end
    const int s = (blockIdx.x >> 4) * kWkXcds + (blockIdx.x & (kWkXcds - 1));
    const int col0 = ((blockIdx.x >> 3) & 1) * kWkBlock;
    const int t_begin = s * args.tiles_per;
    // A slice past the end: the workgroup ends here, before anything is loaded.  Written as the instruction and not as
    // `return`: with the early exit in the control-flow graph the register allocator spilled one 16-register
    // accumulator block per tile (68 bytes of scratch); like this the kernel has none, as mlp_bwd_fused.hip's.  The
    // condition is uniform over the workgroup and nothing is in flight.
    if (t_begin >= args.tiles) asm volatile("s_endpgm" ::: "memory");
    const int t_end = min(args.tiles, t_begin + args.tiles_per);

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int h = lane >> 5;
    const int l32 = lane & 31;
    const int g1 = (lane >> 4) & 1;       // transposed reads: which 16 of a block's 32 columns
    const int tq = (lane >> 2) & 3;       //   row within the 4-row group
    const int tp = lane & 3;              //   column quad
    const int wcol = col0 + 64 * wave;    // this wave's first column of H, dZp and dW

    // LDS lane address parts (the planes' layout and the fragments are mlp_bwd_fused.hip's): la[c & 3] =
    // wk_dz_off(l32, 16 c + 8 h) - c * 2 KiB for the input gradient's row fragments; lt[nb & 1][hi] =
    // wk_dz_off(4 h + tq + 8 hi, 32 nb + 16 g1 + 4 tp) - 2 (nb >> 1) * 4 KiB for the weight gradient's transposed
    // reads; la2 / lt2: the same + two planes (the immediate offset field holds 16 bits)
    const int lbase = static_cast<int>(reinterpret_cast<uintptr_t>(dzl));
    int la[4], la2[4], lt[2][2], lt2[2][2];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        la[c] = lbase + wk_dz_off(l32, 16 * c + 8 * h) - c * kWkChunkB;
        la2[c] = la[c] + 2 * kWkPlane;
    }
#pragma unroll
    for (int nb = 0; nb < 2; ++nb)
#pragma unroll
        for (int hi = 0; hi < 2; ++hi) {
            lt[nb][hi] = lbase + wk_dz_off(4 * h + tq + 8 * hi, 32 * nb + 16 * g1 + 4 * tp);
            lt2[nb][hi] = lt[nb][hi] + 2 * kWkPlane;
        }

    f32x16 dw[2][8];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int nb = 0; nb < 8; ++nb) dw[j][nb] = f32x16{};
    // column sums of the rows = wave and = wave + 4 (mod 8), folded at the end in the order of eight row classes
    float4 csum[2] = {make_float4(0.f, 0.f, 0.f, 0.f), make_float4(0.f, 0.f, 0.f, 0.f)};

    // B fragments: row 64 w + 32 j + l32 of this block's image (the q-th block image holds the output columns
    // [256 q, 256 q + 256)); j's 1 KiB, the chunk and the plane ride in soffset.  The resource covers that image alone.
    const int brow = 64 * wave + l32;
    const int boff = (brow * 2 + (h ^ ((brow >> 3) & 1))) * 16;
    const __amdgpu_buffer_rsrc_t rimg = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<uint4*>(P.img + (col0 / kWkBlock) * kWkImgBlockU), 0, static_cast<uint32_t>(kWkImgBlockU * 16),
        kWkRsrcFlags);
    auto bload = [&](int c, int j, int q) {
        return __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(
                                             rimg, boff, (c * kWkImgChunkU + q * kWkImgPlaneU) * 16 + j * 1024, 0));
    };

    // this wave's two H regions in the accumulator layout: row 32 i + 4 h + rr (rr = (r & 3) + 8 (r >> 2)) sits in slot
    // 32 i + rr + 5 h (rr even) or 32 i + rr + 3 h (rr odd): two lane bases per region, the rest immediate offsets
    float* const reg = reinterpret_cast<float*>(stage + 2 * wave * kWkHRegion) + l32;
    float* const hs[2][2] = {{reg + 5 * h * 32, reg + 3 * h * 32},
                             {reg + kWkHRegion / 4 + 5 * h * 32, reg + kWkHRegion / 4 + 3 * h * 32}};

    // prologue: the first tile's H stage and dZ planes
    {
        const int64_t row0 = static_cast<int64_t>(t_begin) * kWkT;
        wk_dma_h(wk_h_rsrc(P.h, row0), stage, col0, 0, 0, 8);
        wk_dma_h(wk_h_rsrc(P.h, row0), stage, col0, 1, 0, 8);
        float4 v[16];
        wk_load_dz(wk_dz_rsrc(P.dz, row0), v, 0, 16);
        uint2 sp[16][3];
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            csum[i & 1].x += v[i].x;
            csum[i & 1].y += v[i].y;
            csum[i & 1].z += v[i].z;
            csum[i & 1].w += v[i].w;
            split4(v[i], sp[i][0], sp[i][1], sp[i][2]);
        }
        wk_store_planes(sp, dzl);
    }
    __syncthreads();

    for (int t = t_begin; t < t_end; ++t) {
        const int64_t row0 = static_cast<int64_t>(t) * kWkT;
        const bool has_next = t + 1 < t_end;
        // the loads for the next tile are issued unconditionally (a slice's last tile re-reads itself and drops the
        // result): no branch splits the weight gradient's blocks
        const int64_t rown = has_next ? row0 + kWkT : row0;
        // ---- input gradient: block b = 2 c + i is chunk c of row block i, both column blocks j; image chunks
        // kWkBDepth ahead, the A fragments of block b + 1 read beside block b's MFMAs.  Per accumulator the 16 chunks in
        // ascending order, Arith<3>::mfma's six products each
        f32x16 acc[2][2] = {{f32x16{}, f32x16{}}, {f32x16{}, f32x16{}}};
        uint4 bq[kWkBDepth + 1][2][3];
#pragma unroll
        for (int c = 0; c < kWkBDepth; ++c)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int q = 0; q < 3; ++q) bq[c][j][q] = bload(c, j, q);
        auto read_a = [&](int b, bf16x8 (&a)[3]) {
            const int c = b >> 1, ci = c * kWkChunkB + (b & 1) * 1024;
            a[0] = wk_read16(la[c & 3] + ci);
            a[1] = wk_read16(la[c & 3] + ci + kWkPlane);
            a[2] = wk_read16(la2[c & 3] + ci);
        };
        // H of the tile in the accumulator layout and the planes of the weight gradient's row steps ([row step
        // parity][j][plane][pair]): read and split beside the input gradient's last four blocks, when the image ring
        // has drained (the H DMA is this wave's own: its vmcnt(0) waits for nobody else)
        float hr[2][2][16];
        uint32_t hbw[2][2][3][4];
        auto split_h = [&](int rs, int j, int p) {
            // B = H rows pi(8 h + t) of column wcol + 32 j + l32: accumulator entries r = 8 st + t of block i
            float x = hr[j][rs >> 1][8 * (rs & 1) + 2 * p], y = hr[j][rs >> 1][8 * (rs & 1) + 2 * p + 1];
            hbw[rs & 1][j][0][p] = wk_split_pair(x, y);
            hbw[rs & 1][j][1][p] = wk_split_pair(x, y);
            hbw[rs & 1][j][2][p] = pack_pair(x, y);
        };
        bf16x8 af[2][3];
        read_a(0, af[0]);
        wk_static_for<2 * kWkChunks>([&](auto bc) {
            constexpr int b = decltype(bc)::value;
            constexpr int c = b >> 1;
            if constexpr (b >= 28) {
                if constexpr (b == 28) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                const int j = (b - 28) >> 1, i = (b - 28) & 1;
#pragma unroll
                for (int r = 0; r < 16; ++r) hr[j][i][r] = hs[j][r & 1][(32 * i + (r & 3) + 8 * (r >> 2)) * 32];
                if constexpr (b == 29 || b == 31) {
#pragma unroll
                    for (int p = 0; p < 4; ++p) split_h(0, j, p);
                }
            }
            if constexpr ((b & 1) == 0 && c + kWkBDepth < kWkChunks) {
#pragma unroll
                for (int j = 0; j < 2; ++j)
#pragma unroll
                    for (int q = 0; q < 3; ++q) bq[(c + kWkBDepth) % (kWkBDepth + 1)][j][q] = bload(c + kWkBDepth, j, q);
            }
            if constexpr (b + 1 < 2 * kWkChunks) read_a(b + 1, af[(b + 1) & 1]);
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                bf16x8 bf[3];
#pragma unroll
                for (int q = 0; q < 3; ++q) bf[q] = __builtin_bit_cast(bf16x8, bq[c % (kWkBDepth + 1)][j][q]);
                acc[j][b & 1] = Arith<3>::mfma(af[b & 1], bf, acc[j][b & 1]);
            }
            wk_weave<12>();
            __builtin_amdgcn_sched_barrier(0);
        });
        __builtin_amdgcn_sched_barrier(0);
        auto read_t = [&](int k, bf16x8 (&a)[3]) {
            // rows 16 rs + 4 h + tq (lo) and + 8 (hi), columns 32 nb + 16 g1 + 4 tp of dZ
            const int nb = k & 7, rs = k >> 3;
            const int ci = 2 * (nb >> 1) * 2 * kWkChunkB + 16 * rs * 32;
            const int b0 = lt[nb & 1][0] + ci, b1 = lt[nb & 1][1] + ci;
            const int c0 = lt2[nb & 1][0] + ci, c1 = lt2[nb & 1][1] + ci;
            a[0] = wk_cat(wk_tr(b0), wk_tr(b1));
            a[1] = wk_cat(wk_tr(b0 + kWkPlane), wk_tr(b1 + kWkPlane));
            a[2] = wk_cat(wk_tr(c0), wk_tr(c1));
        };
        // epilogue piece (j, i), first half: dZp = acc * ELU'(H) (epilogue_tiles_impl's bits) over the H words
        auto epi_a = [&](int j, int i, int r0, int r1) {
#pragma unroll
            for (int r = r0; r < r1; ++r) {
                const float v = acc[j][i][r];
                const float hv = hr[j][i][r];
                const float g = v * (hv + 1.f);  // ELU'(z) = 1 if z > 0 else h + 1
                hs[j][r & 1][(32 * i + (r & 3) + 8 * (r >> 2)) * 32] = hv > 0.f ? v : g;
            }
        };
        // second half: read back row-contiguous, stored as 16-byte units.  The resource starts at this wave's first
        // column of the tile's first row and ends at the tile's end: the last store (row 63, columns wcol + 60 .. 63)
        // ends at or before it
        const __amdgpu_buffer_rsrc_t rc = __builtin_amdgcn_make_buffer_rsrc(
            P.dz_prev + row0 * kWkK + wcol, 0, kWkHTileBytes - static_cast<uint32_t>(wcol) * 4, kWkRsrcFlags);
        // one 16-byte unit per lane at a time (unit u = 4 (2 j + i) + q: rows 32 i + 8 q + lane / 8 of region j): read
        // back in one block, stored in the next.  One store per block: the CU takes a tile's stores at some 14 bytes
        // per cycle, and a lone wave that issues them faster waits for it
        u32x4 svq;
        auto epi_read = [&](int u) {
            const int j = u >> 3, jj = (u >> 2 & 1) * 4 + (u & 3);
            // the dword writes retire before the 16-byte reads (the LDS does not keep that order by itself)
            if ((u & 3) == 0) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            const float* rs = reinterpret_cast<const float*>(stage + (2 * wave + j) * kWkHRegion) +
                              wk_hslot(lane >> 3) * 32 + 4 * (lane & 7);
            svq = *reinterpret_cast<const u32x4*>(rs + 8 * jj * 32);
        };
        auto epi_store = [&](int u) {
            const int j = u >> 3, jj = (u >> 2 & 1) * 4 + (u & 3);
            __builtin_amdgcn_raw_buffer_store_b128(svq, rc, ((lane >> 3) * kWkK + 4 * (lane & 7)) * 4,
                                                   8 * jj * kWkK * 4 + j * 128, 2 /* nt */);
            // VMEM store-data hazard (mlp_bwd_fused.hip): the data registers stay live past the asm's own wait states,
            // so no VALU write of them lands while the store still reads them
            asm volatile("s_nop 3" ::"v"(svq) : "memory");
        };
        const __amdgpu_buffer_rsrc_t rhn = wk_h_rsrc(P.h, rown);
        const __amdgpu_buffer_rsrc_t rdn = wk_dz_rsrc(P.dz, rown);
        float4 vn[16];
        float4 cs2[2] = {csum[0], csum[1]};  // the sums with the next tile: kept only if there is one
        uint2 sp[16][3];
        bf16x8 tf[2][3];
        read_t(0, tf[0]);
        // ---- weight gradient: block k = 8 rs + nb, row step rs = 2 i + st, dZ^T column block nb, both j:
        // dW[32 nb ..][wcol + 32 j + l32] += sum over the step's 16 rows of dZ[m][n] H[m][wcol + 32 j + l32]
        wk_static_for<32>([&](auto kc) {
            constexpr int k = decltype(kc)::value;
            constexpr int nb = k & 7, rs = k >> 3;
            // the next block's dZ^T fragments first: LDS reads ahead of this block's LDS writes, which then spread
            // over the MFMA gaps instead of queueing in front of the reads
            if constexpr (k + 1 < 32) read_t(k + 1, tf[(k + 1) & 1]);
            if constexpr (k < 8) epi_a(k >> 2, (k >> 1) & 1, 8 * (k & 1), 8 * (k & 1) + 8);
            if constexpr (k >= 2 && k < 18) epi_store(k - 2);
            if constexpr (k >= 1 && k < 17) epi_read(k - 1);
            if constexpr (k == 9 || k == 17) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            if constexpr (k >= 9 && k < 17) wk_dma_h(rhn, stage, col0, 0, k - 9, k - 8);
            if constexpr (k >= 17 && k < 25) wk_dma_h(rhn, stage, col0, 1, k - 17, k - 16);
            if constexpr (k >= 8 && k < 24) wk_load_dz(rdn, vn, k - 8, k - 7);
            if constexpr (k >= 16) {
                const int i = k - 16;
                cs2[i & 1].x += vn[i].x;
                cs2[i & 1].y += vn[i].y;
                cs2[i & 1].z += vn[i].z;
                cs2[i & 1].w += vn[i].w;
                wk_split4(vn[i], sp[i][0], sp[i][1], sp[i][2]);
                // used only under has_next after the loop: pinned here, beside this block's MFMAs, or the optimizer
                // sinks the whole split behind the barrier
#pragma unroll
                for (int q = 0; q < 3; ++q) asm volatile("" : "+v"(sp[i][q].x), "+v"(sp[i][q].y));
                asm volatile("" : "+v"(cs2[i & 1].x), "+v"(cs2[i & 1].y), "+v"(cs2[i & 1].z), "+v"(cs2[i & 1].w));
            }
            if constexpr (rs < 3) split_h(rs + 1, nb >> 2, nb & 3);
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                bf16x8 hb[3];
#pragma unroll
                for (int q = 0; q < 3; ++q)
                    hb[q] = __builtin_bit_cast(bf16x8, make_uint4(hbw[rs & 1][j][q][0], hbw[rs & 1][j][q][1],
                                                                  hbw[rs & 1][j][q][2], hbw[rs & 1][j][q][3]));
                dw[j][nb] = Arith<3>::mfma(tf[k & 1], hb, dw[j][nb]);
            }
            wk_weave<12>();
            __builtin_amdgcn_sched_barrier(0);
        });
        __syncthreads();  // every wave has read the dZ planes
        if (has_next) {
            csum[0] = cs2[0];
            csum[1] = cs2[1];
            wk_store_planes(sp, dzl);
            __syncthreads();
        }
    }

    // ---- the slice's partial row: this block's columns of dW (lane: column wcol + 32 j + l32 of rows 32 nb + (r & 3) +
    // 8 (r >> 2) + 4 h) at row stride 512, then db from block 0
    float* out = P.part + static_cast<int64_t>(s) * kWkPartFloats;
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int nb = 0; nb < 8; ++nb)
#pragma unroll
            for (int r = 0; r < 16; ++r)
                out[(32 * nb + (r & 3) + 8 * (r >> 2) + 4 * h) * kWkK + wcol + 32 * j + l32] = dw[j][nb][r];
    // the last tile's (dropped) H DMA has landed in this wave's regions before the workgroup gives up its LDS
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (col0 != 0) return;  // (the whole workgroup)
    __syncthreads();        // every wave's DMA has landed before the stage is reused
    float4* red = reinterpret_cast<float4*>(stage);
    red[threadIdx.x] = csum[0];
    red[kWkThreads + threadIdx.x] = csum[1];
    __syncthreads();
    if (threadIdx.x < 64) {
        float4 a = red[threadIdx.x];
#pragma unroll
        for (int g = 1; g < 8; ++g) {
            const float4 b = red[64 * g + threadIdx.x];
            a.x += b.x;
            a.y += b.y;
            a.z += b.z;
            a.w += b.w;
        }
        reinterpret_cast<float4*>(out + kWkN * kWkK)[threadIdx.x] = a;
    }
}

bool wk_shape_ok(int32_t K, int32_t N) { return K == kWkK && N == kWkN; }

// (the bound keeps the kernel's first-tile index of the slice after the last one inside an int)
bool wk_rows_ok(int64_t M) { return M >= kWkT && M % kWkT == 0 && M / kWkT <= INT32_MAX - 2 * kWkMaxSlices; }

int64_t wk_tiles_per(int64_t tiles) {
    return std::max<int64_t>(kWkMinTilesPer, ceil_div(tiles, static_cast<int64_t>(kWkMaxSlices)));
}

}  // namespace
}  // namespace rslrl

using namespace rslrl;

extern "C" int64_t rslrl_hidden_bwd_slices_wk(int64_t M, int32_t K, int32_t N) {
    if (!wk_shape_ok(K, N) || !wk_rows_ok(M)) return 0;
    const int64_t tiles = M / kWkT;
    return ceil_div(tiles, wk_tiles_per(tiles));
}

extern "C" size_t rslrl_hidden_bwd_partial_floats_wk(int32_t K, int32_t N) {
    return wk_shape_ok(K, N) ? kWkPartFloats : 0;
}

extern "C" int rslrl_hidden_bwd_pair_wk(const rslrl_hidden_bwd_problem_t* p0, const rslrl_hidden_bwd_problem_t* p1,
                                        int64_t M, int32_t K, int32_t N, rslrl_stream_t stream) {
    if (!p0 || !wk_shape_ok(K, N)) return RSLRL_E_INVALID_ARGUMENT;
    if (!wk_rows_ok(M)) return M == 0 ? RSLRL_OK : RSLRL_E_UNSUPPORTED;
    const rslrl_hidden_bwd_problem_t* a[2] = {p0, p1};
    const int n = p1 ? 2 : 1;
    WkArgs args{};
    for (int i = 0; i < n; ++i) {
        const rslrl_hidden_bwd_problem_t* q = a[i];
        if (!q->dz || !q->h || !q->bimage || !q->dz_prev || !q->partials) return RSLRL_E_INVALID_ARGUMENT;
        const uintptr_t bits = reinterpret_cast<uintptr_t>(q->dz) | reinterpret_cast<uintptr_t>(q->h) |
                               reinterpret_cast<uintptr_t>(q->bimage) | reinterpret_cast<uintptr_t>(q->dz_prev) |
                               reinterpret_cast<uintptr_t>(q->partials);
        if (bits & 15) return RSLRL_E_MISALIGNED;
        args.p[i] = WkProblem{q->dz, q->h, static_cast<const uint4*>(q->bimage), q->dz_prev, q->partials};
    }
    const int64_t tiles = M / kWkT;
    const int64_t per = wk_tiles_per(tiles);
    args.tiles = static_cast<int>(tiles);
    args.tiles_per = static_cast<int>(per);
    // 16 workgroups per 8 slices: the blocks of slice s at x and x + 8
    const int64_t groups = ceil_div(ceil_div(tiles, per), static_cast<int64_t>(kWkXcds));
    const dim3 grid(static_cast<unsigned>(2 * kWkXcds * groups), static_cast<unsigned>(n));
    hipLaunchKernelGGL(hidden_bwd_wk_kernel, grid, dim3(kWkThreads), 0, reinterpret_cast<hipStream_t>(stream), args);
    return launch_status();
}
