// Backward of a square 128-wide hidden layer (Linear(128, 128) + ELU of rsl_rl/networks/mlp.py:106-114, reached from
// ppo.py:367's loss.backward(): the [128, 128, 128] and [256, 128, 128] flat-terrain stacks) in ONE pass over the
// mini-batch rows, on the x6 split-bf16 MFMA path:
//   input gradient   dZp = (dZ W) * ELU'(H)            (rslrl_linear_gemm RSLRL_LINEAR_DGRAD_ELU: the same bits)
//   weight gradient  dW  = dZ^T H,  bias gradient db = sum_m dZ[m]   (rslrl_linear_wgrad_bias, bias_side 1)
// with dZ [M, 128] the gradient at this layer's pre-activation and H [M, 128] this layer's input.  The separate kernels
// move 2,560 B per row (dZ and H read twice); here every 64-row tile of dZ and H is read from HBM once (1,536 B per row
// with the dZp store) and feeds both GEMMs.  The 256-wide kernel (mlp_bwd_fused.hip) is not this one with another
// constant: its 4-wave form exists because 256 x 256 of dW needs the whole 512-register file of one wave per SIMD.
// Here the slice's dW is 64 KiB, so the geometry is chosen for the memory system instead:
//
// Workgroup = 4 waves (one per SIMD), 80 KiB of LDS, at most 256 registers per lane -> TWO workgroups per CU, two
// waves per SIMD that belong to different workgroups and are therefore never at the same barrier: one workgroup's
// epilogue, HBM waits and plane refresh run beside the other's MFMAs with no hand-placed interleaving.  (A 128-row
// tile with one workgroup per CU has the same 2 waves per SIMD but puts them behind the same two barriers per tile, and
// the 160 KiB it needs leaves nothing to overlap the refresh with.)  A workgroup runs a slice of consecutive 64-row
// tiles.  Wave w owns the output columns [32 w, 32 w + 32) of both GEMMs: dZp columns (2 MFMA blocks of 32 x 32 per
// tile) and dW columns k (4 blocks over n = 64 accumulator registers, held for the whole slice).  Per tile:
//  1. the dZ tile sits in LDS as three bf16 planes (48 KiB, split once);
//  2. input gradient: 8 k-chunks of 16 in ascending order, per chunk the two row blocks -- A fragments (dZ rows) by
//     ds_read_b128 from the planes, B fragments (rows [32 w, 32 w + 32) of the W^T image: only the live first 4 KiB of
//     each 8 KiB image plane is ever read) from global memory one chunk ahead; no LDS write and no barrier in the loop;
//  3. epilogue: H in the accumulator layout from the wave's own 8 KiB region of the 32 KiB H stage (the wave DMA'd
//     exactly those columns itself: it waits for its own loads only), ELU', dZp through the same region as 16-byte
//     nontemporal stores; the next tile's H is DMA'd into the region right after and lands during the weight gradient;
//  4. weight gradient: dW[n][k] += sum_m dZ[m][n] H[m][k] -- A = dZ^T from the resident planes by ds_read_b64_tr_b16,
//     B = H straight from the epilogue's registers.  The accumulator layout holds, per lane, column k at rows
//     (r & 3) + 8 (r >> 2) + 4 (lane >> 5), so each 16-deep MFMA step takes the tile's rows in the permuted order
//     pi(8 h + t) = 16 s + 4 h + (t & 3) + 8 (t >> 2); the transposed reads address exactly those rows, i.e. the same
//     sum.  H is never staged as planes: the wave split (output columns per wave in both GEMMs) is what allows it;
//  5. the next tile's dZ is loaded into registers before the weight gradient and split into the planes after a
//     barrier (two barriers per tile).
// db accumulates in fp32 from the staged dZ registers (thread t: columns 4 (t & 31) .. + 3 of rows = t >> 5 mod 8) and
// is folded over the eight row groups in order at the end.  Each slice writes one partial row [dW | db] of
// 128 * 128 + 128 floats; rslrl_fold_partials_batch folds the rows in fp64 in slice order.  No atomics: the summation
// order depends on M alone.
//
// The LDS images of the dZ planes and of the H stage, and why they are bank-conflict free: hidden_bwd_tile.h.
#include <algorithm>

#include "common.h"
#include "hidden_bwd_tile.h"

namespace rslrl {
namespace {

constexpr int kHnPartFloats = kHnW * kHnW + kHnW;  // a slice's partial row: [dW (128 x 128) | db (128)]
// Slices per problem.  Two workgroups fit a CU, so a pair of problems fills the 256 CUs of an MI355X with 2 x 256
// slices; and a slice runs at least two tiles, because its partial row costs 2 x 64.5 KiB (written here, read by the
// fold) against the 96 KiB a tile streams.  24,576 rows: 384 tiles -> 192 slices of 2 (384 workgroups for a pair);
// 393,216 rows: 6,144 tiles -> 256 slices of 24.
constexpr int kHnMaxSlices = 256;
constexpr int kHnMinTilesPer = 2;

struct HnProblem {
    const float* dz;   // [M, 128]
    const float* h;    // [M, 128]
    const uint4* img;  // x6 image of W^T (layout 0, 8 chunks)
    float* dz_prev;    // [M, 128]
    float* part;       // [S][kHnPartFloats]
};

struct HnArgs {
    HnProblem p[2];
    int tiles;      // M / 64
    int tiles_per;  // tiles per slice
};

__global__ __launch_bounds__(kHnThreads, 2) void hidden_bwd_n_kernel(HnArgs args) {
    __shared__ __attribute__((aligned(16))) char lds[kHnLds];
    char* const dzl = lds;
    char* const stage = lds + kHnDzBytes;
    const HnProblem& P = args.p[blockIdx.y];
    const int s = blockIdx.x;
    const int t_begin = s * args.tiles_per;
    const int t_end = min(args.tiles, t_begin + args.tiles_per);

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int h = lane >> 5;
    const int l32 = lane & 31;
    const int g1 = (lane >> 4) & 1;  // transposed reads: which 16 of a block's 32 columns
    const int tq = (lane >> 2) & 3;  //   row within the 4-row group
    const int tp = lane & 3;         //   column quad

    // LDS lane addresses: la[c] = (row l32, columns 16 c + 8 h ..) for the input gradient's row fragments; lt[nb][hi] =
    // (row 4 h + tq + 8 hi, columns 32 nb + 16 g1 + 4 tp ..) for the weight gradient's transposed reads.  Row blocks
    // (+ 32 rows = 1 KiB), row steps (+ 16 rows = 512 B) and planes (+ 16 KiB) are added as constants.
    const int lbase = static_cast<int>(reinterpret_cast<uintptr_t>(dzl));
    int la[kHnChunks], lt[4][2];
#pragma unroll
    for (int c = 0; c < kHnChunks; ++c) la[c] = lbase + hn_dz_off(l32, 16 * c + 8 * h);
#pragma unroll
    for (int nb = 0; nb < 4; ++nb)
#pragma unroll
        for (int hi = 0; hi < 2; ++hi) lt[nb][hi] = lbase + hn_dz_off(4 * h + tq + 8 * hi, 32 * nb + 16 * g1 + 4 * tp);

    f32x16 dw[4];
#pragma unroll
    for (int nb = 0; nb < 4; ++nb) dw[nb] = f32x16{};
    float4 csum = make_float4(0.f, 0.f, 0.f, 0.f);

    // this wave's B fragments: image row 32 w + l32 (output column), half h, swizzled as the image stores it; the
    // chunk and plane offsets ride in soffset.  Rows < 128: the first 4 KiB of every 8 KiB plane.
    const int brow = 32 * wave + l32;
    const int boff = (brow * 2 + (h ^ ((brow >> 3) & 1))) * 16;
    const __amdgpu_buffer_rsrc_t rimg = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<uint4*>(P.img), 0, static_cast<uint32_t>(kHnChunks * kHnImgChunkU * 16), kHnRsrcFlags);
    auto bload = [&](int c, int q) {
        return __builtin_bit_cast(
            uint4, __builtin_amdgcn_raw_buffer_load_b128(rimg, boff, (c * kHnImgChunkU + q * kHnImgPlaneU) * 16, 0));
    };

    // this wave's H region in the accumulator layout: row 32 i + 4 h + rr (rr = (r & 3) + 8 (r >> 2), bit 2 clear) sits
    // in slot 32 i + rr + 5 h (rr even) or 32 i + rr + 3 h (rr odd): two lane bases, the rest immediate offsets
    float* const reg = reinterpret_cast<float*>(stage + wave * kHnHRegion) + l32;
    float* const hs[2] = {reg + 5 * h * 32, reg + 3 * h * 32};

    // prologue: the first tile's H stage and dZ planes
    {
        const int64_t row0 = static_cast<int64_t>(t_begin) * kHnT;
        hn_dma_h(hn_tile_rsrc(P.h, row0), stage);
        float4 v[8];
        hn_load_dz(hn_tile_rsrc(P.dz, row0), v);
        hn_store_dz(v, dzl, csum);
    }
    __syncthreads();

    for (int t = t_begin; t < t_end; ++t) {
        const int64_t row0 = static_cast<int64_t>(t) * kHnT;
        const bool has_next = t + 1 < t_end;
        // ---- input gradient: dZ rows (LDS, resident) x W^T columns (global, one chunk ahead).  Block b = 2 c + i is
        // chunk c of row block i: per accumulator the chunks in ascending order, Arith<3>::mfma's six products each
        f32x16 acc[2] = {f32x16{}, f32x16{}};
        uint4 bq[2][3];  // ring of image chunks
#pragma unroll
        for (int q = 0; q < 3; ++q) bq[0][q] = bload(0, q);
        auto read_a = [&](int b, bf16x8 (&a)[3]) {
            const int c = b >> 1, ci = (b & 1) * 1024;
            a[0] = hn_read16(la[c] + ci);
            a[1] = hn_read16(la[c] + ci + kHnPlane);
            a[2] = hn_read16(la[c] + ci + 2 * kHnPlane);
        };
        bf16x8 af[2][3];
        read_a(0, af[0]);
#pragma unroll
        for (int b = 0; b < 2 * kHnChunks; ++b) {
            const int c = b >> 1;
            if ((b & 1) == 0 && c + 1 < kHnChunks) {
#pragma unroll
                for (int q = 0; q < 3; ++q) bq[(c + 1) & 1][q] = bload(c + 1, q);
            }
            if (b + 1 < 2 * kHnChunks) read_a(b + 1, af[(b + 1) & 1]);
            bf16x8 bf[3];
#pragma unroll
            for (int q = 0; q < 3; ++q) bf[q] = __builtin_bit_cast(bf16x8, bq[c & 1][q]);
            acc[b & 1] = Arith<3>::mfma(af[b & 1], bf, acc[b & 1]);
            __builtin_amdgcn_sched_barrier(0);  // one block's fragments ahead, no more
        }
        // ---- epilogue: H from this wave's stage region (its own DMA: no workgroup barrier), ELU', dZp out
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
        float hr[2][16];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) hr[i][r] = hs[r & 1][(32 * i + (r & 3) + 8 * (r >> 2)) * 32];
        // dZp = acc * ELU'(H) (epilogue_tiles_impl's expression) written over the H words, then read row-contiguous
        // and stored as 16-byte units
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float v = acc[i][r];
                const float hv = hr[i][r];
                const float g = v * (hv + 1.f);  // ELU'(z) = 1 if z > 0 else h + 1
                hs[r & 1][(32 * i + (r & 3) + 8 * (r >> 2)) * 32] = hv > 0.f ? v : g;
            }
        // the dword writes retire before the 16-byte reads (the LDS does not keep that order by itself)
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        {
            const __amdgpu_buffer_rsrc_t rc = __builtin_amdgcn_make_buffer_rsrc(
                P.dz_prev + row0 * kHnW + 32 * wave, 0, kHnTileBytes - 32 * wave * 4, kHnRsrcFlags);
            const float* rs = reinterpret_cast<const float*>(stage + wave * kHnHRegion) + hn_hslot(lane >> 3) * 32 +
                              4 * (lane & 7);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const u32x4 sv = *reinterpret_cast<const u32x4*>(rs + 8 * j * 32);  // row 8 j + lane / 8
                __builtin_amdgcn_raw_buffer_store_b128(sv, rc, ((lane >> 3) * kHnW + 4 * (lane & 7)) * 4,
                                                       8 * j * kHnW * 4, 2 /* nt */);
                // VMEM store-data hazard (mlp_bwd_fused.hip): the data registers stay live past wait states of the
                // asm's own, so no VALU write of them lands while the store still reads them
                asm volatile("s_nop 3" ::"v"(sv) : "memory");
            }
        }
        // the next tile's H into the (now read) region, and its dZ into registers: both land during the weight gradient
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        float4 vn[8];
        if (has_next) {
            hn_dma_h(hn_tile_rsrc(P.h, row0 + kHnT), stage);
            hn_load_dz(hn_tile_rsrc(P.dz, row0 + kHnT), vn);
        }
        // ---- weight gradient of the tile: dW[n][32 w + l32] += sum over rows of dZ[m][n] H[m][32 w + l32].  Block
        // k = 4 rs + nb: row step rs = 2 i + st (16 rows), dZ^T column block nb; the fragments of block k + 1 are read
        // beside block k's MFMAs
        auto read_t = [&](int k, bf16x8 (&a)[3]) {
            const int nb = k & 3, ci = 16 * (k >> 2) * 32;
            const int b0 = lt[nb][0] + ci, b1 = lt[nb][1] + ci;
            a[0] = hn_cat(hn_tr(b0), hn_tr(b1));
            a[1] = hn_cat(hn_tr(b0 + kHnPlane), hn_tr(b1 + kHnPlane));
            a[2] = hn_cat(hn_tr(b0 + 2 * kHnPlane), hn_tr(b1 + 2 * kHnPlane));
        };
        bf16x8 tf[2][3];
        bf16x8 hb[3];
        read_t(0, tf[0]);
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const int nb = k & 3, i = k >> 3, st = (k >> 2) & 1;
            if (nb == 0) {
                // B = H rows pi(8 h + t) of column 32 w + l32: accumulator entries r = 8 st + t of block i
                uint32_t p0[4], p1[4], p2[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    float x = hr[i][8 * st + 2 * j], y = hr[i][8 * st + 2 * j + 1];
                    p0[j] = split_pair(x, y);
                    p1[j] = split_pair(x, y);
                    p2[j] = pack_pair(x, y);
                }
                hb[0] = __builtin_bit_cast(bf16x8, make_uint4(p0[0], p0[1], p0[2], p0[3]));
                hb[1] = __builtin_bit_cast(bf16x8, make_uint4(p1[0], p1[1], p1[2], p1[3]));
                hb[2] = __builtin_bit_cast(bf16x8, make_uint4(p2[0], p2[1], p2[2], p2[3]));
            }
            if (k + 1 < 16) read_t(k + 1, tf[(k + 1) & 1]);
            dw[nb] = Arith<3>::mfma(tf[k & 1], hb, dw[nb]);
            __builtin_amdgcn_sched_barrier(0);
        }
        __syncthreads();  // every wave has read the dZ planes
        if (has_next) {
            hn_store_dz(vn, dzl, csum);
            __syncthreads();
        }
    }

    // ---- the slice's partial row: dW (lane: column 32 w + l32 of rows 32 nb + (r & 3) + 8 (r >> 2) + 4 h), then db
    float* out = P.part + static_cast<int64_t>(s) * kHnPartFloats;
#pragma unroll
    for (int nb = 0; nb < 4; ++nb)
#pragma unroll
        for (int r = 0; r < 16; ++r)
            out[(32 * nb + (r & 3) + 8 * (r >> 2) + 4 * h) * kHnW + 32 * wave + l32] = dw[nb][r];
    // the stage is free: every wave read its last H before the last barrier, and a slice's last tile starts no DMA
    float4* red = reinterpret_cast<float4*>(stage);
    red[threadIdx.x] = csum;
    __syncthreads();
    if (threadIdx.x < 32) {
        float4 a = red[threadIdx.x];
#pragma unroll
        for (int g = 1; g < 8; ++g) {
            const float4 b = red[32 * g + threadIdx.x];
            a.x += b.x;
            a.y += b.y;
            a.z += b.z;
            a.w += b.w;
        }
        reinterpret_cast<float4*>(out + kHnW * kHnW)[threadIdx.x] = a;
    }
}

int64_t hn_tiles_per(int64_t tiles) {
    return std::max<int64_t>(kHnMinTilesPer, ceil_div(tiles, kHnMaxSlices));
}

bool hn_rows_ok(int64_t M) { return M >= kHnT && M % kHnT == 0 && M / kHnT <= INT32_MAX; }

}  // namespace
}  // namespace rslrl

using namespace rslrl;

extern "C" int64_t rslrl_hidden_bwd_slices_n(int64_t M, int32_t width) {
    if (width != kHnW || !hn_rows_ok(M)) return 0;
    const int64_t tiles = M / kHnT;
    return ceil_div(tiles, hn_tiles_per(tiles));
}

extern "C" size_t rslrl_hidden_bwd_partial_floats_n(int32_t width) { return width == kHnW ? kHnPartFloats : 0; }

extern "C" int rslrl_hidden_bwd_pair_n(const rslrl_hidden_bwd_problem_t* p0, const rslrl_hidden_bwd_problem_t* p1,
                                       int64_t M, int32_t width, rslrl_stream_t stream) {
    if (!p0 || width != kHnW) return RSLRL_E_INVALID_ARGUMENT;
    if (!hn_rows_ok(M)) return M == 0 ? RSLRL_OK : RSLRL_E_UNSUPPORTED;
    const rslrl_hidden_bwd_problem_t* a[2] = {p0, p1};
    const int n = p1 ? 2 : 1;
    HnArgs args{};
    for (int i = 0; i < n; ++i) {
        const rslrl_hidden_bwd_problem_t* q = a[i];
        if (!q->dz || !q->h || !q->bimage || !q->dz_prev || !q->partials) return RSLRL_E_INVALID_ARGUMENT;
        const uintptr_t bits = reinterpret_cast<uintptr_t>(q->dz) | reinterpret_cast<uintptr_t>(q->h) |
                               reinterpret_cast<uintptr_t>(q->bimage) | reinterpret_cast<uintptr_t>(q->dz_prev) |
                               reinterpret_cast<uintptr_t>(q->partials);
        if (bits & 15) return RSLRL_E_MISALIGNED;
        args.p[i] = HnProblem{q->dz, q->h, static_cast<const uint4*>(q->bimage), q->dz_prev, q->partials};
    }
    const int64_t tiles = M / kHnT;
    const int64_t per = hn_tiles_per(tiles);
    args.tiles = static_cast<int>(tiles);
    args.tiles_per = static_cast<int>(per);
    const dim3 grid(static_cast<unsigned>(ceil_div(tiles, per)), static_cast<unsigned>(n));
    hipLaunchKernelGGL(hidden_bwd_n_kernel, grid, dim3(kHnThreads), 0, reinterpret_cast<hipStream_t>(stream), args);
    return launch_status();
}
