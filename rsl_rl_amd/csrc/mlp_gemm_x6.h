// Device templates of the tiled split-precision GEMM ("x6": three bf16 planes; "h3": two fp16 planes), shared by the
// units that instantiate kernels from them: mlp_gemm.hip (the hidden-layer ops and their pair forms; its f32 kernel
// shares the tile epilogue) and mlp_heads.hip (the fused last hidden + output layer: RSLRL_LINEAR_FWD_OUT, the value
// and actor heads).  Everything here is inlined into those kernels; each unit gets its own copy.
//
// ---- split-bf16 main loop ("x6"): fp32-accurate products on the bf16 MFMA (16x the f32 MFMA rate).
// Every fp32 operand is split into three bf16 planes (x6_split.h); per 16-deep k step and 32x32 tile six
// bf16 MFMAs accumulate a0b0 + a0b1 + a1b0 + a1b1 + a0b2 + a2b0 in fp32 -- the error of an fp32 GEMM
// (tests/test_gpu_fused_mlp.py measures both against fp64) at 2.67x fewer MFMA cycles than
// v_mfma_f32_32x32x2_f32.
//
// Tile: 128 rows x 256 columns per 512-thread workgroup (two per CU at <= 128 VGPRs), 8 waves as 2 (M) x 4 (N), each
// wave 64 x 64 = 2 x 2 MFMA tiles.  Operands: A (activations, fp32, read once from HBM) is fetched ahead into registers
// and split while it is stored into LDS; B (the weights, re-read by every workgroup from L2) is split once per call by
// bimage_kernel (mlp_image.hip) into an image that is byte-for-byte the kernel's LDS image (mlp_tile.h).
//
// LDS image per buffer: [A plane 0..2][B plane 0..2], each plane [rows][16 bf16] = 32 B per row, halves swizzled (swz).
#pragma once

#include <type_traits>

#include "common.h"
#include "amax.h"
#include "mlp_gemm.h"
#include "mlp_tile.h"
#include "ppo_loss_common.h"
#include "x6_split.h"
#ifdef RSLRL_GEMM_RAGGED
#include "ragged_load.h"
#endif

namespace rslrl {
namespace {

// The actor head with the PPO loss and its backward (mlp_gemm_x6_actor_head_kernel, rslrl_actor_head_fwd_bwd): the
// loss inputs of the mini-batch, the output layer's transposed image and the loss outputs.
constexpr int kActA = 12;                              // actions: 3 per lane of a row's quad
constexpr int kActCols = 4 + kActA;                    // loss partial columns: surrogate, value, entropy, KL, d sigma
constexpr int kActTileFloats = kActA * kBN + kActA;    // per-tile [dW (12 x 256) | db (12)] (a multiple of 4)
// The forms for any action count A = p.nout in [kActMinA, kActMaxA] but 12 (mlp_gemm_x6_actor_head_any_kernel<APL>,
// APL = ceil(A / 4) actions per lane of a row's quad): the LDS side area, the reduction tiles and the per-wave loss
// partials are laid out for kActMaxA whatever A is; the per-tile partial row is act_tile_floats(A) long.
constexpr int kActMinA = 5;                            // below: the NR = 1 output layer (other mu bits)
constexpr int kActMaxA = 16;                           // the d mu tile's width and one k step of the dZ MFMA
constexpr int kActMaxCols = 4 + kActMaxA;              // loss partial columns at kActMaxA
constexpr int kHeadActorAny = 8;                       // mlp_gemm_x6_body's HEAD = kHeadActorAny + APL
// rows of kActMaxA floats in the LDS side area, after the last hidden layer's bias: the prologue stages the first three
enum { kSideObias = 0, kSideSigma, kSideOldSigma, kSideLs, kSideInvDen, kSideInvS, kSideInvS3, kSideKlOs, kSideKlT1,
       kSideKlD, kSideKlRD, kSideEnt, kActSideRows };
// [dW (A x N) | db | 0 pad]: N = kBN but for the narrow heads
__host__ __device__ constexpr int act_tile_floats(int A, int N = kBN) { return A * N + ((A + 3) & ~3); }
struct ActorParams {
    const float* actions;    // [M, A] (A = p.nout: 12, or 5..16 in the any-A forms)
    const float* old_mu;     // [M, A]
    const float* old_sigma;  // [M, A]
    const float* sigma;      // [A] shared std
    const float* old_logp;   // [M]
    const float* adv;        // [M]
    const float* values;     // [M]
    const float* target_values;  // [M]
    const float* returns;    // [M]
    const uint4* w_t_img;    // x6 image of W_out^T (layout 0): row n = hidden column, k = action
    float* wpart;            // [tiles][act_tile_floats(A)] (kActTileFloats at 12)
    float* grad_sigma;       // [A]
    float* stats;            // [8]
    float* grad_mu;          // [M, A] or null
    double* partials;        // [4 + A][tiles], then [4 + A][groups]
    unsigned* tickets;       // 1 + groups, zero between launches
    float clip, ratio_lo, ratio_hi, g_surr, g_ent, value_loss_coef, entropy_coef;
    int clipped_value, compute_kl, kl_fast;
};

// Branch-free masked 16-byte load: out-of-range rows / k-groups read a valid address (the row base) and
// are zeroed by a select, so the load stream has no control flow.  Needs K % 4 == 0.
__device__ __forceinline__ float4 load4_masked(const float* __restrict__ row_base, bool ok, int k) {
    const float4 v = *reinterpret_cast<const float4*>(ok ? row_base + k : row_base);
    return ok ? v : make_float4(0.f, 0.f, 0.f, 0.f);
}

// Row stride of c, h and the column-sum partials.  A dense problem's is its width N -- on a full tile kBN, a
// compile-time constant.  A unit that defines RSLRL_GEMM_WIDE before it includes this header (mlp_wide.hip)
// instantiates the same device code on WideGemmParams, one 256-column block of a wider layer, whose stride is the
// layer's width.  (The preprocessor and not a template parameter: the dense units then compile the token stream they
// always did, and their kernels stay instruction for instruction what they were.)
#ifdef RSLRL_GEMM_WIDE
using GemmP = WideGemmParams;
#define RSLRL_GEMM_LD_FULL(p) (p).ld
#define RSLRL_GEMM_LD(p) (p).ld
#else
using GemmP = GemmParams;
#define RSLRL_GEMM_LD_FULL(p) kBN
#define RSLRL_GEMM_LD(p) (p).N
#endif

// ---- epilogue of one wave's I x J grid of 32x32 tiles at (wrow0, wcol0).  C/D map of a tile:
// col = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5).  Tiles are processed in order b = J i + j;
// for the ELU' epilogue the 16 h values of tile b + 1 are loaded before tile b is finished, so no h load
// waits alone.  colpart[j] returns this lane's sum over its rows of column wcol0 + 32 j + (lane & 31).
template <int EPI, int I, int J, bool FULLT, int NR>
__device__ __forceinline__ void epilogue_tiles_impl(const GemmP& p, f32x16 (&acc)[I][J], int64_t wrow0,
                                                    int wcol0, float (&colpart)[J], const float* dzo, int dzo_row0,
                                                    f32x2 (&wacc)[NR], float& amx) {
    constexpr bool full = FULLT;
    constexpr bool GRAD = EPI == kEpiEluGrad || EPI == kEpiEluGradWgrad;
    const int lane = threadIdx.x & 63;
    const int h = lane >> 5;
    const int l32 = lane & 31;
#pragma unroll
    for (int j = 0; j < J; ++j) colpart[j] = 0.f;
    float hcur[16], hnext[16], hsave[16];
    // full tiles (N == kBN): wave-uniform base pointers (SGPRs) + 32-bit lane offsets with a compile-time row
    // stride -> saddr-form loads/stores whose row-in-group steps fold into the immediate.  A 64-bit address per
    // row (runtime stride) needs 32 VGPRs per tile and spilled ~70 B/lane to scratch around the epilogue.
    const int wr = full ? __builtin_amdgcn_readfirstlane(static_cast<int>(wrow0)) : 0;  // rows < 2^31 (launch)
    const int wc = full ? __builtin_amdgcn_readfirstlane(wcol0) : 0;
    const int64_t ubase = static_cast<int64_t>(wr) * RSLRL_GEMM_LD_FULL(p) + wc;
    auto lane_off = [&](int i, int j, int roff) -> uint32_t {
        return static_cast<uint32_t>((i * 32 + 4 * h + roff) * RSLRL_GEMM_LD_FULL(p) + j * 32 + l32);
    };
    auto load_h = [&](int b, float (&dst)[16]) {
        const int i = b / J, j = b % J;
        if constexpr (full) {
            const float* hb = p.h + ubase;
#pragma unroll
            for (int r = 0; r < 16; ++r) dst[r] = hb[lane_off(i, j, (r & 3) + 8 * (r >> 2))];
            return;
        }
        const int col = wcol0 + j * 32 + l32;
        const int64_t rbase = wrow0 + i * 32 + 4 * h;
        const float* hp = p.h + rbase * RSLRL_GEMM_LD(p) + col;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int roff = (r & 3) + 8 * (r >> 2);
            dst[r] = (rbase + roff < p.M && col < p.N) ? hp[static_cast<int64_t>(roff) * RSLRL_GEMM_LD(p)] : 0.f;
        }
    };
    if constexpr (full && EPI != kEpiEluGradWgrad) {
        // Full tiles: every access through a buffer resource over the wave's rows (wave-uniform base): the
        // lane part of the offset is one VGPR per column tile, the 8-row group step rides in soffset (an SGPR
        // constant) and the row within the group in the 12-bit immediate -- no per-store address arithmetic
        // (the 64-bit vaddr form spent two VALU per store).  The ELU is evaluated branch-free on every lane:
        // as a guarded call the compiler wrapped each element in an exec-mask branch (3 SALU + a skip each).
        const uint32_t rbytes = static_cast<uint32_t>(I * 32 * RSLRL_GEMM_LD_FULL(p) * 4);
        const __amdgpu_buffer_rsrc_t rc = __builtin_amdgcn_make_buffer_rsrc(p.c + ubase, 0, rbytes, 0x00020000);
        const __amdgpu_buffer_rsrc_t rh =
            __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(GRAD ? p.h + ubase : p.c), 0, rbytes, 0x00020000);
        auto voff = [&](int j, int r) {
            return static_cast<int>(((4 * h + (r & 3)) * RSLRL_GEMM_LD_FULL(p) + j * 32 + l32) * 4);
        };
        auto soff = [&](int i, int r) { return (i * 32 + 8 * (r >> 2)) * RSLRL_GEMM_LD_FULL(p) * 4; };
        auto load_hb = [&](int b, float (&dst)[16]) {
            const int i = b / J, j = b % J;
#pragma unroll
            for (int r = 0; r < 16; ++r)
                dst[r] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rh, voff(j, r), soff(i, r), 0));
        };
        if constexpr (EPI == kEpiEluGrad) {
            if (dzo) {  // block 0 was staged in LDS during the last main-loop chunk (row-major 32 x 32)
                // this wave's own DMA must have landed: the barrier after the main loop does not wait for loads
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                const float* hs = dzo + (threadIdx.x >> 6) * (kH0StageBytes / 4);
#pragma unroll
                for (int r = 0; r < 16; ++r) hcur[r] = hs[(4 * h + (r & 3) + 8 * (r >> 2)) * 32 + l32];
            } else {
                load_hb(0, hcur);
            }
        } else if constexpr (GRAD) {
            load_hb(0, hcur);
        }
#pragma unroll
        for (int b = 0; b < I * J; ++b) {
            const int i = b / J, j = b % J;
            if constexpr (GRAD) {
                if (b + 1 < I * J) load_hb(b + 1, hnext);
            }
            float bias = 0.f;
            if constexpr (!GRAD) bias = p.bias[wcol0 + j * 32 + l32];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                float v = acc[i][j][r];
                if constexpr (EPI == kEpiBias) {
                    v = v + bias;
                } else if constexpr (EPI == kEpiBiasElu) {
                    v = v + bias;
                    const float n = elu_neg(fminf(v, 0.f));  // evaluated on every lane: a select, not a branch
                    v = v > 0.f ? v : n;
                } else {
                    const float hv = hcur[r];
                    const float g = v * (hv + 1.f);
                    v = hv > 0.f ? v : g;
                    colpart[j] += v;
                }
                amx = fmaxf(amx, fabsf(v));
                __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(uint32_t, v), rc, voff(j, r), soff(i, r),
                                                      2 /* nt */);
            }
            if constexpr (GRAD) {
#pragma unroll
                for (int r = 0; r < 16; ++r) hcur[r] = hnext[r];
            }
        }
        return;
    }
    if constexpr (GRAD) load_h(0, hcur);
#pragma unroll
    for (int b = 0; b < I * J; ++b) {
        const int i = b / J, j = b % J;
        if constexpr (GRAD) {
            if (b + 1 < I * J) load_h(b + 1, hnext);
        }
        const int col = wcol0 + j * 32 + l32;
        const bool col_ok = col < p.N;
        float bias = 0.f;
        if constexpr (!GRAD) bias = col_ok ? p.bias[col] : 0.f;
        const int64_t rbase = wrow0 + i * 32 + 4 * h;
        float* cp = p.c + rbase * RSLRL_GEMM_LD(p) + col;
        float* cb = p.c + ubase;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int roff = (r & 3) + 8 * (r >> 2);
            if (full || (rbase + roff < p.M && col_ok)) {
                float v = acc[i][j][r];
                if constexpr (EPI == kEpiBias) {
                    v = v + bias;
                } else if constexpr (EPI == kEpiBiasElu) {
                    v = v + bias;
                    v = v > 0.f ? v : elu_neg(v);  // torch ELU, alpha = 1
                } else {  // kEpiEluGrad / kEpiEluGradWgrad
                    const float hv = hcur[r];  // ELU'(z) = 1 if z > 0 else hv + 1
                    v = hv > 0.f ? v : v * (hv + 1.f);
                    colpart[j] += v;
                }
                amx = fmaxf(amx, fabsf(v));
                // streaming store: the outputs are not re-read by this kernel, and keeping them out of L2
                // keeps the B image and the A stream resident (-7% kernel time measured)
                if constexpr (full)
                    __builtin_nontemporal_store(v, cb + lane_off(i, j, roff));
                else
                    __builtin_nontemporal_store(v, cp + static_cast<int64_t>(roff) * RSLRL_GEMM_LD(p));
            }
        }
        if constexpr (EPI == kEpiEluGradWgrad) {
            // dW[o][col] += dZ[row][o] * H[row][col] over this lane's 16 rows (H = 0 outside the matrix); the two
            // column tiles of row tile i share each dZ read and one packed FMA (v_pk_fma_f32)
            static_assert(J == 2, "the fused weight gradient pairs the wave's two column tiles");
            if (j == 0) {
#pragma unroll
                for (int r = 0; r < 16; ++r) hsave[r] = hcur[r];
            } else {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int roff = (r & 3) + 8 * (r >> 2);
                    const float4* d =
                        reinterpret_cast<const float4*>(dzo + (dzo_row0 + i * 32 + 4 * h + roff) * kMaxWgradRows);
                    const f32x2 hh = {hsave[r], hcur[r]};
#pragma unroll
                    for (int o4 = 0; o4 < NR / 4; ++o4) {
                        const float4 dv = d[o4];
                        wacc[4 * o4 + 0] = __builtin_elementwise_fma(f32x2{dv.x, dv.x}, hh, wacc[4 * o4 + 0]);
                        wacc[4 * o4 + 1] = __builtin_elementwise_fma(f32x2{dv.y, dv.y}, hh, wacc[4 * o4 + 1]);
                        wacc[4 * o4 + 2] = __builtin_elementwise_fma(f32x2{dv.z, dv.z}, hh, wacc[4 * o4 + 2]);
                        wacc[4 * o4 + 3] = __builtin_elementwise_fma(f32x2{dv.w, dv.w}, hh, wacc[4 * o4 + 3]);
                    }
                }
            }
        }
        if constexpr (GRAD) {
#pragma unroll
            for (int r = 0; r < 16; ++r) hcur[r] = hnext[r];
        }
    }
}

// full (wave-uniform): every row and column of the tile exists.  The two paths are separate code: a
// runtime `full ||` test per element puts a branch around every store, and the compiler then waits
// vmcnt(0) before each store (64 serialised stores per wave: the epilogue ran 3x longer).
// h0 (kEpiEluGrad, full tiles): the LDS copy of each wave's first H block (stage_h_block0), or nullptr
template <int EPI, int I, int J>
__device__ __forceinline__ void epilogue_tiles(const GemmP& p, f32x16 (&acc)[I][J], int64_t wrow0, int wcol0,
                                               bool full, float (&colpart)[J], float& amx, const float* h0 = nullptr) {
    f32x2 wacc[1];  // unused (no weight-gradient accumulation)
    if (full)
        epilogue_tiles_impl<EPI, I, J, true, 1>(p, acc, wrow0, wcol0, colpart, h0, 0, wacc, amx);
    else
        epilogue_tiles_impl<EPI, I, J, false, 1>(p, acc, wrow0, wcol0, colpart, nullptr, 0, wacc, amx);
}

template <int EPI, int I, int J, int NR>
__device__ __forceinline__ void epilogue_tiles_w(const GemmP& p, f32x16 (&acc)[I][J], int64_t wrow0, int wcol0,
                                                 bool full, float (&colpart)[J], const float* dzo, int dzo_row0,
                                                 f32x2 (&wacc)[NR], float& amx) {
#pragma unroll
    for (int o = 0; o < NR; ++o) wacc[o] = f32x2{0.f, 0.f};
    if (full)
        epilogue_tiles_impl<EPI, I, J, true, NR>(p, acc, wrow0, wcol0, colpart, dzo, dzo_row0, wacc, amx);
    else
        epilogue_tiles_impl<EPI, I, J, false, NR>(p, acc, wrow0, wcol0, colpart, dzo, dzo_row0, wacc, amx);
}

// A chunk: BM rows x 16 k = BM / 128 float4 per thread (unit u = t + 512 i: row u >> 2, k-quad u & 3).
// FULL: the tile's rows exist and K % 16 == 0 -> no masks.
template <int BM, int NT = kThreads>
struct AStage {
    float4 v[BM * 4 / NT];
};

template <int BM, bool FULL, int NT = kThreads>
__device__ __forceinline__ AStage<BM, NT> load_a(const GemmParams& p, int64_t row0, int k0) {
    AStage<BM, NT> s;
#pragma unroll
    for (int i = 0; i < BM * 4 / NT; ++i) {
        const int u = threadIdx.x + NT * i;
        const int k = k0 + 4 * (u & 3);
        const int64_t row = row0 + (u >> 2);
        if constexpr (FULL) {
            s.v[i] = *reinterpret_cast<const float4*>(p.a + row * p.K + k);
        } else {
            const bool row_ok = row < p.M;
#ifdef RSLRL_GEMM_RAGGED
            // K % 4 != 0 (mlp_ragged.hip): rows at 4-byte-aligned bases, the last quad masked element by element
            s.v[i] = load4_ragged_any(p.a + (row_ok ? row : row0) * p.K, k, p.K, p.K >= 4, row_ok);
#else
            s.v[i] = load4_masked(p.a + (row_ok ? row : row0) * p.K, row_ok && k < p.K, k);
#endif
        }
    }
    return s;
}

// PL planes (3: x6 bf16, 2: h3 fp16 of the operand scaled by sc, a power of two)
template <int BM, int PL, int NT = kThreads>
__device__ __forceinline__ void store_a_split(const AStage<BM, NT>& s, char* __restrict__ a_lds, float sc) {
    constexpr int plane = BM * kX6RowB;
#pragma unroll
    for (int i = 0; i < BM * 4 / NT; ++i) {
        const int u = threadIdx.x + NT * i;
        const int q = u & 3;
        const int r = u >> 2;
        const int off = swz(r, q >> 1) + 8 * (q & 1);
        uint2 w[PL];
        float4 v = s.v[i];
        if constexpr (PL == 2) v = make_float4(v.x * sc, v.y * sc, v.z * sc, v.w * sc);
        Arith<PL>::split(v, w);
#pragma unroll
        for (int q2 = 0; q2 < PL; ++q2) *reinterpret_cast<uint2*>(a_lds + q2 * plane + off) = w[q2];
    }
}

// B chunk c of the image -> LDS: PL x 512 16-B units, thread t copies units t, t + 512, ...; the LDS
// destination of a wave's global_load_lds is (wave-uniform base) + 16 * lane.
template <int PL>
__device__ __forceinline__ void load_b_lds(const uint4* __restrict__ img, int c, char* b_lds) {
    const int t = threadIdx.x;
    const uint4* src = img + static_cast<int64_t>(c) * (PL * kX6PlaneB / 16);
#pragma unroll
    for (int i = 0; i < PL; ++i) {
        const int u = t + kThreads * i;
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src + u),
                                         (__attribute__((address_space(3))) void*)(b_lds + 16 * (u & ~63)), 16, 0, 0);
    }
}

template <typename F = bf16x8>
__device__ __forceinline__ F read_frag(const char* __restrict__ plane, int row, int h) {
    return __builtin_bit_cast(F, *reinterpret_cast<const uint4*>(plane + swz(row, h)));
}


#ifndef RSLRL_H3_DEPTH
#define RSLRL_H3_DEPTH 3
#endif
constexpr int kH3Depth = RSLRL_H3_DEPTH;  // A look-ahead (chunks) of the unrolled h3 main loop
#ifndef RSLRL_X6_DEPTH
#define RSLRL_X6_DEPTH 1
#endif
// the same loop on x6 operands (three planes: more fragment registers).  Measured at M = 393,216 (one process
// per build, scripts/x6_probe.py): depth 1 / 2 / 3 -> fwd 329 / 352 / 335 us, dgrad 359 / 375 / 375 us against
// 466-494 us for the generic one-chunk loop; depth 1 is the only one without spills at two workgroups per CU.
constexpr int kX6Depth = RSLRL_X6_DEPTH;
constexpr int kH3DeepDefault = (1 << RSLRL_LINEAR_FWD) | (1 << RSLRL_LINEAR_FWD_ELU) | (1 << RSLRL_LINEAR_DGRAD_ELU) |
                               (1 << RSLRL_LINEAR_FWD_OUT);
__device__ __forceinline__ void amax_commit(const GemmParams& p, float amx) {
    amax_publish<kThreads>(p.amax_out, p.amax_ws, amx);
}

// h3 main loop for a compile-time chunk count (K = 16 NCH, full tiles), fully unrolled so the A operand can be
// fetched D chunks ahead into registers (sa_[k % D] holds chunk k) -- the one-chunk look-ahead of the generic
// loop leaves each chunk waiting out an HBM load latency.  The B image chunk goes through registers as well
// (16-byte loads + ds_write_b128, one chunk ahead): with a global_load_lds DMA in flight the compiler waits
// vmcnt(0) before every LDS read (it cannot tell the DMA's buffer from the one being read), which would drain
// the A look-ahead every chunk.  Per chunk c: read every fragment of chunk c, write A(c+1) and B(c+1) into the
// other buffer, fetch A(c+1+D) and B(c+2), MFMAs, barrier (LDS writes only: lgkmcnt(0)).
template <int PL, int NT = kThreads>
struct BStage {
    uint4 u[PL * kThreads / NT];
};

template <int PL, int NT = kThreads>
__device__ __forceinline__ BStage<PL, NT> load_b_regs(const uint4* __restrict__ img, int c) {
    const uint4* src = img + static_cast<int64_t>(c) * (PL * kX6PlaneB / 16);
    BStage<PL, NT> b;
#pragma unroll
    for (int i = 0; i < PL * kThreads / NT; ++i) b.u[i] = src[threadIdx.x + NT * i];
    return b;
}

template <int PL, int NT = kThreads>
__device__ __forceinline__ void store_b_regs(BStage<PL, NT>& b, char* b_lds) {
#pragma unroll
    for (int i = 0; i < PL * kThreads / NT; ++i) {
        asm volatile("" : "+v"(b.u[i].x), "+v"(b.u[i].y), "+v"(b.u[i].z), "+v"(b.u[i].w));
        *reinterpret_cast<uint4*>(b_lds + 16 * (threadIdx.x + NT * i)) = b.u[i];
    }
}

#ifndef RSLRL_B_FIRST
#define RSLRL_B_FIRST 1
#endif
constexpr bool kBFirst = RSLRL_B_FIRST != 0;  // deep_pipeline's issue order of the look-ahead loads (A/B build knob)

// The pipeline alone, for any fragment schedule: compute(a_lds, b_lds) reads one chunk's fragments from the
// LDS buffer and issues its MFMAs.
struct NoHook {
    __device__ void operator()(char*) const {}
};

// last_hook(free_buffer): called before the last chunk's compute with the LDS buffer no chunk reads any more
// (a compile-time object: a DMA into it does not make the compiler wait for it before the other buffer's reads)
template <int BM, int PL, int NCH, int D, typename Compute, typename Hook = NoHook, int NT = kThreads>
__device__ __forceinline__ void deep_pipeline(const GemmParams& p, int64_t row0, const uint4* __restrict__ bimg,
                                              char* (&lds)[2], float sa, Compute&& compute, Hook&& last_hook = Hook{}) {
    constexpr int planeA = BM * kX6RowB;
    AStage<BM, NT> sa_[D];
    BStage<PL, NT> sb;
    {
        BStage<PL, NT> b0 = load_b_regs<PL, NT>(bimg, 0);
        store_b_regs<PL, NT>(b0, lds[0] + PL * planeA);
    }
    store_a_split<BM, PL, NT>(load_a<BM, true, NT>(p, row0, 0), lds[0], sa);
#pragma unroll
    for (int d = 1; d <= D; ++d)
        if (d < NCH) sa_[d % D] = load_a<BM, true, NT>(p, row0, d * kKC);
    if (NCH > 1) sb = load_b_regs<PL, NT>(bimg, 1);
    __syncthreads();
    constexpr bool kHook = !std::is_same_v<std::decay_t<Hook>, NoHook>;
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
        if (c + 1 == NCH) last_hook(lds[(c + 1) & 1]);
        compute(lds[c & 1], lds[c & 1] + PL * planeA);
        if (c + 1 < NCH) {  // buffer (c+1)&1 was last read in chunk c-1; every wave passed the barrier after it
            // pin the use of the prefetched registers here: otherwise the scheduler hoists the scaling
            // multiply right behind the load and the wave waits out the look-ahead right away
#pragma unroll
            for (int u = 0; u < BM * 4 / NT; ++u) {
                float4& v = sa_[(c + 1) % D].v[u];
                asm volatile("" : "+v"(v.x), "+v"(v.y), "+v"(v.z), "+v"(v.w));
            }
            store_a_split<BM, PL, NT>(sa_[(c + 1) % D], lds[(c + 1) & 1], sa);
            store_b_regs<PL, NT>(sb, lds[(c + 1) & 1] + PL * planeA);
            if constexpr (kBFirst) {
                // B (one chunk ahead) issued before A (D chunks ahead): vmcnt retires in issue order, so the next
                // chunk's wait for this B leaves the younger A loads in flight.  Issued after A, that wait was a
                // vmcnt(0) every chunk -- the A look-ahead drained down to one chunk (the .s of the w4 kernel).
                if (c + 2 < NCH) sb = load_b_regs<PL, NT>(bimg, c + 2);
                if (c + 1 + D < NCH) sa_[(c + 1) % D] = load_a<BM, true, NT>(p, row0, (c + 1 + D) * kKC);
            } else {
                if (c + 1 + D < NCH) sa_[(c + 1) % D] = load_a<BM, true, NT>(p, row0, (c + 1 + D) * kKC);
                if (c + 2 < NCH) sb = load_b_regs<PL, NT>(bimg, c + 2);
            }
        }
        // only LDS writes to retire (lgkmcnt); __syncthreads' release fence would also wait vmcnt(0) and drain
        // the look-ahead every chunk
        if (c + 1 < NCH) {
            asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
        } else {
            // a hook's LDS DMA may be read by other waves after the barrier, which does not wait for loads
            if constexpr (kHook) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();  // the epilogue may reuse the LDS
        }
    }
}

// Input-gradient epilogue: H block (i = 0, j = 0) of each wave (32 x 32 fp32, row-major, kH0StageBytes at wave *
// kH0StageBytes) DMA'd into the free LDS buffer during the last chunk, so the epilogue's first ELU' does not wait
// out an HBM load (the later blocks are prefetched one ahead in registers).  Full tiles only (the caller checks).
__device__ __forceinline__ void stage_h_block0(const GemmParams& p, int64_t row0, int wm, int wn, char* buf) {
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const float* hb = p.h + (row0 + wm * 64) * kBN + wn * 64;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int r = 8 * k + (lane >> 3), c4 = lane & 7;
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(hb + r * kBN + 4 * c4),
                                         (__attribute__((address_space(3))) void*)(buf + wave * kH0StageBytes + k * 1024),
                                         16, 0, 0);
    }
}

// NW < 4 (the narrow heads, N = 64 NW): the wave columns wn >= NW hold no output column -- they take their share of
// the operand staging and every barrier, and skip the fragment reads and the MFMAs (wn is wave-uniform)
template <int EPI, int BM, int PL, int NCH, int D, typename Frag, int NW = 4>
__device__ __forceinline__ void h3_deep_loop(const GemmParams& p, int64_t row0, const uint4* __restrict__ bimg,
                                             char* (&lds)[2], f32x16 (&acc)[BM / 64][2], float sa, int wm,
                                             int wn, int l32, int h, bool stage_h0 = false) {
    constexpr int I = BM / 64;
    constexpr int planeA = BM * kX6RowB;
    auto hook = [&](char* free_buf) {
        // (the forward's biases staged the same way measured 2-4 % slower: kept as L2 loads)
        if constexpr (EPI == kEpiEluGrad && PL == 3)
            if (stage_h0) stage_h_block0(p, row0, wm, wn, free_buf);
    };
    deep_pipeline<BM, PL, NCH, D>(p, row0, bimg, lds, sa, [&](const char* a_lds, const char* b_lds) {
        if constexpr (NW < 4) {
            if (wn >= NW) return;
        }
        Frag bf[2][PL];
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int q = 0; q < PL; ++q) bf[j][q] = read_frag<Frag>(b_lds + q * kX6PlaneB, wn * 64 + j * 32 + l32, h);
#pragma unroll
        for (int i = 0; i < I; ++i) {
            Frag af[PL];
#pragma unroll
            for (int q = 0; q < PL; ++q) af[q] = read_frag<Frag>(a_lds + q * planeA, wm * (BM / 2) + i * 32 + l32, h);
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                if constexpr (EPI == kEpiBiasEluOut)
                    acc[i][j] = Arith<PL>::mfma(bf[j], af, acc[i][j]);
                else
                    acc[i][j] = Arith<PL>::mfma(af, bf[j], acc[i][j]);
            }
        }
    }, hook);
}

// 128 rows x 256 columns per workgroup: waves 2 (M) x 4 (N) of 64 x 64 (2 x 2 MFMA tiles); MINW = 4:
// two workgroups per CU (<= 128 VGPRs), 2: one (the register-hungrier short-K dgrad epilogues).
// NR: rows of the fused weight gradient (kEpiEluGradWgrad: Nred rounded up to 4); kEpiBiasEluOut: 1 = VALU output
// layer (<= 4 outputs), 4 = MFMA output layer (separate code: one register allocation for both spilled).
// PL: operand planes (3: x6 bf16 on a layout-0 image; 2: h3 fp16 on a layout-2 image, A scaled from *p.a_amax).
// KCH = 3: a kernel for K = 48 only (the first layer), whose look-ahead loop is its only main loop (one body with
// both loop instances ran the K = 256 forward ~2 % slower)
// bytes of each of the two LDS buffers of the x6 GEMM body
template <int EPI, int PL>
constexpr int x6_buf_bytes() {
    // the fused output layer's epilogue needs 40 KiB per buffer (h stage in one, reduction tiles in the other)
    return EPI == kEpiBiasEluOut ? 40960 : (PL * kBM * kX6RowB + PL * kX6PlaneB);
}

// The actor head's epilogue (mlp_heads.hip): last hidden layer's H -> output layer, PPO loss, output-layer backward.
__device__ __forceinline__ void actor_head_epilogue(const GemmParams& p, const ActorParams& ap, f32x16 (&acc)[2][2],
                                                    char* lds0, char* lds1, const float* xsb, int wm, int wn, int lane,
                                                    int wave, int64_t row0);
template <int APL, int NW = 4>
__device__ __forceinline__ void actor_head_any_epilogue(const GemmParams& p, const ActorParams& ap,
                                                        f32x16 (&acc)[2][2], char* lds0, char* lds1, const float* xsb,
                                                        int wm, int wn, int lane, int wave, int64_t row0);

// lds_b0 / lds_b1: the kernel's two LDS buffers (x6_buf_bytes<EPI, PL>() each).  Two LDS objects, not one [2][bytes]
// array: the waitcnt pass can then tell a DMA into one buffer from reads of the other (distinct alias scopes) where
// the buffer index is a compile-time constant.  Declared by the kernel so that two bodies in one kernel (the
// output-layer pair) share them.
// HEAD (kEpiBiasEluOut, NR 1, full tiles): the value head's backward fused behind it (mlp_gemm_x6_value_head_kernel)
// NW (the heads only): live 64-column wave columns, p.N == 64 NW; below 4 the narrow heads (mlp_heads.hip)
template <int EPI, bool FULL, int NR, int PL, bool STAGE = true, int KCH = 0, int HEAD = 0, int NW = 4>
__device__ __forceinline__ void mlp_gemm_x6_body(GemmP p, const uint4* __restrict__ bimg, char* lds_b0,
                                                 char* lds_b1, const ActorParams* ap = nullptr) {
    static_assert(PL == 3 || EPI != kEpiEluGradWgrad, "the fused output-layer backward is x6 only");
    static_assert(NW == 4 || (NW >= 1 && NW < 4 && HEAD != 0 && HEAD != 2), "narrow tiles: the heads' any-A and value forms");
    using Frag = typename Arith<PL>::frag;
    constexpr int BM = kBM;
    constexpr int I = BM / 64;
    constexpr int planeA = BM * kX6RowB;
    constexpr int bufBytes = x6_buf_bytes<EPI, PL>();
    static_assert(bufBytes >= PL * planeA + PL * kX6PlaneB, "LDS buffer");
    char* lds[2];
    lds[0] = lds_b0;
    lds[1] = lds_b1;
    // kEpiBiasEluOut: the bias and (1 output on the VALU: the value head) the fp32 output weights live in the 4 KiB of buffer 0
    // that neither the main loop nor the epilogue uses, so the epilogue's dependent chain reads them from LDS
    // instead of waiting on L2 loads (xs: [256] bias, then [32 (wn, j, s, h)][kXsOut][8] weights)
    // past the main loop's operands and past the epilogue's H stage / reduction tiles (8 waves x 4 KiB)
    constexpr int kXsOff = PL * planeA + PL * kX6PlaneB > 8 * 4096 ? PL * planeA + PL * kX6PlaneB : 8 * 4096;
    constexpr int kXsOut = 1;  // the value head
    constexpr int kVhWOff = kBN + kOutImageThreads / 32 * kXsOut * 8;  // HEAD: floats from xs to the value weights
    if constexpr (EPI == kEpiBiasEluOut) {
        static_assert(kXsOff + 4 * (kBN + kOutImageThreads / 32 * kXsOut * 8) <= bufBytes, "LDS side area");
        float* xs = reinterpret_cast<float*>(lds_b0 + kXsOff);
        const int t = threadIdx.x;
        if (t < kBN / 4)
            reinterpret_cast<float4*>(xs)[t] =
                4 * t < p.N ? *reinterpret_cast<const float4*>(p.bias + 4 * t) : make_float4(0.f, 0.f, 0.f, 0.f);
        if constexpr (NR == 1) {
            // the fp32 section holds kOutImageThreads / 32 = 32 (wn, j, s, h) combinations x 32 outputs
            if (p.nout <= kXsOut && t >= 64 && t < 64 + kOutImageThreads / 32 * kXsOut) {
                const int e = t - 64, combo = e / kXsOut, o = e % kXsOut;
                const float4* src = reinterpret_cast<const float4*>(p.oimg + kOutImagePlaneUnits) + 2 * (combo * 32 + o);
                float4* dst = reinterpret_cast<float4*>(xs + kBN) + 2 * e;
                const bool ok = o < p.nout;
                dst[0] = ok ? src[0] : make_float4(0.f, 0.f, 0.f, 0.f);
                dst[1] = ok ? src[1] : make_float4(0.f, 0.f, 0.f, 0.f);
            }
        }
        if constexpr (HEAD == 2) {
            // the actor head: [output bias | shared std | old std of the mini-batch's sample 0] per action after the bias
            // (actor_head_epilogue's mu and per-action loss constants)
            if (t >= 64 && t < 64 + kActA) {
                const int a = t - 64;
                xs[kBN + a] = p.obias[a];
                xs[kBN + kActA + a] = ap->sigma[a];
                xs[kBN + 2 * kActA + a] = ap->old_sigma[a];
            }
        }
        if constexpr (HEAD > kHeadActorAny) {
            // the actor head for p.nout actions: the same three rows at a stride of kActMaxA; past the per-wave loss
            // partials, the folded columns and the flag that actor_head_any_epilogue keeps from byte 32768 on
            static_assert(32768 + 8 * (9 * kActMaxCols) + 4 <= kXsOff, "actor head: loss partials below the side area");
            static_assert(kXsOff + 4 * (kBN + kActSideRows * kActMaxA) <= bufBytes, "LDS side area (actor head)");
            if (t >= 64 && t < 64 + p.nout) {
                const int a = t - 64;
                xs[kBN + kSideObias * kActMaxA + a] = p.obias[a];
                xs[kBN + kSideSigma * kActMaxA + a] = ap->sigma[a];
                xs[kBN + kSideOldSigma * kActMaxA + a] = ap->old_sigma[a];
            }
        }
        if constexpr (HEAD == 1) {
            // after the side area: the value weight row in column order [N], then the tile's target values and returns
            // [BM] each, DMA'd now (no registers held through the main loop; its final barrier drains them) -- the
            // epilogue replaces the targets by dV
            static_assert(kXsOff + 4 * (kVhWOff + kBN + 2 * BM) <= bufBytes, "LDS side area (value head)");
            if (t >= 128 && t < 128 + NW * 16)  // the row's N = 64 NW weights
                reinterpret_cast<float4*>(xs + kVhWOff)[t - 128] = *reinterpret_cast<const float4*>(p.vh_w + 4 * (t - 128));
            if (t < BM) {
                const int w = t >> 6;  // waves 0 and 1: 64 rows each, lane l -> row 64 w + l
                const int64_t r = static_cast<int64_t>(blockIdx.x) * BM + t;
                __builtin_amdgcn_global_load_lds(
                    (const __attribute__((address_space(1))) void*)(p.vh_tv + r),
                    (__attribute__((address_space(3))) void*)(xs + kVhWOff + kBN + 64 * w), 4, 0, 0);
                __builtin_amdgcn_global_load_lds(
                    (const __attribute__((address_space(1))) void*)(p.vh_ret + r),
                    (__attribute__((address_space(3))) void*)(xs + kVhWOff + kBN + BM + 64 * w), 4, 0, 0);
            }
        }
    }
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // wave-uniform: SGPR arithmetic
    const int wm = wave >> 2;  // rows wm * BM / 2
    const int wn = wave & 3;   // cols wn * 64
    const int h = lane >> 5;
    const int l32 = lane & 31;
    const int64_t row0 = static_cast<int64_t>(blockIdx.x) * BM;

    f32x16 acc[I][2];
#pragma unroll
    for (int i = 0; i < I; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = f32x16{};

    const float sa = PL == 2 ? h3_scale(*p.a_amax) : 1.f;
    bool deep = false;
    // x6 input gradient on a full tile: each wave's first H block goes to the free LDS buffer during the last
    // chunk (stage_h_block0); lds[0] is that buffer for the 16-chunk loop (the last chunk reads lds[1])
    // (the same condition as the deep loop below: FULL, K = 256, p.deep -- the DMA is issued from that loop)
    // STAGE = false (the pair kernel): a spill at its register budget cost more than the staged loads save
    const bool stage_h0 = STAGE && FULL && EPI == kEpiEluGrad && PL == 3 && p.h != nullptr && (row0 + BM <= p.M) &&
                          p.N == kBN && p.K == 16 * kKC && p.deep;
    static_assert(EPI != kEpiEluGrad || PL != 3 || 8 * kH0StageBytes <= bufBytes, "H block stage");
    if constexpr (FULL && KCH == 3) {
        // the first layer (K = 48: three chunks) on the look-ahead loop: the generic loop's per-chunk __syncthreads
        // drains every load, which a three-chunk tile pays in full (the host launches KCH = 3 for K = 48 only)
        h3_deep_loop<EPI, BM, PL, 3, 1, Frag>(p, row0, bimg, lds, acc, sa, wm, wn, l32, h);
        deep = true;
    } else if constexpr (FULL) {
        if (p.K == 16 * kKC && p.deep) {
            h3_deep_loop<EPI, BM, PL, 16, PL == 2 ? kH3Depth : kX6Depth, Frag, NW>(p, row0, bimg, lds, acc, sa, wm, wn,
                                                                                l32, h, stage_h0);
            deep = true;
        }
    }
    // Pipeline: B of chunk c+1 is copied (global_load_lds) and A of chunk c+1 fetched into registers at
    // the start of chunk c; A is split into the other LDS buffer at its end.
    const int nchunks = deep ? 0 : (p.K + kKC - 1) / kKC;
    if (NW == 4 && !deep) {  // (a narrow head is only launched onto the look-ahead loop above)
    load_b_lds<PL>(bimg, 0, lds[0] + PL * planeA);
    store_a_split<BM, PL>(load_a<BM, FULL>(p, row0, 0), lds[0], sa);
    __syncthreads();
    for (int c = 0; c < nchunks; ++c) {
        const int buf = c & 1;
        const bool more = c + 1 < nchunks;
        const char* a_lds = lds[buf];
        const char* b_lds = lds[buf] + PL * planeA;
        AStage<BM> an;
        Frag bf[2][PL];
        if constexpr (PL == 2) {
            // h3: every fragment of the chunk is read before the next chunk's loads issue -- the compiler
            // cannot tell the global_load_lds destination (the other buffer) from this one and waits
            // vmcnt(0) before any LDS read that follows it, which would expose the loads' full latency
            Frag af[I][PL];
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int q = 0; q < PL; ++q)
                    bf[j][q] = read_frag<Frag>(b_lds + q * kX6PlaneB, wn * 64 + j * 32 + l32, h);
#pragma unroll
            for (int i = 0; i < I; ++i)
#pragma unroll
                for (int q = 0; q < PL; ++q)
                    af[i][q] = read_frag<Frag>(a_lds + q * planeA, wm * (BM / 2) + i * 32 + l32, h);
            if (more) {  // the other buffer was last read in chunk c-1, and every wave passed the barrier after it
                load_b_lds<PL>(bimg, c + 1, lds[buf ^ 1] + PL * planeA);
                an = load_a<BM, FULL>(p, row0, (c + 1) * kKC);
            }
#pragma unroll
            for (int i = 0; i < I; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    if constexpr (EPI == kEpiBiasEluOut)  // C^T tile: the weight fragment is the MFMA's A operand
                        acc[i][j] = Arith<PL>::mfma(bf[j], af[i], acc[i][j]);
                    else
                        acc[i][j] = Arith<PL>::mfma(af[i], bf[j], acc[i][j]);
                }
        } else {
            if (more) {  // the other buffer was last read in chunk c-1, and every wave passed the barrier after it
                load_b_lds<PL>(bimg, c + 1, lds[buf ^ 1] + PL * planeA);
                an = load_a<BM, FULL>(p, row0, (c + 1) * kKC);
            }
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int q = 0; q < PL; ++q)
                    bf[j][q] = read_frag<Frag>(b_lds + q * kX6PlaneB, wn * 64 + j * 32 + l32, h);
#pragma unroll
            for (int i = 0; i < I; ++i) {
                Frag af[PL];
#pragma unroll
                for (int q = 0; q < PL; ++q)
                    af[q] = read_frag<Frag>(a_lds + q * planeA, wm * (BM / 2) + i * 32 + l32, h);
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    if constexpr (EPI == kEpiBiasEluOut)  // C^T tile: the weight fragment is the MFMA's A operand
                        acc[i][j] = Arith<PL>::mfma(bf[j], af, acc[i][j]);
                    else
                        acc[i][j] = Arith<PL>::mfma(af, bf[j], acc[i][j]);
                }
            }
        }
        if (more) store_a_split<BM, PL>(an, lds[buf ^ 1], sa);
        __syncthreads();  // also retires the global_load_lds of chunk c+1 (vmcnt(0))
    }
    }  // !deep
    const float inv_sa = 1.f / sa;
    if constexpr (PL == 2) {
        // undo the operand scales: C[m][n] = acc / (s_a t_n), exact (powers of two)
        const float* inv_t =
            reinterpret_cast<const float*>(reinterpret_cast<const char*>(bimg) + h3_image_scales_offset(p.K));
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            if constexpr (EPI == kEpiBiasEluOut) {
                // C^T tiles: unscaled column by column in the epilogue below (its bias loads)
            } else {
                const float f = inv_t[wn * 64 + j * 32 + l32] * inv_sa;
#pragma unroll
                for (int i = 0; i < I; ++i)
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[i][j][r] *= f;
            }
        }
    }

    const bool full = (row0 + BM <= p.M) && (p.N == kBN);
    float colpart[2];
    float amx = 0.f;  // max |stored output| of this lane (amax_commit)
    if constexpr (EPI == kEpiEluGradWgrad) {
        // one chunk (K <= 16): buffer 0 holds the tile's dZ planes; rebuild the fp32 rows (p0 + p1 + p2 is
        // exact) into buffer 1 as [128][16] for the weight-gradient accumulation
        float* dzo = reinterpret_cast<float*>(lds[1]);
        {
            const int r = threadIdx.x >> 2, q = threadIdx.x & 3;
            const int off = swz(r, q >> 1) + 8 * (q & 1);
            const uint2 p0 = *reinterpret_cast<const uint2*>(lds[0] + off);
            const uint2 p1 = *reinterpret_cast<const uint2*>(lds[0] + planeA + off);
            const uint2 p2 = *reinterpret_cast<const uint2*>(lds[0] + 2 * planeA + off);
            auto lo = [](uint32_t w) { return __uint_as_float(w << 16); };
            auto hi = [](uint32_t w) { return __uint_as_float(w & 0xffff0000u); };
            float4 v;
            v.x = (lo(p0.x) + lo(p1.x)) + lo(p2.x);
            v.y = (hi(p0.x) + hi(p1.x)) + hi(p2.x);
            v.z = (lo(p0.y) + lo(p1.y)) + lo(p2.y);
            v.w = (hi(p0.y) + hi(p1.y)) + hi(p2.y);
            *reinterpret_cast<float4*>(dzo + r * kMaxWgradRows + 4 * q) = v;
        }
        __syncthreads();
        f32x2 wacc[NR];
        epilogue_tiles_w<EPI, I, 2, NR>(p, acc, row0 + wm * (BM / 2), wn * 64, full, colpart, dzo, wm * (BM / 2), wacc,
                                        amx);
        // per-tile partial dW[o][col]: lane halves (rows 4h..) by shuffle, then the two wave rows in a fixed
        // order through LDS (the B region of buffer 0 is free after the main loop)
        float* red = reinterpret_cast<float*>(lds[0] + 3 * planeA);  // [16][256]
#pragma unroll
        for (int o = 0; o < NR; ++o)
#pragma unroll
            for (int j = 0; j < 2; ++j) wacc[o][j] += __shfl_xor(wacc[o][j], 32, 64);
        if (wm == 0 && h == 0) {
#pragma unroll
            for (int o = 0; o < NR; ++o)
#pragma unroll
                for (int j = 0; j < 2; ++j) red[o * kBN + wn * 64 + j * 32 + l32] = wacc[o][j];
        }
        __syncthreads();
        // per-tile partial sums of dZ itself (the layer's bias gradient): wave 0, lane (q, c) sums rows
        // 32 q .. 32 q + 31 of column c in order, the four quarters are added in order
        const int64_t tile_floats = static_cast<int64_t>(p.K) * p.N + p.K;
        if (threadIdx.x < 64) {
            const int c = threadIdx.x & 15, q = threadIdx.x >> 4;
            float sz = 0.f;
            for (int r = 32 * q; r < 32 * q + 32; ++r) sz += dzo[r * kMaxWgradRows + c];
            const float s1 = __shfl(sz, c + 16, 64), s2 = __shfl(sz, c + 32, 64), s3 = __shfl(sz, c + 48, 64);
            if (q == 0 && c < p.K)
                p.wpart[static_cast<int64_t>(blockIdx.x) * tile_floats + static_cast<int64_t>(p.K) * p.N + c] =
                    ((sz + s1) + s2) + s3;
        }
        if (wm == 1 && h == 0) {
            float* out = p.wpart + static_cast<int64_t>(blockIdx.x) * tile_floats;
#pragma unroll
            for (int o = 0; o < NR; ++o)
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const int col = wn * 64 + j * 32 + l32;
                    if (o < p.K && col < p.N) out[o * p.N + col] = red[o * kBN + col] + wacc[o][j];
                }
        }
    } else if constexpr (EPI == kEpiBiasEluOut && HEAD == 2) {
        static_assert(FULL && PL == 3, "actor head: full x6 tiles");
        actor_head_epilogue(p, *ap, acc, lds_b0, lds_b1, reinterpret_cast<const float*>(lds_b0 + kXsOff), wm, wn, lane,
                            wave, row0);
    } else if constexpr (EPI == kEpiBiasEluOut && HEAD > kHeadActorAny) {
        static_assert(FULL && PL == 3, "actor head: full x6 tiles");
        actor_head_any_epilogue<HEAD - kHeadActorAny, NW>(p, *ap, acc, lds_b0, lds_b1,
                                                          reinterpret_cast<const float*>(lds_b0 + kXsOff), wm, wn, lane,
                                                          wave, row0);
    } else if constexpr (EPI == kEpiBiasEluOut && HEAD == 1) {
        // The critic's head with its backward.  V = ELU(acc + b) w^T + b_out exactly as the plain value-head epilogue
        // below computes it (same operations, same order: the same bits), then dV = d loss / dV per row
        // (value_loss_grad), then the output layer's backward over the H tile still in registers (acc holds H after
        // the first pass): dZ = (dV w) * ELU'(H) -> p.c through the per-wave stage (whole-line stores), and this
        // tile's partial row of p.wpart = [dW = sum dV H | db = sum dV | 0 pad] (out_bwd_valu_body's layout; the
        // reduction order over the tile's rows differs).  dZ per element is out_bwd_valu_body's expression: the same
        // bits.  H never reaches HBM, and the output layer's backward reads nothing back.
        static_assert(NR == 1 && FULL && PL == 3, "value head: full x6 tiles, the VALU value head");
        float* xsb = reinterpret_cast<float*>(lds_b0 + kXsOff);
        float* wvl = xsb + kVhWOff;  // [N] value weights, column order
        float* dvl = wvl + kBN;      // [BM] the tile's target values (prologue DMA), replaced by dV
        const float* retl = dvl + BM;  // [BM] the tile's returns (prologue DMA)
        float* red = reinterpret_cast<float*>(lds[1]);  // [wm][wn][i][32] V partials (2 KiB)
        float* hred = reinterpret_cast<float*>(lds[1]) + 1024;  // [dZ sums wm 0, 1 | dW sums wm 0, 1][N] (4 KiB)
        // two 32 x 32 H blocks per wave in LDS (the i = 1 row of blocks, written in the first pass: 32 registers fewer
        // held through the dV step): area A = buffer 0 (block j = 1), area B = buffer 1 past red / hred (block j = 0);
        // each later stages one of the wave's i = 0 blocks.  Layout of the whole-line store stage: float4 column quads
        // XOR-swizzled by (row >> 1) & 7.
        float* const area0 = reinterpret_cast<float*>(lds[1] + 8192) + wave * 1024;
        float* const area1 = reinterpret_cast<float*>(lds[0]) + wave * 1024;
        static_assert(8192 + 8 * 4096 <= bufBytes, "value head: H blocks in LDS");
        auto stage_block = [&](float* blk, f32x16 v) {
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const f32x4 hv = {v[4 * g], v[4 * g + 1], v[4 * g + 2], v[4 * g + 3]};
                *reinterpret_cast<f32x4*>(blk + l32 * 32 + 4 * ((2 * g + h) ^ ((l32 >> 1) & 7))) = hv;
            }
        };
        // NW < 4: a wave column past N holds no H -- its V partials are the exact zeros the plain epilogue's zero-padded
        // columns give (the sum below keeps its four terms and their order), and it owns no dZ or dW column
        const bool live = NW == 4 || wn < NW;  // wave-uniform
        if constexpr (NW < 4) {
            if (!live && h == 0) {
#pragma unroll
                for (int i = 0; i < I; ++i) red[((wm * 4 + wn) * I + i) * 32 + l32] = 0.f;
            }
        }
#pragma unroll
        for (int ii = 0; ii < I; ++ii) {
            if (!live) continue;
            const int i = I - 1 - ii;  // the parked row of blocks first: its registers die before the other's H forms
            float oval = 0.f;
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int cb = wn * 64 + j * 32 + 4 * h;
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const float4 b4 = *reinterpret_cast<const float4*>(xsb + cb + 8 * g);
                    float t[4] = {acc[i][j][4 * g], acc[i][j][4 * g + 1], acc[i][j][4 * g + 2], acc[i][j][4 * g + 3]};
                    t[0] += b4.x;
                    t[1] += b4.y;
                    t[2] += b4.z;
                    t[3] += b4.w;
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float n = elu_neg(fminf(t[e], 0.f));
                        acc[i][j][4 * g + e] = t[e] > 0.f ? t[e] : n;
                    }
                }
                const float4* wl = reinterpret_cast<const float4*>(xsb + kBN) + 2 * ((((wn * 2 + j) * 2) * 2 + h) * kXsOut);
#pragma unroll
                for (int s2 = 0; s2 < 2; ++s2) {
                    const float4* q = wl + 2 * (s2 * 2 * kXsOut);
                    const float4 w0 = q[0], w1 = q[1];
                    const float w[8] = {w0.x, w0.y, w0.z, w0.w, w1.x, w1.y, w1.z, w1.w};
#pragma unroll
                    for (int t = 0; t < 8; ++t) oval = fmaf(acc[i][j][8 * s2 + t], w[t], oval);
                }
                if (i == I - 1) stage_block(j ? area1 : area0, acc[i][j]);
            }
            const float tsum = oval + __shfl_xor(oval, 32, 64);
            if (h == 0) red[((wm * 4 + wn) * I + i) * 32 + l32] = tsum;
        }
        __syncthreads();
        if (threadIdx.x < BM) {  // the four wn partials in the plain epilogue's order
            const int rl = threadIdx.x;
            const float tv = dvl[rl], ret = retl[rl];
            const float* b = red + (rl >> 6) * 4 * I * 32 + ((rl & 63) >> 5) * 32 + (rl & 31);
            const float sum = ((b[0] + b[I * 32]) + b[2 * I * 32]) + b[3 * I * 32];
            const float V = sum + p.obias[0];
            p.y[row0 + rl] = V;
            dvl[rl] = value_loss_grad(V, tv, ret, p.vh_clipped, p.vh_clip, p.vh_g);
        }
        __syncthreads();
        const int cq = lane & 7;
        // dZ of one staged block (i, j): lane (row 8 k + lane >> 3, column quad cq) -> whole-line stores
        auto block_bwd = [&](const float* blk, int i, int j, float (&cs)[4], float (&wsum)[4]) {
            const int64_t trow = row0 + wm * (BM / 2) + i * 32;
            float* ct = p.c + trow * p.N + (wn * 64 + j * 32);
            const float4 w4 = *reinterpret_cast<const float4*>(wvl + wn * 64 + j * 32 + 4 * cq);
            const float w[4] = {w4.x, w4.y, w4.z, w4.w};
#pragma unroll 1
            for (int k = 0; k < 4; ++k) {
                const int sr = 8 * k + (lane >> 3);
                const f32x4 hq = *reinterpret_cast<const f32x4*>(blk + sr * 32 + 4 * (cq ^ ((sr >> 1) & 7)));
                const float hh4[4] = {hq[0], hq[1], hq[2], hq[3]};
                const float dv = dvl[wm * (BM / 2) + i * 32 + sr];
                float o[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float hh = hh4[e];
                    const float z = __fmaf_rn(dv, w[e], 0.f);  // out_bwd_valu_body's fma chain of one term
                    const float v = hh > 0.f ? z : z * (hh + 1.f);  // ELU'(x) = 1 if h > 0 else h + 1
                    o[e] = v;
                    cs[e] += v;
                    wsum[e] = fmaf(dv, hh, wsum[e]);
                }
                const f32x4 ov = {o[0], o[1], o[2], o[3]};
                f32x4* dst = reinterpret_cast<f32x4*>(ct + static_cast<uint32_t>(sr * p.N + 4 * cq));
                if (p.nt) __builtin_nontemporal_store(ov, dst);
                else *dst = ov;
            }
        };
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            if (!live) continue;
            float cs[4] = {0.f, 0.f, 0.f, 0.f}, wsum[4] = {0.f, 0.f, 0.f, 0.f};
            float* const blk = j ? area1 : area0;
            block_bwd(blk, I - 1, j, cs, wsum);  // the block parked in the first pass
            __builtin_amdgcn_wave_barrier();     // one wave's LDS accesses execute in order
            stage_block(blk, acc[0][j]);         // then block (0, j) through the same area
            __builtin_amdgcn_wave_barrier();
            block_bwd(blk, 0, j, cs, wsum);
            // column sums over the wave's 64 rows: lanes of one column quad (lane & 7) differ in lane >> 3
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int off = 8; off < 64; off <<= 1) {
                    cs[e] += __shfl_xor(cs[e], off, 64);
                    wsum[e] += __shfl_xor(wsum[e], off, 64);
                }
            if (lane < 8) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int col = wn * 64 + j * 32 + 4 * lane + e;
                    hred[wm * kBN + col] = cs[e];
                    hred[(2 + wm) * kBN + col] = wsum[e];
                }
            }
        }
        __syncthreads();
        const int64_t tile_floats = (static_cast<int64_t>(p.N) + 1 + 3) / 4 * 4;  // dgrad_wgrad_tile_floats(1, N)
        float* wp = p.wpart + static_cast<int64_t>(blockIdx.x) * tile_floats;
        constexpr int kN = NW * 64;  // = p.N (kBN unless a narrow head)
        if (threadIdx.x < kN) {
            const int c = threadIdx.x;
            wp[c] = hred[2 * kBN + c] + hred[3 * kBN + c];
            if (p.colsum) p.colsum[static_cast<int64_t>(blockIdx.x) * p.N + c] = hred[c] + hred[kBN + c];
        }
        if (threadIdx.x < 64) {  // db = sum of the tile's dV (fixed butterfly order)
            float sv = dvl[lane] + dvl[lane + 64];
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) sv += __shfl_xor(sv, off, 64);
            if (lane == 0) wp[kN] = sv;
            else if (lane < static_cast<int>(tile_floats - kN)) wp[kN + lane] = 0.f;
        }
    } else if constexpr (EPI == kEpiBiasEluOut) {
        // C^T tiles: lane (l32, h) holds row l32 of the tile, columns (r & 3) + 8 (r >> 2) + 4 h (r < 16).
        // h = ELU(acc + b) is stored (when wanted) as float4 column quads, split into bf16 planes in
        // registers and multiplied by the output weight: Y'[o][row] = sum over this wave's 64 columns,
        // 2 k steps of 16 per 32-column tile (lane half h carries columns {0-3, 8-11} + 4 h, then
        // {16-19, 24-27} + 4 h; the image orders the weight the same way).  The four wn waves' partial
        // Y' tiles are added in a fixed order through LDS.
        // h leaves through a per-wave LDS stage (32 x 32 floats, float4 quads XOR-swizzled by (row >> 1) & 7):
        // written as the C^T quads, read back as 8 rows x 128 B per instruction -> whole-line stores (direct
        // C^T stores write 32-B pieces: +48 us per launch at M = 393216).  red: [wm][wn][i][o][32 rows].
        const bool staged = p.c != nullptr && p.nout <= kStagedOutWidth;
        const int red_rows = staged ? kStagedOutWidth : 32;
        // stage: buffer 0 (32 KiB); red: [wm][wn][i][o][32] in buffer 1 when staged (<= 40 KiB), else wave row wm
        // in buffer wm (32 KiB each)
        float* stage = reinterpret_cast<float*>(lds[0]) + wave * 1024;
        const int tile = red_rows * 32;
        auto red_of = [&](int w) {
            return staged ? reinterpret_cast<float*>(lds[1]) + w * 4 * I * tile : reinterpret_cast<float*>(lds[w]);
        };
        const uint4* oimg = p.oimg + wn * (2 * 2 * 3 * 64);
        constexpr bool valu = NR == 1;  // the critic's value head: VALU dot products beat 32-row MFMA tiles
#pragma unroll
        for (int i = 0; i < I; ++i) {
            const int64_t row = row0 + wm * (BM / 2) + i * 32 + l32;
            const bool row_ok = row < p.M;
            f32x16 oacc = f32x16{};
            float oval[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int cb = wn * 64 + j * 32 + 4 * h;
                float v[16];
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int col = cb + 8 * g;
                    const bool col_ok = col < p.N;  // N % 4 == 0
                    // (zero past N in the LDS copy)
                    const float4 b4 = *reinterpret_cast<const float4*>(reinterpret_cast<const float*>(lds[0] + kXsOff) + col);
                    float t[4] = {acc[i][j][4 * g], acc[i][j][4 * g + 1], acc[i][j][4 * g + 2], acc[i][j][4 * g + 3]};
                    if constexpr (PL == 2) {  // h3: C = acc / (s_a t_n), exact
                        const float4 f4 = *reinterpret_cast<const float4*>(
                            reinterpret_cast<const float*>(reinterpret_cast<const char*>(bimg) +
                                                           h3_image_scales_offset(p.K)) + col);
                        t[0] *= f4.x * inv_sa;
                        t[1] *= f4.y * inv_sa;
                        t[2] *= f4.z * inv_sa;
                        t[3] *= f4.w * inv_sa;
                    }
                    t[0] += b4.x;
                    t[1] += b4.y;
                    t[2] += b4.z;
                    t[3] += b4.w;
#pragma unroll
                    for (int e = 0; e < 4; ++e) {  // branch-free (see the full-tile epilogue)
                        const float n = elu_neg(fminf(t[e], 0.f));
                        v[4 * g + e] = t[e] > 0.f ? t[e] : n;
                    }
                    const f32x4 hv = {v[4 * g], v[4 * g + 1], v[4 * g + 2], v[4 * g + 3]};
                    if (staged) {
                        *reinterpret_cast<f32x4*>(stage + l32 * 32 + 4 * ((2 * g + h) ^ ((l32 >> 1) & 7))) = hv;
                    } else if (p.c && row_ok && col_ok) {
                        *reinterpret_cast<f32x4*>(p.c + row * p.N + col) = hv;
                    }
                }
                if (staged) {
                    __builtin_amdgcn_wave_barrier();  // one wave's LDS accesses execute in order
                    // wave-uniform tile base + 32-bit lane offsets (one VGPR per store, not a 64-bit address)
                    const int64_t trow = row0 + wm * (BM / 2) + i * 32;
                    float* ct = p.c + trow * p.N + (wn * 64 + j * 32);
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const int sr = 8 * k + (lane >> 3);
                        const int cq = lane & 7;
                        const f32x4 hv = *reinterpret_cast<const f32x4*>(stage + sr * 32 + 4 * (cq ^ ((sr >> 1) & 7)));
                        const int gcol = wn * 64 + j * 32 + 4 * cq;
                        if (trow + sr < p.M && gcol < p.N) {
                            f32x4* dst = reinterpret_cast<f32x4*>(ct + static_cast<uint32_t>(sr * p.N + 4 * cq));
                            if (p.nt) __builtin_nontemporal_store(hv, dst);
                            else *dst = hv;
                        }
                    }
                    __builtin_amdgcn_wave_barrier();
                }
                if constexpr (valu) {
                    // <= 4 outputs: fp32 FMA chains over the lane's 16 columns (the image's fp32 copy; for 1
                    // output the copy in LDS, kXsOut entries per (wn, j, s, h))
                    const bool in_lds = p.nout <= kXsOut;
                    const float4* wf = reinterpret_cast<const float4*>(p.oimg + kOutImagePlaneUnits) +
                                       2 * ((((wn * 2 + j) * 2) * 2 + h) * 32);
                    const float4* wl = reinterpret_cast<const float4*>(reinterpret_cast<const float*>(lds[0] + kXsOff) +
                                                                       kBN) + 2 * ((((wn * 2 + j) * 2) * 2 + h) * kXsOut);
#pragma unroll
                    for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
                        for (int o = 0; o < 4; ++o) {
                            if (o >= p.nout) break;
                            const float4* q = in_lds ? wl + 2 * (s2 * 2 * kXsOut + o) : wf + 2 * (s2 * 64 + o);
                            const float4 w0 = q[0], w1 = q[1];
                            const float w[8] = {w0.x, w0.y, w0.z, w0.w, w1.x, w1.y, w1.z, w1.w};
#pragma unroll
                            for (int t = 0; t < 8; ++t) oval[o] = fmaf(v[8 * s2 + t], w[t], oval[o]);
                        }
                    continue;
                }
#pragma unroll
                for (int s2 = 0; s2 < 2; ++s2) {
                    bf16x8 vb[3], wa[3];
                    uint2 lo[3], hi[3];
                    split4(make_float4(v[8 * s2], v[8 * s2 + 1], v[8 * s2 + 2], v[8 * s2 + 3]), lo[0], lo[1], lo[2]);
                    split4(make_float4(v[8 * s2 + 4], v[8 * s2 + 5], v[8 * s2 + 6], v[8 * s2 + 7]), hi[0], hi[1],
                           hi[2]);
#pragma unroll
                    for (int q = 0; q < 3; ++q) {
                        vb[q] = __builtin_bit_cast(bf16x8, make_uint4(lo[q].x, lo[q].y, hi[q].x, hi[q].y));
                        wa[q] = __builtin_bit_cast(bf16x8, oimg[((j * 2 + s2) * 3 + q) * 64 + lane]);
                    }
                    oacc = mfma_x6(wa, vb, oacc);
                }
            }
            float* rd = red_of(wm) + (wn * I + i) * tile;
            if constexpr (valu) {  // the two lane halves hold different columns of the same row
#pragma unroll
                for (int o = 0; o < 4; ++o) {
                    const float t = oval[o] + __shfl_xor(oval[o], 32, 64);
                    if (h == 0 && o < p.nout) rd[o * 32 + l32] = t;
                }
            } else {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int o = (r & 3) + 8 * (r >> 2) + 4 * h;
                    if (o < red_rows) rd[o * 32 + l32] = oacc[r];
                }
            }
        }
        __syncthreads();
        const int nout = p.nout;
        for (int idx = threadIdx.x; idx < BM * nout; idx += kThreads) {
            const int rl = idx / nout;
            const int o = idx - rl * nout;
            const float* b = red_of(rl >> 6) + ((rl & 63) >> 5) * tile + o * 32 + (rl & 31);
            const float sum = ((b[0] + b[I * tile]) + b[2 * I * tile]) + b[3 * I * tile];
            const int64_t row = row0 + rl;
            if (row < p.M) p.y[row * nout + o] = sum + p.obias[o];
        }
    } else {
        epilogue_tiles<EPI, I, 2>(p, acc, row0 + wm * (BM / 2), wn * 64, full, colpart, amx,
                                  stage_h0 && full ? reinterpret_cast<const float*>(lds[0]) : nullptr);
    }
    // (colsum == nullptr: the previous layer's bias gradient comes from its weight-gradient kernel instead)
    if (EPI == kEpiEluGrad || EPI == kEpiEluGradWgrad) if (p.colsum) {
        // column sums over the tile's 128 rows -> colsum[tile][col]: lanes l and l + 32 hold the two row
        // halves of a column, the two wave rows (wm) are combined in a fixed order through LDS
        float s[2];
#pragma unroll
        for (int j = 0; j < 2; ++j) s[j] = colpart[j] + __shfl_xor(colpart[j], 32, 64);
        float* colred = reinterpret_cast<float*>(lds[0]);
        __syncthreads();  // the LDS tiles are no longer read
#pragma unroll
        for (int j = 0; j < 2; ++j)
            if (h == 0) colred[wm * kBN + wn * 64 + j * 32 + l32] = s[j];
        __syncthreads();
        for (int col = threadIdx.x; col < p.N && col < kBN; col += kThreads)
            p.colsum[static_cast<int64_t>(blockIdx.x) * RSLRL_GEMM_LD(p) + col] = colred[col] + colred[kBN + col];
    }
    if constexpr (EPI != kEpiBiasEluOut) amax_commit(p, amx);
}

template <int EPI, bool FULL, int MINW, int NR = 4, int PL = 3, int KCH = 0>
__global__ __launch_bounds__(kThreads, MINW) void mlp_gemm_x6_kernel(GemmParams p, const uint4* __restrict__ bimg) {
    __shared__ __attribute__((aligned(16))) char lds_b0[x6_buf_bytes<EPI, PL>()];
    __shared__ __attribute__((aligned(16))) char lds_b1[x6_buf_bytes<EPI, PL>()];
    mlp_gemm_x6_body<EPI, FULL, NR, PL, true, KCH>(p, bimg, lds_b0, lds_b1);
}

}  // namespace
}  // namespace rslrl
