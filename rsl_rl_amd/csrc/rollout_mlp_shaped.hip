// The rollout's actor and critic forward in one launch for three-hidden-layer stacks that are not uniformly 256 wide
// (rslrl_rollout_mlp_shaped_pair): [512, 256, 128] (Legged-Gym, Isaac Lab rough terrain), [256, 256, 128],
// [256, 128, 128] (G1 flat) and [128, 128, 128] (Isaac Lab flat), each network on its own input width 1..256 -- the
// 235-float rough-terrain observation included, read in place -- ELU hidden layers, 1..16 outputs, x6 arithmetic, and the
// first network's optional Normal sample.  rollout_mlp.hip takes the 256-wide stacks on 16..64 inputs only; below the
// wide and ragged kernels' row bounds these stacks ran layer by layer through torch (about 14 launches per env step).
//
// Work split: a 32-row tile per 4-wave workgroup, grid (M / 32, 2): at 4,096 envs 128 tiles x 2 networks = 256
// workgroups, one per CU (the 64-row tile of rollout_mlp.hip would leave half of them idle there).  Wave w owns columns
// [w N / 4, (w + 1) N / 4) of each layer as NB = N / 128 C^T accumulator blocks of 32 x 32 (4, 2 or 1: at most 64
// accumulator registers), in rollout_mlp.hip's lane mapping: lane (l32, h) holds row l32 and columns
// 32 j + (r & 3) + 8 (r >> 2) + 4 h of block j.
// LDS (79.5 KiB at [512, 256, 128]: two workgroups per CU):
//   H      32 rows x 512 fp32 (64 KiB), row r's 16-byte unit u at 2048 r + 16 (u ^ (r & 15)): the layer input -- first
//          the observation tile, zero-padded to a multiple of 32 columns, then each layer's ELU output over it, in place,
//          with a barrier between a layer's last read and its epilogue's writes;
//   stage  2 x 6 KiB: a PAIR of 16-deep k-chunks split once per workgroup into its three bf16 planes (every thread
//          splits one quad: rows t & 31, quad t >> 5), double-buffered: one barrier per 32 columns of K.  Plane:
//          [2 chunks][32 rows][32 B], halves swapped when (row >> 3) & 1 (rollout_mlp.hip's stage with 32 rows);
//   bias   the three hidden layers' biases (N1 + N2 + N3 floats), copied once: no epilogue waits on L2.
// Weights: fragments straight from the images the layer-by-layer forward holds -- layout-GEMM images, for a 512-wide
// layer its two 256-row block images (rslrl_linear_prepare_bimage_wide), for the first layer the image at depth k0 --
// L2-resident, one chunk ahead in registers, no LDS, no new image format.
// Bits: every output carries the bits of the fused training forward (rslrl_linear_gemm / _wide / _ragged per hidden
// layer, RSLRL_LINEAR_FWD_OUT for the last hidden + output layer): the hidden layers issue the six products of
// mfma_x6(x, w) on the C^T tile, chunks in ascending k from zero accumulators (a masked or padded element enters its
// split as an exact zero, as in the ragged and the wide kernels), + b, ELU (elu_neg); the last hidden layer in
// mfma_x6(w, x)'s order; the output layer as the fused output kernel's epilogue at N = 128 computes it: one wave runs a
// whole 64-column group's chain from H3 in LDS -- x6 MFMAs over (j, s2) for more than 4 outputs, fp32 fma chains for up
// to 4 --, then ((g0 + g1) + 0) + 0, the two zero partials of that kernel's empty column groups, + the output bias.
#include <type_traits>

#include "common.h"
#include "mlp_tile.h"
#include "ragged_load.h"
#include "x6_split.h"

namespace rslrl {
namespace {

constexpr int kRsT = 32;                 // rows per tile
constexpr int kRsThreads = 256;          // 4 waves
constexpr int kRsOutMax = 16;            // output width
constexpr int kRsMaxK0 = 256;            // input width
constexpr int kRsRowB = 512 * 4;         // bytes of a row of H
constexpr int kRsHB = kRsT * kRsRowB;    // 64 KiB
constexpr int kRsStChunk = kRsT * 32;    // one chunk of one plane: 1 KiB
constexpr int kRsStPlane = 2 * kRsStChunk;
constexpr int kRsStBuf = 3 * kRsStPlane;  // 6 KiB
constexpr uint32_t kRsRsrcFlags = 0x00020000;

struct RsProblem {
    const float* x;             // [M, k0], rows k0 floats apart
    const uint4* img[3];        // the hidden layers' images
    const float* bias[3];
    const uint4* oimg;          // output layer image (BIMAGE_LAYOUT_OUT)
    const float* obias;         // [nout]
    float* y;                   // [M, nout]
    float* sample;              // [M, nout] standard normals in, actions out (or null)
    const float* sample_scale;  // [nout]
    int k0;
    int nout;
    int x16;                    // rows take 16-byte loads (k0 % 4 == 0, 16-byte aligned base)
};

struct RsArgs {
    RsProblem p[2];
};

__device__ __forceinline__ float rs_elu(float v) {
    const float n = elu_neg(fminf(v, 0.f));
    return v > 0.f ? v : n;
}

// the six products of mfma_x6(x, w) on the C^T tile: MFMA(w_q, x_p) = MFMA(x_p, w_q)^T
__device__ __forceinline__ f32x16 rs_mfma_ct(const bf16x8 (&x)[3], const bf16x8 (&w)[3], f32x16 acc) {
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w[0], x[2], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w[2], x[0], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w[1], x[1], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w[0], x[1], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w[1], x[0], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w[0], x[0], acc, 0, 0, 0);
    return acc;
}

using rs_u32x2 = __attribute__((ext_vector_type(2))) unsigned int;

__device__ __forceinline__ bf16x8 rs_lds_frag(int addr) {
    typedef __attribute__((address_space(3))) bf16x8 lds_b8;
    return *reinterpret_cast<const lds_b8*>(addr);
}

// workgroup barrier for LDS hand-offs only: the weight prefetches in flight stay in flight
__device__ __forceinline__ void rs_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

__device__ __forceinline__ float4 rs_lds_read(int addr) {
    typedef __attribute__((address_space(3))) f32x4 lds_f4;
    const f32x4 v = *reinterpret_cast<const lds_f4*>(addr);
    return make_float4(v[0], v[1], v[2], v[3]);
}

__device__ __forceinline__ void rs_lds_write(int addr, float4 v) {
    typedef __attribute__((address_space(3))) f32x4 lds_f4;
    *reinterpret_cast<lds_f4*>(addr) = f32x4{v.x, v.y, v.z, v.w};
}

template <int N1, int N2, int N3>
constexpr int rs_lds_bytes() {
    return kRsHB + 2 * kRsStBuf + 4 * (N1 + N2 + N3);
}

// One problem's forward over one 32-row tile.
template <int N1, int N2, int N3>
__device__ __forceinline__ void rs_body(const RsProblem& P, char* lds) {
    static_assert(N1 % 128 == 0 && N2 % 128 == 0 && N3 == 128 && N1 <= 512 && N2 <= 256, "hidden widths");
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int h = lane >> 5;
    const int l32 = lane & 31;
    const int s = l32 & 15;  // the H swizzle of this lane's row
    const int64_t row0 = static_cast<int64_t>(blockIdx.x) * kRsT;
    const int hb = static_cast<int>(reinterpret_cast<uintptr_t>(lds));
    const int sb = hb + kRsHB;
    const int bb = sb + 2 * kRsStBuf;  // biases: layer 0 at 0, layer 1 at N1, layer 2 at N1 + N2 (floats)
    const int hrow = hb + l32 * kRsRowB;

    // ---- the biases and the observation tile into LDS.  Thread t: column quad t & 63, rows (t >> 6) + 4 i; the quads
    // from k0 on are zeros up to the next multiple of 32 columns (the stage works on chunk pairs)
    const int k0 = P.k0;
    const int nch0 = (k0 + 15) >> 4;  // 16-deep chunks of the first layer (its image's)
    const int np0 = (nch0 + 1) >> 1;
    {
        typedef __attribute__((address_space(3))) float lds_f;
        for (int i = threadIdx.x; i < N1 + N2 + N3; i += kRsThreads) {
            const float* src = i < N1 ? P.bias[0] + i : (i < N1 + N2 ? P.bias[1] + (i - N1) : P.bias[2] + (i - N1 - N2));
            *reinterpret_cast<lds_f*>(bb + 4 * i) = *src;
        }
        const int qc = threadIdx.x & 63, rg = threadIdx.x >> 6;
        if (qc < 8 * np0) {
            float4 v[8];
            const bool x16 = P.x16 != 0, wide = k0 >= 4;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const float* row = P.x + (row0 + rg + 4 * i) * k0;
                if (x16) {  // k0 % 4 == 0: a quad is whole or absent
                    const bool ok = 4 * qc < k0;
                    const float4 t = *reinterpret_cast<const float4*>(row + (ok ? 4 * qc : 0));
                    v[i] = ok ? t : make_float4(0.f, 0.f, 0.f, 0.f);
                } else {
                    v[i] = load4_ragged_any(row, 4 * qc, k0, wide, true);
                }
            }
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int r = rg + 4 * i;
                rs_lds_write(hb + r * kRsRowB + ((qc ^ (r & 15)) << 4), v[i]);
            }
        }
    }
    __syncthreads();

    // ---- the cooperative split of chunk pair p (columns 32 p .. 32 p + 31 of H) into stage buffer buf
    const int srow = threadIdx.x & 31, sq8 = threadIdx.x >> 5;  // row, quad of the pair (chunk sq8 >> 2, quad sq8 & 3)
    const int s_rd = hb + srow * kRsRowB;
    const int s_wr = sb + (sq8 >> 2) * kRsStChunk + srow * 32 + 16 * (((sq8 >> 1) & 1) ^ ((srow >> 3) & 1)) + 8 * (sq8 & 1);
    auto stage_pair = [&](int p, int buf) {
        typedef __attribute__((address_space(3))) rs_u32x2 lds_u2;
        uint2 w[3];
        split4(rs_lds_read(s_rd + (((8 * p + sq8) ^ (srow & 15)) << 4)), w[0], w[1], w[2]);
#pragma unroll
        for (int q = 0; q < 3; ++q)
            *reinterpret_cast<lds_u2*>(s_wr + buf * kRsStBuf + q * kRsStPlane) = rs_u32x2{w[q].x, w[q].y};
    };
    const int f_rd = sb + l32 * 32 + 16 * (h ^ ((l32 >> 3) & 1));  // fragment (row l32, half h) of a stage plane

    // ---- one hidden layer: NB column blocks per wave over nch chunks of the image (np pairs of H), then + b, ELU into
    // H.  CT: the six products in mfma_x6(x, w)'s order (the hidden-layer kernels), else mfma_x6(w, x)'s (the fused
    // output kernel's last hidden layer).  The image: ceil(4 * 32 NB / 256) blocks of nch chunks.
    auto hidden_layer = [&](auto nb_c, auto ct_c, const uint4* img, int nch, int np, int bias_off) {
        constexpr int NB = decltype(nb_c)::value;
        constexpr bool CT = decltype(ct_c)::value;
        constexpr int kBlocks = NB == 4 ? 2 : 1;
        const int n0 = 32 * NB * wave;  // this wave's first column
        const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc(
            const_cast<uint4*>(img), 0, static_cast<uint32_t>(kBlocks * nch * kX6ChunkB), kRsRsrcFlags);
        // image row n = n0 + 32 j + l32 of block n >> 8, half h (swapped on rows with (n >> 3) & 1 = (l32 >> 3) & 1)
        const int wvoff = (n0 >> 8) * nch * kX6ChunkB + ((n0 & 255) + l32) * kX6RowB + 16 * (h ^ ((l32 >> 3) & 1));
        auto wload = [&](int c, int j, int q) {
            return __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(rw, wvoff + 32 * kX6RowB * j,
                                                                                   c * kX6ChunkB + q * kX6PlaneB, 0));
        };
        f32x16 acc[NB];
        bf16x8 wf[2][NB][3];
#pragma unroll
        for (int j = 0; j < NB; ++j) {
            acc[j] = f32x16{};
#pragma unroll
            for (int q = 0; q < 3; ++q) wf[0][j][q] = wload(0, j, q);  // in flight over the stage's barrier
        }
        stage_pair(0, 0);
        rs_barrier();
        for (int p = 0; p < np; ++p) {
            const int buf = p & 1;
            if (p + 1 < np) stage_pair(p + 1, buf ^ 1);
#pragma unroll
            for (int cc = 0; cc < 2; ++cc) {
                const int c = 2 * p + cc;
                bf16x8 xf[3];
#pragma unroll
                for (int q = 0; q < 3; ++q) xf[q] = rs_lds_frag(f_rd + buf * kRsStBuf + q * kRsStPlane + cc * kRsStChunk);
                const int cn = c + 1 < nch ? c + 1 : nch - 1;  // (past the last chunk: a reload nobody uses)
#pragma unroll
                for (int j = 0; j < NB; ++j)
#pragma unroll
                    for (int q = 0; q < 3; ++q) wf[cc ^ 1][j][q] = wload(cn, j, q);
                if (c < nch) {  // (an odd chunk count: the pair's second half is padding)
#pragma unroll
                    for (int j = 0; j < NB; ++j)
                        acc[j] = CT ? rs_mfma_ct(xf, wf[cc][j], acc[j]) : mfma_x6(wf[cc][j], xf, acc[j]);
                }
            }
            rs_barrier();  // pair p + 1 staged; buffer buf free again; after the last pair: H free for the epilogue
        }
#pragma unroll
        for (int j = 0; j < NB; ++j)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int col = n0 + 32 * j + 8 * g + 4 * h;
                const float4 b4 = rs_lds_read(bb + 4 * (bias_off + col));
                float4 v;
                v.x = rs_elu(acc[j][4 * g + 0] + b4.x);
                v.y = rs_elu(acc[j][4 * g + 1] + b4.y);
                v.z = rs_elu(acc[j][4 * g + 2] + b4.z);
                v.w = rs_elu(acc[j][4 * g + 3] + b4.w);
                rs_lds_write(hrow + (((col >> 2) ^ s) << 4), v);
            }
        rs_barrier();
    };
    using std::integral_constant;
    hidden_layer(integral_constant<int, N1 / 128>{}, integral_constant<bool, true>{}, P.img[0], nch0, np0, 0);
    hidden_layer(integral_constant<int, N2 / 128>{}, integral_constant<bool, true>{}, P.img[1], N1 / 16, N1 / 32, N1);
    hidden_layer(integral_constant<int, N3 / 128>{}, integral_constant<bool, false>{}, P.img[2], N2 / 16, N2 / 32,
                 N1 + N2);

    // ---- the output layer over H3 (128 columns, in H): wave g < 2 runs the whole chain of the 64-column group g (the
    // fused output kernel's wave column wn = g) for its 32 rows: mlp_gemm_x6.h kEpiBiasEluOut, NR 4 / NR 1.
    // red (the stage area): [g][o][32 rows]
    const int nout = P.nout;
    float* red = reinterpret_cast<float*>(lds + kRsHB);
    if (wave < 2) {
        const uint4* oimg = P.oimg + wave * (2 * 2 * 3 * 64);
        const float4* owf =
            reinterpret_cast<const float4*>(P.oimg + kOutImagePlaneUnits) + 2 * (wave * 2 * 2 * 2 * 32 + h * 32);
        static_assert(out_image_f32_pair(1, 0, 0, 1, 0) == 2 * 2 * 2 * 32 + 32, "out-image fp32 section");
        f32x16 oacc = f32x16{};
        float oval[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2) {
                // the lane's 8 columns of k step s2: 64 g + 32 j + 16 s2 + 4 h + {0..3, 8..11}
                const int u = 16 * wave + 8 * j + 4 * s2 + h;
                const float4 lo4 = rs_lds_read(hrow + ((u ^ s) << 4));
                const float4 hi4 = rs_lds_read(hrow + (((u + 2) ^ s) << 4));
                if (nout <= 4) {
                    const float v[8] = {lo4.x, lo4.y, lo4.z, lo4.w, hi4.x, hi4.y, hi4.z, hi4.w};
#pragma unroll
                    for (int o = 0; o < 4; ++o) {
                        if (o >= nout) break;
                        const float4* q = owf + 2 * ((j * 2 + s2) * 2 * 32 + o);
                        const float4 w0 = q[0], w1 = q[1];
                        const float w[8] = {w0.x, w0.y, w0.z, w0.w, w1.x, w1.y, w1.z, w1.w};
#pragma unroll
                        for (int t = 0; t < 8; ++t) oval[o] = fmaf(v[t], w[t], oval[o]);
                    }
                } else {
                    uint2 lo[3], hi[3];
                    split4(lo4, lo[0], lo[1], lo[2]);
                    split4(hi4, hi[0], hi[1], hi[2]);
                    bf16x8 vb[3], wa[3];
#pragma unroll
                    for (int q = 0; q < 3; ++q) {
                        vb[q] = __builtin_bit_cast(bf16x8, make_uint4(lo[q].x, lo[q].y, hi[q].x, hi[q].y));
                        wa[q] = __builtin_bit_cast(bf16x8, oimg[((j * 2 + s2) * 3 + q) * 64 + lane]);
                    }
                    oacc = mfma_x6(wa, vb, oacc);
                }
            }
        float* rd_out = red + wave * kRsOutMax * 32;
        if (nout <= 4) {  // the two lane halves hold different columns of the same row
#pragma unroll
            for (int o = 0; o < 4; ++o) {
                const float t = oval[o] + __shfl_xor(oval[o], 32, 64);
                if (h == 0 && o < nout) rd_out[o * 32 + l32] = t;
            }
        } else {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int o = (r & 3) + 8 * (r >> 2) + 4 * h;
                if (o < nout) rd_out[o * 32 + l32] = oacc[r];
            }
        }
    }
    // this thread's output elements: their bias and the sample's normal and scale are loaded before the barrier
    constexpr int kPer = kRsT * kRsOutMax / kRsThreads;
    float ob[kPer], se[kPer], ss[kPer];
#pragma unroll
    for (int k = 0; k < kPer; ++k) {
        const int idx = threadIdx.x + k * kRsThreads;
        ob[k] = se[k] = ss[k] = 0.f;
        if (idx < kRsT * nout) {
            const int rl = idx & (kRsT - 1), o = idx / kRsT;
            ob[k] = P.obias[o];
            if (P.sample) {
                se[k] = P.sample[(row0 + rl) * nout + o];
                ss[k] = P.sample_scale[o];
            }
        }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kPer; ++k) {
        const int idx = threadIdx.x + k * kRsThreads;
        if (idx >= kRsT * nout) break;
        const int rl = idx & (kRsT - 1), o = idx / kRsT;
        const float* b = red + o * 32 + rl;
        // the fused output kernel adds its four column groups' partials in order; at N = 128 the last two are +0
        const float sum = ((b[0] + b[kRsOutMax * 32]) + 0.f) + 0.f;
        const float mu = sum + ob[k];
        const int64_t e = (row0 + rl) * nout + o;
        P.y[e] = mu;
        if (P.sample)  // the Normal sample (rslrl_normal_affine's expression): eps * sigma, then + mu
            P.sample[e] = __fadd_rn(__fmul_rn(se[k], ss[k]), mu);
    }
}

template <int N1, int N2, int N3>
__global__ __launch_bounds__(kRsThreads, 2) void rollout_mlp_shaped_kernel(RsArgs a) {
    __shared__ __attribute__((aligned(16))) char lds[rs_lds_bytes<N1, N2, N3>()];
    rs_body<N1, N2, N3>(a.p[blockIdx.y], lds);
}

template <int N1, int N2, int N3>
void rs_launch(const RsArgs& a, int64_t M, int problems, hipStream_t st) {
    const dim3 g(static_cast<unsigned>(M / kRsT), static_cast<unsigned>(problems)), b(kRsThreads);
    hipLaunchKernelGGL((rollout_mlp_shaped_kernel<N1, N2, N3>), g, b, 0, st, a);
}

bool rs_aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

}  // namespace
}  // namespace rslrl

using namespace rslrl;

extern "C" int rslrl_rollout_mlp_shaped_pair(const rslrl_rollout_mlp_shaped_t* a0, const rslrl_rollout_mlp_shaped_t* a1,
                                             int64_t M, rslrl_stream_t stream) {
    if (!a0 || M < 0) return RSLRL_E_INVALID_ARGUMENT;
    if (M == 0) return RSLRL_OK;
    const int problems = a1 ? 2 : 1;
    const rslrl_rollout_mlp_shaped_t* in[2] = {a0, a1};
    const int n1 = a0->width[0], n2 = a0->width[1], n3 = a0->width[2];
    if (a1 && (a1->width[0] != n1 || a1->width[1] != n2 || a1->width[2] != n3)) return RSLRL_E_UNSUPPORTED;
    const bool listed = n3 == 128 && ((n1 == 512 && n2 == 256) || (n1 == 256 && n2 == 256) || (n1 == 256 && n2 == 128) ||
                                      (n1 == 128 && n2 == 128));
    if (!listed || M % kRsT || M / kRsT > INT32_MAX) return RSLRL_E_UNSUPPORTED;
    RsArgs args{};
    for (int i = 0; i < problems; ++i) {
        const rslrl_rollout_mlp_shaped_t& s = *in[i];
        if (s.k0 < 1 || s.k0 > kRsMaxK0 || s.nout < 1 || s.nout > kRsOutMax) return RSLRL_E_UNSUPPORTED;
    }
    for (int i = 0; i < problems; ++i) {
        const rslrl_rollout_mlp_shaped_t& s = *in[i];
        if (!s.x || !s.out_image || !s.out_bias || !s.y) return RSLRL_E_INVALID_ARGUMENT;
        if (s.sample && !s.sample_scale) return RSLRL_E_INVALID_ARGUMENT;
        if (!rs_aligned(s.x, 4) || !rs_aligned(s.out_image, 16) || !rs_aligned(s.y, 4) || !rs_aligned(s.out_bias, 4) ||
            (s.sample && (!rs_aligned(s.sample, 4) || !rs_aligned(s.sample_scale, 4))))
            return RSLRL_E_MISALIGNED;
        RsProblem& p = args.p[i];
        for (int l = 0; l < 3; ++l) {
            if (!s.bimage[l] || !s.bias[l]) return RSLRL_E_INVALID_ARGUMENT;
            if (!rs_aligned(s.bimage[l], 16) || !rs_aligned(s.bias[l], 4)) return RSLRL_E_MISALIGNED;
            p.img[l] = static_cast<const uint4*>(s.bimage[l]);
            p.bias[l] = s.bias[l];
        }
        p.x = s.x;
        p.oimg = static_cast<const uint4*>(s.out_image);
        p.obias = s.out_bias;
        p.y = s.y;
        p.sample = s.sample;
        p.sample_scale = s.sample_scale;
        p.k0 = s.k0;
        p.nout = s.nout;
        p.x16 = s.k0 % 4 == 0 && rs_aligned(s.x, 16);
    }
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (n1 == 512) rs_launch<512, 256, 128>(args, M, problems, st);
    else if (n1 == 256 && n2 == 256) rs_launch<256, 256, 128>(args, M, problems, st);
    else if (n1 == 256) rs_launch<256, 128, 128>(args, M, problems, st);
    else rs_launch<128, 128, 128>(args, M, problems, st);
    return launch_status();
}
