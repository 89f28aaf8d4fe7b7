// ---- Output-layer backward on the VALU (RSLRL_LINEAR_DGRAD_ELU_WGRAD; x6 image of W^T as input).  With a
// 4-16 wide reduction this op is a stream over H (read) and dZ_prev (written) with ~24 FMAs per element: MFMA
// tiles buy nothing here and their epilogue needed 256 registers (one workgroup per CU, hundreds of bytes of
// scratch per lane).  Per 128-row tile (workgroup of 4 waves, 32 rows each; lane l owns columns 4l..4l+3):
//   z[c] = sum_o dZ[row][o] W[o][c] (fp32 FMA chain, o ascending; W rebuilt exactly from the image's three
//   bf16 planes), dZ_prev = z * ELU'(H), column sums of dZ_prev, dW[o][c] += dZ[row][o] H[row][c], and
//   db_out[o] = sum of dZ[row][o] -- the same per-tile partial layouts as the MFMA kernel (tile-major).
// dZ rows are wave-uniform (scalar loads); four rows of H are in flight per wave.
#include <type_traits>

#include "common.h"
#include "amax.h"
#include "mlp_gemm.h"
#include "x6_split.h"

namespace rslrl {
namespace {

constexpr int kOutBwdThreads = 256;

// per-tile partial row of the output-layer backward: dW [Nred][N], db [Nred], zero pad to a multiple of 4 floats
__host__ __device__ inline int64_t dgrad_wgrad_tile_floats(int nred, int n) {
    return (static_cast<int64_t>(nred) * n + nred + 3) / 4 * 4;
}

// CPL columns per lane (4: a wave spans a 256-column row; 2: two waves share a row, so W and the dW
// accumulators take 2 NR registers each instead of 4 NR -- NR >= 12 needed 178+ registers at CPL 4)
// LDS of one out_bwd body: red [RG][NR + 1][kBN] floats (per-row-group dW rows, then column sums), dzt4 [kBM][NR / 4]
// float4s (the tile's dZ rows), dzsum [RG][NR] floats
template <int NR, int CPL>
struct OutBwdLds {
    static constexpr int WPR = kBN / (kWave * CPL);          // waves per row
    static constexpr int RG = (kOutBwdThreads / kWave) / WPR;  // row groups per workgroup
    static constexpr int kRed = RG * (NR + 1) * kBN * 4;
    static constexpr int kDzt = kBM * (NR / 4) * 16;
    static constexpr int kBytes = kRed + kDzt + RG * NR * 4;
};

template <int NR, int CPL>
__device__ __forceinline__ void out_bwd_valu_body(const GemmParams& p, const uint4* __restrict__ bimg, char* smem) {
    using LD = OutBwdLds<NR, CPL>;
    constexpr int WPR = LD::WPR;
    constexpr int RG = LD::RG;
    constexpr int RPW = kBM / RG;                      // rows per wave
    using vec = typename std::conditional<CPL == 4, f32x4, f32x2>::type;
    auto red = reinterpret_cast<float (*)[NR + 1][kBN]>(smem);
    auto dzt4 = reinterpret_cast<float4 (*)[NR / 4]>(smem + LD::kRed);
    auto dzsum = reinterpret_cast<float (*)[NR]>(smem + LD::kRed + LD::kDzt);
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int rg = wave / WPR;
    const int c0 = CPL * (lane + kWave * (wave % WPR));
    const bool col_ok = c0 < p.N;  // N % 4 == 0
    // W[o][c0 + e] from the image of W^T: chunk 0, row n = c0 + e, k = o; 16-byte half ph holds k = 8 lh + j
    float w[NR][CPL];
#pragma unroll
    for (int e = 0; e < CPL; ++e) {
        const int n = c0 + e;
#pragma unroll
        for (int lh = 0; lh < (NR + 7) / 8; ++lh) {
            const int ph = lh ^ ((n >> 3) & 1);
            uint4 q[3];
#pragma unroll
            for (int pl = 0; pl < 3; ++pl)
                q[pl] = col_ok ? bimg[(pl * kX6PlaneB + n * kX6RowB + 16 * ph) / 16] : make_uint4(0, 0, 0, 0);
            const uint32_t* u0 = reinterpret_cast<const uint32_t*>(&q[0]);
            const uint32_t* u1 = reinterpret_cast<const uint32_t*>(&q[1]);
            const uint32_t* u2 = reinterpret_cast<const uint32_t*>(&q[2]);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int o = 8 * lh + j;
                if (o >= NR) break;
                auto f = [j](const uint32_t* u) {
                    const uint32_t x = u[j >> 1];
                    return __uint_as_float((j & 1) ? (x & 0xffff0000u) : (x << 16));
                };
                w[o][e] = (f(u0) + f(u1)) + f(u2);  // exact: the planes were split from this fp32 value
            }
        }
    }
    float wacc[NR][CPL], cs[CPL], dzs[NR];
#pragma unroll
    for (int e = 0; e < CPL; ++e) cs[e] = 0.f;
#pragma unroll
    for (int o = 0; o < NR; ++o) {
        dzs[o] = 0.f;
#pragma unroll
        for (int e = 0; e < CPL; ++e) wacc[o][e] = 0.f;
    }
    float amx = 0.f;
    // the tile's dZ rows (128 x NR floats) staged once in LDS: a per-row uniform global load is a vector load
    // the waves would wait on (the compiler cannot prove dZ read-only for the scalar cache)
    // (p.K = Nred, the row stride of dZ: NR = Nred rounded up to 4, the missing rows staged as zeros -- a 1-wide
    // value head reads its [M, 1] gradient as it is, no zero-padded copy)
    {
        const int64_t t0 = static_cast<int64_t>(blockIdx.x) * kBM;
        if (p.K == NR) {
            for (int i = threadIdx.x; i < kBM * NR / 4; i += kOutBwdThreads) {
                const int r = i / (NR / 4), q = i % (NR / 4);
                dzt4[r][q] = t0 + r < p.M ? *reinterpret_cast<const float4*>(p.a + (t0 + r) * p.K + 4 * q)
                                          : make_float4(0.f, 0.f, 0.f, 0.f);
            }
        } else {
            float* dzt = reinterpret_cast<float*>(dzt4);
            for (int i = threadIdx.x; i < kBM * NR; i += kOutBwdThreads) {
                const int r = i / NR, o = i % NR;
                dzt[i] = (t0 + r < p.M && o < p.K) ? p.a[(t0 + r) * p.K + o] : 0.f;
            }
        }
        __syncthreads();
    }
    const int64_t row0 = static_cast<int64_t>(blockIdx.x) * kBM + rg * RPW;
    const int64_t rows = p.M - row0 < RPW ? (p.M - row0 > 0 ? p.M - row0 : 0) : RPW;
#ifndef RSLRL_OUTBWD_U
#define RSLRL_OUTBWD_U 4  // (8: 188.4 us, 16: 223 us, 4: 185.5 us -- the actor's 393,216 rows, scripts/outbwd_u_ab.sh)
#endif
    constexpr int U = RSLRL_OUTBWD_U;  // rows of H in flight per wave
    for (int r0 = 0; r0 < rows; r0 += U) {
        vec hv[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t row = row0 + (r0 + u < rows ? r0 + u : rows - 1);
            hv[u] = col_ok ? *reinterpret_cast<const vec*>(p.h + row * p.N + c0) : vec{};
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (r0 + u >= rows) break;  // wave-uniform
            const int64_t row = row0 + r0 + u;
            float d[NR];
#pragma unroll
            for (int o4 = 0; o4 < NR / 4; ++o4) {  // LDS broadcast (every lane reads the same 16 bytes)
                const float4 t = dzt4[rg * RPW + r0 + u][o4];
                d[4 * o4] = t.x;
                d[4 * o4 + 1] = t.y;
                d[4 * o4 + 2] = t.z;
                d[4 * o4 + 3] = t.w;
            }
            vec out;
#pragma unroll
            for (int e = 0; e < CPL; ++e) {
                const float hh = hv[u][e];
                float z = 0.f;
#pragma unroll
                for (int o = 0; o < NR; ++o) z = fmaf(d[o], w[o][e], z);
                const float v = hh > 0.f ? z : z * (hh + 1.f);  // ELU'(x) = 1 if h > 0 else h + 1
                out[e] = v;
                cs[e] += v;
                amx = fmaxf(amx, fabsf(v));
#pragma unroll
                for (int o = 0; o < NR; ++o) wacc[o][e] = fmaf(d[o], hh, wacc[o][e]);
            }
            if (wave % WPR == 0)
#pragma unroll
                for (int o = 0; o < NR; ++o) dzs[o] += d[o];
            if (col_ok) __builtin_nontemporal_store(out, reinterpret_cast<vec*>(p.c + row * p.N + c0));
        }
    }
    // per-tile partials, the row groups added in order
#pragma unroll
    for (int o = 0; o <= NR; ++o)
#pragma unroll
        for (int e = 0; e < CPL; ++e) red[rg][o][c0 + e] = o < NR ? wacc[o][e] : cs[e];
    if (lane == 0 && wave % WPR == 0)
#pragma unroll
        for (int o = 0; o < NR; ++o) dzsum[rg][o] = dzs[o];
    __syncthreads();
    const int nred = p.K;
    const int64_t tile_floats = dgrad_wgrad_tile_floats(nred, p.N);
    float* wp = p.wpart + static_cast<int64_t>(blockIdx.x) * tile_floats;
    for (int idx = threadIdx.x; idx < (NR + 1) * kBN; idx += kOutBwdThreads) {
        const int o = idx / kBN, c = idx % kBN;
        if (c >= p.N) continue;
        float v = red[0][o][c];
#pragma unroll
        for (int g = 1; g < RG; ++g) v += red[g][o][c];
        if (o < nred) wp[static_cast<int64_t>(o) * p.N + c] = v;
        else if (o == NR && p.colsum) p.colsum[static_cast<int64_t>(blockIdx.x) * p.N + c] = v;
    }
    if (threadIdx.x < nred) {
        float v = dzsum[0][threadIdx.x];
#pragma unroll
        for (int g = 1; g < RG; ++g) v += dzsum[g][threadIdx.x];
        wp[static_cast<int64_t>(nred) * p.N + threadIdx.x] = v;
    }
    // the row's pad to a 16-byte multiple (the fold reads float4 columns): zeros
    const int pad = static_cast<int>(tile_floats - (static_cast<int64_t>(nred) * p.N + nred));
    if (threadIdx.x < pad) wp[static_cast<int64_t>(nred) * p.N + nred + threadIdx.x] = 0.f;
    amax_publish<kOutBwdThreads>(p.amax_out, p.amax_ws, amx);
}

template <int NR, int CPL>
__global__ __launch_bounds__(kOutBwdThreads, NR >= 16 ? 3 : 4) void out_bwd_valu_kernel(GemmParams p, const uint4* __restrict__ bimg) {
    __shared__ __attribute__((aligned(16))) char smem[OutBwdLds<NR, CPL>::kBytes];
    out_bwd_valu_body<NR, CPL>(p, bimg, smem);
}

// The actor's and the critic's output-layer backward in one launch (blockIdx.y; e.g. Nred 12 and 1), one body each
// over one LDS area: at 98,304 rows each fills three quarters of the workgroup slots.
template <int NR0, int CPL0, int NR1, int CPL1>
__global__ __launch_bounds__(kOutBwdThreads, 4) void out_bwd_valu_pair_kernel(GemmPair b) {
    constexpr int kBytes = OutBwdLds<NR0, CPL0>::kBytes > OutBwdLds<NR1, CPL1>::kBytes ? OutBwdLds<NR0, CPL0>::kBytes
                                                                                       : OutBwdLds<NR1, CPL1>::kBytes;
    __shared__ __attribute__((aligned(16))) char smem[kBytes];
    if (blockIdx.y == 0) {
        asm volatile("; out bwd pair: problem 0" ::: "memory");
        out_bwd_valu_body<NR0, CPL0>(b.p[0], b.img[0], smem);
    } else {
        asm volatile("; out bwd pair: problem 1" ::: "memory");
        out_bwd_valu_body<NR1, CPL1>(b.p[1], b.img[1], smem);
    }
}

template <int NR0, int NR1>
void launch_out_bwd_pair(const GemmPair& b, dim3 g, hipStream_t st) {
    constexpr int C0 = NR0 <= 4 ? 4 : 2, C1 = NR1 <= 4 ? 4 : 2;
    hipLaunchKernelGGL((out_bwd_valu_pair_kernel<NR0, C0, NR1, C1>), g, dim3(kOutBwdThreads), 0, st, b);
}

}  // namespace

void out_bwd_valu_launch(const GemmParams& p, const uint4* img, dim3 g, hipStream_t st) {
    auto go = [&](auto nr) {
        constexpr int NR = decltype(nr)::value;
        constexpr int CPL = NR <= 4 ? 4 : 2;
        hipLaunchKernelGGL((out_bwd_valu_kernel<NR, CPL>), g, dim3(kOutBwdThreads), 0, st, p, img);
    };
    switch ((p.K + 3) / 4 * 4) {  // Nred 1..16; a partial last group of 4 is staged with zeros
        case 4: go(std::integral_constant<int, 4>{}); break;
        case 8: go(std::integral_constant<int, 8>{}); break;
        case 12: go(std::integral_constant<int, 12>{}); break;
        default: go(std::integral_constant<int, 16>{}); break;
    }
}

// (one of the two reductions <= 4 wide -- the value head -- the other any of 4 / 8 / 12 / 16)
bool out_bwd_pair_dispatch(const GemmPair& b, int nr0, int nr1, dim3 g, hipStream_t st) {
    auto other = [&](int nr, auto small_first) {
        constexpr bool F = decltype(small_first)::value;
        switch (nr) {
            case 4: launch_out_bwd_pair<4, 4>(b, g, st); return true;
            case 8: F ? launch_out_bwd_pair<4, 8>(b, g, st) : launch_out_bwd_pair<8, 4>(b, g, st); return true;
            case 12: F ? launch_out_bwd_pair<4, 12>(b, g, st) : launch_out_bwd_pair<12, 4>(b, g, st); return true;
            case 16: F ? launch_out_bwd_pair<4, 16>(b, g, st) : launch_out_bwd_pair<16, 4>(b, g, st); return true;
            default: return false;
        }
    };
    if (nr1 == 4) return other(nr0, std::false_type{});
    if (nr0 == 4) return other(nr1, std::true_type{});
    return false;
}

}  // namespace rslrl
