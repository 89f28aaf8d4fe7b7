// Device templates of the split-K weight-gradient GEMM on the x6 / h3 MFMA path, shared by the units that instantiate
// kernels from them: mlp_wgrad.hip (layers up to 256 x 256, described there) and mlp_wide.hip (the 256 x 256 blocks of
// a wider layer's weight gradient).  Everything here is inlined into those kernels; each unit gets its own copy.
#pragma once

#include <algorithm>
#include <type_traits>

#include "common.h"
#include "x6_split.h"
#ifdef RSLRL_WGRAD_RAGGED
#include "ragged_load.h"
#endif

namespace rslrl {
namespace {

constexpr int kThreadsW = 512;
constexpr int kMC = 16;  // rows of m per chunk (one MFMA k step)
constexpr int kTK = 256;
#ifndef RSLRL_WGRAD_DEPTH
#define RSLRL_WGRAD_DEPTH 2
#endif
constexpr int kWgradDepth = RSLRL_WGRAD_DEPTH;  // chunks of look-ahead in registers (full tiles): 2 or 4

using s16x4 = __attribute__((ext_vector_type(4))) short;

struct WgradParams {
    const float* dz;  // [M, N]
    const float* x;   // [M, K]
    float* part;      // [S, N, K]
    int64_t M;
    int64_t rows_per;  // multiple of kMC
    int N;
    int K;
    const float* dz_amax;  // h3 (PL = 2): max |dz|, max |x| -> the operands' power-of-two scales
    const float* x_amax;
};

// One TN x 256 block of a wider layer's weight gradient (mlp_wide.hip): dz and x point at the block's first columns,
// part at the block's first element of slice 0, N and K are the block's widths.  A struct of its own: the dense
// kernels keep WgradParams as their kernel argument.
struct WideWgradParams : WgradParams {
    int ldz;               // row stride of dz (the layer's N)
    int ldx;               // row stride of x and of a partial's dW rows (the layer's K)
    int64_t slice_floats;  // floats per slice of part: the layer's N * K + column sums
    float* cs;             // slice 0's column sums of this block, or nullptr (another block of the same columns writes them)
};

// Strides and destinations of a problem: a dense one's follow from its N and K.  A unit that defines RSLRL_WGRAD_WIDE
// before it includes this header (mlp_wide.hip) instantiates the same device code on WideWgradParams.  (The
// preprocessor and not a template parameter: the dense unit then compiles the token stream it always did, and its
// kernels stay instruction for instruction what they were.)
// A block whose dz (RAG 1) or x (RAG 2) rows have a stride that is no multiple of 4 floats (mlp_ragged.hip, which
// defines RSLRL_WGRAD_RAGGED beside RSLRL_WGRAD_WIDE): back = columns of the same rows in front of the block.
struct RaggedWgradParams : WideWgradParams {
    int back;
};

#ifdef RSLRL_WGRAD_RAGGED
#define RSLRL_WGRAD_BACK(p) (p).back
#else
#define RSLRL_WGRAD_BACK(p) 0
#endif
#if defined(RSLRL_WGRAD_RAGGED)
using WgradP = RaggedWgradParams;
#elif defined(RSLRL_WGRAD_WIDE)
using WgradP = WideWgradParams;
#endif
#ifdef RSLRL_WGRAD_WIDE
#define RSLRL_WGRAD_LDZ(p) (p).ldz
#define RSLRL_WGRAD_LDX(p) (p).ldx
#define RSLRL_WGRAD_SLICE_FLOATS(p, E) (p).slice_floats
#define RSLRL_WGRAD_AND_CS(p) && (p).cs != nullptr
#define RSLRL_WGRAD_CS_DST(p, out) ((p).cs + static_cast<int64_t>(blockIdx.x) * (p).slice_floats)
#else
using WgradP = WgradParams;
#define RSLRL_WGRAD_LDZ(p) (p).N
#define RSLRL_WGRAD_LDX(p) (p).K
#define RSLRL_WGRAD_SLICE_FLOATS(p, E) (static_cast<int64_t>((p).N) * (p).K + (E))
#define RSLRL_WGRAD_AND_CS(p)
#define RSLRL_WGRAD_CS_DST(p, out) ((out) + static_cast<int64_t>((p).N) * (p).K)
#endif

template <int COLS>
__device__ __forceinline__ int swz(int m, int col) {  // byte offset of (m, col), col % 4 == 0, within a plane
    constexpr int rowb = COLS * 2;
    if constexpr (rowb >= 512) return rowb * m + 16 * ((col >> 3) ^ (4 * (m & 3))) + 8 * ((col >> 2) & 1);
    if constexpr (rowb == 128) return rowb * m + 16 * ((col >> 3) ^ (4 * ((m >> 1) & 1))) + 8 * ((col >> 2) & 1);
    return rowb * m + 2 * col;
}

// stage one operand chunk: rows m0.. m0+15 (global rows < m_end valid), columns < ncols valid
// MASKC (full tiles whose operand has fewer than COLS columns, e.g. the first layer's 48 inputs on 64-row tiles):
// columns >= ncols load a clamped in-row address unconditionally and are zeroed by a select, so the load stream
// keeps no control flow (the look-ahead's waitcnt counting needs that)
// RAGGED (mlp_ragged.hip): ld is no multiple of 4 -- rows at 4-byte-aligned bases, the row's last quad masked element
// by element (ragged_load.h); back: columns of the same rows in front of src.  FULL needs ncols + back >= 4.
template <int COLS, bool FULL, bool MASKC = false, bool RAGGED = false>
__device__ __forceinline__ void load_tile(const float* __restrict__ src, int ld, int64_t m0, int64_t m_end,
                                          int ncols, float4 (&v)[(kMC * COLS / 4 + kThreadsW - 1) / kThreadsW],
                                          int back = 0) {
    constexpr int units = kMC * COLS / 4;
    constexpr int per = (units + kThreadsW - 1) / kThreadsW;
#pragma unroll
    for (int i = 0; i < per; ++i) {
        const int u = threadIdx.x + kThreadsW * i;
        const int m = u / (COLS / 4);
        const int c = 4 * (u % (COLS / 4));
        const int64_t row = m0 + m;
#ifdef RSLRL_WGRAD_RAGGED
        if constexpr (RAGGED) {
            // a unit past the chunk or a row past the slice reads row m0 (it exists) and is zeroed
            const bool row_ok = (units % kThreadsW == 0 || u < units) && (FULL || row < m_end);
            const float* rp = src + (row_ok ? row : m0) * ld;
            if constexpr (FULL) v[i] = load4_ragged(rp, c, ncols, row_ok);
            else v[i] = load4_ragged_any(rp, c, ncols, ncols + back >= 4, row_ok);
            continue;
        }
#endif
        if constexpr (FULL && MASKC) {
            const bool ok = c < ncols;
            const float4 t = *reinterpret_cast<const float4*>(src + row * ld + (ok ? c : 0));
            v[i] = ((units % kThreadsW == 0 || u < units) && ok) ? t : make_float4(0.f, 0.f, 0.f, 0.f);
        } else if constexpr (FULL) {
            v[i] = (units % kThreadsW == 0 || u < units)
                       ? *reinterpret_cast<const float4*>(src + row * ld + c) : make_float4(0.f, 0.f, 0.f, 0.f);
        } else {
            const bool ok = (units % kThreadsW == 0 || u < units) && row < m_end && c < ncols;
            const float4 t = *reinterpret_cast<const float4*>(src + (ok ? row * ld + c : 0));
            v[i] = ok ? t : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    }
}

template <int COLS, int PL>
__device__ __forceinline__ void store_tile(const float4 (&v)[(kMC * COLS / 4 + kThreadsW - 1) / kThreadsW],
                                           char* __restrict__ img, float sc) {
    constexpr int units = kMC * COLS / 4;
    constexpr int per = (units + kThreadsW - 1) / kThreadsW;
    constexpr int plane = kMC * COLS * 2;
#pragma unroll
    for (int i = 0; i < per; ++i) {
        const int u = threadIdx.x + kThreadsW * i;
        if (units % kThreadsW == 0 || u < units) {
            const int m = u / (COLS / 4);
            const int c = 4 * (u % (COLS / 4));
            uint2 w[PL];
            float4 x = v[i];
            if constexpr (PL == 2) x = make_float4(x.x * sc, x.y * sc, x.z * sc, x.w * sc);
            Arith<PL>::split(x, w);
            const int off = swz<COLS>(m, c);
#pragma unroll
            for (int q = 0; q < PL; ++q) *reinterpret_cast<uint2*>(img + q * plane + off) = w[q];
        }
    }
}

// 32x32x16 operand fragment of columns [cb, cb + 32) (all 16 rows) of one plane, via two transposed reads
template <int COLS, typename F = bf16x8>
__device__ __forceinline__ F read_frag_tr(const char* __restrict__ plane, int cb) {
    const int lane = threadIdx.x & 63;
    const int g = lane >> 4;
    const int q = (lane >> 2) & 3;
    const int p = lane & 3;
    const int col = cb + 16 * (g & 1) + 4 * p;
    const int m = 8 * (g >> 1) + q;
    typedef __attribute__((address_space(3))) s16x4 lds_s16x4;
    const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(plane + swz<COLS>(m, col)));
    const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(plane + swz<COLS>(m + 4, col)));
    const __attribute__((ext_vector_type(8))) short v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    return __builtin_bit_cast(F, v);
}

// TN = rows of dW per workgroup (256: waves 2 (n) x 4 (k), wave tile 128 x 64; 64: waves 2 x 4, 32 x 64;
// 32: waves 1 x 8, 32 x 32)
// CS: also the column sums of one operand -- the bias gradient of the layer (1: of dz, the TN-row side, TN = 256;
// 2: of x, the 256-column side) -- accumulated in fp32 from the staged registers (every thread's float4 units
// share their 4 columns), folded over the 8 threads of a column quad through LDS in a fixed order and written
// after the tile as the slice's extra partial row: part[s] = [dW (N x K) | colsum (N or K)].
// RAG (mlp_ragged.hip): 1 = the dz operand's, 2 = the x operand's row stride is no multiple of 4
template <int TN, bool FULL, int PL = 3, bool MASKN = false, int CS = 0, int RAG = 0>
__device__ __forceinline__ void wgrad_x6_body(const WgradP& p) {
    static_assert(CS != 1 || TN == kTK, "column sums of the dz side need 256-row tiles");
    using Frag = typename Arith<PL>::frag;
    constexpr int WN = TN == 32 ? 1 : 2;
    constexpr int WK = 8 / WN;
    constexpr int I = TN / WN / 32;
    constexpr int J = kTK / WK / 32;
    constexpr int planeA = kMC * TN * 2;
    constexpr int planeB = kMC * kTK * 2;
    constexpr int bufBytes = PL * planeA + PL * planeB;
    constexpr int perA = (kMC * TN / 4 + kThreadsW - 1) / kThreadsW;
    constexpr int perB = (kMC * kTK / 4 + kThreadsW - 1) / kThreadsW;
    __shared__ __attribute__((aligned(16))) char lds[2][bufBytes];

    const int wave = threadIdx.x >> 6;
    const int wn = wave / WK;
    const int wk = wave % WK;
    const int64_t m_begin = static_cast<int64_t>(blockIdx.x) * p.rows_per;
    const int64_t m_end = m_begin + p.rows_per < p.M ? m_begin + p.rows_per : p.M;
    const int nchunks = static_cast<int>((m_end - m_begin + kMC - 1) / kMC);
    const float sa = PL == 2 ? h3_scale(*p.dz_amax) : 1.f;
    const float sb = PL == 2 ? h3_scale(*p.x_amax) : 1.f;

    f32x16 acc[I][J];
#pragma unroll
    for (int i = 0; i < I; ++i)
#pragma unroll
        for (int j = 0; j < J; ++j) acc[i][j] = f32x16{};
    float4 csum = make_float4(0.f, 0.f, 0.f, 0.f);  // CS: this thread's 4 columns
    // sum the staged chunk of the CS operand (raw values, before any h3 scaling)
    auto accum_a = [&](const float4 (&v)[perA]) {
        if constexpr (CS == 1) {
#pragma unroll
            for (int i = 0; i < perA; ++i) { csum.x += v[i].x; csum.y += v[i].y; csum.z += v[i].z; csum.w += v[i].w; }
        }
    };
    auto accum_b = [&](const float4 (&v)[perB]) {
        if constexpr (CS == 2) {
#pragma unroll
            for (int i = 0; i < perB; ++i) { csum.x += v[i].x; csum.y += v[i].y; csum.z += v[i].z; csum.w += v[i].w; }
        }
    };

    auto compute = [&](const char* a_img) {
        const char* b_img = a_img + PL * planeA;
        Frag bf[J][PL];
#pragma unroll
        for (int j = 0; j < J; ++j)
#pragma unroll
            for (int q = 0; q < PL; ++q) bf[j][q] = read_frag_tr<kTK, Frag>(b_img + q * planeB, wk * (J * 32) + j * 32);
#pragma unroll
        for (int i = 0; i < I; ++i) {
            Frag af[PL];
#pragma unroll
            for (int q = 0; q < PL; ++q) af[q] = read_frag_tr<TN, Frag>(a_img + q * planeA, wn * (I * 32) + i * 32);
#pragma unroll
            for (int j = 0; j < J; ++j) acc[i][j] = Arith<PL>::mfma(af, bf[j], acc[i][j]);
        }
    };

    if constexpr (FULL) {
        // Look-ahead pipeline: chunk c + 1 is split into LDS at the end of chunk c from registers loaded kWgradDepth
        // chunks earlier, so kWgradDepth chunks (2 x 32 KiB per workgroup at TN = 256) stay in flight across
        // the chunk barriers -- a one-chunk look-ahead behind __syncthreads (whose release fence waits
        // vmcnt(0)) left ~32 KiB per CU in flight, about half of what the HBM latency asks for.
        constexpr int D = kWgradDepth;
        float4 ra[D][perA], rb[D][perB];
        {
            float4 va[perA], vb[perB];
            load_tile<TN, true, MASKN, RAG == 1>(p.dz, RSLRL_WGRAD_LDZ(p), m_begin, m_end, p.N, va, RSLRL_WGRAD_BACK(p));
            load_tile<kTK, true, false, RAG == 2>(p.x, RSLRL_WGRAD_LDX(p), m_begin, m_end, p.K, vb, RSLRL_WGRAD_BACK(p));
            accum_a(va);
            accum_b(vb);
            store_tile<TN, PL>(va, lds[0], sa);
            store_tile<kTK, PL>(vb, lds[0] + PL * planeA, sb);
        }
        // every look-ahead load is issued, past the end clamped to the last chunk (data unused): with
        // conditional loads the waitcnt pass cannot count the younger slot's loads and waits vmcnt(0)
        auto chunk_row = [&](int c) { return m_begin + static_cast<int64_t>(c < nchunks ? c : nchunks - 1) * kMC; };
#pragma unroll
        for (int d = 1; d <= D; ++d) {
            load_tile<TN, true, MASKN, RAG == 1>(p.dz, RSLRL_WGRAD_LDZ(p), chunk_row(d), m_end, p.N, ra[d % D], RSLRL_WGRAD_BACK(p));
            load_tile<kTK, true, false, RAG == 2>(p.x, RSLRL_WGRAD_LDX(p), chunk_row(d), m_end, p.K, rb[d % D], RSLRL_WGRAD_BACK(p));
        }
        __syncthreads();
        // chunk c (ring position u = c % D) followed by chunk c + 1: no branch between a slot's loads and their
        // use, so the waitcnt pass counts the younger slot's loads (vmcnt(4 per slot)) instead of draining
        auto step = [&](auto uc, int c) {
            constexpr int u = decltype(uc)::value;
            constexpr int s = (u + 1) % D;
            compute(lds[u & 1]);
            __builtin_amdgcn_sched_barrier(0);  // the splits below stay behind this chunk's MFMAs
            accum_a(ra[s]);  // chunk c + 1: every real chunk is stored (and summed) exactly once
            accum_b(rb[s]);
            store_tile<TN, PL>(ra[s], lds[(u + 1) & 1], sa);
            store_tile<kTK, PL>(rb[s], lds[(u + 1) & 1] + PL * planeA, sb);
            load_tile<TN, true, MASKN, RAG == 1>(p.dz, RSLRL_WGRAD_LDZ(p), chunk_row(c + 1 + D), m_end, p.N, ra[s], RSLRL_WGRAD_BACK(p));
            load_tile<kTK, true, false, RAG == 2>(p.x, RSLRL_WGRAD_LDX(p), chunk_row(c + 1 + D), m_end, p.K, rb[s], RSLRL_WGRAD_BACK(p));
            // only the LDS writes must retire before the barrier (not the look-ahead loads)
            asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
        };
        static_assert(D == 2 || D == 4, "the host guarantees a chunk count that is a multiple of D >= 2");
        int c0 = 0;
        for (; c0 + D < nchunks; c0 += D) {
            step(std::integral_constant<int, 0>{}, c0);
            step(std::integral_constant<int, 1>{}, c0 + 1);
            if constexpr (D == 4) {
                step(std::integral_constant<int, 2>{}, c0 + 2);
                step(std::integral_constant<int, 3>{}, c0 + 3);
            }
        }
        step(std::integral_constant<int, 0>{}, c0);
        if constexpr (D == 4) {
            step(std::integral_constant<int, 1>{}, c0 + 1);
            step(std::integral_constant<int, 2>{}, c0 + 2);
        }
        compute(lds[1]);
    } else {
    float4 va[perA], vb[perB];
    if (nchunks > 0) {
        load_tile<TN, FULL, false, RAG == 1>(p.dz, RSLRL_WGRAD_LDZ(p), m_begin, m_end, p.N, va, RSLRL_WGRAD_BACK(p));
        load_tile<kTK, FULL, false, RAG == 2>(p.x, RSLRL_WGRAD_LDX(p), m_begin, m_end, p.K, vb, RSLRL_WGRAD_BACK(p));
        accum_a(va);
        accum_b(vb);
        store_tile<TN, PL>(va, lds[0], sa);
        store_tile<kTK, PL>(vb, lds[0] + PL * planeA, sb);
    }
    __syncthreads();
    for (int c = 0; c < nchunks; ++c) {
        const int buf = c & 1;
        const bool more = c + 1 < nchunks;
        if (more) {
            const int64_t m0 = m_begin + static_cast<int64_t>(c + 1) * kMC;
            load_tile<TN, FULL, false, RAG == 1>(p.dz, RSLRL_WGRAD_LDZ(p), m0, m_end, p.N, va, RSLRL_WGRAD_BACK(p));
            load_tile<kTK, FULL, false, RAG == 2>(p.x, RSLRL_WGRAD_LDX(p), m0, m_end, p.K, vb, RSLRL_WGRAD_BACK(p));
        }
        compute(lds[buf]);
        if (more) {
            accum_a(va);
            accum_b(vb);
            store_tile<TN, PL>(va, lds[buf ^ 1], sa);
            store_tile<kTK, PL>(vb, lds[buf ^ 1] + PL * planeA, sb);
        }
        __syncthreads();
    }
    }  // !FULL

    // partial tile -> part[s][n][k]; C/D map: col (k) = lane & 31, row (n) = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
    const int lane = threadIdx.x & 63;
    const int l32 = lane & 31;
    const int h = lane >> 5;
    const float unscale = PL == 2 ? (1.f / sa) * (1.f / sb) : 1.f;  // exact: powers of two
    const int E = CS == 1 ? p.N : (CS == 2 ? p.K : 0);
    float* out = p.part + static_cast<int64_t>(blockIdx.x) * RSLRL_WGRAD_SLICE_FLOATS(p, E);
    if constexpr (CS != 0) {
        // threads t, t + 64, ..., t + 448 hold columns 4 (t & 63) .. + 3 of different rows: fixed-order fold
        float* red = reinterpret_cast<float*>(&lds[0][0]);  // [8][256]
        __syncthreads();  // the last chunk's fragments have been read
        reinterpret_cast<float4*>(red)[threadIdx.x] = csum;
        __syncthreads();
        if (threadIdx.x < 64 RSLRL_WGRAD_AND_CS(p)) {
            float4 t = reinterpret_cast<const float4*>(red)[threadIdx.x];
#pragma unroll
            for (int g = 1; g < 8; ++g) {
                const float4 v = reinterpret_cast<const float4*>(red)[64 * g + threadIdx.x];
                t.x += v.x; t.y += v.y; t.z += v.z; t.w += v.w;
            }
            const int col = 4 * threadIdx.x;
            float* dst = RSLRL_WGRAD_CS_DST(p, out);
            if (col + 3 < E) {
                *reinterpret_cast<float4*>(dst + col) = t;
            } else {
                const float tv[4] = {t.x, t.y, t.z, t.w};
                for (int e = 0; e < 4; ++e)
                    if (col + e < E) dst[col + e] = tv[e];
            }
        }
    }
#pragma unroll
    for (int i = 0; i < I; ++i)
#pragma unroll
        for (int j = 0; j < J; ++j) {
            const int k = wk * (J * 32) + j * 32 + l32;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int n = wn * (I * 32) + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
                if (n < p.N && k < p.K) out[n * RSLRL_WGRAD_LDX(p) + k] = PL == 2 ? acc[i][j][r] * unscale : acc[i][j][r];
            }
        }
}

// ---- host: the row slices of a launch (the units that launch the body share them: a slice count is part of a
// result's bits)
// the dense entry (mlp_wgrad.hip):
// one workgroup per CU for the 256-row tiles (98 KiB of LDS each); the 32 / 64-row tiles (<= 60 KiB) run two
// per CU, so twice as many slices keep 16 waves per CU in flight; at least 4 chunks per slice
int64_t wgrad_slices(int64_t M, int N) {
    const int64_t chunks = ceil_div(M, kMC);
    const int64_t max_slices = N <= 64 ? 512 : 256;
    return std::max<int64_t>(1, std::min<int64_t>(max_slices, chunks / 4));
}

int64_t wgrad_rows_per(int64_t M, int N) { return ceil_div(ceil_div(M, wgrad_slices(M, N)), kMC) * kMC; }

// the wide entry (mlp_wide.hip): TN x 256 blocks
int wide_tn(int32_t N) { return N <= 64 ? 64 : 256; }

// row slices: the grid stays near one workgroup per CU (two for the 64-row tiles), at least 4 chunks per slice
int64_t wide_rows_per(int64_t M, int32_t N, int32_t K) {
    const int tn = wide_tn(N);
    const int64_t blocks = ceil_div(N, tn) * ceil_div(K, kTK);
    const int64_t chunks = ceil_div(M, kMC);
    const int64_t S = std::max<int64_t>(1, std::min<int64_t>((tn == 64 ? 512 : 256) / blocks, chunks / 4));
    return ceil_div(ceil_div(M, S), kMC) * kMC;
}

}  // namespace
}  // namespace rslrl
