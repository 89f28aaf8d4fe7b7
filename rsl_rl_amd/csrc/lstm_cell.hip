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
//
// ABI 26 adds the training form of the step (rslrl_lstm_cell_train: resets on read, the activated gates kept) and
// its reverse step (rslrl_lstm_cell_bwd) on the same tile; lstm_cell_kernel itself is unchanged.
// ABI 27 adds restart states to both (a reset row reads h_restart / c_restart instead of zero), the state as consumed
// (h_in_out, dW_hh's operand) and the pair forms of both (two problems of one M in one launch, blockIdx.z).
// The `_h` forms (hidden size 512, additions to ABI 34) are the H = 512 instantiations of the any-width forward kernel
// and of the reverse kernel, which take the hidden size as a template parameter; the 256 instantiations keep their
// machine code (profiles/rnn_h512_isa.json).

#include <type_traits>

#include "rnn_cell.h"  // the tile constants, lc_split8, lc_mfma, lc_sigmoid (shared with gru_cell.hip)
#include "rnn_cell_anyd.h"  // the x loads of the forms for any input width (ABI 31)

namespace rslrl {
namespace {

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

// ---------------------------------------------------------------------------------------------------------------
// The training form of the step (rslrl_lstm_cell_train, ABI 26): the same tile, loop and cell update as
// lstm_cell_kernel -- h' and c' carry its bits -- plus a `reset` vector applied on read (a row whose flag is set reads
// its h and c as zero, before the split: the masked_fill_ between two steps without touching the stored h) and the four
// activated gates i, f, g, o of every element, which the lane that owns the element already holds.  Gates are stored
// gate-major: gates[g * gate_stride + row * 256 + col].
//
// ABI 27: a reset row reads h_restart / c_restart (null: zero) in place of its h and c, and h_in_out (null: not
// stored) receives the state as consumed.  Every wave of a workgroup reads all 16 chunks of the 64 rows' h; wave w of
// column half y stores the two chunks 8 y + 2 w, + 1 -- its own 32 columns -- from the registers it has just loaded,
// so the two workgroups of a row tile write disjoint 128-column halves with plain vector stores.
struct LtProblem {
    LcProblem p;
    float* gates;
    const unsigned char* reset;  // [M] or null
    int64_t gate_stride;
    const float* h_restart;      // [M, 256] or null
    const float* c_restart;      // [M, 256] or null
    float* h_in_out;             // [M, 256] or null
};

struct LtArgs {
    LtProblem p[2];
};

__global__ __launch_bounds__(kBlock) void lstm_cell_train_kernel(LtArgs args) {
    const LtProblem& T = args.p[blockIdx.z];
    const LcProblem& P = T.p;
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int hh = lane >> 5;
    const int l32 = lane & 31;
    const int64_t row0 = static_cast<int64_t>(blockIdx.x) * kLcRows;
    const int n0 = 128 * blockIdx.y + 32 * wave;
    const int kc_x = P.D / 16;
    // h == null and nothing to restart from or to store: its chunks contribute nothing
    const bool h_chunks = P.h || T.h_in_out || (T.reset && T.h_restart);
    const int kc = kc_x + (h_chunks ? kLcH / 16 : 0);
    const int gate_units = (kc_x + kLcH / 16) * kLcChunkU;
    const int wunit = (n0 + l32) * 2 + (hh ^ ((l32 >> 3) & 1));
    const int store_c0 = kc_x + 8 * blockIdx.y + 2 * wave;  // the first of this wave's two chunks of h_in_out
    bool rst[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) rst[i] = T.reset && T.reset[row0 + 32 * i + l32] != 0;

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
            float4 lo = make_float4(0.f, 0.f, 0.f, 0.f), hi = lo;
            if (c < kc_x) {
                const float* src = P.x + r * P.D + 16 * c + 8 * hh;
                lo = *reinterpret_cast<const float4*>(src);
                hi = *reinterpret_cast<const float4*>(src + 4);
            } else {
                const float* state = rst[i] ? T.h_restart : P.h;
                const int64_t at = r * kLcH + 16 * (c - kc_x) + 8 * hh;
                if (state) {
                    lo = *reinterpret_cast<const float4*>(state + at);
                    hi = *reinterpret_cast<const float4*>(state + at + 4);
                }
                if (T.h_in_out && (c == store_c0 || c == store_c0 + 1)) {
                    *reinterpret_cast<float4*>(T.h_in_out + at) = lo;
                    *reinterpret_cast<float4*>(T.h_in_out + at + 4) = hi;
                }
            }
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
            const float* cstate = rst[i] ? T.c_restart : P.c;
            if (cstate) cp = *reinterpret_cast<const float4*>(cstate + r * kLcH + n);
            const float cpa[4] = {cp.x, cp.y, cp.z, cp.w};
            float cn[4], hn[4], act[4][4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const double si = lc_sigmoid(static_cast<double>(gate[0][e]));
                const double sf = lc_sigmoid(static_cast<double>(gate[1][e]));
                const double tg = tanh(static_cast<double>(gate[2][e]));
                const double so = lc_sigmoid(static_cast<double>(gate[3][e]));
                const double cd = sf * static_cast<double>(cpa[e]) + si * tg;
                cn[e] = static_cast<float>(cd);
                hn[e] = static_cast<float>(so * tanh(static_cast<double>(cn[e])));  // of the stored c'
                act[0][e] = static_cast<float>(si);
                act[1][e] = static_cast<float>(sf);
                act[2][e] = static_cast<float>(tg);
                act[3][e] = static_cast<float>(so);
            }
            *reinterpret_cast<float4*>(P.c_out + r * kLcH + n) = make_float4(cn[0], cn[1], cn[2], cn[3]);
            *reinterpret_cast<float4*>(P.h_out + r * kLcH + n) = make_float4(hn[0], hn[1], hn[2], hn[3]);
#pragma unroll
            for (int g = 0; g < 4; ++g)
                *reinterpret_cast<float4*>(T.gates + g * T.gate_stride + r * kLcH + n) =
                    make_float4(act[g][0], act[g][1], act[g][2], act[g][3]);
        }
    }
}

// One reverse step (rslrl_lstm_cell_bwd, ABI 26; at H = 512 rslrl_lstm_cell_bwd_h: K = 4 x 512 onto 512 columns, dg_next
// walked gate-major with the chunks ascending as here, W_hh^T as two 256-row images of depth 512 per gate block).  The recurrent term dG_{t+1} W_hh is an x6 GEMM of K = 1024 (the
// four gate blocks of dG_{t+1}, 64 chunks of 16) onto 256 columns, from the layout-0 image of W_hh^T (256 rows, depth
// 1024); the same tile as the forward with one 64 x 32 accumulator per wave, summed by lc_mfma's per-chunk rule.  The
// cell's derivative is register-local and runs in fp64, rounded once per stored value.  Every output element is
// written by exactly one lane; no LDS, no atomics.
struct LbProblem {
    const float* dh;                  // [M, 256]
    const float* dg_next;             // gate-major, or null
    const float* dc_next;             // [M, 256] or null
    const unsigned char* reset_next;  // [M] or null: rows reset between this step and the next
    const float* gates;               // gate-major i, f, g, o of this step
    const float* c_out;               // [M, 256]: c' of this step
    const float* c_prev;              // [M, 256] or null (zeros)
    const unsigned char* reset_cur;   // [M] or null: rows whose c_prev was read as zero
    const uint4* whh_t;               // image of W_hh^T
    float* dg;                        // gate-major out
    float* dc_prev;                   // [M, 256] out
    int64_t gate_stride;              // of gates and dg
    int64_t next_stride;              // of dg_next
    const float* c_restart;           // [M, 256] or null: what c_prev reads where reset_cur is set (ABI 27)
};

struct LbArgs {
    LbProblem p[2];
};

template <int H>
__global__ __launch_bounds__(kBlock) void lstm_cell_bwd_kernel(LbArgs args) {
    const LbProblem& P = args.p[blockIdx.z];
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int hh = lane >> 5;
    const int l32 = lane & 31;
    const int64_t row0 = static_cast<int64_t>(blockIdx.x) * kLcRows;
    const int n0 = 128 * blockIdx.y + 32 * wave;
    int wunit = (n0 + l32) * 2 + (hh ^ ((l32 >> 3) & 1));
    // H > 256: per gate block H / 256 images of W_hh^T's 256 rows n0 / 256 .., each H deep
    if constexpr (H > kLcBlockRows)
        wunit = (n0 / kLcBlockRows) * (H / 16) * kLcChunkU + ((n0 % kLcBlockRows) + l32) * 2 + (hh ^ ((l32 >> 3) & 1));
    bool rn[2], rc[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        rn[i] = P.reset_next && P.reset_next[row0 + 32 * i + l32] != 0;
        rc[i] = P.reset_cur && P.reset_cur[row0 + 32 * i + l32] != 0;
    }
    f32x16 acc[2] = {f32x16{}, f32x16{}};
    constexpr int kSh = H == 512 ? 5 : 4;  // log2 of a gate block's chunks
    static_assert(H / 16 == 1 << kSh, "hidden size");
    if (P.dg_next) {
        for (int c = 0; c < 4 * H / 16; ++c) {
            bf16x8 xf[2][3];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int64_t r = row0 + 32 * i + l32;
                const float* src = P.dg_next + (c >> kSh) * P.next_stride + r * H + 16 * (c & (H / 16 - 1)) + 8 * hh;
                const float4 lo = *reinterpret_cast<const float4*>(src);
                const float4 hi = *reinterpret_cast<const float4*>(src + 4);
                lc_split8(lo, hi, xf[i]);
            }
            bf16x8 wf[3];
            const uint4* img = P.whh_t + c * kLcChunkU + wunit;
            if constexpr (H > kLcBlockRows)
                img = P.whh_t + ((c >> kSh) * (H / kLcBlockRows) * (H / 16) + (c & (H / 16 - 1))) * kLcChunkU + wunit;
#pragma unroll
            for (int q = 0; q < 3; ++q) wf[q] = __builtin_bit_cast(bf16x8, img[q * kLcPlaneU]);
#pragma unroll
            for (int i = 0; i < 2; ++i) acc[i] = lc_mfma(xf[i], wf, acc[i]);
        }
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int64_t r = row0 + 32 * i + l32;
#pragma unroll
        for (int qd = 0; qd < 4; ++qd) {
            const int n = n0 + 8 * qd + 4 * hh;
            const int64_t at = r * H + n;
            const float4 dh4 = *reinterpret_cast<const float4*>(P.dh + at);
            float4 dc4 = make_float4(0.f, 0.f, 0.f, 0.f), cp4 = dc4;
            if (P.dc_next && !rn[i]) dc4 = *reinterpret_cast<const float4*>(P.dc_next + at);
            const float* cstate = rc[i] ? P.c_restart : P.c_prev;
            if (cstate) cp4 = *reinterpret_cast<const float4*>(cstate + at);
            const float4 co4 = *reinterpret_cast<const float4*>(P.c_out + at);
            float4 g4[4];
#pragma unroll
            for (int g = 0; g < 4; ++g) g4[g] = *reinterpret_cast<const float4*>(P.gates + g * P.gate_stride + at);
            const float dha[4] = {dh4.x, dh4.y, dh4.z, dh4.w}, dca[4] = {dc4.x, dc4.y, dc4.z, dc4.w};
            const float cpa[4] = {cp4.x, cp4.y, cp4.z, cp4.w}, coa[4] = {co4.x, co4.y, co4.z, co4.w};
            float ga[4][4];
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                ga[g][0] = g4[g].x;
                ga[g][1] = g4[g].y;
                ga[g][2] = g4[g].z;
                ga[g][3] = g4[g].w;
            }
            float out[4][4], dcp[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float rec = rn[i] ? 0.0f : acc[i][4 * qd + e];
                const double dht = static_cast<double>(dha[e]) + static_cast<double>(rec);
                const double gi = ga[0][e], gf = ga[1][e], gg = ga[2][e], go = ga[3][e];
                const double tc = tanh(static_cast<double>(coa[e]));
                const double d_o = dht * tc;
                const double dc = static_cast<double>(dca[e]) + dht * go * (1.0 - tc * tc);
                out[0][e] = static_cast<float>(dc * gg * gi * (1.0 - gi));
                out[1][e] = static_cast<float>(dc * static_cast<double>(cpa[e]) * gf * (1.0 - gf));
                out[2][e] = static_cast<float>(dc * gi * (1.0 - gg * gg));
                out[3][e] = static_cast<float>(d_o * go * (1.0 - go));
                dcp[e] = static_cast<float>(dc * gf);
            }
#pragma unroll
            for (int g = 0; g < 4; ++g)
                *reinterpret_cast<float4*>(P.dg + g * P.gate_stride + at) =
                    make_float4(out[g][0], out[g][1], out[g][2], out[g][3]);
            *reinterpret_cast<float4*>(P.dc_prev + at) = make_float4(dcp[0], dcp[1], dcp[2], dcp[3]);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------
// ABI 31: the forward forms for any input width 1 <= D <= 1024 (rslrl_lstm_cell_anyd and its pair / training
// forms).  Tile, gate images, per-chunk summation and the cell update are the kernels' above; the x side of [x | h] is
// K = ceil(D / 16) chunks deep: the D / 16 whole chunks, then the one partial chunk, which alone takes the masked
// loads (rnn_cell_anyd.h holds the two load forms, XL), then the 16 chunks of h.  A masked element is an exact zero and
// the image is zero beyond column D, so h', c', the gates and h_in_out equal, bit for bit, the kernels above on the
// problem zero-padded to 16 K columns (tests/test_gpu_rnn_anyd.py).  TRAIN: lstm_cell_train_kernel's extras.
//
// H: the hidden size, 256 or 512.  Same tile at both: grid.y = H / 128 column slabs, K = ceil(D / 16) + H / 16 chunks in
// the same order (x chunks, then the h chunks ascending), every state row H floats, the training form's h_in_out store
// over all H / 16 h chunks (wave w of slab y still owns the chunks 8 y + 2 w, + 1).  At 512 a gate's image is two 256-row
// blocks (rslrl_lstm_prepare_image_h) and the wave reads the block n0 / 256.
__device__ __forceinline__ const LcProblem& lc_cell_of(const LcProblem& p) { return p; }
__device__ __forceinline__ const LcProblem& lc_cell_of(const LtProblem& t) { return t.p; }

template <int XL, bool TRAIN, int H>
__global__ __launch_bounds__(kBlock) void lstm_cell_anyd_kernel(std::conditional_t<TRAIN, LtArgs, LcArgs> args) {
    const auto& T = args.p[blockIdx.z];
    const LcProblem& P = lc_cell_of(T);
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int hh = lane >> 5;
    const int l32 = lane & 31;
    const int64_t row0 = static_cast<int64_t>(blockIdx.x) * kLcRows;
    const int n0 = 128 * blockIdx.y + 32 * wave;
    const int kc_whole = P.D / 16;
    const int kc_x = anyd_x_chunks(P.D);
    bool h_chunks = P.h != nullptr;  // h == null (and nothing to restart from or to store): no h chunks
    if constexpr (TRAIN) h_chunks = P.h || T.h_in_out || (T.reset && T.h_restart);
    // one image block holds 256 rows of a gate: H / 256 consecutive blocks per gate, this wave's is n0 / 256
    const int block_units = (kc_x + H / 16) * kLcChunkU;
    const int gate_units = (H / kLcBlockRows) * block_units;
    const uint4* img = P.image + (n0 + l32) * 2 + (hh ^ ((l32 >> 3) & 1));
    if constexpr (H > kLcBlockRows)
        img = P.image + (n0 / kLcBlockRows) * block_units + ((n0 % kLcBlockRows) + l32) * 2 + (hh ^ ((l32 >> 3) & 1));
    const int kc = kc_x + (h_chunks ? H / 16 : 0);
    const int store_c0 = kc_x + 8 * blockIdx.y + 2 * wave;  // the first of this wave's two chunks of h_in_out
    bool rst[2] = {false, false};
    if constexpr (TRAIN) {
#pragma unroll
        for (int i = 0; i < 2; ++i) rst[i] = T.reset && T.reset[row0 + 32 * i + l32] != 0;
    }

    f32x16 acc[4][2];
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
        for (int i = 0; i < 2; ++i) acc[g][i] = f32x16{};

    // one loop over the chunks of [x | h], as above; which load a chunk takes is wave-uniform
    for (int c = 0; c < kc; ++c) {
        bf16x8 xf[2][3];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int64_t r = row0 + 32 * i + l32;
            float4 lo = make_float4(0.f, 0.f, 0.f, 0.f), hi = lo;
            if (c < kc_whole) {
                xl_load_whole<XL>(P.x + r * P.D, 16 * c + 8 * hh, lo, hi);
            } else if (c < kc_x) {  // the one partial chunk
                xl_load_tail<XL>(P.x + r * P.D, 16 * c + 8 * hh, P.D, lo, hi);
            } else {
                const int64_t at = r * H + 16 * (c - kc_x) + 8 * hh;
                const float* state = P.h;
                if constexpr (TRAIN) state = rst[i] ? T.h_restart : P.h;
                if (state) {
                    lo = *reinterpret_cast<const float4*>(state + at);
                    hi = *reinterpret_cast<const float4*>(state + at + 4);
                }
                if constexpr (TRAIN) {
                    if (T.h_in_out && (c == store_c0 || c == store_c0 + 1)) {
                        *reinterpret_cast<float4*>(T.h_in_out + at) = lo;
                        *reinterpret_cast<float4*>(T.h_in_out + at + 4) = hi;
                    }
                }
            }
            lc_split8(lo, hi, xf[i]);
        }
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            bf16x8 wf[3];
            const uint4* gi = img + static_cast<int64_t>(g) * gate_units + c * kLcChunkU;
#pragma unroll
            for (int q = 0; q < 3; ++q) wf[q] = __builtin_bit_cast(bf16x8, gi[q * kLcPlaneU]);
#pragma unroll
            for (int i = 0; i < 2; ++i) acc[g][i] = lc_mfma(xf[i], wf, acc[g][i]);
        }
    }

    // the cell update of the kernels above
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int64_t r = row0 + 32 * i + l32;
#pragma unroll
        for (int qd = 0; qd < 4; ++qd) {
            const int n = n0 + 8 * qd + 4 * hh;
            float gate[4][4];
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const float4 bi = *reinterpret_cast<const float4*>(P.b_ih + g * H + n);
                const float4 bh = *reinterpret_cast<const float4*>(P.b_hh + g * H + n);
                const float bia[4] = {bi.x, bi.y, bi.z, bi.w}, bha[4] = {bh.x, bh.y, bh.z, bh.w};
#pragma unroll
                for (int e = 0; e < 4; ++e) gate[g][e] = (acc[g][i][4 * qd + e] + bia[e]) + bha[e];
            }
            float4 cp = make_float4(0.f, 0.f, 0.f, 0.f);
            const float* cstate = P.c;
            if constexpr (TRAIN) cstate = rst[i] ? T.c_restart : P.c;
            if (cstate) cp = *reinterpret_cast<const float4*>(cstate + r * H + n);
            const float cpa[4] = {cp.x, cp.y, cp.z, cp.w};
            float cn[4], hn[4], act[4][4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const double si = lc_sigmoid(static_cast<double>(gate[0][e]));
                const double sf = lc_sigmoid(static_cast<double>(gate[1][e]));
                const double tg = tanh(static_cast<double>(gate[2][e]));
                const double so = lc_sigmoid(static_cast<double>(gate[3][e]));
                const double cd = sf * static_cast<double>(cpa[e]) + si * tg;
                cn[e] = static_cast<float>(cd);
                hn[e] = static_cast<float>(so * tanh(static_cast<double>(cn[e])));  // of the stored c'
                act[0][e] = static_cast<float>(si);
                act[1][e] = static_cast<float>(sf);
                act[2][e] = static_cast<float>(tg);
                act[3][e] = static_cast<float>(so);
            }
            *reinterpret_cast<float4*>(P.c_out + r * H + n) = make_float4(cn[0], cn[1], cn[2], cn[3]);
            *reinterpret_cast<float4*>(P.h_out + r * H + n) = make_float4(hn[0], hn[1], hn[2], hn[3]);
            if constexpr (TRAIN) {
#pragma unroll
                for (int g = 0; g < 4; ++g)
                    *reinterpret_cast<float4*>(T.gates + g * T.gate_stride + r * H + n) =
                        make_float4(act[g][0], act[g][1], act[g][2], act[g][3]);
            }
        }
    }
}

// anyd: the scope of the ABI 31 forms -- any 1 <= D <= 1024, x's base 4-byte aligned where D % 4 != 0
int lc_check(const rslrl_lstm_cell_t* a, int64_t M, bool anyd = false, int hidden = kLcH) {
    if (!a) return RSLRL_E_INVALID_ARGUMENT;
    const bool width_ok = anyd ? anyd_width_ok(a->D) : (a->D >= 16 && a->D <= 256 && a->D % 16 == 0);
    if (a->hidden != hidden || a->layers != 1 || !width_ok || M < kLcRows || M % kLcRows || M > (INT64_C(1) << 31))
        return RSLRL_E_UNSUPPORTED;
    if (!a->x || !a->image || !a->b_ih || !a->b_hh || !a->h_out || !a->c_out) return RSLRL_E_INVALID_ARGUMENT;
    // every block reads whole rows of h while others write h_out: they must not be one buffer (c_out may be c)
    if (a->h_out == a->h || a->h_out == a->c_out) return RSLRL_E_INVALID_ARGUMENT;
    const uintptr_t ptrs[] = {reinterpret_cast<uintptr_t>(a->h),     reinterpret_cast<uintptr_t>(a->c),
                              reinterpret_cast<uintptr_t>(a->image), reinterpret_cast<uintptr_t>(a->b_ih),
                              reinterpret_cast<uintptr_t>(a->b_hh),  reinterpret_cast<uintptr_t>(a->h_out),
                              reinterpret_cast<uintptr_t>(a->c_out)};
    for (uintptr_t p : ptrs)
        if (p & 15) return RSLRL_E_MISALIGNED;
    if (anyd ? !anyd_x_aligned(a->x, a->D) : (reinterpret_cast<uintptr_t>(a->x) & 15) != 0) return RSLRL_E_MISALIGNED;
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

namespace {

int lt_problem(const rslrl_lstm_train_t* a, int64_t M, LtProblem* out, bool anyd = false, int hidden = kLcH) {
    if (!a) return RSLRL_E_INVALID_ARGUMENT;
    const int rc = lc_check(&a->cell, M, anyd, hidden);
    if (rc != RSLRL_OK) return rc;
    if (!a->gates || a->gate_stride < M * hidden) return RSLRL_E_INVALID_ARGUMENT;
    // other blocks read whole rows of h and h_restart while h_in_out is written, and a wave stores its columns of
    // h_in_out before it reads the same columns of c
    const float* const no_alias[] = {a->cell.h, a->cell.c, a->h_restart, a->c_restart, a->cell.h_out, a->cell.c_out};
    for (const float* p : no_alias)
        if (a->h_in_out && a->h_in_out == p) return RSLRL_E_INVALID_ARGUMENT;
    if (a->h_restart && a->h_restart == a->cell.h_out) return RSLRL_E_INVALID_ARGUMENT;
    if (reinterpret_cast<uintptr_t>(a->gates) & 15 || a->gate_stride % 4 ||
        reinterpret_cast<uintptr_t>(a->h_restart) & 15 || reinterpret_cast<uintptr_t>(a->c_restart) & 15 ||
        reinterpret_cast<uintptr_t>(a->h_in_out) & 15)
        return RSLRL_E_MISALIGNED;
    *out = LtProblem{lc_problem(&a->cell), a->gates, a->reset, a->gate_stride, a->h_restart, a->c_restart, a->h_in_out};
    return RSLRL_OK;
}

}  // namespace

extern "C" int rslrl_lstm_cell_train_pair(const rslrl_lstm_train_t* a0, const rslrl_lstm_train_t* a1, int64_t M,
                                          rslrl_stream_t stream) {
    LtArgs args{};
    int rc = lt_problem(a0, M, &args.p[0]);
    if (rc != RSLRL_OK) return rc;
    unsigned np = 1;
    if (a1) {
        rc = lt_problem(a1, M, &args.p[1]);
        if (rc != RSLRL_OK) return rc;
        np = 2;
    }
    hipLaunchKernelGGL(lstm_cell_train_kernel, dim3(static_cast<unsigned>(M / kLcRows), 2, np), dim3(kBlock), 0,
                       reinterpret_cast<hipStream_t>(stream), args);
    return launch_status();
}

extern "C" int rslrl_lstm_cell_train(const rslrl_lstm_train_t* a, int64_t M, rslrl_stream_t stream) {
    return rslrl_lstm_cell_train_pair(a, nullptr, M, stream);
}

extern "C" size_t rslrl_lstm_whh_t_image_bytes(void) { return rslrl_linear_bimage_bytes(4 * kLcH); }

extern "C" int rslrl_lstm_prepare_whh_t_image(const float* w_hh, int32_t hidden, void* image, rslrl_stream_t stream) {
    if (hidden != kLcH) return RSLRL_E_UNSUPPORTED;
    if (!w_hh || !image) return RSLRL_E_INVALID_ARGUMENT;
    if (reinterpret_cast<uintptr_t>(image) & 15) return RSLRL_E_MISALIGNED;
    return rslrl_linear_prepare_bimage(w_hh, kLcH, 4 * kLcH, 1, image, stream);  // B[n][k] = W_hh[k][n]
}

namespace {

int lb_problem(const rslrl_lstm_bwd_t* a, int64_t M, LbProblem* out, int hidden = kLcH) {
    if (!a) return RSLRL_E_INVALID_ARGUMENT;
    if (a->hidden != hidden || a->layers != 1 || M < kLcRows || M % kLcRows || M > (INT64_C(1) << 31))
        return RSLRL_E_UNSUPPORTED;
    if (!a->dh || !a->gates || !a->c_out || !a->dg || !a->dc_prev || (a->dg_next && !a->whh_t_image))
        return RSLRL_E_INVALID_ARGUMENT;
    if (a->gate_stride < M * hidden || (a->dg_next && a->next_stride < M * hidden)) return RSLRL_E_INVALID_ARGUMENT;
    // a lane reads dc_next and writes dc_prev at its own element only, but the GEMM reads whole rows of dg_next
    if (a->dg == a->dg_next) return RSLRL_E_INVALID_ARGUMENT;
    const uintptr_t ptrs[] = {reinterpret_cast<uintptr_t>(a->dh),      reinterpret_cast<uintptr_t>(a->dg_next),
                              reinterpret_cast<uintptr_t>(a->dc_next), reinterpret_cast<uintptr_t>(a->gates),
                              reinterpret_cast<uintptr_t>(a->c_out),   reinterpret_cast<uintptr_t>(a->c_prev),
                              reinterpret_cast<uintptr_t>(a->whh_t_image), reinterpret_cast<uintptr_t>(a->dg),
                              reinterpret_cast<uintptr_t>(a->dc_prev), reinterpret_cast<uintptr_t>(a->c_restart)};
    for (uintptr_t p : ptrs)
        if (p & 15) return RSLRL_E_MISALIGNED;
    if (a->gate_stride % 4 || a->next_stride % 4) return RSLRL_E_MISALIGNED;
    *out = LbProblem{a->dh, a->dg_next, a->dc_next, a->reset_next, a->gates, a->c_out, a->c_prev, a->reset_cur,
                     static_cast<const uint4*>(a->whh_t_image), a->dg, a->dc_prev, a->gate_stride, a->next_stride,
                     a->c_restart};
    return RSLRL_OK;
}

}  // namespace

extern "C" int rslrl_lstm_cell_bwd_pair(const rslrl_lstm_bwd_t* a0, const rslrl_lstm_bwd_t* a1, int64_t M,
                                        rslrl_stream_t stream) {
    LbArgs args{};
    int rc = lb_problem(a0, M, &args.p[0]);
    if (rc != RSLRL_OK) return rc;
    unsigned np = 1;
    if (a1) {
        rc = lb_problem(a1, M, &args.p[1]);
        if (rc != RSLRL_OK) return rc;
        np = 2;
    }
    hipLaunchKernelGGL(lstm_cell_bwd_kernel<kLcH>, dim3(static_cast<unsigned>(M / kLcRows), 2, np), dim3(kBlock), 0,
                       reinterpret_cast<hipStream_t>(stream), args);
    return launch_status();
}

extern "C" int rslrl_lstm_cell_bwd(const rslrl_lstm_bwd_t* a, int64_t M, rslrl_stream_t stream) {
    return rslrl_lstm_cell_bwd_pair(a, nullptr, M, stream);
}

// ---- ABI 31: any input width (the kernels and scope are described at lstm_cell_anyd_kernel)
extern "C" size_t rslrl_lstm_image_bytes_anyd(int32_t D) {
    if (!anyd_width_ok(D)) return 0;
    return 4 * (rslrl_linear_bimage_bytes(D) + rslrl_linear_bimage_bytes(kLcH));
}

extern "C" int rslrl_lstm_prepare_image_anyd(const float* w_ih, const float* w_hh, int32_t D, int32_t hidden,
                                             void* image, rslrl_stream_t stream) {
    if (hidden != kLcH || !anyd_width_ok(D)) return RSLRL_E_UNSUPPORTED;
    if (!w_ih || !w_hh || !image) return RSLRL_E_INVALID_ARGUMENT;
    if (reinterpret_cast<uintptr_t>(image) & 15) return RSLRL_E_MISALIGNED;
    const size_t x_bytes = rslrl_linear_bimage_bytes(D);  // ceil(D / 16) chunks, zero from column D on
    const size_t gate_bytes = x_bytes + rslrl_linear_bimage_bytes(kLcH);
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

namespace {

// one launch reads both problems with one load form: the ragged one as soon as either width is no multiple of 4
// H / 128 column slabs of 128 in grid.y
template <bool TRAIN, int H = kLcH, typename Args>
int lc_launch_anyd(const Args& args, int d0, int d1, unsigned np, int64_t M, rslrl_stream_t stream) {
    const dim3 grid(static_cast<unsigned>(M / kLcRows), H / 128, np);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (d0 % 4 || d1 % 4)
        hipLaunchKernelGGL((lstm_cell_anyd_kernel<kXlRagged, TRAIN, H>), grid, dim3(kBlock), 0, st, args);
    else
        hipLaunchKernelGGL((lstm_cell_anyd_kernel<kXlQuad, TRAIN, H>), grid, dim3(kBlock), 0, st, args);
    return launch_status();
}

}  // namespace

extern "C" int rslrl_lstm_cell_pair_anyd(const rslrl_lstm_cell_t* a0, const rslrl_lstm_cell_t* a1, int64_t M,
                                         rslrl_stream_t stream) {
    int rc = lc_check(a0, M, true);
    if (rc != RSLRL_OK) return rc;
    LcArgs args{};
    args.p[0] = lc_problem(a0);
    if (a1) {
        rc = lc_check(a1, M, true);
        if (rc != RSLRL_OK) return rc;
        args.p[1] = lc_problem(a1);
    }
    return lc_launch_anyd<false>(args, a0->D, a1 ? a1->D : 0, a1 ? 2 : 1, M, stream);
}

extern "C" int rslrl_lstm_cell_anyd(const rslrl_lstm_cell_t* a, int64_t M, rslrl_stream_t stream) {
    return rslrl_lstm_cell_pair_anyd(a, nullptr, M, stream);
}

extern "C" int rslrl_lstm_cell_train_pair_anyd(const rslrl_lstm_train_t* a0, const rslrl_lstm_train_t* a1, int64_t M,
                                               rslrl_stream_t stream) {
    LtArgs args{};
    int rc = lt_problem(a0, M, &args.p[0], true);
    if (rc != RSLRL_OK) return rc;
    if (a1) {
        rc = lt_problem(a1, M, &args.p[1], true);
        if (rc != RSLRL_OK) return rc;
    }
    return lc_launch_anyd<true>(args, a0->cell.D, a1 ? a1->cell.D : 0, a1 ? 2 : 1, M, stream);
}

extern "C" int rslrl_lstm_cell_train_anyd(const rslrl_lstm_train_t* a, int64_t M, rslrl_stream_t stream) {
    return rslrl_lstm_cell_train_pair_anyd(a, nullptr, M, stream);
}

// ---- The `_h` forms: hidden size 512 (additions to ABI 34; the kernels are the H = 512 instantiations of
// lstm_cell_anyd_kernel and lstm_cell_bwd_kernel, the scope is the `_anyd` forms' with hidden == 512).  A gate's
// weights are two 256-row block images, each the x part (depth D) followed by the h part (depth 512); W_hh^T is, per
// gate block of dg_next, two 256-row images of depth 512.
namespace {

bool lc_hidden_h_ok(int32_t hidden) { return hidden == kLcHWide; }

}  // namespace

extern "C" size_t rslrl_lstm_image_bytes_h(int32_t D, int32_t hidden) {
    if (!lc_hidden_h_ok(hidden) || !anyd_width_ok(D)) return 0;
    return 4 * (kLcHWide / kLcBlockRows) * (rslrl_linear_bimage_bytes(D) + rslrl_linear_bimage_bytes(kLcHWide));
}

extern "C" int rslrl_lstm_prepare_image_h(const float* w_ih, const float* w_hh, int32_t D, int32_t hidden, void* image,
                                          rslrl_stream_t stream) {
    if (!lc_hidden_h_ok(hidden) || !anyd_width_ok(D)) return RSLRL_E_UNSUPPORTED;
    if (!w_ih || !w_hh || !image) return RSLRL_E_INVALID_ARGUMENT;
    if (reinterpret_cast<uintptr_t>(image) & 15) return RSLRL_E_MISALIGNED;
    const size_t x_bytes = rslrl_linear_bimage_bytes(D);
    const size_t block_bytes = x_bytes + rslrl_linear_bimage_bytes(kLcHWide);
    rslrl_bimage_desc_t d[16];
    for (int gb = 0; gb < 8; ++gb) {  // image block gb = 2 gate + block: rows 256 gb .. of W_ih and W_hh
        char* base = static_cast<char*>(image) + gb * block_bytes;
        const int64_t row = static_cast<int64_t>(gb) * kLcBlockRows;
        d[2 * gb] = rslrl_bimage_desc_t{w_ih + row * D, base, kLcBlockRows, D, 0, RSLRL_BIMAGE_LAYOUT_GEMM};
        d[2 * gb + 1] = rslrl_bimage_desc_t{w_hh + row * kLcHWide, base + x_bytes, kLcBlockRows, kLcHWide, 0,
                                            RSLRL_BIMAGE_LAYOUT_GEMM};
    }
    return rslrl_linear_prepare_bimages(d, 16, stream);
}

extern "C" int rslrl_lstm_cell_pair_h(const rslrl_lstm_cell_t* a0, const rslrl_lstm_cell_t* a1, int64_t M,
                                      rslrl_stream_t stream) {
    int rc = lc_check(a0, M, true, kLcHWide);
    if (rc != RSLRL_OK) return rc;
    LcArgs args{};
    args.p[0] = lc_problem(a0);
    if (a1) {
        rc = lc_check(a1, M, true, kLcHWide);
        if (rc != RSLRL_OK) return rc;
        args.p[1] = lc_problem(a1);
    }
    return lc_launch_anyd<false, kLcHWide>(args, a0->D, a1 ? a1->D : 0, a1 ? 2 : 1, M, stream);
}

extern "C" int rslrl_lstm_cell_h(const rslrl_lstm_cell_t* a, int64_t M, rslrl_stream_t stream) {
    return rslrl_lstm_cell_pair_h(a, nullptr, M, stream);
}

extern "C" int rslrl_lstm_cell_train_pair_h(const rslrl_lstm_train_t* a0, const rslrl_lstm_train_t* a1, int64_t M,
                                            rslrl_stream_t stream) {
    LtArgs args{};
    int rc = lt_problem(a0, M, &args.p[0], true, kLcHWide);
    if (rc != RSLRL_OK) return rc;
    if (a1) {
        rc = lt_problem(a1, M, &args.p[1], true, kLcHWide);
        if (rc != RSLRL_OK) return rc;
    }
    return lc_launch_anyd<true, kLcHWide>(args, a0->cell.D, a1 ? a1->cell.D : 0, a1 ? 2 : 1, M, stream);
}

extern "C" int rslrl_lstm_cell_train_h(const rslrl_lstm_train_t* a, int64_t M, rslrl_stream_t stream) {
    return rslrl_lstm_cell_train_pair_h(a, nullptr, M, stream);
}

extern "C" size_t rslrl_lstm_whh_t_image_bytes_h(int32_t hidden) {
    if (!lc_hidden_h_ok(hidden)) return 0;
    return 4 * rslrl_linear_bimage_wide_bytes(kLcHWide, kLcHWide);
}

extern "C" int rslrl_lstm_prepare_whh_t_image_h(const float* w_hh, int32_t hidden, void* image, rslrl_stream_t stream) {
    if (!lc_hidden_h_ok(hidden)) return RSLRL_E_UNSUPPORTED;
    if (!w_hh || !image) return RSLRL_E_INVALID_ARGUMENT;
    if (reinterpret_cast<uintptr_t>(image) & 15) return RSLRL_E_MISALIGNED;
    const size_t gate_bytes = rslrl_linear_bimage_wide_bytes(kLcHWide, kLcHWide);
    for (int g = 0; g < 4; ++g) {  // B[n][k] = W_hh[512 g + k][n]: the two 256-row blocks of n, each 512 deep
        const int rc = rslrl_linear_prepare_bimage_wide(w_hh + static_cast<int64_t>(g) * kLcHWide * kLcHWide, kLcHWide,
                                                        kLcHWide, 1, static_cast<char*>(image) + g * gate_bytes, stream);
        if (rc != RSLRL_OK) return rc;
    }
    return RSLRL_OK;
}

extern "C" int rslrl_lstm_cell_bwd_pair_h(const rslrl_lstm_bwd_t* a0, const rslrl_lstm_bwd_t* a1, int64_t M,
                                          rslrl_stream_t stream) {
    LbArgs args{};
    int rc = lb_problem(a0, M, &args.p[0], kLcHWide);
    if (rc != RSLRL_OK) return rc;
    unsigned np = 1;
    if (a1) {
        rc = lb_problem(a1, M, &args.p[1], kLcHWide);
        if (rc != RSLRL_OK) return rc;
        np = 2;
    }
    hipLaunchKernelGGL(lstm_cell_bwd_kernel<kLcHWide>, dim3(static_cast<unsigned>(M / kLcRows), kLcHWide / 128, np),
                       dim3(kBlock), 0, reinterpret_cast<hipStream_t>(stream), args);
    return launch_status();
}

extern "C" int rslrl_lstm_cell_bwd_h(const rslrl_lstm_bwd_t* a, int64_t M, rslrl_stream_t stream) {
    return rslrl_lstm_cell_bwd_pair_h(a, nullptr, M, stream);
}
