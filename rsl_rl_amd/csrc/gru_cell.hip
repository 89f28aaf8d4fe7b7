// One GRU time step for M rows in one launch on gfx950 (rslrl_gru_cell / _pair, ABI 28), its training form
// (rslrl_gru_cell_train / _pair) and its reverse step (rslrl_gru_cell_bwd / _pair): what lstm_cell.hip is to an
// nn.LSTM of one layer and hidden size 256, for an nn.GRU of the same shape (rnn_type="gru").
//
//   r = s(x W_ir^T + b_ir + h W_hr^T + b_hr)      z = s(x W_iz^T + b_iz + h W_hz^T + b_hz)      (torch's order r, z, n)
//   a = h W_hn^T + b_hn                           n = tanh(x W_in^T + b_in + r a)
//   h' = (1 - z) n + z h                                                    h NULL: zeros (the step after reset())
//
// Tile, image layout and arithmetic are the LSTM cell's (rnn_cell.h): a wave owns 32 hidden columns of all gates for 64
// rows in four 64 x 32 accumulator groups (128 registers) -- here r, z, the x side of n and the h side of n, which
// must stay apart because r multiplies the h side only.  r and z take every 16-deep chunk of [x | h], n_x the x
// chunks and n_h the h chunks: three gate blocks per chunk where the LSTM has four.  x6 split-bf16 MFMA with
// lc_mfma's per-chunk summation, fp32 accumulation; the pointwise part in fp64, rounded once per stored value.  No
// LDS, no atomics, every output element written by one lane: two calls give the same bits.
// Weights: per gate one layout-0 image of the 256 rows of [W_ih | W_hh] (rslrl_gru_prepare_image).
// The `_h` forms (hidden size 512, additions to ABI 34) are the H = 512 instantiations of gru_cell_anyd_kernel and
// gru_cell_bwd_kernel, as in lstm_cell.hip: grid.y = 4 column slabs, two 256-row block images per gate, the chunk order
// unchanged; the 256 instantiations keep their machine code (profiles/rnn_h512_isa.json).

#include <type_traits>

#include "rnn_cell.h"
#include "rnn_cell_anyd.h"  // the x loads of the forms for any input width (ABI 31)

namespace rslrl {
namespace {

constexpr int kGcHChunks = kLcH / 16;

struct GcProblem {
    const float* x;     // [M, D]
    const float* h;     // [M, 256] or null
    const uint4* image; // 3 gate images of depth D + 256
    const float* b_ih;  // [768]
    const float* b_hh;  // [768]
    float* h_out;       // [M, 256]
    int D;
};

struct GcArgs {
    GcProblem p[2];
};

// One chunk's MFMAs of the three gate blocks: r and z into their accumulators, n into `an` (the x-side or the h-side
// group -- the caller's loop decides, so no accumulator is ever indexed by a run-time value).
// The scheduling barrier after each gate block keeps the compiler from issuing all nine weight loads of a chunk at the
// top of the loop body: with the 128 accumulator registers live that put the two forward kernels at 352 registers and
// one wave per SIMD.  With it, and __launch_bounds__(kBlock, 2), they run two waves per SIMD like the LSTM kernels:
// 257 -> 176 us per gru_cell_pair launch and 300 -> 245 us per gru_cell_train_pair launch at 16,384 rows, equal at
// 1,024.
__device__ __forceinline__ void gc_chunk(const uint4* img, int gate_units, const bf16x8 (&xf)[2][3], f32x16 (&ar)[2],
                                         f32x16 (&az)[2], f32x16 (&an)[2]) {
#pragma unroll
    for (int g = 0; g < 3; ++g) {
        bf16x8 wf[3];
#pragma unroll
        for (int q = 0; q < 3; ++q) wf[q] = __builtin_bit_cast(bf16x8, img[g * gate_units + q * kLcPlaneU]);
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            if (g == 0) ar[i] = lc_mfma(xf[i], wf, ar[i]);
            if (g == 1) az[i] = lc_mfma(xf[i], wf, az[i]);
            if (g == 2) an[i] = lc_mfma(xf[i], wf, an[i]);
        }
        __builtin_amdgcn_sched_barrier(0);
    }
}

__device__ __forceinline__ void gc_unpack(const float4& v, float (&a)[4]) {
    a[0] = v.x;
    a[1] = v.y;
    a[2] = v.z;
    a[3] = v.w;
}

// The pointwise part of one column quad: the activated r, z, n, the biased h-side pre-activation a and h' from the four
// accumulators, the biases and the entering h.  Shared by the rollout step and the training form, so that both round
// the same values.  Pre-activations are fp32 sums in the LSTM cell's order, (acc + b_ih) + b_hh; everything after them
// is fp64.
struct GcQuad {
    float act[4][4];  // r, z, n, a
    float hn[4];
};

template <int H = kLcH>
__device__ __forceinline__ void gc_pointwise(const f32x16& cr, const f32x16& cz, const f32x16& cnx, const f32x16& cnh,
                                             int qd, const float* b_ih, const float* b_hh, int n, const float (&hp)[4],
                                             GcQuad& q) {
    float pre[4][4];  // r, z, the x side of n, a
#pragma unroll
    for (int g = 0; g < 3; ++g) {
        float bi[4], bh[4];
        gc_unpack(*reinterpret_cast<const float4*>(b_ih + g * H + n), bi);
        gc_unpack(*reinterpret_cast<const float4*>(b_hh + g * H + n), bh);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int k = 4 * qd + e;
            if (g == 0) pre[0][e] = (cr[k] + bi[e]) + bh[e];
            if (g == 1) pre[1][e] = (cz[k] + bi[e]) + bh[e];
            if (g == 2) {
                pre[2][e] = cnx[k] + bi[e];
                pre[3][e] = cnh[k] + bh[e];
            }
        }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const double r = lc_sigmoid(static_cast<double>(pre[0][e]));
        const double z = lc_sigmoid(static_cast<double>(pre[1][e]));
        const double nn = tanh(static_cast<double>(pre[2][e]) + r * static_cast<double>(pre[3][e]));
        q.hn[e] = static_cast<float>((1.0 - z) * nn + z * static_cast<double>(hp[e]));
        q.act[0][e] = static_cast<float>(r);
        q.act[1][e] = static_cast<float>(z);
        q.act[2][e] = static_cast<float>(nn);
        q.act[3][e] = pre[3][e];
    }
}

__global__ __launch_bounds__(kBlock, 2) void gru_cell_kernel(GcArgs args) {
    const GcProblem& P = args.p[blockIdx.z];
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int hh = lane >> 5;
    const int l32 = lane & 31;
    const int64_t row0 = static_cast<int64_t>(blockIdx.x) * kLcRows;
    const int n0 = 128 * blockIdx.y + 32 * wave;
    const int kc_x = P.D / 16;
    const int kc_h = P.h ? kGcHChunks : 0;  // h == null: its chunks contribute nothing
    const int gate_units = (kc_x + kGcHChunks) * kLcChunkU;
    // weight fragment of image row n = n0 + l32, logical half hh (physical half swapped when (n >> 3) & 1)
    const int wunit = (n0 + l32) * 2 + (hh ^ ((l32 >> 3) & 1));

    f32x16 ar[2] = {f32x16{}, f32x16{}}, az[2] = {f32x16{}, f32x16{}};
    f32x16 anx[2] = {f32x16{}, f32x16{}}, anh[2] = {f32x16{}, f32x16{}};

    for (int c = 0; c < kc_x; ++c) {
        bf16x8 xf[2][3];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const float* src = P.x + (row0 + 32 * i + l32) * P.D + 16 * c + 8 * hh;
            lc_split8(*reinterpret_cast<const float4*>(src), *reinterpret_cast<const float4*>(src + 4), xf[i]);
        }
        gc_chunk(P.image + c * kLcChunkU + wunit, gate_units, xf, ar, az, anx);
    }
    for (int c = 0; c < kc_h; ++c) {
        bf16x8 xf[2][3];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const float* src = P.h + (row0 + 32 * i + l32) * kLcH + 16 * c + 8 * hh;
            lc_split8(*reinterpret_cast<const float4*>(src), *reinterpret_cast<const float4*>(src + 4), xf[i]);
        }
        gc_chunk(P.image + (kc_x + c) * kLcChunkU + wunit, gate_units, xf, ar, az, anh);
    }

    // the cell update, register-local: 4 column quads per row block; the lane reads its own h elements for the blend
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int64_t r = row0 + 32 * i + l32;
#pragma unroll
        for (int qd = 0; qd < 4; ++qd) {
            const int n = n0 + 8 * qd + 4 * hh;
            float hp[4] = {0.f, 0.f, 0.f, 0.f};
            if (P.h) gc_unpack(*reinterpret_cast<const float4*>(P.h + r * kLcH + n), hp);
            GcQuad q;
            gc_pointwise(ar[i], az[i], anx[i], anh[i], qd, P.b_ih, P.b_hh, n, hp, q);
            *reinterpret_cast<float4*>(P.h_out + r * kLcH + n) = make_float4(q.hn[0], q.hn[1], q.hn[2], q.hn[3]);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------
// The training form of the step (rslrl_gru_cell_train): the same tile, loops and pointwise part as gru_cell_kernel --
// h' carries its bits -- plus a `reset` vector applied on read, before the split (a row whose flag is set reads its h
// from h_restart, null: zero), the h as consumed (h_in_out, null: not stored) and the gate-major [4][M][256] tensor
// r, z, n, a of every element, which the lane that owns the element already holds.  a is the biased h-side
// pre-activation of n: d n / d r, and what d r's chain multiplies.
// Every wave of a workgroup reads all 16 chunks of the 64 rows' h; wave w of column half y stores the two chunks
// 8 y + 2 w, + 1 -- its own 32 columns -- from the registers it has just loaded (the LSTM kernel's ownership rule), so
// the two workgroups of a row tile write disjoint 128-column halves with plain vector stores.
struct GtProblem {
    GcProblem p;
    float* gates;
    const unsigned char* reset;  // [M] or null
    int64_t gate_stride;
    const float* h_restart;      // [M, 256] or null
    float* h_in_out;             // [M, 256] or null
};

struct GtArgs {
    GtProblem p[2];
};

__global__ __launch_bounds__(kBlock, 2) void gru_cell_train_kernel(GtArgs args) {
    const GtProblem& T = args.p[blockIdx.z];
    const GcProblem& P = T.p;
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int hh = lane >> 5;
    const int l32 = lane & 31;
    const int64_t row0 = static_cast<int64_t>(blockIdx.x) * kLcRows;
    const int n0 = 128 * blockIdx.y + 32 * wave;
    const int kc_x = P.D / 16;
    // h == null and nothing to restart from or to store: its chunks contribute nothing
    const bool h_chunks = P.h || T.h_in_out || (T.reset && T.h_restart);
    const int kc_h = h_chunks ? kGcHChunks : 0;
    const int gate_units = (kc_x + kGcHChunks) * kLcChunkU;
    const int wunit = (n0 + l32) * 2 + (hh ^ ((l32 >> 3) & 1));
    const int store_c0 = 8 * blockIdx.y + 2 * wave;  // the first of this wave's two chunks of h_in_out
    bool rst[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) rst[i] = T.reset && T.reset[row0 + 32 * i + l32] != 0;

    f32x16 ar[2] = {f32x16{}, f32x16{}}, az[2] = {f32x16{}, f32x16{}};
    f32x16 anx[2] = {f32x16{}, f32x16{}}, anh[2] = {f32x16{}, f32x16{}};

    for (int c = 0; c < kc_x; ++c) {
        bf16x8 xf[2][3];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const float* src = P.x + (row0 + 32 * i + l32) * P.D + 16 * c + 8 * hh;
            lc_split8(*reinterpret_cast<const float4*>(src), *reinterpret_cast<const float4*>(src + 4), xf[i]);
        }
        gc_chunk(P.image + c * kLcChunkU + wunit, gate_units, xf, ar, az, anx);
    }
    for (int c = 0; c < kc_h; ++c) {
        bf16x8 xf[2][3];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const float* state = rst[i] ? T.h_restart : P.h;
            const int64_t at = (row0 + 32 * i + l32) * kLcH + 16 * c + 8 * hh;
            float4 lo = make_float4(0.f, 0.f, 0.f, 0.f), hi = lo;
            if (state) {
                lo = *reinterpret_cast<const float4*>(state + at);
                hi = *reinterpret_cast<const float4*>(state + at + 4);
            }
            if (T.h_in_out && (c == store_c0 || c == store_c0 + 1)) {
                *reinterpret_cast<float4*>(T.h_in_out + at) = lo;
                *reinterpret_cast<float4*>(T.h_in_out + at + 4) = hi;
            }
            lc_split8(lo, hi, xf[i]);
        }
        gc_chunk(P.image + (kc_x + c) * kLcChunkU + wunit, gate_units, xf, ar, az, anh);
    }

#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int64_t r = row0 + 32 * i + l32;
#pragma unroll
        for (int qd = 0; qd < 4; ++qd) {
            const int n = n0 + 8 * qd + 4 * hh;
            float hp[4] = {0.f, 0.f, 0.f, 0.f};
            const float* state = rst[i] ? T.h_restart : P.h;
            if (state) gc_unpack(*reinterpret_cast<const float4*>(state + r * kLcH + n), hp);
            GcQuad q;
            gc_pointwise(ar[i], az[i], anx[i], anh[i], qd, P.b_ih, P.b_hh, n, hp, q);
            *reinterpret_cast<float4*>(P.h_out + r * kLcH + n) = make_float4(q.hn[0], q.hn[1], q.hn[2], q.hn[3]);
#pragma unroll
            for (int g = 0; g < 4; ++g)
                *reinterpret_cast<float4*>(T.gates + g * T.gate_stride + r * kLcH + n) =
                    make_float4(q.act[g][0], q.act[g][1], q.act[g][2], q.act[g][3]);
        }
    }
}

// One reverse step (rslrl_gru_cell_bwd).  The recurrent term [dg_next.r | dg_next.z | dg_next.a] W_hh is an x6 GEMM of
// K = 768 (blocks 0, 1 and 3 of dg_next, 48 chunks of 16) onto 256 columns, from the layout-0 image of W_hh^T (256
// rows, depth 768); the forward's tile with one 64 x 32 accumulator per wave, summed by lc_mfma's per-chunk rule.
//   dh~ = dh + (reset_next ? 0 : dhz_next + that),   dn = dh~ (1 - z) (1 - n^2)
//   dg.r = dn a r (1 - r)   dg.z = dh~ (h_in - n) z (1 - z)   dg.n = dn   dg.a = dn r   dhz = dh~ z
// h_in is the stored h as consumed, so a restart needs no pointer of its own here.  The derivative is register-local
// and runs in fp64, rounded once per stored value; every output element is written by exactly one lane.
struct GbProblem {
    const float* dh;                  // [M, 256]
    const float* dg_next;             // gate-major r, z, n, a of the next step, or null
    const float* dhz_next;            // [M, 256] or null
    const unsigned char* reset_next;  // [M] or null: rows reset between this step and the next
    const float* gates;               // gate-major r, z, n, a of this step
    const float* h_in;                // [M, 256]: the h this step consumed
    const uint4* whh_t;               // image of W_hh^T
    float* dg;                        // gate-major out
    float* dhz_out;                   // [M, 256] out
    int64_t gate_stride;              // of gates and dg
    int64_t next_stride;              // of dg_next
};

struct GbArgs {
    GbProblem p[2];
};

template <int H>
__global__ __launch_bounds__(kBlock) void gru_cell_bwd_kernel(GbArgs args) {
    const GbProblem& P = args.p[blockIdx.z];
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
    constexpr int kSh = H == 512 ? 5 : 4;  // log2 of a gate block's chunks
    static_assert(H / 16 == 1 << kSh, "hidden size");
    bool rn[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) rn[i] = P.reset_next && P.reset_next[row0 + 32 * i + l32] != 0;
    f32x16 acc[2] = {f32x16{}, f32x16{}};
    if (P.dg_next) {
        for (int c = 0; c < 3 * (H / 16); ++c) {
            const int blk = c >> kSh;  // image block 0, 1, 2 = dg_next block r, z, a
            bf16x8 xf[2][3];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const float* src = P.dg_next + (blk == 2 ? 3 : blk) * P.next_stride + (row0 + 32 * i + l32) * H +
                                   16 * (c & (H / 16 - 1)) + 8 * hh;
                lc_split8(*reinterpret_cast<const float4*>(src), *reinterpret_cast<const float4*>(src + 4), xf[i]);
            }
            bf16x8 wf[3];
            const uint4* img = P.whh_t + c * kLcChunkU + wunit;
            if constexpr (H > kLcBlockRows)
                img = P.whh_t + (blk * (H / kLcBlockRows) * (H / 16) + (c & (H / 16 - 1))) * kLcChunkU + wunit;
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
            float dha[4], dza[4] = {0.f, 0.f, 0.f, 0.f}, hia[4], ga[4][4];
            gc_unpack(*reinterpret_cast<const float4*>(P.dh + at), dha);
            if (P.dhz_next && !rn[i]) gc_unpack(*reinterpret_cast<const float4*>(P.dhz_next + at), dza);
            gc_unpack(*reinterpret_cast<const float4*>(P.h_in + at), hia);
#pragma unroll
            for (int g = 0; g < 4; ++g) gc_unpack(*reinterpret_cast<const float4*>(P.gates + g * P.gate_stride + at), ga[g]);
            float out[4][4], dhz[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float rec = rn[i] ? 0.0f : acc[i][4 * qd + e];
                const double dht = static_cast<double>(dha[e]) + (static_cast<double>(dza[e]) + static_cast<double>(rec));
                const double gr = ga[0][e], gz = ga[1][e], gn = ga[2][e], gate_a = ga[3][e];
                const double dn = dht * (1.0 - gz) * (1.0 - gn * gn);
                out[0][e] = static_cast<float>(dn * gate_a * gr * (1.0 - gr));
                out[1][e] = static_cast<float>(dht * (static_cast<double>(hia[e]) - gn) * gz * (1.0 - gz));
                out[2][e] = static_cast<float>(dn);
                out[3][e] = static_cast<float>(dn * gr);
                dhz[e] = static_cast<float>(dht * gz);
            }
#pragma unroll
            for (int g = 0; g < 4; ++g)
                *reinterpret_cast<float4*>(P.dg + g * P.gate_stride + at) =
                    make_float4(out[g][0], out[g][1], out[g][2], out[g][3]);
            *reinterpret_cast<float4*>(P.dhz_out + at) = make_float4(dhz[0], dhz[1], dhz[2], dhz[3]);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------
// ABI 31: the forward forms for any input width 1 <= D <= 1024 (rslrl_gru_cell_anyd and its pair / training forms).
// Tile, gate images, gc_chunk and gc_pointwise are the kernels' above; the x side is K = ceil(D / 16) chunks deep: the
// loop over the D / 16 whole chunks, the one partial chunk peeled out of it (rnn_cell_anyd.h holds the two load forms,
// XL), then the loop over the chunks of h.  A masked element is an exact zero and the image is zero beyond column D,
// so h', the gates and h_in_out equal, bit for bit, the kernels above on the problem zero-padded to 16 K columns
// (tests/test_gpu_rnn_anyd.py).  TRAIN: gru_cell_train_kernel's extras.
__device__ __forceinline__ const GcProblem& gc_cell_of(const GcProblem& p) { return p; }
__device__ __forceinline__ const GcProblem& gc_cell_of(const GtProblem& t) { return t.p; }

template <int XL, bool TRAIN, int H>
__global__ __launch_bounds__(kBlock, 2) void gru_cell_anyd_kernel(std::conditional_t<TRAIN, GtArgs, GcArgs> args) {
    const auto& T = args.p[blockIdx.z];
    const GcProblem& P = gc_cell_of(T);
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
    const int kc_h = h_chunks ? H / 16 : 0;
    // one image block holds 256 rows of a gate: H / 256 consecutive blocks per gate, this wave's is n0 / 256
    const int block_units = (kc_x + H / 16) * kLcChunkU;
    const int gate_units = (H / kLcBlockRows) * block_units;
    const uint4* img = P.image + (n0 + l32) * 2 + (hh ^ ((l32 >> 3) & 1));
    if constexpr (H > kLcBlockRows)
        img = P.image + (n0 / kLcBlockRows) * block_units + ((n0 % kLcBlockRows) + l32) * 2 + (hh ^ ((l32 >> 3) & 1));
    const int store_c0 = 8 * blockIdx.y + 2 * wave;  // the first of this wave's two chunks of h_in_out
    bool rst[2] = {false, false};
    if constexpr (TRAIN) {
#pragma unroll
        for (int i = 0; i < 2; ++i) rst[i] = T.reset && T.reset[row0 + 32 * i + l32] != 0;
    }

    f32x16 ar[2] = {f32x16{}, f32x16{}}, az[2] = {f32x16{}, f32x16{}};
    f32x16 anx[2] = {f32x16{}, f32x16{}}, anh[2] = {f32x16{}, f32x16{}};

    for (int c = 0; c < kc_whole; ++c) {
        bf16x8 xf[2][3];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            float4 lo, hi;
            xl_load_whole<XL>(P.x + (row0 + 32 * i + l32) * P.D, 16 * c + 8 * hh, lo, hi);
            lc_split8(lo, hi, xf[i]);
        }
        gc_chunk(img + c * kLcChunkU, gate_units, xf, ar, az, anx);
    }
    if (kc_whole < kc_x) {
        bf16x8 xf[2][3];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            float4 lo, hi;
            xl_load_tail<XL>(P.x + (row0 + 32 * i + l32) * P.D, 16 * kc_whole + 8 * hh, P.D, lo, hi);
            lc_split8(lo, hi, xf[i]);
        }
        gc_chunk(img + kc_whole * kLcChunkU, gate_units, xf, ar, az, anx);
    }
    for (int c = 0; c < kc_h; ++c) {
        bf16x8 xf[2][3];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int64_t at = (row0 + 32 * i + l32) * H + 16 * c + 8 * hh;
            const float* state = P.h;
            if constexpr (TRAIN) state = rst[i] ? T.h_restart : P.h;
            float4 lo = make_float4(0.f, 0.f, 0.f, 0.f), hi = lo;
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
            lc_split8(lo, hi, xf[i]);
        }
        gc_chunk(img + (kc_x + c) * kLcChunkU, gate_units, xf, ar, az, anh);
    }

#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int64_t r = row0 + 32 * i + l32;
#pragma unroll
        for (int qd = 0; qd < 4; ++qd) {
            const int n = n0 + 8 * qd + 4 * hh;
            float hp[4] = {0.f, 0.f, 0.f, 0.f};
            const float* state = P.h;
            if constexpr (TRAIN) state = rst[i] ? T.h_restart : P.h;
            if (state) gc_unpack(*reinterpret_cast<const float4*>(state + r * H + n), hp);
            GcQuad q;
            gc_pointwise<H>(ar[i], az[i], anx[i], anh[i], qd, P.b_ih, P.b_hh, n, hp, q);
            *reinterpret_cast<float4*>(P.h_out + r * H + n) = make_float4(q.hn[0], q.hn[1], q.hn[2], q.hn[3]);
            if constexpr (TRAIN) {
#pragma unroll
                for (int g = 0; g < 4; ++g)
                    *reinterpret_cast<float4*>(T.gates + g * T.gate_stride + r * H + n) =
                        make_float4(q.act[g][0], q.act[g][1], q.act[g][2], q.act[g][3]);
            }
        }
    }
}

bool gc_width_ok(int32_t D) { return D >= 16 && D <= 256 && D % 16 == 0; }

bool gc_rows_ok(int64_t M) { return M >= kLcRows && M % kLcRows == 0 && M <= (INT64_C(1) << 31); }

// anyd: the scope of the ABI 31 forms -- any 1 <= D <= 1024, x's base 4-byte aligned where D % 4 != 0
int gc_check(const rslrl_gru_cell_t* a, int64_t M, bool anyd = false, int hidden = kLcH) {
    if (!a) return RSLRL_E_INVALID_ARGUMENT;
    const bool width_ok = anyd ? anyd_width_ok(a->D) : gc_width_ok(a->D);
    if (a->hidden != hidden || a->layers != 1 || !width_ok || !gc_rows_ok(M)) return RSLRL_E_UNSUPPORTED;
    if (!a->x || !a->image || !a->b_ih || !a->b_hh || !a->h_out) return RSLRL_E_INVALID_ARGUMENT;
    // every block reads whole rows of h while others write h_out: they must not be one buffer
    if (a->h_out == a->h) return RSLRL_E_INVALID_ARGUMENT;
    const uintptr_t ptrs[] = {reinterpret_cast<uintptr_t>(a->h),    reinterpret_cast<uintptr_t>(a->image),
                              reinterpret_cast<uintptr_t>(a->b_ih), reinterpret_cast<uintptr_t>(a->b_hh),
                              reinterpret_cast<uintptr_t>(a->h_out)};
    for (uintptr_t p : ptrs)
        if (p & 15) return RSLRL_E_MISALIGNED;
    if (anyd ? !anyd_x_aligned(a->x, a->D) : (reinterpret_cast<uintptr_t>(a->x) & 15) != 0) return RSLRL_E_MISALIGNED;
    return RSLRL_OK;
}

GcProblem gc_problem(const rslrl_gru_cell_t* a) {
    return GcProblem{a->x, a->h, static_cast<const uint4*>(a->image), a->b_ih, a->b_hh, a->h_out, a->D};
}

int gt_problem(const rslrl_gru_train_t* a, int64_t M, GtProblem* out, bool anyd = false, int hidden = kLcH) {
    if (!a) return RSLRL_E_INVALID_ARGUMENT;
    const int rc = gc_check(&a->cell, M, anyd, hidden);
    if (rc != RSLRL_OK) return rc;
    if (!a->gates || a->gate_stride < M * hidden) return RSLRL_E_INVALID_ARGUMENT;
    // other blocks read whole rows of h and h_restart while h_out and h_in_out are written
    if (a->h_in_out && (a->h_in_out == a->cell.h || a->h_in_out == a->h_restart || a->h_in_out == a->cell.h_out))
        return RSLRL_E_INVALID_ARGUMENT;
    if (a->h_restart && a->h_restart == a->cell.h_out) return RSLRL_E_INVALID_ARGUMENT;
    if (reinterpret_cast<uintptr_t>(a->gates) & 15 || a->gate_stride % 4 ||
        reinterpret_cast<uintptr_t>(a->h_restart) & 15 || reinterpret_cast<uintptr_t>(a->h_in_out) & 15)
        return RSLRL_E_MISALIGNED;
    *out = GtProblem{gc_problem(&a->cell), a->gates, a->reset, a->gate_stride, a->h_restart, a->h_in_out};
    return RSLRL_OK;
}

int gb_problem(const rslrl_gru_bwd_t* a, int64_t M, GbProblem* out, int hidden = kLcH) {
    if (!a) return RSLRL_E_INVALID_ARGUMENT;
    if (a->hidden != hidden || a->layers != 1 || !gc_rows_ok(M)) return RSLRL_E_UNSUPPORTED;
    if (!a->dh || !a->gates || !a->h_in || !a->dg || !a->dhz_out || (a->dg_next && !a->whh_t_image))
        return RSLRL_E_INVALID_ARGUMENT;
    if (a->gate_stride < M * hidden || (a->dg_next && a->next_stride < M * hidden)) return RSLRL_E_INVALID_ARGUMENT;
    // a lane reads dhz_next and writes dhz_out at its own element only, but the GEMM reads whole rows of dg_next
    if (a->dg == a->dg_next) return RSLRL_E_INVALID_ARGUMENT;
    const uintptr_t ptrs[] = {reinterpret_cast<uintptr_t>(a->dh),          reinterpret_cast<uintptr_t>(a->dg_next),
                              reinterpret_cast<uintptr_t>(a->dhz_next),    reinterpret_cast<uintptr_t>(a->gates),
                              reinterpret_cast<uintptr_t>(a->h_in),        reinterpret_cast<uintptr_t>(a->whh_t_image),
                              reinterpret_cast<uintptr_t>(a->dg),          reinterpret_cast<uintptr_t>(a->dhz_out)};
    for (uintptr_t p : ptrs)
        if (p & 15) return RSLRL_E_MISALIGNED;
    if (a->gate_stride % 4 || a->next_stride % 4) return RSLRL_E_MISALIGNED;
    *out = GbProblem{a->dh, a->dg_next, a->dhz_next, a->reset_next, a->gates, a->h_in,
                     static_cast<const uint4*>(a->whh_t_image), a->dg, a->dhz_out, a->gate_stride, a->next_stride};
    return RSLRL_OK;
}

// H / 128 column slabs of 128 in grid.y
dim3 gc_grid(int64_t M, unsigned problems, int hidden = kLcH) {
    return dim3(static_cast<unsigned>(M / kLcRows), static_cast<unsigned>(hidden / 128), problems);
}

}  // namespace
}  // namespace rslrl

using namespace rslrl;

extern "C" size_t rslrl_gru_image_bytes(int32_t D) {
    if (!gc_width_ok(D)) return 0;
    return 3 * rslrl_linear_bimage_bytes(D + kLcH);
}

extern "C" int rslrl_gru_prepare_image(const float* w_ih, const float* w_hh, int32_t D, int32_t hidden, void* image,
                                       rslrl_stream_t stream) {
    if (hidden != kLcH || !gc_width_ok(D)) return RSLRL_E_UNSUPPORTED;
    if (!w_ih || !w_hh || !image) return RSLRL_E_INVALID_ARGUMENT;
    if (reinterpret_cast<uintptr_t>(image) & 15) return RSLRL_E_MISALIGNED;
    const size_t gate_bytes = rslrl_linear_bimage_bytes(D + kLcH);
    const size_t x_bytes = rslrl_linear_bimage_bytes(D);
    rslrl_bimage_desc_t d[6];
    for (int g = 0; g < 3; ++g) {
        char* base = static_cast<char*>(image) + g * gate_bytes;
        d[2 * g] = rslrl_bimage_desc_t{w_ih + static_cast<int64_t>(g) * kLcH * D, base, kLcH, D, 0,
                                       RSLRL_BIMAGE_LAYOUT_GEMM};
        d[2 * g + 1] = rslrl_bimage_desc_t{w_hh + static_cast<int64_t>(g) * kLcH * kLcH, base + x_bytes, kLcH, kLcH, 0,
                                           RSLRL_BIMAGE_LAYOUT_GEMM};
    }
    return rslrl_linear_prepare_bimages(d, 6, stream);
}

extern "C" int rslrl_gru_cell_pair(const rslrl_gru_cell_t* a0, const rslrl_gru_cell_t* a1, int64_t M,
                                   rslrl_stream_t stream) {
    int rc = gc_check(a0, M);
    if (rc != RSLRL_OK) return rc;
    GcArgs args{};
    args.p[0] = gc_problem(a0);
    unsigned np = 1;
    if (a1) {
        rc = gc_check(a1, M);
        if (rc != RSLRL_OK) return rc;
        args.p[1] = gc_problem(a1);
        np = 2;
    }
    hipLaunchKernelGGL(gru_cell_kernel, gc_grid(M, np), dim3(kBlock), 0, reinterpret_cast<hipStream_t>(stream), args);
    return launch_status();
}

extern "C" int rslrl_gru_cell(const rslrl_gru_cell_t* a, int64_t M, rslrl_stream_t stream) {
    return rslrl_gru_cell_pair(a, nullptr, M, stream);
}

extern "C" int rslrl_gru_cell_train_pair(const rslrl_gru_train_t* a0, const rslrl_gru_train_t* a1, int64_t M,
                                         rslrl_stream_t stream) {
    GtArgs args{};
    int rc = gt_problem(a0, M, &args.p[0]);
    if (rc != RSLRL_OK) return rc;
    unsigned np = 1;
    if (a1) {
        rc = gt_problem(a1, M, &args.p[1]);
        if (rc != RSLRL_OK) return rc;
        np = 2;
    }
    hipLaunchKernelGGL(gru_cell_train_kernel, gc_grid(M, np), dim3(kBlock), 0, reinterpret_cast<hipStream_t>(stream),
                       args);
    return launch_status();
}

extern "C" int rslrl_gru_cell_train(const rslrl_gru_train_t* a, int64_t M, rslrl_stream_t stream) {
    return rslrl_gru_cell_train_pair(a, nullptr, M, stream);
}

extern "C" size_t rslrl_gru_whh_t_image_bytes(void) { return rslrl_linear_bimage_bytes(3 * kLcH); }

extern "C" int rslrl_gru_prepare_whh_t_image(const float* w_hh, int32_t hidden, void* image, rslrl_stream_t stream) {
    if (hidden != kLcH) return RSLRL_E_UNSUPPORTED;
    if (!w_hh || !image) return RSLRL_E_INVALID_ARGUMENT;
    if (reinterpret_cast<uintptr_t>(image) & 15) return RSLRL_E_MISALIGNED;
    return rslrl_linear_prepare_bimage(w_hh, kLcH, 3 * kLcH, 1, image, stream);  // B[n][k] = W_hh[k][n]
}

extern "C" int rslrl_gru_cell_bwd_pair(const rslrl_gru_bwd_t* a0, const rslrl_gru_bwd_t* a1, int64_t M,
                                       rslrl_stream_t stream) {
    GbArgs args{};
    int rc = gb_problem(a0, M, &args.p[0]);
    if (rc != RSLRL_OK) return rc;
    unsigned np = 1;
    if (a1) {
        rc = gb_problem(a1, M, &args.p[1]);
        if (rc != RSLRL_OK) return rc;
        np = 2;
    }
    hipLaunchKernelGGL(gru_cell_bwd_kernel<kLcH>, gc_grid(M, np), dim3(kBlock), 0, reinterpret_cast<hipStream_t>(stream),
                       args);
    return launch_status();
}

extern "C" int rslrl_gru_cell_bwd(const rslrl_gru_bwd_t* a, int64_t M, rslrl_stream_t stream) {
    return rslrl_gru_cell_bwd_pair(a, nullptr, M, stream);
}

// ---- ABI 31: any input width (the kernels and scope are described at gru_cell_anyd_kernel)
extern "C" size_t rslrl_gru_image_bytes_anyd(int32_t D) {
    if (!anyd_width_ok(D)) return 0;
    return 3 * (rslrl_linear_bimage_bytes(D) + rslrl_linear_bimage_bytes(kLcH));
}

extern "C" int rslrl_gru_prepare_image_anyd(const float* w_ih, const float* w_hh, int32_t D, int32_t hidden,
                                            void* image, rslrl_stream_t stream) {
    if (hidden != kLcH || !anyd_width_ok(D)) return RSLRL_E_UNSUPPORTED;
    if (!w_ih || !w_hh || !image) return RSLRL_E_INVALID_ARGUMENT;
    if (reinterpret_cast<uintptr_t>(image) & 15) return RSLRL_E_MISALIGNED;
    const size_t x_bytes = rslrl_linear_bimage_bytes(D);  // ceil(D / 16) chunks, zero from column D on
    const size_t gate_bytes = x_bytes + rslrl_linear_bimage_bytes(kLcH);
    rslrl_bimage_desc_t d[6];
    for (int g = 0; g < 3; ++g) {
        char* base = static_cast<char*>(image) + g * gate_bytes;
        d[2 * g] = rslrl_bimage_desc_t{w_ih + static_cast<int64_t>(g) * kLcH * D, base, kLcH, D, 0,
                                       RSLRL_BIMAGE_LAYOUT_GEMM};
        d[2 * g + 1] = rslrl_bimage_desc_t{w_hh + static_cast<int64_t>(g) * kLcH * kLcH, base + x_bytes, kLcH, kLcH, 0,
                                           RSLRL_BIMAGE_LAYOUT_GEMM};
    }
    return rslrl_linear_prepare_bimages(d, 6, stream);
}

namespace {

// one launch reads both problems with one load form: the ragged one as soon as either width is no multiple of 4
template <bool TRAIN, int H = kLcH, typename Args>
int gc_launch_anyd(const Args& args, int d0, int d1, unsigned np, int64_t M, rslrl_stream_t stream) {
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (d0 % 4 || d1 % 4)
        hipLaunchKernelGGL((gru_cell_anyd_kernel<kXlRagged, TRAIN, H>), gc_grid(M, np, H), dim3(kBlock), 0, st, args);
    else
        hipLaunchKernelGGL((gru_cell_anyd_kernel<kXlQuad, TRAIN, H>), gc_grid(M, np, H), dim3(kBlock), 0, st, args);
    return launch_status();
}

}  // namespace

extern "C" int rslrl_gru_cell_pair_anyd(const rslrl_gru_cell_t* a0, const rslrl_gru_cell_t* a1, int64_t M,
                                        rslrl_stream_t stream) {
    int rc = gc_check(a0, M, true);
    if (rc != RSLRL_OK) return rc;
    GcArgs args{};
    args.p[0] = gc_problem(a0);
    if (a1) {
        rc = gc_check(a1, M, true);
        if (rc != RSLRL_OK) return rc;
        args.p[1] = gc_problem(a1);
    }
    return gc_launch_anyd<false>(args, a0->D, a1 ? a1->D : 0, a1 ? 2 : 1, M, stream);
}

extern "C" int rslrl_gru_cell_anyd(const rslrl_gru_cell_t* a, int64_t M, rslrl_stream_t stream) {
    return rslrl_gru_cell_pair_anyd(a, nullptr, M, stream);
}

extern "C" int rslrl_gru_cell_train_pair_anyd(const rslrl_gru_train_t* a0, const rslrl_gru_train_t* a1, int64_t M,
                                              rslrl_stream_t stream) {
    GtArgs args{};
    int rc = gt_problem(a0, M, &args.p[0], true);
    if (rc != RSLRL_OK) return rc;
    if (a1) {
        rc = gt_problem(a1, M, &args.p[1], true);
        if (rc != RSLRL_OK) return rc;
    }
    return gc_launch_anyd<true>(args, a0->cell.D, a1 ? a1->cell.D : 0, a1 ? 2 : 1, M, stream);
}

extern "C" int rslrl_gru_cell_train_anyd(const rslrl_gru_train_t* a, int64_t M, rslrl_stream_t stream) {
    return rslrl_gru_cell_train_pair_anyd(a, nullptr, M, stream);
}

// ---- The `_h` forms: hidden size 512 (additions to ABI 34; the kernels are the H = 512 instantiations of
// gru_cell_anyd_kernel and gru_cell_bwd_kernel, the scope is the `_anyd` forms' with hidden == 512).  A gate's weights
// are two 256-row block images, each the x part (depth D) followed by the h part (depth 512); W_hh^T is, per gate block
// r, z, n of W_hh, two 256-row images of depth 512.
extern "C" size_t rslrl_gru_image_bytes_h(int32_t D, int32_t hidden) {
    if (hidden != kLcHWide || !anyd_width_ok(D)) return 0;
    return 3 * (kLcHWide / kLcBlockRows) * (rslrl_linear_bimage_bytes(D) + rslrl_linear_bimage_bytes(kLcHWide));
}

extern "C" int rslrl_gru_prepare_image_h(const float* w_ih, const float* w_hh, int32_t D, int32_t hidden, void* image,
                                         rslrl_stream_t stream) {
    if (hidden != kLcHWide || !anyd_width_ok(D)) return RSLRL_E_UNSUPPORTED;
    if (!w_ih || !w_hh || !image) return RSLRL_E_INVALID_ARGUMENT;
    if (reinterpret_cast<uintptr_t>(image) & 15) return RSLRL_E_MISALIGNED;
    const size_t x_bytes = rslrl_linear_bimage_bytes(D);
    const size_t block_bytes = x_bytes + rslrl_linear_bimage_bytes(kLcHWide);
    rslrl_bimage_desc_t d[12];
    for (int gb = 0; gb < 6; ++gb) {  // image block gb = 2 gate + block: rows 256 gb .. of W_ih and W_hh
        char* base = static_cast<char*>(image) + gb * block_bytes;
        const int64_t row = static_cast<int64_t>(gb) * kLcBlockRows;
        d[2 * gb] = rslrl_bimage_desc_t{w_ih + row * D, base, kLcBlockRows, D, 0, RSLRL_BIMAGE_LAYOUT_GEMM};
        d[2 * gb + 1] = rslrl_bimage_desc_t{w_hh + row * kLcHWide, base + x_bytes, kLcBlockRows, kLcHWide, 0,
                                            RSLRL_BIMAGE_LAYOUT_GEMM};
    }
    return rslrl_linear_prepare_bimages(d, 12, stream);
}

extern "C" int rslrl_gru_cell_pair_h(const rslrl_gru_cell_t* a0, const rslrl_gru_cell_t* a1, int64_t M,
                                     rslrl_stream_t stream) {
    int rc = gc_check(a0, M, true, kLcHWide);
    if (rc != RSLRL_OK) return rc;
    GcArgs args{};
    args.p[0] = gc_problem(a0);
    if (a1) {
        rc = gc_check(a1, M, true, kLcHWide);
        if (rc != RSLRL_OK) return rc;
        args.p[1] = gc_problem(a1);
    }
    return gc_launch_anyd<false, kLcHWide>(args, a0->D, a1 ? a1->D : 0, a1 ? 2 : 1, M, stream);
}

extern "C" int rslrl_gru_cell_h(const rslrl_gru_cell_t* a, int64_t M, rslrl_stream_t stream) {
    return rslrl_gru_cell_pair_h(a, nullptr, M, stream);
}

extern "C" int rslrl_gru_cell_train_pair_h(const rslrl_gru_train_t* a0, const rslrl_gru_train_t* a1, int64_t M,
                                           rslrl_stream_t stream) {
    GtArgs args{};
    int rc = gt_problem(a0, M, &args.p[0], true, kLcHWide);
    if (rc != RSLRL_OK) return rc;
    if (a1) {
        rc = gt_problem(a1, M, &args.p[1], true, kLcHWide);
        if (rc != RSLRL_OK) return rc;
    }
    return gc_launch_anyd<true, kLcHWide>(args, a0->cell.D, a1 ? a1->cell.D : 0, a1 ? 2 : 1, M, stream);
}

extern "C" int rslrl_gru_cell_train_h(const rslrl_gru_train_t* a, int64_t M, rslrl_stream_t stream) {
    return rslrl_gru_cell_train_pair_h(a, nullptr, M, stream);
}

extern "C" size_t rslrl_gru_whh_t_image_bytes_h(int32_t hidden) {
    if (hidden != kLcHWide) return 0;
    return 3 * rslrl_linear_bimage_wide_bytes(kLcHWide, kLcHWide);
}

extern "C" int rslrl_gru_prepare_whh_t_image_h(const float* w_hh, int32_t hidden, void* image, rslrl_stream_t stream) {
    if (hidden != kLcHWide) return RSLRL_E_UNSUPPORTED;
    if (!w_hh || !image) return RSLRL_E_INVALID_ARGUMENT;
    if (reinterpret_cast<uintptr_t>(image) & 15) return RSLRL_E_MISALIGNED;
    const size_t gate_bytes = rslrl_linear_bimage_wide_bytes(kLcHWide, kLcHWide);
    for (int g = 0; g < 3; ++g) {  // B[n][k] = W_hh[512 g + k][n]: the two 256-row blocks of n, each 512 deep
        const int rc = rslrl_linear_prepare_bimage_wide(w_hh + static_cast<int64_t>(g) * kLcHWide * kLcHWide, kLcHWide,
                                                        kLcHWide, 1, static_cast<char*>(image) + g * gate_bytes, stream);
        if (rc != RSLRL_OK) return rc;
    }
    return RSLRL_OK;
}

extern "C" int rslrl_gru_cell_bwd_pair_h(const rslrl_gru_bwd_t* a0, const rslrl_gru_bwd_t* a1, int64_t M,
                                         rslrl_stream_t stream) {
    GbArgs args{};
    int rc = gb_problem(a0, M, &args.p[0], kLcHWide);
    if (rc != RSLRL_OK) return rc;
    unsigned np = 1;
    if (a1) {
        rc = gb_problem(a1, M, &args.p[1], kLcHWide);
        if (rc != RSLRL_OK) return rc;
        np = 2;
    }
    hipLaunchKernelGGL(gru_cell_bwd_kernel<kLcHWide>, gc_grid(M, np, kLcHWide), dim3(kBlock), 0,
                       reinterpret_cast<hipStream_t>(stream), args);
    return launch_status();
}

extern "C" int rslrl_gru_cell_bwd_h(const rslrl_gru_bwd_t* a, int64_t M, rslrl_stream_t stream) {
    return rslrl_gru_cell_bwd_pair_h(a, nullptr, M, stream);
}
