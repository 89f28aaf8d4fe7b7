// The x side of [x | h] for an input width D that is no multiple of 16 (the `_anyd` forms of lstm_cell.hip and
// gru_cell.hip, ABI 31): K = ceil(D / 16) chunks of x, of which the first D / 16 are whole and at most one -- the
// last -- is partial.  The kernels peel the partial chunk out of their loop, so the loop over whole chunks has no
// mask in it; the weight images are zero beyond column D (bimage_kernel), and a masked element of x enters the split
// as an exact zero, so every MFMA sees the operands of the problem zero-padded to 16 K columns.
//
// Two load forms (a template parameter of the kernels, wave-uniform per launch):
//   kXlQuad    D % 4 == 0: rows are 16-byte aligned; whole chunks take two 16-byte loads, the partial chunk's quads
//              are whole or absent -- an absent quad reads the row's first four floats and is zeroed by a select
//   kXlRagged  any D: rows are 4-byte aligned only; whole chunks take two dwordx4 loads at 4-byte-aligned addresses,
//              the partial chunk goes through load4_ragged / load4_ragged_short (ragged_load.h): the row's last quad
//              reads the row's last four floats and rotates them, rows shorter than four floats load per element
// No load touches a byte outside its own row of x.
#pragma once

#include "ragged_load.h"
#include "rnn_cell.h"

namespace rslrl {
namespace {

constexpr int kXlQuad = 1;
constexpr int kXlRagged = 2;
constexpr int kAnydMaxD = 1024;

// floats col .. col + 7 of a whole chunk (col + 8 <= D)
template <int XL>
__device__ __forceinline__ void xl_load_whole(const float* __restrict__ row, int col, float4& lo, float4& hi) {
    if constexpr (XL == kXlRagged) {
        const f32x4 a = *reinterpret_cast<const f32x4_a4*>(row + col);
        const f32x4 b = *reinterpret_cast<const f32x4_a4*>(row + col + 4);
        lo = make_float4(a[0], a[1], a[2], a[3]);
        hi = make_float4(b[0], b[1], b[2], b[3]);
    } else {
        lo = *reinterpret_cast<const float4*>(row + col);
        hi = *reinterpret_cast<const float4*>(row + col + 4);
    }
}

// floats col .. col + 7 of the partial chunk: zero from column D on
template <int XL>
__device__ __forceinline__ void xl_load_tail(const float* __restrict__ row, int col, int D, float4& lo, float4& hi) {
    if constexpr (XL == kXlRagged) {
        const bool wide = D >= 4;
        lo = load4_ragged_any(row, col, D, wide, true);
        hi = load4_ragged_any(row, col + 4, D, wide, true);
    } else {
        const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
        const bool ok_lo = col < D, ok_hi = col + 4 < D;  // D % 4 == 0 (so D >= 4): a quad is whole or absent
        const float4 a = *reinterpret_cast<const float4*>(row + (ok_lo ? col : 0));
        const float4 b = *reinterpret_cast<const float4*>(row + (ok_hi ? col + 4 : 0));
        lo = ok_lo ? a : zero;
        hi = ok_hi ? b : zero;
    }
}

inline bool anyd_width_ok(int32_t D) { return D >= 1 && D <= kAnydMaxD; }

// x's base: 16 bytes where the rows are read with 16-byte loads, 4 bytes otherwise
inline bool anyd_x_aligned(const float* x, int32_t D) {
    return (reinterpret_cast<uintptr_t>(x) & (D % 4 ? 3 : 15)) == 0;
}

__host__ __device__ __forceinline__ int anyd_x_chunks(int32_t D) { return (D + 15) / 16; }

}  // namespace
}  // namespace rslrl
