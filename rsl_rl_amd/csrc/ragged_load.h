// Operand loads from rows whose stride is no multiple of 4 floats (an observation 235 floats wide): the row bases are
// 4-byte aligned only, and the last k-quad of a row has 1..3 elements.  Used by the ragged instantiations of the A-stage
// loader (mlp_gemm_x6.h load_a) and of the weight gradient's load_tile (mlp_wgrad_x6.h), both in mlp_ragged.hip.
//
// A quad is one 16-byte load at a 4-byte-aligned address (global memory takes dword-aligned wide loads on gfx9 and
// later; the compiler keeps it one global_load_dwordx4).  The last quad of a row reads the row's LAST four floats
// instead -- the address moves back by 4 - (elements left), never past the row's end -- and the wanted elements are
// rotated to the front by selects; the others enter the split as zeros, the zeros of the padded problem.  A lane that
// has nothing to load (row past the matrix, quad past the row) reads the same last four floats of a valid row and
// is zeroed: no control flow in the load stream, as load4_masked.  Rows shorter than four floats take one dword
// load per element, each clamped to the row's first float.
#pragma once

#include "common.h"
#include "x6_split.h"

namespace rslrl {
namespace {

typedef f32x4 f32x4_a4 __attribute__((aligned(4)));

// Elements c .. c + 3 (c % 4 == 0) of the row at `row`, zero where c + e >= ncols or !ok.  `row` must be a valid row
// even when !ok.  `back`: floats in front of `row` that belong to the same row (a column block of a wider row: the
// block's first column); needs ncols + back >= 4.  Reads only inside [row - back, row + ncols).
__device__ __forceinline__ float4 load4_ragged(const float* __restrict__ row, int c, int ncols, bool ok) {
    const bool any = ok && c < ncols;
    const int last = ncols - 4;                         // >= -back
    const int cc = any ? (c < last ? c : last) : last;  // a whole quad: c; the row's tail: its last four floats
    const f32x4 v = *reinterpret_cast<const f32x4_a4*>(row + cc);
    const int s = c - cc;                               // 0, or 4 - (elements left) in 1..3
    float4 r;
    r.x = s == 0 ? v[0] : (s == 1 ? v[1] : (s == 2 ? v[2] : v[3]));
    r.y = s == 0 ? v[1] : (s == 1 ? v[2] : (s == 2 ? v[3] : 0.f));
    r.z = s == 0 ? v[2] : (s == 1 ? v[3] : 0.f);
    r.w = s == 0 ? v[3] : 0.f;
    return any ? r : make_float4(0.f, 0.f, 0.f, 0.f);
}

// The same for a row of fewer than four floats (ncols in 1..3, nothing in front of it): per-element loads.
__device__ __forceinline__ float4 load4_ragged_short(const float* __restrict__ row, int c, int ncols, bool ok) {
    float e[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const bool in = ok && c + i < ncols;
        const float t = row[in ? c + i : 0];
        e[i] = in ? t : 0.f;
    }
    return make_float4(e[0], e[1], e[2], e[3]);
}

// wide: ncols + back >= 4 (wave-uniform)
__device__ __forceinline__ float4 load4_ragged_any(const float* __restrict__ row, int c, int ncols, bool wide, bool ok) {
    return wide ? load4_ragged(row, c, ncols, ok) : load4_ragged_short(row, c, ncols, ok);
}

}  // namespace
}  // namespace rslrl
