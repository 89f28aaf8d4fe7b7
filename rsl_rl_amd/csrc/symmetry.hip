// Signed-permutation symmetry augmentation on gfx950 (rslrl_symmetry_augment) -- the data_augmentation_func of
// rsl_rl/algorithms/ppo.py:226-234 (:323, :335) for symmetries that permute columns and flip signs (mirror left /
// right, front / back).  The torch form is, per field and augmentation, an index_select, a multiply and one cat
// over everything: 2K + 1 launches per field that read the source K times and write the result twice.
//
// Here one launch serves every field (observation groups and the actions), in the style of gather.hip: a 256-thread
// block owns a tile of source rows, stages the tile of one field in LDS with coalesced reads (16-byte units when the
// source allows it; the rows may be a strided view of a wider buffer) -- each source row is read once -- and writes
// its K signed, column-permuted copies to the contiguous [K * B, width] output, 16 bytes per lane when width % 4 == 0.
// Bytes per row and field: read 4 width, write 4 K width (+ the [K, width] tables, cache-resident).

#include <algorithm>

#include "common.h"

namespace rslrl {
namespace {

constexpr int kSymLdsFloats = 8192;  // 32 KiB of staged rows per block
constexpr int kSymTileRows = 64;     // rows per block at widths <= 128; fewer above (>= 8 at the widest field)

struct SymField {
    const float* src;
    int64_t src_stride;
    float* dst;
    int32_t width;
    int32_t src_vec;  // 16-byte source reads
    int32_t dst_vec;  // 16-byte stores
    const int32_t* perm;
    const float* sign;
};

struct SymAugParams {
    SymField f[RSLRL_SYMMETRY_MAX_FIELDS];
    int32_t nf;
    int32_t K;
    int32_t tile;  // rows per block
    int64_t B;
};

__global__ __launch_bounds__(kBlock) void symmetry_augment_kernel(SymAugParams p) {
    __shared__ __attribute__((aligned(16))) float tile[kSymLdsFloats];
    const int64_t row0 = static_cast<int64_t>(blockIdx.x) * p.tile;
    const int nrows = static_cast<int>(min<int64_t>(p.tile, p.B - row0));
    for (int f = 0; f < p.nf; ++f) {
        const SymField g = p.f[f];
        const unsigned w = static_cast<unsigned>(g.width);
        const unsigned n = static_cast<unsigned>(nrows) * w;  // <= kSymLdsFloats (host: tile * width)
        __syncthreads();  // the previous field's reads of the tile are done
        if (g.src_vec) {
            const unsigned w4 = w >> 2;
            for (unsigned q = threadIdx.x; q < (n >> 2); q += kBlock) {
                const unsigned r = q / w4, c4 = q - r * w4;
                reinterpret_cast<float4*>(tile)[q] =
                    *reinterpret_cast<const float4*>(g.src + (row0 + r) * g.src_stride + 4 * c4);
            }
        } else {
            for (unsigned e = threadIdx.x; e < n; e += kBlock) {
                const unsigned r = e / w, c = e - r * w;
                tile[e] = g.src[(row0 + r) * g.src_stride + c];
            }
        }
        __syncthreads();
        // a thread keeps its column unit (4 columns with 16-byte stores) over the tile's rows, so that unit's
        // perm / sign entries are read once per augmentation and the lanes of a pass cover whole consecutive rows
        const unsigned units = g.dst_vec ? (w >> 2) : w;
        const unsigned lanes = min(units, static_cast<unsigned>(kBlock));
        const unsigned rows_per_pass = kBlock / lanes;
        const unsigned rsub = threadIdx.x / lanes;
        const unsigned u0 = threadIdx.x - rsub * lanes;
        if (rsub >= rows_per_pass) continue;  // (the next field's first barrier is reached by every thread)
        for (int k = 0; k < p.K; ++k) {
            const int32_t* perm = g.perm ? g.perm + static_cast<int64_t>(k) * w : nullptr;
            const float* sign = g.perm ? g.sign + static_cast<int64_t>(k) * w : nullptr;
            float* dst = g.dst + (static_cast<int64_t>(k) * p.B + row0) * w;
            for (unsigned u = u0; u < units; u += lanes) {
                if (g.dst_vec) {
                    const unsigned c = 4 * u;
                    unsigned s4[4];
                    float f4[4];
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        s4[e] = perm ? min(static_cast<unsigned>(perm[c + e]), w - 1) : c + e;  // stays in the row
                        f4[e] = perm ? sign[c + e] : 1.0f;
                    }
                    for (unsigned r = rsub; r < static_cast<unsigned>(nrows); r += rows_per_pass) {
                        const float* row = tile + r * w;
                        *reinterpret_cast<float4*>(dst + r * w + c) =
                            make_float4(__fmul_rn(f4[0], row[s4[0]]), __fmul_rn(f4[1], row[s4[1]]),
                                        __fmul_rn(f4[2], row[s4[2]]), __fmul_rn(f4[3], row[s4[3]]));
                    }
                } else {
                    const unsigned sc = perm ? min(static_cast<unsigned>(perm[u]), w - 1) : u;
                    const float fs = perm ? sign[u] : 1.0f;
                    for (unsigned r = rsub; r < static_cast<unsigned>(nrows); r += rows_per_pass)
                        dst[r * w + u] = __fmul_rn(fs, tile[r * w + sc]);
                }
            }
        }
    }
}

}  // namespace
}  // namespace rslrl

using namespace rslrl;

extern "C" int rslrl_symmetry_augment(const rslrl_symmetry_field_t* fields, int32_t num_fields, int64_t B, int32_t K,
                                      rslrl_stream_t stream) {
    if (num_fields < 0 || num_fields > RSLRL_SYMMETRY_MAX_FIELDS || B < 0 || K < 1 || K > RSLRL_SYMMETRY_MAX_AUG)
        return RSLRL_E_INVALID_ARGUMENT;
    if (num_fields > 0 && !fields) return RSLRL_E_INVALID_ARGUMENT;
    SymAugParams p{};
    p.nf = num_fields;
    p.K = K;
    p.B = B;
    int max_width = 1;
    for (int i = 0; i < num_fields; ++i) {
        const rslrl_symmetry_field_t& f = fields[i];
        if (!f.src || !f.dst || f.width < 1 || f.width > RSLRL_SYMMETRY_MAX_WIDTH || f.src_stride < f.width)
            return RSLRL_E_INVALID_ARGUMENT;
        if ((f.perm == nullptr) != (f.sign == nullptr)) return RSLRL_E_INVALID_ARGUMENT;
        const bool w4 = f.width % 4 == 0;
        const bool src_vec = w4 && f.src_stride % 4 == 0 && (reinterpret_cast<uintptr_t>(f.src) & 15) == 0;
        // block k of dst starts at k * B * width floats: 16-byte aligned for every k and tile when width % 4 == 0
        const bool dst_vec = w4 && (reinterpret_cast<uintptr_t>(f.dst) & 15) == 0;
        p.f[i] = SymField{f.src, f.src_stride, f.dst, f.width, src_vec ? 1 : 0, dst_vec ? 1 : 0, f.perm, f.sign};
        max_width = std::max(max_width, f.width);
    }
    if (B == 0 || num_fields == 0) return RSLRL_OK;
    p.tile = std::min(kSymTileRows, kSymLdsFloats / max_width);
    const int64_t nb = ceil_div(B, p.tile);
    if (nb > INT32_MAX) return RSLRL_E_INVALID_ARGUMENT;
    hipLaunchKernelGGL(symmetry_augment_kernel, dim3(static_cast<unsigned>(nb)), dim3(kBlock), 0,
                       reinterpret_cast<hipStream_t>(stream), p);
    return launch_status();
}
