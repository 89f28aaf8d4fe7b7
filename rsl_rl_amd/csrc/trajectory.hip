// Trajectory bookkeeping of recurrent PPO on gfx950 (ABI 25): rsl_rl/utils/utils.py:78-141
// (split_and_pad_trajectories, unpad_trajectories) and the hidden-state gather of
// rsl_rl/storage/rollout_storage.py:206-260, as index arithmetic instead of nonzero / split / pad_sequence /
// boolean indexing.
//
// rslrl_trajectory_index  dones [T, N] -> for every (t, n) the global trajectory number j (trajectories numbered
//                         env-major, then by time: the reference's order after its transpose and flatten) and the
//                         offset s inside that trajectory; the exclusive prefix of trajectory counts per env; the
//                         num_mini_batches + 1 trajectory boundaries of the env slices (what the host reads, once).
//                         Two launches: per-block trajectory counts, then the walk -- a block sums the counts of the
//                         blocks before it (<= 512 integers at N = 131,072), so no block assumes it is the only one.
// rslrl_trajectory_pad    one launch for <= 4 observation groups (strided rows read in place), the bool masks and the
//                         gather of <= 4 saved state tensors at trajectory starts.  Each mini-batch's padded slice is
//                         its own contiguous [T, n_b, D] block (nn.LSTM wants contiguous input); padded positions are
//                         zeroed by memsets this entry point issues before the launch.  Rows are copied in 16-byte
//                         units where widths, strides and pointers allow, a thread keeping its column unit.
// rslrl_trajectory_unpad  out[t, e] = padded[s(t, e), j(t, e) - first] (gather) or its transpose (scatter: the
//                         backward; padded positions receive the memset's 0).  A valid (s, j) belongs to exactly one
//                         (t, e): no atomics in either direction.
// Pure data movement, integer bookkeeping: bit-identical to the reference and run to run.

#include "common.h"

namespace rslrl {
namespace {

__device__ __forceinline__ bool traj_done(const uint8_t* dones, int64_t T, int64_t N, int64_t t, int64_t n) {
    return t == T - 1 || dones[t * N + n] != 0;  // utils.py:97-98: the last step closes a trajectory
}

// trajectories of the 256 envs of block b
__global__ __launch_bounds__(kBlock) void trajectory_count_kernel(const uint8_t* dones, int64_t T, int64_t N,
                                                                  int32_t* block_counts) {
    __shared__ int32_t scratch[kBlock / kWave];
    const int64_t n = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
    int32_t c = 0;
    if (n < N)
        for (int64_t t = 0; t < T; ++t) c += traj_done(dones, T, N, t, n) ? 1 : 0;
    const int32_t total = block_sum(c, scratch);
    if (threadIdx.x == 0) block_counts[blockIdx.x] = total;
}

struct TrajIndexParams {
    const uint8_t* dones;
    int64_t T, N;
    const int32_t* block_counts;
    int32_t* traj_id;
    int32_t* traj_off;
    int32_t* env_prefix;  // [N + 1]
    int32_t* bounds;      // [num_mini_batches + 1]
    int64_t num_mini_batches;
    int64_t mb_envs;
};

__global__ __launch_bounds__(kBlock) void trajectory_walk_kernel(TrajIndexParams p) {
    __shared__ int32_t scratch[kBlock / kWave];
    __shared__ int32_t scan[kBlock];
    // trajectories of all envs before this block
    int32_t before = 0;
    for (unsigned b = threadIdx.x; b < blockIdx.x; b += kBlock) before += p.block_counts[b];
    before = block_sum(before, scratch);
    const int64_t n = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
    int32_t c = 0;
    if (n < p.N)
        for (int64_t t = 0; t < p.T; ++t) c += traj_done(p.dones, p.T, p.N, t, n) ? 1 : 0;
    // inclusive scan of the block's counts
    scan[threadIdx.x] = c;
    __syncthreads();
    for (int off = 1; off < kBlock; off <<= 1) {
        const int32_t add = threadIdx.x >= static_cast<unsigned>(off) ? scan[threadIdx.x - off] : 0;
        __syncthreads();
        scan[threadIdx.x] += add;
        __syncthreads();
    }
    if (n >= p.N) return;
    const int32_t first = before + scan[threadIdx.x] - c;
    p.env_prefix[n] = first;
    if (n == p.N - 1) p.env_prefix[p.N] = first + c;
    if (p.mb_envs > 0 && n % p.mb_envs == 0 && n / p.mb_envs <= p.num_mini_batches) p.bounds[n / p.mb_envs] = first;
    if (n == p.N - 1 && p.num_mini_batches * p.mb_envs == p.N) p.bounds[p.num_mini_batches] = first + c;
    int32_t j = first, s = 0;
    for (int64_t t = 0; t < p.T; ++t) {
        p.traj_id[t * p.N + n] = j;
        p.traj_off[t * p.N + n] = s;
        if (traj_done(p.dones, p.T, p.N, t, n)) {
            ++j;
            s = 0;
        } else {
            ++s;
        }
    }
}

constexpr int kPadTileRows = 32;  // (t, n) rows per block

struct PadGroup {
    const float* src;
    int64_t src_stride;
    float* dst;
    int32_t width;
    int32_t vec;  // 16-byte copies: width % 4 == 0, stride % 4 == 0, both pointers 16-byte aligned
};

struct PadState {
    const float* src;  // [T, L, N, H]
    float* dst;        // per mini-batch [L, n_b, H] at float offset L * bounds[b] * H
};

struct TrajPadParams {
    int64_t T, N;
    int64_t envs;  // num_mini_batches * mb_envs: envs beyond are dropped
    int64_t mb_envs;
    int64_t n_traj;
    const int32_t* traj_id;
    const int32_t* traj_off;
    const int32_t* bounds;
    PadGroup g[RSLRL_TRAJECTORY_MAX_GROUPS];
    int32_t ng;
    uint8_t* masks;
    PadState st[RSLRL_TRAJECTORY_MAX_STATES];
    int32_t ns;
    int32_t L, H;
};

__global__ __launch_bounds__(kBlock) void trajectory_pad_kernel(TrajPadParams p) {
    // per row of the tile: source row t * N + n, and the destination row inside the flat padded buffer (-1: skip)
    __shared__ int64_t src_row[kPadTileRows];
    __shared__ int64_t dst_row[kPadTileRows];
    __shared__ int64_t hid_row[kPadTileRows];  // destination row l = 0 of the state gather, or -1
    __shared__ int64_t hid_nb[kPadTileRows];
    const int64_t rows = p.T * p.envs;
    const int64_t row0 = static_cast<int64_t>(blockIdx.x) * kPadTileRows;
    if (threadIdx.x < kPadTileRows) {
        const int64_t r = row0 + threadIdx.x;
        int64_t d = -1, h = -1, nbv = 0, sr = 0;
        if (r < rows) {
            const int64_t t = r / p.envs, n = r - t * p.envs;
            sr = t * p.N + n;
            const int64_t j = p.traj_id[sr], s = p.traj_off[sr];
            const int64_t b = n / p.mb_envs;
            const int64_t b0 = p.bounds[b], b1 = p.bounds[b + 1];
            // (consistent inputs always pass; anything else is skipped, never written out of range)
            if (b0 >= 0 && j >= b0 && j < b1 && b1 <= p.n_traj && s >= 0 && s < p.T) {
                nbv = b1 - b0;
                d = p.T * b0 + s * nbv + (j - b0);
                if (s == 0) h = static_cast<int64_t>(p.L) * b0 + (j - b0);
            }
        }
        src_row[threadIdx.x] = sr;
        dst_row[threadIdx.x] = d;
        hid_row[threadIdx.x] = h;
        hid_nb[threadIdx.x] = nbv;
        if (d >= 0) p.masks[d] = 1;
    }
    __syncthreads();
    for (int k = 0; k < p.ng; ++k) {
        const PadGroup g = p.g[k];
        // a thread keeps its column unit over the tile's rows (no division per element)
        const unsigned units = g.vec ? static_cast<unsigned>(g.width) >> 2 : static_cast<unsigned>(g.width);
        const unsigned lanes = min(units, static_cast<unsigned>(kBlock));
        const unsigned rows_per_pass = kBlock / lanes;
        const unsigned rsub = threadIdx.x / lanes, u0 = threadIdx.x - rsub * lanes;
        if (rsub >= rows_per_pass) continue;
        for (unsigned r = rsub; r < kPadTileRows; r += rows_per_pass) {
            const int64_t d = dst_row[r];
            if (d < 0) continue;
            const float* src = g.src + src_row[r] * g.src_stride;
            float* dst = g.dst + d * g.width;
            for (unsigned u = u0; u < units; u += lanes) {
                if (g.vec)
                    reinterpret_cast<float4*>(dst)[u] = reinterpret_cast<const float4*>(src)[u];
                else
                    dst[u] = src[u];
            }
        }
    }
    if (p.ns == 0) return;
    // the saved states at trajectory starts: a wave per row at a time, lanes over the row's L * H floats
    const unsigned H = static_cast<unsigned>(p.H);
    const unsigned wave = threadIdx.x / kWave, lane = threadIdx.x % kWave;
    for (unsigned r = wave; r < kPadTileRows; r += kBlock / kWave) {
        const int64_t h = hid_row[r];
        if (h < 0) continue;
        const int64_t sr = src_row[r];
        const int64_t t = sr / p.N, n = sr - t * p.N;
        const int64_t nb = hid_nb[r];
        for (int q = 0; q < p.ns; ++q) {
            const PadState st = p.st[q];
            for (unsigned l = 0; l < static_cast<unsigned>(p.L); ++l) {
                const float* src = st.src + ((t * p.L + l) * p.N + n) * H;
                float* dst = st.dst + (h + static_cast<int64_t>(l) * nb) * H;
                for (unsigned c = lane; c < H; c += kWave) dst[c] = src[c];
            }
        }
    }
}

struct TrajUnpadParams {
    float* padded;  // [T, n_b, H]
    float* flat;    // [T, E, H]
    const int32_t* traj_id;
    const int32_t* traj_off;
    int64_t T, N, E, env0, first, n_b;
    int32_t H;
    int32_t scatter;
};

__global__ __launch_bounds__(kBlock) void trajectory_unpad_kernel(TrajUnpadParams p) {
    __shared__ int64_t pad_row[kPadTileRows];
    const int64_t rows = p.T * p.E;
    const int64_t row0 = static_cast<int64_t>(blockIdx.x) * kPadTileRows;
    if (threadIdx.x < kPadTileRows) {
        const int64_t r = row0 + threadIdx.x;
        int64_t d = -1;
        if (r < rows) {
            const int64_t t = r / p.E, e = r - t * p.E;
            const int64_t i = t * p.N + p.env0 + e;
            const int64_t j = static_cast<int64_t>(p.traj_id[i]) - p.first, s = p.traj_off[i];
            if (j >= 0 && j < p.n_b && s >= 0 && s < p.T) d = s * p.n_b + j;
        }
        pad_row[threadIdx.x] = d;
    }
    __syncthreads();
    const unsigned H = static_cast<unsigned>(p.H);
    for (unsigned e = threadIdx.x; e < kPadTileRows * H; e += kBlock) {
        const unsigned r = e / H, c = e - r * H;
        if (row0 + r >= rows) break;
        const int64_t d = pad_row[r];
        float* f = p.flat + (row0 + r) * H + c;
        if (p.scatter) {
            if (d >= 0) p.padded[d * H + c] = *f;
        } else {
            *f = d >= 0 ? p.padded[d * H + c] : 0.0f;
        }
    }
}

size_t index_blocks(int64_t N) { return static_cast<size_t>(ceil_div(N, kBlock)); }

}  // namespace
}  // namespace rslrl

using namespace rslrl;

extern "C" size_t rslrl_trajectory_index_workspace_bytes(int64_t T, int64_t N) {
    if (T <= 0 || N <= 0) return 0;
    return align_up(index_blocks(N) * sizeof(int32_t), 256);
}

extern "C" int rslrl_trajectory_index(const rslrl_trajectory_index_args_t* a, void* workspace, size_t workspace_bytes,
                                      rslrl_stream_t stream) {
    if (!a || !a->dones || !a->traj_id || !a->traj_off || !a->env_prefix || !a->bounds)
        return RSLRL_E_INVALID_ARGUMENT;
    if (a->T <= 0 || a->N <= 0 || a->T * a->N > INT32_MAX || a->T > INT32_MAX || a->N > INT32_MAX)
        return RSLRL_E_INVALID_ARGUMENT;
    if (a->num_mini_batches < 1 || a->num_mini_batches > a->N) return RSLRL_E_INVALID_ARGUMENT;
    if (!workspace) return RSLRL_E_INVALID_ARGUMENT;
    if (workspace_bytes < rslrl_trajectory_index_workspace_bytes(a->T, a->N)) return RSLRL_E_WORKSPACE_TOO_SMALL;
    TrajIndexParams p{};
    p.dones = a->dones;
    p.T = a->T;
    p.N = a->N;
    p.block_counts = static_cast<const int32_t*>(workspace);
    p.traj_id = a->traj_id;
    p.traj_off = a->traj_off;
    p.env_prefix = a->env_prefix;
    p.bounds = a->bounds;
    p.num_mini_batches = a->num_mini_batches;
    p.mb_envs = a->N / a->num_mini_batches;
    const unsigned nb = static_cast<unsigned>(index_blocks(a->N));
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(trajectory_count_kernel, dim3(nb), dim3(kBlock), 0, s, a->dones, a->T, a->N,
                       static_cast<int32_t*>(workspace));
    int rc = launch_status();
    if (rc != RSLRL_OK) return rc;
    hipLaunchKernelGGL(trajectory_walk_kernel, dim3(nb), dim3(kBlock), 0, s, p);
    return launch_status();
}

extern "C" int rslrl_trajectory_pad(const rslrl_trajectory_pad_args_t* a, rslrl_stream_t stream) {
    if (!a || !a->traj_id || !a->traj_off || !a->bounds || !a->masks) return RSLRL_E_INVALID_ARGUMENT;
    if (a->T <= 0 || a->N <= 0 || a->T * a->N > INT32_MAX) return RSLRL_E_INVALID_ARGUMENT;
    if (a->num_mini_batches < 1 || a->num_mini_batches > a->N) return RSLRL_E_INVALID_ARGUMENT;
    if (a->n_traj < 0 || a->n_traj > a->T * a->N) return RSLRL_E_INVALID_ARGUMENT;
    if (a->num_groups < 0 || a->num_groups > RSLRL_TRAJECTORY_MAX_GROUPS || a->num_states < 0 ||
        a->num_states > RSLRL_TRAJECTORY_MAX_STATES)
        return RSLRL_E_INVALID_ARGUMENT;
    if (a->num_states > 0 && (a->layers < 1 || a->hidden < 1 || a->layers > 64 || a->hidden > 65536))
        return RSLRL_E_INVALID_ARGUMENT;
    TrajPadParams p{};
    p.T = a->T;
    p.N = a->N;
    p.mb_envs = a->N / a->num_mini_batches;
    p.envs = p.mb_envs * a->num_mini_batches;
    p.n_traj = a->n_traj;
    p.traj_id = a->traj_id;
    p.traj_off = a->traj_off;
    p.bounds = a->bounds;
    p.masks = a->masks;
    p.ng = a->num_groups;
    p.ns = a->num_states;
    p.L = a->layers;
    p.H = a->hidden;
    for (int k = 0; k < a->num_groups; ++k) {
        const rslrl_trajectory_group_t& g = a->groups[k];
        if (!g.src || !g.dst || g.width < 1 || g.width > RSLRL_TRAJECTORY_MAX_WIDTH || g.src_stride < g.width)
            return RSLRL_E_INVALID_ARGUMENT;
        const bool vec = g.width % 4 == 0 && g.src_stride % 4 == 0 &&
                         ((reinterpret_cast<uintptr_t>(g.src) | reinterpret_cast<uintptr_t>(g.dst)) & 15) == 0;
        p.g[k] = PadGroup{g.src, g.src_stride, g.dst, g.width, vec ? 1 : 0};
    }
    for (int q = 0; q < a->num_states; ++q) {
        if (!a->state_src[q] || !a->state_dst[q]) return RSLRL_E_INVALID_ARGUMENT;
        p.st[q] = PadState{a->state_src[q], a->state_dst[q]};
    }
    if (a->n_traj == 0) return RSLRL_OK;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    // every padded position and mask: 0 (the kernel writes the valid ones)
    const size_t cells = static_cast<size_t>(a->T) * static_cast<size_t>(a->n_traj);
    hipError_t e = hipMemsetAsync(a->masks, 0, cells, s);
    for (int k = 0; k < a->num_groups && e == hipSuccess; ++k)
        e = hipMemsetAsync(a->groups[k].dst, 0, cells * a->groups[k].width * sizeof(float), s);
    if (e != hipSuccess) return static_cast<int>(e);
    const int64_t rows = p.T * p.envs;
    hipLaunchKernelGGL(trajectory_pad_kernel, dim3(static_cast<unsigned>(ceil_div(rows, kPadTileRows))), dim3(kBlock),
                       0, s, p);
    return launch_status();
}

extern "C" int rslrl_trajectory_unpad(const rslrl_trajectory_unpad_args_t* a, rslrl_stream_t stream) {
    if (!a || !a->padded || !a->flat || !a->traj_id || !a->traj_off) return RSLRL_E_INVALID_ARGUMENT;
    if (a->T <= 0 || a->N <= 0 || a->T * a->N > INT32_MAX) return RSLRL_E_INVALID_ARGUMENT;
    if (a->envs <= 0 || a->env0 < 0 || a->env0 + a->envs > a->N) return RSLRL_E_INVALID_ARGUMENT;
    if (a->first < 0 || a->n_b <= 0 || a->first + a->n_b > a->T * a->N) return RSLRL_E_INVALID_ARGUMENT;
    if (a->width < 1 || a->width > RSLRL_TRAJECTORY_MAX_WIDTH) return RSLRL_E_INVALID_ARGUMENT;
    TrajUnpadParams p{};
    p.padded = a->padded;
    p.flat = a->flat;
    p.traj_id = a->traj_id;
    p.traj_off = a->traj_off;
    p.T = a->T;
    p.N = a->N;
    p.E = a->envs;
    p.env0 = a->env0;
    p.first = a->first;
    p.n_b = a->n_b;
    p.H = a->width;
    p.scatter = a->scatter ? 1 : 0;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (p.scatter) {
        const hipError_t e = hipMemsetAsync(
            a->padded, 0, static_cast<size_t>(a->T) * static_cast<size_t>(a->n_b) * a->width * sizeof(float), s);
        if (e != hipSuccess) return static_cast<int>(e);
    }
    const int64_t rows = p.T * p.E;
    hipLaunchKernelGGL(trajectory_unpad_kernel, dim3(static_cast<unsigned>(ceil_div(rows, kPadTileRows))),
                       dim3(kBlock), 0, s, p);
    return launch_status();
}
