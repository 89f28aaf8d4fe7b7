// Distillation step record (ABI 32): one launch for RolloutStorage.add_transitions of a distillation storage
// (rsl_rl/storage/rollout_storage.py:77-103 with training_type "distillation"):
//
//   storage[t] <- obs groups [N, w], actions [N, A], privileged_actions [N, A], rewards [N] -> [N, 1],
//                 uint8(dones) [N, 1]
//
// instead of one copy launch per observation group plus four (distillation runs long rollouts: T launches of each).
// Pure data movement.  Every source and every destination row t is a contiguous [N, w] slab, so workgroup b moves
// rows [kRows b, kRows b + kRows) of every field: w kRows consecutive floats per slab, read and written by
// consecutive lanes (coalesced).  A workgroup's part of a slab starts kRows b w floats into it -- a multiple of 64 bytes
// for any w -- so wherever both bases are 16-byte aligned it moves in 16-byte units: all of it for a width that is a
// multiple of 4 (the caller's 16-byte claim), and for any other width (45, 235, 7: dword units in the ABI's terms) the
// aligned quads of the part with its last 1-3 floats as dwords, which only the last, partial workgroup has (kRows w
// is a multiple of 4).  Bases that are not 16-byte aligned move in dwords throughout.  No LDS, no atomics; the loads
// of a pass are issued before its stores.
#include "common.h"

namespace rslrl {
namespace {

constexpr int kRows = 16;   // rows per workgroup: 256 workgroups at 4,096 envs
constexpr int kPass = 4;    // units in flight per thread
constexpr int kSlabs = RSLRL_ROLLOUT_MAX_OBS + 2;  // obs groups, actions, privileged actions

struct Slab {
    const float* src;
    float* dst;
    int32_t w;      // row floats
    int32_t vec16;  // both bases 16-byte aligned: 16-byte units (and a dword tail where rows * w % 4 != 0)
};
struct DistillParams {
    Slab slab[kSlabs];
    int32_t n_slabs;
    int32_t dones_dtype;
    int64_t N;
    const float* rewards;
    const void* dones;
    float* out_rewards;
    uint8_t* out_dones;
};

template <typename U>
__device__ __forceinline__ void copy_units(const U* __restrict__ s, U* __restrict__ d, int count) {
    for (int i0 = threadIdx.x; i0 < count; i0 += kPass * kBlock) {
        U v[kPass];
#pragma unroll
        for (int j = 0; j < kPass; ++j) {
            const int i = i0 + j * kBlock;
            if (i < count) v[j] = s[i];
        }
#pragma unroll
        for (int j = 0; j < kPass; ++j) {
            const int i = i0 + j * kBlock;
            if (i < count) d[i] = v[j];
        }
    }
}

// dones as torch's copy_ into the uint8 buffer converts them (rollout_storage.py:88): a cast of the value, so the
// 0 / 1 flags of every dtype -- and any other value a uint8 holds -- arrive as add_transitions stores them
__device__ __forceinline__ uint8_t flag_u8(const void* p, int dtype, int64_t i) {
    switch (dtype) {
        case RSLRL_DTYPE_U8: return static_cast<const uint8_t*>(p)[i];
        case RSLRL_DTYPE_I32: return static_cast<uint8_t>(static_cast<const int32_t*>(p)[i]);
        case RSLRL_DTYPE_I64: return static_cast<uint8_t>(static_cast<const int64_t*>(p)[i]);
        default: return static_cast<uint8_t>(static_cast<const float*>(p)[i]);
    }
}

__global__ __launch_bounds__(kBlock) void distill_record_kernel(DistillParams p) {
    const int64_t n0 = static_cast<int64_t>(blockIdx.x) * kRows;
    const int rows = static_cast<int>(min<int64_t>(kRows, p.N - n0));  // >= 1: the grid is ceil(N / kRows)
    for (int g = 0; g < p.n_slabs; ++g) {
        const Slab& sl = p.slab[g];
        const int64_t off = n0 * sl.w;   // floats; n0 is a multiple of kRows = 16: a multiple of 64 bytes
        const int floats = rows * sl.w;  // <= 16 * 2^26: checked on the host
        if (sl.vec16) {
            const int quads = floats >> 2;
            copy_units(reinterpret_cast<const float4*>(sl.src + off), reinterpret_cast<float4*>(sl.dst + off), quads);
            const int i = 4 * quads + static_cast<int>(threadIdx.x);  // the last partial workgroup's 0-3 floats
            if (i < floats) sl.dst[off + i] = sl.src[off + i];
        } else {
            copy_units(sl.src + off, sl.dst + off, floats);
        }
    }
    if (static_cast<int>(threadIdx.x) < rows) {
        const int64_t n = n0 + threadIdx.x;
        p.out_rewards[n] = p.rewards[n];
        p.out_dones[n] = flag_u8(p.dones, p.dones_dtype, n);
    }
}

inline bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

}  // namespace
}  // namespace rslrl

using namespace rslrl;

extern "C" int rslrl_distill_record(const rslrl_distill_record_args_t* args, rslrl_stream_t stream) {
    if (!args) return RSLRL_E_INVALID_ARGUMENT;
    const rslrl_distill_record_args_t& a = *args;
    if (a.N < 0 || a.A < 1 || a.n_obs < 0 || a.n_obs > RSLRL_ROLLOUT_MAX_OBS) return RSLRL_E_INVALID_ARGUMENT;
    if (a.dones_dtype < RSLRL_DTYPE_F32 || a.dones_dtype > RSLRL_DTYPE_I64) return RSLRL_E_INVALID_ARGUMENT;
    constexpr int64_t kMaxRowFloats = int64_t{1} << 26;  // kRows rows of a slab stay inside an int
    if (a.A > kMaxRowFloats) return RSLRL_E_INVALID_ARGUMENT;
    for (int g = 0; g < a.n_obs; ++g) {
        const rslrl_distill_obs_t& o = a.obs[g];
        if (o.row_floats < 1 || o.row_floats > kMaxRowFloats || (o.unit_bytes != 4 && o.unit_bytes != 16))
            return RSLRL_E_INVALID_ARGUMENT;
        if (o.unit_bytes == 16 && (o.row_floats & 3)) return RSLRL_E_INVALID_ARGUMENT;
    }
    if (a.N == 0) return RSLRL_OK;
    if (!a.actions || !a.privileged_actions || !a.rewards || !a.dones || !a.out_actions || !a.out_privileged_actions ||
        !a.out_rewards || !a.out_dones)
        return RSLRL_E_INVALID_ARGUMENT;
    for (int g = 0; g < a.n_obs; ++g)
        if (!a.obs[g].src || !a.obs[g].dst) return RSLRL_E_INVALID_ARGUMENT;
    if (ceil_div(a.N, kRows) > INT32_MAX) return RSLRL_E_INVALID_ARGUMENT;

    DistillParams p{};
    for (int g = 0; g < a.n_obs; ++g) {
        const rslrl_distill_obs_t& o = a.obs[g];
        const uintptr_t al = static_cast<uintptr_t>(o.unit_bytes);
        if (!aligned(o.src, al) || !aligned(o.dst, al)) return RSLRL_E_MISALIGNED;
        p.slab[p.n_slabs++] = Slab{o.src, o.dst, static_cast<int32_t>(o.row_floats), aligned(o.src, 16) && aligned(o.dst, 16)};
    }
    if (!aligned(a.actions, 4) || !aligned(a.privileged_actions, 4) || !aligned(a.out_actions, 4) ||
        !aligned(a.out_privileged_actions, 4) || !aligned(a.rewards, 4) || !aligned(a.out_rewards, 4))
        return RSLRL_E_MISALIGNED;
    const size_t flag_bytes = a.dones_dtype == RSLRL_DTYPE_U8 ? 1 : a.dones_dtype == RSLRL_DTYPE_I64 ? 8 : 4;
    if (!aligned(a.dones, flag_bytes)) return RSLRL_E_MISALIGNED;
    const int vec_a = aligned(a.actions, 16) && aligned(a.out_actions, 16);
    const int vec_p = aligned(a.privileged_actions, 16) && aligned(a.out_privileged_actions, 16);
    p.slab[p.n_slabs++] = Slab{a.actions, a.out_actions, a.A, vec_a};
    p.slab[p.n_slabs++] = Slab{a.privileged_actions, a.out_privileged_actions, a.A, vec_p};
    p.dones_dtype = a.dones_dtype;
    p.N = a.N;
    p.rewards = a.rewards;
    p.dones = a.dones;
    p.out_rewards = a.out_rewards;
    p.out_dones = a.out_dones;
    hipLaunchKernelGGL(distill_record_kernel, dim3(static_cast<unsigned>(ceil_div(a.N, kRows))), dim3(kBlock), 0,
                       reinterpret_cast<hipStream_t>(stream), p);
    return launch_status();
}
