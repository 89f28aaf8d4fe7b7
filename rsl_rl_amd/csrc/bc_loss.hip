// Behaviour-cloning loss forward + backward for a window of stored steps on gfx950 (ABI 24).
//
// Replaces, for S stored steps of one optimizer window, rsl_rl/algorithms/distillation.py:120-123 (one
// mse_loss / huber_loss per step, summed over the window) and the backward of :130 down to the student's
// output: step_loss[s] = mean over step s's N * A elements of l(pred - target), grad = d(sum_s step_loss[s]) /
// d pred = l'(d) / (N * A).  The reference evaluates this as one loss launch, one add and one host read-back per
// step plus S chained backward graphs.
//
// Memory-bound: per element 4 B pred + 4 B target read, 4 B grad written = 12 B (8 B forward only).
//
// Work split: workgroups never straddle a step -- step s is covered by `bps` workgroups (blockIdx.x = s * bps + b).
// A step's N * A elements are handled as quads of four consecutive elements; quad q belongs to thread
// (q % (bps * 256)) and a thread adds its quads' four terms in element order into one fp64 sum.  Every access form
// below (16-byte, scalar, strided rows) keeps that assignment, so the summation order -- and with it every bit of
// step_loss -- does not depend on alignment, strides or on whether the gradient is written.  Cross-lane sums are
// fp64 butterflies, workgroup partials are folded in a fixed order by the step's last-arriving workgroup (an
// arrival ticket per step that the call leaves zero): no floating-point atomics, bitwise reproducible.

#include <algorithm>

#include "common.h"

namespace rslrl {
namespace {

constexpr int kMaxBps = 64;            // workgroups per step: the last one folds <= 64 partials with one wave
constexpr int kQuadsPerThread = 4;     // a step gets another workgroup per 4 quads (64 B per stream) per thread
// Per-step workspace record: [arrival ticket (8 B)][kMaxBps fp64 partials].  Its size does not depend on N or A, so a
// ticket never shares bytes with another call's partials whatever shapes the calls on one workspace have.
constexpr int kRecordDoubles = 1 + kMaxBps;

struct BcParams {
    int64_t S, N;
    int32_t A;
    int32_t huber;
    const float* pred;
    int64_t pred_stride;
    const float* target;
    float* step_loss;
    float* grad;  // may be null: forward only
    int64_t grad_stride;
    int32_t bps;
    float g_scale;    // mse: 2 / (N A); huber: 1 / (N A)
    double count;     // N A
};

__device__ __forceinline__ void bc_term(float p, float t, bool huber, float g_scale, float& loss, float& g) {
    const float d = p - t;
    if (huber) {  // torch's huber_loss, delta = 1: 0.5 d^2 inside, |d| - 0.5 outside; gradient d / sign(d)
        const float ad = fabsf(d);
        const bool in = ad < 1.0f;
        loss = in ? 0.5f * d * d : ad - 0.5f;
        g = in ? g_scale * d : (d < 0.0f ? -g_scale : g_scale);
    } else {
        loss = d * d;
        g = g_scale * d;
    }
}

__device__ __forceinline__ bool aligned16_dev(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// One workgroup = one slice of one step's quads.  `flat`: pred (and grad) rows are dense, so a step is one run of
// N * A consecutive floats; otherwise rows are addressed by their strides.
__global__ __launch_bounds__(kBlock) void bc_loss_kernel(BcParams p, double* __restrict__ records) {
    __shared__ double wave_part[kBlock / kWave];
    __shared__ int last_block;
    const int bps = p.bps;
    const int64_t s = blockIdx.x / bps;
    const int b = blockIdx.x - static_cast<int>(s) * bps;
    const int A = p.A;
    const int64_t count = p.N * A;            // elements of a step
    const int64_t nq = (count + 3) >> 2;      // quads of a step (the last one may be partial)
    const int64_t full_q = count >> 2;        // quads with all four elements
    const bool huber = p.huber != 0;
    const bool want_grad = p.grad != nullptr;
    const bool flat = p.pred_stride == A && (!want_grad || p.grad_stride == A);
    const int64_t row0 = s * p.N;

    double acc = 0.0;
    const int64_t qstride = static_cast<int64_t>(bps) * kBlock;
    const int64_t q0 = static_cast<int64_t>(b) * kBlock + threadIdx.x;
    if (flat) {
        const float* __restrict__ ps = p.pred + row0 * A;
        const float* __restrict__ ts = p.target + row0 * A;
        float* __restrict__ gs = want_grad ? p.grad + row0 * A : nullptr;
        // 16-byte accesses when this step starts 16-byte aligned in every operand (workgroup-uniform)
        const bool vec = aligned16_dev(ps) && aligned16_dev(ts) && (!want_grad || aligned16_dev(gs));
#pragma unroll 2
        for (int64_t q = q0; q < nq; q += qstride) {
            const int64_t e = q << 2;
            float pv[4], tv[4], l[4], g[4];
            const bool whole = q < full_q;
            if (vec && whole) {
                const float4 a = *reinterpret_cast<const float4*>(ps + e);
                const float4 c = *reinterpret_cast<const float4*>(ts + e);
                pv[0] = a.x, pv[1] = a.y, pv[2] = a.z, pv[3] = a.w;
                tv[0] = c.x, tv[1] = c.y, tv[2] = c.z, tv[3] = c.w;
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const bool ok = e + k < count;
                    pv[k] = ok ? ps[e + k] : 0.0f;
                    tv[k] = ok ? ts[e + k] : 0.0f;
                }
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                bc_term(pv[k], tv[k], huber, p.g_scale, l[k], g[k]);
                if (whole || e + k < count) acc += static_cast<double>(l[k]);
            }
            if (want_grad) {
                if (vec && whole) {
                    *reinterpret_cast<float4*>(gs + e) = make_float4(g[0], g[1], g[2], g[3]);
                } else {
#pragma unroll
                    for (int k = 0; k < 4; ++k)
                        if (e + k < count) gs[e + k] = g[k];
                }
            }
        }
    } else {
        // strided rows (a padded or sliced pred, a gradient padded to a multiple of four columns): element e of the
        // step is column e % A of row e / A; the thread that holds a row's last column zeroes the row's pad columns
        const int64_t pstr = p.pred_stride, gstr = p.grad_stride;
        const float* __restrict__ ts = p.target + row0 * A;
        for (int64_t q = q0; q < nq; q += qstride) {
            const int64_t e = q << 2;
            int64_t r = e / A;
            int c = static_cast<int>(e - r * A);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (e + k < count) {
                    float l, g;
                    bc_term(p.pred[(row0 + r) * pstr + c], ts[e + k], huber, p.g_scale, l, g);
                    acc += static_cast<double>(l);
                    if (want_grad) {
                        float* grow = p.grad + (row0 + r) * gstr;
                        grow[c] = g;
                        if (c == A - 1)
                            for (int64_t z = A; z < gstr; ++z) grow[z] = 0.0f;
                    }
                }
                if (++c == A) {
                    c = 0;
                    ++r;
                }
            }
        }
    }

    // ---- workgroup partial: wave butterfly, then waves in order
    const int lane = threadIdx.x & (kWave - 1);
    const int wid = threadIdx.x / kWave;
    const double wsum = wave_sum(acc);
    if (lane == 0) wave_part[wid] = wsum;
    __syncthreads();
    unsigned* ticket = reinterpret_cast<unsigned*>(records + s * kRecordDoubles);
    double* step_part = records + s * kRecordDoubles + 1;
    if (threadIdx.x == 0) {
        double v = wave_part[0];
#pragma unroll
        for (int w = 1; w < kBlock / kWave; ++w) v += wave_part[w];
        if (bps == 1) {  // the only workgroup of its step: nothing to hand over
            p.step_loss[s] = static_cast<float>(v / p.count);
            last_block = 0;
        } else {
            // the partial is stored write-through (an 8-byte agent-scope atomic store), drained, then the ticket is
            // taken: the last arriver acquires once and reads every partial past its L1 (as ppo_loss.hip)
            __hip_atomic_store(reinterpret_cast<unsigned long long*>(step_part + b), __double_as_longlong(v),
                               __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            const unsigned t = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const int last = (t == static_cast<unsigned>(bps) - 1);
            if (last) {
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            }
            last_block = last;
        }
    }
    __syncthreads();
    if (!last_block || wid != 0) return;
    // fixed-order fold by one wave: lane r holds partial r (bps <= 64), fp64 butterfly
    double v = 0.0;
    if (lane < bps) {
        const unsigned long long bits = __hip_atomic_load(reinterpret_cast<unsigned long long*>(step_part + lane),
                                                          __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        v = __longlong_as_double(bits);
    }
    v = wave_sum(v);
    if (lane == 0) {
        p.step_loss[s] = static_cast<float>(v / p.count);
        __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // re-arm (stream-ordered)
    }
}

int bc_blocks_per_step(int64_t N, int32_t A) {
    const int64_t nq = (N * A + 3) / 4;
    return static_cast<int>(std::max<int64_t>(1, std::min<int64_t>(ceil_div(nq, kBlock * kQuadsPerThread), kMaxBps)));
}

}  // namespace
}  // namespace rslrl

using namespace rslrl;

// workspace layout: one record per step (kRecordDoubles fp64 words)
extern "C" size_t rslrl_bc_loss_workspace_bytes(int64_t S, int64_t N, int32_t A) {
    (void)N;
    (void)A;
    return sizeof(double) * kRecordDoubles * static_cast<size_t>(S > 0 ? S : 0);
}

extern "C" int rslrl_bc_loss_fwd_bwd(const rslrl_bc_loss_args_t* a, void* workspace, size_t workspace_bytes,
                                     rslrl_stream_t stream) {
    if (!a) return RSLRL_E_INVALID_ARGUMENT;
    if (a->S < 0 || a->N < 1 || a->A < 1 || a->A > RSLRL_PPO_LOSS_MAX_ACTIONS) return RSLRL_E_INVALID_ARGUMENT;
    if (a->loss_type != RSLRL_BC_LOSS_MSE && a->loss_type != RSLRL_BC_LOSS_HUBER) return RSLRL_E_INVALID_ARGUMENT;
    if (a->S == 0) return RSLRL_OK;
    if (!a->pred || !a->target || !a->step_loss) return RSLRL_E_INVALID_ARGUMENT;
    if (a->pred_stride < a->A) return RSLRL_E_INVALID_ARGUMENT;
    if (a->grad && a->grad_stride != a->A && a->grad_stride != (a->A + 3) / 4 * 4) return RSLRL_E_INVALID_ARGUMENT;
    const int bps = bc_blocks_per_step(a->N, a->A);
    if (a->S * bps > (int64_t{1} << 30)) return RSLRL_E_UNSUPPORTED;
    if (!workspace) return RSLRL_E_INVALID_ARGUMENT;
    if (workspace_bytes < rslrl_bc_loss_workspace_bytes(a->S, a->N, a->A)) return RSLRL_E_WORKSPACE_TOO_SMALL;
    if (reinterpret_cast<uintptr_t>(workspace) & 15) return RSLRL_E_MISALIGNED;

    BcParams p{};
    p.S = a->S;
    p.N = a->N;
    p.A = a->A;
    p.huber = a->loss_type == RSLRL_BC_LOSS_HUBER ? 1 : 0;
    p.pred = a->pred;
    p.pred_stride = a->pred_stride;
    p.target = a->target;
    p.step_loss = a->step_loss;
    p.grad = a->grad;
    p.grad_stride = a->grad ? a->grad_stride : a->A;
    p.bps = bps;
    const double count = static_cast<double>(a->N) * static_cast<double>(a->A);
    p.g_scale = static_cast<float>((p.huber ? 1.0 : 2.0) / count);
    p.count = count;
    hipLaunchKernelGGL(bc_loss_kernel, dim3(static_cast<unsigned>(a->S * bps)), dim3(kBlock), 0,
                       reinterpret_cast<hipStream_t>(stream), p, static_cast<double*>(workspace));
    return launch_status();
}
