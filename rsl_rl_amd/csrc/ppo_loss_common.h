// The PPO loss arithmetic, written once.  Four kernels evaluate it on their own data layouts -- ppo_loss_kernel (a lane
// per sample) and ppo_loss_quad_kernel (four lanes per sample) in ppo_loss.hip, ppo_loss_sym_kernel in
// ppo_loss_sym.hip, and actor_head_epilogue in mlp_heads.hip (the loss inside the actor's last GEMM launch) -- and the
// GPU tests compare them bit for bit, so each keeps its loads, shuffles and reductions and calls these for the
// per-sample expressions (every unit is compiled with -ffp-contract=off: one expression, one bit pattern):
//   sigma_consts, InvDenForm          log sigma and the reciprocals of one sigma; the three roundings of 1 / (2 sigma^2)
//   logp_term, entropy_term,          torch.distributions.Normal log_prob / entropy of one action; the tree sum of a
//   tree_sum                          lane's log-prob terms
//   kl_term_exact, kl_fast_consts,    the adaptive-lr KL of one action: the reference's operation sequence, and the
//   kl_term_fast                      form on per-action constants of a shared sigma with its fall-back flag
//   normalize_adv, adv_den            per-mini-batch advantage normalisation
//   max_nan, clamp_nan                torch.max / torch.clamp of one term: a NaN operand gives NaN
//   surrogate, max_grads              clipped surrogate and d loss / d log-prob (torch.max's backward)
//   value_loss, value_loss_grad       clipped / plain value term and d loss / dV (also the critic heads': mlp_gemm_x6.h,
//                                     mlp_fwd_stream.hip)
//   normal_grads                      d loss / d mu, d loss / d sigma of one action
//   load_row, store_row               a lane's [A] row, 16-byte accesses when VEC
//   quad_sum, fold_columns,           the quad-lane sum and the fixed-order fold of per-block fp64 partials over the grid
//   fold_grid_partials
//   loss_scalars, kl_fast_enabled     host: the launch's scalars and the RSLRL_KL_FAST knob
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdlib>

#include "common.h"

namespace rslrl {
namespace {

constexpr float kLogSqrt2Pi = 0.91893853320467274178f;  // log(sqrt(2*pi)), normal.py log_prob
constexpr float kEntC = 1.41893853320467274178f;         // 0.5 + 0.5*log(2*pi), normal.py entropy

// torch.max(a, b) backward (derivatives.yaml, maximum): ties give each side grad / 2.
__device__ __forceinline__ void max_grads(float a, float b, float g, float& ga, float& gb) {
    const float half = __fmul_rn(g, 0.5f);
    ga = (a > b) ? g : ((a == b) ? half : 0.0f);
    gb = (b > a) ? g : ((a == b) ? half : 0.0f);
}

// torch.max / torch.clamp of the loss terms: a NaN operand gives NaN (fmaxf / fminf would drop it and report a finite
// statistic beside NaN gradients).  On ordered operands: the larger, and min(max(x, lo), hi).
__device__ __forceinline__ float max_nan(float a, float b) { return (a > b || a != a) ? a : b; }
__device__ __forceinline__ float clamp_nan(float x, float lo, float hi) {
    const float t = (x < lo) ? lo : x;
    return (t > hi) ? hi : t;
}

// 1 / (2 sigma^2) is spelled three ways today; they round differently at the extremes of sigma, so each caller's
// spelling is behaviour and stays (DESIGN 5e lists who uses which)
enum InvDenForm {
    kInvDenRn,       // 1 / (2 (s s)): every shared-sigma prologue; ppo_loss_sym_kernel's per-row sigma, both sides
    kInvDenRowLogp,  // 1 / ((2 s) s): ppo_loss.hip's per-row sigma, log-prob side
    kInvDenRowGrad,  // 0.5 (1 / s)^2: ppo_loss.hip's per-row sigma, gradient side
};

// log sigma and the reciprocals the log-prob and the gradients use (<= 2 ulp from the reference's divisions)
struct SigmaConsts {
    float s, ls, inv_den, inv_s, inv_s3;
};

__device__ __forceinline__ SigmaConsts sigma_consts(float s, InvDenForm form = kInvDenRn) {
    const float inv_s = 1.0f / s;
    // log sigma.  The device's logf is off by up to 1.85 ulp (0.67 rms) and its absolute error grows with |log sigma|:
    // at sigma in 0.03 .. 0.1 (|log sigma| ~ 3) the A errors add up in the log-prob and put the ratio, and with it every
    // gradient, at 2 to 3 times torch fp32's error against fp64 (tests/test_gpu_loss_regimes.py, regime `late`).  So
    // outside (1/2, 2) the logarithm is rounded once from fp64.  Inside, |log sigma| < 0.7 and logf's error (< 1.2e-7)
    // stays below half an ulp of a log-prob of four actions or more: logf stays, at its cost and with its bits.
    const float ls = (s > 0.5f && s < 2.0f) ? logf(s) : static_cast<float>(log(static_cast<double>(s)));
    const float inv_den = form == kInvDenRn        ? 1.0f / __fmul_rn(2.0f, __fmul_rn(s, s))
                          : form == kInvDenRowLogp ? 1.0f / (2.0f * s * s)
                                                   : 0.5f * inv_s * inv_s;
    return {s, ls, inv_den, inv_s, inv_s * inv_s * inv_s};
}

// Normal(mu, sigma).log_prob(x) of one action, d = x - mu (normal.py)
__device__ __forceinline__ float logp_term(float d, float inv_den, float ls) {
    return (-(d * d) * inv_den - ls) - kLogSqrt2Pi;
}

// The log-prob of a sample held by one lane: pairwise summation of its A (<= N) terms with a base block of four -- a
// running sum inside each block of four consecutive actions, then a binary tree over the blocks' index, an odd node
// carried up as it is.  Entries from A on count as 0, so the bits do not depend on N (the lane kernel's MAXA, the actor
// head's padded width); up to four actions it is the running sum, at 16 the quad kernel's order (four per lane, then
// quad_sum).  A running sum over all A rounds at the size of the growing partial sum each time: at 16 actions twice the
// error of this form, where it missed the fp32-class bar (tests/test_gpu_loss_regimes.py, `saturated`).
// Clobbers t.
template <int N>
__device__ __forceinline__ float tree_sum(float (&t)[N], int A) {
    constexpr int NB = (N + 3) / 4;
    float b[NB];
#pragma unroll
    for (int a = 0; a < N; ++a)
        if (a >= A) t[a] = 0.0f;
#pragma unroll
    for (int q = 0; q < NB; ++q) {
        b[q] = t[4 * q];
#pragma unroll
        for (int k = 1; k < 4; ++k)
            if (4 * q + k < N) b[q] = __fadd_rn(b[q], t[4 * q + k]);
    }
#pragma unroll
    for (int w = 1; w < NB; w *= 2) {
#pragma unroll
        for (int q = 0; q + w < NB; q += 2 * w) b[q] = __fadd_rn(b[q], b[q + w]);
    }
    return b[0];
}

// Normal(mu, sigma).entropy() of one action (normal.py)
__device__ __forceinline__ float entropy_term(float ls) { return kEntC + ls; }

// KL(old || new) of one action (ppo.py:262-268) in the reference's exact fp32 operation sequence (true divisions,
// logf): near a zero KL its terms cancel to ~1e-5 and any reordering would show up relative to it.
__device__ __forceinline__ float kl_term_exact(float s, float os, float mu, float omu) {
    const float dm = __fsub_rn(omu, mu);
    const float t1 = logf(__fadd_rn(__fdiv_rn(s, os), 1.0e-5f));
    const float t2 = __fdiv_rn(__fadd_rn(__fmul_rn(os, os), __fmul_rn(dm, dm)), __fmul_rn(2.0f, __fmul_rn(s, s)));
    return __fsub_rn(__fadd_rn(t1, t2), 0.5f);
}

// The same term with a shared sigma: the rollout stored one sigma per action for every sample (the same std
// parameter), so log(sigma / old_sigma + 1e-5) is a per-action constant -- evaluated once from sample 0's old sigma
// and used for every element whose old sigma has exactly those bits -- and the division by the per-action constant
// D = 2 sigma^2 is done as q0 = n * RN(1/D), q = fma(fma(-q0, D, n), RN(1/D), q0): the correctly rounded quotient
// (Markstein's theorem; tested against true division in oracle/kl_division_check.c) for n and D in the normal range.
// Same bits as __fdiv_rn, ~30 fewer VALU.  `slow` is set for an element outside those conditions: the caller then
// takes kl_term_exact for every element of the lane.
struct KlFastConsts {
    float os, t1, D, rD;
};

__device__ __forceinline__ KlFastConsts kl_fast_consts(float s, float os0, int kl_fast) {
    const float D = __fmul_rn(2.0f, __fmul_rn(s, s));
    const bool d_ok = D >= 0x1p-60f && D <= 0x1p60f;  // else: every element takes the full path
    return {(d_ok && kl_fast) ? os0 : __builtin_nanf(""),  // NaN never compares equal
            logf(__fadd_rn(__fdiv_rn(s, os0), 1.0e-5f)), D, __fdiv_rn(1.0f, D)};
}

__device__ __forceinline__ float kl_term_fast(const KlFastConsts& c, float os, float mu, float omu, bool& slow) {
    const float dm = __fsub_rn(omu, mu);
    const float n = __fadd_rn(__fmul_rn(os, os), __fmul_rn(dm, dm));
    const float q0 = __fmul_rn(n, c.rD);
    const float t2 = __builtin_fmaf(__builtin_fmaf(-q0, c.D, n), c.rD, q0);
    slow |= !(os == c.os && n >= 0x1p-60f && n <= 0x1p60f);
    return __fsub_rn(__fadd_rn(c.t1, t2), 0.5f);
}

// ppo.py:221-223: (adv - mean) / (std + 1e-8) with the mini-batch's statistics
__device__ __forceinline__ float adv_den(float std) { return __fadd_rn(std, 1e-8f); }
__device__ __forceinline__ float normalize_adv(float adv, float mean, float den) {
    return __fdiv_rn(__fsub_rn(adv, mean), den);
}

// Clipped surrogate of one sample (ppo.py:297-302): returns the loss term max(surr, surr_c); g_logp = d loss /
// d log-prob (torch.max ties split 1/2 : 1/2; clamp passes the gradient on the closed interval).
__device__ __forceinline__ float surrogate(float logp, float old_logp, float adv, float ratio_lo, float ratio_hi,
                                           float g_surr, float& g_logp) {
    const float ratio = expf(logp - old_logp);
    const float nadv = -adv;
    const float surr = nadv * ratio;
    const float rc = clamp_nan(ratio, ratio_lo, ratio_hi);
    const float surr_c = nadv * rc;
    float g_s, g_sc;
    max_grads(surr, surr_c, g_surr, g_s, g_sc);
    const bool in_clip = (ratio >= ratio_lo) && (ratio <= ratio_hi);
    const float g_ratio = g_s * nadv + (in_clip ? g_sc * nadv : 0.0f);
    g_logp = g_ratio * ratio;
    return max_nan(surr, surr_c);
}

// Value loss of one sample (ppo.py:305-313, :367 backward): returns d loss / dV, vterm = the loss term.  A caller that
// uses only one of the two (the actor head: the term; the critic heads: the gradient) pays for that one alone.
__device__ __forceinline__ float value_loss(float V, float tv, float R, int clipped, float clip, float g_value,
                                            float& vterm) {
    if (clipped) {
        const float dv = V - tv;
        const float vc = tv + clamp_nan(dv, -clip, clip);
        const float e1 = V - R;
        const float e2 = vc - R;
        const float vl = e1 * e1;
        const float vlc = e2 * e2;
        vterm = max_nan(vl, vlc);
        float g1, g2;
        max_grads(vl, vlc, g_value, g1, g2);
        float dV = 2.0f * g1 * e1;
        if (dv >= -clip && dv <= clip) dV += 2.0f * g2 * e2;
        return dV;
    }
    const float e = R - V;
    vterm = e * e;
    return -2.0f * g_value * e;
}

__device__ __forceinline__ float value_loss_grad(float V, float tv, float R, int clipped, float clip, float g_value) {
    float vterm;
    return value_loss(V, tv, R, clipped, clip, g_value, vterm);
}

// d/dmu = g_logp (x - mu) / sigma^2;  d/dsigma = g_logp ((x - mu)^2 / sigma^3 - 1 / sigma) + g_ent / sigma
__device__ __forceinline__ void normal_grads(float d, float inv_den, float inv_s, float inv_s3, float g_logp,
                                             float g_ent, float& gmu, float& gsg) {
    gmu = 2.0f * g_logp * d * inv_den;
    // autograd reaches sigma over two paths of g_logp (the variance and the log) and adds them: an infinite g_logp gives
    // inf - inf = NaN there, +-inf in the factored form below.  g_logp * 0 is 0 for a finite g_logp (the same bits as
    // without it) and NaN otherwise: fail the way the reference fails
    gsg = g_logp * (d * d * inv_s3 - inv_s) + (g_ent + g_logp * 0.0f) * inv_s;
}

template <int MAXA, bool VEC>
__device__ __forceinline__ void load_row(const float* __restrict__ p, int A, float (&r)[MAXA]) {
    if constexpr (VEC) {
#pragma unroll
        for (int a = 0; a < MAXA; a += 4) {
            if (a < A) {
                const float4 v = *reinterpret_cast<const float4*>(p + a);
                r[a] = v.x;
                r[a + 1] = v.y;
                r[a + 2] = v.z;
                r[a + 3] = v.w;
            }
        }
    } else {
#pragma unroll
        for (int a = 0; a < MAXA; ++a)
            if (a < A) r[a] = p[a];
    }
}

template <int MAXA, bool VEC>
__device__ __forceinline__ void store_row(float* __restrict__ p, int A, const float (&r)[MAXA]) {
    if constexpr (VEC) {
#pragma unroll
        for (int a = 0; a < MAXA; a += 4)
            if (a < A) *reinterpret_cast<float4*>(p + a) = make_float4(r[a], r[a + 1], r[a + 2], r[a + 3]);
    } else {
#pragma unroll
        for (int a = 0; a < MAXA; ++a)
            if (a < A) p[a] = r[a];
    }
}

// Host: the scalars of one loss launch.  rows: the stored mini-batch B; k_ppo: copies of it the surrogate and the value
// loss average over (the symmetric kernel's augmented blocks; 1 elsewhere) -- the entropy always averages over B.
struct LossScalars {
    float ratio_lo, ratio_hi;  // (float)(1 -/+ clip_param)
    float g_surr;              // 1 / (k_ppo B)                (MeanBackward of surrogate_loss)
    float g_value;             // value_loss_coef / (k_ppo B)  (MulBackward then MeanBackward)
    float g_ent;               // -entropy_coef / B
};

inline LossScalars loss_scalars(float clip_param, float value_loss_coef, float entropy_coef, int64_t rows,
                                int64_t k_ppo = 1) {
    const float n_ppo = static_cast<float>(rows * k_ppo);
    return {static_cast<float>(1.0 - static_cast<double>(clip_param)),
            static_cast<float>(1.0 + static_cast<double>(clip_param)), 1.0f / n_ppo, value_loss_coef / n_ppo,
            -entropy_coef / static_cast<float>(rows)};
}

// RSLRL_KL_FAST=0 disables the per-action-constant KL (kl_term_fast); read per call: the tests compare both bitwise
inline bool kl_fast_enabled() {
    const char* e = std::getenv("RSLRL_KL_FAST");
    return !(e && e[0] == '0');
}

constexpr int kFoldGroup = 64;

// Sum over the 4 lanes of a quad (DPP quad_perm [1,0,3,2] then [2,3,0,1]); every lane of the quad
// gets the same bits ((v0 + v1) + (v2 + v3), fp addition being commutative).
__device__ __forceinline__ float quad_sum(float v) {
    const float a = __fadd_rn(v, __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), 0xB1,
                                                                                      0xF, 0xF, false)));
    return __fadd_rn(a, __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, a), 0x4E, 0xF,
                                                                             0xF, false)));
}

// Fixed-order fold of `n` (<= 64) partials per column (column c at src[c * ld + r]) into out[c]:
// 16 lanes per column, each adding rows l16, l16+16, l16+32, l16+48 in that order, then a 16-lane
// butterfly.  Every load is issued before the first add, so the fold costs one memory round trip.
// Loads use sc1 (bypass the non-coherent per-CU cache); the caller has acquired.
// kRows = 8 (rows l16 + 16 i, i < 8: n <= 128) for the groups of 128 blocks of a grid over 4096 blocks.
template <int kMaxC, int kRows = 4>
__device__ __forceinline__ void fold_columns(const double* __restrict__ src, int ld, int n, int ncols,
                                             double* __restrict__ out) {
    constexpr int kPasses = (kMaxC + 15) / 16;
    const int l16 = threadIdx.x & 15;
    const int cc = threadIdx.x >> 4;
    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<double*>(src), 0, static_cast<int>(sizeof(double) * ncols * ld), 0x00020000);
    double v[kPasses][kRows];
#pragma unroll
    for (int ps = 0; ps < kPasses; ++ps) {
        const int c = ps * 16 + cc;
#pragma unroll
        for (int i = 0; i < kRows; ++i) {
            const int r = l16 + 16 * i;
            // out-of-range offsets read 0 through the buffer resource
            const int off = (c < ncols && r < n) ? (c * ld + r) * 8 : 0x7ffffff0;
            v[ps][i] = __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(rsrc, off, 0, 16 /* sc1 */));
        }
    }
#pragma unroll
    for (int ps = 0; ps < kPasses; ++ps) {
        double t = ((v[ps][0] + v[ps][1]) + v[ps][2]) + v[ps][3];
#pragma unroll
        for (int i = 4; i < kRows; ++i) t += v[ps][i];
#pragma unroll
        for (int off = 8; off >= 1; off >>= 1) t += __shfl_xor(t, off, kWave);
        const int c = ps * 16 + cc;
        if (l16 == 0 && c < ncols) out[c] = t;
    }
}

// Two-level fixed-order reduction of one fp64 value per column and block over the grid (at most kFoldGroup^2
// blocks): every block publishes `v` of column threadIdx.x (< ncols) to partials[c * nb + block]; the last
// arriving block of each group of kFoldGroup folds the group (fold_columns: the same order whatever the arrival
// order) into partials[ncols * nb + c * ng + g], and the last group to finish folds the groups into `folded` (LDS,
// ncols doubles).  Returns true only in that final block, with `folded` complete.  tickets: 1 + ng words, zero
// before the launch and re-armed to zero by it (the global word by the caller of the final block: it returns with
// tickets[0] still counting).  `flag`: an LDS int.  Called by every thread of the block.
// G: blocks per group -- kFoldGroup, or 2 kFoldGroup for grids over kFoldGroup^2 blocks (up to 8192; the groups then
// fold 8 rows per lane, fold_columns<kMaxC, 8>)
template <int kMaxC, int G = kFoldGroup>
__device__ __forceinline__ bool fold_grid_partials(double* __restrict__ partials, unsigned* __restrict__ tickets,
                                                   int nb, int ncols, double v, double* folded, int* flag) {
    constexpr int kFoldGroup = G;
    const int ng = (nb + kFoldGroup - 1) / kFoldGroup;
    if (static_cast<int>(threadIdx.x) < ncols)
        __hip_atomic_store(reinterpret_cast<unsigned long long*>(partials + static_cast<int64_t>(threadIdx.x) * nb +
                                                                 blockIdx.x),
                           __double_as_longlong(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    const int g = blockIdx.x / kFoldGroup;
    const int g0 = g * kFoldGroup;
    const int gsz = min(kFoldGroup, nb - g0);
    if (threadIdx.x == 0) {
        const unsigned t = __hip_atomic_fetch_add(tickets + 1 + g, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const int last = (t == static_cast<unsigned>(gsz) - 1);
        if (last) {
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        *flag = last;
    }
    __syncthreads();
    if (!*flag) return false;
    if (threadIdx.x == 0) __hip_atomic_store(tickets + 1 + g, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    fold_columns<kMaxC, (G > 64 ? 8 : 4)>(partials + g0, nb, gsz, ncols, folded);
    __syncthreads();
    if (ng == 1) return true;
    double* gpart = partials + static_cast<int64_t>(ncols) * nb;
    if (static_cast<int>(threadIdx.x) < ncols)
        __hip_atomic_store(reinterpret_cast<unsigned long long*>(gpart + static_cast<int64_t>(threadIdx.x) * ng + g),
                           __double_as_longlong(folded[threadIdx.x]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned t = __hip_atomic_fetch_add(tickets, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const int last = (t == static_cast<unsigned>(ng) - 1);
        if (last) {
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        *flag = last;
    }
    __syncthreads();
    if (!*flag) return false;
    fold_columns<kMaxC>(gpart, ng, ng, ncols, folded);
    __syncthreads();
    return true;
}

}  // namespace
}  // namespace rslrl
