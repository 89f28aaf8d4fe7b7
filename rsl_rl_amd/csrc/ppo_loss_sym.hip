// Fused symmetric PPO loss forward + backward on gfx950 (rslrl_ppo_loss_sym_fwd_bwd).
//
// The mini-batch of ppo_loss.hip evaluated on K symmetry-augmented copies of its B stored rows -- rsl_rl/algorithms/
// ppo.py:213-257 (data augmentation: the policy runs on K * B rows, the stored scalars are repeated) and :317-348 (the
// mirror loss MSE(mean[B:], augment(mean[:B]).detach()[B:])).  The reference evaluates the mirror term with a second,
// deterministic actor forward on the same inputs; both graph branches add their gradients at the mean, so one
// forward and a summed d loss / d mu is the same mathematics, and that sum is what this kernel writes.
//
// One lane per row i = k * B + j (block k, stored row j), the lane-per-sample form of ppo_loss.hip:
//   k <  k_ppo : log-prob, ratio, clipped surrogate, clipped / plain value loss and their gradients; the five stored
//                scalars are read at j (the repeat is never materialised); means over k_ppo * B rows
//   k == 0     : entropy (mean over B) and the KL of the adaptive learning rate (mean over B)
//   k >= 1     : the mirror term against t[i][a] = sign[k][a] * mu[j][perm[k][a]] (tables; the base row is read
//                again, from the cache its own lane filled) or against a caller-made target tensor; gradient to
//                grad_mu[i] only
// Loss terms, the symmetry sum and a shared sigma's gradient fold into fp64 per-block partials and then over the grid
// in a fixed order (fold_grid_partials): deterministic.
// Bytes per row of block k (sigma shared, A actions, KL on), HBM-bound like its sibling:
//   k == 0            : read 4A mu + 4A actions + 8A old mu / sigma + 20 scalars, write 4A d mu + 4 d V    = 20A + 24
//   0 < k < k_ppo     : read 4A mu + 4A actions + 20 scalars (+ 4A target, pointer form), write 4A + 4    = 12A + 24 (+ 4A)
//   k >= k_ppo        : read 4A mu (+ 4A target), write 4A d mu                                            = 8A (+ 4A)
// so K = k_ppo = k_mir = 2 with tables moves (32A + 48) B bytes per mini-batch.

#include <algorithm>
#include <cstdint>

#include "common.h"
#include "ppo_loss_common.h"

namespace rslrl {
namespace {

constexpr int kSymMaxBlocks = 512;  // <= kFoldGroup^2 / 8: the two-level fold of fold_grid_partials
constexpr size_t kSymTicketBytes = 1024;

enum { kSymSurr = 0, kSymValue, kSymEnt, kSymKl, kSymMirror, kSymScalarCols };

struct SymParams {
    int64_t B;
    int64_t rows;  // k_mir * B
    int32_t A;
    int32_t k_ppo;
    int32_t k_mir;
    const float* mu;
    int64_t mu_stride;
    const float* sigma;
    int64_t sigma_stride;
    const float* values;
    const float* actions;
    const float* old_logp;
    const float* adv;
    const float* target_values;
    const float* returns;
    const float* old_mu;
    const float* old_sigma;
    const float* mirror_target;
    const int32_t* act_perm;
    const float* act_sign;
    float clip;
    float ratio_lo;
    float ratio_hi;
    float g_surr;    // 1 / (k_ppo B)
    float g_value;   // value_loss_coef / (k_ppo B)
    float g_ent;     // -entropy_coef / B
    float g_mirror;  // mirror_coeff * 2 / ((k_mir - 1) B A)
    float mirror_coeff;
    float value_loss_coef;
    float entropy_coef;
    int32_t clipped_value;
    int32_t compute_kl;
    int32_t normalize_adv;
    float* grad_mu;
    int64_t grad_mu_stride;
    float* grad_sigma;
    int64_t grad_sigma_stride;
    float* grad_values;
    int64_t gv_stride;
    float* stats;
    double* symmetry_sum;
};

// SHARED: sigma is the policy's [A] vector (its gradient folds over the grid; its log and reciprocals are per-action
// constants, computed once per block and read from LDS as broadcasts -- they would cost 4 MAXA registers per lane);
// otherwise sigma is per row [rows, A].  EXACT: A == MAXA, so every `a < A` guard folds away at compile time.
template <int MAXA, bool VEC, bool SHARED, bool EXACT>
__global__ __launch_bounds__(kBlock) void ppo_loss_sym_kernel(SymParams p, double* __restrict__ partials,
                                                              unsigned* __restrict__ tickets) {
    constexpr int kMaxCols = kSymScalarCols + MAXA;
    __shared__ double wave_part[kBlock / kWave][kMaxCols];
    __shared__ double folded[kMaxCols];
    __shared__ float k_const[4][MAXA];  // log sigma, 1 / (2 sigma^2), 1 / sigma, 1 / sigma^3
    __shared__ int flag;
    const int A = EXACT ? MAXA : p.A;
    const int ncols = kSymScalarCols + (SHARED ? A : 0);
    if constexpr (SHARED) {
        if (static_cast<int>(threadIdx.x) < A) {
            const SigmaConsts c = sigma_consts(p.sigma[threadIdx.x]);
            k_const[0][threadIdx.x] = c.ls;
            k_const[1][threadIdx.x] = c.inv_den;
            k_const[2][threadIdx.x] = c.inv_s;
            k_const[3][threadIdx.x] = c.inv_s3;
        }
        __syncthreads();
    }

    float adv_mean = 0.0f, adv_d = 1.0f;
    if (p.normalize_adv) {
        adv_mean = p.stats[5];
        adv_d = adv_den(p.stats[6]);
    }
    float ent_shared = 0.0f;
    if constexpr (SHARED) {
#pragma unroll
        for (int a = 0; a < MAXA; ++a)
            if (a < A) ent_shared = __fadd_rn(ent_shared, entropy_term(k_const[0][a]));
    }

    // per-lane sums stay fp32 (a lane sees a few rows); cross-lane / cross-block folds are fp64
    float acc[kMaxCols];
#pragma unroll
    for (int c = 0; c < kMaxCols; ++c) acc[c] = 0.0f;

    const int64_t stride = static_cast<int64_t>(gridDim.x) * kBlock;
    for (int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; i < p.rows; i += stride) {
        const int k = static_cast<int>(i / p.B);
        const int64_t j = i - static_cast<int64_t>(k) * p.B;
        const bool ppo = k < p.k_ppo;
        const bool base = k == 0;

        float mu[MAXA], gmu[MAXA];
        load_row<MAXA, VEC>(p.mu + i * p.mu_stride, A, mu);
#pragma unroll
        for (int a = 0; a < MAXA; ++a) gmu[a] = 0.0f;
        const float* sg_row = SHARED ? p.sigma : p.sigma + i * p.sigma_stride;
        float* gsg_row = SHARED ? nullptr : p.grad_sigma + i * p.grad_sigma_stride;
        const auto consts = [&](int a) {  // of action a: the block's LDS copy, or this row's (kInvDenRn there too)
            return SHARED ? SigmaConsts{sg_row[a], k_const[0][a], k_const[1][a], k_const[2][a], k_const[3][a]}
                          : sigma_consts(sg_row[a]);
        };

        if (ppo) {
            const float* x = p.actions + i * A;
            const float old_logp = p.old_logp[j];
            float adv = p.adv[j];
            const float V = p.values[i];
            const float tv = p.target_values[j];
            const float R = p.returns[j];
            if (p.normalize_adv) adv = normalize_adv(adv, adv_mean, adv_d);

            // Normal(mu, sigma).log_prob(x).sum(-1), entropy().sum(-1), KL (normal.py; ppo.py:262-268)
            float d[MAXA];
            float lterm[MAXA];
            float ent = 0.0f, kl = 0.0f;
            const bool want_kl = base && p.compute_kl;
            {
                float xr[MAXA];
                load_row<MAXA, VEC>(x, A, xr);
#pragma unroll
                for (int a = 0; a < MAXA; ++a) {
                    if (a < A) {
                        const SigmaConsts c = consts(a);
                        if constexpr (!SHARED) ent += entropy_term(c.ls);
                        d[a] = xr[a] - mu[a];
                        lterm[a] = logp_term(d[a], c.inv_den, c.ls);
                    }
                }
            }
            const float logp = tree_sum<MAXA>(lterm, A);
            if (want_kl) {
                float omu[MAXA], osg[MAXA];
                load_row<MAXA, VEC>(p.old_mu + j * A, A, omu);
                load_row<MAXA, VEC>(p.old_sigma + j * A, A, osg);
#pragma unroll
                for (int a = 0; a < MAXA; ++a) {
                    if (a < A) kl = __fadd_rn(kl, kl_term_exact(sg_row[a], osg[a], mu[a], omu[a]));
                }
            }
            if (SHARED) ent = ent_shared;

            float g_logp, vterm;
            const float sterm = surrogate(logp, old_logp, adv, p.ratio_lo, p.ratio_hi, p.g_surr, g_logp);
            p.grad_values[i * p.gv_stride] = value_loss(V, tv, R, p.clipped_value, p.clip, p.g_value, vterm);

            const float g_ent = base ? p.g_ent : 0.0f;
            float gsg[MAXA];
#pragma unroll
            for (int a = 0; a < MAXA; ++a) {
                if (a < A) {
                    const SigmaConsts c = consts(a);
                    normal_grads(d[a], c.inv_den, c.inv_s, c.inv_s3, g_logp, g_ent, gmu[a], gsg[a]);
                } else {
                    gsg[a] = 0.0f;
                }
            }
            if constexpr (SHARED) {
#pragma unroll
                for (int a = 0; a < MAXA; ++a)
                    if (a < A) acc[kSymScalarCols + a] += gsg[a];
            } else {
                store_row<MAXA, VEC>(gsg_row, A, gsg);
            }
            acc[kSymSurr] += sterm;
            acc[kSymValue] += vterm;
            if (base) {
                acc[kSymEnt] += ent;
                acc[kSymKl] += kl;
            }
        } else if constexpr (!SHARED) {
            float zero[MAXA];
#pragma unroll
            for (int a = 0; a < MAXA; ++a) zero[a] = 0.0f;
            store_row<MAXA, VEC>(gsg_row, A, zero);  // no loss term reads this row's sigma
        }

        // mirror term (ppo.py:328-343): rows of the augmented blocks against the augmented base mean (detached)
        if (!base && p.k_mir > 1) {
            float t[MAXA];
            if (p.mirror_target) {
                load_row<MAXA, VEC>(p.mirror_target + i * A, A, t);
            } else {
                const float* mb = p.mu + j * p.mu_stride;
                const int32_t* perm = p.act_perm + k * A;
                const float* sign = p.act_sign + k * A;
#pragma unroll
                for (int a = 0; a < MAXA; ++a) {
                    if (a < A) {
                        const int src = min(max(perm[a], 0), A - 1);  // a bad table cannot leave the row
                        t[a] = __fmul_rn(sign[a], mb[src]);
                    }
                }
            }
            float sq = 0.0f;
#pragma unroll
            for (int a = 0; a < MAXA; ++a) {
                if (a < A) {
                    const float diff = __fsub_rn(mu[a], t[a]);
                    sq = __fadd_rn(sq, __fmul_rn(diff, diff));
                    gmu[a] = __fadd_rn(gmu[a], __fmul_rn(p.g_mirror, diff));
                }
            }
            acc[kSymMirror] += sq;
        }
        store_row<MAXA, VEC>(p.grad_mu + i * p.grad_mu_stride, A, gmu);
    }

    // ---- per-block partials: wave butterfly per column, waves in order, then the grid fold
    const int lane = threadIdx.x & (kWave - 1);
    const int wid = threadIdx.x / kWave;
#pragma unroll
    for (int c = 0; c < kMaxCols; ++c) {
        if (c < ncols) {
            const double v = wave_sum(static_cast<double>(acc[c]));
            if (lane == 0) wave_part[wid][c] = v;
        }
    }
    __syncthreads();
    double v = 0.0;
    if (static_cast<int>(threadIdx.x) < ncols) {
        v = wave_part[0][threadIdx.x];
#pragma unroll
        for (int w = 1; w < kBlock / kWave; ++w) v += wave_part[w][threadIdx.x];
    }
    if (!fold_grid_partials<kMaxCols>(partials, tickets, static_cast<int>(gridDim.x), ncols, v, folded, &flag)) return;
    if (threadIdx.x == 0) {
        const double n_ppo = static_cast<double>(p.k_ppo) * static_cast<double>(p.B);
        const double Bd = static_cast<double>(p.B);
        float* stats = p.stats;
        stats[1] = static_cast<float>(folded[kSymSurr] / n_ppo);
        stats[2] = static_cast<float>(folded[kSymValue] / n_ppo);
        stats[3] = static_cast<float>(folded[kSymEnt] / Bd);
        stats[4] = static_cast<float>(folded[kSymKl] / Bd);
        const float sym = p.k_mir > 1 ? static_cast<float>(folded[kSymMirror] /
                                                           (static_cast<double>(p.k_mir - 1) * Bd * A))
                                      : 0.0f;
        // ppo.py:315 in fp32: surrogate_loss + c_v * value_loss - c_e * entropy.mean(); :346 + c_m * symmetry_loss
        float loss = __fsub_rn(__fadd_rn(stats[1], __fmul_rn(p.value_loss_coef, stats[2])),
                               __fmul_rn(p.entropy_coef, stats[3]));
        if (p.mirror_coeff != 0.0f) loss = __fadd_rn(loss, __fmul_rn(p.mirror_coeff, sym));
        stats[0] = loss;
        if (!p.normalize_adv) {
            stats[5] = 0.0f;
            stats[6] = 0.0f;
        }
        stats[7] = sym;
        if (p.symmetry_sum) *p.symmetry_sum += static_cast<double>(sym);
        __hip_atomic_store(tickets, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // re-arm (stream-ordered)
    }
    if constexpr (SHARED) {
        if (static_cast<int>(threadIdx.x) < A)
            p.grad_sigma[threadIdx.x] = static_cast<float>(folded[kSymScalarCols + threadIdx.x]);
    }
}

// Per-mini-batch advantage statistics (ppo.py:221-223) over the B stored values: (mean, unbiased std) in
// stats[5..6], one block, fp64, fixed order.
__global__ __launch_bounds__(kBlock) void sym_adv_moments_kernel(const float* __restrict__ x, int64_t n,
                                                                 float* __restrict__ stats) {
    __shared__ double scratch[2][kBlock / kWave];
    double s = 0.0, ss = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += kBlock) {
        const double a = x[i];
        s += a;
        ss += a * a;
    }
    s = block_sum(s, scratch[0]);
    ss = block_sum(ss, scratch[1]);
    if (threadIdx.x == 0) {
        const double mean = s / static_cast<double>(n);
        double var = (ss - s * mean) / static_cast<double>(n - 1);
        if (var < 0.0) var = 0.0;
        stats[5] = static_cast<float>(mean);
        stats[6] = static_cast<float>(sqrt(var));
    }
}

int sym_blocks(int64_t rows) {
    return static_cast<int>(std::max<int64_t>(1, std::min<int64_t>(ceil_div(rows, kBlock), kSymMaxBlocks)));
}

bool sym_aligned16(const void* ptr) { return (reinterpret_cast<uintptr_t>(ptr) & 15) == 0; }

template <int MAXA, bool EXACT>
void launch_sym_exact(const SymParams& p, bool vec, bool shared, int nb, double* part, unsigned* tickets,
                      hipStream_t st) {
    const dim3 g(nb), b(kBlock);
    if (vec && shared)
        hipLaunchKernelGGL((ppo_loss_sym_kernel<MAXA, true, true, EXACT>), g, b, 0, st, p, part, tickets);
    else if (vec)
        hipLaunchKernelGGL((ppo_loss_sym_kernel<MAXA, true, false, EXACT>), g, b, 0, st, p, part, tickets);
    else if (shared)
        hipLaunchKernelGGL((ppo_loss_sym_kernel<MAXA, false, true, EXACT>), g, b, 0, st, p, part, tickets);
    else
        hipLaunchKernelGGL((ppo_loss_sym_kernel<MAXA, false, false, EXACT>), g, b, 0, st, p, part, tickets);
}

template <int MAXA>
void launch_sym(const SymParams& p, bool vec, bool shared, int nb, double* part, unsigned* tickets, hipStream_t st) {
    if (p.A == MAXA)
        launch_sym_exact<MAXA, true>(p, vec, shared, nb, part, tickets, st);
    else
        launch_sym_exact<MAXA, false>(p, vec, shared, nb, part, tickets, st);
}

}  // namespace
}  // namespace rslrl

using namespace rslrl;

extern "C" size_t rslrl_ppo_loss_sym_workspace_bytes(int64_t B, int32_t A, int32_t k_mir) {
    const size_t cols = kSymScalarCols + static_cast<size_t>(A > 0 ? A : 0);
    const int64_t rows = (B > 0 ? B : 0) * static_cast<int64_t>(k_mir > 0 ? k_mir : 1);
    const size_t nb = static_cast<size_t>(sym_blocks(rows));
    return kSymTicketBytes + align_up(sizeof(double) * cols * (nb + ceil_div(nb, kFoldGroup)), 256);
}

extern "C" int rslrl_ppo_loss_sym_fwd_bwd(const rslrl_ppo_loss_sym_args_t* s, void* workspace, size_t workspace_bytes,
                                          rslrl_stream_t stream) {
    if (!s) return RSLRL_E_INVALID_ARGUMENT;
    const rslrl_ppo_loss_args_t* a = &s->loss;
    if (a->B < 1 || a->A < 1 || a->A > RSLRL_PPO_LOSS_MAX_ACTIONS) return RSLRL_E_INVALID_ARGUMENT;
    if (s->k_mir < 1 || s->k_mir > RSLRL_SYMMETRY_MAX_AUG) return RSLRL_E_INVALID_ARGUMENT;
    if (s->k_ppo != 1 && s->k_ppo != s->k_mir) return RSLRL_E_INVALID_ARGUMENT;
    if (a->sigma_mode != 0 && a->sigma_mode != 1) return RSLRL_E_INVALID_ARGUMENT;
    if (!a->mu || !a->sigma || !a->values || !a->actions || !a->old_logp || !a->advantages || !a->target_values ||
        !a->returns || !a->old_mu || !a->old_sigma || !a->grad_mu || !a->grad_sigma || !a->grad_values || !a->stats)
        return RSLRL_E_INVALID_ARGUMENT;
    const bool tables = s->act_perm || s->act_sign;
    if (tables && (!s->act_perm || !s->act_sign)) return RSLRL_E_INVALID_ARGUMENT;
    if (s->k_mir > 1 ? (tables == (s->mirror_target != nullptr)) : (tables || s->mirror_target))
        return RSLRL_E_INVALID_ARGUMENT;  // exactly one target form with a mirror term, none without
    if (a->mu_stride < a->A || a->grad_mu_stride < a->A) return RSLRL_E_INVALID_ARGUMENT;
    if (a->sigma_mode == 1 && (a->sigma_stride < a->A || a->grad_sigma_stride < a->A)) return RSLRL_E_INVALID_ARGUMENT;
    if (a->B > (int64_t{1} << 40)) return RSLRL_E_INVALID_ARGUMENT;
    if (!workspace) return RSLRL_E_INVALID_ARGUMENT;
    if (workspace_bytes < rslrl_ppo_loss_sym_workspace_bytes(a->B, a->A, s->k_mir)) return RSLRL_E_WORKSPACE_TOO_SMALL;
    if (!sym_aligned16(workspace)) return RSLRL_E_MISALIGNED;

    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int A = a->A;
    SymParams p{};
    p.B = a->B;
    p.rows = a->B * s->k_mir;
    p.A = A;
    p.k_ppo = s->k_ppo;
    p.k_mir = s->k_mir;
    p.mu = a->mu;
    p.mu_stride = a->mu_stride;
    p.sigma = a->sigma;
    p.sigma_stride = a->sigma_stride;
    p.values = a->values;
    p.actions = a->actions;
    p.old_logp = a->old_logp;
    p.adv = a->advantages;
    p.target_values = a->target_values;
    p.returns = a->returns;
    p.old_mu = a->old_mu;
    p.old_sigma = a->old_sigma;
    p.mirror_target = s->mirror_target;
    p.act_perm = s->act_perm;
    p.act_sign = s->act_sign;
    p.clip = a->clip_param;
    const LossScalars k = loss_scalars(a->clip_param, a->value_loss_coef, a->entropy_coef, a->B, s->k_ppo);
    p.ratio_lo = k.ratio_lo;
    p.ratio_hi = k.ratio_hi;
    p.g_surr = k.g_surr;
    p.g_value = k.g_value;
    p.g_ent = k.g_ent;
    p.g_mirror = s->k_mir > 1 ? static_cast<float>(2.0 * static_cast<double>(s->mirror_coeff) /
                                                   (static_cast<double>(s->k_mir - 1) * static_cast<double>(a->B) * A))
                              : 0.0f;
    p.mirror_coeff = s->mirror_coeff;
    p.value_loss_coef = a->value_loss_coef;
    p.entropy_coef = a->entropy_coef;
    p.clipped_value = a->use_clipped_value_loss ? 1 : 0;
    p.compute_kl = a->compute_kl ? 1 : 0;
    p.normalize_adv = a->normalize_advantage ? 1 : 0;
    p.grad_mu = a->grad_mu;
    p.grad_mu_stride = a->grad_mu_stride;
    p.grad_sigma = a->grad_sigma;
    p.grad_sigma_stride = a->grad_sigma_stride;
    p.grad_values = a->grad_values;
    p.gv_stride = a->grad_values_stride > 1 ? a->grad_values_stride : 1;
    p.stats = a->stats;
    p.symmetry_sum = s->symmetry_sum;

    if (p.normalize_adv) {
        hipLaunchKernelGGL(sym_adv_moments_kernel, dim3(1), dim3(kBlock), 0, st, a->advantages, a->B, a->stats);
        const int rc = launch_status();
        if (rc != RSLRL_OK) return rc;
    }

    // 16-byte row accesses when every [rows, A] operand allows it
    bool vec = (A % 4 == 0) && (a->mu_stride % 4 == 0) && (a->grad_mu_stride % 4 == 0) && sym_aligned16(a->mu) &&
               sym_aligned16(a->actions) && sym_aligned16(a->old_mu) && sym_aligned16(a->old_sigma) &&
               sym_aligned16(a->grad_mu) && sym_aligned16(s->mirror_target);
    if (a->sigma_mode == 1)
        vec = vec && (a->sigma_stride % 4 == 0) && (a->grad_sigma_stride % 4 == 0) && sym_aligned16(a->sigma) &&
              sym_aligned16(a->grad_sigma);
    const bool shared = a->sigma_mode == 0;
    const int nb = sym_blocks(p.rows);
    unsigned* tickets = static_cast<unsigned*>(workspace);
    double* part = reinterpret_cast<double*>(static_cast<char*>(workspace) + kSymTicketBytes);
    if (A <= 4)
        launch_sym<4>(p, vec, shared, nb, part, tickets, st);
    else if (A <= 8)
        launch_sym<8>(p, vec, shared, nb, part, tickets, st);
    else if (A <= 12)
        launch_sym<12>(p, vec, shared, nb, part, tickets, st);
    else if (A <= 16)
        launch_sym<16>(p, vec, shared, nb, part, tickets, st);
    else if (A <= 32)
        launch_sym<32>(p, vec, shared, nb, part, tickets, st);
    else
        launch_sym<64>(p, vec, shared, nb, part, tickets, st);
    return launch_status();
}
