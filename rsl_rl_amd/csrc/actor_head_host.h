// Host side of the fused actor heads, shared by the units that launch them (mlp_heads.hip: 5 to 16 actions;
// mlp_head_wide.hip: 17 to 32): the argument struct's pointers, alignment, workspace and loss constants into ActorParams.
#pragma once

#include "common.h"
#include "mlp_gemm_x6.h"

namespace rslrl {
namespace {

// What the actor-head entries share behind their shape checks: pointers, alignment, the workspace and the loss constants into ap
inline int actor_head_params(const rslrl_linear_args_t* a, const rslrl_actor_head_args_t* h, void* workspace,
                      size_t workspace_bytes, ActorParams& ap, size_t need_bytes, bool kl_fast) {
    if (!a->c || !h->actions || !h->old_log_prob || !h->advantages || !h->values || !h->target_values ||
        !h->returns || !h->old_mu || !h->old_sigma || !h->sigma || !h->out_weight_t_image || !h->wgrad_partials ||
        !h->grad_sigma || !h->stats || !workspace)
        return RSLRL_E_INVALID_ARGUMENT;
    if (!aligned16(a->c) || !aligned16(h->out_weight_t_image) || !aligned16(workspace)) return RSLRL_E_MISALIGNED;
    if (workspace_bytes < need_bytes) return RSLRL_E_WORKSPACE_TOO_SMALL;
    ap.actions = h->actions;
    ap.old_mu = h->old_mu;
    ap.old_sigma = h->old_sigma;
    ap.sigma = h->sigma;
    ap.old_logp = h->old_log_prob;
    ap.adv = h->advantages;
    ap.values = h->values;
    ap.target_values = h->target_values;
    ap.returns = h->returns;
    ap.w_t_img = static_cast<const uint4*>(h->out_weight_t_image);
    ap.wpart = h->wgrad_partials;
    ap.grad_sigma = h->grad_sigma;
    ap.stats = h->stats;
    ap.grad_mu = h->grad_mu;
    ap.tickets = static_cast<unsigned*>(workspace);
    ap.partials = reinterpret_cast<double*>(static_cast<char*>(workspace) + 1024);
    const LossScalars k = loss_scalars(h->clip_param, h->value_loss_coef, h->entropy_coef, a->M);
    ap.clip = h->clip_param;
    ap.ratio_lo = k.ratio_lo;
    ap.ratio_hi = k.ratio_hi;
    ap.g_surr = k.g_surr;
    ap.g_ent = k.g_ent;
    ap.value_loss_coef = h->value_loss_coef;
    ap.entropy_coef = h->entropy_coef;
    ap.clipped_value = h->use_clipped_value_loss ? 1 : 0;
    ap.compute_kl = h->compute_kl ? 1 : 0;
    ap.kl_fast = kl_fast ? 1 : 0;  // the entry point reads RSLRL_KL_FAST per call (kl_fast_enabled)
    return RSLRL_OK;
}

// wave columns of a narrow head's N (64, 128, 192), else 0
inline int narrow_wave_cols(int64_t N) { return N == 64 || N == 128 || N == 192 ? static_cast<int>(N / 64) : 0; }

}  // namespace
}  // namespace rslrl
