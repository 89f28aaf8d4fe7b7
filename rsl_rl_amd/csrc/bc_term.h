// The behaviour-cloning loss of one element (rsl_rl/algorithms/distillation.py:120-123: mse_loss / huber_loss, delta =
// 1) and its gradient: the one definition both the loss kernel (bc_loss.hip) and the fused distillation head
// (mlp_heads.hip, bc_head_epilogue) evaluate, so their gradients agree bit for bit.
#pragma once

#include "common.h"

namespace rslrl {
namespace {

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

// d loss / d pred's scale as rslrl_bc_loss_fwd_bwd computes it: mse 2 / (N A), huber 1 / (N A)
inline float bc_g_scale(bool huber, double count) { return static_cast<float>((huber ? 1.0 : 2.0) / count); }

}  // namespace
}  // namespace rslrl
