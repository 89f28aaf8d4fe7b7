"""The wide-update fixture (tests/golden/make_golden_wide.py: one reference PPO.update() at hidden [320, 260, 64]): its
arrays, stored as three files of one key group each, as one mapping with np.load's interface (`files`, `[]`) for
update_fixtures.build_update / check_update; and the update run those two bracket."""

import json
import os

import numpy as np

from conftest import GOLDEN


class Arrays:
    def __init__(self, names):
        self._z = [np.load(os.path.join(GOLDEN, n)) for n in names]
        self._of = {k: z for z in self._z for k in z.files}
        self.files = list(self._of)

    def __getitem__(self, key):
        return self._of[key][key]


def load():
    with open(os.path.join(GOLDEN, "golden_wide.json")) as f:
        meta = json.load(f)["wide"]
    return Arrays(meta["files"]), meta


def _torch_update(alg, pol):
    """PPO.update() in plain torch on the policy's device (the hot path has no CPU form): the policy's own forward under
    autograd, one permutation per update (rollout_storage.py:160-203), the KL and the host lr rule (ppo.py:259-285),
    the PPO loss written out (:287-315), and alg.optimizer.step -- which build_update_cpu makes clip first."""
    import torch

    from rsl_rl_amd.algorithms.ppo import adapt_learning_rate

    st, M, E = alg.storage, alg.num_mini_batches, alg.num_learning_epochs
    flat = lambda t: t.flatten(0, 1)  # noqa: E731
    obs, actions, values, returns = flat(st.observations["policy"]), flat(st.actions), flat(st.values), flat(st.returns)
    old_lp, adv, old_mu, old_sigma = flat(st.actions_log_prob), flat(st.advantages), flat(st.mu), flat(st.sigma)
    B = obs.shape[0] // M
    indices = torch.randperm(M * B)
    lr = alg.learning_rate
    sums = {"value_function": 0.0, "surrogate": 0.0, "entropy": 0.0}
    for _ in range(E):
        for i in range(M):
            idx = indices[i * B:(i + 1) * B]
            mean, std = pol.action_distribution_params({"policy": obs[idx]})
            std = std.expand_as(mean)
            dist = torch.distributions.Normal(mean, std)
            logp, entropy = dist.log_prob(actions[idx]).sum(-1), dist.entropy().sum(-1)
            value = pol.evaluate({"policy": obs[idx]})
            with torch.no_grad():
                kl = torch.sum(torch.log(std / old_sigma[idx] + 1.0e-5) + (old_sigma[idx].square() + (
                    old_mu[idx] - mean).square()) / (2.0 * std.square()) - 0.5, -1).mean()
                lr = adapt_learning_rate(lr, kl.item(), alg.desired_kl)
                for g in alg.optimizer.param_groups:
                    g["lr"] = lr
            a, tv, ret = adv[idx].squeeze(-1), values[idx], returns[idx]
            ratio = torch.exp(logp - old_lp[idx].squeeze(-1))
            surrogate = torch.max(-a * ratio, -a * ratio.clamp(1.0 - alg.clip_param, 1.0 + alg.clip_param)).mean()
            clipped = tv + (value - tv).clamp(-alg.clip_param, alg.clip_param)
            value_loss = torch.max((value - ret).square(), (clipped - ret).square()).mean()
            loss = surrogate + alg.value_loss_coef * value_loss - alg.entropy_coef * entropy.mean()
            alg.optimizer.zero_grad()
            loss.backward()
            alg.optimizer.step()
            sums["value_function"] += value_loss.item()
            sums["surrogate"] += surrogate.item()
            sums["entropy"] += entropy.mean().item()
    alg.learning_rate = lr
    return {k: v / (M * E) for k, v in sums.items()}


def build_update_cpu(z, meta):
    """update_fixtures.build_update on the CPU.  compute_returns and update() run HIP kernels only, so for the length
    of the call compute_returns is the reference's GAE written in torch (recurrent_fused_fixtures.gae_torch), and the
    PPO it returns runs _torch_update as its update() with the gradient clip in front of its optimizer's step (where
    run_recorded_update reads the pre-clip gradient)."""
    import torch

    from recurrent_fused_fixtures import gae_torch
    from rsl_rl_amd.algorithms import PPO
    from update_fixtures import build_update

    def returns_cpu(self, obs):
        gae_torch(self.storage, self.policy.evaluate(obs).detach(), self.gamma, self.lam)

    orig = PPO.compute_returns
    PPO.compute_returns = returns_cpu
    try:
        alg, pol = build_update(z, "r0/", meta, meta["ranks"][0], "cpu")
    finally:
        PPO.compute_returns = orig
    assert alg._clip_adam is None
    step = alg.optimizer.step

    def clip_step(*a, **k):
        torch.nn.utils.clip_grad_norm_(pol.parameters(), alg.max_grad_norm)
        return step(*a, **k)

    alg.optimizer.step = clip_step
    alg.update = lambda: _torch_update(alg, pol)
    return alg, pol


def run_update(z, meta, device):
    """The fixture's update on `device`: (update_fixtures.check_update's `out`, the PPO)."""
    import torch

    from update_fixtures import build_update, run_recorded_update

    if torch.device(device).type == "cpu":
        alg, pol = build_update_cpu(z, meta)
    else:
        alg, pol = build_update(z, "r0/", meta, meta["ranks"][0], device)
    grads = [None]
    loss, lr_trace = run_recorded_update(alg, grads)
    out = {"loss": loss, "lr_trace": lr_trace, "lr": alg.learning_rate,
           "final": {k: v.detach().cpu() for k, v in pol.state_dict().items()}, "grad_mb0": grads[0]}
    return out, alg
