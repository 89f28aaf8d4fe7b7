"""Helpers of the fused recurrent PPO update's tests: the rec_d fixture's metadata, the reference's GAE
written in torch (compute_returns has no CPU path), and the env-major sequence form of the update's forward and loss
in plain torch -- LSTM steps with a `where`-merge of the restart states, the MLPs, the PPO loss written out -- on any
device and dtype, under autograd."""

import json
import os

import torch
import torch.nn.functional as F

import recurrent_fixtures as RF


def load_meta():
    with open(os.path.join(RF.GOLDEN, "golden_recurrent_fused.json")) as f:
        return json.load(f)


def gae_torch(st, last_values, gamma, lam):
    """rollout_storage.py:106-130 of the reference on the storage's tensors: returns, then advantages normalised over
    the whole storage."""
    T = st.num_transitions_per_env
    advantage = 0
    for step in reversed(range(T)):
        next_values = last_values if step == T - 1 else st.values[step + 1]
        not_terminal = 1.0 - st.dones[step].float()
        delta = st.rewards[step] + not_terminal * gamma * next_values - st.values[step]
        advantage = delta + not_terminal * gamma * lam * advantage
        st.returns[step] = advantage + st.values[step]
    st.advantages.copy_(st.returns - st.values)
    st.advantages.copy_((st.advantages - st.advantages.mean()) / (st.advantages.std() + 1e-8))


def build_update_cpu(z, meta):
    """RF.build_update on CPU tensors with the returns from gae_torch."""
    alg, pol = RF.build_update(z, meta, "cpu", compute_returns=False)
    nz = RF.storage_inputs(meta["ranks"][0]["noise_seed"], meta["T"], meta["N"], meta["O"], meta["A"], meta["L"],
                           meta["H"], meta["n_states"])
    with torch.inference_mode():
        last_values = pol.evaluate({"policy": torch.from_numpy(nz["last_obs"])}).detach()
        gae_torch(alg.storage, last_values, alg.gamma, alg.lam)
    return alg, pol


def lstm_sequence(rnn, x, reset, restart):
    """h [T, E, H] of a one-layer nn.LSTM's weights over the env-major sequence x [T, E, D]: step t continues from
    step t - 1 except in the rows whose reset[t] is set, which restart from restart = (h, c) [T, E, H] at t (every row
    at t = 0); the merge is a torch.where, so no gradient crosses a restart."""
    w_ih, w_hh, b_ih, b_hh = rnn.weight_ih_l0, rnn.weight_hh_l0, rnn.bias_ih_l0, rnn.bias_hh_l0
    h, c = restart[0][0], restart[1][0]
    out = []
    for t in range(x.shape[0]):
        if t:
            r = reset[t].bool().unsqueeze(-1)
            h, c = torch.where(r, restart[0][t], h), torch.where(r, restart[1][t], c)
        i, f, g, o = (F.linear(x[t], w_ih, b_ih) + F.linear(h, w_hh, b_hh)).chunk(4, dim=-1)
        c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
        h = torch.sigmoid(o) * torch.tanh(c)
        out.append(h)
    return torch.stack(out)


def sequence_loss(alg, pol, batch):
    """The PPO loss of one recurrent_sequence_generator mini-batch, written out as RF.torch_baseline_update does."""
    obs, actions, tv, adv, ret, old_lp, old_mu, old_sigma, (hid_a, hid_c), reset = batch
    x = pol.actor_obs_normalizer(pol.get_actor_obs(obs))
    mean = pol._rows(pol.actor, lstm_sequence(pol.memory_a.rnn, x, reset, hid_a))
    std = (pol.std if pol.noise_std_type == "scalar" else torch.exp(pol.log_std)).expand_as(mean)
    dist = torch.distributions.Normal(mean, std)
    logp = dist.log_prob(actions).sum(-1)
    entropy = dist.entropy().sum(-1)
    xc = pol.critic_obs_normalizer(pol.get_critic_obs(obs))
    value = pol._rows(pol.critic, lstm_sequence(pol.memory_c.rnn, xc, reset, hid_c))
    ratio = torch.exp(logp - old_lp.squeeze(-1))
    a = adv.squeeze(-1)
    surrogate = torch.max(-a * ratio, -a * ratio.clamp(1.0 - alg.clip_param, 1.0 + alg.clip_param)).mean()
    clipped = tv + (value - tv).clamp(-alg.clip_param, alg.clip_param)
    value_loss = torch.max((value - ret).square(), (clipped - ret).square()).mean()
    return surrogate + alg.value_loss_coef * value_loss - alg.entropy_coef * entropy.mean()
