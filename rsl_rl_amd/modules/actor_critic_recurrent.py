"""Recurrent Gaussian actor + critic (rsl_rl/modules/actor_critic_recurrent.py:16-219).

Same constructor, attributes, parameter names and behaviour as the reference: an LSTM / GRU memory in front of the
actor's and the critic's MLP, so configs and checkpoints carry over (memory_a.rnn.weight_ih_l0, actor.0.weight, ...).
The memories run on PyTorch-ROCm's RNN library (networks/memory.py); the MLPs behind them see 2-D rows -- a padded
update batch [T, B, H] is flattened to [T * B, H] first -- so that Linear+ELU stacks take the fused MFMA path of
networks/fused_mlp.py in the rollout and under autograd alike.
"""

from __future__ import annotations

import warnings

import torch
import torch.nn as nn
from torch.distributions import Normal

from .. import kernels
from ..networks import MLP, EmpiricalNormalization, Memory


class ActorCriticRecurrent(nn.Module):
    is_recurrent = True

    def __init__(
        self,
        obs,
        obs_groups,
        num_actions,
        actor_obs_normalization=False,
        critic_obs_normalization=False,
        actor_hidden_dims=[256, 256, 256],
        critic_hidden_dims=[256, 256, 256],
        activation="elu",
        init_noise_std=1.0,
        noise_std_type: str = "scalar",
        state_dependent_std=False,
        rnn_type="lstm",
        rnn_hidden_dim=256,
        rnn_num_layers=1,
        **kwargs,
    ):
        if "rnn_hidden_size" in kwargs:
            warnings.warn("`rnn_hidden_size` is deprecated: pass `rnn_hidden_dim` (it wins when both are given).",
                          DeprecationWarning)
            size = kwargs.pop("rnn_hidden_size")
            if rnn_hidden_dim == 256:  # the old name only counts while the new one is at its default
                rnn_hidden_dim = size
        if kwargs:
            print("ActorCriticRecurrent.__init__ got unexpected arguments, which will be ignored: "
                  + str(list(kwargs)))
        super().__init__()
        if noise_std_type not in ("scalar", "log"):
            raise ValueError(f"Unknown standard deviation type: {noise_std_type}. Should be 'scalar' or 'log'")
        self.obs_groups = obs_groups
        num_actor_obs = self._group_dim(obs, obs_groups["policy"])
        num_critic_obs = self._group_dim(obs, obs_groups["critic"])
        self.state_dependent_std = state_dependent_std
        self.noise_std_type = noise_std_type

        self.memory_a = Memory(num_actor_obs, type=rnn_type, num_layers=rnn_num_layers, hidden_size=rnn_hidden_dim)
        out = [2, num_actions] if state_dependent_std else num_actions
        self.actor = MLP(rnn_hidden_dim, out, actor_hidden_dims, activation)
        self.actor_obs_normalization = actor_obs_normalization
        self.actor_obs_normalizer = EmpiricalNormalization(num_actor_obs) if actor_obs_normalization else nn.Identity()
        print(f"Actor RNN: {self.memory_a}")
        print(f"Actor MLP: {self.actor}")

        self.memory_c = Memory(num_critic_obs, type=rnn_type, num_layers=rnn_num_layers, hidden_size=rnn_hidden_dim)
        self.critic = MLP(rnn_hidden_dim, 1, critic_hidden_dims, activation)
        self.critic_obs_normalization = critic_obs_normalization
        self.critic_obs_normalizer = (
            EmpiricalNormalization(num_critic_obs) if critic_obs_normalization else nn.Identity()
        )
        print(f"Critic RNN: {self.memory_c}")
        print(f"Critic MLP: {self.critic}")

        if state_dependent_std:
            # the std half of the last layer starts at weight 0 and bias = init std (actor_critic_recurrent.py:93-102)
            last = self.actor[-2]
            nn.init.zeros_(last.weight[num_actions:])
            init_bias = init_noise_std if noise_std_type == "scalar" else torch.log(torch.tensor(init_noise_std + 1e-7))
            nn.init.constant_(last.bias[num_actions:], init_bias)
        elif noise_std_type == "scalar":
            self.std = nn.Parameter(init_noise_std * torch.ones(num_actions))
        else:
            self.log_std = nn.Parameter(torch.log(init_noise_std * torch.ones(num_actions)))

        self.distribution = None
        Normal.set_default_validate_args(False)

    @staticmethod
    def _group_dim(obs, groups):
        dim = 0
        for g in groups:
            assert len(obs[g].shape) == 2, "The ActorCriticRecurrent module only supports 1D observations."
            dim += obs[g].shape[-1]
        return dim

    @property
    def action_mean(self):
        return self.distribution.mean

    @property
    def action_std(self):
        return self.distribution.stddev

    @property
    def entropy(self):
        return self.distribution.entropy().sum(dim=-1)

    def reset(self, dones=None):
        self.memory_a.reset(dones)
        self.memory_c.reset(dones)

    def forward(self):
        raise NotImplementedError

    @staticmethod
    def _rows(mlp, x):
        """mlp(x) with the leading dimensions of x folded into rows (the fused MLP kernels take 2-D input)."""
        if x.dim() == 2:
            return mlp(x)
        y = mlp(x.reshape(-1, x.shape[-1]))
        return y.reshape(*x.shape[:-1], *y.shape[1:])

    def update_distribution(self, obs):
        out = self._rows(self.actor, obs)
        if self.state_dependent_std:
            mean, std = torch.unbind(out, dim=-2)
            if self.noise_std_type == "log":
                std = torch.exp(std)
        else:
            mean = out
            std = (self.std if self.noise_std_type == "scalar" else torch.exp(self.log_std)).expand_as(mean)
        self.distribution = Normal(mean, std)

    def act(self, obs, masks=None, hidden_states=None):
        obs = self.actor_obs_normalizer(self.get_actor_obs(obs))
        out_mem = self.memory_a(obs, masks, hidden_states).squeeze(0)
        self.update_distribution(out_mem)
        return self._sample()

    def _sample(self):
        # = self.distribution.sample(): torch.normal(loc, scale) draws normal_(0, 1) and applies .mul_(scale).add_(loc)
        # -- the same values from the same generator stream -- but first checks scale.min() >= 0 with a
        # device-to-host read, once per env step
        loc, scale = self.distribution.loc, self.distribution.scale
        with torch.no_grad():
            return torch.empty_like(loc).normal_().mul_(scale).add_(loc)

    def act_and_evaluate(self, obs):
        """(act(obs), evaluate(obs)) of the rollout step (ppo.py:155-156): when both memories qualify for the fused LSTM
        cell (Memory.cell_ok) their steps run as one launch (kernels.lstm_cell_pair: the bits of the two single
        launches); otherwise each memory takes its own path.  The same values, distribution and generator draws as
        the two calls."""
        a_obs = self.actor_obs_normalizer(self.get_actor_obs(obs))
        c_obs = self.critic_obs_normalizer(self.get_critic_obs(obs))
        ma, mc = self.memory_a, self.memory_c
        if ma.cell_ok(a_obs) and mc.cell_ok(c_obs) and a_obs.shape[0] == c_obs.shape[0]:
            (ha, ca), (hc, cc) = kernels.lstm_cell_pair(a_obs, ma.hidden_states, *ma.cell_operands(),
                                                        c_obs, mc.hidden_states, *mc.cell_operands())
            ma.hidden_states = (ha.unsqueeze(0), ca.unsqueeze(0))
            mc.hidden_states = (hc.unsqueeze(0), cc.unsqueeze(0))
            out_a, out_c = ha, hc
        else:
            out_a, out_c = ma(a_obs).squeeze(0), mc(c_obs).squeeze(0)
        self.update_distribution(out_a)
        actions = self._sample()
        return actions, self._rows(self.critic, out_c)

    def action_distribution_params(self, obs, masks=None, hidden_states=None):
        """The actor's forward for the fused PPO loss (the update's batch mode): (mean, sigma) as act() leaves them in
        the distribution, without drawing a sample nobody reads; sigma is the shared [A] vector (gradient flows to
        std / log_std) unless the std is state dependent."""
        obs = self.actor_obs_normalizer(self.get_actor_obs(obs))
        out_mem = self.memory_a(obs, masks, hidden_states).squeeze(0)
        self.update_distribution(out_mem)
        mean = self.distribution.loc
        if self.state_dependent_std:
            return mean, self.distribution.scale
        return mean, (self.std if self.noise_std_type == "scalar" else torch.exp(self.log_std))

    def act_inference(self, obs):
        obs = self.actor_obs_normalizer(self.get_actor_obs(obs))
        out_mem = self.memory_a(obs).squeeze(0)
        return self._rows(self.actor, out_mem)

    def evaluate(self, obs, masks=None, hidden_states=None):
        obs = self.critic_obs_normalizer(self.get_critic_obs(obs))
        out_mem = self.memory_c(obs, masks, hidden_states).squeeze(0)
        return self._rows(self.critic, out_mem)

    def get_actor_obs(self, obs):
        return torch.cat([obs[g] for g in self.obs_groups["policy"]], dim=-1)

    def get_critic_obs(self, obs):
        return torch.cat([obs[g] for g in self.obs_groups["critic"]], dim=-1)

    def get_actions_log_prob(self, actions):
        return self.distribution.log_prob(actions).sum(dim=-1)

    def get_hidden_states(self):
        return self.memory_a.hidden_states, self.memory_c.hidden_states

    def update_normalization(self, obs):
        if self.actor_obs_normalization:
            self.actor_obs_normalizer.update(self.get_actor_obs(obs))
        if self.critic_obs_normalization:
            self.critic_obs_normalizer.update(self.get_critic_obs(obs))

    def load_state_dict(self, state_dict, strict=True):
        """Load the parameters; returns True: a training of this policy resumes (OnPolicyRunner.load then also
        restores the optimizer and the iteration count)."""
        super().load_state_dict(state_dict, strict=strict)
        return True
