"""Recurrent Gaussian actor + critic (rsl_rl/modules/actor_critic_recurrent.py:16-219).

Same constructor, attributes, parameter names and behaviour as the reference: an LSTM / GRU memory in front of the
actor's and the critic's MLP, so configs and checkpoints carry over (memory_a.rnn.weight_ih_l0, actor.0.weight, ...).
The memories run on PyTorch-ROCm's RNN library (networks/memory.py); the MLPs behind them see 2-D rows -- a padded
update batch [T, B, H] is flattened to [T * B, H] first -- so that Linear+ELU stacks take the fused MFMA path of
networks/fused_mlp.py in the rollout and under autograd alike.

The PPO update of two one-layer LSTMs of hidden size 256 or 512 runs without autograd (manual_update_ok, train_forward,
train_backward): the env-major sequence of a mini-batch goes through T paired launches of the fused
cell's training form, the MLP pair, heads and loss are ActorCritic's (train_forward_rows / train_backward, shared, not
copied), and T paired reverse launches plus the gate blocks' weight-gradient launches write the LSTMs' gradients.
Two one-layer GRUs of hidden size 256 take the same route on the fused GRU cell: act_and_evaluate runs
both steps in one launch (networks/memory.paired_step), and train_tape / train_forward / train_backward are written once
over the kind of the memories (_cell, a kernels.Cell): the kind decides how many state tensors the tape
holds and, through Cell.train_operands / bwd_operands, what a step hands the kernels.  The GRU's tape holds h', the h as
consumed, r, z, n, a and their gradients; its weight gradients come from the blocks r, z, n against the observations
and r, z, a against the h as consumed.
"""

from __future__ import annotations

import warnings
from types import SimpleNamespace

import torch
import torch.nn as nn
from torch.distributions import Normal

from .. import kernels
from ..networks import MLP, EmpiricalNormalization, Memory, fused_mlp
from ..networks.memory import paired_step
from .actor_critic import ActorCritic


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
        self.num_actions = num_actions

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
        """(act(obs), evaluate(obs)) of the rollout step (ppo.py:155-156): when both memories qualify for the fused cell
        of one kind their steps run as one launch (networks/memory.paired_step: the bits of the two single launches);
        otherwise each memory takes its own path.  The same values, distribution and generator draws as the two
        calls."""
        a_obs = self.actor_obs_normalizer(self.get_actor_obs(obs))
        c_obs = self.critic_obs_normalizer(self.get_critic_obs(obs))
        pair = paired_step(self.memory_a, a_obs, self.memory_c, c_obs)
        out_a, out_c = pair if pair is not None else (self.memory_a(a_obs).squeeze(0), self.memory_c(c_obs).squeeze(0))
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

    # ---------------------------------------------------------------- PPO update without autograd
    # the MLP pair, the heads and their backward are ActorCritic's own functions, run on the memories' outputs
    _linears = staticmethod(ActorCritic._linears)
    train_forward_rows = ActorCritic.train_forward_rows
    train_grad_buffers = ActorCritic.train_grad_buffers
    _train_backward_rows = ActorCritic.train_backward

    def manual_update_ok(self, obs, rows: int) -> bool:
        """The PPO update may drive this policy through train_forward / train_backward on mini-batches of `rows` envs:
        an unmodified class with unmodified memories, both one-layer LSTMs or both one-layer GRUs the fused cell of
        their kind takes at that row count (hidden size 256, or 512 on the `_h` forms), fused or wide Linear+ELU MLPs
        (those of ActorCritic.manual_update_structure_ok), a shared std, every parameter trainable, fp32
        observations on a ROCm device, and RSLRL_LSTM_CELL (RSLRL_GRU_CELL for GRUs) not 0.  An LSTM policy of hidden
        size 512, or with wide MLPs, qualifies from kernels.RNN_H512_LSTM_UPDATE_MIN_ROWS rows on."""
        cls = type(self)
        if (cls.action_distribution_params is not ActorCriticRecurrent.action_distribution_params
                or cls.evaluate is not ActorCriticRecurrent.evaluate or cls.act is not ActorCriticRecurrent.act):
            return False
        cell = self._cell()
        if cell is None or self.state_dependent_std or not cell.enabled():
            return False
        if self.memory_a.rnn.hidden_size != self.memory_c.rnn.hidden_size:  # one H for the tape and the pair launches
            return False
        groups = self.obs_groups["policy"] + self.obs_groups["critic"]
        if not all(obs[g].is_cuda and obs[g].dtype == torch.float32 for g in groups):
            return False
        for mem, width in ((self.memory_a, self._group_width(obs, "policy")),
                           (self.memory_c, self._group_width(obs, "critic"))):
            rnn = mem.rnn
            if (type(mem) is not Memory or not rnn.bias or rnn.bidirectional
                    or getattr(rnn, "proj_size", 0) != 0 or rnn.input_size != width
                    or not cell.takes(rows, width, rnn.hidden_size, rnn.num_layers)):
                return False
        def ok(mlp):  # the stacks ActorCritic.manual_update_structure_ok admits
            return getattr(mlp, "_fused", False) or (getattr(mlp, "_wide", False) and fused_mlp.wide_enabled())

        if not (ok(self.actor) and ok(self.critic)):
            return False
        # the ground DESIGN §27 added (hidden size 512, wide MLPs behind the memories): an LSTM policy's update is ahead
        # of autograd from kernels.RNN_H512_LSTM_UPDATE_MIN_ROWS rows on and stays there below
        added = (self.memory_a.rnn.hidden_size != kernels.LSTM_CELL_HIDDEN
                 or not (getattr(self.actor, "_fused", False) and getattr(self.critic, "_fused", False)))
        if cell is kernels.LSTM and added and rows < kernels.RNN_H512_LSTM_UPDATE_MIN_ROWS:
            return False
        return all(p.requires_grad for p in self.parameters())

    def _cell(self):
        """The kernels.Cell of the two memories when both hold exactly that kind of RNN, else None (mixed policies stay
        on autograd)."""
        cell = kernels.cell_of(self.memory_a.rnn)
        return cell if cell is kernels.cell_of(self.memory_c.rnn) else None

    def _group_width(self, obs, name):
        return sum(obs[g].shape[-1] for g in self.obs_groups[name])

    def train_tape(self, T: int, E: int, device) -> SimpleNamespace:
        """The sequence tape of one update, per LSTM memory 11 [T, E, H] fp32 tensors (H the memories' hidden size):
        h', c' (`out`), the h as consumed, the four activated gates and the four gate gradients (gate-major, so that
        each gate block is one [T * E, H] operand of the weight-gradient kernel), plus the two alternating carries d c; per GRU memory 10:
        h', the h as consumed, r, z, n, a and their four gradients, plus the two alternating carries dhz."""
        f32 = dict(dtype=torch.float32, device=device)
        H = self.memory_a.rnn.hidden_size
        n_state = self._cell().n_state
        return SimpleNamespace(mem=[SimpleNamespace(
            out=tuple(torch.empty(T, E, H, **f32) for _ in range(n_state)), hin=torch.empty(T, E, H, **f32),
            gates=torch.empty(4, T, E, H, **f32), dg=torch.empty(4, T, E, H, **f32),
            carry=torch.empty(2, E, H, **f32)) for _ in range(2)])

    def train_forward(self, x_a, x_c, reset, hid_a, hid_c, seq, value_head=None, actor_head=None):
        """The update's forward on one env-major sequence without an autograd graph (call under torch.no_grad()): x_a /
        x_c the normalised observations [T, E, D], reset the uint8 [T, E] matrix and hid_a / hid_c the restart slices
        [T, E, H] of RolloutStorage.recurrent_sequence_generator ((h, c) for LSTMs, the bare h for GRUs), seq a
        train_tape.  T paired launches of the
        cell's training form -- a row whose reset flag is set restarts from the storage's saved state of that step --
        then ActorCritic.train_forward_rows on the [T * E, H] views of the stored h.  Returns its (mean, sigma,
        value, tape).  The memories' hidden_states are not touched."""
        T, E = reset.shape
        cell, mems = self._cell(), (self.memory_a.rnn, self.memory_c.rnn)
        seq.x, seq.reset = (x_a, x_c), reset
        restarts = (cell.unpack(hid_a), cell.unpack(hid_c))
        # the weights move every optimizer step: both images are rebuilt per mini-batch
        images = [cell.image(r.weight_ih_l0, r.weight_hh_l0) for r in mems]
        seq.steps = []  # per t and memory the step as kernels' *_operands take it; train_backward reads it again
        for t in range(T):
            rst = reset[t] if t else None
            steps = [(prev[1] if t else tuple([r[0] for r in rs]), tuple([o[t] for o in m.out]), rst,
                      tuple([r[t] for r in rs]) if t else None, m.hin[t])
                     for m, rs, prev in zip(seq.mem, restarts, seq.steps[-1] if t else (None, None))]
            cell.train_pair(*[cell.train_operands(x[t], image, rnn.bias_ih_l0, rnn.bias_hh_l0, m.gates[:, t], s, s[4])
                              for m, rnn, x, image, s in zip(seq.mem, mems, seq.x, images, steps)])
            seq.steps.append(steps)
        H = self.memory_a.rnn.hidden_size
        return self.train_forward_rows(seq.mem[0].out[0].view(T * E, H), seq.mem[1].out[0].view(T * E, H),
                                       value_head=value_head, actor_head=actor_head)

    def train_backward(self, tape, g_mean, g_sigma, g_value, std, slot, seq):
        """Backward of train_forward into the gradient slots `slot(param)`: ActorCritic's MLP-pair backward down to
        d loss / d h, T paired reverse launches of the cell (no gradient crosses a restart), and the gate blocks'
        weight gradients over all T * E rows (fused_mlp.lstm_gate_wgrads: dW_ih against the observations, dW_hh
        against the h as consumed, db_ih = db_hh = the column sums; for GRUs gru_gate_wgrads) -- the two memories' in
        paired launches where their shapes agree."""
        T, E = seq.reset.shape
        H, rows = self.memory_a.rnn.hidden_size, T * E
        dhs = self._train_backward_rows(tape, g_mean, g_sigma, g_value, std, slot, need_dx=True)
        cell, mems = self._cell(), (self.memory_a.rnn, self.memory_c.rnn)
        whh_t = [cell.whh_t_image(r.weight_hh_l0) for r in mems]
        for t in range(T - 1, -1, -1):
            after = seq.steps[t + 1] if t < T - 1 else (None, None)  # the chain ends at the sequence's last step
            cell.bwd_pair(*[cell.bwd_operands(
                dh.view(T, E, H)[t], m.gates[:, t], s, m.dg[:, t + 1] if nxt else None,
                m.carry[(t + 1) & 1] if nxt else None, nxt[2] if nxt else None, img, m.dg[:, t], m.carry[t & 1])
                for m, dh, img, s, nxt in zip(seq.mem, dhs, whh_t, seq.steps[t], after)])
        fused_mlp.GATE_WGRADS[cell.name](
            [m.dg.view(4, rows, H) for m in seq.mem], [x.view(rows, -1) for x in seq.x],
            [m.hin.view(rows, H) for m in seq.mem], [fused_mlp.gate_grad_views(cell, r, slot) for r in mems])

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
