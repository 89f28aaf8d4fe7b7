"""Recurrent student (memory + MLP) and frozen teacher for distillation
(rsl_rl/modules/student_teacher_recurrent.py:16-249).

Same constructor, attributes, registration order and state_dict keys as the reference (`std` / `log_std`,
`memory_s.rnn.*`, `student.*`, optional `student_obs_normalizer.*`, `memory_t.rnn.*` when the teacher is recurrent,
`teacher.*`, optional `teacher_obs_normalizer.*`), so configs and checkpoints carry over -- including
load_state_dict's three branches: an RL checkpoint fills the teacher (`actor.*`, and `memory_a.*` into `memory_t` for
a recurrent teacher), a distillation checkpoint resumes, anything else is an error.

The construction is the reference's as it stands, oddities included: with `teacher_recurrent=True` the
teacher's normaliser is sized `rnn_hidden_dim` although evaluate() applies it to the teacher observations in front of
the memory, so teacher normalisation with a recurrent teacher only works when the two widths agree.

The memories are networks/memory.Memory: reset / detach keep the reference's semantics without a boolean index, and
a qualifying LSTM or GRU takes its rollout steps on the fused cell.  `act_and_evaluate()` runs the rollout step's two
memory steps as one launch when both qualify (networks/memory.paired_step) and the two MLPs through
the pair forward when their shapes allow it.
"""

from __future__ import annotations

import warnings

import torch
import torch.nn as nn
from torch.distributions import Normal

from ..networks import MLP, EmpiricalNormalization, Memory
from ..networks.fused_mlp import fused_mlp_forward_pair
from ..networks.memory import paired_step
from .actor_critic import ActorCritic
from .student_teacher import StudentTeacher


class StudentTeacherRecurrent(nn.Module):
    is_recurrent = True

    def __init__(
        self,
        obs,
        obs_groups,
        num_actions,
        student_obs_normalization=False,
        teacher_obs_normalization=False,
        student_hidden_dims=[256, 256, 256],
        teacher_hidden_dims=[256, 256, 256],
        activation="elu",
        init_noise_std=0.1,
        noise_std_type: str = "scalar",
        rnn_type="lstm",
        rnn_hidden_dim=256,
        rnn_num_layers=1,
        teacher_recurrent=False,
        **kwargs,
    ):
        if "rnn_hidden_size" in kwargs:
            warnings.warn("`rnn_hidden_size` is deprecated: pass `rnn_hidden_dim` (it wins when both are given).",
                          DeprecationWarning)
            if rnn_hidden_dim == 256:  # the old name only counts while the new one is at its default
                rnn_hidden_dim = kwargs.pop("rnn_hidden_size")
        if kwargs:
            print("StudentTeacherRecurrent.__init__ got unexpected arguments, which will be ignored: "
                  + str(list(kwargs)))
        super().__init__()
        self.loaded_teacher = False  # indicates if teacher has been loaded
        self.teacher_recurrent = teacher_recurrent  # indicates if teacher is recurrent too
        self.obs_groups = obs_groups
        num_student_obs = StudentTeacher._group_dim(obs, obs_groups["policy"])
        num_teacher_obs = StudentTeacher._group_dim(obs, obs_groups["teacher"])

        self.memory_s = Memory(num_student_obs, type=rnn_type, num_layers=rnn_num_layers, hidden_size=rnn_hidden_dim)
        self.student = MLP(rnn_hidden_dim, num_actions, student_hidden_dims, activation)
        self.student_obs_normalization = student_obs_normalization
        self.student_obs_normalizer = (
            EmpiricalNormalization(num_student_obs) if student_obs_normalization else nn.Identity()
        )
        print(f"Student RNN: {self.memory_s}")
        print(f"Student MLP: {self.student}")

        if teacher_recurrent:
            self.memory_t = Memory(num_teacher_obs, type=rnn_type, num_layers=rnn_num_layers,
                                   hidden_size=rnn_hidden_dim)
            num_teacher_obs = rnn_hidden_dim  # (also sizes the teacher's normaliser below, as in the reference)
        self.teacher = MLP(num_teacher_obs, num_actions, teacher_hidden_dims, activation)
        self.teacher_obs_normalization = teacher_obs_normalization
        self.teacher_obs_normalizer = (
            EmpiricalNormalization(num_teacher_obs) if teacher_obs_normalization else nn.Identity()
        )
        if teacher_recurrent:
            print(f"Teacher RNN: {self.memory_t}")
        print(f"Teacher MLP: {self.teacher}")

        self.noise_std_type = noise_std_type
        if noise_std_type == "scalar":
            self.std = nn.Parameter(init_noise_std * torch.ones(num_actions))
        elif noise_std_type == "log":
            self.log_std = nn.Parameter(torch.log(init_noise_std * torch.ones(num_actions)))
        else:
            raise ValueError(f"Unknown standard deviation type: {noise_std_type}. Should be 'scalar' or 'log'")

        self.distribution = None
        Normal.set_default_validate_args(False)

    def reset(self, dones=None, hidden_states=None):
        if hidden_states is None:
            hidden_states = (None, None)
        self.memory_s.reset(dones, hidden_states[0])
        if self.teacher_recurrent:
            self.memory_t.reset(dones, hidden_states[1])

    def forward(self):
        raise NotImplementedError

    @property
    def action_mean(self):
        return self.distribution.mean

    @property
    def action_std(self):
        return self.distribution.stddev

    @property
    def entropy(self):
        return self.distribution.entropy().sum(dim=-1)

    def _std(self):
        return self.std if self.noise_std_type == "scalar" else torch.exp(self.log_std)

    def update_distribution(self, obs, mean=None):
        """obs: the student memory's output; mean: the student's output when it was already computed
        (act_and_evaluate)."""
        mean = self.student(obs) if mean is None else mean
        self.distribution = Normal(mean, self._std().expand_as(mean))

    # the sample without Normal.sample()'s device-to-host check (same values and generator draws; see
    # ActorCritic._sample)
    _sample = ActorCritic._sample

    def act(self, obs):
        obs = self.student_obs_normalizer(self.get_student_obs(obs))
        out_mem = self.memory_s(obs).squeeze(0)
        self.update_distribution(out_mem)
        return self._sample()

    def act_inference(self, obs):
        obs = self.student_obs_normalizer(self.get_student_obs(obs))
        out_mem = self.memory_s(obs).squeeze(0)
        return self.student(out_mem)

    def evaluate(self, obs):
        obs = self.teacher_obs_normalizer(self.get_teacher_obs(obs))
        with torch.no_grad():
            if self.teacher_recurrent:
                self.memory_t.eval()
                obs = self.memory_t(obs).squeeze(0)
            return self.teacher(obs)

    def act_and_evaluate(self, obs):
        """(act(obs), evaluate(obs)) of the rollout step (distillation.py:87-88): when both memories qualify for the
        fused cell of one kind their steps run as one launch (networks/memory.paired_step: the bits of the two single
        launches), and the two MLPs go through the pair forward when their shapes allow it
        (networks/fused_mlp.fused_mlp_forward_pair); otherwise each takes its own path.  The same values,
        distribution and generator draws as the two calls."""
        s_obs = self.student_obs_normalizer(self.get_student_obs(obs))
        t_obs = self.teacher_obs_normalizer(self.get_teacher_obs(obs))
        ms = self.memory_s
        if self.teacher_recurrent:
            mt = self.memory_t
            mt.eval()
            pair = paired_step(ms, s_obs, mt, t_obs)
            if pair is not None:
                s_in, t_in = pair
            else:
                s_in = ms(s_obs).squeeze(0)
                with torch.no_grad():
                    t_in = mt(t_obs).squeeze(0)
        else:
            s_in, t_in = ms(s_obs).squeeze(0), t_obs
        pair = fused_mlp_forward_pair(self.student, s_in, self.teacher, t_in) if s_in.is_cuda else None
        if pair is None:
            self.update_distribution(s_in)
            actions = self._sample()
            with torch.no_grad():
                return actions, self.teacher(t_in)
        self.update_distribution(s_in, mean=pair[0])
        return self._sample(), pair[1]

    get_student_obs = StudentTeacher.get_student_obs
    get_teacher_obs = StudentTeacher.get_teacher_obs
    _concat = staticmethod(StudentTeacher._concat)

    def get_hidden_states(self):
        if self.teacher_recurrent:
            return self.memory_s.hidden_states, self.memory_t.hidden_states
        return self.memory_s.hidden_states, None

    def detach_hidden_states(self, dones=None):
        self.memory_s.detach_hidden_states(dones)
        if self.teacher_recurrent:
            self.memory_t.detach_hidden_states(dones)

    def train(self, mode=True):
        super().train(mode)
        # the teacher (and its normaliser) stay in eval mode
        self.teacher.eval()
        self.teacher_obs_normalizer.eval()
        return self

    def update_normalization(self, obs):
        if self.student_obs_normalization:
            self.student_obs_normalizer.update(self.get_student_obs(obs))

    def load_state_dict(self, state_dict, strict=True):
        """Load the student's and the teacher's parameters (student_teacher_recurrent.py:204-249).  Returns whether
        this resumes a distillation run (True) or only filled the teacher from an RL checkpoint (False); the runner's
        load() uses it to decide about the optimizer state and the iteration counter."""
        if any("actor" in key for key in state_dict.keys()):  # parameters of an RL training run
            teacher, teacher_norm, memory_t = {}, {}, {}
            for key, value in state_dict.items():
                if "actor." in key:
                    teacher[key.replace("actor.", "")] = value
                if "actor_obs_normalizer." in key:
                    teacher_norm[key.replace("actor_obs_normalizer.", "")] = value
                if "memory_a." in key:
                    memory_t[key.replace("memory_a.", "")] = value
            self.teacher.load_state_dict(teacher, strict=strict)
            self.teacher_obs_normalizer.load_state_dict(teacher_norm, strict=strict)
            if self.teacher_recurrent:  # the actor's memory of an ActorCriticRecurrent checkpoint
                self.memory_t.load_state_dict(memory_t, strict=strict)
            self.loaded_teacher = True
            self.teacher.eval()
            self.teacher_obs_normalizer.eval()
            return False
        if any("student" in key for key in state_dict.keys()):  # parameters of a distillation run
            super().load_state_dict(state_dict, strict=strict)
            self.loaded_teacher = True
            self.teacher.eval()
            self.teacher_obs_normalizer.eval()
            return True
        raise ValueError("state_dict does not contain student or teacher parameters")
