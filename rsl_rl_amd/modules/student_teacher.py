"""Student MLP + frozen teacher MLP for distillation (rsl_rl/modules/student_teacher.py:15-206).

Same constructor, attributes, parameter order and state_dict keys as the reference (`std` / `log_std`, `student.*`,
optional `student_obs_normalizer.*`, `teacher.*`, optional `teacher_obs_normalizer.*`), so configs and checkpoints
carry over -- including load_state_dict's three branches: an RL checkpoint (`actor.*`) fills the teacher, a
distillation checkpoint resumes, anything else is an error.  In addition `act_and_evaluate()` runs the rollout
step's student and teacher forwards with their same-shape layers batched into one launch each, as
ActorCritic.act_and_evaluate does for the actor and the critic.
"""

from __future__ import annotations

import torch
import torch.nn as nn
from torch.distributions import Normal

from ..networks import MLP, EmpiricalNormalization
from ..networks.fused_mlp import fused_mlp_forward_pair
from .actor_critic import ActorCritic


class StudentTeacher(nn.Module):
    is_recurrent = False

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
        **kwargs,
    ):
        if kwargs:
            print("StudentTeacher.__init__ got unexpected arguments, which will be ignored: " + str(list(kwargs)))
        super().__init__()
        self.loaded_teacher = False  # indicates if teacher has been loaded
        self.obs_groups = obs_groups
        num_student_obs = self._group_dim(obs, obs_groups["policy"])
        num_teacher_obs = self._group_dim(obs, obs_groups["teacher"])

        self.student = MLP(num_student_obs, num_actions, student_hidden_dims, activation)
        self.student_obs_normalization = student_obs_normalization
        self.student_obs_normalizer = (
            EmpiricalNormalization(num_student_obs) if student_obs_normalization else nn.Identity()
        )
        print(f"Student MLP: {self.student}")

        self.teacher = MLP(num_teacher_obs, num_actions, teacher_hidden_dims, activation)
        self.teacher.eval()
        self.teacher_obs_normalization = teacher_obs_normalization
        self.teacher_obs_normalizer = (
            EmpiricalNormalization(num_teacher_obs) if teacher_obs_normalization else nn.Identity()
        )
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

    @staticmethod
    def _group_dim(obs, groups):
        dim = 0
        for g in groups:
            assert len(obs[g].shape) == 2, "The StudentTeacher module only supports 1D observations."
            dim += obs[g].shape[-1]
        return dim

    def reset(self, dones=None, hidden_states=None):
        pass

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
        """mean: the student's output when it was already computed (act_and_evaluate)."""
        mean = self.student(obs) if mean is None else mean
        self.distribution = Normal(mean, self._std().expand_as(mean))

    # the sample without Normal.sample()'s device-to-host check, in one launch on a ROCm device (same values and
    # generator draws as self.distribution.sample(); see ActorCritic._sample)
    _sample = ActorCritic._sample

    def act(self, obs):
        obs = self.student_obs_normalizer(self.get_student_obs(obs))
        self.update_distribution(obs)
        return self._sample()

    def act_inference(self, obs):
        obs = self.student_obs_normalizer(self.get_student_obs(obs))
        return self.student(obs)

    def evaluate(self, obs):
        obs = self.teacher_obs_normalizer(self.get_teacher_obs(obs))
        with torch.no_grad():
            return self.teacher(obs)

    def act_and_evaluate(self, obs):
        """(act(obs), evaluate(obs)) of the rollout step (distillation.py:87-88) with the student's and the teacher's
        same-shape layers batched into one launch each (networks/fused_mlp.fused_mlp_forward_pair); the same values,
        distribution and generator draws as the two calls.  Falls back to them when the pair does not qualify
        (gradients wanted, different hidden shapes, a CPU tensor)."""
        s_obs = self.student_obs_normalizer(self.get_student_obs(obs))
        t_obs = self.teacher_obs_normalizer(self.get_teacher_obs(obs))
        pair = fused_mlp_forward_pair(self.student, s_obs, self.teacher, t_obs) if s_obs.is_cuda else None
        if pair is None:
            self.update_distribution(s_obs)
            actions = self._sample()
            with torch.no_grad():
                return actions, self.teacher(t_obs)
        self.update_distribution(s_obs, mean=pair[0])
        return self._sample(), pair[1]

    @staticmethod
    def _concat(obs, groups):
        # a single group is used as is (the reference's torch.cat of one tensor is a pure copy)
        return obs[groups[0]] if len(groups) == 1 else torch.cat([obs[g] for g in groups], dim=-1)

    def get_student_obs(self, obs):
        return self._concat(obs, self.obs_groups["policy"])

    def get_teacher_obs(self, obs):
        return self._concat(obs, self.obs_groups["teacher"])

    def get_hidden_states(self):
        return None

    def detach_hidden_states(self, dones=None):
        pass

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
        """Load the student's and the teacher's parameters (student_teacher.py:168-206).  Returns whether this resumes
        a distillation run (True) or only filled the teacher from an RL checkpoint (False); the runner's load() uses
        it to decide about the optimizer state and the iteration counter."""
        if any("actor" in key for key in state_dict.keys()):  # parameters of an RL training run
            teacher, teacher_norm = {}, {}
            for key, value in state_dict.items():
                if "actor." in key:
                    teacher[key.replace("actor.", "")] = value
                if "actor_obs_normalizer." in key:
                    teacher_norm[key.replace("actor_obs_normalizer.", "")] = value
            self.teacher.load_state_dict(teacher, strict=strict)
            self.teacher_obs_normalizer.load_state_dict(teacher_norm, strict=strict)
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
