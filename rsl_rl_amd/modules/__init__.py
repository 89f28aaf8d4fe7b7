"""Policy modules (mirrors rsl_rl.modules for the PPO and distillation paths)."""

from .actor_critic import ActorCritic
from .actor_critic_recurrent import ActorCriticRecurrent
from .rnd import RandomNetworkDistillation, resolve_rnd_config
from .student_teacher import StudentTeacher
from .student_teacher_recurrent import StudentTeacherRecurrent
from .symmetry import SignedPermutationSymmetry, resolve_symmetry_config

__all__ = ["ActorCritic", "ActorCriticRecurrent", "StudentTeacher", "StudentTeacherRecurrent",
           "RandomNetworkDistillation", "resolve_rnd_config", "resolve_symmetry_config", "SignedPermutationSymmetry"]
