"""Policy modules (mirrors rsl_rl.modules for the PPO and distillation paths)."""

from .actor_critic import ActorCritic
from .rnd import RandomNetworkDistillation, resolve_rnd_config
from .student_teacher import StudentTeacher
from .symmetry import SignedPermutationSymmetry, resolve_symmetry_config

__all__ = ["ActorCritic", "StudentTeacher", "RandomNetworkDistillation", "resolve_rnd_config",
           "resolve_symmetry_config", "SignedPermutationSymmetry"]
