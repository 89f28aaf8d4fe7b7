"""Learning algorithms (mirrors rsl_rl.algorithms: PPO and Distillation)."""

from .distillation import Distillation, distillation_windows
from .ppo import PPO

__all__ = ["PPO", "Distillation", "distillation_windows"]
