"""Learning algorithms (mirrors rsl_rl.algorithms: PPO and Distillation)."""

from .distillation import Distillation, distillation_windows, recurrent_window_plan
from .ppo import PPO

__all__ = ["PPO", "Distillation", "distillation_windows", "recurrent_window_plan"]
