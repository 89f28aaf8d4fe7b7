"""Runners (mirrors rsl_rl.runners: PPO and distillation)."""

from .on_policy_runner import OnPolicyRunner
from .distillation_runner import DistillationRunner

__all__ = ["OnPolicyRunner", "DistillationRunner"]
