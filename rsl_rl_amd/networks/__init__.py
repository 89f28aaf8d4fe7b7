"""Network building blocks (mirrors rsl_rl.networks for the PPO path)."""

from .memory import Memory
from .mlp import MLP
from .normalization import EmpiricalDiscountedVariationNormalization, EmpiricalNormalization

__all__ = ["MLP", "Memory", "EmpiricalNormalization", "EmpiricalDiscountedVariationNormalization"]
