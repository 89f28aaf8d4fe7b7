"""PPO.update and Distillation.update are one step per strategy: the host lr rule and the autograd
backward tail are written once in algorithms/ppo.py, no function under algorithms/ needs a complexity waiver, and none
but the two constructors is longer than 100 lines.  A source check, modelled on test_loss_one_definition."""

import ast
import glob
import os
import re

from conftest import ROOT

SRC = os.path.join(ROOT, "rsl_rl_amd", "algorithms")


def sources():
    return {os.path.basename(p): open(p).read() for p in sorted(glob.glob(os.path.join(SRC, "*.py")))}


def test_no_complexity_waiver():
    for name, text in sources().items():
        assert "noqa: C901" not in text, name


def test_lr_rule_and_autograd_tail_are_called_at_one_place():
    ppo = sources()["ppo.py"]
    assert len(re.findall(r"(?<!def )\badapt_learning_rate\(", ppo)) == 1
    assert len(re.findall(r"torch\.autograd\.backward\(", ppo)) == 1


def test_function_lengths():
    lengths = {}
    for name, text in sources().items():
        for node in ast.walk(ast.parse(text)):
            if isinstance(node, (ast.FunctionDef, ast.AsyncFunctionDef)):
                lengths[(name, node.name, node.lineno)] = node.end_lineno - node.lineno + 1
    long = {k: v for k, v in lengths.items() if v > 100 and k[1] != "__init__"}
    assert not long, long
    assert max(v for k, v in lengths.items() if k[:2] == ("ppo.py", "update")) <= 100
