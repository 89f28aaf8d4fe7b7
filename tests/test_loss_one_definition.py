"""The PPO loss arithmetic is written once, in csrc/ppo_loss_common.h: the four kernels that evaluate it (the lane and
quad kernels of ppo_loss.hip, ppo_loss_sym.hip, the actor head of mlp_heads.hip) call its helpers, and the GPU tests
compare their outputs bit for bit.  A source-text check, modelled on test_every_epilogue_uses_the_same_polynomial: the
expressions, constants and helpers named here occur in that header and nowhere else in csrc/."""

import glob
import os
import re

from conftest import ROOT

SRC = os.path.join(ROOT, "rsl_rl_amd", "csrc")
HOME = "ppo_loss_common.h"


def sources():
    paths = sorted(glob.glob(os.path.join(SRC, "*.hip")) + glob.glob(os.path.join(SRC, "*.h")))
    return {os.path.basename(p): open(p).read() for p in paths}


def holders(src, needle):
    return [name for name, text in src.items() if needle in text]


def test_loss_expressions_live_in_one_header():
    src = sources()
    for needle in ("expf(logp - old_logp)", "max_grads(", "1.0e-5f", "kLogSqrt2Pi", "kEntC"):
        assert holders(src, needle) == [HOME], (needle, holders(src, needle))


def test_row_helpers_and_tail_are_defined_once():
    src = sources()
    for pattern, home in ((r"void load_row\(", HOME), (r"void store_row\(", HOME),
                          (r"void ppo_tail_device\(", "optim.hip")):
        defs = [name for name, text in src.items() for _ in re.finditer(pattern, text)]
        assert defs == [home], (pattern, defs)
    assert holders(src, "sym_load_row") == [] and holders(src, "sym_store_row") == []
    # both of the tail's launches call the one definition
    assert len(re.findall(r"(?<!void )ppo_tail_device\(", src["optim.hip"])) == 2


def test_every_loss_kernel_calls_the_shared_helpers():
    src = sources()
    for user in ("ppo_loss.hip", "ppo_loss_sym.hip", "mlp_heads.hip"):
        for helper in ("surrogate", "kl_term_exact", "logp_term", "normal_grads", "value_loss", "sigma_consts",
                       "loss_scalars"):
            assert re.search(r"(?<!\w)%s\(" % helper, src[user]), (user, helper)
    for user in ("ppo_loss.hip", "mlp_heads.hip"):  # the kernels with the per-action-constant KL and its knob
        for helper in ("kl_term_fast", "kl_fast_consts", "kl_fast_enabled"):
            assert re.search(r"(?<!\w)%s\(" % helper, src[user]), (user, helper)
    assert holders(src, "RSLRL_KL_FAST\"") == [HOME]


def test_moved_entry_points_left_ppo_loss():
    src = sources()
    for symbol, home in (("int rslrl_launch_timing_enable(", "launch_timing.hip"),
                         ("int rslrl_ppo_update_tail(", "optim.hip")):
        assert holders(src, symbol) == [home], (symbol, holders(src, symbol))
    makefile = open(os.path.join(SRC, "Makefile")).read()
    assert re.search(r"^HIP_SRCS :=.*\blaunch_timing\.hip\b", makefile, re.M)
