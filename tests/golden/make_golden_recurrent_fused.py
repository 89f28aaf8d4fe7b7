"""Generate the fixture of the fused recurrent PPO update (rec_d) under tests/golden/ by running the REFERENCE on CPU.

Test infrastructure only, like make_golden_recurrent.py, whose update-case machinery (run_update_case /
make_update_case: the seeded storage, the rollout-consistent stored fields, one reference PPO.update() with the first
mini-batch's gradient, the lr trace and the one-ulp sensitivity envelope) it imports and calls unchanged.  It adds one
case and writes tests/golden/rec_d_*.npz plus tests/golden/golden_recurrent_fused.json.

rec_d is the smallest case the fused update accepts: an LSTM of hidden size 256 in front of 3 x 256
MLPs, 48 observations, 12 actions, T 8, 128 envs in 2 mini-batches -- E = 64 rows, one row tile per mini-batch -- and 2
epochs, so the weight images are rebuilt four times.  The saved hidden states are random, not zero after a done: the
update must restart a row from what the storage holds.

The script asserts that each mini-batch's env slice holds an env that is never done, a done at t = 0, a done at
t = T - 1 and two consecutive dones, and that every optimizer step's KL lies at least 10 % away from both lr-rule
thresholds (the nearest, 0.01704 against 0.02, is 14.8 % away).

Usage:  python tests/golden/make_golden_recurrent_fused.py --reference PATH_TO_RSL_RL_CHECKOUT
"""

from __future__ import annotations

import argparse
import json
import os

import torch

import make_golden_recurrent as MGR

HERE = os.path.dirname(os.path.abspath(__file__))
CASE = dict(T=8, N=128, O=48, A=12, hidden=[256, 256, 256], H=256, L=1, M=2, E=2, rnn_type="lstm", policy_kw={},
            seed=421, sensitivity=True)


def check_dones(cfg):
    """Every mini-batch's env slice exercises each kind of restart."""
    T, N, M = cfg["T"], cfg["N"], cfg["M"]
    nz = MGR.RF.storage_inputs(cfg["seed"] * 100, T, N, cfg["O"], cfg["A"], cfg["L"], cfg["H"], 2)
    d = nz["dones"][:, :, 0]
    E = N // M
    fractions = []
    for i in range(M):
        s = d[:, i * E:(i + 1) * E]
        assert (~s.any(axis=0)).any(), ("no env without a done", i)
        assert s[0].any(), ("no done at t = 0", i)
        assert s[T - 1].any(), ("no done at t = T - 1", i)
        assert (s[:-1] & s[1:]).any(), ("no two consecutive dones", i)
        fractions.append(float(s.mean()))
    return fractions


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="the rsl_rl 3.1.0 checkout (the directory holding rsl_rl/)")
    args = ap.parse_args()
    torch.set_num_threads(1)
    fractions = check_dones(CASE)
    mods = MGR.import_recurrent(args.reference)
    MGR.UPDATE_CASES["d"] = CASE
    meta = MGR.make_update_case(mods, "d")
    for kl in meta["ranks"][0]["kl_trace"]:
        for thr in (2 * MGR.DESIRED_KL, MGR.DESIRED_KL / 2):
            assert abs(kl - thr) >= 0.10 * thr, ("KL within 10 % of an lr-rule threshold", meta["ranks"][0]["kl_trace"])
    meta["done_fractions"] = fractions
    with open(os.path.join(HERE, "golden_recurrent_fused.json"), "w") as f:
        json.dump({"rec_d": meta}, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
