"""Generate the fixture of the fused recurrent PPO update of a GRU policy (rec_e) under tests/golden/ by running the
REFERENCE on CPU.

Test infrastructure only, like make_golden_recurrent_fused.py, on which it is modelled: the update-case machinery of
make_golden_recurrent.py (run_update_case / make_update_case) is imported and called unchanged.  It adds one case and
writes tests/golden/rec_e_*.npz plus tests/golden/golden_recurrent_gru.json.

rec_e is rec_d's shape with rnn_type="gru" (DESIGN.md §19): a GRU of hidden size 256 in front of 3 x 256 MLPs, 48
observations, 12 actions, T 8, 128 envs in 2 mini-batches -- E = 64 rows, one row tile per mini-batch -- and 2 epochs.
One saved state per memory (n_states 1), random, not zero after a done: the update must restart a row from what the
storage holds.

The script asserts rec_d's two conditions: each mini-batch's env slice holds an env that is never done, a done at
t = 0, a done at t = T - 1 and two consecutive dones, and every optimizer step's KL lies at least 10 % away from both
lr-rule thresholds.  Seed 449 meets both (KLs 1.2e-4, 0.01174, 0.01586, 0.01496: the nearest is 20.7 % from 0.02);
seeds 431, 433, 439 and 443 do not.

Usage:  python tests/golden/make_golden_recurrent_gru.py --reference PATH_TO_RSL_RL_CHECKOUT
"""

from __future__ import annotations

import argparse
import json
import os

import torch

import make_golden_recurrent as MGR
import make_golden_recurrent_fused as MGF

HERE = os.path.dirname(os.path.abspath(__file__))
CASE = dict(MGF.CASE, rnn_type="gru", seed=449)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="the rsl_rl 3.1.0 checkout (the directory holding rsl_rl/)")
    args = ap.parse_args()
    torch.set_num_threads(1)
    fractions = MGF.check_dones(CASE)  # (the dones are drawn before the saved states: their number does not matter)
    mods = MGR.import_recurrent(args.reference)
    MGR.UPDATE_CASES["e"] = CASE
    meta = MGR.make_update_case(mods, "e")
    assert meta["n_states"] == 1
    for kl in meta["ranks"][0]["kl_trace"]:
        for thr in (2 * MGR.DESIRED_KL, MGR.DESIRED_KL / 2):
            assert abs(kl - thr) >= 0.10 * thr, ("KL within 10 % of an lr-rule threshold", meta["ranks"][0]["kl_trace"])
    meta["done_fractions"] = fractions
    with open(os.path.join(HERE, "golden_recurrent_gru.json"), "w") as f:
        json.dump({"rec_e": meta}, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
