"""Generate the recurrent distillation fixture at a student observation width that is no multiple of 16 (drec_d;
DESIGN.md §22) under tests/golden/ by running the REFERENCE's Distillation.update() on CPU.

Test infrastructure only: the machinery of make_golden_distillation_recurrent.py (run_case / make_case / pack, the
hand-placed dones and their assertions, the clip assertions, the one-ulp sensitivity envelope) is imported and called
unchanged.  It adds one case and writes tests/golden/drec_d*.npz plus
tests/golden/golden_distillation_recurrent_anyd.json.

  d  case c with O_student = 45: LSTM H 256, one layer; N 128, O 45 / 64, A 4, MLPs [64, 64]; T 8, E 2, G 3, MSE,
     clip 1.0; seeded non-zero last_hidden_states; the student's first layer x 4; the sensitivity envelope

Usage:  python tests/golden/make_golden_distillation_recurrent_anyd.py --reference PATH_TO_RSL_RL_CHECKOUT
"""

from __future__ import annotations

import argparse
import json
import os

import torch

import make_golden_distillation_recurrent as MGD

HERE = os.path.dirname(os.path.abspath(__file__))
CASE = dict(MGD.CASES["c"], O_student=45, seed=419)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="the rsl_rl 3.1.0 checkout (the directory holding rsl_rl/)")
    args = ap.parse_args()
    torch.set_num_threads(1)
    MGD.CASES["d"] = CASE
    meta = {"d": MGD.make_case(args.reference, "d")}
    with open(os.path.join(HERE, "golden_distillation_recurrent_anyd.json"), "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
