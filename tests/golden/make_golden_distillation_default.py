"""Generate the distillation fixtures of the students that take the window-batched update since DESIGN.md §23 -- wide,
ragged and GRU students -- under tests/golden/ by running the REFERENCE's Distillation.update() on CPU.

Test infrastructure only: the machinery of make_golden_distillation.py (feed-forward students) and of
make_golden_distillation_recurrent.py (recurrent ones: run_case / make_case, the hand-placed dones and their assertions,
the clip assertions, the one-ulp sensitivity envelope) is imported and called unchanged.  Only where the arrays go
differs: recurrent_fixtures.save_split writes them (row blocks `<key>@<i>`, which drec_fixtures.Arrays and
recurrent_fixtures.Arrays join), with its part size lowered so that no file exceeds the largest distillation fixture
committed before (drec_c.npz, 818,540 bytes).  Writes tests/golden/distill_{d,e}_*.npz, drec_{e,f}_*.npz and
tests/golden/golden_distillation_default.json.

  distill_d  StudentTeacher; student obs 45, teacher obs 64, A 12, hidden [320, 260, 64] (a ragged first layer and
             wide layers); N 64, T 8, E 2, G 3: five full windows, one of them across the epoch boundary, and a trailing
             one; MSE, clip 1.0; the sensitivity envelope
  distill_e  StudentTeacher; student obs 19, hidden [64, 64] (ragged, no wide layer); N 128, T 8, E 2, G 3; Huber, log
             std, student normalisation with non-trivial buffers, no clip
  drec_e     StudentTeacherRecurrent, make_golden_distillation_recurrent's case c with rnn_type "gru": GRU 256, one
             layer; N 128, O 48 / 64, A 4, MLPs [64, 64]; T 8, E 2, G 3, MSE, clip 1.0; seeded non-zero
             last_hidden_states; the student's first layer x 4; the sensitivity envelope
  drec_f     as drec_e with student obs 45, MLPs [320, 260, 64] and teacher_recurrent (a GRU teacher)

Dones of the recurrent cases: place_dones puts them by hand, whatever the seed; this script asserts on the stored array
that it holds an env that is never done, a done at t = 0, a done at t = T - 1 and an env done on two consecutive steps.
Seeds: 521 (distill_d), 523 (distill_e), 431 (drec_e), 433 (drec_f).  distill_d at make_golden_distillation's teacher
scale (actions x 3) was rejected by that generator's clip assertion for every seed tried, 521 to 559: the first
gradient's norm came out between 0.46 and 0.88, below max_grad_norm = 1.0, so the clip would never act.  The case
therefore scales the teacher's actions by 10, as the recurrent generator does (`target_scale` below, recorded in the
meta), and seed 521 passes.  For the other three the first seed tried passed the generators' assertions (both Huber
branches populated; the memory's share of the gradient norm).

Usage:  python tests/golden/make_golden_distillation_default.py --reference PATH_TO_RSL_RL_CHECKOUT [--cases distill_d,...]
"""

from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch

import make_golden_distillation as MD
import make_golden_distillation_recurrent as MGD

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import recurrent_fixtures as RF  # noqa: E402

LARGEST_BEFORE = 818540  # drec_c.npz
RF.PART_BYTES = 760 * 1024  # (fp32 noise compresses by ~8 %)

FF_CASES = {
    "distill_d": dict(T=8, N=64, O_student=45, O_teacher=64, A=12, hidden=[320, 260, 64], E=2, G=3, world=1,
                      loss_type="mse", max_grad_norm=1.0, policy_kw={}, seed=521, sensitivity=True,
                      target_scale=10.0),
    "distill_e": dict(T=8, N=128, O_student=19, O_teacher=24, A=4, hidden=[64, 64], E=2, G=3, world=1,
                      loss_type="huber", max_grad_norm=None, seed=523,
                      policy_kw={"noise_std_type": "log", "student_obs_normalization": True}),
}
REC_CASES = {
    "drec_e": dict(MGD.CASES["c"], rnn_type="gru", seed=431),
    "drec_f": dict(MGD.CASES["c"], rnn_type="gru", O_student=45, hidden=[320, 260, 64], teacher_recurrent=True,
                   seed=433),
}


def _save(arrays, stem):
    files = RF.save_split(arrays, stem)
    for f in files:
        assert os.path.getsize(os.path.join(HERE, f)) <= LARGEST_BEFORE, (f, os.path.getsize(os.path.join(HERE, f)))
    return files


def make_ff(ref_path, name):
    """make_golden_distillation.make_case, then its files rewritten by save_split (and removed): the runs, the envelope
    and the meta are its own."""
    short = name[len("distill_"):]  # make_case writes distill_<short>*.npz
    MD.CASES[short] = FF_CASES[name]
    scale = MD.TARGET_SCALE
    MD.TARGET_SCALE = FF_CASES[name].get("target_scale", scale)  # (run_case and the meta read the module's)
    try:
        meta = MD.make_case(ref_path, short)
    finally:
        MD.TARGET_SCALE = scale
    arrays = {}
    for f in meta["files"]:
        with np.load(os.path.join(HERE, f)) as z:
            arrays.update({k: z[k] for k in z.files})
        os.remove(os.path.join(HERE, f))
    meta["files"] = _save(arrays, name)
    return meta


def check_dones(d):
    T, N = d.shape
    assert any(not d[:, n].any() for n in range(N)), "no env that is never done"
    assert d[0].any() and d[T - 1].any(), "no done at t = 0 or at t = T - 1"
    assert any(d[t, n] and d[t + 1, n] for t in range(T - 1) for n in range(N)), "no two consecutive dones"


def make_rec(ref_path, name):
    def pack(case, arrays):
        check_dones(arrays["r0/dones"])
        return _save(arrays, case)

    real = MGD.pack
    MGD.pack = pack
    try:
        MGD.CASES[name] = REC_CASES[name]
        meta = MGD.make_case(ref_path, name)
    finally:
        MGD.pack = real
    print(name, "ulp sensitivity (max over tensors)", max(meta["ulp_sensitivity"].values()), flush=True)
    return meta


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="the rsl_rl 3.1.0 checkout (the directory holding rsl_rl/)")
    ap.add_argument("--cases", default=None, help="comma-separated case names (default: all)")
    args = ap.parse_args()
    torch.set_num_threads(1)
    path = os.path.join(HERE, "golden_distillation_default.json")
    meta = {}
    if args.cases and os.path.exists(path):
        with open(path) as f:
            meta = json.load(f)
    for name in list(FF_CASES) + list(REC_CASES):
        if args.cases is None or name in args.cases.split(","):
            meta[name] = (make_ff if name in FF_CASES else make_rec)(args.reference, name)
    with open(path, "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
