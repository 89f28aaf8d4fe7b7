"""Golden fixture of one PPO update with a wide actor / critic (hidden widths above 256: DESIGN.md §20), by running the
REFERENCE (rsl_rl 3.1.0) on the CPU.

make_golden.py (_update_case through _make_update_family, with its one-ulp sensitivity probes) is imported and called
unchanged.  This script adds one case -- T 8, N 256, O 16, A 4, hidden [320, 260, 64] (a 4-aligned width that is no
multiple of the 256-column tile, a second layer wide on both sides, a last hidden layer with more than 256 inputs), E 5,
M 4, adaptive schedule -- and writes tests/golden/update_wide_{init,final,rest}.npz plus tests/golden/golden_wide.json.
The arrays are one fixture, split by key group (tests/wide_fixtures.py puts them back together): the repository takes no
new file above 1 MiB, the rule make_golden_recurrent.py and the fixtures after it follow; the larger update_*.npz beside
them were committed before it.

The case's seed is the first of SEEDS for which every mini-batch KL of the reference's run lies at least 10 % away from
both thresholds of the adaptive schedule (desired_kl / 2 and 2 desired_kl: a last-bit difference must not flip a
learning-rate decision).  The KLs are read where the reference computes them, through a recording wrapper around
torch.mean (rsl_rl/algorithms/ppo.py:269 is its only call during update()).  Seeds tried and turned away are listed
in golden_wide.json ("seeds_rejected").

Usage:  python tests/golden/make_golden_wide.py --reference <checkout of rsl_rl 3.1.0>   (or RSL_RL_REFERENCE)
"""

from __future__ import annotations

import argparse
import json
import os

import numpy as np
import torch

import make_golden as MG

HERE = os.path.dirname(os.path.abspath(__file__))
SEEDS = (113, 127, 131, 137, 139, 149, 151, 157)
DESIRED_KL = 0.01  # the reference's default (ppo.py:39)
PARTS = {"init": ("r0/init/",), "final": ("r0/final/",)}  # every other key goes to "rest"


def case_of(seed):
    return ("wide", 1, 8, 256, 16, 4, [320, 260, 64], seed, 1e-3, {"sensitivity": True, "grad_batches": 1})


class KlRecorder:
    """Records every scalar the reference forms with torch.mean(<1-D tensor>) -- the mini-batch KL."""

    def __enter__(self):
        self.values, self._mean = [], torch.mean

        def mean(x, *a, **k):
            out = self._mean(x, *a, **k)
            if not a and not k and x.dim() == 1:
                self.values.append(float(out))
            return out

        torch.mean = mean
        return self

    def __exit__(self, *exc):
        torch.mean = self._mean


def kl_margin_ok(kls):
    return all(abs(kl - thr) >= 0.10 * thr for kl in kls for thr in (DESIRED_KL / 2, 2 * DESIRED_KL))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("RSL_RL_REFERENCE"), required="RSL_RL_REFERENCE" not in os.environ)
    args = ap.parse_args()
    torch.set_num_threads(1)
    rejected, seed, kls = [], None, None
    for s in SEEDS:
        with KlRecorder() as rec:
            MG._run_update_case(args.reference, case_of(s))
        assert len(rec.values) == 5 * 4, len(rec.values)
        if kl_margin_ok(rec.values):
            seed, kls = s, rec.values
            break
        rejected.append({"seed": s, "kl_trace": rec.values})
    assert seed is not None, "no seed of SEEDS keeps every KL 10 % away from the lr thresholds"
    meta = MG._make_update_family(args.reference, [case_of(seed)])["wide"]
    big = os.path.join(HERE, "update_wide.npz")
    z = np.load(big)
    groups = {name: {} for name in list(PARTS) + ["rest"]}
    for k in z.files:
        part = next((name for name, pres in PARTS.items() if k.startswith(pres)), "rest")
        groups[part][k] = z[k]
    z.close()
    os.remove(big)
    files = []
    for name, arrays in groups.items():
        path = os.path.join(HERE, f"update_wide_{name}.npz")
        np.savez_compressed(path, **arrays)
        assert os.path.getsize(path) <= 1 << 20, (path, os.path.getsize(path))
        files.append(os.path.basename(path))
    assert kl_margin_ok(kls)
    meta.update({"kl_trace": kls, "desired_kl": DESIRED_KL, "seeds_rejected": rejected, "files": files})
    with open(os.path.join(HERE, "golden_wide.json"), "w") as f:
        json.dump({"wide": meta}, f, indent=1, sort_keys=True)
    print("wide fixture: seed", seed, "KLs", [round(k, 5) for k in kls], "rejected", [r["seed"] for r in rejected])


if __name__ == "__main__":
    main()
