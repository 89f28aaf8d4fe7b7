"""The rollout step's policy half (ActorCritic.act_and_evaluate under the act graph of modules/act_graph.py, inside
frozen_weights()) with the shaped one-launch forward (rollout_mlp_shaped.hip) against the path it replaces
(RSLRL_ROLLOUT_MLP_SHAPED=0), the knob alternating in one process: HIP-event time per step, medians of five, for the four
stacks at obs 48 and 235; and the forward pair alone, eager, the same way (the launch against the launches it replaces).

    python scripts/rollout_mlp_shaped_probe.py --out profiles/rollout_mlp_shaped_probe.json
"""

from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rsl_rl_amd import _lib  # noqa: E402
from rsl_rl_amd.modules import ActorCritic  # noqa: E402
from rsl_rl_amd.modules.act_graph import RolloutActGraph  # noqa: E402
from rsl_rl_amd.networks import fused_mlp  # noqa: E402


def timed(fn, steps):
    for _ in range(4):  # eager, capture, replays
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--num-envs", type=int, nargs="+", default=[4096, 8192, 16384])
    ap.add_argument("--big", type=int, default=65536, help="extra env count of the 4-aligned narrow stacks (no bound)")
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default="profiles/rollout_mlp_shaped_probe.json")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    out = {"note": __doc__.strip().splitlines()[0], "unit": "us per step", "runs": []}
    for hidden in _lib.ROLLOUT_MLP_SHAPED_WIDTHS:
        for k0 in (48, 235):
            envs = list(a.num_envs) + ([a.big] if k0 % 4 == 0 and max(hidden) <= fused_mlp.MAX_WIDTH else [])
            for n in envs:
                torch.manual_seed(0)
                obs = {"policy": torch.randn(n, k0, device=dev)}
                pol = ActorCritic(obs, {"policy": ["policy"], "critic": ["policy"]}, 12, actor_hidden_dims=list(hidden),
                                  critic_hidden_dims=list(hidden)).to(dev)
                x = obs["policy"]
                step = {"0": [], "1": []}
                pair = {"0": [], "1": []}
                launches = 0
                for r in range(a.rounds):
                    for mode in (("0", "1") if r % 2 == 0 else ("1", "0")):
                        fused_mlp._ROLLOUT_MLP_SHAPED = mode == "1"
                        g = RolloutActGraph(pol)
                        n0 = fused_mlp.rollout_mlp_shaped_launches
                        with torch.inference_mode(), fused_mlp.frozen_weights():
                            step[mode].append(timed(lambda: g(obs) is None and pol.act_and_evaluate(obs), a.steps))

                            def forward():
                                if fused_mlp.fused_mlp_forward_pair(pol.actor, x, pol.critic, x) is None:
                                    pol.actor(x), pol.critic(x)
                            pair[mode].append(timed(forward, a.steps))
                        launches += fused_mlp.rollout_mlp_shaped_launches - n0
                run = {"hidden": list(hidden), "obs": k0, "num_envs": n, "shaped_launches": launches}
                for name, res in (("step", step), ("forward_pair_eager", pair)):
                    run[name] = {("before" if m == "0" else "shaped"): {"us": [round(v, 2) for v in vs],
                                                                       "median": round(statistics.median(vs), 2),
                                                                       "min": round(min(vs), 2)}
                                 for m, vs in res.items()}
                # the project's rule: the default where the median is below the other variant's fastest run
                run["shaped_wins_step"] = run["step"]["shaped"]["median"] < run["step"]["before"]["min"]
                out["runs"].append(run)
                print(json.dumps(run), flush=True)
    fused_mlp._ROLLOUT_MLP_SHAPED = True
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
