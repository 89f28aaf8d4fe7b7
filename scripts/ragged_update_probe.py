"""Cost of PPO at the rough-terrain observation width -- obs 235 (48 proprioceptive values + 187 height samples), 12
actions, T 24, 4 mini-batches, 5 epochs -- with actor and critic [512, 256, 128] and 3 x 256, at N = 4096 and N = 65536
envs.  The protocol is scripts/wide_update_probe.py's, whose functions this script drives: per N, in one
process, alternating
  ragged  the ragged first layer (networks/fused_mlp.py ragged_structure): PPO._manual_minibatch
  off     RSLRL_RAGGED_INPUT=0 (here: the knob's module flag held off while the policy is built): layer by layer through
          networks/linear.py, PPO._autograd_minibatch -- the parent's update, the yardstick
update() medians of `--updates` and the rollout step (PPO.act + process_env_step).  --obs 236 times the 4-aligned
neighbour (both variants then take the same fused path: the ratio ragged / aligned is the cost of the ragged loads).  On
a tree without the ragged path (the parent commit) both variants take the parent's path.

--kernels: event-bracketed medians of 40 launches of the two ragged first-layer kernels at the mini-batch rows, alternating
with today's entry points on the 4-aligned neighbour width K + 1 (236).

--rollout-envs: further sizes at which only the rollout step is timed (where the ragged forward of a stack without wide
layers starts paying against the layer-by-layer step: RAGGED_FWD_MIN_ROWS).  --all-rows holds that threshold at 0 for
the run, so that every such forward takes the ragged kernel, which is how the threshold itself is measured.

Usage:  python scripts/ragged_update_probe.py [--obs 235] [--envs 4096,65536] [--updates 5] [--kernels]
                                              [--rollout-envs 8192,16384] [--all-rows] [--out FILE.json]
"""

import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wide_update_probe as W  # noqa: E402
from rsl_rl_amd import _lib  # noqa: E402
from rsl_rl_amd.algorithms import PPO  # noqa: E402
from rsl_rl_amd.modules import ActorCritic  # noqa: E402
from rsl_rl_amd.networks import fused_mlp  # noqa: E402

HAS_RAGGED = hasattr(fused_mlp, "ragged_structure")
KNOB_ON = bool(getattr(fused_mlp, "_RAGGED", False))
STACKS = {"512x256x128": [512, 256, 128], "256x256x256": [256, 256, 256]}


def build(N, dev, ragged):
    """wide_update_probe.build with the ragged knob's module flag in place of the wide one's."""
    torch.manual_seed(0)
    obs0 = {"policy": torch.zeros(N, W.O, device=dev)}
    prev = getattr(fused_mlp, "_RAGGED", None)
    if HAS_RAGGED:
        fused_mlp._RAGGED = bool(ragged) and KNOB_ON  # what RSLRL_RAGGED_INPUT sets at import; MLP reads it when built
    try:
        pol = ActorCritic(obs0, {"policy": ["policy"], "critic": ["policy"]}, W.A, actor_hidden_dims=W.HIDDEN,
                          critic_hidden_dims=W.HIDDEN)
    finally:
        if HAS_RAGGED:
            fused_mlp._RAGGED = prev
    alg = PPO(pol, num_learning_epochs=W.EPOCHS, num_mini_batches=W.M, device=str(dev))
    alg.init_storage("rl", N, W.T, obs0, [W.A])
    return alg


def probe_kernels(B, K, dev, calls=40):
    g = torch.Generator(device=dev).manual_seed(3)
    rn = lambda *s: torch.randn(*s, device=dev, generator=g)  # noqa: E731
    F, X6, Ka = fused_mlp, _lib.ARITH_X6, K + (-K) % 4 or K + 4
    res = {}
    for N in (512, 256):
        wide = N > 256
        img_of = F.bimage_wide if wide else F.bimage
        x, xa, dz, b = rn(B, K), rn(B, Ka), rn(B, N), rn(N)
        w, wa = rn(N, K) / K ** 0.5, rn(N, Ka) / Ka ** 0.5
        img, imga = img_of(w, False), img_of(wa, False)
        wg = F.linear_wgrad_wide if wide else F.linear_wgrad
        cases = {f"fwd_elu[K={K},N={N}]": (lambda: F.linear_fwd_ragged(x, b, N, True, img),
                                             lambda: F.linear_fwd_ex(xa, b, N, True, imga, X6, wide=wide)),
                 f"wgrad_bias[N={N},K={K}]": (lambda: F.linear_wgrad_ragged(dz, x, with_bias=True),
                                               lambda: wg(dz, xa, bias_side=1))}
        for name, (rag, ali) in cases.items():
            rag()
            ali()
            tr, ta = [], []
            for _ in range(calls):
                tr.append(W.timed(rag)[0])
                ta.append(W.timed(ali)[0])
            res[name] = {"rows": B, "aligned_K": Ka, "ragged_us": 1e3 * float(np.median(tr)), "ragged_us_min": 1e3 * min(tr),
                         "aligned_us": 1e3 * float(np.median(ta)), "aligned_us_min": 1e3 * min(ta),
                         "ratio": float(np.median(tr) / np.median(ta))}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--obs", type=int, default=235)
    ap.add_argument("--envs", default="4096,65536")
    ap.add_argument("--updates", type=int, default=5)
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--rollout-envs", default="", help="sizes at which only the rollout step is timed")
    ap.add_argument("--all-rows", action="store_true", help="RAGGED_FWD_MIN_ROWS = 0 for this run")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ragged_update_probe: needs a ROCm GPU; a CPU run measures nothing")
    dev = torch.device("cuda:0")
    if args.all_rows and HAS_RAGGED:
        fused_mlp.RAGGED_FWD_MIN_ROWS = 0
    W.O, W.HAS_WIDE = args.obs, False  # (HAS_WIDE off: wide_update_probe's own launch-count assertion does not apply)
    W.build = build
    W.launches = lambda: getattr(fused_mlp, "ragged_launches", 0)
    res = {"shape": {"T": W.T, "obs": W.O, "actions": W.A, "stacks": STACKS, "mini_batches": W.M, "epochs": W.EPOCHS,
                     "device": torch.cuda.get_device_name(0), "tree_has_ragged_path": HAS_RAGGED,
                     "ragged_knob_on": KNOB_ON, "all_rows": bool(args.all_rows)}}
    for N in [int(x) for x in args.rollout_envs.split(",") if x]:
        for name, hidden in STACKS.items():
            W.HIDDEN = hidden
            r = W.probe_rollout(N, dev)
            res[f"rollout_envs_{N}_{name}"] = {"ragged": r["wide"], "off": r["off"]}
            print(N, name, json.dumps(res[f"rollout_envs_{N}_{name}"]), flush=True)
            torch.cuda.empty_cache()
    for N in [int(x) for x in args.envs.split(",") if x]:
        for name, hidden in STACKS.items():
            W.HIDDEN = hidden
            r = {"update": W.probe_updates(N, dev, args.updates)}
            torch.cuda.empty_cache()
            r["rollout_step"] = W.probe_rollout(N, dev)
            for part in ("update", "rollout_step"):  # wide_update_probe's variant names: "wide" is the feature here
                r[part] = {"ragged": r[part]["wide"], "off": r[part]["off"]}
            res[f"envs_{N}_{name}"] = r
            print(N, name, json.dumps(r), flush=True)
            torch.cuda.empty_cache()
        if args.kernels and HAS_RAGGED and args.obs % 4:
            res[f"envs_{N}_kernels"] = probe_kernels(N * W.T // W.M, args.obs, dev)
            print(N, json.dumps(res[f"envs_{N}_kernels"]), flush=True)
            torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
