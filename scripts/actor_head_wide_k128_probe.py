"""Cost of the fused actor head for 17 to 32 actions on a last hidden layer with 128 inputs
(csrc/mlp_heads_wide_k128.hip).

Not a test.  scripts/head_k128_probe.py's two measurements at the new action counts, each alternating its two variants
in one process so that both see the same clocks:

  update   one PPO.update() -- obs 48, T 24, 4 mini-batches, 5 epochs -- at N envs for the hidden stacks [128, 128, 128]
           and [256, 128, 64] at 19, 24 and 32 actions: `head` against `off` (RSLRL_ACTOR_HEAD_WIDE_K128=0, here the
           module flag held off around update(): linear_fwd_out with H stored, the loss kernel, the padded d mu copy, the
           dgrad + ELU' GEMM, the weight gradient and the bias sum -- and no paired passes).  One warm-up round, then the
           median of `--updates` updates, every sample kept.  The head is the default at a shape where its median is
           below the other variant's fastest run.
  launch   the head's launch alone at the mini-batch's M rows (K = 128, N = 128 and 64) against the launches it
           replaces, `--iters` calls per event pair, the median of `--rounds` rounds.

Usage:  python scripts/actor_head_wide_k128_probe.py [--envs 4096,65536] [--out profiles/actor_head_wide_k128_probe.json]
"""

import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import head_narrow_probe as hnp  # noqa: E402  (also puts the repository on sys.path)
from head_narrow_probe import EPOCHS, MB, T, build, fill, timed  # noqa: E402
from rsl_rl_amd import _lib, kernels  # noqa: E402
from rsl_rl_amd.networks import fused_mlp  # noqa: E402

O, K = 48, 128
STACKS = {"128-128-128": [128, 128, 128], "256-128-64": [256, 128, 64]}
ACTIONS = (19, 24, 32)


def probe_update(N, hidden, A, dev, updates):
    hnp.A = A  # build and fill size the policy and the stored fields by the module's action count
    variants = {"head": build(N, O, hidden, dev), "off": build(N, O, hidden, dev)}
    times, used = {k: [] for k in variants}, {}
    knob = fused_mlp._ACTOR_HEAD_WIDE_K128
    try:
        for it in range(updates + 1):  # the first round warms every shape up
            for name, alg in variants.items():
                fill(alg, N, O, dev, seed=it)
                fused_mlp._ACTOR_HEAD_WIDE_K128 = name == "head"
                before = fused_mlp.actor_head_wide_launches
                ms, _ = timed(alg.update)
                used[name] = fused_mlp.actor_head_wide_launches - before
                if it > 0:
                    times[name].append(ms)
    finally:
        fused_mlp._ACTOR_HEAD_WIDE_K128 = knob
    res = {k: {"ms_per_update": statistics.median(v), "ms_min": min(v), "ms_all": v,
               "actor_head_wide_launches_per_update": used[k]} for k, v in times.items()}
    res["head_is_default"] = res["head"]["ms_per_update"] < res["off"]["ms_min"]
    res["head_vs_off"] = res["head"]["ms_per_update"] / res["off"]["ms_per_update"]
    return res


def probe_launch(M, N, A, dev, rounds, iters):
    g = torch.Generator(device=dev).manual_seed(0)
    r = lambda *s: torch.randn(*s, device=dev, generator=g)  # noqa: E731
    x = F.elu(r(M, K))
    w, b, wo, bo = r(N, K) / 11, r(N) * 0.1, r(A, N) / 16, r(A) * 0.1
    sigma = torch.rand(A, device=dev, generator=g) * 0.5 + 0.5
    old_sigma = sigma.expand(M, A).contiguous()
    acts, ologp, adv, tv, ret, omu, vals = r(M, A), r(M, 1) - 1.5 * A, r(M, 1), r(M, 1), r(M, 1), r(M, A) * 0.1, r(M, 1)
    img, out_img, img_t = fused_mlp.bimages([(w, False), (wo, False, _lib.BIMAGE_LAYOUT_OUT), (wo, True)])
    head = fused_mlp.ActorHeadWide(acts, ologp, adv, tv, ret, omu, old_sigma, sigma, clip_param=0.2, value_loss_coef=1.0,
                                   entropy_coef=0.01, use_clipped=True, compute_kl=True,
                                   grad_sigma=torch.empty(A, device=dev), stats=torch.empty(8, device=dev))
    head.values = vals

    def fused():
        assert fused_mlp.actor_head_wide_fwd_bwd(x, b, N, img, bo, out_img, img_t, head) is not None

    def separate():
        h, mu = fused_mlp.linear_fwd_out_ex(x, b, N, img, _lib.ARITH_X6, None, bo, out_img, store_h=True)
        _, gmu, _, _ = kernels.ppo_loss_fwd_bwd(mu, sigma, vals, acts, ologp, adv, tv, ret, omu, old_sigma,
                                                compute_kl=True)
        fused_mlp.linear_dgrad_elu_ex(F.pad(gmu, (0, (-A) % 4)), h, img_t, _lib.ARITH_X6, None, False, want_db=False)
        fused_mlp._weight_grad(gmu, h, True)
        gmu.sum(0)

    fns = {"fused": fused, "separate": separate}
    res = {k: [] for k in fns}
    knob = fused_mlp._ACTOR_HEAD_WIDE_K128
    fused_mlp._ACTOR_HEAD_WIDE_K128 = True
    try:
        for fn in fns.values():
            fn()
        torch.cuda.synchronize()
        for _ in range(rounds):
            for name, fn in fns.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(iters):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                res[name].append(e0.elapsed_time(e1) * 1000.0 / iters)
    finally:
        fused_mlp._ACTOR_HEAD_WIDE_K128 = knob
    return {k: {"median_us": round(statistics.median(v), 2), "runs_us": [round(t, 2) for t in v]}
            for k, v in res.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", default="4096,65536")
    ap.add_argument("--updates", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("actor_head_wide_k128_probe: needs a GPU")
    dev = torch.device("cuda:0")
    envs = [int(n) for n in args.envs.split(",")]
    out = {"device": torch.cuda.get_device_name(dev), "abi": _lib.lib().rslrl_abi_version(),
           "config": {"obs": O, "T": T, "actions": ACTIONS, "mini_batches": MB, "epochs": EPOCHS,
                      "updates": args.updates, "rounds": args.rounds, "iters": args.iters, "stacks": STACKS},
           "update": {}, "launch": {}}
    for N in envs:
        for name, hidden in STACKS.items():
            for A in ACTIONS:
                out["update"][f"N={N},hidden={name},A={A}"] = probe_update(N, hidden, A, dev, args.updates)
                torch.cuda.empty_cache()
    for N in envs:
        for width in _lib.HEAD_K128_WIDTHS[::-1]:
            for A in ACTIONS:
                out["launch"][f"M={T * N // MB},N={width},A={A}"] = probe_launch(T * N // MB, width, A, dev, args.rounds,
                                                                                args.iters)
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
