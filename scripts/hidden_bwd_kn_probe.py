"""Cost of the fused backward of the 256 -> 128 hidden layers (rslrl_hidden_bwd_pair_kn).

Not a test.  Two measurements, each alternating its variants in one process so that all see the same clocks:

  update   one PPO.update() -- obs 48, 12 actions, T 24, 4 mini-batches, 5 epochs -- at N envs for the hidden stacks
           [512, 256, 128] (one single-problem launch per network and mini-batch), [256, 256, 128] and [256, 128, 128]
           (one two-problem launch per mini-batch): `fused` against `off` (RSLRL_HIDDEN_BWD_KN=0, here the module flag
           held off around update(): the weight-gradient and input-gradient launches).  One warm-up round, then the
           median of `--updates` updates with device events around update(), every sample kept.  The launch is the
           default at a shape where its median is below the other variant's fastest run.
  launch   the launch alone at the mini-batch's M rows against the two launches it replaces, `--iters` calls per event
           pair, the median of `--rounds` rounds.  pair: two problems against linear_wgrad_pair(bias_side=1) +
           linear_dgrad_elu_pair, the folds left out of both.  single: one problem against linear_wgrad(bias_side=1)
           + linear_dgrad_elu_ex; that weight-gradient entry runs its own fold, so the fused side is timed without
           its fold (`fused`) and with it (`fused_with_fold`, the like-for-like figure).  And the HBM rate the launch's
           median stands for at its algorithmic 2,560 B per row and problem (dz and h read once, dz_prev written; the
           second read of dz, the partial rows and the L2-resident weight image are not counted).

Usage:  python scripts/hidden_bwd_kn_probe.py [--envs 4096,65536] [--updates 5] [--out FILE.json]
"""

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rsl_rl_amd import _lib  # noqa: E402
from rsl_rl_amd.algorithms import PPO  # noqa: E402
from rsl_rl_amd.modules import ActorCritic  # noqa: E402
from rsl_rl_amd.networks import fused_mlp  # noqa: E402

T, O, A, MB, EPOCHS = 24, 48, 12, 4, 5
K, NW = fused_mlp.HIDDEN_BWD_KN_SHAPE
STACKS = {"512-256-128": [512, 256, 128], "256-256-128": [256, 256, 128], "256-128-128": [256, 128, 128]}
BYTES_PER_ROW = (NW + 2 * K) * 4  # per problem


def build(N, hidden, dev):
    torch.manual_seed(0)
    obs0 = {"policy": torch.zeros(N, O, device=dev)}
    pol = ActorCritic(obs0, {"policy": ["policy"], "critic": ["policy"]}, A, actor_hidden_dims=hidden,
                      critic_hidden_dims=hidden)
    alg = PPO(pol, num_learning_epochs=EPOCHS, num_mini_batches=MB, device=str(dev))
    alg.init_storage("rl", N, T, obs0, [A])
    return alg


def fill(alg, N, dev, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    rn = lambda *s: torch.randn(*s, device=dev, generator=g)  # noqa: E731
    st = alg.storage
    st.observations["policy"].copy_(rn(T, N, O))
    st.rewards.copy_(rn(T, N, 1))
    st.dones.copy_((torch.rand(T, N, 1, device=dev, generator=g) < 0.02).to(torch.uint8))
    mu, sigma = 0.1 * rn(T, N, A), torch.ones(T, N, A, device=dev)
    actions = mu + sigma * rn(T, N, A)
    st.mu.copy_(mu)
    st.sigma.copy_(sigma)
    st.actions.copy_(actions)
    st.values.copy_(0.1 * rn(T, N, 1))
    st.actions_log_prob.copy_(torch.distributions.Normal(mu, sigma).log_prob(actions).sum(-1, keepdim=True))
    st.step = T
    with torch.inference_mode():
        alg.compute_returns({"policy": rn(N, O)})


def timed(fn):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    out = fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end), out


def probe_update(N, hidden, dev, updates):
    variants = {"fused": build(N, hidden, dev), "off": build(N, hidden, dev)}
    times, used, losses = {k: [] for k in variants}, {}, {}
    knob, real = fused_mlp._HIDDEN_BWD_KN, fused_mlp.hidden_bwd_pair_kn
    calls = []
    fused_mlp.hidden_bwd_pair_kn = lambda *a, **k: calls.append(1) or real(*a, **k)
    try:
        for it in range(updates + 1):  # the first round warms every shape up
            for name, alg in variants.items():
                fill(alg, N, dev, seed=it)
                fused_mlp._HIDDEN_BWD_KN = name == "fused"
                calls.clear()
                ms, loss = timed(alg.update)
                used[name] = len(calls)
                if it > 0:
                    times[name].append(ms)
                    losses[name] = loss
    finally:
        fused_mlp._HIDDEN_BWD_KN, fused_mlp.hidden_bwd_pair_kn = knob, real
    res = {k: {"ms_per_update": statistics.median(v), "ms_min": min(v), "ms_all": v,
               "hidden_bwd_kn_launches_per_update": used[k], "loss": losses[k]} for k, v in times.items()}
    res["fused_is_default"] = res["fused"]["ms_per_update"] < res["off"]["ms_min"]
    res["fused_vs_off"] = res["fused"]["ms_per_update"] / res["off"]["ms_per_update"]
    return res


def probe_launch(M, n, dev, rounds, iters):
    g = torch.Generator(device=dev).manual_seed(0)
    r = lambda *s: torch.randn(*s, device=dev, generator=g)  # noqa: E731
    dzs = [r(M, NW) * 0.01 for _ in range(n)]
    hs = [torch.nn.functional.elu(r(M, K)) for _ in range(n)]
    imgs = fused_mlp.bimages([(r(NW, K) / 16, True) for _ in range(n)])

    def fused():
        fused_mlp.hidden_bwd_pair_kn(dzs, hs, imgs, defer=fused_mlp._FoldBatch())

    def fused_with_fold():
        fused_mlp.hidden_bwd_pair_kn(dzs, hs, imgs)

    def separate():
        if n == 2:
            fused_mlp.linear_wgrad_pair(dzs, hs, bias_side=1, defer=fused_mlp._FoldBatch())
            fused_mlp.linear_dgrad_elu_pair(dzs, hs, imgs, _lib.ARITH_X6)
        else:
            fused_mlp.linear_wgrad(dzs[0], hs[0], bias_side=1)
            fused_mlp.linear_dgrad_elu_ex(dzs[0], hs[0], imgs[0], _lib.ARITH_X6, want_db=False)

    fns = {"fused": fused, "separate": separate}
    if n == 1:
        fns["fused_with_fold"] = fused_with_fold
    res = {k: [] for k in fns}
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
    out = {k: {"median_us": round(statistics.median(v), 2), "min_us": round(min(v), 2),
               "runs_us": [round(t, 2) for t in v]} for k, v in res.items()}
    like = "fused" if n == 2 else "fused_with_fold"  # the side that does what `separate` does
    out["fused_vs_separate"] = round(out[like]["median_us"] / out["separate"]["median_us"], 4)
    out["fused_is_default"] = out[like]["median_us"] < out["separate"]["min_us"]
    out["algorithmic_bytes"] = n * M * BYTES_PER_ROW
    out["fused_hbm_tb_per_s"] = round(n * M * BYTES_PER_ROW / out["fused"]["median_us"] * 1e-6, 3)
    out["slices_per_problem"] = _lib.lib().rslrl_hidden_bwd_slices_kn(M, K, NW)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", default="4096,65536")
    ap.add_argument("--updates", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("hidden_bwd_kn_probe: needs a GPU")
    dev = torch.device("cuda:0")
    envs = [int(n) for n in args.envs.split(",")]
    out = {"device": torch.cuda.get_device_name(dev), "abi": _lib.lib().rslrl_abi_version(),
           "config": {"T": T, "obs": O, "actions": A, "mini_batches": MB, "epochs": EPOCHS, "updates": args.updates,
                      "rounds": args.rounds, "iters": args.iters, "stacks": STACKS},
           "launch": {}, "update": {}}
    for N in envs:
        M = T * N // MB
        for n, kind in ((2, "pair"), (1, "single")):
            out["launch"][f"M={M},{kind}"] = probe_launch(M, n, dev, args.rounds, args.iters)
        torch.cuda.empty_cache()
    for N in envs:
        for name, hidden in STACKS.items():
            out["update"][f"N={N},hidden={name}"] = probe_update(N, hidden, dev, args.updates)
            torch.cuda.empty_cache()
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
