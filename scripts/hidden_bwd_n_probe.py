"""Cost of the fused backward of the 128 x 128 hidden layers (rslrl_hidden_bwd_pair_n).

Not a test.  Two measurements, each alternating its two variants in one process so that both see the same clocks:

  update   one PPO.update() -- obs 48, 12 actions, T 24, 4 mini-batches, 5 epochs -- at N envs for the hidden stacks
           [128, 128, 128] and [256, 128, 128]: `fused` (hidden_bwd_pair_n once per mini-batch and square 128 layer)
           against `off` (RSLRL_HIDDEN_BWD_N=0, here the module flag held off around update(): linear_wgrad_pair and
           linear_dgrad_elu_pair).  One warm-up round, then the median of `--updates` updates with device events around
           update(), every sample kept.  The launch is the default at a shape where its median is below the other
           variant's fastest run.
  launch   the launch alone for a pair of problems at the mini-batch's M rows against the two launches it replaces (the
           folds are left out of both), `--iters` calls per event pair, the median of `--rounds` rounds; and the HBM
           rate the launch's median stands for at its algorithmic 1,536 B per row and problem (dz and h read, dz_prev
           written; the partial rows and the L2-resident weight image are not counted).

Usage:  python scripts/hidden_bwd_n_probe.py [--envs 4096,65536] [--updates 5] [--out FILE.json]
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
W = fused_mlp.HIDDEN_BWD_N_WIDTH
STACKS = {"128-128-128": [128, 128, 128], "256-128-128": [256, 128, 128]}
BYTES_PER_ROW = 3 * W * 4  # per problem


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
    knob, real = fused_mlp._HIDDEN_BWD_N, fused_mlp.hidden_bwd_pair_n
    calls = []
    fused_mlp.hidden_bwd_pair_n = lambda *a, **k: calls.append(1) or real(*a, **k)
    try:
        for it in range(updates + 1):  # the first round warms every shape up
            for name, alg in variants.items():
                fill(alg, N, dev, seed=it)
                fused_mlp._HIDDEN_BWD_N = name == "fused"
                calls.clear()
                ms, loss = timed(alg.update)
                used[name] = len(calls)
                if it > 0:
                    times[name].append(ms)
                    losses[name] = loss
    finally:
        fused_mlp._HIDDEN_BWD_N, fused_mlp.hidden_bwd_pair_n = knob, real
    res = {k: {"ms_per_update": statistics.median(v), "ms_min": min(v), "ms_all": v,
               "hidden_bwd_n_launches_per_update": used[k], "loss": losses[k]} for k, v in times.items()}
    res["fused_is_default"] = res["fused"]["ms_per_update"] < res["off"]["ms_min"]
    res["fused_vs_off"] = res["fused"]["ms_per_update"] / res["off"]["ms_per_update"]
    return res


def probe_launch(M, dev, rounds, iters):
    g = torch.Generator(device=dev).manual_seed(0)
    r = lambda *s: torch.randn(*s, device=dev, generator=g)  # noqa: E731
    dzs = [r(M, W) * 0.01 for _ in range(2)]
    hs = [torch.nn.functional.elu(r(M, W)) for _ in range(2)]
    imgs = fused_mlp.bimages([(r(W, W) / 16, True) for _ in range(2)])

    def fused():
        fused_mlp.hidden_bwd_pair_n(dzs, hs, imgs, defer=fused_mlp._FoldBatch())

    def separate():
        fused_mlp.linear_wgrad_pair(dzs, hs, bias_side=1, defer=fused_mlp._FoldBatch())
        fused_mlp.linear_dgrad_elu_pair(dzs, hs, imgs, _lib.ARITH_X6)

    fns = {"fused": fused, "separate": separate}
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
    out["fused_vs_separate"] = round(out["fused"]["median_us"] / out["separate"]["median_us"], 4)
    out["fused_is_default"] = out["fused"]["median_us"] < out["separate"]["min_us"]
    out["algorithmic_bytes"] = 2 * M * BYTES_PER_ROW
    out["fused_hbm_tb_per_s"] = round(2 * M * BYTES_PER_ROW / out["fused"]["median_us"] * 1e-6, 3)
    out["slices_per_problem"] = _lib.lib().rslrl_hidden_bwd_slices_n(M, W)
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
        sys.exit("hidden_bwd_n_probe: needs a GPU")
    dev = torch.device("cuda:0")
    envs = [int(n) for n in args.envs.split(",")]
    out = {"device": torch.cuda.get_device_name(dev), "abi": _lib.lib().rslrl_abi_version(),
           "config": {"T": T, "obs": O, "actions": A, "mini_batches": MB, "epochs": EPOCHS, "updates": args.updates,
                      "rounds": args.rounds, "iters": args.iters, "stacks": STACKS},
           "launch": {}, "update": {}}
    for N in envs:
        M = T * N // MB
        out["launch"][f"M={M}"] = probe_launch(M, dev, args.rounds, args.iters)
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
