"""Cost of the fused backward of the 512 -> 256 layer of a wide stack (rslrl_hidden_bwd_pair_wk).

Not a test.  Two measurements, each alternating its variants in one process so that all see the same clocks:

  update   one PPO.update() -- 12 actions, T 24, 4 mini-batches, 5 epochs -- of the hidden stack [512, 256, 128] at N
           envs and each observation width (48; 235: a ragged first layer in front of the wide one): `fused` against
           `off` (RSLRL_HIDDEN_BWD_WK=0, here the module flag held off around update(): the weight-gradient and
           input-gradient launches).  One warm-up round, then the median of `--updates` updates with device events
           around update(), every sample kept.  The launch is the default at a shape where its median is below the
           other variant's fastest run.
  launch   the launch alone, one problem at the mini-batch's M rows, against the two launches it replaces
           (linear_wgrad_wide(bias_side=1), which runs its own fold, + linear_dgrad_elu_ex(wide=True)), `--iters` calls
           per event pair, the median of `--rounds` rounds: without its fold (`fused`) and with it (`fused_with_fold`,
           the like-for-like figure).  And the HBM rate the launch's median stands for at its algorithmic 5,120 B per
           row (dz and h read once, dz_prev written; the second read of dz, the partial rows and the L2-resident
           weight image are not counted).

Usage:  python scripts/hidden_bwd_wk_probe.py [--envs 4096,65536] [--obs 48,235] [--updates 5] [--out FILE.json]
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

T, A, MB, EPOCHS = 24, 12, 4, 5
K, NW = fused_mlp.HIDDEN_BWD_WK_SHAPE
HIDDEN = [512, 256, 128]
BYTES_PER_ROW = (NW + 2 * K) * 4


def build(N, O, dev):
    torch.manual_seed(0)
    obs0 = {"policy": torch.zeros(N, O, device=dev)}
    pol = ActorCritic(obs0, {"policy": ["policy"], "critic": ["policy"]}, A, actor_hidden_dims=HIDDEN,
                      critic_hidden_dims=HIDDEN)
    alg = PPO(pol, num_learning_epochs=EPOCHS, num_mini_batches=MB, device=str(dev))
    alg.init_storage("rl", N, T, obs0, [A])
    return alg


def fill(alg, N, O, dev, seed):
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


def probe_update(N, O, dev, updates):
    variants = {"fused": build(N, O, dev), "off": build(N, O, dev)}
    times, used, losses = {k: [] for k in variants}, {}, {}
    knob, real = fused_mlp._HIDDEN_BWD_WK, fused_mlp.hidden_bwd_pair_wk
    calls = []
    fused_mlp.hidden_bwd_pair_wk = lambda *a, **k: calls.append(1) or real(*a, **k)
    try:
        for it in range(updates + 1):  # the first round warms every shape up
            for name, alg in variants.items():
                fill(alg, N, O, dev, seed=it)
                fused_mlp._HIDDEN_BWD_WK = name == "fused"
                calls.clear()
                ms, loss = timed(alg.update)
                used[name] = len(calls)
                if it > 0:
                    times[name].append(ms)
                    losses[name] = loss
    finally:
        fused_mlp._HIDDEN_BWD_WK, fused_mlp.hidden_bwd_pair_wk = knob, real
    res = {k: {"ms_per_update": statistics.median(v), "ms_min": min(v), "ms_all": v,
               "hidden_bwd_wk_launches_per_update": used[k], "loss": losses[k]} for k, v in times.items()}
    res["fused_is_default"] = res["fused"]["ms_per_update"] < res["off"]["ms_min"]
    res["fused_vs_off"] = res["fused"]["ms_per_update"] / res["off"]["ms_per_update"]
    return res


def probe_launch(M, dev, rounds, iters):
    g = torch.Generator(device=dev).manual_seed(0)
    r = lambda *s: torch.randn(*s, device=dev, generator=g)  # noqa: E731
    dz, h = r(M, NW) * 0.01, torch.nn.functional.elu(r(M, K))
    img = fused_mlp.bimage_wide(r(NW, K) / 16, True)

    def fused():
        fused_mlp.hidden_bwd_pair_wk([dz], [h], [img], defer=fused_mlp._FoldBatch())

    def fused_with_fold():
        fused_mlp.hidden_bwd_pair_wk([dz], [h], [img])

    def separate():
        fused_mlp.linear_wgrad_wide(dz, h, bias_side=1)
        fused_mlp.linear_dgrad_elu_ex(dz, h, img, _lib.ARITH_X6, want_db=False, wide=True)

    fns = {"fused": fused, "separate": separate, "fused_with_fold": fused_with_fold}
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
    out["fused_vs_separate"] = round(out["fused_with_fold"]["median_us"] / out["separate"]["median_us"], 4)
    out["fused_is_default"] = out["fused_with_fold"]["median_us"] < out["separate"]["min_us"]
    out["algorithmic_bytes"] = M * BYTES_PER_ROW
    out["fused_hbm_tb_per_s"] = round(M * BYTES_PER_ROW / out["fused"]["median_us"] * 1e-6, 3)
    out["slices"] = _lib.lib().rslrl_hidden_bwd_slices_wk(M, K, NW)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", default="4096,65536")
    ap.add_argument("--obs", default="48,235")
    ap.add_argument("--updates", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("hidden_bwd_wk_probe: needs a GPU")
    dev = torch.device("cuda:0")
    envs = [int(n) for n in args.envs.split(",")]
    widths = [int(o) for o in args.obs.split(",")]
    out = {"device": torch.cuda.get_device_name(dev), "abi": _lib.lib().rslrl_abi_version(),
           "config": {"T": T, "obs": widths, "actions": A, "mini_batches": MB, "epochs": EPOCHS,
                      "updates": args.updates, "rounds": args.rounds, "iters": args.iters, "hidden": HIDDEN},
           "launch": {}, "update": {}}
    for N in envs:
        M = T * N // MB
        out["launch"][f"M={M}"] = probe_launch(M, dev, args.rounds, args.iters)
        torch.cuda.empty_cache()
    for N in envs:
        for O in widths:
            out["update"][f"N={N},obs={O}"] = probe_update(N, O, dev, args.updates)
            torch.cuda.empty_cache()
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
