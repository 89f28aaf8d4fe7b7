"""Cost of PPO with the locomotion tasks' default networks -- obs 48, 12 actions, actor and critic [512, 256, 128] ELU,
T 24, 4 mini-batches, 5 epochs -- at N = 4096 and N = 65536 envs.

Not a test.  For each N, on one box and in one process, alternating so that both variants see the same clocks:
  wide   the wide path (networks/fused_mlp.py wide_structure): PPO._manual_minibatch, the layers wider than 256 on
         csrc/mlp_wide.hip
  off    RSLRL_WIDE_MLP=0 (here: the knob's module flag held off while the policy is built): layer by layer through
         networks/linear.py, PPO._autograd_minibatch -- the parent's update, the yardstick
Each is warmed up once, then timed over `--updates` updates with device events around update(); the median is reported
with every sample and the peak device allocation of an update (DESIGN §14's protocol).  The rollout step (PPO.act +
process_env_step on a SyntheticVecEnv, under the runner's frozen_weights scope) is timed the same way per step.  On a
tree without the wide path (the parent commit) the script needs nothing new: both variants then take the parent's path,
which shows that `off` is the parent's figure.

--kernels: event-bracketed medians of 40 launches of the three wide kernels at the mini-batch shapes, alternating with
the tiled kernels run on the dense 256-column blocks of the same problem (the sum over the blocks is the yardstick).

--rollout-envs: further sizes at which only the rollout step is timed (where the per-layer launches of the wide forward
stop paying against the layer-by-layer step).  With RSLRL_WIDE_MLP=0 in the environment both variants run `off`.

Usage:  python scripts/wide_update_probe.py [--envs 4096,65536] [--updates 5] [--kernels] [--rollout-envs 8192,16384]
                                            [--out FILE.json]
"""

import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rsl_rl_amd import _lib  # noqa: E402
from rsl_rl_amd.algorithms import PPO  # noqa: E402
from rsl_rl_amd.env import SyntheticVecEnv  # noqa: E402
from rsl_rl_amd.modules import ActorCritic  # noqa: E402
from rsl_rl_amd.networks import fused_mlp  # noqa: E402

T, O, A, HIDDEN, M, EPOCHS = 24, 48, 12, [512, 256, 128], 4, 5
HAS_WIDE = hasattr(fused_mlp, "wide_structure")
KNOB_ON = bool(getattr(fused_mlp, "_WIDE_MLP", False))  # RSLRL_WIDE_MLP=0 in the environment: both variants run `off`


def build(N, dev, wide):
    torch.manual_seed(0)
    obs0 = {"policy": torch.zeros(N, O, device=dev)}
    prev = getattr(fused_mlp, "_WIDE_MLP", None)
    if HAS_WIDE:
        fused_mlp._WIDE_MLP = bool(wide) and KNOB_ON  # what RSLRL_WIDE_MLP sets at import; MLP reads it when built
    try:
        pol = ActorCritic(obs0, {"policy": ["policy"], "critic": ["policy"]}, A, actor_hidden_dims=HIDDEN,
                          critic_hidden_dims=HIDDEN)
    finally:
        if HAS_WIDE:
            fused_mlp._WIDE_MLP = prev
    alg = PPO(pol, num_learning_epochs=EPOCHS, num_mini_batches=M, device=str(dev))
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


def launches():
    return getattr(fused_mlp, "wide_launches", 0)


def probe_updates(N, dev, updates):
    variants = {"wide": build(N, dev, True), "off": build(N, dev, False)}
    times, peaks, losses, used = {k: [] for k in variants}, {}, {}, {}
    for it in range(updates + 1):  # the first round warms every shape up
        for name, alg in variants.items():
            fill(alg, N, dev, seed=it)
            torch.cuda.reset_peak_memory_stats(dev)
            before = launches()
            ms, loss = timed(alg.update)
            used[name] = launches() - before
            if it > 0:
                times[name].append(ms)
                losses[name] = loss
                peaks[name] = torch.cuda.max_memory_allocated(dev)
    if HAS_WIDE and KNOB_ON:
        assert used["wide"] > 0 and used["off"] == 0, used
    return {k: {"ms_per_update": float(np.median(v)), "ms_min": min(v), "ms_all": v, "peak_allocated_bytes": peaks[k],
                "wide_launches_per_update": used[k], "loss": losses[k]} for k, v in times.items()}


def probe_rollout(N, dev, rollouts=3):
    """ms per env step of PPO.act + process_env_step (the env's own step is outside the events)."""
    res = {}
    envs = {k: SyntheticVecEnv(N, O, A, device=dev, seed=0) for k in ("wide", "off")}
    algs = {"wide": build(N, dev, True), "off": build(N, dev, False)}
    times = {k: [] for k in algs}
    obs = {k: envs[k].get_observations() for k in algs}
    for r in range(rollouts + 1):
        for name, alg in algs.items():
            env = envs[name]
            with torch.inference_mode(), fused_mlp.frozen_weights():
                for _ in range(T):
                    o = obs[name]
                    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    torch.cuda.synchronize()
                    start.record()
                    actions = alg.act(o)
                    mid = torch.cuda.Event(enable_timing=True)
                    mid.record()
                    o, rewards, dones, extras = env.step(actions)
                    env_done = torch.cuda.Event(enable_timing=True)
                    env_done.record()
                    alg.process_env_step(o, rewards, dones, extras)
                    end.record()
                    torch.cuda.synchronize()
                    obs[name] = o
                    if r > 0:
                        times[name].append(start.elapsed_time(mid) + env_done.elapsed_time(end))
                alg.compute_returns(obs[name])
            alg.storage.clear()
    for k, v in times.items():
        res[k] = {"ms_per_step": float(np.median(v)), "ms_min": min(v), "steps": len(v)}
    return res


def probe_kernels(B, dev, calls=40):
    """The wide kernels at the layers of [48 -> 512 -> 256] over B rows, beside the tiled kernels on the dense blocks."""
    g = torch.Generator(device=dev).manual_seed(3)
    rn = lambda *s: torch.randn(*s, device=dev, generator=g)  # noqa: E731
    X6 = _lib.ARITH_X6
    F = fused_mlp
    cases = {}

    def blocks(n):
        return [(c0, min(256, n - c0)) for c0 in range(0, n, 256)]

    for K, N in ((48, 512), (512, 256)):  # forward of the two wide layers
        x, w, b = rn(B, K), rn(N, K) / K ** 0.5, rn(N)
        img = F.bimage_wide(w, False)
        dense = [(F.bimage(w[c0:c0 + n].contiguous(), False), b[c0:c0 + n].contiguous(), n) for c0, n in blocks(N)]
        cases[f"fwd_elu[K={K},N={N}]"] = (
            lambda x=x, b=b, N=N, img=img: F.linear_fwd_ex(x, b, N, True, img, X6, wide=True),
            [lambda x=x, d=d: F.linear_fwd_ex(x, d[1], d[2], True, d[0], X6) for d in dense])
    for Nred, K in ((256, 512),):  # the input gradient through the 512 -> 256 layer (reduction 256, 512 outputs)
        dz, w, h = rn(B, Nred), rn(Nred, K) / Nred ** 0.5, torch.nn.functional.elu(rn(B, K))
        img = F.bimage_wide(w, True)
        dense = [(F.bimage(w[:, c0:c0 + n].contiguous(), True), h[:, c0:c0 + n].contiguous()) for c0, n in blocks(K)]
        cases[f"dgrad_elu[Nred={Nred},K={K}]"] = (
            lambda dz=dz, h=h, img=img: F.linear_dgrad_elu_ex(dz, h, img, X6, want_db=False, wide=True),
            [lambda dz=dz, d=d: F.linear_dgrad_elu_ex(dz, d[1], d[0], X6, want_db=False) for d in dense])
    for N, K in ((256, 512), (512, 48)):  # the weight gradients of the two wide layers
        dz, x = rn(B, N), rn(B, K)
        if K <= 64:  # the first layer's (x^T dz)^T form on both sides
            wide = lambda dz=dz, x=x: F.linear_wgrad_wide(x, dz, bias_side=2)  # noqa: E731
            dense = [lambda x=x, d=dz[:, c0:c0 + n].contiguous(): F.linear_wgrad(x, d, bias_side=2)
                     for c0, n in blocks(N)]
        else:
            wide = lambda dz=dz, x=x: F.linear_wgrad_wide(dz, x, bias_side=1)  # noqa: E731
            dense = [lambda dz=dz, d=x[:, c0:c0 + n].contiguous(): F.linear_wgrad(dz, d, bias_side=1)
                     for c0, n in blocks(K)]
        cases[f"wgrad[N={N},K={K}]"] = (wide, dense)
    res = {}
    for name, (wide, dense) in cases.items():
        wide()
        for d in dense:
            d()
        tw, td = [], [[] for _ in dense]
        for _ in range(calls):  # alternating: the wide launch, then each dense block
            tw.append(timed(wide)[0])
            for i, d in enumerate(dense):
                td[i].append(timed(d)[0])
        dsum = [sum(t[i] for t in td) for i in range(calls)]
        res[name] = {"rows": B, "wide_us": 1e3 * float(np.median(tw)), "wide_us_min": 1e3 * min(tw),
                     "wide_us_p90": 1e3 * float(np.percentile(tw, 90)),
                     "dense_blocks_us": [1e3 * float(np.median(t)) for t in td],
                     "dense_sum_us": 1e3 * float(np.median(dsum)), "dense_sum_us_min": 1e3 * min(dsum),
                     "dense_sum_us_p90": 1e3 * float(np.percentile(dsum, 90))}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", default="4096,65536")
    ap.add_argument("--updates", type=int, default=5)
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--rollout-envs", default="", help="sizes at which only the rollout step is timed")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("wide_update_probe: needs a ROCm GPU; a CPU run measures nothing")
    dev = torch.device("cuda:0")
    res = {"shape": {"T": T, "obs": O, "actions": A, "hidden": HIDDEN, "mini_batches": M, "epochs": EPOCHS,
                     "device": torch.cuda.get_device_name(0), "tree_has_wide_path": HAS_WIDE,
                     "wide_knob_on": KNOB_ON}}
    for N in [int(x) for x in args.rollout_envs.split(",") if x]:
        res[f"rollout_envs_{N}"] = probe_rollout(N, dev)
        print(N, json.dumps(res[f"rollout_envs_{N}"]), flush=True)
        torch.cuda.empty_cache()
    for N in [int(x) for x in args.envs.split(",") if x]:
        r = {"update": probe_updates(N, dev, args.updates)}
        torch.cuda.empty_cache()
        r["rollout_step"] = probe_rollout(N, dev)
        u = r["update"]
        r["wide_median_below_off_min"] = u["wide"]["ms_per_update"] < u["off"]["ms_min"]
        if args.kernels and HAS_WIDE:
            torch.cuda.empty_cache()
            r["kernels"] = probe_kernels(N * T // M, dev)
        res[f"envs_{N}"] = r
        print(N, json.dumps(r), flush=True)
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
