"""Cost of the fused actor head at action counts other than 12.

Not a test.  Two measurements, each alternating its two variants in one process so that both see the same clocks:

  update   one PPO.update() -- obs 48, actor and critic 3 x 256 ELU, T 24, 4 mini-batches, 5 epochs -- at N envs with A
           actions: `head` (the default: the actor's last launch runs the loss and the output layer's backward) against
           `off` (RSLRL_ACTOR_HEAD=0, here the module flag held off around update(): the three launches).  One warm-up
           round, then the median of `--updates` updates with device events around update(), every sample kept.  The
           head is the default at a width where its median is below the other variant's fastest run.
  launch   the head's launch alone at M rows against the three launches it replaces (fused output-layer forward, PPO loss
           kernel, output-layer backward), `--iters` calls per event pair, the median of `--rounds` rounds.

Usage:  python scripts/actor_head_anya_probe.py [--envs 4096,65536] [--actions 6,8,10,16] [--updates 5] [--M 98304]
                                                [--out FILE.json]
"""

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rsl_rl_amd import _lib, kernels  # noqa: E402
from rsl_rl_amd.algorithms import PPO  # noqa: E402
from rsl_rl_amd.modules import ActorCritic  # noqa: E402
from rsl_rl_amd.networks import fused_mlp  # noqa: E402

T, O, HIDDEN, MB, EPOCHS = 24, 48, [256, 256, 256], 4, 5


def build(N, A, dev):
    torch.manual_seed(0)
    obs0 = {"policy": torch.zeros(N, O, device=dev)}
    pol = ActorCritic(obs0, {"policy": ["policy"], "critic": ["policy"]}, A, actor_hidden_dims=HIDDEN,
                      critic_hidden_dims=HIDDEN)
    alg = PPO(pol, num_learning_epochs=EPOCHS, num_mini_batches=MB, device=str(dev))
    alg.init_storage("rl", N, T, obs0, [A])
    return alg


def fill(alg, N, A, dev, seed):
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


def probe_update(N, A, dev, updates):
    variants = {"head": build(N, A, dev), "off": build(N, A, dev)}
    times, used, losses = {k: [] for k in variants}, {}, {}
    knob = fused_mlp._ACTOR_HEAD
    try:
        for it in range(updates + 1):  # the first round warms every shape up
            for name, alg in variants.items():
                fill(alg, N, A, dev, seed=it)
                fused_mlp._ACTOR_HEAD = knob and name == "head"
                before = fused_mlp.actor_head_launches
                ms, loss = timed(alg.update)
                used[name] = fused_mlp.actor_head_launches - before
                if it > 0:
                    times[name].append(ms)
                    losses[name] = loss
    finally:
        fused_mlp._ACTOR_HEAD = knob
    res = {k: {"ms_per_update": statistics.median(v), "ms_min": min(v), "ms_all": v,
               "actor_head_launches_per_update": used[k], "loss": losses[k]} for k, v in times.items()}
    res["head_is_default"] = res["head"]["ms_per_update"] < res["off"]["ms_min"]
    return res


def probe_launch(M, A, dev, rounds, iters):
    K = N = 256
    g = torch.Generator(device=dev).manual_seed(0)
    r = lambda *s: torch.randn(*s, device=dev, generator=g)  # noqa: E731
    x = torch.nn.functional.elu(r(M, K))
    w, b, wo, bo = r(N, K) / 16, r(N) * 0.1, r(A, N) / 16, r(A) * 0.1
    sigma = torch.rand(A, device=dev, generator=g) * 0.5 + 0.5
    old_sigma = sigma.expand(M, A).contiguous()
    acts, ologp, adv, tv, ret, omu, vals = r(M, A), r(M, 1) - 8, r(M, 1), r(M, 1), r(M, 1), r(M, A) * 0.1, r(M, 1)
    img, out_img, img_t = fused_mlp.bimages([(w, False), (wo, False, _lib.BIMAGE_LAYOUT_OUT), (wo, True)])
    head = fused_mlp.ActorHead(acts, ologp, adv, tv, ret, omu, old_sigma, sigma, clip_param=0.2, value_loss_coef=1.0,
                               entropy_coef=0.01, use_clipped=True, compute_kl=True,
                               grad_sigma=torch.empty(A, device=dev), stats=torch.empty(8, device=dev))
    head.values = vals

    def fused():
        assert fused_mlp.actor_head_fwd_bwd(x, b, N, img, bo, out_img, img_t, head) is not None

    def separate():
        h, mu = fused_mlp.linear_fwd_out_ex(x, b, N, img, _lib.ARITH_X6, None, bo, out_img, store_h=True)
        _, gmu, _, _ = kernels.ppo_loss_fwd_bwd(mu, sigma, vals, acts, ologp, adv, tv, ret, omu, old_sigma,
                                                compute_kl=True)
        fused_mlp.linear_dgrad_elu_wgrad(gmu, wo, h, img_t, want_db_prev=False)

    res = {"fused": [], "separate": []}
    for fn in (fused, separate):
        fn()
    torch.cuda.synchronize()
    for _ in range(rounds):
        for name, fn in (("fused", fused), ("separate", separate)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                fn()
            e1.record()
            torch.cuda.synchronize()
            res[name].append(e0.elapsed_time(e1) * 1000.0 / iters)
    return {k: {"median_us": round(statistics.median(v), 2), "runs_us": [round(t, 2) for t in v]}
            for k, v in res.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", default="4096,65536")
    ap.add_argument("--actions", default="6,8,10,16")
    ap.add_argument("--updates", type=int, default=5)
    ap.add_argument("--M", type=int, default=98304)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("actor_head_anya_probe: needs a GPU")
    dev = torch.device("cuda:0")
    widths = [int(a) for a in args.actions.split(",")]
    out = {"device": torch.cuda.get_device_name(dev), "abi": _lib.lib().rslrl_abi_version(),
           "config": {"T": T, "obs": O, "hidden": HIDDEN, "mini_batches": MB, "epochs": EPOCHS,
                      "updates": args.updates, "launch_rows": args.M, "rounds": args.rounds, "iters": args.iters},
           "update": {}, "launch": {}}
    for N in (int(n) for n in args.envs.split(",")):
        for A in widths:
            out["update"][f"N={N},A={A}"] = probe_update(N, A, dev, args.updates)
            torch.cuda.empty_cache()
    for A in widths:
        out["launch"][f"A={A}"] = probe_launch(args.M, A, dev, args.rounds, args.iters)
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
