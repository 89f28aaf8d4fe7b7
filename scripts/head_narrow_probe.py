"""Cost of the fused heads on a last hidden layer narrower than 256 (the narrow heads, ABI 34).

Not a test.  Two measurements, each alternating its two variants in one process so that both see the same clocks:

  update   one PPO.update() -- 12 actions, T 24, 4 mini-batches, 5 epochs -- at N envs, for obs 48 and obs 235 and the
           hidden stacks [512, 256, 128] (one pass per network) and [256, 256, 128] (the paired pass): `heads` (the
           critic's and the actor's last launches run the loss and the output layers' backward) against `off`
           (RSLRL_HEAD_NARROW=0, here the module flag held off around update(): linear_fwd_out twice, the loss kernel,
           linear_dgrad_elu_wgrad twice).  One warm-up round, then the median of `--updates` updates with device events
           around update(), every sample kept.  The heads are the default at a shape where their median is below the
           other variant's fastest run.
  launch   the two heads' launches alone at the mini-batch's M rows (N = 128, K = 256) against the launches they
           replace -- actor: fused output-layer forward, PPO loss kernel, output-layer backward; critic: the forward and
           the backward (the loss kernel is counted once, with the actor) -- `--iters` calls per event pair, the median
           of `--rounds` rounds.

Usage:  python scripts/head_narrow_probe.py [--envs 4096,65536] [--obs 48,235] [--updates 5] [--out FILE.json]
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

T, A, MB, EPOCHS = 24, 12, 4, 5
STACKS = {"512-256-128": [512, 256, 128], "256-256-128": [256, 256, 128]}


def build(N, O, hidden, dev):
    torch.manual_seed(0)
    obs0 = {"policy": torch.zeros(N, O, device=dev)}
    pol = ActorCritic(obs0, {"policy": ["policy"], "critic": ["policy"]}, A, actor_hidden_dims=hidden,
                      critic_hidden_dims=hidden)
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


def probe_update(N, O, hidden, dev, updates):
    variants = {"heads": build(N, O, hidden, dev), "off": build(N, O, hidden, dev)}
    times, used, losses = {k: [] for k in variants}, {}, {}
    knob = fused_mlp._HEAD_NARROW
    try:
        for it in range(updates + 1):  # the first round warms every shape up
            for name, alg in variants.items():
                fill(alg, N, O, dev, seed=it)
                fused_mlp._HEAD_NARROW = name == "heads"
                before = fused_mlp.actor_head_launches
                ms, loss = timed(alg.update)
                used[name] = fused_mlp.actor_head_launches - before
                if it > 0:
                    times[name].append(ms)
                    losses[name] = loss
    finally:
        fused_mlp._HEAD_NARROW = knob
    res = {k: {"ms_per_update": statistics.median(v), "ms_min": min(v), "ms_all": v,
               "actor_head_launches_per_update": used[k], "loss": losses[k]} for k, v in times.items()}
    res["heads_are_default"] = res["heads"]["ms_per_update"] < res["off"]["ms_min"]
    res["heads_vs_off"] = res["heads"]["ms_per_update"] / res["off"]["ms_per_update"]
    return res


def probe_launch(M, N, dev, rounds, iters):
    K = 256
    g = torch.Generator(device=dev).manual_seed(0)
    r = lambda *s: torch.randn(*s, device=dev, generator=g)  # noqa: E731
    x = torch.nn.functional.elu(r(M, K))
    w, b, wo, bo = r(N, K) / 16, r(N) * 0.1, r(A, N) / 16, r(A) * 0.1
    wv, bv = r(1, N) / 16, r(1) * 0.1
    sigma = torch.rand(A, device=dev, generator=g) * 0.5 + 0.5
    old_sigma = sigma.expand(M, A).contiguous()
    acts, ologp, adv, tv, ret, omu, vals = r(M, A), r(M, 1) - 8, r(M, 1), r(M, 1), r(M, 1), r(M, A) * 0.1, r(M, 1)
    img, out_img, img_t, outv_img, imgv_t = fused_mlp.bimages(
        [(w, False), (wo, False, _lib.BIMAGE_LAYOUT_OUT), (wo, True), (wv, False, _lib.BIMAGE_LAYOUT_OUT), (wv, True)])
    head = fused_mlp.ActorHead(acts, ologp, adv, tv, ret, omu, old_sigma, sigma, clip_param=0.2, value_loss_coef=1.0,
                               entropy_coef=0.01, use_clipped=True, compute_kl=True,
                               grad_sigma=torch.empty(A, device=dev), stats=torch.empty(8, device=dev))
    head.values = vals
    vhead = fused_mlp.ValueHead(tv, ret, 0.2, 1.0, True)
    dv = r(M, 1) / M

    def actor_fused():
        assert fused_mlp.actor_head_fwd_bwd(x, b, N, img, bo, out_img, img_t, head) is not None

    def actor_separate():
        h, mu = fused_mlp.linear_fwd_out_ex(x, b, N, img, _lib.ARITH_X6, None, bo, out_img, store_h=True)
        _, gmu, _, _ = kernels.ppo_loss_fwd_bwd(mu, sigma, vals, acts, ologp, adv, tv, ret, omu, old_sigma,
                                                compute_kl=True)
        fused_mlp.linear_dgrad_elu_wgrad(gmu, wo, h, img_t, want_db_prev=False)

    def critic_fused():
        assert fused_mlp.value_head_fwd_bwd(x, b, N, img, bv, outv_img, wv, vhead) is not None

    def critic_separate():
        h, _ = fused_mlp.linear_fwd_out_ex(x, b, N, img, _lib.ARITH_X6, None, bv, outv_img, store_h=True)
        fused_mlp.linear_dgrad_elu_wgrad(dv, wv, h, imgv_t, want_db_prev=False)

    fns = {"actor_fused": actor_fused, "actor_separate": actor_separate, "critic_fused": critic_fused,
           "critic_separate": critic_separate}
    res = {k: [] for k in fns}
    knob = fused_mlp._HEAD_NARROW
    fused_mlp._HEAD_NARROW = True
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
        fused_mlp._HEAD_NARROW = knob
    return {k: {"median_us": round(statistics.median(v), 2), "runs_us": [round(t, 2) for t in v]}
            for k, v in res.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", default="4096,65536")
    ap.add_argument("--obs", default="48,235")
    ap.add_argument("--updates", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("head_narrow_probe: needs a GPU")
    dev = torch.device("cuda:0")
    envs = [int(n) for n in args.envs.split(",")]
    out = {"device": torch.cuda.get_device_name(dev), "abi": _lib.lib().rslrl_abi_version(),
           "config": {"T": T, "actions": A, "mini_batches": MB, "epochs": EPOCHS, "updates": args.updates,
                      "rounds": args.rounds, "iters": args.iters, "stacks": STACKS},
           "update": {}, "launch": {}}
    for N in envs:
        for O in (int(o) for o in args.obs.split(",")):
            for name, hidden in STACKS.items():
                out["update"][f"N={N},obs={O},hidden={name}"] = probe_update(N, O, hidden, dev, args.updates)
                torch.cuda.empty_cache()
    for N in envs:
        M = T * N // MB
        out["launch"][f"M={M},N=128"] = probe_launch(M, 128, dev, args.rounds, args.iters)
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
