"""Cost of the fused recurrent path at observation widths that are no multiple of 16: one
PPO.update() and one rollout step of an ActorCriticRecurrent (12 actions, one LSTM or GRU layer of 256 in front of
3 x 256 ELU for the actor and the critic, T 24, 4 mini-batches, 5 epochs, 2 % dones -- the shape of
scripts/recurrent_update_probe.py) at obs 45 and 235, N = 4096 and 65536.

Not a test.  Per (rnn type, obs, N), on one box and in one process, alternating so that every variant sees the same
clocks:
  anyd       the routing of this tree: the `_anyd` cell kernels, dW_ih on the ragged weight-gradient kernel
  knob_off   RSLRL_RNN_ANY_INPUT=0 (the module flag kernels._RNN_ANY_INPUT, which that variable sets at import): the
             width is refused, the update runs nn.LSTM / nn.GRU under autograd, the rollout step the RNN library
  neighbour  the next multiple of 16 (obs 48 / 240) on the first kernels
and, for the rollout step only,
  nn         RSLRL_LSTM_CELL=0 / RSLRL_GRU_CELL=0: nn.LSTM / nn.GRU
Each is warmed up once, then timed over five rounds with device events; medians, every sample kept.  The rollout step
is ActorCriticRecurrent.act_and_evaluate inside fused_mlp.frozen_weights() (the runner's rollout).  The cell kernels
are timed on their own at E = N / 4 rows (pair forms, rollout and training) at each width and its neighbour: an event
pair around each of 20 calls, medians, and the ratio.

--tree-default measures one variant only, whatever routing the imported tree has, and touches no name that an older
tree lacks: run from a checkout of the parent commit it shows what that tree does at these widths.

Usage:  python scripts/rnn_anyd_probe.py [--rnn-types lstm,gru] [--obs 45,235] [--envs 4096,65536] [--rounds 5]
                                         [--tree-default] [--out FILE.json]
"""

import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rsl_rl_amd import kernels  # noqa: E402
from rsl_rl_amd.algorithms import PPO  # noqa: E402
from rsl_rl_amd.modules import ActorCriticRecurrent  # noqa: E402
from rsl_rl_amd.networks import fused_mlp  # noqa: E402

T, A, HIDDEN, H, M, EPOCHS, P_DONE = 24, 12, [256, 256, 256], 256, 4, 5, 0.02
CELL_SWITCH = {"lstm": "RSLRL_LSTM_CELL", "gru": "RSLRL_GRU_CELL"}


def set_knob(on):
    if hasattr(kernels, "_RNN_ANY_INPUT"):
        kernels._RNN_ANY_INPUT = on


def build(N, O, dev, rnn_type):
    torch.manual_seed(0)
    obs0 = {"policy": torch.zeros(N, O, device=dev)}
    pol = ActorCriticRecurrent(obs0, {"policy": ["policy"], "critic": ["policy"]}, A, actor_hidden_dims=HIDDEN,
                               critic_hidden_dims=HIDDEN, rnn_hidden_dim=H, rnn_type=rnn_type)
    alg = PPO(pol, num_learning_epochs=EPOCHS, num_mini_batches=M, device=str(dev))
    alg.init_storage("rl", N, T, obs0, [A])
    return alg


def fill(alg, N, O, dev, seed):
    """A storage as a rollout leaves it (scripts/recurrent_update_probe.py's)."""
    g = torch.Generator(device=dev).manual_seed(seed)
    rn = lambda *s: torch.randn(*s, device=dev, generator=g)  # noqa: E731
    st = alg.storage
    st.observations["policy"].copy_(rn(T, N, O))
    st.rewards.copy_(rn(T, N, 1))
    st.dones.copy_((torch.rand(T, N, 1, device=dev, generator=g) < P_DONE).to(torch.uint8))
    mu, sigma = 0.1 * rn(T, N, A), torch.ones(T, N, A, device=dev)
    actions = mu + sigma * rn(T, N, A)
    st.mu.copy_(mu)
    st.sigma.copy_(sigma)
    st.actions.copy_(actions)
    st.values.copy_(0.1 * rn(T, N, 1))
    st.actions_log_prob.copy_(torch.distributions.Normal(mu, sigma).log_prob(actions).sum(-1, keepdim=True))
    live = torch.ones(T, 1, N, 1, device=dev)
    live[1:] = (st.dones[:T - 1] == 0).view(T - 1, 1, N, 1)
    n_states = 1 if isinstance(alg.policy.memory_a.rnn, torch.nn.GRU) else 2
    st.saved_hidden_states_a = [0.3 * rn(T, 1, N, H) * live for _ in range(n_states)]
    st.saved_hidden_states_c = [0.3 * rn(T, 1, N, H) * live for _ in range(n_states)]
    st.step = T
    with torch.inference_mode():
        alg.policy.reset()
        alg.compute_returns({"policy": rn(N, O)})


def timed(fn):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    out = fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end), out


def summary(v, unit="ms"):
    return {f"{unit}_median": float(np.median(v)), f"{unit}_min": min(v), f"{unit}_all": v}


def variants_of(O, tree_default):
    """{name: (obs width, knob)}"""
    if tree_default:
        return {"tree_default": (O, None)}
    return {"anyd": (O, True), "knob_off": (O, False), "neighbour": (-(-O // 16) * 16, True)}


def probe_updates(N, O, dev, rounds, rnn_type, tree_default):
    vs = variants_of(O, tree_default)
    algs = {k: build(N, w, dev, rnn_type) for k, (w, _) in vs.items()}
    times, fused = {k: [] for k in vs}, {}
    launches = []
    pair_name = f"{rnn_type}_cell_train_pair"
    inner = getattr(kernels, pair_name)

    def spy(*a, **k):
        launches.append(1)
        return inner(*a, **k)

    setattr(kernels, pair_name, spy)
    try:
        for it in range(rounds + 1):  # the first round warms every shape up
            for name, (w, knob) in vs.items():
                if knob is not None:
                    set_knob(knob)
                fill(algs[name], N, w, dev, seed=it)
                before = len(launches)
                ms, _ = timed(algs[name].update)
                fused[name] = (len(launches) - before) == EPOCHS * M * T
                if it > 0:
                    times[name].append(ms)
    finally:
        setattr(kernels, pair_name, inner)
        set_knob(True)
    return {k: dict(summary(v), obs=vs[k][0], fused_update=fused[k]) for k, v in times.items()}


def probe_rollout(N, O, dev, rounds, rnn_type, tree_default, steps=8):
    """ms per act_and_evaluate call: `steps` chained calls per sample inside one frozen_weights() scope."""
    vs = dict(variants_of(O, tree_default))
    if not tree_default:
        vs["nn"] = (O, True)
    pols, obs = {}, {}
    for k, (w, _) in vs.items():
        pols[k] = build(N, w, dev, rnn_type).policy
        obs[k] = {"policy": torch.randn(N, w, device=dev)}
    times, cell = {k: [] for k in vs}, {}
    try:
        for it in range(rounds + 1):
            for name, (w, knob) in vs.items():
                if knob is not None:
                    set_knob(knob)
                os.environ[CELL_SWITCH[rnn_type]] = "0" if name == "nn" else "1"
                pol = pols[name]

                def run():
                    with torch.inference_mode(), fused_mlp.frozen_weights():
                        for _ in range(steps):
                            pol.act_and_evaluate(obs[name])  # noqa: B023

                with torch.inference_mode():
                    x = obs[name]["policy"]
                    cell[name] = pol.memory_a.fused_cell(x) is not None
                pol.reset()
                ms, _ = timed(run)
                if it > 0:
                    times[name].append(ms / steps)
    finally:
        os.environ.pop(CELL_SWITCH[rnn_type], None)
        set_knob(True)
    return {k: dict(summary(v), obs=vs[k][0], fused_cell=cell[k]) for k, v in times.items()}


def probe_kernels(E, O, dev, rnn_type, calls=20):
    """The pair forms of the rollout step and of the training step at width O and at its 16-aligned neighbour."""
    G = 4 if rnn_type == "lstm" else 3
    res = {}
    for w in (O, -(-O // 16) * 16):
        g = torch.Generator(device=dev).manual_seed(3)
        rn = lambda *s: torch.randn(*s, device=dev, generator=g)  # noqa: E731
        step_args, train_args = [], []
        image = kernels.lstm_image if rnn_type == "lstm" else kernels.gru_image
        for _ in range(2):
            w_ih, w_hh, b = rn(G * H, w) / 16, rn(G * H, H) / 16, rn(G * H) / 16
            img, x = image(w_ih, w_hh), rn(E, w)
            reset = (torch.rand(E, device=dev, generator=g) < P_DONE).to(torch.uint8)
            new = lambda *s: torch.empty(*s, device=dev)  # noqa: E731
            if rnn_type == "lstm":
                step_args += [x, (rn(E, H), rn(E, H)), img, b, b]
                train_args.append(dict(x=x, state=(rn(E, H), rn(E, H)), image=img, b_ih=b, b_hh=b, reset=reset,
                                       h_out=new(E, H), c_out=new(E, H), gates=new(4, E, H), h_restart=rn(E, H),
                                       c_restart=rn(E, H), h_in_out=new(E, H)))
            else:
                step_args += [x, rn(E, H), img, b, b]
                train_args.append(dict(x=x, h=rn(E, H), image=img, b_ih=b, b_hh=b, reset=reset, h_out=new(E, H),
                                       gates=new(4, E, H), h_restart=rn(E, H), h_in_out=new(E, H)))
        pair = getattr(kernels, f"{rnn_type}_cell_pair")
        train_pair = getattr(kernels, f"{rnn_type}_cell_train_pair")
        for name, fn in ((f"{rnn_type}_cell_pair", lambda: pair(*step_args)),
                         (f"{rnn_type}_cell_train_pair", lambda: train_pair(*train_args))):
            fn()
            t = [1e3 * timed(fn)[0] for _ in range(calls)]
            res.setdefault(name, {})[f"obs_{w}"] = dict(summary(t, "us"), rows=E)
    for name, r in res.items():
        a, b = (r[f"obs_{w}"]["us_median"] for w in (O, -(-O // 16) * 16))
        r["ratio_to_neighbour"] = a / b
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rnn-types", default="lstm,gru")
    ap.add_argument("--obs", default="45,235")
    ap.add_argument("--envs", default="4096,65536")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--tree-default", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("rnn_anyd_probe: needs a ROCm GPU; a CPU run measures nothing")
    dev = torch.device("cuda:0")
    res = {"shape": {"T": T, "actions": A, "hidden": HIDDEN, "memory": H, "mini_batches": M, "epochs": EPOCHS,
                     "p_done": P_DONE, "device": torch.cuda.get_device_name(0), "rounds": args.rounds,
                     "tree_default": args.tree_default}}
    for rnn_type in args.rnn_types.split(","):
        for O in [int(x) for x in args.obs.split(",")]:
            for N in [int(x) for x in args.envs.split(",")]:
                r = {"update": probe_updates(N, O, dev, args.rounds, rnn_type, args.tree_default),
                     "rollout_step": probe_rollout(N, O, dev, args.rounds, rnn_type, args.tree_default)}
                if not args.tree_default:
                    r["kernels"] = probe_kernels(N // M, O, dev, rnn_type)
                    for part in ("update", "rollout_step"):
                        p = r[part]
                        p["anyd_median_below_others_min"] = {
                            k: p["anyd"]["ms_median"] < p[k]["ms_min"] for k in p if k not in ("anyd", "neighbour")}
                res[f"{rnn_type}_obs{O}_envs{N}"] = r
                print(rnn_type, O, N, json.dumps(r), flush=True)
                torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
