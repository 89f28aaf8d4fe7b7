"""Cost of the fused recurrent path at hidden size 512: one PPO.update() and one rollout step of
an ActorCriticRecurrent (12 actions, one LSTM or GRU layer in front of [512, 256, 128] ELU for the actor and the
critic, T 24, 4 mini-batches, 5 epochs, 2 % dones -- legged_gym's recurrent default) with a 512-wide memory at obs 48
and 235, and with a 256-wide memory at obs 48 (the wide MLP behind a memory), N = 4096 and
65536.

Not a test.  Per (rnn type, memory, obs, N), on one box and in one process, alternating so that both variants see the
same clocks:
  feature    the routing of this tree: the `_h` cell kernels, the update without autograd (at every size: the row
             gate kernels.RNN_H512_LSTM_UPDATE_MIN_ROWS, which this probe's figures set, is held open)
  off        what the tree did before: RSLRL_RNN_HIDDEN_512=0 (the module flag kernels._RNN_HIDDEN_512, which that
             variable sets at import) for a 512-wide memory -- nn.LSTM / nn.GRU in the rollout, autograd in the update;
             RSLRL_RECURRENT_FUSED=0 for the 256-wide one, whose rollout step does not change and is not timed
The variants are switched inside the process (the module flag, the environment variable that
PPO._recurrent_fused_ok reads per call), not by starting processes with the variables set.  That relies on nothing
caching a decision made under the other value: Cell.takes, Memory.fused_cell and manual_update_ok are evaluated on
every call, and the memories' weight images live only inside one frozen_weights() scope.
Each is warmed up once, then timed over five rounds with device events; medians, every sample and each variant's
fastest run kept, and the peak allocation of an update (torch.cuda.max_memory_allocated above what was allocated when
it began).  An `off` update that the RNN library refuses (a RuntimeError from its argument check) is recorded as failed
and not tried again.  The rollout step is
ActorCriticRecurrent.act_and_evaluate inside fused_mlp.frozen_weights() (the runner's rollout).

--kernels times the pair forms of the rollout step, the training step and the reverse step on their own at hidden 512
against their 256 twins (obs 48; 1,024 and 16,384 rows): an event pair around each of 20 calls, medians, and the ratio.

Usage:  python scripts/rnn_h512_probe.py [--rnn-types lstm,gru] [--envs 4096,65536] [--rounds 5] [--kernels]
                                         [--out FILE.json]
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

T, A, HIDDEN, M, EPOCHS, P_DONE = 24, 12, [512, 256, 128], 4, 5, 0.02
CONFIGS = ((512, 48), (512, 235), (256, 48))  # (memory, obs)


def set_variant(feature, H):
    kernels._RNN_HIDDEN_512 = feature
    kernels.RNN_H512_LSTM_UPDATE_MIN_ROWS = 0  # the row gate of the LSTM update is what this probe decides: open
    if H == 256 and not feature:
        os.environ["RSLRL_RECURRENT_FUSED"] = "0"
    else:
        os.environ.pop("RSLRL_RECURRENT_FUSED", None)


def build(N, O, H, dev, rnn_type):
    torch.manual_seed(0)
    obs0 = {"policy": torch.zeros(N, O, device=dev)}
    pol = ActorCriticRecurrent(obs0, {"policy": ["policy"], "critic": ["policy"]}, A, actor_hidden_dims=HIDDEN,
                               critic_hidden_dims=HIDDEN, rnn_hidden_dim=H, rnn_type=rnn_type)
    alg = PPO(pol, num_learning_epochs=EPOCHS, num_mini_batches=M, device=str(dev))
    alg.init_storage("rl", N, T, obs0, [A])
    return alg


def fill(alg, N, O, H, dev, seed):
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


VARIANTS = {"feature": True, "off": False}


def probe_updates(N, O, H, dev, rounds, rnn_type):
    alg = build(N, O, H, dev, rnn_type)  # one policy and storage: the variants differ in routing only
    times, peaks, fused, failed = {k: [] for k in VARIANTS}, {k: 0 for k in VARIANTS}, {}, {}
    launches = []
    pair_name = f"{rnn_type}_cell_train_pair"
    inner = getattr(kernels, pair_name)

    def spy(*a, **k):
        launches.append(1)
        return inner(*a, **k)

    setattr(kernels, pair_name, spy)
    try:
        for it in range(rounds + 1):  # the first round warms every shape up
            for name, feature in VARIANTS.items():
                set_variant(feature, H)
                fill(alg, N, O, H, dev, seed=it)
                before = len(launches)
                if name in failed:
                    continue
                torch.cuda.reset_peak_memory_stats()  # (the caching allocator stays warm, as in a training run)
                base = torch.cuda.memory_allocated()
                try:
                    ms, _ = timed(alg.update)
                except RuntimeError as e:  # the RNN library refuses some sizes (an argument check, nothing has run)
                    if name == "feature":
                        raise
                    failed[name] = str(e).splitlines()[0][:200]
                    continue
                peaks[name] = max(peaks[name], torch.cuda.max_memory_allocated() - base)
                fused[name] = (len(launches) - before) == EPOCHS * M * T
                if it > 0:
                    times[name].append(ms)
    finally:
        setattr(kernels, pair_name, inner)
        set_variant(True, H)
    return {k: (dict(failed=failed[k]) if k in failed else
                dict(summary(v), fused_update=fused[k], peak_update_bytes=peaks[k])) for k, v in times.items()}


def probe_rollout(N, O, H, dev, rounds, rnn_type, steps=8):
    """ms per act_and_evaluate call: `steps` chained calls per sample inside one frozen_weights() scope."""
    pol = build(N, O, H, dev, rnn_type).policy
    obs = {"policy": torch.randn(N, O, device=dev)}
    times, cell = {k: [] for k in VARIANTS}, {}
    try:
        for it in range(rounds + 1):
            for name, feature in VARIANTS.items():
                set_variant(feature, H)

                def run():
                    with torch.inference_mode(), fused_mlp.frozen_weights():
                        for _ in range(steps):
                            pol.act_and_evaluate(obs)

                with torch.inference_mode():
                    cell[name] = pol.memory_a.fused_cell(obs["policy"]) is not None
                pol.reset()
                ms, _ = timed(run)
                if it > 0:
                    times[name].append(ms / steps)
    finally:
        set_variant(True, H)
    return {k: dict(summary(v), fused_cell=cell[k]) for k, v in times.items()}


def probe_kernels(E, dev, rnn_type, O=48, calls=20):
    """The pair forms of the rollout step, the training step and the reverse step at hidden 512 and 256."""
    cell = kernels.LSTM if rnn_type == "lstm" else kernels.GRU
    G, n = cell.blocks, cell.n_state
    res = {}
    for H in (512, 256):
        g = torch.Generator(device=dev).manual_seed(3)
        rn = lambda *s: torch.randn(*s, device=dev, generator=g)  # noqa: E731
        new = lambda *s: torch.empty(*s, device=dev)  # noqa: E731
        step_args, train_ops, bwd_ops = [], [], []
        for _ in range(2):
            w_ih, w_hh, b = rn(G * H, O) / 16, rn(G * H, H) / 16, rn(G * H) / 16
            img, whh_t, x = cell.image(w_ih, w_hh), cell.whh_t_image(w_hh), rn(E, O)
            reset = (torch.rand(E, device=dev, generator=g) < P_DONE).to(torch.uint8)
            state, restart = tuple(rn(E, H) for _ in range(n)), tuple(rn(E, H) for _ in range(n))
            out, gates, hin = tuple(new(E, H) for _ in range(n)), rn(4, E, H).sigmoid(), rn(E, H)
            step = (state, out, reset, restart, hin)
            step_args += [x, state, img, b, b]
            train_ops.append(cell.train_operands(x, img, b, b, gates, step, hin))
            bwd_ops.append(cell.bwd_operands(rn(E, H), gates, (state, tuple(rn(E, H) for _ in range(n)), reset, restart,
                                                               hin), rn(4, E, H), rn(E, H), reset, whh_t, new(4, E, H),
                                             new(E, H)))
        for name, fn in ((f"{rnn_type}_cell_pair", lambda: cell.step_pair(*step_args)),
                         (f"{rnn_type}_cell_train_pair", lambda: cell.train_pair(*train_ops)),
                         (f"{rnn_type}_cell_bwd_pair", lambda: cell.bwd_pair(*bwd_ops))):
            fn()
            t = [1e3 * timed(fn)[0] for _ in range(calls)]
            res.setdefault(name, {})[f"hidden_{H}"] = dict(summary(t, "us"), rows=E, obs=O)
    for r in res.values():
        r["ratio_512_to_256"] = r["hidden_512"]["us_median"] / r["hidden_256"]["us_median"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rnn-types", default="lstm,gru")
    ap.add_argument("--envs", default="4096,65536")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("rnn_h512_probe: needs a ROCm GPU; a CPU run measures nothing")
    dev = torch.device("cuda:0")
    res = {"shape": {"T": T, "actions": A, "hidden": HIDDEN, "mini_batches": M, "epochs": EPOCHS, "p_done": P_DONE,
                     "device": torch.cuda.get_device_name(0), "rounds": args.rounds}}

    def save():
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                json.dump(res, f, indent=1)
                f.write("\n")

    for rnn_type in args.rnn_types.split(","):
        if args.kernels:
            for E in (1024, 16384):
                res[f"{rnn_type}_kernels_rows{E}"] = r = probe_kernels(E, dev, rnn_type)
                print(rnn_type, "kernels", E, json.dumps({k: (v["hidden_512"]["us_median"], v["hidden_256"]["us_median"])
                                                          for k, v in r.items()}), flush=True)
            save()
            continue
        for H, O in CONFIGS:
            for N in [int(x) for x in args.envs.split(",")]:
                r = {"update": probe_updates(N, O, H, dev, args.rounds, rnn_type)}
                if H == 512:
                    r["rollout_step"] = probe_rollout(N, O, H, dev, args.rounds, rnn_type)
                for p in r.values():
                    if "failed" not in p["off"]:
                        p["feature_median_below_off_min"] = p["feature"]["ms_median"] < p["off"]["ms_min"]
                res[f"{rnn_type}_h{H}_obs{O}_envs{N}"] = r
                print(rnn_type, H, O, N, json.dumps(r), flush=True)
                save()
                torch.cuda.empty_cache()
    save()


if __name__ == "__main__":
    main()
