"""Cost of one recurrent PPO.update() with an ActorCriticRecurrent (obs 48, 12 actions, one LSTM layer of 256 in front
of 3 x 256 ELU for the actor and the critic, T 24, 4 mini-batches, 5 epochs, 2 % dones) at N = 4096 and N = 65536.

Not a test.  For each N, on one box and in one process, alternating so that both variants see the same clocks:
  fused      PPO._recurrent_minibatch: env-major sequences, per mini-batch T paired lstm_cell_train
             launches, the MLP pair with the loss in the actor's last launch, T paired lstm_cell_bwd launches, the gate
             blocks' weight gradients; one read-back at the end
  autograd   RSLRL_RECURRENT_FUSED=0: zero-padded trajectories through nn.LSTM under autograd, the fused MLP path and
             the loss kernel behind it, two read-backs -- the parent's update, the yardstick
Each is warmed up once, then timed over `--updates` updates with device events around update(); the median is reported
with every sample and the peak device allocation of an update (DESIGN §14's protocol).  The two pair kernels are timed
on their own at E = N / 4 rows: an event pair around each of 20 calls, medians.

--rnn-type gru measures the same shape with one GRU layer of 256: gru_cell_train_pair /
gru_cell_bwd_pair, one saved state per memory.

Usage:  python scripts/recurrent_update_probe.py [--rnn-type lstm|gru] [--envs 4096,65536] [--updates 5] [--out FILE.json]
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

T, O, A, HIDDEN, H, M, EPOCHS, P_DONE = 24, 48, 12, [256, 256, 256], 256, 4, 5, 0.02


def build(N, dev, rnn_type="lstm"):
    torch.manual_seed(0)
    obs0 = {"policy": torch.zeros(N, O, device=dev)}
    pol = ActorCriticRecurrent(obs0, {"policy": ["policy"], "critic": ["policy"]}, A, actor_hidden_dims=HIDDEN,
                               critic_hidden_dims=HIDDEN, rnn_hidden_dim=H, rnn_type=rnn_type)
    alg = PPO(pol, num_learning_epochs=EPOCHS, num_mini_batches=M, device=str(dev))
    alg.init_storage("rl", N, T, obs0, [A])
    return alg


def fill(alg, N, dev, seed):
    """A storage as a rollout leaves it, from a seeded generator: actions drawn around a small stored mean with the
    stored std, their log-prob, saved states that are zero at a trajectory start, returns from the GAE kernel."""
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


def probe_updates(N, dev, updates, rnn_type="lstm"):
    variants = {"fused": build(N, dev, rnn_type), "autograd": build(N, dev, rnn_type)}
    times, peaks, losses = {k: [] for k in variants}, {}, {}
    launches = []
    pair_name = f"{rnn_type}_cell_train_pair"
    inner = getattr(kernels, pair_name)

    def spy(*a, **k):
        launches.append(1)
        return inner(*a, **k)

    setattr(kernels, pair_name, spy)
    try:
        for it in range(updates + 1):  # the first round warms every shape up
            for name, alg in variants.items():
                fill(alg, N, dev, seed=it)
                os.environ["RSLRL_RECURRENT_FUSED"] = "0" if name == "autograd" else "1"
                torch.cuda.reset_peak_memory_stats(dev)
                before = len(launches)
                ms, loss = timed(alg.update)
                assert (len(launches) - before) == (EPOCHS * M * T if name == "fused" else 0), (name, len(launches))
                if it > 0:
                    times[name].append(ms)
                    losses[name] = loss
                    peaks[name] = torch.cuda.max_memory_allocated(dev)
    finally:
        setattr(kernels, pair_name, inner)
        os.environ.pop("RSLRL_RECURRENT_FUSED", None)
    return {k: {"ms_per_update": float(np.median(v)), "ms_min": min(v), "ms_all": v, "peak_allocated_bytes": peaks[k],
                "loss": losses[k]} for k, v in times.items()}


def probe_kernels(E, dev, calls=20):
    g = torch.Generator(device=dev).manual_seed(3)
    rn = lambda *s: torch.randn(*s, device=dev, generator=g)  # noqa: E731
    fwd_args, bwd_args = [], []
    for _ in range(2):
        w_ih, w_hh, b = rn(4 * H, O) / 16, rn(4 * H, H) / 16, rn(4 * H) / 16
        reset = (torch.rand(E, device=dev, generator=g) < P_DONE).to(torch.uint8)
        gates, dg = torch.empty(4, 2, E, H, device=dev), torch.empty(4, 2, E, H, device=dev)
        dg[:, 1].normal_(generator=g)
        c, cout = rn(E, H), torch.empty(E, H, device=dev)
        fwd_args.append(dict(x=rn(E, O), state=(rn(E, H), c), image=kernels.lstm_image(w_ih, w_hh), b_ih=b, b_hh=b,
                             reset=reset, h_out=torch.empty(E, H, device=dev), c_out=cout, gates=gates[:, 0],
                             h_restart=rn(E, H), c_restart=rn(E, H), h_in_out=torch.empty(E, H, device=dev)))
        bwd_args.append(dict(dh=rn(E, H), gates=gates[:, 0], c_out=cout, c_prev=c, reset_cur=reset, dg_next=dg[:, 1],
                             dc_next=rn(E, H), reset_next=reset, whh_t_image=kernels.lstm_whh_t_image(w_hh),
                             dg=dg[:, 0], dc_prev=torch.empty(E, H, device=dev), c_restart=rn(E, H)))
    res = {}
    for name, fn in (("lstm_cell_train_pair", lambda: kernels.lstm_cell_train_pair(*fwd_args)),
                     ("lstm_cell_bwd_pair", lambda: kernels.lstm_cell_bwd_pair(*bwd_args))):
        fn()
        t = [timed(fn)[0] for _ in range(calls)]
        res[name] = {"rows": E, "call_us": 1e3 * float(np.median(t)), "call_us_min": 1e3 * min(t)}
    return res


def probe_gru_kernels(E, dev, calls=20):
    g = torch.Generator(device=dev).manual_seed(3)
    rn = lambda *s: torch.randn(*s, device=dev, generator=g)  # noqa: E731
    fwd_args, bwd_args = [], []
    for _ in range(2):
        w_ih, w_hh, b = rn(3 * H, O) / 16, rn(3 * H, H) / 16, rn(3 * H) / 16
        reset = (torch.rand(E, device=dev, generator=g) < P_DONE).to(torch.uint8)
        gates, dg = torch.empty(4, 2, E, H, device=dev), torch.empty(4, 2, E, H, device=dev)
        dg[:, 1].normal_(generator=g)
        hin = torch.empty(E, H, device=dev)
        fwd_args.append(dict(x=rn(E, O), h=rn(E, H), image=kernels.gru_image(w_ih, w_hh), b_ih=b, b_hh=b, reset=reset,
                             h_out=torch.empty(E, H, device=dev), gates=gates[:, 0], h_restart=rn(E, H), h_in_out=hin))
        bwd_args.append(dict(dh=rn(E, H), gates=gates[:, 0], h_in=hin, dg_next=dg[:, 1], dhz_next=rn(E, H),
                             reset_next=reset, whh_t_image=kernels.gru_whh_t_image(w_hh), dg=dg[:, 0],
                             dhz_out=torch.empty(E, H, device=dev)))
    res = {}
    for name, fn in (("gru_cell_train_pair", lambda: kernels.gru_cell_train_pair(*fwd_args)),
                     ("gru_cell_bwd_pair", lambda: kernels.gru_cell_bwd_pair(*bwd_args))):
        fn()
        t = [timed(fn)[0] for _ in range(calls)]
        res[name] = {"rows": E, "call_us": 1e3 * float(np.median(t)), "call_us_min": 1e3 * min(t)}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rnn-type", default="lstm", choices=["lstm", "gru"])
    ap.add_argument("--envs", default="4096,65536")
    ap.add_argument("--updates", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("recurrent_update_probe: needs a ROCm GPU; a CPU run measures nothing")
    dev = torch.device("cuda:0")
    res = {"shape": {"T": T, "obs": O, "actions": A, "hidden": HIDDEN, args.rnn_type: H, "mini_batches": M, "epochs": EPOCHS,
                     "p_done": P_DONE, "device": torch.cuda.get_device_name(0)}}
    for N in [int(x) for x in args.envs.split(",")]:
        kernel_probe = probe_gru_kernels if args.rnn_type == "gru" else probe_kernels
        r = {"update": probe_updates(N, dev, args.updates, args.rnn_type), "kernels": kernel_probe(N // M, dev)}
        u = r["update"]
        r["fused_median_below_autograd_min"] = u["fused"]["ms_per_update"] < u["autograd"]["ms_min"]
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
