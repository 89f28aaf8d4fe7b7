"""Cost of the recurrent path's bookkeeping on the synthetic shapes (T 24, obs 48, 12 actions, LSTM H 256, MLPs
3 x 256, about 2 % dones per step), at N = 4096 and N = 65536.

Not a test.  For each N, in a child process of its own under a time limit (the parent stops at the first child that
fails), on one box:
  rollout_step   one recurrent rollout step (PPO.act + process_env_step: both memories' LSTM steps, the MLPs, the
                 sample, the storage copies and the hidden-state copies) with the fused cell (kernels.lstm_cell_pair,
                 one launch for both memories) and with RSLRL_LSTM_CELL=0 (nn.LSTM), alternating in one process, median
                 over the steps of three rollouts each, with the host read-backs counted (torch's sync debug mode in
                 "warn")
  setup_kernels  the generator's set-up on the trajectory kernels (index + pad + hidden gather: everything
                 recurrent_mini_batch_generator does before its first yield)
  setup_eager    a restatement of the reference's lines in plain torch on the same GPU (this script's own code:
                 nonzero / tolist / split / pad_sequence, then per mini-batch the count of trajectory starts, slices
                 with device-tensor bounds and boolean indexing of the permuted hidden states)
Each is warmed up once, then timed with device events plus the host wall clock around it (the eager form is bound
by the host); launches are counted with torch.profiler where it is available, host read-backs with the sync debug
mode's warnings.  Writes profiles/recurrent_probe.json.

--rnn-type gru measures the same with GRU memories: kernels.gru_cell_pair against RSLRL_GRU_CELL=0 (nn.GRU); the result
keys keep their names (fused_cell, nn_lstm = the RNN library's module).

Usage:  python scripts/recurrent_probe.py [--rnn-type lstm|gru] [--envs 4096,65536] [--reps 5]
                                          [--out profiles/recurrent_probe.json]
"""

import argparse
import json
import os
import statistics
import subprocess
import sys
import time
import warnings

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

T, O, A, H, HIDDEN, M, P_DONE = 24, 48, 12, 256, [256, 256, 256], 4, 0.02
CHILD_LIMIT_S = 240


def build(N, dev, rnn_type="lstm"):
    from rsl_rl_amd.algorithms import PPO
    from rsl_rl_amd.modules import ActorCriticRecurrent
    torch.manual_seed(0)
    obs0 = {"policy": torch.zeros(N, O)}
    pol = ActorCriticRecurrent(obs0, {"policy": ["policy"], "critic": ["policy"]}, A, actor_hidden_dims=HIDDEN,
                               critic_hidden_dims=HIDDEN, rnn_hidden_dim=H, rnn_type=rnn_type)
    alg = PPO(pol, num_mini_batches=M, device=str(dev))
    alg.init_storage("rl", N, T, obs0, [A])
    return alg


def rollout(alg, N, dev, timed):
    g = torch.Generator(device=dev).manual_seed(1)
    obs = [{"policy": torch.randn(N, O, device=dev, generator=g)} for _ in range(T)]
    rew = torch.randn(N, device=dev, generator=g)
    dones = [(torch.rand(N, device=dev, generator=g) < P_DONE).long() for _ in range(T)]
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(T)]
    alg.storage.clear()
    with torch.inference_mode():
        for t in range(T):
            ev[t][0].record()
            alg.act(obs[t])
            alg.process_env_step(obs[t], rew, dones[t], {})
            ev[t][1].record()
    torch.cuda.synchronize()
    return [a.elapsed_time(b) for a, b in ev[2:]] if timed else None  # (the first steps allocate)


def setup_kernels(st):
    gen = st.recurrent_mini_batch_generator(M, 1)
    return next(gen)


def setup_eager(st):
    """The reference's generator set-up restated (utils.py:97-131 and rollout_storage.py:209-253)."""
    from torch.nn.utils.rnn import pad_sequence
    dones = st.dones.clone()
    dones[-1] = 1
    N = st.num_envs
    flat = dones.transpose(1, 0).reshape(-1)
    ends = flat.nonzero()[:, 0]
    lengths = torch.diff(ends, prepend=ends.new_full((1,), -1))
    as_list = lengths.tolist()
    padded = {}
    for k, v in st.observations.items():
        pieces = torch.split(v.transpose(1, 0).flatten(0, 1), as_list)
        pieces = pieces + (torch.zeros(T, *v.shape[2:], device=v.device),)
        padded[k] = pad_sequence(pieces)[:, :-1]
    masks = lengths > torch.arange(T, device=lengths.device).unsqueeze(1)
    d = st.dones.squeeze(-1)
    starts = torch.zeros_like(d, dtype=torch.bool)
    starts[1:] = d[:-1]
    starts[0] = True
    E = N // M
    first, out = 0, []
    for i in range(M):
        last = first + torch.sum(starts[:, i * E:(i + 1) * E])
        # boolean-mask selection of the trajectory starts (env-major), then a slice with device-tensor bounds
        hid = [torch.movedim(h, 2, 0)[starts.t()][first:last].movedim(0, 1).contiguous()
               for h in st.saved_hidden_states_a + st.saved_hidden_states_c]
        out.append(({k: v[:, first:last] for k, v in padded.items()}, masks[:, first:last], hid))
        first = last
    return out


def measure(fn, reps):
    fn()  # warm-up
    torch.cuda.synchronize()
    dev_ms, host_ms = [], []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        host_ms.append(1e3 * (time.perf_counter() - t0))
        dev_ms.append(a.elapsed_time(b))
    torch.cuda.set_sync_debug_mode("warn")
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        fn()
    torch.cuda.set_sync_debug_mode("default")
    syncs = sum("synchroniz" in str(x.message) for x in w)
    launches = None
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        launches = sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)
    except Exception as e:  # the profiler is optional here
        launches = f"unavailable: {type(e).__name__}"
    return {"event_ms_median": statistics.median(dev_ms), "event_ms": dev_ms, "wall_ms_median":
            statistics.median(host_ms), "wall_ms": host_ms, "host_syncs": syncs, "launches": launches}


def one(N, reps, rnn_type="lstm"):
    dev = torch.device("cuda:0")
    alg = build(N, dev, rnn_type)
    switch = "RSLRL_GRU_CELL" if rnn_type == "gru" else "RSLRL_LSTM_CELL"
    # the rollout step on the fused LSTM cell and on nn.LSTM (RSLRL_LSTM_CELL=0), alternating in this process
    from rsl_rl_amd.networks import fused_mlp
    step = {}
    for rep in range(3):
        for mode, name in (("1", "fused_cell"), ("0", "nn_lstm")):
            os.environ[switch] = mode
            alg.policy.reset()
            with fused_mlp.frozen_weights():  # as the runner's rollout: weight images built once per rollout
                if rep == 0:
                    rollout(alg, N, dev, timed=False)
                    torch.cuda.set_sync_debug_mode("warn")
                    with warnings.catch_warnings(record=True) as w:
                        warnings.simplefilter("always")
                        rollout(alg, N, dev, timed=False)
                    torch.cuda.set_sync_debug_mode("default")
                    # (rollout()'s own torch.cuda.synchronize() at its end is not a read-back and raises no warning)
                    step[name] = {"ms": [], "host_syncs_per_rollout": sum("synchroniz" in str(x.message) for x in w)}
                step[name]["ms"] += rollout(alg, N, dev, timed=True)
    for v in step.values():
        v["ms_median"] = statistics.median(v["ms"])
    os.environ[switch] = "1"
    st = alg.storage
    res = {"N": N, "rollout_step": step,
           "setup_kernels": measure(lambda: setup_kernels(st), reps),
           "setup_eager": measure(lambda: setup_eager(st), reps),
           "n_traj": int(st.dones[:-1].sum().item()) + N}
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rnn-type", default="lstm", choices=["lstm", "gru"])
    ap.add_argument("--envs", default="4096,65536")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "recurrent_probe.json"))
    ap.add_argument("--one", type=int, default=None, help="(internal) measure this N in this process")
    args = ap.parse_args()
    if args.one is not None:
        one(args.one, args.reps, args.rnn_type)
        return
    results = []
    for n in args.envs.split(","):
        # a fresh process per size under its own time limit; nothing more is started after a failure
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", n, "--reps", str(args.reps),
                            "--rnn-type", args.rnn_type],
                           capture_output=True, text=True, timeout=CHILD_LIMIT_S)
        if r.returncode != 0:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            sys.exit(r.returncode)
        results.append(json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]))
    out = {"rnn_type": args.rnn_type, "shapes": {"T": T, "obs": O, "actions": A, "H": H, "hidden": HIDDEN, "mini_batches": M, "p_done": P_DONE},
           "device": torch.cuda.get_device_name(0), "results": results}
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    for r in results:
        print(r["N"], "rollout step fused", round(r["rollout_step"]["fused_cell"]["ms_median"], 3), "ms, the RNN library",
              round(r["rollout_step"]["nn_lstm"]["ms_median"], 3), "ms; set-up kernels",
              round(r["setup_kernels"]["wall_ms_median"], 3), "ms wall, eager",
              round(r["setup_eager"]["wall_ms_median"], 3), "ms wall")


if __name__ == "__main__":
    main()
