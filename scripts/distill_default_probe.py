"""Cost of Distillation.update() and of the distillation rollout step for the students DESIGN.md §23 moved onto the
window-batched update, on the protocol of scripts/distill_probe.py: T 24, gradient_length 15, one epoch, 12 actions,
teacher obs 235 with [512, 256, 128], at N = 4096 and N = 65536, for

  wide48     a [512, 256, 128] student at obs 48
  wide45     a [512, 256, 128] student at obs 45 (a ragged first layer)
  gru_wide   a GRU-256 student (obs 48) in front of [512, 256, 128]
  gru_3x256  a GRU-256 student (obs 48) in front of 3 x 256

Not a test.  Per student and N, in one process and alternating so that every variant sees the same clocks:
  update   windows (the default) against per_step (RSLRL_DISTILL_FUSED=0)
  rollout  T env steps of Distillation.act + process_env_step on given observations, record (the one-launch step
           record, RSLRL_DISTILL_RECORD=1: taken at any number of envs) against copies (RSLRL_DISTILL_RECORD=0);
           reported per env step.  --parts rollout --envs 8192,16384,32768 locates the crossover behind
           algorithms/distillation.DISTILL_RECORD_MAX_ROWS
Each variant is warmed up once, then timed `--updates` times with device events; the median is reported with every
sample, and `default_rule` says whether the new path's median lies below the other variant's fastest run.

--tree PATH imports rsl_rl_amd from another checkout (the parent commit's, with its own built library): there both
update variants are the per-step loop, which is how `per_step` here is confirmed to be the parent's speed.

Usage:  python scripts/distill_default_probe.py [--envs 4096,65536] [--updates 5] [--students wide48,...]
                                                [--tree PATH] [--out profiles/distill_default_probe.json]
"""

import argparse
import json
import os
import sys

import numpy as np
import torch

T, OT, A, G, E = 24, 235, 12, 15, 1
TEACHER = [512, 256, 128]
STUDENTS = {
    "wide48": dict(obs=48, hidden=[512, 256, 128], gru=False),
    "wide45": dict(obs=45, hidden=[512, 256, 128], gru=False),
    "gru_wide": dict(obs=48, hidden=[512, 256, 128], gru=True),
    "gru_3x256": dict(obs=48, hidden=[256, 256, 256], gru=True),
}


def build(cfg, N, dev):
    from rsl_rl_amd.algorithms import Distillation
    from rsl_rl_amd.modules import StudentTeacher, StudentTeacherRecurrent
    from rsl_rl_amd.utils.tensordict import TensorDict

    torch.manual_seed(0)
    obs0 = TensorDict({"policy": torch.zeros(N, cfg["obs"], device=dev), "teacher": torch.zeros(N, OT, device=dev)},
                      batch_size=[N])
    groups = {"policy": ["policy"], "teacher": ["teacher"]}
    kw = dict(student_hidden_dims=cfg["hidden"], teacher_hidden_dims=TEACHER)
    if cfg["gru"]:
        pol = StudentTeacherRecurrent(obs0, groups, A, rnn_type="gru", rnn_hidden_dim=256, rnn_num_layers=1, **kw)
    else:
        pol = StudentTeacher(obs0, groups, A, **kw)
    pol.loaded_teacher = True
    alg = Distillation(pol, num_learning_epochs=E, gradient_length=G, max_grad_norm=1.0, device=str(dev))
    alg.policy.train()
    alg.init_storage("distillation", N, T, obs0, [A])
    return alg


def fill(alg, cfg, N, dev, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    st = alg.storage
    st.observations["policy"].copy_(torch.randn(T, N, cfg["obs"], device=dev, generator=g))
    st.observations["teacher"].copy_(torch.randn(T, N, OT, device=dev, generator=g))
    st.dones.copy_((torch.rand(T, N, 1, device=dev, generator=g) < 0.02).to(torch.uint8))
    with torch.inference_mode():
        for t in range(T):
            st.privileged_actions[t].copy_(3.0 * alg.policy.evaluate({"teacher": st.observations["teacher"][t]}))
    st.step = T


def timed(fn):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    out = fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end), out


def summary(times, new, old, extra=None):
    res = {k: {"ms": float(np.median(v)), "ms_all": v} for k, v in times.items()}
    res["ratio_old_over_new"] = res[old]["ms"] / res[new]["ms"]
    res["default_rule"] = {"new_median": res[new]["ms"], "old_fastest": min(times[old]),
                           "new_is_default": res[new]["ms"] < min(times[old])}
    res.update(extra or {})
    return res


def probe_update(cfg, N, dev, updates):
    algs = {name: build(cfg, N, dev) for name in ("windows", "per_step")}
    times, losses, path = {k: [] for k in algs}, {}, {}
    for it in range(updates + 1):  # the first round warms every shape up
        for name, alg in algs.items():
            fill(alg, cfg, N, dev, seed=it)
            alg.last_hidden_states = None
            os.environ["RSLRL_DISTILL_FUSED"] = "0" if name == "per_step" else "1"
            path[name] = bool(alg._fused_recurrent_ok() if cfg["gru"] else alg._fused_ok())
            ms, loss = timed(alg.update)
            if it > 0:
                times[name].append(ms)
                losses[name] = loss["behavior"]
    os.environ.pop("RSLRL_DISTILL_FUSED", None)
    return summary(times, "windows", "per_step", {"loss": losses, "took_the_window_path": path})


def probe_rollout(cfg, N, dev, updates):
    from rsl_rl_amd.networks import fused_mlp
    from rsl_rl_amd.utils.tensordict import TensorDict

    alg = build(cfg, N, dev)
    g = torch.Generator(device=dev).manual_seed(1)
    obs = [TensorDict({"policy": torch.randn(N, cfg["obs"], device=dev, generator=g),
                       "teacher": torch.randn(N, OT, device=dev, generator=g)}, batch_size=[N]) for _ in range(T)]
    rew = torch.randn(N, device=dev, generator=g)
    dones = (torch.rand(N, device=dev, generator=g) < 0.02).long()

    def rollout():
        alg.storage.clear()
        with torch.inference_mode(), fused_mlp.frozen_weights():
            for t in range(T):
                alg.act(obs[t])
                alg.process_env_step(obs[t], rew, dones, {})

    times = {"record": [], "copies": []}
    for it in range(updates + 1):
        for name in times:
            os.environ["RSLRL_DISTILL_RECORD"] = "0" if name == "copies" else "1"  # (1: at any number of envs)
            ms, _ = timed(rollout)
            if it > 0:
                times[name].append(ms / T)
    os.environ.pop("RSLRL_DISTILL_RECORD", None)
    return summary(times, "record", "copies", {"unit": "ms per env step (act + process_env_step), T steps timed"})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", default="4096,65536")
    ap.add_argument("--updates", type=int, default=5)
    ap.add_argument("--students", default=",".join(STUDENTS))
    ap.add_argument("--parts", default="update,rollout", help="what to time: update, rollout or both")
    ap.add_argument("--tree", default=None, help="import rsl_rl_amd from this checkout instead of this script's")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.tree) if args.tree
                    else os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    if not torch.cuda.is_available():
        raise SystemExit("distill_default_probe: needs a ROCm GPU; a CPU run measures nothing")
    import rsl_rl_amd

    dev = torch.device("cuda:0")
    res = {"shape": {"T": T, "teacher_obs": OT, "teacher_hidden": TEACHER, "actions": A, "gradient_length": G,
                     "epochs": E, "students": {k: STUDENTS[k] for k in args.students.split(",")},
                     "device": torch.cuda.get_device_name(0), "package": os.path.dirname(rsl_rl_amd.__file__)
                     if args.tree else "this tree"}}
    for N in [int(x) for x in args.envs.split(",")]:
        for name in args.students.split(","):
            r = {}
            if "update" in args.parts:
                r["update"] = probe_update(STUDENTS[name], N, dev, args.updates)
            if "rollout" in args.parts:
                r["rollout_step"] = probe_rollout(STUDENTS[name], N, dev, args.updates)
            res.setdefault(f"envs_{N}", {})[name] = r
            print(N, name, json.dumps(r), flush=True)
            torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
