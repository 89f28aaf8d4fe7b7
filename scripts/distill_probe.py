"""Cost of one Distillation.update() on the synthetic env's shapes extended with a teacher group (student obs 48,
teacher obs 64, 12 actions, 3 x 256 ELU, T 24, gradient_length 15, one epoch: one optimizer step over 15 * N rows and
9 trailing steps), at N = 4096 and N = 65536.

Not a test.  For each N, on one box and in one process, alternating so that every variant sees the same clocks:
  windows    the window-batched update (one forward / loss launch / backward per optimizer step, one read-back)
  per_step   RSLRL_DISTILL_FUSED=0: the reference's loop structure on the fused MLP + kernels.bc_loss behind autograd
  eager      a restatement of the reference's loop in plain torch on the same GPU (this script's own code:
             nn.Sequential, F.mse_loss, one .item() per step, autograd every 15 steps, torch's clip_grad_norm_ + Adam)
Each is warmed up once, then timed over `--updates` updates with device events around update(); the median is
reported with every sample.  The loss kernel is timed on its own at the window's shape (15 steps): event pairs
around single calls that rotate through enough operand sets to exceed the 256 MiB last-level cache, so every call
reads from HBM; reported against its 12 bytes per element at 8 TB/s.

Usage:  python scripts/distill_probe.py [--envs 4096,65536] [--updates 5] [--out profiles/distill_probe.json]
"""

import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rsl_rl_amd import kernels  # noqa: E402
from rsl_rl_amd.algorithms import Distillation  # noqa: E402
from rsl_rl_amd.modules import StudentTeacher  # noqa: E402
from rsl_rl_amd.utils.tensordict import TensorDict  # noqa: E402

T, OS, OT, A, HIDDEN, G, E = 24, 48, 64, 12, [256, 256, 256], 15, 1
HBM_PEAK = 8.0e12  # bytes / s: the HBM peak every roofline in DESIGN.md is stated against
LLC_BYTES = 256 << 20


def build(N, dev):
    torch.manual_seed(0)
    obs0 = TensorDict({"policy": torch.zeros(N, OS, device=dev), "teacher": torch.zeros(N, OT, device=dev)},
                      batch_size=[N])
    groups = {"policy": ["policy"], "teacher": ["teacher"]}
    pol = StudentTeacher(obs0, groups, A, student_hidden_dims=HIDDEN, teacher_hidden_dims=HIDDEN)
    pol.loaded_teacher = True
    alg = Distillation(pol, num_learning_epochs=E, gradient_length=G, max_grad_norm=1.0, device=str(dev))
    alg.init_storage("distillation", N, T, obs0, [A])
    return alg


def fill(alg, N, dev, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    st = alg.storage
    st.observations["policy"].copy_(torch.randn(T, N, OS, device=dev, generator=g))
    st.observations["teacher"].copy_(torch.randn(T, N, OT, device=dev, generator=g))
    with torch.inference_mode():
        for t in range(T):
            st.privileged_actions[t].copy_(3.0 * alg.policy.evaluate({"teacher": st.observations["teacher"][t]}))
    st.step = T


class EagerDistillation:
    """The reference's update loop (one small forward, an mse_loss and an .item() per stored step; autograd through
    the chained graphs every G steps; clip + Adam) in plain torch, on a copy of the student."""

    def __init__(self, alg, dev):
        src = [m for m in alg.policy.student]
        layers = []
        for m in src:
            if isinstance(m, nn.Linear):
                lin = nn.Linear(m.in_features, m.out_features).to(dev)
                lin.load_state_dict(m.state_dict())
                layers.append(lin)
            else:
                layers.append(nn.ELU())
        self.student = nn.Sequential(*layers)
        self.optimizer = torch.optim.Adam(self.student.parameters(), lr=1e-3)
        self.storage = alg.storage

    def update(self):
        mean, loss, cnt = 0.0, 0, 0
        st = self.storage
        for _ in range(E):
            for t in range(T):
                actions = self.student(st.observations["policy"][t])
                behavior_loss = F.mse_loss(actions, st.privileged_actions[t])
                loss = loss + behavior_loss
                mean += behavior_loss.item()
                cnt += 1
                if cnt % G == 0:
                    self.optimizer.zero_grad()
                    loss.backward()
                    nn.utils.clip_grad_norm_(self.student.parameters(), 1.0)
                    self.optimizer.step()
                    loss = 0
        return {"behavior": mean / cnt}


def timed(fn):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    out = fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end), out


def probe_updates(N, dev, updates):
    variants = {}
    for name in ("windows", "per_step"):
        alg = build(N, dev)
        variants[name] = (alg, alg.update)
    eager_src = build(N, dev)
    variants["eager"] = (eager_src, EagerDistillation(eager_src, dev).update)
    times = {k: [] for k in variants}
    losses = {}
    for it in range(updates + 1):  # the first round warms every shape up
        for name, (alg, update) in variants.items():
            fill(alg, N, dev, seed=it)
            os.environ["RSLRL_DISTILL_FUSED"] = "0" if name == "per_step" else "1"
            ms, loss = timed(update)
            alg.storage.clear()
            if it > 0:
                times[name].append(ms)
                losses[name] = loss
    os.environ.pop("RSLRL_DISTILL_FUSED", None)
    return {k: {"ms_per_update": float(np.median(v)), "ms_all": v, "loss": losses[k]} for k, v in times.items()}


def probe_kernel(N, dev, calls=40):
    rows = G * N
    per_set = 12 * rows * A
    nsets = max(2, -(-2 * LLC_BYTES // per_set))
    sets = [(torch.randn(rows, A, device=dev), torch.randn(rows, A, device=dev), torch.empty(rows, A, device=dev))
            for _ in range(nsets)]
    out = torch.empty(G, device=dev)
    res = {}
    for loss in ("mse", "huber"):
        for i in range(nsets):  # warm-up: code object, workspace, every operand set touched once
            kernels.bc_loss(sets[i][0], sets[i][1], N, loss, out, sets[i][2])
        t = []
        for i in range(calls):
            p, tg, g = sets[i % nsets]
            t.append(timed(lambda: kernels.bc_loss(p, tg, N, loss, out, g))[0])
        us = 1e3 * float(np.median(t))
        res[loss] = {"call_us": us, "call_us_min": 1e3 * min(t), "bytes": per_set, "operand_sets": nsets,
                     "floor_us_at_8TBs": per_set / HBM_PEAK * 1e6, "share_of_hbm_peak": per_set / HBM_PEAK * 1e6 / us}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", default="4096,65536")
    ap.add_argument("--updates", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("distill_probe: needs a ROCm GPU; a CPU run measures nothing")
    dev = torch.device("cuda:0")
    res = {"shape": {"T": T, "student_obs": OS, "teacher_obs": OT, "actions": A, "hidden": HIDDEN,
                     "gradient_length": G, "epochs": E, "device": torch.cuda.get_device_name(0)}}
    for N in [int(x) for x in args.envs.split(",")]:
        r = {"update": probe_updates(N, dev, args.updates), "bc_loss_window": probe_kernel(N, dev)}
        res[f"envs_{N}"] = r
        print(N, json.dumps(r), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
