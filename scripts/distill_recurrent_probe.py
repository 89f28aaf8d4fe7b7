"""Cost of one recurrent Distillation.update() and of one rollout step with a StudentTeacherRecurrent (student obs 48,
teacher obs 64, 12 actions, one LSTM layer of 256 in front of 3 x 256 ELU, T 24, gradient_length 15, one epoch: one
optimizer step through 15 chained steps, 9 trailing steps), at N = 4096 and N = 65536.

Not a test.  For each N, on one box and in one process, alternating so that every variant sees the same clocks:
  windows    Distillation.update() window-batched: per optimizer step G lstm_cell_train launches, one fused-MLP
             forward / loss launch / backward over the window's rows, G lstm_cell_bwd launches, the gate blocks'
             weight gradients, the subset clip + Adam in two launches; one read-back at the end
  per_step   RSLRL_DISTILL_FUSED=0: the reference's loop on nn.LSTM under autograd, the fused MLP path and
             kernels.bc_loss behind it, the same optimizer step and read-back
  eager      a restatement of the reference's loop in plain torch on the same GPU (this script's own code: nn.LSTM,
             nn.Sequential, F.mse_loss, one .item() per step, indexed resets, torch's clip_grad_norm_ over the MLP + Adam)
Each is warmed up once, then timed over `--updates` updates with device events around update(); the median is
reported with every sample (the protocol of DESIGN §14).  The rollout step (Distillation.act + process_env_step
under inference_mode, a recurrent teacher) is timed the same way with the fused LSTM cell and with RSLRL_LSTM_CELL=0.
The two training kernels are timed on their own at N rows: an event pair around each of 20 single calls, medians; the
reverse step's x6 MFMA work (6 bf16 products of 2 * N * 1024 * 256 flop) is stated against the 2.5 PFLOP/s dense bf16
peak the other rooflines of DESIGN.md use.

Usage:  python scripts/distill_recurrent_probe.py [--envs 4096,65536] [--updates 5] [--out FILE.json]
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
from rsl_rl_amd.modules import StudentTeacherRecurrent  # noqa: E402
from rsl_rl_amd.networks import fused_mlp  # noqa: E402
from rsl_rl_amd.utils.tensordict import TensorDict  # noqa: E402

T, OS, OT, A, HIDDEN, H, G, E = 24, 48, 64, 12, [256, 256, 256], 256, 15, 1


def build(N, dev, teacher_recurrent=False):
    torch.manual_seed(0)
    obs0 = TensorDict({"policy": torch.zeros(N, OS, device=dev), "teacher": torch.zeros(N, OT, device=dev)},
                      batch_size=[N])
    groups = {"policy": ["policy"], "teacher": ["teacher"]}
    pol = StudentTeacherRecurrent(obs0, groups, A, student_hidden_dims=HIDDEN, teacher_hidden_dims=HIDDEN,
                                  rnn_hidden_dim=H, teacher_recurrent=teacher_recurrent)
    pol.loaded_teacher = True
    pol.train()
    alg = Distillation(pol, num_learning_epochs=E, gradient_length=G, max_grad_norm=1.0, device=str(dev))
    alg.init_storage("distillation", N, T, obs0, [A])
    return alg


def fill(alg, N, dev, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    st = alg.storage
    st.observations["policy"].copy_(torch.randn(T, N, OS, device=dev, generator=g))
    st.privileged_actions.copy_(torch.randn(T, N, A, device=dev, generator=g))
    st.dones.copy_((torch.rand(T, N, 1, device=dev, generator=g) < 0.02).to(torch.uint8))
    st.step = T


class EagerRecurrentDistillation:
    """The reference's recurrent update loop in plain torch, on copies of the student's memory and MLP."""

    def __init__(self, alg, dev):
        pol = alg.policy
        self.rnn = nn.LSTM(OS, H, 1).to(dev)
        self.rnn.load_state_dict(pol.memory_s.rnn.state_dict())
        layers = []
        for m in pol.student:
            if isinstance(m, nn.Linear):
                lin = nn.Linear(m.in_features, m.out_features).to(dev)
                lin.load_state_dict(m.state_dict())
                layers.append(lin)
            else:
                layers.append(nn.ELU())
        self.student = nn.Sequential(*layers)
        self.optimizer = torch.optim.Adam(list(self.rnn.parameters()) + list(self.student.parameters()), lr=1e-3)
        self.storage = alg.storage
        self.last = None

    def update(self):
        mean, loss, cnt = 0.0, 0, 0
        st = self.storage
        state = None
        for _ in range(E):
            state = None if self.last is None else tuple(s.detach() for s in self.last)
            for t in range(T):
                out, state = self.rnn(st.observations["policy"][t].unsqueeze(0), state)
                behavior_loss = F.mse_loss(self.student(out.squeeze(0)), st.privileged_actions[t])
                loss = loss + behavior_loss
                mean += behavior_loss.item()
                cnt += 1
                if cnt % G == 0:
                    self.optimizer.zero_grad()
                    loss.backward()
                    nn.utils.clip_grad_norm_(self.student.parameters(), 1.0)
                    self.optimizer.step()
                    state = tuple(s.detach() for s in state)
                    loss = 0
                done = st.dones[t].view(-1) == 1
                for s in state:  # the reference's indexed reset and detach of the done rows
                    s[..., done, :] = 0.0
                    s[..., done, :] = s[..., done, :].detach()
        self.last = tuple(s.detach() for s in state)
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
    variants["eager"] = (eager_src, EagerRecurrentDistillation(eager_src, dev).update)
    times = {k: [] for k in variants}
    losses = {}
    for it in range(updates + 1):  # the first round warms every shape up
        for name, (a, update) in variants.items():
            fill(a, N, dev, seed=it)
            os.environ["RSLRL_DISTILL_FUSED"] = "0" if name == "per_step" else "1"
            ms, loss = timed(update)
            a.storage.clear()
            if it > 0:
                times[name].append(ms)
                losses[name] = loss
    os.environ.pop("RSLRL_DISTILL_FUSED", None)
    return {k: {"ms_per_update": float(np.median(v)), "ms_all": v, "loss": losses[k]} for k, v in times.items()}


BF16_PEAK = 2.5e15  # flop / s, dense bf16 MFMA


def probe_kernels(N, dev, calls=20):
    g = torch.Generator(device=dev).manual_seed(3)
    rn = lambda *s: torch.randn(*s, device=dev, generator=g)  # noqa: E731
    w_ih, w_hh, b = rn(4 * H, OS) / 16, rn(4 * H, H) / 16, rn(4 * H) / 16
    image, whh_t = kernels.lstm_image(w_ih, w_hh), kernels.lstm_whh_t_image(w_hh)
    x, h, c = rn(N, OS), rn(N, H), rn(N, H)
    reset = (torch.rand(N, device=dev, generator=g) < 0.02).to(torch.uint8)
    hout, cout, dcp = (torch.empty(N, H, device=dev) for _ in range(3))
    gates, dg = torch.empty(4, 2, N, H, device=dev), torch.empty(4, 2, N, H, device=dev)
    dg[:, 1].normal_(generator=g)
    dh = rn(N, H)
    fwd = lambda: kernels.lstm_cell_train(x, (h, c), image, b, b, reset, hout, cout, gates[:, 0])  # noqa: E731
    bwd = lambda: kernels.lstm_cell_bwd(dh, gates[:, 0], cout, c, reset, dg[:, 1], h, reset, whh_t, dg[:, 0],  # noqa: E731
                                        dcp)
    res = {}
    for name, fn, flop in (("lstm_cell_train", fwd, 12 * N * (OS + H) * 4 * H), ("lstm_cell_bwd", bwd, 12 * N * 4 * H * H)):
        fn()
        t = [timed(fn)[0] for _ in range(calls)]
        us = 1e3 * float(np.median(t))
        res[name] = {"call_us": us, "call_us_min": 1e3 * min(t), "x6_mfma_flop": flop,
                     "share_of_bf16_peak": flop / BF16_PEAK / (us * 1e-6)}
    return res


def probe_rollout_step(N, dev, steps=20):
    alg = build(N, dev, teacher_recurrent=True)
    g = torch.Generator(device=dev).manual_seed(1)
    obs = {"policy": torch.randn(N, OS, device=dev, generator=g), "teacher": torch.randn(N, OT, device=dev, generator=g)}
    rew = torch.zeros(N, device=dev)
    dones = (torch.rand(N, device=dev, generator=g) < 0.02).long()

    def step():
        alg.act(obs)
        alg.process_env_step(obs, rew, dones, {})
        alg.storage.clear()

    res = {}
    for it in range(2):  # alternate the two modes, the first round warms up
        for name, flag in (("fused_cell", "1"), ("rnn_library", "0")):
            os.environ["RSLRL_LSTM_CELL"] = flag
            with torch.inference_mode(), fused_mlp.frozen_weights():
                alg.policy.reset()
                step()
                t = [timed(step)[0] for _ in range(steps)]
            if it:
                res[name] = {"step_us": 1e3 * float(np.median(t)), "step_us_min": 1e3 * min(t)}
    os.environ.pop("RSLRL_LSTM_CELL", None)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", default="4096,65536")
    ap.add_argument("--updates", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("distill_recurrent_probe: needs a ROCm GPU; a CPU run measures nothing")
    dev = torch.device("cuda:0")
    res = {"shape": {"T": T, "student_obs": OS, "teacher_obs": OT, "actions": A, "hidden": HIDDEN, "lstm": H,
                     "gradient_length": G, "epochs": E, "device": torch.cuda.get_device_name(0)}}
    for N in [int(x) for x in args.envs.split(",")]:
        r = {"update": probe_updates(N, dev, args.updates), "rollout_step": probe_rollout_step(N, dev),
             "kernels": probe_kernels(N, dev)}
        res[f"envs_{N}"] = r
        print(N, json.dumps(r), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
