"""Cost of the distillation head (rslrl_bc_head_fwd_bwd): the BC loss inside the student's last launch.

Not a test.  Two measurements, each alternating its two variants in one process so that both see the same clocks:

  update   one Distillation.update() -- 12 actions, T 24, gradient_length 15, one epoch -- at N envs for the students
           [512, 256, 128] and 3 x 256 at obs 48 and a GRU 256 in front of 3 x 256: `head` (the last launch of every
           optimizer step runs the loss and the output layer's backward) against `off` (RSLRL_BC_HEAD=0, here the module
           flag held off around update(): linear_fwd_out, the loss kernel, linear_dgrad_elu_wgrad).  One warm-up round,
           then the median of `--updates` updates with device events around update(), every sample kept.  The head is
           the default where its median is below the other variant's fastest run.
  launch   the head's launch alone at 15 x N rows (K = 256, N = 256 and 128 columns) against the three launches it
           replaces -- `--iters` calls per event pair, the median of `--rounds` rounds.

Usage:  python scripts/bc_head_probe.py [--envs 4096,65536] [--updates 5] [--out FILE.json]
"""

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rsl_rl_amd import _lib, kernels  # noqa: E402
from rsl_rl_amd.algorithms import distillation  # noqa: E402
from rsl_rl_amd.networks import fused_mlp  # noqa: E402

T, A, G, E, OT = 24, 12, 15, 1, 64
STUDENTS = {
    "512-256-128": dict(obs=48, hidden=[512, 256, 128], gru=False),
    "3x256": dict(obs=48, hidden=[256, 256, 256], gru=False),
    "gru256+3x256": dict(obs=48, hidden=[256, 256, 256], gru=True),
}


def build(cfg, N, dev):
    from rsl_rl_amd.modules import StudentTeacher, StudentTeacherRecurrent
    from rsl_rl_amd.utils.tensordict import TensorDict

    torch.manual_seed(0)
    obs0 = TensorDict({"policy": torch.zeros(N, cfg["obs"], device=dev), "teacher": torch.zeros(N, OT, device=dev)},
                      batch_size=[N])
    groups = {"policy": ["policy"], "teacher": ["teacher"]}
    kw = dict(student_hidden_dims=cfg["hidden"], teacher_hidden_dims=[256, 256, 256])
    if cfg["gru"]:
        pol = StudentTeacherRecurrent(obs0, groups, A, rnn_type="gru", rnn_hidden_dim=256, rnn_num_layers=1, **kw)
    else:
        pol = StudentTeacher(obs0, groups, A, **kw)
    pol.loaded_teacher = True
    alg = distillation.Distillation(pol, num_learning_epochs=E, gradient_length=G, max_grad_norm=1.0, device=str(dev))
    alg.policy.train()
    alg.init_storage("distillation", N, T, obs0, [A])
    return alg


def fill(alg, cfg, N, dev, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    st = alg.storage
    st.observations["policy"].copy_(torch.randn(T, N, cfg["obs"], device=dev, generator=g))
    st.observations["teacher"].copy_(torch.randn(T, N, OT, device=dev, generator=g))
    st.dones.copy_((torch.rand(T, N, 1, device=dev, generator=g) < 0.02).to(torch.uint8))
    st.privileged_actions.copy_(torch.randn(T, N, A, device=dev, generator=g))
    st.step = T


def timed(fn):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    out = fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end), out


def probe_update(cfg, N, dev, updates):
    variants = {"head": build(cfg, N, dev), "off": build(cfg, N, dev)}
    times, used, losses = {k: [] for k in variants}, {}, {}
    knob = distillation._BC_HEAD
    try:
        for it in range(updates + 1):  # the first round warms every shape up
            for name, alg in variants.items():
                fill(alg, cfg, N, dev, seed=it)
                alg.last_hidden_states = None
                distillation._BC_HEAD = name == "head"
                before = fused_mlp.bc_head_launches
                ms, loss = timed(alg.update)
                used[name] = fused_mlp.bc_head_launches - before
                if it > 0:
                    times[name].append(ms)
                    losses[name] = loss
    finally:
        distillation._BC_HEAD = knob
    res = {k: {"ms_per_update": statistics.median(v), "ms_min": min(v), "ms_all": v,
               "bc_head_launches_per_update": used[k], "loss": losses[k]} for k, v in times.items()}
    res["head_is_default"] = res["head"]["ms_per_update"] < res["off"]["ms_min"]
    res["head_vs_off"] = res["head"]["ms_per_update"] / res["off"]["ms_per_update"]
    return res


def probe_launch(rps, N, dev, rounds, iters):
    K, M = 256, G * rps
    g = torch.Generator(device=dev).manual_seed(0)
    r = lambda *s: torch.randn(*s, device=dev, generator=g)  # noqa: E731
    x = torch.nn.functional.elu(r(M, K))
    w, b, wo, bo, target = r(N, K) / 16, r(N) * 0.1, r(A, N) / 16, r(A) * 0.1, r(M, A)
    img, out_img, img_t = fused_mlp.bimages([(w, False), (wo, False, _lib.BIMAGE_LAYOUT_OUT), (wo, True)])
    step, gbuf = torch.empty(G, device=dev), torch.empty(M, A, device=dev)
    head = fused_mlp.BCHead(target, rps, "mse", step)

    def fused():
        assert fused_mlp.bc_head_fwd_bwd(x, b, N, img, bo, out_img, img_t, head) is not None

    def separate():
        h, y = fused_mlp.linear_fwd_out_ex(x, b, N, img, _lib.ARITH_X6, None, bo, out_img, store_h=True)
        kernels.bc_loss(y, target, rps, "mse", step, grad_out=gbuf)
        fused_mlp.linear_dgrad_elu_wgrad(gbuf, wo, h, img_t, want_db_prev=False)

    fns = {"fused": fused, "separate": separate}
    res = {k: [] for k in fns}
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
    return {k: {"median_us": round(statistics.median(v), 2), "runs_us": [round(t, 2) for t in v]}
            for k, v in res.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", default="4096,65536")
    ap.add_argument("--updates", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bc_head_probe: needs a GPU")
    dev = torch.device("cuda:0")
    envs = [int(n) for n in args.envs.split(",")]
    out = {"device": torch.cuda.get_device_name(dev), "abi": _lib.lib().rslrl_abi_version(),
           "config": {"T": T, "actions": A, "gradient_length": G, "epochs": E, "updates": args.updates,
                      "rounds": args.rounds, "iters": args.iters, "students": STUDENTS},
           "update": {}, "launch": {}}
    for N in envs:
        for name, cfg in STUDENTS.items():
            out["update"][f"N={N},student={name}"] = probe_update(cfg, N, dev, args.updates)
            torch.cuda.empty_cache()
    for N in (256, 128):
        out["launch"][f"M={G * envs[0]},N={N}"] = probe_launch(envs[0], N, dev, args.rounds, args.iters)
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
