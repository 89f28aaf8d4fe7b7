"""Generate the recurrent distillation fixtures under tests/golden/ by running the REFERENCE's Distillation.update()
on CPU with StudentTeacherRecurrent (rsl_rl/algorithms/distillation.py:105-151,
rsl_rl/modules/student_teacher_recurrent.py, rsl_rl/networks/memory.py).

Test infrastructure only, like make_golden_distillation.py: it reuses make_golden's import shims and
distill_fixtures.storage_obs without editing either, runs where a reference checkout exists and writes
tests/golden/drec_<case>*.npz plus tests/golden/golden_distillation_recurrent.json in the update_* family's layout
(r0/init/, r0/final/, per-rank lr_trace and loss_dict), so tests/update_fixtures.check_update applies;
tests/drec_fixtures.py rebuilds the storage.  An array above ~400 KB is stored as row chunks `<key>@<i>` and the
files are packed below 1 MiB each (drec_fixtures.Arrays joins them).

Stored per case: the initial and final parameters of memory_s and student (with std / log_std and the student
normaliser's buffers); the teacher's actions (TARGET_SCALE x the teacher's output, a recurrent teacher stepped through the
rollout from the supplied state with the dones' resets) and the dones; the supplied last_hidden_states; all E * T
step losses; one lr per optimizer step; the first step's gradient per tensor (memory and MLP) before clipping, the
norm clip_grad_norm_ saw (the MLP's) and the norm over memory and MLP; get_hidden_states() of both memories after
the update.

Cases (dones hand-placed, see place_dones)
  a  LSTM H 32, one layer, feed-forward teacher; T 8, N 64, O 16 / 24, A 4, MLPs [64, 64]; E 2, G 3: five steps, one
     window across the epoch boundary, one trailing step; MSE, clip 1.0, last_hidden_states None
  b  GRU H 32, two layers, teacher_recurrent; log std, student normalisation with non-trivial buffers; Huber, no clip;
     seeded non-zero last_hidden_states for both memories
  c  LSTM H 256, one layer; N 128, O 48 / 64, A 4, MLPs [64, 64]; T 8, E 2, G 3, MSE, clip 1.0; seeded non-zero
     last_hidden_states; the student's first layer x 4 (see student_in_gain); with the reference's own one-ulp sensitivity envelope, as distill_c stores it

Usage:  python tests/golden/make_golden_distillation_recurrent.py --reference PATH_TO_RSL_RL_CHECKOUT [--cases a,b]
"""

from __future__ import annotations

import argparse
import hashlib
import json
import os
import sys

import numpy as np
import torch

import make_golden as G

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from distill_fixtures import storage_obs  # noqa: E402

TARGET_SCALE = 10.0
CHUNK_BYTES = 400 << 10
FILE_BYTES = 900 << 10
BASE = dict(T=8, O_student=16, O_teacher=24, A=4, hidden=[64, 64], E=2, G=3)
CASES = {
    "a": dict(BASE, N=64, rnn_type="lstm", rnn_hidden_dim=32, rnn_num_layers=1, teacher_recurrent=False,
              loss_type="mse", max_grad_norm=1.0, policy_kw={}, seed=411, seeded_state=False),
    "b": dict(BASE, N=64, rnn_type="gru", rnn_hidden_dim=32, rnn_num_layers=2, teacher_recurrent=True,
              loss_type="huber", max_grad_norm=None, seed=413, seeded_state=True,
              policy_kw={"noise_std_type": "log", "student_obs_normalization": True}),
    "c": dict(BASE, N=128, O_student=48, O_teacher=64, rnn_type="lstm", rnn_hidden_dim=256, rnn_num_layers=1,
              teacher_recurrent=False, loss_type="mse", max_grad_norm=1.0, policy_kw={}, seed=417, seeded_state=True,
              sensitivity=True, student_in_gain=4.0),
}
PROBES = ("par0", "par1", "tgt0")


def import_distillation(ref_path):
    G.import_reference(ref_path)
    from rsl_rl.algorithms import Distillation
    from rsl_rl.modules import StudentTeacherRecurrent

    return Distillation, StudentTeacherRecurrent


def windows(T, E, G_):
    seq = [t for _ in range(E) for t in range(T)]
    return [seq[i:i + G_] for i in range(0, len(seq), G_)]


def place_dones(T, N, E, G_):
    """Hand-placed dones [T, N] (uint8) and the assertions that make them meaningful: about 10 % overall; env 0 never
    resets; in every window an env that resets inside it (not on its last step); a reset on a window's last step; a
    reset at t = T - 1; env 3 resets on two consecutive steps."""
    d = np.zeros((T, N), dtype=np.uint8)
    for t in range(T):
        for n in range(N):
            if (n + 3 * t) % 10 == 5:
                d[t, n] = 1
    d[:, 0] = 0          # never resets
    d[G_ - 1, 1] = 1     # the first window's last step
    d[T - 1, 2] = 1      # the rollout's last step
    d[3, 3] = d[4, 3] = 1  # consecutive steps
    frac = float(d.mean())
    assert 0.07 <= frac <= 0.14, frac
    assert not d[:, 0].any()
    assert d[T - 1].any() and d[3, 3] and d[4, 3]
    for w in windows(T, E, G_):
        if len(w) < G_:
            continue
        inside = [t for t in w[:-1]]
        assert any(d[t].any() for t in inside), ("no reset inside window", w)
        never = [n for n in range(N) if not any(d[t, n] for t in w)]
        assert never, ("every env resets in window", w)
    assert any(d[w[-1]].any() for w in windows(T, E, G_) if len(w) == G_)
    return d


def _ulp_jitter(t, seed):
    g = torch.Generator().manual_seed(seed)
    up = torch.nextafter(t, torch.full_like(t, float("inf")))
    down = torch.nextafter(t, torch.full_like(t, float("-inf")))
    return torch.where(torch.rand(t.shape, generator=g) < 0.5, up, down)


def _states(x):
    """A memory's hidden states as a list of arrays (LSTM: h, c; GRU: h; None: empty)."""
    if x is None:
        return []
    return [G.f32(s) for s in (x if isinstance(x, tuple) else (x,))]


def _seeded_state(kind, L, N, H, seed):
    g = torch.Generator().manual_seed(seed)
    mk = lambda: 0.5 * torch.randn(L, N, H, generator=g)  # noqa: E731
    return (mk(), mk()) if kind == "lstm" else mk()


def _clone(x):
    if x is None:
        return None
    return tuple(s.clone() for s in x) if isinstance(x, tuple) else x.clone()


def trained(name):
    return name.startswith(("memory_s.", "student."))


def run_case(Distillation, Policy, cfg, probe=None):
    T, N, A, Os, Ot = cfg["T"], cfg["N"], cfg["A"], cfg["O_student"], cfg["O_teacher"]
    seed, H, L = cfg["seed"], cfg["rnn_hidden_dim"], cfg["rnn_num_layers"]
    torch.manual_seed(seed)
    obs0 = {"policy": torch.zeros(N, Os), "teacher": torch.zeros(N, Ot)}
    groups = {"policy": ["policy"], "teacher": ["teacher"]}
    pol = Policy(obs0, groups, A, student_hidden_dims=cfg["hidden"], teacher_hidden_dims=cfg["hidden"],
                 rnn_type=cfg["rnn_type"], rnn_hidden_dim=H, rnn_num_layers=L,
                 teacher_recurrent=cfg["teacher_recurrent"], **cfg["policy_kw"])
    pol.loaded_teacher = True
    pol.train()
    if cfg.get("student_in_gain"):
        # a larger first student layer: more of the gradient reaches the memory, so that the norm over memory and
        # MLP is told apart from the MLP's (the assertion on norms["full"] below)
        with torch.no_grad():
            pol.student[0].weight.mul_(cfg["student_in_gain"])
    if cfg["policy_kw"].get("student_obs_normalization"):
        nrng = np.random.default_rng(seed * 100 + 50)
        for _ in range(2):  # non-trivial running statistics, as a rollout's update_normalization leaves them
            x = nrng.standard_normal((N, Os), dtype=np.float32) * 1.5 + 0.25
            pol.update_normalization({"policy": torch.from_numpy(x), "teacher": obs0["teacher"]})
    alg = Distillation(pol, num_learning_epochs=cfg["E"], gradient_length=cfg["G"], learning_rate=1e-3,
                       max_grad_norm=cfg["max_grad_norm"], loss_type=cfg["loss_type"], device="cpu")
    init = {k: (v.numpy().copy() if v.dtype == torch.int64 else G.f32(v)) for k, v in pol.state_dict().items()
            if not k.startswith(("teacher", "memory_t"))}
    obs_seed = seed * 100
    obs = storage_obs(obs_seed, T, N, Os, Ot)
    dones = place_dones(T, N, cfg["E"], cfg["G"])
    dones_t = torch.from_numpy(dones)

    last = None
    if cfg["seeded_state"]:
        last = (_seeded_state(cfg["rnn_type"], L, N, H, seed * 10 + 1),
                _seeded_state(cfg["rnn_type"], L, N, H, seed * 10 + 2) if cfg["teacher_recurrent"] else None)

    # the teacher's actions: the rollout's evaluate() per step, a recurrent teacher from the supplied state with the
    # dones' resets in between
    with torch.no_grad():
        pol.reset(hidden_states=(None, _clone(last[1])) if last is not None else None)
        priv = torch.empty(T, N, A)
        for t in range(T):
            priv[t] = TARGET_SCALE * pol.evaluate({"teacher": torch.from_numpy(obs["teacher"][t])})
            if cfg["teacher_recurrent"]:
                pol.memory_t.reset(dones_t[t])
        pol.reset()
    if probe is not None and probe.startswith("par"):
        with torch.no_grad():
            for n_, p in pol.named_parameters():
                if trained(n_):
                    p.copy_(_ulp_jitter(p, int(probe[3:]) * 1000 + 7))
    if probe is not None and probe.startswith("tgt"):
        priv = _ulp_jitter(priv, int(probe[3:]) * 1000 + 11)

    alg.init_storage("distillation", N, T, obs0, [A])
    st = alg.storage
    st.observations["policy"].copy_(torch.from_numpy(obs["policy"]))
    st.observations["teacher"].copy_(torch.from_numpy(obs["teacher"]))
    st.privileged_actions.copy_(priv)
    st.dones.copy_(dones_t.reshape(T, N, 1))
    st.step = T
    alg.last_hidden_states = None if last is None else (_clone(last[0]), _clone(last[1]))

    step_losses, lr_trace, grad0, norms = [], [], {}, {}
    loss_fn = alg.loss_fn
    names = [n_ for n_, _ in pol.named_parameters() if trained(n_)]
    params = dict(pol.named_parameters())

    def rec_loss(a, b):
        r = loss_fn(a, b)
        step_losses.append(r.item())
        return r

    def grab():
        if not grad0:
            for n_ in names:
                grad0[n_] = G.f32(params[n_].grad)
            sq = lambda pre: sum(float(params[n_].grad.double().pow(2).sum()) for n_ in names  # noqa: E731
                                 if n_.startswith(pre))
            norms["mlp"] = sq("student.") ** 0.5
            norms["memory"] = sq("memory_s.") ** 0.5
            norms["full"] = (sq("student.") + sq("memory_s.")) ** 0.5

    clip, step = torch.nn.utils.clip_grad_norm_, alg.optimizer.step

    def rec_clip(ps, *a, **k):
        ps = list(ps)
        assert [id(p) for p in ps] == [id(p) for p in pol.student.parameters()], "the clip spans the student MLP"
        grab()
        r = clip(ps, *a, **k)
        norms.setdefault("clip_saw", float(r))
        return r

    def rec_step(*a, **k):
        grab()
        lr_trace.append(float(alg.optimizer.param_groups[0]["lr"]))
        return step(*a, **k)

    alg.loss_fn, alg.optimizer.step = rec_loss, rec_step
    torch.nn.utils.clip_grad_norm_ = rec_clip
    try:
        loss_dict = alg.update()
    finally:
        torch.nn.utils.clip_grad_norm_ = clip
    assert len(step_losses) == cfg["E"] * T
    assert len(lr_trace) == (cfg["E"] * T) // cfg["G"]
    assert norms["memory"] > 0.0, "the memory's gradient is zero"
    if cfg["max_grad_norm"]:
        assert norms["mlp"] > cfg["max_grad_norm"], ("clip case: the MLP's gradient is not clipped", norms)
        assert abs(norms["clip_saw"] - norms["mlp"]) <= 1e-4 * norms["mlp"], norms
    if cfg["rnn_hidden_dim"] >= 256:
        assert norms["full"] > 1.01 * norms["mlp"], ("clipping the wrong set would pass", norms)
    assert all(p.grad is None for n_, p in pol.named_parameters() if not trained(n_))

    hs, ht = pol.get_hidden_states()
    arrays = {f"init/{k}": v for k, v in init.items()}
    arrays.update({f"final/{k}": G.f32(v) for k, v in pol.state_dict().items() if trained(k)})
    arrays.update({f"grad_mb0/{k}": v for k, v in grad0.items()})
    arrays["privileged_actions"] = G.f32(priv)
    arrays["dones"] = dones
    arrays["step_losses"] = np.asarray(step_losses, dtype=np.float64)
    arrays["obs_sha256"] = np.frombuffer(hashlib.sha256(obs["policy"].tobytes()).digest(), dtype=np.uint8)
    if last is not None:
        for tag, x in (("s", last[0]), ("t", last[1])):
            for i, s in enumerate(_states(x)):
                arrays[f"last_hidden/{tag}{i}"] = s
    for tag, x in (("s", hs), ("t", ht)):
        for i, s in enumerate(_states(x)):
            arrays[f"hidden_final/{tag}{i}"] = s
    meta = {"loss_dict": loss_dict, "lr_trace": lr_trace, "final_lr": alg.learning_rate, "obs_seed": obs_seed,
            "num_steps": len(lr_trace), "grad_norms": norms, "done_fraction": float(dones.mean())}
    return arrays, meta


def pack(name, arrays):
    """Row chunks of the large arrays, packed into files below 1 MiB."""
    items = []
    for k, v in arrays.items():
        if v.nbytes > CHUNK_BYTES:
            parts = np.array_split(v, -(-v.nbytes // CHUNK_BYTES), axis=0)
            items += [(f"{k}@{i}", np.ascontiguousarray(p)) for i, p in enumerate(parts)]
        else:
            items.append((k, v))
    files, cur, size = [], {}, 0
    for k, v in items:
        if cur and size + v.nbytes > FILE_BYTES:
            files.append(cur)
            cur, size = {}, 0
        cur[k] = v
        size += v.nbytes
    files.append(cur)
    out = []
    for i, f in enumerate(files):
        fname = f"drec_{name}.npz" if i == 0 else f"drec_{name}_{i}.npz"
        path = os.path.join(HERE, fname)
        np.savez_compressed(path, **f)
        assert os.path.getsize(path) < (1 << 20), (fname, os.path.getsize(path))
        out.append(fname)
    return out


def make_case(ref_path, name):
    cfg = CASES[name]
    Distillation, Policy = import_distillation(ref_path)
    a, m = run_case(Distillation, Policy, cfg)
    arrays = {f"r0/{k}": v for k, v in a.items()}
    sens = {}
    if cfg.get("sensitivity"):
        for probe in PROBES:
            ulp, _ = run_case(Distillation, Policy, cfg, probe=probe)
            for k in [k for k in arrays if k.startswith("r0/final/")]:
                pname = k[len("r0/final/"):]
                ref = arrays[k].astype(np.float64)
                moved = np.linalg.norm(ref - arrays["r0/init/" + pname].astype(np.float64))
                d = np.linalg.norm(ulp["final/" + pname].astype(np.float64) - ref)
                sens[pname] = max(sens.get(pname, 0.0), float(d / moved) if moved else float(d))
            for k in [k for k in arrays if k.startswith("r0/hidden_final/")]:
                d = np.abs(ulp[k[3:]].astype(np.float64) - arrays[k].astype(np.float64)).max()
                sens[k[3:]] = max(sens.get(k[3:], 0.0), float(d))
    files = pack(name, arrays)
    meta = {k: cfg[k] for k in ("T", "N", "O_student", "O_teacher", "A", "hidden", "E", "G", "loss_type",
                                "max_grad_norm", "policy_kw", "seed", "rnn_type", "rnn_hidden_dim", "rnn_num_layers",
                                "teacher_recurrent", "seeded_state")}
    meta.update({"world": 1, "ranks": [m], "shared_params": True, "files": files, "ulp_sensitivity": sens,
                 "ulp_probes": list(PROBES) if sens else [], "target_scale": TARGET_SCALE, "learning_rate": 1e-3,
                 "init_keys": [k[len("r0/init/"):] for k in arrays if k.startswith("r0/init/")]})
    print(f"case {name}: steps {m['num_steps']} norms {m['grad_norms']} loss {m['loss_dict']} "
          f"dones {m['done_fraction']:.3f} files {files}", flush=True)
    return meta


def state_dict_keys(Policy):
    """The reference's state_dict key and parameter orders: teacher_recurrent on and off, both std types (with both
    normalisers; a recurrent teacher's normaliser is sized rnn_hidden_dim, the reference's construction)."""
    obs0 = {"policy": torch.zeros(2, 16), "teacher": torch.zeros(2, 24)}
    groups = {"policy": ["policy"], "teacher": ["teacher"]}
    out = {}
    for std_type in ("scalar", "log"):
        for rec in (False, True):
            pol = Policy(obs0, groups, 4, student_hidden_dims=[64, 64], teacher_hidden_dims=[64, 64],
                         noise_std_type=std_type, student_obs_normalization=True, teacher_obs_normalization=True,
                         rnn_hidden_dim=32, teacher_recurrent=rec)
            sd = pol.state_dict()
            out[f"{std_type}_{'recurrent' if rec else 'plain'}"] = {
                "state_dict": list(sd.keys()), "parameters": [n for n, _ in pol.named_parameters()],
                "shapes": {k: list(v.shape) for k, v in sd.items()}}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="the rsl_rl 3.1.0 checkout (the directory holding rsl_rl/)")
    ap.add_argument("--cases", default=None, help="comma-separated case names (default: all)")
    args = ap.parse_args()
    torch.set_num_threads(1)
    path = os.path.join(HERE, "golden_distillation_recurrent.json")
    meta = {}
    if args.cases and os.path.exists(path):
        with open(path) as f:
            meta = json.load(f)
    for name in CASES:
        if args.cases is None or name in args.cases.split(","):
            meta[name] = make_case(args.reference, name)
    _, Policy = import_distillation(args.reference)
    meta["state_dict_keys"] = state_dict_keys(Policy)
    with open(path, "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
