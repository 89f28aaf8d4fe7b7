"""Rebuild the recurrent distillation fixtures (tests/golden/make_golden_distillation_recurrent.py) on any device: the
observations are regenerated from the fixture's numpy seed (checked against the stored sha256); the teacher's actions,
the dones, the supplied last_hidden_states, the initial parameters of the student's memory and MLP and the reference's
results come from the fixture.  The layout is the update_* family's, so update_fixtures.check_update applies; the
first step's gradient is stored per tensor (`r0/grad_mb0/<name>`) and checked here."""

import hashlib
import json
import os

import numpy as np
import torch

from distill_fixtures import storage_obs

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")


def load_meta():
    with open(os.path.join(GOLDEN, "golden_distillation_recurrent.json")) as f:
        return json.load(f)


class Arrays:
    """The arrays of a case, whichever of its files holds them, with the row chunks `<key>@<i>` of a large array
    joined (np.load's `files` / [] interface)."""

    def __init__(self, paths):
        self._z = [np.load(p) for p in paths]
        self._where, self._chunks = {}, {}
        for z in self._z:
            for k in z.files:
                if "@" in k:
                    name, i = k.rsplit("@", 1)
                    self._chunks.setdefault(name, {})[int(i)] = (z, k)
                else:
                    self._where[k] = z
        self.files = list(self._where) + list(self._chunks)
        self._cache = {}

    def __getitem__(self, key):
        if key in self._where:
            return self._where[key][key]
        if key in self._chunks:
            if key not in self._cache:
                parts = self._chunks[key]
                assert sorted(parts) == list(range(len(parts))), (key, sorted(parts))
                self._cache[key] = np.concatenate([parts[i][0][parts[i][1]] for i in range(len(parts))], axis=0)
            return self._cache[key]
        raise KeyError(key)


def load_arrays(meta):
    return Arrays([os.path.join(GOLDEN, f) for f in meta["files"]])


def trained_names(pol):
    return [n for n, _ in pol.named_parameters() if n.startswith(("memory_s.", "student."))]


def _state(z, tag, kind, device):
    keys = [k for k in (f"{tag}0", f"{tag}1") if k in z.files]
    if not keys:
        return None
    s = tuple(torch.from_numpy(z[k]).to(device) for k in keys)
    return s if kind == "lstm" else s[0]


def build_distillation(z, meta, device):
    """(Distillation, StudentTeacherRecurrent) ready for update()."""
    from rsl_rl_amd.algorithms import Distillation
    from rsl_rl_amd.modules import StudentTeacherRecurrent

    T, N, A = meta["T"], meta["N"], meta["A"]
    Os, Ot = meta["O_student"], meta["O_teacher"]
    obs = storage_obs(meta["ranks"][0]["obs_seed"], T, N, Os, Ot)
    assert hashlib.sha256(obs["policy"].tobytes()).digest() == z["r0/obs_sha256"].tobytes(), "numpy stream differs"
    obs0 = {"policy": torch.zeros(N, Os), "teacher": torch.zeros(N, Ot)}
    groups = {"policy": ["policy"], "teacher": ["teacher"]}
    torch.manual_seed(0)
    pol = StudentTeacherRecurrent(obs0, groups, A, student_hidden_dims=meta["hidden"],
                                  teacher_hidden_dims=meta["hidden"], rnn_type=meta["rnn_type"],
                                  rnn_hidden_dim=meta["rnn_hidden_dim"], rnn_num_layers=meta["rnn_num_layers"],
                                  teacher_recurrent=meta["teacher_recurrent"], **meta["policy_kw"])
    sd = pol.state_dict()
    init = {k[len("r0/init/"):]: torch.from_numpy(z[k]) for k in z.files if k.startswith("r0/init/")}
    assert init and not any(k.startswith(("teacher.", "memory_t.")) for k in init)
    sd.update(init)
    assert pol.load_state_dict(sd) is True
    pol.train()
    alg = Distillation(pol, num_learning_epochs=meta["E"], gradient_length=meta["G"], learning_rate=1e-3,
                       max_grad_norm=meta["max_grad_norm"], loss_type=meta["loss_type"], device=device)
    alg.init_storage("distillation", N, T, obs0, [A])
    st = alg.storage
    st.observations["policy"].copy_(torch.from_numpy(obs["policy"]))
    st.observations["teacher"].copy_(torch.from_numpy(obs["teacher"]))
    st.privileged_actions.copy_(torch.from_numpy(z["r0/privileged_actions"]))
    st.dones.copy_(torch.from_numpy(z["r0/dones"]).reshape(T, N, 1))
    st.step = T
    if meta["seeded_state"]:
        kind = meta["rnn_type"]
        alg.last_hidden_states = (_state(z, "r0/last_hidden/s", kind, device),
                                  _state(z, "r0/last_hidden/t", kind, device))
    return alg, pol


def run_recorded_update(alg):
    """update() with every optimizer step's learning rate recorded and the first step's gradients (memory and MLP, per
    tensor) captured right before the step, before clipping (the fused step clips itself; torch's path clips before
    its step).  Returns check_update's `out` dict plus the per-step losses, the gradients and the hidden states."""
    lr_trace, got = [], {}
    stepper = alg._clip_adam if alg._clip_adam is not None else alg.optimizer
    step = stepper.step
    clip = torch.nn.utils.clip_grad_norm_
    pol = alg.policy
    params = dict(pol.named_parameters())

    def grab():
        if not got:
            got.update({n: params[n].grad.detach().clone() for n in trained_names(pol)})

    def rec_clip(*a, **k):
        grab()
        return clip(*a, **k)

    def rec(*a, **k):
        grab()
        lr_trace.append(float(alg.optimizer.param_groups[0]["lr"]))
        return step(*a, **k)

    stepper.step = rec
    torch.nn.utils.clip_grad_norm_ = rec_clip
    try:
        loss = alg.update()
    finally:
        stepper.step = step
        torch.nn.utils.clip_grad_norm_ = clip
    final = {k: v.detach().cpu() for k, v in pol.state_dict().items()}
    return {"loss": loss, "lr_trace": lr_trace, "lr": alg.learning_rate, "final": final,
            "grads": {k: v.cpu() for k, v in got.items()}, "step_losses": list(alg.last_step_losses),
            "hidden": pol.get_hidden_states()}


def hidden_lists(hidden):
    """get_hidden_states() as {"s0": h, "s1": c, "t0": ...} on the CPU."""
    out = {}
    for tag, x in zip("st", hidden):
        if x is not None:
            for i, s in enumerate(x if isinstance(x, tuple) else (x,)):
                out[f"{tag}{i}"] = s.detach().cpu()
    return out


def tolerance_meta(meta):
    """The meta check_update selects its parameter tolerance by: the widest layer of the trained networks, which for
    these cases includes the memory (a 256-wide memory takes the reference's sensitivity envelope)."""
    return dict(meta, hidden=list(meta["hidden"]) + [meta["rnn_hidden_dim"]])


def torch_eager_update(z, meta, device, normalizer=None):
    """The reference's update loop (distillation.py:105-151 with student_teacher_recurrent.py and memory.py) restated
    in plain torch on `device`: nn.LSTM / nn.GRU, nn.Linear + ELU, torch's losses, clip_grad_norm_ over the MLP and
    torch.optim.Adam -- the yardstick for what fp32 autograd of this update gives on the device.
    normalizer: the student's observation normaliser (a module applied as is).  Returns (final parameters by their
    state_dict names, step losses [E * T] on the device, the student memory's end state)."""
    import torch.nn as nn
    import torch.nn.functional as F

    T, N, E, G = meta["T"], meta["N"], meta["E"], meta["G"]
    init = {k[len("r0/init/"):]: torch.from_numpy(z[k]) for k in z.files if k.startswith("r0/init/")}
    kind = meta["rnn_type"]
    rnn = (nn.GRU if kind == "gru" else nn.LSTM)(meta["O_student"], meta["rnn_hidden_dim"], meta["rnn_num_layers"])
    rnn.load_state_dict({k[len("memory_s.rnn."):]: v for k, v in init.items() if k.startswith("memory_s.rnn.")})
    dims = [meta["rnn_hidden_dim"]] + list(meta["hidden"]) + [meta["A"]]
    layers = []
    for i in range(len(dims) - 1):
        layers.append(nn.Linear(dims[i], dims[i + 1]))
        if i < len(dims) - 2:
            layers.append(nn.ELU())
    mlp = nn.Sequential(*layers)
    mlp.load_state_dict({k[len("student."):]: v for k, v in init.items() if k.startswith("student.")})
    rnn.to(device).train()
    mlp.to(device).train()
    obs = torch.from_numpy(storage_obs(meta["ranks"][0]["obs_seed"], T, N, meta["O_student"],
                                       meta["O_teacher"])["policy"]).to(device)
    if normalizer is not None:
        with torch.no_grad():
            obs = normalizer(obs.reshape(T * N, -1)).reshape(T, N, -1)
    target = torch.from_numpy(z["r0/privileged_actions"]).to(device)
    done = (torch.from_numpy(z["r0/dones"]).to(device) == 1).reshape(T, 1, N, 1)
    last = _state(z, "r0/last_hidden/s", kind, device) if meta["seeded_state"] else None
    opt = torch.optim.Adam(list(rnn.parameters()) + list(mlp.parameters()), lr=1e-3)
    loss_fn = F.mse_loss if meta["loss_type"] == "mse" else F.huber_loss
    each = lambda f, s: None if s is None else (tuple(f(x) for x in s) if isinstance(s, tuple) else f(s))  # noqa: E731
    losses, loss, cnt, state = [], 0, 0, None
    for _ in range(E):
        state = each(lambda x: x.detach(), last)
        for t in range(T):
            out, state = rnn(obs[t].unsqueeze(0), state)
            step_loss = loss_fn(mlp(out.squeeze(0)), target[t])
            loss = loss + step_loss
            losses.append(step_loss.detach())
            cnt += 1
            if cnt % G == 0:
                opt.zero_grad()
                loss.backward()
                if meta["max_grad_norm"]:
                    nn.utils.clip_grad_norm_(mlp.parameters(), meta["max_grad_norm"])
                opt.step()
                state = each(lambda x: x.detach(), state)
                loss = 0
            state = each(lambda x: torch.where(done[t], torch.zeros_like(x), x), state)  # noqa: B023
    final = {"memory_s.rnn." + k: v.detach().cpu() for k, v in rnn.state_dict().items()}
    final.update({"student." + k: v.detach().cpu() for k, v in mlp.state_dict().items()})
    return final, torch.stack(losses), each(lambda x: x.detach().cpu(), state)
