"""Rebuild the distillation fixtures (tests/golden/make_golden_distillation.py) on any device: the observations are
regenerated from the fixture's numpy seed (PCG64, bit-reproducible; checked against the stored sha256), the teacher's
actions, the student's initial parameters and the reference's results come from the fixture.  The fixtures follow the
update_* family's layout (r<rank>/init/, r<rank>/final/, r0/grad_mb0, per-rank lr_trace / loss_dict in the JSON), so
tests/update_fixtures.check_update applies to them as it stands."""

import hashlib
import json
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")


def storage_obs(seed, T, N, O_student, O_teacher):
    """The stored observations of one rank: student group, then teacher group, from one PCG64 stream."""
    rng = np.random.default_rng(seed)
    return {
        "policy": rng.standard_normal((T, N, O_student), dtype=np.float32),
        "teacher": rng.standard_normal((T, N, O_teacher), dtype=np.float32),
    }


def load_meta():
    with open(os.path.join(GOLDEN, "golden_distillation.json")) as f:
        return json.load(f)


class Arrays:
    """The arrays of a case, whichever of its files holds them (np.load's `files` / [] interface)."""

    def __init__(self, paths):
        self._z = [np.load(p) for p in paths]
        self.files = [k for z in self._z for k in z.files]

    def __getitem__(self, key):
        for z in self._z:
            if key in z.files:
                return z[key]
        raise KeyError(key)


def load_arrays(case, meta):
    return Arrays([os.path.join(GOLDEN, f) for f in meta["files"]])


def build_distillation(z, meta, rank, device, world=1):
    """(Distillation, StudentTeacher) ready for update(): the fixture's initial student (and std, normaliser
    buffers), a storage holding the regenerated observations and the fixture's teacher actions."""
    from rsl_rl_amd.algorithms import Distillation
    from rsl_rl_amd.modules import StudentTeacher

    T, N, A = meta["T"], meta["N"], meta["A"]
    Os, Ot = meta["O_student"], meta["O_teacher"]
    pre = f"r{rank}/"
    obs = storage_obs(meta["ranks"][rank]["obs_seed"], T, N, Os, Ot)
    assert hashlib.sha256(obs["policy"].tobytes()).digest() == z[pre + "obs_sha256"].tobytes(), "numpy stream differs"
    obs0 = {"policy": torch.zeros(N, Os), "teacher": torch.zeros(N, Ot)}
    groups = {"policy": ["policy"], "teacher": ["teacher"]}
    torch.manual_seed(0)
    pol = StudentTeacher(obs0, groups, A, student_hidden_dims=meta["hidden"], teacher_hidden_dims=meta["hidden"],
                         **meta["policy_kw"])
    sd = pol.state_dict()
    init = {k[len("r0/init/"):]: torch.from_numpy(z[k]) for k in z.files if k.startswith("r0/init/")}
    assert init and not any(k.startswith("teacher.") for k in init)
    sd.update(init)
    assert pol.load_state_dict(sd) is True
    mcfg = {"global_rank": rank, "local_rank": 0, "world_size": world} if world > 1 else None
    alg = Distillation(pol, num_learning_epochs=meta["E"], gradient_length=meta["G"], learning_rate=1e-3,
                       max_grad_norm=meta["max_grad_norm"], loss_type=meta["loss_type"], device=device,
                       optimizer=meta.get("optimizer", "adam"), multi_gpu_cfg=mcfg)
    alg.init_storage("distillation", N, T, obs0, [A])
    st = alg.storage
    st.observations["policy"].copy_(torch.from_numpy(obs["policy"]))
    st.observations["teacher"].copy_(torch.from_numpy(obs["teacher"]))
    st.privileged_actions.copy_(torch.from_numpy(z[pre + "privileged_actions"]))
    st.step = T
    return alg, pol


def run_recorded_update(alg):
    """update() with every optimizer step's learning rate recorded and the first step's student gradient captured
    right before the step (after any all-reduce, before clipping: the step itself clips).  Returns check_update's
    `out` dict plus the per-step losses."""
    lr_trace, got = [], []
    stepper = alg._clip_adam if alg._clip_adam is not None else alg.optimizer
    step = stepper.step
    clip = torch.nn.utils.clip_grad_norm_

    def grab():
        if not got:
            got.append(torch.cat([p.grad.reshape(-1) for p in alg.policy.student.parameters()]).cpu())

    def rec_clip(*a, **k):  # the torch path clips before its step
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
    pol = alg.policy
    final = {k: v.detach().cpu() for k, v in pol.state_dict().items()}
    return {"loss": loss, "lr_trace": lr_trace, "lr": alg.learning_rate, "final": final,
            "grad_mb0": got[0] if got else None, "step_losses": list(alg.last_step_losses)}
