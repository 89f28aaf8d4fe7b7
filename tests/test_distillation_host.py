"""Distillation without a GPU: the optimizer schedule, the StudentTeacher module's checkpoint rules, the constructors'
errors, the runner's refusal to start without a teacher, and the argument validation of rslrl_bc_loss_fwd_bwd (every
error is returned before a launch, so no device is needed)."""

import ctypes
import os

import pytest
import torch

from conftest import GOLDEN
from distill_fixtures import load_meta


# ---------------------------------------------------------------------------------------------- the schedule
def test_distillation_windows():
    from rsl_rl_amd.algorithms import distillation_windows as dw

    # T 8, E 2, G 3: 5 full windows, the third across the epoch boundary, one trailing step
    assert dw(8, 2, 3) == [((0, 1, 2), True), ((3, 4, 5), True), ((6, 7, 0), True), ((1, 2, 3), True),
                           ((4, 5, 6), True), ((7,), False)]
    # T 24, E 1, G 15: one step, 9 trailing steps
    assert dw(24, 1, 15) == [(tuple(range(15)), True), (tuple(range(15, 24)), False)]
    # E * T < G: no optimizer step at all
    assert dw(4, 1, 15) == [((0, 1, 2, 3), False)]
    # windows that are exactly the epochs
    assert dw(5, 3, 5) == [((0, 1, 2, 3, 4), True)] * 3
    for T, E, G in [(8, 2, 3), (24, 1, 15), (4, 1, 15), (5, 3, 5), (2, 4, 5)]:
        w = dw(T, E, G)
        assert [t for s, _ in w for t in s] == [t for _ in range(E) for t in range(T)]
        assert sum(full for _, full in w) == (E * T) // G  # the reference steps whenever cnt % G == 0
        assert all(len(s) == G for s, full in w if full) and all(full for _, full in w[:-1])


# ---------------------------------------------------------------------------------------------- StudentTeacher
OBS0 = {"policy": torch.zeros(3, 16), "teacher": torch.zeros(3, 24)}
GROUPS = {"policy": ["policy"], "teacher": ["teacher"]}


def _student_teacher(**kw):
    from rsl_rl_amd.modules import StudentTeacher

    kw.setdefault("student_hidden_dims", [64, 64])
    kw.setdefault("teacher_hidden_dims", [64, 64])
    return StudentTeacher(OBS0, GROUPS, 4, **kw)


@pytest.mark.parametrize("std_type", ["scalar", "log"])
@pytest.mark.parametrize("norm", [False, True])
def test_state_dict_key_order(std_type, norm):
    ref = load_meta()["state_dict_keys"][f"{std_type}_{'norm' if norm else 'plain'}"]
    pol = _student_teacher(noise_std_type=std_type, student_obs_normalization=norm, teacher_obs_normalization=norm)
    assert list(pol.state_dict().keys()) == ref["state_dict"]
    assert [n for n, _ in pol.named_parameters()] == ref["parameters"]
    assert ref["state_dict"][0] == ("std" if std_type == "scalar" else "log_std")


def test_unknown_std_type():
    with pytest.raises(ValueError, match="Unknown standard deviation type"):
        _student_teacher(noise_std_type="softplus")


def test_load_state_dict_branches():
    from rsl_rl_amd.modules import ActorCritic

    # 1. an RL checkpoint: the actor (and its normaliser) become the teacher; training does not resume
    torch.manual_seed(3)
    ac = ActorCritic({"policy": torch.zeros(3, 24)}, {"policy": ["policy"], "critic": ["policy"]}, 4,
                     actor_hidden_dims=[64, 64], critic_hidden_dims=[64, 64], actor_obs_normalization=True)
    ac.train()
    ac.update_normalization({"policy": torch.randn(32, 24) * 2 + 1})
    pol = _student_teacher(teacher_obs_normalization=True)
    student_before = {k: v.clone() for k, v in pol.student.state_dict().items()}
    assert pol.loaded_teacher is False
    assert pol.load_state_dict(ac.state_dict()) is False
    assert pol.loaded_teacher is True
    for k, v in ac.actor.state_dict().items():
        assert torch.equal(pol.teacher.state_dict()[k], v), k
    for k, v in ac.actor_obs_normalizer.state_dict().items():
        assert torch.equal(pol.teacher_obs_normalizer.state_dict()[k], v), k
    for k, v in student_before.items():
        assert torch.equal(pol.student.state_dict()[k], v), k
    assert not pol.teacher.training and not pol.teacher_obs_normalizer.training
    x = {"policy": torch.randn(5, 16), "teacher": torch.randn(5, 24)}
    assert torch.equal(pol.evaluate(x), ac.act_inference({"policy": x["teacher"]}))

    # 2. a distillation checkpoint: everything loads; training resumes
    other = _student_teacher(teacher_obs_normalization=True)
    assert other.load_state_dict(pol.state_dict()) is True
    assert other.loaded_teacher is True
    for k, v in pol.state_dict().items():
        assert torch.equal(other.state_dict()[k], v), k

    # 3. neither
    with pytest.raises(ValueError, match="does not contain student or teacher parameters"):
        _student_teacher().load_state_dict({"critic.0.weight": torch.zeros(1)})


def test_train_keeps_teacher_in_eval_mode():
    pol = _student_teacher(student_obs_normalization=True, teacher_obs_normalization=True)
    pol.train()
    assert pol.training and pol.student.training and pol.student_obs_normalizer.training
    assert not pol.teacher.training and not pol.teacher_obs_normalizer.training
    pol.eval()
    pol.train(True)
    assert not pol.teacher.training and not pol.teacher_obs_normalizer.training
    assert pol.get_hidden_states() is None and pol.reset() is None and pol.detach_hidden_states() is None


# ---------------------------------------------------------------------------------------------- Distillation
def test_unknown_loss_type():
    from rsl_rl_amd.algorithms import Distillation

    with pytest.raises(ValueError, match="Unknown loss type: l1"):
        Distillation(_student_teacher(), loss_type="l1", device="cpu")
    alg = Distillation(_student_teacher(), loss_type="huber", device="cpu")
    assert alg.num_updates == 0 and alg.gradient_length == 15 and alg.max_grad_norm is None and alg.rnd is None


def test_recurrent_policy_is_refused():
    from rsl_rl_amd.algorithms import Distillation
    from rsl_rl_amd.modules import StudentTeacher

    class Recurrent(StudentTeacher):
        is_recurrent = True

    alg = Distillation(Recurrent(OBS0, GROUPS, 4, student_hidden_dims=[32], teacher_hidden_dims=[32]), device="cpu")
    with pytest.raises(NotImplementedError, match=r"distillation\.py:112-113"):
        alg.update()
    assert alg.num_updates == 0


def test_class_names_resolve():
    from rsl_rl_amd.algorithms import Distillation
    from rsl_rl_amd.modules import StudentTeacher
    from rsl_rl_amd.runners.on_policy_runner import _resolve_class

    assert _resolve_class("StudentTeacher") is StudentTeacher and _resolve_class("Distillation") is Distillation


def test_runner_refuses_to_learn_without_teacher(monkeypatch):
    from rsl_rl_amd import _lib
    from rsl_rl_amd.env import SyntheticVecEnv
    from rsl_rl_amd.runners import DistillationRunner

    env = SyntheticVecEnv(8, 16, 4, device="cpu", num_privileged_obs=24)
    cfg = {
        "num_steps_per_env": 4, "save_interval": 10,
        "obs_groups": {"policy": ["policy"], "teacher": ["privileged"]},
        "policy": {"class_name": "StudentTeacher", "student_hidden_dims": [32, 32], "teacher_hidden_dims": [32, 32]},
        "algorithm": {"class_name": "Distillation", "gradient_length": 2},
    }
    runner = DistillationRunner(env, cfg, log_dir=None, device="cpu")
    assert runner.alg.storage.training_type == "distillation"
    assert runner.alg.storage.privileged_actions.shape == (4, 8, 4)

    def no_kernel():  # learn() must raise before anything reaches the library
        raise AssertionError("a kernel was reached")

    monkeypatch.setattr(_lib, "lib", no_kernel)
    with pytest.raises(ValueError, match="Teacher model parameters not loaded"):
        runner.learn(1)


# ---------------------------------------------------------------------------------------------- the C entry point
def _args(**kw):
    from rsl_rl_amd import _lib

    a = _lib.BCLossArgs()
    a.S, a.N, a.A, a.loss_type = kw.get("S", 2), kw.get("N", 8), kw.get("A", 4), kw.get("loss_type", 0)
    a.pred_stride = a.grad_stride = a.A
    return a


def test_bc_loss_argument_validation():
    from rsl_rl_amd import _lib

    L = _lib.lib()
    assert L.rslrl_abi_version() == _lib.ABI_VERSION >= 24
    call = lambda a: L.rslrl_bc_loss_fwd_bwd(ctypes.byref(a), None, 0, None)  # noqa: E731
    assert call(_args(A=0)) == _lib.E_INVALID_ARGUMENT
    assert call(_args(A=_lib.PPO_LOSS_MAX_ACTIONS + 1)) == _lib.E_INVALID_ARGUMENT == -1
    assert call(_args(N=0)) == _lib.E_INVALID_ARGUMENT
    assert call(_args(S=-1)) == _lib.E_INVALID_ARGUMENT
    assert call(_args(loss_type=2)) == _lib.E_INVALID_ARGUMENT
    assert call(_args(S=0)) == 0  # a no-op
    assert call(_args()) == _lib.E_INVALID_ARGUMENT  # null operands
    assert L.rslrl_bc_loss_fwd_bwd(None, None, 0, None) == _lib.E_INVALID_ARGUMENT
    sizes = [L.rslrl_bc_loss_workspace_bytes(S, 4096, 12) for S in (1, 2, 3, 15, 16, 48)]
    assert all(b > a for a, b in zip(sizes, sizes[1:])), sizes


def test_bc_loss_wrapper_rejects_cpu_tensors():
    from rsl_rl_amd import kernels

    with pytest.raises(RuntimeError, match="no CPU fallback"):
        kernels.bc_loss(torch.zeros(8, 4), torch.zeros(8, 4), 8, "mse", torch.zeros(1))


# ---------------------------------------------------------------------------------------------- fixtures
def test_fixtures_present():
    meta = load_meta()
    for case in ("a", "b", "c", "w2"):
        assert case in meta, case
        for f in meta[case]["files"]:
            path = os.path.join(GOLDEN, f)
            assert os.path.exists(path), path
            assert os.path.getsize(path) < (1 << 20), path
        m = meta[case]
        assert len(m["ranks"]) == m["world"]
        assert m["ranks"][0]["num_steps"] == (m["E"] * m["T"]) // m["G"]
    assert meta["a"]["ranks"][0]["num_steps"] == 5 and meta["c"]["ranks"][0]["num_steps"] == 1
    assert meta["a"]["ranks"][0]["grad_norm0"] > 1.0 and meta["c"]["ranks"][0]["grad_norm0"] > 1.0
    assert min(meta["b"]["ranks"][0]["huber_fractions"]) >= 0.02
