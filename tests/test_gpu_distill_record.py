"""The one-launch distillation step record (csrc/distill_record.hip, kernels.distill_record,
RolloutStorage.add_transition_distill) against RolloutStorage.add_transitions on a twin storage: row t
of every field bit for bit, every other row untouched; which transitions Distillation.process_env_step hands it; and a
DistillationRunner iteration that leaves the same storage bytes with RSLRL_DISTILL_RECORD on and off."""

import pytest
import torch

pytestmark = pytest.mark.gpu

T = 3
DONES = {"f32": torch.float32, "u8": torch.uint8, "bool": torch.bool, "i32": torch.int32, "i64": torch.int64}
GROUPS = {"one_ragged": (45,), "aligned_and_ragged": (48, 7), "four": (235, 48, 3, 64)}


def _storages(N, widths, A, dev):
    from rsl_rl_amd.storage import RolloutStorage

    obs0 = {f"g{i}": torch.zeros(N, w) for i, w in enumerate(widths)}
    pair = [RolloutStorage("distillation", N, T, obs0, [A], dev) for _ in range(2)]
    for st in pair:  # sentinels: NaN (0xFF for the uint8 dones)
        for buf in list(st.observations.values()) + [st.actions, st.privileged_actions, st.rewards]:
            buf.fill_(float("nan"))
        st.dones.fill_(0xFF)
    return pair


def _transition(N, widths, A, dones_dtype, dev, seed):
    from rsl_rl_amd.storage import RolloutStorage
    from rsl_rl_amd.utils import TensorDict

    g = torch.Generator(device=dev).manual_seed(seed)
    tr = RolloutStorage.Transition()
    tr.observations = TensorDict({f"g{i}": torch.randn(N, w, device=dev, generator=g) for i, w in enumerate(widths)},
                                 batch_size=[N], device=dev)
    tr.actions = torch.randn(N, A, device=dev, generator=g)
    tr.privileged_actions = torch.randn(N, A, device=dev, generator=g)
    tr.rewards = torch.randn(N, device=dev, generator=g)
    tr.dones = (torch.rand(N, device=dev, generator=g) < 0.4).to(dones_dtype)
    return tr


def _fields(st):
    return dict(st.observations.items(), actions=st.actions, privileged_actions=st.privileged_actions,
                rewards=st.rewards, dones=st.dones)


def _same_bytes(a, b):
    """Bit equality, NaN sentinels included."""
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8),
                                                                      b.contiguous().view(torch.uint8))


@pytest.mark.parametrize("dones", list(DONES))
@pytest.mark.parametrize("A", [3, 12])
@pytest.mark.parametrize("groups", list(GROUPS))
@pytest.mark.parametrize("N", [1, 100, 256])
def test_row_matches_add_transitions(N, groups, A, dones, cuda_device):
    widths = GROUPS[groups]
    ours, ref = _storages(N, widths, A, cuda_device)
    for t in range(T):  # t = 0 ... T - 1: step and _fills advance as add_transitions advances them
        tr = _transition(N, widths, A, DONES[dones], cuda_device, seed=7 + t)
        assert ours.step == ref.step == t and ours.distill_record_ok(tr)
        if t == 1:  # only rows 0 and T - 1 go through the kernel: row 1 keeps its sentinels in both storages
            ours.step, ref.step = 2, 2
            continue
        ours.add_transition_distill(tr)
        ref.add_transitions(tr)
        assert ours._fills == ref._fills
    assert ours.step == ref.step == T
    assert N == 1 or (tr.dones.any() and not tr.dones.all())
    for (name, a), b in zip(_fields(ours).items(), _fields(ref).values()):
        for t in (0, T - 1):
            assert torch.equal(a[t], b[t]) and not torch.isnan(a[t].float()).any(), (name, t)
        assert _same_bytes(a, b), name  # row 1 is still the sentinel
        assert (torch.isnan(a[1]).all() if a.dtype == torch.float32 else (a[1] == 0xFF).all()), name
    with pytest.raises(OverflowError):
        ours.add_transition_distill(tr)


def test_misaligned_groups_take_dword_units(cuda_device):
    """A source that starts 4 bytes into an allocation (contiguous, 4-aligned width): no 16-byte claim, same bytes."""
    N, A = 100, 12
    ours, ref = _storages(N, (48,), A, cuda_device)
    tr = _transition(N, (48,), A, torch.int64, cuda_device, seed=3)
    shifted = torch.randn(N * 48 + 1, device=cuda_device)[1:].view(N, 48)
    assert shifted.is_contiguous() and shifted.data_ptr() % 16 == 4
    tr.observations["g0"] = shifted
    assert ours.distill_record_ok(tr)
    ours.add_transition_distill(tr)
    ref.add_transitions(tr)
    for (name, a), b in zip(_fields(ours).items(), _fields(ref).values()):
        assert _same_bytes(a, b), name


def _spied_algorithm(monkeypatch, dev, N=64, widths=(45, 64), A=12):
    from rsl_rl_amd.algorithms import Distillation
    from rsl_rl_amd.modules import StudentTeacher
    from rsl_rl_amd.storage import RolloutStorage

    obs0 = {"policy": torch.zeros(N, widths[0]), "teacher": torch.zeros(N, widths[1])}
    pol = StudentTeacher(obs0, {"policy": ["policy"], "teacher": ["teacher"]}, A, student_hidden_dims=[64, 64],
                         teacher_hidden_dims=[64, 64])
    alg = Distillation(pol, device=dev)
    alg.init_storage("distillation", N, T, obs0, [A])
    calls = {"distill": 0, "copies": 0}
    for name, key in (("add_transition_distill", "distill"), ("add_transitions", "copies")):
        real = getattr(RolloutStorage, name)

        def counted(self, tr, real=real, key=key):
            calls[key] += 1
            return real(self, tr)

        monkeypatch.setattr(RolloutStorage, name, counted)
    return alg, calls


def _env_step(alg, dev, N=64, widths=(45, 64), dones_dtype=torch.int64, noncontiguous=False):
    from rsl_rl_amd.utils import TensorDict

    obs = TensorDict({"policy": torch.randn(N, widths[0], device=dev), "teacher": torch.randn(N, widths[1], device=dev)},
                     batch_size=[N], device=dev)
    if noncontiguous:
        obs["teacher"] = torch.randn(N, 2 * widths[1], device=dev)[:, ::2]
    with torch.inference_mode():
        alg.act(obs)
        alg.process_env_step(obs, torch.randn(N, device=dev), (torch.rand(N, device=dev) < 0.3).to(dones_dtype), {})


def test_process_env_step_takes_the_record_where_it_applies(cuda_device, monkeypatch):
    alg, calls = _spied_algorithm(monkeypatch, cuda_device)
    _env_step(alg, cuda_device)
    assert calls == {"distill": 1, "copies": 0}
    _env_step(alg, cuda_device, noncontiguous=True)  # a strided source: the per-field copies
    assert calls == {"distill": 1, "copies": 1}
    monkeypatch.setenv("RSLRL_DISTILL_RECORD", "0")
    _env_step(alg, cuda_device)
    assert calls == {"distill": 1, "copies": 2} and alg.storage.step == 3
    monkeypatch.delenv("RSLRL_DISTILL_RECORD")
    alg.storage.clear()
    _env_step(alg, cuda_device, dones_dtype=torch.float16)  # a dones dtype without a code
    assert calls == {"distill": 1, "copies": 3}
    alg.transition.hidden_states = (None, None)  # anything but None keeps add_transitions
    _env_step(alg, cuda_device)
    assert calls == {"distill": 1, "copies": 4}
    # above DISTILL_RECORD_MAX_ROWS envs the launch is opt-in: RSLRL_DISTILL_RECORD=1 takes it at any size
    from rsl_rl_amd.algorithms import distillation

    assert alg.storage.num_envs <= distillation.DISTILL_RECORD_MAX_ROWS
    monkeypatch.setattr(distillation, "DISTILL_RECORD_MAX_ROWS", alg.storage.num_envs - 1)
    alg.storage.clear()
    _env_step(alg, cuda_device)
    assert calls == {"distill": 1, "copies": 5}
    monkeypatch.setenv("RSLRL_DISTILL_RECORD", "1")
    _env_step(alg, cuda_device)
    assert calls == {"distill": 2, "copies": 5}


@pytest.mark.parametrize("n_obs", [45, 48])
def test_runner_leaves_the_same_storage(n_obs, cuda_device, monkeypatch, tmp_path):
    from rsl_rl_amd.env import SyntheticVecEnv
    from rsl_rl_amd.modules import ActorCritic
    from rsl_rl_amd.runners import DistillationRunner
    from rsl_rl_amd.storage import RolloutStorage

    N, steps, Ot, A = 128, 4, 24, 4
    torch.manual_seed(7)
    ac = ActorCritic({"policy": torch.zeros(N, Ot)}, {"policy": ["policy"], "critic": ["policy"]}, A,
                     actor_hidden_dims=[64, 64], critic_hidden_dims=[64, 64])
    ckpt = str(tmp_path / "ppo_model.pt")
    torch.save({"model_state_dict": ac.state_dict(), "optimizer_state_dict": {}, "iter": 0, "infos": None}, ckpt)

    def run(knob):
        monkeypatch.setenv("RSLRL_DISTILL_RECORD", knob)
        taken = []
        real = RolloutStorage.add_transition_distill
        monkeypatch.setattr(RolloutStorage, "add_transition_distill", lambda self, tr: (taken.append(1), real(self, tr))[1])
        env = SyntheticVecEnv(N, n_obs, A, device="cuda:0", seed=3, num_privileged_obs=Ot)
        cfg = {"num_steps_per_env": steps, "save_interval": 100,
               "obs_groups": {"policy": ["policy"], "teacher": ["privileged"]},
               "policy": {"class_name": "StudentTeacher", "student_hidden_dims": [64, 64],
                          "teacher_hidden_dims": [64, 64]},
               "algorithm": {"class_name": "Distillation", "gradient_length": 2, "learning_rate": 1e-3}}
        torch.manual_seed(11)
        runner = DistillationRunner(env, cfg, log_dir=None, device="cuda:0")
        runner.load(ckpt)
        runner.learn(1)
        monkeypatch.setattr(RolloutStorage, "add_transition_distill", real)
        return _fields(runner.alg.storage), len(taken)

    on, n_on = run("1")
    off, n_off = run("0")
    assert (n_on, n_off) == (steps, 0)
    assert sorted(on) == sorted(off) and len(on) == 6
    for name in on:
        assert _same_bytes(on[name], off[name]), name
        assert on[name].float().abs().sum() > 0 or name == "dones", name
