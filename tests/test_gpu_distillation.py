"""Distillation.update() on the GPU against the reference's own update (tests/golden/distill_<case>.npz, written by
tests/golden/make_golden_distillation.py from rsl_rl/algorithms/distillation.py run on CPU), the paired rollout step
of StudentTeacher, and one DistillationRunner run end to end.

Cases a (MSE, clip, a window across the epoch boundary, a trailing step), b (Huber, log std, student normaliser, no
clip) and c (3 x 256, one step and 9 trailing steps), each on the window-batched path and, with RSLRL_DISTILL_FUSED=0,
on the per-step path.  Tolerances are tests/update_fixtures.check_update's: the number of optimizer steps exact (one
learning rate per step), loss_dict rtol 1e-4, the first gradient within 1e-5, parameters within atol 2e-5 at width 64
and within the reference's own one-ulp sensitivity envelope (2 * sens + 1e-4 of the distance moved) at 3 x 256; in
addition every step loss rtol 1e-4 and the first gradient within 1e-5 of each tensor's max."""

import os

import numpy as np
import pytest
import torch

from distill_fixtures import build_distillation, load_arrays, load_meta, run_recorded_update
from update_fixtures import check_update

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("fused", [True, False], ids=["windows", "per_step"])
@pytest.mark.parametrize("case", ["a", "b", "c"])
def test_update_matches_reference(case, fused, cuda_device, monkeypatch):
    monkeypatch.setenv("RSLRL_DISTILL_FUSED", "1" if fused else "0")
    meta = load_meta()[case]
    z = load_arrays(case, meta)
    alg, pol = build_distillation(z, meta, 0, "cuda:0")
    assert alg._fused_ok() is fused
    before = {k: v.detach().clone() for k, v in pol.state_dict().items()}
    out = run_recorded_update(alg)
    ref = meta["ranks"][0]

    # the schedule: one optimizer step per full window, every step loss (trailing ones included) in the statistic
    assert len(out["lr_trace"]) == ref["num_steps"] == alg.optimizer.state[pol.student[0].weight]["step"].item()
    ref_steps = z["r0/step_losses"]
    ours = np.asarray(out["step_losses"])
    assert ours.shape == ref_steps.shape == (meta["E"] * meta["T"],)
    print(case, "step losses: max rel err", np.max(np.abs(ours - ref_steps) / np.abs(ref_steps)))
    assert np.all(np.abs(ours - ref_steps) <= 1e-4 * np.abs(ref_steps)), (ours, ref_steps)
    assert set(out["loss"]) == {"behavior"}
    check_update(out, z, meta, 0, mode="windows" if fused else "per_step")

    # the first gradient, tensor by tensor
    ref_grad = torch.from_numpy(z["r0/grad_mb0"]).double()
    off = 0
    for name, p in pol.student.named_parameters():
        r = ref_grad[off:off + p.numel()]
        o = out["grad_mb0"][off:off + p.numel()].double()
        off += p.numel()
        assert (o - r).abs().max().item() <= 1e-5 * r.abs().max().item(), name
    assert off == ref_grad.numel()

    # only the student moves; only its parameters carry a gradient and optimizer state
    for k, v in pol.state_dict().items():
        if k.startswith("student."):
            assert not torch.equal(v, before[k]), k
        else:
            assert torch.equal(v, before[k]), k
    for name, p in pol.named_parameters():
        is_student = name.startswith("student.")
        assert (p.grad is not None) == is_student, name
        assert (len(alg.optimizer.state.get(p, {})) > 0) == is_student, name
    if fused:  # the gradients are views of one flat arena
        flat = alg._arena.flat
        assert all(flat.data_ptr() <= p.grad.data_ptr() < flat.data_ptr() + 4 * flat.numel()
                   for p in pol.student.parameters())
    assert alg.num_updates == 1 and alg.storage.step == 0


def test_update_without_a_full_window(cuda_device):
    """E * T < gradient_length: every step loss is evaluated, no optimizer step is taken."""
    meta = dict(load_meta()["a"], G=40)
    z = load_arrays("a", meta)
    alg, pol = build_distillation(z, meta, 0, "cuda:0")
    before = {k: v.detach().clone() for k, v in pol.state_dict().items()}
    out = run_recorded_update(alg)
    assert out["lr_trace"] == [] and len(out["step_losses"]) == meta["E"] * meta["T"]
    # at the initial parameters the two epochs see the same losses: the reference's first three (before its first step)
    assert np.allclose(out["step_losses"][:3], z["r0/step_losses"][:3], rtol=1e-4, atol=0)
    assert out["step_losses"][:meta["T"]] == out["step_losses"][meta["T"]:]
    for k, v in pol.state_dict().items():
        assert torch.equal(v, before[k]), k


def test_update_with_an_optimizer_the_fused_step_does_not_take(cuda_device):
    """optimizer="sgd": the per-step path is taken by itself, with torch's clip_grad_norm_ over the student's
    parameters and optimizer.step().  The schedule is the same; the losses before the first step are the reference's."""
    meta = dict(load_meta()["a"], optimizer="sgd")
    z = load_arrays("a", meta)
    alg, pol = build_distillation(z, meta, 0, "cuda:0")
    assert alg._clip_adam is None and not alg._fused_ok()
    before = {k: v.detach().clone() for k, v in pol.state_dict().items()}
    out = run_recorded_update(alg)
    assert len(out["lr_trace"]) == meta["ranks"][0]["num_steps"]
    assert np.allclose(out["step_losses"][:3], z["r0/step_losses"][:3], rtol=1e-4, atol=0)
    assert np.all(np.isfinite(out["step_losses"])) and len(out["step_losses"]) == meta["E"] * meta["T"]
    # the first gradient is the reference's (taken before torch's clip), and it was clipped to max_grad_norm
    ref_grad = torch.from_numpy(z["r0/grad_mb0"]).double()
    assert (out["grad_mb0"].double() - ref_grad).abs().max() <= 1e-5 * ref_grad.abs().max()
    for k, v in pol.state_dict().items():
        assert torch.equal(v, before[k]) != k.startswith("student."), k


@pytest.mark.parametrize("n_envs,o_teacher", [(256, 48), (100, 48), (256, 64)],
                         ids=["pair_n256", "fallback_n100", "other_widths"])
def test_act_and_evaluate_matches_act_then_evaluate(n_envs, o_teacher, cuda_device):
    from rsl_rl_amd.modules import StudentTeacher

    torch.manual_seed(5)
    obs = {"policy": torch.randn(n_envs, 48, device=cuda_device), "teacher": torch.randn(n_envs, o_teacher,
                                                                                           device=cuda_device)}
    groups = {"policy": ["policy"], "teacher": ["teacher"]}
    pol = StudentTeacher(obs, groups, 12, student_obs_normalization=True).to(cuda_device)
    pol.train()
    pol.update_normalization({k: v * 2 + 1 for k, v in obs.items()})
    with torch.inference_mode():
        state = torch.cuda.get_rng_state(cuda_device)
        a0, t0 = pol.act(obs), pol.evaluate(obs)
        mean0 = pol.action_mean.clone()
        after0 = torch.cuda.get_rng_state(cuda_device)
        torch.cuda.set_rng_state(state, cuda_device)
        a1, t1 = pol.act_and_evaluate(obs)
        after1 = torch.cuda.get_rng_state(cuda_device)
    assert torch.equal(t1, t0)
    assert torch.equal(pol.action_mean, mean0)
    assert torch.equal(a1, a0)
    assert torch.equal(after0, after1)  # the same generator draws
    assert not torch.equal(a0, mean0)


class _Writer:
    def __init__(self):
        self.scalars = {}

    def add_scalar(self, key, value, step):
        self.scalars.setdefault(key, []).append((step, float(value)))


def test_runner_end_to_end(cuda_device, tmp_path):
    from rsl_rl_amd.env import SyntheticVecEnv
    from rsl_rl_amd.modules import ActorCritic
    from rsl_rl_amd.runners import DistillationRunner

    dev = "cuda:0"
    N, T, Os, Ot, A = 256, 8, 16, 24, 4

    def make_runner(log_dir=None):
        env = SyntheticVecEnv(N, Os, A, device=dev, seed=3, num_privileged_obs=Ot)
        cfg = {
            "num_steps_per_env": T, "save_interval": 1,
            "obs_groups": {"policy": ["policy"], "teacher": ["privileged"]},
            "policy": {"class_name": "StudentTeacher", "student_hidden_dims": [64, 64],
                       "teacher_hidden_dims": [64, 64], "student_obs_normalization": True},
            "algorithm": {"class_name": "Distillation", "gradient_length": 3, "num_learning_epochs": 2,
                          "learning_rate": 1e-3, "max_grad_norm": 1.0},
        }
        torch.manual_seed(11)
        return DistillationRunner(env, cfg, log_dir=log_dir, device=dev)

    # the teacher: the actor of a PPO-format checkpoint
    torch.manual_seed(7)
    ac = ActorCritic({"policy": torch.zeros(N, Ot)}, {"policy": ["policy"], "critic": ["policy"]}, A,
                     actor_hidden_dims=[64, 64], critic_hidden_dims=[64, 64])
    with torch.no_grad():
        ac.actor[-1].weight.mul_(4.0)  # a teacher with outputs of order one
    ppo_ckpt = str(tmp_path / "ppo_model.pt")
    torch.save({"model_state_dict": ac.state_dict(), "optimizer_state_dict": {}, "iter": 17, "infos": None}, ppo_ckpt)

    (tmp_path / "run").mkdir()  # the tensorboard writer creates its log_dir; the stub below does not
    runner = make_runner(log_dir=str(tmp_path / "run"))
    runner.writer = _Writer()
    with pytest.raises(ValueError, match="Teacher model parameters not loaded"):
        runner.learn(1)
    runner.load(ppo_ckpt)
    pol = runner.alg.policy
    assert pol.loaded_teacher and runner.current_learning_iteration == 0  # an RL checkpoint does not resume
    assert torch.equal(pol.teacher[0].weight.cpu(), ac.actor[0].weight)

    losses = []
    for _ in range(2):
        runner.learn(1)
        runner.current_learning_iteration += 1
        stats = runner.last_iteration_stats
        assert set(stats["loss_dict"]) == {"behavior"} and np.isfinite(stats["loss_dict"]["behavior"])
        assert stats["collection_time"] > 0 and stats["learn_time"] > 0 and stats["total_fps"] > 0
        losses.append(stats["loss_dict"]["behavior"])
    print("behavior loss per iteration:", losses)
    assert losses[1] <= losses[0], losses
    assert [v for _, v in runner.writer.scalars["Loss/behavior"]] == losses
    assert runner.alg.num_updates == 2
    assert pol.student_obs_normalizer.count.item() == 2 * T * N

    # save, then load into a fresh runner: the same parameters, and the run resumes
    path = str(tmp_path / "distill_model.pt")
    runner.save(path)
    saved = {k: v.detach().clone() for k, v in pol.state_dict().items()}
    other = make_runner()
    assert not other.alg.policy.loaded_teacher
    other.load(path)
    assert other.alg.policy.loaded_teacher
    assert other.current_learning_iteration == runner.current_learning_iteration == 2
    for k, v in other.alg.policy.state_dict().items():
        assert torch.equal(v, saved[k]), k
    other.learn(1)  # the loaded optimizer state steps on
    assert np.isfinite(other.last_iteration_stats["loss_dict"]["behavior"])
    assert os.path.exists(str(tmp_path / "run" / "model_1.pt"))
