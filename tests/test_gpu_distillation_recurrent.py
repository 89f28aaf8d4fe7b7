"""Recurrent distillation on the GPU: Distillation.update() with a StudentTeacherRecurrent against the reference's own
update (tests/golden/drec_<case>*.npz, written by tests/golden/make_golden_distillation_recurrent.py from
rsl_rl/algorithms/distillation.py run on CPU) -- case c on the window-batched path and, with RSLRL_DISTILL_FUSED=0, on
the per-step path; a and b (H 32; a two-layer GRU) on the per-step path they fall back to -- which path ran (reverse
cell steps counted), which parameters the clip spans, the gradient arena, the read-backs, the paired rollout step, the
subset clip of the fused optimizer step, and one DistillationRunner run end to end.

Tolerances: the number of optimizer steps exact, loss_dict and every step loss rtol 1e-4, the first
gradient within 1e-5 of each tensor's max, parameters within atol 2e-5 for the narrow cases a and b and within the
reference's own one-ulp sensitivity envelope (2 * sens + 1e-4 of the distance moved) for the 256-wide case c; hidden
states after the update within 2e-5 (a, b) / 2 * sens + 1e-4 of the largest state (c), the teacher's exactly.  Where
a quantity misses its tolerance, torch's own GPU autograd of the same update (drec_fixtures.torch_eager_update) is
measured on the same fixture and device, and twice its distance is allowed."""

import os

import numpy as np
import pytest
import torch

import drec_fixtures as D
from update_fixtures import param_errors

pytestmark = pytest.mark.gpu

META = D.load_meta()


class _Baseline:
    """torch's own GPU autograd of the case, computed at most once and only when a tolerance is missed."""

    def __init__(self, z, meta, pol, device):
        self.args, self.value = (z, meta, device, pol.student_obs_normalizer), None
        self.init_norm = {k: v.detach().clone() for k, v in pol.student_obs_normalizer.state_dict().items()}

    def get(self):
        if self.value is None:
            z, meta, device, norm = self.args
            import copy
            norm = copy.deepcopy(norm)
            norm.load_state_dict(self.init_norm)
            norm.eval()
            final, _, state = D.torch_eager_update(z, meta, device, normalizer=norm)
            states = state if isinstance(state, tuple) else (state,)
            self.value = (param_errors(final, z, "r0/"),
                          {f"s{i}": (s - torch.from_numpy(z[f"r0/hidden_final/s{i}"])).abs().max().item()
                           for i, s in enumerate(states)})
            print("torch GPU autograd baseline:", {k: f"{a:.1e}/{m:.1e}" for k, (a, m) in self.value[0].items()},
                  self.value[1])
        return self.value


def _count_backward_launches(monkeypatch):
    """Counts calls of the reverse-step wrapper: the window-batched path runs one per step of every full window."""
    from rsl_rl_amd import kernels

    calls = []
    real = kernels.lstm_cell_bwd

    def counted(*a, **k):
        calls.append(1)
        return real(*a, **k)

    monkeypatch.setattr(kernels, "lstm_cell_bwd", counted)
    return calls


@pytest.mark.parametrize("case,fused", [("a", True), ("b", True), ("c", True), ("c", False)],
                         ids=["a", "b", "c_windows", "c_per_step"])
def test_update_matches_reference(case, fused, cuda_device, monkeypatch):
    monkeypatch.setenv("RSLRL_DISTILL_FUSED", "1" if fused else "0")
    meta = META[case]
    z = D.load_arrays(meta)
    alg, pol = D.build_distillation(z, meta, "cuda:0")
    windows = fused and case == "c"  # a (H 32) and b (GRU, two layers) do not qualify for the fused cell
    assert alg._clip_adam is not None and not alg._fused_ok() and alg._fused_recurrent_ok() is windows
    calls = _count_backward_launches(monkeypatch)
    before = {k: v.detach().clone() for k, v in pol.state_dict().items()}
    base = _Baseline(z, meta, pol, "cuda:0")
    out = D.run_recorded_update(alg)
    ref = meta["ranks"][0]
    # the window path really ran: one reverse step per step of each of the five full windows -- or not at all
    assert len(calls) == (ref["num_steps"] * meta["G"] if windows else 0)
    if windows:  # every gradient is a view of the one arena the multi-GPU all-reduce runs on
        flat = alg._arena.flat
        with_grad = [p for p in pol.parameters() if p.grad is not None]
        assert len(with_grad) == len(alg._arena.params) == len(D.trained_names(pol))
        assert all(p is q and p.grad.data_ptr() == v.data_ptr()
                   for p, q, v in zip(with_grad, alg._arena.params, alg._arena.views))
        assert all(flat.data_ptr() <= p.grad.data_ptr() < flat.data_ptr() + 4 * flat.numel() for p in with_grad)
        assert flat.numel() == sum(p.numel() for p in with_grad)

    # the schedule and the losses
    assert out["lr_trace"] == ref["lr_trace"] and out["lr"] == ref["final_lr"]
    assert len(out["lr_trace"]) == ref["num_steps"] == alg.optimizer.state[pol.student[0].weight]["step"].item()
    ref_steps = z["r0/step_losses"]
    ours = np.asarray(out["step_losses"])
    assert ours.shape == ref_steps.shape == (meta["E"] * meta["T"],)
    print(case, "step losses: max rel err", np.max(np.abs(ours - ref_steps) / np.abs(ref_steps)))
    assert np.all(np.abs(ours - ref_steps) <= 1e-4 * np.abs(ref_steps)), (ours, ref_steps)
    assert set(out["loss"]) == {"behavior"}
    v = ref["loss_dict"]["behavior"]
    assert abs(out["loss"]["behavior"] - v) <= 1e-4 * abs(v) + 1e-6

    # the first gradient before clipping, tensor by tensor, memory and MLP
    names = D.trained_names(pol)
    assert sorted(out["grads"]) == sorted(names) and any(n.startswith("memory_s.") for n in names)
    gerr = {}
    for n in names:
        r = torch.from_numpy(z["r0/grad_mb0/" + n]).double()
        gerr[n] = (out["grads"][n].double() - r).abs().max().item() / r.abs().max().item()
    print(case, "first gradient, max err / max:", {k: f"{e:.1e}" for k, e in gerr.items()})
    assert all(e <= 1e-5 for e in gerr.values()), gerr

    # the parameters
    errs = param_errors(out["final"], z, "r0/")
    print(case, "param errors (max abs / ||d|| over ||moved||):", {k: f"{a:.1e}/{m:.1e}" for k, (a, m) in errs.items()})
    assert sorted(errs) == sorted(names)
    wide = meta["rnn_hidden_dim"] >= 256
    sens = meta["ulp_sensitivity"]
    for name, (abs_err, rel_moved) in errs.items():
        ok = rel_moved <= 2 * sens[name] + 1e-4 if wide else abs_err <= 2e-5
        if not ok:
            b_abs, b_rel = base.get()[0][name]
            assert (rel_moved <= 2 * b_rel) if wide else (abs_err <= 2 * b_abs), (name, abs_err, rel_moved, b_abs, b_rel)

    # the hidden states of both memories after the update
    hid = D.hidden_lists(out["hidden"])
    assert sorted(hid) == sorted(k[len("r0/hidden_final/"):] for k in z.files if k.startswith("r0/hidden_final/"))
    for k, h in hid.items():
        r = torch.from_numpy(z["r0/hidden_final/" + k])
        if k.startswith("t"):  # the teacher's memory is only ever zeroed
            assert torch.equal(h, r), k
            continue
        d = (h - r).abs().max().item()
        tol = 2 * sens["hidden_final/" + k] + 1e-4 * r.abs().max().item() if wide else 2e-5
        print(case, "hidden state", k, "max err", d, "tolerance", tol)
        if d > tol:
            assert d <= 2 * base.get()[1][k], (k, d, base.get()[1][k])
    done_last = torch.from_numpy(z["r0/dones"])[-1] == 1
    assert (hid["s0"][:, done_last] == 0).all() and (hid["s0"][:, ~done_last] != 0).any()

    # the memory and the MLP move, nothing else does; only they carry a gradient and optimizer state
    for k, v in pol.state_dict().items():
        assert torch.equal(v, before[k]) != k.startswith(("student.", "memory_s.")), k
    for name, p in pol.named_parameters():
        trained = name in names
        assert (p.grad is not None) == trained, name
        assert (len(alg.optimizer.state.get(p, {})) > 0) == trained, name
    assert alg.num_updates == 1 and alg.storage.step == 0
    # the next update starts from this one's end state
    assert all(torch.equal(a, b) for a, b in zip(D.hidden_lists(alg.last_hidden_states).values(), hid.values()))


def test_the_clip_spans_the_student_mlp_only(cuda_device):
    """Case c is built so that the norm over memory and MLP differs from the MLP's by more than 1 %: clipping by the
    wrong norm moves the first step's MLP parameters by that much.  Checked on the first optimizer step alone."""
    meta = dict(META["c"], E=1, T=3)
    norms = META["c"]["ranks"][0]["grad_norms"]
    assert norms["mlp"] > 1.0 and norms["full"] > 1.01 * norms["mlp"] and norms["memory"] > 0
    z = D.load_arrays(META["c"])
    alg, pol = D.build_distillation(z, META["c"], "cuda:0")
    assert alg._clip_adam.clip_params is not None
    assert [id(p) for p in alg._clip_adam.clip_params] == [id(p) for p in pol.student.parameters()]
    alg.storage.num_transitions_per_env, alg.num_learning_epochs = meta["T"], 1  # the first window only
    out = D.run_recorded_update(alg)
    assert len(out["lr_trace"]) == 1
    # after the step .grad holds what was stepped: the MLP's scaled by max_norm / (its own norm + 1e-6), the memory's
    # as the backward left it
    coef = 1.0 / (norms["mlp"] + 1e-6)
    for n, p in pol.named_parameters():
        if n.startswith("student."):
            want = out["grads"][n].double() * coef
            assert (p.grad.cpu().double() - want).abs().max() <= 1e-4 * want.abs().max(), n
        elif n.startswith("memory_s."):
            assert torch.equal(p.grad.cpu(), out["grads"][n]), n


@pytest.mark.parametrize("case", ["a", "b", "c"])
def test_update_reads_the_device_back_once(case, cuda_device):
    """On the per-step path (a, b) and on the window path (c)."""
    meta = META[case]
    z = D.load_arrays(meta)
    alg, _ = D.build_distillation(z, meta, "cuda:0")
    alg.update()  # warm-up: allocations, library initialisation
    alg2, _ = D.build_distillation(z, meta, "cuda:0")
    assert alg2._fused_recurrent_ok() is (case == "c")
    reads = []
    tolist = torch.Tensor.tolist

    def counted(self):
        if not self.is_cuda:
            return tolist(self)
        reads.append(self.numel())
        torch.cuda.set_sync_debug_mode("default")
        try:
            return tolist(self)
        finally:
            torch.cuda.set_sync_debug_mode("error")

    torch.cuda.synchronize()
    torch.Tensor.tolist = counted
    torch.cuda.set_sync_debug_mode("error")
    try:
        loss = alg2.update()
    finally:
        torch.cuda.set_sync_debug_mode("default")
        torch.Tensor.tolist = tolist
    assert reads == [meta["E"] * meta["T"]], reads
    assert np.isfinite(loss["behavior"])


def _policy(n_envs, dev, rnn_type="lstm", hidden=256, layers=1, teacher_recurrent=False, Os=48, Ot=64, A=12, **kw):
    from rsl_rl_amd.modules import StudentTeacherRecurrent

    obs0 = {"policy": torch.zeros(n_envs, Os), "teacher": torch.zeros(n_envs, Ot)}
    groups = {"policy": ["policy"], "teacher": ["teacher"]}
    pol = StudentTeacherRecurrent(obs0, groups, A, rnn_type=rnn_type, rnn_hidden_dim=hidden, rnn_num_layers=layers,
                                  teacher_recurrent=teacher_recurrent, **kw).to(dev)
    pol.train()
    return pol


def test_rollout_step_has_no_read_back(cuda_device):
    from rsl_rl_amd.algorithms import Distillation

    torch.manual_seed(0)
    N, T, Os, Ot, A = 64, 4, 48, 64, 12
    pol = _policy(N, cuda_device, teacher_recurrent=True, student_obs_normalization=True)
    alg = Distillation(pol, device=cuda_device)
    obs0 = {"policy": torch.zeros(N, Os), "teacher": torch.zeros(N, Ot)}
    alg.init_storage("distillation", N, T, obs0, [A])
    obs = [{"policy": torch.randn(N, Os, device=cuda_device), "teacher": torch.randn(N, Ot, device=cuda_device)}
           for _ in range(T)]
    rew = torch.randn(N, device=cuda_device)
    dones = (torch.rand(N, device=cuda_device) < 0.3).long()
    with torch.inference_mode():
        alg.act(obs[0])  # warm-up
        alg.process_env_step(obs[0], rew, dones, {})
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            for t in range(1, T):
                alg.act(obs[t])
                alg.process_env_step(obs[t], rew, dones, {})
        finally:
            torch.cuda.set_sync_debug_mode("default")
    for h, c in pol.get_hidden_states():
        assert (h[:, dones == 1] == 0.0).all() and (c[:, dones == 1] == 0.0).all() and (h[:, dones == 0] != 0).any()
    assert alg.storage.step == T


@pytest.mark.parametrize("teacher_recurrent", [False, True], ids=["ff_teacher", "recurrent_teacher"])
@pytest.mark.parametrize("rnn_type,hidden,n_envs", [("lstm", 256, 128), ("gru", 32, 100)], ids=["fused", "fallback"])
def test_act_and_evaluate_matches_act_then_evaluate(rnn_type, hidden, n_envs, teacher_recurrent, cuda_device):
    torch.manual_seed(5)
    pol = _policy(n_envs, cuda_device, rnn_type, hidden, teacher_recurrent=teacher_recurrent,
                  student_obs_normalization=True)
    obs = [{"policy": torch.randn(n_envs, 48, device=cuda_device), "teacher": torch.randn(n_envs, 64,
                                                                                        device=cuda_device)}
           for _ in range(3)]
    pol.update_normalization({k: v * 2 + 1 for k, v in obs[0].items()})
    dones = (torch.rand(n_envs, device=cuda_device) < 0.3).long()

    def run(step):
        pol.reset()
        outs = []
        for o in obs:  # three steps: from no state, from a state, after a reset of the done rows
            outs.append(step(o) + (pol.action_mean.clone(),))
            pol.reset(dones)
        return outs, pol.get_hidden_states()

    with torch.inference_mode():
        assert pol.memory_s.cell_ok(obs[0]["policy"]) == (rnn_type == "lstm")
        state = torch.cuda.get_rng_state(cuda_device)
        outs0, hid0 = run(lambda o: (pol.act(o), pol.evaluate(o)))
        after0 = torch.cuda.get_rng_state(cuda_device)
        torch.cuda.set_rng_state(state, cuda_device)
        outs1, hid1 = run(pol.act_and_evaluate)
        after1 = torch.cuda.get_rng_state(cuda_device)
    assert torch.equal(after0, after1)  # the same generator draws
    # the paired launches give the bits of the single ones (kernels.lstm_cell_pair, fused_mlp_forward_pair)
    for (a0, t0, m0), (a1, t1, m1) in zip(outs0, outs1):
        assert torch.equal(m1, m0) and torch.equal(a1, a0) and torch.equal(t1, t0)
        assert not torch.equal(a0, m0)
    h0, h1 = D.hidden_lists(hid0), D.hidden_lists(hid1)
    assert sorted(h0) == sorted(h1) and len(h0) == (2 if rnn_type == "lstm" else 1) * (2 if teacher_recurrent else 1)
    for k in h0:
        assert torch.equal(h0[k], h1[k]), k


def _params(dev, seed):
    torch.manual_seed(seed)
    shapes = [(128, 48), (128,), (64, 32), (64,), (4, 64), (4,), (7,)]
    return [torch.nn.Parameter(torch.randn(s, device=dev) * 0.1) for s in shapes]


@pytest.mark.parametrize("max_norm", [1e9, 0.5], ids=["inactive", "active"])
def test_subset_clip_matches_torch(max_norm, cuda_device):
    """clip_grad_norm_ on a subset plus Adam.step() (distillation.py:134-135).  What the existing optimizer tests
    require: without an active clip every parameter and both moments bit-equal to torch; with it, the clipped tensors
    within 1e-6 relative (the norm is accumulated in another order) -- and the tensors outside the clipped set, which
    no coefficient touches, bit-equal in either case."""
    from rsl_rl_amd import kernels

    ours = _params(cuda_device, 0)
    ref = [torch.nn.Parameter(p.detach().clone()) for p in ours]
    subset = [2, 3, 4, 5]  # in the middle of the list, as the student MLP between the memory and the rest
    opt_o = torch.optim.Adam(ours, lr=1e-3, fused=True)
    opt_r = torch.optim.Adam(ref, lr=1e-3, fused=True)
    fused = kernels.FusedClipAdam(opt_o, max_norm, clip_params=[ours[i] for i in subset])
    g = torch.Generator(device=cuda_device).manual_seed(1)
    for it in range(4):
        grads = [torch.randn(p.shape, device=cuda_device, generator=g) * (0.3 if it % 2 else 3.0) for p in ours]
        for po, pr, gr in zip(ours, ref, grads):
            po.grad, pr.grad = gr.clone(), gr.clone()
        fused.step()
        torch.nn.utils.clip_grad_norm_([ref[i] for i in subset], max_norm)
        opt_r.step()
        for i, (po, pr) in enumerate(zip(ours, ref)):
            so, sr = opt_o.state[po], opt_r.state[pr]
            pairs = [(po, pr), (so["exp_avg"], sr["exp_avg"]), (so["exp_avg_sq"], sr["exp_avg_sq"]),
                     (po.grad, pr.grad)]
            assert so["step"].item() == sr["step"].item() == it + 1
            if i not in subset or max_norm > 1e8:
                assert all(torch.equal(a, b) for a, b in pairs), (it, i)
                if i not in subset:
                    assert torch.equal(po.grad, grads[i]), (it, i)
            else:
                for a, b in pairs:
                    assert (a - b).abs().max() <= 1e-6 * b.abs().max(), (it, i)


@pytest.mark.parametrize("max_norm", [1e9, 0.5], ids=["inactive", "active"])
def test_default_clipped_set_is_every_tensor(max_norm, cuda_device):
    """clip_params=None and clip_params=<every parameter> are the same launch arguments' bits: no tensor is taken out
    (rslrl_adam_args_t.no_clip_mask 0)."""
    from rsl_rl_amd import kernels

    a, b = _params(cuda_device, 3), _params(cuda_device, 3)
    opt_a, opt_b = torch.optim.Adam(a, lr=1e-3, fused=True), torch.optim.Adam(b, lr=1e-3, fused=True)
    fa, fb = kernels.FusedClipAdam(opt_a, max_norm), kernels.FusedClipAdam(opt_b, max_norm, clip_params=list(b))
    g = torch.Generator(device=cuda_device).manual_seed(2)
    for _ in range(3):
        for pa, pb in zip(a, b):
            gr = torch.randn(pa.shape, device=cuda_device, generator=g) * 2.0
            pa.grad, pb.grad = gr.clone(), gr.clone()
        fa.step()
        fb.step()
        assert fa.args.no_clip_mask == fb.args.no_clip_mask == 0
    for pa, pb in zip(a, b):
        assert torch.equal(pa, pb) and torch.equal(pa.grad, pb.grad)
        assert torch.equal(opt_a.state[pa]["exp_avg_sq"], opt_b.state[pb]["exp_avg_sq"])


@pytest.mark.parametrize("kw", [dict(), dict(rnn_type="gru"), dict(hidden=32), dict(layers=2), dict(n_envs=100)],
                         ids=["lstm256", "gru", "h32", "two_layers", "n100"])
def test_any_memory_trains(kw, cuda_device, monkeypatch):
    """GRU or LSTM, any width, depth and number of envs: the update runs, moves the memory and the MLP and lowers the
    loss of the same rollout.  Only the one-layer LSTM of width 256 at a multiple of 64 envs takes the window path; a
    GRU, H 32, two layers and N = 100 fall back to the per-step path and still train."""
    from rsl_rl_amd.algorithms import Distillation

    windows = not kw
    calls = _count_backward_launches(monkeypatch)
    torch.manual_seed(2)
    N, T, Os, Ot, A = kw.pop("n_envs", 64), 6, 48, 64, 12
    pol = _policy(N, cuda_device, student_hidden_dims=[64, 64], teacher_hidden_dims=[64, 64], **kw)
    alg = Distillation(pol, gradient_length=3, num_learning_epochs=1, learning_rate=1e-3, max_grad_norm=1.0,
                       device=cuda_device)
    obs0 = {"policy": torch.zeros(N, Os), "teacher": torch.zeros(N, Ot)}
    alg.init_storage("distillation", N, T, obs0, [A])
    g = torch.Generator(device=cuda_device).manual_seed(4)

    def fill():
        st = alg.storage
        st.observations["policy"].copy_(torch.randn(T, N, Os, device=cuda_device, generator=g.manual_seed(4)))
        st.privileged_actions.copy_(torch.randn(T, N, A, device=cuda_device, generator=g))
        st.dones.copy_((torch.rand(T, N, 1, device=cuda_device, generator=g) < 0.1).to(torch.uint8))
        st.step = T

    before = {k: v.detach().clone() for k, v in pol.state_dict().items()}
    losses = []
    for _ in range(3):
        fill()
        alg.last_hidden_states = None
        losses.append(alg.update()["behavior"])
    assert np.all(np.isfinite(losses)) and losses[2] < losses[0], losses
    assert len(calls) == (3 * 2 * 3 if windows else 0)  # three updates of two full windows of three steps
    for k, v in pol.state_dict().items():
        assert torch.equal(v, before[k]) != k.startswith(("student.", "memory_s.")), k


def test_other_recurrent_policies_are_refused(cuda_device):
    from rsl_rl_amd.algorithms import Distillation
    from rsl_rl_amd.modules import StudentTeacher

    class Recurrent(StudentTeacher):
        is_recurrent = True

    obs0 = {"policy": torch.zeros(4, 16), "teacher": torch.zeros(4, 24)}
    pol = Recurrent(obs0, {"policy": ["policy"], "teacher": ["teacher"]}, 4, student_hidden_dims=[32],
                    teacher_hidden_dims=[32])
    alg = Distillation(pol, device=cuda_device)
    with pytest.raises(NotImplementedError, match=r"distillation\.py:112-113"):
        alg.update()
    assert alg.num_updates == 0


class _Writer:
    def __init__(self):
        self.scalars = {}

    def add_scalar(self, key, value, step):
        self.scalars.setdefault(key, []).append((step, float(value)))


def test_runner_end_to_end(cuda_device, tmp_path):
    from rsl_rl_amd.env import SyntheticVecEnv
    from rsl_rl_amd.modules import ActorCriticRecurrent, StudentTeacherRecurrent
    from rsl_rl_amd.runners import DistillationRunner

    dev = "cuda:0"
    N, T, Os, Ot, A = 128, 8, 16, 32, 4

    def make_runner(log_dir=None):
        env = SyntheticVecEnv(N, Os, A, device=dev, seed=3, num_privileged_obs=Ot)
        cfg = {
            "num_steps_per_env": T, "save_interval": 1,
            "obs_groups": {"policy": ["policy"], "teacher": ["privileged"]},
            "policy": {"class_name": "StudentTeacherRecurrent", "student_hidden_dims": [64, 64],
                       "teacher_hidden_dims": [64, 64], "student_obs_normalization": True, "rnn_type": "lstm",
                       "rnn_hidden_dim": 256, "teacher_recurrent": True},
            "algorithm": {"class_name": "Distillation", "gradient_length": 3, "num_learning_epochs": 2,
                          "learning_rate": 1e-3, "max_grad_norm": 1.0},
        }
        torch.manual_seed(11)
        return DistillationRunner(env, cfg, log_dir=log_dir, device=dev)

    # the teacher: the actor and its memory of a recurrent PPO-format checkpoint
    torch.manual_seed(7)
    ac = ActorCriticRecurrent({"policy": torch.zeros(N, Ot)}, {"policy": ["policy"], "critic": ["policy"]}, A,
                              actor_hidden_dims=[64, 64], critic_hidden_dims=[64, 64], rnn_hidden_dim=256)
    with torch.no_grad():
        ac.actor[-1].weight.mul_(8.0)  # a teacher with outputs of order one
    ppo_ckpt = str(tmp_path / "ppo_model.pt")
    torch.save({"model_state_dict": ac.state_dict(), "optimizer_state_dict": {}, "iter": 17, "infos": None}, ppo_ckpt)

    (tmp_path / "run").mkdir()
    runner = make_runner(log_dir=str(tmp_path / "run"))
    runner.writer = _Writer()
    pol = runner.alg.policy
    assert isinstance(pol, StudentTeacherRecurrent)
    with pytest.raises(ValueError, match="Teacher model parameters not loaded"):
        runner.learn(1)
    runner.load(ppo_ckpt)
    assert pol.loaded_teacher and runner.current_learning_iteration == 0  # an RL checkpoint does not resume
    assert torch.equal(pol.teacher[0].weight.cpu(), ac.actor[0].weight)
    assert torch.equal(pol.memory_t.rnn.weight_hh_l0.cpu(), ac.memory_a.rnn.weight_hh_l0)

    losses = []
    for _ in range(2):
        runner.learn(1)
        runner.current_learning_iteration += 1
        stats = runner.last_iteration_stats
        assert set(stats["loss_dict"]) == {"behavior"} and np.isfinite(stats["loss_dict"]["behavior"])
        losses.append(stats["loss_dict"]["behavior"])
    print("behavior loss per iteration:", losses)
    assert losses[1] <= losses[0], losses
    assert runner.alg.num_updates == 2
    assert pol.student_obs_normalizer.count.item() == 2 * T * N
    # the reference's protocol: every update() resets both memories to last_hidden_states, which for the teacher is
    # what the previous update() left -- None from the first one on
    hs, ht = pol.get_hidden_states()
    assert hs[0].shape == (1, N, 256) and ht is None

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
