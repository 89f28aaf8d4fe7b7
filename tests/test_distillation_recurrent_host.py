"""Recurrent distillation without a GPU: StudentTeacherRecurrent's checkpoint surface against the reference's recorded
orders, its constructor's rules, load_state_dict's three branches (with a recurrent PPO fixture as the teacher), the
hidden-state protocol on a CPU module against hand-computed states, the runner's class table, the clipped set of the
fused optimizer step (validated before any launch) and the fixtures."""

import ctypes
import os
import warnings

import pytest
import torch

import drec_fixtures as D
import recurrent_fixtures as RF

META = D.load_meta()
OBS0 = {"policy": torch.zeros(3, 16), "teacher": torch.zeros(3, 24)}
GROUPS = {"policy": ["policy"], "teacher": ["teacher"]}


def _policy(**kw):
    from rsl_rl_amd.modules import StudentTeacherRecurrent

    kw.setdefault("student_hidden_dims", [64, 64])
    kw.setdefault("teacher_hidden_dims", [64, 64])
    kw.setdefault("rnn_hidden_dim", 32)
    return StudentTeacherRecurrent(OBS0, GROUPS, 4, **kw)


@pytest.mark.parametrize("std_type", ["scalar", "log"])
@pytest.mark.parametrize("teacher_recurrent", [False, True])
def test_state_dict_key_order(std_type, teacher_recurrent):
    ref = META["state_dict_keys"][f"{std_type}_{'recurrent' if teacher_recurrent else 'plain'}"]
    pol = _policy(noise_std_type=std_type, student_obs_normalization=True, teacher_obs_normalization=True,
                  teacher_recurrent=teacher_recurrent)
    sd = pol.state_dict()
    assert list(sd.keys()) == ref["state_dict"]
    assert [n for n, _ in pol.named_parameters()] == ref["parameters"]
    assert {k: list(v.shape) for k, v in sd.items()} == ref["shapes"]
    assert ref["state_dict"][0] == ("std" if std_type == "scalar" else "log_std")
    keys = ref["state_dict"]
    assert keys.index("memory_s.rnn.weight_ih_l0") < keys.index("student.0.weight") < keys.index("teacher.0.weight")
    assert ("memory_t.rnn.weight_ih_l0" in keys) == teacher_recurrent
    if teacher_recurrent:
        assert keys.index("student_obs_normalizer._mean") < keys.index("memory_t.rnn.weight_ih_l0")
        # the reference's construction: a recurrent teacher's normaliser is sized rnn_hidden_dim
        assert ref["shapes"]["teacher_obs_normalizer._mean"][-1] == 32
    else:
        assert ref["shapes"]["teacher_obs_normalizer._mean"][-1] == 24


def test_rnn_hidden_size_is_deprecated():
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        pol = _policy(rnn_hidden_dim=256, rnn_hidden_size=12, student_hidden_dims=[8], teacher_hidden_dims=[8])
    assert any(issubclass(x.category, DeprecationWarning) for x in w)
    assert pol.memory_s.rnn.hidden_size == 12 and pol.student[0].in_features == 12
    with warnings.catch_warnings(record=True):
        warnings.simplefilter("always")
        pol = _policy(rnn_hidden_dim=20, rnn_hidden_size=12)  # the new name wins when both are given
    assert pol.memory_s.rnn.hidden_size == 20


def test_unknown_std_type():
    with pytest.raises(ValueError, match="Unknown standard deviation type"):
        _policy(noise_std_type="softplus")


def test_load_state_dict_branches():
    from rsl_rl_amd.modules import ActorCriticRecurrent

    # 1. a recurrent RL checkpoint: the actor, its normaliser and memory_a become the teacher; no resume
    torch.manual_seed(3)
    ac = ActorCriticRecurrent({"policy": torch.zeros(3, 24)}, {"policy": ["policy"], "critic": ["policy"]}, 4,
                              actor_hidden_dims=[64, 64], critic_hidden_dims=[64, 64], rnn_hidden_dim=32)
    pol = _policy(teacher_recurrent=True)
    student_before = {k: v.clone() for k, v in pol.state_dict().items() if k.startswith(("student.", "memory_s."))}
    assert pol.loaded_teacher is False
    assert pol.load_state_dict(ac.state_dict()) is False
    assert pol.loaded_teacher is True
    for k, v in ac.actor.state_dict().items():
        assert torch.equal(pol.teacher.state_dict()[k], v), k
    for k, v in ac.memory_a.state_dict().items():
        assert torch.equal(pol.memory_t.state_dict()[k], v), k
    for k, v in student_before.items():
        assert torch.equal(pol.state_dict()[k], v), k
    assert not pol.teacher.training and not pol.teacher_obs_normalizer.training
    # the teacher then acts as the checkpoint's actor did, step after step
    x = [{"policy": torch.randn(3, 16), "teacher": torch.randn(3, 24)} for _ in range(2)]
    for o in x:
        assert torch.equal(pol.evaluate(o), ac.act_inference({"policy": o["teacher"]}))
    # a feed-forward teacher ignores the checkpoint's memory
    ff = _policy(teacher_recurrent=False, teacher_hidden_dims=[64, 64])
    with pytest.raises(RuntimeError, match="size mismatch"):
        ff.load_state_dict(ac.state_dict())  # the actor's first layer is rnn_hidden_dim wide, not 24

    # 2. a distillation checkpoint: everything loads; training resumes
    other = _policy(teacher_recurrent=True)
    assert other.load_state_dict(pol.state_dict()) is True
    assert other.loaded_teacher is True
    for k, v in pol.state_dict().items():
        assert torch.equal(other.state_dict()[k], v), k

    # 3. neither
    with pytest.raises(ValueError, match="does not contain student or teacher parameters"):
        _policy().load_state_dict({"critic.0.weight": torch.zeros(1)})


def test_recurrent_ppo_fixture_loads_as_the_teacher():
    """The reference's own recurrent PPO parameters (the rec_a fixture): actor.* -> teacher.*, memory_a.* ->
    memory_t.*, the critic's are dropped."""
    from rsl_rl_amd.modules import StudentTeacherRecurrent

    meta = RF.load_meta()["rec_a"]
    z = RF.Arrays(meta["files"])
    sd = {k[len("r0/init/"):]: torch.from_numpy(z[k]) for k in z.files if k.startswith("r0/init/")}
    kw = RF.policy_kwargs(meta)
    obs0 = {"policy": torch.zeros(2, 16), "teacher": torch.zeros(2, meta["O"])}
    pol = StudentTeacherRecurrent(obs0, GROUPS, meta["A"], teacher_hidden_dims=kw["actor_hidden_dims"],
                                  student_hidden_dims=[32], teacher_recurrent=True,
                                  **{k: kw[k] for k in ("rnn_type", "rnn_hidden_dim", "rnn_num_layers") if k in kw})
    assert pol.load_state_dict(sd, strict=True) is False and pol.loaded_teacher
    for k, v in sd.items():
        if k.startswith("actor."):
            assert torch.equal(pol.state_dict()["teacher." + k[len("actor."):]], v), k
        if k.startswith("memory_a."):
            assert torch.equal(pol.state_dict()["memory_t." + k[len("memory_a."):]], v), k
    assert any(k.startswith("memory_a.") for k in sd)


@pytest.mark.parametrize("rnn_type", ["lstm", "gru"])
def test_hidden_state_protocol(rnn_type):
    pol = _policy(rnn_type=rnn_type, teacher_recurrent=True, rnn_hidden_dim=5)
    assert pol.is_recurrent and pol.get_hidden_states() == (None, None)
    pol.reset(torch.tensor([1, 0, 0]))  # nothing to reset yet
    n = 2 if rnn_type == "lstm" else 1
    mk = lambda v: tuple(torch.full((1, 3, 5), v + i) for i in range(n)) if n == 2 else torch.full((1, 3, 5), v)  # noqa: E731
    hs, ht = mk(1.0), mk(10.0)
    pol.reset(hidden_states=(hs, ht))
    got_s, got_t = pol.get_hidden_states()
    assert got_s is hs and got_t is ht  # handed over as they are, as the reference does
    # done rows become exactly 0, the others keep their values -- in both memories
    pol.reset(torch.tensor([0, 1, 0]))
    for x, v in ((pol.memory_s.hidden_states, 1.0), (pol.memory_t.hidden_states, 10.0)):
        for i, s in enumerate(x if n == 2 else (x,)):
            want = torch.full((1, 3, 5), v + i)
            want[:, 1] = 0.0
            assert torch.equal(s, want)
    # detach: all rows, or the done rows only (values unchanged, the other rows keep their graph)
    w = torch.ones(1, 3, 5, requires_grad=True)
    live = tuple(w * (2.0 + i) for i in range(n)) if n == 2 else w * 2.0
    pol.reset(hidden_states=(live, None))
    pol.detach_hidden_states(torch.tensor([1, 0, 0]))
    s0 = pol.memory_s.hidden_states[0] if n == 2 else pol.memory_s.hidden_states
    assert torch.equal(s0, torch.full((1, 3, 5), 2.0)) and s0.requires_grad
    s0.sum().backward()
    assert torch.equal(w.grad[0, 0], torch.zeros(5)) and torch.equal(w.grad[0, 1], torch.full((5,), 2.0))
    pol.detach_hidden_states()
    s0 = pol.memory_s.hidden_states[0] if n == 2 else pol.memory_s.hidden_states
    assert not s0.requires_grad
    # a feed-forward teacher has no second state
    ff = _policy(rnn_type=rnn_type)
    ff.reset(hidden_states=(hs, None))
    assert ff.get_hidden_states()[1] is None and not hasattr(ff, "memory_t")
    ff.reset()
    assert ff.get_hidden_states() == (None, None)


def test_steps_follow_the_memory():
    """act_inference / evaluate / act_and_evaluate on a CPU module: one memory step each, the teacher's memory under
    no_grad and in eval mode; act_and_evaluate is act then evaluate."""
    torch.manual_seed(1)
    pol = _policy(teacher_recurrent=True, student_obs_normalization=True)
    pol.train()
    obs = {"policy": torch.randn(3, 16), "teacher": torch.randn(3, 24)}
    pol.update_normalization(obs)
    out = pol.act_inference(obs)
    h, c = pol.memory_s.hidden_states
    want, _ = pol.memory_s.rnn(pol.student_obs_normalizer(obs["policy"]).unsqueeze(0))
    assert torch.equal(h, want) and torch.equal(out, pol.student(want.squeeze(0))) and out.requires_grad
    t = pol.evaluate(obs)
    assert not t.requires_grad and not pol.memory_t.training and pol.memory_s.training
    assert not pol.memory_t.hidden_states[0].requires_grad
    pol.reset()
    torch.manual_seed(2)
    a0, t0 = pol.act(obs), pol.evaluate(obs)
    st0 = pol.get_hidden_states()
    pol.reset()
    torch.manual_seed(2)
    a1, t1 = pol.act_and_evaluate(obs)
    assert torch.equal(a0, a1) and torch.equal(t0, t1)
    for x, y in zip(D.hidden_lists(st0).values(), D.hidden_lists(pol.get_hidden_states()).values()):
        assert torch.equal(x, y)


def test_train_keeps_teacher_in_eval_mode():
    pol = _policy(student_obs_normalization=True, teacher_obs_normalization=True)
    assert pol.train() is pol
    assert pol.training and pol.student.training and pol.memory_s.training and pol.student_obs_normalizer.training
    assert not pol.teacher.training and not pol.teacher_obs_normalizer.training
    pol.eval()
    pol.train(True)
    assert not pol.teacher.training and not pol.teacher_obs_normalizer.training


def test_class_names_resolve():
    import rsl_rl_amd.modules as M
    from rsl_rl_amd.runners.on_policy_runner import _resolve_class

    assert _resolve_class("StudentTeacherRecurrent") is M.StudentTeacherRecurrent
    assert "StudentTeacherRecurrent" in M.__all__


def test_distillation_accepts_the_class_and_refuses_other_recurrent_policies():
    from rsl_rl_amd.algorithms import Distillation
    from rsl_rl_amd.modules import StudentTeacher

    alg = Distillation(_policy(), max_grad_norm=1.0, device="cpu")
    assert alg._clip_adam is None  # a CPU device keeps torch's clip over policy.student and optimizer.step()
    alg.init_storage("distillation", 3, 2, OBS0, [4])
    with pytest.raises(RuntimeError, match="no CPU fallback"):  # past the refusal: the loss kernel needs the device
        alg.update()
    assert alg.num_updates == 1

    class Recurrent(StudentTeacher):
        is_recurrent = True

    other = Distillation(Recurrent(OBS0, GROUPS, 4, student_hidden_dims=[32], teacher_hidden_dims=[32]), device="cpu")
    with pytest.raises(NotImplementedError, match=r"distillation\.py:112-113"):
        other.update()
    assert other.num_updates == 0


def test_clipped_set_is_validated_before_any_launch():
    from rsl_rl_amd import _lib

    L = _lib.lib()
    assert L.rslrl_abi_version() == _lib.ABI_VERSION >= 26
    p = 4096  # never dereferenced: every call below is rejected on its arguments
    ws_bytes = L.rslrl_adam_workspace_bytes()

    def args(n, mask):
        a = _lib.AdamArgs()
        a.n, a.max_grad_norm, a.lr, a.beta1, a.beta2, a.eps = n, 1.0, 1e-3, 0.9, 0.999, 1e-8
        for i in range(n):
            t = a.t[i]
            t.param, t.grad, t.exp_avg, t.exp_avg_sq, t.step, t.numel = p, p, p, p, p, 8
        a.no_clip_mask = mask
        return a

    assert ctypes.sizeof(_lib.AdamArgs) % 8 == 0
    assert _lib.AdamArgs.no_clip_mask.offset == _lib.AdamArgs.t.offset + 48 * _lib.ADAM_MAX_TENSORS
    # a bit that names a tensor beyond n
    assert L.rslrl_clip_adam_step(ctypes.byref(args(3, 0b1000)), p, ws_bytes, None) == _lib.E_INVALID_ARGUMENT
    assert L.rslrl_clip_adam_step(ctypes.byref(args(2, 1 << 23)), p, ws_bytes, None) == _lib.E_INVALID_ARGUMENT
    tail = _lib.PpoTail()
    tail.stats = p
    assert L.rslrl_clip_adam_step_tail(ctypes.byref(args(3, 0b1000)), ctypes.byref(tail), p, ws_bytes,
                                       None) == _lib.E_INVALID_ARGUMENT
    # a valid mask passes this check and is stopped by the next one (the workspace), still before a launch
    assert L.rslrl_clip_adam_step(ctypes.byref(args(3, 0b101)), p, 0, None) == -2


def test_fixtures_present():
    for case in ("a", "b", "c"):
        m = META[case]
        assert m["files"] and all(f.startswith("drec_") for f in m["files"])
        for f in m["files"]:
            path = os.path.join(D.GOLDEN, f)
            assert os.path.exists(path), path
            assert os.path.getsize(path) < (1 << 20), path
        r = m["ranks"][0]
        assert r["num_steps"] == (m["E"] * m["T"]) // m["G"] == 5 and (m["E"] * m["T"]) % m["G"] == 1
        assert 0.07 <= r["done_fraction"] <= 0.14 and r["grad_norms"]["memory"] > 0
        z = D.load_arrays(m)
        d = z["r0/dones"]
        assert d.shape == (m["T"], m["N"]) and not d[:, 0].any() and d[-1].any() and d[3, 3] and d[4, 3]
        assert ("r0/last_hidden/s0" in z.files) == m["seeded_state"]
    assert META["a"]["rnn_type"] == "lstm" and META["b"]["rnn_type"] == "gru" and META["b"]["rnn_num_layers"] == 2
    assert META["b"]["teacher_recurrent"] and META["b"]["max_grad_norm"] is None
    for case in ("a", "c"):
        n = META[case]["ranks"][0]["grad_norms"]
        assert n["mlp"] > 1.0 and abs(n["clip_saw"] - n["mlp"]) <= 1e-4 * n["mlp"]
    n = META["c"]["ranks"][0]["grad_norms"]
    assert META["c"]["rnn_hidden_dim"] == 256 and n["full"] > 1.01 * n["mlp"]
    assert set(META["c"]["ulp_sensitivity"]) >= {"memory_s.rnn.weight_hh_l0", "student.0.weight", "hidden_final/s0"}


def test_lstm_train_entry_points_validate_before_any_launch():
    from rsl_rl_amd import _lib

    L = _lib.lib()
    p = 4096  # never dereferenced: every call below is rejected on its arguments

    def train(M=64, **kw):
        cell = dict(x=p, h=p * 2, c=p * 3, image=p * 4, b_ih=p * 5, b_hh=p * 6, h_out=p * 7, c_out=p * 8, D=48,
                    hidden=256, layers=1, reserved=0)
        outer = dict(gates=p * 9, reset=p * 10, gate_stride=M * 256)
        for k, v in kw.items():
            (outer if k in outer else cell)[k] = v
        return _lib.LstmTrain(cell=_lib.LstmCell(**cell), **outer)

    assert L.rslrl_lstm_cell_train(None, 64, None) == _lib.E_INVALID_ARGUMENT
    for kw, M in ((dict(hidden=128), 64), (dict(D=40), 64), (dict(), 100), (dict(layers=2), 64), (dict(D=272), 64),
                  (dict(), 0)):
        assert L.rslrl_lstm_cell_train(ctypes.byref(train(**kw)), M, None) == _lib.E_UNSUPPORTED, (kw, M)
    for kw in (dict(x=None), dict(image=None), dict(h_out=None), dict(gates=None), dict(gate_stride=64 * 256 - 4),
               dict(h_out=p * 2)):
        assert L.rslrl_lstm_cell_train(ctypes.byref(train(**kw)), 64, None) == _lib.E_INVALID_ARGUMENT, kw
    assert L.rslrl_lstm_cell_train(ctypes.byref(train(gates=p * 9 + 4)), 64, None) == -4  # misaligned
    assert L.rslrl_lstm_cell_train(ctypes.byref(train(gate_stride=64 * 256 + 2)), 64, None) == -4

    def bwd(M=64, **kw):
        base = dict(dh=p, dg_next=p * 2, dc_next=p * 3, reset_next=p * 4, gates=p * 5, c_out=p * 6, c_prev=p * 7,
                    reset_cur=p * 8, whh_t_image=p * 9, dg=p * 10, dc_prev=p * 11, gate_stride=M * 256,
                    next_stride=M * 256, hidden=256, layers=1)
        base.update(kw)
        return _lib.LstmBwd(**base)

    assert L.rslrl_lstm_cell_bwd(None, 64, None) == _lib.E_INVALID_ARGUMENT
    for kw, M in ((dict(hidden=128), 64), (dict(layers=2), 64), (dict(), 100), (dict(), 0)):
        assert L.rslrl_lstm_cell_bwd(ctypes.byref(bwd(**kw)), M, None) == _lib.E_UNSUPPORTED, (kw, M)
    for kw in (dict(dh=None), dict(gates=None), dict(c_out=None), dict(dg=None), dict(dc_prev=None),
               dict(whh_t_image=None), dict(gate_stride=64), dict(next_stride=64), dict(dg=p * 2)):
        assert L.rslrl_lstm_cell_bwd(ctypes.byref(bwd(**kw)), 64, None) == _lib.E_INVALID_ARGUMENT, kw
    assert L.rslrl_lstm_cell_bwd(ctypes.byref(bwd(dh=p + 4)), 64, None) == -4  # misaligned
    assert L.rslrl_lstm_whh_t_image_bytes() == L.rslrl_linear_bimage_bytes(1024)
    assert L.rslrl_lstm_prepare_whh_t_image(p, 128, p, None) == _lib.E_UNSUPPORTED
    assert L.rslrl_lstm_prepare_whh_t_image(None, 256, p, None) == _lib.E_INVALID_ARGUMENT
    assert L.rslrl_lstm_prepare_whh_t_image(p, 256, p + 4, None) == -4


def test_recurrent_window_plan_against_the_reference_loop():
    """Where the chain is cut, against a brute-force walk of the reference's loop (distillation.py:111-141): a graph
    edge runs from step k to k + 1 unless an epoch started in between (reset(hidden_states=...) +
    detach_hidden_states()) or a window ended there (detach_hidden_states() after the optimizer step)."""
    from rsl_rl_amd.algorithms import distillation_windows, recurrent_window_plan

    for T, E, G in [(8, 2, 3), (24, 1, 15), (4, 1, 15), (5, 3, 5), (2, 4, 5), (3, 3, 2), (1, 4, 3)]:
        walk, cnt = [], 0  # per global step: (t, the state was restarted before it, an edge leaves it)
        for _ in range(E):
            for t in range(T):
                cnt += 1
                walk.append([t, t == 0, True])
                if cnt % G == 0:
                    walk[-1][2] = False  # the window ends: detach
            walk[-1][2] = False  # the next epoch restarts the state
        walk[-1][2] = False
        # a trailing window's graph is never differentiated, but its steps still chain
        got = [list(p) for steps, _ in distillation_windows(T, E, G) for p in recurrent_window_plan(steps)]
        full_steps = (E * T) // G * G
        for k, (w, g) in enumerate(zip(walk, got)):
            assert w[:2] == g[:2], (T, E, G, k)
            if k < full_steps:
                assert w[2] == g[2], (T, E, G, k, w, g)
        assert len(walk) == len(got) == E * T
