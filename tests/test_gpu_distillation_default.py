"""Distillation.update() of the students that take the window-batched update since DESIGN.md §23 -- a wide + ragged
stack (distill_d: obs 45, [320, 260, 64]), a ragged narrow one (distill_e: obs 19, [64, 64]), a GRU-256 student
(drec_e) and a GRU-256 student at obs 45 in front of [320, 260, 64] with a GRU teacher (drec_f) -- against the
reference's own update (tests/golden/make_golden_distillation_default.py), each on the window path and, with
RSLRL_DISTILL_FUSED=0, on the per-step path; which path ran (launch spies), the gradient arena, the one read-back, and
the paired rollout step of a GRU student with a GRU teacher.

Tolerances: those of tests/test_gpu_distillation.py (feed-forward) and tests/test_gpu_distillation_recurrent.py
(recurrent), unchanged -- the schedule and the lr trace exact, loss_dict and every step loss rtol 1e-4, the first
gradient within 1e-5 of each tensor's max, parameters within the reference's own one-ulp sensitivity envelope
(2 * sens + 1e-4 of the distance moved) where a trained layer is 256 wide or wider (distill_d, drec_e, drec_f) and
within atol 2e-5 at width 64 (distill_e); for the recurrent cases twice torch's own GPU autograd of the same update
where the envelope is missed, and the hidden states after the update."""

import json
import os

import numpy as np
import pytest
import torch

import distill_fixtures as DF
import drec_fixtures as D
import recurrent_fixtures as RF
import test_gpu_distillation_recurrent as TR
from update_fixtures import check_update, param_errors

pytestmark = pytest.mark.gpu

with open(os.path.join(RF.GOLDEN, "golden_distillation_default.json")) as _f:
    META = json.load(_f)
FF, REC = ("distill_d", "distill_e"), ("drec_e", "drec_f")


def _spy(monkeypatch, module, name, log):
    real = getattr(module, name)

    def counted(*a, **k):
        log.append((a, k))
        return real(*a, **k)

    monkeypatch.setattr(module, name, counted)


def _in_arena(alg, params):
    flat = alg._arena.flat
    return all(flat.data_ptr() <= p.grad.data_ptr() < flat.data_ptr() + 4 * flat.numel() for p in params)


@pytest.mark.parametrize("fused", [True, False], ids=["windows", "per_step"])
@pytest.mark.parametrize("case", FF)
def test_feed_forward_update_matches_reference(case, fused, cuda_device, monkeypatch):
    from rsl_rl_amd.algorithms import Distillation
    from rsl_rl_amd.networks import fused_mlp

    monkeypatch.setenv("RSLRL_DISTILL_FUSED", "1" if fused else "0")
    meta = META[case]
    z = RF.Arrays(meta["files"])
    alg, pol = DF.build_distillation(z, meta, 0, "cuda:0")
    assert pol.student._ragged and not pol.student._fused and not fused_mlp.fusable_structure(pol.student)
    assert fused_mlp.ragged_wide_stack(pol.student) is (case == "distill_d")
    assert alg._fused_ok() is fused  # (True fails on the parent commit: a ragged student took the per-step loop)
    steps = []
    _spy(monkeypatch, Distillation, "_mlp_step", steps)
    wide0, ragged0, copies0 = fused_mlp.wide_launches, fused_mlp.ragged_launches, fused_mlp.ragged_realign_copies
    before = {k: v.detach().clone() for k, v in pol.state_dict().items()}
    out = DF.run_recorded_update(alg)
    ref = meta["ranks"][0]
    # which path ran: one window step per optimizer step, or none; both run the first layer on the ragged kernels (the
    # per-step loop under autograd) and distill_d its wide layers on the wide ones; no window's rows were realigned
    assert len(steps) == (ref["num_steps"] if fused else 0)
    assert fused_mlp.ragged_launches > ragged0
    assert (fused_mlp.wide_launches > wide0) is (case == "distill_d")
    assert fused_mlp.ragged_realign_copies == copies0

    assert len(out["lr_trace"]) == ref["num_steps"] == alg.optimizer.state[pol.student[0].weight]["step"].item() == 5
    ref_steps = z["r0/step_losses"]
    ours = np.asarray(out["step_losses"])
    assert ours.shape == ref_steps.shape == (meta["E"] * meta["T"],)
    print(case, "step losses: max rel err", np.max(np.abs(ours - ref_steps) / np.abs(ref_steps)))
    assert np.all(np.abs(ours - ref_steps) <= 1e-4 * np.abs(ref_steps)), (ours, ref_steps)
    assert set(out["loss"]) == {"behavior"}
    check_update(out, z, meta, 0, mode=case + (" windows" if fused else " per_step"))

    ref_grad = torch.from_numpy(z["r0/grad_mb0"]).double()
    off = 0
    for name, p in pol.student.named_parameters():
        r = ref_grad[off:off + p.numel()]
        o = out["grad_mb0"][off:off + p.numel()].double()
        off += p.numel()
        assert (o - r).abs().max().item() <= 1e-5 * r.abs().max().item(), name
    assert off == ref_grad.numel()

    for k, v in pol.state_dict().items():
        assert torch.equal(v, before[k]) != k.startswith("student."), k
    for name, p in pol.named_parameters():
        assert (p.grad is not None) == name.startswith("student."), name
    if fused:  # every gradient is a view of the one arena the multi-GPU all-reduce runs on
        assert _in_arena(alg, list(pol.student.parameters()))
        assert alg._arena.flat.numel() == sum(p.numel() for p in pol.student.parameters())
    assert alg.num_updates == 1 and alg.storage.step == 0


@pytest.mark.parametrize("fused", [True, False], ids=["windows", "per_step"])
@pytest.mark.parametrize("case", REC)
def test_gru_update_matches_reference(case, fused, cuda_device, monkeypatch):
    from rsl_rl_amd import kernels
    from rsl_rl_amd.networks import fused_mlp

    monkeypatch.setenv("RSLRL_DISTILL_FUSED", "1" if fused else "0")
    meta = META[case]
    z = D.load_arrays(meta)
    alg, pol = D.build_distillation(z, meta, "cuda:0")
    assert isinstance(pol.memory_s.rnn, torch.nn.GRU) and pol.teacher_recurrent is (case == "drec_f")
    assert pol.student._wide is (case == "drec_f")
    assert alg._clip_adam is not None and not alg._fused_ok()
    assert alg._fused_recurrent_ok() is fused  # (True fails on the parent commit: a GRU took the per-step loop)
    fwd, bwd, lstm_bwd = [], [], []
    _spy(monkeypatch, kernels, "gru_cell_train", fwd)
    _spy(monkeypatch, kernels, "gru_cell_bwd", bwd)
    _spy(monkeypatch, kernels, "lstm_cell_bwd", lstm_bwd)
    wide0, ragged0 = fused_mlp.wide_launches, fused_mlp.ragged_launches
    before = {k: v.detach().clone() for k, v in pol.state_dict().items()}
    base = TR._Baseline(z, meta, pol, "cuda:0")
    out = D.run_recorded_update(alg)
    ref = meta["ranks"][0]
    # the window path really ran: a forward cell step per stored step of every epoch, a reverse one per step of each
    # of the five full windows -- or neither
    assert len(bwd) == (ref["num_steps"] * meta["G"] if fused else 0) and not lstm_bwd
    assert len(fwd) == (meta["E"] * meta["T"] if fused else 0)
    assert all(a[0].shape == (meta["N"], meta["O_student"]) for a, _ in fwd)
    if case == "drec_f":
        assert fused_mlp.wide_launches > wide0  # the MLP behind the memory, on both paths
        assert (fused_mlp.ragged_launches > ragged0) is fused  # dW_ih against the 45-wide observations
    if fused:
        flat = alg._arena.flat
        with_grad = [p for p in pol.parameters() if p.grad is not None]
        assert len(with_grad) == len(alg._arena.params) == len(D.trained_names(pol))
        assert all(p is q and p.grad.data_ptr() == v.data_ptr()
                   for p, q, v in zip(with_grad, alg._arena.params, alg._arena.views))
        assert _in_arena(alg, with_grad) and flat.numel() == sum(p.numel() for p in with_grad)

    assert out["lr_trace"] == ref["lr_trace"] and out["lr"] == ref["final_lr"]
    assert len(out["lr_trace"]) == ref["num_steps"] == alg.optimizer.state[pol.student[0].weight]["step"].item()
    ref_steps = z["r0/step_losses"]
    ours = np.asarray(out["step_losses"])
    assert ours.shape == ref_steps.shape == (meta["E"] * meta["T"],)
    print(case, "step losses: max rel err", np.max(np.abs(ours - ref_steps) / np.abs(ref_steps)))
    assert np.all(np.abs(ours - ref_steps) <= 1e-4 * np.abs(ref_steps)), (ours, ref_steps)
    v = ref["loss_dict"]["behavior"]
    assert set(out["loss"]) == {"behavior"} and abs(out["loss"]["behavior"] - v) <= 1e-4 * abs(v) + 1e-6

    names = D.trained_names(pol)
    assert sorted(out["grads"]) == sorted(names) and any(n.startswith("memory_s.") for n in names)
    gerr = {}
    for n in names:
        r = torch.from_numpy(z["r0/grad_mb0/" + n]).double()
        gerr[n] = (out["grads"][n].double() - r).abs().max().item() / r.abs().max().item()
    print(case, "first gradient, max err / max:", {k: f"{e:.1e}" for k, e in gerr.items()})
    assert all(e <= 1e-5 for e in gerr.values()), gerr

    errs = param_errors(out["final"], z, "r0/")
    print(case, "param errors (max abs / ||d|| over ||moved||):", {k: f"{a:.1e}/{m:.1e}" for k, (a, m) in errs.items()})
    assert sorted(errs) == sorted(names)
    sens = meta["ulp_sensitivity"]
    for name, (abs_err, rel_moved) in errs.items():
        if not rel_moved <= 2 * sens[name] + 1e-4:
            b_abs, b_rel = base.get()[0][name]
            assert rel_moved <= 2 * b_rel, (name, abs_err, rel_moved, b_abs, b_rel)

    hid = D.hidden_lists(out["hidden"])
    assert sorted(hid) == sorted(k[len("r0/hidden_final/"):] for k in z.files if k.startswith("r0/hidden_final/"))
    assert sorted(hid) == (["s0", "t0"] if case == "drec_f" else ["s0"])
    for k, h in hid.items():
        r = torch.from_numpy(z["r0/hidden_final/" + k])
        if k.startswith("t"):  # the teacher's memory is only ever zeroed
            assert torch.equal(h, r), k
            continue
        d = (h - r).abs().max().item()
        tol = 2 * sens["hidden_final/" + k] + 1e-4 * r.abs().max().item()
        print(case, "hidden state", k, "max err", d, "tolerance", tol)
        if d > tol:
            assert d <= 2 * base.get()[1][k], (k, d, base.get()[1][k])
    done_last = torch.from_numpy(z["r0/dones"])[-1] == 1
    assert (hid["s0"][:, done_last] == 0).all() and (hid["s0"][:, ~done_last] != 0).any()

    for k, v in pol.state_dict().items():
        assert torch.equal(v, before[k]) != k.startswith(("student.", "memory_s.")), k
    for name, p in pol.named_parameters():
        assert (p.grad is not None) == (name in names), name
        assert (len(alg.optimizer.state.get(p, {})) > 0) == (name in names), name
    assert alg.num_updates == 1 and alg.storage.step == 0
    assert all(torch.equal(a, b) for a, b in zip(D.hidden_lists(alg.last_hidden_states).values(), hid.values()))


@pytest.mark.parametrize("case", FF + REC)
def test_update_reads_the_device_back_once(case, cuda_device):
    meta = META[case]

    def build():
        if case in FF:
            return DF.build_distillation(RF.Arrays(meta["files"]), meta, 0, "cuda:0")[0]
        return D.build_distillation(D.load_arrays(meta), meta, "cuda:0")[0]

    build().update()  # warm-up: allocations, library initialisation
    alg = build()
    assert alg._fused_ok() if case in FF else alg._fused_recurrent_ok()
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
        loss = alg.update()
    finally:
        torch.cuda.set_sync_debug_mode("default")
        torch.Tensor.tolist = tolist
    assert reads == [meta["E"] * meta["T"]], reads
    assert np.isfinite(loss["behavior"])


def test_knobs_keep_the_per_step_path(cuda_device, monkeypatch):
    """RSLRL_GRU_CELL=0 for a GRU student; a wide / ragged student outside x6 arithmetic."""
    from rsl_rl_amd.networks import fused_mlp

    meta = META["drec_e"]
    alg, _ = D.build_distillation(D.load_arrays(meta), meta, "cuda:0")
    assert alg._fused_recurrent_ok()
    monkeypatch.setenv("RSLRL_GRU_CELL", "0")
    assert not alg._fused_recurrent_ok()
    meta = META["distill_d"]
    alg, _ = DF.build_distillation(RF.Arrays(meta["files"]), meta, 0, "cuda:0")
    assert alg._fused_ok()
    mode = fused_mlp.set_gemm_mode(fused_mlp.GEMM_F32)
    try:
        assert not alg._fused_ok()
    finally:
        fused_mlp.set_gemm_mode(mode)
    assert alg._fused_ok()


def test_act_and_evaluate_pairs_two_grus(cuda_device, monkeypatch):
    """A GRU student and a GRU teacher: one gru_cell_pair launch per rollout step, the bits of act() then evaluate()."""
    from rsl_rl_amd import kernels

    n_envs = 128
    torch.manual_seed(5)
    pol = TR._policy(n_envs, cuda_device, "gru", 256, teacher_recurrent=True, student_obs_normalization=True)
    obs = [{"policy": torch.randn(n_envs, 48, device=cuda_device), "teacher": torch.randn(n_envs, 64,
                                                                                        device=cuda_device)}
           for _ in range(3)]
    pol.update_normalization({k: v * 2 + 1 for k, v in obs[0].items()})
    dones = (torch.rand(n_envs, device=cuda_device) < 0.3).long()
    pairs = []
    _spy(monkeypatch, kernels, "gru_cell_pair", pairs)

    def run(step):
        pol.reset()
        outs = []
        for o in obs:  # three steps: from no state, from a state, after a reset of the done rows
            outs.append(step(o) + (pol.action_mean.clone(),))
            pol.reset(dones)
        return outs, pol.get_hidden_states()

    with torch.inference_mode():
        assert pol.memory_s.gru_cell_ok(obs[0]["policy"]) and pol.memory_t.gru_cell_ok(obs[0]["teacher"])
        state = torch.cuda.get_rng_state(cuda_device)
        outs0, hid0 = run(lambda o: (pol.act(o), pol.evaluate(o)))
        after0 = torch.cuda.get_rng_state(cuda_device)
        assert not pairs
        torch.cuda.set_rng_state(state, cuda_device)
        outs1, hid1 = run(pol.act_and_evaluate)
        after1 = torch.cuda.get_rng_state(cuda_device)
    assert len(pairs) == len(obs)
    assert torch.equal(after0, after1)  # the same generator draws
    for (a0, t0, m0), (a1, t1, m1) in zip(outs0, outs1):
        assert torch.equal(m1, m0) and torch.equal(a1, a0) and torch.equal(t1, t0)
        assert not torch.equal(a0, m0)
    h0, h1 = D.hidden_lists(hid0), D.hidden_lists(hid1)
    assert sorted(h0) == sorted(h1) == ["s0", "t0"]
    for k in h0:
        assert torch.equal(h0[k], h1[k]) and h0[k].shape == (1, n_envs, 256), k
