"""Recurrent distillation at a student observation width that is no multiple of 16: Distillation.update()
with a StudentTeacherRecurrent against the reference's drec_d fixture (tests/golden/make_golden_distillation_recurrent_anyd.py:
case c of tests/test_gpu_distillation_recurrent.py with 45 student observations) on the window-batched path -- the
forward and reverse cell launches counted -- and, with RSLRL_DISTILL_FUSED=0, on the per-step path.  The checks and
tolerances are that file's for case c."""

import json
import os

import numpy as np
import pytest
import torch

import drec_fixtures as D
import test_gpu_distillation_recurrent as T
from update_fixtures import param_errors

pytestmark = pytest.mark.gpu

with open(os.path.join(D.GOLDEN, "golden_distillation_recurrent_anyd.json")) as _f:
    META = json.load(_f)


@pytest.mark.parametrize("fused", [True, False], ids=["d_windows", "d_per_step"])
def test_update_matches_reference(fused, cuda_device, monkeypatch):
    from rsl_rl_amd import kernels
    from rsl_rl_amd.networks import fused_mlp
    monkeypatch.setenv("RSLRL_DISTILL_FUSED", "1" if fused else "0")
    meta = META["d"]
    assert meta["O_student"] == 45 and kernels._rnn_anyd(meta["O_student"]) and meta["rnn_hidden_dim"] == 256
    z = D.load_arrays(meta)
    alg, pol = D.build_distillation(z, meta, "cuda:0")
    assert alg._clip_adam is not None and not alg._fused_ok() and alg._fused_recurrent_ok() is fused
    calls = T._count_backward_launches(monkeypatch)
    forward = []
    real = kernels.lstm_cell_train

    def counted(*a, **k):
        forward.append(a[0].shape[1])
        return real(*a, **k)

    monkeypatch.setattr(kernels, "lstm_cell_train", counted)
    ragged = fused_mlp.ragged_launches
    before = {k: v.detach().clone() for k, v in pol.state_dict().items()}
    base = T._Baseline(z, meta, pol, "cuda:0")
    out = D.run_recorded_update(alg)
    ref = meta["ranks"][0]
    # the window path really ran: per step of each full window one reverse launch, one forward launch for every step
    # of the schedule (the trailing window's included), dW_ih on the ragged kernel once per gate block and full window
    assert len(calls) == (ref["num_steps"] * meta["G"] if fused else 0)
    assert forward == ([45] * (meta["E"] * meta["T"]) if fused else [])
    assert fused_mlp.ragged_launches - ragged == (4 * ref["num_steps"] if fused else 0)
    if fused:  # every gradient is a view of the one arena the multi-GPU all-reduce runs on
        flat = alg._arena.flat
        with_grad = [p for p in pol.parameters() if p.grad is not None]
        assert len(with_grad) == len(alg._arena.params) == len(D.trained_names(pol))
        assert all(flat.data_ptr() <= p.grad.data_ptr() < flat.data_ptr() + 4 * flat.numel() for p in with_grad)

    # the schedule and the losses
    assert out["lr_trace"] == ref["lr_trace"] and out["lr"] == ref["final_lr"]
    assert len(out["lr_trace"]) == ref["num_steps"]
    ref_steps = z["r0/step_losses"]
    ours = np.asarray(out["step_losses"])
    assert ours.shape == ref_steps.shape == (meta["E"] * meta["T"],)
    print("d step losses: max rel err", np.max(np.abs(ours - ref_steps) / np.abs(ref_steps)))
    assert np.all(np.abs(ours - ref_steps) <= 1e-4 * np.abs(ref_steps)), (ours, ref_steps)
    v = ref["loss_dict"]["behavior"]
    assert set(out["loss"]) == {"behavior"} and abs(out["loss"]["behavior"] - v) <= 1e-4 * abs(v) + 1e-6

    # the first gradient before clipping, tensor by tensor, memory and MLP
    names = D.trained_names(pol)
    assert sorted(out["grads"]) == sorted(names) and any(n.startswith("memory_s.") for n in names)
    gerr = {}
    for n in names:
        r = torch.from_numpy(z["r0/grad_mb0/" + n]).double()
        gerr[n] = (out["grads"][n].double() - r).abs().max().item() / r.abs().max().item()
    print("d first gradient, max err / max:", {k: f"{e:.1e}" for k, e in gerr.items()})
    assert all(e <= 1e-5 for e in gerr.values()), gerr

    # the parameters: within the reference's own one-ulp sensitivity envelope (or twice torch's own GPU autograd)
    errs = param_errors(out["final"], z, "r0/")
    print("d param errors (max abs / ||d|| over ||moved||):", {k: f"{a:.1e}/{m:.1e}" for k, (a, m) in errs.items()})
    assert sorted(errs) == sorted(names)
    sens = meta["ulp_sensitivity"]
    for name, (abs_err, rel_moved) in errs.items():
        if not rel_moved <= 2 * sens[name] + 1e-4:
            b_abs, b_rel = base.get()[0][name]
            assert rel_moved <= 2 * b_rel, (name, abs_err, rel_moved, b_abs, b_rel)

    # the hidden states of both memories after the update
    hid = D.hidden_lists(out["hidden"])
    assert sorted(hid) == sorted(k[len("r0/hidden_final/"):] for k in z.files if k.startswith("r0/hidden_final/"))
    for k, h in hid.items():
        r = torch.from_numpy(z["r0/hidden_final/" + k])
        d = (h - r).abs().max().item()
        tol = 2 * sens["hidden_final/" + k] + 1e-4 * r.abs().max().item()
        print("d hidden state", k, "max err", d, "tolerance", tol)
        if d > tol:
            assert d <= 2 * base.get()[1][k], (k, d, base.get()[1][k])
    done_last = torch.from_numpy(z["r0/dones"])[-1] == 1
    assert (hid["s0"][:, done_last] == 0).all() and (hid["s0"][:, ~done_last] != 0).any()

    # the memory and the MLP move, nothing else does
    for k, val in pol.state_dict().items():
        assert torch.equal(val, before[k]) != k.startswith(("student.", "memory_s.")), k
    assert alg.num_updates == 1 and alg.storage.step == 0
