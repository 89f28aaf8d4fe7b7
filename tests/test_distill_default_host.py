"""Host-side checks of the distillation default paths: the structure predicate of the window-batched
update over a width grid (with fusable / *_structure answering as before on it), the C entry point of the one-launch
step record (every refusal comes before any launch, so none of this needs a device), the ABI version, and the GRU
window's launch plan and arithmetic on CPU tensors: Distillation's GRU helpers run with the two cell entry points
replaced by plain-torch restatements of include/rslrl_amd.h, and the gate gradients they leave give nn.GRU's autograd
weight gradients of the reference's replay (resets by the stored dones, the chain cut at an epoch start)."""

import ctypes
from types import SimpleNamespace

import pytest
import torch
import torch.nn as nn

from rsl_rl_amd import _lib, kernels
from rsl_rl_amd.algorithms import distillation as DM
from rsl_rl_amd.networks import MLP, fused_mlp

# name: (input width, hidden, output, activation) -> (fusable_structure, wide_structure, ragged_structure), form
GRID = {
    "narrow": ((48, [256, 256, 256], 12, "elu"), (True, False, False), "fused"),
    "narrow64": ((16, [64, 64], 4, "elu"), (True, False, False), "fused"),
    "wide": ((48, [512, 256, 128], 12, "elu"), (False, True, False), "wide"),
    "ragged": ((45, [64, 64], 4, "elu"), (False, False, True), "ragged"),
    "ragged19": ((19, [64, 64], 4, "elu"), (False, False, True), "ragged"),
    "ragged_wide": ((45, [320, 260, 64], 12, "elu"), (False, False, True), "ragged"),
    "ragged235": ((235, [512, 256, 128], 12, "elu"), (False, False, True), "ragged"),
    "512x512": ((48, [512, 512], 12, "elu"), (False, False, False), None),
    "in1028_narrow": ((1028, [256, 256], 12, "elu"), (True, False, False), "fused"),
    "in1028_wide": ((1028, [512, 256, 128], 12, "elu"), (False, False, False), None),
    "in1029": ((1029, [256, 256], 12, "elu"), (False, False, False), None),
    "unflatten": ((48, [256, 256], (2, 12), "elu"), (True, False, False), None),
    "unflatten_ragged": ((45, [64, 64], (2, 4), "elu"), (False, False, True), None),
    "relu": ((48, [256, 256], 12, "relu"), (False, False, False), None),
    "odd_hidden": ((48, [250, 64], 12, "elu"), (False, False, False), None),
}


@pytest.mark.parametrize("name", list(GRID))
def test_window_trainable_over_the_width_grid(name):
    (width, hidden, out, act), structure, form = GRID[name]
    mlp = MLP(width, out, hidden, act)
    # the three predicates it is made of answer as before, and MLP's flags follow them
    assert (fused_mlp.fusable_structure(mlp), fused_mlp.wide_structure(mlp),
            fused_mlp.ragged_structure(mlp)) == structure
    assert (mlp._fused, mlp._wide, mlp._ragged) == structure
    assert fused_mlp.fusable(mlp, torch.empty(0, width)) is False  # a CPU tensor
    assert fused_mlp.window_trainable(mlp, width) == form
    # rows of another width are never taken (observation groups that do not add up to the first layer's input)
    assert fused_mlp.window_trainable(mlp, width + 4) is None and fused_mlp.window_trainable(mlp, width - 1) is None


def test_window_trainable_refuses_other_modules():
    assert fused_mlp.window_trainable(nn.Sequential(nn.Linear(48, 64), nn.Tanh(), nn.Linear(64, 4)), 48) is None
    assert fused_mlp.window_trainable(nn.Sequential(nn.Linear(48, 4)), 48) is None
    no_bias = nn.Sequential(nn.Linear(48, 64, bias=False), nn.ELU(), nn.Linear(64, 4))
    assert fused_mlp.window_trainable(no_bias, 48) is None


# ---------------------------------------------------------------------------------------------------- the C entry point
def test_abi_32_symbol_and_struct():
    L = _lib.lib()
    assert L.rslrl_abi_version() == _lib.ABI_VERSION >= 32
    assert hasattr(L, "rslrl_distill_record") and "rslrl_distill_record" in _lib.EXPORTED_SYMBOLS
    assert ctypes.sizeof(_lib.DistillObs) == 32
    assert ctypes.sizeof(_lib.DistillRecordArgs) == 16 + 4 * 32 + 4 * 8 + 8 + 4 * 8


def _args(N=64, A=12, groups=((48, 16),), dones_dtype=_lib.DTYPE_I64, base=0x1000):
    """A well-formed argument struct over made-up addresses (nothing is ever launched with them)."""
    a = _lib.DistillRecordArgs()
    a.N, a.A, a.n_obs = N, A, len(groups)
    for i, (w, unit) in enumerate(groups[:_lib.ROLLOUT_MAX_OBS]):
        a.obs[i].src, a.obs[i].dst = base * (2 * i + 2), base * (2 * i + 3)
        a.obs[i].row_floats, a.obs[i].unit_bytes = w, unit
    a.actions, a.privileged_actions, a.rewards, a.dones = 0x100000, 0x200000, 0x300000, 0x400000
    a.dones_dtype = dones_dtype
    a.out_actions, a.out_privileged_actions, a.out_rewards, a.out_dones = 0x500000, 0x600000, 0x700000, 0x800000
    return a


def _call(a):
    return _lib.lib().rslrl_distill_record(ctypes.byref(a) if a is not None else None, None)


def test_distill_record_refuses_before_any_launch():
    INVALID, MISALIGNED = -1, -4  # RSLRL_E_INVALID_ARGUMENT, RSLRL_E_MISALIGNED (include/rslrl_amd.h)
    assert _call(None) == INVALID
    assert _call(_args(N=-1)) == INVALID
    assert _call(_args(A=0)) == INVALID
    # N = 0: nothing to write, whatever the pointers
    empty = _args(N=0)
    assert _call(empty) == 0
    empty.actions = empty.out_dones = None
    assert _call(empty) == 0
    # nulls
    for field in ("actions", "privileged_actions", "rewards", "dones", "out_actions", "out_privileged_actions",
                  "out_rewards", "out_dones"):
        a = _args()
        setattr(a, field, None)
        assert _call(a) == INVALID, field
    for field in ("src", "dst"):
        a = _args()
        setattr(a.obs[0], field, None)
        assert _call(a) == INVALID, field
    # five groups; a group of no width; a unit that is neither a dword nor 16 bytes
    a = _args()
    a.n_obs = 5
    assert _call(a) == INVALID
    a = _args()
    a.n_obs = -1
    assert _call(a) == INVALID
    assert _call(_args(groups=((0, 4),))) == INVALID
    assert _call(_args(groups=((48, 8),))) == INVALID
    # dones dtype codes
    for code in (-1, 4, 17):
        assert _call(_args(dones_dtype=code)) == INVALID, code
    # a 16-byte claim on a width that is no multiple of 4, or on a pointer that is not 16-byte aligned
    assert _call(_args(groups=((45, 16),))) == INVALID
    for field in ("src", "dst"):
        a = _args()
        setattr(a.obs[0], field, getattr(a.obs[0], field) + 4)
        assert _call(a) == MISALIGNED, field
    a = _args(groups=((45, 4),))
    a.obs[0].src += 2  # not even a float's alignment
    assert _call(a) == MISALIGNED
    for field in ("actions", "out_rewards"):
        a = _args()
        setattr(a, field, getattr(a, field) + 1)
        assert _call(a) == MISALIGNED, field
    a = _args(dones_dtype=_lib.DTYPE_I64)
    a.dones += 4
    assert _call(a) == MISALIGNED


def test_distill_record_wrapper_refuses_cpu_tensors():
    t = torch.zeros(4, 3)
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        kernels.distill_record(obs_pairs=[], actions=t, privileged_actions=t, rewards=torch.zeros(4),
                               dones=torch.zeros(4), out_actions=t, out_privileged_actions=t,
                               out_rewards=torch.zeros(4, 1), out_dones=torch.zeros(4, 1, dtype=torch.uint8))
    assert not kernels.distill_record_ok([], t, t, torch.zeros(4), torch.zeros(4))


# ---------------------------------------------------------------------------------- the GRU window on CPU tensors
H = 256


def _fake_cells(monkeypatch, log):
    """kernels.gru_* restated in plain torch from include/rslrl_amd.h (any dtype), each call logged."""

    def gru_image(w_ih, w_hh):
        return (w_ih.detach(), w_hh.detach())

    def gru_cell_train(x, h, image, b_ih, b_hh, reset, h_out, gates, h_restart=None, h_in_out=None):
        w_ih, w_hh = image
        h_in = torch.zeros(x.shape[0], H, dtype=x.dtype) if h is None else h
        if reset is not None:
            assert reset.dtype == torch.uint8 and reset.shape == (x.shape[0],)
            h_in = torch.where(reset.view(-1, 1) != 0, torch.zeros_like(h_in), h_in)
        gi = x @ w_ih.t() + b_ih.detach()
        gh = h_in @ w_hh.t() + b_hh.detach()
        r = torch.sigmoid(gi[:, :H] + gh[:, :H])
        z = torch.sigmoid(gi[:, H:2 * H] + gh[:, H:2 * H])
        a = gh[:, 2 * H:]
        n = torch.tanh(gi[:, 2 * H:] + r * a)
        log.append(("fwd", x, h, reset, h_out, h_in_out))
        for blk, v in zip(gates, (r, z, n, a)):
            blk.copy_(v)
        if h_in_out is not None:
            h_in_out.copy_(h_in)
        h_out.copy_((1 - z) * n + z * h_in)

    def gru_whh_t_image(w_hh):
        return w_hh.detach()

    def gru_cell_bwd(dh, gates, h_in, dg_next, dhz_next, reset_next, w_hh, dg, dhz_out):
        log.append(("bwd", dh, dg_next, dhz_next, reset_next, dg, dhz_out))
        r, z, n, a = gates
        dht = dh.clone()
        if dg_next is not None:
            back = dhz_next + torch.cat([dg_next[0], dg_next[1], dg_next[3]], dim=1) @ w_hh
            if reset_next is not None:
                back = torch.where(reset_next.view(-1, 1) != 0, torch.zeros_like(back), back)
            dht = dht + back
        dn = dht * (1 - z) * (1 - n * n)
        out = (dn * a * r * (1 - r), dht * (h_in - n) * z * (1 - z), dn, dn * r)
        carry = dht * z
        for blk, v in zip(dg, out):
            blk.copy_(v)
        dhz_out.copy_(carry)

    for name, fn in (("gru_image", gru_image), ("gru_cell_train", gru_cell_train),
                     ("gru_whh_t_image", gru_whh_t_image), ("gru_cell_bwd", gru_cell_bwd)):
        monkeypatch.setattr(kernels, name, fn)


@pytest.mark.parametrize("steps", [(0, 1, 2), (3, 4, 5), (6, 7, 0), (7, 0, 1), (2,), (0,)],
                         ids=["epoch_start", "inside", "across_epochs", "across_epochs_early", "one_step", "one_start"])
@pytest.mark.parametrize("seeded", [True, False], ids=["state", "no_state"])
def test_gru_window_against_the_plan_and_autograd(steps, seeded, monkeypatch):
    torch.manual_seed(3)
    f64 = dict(dtype=torch.float64)
    N, O, T, G = 6, 5, 8, len(steps)
    rnn = nn.GRU(O, H).double()
    dones = (torch.rand(T, N) < 0.3).to(torch.uint8)
    dones[:, 0] = 0
    dones[0, 1] = dones[1, 1] = dones[T - 1, 2] = 1  # consecutive dones, a done at t = 0 and one at T - 1
    obs = torch.randn(T, N, O, **f64)
    first = (0.5 * torch.randn(N, H, **f64),) if seeded else None
    entering = (0.5 * torch.randn(N, H, **f64),) if steps[0] != 0 else None  # the state the previous window left
    dh = torch.randn(G, N, H, **f64)
    x = torch.cat([obs[t] for t in steps], dim=0)

    log = []
    _fake_cells(monkeypatch, log)
    fake = SimpleNamespace(storage=SimpleNamespace(num_envs=N), policy=SimpleNamespace(memory_s=SimpleNamespace(rnn=rnn)))
    w = SimpleNamespace(hout=torch.empty(G, N, H, **f64), hin=torch.full((G, N, H), float("nan"), **f64),
                        gates=torch.empty(4, G, N, H, **f64), dg=torch.empty(4, G, N, H, **f64),
                        dc=[torch.empty(N, H, **f64) for _ in range(2)])
    plan = DM.recurrent_window_plan(steps)
    with torch.no_grad():
        tape, state = DM.Distillation._gru_window_forward(fake, w, x, plan, True, entering, first, dones)
        DM.Distillation._gru_window_backward(fake, w, dh, plan, tape)

    # ---- the launches against recurrent_window_plan
    fwd = [e for e in log if e[0] == "fwd"]
    bwd = [e for e in log if e[0] == "bwd"]
    assert len(fwd) == len(bwd) == G and len(state) == 1 and state[0].data_ptr() == w.hout[G - 1].data_ptr()
    for k, (t, starts, chained) in enumerate(plan):
        _, xk, h, reset, h_out, h_in_out = fwd[k]
        assert torch.equal(xk, obs[t]) and h_out.data_ptr() == w.hout[k].data_ptr()
        if starts:  # an epoch start: the supplied state (or none), no reset
            assert reset is None and (h is None if first is None else h is first[0])
        else:  # the previous step's state, the rows done at t - 1 restarting from zero
            assert torch.equal(reset, dones[t - 1])
            assert h.data_ptr() == (w.hout[k - 1] if k else entering[0]).data_ptr()
        # the h as consumed comes from the cell; with no state at all it is zero
        assert (h_in_out is None) == (h is None) and (h is not None or not w.hin[k].any())
        _, dhk, dg_next, dhz_next, reset_next, dg, dhz_out = bwd[G - 1 - k]  # reverse order
        assert dhk.data_ptr() == dh[k].data_ptr() and dg.data_ptr() == w.dg[:, k].data_ptr()
        assert dhz_out is w.dc[k & 1]
        if chained:
            assert dg_next.data_ptr() == w.dg[:, k + 1].data_ptr() and dhz_next is w.dc[(k + 1) & 1]
            assert torch.equal(reset_next, dones[steps[k + 1] - 1])
        else:  # the window's last step, or the next one starts an epoch: the chain is cut
            assert dg_next is None and dhz_next is None and reset_next is None
    assert not torch.isnan(w.hin).any()

    # ---- the gate gradients give autograd's weight gradients of the reference's replay of this window
    state_ref = None if entering is None else entering[0].unsqueeze(0)
    loss = 0
    for k, t in enumerate(steps):
        if t == 0:
            state_ref = None if first is None else first[0].unsqueeze(0)
        elif state_ref is not None:  # Memory.reset(dones[t - 1]) + detach_hidden_states(dones[t - 1])
            state_ref = torch.where(dones[t - 1].view(1, N, 1) != 0, torch.zeros_like(state_ref), state_ref)
        out, state_ref = rnn(obs[t].unsqueeze(0), state_ref)
        assert torch.allclose(out[0], w.hout[k], rtol=0, atol=1e-12), k
        loss = loss + (out[0] * dh[k]).sum()
    g_wih, g_whh, g_bih, g_bhh = torch.autograd.grad(loss, [rnn.weight_ih_l0, rnn.weight_hh_l0, rnn.bias_ih_l0,
                                                            rnn.bias_hh_l0])
    rows = G * N
    dg, hin = w.dg.view(4, rows, H), w.hin.view(rows, H)
    d_ih = torch.cat([dg[0], dg[1], dg[2]], dim=1)  # r, z, n against x
    d_hh = torch.cat([dg[0], dg[1], dg[3]], dim=1)  # r, z, a against the h as consumed
    for ours, ref in ((d_ih.t() @ x, g_wih), (d_hh.t() @ hin, g_whh), (d_ih.sum(0), g_bih), (d_hh.sum(0), g_bhh)):
        assert torch.allclose(ours, ref, rtol=1e-9, atol=1e-11 * ref.abs().max().item())
