"""Host-side checks of the distillation default paths: the structure predicate of the window-batched
update over a width grid (with fusable / *_structure answering as before on it), the C entry point of the one-launch
step record (every refusal comes before any launch, so none of this needs a device), the ABI version, and the GRU
and the LSTM window's launch plan and arithmetic on CPU tensors: Distillation's window helpers run with the cell's entry
points replaced by plain-torch restatements of include/rslrl_amd.h, and the gate gradients they leave give nn.GRU's /
nn.LSTM's autograd weight gradients of the reference's replay (resets by the stored dones, the chain cut at an epoch
start).  Last, the table of cell kinds (kernels.Cell) against the predicates it stands for."""

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
    """kernels.gru_* and kernels.lstm_* restated in plain torch from include/rslrl_amd.h (any dtype), each call
    logged."""

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

    def lstm_image(w_ih, w_hh):
        return (w_ih.detach(), w_hh.detach())

    def lstm_cell_train(x, state, image, b_ih, b_hh, reset, h_out, c_out, gates, h_restart=None, c_restart=None,
                        h_in_out=None):
        w_ih, w_hh = image
        zeros = torch.zeros(x.shape[0], H, dtype=x.dtype)
        h_in, c_in = (zeros, zeros) if state is None else state
        if reset is not None:
            assert reset.dtype == torch.uint8 and reset.shape == (x.shape[0],)
            h_in = torch.where(reset.view(-1, 1) != 0, zeros, h_in)
            c_in = torch.where(reset.view(-1, 1) != 0, zeros, c_in)
        pre = x @ w_ih.t() + b_ih.detach() + h_in @ w_hh.t() + b_hh.detach()
        i, f, o = (torch.sigmoid(pre[:, b * H:(b + 1) * H]) for b in (0, 1, 3))
        g = torch.tanh(pre[:, 2 * H:3 * H])
        log.append(("fwd", x, state, reset, h_out, c_out, h_restart, c_restart, h_in_out))
        for blk, v in zip(gates, (i, f, g, o)):
            blk.copy_(v)
        c_out.copy_(f * c_in + i * g)
        h_out.copy_(o * torch.tanh(c_out))

    def lstm_whh_t_image(w_hh):
        return w_hh.detach()

    def lstm_cell_bwd(dh, gates, c_out, c_prev, reset_cur, dg_next, dc_next, reset_next, whh_t_image, dg, dc_prev,
                      c_restart=None):
        log.append(("bwd", dh, c_out, c_prev, reset_cur, dg_next, dc_next, reset_next, dg, dc_prev, c_restart))
        i, f, g, o = gates
        dht, dc = dh.clone(), torch.zeros_like(dh)
        if dg_next is not None:
            back = torch.cat(list(dg_next), dim=1) @ whh_t_image
            cut = torch.zeros(dh.shape[0], 1, dtype=torch.bool) if reset_next is None else reset_next.view(-1, 1) != 0
            dht = dht + torch.where(cut, torch.zeros_like(back), back)
            dc = torch.where(cut, torch.zeros_like(dc_next), dc_next)
        c_in = torch.zeros_like(c_out) if c_prev is None else c_prev
        if reset_cur is not None:
            c_in = torch.where(reset_cur.view(-1, 1) != 0, torch.zeros_like(c_in), c_in)
        t = torch.tanh(c_out)
        dc = dc + dht * o * (1 - t * t)
        out = (dc * g * i * (1 - i), dc * c_in * f * (1 - f), dc * i * (1 - g * g), dht * t * o * (1 - o))
        carry = dc * f
        for blk, v in zip(dg, out):
            blk.copy_(v)
        dc_prev.copy_(carry)

    for fn in (gru_image, gru_cell_train, gru_whh_t_image, gru_cell_bwd,
               lstm_image, lstm_cell_train, lstm_whh_t_image, lstm_cell_bwd):
        monkeypatch.setattr(kernels, fn.__name__, fn)


def _check_lstm_window(log, w, plan, steps, dones, obs, dh, first, entering, state, rnn, x):
    """The LSTM's side of the window test: what test_gru_window_against_the_plan_and_autograd asserts for the GRU, for
    the state (h, c), the h as consumed composed on the host, and nn.LSTM."""
    G, N = dh.shape[:2]
    fwd = [e for e in log if e[0] == "fwd"]
    bwd = [e for e in log if e[0] == "bwd"]
    assert len(fwd) == len(bwd) == G and len(state) == 2
    assert [s.data_ptr() for s in state] == [o[G - 1].data_ptr() for o in w.out]
    # ---- the launches against recurrent_window_plan
    for k, (t, starts, chained) in enumerate(plan):
        _, xk, st, reset, h_out, c_out, h_restart, c_restart, h_in_out = fwd[k]
        assert torch.equal(xk, obs[t]) and h_out.data_ptr() == w.out[0][k].data_ptr()
        assert c_out.data_ptr() == w.out[1][k].data_ptr()
        assert h_restart is None and c_restart is None and h_in_out is None  # no restart states; hin is the host's
        if starts:  # an epoch start: the supplied state (or none), no reset
            assert reset is None and (st is None if first is None else st is first)
        else:  # the previous step's state, the rows done at t - 1 restarting from zero
            assert torch.equal(reset, dones[t - 1])
            src = [o[k - 1] for o in w.out] if k else entering
            assert [s.data_ptr() for s in st] == [s.data_ptr() for s in src]
        # the h as consumed: the entering h with the reset rows zeroed; with no state at all it is zero
        if st is None:
            assert not w.hin[k].any()
        else:
            keep = torch.ones(N, 1, dtype=torch.bool) if reset is None else reset.view(N, 1) == 0
            assert torch.equal(w.hin[k], torch.where(keep, st[0], torch.zeros_like(st[0])))
        _, dhk, c_out, c_prev, reset_cur, dg_next, dc_next, reset_next, dg, dc_prev, c_restart = bwd[G - 1 - k]
        assert dhk.data_ptr() == dh[k].data_ptr() and dg.data_ptr() == w.dg[:, k].data_ptr()
        assert c_out.data_ptr() == w.out[1][k].data_ptr() and dc_prev is w.dc[k & 1] and c_restart is None
        # the c entering the step and its reset vector are the forward's
        assert (c_prev is None) if st is None else (c_prev is st[1])
        assert (reset_cur is None) if reset is None else torch.equal(reset_cur, reset)
        if chained:
            assert dg_next.data_ptr() == w.dg[:, k + 1].data_ptr() and dc_next is w.dc[(k + 1) & 1]
            assert torch.equal(reset_next, dones[steps[k + 1] - 1])
        else:  # the window's last step, or the next one starts an epoch: the chain is cut
            assert dg_next is None and dc_next is None and reset_next is None
    assert not torch.isnan(w.hin).any()

    # ---- the gate gradients give autograd's weight gradients of the reference's replay of this window
    state_ref = None if entering is None else tuple(s.unsqueeze(0) for s in entering)
    loss = 0
    for k, t in enumerate(steps):
        if t == 0:
            state_ref = None if first is None else tuple(s.unsqueeze(0) for s in first)
        elif state_ref is not None:  # Memory.reset(dones[t - 1]) + detach_hidden_states(dones[t - 1])
            gone = dones[t - 1].view(1, N, 1) != 0
            state_ref = tuple(torch.where(gone, torch.zeros_like(s), s) for s in state_ref)
        out, state_ref = rnn(obs[t].unsqueeze(0), state_ref)
        assert torch.allclose(out[0], w.hout[k], rtol=0, atol=1e-12), k
        assert torch.allclose(state_ref[1][0], w.out[1][k], rtol=0, atol=1e-12), k
        loss = loss + (out[0] * dh[k]).sum()
    g_wih, g_whh, g_bih, g_bhh = torch.autograd.grad(loss, [rnn.weight_ih_l0, rnn.weight_hh_l0, rnn.bias_ih_l0,
                                                            rnn.bias_hh_l0])
    rows = G * N
    d = torch.cat(list(w.dg.view(4, rows, H)), dim=1)  # i, f, g, o against x and against the h as consumed
    hin = w.hin.view(rows, H)
    for ours, ref in ((d.t() @ x, g_wih), (d.t() @ hin, g_whh), (d.sum(0), g_bih), (d.sum(0), g_bhh)):
        assert torch.allclose(ours, ref, rtol=1e-9, atol=1e-11 * ref.abs().max().item())


# (the GRU's cases keep the ids they had before the LSTM's joined them)
@pytest.mark.parametrize("steps", [(0, 1, 2), (3, 4, 5), (6, 7, 0), (7, 0, 1), (2,), (0,)],
                         ids=["epoch_start", "inside", "across_epochs", "across_epochs_early", "one_step", "one_start"])
@pytest.mark.parametrize("kind,seeded", [("gru", True), ("gru", False), ("lstm", True), ("lstm", False)],
                         ids=["state", "no_state", "lstm-state", "lstm-no_state"])
def test_gru_window_against_the_plan_and_autograd(steps, kind, seeded, monkeypatch):
    torch.manual_seed(3)
    f64 = dict(dtype=torch.float64)
    N, O, T, G = 6, 5, 8, len(steps)
    cell = {"gru": kernels.GRU, "lstm": kernels.LSTM}[kind]
    rnn = {"gru": nn.GRU, "lstm": nn.LSTM}[kind](O, H).double()
    dones = (torch.rand(T, N) < 0.3).to(torch.uint8)
    dones[:, 0] = 0
    dones[0, 1] = dones[1, 1] = dones[T - 1, 2] = 1  # consecutive dones, a done at t = 0 and one at T - 1
    obs = torch.randn(T, N, O, **f64)
    first = tuple(0.5 * torch.randn(N, H, **f64) for _ in range(cell.n_state)) if seeded else None
    # the state the previous window left
    entering = tuple(0.5 * torch.randn(N, H, **f64) for _ in range(cell.n_state)) if steps[0] != 0 else None
    dh = torch.randn(G, N, H, **f64)
    x = torch.cat([obs[t] for t in steps], dim=0)

    log = []
    _fake_cells(monkeypatch, log)
    fake = SimpleNamespace(storage=SimpleNamespace(num_envs=N), policy=SimpleNamespace(memory_s=SimpleNamespace(rnn=rnn)))
    w = SimpleNamespace(out=tuple(torch.empty(G, N, H, **f64) for _ in range(cell.n_state)),
                        hin=torch.full((G, N, H), float("nan"), **f64),
                        gates=torch.empty(4, G, N, H, **f64), dg=torch.empty(4, G, N, H, **f64),
                        dc=[torch.empty(N, H, **f64) for _ in range(2)])
    w.hout = w.out[0]
    plan = DM.recurrent_window_plan(steps)
    with torch.no_grad():
        tape, state = DM.Distillation._window_forward(fake, cell, w, x, plan, True, entering, first, dones)
        DM.Distillation._window_backward(fake, cell, w, dh, plan, tape)
    if kind == "lstm":
        return _check_lstm_window(log, w, plan, steps, dones, obs, dh, first, entering, state, rnn, x)

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


# ---------------------------------------------------------------------------------------------- the table of cell kinds
def test_cell_table_of_kinds():
    assert kernels.cell_of(nn.LSTM(5, H)) is kernels.LSTM and kernels.cell_of(nn.GRU(5, H)) is kernels.GRU
    assert kernels.cell_of(nn.RNN(5, H)) is None and kernels.cell_of(nn.Linear(5, H)) is None

    class MyLSTM(nn.LSTM):
        pass

    assert kernels.cell_of(MyLSTM(5, H)) is None  # exactly nn.LSTM / nn.GRU
    assert (kernels.LSTM.name, kernels.LSTM.n_state, kernels.LSTM.blocks, kernels.LSTM.knob) == \
        ("lstm", 2, 4, "RSLRL_LSTM_CELL")
    assert (kernels.GRU.name, kernels.GRU.n_state, kernels.GRU.blocks, kernels.GRU.knob) == \
        ("gru", 1, 3, "RSLRL_GRU_CELL")
    with pytest.raises(Exception):
        kernels.LSTM.blocks = 3  # immutable


def test_cell_state_conversions_round_trip():
    h, c = torch.randn(1, 4, H), torch.randn(1, 4, H)
    for cell, hidden in ((kernels.LSTM, (h, c)), (kernels.GRU, h)):
        assert cell.unpack(None) is None
        state = cell.unpack(hidden)
        assert isinstance(state, tuple) and len(state) == cell.n_state and state[0] is h
        back = cell.pack(state)
        assert cell.unpack(back) == state
        if cell is kernels.GRU:
            assert back is h and cell.unpack((h,)) == (h,) and cell.unpack([h]) == (h,)
        else:
            assert isinstance(back, tuple) and back[0] is h and back[1] is c and cell.unpack([h, c]) == (h, c)


@pytest.mark.parametrize("any_input", [True, False], ids=["any_input", "first_widths_only"])
def test_cell_supported_and_enabled_follow_the_predicates(any_input, monkeypatch):
    from test_rnn_anyd_host import GRID_D, GRID_M

    monkeypatch.setattr(kernels, "_RNN_ANY_INPUT", any_input)  # RSLRL_RNN_ANY_INPUT, read at import
    for cell in (kernels.LSTM, kernels.GRU):
        first = getattr(kernels, f"{cell.name}_cell_supported")
        anyd = getattr(kernels, f"{cell.name}_cell_anyd_supported")
        for M in GRID_M:
            for D in GRID_D:
                for hidden, layers in ((256, 1), (512, 1), (256, 2)):
                    got = cell.supported(M, D, hidden, layers)
                    assert got == anyd(M, D, hidden, layers) == (anyd if any_input else first)(M, D, hidden, layers)
        assert cell.supported(64, 45, 256) == any_input and cell.supported(64, 48, 256)
        # the knob is read at call time
        monkeypatch.delenv(cell.knob, raising=False)
        assert cell.enabled()
        monkeypatch.setenv(cell.knob, "0")
        assert not cell.enabled()
        monkeypatch.setenv(cell.knob, "1")
        assert cell.enabled()
