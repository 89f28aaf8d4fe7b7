"""The distillation head's C ABI (rslrl_bc_head_fwd_bwd, an addition to ABI 34) validates its arguments before touching
the GPU: an RSLRL_LINEAR_FWD_OUT problem with K = 256, N in {64, 128, 192, 256}, x6, 5 to 16 outputs, whole steps of a
multiple of 128 rows -- every other shape is RSLRL_E_UNSUPPORTED.  Plus the Python side's choice of path.  No compute
calls here: this runs without a GPU."""

import ctypes
from types import SimpleNamespace

import pytest
import torch

import test_capi as C
from rsl_rl_amd import _lib
from rsl_rl_amd.algorithms import distillation
from rsl_rl_amd.networks import fused_mlp

_OUT, _ELU = _lib.LINEAR_FWD_OUT, _lib.LINEAR_FWD_ELU
_X6, _H3, _F32 = _lib.ARITH_X6, _lib.ARITH_H3, _lib.ARITH_F32
_WS = (16, 1 << 20)


def _bc_head(**over):
    f = dict(target=16, num_outputs=12, rows_per_step=128, huber=0, out_weight_t_image=16, wgrad_partials=16,
             step_loss=16, grad_out=None)
    f.update(over)
    return _lib.BCHeadArgs(*(f[k] for k, _ in _lib.BCHeadArgs._fields_))


# (op, arith, problem fields (M = 384, N = 128 unless a row says otherwise), head fields, workspace, code)
ROWS = [
    (_ELU, _X6, {}, {}, _WS, -1),  # not a FWD_OUT problem
    (_OUT, _H3, {}, {}, _WS, -3),
    (_OUT, _F32, {}, {}, _WS, -3),
    (_OUT, _X6, dict(K=128), {}, _WS, -3),
    (_OUT, _X6, dict(N=32), {}, _WS, -3),
    (_OUT, _X6, dict(N=100), {}, _WS, -3),
    (_OUT, _X6, dict(nout=4), dict(num_outputs=4), _WS, -3),
    (_OUT, _X6, dict(nout=17), dict(num_outputs=17), _WS, -3),
    (_OUT, _X6, {}, dict(rows_per_step=192), _WS, -3),
    (_OUT, _X6, {}, dict(rows_per_step=0), _WS, -3),
    (_OUT, _X6, {}, dict(rows_per_step=256), _WS, -3),  # 384 rows are no whole number of steps
    (_OUT, _X6, dict(M=0), {}, _WS, -3),  # the loss divides by the step's rows
    (_OUT, _X6, dict(M=-1), {}, _WS, -1),
    (_OUT, _X6, {}, dict(num_outputs=11), _WS, -1),
    (_OUT, _X6, {}, dict(huber=2), _WS, -1),
    (_OUT, _X6, dict(bimage=None), {}, _WS, -1),
    (_OUT, _X6, dict(y=None), {}, _WS, -1),
    (_OUT, _X6, dict(c=None), {}, _WS, -1),  # dZ is the head's output
    (_OUT, _X6, {}, dict(target=None), _WS, -1),
    (_OUT, _X6, {}, dict(step_loss=None), _WS, -1),
    (_OUT, _X6, {}, dict(wgrad_partials=None), _WS, -1),
    (_OUT, _X6, {}, {}, (None, 1 << 20), -1),
    (_OUT, _X6, dict(bias=8), {}, _WS, -4),
    (_OUT, _X6, dict(c=8), {}, _WS, -4),
    (_OUT, _X6, {}, dict(out_weight_t_image=8), _WS, -4),
    (_OUT, _X6, {}, {}, (8, 1 << 20), -4),
    (_OUT, _X6, {}, {}, (16, 47), -2),  # three tiles need 48 bytes
    (_OUT, _X6, dict(N=256), {}, (16, 47), -2),  # every width reaches the workspace check
    (_OUT, _X6, dict(N=64), {}, (16, 47), -2),
    (_OUT, _X6, dict(N=192), dict(rows_per_step=384, huber=1), (16, 47), -2),
]


@pytest.mark.parametrize("op,arith,over,head,ws,expected", ROWS)
def test_bc_head_validation_table(op, arith, over, head, ws, expected):
    a = C._linear_args(op, arith, **{"M": 384, "N": 128, **over})
    assert _lib.lib().rslrl_bc_head_fwd_bwd(ctypes.byref(a), ctypes.byref(_bc_head(**head)), ws[0], ws[1], None) == expected


def test_abi_and_workspace():
    L = _lib.lib()
    assert _lib.ABI_VERSION == 34 and L.rslrl_abi_version() == 34
    assert L.rslrl_bc_head_fwd_bwd(None, ctypes.byref(_bc_head()), 16, 1 << 20, None) == -1
    assert L.rslrl_bc_head_fwd_bwd(ctypes.byref(C._linear_args(_OUT, _X6)), None, 16, 1 << 20, None) == -1
    # one 16-byte record per 128-row tile, whatever the step length
    assert [L.rslrl_bc_head_workspace_bytes(M, n) for M, n in ((0, 128), (128, 128), (3840, 256), (3840, 1280))] == \
        [0, 16, 480, 480]


@pytest.mark.parametrize("A,rps,M,ok", [(12, 128, 384, True), (5, 384, 384, True), (16, 256, 3840, True),
                                        (4, 128, 384, False), (17, 128, 384, False), (12, 192, 384, False),
                                        (12, 256, 384, False), (12, 64, 384, False)])
def test_bc_head_supported(A, rps, M, ok):
    head = fused_mlp.BCHead(torch.zeros(M, A), rps, "huber", torch.zeros(max(M // max(rps, 1), 1)))
    assert head.huber and head.supported(M) is ok
    assert not fused_mlp.BCHead(torch.zeros(M, 20)[:, :8], rps, "mse", torch.zeros(1)).supported(M)  # strided target


@pytest.mark.parametrize("knob,N,ran", [(True, 256, True), (True, 200, False), (False, 256, False), (True, 128, False)])
def test_mlp_step_choice(monkeypatch, knob, N, ran):
    """_mlp_step hands train_forward a BCHead when the knob is on and num_envs is a multiple of 128, skips the loss and
    the output-layer backward launches when the head ran (N = 128 here: the head declines), and keeps them otherwise."""
    calls = []
    monkeypatch.setattr(distillation, "_BC_HEAD", knob)

    def train_forward(x, ws, bs, bc_head=None):
        calls.append(("fwd", bc_head is not None))
        if bc_head is not None and ran:
            bc_head.done = True
        return "y", "tape"

    monkeypatch.setattr(fused_mlp, "train_forward", train_forward)
    monkeypatch.setattr(fused_mlp, "train_backward", lambda tape, dy, **kw: (calls.append(("bwd", dy is None)), None))
    monkeypatch.setattr(distillation.kernels, "bc_loss", lambda *a, **kw: calls.append(("loss",)))
    alg = SimpleNamespace(storage=SimpleNamespace(num_envs=N), loss_type="mse")
    distillation.Distillation._mlp_step(alg, None, torch.zeros(15 * N, 12), torch.zeros(15), ([], [], []),
                                        torch.zeros(15 * N, 12))
    built = knob and N % 128 == 0
    assert calls == ([("fwd", True), ("bwd", True)] if ran else [("fwd", built), ("loss",), ("bwd", False)])
