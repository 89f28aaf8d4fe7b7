"""The C ABI of the heads for a last hidden layer with 128 inputs (rslrl_value_head_fwd_bwd_k128,
rslrl_actor_head_fwd_bwd_k128: additions to ABI 34) validates its arguments before touching the GPU: an
RSLRL_LINEAR_FWD_OUT problem with K = 128, N in {64, 128}, x6, M a positive multiple of 64 (the critic: one output, no
column sums; the actor: 5 to 16 actions) -- every other shape is RSLRL_E_UNSUPPORTED.  No compute calls: this runs
without a GPU."""

import ctypes

import pytest

import test_capi as C
from rsl_rl_amd import _lib

_OUT, _ELU = _lib.LINEAR_FWD_OUT, _lib.LINEAR_FWD_ELU
_X6, _H3, _F32 = _lib.ARITH_X6, _lib.ARITH_H3, _lib.ARITH_F32
_WS = (16, 1 << 20)
_SHAPES = [dict(K=256)] + [dict(N=n) for n in (0, 32, 100, 192, 256)] + [dict(M=m) for m in (0, 32, 100)]

# (op, arith, problem fields, head fields, code); the problem is K = 128, N = 128, M = 128 unless a row says otherwise
VALUE_ROWS = [(_ELU, _X6, {}, {}, -1)] + [(_OUT, _X6, s, {}, -3) for s in _SHAPES] + [
    (_OUT, _H3, {}, {}, -3),
    (_OUT, _F32, {}, {}, -3),
    (_OUT, _X6, dict(nout=2), {}, -3),
    (_OUT, _X6, {}, dict(colsum_partials=16), -3),
    (_OUT, _X6, dict(a=None), {}, -1),
    (_OUT, _X6, dict(bias=None), {}, -1),
    (_OUT, _X6, dict(c=None), {}, -1),  # dZ is the head's output
    (_OUT, _X6, dict(a=8), {}, -4),
    (_OUT, _X6, dict(out_image=8), {}, -4),
    (_OUT, _X6, {}, dict(target_values=None), -1),
    (_OUT, _X6, {}, dict(returns=None), -1),
    (_OUT, _X6, {}, dict(out_weight=None), -1),
    (_OUT, _X6, {}, dict(wgrad_partials=None), -1),
    (_OUT, _X6, {}, dict(out_weight=8), -4),
]
# ... and (workspace pointer, workspace bytes) for the actor
ACTOR_ROWS = [(_ELU, _X6, {}, {}, _WS, -1)] + [(_OUT, _X6, s, {}, _WS, -3) for s in _SHAPES] + [
    (_OUT, _H3, {}, {}, _WS, -3),
    (_OUT, _F32, {}, {}, _WS, -3),
    (_OUT, _X6, dict(nout=4), dict(num_actions=4), _WS, -3),
    (_OUT, _X6, dict(nout=17), dict(num_actions=17), _WS, -3),
    (_OUT, _X6, {}, dict(num_actions=11), _WS, -3),
    (_OUT, _X6, dict(bimage=None), {}, _WS, -1),
    (_OUT, _X6, dict(y=None), {}, _WS, -1),
    (_OUT, _X6, dict(c=None), {}, _WS, -1),
    (_OUT, _X6, dict(bias=8), {}, _WS, -4),
    (_OUT, _X6, dict(c=8), {}, _WS, -4),
    (_OUT, _X6, {}, dict(actions=None), _WS, -1),
    (_OUT, _X6, {}, dict(sigma=None), _WS, -1),
    (_OUT, _X6, {}, dict(stats=None), _WS, -1),
    (_OUT, _X6, {}, dict(out_weight_t_image=8), _WS, -4),
    (_OUT, _X6, {}, {}, (None, 1 << 20), -1),
    (_OUT, _X6, {}, {}, (8, 1 << 20), -4),
    (_OUT, _X6, {}, {}, (16, 1024), -2),  # workspace too small
    (_OUT, _X6, dict(N=64), {}, (16, 1024), -2),
]


@pytest.mark.parametrize("op,arith,over,head,expected", VALUE_ROWS)
def test_value_head_k128_validation_table(op, arith, over, head, expected):
    a = C._linear_args(op, arith, **{"nout": 1, "K": 128, "N": 128, **over})
    rc = _lib.lib().rslrl_value_head_fwd_bwd_k128(ctypes.byref(a), ctypes.byref(C._value_head(**head)), None)
    assert rc == expected


@pytest.mark.parametrize("op,arith,over,head,ws,expected", ACTOR_ROWS)
def test_actor_head_k128_validation_table(op, arith, over, head, ws, expected):
    a = C._linear_args(op, arith, **{"K": 128, "N": 128, **over})
    rc = _lib.lib().rslrl_actor_head_fwd_bwd_k128(ctypes.byref(a), ctypes.byref(C._actor_head(**head)), ws[0], ws[1],
                                                  None)
    assert rc == expected


def test_null_structs_are_invalid_arguments():
    L = _lib.lib()
    a = C._linear_args(_OUT, _X6, K=128, N=128)
    assert L.rslrl_value_head_fwd_bwd_k128(None, ctypes.byref(C._value_head()), None) == -1
    assert L.rslrl_value_head_fwd_bwd_k128(ctypes.byref(a), None, None) == -1
    assert L.rslrl_actor_head_fwd_bwd_k128(None, ctypes.byref(C._actor_head()), 16, 1 << 20, None) == -1
    assert L.rslrl_actor_head_fwd_bwd_k128(ctypes.byref(a), None, 16, 1 << 20, None) == -1


def test_partial_rows_and_workspace():
    """One partial row per slice, per = ceil(tiles / 512) tiles each: positive and non-decreasing over the GPU tests'
    rows (513 and 514 tiles: two per slice), 0 for an M the entries refuse; the workspace covers 20 fp64 columns per
    slice and fold group behind the 1 KiB of tickets."""
    L = _lib.lib()
    assert _lib.ABI_VERSION == 34 and _lib.HEAD_K128_WIDTHS == (64, 128)
    rows = [L.rslrl_head_k128_partial_rows(m) for m in (64, 192, 32832, 32896)]
    assert rows == [1, 3, 257, 257] and rows == sorted(rows)
    assert [L.rslrl_head_k128_partial_rows(m) for m in (24576, 32768, 393216)] == [384, 512, 512]
    assert [L.rslrl_head_k128_partial_rows(m) for m in (0, 32, 100, -64)] == [0, 0, 0, 0]
    assert L.rslrl_actor_head_k128_workspace_bytes(32832) == 1024 + 8 * 20 * (257 + 5)


def test_other_entries_still_refuse_128_inputs():
    L = _lib.lib()
    for N in _lib.HEAD_K128_WIDTHS:
        a = C._linear_args(_OUT, _X6, K=128, N=N, nout=1)
        assert L.rslrl_value_head_fwd_bwd_n(ctypes.byref(a), ctypes.byref(C._value_head()), None) == -3
        assert L.rslrl_value_head_fwd_bwd(ctypes.byref(a), ctypes.byref(C._value_head()), None) == -3
        a = C._linear_args(_OUT, _X6, K=128, N=N)
        assert L.rslrl_actor_head_fwd_bwd_n(ctypes.byref(a), ctypes.byref(C._actor_head()), 16, 1 << 20, None) == -3
        assert L.rslrl_actor_head_fwd_bwd(ctypes.byref(a), ctypes.byref(C._actor_head()), 16, 1 << 20, None) == -3


def test_python_dispatch_helpers(monkeypatch):
    import torch

    from rsl_rl_amd.networks import fused_mlp
    assert [fused_mlp._head_k128(n, k) for n, k in ((64, 128), (128, 128), (192, 128), (128, 256), (256, 128))] == \
        [True, True, False, False, False]
    stack = [torch.empty(128, 48), torch.empty(128, 128), torch.empty(64, 128), torch.empty(12, 64)]
    assert fused_mlp.narrow_heads_enabled(stack) == (fused_mlp._HEAD_K128 and fused_mlp._VALUE_HEAD)
    monkeypatch.setattr(fused_mlp, "_HEAD_K128", False)
    assert not fused_mlp.narrow_heads_enabled(stack)
