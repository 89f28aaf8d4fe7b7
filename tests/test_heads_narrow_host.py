"""The narrow heads' C ABI (ABI 34: rslrl_value_head_fwd_bwd_n, rslrl_actor_head_fwd_bwd_n) validates its arguments
before touching the GPU: an RSLRL_LINEAR_FWD_OUT problem with K = 256, N in {64, 128, 192}, x6, M a multiple of 128 (and
5 to 16 actions for the actor) -- every other shape is RSLRL_E_UNSUPPORTED, N = 256 included (the original entries').
No compute calls here: this runs without a GPU."""

import ctypes

import pytest

import test_capi as C
from rsl_rl_amd import _lib

_OUT, _ELU = _lib.LINEAR_FWD_OUT, _lib.LINEAR_FWD_ELU
_X6, _H3, _F32 = _lib.ARITH_X6, _lib.ARITH_H3, _lib.ARITH_F32
_WS = (16, 1 << 20)


def test_abi_version_is_34():
    assert _lib.ABI_VERSION == 34
    assert _lib.lib().rslrl_abi_version() == 34
    assert _lib.HEAD_NARROW_WIDTHS == (64, 128, 192)


# (op, arith, problem fields, head fields, code); the problem is N = 128 unless a row says otherwise
VALUE_ROWS = [
    (_ELU, _X6, {}, {}, -1),  # not a FWD_OUT problem
    (_OUT, _X6, dict(N=256), {}, -3),  # rslrl_value_head_fwd_bwd's shape
    (_OUT, _X6, dict(N=0), {}, -3),
    (_OUT, _X6, dict(N=32), {}, -3),
    (_OUT, _X6, dict(N=100), {}, -3),
    (_OUT, _X6, dict(N=320), {}, -3),
    (_OUT, _X6, dict(K=128), {}, -3),
    (_OUT, _X6, dict(M=100), {}, -3),
    (_OUT, _X6, dict(nout=2), {}, -3),
    (_OUT, _H3, {}, {}, -3),
    (_OUT, _F32, {}, {}, -3),
    (_OUT, _X6, dict(M=0), {}, 0),
    (_OUT, _X6, dict(M=0, N=64), {}, 0),
    (_OUT, _X6, dict(M=0, N=192), {}, 0),
    (_OUT, _X6, dict(M=-1), {}, -1),
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
ACTOR_ROWS = [
    (_ELU, _X6, {}, {}, _WS, -1),
    (_OUT, _X6, dict(N=256), {}, _WS, -3),  # rslrl_actor_head_fwd_bwd's shape
    (_OUT, _X6, dict(N=0), {}, _WS, -3),
    (_OUT, _X6, dict(N=32), {}, _WS, -3),
    (_OUT, _X6, dict(N=100), {}, _WS, -3),
    (_OUT, _X6, dict(N=320), {}, _WS, -3),
    (_OUT, _X6, dict(K=128), {}, _WS, -3),
    (_OUT, _X6, dict(M=100), {}, _WS, -3),
    (_OUT, _X6, dict(M=0), {}, _WS, -3),  # the fused loss divides by M
    (_OUT, _X6, dict(nout=4), dict(num_actions=4), _WS, -3),
    (_OUT, _X6, dict(nout=17), dict(num_actions=17), _WS, -3),
    (_OUT, _X6, {}, dict(num_actions=11), _WS, -3),
    (_OUT, _H3, {}, {}, _WS, -3),
    (_OUT, _F32, {}, {}, _WS, -3),
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
    (_OUT, _X6, dict(N=192), {}, (16, 1024), -2),
]


@pytest.mark.parametrize("op,arith,over,head,expected", VALUE_ROWS)
def test_value_head_n_validation_table(op, arith, over, head, expected):
    a = C._linear_args(op, arith, **{"nout": 1, "N": 128, **over})
    rc = _lib.lib().rslrl_value_head_fwd_bwd_n(ctypes.byref(a), ctypes.byref(C._value_head(**head)), None)
    assert rc == expected


@pytest.mark.parametrize("op,arith,over,head,ws,expected", ACTOR_ROWS)
def test_actor_head_n_validation_table(op, arith, over, head, ws, expected):
    a = C._linear_args(op, arith, **{"N": 128, **over})
    rc = _lib.lib().rslrl_actor_head_fwd_bwd_n(ctypes.byref(a), ctypes.byref(C._actor_head(**head)), ws[0], ws[1], None)
    assert rc == expected


def test_null_structs_are_invalid_arguments():
    L = _lib.lib()
    a = C._linear_args(_OUT, _X6, N=128)
    assert L.rslrl_value_head_fwd_bwd_n(None, ctypes.byref(C._value_head()), None) == -1
    assert L.rslrl_value_head_fwd_bwd_n(ctypes.byref(a), None, None) == -1
    assert L.rslrl_actor_head_fwd_bwd_n(None, ctypes.byref(C._actor_head()), 16, 1 << 20, None) == -1
    assert L.rslrl_actor_head_fwd_bwd_n(ctypes.byref(a), None, 16, 1 << 20, None) == -1


def test_original_entries_still_refuse_narrow_widths():
    """N = 64 / 128 / 192 belong to the new entries alone."""
    L = _lib.lib()
    for N in _lib.HEAD_NARROW_WIDTHS:
        a = C._linear_args(_OUT, _X6, N=N, nout=1)
        assert L.rslrl_value_head_fwd_bwd(ctypes.byref(a), ctypes.byref(C._value_head()), None) == -3
        a = C._linear_args(_OUT, _X6, N=N)
        assert L.rslrl_actor_head_fwd_bwd(ctypes.byref(a), ctypes.byref(C._actor_head()), 16, 1 << 20, None) == -3


def test_python_dispatch_helpers():
    from rsl_rl_amd.networks import fused_mlp
    assert [fused_mlp._head_narrow(n) for n in (64, 128, 192, 256, 100, 0)] == [True, True, True, False, False, False]
