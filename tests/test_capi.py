"""The C ABI library loads, exports every entry point include/rslrl_amd.h declares, and validates its
arguments before touching the GPU (no compute calls here: this runs without a GPU)."""

import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT, golden_path
from rsl_rl_amd import _lib

HEADER = os.path.join(ROOT, "include", "rslrl_amd.h")


def declared_functions():
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(rslrl_[a-z0-9_]+)\s*\(", text)))


def test_header_matches_binding_list():
    assert declared_functions() == sorted(_lib.EXPORTED_SYMBOLS)


def test_library_exports_every_declared_symbol():
    L = _lib.lib()
    for name in declared_functions():
        assert hasattr(L, name), name
    assert L.rslrl_abi_version() == _lib.ABI_VERSION


def test_status_strings():
    L = _lib.lib()
    assert L.rslrl_status_string(0) == b"ok"
    assert b"invalid" in L.rslrl_status_string(-1)
    assert b"hipError_t" in L.rslrl_status_string(1)


def test_argument_validation_without_gpu():
    L = _lib.lib()
    # negative sizes / null pointers are rejected before any launch
    assert L.rslrl_compute_returns(None, None, None, None, 0.99, 0.95, -1, 4, 1, None, None, None, 0, None) == -1
    assert L.rslrl_compute_returns(None, None, None, None, 0.99, 0.95, 4, 4, 1, None, None, None, 0, None) == -1
    assert L.rslrl_compute_returns(None, None, None, None, 0.99, 0.95, 0, 4, 1, None, None, None, 0, None) == 0
    f = (_lib.GatherField * 1)(_lib.GatherField(8, 8, 6))  # row_bytes not a multiple of 4
    assert L.rslrl_gather_rows(f, 1, 8, 4, None) == -1
    assert L.rslrl_gather_rows(f, 17, 8, 4, None) == -1
    args = _lib.PPOLossArgs()
    args.B, args.A = 0, 4
    assert L.rslrl_ppo_loss_fwd_bwd(ctypes.byref(args), None, 0, None) == -1
    args.B, args.A = 10, 65
    assert L.rslrl_ppo_loss_fwd_bwd(ctypes.byref(args), None, 0, None) == -1
    assert L.rslrl_ppo_loss_workspace_bytes(393216, 12) >= 8 * 16 * 512
    assert L.rslrl_compute_returns_workspace_bytes(24, 65536) >= 16 * 256


def test_gae_workspace_words_and_knobs_without_gpu():
    """ABI 18: the status word sits after the partials and the barrier's ticket / generation, inside the workspace;
    the test knobs validate their names and ranges and hand back the previous value (host code, no GPU)."""
    L = _lib.lib()
    ws = L.rslrl_compute_returns_workspace_bytes(24, 131072)
    off = L.rslrl_compute_returns_status_offset()
    assert off % 4 == 0 and off >= 8 + 2048 * 32 and off + 4 <= ws
    prev = ctypes.c_int64(0)
    assert L.rslrl_debug_knob(b"no_such_knob", 1, None) == -1
    assert L.rslrl_debug_knob(None, 1, None) == -1
    assert L.rslrl_debug_knob(b"gae_spin_limit", -1, None) == -1
    assert L.rslrl_debug_knob(b"gae_spin_limit", 5, ctypes.byref(prev)) == 0
    assert prev.value == 1 << 22
    assert L.rslrl_debug_knob(b"gae_spin_limit", prev.value, ctypes.byref(prev)) == 0 and prev.value == 5
    assert L.rslrl_debug_knob(b"gae_form", -1, ctypes.byref(prev)) == 0 and prev.value == -1
    # forms need T in {8, 16, 24, 32} for a one-launch form; invalid sizes report the two-launch form
    assert L.rslrl_compute_returns_slots_form(0, 4, None, None, None, None, None, None) == 0
    assert L.rslrl_compute_returns_slots_form(5, 4096, None, None, None, None, None, None) == 0


def test_value_head_partial_rows_follows_the_dispatch():
    """ABI 18: a call with colsum_partials always takes the tiled head, so its partial-row count is M / 128
    whatever the streaming default; without it the streaming form's per-slice count (<= 256 rows)."""
    L = _lib.lib()
    M = 393216
    assert L.rslrl_value_head_partial_rows(M, 1) == M // 128
    assert L.rslrl_value_head_partial_rows(M, 0) in (M // 128,) or L.rslrl_value_head_partial_rows(M, 0) <= 256
    assert L.rslrl_value_head_partial_rows(0, 0) == 0


def _linear_args(op, arith=_lib.ARITH_X6, **over):
    """A rslrl_linear_args_t that passes every check of `op` (small fake pointers: 16-byte aligned, never
    dereferenced because each caller adds one fault or an empty batch), with the fields in `over` replaced."""
    f = dict(a=16, a_amax=16 if arith == _lib.ARITH_H3 else None, M=128,
             K=12 if op == _lib.LINEAR_DGRAD_ELU_WGRAD else 256, N=256, bimage=16, bias=16, h=16, c=16,
             colsum_partials=16, wgrad_partials=16, out_image=16, out_bias=16, y=16,
             nout=12 if op == _lib.LINEAR_FWD_OUT else 0, amax_out=None, amax_workspace=None)
    f.update(over)
    return _lib.LinearArgs(op, arith, f["a"], f["a_amax"], f["M"], f["K"], f["N"], f["bimage"], f["bias"], f["h"],
                           f["c"], f["colsum_partials"], f["wgrad_partials"], f["out_image"], f["out_bias"], f["y"],
                           f["nout"], f["amax_out"], f["amax_workspace"])


def test_linear_abi_rejects_bad_shapes():
    L = _lib.lib()

    def gemm(op, arith, **over):
        return L.rslrl_linear_gemm(ctypes.byref(_linear_args(op, arith, **over)), None)

    FWD, DGRAD, F32 = _lib.LINEAR_FWD_ELU, _lib.LINEAR_DGRAD_ELU, _lib.ARITH_F32
    assert gemm(FWD, F32, a=8, M=10, K=6, N=16, bimage=8, bias=8, c=8) == -1  # K % 4 != 0
    assert gemm(FWD, F32, a=8, M=10, K=8, N=300, bimage=8, bias=8, c=8) == -1  # N > 256
    assert gemm(FWD, F32, a=8, M=0, K=8, N=16, bimage=8, bias=8, c=8) == 0  # empty batch
    assert gemm(FWD, F32, M=10, K=8, N=16, bimage=None) == -1  # no B operand (neither a weight nor an image)
    assert gemm(FWD, _lib.ARITH_X6, M=10, K=8, N=16, bimage=24) == -4  # misaligned image
    assert gemm(DGRAD, F32, a=8, M=10, K=6, N=16, bimage=8, h=8, c=8, colsum_partials=8) == -1  # Nred % 4 != 0
    assert L.rslrl_linear_tiles(393216) == 3072
    assert L.rslrl_linear_bimage_bytes(256) == 16 * 3 * 256 * 32  # 16 chunks x 3 planes x 256 rows x 32 B
    assert L.rslrl_linear_bimage_bytes(12) == 3 * 256 * 32
    assert L.rslrl_linear_prepare_bimage(16, 300, 16, 0, 16, None) == -1  # rows > 256
    assert L.rslrl_linear_prepare_bimage(16, 16, 16, 0, 8, None) == -4  # misaligned image


_FWD, _ELU, _DGRAD, _OUTBWD, _OUT = (_lib.LINEAR_FWD, _lib.LINEAR_FWD_ELU, _lib.LINEAR_DGRAD_ELU,
                                     _lib.LINEAR_DGRAD_ELU_WGRAD, _lib.LINEAR_FWD_OUT)
_ALL = (_FWD, _ELU, _DGRAD, _OUTBWD, _OUT)
_X6, _H3 = _lib.ARITH_X6, _lib.ARITH_H3
_AMAX = dict(amax_out=16, amax_workspace=32)

# One fault (or an empty batch) per row: (ops, arith, replaced fields, expected code).  The codes of the x6 / h3 rows
# were recorded from the library before the linear entry points were folded into one validator (ABI 22).
GEMM_ROWS = [
    (_ALL, 7, {}, -1),  # unknown arith
    (_ALL, _X6, dict(M=-1), -1),
    (_ALL, _X6, dict(M=0), 0),  # empty batch: nothing launched
    (_ALL, _X6, dict(K=0), -1),
    (_ALL, _X6, dict(N=0), -1),
    (_ALL, _X6, dict(N=260), -1),
    ((_FWD, _ELU, _DGRAD, _OUT), _X6, dict(K=6), -1),  # K % 4
    ((_FWD, _ELU, _DGRAD, _OUT), _X6, dict(K=1 << 30), -1),  # K > INT32_MAX / 2
    ((_OUTBWD,), _X6, dict(K=17), -1),  # Nred > 16
    (_ALL, _X6, dict(a=None), -1),
    (_ALL, _X6, dict(bimage=None), -1),
    (_ALL, _X6, dict(a=8), -4),
    (_ALL, _X6, dict(bimage=24), -4),
    ((_FWD, _ELU, _OUT), _X6, dict(bias=None), -1),
    ((_FWD, _ELU, _DGRAD, _OUTBWD), _X6, dict(c=None), -1),
    ((_DGRAD, _OUTBWD), _X6, dict(h=None), -1),
    ((_OUTBWD,), _X6, dict(wgrad_partials=None), -1),
    ((_OUT,), _X6, dict(N=254), -1),  # N % 4
    ((_OUT,), _X6, dict(nout=0), -1),
    ((_OUT,), _X6, dict(nout=33), -1),
    ((_OUT,), _X6, dict(out_bias=None), -1),
    ((_OUT,), _X6, dict(out_image=None), -1),
    ((_OUT,), _X6, dict(y=None), -1),
    ((_OUT,), _X6, dict(bias=8), -4),
    ((_OUT,), _X6, dict(out_image=8), -4),
    ((_OUT,), _X6, dict(c=8), -4),
    ((_FWD, _ELU, _DGRAD, _OUTBWD), _X6, dict(amax_out=16), -1),  # amax_out without its workspace
    ((_OUT,), _X6, _AMAX, -3),  # no amax from the fused output layer
    ((_FWD, _ELU, _DGRAD, _OUT), _H3, dict(a_amax=None), -1),
    ((_OUTBWD,), _H3, {}, -3),  # the output-layer backward is x6 only
    ((9,), _X6, {}, -1),  # unknown op
]
# ABI 23: RSLRL_ARITH_F32 (bimage = the fp32 B operand itself)
GEMM_ROWS_F32 = [
    ((_FWD, _ELU, _DGRAD), _lib.ARITH_F32, dict(M=0), 0),
    ((_FWD, _ELU, _DGRAD), _lib.ARITH_F32, dict(K=6), -1),
    ((_FWD, _ELU, _DGRAD), _lib.ARITH_F32, dict(N=260), -1),
    ((_FWD, _ELU, _DGRAD), _lib.ARITH_F32, dict(bimage=None), -1),
    ((_FWD, _ELU, _DGRAD), _lib.ARITH_F32, dict(bimage=24), -4),
    ((_FWD, _ELU), _lib.ARITH_F32, dict(bias=None), -1),
    ((_DGRAD,), _lib.ARITH_F32, dict(h=None), -1),
    ((_DGRAD,), _lib.ARITH_F32, dict(colsum_partials=None), -1),  # the f32 kernel always writes them
    ((_FWD, _ELU, _DGRAD), _lib.ARITH_F32, _AMAX, -3),
    ((_OUT, _OUTBWD), _lib.ARITH_F32, {}, -3),
]
# rslrl_linear_gemm_pair: (ops, arith, fields of both problems, fields of problem 1 alone, expected code)
PAIR_ROWS = [
    (_ALL, _X6, dict(M=0), {}, 0),
    ((9,), _X6, {}, {}, -3),  # unknown op
    (_ALL, _X6, {}, dict(M=256), -1),
    (_ALL, _X6, {}, dict(N=128), -1),
    ((_FWD, _ELU, _DGRAD, _OUT), _X6, {}, dict(K=128), -1),
    ((_FWD, _ELU, _DGRAD), _X6, dict(amax_out=16, amax_workspace=32), {}, -1),  # one amax workspace for both
    (_ALL, _X6, dict(a=None), {}, -1),
    (_ALL, _X6, dict(bimage=24), {}, -4),
    ((_FWD, _ELU, _DGRAD, _OUTBWD), _X6, dict(c=None), {}, -1),
    ((_OUT,), _X6, dict(y=None), {}, -1),
    ((_FWD, _ELU, _DGRAD, _OUT), _X6, dict(K=6), {}, -1),
    ((_OUT,), _X6, dict(nout=33), {}, -1),
    ((_OUTBWD,), _X6, dict(K=17), {}, -1),
    ((_FWD, _ELU, _DGRAD), _H3, dict(a_amax=None), {}, -1),
]
PAIR_ROWS_F32 = [((_FWD, _ELU, _DGRAD), _lib.ARITH_F32, {}, {}, -3)]


@pytest.mark.parametrize("ops,arith,over,expected", GEMM_ROWS + GEMM_ROWS_F32)
def test_linear_gemm_validation_table(ops, arith, over, expected):
    L = _lib.lib()
    for op in ops:
        assert L.rslrl_linear_gemm(ctypes.byref(_linear_args(op, arith, **over)), None) == expected, op


@pytest.mark.parametrize("ops,arith,both,second,expected", PAIR_ROWS + PAIR_ROWS_F32)
def test_linear_gemm_pair_validation_table(ops, arith, both, second, expected):
    L = _lib.lib()
    for op in ops:
        a0 = _linear_args(op, arith, **both)
        a1 = _linear_args(op, arith, **{**both, **second})
        assert L.rslrl_linear_gemm_pair(ctypes.byref(a0), ctypes.byref(a1), None) == expected, op


def test_linear_gemm_pair_rejects_mixed_problems():
    L = _lib.lib()
    for op in (_FWD, _ELU, _DGRAD, _OUT):  # x6 beside h3
        a0, a1 = _linear_args(op, _X6), _linear_args(op, _H3)
        assert L.rslrl_linear_gemm_pair(ctypes.byref(a0), ctypes.byref(a1), None) == -1, op
    a0, a1 = _linear_args(_ELU), _linear_args(_FWD)
    assert L.rslrl_linear_gemm_pair(ctypes.byref(a0), ctypes.byref(a1), None) == -3  # two ops


def _value_head(**over):
    f = dict(target_values=16, returns=16, out_weight=16, wgrad_partials=16, colsum_partials=None)
    f.update(over)
    return _lib.ValueHeadArgs(f["target_values"], f["returns"], f["out_weight"], 0.2, 1.0, 1, f["wgrad_partials"],
                              f["colsum_partials"])


def _actor_head(**over):
    f = dict(actions=16, old_log_prob=16, advantages=16, values=16, target_values=16, returns=16, old_mu=16,
             old_sigma=16, sigma=16, num_actions=12, out_weight_t_image=16, wgrad_partials=16, grad_sigma=16, stats=16)
    f.update(over)
    return _lib.ActorHeadArgs(f["actions"], f["old_log_prob"], f["advantages"], f["values"], f["target_values"],
                              f["returns"], f["old_mu"], f["old_sigma"], f["sigma"], f["num_actions"], 0.2, 1.0, 0.01, 1,
                              1, f["out_weight_t_image"], f["wgrad_partials"], f["grad_sigma"], f["stats"], None)


# the heads take an RSLRL_LINEAR_FWD_OUT problem of their one shape: (op, arith, problem fields, head fields, code)
VALUE_HEAD_ROWS = [
    (_ELU, _X6, {}, {}, -1),  # not a FWD_OUT problem
    (_OUT, _X6, dict(M=0), {}, 0),
    (_OUT, _X6, dict(nout=2), {}, -3),
    (_OUT, _X6, dict(K=48), {}, -3),
    (_OUT, _X6, dict(N=128), {}, -3),
    (_OUT, _X6, dict(M=100), {}, -3),
    (_OUT, _H3, {}, {}, -3),
    (_OUT, _X6, _AMAX, {}, -3),
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
# ... and for the actor head (workspace pointer, workspace bytes) as well
ACTOR_HEAD_ROWS = [
    (_ELU, _X6, {}, {}, (16, 1 << 20), -1),
    (_OUT, _X6, dict(M=0), {}, (16, 1 << 20), -3),  # the fused loss divides by M
    (_OUT, _X6, dict(nout=1), {}, (16, 1 << 20), -3),
    (_OUT, _X6, {}, dict(num_actions=11), (16, 1 << 20), -3),
    (_OUT, _X6, dict(K=48), {}, (16, 1 << 20), -3),
    (_OUT, _X6, dict(M=100), {}, (16, 1 << 20), -3),
    (_OUT, _H3, {}, {}, (16, 1 << 20), -3),
    (_OUT, _X6, dict(bimage=None), {}, (16, 1 << 20), -1),
    (_OUT, _X6, dict(y=None), {}, (16, 1 << 20), -1),
    (_OUT, _X6, dict(c=None), {}, (16, 1 << 20), -1),
    (_OUT, _X6, dict(bias=8), {}, (16, 1 << 20), -4),
    (_OUT, _X6, {}, dict(actions=None), (16, 1 << 20), -1),
    (_OUT, _X6, {}, dict(sigma=None), (16, 1 << 20), -1),
    (_OUT, _X6, {}, dict(stats=None), (16, 1 << 20), -1),
    (_OUT, _X6, {}, dict(out_weight_t_image=8), (16, 1 << 20), -4),
    (_OUT, _X6, {}, {}, (None, 1 << 20), -1),
    (_OUT, _X6, {}, {}, (8, 1 << 20), -4),
    (_OUT, _X6, {}, {}, (16, 1024), -2),  # workspace too small
]
_HEAD_F32 = (_OUT, _lib.ARITH_F32, {}, {})


@pytest.mark.parametrize("op,arith,over,head,expected", VALUE_HEAD_ROWS + [_HEAD_F32 + (-3,)])
def test_value_head_validation_table(op, arith, over, head, expected):
    a = _linear_args(op, arith, **{"nout": 1, **over})
    rc = _lib.lib().rslrl_value_head_fwd_bwd(ctypes.byref(a), ctypes.byref(_value_head(**head)), None)
    assert rc == expected


@pytest.mark.parametrize("op,arith,over,head,ws,expected", ACTOR_HEAD_ROWS + [_HEAD_F32 + ((16, 1 << 20), -3)])
def test_actor_head_validation_table(op, arith, over, head, ws, expected):
    a = _linear_args(op, arith, **over)
    rc = _lib.lib().rslrl_actor_head_fwd_bwd(ctypes.byref(a), ctypes.byref(_actor_head(**head)), ws[0], ws[1], None)
    assert rc == expected


def test_pair_and_optimizer_abi_validation():
    L = _lib.lib()
    a0 = _lib.LinearArgs(_lib.LINEAR_FWD_ELU, _lib.ARITH_X6, 16, None, 128, 48, 256, 16, 16, None, 16)
    a1 = _lib.LinearArgs(_lib.LINEAR_FWD_ELU, _lib.ARITH_X6, 16, None, 64, 48, 256, 16, 16, None, 16)
    assert L.rslrl_linear_gemm_pair(ctypes.byref(a0), ctypes.byref(a1), None) == -1  # different M
    a1.M, a1.op = 128, _lib.LINEAR_DGRAD_ELU
    assert L.rslrl_linear_gemm_pair(ctypes.byref(a0), ctypes.byref(a1), None) == -3  # not a forward pair
    a1.op = _lib.LINEAR_FWD_ELU
    a0.M = a1.M = 0
    assert L.rslrl_linear_gemm_pair(ctypes.byref(a0), ctypes.byref(a1), None) == 0  # empty batch: no launch
    assert L.rslrl_linear_gemm_pair(None, ctypes.byref(a1), None) == -1
    args = _lib.AdamArgs()
    ws_bytes = L.rslrl_adam_workspace_bytes()
    assert ws_bytes >= 256 + 128 * 8 + 4
    args.n = 0
    assert L.rslrl_clip_adam_step(ctypes.byref(args), 16, ws_bytes, None) == -1  # no tensors
    args.n = _lib.ADAM_MAX_TENSORS + 1
    assert L.rslrl_clip_adam_step(ctypes.byref(args), 16, ws_bytes, None) == -1  # too many tensors
    args.n = 1
    assert L.rslrl_clip_adam_step(ctypes.byref(args), 16, ws_bytes - 1, None) == -2  # workspace too small
    assert L.rslrl_clip_adam_step(ctypes.byref(args), 16, ws_bytes, None) == -1  # null tensor pointers


def test_randperm_rejects_bad_state():
    L = _lib.lib()
    out = np.empty(10, np.int32)
    bad = np.zeros(100, np.uint8)
    assert L.rslrl_randperm_mt19937(bad.ctypes.data, bad.nbytes, 10, out.ctypes.data) == -5
    st = torch.Generator().manual_seed(0).get_state().numpy().copy()
    st[8:12] = np.frombuffer(np.int32(9999).tobytes(), np.uint8)  # left out of range
    assert L.rslrl_randperm_mt19937(st.ctypes.data, st.nbytes, 10, out.ctypes.data) == -5


def test_hot_path_refuses_cpu_tensors():
    from rsl_rl_amd import kernels

    t = torch.zeros(4, 3, 1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        kernels.compute_returns(t, t, t.to(torch.uint8), torch.zeros(3, 1), 0.99, 0.95, True, t.clone(), t.clone())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        kernels.normalize_advantages_(torch.zeros(8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        kernels.gather_rows([(torch.zeros(4, 2), torch.zeros(2, 2))], torch.zeros(2, dtype=torch.int32))


def test_golden_files_present():
    for f in ("gae.npz", "perm.npz", "minibatch.npz", "update_c1.npz", "golden.json"):
        assert os.path.exists(golden_path(f)), f
