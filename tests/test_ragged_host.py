"""The ragged first layer without a GPU: ABI 30's symbols and size functions, the argument validation of
the two entry points (every call below is rejected on its arguments, or is an empty batch: nothing is launched), the
weight images at a depth that is no multiple of 4, and the structure predicates -- ragged_structure, MLP._ragged and
ActorCritic.ragged_update_structure_ok beside the older ones, which keep refusing these stacks."""

import ctypes
import importlib
import os
import subprocess
import sys

import torch

from rsl_rl_amd import _lib
from rsl_rl_amd.modules import ActorCritic
from rsl_rl_amd.networks import MLP, fused_mlp

P = 4096  # never dereferenced
RAGGED = ((50, [256]), (235, [512, 256, 128]), (77, [320, 64]), (19, [64, 64]))
# (1027, [256, 256]), (1029, ...), (2049, ...): an input wider than the entry points' K <= 1024, whatever the stack
NOT_RAGGED = ((48, [256, 256]), (48, [512, 256, 128]), (235, [512, 512]), (1027, [512, 256]), (1027, [256, 256]),
              (1029, [256, 128]), (2049, [128, 128]))


def _args(op=_lib.LINEAR_FWD_ELU, **kw):
    base = dict(op=op, arith=_lib.ARITH_X6, a=P, M=200, K=235, N=512, bimage=P * 2, bias=P * 3, c=P * 5)
    base.update(kw)
    return _lib.LinearArgs(**base)


def _gemm(**kw):
    return _lib.lib().rslrl_linear_gemm_ragged(ctypes.byref(_args(**kw)), None)


def test_abi_30_symbols_and_sizes():
    L = _lib.lib()
    assert L.rslrl_abi_version() == _lib.ABI_VERSION >= 30
    for name in ("rslrl_linear_gemm_ragged", "rslrl_linear_wgrad_bias_ragged",
                 "rslrl_linear_wgrad_bias_ragged_workspace_bytes"):
        assert hasattr(L, name) and name in _lib.EXPORTED_SYMBOLS, name
    ws = L.rslrl_linear_wgrad_bias_ragged_workspace_bytes
    for k0, hidden in RAGGED:
        n = hidden[0]
        # the image functions take the depth as it is
        assert L.rslrl_linear_bimage_bytes(k0) == L.rslrl_linear_bimage_bytes(k0 + (-k0) % 4) > 0
        assert L.rslrl_linear_bimage_wide_bytes(n, k0) > 0
        if fused_mlp.ragged_wgrad_ok(n, k0):
            bias = 1 if n > 64 else 0
            assert ws(3001, n, k0, bias) >= 4 * (n * k0 + bias * n) and ws(3001, n, k0, bias) % 16 == 0, (k0, n)
        else:  # (19, [64, 64]): K, N <= 64 has no split-kernel form, as for a 20-wide input -- that stack's first-layer
            # weight gradient stays on the split-K fallback inside the manual update (README)
            assert (k0, n) == (19, 64) and ws(3001, n, k0, 0) == 0 and fused_mlp._wgrad_form(n, k0, True) is None
    assert fused_mlp.ragged_wgrad_ok(256, 50) and fused_mlp.ragged_wgrad_ok(512, 235) and fused_mlp.ragged_wgrad_ok(320, 77)
    assert not fused_mlp.ragged_wgrad_ok(64, 19) and not fused_mlp.ragged_wgrad_ok(512, 236)
    assert ws(3001, 512, 236, 1) == 0 and ws(3001, 512, 1027, 1) == 0 and ws(3001, 510, 235, 1) == 0
    assert ws(3001, 64, 235, 1) == 0 and ws(3001, 64, 235, 0) > 0 and ws(0, 512, 235, 1) == 0


def test_gemm_ragged_validates_before_any_launch():
    for op in (_lib.LINEAR_FWD, _lib.LINEAR_FWD_ELU):
        for kw in (dict(K=236), dict(K=48), dict(K=1027), dict(K=0), dict(N=1028), dict(N=258), dict(N=0)):
            assert _gemm(op=op, **kw) == _lib.E_UNSUPPORTED, kw
        for kw in (dict(a=None), dict(bimage=None), dict(c=None), dict(bias=None)):
            assert _gemm(op=op, **kw) == _lib.E_INVALID_ARGUMENT, kw
        assert _gemm(op=op, M=-1) == _lib.E_INVALID_ARGUMENT
        assert _gemm(op=op, a=P + 4) == _lib.E_MISALIGNED and _gemm(op=op, c=P * 5 + 8) == _lib.E_MISALIGNED
        assert _gemm(op=op, bimage=P * 2 + 4) == _lib.E_MISALIGNED
        assert _gemm(op=op, M=0) == 0 and _gemm(op=op, M=0, K=236) == _lib.E_UNSUPPORTED
    for op in (_lib.LINEAR_DGRAD_ELU, _lib.LINEAR_FWD_OUT, _lib.LINEAR_DGRAD_ELU_WGRAD, 7):
        assert _gemm(op=op) == _lib.E_UNSUPPORTED, op
    for arith in (_lib.ARITH_F32, _lib.ARITH_H3):
        assert _gemm(arith=arith) == _lib.E_UNSUPPORTED, arith
    assert _gemm(amax_out=P * 7, amax_workspace=P * 8) == _lib.E_UNSUPPORTED
    assert _lib.lib().rslrl_linear_gemm_ragged(None, None) == _lib.E_INVALID_ARGUMENT
    # the existing entry points keep their K % 4 == 0 rule
    a = _args(K=235, N=256)
    assert _lib.lib().rslrl_linear_gemm(ctypes.byref(a), None) == _lib.E_INVALID_ARGUMENT
    assert _lib.lib().rslrl_linear_gemm_wide(ctypes.byref(_args()), None) == _lib.E_UNSUPPORTED


def test_wgrad_ragged_validates_before_any_launch():
    wg = _lib.lib().rslrl_linear_wgrad_bias_ragged
    big = 1 << 40

    def call(dz=P, x=P * 2, M=3001, N=512, K=235, bias=1, out=P * 3, ws=P * 4, nbytes=big):
        return wg(dz, x, M, N, K, bias, out, ws, nbytes, None)

    for kw in (dict(K=236), dict(K=1027), dict(K=0), dict(N=1028), dict(N=258), dict(bias=2), dict(bias=-1),
               dict(N=64, bias=1), dict(N=64, K=19, bias=0), dict(N=32, K=235, bias=0)):
        assert call(**kw) == _lib.E_UNSUPPORTED, kw
    for kw in (dict(dz=None), dict(x=None), dict(out=None), dict(ws=None)):
        assert call(**kw) == _lib.E_INVALID_ARGUMENT, kw
    assert call(M=-1) == _lib.E_INVALID_ARGUMENT
    assert call(dz=P + 4) == _lib.E_MISALIGNED and call(x=P * 2 + 8) == _lib.E_MISALIGNED
    assert call(nbytes=1024) == -2  # RSLRL_E_WORKSPACE_TOO_SMALL
    assert call(M=0) == 0 and call(M=0, K=236) == _lib.E_UNSUPPORTED
    assert call(K=19, N=256, M=0) == 0 and call(K=1021, M=0) == 0 and call(N=64, bias=0, M=0) == 0


def test_ragged_structure_truth_table():
    for k0, hidden in RAGGED:
        m = MLP(k0, 12, hidden)
        assert fused_mlp.ragged_structure(m) and m._ragged, (k0, hidden)
        assert not m._fused and not m._wide, (k0, hidden)
        assert not fused_mlp.fusable_structure(m) and not fused_mlp.wide_structure(m), (k0, hidden)
        first = m[0]
        assert isinstance(first, torch.nn.Linear) and tuple(first.weight.shape) == (hidden[0], k0)
        sd = m.state_dict()
        assert list(sd)[:2] == ["0.weight", "0.bias"] and tuple(sd["0.weight"].shape) == (hidden[0], k0)
    for k0, hidden in NOT_RAGGED:
        m = MLP(k0, 12, hidden)
        assert not fused_mlp.ragged_structure(m) and not m._ragged, (k0, hidden)
    assert not MLP(235, 12, [512, 256, 128], activation="relu")._ragged
    assert not fused_mlp.ragged_structure(MLP(235, 12, [510, 256]))  # a ragged hidden width stays out of scope
    assert MLP(235, [2, 12], [512, 256, 128])._ragged  # a state-dependent-std head
    # which ragged stacks have wide layers (and follow the wide stacks' row threshold and knob): by outputs or inputs
    assert fused_mlp.ragged_wide_stack(MLP(1021, 12, [256, 128])) and fused_mlp.ragged_wide_stack(MLP(235, 12, [512, 256, 128]))
    assert not fused_mlp.ragged_wide_stack(MLP(235, 12, [256, 256])) and not fused_mlp.ragged_wide_stack(MLP(19, 12, [64, 64]))
    x = torch.zeros(8, 19)
    with torch.no_grad():  # a forward nothing differentiates: by rows
        assert fused_mlp.ragged_forward_ok(MLP(19, 12, [64, 64]), x) == (8 >= fused_mlp.RAGGED_FWD_MIN_ROWS)
        big = torch.zeros(fused_mlp.RAGGED_FWD_MIN_ROWS, 19)
        assert fused_mlp.ragged_forward_ok(MLP(19, 12, [64, 64]), big)
        assert not fused_mlp.ragged_forward_ok(MLP(1021, 12, [256, 128]), torch.zeros(8, 1021))
    assert fused_mlp.ragged_forward_ok(MLP(19, 12, [64, 64]), x)  # under autograd: always


def test_rnd_keeps_its_own_width_rules():
    """RND's networks are out of the feature's scope: a 33-wide gated state (tests/test_gpu_rnd.py) stays on the path it
    had, layer by layer, whatever the knob says."""
    from rsl_rl_amd.modules.rnd import RandomNetworkDistillation

    rnd = RandomNetworkDistillation(33, {"rnd_state": ["policy"]}, 4, [40], [40])
    assert fused_mlp.ragged_structure(rnd.predictor) and not rnd.predictor._ragged and not rnd.target._ragged
    assert not rnd.predictor._fused and not rnd.predictor._wide


def _policy(k0, actor, critic, **kw):
    groups = {"policy": ["policy"], "critic": ["policy"]}
    return ActorCritic({"policy": torch.zeros(4, k0)}, groups, 12, actor_hidden_dims=actor, critic_hidden_dims=critic, **kw)


def test_update_predicates():
    for k0, hidden in RAGGED:
        pol = _policy(k0, hidden, hidden)
        assert not pol.manual_update_structure_ok(), (k0, hidden)  # the older predicate keeps its answer
        assert pol.ragged_update_structure_ok() and pol.has_ragged_mlp, (k0, hidden)
        assert not pol.manual_update_ok({"policy": torch.zeros(4, k0)})  # CPU observations
    for k0, hidden in NOT_RAGGED:
        pol = _policy(k0, hidden, hidden)
        assert not pol.ragged_update_structure_ok() and not pol.has_ragged_mlp, (k0, hidden)
    assert not _policy(235, [512, 256, 128], [512, 512]).ragged_update_structure_ok()
    assert not _policy(235, [512, 256, 128], [512, 256, 128], activation="relu").ragged_update_structure_ok()
    prev = fused_mlp.set_gemm_mode(fused_mlp.GEMM_F32)  # ragged stacks run fused in x6 arithmetic only
    try:
        assert not fused_mlp.ragged_enabled()
        assert not _policy(235, [512, 256, 128], [512, 256, 128]).ragged_update_structure_ok()
    finally:
        fused_mlp.set_gemm_mode(prev)
    assert fused_mlp.ragged_enabled()
    # the forms: a ragged width takes the ragged entry where its padded width has a split-kernel form
    assert fused_mlp._wgrad_form(256, 50, True) == "ragged" and fused_mlp._wgrad_form(512, 235, True, True) == "ragged"
    assert fused_mlp._wgrad_form(64, 19, True) is None and fused_mlp._wgrad_form(256, 48, True) == "first"
    assert fused_mlp._bias_from_wgrad(256, 235, True) and not fused_mlp._bias_from_wgrad(64, 235, True)


def test_knob_off_keeps_the_old_routing():
    code = ("from rsl_rl_amd.networks import MLP, fused_mlp\n"
            "m = MLP(235, 12, [512, 256, 128])\n"
            "assert fused_mlp.ragged_structure(m) and not m._ragged and not m._fused and not m._wide\n"
            "assert not fused_mlp.ragged_enabled() and fused_mlp._wgrad_form(256, 50, True) == 'first'\n")
    env = dict(os.environ, RSLRL_RAGGED_INPUT="0")
    root = os.path.dirname(os.path.dirname(os.path.abspath(importlib.import_module("rsl_rl_amd").__file__)))
    env["PYTHONPATH"] = root + os.pathsep + env.get("PYTHONPATH", "")
    subprocess.run([sys.executable, "-c", code], check=True, env=env, cwd=root)
