"""The fused actor head for 5 to 16 actions (ABI 33), host side: what rslrl_actor_head_fwd_bwd takes and refuses before
any launch (fake pointers, never dereferenced: every row has one fault or stops at a null pointer), and the same rule in
ActorHead.supported and PPO._loss_heads with the RSLRL_ACTOR_HEAD_ANY knob on and off."""

import ctypes
from types import SimpleNamespace

import pytest
import torch

from rsl_rl_amd import _lib
from rsl_rl_amd.algorithms import PPO
from rsl_rl_amd.networks import fused_mlp

_WS = (16, 1 << 20)


def _linear(**over):
    f = dict(a=16, M=128, K=256, N=256, bimage=16, bias=16, h=16, c=16, out_image=16, out_bias=16, y=16, nout=12)
    f.update(over)
    return _lib.LinearArgs(_lib.LINEAR_FWD_OUT, _lib.ARITH_X6, f["a"], None, f["M"], f["K"], f["N"], f["bimage"],
                           f["bias"], f["h"], f["c"], 16, 16, f["out_image"], f["out_bias"], f["y"], f["nout"], None,
                           None)


def _head(**over):
    f = dict(actions=16, num_actions=12)
    f.update(over)
    return _lib.ActorHeadArgs(f["actions"], 16, 16, 16, 16, 16, 16, 16, 16, f["num_actions"], 0.2, 1.0, 0.01, 1, 1, 16,
                              16, 16, 16, None)


def _call(lin, head, ws=_WS):
    return _lib.lib().rslrl_actor_head_fwd_bwd(ctypes.byref(_linear(**lin)), ctypes.byref(_head(**head)), ws[0],
                                               ws[1], None)


# (problem fields, head fields, code): -3 = out of the head's scope, -1 = in scope (the null pointer is found next)
ROWS = [
    (dict(nout=4), dict(num_actions=4), -3),
    (dict(nout=17), dict(num_actions=17), -3),
    (dict(nout=10), dict(num_actions=9), -3),
    (dict(nout=10), dict(num_actions=10, actions=None), -1),
] + [(dict(nout=A), dict(num_actions=A, actions=None), -1) for A in (5, 8, 13, 16)]


@pytest.mark.parametrize("lin,head,expected", ROWS)
def test_actor_head_anya_validation_table(lin, head, expected):
    assert _call(lin, head) == expected


@pytest.mark.parametrize("A", [5, 10, 12, 16])
@pytest.mark.parametrize("M", [128, 8320, 4097 * 128])
def test_actor_head_workspace_is_sized_for_20_columns(A, M):
    L = _lib.lib()
    need = L.rslrl_actor_head_workspace_bytes(M)
    tiles = M // 128
    assert need >= 1024 + 8 * 20 * (tiles + (tiles + 127) // 128)  # [20][tiles] + [20][groups] fp64 behind the tickets
    assert _call(dict(nout=A, M=M), dict(num_actions=A), (16, need - 8)) == -2
    # (the exact size passes the workspace check: the launch itself needs a GPU, tests/test_gpu_actor_head_anya.py)


def test_abi_version():
    assert _lib.lib().rslrl_abi_version() >= 33
    assert (_lib.ACTOR_HEAD_MIN_ACTIONS, _lib.ACTOR_HEAD_ACTIONS, _lib.ACTOR_HEAD_MAX_ACTIONS) == (5, 12, 16)


def _actor_head(A, M=128):
    z = lambda *s: torch.zeros(*s)  # noqa: E731
    return fused_mlp.ActorHead(z(M, A), z(M, 1), z(M, 1), z(M, 1), z(M, 1), z(M, A), z(M, A), torch.ones(A),
                               clip_param=0.2, value_loss_coef=1.0, entropy_coef=0.01, use_clipped=True,
                               compute_kl=True, grad_sigma=z(A), stats=z(8))


@pytest.mark.parametrize("any_on", [True, False])
def test_supported_follows_the_width_rule(any_on, monkeypatch):
    monkeypatch.setattr(_lib, "ACTOR_HEAD_ANY", any_on)
    for A in range(1, 21):
        want = (5 <= A <= 16) if any_on else A == 12
        assert _actor_head(A).supported(128) == want, A
        assert _lib.actor_head_width_ok(A) == want, A
    head = _actor_head(10)
    head.grad_sigma = torch.zeros(12)  # a destination of another width
    assert not head.supported(128)
    assert not _actor_head(10, M=128).supported(256)


@pytest.mark.parametrize("any_on", [True, False])
def test_loss_heads_builds_the_head_for_5_to_16(any_on, monkeypatch):
    monkeypatch.setattr(_lib, "ACTOR_HEAD_ANY", any_on)
    M = 128
    for A in range(1, 21):
        z = lambda *s: torch.zeros(*s)  # noqa: E731
        stored = (z(M, A), z(M, 1), z(M, 1), z(M, 1), z(M, 1), z(M, A), z(M, A))
        alg = SimpleNamespace(clip_param=0.2, value_loss_coef=1.0, entropy_coef=0.01, use_clipped_value_loss=True,
                              normalize_advantage_per_mini_batch=False,
                              policy=SimpleNamespace(state_dependent_std=False),
                              _grad_sigma_dest=lambda arena, width, dev: torch.zeros(width))
        u = SimpleNamespace(adaptive=True, arena=None, dev=torch.device("cpu"), stats_buf=z(8))
        vh, ah = PPO._loss_heads(alg, u, stored)
        assert vh is not None
        assert (ah is not None) == ((5 <= A <= 16) if any_on else A == 12), A
        if ah is not None:
            assert ah.grad_sigma.numel() == A
        alg.normalize_advantage_per_mini_batch = True  # not fused at any width
        assert PPO._loss_heads(alg, u, stored)[1] is None
