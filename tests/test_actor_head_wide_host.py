"""The fused actor head for 17 to 32 actions, host side: what rslrl_actor_head_wide_fwd_bwd takes and refuses before any
launch (fake pointers, never dereferenced), its workspace size, and the same rule in ActorHeadWide.supported,
PPO._loss_head_wide and fused_mlp._pairable with the RSLRL_ACTOR_HEAD_WIDE knob on and off."""

import ctypes
from types import SimpleNamespace

import pytest
import torch

from rsl_rl_amd import _lib
from rsl_rl_amd.algorithms import PPO
from rsl_rl_amd.networks import fused_mlp


def _call(fn, ws=(16, 1 << 24), arith=_lib.ARITH_X6, M=128, K=256, N=256, nout=24, num_actions=None, actions=16):
    lin = _lib.LinearArgs(_lib.LINEAR_FWD_OUT, arith, 16, None, M, K, N, 16, 16, 16, 16, 16, 16, 16, 16, 16, nout, None,
                          None)
    head = _lib.ActorHeadArgs(actions, 16, 16, 16, 16, 16, 16, 16, 16, nout if num_actions is None else num_actions,
                              0.2, 1.0, 0.01, 1, 1, 16, 16, 16, 16, None)
    return getattr(_lib.lib(), fn)(ctypes.byref(lin), ctypes.byref(head), ws[0], ws[1], None)


# -3 = out of the head's scope, -1 = in scope (the null pointer is found next)
ROWS = [(dict(nout=16), -3), (dict(nout=33), -3), (dict(N=96), -3), (dict(N=320), -3), (dict(K=128), -3),
        (dict(arith=_lib.ARITH_H3), -3), (dict(M=1000), -3), (dict(num_actions=20), -3)]
ROWS += [(dict(nout=A, N=N, actions=None), -1) for A, N in ((17, 256), (20, 64), (29, 128), (32, 192))]


@pytest.mark.parametrize("kw,expected", ROWS)
def test_wide_head_validation_table(kw, expected):
    assert _call("rslrl_actor_head_wide_fwd_bwd", **kw) == expected


@pytest.mark.parametrize("fn", ["rslrl_actor_head_fwd_bwd", "rslrl_actor_head_fwd_bwd_n"])
def test_the_other_heads_still_refuse_17(fn):
    assert _call(fn, nout=17, N=256 if fn.endswith("bwd") else 128) == -3


@pytest.mark.parametrize("tiles", [1, 65, 4097])
def test_wide_head_workspace_is_sized_for_36_columns(tiles):
    M = 128 * tiles
    need = _lib.lib().rslrl_actor_head_wide_workspace_bytes(M)
    # behind the tickets: the loss's [36][tiles] + [36][groups of 64] fp64, then db's [32][tiles] + [32][groups of 64]
    assert need == 1024 + 8 * (36 + 32) * (tiles + (tiles + 63) // 64)
    assert _call("rslrl_actor_head_wide_fwd_bwd", ws=(16, need - 8), M=M, nout=32) == -2
    assert _call("rslrl_actor_head_wide_fwd_bwd", ws=(16, need), M=M, nout=32, actions=None) == -1


def _wide_head(A, M=128):
    z = lambda *s: torch.zeros(*s)  # noqa: E731
    return fused_mlp.ActorHeadWide(z(M, A), z(M, 1), z(M, 1), z(M, 1), z(M, 1), z(M, A), z(M, A), torch.ones(A),
                                   clip_param=0.2, value_loss_coef=1.0, entropy_coef=0.01, use_clipped=True,
                                   compute_kl=True, grad_sigma=z(A), stats=z(8))


@pytest.mark.parametrize("on", [True, False])
def test_supported_and_the_ppo_step_follow_the_width_rule(on, monkeypatch):
    monkeypatch.setattr(_lib, "ACTOR_HEAD_WIDE", on)
    assert (_lib.ACTOR_HEAD_WIDE_MIN_ACTIONS, _lib.ACTOR_HEAD_WIDE_MAX_ACTIONS, _lib.ACTOR_HEAD_MAX_ACTIONS) == (17, 32, 16)
    z = lambda *s: torch.zeros(*s)  # noqa: E731
    for A in range(12, 37):
        want = on and 17 <= A <= 32
        assert _lib.actor_head_wide_ok(A) == want and _wide_head(A).supported(128) == want, A
        assert not _lib.actor_head_width_ok(A) or A <= 16
        stored = (z(128, A), z(128, 1), z(128, 1), z(128, 1), z(128, 1), z(128, A), z(128, A))
        alg = SimpleNamespace(clip_param=0.2, value_loss_coef=1.0, entropy_coef=0.01, use_clipped_value_loss=True,
                              normalize_advantage_per_mini_batch=False,
                              policy=SimpleNamespace(state_dependent_std=False),
                              _grad_sigma_dest=lambda arena, width, dev: torch.zeros(width))
        u = SimpleNamespace(adaptive=True, arena=None, dev=torch.device("cpu"), stats_buf=z(8))
        ah = PPO._loss_head_wide(alg, u, stored)
        assert isinstance(ah, fused_mlp.ActorHeadWide) == want, A
        assert PPO._loss_head_wide(alg, u, stored, "given") == "given"  # _loss_heads' head stays
        alg.normalize_advantage_per_mini_batch = True
        assert PPO._loss_head_wide(alg, u, stored) is None
    assert not _wide_head(24, M=1000).supported(1000) and not _wide_head(24).supported(256)
    assert not fused_mlp.ActorHead.supported(_wide_head(24), 128)  # the 5..16 rule is unchanged


def test_pairable_admits_a_wide_actor_only_with_its_head(monkeypatch):
    monkeypatch.setattr(fused_mlp, "_PAIR_TRAIN", True)
    ws = lambda out: [torch.zeros(256, 48), torch.zeros(256, 256), torch.zeros(256, 256), torch.zeros(out, 256)]  # noqa: E731
    x = torch.zeros(128, 48)
    base = fused_mlp._pairable(ws(12), ws(1), x, x)  # (False where the build's GEMM mode is not x6: nothing pairs)
    assert fused_mlp._pairable(ws(24), ws(1), x, x) is False
    assert fused_mlp._pairable(ws(24), ws(1), x, x, _wide_head(24)) == base
    assert fused_mlp._pairable(ws(24), ws(1), x, x, _wide_head(20)) is False  # another width's head
    assert fused_mlp._pairable(ws(24), ws(1), torch.zeros(1000, 48), torch.zeros(1000, 48), _wide_head(24, 1000)) is False
    monkeypatch.setattr(_lib, "ACTOR_HEAD_WIDE", False)
    assert fused_mlp._pairable(ws(24), ws(1), x, x, _wide_head(24)) is False
