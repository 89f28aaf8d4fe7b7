"""The fused actor head for 17 to 32 actions on a last hidden layer with 128 inputs, host side: what
rslrl_actor_head_wide_fwd_bwd_k128 takes and refuses before any launch (fake pointers, never dereferenced), its
workspace size, and the same rule in fused_mlp.actor_head_wide_fwd_bwd's (N, K) dispatch and fused_mlp._pairable with the
RSLRL_ACTOR_HEAD_WIDE_K128 knob (the module flag) on and off."""

import ctypes

import pytest
import torch

from rsl_rl_amd import _lib
from rsl_rl_amd.networks import fused_mlp

FN = "rslrl_actor_head_wide_fwd_bwd_k128"


def _call(ws=(16, 1 << 24), arith=_lib.ARITH_X6, M=128, K=128, N=128, nout=24, num_actions=None, actions=16):
    lin = _lib.LinearArgs(_lib.LINEAR_FWD_OUT, arith, 16, None, M, K, N, 16, 16, 16, 16, 16, 16, 16, 16, 16, nout, None,
                          None)
    head = _lib.ActorHeadArgs(actions, 16, 16, 16, 16, 16, 16, 16, 16, nout if num_actions is None else num_actions,
                              0.2, 1.0, 0.01, 1, 1, 16, 16, 16, 16, None)
    return getattr(_lib.lib(), FN)(ctypes.byref(lin), ctypes.byref(head), ws[0], ws[1], None)


# -3 = out of the head's scope, -1 = in scope (the null pointer is found next)
ROWS = [(dict(nout=16), -3), (dict(nout=33), -3), (dict(K=256), -3), (dict(N=192), -3), (dict(N=256), -3),
        (dict(M=100), -3), (dict(arith=_lib.ARITH_H3), -3), (dict(num_actions=20), -3)]
ROWS += [(dict(nout=A, N=N, actions=None), -1) for A, N in ((17, 64), (19, 128), (32, 128))]


@pytest.mark.parametrize("kw,expected", ROWS)
def test_validation_table(kw, expected):
    assert _call(**kw) == expected


@pytest.mark.parametrize("M", [64, 192, 64 * 513, 64 * 100000])
def test_workspace_is_36_columns_per_slice_and_fold_group(M):
    L = _lib.lib()
    S = L.rslrl_head_k128_partial_rows(M)
    need = L.rslrl_actor_head_wide_k128_workspace_bytes(M)
    assert 1 <= S <= 512 and need == 1024 + 8 * 36 * (S + (S + 63) // 64)
    assert _call(ws=(16, need - 4), M=M, nout=32) == -2
    assert _call(ws=(16, need), M=M, nout=32, actions=None) == -1


def _wide_head(A, M=128):
    z = lambda *s: torch.zeros(*s)  # noqa: E731
    return fused_mlp.ActorHeadWide(z(M, A), z(M, 1), z(M, 1), z(M, 1), z(M, 1), z(M, A), z(M, A), torch.ones(A),
                                   clip_param=0.2, value_loss_coef=1.0, entropy_coef=0.01, use_clipped=True,
                                   compute_kl=True, grad_sigma=z(A), stats=z(8))


@pytest.mark.parametrize("on", [True, False])
def test_layer_rule_and_pairable_follow_the_knob(on, monkeypatch):
    monkeypatch.setattr(fused_mlp, "_ACTOR_HEAD_WIDE_K128", on)
    monkeypatch.setattr(fused_mlp, "_PAIR_TRAIN", True)
    ok = fused_mlp._actor_head_wide_layer_ok
    assert all(ok(N, 256) for N in (64, 128, 192, 256))  # the 256-input entry's shapes do not read this knob
    assert [ok(N, 128) for N in (64, 128, 192, 256)] == [on, on, False, False] and not ok(128, 64)
    ws = lambda out: [torch.zeros(128, 48), torch.zeros(128, 128), torch.zeros(128, 128), torch.zeros(out, 128)]  # noqa: E731
    x = torch.zeros(128, 48)
    base = fused_mlp._pairable(ws(12), ws(1), x, x)  # (False where the build's GEMM mode is not x6: nothing pairs)
    assert fused_mlp._pairable(ws(19), ws(1), x, x) is False
    assert fused_mlp._pairable(ws(19), ws(1), x, x, _wide_head(19)) == (base and on)
    assert fused_mlp._pairable(ws(19), ws(1), x, x, _wide_head(24)) is False  # another width's head
    x64 = torch.zeros(64, 48)  # the C entry takes 64 rows; ActorHeadWide.supported keeps whole 128-row tiles
    assert fused_mlp._pairable(ws(19), ws(1), x64, x64, _wide_head(19, 64)) is False
    monkeypatch.setattr(fused_mlp, "_HEAD_K128", False)  # the critic's head runs first: without it the actor's cannot
    assert fused_mlp._pairable(ws(19), ws(1), x, x, _wide_head(19)) is False
