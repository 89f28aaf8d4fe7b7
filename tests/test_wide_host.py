"""The wide MLP path without a GPU: ABI 29's symbols and size functions, the argument validation of
the three entry points (every call below is rejected on its arguments, or is an empty batch: nothing is launched), and
the structure predicates -- wide_structure, fusable_structure, MLP._wide and ActorCritic.manual_update_structure_ok; and
the launch-plan mirror of tests/wide_plan.py against the library's workspace sizes, with the list of shapes that take
the full-tile kernel variants."""

import ctypes

import pytest
import torch
import torch.nn as nn

import wide_plan
from rsl_rl_amd import _lib
from rsl_rl_amd.modules import ActorCritic
from rsl_rl_amd.networks import MLP, fused_mlp

P = 4096  # never dereferenced
SYMBOLS = ("rslrl_linear_gemm_wide", "rslrl_linear_prepare_bimage_wide", "rslrl_linear_wgrad_bias_wide",
           "rslrl_linear_bimage_wide_bytes", "rslrl_linear_wgrad_bias_wide_workspace_bytes")


def _args(op=_lib.LINEAR_FWD_ELU, **kw):
    base = dict(op=op, arith=_lib.ARITH_X6, a=P, M=200, K=48, N=512, bimage=P * 2, bias=P * 3, h=P * 4, c=P * 5,
                colsum_partials=P * 6)
    base.update(kw)
    return _lib.LinearArgs(**base)


def _gemm(**kw):
    return _lib.lib().rslrl_linear_gemm_wide(ctypes.byref(_args(**kw)), None)


def test_abi_29_symbols_and_sizes():
    L = _lib.lib()
    assert L.rslrl_abi_version() == _lib.ABI_VERSION >= 29
    for name in SYMBOLS:
        assert hasattr(L, name) and name in _lib.EXPORTED_SYMBOLS, name
    one = L.rslrl_linear_bimage_bytes
    assert L.rslrl_linear_bimage_wide_bytes(512, 48) == 2 * one(48)
    assert L.rslrl_linear_bimage_wide_bytes(260, 320) == 2 * one(320)
    assert L.rslrl_linear_bimage_wide_bytes(256, 512) == one(512)
    assert L.rslrl_linear_bimage_wide_bytes(1024, 1024) == 4 * one(1024)
    assert L.rslrl_linear_bimage_wide_bytes(1025, 48) == 0 and L.rslrl_linear_bimage_wide_bytes(48, 1025) == 0
    ws = L.rslrl_linear_wgrad_bias_wide_workspace_bytes
    assert ws(3001, 512, 512, 1) >= 4 * (512 * 512 + 512) and ws(3001, 512, 512, 1) % 16 == 0
    assert ws(3001, 1028, 512, 0) == 0 and ws(3001, 512, 6, 0) == 0 and ws(3001, 48, 512, 1) == 0 and ws(0, 512, 512, 0) == 0


@pytest.mark.parametrize("op", [_lib.LINEAR_FWD, _lib.LINEAR_FWD_ELU, _lib.LINEAR_DGRAD_ELU])
def test_gemm_wide_validates_before_any_launch(op):
    for kw in (dict(N=1028), dict(N=258), dict(K=1028), dict(K=6), dict(N=0), dict(K=0)):
        assert _gemm(op=op, **kw) == _lib.E_UNSUPPORTED, kw
    assert _gemm(op=op, bimage=None) == _lib.E_INVALID_ARGUMENT
    assert _gemm(op=op, a=None) == _lib.E_INVALID_ARGUMENT and _gemm(op=op, c=None) == _lib.E_INVALID_ARGUMENT
    assert _gemm(op=op, M=-1) == _lib.E_INVALID_ARGUMENT
    assert _gemm(op=op, c=P * 5 + 4) == _lib.E_MISALIGNED
    assert _gemm(op=op, a=P + 8) == _lib.E_MISALIGNED and _gemm(op=op, bimage=P * 2 + 4) == _lib.E_MISALIGNED
    assert _gemm(op=op, M=0) == 0  # an empty batch: nothing to launch
    assert _gemm(op=op, M=0, N=1028) == _lib.E_UNSUPPORTED  # the shape is checked first


def test_gemm_wide_ops_and_arithmetics():
    assert _gemm(bias=None) == _lib.E_INVALID_ARGUMENT  # the forward needs the bias,
    assert _gemm(op=_lib.LINEAR_DGRAD_ELU, h=None) == _lib.E_INVALID_ARGUMENT  # the input gradient h
    assert _gemm(op=_lib.LINEAR_DGRAD_ELU, h=P * 4 + 4) == _lib.E_MISALIGNED
    for op in (_lib.LINEAR_FWD_OUT, _lib.LINEAR_DGRAD_ELU_WGRAD, 7):
        assert _gemm(op=op) == _lib.E_UNSUPPORTED, op
    for arith in (_lib.ARITH_F32, _lib.ARITH_H3):
        assert _gemm(arith=arith) == _lib.E_UNSUPPORTED, arith
    assert _gemm(amax_out=P * 7, amax_workspace=P * 8) == _lib.E_UNSUPPORTED
    assert _lib.lib().rslrl_linear_gemm_wide(None, None) == _lib.E_INVALID_ARGUMENT


def test_image_and_wgrad_validate_before_any_launch():
    L = _lib.lib()
    img = L.rslrl_linear_prepare_bimage_wide
    assert img(P, 1028, 48, 0, P * 2, None) == _lib.E_UNSUPPORTED and img(P, 512, 1028, 1, P * 2, None) == _lib.E_UNSUPPORTED
    assert img(P, 0, 48, 0, P * 2, None) == _lib.E_UNSUPPORTED
    assert img(None, 512, 48, 0, P * 2, None) == _lib.E_INVALID_ARGUMENT
    assert img(P, 512, 48, 0, None, None) == _lib.E_INVALID_ARGUMENT
    assert img(P, 512, 48, 1, P * 2 + 8, None) == _lib.E_MISALIGNED
    wg = L.rslrl_linear_wgrad_bias_wide
    big = 1 << 40

    def call(dz=P, x=P * 2, M=3001, N=512, K=512, side=1, out=P * 3, ws=P * 4, nbytes=big):
        return wg(dz, x, M, N, K, side, out, ws, nbytes, None)

    for kw in (dict(N=1028), dict(N=258), dict(K=1028), dict(K=6), dict(side=3), dict(side=-1), dict(N=64, side=1)):
        assert call(**kw) == _lib.E_UNSUPPORTED, kw
    for kw in (dict(dz=None), dict(x=None), dict(out=None), dict(ws=None)):
        assert call(**kw) == _lib.E_INVALID_ARGUMENT, kw
    assert call(M=-1) == _lib.E_INVALID_ARGUMENT
    assert call(dz=P + 4) == _lib.E_MISALIGNED and call(x=P * 2 + 8) == _lib.E_MISALIGNED
    assert call(nbytes=1024) == -2  # RSLRL_E_WORKSPACE_TOO_SMALL
    assert call(M=0) == 0 and call(M=0, N=1028) == _lib.E_UNSUPPORTED


PLAN_M = (16, 32, 64, 96, 128, 200, 1000, 1024, 1056, 2048, 3001, 4096, 8192, 16384, 32768, 393216)
PLAN_N = (4, 48, 64, 68, 256, 260, 512, 768, 1024)
PLAN_K = (4, 16, 48, 256, 260, 320, 512, 768, 1024)


def test_wgrad_plan_mirror_is_the_librarys():
    """tests/wide_plan.py against the library: the workspace of rslrl_linear_wgrad_bias_wide is S slices of partials
    plus the fold's, so a slice rule that moves away from the mirror's (a retune of wide_rows_per) fails here, on the
    host, and the full-tile GPU tests do not silently leave their variants.  Likewise the dense entry's."""
    L = _lib.lib()
    ws, fold = L.rslrl_linear_wgrad_bias_wide_workspace_bytes, L.rslrl_fold_partials_workspace_bytes
    shapes = {(M, N, K) for M in PLAN_M for N in PLAN_N for K in PLAN_K}
    shapes |= set(wide_plan.FULL_WGRAD) | {wide_plan.NEAR_FULL_WGRAD} | set(wide_plan.GENERAL_WGRAD)
    for M, N, K in sorted(shapes):
        plan = wide_plan.wgrad_plan(M, N, K)
        assert plan.S == -(-M // plan.rows_per) and plan.rows_per % 16 == 0 and plan.grid[0] == plan.S
        for side in (0, 1, 2):
            if not wide_plan.wgrad_side_ok(N, K, side):
                assert ws(M, N, K, side) == 0, (M, N, K, side)
                continue
            nke = wide_plan.wgrad_nke(N, K, side)
            assert ws(M, N, K, side) == plan.S * nke * 4 + fold(plan.S, nke), (M, N, K, side)
    dws = L.rslrl_linear_wgrad_bias_workspace_bytes
    for M, N, K in list(wide_plan.FULL_DENSE_WGRAD) + [(393216, 256, 256), (3001, 256, 256), (200, 48, 256)]:
        plan = wide_plan.dense_wgrad_plan(M, N, K)
        for side in (0, 1, 2):
            nke = wide_plan.wgrad_nke(N, K, side)
            assert dws(M, N, K, side) == plan.S * nke * 4 + fold(plan.S, nke), (M, N, K, side)


def test_full_tile_shapes_are_full_and_the_older_ones_are_not():
    """Why tests/test_gpu_wide_full_tiles.py exists: the look-ahead (FULL) weight-gradient variants run only at these
    shapes; every weight-gradient shape of tests/test_gpu_wide_mlp.py, direct or through the stacks at 1000 / 3001
    rows, takes the general loop."""
    for shape, (tn, S, chunks, maskn) in wide_plan.FULL_WGRAD.items():
        plan = wide_plan.wgrad_plan(*shape)
        assert plan.full and (plan.tn, plan.S, plan.chunks, plan.maskn) == (tn, S, chunks, maskn), (shape, plan)
        assert plan.chunks % wide_plan.DEPTH == 0 and plan.chunks >= 2
    assert [s for s in wide_plan.FULL_WGRAD if wide_plan.wgrad_plan(*s, depth=4).full] != []  # some survive depth 4
    assert wide_plan.wgrad_plan(64, 512, 512, depth=4).full and not wide_plan.wgrad_plan(96, 512, 512, depth=4).full
    near = wide_plan.wgrad_plan(*wide_plan.NEAR_FULL_WGRAD)
    assert not near.full and (near.S, near.chunks) == (14, 5)
    for shape in wide_plan.GENERAL_WGRAD:
        assert not wide_plan.wgrad_plan(*shape).full, shape
    # the stacks of test_wide_stack_forward_backward / _gradients_into_arena_slots at their row counts: as _weight_grad
    # calls the entry (the first layer swapped)
    for M, widths in ((3001, (48, 512, 256, 128)), (3001, (16, 320, 260, 64)), (3001, (48, 1024, 512, 256)),
                      (1000, (16, 320, 260, 64))):
        for k, n in zip(widths, widths[1:]):
            if max(k, n) > 256:
                assert not wide_plan.wgrad_plan(M, *((k, n) if k <= 64 < n else (n, k))).full, (M, n, k)
    # ... and at whole-tile row counts they are full, the first layer masked
    for M, widths in ((1024, (48, 512, 256, 128)), (4096, (48, 512, 256, 128)), (1024, (48, 1024, 512, 256)),
                      (4096, (48, 1024, 512, 256))):
        for k, n in zip(widths, widths[1:]):
            if max(k, n) > 256:
                plan = wide_plan.wgrad_plan(M, *((k, n) if k <= 64 < n else (n, k)))
                assert plan.full and plan.maskn == (k == 48), (M, n, k, plan)
    for shape, (tn, S, chunks, maskn) in wide_plan.FULL_DENSE_WGRAD.items():
        plan = wide_plan.dense_wgrad_plan(*shape)
        assert plan.full and (plan.tn, plan.S, plan.chunks, plan.maskn) == (tn, S, chunks, maskn), (shape, plan)
    assert not wide_plan.dense_wgrad_plan(3001, 256, 256).full


def test_gemm_plan_variants():
    """The wide GEMM shapes of tests/test_gpu_wide_full_tiles.py: full tiles at M = 256, none on the deep loop of
    K = 256, the last two on the MINW = 2 input gradient."""
    for K, N in wide_plan.FULL_GEMM_KN:
        for grad in (False, True):
            plan = wide_plan.gemm_plan(256, K, N, grad)
            assert plan.full and not plan.deep and plan.minw2 == (grad and K <= 32), (K, N, grad)
            assert plan.grid == (2, -(-N // 256))
    assert wide_plan.gemm_plan(256, 256, 512, True).deep and not wide_plan.gemm_plan(200, 48, 512, False).full
    assert [kn for kn in wide_plan.FULL_GEMM_KN if wide_plan.gemm_plan(256, *kn, True).minw2] == [(16, 512), (32, 260)]


def _relu_stack():
    return nn.Sequential(nn.Linear(48, 512), nn.ReLU(), nn.Linear(512, 128), nn.ReLU(), nn.Linear(128, 12))


WIDE = ((48, [512, 256, 128]), (48, [260, 64]), (48, [1024, 512, 256]), (1024, [512, 256]))
# the last three: more than MAX_WIDE inputs -- the first layer's K is a side of a wide layer, which the entry points refuse
NOT_WIDE = ((48, [512]), (48, [512, 512]), (48, [2048, 256]), (50, [512, 256, 128]),
            (1028, [512, 256, 128]), (1500, [256, 512, 256]), (2048, [512, 256]))


def test_wide_structure_truth_table():
    for k0, hidden in WIDE:
        m = MLP(k0, 12, hidden)
        assert fused_mlp.wide_structure(m) and m._wide and not m._fused, hidden
        assert not fused_mlp.fusable_structure(m), hidden
        for lin in (mod for mod in m if isinstance(mod, nn.Linear)):  # every layer it sends to the wide entry fits it
            if fused_mlp._wide_layer(lin.out_features, lin.in_features):
                assert _lib.lib().rslrl_linear_bimage_wide_bytes(lin.out_features, lin.in_features) > 0, (k0, hidden)
    for k0, hidden in NOT_WIDE:
        m = MLP(k0, 12, hidden)
        assert not fused_mlp.wide_structure(m) and not m._wide, (k0, hidden)
        assert not fused_mlp.fusable_structure(m), (k0, hidden)
    assert not fused_mlp.wide_structure(_relu_stack()) and not fused_mlp.fusable_structure(_relu_stack())
    assert not MLP(48, 12, [512, 256, 128], activation="relu")._wide
    # a width that is not 4-aligned, a narrow stack (fusable, not wide), a state-dependent-std head
    assert not fused_mlp.wide_structure(MLP(48, 12, [510, 256]))
    narrow = MLP(48, 12, [256, 256, 256])
    assert narrow._fused and not narrow._wide and not fused_mlp.wide_structure(narrow)
    assert MLP(48, [2, 12], [1024, 512, 256])._wide
    assert fused_mlp.MAX_WIDTH == 256 and fused_mlp.MAX_WIDE == 1024


def _policy(k0, actor, critic, **kw):
    groups = {"policy": ["policy"], "critic": ["policy"]}
    return ActorCritic({"policy": torch.zeros(4, k0)}, groups, 12, actor_hidden_dims=actor, critic_hidden_dims=critic, **kw)


def test_manual_update_structure_follows_the_table():
    for k0, hidden in WIDE:
        pol = _policy(k0, hidden, hidden)
        assert pol.manual_update_structure_ok() and pol.has_wide_mlp, hidden
        assert not pol.manual_update_ok({"policy": torch.zeros(4, k0)})  # CPU observations
    for k0, hidden in NOT_WIDE:
        assert not _policy(k0, hidden, hidden).manual_update_structure_ok(), (k0, hidden)
    assert not _policy(48, [512, 256, 128], [512, 256, 128], activation="relu").manual_update_structure_ok()
    mixed = _policy(48, [512, 256, 128], [256, 256, 256])  # narrow and wide: each network runs its own pass
    assert mixed.manual_update_structure_ok() and mixed.has_wide_mlp
    narrow = _policy(48, [256, 256, 256], [256, 256, 256])
    assert narrow.manual_update_structure_ok() and not narrow.has_wide_mlp
    assert not _policy(48, [512, 256, 128], [512, 512]).manual_update_structure_ok()
    # wide stacks run fused in x6 arithmetic only
    prev = fused_mlp.set_gemm_mode(fused_mlp.GEMM_F32)
    try:
        assert not fused_mlp.wide_enabled()
        assert not _policy(48, [512, 256, 128], [512, 256, 128]).manual_update_structure_ok()
        assert narrow.manual_update_structure_ok()
    finally:
        fused_mlp.set_gemm_mode(prev)


def test_wide_pairs_and_plans_decline():
    """The paired forms and the fused output layer keep their predicates: wide stacks decline them."""
    ws = [torch.zeros(512, 48), torch.zeros(256, 512), torch.zeros(128, 256), torch.zeros(12, 128)]
    x = torch.zeros(128, 48)
    assert not fused_mlp._pairable(ws, ws, x, x)
    assert fused_mlp._wide_ws(ws) and not fused_mlp._wide_ws([torch.zeros(256, 300), torch.zeros(12, 256)])
    assert fused_mlp._fuse_out_fwd(ws)  # the last hidden layer reads 256 inputs
    assert not fused_mlp._fuse_out_fwd([torch.zeros(320, 16), torch.zeros(260, 320), torch.zeros(64, 260), torch.zeros(4, 64)])
    assert fused_mlp._wgrad_form(512, 48, True, True) == "wide_first" and fused_mlp._wgrad_form(64, 260, True, True) == "wide"
    assert fused_mlp._bias_from_wgrad(512, 256, True, True) and not fused_mlp._bias_from_wgrad(64, 260, True, True)
    assert fused_mlp._wgrad_form(256, 256, True) == "square" and fused_mlp._wgrad_form(256, 48, True) == "first"
