"""SignedPermutationSymmetry's contract on CPU (the torch path, which is also the augment kernel's oracle) and the
argument validation of the two symmetry entry points of the C ABI (no launch: this runs without a GPU)."""

import ctypes

import pytest
import torch

from rsl_rl_amd import _lib
from rsl_rl_amd.modules import SignedPermutationSymmetry
from rsl_rl_amd.utils.tensordict import TensorDict


def mirror(width, swaps, flips):
    """(perm, sign) of one mirror: columns swapped pairwise, `flips` negated."""
    perm = list(range(width))
    for a, b in swaps:
        perm[a], perm[b] = b, a
    sign = [-1.0 if c in flips else 1.0 for c in range(width)]
    return perm, sign


def identity(width):
    return list(range(width)), [1.0] * width


def make_symmetry():
    obs = [identity(6), mirror(6, [(0, 1), (2, 5)], {3, 4})]
    act = [identity(4), mirror(4, [(0, 3)], {1})]
    return SignedPermutationSymmetry({"policy": obs}, act)


def test_shapes_first_block_and_values():
    sym = make_symmetry()
    g = torch.Generator().manual_seed(0)
    B = 5
    obs = TensorDict({"policy": torch.randn(B, 6, generator=g), "extra": torch.randn(B, 3, generator=g)},
                     batch_size=[B])
    act = torch.randn(B, 4, generator=g)
    o, a = sym(obs=obs, actions=act, env=None)
    assert isinstance(o, TensorDict) and list(o.batch_size) == [2 * B]
    assert o["policy"].shape == (2 * B, 6) and o["extra"].shape == (2 * B, 3) and a.shape == (2 * B, 4)
    assert torch.equal(o["policy"][:B], obs["policy"]) and torch.equal(a[:B], act)
    # a group without a map is repeated unchanged
    assert torch.equal(o["extra"][:B], obs["extra"]) and torch.equal(o["extra"][B:], obs["extra"])
    perm, sign = mirror(6, [(0, 1), (2, 5)], {3, 4})
    assert torch.equal(o["policy"][B:], obs["policy"][:, perm] * torch.tensor(sign))
    perm, sign = mirror(4, [(0, 3)], {1})
    assert torch.equal(a[B:], act[:, perm] * torch.tensor(sign))


def test_none_handling():
    sym = make_symmetry()
    obs = TensorDict({"policy": torch.randn(3, 6)}, batch_size=[3])
    o, a = sym(obs=obs, actions=None, env=None)
    assert a is None and o["policy"].shape == (6, 6)
    o, a = sym(obs=None, actions=torch.randn(3, 4), env=None)
    assert o is None and a.shape == (6, 4)
    assert sym() == (None, None)


def test_mirror_twice_is_identity():
    sym = make_symmetry()
    x = torch.randn(7, 4)
    _, once = sym(actions=x)
    _, twice = sym(actions=once[7:])
    assert torch.equal(twice[7:], x)
    obs = TensorDict({"policy": torch.randn(7, 6)}, batch_size=[7])
    o1, _ = sym(obs=obs)
    o2, _ = sym(obs=TensorDict({"policy": o1["policy"][7:]}, batch_size=[7]))
    assert torch.equal(o2["policy"][7:], obs["policy"])


def test_action_tables_are_kept_per_device():
    sym = make_symmetry()
    perm, sign = sym.action_tables("cpu")
    assert perm.dtype == torch.int32 and sign.dtype == torch.float32 and perm.shape == sign.shape == (2, 4)
    assert sym.action_tables("cpu")[0] is perm


@pytest.mark.parametrize("obs_maps, act_maps, match", [
    ({}, [mirror(4, [(0, 3)], {1})], "actions, augmentation 0: augmentation 0 must be the identity"),
    ({}, [([0, 1, 2, 3], [1.0, 1.0, -1.0, 1.0])], "augmentation 0 must be the identity"),
    ({}, [identity(4), ([0, 1, 1, 3], [1.0] * 4)], "actions, augmentation 1: perm is not a permutation"),
    ({}, [identity(4), ([0, 1, 2, 4], [1.0] * 4)], "perm is not a permutation"),
    ({}, [identity(4), ([0, 1, 2, 3], [1.0, 0.5, 1.0, 1.0])], "actions, augmentation 1: every sign must be"),
    ({}, [identity(4), ([0, 1, 2], [1.0] * 3)], "must both have the field's 4 columns"),
    ({"policy": [identity(6)]}, [identity(4), identity(4)], "observation group 'policy' has 1 maps"),
    ({"policy": [identity(6), ([0, 0, 2, 3, 4, 5], [1.0] * 6)]}, [identity(4), identity(4)],
     "observation group 'policy', augmentation 1: perm is not a permutation"),
    ({"policy": [identity(6), (list(range(6)), [1.0, 1.0, 1.0, 1.0, 1.0, 2.0])]}, [identity(4), identity(4)],
     "observation group 'policy', augmentation 1: every sign"),
    ({}, [], "at least the identity"),
])
def test_validation_errors(obs_maps, act_maps, match):
    with pytest.raises(ValueError, match=match):
        SignedPermutationSymmetry(obs_maps, act_maps)


def test_width_mismatch_at_call():
    sym = make_symmetry()
    with pytest.raises(ValueError, match="columns"):
        sym(actions=torch.zeros(2, 5))


# ---------------------------------------------------------------------------------------------------- C ABI
def test_symbols_and_version():
    L = _lib.lib()
    for name in ("rslrl_ppo_loss_sym_fwd_bwd", "rslrl_ppo_loss_sym_workspace_bytes", "rslrl_symmetry_augment"):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(L, name), name
    assert L.rslrl_abi_version() == _lib.ABI_VERSION >= 22  # the symmetry entry points came with ABI 22


def _loss_args(B=10, A=4, k_ppo=2, k_mir=2):
    s = _lib.PPOLossSymArgs()
    a = s.loss
    a.B, a.A, a.sigma_mode = B, A, 0
    for f in ("mu", "sigma", "values", "actions", "old_logp", "advantages", "target_values", "returns", "old_mu",
              "old_sigma", "grad_mu", "grad_sigma", "grad_values", "stats"):
        setattr(a, f, 256)  # non-null; never dereferenced: every call below is refused before a launch
    a.mu_stride = a.grad_mu_stride = A
    s.k_ppo, s.k_mir = k_ppo, k_mir
    s.act_perm = s.act_sign = 256
    return s


def test_loss_argument_validation_without_gpu():
    L = _lib.lib()
    call = lambda s, ws=256, n=1 << 20: L.rslrl_ppo_loss_sym_fwd_bwd(ctypes.byref(s), ws, n, None)  # noqa: E731
    assert L.rslrl_ppo_loss_sym_fwd_bwd(None, 256, 1 << 20, None) == -1
    assert call(_loss_args(k_ppo=9, k_mir=9)) == -1  # K > 8
    assert call(_loss_args(A=65)) == -1  # A > 64
    assert call(_loss_args(B=0)) == -1
    assert call(_loss_args(k_ppo=2, k_mir=4)) == -1  # the PPO terms cover one block or all of them
    assert call(_loss_args(k_ppo=0, k_mir=2)) == -1
    for f in ("mu", "values", "actions", "old_mu", "grad_mu", "grad_values", "stats"):
        s = _loss_args()
        setattr(s.loss, f, None)
        assert call(s) == -1, f  # a required pointer is null
    s = _loss_args()
    s.mirror_target = 256  # both target forms
    assert call(s) == -1
    s = _loss_args()
    s.act_perm = s.act_sign = None  # neither
    assert call(s) == -1
    s = _loss_args()
    s.act_sign = None  # half a table
    assert call(s) == -1
    s = _loss_args(k_ppo=1, k_mir=1)  # no mirror term: no target may be given
    assert call(s) == -1
    s = _loss_args()
    s.loss.mu_stride = 3
    assert call(s) == -1
    assert call(_loss_args(), ws=None) == -1
    assert call(_loss_args(), n=16) == -2  # workspace too small
    assert call(_loss_args(), ws=264) == -4  # misaligned workspace
    assert L.rslrl_ppo_loss_sym_workspace_bytes(98304, 12, 2) >= 1024 + 8 * 17 * 512


def test_augment_argument_validation_without_gpu():
    L = _lib.lib()
    F = _lib.SymmetryField
    one = lambda **kw: (F * 1)(F(**{**dict(src=256, src_stride=8, dst=512, width=8, perm=1024, sign=2048), **kw}))  # noqa: E731
    call = lambda arr, n=1, B=4, K=2: L.rslrl_symmetry_augment(arr, n, B, K, None)  # noqa: E731
    assert call(one(), K=9) == -1
    assert call(one(), K=0) == -1
    assert call(one(), n=9) == -1
    assert call(None) == -1
    assert call(one(), B=-1) == -1
    assert call(one(width=1025, src_stride=1025)) == -1
    assert call(one(width=0)) == -1
    assert call(one(src_stride=4)) == -1  # rows would overlap
    assert call(one(src=None)) == -1
    assert call(one(dst=None)) == -1
    assert call(one(sign=None)) == -1  # perm without sign
    assert call(one(), B=0) == 0  # nothing to do: no launch
    assert call(one(), n=0) == 0
