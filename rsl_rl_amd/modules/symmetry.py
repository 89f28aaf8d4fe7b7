"""Symmetry config resolution (rsl_rl/modules/symmetry.py:9-24) and a declarative signed-permutation symmetry
whose augmentation runs as one HIP launch (kernels.symmetry_augment)."""

from __future__ import annotations

import torch

from .. import _lib, kernels
from ..utils.tensordict import TensorDict


def resolve_symmetry_config(alg_cfg, env):
    """Inject the environment into symmetry_cfg["_env"] for the augmentation function."""
    if alg_cfg.get("symmetry_cfg") is not None:
        alg_cfg["symmetry_cfg"]["_env"] = env
    return alg_cfg


class SignedPermutationSymmetry:
    """A data_augmentation_func (ppo.py:226-234, :323, :335) given as tables: augmentation k maps a row x of a field
    to  sign_k * x[perm_k]  (mirror left / right, front / back: swap and negate columns).

    obs_maps: {observation group: [(perm_0, sign_0), ..., (perm_{K-1}, sign_{K-1})]} over that group's columns;
    action_maps: the K pairs over the action columns.  Augmentation 0 must be the identity (the reference takes the
    first block of the result for the original batch), every perm a permutation, every sign +1 or -1; a ValueError
    names the offender.  Groups without a map are repeated unchanged.

    Called with the reference's contract f(obs=None, actions=None, env=None) -> (obs_aug, actions_aug): outputs are
    [K * B, ...] with block k holding augmentation k (obs_aug a TensorDict with batch_size [K * B]); a None input gives
    a None output.  CPU tensors take plain torch (index, multiply, cat); fp32 tensors on a ROCm device take one
    kernels.symmetry_augment launch for every group plus the actions (K <= 8, widths <= 1024, <= 8 fields; anything
    else takes the torch path there too).  PPO recognises an instance and hands its action tables to the loss kernel
    (kernels.ppo_loss_sym_fwd_bwd), which then forms the mirror target itself."""

    def __init__(self, obs_maps, action_maps):
        self.num_aug = len(action_maps)
        if self.num_aug < 1:
            raise ValueError("SignedPermutationSymmetry: action_maps needs at least the identity")
        self.action_perm, self.action_sign = self._tables("actions", action_maps)
        self.obs_tables = {}
        for group, maps in obs_maps.items():
            if len(maps) != self.num_aug:
                raise ValueError(f"SignedPermutationSymmetry: observation group {group!r} has {len(maps)} maps, the "
                                 f"actions have {self.num_aug}")
            self.obs_tables[group] = self._tables(f"observation group {group!r}", maps)
        self._device_tables = {}  # (device, field) -> (perm int32 [K, w], sign fp32 [K, w])

    @staticmethod
    def _tables(what, maps):
        perms, signs = [], []
        width = None
        for k, (perm, sign) in enumerate(maps):
            perm = torch.as_tensor(perm, dtype=torch.int64).reshape(-1).cpu()
            sign = torch.as_tensor(sign, dtype=torch.float32).reshape(-1).cpu()
            where = f"SignedPermutationSymmetry: {what}, augmentation {k}"
            width = perm.numel() if width is None else width
            if perm.numel() != width or sign.numel() != width or width < 1:
                raise ValueError(f"{where}: perm and sign must both have the field's {width} columns")
            if not torch.equal(torch.sort(perm).values, torch.arange(width)):
                raise ValueError(f"{where}: perm is not a permutation of 0..{width - 1}")
            if not bool(((sign == 1.0) | (sign == -1.0)).all()):
                raise ValueError(f"{where}: every sign must be +1 or -1")
            if k == 0 and not (torch.equal(perm, torch.arange(width)) and bool((sign == 1.0).all())):
                raise ValueError(f"{where}: augmentation 0 must be the identity")
            perms.append(perm)
            signs.append(sign)
        return torch.stack(perms), torch.stack(signs)

    # -------------------------------------------------------------------------------------------- tables
    def _on(self, device, field):
        key = (device, field)
        t = self._device_tables.get(key)
        if t is None:
            perm, sign = (self.action_perm, self.action_sign) if field is None else self.obs_tables[field]
            t = (perm.to(device=device, dtype=torch.int32).contiguous(), sign.to(device).contiguous())
            self._device_tables[key] = t
        return t

    def action_tables(self, device):
        """(perm int32 [K, A], sign fp32 [K, A]) on `device`, kept per instance."""
        return self._on(torch.device(device), None)

    # -------------------------------------------------------------------------------------------- call
    def __call__(self, obs=None, actions=None, env=None):
        fields = []  # (key or None for the actions, tensor, tables or None)
        if obs is not None:
            for key in obs.keys():
                fields.append((key, obs[key], key if key in self.obs_tables else None))
        if actions is not None:
            fields.append((None, actions, "actions"))
        for key, x, tab in fields:
            if tab is not None:
                w = (self.action_perm if key is None else self.obs_tables[key][0]).shape[1]
                if x.shape[-1] != w:
                    raise ValueError(f"SignedPermutationSymmetry: {'actions' if key is None else key!r} has "
                                     f"{x.shape[-1]} columns, its maps have {w}")
        outs = self._augment_hip(fields) if self._hip_ok(fields) else [self._augment_torch(*f) for f in fields]
        obs_aug = actions_aug = None
        if obs is not None:
            n = len(fields) - (1 if actions is not None else 0)
            B = obs.batch_size[0]
            obs_aug = TensorDict({f[0]: o for f, o in zip(fields[:n], outs[:n])}, batch_size=[self.num_aug * B],
                                 device=getattr(obs, "device", None))
        if actions is not None:
            actions_aug = outs[-1]
        return obs_aug, actions_aug

    def _augment_torch(self, key, x, tab):
        """The plain torch form (and the kernel's oracle): index, multiply, cat."""
        K = self.num_aug
        if tab is None:
            return x.repeat(K, *([1] * (x.dim() - 1)))
        perm, sign = (self.action_perm, self.action_sign) if key is None else self.obs_tables[key]
        perm, sign = perm.to(x.device), sign.to(device=x.device, dtype=x.dtype)
        return torch.cat([x.index_select(-1, perm[k]) * sign[k] for k in range(K)], dim=0)

    def _hip_ok(self, fields) -> bool:
        if not fields or self.num_aug > _lib.SYMMETRY_MAX_AUG or len(fields) > _lib.SYMMETRY_MAX_FIELDS:
            return False
        B = fields[0][1].shape[0]
        for _, x, _ in fields:
            if not (x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and x.shape[0] == B and B >= 1
                    and 1 <= x.shape[1] <= _lib.SYMMETRY_MAX_WIDTH and (x.shape[1] == 1 or x.stride(1) == 1)
                    and (B == 1 or x.stride(0) >= x.shape[1]) and not x.requires_grad):
                return False
        return True

    def _augment_hip(self, fields):
        K = self.num_aug
        B = fields[0][1].shape[0]
        launch, outs = [], []
        for key, x, tab in fields:
            dst = torch.empty(K * B, x.shape[1], dtype=torch.float32, device=x.device)
            perm, sign = self._on(x.device, key) if tab is not None else (None, None)
            launch.append((x, dst, perm, sign))
            outs.append(dst)
        kernels.symmetry_augment(launch, B, K)
        return outs
