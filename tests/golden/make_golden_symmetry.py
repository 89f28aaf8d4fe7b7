"""Generate the symmetry fixtures under tests/golden/ by running the REFERENCE's PPO.update() on CPU with a
symmetry_cfg (ppo.py:213-257 data augmentation, :317-348 mirror loss).

Test infrastructure only, like make_golden.py (whose import shims and storage helpers it reuses without editing
that file): it runs where a reference checkout exists and writes tests/golden/update_sym_<case>.npz plus
tests/golden/golden_symmetry.json.  The files follow the update_* family's layout (initial and final parameters,
the policy-dependent storage, generator state, lr_trace, loss_dict including "symmetry", grad_mb0, and the one-ulp
ulp_sensitivity envelope); the signed-permutation tables are stored in the JSON, so that the tests rebuild the same
symmetry.  The symmetry_cfg function is this script's own torch code.

Every case: T 8, N 256, O 16, A 4, hidden [64, 64], E 5, M 4 (B = 512).  The generator asserts that in every
mini-batch the reference's KL stays at least 1e-3 (relative) away from both adaptive-lr thresholds, so that an exact
lr_trace comparison is meaningful; a case whose seed does not satisfy this is given another seed here.

Usage:  python tests/golden/make_golden_symmetry.py --reference PATH_TO_RSL_RL_CHECKOUT [--cases a,b]
"""

from __future__ import annotations

import argparse
import hashlib
import json
import os

import numpy as np
import torch

import make_golden as G

HERE = os.path.dirname(os.path.abspath(__file__))
T, N, O, A, HIDDEN, E, M = 8, 256, 16, 4, [64, 64], 5, 4
DESIRED_KL = 0.01
KL_MARGIN = 1e-3

RND_STATENORM = dict(weight=0.5, num_outputs=3, predictor_hidden_dims=[32], target_hidden_dims=[32],
                     state_normalization=True, learning_rate=2e-3)  # make_golden's rnd_statenorm_w1

# name, K, use_data_augmentation, use_mirror_loss, mirror_loss_coeff, seed, rnd_cfg
CASES = [
    ("a", 2, True, True, 0.5, 211, None),
    ("b", 4, True, False, 0.0, 223, None),
    ("c", 2, False, True, 1.0, 227, None),
    ("d", 2, False, False, 0.0, 229, None),
    ("e", 2, True, True, 0.5, 233, RND_STATENORM),
]


class _AugDict(G._RowDict):
    """The augmented observations: the reference also detaches and clones them (ppo.py:328)."""

    def detach(self):
        return _AugDict({k: v.detach() for k, v in self._d.items()}, self.batch_size, self.device)

    def clone(self):
        return _AugDict({k: v.clone() for k, v in self._d.items()}, self.batch_size, self.device)


def signed_permutations(seed, width, K):
    """K (perm, sign) pairs over `width` columns: the identity, then signed permutations without fixed points in
    the permutation (numpy PCG64, so the tables are the same wherever this runs)."""
    rng = np.random.default_rng(seed)
    perms, signs = [np.arange(width)], [np.ones(width, np.float32)]
    while len(perms) < K:
        p = rng.permutation(width)
        s = rng.choice(np.array([-1.0, 1.0], np.float32), width)
        if (p == np.arange(width)).any() or (s == 1.0).all() or any((p == q).all() for q in perms):
            continue
        perms.append(p)
        signs.append(s)
    return np.stack(perms), np.stack(signs)


def make_augmentation(tables):
    obs_perm = torch.from_numpy(tables["obs_perm"]).long()
    obs_sign = torch.from_numpy(tables["obs_sign"])
    act_perm = torch.from_numpy(tables["act_perm"]).long()
    act_sign = torch.from_numpy(tables["act_sign"])

    def apply(x, perm, sign):
        return torch.cat([x[:, perm[k]] * sign[k] for k in range(perm.shape[0])], dim=0)

    def augment(obs=None, actions=None, env=None):
        obs_aug = actions_aug = None
        if obs is not None:
            out = {k: apply(obs[k], obs_perm, obs_sign) for k in obs.keys()}
            obs_aug = _AugDict(out, batch_size=[obs_perm.shape[0] * obs.batch_size[0]])
        if actions is not None:
            actions_aug = apply(actions, act_perm, act_sign)
        return obs_aug, actions_aug

    return augment


def run_update(PPO, ActorCritic, *, seed, symmetry_cfg, rnd_cfg, probe=None):
    """One reference update() (make_golden._update_case's steps, with a symmetry_cfg): (arrays, meta, KL trace)."""
    torch.manual_seed(seed)
    obs0 = {"policy": torch.zeros(N, O)}
    groups = {"policy": ["policy"], "critic": ["policy"]}
    if rnd_cfg is not None:
        groups["rnd_state"] = ["policy"]
    pol = ActorCritic(obs0, groups, A, actor_hidden_dims=HIDDEN, critic_hidden_dims=HIDDEN)
    rcfg = None if rnd_cfg is None else dict(rnd_cfg, num_states=O, obs_groups=groups)
    scfg = None if symmetry_cfg is None else dict(symmetry_cfg, _env=None)
    alg = PPO(pol, num_learning_epochs=E, num_mini_batches=M, device="cpu", learning_rate=1e-3, rnd_cfg=rcfg,
              symmetry_cfg=scfg, desired_kl=DESIRED_KL)
    init_state = {k: G.f32(v) for k, v in pol.state_dict().items()}
    if probe is not None and probe.startswith("par"):  # every initial policy parameter one ulp up or down
        g = torch.Generator().manual_seed(int(probe[3:]) * 1000 + 7)
        with torch.no_grad():
            for p in pol.parameters():
                up = torch.nextafter(p, torch.full_like(p, float("inf")))
                down = torch.nextafter(p, torch.full_like(p, float("-inf")))
                p.copy_(torch.where(torch.rand(p.shape, generator=g) < 0.5, up, down))
    rnd_init = {}
    if alg.rnd is not None:
        if alg.rnd.state_normalization:
            nrng = np.random.default_rng(seed * 100 + 50)
            for _ in range(2):
                x = nrng.standard_normal((N, O), dtype=np.float32) * 1.5 + 0.25
                alg.rnd.update_normalization({"policy": torch.from_numpy(x)})
        rnd_init = {k: (v.numpy().copy() if v.dtype == torch.int64 else G.f32(v))
                    for k, v in alg.rnd.state_dict().items()}
    alg.init_storage("rl", N, T, obs0, [A])
    nz = G.storage_noise(seed * 100, T, N, O, A)
    stored = G._fill_storage_from_noise(alg.storage, pol, nz, False)
    if probe is not None and not probe.startswith("par"):  # the stored log-probs one ulp off
        lp = alg.storage.actions_log_prob
        up = torch.nextafter(lp, torch.full_like(lp, float("inf")))
        down = torch.nextafter(lp, torch.full_like(lp, float("-inf")))
        if probe == "up":
            lp.copy_(up)
        elif probe == "down":
            lp.copy_(down)
        else:
            g = torch.Generator().manual_seed(int(probe[4:]) * 1000)
            lp.copy_(torch.where(torch.rand(lp.shape, generator=g) < 0.5, up, down))
    with torch.inference_mode():
        alg.compute_returns({"policy": torch.from_numpy(nz["last_obs"])})
    torch.manual_seed(5000)
    gen_state = torch.default_generator.get_state().numpy().copy()

    # the reference's kl_mean = torch.mean(kl) is its only torch.mean under inference mode (ppo.py:261-269)
    kls = []
    orig_mean = torch.mean

    def rec_mean(x, *a, **kw):
        r = orig_mean(x, *a, **kw)
        if torch.is_inference_mode_enabled() and r.dim() == 0:
            kls.append(float(r))
        return r

    torch.mean = rec_mean
    try:
        loss_dict, lr_trace, grads, rnd_grads = G._run_recorded_update(alg, 1)
    finally:
        torch.mean = orig_mean
    assert len(kls) == E * M, len(kls)
    arrays = {f"init/{k}": v for k, v in init_state.items()}
    arrays["grad_mb0"] = G.f32(grads[0])
    if rnd_grads:
        arrays["rnd_grad_mb0"] = G.f32(rnd_grads[0])
    arrays.update({f"final/{k}": G.f32(v) for k, v in pol.state_dict().items()})
    if alg.rnd is not None:
        arrays.update({f"rnd_init/{k}": v for k, v in rnd_init.items()})
        arrays.update({f"rnd_final/{k}": G.f32(v) for k, v in alg.rnd.predictor.state_dict().items()})
    arrays.update({f"storage/{k}": v for k, v in stored.items()})
    arrays["storage/returns_head"] = G.f32(alg.storage.returns[:2])
    arrays["gen_state"] = gen_state
    arrays["obs_sha256"] = np.frombuffer(hashlib.sha256(nz["obs"].tobytes()).digest(), dtype=np.uint8)
    meta = {"loss_dict": loss_dict, "lr_trace": lr_trace, "final_lr": alg.learning_rate, "noise_seed": seed * 100}
    return {f"r0/{k}": v for k, v in arrays.items()}, meta, kls


def kl_margin(kls):
    """Smallest relative distance of a mini-batch KL from the adaptive-lr thresholds 2 kl* and kl* / 2."""
    return min(min(abs(k - 2.0 * DESIRED_KL) / (2.0 * DESIRED_KL), abs(k - DESIRED_KL / 2.0) / (DESIRED_KL / 2.0))
               for k in kls)


def make_case(PPO, ActorCritic, name, K, augment, mirror, coeff, seed, rnd_cfg):
    for attempt in range(20):  # another seed until the reference alone keeps its KL off the thresholds
        s = seed + 1000 * attempt
        obs_perm, obs_sign = signed_permutations(s * 10 + 1, O, K)
        act_perm, act_sign = signed_permutations(s * 10 + 2, A, K)
        tables = {"obs_perm": obs_perm, "obs_sign": obs_sign, "act_perm": act_perm, "act_sign": act_sign}
        cfg = {"use_data_augmentation": augment, "use_mirror_loss": mirror, "mirror_loss_coeff": coeff,
               "data_augmentation_func": make_augmentation(tables)}
        arrays, rank, kls = run_update(PPO, ActorCritic, seed=s, symmetry_cfg=cfg, rnd_cfg=rnd_cfg)
        margin = kl_margin(kls)
        if margin >= KL_MARGIN:
            break
        print(f"case {name}: seed {s} has a KL within {margin:.1e} of a threshold, trying another", flush=True)
    assert margin >= KL_MARGIN, (name, margin)
    if not augment and not mirror:
        # logged only: the parameters are those of the same update without symmetry_cfg, bit for bit
        plain, _, _ = run_update(PPO, ActorCritic, seed=s, symmetry_cfg=None, rnd_cfg=rnd_cfg)
        for k in [k for k in arrays if k.startswith("r0/final/")]:
            assert np.array_equal(arrays[k], plain[k]), k
    sens = {}
    probes = ("up", "down", "rand0", "par0", "par1")
    for probe in probes:
        cfg_p = dict(cfg, data_augmentation_func=make_augmentation(tables))
        ulp, _, _ = run_update(PPO, ActorCritic, seed=s, symmetry_cfg=cfg_p, rnd_cfg=rnd_cfg, probe=probe)
        for pre, init_pre in (("r0/final/", "r0/init/"), ("r0/rnd_final/", None)):
            for k in [k for k in arrays if k.startswith(pre)]:
                pname = k[len(pre):]
                init = arrays[init_pre + pname] if init_pre else arrays["r0/rnd_init/predictor." + pname]
                moved = np.linalg.norm(arrays[k].astype(np.float64) - init.astype(np.float64))
                d = np.linalg.norm(ulp[k].astype(np.float64) - arrays[k].astype(np.float64))
                key = ("rnd/" if init_pre is None else "") + pname
                sens[key] = max(sens.get(key, 0.0), float(d / moved) if moved else float(d))
    np.savez_compressed(os.path.join(HERE, f"update_sym_{name}.npz"), **arrays)
    meta = {"world": 1, "T": T, "N": N, "O": O, "A": A, "hidden": HIDDEN, "M": M, "E": E, "seed": s,
            "learning_rate": 1e-3, "ranks": [rank], "mu_fp16": False, "shared_params": False, "rnd_cfg": rnd_cfg,
            "policy_kw": {}, "ulp_sensitivity": sens, "ulp_probes": list(probes), "kl_trace": kls,
            "kl_margin": margin,
            "symmetry": {"K": K, "use_data_augmentation": augment, "use_mirror_loss": mirror,
                         "mirror_loss_coeff": coeff, "obs_perm": obs_perm.tolist(), "obs_sign": obs_sign.tolist(),
                         "act_perm": act_perm.tolist(), "act_sign": act_sign.tolist()}}
    print(f"case {name}: seed {s} K {K} KL margin {margin:.2e} losses {rank['loss_dict']} final lr "
          f"{rank['final_lr']}", flush=True)
    return meta


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="the rsl_rl 3.1.0 checkout (the directory holding rsl_rl/)")
    ap.add_argument("--cases", default=None, help="comma-separated case names (default: all)")
    args = ap.parse_args()
    torch.set_num_threads(1)
    PPO, ActorCritic, _ = G.import_reference(args.reference)
    path = os.path.join(HERE, "golden_symmetry.json")
    meta = {}
    if args.cases and os.path.exists(path):
        with open(path) as f:
            meta = json.load(f)
    for case in CASES:
        if args.cases is None or case[0] in args.cases.split(","):
            meta[case[0]] = make_case(PPO, ActorCritic, *case)
    with open(path, "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
