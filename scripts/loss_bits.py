"""SHA-256 of every output of the four PPO-loss entry points, per library build: a refactor's "same bits" check.

    python scripts/loss_bits.py PARENT.so BRANCH.so [--out profiles/loss_common_bits.json]

Each library runs in a fresh child process (selected by RSLRL_AMD_LIB) on the same inputs, drawn once per case from a
seeded numpy generator: rslrl_ppo_loss_fwd_bwd, rslrl_ppo_loss_sym_fwd_bwd, rslrl_actor_head_fwd_bwd and
rslrl_value_head_fwd_bwd at small shapes that reach every branch of their kernels, each with the clipped value loss on
and off, the KL on and off, RSLRL_KL_FAST 1 and 0 and the advantage normalisation on and off where the entry point
has them.  Exit status 1 if a hash differs between the two libraries."""

import argparse
import hashlib
import itertools
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

LOSS = [  # B, A, shared sigma, RSLRL_LOSS_KERNEL
    (300, 12, True, "quad"), (300, 12, True, "lane"), (64, 4, False, "quad"), (64, 4, False, "lane"),
    (111, 3, True, None)]  # A = 3: scalar loads
SYM = [(111, 2, 2, 12, True), (64, 2, 2, 4, False)]  # B, k_ppo, k_mir, A, shared sigma
HEAD_M = [128, 384]  # one and three 128-row tiles


def sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def child():
    import numpy as np
    import torch

    sys.path.insert(0, ROOT)
    from rsl_rl_amd import _lib, kernels
    from rsl_rl_amd.networks import fused_mlp

    dev = torch.device("cuda:0")
    out = {}

    def dv(a):
        return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)

    def loss_inputs(rng, rows, n, B, A, shared):
        return dict(mu=dv(rng.standard_normal((rows, A))),
                    sigma=dv(rng.uniform(0.5, 1.5, A if shared else (rows, A))),
                    V=dv(0.3 * rng.standard_normal((n, 1))), x=dv(rng.standard_normal((n, A))),
                    old_logp=dv(rng.standard_normal((B, 1)) - 1.4 * A), adv=dv(rng.standard_normal((B, 1))),
                    tv=dv(0.3 * rng.standard_normal((B, 1))), R=dv(rng.standard_normal((B, 1))),
                    omu=dv(rng.standard_normal((B, A))))

    def old_sigma(rng, B, A, shared):
        # shared: sample 0's sigma for every row but every third (the fast KL's per-element fall-back)
        if not shared:
            return dv(rng.uniform(0.5, 1.5, (B, A)))
        os_ = np.tile(rng.uniform(0.5, 1.5, (1, A)), (B, 1))
        os_[1::3] *= 1.0 + 0.05 * rng.random(os_[1::3].shape)
        return dv(os_)

    flags = list(itertools.product((True, False), (True, False), ("1", "0"), (False, True)))
    for B, A, shared, kern in LOSS:
        rng = np.random.default_rng(1000 * B + A)
        d = loss_inputs(rng, B, B, B, A, shared)
        d["osig"] = old_sigma(rng, B, A, shared)
        for clipped, kl, fast, norm in flags:
            os.environ["RSLRL_KL_FAST"] = fast
            if kern:
                os.environ["RSLRL_LOSS_KERNEL"] = kern
            else:
                os.environ.pop("RSLRL_LOSS_KERNEL", None)
            res = kernels.ppo_loss_fwd_bwd(d["mu"], d["sigma"], d["V"], d["x"], d["old_logp"], d["adv"], d["tv"],
                                           d["R"], d["omu"], d["osig"], clip_param=0.2, value_loss_coef=1.0,
                                           entropy_coef=0.01, use_clipped_value_loss=clipped, compute_kl=kl,
                                           normalize_advantage=norm)
            torch.cuda.synchronize()
            key = f"loss B={B} A={A} shared={shared} kernel={kern} clipped={clipped} kl={kl} fast={fast} norm={norm}"
            out[key] = dict(zip(("stats", "grad_mu", "grad_sigma", "grad_values"), map(sha, res)))
    os.environ.pop("RSLRL_LOSS_KERNEL", None)
    for B, k_ppo, k_mir, A, shared in SYM:
        rng = np.random.default_rng(7000 * B + A)
        d = loss_inputs(rng, k_mir * B, k_ppo * B, B, A, shared)
        d["osig"] = old_sigma(rng, B, A, False)
        perm = torch.from_numpy(np.stack([rng.permutation(A) for _ in range(k_mir)])).to(torch.int32).to(dev)
        sign = dv(rng.choice([-1.0, 1.0], (k_mir, A)))
        for clipped, kl, fast, norm in flags:
            os.environ["RSLRL_KL_FAST"] = fast
            res = kernels.ppo_loss_sym_fwd_bwd(d["mu"], d["sigma"], d["V"], d["x"], d["old_logp"], d["adv"], d["tv"],
                                               d["R"], d["omu"], d["osig"], B=B, k_ppo=k_ppo, k_mir=k_mir,
                                               mirror_coeff=0.5, act_perm=perm, act_sign=sign, clip_param=0.2,
                                               value_loss_coef=1.0, entropy_coef=0.01, use_clipped_value_loss=clipped,
                                               compute_kl=kl, normalize_advantage=norm)
            torch.cuda.synchronize()
            key = f"sym B={B} k={k_ppo},{k_mir} A={A} shared={shared} clipped={clipped} kl={kl} fast={fast} norm={norm}"
            out[key] = dict(zip(("stats", "grad_mu", "grad_sigma", "grad_values"), map(sha, res)))
    A, K, N = 12, 256, 256
    for M in HEAD_M:
        rng = np.random.default_rng(31 * M)
        x, w, b = dv(np.maximum(rng.standard_normal((M, K)), -0.9)), dv(rng.standard_normal((N, K)) / 16), \
            dv(0.1 * rng.standard_normal(N))
        wo, bo = dv(rng.standard_normal((A, N)) / 16), dv(0.1 * rng.standard_normal(A))
        wv, bv = dv(rng.standard_normal((1, N)) / 16), dv(0.1 * rng.standard_normal(1))
        d = loss_inputs(rng, M, M, M, A, True)
        d["osig"] = old_sigma(rng, M, A, True)
        img, out_img, img_t, vout_img = fused_mlp.bimages([(w, False), (wo, False, _lib.BIMAGE_LAYOUT_OUT), (wo, True),
                                                           (wv, False, _lib.BIMAGE_LAYOUT_OUT)])
        for clipped, kl, fast, _ in flags[::2]:  # (the heads have no advantage normalisation)
            os.environ["RSLRL_KL_FAST"] = fast
            head = fused_mlp.ActorHead(d["x"], d["old_logp"], d["adv"], d["tv"], d["R"], d["omu"], d["osig"],
                                       d["sigma"], clip_param=0.2, value_loss_coef=1.0, entropy_coef=0.01,
                                       use_clipped=clipped, compute_kl=kl, grad_sigma=torch.empty(A, device=dev),
                                       stats=torch.empty(8, device=dev), grad_mu=torch.empty(M, A, device=dev))
            head.values = d["V"]
            dz, mu, wpart = fused_mlp.actor_head_fwd_bwd(x, b, N, img, bo, out_img, img_t, head)
            torch.cuda.synchronize()
            out[f"actor_head M={M} clipped={clipped} kl={kl} fast={fast}"] = {
                "dz": sha(dz), "mu": sha(mu), "wpart": sha(wpart), "stats": sha(head.stats),
                "grad_sigma": sha(head.grad_sigma), "grad_mu": sha(head.grad_mu)}
        for clipped in (True, False):
            vh = fused_mlp.ValueHead(d["tv"], d["R"], 0.2, 1.0, clipped)
            dz, y, wpart = fused_mlp.value_head_fwd_bwd(x, b, N, img, bv, vout_img, wv, vh)
            torch.cuda.synchronize()
            out[f"value_head M={M} clipped={clipped}"] = {"dz": sha(dz), "y": sha(y), "wpart": sha(wpart)}
    print("LOSS_BITS " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("libs", nargs="*", help="two library builds to compare: parent, then this tree")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.child:
        return child()
    if len(a.libs) != 2:
        ap.error("two libraries")
    tables = []
    for lib in a.libs:
        env = dict(os.environ, RSLRL_AMD_LIB=os.path.abspath(lib))
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=env, capture_output=True,
                           text=True, timeout=300)
        line = [ln for ln in r.stdout.split("\n") if ln.startswith("LOSS_BITS ")]
        if r.returncode != 0 or not line:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            return 2  # (nothing more is started after a failed child)
        tables.append(json.loads(line[0][len("LOSS_BITS "):]))
    parent, branch = tables
    differ = sorted(f"{case}: {name}" for case in parent for name in parent[case]
                    if branch.get(case, {}).get(name) != parent[case][name])
    res = {"cases": len(parent), "tensors": sum(len(v) for v in parent.values()), "differ": differ,
           "identical": not differ and parent.keys() == branch.keys(), "parent": parent, "branch": branch}
    print(json.dumps({k: res[k] for k in ("cases", "tensors", "differ", "identical")}))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    return 0 if res["identical"] else 1


if __name__ == "__main__":
    sys.exit(main())
