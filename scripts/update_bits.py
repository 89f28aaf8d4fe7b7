"""SHA-256 of what PPO.update() and Distillation.update() leave behind on every committed golden update case: a
refactor's "same bits" check for the Python side of the update, as scripts/loss_bits.py is for the loss kernels.

    python scripts/update_bits.py --root TREE --table out/bits_TREE.json            # one table per run (needs the GPU)
    python scripts/update_bits.py --compare PARENT_1.json PARENT_2.json THIS.json --out profiles/update_split_bits.json

--root is the checkout whose rsl_rl_amd package and tests/ fixture modules are used (default: this one), so that the
same script measures a parent checkout and this tree.  Each case is built through the fixture modules under tests/
(update_fixtures, recurrent_fixtures, distill_fixtures, drec_fixtures and the builders of test_gpu_update_c3 /
test_gpu_symmetry_update), runs one update() and yields a hash per parameter and buffer, per optimizer-state tensor,
per returned loss value and of the final learning rate.  Cases: update_c1 (over a world-1 group), c2 (width), c3, the
RND and std-variant cases (the latter also on the autograd path), sym_a..e (a also as an opaque callable and on the
autograd path), rec_a..c, distill_a..c and drec_a..c (a / c also on the per-step path), and the multi-rank cases (w2,
w4, w8, w2_c4net, rnd_c5_w2, distill_w2: spawned ranks on one device over gloo, a table entry per rank).

--compare: every hash on which the two parent tables agree must equal this tree's; a case on which the parent differs
from itself is listed under "parent_unstable" instead.  Exit status 1 on a difference."""

import argparse
import hashlib
import json
import os
import socket
import struct
import sys
import tempfile

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MULTI = [("w2", "multirank"), ("w4", "multirank"), ("w8", "multirank"), ("w2_c4net", "multirank"),
         ("rnd_c5_w2", "update_rnd"), ("distill_w2", None)]


def use_tree(root):
    for p in (os.path.join(root, "tests"), root):
        if p not in sys.path:
            sys.path.insert(0, p)


def sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def sha_float(v):
    return hashlib.sha256(struct.pack("<d", float(v))).hexdigest()


def digest(alg, loss):
    """The table entry of one finished update()."""
    import torch

    out = {"lr": sha_float(alg.learning_rate)}
    out.update({f"loss/{k}": sha_float(v) for k, v in loss.items()})
    for i, v in enumerate(getattr(alg, "last_step_losses", [])):
        out[f"step_loss/{i}"] = sha_float(v)
    mods = [("policy", alg.policy, alg.optimizer)]
    if getattr(alg, "rnd", None):
        mods.append(("rnd", alg.rnd, alg.rnd_optimizer))
    for tag, mod, opt in mods:
        out.update({f"{tag}/{k}": sha(v) for k, v in mod.state_dict().items()})
        for i, st in opt.state_dict()["state"].items():
            out.update({f"{tag}_opt/{i}/{k}": sha(v) for k, v in st.items() if isinstance(v, torch.Tensor)})
    hidden = getattr(alg, "last_hidden_states", None)
    flat = []
    for h in hidden if isinstance(hidden, (tuple, list)) else []:
        flat += list(h) if isinstance(h, (tuple, list)) else [h]
    out.update({f"hidden/{i}": sha(h) for i, h in enumerate(flat) if h is not None})
    return out


def build_plain(golden, case, dev):
    """The set-ups of tests/test_gpu_update.py (update_c1: the stored storage, a world-1 multi-GPU update) and of
    tests/test_gpu_update_c3.py (update_c3: the storage regenerated from the fixture's seed)."""
    import numpy as np
    import torch
    from conftest import golden_path
    from rsl_rl_amd.algorithms import PPO
    from rsl_rl_amd.modules import ActorCritic
    from test_gpu_update_c3 import storage_c3

    m, z = golden[case], np.load(golden_path(case + ".npz"))
    T, N, O, A = m["T"], m["N"], m["O"], m["A"]
    obs0 = {"policy": torch.zeros(N, O)}
    pol = ActorCritic(obs0, {"policy": ["policy"], "critic": ["policy"]}, A, actor_hidden_dims=m["hidden"],
                      critic_hidden_dims=m["hidden"])
    pol.load_state_dict({k[5:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("init/")})
    c1 = case == "update_c1"
    alg = PPO(pol, num_learning_epochs=m["E"], num_mini_batches=m["M"], device=dev,
              multi_gpu_cfg={"global_rank": 0, "local_rank": 0, "world_size": 1} if c1 else None)
    alg.init_storage("rl", N, T, obs0, [A])
    if c1:
        f = {k: torch.from_numpy(z[f"storage/{k}"]) for k in ("rewards", "values", "actions_log_prob", "mu", "sigma",
                                                              "actions", "dones", "obs_policy", "last_obs")}
    else:
        nz = storage_c3(m["noise_seed"], T, N, O, A)
        f = {k: torch.from_numpy(nz[k]) for k in ("rewards", "values", "mu", "dones", "last_obs")}
        f.update(obs_policy=torch.from_numpy(nz["obs"]), actions_log_prob=torch.from_numpy(nz["logp"]),
                 sigma=torch.from_numpy(z["std"]).reshape(1, 1, A).expand(T, N, A))
        f["actions"] = f["mu"] + f["sigma"] * torch.from_numpy(nz["noise"])  # the fixture's fp32 mul then add
    alg.storage.observations["policy"].copy_(f["obs_policy"])
    for k in ("rewards", "values", "actions_log_prob", "mu", "sigma", "actions", "dones"):
        getattr(alg.storage, k).copy_(f[k])
    alg.storage.step = T
    with torch.inference_mode():
        alg.compute_returns({"policy": f["last_obs"].to(dev)})
    torch.default_generator.set_state(torch.from_numpy(z["gen_state"].copy()))
    return alg


def single_rank_cases(dev):
    """[(name, build)]: build() returns the algorithm ready for update(); a `patch` context wraps both."""
    import contextlib

    import numpy as np
    import distill_fixtures as DF
    import drec_fixtures as DR
    import recurrent_fixtures as RF
    import test_gpu_symmetry_update as SY
    from conftest import GOLDEN, golden_path
    from rsl_rl_amd.modules import ActorCritic, SignedPermutationSymmetry
    from update_fixtures import build_update

    with open(os.path.join(GOLDEN, "golden.json")) as f:
        golden = json.load(f)

    @contextlib.contextmanager
    def autograd_path():
        orig = ActorCritic.manual_update_ok
        ActorCritic.manual_update_ok = lambda self, obs: False
        try:
            yield
        finally:
            ActorCritic.manual_update_ok = orig

    @contextlib.contextmanager
    def per_step_path():
        prev = os.environ.get("RSLRL_DISTILL_FUSED")
        os.environ["RSLRL_DISTILL_FUSED"] = "0"
        try:
            yield
        finally:
            os.environ.pop("RSLRL_DISTILL_FUSED") if prev is None else os.environ.update(RSLRL_DISTILL_FUSED=prev)

    plain = contextlib.nullcontext

    def std_update(npz, meta, prefix="r0/"):
        rank_meta = meta["ranks"][0] if "ranks" in meta else meta
        return lambda: build_update(np.load(golden_path(npz)), prefix, meta, rank_meta, dev)[0]

    def sym(case, form):
        def build():
            meta = SY.META[case]
            alg = std_update(f"update_sym_{case}.npz", meta)()
            s = meta["symmetry"]
            fn = SignedPermutationSymmetry(*SY.tables(meta)) if form == "declarative" else SY.opaque(meta)
            alg.symmetry = {"use_data_augmentation": s["use_data_augmentation"],
                            "use_mirror_loss": s["use_mirror_loss"], "mirror_loss_coeff": s["mirror_loss_coeff"],
                            "data_augmentation_func": fn, "_env": None}
            return alg
        return build

    cases = [("update_c1", lambda: build_plain(golden, "update_c1", dev), plain),
             ("update_c2", std_update("update_c2.npz", golden["update_c2"], ""), plain),
             ("update_c3", lambda: build_plain(golden, "update_c3", dev), plain)]
    for case in ("rnd_c5_w1", "rnd_statenorm_w1"):
        cases.append((f"update_{case}", std_update(f"update_{case}.npz", golden["update_rnd"][case]), plain))
    for case in ("sdstd_scalar", "sdstd_log", "logstd"):
        build = std_update(f"update_{case}.npz", golden["update_std"][case])
        cases += [(f"update_{case}", build, plain), (f"update_{case}/autograd", build, autograd_path)]
    for case in "abcde":
        cases.append((f"update_sym_{case}", sym(case, "declarative"), plain))
    cases += [("update_sym_a/opaque", sym("a", "opaque"), plain),
              ("update_sym_a/autograd", sym("a", "declarative"), autograd_path)]
    rmeta = RF.load_meta()
    for case in ("rec_a", "rec_b", "rec_c"):
        cases.append((case, lambda m=rmeta[case]: RF.build_update(RF.Arrays(m["files"]), m, dev)[0], plain))
    dmeta = DF.load_meta()
    for case in "abc":
        build = lambda c=case: DF.build_distillation(DF.load_arrays(c, dmeta[c]), dmeta[c], 0, dev)[0]  # noqa: E731
        cases.append((f"distill_{case}", build, plain))
        if case == "a":
            cases.append((f"distill_{case}/per_step", build, per_step_path))
    qmeta = DR.load_meta()
    for case in "abc":
        build = lambda m=qmeta[case]: DR.build_distillation(DR.load_arrays(m), m, dev)[0]  # noqa: E731
        cases.append((f"drec_{case}", build, plain))
        if case == "c":
            cases.append((f"drec_{case}/per_step", build, per_step_path))
    return cases


def rank_worker(rank, world, port, root, case, family, out_dir):
    use_tree(root)
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    import numpy as np
    import torch
    import torch.distributed as dist

    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from conftest import GOLDEN
        if family is None:
            import distill_fixtures as DF
            meta = DF.load_meta()["w2"]
            alg, _ = DF.build_distillation(DF.load_arrays("w2", meta), meta, rank, "cuda:0", world=world)
        else:
            from update_fixtures import build_update
            with open(os.path.join(GOLDEN, "golden.json")) as f:
                meta = json.load(f)[family][case]
            z = np.load(os.path.join(GOLDEN, f"update_{case}.npz"))
            alg, _ = build_update(z, f"r{rank}/", meta, meta["ranks"][rank], "cuda:0", world=world, rank=rank)
        table = digest(alg, alg.update())
        torch.cuda.synchronize()
        with open(os.path.join(out_dir, f"rank{rank}.json"), "w") as f:
            json.dump(table, f)
    finally:
        dist.destroy_process_group()


def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def run(root, table_path, only=None):
    use_tree(root)
    import torch
    import torch.distributed as dist
    import torch.multiprocessing as mp

    dev = torch.device("cuda:0")
    tables = {}
    fd, path = tempfile.mkstemp()
    os.close(fd)
    dist.init_process_group("gloo", init_method=f"file://{path}", rank=0, world_size=1)  # update_c1's world-1 group
    try:
        for name, build, patch in single_rank_cases(dev):
            if only and not any(name.startswith(o) for o in only):
                continue
            with patch():
                alg = build()
                tables[name] = digest(alg, alg.update())
            torch.cuda.synchronize()
            print(name, len(tables[name]), "hashes", flush=True)
            del alg
    finally:
        dist.destroy_process_group()
        os.unlink(path)
    for case, family in MULTI:
        if only and not any(case.startswith(o) for o in only):
            continue
        world = 2 if family is None or "w2" in case else int(case[1:])
        with tempfile.TemporaryDirectory() as d:
            # (a failed rank raises here: nothing more is started after it)
            mp.start_processes(rank_worker, args=(world, free_port(), root, case, family, d), nprocs=world, join=True,
                               start_method="spawn")
            for r in range(world):
                with open(os.path.join(d, f"rank{r}.json")) as f:
                    tables[f"{case if family is None else 'update_' + case}/rank{r}"] = json.load(f)
        print(case, world, "ranks", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(table_path)), exist_ok=True)
    with open(table_path, "w") as f:
        json.dump(tables, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps({"cases": len(tables), "hashes": sum(len(v) for v in tables.values())}))
    return 0


def compare(paths, out):
    p1, p2, branch = (json.load(open(p)) for p in paths)
    unstable = sorted(c for c in p1 if p1[c] != p2.get(c))
    differ = sorted(f"{c}: {k}" for c in p1 if c not in unstable for k in p1[c] if branch.get(c, {}).get(k) != p1[c][k])

    def fold(case):  # one SHA-256 over a case's sorted (name, hash) pairs: the stored file stays small
        return hashlib.sha256(json.dumps(sorted(case.items())).encode()).hexdigest()

    res = {"cases": len(p1), "hashes": sum(len(v) for v in p1.values()), "parent_unstable": unstable, "differ": differ,
           "identical": not differ and p1.keys() == p2.keys() == branch.keys(),
           # per case: the folded hash where the three tables agree, else one per table
           "per_case": {c: fold(p1[c]) if p1[c] == p2.get(c) == branch.get(c) else
                        {"parent": fold(p1[c]), "parent_again": fold(p2.get(c, {})), "branch": fold(branch.get(c, {}))}
                        for c in p1}}
    print(json.dumps({k: res[k] for k in ("cases", "hashes", "parent_unstable", "differ", "identical")}))
    if out:
        with open(out, "w") as f:
            json.dump(res, f, indent=1, sort_keys=True)
            f.write("\n")
    return 0 if res["identical"] else 1


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--root", default=HERE, help="the checkout to measure (default: this one)")
    ap.add_argument("--table", help="where to write this run's table")
    ap.add_argument("--only", nargs="*", help="case-name prefixes (default: every case)")
    ap.add_argument("--compare", nargs=3, metavar=("PARENT_1", "PARENT_2", "THIS"))
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.compare:
        return compare(a.compare, a.out)
    if not a.table:
        ap.error("--table or --compare")
    return run(os.path.abspath(a.root), a.table, a.only)


if __name__ == "__main__":
    sys.exit(main())
