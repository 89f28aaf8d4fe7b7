"""Multi-rank Distillation.update() against the reference's own two-rank update (tests/golden/distill_w2.npz: the
reference ran with world_size 2 over a gloo group on CPU, every rank its own observation shard, the gradients averaged
by reduce_parameters, distillation.py:166-185).  Here the same ranks run our update on the GPU the way
tests/test_multi_rank_update.py runs its cases: spawned processes, all on cuda:0, a gloo group (RCCL refuses two ranks
on one device); each optimizer step issues ONE all-reduce of the student's gradient arena.  Per rank the tolerances of
tests/test_gpu_distillation.py apply, and both ranks must end with bit-identical student parameters."""

import os
import socket
import tempfile

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from conftest import ROOT

pytestmark = pytest.mark.gpu


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, case, out_dir):
    import sys

    for p in (ROOT, os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import torch.distributed as dist

    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from distill_fixtures import build_distillation, load_arrays, load_meta, run_recorded_update

        meta = load_meta()[case]
        z = load_arrays(case, meta)
        alg, pol = build_distillation(z, meta, rank, "cuda:0", world=world)
        assert alg._fused_ok()
        out = run_recorded_update(alg)
        out["teacher_unchanged"] = all(p.grad is None for n, p in pol.named_parameters()
                                       if not n.startswith("student."))
        torch.save(out, os.path.join(out_dir, f"rank{rank}.pt"))
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(600)
def test_two_rank_update_matches_reference(cuda_device):
    from distill_fixtures import load_arrays, load_meta
    from update_fixtures import check_update

    case = "w2"
    meta = load_meta()[case]
    world = meta["world"]
    z = load_arrays(case, meta)
    with tempfile.TemporaryDirectory() as d:
        mp.start_processes(_worker, args=(world, _free_port(), case, d), nprocs=world, join=True,
                           start_method="spawn")
        res = [torch.load(os.path.join(d, f"rank{r}.pt"), weights_only=True) for r in range(world)]
    for r, out in enumerate(res):
        ref = meta["ranks"][r]
        assert len(out["lr_trace"]) == ref["num_steps"]
        ours, ref_steps = np.asarray(out["step_losses"]), z[f"r{r}/step_losses"]
        assert np.all(np.abs(ours - ref_steps) <= 1e-4 * np.abs(ref_steps)), (r, ours, ref_steps)
        check_update(out, z, meta, r, mode="w2")
        assert out["teacher_unchanged"]
    assert res[0]["loss"] != res[1]["loss"]  # per-rank means over different shards
    for k, v in res[0]["final"].items():  # data parallel: identical parameters on every rank
        assert torch.equal(v, res[1]["final"][k]), k
    assert torch.equal(res[0]["grad_mb0"], res[1]["grad_mb0"])
