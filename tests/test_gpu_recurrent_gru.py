"""The recurrent PPO update of a GRU policy on the fused GRU kernels (PPO._recurrent_minibatch): the whole
update against the reference's rec_e fixture with the launches counted, the same check with RSLRL_RECURRENT_FUSED=0,
the update's one read-back, the memories' states and the arena, and a runner end to end."""

import os

import numpy as np
import pytest
import torch

import gru_fixtures as GF
import recurrent_fixtures as RF
from update_fixtures import run_recorded_update

pytestmark = pytest.mark.gpu
META_E = GF.load_meta()


@pytest.fixture
def pair_launches(monkeypatch):
    """Counts the paired forward launches of the fused GRU step."""
    from rsl_rl_amd import kernels
    calls = []
    inner = kernels.gru_cell_train_pair

    def spy(*a, **k):
        calls.append(1)
        return inner(*a, **k)

    monkeypatch.setattr(kernels, "gru_cell_train_pair", spy)
    return calls


def _run_update(meta, dev):
    z = RF.Arrays(meta["files"])
    alg, pol = RF.build_update(z, meta, dev)
    grads = [None]
    loss, lr_trace = run_recorded_update(alg, grads)
    out = {"loss": loss, "lr_trace": lr_trace, "lr": alg.learning_rate, "grad_mb0": grads[0],
           "final": pol.state_dict()}
    return out, z


def test_rec_e_update_matches_the_reference(cuda_device, pair_launches):
    meta = META_E["rec_e"]
    out, z = _run_update(meta, cuda_device)
    assert len(pair_launches) == meta["E"] * meta["M"] * meta["T"] == 32
    RF.check_recurrent_update(out, z, meta, mode="rec_e fused")


def test_rec_e_without_the_fused_path(cuda_device, pair_launches, monkeypatch):
    monkeypatch.setenv("RSLRL_RECURRENT_FUSED", "0")
    meta = META_E["rec_e"]
    out, z = _run_update(meta, cuda_device)
    assert not pair_launches
    RF.check_recurrent_update(out, z, meta, mode="rec_e autograd")


def test_update_reads_the_device_back_once(cuda_device, pair_launches):
    """One update() of rec_e under torch's sync debug mode: any synchronising call raises, except the one sanctioned
    read-back (the statistics at the end), the only .tolist() of a device tensor.  The memories' hidden states are not
    touched, and every parameter's gradient is a view of the one arena."""
    meta = META_E["rec_e"]
    z = RF.Arrays(meta["files"])
    alg, pol = RF.build_update(z, meta, cuda_device)
    alg.update()  # warm-up: allocations, the arena
    alg, pol = RF.build_update(z, meta, cuda_device)
    states = {n: m.hidden_states for n, m in (("a", pol.memory_a), ("c", pol.memory_c))}
    assert torch.is_tensor(states["c"])  # compute_returns' evaluate advanced the critic's memory: a bare tensor
    before = {n: None if s is None else s.clone() for n, s in states.items()}
    reads = []
    tolist = torch.Tensor.tolist
    del pair_launches[:]

    def counted(self):
        if not self.is_cuda:
            return tolist(self)
        reads.append(self.numel())
        torch.cuda.set_sync_debug_mode("default")
        try:
            return tolist(self)
        finally:
            torch.cuda.set_sync_debug_mode("error")

    torch.cuda.synchronize()
    torch.Tensor.tolist = counted
    torch.cuda.set_sync_debug_mode("error")
    try:
        loss = alg.update()
    finally:
        torch.cuda.set_sync_debug_mode("default")
        torch.Tensor.tolist = tolist
    assert len(pair_launches) == 32  # the update under watch ran on the fused kernels
    assert len(reads) == 1, reads
    assert all(np.isfinite(v) for v in loss.values())
    for n, m in (("a", pol.memory_a), ("c", pol.memory_c)):
        assert m.hidden_states is states[n]
        if before[n] is not None:
            assert torch.equal(m.hidden_states, before[n])
    arena = alg.grad_arena()
    lo, hi = arena.flat.data_ptr(), arena.flat.data_ptr() + 4 * arena.numel
    for name, p in pol.named_parameters():
        assert p.grad is not None and lo <= p.grad.data_ptr() and p.grad.data_ptr() + 4 * p.numel() <= hi, name
        assert p.grad.data_ptr() == arena.slot(p).data_ptr(), name


def test_runner_end_to_end(cuda_device, tmp_path, pair_launches):
    from rsl_rl_amd.env import SyntheticVecEnv
    from rsl_rl_amd.runners import OnPolicyRunner
    torch.manual_seed(1)
    env = SyntheticVecEnv(256, 16, 4, device=cuda_device, seed=0)
    cfg = {"num_steps_per_env": 8, "save_interval": 100, "obs_groups": {"policy": ["policy"]},
           "policy": {"class_name": "ActorCriticRecurrent", "actor_hidden_dims": [32, 32],
                      "critic_hidden_dims": [32, 32], "rnn_type": "gru", "rnn_hidden_dim": 256, "rnn_num_layers": 1},
           "algorithm": {"class_name": "PPO", "num_learning_epochs": 2, "num_mini_batches": 2}}
    runner = OnPolicyRunner(env, cfg, log_dir=None, device="cuda:0")
    runner.learn(2)
    assert len(pair_launches) == 2 * 32  # per iteration 2 epochs x 2 mini-batches x 8 steps = 32, E = 128
    losses = runner.last_iteration_stats["loss_dict"]
    assert all(np.isfinite(v) for v in losses.values()), losses
    path = os.path.join(tmp_path, "model.pt")
    runner.save(path)
    before = {k: v.clone() for k, v in runner.alg.policy.state_dict().items()}
    with torch.no_grad():
        for p in runner.alg.policy.parameters():
            p.add_(1.0)
    runner.load(path)
    after = runner.alg.policy.state_dict()
    assert all(torch.equal(before[k], after[k]) for k in before)
