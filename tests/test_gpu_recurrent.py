"""Recurrent PPO on the GPU: the trajectory kernels against the reference's fixtures and against the torch form (bit
for bit), unpad's autograd, the whole update against the reference's rec_* fixtures, the host read-backs of an update
and of a rollout step, and a runner end to end."""

import os

import numpy as np
import pytest
import torch

import recurrent_fixtures as RF
from test_recurrent_host import GEN_CASES, META, check_generator, gen_storage
from update_fixtures import param_errors, run_recorded_update

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("record_layout", ["1", "0"])
@pytest.mark.parametrize("case", GEN_CASES)
def test_generator_matches_the_reference(cuda_device, monkeypatch, case, record_layout):
    monkeypatch.setenv("RSLRL_RECORD_LAYOUT", record_layout)
    st, z, m = gen_storage(case, cuda_device)
    assert (st.records is not None) == (record_layout == "1")
    batches = check_generator(st, z, m)
    for obs_b, *_, (hid_a, hid_c), masks_b in batches:
        # every mini-batch's slice is contiguous (what nn.LSTM wants), and the masks carry the index map
        assert all(v.is_contiguous() for v in obs_b.values()) and masks_b.is_contiguous()
        assert masks_b.trajectory_map.n_b == masks_b.shape[1]
    # two calls give equal bytes
    again = list(st.recurrent_mini_batch_generator(m["M"], 1))
    for a, b in zip(batches, again):
        for k in m["widths"]:
            assert torch.equal(a[0][k], b[0][k])
        assert torch.equal(a[9], b[9])


@pytest.mark.parametrize("case", GEN_CASES)
def test_split_pad_unpad_on_the_device(cuda_device, case):
    from rsl_rl_amd.utils import split_and_pad_trajectories, unpad_trajectories
    st, z, m = gen_storage(case, cuda_device)
    padded, masks = split_and_pad_trajectories(st.observations, st.dones)
    for k in m["widths"]:
        assert np.array_equal(padded[k].cpu().numpy(), z["pad/" + k]), k
        # a plain bool mask: the reference's boolean indexing
        assert torch.equal(unpad_trajectories(padded[k], masks), st.observations[k])
    assert masks.dtype == torch.bool and np.array_equal(masks.cpu().numpy(), z["pad/masks"])


def _device_case(dev, T=24, N=4096, p=0.05, widths=(48, 12), L=1, H=16, seed=7):
    g = torch.Generator().manual_seed(seed)
    dones = (torch.rand(T, N, generator=g) < p).to(torch.uint8).to(dev)
    groups = [torch.randn(T, N, w, generator=g).to(dev) for w in widths]
    states = [torch.randn(T, L, N, H, generator=g).to(dev) for _ in range(2)]
    return dones, groups, states


def test_index_and_pad_match_the_torch_form_beyond_one_block(cuda_device):
    """T 24, N 4096 (16 blocks of envs: the prefix sum spans blocks), 5 % dones, 3 mini-batches with 1 env dropped."""
    from rsl_rl_amd import kernels
    from rsl_rl_amd.utils.utils import trajectory_index_torch
    T, N, M = 24, 4096, 3
    E = N // M
    dones, groups, states = _device_case(cuda_device)
    traj, off, prefix = trajectory_index_torch(dones)
    ix = kernels.trajectory_index(dones, M)
    assert torch.equal(ix.traj_id.long(), traj) and torch.equal(ix.traj_off.long(), off)
    assert torch.equal(ix.env_prefix.long(), prefix)
    bounds = ix.read_bounds()
    assert bounds == prefix[torch.arange(M + 1, device=cuda_device) * E].tolist()
    padded, masks, gathered = kernels.trajectory_pad(ix, groups, states)
    n_used = bounds[-1]
    tr, of = traj[:, :M * E], off[:, :M * E]
    for g, flat in zip(groups, padded):
        ref = torch.zeros(T, n_used, g.shape[-1], device=cuda_device)
        ref[of, tr] = g[:, :M * E]
        for i, v in enumerate(kernels.trajectory_views(ix, flat, T, g.shape[-1])):
            assert torch.equal(v, ref[:, bounds[i]:bounds[i + 1]]), i
    ref_m = torch.zeros(T, n_used, dtype=torch.bool, device=cuda_device)
    ref_m[of, tr] = True
    for i, v in enumerate(kernels.trajectory_views(ix, masks, T, None)):
        assert torch.equal(v, ref_m[:, bounds[i]:bounds[i + 1]])
    starts = (off.t() == 0)[:M * E]
    for s, flat in zip(states, gathered):
        first = s.permute(2, 0, 1, 3)[:M * E][starts]
        for i, v in enumerate(kernels.trajectory_views(ix, flat, s.shape[1], s.shape[3])):
            assert torch.equal(v, first[bounds[i]:bounds[i + 1]].transpose(1, 0)), i
    # two calls give equal bytes
    padded2, masks2, gathered2 = kernels.trajectory_pad(kernels.trajectory_index(dones, M), groups, states)
    assert all(torch.equal(a, b) for a, b in zip(padded + gathered + [masks], padded2 + gathered2 + [masks2]))


def test_unpad_forward_and_backward_equal_boolean_indexing(cuda_device):
    from rsl_rl_amd import kernels
    from rsl_rl_amd.utils import unpad_trajectories
    T, N, M, H = 24, 515, 2, 20  # 257 envs per mini-batch (more than one block of rows), env 514 dropped
    E = N // M
    dones, _, _ = _device_case(cuda_device, T, N, 0.07, (), seed=11)
    ix = kernels.trajectory_index(dones, M)
    b = ix.read_bounds()
    g = torch.Generator().manual_seed(5)
    for i in range(M):
        n_b = b[i + 1] - b[i]
        x = torch.randn(T, n_b, H, generator=g).to(cuda_device)
        _, masks, _ = kernels.trajectory_pad(ix, [], [])
        masks_b = kernels.trajectory_views(ix, masks, T, None)[i]
        plain = masks_b.clone()  # no index map: boolean indexing
        masks_b.trajectory_map = kernels.TrajectoryMap(ix, i * E, E, b[i], n_b)
        w = torch.randn(T, E, H, generator=g).to(cuda_device)
        xa, xb = x.clone().requires_grad_(), x.clone().requires_grad_()
        ya = unpad_trajectories(xa, masks_b)
        yb = xb.permute(1, 0, 2)[plain.t()].reshape(E, T, H).permute(1, 0, 2)  # boolean indexing under autograd
        assert ya.shape == (T, E, H) and torch.equal(ya, yb)
        assert torch.equal(unpad_trajectories(x, plain), yb)  # a plain bool mask: the same values
        (ya * w).sum().backward()
        (yb * w).sum().backward()
        assert torch.equal(xa.grad, xb.grad)
        assert (xa.grad[~plain] == 0).all()


def _run_update(case, dev):
    meta = META[case]
    z = RF.Arrays(meta["files"])
    alg, pol = RF.build_update(z, meta, dev)
    grads = [None]
    loss, lr_trace = run_recorded_update(alg, grads)
    out = {"loss": loss, "lr_trace": lr_trace, "lr": alg.learning_rate, "grad_mb0": grads[0],
           "final": pol.state_dict()}
    return out, z, meta


@pytest.mark.parametrize("case", ["rec_a", "rec_b", "rec_c"])
def test_update_matches_the_reference(cuda_device, case):
    out, z, meta = _run_update(case, cuda_device)
    assert len(out["lr_trace"]) == meta["E"] * meta["M"]
    # PyTorch's own GPU autograd on the same fixture: the yardstick where the RNN library's fp32 differs from the CPU's
    alg, pol = RF.build_update(z, meta, cuda_device)
    RF.torch_baseline_update(alg, pol)
    baseline = param_errors(pol.state_dict(), z, "r0/")
    RF.check_recurrent_update(out, z, meta, baseline, mode=case)


def test_update_reads_the_device_back_twice(cuda_device):
    """One update() of rec_a under torch's sync debug mode: any synchronising call raises, except the two sanctioned
    read-backs (the trajectory boundaries before the first mini-batch, the statistics at the end), which are the
    only .tolist() calls on device tensors."""
    meta = META["rec_a"]
    z = RF.Arrays(meta["files"])
    alg, _ = RF.build_update(z, meta, cuda_device)
    reads = []
    tolist = torch.Tensor.tolist

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
    assert len(reads) == 2 and reads[0] == meta["M"] + 1, reads
    assert all(np.isfinite(v) for v in loss.values())


def test_rollout_step_has_no_read_back(cuda_device):
    from rsl_rl_amd.algorithms import PPO
    from rsl_rl_amd.modules import ActorCriticRecurrent
    torch.manual_seed(0)
    N, O, A, T = 64, 16, 4, 4
    obs0 = {"policy": torch.zeros(N, O)}
    pol = ActorCriticRecurrent(obs0, {"policy": ["policy"], "critic": ["policy"]}, A, actor_hidden_dims=[32],
                               critic_hidden_dims=[32], rnn_hidden_dim=32)
    alg = PPO(pol, device=cuda_device)
    alg.init_storage("rl", N, T, obs0, [A])
    obs = [{"policy": torch.randn(N, O, device=cuda_device)} for _ in range(T)]
    rew = torch.randn(N, device=cuda_device)
    dones = (torch.rand(N, device=cuda_device) < 0.3).long()
    with torch.inference_mode():
        alg.act(obs[0])  # warm-up: allocations, library initialisation
        alg.process_env_step(obs[0], rew, dones, {})
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            for t in range(1, T):
                alg.act(obs[t])
                alg.process_env_step(obs[t], rew, dones, {})
        finally:
            torch.cuda.set_sync_debug_mode("default")
    h, c = pol.get_hidden_states()[0]
    assert (h[:, dones == 1] == 0.0).all() and (c[:, dones == 1] == 0.0).all() and (h[:, dones == 0] != 0).any()
    assert alg.storage.saved_hidden_states_a[0].shape == (T, 1, N, 32)


@pytest.mark.parametrize("rnn", ["lstm", "gru"])
def test_runner_end_to_end(cuda_device, tmp_path, rnn):
    from rsl_rl_amd.env import SyntheticVecEnv
    from rsl_rl_amd.runners import OnPolicyRunner
    torch.manual_seed(1)
    env = SyntheticVecEnv(256, 16, 4, device=cuda_device, seed=0)
    cfg = {"num_steps_per_env": 8, "save_interval": 100, "obs_groups": {"policy": ["policy"]},
           "policy": {"class_name": "ActorCriticRecurrent", "actor_hidden_dims": [32, 32],
                      "critic_hidden_dims": [32, 32], "rnn_type": rnn, "rnn_hidden_dim": 32, "rnn_num_layers": 1},
           "algorithm": {"class_name": "PPO", "num_learning_epochs": 2, "num_mini_batches": 2}}
    runner = OnPolicyRunner(env, cfg, log_dir=None, device="cuda:0")
    runner.learn(2)
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
    policy = runner.get_inference_policy(device="cuda:0")
    with torch.inference_mode():
        act = policy(env.get_observations().to("cuda:0"))
    assert act.shape == (256, 4) and torch.isfinite(act).all()
