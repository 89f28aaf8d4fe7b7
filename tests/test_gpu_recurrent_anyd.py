"""The recurrent PPO update at observation widths that are no multiple of 16: the whole update against
the reference's rec_f (LSTM, 45 observations) and rec_g (GRU, 235 observations) fixtures on the fused path with the
launches counted, the same check with RSLRL_RECURRENT_FUSED=0, the update's one read-back and the arena, two memories of
unequal widths (45 and 53) against fp64 autograd, and a runner end to end at 45 observations."""

import copy
import json
import os

import numpy as np
import pytest
import torch

import gru_fixtures as GF
import recurrent_fixtures as RF
import recurrent_fused_fixtures as RFF
from update_fixtures import run_recorded_update

pytestmark = pytest.mark.gpu

with open(os.path.join(RF.GOLDEN, "golden_recurrent_anyd.json")) as _f:
    META = json.load(_f)
CASES = {"rec_f": "lstm", "rec_g": "gru"}


def _count(monkeypatch, kind):
    """Counts the paired forward launches of the fused step of that kind."""
    from rsl_rl_amd import kernels
    calls = []
    name = f"{kind}_cell_train_pair"
    inner = getattr(kernels, name)

    def spy(*a, **k):
        calls.append(1)
        return inner(*a, **k)

    monkeypatch.setattr(kernels, name, spy)
    return calls


def _tolerance_meta(meta):
    """check_recurrent_update selects its parameter tolerance by the widest layer of the trained networks, which here
    is the 256-wide memory in front of the [128, 64] MLPs: the reference's own one-ulp sensitivity envelope."""
    return dict(meta, hidden=list(meta["hidden"]) + [meta["H"]])


def _run_update(meta, dev):
    z = RF.Arrays(meta["files"])
    alg, pol = RF.build_update(z, meta, dev)
    grads = [None]
    loss, lr_trace = run_recorded_update(alg, grads)
    out = {"loss": loss, "lr_trace": lr_trace, "lr": alg.learning_rate, "grad_mb0": grads[0],
           "final": pol.state_dict()}
    return out, z, alg, pol


@pytest.mark.parametrize("case", sorted(CASES))
def test_update_matches_the_reference(cuda_device, case, monkeypatch):
    from rsl_rl_amd import kernels
    meta = META[case]
    assert meta["rnn_type"] == CASES[case] and meta["O"] % 16 and kernels._rnn_anyd(meta["O"])
    calls = _count(monkeypatch, CASES[case])
    out, z, alg, pol = _run_update(meta, cuda_device)
    assert alg._recurrent_fused_ok()
    assert len(calls) == meta["E"] * meta["M"] * meta["T"] == 32
    RF.check_recurrent_update(out, z, _tolerance_meta(meta), mode=case + " fused")


@pytest.mark.parametrize("case", sorted(CASES))
def test_update_without_the_fused_path(cuda_device, case, monkeypatch):
    monkeypatch.setenv("RSLRL_RECURRENT_FUSED", "0")
    meta = META[case]
    calls = _count(monkeypatch, CASES[case])
    out, z, _, _ = _run_update(meta, cuda_device)
    assert not calls
    RF.check_recurrent_update(out, z, _tolerance_meta(meta), mode=case + " autograd")


@pytest.mark.parametrize("case", sorted(CASES))
def test_update_reads_the_device_back_once(cuda_device, case, monkeypatch):
    """One update() under torch's sync debug mode: any synchronising call raises, except the one sanctioned read-back
    (the statistics at the end); every parameter's gradient is a view of the one arena."""
    meta = META[case]
    z = RF.Arrays(meta["files"])
    alg, pol = RF.build_update(z, meta, cuda_device)
    alg.update()  # warm-up: allocations, the arena
    alg, pol = RF.build_update(z, meta, cuda_device)
    calls = _count(monkeypatch, CASES[case])
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
    assert len(calls) == 32  # the update under watch ran on the fused kernels
    assert len(reads) == 1, reads
    assert all(np.isfinite(v) for v in loss.values())
    arena = alg.grad_arena()
    lo, hi = arena.flat.data_ptr(), arena.flat.data_ptr() + 4 * arena.numel
    for name, p in pol.named_parameters():
        assert p.grad is not None and lo <= p.grad.data_ptr() and p.grad.data_ptr() + 4 * p.numel() <= hi, name
        assert p.grad.data_ptr() == arena.slot(p).data_ptr(), name


# ---- two memories of unequal widths: the policy group 45 wide, the critic's groups 45 + 8 = 53
def _unequal_update(kind, dev, seed=7):
    """(PPO, policy) with 64 envs, T 4, one mini-batch, one epoch, the storage filled from a seed."""
    from rsl_rl_amd.algorithms import PPO
    from rsl_rl_amd.modules import ActorCriticRecurrent
    T, N, A, H = 4, 64, 12, 256
    n_states = 2 if kind == "lstm" else 1
    torch.manual_seed(seed)
    obs0 = {"policy": torch.zeros(N, 45), "priv": torch.zeros(N, 8)}
    groups = {"policy": ["policy"], "critic": ["policy", "priv"]}
    pol = ActorCriticRecurrent(obs0, groups, A, actor_hidden_dims=[64, 64], critic_hidden_dims=[64, 64], rnn_type=kind,
                               rnn_hidden_dim=H, rnn_num_layers=1)
    alg = PPO(pol, num_learning_epochs=1, num_mini_batches=1, device=dev, learning_rate=1e-3)
    alg.init_storage("rl", N, T, obs0, [A])
    st = alg.storage
    g = torch.Generator().manual_seed(seed + 1)
    rand = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    st.observations["policy"].copy_(rand(T, N, 45))
    st.observations["priv"].copy_(rand(T, N, 8))
    st.rewards.copy_(rand(T, N, 1))
    dones = (torch.rand(T, N, 1, generator=g) < 0.15).to(torch.uint8)
    dones[1, 3] = dones[2, 3] = dones[0, 40] = dones[T - 1, 41] = 1
    st.dones.copy_(dones)
    mu, sigma = 0.3 * rand(T, N, A), torch.full((T, N, A), 1.0)
    actions = mu + sigma * rand(T, N, A)
    st.mu.copy_(mu)
    st.sigma.copy_(sigma)
    st.actions.copy_(actions)
    st.values.copy_(rand(T, N, 1))
    st.actions_log_prob.copy_(torch.distributions.Normal(mu, sigma).log_prob(actions).sum(-1, keepdim=True))
    st.saved_hidden_states_a = [(0.3 * rand(T, 1, N, H)).to(dev) for _ in range(n_states)]
    st.saved_hidden_states_c = [(0.3 * rand(T, 1, N, H)).to(dev) for _ in range(n_states)]
    st.step = T
    last = {"policy": rand(N, 45).to(dev), "priv": rand(N, 8).to(dev)}
    with torch.inference_mode():
        alg.compute_returns(last)
    return alg, pol


def _to64(x):
    if torch.is_tensor(x):
        return x.detach().cpu().double() if x.is_floating_point() else x.detach().cpu()
    if isinstance(x, (tuple, list)):
        return tuple(_to64(v) for v in x)
    return {k: _to64(x[k]) for k in x.keys()}


@pytest.mark.parametrize("kind", ["lstm", "gru"])
def test_unequal_memory_widths_against_fp64_autograd(cuda_device, kind, monkeypatch):
    """One fused update() against the same mini-batch's loss under fp64 autograd on the CPU: per parameter the gradient's
    RMS error -- the project's measure wherever torch's fp32 result is the yardstick (tests/test_gpu_lstm_cell.py,
    test_gpu_lstm_train.py, test_gpu_gru_cell.py) -- is at most 2x that of the fp32 autograd path
    (RSLRL_RECURRENT_FUSED=0) on the same device.  The largest single-element errors are printed beside it: measured
    on an MI355X they lie between 0.2x and 1.3x torch's for every parameter but the critic LSTM's W_hh, whose one
    worst element of 262,144 is 4.77e-10 against torch's 2.37e-10 (dW_hh and the reverse steps are the kernels of
    DESIGN §18, which this width-independent path shares with obs 48)."""
    from rsl_rl_amd import kernels
    from rsl_rl_amd.networks import fused_mlp
    dev = cuda_device
    # the fp64 gradient of the one mini-batch
    alg, pol = _unequal_update(kind, dev)
    assert alg._recurrent_fused_ok()
    (batch,) = list(alg.storage.recurrent_sequence_generator(1, 1))
    pol64 = copy.deepcopy(pol).cpu().double()
    loss = (GF if kind == "gru" else RFF).sequence_loss(alg, pol64, _to64(tuple(batch)))
    ref = torch.autograd.grad(loss, list(pol64.parameters()))
    names = [n for n, _ in pol.named_parameters()]
    sizes = [p.numel() for p in pol.parameters()]

    def errors(fused):
        monkeypatch.setenv("RSLRL_RECURRENT_FUSED", "1" if fused else "0")
        alg, pol = _unequal_update(kind, dev)
        calls = _count(monkeypatch, kind)
        ragged = fused_mlp.ragged_launches
        grads = [None]
        run_recorded_update(alg, grads)
        assert len(calls) == (4 if fused else 0)
        if fused:  # dW_ih of both memories: one ragged launch per memory and gate block
            assert fused_mlp.ragged_launches - ragged == 2 * (4 if kind == "lstm" else 3)
        parts = torch.split(grads[0].double(), sizes)
        diffs = [g - r.reshape(-1) for g, r in zip(parts, ref)]
        return ({n: d.square().mean().sqrt().item() for n, d in zip(names, diffs)},
                {n: d.abs().max().item() for n, d in zip(names, diffs)})

    assert kernels._rnn_anyd(45, 53)
    (ours, ours_max), (theirs, theirs_max) = errors(True), errors(False)
    for n in names:
        print(f"{kind} {n:28s} rms fused {ours[n]:.2e} autograd {theirs[n]:.2e}; "
              f"max fused {ours_max[n]:.2e} autograd {theirs_max[n]:.2e}")
    bad = {n: (ours[n], theirs[n]) for n in names if ours[n] > 2 * theirs[n]}
    assert not bad, bad


@pytest.mark.parametrize("kind", ["gru", "lstm"])
def test_runner_end_to_end_at_45_observations(cuda_device, tmp_path, kind, monkeypatch):
    from rsl_rl_amd.env import SyntheticVecEnv
    from rsl_rl_amd.runners import OnPolicyRunner
    calls = _count(monkeypatch, kind)
    torch.manual_seed(1)
    env = SyntheticVecEnv(256, 45, 4, device=cuda_device, seed=0)
    cfg = {"num_steps_per_env": 8, "save_interval": 100, "obs_groups": {"policy": ["policy"]},
           "policy": {"class_name": "ActorCriticRecurrent", "actor_hidden_dims": [32, 32],
                      "critic_hidden_dims": [32, 32], "rnn_type": kind, "rnn_hidden_dim": 256, "rnn_num_layers": 1},
           "algorithm": {"class_name": "PPO", "num_learning_epochs": 2, "num_mini_batches": 2}}
    runner = OnPolicyRunner(env, cfg, log_dir=None, device="cuda:0")
    runner.learn(2)
    assert len(calls) == 2 * 32  # per iteration 2 epochs x 2 mini-batches x 8 steps = 32, E = 128
    pol = runner.alg.policy
    with torch.inference_mode():  # the rollout's steps ran on the fused cell too
        x = torch.zeros(256, 45, device=cuda_device)
        assert (pol.memory_a.cell_ok(x), pol.memory_a.gru_cell_ok(x)) == (kind == "lstm", kind == "gru")
    losses = runner.last_iteration_stats["loss_dict"]
    assert all(np.isfinite(v) for v in losses.values()), losses
    path = os.path.join(tmp_path, "model.pt")
    runner.save(path)
    before = {k: v.clone() for k, v in pol.state_dict().items()}
    with torch.no_grad():
        for p in pol.parameters():
            p.add_(1.0)
    runner.load(path)
    after = runner.alg.policy.state_dict()
    assert all(torch.equal(before[k], after[k]) for k in before)
