"""The recurrent PPO update at hidden size 512, and behind a wide MLP at 256 (the lifted §9 item 14e):
one update() against fp64 autograd on the CPU with the launches counted, the update's one read-back and the arena, a
runner end to end, and the RSLRL_RNN_HIDDEN_512=0 routing in a child process.  Follows test_gpu_recurrent_anyd.py."""

import copy
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import gru_fixtures as GF
import recurrent_fused_fixtures as RFF
from update_fixtures import run_recorded_update

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = ["lstm", "gru"]
# (hidden size of the memories, observation width, the MLPs behind them)
SHAPES = {"h512-obs48-narrow": (512, 48, [64, 64]), "h512-obs45-wide": (512, 45, [512, 256, 128]),
          "h256-obs48-wide": (256, 48, [512, 256, 128])}


@pytest.fixture(autouse=True)
def update_at_every_row_count(monkeypatch):
    """The LSTM update of §27 is the default from kernels.RNN_H512_LSTM_UPDATE_MIN_ROWS rows on (a speed rule: below, it
    is no faster than autograd).  These tests are about what it computes, at 64 and 128 rows: they open the gate;
    test_lstm_update_is_gated_by_rows checks the rule itself."""
    from rsl_rl_amd import kernels
    monkeypatch.setattr(kernels, "RNN_H512_LSTM_UPDATE_MIN_ROWS", 0)


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


def _update(kind, dev, H, O, mlp, seed=7):
    """(PPO, policy) with 64 envs, T 4, one mini-batch, one epoch, 12 actions, the storage filled from a seed."""
    from rsl_rl_amd.algorithms import PPO
    from rsl_rl_amd.modules import ActorCriticRecurrent
    T, N, A = 4, 64, 12
    n_states = 2 if kind == "lstm" else 1
    torch.manual_seed(seed)
    obs0 = {"policy": torch.zeros(N, O)}
    groups = {"policy": ["policy"], "critic": ["policy"]}
    pol = ActorCriticRecurrent(obs0, groups, A, actor_hidden_dims=mlp, critic_hidden_dims=mlp, rnn_type=kind,
                               rnn_hidden_dim=H, rnn_num_layers=1)
    alg = PPO(pol, num_learning_epochs=1, num_mini_batches=1, device=dev, learning_rate=1e-3)
    alg.init_storage("rl", N, T, obs0, [A])
    st = alg.storage
    g = torch.Generator().manual_seed(seed + 1)
    rand = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    st.observations["policy"].copy_(rand(T, N, O))
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
    last = {"policy": rand(N, O).to(dev)}
    with torch.inference_mode():
        alg.compute_returns(last)
    return alg, pol


def _to64(x):
    if torch.is_tensor(x):
        return x.detach().cpu().double() if x.is_floating_point() else x.detach().cpu()
    if isinstance(x, (tuple, list)):
        return tuple(_to64(v) for v in x)
    return {k: _to64(x[k]) for k in x.keys()}


@pytest.mark.parametrize("shape", sorted(SHAPES))
@pytest.mark.parametrize("kind", KINDS)
def test_update_against_fp64_autograd(cuda_device, kind, shape, monkeypatch):
    """One fused update() against the same mini-batch's loss under fp64 autograd on the CPU: per parameter the first
    mini-batch's gradient RMS error is at most 2x that of the fp32 autograd path (RSLRL_RECURRENT_FUSED=0) on the same
    device; the largest single-element errors are printed beside it."""
    from rsl_rl_amd.networks import fused_mlp
    dev = cuda_device
    H, O, mlp = SHAPES[shape]
    alg, pol = _update(kind, dev, H, O, mlp)
    assert alg._recurrent_fused_ok()
    wide = len(mlp) == 3
    assert bool(getattr(pol.actor, "_wide", False)) == wide and bool(getattr(pol.actor, "_fused", False)) == (not wide)
    (batch,) = list(alg.storage.recurrent_sequence_generator(1, 1))
    pol64 = copy.deepcopy(pol).cpu().double()
    loss = (GF if kind == "gru" else RFF).sequence_loss(alg, pol64, _to64(tuple(batch)))
    ref = torch.autograd.grad(loss, list(pol64.parameters()))
    names = [n for n, _ in pol.named_parameters()]
    sizes = [p.numel() for p in pol.parameters()]

    def errors(fused):
        monkeypatch.setenv("RSLRL_RECURRENT_FUSED", "1" if fused else "0")
        alg, pol = _update(kind, dev, H, O, mlp)
        assert alg._recurrent_fused_ok() == fused
        calls = _count(monkeypatch, kind)
        launches = fused_mlp.wide_launches
        grads = [None]
        run_recorded_update(alg, grads)
        assert len(calls) == (4 if fused else 0)  # the train-pair launches: T
        if fused and (H == 512 or wide):  # the wide kernels ran: wide layers, 512-wide gate blocks, 512 input columns
            assert fused_mlp.wide_launches > launches
        parts = torch.split(grads[0].double(), sizes)
        diffs = [g - r.reshape(-1) for g, r in zip(parts, ref)]
        return ({n: d.square().mean().sqrt().item() for n, d in zip(names, diffs)},
                {n: d.abs().max().item() for n, d in zip(names, diffs)})

    (ours, ours_max), (theirs, theirs_max) = errors(True), errors(False)
    for n in names:
        print(f"{kind} {shape} {n:28s} rms fused {ours[n]:.2e} autograd {theirs[n]:.2e}; "
              f"max fused {ours_max[n]:.2e} autograd {theirs_max[n]:.2e}")
    bad = {n: (ours[n], theirs[n]) for n in names if ours[n] > 2 * theirs[n]}
    assert not bad, bad


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_lstm_update_is_gated_by_rows(cuda_device, shape, monkeypatch):
    """Below the probe's constant an LSTM policy on the added ground keeps autograd; a GRU policy is never gated."""
    from rsl_rl_amd import kernels
    H, O, mlp = SHAPES[shape]
    lstm, _ = _update("lstm", cuda_device, H, O, mlp)
    gru, _ = _update("gru", cuda_device, H, O, mlp)
    assert lstm._recurrent_fused_ok() and gru._recurrent_fused_ok()  # the gate is open in this module
    monkeypatch.setattr(kernels, "RNN_H512_LSTM_UPDATE_MIN_ROWS", 4096)
    assert not lstm._recurrent_fused_ok() and gru._recurrent_fused_ok()
    monkeypatch.setattr(kernels, "RNN_H512_LSTM_UPDATE_MIN_ROWS", 64)
    assert lstm._recurrent_fused_ok()
    # what was fused before stays so at every row count: hidden 256 in front of fused stacks
    monkeypatch.setattr(kernels, "RNN_H512_LSTM_UPDATE_MIN_ROWS", 4096)
    old, _ = _update("lstm", cuda_device, 256, 48, [64, 64])
    assert old._recurrent_fused_ok()


@pytest.mark.parametrize("kind", KINDS)
def test_update_reads_the_device_back_once(cuda_device, kind, monkeypatch):
    """One update() under torch's sync debug mode: any synchronising call raises, except the one sanctioned read-back
    (the statistics at the end); every parameter's gradient is a view of the one arena."""
    H, O, mlp = SHAPES["h512-obs45-wide"]
    alg, pol = _update(kind, cuda_device, H, O, mlp)
    alg.update()  # warm-up: allocations, the arena
    alg, pol = _update(kind, cuda_device, H, O, mlp)
    calls = _count(monkeypatch, kind)
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
    assert len(calls) == 4  # the update under watch ran on the fused kernels
    assert len(reads) == 1, reads
    assert all(np.isfinite(v) for v in loss.values())
    arena = alg.grad_arena()
    lo, hi = arena.flat.data_ptr(), arena.flat.data_ptr() + 4 * arena.numel
    for name, p in pol.named_parameters():
        assert p.grad is not None and lo <= p.grad.data_ptr() and p.grad.data_ptr() + 4 * p.numel() <= hi, name
        assert p.grad.data_ptr() == arena.slot(p).data_ptr(), name


def _runner(kind, dev):
    from rsl_rl_amd.env import SyntheticVecEnv
    from rsl_rl_amd.runners import OnPolicyRunner
    torch.manual_seed(1)
    env = SyntheticVecEnv(256, 45, 4, device=dev, seed=0)
    cfg = {"num_steps_per_env": 8, "save_interval": 100, "obs_groups": {"policy": ["policy"]},
           "policy": {"class_name": "ActorCriticRecurrent", "actor_hidden_dims": [512, 256, 128],
                      "critic_hidden_dims": [512, 256, 128], "rnn_type": kind, "rnn_hidden_dim": 512,
                      "rnn_num_layers": 1},
           "algorithm": {"class_name": "PPO", "num_learning_epochs": 2, "num_mini_batches": 2}}
    return OnPolicyRunner(env, cfg, log_dir=None, device="cuda:0")


@pytest.mark.parametrize("kind", KINDS)
def test_runner_end_to_end(cuda_device, tmp_path, kind, monkeypatch):
    from rsl_rl_amd import kernels
    calls = _count(monkeypatch, kind)
    steps = []
    inner = getattr(kernels, f"{kind}_cell_pair")
    monkeypatch.setattr(kernels, f"{kind}_cell_pair", lambda *a, **k: (steps.append(1), inner(*a, **k))[1])
    runner = _runner(kind, cuda_device)
    runner.learn(2)
    assert runner.alg._recurrent_fused_ok()
    assert len(calls) == 2 * 32  # per iteration 2 epochs x 2 mini-batches x 8 steps = 32, E = 128
    assert len(steps) >= 2 * 8  # the rollout took the fused cell: both memories' step in one pair launch per env step
    pol = runner.alg.policy
    with torch.inference_mode():
        x = torch.zeros(256, 45, device=cuda_device)
        assert pol.memory_a.fused_cell(x) is kernels.cell_of(pol.memory_a.rnn) is not None
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


KNOB_SCRIPT = """
import sys
sys.path.insert(0, {root!r})
sys.path.insert(0, {tests!r})
import numpy as np
import torch
from rsl_rl_amd import _lib, kernels
import test_gpu_recurrent_h512 as T

assert not kernels._RNN_HIDDEN_512
L = _lib.lib()
fused = []
for kind in ("lstm", "gru"):
    for name in ("cell_h", "cell_pair_h", "cell_train_pair_h", "cell_bwd_pair_h", "cell_pair", "cell_pair_anyd",
                 "cell_train_pair", "cell_train_pair_anyd", "cell_bwd_pair"):
        entry = f"rslrl_{{kind}}_{{name}}"
        real = getattr(L, entry)
        setattr(L, entry, lambda *a, _r=real, _e=entry: (fused.append(_e), _r(*a))[1])
for kind in ("lstm", "gru"):
    runner = T._runner(kind, torch.device("cuda:0"))
    assert not runner.alg.policy.memory_a.fused_cell(torch.zeros(256, 45, device="cuda:0"))
    runner.learn(1)
    assert not runner.alg._recurrent_fused_ok()
    losses = runner.last_iteration_stats["loss_dict"]
    assert all(np.isfinite(v) for v in losses.values()), losses
assert not fused, fused
print("knob ok")
"""


def test_knob_keeps_the_rnn_library_and_autograd(cuda_device):
    """RSLRL_RNN_HIDDEN_512=0 in a fresh interpreter: no fused launch of either kind, the update runs on autograd."""
    env = dict(os.environ, RSLRL_RNN_HIDDEN_512="0")
    script = KNOB_SCRIPT.format(root=ROOT, tests=os.path.join(ROOT, "tests"))
    out = subprocess.run([sys.executable, "-c", script], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "knob ok" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]
