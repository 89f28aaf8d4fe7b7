"""A ragged stack (an observation width that is no multiple of 4) through the layers above the kernels:
the reference's PPO update (tests/golden/make_golden_ragged.py) through update_fixtures.check_update unchanged, on the
manual path and, with RSLRL_RAGGED_INPUT=0 in a fresh process, on the old one; FusedMLPFunction against the zero-padded
stack bit for bit; the runner at the rough-terrain shape (obs 235, [512, 256, 128]); the rollout's act() replayed as a
captured graph; one symmetric and one distillation step under autograd."""

import contextlib
import io
import json
import math
import os
import subprocess
import sys

import pytest
import torch
import torch.nn as nn

import ragged_fixtures as RF
from update_fixtures import check_update
from rsl_rl_amd.networks import MLP, fused_mlp

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", RF.CASES)
def test_update_matches_reference_on_the_manual_path(case, cuda_device, monkeypatch):
    from rsl_rl_amd.algorithms import PPO

    z, meta = RF.load(case)
    calls = {"manual": 0, "autograd": 0, "backward": 0}
    for name, key in (("_manual_minibatch", "manual"), ("_autograd_minibatch", "autograd"),
                      ("_autograd_backward", "backward")):
        def spy(self, *a, _orig=getattr(PPO, name), _key=key, **k):
            calls[_key] += 1
            return _orig(self, *a, **k)
        monkeypatch.setattr(PPO, name, spy)
    pads = []
    fpad = torch.nn.functional.pad
    monkeypatch.setattr(fused_mlp.F, "pad", lambda t, *a, **k: (pads.append(tuple(t.shape)), fpad(t, *a, **k))[1])
    before, copies = fused_mlp.ragged_launches, fused_mlp.ragged_realign_copies
    out, alg = RF.run_update(z, meta, cuda_device)
    pol = alg.policy
    assert pol.actor._ragged and pol.critic._ragged and not pol.manual_update_structure_ok()
    assert pol.ragged_update_structure_ok()
    assert fused_mlp.ragged_launches > before
    assert calls == {"manual": meta["E"] * meta["M"], "autograd": 0, "backward": 0}, calls
    # no pad copy and no re-aligning copy of the observation batch
    assert not [s for s in pads if len(s) == 2 and s[1] == meta["O"]], pads
    assert fused_mlp.ragged_realign_copies == copies
    check_update(out, z, meta, 0, mode=case)


CHILD = """
import json, sys
import conftest  # puts the repository on sys.path
import torch
import ragged_fixtures as RF
from update_fixtures import check_update
from rsl_rl_amd.networks import fused_mlp
z, meta = RF.load(sys.argv[1])
out, alg = RF.run_update(z, meta, torch.device("cuda:0"))
check_update(out, z, meta, 0, mode="knob off")
pol = alg.policy
print("RESULT " + json.dumps({"ragged_launches": fused_mlp.ragged_launches, "ragged": bool(pol.actor._ragged),
                             "manual": bool(pol.manual_update_ok({"policy": torch.zeros(4, meta["O"], device="cuda:0")}))}))
"""


@pytest.mark.parametrize("case", RF.CASES)
def test_knob_off_keeps_the_old_path(case, cuda_device):
    env = dict(os.environ, RSLRL_RAGGED_INPUT="0")
    here = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, "-c", CHILD, case], cwd=here, env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1]
    assert json.loads(line[7:]) == {"ragged_launches": 0, "ragged": False, "manual": False}


# (50, [256]): the ragged first layer is also the last hidden one -- the ragged kernel, then the output layer by torch
STACKS = ((77, [320, 260, 64], 4), (19, [64, 64], 4), (235, [512, 256, 128], 12), (50, [256, 256], 12), (50, [256], 12))


def _padded_copy(mlp, k0):
    """The same stack with the input width rounded up to 4 and zero weight columns there."""
    pad = (-k0) % 4
    hidden = [m.out_features for m in mlp if isinstance(m, nn.Linear)]
    big = MLP(k0 + pad, hidden[-1], hidden[:-1]).to(mlp[0].weight.device)
    with torch.no_grad():
        for a, b in zip((m for m in big if isinstance(m, nn.Linear)), (m for m in mlp if isinstance(m, nn.Linear))):
            a.weight.zero_()
            a.weight[:, :b.in_features].copy_(b.weight)
            a.bias.copy_(b.bias)
    return big


@pytest.mark.parametrize("k0,hidden,nout", STACKS)
@pytest.mark.parametrize("M", [200, 1024])
def test_function_equals_padded_stack(k0, hidden, nout, M, cuda_device):
    torch.manual_seed(k0 + M)
    mlp = MLP(k0, nout, hidden).to(cuda_device)
    assert mlp._ragged and not mlp._fused and not mlp._wide
    big = _padded_copy(mlp, k0)
    assert big._fused or big._wide
    x = torch.randn(M, k0, device=cuda_device)
    xp = torch.nn.functional.pad(x, (0, (-k0) % 4))
    g = torch.randn(M, nout, device=cuda_device)
    before = fused_mlp.ragged_launches
    pads = []
    orig = torch.nn.functional.pad
    fused_mlp.F.pad = lambda t, *a, **k: (pads.append(tuple(t.shape)), orig(t, *a, **k))[1]
    try:
        y = mlp(x)
        y.backward(g)
    finally:
        fused_mlp.F.pad = orig
    assert fused_mlp.ragged_launches > before
    assert not [s for s in pads if s[1] == k0], pads  # no pad copy of the observation batch
    # a single hidden layer: the ragged stack applies its output layer with torch (the fused output layer has no ragged
    # form), and the fused output-layer kernel forms the hidden activation as C^T tiles, a different product order; so
    # the oracle is the padded stack with its output layer unfused too (RSLRL_FUSE_OUT_FWD=0's flag) -- the same
    # FWD_ELU kernel on the padded problem, then torch: the same bits again
    prev = fused_mlp._FUSE_OUT_FWD
    fused_mlp._FUSE_OUT_FWD = prev and len(hidden) > 1
    try:
        yp = big(xp)
        yp.backward(g)
    finally:
        fused_mlp._FUSE_OUT_FWD = prev
    assert torch.equal(y, yp)
    for (name, p), (_, q) in zip(mlp.named_parameters(), big.named_parameters()):
        ref = q.grad[:, :k0] if name == "0.weight" else q.grad
        assert torch.equal(p.grad, ref), (name, (p.grad - ref).abs().max().item())
    # the inference forward (the rollout's) at these row counts stays layer by layer (RAGGED_FWD_MIN_ROWS /
    # WIDE_FWD_MIN_ROWS): close, no ragged launch
    with torch.no_grad():
        before = fused_mlp.ragged_launches
        y_inf = mlp(x)
        assert M < min(fused_mlp.RAGGED_FWD_MIN_ROWS, fused_mlp.WIDE_FWD_MIN_ROWS) and fused_mlp.ragged_launches == before
        assert (y_inf - y).abs().max().item() <= 1e-5 * y.abs().max().item()


@pytest.mark.parametrize("k0,hidden,nout", [(19, [64, 64], 4), (50, [256, 256], 12), (235, [512, 256, 128], 12)])
def test_inference_forward_takes_the_ragged_kernel_from_its_threshold(k0, hidden, nout, cuda_device):
    """A forward nothing differentiates: from RAGGED_FWD_MIN_ROWS rows (WIDE_FWD_MIN_ROWS for a stack with wide layers)
    on the first layer runs on the ragged kernel, and gives the bits of the forward under autograd; one 128-row tile
    below, it stays layer by layer."""
    torch.manual_seed(k0)
    mlp = MLP(k0, nout, hidden).to(cuda_device)
    rows = fused_mlp.WIDE_FWD_MIN_ROWS if fused_mlp.ragged_wide_stack(mlp) else fused_mlp.RAGGED_FWD_MIN_ROWS
    x = torch.randn(rows, k0, device=cuda_device)
    y = mlp(x).detach()
    with torch.no_grad():
        before = fused_mlp.ragged_launches
        assert torch.equal(mlp(x), y) and fused_mlp.ragged_launches == before + 1
        below = mlp(x[:rows - 128])
        assert fused_mlp.ragged_launches == before + 1
        assert (below - y[:rows - 128]).abs().max().item() <= 1e-5 * y.abs().max().item()


def _runner(obs, hidden, envs, device, **alg):
    from rsl_rl_amd.env import SyntheticVecEnv
    from rsl_rl_amd.runners import OnPolicyRunner

    env = SyntheticVecEnv(envs, obs, 12, device=device, seed=0)
    cfg = {"num_steps_per_env": 8, "save_interval": 100, "obs_groups": {"policy": ["policy"]},
           "policy": {"class_name": "ActorCritic", "actor_hidden_dims": hidden, "critic_hidden_dims": hidden},
           "algorithm": dict({"class_name": "PPO", "num_learning_epochs": 2, "num_mini_batches": 2}, **alg)}
    return OnPolicyRunner(env, cfg, log_dir=None, device=str(device))


@pytest.mark.parametrize("obs,hidden", [(235, [512, 256, 128]), (19, [256, 256])])
def test_runner_learns_on_the_manual_strategy(obs, hidden, cuda_device, monkeypatch):
    import numpy as np

    from rsl_rl_amd.algorithms import PPO

    torch.manual_seed(3)
    runner = _runner(obs, hidden, 256, cuda_device)
    pol = runner.alg.policy
    assert pol.actor._ragged and pol.critic._ragged and not pol.manual_update_structure_ok()
    taken = []
    orig = PPO._manual_minibatch
    monkeypatch.setattr(PPO, "_manual_minibatch", lambda self, u, mb: (taken.append(1), orig(self, u, mb))[1])
    pads = []
    fpad = torch.nn.functional.pad
    monkeypatch.setattr(fused_mlp.F, "pad", lambda t, *a, **k: (pads.append(tuple(t.shape)), fpad(t, *a, **k))[1])
    before = fused_mlp.ragged_launches
    runner.learn(2)
    losses = runner.last_iteration_stats["loss_dict"]
    assert all(np.isfinite(v) for v in losses.values()), losses
    assert len(taken) == 2 * 2 * 2, len(taken)  # every mini-batch of both iterations on _manual_minibatch
    assert fused_mlp.ragged_launches > before
    assert not [s for s in pads if len(s) == 2 and s[1] == obs], pads


@pytest.mark.parametrize("obs,hidden,N", [(19, [256, 256], fused_mlp.RAGGED_FWD_MIN_ROWS),
                                          (235, [512, 256, 128], fused_mlp.WIDE_FWD_MIN_ROWS)])
def test_graph_replayed_act_is_the_eager_act(obs, hidden, N, cuda_device):
    """The rollout's ragged first-layer launches under modules/act_graph.py's capture: the same observations and the
    same noise give the eager step's actions, values and mean bit for bit.  The narrow stack takes the ragged forward from
    RAGGED_FWD_MIN_ROWS envs on, the one with wide layers from WIDE_FWD_MIN_ROWS."""
    from rsl_rl_amd.modules import ActorCritic
    from rsl_rl_amd.modules.act_graph import RolloutActGraph

    torch.manual_seed(0)
    dev = cuda_device
    pol = ActorCritic({"policy": torch.zeros(N, obs, device=dev)}, {"policy": ["policy"], "critic": ["policy"]}, 4,
                      actor_hidden_dims=hidden, critic_hidden_dims=hidden).to(dev)
    assert pol.actor._ragged and pol.critic._ragged
    g = RolloutActGraph(pol)
    gen = torch.Generator(device=dev).manual_seed(1)
    replayed, eager_launches = 0, 0
    start = fused_mlp.ragged_launches
    with torch.inference_mode(), fused_mlp.frozen_weights():
        for step in range(6):
            x = torch.randn(N, obs, device=dev, generator=gen)
            torch.cuda.manual_seed(100 + step)
            res = g({"policy": x})
            replayed += res is not None
            if res is None:
                res = pol.act_and_evaluate({"policy": x})
            a, v, mu = res[0].clone(), res[1].clone(), pol.action_mean.clone()
            torch.cuda.manual_seed(100 + step)
            before = fused_mlp.ragged_launches
            a_ref, v_ref = pol.act_and_evaluate({"policy": x.clone()})
            eager_launches += fused_mlp.ragged_launches - before
            assert torch.equal(a, a_ref) and torch.equal(v, v_ref) and torch.equal(mu, pol.action_mean), step
    assert g._graph is not None and replayed >= 4, "the ragged step was not captured"
    assert eager_launches == 6 * 2  # one ragged first layer per network in every eager step
    # ... and the capture itself (and the un-replayed steps before it) issued ragged launches of its own
    assert fused_mlp.ragged_launches > start + eager_launches


def _symmetric_iteration(dev, ragged):
    """One OnPolicyRunner iteration (one epoch, one mini-batch: a single symmetric step) with a symmetry_cfg at obs 19,
    hidden [256, 256]; ragged=False sends the two MLPs layer by layer, as RSLRL_RAGGED_INPUT=0 would."""
    import numpy as np

    from rsl_rl_amd.algorithms import PPO
    from rsl_rl_amd.env import SyntheticVecEnv
    from rsl_rl_amd.modules.symmetry import SignedPermutationSymmetry
    from rsl_rl_amd.runners import OnPolicyRunner

    rng = np.random.default_rng(11)

    def maps(width):
        return [(np.arange(width), np.ones(width, np.float32)),
                (rng.permutation(width), rng.choice(np.array([-1.0, 1.0], np.float32), width))]

    cfg = {"num_steps_per_env": 8, "save_interval": 10**9, "obs_groups": {"policy": ["policy"], "critic": ["policy"]},
           "policy": {"class_name": "ActorCritic", "activation": "elu", "actor_hidden_dims": [256, 256],
                      "critic_hidden_dims": [256, 256], "init_noise_std": 1.0},
           "algorithm": {"class_name": "PPO", "num_learning_epochs": 1, "num_mini_batches": 1, "symmetry_cfg": {
               "use_data_augmentation": True, "use_mirror_loss": True, "mirror_loss_coeff": 0.5,
               "data_augmentation_func": SignedPermutationSymmetry({"policy": maps(19)}, maps(4))}}}
    torch.manual_seed(1)
    torch.cuda.manual_seed(1)
    env = SyntheticVecEnv(256, 19, 4, device=dev, seed=0)
    launches = []
    update = PPO.update

    def counted(self):
        before = fused_mlp.ragged_launches
        try:
            return update(self)
        finally:
            launches.append(fused_mlp.ragged_launches - before)

    with contextlib.redirect_stdout(io.StringIO()):
        runner = OnPolicyRunner(env, cfg, log_dir=None, device=str(dev))
        pol = runner.alg.policy
        assert pol.actor._ragged and pol.critic._ragged
        pol.actor._ragged = pol.critic._ragged = ragged
        PPO.update = counted
        try:
            runner.learn(1)
        finally:
            PPO.update = update
    grads = {k: p.grad.clone() for k, p in pol.named_parameters()}
    return grads, runner.last_iteration_stats["loss_dict"], launches[0]


def test_symmetric_update_runs_the_ragged_kernels_under_autograd(cuda_device, monkeypatch):
    """With a symmetry_cfg a ragged policy keeps the autograd strategy, and under autograd its forward and backward are
    FusedMLPFunction's with the ragged first layer: the same step with the two MLPs sent layer by layer gives the same
    losses and gradients.  Bound: 1e-4 of a tensor's largest entry, the bound and the reasoning of
    tests/test_gpu_wide_update.py's symmetric test (three composed passes, each held to 1e-5 / 2e-5 alone)."""
    from rsl_rl_amd.algorithms import PPO

    calls = {"manual": 0, "backward": 0}
    for name, key in (("_manual_minibatch", "manual"), ("_autograd_backward", "backward")):
        def spy(self, *a, _orig=getattr(PPO, name), _key=key, **k):
            calls[_key] += 1
            return _orig(self, *a, **k)
        monkeypatch.setattr(PPO, name, spy)
    g_rag, loss_rag, n_rag = _symmetric_iteration(cuda_device, True)
    assert calls == {"manual": 0, "backward": 1}, calls
    assert n_rag >= 4, n_rag  # forward and weight gradient of the first layer of both networks
    g_ref, loss_ref, n_ref = _symmetric_iteration(cuda_device, False)
    assert n_ref == 0 and calls == {"manual": 0, "backward": 2}, (n_ref, calls)
    assert loss_rag.keys() == loss_ref.keys() and "symmetry" in loss_rag
    for k, v in loss_ref.items():
        print(k, loss_rag[k], v)
        assert math.isfinite(v) and abs(loss_rag[k] - v) <= 1e-4 * max(abs(v), 1.0), (k, loss_rag[k], v)
    for k, ref in g_ref.items():
        err, top = (g_rag[k] - ref).abs().max().item(), ref.abs().max().item()
        print(k, err, top)
        assert err <= 1e-4 * top + 1e-12, (k, err, top)


def test_distillation_step_runs_the_ragged_kernels_under_autograd(cuda_device):
    """A student with a ragged observation (19 wide): Distillation keeps its per-step autograd strategy for it (its
    fused predicate reads MLP._fused), and one behaviour-cloning step -- act_inference under autograd, the project's BC
    loss, backward -- runs the student's first layer on the ragged kernels.  The same step with the student sent layer
    by layer gives the same loss and gradients, to the 1e-5 / 2e-5 (bias) bound one forward + backward of a stack is
    held to in tests/test_gpu_fused_mlp.py."""
    from rsl_rl_amd import kernels
    from rsl_rl_amd.modules import StudentTeacher

    torch.manual_seed(5)
    dev = cuda_device
    obs = {"policy": torch.randn(256, 19, device=dev), "teacher": torch.randn(256, 48, device=dev)}
    pol = StudentTeacher(obs, {"policy": ["policy"], "teacher": ["teacher"]}, 12).to(dev)
    assert pol.student._ragged and not pol.student._fused
    # (Distillation._fused_common asks for student._fused and fused_mlp.fusable(student, .): both false here)
    assert not fused_mlp.fusable(pol.student, obs["policy"])

    def step(ragged):
        pol.student._ragged = ragged
        pol.zero_grad(set_to_none=True)
        before = fused_mlp.ragged_launches
        with torch.no_grad():
            target = pol.evaluate(obs)
        loss = kernels.BCLossFunction.apply(pol.act_inference(obs), target, "mse")
        loss.backward()
        return loss.item(), {k: p.grad.clone() for k, p in pol.student.named_parameters()}, \
            fused_mlp.ragged_launches - before

    try:
        loss_r, g_r, n_r = step(True)
        loss_l, g_l, n_l = step(False)
    finally:
        pol.student._ragged = True
    assert n_r >= 2 and n_l == 0, (n_r, n_l)
    assert math.isfinite(loss_l) and abs(loss_r - loss_l) <= 1e-5 * abs(loss_l)
    for k, ref in g_l.items():
        err, top = (g_r[k] - ref).abs().max().item(), ref.abs().max().item()
        assert err <= (2e-5 if "bias" in k else 1e-5) * top + 1e-12, (k, err, top)
