"""PPO with a wide actor / critic (hidden [320, 260, 64]: DESIGN.md §20) on the manual update path: the reference's
update (tests/golden/make_golden_wide.py) through update_fixtures.check_update unchanged -- max(hidden) >= 256, so the
parameters are held to the fixture's own one-ulp sensitivity bound --, the same fixture with RSLRL_WIDE_MLP=0 in a fresh
process (the knob is read at import), two training iterations through OnPolicyRunner, and the rollout's act() replayed as
a captured graph against the eager step."""

import contextlib
import io
import json
import math
import os
import subprocess
import sys

import pytest
import torch

import wide_fixtures as WF
from update_fixtures import check_update

pytestmark = pytest.mark.gpu

HIDDEN = [320, 260, 64]


def test_update_matches_reference_on_the_manual_path(cuda_device, monkeypatch):
    from rsl_rl_amd.algorithms import PPO
    from rsl_rl_amd.networks import fused_mlp

    z, meta = WF.load()
    calls = {"manual": 0, "autograd": 0, "backward": 0}
    for name, key in (("_manual_minibatch", "manual"), ("_autograd_minibatch", "autograd"),
                      ("_autograd_backward", "backward")):
        def spy(self, *a, _orig=getattr(PPO, name), _key=key, **k):
            calls[_key] += 1
            return _orig(self, *a, **k)
        monkeypatch.setattr(PPO, name, spy)
    before = fused_mlp.wide_launches
    out, alg = WF.run_update(z, meta, cuda_device)
    assert alg.policy.actor._wide and alg.policy.critic._wide and alg.policy.manual_update_structure_ok()
    assert fused_mlp.wide_launches > before
    # every mini-batch on _manual_minibatch: no autograd graph is built, nothing is pushed through one
    assert calls == {"manual": meta["E"] * meta["M"], "autograd": 0, "backward": 0}, calls
    check_update(out, z, meta, 0, mode="wide")


CHILD = """
import json, sys
import conftest  # puts the repository on sys.path
import torch
import wide_fixtures as WF
from update_fixtures import check_update
from rsl_rl_amd.networks import fused_mlp
z, meta = WF.load()
out, alg = WF.run_update(z, meta, torch.device("cuda:0"))
check_update(out, z, meta, 0, mode="knob off")
print("RESULT " + json.dumps({"wide_launches": fused_mlp.wide_launches, "wide": bool(alg.policy.actor._wide),
                             "manual": bool(alg.policy.manual_update_structure_ok())}))
"""


def test_knob_off_keeps_the_layer_by_layer_path(cuda_device):
    env = dict(os.environ, RSLRL_WIDE_MLP="0")
    here = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, "-c", CHILD], cwd=here, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1]
    assert json.loads(line[7:]) == {"wide_launches": 0, "wide": False, "manual": False}


def _cfg():
    return {"num_steps_per_env": 8, "save_interval": 10**9, "obs_groups": {"policy": ["policy"], "critic": ["policy"]},
            "policy": {"class_name": "ActorCritic", "activation": "elu", "actor_hidden_dims": HIDDEN,
                       "critic_hidden_dims": HIDDEN, "init_noise_std": 1.0},
            "algorithm": {"class_name": "PPO", "num_learning_epochs": 2, "num_mini_batches": 2}}


def test_runner_learns_two_iterations(cuda_device):
    from rsl_rl_amd.env import SyntheticVecEnv
    from rsl_rl_amd.networks import fused_mlp
    from rsl_rl_amd.runners import OnPolicyRunner

    torch.manual_seed(1)
    env = SyntheticVecEnv(256, 16, 4, device=cuda_device, seed=0)
    before = fused_mlp.wide_launches
    with contextlib.redirect_stdout(io.StringIO()):
        runner = OnPolicyRunner(env, _cfg(), log_dir=None, device=str(cuda_device))
        runner.learn(2)
    losses = runner.last_iteration_stats["loss_dict"]
    assert all(math.isfinite(v) for v in losses.values()), losses
    assert fused_mlp.wide_launches > before
    assert all(torch.isfinite(p).all() for p in runner.alg.policy.parameters())


def _symmetric_iteration(dev, wide):
    """One OnPolicyRunner iteration (one epoch, one mini-batch: a single symmetric step) with a symmetry_cfg on
    [320, 260, 64]; wide=False sends the two MLPs layer by layer, as RSLRL_WIDE_MLP=0 would.  Returns (the gradients
    the step left in .grad, the loss dict, wide launches during the update)."""
    import numpy as np

    from rsl_rl_amd.algorithms import PPO
    from rsl_rl_amd.env import SyntheticVecEnv
    from rsl_rl_amd.modules.symmetry import SignedPermutationSymmetry
    from rsl_rl_amd.networks import fused_mlp
    from rsl_rl_amd.runners import OnPolicyRunner

    rng = np.random.default_rng(11)

    def maps(width):
        return [(np.arange(width), np.ones(width, np.float32)),
                (rng.permutation(width), rng.choice(np.array([-1.0, 1.0], np.float32), width))]

    cfg = _cfg()
    cfg["algorithm"].update(num_learning_epochs=1, num_mini_batches=1, symmetry_cfg={
        "use_data_augmentation": True, "use_mirror_loss": True, "mirror_loss_coeff": 0.5,
        "data_augmentation_func": SignedPermutationSymmetry({"policy": maps(16)}, maps(4))})
    torch.manual_seed(1)
    torch.cuda.manual_seed(1)
    env = SyntheticVecEnv(256, 16, 4, device=dev, seed=0)
    launches = []
    update = PPO.update

    def counted(self):
        before = fused_mlp.wide_launches
        try:
            return update(self)
        finally:
            launches.append(fused_mlp.wide_launches - before)

    with contextlib.redirect_stdout(io.StringIO()):
        runner = OnPolicyRunner(env, cfg, log_dir=None, device=str(dev))
        pol = runner.alg.policy
        assert pol.actor._wide and pol.critic._wide
        pol.actor._wide = pol.critic._wide = wide
        PPO.update = counted
        try:
            runner.learn(1)
        finally:
            PPO.update = update
    grads = {k: p.grad.clone() for k, p in pol.named_parameters()}
    return grads, runner.last_iteration_stats["loss_dict"], launches[0]


def test_symmetric_update_runs_the_wide_kernels_under_autograd(cuda_device, monkeypatch):
    """With a symmetry_cfg a wide policy keeps the autograd strategy (PPO._choose_strategy), and under autograd a wide
    MLP's forward and backward are FusedMLPFunction's, on the wide kernels: the same step with the two MLPs sent layer
    by layer gives the same losses and gradients.  Bound: 1e-4 of a tensor's largest entry -- ten times the bound the
    stack test holds one forward or one backward to (test_gpu_wide_mlp.py, 1e-5; 2e-5 for a bias), for the three passes
    composed (forward, the loss kernel's gradient of those outputs, backward) and the loss' second derivative, which
    at the first step of an update (ratio 1, nothing clipped, noise std 1) is smooth and of order one."""
    from rsl_rl_amd.algorithms import PPO

    calls = {"manual": 0, "backward": 0}
    for name, key in (("_manual_minibatch", "manual"), ("_autograd_backward", "backward")):
        def spy(self, *a, _orig=getattr(PPO, name), _key=key, **k):
            calls[_key] += 1
            return _orig(self, *a, **k)
        monkeypatch.setattr(PPO, name, spy)
    g_wide, loss_wide, n_wide = _symmetric_iteration(cuda_device, True)
    assert calls == {"manual": 0, "backward": 1}, calls
    # three wide layers per network, forward and input gradient or weight gradient each: at least 6 + 6 launches
    assert n_wide >= 12, n_wide
    g_ref, loss_ref, n_ref = _symmetric_iteration(cuda_device, False)
    assert n_ref == 0 and calls == {"manual": 0, "backward": 2}, (n_ref, calls)
    assert loss_wide.keys() == loss_ref.keys() and "symmetry" in loss_wide and loss_wide["symmetry"] > 0
    for k, v in loss_ref.items():
        print(k, loss_wide[k], v)
        assert math.isfinite(v) and abs(loss_wide[k] - v) <= 1e-4 * max(abs(v), 1.0), (k, loss_wide[k], v)
    for k, ref in g_ref.items():
        err, top = (g_wide[k] - ref).abs().max().item(), ref.abs().max().item()
        print(k, err, top)
        assert err <= 1e-4 * top + 1e-12, (k, err, top)


def test_graph_replayed_act_is_the_eager_act(cuda_device):
    """The rollout's per-layer wide launches under modules/act_graph.py's capture: the same observations and the same
    noise give the eager step's actions, values and mean bit for bit."""
    from rsl_rl_amd.modules import ActorCritic
    from rsl_rl_amd.modules.act_graph import RolloutActGraph
    from rsl_rl_amd.networks import fused_mlp

    torch.manual_seed(0)
    dev = cuda_device
    N = fused_mlp.WIDE_FWD_MIN_ROWS  # the rollout's forward takes the wide kernels from this many envs on
    pol = ActorCritic({"policy": torch.zeros(N, 16, device=dev)}, {"policy": ["policy"], "critic": ["policy"]}, 4,
                      actor_hidden_dims=HIDDEN, critic_hidden_dims=HIDDEN).to(dev)
    g = RolloutActGraph(pol)
    gen = torch.Generator(device=dev).manual_seed(1)
    replayed = 0
    before = fused_mlp.wide_launches
    with torch.inference_mode(), fused_mlp.frozen_weights():
        for step in range(6):
            x = torch.randn(N, 16, device=dev, generator=gen)
            torch.cuda.manual_seed(100 + step)
            res = g({"policy": x})
            replayed += res is not None
            if res is None:
                res = pol.act_and_evaluate({"policy": x})
            a, v, mu = res[0].clone(), res[1].clone(), pol.action_mean.clone()
            torch.cuda.manual_seed(100 + step)
            a_ref, v_ref = pol.act_and_evaluate({"policy": x.clone()})
            assert torch.equal(a, a_ref) and torch.equal(v, v_ref) and torch.equal(mu, pol.action_mean), step
    assert g._graph is not None and replayed >= 4, "the wide step was not captured"
    assert fused_mlp.wide_launches >= before + 6 * 6  # three wide layers per network in every eager step
