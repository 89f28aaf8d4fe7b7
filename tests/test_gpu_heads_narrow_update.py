"""One PPO.update() with the narrow heads (a last hidden layer of 256 -> 128) on the smallest policy shapes --
256 envs, T = 8, 2 mini-batches (1,024 rows each), 1 epoch:

* [512, 256, 128] (a wide stack: one pass per network, the heads offered there by ActorCritic.train_forward_rows) at
  obs 48 and at obs 45 (a ragged first layer),
* [256, 256, 128] (the paired pass) at obs 48 and obs 45,
* ActorCriticRecurrent with a GRU of 256 in front of [256, 256, 128] (the recurrent update goes through
  train_forward_rows too).

RSLRL_HEAD_NARROW is read at import, so each knob value runs in a fresh child process (one child for all five shapes).
With the knob on, fused_mlp.actor_head_launches advances by mini-batches x epochs; with RSLRL_HEAD_NARROW=0 it does not.
Parameters, the loss means and the learning rate agree between the two within the bound tests/test_gpu_wide_update.py
holds its two paths to (1e-4 of a tensor's largest entry; the learning rate exactly).

The comparison is of parameters after Adam, whose first steps move an element by lr g / (|g| + 1e-8): among 131,072
entries of a 256 x 512 weight a few have |g| near 1e-8, and there the last bits of the gradient are a visible part of
a step.  So the bound holds only where the gradients behind the last hidden layer
are the same bits with and without the heads, and the narrow heads are built that way: the critic's dz is one fp32
product either way, and the actor's narrow head forms dz with linear_dgrad_elu_wgrad's fp32 FMA chain (csrc/mlp_heads.hip).
What still differs is the two output layers' [dW | db] (another summation order): 1,536 and 128 entries whose gradients
are nowhere near 1e-8.  (A head whose dz came from x6 MFMA products missed the bound at [512, 256, 128].)

The reference fixtures of the wide and ragged stacks (tests/golden/golden_wide.json, golden_ragged.json) still pass
check_update with the knob on; their last hidden layers are 260 -> 64 and 64 -> 64, so what they exercise is the decline
path (K != 256: no head launch, the critic-first order of the single passes), and the tests assert that.  And the route
on which a tape with a head reaches fused_mlp.train_backward from a paired forward is driven once per head width."""

import json
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

CASES = ["wide_48", "wide_45", "pair_48", "pair_45", "gru"]
EPOCHS, MINI_BATCHES = 1, 2

CHILD = r"""
import json, sys
import conftest  # puts the repository on sys.path
import numpy as np
import torch
import recurrent_fixtures as RF
from rsl_rl_amd.algorithms import PPO
from rsl_rl_amd.modules import ActorCritic, ActorCriticRecurrent
from rsl_rl_amd.networks import fused_mlp

dev = torch.device("cuda:0")
T, N, A, E, M = 8, 256, 12, %d, %d
GROUPS = {"policy": ["policy"], "critic": ["policy"]}


def stored_fields(rng, noise):
    # the fields an older policy left behind: its mean a little off this one's (near 0 at initialisation), std 1, the
    # log-prob of the actions it drew -- ratios on both sides of the clip
    mu = (0.15 * rng.standard_normal((T, N, A))).astype(np.float32)
    logp = (-0.5 * noise.astype(np.float64) ** 2 - 0.5 * np.log(2 * np.pi)).sum(-1, keepdims=True).astype(np.float32)
    values = (0.3 * rng.standard_normal((T, N, 1))).astype(np.float32)
    return mu, logp, values


def feedforward(hidden, O):
    rng = np.random.default_rng(5)
    data = {k: rng.standard_normal(s).astype(np.float32) for k, s in
            (("obs", (T, N, O)), ("rewards", (T, N, 1)), ("noise", (T, N, A)), ("last", (N, O)))}
    mu, logp, values = stored_fields(rng, data["noise"])
    obs0 = {"policy": torch.zeros(N, O)}
    torch.manual_seed(0)
    pol = ActorCritic(obs0, GROUPS, A, actor_hidden_dims=hidden, critic_hidden_dims=hidden)
    alg = PPO(pol, num_learning_epochs=E, num_mini_batches=M, device=dev, desired_kl=0.01)
    alg.init_storage("rl", N, T, obs0, [A])
    st = alg.storage
    st.observations["policy"].copy_(torch.from_numpy(data["obs"]))
    st.rewards.copy_(torch.from_numpy(data["rewards"]))
    st.values.copy_(torch.from_numpy(values))
    st.actions_log_prob.copy_(torch.from_numpy(logp))
    st.mu.copy_(torch.from_numpy(mu))
    st.sigma.copy_(torch.ones(T, N, A))
    st.actions.copy_(torch.from_numpy(mu + data["noise"]))
    st.dones.zero_()
    st.step = T
    with torch.inference_mode():
        alg.compute_returns({"policy": torch.from_numpy(data["last"]).to(dev)})
    st.perm_generator = torch.Generator().manual_seed(1)
    return alg, pol


def recurrent():
    O, H = 48, 256
    nz = RF.storage_inputs(17, T, N, O, A, 1, H, 1)
    rng = np.random.default_rng(6)
    mu, logp, values = stored_fields(rng, nz["noise"])
    obs0 = {"policy": torch.zeros(N, O)}
    torch.manual_seed(0)
    pol = ActorCriticRecurrent(obs0, GROUPS, A, actor_hidden_dims=[256, 256, 128], critic_hidden_dims=[256, 256, 128],
                               rnn_type="gru", rnn_hidden_dim=H, rnn_num_layers=1)
    alg = PPO(pol, num_learning_epochs=E, num_mini_batches=M, device=dev, desired_kl=0.01)
    alg.init_storage("rl", N, T, obs0, [A])
    RF.fill_storage(alg.storage, nz, {"mu": mu, "sigma": np.ones(A, np.float32), "values": values,
                                      "actions_log_prob": logp}, dev)
    with torch.inference_mode():
        alg.compute_returns({"policy": torch.from_numpy(nz["last_obs"]).to(dev)})
    assert alg._recurrent_fused_ok()
    return alg, pol


BUILD = {"wide_48": lambda: feedforward([512, 256, 128], 48), "wide_45": lambda: feedforward([512, 256, 128], 45),
         "pair_48": lambda: feedforward([256, 256, 128], 48), "pair_45": lambda: feedforward([256, 256, 128], 45),
         "gru": recurrent}
result, tensors = {}, {}
for name, build in BUILD.items():
    alg, pol = build()
    before = fused_mlp.actor_head_launches
    loss = alg.update()
    torch.cuda.synchronize()
    result[name] = {"launches": fused_mlp.actor_head_launches - before, "loss": loss, "lr": alg.learning_rate}
    tensors[name] = {k: v.detach().cpu() for k, v in pol.state_dict().items()}
torch.save(tensors, sys.argv[1])
print("RESULT " + json.dumps({"knob": fused_mlp._HEAD_NARROW, "cases": result}))
""" % (EPOCHS, MINI_BATCHES)


def _child(knob, path):
    env = dict(os.environ, RSLRL_HEAD_NARROW=knob)
    here = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, "-c", CHILD, str(path)], cwd=here, env=env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1]
    return json.loads(line[7:]), torch.load(path)


@pytest.fixture(scope="module")
def runs(cuda_device, tmp_path_factory):
    d = tmp_path_factory.mktemp("heads_narrow")
    return {knob: _child(knob, d / f"params_{knob}.pt") for knob in ("1", "0")}


def test_the_children_read_the_knob(runs):
    assert runs["1"][0]["knob"] is True and runs["0"][0]["knob"] is False


@pytest.mark.parametrize("case", CASES)
def test_actor_head_launches_follow_the_knob(runs, case):
    assert runs["1"][0]["cases"][case]["launches"] == EPOCHS * MINI_BATCHES
    assert runs["0"][0]["cases"][case]["launches"] == 0


@pytest.mark.parametrize("case", CASES)
def test_update_agrees_between_knob_on_and_off(runs, case):
    (on, p_on), (off, p_off) = runs["1"], runs["0"]
    on, off = on["cases"][case], off["cases"][case]
    assert on["lr"] == off["lr"]
    assert on["loss"].keys() == off["loss"].keys()
    for k, v in off["loss"].items():
        print(case, k, on["loss"][k], v)
        assert abs(on["loss"][k] - v) <= 1e-4 * max(abs(v), 1.0), (k, on["loss"][k], v)
    for k, ref in p_off[case].items():
        err, top = (p_on[case][k] - ref).abs().max().item(), ref.abs().max().item()
        print(case, k, err, top)
        assert err <= 1e-4 * top + 1e-12, (k, err, top)


def _declined(monkeypatch):
    """Records what the two head wrappers return during an update: (results list, launches before)."""
    from rsl_rl_amd.networks import fused_mlp

    monkeypatch.setattr(fused_mlp, "_HEAD_NARROW", True)
    results = []
    for name in ("value_head_fwd_bwd", "actor_head_fwd_bwd"):
        def spy(*a, _orig=getattr(fused_mlp, name), **k):
            results.append(_orig(*a, **k))
            return results[-1]
        monkeypatch.setattr(fused_mlp, name, spy)
    return results, fused_mlp.actor_head_launches


def test_wide_reference_fixture_is_declined_by_the_heads(cuda_device, monkeypatch):
    """[320, 260, 64] ends in 260 -> 64: N is a narrow width, K is not 256.  With the knob on no head runs (the wrappers
    decline before they allocate or launch) and the fixture passes check_update as before."""
    import wide_fixtures as WF
    from rsl_rl_amd.networks import fused_mlp
    from update_fixtures import check_update

    results, before = _declined(monkeypatch)
    z, meta = WF.load()
    out, _ = WF.run_update(z, meta, cuda_device)
    assert all(r is None for r in results) and fused_mlp.actor_head_launches == before
    check_update(out, z, meta, 0, mode="wide, narrow heads declined")


@pytest.mark.parametrize("name", ["ragged_wide", "ragged_narrow"])
def test_ragged_reference_fixtures_are_declined_by_the_heads(name, cuda_device, monkeypatch):
    """obs 77 [320, 260, 64] and obs 19 [64, 64]: K = 260 and K = 64, the same decline path."""
    import ragged_fixtures as RG
    from rsl_rl_amd.networks import fused_mlp
    from update_fixtures import check_update

    results, before = _declined(monkeypatch)
    z, meta = RG.load(name)
    out, _ = RG.run_update(z, meta, cuda_device)
    assert all(r is None for r in results) and fused_mlp.actor_head_launches == before
    check_update(out, z, meta, 0, mode=name + ", narrow heads declined")


ROUTE_CHILD = r"""
import json, sys
import conftest  # puts the repository on sys.path
import torch
from rsl_rl_amd.networks import fused_mlp
from update_fixtures import run_recorded_update
exec(open(sys.argv[1]).read().split("# ---- CASES")[0])  # the builders of the update child

hidden = json.loads(sys.argv[2])
out = {}
for route in ("paired", "single"):
    if route == "single":  # the paired backward declines: ActorCritic.train_backward takes the tapes one by one
        fused_mlp.train_backward_pair = lambda *a, **k: False
    alg, pol = feedforward(hidden, 48)
    grads = [None]
    before = fused_mlp.actor_head_launches
    run_recorded_update(alg, grads)
    torch.cuda.synchronize()
    off, o = {}, 0
    for k, p in pol.named_parameters():
        off[k] = (o, o + p.numel())
        o += p.numel()
    out[route] = (grads[0].detach().cpu().double(), off, fused_mlp.actor_head_launches - before)
(g1, off, n1), (g0, _, n0) = out["paired"], out["single"]
rep = {k: [float((g1[a:b] - g0[a:b]).abs().max()), float(g0[a:b].abs().max())] for k, (a, b) in off.items()}
print("RESULT " + json.dumps({"launches": [n1, n0], "tensors": rep}))
"""


@pytest.mark.parametrize("hidden", [[256, 256, 256], [256, 256, 128]])
def test_head_tapes_through_the_unpaired_backward(hidden, cuda_device, tmp_path):
    """A paired forward whose tapes carry heads (256-wide and narrow) where train_backward_pair does not apply:
    ActorCritic.train_backward then hands each tape to fused_mlp.train_backward, which takes dz and the [dW | db]
    partials from the head (before ABI 34 this route raised).  The first mini-batch's pre-clip gradients against the
    paired backward's, at the bound tests/test_gpu_wide_update.py holds two paths' gradients to (1e-4 of a tensor's
    largest entry).  A fresh process: the route is forced by replacing a module function."""
    src = tmp_path / "builders.py"
    src.write_text(CHILD.replace("BUILD = {", "# ---- CASES\nBUILD = {"))
    here = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, "-c", ROUTE_CHILD, str(src), json.dumps(hidden)], cwd=here,
                       env=dict(os.environ, RSLRL_HEAD_NARROW="1"), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    res = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    assert res["launches"] == [EPOCHS * MINI_BATCHES] * 2
    for k, (err, top) in res["tensors"].items():
        print(hidden, k, err, top)
        assert err <= 1e-4 * top + 1e-12, (k, err, top)
