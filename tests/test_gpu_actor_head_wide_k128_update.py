"""One PPO.update() with the actor head for 17 to 32 actions on a last hidden layer with 128 inputs
at the smallest policy shapes -- 256 envs, T = 8, 2 mini-batches (1,024 rows each), 1 epoch, obs 48:

* [128, 128, 128] with 19 actions: the paired pass (the head admits the pair), the head's dz into the 128-wide backward;
* [256, 128, 64] with 24 actions: one backward per network (the 128 -> 64 layer's bias gradient is dz.sum(0)).

RSLRL_ACTOR_HEAD_WIDE_K128 is read at import, so each knob value runs in a fresh child process (one child for both
stacks).  fused_mlp.actor_head_wide_launches advances by mini-batches x epochs with the knob on and not at all with it
off; the learning rate is equal and every parameter agrees within 1e-4 of its tensor's largest entry, the bound
tests/test_gpu_heads_narrow_update.py holds its knobs to."""

import json
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

CASES = {"flat_19": ([128, 128, 128], 19), "g1_24": ([256, 128, 64], 24)}
CHILD = r"""
import json, sys
import conftest  # puts the repository on sys.path
import numpy as np
import torch
from rsl_rl_amd.algorithms import PPO
from rsl_rl_amd.modules import ActorCritic
from rsl_rl_amd.networks import fused_mlp

dev = torch.device("cuda:0")
T, N, O = 8, 256, 48
result, tensors = {"knob": fused_mlp._ACTOR_HEAD_WIDE_K128, "cases": {}}, {}
pairs = []
real = fused_mlp.train_forward_pair
fused_mlp.train_forward_pair = lambda *a, **k: pairs.append(real(*a, **k)) or pairs[-1]
for name, (hidden, A) in json.loads(sys.argv[2]).items():
    rng = np.random.default_rng(5)
    obs, rewards, noise = (rng.standard_normal(s).astype(np.float32) for s in ((T, N, O), (T, N, 1), (T, N, A)))
    last = rng.standard_normal((N, O)).astype(np.float32)
    # the fields an older policy left behind: its mean a little off this one's, std 1, the log-prob of its actions
    mu = (0.15 * rng.standard_normal((T, N, A))).astype(np.float32)
    logp = (-0.5 * noise.astype(np.float64) ** 2 - 0.5 * np.log(2 * np.pi)).sum(-1, keepdims=True).astype(np.float32)
    obs0 = {"policy": torch.zeros(N, O)}
    torch.manual_seed(0)
    pol = ActorCritic(obs0, {"policy": ["policy"], "critic": ["policy"]}, A, actor_hidden_dims=hidden,
                      critic_hidden_dims=hidden)
    alg = PPO(pol, num_learning_epochs=1, num_mini_batches=2, device=dev, desired_kl=0.01)
    alg.init_storage("rl", N, T, obs0, [A])
    st = alg.storage
    st.observations["policy"].copy_(torch.from_numpy(obs))
    st.rewards.copy_(torch.from_numpy(rewards))
    st.values.copy_(torch.from_numpy((0.3 * rng.standard_normal((T, N, 1))).astype(np.float32)))
    st.actions_log_prob.copy_(torch.from_numpy(logp))
    st.mu.copy_(torch.from_numpy(mu))
    st.sigma.copy_(torch.ones(T, N, A))
    st.actions.copy_(torch.from_numpy(mu + noise))
    st.dones.zero_()
    st.step = T
    with torch.inference_mode():
        alg.compute_returns({"policy": torch.from_numpy(last).to(dev)})
    st.perm_generator = torch.Generator().manual_seed(1)
    before, n0 = fused_mlp.actor_head_wide_launches, len(pairs)
    alg.update()
    torch.cuda.synchronize()
    result["cases"][name] = {"launches": fused_mlp.actor_head_wide_launches - before, "lr": alg.learning_rate,
                             "paired_heads": sum(r is not None and r[1].head is not None for r in pairs[n0:])}
    tensors[name] = {k: v.detach().cpu() for k, v in pol.state_dict().items()}
torch.save(tensors, sys.argv[1])
print("RESULT " + json.dumps(result))
"""


def _child(knob, path):
    here = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, "-c", CHILD, str(path), json.dumps(CASES)], cwd=here,
                       env=dict(os.environ, RSLRL_ACTOR_HEAD_WIDE_K128=knob), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1]
    return json.loads(line[7:]), torch.load(path)


@pytest.fixture(scope="module")
def runs(cuda_device, tmp_path_factory):
    d = tmp_path_factory.mktemp("actor_head_wide_k128")
    return {knob: _child(knob, d / f"params_{knob}.pt") for knob in ("1", "0")}


@pytest.mark.parametrize("case", CASES)
def test_head_launches_and_the_paired_pass_follow_the_knob(runs, case):
    on, off = runs["1"][0], runs["0"][0]
    assert on["knob"] is True and off["knob"] is False
    assert on["cases"][case]["launches"] == 2 and off["cases"][case]["launches"] == 0
    # without the head a 17-to-32 actor never pairs; with it both mini-batches of [128, 128, 128] take the paired pass,
    # the actor's head on its tape
    assert off["cases"][case]["paired_heads"] == 0
    if case == "flat_19":
        assert on["cases"][case]["paired_heads"] == 2


@pytest.mark.parametrize("case", CASES)
def test_update_agrees_between_knob_on_and_off(runs, case):
    (on, p_on), (off, p_off) = runs["1"], runs["0"]
    assert on["cases"][case]["lr"] == off["cases"][case]["lr"]
    for k, ref in p_off[case].items():
        err, top = (p_on[case][k] - ref).abs().max().item(), ref.abs().max().item()
        print(case, k, err, top)
        assert err <= 1e-4 * top, (k, err, top)
