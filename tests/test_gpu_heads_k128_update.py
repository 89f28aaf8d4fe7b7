"""One PPO.update() with the heads for a last hidden layer with 128 inputs on the smallest policy
shapes -- 256 envs, T = 8, 2 mini-batches (1,024 rows each), 1 epoch, obs 48, 12 actions:

* [128, 128, 128] (the paired pass; the heads' dz goes into the fused 128-wide hidden backward),
* [256, 128, 64] (the paired forward, then one backward per network: the 128 -> 64 layer's bias gradient is dz.sum(0)),
* ActorCriticRecurrent with a GRU of 256 in front of [256, 128, 128] (through train_forward_rows).

RSLRL_HEAD_K128 is read at import, so each knob value runs in a fresh child process (one child for the three shapes; the
builders are tests/test_gpu_heads_narrow_update.py's).  With the knob on, fused_mlp.actor_head_launches advances by
mini-batches x epochs; with RSLRL_HEAD_K128=0 it does not.  The learning rate is equal, the loss means and every
parameter agree within 1e-4 of the tensor's largest entry -- the bound the project holds two update paths to, valid here
because the heads' dz carries the separate launches' bits (tests/test_gpu_heads_k128.py): only the two output layers'
[dW | db] have another summation order."""

import json
import os
import subprocess
import sys

import pytest
import torch

from test_gpu_heads_narrow_update import CHILD as NARROW_CHILD, EPOCHS, MINI_BATCHES

pytestmark = pytest.mark.gpu

CASES = ["flat", "g1_64", "gru"]
# The child is tests/test_gpu_heads_narrow_update.py's with other stacks and the other knob.  Each edit of its text is
# checked here, and the stacks the children really built are checked from their parameters' shapes (test below).
_BUILDERS, _LOOP = NARROW_CHILD.split("BUILD = {")
_SETUP, _RUN = _LOOP.split("result, tensors = {}, {}")
assert _BUILDERS.count("[256, 256, 128]") == 2 and _RUN.count("_HEAD_NARROW") == 1 and "feedforward(" in _SETUP
CHILD = (_BUILDERS.replace("[256, 256, 128]", "[256, 128, 128]")  # the recurrent builder's actor and critic stacks
         + 'BUILD = {"flat": lambda: feedforward([128, 128, 128], 48), "g1_64": lambda: feedforward([256, 128, 64], 48),\n'
         + '         "gru": recurrent}\nresult, tensors = {}, {}' + _RUN.replace("_HEAD_NARROW", "_HEAD_K128"))
STACKS = {"flat": [128, 128, 128], "g1_64": [256, 128, 64], "gru": [256, 128, 128]}


def _child(knob, path):
    here = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, "-c", CHILD, str(path)], cwd=here, env=dict(os.environ, RSLRL_HEAD_K128=knob),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1]
    return json.loads(line[7:]), torch.load(path)


@pytest.fixture(scope="module")
def runs(cuda_device, tmp_path_factory):
    d = tmp_path_factory.mktemp("heads_k128")
    return {knob: _child(knob, d / f"params_{knob}.pt") for knob in ("1", "0")}


@pytest.mark.parametrize("case", CASES)
def test_actor_head_launches_follow_the_knob(runs, case):
    for params in (runs["1"][1][case], runs["0"][1][case]):  # the stack the child built: 128 inputs into the last layer
        for net in ("actor", "critic"):
            assert [params[f"{net}.{2 * i}.weight"].shape[0] for i in range(3)] == STACKS[case]
    assert runs["1"][0]["knob"] is True and runs["0"][0]["knob"] is False
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
