"""rslrl_rollout_mlp_shaped_pair (csrc/rollout_mlp_shaped.hip: the rollout's actor and critic forward in one launch for
[512, 256, 128], [256, 256, 128], [256, 128, 128] and [128, 128, 128] stacks on any input width up to 256) against the
fused training forward -- bit for bit -- and against fp64 torch; masked reads, the Normal sample, the routing of
ActorCritic.act_and_evaluate and the C ABI's refusals."""

import ctypes
import functools

import pytest
import torch

from rsl_rl_amd import _lib, kernels
from rsl_rl_amd.modules import ActorCritic
from rsl_rl_amd.modules.act_graph import RolloutActGraph
from rsl_rl_amd.networks import MLP, fused_mlp

pytestmark = pytest.mark.gpu

# (hidden widths, (k0 actor, k0 critic), (outputs actor, critic), rows); 4128 rows = 129 tiles
CASES = [
    ([512, 256, 128], (235, 235), (12, 1), 4128),
    ([512, 256, 128], (48, 53), (16, 3), 32),
    ([256, 256, 128], (45, 48), (7, 1), 96),
    ([256, 128, 128], (123, 256), (12, 1), 32),
    ([128, 128, 128], (48, 48), (12, 1), 4128),
    ([128, 128, 128], (1, 5), (5, 4), 32),
]


def _mlp(k0, hidden, nout, dev, g):
    m = MLP(k0, nout, hidden).to(dev)
    with torch.no_grad():
        for p in m.parameters():  # tests/test_gpu_rollout_mlp.py's scales: ELU takes both branches
            p.copy_(torch.randn(p.shape, device=dev, generator=g) * (0.3 if p.dim() == 1 else 1.2 / p.shape[-1] ** 0.5))
    return m


@functools.lru_cache(maxsize=None)
def _case(idx):
    """The case's networks, inputs, plan (weights, biases, images) and one-launch outputs, computed once."""
    hidden, k0s, nouts, M = CASES[idx]
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(100 + idx)
    ms = [_mlp(k0s[i], hidden, nouts[i], dev, g) for i in range(2)]
    xs = [torch.randn(M, k0s[0], device=dev, generator=g), torch.randn(M, k0s[1], device=dev, generator=g) * 3.0]
    plan = fused_mlp._shaped_pair_plan(*ms)
    assert plan is not None
    with torch.inference_mode():
        ys = fused_mlp.rollout_mlp_shaped_pair(xs, *plan[:3])
    assert ys is not None
    return ms, xs, plan, ys


def _struct(plan, i, x, y, eps=None, std=None):
    ws, bs, imgs, _ = plan
    a = _lib.RolloutMlpShaped()
    a.x, a.k0, a.nout, a.y = x.data_ptr(), x.shape[1], ws[i][3].shape[0], y.data_ptr()
    for l in range(3):
        a.width[l], a.bimage[l], a.bias[l] = ws[i][l].shape[0], imgs[i][0][l].data_ptr(), bs[i][l].data_ptr()
    a.out_image, a.out_bias = imgs[i][2].data_ptr(), bs[i][3].data_ptr()
    if eps is not None:
        a.sample, a.sample_scale = eps.data_ptr(), std.data_ptr()
    return a


@pytest.mark.parametrize("idx", range(len(CASES)))
def test_bits_of_the_training_forward_and_fp64(idx, cuda_device):
    ms, xs, _, ys = _case(idx)
    for m, x, y in zip(ms, xs, ys):
        ref = m(x).detach()  # under autograd: FusedMLPFunction, the fused training forward at any row count
        assert torch.equal(y, ref), float((y - ref).abs().max())
        y64 = m.double()(x.double()).detach()
        m.float()
        top = max(1.0, float(y64.abs().max()))
        print(CASES[idx], "err", float((y.double() - y64).abs().max()), "bound", 2e-5 * top)
        assert float((y.double() - y64).abs().max()) <= 2e-5 * top


@pytest.mark.parametrize("idx", [1, 4])  # ragged (53 floats: rows at 4-byte-aligned bases) and 4-aligned inputs
def test_reads_and_writes_stay_inside_their_rows(idx, cuda_device):
    """x as the last rows of a buffer followed by a NaN band, y and eps inside NaN bands: finite outputs equal to the
    plain launch's, the bands untouched."""
    ms, xs, plan, ys = _case(idx)
    M, band = xs[0].shape[0], 3
    std = torch.rand(ys[0].shape[1], device=xs[0].device) + 0.2

    def banded(t):
        buf = torch.full((M + 2 * band, t.shape[1]), float("nan"), device=t.device)
        buf[band:band + M] = t
        return buf

    xb = [banded(x) for x in xs]
    yb = [banded(torch.zeros_like(y)) for y in ys]
    eb = banded(torch.zeros_like(ys[0]))
    args = [_struct(plan, i, xb[i][band:band + M], yb[i][band:band + M], *((eb[band:band + M], std) if i == 0 else ()))
            for i in range(2)]
    assert _lib.lib().rslrl_rollout_mlp_shaped_pair(ctypes.byref(args[0]), ctypes.byref(args[1]), M, None) == 0
    torch.cuda.synchronize()
    for buf, y in zip(yb, ys):
        assert torch.equal(buf[band:band + M], y)
        assert bool(buf[:band].isnan().all()) and bool(buf[band + M:].isnan().all())
    assert torch.equal(eb[band:band + M], ys[0])  # eps 0: the sample is 0 * std + mu
    assert bool(eb[:band].isnan().all()) and bool(eb[band + M:].isnan().all())


def test_sample_matches_normal_affine(cuda_device):
    ms, xs, plan, ys = _case(1)
    dev, (M, A) = xs[0].device, ys[0].shape
    g = torch.Generator(device=dev).manual_seed(3)
    std = torch.rand(A, device=dev, generator=g) + 0.2
    eps = torch.randn(M, A, device=dev, generator=g)
    eps0 = eps.clone()
    with torch.inference_mode():
        y = fused_mlp.rollout_mlp_shaped_pair(xs, *plan[:3], sample=(eps, std))
        ref = kernels.normal_affine_(eps0.clone(), std.expand(M, A), ys[0])
    assert torch.equal(y[0], ys[0]) and torch.equal(y[1], ys[1])
    assert torch.equal(eps, ref) and not torch.equal(eps, eps0)


def _policy(n, dev):
    torch.manual_seed(0)
    obs = {"policy": torch.randn(n, 235, device=dev)}
    pol = ActorCritic(obs, {"policy": ["policy"], "critic": ["policy"]}, 12, actor_hidden_dims=[512, 256, 128],
                      critic_hidden_dims=[512, 256, 128]).to(dev)
    return pol, obs


def _counts():
    return fused_mlp.rollout_mlp_shaped_launches, fused_mlp.wide_launches, fused_mlp.ragged_launches


def test_act_and_evaluate_takes_one_shaped_launch(cuda_device, monkeypatch):
    pol, obs = _policy(4096, cuda_device)
    with torch.inference_mode():
        c0 = _counts()
        torch.cuda.manual_seed(5)
        a, v = pol.act_and_evaluate(obs)
        c1 = _counts()
        torch.cuda.manual_seed(5)
        eps = torch.empty_like(a).normal_()
    assert (c1[0] - c0[0], c1[1] - c0[1], c1[2] - c0[2]) == (1, 0, 0)
    mean = pol.actor(obs["policy"]).detach()  # under autograd: the fused training forward
    assert torch.equal(pol.action_mean, mean) and torch.equal(v, pol.critic(obs["policy"]).detach())
    assert torch.equal(a, eps * pol.action_std + mean)
    with torch.inference_mode():  # at the wide bound, and with the knob off: today's path
        big = {"policy": torch.randn(fused_mlp.WIDE_FWD_MIN_ROWS, 235, device=cuda_device)}
        n0 = fused_mlp.rollout_mlp_shaped_launches
        pol.act_and_evaluate(big)
        monkeypatch.setattr(fused_mlp, "_ROLLOUT_MLP_SHAPED", False)
        pol.act_and_evaluate(obs)
    assert fused_mlp.rollout_mlp_shaped_launches == n0


def test_graph_replayed_act_is_the_eager_act(cuda_device):
    """tests/test_gpu_ragged_update.py's graph test on the shaped launch: six steps at 4,096 envs."""
    N = 4096
    pol, _ = _policy(N, cuda_device)
    g = RolloutActGraph(pol)
    gen = torch.Generator(device=cuda_device).manual_seed(1)
    replayed, start = 0, fused_mlp.rollout_mlp_shaped_launches
    with torch.inference_mode(), fused_mlp.frozen_weights():
        for step in range(6):
            x = torch.randn(N, 235, device=cuda_device, generator=gen)
            torch.cuda.manual_seed(100 + step)
            res = g({"policy": x})
            replayed += res is not None
            if res is None:
                res = pol.act_and_evaluate({"policy": x})
            a, v, mu = res[0].clone(), res[1].clone(), pol.action_mean.clone()
            torch.cuda.manual_seed(100 + step)
            a_ref, v_ref = pol.act_and_evaluate({"policy": x.clone()})
            assert torch.equal(a, a_ref) and torch.equal(v, v_ref) and torch.equal(mu, pol.action_mean), step
    assert g._graph is not None and replayed >= 4, "the shaped step was not captured"
    assert fused_mlp.rollout_mlp_shaped_launches >= start + 6


@pytest.mark.parametrize("change", [
    {"width": (256, 256, 256)}, {"width1": (256, 128, 128)}, {"k0": 0}, {"k0": 257}, {"nout": 17}, {"M": 40},
], ids=lambda c: next(iter(c)) + str(next(iter(c.values()))))
def test_c_abi_refuses(change, cuda_device):
    x = torch.zeros(64, 48, device=cuda_device)
    y = torch.full((64, 17), 7.0, device=cuda_device)
    a = [_lib.RolloutMlpShaped() for _ in range(2)]
    for s in a:
        s.x, s.k0, s.nout, s.y = x.data_ptr(), 48, 12, y.data_ptr()
        s.width[:] = (128, 128, 128)
    for s in a:
        s.k0, s.nout = change.get("k0", s.k0), change.get("nout", s.nout)
        s.width[:] = change.get("width", (128, 128, 128))
    a[1].width[:] = change.get("width1", tuple(a[1].width))
    L = _lib.lib()
    assert L.rslrl_rollout_mlp_shaped_pair(ctypes.byref(a[0]), ctypes.byref(a[1]), change.get("M", 64), None) \
        == _lib.E_UNSUPPORTED
    assert L.rslrl_rollout_mlp_shaped_pair(ctypes.byref(a[0]), ctypes.byref(a[1]), 0, None) == 0
    torch.cuda.synchronize()
    assert bool((y == 7.0).all())
