"""The fused GRU step (kernels.gru_cell / gru_cell_pair) against an fp64 evaluation of its formulas
(tests/gru_fixtures.py), with torch's own fp32 nn.GRU step on the same device as the yardstick (RMS error within 2x
torch's, the criterion of tests/test_gpu_lstm_cell.py), Memory's chained steps on it, and
ActorCriticRecurrent.act_and_evaluate on it against RSLRL_GRU_CELL=0."""

import ctypes

import pytest
import torch
import torch.nn as nn

import gru_fixtures as GF

pytestmark = pytest.mark.gpu

H = GF.H


def _gru(D, dev, seed):
    torch.manual_seed(seed)
    return nn.GRU(D, H).to(dev)


def _ref64(rnn, x, h):
    return GF.gru_step(x.double(), None if h is None else h.double(), *GF.params(rnn, torch.float64))[0]


def _rms(a, ref):
    return (a.double() - ref).square().mean().sqrt().item()


def _torch_step(rnn, x, h):
    _, hn = rnn(x.unsqueeze(0), None if h is None else h.unsqueeze(0).contiguous())
    return hn[0]


@pytest.mark.parametrize("D", [16, 48, 256])
@pytest.mark.parametrize("M", [64, 192])
def test_cell_matches_fp64_within_twice_torch(cuda_device, M, D):
    from rsl_rl_amd import kernels
    dev = cuda_device
    rnns = (_gru(D, dev, 1), _gru(D, dev, 2))
    g = torch.Generator().manual_seed(10 * M + D)
    xs = [torch.randn(M, D, generator=g).to(dev) for _ in range(2)]
    states = [0.5 * torch.randn(M, H, generator=g).to(dev) for _ in range(2)]
    with torch.no_grad():
        ops = [(kernels.gru_image(r.weight_ih_l0, r.weight_hh_l0), r.bias_ih_l0, r.bias_hh_l0) for r in rnns]
        for with_state in (False, True):
            st = states if with_state else [None, None]
            single = [kernels.gru_cell(xs[k], st[k], *ops[k]) for k in range(2)]
            pair = kernels.gru_cell_pair(xs[0], st[0], *ops[0], xs[1], st[1], *ops[1])
            again = [kernels.gru_cell(xs[k], st[k], *ops[k]) for k in range(2)]
            for k, rnn in enumerate(rnns):
                # the pair form equals two single calls bit for bit; repeated calls are bitwise equal
                assert torch.equal(pair[k], single[k]) and torch.equal(again[k], single[k])
                ref, tor = _ref64(rnn, xs[k], st[k]), _torch_step(rnn, xs[k], st[k])
                e_ours, e_torch = _rms(single[k], ref), _rms(tor, ref)
                print(f"M {M} D {D} state {with_state} net {k} h': rms ours {e_ours:.3e} torch {e_torch:.3e}")
                assert e_ours <= 2 * e_torch, (M, D, with_state, k, e_ours, e_torch)


def test_chained_steps_with_resets(cuda_device):
    """24 chained steps through Memory (the rollout's use), rows reset in between: reset rows exactly 0, the bare
    [1, M, 256] state kept, and the state after the chain within 2x torch's own chained fp32 error against the fp64
    chain."""
    from rsl_rl_amd.networks import Memory
    dev, M, D = cuda_device, 192, 48
    torch.manual_seed(3)
    mem = Memory(D, type="gru", num_layers=1, hidden_size=H).to(dev)
    g = torch.Generator().manual_seed(4)
    xs = [torch.randn(M, D, generator=g).to(dev) for _ in range(24)]
    dones = [(torch.rand(M, generator=g) < 0.1).to(dev).long() for _ in range(24)]
    ref = tor = None
    with torch.inference_mode():
        for t in range(24):
            assert mem.gru_cell_ok(xs[t]) and not mem.cell_ok(xs[t])
            out = mem(xs[t])
            assert out.shape == (1, M, H) and torch.is_tensor(mem.hidden_states)
            assert mem.hidden_states.shape == (1, M, H)
            ref = _ref64(mem.rnn, xs[t], ref)
            tor = _torch_step(mem.rnn, xs[t], tor)
            mem.reset(dones[t])
            mask = (dones[t] == 1).unsqueeze(1)
            ref, tor = torch.where(mask, torch.zeros_like(ref), ref), torch.where(mask, torch.zeros_like(tor), tor)
            assert (mem.hidden_states[0][dones[t] == 1] == 0.0).all()
        e_ours, e_torch = _rms(mem.hidden_states[0], ref), _rms(tor, ref)
        print(f"24 steps h: rms ours {e_ours:.3e} torch {e_torch:.3e}")
        assert e_ours <= 2 * e_torch, (e_ours, e_torch)


def test_unsupported_shapes_are_refused(cuda_device):
    from rsl_rl_amd import _lib, kernels
    dev = cuda_device
    rnn = _gru(48, dev, 5)
    img = kernels.gru_image(rnn.weight_ih_l0, rnn.weight_hh_l0)
    x = torch.zeros(128, 48, device=dev)
    out = torch.full((128, H), 7.0, device=dev)
    for M, D, hidden, layers in ((100, 48, 256, 1), (64, 40, 256, 1), (64, 48, 64, 1), (64, 48, 256, 2)):
        assert not kernels.gru_cell_supported(M, D, hidden, layers)
        a = _lib.GruCell(x.data_ptr(), None, img.data_ptr(), rnn.bias_ih_l0.data_ptr(), rnn.bias_hh_l0.data_ptr(),
                         out.data_ptr(), D, hidden, layers, 0)
        assert _lib.lib().rslrl_gru_cell(ctypes.byref(a), M, None) == _lib.E_UNSUPPORTED
    with pytest.raises(_lib.RslrlError):
        kernels.gru_cell(torch.zeros(100, 48, device=dev), None, img, rnn.bias_ih_l0, rnn.bias_hh_l0)
    torch.cuda.synchronize()
    assert (out == 7.0).all()  # nothing was launched


def _policy(dev, seed=0):
    from rsl_rl_amd.modules import ActorCriticRecurrent
    torch.manual_seed(seed)
    obs0 = {"policy": torch.zeros(128, 48)}
    return ActorCriticRecurrent(obs0, {"policy": ["policy"], "critic": ["policy"]}, 12, actor_hidden_dims=[64, 64],
                                critic_hidden_dims=[64, 64], rnn_type="gru", rnn_hidden_dim=H).to(dev)


def test_act_and_evaluate_fused_against_fallback(cuda_device, monkeypatch):
    from rsl_rl_amd import kernels
    dev = cuda_device
    pol = _policy(dev)
    g = torch.Generator().manual_seed(9)
    obs = [{"policy": torch.randn(128, 48, generator=g).to(dev)} for _ in range(3)]
    launches = []
    inner = kernels.gru_cell_pair
    monkeypatch.setattr(kernels, "gru_cell_pair", lambda *a: (launches.append(1), inner(*a))[1])
    results = {}
    for mode in ("1", "0"):
        monkeypatch.setenv("RSLRL_GRU_CELL", mode)
        pol.reset()
        torch.manual_seed(77)
        with torch.inference_mode():
            assert pol.memory_a.gru_cell_ok(obs[0]["policy"]) == (mode == "1")
            assert not pol.memory_a.cell_ok(obs[0]["policy"])  # cell_ok stays the LSTM cell's predicate
            for o in obs:
                actions, values = pol.act_and_evaluate(o)
            assert len(launches) == 3  # both memories in one launch per step, and none with RSLRL_GRU_CELL=0
            assert all(torch.is_tensor(m.hidden_states) and m.hidden_states.shape == (1, 128, H)
                       for m in (pol.memory_a, pol.memory_c))
            results[mode] = (actions, values, pol.action_mean.clone(), pol.memory_a.hidden_states.clone(),
                             pol.memory_c.hidden_states.clone(), torch.cuda.get_rng_state(dev))
    f, b = results["1"], results["0"]
    assert torch.equal(f[5], b[5])  # the same draws: the generator state afterwards is equal
    assert torch.allclose(f[0] - f[2], b[0] - b[2], atol=1e-5)  # the same standard normals
    # means, values and states: the existing bound of tests/test_gpu_lstm_cell.py (two fp32-faithful evaluations of
    # the same formulas over 3 chained steps and two 64-wide layers)
    for x, y in ((f[2], b[2]), (f[1], b[1]), (f[3], b[3]), (f[4], b[4])):
        assert x.shape == y.shape and (x - y).abs().max().item() <= 2e-5 * (1 + y.abs().max().item())
