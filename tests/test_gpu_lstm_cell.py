"""The fused LSTM step (kernels.lstm_cell / lstm_cell_pair) against an fp64 evaluation of its formulas, with torch's
own fp32 nn.LSTM step on the same device as the yardstick (the criterion tests/test_gpu_fused_mlp.py applies to the
x6 GEMMs: RMS error within 2x torch's), and ActorCriticRecurrent.act_and_evaluate on it against RSLRL_LSTM_CELL=0."""

import ctypes

import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

H = 256


def _lstm(D, dev, seed):
    torch.manual_seed(seed)
    return nn.LSTM(D, H).to(dev)


def _ref64(rnn, x, state):
    """gates = x W_ih^T + b_ih + h W_hh^T + b_hh (i, f, g, o); c' = s(f) c + s(i) tanh(g); h' = s(o) tanh(c')."""
    w_ih, w_hh = rnn.weight_ih_l0.double(), rnn.weight_hh_l0.double()
    b_ih, b_hh = rnn.bias_ih_l0.double(), rnn.bias_hh_l0.double()
    h, c = (torch.zeros(x.shape[0], H, dtype=torch.float64, device=x.device),) * 2 if state is None else \
        (state[0].double(), state[1].double())
    gates = x.double() @ w_ih.t() + b_ih + h @ w_hh.t() + b_hh
    i, f, g, o = gates.chunk(4, dim=1)
    c2 = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
    return torch.sigmoid(o) * torch.tanh(c2), c2


def _rms(a, ref):
    return (a.double() - ref).square().mean().sqrt().item()


def _torch_step(rnn, x, state):
    st = None if state is None else (state[0].unsqueeze(0).contiguous(), state[1].unsqueeze(0).contiguous())
    _, (h, c) = rnn(x.unsqueeze(0), st)
    return h[0], c[0]


@pytest.mark.parametrize("D", [16, 48, 256])
@pytest.mark.parametrize("M", [64, 192])
def test_cell_matches_fp64_within_twice_torch(cuda_device, M, D):
    from rsl_rl_amd import kernels
    dev = cuda_device
    rnn_a, rnn_c = _lstm(D, dev, 1), _lstm(D, dev, 2)
    g = torch.Generator().manual_seed(10 * M + D)
    xs = [torch.randn(M, D, generator=g).to(dev) for _ in range(2)]
    states = [(0.5 * torch.randn(M, H, generator=g).to(dev), torch.randn(M, H, generator=g).to(dev))
              for _ in range(2)]
    with torch.no_grad():
        ops = [(kernels.lstm_image(r.weight_ih_l0, r.weight_hh_l0), r.bias_ih_l0, r.bias_hh_l0)
               for r in (rnn_a, rnn_c)]
        for with_state in (False, True):
            st = states if with_state else [None, None]
            single = [kernels.lstm_cell(xs[k], st[k], *ops[k]) for k in range(2)]
            pair = kernels.lstm_cell_pair(xs[0], st[0], *ops[0], xs[1], st[1], *ops[1])
            again = [kernels.lstm_cell(xs[k], st[k], *ops[k]) for k in range(2)]
            for k, rnn in enumerate((rnn_a, rnn_c)):
                # the pair form equals two single calls bit for bit; repeated calls are bitwise equal
                assert torch.equal(pair[k][0], single[k][0]) and torch.equal(pair[k][1], single[k][1])
                assert torch.equal(again[k][0], single[k][0]) and torch.equal(again[k][1], single[k][1])
                ref = _ref64(rnn, xs[k], st[k])
                tor = _torch_step(rnn, xs[k], st[k])
                for name, ours, theirs, r in (("h'", single[k][0], tor[0], ref[0]), ("c'", single[k][1], tor[1], ref[1])):
                    e_ours, e_torch = _rms(ours, r), _rms(theirs, r)
                    print(f"M {M} D {D} state {with_state} net {k} {name}: rms ours {e_ours:.3e} torch {e_torch:.3e}")
                    assert e_ours <= 2 * e_torch, (M, D, with_state, k, name, e_ours, e_torch)


def test_chained_steps_with_resets(cuda_device):
    """24 chained steps through Memory (the rollout's use), rows reset in between: reset rows exactly 0, and the
    states after the chain within 2x torch's own chained fp32 error against the fp64 chain."""
    from rsl_rl_amd.networks import Memory
    dev, M, D = cuda_device, 192, 48
    torch.manual_seed(3)
    mem = Memory(D, type="lstm", num_layers=1, hidden_size=H).to(dev)
    g = torch.Generator().manual_seed(4)
    xs = [torch.randn(M, D, generator=g).to(dev) for _ in range(24)]
    dones = [(torch.rand(M, generator=g) < 0.1).to(dev).long() for _ in range(24)]
    ref = tor = None
    with torch.inference_mode():
        for t in range(24):
            assert mem.cell_ok(xs[t])
            out = mem(xs[t])
            assert out.shape == (1, M, H)
            ref = _ref64(mem.rnn, xs[t], ref)
            tor = _torch_step(mem.rnn, xs[t], tor)
            mem.reset(dones[t])
            mask = (dones[t] == 1).unsqueeze(1)
            ref = tuple(torch.where(mask, torch.zeros_like(s), s) for s in ref)
            tor = tuple(torch.where(mask, torch.zeros_like(s), s) for s in tor)
            for s in mem.hidden_states:
                assert (s[0][dones[t] == 1] == 0.0).all()
        for name, ours, theirs, r in (("h", mem.hidden_states[0][0], tor[0], ref[0]),
                                      ("c", mem.hidden_states[1][0], tor[1], ref[1])):
            e_ours, e_torch = _rms(ours, r), _rms(theirs, r)
            print(f"24 steps {name}: rms ours {e_ours:.3e} torch {e_torch:.3e}")
            assert e_ours <= 2 * e_torch, (name, e_ours, e_torch)


def test_unsupported_shapes_are_refused(cuda_device):
    from rsl_rl_amd import _lib, kernels
    dev = cuda_device
    assert not kernels.lstm_cell_supported(100, 48, 256) and not kernels.lstm_cell_supported(64, 40, 256)
    assert not kernels.lstm_cell_supported(64, 48, 64) and not kernels.lstm_cell_supported(64, 48, 256, 2)
    rnn = _lstm(48, dev, 5)
    img = kernels.lstm_image(rnn.weight_ih_l0, rnn.weight_hh_l0)
    x = torch.zeros(128, 48, device=dev)
    out = torch.full((2, 128, H), 7.0, device=dev)
    for M, D, hidden in ((100, 48, 256), (64, 40, 256), (64, 48, 128)):
        a = _lib.LstmCell(x.data_ptr(), None, None, img.data_ptr(), rnn.bias_ih_l0.data_ptr(),
                          rnn.bias_hh_l0.data_ptr(), out[0].data_ptr(), out[1].data_ptr(), D, hidden, 1, 0)
        assert _lib.lib().rslrl_lstm_cell(ctypes.byref(a), M, None) == _lib.E_UNSUPPORTED
    torch.cuda.synchronize()
    assert (out == 7.0).all()  # nothing was launched


def _policy(dev, rnn="lstm", hidden=H, seed=0):
    from rsl_rl_amd.modules import ActorCriticRecurrent
    torch.manual_seed(seed)
    obs0 = {"policy": torch.zeros(128, 48)}
    return ActorCriticRecurrent(obs0, {"policy": ["policy"], "critic": ["policy"]}, 12, actor_hidden_dims=[64, 64],
                                critic_hidden_dims=[64, 64], rnn_type=rnn, rnn_hidden_dim=hidden).to(dev)


def test_act_and_evaluate_fused_against_fallback(cuda_device, monkeypatch):
    dev = cuda_device
    pol = _policy(dev)
    g = torch.Generator().manual_seed(9)
    obs = [{"policy": torch.randn(128, 48, generator=g).to(dev)} for _ in range(3)]
    results = {}
    for mode in ("1", "0"):
        monkeypatch.setenv("RSLRL_LSTM_CELL", mode)
        pol.reset()
        torch.manual_seed(77)
        with torch.inference_mode():
            assert pol.memory_a.cell_ok(obs[0]["policy"]) == (mode == "1")
            for o in obs:
                actions, values = pol.act_and_evaluate(o)
            results[mode] = (actions, values, pol.action_mean.clone(), [s.clone() for s in pol.memory_a.hidden_states],
                             [s.clone() for s in pol.memory_c.hidden_states], torch.cuda.get_rng_state(dev))
    f, b = results["1"], results["0"]
    assert torch.equal(f[5], b[5])  # the same draws: the generator state afterwards is equal
    # the same standard normals: actions differ only through the means
    assert torch.allclose(f[0] - f[2], b[0] - b[2], atol=1e-5)
    # means, values and hidden states: two fp32-faithful evaluations of the same formulas (each within the cell bound
    # of the fp64 value: test_cell_matches_fp64_within_twice_torch).  A gate is an fp32 sum of <= 304 products of
    # O(1) size: rounding ~ sqrt(304) * 6e-8 ~ 1e-6, carried through 3 chained steps and two 64-wide layers with
    # O(1) gains; 2e-5 relative to the tensor's scale leaves about an order of magnitude over that
    for x, y in [(f[2], b[2]), (f[1], b[1])] + list(zip(f[3], b[3])) + list(zip(f[4], b[4])):
        assert x.shape == y.shape and (x - y).abs().max().item() <= 2e-5 * (1 + y.abs().max().item())


@pytest.mark.parametrize("rnn,hidden", [("gru", 256), ("lstm", 64)])
def test_other_memories_take_the_fallback(cuda_device, rnn, hidden):
    dev = cuda_device
    pol = _policy(dev, rnn, hidden)
    obs = {"policy": torch.randn(128, 48, device=dev)}
    with torch.inference_mode():
        assert not pol.memory_a.cell_ok(obs["policy"]) and not pol.memory_c.cell_ok(obs["policy"])
        actions, values = pol.act_and_evaluate(obs)
        torch.manual_seed(1)
        pol.reset()
        a1, v1 = pol.act_and_evaluate(obs)
        torch.manual_seed(1)
        pol.reset()
        a2, v2 = pol.act(obs), pol.evaluate(obs)
    assert actions.shape == (128, 12) and values.shape == (128, 1)
    assert torch.equal(a1, a2) and torch.equal(v1, v2)
