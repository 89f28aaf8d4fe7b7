"""The fused LSTM / GRU cells at input widths that are no multiple of 16 (the `_anyd` entry points).

The central check is the padded-problem identity: a masked element enters every MFMA as an exact zero and the chunk
order and per-chunk summation are those of the first kernels, so the new entry on (x, W_ih) equals, bit for bit, the
first entry on x and W_ih zero-padded to the next multiple of 16 columns -- rollout form and training form (stored
gates, h as consumed, resets and restart states), single and paired.  x lies inside a buffer whose bytes before and
after are NaN: a load outside [x, x + 4 M D) would show in the outputs.  Above 256 columns, where there is no first
kernel, the new entry on D equals the new entry on the padded problem, and the accuracy criterion of
tests/test_gpu_lstm_cell.py applies (RMS error against fp64 within 2x that of torch's fp32 step on the same device)."""

import ctypes

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

H = 256
IDENTITY_D = [1, 2, 3, 5, 17, 30, 40, 45, 63, 235, 255]
GUARD = 64  # floats of NaN on either side of x (a multiple of 4: x's base stays 16-byte aligned where D % 4 == 0)


def _ceil16(D):
    return -(-D // 16) * 16


def _rnn(kind, D, dev, seed):
    torch.manual_seed(seed)
    return (nn.LSTM if kind == "lstm" else nn.GRU)(D, H).to(dev)


def _guarded(x, lead=GUARD):
    """x copied into the middle of a NaN buffer; where its width is no multiple of 4 the base is 4-byte aligned only."""
    M, D = x.shape
    lead = lead + (1 if D % 4 else 0)
    buf = torch.full((lead + M * D + GUARD,), float("nan"), device=x.device)
    view = buf[lead:lead + M * D].view(M, D)
    view.copy_(x)
    assert view.is_contiguous() and view.data_ptr() % (4 if D % 4 else 16) == 0
    return view


class Problem:
    """One memory at width D with its operands at width D and zero-padded to Dp = ceil16(D)."""

    def __init__(self, kind, D, M, dev, seed):
        from rsl_rl_amd import kernels
        self.kind, self.D, self.M, self.Dp = kind, D, M, _ceil16(D)
        self.rnn = rnn = _rnn(kind, D, dev, seed)
        g = torch.Generator().manual_seed(100 * seed + D + M)
        x = torch.randn(M, D, generator=g).to(dev)
        self.x, self.xp = _guarded(x), F.pad(x, (0, self.Dp - D)).contiguous()
        n = 2 if kind == "lstm" else 1
        self.state = tuple((0.5 if i == 0 else 1.0) * torch.randn(M, H, generator=g).to(dev) for i in range(n))
        self.restart = tuple(torch.randn(M, H, generator=g).to(dev) for _ in range(n))
        reset = torch.rand(M, generator=g) < 0.1
        reset[3::32] = True  # a reset row in every 32-row block
        self.reset = reset.to(torch.uint8).to(dev)
        image = kernels.lstm_image if kind == "lstm" else kernels.gru_image
        with torch.no_grad():
            w_ih, w_hh = rnn.weight_ih_l0.detach(), rnn.weight_hh_l0.detach()
            self.ops = (image(w_ih, w_hh), rnn.bias_ih_l0.detach(), rnn.bias_hh_l0.detach())
            self.ops_p = (image(F.pad(w_ih, (0, self.Dp - D)).contiguous(), w_hh), self.ops[1], self.ops[2])

    def _st(self, with_state):
        if not with_state:
            return None
        return self.state if self.kind == "lstm" else self.state[0]

    def step_args(self, with_state, padded=False):
        return ((self.xp if padded else self.x), self._st(with_state)) + (self.ops_p if padded else self.ops)

    def step(self, with_state, padded=False):
        from rsl_rl_amd import kernels
        out = (kernels.lstm_cell if self.kind == "lstm" else kernels.gru_cell)(*self.step_args(with_state, padded))
        return out if self.kind == "lstm" else (out,)

    def train_args(self, with_state, padded=False):
        """(arguments of the training form, its outputs): h', (c',) gates, h as consumed."""
        dev, M = self.x.device, self.M
        x, st, image, b_ih, b_hh = self.step_args(with_state, padded)
        new = lambda *s: torch.full(s, float("nan"), device=dev)  # noqa: E731
        h_out, gates, h_in = new(M, H), new(4, M, H), new(M, H)
        a = dict(x=x, image=image, b_ih=b_ih, b_hh=b_hh, reset=self.reset, h_out=h_out, gates=gates,
                 h_restart=self.restart[0], h_in_out=h_in)
        if self.kind == "lstm":
            c_out = new(M, H)
            a.update(state=st, c_out=c_out, c_restart=self.restart[1])
            return a, (h_out, c_out, gates, h_in)
        a.update(h=st)
        return a, (h_out, gates, h_in)

    def train(self, with_state, padded=False):
        from rsl_rl_amd import kernels
        a, outs = self.train_args(with_state, padded)
        (kernels.lstm_cell_train if self.kind == "lstm" else kernels.gru_cell_train)(**a)
        return outs


def _same(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


def _finite(ts):
    return all(bool(torch.isfinite(t).all()) for t in ts)


@pytest.mark.parametrize("M", [64, 192])
@pytest.mark.parametrize("D", IDENTITY_D)
@pytest.mark.parametrize("kind", ["lstm", "gru"])
def test_padded_problem_identity(cuda_device, kind, D, M):
    from rsl_rl_amd import kernels
    assert kernels._rnn_anyd(D) and not kernels._rnn_anyd(_ceil16(D))  # the new entry against the first one
    p = Problem(kind, D, M, cuda_device, 1)
    # the other problem of the pair launches: a width of the other load form, so that one launch mixes the two
    q = Problem(kind, 53 if D % 4 == 0 else 40, M, cuda_device, 2)
    pair = kernels.lstm_cell_pair if kind == "lstm" else kernels.gru_cell_pair
    train_pair = kernels.lstm_cell_train_pair if kind == "lstm" else kernels.gru_cell_train_pair
    with torch.no_grad():
        for with_state in (False, True):
            new, first = p.step(with_state), p.step(with_state, padded=True)
            assert _finite(new) and _same(new, first), (kind, D, M, with_state, "rollout form")
            assert _same(p.step(with_state), new)  # a repeated call
            both = pair(*p.step_args(with_state), *q.step_args(with_state))
            both = both if kind == "lstm" else ((both[0],), (both[1],))
            assert _same(both[0], new) and _same(both[1], q.step(with_state)), (kind, D, M, with_state, "pair")

            new, first = p.train(with_state), p.train(with_state, padded=True)
            assert _finite(new) and _same(new, first), (kind, D, M, with_state, "training form")
            assert _same(p.train(with_state), new)
            (a0, o0), (a1, o1) = p.train_args(with_state), q.train_args(with_state)
            train_pair(a0, a1)
            assert _same(o0, new) and _same(o1, q.train(with_state)), (kind, D, M, with_state, "training pair")
            # rows whose reset flag is set consumed the restart state, the others the given one (or zero)
            h_in = new[-1]
            rst = p.reset.bool()
            assert torch.equal(h_in[rst], p.restart[0][rst])
            want = p.state[0][~rst] if with_state else torch.zeros_like(h_in[~rst])
            assert torch.equal(h_in[~rst], want)


@pytest.mark.parametrize("D", [260, 1021])
@pytest.mark.parametrize("kind", ["lstm", "gru"])
def test_wide_inputs_equal_their_padded_problem(cuda_device, kind, D):
    """No first kernel above 256 columns: the new entry on D against the new entry on ceil16(D) (whole chunks only)."""
    from rsl_rl_amd import kernels
    assert kernels._rnn_anyd(D) and kernels._rnn_anyd(_ceil16(D))
    p = Problem(kind, D, 64, cuda_device, 3)
    with torch.no_grad():
        for with_state in (False, True):
            new = p.step(with_state)
            assert _finite(new) and _same(new, p.step(with_state, padded=True))
            new = p.train(with_state)
            assert _finite(new) and _same(new, p.train(with_state, padded=True))


def _ref64(kind, rnn, x, state):
    w_ih, w_hh = rnn.weight_ih_l0.double(), rnn.weight_hh_l0.double()
    b_ih, b_hh = rnn.bias_ih_l0.double(), rnn.bias_hh_l0.double()
    zeros = torch.zeros(x.shape[0], H, dtype=torch.float64, device=x.device)
    if kind == "lstm":
        h, c = (zeros, zeros) if state is None else (state[0].double(), state[1].double())
        i, f, g, o = (x.double() @ w_ih.t() + b_ih + h @ w_hh.t() + b_hh).chunk(4, dim=1)
        c2 = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
        return torch.sigmoid(o) * torch.tanh(c2), c2
    h = zeros if state is None else state[0].double()
    xr, xz, xn = (x.double() @ w_ih.t() + b_ih).chunk(3, dim=1)
    hr, hz, hn = (h @ w_hh.t() + b_hh).chunk(3, dim=1)
    r, z = torch.sigmoid(xr + hr), torch.sigmoid(xz + hz)
    n = torch.tanh(xn + r * hn)
    return ((1 - z) * n + z * h,)


def _torch_step(kind, rnn, x, state):
    st = None if state is None else tuple(s.unsqueeze(0).contiguous() for s in state)
    if kind == "lstm":
        _, (h, c) = rnn(x.unsqueeze(0), st)
        return h[0], c[0]
    _, h = rnn(x.unsqueeze(0), None if st is None else st[0])
    return (h[0],)


def _rms(a, ref):
    return (a.double() - ref).square().mean().sqrt().item()


@pytest.mark.parametrize("D", [260, 300, 1021, 1024])
@pytest.mark.parametrize("kind", ["lstm", "gru"])
def test_wide_inputs_match_fp64_within_twice_torch(cuda_device, kind, D):
    p = Problem(kind, D, 64, cuda_device, 4)
    with torch.no_grad():
        for with_state in (False, True):
            st = p.state if with_state else None
            ours, ref, tor = p.step(with_state), _ref64(kind, p.rnn, p.x, st), _torch_step(kind, p.rnn, p.x, st)
            for name, o, t, r in zip(("h'", "c'"), ours, tor, ref):
                e_ours, e_torch = _rms(o, r), _rms(t, r)
                print(f"{kind} D {D} state {with_state} {name}: rms ours {e_ours:.3e} torch {e_torch:.3e}")
                assert e_ours <= 2 * e_torch, (kind, D, with_state, name, e_ours, e_torch)


@pytest.mark.parametrize("kind", ["lstm", "gru"])
def test_chained_steps_with_resets_at_45(cuda_device, kind):
    """24 chained steps through Memory at the blind-locomotion width, rows reset in between."""
    from rsl_rl_amd.networks import Memory
    dev, M, D = cuda_device, 192, 45
    torch.manual_seed(3)
    mem = Memory(D, type=kind, num_layers=1, hidden_size=H).to(dev)
    g = torch.Generator().manual_seed(4)
    xs = [torch.randn(M, D, generator=g).to(dev) for _ in range(24)]
    dones = [(torch.rand(M, generator=g) < 0.1).to(dev).long() for _ in range(24)]
    ref = tor = None
    with torch.inference_mode():
        for t in range(24):
            assert (mem.cell_ok(xs[t]), mem.gru_cell_ok(xs[t])) == (kind == "lstm", kind == "gru")
            assert mem(xs[t]).shape == (1, M, H)
            ref = _ref64(kind, mem.rnn, xs[t], ref)
            tor = _torch_step(kind, mem.rnn, xs[t], tor)
            mem.reset(dones[t])
            mask = (dones[t] == 1).unsqueeze(1)
            ref = tuple(torch.where(mask, torch.zeros_like(s), s) for s in ref)
            tor = tuple(torch.where(mask, torch.zeros_like(s), s) for s in tor)
            states = mem.hidden_states if kind == "lstm" else (mem.hidden_states,)
            for s in states:
                assert (s[0][dones[t] == 1] == 0.0).all()
        for name, ours, theirs, r in zip("hc", states, tor, ref):
            e_ours, e_torch = _rms(ours[0], r), _rms(theirs, r)
            print(f"{kind} 24 steps {name}: rms ours {e_ours:.3e} torch {e_torch:.3e}")
            assert e_ours <= 2 * e_torch, (kind, name, e_ours, e_torch)


@pytest.mark.parametrize("kind", ["lstm", "gru"])
def test_first_widths_keep_the_first_entry(cuda_device, kind, monkeypatch):
    """At a width the first entry takes (48) the wrapper launches the first entry, once, and returns its bits."""
    from rsl_rl_amd import _lib, kernels
    dev, M, D = cuda_device, 64, 48
    p = Problem(kind, D, M, dev, 5)
    L = _lib.lib()
    calls = {}

    def spy(name):
        real = getattr(L, name)

        def counted(*a):
            calls[name] = calls.get(name, 0) + 1
            return real(*a)

        monkeypatch.setattr(L, name, counted, raising=False)

    for name in ("cell", "cell_anyd", "prepare_image", "prepare_image_anyd"):
        spy(f"rslrl_{kind}_{name}")
    with torch.no_grad():
        image = (kernels.lstm_image if kind == "lstm" else kernels.gru_image)(p.rnn.weight_ih_l0, p.rnn.weight_hh_l0)
        assert torch.equal(image, p.ops[0])
        out = p.step(True)
    assert calls == {f"rslrl_{kind}_cell": 1, f"rslrl_{kind}_prepare_image": 1}
    monkeypatch.undo()
    # the first entry called directly
    x, b_ih, b_hh = p.x, p.ops[1], p.ops[2]
    direct = torch.empty(2, M, H, device=dev)
    if kind == "lstm":
        a = _lib.LstmCell(x.data_ptr(), p.state[0].data_ptr(), p.state[1].data_ptr(), image.data_ptr(), b_ih.data_ptr(),
                          b_hh.data_ptr(), direct[0].data_ptr(), direct[1].data_ptr(), D, H, 1, 0)
        assert L.rslrl_lstm_cell(ctypes.byref(a), M, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
        assert torch.equal(out[0], direct[0]) and torch.equal(out[1], direct[1])
    else:
        a = _lib.GruCell(x.data_ptr(), p.state[0].data_ptr(), image.data_ptr(), b_ih.data_ptr(), b_hh.data_ptr(),
                         direct[0].data_ptr(), D, H, 1, 0)
        assert L.rslrl_gru_cell(ctypes.byref(a), M, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
        assert torch.equal(out[0], direct[0])
    # and at that width the new entry gives the same bytes: its image and its kernel
    entry = getattr(L, f"rslrl_{kind}_cell_anyd")
    again = torch.empty(2, M, H, device=dev)
    if kind == "lstm":
        a.h_out, a.c_out = again[0].data_ptr(), again[1].data_ptr()
    else:
        a.h_out = again[0].data_ptr()
    assert entry(ctypes.byref(a), M, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
    n = 2 if kind == "lstm" else 1
    assert torch.equal(again[:n], direct[:n])


@pytest.mark.parametrize("D", [40, 45, 235, 260, 1021])
def test_gate_weight_gradient_forms(cuda_device, D):
    """fused_mlp.gate_wgrad_x (dW_ih and the bias gradient of a gate block) at every form x's width selects, against
    the fp64 product: x6 arithmetic is fp32-faithful, so the error stays within a few fp32 roundings of the 512-term
    sums (5e-6 of the largest entry allows ~ 4 sqrt(512) ulp)."""
    from rsl_rl_amd.networks import fused_mlp
    dev, rows = cuda_device, 512
    g = torch.Generator().manual_seed(D)
    dzs = [torch.randn(rows, H, generator=g).to(dev) for _ in range(2)]
    xs = [torch.randn(rows, D, generator=g).to(dev) for _ in range(2)]
    for (dw, db), dz, x in zip(fused_mlp.gate_wgrad_x(dzs, xs), dzs, xs):
        ref = dz.double().t() @ x.double()
        assert dw.shape == (H, D) and db.shape == (H,)
        assert (dw.double() - ref).abs().max() <= 5e-6 * ref.abs().max()
        assert (db.double() - dz.double().sum(0)).abs().max() <= 5e-6 * dz.double().sum(0).abs().max()
    (dw, db), = fused_mlp.gate_wgrad_x(dzs[:1], xs[:1])
    assert (dw.double() - dzs[0].double().t() @ xs[0].double()).abs().max() <= 5e-6 * ref.abs().max()
