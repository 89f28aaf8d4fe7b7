"""The fused LSTM / GRU cells at hidden size 512 (the `_h` entry points), both kinds, rows 64 and 192.

Bit equality with the 256 kernels by zero embedding.  The 512 kernels keep lc_mfma's per-chunk summation and the chunk
order (x chunks, then the h chunks ascending; in the reverse step gate-major, chunks ascending), a chunk whose weights
are zero adds an exact +0, and the pointwise part is register-local.  So with W_hh's columns 256..511 zero the hidden
columns [0, 256) of every output carry the bits of the 256 kernels on the sub-problem (rows 512 g + j, j < 256, of W_ih,
W_hh[:, :256] and the biases, the states' first 256 columns), and with columns 0..255 zero the columns [256, 512) those
of the upper sub-problem; for the reverse step the same with the corresponding 256 rows per gate block of W_hh zero.
The dead half of every state is random but finite.  Every output lies between NaN guard bands.

Dense weights: h' and c' against the fp64 formulas within twice the RMS error of torch's fp32 nn.LSTM / nn.GRU step on
the same device (the criterion of test_gpu_lstm_cell.py and test_gpu_gru_cell.py), 24 chained steps through Memory, and a
train x 4 / bwd x 4 sequence with the gate blocks' weight gradients against fp64 autograd on the CPU, per tensor within
twice torch's fp32 autograd on the device (the pattern of test_gpu_lstm_train.py).  The reverse step forms no gradient
w.r.t. the observations, so there is no dx to compare."""

import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

H, HS = 512, 256
GUARD = 64
KINDS = ["lstm", "gru"]


def _cell(kind):
    from rsl_rl_amd import kernels
    return kernels.LSTM if kind == "lstm" else kernels.GRU


class Guarded:
    """Output tensors inside NaN buffers: NaN-filled themselves, with GUARD NaN floats on either side."""

    def __init__(self, dev):
        self.dev, self.bufs = dev, []

    def new(self, *shape):
        n = 1
        for s in shape:
            n *= s
        buf = torch.full((n + 2 * GUARD,), float("nan"), device=self.dev)
        self.bufs.append((buf, n))
        return buf[GUARD:GUARD + n].view(*shape)

    def intact(self):
        return all(bool(torch.isnan(b[:GUARD]).all()) and bool(torch.isnan(b[GUARD + n:]).all()) for b, n in self.bufs)


def _weights(blocks, D, hidden, gen, dev):
    k = hidden ** -0.5
    mk = lambda *s: ((torch.rand(*s, generator=gen) * 2 - 1) * k).to(dev)  # noqa: E731
    return mk(blocks * hidden, D), mk(blocks * hidden, hidden), mk(blocks * hidden), mk(blocks * hidden)


def _half_rows(blocks, lo, dev):
    return torch.cat([torch.arange(g * H + lo, g * H + lo + HS) for g in range(blocks)]).to(dev)


def _sub(t, lo):
    """columns [lo, lo + 256) of the last dimension as a contiguous tensor; None stays"""
    return None if t is None else t[..., lo:lo + HS].contiguous()


def _subs(ts, lo):
    return None if ts is None else tuple(_sub(t, lo) for t in ts)


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def _finite(ts):
    return all(bool(torch.isfinite(t).all()) for t in ts)


class Embedded:
    """One memory at hidden size 512 whose W_hh couples only one half of h to itself, and the 256 problem of that half."""

    def __init__(self, kind, D, M, half, dev, seed, reverse=False):
        self.cell, self.M, self.D, self.dev = _cell(kind), M, D, dev
        self.lo = lo = 0 if half == "low" else HS
        self.gen = gen = torch.Generator().manual_seed(1000 * seed + 10 * D + M + lo)
        blocks = self.cell.blocks
        w_ih, w_hh, b_ih, b_hh = _weights(blocks, D, H, gen, dev)
        dead = slice(HS, H) if half == "low" else slice(0, HS)
        if reverse:  # the reverse step reads W_hh^T: the dead half's rows of every gate block
            w_hh.view(blocks, H, H)[:, dead, :] = 0
        else:
            w_hh[:, dead] = 0
        rows = _half_rows(blocks, lo, dev)
        self.w = (w_ih, w_hh, b_ih, b_hh)
        self.w_sub = (w_ih[rows].contiguous(), w_hh[rows][:, lo:lo + HS].contiguous(), b_ih[rows].contiguous(),
                      b_hh[rows].contiguous())
        self.ops = (self.cell.image(w_ih, w_hh), b_ih, b_hh)
        self.ops_sub = (self.cell.image(*self.w_sub[:2]), self.w_sub[2], self.w_sub[3])
        assert self.ops[0].numel() * 4 == blocks * 2 * (_bimage(D) + _bimage(H))
        n = self.cell.n_state
        self.x = self.rn(M, D)
        self.state = tuple(0.5 * self.rn(M, H) for _ in range(n))
        self.restart = tuple(self.rn(M, H) for _ in range(n))
        reset = torch.rand(M, generator=gen) < 0.2
        reset[3::32] = True  # a reset row in every 32-row block
        reset[4::32] = False
        self.reset = reset.to(torch.uint8).to(dev)

    def rn(self, *s):
        return torch.randn(*s, generator=self.gen).to(self.dev)

    def train(self, state, reset, restart, width, x=None):
        """One training step at `width` (512: the embedded problem, 256: its live half): (h', [c',] gates, h as
        consumed) and the guard."""
        lo, M, g = self.lo, self.M, Guarded(self.dev)
        n = self.cell.n_state
        out, gates, hin = tuple(g.new(M, width) for _ in range(n)), g.new(4, M, width), g.new(M, width)
        if width == HS:
            state, restart, ops = _subs(state, lo), _subs(restart, lo), self.ops_sub
        else:
            ops = self.ops
        step = (state, out, reset, restart, hin)
        self.cell.train(self.cell.train_operands(self.x if x is None else x, *ops, gates, step, hin))
        return out + (gates, hin), g


def _bimage(depth):
    from rsl_rl_amd import _lib
    return _lib.lib().rslrl_linear_bimage_bytes(depth)


def _live(ts, lo):
    return tuple(t[..., lo:lo + HS] for t in ts)


@pytest.mark.parametrize("half", ["low", "high"])
@pytest.mark.parametrize("M", [64, 192])
@pytest.mark.parametrize("D", [48, 45])
@pytest.mark.parametrize("kind", KINDS)
def test_forward_forms_carry_the_256_kernels_bits(cuda_device, kind, D, M, half):
    p = Embedded(kind, D, M, half, cuda_device, 1)
    q = Embedded(kind, 45 if D == 48 else 48, M, half, cuda_device, 2)  # the pair's other problem: the other load form
    cell, lo = p.cell, p.lo
    with torch.no_grad():
        # the rollout form, with and without a state
        for state in (p.state, None):
            new = cell.step(p.x, state, *p.ops)
            assert all(t.shape == (M, H) for t in new) and _finite(new)
            assert _same(_live(new, lo), cell.step(p.x, _subs(state, lo), *p.ops_sub)), (kind, D, M, half, "rollout")
            assert _same(cell.step(p.x, state, *p.ops), new)  # a repeated call
            qs = q.state if state is not None else None
            both = cell.step_pair(p.x, state, *p.ops, q.x, qs, *q.ops)
            assert _same(both[0], new) and _same(both[1], cell.step(q.x, qs, *q.ops)), (kind, D, M, half, "pair")
        # the training form: the first step without a state, reset rows that restart from a saved state, reset rows
        # that restart from zero, and a state without resets
        for state, reset, restart in ((None, None, None), (p.state, p.reset, p.restart), (p.state, p.reset, None),
                                      (p.state, None, None), (None, p.reset, p.restart)):
            new, guard = p.train(state, reset, restart, H)
            first, guard_s = p.train(state, reset, restart, HS)
            assert _finite(new) and guard.intact() and guard_s.intact()
            assert _same(_live(new, lo), first), (kind, D, M, half, "training form")
            again, _ = p.train(state, reset, restart, H)
            assert _same(again, new)
            # h' and c' are the rollout form's on the state as consumed, which is what h_in_out holds
            hin = new[-1]
            rst = reset.bool() if reset is not None else torch.zeros(M, dtype=torch.bool, device=cuda_device)
            want = torch.zeros(M, H, device=cuda_device) if state is None else state[0].clone()
            want[rst] = restart[0][rst] if restart is not None else 0.0
            assert torch.equal(hin, want)
            consumed = [want]
            if cell.n_state == 2:
                c_in = torch.zeros(M, H, device=cuda_device) if state is None else state[1].clone()
                c_in[rst] = restart[1][rst] if restart is not None else 0.0
                consumed.append(c_in)
            assert _same(new[:cell.n_state], cell.step(p.x, tuple(consumed), *p.ops))
        # the pair form of the training step: two single launches, bit for bit
        gp, gq = Guarded(cuda_device), Guarded(cuda_device)
        n = cell.n_state
        outs = []
        operands = []
        for pr, g in ((p, gp), (q, gq)):
            out, gates, hin = tuple(g.new(M, H) for _ in range(n)), g.new(4, M, H), g.new(M, H)
            outs.append(out + (gates, hin))
            operands.append(cell.train_operands(pr.x, *pr.ops, gates, (pr.state, out, pr.reset, pr.restart, hin), hin))
        cell.train_pair(*operands)
        assert gp.intact() and gq.intact()
        assert _same(outs[0], p.train(p.state, p.reset, p.restart, H)[0])
        assert _same(outs[1], q.train(q.state, q.reset, q.restart, H)[0])


def _bwd(p, width, tape, dh, nxt, carry_next, reset_next, reset_cur, restart, c_prev_none=False):
    """One reverse step at `width`: (dg, carry out) and the guard.  tape: (state, out, gates, hin) of a training step at
    512; nxt: dg_next or None."""
    cell, lo, M, g = p.cell, p.lo, p.M, Guarded(p.dev)
    state, out, gates, hin = tape
    if c_prev_none:
        state = None
    w_hh = p.w[1]
    if width == HS:
        state, out, restart = _subs(state, lo), _subs(out, lo), _subs(restart, lo)
        gates, hin, dh, nxt, carry_next = (_sub(t, lo) for t in (gates, hin, dh, nxt, carry_next))
        w_hh = p.w_sub[1]
    whh_t = cell.whh_t_image(w_hh) if nxt is not None else None
    dg, carry = g.new(4, M, width), g.new(M, width)
    step = (state, out, reset_cur, restart, hin)
    cell.bwd(cell.bwd_operands(dh.contiguous(), gates, step, nxt, carry_next, reset_next, whh_t, dg, carry))
    return (dg, carry), g


@pytest.mark.parametrize("half", ["low", "high"])
@pytest.mark.parametrize("M", [64, 192])
@pytest.mark.parametrize("kind", KINDS)
def test_reverse_step_carries_the_256_kernels_bits(cuda_device, kind, M, half):
    p = Embedded(kind, 48, M, half, cuda_device, 3, reverse=True)
    q = Embedded(kind, 48, M, half, cuda_device, 4, reverse=True)
    cell, lo = p.cell, p.lo
    with torch.no_grad():
        cases = []
        for pr in (p, q):
            new, _ = pr.train(pr.state, pr.reset, pr.restart, H)
            n = cell.n_state
            tape = (pr.state, new[:n], new[n], new[n + 1])
            dh, nxt, carry_next = pr.rn(M, H), 0.2 * pr.rn(4, M, H), pr.rn(M, H)
            reset_next = pr.reset.flip(0).contiguous()
            cases.append((tape, dh, nxt, carry_next, reset_next))
        tape, dh, nxt, carry_next, reset_next = cases[0]
        # chained with resets on both sides and restart states; chained without resets; the last step of a chain;
        # the first step of a sequence (no entering c)
        for args in ((nxt, carry_next, reset_next, p.reset, p.restart), (nxt, carry_next, None, None, None),
                     (None, None, None, p.reset, None), (nxt, carry_next, reset_next, None, None, True)):
            new, guard = _bwd(p, H, tape, dh, *args)
            first, guard_s = _bwd(p, HS, tape, dh, *args)
            assert _finite(new) and guard.intact() and guard_s.intact()
            assert _same(_live(new, lo), first), (kind, M, half, "reverse step")
            assert _same(_bwd(p, H, tape, dh, *args)[0], new)  # a repeated call
        # rows reset after the step take nothing from the next one
        chained, _ = _bwd(p, H, tape, dh, nxt, carry_next, reset_next, p.reset, p.restart)
        last, _ = _bwd(p, H, tape, dh, None, None, None, p.reset, p.restart)
        rows = reset_next.bool()
        assert rows.any() and not rows.all()
        assert torch.equal(chained[0][:, rows], last[0][:, rows]) and not torch.equal(chained[0][:, ~rows], last[0][:, ~rows])
        # the pair form: two single launches, bit for bit
        guards, outs, operands = [], [], []
        for pr, (tp, d, nx, cn, rn_) in zip((p, q), cases):
            g = Guarded(cuda_device)
            dg, carry = g.new(4, M, H), g.new(M, H)
            step = (tp[0], tp[1], pr.reset, pr.restart, tp[3])
            operands.append(cell.bwd_operands(d, tp[2], step, nx, cn, rn_, cell.whh_t_image(pr.w[1]), dg, carry))
            guards.append(g)
            outs.append((dg, carry))
        cell.bwd_pair(*operands)
        assert all(g.intact() for g in guards)
        for pr, (tp, d, nx, cn, rn_), o in zip((p, q), cases, outs):
            assert _same(o, _bwd(pr, H, tp, d, nx, cn, rn_, pr.reset, pr.restart)[0])


# ---------------------------------------------------------------------------------------------------------------------
# dense weights


def _rnn(kind, D, dev, seed, dtype=torch.float32):
    torch.manual_seed(seed)
    return (nn.LSTM if kind == "lstm" else nn.GRU)(D, H).to(device=dev, dtype=dtype)


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
    return (a.double() - ref.double()).square().mean().sqrt().item()


@pytest.mark.parametrize("M", [64, 192])
@pytest.mark.parametrize("D", [48, 45, 235])
@pytest.mark.parametrize("kind", KINDS)
def test_dense_step_matches_fp64_within_twice_torch(cuda_device, kind, D, M):
    cell = _cell(kind)
    rnn = _rnn(kind, D, cuda_device, 5)
    gen = torch.Generator().manual_seed(D + M)
    x = torch.randn(M, D, generator=gen).to(cuda_device)
    state = tuple((0.5 if i == 0 else 1.0) * torch.randn(M, H, generator=gen).to(cuda_device) for i in range(cell.n_state))
    with torch.no_grad():
        ops = (cell.image(rnn.weight_ih_l0, rnn.weight_hh_l0), rnn.bias_ih_l0.detach(), rnn.bias_hh_l0.detach())
        for st in (None, state):
            ours, ref, tor = cell.step(x, st, *ops), _ref64(kind, rnn, x, st), _torch_step(kind, rnn, x, st)
            for name, o, t, r in zip(("h'", "c'"), ours, tor, ref):
                e_ours, e_torch = _rms(o, r), _rms(t, r)
                print(f"{kind} D {D} M {M} state {st is not None} {name}: rms ours {e_ours:.3e} torch {e_torch:.3e}")
                assert e_ours <= 2 * e_torch, (kind, D, M, st is not None, name, e_ours, e_torch)


@pytest.mark.parametrize("kind", KINDS)
def test_chained_steps_through_memory(cuda_device, kind):
    """24 chained steps through Memory at hidden size 512, rows reset in between."""
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
            assert mem.fused_cell(xs[t]) is _cell(kind)
            assert mem(xs[t]).shape == (1, M, H)
            ref = _ref64(kind, mem.rnn, xs[t], ref)
            tor = _torch_step(kind, mem.rnn, xs[t], tor)
            mem.reset(dones[t])
            mask = (dones[t] == 1).unsqueeze(1)
            ref = tuple(torch.where(mask, torch.zeros_like(s), s) for s in ref)
            tor = tuple(torch.where(mask, torch.zeros_like(s), s) for s in tor)
            states = mem.hidden_states if kind == "lstm" else (mem.hidden_states,)
            for s in states:
                assert s.shape == (1, M, H) and (s[0][dones[t] == 1] == 0.0).all()
        for name, ours, theirs, r in zip("hc", states, tor, ref):
            e_ours, e_torch = _rms(ours[0], r), _rms(theirs, r)
            print(f"{kind} 24 steps {name}: rms ours {e_ours:.3e} torch {e_torch:.3e}")
            assert e_ours <= 2 * e_torch, (kind, name, e_ours, e_torch)


def _autograd_chain(kind, rnn, xs, state0, resets, gs):
    """Gradients of sum_t <h_t, gs[t]> through T chained steps of nn.LSTM / nn.GRU in rnn's dtype and on its device; rows
    whose reset flag is set enter step t from zero."""
    dev, dt = rnn.weight_ih_l0.device, rnn.weight_ih_l0.dtype
    rnn.zero_grad()
    state = tuple(s.to(device=dev, dtype=dt).unsqueeze(0) for s in state0)
    loss = 0
    for t in range(xs.shape[0]):
        if t:
            keep = (resets[t] == 0).to(device=dev, dtype=dt).view(1, -1, 1)
            state = tuple(s * keep for s in state)
        out, new = rnn(xs[t].to(device=dev, dtype=dt).unsqueeze(0), state if kind == "lstm" else state[0])
        state = new if kind == "lstm" else (new,)
        loss = loss + (out[0] * gs[t].to(device=dev, dtype=dt)).sum()
    loss.backward()
    return [p.grad.detach().cpu().double() for p in (rnn.weight_ih_l0, rnn.weight_hh_l0, rnn.bias_ih_l0, rnn.bias_hh_l0)]


@pytest.mark.parametrize("D", [48, 45])
@pytest.mark.parametrize("kind", KINDS)
def test_sequence_gradients_against_fp64_autograd(cuda_device, kind, D):
    """train x 4, bwd x 4 and the gate blocks' weight gradients, the way ActorCriticRecurrent.train_forward /
    train_backward drive them, against fp64 autograd of the same chain on the CPU."""
    from rsl_rl_amd.networks import fused_mlp
    cell, dev, T, M = _cell(kind), cuda_device, 4, 64
    rnn = _rnn(kind, D, dev, 6)
    gen = torch.Generator().manual_seed(7 + D)
    rn = lambda *s: torch.randn(*s, generator=gen)  # noqa: E731
    xs, gs = rn(T, M, D), rn(T, M, H)
    state0 = tuple(0.5 * rn(M, H) for _ in range(cell.n_state))
    resets = (torch.rand(T, M, generator=gen) < 0.25).to(torch.uint8)
    resets[2, :8] = 1
    n = cell.n_state
    new = lambda *s: torch.full(s, float("nan"), device=dev)  # noqa: E731
    out, hin = tuple(new(T, M, H) for _ in range(n)), new(T, M, H)
    gates, dg, carry = new(4, T, M, H), new(4, T, M, H), new(2, M, H)
    x_d, g_d, r_d = xs.to(dev), gs.to(dev), resets.to(dev)
    with torch.no_grad():
        w_ih, w_hh = rnn.weight_ih_l0, rnn.weight_hh_l0
        image, whh_t = cell.image(w_ih, w_hh), cell.whh_t_image(w_hh)
        steps = []
        for t in range(T):
            step = (steps[-1][1] if t else tuple(s.to(dev) for s in state0), tuple(o[t] for o in out),
                    r_d[t] if t else None, None, hin[t])
            cell.train(cell.train_operands(x_d[t], image, rnn.bias_ih_l0, rnn.bias_hh_l0, gates[:, t], step, hin[t]))
            steps.append(step)
        for t in range(T - 1, -1, -1):
            nxt = steps[t + 1] if t < T - 1 else None
            cell.bwd(cell.bwd_operands(g_d[t], gates[:, t], steps[t], dg[:, t + 1] if nxt else None,
                                       carry[(t + 1) & 1] if nxt else None, nxt[2] if nxt else None, whh_t, dg[:, t],
                                       carry[t & 1]))
        params = (rnn.weight_ih_l0, rnn.weight_hh_l0, rnn.bias_ih_l0, rnn.bias_hh_l0)
        grads = [torch.full_like(p, float("nan")) for p in params]
        views = [g.view(cell.blocks, H, *p.shape[1:]) for g, p in zip(grads, params)]
        before = fused_mlp.wide_launches
        fused_mlp.GATE_WGRADS[cell.name]([dg.view(4, T * M, H)], [x_d.view(T * M, D)], [hin.view(T * M, H)], [views])
        assert fused_mlp.wide_launches > before  # the 512 x 512 blocks of dW_hh go through the wide form
    ref_rnn = _rnn(kind, D, "cpu", 6, torch.float64)
    ref = _autograd_chain(kind, ref_rnn, xs, state0, resets, gs)
    yard = _autograd_chain(kind, rnn, xs, state0, resets, gs)
    for name, ours, r, y in zip(("dW_ih", "dW_hh", "db_ih", "db_hh"), grads, ref, yard):
        e_ours, e_torch = _rms(ours.cpu(), r), _rms(y, r)
        print(f"{kind} D {D} {name}: rms ours {e_ours:.3e} torch fp32 autograd {e_torch:.3e}")
        assert torch.isfinite(ours).all() and e_ours <= 2 * e_torch, (kind, D, name, e_ours, e_torch)
