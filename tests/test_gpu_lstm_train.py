"""The training form of the fused LSTM step and its reverse step (csrc/lstm_cell.hip: rslrl_lstm_cell_train,
rslrl_lstm_cell_bwd) at M 64 and 192, D 16, 48 and 256.

Forward: h' and c' bit-equal to rslrl_lstm_cell on rows zeroed beforehand; repeated calls bit-equal; unsupported shapes
refused with the outputs untouched.  The stored gates: "within one fp32 rounding of the fp64 formulas" cannot be
checked as worded, because the formulas' argument -- the pre-activations the kernel accumulated -- is not an output.
Two checks stand in for it: c' and h' recomputed in fp64 from the stored gates agree with the stored c' and h' to fp32
rounding (2^-22: the gates' rounding and the result's), which pins every stored gate to the value the update used; and
against the fp64 formulas evaluated from the inputs the gates' RMS error is at most twice that of torch's own fp32
evaluation on the device, which bounds the pre-activations' error by the criterion of the other tests.
Backward: against an fp64 autograd evaluation of the cell's formulas; the yardstick is torch's fp32 autograd of the
same step on the same device, and the RMS error of dG, dc_prev (and with them the recurrent term) may be twice the
yardstick's -- the criterion of test_gpu_lstm_cell.py and test_gpu_fused_mlp.py.  Rows reset after the step pass
exactly nothing from the next step.  A three-step chain with resets checks dW_ih, dW_hh, db and the gradient into the
first state (dc from the last reverse launch; dh formed from that launch's dG_0, since it would be the recurrent term
of one more launch, which no window runs: the chain is cut where a window starts) against nn.LSTM in double."""

import pytest
import torch

from rsl_rl_amd import _lib, kernels
from rsl_rl_amd.networks import fused_mlp

pytestmark = pytest.mark.gpu
H = 256


def rms(a, b):
    return (a.double() - b.double()).pow(2).mean().sqrt().item()


def _resets(M, dev, gen):
    """uint8 [M]: random 30 %; at M 192 the first 64-row tile fully reset and the second without a reset."""
    r = (torch.rand(M, device=dev, generator=gen) < 0.3).to(torch.uint8)
    if M >= 192:
        r[:64] = 1
        r[64:128] = 0
    return r


def _weights(D, dev, gen):
    k = 1.0 / 16
    mk = lambda *s: (torch.rand(*s, device=dev, generator=gen) * 2 - 1) * k  # noqa: E731
    return mk(4 * H, D), mk(4 * H, H), mk(4 * H), mk(4 * H)


def _gates64(x, h, c, w_ih, w_hh, b_ih, b_hh, dtype):
    z = x.to(dtype) @ w_ih.to(dtype).t() + b_ih.to(dtype) + h.to(dtype) @ w_hh.to(dtype).t() + b_hh.to(dtype)
    i, f, g, o = z.chunk(4, dim=1)
    return torch.sigmoid(i), torch.sigmoid(f), torch.tanh(g), torch.sigmoid(o)


@pytest.mark.parametrize("D", [16, 48, 256])
@pytest.mark.parametrize("M", [64, 192])
def test_train_cell_against_the_cell(M, D, cuda_device):
    gen = torch.Generator(device=cuda_device).manual_seed(M + D)
    rn = lambda *s: torch.randn(*s, device=cuda_device, generator=gen)  # noqa: E731
    w_ih, w_hh, b_ih, b_hh = _weights(D, cuda_device, gen)
    image = kernels.lstm_image(w_ih, w_hh)
    x, h, c = rn(M, D), rn(M, H) * 0.5, rn(M, H) * 0.5
    reset = _resets(M, cuda_device, gen)
    keep = (reset == 0).view(M, 1)
    h0, c0 = h * keep, c * keep
    ref_h, ref_c = kernels.lstm_cell(x, (h0, c0), image, b_ih, b_hh)

    def run(state, rst):
        ho, co = torch.empty(M, H, device=cuda_device), torch.empty(M, H, device=cuda_device)
        ga = torch.empty(4, 3, M, H, device=cuda_device)  # a window buffer: this step's gates are a strided view
        kernels.lstm_cell_train(x, state, image, b_ih, b_hh, rst, ho, co, ga[:, 1])
        return ho, co, ga[:, 1].clone()

    ho, co, ga = run((h, c), reset)
    assert torch.equal(ho, ref_h) and torch.equal(co, ref_c)
    ho2, co2, ga2 = run((h, c), reset)
    assert torch.equal(ho, ho2) and torch.equal(co, co2) and torch.equal(ga, ga2)
    # no reset vector and no state at all
    hn, cn, _ = run((h0, c0), None)
    assert torch.equal(hn, ref_h) and torch.equal(cn, ref_c)
    rz_h, rz_c = kernels.lstm_cell(x, None, image, b_ih, b_hh)
    hz, cz, _ = run(None, reset)
    assert torch.equal(hz, rz_h) and torch.equal(cz, rz_c)
    # the stored gates reproduce c' and h' to fp32 rounding ...
    i, f, g, o = (t.double() for t in ga)
    c64 = f * c0.double() + i * g
    assert (co.double() - c64).abs().max() <= 2.0 ** -22 * (1 + c64.abs().max())
    assert (ho.double() - o * torch.tanh(co.double())).abs().max() <= 2.0 ** -22
    # ... and are the fp64 formulas' within twice torch's own fp32 evaluation
    ref64 = torch.stack(_gates64(x, h0, c0, w_ih, w_hh, b_ih, b_hh, torch.float64))
    ref32 = torch.stack(_gates64(x, h0, c0, w_ih, w_hh, b_ih, b_hh, torch.float32))
    ours, yard = rms(ga, ref64), rms(ref32, ref64)
    print(f"M {M} D {D}: gates rms err {ours:.2e}, torch fp32 {yard:.2e}")
    assert ours <= 2 * yard


def test_entry_points_refuse_other_shapes(cuda_device):
    gen = torch.Generator(device=cuda_device).manual_seed(1)
    w_ih, w_hh, b_ih, b_hh = _weights(48, cuda_device, gen)
    image = kernels.lstm_image(w_ih, w_hh)
    M = 100  # not a multiple of 64
    x = torch.randn(M, 48, device=cuda_device)
    ho, co = torch.full((M, H), 7.0, device=cuda_device), torch.full((M, H), 7.0, device=cuda_device)
    ga = torch.full((4, M, H), 7.0, device=cuda_device)
    with pytest.raises(_lib.RslrlError):
        kernels.lstm_cell_train(x, None, image, b_ih, b_hh, None, ho, co, ga)
    dg, dcp = torch.full((4, M, H), 7.0, device=cuda_device), torch.full((M, H), 7.0, device=cuda_device)
    with pytest.raises(_lib.RslrlError):
        kernels.lstm_cell_bwd(ho, ga, co, None, None, None, None, None, None, dg, dcp)
    torch.cuda.synchronize()
    for t in (ho, co, ga, dg, dcp):
        assert (t == 7.0).all()


def _bwd_case(M, cuda_device, gen, with_next, with_prev):
    rn = lambda *s: torch.randn(*s, device=cuda_device, generator=gen)  # noqa: E731
    z = rn(4, M, H)
    c_prev = rn(M, H) * 0.7 if with_prev else None
    reset_cur = _resets(M, cuda_device, gen) if with_prev else None
    reset_next = _resets(M, cuda_device, gen).flip(0) if with_next else None
    dh, dg_next, dc_next = rn(M, H), (rn(4, M, H) * 0.2 if with_next else None), (rn(M, H) if with_next else None)
    w_hh = (torch.rand(4 * H, H, device=cuda_device, generator=gen) * 2 - 1) / 16
    return z, c_prev, reset_cur, reset_next, dh, dg_next, dc_next, w_hh


def _bwd_reference(z, c_prev, reset_cur, reset_next, dh, dg_next, dc_next, w_hh, dtype):
    """(dG [4, M, 256], dc_prev, the recurrent term) by autograd of the cell's formulas in `dtype`."""
    M = z.shape[1]
    zz = z.to(dtype).clone().requires_grad_(True)
    cp = (torch.zeros(M, H, device=z.device) if c_prev is None else c_prev).to(dtype)
    if reset_cur is not None:
        cp = cp * (reset_cur == 0).view(M, 1)
    cp = cp.clone().requires_grad_(True)
    i, f, g, o = torch.sigmoid(zz[0]), torch.sigmoid(zz[1]), torch.tanh(zz[2]), torch.sigmoid(zz[3])
    c = f * cp + i * g
    h = o * torch.tanh(c)
    rec = torch.zeros(M, H, device=z.device, dtype=dtype)
    dc_in = torch.zeros(M, H, device=z.device, dtype=dtype)
    if dg_next is not None:
        live = (reset_next == 0).view(M, 1)
        rec = (dg_next.to(dtype).permute(1, 0, 2).reshape(M, 4 * H) @ w_hh.to(dtype)) * live
        dc_in = dc_next.to(dtype) * live
    ((h * (dh.to(dtype) + rec)).sum() + (c * dc_in).sum()).backward()
    return zz.grad, cp.grad, rec


@pytest.mark.parametrize("with_next,with_prev", [(True, True), (False, True), (True, False), (False, False)],
                         ids=["chained", "last_step", "first_step", "single"])
@pytest.mark.parametrize("M", [64, 192])
def test_backward_step_against_autograd(M, with_next, with_prev, cuda_device):
    gen = torch.Generator(device=cuda_device).manual_seed(10 * M + 2 * with_next + with_prev)
    case = _bwd_case(M, cuda_device, gen, with_next, with_prev)
    z, c_prev, reset_cur, reset_next, dh, dg_next, dc_next, w_hh = case
    # what the training cell would have stored: the activated gates and c' as fp32 roundings of the fp64 values
    zd = z.double()
    acts = torch.stack([torch.sigmoid(zd[0]), torch.sigmoid(zd[1]), torch.tanh(zd[2]), torch.sigmoid(zd[3])])
    cp = torch.zeros(M, H, device=cuda_device) if c_prev is None else c_prev
    if reset_cur is not None:
        cp = cp * (reset_cur == 0).view(M, 1)
    gates = torch.empty(4, 2, M, H, device=cuda_device)  # window buffers: gates and dG share their gate stride
    gates[:, 0] = acts.float()
    gates = gates[:, 0]
    c_out = (gates[1].double() * cp.double() + gates[0].double() * gates[2].double()).float()
    whh_t = kernels.lstm_whh_t_image(w_hh) if with_next else None

    def run(dgn, dcn, rstn):
        dg = torch.empty(4, 2, M, H, device=cuda_device)  # a window buffer, this step at index 0
        dcp = torch.empty(M, H, device=cuda_device)
        nxt = None
        if dgn is not None:
            nxt = torch.empty(4, 2, M, H, device=cuda_device)
            nxt[:, 1] = dgn
            nxt = nxt[:, 1]
        kernels.lstm_cell_bwd(dh, gates, c_out, c_prev, reset_cur, nxt, dcn, rstn, whh_t, dg[:, 0], dcp)
        return dg[:, 0].clone(), dcp

    dg, dcp = run(dg_next, dc_next, reset_next)
    dg2, dcp2 = run(dg_next, dc_next, reset_next)
    assert torch.equal(dg, dg2) and torch.equal(dcp, dcp2)
    ref_dg, ref_dcp, ref_rec = _bwd_reference(*case, torch.float64)
    y_dg, y_dcp, y_rec = _bwd_reference(*case, torch.float32)
    for name, ours, ref, yard in (("dG", dg, ref_dg, y_dg), ("dc_prev", dcp, ref_dcp, y_dcp)):
        e, y = rms(ours, ref), rms(yard, ref)
        print(f"M {M} {name}: rms err {e:.2e}, torch fp32 autograd {y:.2e}")
        assert e <= 2 * y, (name, e, y)
    if with_next:
        # the recurrent term alone: dG_o = (dh + rec) * tanh(c') * o (1 - o), so it is read back from two calls
        base_dg, base_dcp = run(None, None, None)
        rows = reset_next != 0
        assert rows.any() and not rows.all()
        # rows reset after this step pass exactly nothing from the next one
        assert torch.equal(dg[:, rows], base_dg[:, rows]) and torch.equal(dcp[rows], base_dcp[rows])
        assert not torch.equal(dg[:, ~rows], base_dg[:, ~rows])
        # the recurrent term alone, read back through dG_o = rec * tanh(c') * o (1 - o) of a call with dh = 0; the
        # same criterion as dG and dc_prev, the read-back's own rounding included in our side
        zero_dg = torch.empty(4, 2, M, H, device=cuda_device)[:, 0]
        kernels.lstm_cell_bwd(torch.zeros_like(dh), gates, c_out, c_prev, reset_cur, dg_next.contiguous(), None,
                              None, whh_t, zero_dg, torch.empty(M, H, device=cuda_device))
        t = torch.tanh(c_out.double()) * gates[3].double() * (1 - gates[3].double())
        ok = t.abs() > 0.05
        full = (dg_next.double().permute(1, 0, 2).reshape(M, 4 * H) @ w_hh.double())
        full32 = (dg_next.permute(1, 0, 2).reshape(M, 4 * H) @ w_hh).double()
        rec = (zero_dg[3].double() / t)[ok]
        e, y = rms(rec, full[ok]), rms(full32[ok], full[ok])
        print(f"M {M} recurrent term: rms err {e:.2e}, torch fp32 {y:.2e}")
        assert e <= 2 * y, (e, y)


def _chain_reference(x, h0, c0, resets, wts, w_out, dtype, dev):
    """Three nn.LSTM steps in `dtype` with the resets between them; loss = sum_t <h_t, w_out_t>."""
    w_ih, w_hh, b_ih, b_hh = wts
    D = x.shape[2]
    rnn = torch.nn.LSTM(D, H, 1).to(dev).to(dtype)
    with torch.no_grad():
        rnn.weight_ih_l0.copy_(w_ih)
        rnn.weight_hh_l0.copy_(w_hh)
        rnn.bias_ih_l0.copy_(b_ih)
        rnn.bias_hh_l0.copy_(b_hh)
    c_first = c0.to(dtype).clone().requires_grad_(True)
    h_first = h0.to(dtype).clone().requires_grad_(True)
    h, c = h_first.unsqueeze(0), c_first.unsqueeze(0)
    loss = 0
    for t in range(x.shape[0]):
        if resets[t] is not None:
            keep = (resets[t] == 0).view(1, -1, 1)
            h, c = h * keep, c * keep
        out, (h, c) = rnn(x[t].to(dtype).unsqueeze(0), (h, c))
        loss = loss + (out[0] * w_out[t].to(dtype)).sum()
    loss.backward()
    return (rnn.weight_ih_l0.grad, rnn.weight_hh_l0.grad, rnn.bias_ih_l0.grad, c_first.grad, h_first.grad)


def test_three_step_chain_against_nn_lstm(cuda_device):
    M, D, S = 192, 48, 3
    gen = torch.Generator(device=cuda_device).manual_seed(5)
    rn = lambda *s: torch.randn(*s, device=cuda_device, generator=gen)  # noqa: E731
    wts = _weights(D, cuda_device, gen)
    w_ih, w_hh, b_ih, b_hh = wts
    x, h0, c0, w_out = rn(S, M, D), rn(M, H) * 0.5, rn(M, H) * 0.5, rn(S, M, H)
    resets = [None, _resets(M, cuda_device, gen), _resets(M, cuda_device, gen).flip(0)]
    image, whh_t = kernels.lstm_image(w_ih, w_hh), kernels.lstm_whh_t_image(w_hh)
    f32 = dict(device=cuda_device)
    hout, cout, hin = torch.empty(S, M, H, **f32), torch.empty(S, M, H, **f32), torch.empty(S, M, H, **f32)
    gates, dg = torch.empty(4, S, M, H, **f32), torch.empty(4, S, M, H, **f32)
    dc = [torch.empty(M, H, **f32) for _ in range(2)]
    state, tape = (h0, c0), []
    for t in range(S):
        hin[t] = state[0] if resets[t] is None else state[0] * (resets[t] == 0).view(M, 1)
        kernels.lstm_cell_train(x[t], state, image, b_ih, b_hh, resets[t], hout[t], cout[t], gates[:, t])
        tape.append((state[1], resets[t]))
        state = (hout[t], cout[t])
    for t in range(S - 1, -1, -1):
        nxt = t + 1 < S
        kernels.lstm_cell_bwd(w_out[t].contiguous(), gates[:, t], cout[t], tape[t][0], tape[t][1],
                              dg[:, t + 1] if nxt else None, dc[(t + 1) & 1] if nxt else None,
                              tape[t + 1][1] if nxt else None, whh_t, dg[:, t], dc[t & 1])
    dw_ih, dw_hh, db = [], [], []
    for g in range(4):
        dz = dg[g].view(S * M, H)
        w, b = fused_mlp.linear_wgrad(dz, x.view(S * M, D), bias_side=1)
        dw_ih.append(w)
        db.append(b)
        dw_hh.append(fused_mlp.linear_wgrad(dz, hin.view(S * M, H)))
    # the first state's dh is the recurrent term of step 0's gate gradient (no reset in front of step 0); no launch of
    # a window computes it, so it is formed here from the kernel's dG_0 -- which checks that gradient element by element
    dh0 = dg[:, 0].permute(1, 0, 2).reshape(M, 4 * H).double() @ w_hh.double()
    ours = (torch.cat(dw_ih), torch.cat(dw_hh), torch.cat(db), dc[0], dh0)
    ref = _chain_reference(x, h0, c0, resets, wts, w_out, torch.float64, cuda_device)
    yard = _chain_reference(x, h0, c0, resets, wts, w_out, torch.float32, cuda_device)
    for name, o, r, y in zip(("dW_ih", "dW_hh", "db", "dc_0", "dh_0"), ours, ref, yard):
        e, ye = rms(o, r), rms(y, r)
        print(f"chain {name}: rms err {e:.2e}, fp32 nn.LSTM autograd {ye:.2e}, scale {r.abs().max().item():.2e}")
        assert e <= 2 * ye, (name, e, ye)
