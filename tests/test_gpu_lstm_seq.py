"""ABI 27 of the fused LSTM step (csrc/lstm_cell.hip) at M 64 and 192, D 16, 48 and 256, with a row tile
where every row resets and one where none does (M 192): restart states in the training form and in the reverse step,
the stored state as consumed, the pair forms -- all bit for bit against calls on inputs merged beforehand or against
the single calls -- and a four-step sequence with restarts against an fp64 torch restatement, where the weight
gradients and the first state's dc may be off by twice the RMS error of the same restatement in fp32 on the device."""

from types import SimpleNamespace

import pytest
import torch

import recurrent_fused_fixtures as RFF
from rsl_rl_amd import kernels
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
    mk = lambda *s: (torch.rand(*s, device=dev, generator=gen) * 2 - 1) / 16  # noqa: E731
    return mk(4 * H, D), mk(4 * H, H), mk(4 * H), mk(4 * H)


def _train_case(M, D, dev, seed):
    gen = torch.Generator(device=dev).manual_seed(seed)
    rn = lambda *s: torch.randn(*s, device=dev, generator=gen)  # noqa: E731
    w_ih, w_hh, b_ih, b_hh = _weights(D, dev, gen)
    c = SimpleNamespace(M=M, D=D, x=rn(M, D), h=rn(M, H) * 0.5, c=rn(M, H) * 0.5, hr=rn(M, H) * 0.3, cr=rn(M, H) * 0.3,
                        reset=_resets(M, dev, gen), image=kernels.lstm_image(w_ih, w_hh), b_ih=b_ih, b_hh=b_hh)
    r = (c.reset != 0).view(M, 1)
    c.h_merged, c.c_merged = torch.where(r, c.hr, c.h), torch.where(r, c.cr, c.c)
    return c


def _train_args(c, restart=True, store=True):
    dev = c.x.device
    out = SimpleNamespace(h=torch.empty(c.M, H, device=dev), c=torch.empty(c.M, H, device=dev),
                          gates=torch.empty(4, 2, c.M, H, device=dev)[:, 1],
                          hin=torch.full((c.M, H), 7.0, device=dev) if store else None)
    args = dict(x=c.x, state=(c.h, c.c), image=c.image, b_ih=c.b_ih, b_hh=c.b_hh, reset=c.reset, h_out=out.h,
                c_out=out.c, gates=out.gates, h_restart=c.hr if restart else None,
                c_restart=c.cr if restart else None, h_in_out=out.hin)
    return args, out


@pytest.mark.parametrize("D", [16, 48, 256])
@pytest.mark.parametrize("M", [64, 192])
def test_training_cell_restarts_from_the_given_state(M, D, cuda_device):
    c = _train_case(M, D, cuda_device, 100 + M + D)
    assert c.reset.any() and not c.reset.all()
    ref_h, ref_c = kernels.lstm_cell(c.x, (c.h_merged, c.c_merged), c.image, c.b_ih, c.b_hh)
    args, out = _train_args(c)
    kernels.lstm_cell_train(**args)
    assert torch.equal(out.h, ref_h) and torch.equal(out.c, ref_c)
    # the stored state as consumed: dW_hh's operand
    assert torch.equal(out.hin, c.h_merged)
    # the gates of a call on the merged inputs
    plain = dict(args, state=(c.h_merged, c.c_merged), reset=None, h_restart=None, c_restart=None, h_in_out=None,
                 h_out=torch.empty_like(out.h), c_out=torch.empty_like(out.c), gates=torch.empty(4, M, H,
                                                                                                  device=cuda_device))
    kernels.lstm_cell_train(**plain)
    assert torch.equal(out.gates, plain["gates"]) and torch.equal(plain["h_out"], ref_h)
    # no state at all: the reset rows restart, the others read zero
    r = (c.reset != 0).view(M, 1)
    zh, zc = kernels.lstm_cell(c.x, (c.hr * r, c.cr * r), c.image, c.b_ih, c.b_hh)
    args0, out0 = _train_args(c)
    kernels.lstm_cell_train(**dict(args0, state=None))
    assert torch.equal(out0.h, zh) and torch.equal(out0.c, zc) and torch.equal(out0.hin, c.hr * r)


@pytest.mark.parametrize("D", [16, 48, 256])
@pytest.mark.parametrize("M", [64, 192])
def test_new_fields_null_keep_the_abi_26_outputs(M, D, cuda_device):
    """Without the ABI 27 operands a reset row reads zero, as before: h' and c' are rslrl_lstm_cell's (whose kernel is
    untouched) on rows zeroed beforehand, and storing h_in_out changes none of the other outputs."""
    c = _train_case(M, D, cuda_device, 200 + M + D)
    keep = (c.reset == 0).view(M, 1)
    ref_h, ref_c = kernels.lstm_cell(c.x, (c.h * keep, c.c * keep), c.image, c.b_ih, c.b_hh)
    args, out = _train_args(c, restart=False, store=False)
    kernels.lstm_cell_train(*[args[k] for k in ("x", "state", "image", "b_ih", "b_hh", "reset", "h_out", "c_out",
                                                "gates")])  # the ABI 26 call, positionally
    assert torch.equal(out.h, ref_h) and torch.equal(out.c, ref_c)
    args2, out2 = _train_args(c, restart=False, store=True)
    kernels.lstm_cell_train(**args2)
    assert torch.equal(out2.h, out.h) and torch.equal(out2.c, out.c) and torch.equal(out2.gates, out.gates)
    assert torch.equal(out2.hin, c.h * keep)


def _bwd_case(M, dev, seed):
    gen = torch.Generator(device=dev).manual_seed(seed)
    rn = lambda *s: torch.randn(*s, device=dev, generator=gen)  # noqa: E731
    z = rn(4, M, H).double()
    acts = torch.stack([torch.sigmoid(z[0]), torch.sigmoid(z[1]), torch.tanh(z[2]), torch.sigmoid(z[3])]).float()
    gates = torch.empty(4, 2, M, H, device=dev)
    gates[:, 0] = acts
    w_hh = (torch.rand(4 * H, H, device=dev, generator=gen) * 2 - 1) / 16
    c = SimpleNamespace(M=M, gates=gates[:, 0], c_prev=rn(M, H) * 0.7, cr=rn(M, H) * 0.4,
                        reset_cur=_resets(M, dev, gen), reset_next=_resets(M, dev, gen).flip(0), dh=rn(M, H),
                        dg_next=(rn(4, 2, M, H) * 0.2)[:, 1], dc_next=rn(M, H), whh_t=kernels.lstm_whh_t_image(w_hh))
    c.merged = torch.where((c.reset_cur != 0).view(M, 1), c.cr, c.c_prev)
    c.c_out = (c.gates[1].double() * c.merged.double() + c.gates[0].double() * c.gates[2].double()).float()
    return c


def _bwd_args(c, **kw):
    dev = c.dh.device
    args = dict(dh=c.dh, gates=c.gates, c_out=c.c_out, c_prev=c.c_prev, reset_cur=c.reset_cur, dg_next=c.dg_next,
                dc_next=c.dc_next, reset_next=c.reset_next, whh_t_image=c.whh_t,
                dg=torch.empty(4, 2, c.M, H, device=dev)[:, 0], dc_prev=torch.empty(c.M, H, device=dev),
                c_restart=c.cr)
    args.update(kw)
    return args


@pytest.mark.parametrize("M", [64, 192])
def test_reverse_step_reads_c_restart(M, cuda_device):
    c = _bwd_case(M, cuda_device, 300 + M)
    a = _bwd_args(c)
    kernels.lstm_cell_bwd(**a)
    b = _bwd_args(c, c_prev=c.merged, reset_cur=None, c_restart=None)
    kernels.lstm_cell_bwd(**b)
    assert torch.equal(a["dg"], b["dg"]) and torch.equal(a["dc_prev"], b["dc_prev"])
    # c_restart NULL: the reset rows' c_prev reads zero, as in ABI 26 -- the call on rows zeroed beforehand
    z = _bwd_args(c, c_restart=None)
    kernels.lstm_cell_bwd(*[z[k] for k in ("dh", "gates", "c_out", "c_prev", "reset_cur", "dg_next", "dc_next",
                                           "reset_next", "whh_t_image", "dg", "dc_prev")])
    z0 = _bwd_args(c, c_prev=c.c_prev * (c.reset_cur == 0).view(M, 1), reset_cur=None, c_restart=None)
    kernels.lstm_cell_bwd(**z0)
    assert torch.equal(z["dg"], z0["dg"]) and torch.equal(z["dc_prev"], z0["dc_prev"])
    assert not torch.equal(z["dg"][1], a["dg"][1])  # dg_f = dc c_prev f (1 - f) sees the restart state
    # the cut at reset_next is unchanged: rows reset after this step take nothing from the next one
    last = _bwd_args(c, dg_next=None, dc_next=None, reset_next=None)
    kernels.lstm_cell_bwd(**last)
    rows = c.reset_next != 0
    assert torch.equal(a["dg"][:, rows], last["dg"][:, rows]) and torch.equal(a["dc_prev"][rows], last["dc_prev"][rows])


@pytest.mark.parametrize("M", [64, 192])
def test_pair_forms_equal_two_single_calls(M, cuda_device):
    cases = [_train_case(M, 48, cuda_device, 400 + M), _train_case(M, 32, cuda_device, 500 + M)]
    single, paired = [], []
    for c in cases:
        args, out = _train_args(c)
        kernels.lstm_cell_train(**args)
        single.append(out)
    pair_args = []
    for c in cases:
        args, out = _train_args(c)
        pair_args.append(args)
        paired.append(out)
    kernels.lstm_cell_train_pair(*pair_args)
    for s, p in zip(single, paired):
        assert torch.equal(s.h, p.h) and torch.equal(s.c, p.c) and torch.equal(s.gates, p.gates)
        assert torch.equal(s.hin, p.hin)
    bcases = [_bwd_case(M, cuda_device, 600 + M), _bwd_case(M, cuda_device, 700 + M)]
    singles = [_bwd_args(c) for c in bcases]
    for a in singles:
        kernels.lstm_cell_bwd(**a)
    pairs = [_bwd_args(c) for c in bcases]
    kernels.lstm_cell_bwd_pair(*pairs)
    for s, p in zip(singles, pairs):
        assert torch.equal(s["dg"], p["dg"]) and torch.equal(s["dc_prev"], p["dc_prev"])
    # a pair of unequal row counts is refused
    with pytest.raises(ValueError):
        other = _train_case(64 if M != 64 else 128, 32, cuda_device, 1)
        kernels.lstm_cell_train_pair(pair_args[0], _train_args(other)[0])


def _sequence_reference(x, reset, restart, wts, w_out, dtype):
    """The restatement (recurrent_fused_fixtures.lstm_sequence: a where-merge of the restart states) in `dtype`;
    loss = sum_t <h_t, w_out_t>.  Returns (dW_ih, dW_hh, db, dc of the first state)."""
    w = [t.to(dtype).clone().requires_grad_(True) for t in wts]
    rnn = SimpleNamespace(weight_ih_l0=w[0], weight_hh_l0=w[1], bias_ih_l0=w[2], bias_hh_l0=w[3])
    c0 = restart[1][0].to(dtype).clone().requires_grad_(True)
    hs = [h.to(dtype) for h in restart[0]]
    cs = [c0] + [c.to(dtype) for c in restart[1][1:]]
    h = RFF.lstm_sequence(rnn, x.to(dtype), reset, (hs, cs))
    (h * w_out.to(dtype)).sum().backward()
    return w[0].grad, w[1].grad, w[2].grad, c0.grad


def test_four_step_sequence_with_restarts(cuda_device):
    M, D, S = 192, 48, 4
    dev = cuda_device
    gen = torch.Generator(device=dev).manual_seed(9)
    rn = lambda *s: torch.randn(*s, device=dev, generator=gen)  # noqa: E731
    wts = _weights(D, dev, gen)
    w_ih, w_hh, b_ih, b_hh = wts
    x, w_out = rn(S, M, D), rn(S, M, H)
    restart = (rn(S, M, H) * 0.5, rn(S, M, H) * 0.5)
    reset = torch.stack([torch.zeros(M, dtype=torch.uint8, device=dev), _resets(M, dev, gen),
                         _resets(M, dev, gen).flip(0), _resets(M, dev, gen)])
    assert (reset[1] & reset[2]).any()  # two consecutive restarts
    image, whh_t = kernels.lstm_image(w_ih, w_hh), kernels.lstm_whh_t_image(w_hh)
    hout, cout, hin = (torch.empty(S, M, H, device=dev) for _ in range(3))
    gates, dg = torch.empty(4, S, M, H, device=dev), torch.empty(4, S, M, H, device=dev)
    dc = torch.empty(2, M, H, device=dev)
    for t in range(S):
        state = (hout[t - 1], cout[t - 1]) if t else (restart[0][0], restart[1][0])
        kernels.lstm_cell_train(x[t], state, image, b_ih, b_hh, reset[t] if t else None, hout[t], cout[t], gates[:, t],
                                h_restart=restart[0][t] if t else None, c_restart=restart[1][t] if t else None,
                                h_in_out=hin[t])
    for t in range(S - 1, -1, -1):
        nxt = t + 1 < S
        kernels.lstm_cell_bwd(w_out[t], gates[:, t], cout[t], cout[t - 1] if t else restart[1][0],
                              reset[t] if t else None, dg[:, t + 1] if nxt else None, dc[(t + 1) & 1] if nxt else None,
                              reset[t + 1] if nxt else None, whh_t, dg[:, t], dc[t & 1],
                              c_restart=restart[1][t] if t else None)
    dw_ih, dw_hh, db = [], [], []
    for g in range(4):
        dz = dg[g].view(S * M, H)
        w, b = fused_mlp.linear_wgrad(dz, x.view(S * M, D), bias_side=1)
        dw_ih.append(w)
        db.append(b)
        dw_hh.append(fused_mlp.linear_wgrad(dz, hin.view(S * M, H)))
    ours = (torch.cat(dw_ih), torch.cat(dw_hh), torch.cat(db), dc[0])
    ref = _sequence_reference(x, reset, restart, wts, w_out, torch.float64)
    yard = _sequence_reference(x, reset, restart, wts, w_out, torch.float32)
    for name, o, r, y in zip(("dW_ih", "dW_hh", "db", "dc_0"), ours, ref, yard):
        e, ye = rms(o, r), rms(y, r)
        print(f"sequence {name}: rms err {e:.2e}, the fp32 restatement {ye:.2e}, scale {r.abs().max().item():.2e}")
        assert e <= 2 * ye, (name, e, ye)
