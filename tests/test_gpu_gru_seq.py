"""The training form and the reverse step of the fused GRU cell (csrc/gru_cell.hip) at M 64 and 192, with
a row tile where every row resets and one where none does (M 192): the training form against the rollout step's bits,
restarts against calls on inputs merged beforehand, the stored state as consumed, the chain's cut at reset_next, the
pair forms against the single calls -- all bit for bit -- and a four-step sequence with two consecutive restarts
against the fp64 restatement of tests/gru_fixtures.py, where each quantity may be off by twice the RMS error of the
same restatement in fp32 on the device."""

from types import SimpleNamespace

import pytest
import torch

import gru_fixtures as GF
from rsl_rl_amd import kernels
from rsl_rl_amd.networks import fused_mlp

pytestmark = pytest.mark.gpu
H = GF.H


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
    return mk(3 * H, D), mk(3 * H, H), mk(3 * H), mk(3 * H)


def _train_case(M, D, dev, seed):
    gen = torch.Generator(device=dev).manual_seed(seed)
    rn = lambda *s: torch.randn(*s, device=dev, generator=gen)  # noqa: E731
    w_ih, w_hh, b_ih, b_hh = _weights(D, dev, gen)
    c = SimpleNamespace(M=M, D=D, x=rn(M, D), h=rn(M, H) * 0.5, hr=rn(M, H) * 0.3, reset=_resets(M, dev, gen),
                        image=kernels.gru_image(w_ih, w_hh), b_ih=b_ih, b_hh=b_hh, ws=(w_ih, w_hh, b_ih, b_hh))
    c.h_merged = torch.where((c.reset != 0).view(M, 1), c.hr, c.h)
    return c


def _train_args(c, restart=True, store=True):
    dev = c.x.device
    out = SimpleNamespace(h=torch.empty(c.M, H, device=dev), gates=torch.empty(4, 2, c.M, H, device=dev)[:, 1],
                          hin=torch.full((c.M, H), 7.0, device=dev) if store else None)
    args = dict(x=c.x, h=c.h, image=c.image, b_ih=c.b_ih, b_hh=c.b_hh, reset=c.reset, h_out=out.h, gates=out.gates,
                h_restart=c.hr if restart else None, h_in_out=out.hin)
    return args, out


@pytest.mark.parametrize("D", [16, 48, 256])
@pytest.mark.parametrize("M", [64, 192])
def test_training_form_against_the_cell(M, D, cuda_device):
    c = _train_case(M, D, cuda_device, 100 + M + D)
    assert c.reset.any() and not c.reset.all()
    # reset, h_restart and h_in_out NULL: the rollout step's bits, with and without a state
    for h in (c.h, None):
        out = torch.empty(M, H, device=cuda_device)
        gates = torch.empty(4, M, H, device=cuda_device)
        kernels.gru_cell_train(c.x, h, c.image, c.b_ih, c.b_hh, None, out, gates)
        assert torch.equal(out, kernels.gru_cell(c.x, h, c.image, c.b_ih, c.b_hh))
        # the stored gates are the formulas' r, z, n, a.  A pre-activation is an fp32 sum of <= 512 products with
        # |w| <= 1/16 and O(1) inputs: rounding ~ sqrt(512) * 6e-8 ~ 1.4e-6 on values of O(1), through activations of
        # slope <= 1 and one fp32 rounding of the stored value; 1e-5 absolute leaves about 7x over that
        ref = torch.stack(GF.gru_step(c.x.double(), None if h is None else h.double(),
                                      *(w.double() for w in c.ws))[1])
        assert (gates.double() - ref).abs().max().item() <= 1e-5
    # restarts: the cell on inputs merged beforehand; the state as consumed is the merged state
    ref_h = kernels.gru_cell(c.x, c.h_merged, c.image, c.b_ih, c.b_hh)
    args, out = _train_args(c)
    kernels.gru_cell_train(**args)
    assert torch.equal(out.h, ref_h) and torch.equal(out.hin, c.h_merged)
    plain = dict(args, h=c.h_merged, reset=None, h_restart=None, h_in_out=None, h_out=torch.empty_like(out.h),
                 gates=torch.empty(4, M, H, device=cuda_device))
    kernels.gru_cell_train(**plain)
    assert torch.equal(out.gates, plain["gates"]) and torch.equal(plain["h_out"], ref_h)
    # h_restart NULL: a reset row reads zero; storing h_in_out changes no other output
    keep = (c.reset == 0).view(M, 1)
    args0, out0 = _train_args(c, restart=False, store=False)
    kernels.gru_cell_train(**args0)
    assert torch.equal(out0.h, kernels.gru_cell(c.x, c.h * keep, c.image, c.b_ih, c.b_hh))
    args1, out1 = _train_args(c, restart=False, store=True)
    kernels.gru_cell_train(**args1)
    assert torch.equal(out1.h, out0.h) and torch.equal(out1.gates, out0.gates) and torch.equal(out1.hin, c.h * keep)
    # no state at all: the reset rows restart, the others read zero
    r = (c.reset != 0).view(M, 1)
    args2, out2 = _train_args(c)
    kernels.gru_cell_train(**dict(args2, h=None))
    assert torch.equal(out2.h, kernels.gru_cell(c.x, c.hr * r, c.image, c.b_ih, c.b_hh))
    assert torch.equal(out2.hin, c.hr * r)


def _bwd_case(M, dev, seed):
    gen = torch.Generator(device=dev).manual_seed(seed)
    rn = lambda *s: torch.randn(*s, device=dev, generator=gen)  # noqa: E731
    z = rn(4, M, H).double()
    gates = torch.empty(4, 2, M, H, device=dev)
    gates[:, 0] = torch.stack([torch.sigmoid(z[0]), torch.sigmoid(z[1]), torch.tanh(z[2]), 0.5 * z[3]]).float()
    w_hh = (torch.rand(3 * H, H, device=dev, generator=gen) * 2 - 1) / 16
    return SimpleNamespace(M=M, gates=gates[:, 0], h_in=rn(M, H) * 0.5, reset_next=_resets(M, dev, gen), dh=rn(M, H),
                           dg_next=(rn(4, 2, M, H) * 0.2)[:, 1], dhz_next=rn(M, H), w_hh=w_hh,
                           whh_t=kernels.gru_whh_t_image(w_hh))


def _bwd_args(c, **kw):
    dev = c.dh.device
    args = dict(dh=c.dh, gates=c.gates, h_in=c.h_in, dg_next=c.dg_next, dhz_next=c.dhz_next, reset_next=c.reset_next,
                whh_t_image=c.whh_t, dg=torch.empty(4, 2, c.M, H, device=dev)[:, 0],
                dhz_out=torch.empty(c.M, H, device=dev))
    args.update(kw)
    return args


@pytest.mark.parametrize("M", [64, 192])
def test_reverse_step(M, cuda_device):
    c = _bwd_case(M, cuda_device, 300 + M)
    a = _bwd_args(c)
    kernels.gru_cell_bwd(**a)
    # rows reset after this step take nothing from the next one: the last-step form's bits
    last = _bwd_args(c, dg_next=None, dhz_next=None, reset_next=None)
    kernels.gru_cell_bwd(**last)
    rows = c.reset_next != 0
    assert rows.any() and not rows.all()
    assert torch.equal(a["dg"][:, rows], last["dg"][:, rows]) and torch.equal(a["dhz_out"][rows], last["dhz_out"][rows])
    assert not torch.equal(a["dg"][:, ~rows], last["dg"][:, ~rows])
    # every row against the formulas in fp64 (the GEMM reads blocks 0, 1 and 3 of dg_next, never block 2): the
    # recurrent term is an fp32-faithful sum of 768 products of O(0.2) x <= 1/16, the rest fp64 rounded once, so the
    # error is a few fp32 ulps of O(1) values -- 1e-5 relative to the tensor's scale, the bound used above
    r, z, n, g_a = c.gates.double()
    rec = torch.cat([c.dg_next[0], c.dg_next[1], c.dg_next[3]], dim=1).double() @ c.w_hh.double() + c.dhz_next.double()
    dht = c.dh.double() + torch.where(rows.view(M, 1), torch.zeros_like(rec), rec)
    dn = dht * (1 - z) * (1 - n * n)
    ref = torch.stack([dn * g_a * r * (1 - r), dht * (c.h_in.double() - n) * z * (1 - z), dn, dn * r])
    assert (a["dg"].double() - ref).abs().max().item() <= 1e-5 * (1 + ref.abs().max().item())
    assert (a["dhz_out"].double() - dht * z).abs().max().item() <= 1e-5 * (1 + dht.abs().max().item())
    poisoned = c.dg_next.clone()
    poisoned[2] = float("nan")
    b = _bwd_args(c, dg_next=poisoned)
    kernels.gru_cell_bwd(**b)
    assert torch.equal(a["dg"], b["dg"]) and torch.equal(a["dhz_out"], b["dhz_out"])
    # dhz_out may be dhz_next; a repeated call gives the same bits
    carry = c.dhz_next.clone()
    inplace = _bwd_args(c, dhz_next=carry, dhz_out=carry)
    kernels.gru_cell_bwd(**inplace)
    assert torch.equal(inplace["dg"], a["dg"]) and torch.equal(carry, a["dhz_out"])


@pytest.mark.parametrize("M", [64, 192])
def test_pair_forms_equal_two_single_calls(M, cuda_device):
    cases = [_train_case(M, 48, cuda_device, 400 + M), _train_case(M, 32, cuda_device, 500 + M)]
    single, paired, pair_args = [], [], []
    for c in cases:
        args, out = _train_args(c)
        kernels.gru_cell_train(**args)
        single.append(out)
        args, out = _train_args(c)
        pair_args.append(args)
        paired.append(out)
    kernels.gru_cell_train_pair(*pair_args)
    for s, p in zip(single, paired):
        assert torch.equal(s.h, p.h) and torch.equal(s.gates, p.gates) and torch.equal(s.hin, p.hin)
    bcases = [_bwd_case(M, cuda_device, 600 + M), _bwd_case(M, cuda_device, 700 + M)]
    singles = [_bwd_args(c) for c in bcases]
    for a in singles:
        kernels.gru_cell_bwd(**a)
    pairs = [_bwd_args(c) for c in bcases]
    kernels.gru_cell_bwd_pair(*pairs)
    for s, p in zip(singles, pairs):
        assert torch.equal(s["dg"], p["dg"]) and torch.equal(s["dhz_out"], p["dhz_out"])
    with pytest.raises(ValueError):  # a pair of unequal row counts is refused
        other = _train_case(64 if M != 64 else 128, 32, cuda_device, 1)
        kernels.gru_cell_train_pair(pair_args[0], _train_args(other)[0])


def _restatement(ws, x, reset, restart, w_out, dtype):
    ws = tuple(w.to(dtype) for w in ws)
    tape = SimpleNamespace()
    GF.gru_sequence(ws, x.to(dtype), reset, restart.to(dtype), tape)
    g = GF.gru_sequence_backward(ws, x.to(dtype), reset, tape, w_out.to(dtype))
    return g.dw_ih, g.dw_hh, g.db_ih, g.db_hh, g.carry0


def test_four_step_sequence_with_restarts(cuda_device):
    M, D, S = 192, 48, 4
    dev = cuda_device
    gen = torch.Generator(device=dev).manual_seed(9)
    rn = lambda *s: torch.randn(*s, device=dev, generator=gen)  # noqa: E731
    ws = _weights(D, dev, gen)
    w_ih, w_hh, b_ih, b_hh = ws
    x, w_out, restart = rn(S, M, D), rn(S, M, H), rn(S, M, H) * 0.5
    reset = torch.stack([torch.zeros(M, dtype=torch.uint8, device=dev), _resets(M, dev, gen),
                         _resets(M, dev, gen).flip(0), _resets(M, dev, gen)])
    assert (reset[1] & reset[2]).any()  # two consecutive restarts
    image, whh_t = kernels.gru_image(w_ih, w_hh), kernels.gru_whh_t_image(w_hh)
    hout, hin = torch.empty(S, M, H, device=dev), torch.empty(S, M, H, device=dev)
    gates, dg = torch.empty(4, S, M, H, device=dev), torch.empty(4, S, M, H, device=dev)
    dhz = torch.empty(2, M, H, device=dev)
    for t in range(S):
        kernels.gru_cell_train(x[t], hout[t - 1] if t else restart[0], image, b_ih, b_hh, reset[t] if t else None,
                               hout[t], gates[:, t], h_restart=restart[t] if t else None, h_in_out=hin[t])
    for t in range(S - 1, -1, -1):
        nxt = t + 1 < S
        kernels.gru_cell_bwd(w_out[t], gates[:, t], hin[t], dg[:, t + 1] if nxt else None,
                             dhz[(t + 1) & 1] if nxt else None, reset[t + 1] if nxt else None, whh_t, dg[:, t],
                             dhz[t & 1])
    flat = lambda t: t.view(S * M, -1)  # noqa: E731
    dw_ih, dw_hh, db_ih, db_hh = [], [], [], []
    for gi, gh in ((0, 0), (1, 1), (2, 3)):  # W_ih takes the blocks r, z, n; W_hh takes r, z, a
        w, b = fused_mlp.linear_wgrad(flat(dg[gi]), flat(x), bias_side=1)
        dw_ih.append(w)
        db_ih.append(b)
        w, b = fused_mlp.linear_wgrad(flat(dg[gh]), flat(hin), bias_side=1)
        dw_hh.append(w)
        db_hh.append(b)
    ours = (torch.cat(dw_ih), torch.cat(dw_hh), torch.cat(db_ih), torch.cat(db_hh), dhz[0])
    ref = _restatement(ws, x, reset, restart, w_out, torch.float64)
    yard = _restatement(ws, x, reset, restart, w_out, torch.float32)
    for name, o, r, y in zip(("dW_ih", "dW_hh", "db_ih", "db_hh", "dhz_0"), ours, ref, yard):
        e, ye = rms(o, r), rms(y, r)
        print(f"sequence {name}: rms err {e:.2e}, the fp32 restatement {ye:.2e}, scale {r.abs().max().item():.2e}")
        assert e <= 2 * ye, (name, e, ye)
