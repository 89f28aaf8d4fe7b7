"""The fused GRU cell's formulas restated in plain torch, shared by the GRU tests: one step, the
env-major sequence with a `where`-merge of the restart states (differentiable: what CPU autograd and the rec_e gradient
check run), the hand-written reverse pass that the kernels implement, and the rec_e fixture's metadata.  Any device,
any dtype.

  r = s(x W_ir^T + b_ir + h W_hr^T + b_hr)      z = s(x W_iz^T + b_iz + h W_hz^T + b_hz)
  a = h W_hn^T + b_hn                           n = tanh(x W_in^T + b_in + r a)             h' = (1 - z) n + z h
  dh~ = dh + (reset_next ? 0 : dhz_next + [dg_next.r | dg_next.z | dg_next.a] W_hh)
  dn = dh~ (1 - z) (1 - n^2)     dg.r = dn a r (1 - r)     dg.z = dh~ (h_in - n) z (1 - z)     dg.n = dn     dg.a = dn r
  dhz = dh~ z
"""

import json
import os
from types import SimpleNamespace

import torch
import torch.nn.functional as F

import recurrent_fixtures as RF
import recurrent_fused_fixtures as RFF

H = 256


def load_meta():
    with open(os.path.join(RF.GOLDEN, "golden_recurrent_gru.json")) as f:
        return json.load(f)


def params(rnn, dtype=None):
    """(W_ih, W_hh, b_ih, b_hh) of a one-layer nn.GRU (or anything with its attribute names)."""
    ws = (rnn.weight_ih_l0, rnn.weight_hh_l0, rnn.bias_ih_l0, rnn.bias_hh_l0)
    return ws if dtype is None else tuple(w.to(dtype) for w in ws)


def gru_step(x, h, w_ih, w_hh, b_ih, b_hh):
    """(h', [r, z, n, a]) of one step; h None: zeros."""
    if h is None:
        h = torch.zeros(x.shape[0], w_hh.shape[1], dtype=x.dtype, device=x.device)
    xr, xz, xn = F.linear(x, w_ih, b_ih).chunk(3, dim=-1)
    hr, hz, a = F.linear(h, w_hh, b_hh).chunk(3, dim=-1)
    r, z = torch.sigmoid(xr + hr), torch.sigmoid(xz + hz)
    n = torch.tanh(xn + r * a)
    return (1 - z) * n + z * h, [r, z, n, a]


def gru_sequence(ws, x, reset, restart, tape=None):
    """h' [T, E, H] over the env-major sequence x [T, E, D]: step t continues from step t - 1 except in the rows whose
    reset[t] is set, which restart from restart[t] (every row at t = 0; restart may be a list of per-step tensors); the
    merge is a torch.where, so no gradient crosses a restart.  tape: a SimpleNamespace that receives hin [T, E, H] and
    gates [4, T, E, H]."""
    h, out, hin, gates = restart[0], [], [], []
    for t in range(x.shape[0]):
        if t:
            h = torch.where(reset[t].bool().unsqueeze(-1), restart[t], h)
        hin.append(h)
        h, g = gru_step(x[t], h, *ws)
        out.append(h)
        gates.append(torch.stack(g))
    if tape is not None:
        tape.hin, tape.gates = torch.stack(hin), torch.stack(gates, dim=1)
    return torch.stack(out)


def gru_sequence_backward(ws, x, reset, tape, dh):
    """The reverse pass by the formulas above from dh [T, E, H] = d loss / d h'_t and the forward's tape: returns
    SimpleNamespace(dw_ih, dw_hh, db_ih, db_hh, carry0, dg) -- carry0 is dhz of step 0; d loss / d h_0 is carry0 +
    [dg_0.r | dg_0.z | dg_0.a] W_hh."""
    w_hh = ws[1]
    T = x.shape[0]
    dg = torch.zeros_like(tape.gates)
    dhz = None
    for t in range(T - 1, -1, -1):
        dht = dh[t]
        if t + 1 < T:
            rec = dhz + torch.cat([dg[0, t + 1], dg[1, t + 1], dg[3, t + 1]], dim=-1) @ w_hh
            dht = dht + torch.where(reset[t + 1].bool().unsqueeze(-1), torch.zeros_like(rec), rec)
        r, z, n, a = tape.gates[:, t]
        dn = dht * (1 - z) * (1 - n * n)
        dg[0, t], dg[1, t], dg[2, t], dg[3, t] = dn * a * r * (1 - r), dht * (tape.hin[t] - n) * z * (1 - z), dn, dn * r
        dhz = dht * z
    flat = lambda t: t.reshape(-1, t.shape[-1])  # noqa: E731
    gi = torch.cat([flat(dg[0]), flat(dg[1]), flat(dg[2])], dim=-1)  # against x
    gh = torch.cat([flat(dg[0]), flat(dg[1]), flat(dg[3])], dim=-1)  # against the h as consumed
    return SimpleNamespace(dw_ih=gi.t() @ flat(x), dw_hh=gh.t() @ flat(tape.hin), db_ih=gi.sum(0), db_hh=gh.sum(0),
                           carry0=dhz, dg=dg)


def sequence_loss(alg, pol, batch):
    """recurrent_fused_fixtures.sequence_loss with the GRU sequence in place of the LSTM's (the rest is that function's,
    reached by swapping the one helper it calls)."""
    inner = RFF.lstm_sequence
    RFF.lstm_sequence = lambda rnn, x, reset, restart: gru_sequence(params(rnn), x, reset, restart)
    try:
        return RFF.sequence_loss(alg, pol, batch)
    finally:
        RFF.lstm_sequence = inner
