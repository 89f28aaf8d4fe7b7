"""The fused GRU cell without a GPU: ABI 28's symbols and argument validation (nothing is launched),
the shapes the cell refuses, the formulas of tests/gru_fixtures.py against CPU autograd of nn.GRU in fp64 on a sequence
with restarts, and the env-major formulation under CPU autograd against the reference's first-mini-batch gradient of
the rec_e fixture."""

import ctypes
from types import SimpleNamespace

import torch
import torch.nn as nn

import gru_fixtures as GF
import recurrent_fixtures as RF
import recurrent_fused_fixtures as RFF
from rsl_rl_amd import _lib, kernels

META_E = GF.load_meta()
P = 4096  # never dereferenced: every call below is rejected on its arguments
SYMBOLS = ("rslrl_gru_image_bytes", "rslrl_gru_prepare_image", "rslrl_gru_cell", "rslrl_gru_cell_pair",
           "rslrl_gru_cell_train", "rslrl_gru_cell_train_pair", "rslrl_gru_whh_t_image_bytes",
           "rslrl_gru_prepare_whh_t_image", "rslrl_gru_cell_bwd", "rslrl_gru_cell_bwd_pair")
UNSUPPORTED = ((100, 48, 256, 1), (64, 40, 256, 1), (64, 48, 64, 1), (64, 48, 256, 2))  # M, D, hidden, layers


def _cell(**kw):
    base = dict(x=P, h=P * 2, image=P * 4, b_ih=P * 5, b_hh=P * 6, h_out=P * 7, D=48, hidden=256, layers=1, reserved=0)
    base.update(kw)
    return _lib.GruCell(**base)


def _train(**kw):
    top = dict(gates=P * 9, reset=P * 10, gate_stride=64 * 256, h_restart=P * 11, h_in_out=P * 13)
    cell = {k: kw.pop(k) for k in list(kw) if k not in top}
    top.update(kw)
    return _lib.GruTrain(cell=_cell(**cell), **top)


def _bwd(**kw):
    base = dict(dh=P, dg_next=P * 2, dhz_next=P * 3, reset_next=P * 4, gates=P * 5, h_in=P * 6, whh_t_image=P * 9,
                dg=P * 10, dhz_out=P * 11, gate_stride=64 * 256, next_stride=64 * 256, hidden=256, layers=1)
    base.update(kw)
    return _lib.GruBwd(**base)


def test_abi_28_symbols():
    L = _lib.lib()
    assert L.rslrl_abi_version() == _lib.ABI_VERSION >= 28
    for name in SYMBOLS:
        assert hasattr(L, name), name
    # the images: three gate blocks of depth D + 256, and W_hh^T at depth 768
    assert L.rslrl_gru_image_bytes(48) == 3 * L.rslrl_linear_bimage_bytes(48 + 256)
    assert L.rslrl_gru_whh_t_image_bytes() == L.rslrl_linear_bimage_bytes(768)
    assert L.rslrl_gru_image_bytes(40) == 0 and L.rslrl_gru_image_bytes(272) == 0 and L.rslrl_gru_image_bytes(0) == 0


def test_supported_shapes():
    for M, D, hidden, layers in UNSUPPORTED:
        assert not kernels.gru_cell_supported(M, D, hidden, layers), (M, D, hidden, layers)
    for M, D in ((64, 16), (192, 48), (65536, 256)):
        assert kernels.gru_cell_supported(M, D, 256) and kernels.gru_cell_supported(M, D, 256, 1)
    assert not kernels.gru_cell_supported(0, 48, 256) and not kernels.gru_cell_supported(64, 272, 256)


def test_entry_points_refuse_unsupported_shapes_before_any_launch():
    L = _lib.lib()
    ok_c, ok_t, ok_b = _cell(), _train(), _bwd()
    for M, D, hidden, layers in UNSUPPORTED:
        kw = dict(D=D, hidden=hidden, layers=layers)
        bad_c, bad_t = _cell(**kw), _train(**kw)
        assert L.rslrl_gru_cell(ctypes.byref(bad_c), M, None) == _lib.E_UNSUPPORTED, (M, kw)
        assert L.rslrl_gru_cell_train(ctypes.byref(bad_t), M, None) == _lib.E_UNSUPPORTED, (M, kw)
        for first, second in ((ok_c, bad_c), (bad_c, ok_c)):
            assert L.rslrl_gru_cell_pair(ctypes.byref(first), ctypes.byref(second), M, None) == _lib.E_UNSUPPORTED
        for first, second in ((ok_t, bad_t), (bad_t, ok_t)):
            assert L.rslrl_gru_cell_train_pair(ctypes.byref(first), ctypes.byref(second), M, None) == _lib.E_UNSUPPORTED
        if D == 48:  # the reverse step has no input width
            bad_b = _bwd(hidden=hidden, layers=layers)
            assert L.rslrl_gru_cell_bwd(ctypes.byref(bad_b), M, None) == _lib.E_UNSUPPORTED, (M, kw)
            for first, second in ((ok_b, bad_b), (bad_b, ok_b)):
                assert L.rslrl_gru_cell_bwd_pair(ctypes.byref(first), ctypes.byref(second), M, None) == _lib.E_UNSUPPORTED
    assert L.rslrl_gru_prepare_image(P, P * 2, 40, 256, P * 3, None) == _lib.E_UNSUPPORTED
    assert L.rslrl_gru_prepare_image(P, P * 2, 48, 128, P * 3, None) == _lib.E_UNSUPPORTED
    assert L.rslrl_gru_prepare_whh_t_image(P, 128, P * 3, None) == _lib.E_UNSUPPORTED


def test_entry_points_validate_pointers_aliasing_and_alignment():
    L = _lib.lib()
    ok_t, ok_b = _train(), _bwd()
    assert L.rslrl_gru_cell_pair(None, None, 64, None) == _lib.E_INVALID_ARGUMENT
    assert L.rslrl_gru_cell_train_pair(None, None, 64, None) == _lib.E_INVALID_ARGUMENT
    assert L.rslrl_gru_cell_bwd_pair(None, None, 64, None) == _lib.E_INVALID_ARGUMENT
    for kw in (dict(x=None), dict(h_out=None), dict(image=None), dict(h_out=P * 2)):  # h_out must not be h
        assert L.rslrl_gru_cell(ctypes.byref(_cell(**kw)), 64, None) == _lib.E_INVALID_ARGUMENT, kw
    assert L.rslrl_gru_cell(ctypes.byref(_cell(h=P + 4)), 64, None) == -4
    # the second problem is validated like the first
    for kw in (dict(gates=None), dict(x=None), dict(h_in_out=P * 2), dict(h_in_out=P * 11), dict(h_in_out=P * 7),
               dict(h_restart=P * 7), dict(gate_stride=64 * 256 - 4)):
        assert L.rslrl_gru_cell_train_pair(ctypes.byref(ok_t), ctypes.byref(_train(**kw)), 64, None) == \
            _lib.E_INVALID_ARGUMENT, kw
    for kw in (dict(h_restart=P + 4), dict(h_in_out=P + 4), dict(gate_stride=64 * 256 + 2)):
        assert L.rslrl_gru_cell_train_pair(ctypes.byref(ok_t), ctypes.byref(_train(**kw)), 64, None) == -4, kw
    for kw in (dict(dh=None), dict(dg=None), dict(dg=P * 2), dict(whh_t_image=None), dict(h_in=None),
               dict(dhz_out=None), dict(gate_stride=64)):  # dg must not be dg_next
        assert L.rslrl_gru_cell_bwd_pair(ctypes.byref(ok_b), ctypes.byref(_bwd(**kw)), 64, None) == \
            _lib.E_INVALID_ARGUMENT, kw
    for kw in (dict(dhz_next=P + 4), dict(h_in=P + 8)):
        assert L.rslrl_gru_cell_bwd_pair(ctypes.byref(ok_b), ctypes.byref(_bwd(**kw)), 64, None) == -4, kw


def test_formulas_match_autograd_of_nn_gru_in_fp64():
    """A four-step env-major sequence with restarts, two consecutive ones included, through nn.GRU itself under CPU
    autograd in fp64, against gru_fixtures' forward and hand-written reverse pass: h', the four parameter gradients
    (db_ih and db_hh differ in the n block) and d loss / d h_0."""
    torch.manual_seed(0)
    S, E, D = 4, 6, 5
    rnn = nn.GRU(D, GF.H).double()
    x, w_out = torch.randn(S, E, D, dtype=torch.float64), torch.randn(S, E, GF.H, dtype=torch.float64)
    restart = torch.randn(S, E, GF.H, dtype=torch.float64) * 0.5
    reset = torch.zeros(S, E, dtype=torch.uint8)
    reset[1, [0, 1]] = reset[2, [1, 2]] = reset[3, [1, 4]] = 1  # row 1 restarts three times in a row; rows 3, 5 never
    h0 = restart[0].clone().requires_grad_(True)
    h, outs = h0, []
    for t in range(S):
        if t:
            h = torch.where(reset[t].bool().unsqueeze(-1), restart[t], h)
        out, hn = rnn(x[t].unsqueeze(0), h.unsqueeze(0))
        h = hn[0]
        outs.append(out[0])
    ref_h = torch.stack(outs)
    (ref_h * w_out).sum().backward()

    ws = GF.params(rnn)
    tape = SimpleNamespace()
    with torch.no_grad():
        ours_h = GF.gru_sequence(ws, x, reset, restart, tape)
        g = GF.gru_sequence_backward(ws, x, reset, tape, w_out)
        dh0 = g.carry0 + torch.cat([g.dg[0, 0], g.dg[1, 0], g.dg[3, 0]], dim=-1) @ ws[1]
    assert (ours_h - ref_h).abs().max().item() <= 1e-14
    for name, ours, ref in (("dW_ih", g.dw_ih, rnn.weight_ih_l0.grad), ("dW_hh", g.dw_hh, rnn.weight_hh_l0.grad),
                            ("db_ih", g.db_ih, rnn.bias_ih_l0.grad), ("db_hh", g.db_hh, rnn.bias_hh_l0.grad),
                            ("dh_0", dh0, h0.grad)):
        err = (ours - ref).abs().max().item() / ref.abs().max().item()
        print(f"{name}: error / max {err:.1e}")
        assert err <= 1e-13, (name, err)  # fp64 rounding of sums of <= 24 rows x 768 terms; the issue saw 3e-16
    assert not torch.equal(rnn.bias_ih_l0.grad[2 * GF.H:], rnn.bias_hh_l0.grad[2 * GF.H:])
    assert torch.equal(g.db_ih[:2 * GF.H], g.db_hh[:2 * GF.H])


def test_sequence_gradient_matches_the_reference_on_cpu():
    """The env-major formulation in plain torch under CPU autograd: rec_e's first-mini-batch gradient within 1e-5 of
    its max of the reference's (the project's bound for that quantity)."""
    meta = META_E["rec_e"]
    z = RF.Arrays(meta["files"])
    torch.set_num_threads(1)
    alg, pol = RFF.build_update_cpu(z, meta)
    assert isinstance(pol.memory_a.rnn, nn.GRU) and len(alg.storage.saved_hidden_states_a) == 1
    batch = next(iter(alg.storage.recurrent_sequence_generator(meta["M"], 1)))
    loss = GF.sequence_loss(alg, pol, batch)
    grads = torch.autograd.grad(loss, list(pol.parameters()))
    ours = torch.cat([g.reshape(-1) for g in grads]).double()
    ref = torch.from_numpy(z["r0/grad_mb0"]).double()
    err = (ours - ref).abs().max().item() / ref.abs().max().item()
    print("rec_e first mini-batch gradient error / max:", f"{err:.2e}")
    assert err <= 1e-5, err


def test_rec_e_fixture_exercises_every_restart():
    meta = META_E["rec_e"]
    assert (meta["T"], meta["N"], meta["M"], meta["H"], meta["L"], meta["n_states"]) == (8, 128, 2, 256, 1, 1)
    assert meta["rnn_type"] == "gru" and len(meta["files"]) == 16
    nz = RF.storage_inputs(meta["ranks"][0]["noise_seed"], meta["T"], meta["N"], meta["O"], meta["A"], 1, 256, 1)
    assert RF.inputs_digest(nz) == meta["ranks"][0]["inputs_sha256"]
    d = nz["dones"][:, :, 0].astype(bool)
    E = meta["N"] // meta["M"]
    assert E % 64 == 0
    for i in range(meta["M"]):
        s = d[:, i * E:(i + 1) * E]
        assert (~s.any(axis=0)).any() and s[0].any() and s[-1].any() and (s[:-1] & s[1:]).any()
    for kl in meta["ranks"][0]["kl_trace"]:
        assert all(abs(kl - thr) >= 0.10 * thr for thr in (0.02, 0.005)), kl
    assert meta["ranks"][0]["lr_trace"] == [0.0015] * 4
