"""The fused cells' `_h` entry points (hidden size 512; additions to ABI 34) without a GPU: their argument validation
(nothing is launched), the image byte counts, the Python predicates against the library, Cell.takes beside the unchanged
Cell.supported, the RSLRL_RNN_HIDDEN_512 knob, and the callers that must keep refusing: the distillation window at 512
and the recurrent PPO update on CPU tensors."""

import ctypes
import os
import subprocess
import sys

import pytest
import torch

from rsl_rl_amd import _lib, kernels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 4096  # never dereferenced: every call below is rejected on its arguments
H = 512
KINDS = ("lstm", "gru")


def lstm(**kw):
    base = dict(x=P, h=P * 2, c=P * 3, image=P * 4, b_ih=P * 5, b_hh=P * 6, h_out=P * 7, c_out=P * 8, D=45,
                hidden=H, layers=1, reserved=0)
    base.update(kw)
    return _lib.LstmCell(**base)


def gru(**kw):
    base = dict(x=P, h=P * 2, image=P * 4, b_ih=P * 5, b_hh=P * 6, h_out=P * 7, D=45, hidden=H, layers=1, reserved=0)
    base.update(kw)
    return _lib.GruCell(**base)


def _train(struct, cell, cell_kw, kw):
    t = struct()
    t.cell = cell(**(cell_kw or {}))
    t.gates, t.reset, t.gate_stride = P * 9, P * 10, 64 * H
    for k, v in kw.items():
        setattr(t, k, v)
    return t


def lstm_train(cell_kw=None, **kw):
    return _train(_lib.LstmTrain, lstm, cell_kw, kw)


def gru_train(cell_kw=None, **kw):
    return _train(_lib.GruTrain, gru, cell_kw, kw)


def lstm_bwd(**kw):
    base = dict(dh=P, dg_next=P * 2, dc_next=P * 3, reset_next=P * 4, gates=P * 5, c_out=P * 6, c_prev=P * 7,
                reset_cur=P * 8, whh_t_image=P * 9, dg=P * 10, dc_prev=P * 11, gate_stride=64 * H, next_stride=64 * H,
                hidden=H, layers=1, c_restart=P * 12)
    base.update(kw)
    return _lib.LstmBwd(**base)


def gru_bwd(**kw):
    base = dict(dh=P, dg_next=P * 2, dhz_next=P * 3, reset_next=P * 4, gates=P * 5, h_in=P * 6, whh_t_image=P * 9,
                dg=P * 10, dhz_out=P * 11, gate_stride=64 * H, next_stride=64 * H, hidden=H, layers=1)
    base.update(kw)
    return _lib.GruBwd(**base)


BAD_HIDDEN = (dict(hidden=128), dict(hidden=256), dict(hidden=1024), dict(layers=0), dict(layers=2))
BAD_WIDTHS = (dict(D=0), dict(D=1025))
BAD_ROWS = (0, 32, 100, -64)


def _refused(one, pair, ok, bads, code):
    for bad, M in bads:
        assert one(ctypes.byref(bad), M, None) == code
        assert pair(ctypes.byref(ok), ctypes.byref(bad), M, None) == code
        assert pair(ctypes.byref(bad), ctypes.byref(ok), M, None) == code


def test_the_abi_number_stays_34():
    assert _lib.lib().rslrl_abi_version() == _lib.ABI_VERSION == 34


@pytest.mark.parametrize("kind", KINDS)
def test_cell_entries_refuse_bad_problems_before_any_launch(kind):
    L = _lib.lib()
    cell = lstm if kind == "lstm" else gru
    one, pair = getattr(L, f"rslrl_{kind}_cell_h"), getattr(L, f"rslrl_{kind}_cell_pair_h")
    ok = cell()
    assert one(None, 64, None) == _lib.E_INVALID_ARGUMENT
    assert pair(None, ctypes.byref(ok), 64, None) == _lib.E_INVALID_ARGUMENT
    bads = [(cell(**kw), 64) for kw in BAD_HIDDEN + BAD_WIDTHS] + [(cell(), M) for M in BAD_ROWS]
    _refused(one, pair, ok, bads, _lib.E_UNSUPPORTED)
    nulls = [dict(x=None), dict(image=None), dict(b_ih=None), dict(b_hh=None), dict(h_out=None)]
    nulls += [dict(h_out=P * 2)]  # h_out must not be h
    if kind == "lstm":
        nulls += [dict(c_out=None), dict(h_out=P * 8)]  # nor c_out
    _refused(one, pair, ok, [(cell(**kw), 64) for kw in nulls], _lib.E_INVALID_ARGUMENT)
    # alignment: 16 bytes for everything but x, whose base needs 4 bytes where D % 4 != 0 and 16 where D % 4 == 0
    for kw in (dict(h=P * 2 + 4), dict(image=P * 4 + 8), dict(b_ih=P * 5 + 4), dict(h_out=P * 7 + 4), dict(x=P + 2),
               dict(x=P + 4, D=40), dict(x=P + 8, D=260)):
        bad = cell(**kw)
        assert one(ctypes.byref(bad), 64, None) == _lib.E_MISALIGNED, kw
        assert pair(ctypes.byref(ok), ctypes.byref(bad), 64, None) == _lib.E_MISALIGNED, kw


@pytest.mark.parametrize("kind", KINDS)
def test_train_entries_refuse_bad_problems_before_any_launch(kind):
    L = _lib.lib()
    train = lstm_train if kind == "lstm" else gru_train
    one, pair = getattr(L, f"rslrl_{kind}_cell_train_h"), getattr(L, f"rslrl_{kind}_cell_train_pair_h")
    ok = train()
    assert one(None, 64, None) == _lib.E_INVALID_ARGUMENT
    bads = [(train(kw), 64) for kw in BAD_HIDDEN + BAD_WIDTHS] + [(train(), M) for M in BAD_ROWS]
    _refused(one, pair, ok, bads, _lib.E_UNSUPPORTED)
    invalid = [train(dict(x=None)), train(gates=None),
               train(gate_stride=64 * H - 4),  # the gate blocks would overlap
               train(gate_stride=64 * 256),    # the 256 forms' stride
               train(h_in_out=P * 2),   # the h other blocks read
               train(h_in_out=P * 7),   # h_out
               train(h_in_out=P * 11, h_restart=P * 11), train(h_restart=P * 7)]
    if kind == "lstm":
        invalid += [train(h_in_out=P * 3), train(h_in_out=P * 8), train(h_in_out=P * 11, c_restart=P * 11)]
    _refused(one, pair, ok, [(bad, 64) for bad in invalid], _lib.E_INVALID_ARGUMENT)
    for bad in (train(gates=P * 9 + 4), train(gate_stride=64 * H + 2), train(h_restart=P * 11 + 4),
                train(h_in_out=P * 11 + 8), train(dict(x=P + 4, D=44))):
        assert one(ctypes.byref(bad), 64, None) == _lib.E_MISALIGNED


@pytest.mark.parametrize("kind", KINDS)
def test_bwd_entries_refuse_bad_problems_before_any_launch(kind):
    L = _lib.lib()
    bwd = lstm_bwd if kind == "lstm" else gru_bwd
    one, pair = getattr(L, f"rslrl_{kind}_cell_bwd_h"), getattr(L, f"rslrl_{kind}_cell_bwd_pair_h")
    ok = bwd()
    assert one(None, 64, None) == _lib.E_INVALID_ARGUMENT
    bads = [(bwd(**kw), 64) for kw in BAD_HIDDEN] + [(bwd(), M) for M in BAD_ROWS]  # (the reverse step never sees D)
    _refused(one, pair, ok, bads, _lib.E_UNSUPPORTED)
    invalid = [bwd(dh=None), bwd(gates=None), bwd(dg=None), bwd(whh_t_image=None),  # dg_next needs the image
               bwd(gate_stride=64 * H - 4), bwd(next_stride=64 * 256),
               bwd(dg=P * 2)]  # dg must not be dg_next: the GEMM reads whole rows of it
    invalid += [bwd(c_out=None), bwd(dc_prev=None)] if kind == "lstm" else [bwd(h_in=None), bwd(dhz_out=None)]
    _refused(one, pair, ok, [(bad, 64) for bad in invalid], _lib.E_INVALID_ARGUMENT)
    for bad in (bwd(dh=P + 4), bwd(dg_next=P * 2 + 8), bwd(whh_t_image=P * 9 + 4), bwd(dg=P * 10 + 4),
                bwd(gate_stride=64 * H + 2), bwd(next_stride=64 * H + 2)):
        assert one(ctypes.byref(bad), 64, None) == _lib.E_MISALIGNED
    # the last step of a chain: no dg_next, and then no image either -- in scope (a null dh stands for "would launch")
    assert one(ctypes.byref(bwd(dg_next=None, whh_t_image=None, dh=None)), 64, None) == _lib.E_INVALID_ARGUMENT


@pytest.mark.parametrize("kind,gates", [("lstm", 4), ("gru", 3)])
def test_image_entries(kind, gates):
    L = _lib.lib()
    nbytes, prepare = getattr(L, f"rslrl_{kind}_image_bytes_h"), getattr(L, f"rslrl_{kind}_prepare_image_h")
    for D in (0, -1, 1025):
        assert nbytes(D, H) == 0
        assert prepare(P, P, D, H, P, None) == _lib.E_UNSUPPORTED
    for hidden in (128, 256, 1024):
        assert nbytes(45, hidden) == 0
        assert prepare(P, P, 45, hidden, P, None) == _lib.E_UNSUPPORTED
    for D in (1, 15, 16, 17, 45, 48, 235, 256, 260, 1021, 1024):
        # per gate two 256-row blocks, each the image of W_ih's rows followed by that of W_hh's: no image deeper than 1024
        assert nbytes(D, H) == gates * 2 * (L.rslrl_linear_bimage_bytes(D) + L.rslrl_linear_bimage_bytes(H)), D
    assert prepare(None, P, 45, H, P, None) == _lib.E_INVALID_ARGUMENT
    assert prepare(P, None, 45, H, P, None) == _lib.E_INVALID_ARGUMENT
    assert prepare(P, P, 45, H, None, None) == _lib.E_INVALID_ARGUMENT
    assert prepare(P, P, 45, H, P + 4, None) == _lib.E_MISALIGNED
    # W_hh^T: per gate block of W_hh two 256-row images of depth 512
    tbytes, tprepare = getattr(L, f"rslrl_{kind}_whh_t_image_bytes_h"), getattr(L, f"rslrl_{kind}_prepare_whh_t_image_h")
    assert tbytes(H) == gates * 2 * L.rslrl_linear_bimage_bytes(H) == gates * L.rslrl_linear_bimage_wide_bytes(H, H)
    for hidden in (128, 256, 1024):
        assert tbytes(hidden) == 0
        assert tprepare(P, hidden, P, None) == _lib.E_UNSUPPORTED
    assert tprepare(None, H, P, None) == _lib.E_INVALID_ARGUMENT
    assert tprepare(P, H, None, None) == _lib.E_INVALID_ARGUMENT
    assert tprepare(P, H, P + 4, None) == _lib.E_MISALIGNED


GRID_M = (-64, 0, 1, 32, 63, 64, 65, 100, 128, 192, 4096, 4100)
GRID_D = (-1, 0, 1, 2, 3, 4, 5, 15, 16, 17, 40, 45, 48, 63, 64, 235, 255, 256, 257, 260, 272, 1021, 1023, 1024, 1025, 2048)


@pytest.mark.parametrize("kind", KINDS)
def test_predicates_agree_with_the_library(kind):
    L = _lib.lib()
    cell = lstm if kind == "lstm" else gru
    entry = getattr(L, f"rslrl_{kind}_cell_h")
    h_supported = getattr(kernels, f"{kind}_cell_h_supported")
    for M in GRID_M:
        for D in GRID_D:
            for hidden, layers in ((512, 1), (256, 1), (1024, 1), (512, 2)):
                # a supported problem would be launched: give it a null x and read INVALID_ARGUMENT as "in scope"
                a = cell(D=D, hidden=hidden, layers=layers, x=None)
                rc = entry(ctypes.byref(a), M, None)
                assert rc in (_lib.E_UNSUPPORTED, _lib.E_INVALID_ARGUMENT)
                assert h_supported(M, D, hidden, layers) == (rc == _lib.E_INVALID_ARGUMENT), (kind, M, D, hidden, layers)


@pytest.mark.parametrize("cell", [kernels.LSTM, kernels.GRU], ids=KINDS)
def test_takes_beside_the_unchanged_supported(cell):
    assert kernels._RNN_HIDDEN_512 == (os.environ.get("RSLRL_RNN_HIDDEN_512", "1") != "0")
    for M, D in ((64, 48), (192, 45), (4096, 235)):
        assert not cell.supported(M, D, 512, 1)
        assert cell.takes(M, D, 512, 1) == kernels._RNN_HIDDEN_512
        assert cell.takes(M, D, 256, 1) == cell.supported(M, D, 256, 1)
    for M, D, hidden, layers in ((100, 48, 512, 1), (64, 0, 512, 1), (64, 1025, 512, 1), (64, 48, 512, 2),
                                 (64, 48, 384, 1), (64, 48, 1024, 1)):
        assert not cell.takes(M, D, hidden, layers)


KNOB_SCRIPT = """
import sys
sys.path.insert(0, {root!r})
from rsl_rl_amd import kernels
assert not kernels._RNN_HIDDEN_512
for cell in (kernels.LSTM, kernels.GRU):
    for M in (0, 64, 100, 192):
        for D in (1, 16, 45, 48, 235, 1024, 1025):
            for hidden in (256, 512):
                assert cell.takes(M, D, hidden, 1) == cell.supported(M, D, hidden, 1), (M, D, hidden)
    assert not cell.takes(64, 48, 512, 1) and cell.takes(64, 48, 256, 1)
assert kernels.lstm_cell_h_supported(64, 48, 512)  # the library's scope, whatever the knob says
assert kernels._rnn_width(4 * 512, 4) == 256  # every operand is read as [M, 256] again
print("knob ok")
"""


def test_knob_restores_the_first_routing():
    """RSLRL_RNN_HIDDEN_512 is read at import: a fresh interpreter with it set to 0 has takes == supported."""
    env = dict(os.environ, RSLRL_RNN_HIDDEN_512="0")
    out = subprocess.run([sys.executable, "-c", KNOB_SCRIPT.format(root=ROOT)], env=env, capture_output=True, text=True)
    assert out.returncode == 0 and "knob ok" in out.stdout, out.stderr


def test_wrappers_read_the_width_off_the_weights():
    on = kernels._RNN_HIDDEN_512
    assert kernels._rnn_width(4 * 512, 4) == (512 if on else 256) and kernels._rnn_width(3 * 512, 3) == (512 if on else 256)
    assert kernels._rnn_width(4 * 256, 4) == 256 and kernels._rnn_width(4 * 384, 4) == 256
    assert kernels._rnn_width(64 * 512, 64) == (512 if on else 256) and kernels._rnn_width(0, 0) == 256


@pytest.mark.parametrize("rnn_type", KINDS)
def test_distillation_window_refuses_a_512_student(rnn_type, monkeypatch):
    """Distillation's recurrent predicate asks Cell.supported: with everything else granted (the part that needs a
    device is stubbed) a 256-wide student memory is taken and a 512-wide one is not."""
    from rsl_rl_amd.algorithms import Distillation
    from rsl_rl_amd.modules import StudentTeacherRecurrent

    obs = {"policy": torch.zeros(64, 48), "teacher": torch.zeros(64, 48)}
    groups = {"policy": ["policy"], "teacher": ["teacher"]}
    answers = {}
    for hidden in (256, 512):
        pol = StudentTeacherRecurrent(obs, groups, 4, student_hidden_dims=[64, 64], teacher_hidden_dims=[64, 64],
                                      rnn_type=rnn_type, rnn_hidden_dim=hidden)
        alg = Distillation(pol, device="cpu")
        alg.init_storage("distillation", 64, 4, obs, [4])
        monkeypatch.setattr(alg, "_fused_common", lambda base, mlp_width=None: 48)
        answers[hidden] = alg._fused_recurrent_ok()
    assert answers == {256: True, 512: False}


@pytest.mark.parametrize("rnn_type", KINDS)
def test_recurrent_update_stays_off_on_cpu_tensors(rnn_type):
    from rsl_rl_amd.modules import ActorCriticRecurrent

    obs = {"policy": torch.zeros(64, 48)}
    pol = ActorCriticRecurrent(obs, {"policy": ["policy"], "critic": ["policy"]}, 12, actor_hidden_dims=[512, 256, 128],
                               critic_hidden_dims=[512, 256, 128], rnn_type=rnn_type, rnn_hidden_dim=512)
    assert pol.memory_a.rnn.hidden_size == 512 and pol._cell() is kernels.cell_of(pol.memory_a.rnn)
    assert not pol.manual_update_ok(obs, 64)
    assert pol.memory_a.fused_cell(obs["policy"]) is None  # a CPU step stays on the RNN library
    tape = pol.train_tape(2, 64, "cpu")
    assert tape.mem[0].hin.shape == (2, 64, 512) and tape.mem[1].gates.shape == (4, 2, 64, 512)
