"""The fused cells' entry points for any input width (ABI 31) without a GPU: their argument validation (nothing is
launched), the Python predicates against the library, and the RSLRL_RNN_ANY_INPUT knob."""

import ctypes
import os
import subprocess
import sys

import pytest

from rsl_rl_amd import _lib, kernels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 4096  # never dereferenced: every call below is rejected on its arguments


def lstm(**kw):
    base = dict(x=P, h=P * 2, c=P * 3, image=P * 4, b_ih=P * 5, b_hh=P * 6, h_out=P * 7, c_out=P * 8, D=45,
                hidden=256, layers=1, reserved=0)
    base.update(kw)
    return _lib.LstmCell(**base)


def gru(**kw):
    base = dict(x=P, h=P * 2, image=P * 4, b_ih=P * 5, b_hh=P * 6, h_out=P * 7, D=45, hidden=256, layers=1, reserved=0)
    base.update(kw)
    return _lib.GruCell(**base)


def lstm_train(cell_kw=None, **kw):
    t = _lib.LstmTrain()
    t.cell = lstm(**(cell_kw or {}))
    t.gates, t.reset, t.gate_stride = P * 9, P * 10, 64 * 256
    for k, v in kw.items():
        setattr(t, k, v)
    return t


def gru_train(cell_kw=None, **kw):
    t = _lib.GruTrain()
    t.cell = gru(**(cell_kw or {}))
    t.gates, t.reset, t.gate_stride = P * 9, P * 10, 64 * 256
    for k, v in kw.items():
        setattr(t, k, v)
    return t


BAD_SHAPES = ((dict(hidden=128), 64), (dict(hidden=512), 64), (dict(layers=2), 64), (dict(layers=0), 64),
              (dict(D=0), 64), (dict(D=-3), 64), (dict(D=1025), 64), (dict(), 0), (dict(), 100), (dict(), 32),
              (dict(), -64))


def test_abi_is_at_least_31():
    assert _lib.lib().rslrl_abi_version() == _lib.ABI_VERSION >= 31


@pytest.mark.parametrize("kind", ["lstm", "gru"])
def test_cell_entries_refuse_bad_problems_before_any_launch(kind):
    L = _lib.lib()
    cell = lstm if kind == "lstm" else gru
    one, pair = getattr(L, f"rslrl_{kind}_cell_anyd"), getattr(L, f"rslrl_{kind}_cell_pair_anyd")
    ok = cell()
    assert one(None, 64, None) == _lib.E_INVALID_ARGUMENT
    assert pair(None, ctypes.byref(ok), 64, None) == _lib.E_INVALID_ARGUMENT
    for kw, M in BAD_SHAPES:
        bad = cell(**kw)
        assert one(ctypes.byref(bad), M, None) == _lib.E_UNSUPPORTED, (kw, M)
        assert pair(ctypes.byref(ok), ctypes.byref(bad), M, None) == _lib.E_UNSUPPORTED, (kw, M)
        assert pair(ctypes.byref(bad), ctypes.byref(ok), M, None) == _lib.E_UNSUPPORTED, (kw, M)
    nulls = [dict(x=None), dict(image=None), dict(b_ih=None), dict(b_hh=None), dict(h_out=None)]
    nulls += [dict(h_out=P * 2)]  # h_out must not be h
    if kind == "lstm":
        nulls += [dict(c_out=None), dict(h_out=P * 8)]  # nor c_out
    for kw in nulls:
        bad = cell(**kw)
        assert one(ctypes.byref(bad), 64, None) == _lib.E_INVALID_ARGUMENT, kw
        assert pair(ctypes.byref(ok), ctypes.byref(bad), 64, None) == _lib.E_INVALID_ARGUMENT, kw
        assert pair(ctypes.byref(bad), ctypes.byref(ok), 64, None) == _lib.E_INVALID_ARGUMENT, kw
    # alignment: 16 bytes for everything but x, whose base needs 4 bytes where D % 4 != 0 and 16 where D % 4 == 0
    for kw in (dict(h=P * 2 + 4), dict(image=P * 4 + 8), dict(b_ih=P * 5 + 4), dict(h_out=P * 7 + 4), dict(x=P + 2),
               dict(x=P + 4, D=40), dict(x=P + 8, D=260)):
        bad = cell(**kw)
        assert one(ctypes.byref(bad), 64, None) == _lib.E_MISALIGNED, kw
        assert pair(ctypes.byref(ok), ctypes.byref(bad), 64, None) == _lib.E_MISALIGNED, kw


@pytest.mark.parametrize("kind", ["lstm", "gru"])
def test_train_entries_refuse_bad_problems_before_any_launch(kind):
    L = _lib.lib()
    train = lstm_train if kind == "lstm" else gru_train
    one, pair = getattr(L, f"rslrl_{kind}_cell_train_anyd"), getattr(L, f"rslrl_{kind}_cell_train_pair_anyd")
    ok = train()
    assert one(None, 64, None) == _lib.E_INVALID_ARGUMENT
    for kw, M in BAD_SHAPES:
        bad = train(kw)
        assert one(ctypes.byref(bad), M, None) == _lib.E_UNSUPPORTED, (kw, M)
        assert pair(ctypes.byref(ok), ctypes.byref(bad), M, None) == _lib.E_UNSUPPORTED, (kw, M)
        assert pair(ctypes.byref(bad), ctypes.byref(ok), M, None) == _lib.E_UNSUPPORTED, (kw, M)
    invalid = [train(dict(x=None)), train(gates=None), train(gate_stride=64 * 256 - 4),
               train(h_in_out=P * 2),   # the h other blocks read
               train(h_in_out=P * 7),   # h_out
               train(h_in_out=P * 11, h_restart=P * 11), train(h_restart=P * 7)]
    if kind == "lstm":
        invalid += [train(h_in_out=P * 3), train(h_in_out=P * 8), train(h_in_out=P * 11, c_restart=P * 11)]
    for bad in invalid:
        assert one(ctypes.byref(bad), 64, None) == _lib.E_INVALID_ARGUMENT
        assert pair(ctypes.byref(ok), ctypes.byref(bad), 64, None) == _lib.E_INVALID_ARGUMENT
        assert pair(ctypes.byref(bad), ctypes.byref(ok), 64, None) == _lib.E_INVALID_ARGUMENT
    for bad in (train(gates=P * 9 + 4), train(gate_stride=64 * 256 + 2), train(h_restart=P * 11 + 4),
                train(h_in_out=P * 11 + 8), train(dict(x=P + 4, D=44))):
        assert one(ctypes.byref(bad), 64, None) == _lib.E_MISALIGNED


@pytest.mark.parametrize("kind,gates", [("lstm", 4), ("gru", 3)])
def test_image_entries(kind, gates):
    L = _lib.lib()
    nbytes, prepare = getattr(L, f"rslrl_{kind}_image_bytes_anyd"), getattr(L, f"rslrl_{kind}_prepare_image_anyd")
    for D in (0, -1, 1025):
        assert nbytes(D) == 0
        assert prepare(P, P, D, 256, P, None) == _lib.E_UNSUPPORTED
    for D in (1, 15, 16, 17, 45, 235, 256, 260, 1021, 1024):
        depth = -(-D // 16) * 16 + 256  # the W_ih part ceil(D / 16) chunks deep, then W_hh's 16
        assert nbytes(D) == gates * L.rslrl_linear_bimage_bytes(depth), D
    for D in (16, 48, 256):  # the first entry's widths: the first entry's image
        assert nbytes(D) == getattr(L, f"rslrl_{kind}_image_bytes")(D)
    assert prepare(P, P, 45, 128, P, None) == _lib.E_UNSUPPORTED
    assert prepare(None, P, 45, 256, P, None) == _lib.E_INVALID_ARGUMENT
    assert prepare(P, None, 45, 256, P, None) == _lib.E_INVALID_ARGUMENT
    assert prepare(P, P, 45, 256, None, None) == _lib.E_INVALID_ARGUMENT
    assert prepare(P, P, 45, 256, P + 4, None) == _lib.E_MISALIGNED


GRID_M = (-64, 0, 1, 32, 63, 64, 65, 100, 128, 192, 4096, 4100)
GRID_D = (-1, 0, 1, 2, 3, 4, 5, 15, 16, 17, 40, 45, 48, 63, 64, 235, 255, 256, 257, 260, 272, 1021, 1023, 1024, 1025, 2048)


@pytest.mark.parametrize("kind", ["lstm", "gru"])
def test_predicates_agree_with_the_library(kind):
    L = _lib.lib()
    cell = lstm if kind == "lstm" else gru
    new, first = getattr(L, f"rslrl_{kind}_cell_anyd"), getattr(L, f"rslrl_{kind}_cell")
    supported = getattr(kernels, f"{kind}_cell_supported")
    anyd_supported = getattr(kernels, f"{kind}_cell_anyd_supported")
    for M in GRID_M:
        for D in GRID_D:
            for hidden, layers in ((256, 1), (512, 1), (256, 2)):
                # a supported problem would be launched: give it a null x and read INVALID_ARGUMENT as "in scope"
                a = cell(D=D, hidden=hidden, layers=layers, x=None)
                for entry, pred in ((new, anyd_supported), (first, supported)):
                    rc = entry(ctypes.byref(a), M, None)
                    assert rc in (_lib.E_UNSUPPORTED, _lib.E_INVALID_ARGUMENT)
                    assert pred(M, D, hidden, layers) == (rc == _lib.E_INVALID_ARGUMENT), (kind, M, D, hidden, layers)
    # the first entry points and predicates answer as before
    assert not supported(64, 40, 256) and not supported(64, 45, 256) and not supported(64, 272, 256)
    assert anyd_supported(64, 40, 256) and anyd_supported(64, 45, 256) and anyd_supported(64, 1024, 256)
    assert getattr(L, f"rslrl_{kind}_image_bytes")(40) == 0


KNOB_SCRIPT = """
import sys
sys.path.insert(0, {root!r})
from rsl_rl_amd import kernels
grid = [(M, D) for M in (0, 64, 100, 192) for D in (1, 16, 40, 45, 48, 235, 256, 260, 272, 1024, 1025)]
for M, D in grid:
    assert kernels.lstm_cell_anyd_supported(M, D, 256) == kernels.lstm_cell_supported(M, D, 256), (M, D)
    assert kernels.gru_cell_anyd_supported(M, D, 256) == kernels.gru_cell_supported(M, D, 256), (M, D)
assert kernels.lstm_cell_supported(64, 48, 256) and not kernels.lstm_cell_anyd_supported(64, 45, 256)
assert not kernels._rnn_anyd(45) and not kernels._rnn_anyd(48, 53)
print("knob ok")
"""


def test_knob_restores_the_first_routing():
    """RSLRL_RNN_ANY_INPUT is read at import: a fresh interpreter with it set to 0 answers as lstm_cell_supported."""
    assert kernels._RNN_ANY_INPUT == (os.environ.get("RSLRL_RNN_ANY_INPUT", "1") != "0")
    env = dict(os.environ, RSLRL_RNN_ANY_INPUT="0")
    out = subprocess.run([sys.executable, "-c", KNOB_SCRIPT.format(root=ROOT)], env=env, capture_output=True, text=True)
    assert out.returncode == 0 and "knob ok" in out.stdout, out.stderr
    if kernels._RNN_ANY_INPUT:
        assert kernels._rnn_anyd(45) and kernels._rnn_anyd(48, 53) and not kernels._rnn_anyd(48) \
            and not kernels._rnn_anyd(48, 240)
