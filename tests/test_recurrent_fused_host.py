"""The fused recurrent PPO update without a GPU: RolloutStorage.recurrent_sequence_generator against
the padded form (every padded trajectory of the reference's mini-batch is a run of rows of the env-major slice, and its
first hidden state is the restart row at its start), the sequence formulation's gradient under CPU autograd against the
reference's first-mini-batch gradient, and the ABI 27 entry points' argument validation (nothing is launched)."""

import ctypes

import numpy as np
import pytest
import torch

import recurrent_fixtures as RF
import recurrent_fused_fixtures as RFF
from rsl_rl_amd import _lib
from test_recurrent_host import GEN_CASES, META, gen_storage

META_D = RFF.load_meta()
FIELDS = ("actions", "values", "advantages", "returns", "actions_log_prob", "mu", "sigma")


def check_sequences_cover_the_padded_form(st, M):
    T, N = st.num_transitions_per_env, st.num_envs
    E = N // M
    padded = list(st.recurrent_mini_batch_generator(M, 1))
    seqs = list(st.recurrent_sequence_generator(M, 1))
    assert len(seqs) == M and all(len(b) == 10 for b in seqs)
    dones = st.dones.reshape(T, N)
    for i, (pad, seq) in enumerate(zip(padded, seqs)):
        s = slice(i * E, (i + 1) * E)
        obs_p, *fields_p, (hid_ap, hid_cp), masks = pad
        obs_s, *fields_s, (hid_as, hid_cs), reset = seq
        assert reset.dtype == torch.uint8 and tuple(reset.shape) == (T, E) and reset.is_contiguous()
        assert not reset[0].any() and torch.equal(reset[1:], (dones[:T - 1, s] != 0).to(torch.uint8))
        for name, a, b in zip(FIELDS, fields_p, fields_s):  # the other fields: the reference's own [T, E, ...] slices
            assert torch.equal(a, b) and b.is_contiguous(), (i, name)
        for k in obs_s.keys():
            assert torch.equal(obs_s[k], st.observations[k][:, s]) and obs_s[k].is_contiguous()
        pairs = []
        for hp, hs in ((hid_ap, hid_as), (hid_cp, hid_cs)):
            assert isinstance(hs, tuple) == isinstance(hp, tuple)  # (h, c) for LSTM, a bare tensor for GRU
            pairs += list(zip(hp, hs)) if isinstance(hp, tuple) else [(hp, hs)]
        j = 0
        for n in range(E):
            t0 = 0
            while t0 < T:
                length = int(masks[:, j].sum())
                assert length > 0 and masks[:length, j].all()
                assert bool(reset[t0, n]) == (t0 > 0) and not reset[t0 + 1:t0 + length, n].any(), (i, n, t0)
                for k in obs_s.keys():  # the padded trajectory is this run of rows, then zeros
                    assert torch.equal(obs_p[k][:length, j], obs_s[k][t0:t0 + length, n]), (i, j, k)
                    assert not obs_p[k][length:, j].any()
                for hp, hs in pairs:  # hp [L, n_traj, H]; hs [T, E, H] (L 1) or [T, L, E, H]
                    row = hs[t0, n].unsqueeze(0) if hs.dim() == 3 else hs[t0, :, n]
                    assert torch.equal(hp[:, j], row), (i, j)
                t0 += length
                j += 1
        assert j == masks.shape[1]
    # every epoch walks the same objects: the contiguous copies are made once
    two = list(st.recurrent_sequence_generator(M, 2))
    assert len(two) == 2 * M and all(two[k][1] is two[M + k][1] and two[k][0] is two[M + k][0] for k in range(M))


@pytest.mark.parametrize("case", GEN_CASES)
def test_sequences_cover_the_padded_trajectories(case):
    st, _, m = gen_storage(case)
    check_sequences_cover_the_padded_form(st, m["M"])


def test_sequences_cover_the_padded_trajectories_of_rec_a():
    meta = META["rec_a"]
    alg, _ = RF.build_update(RF.Arrays(meta["files"]), meta, "cpu", compute_returns=False)
    check_sequences_cover_the_padded_form(alg.storage, meta["M"])


def test_generator_refuses_what_the_padded_one_refuses():
    st, _, m = gen_storage(GEN_CASES[0])
    st.saved_hidden_states_a = None
    with pytest.raises(ValueError):
        next(st.recurrent_sequence_generator(m["M"], 1))


@pytest.mark.parametrize("case", ["rec_a", "rec_c", "rec_d"])
def test_sequence_gradient_matches_the_reference_on_cpu(case):
    """The formulation itself, in plain torch under CPU autograd: the first mini-batch's gradient within 1e-5 of its
    max of the reference's (the project's bound for that quantity)."""
    meta = META_D[case] if case in META_D else META[case]
    z = RF.Arrays(meta["files"])
    torch.set_num_threads(1)
    alg, pol = RFF.build_update_cpu(z, meta)
    batch = next(iter(alg.storage.recurrent_sequence_generator(meta["M"], 1)))
    loss = RFF.sequence_loss(alg, pol, batch)
    grads = torch.autograd.grad(loss, list(pol.parameters()))
    ours = torch.cat([g.reshape(-1) for g in grads]).double()
    ref = torch.from_numpy(z["r0/grad_mb0"]).double()
    err = (ours - ref).abs().max().item() / ref.abs().max().item()
    print(case, "first mini-batch gradient error / max:", f"{err:.2e}")
    assert err <= 1e-5, (case, err)


def test_rec_d_fixture_exercises_every_restart():
    meta = META_D["rec_d"]
    assert (meta["T"], meta["N"], meta["M"], meta["H"], meta["L"]) == (8, 128, 2, 256, 1)
    nz = RF.storage_inputs(meta["ranks"][0]["noise_seed"], meta["T"], meta["N"], meta["O"], meta["A"], 1, 256, 2)
    assert RF.inputs_digest(nz) == meta["ranks"][0]["inputs_sha256"]
    d = nz["dones"][:, :, 0].astype(bool)
    E = meta["N"] // meta["M"]
    assert E % 64 == 0
    for i in range(meta["M"]):
        s = d[:, i * E:(i + 1) * E]
        assert (~s.any(axis=0)).any() and s[0].any() and s[-1].any() and (s[:-1] & s[1:]).any()
    assert meta["ranks"][0]["lr_trace"] == [0.0015] * 4


# ------------------------------------------------------------------------------------------------------- C ABI
P = 4096  # never dereferenced: every call below is rejected on its arguments


def _train(**kw):
    cell = dict(x=P, h=P * 2, c=P * 3, image=P * 4, b_ih=P * 5, b_hh=P * 6, h_out=P * 7, c_out=P * 8, D=48, hidden=256,
                layers=1, reserved=0)
    top = dict(gates=P * 9, reset=P * 10, gate_stride=64 * 256, h_restart=P * 11, c_restart=P * 12, h_in_out=P * 13)
    for k, v in kw.items():
        (cell if k in cell else top)[k] = v
    return _lib.LstmTrain(cell=_lib.LstmCell(**cell), **top)


def _bwd(**kw):
    base = dict(dh=P, dg_next=P * 2, dc_next=P * 3, reset_next=P * 4, gates=P * 5, c_out=P * 6, c_prev=P * 7,
                reset_cur=P * 8, whh_t_image=P * 9, dg=P * 10, dc_prev=P * 11, gate_stride=64 * 256,
                next_stride=64 * 256, hidden=256, layers=1, c_restart=P * 12)
    base.update(kw)
    return _lib.LstmBwd(**base)


def test_abi_27_symbols_and_struct_tails():
    L = _lib.lib()
    assert L.rslrl_abi_version() == _lib.ABI_VERSION >= 27
    for name in ("rslrl_lstm_cell_train_pair", "rslrl_lstm_cell_bwd_pair"):
        assert hasattr(L, name), name
    # appended at the end: every ABI 26 field keeps its offset, and a zero-initialised mirror reads as ABI 26
    assert [f[0] for f in _lib.LstmTrain._fields_][-3:] == ["h_restart", "c_restart", "h_in_out"]
    assert _lib.LstmTrain.h_restart.offset == _lib.LstmTrain.gate_stride.offset + 8
    assert _lib.LstmBwd._fields_[-1][0] == "c_restart"
    assert _lib.LstmBwd.c_restart.offset == _lib.LstmBwd.layers.offset + 4
    t, b = _lib.LstmTrain(), _lib.LstmBwd()
    assert t.h_restart is None and t.c_restart is None and t.h_in_out is None and b.c_restart is None


def test_pair_entry_points_refuse_before_any_launch():
    L = _lib.lib()
    ok_t, ok_b = _train(), _bwd()
    tp, bp = L.rslrl_lstm_cell_train_pair, L.rslrl_lstm_cell_bwd_pair
    assert tp(None, None, 64, None) == _lib.E_INVALID_ARGUMENT
    assert bp(None, None, 64, None) == _lib.E_INVALID_ARGUMENT
    for kw, M in ((dict(hidden=128), 64), (dict(D=40), 64), (dict(), 100), (dict(layers=2), 64), (dict(D=272), 64),
                  (dict(D=0), 64), (dict(), 0), (dict(), 96)):
        bad = _train(**kw)
        assert L.rslrl_lstm_cell_train(ctypes.byref(bad), M, None) == _lib.E_UNSUPPORTED, (kw, M)
        assert tp(ctypes.byref(ok_t), ctypes.byref(bad), M, None) == _lib.E_UNSUPPORTED, (kw, M)
        assert tp(ctypes.byref(bad), ctypes.byref(ok_t), M, None) == _lib.E_UNSUPPORTED, (kw, M)
    for kw, M in ((dict(hidden=128), 64), (dict(layers=2), 64), (dict(), 100), (dict(), 0)):
        bad = _bwd(**kw)
        assert L.rslrl_lstm_cell_bwd(ctypes.byref(bad), M, None) == _lib.E_UNSUPPORTED, (kw, M)
        assert bp(ctypes.byref(ok_b), ctypes.byref(bad), M, None) == _lib.E_UNSUPPORTED, (kw, M)
        assert bp(ctypes.byref(bad), ctypes.byref(ok_b), M, None) == _lib.E_UNSUPPORTED, (kw, M)
    # the second problem is validated like the first: pointers, aliasing, alignment
    for kw in (dict(gates=None), dict(x=None), dict(h_in_out=P * 2), dict(h_in_out=P * 3), dict(h_in_out=P * 11), dict(h_in_out=P * 12),
               dict(h_in_out=P * 7), dict(h_in_out=P * 8),
               dict(h_restart=P * 7), dict(gate_stride=64 * 256 - 4)):
        assert tp(ctypes.byref(ok_t), ctypes.byref(_train(**kw)), 64, None) == _lib.E_INVALID_ARGUMENT, kw
    for kw in (dict(h_restart=P + 4), dict(c_restart=P + 8), dict(h_in_out=P + 4), dict(gate_stride=64 * 256 + 2)):
        assert tp(ctypes.byref(ok_t), ctypes.byref(_train(**kw)), 64, None) == -4, kw
    for kw in (dict(dh=None), dict(dg=None), dict(dg=P * 2), dict(whh_t_image=None), dict(gate_stride=64)):
        assert bp(ctypes.byref(ok_b), ctypes.byref(_bwd(**kw)), 64, None) == _lib.E_INVALID_ARGUMENT, kw
    for kw in (dict(c_restart=P + 4), dict(c_prev=P + 4)):
        assert bp(ctypes.byref(ok_b), ctypes.byref(_bwd(**kw)), 64, None) == -4, kw
