"""Recurrent PPO without a GPU: the torch forms of split / pad / unpad and the CPU generator against the reference's
fixtures (bit for bit), Memory's reset semantics, ActorCriticRecurrent's checkpoint surface, the runner's class
table, the refusals, and the argument validation of the trajectory entry points (nothing is launched)."""

import ctypes
import os
import warnings

import numpy as np
import pytest
import torch

import recurrent_fixtures as RF
from rsl_rl_amd import _lib
from rsl_rl_amd.algorithms import PPO
from rsl_rl_amd.modules import ActorCriticRecurrent
from rsl_rl_amd.networks import Memory
from rsl_rl_amd.storage import RolloutStorage
from rsl_rl_amd.utils import TensorDict, split_and_pad_trajectories, unpad_trajectories

META = RF.load_meta()
GEN_CASES = sorted(META["generator"])
FIELDS = ("actions", "values", "advantages", "returns", "actions_log_prob", "mu", "sigma")


def gen_storage(case, device="cpu"):
    m = META["generator"][case]
    z = np.load(os.path.join(RF.GOLDEN, m["file"]))
    T, N, A = m["T"], m["N"], m["A"]
    obs0 = TensorDict({k: torch.zeros(N, w) for k, w in m["widths"].items()}, batch_size=[N])
    st = RolloutStorage("rl", N, T, obs0, [A], device)
    for k in m["widths"]:
        st.observations[k].copy_(torch.from_numpy(z["in/obs/" + k]))
    for name in FIELDS:
        getattr(st, name).copy_(torch.from_numpy(z["in/" + name]))
    st.dones.copy_(torch.from_numpy(z["in/dones"]))
    for net in "ac":
        setattr(st, "saved_hidden_states_" + net,
                [torch.from_numpy(z[f"in/hid_{net}{i}"]).to(device) for i in range(m["n_states"])])
    st.step = T
    return st, z, m


def check_generator(st, z, m):
    """One epoch of st.recurrent_mini_batch_generator against the fixture, bit for bit."""
    batches = list(st.recurrent_mini_batch_generator(m["M"], 1))
    assert len(batches) == m["M"]
    for i, batch in enumerate(batches):
        assert len(batch) == 10
        obs_b, *fields, (hid_a, hid_c), masks_b = batch
        for k in m["widths"]:
            ref = z[f"mb{i}/obs/{k}"]
            assert tuple(obs_b[k].shape) == ref.shape and np.array_equal(obs_b[k].cpu().numpy(), ref), (i, k)
        for name, f in zip(FIELDS, fields):
            ref = z[f"mb{i}/{name}"]
            assert tuple(f.shape) == ref.shape and np.array_equal(f.cpu().numpy(), ref), (i, name)
        assert masks_b.dtype == torch.bool and np.array_equal(masks_b.cpu().numpy(), z[f"mb{i}/masks"]), i
        assert masks_b.shape[1] == m["traj_counts"][i]
        for net, hid in (("a", hid_a), ("c", hid_c)):
            if m["n_states"] == 1:
                assert isinstance(hid, torch.Tensor)  # GRU: a bare tensor
                hid = (hid,)
            else:
                assert isinstance(hid, (tuple, list)) and len(hid) == 2
            for j, h in enumerate(hid):
                ref = z[f"mb{i}/hid_{net}{j}"]
                assert tuple(h.shape) == ref.shape and np.array_equal(h.cpu().numpy(), ref), (i, net, j)
    return batches


@pytest.mark.parametrize("case", GEN_CASES)
def test_split_pad_unpad_match_the_reference(case):
    st, z, m = gen_storage(case)
    padded, masks = split_and_pad_trajectories(st.observations, st.dones)
    assert list(padded.batch_size) == [m["T"], m["n_traj"]]
    for k in m["widths"]:
        assert np.array_equal(padded[k].numpy(), z["pad/" + k]), k
        single, masks1 = split_and_pad_trajectories(st.observations[k], st.dones)
        assert torch.equal(single, padded[k]) and torch.equal(masks1, masks)
        assert torch.equal(unpad_trajectories(padded[k], masks), st.observations[k])  # unpad(pad(x)) == x
    assert masks.dtype == torch.bool and np.array_equal(masks.numpy(), z["pad/masks"])


@pytest.mark.parametrize("case", GEN_CASES)
def test_cpu_generator_matches_the_reference(case):
    st, z, m = gen_storage(case)
    check_generator(st, z, m)
    # every epoch walks the same mini-batches
    assert len(list(st.recurrent_mini_batch_generator(m["M"], 2))) == 2 * m["M"]


def test_unpad_of_random_dones_round_trips():
    g = torch.Generator().manual_seed(3)
    x = torch.randn(11, 37, 5, generator=g)
    dones = (torch.rand(11, 37, 1, generator=g) < 0.2).to(torch.uint8)
    padded, masks = split_and_pad_trajectories(x, dones)
    assert padded.shape[0] == 11 and masks.sum() == 11 * 37
    assert (padded[~masks] == 0).all()
    assert torch.equal(unpad_trajectories(padded, masks), x)


@pytest.mark.parametrize("rnn", ["lstm", "gru"])
def test_memory_reset_and_detach(rnn):
    torch.manual_seed(0)
    mem = Memory(6, type=rnn, num_layers=2, hidden_size=5)
    assert mem.hidden_states is None
    mem.reset(torch.tensor([1, 0, 1]))  # nothing to reset yet
    out = mem(torch.randn(3, 6))
    assert out.shape == (1, 3, 5)
    states = mem.hidden_states if rnn == "lstm" else (mem.hidden_states,)
    assert isinstance(mem.hidden_states, tuple) == (rnn == "lstm")
    before = [s.detach().clone() for s in states]
    dones = torch.tensor([1, 0, 1])
    mem.reset(dones)
    states = mem.hidden_states if rnn == "lstm" else (mem.hidden_states,)
    for s, b in zip(states, before):
        assert (s[:, [0, 2]] == 0.0).all() and torch.equal(s[:, 1], b[:, 1])
    # detach of done rows: same values, no gradient through those rows
    mem(torch.randn(3, 6))
    keep = [s.clone() for s in (mem.hidden_states if rnn == "lstm" else (mem.hidden_states,))]
    mem.detach_hidden_states(dones)
    states = mem.hidden_states if rnn == "lstm" else (mem.hidden_states,)
    for s, k in zip(states, keep):
        assert torch.equal(s, k) and s.requires_grad
    (g,) = torch.autograd.grad(states[0].sum(), mem.rnn.weight_hh_l0, retain_graph=True)
    assert torch.isfinite(g).all()
    mem.detach_hidden_states()
    states = mem.hidden_states if rnn == "lstm" else (mem.hidden_states,)
    assert all(not s.requires_grad for s in states)
    mem.reset()
    assert mem.hidden_states is None
    with pytest.raises(ValueError):
        mem(torch.randn(4, 3, 6), masks=torch.ones(4, 3, dtype=torch.bool))


def _policy(rnn="lstm", std="scalar", norm=False, **kw):
    obs0 = TensorDict({"policy": torch.zeros(2, 16)}, batch_size=[2])
    groups = {"policy": ["policy"], "critic": ["policy"]}
    return ActorCriticRecurrent(obs0, groups, 4, actor_hidden_dims=[32], critic_hidden_dims=[32], rnn_type=rnn,
                                rnn_hidden_dim=16, rnn_num_layers=2, noise_std_type=std, actor_obs_normalization=norm,
                                critic_obs_normalization=norm, **kw)


@pytest.mark.parametrize("key", sorted(META["state_dict_keys"]))
def test_state_dict_keys_match_the_reference(key):
    rnn, std, norm = key.split("_")
    pol = _policy(rnn, std, norm == "norm")
    ref = META["state_dict_keys"][key]
    assert list(pol.state_dict().keys()) == ref["state_dict"]
    assert [n for n, _ in pol.named_parameters()] == ref["parameters"]
    assert "memory_a.rnn.weight_ih_l0" in ref["state_dict"]


@pytest.mark.parametrize("case", ["rec_a", "rec_b"])
def test_reference_parameters_load_strictly(case):
    meta = META[case]
    z = RF.Arrays(meta["files"])
    obs0 = {"policy": torch.zeros(meta["N"], meta["O"])}
    pol = ActorCriticRecurrent(obs0, {"policy": ["policy"], "critic": ["policy"]}, meta["A"], **RF.policy_kwargs(meta))
    sd = {k[len("r0/init/"):]: torch.from_numpy(z[k]) for k in z.files if k.startswith("r0/init/")}
    assert pol.load_state_dict(sd, strict=True) is True
    assert pol.is_recurrent and pol.get_hidden_states() == (None, None)


def test_rnn_hidden_size_is_deprecated():
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        obs0 = {"policy": torch.zeros(2, 6)}
        pol = ActorCriticRecurrent(obs0, {"policy": ["policy"], "critic": ["policy"]}, 2, actor_hidden_dims=[8],
                                   critic_hidden_dims=[8], rnn_hidden_size=12)
    assert any(issubclass(x.category, DeprecationWarning) for x in w)
    assert pol.memory_a.rnn.hidden_size == 12


def test_runner_resolves_the_class():
    from rsl_rl_amd.runners.on_policy_runner import _resolve_class
    assert _resolve_class("ActorCriticRecurrent") is ActorCriticRecurrent


def test_symmetry_and_rnd_are_refused():
    sym = {"use_data_augmentation": True, "use_mirror_loss": False, "data_augmentation_func": lambda **k: None}
    with pytest.raises(NotImplementedError, match="ppo.py"):
        PPO(_policy(), device="cpu", symmetry_cfg=sym)
    with pytest.raises(NotImplementedError, match="ppo.py"):
        PPO(_policy(), device="cpu", rnd_cfg={"num_states": 16})


def test_cpu_batch_forward_reproduces_the_stored_rollout():
    """GAE and the loss kernel need the GPU; the generator, the memories and the unpadding of an update fixture run
    here on CPU tensors through one batch-mode forward of the first mini-batch."""
    meta = META["rec_a"]
    z = RF.Arrays(meta["files"])
    alg, pol = RF.build_update(z, meta, "cpu", compute_returns=False)
    batch = next(iter(alg.storage.recurrent_mini_batch_generator(meta["M"], 1)))
    obs_b, actions_b, *_, (hid_a, hid_c), masks_b = batch
    pol.act(obs_b, masks=masks_b, hidden_states=hid_a)
    E = meta["N"] // meta["M"]
    assert pol.action_mean.shape == (meta["T"], E, meta["A"])
    # rollout-consistent fixture: the mean equals the stored (fp16-rounded) one up to that rounding
    stored = alg.storage.mu[:, :E]
    assert (pol.action_mean - stored).abs().max() <= 1e-3 * (1 + stored.abs().max())
    assert pol.evaluate(obs_b, masks=masks_b, hidden_states=hid_c).shape == (meta["T"], E, 1)


def test_trajectory_entry_points_validate_before_any_launch():
    L = _lib.lib()
    assert L.rslrl_abi_version() == _lib.ABI_VERSION >= 25
    p = 4096  # never dereferenced: every call below is rejected on its arguments
    ia = _lib.TrajectoryIndexArgs(p, 8, 12, 3, p, p, p, p)
    assert L.rslrl_trajectory_index(None, p, 1 << 20, None) == _lib.E_INVALID_ARGUMENT
    assert L.rslrl_trajectory_index(ctypes.byref(ia), None, 0, None) == _lib.E_INVALID_ARGUMENT
    assert L.rslrl_trajectory_index(ctypes.byref(ia), p, 0, None) == -2  # workspace too small
    for field, bad in (("dones", None), ("traj_id", None), ("bounds", None), ("T", 0), ("N", -1),
                       ("num_mini_batches", 0), ("num_mini_batches", 13)):
        a = _lib.TrajectoryIndexArgs(p, 8, 12, 3, p, p, p, p)
        setattr(a, field, bad)
        assert L.rslrl_trajectory_index(ctypes.byref(a), p, 1 << 20, None) == _lib.E_INVALID_ARGUMENT, field
    assert L.rslrl_trajectory_index_workspace_bytes(24, 131072) >= 4 * 512
    assert L.rslrl_trajectory_index_workspace_bytes(0, 4) == 0

    def pad_args(**kw):
        a = _lib.TrajectoryPadArgs()
        a.T, a.N, a.num_mini_batches, a.n_traj = 8, 12, 3, 20
        a.traj_id, a.traj_off, a.bounds, a.masks = p, p, p, p
        a.num_groups = 1
        a.groups[0].src, a.groups[0].dst, a.groups[0].src_stride, a.groups[0].width = p, p, 8, 8
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    assert L.rslrl_trajectory_pad(None, None) == _lib.E_INVALID_ARGUMENT
    for kw in (dict(T=0), dict(N=0), dict(traj_id=None), dict(masks=None), dict(num_groups=5), dict(num_states=5),
               dict(n_traj=-1), dict(n_traj=97), dict(num_states=1)):
        assert L.rslrl_trajectory_pad(ctypes.byref(pad_args(**kw)), None) == _lib.E_INVALID_ARGUMENT, kw
    a = pad_args()
    a.groups[0].src = None
    assert L.rslrl_trajectory_pad(ctypes.byref(a), None) == _lib.E_INVALID_ARGUMENT
    a = pad_args()
    a.groups[0].src_stride = 4  # rows narrower than the group
    assert L.rslrl_trajectory_pad(ctypes.byref(a), None) == _lib.E_INVALID_ARGUMENT
    assert L.rslrl_trajectory_pad(ctypes.byref(pad_args(n_traj=0)), None) == 0  # nothing to do, nothing launched

    assert L.rslrl_trajectory_unpad(None, None) == _lib.E_INVALID_ARGUMENT
    for kw in (dict(padded=None), dict(flat=None), dict(T=0), dict(N=0), dict(envs=0), dict(env0=9), dict(first=-1),
               dict(n_b=0), dict(width=0)):
        base = dict(padded=p, flat=p, traj_id=p, traj_off=p, T=8, N=12, envs=4, env0=4, first=0, n_b=7, width=8,
                    scatter=0)
        base.update(kw)
        u = _lib.TrajectoryUnpadArgs(**base)
        assert L.rslrl_trajectory_unpad(ctypes.byref(u), None) == _lib.E_INVALID_ARGUMENT, kw


def test_lstm_cell_entry_points_validate_before_any_launch():
    L = _lib.lib()
    p = 4096  # never dereferenced

    def cell(**kw):
        base = dict(x=p, h=p * 2, c=p * 3, image=p * 4, b_ih=p * 5, b_hh=p * 6, h_out=p * 7, c_out=p * 8, D=48,
                    hidden=256, layers=1, reserved=0)
        base.update(kw)
        return _lib.LstmCell(**base)

    ok = cell()
    assert L.rslrl_lstm_cell(None, 64, None) == _lib.E_INVALID_ARGUMENT
    for kw, M in ((dict(hidden=128), 64), (dict(D=40), 64), (dict(), 100), (dict(layers=2), 64), (dict(D=272), 64),
                  (dict(D=0), 64), (dict(), 0)):
        bad = cell(**kw)
        assert L.rslrl_lstm_cell(ctypes.byref(bad), M, None) == _lib.E_UNSUPPORTED, (kw, M)
        assert L.rslrl_lstm_cell_pair(ctypes.byref(ok), ctypes.byref(bad), M, None) == _lib.E_UNSUPPORTED, (kw, M)
        assert L.rslrl_lstm_cell_pair(ctypes.byref(bad), ctypes.byref(ok), M, None) == _lib.E_UNSUPPORTED, (kw, M)
    for kw in (dict(x=None), dict(image=None), dict(b_ih=None), dict(h_out=None), dict(c_out=None),
               dict(h_out=p * 2)):  # h_out must not be h
        assert L.rslrl_lstm_cell(ctypes.byref(cell(**kw)), 64, None) == _lib.E_INVALID_ARGUMENT, kw
    assert L.rslrl_lstm_cell(ctypes.byref(cell(x=p + 4)), 64, None) == -4  # misaligned
    assert L.rslrl_lstm_image_bytes(40) == 0 and L.rslrl_lstm_image_bytes(272) == 0
    assert L.rslrl_lstm_image_bytes(48) == 4 * L.rslrl_linear_bimage_bytes(48 + 256)
    assert L.rslrl_lstm_prepare_image(p, p, 40, 256, p, None) == _lib.E_UNSUPPORTED
    assert L.rslrl_lstm_prepare_image(p, p, 48, 64, p, None) == _lib.E_UNSUPPORTED
    assert L.rslrl_lstm_prepare_image(None, p, 48, 256, p, None) == _lib.E_INVALID_ARGUMENT
