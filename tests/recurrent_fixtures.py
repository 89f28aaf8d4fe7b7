"""Helpers of the recurrent-policy fixtures (tests/golden/make_golden_recurrent.py writes them; the tests and that
script share what is here): the seeded storage inputs, the loader of arrays split over several files, and the rebuild
of a fixture's PPO + storage on any device."""

import hashlib
import json
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PART_BYTES = 900 * 1024  # an array larger than this is stored as row blocks "<key>@<i>"


def storage_inputs(seed, T, N, O, A, L, H, n_states, p_done=0.08):
    """The policy-independent storage inputs from a numpy PCG64 seed (bit-reproducible): observations, rewards,
    dones, action noise, the last observation and the saved hidden states ([T, L, N, H] per state and network; only
    the rows at trajectory starts are ever read)."""
    rng = np.random.default_rng(seed)
    out = {
        "obs": rng.standard_normal((T, N, O), dtype=np.float32),
        "rewards": rng.standard_normal((T, N, 1), dtype=np.float32),
        "dones": (rng.random((T, N, 1)) < p_done).astype(np.uint8),
        "noise": rng.standard_normal((T, N, A), dtype=np.float32),
        "last_obs": rng.standard_normal((N, O), dtype=np.float32),
    }
    for net in "ac":
        out["hid_" + net] = [(0.3 * rng.standard_normal((T, L, N, H), dtype=np.float32)).astype(np.float32)
                             for _ in range(n_states)]
    return out


def inputs_digest(nz):
    h = hashlib.sha256()
    for k in ("obs", "rewards", "dones", "noise", "last_obs"):
        h.update(nz[k].tobytes())
    for net in "ac":
        for a in nz["hid_" + net]:
            h.update(a.tobytes())
    return h.hexdigest()


def load_meta():
    with open(os.path.join(GOLDEN, "golden_recurrent.json")) as f:
        return json.load(f)


class Arrays:
    """The arrays of several .npz files behind one `files` / `[key]` interface (what update_fixtures.check_update
    reads); row blocks "<key>@<i>" are joined back."""

    def __init__(self, names):
        self._z = [np.load(os.path.join(GOLDEN, n)) for n in names]
        self._where, parts = {}, {}
        for z in self._z:
            for k in z.files:
                if "@" in k:
                    base, i = k.rsplit("@", 1)
                    parts.setdefault(base, {})[int(i)] = z
                else:
                    self._where[k] = z
        self._parts = parts
        self.files = list(self._where) + list(parts)

    def __getitem__(self, k):
        if k in self._parts:
            p = self._parts[k]
            return np.concatenate([p[i][f"{k}@{i}"] for i in range(len(p))], axis=0)
        return self._where[k][k]


def save_split(arrays, stem):
    """Write arrays to <stem>_<i>.npz files, each below 1 MiB; returns the file names."""
    items = []
    for k, v in arrays.items():
        v = np.ascontiguousarray(v)
        if v.nbytes > PART_BYTES and v.ndim >= 1:
            rows = max(1, int(PART_BYTES // (v.nbytes // v.shape[0])))
            for i, r in enumerate(range(0, v.shape[0], rows)):
                items.append((f"{k}@{i}", v[r:r + rows]))
        else:
            items.append((k, v))
    files, cur, size = [], {}, 0
    for k, v in items:
        if cur and size + v.nbytes > PART_BYTES:
            files.append(cur)
            cur, size = {}, 0
        cur[k] = v
        size += v.nbytes + 256
    if cur:
        files.append(cur)
    names = []
    for i, f in enumerate(files):
        name = f"{os.path.basename(stem)}_{i:02d}.npz"
        path = os.path.join(GOLDEN, name)
        np.savez_compressed(path, **f)
        assert os.path.getsize(path) < (1 << 20), (name, os.path.getsize(path))
        names.append(name)
    return names


def policy_kwargs(meta):
    return dict(actor_hidden_dims=meta["hidden"], critic_hidden_dims=meta["hidden"], rnn_type=meta["rnn_type"],
                rnn_hidden_dim=meta["H"], rnn_num_layers=meta["L"], **meta.get("policy_kw", {}))


def fill_storage(st, nz, stored, device="cpu"):
    """The fixture's storage: seeded inputs, the stored policy-dependent fields, actions = mu + sigma * noise with
    the fixture's fp32 mul-then-add (CPU, IEEE)."""
    T, N, A = nz["noise"].shape
    mu = torch.from_numpy(stored["mu"].astype(np.float32))
    sigma = torch.from_numpy(stored["sigma"]).reshape(1, 1, A).expand(T, N, A)
    actions = mu + sigma * torch.from_numpy(nz["noise"])
    st.observations["policy"].copy_(torch.from_numpy(nz["obs"]))
    st.rewards.copy_(torch.from_numpy(nz["rewards"]))
    st.dones.copy_(torch.from_numpy(nz["dones"]))
    st.mu.copy_(mu)
    st.sigma.copy_(sigma)
    st.actions.copy_(actions)
    st.values.copy_(torch.from_numpy(stored["values"]))
    st.actions_log_prob.copy_(torch.from_numpy(stored["actions_log_prob"]))
    st.saved_hidden_states_a = [torch.from_numpy(a).to(device) for a in nz["hid_a"]]
    st.saved_hidden_states_c = [torch.from_numpy(a).to(device) for a in nz["hid_c"]]
    st.step = T


def build_update(z, meta, device, compute_returns=True):
    """(PPO, policy) of a rec_* case ready for update(): initial parameters, storage, compute_returns done (its
    evaluate advances the critic's memory from no state, as in the reference)."""
    from rsl_rl_amd.algorithms import PPO
    from rsl_rl_amd.modules import ActorCriticRecurrent

    T, N, O, A = meta["T"], meta["N"], meta["O"], meta["A"]
    rank = meta["ranks"][0]
    nz = storage_inputs(rank["noise_seed"], T, N, O, A, meta["L"], meta["H"], meta["n_states"])
    assert inputs_digest(nz) == rank["inputs_sha256"], "numpy stream differs"
    obs0 = {"policy": torch.zeros(N, O)}
    groups = {"policy": ["policy"], "critic": ["policy"]}
    pol = ActorCriticRecurrent(obs0, groups, A, **policy_kwargs(meta))
    pol.load_state_dict({k[len("r0/init/"):]: torch.from_numpy(z[k]) for k in z.files if k.startswith("r0/init/")})
    alg = PPO(pol, num_learning_epochs=meta["E"], num_mini_batches=meta["M"], device=device, learning_rate=1e-3)
    alg.init_storage("rl", N, T, obs0, [A])
    fill_storage(alg.storage, nz, {k: z["r0/storage/" + k] for k in ("mu", "sigma", "values", "actions_log_prob")},
                 device)
    if compute_returns:  # (the GAE kernel: a ROCm device)
        with torch.inference_mode():
            alg.compute_returns({"policy": torch.from_numpy(nz["last_obs"]).to(device)})
    return alg, pol


def torch_baseline_update(alg, pol):
    """The same update() in plain torch ops on the policy's device -- nn.LSTM / nn.GRU and F.linear under autograd,
    boolean-mask unpadding, the PPO loss written out in torch (ppo.py:259-315), clip_grad_norm_, torch's Adam, the
    host lr rule -- on the storage `alg` holds.  It measures how far PyTorch's own GPU arithmetic (the RNN library
    above all) lands from the CPU reference on a fixture: the yardstick for the recurrent parameters' bound.
    Returns (loss_dict, lr_trace)."""
    import torch.nn.functional as F
    from rsl_rl_amd.algorithms.ppo import adapt_learning_rate

    def mlp(net, x):
        for layer in net:
            x = F.linear(x, layer.weight, layer.bias) if isinstance(layer, torch.nn.Linear) else layer(x)
        return x

    opt = torch.optim.Adam(pol.parameters(), lr=alg.learning_rate)
    lr, lr_trace = alg.learning_rate, []
    sums = {"value_function": 0.0, "surrogate": 0.0, "entropy": 0.0}
    gen = alg.storage.recurrent_mini_batch_generator(alg.num_mini_batches, alg.num_learning_epochs)
    for obs, actions, tv, adv, ret, old_lp, old_mu, old_sigma, (hid_a, hid_c), masks in gen:
        masks = masks.clone()  # a plain bool mask: torch's boolean indexing
        x = pol.actor_obs_normalizer(pol.get_actor_obs(obs))
        mean = mlp(pol.actor, pol.memory_a(x, masks, hid_a))
        std = (pol.std if pol.noise_std_type == "scalar" else torch.exp(pol.log_std)).expand_as(mean)
        dist = torch.distributions.Normal(mean, std)
        logp = dist.log_prob(actions).sum(-1)
        entropy = dist.entropy().sum(-1)
        xc = pol.critic_obs_normalizer(pol.get_critic_obs(obs))
        value = mlp(pol.critic, pol.memory_c(xc, masks, hid_c))
        with torch.no_grad():
            kl = torch.sum(torch.log(std / old_sigma + 1.0e-5)
                           + (old_sigma.square() + (old_mu - mean).square()) / (2.0 * std.square()) - 0.5, -1).mean()
            lr = adapt_learning_rate(lr, kl.item(), alg.desired_kl)
            for g in opt.param_groups:
                g["lr"] = lr
        ratio = torch.exp(logp - old_lp.squeeze(-1))
        a = adv.squeeze(-1)
        surrogate = torch.max(-a * ratio, -a * ratio.clamp(1.0 - alg.clip_param, 1.0 + alg.clip_param)).mean()
        clipped = tv + (value - tv).clamp(-alg.clip_param, alg.clip_param)
        value_loss = torch.max((value - ret).square(), (clipped - ret).square()).mean()
        loss = surrogate + alg.value_loss_coef * value_loss - alg.entropy_coef * entropy.mean()
        opt.zero_grad()
        loss.backward()
        torch.nn.utils.clip_grad_norm_(pol.parameters(), alg.max_grad_norm)
        lr_trace.append(lr)
        opt.step()
        sums["value_function"] += value_loss.item()
        sums["surrogate"] += surrogate.item()
        sums["entropy"] += entropy.mean().item()
    n = alg.num_mini_batches * alg.num_learning_epochs
    return {k: v / n for k, v in sums.items()}, lr_trace


def check_recurrent_update(out, z, meta, baseline=None, mode=""):
    """The rules of update_fixtures.check_update for a rec_* case: lr trace and final lr exact, loss means rtol 1e-4,
    the first mini-batch's gradient within 1e-5 of its max, parameters within atol 2e-5 (narrow cases) or within
    2 * ulp_sensitivity + 1e-4 of the distance moved (rec_c).

    baseline: {name: (max abs error, ...)} of torch_baseline_update on the same device against the same fixture.
    Where PyTorch's own GPU autograd of nn.LSTM / nn.GRU already lands further from the CPU reference than 2e-5, a
    parameter may differ by 2x that measured distance instead (measured on an MI355X for rec_b's actor.2.weight:
    torch 2.83e-5, this code 3.53e-5; every other narrow parameter is below 2e-5 on both).  Prints both errors."""
    from update_fixtures import param_errors

    ref = meta["ranks"][0]
    assert out["lr_trace"] == ref["lr_trace"], (mode, out["lr_trace"], ref["lr_trace"])
    assert out["lr"] == ref["final_lr"], (mode, out["lr"], ref["final_lr"])
    assert set(out["loss"]) == set(ref["loss_dict"])
    for k, v in ref["loss_dict"].items():
        assert abs(out["loss"][k] - v) <= 1e-4 * abs(v) + 1e-6, (mode, k, out["loss"][k], v)
    r = torch.from_numpy(z["r0/grad_mb0"]).double()
    err = (out["grad_mb0"].double() - r).abs().max().item() / r.abs().max().item()
    print(mode, "first mini-batch gradient error / max:", f"{err:.2e}")
    assert err <= 1e-5, (mode, "grad_mb0", err)
    errs = param_errors(out["final"], z, "r0/")
    wide = max(meta["hidden"]) >= 256
    sens = meta.get("ulp_sensitivity", {})
    for name, (abs_err, rel_moved) in errs.items():
        base = baseline[name][0] if baseline is not None else 0.0
        print(f"{mode} {name:32s} ours {abs_err:.2e} / {rel_moved:.2e} of moved; torch on this device {base:.2e}")
    for name, (abs_err, rel_moved) in errs.items():
        if wide:
            assert rel_moved <= 2 * sens[name] + 1e-4, (mode, name, rel_moved, sens[name])
        else:
            base = baseline[name][0] if baseline is not None else 0.0
            # the measured yardstick itself is bounded: a broken or noisy baseline must not widen anything
            assert base <= 5e-5, (mode, name, "torch baseline", base)
            assert abs_err <= max(2e-5, 2 * base), (mode, name, abs_err, base)
    return errs
