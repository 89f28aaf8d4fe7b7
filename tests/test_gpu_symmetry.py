"""The two symmetry kernels on the GPU.

rslrl_ppo_loss_sym_fwd_bwd against an fp64 CPU torch-autograd transcription of the reference's update lines
(tests/loss_regimes.py: ppo.py:213-257 augmentation, :259-269 KL, :297-315 losses, :317-348 mirror loss), with the
tolerances tests/test_gpu_loss.py uses for the same quantities: gradients within 1e-5 of each tensor's max (a row whose
ratio or value difference sits within an fp32 ulp of a clip bound may take the other branch than the fp64 oracle: at
most max(1, 1e-5 rows) such rows, as test_random_vs_oracle allows), scalars rtol 1e-5 + 1e-6, the KL rtol 1e-5 + 1e-7.

rslrl_symmetry_augment (through SignedPermutationSymmetry) bit-equal to the class's torch path."""

import numpy as np
import pytest
import torch

from loss_regimes import apply_maps, oracle  # the one fp64 transcription of the reference's update lines
from rsl_rl_amd import kernels
from rsl_rl_amd.modules import SignedPermutationSymmetry
from rsl_rl_amd.utils.tensordict import TensorDict

pytestmark = pytest.mark.gpu

RTOL = 1e-5
CLIP, CV, CE = 0.2, 1.0, 0.01


def signed_maps(rng, width, K):
    """K (perm, sign) pairs over `width` columns, the identity first."""
    maps = [(np.arange(width), np.ones(width, np.float32))]
    for _ in range(K - 1):
        maps.append((rng.permutation(width), rng.choice(np.array([-1.0, 1.0], np.float32), width)))
    return maps


# ------------------------------------------------------------------------------------------------ loss kernel
def make_inputs(B, k_ppo, k_mir, A, shared, seed):
    rng = np.random.default_rng(seed)
    rows, n = k_mir * B, k_ppo * B
    d = {"mu": rng.standard_normal((rows, A), dtype=np.float32),
         "sigma": (rng.uniform(0.5, 1.5, A) if shared else rng.uniform(0.5, 1.5, (rows, A))).astype(np.float32),
         "x": rng.standard_normal((n, A), dtype=np.float32),
         "omu": rng.standard_normal((B, A), dtype=np.float32),
         "osig": rng.uniform(0.5, 1.5, (B, A)).astype(np.float32),
         "adv": rng.standard_normal((B, 1), dtype=np.float32),
         "tv": rng.standard_normal((B, 1), dtype=np.float32),
         "R": rng.standard_normal((B, 1), dtype=np.float32)}
    d["maps"] = signed_maps(rng, A, k_mir)
    # augmented blocks: the mean near the augmented base mean (a policy that is roughly symmetric), a per-row sigma
    # that of the base row, and actions at the base row's deviation from the mean (+ noise), so that every block's
    # log-prob stays near the stored one, as the augmented actions of a symmetric policy do
    for k in range(1, k_mir):
        perm, sign = d["maps"][k]
        blk = slice(k * B, (k + 1) * B)
        d["mu"][blk] = d["mu"][:B][:, perm] * sign + 0.3 * rng.standard_normal((B, A), dtype=np.float32)
        if not shared:
            d["sigma"][blk] = d["sigma"][:B]
        if k < k_ppo:
            d["x"][blk] = d["mu"][blk] + (d["x"][:B] - d["mu"][:B]) + 0.05 * rng.standard_normal((B, A), dtype=np.float32)
    # stored log-prob: that of the ORIGINAL block's actions + N(0, 0.3^2) (ratios on both sides of the clip);
    # values: target + N(0, 0.3^2) (differences on both sides of the value clip)
    sig = np.broadcast_to(d["sigma"], (rows, A))
    logp = (-(d["x"][:B] - d["mu"][:B]) ** 2 / (2 * sig[:B] ** 2) - np.log(sig[:B]) - 0.9189385).sum(-1)
    d["old_logp"] = (logp + 0.3 * rng.standard_normal(B)).astype(np.float32).reshape(B, 1)
    d["V"] = (np.tile(d["tv"], (k_ppo, 1)) + 0.3 * rng.standard_normal((n, 1))).astype(np.float32)
    return {k: (torch.from_numpy(v) if isinstance(v, np.ndarray) else v) for k, v in d.items()}


def run_kernel(d, dev, B, k_ppo, k_mir, coeff, clipped, norm_adv, form, symmetry_sum=None):
    g = lambda k: d[k].to(dev)  # noqa: E731
    kw = {}
    if k_mir > 1 and form == "tables":
        kw = dict(act_perm=torch.from_numpy(np.stack([p for p, _ in d["maps"]])).to(torch.int32).to(dev),
                  act_sign=torch.from_numpy(np.stack([s for _, s in d["maps"]])).to(dev))
    elif k_mir > 1:
        kw = dict(mirror_target=apply_maps(g("mu")[:B], d["maps"]).contiguous())  # fp32: sign * mu[perm], exact
    out = kernels.ppo_loss_sym_fwd_bwd(
        g("mu"), g("sigma"), g("V"), g("x"), g("old_logp"), g("adv"), g("tv"), g("R"), g("omu"), g("osig"), B=B,
        k_ppo=k_ppo, k_mir=k_mir, mirror_coeff=coeff, symmetry_sum=symmetry_sum, clip_param=CLIP, value_loss_coef=CV,
        entropy_coef=CE, use_clipped_value_loss=clipped, compute_kl=True, normalize_advantage=norm_adv, **kw)
    torch.cuda.synchronize()
    return [t.cpu() for t in out]


def rel_err(a, ref):
    a, ref = a.double().reshape(-1), ref.double().reshape(-1)
    return float((a - ref).abs().max() / (ref.abs().max() + 1e-30))


def close_but_rare_flips(a, ref, rows, what):
    a, ref = a.double().reshape(rows, -1), ref.double().reshape(rows, -1)
    bad = ((a - ref).abs() > RTOL * (ref.abs().max() + 1e-30)).any(dim=1)
    print(what, "max err / max", rel_err(a, ref), "rows off", int(bad.sum()))
    assert int(bad.sum()) <= max(1, int(1e-5 * rows)), (what, int(bad.sum()))


SHAPES = [  # B, k_ppo, k_mir, A, shared sigma
    (111, 2, 2, 12, True),
    (111, 1, 2, 12, True),
    (300, 4, 4, 3, True),   # scalar loads, rows across several blocks
    (64, 2, 2, 4, False),
    (1, 2, 2, 4, True),
    (111, 1, 1, 12, True),  # no mirror term
]


# every shape with and without the clipped value loss and per-mini-batch advantage normalisation -- but for the
# normalisation at B = 1, where the reference's std of one advantage is NaN
LOSS_CASES = [s + (clipped, norm) for s in SHAPES for clipped in (True, False) for norm in (False, True)
              if not (norm and s[0] == 1)]


@pytest.mark.parametrize("B,k_ppo,k_mir,A,shared,clipped,norm_adv", LOSS_CASES)
def test_loss_vs_fp64_autograd(B, k_ppo, k_mir, A, shared, clipped, norm_adv, cuda_device):
    coeff = 0.5
    d = make_inputs(B, k_ppo, k_mir, A, shared, seed=1000 * B + 10 * A + k_ppo + k_mir)
    ref = oracle(d, B, k_ppo, k_mir, coeff, clipped, norm_adv)
    if k_ppo * B >= 64:  # (two rows cannot populate four branches)
        assert 0.1 <= ref["outside_ratio"] <= 0.9, ref["outside_ratio"]
        assert 0.1 <= ref["outside_value"] <= 0.9, ref["outside_value"]
    rows = k_mir * B
    results = {}
    for form in (("tables", "pointer") if k_mir > 1 else ("none",)):
        stats, gmu, gsig, gv = run_kernel(d, cuda_device, B, k_ppo, k_mir, coeff, clipped, norm_adv, form)
        results[form] = (stats, gmu, gsig, gv)
        close_but_rare_flips(gmu, ref["dmu"], rows, "d mu")
        close_but_rare_flips(gv, ref["dV"], k_ppo * B, "d V")
        if shared:
            assert rel_err(gsig, ref["dsigma"]) < RTOL
        else:
            close_but_rare_flips(gsig, ref["dsigma"], rows, "d sigma")
        s = stats.double()
        for key, col in (("loss", kernels.STATS_LOSS), ("surrogate", kernels.STATS_SURROGATE),
                         ("value", kernels.STATS_VALUE), ("entropy", kernels.STATS_ENTROPY),
                         ("symmetry", kernels.STATS_SYMMETRY)):
            print(form, key, float(s[col]), ref[key])
            assert abs(float(s[col]) - ref[key]) <= RTOL * abs(ref[key]) + 1e-6, (form, key)
        assert abs(float(s[kernels.STATS_KL]) - ref["kl"]) <= RTOL * abs(ref["kl"]) + 1e-7
    if k_mir > 1:  # the kernel's own sign * mu[perm] and the caller's target tensor: the same bits
        for a, b in zip(results["tables"], results["pointer"]):
            assert torch.equal(a, b)


def test_loss_invariants(cuda_device):
    B, k, A = 111, 2, 12
    d = make_inputs(B, k, k, A, True, seed=5)
    zero = run_kernel(d, cuda_device, B, k, k, 0.0, True, False, "tables")
    half = run_kernel(d, cuda_device, B, k, k, 0.5, True, False, "tables")
    again = run_kernel(d, cuda_device, B, k, k, 0.5, True, False, "tables")
    # the target is detached: the original rows see no mirror gradient, whatever the coefficient
    assert torch.equal(zero[1][:B], half[1][:B])
    assert not torch.equal(zero[1][B:], half[1][B:])
    # the coefficient scales the gradient only; the statistic is reported either way
    assert zero[0][kernels.STATS_SYMMETRY] == half[0][kernels.STATS_SYMMETRY] > 0
    assert torch.equal(zero[3], half[3]) and torch.equal(zero[2], half[2])
    for a, b in zip(half, again):  # deterministic
        assert torch.equal(a, b)
    # the fp64 accumulator sums slot 7 over calls (one read-back per update)
    acc = torch.zeros(1, dtype=torch.float64, device=cuda_device)
    want = 0.0
    for seed, form in ((6, "tables"), (7, "pointer"), (8, "tables")):
        dd = make_inputs(B, k, k, A, True, seed=seed)
        stats = run_kernel(dd, cuda_device, B, k, k, 0.5, True, False, form, symmetry_sum=acc)[0]
        want += float(stats[kernels.STATS_SYMMETRY].double())
    assert acc.item() == want


def test_loss_wrapper_rejects_unsupported(cuda_device):
    d = make_inputs(4, 1, 1, 4, True, seed=1)
    with pytest.raises(ValueError, match="k_mir"):
        run_kernel(d, cuda_device, 4, 1, 9, 0.0, True, False, "none")


# ------------------------------------------------------------------------------------------------ augment kernel
class Counter:
    def __init__(self, monkeypatch):
        self.calls = 0
        orig = kernels.symmetry_augment

        def spy(*a, **k):
            self.calls += 1
            return orig(*a, **k)

        monkeypatch.setattr(kernels, "symmetry_augment", spy)


def check_equal(sym, obs_cpu, act_cpu, dev, strided=False):
    """The class on `dev` (the kernel) against the class on CPU tensors (its torch path)."""
    def to_dev(x):
        if not strided:
            return x.to(dev)
        wide = torch.full((x.shape[0], x.shape[1] + 20), 7.0, device=dev)  # a view of a wider record buffer
        wide[:, 8:8 + x.shape[1]] = x.to(dev)
        return wide[:, 8:8 + x.shape[1]]

    obs_dev = None if obs_cpu is None else TensorDict({k: to_dev(v) for k, v in obs_cpu.items()},
                                                      batch_size=obs_cpu.batch_size)
    act_dev = None if act_cpu is None else to_dev(act_cpu)
    want_o, want_a = sym(obs=obs_cpu, actions=act_cpu)
    got_o, got_a = sym(obs=obs_dev, actions=act_dev)
    torch.cuda.synchronize()
    if want_o is None:
        assert got_o is None
    else:
        assert list(got_o.batch_size) == list(want_o.batch_size)
        for k in want_o.keys():
            assert got_o[k].is_cuda and got_o[k].is_contiguous() and torch.equal(got_o[k].cpu(), want_o[k]), k
    if want_a is None:
        assert got_a is None
    else:
        assert got_a.is_cuda and torch.equal(got_a.cpu(), want_a)


@pytest.mark.parametrize("strided", [False, True])
@pytest.mark.parametrize("B", [1, 63, 1000])
@pytest.mark.parametrize("K", [2, 4])
@pytest.mark.parametrize("width", [48, 45, 3])
def test_augment_bit_equal_to_torch(width, K, B, strided, cuda_device, monkeypatch):
    rng = np.random.default_rng(width * 100 + K * 10 + B)
    A = 12
    sym = SignedPermutationSymmetry({"policy": signed_maps(rng, width, K), "critic": signed_maps(rng, 16, K)},
                                    signed_maps(rng, A, K))
    g = torch.Generator().manual_seed(B)
    obs = TensorDict({"policy": torch.randn(B, width, generator=g), "critic": torch.randn(B, 16, generator=g),
                      "plain": torch.randn(B, 5, generator=g)}, batch_size=[B])  # "plain": no map, repeated
    act = torch.randn(B, A, generator=g)
    count = Counter(monkeypatch)
    check_equal(sym, obs, act, cuda_device, strided)
    assert count.calls == 1, "every group and the actions must go through one launch"
    check_equal(sym, obs, None, cuda_device, strided)
    check_equal(sym, None, act, cuda_device, strided)
    assert count.calls == 3
    assert sym(obs=None, actions=None) == (None, None)


def test_augment_over_the_width_limit_falls_back(cuda_device, monkeypatch):
    rng = np.random.default_rng(3)
    width, K, B = 1028, 2, 3
    sym = SignedPermutationSymmetry({"policy": signed_maps(rng, width, K)}, signed_maps(rng, 4, K))
    obs = TensorDict({"policy": torch.randn(B, width)}, batch_size=[B])
    count = Counter(monkeypatch)
    check_equal(sym, obs, torch.randn(B, 4), cuda_device)
    assert count.calls == 0, "a group wider than the kernel's limit takes the torch path"
    # at the limit the kernel runs (its smallest tile: 8 rows per block)
    sym = SignedPermutationSymmetry({"policy": signed_maps(rng, 1024, K)}, signed_maps(rng, 4, K))
    check_equal(sym, TensorDict({"policy": torch.randn(19, 1024)}, batch_size=[19]), torch.randn(19, 4), cuda_device)
    assert count.calls == 1
