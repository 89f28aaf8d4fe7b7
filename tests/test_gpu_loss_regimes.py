"""The PPO loss kernels against an independent reference at trained-policy regimes and on the branch points.

The loss arithmetic (csrc/ppo_loss_common.h) runs in five kernels that the suite ties to each other bit for bit; here it
meets torch autograd (tests/loss_regimes.py: float64 the reference, float32 the yardstick) where the random tests do not
go:
  regimes      sigma of a trained policy (0.03 to 0.1), 1e-3 and 5 to 20, ratios from e^-9 to e^9, values of 1e3, a KL
               whose terms cancel, advantages of 1e3 normalised per mini-batch.  d mu, d sigma, d V: rms error against
               float64 within 2x of torch fp32's, max within 3x; no row excused (the inputs keep every ratio and value
               difference 2^-10 clear of its clip bound); statistics within the suite's 1e-5.
  exact table  ties of torch.max, both ends of clamp's closed interval, a tie whose half share meets a blocking clamp,
               a zero advantage: torch.equal with float64 autograd.
  non-finite   one NaN / inf in one row: the NaN and signed-inf masks of every output are torch fp32's.
and the other three kernels through the comparisons they already have: ppo_loss_sym_fwd_bwd against the same
transcription, the two actor-head epilogues against the separate launches."""

import json
import os

import numpy as np
import pytest
import torch

import loss_regimes as LR
import test_gpu_actor_head as H12
import test_gpu_actor_head_anya as HA
import test_gpu_symmetry as SYM
from rsl_rl_amd import _lib, kernels
from rsl_rl_amd.networks import fused_mlp

pytestmark = pytest.mark.gpu

B = 333  # five 64-sample tiles and a ragged one; two blocks of the lane kernel
STAT_COL = {"loss": kernels.STATS_LOSS, "surrogate": kernels.STATS_SURROGATE, "value": kernels.STATS_VALUE,
            "entropy": kernels.STATS_ENTROPY, "kl": kernels.STATS_KL, "symmetry": kernels.STATS_SYMMETRY}
KERNEL_A = [(4, "lane"), (4, "quad"), (12, "lane"), (12, "quad"), (16, "lane"), (16, "quad"), (7, "lane"), (33, "lane")]
RESULTS = {}


@pytest.fixture(scope="module", autouse=True)
def _ratio_record():
    """RSLRL_LOSS_REGIMES_OUT=<file>: the measured error ratios of this run, as JSON (profiles/loss_regimes.json)."""
    yield
    path = os.environ.get("RSLRL_LOSS_REGIMES_OUT")
    if path:
        with open(path, "w") as f:
            json.dump(RESULTS, f, indent=1, sort_keys=True)


def run_loss(d, dev, *, kernel=None, clipped=True, norm_adv=False, clip=LR.CLIP, cv=LR.CV, ce=LR.CE, **_):
    """kernel: "quad" / "lane", the kernel RSLRL_LOSS_KERNEL asks for.  The dispatch falls back to the lane kernel when
    an operand misses the quad layout's conditions; only quad launches carry a launch-bound event pair, so the count of
    those tells which kernel ran."""
    g = lambda k: d[k].to(dev).contiguous()  # noqa: E731
    args = [g(k) for k in ("mu", "sigma", "V", "x", "old_logp", "adv", "tv", "R", "omu", "osig")]
    kernels.timer.arm_launch_events(4)
    try:
        stats, gmu, gsig, gv = kernels.ppo_loss_fwd_bwd(
            *args, clip_param=clip, value_loss_coef=cv, entropy_coef=ce, use_clipped_value_loss=clipped,
            compute_kl=True, normalize_advantage=norm_adv)
        torch.cuda.synchronize()
    finally:
        kernels.timer.disarm_launch_events()
    if kernel is not None:
        assert kernels.timer.launch_events()[1] == (1 if kernel == "quad" else 0), "another kernel than asked for ran"
    s = stats.cpu()
    out = {"dmu": gmu.cpu(), "dsigma": gsig.cpu(), "dV": gv.cpu(), "stats": s}
    out.update({k: float(s[c].double()) for k, c in STAT_COL.items()})
    return out


def check_stats(got, c, keys=LR.STAT_KEYS):
    for k in keys:
        bound = LR.stat_bound(k, c.ref, c.yard, c.name)
        print(k, got[k], c.ref[k], "err %.2e bound %.2e" % (abs(got[k] - c.ref[k]), bound))
        assert abs(got[k] - c.ref[k]) <= bound, (k, got[k], c.ref[k])


def record(what, ratios):
    RESULTS[what] = {k: {"rms_over_fp32": round(r, 3), "max_over_fp32": round(m, 3)} for k, (r, m) in ratios.items()}


# ------------------------------------------------------------------------------------------------ regimes
@pytest.mark.parametrize("shared", [True, False])
@pytest.mark.parametrize("A,kernel", KERNEL_A)
@pytest.mark.parametrize("name", sorted(LR.REGIMES))
def test_regime(name, A, kernel, shared, cuda_device, monkeypatch):
    monkeypatch.setenv("RSLRL_LOSS_KERNEL", kernel)
    c = LR.regime_case(name, B, A, shared)
    got = run_loss(c.d, cuda_device, kernel=kernel, **c.kw)
    what = "%s/%s/A%d/%s" % (name, kernel, A, "shared" if shared else "per_row")
    ok, ratios = LR.within_bar(got, c, what)
    record(what, ratios)
    assert ok, ratios
    check_stats(got, c)
    if name == "kl_near_zero":  # the per-action-constant KL and the reference's full expression: the same bits
        monkeypatch.setenv("RSLRL_KL_FAST", "0")
        full = run_loss(c.d, cuda_device, kernel=kernel, **c.kw)
        for k in ("dmu", "dsigma", "dV", "stats"):
            assert torch.equal(got[k], full[k]), k
        check_stats(full, c, ("kl",))


# ------------------------------------------------------------------------------------------------ exact table
EXACT = [(A, kernel, clip, ce, clipped, per_row) for A, kernel in ((4, "lane"), (4, "quad"), (2, "lane"))
         for clip in (0.25, 0.0) for ce in (2.0 ** -7, 0.0) for clipped in (True, False) for per_row in (False, True)]


def check_exact(got, ref, A, ce):
    for k in ("dmu", "dsigma", "dV"):
        want = ref[k].float()
        assert torch.equal(want.double(), ref[k]), (k, "the expected output is not exact in fp32")
        bad = (got[k].reshape(want.shape) != want).nonzero()
        assert torch.equal(got[k].reshape(want.shape), want), (k, bad[:4], got[k].reshape(want.shape)[tuple(bad[0])],
                                                               want[tuple(bad[0])])
    for k in ("surrogate", "value"):
        assert got[k] == ref[k], (k, got[k], ref[k])
    assert LR.ulps(got["entropy"], ref["entropy"]) <= A, (got["entropy"], ref["entropy"])
    tol = A * max(np.spacing(np.float32(abs(ref["loss"]))), ce * np.spacing(np.float32(ref["entropy"])))
    assert abs(got["loss"] - ref["loss"]) <= tol, (got["loss"], ref["loss"])


@pytest.mark.parametrize("A,kernel,clip,ce,clipped,per_row", EXACT)
def test_exact_table(A, kernel, clip, ce, clipped, per_row, cuda_device, monkeypatch):
    monkeypatch.setenv("RSLRL_LOSS_KERNEL", kernel)
    d, kw = LR.exact_table(A, clip, ce, per_row)
    ref = LR.evaluate(d, torch.float64, clipped=clipped, **kw)
    got = run_loss(d, cuda_device, kernel=kernel, clipped=clipped, **kw)
    check_exact(got, ref, A, ce)


# ------------------------------------------------------------------------------------------------ non-finite table
@pytest.mark.parametrize("shared", [True, False])
@pytest.mark.parametrize("kernel", ["lane", "quad"])
@pytest.mark.parametrize("name", LR.NONFINITE)
def test_nonfinite(name, kernel, shared, cuda_device, monkeypatch):
    monkeypatch.setenv("RSLRL_LOSS_KERNEL", kernel)
    c = LR.nonfinite_case(name, 12, shared)
    got = run_loss(c.d, cuda_device, kernel=kernel, **c.kw)
    wrong = [k for k in ("dmu", "dsigma", "dV") + LR.STAT_KEYS if not LR.same_nonfinite(got[k], c.yard[k])]
    for k in wrong:
        print(k, "kernel", got[k] if k in LR.STAT_KEYS else got[k].reshape(c.yard[k].shape)[~torch.isfinite(c.yard[k])],
              "torch fp32", c.yard[k] if k in LR.STAT_KEYS else c.yard[k][~torch.isfinite(c.yard[k])])
    assert not wrong, wrong
    ok, ratios = LR.within_bar(got, c, name, where=c.finite)
    assert ok, ratios
    check_stats(got, c, [k for k in LR.STAT_KEYS if np.isfinite(c.yard[k])])


# ------------------------------------------------------------------------------------------------ symmetric kernel
SYM_SHAPES = [(111, 2, 2, 12, True), (64, 2, 2, 4, False)]  # B, k_ppo, k_mir, A, shared sigma


@pytest.mark.parametrize("Bs,k_ppo,k_mir,A,shared", SYM_SHAPES)
@pytest.mark.parametrize("name", ["late", "tiny_sigma"])
def test_sym_regime(name, Bs, k_ppo, k_mir, A, shared, cuda_device):
    coeff = 0.5
    c = LR.regime_case(name, Bs, A, shared, k_ppo, k_mir)
    ref = LR.oracle(c.d, Bs, k_ppo, k_mir, coeff, True, False)
    kw = dict(c.kw, coeff=coeff)
    yard = LR.evaluate(c.d, torch.float32, **kw)
    case = type(c)(name=name, ref=ref, yard=yard, yard_err=LR.yardstick_errors(c.d, kw, ref, yard))
    d = dict(c.d, adv=c.d["adv"].reshape(-1, 1), tv=c.d["tv"].reshape(-1, 1), R=c.d["R"].reshape(-1, 1),
             old_logp=c.d["old_logp"].reshape(-1, 1), V=c.d["V"].reshape(-1, 1))
    for form in ("tables", "pointer"):
        stats, gmu, gsig, gv = SYM.run_kernel(d, cuda_device, Bs, k_ppo, k_mir, coeff, True, False, form)
        got = {"dmu": gmu, "dsigma": gsig, "dV": gv}
        got.update({k: float(stats[col].double()) for k, col in STAT_COL.items()})
        what = "sym/%s/%s/B%d_A%d" % (name, form, Bs, A)
        ok, ratios = LR.within_bar(got, case, what)
        record(what, ratios)
        assert ok, ratios
        check_stats(got, case, LR.STAT_KEYS + ("symmetry",))


@pytest.mark.parametrize("shared", [True, False])
@pytest.mark.parametrize("clip", [0.25, 0.0])
def test_sym_exact_table(clip, shared, cuda_device):
    """64 rows of the table as block 0 and again as block 1 under the identity map (the mirror term is exactly zero):
    128 rows, every expected output still exact."""
    Bs, A, ce = 64, 4, 2.0 ** -7
    t, kw = LR.exact_table(A, clip, ce, per_row_sigma=not shared)
    d = {k: v[:Bs] for k, v in t.items() if k != "sigma"}
    two = lambda v: torch.cat([v, v])  # noqa: E731
    d.update(mu=two(d["mu"]), x=two(d["x"]), V=two(d["V"]), sigma=t["sigma"] if shared else t["sigma"][:2 * Bs],
             maps=[(np.arange(A), np.ones(A, np.float32))] * 2)
    ref = LR.evaluate(d, torch.float64, B=Bs, k_ppo=2, k_mir=2, coeff=0.5, **kw)
    g = lambda k: d[k].to(cuda_device).contiguous()  # noqa: E731
    stats, gmu, gsig, gv = kernels.ppo_loss_sym_fwd_bwd(
        g("mu"), g("sigma"), g("V"), g("x"), g("old_logp"), g("adv"), g("tv"), g("R"), g("omu"), g("osig"), B=Bs,
        k_ppo=2, k_mir=2, mirror_coeff=0.5, mirror_target=g("mu"), clip_param=clip, value_loss_coef=1.0,
        entropy_coef=ce, use_clipped_value_loss=True, compute_kl=True)
    torch.cuda.synchronize()
    got = {"dmu": gmu.cpu(), "dsigma": gsig.cpu(), "dV": gv.cpu()}
    got.update({k: float(stats[col].double()) for k, col in STAT_COL.items()})
    check_exact(got, ref, A, ce)
    assert got["symmetry"] == 0.0


# ------------------------------------------------------------------------------------------------ actor head
def _head_problem(A, M, dev, name, nan_row=None):
    """The actor-head tests' problem with the loss inputs of a regime: mu from the separate forward launch, then
    sigma, actions and the stored log-prob built around that mu on the host."""
    mod = H12 if A == 12 else HA
    p = mod._problem(M, dev, 900 + M) if A == 12 else mod._problem(A, M, dev, 900 + M + A)
    x, w, b, wo, bo, _, values, batch = p
    imgs = HA._images(w, wo)
    if nan_row is not None:
        x[nan_row, 3] = float("nan")
    _, mu = fused_mlp.linear_fwd_out_ex(x, b, w.shape[0], imgs[0], _lib.ARITH_X6, None, bo, imgs[1], store_h=True)
    torch.cuda.synchronize()
    mu = mu.cpu().numpy()
    mu = np.where(np.isnan(mu), 0.0, mu).astype(np.float32)
    (s_lo, s_hi), delta_scale, _, _ = LR.REGIMES[name]
    rng = np.random.default_rng(M + A)
    f = np.float32
    sigma = rng.uniform(s_lo, s_hi, A).astype(f)
    act = (mu + sigma * rng.standard_normal((M, A))).astype(f)
    old_logp = (LR._logp64(mu, sigma, act) - delta_scale * rng.standard_normal(M)).astype(f).reshape(M, 1)
    old_sigma = np.broadcast_to((sigma * rng.uniform(0.9, 1.1, A)).astype(f), (M, A)).copy()
    old_mu = (mu + 0.1 * sigma * rng.standard_normal((M, A))).astype(f)
    t = lambda a: torch.from_numpy(a).to(dev)  # noqa: E731
    batch = dict(batch, actions=t(act), old_log_prob=t(old_logp), old_mu=t(old_mu), old_sigma=t(old_sigma))
    return mod, (x, w, b, wo, bo, t(sigma), values, batch), imgs


@pytest.mark.parametrize("name", ["late", "tiny_sigma"])
@pytest.mark.parametrize("M", [128, 384])
@pytest.mark.parametrize("A", [12, 7])
def test_actor_head_regime(A, M, name, cuda_device):
    mod, p, imgs = _head_problem(A, M, cuda_device, name)
    ref = mod._separate(*p, *imgs, True, True)
    got = mod._fused(*p, *imgs, True, True)
    torch.cuda.synchronize()
    HA._compare(got, ref)


@pytest.mark.parametrize("where", ["x", "actions"])
@pytest.mark.parametrize("A", [12, 7])
def test_actor_head_nan_row(A, where, cuda_device):
    """One NaN in a row of the layer's input, or of the actions (which reaches the loss epilogue: that row's gradient and
    the loss and surrogate statistics are NaN): the head and the separate launches put NaN in the same places and agree as
    before everywhere else."""
    row = 133
    mod, p, imgs = _head_problem(A, 384, cuda_device, "late", nan_row=row if where == "x" else None)
    if where == "actions":
        p[7]["actions"][row, A // 2] = float("nan")
    ref = mod._separate(*p, *imgs, True, True)
    got = mod._fused(*p, *imgs, True, True)
    torch.cuda.synchronize()
    if where == "actions":
        assert bool(torch.isnan(ref[2][row]).all()) and bool(torch.isnan(ref[1][:2]).all())  # the loss, the surrogate
        assert not bool(torch.isnan(ref[2][:row]).any()) and not bool(torch.isnan(ref[1][2:]).any())
    for u, v in zip(got, ref):
        assert torch.equal(torch.isnan(u), torch.isnan(v))
    HA._compare([torch.nan_to_num(u, nan=0.0) for u in got], [torch.nan_to_num(v, nan=0.0) for v in ref])
