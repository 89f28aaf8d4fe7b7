"""The fixtures of tests/loss_regimes.py, and the numpy oracle's hand-written backward (oracle/ppo_oracle.py) against
torch autograd on them -- on the CPU.

Fixtures: every regime meets the branch-separation condition with no row excused, the float32 and float64 evaluations
take the same branches, every branch is populated, and the float32 yardstick's error is not zero.  Oracle: within the
GPU test's bar on the regimes (RMS error of a gradient tensor against float64 within 2x of torch fp32's, max within 3x;
statistics within the suite's bound), bit for bit on the exact table, the same NaN and signed-inf masks as torch fp32 on
the non-finite table."""

import numpy as np
import pytest
import torch

import loss_regimes as LR
from oracle import ppo_oracle as O

B = 333
SHAPES = [(A, shared) for A in (4, 7, 12, 16, 33) for shared in (True, False)]


def run_oracle(d, kw=None, **extra):
    """oracle.ppo_loss on a helper's inputs, in evaluate()'s key names; d sigma summed over rows for a shared sigma."""
    kw = dict(kw or {}, **extra)
    n = d["mu"].shape[0]
    A = d["mu"].shape[1]
    g = lambda k: d[k].numpy()  # noqa: E731
    shared = d["sigma"].dim() == 1
    sig = np.broadcast_to(g("sigma"), (n, A)).copy()
    with np.errstate(all="ignore"):
        o = O.ppo_loss(g("mu"), sig, g("V"), g("x"), g("old_logp"), g("adv"), g("tv"), g("R"), g("omu"), g("osig"),
                       clip_param=kw.get("clip", LR.CLIP), value_loss_coef=kw.get("cv", LR.CV),
                       entropy_coef=kw.get("ce", LR.CE), use_clipped_value_loss=kw.get("clipped", True),
                       normalize_advantage_per_mini_batch=kw.get("norm_adv", False))
        dsig = o["dsigma"].astype(np.float64).sum(0) if shared else o["dsigma"]
    return {"dmu": torch.from_numpy(o["dmu"]), "dsigma": torch.from_numpy(np.asarray(dsig)),
            "dV": torch.from_numpy(o["dV"]), "loss": o["loss"], "surrogate": o["surrogate"],
            "value": o["value_function"], "entropy": o["entropy"], "kl": o["kl_mean"]}


def eval_kw(kw):
    return {k: v for k, v in kw.items() if k in ("clipped", "norm_adv", "clip", "cv", "ce")}


# ------------------------------------------------------------------------------------------------ fixtures
@pytest.mark.parametrize("A,shared", SHAPES)
@pytest.mark.parametrize("name", sorted(LR.REGIMES))
def test_regime_fixture(name, A, shared):
    c = LR.regime_case(name, B, A, shared)
    masks, ref, yard = c.masks, c.ref, c.yard
    assert int(LR.unseparated_rows(ref).sum()) == 0  # zero excused rows
    m32 = LR.branch_masks(yard)
    for k, m in masks.items():
        assert torch.equal(m, m32[k]), (k, "fp32 and fp64 take different branches")
    out_ratio = float((masks["ratio_lo"] | masks["ratio_hi"]).double().mean())
    out_value = float(masks["value_out"].double().mean())
    assert 0.1 <= out_value <= 0.9, out_value
    inside = ~(masks["ratio_lo"] | masks["ratio_hi"])
    if name == "saturated":
        # delta ~ 3 N puts P(|3 N| > ~0.2) = 95 % of the ratios outside the clip range by the regime's definition, so
        # the 10 to 90 % share cannot hold; the three ratio branches are populated all the same (17 rows expected inside)
        assert out_ratio > 0.9 and int(inside.sum()) >= 8, (out_ratio, int(inside.sum()))
    else:
        assert 0.1 <= out_ratio <= 0.9, out_ratio
    assert int(masks["ratio_lo"].sum()) >= 8 and int(masks["ratio_hi"].sum()) >= 8
    assert masks["vl_gt"].any() and (masks["value_out"] & ~masks["vl_gt"]).any()
    rel = ((yard["ratio"].double() - ref["ratio"]).abs() / ref["ratio"]).max()
    assert float(rel) < LR.SEP / 4, float(rel)  # fp32's own ratio error: well inside the separation margin
    for k in ("dmu", "dsigma", "dV"):
        assert LR.errors(yard[k], ref[k])[1] > 0.0, k


def test_print_yardstick_statistics():
    """The float32 yardstick's own error on each statistic, relative to the float64 value: the table beside REGIMES."""
    for name in sorted(LR.REGIMES):
        worst, misses = dict.fromkeys(LR.STAT_KEYS, 0.0), dict.fromkeys(LR.STAT_KEYS, 0.0)
        for A, shared in SHAPES:
            c = LR.regime_case(name, B, A, shared)
            ref, yard = c.ref, c.yard
            for k in LR.STAT_KEYS:
                err = abs(yard[k] - ref[k])
                rel = err / (abs(ref[k]) + 1e-300)
                worst[k] = max(worst[k], rel)
                if err > LR.STAT_RTOL * abs(ref[k]) + LR.STAT_FLOOR[k]:
                    misses[k] = max(misses[k], rel)
        print(name, {k: "%.1e" % v for k, v in worst.items()}, "misses:", {k: "%.1e" % v for k, v in misses.items() if v})


# ------------------------------------------------------------------------------------------------ oracle
@pytest.mark.parametrize("A,shared", [(4, True), (12, True), (12, False), (33, True), (7, False)])
@pytest.mark.parametrize("name", sorted(LR.REGIMES))
def test_oracle_on_regimes(name, A, shared):
    c = LR.regime_case(name, B, A, shared)
    ref, yard = c.ref, c.yard
    got = run_oracle(c.d, c.kw)
    ok, _ = LR.within_bar(got, c, "%s A=%d shared=%d" % (name, A, shared))
    assert ok
    for k in LR.STAT_KEYS:
        assert abs(got[k] - ref[k]) <= LR.stat_bound(k, ref, yard, name), (k, got[k], ref[k], yard[k])


EXACT = [(A, clip, ce, clipped, per_row) for A in (2, 4) for clip in (0.25, 0.0) for ce in (2.0 ** -7, 0.0)
         for clipped in (True, False) for per_row in (False, True)]


@pytest.mark.parametrize("A,clip,ce,clipped,per_row", EXACT)
def test_exact_table(A, clip, ce, clipped, per_row):
    """The table's expected outputs are exact in fp32 (the float32 yardstick gives the float64 bits), it holds the ties
    it is built for, and the oracle reproduces it bit for bit."""
    d, kw = LR.exact_table(A, clip, ce, per_row)
    ref = LR.evaluate(d, torch.float64, clipped=clipped, **kw)
    yard = LR.evaluate(d, torch.float32, clipped=clipped, **kw)
    assert bool((ref["ratio"] == 1.0).all()) and bool((yard["ratio"] == 1.0).all())
    out = ref["dv"].abs() > clip
    assert bool((out & (ref["vl"] == ref["vlc"])).any()), "no tie that meets a blocking clamp"
    assert bool((out & (ref["vl"] > ref["vlc"])).any()) and bool((out & (ref["vl"] < ref["vlc"])).any())
    assert bool((ref["dv"].abs() == clip).any()), "no row on the value clip's bound"
    got = run_oracle(d, kw, clipped=clipped)
    for k in ("dmu", "dsigma", "dV"):
        want = ref[k].float()
        assert torch.equal(want.double(), ref[k]), (k, "the expected output is not exact in fp32")
        assert torch.equal(yard[k], want), (k, "torch fp32")
        assert torch.equal(got[k].float().reshape(want.shape), want), (k, "oracle")
    for k in ("surrogate", "value"):
        assert float(np.float32(ref[k])) == ref[k]
        assert float(np.float32(got[k])) == ref[k], k
    assert LR.ulps(got["entropy"], ref["entropy"]) <= A
    assert abs(got["loss"] - ref["loss"]) <= A * max(np.spacing(np.float32(abs(ref["loss"]))),
                                                       ce * np.spacing(np.float32(ref["entropy"])))


@pytest.mark.parametrize("shared", [True, False])
@pytest.mark.parametrize("name", LR.NONFINITE)
def test_oracle_nonfinite(name, shared):
    c = LR.nonfinite_case(name, 12, shared)
    yard = c.yard
    got = run_oracle(c.d, c.kw)
    ok, _ = LR.within_bar(got, c, name, where=c.finite)
    assert ok
    for k in ("dmu", "dsigma", "dV") + LR.STAT_KEYS:
        assert LR.same_nonfinite(got[k], yard[k]), (k, got[k], yard[k])
    assert not all(bool(torch.isfinite(torch.as_tensor(yard[k])).all()) for k in ("dmu", "dV", "loss")), \
        "the case does not reach a non-finite output"
