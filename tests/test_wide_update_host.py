"""The wide-update fixture on the CPU: this package's own PPO.update() in plain torch fp32 -- no HIP
kernel runs here -- against the reference's, through the same build_update / run_recorded_update / check_update the GPU
test uses.  It shows that check_update's bounds (exact learning-rate trace, losses rtol 1e-4, first-mini-batch gradient
1e-5 of its max, parameters within twice the reference's own one-ulp sensitivity) are reachable at hidden
[320, 260, 64] by an implementation that differs from the reference only in the order of fp32 operations."""

import torch

import wide_fixtures as WF
from update_fixtures import check_update


def test_fixture_shape_and_margins():
    z, meta = WF.load()
    assert (meta["T"], meta["N"], meta["O"], meta["A"], meta["hidden"]) == (8, 256, 16, 4, [320, 260, 64])
    assert (meta["E"], meta["M"]) == (5, 4) and len(meta["kl_trace"]) == 20
    for kl in meta["kl_trace"]:  # no learning-rate decision hangs on a last bit
        for thr in (meta["desired_kl"] / 2, 2 * meta["desired_kl"]):
            assert abs(kl - thr) >= 0.10 * thr, (kl, thr)
    assert max(meta["hidden"]) >= 256 and set(meta["ulp_sensitivity"]) == {k[9:] for k in z.files if k.startswith("r0/final/")}
    assert z["r0/init/actor.2.weight"].shape == (260, 320) and z["r0/init/critic.4.weight"].shape == (64, 260)


def test_update_on_cpu_meets_the_bounds():
    z, meta = WF.load()
    out, alg = WF.run_update(z, meta, torch.device("cpu"))
    check_update(out, z, meta, 0, mode="cpu")
