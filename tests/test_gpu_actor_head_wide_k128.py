"""The actor's fused head for 17 to 32 actions on a last hidden layer with 128 inputs (rslrl_actor_head_wide_fwd_bwd_k128;
csrc/mlp_heads_wide_k128.hip) against the launches it replaces on the same inputs -- linear_fwd_out_ex with H stored,
kernels.ppo_loss_fwd_bwd, the padded d mu copy, linear_dgrad_elu_ex and the weight gradient:

* mu, d mu: the same bits; the statistics and d sigma: equal (fp64 sums of the same fp32 terms, rounded once);
* a second launch: the same bits in every output; every output between NaN guard bands, the workspace's tail too;
* dz and the folded [dW | db]: both paths against fp64 torch on the CPU from the same fp32 inputs; the head's largest
  error may be at most twice the separate launches' own (tests/test_gpu_heads_k128.py's form: the largest absolute
  error over the whole result, so an entry at rounding level weighs what the result's largest entries weigh).

Rows: 64 is one tile, 192 three slices of one tile, 32,832 = 513 tiles the first shape with two tiles in a slice (and a
shorter last slice), 32,896 the first whose slices all hold two.  Actions: one live slot in the fifth lane (17), H1 flat's
19, whole lanes (24), the full octet (32)."""

import ctypes

import pytest
import torch
import torch.nn.functional as F

from rsl_rl_amd import _lib, kernels
from rsl_rl_amd.networks import fused_mlp
from test_gpu_heads_k128 import _case
from test_gpu_heads_narrow import (BAND, CLIP, ECOEF, VCOEF, _SENTINEL, _actor_head_args, _bands_untouched, _err, _fold,
                                   _guarded, _stream)

pytestmark = pytest.mark.gpu

SHAPES = [(A, N, M) for A in (17, 19, 24, 32) for N in (64, 128) for M in (64, 192, 32832)] + [(19, 128, 32896)]
# (A, N, M, clipped value loss, KL): every shape with both on; each setting off at one shape
CASES = [s + (True, True) for s in SHAPES] + [(19, 128, 192, False, True), (24, 64, 192, True, False)]


def _separate(c, clipped, kl):
    """Today's launches on the case's mu and H, and the fp64 references of dz and [dW | db] from the same d mu."""
    bt, A = c["batch"], c["wo"].shape[0]
    stats, gmu, gsig, _ = kernels.ppo_loss_fwd_bwd(
        c["mu"], c["sigma"], c["values"], bt["actions"], bt["old_log_prob"], bt["advantages"], bt["target_values"],
        bt["returns"], bt["old_mu"], bt["old_sigma"], clip_param=CLIP, value_loss_coef=VCOEF, entropy_coef=ECOEF,
        use_clipped_value_loss=clipped, compute_kl=kl)
    stats, gmu, gsig = stats.clone(), gmu.clone(), gsig.clone()
    dz = fused_mlp.linear_dgrad_elu_ex(F.pad(gmu, (0, (-A) % 4)), c["h"], c["img_t"], _lib.ARITH_X6, None, False,
                                       want_db=False)[0]
    dwb = torch.cat([fused_mlp._weight_grad(gmu, c["h"], True)[0].reshape(-1), gmu.sum(0)])
    g64, h64, wo64 = gmu.double().cpu(), c["h"].double().cpu(), c["wo"].double().cpu()
    dz64 = (g64 @ wo64) * torch.where(h64 > 0, torch.ones_like(h64), h64 + 1.0)
    dwb64 = torch.cat([(g64.t() @ h64).reshape(-1), g64.sum(0)])
    return stats, gmu, gsig, dz, dwb, dz64, dwb64


@pytest.mark.parametrize("A,N,M,clipped,kl", CASES)
def test_head_matches_separate_launches(A, N, M, clipped, kl, cuda_device):
    dev = cuda_device
    c = _case(N, M, A, dev)
    st_r, gmu_r, gs_r, dz_r, dwb_r, dz64, dwb64 = _separate(c, clipped, kl)
    L = _lib.lib()
    S = L.rslrl_head_k128_partial_rows(M)
    P = A * N + (A + 3) // 4 * 4
    bufs = {k: _guarded(n, dev) for k, n in (("dz", M * N), ("mu", M * A), ("gmu", M * A), ("wpart", S * P),
                                             ("gsig", A), ("stats", 8))}
    dz, mu, gmu, wpart, gsig, stats = (bufs[k][1] for k in ("dz", "mu", "gmu", "wpart", "gsig", "stats"))
    nbytes = L.rslrl_actor_head_wide_k128_workspace_bytes(M)
    ws = torch.zeros(nbytes // 4 + BAND, dtype=torch.int32, device=dev)
    ws[nbytes // 4:] = _SENTINEL
    args = fused_mlp._gemm_args(_lib.LINEAR_FWD_OUT, _lib.ARITH_X6, c["x"], None, N, c["img"], bias=c["b"],
                                c=dz.view(M, N), out_img=c["out_img"], out_bias=c["bo"], y=mu.view(M, A), nout=A)
    hargs = _actor_head_args(c, A, clipped, kl, c["img_t"], wpart, gsig, stats, gmu)
    results = []
    for _ in range(2):  # the launch re-arms its fold tickets: a second run gives the same bits
        rc = L.rslrl_actor_head_wide_fwd_bwd_k128(ctypes.byref(args), ctypes.byref(hargs), ws.data_ptr(), nbytes,
                                                  _stream(dev))
        assert rc == 0
        results.append([t.clone() for t in (dz, mu, gmu, wpart, gsig, stats)])
    torch.cuda.synchronize()
    for u, v in zip(*results):
        assert torch.equal(u, v)
    for k, (buf, mid) in bufs.items():
        assert _bands_untouched(buf), k
        assert bool(torch.isfinite(mid).all()), k
    assert bool((ws[nbytes // 4:] == _SENTINEL).all()) and bool((ws[:256] == 0).all())
    rows = wpart.view(S, P)
    assert bool((rows[:, A * N + A:] == 0).all())
    assert torch.equal(mu.view(M, A), c["mu"])
    assert torch.equal(gmu.view(M, A), gmu_r)
    assert torch.equal(stats, st_r), (stats, st_r)
    assert torch.equal(gsig, gs_r), (gsig, gs_r)
    for name, got, sep, ref in (("dz", dz.view(M, N).cpu(), dz_r.cpu(), dz64),
                                ("[dW | db]", _fold(rows, A * N + A, dev).cpu(), dwb_r.cpu(), dwb64)):
        e, e_r = _err(got, ref), _err(sep, ref)
        n = A * N
        tail = f", db alone {_err(got[n:], ref[n:]):.3e} / {_err(sep[n:], ref[n:]):.3e}" if name != "dz" else ""
        print(f"A={A} N={N} M={M} {name} max |err| vs fp64: head {e:.3e}, separate {e_r:.3e}, ratio {e / e_r:.3f}{tail}")
        assert e_r > 0.0 and e <= 2.0 * e_r, (name, e, e_r)


@pytest.mark.parametrize("N,M,knob", [(192, 128, True), (128, 96, True), (128, 128, False)])
def test_python_dispatch_declines(N, M, knob, cuda_device, monkeypatch):
    """K = 128 with N = 192, with M = 96, and with the knob off: None, nothing launched, nothing written."""
    dev, A = cuda_device, 19
    monkeypatch.setattr(fused_mlp, "_ACTOR_HEAD_WIDE_K128", knob)
    z = lambda *s: torch.zeros(*s, device=dev)  # noqa: E731
    head = fused_mlp.ActorHeadWide(z(M, A), z(M, 1), z(M, 1), z(M, 1), z(M, 1), z(M, A), z(M, A) + 1, z(A) + 1,
                                   clip_param=CLIP, value_loss_coef=VCOEF, entropy_coef=ECOEF, use_clipped=True,
                                   compute_kl=True, grad_sigma=z(A) - 7, stats=z(8) - 7)
    head.values = z(M, 1)
    w, wo = z(N, 128), z(A, N)
    img, out_img, img_t = fused_mlp.bimages([(w, False), (wo, False, _lib.BIMAGE_LAYOUT_OUT), (wo, True)])
    launches = fused_mlp.actor_head_wide_launches
    assert fused_mlp.actor_head_wide_fwd_bwd(z(M, 128), z(N), N, img, z(A), out_img, img_t, head) is None
    torch.cuda.synchronize()
    assert not head.done and fused_mlp.actor_head_wide_launches == launches
    assert bool((head.stats == -7).all()) and bool((head.grad_sigma == -7).all())


def test_python_dispatch_runs_the_head(cuda_device):
    """fused_mlp.actor_head_wide_fwd_bwd routes (N, K) = (128, 128) to the new entry: one partial row per slice, mu's bits."""
    dev, A, N, M = cuda_device, 19, 128, 384
    c = _case(N, M, A, dev)
    bt = c["batch"]
    head = fused_mlp.ActorHeadWide(bt["actions"], bt["old_log_prob"], bt["advantages"], bt["target_values"],
                                   bt["returns"], bt["old_mu"], bt["old_sigma"], c["sigma"], clip_param=CLIP,
                                   value_loss_coef=VCOEF, entropy_coef=ECOEF, use_clipped=True, compute_kl=True,
                                   grad_sigma=torch.empty(A, device=dev), stats=torch.empty(8, device=dev))
    head.values = c["values"]
    launches = fused_mlp.actor_head_wide_launches
    res = fused_mlp.actor_head_wide_fwd_bwd(c["x"], c["b"], N, c["img"], c["bo"], c["out_img"], c["img_t"], head)
    assert res is not None and head.done and fused_mlp.actor_head_wide_launches == launches + 1
    assert res[2].shape == (6, A * N + 20) and torch.equal(res[1], c["mu"])
