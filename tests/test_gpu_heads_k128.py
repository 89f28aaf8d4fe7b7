"""The heads for a last hidden layer with 128 inputs (rslrl_value_head_fwd_bwd_k128, rslrl_actor_head_fwd_bwd_k128;
csrc/mlp_heads_k128.hip) against the launches they replace on the same inputs -- linear_fwd_out_ex,
kernels.ppo_loss_fwd_bwd, linear_dgrad_elu_wgrad:

* mu, V, d mu and dz: the same bits (the same expressions in the same order);
* the statistics and d sigma: tests/test_gpu_heads_narrow.py's comparisons;
* the folded [dW | db]: both paths against fp64 torch (d out^T H, d out.sum(0)); the head's largest error may be at most
  twice the separate launches' own (the project's bound for a changed summation order); the ratios are printed;
* a second launch on the same inputs: the same bits in every output, the statistics included;
* every output between NaN guard bands, the workspace's tail and its re-armed tickets.

Rows.  The slice rule is per = ceil(tiles / 512) 64-row tiles per workgroup, S = ceil(tiles / per) workgroups: 64 rows is
one tile, 192 three workgroups of one; per first becomes 2 at 513 tiles = 32,832 rows, which is also the smallest M
whose last slice is shorter than the others (256 slices of two tiles and one of one); 514 tiles = 32,896 rows is the
smallest M whose slices all hold two.  Actions 5, 12, 16: a masked tail, and 2, 3, 4 actions per quad lane."""

import ctypes
import functools

import pytest
import torch

from rsl_rl_amd import _lib
from rsl_rl_amd.networks import fused_mlp
from test_gpu_heads_narrow import (BAND, CLIP, ECOEF, VCOEF, _SENTINEL, _actor_head_args, _actor_reference,
                                   _bands_untouched, _err, _fold, _guarded, _loss_dv, _stream)

pytestmark = pytest.mark.gpu

K = 128
WIDTHS = [64, 128]
ROWS = [64, 192, 32832, 32896]
ACTIONS = [5, 12, 16]


@functools.lru_cache(maxsize=None)
def _case(N, M, A, dev):
    """Inputs and the forward reference of one shape (A = 1: the critic), computed once: H on both sides of ELU, and
    for the actor the stored fields of a slightly older policy (ratios on both sides of the surrogate clip, values on
    both sides of the value clip)."""
    g = torch.Generator(device=dev).manual_seed(1000 * N + M + A)
    r = lambda *s: torch.randn(*s, device=dev, generator=g)  # noqa: E731
    x = torch.nn.functional.elu(r(M, K))
    w, b, wo, bo = r(N, K) / 11, r(N) * 0.1, r(A, N) / 8, r(A) * 0.1
    img, out_img, img_t = fused_mlp.bimages([(w, False), (wo, False, _lib.BIMAGE_LAYOUT_OUT), (wo, True)])
    h, mu = fused_mlp.linear_fwd_out_ex(x, b, N, img, _lib.ARITH_X6, None, bo, out_img, store_h=True)
    assert bool((h > 0).any()) and bool((h <= 0).any())
    c = dict(g=g, x=x, b=b, wo=wo, bo=bo, img=img, out_img=out_img, img_t=img_t, h=h, mu=mu)
    if A == 1:
        return c
    sigma = torch.rand(A, device=dev, generator=g) * 0.5 + 0.5
    old_mu = mu + 0.06 * r(M, A)
    old_sigma = (sigma * 1.03).expand(M, A).contiguous()
    actions = old_mu + old_sigma * r(M, A)
    old_logp = torch.distributions.Normal(old_mu, old_sigma).log_prob(actions).sum(1, keepdim=True)
    tv = r(M, 1) * 0.3
    ratio = torch.exp(torch.distributions.Normal(mu, sigma).log_prob(actions).sum(1) - old_logp[:, 0])
    assert bool((ratio > 1 + CLIP).any()) and bool((ratio < 1 - CLIP).any()) and bool(((ratio - 1).abs() < CLIP).any())
    c.update(sigma=sigma, values=(tv + 0.15 * r(M, 1)).contiguous(),
             batch=dict(actions=actions.contiguous(), old_log_prob=old_logp.contiguous(), advantages=r(M, 1),
                        target_values=tv, returns=tv + 0.3 * r(M, 1), old_mu=old_mu.contiguous(), old_sigma=old_sigma))
    return c


def _dwb_within_bound(tag, dwb, dwb_r, dout, h):
    """The folded [dW | db] of both paths against fp64 (d out^T H, d out.sum(0)): the 2x bound, the ratio printed."""
    h64, g64 = h.double(), dout.double()
    dwb64 = torch.cat([(g64.t() @ h64).reshape(-1), g64.sum(0)])
    e, e_r = _err(dwb, dwb64), _err(dwb_r, dwb64)
    print(f"{tag} [dW | db] max |err| vs fp64: head {e:.3e}, separate {e_r:.3e}, ratio {e / e_r:.3f}")
    assert e <= 2.0 * e_r, (e, e_r)


@pytest.mark.parametrize("A", ACTIONS)
@pytest.mark.parametrize("M", ROWS)
@pytest.mark.parametrize("N", WIDTHS)
def test_actor_head_k128_matches_three_launches(N, M, A, cuda_device):
    dev = cuda_device
    c = _case(N, M, A, dev)
    clipped = kl = A != 12  # both value-loss forms and the KL on and off across the widths
    st_r, gmu_r, gs_r, dz_r, dw_r, db_r = _actor_reference(c, clipped, kl)
    L = _lib.lib()
    S = L.rslrl_head_k128_partial_rows(M)
    P = A * N + (A + 3) // 4 * 4
    bufs = {k: _guarded(n, dev) for k, n in (("dz", M * N), ("mu", M * A), ("gmu", M * A), ("wpart", S * P),
                                             ("gsig", A), ("stats", 8))}
    dz, mu, gmu, wpart, gsig, stats = (bufs[k][1] for k in ("dz", "mu", "gmu", "wpart", "gsig", "stats"))
    nbytes = L.rslrl_actor_head_k128_workspace_bytes(M)
    ws = torch.zeros(nbytes // 4 + BAND, dtype=torch.int32, device=dev)
    ws[nbytes // 4:] = _SENTINEL
    args = fused_mlp._gemm_args(_lib.LINEAR_FWD_OUT, _lib.ARITH_X6, c["x"], None, N, c["img"], bias=c["b"],
                                c=dz.view(M, N), out_img=c["out_img"], out_bias=c["bo"], y=mu.view(M, A), nout=A)
    hargs = _actor_head_args(c, A, clipped, kl, c["img_t"], wpart, gsig, stats, gmu)
    results = []
    for _ in range(2):  # the launch re-arms its fold tickets: a second run gives the same bits
        rc = L.rslrl_actor_head_fwd_bwd_k128(ctypes.byref(args), ctypes.byref(hargs), ws.data_ptr(), nbytes,
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
    assert bool((dz_r == 0).any()) and torch.equal(dz.view(M, N), dz_r)
    assert torch.allclose(stats[:5], st_r[:5], rtol=2e-6, atol=1e-9), (stats, st_r)
    assert torch.equal(stats[5:], st_r[5:])
    assert torch.allclose(gsig, gs_r, rtol=1e-5, atol=1e-9)
    _dwb_within_bound(f"actor N={N} M={M} A={A}", _fold(rows, A * N + A, dev),
                      torch.cat([dw_r[:A].reshape(-1), db_r[:A]]), gmu_r, c["h"])


@pytest.mark.parametrize("clipped", [True, False])
@pytest.mark.parametrize("M", ROWS)
@pytest.mark.parametrize("N", WIDTHS)
def test_value_head_k128_matches_three_launches(N, M, clipped, cuda_device):
    dev = cuda_device
    c = _case(N, M, 1, dev)
    g, y_r = c["g"], c["mu"]
    tv = y_r + 0.15 * torch.randn(M, 1, device=dev, generator=g)  # V on both sides of the value clip around the target
    ret = tv + 0.3 * torch.randn(M, 1, device=dev, generator=g)
    dv = _loss_dv(y_r, tv, ret, clipped, dev, g)
    dz_r, _, dw_r, db_r = fused_mlp.linear_dgrad_elu_wgrad(dv, c["wo"], c["h"], c["img_t"])
    L = _lib.lib()
    S = L.rslrl_head_k128_partial_rows(M)
    P = N + 4
    bufs = {k: _guarded(n, dev) for k, n in (("dz", M * N), ("y", M), ("wpart", S * P))}
    dz, y, wpart = (bufs[k][1] for k in ("dz", "y", "wpart"))
    args = fused_mlp._gemm_args(_lib.LINEAR_FWD_OUT, _lib.ARITH_X6, c["x"], None, N, c["img"], bias=c["b"],
                                c=dz.view(M, N), out_img=c["out_img"], out_bias=c["bo"], y=y.view(M, 1), nout=1)
    vargs = _lib.ValueHeadArgs(tv.data_ptr(), ret.data_ptr(), c["wo"].data_ptr(), CLIP, VCOEF, int(clipped),
                               wpart.data_ptr(), None)
    results = []
    for _ in range(2):
        assert L.rslrl_value_head_fwd_bwd_k128(ctypes.byref(args), ctypes.byref(vargs), _stream(dev)) == 0
        results.append([t.clone() for t in (dz, y, wpart)])
    torch.cuda.synchronize()
    for u, v in zip(*results):
        assert torch.equal(u, v)
    for k, (buf, mid) in bufs.items():
        assert _bands_untouched(buf), k
        assert bool(torch.isfinite(mid).all()), k
    rows = wpart.view(S, P)
    assert bool((rows[:, N + 1:] == 0).all())
    assert torch.equal(y.view(M, 1), y_r)
    assert torch.equal(dz.view(M, N), dz_r)
    _dwb_within_bound(f"critic N={N} M={M} clipped={clipped}", _fold(rows, N + 1, dev),
                      torch.cat([dw_r[:1].reshape(-1), db_r[:1]]), dv, c["h"])


def test_actor_head_k128_python_dispatch(cuda_device, monkeypatch):
    """fused_mlp.actor_head_fwd_bwd routes (N, K) = (128, 128) to the new entry (the direct call's outputs, one partial
    row per slice) and declines it, with nothing counted, under RSLRL_HEAD_K128=0 (the module flag)."""
    dev, N, M, A = cuda_device, 128, 192, 12
    c = _case(N, M, A, dev)
    bt = c["batch"]

    def head():
        hd = fused_mlp.ActorHead(bt["actions"], bt["old_log_prob"], bt["advantages"], bt["target_values"],
                                 bt["returns"], bt["old_mu"], bt["old_sigma"], c["sigma"], clip_param=CLIP,
                                 value_loss_coef=VCOEF, entropy_coef=ECOEF, use_clipped=True, compute_kl=True,
                                 grad_sigma=torch.empty(A, device=dev), stats=torch.empty(8, device=dev))
        hd.values = c["values"]
        return hd

    _, gmu_r, _, dz_r, _, _ = _actor_reference(c, True, True)
    launches = fused_mlp.actor_head_launches
    hd = head()
    res = fused_mlp.actor_head_fwd_bwd(c["x"], c["b"], N, c["img"], c["bo"], c["out_img"], c["img_t"], hd)
    assert res is not None and hd.done and fused_mlp.actor_head_launches == launches + 1
    dz, mu, wpart = res
    assert wpart.shape == (3, A * N + A) and torch.equal(mu, c["mu"]) and torch.equal(dz, dz_r)
    monkeypatch.setattr(fused_mlp, "_HEAD_K128", False)
    hd = head()
    assert fused_mlp.actor_head_fwd_bwd(c["x"], c["b"], N, c["img"], c["bo"], c["out_img"], c["img_t"], hd) is None
    assert not hd.done and fused_mlp.actor_head_launches == launches + 1


def test_value_head_k128_python_dispatch(cuda_device, monkeypatch):
    dev, N, M = cuda_device, 64, 192
    c = _case(N, M, 1, dev)
    head = fused_mlp.ValueHead(torch.zeros(M, 1, device=dev), torch.ones(M, 1, device=dev), CLIP, VCOEF, True)
    res = fused_mlp.value_head_fwd_bwd(c["x"], c["b"], N, c["img"], c["bo"], c["out_img"], c["wo"], head)
    assert res is not None
    dz, y, wpart = res
    assert dz.shape == (M, N) and wpart.shape == (3, N + 4) and torch.equal(y, c["mu"])
    assert fused_mlp.value_head_fwd_bwd(c["x"][:100], c["b"], N, c["img"], c["bo"], c["out_img"], c["wo"],
                                        fused_mlp.ValueHead(head.target_values[:100], head.returns[:100], CLIP, VCOEF,
                                                            True)) is None  # M no multiple of 64
    monkeypatch.setattr(fused_mlp, "_HEAD_K128", False)
    assert fused_mlp.value_head_fwd_bwd(c["x"], c["b"], N, c["img"], c["bo"], c["out_img"], c["wo"], head) is None
