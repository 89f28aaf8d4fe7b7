"""The narrow heads (ABI 34: rslrl_value_head_fwd_bwd_n, rslrl_actor_head_fwd_bwd_n; a last hidden layer of 64, 128 or
192 columns) against the three launches they replace on the same inputs -- linear_fwd_out_ex, kernels.ppo_loss_fwd_bwd,
linear_dgrad_elu_wgrad:

* mu, the value and the actor's grad_mu output: the same bits;
* the statistics and d sigma: tests/test_gpu_actor_head_anya.py's comparisons for the 256-wide head;
* dz and the folded [dW | db]: the reduction orders differ, so both paths are measured against an fp64 torch reference
  and the head's max error may be at most 2x the three-launch path's (the partials cover other row groups; nothing more
  is known).  [dW | db] is the fold's one output vector and is held as a whole; its parts are printed.  (The critic's
  db alone is one scalar, the sum of M values of d loss / dV: the ratio of the two paths' single rounding errors, each
  within an ulp of db, says nothing, and on an MI355X it exceeds 2 at some shapes; the test prints both.)
* dz exactly wherever the three-launch dz is exactly 0 (a clipped row's d mu is 0) and wherever ELU' is 1 -- and
  everywhere else: the critic's dz is one fp32 product times ELU', the actor's narrow head forms dz with
  linear_dgrad_elu_wgrad's fp32 FMA chain, and both are held to that launch's bits on the whole tensor.  The per-tile [dW | db] partials are the 256-wide head's on the zero-padded
  problem, bit for bit.  A write into a neighbouring row's columns is an inequality, not a tolerance miss;
* dz, mu, d mu, the partials, d sigma and the workspace tail sit inside guard bands that come back untouched.

Shapes: one tile and three tiles (the cross-tile fold and the ticketed statistics); 5, 12 and 16 actions (each APL form
and the 12-action layout).  Stored fields come from a slightly perturbed policy: ratios on both sides of the clip."""

import ctypes
import functools

import pytest
import torch

from rsl_rl_amd import _lib, kernels
from rsl_rl_amd.networks import fused_mlp

pytestmark = pytest.mark.gpu

K = 256
WIDTHS = [64, 128, 192]
ROWS = [128, 384]
ACTIONS = [5, 12, 16]
CLIP, VCOEF, ECOEF = 0.2, 1.0, 0.01
BAND = 64
_SENTINEL = 0x7FC00123  # a NaN's bits: the workspace's tail band as int32


def _guarded(n, dev):
    """A NaN-filled buffer of BAND + n + BAND floats and the view of its middle."""
    buf = torch.full((n + 2 * BAND,), float("nan"), device=dev)
    return buf, buf[BAND:BAND + n]


def _bands_untouched(buf):
    return bool(torch.isnan(buf[:BAND]).all()) and bool(torch.isnan(buf[-BAND:]).all())


def _stream(dev):
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _elu_grad(h):
    return torch.where(h > 0, torch.ones_like(h), h + 1.0)


def _err(a, ref64):
    return float((a.double() - ref64).abs().max())


BOUNDED = ("dz", "[dW | db]")  # the two results held to 2x the three-launch path's max error


def _figures(dz, dz_r, dz64, dwb, dwb_r, dw64, db64):
    """{name: (the head's max |error| against fp64, the three-launch path's)} for dz and for the folded [dW | db]
    vector -- the fold's one output, held as a whole -- and, printed for the record only, for its two parts."""
    n = dw64.numel()
    dwb64 = torch.cat([dw64.reshape(-1), db64.reshape(-1)])
    return {"dz": (_err(dz, dz64), _err(dz_r, dz64)), "[dW | db]": (_err(dwb, dwb64), _err(dwb_r, dwb64)),
            "dW alone": (_err(dwb[:n], dwb64[:n]), _err(dwb_r[:n], dwb64[:n])),
            "db alone": (_err(dwb[n:], dwb64[n:]), _err(dwb_r[n:], dwb64[n:]))}


def _layer(N, nout, M, dev, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    r = lambda *s: torch.randn(*s, device=dev, generator=g)  # noqa: E731
    x = torch.nn.functional.elu(r(M, K))
    w, b = r(N, K) / 16, r(N) * 0.1
    wo, bo = r(nout, N) / 8, r(nout) * 0.1
    return g, x, w, b, wo, bo


def _fold(wpart, out_len, dev):
    folds = fused_mlp._FoldBatch()
    dwb = torch.empty(out_len, device=dev)
    folds.add(wpart, wpart.shape[0], wpart.shape[1], dwb, out_len)
    folds.run(dev)
    return dwb


# ---- the actor ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _actor_case(N, M, A, dev):
    """Inputs and the three-launch reference of one shape, computed once and shared by the flag variants that can
    (the loss depends on the flags: its part is computed per variant in _actor_reference)."""
    g, x, w, b, wo, bo = _layer(N, A, M, dev, 1000 * N + 10 * M + A)
    r = lambda *s: torch.randn(*s, device=dev, generator=g)  # noqa: E731
    img, out_img, img_t = fused_mlp.bimages([(w, False), (wo, False, _lib.BIMAGE_LAYOUT_OUT), (wo, True)])
    h, mu = fused_mlp.linear_fwd_out_ex(x, b, N, img, _lib.ARITH_X6, None, bo, out_img, store_h=True)
    sigma = torch.rand(A, device=dev, generator=g) * 0.5 + 0.5
    # the stored fields of a slightly older policy: its mean a little off, its std a little wider
    old_mu = mu + 0.06 * r(M, A)
    old_sigma = (sigma * 1.03).expand(M, A).contiguous()
    actions = old_mu + old_sigma * r(M, A)
    old_logp = torch.distributions.Normal(old_mu, old_sigma).log_prob(actions).sum(1, keepdim=True)
    tv = r(M, 1) * 0.3
    batch = dict(actions=actions.contiguous(), old_log_prob=old_logp.contiguous(), advantages=r(M, 1),
                 target_values=tv, returns=tv + 0.3 * r(M, 1), old_mu=old_mu.contiguous(), old_sigma=old_sigma)
    values = tv + 0.15 * r(M, 1)  # on both sides of the value clip
    ratio = torch.exp(torch.distributions.Normal(mu, sigma).log_prob(actions).sum(1) - old_logp[:, 0])
    assert bool((ratio > 1 + CLIP).any()) and bool((ratio < 1 - CLIP).any()) and bool(((ratio - 1).abs() < CLIP).any())
    return dict(x=x, w=w, b=b, wo=wo, bo=bo, img=img, out_img=out_img, img_t=img_t, h=h, mu=mu, sigma=sigma,
                values=values.contiguous(), batch=batch)


def _actor_reference(c, clipped, kl):
    bt = c["batch"]
    stats, gmu, gsig, _ = kernels.ppo_loss_fwd_bwd(
        c["mu"], c["sigma"], c["values"], bt["actions"], bt["old_log_prob"], bt["advantages"], bt["target_values"],
        bt["returns"], bt["old_mu"], bt["old_sigma"], clip_param=CLIP, value_loss_coef=VCOEF, entropy_coef=ECOEF,
        use_clipped_value_loss=clipped, compute_kl=kl)
    dz, _, dw, db = fused_mlp.linear_dgrad_elu_wgrad(gmu, c["wo"], c["h"], c["img_t"])
    return stats.clone(), gmu.clone(), gsig.clone(), dz, dw, db


def _actor_head_args(c, A, clipped, kl, img_t, wpart, gsig, stats, gmu):
    bt = c["batch"]
    return _lib.ActorHeadArgs(bt["actions"].data_ptr(), bt["old_log_prob"].data_ptr(), bt["advantages"].data_ptr(),
                              c["values"].data_ptr(), bt["target_values"].data_ptr(), bt["returns"].data_ptr(),
                              bt["old_mu"].data_ptr(), bt["old_sigma"].data_ptr(), c["sigma"].data_ptr(), A, CLIP, VCOEF,
                              ECOEF, int(clipped), int(kl), img_t.data_ptr(), wpart.data_ptr(), gsig.data_ptr(),
                              stats.data_ptr(), gmu.data_ptr())


def _actor_padded_256(c, N, M, A, clipped, kl, dev):
    """The 256-wide head's per-tile partial rows on the same problem zero-padded to 256 hidden columns."""
    z = lambda *s: torch.zeros(*s, device=dev)  # noqa: E731
    w = torch.cat([c["w"], z(256 - N, K)])
    b = torch.cat([c["b"], z(256 - N)])
    wo = torch.cat([c["wo"], z(A, 256 - N)], dim=1).contiguous()
    img, out_img, img_t = fused_mlp.bimages([(w, False), (wo, False, _lib.BIMAGE_LAYOUT_OUT), (wo, True)])
    bt = c["batch"]
    head = fused_mlp.ActorHead(bt["actions"], bt["old_log_prob"], bt["advantages"], bt["target_values"], bt["returns"],
                               bt["old_mu"], bt["old_sigma"], c["sigma"], clip_param=CLIP, value_loss_coef=VCOEF,
                               entropy_coef=ECOEF, use_clipped=clipped, compute_kl=kl,
                               grad_sigma=torch.empty(A, device=dev), stats=torch.empty(8, device=dev))
    head.values = c["values"]
    res = fused_mlp.actor_head_fwd_bwd(c["x"], b, 256, img, c["bo"], out_img, img_t, head)
    assert res is not None
    return res[2]


@pytest.mark.parametrize("clipped,kl", [(True, True), (False, False)])
@pytest.mark.parametrize("A", ACTIONS)
@pytest.mark.parametrize("M", ROWS)
@pytest.mark.parametrize("N", WIDTHS)
def test_actor_head_n_matches_three_launches(N, M, A, clipped, kl, cuda_device):
    dev = cuda_device
    c = _actor_case(N, M, A, dev)
    st_r, gmu_r, gs_r, dz_r, dw_r, db_r = _actor_reference(c, clipped, kl)
    L = _lib.lib()
    tiles = L.rslrl_linear_tiles(M)
    P = A * N + (A + 3) // 4 * 4
    bufs = {k: _guarded(n, dev) for k, n in (("dz", M * N), ("mu", M * A), ("gmu", M * A), ("wpart", tiles * P),
                                             ("gsig", A), ("stats", 8))}
    dz, mu, gmu, wpart, gsig, stats = (bufs[k][1] for k in ("dz", "mu", "gmu", "wpart", "gsig", "stats"))
    nbytes = L.rslrl_actor_head_workspace_bytes(M)
    assert nbytes % 4 == 0
    ws = torch.zeros(nbytes // 4 + BAND, dtype=torch.int32, device=dev)
    ws[nbytes // 4:] = _SENTINEL
    args = fused_mlp._gemm_args(_lib.LINEAR_FWD_OUT, _lib.ARITH_X6, c["x"], None, N, c["img"], bias=c["b"],
                                c=dz.view(M, N), out_img=c["out_img"], out_bias=c["bo"], y=mu.view(M, A), nout=A)
    hargs = _actor_head_args(c, A, clipped, kl, c["img_t"], wpart, gsig, stats, gmu)
    results = []
    for _ in range(2):  # the launch re-arms its fold tickets: a second run gives the same bits
        rc = L.rslrl_actor_head_fwd_bwd_n(ctypes.byref(args), ctypes.byref(hargs), ws.data_ptr(), nbytes, _stream(dev))
        assert rc == 0
        results.append([t.clone() for t in (dz, mu, gmu, wpart, gsig, stats)])
    wpart256 = _actor_padded_256(c, N, M, A, clipped, kl, dev)
    torch.cuda.synchronize()
    for u, v in zip(*results):
        assert torch.equal(u, v)
    # guard bands, the workspace tail, the re-armed tickets, the partial rows' padding
    for k, (buf, mid) in bufs.items():
        assert _bands_untouched(buf), k
        assert bool(torch.isfinite(mid).all()), k
    assert bool((ws[nbytes // 4:] == _SENTINEL).all())
    assert bool((ws[:256] == 0).all())  # the ticket block, zero between launches
    dz, mu, gmu = dz.view(M, N), mu.view(M, A), gmu.view(M, A)
    rows = wpart.view(tiles, P)
    assert bool((rows[:, A * N + A:] == 0).all())
    # the same bits as the three launches
    assert torch.equal(mu, c["mu"])
    assert torch.equal(gmu, gmu_r)
    # tests/test_gpu_actor_head_anya.py's comparisons of the statistics and d sigma
    assert torch.allclose(stats[:5], st_r[:5], rtol=2e-6, atol=1e-9), (stats, st_r)
    assert torch.equal(stats[5:], st_r[5:])
    assert torch.allclose(gsig, gs_r, rtol=1e-5, atol=1e-9)
    # dz and the folded [dW | db] against fp64, the bound from the three-launch path's own error
    dwb = _fold(rows, A * N + A, dev)
    h64, g64, wo64 = c["h"].double(), gmu_r.double(), c["wo"].double()
    dz64 = (g64 @ wo64) * _elu_grad(h64)
    dw64, db64 = g64.t() @ h64, g64.sum(0)
    figures = _figures(dz, dz_r, dz64, dwb, torch.cat([dw_r[:A].reshape(-1), db_r[:A]]), dw64, db64)
    print(f"actor N={N} M={M} A={A} clipped={clipped} kl={kl} max |err| vs fp64 (head, three launches): {figures}")
    for k in BOUNDED:
        assert figures[k][0] <= 2.0 * figures[k][1], (k, figures[k])
    # exact: the three-launch dz, everywhere -- so where it is exactly 0 (rows whose ratio is clipped have d mu = 0) and
    # where ELU' is 1, and the inputs hold both
    zero = dz_r == 0
    assert bool(zero.any()) and not bool(zero.all()) and bool((c["h"] > 0).any()) and bool((c["h"] <= 0).any())
    assert torch.equal(dz, dz_r)
    # exact: the 256-wide head's per-tile [dW | db] partials on the zero-padded problem (the partial rows' layout)
    assert torch.equal(rows[:, :A * N].view(tiles, A, N), wpart256[:, :A * 256].view(tiles, A, 256)[:, :, :N])
    assert torch.equal(rows[:, A * N:A * N + A], wpart256[:, A * 256:A * 256 + A])


def test_actor_head_n_python_dispatch(cuda_device, monkeypatch):
    """fused_mlp.actor_head_fwd_bwd routes 128 columns to the new entry (the same outputs as the direct call) and
    declines them under RSLRL_HEAD_NARROW=0 (the module flag)."""
    dev, N, M, A = cuda_device, 128, 384, 12
    c = _actor_case(N, M, A, dev)
    bt = c["batch"]

    def head():
        hd = fused_mlp.ActorHead(bt["actions"], bt["old_log_prob"], bt["advantages"], bt["target_values"],
                                 bt["returns"], bt["old_mu"], bt["old_sigma"], c["sigma"], clip_param=CLIP,
                                 value_loss_coef=VCOEF, entropy_coef=ECOEF, use_clipped=True, compute_kl=True,
                                 grad_sigma=torch.empty(A, device=dev), stats=torch.empty(8, device=dev))
        hd.values = c["values"]
        return hd

    launches = fused_mlp.actor_head_launches
    hd = head()
    res = fused_mlp.actor_head_fwd_bwd(c["x"], c["b"], N, c["img"], c["bo"], c["out_img"], c["img_t"], hd)
    assert res is not None and hd.done and fused_mlp.actor_head_launches == launches + 1
    dz, mu, wpart = res
    assert dz.shape == (M, N) and wpart.shape == (M // 128, A * N + A)
    assert torch.equal(mu, c["mu"])
    monkeypatch.setattr(fused_mlp, "_HEAD_NARROW", False)
    hd = head()
    assert fused_mlp.actor_head_fwd_bwd(c["x"], c["b"], N, c["img"], c["bo"], c["out_img"], c["img_t"], hd) is None
    assert not hd.done and fused_mlp.actor_head_launches == launches + 1


# ---- the critic ---------------------------------------------------------------------------------------------------
def _loss_dv(values, tv, ret, clipped, dev, g):
    """The loss kernel's d loss / dV for these values (random actor-side inputs: they do not enter d/dV)."""
    B, A = values.shape[0], 12
    z = lambda *s: torch.randn(*s, device=dev, generator=g)  # noqa: E731
    sigma = torch.rand(A, device=dev, generator=g) + 0.5
    _, _, _, g_value = kernels.ppo_loss_fwd_bwd(
        z(B, A), sigma, values, z(B, A), z(B, 1), z(B, 1), tv, ret, z(B, A), sigma.expand(B, A).contiguous(),
        clip_param=CLIP, value_loss_coef=VCOEF, use_clipped_value_loss=clipped)
    return g_value.reshape(B, 1).contiguous()


@pytest.mark.parametrize("with_colsum", [False, True])
@pytest.mark.parametrize("clipped", [True, False])
@pytest.mark.parametrize("M", ROWS)
@pytest.mark.parametrize("N", WIDTHS)
def test_value_head_n_matches_three_launches(N, M, clipped, with_colsum, cuda_device):
    dev = cuda_device
    g, x, w, b, wo, bo = _layer(N, 1, M, dev, 7 + 1000 * N + M)
    img, out_img, img_t = fused_mlp.bimages([(w, False), (wo, False, _lib.BIMAGE_LAYOUT_OUT), (wo, True)])
    h, y_r = fused_mlp.linear_fwd_out_ex(x, b, N, img, _lib.ARITH_X6, None, bo, out_img, store_h=True)
    tv = y_r + 0.15 * torch.randn(M, 1, device=dev, generator=g)  # V on both sides of the value clip around the target
    ret = tv + 0.3 * torch.randn(M, 1, device=dev, generator=g)
    dv = _loss_dv(y_r, tv, ret, clipped, dev, g)
    dz_r, _, dw_r, db_r = fused_mlp.linear_dgrad_elu_wgrad(dv, wo, h, img_t)
    L = _lib.lib()
    tiles = L.rslrl_linear_tiles(M)
    P = (N + 1 + 3) // 4 * 4
    bufs = {k: _guarded(n, dev) for k, n in (("dz", M * N), ("y", M), ("wpart", tiles * P), ("colsum", tiles * N))}
    dz, y, wpart, colsum = (bufs[k][1] for k in ("dz", "y", "wpart", "colsum"))
    args = fused_mlp._gemm_args(_lib.LINEAR_FWD_OUT, _lib.ARITH_X6, x, None, N, img, bias=b, c=dz.view(M, N),
                                out_img=out_img, out_bias=bo, y=y.view(M, 1), nout=1)
    vargs = _lib.ValueHeadArgs(tv.data_ptr(), ret.data_ptr(), wo.data_ptr(), CLIP, VCOEF, int(clipped), wpart.data_ptr(),
                               colsum.data_ptr() if with_colsum else None)
    assert L.rslrl_value_head_fwd_bwd_n(ctypes.byref(args), ctypes.byref(vargs), _stream(dev)) == 0
    torch.cuda.synchronize()
    for k, (buf, mid) in bufs.items():
        assert _bands_untouched(buf), k
        if k != "colsum" or with_colsum:
            assert bool(torch.isfinite(mid).all()), k
    if not with_colsum:
        assert bool(torch.isnan(colsum).all())
    dz, rows = dz.view(M, N), wpart.view(tiles, P)
    assert bool((rows[:, N + 1:] == 0).all())
    assert torch.equal(y.view(M, 1), y_r)
    dwb = _fold(rows, N + 1, dev)
    h64, dv64, wo64 = h.double(), dv.double(), wo.double()
    dz64 = (dv64 @ wo64) * _elu_grad(h64)
    dw64, db64 = dv64.t() @ h64, dv64.sum(0)
    figures = _figures(dz, dz_r, dz64, dwb, torch.cat([dw_r[:1].reshape(-1), db_r[:1]]), dw64, db64)
    print(f"critic N={N} M={M} clipped={clipped} max |err| vs fp64 (head, three launches): {figures}")
    for k in BOUNDED:
        assert figures[k][0] <= 2.0 * figures[k][1], (k, figures[k])
    # exact: the three-launch dz on the whole tensor (dz = dV w ELU'(H), the same expression), so wherever it is 0 and
    # wherever ELU' is 1 (one product, no other rounding); the inputs hold both sides of ELU
    assert bool((h > 0).any()) and bool((h <= 0).any())
    assert torch.equal(dz, dz_r)
    if with_colsum:  # per-tile column sums of dz (the last hidden layer's bias gradient), any summation order
        cs64 = dz.double().view(tiles, 128, N).sum(1)
        assert torch.allclose(colsum.view(tiles, N).double(), cs64, rtol=1e-5, atol=1e-6 * float(cs64.abs().max()))


def test_value_head_n_python_dispatch(cuda_device, monkeypatch):
    dev, N, M = cuda_device, 192, 384
    g, x, w, b, wo, bo = _layer(N, 1, M, dev, 99)
    img, out_img = fused_mlp.bimages([(w, False), (wo, False, _lib.BIMAGE_LAYOUT_OUT)])
    y_r = fused_mlp.linear_fwd_out_ex(x, b, N, img, _lib.ARITH_X6, None, bo, out_img, store_h=False)[1]
    head = fused_mlp.ValueHead(torch.zeros(M, 1, device=dev), torch.ones(M, 1, device=dev), CLIP, VCOEF, True)
    res = fused_mlp.value_head_fwd_bwd(x, b, N, img, bo, out_img, wo, head)
    assert res is not None
    dz, y, wpart = res
    assert dz.shape == (M, N) and wpart.shape == (M // 128, (N + 4) // 4 * 4)  # one row per tile, never per slice
    assert torch.equal(y, y_r)
    monkeypatch.setattr(fused_mlp, "_HEAD_NARROW", False)
    assert fused_mlp.value_head_fwd_bwd(x, b, N, img, bo, out_img, wo, head) is None
