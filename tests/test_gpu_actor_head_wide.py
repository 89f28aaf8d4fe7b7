"""The actor's fused head for 17 to 32 actions (rslrl_actor_head_wide_fwd_bwd) against the launches it replaces: mu
bit for bit linear_fwd_out_ex's, d mu bit for bit kernels.ppo_loss_fwd_bwd's (ppo_loss_kernel<32>'s tree_sum on an
octet of lanes), the statistics and d sigma at tests/test_gpu_actor_head_anya.py's tolerances, and dZ and the folded
[dW | db] against fp64 within twice the separate launches' own error (a re-ordered fp32 sum).  Then guard bands, the
declined shapes, and PPO.update() with the head against RSLRL_ACTOR_HEAD_WIDE=0."""

import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from rsl_rl_amd import _lib, kernels
from rsl_rl_amd.networks import fused_mlp

pytestmark = pytest.mark.gpu

WIDTHS = [17, 20, 23, 29, 32]  # one live slot in the fifth lane, a whole lane count, ragged tails, the full octet


def _problem(A, N, M, dev, seed, old_sigma_per_row=False):
    g = torch.Generator(device=dev).manual_seed(seed)
    K = 256
    r = lambda *s: torch.randn(*s, device=dev, generator=g)  # noqa: E731
    x = F.elu(r(M, K))
    w, b = r(N, K) / 16, r(N) * 0.1
    wo, bo = r(A, N) / 16, r(A) * 0.1
    sigma = torch.rand(A, device=dev, generator=g) * 0.5 + 0.5
    old_sigma = (sigma * (1.0 + 0.1 * torch.rand(A, device=dev, generator=g))).expand(M, A).contiguous()
    if old_sigma_per_row:  # every third row's sigma_old differs from row 0's bits: the per-element KL expression
        old_sigma[1::3] *= 1.0 + 0.05 * torch.rand(old_sigma[1::3].shape, device=dev, generator=g)
    batch = dict(actions=r(M, A), old_log_prob=r(M, 1) - 1.5 * A, advantages=r(M, 1), target_values=r(M, 1) * 0.3,
                 returns=r(M, 1), old_mu=r(M, A) * 0.1, old_sigma=old_sigma)
    return x, w, b, wo, bo, sigma, r(M, 1) * 0.3, batch


def _images(w, wo):
    return fused_mlp.bimages([(w, False), (wo, False, _lib.BIMAGE_LAYOUT_OUT), (wo, True)])


def _separate(x, w, b, wo, bo, sigma, values, batch, img, out_img, img_t, clipped, kl):
    """Today's launches: the fused forward with H stored, the loss kernel, dgrad + ELU', the weight gradient."""
    A, N = wo.shape
    h, mu = fused_mlp.linear_fwd_out_ex(x, b, N, img, _lib.ARITH_X6, None, bo, out_img, store_h=True)
    stats, gmu, gsig, _ = kernels.ppo_loss_fwd_bwd(
        mu, sigma, values, batch["actions"], batch["old_log_prob"], batch["advantages"], batch["target_values"],
        batch["returns"], batch["old_mu"], batch["old_sigma"], clip_param=0.2, value_loss_coef=1.0,
        entropy_coef=0.01, use_clipped_value_loss=clipped, compute_kl=kl)
    gp = F.pad(gmu, (0, (-A) % 4))
    dz = fused_mlp.linear_dgrad_elu_ex(gp, h, img_t, _lib.ARITH_X6, None, False, want_db=False)[0]
    dw = fused_mlp._weight_grad(gmu, h, True)[0]  # train_backward's output layer: this weight gradient, db = column sums
    return mu, stats.clone(), gmu, gsig.clone(), dz, dw, gmu.sum(0)


def _head(A, M, dev, sigma, values, batch, clipped=True, kl=True, fill=None):
    new = (lambda *s: torch.full(s, fill, device=dev)) if fill is not None else (lambda *s: torch.empty(*s, device=dev))
    head = fused_mlp.ActorHeadWide(
        batch["actions"], batch["old_log_prob"], batch["advantages"], batch["target_values"], batch["returns"],
        batch["old_mu"], batch["old_sigma"], sigma, clip_param=0.2, value_loss_coef=1.0, entropy_coef=0.01,
        use_clipped=clipped, compute_kl=kl, grad_sigma=new(A), stats=new(8), grad_mu=new(M, A))
    head.values = values
    return head


def _fused(x, w, b, wo, bo, sigma, values, batch, img, out_img, img_t, clipped, kl):
    M, N, A = x.shape[0], w.shape[0], wo.shape[0]
    head = _head(A, M, x.device, sigma, values, batch, clipped, kl)
    res = fused_mlp.actor_head_wide_fwd_bwd(x, b, N, img, bo, out_img, img_t, head)
    assert res is not None and head.done
    dz, mu, wpart = res
    assert wpart.shape[1] == A * N + (A + 3) // 4 * 4
    folds = fused_mlp._FoldBatch()
    dwb = torch.empty(A * N + A, device=x.device)
    folds.add(wpart, wpart.shape[0], wpart.shape[1], dwb, A * N + A)
    folds.run(x.device)
    return mu, head.stats, head.grad_mu, head.grad_sigma, dz, dwb[:A * N].view(A, N), dwb[A * N:]


def _err(a, ref):
    return float((a.double() - ref).abs().max() / ref.abs().max())


def _compare(got, sep, p):
    x, w, b, wo = (t.double() for t in p[:4])
    mu, st, gmu, gs, dz, dw, db = got
    mu_r, st_r, gmu_r, gs_r = sep[:4]
    assert torch.equal(mu, mu_r)
    assert torch.equal(gmu, gmu_r)
    assert torch.allclose(st[:5], st_r[:5], rtol=2e-6, atol=1e-9), (st, st_r)
    assert torch.equal(st[5:], st_r[5:])
    assert torch.allclose(gs, gs_r, rtol=1e-5, atol=1e-9)
    # the backward against fp64 from the same inputs (d mu is the loss kernel's, bit for bit)
    h64 = F.elu(x @ w.t() + p[2].double())
    g64 = gmu_r.double()
    refs = ((g64 @ wo) * torch.where(h64 > 0, torch.ones_like(h64), h64 + 1.0), g64.t() @ h64, g64.sum(0))
    for name, a, s, ref in zip(("dz", "dw", "db"), (dz, dw, db), sep[4:], refs):
        e_head, e_sep = _err(a, ref), _err(s, ref)
        print(f"{name}: head {e_head:.3e} separate {e_sep:.3e}")
        assert e_sep > 0.0 and e_head <= 2.0 * e_sep, (name, e_head, e_sep)


def _check(A, N, M, clipped, kl, dev, **kw):
    p = _problem(A, N, M, dev, 21 + 1000 * A + M + N, **kw)
    imgs = _images(p[1], p[3])
    sep = _separate(*p, *imgs, clipped, kl)
    got = _fused(*p, *imgs, clipped, kl)
    torch.cuda.synchronize()
    _compare(got, sep, p)
    again = _fused(*p, *imgs, clipped, kl)  # the launch re-arms its fold tickets: a second run gives the same bits
    torch.cuda.synchronize()
    for u, v in zip(got, again):
        assert torch.equal(u, v)
    return got


@pytest.mark.parametrize("M", [128, 384])
@pytest.mark.parametrize("N", [256, 128, 64])
@pytest.mark.parametrize("A", WIDTHS)
def test_wide_head_matches_separate_launches(A, N, M, cuda_device):
    _check(A, N, M, True, True, cuda_device)


def test_wide_head_crosses_the_fold_group(cuda_device):
    """65 tiles: two fold groups of the 36-column partials."""
    _check(32, 256, 8320, True, True, cuda_device)


@pytest.mark.parametrize("N,clipped,kl", [(256, False, True), (256, True, False), (192, True, True)])
def test_wide_head_without_clipped_value_loss_or_kl_and_at_192(N, clipped, kl, cuda_device):
    _check(23, N, 384, clipped, kl, cuda_device)


@pytest.mark.parametrize("case", ["old_sigma_per_row", "kl_fast_off"])
def test_wide_head_kl_fallbacks_match_loss_kernel(case, cuda_device, monkeypatch):
    """Both KL fall-backs at one width."""
    if case == "kl_fast_off":
        monkeypatch.setenv("RSLRL_KL_FAST", "0")
    got = _check(23, 256, 384, True, True, cuda_device, old_sigma_per_row=case == "old_sigma_per_row")
    assert float(got[1][4]) > 0.0  # the KL of these inputs is not the rollout-consistent ~0


def _guarded(n, dev, band=64):
    buf = torch.full((n + 2 * band,), float("nan"), device=dev)
    return buf, buf[band:band + n]


@pytest.mark.parametrize("A,N", [(17, 256), (23, 192), (32, 64)])
def test_wide_head_writes_nothing_past_its_rows(A, N, cuda_device):
    """mu, d mu, dZ, the partial rows and d sigma inside NaN-filled buffers with 64 floats on either side: the bands
    stay NaN, every output is finite and the partial rows' padding is zero."""
    dev, M = cuda_device, 384
    x, w, b, wo, bo, sigma, values, batch = _problem(A, N, M, dev, 300 + A)
    img, out_img, img_t = _images(w, wo)
    L = _lib.lib()
    tiles = L.rslrl_linear_tiles(M)
    P = A * N + (A + 3) // 4 * 4
    sizes = (("mu", M * A), ("gmu", M * A), ("dz", M * N), ("wpart", tiles * P), ("gsig", A))
    bufs = {k: _guarded(n, dev) for k, n in sizes}
    mu, gmu, dz, wpart, gsig = (bufs[k][1] for k, _ in sizes)
    stats = torch.empty(8, device=dev)
    args = fused_mlp._gemm_args(_lib.LINEAR_FWD_OUT, _lib.ARITH_X6, x, None, N, img, bias=b, c=dz.view(M, N),
                                out_img=out_img, out_bias=bo, y=mu.view(M, A), nout=A)
    h = _lib.ActorHeadArgs(batch["actions"].data_ptr(), batch["old_log_prob"].data_ptr(),
                           batch["advantages"].data_ptr(), values.data_ptr(), batch["target_values"].data_ptr(),
                           batch["returns"].data_ptr(), batch["old_mu"].data_ptr(), batch["old_sigma"].data_ptr(),
                           sigma.data_ptr(), A, 0.2, 1.0, 0.01, 1, 1, img_t.data_ptr(), wpart.data_ptr(),
                           gsig.data_ptr(), stats.data_ptr(), gmu.data_ptr())
    nbytes = L.rslrl_actor_head_wide_workspace_bytes(M)
    ws = torch.zeros(nbytes // 4 + 4, dtype=torch.int32, device=dev)
    st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    assert L.rslrl_actor_head_wide_fwd_bwd(ctypes.byref(args), ctypes.byref(h), ws.data_ptr(), nbytes, st) == 0
    torch.cuda.synchronize()
    for k, (buf, mid) in bufs.items():
        assert bool(torch.isnan(buf[:64]).all()) and bool(torch.isnan(buf[-64:]).all()), k
        assert bool(torch.isfinite(mid).all()), k
    assert bool(torch.isfinite(stats).all())
    assert bool((wpart.view(tiles, P)[:, A * N + A:] == 0).all())


@pytest.mark.parametrize("A,M", [(16, 128), (33, 128), (23, 1000)])
def test_wide_head_declines_unsupported(A, M, cuda_device):
    dev = cuda_device
    x, w, b, wo, bo, sigma, values, batch = _problem(min(A, 32), 256, M, dev, 5)
    img, out_img, img_t = _images(w, wo)
    if A > 32:  # (no image of 33 outputs exists: the head refuses the width before it reads one)
        sigma = torch.ones(A, device=dev)
        batch = {k: (v if v.shape[1] == 1 else v[:, :1].expand(M, A).contiguous()) for k, v in batch.items()}
        bo = torch.zeros(A, device=dev)
    head = _head(A, M, dev, sigma, values, batch, fill=-7.0)
    launches = fused_mlp.actor_head_wide_launches
    assert fused_mlp.actor_head_wide_fwd_bwd(x, b, 256, img, bo, out_img, img_t, head) is None
    torch.cuda.synchronize()
    assert not head.done and fused_mlp.actor_head_wide_launches == launches
    for t in (head.stats, head.grad_sigma, head.grad_mu):
        assert bool((t == -7.0).all())


def _update(A, dims, dev, data):
    from rsl_rl_amd.algorithms import PPO
    from rsl_rl_amd.modules import ActorCritic

    T, N, O = data["obs"].shape
    obs0 = {"policy": torch.zeros(N, O)}
    torch.manual_seed(0)
    pol = ActorCritic(obs0, {"policy": ["policy"], "critic": ["policy"]}, A, actor_hidden_dims=dims,
                      critic_hidden_dims=dims, noise_std_type="scalar")
    alg = PPO(pol, num_learning_epochs=2, num_mini_batches=4, device=dev, desired_kl=0.01)
    alg.init_storage("rl", N, T, obs0, [A])
    st = alg.storage
    st.observations["policy"].copy_(torch.from_numpy(data["obs"]))
    st.rewards.copy_(torch.from_numpy(data["rewards"]))
    st.values.copy_(torch.from_numpy(data["values"]))
    st.actions_log_prob.copy_(torch.from_numpy(data["logp"]) - 1.5 * A)
    st.mu.copy_(torch.from_numpy(data["mu"]) * 0.1)
    st.sigma.copy_(torch.ones(T, N, A))
    st.actions.copy_(torch.from_numpy(data["actions"]))
    st.dones.zero_()
    st.step = T
    with torch.inference_mode():
        alg.compute_returns({"policy": torch.from_numpy(data["last"]).to(dev)})
    st.perm_generator = torch.Generator().manual_seed(1)
    loss = alg.update()
    return loss, alg.learning_rate, {k: v.detach().clone() for k, v in pol.state_dict().items()}


@pytest.mark.parametrize("dims", [[256, 256, 256], [512, 256, 128]])
def test_update_with_wide_head_matches_separate_launches(dims, cuda_device, monkeypatch):
    """PPO.update() at 19 actions with the head and with RSLRL_ACTOR_HEAD_WIDE=0 (the module flag): every parameter
    within 1e-4 of its tensor's largest entry; the 3 x 256 stack takes the paired pass with the head."""
    A, T, N, O = 19, 8, 512, 48  # 4096 rows: 4 mini-batches of 1024 (8 tiles each)
    rng = np.random.default_rng(4)
    data = {k: rng.standard_normal(s).astype(np.float32) for k, s in
            (("obs", (T, N, O)), ("rewards", (T, N, 1)), ("values", (T, N, 1)), ("logp", (T, N, 1)),
             ("mu", (T, N, A)), ("actions", (T, N, A)), ("last", (N, O)))}
    pairs = []
    real = fused_mlp.train_forward_pair
    monkeypatch.setattr(fused_mlp, "train_forward_pair", lambda *a, **k: pairs.append(real(*a, **k)) or pairs[-1])
    results = []
    for on in (True, False):
        monkeypatch.setattr(_lib, "ACTOR_HEAD_WIDE", on)
        launches, n0 = fused_mlp.actor_head_wide_launches, len(pairs)
        results.append(_update(A, dims, cuda_device, data))
        assert fused_mlp.actor_head_wide_launches - launches == (8 if on else 0)
        if on and dims == [256, 256, 256]:
            assert len(pairs) - n0 == 8 and all(r is not None and r[1].head is not None for r in pairs[n0:])
    (l1, lr1, p1), (l0, lr0, p0) = results
    assert lr1 == lr0
    for k in p0:
        assert float((p1[k] - p0[k]).abs().max()) <= 1e-4 * float(p0[k].abs().max()), k
