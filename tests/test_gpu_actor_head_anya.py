"""The actor's fused head for every action count from 5 to 16 (ABI 33; 12 is tests/test_gpu_actor_head.py's) against the
separate launches it replaces, built like that file: mu and d loss / d mu bit for bit (mu: the NR = 4 MFMA output layer
of linear_fwd_out_ex; d mu: the log-prob summed as ppo_loss_fwd_bwd's kernel for that width sums it -- per quad lane
and then over the quad at 8 and 16, ppo_loss_common.h's tree_sum everywhere else), the statistics, d sigma, dZ, dW
and db fp32-close with that file's tolerances.  Then the masked tail of a row at A % 4 != 0 (guard bands), the widths
and shapes the head declines, and a whole PPO.update() with and without it."""

import ctypes

import numpy as np
import pytest
import torch

from rsl_rl_amd import _lib, kernels
from rsl_rl_amd.networks import fused_mlp

pytestmark = pytest.mark.gpu

WIDTHS = [5, 6, 7, 8, 9, 10, 11, 13, 14, 15, 16]


def _problem(A, M, dev, seed, old_sigma_per_row=False):
    g = torch.Generator(device=dev).manual_seed(seed)
    K = N = 256
    r = lambda *s: torch.randn(*s, device=dev, generator=g)  # noqa: E731
    x = torch.nn.functional.elu(r(M, K))
    w, b = r(N, K) / 16, r(N) * 0.1
    wo, bo = r(A, N) / 16, r(A) * 0.1
    sigma = torch.rand(A, device=dev, generator=g) * 0.5 + 0.5
    old_sigma = (sigma * (1.0 + 0.1 * torch.rand(A, device=dev, generator=g))).expand(M, A).contiguous()
    if old_sigma_per_row:  # every third row's sigma_old differs from row 0's bits: the per-element KL expression
        old_sigma[1::3] *= 1.0 + 0.05 * torch.rand(old_sigma[1::3].shape, device=dev, generator=g)
    batch = dict(actions=r(M, A), old_log_prob=r(M, 1) - 8.0, advantages=r(M, 1), target_values=r(M, 1) * 0.3,
                 returns=r(M, 1), old_mu=r(M, A) * 0.1, old_sigma=old_sigma)
    values = r(M, 1) * 0.3
    return x, w, b, wo, bo, sigma, values, batch


def _images(w, wo):
    return fused_mlp.bimages([(w, False), (wo, False, _lib.BIMAGE_LAYOUT_OUT), (wo, True)])


def _separate(x, w, b, wo, bo, sigma, values, batch, img, out_img, img_t, clipped, kl):
    N = w.shape[0]
    h, mu = fused_mlp.linear_fwd_out_ex(x, b, N, img, _lib.ARITH_X6, None, bo, out_img, store_h=True)
    stats, gmu, gsig, _ = kernels.ppo_loss_fwd_bwd(
        mu, sigma, values, batch["actions"], batch["old_log_prob"], batch["advantages"], batch["target_values"],
        batch["returns"], batch["old_mu"], batch["old_sigma"], clip_param=0.2, value_loss_coef=1.0,
        entropy_coef=0.01, use_clipped_value_loss=clipped, compute_kl=kl)
    dz, _, dw, db = fused_mlp.linear_dgrad_elu_wgrad(gmu, wo, h, img_t)
    return mu, stats.clone(), gmu, gsig.clone(), dz, dw, db


def _head(A, M, dev, sigma, values, batch, clipped=True, kl=True, fill=None):
    new = (lambda *s: torch.full(s, fill, device=dev)) if fill is not None else (lambda *s: torch.empty(*s, device=dev))
    head = fused_mlp.ActorHead(batch["actions"], batch["old_log_prob"], batch["advantages"], batch["target_values"],
                               batch["returns"], batch["old_mu"], batch["old_sigma"], sigma, clip_param=0.2,
                               value_loss_coef=1.0, entropy_coef=0.01, use_clipped=clipped, compute_kl=kl,
                               grad_sigma=new(A), stats=new(8), grad_mu=new(M, A))
    head.values = values
    return head


def _fused(x, w, b, wo, bo, sigma, values, batch, img, out_img, img_t, clipped, kl):
    M, N, A = x.shape[0], w.shape[0], wo.shape[0]
    dev = x.device
    head = _head(A, M, dev, sigma, values, batch, clipped, kl)
    res = fused_mlp.actor_head_fwd_bwd(x, b, N, img, bo, out_img, img_t, head)
    assert res is not None and head.done
    dz, mu, wpart = res
    assert wpart.shape[1] == A * N + (A + 3) // 4 * 4
    folds = fused_mlp._FoldBatch()
    dwb = torch.empty(A * N + A, device=dev)
    folds.add(wpart, wpart.shape[0], wpart.shape[1], dwb, A * N + A)
    folds.run(dev)
    return mu, head.stats, head.grad_mu, head.grad_sigma, dz, dwb[:A * N].view(A, N), dwb[A * N:]


def _close(a, b, rtol):
    scale = float(b.abs().max()) + 1e-30
    return torch.allclose(a, b, rtol=rtol, atol=rtol * 0.1 * scale)


def _compare(got, ref):
    mu_r, st_r, gmu_r, gs_r, dz_r, dw_r, db_r = ref
    mu, st, gmu, gs, dz, dw, db = got
    assert torch.equal(mu, mu_r)
    assert torch.equal(gmu, gmu_r)
    assert torch.allclose(st[:5], st_r[:5], rtol=2e-6, atol=1e-9), (st, st_r)
    assert torch.equal(st[5:], st_r[5:])
    assert torch.allclose(gs, gs_r, rtol=1e-5, atol=1e-9)
    assert _close(dz, dz_r, 1e-5)
    assert _close(dw, dw_r, 1e-5)
    assert _close(db, db_r, 1e-5)


def _check(A, M, clipped, kl, dev):
    p = _problem(A, M, dev, 21 + 1000 * A + M)
    imgs = _images(p[1], p[3])
    ref = _separate(*p, *imgs, clipped, kl)
    got = _fused(*p, *imgs, clipped, kl)
    torch.cuda.synchronize()
    _compare(got, ref)
    # the launch re-arms its fold tickets: a second run gives the same bits
    again = _fused(*p, *imgs, clipped, kl)
    torch.cuda.synchronize()
    for u, v in zip(got, again):
        assert torch.equal(u, v)


# one tile; three tiles; 65 tiles = two fold groups
@pytest.mark.parametrize("M", [128, 384, 8320])
@pytest.mark.parametrize("A", WIDTHS)
def test_actor_head_matches_separate_launches(A, M, cuda_device):
    _check(A, M, True, True, cuda_device)


@pytest.mark.parametrize("clipped,kl", [(False, True), (True, False), (False, False)])
@pytest.mark.parametrize("A", WIDTHS)
def test_actor_head_without_clipped_value_loss_or_kl(A, clipped, kl, cuda_device):
    _check(A, 384, clipped, kl, cuda_device)


def test_actor_head_16_actions_folds_in_groups_of_128(cuda_device):
    """4,097 tiles: a grid over kFoldGroup^2 tiles takes the 128-tile fold groups at 20 partial columns."""
    _check(16, 4097 * 128, True, True, cuda_device)


@pytest.mark.parametrize("case", ["old_sigma_per_row", "kl_fast_off"])
@pytest.mark.parametrize("A", [10, 16])
def test_actor_head_kl_fallbacks_match_loss_kernel(A, case, cuda_device, monkeypatch):
    """The KL on rows whose sigma_old is not sample 0's, and with the per-action-constant form switched off
    (RSLRL_KL_FAST=0, read per launch by both kernels): as ppo_loss_fwd_bwd's on the same inputs."""
    dev, M = cuda_device, 1024
    if case == "kl_fast_off":
        monkeypatch.setenv("RSLRL_KL_FAST", "0")
    p = _problem(A, M, dev, 77 + A, old_sigma_per_row=case == "old_sigma_per_row")
    imgs = _images(p[1], p[3])
    ref = _separate(*p, *imgs, True, True)
    got = _fused(*p, *imgs, True, True)
    torch.cuda.synchronize()
    _compare(got, ref)
    assert float(got[1][4]) > 0.0  # the KL of these inputs is not the rollout-consistent ~0


def _guarded(n, dev, band=64):
    """A NaN-filled buffer of band + n + band floats and the view of its middle."""
    buf = torch.full((n + 2 * band,), float("nan"), device=dev)
    return buf, buf[band:band + n]


@pytest.mark.parametrize("A", WIDTHS)
def test_actor_head_writes_nothing_past_its_rows(A, cuda_device):
    """mu, d mu, the partial rows and d sigma inside NaN-filled buffers with 64 floats on either side: the bands stay
    NaN (a masked action of the last quad lane stores nothing) and every output is finite."""
    dev, M, N = cuda_device, 384, 256
    x, w, b, wo, bo, sigma, values, batch = _problem(A, M, dev, 300 + A)
    img, out_img, img_t = _images(w, wo)
    L = _lib.lib()
    tiles = L.rslrl_linear_tiles(M)
    P = A * N + (A + 3) // 4 * 4
    bufs = {k: _guarded(n, dev) for k, n in (("mu", M * A), ("gmu", M * A), ("wpart", tiles * P), ("gsig", A))}
    mu, gmu, wpart, gsig = (bufs[k][1] for k in ("mu", "gmu", "wpart", "gsig"))
    dz = torch.empty(M, N, device=dev)
    stats = torch.empty(8, device=dev)
    args = fused_mlp._gemm_args(_lib.LINEAR_FWD_OUT, _lib.ARITH_X6, x, None, N, img, bias=b, c=dz, out_img=out_img,
                                out_bias=bo, y=mu.view(M, A), nout=A)
    h = _lib.ActorHeadArgs(batch["actions"].data_ptr(), batch["old_log_prob"].data_ptr(),
                           batch["advantages"].data_ptr(), values.data_ptr(), batch["target_values"].data_ptr(),
                           batch["returns"].data_ptr(), batch["old_mu"].data_ptr(), batch["old_sigma"].data_ptr(),
                           sigma.data_ptr(), A, 0.2, 1.0, 0.01, 1, 1, img_t.data_ptr(), wpart.data_ptr(),
                           gsig.data_ptr(), stats.data_ptr(), gmu.data_ptr())
    nbytes = L.rslrl_actor_head_workspace_bytes(M)
    ws = torch.zeros(nbytes // 4 + 4, dtype=torch.int32, device=dev)
    st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    rc = L.rslrl_actor_head_fwd_bwd(ctypes.byref(args), ctypes.byref(h), ws.data_ptr(), nbytes, st)
    assert rc == 0
    torch.cuda.synchronize()
    for k, (buf, mid) in bufs.items():
        assert bool(torch.isnan(buf[:64]).all()) and bool(torch.isnan(buf[-64:]).all()), k
        assert bool(torch.isfinite(mid).all()), k
    assert bool(torch.isfinite(dz).all()) and bool(torch.isfinite(stats).all())
    assert bool((wpart.view(tiles, P)[:, A * N + A:] == 0).all())  # the partial row's padding
    ref_mu = fused_mlp.linear_fwd_out_ex(x, b, N, img, _lib.ARITH_X6, None, bo, out_img, store_h=True)[1]
    assert torch.equal(mu.view(M, A), ref_mu)


@pytest.mark.parametrize("A,M", [(4, 128), (17, 128), (10, 1000)])
def test_actor_head_declines_unsupported(A, M, cuda_device):
    """Fewer than 5 or more than 16 actions, or partial tiles: nothing launched, the caller keeps the separate
    launches."""
    dev = cuda_device
    x, w, b, wo, bo, sigma, values, batch = _problem(A, M, dev, 5)
    img, out_img, img_t = _images(w, wo)
    head = _head(A, M, dev, sigma, values, batch, fill=-7.0)
    launches = fused_mlp.actor_head_launches
    assert fused_mlp.actor_head_fwd_bwd(x, b, 256, img, bo, out_img, img_t, head) is None
    torch.cuda.synchronize()
    assert not head.done and fused_mlp.actor_head_launches == launches
    for t in (head.stats, head.grad_sigma, head.grad_mu):
        assert bool((t == -7.0).all())


def _update(A, noise_std_type, dev, epochs, data):
    from rsl_rl_amd.algorithms import PPO
    from rsl_rl_amd.modules import ActorCritic

    T, N, O = data["obs"].shape
    obs0 = {"policy": torch.zeros(N, O)}
    groups = {"policy": ["policy"], "critic": ["policy"]}
    torch.manual_seed(0)
    pol = ActorCritic(obs0, groups, A, actor_hidden_dims=[256, 256, 256], critic_hidden_dims=[256, 256, 256],
                      noise_std_type=noise_std_type)
    alg = PPO(pol, num_learning_epochs=epochs, num_mini_batches=4, device=dev, desired_kl=0.01)
    alg.init_storage("rl", N, T, obs0, [A])
    st = alg.storage
    st.observations["policy"].copy_(torch.from_numpy(data["obs"]))
    st.rewards.copy_(torch.from_numpy(data["rewards"]))
    st.values.copy_(torch.from_numpy(data["values"]))
    st.actions_log_prob.copy_(torch.from_numpy(data["logp"]) - 10.0)
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


def _data(A, T=8, N=2048, O=48):  # 16384 rows: 4 mini-batches of 4096 (32 tiles each)
    rng = np.random.default_rng(4)
    return {k: rng.standard_normal(s).astype(np.float32) for k, s in
            (("obs", (T, N, O)), ("rewards", (T, N, 1)), ("values", (T, N, 1)), ("logp", (T, N, 1)),
             ("mu", (T, N, A)), ("actions", (T, N, A)), ("last", (N, O)))}


@pytest.mark.parametrize("noise_std_type", ["scalar", "log"])
@pytest.mark.parametrize("A", [7, 16])
def test_update_with_actor_head_matches_separate_launches(A, noise_std_type, cuda_device, monkeypatch):
    """PPO.update() on one storage with the fused actor head and with the separate launches (RSLRL_ACTOR_HEAD off; the
    critic's fused head on in both): the same learning-rate trace and loss statistics, and parameters within fp32
    accumulation-order noise."""
    data = _data(A)
    results = []
    for fused in (True, False):
        monkeypatch.setattr(fused_mlp, "_ACTOR_HEAD", fused)
        calls = []
        real = fused_mlp.actor_head_fwd_bwd
        monkeypatch.setattr(fused_mlp, "actor_head_fwd_bwd", lambda *a, **k: calls.append(1) or real(*a, **k))
        launches = fused_mlp.actor_head_launches
        results.append(_update(A, noise_std_type, cuda_device, 2, data))
        assert len(calls) == (8 if fused else 0)
        assert fused_mlp.actor_head_launches - launches == (8 if fused else 0)
        monkeypatch.setattr(fused_mlp, "actor_head_fwd_bwd", real)
    (l1, lr1, p1), (l0, lr0, p0) = results
    assert lr1 == lr0
    for k in l0:
        assert np.isclose(l1[k], l0[k], rtol=1e-4, atol=1e-7), k
    for k in p0:
        assert torch.allclose(p1[k], p0[k], rtol=1e-4, atol=2e-6), k


@pytest.mark.parametrize("A,want", [(7, 0), (12, 4)])
def test_update_with_the_any_width_knob_off(A, want, cuda_device, monkeypatch):
    """RSLRL_ACTOR_HEAD_ANY=0 (the module flag): 7 actions keep the separate launches, 12 keep the head."""
    monkeypatch.setattr(_lib, "ACTOR_HEAD_ANY", False)
    launches = fused_mlp.actor_head_launches
    _update(A, "scalar", cuda_device, 1, _data(A))
    assert fused_mlp.actor_head_launches - launches == want
