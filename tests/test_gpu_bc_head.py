"""The distillation head (rslrl_bc_head_fwd_bwd: the student's last hidden layer, output layer, the BC loss per stored
step and the output layer's backward in one launch) against the three launches it replaces on the same inputs --
linear_fwd_out_ex, kernels.bc_loss, linear_dgrad_elu_wgrad -- and against plain fp64 torch on the CPU:

* y, d loss / d y and dZ: the same bits (torch.equal);
* the folded dW and db: the head's per-tile partials add a tile's rows in another order than the separate launch's, so
  they are held to 1e-5 of the tensor's largest entry against it, and dW to 2x the separate launches' own error
  against fp64;
* step_loss: rtol 2e-6 against kernels.bc_loss's (two fp64 sums rounded once), and 2x the separate launches' own error
  against F.mse_loss / F.huber_loss per step in fp64;
* a second launch gives the same bits and the workspace's tickets are zero again;
* every output sits inside NaN guard bands that come back untouched (the masked tail at A = 5 and 11, the tile's zero
  columns); the Huber cases have at least 10 % of the reference's |d| on each side of 1.

Declined shapes return None, launch nothing and leave sentinels intact.  One Distillation.update() on the 3 x 256
fixture runs with the knob on and off."""

import ctypes
import functools

import pytest
import torch
import torch.nn.functional as F

import distill_fixtures as DF
from rsl_rl_amd import _lib, kernels
from rsl_rl_amd.algorithms import distillation
from rsl_rl_amd.networks import fused_mlp

pytestmark = pytest.mark.gpu

K, BAND = 256, 64
ROWS = [(128, 1), (128, 3), (384, 2)]  # (rows per step, steps): one tile; one tile per step; three tiles per step
CASES = [(A, N, rps, S, loss) for A in (5, 8, 11, 16) for N in (64, 256) for rps, S in ROWS for loss in ("mse", "huber")]
CASES.append((11, 128, 384, 2, "huber"))


def _guarded(shape, dev):
    """A NaN-filled buffer with BAND floats on either side of a contiguous view of `shape`."""
    n = 1
    for s in shape:
        n *= s
    buf = torch.full((n + 2 * BAND,), float("nan"), device=dev)
    return buf, buf[BAND:BAND + n].view(shape)


def _bands_untouched(buf):
    return bool(torch.isnan(buf[:BAND]).all()) and bool(torch.isnan(buf[-BAND:]).all())


def _fold(wpart, out_len, dev):
    folds = fused_mlp._FoldBatch()
    dwb = torch.empty(out_len, device=dev)
    folds.add(wpart, wpart.shape[0], wpart.shape[1], dwb, out_len)
    folds.run(dev)
    return dwb


@functools.lru_cache(maxsize=None)
def _case(A, N, rps, S, dev):
    """Inputs, the fp64 CPU reference's forward and the fused forward of one shape, shared by both loss types."""
    M = rps * S
    g = torch.Generator().manual_seed(1000 * N + 10 * M + A)
    r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    x, w, b, wo, bo = F.elu(r(M, K)), r(N, K) / 16, r(N) * 0.1, r(A, N) / 8, r(A) * 0.1
    y64 = F.elu(x.double() @ w.double().t() + b.double()) @ wo.double().t() + bo.double()
    target = (y64 + 1.2 * r(M, A).double()).float()  # |d| on both sides of the Huber threshold
    d = (y64 - target.double()).abs()
    assert 0.1 <= float((d < 1).double().mean()) <= 0.9
    c = {k: v.to(dev) for k, v in dict(x=x, w=w, b=b, wo=wo, bo=bo, target=target.contiguous()).items()}
    c["img"], c["out_img"], c["img_t"] = fused_mlp.bimages([(c["w"], False), (c["wo"], False, _lib.BIMAGE_LAYOUT_OUT),
                                                            (c["wo"], True)])
    c["h"], c["y"] = fused_mlp.linear_fwd_out_ex(c["x"], c["b"], N, c["img"], _lib.ARITH_X6, None, c["bo"],
                                                 c["out_img"], store_h=True)
    c["cpu"] = (x.double(), w.double(), b.double(), wo.double(), bo.double(), target.double())
    return c


def _fp64(c, rps, S, loss):
    """(step losses, dW, db) of the window in fp64 autograd: one F.mse_loss / F.huber_loss per step, summed."""
    x, w, b, wo, bo, target = c["cpu"]
    wo, bo = wo.clone().requires_grad_(), bo.clone().requires_grad_()
    y = F.elu(x @ w.t() + b) @ wo.t() + bo
    fn = F.mse_loss if loss == "mse" else F.huber_loss
    steps = torch.stack([fn(y[s * rps:(s + 1) * rps], target[s * rps:(s + 1) * rps]) for s in range(S)])
    steps.sum().backward()
    return steps.detach(), wo.grad, bo.grad


@pytest.mark.parametrize("A,N,rps,S,loss", CASES)
def test_bc_head_against_three_launches(A, N, rps, S, loss):
    dev = torch.device("cuda")
    M, A4, tiles = rps * S, (A + 3) // 4 * 4, rps * S // 128
    c = _case(A, N, rps, S, dev)
    # ---- the three launches
    gbuf, step_r = torch.empty(M, A4, device=dev), torch.empty(S, device=dev)
    kernels.bc_loss(c["y"], c["target"], rps, loss, step_r, grad_out=gbuf)
    assert not gbuf[:, A:].any()
    dz_r, _, dw_r, db_r = fused_mlp.linear_dgrad_elu_wgrad(gbuf, c["wo"], c["h"], c["img_t"])
    dw_r, db_r = dw_r[:A], db_r[:A]
    # ---- the head, through the C ABI into guarded buffers
    P = A * N + A4
    bufs = {k: _guarded(s, dev) for k, s in dict(y=(M, A), g=(M, A), dz=(M, N), wpart=(tiles, P), step=(S,)).items()}
    y, gout, dz, wpart, step = (bufs[k][1] for k in ("y", "g", "dz", "wpart", "step"))
    L = _lib.lib()
    ws = torch.zeros(L.rslrl_bc_head_workspace_bytes(M, rps), dtype=torch.uint8, device=dev)
    args = fused_mlp._gemm_args(_lib.LINEAR_FWD_OUT, _lib.ARITH_X6, c["x"], None, N, c["img"], bias=c["b"], c=dz,
                                out_img=c["out_img"], out_bias=c["bo"], y=y, nout=A)
    hargs = _lib.BCHeadArgs(c["target"].data_ptr(), A, rps, int(loss == "huber"), c["img_t"].data_ptr(),
                            wpart.data_ptr(), step.data_ptr(), gout.data_ptr())
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    launch = lambda: L.rslrl_bc_head_fwd_bwd(ctypes.byref(args), ctypes.byref(hargs), ws.data_ptr(), ws.numel(), stream)  # noqa: E731
    assert launch() == 0
    first = {k: v[0].clone() for k, v in bufs.items()}
    assert not ws.view(torch.int32)[2::4].any(), "tickets not re-armed"
    assert launch() == 0
    for k, (buf, _) in bufs.items():
        assert torch.equal(buf.view(torch.int32), first[k].view(torch.int32)), f"{k}: second launch differs"
        assert _bands_untouched(buf), f"{k}: guard band written"
    # ---- bits
    assert torch.equal(y, c["y"])
    assert torch.equal(gout, gbuf[:, :A])
    assert torch.equal(dz, dz_r)
    assert not wpart[:, A * N + A:].any()  # the partial rows' padding: sums of the tile's zero columns
    # ---- the folded [dW | db] and the step losses against the separate launches
    dwb = _fold(wpart, A * N + A, dev)
    dw, db = dwb[:A * N].view(A, N), dwb[A * N:]
    for name, a, ref in (("dW", dw, dw_r), ("db", db, db_r)):
        err, top = float((a - ref).abs().max()), float(ref.abs().max())
        print(f"{name}: max |head - launches| {err:.3e}, max |ref| {top:.3e}")
        assert err <= 1e-5 * top
    torch.testing.assert_close(step, step_r, rtol=2e-6, atol=0)
    # ---- against fp64: at most 2x the separate launches' own error
    step64, dw64, _ = _fp64(c, rps, S, loss)
    for name, a, ref, r64 in (("step_loss", step, step_r, step64), ("dW", dw, dw_r, dw64)):
        e_head = float((a.double().cpu() - r64).abs().max())
        e_ref = float((ref.double().cpu() - r64).abs().max())
        print(f"{name}: error against fp64, head {e_head:.3e}, three launches {e_ref:.3e}")
        assert e_head <= 2 * e_ref


@pytest.mark.parametrize("A,rps,k", [(4, 128, 256), (17, 128, 256), (12, 192, 256), (12, 128, 128)])
def test_declined_shapes_launch_nothing(A, rps, k):
    dev = torch.device("cuda")
    M, N = 384, 128
    x, w, b = torch.randn(M, k, device=dev), torch.randn(N, k, device=dev) / 16, torch.zeros(N, device=dev)
    bo = torch.zeros(A, device=dev)
    step = torch.full((M // rps,), float("nan"), device=dev)
    head = fused_mlp.BCHead(torch.zeros(M, A, device=dev), rps, "mse", step)
    before = fused_mlp.bc_head_launches
    # (a declined call returns before it looks at an image: the weight stands in for all three)
    assert fused_mlp.bc_head_fwd_bwd(x, b, N, w, bo, w, w, head) is None
    assert fused_mlp.bc_head_launches == before and not head.done and bool(torch.isnan(step).all())


def test_update_with_and_without_the_head(monkeypatch):
    """One update() of the 3 x 256 fixture (256 envs, 12 actions, one optimizer step): the parameters within 1e-4 of each
    tensor's largest entry (dW is not bit-equal), the loss within 1e-6 relative, and the launch counter."""
    dev = torch.device("cuda")
    meta = DF.load_meta()["c"]
    z = DF.load_arrays("c", meta)
    res = {}
    for on in (True, False):
        monkeypatch.setattr(distillation, "_BC_HEAD", on)
        alg, pol = DF.build_distillation(z, meta, 0, dev)
        before = fused_mlp.bc_head_launches
        loss = alg.update()
        steps = sum(full for _, full in distillation.distillation_windows(meta["T"], meta["E"], meta["G"]))
        assert fused_mlp.bc_head_launches - before == (steps if on else 0)
        res[on] = (loss, {k: v.detach().clone() for k, v in pol.student.state_dict().items()})
    assert res[True][0]["behavior"] == pytest.approx(res[False][0]["behavior"], rel=1e-6)
    for k, v in res[False][1].items():
        assert float((res[True][1][k] - v).abs().max()) <= 1e-4 * float(v.abs().max()), k
