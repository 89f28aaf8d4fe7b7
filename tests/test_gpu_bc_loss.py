"""kernels.bc_loss (rslrl_bc_loss_fwd_bwd) against torch's mse_loss / huber_loss + autograd on the CPU, fp32, step by
step.  Shapes cover a one-element problem, a step start that is not 16-byte aligned (N * A odd), tails that are no
multiple of 4 or 64 elements, and several workgroups per step (N * A > 4096 elements).  pred ~ N(0, 1) and
target = pred + N(0, 1), so both Huber branches are populated.  Tolerance: rtol 1e-5 on the step losses and the
gradient, the project's parity contract for loss scalars and gradients."""

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

# the last two: dense steps that start off a 16-byte boundary (N * A odd), one of them with several workgroups per step
SHAPES = [(1, 1, 1), (1, 65, 3), (2, 193, 12), (3, 256, 4), (15, 64, 12), (2, 4099, 12), (3, 65, 3), (2, 1031, 5)]
LOSSES = {"mse": F.mse_loss, "huber": F.huber_loss}
_cache = {}


def _problem(S, N, A):
    """(pred, target, {loss: (step losses [S], grad [S*N, A])}) on the CPU; computed once per shape."""
    key = (S, N, A)
    if key not in _cache:
        g = torch.Generator().manual_seed(1000 * S + 10 * N + A)
        pred = torch.randn(S * N, A, generator=g)
        target = pred + torch.randn(S * N, A, generator=g)
        ref = {}
        for name, fn in LOSSES.items():
            p = pred.clone().requires_grad_(True)
            steps = [fn(p[s * N:(s + 1) * N], target[s * N:(s + 1) * N]) for s in range(S)]
            torch.stack(steps).sum().backward()
            ref[name] = (torch.stack(steps).detach(), p.grad.clone())
        if A > 1 and N * A > 64:
            d = (pred - target).abs()
            assert 0.1 < (d > 1).float().mean() < 0.9  # both Huber branches
        _cache[key] = (pred, target, ref)
    return _cache[key]


def _run(dev, pred, target, N, loss, pad=False, grad=True):
    from rsl_rl_amd import kernels

    rows, A = pred.shape
    out = torch.full((rows // N,), float("nan"), device=dev)
    g = None
    if grad:
        g = torch.full((rows, A + ((-A) % 4 if pad else 0)), float("nan"), device=dev)
    kernels.bc_loss(pred, target, N, loss, out, g)
    return out, g


def _close(ours, ref):
    assert torch.isfinite(ours).all()
    err = ((ours.double() - ref.double()).abs() / ref.double().abs().clamp_min(1e-30)).max().item()
    assert torch.allclose(ours, ref, rtol=1e-5, atol=0.0), err


@pytest.mark.parametrize("loss", ["mse", "huber"])
@pytest.mark.parametrize("S,N,A", SHAPES)
def test_bc_loss_matches_torch(S, N, A, loss, cuda_device):
    pred, target, ref = _problem(S, N, A)
    ref_loss, ref_grad = ref[loss]
    p, t = pred.to(cuda_device), target.to(cuda_device)
    out, g = _run(cuda_device, p, t, N, loss)
    _close(out.cpu(), ref_loss)
    _close(g.cpu(), ref_grad)

    # the gradient padded to a multiple of four columns: the same values, pad columns exactly zero
    out_p, g_p = _run(cuda_device, p, t, N, loss, pad=True)
    assert torch.equal(out_p, out)
    assert torch.equal(g_p[:, :A], g)
    assert g_p.shape[1] % 4 == 0 and torch.equal(g_p[:, A:], torch.zeros_like(g_p[:, A:]))

    # a strided pred (a column slice of a wider buffer): the same bits as the contiguous one
    wide = torch.randn(S * N, A + 3, device=cuda_device)
    wide[:, 1:1 + A] = p
    out_s, g_s = _run(cuda_device, wide[:, 1:1 + A], t, N, loss)
    assert torch.equal(out_s, out) and torch.equal(g_s, g)

    # forward only: the same step-loss bits
    out_f, _ = _run(cuda_device, p, t, N, loss, grad=False)
    assert torch.equal(out_f, out)

    # deterministic
    out2, g2 = _run(cuda_device, p, t, N, loss)
    assert torch.equal(out2, out) and torch.equal(g2, g)


def test_bc_loss_workspace_rearmed(cuda_device):
    """Calls of different shapes share one workspace: after a many-workgroup call and a call with more steps, the
    first shape still gives its first result (every arrival ticket was left zero)."""
    first = _problem(2, 4099, 12)
    other = _problem(15, 64, 12)
    p, t = first[0].to(cuda_device), first[1].to(cuda_device)
    out, g = _run(cuda_device, p, t, 4099, "mse")
    _run(cuda_device, p, t, 4099, "mse")
    out_o, _ = _run(cuda_device, other[0].to(cuda_device), other[1].to(cuda_device), 64, "huber")
    _close(out_o.cpu(), other[2]["huber"][0])
    out3, g3 = _run(cuda_device, p, t, 4099, "mse")
    assert torch.equal(out3, out) and torch.equal(g3, g)
    _close(out3.cpu(), first[2]["mse"][0])


def test_bc_loss_autograd_function(cuda_device):
    from rsl_rl_amd import kernels

    pred, target, ref = _problem(1, 65, 3)
    p = pred.to(cuda_device).requires_grad_(True)
    loss = kernels.BCLossFunction.apply(p, target.to(cuda_device), "huber")
    (3.0 * loss).backward()
    _close(loss.detach().cpu().reshape(1), ref["huber"][0])
    _close(p.grad.cpu(), 3.0 * ref["huber"][1])
