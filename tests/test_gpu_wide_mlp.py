"""Linear + ELU layers wider than 256 on the wide entry points (csrc/mlp_wide.hip) against PyTorch-ROCm,
and every 256-column block of a wide GEMM against the tiled kernel on the dense block, bit for bit.  _close /
_reference / TOL are tests/test_gpu_fused_mlp.py's."""

import pytest
import torch

from rsl_rl_amd import _lib
from rsl_rl_amd.networks import MLP, fused_mlp
from rsl_rl_amd.networks.fused_mlp import bimage, bimage_wide, linear_dgrad_elu_ex, linear_fwd_ex, linear_wgrad_wide

pytestmark = pytest.mark.gpu

TOL = 1e-5
F = torch.nn.functional
X6 = _lib.ARITH_X6
KN = [(4, 260), (48, 512), (320, 260), (512, 256), (512, 1024)]
SHAPES = [(1, 4, 260), (129, 48, 512), (200, 320, 260), (200, 512, 256), (3001, 512, 1024)]


def _close(a, b, tol=TOL):
    assert (a - b).abs().max().item() <= tol * b.abs().max().item() + 1e-12, (a - b).abs().max().item()


def _reference(mlp, x):
    y = x
    for layer in mlp:
        y = layer(y)
    return y


def _fwd_case(M, K, N, dev):
    torch.manual_seed(M + K + N)
    return (torch.randn(M, K, device=dev), torch.randn(N, K, device=dev) / K ** 0.5, torch.randn(N, device=dev))


def _dgrad_case(M, K, N, dev):
    """dz [M, K] through W [K, N] (the layer's weight: K outputs, N inputs), gated by h [M, N]."""
    torch.manual_seed(M + K + N + 1)
    return (torch.randn(M, K, device=dev), torch.randn(K, N, device=dev) / K ** 0.5,
            F.elu(torch.randn(M, N, device=dev)))


@pytest.mark.parametrize("M,K,N", SHAPES)
@pytest.mark.parametrize("elu", [True, False])
def test_wide_forward(M, K, N, elu, cuda_device):
    x, w, b = _fwd_case(M, K, N, cuda_device)
    before = fused_mlp.wide_launches
    img = bimage_wide(w, False)
    y, _ = linear_fwd_ex(x, b, N, elu, img, X6, wide=True)
    assert fused_mlp.wide_launches == before + 1
    ref = F.linear(x, w, b)
    _close(y, F.elu(ref) if elu else ref)
    assert torch.equal(y, linear_fwd_ex(x, b, N, elu, img, X6, wide=True)[0])  # a repeated call: the same bits


@pytest.mark.parametrize("M,K,N", SHAPES)
def test_wide_input_gradient(M, K, N, cuda_device):
    dz, w, h = _dgrad_case(M, K, N, cuda_device)
    img = bimage_wide(w, True)
    out, db, _ = linear_dgrad_elu_ex(dz, h, img, X6, wide=True)
    ref = dz.mm(w)
    ref = torch.where(h > 0, ref, ref * (h + 1))
    _close(out, ref)
    _close(db, ref.double().sum(0).float(), 1e-4)
    out2, db2, _ = linear_dgrad_elu_ex(dz, h, img, X6, wide=True)
    assert torch.equal(out, out2) and torch.equal(db, db2)
    assert linear_dgrad_elu_ex(dz, h, img, X6, want_db=False, wide=True)[1] is None


@pytest.mark.parametrize("K,N", KN)
def test_wide_blocks_are_the_dense_kernels_bits(K, N, cuda_device):
    """M = 200 is no multiple of the 128-row tile, so the dense call takes the tiled kernel (no streaming form)."""
    M = 200
    x, w, b = _fwd_case(M, K, N, cuda_device)
    dz, wt, h = _dgrad_case(M, K, N, cuda_device)
    for elu in (True, False):
        y, _ = linear_fwd_ex(x, b, N, elu, bimage_wide(w, False), X6, wide=True)
        for c0 in range(0, N, 256):
            wb, bb = w[c0:c0 + 256].contiguous(), b[c0:c0 + 256].contiguous()
            dense, _ = linear_fwd_ex(x, bb, wb.shape[0], elu, bimage(wb, False), X6)
            assert torch.equal(y[:, c0:c0 + 256], dense), (elu, c0)
    out, db, _ = linear_dgrad_elu_ex(dz, h, bimage_wide(wt, True), X6, wide=True)
    for c0 in range(0, N, 256):
        wb, hb = wt[:, c0:c0 + 256].contiguous(), h[:, c0:c0 + 256].contiguous()
        dense, dbb, _ = linear_dgrad_elu_ex(dz, hb, bimage(wb, True), X6)
        assert torch.equal(out[:, c0:c0 + 256], dense), c0
        assert torch.equal(db[c0:c0 + 256], dbb), c0


def test_wide_full_tiles_k256_are_the_dense_kernels_bits(cuda_device):
    """Whole 128-row tiles at a reduction depth of 256: the unrolled look-ahead main loop, the one the input gradient
    256 -> 512 of [512, 256, 128] takes in the update.  The dense single-problem entry has no streaming form, so at
    M = 256 it runs the tiled kernel's same loop on the dense block."""
    M, K, N = 256, 256, 512
    x, w, b = _fwd_case(M, K, N, cuda_device)
    dz, wt, h = _dgrad_case(M, K, N, cuda_device)
    for elu in (True, False):
        y, _ = linear_fwd_ex(x, b, N, elu, bimage_wide(w, False), X6, wide=True)
        ref = F.linear(x, w, b)
        _close(y, F.elu(ref) if elu else ref)
        for c0 in range(0, N, 256):
            wb, bb = w[c0:c0 + 256].contiguous(), b[c0:c0 + 256].contiguous()
            dense, _ = linear_fwd_ex(x, bb, 256, elu, bimage(wb, False), X6)
            assert torch.equal(y[:, c0:c0 + 256], dense), (elu, c0)
    out, db, _ = linear_dgrad_elu_ex(dz, h, bimage_wide(wt, True), X6, wide=True)
    ref = dz.mm(wt)
    ref = torch.where(h > 0, ref, ref * (h + 1))
    _close(out, ref)
    _close(db, ref.double().sum(0).float(), 1e-4)
    for c0 in range(0, N, 256):
        wb, hb = wt[:, c0:c0 + 256].contiguous(), h[:, c0:c0 + 256].contiguous()
        dense, dbb, _ = linear_dgrad_elu_ex(dz, hb, bimage(wb, True), X6)
        assert torch.equal(out[:, c0:c0 + 256], dense), c0
        assert torch.equal(db[c0:c0 + 256], dbb), c0


def test_wide_image_is_the_block_images(cuda_device):
    torch.manual_seed(5)
    w = torch.randn(520, 320, device=cuda_device)
    for tr in (False, True):
        rows = w.shape[1] if tr else w.shape[0]
        wide = bimage_wide(w, tr)
        per = wide.numel() // ((rows + 255) // 256)
        for j, c0 in enumerate(range(0, rows, 256)):
            blk = (w[:, c0:c0 + 256] if tr else w[c0:c0 + 256]).contiguous()
            assert torch.equal(wide[j * per:(j + 1) * per], bimage(blk, tr)), (tr, j)


@pytest.mark.parametrize("kind", ["fwd", "dgrad"])
def test_wide_x6_error_matches_fp32(kind, cuda_device):
    """tests/test_gpu_fused_mlp.py test_x6_error_matches_fp32's rule at a wide shape: against fp64 the RMS error within
    2x and the max error within 3x of torch fp32's on the same data."""
    M, K, N = 4096, 512, 512
    if kind == "fwd":
        x, w, b = _fwd_case(M, K, N, cuda_device)
        ref = F.linear(x.double(), w.double(), b.double())
        ref = torch.where(ref > 0, ref, torch.expm1(ref))
        ours = linear_fwd_ex(x, b, N, True, bimage_wide(w, False), X6, wide=True)[0]
        torch_fp32 = F.elu(F.linear(x, w, b))
    else:
        dz, w, h = _dgrad_case(M, K, N, cuda_device)
        d = dz.double().mm(w.double())
        ref = torch.where(h > 0, d, d * (h.double() + 1))
        ours = linear_dgrad_elu_ex(dz, h, bimage_wide(w, True), X6, wide=True)[0]
        d32 = dz.mm(w)
        torch_fp32 = torch.where(h > 0, d32, d32 * (h + 1))

    def err(a):
        d = a.double() - ref
        return d.abs().max().item(), d.square().mean().sqrt().item()

    (m_ours, r_ours), (m_fp32, r_fp32) = err(ours), err(torch_fp32)
    print(kind, "rms ours / fp32", r_ours, r_fp32, "max ours / fp32", m_ours, m_fp32)
    assert r_ours <= 2.0 * r_fp32, (r_ours, r_fp32)
    assert m_ours <= 3.0 * m_fp32, (m_ours, m_fp32)


@pytest.mark.parametrize("M,N,K", [(200, 320, 16), (3001, 260, 320), (3001, 512, 512)])
@pytest.mark.parametrize("bias_side", [0, 1, 2])
def test_wide_weight_gradient(M, N, K, bias_side, cuda_device):
    torch.manual_seed(M + N + K)
    dz = torch.randn(M, N, device=cuda_device)
    x = F.elu(torch.randn(M, K, device=cuda_device))
    ref = dz.double().t().mm(x.double()).float()
    before = fused_mlp.wide_launches
    res = linear_wgrad_wide(dz, x, bias_side=bias_side)
    assert fused_mlp.wide_launches == before + 1
    dw, cs = res if bias_side else (res, None)
    _close(dw, ref)
    if bias_side:
        _close(cs, (dz if bias_side == 1 else x).double().sum(0).float(), 2e-5)
    again = linear_wgrad_wide(dz, x, bias_side=bias_side)
    assert torch.equal(dw, again[0] if bias_side else again)
    if bias_side:
        assert torch.equal(cs, again[1])
        # in place in a larger buffer (a gradient arena's slots): the neighbouring floats stay
        n = N * K + cs.numel()
        buf = torch.full((n + 64,), 7.5, device=cuda_device)
        dw2, cs2 = linear_wgrad_wide(dz, x, bias_side=bias_side, dwb_out=buf[32:32 + n])
        assert dw2.data_ptr() == buf.data_ptr() + 4 * 32
        assert torch.equal(dw2, dw) and torch.equal(cs2, cs)
        assert torch.all(buf[:32] == 7.5) and torch.all(buf[32 + n:] == 7.5)
    else:
        buf = torch.full((N * K + 64,), 7.5, device=cuda_device)
        dw2 = linear_wgrad_wide(dz, x, out=buf[32:32 + N * K].view(N, K))
        assert torch.equal(dw2, dw) and torch.all(buf[:32] == 7.5) and torch.all(buf[32 + N * K:] == 7.5)


def test_wide_weight_gradient_swapped_form(cuda_device):
    """A wide layer with at most 64 inputs (the first layer): (x^T dz)^T on the 64-row tiles, the bias from dz."""
    torch.manual_seed(9)
    dz = torch.randn(3001, 512, device=cuda_device)
    x = torch.randn(3001, 48, device=cuda_device)
    dw, db = fused_mlp._weight_grad(dz, x, True, want_bias=True, wide=True)
    _close(dw, dz.double().t().mm(x.double()).float())
    _close(db, dz.double().sum(0).float(), 2e-5)
    assert dw.shape == (512, 48) and dw.is_contiguous()


@pytest.mark.parametrize("din,dout,hidden", [(48, 12, [512, 256, 128]), (48, 1, [512, 256, 128]),
                                             (16, 4, [320, 260, 64]), (48, [2, 12], [1024, 512, 256])])
def test_wide_stack_forward_backward(din, dout, hidden, cuda_device):
    _stack_forward_backward(3001, din, dout, hidden, cuda_device)


@pytest.mark.parametrize("din,dout,hidden", [(48, 12, [512, 256, 128]), (48, [2, 12], [1024, 512, 256])])
@pytest.mark.parametrize("M", [1024, 4096])
def test_wide_stack_forward_backward_whole_tiles(M, din, dout, hidden, cuda_device):
    """Row counts of whole tiles: every wide layer's weight gradient takes the look-ahead variant (the first layer's the
    masked 64-row one) and every wide GEMM the unmasked one (tests/wide_plan.py; 3001 rows take neither)."""
    _stack_forward_backward(M, din, dout, hidden, cuda_device)


def _stack_forward_backward(M, din, dout, hidden, cuda_device):
    torch.manual_seed(7)
    mlp = MLP(din, dout, hidden, "elu").to(cuda_device)
    assert mlp._wide and not mlp._fused
    x = torch.randn(M, din, device=cuda_device, requires_grad=True)
    before = fused_mlp.wide_launches
    y = mlp(x)
    g = torch.randn_like(y)
    y.backward(g)
    assert fused_mlp.wide_launches > before
    ours = [p.grad.clone() for p in mlp.parameters()]
    gx = x.grad.clone()
    mlp.zero_grad()
    x.grad = None
    ref = _reference(mlp, x)
    _close(y, ref)
    ref.backward(g)
    for (name, p), a in zip(mlp.named_parameters(), ours):
        _close(a, p.grad, 2e-5 if "bias" in name else TOL)
    _close(gx, x.grad)
    with torch.inference_mode():
        _close(mlp(x.detach()), ref.detach())


def test_wide_stack_inference_forward(cuda_device):
    """A forward that nothing differentiates takes the wide kernels from WIDE_FWD_MIN_ROWS rows on -- the training
    forward's bits -- and runs layer by layer below."""
    torch.manual_seed(2)
    mlp = MLP(48, 12, [512, 256, 128], "elu").to(cuda_device)
    M = fused_mlp.WIDE_FWD_MIN_ROWS
    x = torch.randn(M, 48, device=cuda_device)
    y = mlp(x)  # under autograd: FusedMLPFunction
    before = fused_mlp.wide_launches
    with torch.inference_mode():
        z = mlp(x)
        assert fused_mlp.wide_launches == before + 2  # the two layers wider than 256; the last two run fused as one
        assert torch.equal(z, y.detach())
        _close(z, _reference(mlp, x))
        with fused_mlp.frozen_weights():
            assert torch.equal(mlp(x), z) and torch.equal(mlp(x), z)  # cached block images
        small = mlp(x[:M - 128])
        assert fused_mlp.wide_launches == before + 6
        assert torch.equal(small, _reference(mlp, x[:M - 128]))


def test_wide_stack_gradients_into_arena_slots(cuda_device):
    """train_backward with adjacent (dW, db) destinations, as the PPO update's gradient arena hands them over."""
    _gradients_into_arena_slots(lambda: MLP(16, 4, [320, 260, 64], "elu"), 1000, cuda_device)


def test_wide_stack_gradients_into_arena_slots_whole_tiles(cuda_device):
    """The default policy's widths at 1024 rows: the look-ahead weight-gradient variants write the slots (the
    [320, 260, 64] stack has no full tile at any row count: no side of it is a multiple of 256)."""
    _gradients_into_arena_slots(lambda: MLP(48, 12, [512, 256, 128], "elu"), 1024, cuda_device)


def _gradients_into_arena_slots(make, rows, cuda_device):
    torch.manual_seed(3)
    mlp = make().to(cuda_device)
    lin = [m for m in mlp if isinstance(m, torch.nn.Linear)]
    ws, bs = [m.weight for m in lin], [m.bias for m in lin]
    x = torch.randn(rows, lin[0].in_features, device=cuda_device)
    flat = torch.full((sum(w.numel() + b.numel() for w, b in zip(ws, bs)) + 8,), 3.25, device=cuda_device)
    outs, off = [], 4
    for w, b in zip(ws, bs):
        outs.append((flat[off:off + w.numel()].view_as(w), flat[off + w.numel():off + w.numel() + b.numel()]))
        off += w.numel() + b.numel()
    with torch.no_grad():
        y, tape = fused_mlp.train_forward(x, ws, bs)
        g = torch.randn_like(y)
        fused_mlp.train_backward(tape, g, outs=outs)
    ref = _reference(mlp, x)
    ref.backward(g)
    for (wo, bo), m in zip(outs, lin):
        _close(wo, m.weight.grad)
        _close(bo, m.bias.grad, 2e-5)
    assert torch.all(flat[:4] == 3.25) and torch.all(flat[-4:] == 3.25)


def test_wide_stack_other_modes_stay_layer_by_layer(cuda_device):
    torch.manual_seed(1)
    mlp = MLP(48, 12, [512, 256, 128], "elu").to(cuda_device)
    x = torch.randn(300, 48, device=cuda_device)
    for mode in (fused_mlp.GEMM_F32, fused_mlp.GEMM_H3):
        prev = fused_mlp.set_gemm_mode(mode)
        try:
            before = fused_mlp.wide_launches
            with torch.no_grad():
                y = mlp(x)
            assert fused_mlp.wide_launches == before and torch.equal(y, _reference(mlp, x).detach())
        finally:
            fused_mlp.set_gemm_mode(prev)
