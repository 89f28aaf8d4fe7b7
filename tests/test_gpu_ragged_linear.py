"""The ragged first-layer kernels (csrc/mlp_ragged.hip) against their exact oracle: today's entry
points on the zero-padded problem -- x padded to Kp = K + (-K) % 4 columns, W padded with zero columns, the pad column
of dW dropped -- compared with torch.equal.  Operands and outputs lie inside larger NaN-filled buffers: the results
must be finite and equal to the oracle's, and every guard float untouched.  (That no load leaves the operand is read
off the loader, csrc/ragged_load.h; an over-read inside an allocation cannot be caught here.)"""

import ctypes

import pytest
import torch

import wide_plan
from rsl_rl_amd.networks import fused_mlp
from rsl_rl_amd.networks.fused_mlp import (bimage, bimage_wide, linear_fwd_ex, linear_fwd_ragged, linear_wgrad,
                                           linear_wgrad_ragged, linear_wgrad_wide)
from rsl_rl_amd import _lib

pytestmark = pytest.mark.gpu

GUARD = 64  # floats in front of and behind each view (256 bytes: the views stay 16-byte aligned)
SMALL_KN = [(K, N) for K in (1, 5, 19, 47, 63) for N in (64, 256)]
LARGE_KN = [(K, N) for K in (65, 77, 235, 255) for N in (256, 260, 512)] + [(1021, 512)]
FWD_M = (1, 63, 128, 200, 256)


def _guarded(t):
    """A copy of t as a view inside a NaN-filled buffer; returns (view, buffer)."""
    buf = torch.full((t.numel() + 2 * GUARD,), float("nan"), device=t.device)
    view = buf[GUARD:GUARD + t.numel()].view(t.shape)
    view.copy_(t)
    return view, buf


def _guards_untouched(buf, n):
    return bool(torch.isnan(buf[:GUARD]).all() and torch.isnan(buf[GUARD + n:]).all())


def _pad(t):
    return torch.nn.functional.pad(t, (0, (-t.shape[1]) % 4))


def _image(w):
    return bimage_wide(w, False) if w.shape[0] > 256 else bimage(w, False)


def _fwd_padded(x, w, b, elu):
    xp, wp = _pad(x).contiguous(), _pad(w).contiguous()
    wide = fused_mlp._wide_layer(*wp.shape)
    return linear_fwd_ex(xp, b, w.shape[0], elu, _image(wp), _lib.ARITH_X6, wide=wide)[0]


@pytest.fixture(scope="module")
def fwd_data(cuda_device):
    """Per (K, N): x for the largest M (smaller M take its first rows), W, b and the padded oracle per (M, elu)."""
    torch.manual_seed(21)
    data = {}
    for K, N in SMALL_KN + LARGE_KN:
        x = torch.randn(max(FWD_M), K, device=cuda_device)
        w = torch.randn(N, K, device=cuda_device) / K ** 0.5
        b = torch.randn(N, device=cuda_device)
        ref = {(M, elu): _fwd_padded(x[:M].contiguous(), w, b, elu) for M in FWD_M for elu in (False, True)}
        data[(K, N)] = (x, w, b, ref)
    return data


@pytest.mark.parametrize("elu", [False, True])
@pytest.mark.parametrize("K,N", SMALL_KN + LARGE_KN)
def test_forward_equals_padded_problem(K, N, elu, fwd_data, cuda_device):
    x, w, b, ref = fwd_data[(K, N)]
    img = _image(w)  # the image functions take the ragged depth as it is
    assert torch.equal(img, _image(_pad(w).contiguous()))
    b, bbuf = _guarded(b)
    img, ibuf = _guarded(img)  # (GUARD floats = 256 bytes: the view keeps the image's 16-byte alignment)
    for M in FWD_M:
        xv, xbuf = _guarded(x[:M])
        # the output inside a NaN buffer too: the entry writes c through the args, so call it on a guarded view
        cbuf = torch.full((M * N + 2 * GUARD,), float("nan"), device=cuda_device)
        cv = cbuf[GUARD:GUARD + M * N].view(M, N)
        args = fused_mlp._gemm_args(_lib.LINEAR_FWD_ELU if elu else _lib.LINEAR_FWD, _lib.ARITH_X6, xv, None, N, img,
                                    bias=b, c=cv)
        rc = _lib.lib().rslrl_linear_gemm_ragged(ctypes.byref(args), fused_mlp._stream(xv))
        assert rc == 0
        assert torch.isfinite(cv).all()
        assert torch.equal(cv, ref[(M, elu)]), (M, K, N, (cv - ref[(M, elu)]).abs().max().item())
        assert _guards_untouched(cbuf, M * N) and _guards_untouched(xbuf, M * K) and _guards_untouched(bbuf, N)
        assert _guards_untouched(ibuf, img.numel())
        assert torch.equal(linear_fwd_ragged(xv, b, N, elu, img), ref[(M, elu)])


def _wgrad_padded(dz, x, with_bias):
    """_weight_grad's dispatch of the padded problem: (dw [N, K], db or None)."""
    N, K = dz.shape[1], x.shape[1]
    xp = _pad(x).contiguous()
    Kp = xp.shape[1]
    wide = fused_mlp._wide_layer(N, Kp)
    if K <= 64 < N:  # (x^T dz)^T, the bias on the kernel's K side
        f = linear_wgrad_wide if wide else linear_wgrad
        if with_bias:
            dwt, db = f(xp, dz, bias_side=2)
            return dwt[:K].t().contiguous(), db
        return f(xp, dz)[:K].t().contiguous(), None
    f = linear_wgrad_wide if wide else linear_wgrad
    if with_bias:
        dw, db = f(dz, xp, bias_side=1)
        return dw[:, :K].contiguous(), db
    return f(dz, xp)[:, :K].contiguous(), None


def _full_m(K, N):
    """The smallest M (a multiple of 16) at which the padded problem takes the full-tile look-ahead variant, or None."""
    Kp = K + (-K) % 4
    wide = N > 256 or Kp > 256
    for M in range(32, 4097, 16):
        if K <= 64 < N:
            plan = wide_plan.wgrad_plan(M, Kp, N) if wide else wide_plan.dense_wgrad_plan(M, Kp, N)
        else:
            plan = wide_plan.wgrad_plan(M, N, Kp) if wide else wide_plan.dense_wgrad_plan(M, N, Kp)
        if plan.full:
            return M
    return None


WGRAD_KN = [(K, N) for K, N in SMALL_KN + LARGE_KN if fused_mlp.ragged_wgrad_ok(N, K)]


def test_wgrad_grid_covers_every_form():
    assert {(K, N) for K, N in SMALL_KN if N == 256} <= set(WGRAD_KN) and set(LARGE_KN) <= set(WGRAD_KN)
    assert _full_m(47, 256) is not None and _full_m(255, 256) is not None and _full_m(1021, 512) is not None
    assert _full_m(235, 512) is None  # 236 columns are no whole 256-column block: the general loop at every M


@pytest.mark.parametrize("K,N", WGRAD_KN)
def test_wgrad_equals_padded_problem(K, N, cuda_device):
    torch.manual_seed(K * 1031 + N)
    ms = [64, 200, 256]
    fm = _full_m(K, N)
    if fm is not None and fm not in ms:
        ms.append(fm)
    x_all = torch.randn(max(ms), K, device=cuda_device)
    dz_all = torch.randn(max(ms), N, device=cuda_device)
    for M in ms:
        x, dz = x_all[:M].contiguous(), dz_all[:M].contiguous()
        xv, xbuf = _guarded(x)
        dzv, dzbuf = _guarded(dz)
        for with_bias in (False, True):
            if with_bias and N <= 64:
                continue
            ref_w, ref_b = _wgrad_padded(dz, x, with_bias)
            n_out = N * K + (N if with_bias else 0)
            obuf = torch.full((n_out + 2 * GUARD,), float("nan"), device=cuda_device)
            out = obuf[GUARD:GUARD + n_out]
            if with_bias:
                dw, db = linear_wgrad_ragged(dzv, xv, with_bias=True, dwb_out=out)
                assert torch.equal(db, ref_b), (M, K, N)
            else:
                dw = linear_wgrad_ragged(dzv, xv, out=out.view(N, K))
            assert torch.isfinite(out).all()
            assert torch.equal(dw, ref_w), (M, K, N, with_bias, (dw - ref_w).abs().max().item())
            assert _guards_untouched(obuf, n_out) and _guards_untouched(xbuf, M * K) and _guards_untouched(dzbuf, M * N)
            again = linear_wgrad_ragged(dzv, xv, with_bias=with_bias)
            again = torch.cat([again[0].flatten(), again[1]]) if with_bias else again.flatten()
            assert torch.equal(again, out)  # deterministic: two calls, the same bits


def test_accuracy_against_fp64(cuda_device):
    """K = 235, N = 512, M = 256 against fp64 with the bounds tests/test_gpu_fused_mlp.py applies to x6
    (test_x6_error_matches_fp32): RMS error within 2x and max error within 3x of torch's fp32 GEMM on the same data."""
    torch.manual_seed(235 * 512)
    F = torch.nn.functional
    M, K, N = 256, 235, 512
    x = torch.randn(M, K, device=cuda_device)
    w = torch.randn(N, K, device=cuda_device) / K ** 0.5
    b = torch.randn(N, device=cuda_device)
    ref = F.linear(x.double(), w.double(), b.double())
    ref = torch.where(ref > 0, ref, torch.expm1(ref))
    ours = linear_fwd_ragged(x, b, N, True, _image(w))
    torch_fp32 = F.elu(F.linear(x, w, b))

    def err(a):
        d = a.double() - ref
        return d.abs().max().item(), d.square().mean().sqrt().item(), d.mean().item()

    (m_ours, r_ours, b_ours), (m_fp32, r_fp32, _) = err(ours), err(torch_fp32)
    print("ragged fwd vs fp64: rms", r_ours, "fp32 rms", r_fp32, "max", m_ours, "fp32 max", m_fp32, "bias", b_ours)
    assert r_ours <= 2.0 * r_fp32, (r_ours, r_fp32)
    assert m_ours <= 3.0 * m_fp32, (m_ours, m_fp32)
    assert abs(b_ours) <= 0.25 * r_ours, (b_ours, r_ours)
    dz = torch.randn(M, N, device=cuda_device)
    dw, db = linear_wgrad_ragged(dz, x, with_bias=True)
    ref_w = dz.double().t().mm(x.double())
    e_ours = (dw.double() - ref_w).square().mean().sqrt().item()
    e_fp32 = (dz.t().mm(x).double() - ref_w).square().mean().sqrt().item()
    print("ragged wgrad vs fp64: rms", e_ours, "fp32 rms", e_fp32)
    assert e_ours <= 2.0 * e_fp32, (e_ours, e_fp32)
    assert (db.double() - dz.double().sum(0)).abs().max().item() <= 1e-4 * dz.double().sum(0).abs().max().item()
