"""The full-tile variants of the wide kernels (csrc/mlp_wide.hip), the ones every real update takes:
the look-ahead ring of wgrad_x6_body (csrc/mlp_wgrad_x6.h, FULL: kWgradDepth chunks in registers, loads past the slice
end clamped to the last chunk, a hand-written waitcnt + barrier, unconditional masked loads on a dz side narrower than
64) and the FULL instantiations of mlp_gemm_x6_wide_kernel off the K = 256 loop.  tests/wide_plan.py says which variant a
shape takes and tests/test_wide_host.py holds that to the library, so these shapes cannot drift off their variants.

Two kinds of check.  Exact: small-integer operands are exact in the first bf16 plane of the x6 split (the two lower
planes are zero), every product and every fp32 partial sum is an integer below 2^24 and the fp64 fold is exact, so the
result must equal the integer product -- no tolerance; a chunk of the ring dropped, counted twice or paired with the
wrong partner, or a column sum that counts a clamped look-ahead load, changes integers.  Float: the rule of
tests/test_gpu_fused_mlp.py test_linear_wgrad and tests/test_gpu_wide_mlp.py on random data, with their constants."""

import functools

import pytest
import torch

import wide_plan
from rsl_rl_amd import _lib
from rsl_rl_amd.networks import fused_mlp
from rsl_rl_amd.networks.fused_mlp import bimage, bimage_wide, linear_dgrad_elu_ex, linear_fwd_ex, linear_wgrad_wide

pytestmark = pytest.mark.gpu

F = torch.nn.functional
X6 = _lib.ARITH_X6
EXACT_BOUND = 2 ** 22  # rows x max |a| x max |b|: every fp32 partial sum stays an exactly represented integer


def _close(a, b, tol=1e-5):
    assert (a - b).abs().max().item() <= tol * b.abs().max().item() + 1e-12, (a - b).abs().max().item()


def _ints(shape, lo, hi, dev, gen):
    return torch.randint(lo, hi + 1, shape, generator=gen, device="cpu").float().to(dev)


def _exact_product(a, b):
    """a^T b of integer-valued fp32 matrices, exact: fp64 holds every sum here (far below 2^53), so this is
    a.long().t() @ b.long(), for which the GPU has no kernel; small cases are held to that on the host."""
    ref = a.double().t().mm(b.double())
    assert torch.equal(ref, ref.round())
    if a.shape[0] <= 128:
        assert torch.equal(ref.cpu().long(), a.cpu().long().t() @ b.cpu().long())
    return ref


@functools.lru_cache(maxsize=2)
def _int_case(M, N, K, dev):
    """Integer dz [M, N], x [M, K] in [-3, 3]; the last chunk of 16 rows one higher, in [-2, 4] -- its column sums are
    16 above a middle chunk's in expectation, so a clamped look-ahead load (the last chunk again) that reached dW or a
    column sum could not cancel.  With the exact dW and column sums, computed once per shape."""
    gen = torch.Generator().manual_seed(1000003 * M + 1009 * N + K)
    dz, x = _ints((M, N), -3, 3, dev, gen), _ints((M, K), -3, 3, dev, gen)
    dz[-16:] += 1
    x[-16:] += 1
    assert M * dz.abs().max().item() * x.abs().max().item() < EXACT_BOUND
    return dz, x, _exact_product(dz, x), dz.double().sum(0), x.double().sum(0)


def _sides(shapes):
    return [(*s, side) for s in shapes for side in wide_plan.legal_sides(s[1], s[2])]


WGRAD_SHAPES = list(wide_plan.FULL_WGRAD) + [wide_plan.NEAR_FULL_WGRAD]


@pytest.mark.parametrize("M,N,K,bias_side", _sides(WGRAD_SHAPES))
def test_full_tile_weight_gradient_exact(M, N, K, bias_side, cuda_device):
    """dW and the column sums equal the integer product and sums, bit for bit, at every full-tile shape and at the one a
    chunk off (the general loop)."""
    dz, x, ref, csz, csx = _int_case(M, N, K, str(cuda_device))
    res = linear_wgrad_wide(dz, x, bias_side=bias_side)
    dw, cs = res if bias_side else (res, None)
    assert dw.shape == (N, K)
    assert torch.equal(dw.double(), ref), (dw.double() - ref).abs().max().item()
    if bias_side:
        want = csz if bias_side == 1 else csx
        assert torch.equal(cs.double(), want), (cs.double() - want).abs().max().item()


def _one_hot_cases():
    """(M, N, K, bias side, slice, chunk): every chunk of the one-slice rings (2, 4 and 6 chunks); the first, second,
    depth-th and last two chunks of the first and the last slice of a 16-chunk ring on the 256-row tiles, of the 4-chunk
    ring on the masked 64-row tiles and of an 8-chunk ring on the unmasked ones."""
    out = []
    for (M, N, K), side in (((32, 512, 512), 1), ((64, 512, 512), 1), ((96, 512, 512), 2), ((16384, 512, 512), 1),
                            ((1024, 48, 512), 2), ((32768, 64, 512), 2)):
        plan = wide_plan.wgrad_plan(M, N, K)
        assert plan.full
        last = plan.chunks - 1
        chunks = range(plan.chunks) if plan.S == 1 else sorted({0, 1, wide_plan.DEPTH, last - 1, last})
        out += [(M, N, K, side, s, c) for s in sorted({0, plan.S - 1}) for c in chunks]
    return out


@pytest.mark.parametrize("M,N,K,bias_side,s,c", _one_hot_cases())
def test_full_tile_weight_gradient_one_chunk(M, N, K, bias_side, s, c, cuda_device):
    """dz is 1 in the 16 rows of chunk c of slice s and 0 elsewhere: every row of dW is that chunk's column sums of x --
    a ring that drops the chunk gives 0, one that counts it twice the double, one that pairs it with another chunk's x
    that chunk's sums (the chunks differ; the last is offset by one)."""
    dev = str(cuda_device)
    plan = wide_plan.wgrad_plan(M, N, K)
    _, x, _, _, csx = _int_case(M, N, K, dev)
    r0 = s * plan.rows_per + 16 * c
    assert r0 + 16 <= M
    dz = torch.zeros(M, N, device=dev)
    dz[r0:r0 + 16] = 1.0
    want = x[r0:r0 + 16].double().sum(0)
    assert 16 * x.abs().max().item() < EXACT_BOUND and want.abs().max().item() > 0
    dw, cs = linear_wgrad_wide(dz, x, bias_side=bias_side)
    assert torch.equal(dw.double(), want.expand(N, K)), (s, c, (dw.double() - want).abs().max().item())
    assert torch.equal(cs.double(), torch.full((N,), 16.0, device=dev, dtype=torch.float64) if bias_side == 1 else csx)


def test_full_tile_weight_gradient_swapped_form_exact(cuda_device):
    """The default policy's first layer 48 -> 512 as _weight_grad runs it ("wide_first"): (x^T dz)^T on the masked
    64-row tiles with the bias from the 256-column side (wgrad_x6_wide_kernel<64, true, true, 2>)."""
    assert fused_mlp._wgrad_form(512, 48, True, True) == "wide_first"
    x, dz, ref_t, _, csz = _int_case(1024, 48, 512, str(cuda_device))  # the kernel's dz side is the layer's input
    dw, db = fused_mlp._weight_grad(dz, x, True, want_bias=True, wide=True)
    assert dw.shape == (512, 48) and dw.is_contiguous()
    assert torch.equal(dw.double(), ref_t.t())
    assert torch.equal(db.double(), csz)


@functools.lru_cache(maxsize=2)
def _float_case(M, N, K, dev):
    torch.manual_seed(M + N + K)
    dz = torch.randn(M, N, device=dev)
    x = F.elu(torch.randn(M, K, device=dev))
    ref = dz.double().t().mm(x.double())
    d = dz.t().mm(x).double() - ref
    return dz, x, ref, d.square().mean().sqrt().item()


@pytest.mark.parametrize("M,N,K,bias_side", _sides(WGRAD_SHAPES))
def test_full_tile_weight_gradient_float_rule(M, N, K, bias_side, cuda_device):
    """test_linear_wgrad's rule on random data: against fp64 the RMS error within 2x of torch fp32's, the max error
    within 1e-5 of max |ref|, the column sums within 2e-5; two calls bit-identical; in place in a larger buffer the 32
    floats on each side stay (test_wide_weight_gradient's guard)."""
    dev = str(cuda_device)
    dz, x, ref, rms32 = _float_case(M, N, K, dev)
    res = linear_wgrad_wide(dz, x, bias_side=bias_side)
    dw, cs = res if bias_side else (res, None)
    rms = (dw.double() - ref).square().mean().sqrt().item()
    print(f"wgrad {M}x{N}x{K} side {bias_side}: rms ours / fp32 {rms:.3e} {rms32:.3e}, "
          f"max err / max |ref| {(dw.double() - ref).abs().max().item() / ref.abs().max().item():.3e}")
    assert rms <= 2.0 * rms32 + 1e-12, (rms, rms32)
    _close(dw, ref.float(), 1e-5)
    if bias_side:
        _close(cs, (dz if bias_side == 1 else x).double().sum(0).float(), 2e-5)
    again = linear_wgrad_wide(dz, x, bias_side=bias_side)
    assert torch.equal(dw, again[0] if bias_side else again)
    if bias_side:
        assert torch.equal(cs, again[1])
        n = N * K + cs.numel()
        buf = torch.full((n + 64,), 7.5, device=dev)
        dw2, cs2 = linear_wgrad_wide(dz, x, bias_side=bias_side, dwb_out=buf[32:32 + n])
        assert dw2.data_ptr() == buf.data_ptr() + 4 * 32
        assert torch.equal(dw2, dw) and torch.equal(cs2, cs)
        assert torch.all(buf[:32] == 7.5) and torch.all(buf[32 + n:] == 7.5)
    else:
        buf = torch.full((N * K + 64,), 7.5, device=dev)
        dw2 = linear_wgrad_wide(dz, x, out=buf[32:32 + N * K].view(N, K))
        assert torch.equal(dw2, dw) and torch.all(buf[:32] == 7.5) and torch.all(buf[32 + N * K:] == 7.5)


@pytest.mark.parametrize("M,N,K,bias_side", [(*s, side) for s in wide_plan.FULL_DENSE_WGRAD
                                             for side in (0, 1, 2) if side != 1 or s[1] > 64])
def test_dense_full_tile_weight_gradient_exact(M, N, K, bias_side, cuda_device):
    """The dense unit (csrc/mlp_wgrad.hip) shares wgrad_x6_body; its full-tile branch (M a multiple of the slice's
    rows, an even chunk count, K = 256) was held to a tolerance at 393,216 rows only.  By the launch rule of
    rslrl_linear_wgrad_bias (wide_plan.dense_wgrad_plan): 1024 x 256 x 256 takes wgrad_x6_kernel<256, true, 3, false,
    CS>, 1024 x 128 x 256 the masked <256, true, 3, true, CS>, 1024 x 48 x 256 <64, true, 3, true, CS> (16 slices of 4
    chunks each) and 96 x 32 x 256 <32, true, 3, false, CS> (one slice of 6 chunks)."""
    assert wide_plan.dense_wgrad_plan(M, N, K).full
    dz, x, ref, csz, csx = _int_case(M, N, K, str(cuda_device))
    res = fused_mlp.linear_wgrad(dz, x, bias_side=bias_side)
    dw, cs = res if bias_side else (res, None)
    assert torch.equal(dw.double(), ref), (dw.double() - ref).abs().max().item()
    if bias_side:
        assert torch.equal(cs.double(), csz if bias_side == 1 else csx)


# ---- the wide GEMM's full tiles (M = 256: two row tiles, whole)

GM = 256


def _fwd_case(M, K, N, dev):
    torch.manual_seed(M + K + N)
    return (torch.randn(M, K, device=dev), torch.randn(N, K, device=dev) / K ** 0.5, torch.randn(N, device=dev))


def _dgrad_case(M, K, N, dev):
    """dz [M, K] through W [K, N] (the layer's weight: K outputs, N inputs), gated by h [M, N]."""
    torch.manual_seed(M + K + N + 1)
    return (torch.randn(M, K, device=dev), torch.randn(K, N, device=dev) / K ** 0.5,
            F.elu(torch.randn(M, N, device=dev)))


@pytest.mark.parametrize("K,N", wide_plan.FULL_GEMM_KN)
def test_wide_full_tiles_are_the_dense_kernels_bits(K, N, cuda_device):
    """test_wide_full_tiles_k256_are_the_dense_kernels_bits off the K = 256 loop: whole 128-row tiles on the plain
    chunk loop at K = 16 ... 1024, a last column block 4 wide under a row stride of 260, and (K <= 32) the input
    gradient's one-workgroup-per-CU form.  Every block against the tiled kernel on the dense block, bit for bit, and the
    whole against fp64."""
    plan = wide_plan.gemm_plan(GM, K, N, True)
    assert plan.full and not plan.deep
    x, w, b = _fwd_case(GM, K, N, cuda_device)
    dz, wt, h = _dgrad_case(GM, K, N, cuda_device)
    for elu in (True, False):
        y, _ = linear_fwd_ex(x, b, N, elu, bimage_wide(w, False), X6, wide=True)
        ref = F.linear(x.double(), w.double(), b.double())
        _close(y, (torch.where(ref > 0, ref, torch.expm1(ref)) if elu else ref).float())
        for c0 in range(0, N, 256):
            wb, bb = w[c0:c0 + 256].contiguous(), b[c0:c0 + 256].contiguous()
            dense, _ = linear_fwd_ex(x, bb, wb.shape[0], elu, bimage(wb, False), X6)
            assert torch.equal(y[:, c0:c0 + 256], dense), (elu, c0)
    out, db, _ = linear_dgrad_elu_ex(dz, h, bimage_wide(wt, True), X6, wide=True)
    d = dz.double().mm(wt.double())
    ref = torch.where(h > 0, d, d * (h.double() + 1))
    _close(out, ref.float())
    _close(db, ref.sum(0).float(), 1e-4)
    for c0 in range(0, N, 256):
        wb, hb = wt[:, c0:c0 + 256].contiguous(), h[:, c0:c0 + 256].contiguous()
        dense, dbb, _ = linear_dgrad_elu_ex(dz, hb, bimage(wb, True), X6)
        assert torch.equal(out[:, c0:c0 + 256], dense), c0
        assert torch.equal(db[c0:c0 + 256], dbb), c0


def _fwd_into(x, b, img, y):
    """linear_fwd_ex (no ELU) into the caller's y."""
    fused_mlp._gemm(_lib.LINEAR_FWD, X6, x, None, y.shape[1], img, wide=True, bias=b, c=y)


def _dgrad_into(dz, h, img, out, part):
    """linear_dgrad_elu_ex's launch into the caller's out and column-sum partials."""
    fused_mlp._gemm(_lib.LINEAR_DGRAD_ELU, X6, dz, None, h.shape[1], img, wide=True, h=h, c=out, colsum=part)


@pytest.mark.parametrize("K,N", wide_plan.FULL_GEMM_KN)
def test_wide_full_tiles_exact(K, N, cuda_device):
    """Integer x (|x| <= 4), W (|W| <= 2) and b: the forward without ELU equals the integer product; with h of 1.0 or
    -0.5 the ELU' gate is x1 or x0.5 exactly, so the input gradient and its column sums equal the half-integer
    reference.  At N = 260 also into a view inside a sentinel-filled buffer: the floats around it stay."""
    dev = cuda_device
    gen = torch.Generator().manual_seed(7919 * K + N)
    assert GM * K * 4 * 2 < EXACT_BOUND
    x, w, b = _ints((GM, K), -4, 4, dev, gen), _ints((N, K), -2, 2, dev, gen), _ints((N,), -8, 8, dev, gen)
    ref = F.linear(x.double(), w.double(), b.double())
    img = bimage_wide(w, False)
    y, _ = linear_fwd_ex(x, b, N, False, img, X6, wide=True)
    assert torch.equal(y.double(), ref), (y.double() - ref).abs().max().item()

    dz, wt = _ints((GM, K), -4, 4, dev, gen), _ints((K, N), -2, 2, dev, gen)
    h = torch.where(torch.rand(GM, N, generator=gen) < 0.5, 1.0, -0.5).to(dev)
    d = dz.double().mm(wt.double())
    gref = torch.where(h > 0, d, d * 0.5)
    timg = bimage_wide(wt, True)
    out, db, _ = linear_dgrad_elu_ex(dz, h, timg, X6, wide=True)
    assert torch.equal(out.double(), gref), (out.double() - gref).abs().max().item()
    assert torch.equal(db.double(), gref.sum(0)), (db.double() - gref.sum(0)).abs().max().item()

    if N % 256:
        n, tiles = GM * N, _lib.lib().rslrl_linear_tiles(GM)
        buf = torch.full((n + 64,), 7.5, device=dev)
        _fwd_into(x, b, img, buf[32:32 + n].view(GM, N))
        assert torch.equal(buf[32:32 + n].view(GM, N), y)
        assert torch.all(buf[:32] == 7.5) and torch.all(buf[32 + n:] == 7.5)
        buf.fill_(7.5)
        pbuf = torch.full((tiles * N + 64,), 7.5, device=dev)
        _dgrad_into(dz, h, timg, buf[32:32 + n].view(GM, N), pbuf[32:32 + tiles * N])
        assert torch.equal(buf[32:32 + n].view(GM, N), out)
        assert torch.all(buf[:32] == 7.5) and torch.all(buf[32 + n:] == 7.5)
        assert torch.all(pbuf[:32] == 7.5) and torch.all(pbuf[32 + tiles * N:] == 7.5)
        assert torch.equal(pbuf[32:32 + tiles * N].view(tiles, N).double().sum(0), gref.sum(0))
