"""The fused backward of the 512 -> 256 layer of a wide stack (rslrl_hidden_bwd_pair_wk, csrc/mlp_bwd_fused_wk.hip: the
input gradient and the weight + bias gradients of Linear(512, 256) + ELU from one pass over dz and h).  Reference
arithmetic: the autograd backward of rsl_rl/networks/mlp.py:106-114's layers (ppo.py:367), in fp64.

* Exact inputs: dz integers in -3 .. 3, W = randperm(256 * 512) % 16384 - 8192 (131,072 distinct values would break
  3 max(|dz| |W|) < 2^24), h from {-0.5, -0.25, 0, 1, 2, 3}.  Every x6 plane product and every partial sum is then
  exact in fp32 (the reference builder checks the ranges), so dz_prev, dW and db must EQUAL the fp64 reference, at every
  branch point of the slice rule.
* Random inputs: dz_prev bit-equal to linear_dgrad_elu_ex(wide=True), a second launch bit-equal, [dW | db] against fp64
  relative to the error of linear_wgrad_wide(bias_side=1).  Measured ratios: DESIGN.md section 33.
* Declines launch nothing."""

import ctypes
import functools

import pytest
import torch

from rsl_rl_amd import _lib
from rsl_rl_amd.networks import fused_mlp

pytestmark = pytest.mark.gpu
K, N = 512, 256
BAND = 64
ERR_RATIO_BOUND = 3.0  # tests/test_gpu_hidden_bwd.py's bound for the 256 kernel: not fitted to this one


@functools.lru_cache(maxsize=None)
def _exact(M, seed):
    """(dz, h, w) on the CPU and the fp64 (dz_prev, dw, db), with the ranges that keep fp32 exact checked."""
    g = torch.Generator().manual_seed(seed)
    dz = torch.randint(-3, 4, (M, N), generator=g).float()
    h = torch.tensor([-0.5, -0.25, 0.0, 1.0, 2.0, 3.0])[torch.randint(0, 6, (M, K), generator=g)]
    w = (torch.randperm(N * K, generator=g) % 16384 - 8192).float().view(N, K)
    pre = dz.double() @ w.double()
    dzp = pre * torch.where(h > 0, 1.0, h.double() + 1.0)
    dw, db = dz.double().t() @ h.double(), dz.double().sum(0)
    # integers below 2^24 / 3 before ELU' in {1, 1/2, 3/4}; multiples of 1/4 below 2^22; integers below 2^24
    assert 3 * float((dz.double().abs() @ w.double().abs()).max()) < 2 ** 24
    assert 4 * float((dz.double().abs().t() @ h.double().abs()).max()) < 2 ** 24 and float(dz.abs().sum(0).max()) < 2 ** 24
    return dz, h, w, dzp, dw, db


def _guarded(n, dev):
    buf = torch.full((n + 2 * BAND,), float("nan"), device=dev)
    return buf, buf[BAND:BAND + n]


def _stream(dev):
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


# the slice rule's branch points: one tile; one slice of two tiles; two slices, the last one shorter; many slices; the
# slice cap with two tiles each; past the cap (three tiles per slice, the last slice two: its group of 8 is not full)
@pytest.mark.parametrize("n", [1, 2])
@pytest.mark.parametrize("M, slices", [(64, 1), (128, 1), (192, 2), (4096, 32), (16384, 128), (16448, 86)])
def test_exact_inputs_equal_fp64(M, slices, n, cuda_device):
    dev = cuda_device
    L = _lib.lib()
    assert L.rslrl_hidden_bwd_slices_wk(M, K, N) == slices
    NK = L.rslrl_hidden_bwd_partial_floats_wk(K, N)
    assert NK == N * K + N
    keep, probs, bufs, refs = [], [], [], []
    for i in range(n):
        dz, h, w, *ref = _exact(M, 5 + i)
        dz, h, w = dz.to(dev), h.to(dev), w.to(dev)
        img = fused_mlp.bimage_wide(w, True)
        out, part = _guarded(M * K, dev), _guarded(slices * NK, dev)
        probs.append(_lib.HiddenBwdProblem(dz.data_ptr(), h.data_ptr(), img.data_ptr(), out[1].data_ptr(),
                                           part[1].data_ptr()))
        keep.append((dz, h, w, img))
        bufs.append((out, part))
        refs.append(ref)
    rc = L.rslrl_hidden_bwd_pair_wk(ctypes.byref(probs[0]), ctypes.byref(probs[1]) if n == 2 else None, M, K, N,
                                    _stream(dev))
    assert rc == 0
    folds = fused_mlp._FoldBatch()
    dwbs = [torch.empty(NK, device=dev) for _ in range(n)]
    for (out, part), dwb in zip(bufs, dwbs):
        folds.add(part[1], slices, NK, dwb, NK)
    folds.run(dev)
    torch.cuda.synchronize()
    for i, ((out, part), dwb, (dzp, dw, db)) in enumerate(zip(bufs, dwbs, refs)):
        for buf, _ in (out, part):
            assert bool(torch.isnan(buf[:BAND]).all()) and bool(torch.isnan(buf[-BAND:]).all()), i
        assert not bool(torch.isnan(part[1]).any()), i  # every float of every partial row is written
        assert torch.equal(out[1].view(M, K).cpu().double(), dzp), i
        assert torch.equal(dwb[:N * K].view(N, K).cpu().double(), dw), i
        assert torch.equal(dwb[N * K:].cpu().double(), db), i


def _problem(M, dev, seed):  # tests/test_gpu_hidden_bwd.py's distributions at this shape
    g = torch.Generator(device=dev).manual_seed(seed)
    dz = torch.randn(M, N, device=dev, generator=g) * 0.01
    h = torch.nn.functional.elu(torch.randn(M, K, device=dev, generator=g))
    w = torch.randn(N, K, device=dev, generator=g) / 16
    return dz, h, w


@pytest.mark.parametrize("n", [1, 2])
@pytest.mark.parametrize("M", [64, 4096, 24576])
def test_random_inputs(M, n, cuda_device):
    dev = cuda_device
    p = [_problem(M, dev, 11 + M + i) for i in range(n)]
    dzs, hs = [q[0] for q in p], [q[1] for q in p]
    imgs = [fused_mlp.bimage_wide(q[2], True) for q in p]
    assert fused_mlp.hidden_bwd_wk_ok(dzs, hs) and not fused_mlp.hidden_bwd_kn_ok(dzs, hs)
    got = fused_mlp.hidden_bwd_pair_wk(dzs, hs, imgs)
    again = fused_mlp.hidden_bwd_pair_wk(dzs, hs, imgs)
    torch.cuda.synchronize()
    for i in range(n):
        dzp, dw, db = got[i]
        ref_dz = fused_mlp.linear_dgrad_elu_ex(dzs[i], hs[i], imgs[i], _lib.ARITH_X6, want_db=False, wide=True)[0]
        assert torch.equal(dzp, ref_dz), i  # the same products in the same order: the same bits
        for u, v in zip(got[i], again[i]):
            assert torch.equal(u, v)  # deterministic
        sep_dw, sep_db = fused_mlp.linear_wgrad_wide(dzs[i], hs[i], bias_side=1)
        dw64 = dzs[i].double().t() @ hs[i].double()
        db64 = dzs[i].double().sum(0)
        for name, a, b, ref in (("dw", dw, sep_dw, dw64), ("db", db, sep_db, db64)):
            err = float((a.double() - ref).abs().max())
            err_sep = float((b.double() - ref).abs().max())
            print(f"hidden_bwd_wk M={M} n={n} problem {i} {name}: err {err:.3e} separate {err_sep:.3e} "
                  f"ratio {err / max(err_sep, 1e-300):.3f}")
            assert err <= ERR_RATIO_BOUND * err_sep + 1e-12 * float(ref.abs().max()), (name, err, err_sep)


def test_declines_launch_nothing(cuda_device):
    dev = cuda_device
    L = _lib.lib()
    M = 1024
    dz, h, w = _problem(M, dev, 3)
    img = fused_mlp.bimage_wide(w, True)
    out = torch.full((M * K + 4,), float("nan"), device=dev)
    part = torch.full((L.rslrl_hidden_bwd_slices_wk(M, K, N) * (N * K + N),), float("nan"), device=dev)

    def run(rows, k, n, out_ptr):
        prob = _lib.HiddenBwdProblem(dz.data_ptr(), h.data_ptr(), img.data_ptr(), out_ptr, part.data_ptr())
        return L.rslrl_hidden_bwd_pair_wk(ctypes.byref(prob), None, rows, k, n, _stream(dev))

    for k, n in ((256, 128), (256, 256), (512, 128), (1024, 256)):
        assert run(M, k, n, out.data_ptr()) == -1  # RSLRL_E_INVALID_ARGUMENT
        assert L.rslrl_hidden_bwd_slices_wk(M, k, n) == 0 and L.rslrl_hidden_bwd_partial_floats_wk(k, n) == 0
    assert run(1000, K, N, out.data_ptr()) == -3  # RSLRL_E_UNSUPPORTED
    assert run(M, K, N, out.data_ptr() + 4) == -4  # RSLRL_E_MISALIGNED
    assert not fused_mlp.hidden_bwd_wk_ok([dz[:1000]], [h[:1000]])
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()) and bool(torch.isnan(part).all())
