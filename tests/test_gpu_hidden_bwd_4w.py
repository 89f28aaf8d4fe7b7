"""The 4-wave form of the fused hidden-layer backward (csrc/mlp_bwd_fused.hip, hidden_bwd4_kernel: one wave per SIMD,
the slice's dW in the accumulator registers: the default) against the 8-wave kernel it replaced (RSLRL_HB_VARIANT=8w): every
output element gets the same MFMAs in the same order and db folds the same eight sums in the same order, so dZp, dW and
db must be the same bits.  Row counts: 64 (one tile: the prologue only), 8,256 (129 tiles: 64 slices of 2 and a ragged
last one of 1 -- the next-tile loads and the exit without a next tile), 24,576 (3 tiles per slice: an odd count through
the alternating buffers), 49,216 (769 tiles: 7 per slice and a short last slice)."""

import pytest
import torch

from rsl_rl_amd.networks import fused_mlp

pytestmark = pytest.mark.gpu
W = 256
ROWS = [64, 8256, 24576, 49216]


def _problem(M, dev, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    dz = torch.randn(M, W, device=dev, generator=g) * 0.01
    h = torch.nn.functional.elu(torch.randn(M, W, device=dev, generator=g))
    w = torch.randn(W, W, device=dev, generator=g) / 16
    return dz, h, w


def _run(monkeypatch, variant, dzs, hs, imgs):
    monkeypatch.setenv("RSLRL_HB_VARIANT", variant)
    out = fused_mlp.hidden_bwd_pair(dzs, hs, imgs)
    torch.cuda.synchronize()
    return [[x.clone() for x in o] for o in out]


def _same(a, b):
    for pa, pb in zip(a, b):
        for name, u, v in zip(("dzp", "dw", "db"), pa, pb):
            assert torch.equal(u, v), (name, float((u - v).abs().max()))


@pytest.mark.parametrize("n", [2, 1])
@pytest.mark.parametrize("M", ROWS)
def test_4wave_matches_8wave_bits(M, n, cuda_device, monkeypatch):
    p = [_problem(M, cuda_device, 21 + M + i) for i in range(n)]
    dzs, hs = [q[0] for q in p], [q[1] for q in p]
    imgs = fused_mlp.bimages([(q[2], True) for q in p])
    assert fused_mlp.hidden_bwd_ok(dzs, hs)
    ref = _run(monkeypatch, "8w", dzs, hs, imgs)
    got = _run(monkeypatch, "4w", dzs, hs, imgs)
    assert float(ref[0][1].abs().max()) > 0  # the reference ran
    _same(got, ref)
    # a second launch gives the same bits
    _same(_run(monkeypatch, "4w", dzs, hs, imgs), got)
