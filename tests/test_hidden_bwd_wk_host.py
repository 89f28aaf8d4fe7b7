"""The slice rule of the 512 -> 256 fused hidden-layer backward (rslrl_hidden_bwd_slices_wk, csrc/mlp_bwd_fused_wk.hip):
a slice runs max(2, ceil(tiles / 128)) tiles of 64 rows as two workgroups, so one problem gives the 256 CUs at most one
workgroup each; and fused_mlp.hidden_bwd_wk_ok on CPU tensors.  Host code only."""

import pytest
import torch

from rsl_rl_amd import _lib
from rsl_rl_amd.networks import fused_mlp


@pytest.mark.parametrize("M, slices", [(64, 1), (128, 1), (192, 2), (4096, 32), (16320, 128), (16384, 128),
                                       (16448, 86), (24576, 128), (393216, 128), (64 * 3_000_001, 128)])
def test_slice_rule(M, slices):
    L = _lib.lib()
    tiles = M // 64
    per = max(2, -(-tiles // 128))
    S = L.rslrl_hidden_bwd_slices_wk(M, 512, 256)
    assert S == slices == -(-tiles // per)
    assert (S - 1) * per < tiles <= S * per  # every slice has a tile; the last one may be shorter


def test_sizes_and_declines():
    L = _lib.lib()
    assert L.rslrl_hidden_bwd_partial_floats_wk(512, 256) == 256 * 512 + 256
    for M, K, N in ((0, 512, 256), (63, 512, 256), (1000, 512, 256), (-64, 512, 256), (4096, 256, 128),
                    (4096, 256, 256), (4096, 512, 128), (4096, 1024, 256), (4096, 256, 512)):
        assert L.rslrl_hidden_bwd_slices_wk(M, K, N) == 0
    for K, N in ((256, 128), (256, 256), (512, 128), (1024, 256)):
        assert L.rslrl_hidden_bwd_partial_floats_wk(K, N) == 0


def test_hidden_bwd_wk_ok_on_cpu_tensors():
    dz, h = torch.zeros(128, 256), torch.zeros(128, 512)
    assert fused_mlp.hidden_bwd_wk_ok([dz], [h]) and fused_mlp.hidden_bwd_wk_ok([dz, dz], [h, h])
    assert not fused_mlp.hidden_bwd_wk_ok([torch.zeros(128, 128)], [h])  # a 256 -> 128 layer's dz
    assert not fused_mlp.hidden_bwd_wk_ok([dz], [torch.zeros(128, 256)])  # a square layer's h
    assert not fused_mlp.hidden_bwd_wk_ok([torch.zeros(1000, 256)], [torch.zeros(1000, 512)])
    assert not fused_mlp.hidden_bwd_wk_ok([dz], [torch.zeros(128, 1024)[:, ::2]])  # not contiguous
