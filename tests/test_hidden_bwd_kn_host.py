"""The slice rule of the 256 -> 128 fused hidden-layer backward (rslrl_hidden_bwd_slices_kn, csrc/mlp_bwd_fused_kn.hip):
a slice runs max(2, ceil(tiles / 128)) tiles of 64 rows as two workgroups, so a pair of problems gives the 256 CUs at
most two workgroups each.  Host code only."""

import pytest

from rsl_rl_amd import _lib


@pytest.mark.parametrize("M", [64, 128, 192, 4096, 16320, 16384, 16448, 24576, 393216, 64 * 3_000_001])
def test_slice_rule(M):
    L = _lib.lib()
    tiles = M // 64
    per = max(2, -(-tiles // 128))
    S = L.rslrl_hidden_bwd_slices_kn(M, 256, 128)
    assert S == -(-tiles // per) and 1 <= S <= 128
    assert (S - 1) * per < tiles <= S * per  # every slice has a tile; the last one may be shorter


def test_slice_rule_real_updates_and_declines():
    L = _lib.lib()
    assert L.rslrl_hidden_bwd_slices_kn(24576, 256, 128) == 128  # 384 tiles, 3 per slice
    assert L.rslrl_hidden_bwd_slices_kn(393216, 256, 128) == 128  # 6,144 tiles, 48 per slice
    assert L.rslrl_hidden_bwd_partial_floats_kn(256, 128) == 128 * 256 + 128
    for M, K, N in ((0, 256, 128), (63, 256, 128), (1000, 256, 128), (-64, 256, 128), (4096, 128, 256),
                    (4096, 256, 256), (4096, 128, 128), (4096, 256, 64)):
        assert L.rslrl_hidden_bwd_slices_kn(M, K, N) == 0
    assert L.rslrl_hidden_bwd_partial_floats_kn(128, 256) == 0
