"""The slice rule of the 128-wide fused hidden-layer backward (rslrl_hidden_bwd_slices_n, csrc/mlp_bwd_fused_n.hip): a
slice runs max(2, ceil(tiles / 256)) tiles of 64 rows, so a pair of problems gives the 256 CUs at most two workgroups
each.  Host code only."""

import pytest

from rsl_rl_amd import _lib


@pytest.mark.parametrize("M", [64, 128, 192, 4096, 24576, 32704, 32768, 32832, 393216, 64 * 3_000_001])
def test_slice_rule(M):
    L = _lib.lib()
    tiles = M // 64
    per = max(2, -(-tiles // 256))
    S = L.rslrl_hidden_bwd_slices_n(M, 128)
    assert S == -(-tiles // per) and 1 <= S <= 256
    assert (S - 1) * per < tiles <= S * per  # every slice has a tile; the last one may be shorter


def test_slice_rule_real_updates_and_declines():
    L = _lib.lib()
    assert L.rslrl_hidden_bwd_slices_n(24576, 128) == 192  # 384 tiles, 2 per slice: 384 workgroups for a pair
    assert L.rslrl_hidden_bwd_slices_n(393216, 128) == 256  # 6,144 tiles, 24 per slice
    assert L.rslrl_hidden_bwd_partial_floats_n(128) == 128 * 128 + 128
    for M, width in ((0, 128), (63, 128), (1000, 128), (-64, 128), (4096, 256), (4096, 64), (4096, 192)):
        assert L.rslrl_hidden_bwd_slices_n(M, width) == 0
    assert L.rslrl_hidden_bwd_partial_floats_n(256) == 0
