"""Which kernel variant a wide launch takes, transcribed from csrc/mlp_wide.hip (wide_tn, wide_rows_per, the `full`
expression of rslrl_linear_wgrad_bias_wide, launch_wide) and, for the dense weight gradient, from csrc/mlp_wgrad.hip
(wgrad_slices, wgrad_rows_per, rslrl_linear_wgrad_bias).  tests/test_wide_host.py pins the mirror to the library through
the workspace size, the one place the library shows its slice count; the GPU tests of the full-tile variants
(tests/test_gpu_wide_full_tiles.py) take their shapes from FULL_WGRAD below, so a retune of the slice rule that moves
one of them off its variant fails a host test instead of silently leaving the variant unrun."""

from collections import namedtuple

MC = 16  # kMC: rows per chunk
TK = 256  # kTK: columns of x per block
# kWgradDepth (RSLRL_WGRAD_DEPTH): chunks of look-ahead of the full-tile loop.  The library does not export it; 2 is the
# shipped build's.  A build with depth 4 keeps this module's slice counts and workspace sizes, only `full` changes.
DEPTH = 2

WgradPlan = namedtuple("WgradPlan", "tn S rows_per chunks full maskn grid")
GemmPlan = namedtuple("GemmPlan", "full deep minw2 grid")


def _ceil_div(a, b):
    return -(-a // b)


def wgrad_plan(M, N, K, depth=DEPTH):
    """rslrl_linear_wgrad_bias_wide on dz [M, N], x [M, K]: tile rows, slices, rows and chunks per slice, whether the
    launch takes the look-ahead (FULL) variant, whether that one masks the dz side (MASKN), and the grid."""
    tn = 64 if N <= 64 else 256
    blocks = _ceil_div(N, tn) * _ceil_div(K, TK)
    chunks = _ceil_div(M, MC)
    slices = max(1, min((512 if tn == 64 else 256) // blocks, chunks // 4))
    rows_per = _ceil_div(_ceil_div(M, slices), MC) * MC
    S = _ceil_div(M, rows_per)
    full = M % rows_per == 0 and (rows_per // MC) % depth == 0 and K % TK == 0 and (tn == 64 or N % TK == 0)
    maskn = full and tn == 64 and N != tn
    return WgradPlan(tn, S, rows_per, rows_per // MC, full, maskn, (S, _ceil_div(N, tn), _ceil_div(K, TK)))


def dense_wgrad_plan(M, N, K, depth=DEPTH):
    """rslrl_linear_wgrad_bias (N, K <= 256) in the same terms; its full tiles need K == 256."""
    tn = 32 if N <= 32 else (64 if N <= 64 else 256)
    slices = max(1, min(512 if N <= 64 else 256, _ceil_div(M, MC) // 4))
    rows_per = _ceil_div(_ceil_div(M, slices), MC) * MC
    S = _ceil_div(M, rows_per)
    full = M % rows_per == 0 and K == TK and (rows_per // MC) % depth == 0
    return WgradPlan(tn, S, rows_per, rows_per // MC, full, full and N < tn, (S, 1, 1))


def wgrad_nke(N, K, bias_side):
    """Floats per slice of the partials: dW and the column sums of the bias side."""
    return N * K + (N if bias_side == 1 else (K if bias_side == 2 else 0))


def wgrad_side_ok(N, K, bias_side):
    """wgrad_shape_ok: both widths 4-aligned in [4, 1024]; the dz-side sums need the 256-row tiles."""
    side = lambda n: 4 <= n <= 1024 and n % 4 == 0  # noqa: E731
    return side(N) and side(K) and 0 <= bias_side <= 2 and not (bias_side == 1 and N <= 64)


def gemm_plan(M, K, N, grad):
    """rslrl_linear_gemm_wide on M rows, reduction depth K, N outputs; grad: RSLRL_LINEAR_DGRAD_ELU.  full: the FULL
    template variant (no row or K masks); deep: the unrolled look-ahead loop of K = 256; minw2: the one-workgroup-per-CU
    input gradient of a short reduction."""
    return GemmPlan(M % 128 == 0 and K % 16 == 0, K == 256, bool(grad) and K <= 32, (_ceil_div(M, 128), _ceil_div(N, 256)))


# (M, N, K): (tn, S, chunks, maskn) at depth 2 -- the full-tile weight-gradient shapes of the GPU tests
FULL_WGRAD = {
    (32, 512, 512): (256, 1, 2, False),  # smallest ring: main loop skipped; prologue, one step, tail
    (64, 512, 512): (256, 1, 4, False),  # one pass of the main loop; also full at depth 4
    (96, 512, 512): (256, 1, 6, False),  # full at depth 2 only
    (1024, 512, 512): (256, 16, 4, False),  # many slices, 2 x 2 blocks
    (16384, 512, 512): (256, 64, 16, False),  # slice count at its cap, long ring
    (4096, 256, 512): (256, 64, 4, False),  # [512, 256, 128]'s second layer: one N block, two K blocks
    (1024, 512, 768): (256, 16, 4, False),  # 2 x 3 blocks
    (2048, 1024, 1024): (256, 16, 8, False),  # widest, 4 x 4 blocks
    (1024, 64, 512): (64, 16, 4, False),  # TN = 64, no mask
    (1024, 48, 512): (64, 16, 4, True),  # TN = 64, MASKN: the default first layer in swapped form
    (1024, 4, 1024): (64, 16, 4, True),  # MASKN at its narrowest
}
# one chunk off a full tile (14 slices of 5 chunks): the general branch, which must agree
NEAR_FULL_WGRAD = (1056, 512, 512)
# tests/test_gpu_wide_mlp.py test_wide_weight_gradient and its swapped form (as called: x, dz): none is full
GENERAL_WGRAD = [(200, 320, 16), (3001, 260, 320), (3001, 512, 512), (3001, 48, 512)]
# the dense unit's full-tile variants (shared body): (M, N, K): (tn, S, chunks, maskn)
FULL_DENSE_WGRAD = {
    (1024, 256, 256): (256, 16, 4, False),  # wgrad_x6_kernel<256, true, 3, false, CS>
    (1024, 128, 256): (256, 16, 4, True),  # <256, true, 3, true, CS>: masked dz side on the 256-row tiles
    (1024, 48, 256): (64, 16, 4, True),  # <64, true, 3, true, CS>
    (96, 32, 256): (32, 1, 6, False),  # <32, true, 3, false, CS>: one slice, main loop twice
}


# (K, N) of the wide GEMM's full tiles at M = 256: a short first-layer reduction, a ragged last column block (row stride
# 260 against a block 4 wide), 4 blocks, 64 chunks, and the two short reductions of the MINW = 2 input gradient
FULL_GEMM_KN = [(48, 512), (512, 260), (512, 1024), (1024, 512), (16, 512), (32, 260)]


def legal_sides(N, K):
    return [s for s in (0, 1, 2) if wgrad_side_ok(N, K, s)]
