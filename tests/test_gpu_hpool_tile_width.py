"""The horizontally pooled form of the fused separable block (csrc/sepconv_fused.hip, HPOOL) computes 31 valid columns
per tile row -- 15 pooling windows, tiles 30 columns apart -- from a patch of 33 pixels per row: 32 from the LDS DMA
pieces and a 33rd that wave 0 fetches on its own into a pad of the patch row.  Every case compares, bit for bit,

    separable_block_then_pool_add(op, x, res)        (pooled epilogue + vertical pass)

with the whole pool behind a block that does NOT run the pooled kernel: the two-kernel depthwise -> pointwise block
(fused=False), and the one-kernel block in its unpooled form (fused=True).  Inputs are random normal, so a stale,
missing or misplaced 33rd column, a window stored from the wrong register or a tile at the wrong stride changes bits."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# (N, H, W, cin, cout, relu_in): the smallest shapes at which the 15-window geometry can go wrong
CASES = [
    (2, 5, 29, 32, 128, True),      # one tile, pad 1/1: window 14 ends on the pool's right pad, 33rd pixel outside the image (zero)
    (2, 5, 30, 32, 128, False),     # pad 0/1: window 14's last column is the pool's right pad
    (1, 4, 31, 64, 256, False),     # second tile with a single window; the 256-wide layout
    (2, 9, 59, 64, 128, True),      # exactly two tiles: the 33rd pixel of tile 0 is live image data
    (1, 5, 60, 32, 256, True),      # exactly two tiles, live 33rd pixel, the 256-wide layout
    (2, 4, 61, 32, 128, False),     # third tile with one window
    (1, 8, 119, 32, 128, True),     # the workload's width: 4 tiles per row
    (1, 4, 237, 32, 128, False),    # the workload's width: 8 tiles per row
    (1, 1, 91, 96, 128, True),      # single row, three chunks
    (1, 9, 61, 160, 128, True),     # five chunks: the three-slot ring wraps inside a tile
    (2, 80, 237, 32, 128, True),    # 320 tiles on at most 256 workgroups: some workgroups take a second tile
    (4, 80, 237, 64, 128, False),   # 640 tiles of two chunks: three tiles per workgroup, so the 33rd column of a NEW tile
                                    # is requested and stored from inside the step loop, into a reused ring slot
]


@pytest.mark.parametrize('case', CASES)
@pytest.mark.parametrize('prec', ['f16x3', 'f16'])
def test_pooled_block_with_15_window_tiles_equals_block_then_whole_pool(case, prec):
    from xdet.ops import SeparableConvBN, max_pool_3x3_s2_same_add, separable_block_then_pool_add
    from xdet.runtime import DeviceTensor, set_precision
    N, H, W, cin, cout, relu_in = case
    rng = np.random.default_rng(H * 13 + W + cin)
    x = rng.standard_normal((N, H, W, cin)).astype(np.float32)
    dk = rng.standard_normal((3, 3, cin, 1)).astype(np.float32) / 3
    pk = (rng.standard_normal((1, 1, cin, cout)) / np.sqrt(cin)).astype(np.float32)
    scale = rng.uniform(0.5, 1.5, cout).astype(np.float32)
    shift = rng.standard_normal(cout).astype(np.float32)
    res = rng.standard_normal((N, -(-H // 2), -(-W // 2), cout)).astype(np.float32)
    set_precision(prec)
    try:
        op = SeparableConvBN(dk, pk, scale, shift, relu=False)
    finally:
        set_precision('f32')
    xd, rd = DeviceTensor.from_numpy(x), DeviceTensor.from_numpy(res)
    ref = max_pool_3x3_s2_same_add(op(xd, relu_in=relu_in, fused=False), rd).numpy()
    assert ref.shape == res.shape and np.isfinite(ref).all()
    ref_fused = max_pool_3x3_s2_same_add(op(xd, relu_in=relu_in, fused=True), rd).numpy()
    assert np.array_equal(ref_fused, ref)
    split = separable_block_then_pool_add(op, xd, rd, relu_in=relu_in).numpy()
    assert split.shape == ref.shape
    bad = np.argwhere(split != ref)
    assert np.array_equal(split, ref), ('%d elements differ, first (n, y, x, c) = %s' % (len(bad), bad[:1].tolist()))
