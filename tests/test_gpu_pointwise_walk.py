"""The tile walk of the 256 x 256 LDS-DMA kernels (csrc/conv_mfma_dma.hip, WALK): a grid of more than one round of tiles is
launched as one workgroup per compute unit, each walking the virtual blocks vb = blockIdx.x + i * gridDim.x with the next
tile's first operand stage requested under the epilogue of the current one.  K order, product order and epilogue are the
one-tile-per-workgroup kernel's, so an image's rows must be, bit for bit, what the small-batch kernels (deep ring, 128-wide
tiles -- untouched by the walk) give the same image in a batch of 1 - 3, as in
tests/test_gpu_layers.py::test_large_batch_pointwise_gemm_is_the_same_function; the first two images are also held
against a float64 statement with that test's bar, 3e-5 of max(1, |ref|max).

All conv cases are 80 images of 30 x 30: 72,000 rows = 281.25 M tiles, a ragged last tile.  What a case exercises:
  32 -> 256            one K step, one N tile.  282 tiles are NOT a grid the launch rule gives the 256 x 256 tile (it wants
                       >= 512 tiles, whole rounds of 256, or >= 200 tiles with >= 40 K steps), so this shape runs on
                       128 x 128 tiles and never walks: it is kept as a statement about the rule's other side, and
  32 -> 512            is its walking twin: one K step (the prefetch is issued in the tile's only step), 564 tiles;
  64 -> 728            two K steps, the output planes emitted as well, the dead 32-column block of the third N tile;
  96 -> 728            three K steps (odd: the last stage read is stage 0, the one the prefetch overwrites), residual and ReLU;
  64 -> 512, 3x3 SAME  the multi-tap buffer form (GBUF): per-tile window descriptors and tap counters restart.
`launch_form` restates the launcher's rule (launch_conv_mfma_dma / launch_d) and every walking case asserts that its
large batch takes the 256 x 256 tile on more virtual blocks than any gfx9 part has compute units (304), and that its
sub-batches do not take that tile -- so that a case cannot silently compare the old path with itself.
The grouped cases (SpectralConv, F = 30, 64 -> 256): 64 images (22 bins x 8 M tiles x 2 = 352 tiles, the last tile of a bin
half padding; by the same rule 128-wide tiles, no walk) and 98 images (22 bins of 3,072 rows, 2,940 live, 528 tiles: the
walk, with the per-tile weight matrix and scale / shift rows, the two all-padding groups 22 and 23 skipped)."""
import numpy as np
import pytest

from planes_util import planes_rows

pytestmark = pytest.mark.gpu

f32 = np.float32
N_IMG, S = 80, 30
SUBS = ((0, 1), (N_IMG // 2, 3), (N_IMG - 2, 2))           # (first image, images): the ragged last M tile is in the last one
MAX_CUS = 304


def _cdiv(a, b):
    return -(-a // b)


def launch_form(M, cout, kp, group_rows=0):
    """the rule of launch_conv_mfma_dma for an f16x3 layer on the planes path: -> virtual blocks of the 256 x 256 grid when
    the layer takes that tile, else 0"""
    n_tile = 64 if _cdiv(cout, 64) * 64 < _cdiv(cout, 128) * 128 else 128
    cout_pad = _cdiv(cout, n_tile) * n_tile
    if n_tile != 128 or cout_pad % 256 or (group_rows and group_rows % 256):
        return 0
    b256, nk = _cdiv(M, 256) * (cout_pad // 256), kp // 32
    full_rounds = b256 >= 240 and (b256 % 256 == 0 or b256 % 256 >= 240)
    if not (b256 >= 512 or full_rounds or (b256 >= 200 and nk >= 40)):
        return 0
    if group_rows:
        return _cdiv(M // group_rows, 8) * 8 * (group_rows // 256) * (cout_pad // 256)
    return _cdiv(_cdiv(M, 256), 8) * 8 * (cout_pad // 256)


def _assert_walks(cin, cout, taps, walks):
    kp = taps * _cdiv(cin, 32) * 32
    nvb = launch_form(N_IMG * S * S, cout, kp)
    assert (nvb > MAX_CUS) == walks, (cin, cout, nvb)
    for _, n in SUBS:
        assert launch_form(n * S * S, cout, kp) == 0, (cin, cout, n)


# cin, cout, taps per side, residual, relu, planes out, walks
CONV_CASES = {
    '32_256': (32, 256, 1, False, False, False, False),
    '32_512': (32, 512, 1, False, True, False, True),
    '64_728_planes': (64, 728, 1, False, False, True, True),
    '96_728_res_relu': (96, 728, 1, True, True, False, True),
    '64_512_3x3': (64, 512, 3, False, True, False, True),
}


@pytest.mark.parametrize('name', sorted(CONV_CASES))
def test_walked_tiles_are_the_small_batch_kernels_bits(name, oracle):
    from xdet._lib import lib, check
    from xdet.ops import Conv2D
    from xdet.runtime import DeviceBuffer, DeviceTensor, set_precision, synchronize, to_host
    cin, cout, t, with_res, relu, planes_out, walks = CONV_CASES[name]
    _assert_walks(cin, cout, t * t, walks)
    rng = np.random.default_rng(23)
    x = rng.standard_normal((N_IMG, S, S, cin)).astype(f32)
    k = (rng.standard_normal((t, t, cin, cout)) / np.sqrt(t * t * cin)).astype(f32)
    sc = rng.uniform(0.5, 1.5, cout).astype(f32)
    sh = rng.standard_normal(cout).astype(f32)
    res = rng.standard_normal((N_IMG, S, S, cout)).astype(f32) if with_res else None
    ld = _cdiv(cout, 32) * 32

    def run(conv, n0, n):
        """-> out [n, S, S, cout] and, with planes_out, the (hi, lo) planes as uint16 rows [n * S * S][ld]"""
        xs = DeviceTensor.from_numpy(x[n0:n0 + n])
        r = DeviceTensor.from_numpy(res[n0:n0 + n]) if with_res else None
        if not planes_out:
            return conv(xs, residual=r, planes=True).numpy(), None
        M = n * S * S
        Mp = _cdiv(M, 16) * 16
        ih, il = DeviceBuffer(Mp * xs.ld * 2 + 512, zero=True), DeviceBuffer(Mp * xs.ld * 2 + 512, zero=True)
        check(lib().xdet_split_f32(xs.ptr, ih.ptr, il.ptr, M, xs.ld, 0, None))
        synchronize()
        out = DeviceTensor.empty((n, S, S, cout))
        oh, ol = DeviceBuffer(Mp * ld * 2 + 512, zero=True), DeviceBuffer(Mp * ld * 2 + 512, zero=True)
        conv.emit(in_planes=(ih, il), shape=(n, S, S), residual=r, out=out, out_planes=(oh, ol), planes_relu=True)
        pl = [planes_rows(to_host(b.ptr, (Mp * ld,), np.uint16), M, ld)[:M] for b in (oh, ol)]
        return out.numpy(), pl

    set_precision('f16x3')
    try:
        conv = Conv2D(k, 1, 'SAME', 1, sc, sh, relu=relu)
        big, big_pl = run(conv, 0, N_IMG)
        for n0, n in SUBS:
            small, small_pl = run(conv, n0, n)
            assert np.array_equal(small.view(np.uint32), big[n0:n0 + n].view(np.uint32)), (name, n0, n)
            if planes_out:
                for a, b in zip(small_pl, big_pl):
                    assert np.array_equal(a, b[n0 * S * S:(n0 + n) * S * S]), (name, 'planes', n0, n)
    finally:
        set_precision('f32')
    if t == 1:
        ref = x[:2].reshape(-1, cin).astype(np.float64) @ k.reshape(cin, cout).astype(np.float64)
    else:
        ref = oracle.conv2d(x[:2], k, 1, 'SAME', 1, dtype=np.float64).reshape(-1, cout)
    ref = ref * sc + sh
    if with_res:
        ref = ref + res[:2].reshape(-1, cout)
    if relu:
        ref = np.maximum(ref, 0)
    err, bar = np.abs(big[:2].reshape(-1, cout) - ref).max(), 3e-5 * max(1.0, np.abs(ref).max())
    print('%s: err %.3g bar %.3g' % (name, err, bar))
    assert err < bar, (name, err, bar)


@pytest.mark.parametrize('n_img,walks', [(64, False), (98, True)])
def test_grouped_walk_gives_every_image_the_bits_of_a_batch_of_two(n_img, walks):
    from xdet import ops
    from xdet.runtime import DeviceTensor, set_precision
    F, cin, cout, T = 30, 64, 256, 15
    # the bins' GEMM: 22 groups of m_pad rows, K = 2 * cin (re | im), N = 2 * cout
    m_pad = 128 if n_img * F <= 128 else _cdiv(n_img * F, 256) * 256
    nvb = launch_form(22 * m_pad, 2 * cout, 2 * cin, group_rows=m_pad)
    assert (nvb > MAX_CUS) == walks, nvb
    assert launch_form(22 * 128, 2 * cout, 2 * cin, group_rows=128) == 0
    rng = np.random.default_rng(29)
    x = rng.standard_normal((n_img, F, F, cin)).astype(f32)
    w = (rng.standard_normal((T, cin, cout)) / np.sqrt(T * cin)).astype(f32)
    sc = rng.uniform(0.5, 1.5, cout).astype(f32)
    sh = rng.standard_normal(cout).astype(f32)
    set_precision('f16x3')
    try:
        layer = ops.SpectralConv(w, 0, F, sc, sh, relu=True)
        big = layer(DeviceTensor.from_numpy(x)).numpy()
        for n0 in (0, n_img // 2 - 1, n_img - 2):
            small = layer(DeviceTensor.from_numpy(x[n0:n0 + 2])).numpy()
            assert np.array_equal(small.view(np.uint32), big[n0:n0 + 2].view(np.uint32)), n0
    finally:
        set_precision('f32')
