"""The stem and pre-activation kernels that were only ever reached from inside a built net, on their own C-ABI doors, at the
shapes the nets' test sizes never produce: stem_conv3x3s2_kernel (Xception block1_conv1, NCHW -> planes) at odd image
sides and pixel counts that are no multiple of 16 / 256; resnet_stem7x7 (8 x 32 output tiles) with ragged row and column
tiles and odd sides; maxpool3x3s2_bn_planes_kernel on odd maps (pad 1 / 1), with and without its second destination;
resnet_preconv at pixel counts below and across its 128-pixel tile.  References: float64 restatements (oracle.conv2d with
dtype=float64, oracle.max_pool_3x3_s2_same) and, where the kernel claims it, the bits of the generic layer path.
Largest distances measured on an MI355X, as fractions of each family's bar: stem_conv3x3s2 0.13 (of 1e-6 + 2^-20 of scale),
resnet_stem7x7 0.011 (of 3e-5; the bits of the generic path in every case), maxpool3x3s2_bn_planes 0.082 (of 2^-20, both
destinations), resnet_preconv 0.018 (of 3e-5; the bits of the layer path in every case)."""

import numpy as np
import pytest

from planes_util import planes_raw, planes_to_f32

pytestmark = pytest.mark.gpu
f32 = np.float32
POISON16, POISON_BYTE = 0xA5A5, 0xA5


def poisoned_planes(n_pix, ld):
    """(hi, lo) plane buffers of ceil(n_pix / 16) * 16 pixels, every byte 0xA5"""
    from xdet import ops
    from xdet._lib import lib, check
    from xdet.runtime import DeviceBuffer, synchronize
    bufs = []
    for _ in range(2):
        b = DeviceBuffer(ops.planes_bytes(n_pix, ld))
        check(lib().xdet_memset(b.ptr, POISON_BYTE, b.nbytes, None))
        bufs.append(b)
    synchronize()
    return tuple(bufs)


def f16x3_conv(*args, **kw):
    from xdet import ops
    from xdet.runtime import set_precision
    set_precision('f16x3')
    try:
        return ops.Conv2D(*args, **kw)
    finally:
        set_precision('f32')


@pytest.mark.parametrize('N', [1, 3])
@pytest.mark.parametrize('S', [64, 65, 67, 99, 130])
def test_stem_conv3x3s2_matches_float64(S, N, oracle):
    """Ho = 31, 32, 33, 49, 64: N * Ho * Ho = 961, 1089, 2401 (N = 1) and 2883, 3267, 7203 (N = 3) are no multiples of 16 (a
    partly written last pixel group) nor of 256 (a partly filled last workgroup), 3072 is one of 16 only, 1024, 4096 and 12288 of
    both.  Bar: tests/test_gpu_layers.py's test_depthwise_matches_oracle (1e-6 of scale: f32 FMA chains in a fixed order) plus
    2^-20 for hi + lo."""
    from xdet import ops
    rng = np.random.default_rng(S * 10 + N)
    x = rng.standard_normal((N, 3, S, S)).astype(f32)
    k = (rng.standard_normal((3, 3, 3, 32)) / np.sqrt(27)).astype(f32)
    scale = rng.uniform(0.5, 1.5, 32).astype(f32)
    shift = rng.standard_normal(32).astype(f32)
    Ho = (S - 3) // 2 + 1
    n_pix = N * Ho * Ho
    ref = oracle.conv2d(x.transpose(0, 2, 3, 1), k, 2, 'VALID', dtype=np.float64)
    ref = np.maximum(ref * scale.astype(np.float64) + shift.astype(np.float64), 0).reshape(n_pix, 32)
    hi, lo = ops.stem_conv3x3s2(x, k, scale, shift, out=poisoned_planes(n_pix, 32))
    got = planes_to_f32(hi, lo, n_pix, 32)
    sc = max(1.0, float(np.abs(ref).max()))
    bar = (1e-6 + 2.0 ** -20) * sc
    err = float(np.abs(got - ref).max())
    print('stem_conv3x3s2 S=%d N=%d (%d pixels): distance / bar = %.4f' % (S, N, n_pix, err / bar))
    assert err <= bar, (err, bar)
    # pixels past N * Ho * Ho of the last 16-pixel group are nobody's: still the poison
    for b in (hi, lo):
        assert (planes_raw(b, n_pix, 32)[n_pix:] == POISON16).all()


@pytest.mark.parametrize('N', [1, 3])
@pytest.mark.parametrize('S', [64, 75, 100, 131, 200])
def test_resnet_stem7x7_matches_generic_path_and_float64(S, N, oracle):
    """output sides 32, 38, 50, 66, 100: rows mod 8 in {0, 6, 2, 2, 4}, columns mod 32 in {0, 6, 18, 2, 4}, two odd image sides.
    csrc/resnet_stem.hip claims the bits of the generic small-cin kernel on an NHWC4 copy of the image."""
    from xdet import ops
    from xdet.runtime import DeviceTensor
    rng = np.random.default_rng(S * 10 + N)
    x = rng.standard_normal((N, 3, S, S)).astype(f32)
    k = (rng.standard_normal((7, 7, 3, 64)) / 12).astype(f32)
    scale = rng.uniform(0.5, 1.5, 64).astype(f32)
    shift = rng.standard_normal(64).astype(f32)
    conv = f16x3_conv(k, 2, 'EXPLICIT', scale=scale, shift=shift, explicit_pad=3)
    nhwc = np.ascontiguousarray(x.transpose(0, 2, 3, 1))
    generic = conv(DeviceTensor.from_numpy(nhwc)).numpy()
    got = ops.resnet_stem7x7(conv, x).numpy()
    Ho = (S - 1) // 2 + 1
    assert got.shape == generic.shape == (N, Ho, Ho, 64)
    assert np.array_equal(got.view(np.uint32), generic.view(np.uint32)), float(np.abs(got - generic).max())
    ref = oracle.conv2d(nhwc, k, 2, ((3, 3), (3, 3)), dtype=np.float64) * scale.astype(np.float64) + shift.astype(np.float64)
    sc = max(1.0, float(np.abs(ref).max()))
    err = float(np.abs(got - ref).max())
    print('resnet_stem7x7 S=%d N=%d: distance / bar = %.4f' % (S, N, err / (3e-5 * sc)))
    assert err <= 3e-5 * sc, (err, sc)


def test_resnet_stem7x7_refuses_what_it_cannot_run():
    """the kernel's epilogue has no ReLU and its filter layout is the f16x3 one: such layers are an error, not another kernel"""
    from xdet import ops
    from xdet._lib import InvalidArgumentError
    rng = np.random.default_rng(0)
    x = rng.standard_normal((1, 3, 64, 64)).astype(f32)
    k = (rng.standard_normal((7, 7, 3, 64)) / 12).astype(f32)
    for conv in (f16x3_conv(k, 2, 'EXPLICIT', relu=True, explicit_pad=3), f16x3_conv(k, 2, 'SAME'),
                 f16x3_conv(k[:5, :5], 2, 'EXPLICIT', explicit_pad=3), ops.Conv2D(k, 2, 'EXPLICIT', explicit_pad=3)):
        with pytest.raises(InvalidArgumentError):
            ops.resnet_stem7x7(conv, x)


@pytest.mark.parametrize('N', [1, 3])
@pytest.mark.parametrize('ld', [64, 96])
@pytest.mark.parametrize('H,W', [(48, 48), (37, 37), (7, 10), (9, 65), (50, 33)])
def test_maxpool3x3s2_bn_planes(H, W, ld, N, oracle):
    """TF SAME padding 0 / 1 on even sides, 1 / 1 on odd ones; Ho in {24, 19, 4, 5, 25} (bands of 8 rows: ragged but for 24),
    N * bands in {1, 3, 4, 9, 12} (the grid rounds them up to 8), Wo * ld / 4 in {384, 576, 304, 456, 80, 120, 528, 792, 272,
    408} (none a multiple of 256).  Power-of-two BN scales make numpy's x * s + h the kernel's one-rounding fma, so hi + lo
    is the float64 statement within the planes' 2^-20."""
    from xdet import ops
    from xdet.runtime import DeviceTensor
    rng = np.random.default_rng(H * 1000 + W * 10 + ld + N)
    x = rng.standard_normal((N, H, W, ld)).astype(f32)
    s = rng.choice(np.array([0.5, 1.0, 2.0], f32), ld)
    h = rng.uniform(-0.5, 0.5, ld).astype(f32)
    mul = 0.5
    Ho, Wo = -(-H // 2), -(-W // 2)
    n_pix = N * Ho * Wo
    want = np.maximum(oracle.max_pool_3x3_s2_same(x).astype(np.float64) * s + h, 0).reshape(n_pix, ld)
    sc = max(1.0, float(np.abs(want).max()))
    dx = DeviceTensor.from_numpy(x)
    hi, lo = ops.max_pool_3x3_s2_bn_planes(dx, s, h, mul, out=poisoned_planes(n_pix, ld))
    got = planes_to_f32(hi, lo, n_pix, ld)
    err = float(np.abs(got - want * mul).max())
    print('maxpool3x3s2_bn_planes %dx%d ld=%d N=%d: distance / bar = %.4f' % (H, W, ld, N, err / (2.0 ** -20 * sc)))
    assert err <= 2.0 ** -20 * sc, (err, sc)
    raw1 = [planes_raw(b, n_pix, ld) for b in (hi, lo)]
    for r in raw1:
        assert (r[n_pix:] == POISON16).all()
    # the second destination: channel blocks [2, 2 + ld / 32) of a planes tensor ld / 32 + 3 blocks wide, * mul / 4
    c32_2, first = ld // 32 + 3, 2
    wide = poisoned_planes(n_pix, c32_2 * 32)
    hi1, lo1 = ops.max_pool_3x3_s2_bn_planes(dx, s, h, mul, out=poisoned_planes(n_pix, ld),
                                             second=(wide[0].ptr + first * 1024, wide[1].ptr + first * 1024, c32_2, mul / 4))
    for b, r in zip((hi1, lo1), raw1):
        assert np.array_equal(planes_raw(b, n_pix, ld), r)                    # the first destination: the same bits
    wraw = [planes_raw(b, n_pix, c32_2 * 32) for b in wide]
    mine = slice(first * 32, first * 32 + ld)
    got2 = (wraw[0].view(np.float16).astype(f32) + wraw[1].view(np.float16).astype(f32))[:n_pix, mine]
    err2 = float(np.abs(got2 - want * (mul / 4)).max())
    print('  second destination: distance / bar = %.4f' % (err2 / (2.0 ** -20 * sc * 0.25)))
    assert err2 <= 2.0 ** -20 * sc * 0.25, (err2, sc)
    for r in wraw:
        assert (r[:, :first * 32] == POISON16).all() and (r[:, first * 32 + ld:] == POISON16).all()
        assert (r[n_pix:] == POISON16).all()


@pytest.mark.parametrize('N,H,W', [(1, 5, 7), (3, 10, 37), (2, 60, 60)])
@pytest.mark.parametrize('cin', [256, 512])
def test_resnet_preconv_matches_layer_path_and_float64(cin, N, H, W, oracle):
    """M = 35 (less than one 128-pixel tile, 3 pixels in the last group of 16), 1110 (a ragged ninth tile), 7200 (57 tiles
    over persistent workgroups).  csrc/resnet_preconv.hip claims the bits of bn_relu -> split -> the LDS-DMA conv -> split."""
    from xdet import ops
    from xdet._lib import lib, check
    from xdet.runtime import DeviceTensor, synchronize
    rng = np.random.default_rng(cin + N * 1000 + H * 10 + W)
    cmid = 128
    x = rng.standard_normal((N, H, W, cin)).astype(f32)
    ps = rng.choice(np.array([0.5, 1.0, 2.0], f32), cin)           # (numpy's x * s + h is then the kernel's fused multiply-add)
    ph = rng.uniform(-0.3, 0.3, cin).astype(f32)
    pre = np.maximum(x * ps + ph, 0).astype(f32)
    wa = (rng.standard_normal((1, 1, cin, cmid)) / np.sqrt(cin)).astype(f32)
    sa = rng.uniform(0.5, 1.5, cmid).astype(f32)
    ha = rng.uniform(-0.2, 0.2, cmid).astype(f32)
    A = f16x3_conv(wa, scale=sa, shift=ha, relu=True)
    n_pix = N * H * W
    y1 = A(DeviceTensor.from_numpy(pre), planes=True)
    rhi, rlo = poisoned_planes(n_pix, cmid)
    check(lib().xdet_split_f32(y1.ptr, rhi.ptr, rlo.ptr, n_pix, cmid, 0, None))
    synchronize()
    hi, lo = ops.resnet_preconv(A, ps, ph, DeviceTensor.from_numpy(x), out=poisoned_planes(n_pix, cmid))
    for got, want in ((hi, rhi), (lo, rlo)):
        g, w = planes_raw(got, n_pix, cmid), planes_raw(want, n_pix, cmid)
        assert np.array_equal(g[:n_pix], w[:n_pix]), int((g[:n_pix] != w[:n_pix]).sum())
        assert (g[n_pix:] == POISON16).all()
    ref = oracle.conv2d(pre, wa, dtype=np.float64) * sa.astype(np.float64) + ha.astype(np.float64)
    ref = np.maximum(ref, 0).reshape(n_pix, cmid)
    sc = max(1.0, float(np.abs(ref).max()))
    err = float(np.abs(planes_to_f32(hi, lo, n_pix, cmid) - ref).max())
    print('resnet_preconv cin=%d M=%d: distance / bar = %.4f' % (cin, n_pix, err / (3e-5 * sc)))
    assert err <= 3e-5 * sc, (err, sc)
