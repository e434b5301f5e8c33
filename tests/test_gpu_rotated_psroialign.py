"""RotatedPsRoiAlign on the GPU: the reference's known answers and fixture (bit for bit in the forward, to rounding
in the gradient), random sweeps against the NumPy restatement, both layouts, no index output, a guard band around
the map, and two streams at once."""
import numpy as np
import pytest

import rotated_psroi_ref as RR

pytestmark = pytest.mark.gpu

KAT_ROIS = np.array([[[0.1, 0.1, 0.2, 0.3, 0.5, 0.5, 0.3, 0.2], [0.5, 0.5, 0.6, 0.7, 0.9, 0.9, 0.7, 0.6],
                      [0.6, 0.7, 0.9, 0.9, 0.7, 0.6, 0.2, 0.2]]], np.float32)
KAT_ORDERS = np.array([[1, -1, 0]], np.int32)
KAT = {      # the reference's CPU functor on cpp/PSROIPooling/test_op.py:133-141; every bank channel of a bin equal
    'mean': ([[8.5625, 12.4375, 6.4375, 9.5625], [18.4375, 20.5625, 21.5625, 24.4375], [18.875, 23.875, 13.375, 19.875]],
             [[0] * 4] * 3),
    'max': ([[8.5625, 12.4375, 6.4375, 9.5625], [18.4375, 20.5625, 21.5625, 24.4375],
             [19.604166666666668, 23.875, 14.25, 20.020833333333332]], [[0] * 4, [0] * 4, [0, 0, 1, 1]]),
}


def kat_input():
    plane = np.arange(1, 26, dtype=np.float32).reshape(5, 5)
    return np.ascontiguousarray(np.tile(plane, (1, 16, 1, 1)), np.float32)


@pytest.mark.parametrize('method', ['mean', 'max'])
def test_known_answers(method):
    import xdet
    p, i = xdet.rotated_ps_roi_align(kat_input(), KAT_ROIS, KAT_ORDERS, 2, 2, method)
    assert p.shape == (1, 3, 4, 4) and i.shape == (1, 3, 4, 4) and i.dtype == np.int32
    vals, idx = KAT[method]
    for r in range(3):
        for b in range(4):
            assert np.all(p[0, r, b] == np.float32(vals[r][b])), (r, b, p[0, r, b])
            assert np.all(i[0, r, b] == idx[r][b])
    g = xdet.rotated_ps_roi_align_grad(kat_input(), KAT_ROIS, KAT_ORDERS, np.ones_like(p), i, 2, 2, method)
    assert g.shape == (1, 16, 5, 5)
    assert abs(float(g.astype(np.float64).sum()) - 48.) < 1e-4        # the 48 ones redistributed


@pytest.mark.parametrize('method', ['mean', 'max'])
@pytest.mark.parametrize('case', ['kat', 'g7', 'g32'])
def test_reference_fixture(case, method):
    import os
    import xdet
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'rotated_psroi_golden.npz'))
    gw, gh = (int(v) for v in z[case + '_grid'])
    inp, rois, orders = z[case + '_inputs'], z[case + '_rois'], z[case + '_orders']
    p, i = xdet.rotated_ps_roi_align(inp, rois, orders, gw, gh, method)
    assert np.array_equal(p.view(np.int32), z['%s_%s_pooled' % (case, method)].view(np.int32))
    assert np.array_equal(i, z['%s_%s_index' % (case, method)])
    g = xdet.rotated_ps_roi_align_grad(inp, rois, orders, z[case + '_grad'], i, gw, gh, method)
    assert np.abs(g - z['%s_%s_grad_inputs' % (case, method)]).max() <= 1e-5


def random_quads(rng, n, r):
    """rotated rectangles at random angles, general quads, 1-pixel quads, degenerate ones; orders in [-1, 4)"""
    cy, cx = rng.uniform(0.1, 0.9, (n, r)), rng.uniform(0.1, 0.9, (n, r))
    h, w = rng.uniform(0.02, 0.9, (n, r)), rng.uniform(0.02, 0.9, (n, r))
    a = rng.uniform(-np.pi, np.pi, (n, r))
    c, s = np.cos(a), np.sin(a)
    pts = []
    for dy, dx in ((-h / 2, -w / 2), (-h / 2, w / 2), (h / 2, w / 2), (h / 2, -w / 2)):
        pts += [cy + dy * c + dx * s, cx - dy * s + dx * c]
    q = np.stack(pts, -1)
    k = rng.random((n, r)) < 0.2                                      # general (also concave / crossing) quads
    q[k] = rng.uniform(0, 1, (int(k.sum()), 8))
    q = np.clip(q, 0., 1.).astype(np.float32)
    q[:, 0] = [0.5, 0.5, 0.5, 0.5, 0.5, 0.5, 0.5, 0.5]               # degenerate (a point)
    q[:, 1] = [0.2, 0.2, 0.2, 0.2, 0.6, 0.6, 0.6, 0.2]               # repeated vertex
    q[:, 2] = [0., 0., 0., 1., 1., 1., 1., 0.]                       # the full map
    orders = rng.integers(-1, 4, (n, r)).astype(np.int32)
    return q, orders


@pytest.mark.parametrize('method', ['max', 'mean'])
@pytest.mark.parametrize('shape', [(1, 490, 30, 30, 300, 7, 7), (3, 490, 30, 30, 1000, 7, 7), (64, 490, 30, 30, 300, 7, 7),
                                   (1, 490, 30, 30, 1000, 7, 7), (2, 490, 50, 50, 300, 7, 7), (2, 12, 9, 11, 40, 3, 2),
                                   (1, 6, 50, 50, 8, 1, 1), (3, 15, 8, 13, 50, 5, 3)])
def test_random_bit_exact(method, shape):
    """small calls run the direct kernel, the large NCHW ones the transposed-scratch form (R*C >= 4*H*W, even bank);
    odd banks keep the direct form; a 1 x 1 grid over a 50 x 50 map takes 51 x 51 samples per bin"""
    import xdet
    n, c, h, w, r, gw, gh = shape
    rng = np.random.default_rng(n * 1000 + r + h)
    feat = rng.standard_normal((n, c, h, w)).astype(np.float32)
    rois, orders = random_quads(rng, n, r)
    p, i = xdet.rotated_ps_roi_align(feat, rois, orders, gw, gh, method)
    po, io = RR.forward(feat, rois, orders, gw, gh, method)
    assert np.array_equal(p.view(np.int32), po.view(np.int32))
    assert np.array_equal(i, io)


def test_random_bit_exact_light_head_n64_r1000():
    import xdet
    n, c, h, w, r = 64, 490, 30, 30, 1000
    rng = np.random.default_rng(64)
    feat = rng.standard_normal((n, c, h, w)).astype(np.float32)
    rois, orders = random_quads(rng, n, r)
    p, i = xdet.rotated_ps_roi_align(feat, rois, orders, 7, 7, 'max')
    po, io = RR.forward(feat, rois, orders, 7, 7, 'max')
    assert np.array_equal(p.view(np.int32), po.view(np.int32))
    assert np.array_equal(i, io)


def _c_abi_fwd(feat_dev, rois, orders, n, c, h, w, r, gw, gh, use_max, layout, ldc, with_index=True, stream=None):
    from xdet._lib import lib, check
    from xdet.runtime import DeviceBuffer, to_device, to_host
    d_roi, d_ord = to_device(rois), to_device(orders)
    d_pool, d_idx = DeviceBuffer(n * r * c * 4), DeviceBuffer(n * r * c * 4)
    check(lib().xdet_rotated_psroialign_fwd(feat_dev.ptr, d_roi.ptr, d_ord.ptr, d_pool.ptr,
                                            d_idx.ptr if with_index else None, n, c, h, w, r, gw, gh, use_max, layout,
                                            ldc, stream.handle if stream else None))
    if stream:
        stream.synchronize()
    G = gw * gh
    p = to_host(d_pool.ptr, (n, r, G, c // G), np.float32)
    return p, (to_host(d_idx.ptr, (n, r, G, c // G), np.int32) if with_index else None)


@pytest.mark.parametrize('method', ['max', 'mean'])
@pytest.mark.parametrize('shape', [(64, 30, 30, 300, 7, 7, 10), (3, 30, 30, 1000, 7, 7, 10), (2, 13, 17, 40, 3, 5, 3)])
def test_nchw_and_nhwc_give_identical_bits(method, shape):
    """the net's layout (NHWC, channel stride ldc > C, two channels per lane for an even bank) against the op's NCHW --
    and the index output may be NULL"""
    from xdet.runtime import to_device
    n, h, w, r, gw, gh, bank = shape
    c = bank * gw * gh
    ldc = -(-c // 32) * 32 + 32
    rng = np.random.default_rng(r + h)
    feat = rng.standard_normal((n, c, h, w)).astype(np.float32)
    rois, orders = random_quads(rng, n, r)
    um = 1 if method == 'max' else 0
    p0, i0 = _c_abi_fwd(to_device(feat), rois, orders, n, c, h, w, r, gw, gh, um, 0, c)
    nhwc = np.full((n, h, w, ldc), np.nan, np.float32)             # the padding channels are never read
    nhwc[..., :c] = np.transpose(feat, (0, 2, 3, 1))
    d_nhwc = to_device(nhwc)
    p1, i1 = _c_abi_fwd(d_nhwc, rois, orders, n, c, h, w, r, gw, gh, um, 1, ldc)
    assert np.array_equal(p0.view(np.int32), p1.view(np.int32))
    assert np.array_equal(i0, i1)
    p2, _ = _c_abi_fwd(d_nhwc, rois, orders, n, c, h, w, r, gw, gh, um, 1, ldc, with_index=False)
    assert np.array_equal(p0.view(np.int32), p2.view(np.int32))
    p3, _ = _c_abi_fwd(to_device(feat), rois, orders, n, c, h, w, r, gw, gh, um, 0, c, with_index=False)
    assert np.array_equal(p0.view(np.int32), p3.view(np.int32))
    po, io = RR.forward(feat, rois, orders, gw, gh, method)
    assert np.array_equal(p0.view(np.int32), po.view(np.int32)) and np.array_equal(i0, io)


@pytest.mark.parametrize('method', ['max', 'mean'])
@pytest.mark.parametrize('layout', [0, 1])
def test_guard_band(method, layout):
    """the map is image 1 of three in one allocation, images 0 and 2 NaN; quads straddle or leave the map (where the
    reference reads outside the plane).  Outputs are finite and follow the clamping rule (include/xdet.h)"""
    from xdet.runtime import to_device
    c, h, w, r, gw, gh = 98, 9, 11, 200, 7, 7
    rng = np.random.default_rng(3 + layout)
    feat = rng.standard_normal((1, c, h, w)).astype(np.float32)
    rois = rng.uniform(-0.6, 1.6, (1, r, 8)).astype(np.float32)
    rois[0, :4] = [[0., 0., 0., 1., 1., 1., 1., 0.]] * 4            # samples on y = H exactly
    rois[0, 4] = [1., 0.1, 1., 0.9, 1., 0.9, 1., 0.1]
    rois[0, 5] = [1., 0.1, 1., 0.9, 1.0001, 0.9, 1.0001, 0.1]        # all vertices on y ~ 1: integer part = H
    rois[0, 6] = [-0.05, -0.05, -0.05, 0.5, 0.5, 0.5, 0.5, -0.05]    # -1 < coordinate < 0: the reference extrapolates
    orders = rng.integers(-1, 4, (1, r)).astype(np.int32)
    assert RR.out_of_bounds(rois, orders, h, w, gw, gh).sum() > r // 2
    if layout == 0:
        band = np.full((3, c, h, w), np.nan, np.float32)
        band[1] = feat[0]
        ldc = c
    else:
        ldc = c + 30
        band = np.full((3, h, w, ldc), np.nan, np.float32)
        band[1, :, :, :c] = np.transpose(feat[0], (1, 2, 0))
    d = to_device(band)

    class View:
        ptr = d.ptr + band[0].nbytes
    p, i = _c_abi_fwd(View, rois, orders, 1, c, h, w, r, gw, gh, 1 if method == 'max' else 0, layout, ldc)
    assert np.all(np.isfinite(p))
    po, io = RR.forward(feat, rois, orders, gw, gh, method)
    assert np.array_equal(p.view(np.int32), po.view(np.int32))
    assert np.array_equal(i, io)
    # the gradient writes inside the plane only: the guard images stay untouched
    from xdet._lib import lib, check
    from xdet.runtime import DeviceBuffer, to_host
    G = rng.uniform(-1, 1, p.shape).astype(np.float32)
    gband = DeviceBuffer(band.nbytes)
    sentinel = np.full(band.shape, 7., np.float32)
    check(lib().xdet_memcpy_h2d(gband.ptr, sentinel.ctypes.data, band.nbytes, None))
    d_roi, d_ord, d_g, d_i = to_device(rois), to_device(orders), to_device(G), to_device(i)
    check(lib().xdet_rotated_psroialign_grad(d_roi.ptr, d_ord.ptr, d_g.ptr, d_i.ptr, gband.ptr + band[0].nbytes, 1, c,
                                             h, w, r, gw, gh, 1 if method == 'max' else 0, layout, ldc, None))
    got = to_host(gband.ptr, band.shape, np.float32)
    assert np.all(got[0] == 7.) and np.all(got[2] == 7.)
    gm = got[1] if layout == 0 else np.transpose(got[1][..., :c], (2, 0, 1))
    ref = RR.gradient((1, c, h, w), rois, orders, G, i, gw, gh, method)[0]
    assert np.abs(gm - ref).max() <= 1e-5
    if layout == 1:
        assert np.all(got[1][..., c:] == 0.)                         # zero-filled over the whole stride


@pytest.mark.parametrize('method', ['max', 'mean'])
@pytest.mark.parametrize('shape', [(1, 490, 30, 30, 300, 7, 7), (3, 36, 50, 50, 64, 3, 3), (2, 12, 9, 11, 40, 3, 2),
                                   (1, 6, 50, 50, 8, 1, 1)])
def test_gradient_matches_the_restatement(method, shape):
    import xdet
    n, c, h, w, r, gw, gh = shape
    rng = np.random.default_rng(9 + r)
    feat = rng.standard_normal((n, c, h, w)).astype(np.float32)
    rois, orders = random_quads(rng, n, r)
    _, idx = RR.forward(feat, rois, orders, gw, gh, method)
    G = rng.uniform(-1, 1, idx.shape).astype(np.float32)
    got = xdet.rotated_ps_roi_align_grad(feat, rois, orders, G, idx, gw, gh, method)
    ref = RR.gradient(feat.shape, rois, orders, G, idx, gw, gh, method)
    assert got.shape == ref.shape
    assert np.abs(got - ref).max() <= 1e-5


def test_two_streams_concurrently():
    from xdet.runtime import Stream, to_device
    n, c, h, w, r = 8, 490, 30, 30, 300
    rng = np.random.default_rng(2)
    fa, fb = (rng.standard_normal((n, c, h, w)).astype(np.float32) for _ in range(2))
    (ra, oa), (rb, ob) = random_quads(rng, n, r), random_quads(rng, n, r)
    one_a, _ = _c_abi_fwd(to_device(fa), ra, oa, n, c, h, w, r, 7, 7, 1, 0, c)
    one_b, _ = _c_abi_fwd(to_device(fb), rb, ob, n, c, h, w, r, 7, 7, 1, 0, c)
    from xdet._lib import lib, check
    from xdet.runtime import DeviceBuffer, to_host
    sa, sb = Stream(), Stream()
    bufs = []
    for f, ro, o, st in ((fa, ra, oa, sa), (fb, rb, ob, sb)):
        d_f, d_r, d_o, d_p = to_device(f), to_device(ro), to_device(o), DeviceBuffer(n * r * c * 4)
        bufs.append((d_f, d_r, d_o, d_p, st))
    for _ in range(3):
        for d_f, d_r, d_o, d_p, st in bufs:
            check(lib().xdet_rotated_psroialign_fwd(d_f.ptr, d_r.ptr, d_o.ptr, d_p.ptr, None, n, c, h, w, r, 7, 7, 1, 0,
                                                    c, st.handle))
    sa.synchronize()
    sb.synchronize()
    for (d_f, d_r, d_o, d_p, st), one in zip(bufs, (one_a, one_b)):
        got = to_host(d_p.ptr, one.shape, np.float32)
        assert np.array_equal(got.view(np.int32), one.view(np.int32))
