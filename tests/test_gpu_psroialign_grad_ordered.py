"""xdet_psroialign_grad_ordered on the GPU: bit-identical to the oracle's sequential gradient (np.array_equal everywhere),
in both layouts, with leading dimensions, corner boxes, a poisoned output and out-of-range indices; then through the net:
the kept argmax and head_backward(..., to_feat=True)."""
import numpy as np
import pytest

import psroi_grad_ordered_cases as PC

pytestmark = pytest.mark.gpu
f32 = np.float32


def run(rois, grad, index, shape, method, layout=0, ldc=None, corners=0, ld=None, expect=0):
    """one call of the C door on a NaN-filled output -> the raw output array ([N,C,H,W], or [N,H,W,ldc] for layout 1).
    ld: grad / index rows are padded to this leading dimension with sentinels (NaN / 2^30)."""
    from xdet._lib import lib
    from xdet.runtime import DeviceBuffer, to_device, to_host, synchronize
    n, c, h, w, r, g = shape
    ldc = c if ldc is None else ldc
    grad = np.asarray(grad, f32).reshape(n * r, c)
    if ld is not None:
        gp = np.full((n * r, ld), np.nan, f32)
        gp[:, :c] = grad
        grad = gp
    d_grad = to_device(grad) if grad.size else DeviceBuffer(16)
    d_idx = None
    if index is not None:
        index = np.asarray(index, np.int32).reshape(n * r, c)
        if ld is not None:
            ip = np.full((n * r, ld), 2 ** 30, np.int32)
            ip[:, :c] = index
            index = ip
        d_idx = to_device(index) if index.size else DeviceBuffer(16)
    rois = np.ascontiguousarray(rois, f32)
    d_roi = to_device(rois) if rois.size else DeviceBuffer(16)
    out_shape = (n, c, h, w) if layout == 0 else (n, h, w, ldc)
    d_out = to_device(np.full(out_shape, np.nan, f32))
    rc = lib().xdet_psroialign_grad_ordered(d_roi.ptr, d_grad.ptr, ld or c, d_idx.ptr if d_idx else None, ld or c, d_out.ptr,
                                            n, c, h, w, r, g, g, 1 if 'max' in method else 0, layout, ldc, corners, None)
    assert rc == expect, (rc, lib().xdet_last_error())
    synchronize()
    return to_host(d_out.ptr, out_shape, f32)


def nhwc(ref, ldc):
    n, c, h, w = ref.shape
    out = np.zeros((n, h, w, ldc), f32)
    out[..., :c] = ref.transpose(0, 2, 3, 1)
    return out


@pytest.mark.parametrize('method', ['max', 'mean'])
@pytest.mark.parametrize('shape', [PC.SMALL, PC.PLANES10K, PC.NET])
def test_bit_exact_against_the_oracle(shape, method, oracle):
    """every layout on a NaN-filled output: no NaN is left, padding channels are exact zeros, all bits the oracle's"""
    rois, grad, index, ref = PC.case(shape, method, oracle)
    c = shape[1]
    got = run(rois, grad, index, shape, method)
    print('%r %s: %d of %d elements differ (NCHW)' % (shape, method, (got != ref).sum(), ref.size))
    assert ref.any() and np.array_equal(got, ref)
    for ldc in (c, c + 6):
        got = run(rois, grad, index, shape, method, layout=1, ldc=ldc)
        want = nhwc(ref, ldc)
        print('%r %s: %d of %d elements differ (NHWC, ldc %d)' % (shape, method, (got != want).sum(), want.size, ldc))
        assert not np.isnan(got).any()
        assert not got[..., c:].any() and np.array_equal(got, want)


def test_heavy_overlap(oracle):
    """64 copies of the full-image box, 'mean': every pixel sums hundreds of terms, and
    tests/test_psroialign_grad_ordered_math.py shows that another ROI order gives other bits on this input"""
    rois, grad, index, ref = PC.case(PC.HEAVY, 'mean', oracle)
    got = run(rois, grad, index, PC.HEAVY, 'mean')
    print('heavy overlap: %d of %d elements differ' % ((got != ref).sum(), ref.size))
    assert np.array_equal(got, ref)
    assert np.array_equal(run(rois, grad, index, PC.HEAVY, 'mean', layout=1, ldc=22), nhwc(ref, 22))


@pytest.mark.parametrize('method', ['max', 'mean'])
def test_corner_boxes(method, oracle):
    """rois_are_corners=1 gives the bits of the centre boxes converted in f32 NumPy (hh = y1 - y0; cy = y0 + hh / 2)"""
    rois, grad, _, _ = PC.case(PC.SMALL, method, oracle)
    corners, centres = PC.corners_of(rois)
    n, c, h, w, r, g = PC.SMALL
    feat = np.random.default_rng(5).standard_normal((n, c, h, w)).astype(f32)
    _, index = oracle.ps_roi_align(feat, centres, g, g, method)
    ref = oracle.ps_roi_align_grad(feat, centres, grad, index, g, g, method)
    assert np.array_equal(run(centres, grad, index, PC.SMALL, method), ref)
    assert np.array_equal(run(corners, grad, index, PC.SMALL, method, corners=1), ref)
    assert np.array_equal(run(corners, grad, index, PC.SMALL, method, corners=1, layout=1, ldc=c + 6), nhwc(ref, c + 6))


@pytest.mark.parametrize('method', ['max', 'mean'])
def test_leading_dimensions(method, oracle):
    """ld_grad = ld_index = C + 3 with sentinels in the pad columns: the packed call's bits"""
    rois, grad, index, ref = PC.case(PC.SMALL, method, oracle)
    assert np.array_equal(run(rois, grad, index, PC.SMALL, method, ld=PC.SMALL[1] + 3), ref)
    rois, grad, index, ref = PC.case(PC.NET, method, oracle)
    assert np.array_equal(run(rois, grad, index, PC.NET, method, ld=PC.NET[1] + 3, layout=1, ldc=512), nhwc(ref, 512))


def test_out_of_range_index(oracle):
    """one interior box on 30 x 30 with grid 2 (8 x 8 samples per bin; a sample one step past the bin is still inside the map):
    an index of n_h*n_w and of -1 contribute nothing for their elements"""
    shape = (1, 16, 30, 30, 1, 2)
    rng = np.random.default_rng(PC.SEED)
    feat = rng.standard_normal((1, 16, 30, 30)).astype(f32)
    rois = np.array([[[0.5, 0.5, 0.5, 0.5]]], f32)
    grad = rng.standard_normal((1, 1, 16)).astype(f32)
    _, index = oracle.ps_roi_align(feat, rois, 2, 2, 'max')
    index = index.reshape(1, 1, 16).copy()
    assert index.max() < 64
    bad, g0, i0 = index.copy(), grad.copy(), index.copy()
    bad[0, 0, [1, 6, 15]] = 64
    bad[0, 0, [0, 9]] = -1
    bad[0, 0, 12] = 2 ** 31 - 1
    for e in (1, 6, 15, 0, 9, 12):
        g0[0, 0, e] = 0
        i0[0, 0, e] = 0
    ref = oracle.ps_roi_align_grad(feat, rois, g0, i0, 2, 2, 'max')
    got = run(rois, grad, bad, shape, 'max')
    assert ref.any() and np.array_equal(got, ref)
    assert not got[0, [1, 6, 15, 0, 9, 12]].any() and got[0, 2].any()


def test_determinism_and_null_index(oracle):
    rois, grad, index, ref = PC.case(PC.PLANES10K, 'max', oracle)
    a = run(rois, grad, index, PC.PLANES10K, 'max', layout=1, ldc=36)
    b = run(rois, grad, index, PC.PLANES10K, 'max', layout=1, ldc=36)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    rois, grad, index, ref = PC.case(PC.SMALL, 'mean', oracle)
    a = run(rois, grad, None, PC.SMALL, 'mean')
    b = run(rois, grad, np.full(index.shape, 7, np.int32), PC.SMALL, 'mean')
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)) and np.array_equal(a, ref)


def test_refusals_and_empty_input(oracle):
    """the refusals of the no-GPU module with a device present, through both doors; N*R = 0 writes zeros"""
    import xdet
    from xdet._lib import lib
    for kw in PC.REFUSALS:
        assert PC.c_call(lib(), **kw) == -1, kw
    z = np.zeros
    with pytest.raises(xdet.InvalidArgumentError):          # beyond any LDS plane
        xdet.ps_roi_align_grad(z((1, 4, 512, 512), f32), z((1, 2, 4), f32), z((1, 2, 4), f32), z((1, 2, 4), np.int32), 2, 2, 'max',
                               ordered=True)
    assert not xdet.ps_roi_align_grad(z((1, 4, 512, 512), f32), z((1, 2, 4), f32), z((1, 2, 4), f32), z((1, 2, 4), np.int32), 2, 2,
                                      'max').any()          # ... which the atomic entry still takes
    shape = (2, 16, 5, 7, 0, 2)
    for layout, ldc in ((0, 16), (1, 19)):
        got = run(z((2, 0, 4), f32), z((2, 0, 16), f32), z((2, 0, 16), np.int32), shape, 'max', layout=layout, ldc=ldc)
        assert got.size and not got.any() and not np.isnan(got).any()


def test_python_doors(oracle):
    """ops.ps_roi_align_grad(ordered=True) and ops.ps_roi_align_grad_device give the oracle's bits"""
    import xdet
    from xdet.runtime import DeviceTensor, to_host
    n, c, h, w, r, g = PC.SMALL
    for method in ('max', 'mean'):
        rois, grad, index, ref = PC.case(PC.SMALL, method, oracle)
        got = xdet.ps_roi_align_grad(np.empty((n, c, h, w), f32), rois, grad.reshape(n, r, g * g, -1), index.reshape(n, r, g * g, -1),
                                     g, g, method, ordered=True)
        assert np.array_equal(got, ref)
        d_grad = DeviceTensor.from_numpy(grad.reshape(n, r, 1, c))            # ld 32
        t = xdet.ps_roi_align_grad_device(rois, d_grad, index if method == 'max' else None, (n, h, w, c), g, g, method)
        assert isinstance(t, DeviceTensor) and t.shape == (n, h, w, c) and t.ld == 32
        xdet.synchronize()
        assert np.array_equal(to_host(t.ptr, (n, h, w, t.ld)), nhwc(ref, t.ld))


def test_through_the_net(lh_weights, oracle):
    """follows tests/test_gpu_dense_backward.py::test_head_backward_through_the_net: a 64-ROI head detector built with
    pool_index=True, get_head in training mode with OHEM 32, then head_backward(..., to_feat=True)"""
    import xdet
    from xdet import model as M, losses as L
    from xdet.model import LightHeadDetector
    from xdet.runtime import to_host
    S, P, nc, C = 256, 64, 21, 490
    head = LightHeadDetector(lh_weights, image_size=S, max_batch=2, rpn_post_nms_top_n=P, pool_index=True)
    rng = np.random.default_rng(11)
    with head.scope():
        shp = head.buffer('feat', 2).shape
        assert shp == (2, 16, 16, C)
        feat = rng.standard_normal(shp).astype(f32)
        ctr, hw = rng.uniform(0.25, 0.75, (2, P, 2)), rng.uniform(0.1, 0.4, (2, P, 2))
        rois = np.concatenate([ctr - hw / 2, ctr + hw / 2], -1).astype(f32)
        labels = rng.integers(-1, nc, (2, P)).astype(np.int32)
        targets = (rng.standard_normal((2, P, 4)) * 0.2).astype(f32)
        loss_func = L.HeadLoss(labels, targets, 0.25)
        M.get_head(feat, None, 7, 7, loss_func, rois, nc, True, True, 32, 'channels_first', 'final_head')
        pi = head.buffer('pool_index', 2)
        assert pi.shape == (2, P, 1, C)
        kept_index = to_host(pi.ptr, (2, P, pi.ld), np.int32)[..., :C]
        grads = M.head_backward(loss_func, to_feat=True)
        d_feat = grads['feat']
        raw = to_host(d_feat.ptr, (2, 16, 16, d_feat.ld))
        assert d_feat.shape == (2, 16, 16, C) and d_feat.ld == head.buffer('feat', 2).ld
    centres = PC.point2center(rois)
    _, want_index = oracle.ps_roi_align(feat, centres, 7, 7, 'max', layout='NHWC')
    assert np.array_equal(kept_index, want_index.reshape(2, P, C))
    d_pooled = grads['pooled'].numpy().reshape(2, P, C)
    like = np.empty((2, C, 16, 16), f32)
    ref = oracle.ps_roi_align_grad(like, centres, d_pooled, kept_index, 7, 7, 'max')
    assert ref.any() and not raw[..., C:].any()
    assert np.array_equal(raw[..., :C], ref.transpose(0, 2, 3, 1))
    # the ROIs OHEM dropped have all-zero gradient rows: without them (order kept) the oracle gives the same bits
    sel = np.sort(loss_func.result.select, axis=1)
    assert sel.shape == (2, 32)
    take = lambda a: np.stack([a[n][sel[n]] for n in range(2)])
    ref_kept = oracle.ps_roi_align_grad(like, take(centres), take(d_pooled), take(kept_index), 7, 7, 'max')
    assert np.array_equal(ref_kept, ref)
    # the default detector: no index, no 'feat', today's keys
    plain = LightHeadDetector(lh_weights, image_size=S, max_batch=2, rpn_post_nms_top_n=P)
    with plain.scope():
        lf = L.HeadLoss(labels, targets, 0.25)
        M.get_head(feat, None, 7, 7, lf, rois, nc, True, True, 32, 'channels_first', 'final_head')
        with pytest.raises(xdet.InvalidArgumentError):
            M.head_backward(lf, to_feat=True)
        with pytest.raises(xdet.InvalidArgumentError):
            plain.buffer('pool_index', 2)
        g2 = M.head_backward(lf)
        assert set(g2) == set(grads) - {'feat'} and len(g2) == 8
        assert np.array_equal(g2['pooled'].numpy(), grads['pooled'].numpy())
