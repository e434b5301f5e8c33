"""F1 with the reference's `resize` argument (preprocessing/common_preprocessing.py:29-32,383-440) on the CPU: the NumPy
restatement (tests/preprocess_modes_ref.py) against the oracle and against the reference's arithmetic, the host side of
xdet.ops (GT box mapping, difficults, argument checks before any GPU work)."""
import os

import numpy as np
import pytest

import preprocess_modes_ref as P

HERE = os.path.dirname(os.path.abspath(__file__))
f32 = np.float32


def demo_image():
    return np.load(os.path.join(HERE, 'golden', 'demo_test_u8.npz'))['image']


def rand_image(H, W, seed=0):
    return np.random.default_rng(seed + 7 * H + W).integers(0, 256, (H, W, 3), dtype=np.uint8)


def near_integer_shapes(S, limit=8):
    """(H, W) whose f64 factor * H lands within an ulp of an integer: floor() of the f64 product differs from the
    exact rational floor(S * H / max(H, W)), or the product is an integer only up to rounding"""
    out = []
    for W in range(S + 1, 4 * S):
        for H in range(1, W + 1):
            prod = (np.float64(S) / np.float64(W)) * np.float64(H)
            exact_floor = (S * H) // W
            if int(np.floor(prod)) != exact_floor or (prod != np.floor(prod) and abs(prod - round(prod)) <= np.spacing(prod)):
                out.append((H, W))
                if len(out) >= limit:
                    return out
    return out


def test_warp_restatement_is_the_oracle_bit_for_bit(oracle):
    cases = [demo_image()] + [rand_image(h, w) for h, w in ((500, 375), (97, 1013), (1, 1), (479, 481), (64, 64))]
    for img in cases:
        for S in (480, 256):
            got, bimg = P.preprocess(img, S, P.WARP_RESIZE)
            assert np.array_equal(got, oracle.preprocess_for_eval(img, S)), (img.shape, S)
            assert np.array_equal(bimg, np.array([0, 0, 1, 1], f32))


@pytest.mark.parametrize('shape', [(333, 500), (500, 375), (700, 700), (97, 1013), (1013, 97), (300, 200), (1, 1)])
def test_pad_and_resize(shape):
    S = 480
    img = rand_image(*shape)
    out, bimg = P.preprocess(img, S, P.PAD_AND_RESIZE)
    rh, rw = P.pad_resize_shape(*shape, S)
    if max(shape) <= S:
        assert (rh, rw) == shape                               # factor = 1: never upscaled
    else:
        assert max(rh, rw) == S or max(rh, rw) == S - 1
    py, px = (S - rh) // 2, (S - rw) // 2
    inner = np.zeros((3, S, S), bool)
    inner[:, py:py + rh, px:px + rw] = True
    assert np.all(out[~inner] == 0) and not np.signbit(out[~inner]).any()    # +0 in whitened space
    warp = P.bilinear(P.whiten(img), rh, rw).transpose(2, 0, 1)
    assert np.array_equal(out[:, py:py + rh, px:px + rw], warp)
    if max(shape) <= S:                                        # and the resize to the same size is the identity
        assert np.array_equal(warp, P.whiten(img).transpose(2, 0, 1))


def test_pad_and_resize_shape_is_the_f64_formula():
    from xdet import ops
    S = 480
    shapes = near_integer_shapes(S)
    assert shapes, 'no shape lands within an ulp of an integer'
    for H, W in shapes + [(333, 500), (500, 333), (960, 481), (481, 960)]:
        factor = min(1.0, min(np.float64(S) / H, np.float64(S) / W))
        want = (int(np.floor(factor * np.float64(H))), int(np.floor(factor * np.float64(W))))
        assert P.pad_resize_shape(H, W, S) == want
        assert ops.resize_geometry(H, W, S, ops.Resize.PAD_AND_RESIZE)[0] == want
    # the rounding matters: at least one of them differs from the exact rational floor
    assert any(P.pad_resize_shape(H, W, S)[0] != (S * H) // W for H, W in shapes)


@pytest.mark.parametrize('shape', [(700, 300), (301, 481), (480, 480), (481, 479), (1013, 97), (333, 500), (2, 999)])
def test_central_crop_interior_is_pure_whitening(shape):
    S = 480
    H, W = shape
    img = rand_image(H, W)
    out, _ = P.preprocess(img, S, P.CENTRAL_CROP)
    cy, cx = max((H - S) // 2, 0), max((W - S) // 2, 0)
    py, px = max((S - H) // 2, 0), max((S - W) // 2, 0)
    kh, kw = min(S, H), min(S, W)
    x = P.whiten(img).transpose(2, 0, 1)
    assert np.array_equal(out[:, py:py + kh, px:px + kw], x[:, cy:cy + kh, cx:cx + kw])
    mask = np.ones((S, S), bool)
    mask[py:py + kh, px:px + kw] = False
    assert np.all(out[:, mask] == 0)
    # odd differences: floor division puts the extra row / column at the end
    if (H - S) % 2:
        assert cy == (H - S - 1) // 2 if H > S else py == (S - H - 1) // 2


def test_none_is_whitening_and_needs_s_by_s():
    img = rand_image(64, 64)
    out, bimg = P.preprocess(img, 64, P.NONE)
    assert np.array_equal(out, P.whiten(img).transpose(2, 0, 1))
    assert np.array_equal(bimg, np.array([0, 0, 1, 1], f32))
    bad, bb = P.preprocess(rand_image(64, 63), 64, P.NONE)
    assert np.isnan(bad).all() and np.isnan(bb).all()


@pytest.mark.parametrize('mode', [P.CENTRAL_CROP, P.PAD_AND_RESIZE])
@pytest.mark.parametrize('shape', [(333, 500), (700, 300), (301, 481), (97, 1013), (479, 481)])
def test_bbox_img_and_gt_boxes(mode, shape):
    from xdet import ops
    S = 480
    H, W = shape
    _, bimg = P.preprocess(rand_image(H, W), S, mode)
    # the f32 two-step formula, written out
    h, w = P.pad_resize_shape(H, W, S) if mode == P.PAD_AND_RESIZE else (H, W)
    cy, cx, py, px, kh, kw = max((h - S) // 2, 0), max((w - S) // 2, 0), max((S - h) // 2, 0), max((S - w) // 2, 0), min(S, h), min(S, w)
    b = np.array([0, 0, 1, 1], f32)
    b = ((b * np.array([h, w, h, w], f32)) + np.array([-cy, -cx, -cy, -cx], f32)) / np.array([kh, kw, kh, kw], f32)
    b = ((b * np.array([kh, kw, kh, kw], f32)) + np.array([py, px, py, px], f32)) / np.array([S, S, S, S], f32)
    assert b.dtype == f32 and np.array_equal(bimg, b)
    if mode == P.PAD_AND_RESIZE or (H <= S and W <= S):
        assert not np.array_equal(bimg, np.array([0, 0, 1, 1], f32)) or (h, w) == (S, S)
    # the product's host mapping: [0,0,1,1] -> bbox_img, and bboxes_resize(bbox_img, .) undoes the mapping
    assert np.array_equal(ops._map_gt_boxes([[0, 0, 1, 1]], H, W, S, mode)[0], bimg)
    gt = np.array([[0.1, 0.2, 0.6, 0.9], [0.3, 0.3, 0.4, 0.35], [0.45, 0.45, 0.55, 0.55]], f32)
    mapped = ops._map_gt_boxes(gt, H, W, S, mode)
    assert np.array_equal(mapped, P.map_boxes(gt, H, W, S, mode))
    back = P.bboxes_resize(bimg, mapped)
    assert np.abs(back - gt).max() < 4e-6, np.abs(back - gt).max()


def test_difficults_are_removed_with_their_labels(monkeypatch):
    from xdet import ops

    def restated(images, out_size, resize=ops.Resize.WARP_RESIZE, stream=None):
        outs = [P.preprocess(im, out_size, int(resize)) for im in images]
        return (np.stack([o[0] for o in outs]), np.stack([o[1] for o in outs]),
                np.array([im.shape[:2] for im in images], np.int32))
    monkeypatch.setattr(ops, 'light_head_preprocess_batch', restated)
    img = rand_image(333, 500)
    labels = np.array([3, 7, 12, 15], np.int64)
    gt = np.array([[.1, .1, .5, .5], [.2, .3, .4, .9], [.0, .0, 1., 1.], [.6, .6, .7, .8]], f32)
    diff = np.array([0, 1, 0, 1], np.int64)
    for mode in ops.Resize:
        if mode == ops.Resize.NONE:
            continue
        out, lab, bb, bimg = ops.light_head_preprocess_for_eval(img, labels, gt, [480, 480], 'NCHW', diff, resize=mode)
        ref, rb = P.preprocess(img, 480, int(mode))
        assert np.array_equal(out, ref) and np.array_equal(bimg, rb)
        assert lab.tolist() == [3, 12]
        assert np.array_equal(bb, P.map_boxes(gt, 333, 500, 480, int(mode))[[0, 2]])
    # the default: WARP, no difficults -> labels and boxes as given, bbox_img [0,0,1,1]
    out, lab, bb, bimg = ops.light_head_preprocess_for_eval(img, labels, gt, [480, 480], 'NHWC')
    assert out.shape == (480, 480, 3) and lab.tolist() == labels.tolist() and np.array_equal(bb, gt)
    assert np.array_equal(bimg, np.array([0, 0, 1, 1], f32))


def test_resize_enum_is_the_references():
    from xdet import ops
    assert [(m.name, int(m)) for m in ops.Resize] == [('NONE', 1), ('CENTRAL_CROP', 2), ('PAD_AND_RESIZE', 3),
                                                       ('WARP_RESIZE', 4)]
    assert (P.NONE, P.CENTRAL_CROP, P.PAD_AND_RESIZE, P.WARP_RESIZE) == tuple(int(m) for m in ops.Resize)


def test_argument_errors_are_raised_before_any_gpu_work(monkeypatch):
    import xdet
    from xdet import ops
    from xdet import model as M

    def no_gpu(*a, **k):
        raise AssertionError('GPU work before the argument checks')
    monkeypatch.setattr(ops, 'to_device', no_gpu)
    monkeypatch.setattr(ops, 'lib', no_gpu)
    monkeypatch.setattr(M, 'lib', no_gpu)
    monkeypatch.setattr(M, 'DeviceBuffer', no_gpu)
    ok = rand_image(20, 30)
    bad_batches = [
        [ok[..., 0]],                                  # ndim 2
        [ok[None]],                                    # ndim 4
        [np.zeros((20, 30, 4), np.uint8)],             # 4 channels
        [np.zeros((20, 30, 1), np.uint8)],             # 1 channel
        [ok, np.zeros((0, 30, 3), np.uint8)],          # empty
        [np.zeros((20, 0, 3), np.uint8)],
        [ok.astype(np.float32)],                       # not uint8
        [],                                            # no images
        ok,                                            # one image instead of a list
    ]
    for imgs in bad_batches:
        with pytest.raises(xdet.InvalidArgumentError):
            ops.light_head_preprocess_batch(imgs, 64)
    for resize in (0, 5, 'WARP', None):
        with pytest.raises(xdet.InvalidArgumentError):
            ops.light_head_preprocess_batch([ok], 64, resize)
    with pytest.raises(xdet.InvalidArgumentError):
        ops.light_head_preprocess_batch([ok], 0)
    with pytest.raises(xdet.InvalidArgumentError):
        ops.light_head_preprocess_batch([ok], 64, ops.Resize.NONE)      # NONE needs S x S
    with pytest.raises(xdet.InvalidArgumentError):
        ops.light_head_preprocess_for_eval(ok[..., 0])
    with pytest.raises(ValueError):                                     # (the reference raises ValueError)
        ops.light_head_preprocess_for_eval(ok[..., 0])
    with pytest.raises(xdet.InvalidArgumentError):
        ops.light_head_preprocess_for_eval(ok, out_shape=(64, 32))
    det = M.LightHeadDetector.__new__(M.LightHeadDetector)
    det.image_size, det.max_batch = 64, 2
    for imgs in bad_batches + [[ok, ok, ok]]:                           # too many images for max_batch
        with pytest.raises(xdet.InvalidArgumentError):
            det.detect_images(imgs)
    with pytest.raises(xdet.InvalidArgumentError):
        det.detect_images([ok], resize=9)


def test_abi_entries_are_declared():
    from xdet import _lib
    assert 'xdet_preprocess_eval_batch' in _lib.SIGNATURES and 'xdet_net_forward_u8' in _lib.SIGNATURES
    hdr = open(os.path.join(os.path.dirname(HERE), 'include', 'xdet.h')).read()
    for name, v in (('NONE', 1), ('CENTRAL_CROP', 2), ('PAD_AND_RESIZE', 3), ('WARP', 4)):
        assert 'XDET_RESIZE_%s = %d' % (name, v) in hdr
