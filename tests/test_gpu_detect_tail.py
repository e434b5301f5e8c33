"""The detection tail in the form the whole forward runs (csrc/detect.hip: head_decode_probs_lanes_kernel /
head_decode_probs_kernel -> class-major probabilities -> bboxes_eval_kernel<true>) through its own entry points
(xdet_head_decode_probs, xdet_bboxes_eval_probs), against float64 / the oracle, and bit for bit against the logits form
(xdet_ext_decode_rois, xdet_bboxes_eval).  The inputs and what each is for: tests/detect_tail_cases.py; that they have the
properties they are named for: tests/test_detect_tail_math.py.

Bit equality, as measured on an MI355X: the three "same bits" claims of detect.hip hold -- 32 lanes per ROI == one thread per
ROI (2, 21, 28 classes), the register branch and the class_probs_begin branch == the in-kernel softmax of the logits form
(every class count below), batched == per image.

Against the oracle a case asserts: the number of positive scores per class, scores within 1e-6, boxes within 1e-6, and both
forms equal bit for bit.  With a bbox_img other than the frame the oracle's zero-score padding rows carry the resized zero box
(-y0 / h, ...); the kernels write zeros there, as for every other bbox_img: those rows are compared as "zero" instead."""
import numpy as np
import pytest

import detect_tail_cases as T

pytestmark = pytest.mark.gpu

f32 = np.float32
NC_ALL = [2, 21, 28, 29, 32, 33, 81]        # lanes kernel up to 28; registers up to 32; class_probs_begin above


def _bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _same_dets(a, b):
    """two {class: (scores, boxes)} dicts, bit for bit (NaN == NaN when its bits are)"""
    return a.keys() == b.keys() and all(_same_bits(a[c][0], b[c][0]) and _same_bits(a[c][1], b[c][1]) for c in a)


def _vs_oracle(got, ref, nc, topk, tag, unit_frame=True, first_is_nan=False):
    for c in range(1, nc):
        gs, gb = got[c]
        rs, rb = ref[c]
        assert gs.shape == (topk,) and gb.shape == (topk, 4)
        if first_is_nan:
            assert np.isnan(gs[0]), (tag, c)
            gs, rs = gs[1:], rs[1:]
        k, kr = int((gs > 0).sum()), int((rs > 0).sum())
        assert k == kr, (tag, c, k, kr)
        assert np.abs(gs - rs).max(initial=0) <= 1e-6, (tag, c)
        if unit_frame:
            assert np.abs(gb - rb).max() <= 1e-6, (tag, c)
        else:
            k += int(first_is_nan)
            assert np.abs(gb[:k] - rb[:k]).max(initial=0) <= 1e-6 and not gb[k:].any(), (tag, c)


def _pad_nan(cls_reg, extra):
    if not extra:
        return cls_reg
    out = np.full((cls_reg.shape[0], cls_reg.shape[1] + extra), np.nan, f32)
    out[:, :cls_reg.shape[1]] = cls_reg
    return out


def _probs_of(logits, R):
    """class-major probabilities of logits [n, nc] through the net's kernel (zero regression values, unit ROIs)"""
    from xdet import ops
    n, nc = logits.shape
    cls_reg = np.concatenate([logits, np.zeros((n, 4), f32)], 1)
    rois = np.tile(np.array([0, 0, 1, 1], f32), (n, 1))
    _, probs, bad = ops.head_decode_probs(rois, cls_reg, nc, R)
    assert not bad.any()
    return probs


def _both_forms(logits, boxes, R, **kw):
    """logits [N*R, nc], boxes [N*R, 4] -> the detections of the probabilities form, after asserting that the logits form's
    are the same bits"""
    from xdet import ops
    nc = logits.shape[1]
    N = logits.shape[0] // R
    pre = ops.bboxes_eval_from_probs(_probs_of(logits, R), boxes, **kw)
    raw = ops.bboxes_eval(logits.reshape(N, R, nc), boxes.reshape(N, R, 4), num_classes=nc, **kw)
    for i in range(N):
        assert _same_dets(pre[i], raw[i]), ('probabilities form != logits form', i, kw)
    return pre


# ---- softmax and decode ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('R', [1, 7, 300])
@pytest.mark.parametrize('num_classes', NC_ALL)
def test_decode_probs_against_float64(num_classes, R):
    """N = 3: n is odd at R = 1, 7 (the lanes kernel's last wave half empty).  ld = num_classes + 4 and + 11 with NaN in the
    pad columns: never read, so the same bits and no bad flag.  1e-6 on the probabilities: the bound of the scores in
    test_gpu_proposals.py; boxes 1e-6 * max(1, |ref|)."""
    from xdet import ops
    rois, cls_reg, _ = T.random_logits(3, R, num_classes, 3.0)
    ref_b, ref_p = T.reference_decode_probs(rois.reshape(-1, 4), cls_reg, num_classes)
    ref_p = T.class_major(ref_p, R)
    boxes, probs, bad = ops.head_decode_probs(rois, cls_reg, num_classes, R)
    assert boxes.shape == (3 * R, 4) and probs.shape == (3, num_classes, R) and bad.tolist() == [0, 0, 0]
    perr = np.abs(probs - ref_p).max()
    berr = (np.abs(boxes - ref_b) / np.maximum(1.0, np.abs(ref_b))).max()
    print('head_decode_probs nc=%d R=%d: probs err %.3g, boxes err %.3g' % (num_classes, R, perr, berr))
    assert perr <= 1e-6
    assert berr <= 1e-6
    boxes2, probs2, bad2 = ops.head_decode_probs(rois, _pad_nan(cls_reg, 7), num_classes, R)
    assert _same_bits(boxes2, boxes) and _same_bits(probs2, probs) and bad2.tolist() == [0, 0, 0]
    assert np.isfinite(probs2).all() and np.isfinite(boxes2).all()


@pytest.mark.parametrize('R', [7, 300])
@pytest.mark.parametrize('num_classes', [2, 21, 28])
def test_lanes_kernel_equals_thread_kernel(num_classes, R):
    """32 lanes per ROI (form 0 at num_classes + 4 <= 32) against one thread per ROI (form 1): "the same bits" (detect.hip)"""
    from xdet import ops
    rois, cls_reg, _ = T.random_logits(3, R, num_classes, 3.0)
    for extra in (0, 7):
        a = ops.head_decode_probs(rois, _pad_nan(cls_reg, extra), num_classes, R, form=0)
        b = ops.head_decode_probs(rois, _pad_nan(cls_reg, extra), num_classes, R, form=1)
        assert _same_bits(a[0], b[0]) and _same_bits(a[1], b[1]) and np.array_equal(a[2], b[2])


@pytest.mark.parametrize('num_classes', NC_ALL)
def test_probabilities_form_equals_logits_form(num_classes):
    """decode + probabilities + bboxes_eval from them (the net) == ext_decode_rois + bboxes_eval from the logits (the op form),
    detections bit for bit; a batched call == per-image calls"""
    from xdet import ops
    R = 300
    rois, cls_reg, logits = T.random_logits(3, R, num_classes, 3.0)
    boxes, probs, bad = ops.head_decode_probs(rois, cls_reg, num_classes, R)
    pre = ops.bboxes_eval_from_probs(probs, boxes, bad=bad)
    dec = ops.ext_decode_rois(rois, cls_reg[:, num_classes:].reshape(3, R, 4))
    assert _same_bits(dec.reshape(-1, 4), boxes)
    raw = ops.bboxes_eval(logits, dec, num_classes=num_classes)
    n_det = 0
    for i in range(3):
        assert _same_dets(pre[i], raw[i]), i
        b1, p1, bad1 = ops.head_decode_probs(rois[i], cls_reg[i * R:(i + 1) * R], num_classes, R)
        assert _same_bits(b1, boxes[i * R:(i + 1) * R]) and _same_bits(p1[0], probs[i])
        assert _same_dets(ops.bboxes_eval_from_probs(p1[0], b1), pre[i]), i
        n_det += sum(int((pre[i][c][0] > 0).sum()) for c in range(1, num_classes))
    assert n_det > 0


def test_lanes_kernel_grid_stride():
    """n = 129 * 1024 ROIs at 21 classes: 16512 workgroups wanted, 16384 launched: the last 1024 ROIs (image 128) are a second
    trip of the loop.  They, and images on both sides of the seam, equal the same rows computed on their own."""
    from xdet import ops
    R, nc, N = 1024, 21, 129
    rng = np.random.default_rng(129)
    cls_reg = rng.standard_normal((N * R, nc + 4), dtype=f32)
    cls_reg[:, nc:] *= f32(0.2)
    rois = np.tile(T.random_logits(1, R, nc, 3.0)[0][0], (N, 1))
    boxes, probs, bad = ops.head_decode_probs(rois, cls_reg, nc, R)
    assert not bad.any()
    for i in (0, 127, 128):
        b1, p1, _ = ops.head_decode_probs(rois[i * R:(i + 1) * R], cls_reg[i * R:(i + 1) * R], nc, R)
        assert _same_bits(b1, boxes[i * R:(i + 1) * R]) and _same_bits(p1[0], probs[i]), i


def test_thread_kernel_grid_stride():
    """n = 2048 * 256 + 300 ROIs at 33 classes: the last 300 are a second trip of the thread-per-ROI kernel's loop.  The input
    is a block of 4 images of 419 ROIs repeated 313 times: the whole output is the block's, repeated."""
    from xdet import ops
    R, nc, rep = 419, 33, 313
    rois, cls_reg, _ = T.random_logits(4, R, nc, 3.0)
    assert 4 * R * rep == 2048 * 256 + 300
    boxes, probs, bad = ops.head_decode_probs(np.tile(rois.reshape(-1, 4), (rep, 1)), np.tile(cls_reg, (rep, 1)), nc, R)
    b1, p1, _ = ops.head_decode_probs(rois, cls_reg, nc, R)
    assert not bad.any() and np.isfinite(p1).all()
    assert _same_bits(boxes[-4 * R:], b1) and _same_bits(probs[-4:], p1)          # the rows behind the cap
    assert _same_bits(boxes, np.tile(b1, (rep, 1))) and _same_bits(probs, np.tile(p1, (rep, 1, 1)))


# ---- bboxes_eval: ties, valid-count boundaries, settings -------------------------------------------------------------------

@pytest.mark.parametrize('nms_thr', [0.0, 0.3, 1.0])
@pytest.mark.parametrize('nms_topk', [1, 3, 200, 256])
def test_banded_ties_and_valid_counts(nms_topk, nms_thr, oracle):
    """valid ROIs per class 0, 1, 2, 63 .. 1024 (the 64-candidate blocks, 2 * nms_topk +- 1, 512 | 513: rank counting | bitonic
    sort), scores in exact ties of hundreds: "lower ROI index first" in both orderings, the cut at 2 * nms_topk inside a tie"""
    logits, boxes = T.banded()
    kw = dict(nms_threshold=nms_thr, nms_topk=nms_topk)
    got = _both_forms(logits, boxes, 1024, **kw)[0]
    ref = oracle.bboxes_eval(logits, boxes, **kw)
    _vs_oracle(got, ref, 21, nms_topk, kw)


@pytest.mark.parametrize('thr', T.LATTICE_THRESHOLDS + [np.nextafter(f32(0.25), f32(0)), np.nextafter(f32(0.5), f32(0))])
def test_lattice_iou_at_the_threshold(thr, oracle):
    """pairs with IoU == thr exactly (not suppressed) and, at the two thresholds one ulp below 1/4 and 1/2, one ulp above it
    (suppressed): both inside the 1e-5 band in which nms_pairs.h redoes a lane's pairs with the reference's expression.  At
    equality the product test alone happens to decide as the reference does; one ulp above it does not (without the band's
    second pass class 1 keeps 83 detections for the oracle's 53), so the last two thresholds are the ones that need it."""
    logits, boxes = T.lattice()
    got = _both_forms(logits, boxes, 256, nms_threshold=float(thr))[0]
    ref = oracle.bboxes_eval(logits, boxes, nms_threshold=thr)
    _vs_oracle(got, ref, 21, 200, thr)


def test_more_than_512_valid_rois_per_class(oracle):
    """flat logits at R = 1000: every class has more than 512 valid ROIs: the bitonic sort, in the probabilities form"""
    from xdet import ops
    rois, cls_reg, logits = T.random_logits(3, 1000, 21, 0.7)
    boxes = ops.ext_decode_rois(rois, cls_reg[:, 21:].reshape(3, 1000, 4))
    got = _both_forms(logits.reshape(-1, 21), boxes.reshape(-1, 4), 1000)
    for i in range(3):
        _vs_oracle(got[i], oracle.bboxes_eval(logits[i], boxes[i]), 21, 200, i)


def test_select_threshold_at_equality():
    """two classes with equal logits: p = 0.5 exactly.  `score > select_threshold`: 0.5 selects nothing, the float32 below 0.5
    everything (70 ROIs, nms_threshold 1: none suppressed)"""
    R = 70
    rng = np.random.default_rng(70)
    boxes = T.clustered_boxes(rng, 1, R, inside=True)[0]
    logits = np.zeros((R, 2), f32)
    kw = dict(nms_threshold=1.0, nms_topk=256)
    none = _both_forms(logits, boxes, R, select_threshold=0.5, **kw)[0]
    assert not none[1][0].any() and not none[1][1].any()
    below = np.nextafter(f32(0.5), f32(0))
    every = _both_forms(logits, boxes, R, select_threshold=float(below), **kw)[0]
    assert below < 0.5 and np.array_equal(every[1][0][:R], np.full(R, 0.5, f32)) and not every[1][0][R:].any()
    assert _same_bits(every[1][1][:R], boxes)              # all tied: ROI order


def test_bbox_img_and_image_shape(oracle):
    """frames other than [0,0,1,1] (one inside, one around the unit square) and raw image shapes other than the net's: per
    image in one batched call, both forms"""
    from xdet import ops
    rois, cls_reg, logits = T.random_logits(3, 300, 21, 3.0)
    boxes = ops.ext_decode_rois(rois, cls_reg[:, 21:].reshape(3, 300, 4))
    frames = np.array([[0, 0, 1, 1], [0.1, 0, 0.9, 1], [-0.2, -0.1, 1.2, 1.1]], f32)
    shapes = np.array([[333, 500], [480, 480], [500, 333]], np.int32)
    got = _both_forms(logits.reshape(-1, 21), boxes.reshape(-1, 4), 300, image_shape=shapes, bbox_img=frames)
    n_det = 0
    for i in range(3):
        ref = oracle.bboxes_eval(logits[i], boxes[i], tuple(shapes[i]), frames[i])
        _vs_oracle(got[i], ref, 21, 200, i, unit_frame=(i == 0))
        n_det += sum(int((ref[c][0] > 0).sum()) for c in range(1, 21))
    assert n_det > 100


# ---- non-finite head outputs -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize('num_classes,form', [(21, 0), (21, 1), (29, 0), (33, 0)])
def test_bad_flag_marks_the_image_of_the_bad_logit(num_classes, form):
    from xdet import ops
    R = 64
    rois, cls_reg, _ = T.random_logits(3, R, num_classes, 3.0)
    boxes, probs, bad = ops.head_decode_probs(rois, cls_reg, num_classes, R, form=form)
    clean = ops.bboxes_eval_from_probs(probs, boxes, bad=bad)
    assert bad.tolist() == [0, 0, 0] and all(np.isfinite(clean[i][c][0]).all() for i in range(3) for c in range(1, num_classes))
    for value in (np.nan, np.inf, -np.inf):
        x = cls_reg.copy()
        x[R + 17, min(5, num_classes - 1)] = value
        b2, p2, bad2 = ops.head_decode_probs(rois, x, num_classes, R, form=form)
        assert bad2.tolist() == [0, 1, 0], value
        got = ops.bboxes_eval_from_probs(p2, b2, bad=bad2)
        assert all(np.isnan(got[1][c][0][0]) for c in range(1, num_classes)), value
        assert _same_dets(got[0], clean[0]) and _same_dets(got[2], clean[2]), value
        assert _same_bits(p2[[0, 2]], probs[[0, 2]]) and _same_bits(b2, boxes)


def _nan_box_case(num_classes=21, R=64):
    rois, cls_reg, _ = T.random_logits(3, R, num_classes, 3.0)
    x = cls_reg.copy()
    x[R + 9, :num_classes] = 0                    # ROI 9 of image 1: p = 1/21 in every class, above the 0.01 of every class
    return rois, x


@pytest.mark.parametrize('column', [0, 1, 2, 3])
def test_nan_regression_value_is_dropped_and_loud(column, oracle):
    """A NaN regression value makes a NaN box.  The reference's clip keeps the NaN (tf.maximum) and filter_boxes drops the box;
    fmaxf / fminf would turn it into the frame's edge and the ROI into a full-frame detection.  The ROI is no detection, and
    its image is marked as for a non-finite logit (NaN in slot 0 of the classes that selected the ROI: here all), in both
    forms; the other images keep their bits."""
    from xdet import ops
    nc, R = 21, 64
    rois, x = _nan_box_case(nc, R)
    boxes, probs, bad = ops.head_decode_probs(rois, x, nc, R)
    clean = ops.bboxes_eval_from_probs(probs, boxes, bad=bad)
    x = x.copy()
    x[R + 9, nc + column] = np.nan
    b2, p2, bad2 = ops.head_decode_probs(rois, x, nc, R)
    assert bad2.tolist() == [0, 0, 0] and _same_bits(p2, probs) and np.isnan(b2[R + 9]).any()
    logits = np.ascontiguousarray(x[:, :nc]).reshape(3, R, nc)
    with np.errstate(invalid='ignore'):
        ref = oracle.bboxes_eval(logits[1], b2[R:2 * R])
    for got in (ops.bboxes_eval_from_probs(p2, b2, bad=bad2), ops.bboxes_eval(logits, b2.reshape(3, R, 4))):
        _vs_oracle(got[1], ref, nc, 200, column, first_is_nan=True)
        assert all(np.isfinite(got[1][c][1]).all() and np.isfinite(got[1][c][0][1:]).all() for c in range(1, nc))
        assert _same_dets(got[0], clean[0]) and _same_dets(got[2], clean[2])


@pytest.mark.parametrize('value', [np.inf, -np.inf])
def test_infinite_regression_values_clip_to_the_frame(value, oracle):
    """+-inf in a regression value gives +-inf corners, no NaN: they clip to the frame as in the reference, nothing is marked"""
    from xdet import ops
    nc, R = 21, 64
    rois, x = _nan_box_case(nc, R)
    logits = np.ascontiguousarray(x[:, :nc]).reshape(3, R, nc)
    for column in range(4):
        y = x.copy()
        y[R + 9, nc + column] = value
        y[R + 30, nc + column] = value             # (and a ROI that only some classes select)
        with np.errstate(invalid='ignore', over='ignore'):
            b2, p2, bad2 = ops.head_decode_probs(rois, y, nc, R)
            assert not np.isnan(b2).any() and np.isinf(b2[R + 9]).any() == (not (column >= 2 and value < 0))
            ref = oracle.bboxes_eval(logits[1], b2[R:2 * R])
        for got in (ops.bboxes_eval_from_probs(p2, b2, bad=bad2), ops.bboxes_eval(logits, b2.reshape(3, R, 4))):
            _vs_oracle(got[1], ref, nc, 200, (value, column))


# ---- the entry points run what the net runs --------------------------------------------------------------------------------

def test_entry_points_equal_the_net(lh_weights):
    from xdet import ops
    from xdet import weights as W
    from xdet.model import LightHeadDetector
    from xdet.runtime import to_host
    det = LightHeadDetector(lh_weights, image_size=256, max_batch=2, rpn_post_nms_top_n=50)
    det.forward(W.synthetic_images(2, 256, seed=3))
    s, b = det.detections(2)
    proposals = det.flat('proposals', (2, 50, 4))
    t = det.buffer('cls_reg', 2)
    cls_reg = to_host(t.ptr, (100, t.ld))
    assert t.ld > 25
    boxes, probs, bad = ops.head_decode_probs(proposals, cls_reg, 21, 50)
    assert _same_bits(boxes, det.flat('head_boxes', (100, 4))) and not bad.any()
    got = ops.bboxes_eval_from_probs(probs, boxes, (256, 256), train_image_size=256, bad=bad)
    assert (s > 0).sum() > 0
    for i in range(2):
        for c in range(1, 21):
            assert _same_bits(got[i][c][0], s[i, c - 1]) and _same_bits(got[i][c][1], b[i, c - 1]), (i, c)


# ---- argument errors -------------------------------------------------------------------------------------------------------

def test_head_decode_probs_argument_errors():
    from xdet import ops, InvalidArgumentError
    from xdet._lib import lib, check
    from xdet.runtime import DeviceBuffer
    nc, R, n = 21, 4, 8
    rois = np.tile(np.array([0.1, 0.1, 0.5, 0.5], f32), (n, 1))
    cls_reg = np.zeros((n, nc + 4), f32)
    ops.head_decode_probs(rois, cls_reg, nc, R)                                   # fine
    with pytest.raises(InvalidArgumentError):
        ops.head_decode_probs(rois[:1], cls_reg[:1, :5], 1, 1)                    # num_classes < 2
    with pytest.raises(InvalidArgumentError):
        ops.head_decode_probs(rois, cls_reg, nc, 0)                               # R < 1
    with pytest.raises(InvalidArgumentError):
        ops.head_decode_probs(rois, cls_reg, nc, 3)                               # n % R != 0
    with pytest.raises(InvalidArgumentError):
        ops.head_decode_probs(rois, cls_reg[:, :nc + 3], nc, R)                   # ld < num_classes + 4
    for form in (-1, 2):
        with pytest.raises(InvalidArgumentError):
            ops.head_decode_probs(rois, cls_reg, nc, R, form=form)
    buf = [DeviceBuffer(4096, zero=True) for _ in range(5)]
    p = [x.ptr for x in buf]

    def call(rois, cls_reg, boxes, probs, bad, n=n):
        check(lib().xdet_head_decode_probs(rois, cls_reg, nc + 4, nc, R, n, 0, boxes, probs, bad, None))
    call(*p)                                                                      # fine
    for k in range(5):                                                            # NULL
        with pytest.raises(InvalidArgumentError):
            call(*[None if j == k else p[j] for j in range(5)])
    for k in (0, 2):                                                              # rois / boxes off the 16-byte grid
        with pytest.raises(InvalidArgumentError):
            call(*[p[j] + 4 if j == k else p[j] for j in range(5)])
    with pytest.raises(InvalidArgumentError):
        call(*p, n=-4)                                                            # n < 0
    call(*p, n=0)                                                                 # nothing to do: fine


def test_bboxes_eval_probs_argument_errors():
    from xdet import ops, InvalidArgumentError
    from xdet._lib import lib, check
    from xdet.runtime import DeviceBuffer
    boxes = np.tile(np.array([0.1, 0.1, 0.5, 0.5], f32), (4, 1))
    probs = np.full((1, 3, 4), 1.0 / 3, f32)
    ops.bboxes_eval_from_probs(probs, boxes)                                      # fine
    for kw in (dict(nms_topk=0), dict(nms_topk=257), dict(nms_threshold=-0.1)):
        with pytest.raises(InvalidArgumentError):
            ops.bboxes_eval_from_probs(probs, boxes, **kw)
    with pytest.raises(InvalidArgumentError):
        ops.bboxes_eval_from_probs(np.ones((1, 1, 4), f32), boxes)                # num_classes = 1
    with pytest.raises(InvalidArgumentError):
        ops.bboxes_eval_from_probs(np.full((1, 2, 1025), 0.5, f32), np.tile(boxes[:1], (1025, 1)))     # R = 1025
    buf = [DeviceBuffer(4096, zero=True) for _ in range(6)]
    p = [x.ptr for x in buf]

    def call(probs, boxes, shapes, frame, scores, out_boxes, bad=None):
        check(lib().xdet_bboxes_eval_probs(probs, boxes, 1, 4, 3, shapes, frame, 480, 480, 0.01, 0.3, 8, bad, scores, out_boxes,
                                           None))
    for k in range(6):
        with pytest.raises(InvalidArgumentError):
            call(*[None if j == k else p[j] for j in range(6)])
