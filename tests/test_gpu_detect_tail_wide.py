"""The detection tail beyond 1024 ROIs per image (csrc/detect.hip bboxes_eval_wide_kernel) through its doors
xdet_bboxes_eval_probs_wide (ops.bboxes_eval_from_probs(..., wide=True): the narrow kernel up to 1024 ROIs, the wide one above)
and xdet_bboxes_eval_probs_wide_only (wide='force': the wide kernel at any R).

Two yardsticks.  Up to 1024 ROIs the existing kernel: the wide one on the same input gives the same bits (they share the
per-ROI front and everything behind the order; what differs is where the keys and the winners' boxes live).  Beyond, the
oracle, with the criteria of tests/test_gpu_detect_tail.py (_vs_oracle: equal positive counts per class, scores and boxes
within 1e-6), on inputs whose cut at 2 * nms_topk lies inside exact ties that span rows 1024 and 2048.  The inputs and what each
is for: tests/detect_tail_wide_cases.py; that they have those properties: tests/test_detect_tail_wide_math.py.
One image x at most 20 workgroups per launch, except the three-image batch."""
import numpy as np
import pytest

import detect_tail_cases as T
import detect_tail_wide_cases as TW
from test_gpu_detect_tail import _same_bits, _same_dets, _vs_oracle, _probs_of

pytestmark = pytest.mark.gpu

f32 = np.float32
GRID = [(thr, topk) for thr in (0.0, 0.3, 1.0) for topk in (1, 3, 200, 256)]


def _tail(probs, boxes, wide, **kw):
    from xdet import ops
    return ops.bboxes_eval_from_probs(probs, boxes, wide=wide, **kw)


def _n_dets(d):
    return sum(int((s > 0).sum()) for s, _ in d.values())


# ---- the wide kernel against the narrow one ----------------------------------------------------------------------------------

@pytest.mark.parametrize('R', [1, 7, 300, 1000, 1024])
def test_wide_equals_narrow_bit_for_bit(R):
    """random logits at spread 0.7 (at R = 1000, 1024 every class has more than 512 valid ROIs: both sort) and 3.0 (rank
    counting), and the banded ties at every (nms_threshold, nms_topk) of the narrow form's own test; the wide door at these R
    launches the narrow kernel, and gives its bits too"""
    from xdet import ops
    n = 0
    for spread in (0.7, 3.0):
        rois, cls_reg, _ = T.random_logits(1, R, 21, spread)
        boxes, probs, bad = ops.head_decode_probs(rois, cls_reg, 21, R)
        narrow = _tail(probs, boxes, False, bad=bad)
        assert _same_dets(_tail(probs, boxes, 'force', bad=bad)[0], narrow[0]), spread
        assert _same_dets(_tail(probs, boxes, True, bad=bad)[0], narrow[0]), spread
        n += _n_dets(narrow[0])
    logits, boxes = T.banded(R)
    probs = _probs_of(logits, R)
    for thr, topk in GRID:
        kw = dict(nms_threshold=thr, nms_topk=topk)
        narrow = _tail(probs, boxes, False, **kw)
        assert _same_dets(_tail(probs, boxes, 'force', **kw)[0], narrow[0]), kw
        n += _n_dets(narrow[0])
    assert n > 0


# ---- beyond 1024 ROIs: the oracle ------------------------------------------------------------------------------------------

@pytest.mark.parametrize('flipped', [False, True])
@pytest.mark.parametrize('name', ['r1800', 'r2049', 'r6144'])
def test_banded_cases_against_the_oracle(name, flipped, oracle):
    """valid ROIs per class from 0 to R across 512 | 513, 1024 | 1025, 2048 | 2049, 4096 | 4097 (rank counting, and a sort of
    1024, 2048, 4096, 8192 slots), in 2048, 4096 and 8192 key slots; flipped: every winner at r >= 1024, its box read again
    from global memory"""
    logits, boxes, V = TW.case(name, flipped)
    R, nc = logits.shape[0], len(V) + 1
    probs = _probs_of(logits, R)
    for thr, topk in TW.SETTINGS:
        kw = dict(nms_threshold=thr, nms_topk=topk)
        got = _tail(probs, boxes, True, **kw)[0]
        ref = oracle.bboxes_eval(logits, boxes, num_classes=nc, **kw)
        _vs_oracle(got, ref, nc, topk, (name, flipped, kw))
        if R <= 2048:
            assert _same_dets(_tail(probs, boxes, 'force', **kw)[0], got)      # (above 1024 ROIs the door is the wide kernel)


def test_prefix_case_equals_the_narrow_kernel_on_its_first_1024_rows():
    """no row >= 1024 is valid: the wide kernel on 1800 rows == the narrow kernel on rows 0 .. 1023, bit for bit"""
    logits, boxes, V = TW.case('prefix')
    wide_p, narrow_p = _probs_of(logits, 1800), _probs_of(np.ascontiguousarray(logits[:1024]), 1024)
    assert _same_bits(wide_p[:, :, :1024], narrow_p)
    n = 0
    for thr, topk in TW.SETTINGS:
        kw = dict(nms_threshold=thr, nms_topk=topk)
        wide = _tail(wide_p, boxes, True, **kw)[0]
        assert _same_dets(wide, _tail(narrow_p, boxes[:1024], False, **kw)[0]), kw
        n += _n_dets(wide)
    assert n > 0


@pytest.fixture(scope='module')
def flat3():
    """random_logits(3, 1800, 21, 0.7): about 1740 valid ROIs in every class of every image -> (logits, boxes, probs, bad)"""
    from xdet import ops
    rois, cls_reg, logits = T.random_logits(3, 1800, 21, 0.7)
    boxes, probs, bad = ops.head_decode_probs(rois, cls_reg, 21, 1800)
    assert not bad.any()
    return logits, boxes.reshape(3, 1800, 4), probs, bad


def test_batched_equals_per_image_and_the_oracle(flat3, oracle):
    logits, boxes, probs, bad = flat3
    got = _tail(probs, boxes, True, bad=bad)
    for i in range(3):
        assert _same_dets(_tail(probs[i], boxes[i], True), got[i]), i                    # (2-D probabilities: one image)
        _vs_oracle(got[i], oracle.bboxes_eval(logits[i], boxes[i]), 21, 200, i)
        assert _n_dets(got[i]) > 100


def test_bbox_img_and_image_shape(flat3, oracle):
    """the three frames and raw image shapes of the narrow form's test, per image in one batched call"""
    logits, boxes, probs, bad = flat3
    frames = np.array([[0, 0, 1, 1], [0.1, 0, 0.9, 1], [-0.2, -0.1, 1.2, 1.1]], f32)
    shapes = np.array([[333, 500], [480, 480], [500, 333]], np.int32)
    got = _tail(probs, boxes, True, image_shape=shapes, bbox_img=frames, bad=bad)
    n = 0
    for i in range(3):
        ref = oracle.bboxes_eval(logits[i], boxes[i], tuple(shapes[i]), frames[i])
        _vs_oracle(got[i], ref, 21, 200, i, unit_frame=(i == 0))
        n += _n_dets(ref)
    assert n > 100


def test_two_runs_give_equal_bits(flat3):
    logits, boxes, probs, bad = flat3
    a, b = _tail(probs, boxes, True, bad=bad), _tail(probs, boxes, True, bad=bad)
    assert all(_same_dets(a[i], b[i]) for i in range(3))
    lg, bx, V = TW.case('r6144', True)
    p = _probs_of(lg, 6144)
    assert _same_dets(_tail(p, bx, True)[0], _tail(p, bx, True)[0])


# ---- non-finite inputs at a row beyond 1024 ----------------------------------------------------------------------------------

def test_non_finite_inputs_at_row_1500(oracle):
    """image 1, ROI 1500 (p = 1/21 in every class: every class selects it).  A NaN logit sets the image's bad flag; a NaN
    regression value makes a NaN box, which is no detection and as loud: NaN in slot 0 of every class of image 1, the rest of
    it as the oracle's, and the other images keep their bits"""
    from xdet import ops
    nc, R, row = 21, 1800, 1500
    rois, cls_reg, _ = T.random_logits(3, R, nc, 0.7)
    x = cls_reg.copy()
    x[R + row, :nc] = 0
    boxes, probs, bad = ops.head_decode_probs(rois, x, nc, R)
    clean = _tail(probs, boxes, True, bad=bad)
    assert bad.tolist() == [0, 0, 0] and all(np.isfinite(clean[i][c][0]).all() for i in range(3) for c in range(1, nc))
    y = x.copy()
    y[R + row, 5] = np.nan
    b2, p2, bad2 = ops.head_decode_probs(rois, y, nc, R)
    assert bad2.tolist() == [0, 1, 0]
    got = _tail(p2, b2, True, bad=bad2)
    assert all(np.isnan(got[1][c][0][0]) for c in range(1, nc))
    assert _same_dets(got[0], clean[0]) and _same_dets(got[2], clean[2])
    y = x.copy()
    y[R + row, nc + 2] = np.nan
    b2, p2, bad2 = ops.head_decode_probs(rois, y, nc, R)
    assert bad2.tolist() == [0, 0, 0] and _same_bits(p2, probs) and np.isnan(b2[R + row]).any()
    got = _tail(p2, b2, True, bad=bad2)
    logits = np.ascontiguousarray(y[:, :nc]).reshape(3, R, nc)
    with np.errstate(invalid='ignore'):
        ref = oracle.bboxes_eval(logits[1], b2[R:2 * R])
    _vs_oracle(got[1], ref, nc, 200, 'nan box', first_is_nan=True)
    assert all(np.isfinite(got[1][c][1]).all() and np.isfinite(got[1][c][0][1:]).all() for c in range(1, nc))
    assert _same_dets(got[0], clean[0]) and _same_dets(got[2], clean[2])


# ---- limits ------------------------------------------------------------------------------------------------------------------

def test_limits():
    from xdet import InvalidArgumentError
    box = np.array([[0.1, 0.1, 0.5, 0.5]], f32)
    for wide in (True, 'force'):
        got = _tail(np.full((1, 2, 6144), 0.5, f32), np.tile(box, (6144, 1)), wide, nms_threshold=1.0, nms_topk=256)[0]
        assert np.array_equal(got[1][0], np.full(256, 0.5, f32)) and _same_bits(got[1][1], np.tile(box, (256, 1)))
        with pytest.raises(InvalidArgumentError, match='1 <= rois per image <= 6144'):
            _tail(np.full((1, 2, 6145), 0.5, f32), np.tile(box, (6145, 1)), wide)
        for kw in (dict(nms_topk=0), dict(nms_topk=257), dict(nms_threshold=-0.1)):
            with pytest.raises(InvalidArgumentError):
                _tail(np.full((1, 2, 1800), 0.5, f32), np.tile(box, (1800, 1)), wide, **kw)
        with pytest.raises(InvalidArgumentError):
            _tail(np.ones((1, 1, 1800), f32), np.tile(box, (1800, 1)), wide)              # num_classes = 1
    with pytest.raises(InvalidArgumentError, match='1 <= rois per image <= 1024'):
        _tail(np.full((1, 2, 1025), 0.5, f32), np.tile(box, (1025, 1)), False)             # the default door as ever
