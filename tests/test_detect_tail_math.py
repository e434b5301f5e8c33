"""tests/detect_tail_cases.py on the CPU: each input of tests/test_gpu_detect_tail.py has the property it is named for (float64
NumPy and the oracle), and the float64 statement of the decode + softmax pass agrees with the oracle's float32 one."""
import numpy as np
import pytest

import detect_tail_cases as T

f32 = np.float32


def _valid_counts(oracle, logits, boxes, image_shape=(480, 480), thr=0.01):
    """float64 probabilities, the oracle's clip and filter -> valid ROIs per class [num_classes - 1]"""
    _, p = T.reference_decode_probs(np.zeros((logits.shape[0], 4)), np.concatenate([logits, np.zeros((logits.shape[0], 4), f32)], 1),
                                    logits.shape[1])
    keep = oracle._center_filter_mask(oracle.bboxes_clip([0, 0, 1, 1], boxes), oracle.filter_min_size(image_shape))
    return np.array([int(((p[:, c] > thr) & keep).sum()) for c in range(1, logits.shape[1])])


def test_banded_valid_counts_and_ties(oracle):
    logits, boxes = T.banded()
    assert logits.shape == (1024, 21) and boxes.shape == (1024, 4)
    # strictly inside the frame, and every box passes filter_boxes at 480 x 480 (min_size 0.03)
    assert boxes.min() > 0 and boxes.max() < 1
    assert (boxes[:, 2:] - boxes[:, :2]).min() > 0.05
    assert oracle._center_filter_mask(oracle.bboxes_clip([0, 0, 1, 1], boxes), oracle.filter_min_size((480, 480))).all()
    assert _valid_counts(oracle, logits, boxes).tolist() == T.V_BANDED
    # exact ties, in the float32 values every implementation computes (rows of one band are the same row)
    prob = oracle.softmax(logits)
    tied = 0
    for c in range(1, 21):
        s = prob[:T.V_BANDED[c - 1], c]
        distinct = len(np.unique(s))
        assert distinct <= c - 1 or s.size == 0
        tied += distinct < s.size
    assert tied >= 15


@pytest.mark.parametrize('nms_topk,nms_thr', [(3, 0.3), (1, 1.0), (3, 1.0), (200, 1.0), (256, 1.0), (200, 0.3)])
def test_banded_reaches_the_nms_topk_cap(oracle, nms_topk, nms_thr):
    logits, boxes = T.banded()
    ref = oracle.bboxes_eval(logits, boxes, (480, 480), nms_threshold=nms_thr, nms_topk=nms_topk)
    kept = [int((ref[c][0] > 0).sum()) for c in range(1, 21)]
    assert all(k <= min(v, nms_topk) for k, v in zip(kept, T.V_BANDED))
    if nms_thr == 1.0:                     # IoU > 1 never: the first nms_topk of the sorted candidates
        assert kept == [min(v, nms_topk) for v in T.V_BANDED]
    if (nms_topk, nms_thr) != (200, 0.3):
        assert max(kept) == nms_topk
    else:                                  # the default setting is suppression-bound: the cap is not what ends the walk
        assert 0 < max(kept) < nms_topk


def _walk(oracle, boxes, scores, max_output, thr):
    """oracle.non_max_suppression with a record of the pairs it compares: -> (selected, [(candidate, kept box, IoU)] of the
    comparisons of every visited candidate)"""
    order = np.argsort(-scores.astype(f32), kind='stable')
    sel, seen = [], []
    for i in order:
        if len(sel) >= max_output:
            break
        if sel:
            iou = oracle._iou_row(boxes, i, np.array(sel))
            seen.append((int(i), list(sel), iou))
            if np.any(iou > f32(thr)):
                continue
        sel.append(int(i))
    return np.array(sel, np.int64), seen


def _lattice_class_inputs(oracle, c):
    """what oracle.bboxes_eval hands to non_max_suppression for class c of the lattice (bbox_img = the frame: no resize)"""
    logits, boxes = T.lattice()
    s = oracle.softmax(logits)[:, c]
    m = (s > f32(0.01)).astype(f32)
    s, b = s * m, oracle.bboxes_clip([0, 0, 1, 1], boxes * m[:, None])
    keep = oracle._center_filter_mask(b, oracle.filter_min_size((480, 480)))
    s, b = oracle._pad_rows(s[keep], 100), oracle._pad_rows(b[keep], 100)
    s, idx = oracle.top_k(s, min(s.shape[0], 400))
    return s, b[idx]


def test_lattice_meets_iou_equal_to_the_threshold(oracle):
    logits, boxes = T.lattice()
    counts = _valid_counts(oracle, logits, boxes)
    assert counts.min() >= 90 and counts.max() <= 100
    prob = oracle.softmax(logits)
    for c in range(1, 21):
        s = prob[:, c][prob[:, c] > 0.01]
        assert len(np.unique(s)) == s.size                                   # distinct scores: the order is the scores'
    below = [np.nextafter(f32(0.25), f32(0)), np.nextafter(f32(0.5), f32(0))]
    for thr in T.LATTICE_THRESHOLDS + below:
        at_thr = decisive = 0
        for c in range(1, 21):
            s, b = _lattice_class_inputs(oracle, c)
            sel, seen = _walk(oracle, b, s, 200, thr)
            assert np.array_equal(sel, oracle.non_max_suppression(b, s, 200, thr))
            for i, kept, iou in seen:
                if s[i] <= 0:
                    continue
                if thr in below:
                    # IoU one ulp above the threshold: the only thing that suppresses this candidate
                    hit = iou == np.nextafter(thr, f32(1))
                    at_thr += int(hit.sum())
                    decisive += bool(hit.any() and not np.any(iou[~hit] > thr))
                else:
                    hit = iou == thr
                    at_thr += int(hit.sum())
                    decisive += bool(hit.any() and not np.any(iou > thr))   # kept BECAUSE equality does not suppress
        assert at_thr > 0 and decisive > 0, (thr, at_thr, decisive)


@pytest.mark.parametrize('num_classes,spread', [(21, 3.0), (81, 6.0), (2, 3.0), (33, 3.0)])
def test_reference_decode_probs_against_the_oracle(oracle, num_classes, spread):
    rois, cls_reg, logits = T.random_logits(3, 300, num_classes, spread)
    boxes, probs = T.reference_decode_probs(rois.reshape(-1, 4), cls_reg, num_classes)
    ob = oracle.ext_decode_rois(rois.reshape(-1, 4), cls_reg[:, num_classes:])
    assert np.abs(boxes - ob).max() <= 1e-6 * max(1.0, np.abs(boxes).max())
    assert np.abs(probs.sum(1) - 1).max() < 1e-12
    # The kernels' float32 operation sequence against float64 must fit inside the 1e-6 that the GPU test asserts, or no correct
    # kernel could pass it.  Measured: 2.8e-7 (21 classes x 3 sigma), 3.2e-7 (33 x 3), 7.1e-7 (81 x 6): the sum is sequential, 80
    # additions at 81 classes, each rounding a partial sum in [1, 2) to 1.2e-7, and a probability near 1 carries them in full.
    err = np.abs(T.f32_restatement_probs(logits.reshape(-1, num_classes)) - probs).max()
    print('f32 restatement vs float64: %d classes x %g sigma: %.3g' % (num_classes, spread, err))
    assert err <= 1e-6, err
    assert np.abs(oracle.softmax(logits.reshape(-1, num_classes)) - probs).max() <= 1e-6
    cm = T.class_major(probs, 300)
    assert cm.shape == (3, num_classes, 300) and cm[2, num_classes - 1, 17] == probs[2 * 300 + 17, num_classes - 1]


def test_random_logits_flat_case_needs_the_bitonic_sort(oracle):
    rois, cls_reg, logits = T.random_logits(3, 1000, 21, 0.7)
    boxes = oracle.ext_decode_rois(rois.reshape(-1, 4), cls_reg[:, 21:]).reshape(3, 1000, 4)
    for i in range(3):
        counts = _valid_counts(oracle, logits[i], boxes[i])
        assert counts.min() > 512, counts
