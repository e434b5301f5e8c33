"""The scoring half of bboxes_eval on the GPU (csrc/evalmatch.hip): xdet_bboxes_matching against
evaluation.bboxes_matching flag for flag, the streaming accumulator against the host StreamingTpFp whatever the batching
and sharding, overflow, bad images, and LightHeadDetector.evaluate_images end to end."""
import os

import numpy as np
import pytest

import eval_matching_cases as M

pytestmark = pytest.mark.gpu

NET_S = 256          # as tests/test_gpu_ingest.py: a small network input


def host_flags(scores, boxes, gts, thr=M.THR):
    from xdet import evaluation as E
    N, C, K = scores.shape
    nb, tp, fp = np.zeros((N, C), np.int32), np.zeros((N, C, K), bool), np.zeros((N, C, K), bool)
    for n in range(N):
        for c in range(C):
            nb[n, c], tp[n, c], fp[n, c] = E.bboxes_matching(c + 1, scores[n, c], boxes[n, c], *gts[n], matching_threshold=thr)
    return nb, tp, fp


def padded_with_poison(gts, G):
    """pad to exactly G entries; what lies behind n_gt is never to be read: NaN boxes of class 1, difficult"""
    from xdet.evaluation import pad_ground_truth
    gl, gb, gd, ng = pad_ground_truth(gts, min_boxes=G)
    assert gl.shape[1] == G
    for i, k in enumerate(ng):
        gl[i, k:], gb[i, k:], gd[i, k:] = 1, np.nan, 1
    return gl, gb, gd, ng


# ---- 4. the matcher -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('K', [1, 64, 200, 257])
@pytest.mark.parametrize('G', [1, 7, 42, 512])
@pytest.mark.parametrize('N', [1, 3, 64, 128])
def test_matcher_equals_the_host_matching_exactly(N, G, K):
    from xdet import evaluation as E
    C = 20 if N <= 3 else 5                      # (20: three class groups of a workgroup, the last one partial)
    scores, boxes, gts = M.make_batch(1000 * N + 10 * G + K, N, C, K, G, many=G >= 42)
    nb, tp, fp = E.bboxes_matching_batch(scores, boxes, *padded_with_poison(gts, G), matching_threshold=M.THR)
    wnb, wtp, wfp = host_flags(scores, boxes, gts)
    assert np.array_equal(nb, wnb)
    assert np.array_equal(tp, wtp), np.argwhere(tp != wtp)[:5]
    assert np.array_equal(fp, wfp), np.argwhere(fp != wfp)[:5]


def test_matcher_meets_every_corner_and_other_thresholds():
    from xdet import evaluation as E
    seen = dict.fromkeys(M.CORNERS, 0)
    scores, boxes, gts = M.make_batch(100, 40, 4, 24, 7)            # the first leg of the CPU sweep
    for n in range(40):
        for c in range(4):
            for k, v in M.census(c + 1, scores[n, c], boxes[n, c], gts[n]).items():
                seen[k] += v
    assert all(v > 0 for v in seen.values()), seen
    for thr in (0.5, 0.3, 0.0, 0.75):
        nb, tp, fp = E.bboxes_matching_batch(scores, boxes, *padded_with_poison(gts, 7), matching_threshold=thr)
        wnb, wtp, wfp = host_flags(scores, boxes, gts, thr)
        assert np.array_equal(nb, wnb) and np.array_equal(tp, wtp) and np.array_equal(fp, wfp), thr
    # n_gt = None: every one of the G entries exists
    gl, gb, gd, _ = E.pad_ground_truth([g for g in gts if len(g[0]) == 5][:3])
    k = gl.shape[0]
    assert k > 0 and gl.shape[1] == 5
    nb, tp, fp = E.bboxes_matching_batch(scores[:k], boxes[:k], gl, gb, gd)
    wnb, wtp, wfp = host_flags(scores[:k], boxes[:k], [(gl[i], gb[i], gd[i]) for i in range(k)])
    assert np.array_equal(nb, wnb) and np.array_equal(tp, wtp) and np.array_equal(fp, wfp)


def test_matcher_on_the_references_own_voc_eval_fixture():
    """tests/golden/voc_eval_golden.npz through the GPU matcher: flags equal the host's, and the recall / precision curves
    and both APs built from them are the reference's (as test_against_the_references_own_voc_eval for the host path)"""
    from xdet import evaluation as E
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'voc_eval_golden.npz'))
    gt = g['gt']
    classes = list(g['classes'])
    n_img, C = int(gt[:, 0].max()) + 1, len(classes)
    per = {}
    for ci, cls in enumerate(classes):
        det = g['%s_det' % cls]
        for im in range(n_img):
            d = det[det[:, 0] == im]
            per[im, ci] = d[np.argsort(-d[:, 1], kind='stable')]
    K = max(len(d) for d in per.values())
    scores, boxes = np.zeros((n_img, C, K), np.float32), np.zeros((n_img, C, K, 4), np.float32)
    for (im, ci), d in per.items():
        scores[im, ci, :len(d)], boxes[im, ci, :len(d)] = d[:, 1], d[:, [3, 2, 5, 4]]
    gts = []
    for im in range(n_img):
        rows = gt[gt[:, 0] == im]
        gts.append((rows[:, 1].astype(int), rows[:, [4, 3, 6, 5]].astype(np.float32), rows[:, 2].astype(int)))
    nb, tp, fp = E.bboxes_matching_batch(scores, boxes, *E.pad_ground_truth(gts))
    wnb, wtp, wfp = host_flags(scores, boxes, gts)
    assert np.array_equal(nb, wnb) and np.array_equal(tp, wtp) and np.array_equal(fp, wfp)
    for ci, cls in enumerate(classes):
        acc = E.StreamingTpFp()
        all_s, all_tp, all_fp = [], [], []
        for im in range(n_img):
            k = len(per[im, ci])
            acc.update(ci + 1, nb[im, ci], tp[im, ci, :k], fp[im, ci, :k], scores[im, ci, :k])
            all_s.append(scores[im, ci, :k]); all_tp.append(tp[im, ci, :k]); all_fp.append(fp[im, ci, :k])
        npos = int(nb[:, ci].sum())
        order = np.argsort(-np.concatenate(all_s))
        ctp = np.cumsum(np.concatenate(all_tp)[order].astype(np.float64))
        cfp = np.cumsum(np.concatenate(all_fp)[order].astype(np.float64))
        assert np.allclose(ctp / npos, g['%s_rec' % cls], atol=1e-12), cls
        assert np.allclose(ctp / np.maximum(ctp + cfp, np.finfo(np.float64).eps), g['%s_prec' % cls], atol=1e-12), cls
        ap07, ap12 = acc.average_precisions()
        assert abs(ap07[ci + 1] - float(g['%s_ap07' % cls])) < 1e-12, (cls, ap07[ci + 1])
        assert abs(ap12[ci + 1] - float(g['%s_ap12' % cls])) < 1e-12, (cls, ap12[ci + 1])


# ---- 5-7. the streaming accumulator ---------------------------------------------------------------------------------

C_S, K_S = 20, 64


def host_stream(scores, boxes, gts, skip=()):
    from xdet import evaluation as E
    host = E.StreamingTpFp()
    for n in range(scores.shape[0]):
        if n not in skip:
            host.update_image({c + 1: (scores[n, c], boxes[n, c]) for c in range(scores.shape[1])}, *gts[n])
    return host


def feed(acc, scores, boxes, gts, ids, batch, id_offset=0):
    for i in range(0, len(ids), batch):
        sel = ids[i:i + batch]
        acc.update(scores[sel], boxes[sel], image_ids=sel + id_offset, ground_truths=[gts[j] for j in sel])
    return acc


def assert_equals_host(acc, host, classes=None):
    recs, nobj, bad, overflow = acc.state()
    for c in classes or sorted(recs):
        s, tp, fp = recs[c][:3]
        assert np.array_equal(s, host.scores[c]) and np.array_equal(tp, host.tp[c]) and np.array_equal(fp, host.fp[c]), c
        assert nobj[c] == host.nobjects[c], c
    return recs


def test_streaming_is_independent_of_batching_and_sharding():
    from xdet.evaluation import GpuStreamingTpFp
    N = 203
    scores, boxes, gts = M.make_batch(42, N, C_S, K_S, 11)
    host = host_stream(scores, boxes, gts)
    assert sum(len(v) for v in host.scores.values()) > 2000 and sum(int(v.sum()) for v in host.tp.values()) > 100
    ids = np.arange(N)
    accs = [feed(GpuStreamingTpFp(C_S + 1, K_S, 16384), scores, boxes, gts, ids, b) for b in (1, 7, 64)]
    even = feed(GpuStreamingTpFp(C_S + 1, K_S, 16384), scores, boxes, gts, ids[0::2], 16)
    odd = feed(GpuStreamingTpFp(C_S + 1, K_S, 16384), scores, boxes, gts, ids[1::2], 16)
    accs.append(odd.merge(even))
    want = host.average_precisions()
    for acc in accs:
        recs = assert_equals_host(acc, host)
        assert all(np.all(np.diff(r[3] * K_S + r[4]) > 0) for r in recs.values())        # (image_id, slot) ascending
        assert acc.bad_images == 0 and not acc.overflow
        got = acc.average_precisions()
        assert got == want                                  # AP07 / AP12 per class, equal as floats
    s = accs[0].summary()
    assert s['AP_VOC07'] == want[0] and s['mAP_VOC12'] == sum(want[1].values()) / C_S


def test_overflow_sets_the_flag_and_keeps_the_class_untouched():
    from xdet import XdetError
    from xdet.evaluation import GpuStreamingTpFp
    scores, boxes, gts = M.make_batch(43, 32, C_S, K_S, 11)
    light = list(range(11, C_S + 1))                     # classes 11..20 get at most 6 detections per image
    scores[:, 10:, 6:], boxes[:, 10:, 6:] = 0, 0
    host = host_stream(scores, boxes, gts)
    small = host_stream(scores[:1], boxes[:1], gts[:1])
    counts = {c: len(host.scores[c]) for c in host.scores}
    cap = max(len(small.scores[c]) + counts[c] for c in light)
    heavy = [c for c in counts if c not in light]
    assert cap > 0 and min(counts[c] for c in heavy) > cap and max(len(v) for v in small.scores.values()) <= cap
    acc = GpuStreamingTpFp(C_S + 1, K_S, cap)
    feed(acc, scores, boxes, gts, np.arange(1), 1)       # one image fits every class
    assert_equals_host(acc, small)
    assert not acc.overflow
    feed(acc, scores, boxes, gts, np.arange(32), 32, id_offset=100)     # one call with more records than the heavy classes take
    recs, nobj, bad, overflow = acc.state()
    assert overflow
    both = host_stream(np.concatenate([scores[:1], scores]), np.concatenate([boxes[:1], boxes]), gts[:1] + gts)
    for c in heavy:                                      # refused: the class is as it was before the call
        assert np.array_equal(recs[c][0], small.scores[c]) and np.array_equal(recs[c][1], small.tp[c]), c
        assert nobj[c] == small.nobjects[c], c
    for c in light:                                      # the others took the call
        assert np.array_equal(recs[c][0], both.scores[c]) and np.array_equal(recs[c][1], both.tp[c]), c
        assert nobj[c] == both.nobjects[c], c
    with pytest.raises(XdetError, match='capacity'):
        acc.average_precisions()
    acc.reset()
    recs, nobj, bad, overflow = acc.state()
    assert not overflow and bad == 0 and all(len(r[0]) == 0 for r in recs.values()) and not any(nobj.values())
    feed(acc, scores, boxes, gts, np.arange(1), 1)
    assert_equals_host(acc, small)
    assert acc.average_precisions() == small.average_precisions()


def test_a_bad_image_is_counted_and_contributes_nothing():
    from xdet import XdetError
    from xdet import evaluation as E
    scores, boxes, gts = M.make_batch(44, 8, C_S, K_S, 11)
    bad = scores.copy()
    bad[3, :, 0] = np.nan
    acc = feed(E.GpuStreamingTpFp(C_S + 1, K_S, 4096), bad, boxes, gts, np.arange(8), 8)
    host = host_stream(scores, boxes, gts, skip=(3,))
    recs = assert_equals_host(acc, host)
    assert acc.bad_images == 1 and all(3 not in r[3] for r in recs.values())
    with pytest.raises(XdetError, match='1 image'):
        acc.average_precisions()
    assert acc.average_precisions(allow_bad=True) == host.average_precisions()
    # the op alone: flags and object counts of the bad image are zero, the others' are untouched
    nb, tp, fp = E.bboxes_matching_batch(bad, boxes, *E.pad_ground_truth(gts))
    wnb, wtp, wfp = host_flags(scores, boxes, gts)
    keep = np.arange(8) != 3
    assert not nb[3].any() and not tp[3].any() and not fp[3].any()
    assert np.array_equal(nb[keep], wnb[keep]) and np.array_equal(tp[keep], wtp[keep]) and np.array_equal(fp[keep], wfp[keep])
    # NaN in one class only marks the whole image
    one = scores.copy()
    one[5, 7, 0] = np.nan
    nb, tp, fp = E.bboxes_matching_batch(one, boxes, *E.pad_ground_truth(gts))
    assert not nb[5].any() and not tp[5].any() and not fp[5].any() and np.array_equal(tp[4], wtp[4])


def test_the_scratch_grows_with_the_batch_and_is_kept_for_a_smaller_one():
    """one accumulator fed batches of 2, then 5 (its per-batch scratch is freed and re-made larger), then 3 (kept)"""
    from xdet.evaluation import GpuStreamingTpFp
    scores, boxes, gts = M.make_batch(45, 10, 4, 8, 7)
    host = host_stream(scores, boxes, gts)
    assert sum(len(v) for v in host.scores.values()) > 0
    acc = GpuStreamingTpFp(4 + 1, 8, 256)
    for sel in (np.arange(0, 2), np.arange(2, 7), np.arange(7, 10)):
        acc.update(scores[sel], boxes[sel], image_ids=sel, ground_truths=[gts[j] for j in sel])
    assert_equals_host(acc, host)
    assert acc.bad_images == 0 and not acc.overflow


# ---- 8, 9. through the detector -------------------------------------------------------------------------------------

def rand_image(H, W, seed):
    return np.random.default_rng(seed + 7 * H + W).integers(0, 256, (H, W, 3), dtype=np.uint8)


def make_detector(lh_weights):
    from xdet.model import LightHeadDetector
    from xdet.runtime import set_precision, get_precision
    prev = get_precision()
    set_precision('f16x3')
    try:
        return LightHeadDetector(lh_weights, image_size=NET_S, max_batch=4, rpn_post_nms_top_n=100)
    finally:
        set_precision(prev)


@pytest.fixture(scope='module')
def det(lh_weights):
    return make_detector(lh_weights)


def ground_truth_from(dets):
    """ground truth made from an image's own detections: per class with detections, the top box (a true positive; with the
    low matching threshold of the test further detections of the class claim it again: duplicates), for every third such
    class marked difficult, plus one object per image that nothing detects (a miss)"""
    labels, boxes, diff = [], [], []
    for c in sorted(dets):
        s, b = dets[c]
        if s[0] > 0:
            labels.append(c); boxes.append(b[0]); diff.append(int(len(labels) % 3 == 0))
    labels.append(1); boxes.append(np.array([2., 2., 3., 3.], np.float32)); diff.append(0)
    return np.array(labels), np.array(boxes, np.float32), np.array(diff)


def test_evaluate_images_equals_detect_images_plus_the_host_accumulator(det, lh_weights):
    from xdet import evaluation as E
    thr = 0.05
    imgs = [rand_image(h, w, 21) for h, w in [(333, 500), (97, 300), (256, 256), (400, 180)]]
    dets = det.detect_images(imgs)
    gts = [ground_truth_from(d) for d in dets]
    host = E.StreamingTpFp()
    for d, gt in zip(dets, gts):
        host.update_image(d, *gt, matching_threshold=thr)
    n_tp = sum(int(v.sum()) for v in host.tp.values())
    n_obj = sum(host.nobjects.values())
    n_dup = 0
    for d, gt in zip(dets, gts):
        for c, (s, b) in d.items():
            out = M.census(c, s, b, gt, thr)
            n_dup += out['duplicates']
    print('true positives %d, objects %d, (image, class) cases with duplicates %d' % (n_tp, n_obj, n_dup))
    assert n_tp > 0 and n_dup > 0 and n_obj > n_tp          # true positives, duplicates and misses all occur
    acc = E.GpuStreamingTpFp(21, det.nms_topk, 4096)
    assert det.evaluate_images(imgs[:2], gts[:2], accumulator=acc, matching_threshold=thr) is acc
    det.evaluate_images(imgs[2:], gts[2:], accumulator=acc, matching_threshold=thr)      # ids continue: 2, 3
    recs = assert_equals_host(acc, host)                     # one read, after both calls
    assert sorted(set(np.concatenate([r[3] for r in recs.values()]).tolist())) == [0, 1, 2, 3]
    assert acc.average_precisions() == host.average_precisions()
    # the helper: the same dataset through evaluate(), two images per step
    fresh = make_detector(lh_weights)
    acc2 = E.GpuStreamingTpFp(21, det.nms_topk, 4096)
    out = fresh.evaluate(zip(imgs, gts), batch=2, accumulator=acc2, matching_threshold=thr)
    ap07, ap12 = host.average_precisions()
    assert out['AP_VOC07'] == ap07 and out['AP_VOC12'] == ap12
    assert out['mAP_VOC07'] == sum(ap07.values()) / 20 and out['mAP_VOC12'] == sum(ap12.values()) / 20
    # 9. the neighbours are undisturbed: a plain detect_images after evaluate_images equals a fresh detector's
    got = det.detect_images(imgs)
    want = make_detector(lh_weights).detect_images(imgs)
    for a, b, c0 in zip(got, want, dets):
        for c in a:
            assert np.array_equal(a[c][0], b[c][0]) and np.array_equal(a[c][1], b[c][1])
            assert np.array_equal(a[c][0], c0[c][0]) and np.array_equal(a[c][1], c0[c][1])
