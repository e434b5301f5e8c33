"""Shared by tests/test_eval_matching_math.py and tests/test_gpu_eval_matching.py: a seeded generator of detector-shaped
detections with ground truth that meets every corner of evaluation.bboxes_matching, the census of those corners, and the
first-occurrence formulation of the greedy matching (what csrc/evalmatch.hip computes) in NumPy."""
import numpy as np

THR = 0.5
CORNERS = ('duplicates', 'difficult_best', 'other_class_only_box0_difficult', 'other_class_only_box0_plain',
           'iou_at_threshold', 'zero_padded', 'no_ground_truth', 'unsorted_scores', 'tiny_scores', 'tp', 'fp')


def _rand_boxes(rng, n):
    y0, x0 = rng.random(n) * 0.7, rng.random(n) * 0.7
    h, w = 0.05 + rng.random(n) * 0.3, 0.05 + rng.random(n) * 0.3
    return np.stack([y0, x0, y0 + h, x0 + w], 1).astype(np.float32)


def make_image(rng, C, K, G, many=False):
    """-> det_scores [C,K], det_boxes [C,K,4], (glabels [g], gbboxes [g,4], gdifficults [g]) with 0 <= g <= G"""
    u = rng.random()
    if u < 0.08:
        g = 0
    elif many:
        g = int(rng.integers(max(G // 2, 1), G + 1))
    else:
        g = int(rng.integers(1, min(G, 11) + 1))
    kind = rng.random()
    if kind < 0.15:
        glabels = np.full(g, C + 1, np.int64)                   # objects of a class the detector does not have
    elif kind < 0.3:
        glabels = np.full(g, int(rng.integers(1, C + 1)), np.int64)
    else:
        glabels = rng.integers(1, C + 2, g)
    gbboxes = _rand_boxes(rng, g)
    for j in range(g):
        if rng.random() < 0.2:          # dyadic box: half of it has an IoU of exactly 0.5
            a, b = rng.choice([0., .25, .5], 2)
            gbboxes[j] = [a, b, a + .5, b + .5]
    gdiff = (rng.random(g) < 0.25).astype(np.int64)
    scores = np.zeros((C, K), np.float32)
    boxes = np.zeros((C, K, 4), np.float32)
    for c in range(C):
        nd = int(rng.integers(0, K + 1)) if rng.random() < 0.8 else K
        for i in range(nd):
            v = rng.random()
            if g and v < 0.45:
                j = int(rng.integers(g))
                boxes[c, i] = gbboxes[j] + rng.normal(0, 0.02, 4).astype(np.float32)
            elif g and v < 0.55:
                boxes[c, i] = gbboxes[int(rng.integers(g))]
            elif g and v < 0.65:
                b = gbboxes[int(rng.integers(g))].copy()
                b[3] = b[1] + (b[3] - b[1]) * np.float32(0.5)
                boxes[c, i] = b
            else:
                boxes[c, i] = _rand_boxes(rng, 1)[0]
        s = np.sort(0.01 + 0.99 * rng.random(nd).astype(np.float32))[::-1]
        if nd and rng.random() < 0.1:
            s[-1] = np.float32(5e-5)                               # below streaming_tp_fp_arrays' 1e-4
        if rng.random() < 0.2:
            s = rng.permutation(s)
        scores[c, :nd] = s
    return scores, boxes, (glabels, gbboxes, gdiff)


def make_batch(seed, N, C, K, G, many=False):
    """-> det_scores [N,C,K], det_boxes [N,C,K,4], ground truth list of N"""
    rng = np.random.default_rng(seed)
    imgs = [make_image(rng, C, K, G, many) for _ in range(N)]
    return np.stack([i[0] for i in imgs]), np.stack([i[1] for i in imgs]), [i[2] for i in imgs]


def first_occurrence_matching(label, scores, bboxes, glabels, gbboxes, gdifficults, thr=THR):
    """bboxes_matching without the serial chain: every detection's best box on its own, then the first claimant of
    each box.  -> (n_gbboxes, tp, fp, k, iou_best)"""
    from xdet import evaluation as E
    bboxes = np.asarray(bboxes, np.float32).reshape(-1, 4)
    glabels = np.asarray(glabels).reshape(-1)
    gbboxes = np.asarray(gbboxes, np.float32).reshape(-1, 4)
    gdiff = np.asarray(gdifficults).reshape(-1).astype(bool)
    n = bboxes.shape[0]
    same = glabels == label
    n_gb = int(np.count_nonzero(same & ~gdiff))
    if glabels.shape[0] == 0:
        return n_gb, np.zeros(n, bool), np.zeros(n, bool), np.zeros(n, int), np.zeros(n, np.float32)
    jac = np.stack([E.bboxes_jaccard(bboxes[i], gbboxes) for i in range(n)]) * same
    k = jac.argmax(1)
    best = jac[np.arange(n), k]
    match = best > np.float32(thr)
    diff = gdiff[k]
    first = np.full(glabels.shape[0], n, int)
    cand = np.flatnonzero(match & ~diff)
    np.minimum.at(first, k[cand], cand)
    tp = ~diff & match & (first[k] == np.arange(n))
    fp = ~diff & ~tp
    return n_gb, tp, fp, k, best


def census(label, scores, bboxes, gt, thr=THR):
    """which corners one (image, class) case meets"""
    glabels, gbboxes, gdiff = gt
    out = dict.fromkeys(CORNERS, 0)
    n_gb, tp, fp, k, best = first_occurrence_matching(label, scores, bboxes, glabels, gbboxes, gdiff, thr)
    g = len(glabels)
    out['no_ground_truth'] = int(g == 0)
    out['zero_padded'] = int(np.any((scores == 0) & np.all(bboxes == 0, 1)))
    out['unsorted_scores'] = int(np.any(np.diff(scores) > 0))
    out['tiny_scores'] = int(np.any((scores > 0) & (scores <= 1e-4) & (tp | fp)))
    out['tp'], out['fp'] = int(tp.any()), int(fp.any())
    if g:
        match = best > np.float32(thr)
        claimed = k[match & ~np.asarray(gdiff, bool)[k]]
        out['duplicates'] = int(len(claimed) > len(set(claimed.tolist())))
        out['difficult_best'] = int(np.any(np.asarray(gdiff, bool)[k] & match))
        if not np.any(np.asarray(glabels) == label):
            out['other_class_only_box0_difficult' if gdiff[0] else 'other_class_only_box0_plain'] = 1
        out['iou_at_threshold'] = int(np.any(best == np.float32(thr)))
    return out
