"""Shared by tests/test_targets_math.py and tests/test_gpu_targets.py: seeded generators of ground truth and ROIs that meet
every corner of the dual-max match (xdet/targets.py), the census of those corners, and the anchor sets of the two input
sizes."""
import numpy as np

HIGH, LOW = 0.7, 0.3
CORNERS = ('positives', 'ignored', 'forced', 'forced_below_high', 'all_zero_rows', 'two_boxes_one_anchor',
           'forced_not_column_max', 'column_ties', 'row_ties')


def anchors(size):
    """the single-layer anchor set of a size x size input: (yref [h,w], xref [h,w], href [22], wref [22]), h = w = size / 16"""
    from xdet import ops
    s = size // 16
    ac = ops.AnchorCreator([size, size], [(s, s)], [[0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8]], [[0.1]], [[1., 2., .5]], [16])
    return ac.get_all_anchors()[0][0]


def random_boxes(rng, n):
    """centres U(0,1), sides U(0.02, 0.7), clipped to the image"""
    cy, cx = rng.random(n), rng.random(n)
    h, w = 0.02 + 0.68 * rng.random(n), 0.02 + 0.68 * rng.random(n)
    b = np.stack([cy - h / 2, cx - w / 2, cy + h / 2, cx + w / 2], 1)
    return np.clip(b, 0., 1.).astype(np.float32)


def make_ground_truth(seed, N, anchor, max_boxes=11, num_classes=21, min_boxes=1):
    """-> (labels, boxes): lists of N per-image arrays.  Every fourth image ends with a duplicate of its first box, every
    fourth has a box equal to a random anchor, every fourth the box (0.999, 0.999, 1, 1)."""
    from xdet import targets as T
    rng = np.random.default_rng(seed)
    abox = T.anchor_boxes(anchor)[0]
    labels, boxes = [], []
    for n in range(N):
        g = int(rng.integers(min_boxes, max_boxes + 1))
        b = random_boxes(rng, g)
        if n % 4 == 1 and g >= 2:
            b[int(rng.integers(g))] = abox[int(rng.integers(abox.shape[0]))]
        if n % 4 == 2 and g >= 2:
            b[int(rng.integers(g))] = (0.999, 0.999, 1., 1.)
        if n % 4 == 0 and g >= 2:
            b[-1] = b[0]
        labels.append(rng.integers(1, num_classes, g).astype(np.int64))
        boxes.append(b)
    return labels, boxes


def make_rois(seed, N, R, boxes, duplicates=True):
    """proposal-like ROIs [N,R,4]: jittered copies of the image's boxes, random boxes, some reaching over the border, and
    (as the proposal stage's up-sampling produces them) exact duplicates of earlier ROIs"""
    rng = np.random.default_rng(seed)
    out = np.zeros((N, R, 4), np.float32)
    for n in range(N):
        r = random_boxes(rng, R)
        b = np.asarray(boxes[n], np.float32).reshape(-1, 4)
        if len(b):
            k = R // 3
            src = b[rng.integers(len(b), size=k)]
            r[:k] = src + rng.normal(0, 0.03, (k, 4)).astype(np.float32)
            r[k:k + 4] = b[rng.integers(len(b), size=4)]                 # exact copies of boxes
        r[R // 2:R // 2 + 8] += np.float32(0.15)                         # beyond the border of 0.1 on the far side
        if duplicates:
            r[R - R // 8:] = r[:R // 8]
        out[n] = r
    return out


def census(anchor, labels, boxes, allowed_border=0., high=HIGH, low=LOW):
    """the corners a batch meets, counted over its images"""
    from xdet import targets as T
    cand, _ = T.anchor_boxes(anchor)
    lo, hi = T._border(allowed_border)
    out = dict.fromkeys(CORNERS, 0)
    for b in boxes:
        if len(b) == 0:
            continue
        O = T.overlap_matrix(b, cand, lo, hi)
        m, _ = T.dual_max_match(O, high, low)
        mv, best_g, best_a = O.max(0), O.argmax(0), O.argmax(1)
        forced = np.unique(best_a)
        out['positives'] += int((m > -1).sum())
        out['ignored'] += int((m == -2).sum())
        out['forced'] += len(forced)
        out['forced_below_high'] += int((mv[forced] < np.float32(high)).sum())
        out['all_zero_rows'] += int((O.max(1) == 0).sum())
        out['two_boxes_one_anchor'] += int(len(best_a) - len(forced))
        out['forced_not_column_max'] += int((m[forced] != best_g[forced]).sum())
        out['column_ties'] += int(((O == mv[None, :]) & (mv[None, :] > 0)).sum(0).__gt__(1).sum())
        out['row_ties'] += int(((O == O.max(1)[:, None]) & (O.max(1)[:, None] > 0)).sum(1).__gt__(1).sum())
    return out


def threshold_from_batch(anchor, boxes, allowed_border=0., lo=0.35, hi=0.65):
    """an IoU value that occurs in the batch's own overlap matrices as a column maximum, between lo and hi"""
    from xdet import targets as T
    cand, _ = T.anchor_boxes(anchor)
    l, h = T._border(allowed_border)
    for b in boxes:
        if len(b) == 0:
            continue
        mv = T.overlap_matrix(b, cand, l, h).max(0)
        v = mv[(mv > lo) & (mv < hi)]
        if len(v):
            return float(v[len(v) // 2])
    raise AssertionError('no column maximum between %g and %g' % (lo, hi))
