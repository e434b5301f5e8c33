"""The training-target contract (include/xdet.h) without a GPU: the vectorised NumPy statement of
xdet/targets.py against a loop-per-candidate restatement written here from the contract's text, the targets against
float64, the sampler's rules, and the argument errors of the C ABI."""
import math

import numpy as np
import pytest

import target_cases as C

f32 = np.float32
ROI_ARGS = dict(allowed_border=0.1, fg_thr=0.53, bg_high_thr=0.5, bg_low_thr=0.)


# ---- the restatement: one candidate at a time, Python scalars of f32 values -------------------------------------------

def rows_overlap(gb, cand, lo, hi):
    """O[g] for one box at a time (NumPy over the candidates only: every operation is a single f32 operation)"""
    inside = ((cand[:, 0] >= lo) & (cand[:, 1] >= lo) & (cand[:, 2] < hi) & (cand[:, 3] < hi)).astype(f32)
    area_c = (cand[:, 3] - cand[:, 1]) * (cand[:, 2] - cand[:, 0])
    rows = []
    for g in range(gb.shape[0]):
        ymin, xmin, ymax, xmax = gb[g]
        h = np.maximum(np.minimum(ymax, cand[:, 2]) - np.maximum(ymin, cand[:, 0]), f32(0))
        w = np.maximum(np.minimum(xmax, cand[:, 3]) - np.maximum(xmin, cand[:, 1]), f32(0))
        inter = h * w
        union = ((xmax - xmin) * (ymax - ymin) + area_c) - inter
        safe = np.where(union == 0, f32(1), union)
        rows.append((np.where(union == 0, f32(0), inter / safe) * inside).astype(f32))
    return rows


def loop_match(glabels, gb, cand, lo, hi, high, low):
    """-> labels, match, scores by the four steps of the contract, scanning in ascending order with strict >"""
    G, M = gb.shape[0], cand.shape[0]
    if G == 0:
        return [0] * M, [-1] * M, [0.] * M
    O = [r.tolist() for r in rows_overlap(gb, cand, f32(lo), f32(hi))]
    high, low = float(f32(high)), float(f32(low))
    best_a = []
    for g in range(G):                       # step 2
        row, b, bv = O[g], 0, O[g][0]
        for a in range(1, M):
            if row[a] > bv:
                b, bv = a, row[a]
        best_a.append(b)
    named = {}
    for g, a in enumerate(best_a):
        named.setdefault(a, []).append(g)
    labels, match, scores = [], [], []
    for a in range(M):
        bg, mv = 0, O[0][a]                  # step 1
        for g in range(1, G):
            if O[g][a] > mv:
                bg, mv = g, O[g][a]
        m = -1 if mv < low else (-2 if mv < high else bg)
        s = mv
        if a in named:                       # step 3: first maximum of the products, box 0 when all are zero
            prod = [O[g][a] if g in named[a] else 0. for g in range(G)]
            m = 0
            for g in range(1, G):
                if prod[g] > prod[m]:
                    m = g
            s = O[m][a]                      # step 4
        match.append(m)
        scores.append(s)
        labels.append(int(glabels[max(m, 0)]) * (m > -1) - (m < -1))
    return labels, match, scores


def loop_sample(labels, scores, P, fg_fraction, bg_low, seed, image):
    from xdet import targets as T

    def shuffled(S, stream):
        keys = T.shuffle_keys(seed, image, S, stream).tolist() if len(S) else []
        return [e for _, e in sorted(zip(keys, S))]
    x = float(f32(P) * f32(fg_fraction))
    exp_fg = int(math.floor(x)) if x - math.floor(x) < 0.5 else int(math.ceil(x))
    if x - math.floor(x) == 0.5:
        exp_fg = int(math.floor(x)) + int(math.floor(x)) % 2
    pos = [i for i, l in enumerate(labels) if l > 0]
    neg = [i for i, (l, s) in enumerate(zip(labels, scores)) if l == 0 and s > float(f32(bg_low))]
    fg = pos if len(pos) < exp_fg else shuffled(pos, 0)[:exp_fg]
    exp_bg = P - min(len(pos), exp_fg)
    bg = neg if len(neg) < exp_bg else shuffled(neg, 0)[:exp_bg]
    keep = fg + bg
    if not keep:
        return [-1] * P, (len(pos), len(neg), 0)
    if len(keep) < P:
        left = P - len(keep)
        idx = list(range(len(keep))) * (left // len(keep) + 1) + shuffled(list(range(len(keep))), 1)[:left % len(keep)]
        return [keep[i] for i in idx], (len(pos), len(neg), len(keep))
    return keep, (len(pos), len(neg), len(keep))


def targets_f64(gb, refs, match, scaling=(1., 1., 1., 1.)):
    g = np.asarray(gb, np.float64)[np.maximum(match, 0)]
    r = np.asarray(refs, np.float64)
    with np.errstate(divide='ignore', invalid='ignore'):
        t = np.stack([(((g[:, 2] + g[:, 0]) / 2 - r[:, 0]) / r[:, 2]) / scaling[0], (((g[:, 3] + g[:, 1]) / 2 - r[:, 1]) / r[:, 3]) / scaling[1],
                      np.log((g[:, 2] - g[:, 0]) / r[:, 2]) / scaling[2], np.log((g[:, 3] - g[:, 1]) / r[:, 3]) / scaling[3]], -1)
    return t


def assert_targets_close(got, want, where):
    """|delta| <= 1e-6 * max(1, |value|) on the rows `where`"""
    d = np.abs(got[where].astype(np.float64) - want[where])
    bar = 1e-6 * np.maximum(1., np.abs(want[where]))
    worst = float((d / bar).max()) if d.size else 0.
    print('targets: %d rows, largest |delta| / bar = %.3f' % (int(np.count_nonzero(where)), worst))
    assert np.all(d <= bar), worst


def decode_rois(rois, targets):
    """ext_decode_rois (anchor_manipulator.py:671-683) in NumPy f32, scaling 1"""
    r, t = np.asarray(rois, f32), np.asarray(targets, f32)
    h, w = r[:, 2] - r[:, 0], r[:, 3] - r[:, 1]
    cy, cx = t[:, 0] * h + (r[:, 0] + h / f32(2)), t[:, 1] * w + (r[:, 1] + w / f32(2))
    ph, pw = np.exp(t[:, 2]) * h, np.exp(t[:, 3]) * w
    return np.stack([cy - ph / f32(2), cx - pw / f32(2), cy + ph / f32(2), cx + pw / f32(2)], -1)


@pytest.fixture(scope='module')
def anchor():
    return C.anchors(480)


@pytest.fixture(scope='module')
def census_batch(anchor):
    return C.make_ground_truth(7, 40, anchor)


# ---- anchors -------------------------------------------------------------------------------------------------------

def test_census_batch_meets_every_corner(anchor, census_batch):
    cen = C.census(anchor, *census_batch)
    print(cen)
    for k in C.CORNERS:
        assert cen[k] > 0, (k, cen)


def check_anchor_batch(anchor, labels, boxes, n_gt=None, border=0., high=C.HIGH, low=C.LOW):
    from xdet import targets as T
    l, t, s, m = T.host_encode_anchors(anchor, labels, boxes, n_gt, border, high, low, return_match=True)
    gl, gb, ng = T.ground_truth(labels, boxes, n_gt)
    cand, refs = T.anchor_boxes(anchor)
    lo, hi = T._border(border)
    for n in range(gl.shape[0]):
        k = int(ng[n])
        ll, mm, ss = loop_match(gl[n, :k], gb[n, :k], cand, lo, hi, high, low)
        assert np.array_equal(l[n], np.array(ll, np.int32)), n
        assert np.array_equal(m[n], np.array(mm, np.int64)), n
        assert np.array_equal(s[n], np.array(ss, f32)), n
        if k:
            pos = m[n] > -1
            assert_targets_close(t[n], targets_f64(gb[n, :k], refs, m[n]), pos)
            assert np.all(t[n][~pos] == 0)
        else:
            assert not l[n].any() and not t[n].any() and not s[n].any()
    return l, t, s, m


def test_host_anchors_equal_the_loop_restatement_on_the_census_batch(anchor, census_batch):
    l, _, _, m = check_anchor_batch(anchor, *census_batch)
    assert (l > 0).sum() == (m > -1).sum() > 0 and (l == -1).sum() == (m == -2).sum() > 0


@pytest.mark.parametrize('which', ['high', 'low'])
def test_threshold_equality(anchor, census_batch, which):
    """mv == high is a match, mv == low is "ignore": the threshold is an IoU value of the batch's own matrix"""
    from xdet import targets as T
    labels, boxes = census_batch[0][:6], census_batch[1][:6]
    thr = C.threshold_from_batch(anchor, boxes)
    high, low = (thr, 0.3) if which == 'high' else (0.7, thr)
    l, t, s, m = check_anchor_batch(anchor, labels, boxes, high=high, low=low)
    cand, _ = T.anchor_boxes(anchor)
    hit = 0
    for n in range(len(boxes)):
        mv = T.overlap_matrix(boxes[n], cand, *T._border(0.)).max(0)
        at = (mv == f32(thr)) & ~np.isin(np.arange(len(mv)), T.overlap_matrix(boxes[n], cand, *T._border(0.)).argmax(1))
        hit += int(at.sum())
        assert np.all(m[n][at] > -1) if which == 'high' else np.all(m[n][at] == -2)
    assert hit > 0


def test_no_ground_truth_and_poison_behind_n_gt(anchor, census_batch):
    from xdet import targets as T
    labels, boxes = census_batch[0][:4], census_batch[1][:4]
    gl, gb, ng = T.ground_truth(labels, boxes)
    G = gl.shape[1] + 3
    pl, pb = np.ones((4, G), np.int32), np.full((4, G, 4), np.nan, f32)
    for n in range(4):
        pl[n, :ng[n]], pb[n, :ng[n]] = gl[n, :ng[n]], gb[n, :ng[n]]
    ng = ng.copy()
    ng[2] = 0
    got = check_anchor_batch(anchor, pl, pb, ng)
    labels[2], boxes[2] = labels[2][:0], boxes[2][:0]
    want = T.host_encode_anchors(anchor, labels, boxes, return_match=True)
    for a, b in zip(got, want):
        assert np.array_equal(a, b)
    assert not got[0][2].any() and not got[2][2].any()


# ---- ROIs ----------------------------------------------------------------------------------------------------------

def check_roi_batch(rois, labels, boxes, n_gt=None, P=64, fg_fraction=0.25, seed=0, image_ids=None, f64_rows=False):
    from xdet import targets as T
    out = T.host_encode_rois(rois, labels, boxes, n_gt, rois_per_image=P, fg_fraction=fg_fraction, seed=seed,
                             image_ids=image_ids, return_all=True, **ROI_ARGS)
    o_r, o_t, o_l, o_s, o_i, counts, a_l, a_t, a_s, a_m = out
    gl, gb, ng = T.ground_truth(labels, boxes, n_gt)
    lo, hi = T._border(ROI_ARGS['allowed_border'])
    N, R = rois.shape[:2]
    for n in range(N):
        k = int(ng[n])
        sel = gl[n, :k] > 0
        l, b = gl[n, :k][sel], gb[n, :k][sel]
        cand = np.concatenate([rois[n], b], 0)
        M = cand.shape[0]
        ll, mm, ss = loop_match(l, b, cand, lo, hi, ROI_ARGS['fg_thr'], ROI_ARGS['bg_high_thr'])
        assert np.array_equal(a_l[n, :M], np.array(ll, np.int32)) and np.all(a_l[n, M:] == -1), n
        assert np.array_equal(a_m[n, :M], np.array(mm, np.int64)), n
        assert np.array_equal(a_s[n, :M], np.array(ss, f32)), n
        idx, cnt = loop_sample(ll, ss, P, fg_fraction, ROI_ARGS['bg_low_thr'], seed, n if image_ids is None else int(image_ids[n]))
        assert np.array_equal(o_i[n], np.array(idx, np.int32)), n
        assert tuple(counts[n]) == (M,) + cnt, n
        if cnt[2]:
            assert np.array_equal(o_r[n], cand[idx]) and np.array_equal(o_l[n], a_l[n][idx])
            assert np.array_equal(o_s[n], a_s[n][idx]) and np.array_equal(o_t[n], a_t[n][idx], equal_nan=True)
        else:
            assert np.all(o_l[n] == -1) and not o_r[n].any() and not o_t[n].any() and not o_s[n].any()
        if len(l):
            refs = T.roi_refs(cand)
            pos = a_m[n, :M] > -1
            with np.errstate(invalid='ignore'):
                assert np.all((a_t[n, :M][~pos] == 0) | np.isnan(a_t[n, :M][~pos]))
            if f64_rows:
                # the bar is reachable where the reference point is not tiny: the centre terms carry an absolute error of
                # at most 9e-8 (three roundings of values below 1, the sum ymax + ymin below 2) divided by href / wref
                rows = pos & (refs[:, 2] >= 0.12) & (refs[:, 3] >= 0.12)
                assert rows.any()
                assert_targets_close(a_t[n, :M], targets_f64(b, refs, a_m[n, :M]), rows)
            lp = np.flatnonzero(pos & (a_l[n, :M] > 0) & (refs[:, 2] > 0) & (refs[:, 3] > 0))
            back = decode_rois(cand[lp], a_t[n, :M][lp])
            assert np.abs(back - b[a_m[n, :M][lp]]).max() <= 1e-5
    return out


def test_host_rois_equal_the_loop_restatement(anchor, census_batch):
    labels, boxes = census_batch[0][:12], census_batch[1][:12]
    rois = C.make_rois(3, 12, 300, boxes)
    out = check_roi_batch(rois, labels, boxes, f64_rows=True)
    assert (out[5][:, 1] > 0).all() and (out[5][:, 3] > 0).all()


def test_rois_with_background_entries_no_ground_truth_and_poison(anchor, census_batch):
    from xdet import targets as T
    labels = [l.copy() for l in census_batch[0][:6]]
    boxes = [b.copy() for b in census_batch[1][:6]]
    for n in range(6):
        labels[n][::2] = 0                       # entries the ROI form drops
    labels[1][:] = 0                             # nothing left
    labels[3], boxes[3] = labels[3][:0], boxes[3][:0]
    rois = C.make_rois(5, 6, 300, boxes)
    out = check_roi_batch(rois, labels, boxes)
    assert out[5][1, 3] == 0 and out[5][3, 3] == 0 and np.all(out[2][1] == -1)
    gl, gb, ng = T.ground_truth(labels, boxes)
    G = gl.shape[1] + 2
    pl, pb = np.ones((6, G), np.int32), np.full((6, G, 4), np.nan, f32)
    for n in range(6):
        pl[n, :ng[n]], pb[n, :ng[n]] = gl[n, :ng[n]], gb[n, :ng[n]]
    got = check_roi_batch(rois, pl, pb, ng)
    for a, b in zip(got[:6], out[:6]):
        assert np.array_equal(a, b, equal_nan=True)


# ---- the sampler ---------------------------------------------------------------------------------------------------

def synthetic(n_pos, n_neg, n_ign=5, n_low=3, seed=0):
    """labels / scores of n_pos positives, n_neg usable negatives, ignored ones and negatives at score 0, interleaved"""
    rng = np.random.default_rng(seed)
    labels = np.concatenate([rng.integers(1, 21, n_pos), np.zeros(n_neg, int), -np.ones(n_ign, int), np.zeros(n_low, int)])
    scores = np.concatenate([0.6 + 0.4 * rng.random(n_pos), 0.01 + 0.4 * rng.random(n_neg), np.full(n_ign, 0.51), np.zeros(n_low)])
    p = rng.permutation(len(labels))
    return labels[p], scores[p].astype(f32)


@pytest.mark.parametrize('n_pos,n_neg,P,n_keep,n_fg', [
    (10, 200, 64, 64, 10),      # |pos| below exp_fg = 16
    (16, 200, 64, 64, 16),      # equal: shuffled too
    (40, 200, 64, 64, 16),      # above
    (40, 20, 64, 36, 16),       # |neg| short: 28 left, no full tile, remainder 28
    (4, 12, 64, 16, 4),         # n_keep short without a remainder: 48 left = 3 tiles
    (5, 10, 64, 15, 5),         # with one: 49 left = 3 tiles + 4
    (0, 0, 64, 0, 0),           # nothing to keep
])
def test_sampler_counts_and_composition(n_pos, n_neg, P, n_keep, n_fg):
    from xdet import targets as T
    labels, scores = synthetic(n_pos, n_neg)
    idx, cnt = T.sample_rois(labels, scores, P, 0.25, 0., seed=11, image=2)
    want, wcnt = loop_sample(labels.tolist(), scores.tolist(), P, 0.25, 0., 11, 2)
    assert idx.tolist() == want and cnt == wcnt == (n_pos, n_neg, n_keep)
    if n_keep == 0:
        assert np.all(idx == -1)
        return
    head = idx[:n_keep]
    assert len(set(head.tolist())) == n_keep
    assert np.all(labels[head[:n_fg]] > 0) and np.all(labels[head[n_fg:]] == 0) and np.all(scores[head[n_fg:]] > 0)
    if n_pos < 16:
        assert head[:n_fg].tolist() == np.flatnonzero(labels > 0).tolist()        # taken as they are, in index order
    left = P - n_keep
    times = np.bincount(np.searchsorted(np.sort(head), idx), minlength=n_keep)[np.argsort(np.argsort(head))]
    # the tiling rule: every kept one (left div n_keep) + 1 times, (left mod n_keep) of them once more
    q, r = (left // n_keep + 1, left % n_keep) if left else (1, 0)
    assert np.all((times == q) | (times == q + 1)) and int((times == q + 1).sum()) == r
    assert idx[:n_keep * q].tolist() == head.tolist() * q


def test_sampler_seeds_and_fairness():
    from xdet import targets as T
    labels, scores = synthetic(40, 200)
    a = T.sample_rois(labels, scores, 64, 0.25, 0., seed=5, image=0)[0]
    assert np.array_equal(a, T.sample_rois(labels, scores, 64, 0.25, 0., seed=5, image=0)[0])
    assert not np.array_equal(a, T.sample_rois(labels, scores, 64, 0.25, 0., seed=6, image=0)[0])
    assert not np.array_equal(a, T.sample_rois(labels, scores, 64, 0.25, 0., seed=5, image=1)[0])
    # 2,000 seeds, 16 of 40 positives each: a positive is chosen Binomial(2000, 0.4) times; 5 sigma = 5 * sqrt(2000 * .4 * .6)
    pos = np.flatnonzero(labels > 0)
    hits = np.zeros(len(labels), int)
    for seed in range(2000):
        hits[T.shuffle(pos, seed, 0, 0)[:16]] += 1
    sigma = math.sqrt(2000 * 0.4 * 0.6)
    print('chosen %d .. %d times, 800 +- %.1f allowed' % (hits[pos].min(), hits[pos].max(), 5 * sigma))
    assert hits[pos].sum() == 2000 * 16 and np.all(np.abs(hits[pos] - 800) <= 5 * sigma)
    assert T.expected_fg(64, 0.25) == 16 and T.expected_fg(2, 0.25) == 0 and T.expected_fg(6, 0.25) == 2 and T.expected_fg(10, 0.25) == 2


def test_shuffle_keys_are_32_bit_and_never_tie():
    from xdet import targets as T
    k = T.shuffle_keys(0xFFFFFFFF, 123456, np.arange(8192), 0)
    assert k.dtype == np.uint32 and len(set(k.tolist())) == 8192
    assert not np.array_equal(k, T.shuffle_keys(0xFFFFFFFF, 123456, np.arange(8192), 1))
    # the written definition, in Python integers
    def mix(x):
        x ^= x >> 16
        x = x * 0x7FEB352D & 0xFFFFFFFF
        x ^= x >> 15
        x = x * 0x846CA68B & 0xFFFFFFFF
        return x ^ x >> 16
    word = mix((mix(77 ^ 0x9E3779B9) + 3) & 0xFFFFFFFF)
    assert T.shuffle_keys(77, 3, [0, 1, 5000], 1).tolist() == [mix(word ^ (2 * e + 1)) for e in (0, 1, 5000)]


# ---- the C ABI -----------------------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def built():
    from xdet import build
    return build.build()


def test_symbols_are_exported(built):
    import re
    import subprocess
    out = subprocess.check_output(['nm', '-D', '--defined-only', built]).decode()
    exported = set(re.findall(r'\sT\s+(xdet_[a-z0-9_]+)', out))
    assert {'xdet_targets_workspace_bytes', 'xdet_encode_anchors', 'xdet_encode_rois'} <= exported
    blob = open(built, 'rb').read()
    for kern in (b'tg_prepare_kernel', b'tg_colmax_kernel', b'tg_assign_kernel', b'tg_sample_kernel'):
        assert kern in blob
    from xdet._lib import lib
    assert lib().xdet_targets_workspace_bytes(2, 0, 8) > 0
    assert lib().xdet_targets_workspace_bytes(2, 308, 8) >= 2 * 308 * 24


def test_argument_errors_without_a_gpu(built, anchor):
    import xdet
    from xdet import targets as T
    E = xdet.InvalidArgumentError
    one = ([np.array([1])], [np.array([[.1, .1, .5, .5]], f32)])
    pad = lambda G: (np.ones((1, G), np.int32), np.zeros((1, G, 4), f32))
    rois = np.zeros((1, 300, 4), f32)
    with pytest.raises(E):
        T.encode_anchors(anchor, *pad(513))
    with pytest.raises(E):
        T.encode_anchors(anchor, *one, high_thr=float('nan'))
    with pytest.raises(E):
        T.encode_anchors(anchor, *one, allowed_border=float('inf'))
    with pytest.raises(E):
        T.encode_anchors((anchor[0][:0], anchor[1][:0], anchor[2], anchor[3]), *one)
    with pytest.raises(E):
        T.encode_anchors(anchor, np.ones((1, 0), np.int32), np.zeros((1, 0, 4), f32))
    with pytest.raises(E):
        T.encode_rois(rois, *pad(513))
    with pytest.raises(E):
        T.encode_rois(np.zeros((1, 8190, 4), f32), *pad(3))
    with pytest.raises(E):
        T.encode_rois(rois[:, :0], *one)
    with pytest.raises(E):
        T.encode_rois(rois, *one, rois_per_image=0)
    with pytest.raises(E):
        T.encode_rois(rois, *one, fg_fraction=1.5)
    with pytest.raises(E):
        T.encode_rois(rois, *one, fg_fraction=-0.1)
    with pytest.raises(E):
        T.encode_rois(rois, *one, fg_thr=float('nan'))
    with pytest.raises(E):
        T.encode_rois(rois, *one, bg_low_thr=float('-inf'))
    # NULL required pointers, straight at the ABI
    import ctypes
    from xdet._lib import lib, check
    sc = (ctypes.c_float * 4)(1, 1, 1, 1)
    with pytest.raises(E):
        check(lib().xdet_encode_anchors(None, None, 30, 30, 22, 0., None, None, None, 1, 4, .7, .3, sc, None, None, None, None, None))
    with pytest.raises(E):
        check(lib().xdet_encode_rois(None, 300, None, None, None, 1, 4, .1, .53, .5, 0., sc, 64, .25, 0, None, None, None, None,
                                     None, None, None, None, None, None, None, None))
    with pytest.raises(E):
        check(lib().xdet_encode_rois(None, 300, None, None, None, 1, 4, .1, .53, .5, 0., None, 64, .25, 0, None, None, None, None,
                                     None, None, None, None, None, None, None, None))
