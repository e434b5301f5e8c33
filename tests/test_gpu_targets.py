"""xdet_encode_anchors / xdet_encode_rois (csrc/targets.hip) against the NumPy statement of the same contract
(xdet/targets.py, itself pinned by tests/test_targets_math.py): every discrete result and every score bit for bit, the
regression targets within 1e-6 * max(1, |value|) (logf is the one operation that may round differently; the largest
difference measured on an MI355X over all cases of this file is 0.12 of that bar)."""
import ctypes

import numpy as np
import pytest

import target_cases as C

pytestmark = pytest.mark.gpu
f32 = np.float32
ROI = dict(allowed_border=0.1, fg_thr=0.53, bg_high_thr=0.5, bg_low_thr=0.)


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def assert_targets(got, want, what):
    got, want = np.asarray(got, f32), np.asarray(want, f32)
    assert np.array_equal(np.isnan(got), np.isnan(want)), what
    fin = np.isfinite(want)
    assert np.array_equal(got[~fin & ~np.isnan(want)], want[~fin & ~np.isnan(want)]), what
    d = np.abs(got[fin].astype(np.float64) - want[fin].astype(np.float64))
    bar = 1e-6 * np.maximum(1., np.abs(want[fin].astype(np.float64)))
    worst = float((d / bar).max()) if d.size else 0.
    print('%s: targets, largest |delta| / bar = %.4f over %d values (%d differ)' % (what, worst, d.size, int((d > 0).sum())))
    assert np.all(d <= bar), (what, worst)


def check_anchors(anchor, labels, boxes, n_gt=None, border=0., high=C.HIGH, low=C.LOW, what=''):
    from xdet import targets as T
    want = T.host_encode_anchors(anchor, labels, boxes, n_gt, border, high, low)
    got = T.encode_anchors(anchor, labels, boxes, n_gt, border, high, low)
    assert np.array_equal(got[0], want[0]), what
    assert np.array_equal(bits(got[2]), bits(want[2])), what
    assert_targets(got[1], want[1], what)
    return got


@pytest.fixture(scope='module')
def a480():
    return C.anchors(480)


@pytest.fixture(scope='module')
def a800():
    return C.anchors(800)


@pytest.fixture(scope='module')
def census_batch(a480):
    return C.make_ground_truth(7, 40, a480)


def test_anchors_census_batch(a480, census_batch):
    cen = C.census(a480, *census_batch)
    assert all(cen[k] > 0 for k in C.CORNERS), cen
    l, t, s = check_anchors(a480, *census_batch, what='census')
    assert (l > 0).sum() > 0 and (l == -1).sum() > 0


@pytest.mark.parametrize('which', ['high', 'low'])
def test_anchors_threshold_equality(a480, census_batch, which):
    labels, boxes = census_batch[0][:6], census_batch[1][:6]
    thr = C.threshold_from_batch(a480, boxes)
    high, low = (thr, 0.3) if which == 'high' else (0.7, thr)
    check_anchors(a480, labels, boxes, high=high, low=low, what='threshold ' + which)


def test_anchors_128_images_7_boxes_border(a480):
    labels, boxes = C.make_ground_truth(21, 128, a480, max_boxes=7)
    labels[5], boxes[5] = labels[5][:1].repeat(7), np.repeat(boxes[5][:1], 7, 0) + f32(0.01) * np.arange(7, dtype=f32)[:, None]
    assert max(len(l) for l in labels) == 7
    check_anchors(a480, labels, boxes, border=0.1, what='N=128 G=7 480 border 0.1')


def test_anchors_3_images_512_boxes_800(a800):
    labels, boxes = C.make_ground_truth(22, 3, a800, max_boxes=512, min_boxes=300)
    labels[1], boxes[1] = np.resize(labels[1], 512), np.resize(boxes[1], (512, 4))       # G = 512, with repeated boxes
    check_anchors(a800, labels, boxes, what='N=3 G=512 800')


def test_anchors_64_images_42_boxes_no_ground_truth_and_poison(a480):
    from xdet import targets as T
    labels, boxes = C.make_ground_truth(23, 64, a480, max_boxes=42)
    labels[0], boxes[0] = np.resize(labels[0], 42), np.concatenate([boxes[0], C.random_boxes(np.random.default_rng(1), 42)])[:42]
    gl, gb, ng = T.ground_truth(labels, boxes)
    assert gl.shape[1] == 42
    pl, pb = np.ones_like(gl), np.full_like(gb, np.nan)
    for n in range(64):
        pl[n, :ng[n]], pb[n, :ng[n]] = gl[n, :ng[n]], gb[n, :ng[n]]
    ng[3] = ng[40] = 0
    l, t, s = check_anchors(a480, pl, pb, ng, what='N=64 G=42 480 poison')
    assert not l[3].any() and not t[40].any() and not s[3].any()


def test_anchors_one_image_one_box_800_border(a800):
    check_anchors(a800, [np.array([7])], [np.array([[0.2, 0.3, 0.6, 0.55]], f32)], border=0.1, what='N=1 G=1 800 border 0.1')


# ---- ROIs ----------------------------------------------------------------------------------------------------------

def check_rois(rois, labels, boxes, n_gt=None, P=64, fg_fraction=0.25, seed=0, image_ids=None, what='', **kw):
    from xdet import targets as T
    args = dict(ROI)
    args.update(kw)
    want = T.host_encode_rois(rois, labels, boxes, n_gt, rois_per_image=P, fg_fraction=fg_fraction, seed=seed,
                              image_ids=image_ids, return_all=True, **args)
    got = T.encode_rois(rois, labels, boxes, n_gt, rois_per_image=P, fg_fraction=fg_fraction, seed=seed, image_ids=image_ids,
                        return_all=True, **args)
    o_r, o_t, o_l, o_s, o_i, cnt, a_l, a_t, a_s = got
    assert np.array_equal(a_l, want[6]) and np.array_equal(bits(a_s), bits(want[8])), what
    assert_targets(a_t, want[7], what + ' (all)')
    assert np.array_equal(cnt, want[5]), (what, cnt, want[5])
    assert np.array_equal(o_i, want[4]), what
    assert np.array_equal(o_l, want[2]) and np.array_equal(bits(o_s), bits(want[3])) and np.array_equal(bits(o_r), bits(want[0])), what
    assert_targets(o_t, want[1], what)
    plain = T.encode_rois(rois, labels, boxes, n_gt, rois_per_image=P, fg_fraction=fg_fraction, seed=seed, image_ids=image_ids,
                          **args)
    for a, b in zip(plain, got[:6]):           # the workspace's own per-candidate arrays give the same
        assert np.array_equal(a, b, equal_nan=True), what
    return got


@pytest.mark.parametrize('R,P', [(300, 64), (1800, 256), (1800, 64), (300, 256)])
def test_rois(a480, R, P):
    labels, boxes = C.make_ground_truth(31 + R, 16, a480)
    labels[2][::2] = 0                      # background entries among the ground truth
    labels[5][:] = 0                        # none left
    labels[6], boxes[6] = labels[6][:0], boxes[6][:0]
    rois = C.make_rois(R, 16, R, boxes)
    got = check_rois(rois, labels, boxes, P=P, seed=R + P, what='R=%d P=%d' % (R, P))
    cnt = got[5]
    assert cnt[5, 3] == 0 and cnt[6, 3] == 0 and np.all(got[2][5] == -1) and np.all(got[4][6] == -1)
    assert (cnt[:, 3] > 0).sum() >= 13


def test_rois_short_exact_and_long_sampling(a480):
    from xdet import targets as T
    labels, boxes = C.make_ground_truth(41, 8, a480)
    rois = C.make_rois(9, 8, 300, boxes)
    base = T.host_encode_rois(rois, labels, boxes, rois_per_image=64, **ROI)[5]
    n_pos, n_neg = int(base[0, 1]), int(base[0, 2])
    assert n_pos >= 4 and n_neg >= 64
    seen = set()
    for P, frac, kw in ((64, 0.25, {}), (64, 1.0, {}), (256, 0.25, {}), (64, 0.0, {}),
                        (n_pos * 2, 0.5, {}),                           # |pos| == exp_fg in image 0
                        (256, 0.25, dict(bg_low_thr=0.3)), (200, 0.1, dict(bg_low_thr=0.45))):   # few negatives: the tail
        got = check_rois(rois, labels, boxes, P=P, fg_fraction=frac, seed=3, what='P=%d frac=%g %r' % (P, frac, kw), **kw)
        exp_fg = T.expected_fg(P, frac)
        for M, p, q, k in got[5]:
            seen.add(('fg_short' if p < exp_fg else 'fg_exact' if p == exp_fg else 'fg_long'))
            seen.add('bg_short' if q < P - min(p, exp_fg) else 'bg_long')
            if 0 < k < P:
                seen.add('tail_remainder' if (P - k) % k else 'tail_whole')
    print(sorted(seen))
    assert {'fg_short', 'fg_exact', 'fg_long', 'bg_short', 'bg_long', 'tail_remainder'} <= seen


def test_rois_image_ids_make_the_draw_independent_of_the_batch_order(a480):
    from xdet import targets as T
    labels, boxes = C.make_ground_truth(43, 8, a480)
    rois = C.make_rois(10, 8, 300, boxes)
    ids = np.arange(100, 108)
    a = check_rois(rois, labels, boxes, seed=5, image_ids=ids, what='ids')
    perm = np.array([3, 0, 7, 1, 6, 2, 5, 4])
    b = T.encode_rois(rois[perm], [labels[i] for i in perm], [boxes[i] for i in perm], rois_per_image=64, seed=5,
                      image_ids=ids[perm], **ROI)
    for x, y in zip(a[:6], b):
        assert np.array_equal(x[perm], y, equal_nan=True)
    c = T.encode_rois(rois[perm], [labels[i] for i in perm], [boxes[i] for i in perm], rois_per_image=64, seed=5, **ROI)
    assert not np.array_equal(a[4][perm], c[4])          # without ids the index within the call is the key


def test_rois_from_a_device_tensor(a480):
    from xdet import targets as T
    from xdet.runtime import DeviceTensor, to_device
    labels, boxes = C.make_ground_truth(44, 4, a480)
    rois = C.make_rois(11, 4, 300, boxes)
    buf = to_device(rois)
    got = T.encode_rois(DeviceTensor(buf.ptr, (4, 300, 1, 4), 4, owner=buf), labels, boxes, rois_per_image=64, **ROI)
    want = T.encode_rois(rois, labels, boxes, rois_per_image=64, **ROI)
    for x, y in zip(got, want):
        assert np.array_equal(x, y, equal_nan=True)
    enc = T.AnchorEncoder([a480], 21, [0.], 0.7, 0.3, [1., 1., 1., 1.], 0.53, 0.5, 0.)
    r, t, l, s = enc.ext_encode_rois(rois, labels, boxes, 64, 0.25, 0.1)
    assert l.dtype == np.int64 and np.array_equal(r, want[0]) and np.array_equal(l, want[2])
    back = enc.ext_decode_rois(r, t)
    gl, gb, _ = T.ground_truth(labels, boxes)
    pos = l > 0
    assert pos.any()
    for n in range(4):
        d = np.abs(back[n][pos[n]][:, None, :] - gb[n][None, :, :]).max(-1).min(-1)
        assert d.max() <= 1e-5                     # a positive's target decodes to one of the image's boxes
    ll, tt, ss, bb, nl = enc.encode_all_anchors(labels[0], boxes[0])
    w = T.host_encode_anchors(a480, [labels[0]], [boxes[0]])
    assert nl == 1 and ll[0].dtype == np.int64 and np.array_equal(ll[0], w[0][0]) and np.array_equal(bits(ss[0]), bits(w[2][0]))
    assert bb[0].shape == (19800, 4)


# ---- control words -------------------------------------------------------------------------------------------------

def test_second_call_with_fewer_images_in_the_same_workspace(a480):
    """the row maxima and counts of the first call must not leak into a call with a smaller N (and other data) that
    reuses the workspace and the output arrays"""
    from xdet import targets as T
    from xdet._lib import lib, check
    from xdet.runtime import to_device, to_host, DeviceBuffer, synchronize
    sc4 = (ctypes.c_float * 4)(1, 1, 1, 1)
    yref, xref, href, wref = a480
    yx = to_device(np.stack([yref.reshape(-1), xref.reshape(-1)], 1).astype(f32))
    hw = to_device(np.stack([href, wref], 1).astype(f32))
    G, R, P, n_a = 16, 300, 64, 19800
    ws = DeviceBuffer(lib().xdet_targets_workspace_bytes(8, R + G, G))
    d_l, d_t, d_s = DeviceBuffer(8 * n_a * 4), DeviceBuffer(8 * n_a * 16), DeviceBuffer(8 * n_a * 4)
    o = [DeviceBuffer(8 * P * 16), DeviceBuffer(8 * P * 16), DeviceBuffer(8 * P * 4), DeviceBuffer(8 * P * 4), DeviceBuffer(8 * P * 4),
         DeviceBuffer(8 * 16)]
    for N, seed in ((8, 51), (3, 52)):
        labels, boxes = C.make_ground_truth(seed, N, a480)
        gl, gb, ng = T.ground_truth(labels, boxes)
        pl, pb = np.zeros((N, G), np.int32), np.zeros((N, G, 4), f32)
        pl[:, :gl.shape[1]], pb[:, :gl.shape[1]] = gl, gb
        rois = C.make_rois(seed, N, R, boxes)
        dev = [to_device(x) for x in (pl, pb, ng, rois)]
        check(lib().xdet_encode_anchors(yx.ptr, hw.ptr, 30, 30, 22, 0., dev[0].ptr, dev[1].ptr, dev[2].ptr, N, G, .7, .3, sc4, ws.ptr,
                                        d_l.ptr, d_t.ptr, d_s.ptr, None))
        synchronize()
        want = T.host_encode_anchors(a480, pl, pb, ng)
        assert np.array_equal(to_host(d_l.ptr, (N, n_a), np.int32), want[0])
        assert np.array_equal(bits(to_host(d_s.ptr, (N, n_a), f32)), bits(want[2]))
        check(lib().xdet_encode_rois(dev[3].ptr, R, dev[0].ptr, dev[1].ptr, dev[2].ptr, N, G, .1, .53, .5, 0., sc4, P, .25, 9, None,
                                     ws.ptr, o[0].ptr, o[1].ptr, o[2].ptr, o[3].ptr, o[4].ptr, o[5].ptr, None, None, None, None))
        synchronize()
        w = T.host_encode_rois(rois, pl, pb, ng, rois_per_image=P, seed=9, **ROI)
        assert np.array_equal(to_host(o[4].ptr, (N, P), np.int32), w[4])
        assert np.array_equal(to_host(o[5].ptr, (N, 4), np.int32), w[5])
        assert np.array_equal(to_host(o[2].ptr, (N, P), np.int32), w[2])
        assert np.array_equal(bits(to_host(o[3].ptr, (N, P), f32)), bits(w[3]))


# ---- through the net -----------------------------------------------------------------------------------------------

def test_get_proposals_training_branch(lh_weights):
    from xdet import model as M, ops, targets as T
    from xdet import weights as W
    from xdet.model import LightHeadDetector
    S, R, pre = 256, 1800, 5000
    det = LightHeadDetector(lh_weights, image_size=S, max_batch=2, rpn_pre_nms_top_n=pre, rpn_post_nms_top_n=R)
    # stage by stage: the whole forward's detection part takes at most 1024 ROIs per image, the proposal stage 1800
    with det.scope():
        mid, _ = M.XceptionBody(W.synthetic_images(2, S, seed=3), 21, is_training=False, data_format='channels_first')
        cls, box = M.get_rpn(mid, 22, False, 'channels_first', 'rpn_head')
        obj, rb = M.rpn_decode(cls, box)
        props = M.get_proposals(obj, rb, None, pre, R, 0.7, 16. / 480, False, 'channels_first')
    assert props.shape == (2, R, 4)
    assert np.array_equal(bits(props), bits(ops.get_proposals(obj, rb, None, pre, R, 0.7, 16. / 480, False, 'channels_first')))
    labels, boxes = C.make_ground_truth(61, 2, C.anchors(S))
    for n in range(2):                         # boxes the proposals can match: some of the forward's own
        boxes[n][0] = props[n, 0]
        boxes[n][-1] = props[n, 5]
    enc = T.AnchorEncoder([C.anchors(S)], 21, [0.], 0.7, 0.3, [1., 1., 1., 1.], 0.53, 0.5, 0.)
    seen = {}

    def encode_fn(rois):
        seen['rois'] = rois
        return enc.ext_encode_rois(rois, labels, boxes, 64, 0.25, 0.1, seed=4)
    with det.scope():
        same = M.get_proposals(obj, rb, None, pre, R, 0.7, 16. / 480, False, 'channels_first')
        assert np.array_equal(bits(same), bits(props))
        r, t, l, s = M.get_proposals(obj, rb, encode_fn, pre, R, 0.7, 16. / 480, True, 'channels_first')
    assert not isinstance(seen['rois'], np.ndarray)        # handed over on the device
    w = T.host_encode_rois(props, labels, boxes, rois_per_image=64, seed=4, **ROI)
    assert np.array_equal(bits(r), bits(w[0])) and np.array_equal(l, w[2]) and np.array_equal(bits(s), bits(w[3]))
    assert_targets(t, w[1], 'through the net')
    assert (l > 0).any() and l.dtype == np.int64
    r2, t2, l2, s2 = ops.get_proposals(obj, rb, encode_fn, pre, R, 0.7, 16. / 480, True, 'channels_first')
    assert np.array_equal(bits(r2), bits(r)) and np.array_equal(l2, l)
    with pytest.raises(ValueError):
        ops.get_proposals(obj, rb, None, pre, R, 0.7, 16. / 480, True, 'channels_first')
