"""Training targets: what the reference's training script does with the ground truth before any loss.

  AnchorEncoder.encode_all_anchors     preprocessing/anchor_manipulator.py:118-171, 319-335
  AnchorEncoder.ext_encode_rois        preprocessing/anchor_manipulator.py:337-445 (the encode_fn of get_proposals'
                                       training branch, net/xception_body.py:446-448)
  iou_matrix / do_dual_max_match       preprocessing/anchor_manipulator.py:22-94 (ignore_between, gt_max_first: the only
                                       form the reference calls)

Two statements of one contract (include/xdet.h):
  encode_anchors / encode_rois             the GPU path (csrc/targets.hip: xdet_encode_anchors / xdet_encode_rois)
  host_encode_anchors / host_encode_rois   NumPy, f32 in the reference's operation order -- what the kernels are compared
                                           with, and usable by data-pipeline code on a box without a GPU
`AnchorEncoder` carries the reference's class, method names and argument order on top of the GPU path.

The contract in short.  Overlap O[g,a] = IoU (0 where the union is 0) times the 0/1 inside mask of candidate a
(min >= -b, max < f32(1 + b)).  best_g[a] / mv[a]: FIRST maximum of column a; m = -1 below `low`, -2 in [low, high), else
best_g.  best_a[g]: FIRST maximum of row g (an all-zero row points at candidate 0).  A candidate some box points at takes
the first maximum over g of O[g,a] * [best_a[g] == a] (box 0 when all are zero) and that box's overlap as its score.
label = glabels[max(m,0)] * [m > -1] - [m < -1]; target = [m > -1] * encoding of box max(m,0) against the candidate.
No ground truth: labels 0, targets and scores 0.  tf.random_shuffle is replaced by a defined order: shuffle(S) = S ordered
by (key, element), key = shuffle_keys(seed, image, element, stream).
"""
import numpy as np

f32 = np.float32
MAX_GT = 512            # ground-truth boxes per image
MAX_CANDIDATES = 8192   # R + G, and rois_per_image


# ---- the shuffle ---------------------------------------------------------------------------------------------------

def _mix(x):
    """32-bit finaliser (integers only): x ^= x >> 16; x *= 0x7FEB352D; x ^= x >> 15; x *= 0x846CA68B; x ^= x >> 16"""
    m = np.uint64(0xFFFFFFFF)
    x = np.asarray(x, np.uint64) & m
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x7FEB352D)) & m
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x846CA68B)) & m
    return x ^ (x >> np.uint64(16))


def shuffle_keys(seed, image, elements, stream=0):
    """key = mix(mix(mix(seed ^ 0x9E3779B9) + image) ^ (2 * element + stream)) in 32-bit unsigned arithmetic -> uint32.
    stream 0: candidates (fg and bg are disjoint, one stream serves both); stream 1: positions of the up-sampling tail.
    For a fixed (seed, image, stream) the key is a bijection of the element: keys of one shuffle never tie."""
    m = np.uint64(0xFFFFFFFF)
    word = _mix((_mix(np.uint64(int(seed) & 0xFFFFFFFF) ^ np.uint64(0x9E3779B9)) + np.uint64(int(image) & 0xFFFFFFFF)) & m)
    e = np.asarray(elements, np.uint64)
    return _mix(word ^ ((np.uint64(2) * e + np.uint64(int(stream))) & m)).astype(np.uint32)


def shuffle(elements, seed, image, stream=0):
    """`elements` ordered by (key, element) ascending"""
    e = np.asarray(elements, np.int64).reshape(-1)
    return e[np.lexsort((e, shuffle_keys(seed, image, e, stream)))]


# ---- the NumPy statement ---------------------------------------------------------------------------------------------

def _border(allowed_border):
    b = f32(allowed_border)
    return f32(-b), f32(1.0 + float(b))         # 1 + b formed in double, rounded once


def anchor_boxes(anchor):
    """(yref [H,W], xref [H,W], href [A], wref [A]) -> corners [HWA,4] (center2point) and reference points [HWA,4]
    (yref, xref, href, wref), index (y * W + x) * A + k"""
    yref, xref, href, wref = (np.asarray(v, f32) for v in anchor)
    y, x = yref.reshape(-1, 1), xref.reshape(-1, 1)
    h, w = href.reshape(1, -1), wref.reshape(1, -1)
    two = f32(2.)
    box = np.stack([y - h / two, x - w / two, y + h / two, x + w / two], -1).reshape(-1, 4).astype(f32)
    ref = np.stack(np.broadcast_arrays(y, x, h, w), -1).reshape(-1, 4).astype(f32)
    return box, ref


def roi_refs(boxes):
    """point2center: (ymin + h / 2, xmin + w / 2, h, w)"""
    b = np.asarray(boxes, f32).reshape(-1, 4)
    h, w = b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]
    return np.stack([b[:, 0] + h / f32(2.), b[:, 1] + w / f32(2.), h, w], -1).astype(f32)


def overlap_matrix(gbboxes, cand, lo, hi):
    """iou_matrix(gbboxes, cand) * inside mask -> f32 [G,M]"""
    g = np.asarray(gbboxes, f32).reshape(-1, 4)
    c = np.asarray(cand, f32).reshape(-1, 4)
    h = np.maximum(np.minimum(g[:, None, 2], c[None, :, 2]) - np.maximum(g[:, None, 0], c[None, :, 0]), f32(0.))
    w = np.maximum(np.minimum(g[:, None, 3], c[None, :, 3]) - np.maximum(g[:, None, 1], c[None, :, 1]), f32(0.))
    inter = h * w
    area_g = (g[:, 3] - g[:, 1]) * (g[:, 2] - g[:, 0])
    area_c = (c[:, 3] - c[:, 1]) * (c[:, 2] - c[:, 0])
    union = (area_g[:, None] + area_c[None, :]) - inter
    with np.errstate(divide='ignore', invalid='ignore'):
        iou = np.where(union == 0, f32(0.), inter / union).astype(f32)
    inside = (c[:, 0] >= lo) & (c[:, 1] >= lo) & (c[:, 2] < hi) & (c[:, 3] < hi)
    return iou * inside.astype(f32)[None, :]


def dual_max_match(O, high, low):
    """do_dual_max_match(O, high, low) -> (match i64 [M]: box, -1 negative, -2 ignored; scores f32 [M])"""
    high, low = f32(high), f32(low)
    best_g = O.argmax(0)
    mv = O[best_g, np.arange(O.shape[1])]          # the value AT the first maximum (the sign of a zero included)
    m = np.where(mv < low, -1, best_g)
    m = np.where((mv < high) & (mv >= low), -2, m)
    best_a = O.argmax(1)
    cols = np.unique(best_a)
    sub = O[:, cols] * (best_a[:, None] == cols[None, :]).astype(f32)
    fm = sub.argmax(0)
    m[cols] = fm
    scores = mv.copy()
    scores[cols] = O[fm, cols]
    return m.astype(np.int64), scores.astype(f32)


def encode_boxes(gbboxes, refs, scaling):
    """the regression encoding of box i against reference point i, f32 in the reference's order -> [M,4]"""
    g = np.asarray(gbboxes, f32).reshape(-1, 4)
    r = np.asarray(refs, f32).reshape(-1, 4)
    s = np.asarray(scaling, f32).reshape(4)
    two = f32(2.)
    gcy, gcx = (g[:, 2] + g[:, 0]) / two, (g[:, 3] + g[:, 1]) / two
    gh, gw = g[:, 2] - g[:, 0], g[:, 3] - g[:, 1]
    with np.errstate(divide='ignore', invalid='ignore'):
        return np.stack([((gcy - r[:, 0]) / r[:, 2]) / s[0], ((gcx - r[:, 1]) / r[:, 3]) / s[1],
                         np.log(gh / r[:, 2]) / s[2], np.log(gw / r[:, 3]) / s[3]], -1).astype(f32)


def _match_encode(glabels, gbboxes, cand, refs, lo, hi, high, low, scaling):
    """one image -> labels i32 [M], targets f32 [M,4], scores f32 [M], match i64 [M]"""
    M = cand.shape[0]
    if glabels.shape[0] == 0:
        return np.zeros(M, np.int32), np.zeros((M, 4), f32), np.zeros(M, f32), np.full(M, -1, np.int64)
    m, scores = dual_max_match(overlap_matrix(gbboxes, cand, lo, hi), high, low)
    k = np.maximum(m, 0)
    labels = glabels[k].astype(np.int64) * (m > -1) - (m < -1)
    with np.errstate(invalid='ignore'):
        targets = (m > -1).astype(f32)[:, None] * encode_boxes(gbboxes[k], refs, scaling)
    return labels.astype(np.int32), targets.astype(f32), scores, m


def ground_truth(labels, bboxes, n_gt=None):
    """a list of per-image arrays, or arrays already padded to [N,G] / [N,G,4] (evaluation.pad_ground_truth) with n_gt [N]
    (None: all G) -> (glabels i32 [N,G], gbboxes f32 [N,G,4], n_gt i32 [N])"""
    from ._lib import InvalidArgumentError
    if isinstance(labels, (list, tuple)):
        if len(labels) != len(bboxes):
            raise InvalidArgumentError(-1, 'labels of %d images but boxes of %d' % (len(labels), len(bboxes)))
        from .evaluation import pad_ground_truth
        gl, gb, _, ng = pad_ground_truth([(l, b, np.zeros(np.asarray(l).reshape(-1).shape[0])) for l, b in zip(labels, bboxes)])
        return gl, gb, ng
    gl = np.ascontiguousarray(labels, np.int32)
    if gl.ndim != 2:
        raise InvalidArgumentError(-1, 'ground truth must be a list per image or padded to [N,G] / [N,G,4], got labels %r' % (gl.shape,))
    N, G = gl.shape
    gb = np.ascontiguousarray(np.asarray(bboxes, f32).reshape(N, G, 4))
    ng = np.full(N, G, np.int32) if n_gt is None else np.ascontiguousarray(n_gt, np.int32).reshape(N)
    return gl, gb, ng


def host_encode_anchors(anchor, labels, bboxes, n_gt=None, allowed_border=0., high_thr=0.7, low_thr=0.3,
                        prior_scaling=(1., 1., 1., 1.), return_match=False):
    """encode_anchor for one layer's anchors (yref, xref, href, wref) and a batch of images
    -> (labels i32 [N,HWA], targets f32 [N,HWA,4], scores f32 [N,HWA]) (+ match i64 [N,HWA])"""
    gl, gb, ng = ground_truth(labels, bboxes, n_gt)
    cand, refs = anchor_boxes(anchor)
    lo, hi = _border(allowed_border)
    out = []
    for n in range(gl.shape[0]):
        k = int(min(max(ng[n], 0), gl.shape[1]))
        out.append(_match_encode(gl[n, :k], gb[n, :k], cand, refs, lo, hi, high_thr, low_thr, prior_scaling))
    res = tuple(np.stack([o[i] for o in out]) for i in range(4))
    return res if return_match else res[:3]


def expected_fg(rois_per_image, fg_fraction):
    """tf.round(tf.cast(rois_per_image, f32) * fg_fraction): half to even"""
    return int(np.rint(f32(rois_per_image) * f32(fg_fraction)))


def sample_rois(labels, scores, rois_per_image, fg_fraction, bg_low_thr=0., seed=0, image=0):
    """the sampler of ext_encode_rois on one image's per-candidate labels and scores
    -> (index i64 [rois_per_image] into the candidates (-1 everywhere when nothing can be kept), (n_pos, n_neg, n_keep))"""
    labels, scores = np.asarray(labels), np.asarray(scores, f32)
    exp_fg = expected_fg(rois_per_image, fg_fraction)
    pos = np.flatnonzero(labels > 0)
    neg = np.flatnonzero((labels == 0) & (scores > f32(bg_low_thr)))
    fg = pos if len(pos) < exp_fg else shuffle(pos, seed, image, 0)[:exp_fg]
    exp_bg = rois_per_image - min(len(pos), exp_fg)
    bg = neg if len(neg) < exp_bg else shuffle(neg, seed, image, 0)[:exp_bg]
    keep = np.concatenate([fg, bg]).astype(np.int64)
    n_keep = len(keep)
    counts = (len(pos), len(neg), n_keep)
    if n_keep == 0:
        return np.full(rois_per_image, -1, np.int64), counts
    if n_keep < rois_per_image:
        left = rois_per_image - n_keep
        idx = np.concatenate([np.tile(np.arange(n_keep), left // n_keep + 1),
                              shuffle(np.arange(n_keep), seed, image, 1)[:left % n_keep]])
        keep = keep[idx]
    return keep, counts


def host_encode_rois(rois, labels, bboxes, n_gt=None, allowed_border=0.1, fg_thr=0.5, bg_high_thr=0.5, bg_low_thr=0.,
                     prior_scaling=(1., 1., 1., 1.), rois_per_image=256, fg_fraction=0.25, seed=0, image_ids=None,
                     return_all=False):
    """ext_encode_rois: rois f32 [N,R,4] -> (out_rois [N,P,4], out_targets [N,P,4], out_labels i32 [N,P], out_scores [N,P],
    out_index i32 [N,P], counts i32 [N,4]: M, n_pos, n_neg, n_keep), P = rois_per_image; return_all adds the unsampled
    (all_labels i32 [N,R+G], all_targets [N,R+G,4], all_scores [N,R+G], all_match i64 [N,R+G]) (behind M: label -1, zeros)"""
    gl, gb, ng = ground_truth(labels, bboxes, n_gt)
    rois = np.asarray(rois, f32)
    N, R = rois.shape[:2]
    G, P = gl.shape[1], int(rois_per_image)
    lo, hi = _border(allowed_border)
    ids = np.arange(N) if image_ids is None else np.asarray(image_ids).reshape(N)
    o_r, o_t = np.zeros((N, P, 4), f32), np.zeros((N, P, 4), f32)
    o_l, o_s, o_i = np.full((N, P), -1, np.int32), np.zeros((N, P), f32), np.full((N, P), -1, np.int32)
    counts = np.zeros((N, 4), np.int32)
    a_l, a_t, a_s = np.full((N, R + G), -1, np.int32), np.zeros((N, R + G, 4), f32), np.zeros((N, R + G), f32)
    a_m = np.full((N, R + G), -1, np.int64)
    for n in range(N):
        k = int(min(max(ng[n], 0), G))
        sel = gl[n, :k] > 0
        l, b = gl[n, :k][sel], gb[n, :k][sel]
        cand = np.concatenate([rois[n], b], 0)
        M = cand.shape[0]
        lab, tg, sc, m = _match_encode(l, b, cand, roi_refs(cand), lo, hi, fg_thr, bg_high_thr, prior_scaling)
        a_l[n, :M], a_t[n, :M], a_s[n, :M], a_m[n, :M] = lab, tg, sc, m
        idx, (n_pos, n_neg, n_keep) = sample_rois(lab, sc, P, fg_fraction, bg_low_thr, seed, int(ids[n]))
        counts[n] = (M, n_pos, n_neg, n_keep)
        if n_keep:
            o_r[n], o_t[n], o_l[n], o_s[n], o_i[n] = cand[idx], tg[idx], lab[idx], sc[idx], idx
    out = (o_r, o_t, o_l, o_s, o_i, counts)
    return out + (a_l, a_t, a_s, a_m) if return_all else out


# ---- the GPU path (csrc/targets.hip) ---------------------------------------------------------------------------------

def _scaling(prior_scaling):
    import ctypes
    s = [float(v) for v in prior_scaling]
    if len(s) != 4:
        from ._lib import InvalidArgumentError
        raise InvalidArgumentError(-1, 'prior_scaling must have 4 entries, got %d' % len(s))
    return (ctypes.c_float * 4)(*s)


def _device_ground_truth(labels, bboxes, n_gt):
    """True when the ground truth is already in device memory (all three DeviceTensors, shapes agreeing)"""
    from .runtime import DeviceTensor
    from ._lib import InvalidArgumentError
    dev = [isinstance(v, DeviceTensor) for v in (labels, bboxes, n_gt)]
    if not any(dev):
        return False
    if not all(dev) or bboxes.shape != (labels.shape[0], labels.shape[3], 1, 4) or n_gt.shape[3] != labels.shape[0]:
        raise InvalidArgumentError(-1, 'device ground truth: labels [N,1,1,G], bboxes [N,G,1,4] and n_gt [1,1,1,N] expected')
    return True


def _h(stream):
    return stream.handle if stream is not None else None


def _buffer(buffers, key, nbytes, fill=None):
    """a DeviceBuffer of at least nbytes: a new one (buffers None), or the caller's dict entry `key`, made on first use and
    kept there, so a driver that passes the same dict every step allocates once.  fill: a host array uploaded into a new one"""
    from .runtime import DeviceBuffer, to_device
    b = buffers.get(key) if buffers is not None else None
    if b is None or b.nbytes < nbytes:
        b = to_device(fill) if fill is not None else DeviceBuffer(max(nbytes, 16))
        if buffers is not None:
            buffers[key] = b
    return b


def encode_anchors(anchor, labels, bboxes, n_gt=None, allowed_border=0., high_thr=0.7, low_thr=0.3,
                   prior_scaling=(1., 1., 1., 1.), stream=None, keep_device=False, buffers=None):
    """host_encode_anchors on the GPU (xdet_encode_anchors) -> (labels i32 [N,HWA], targets f32 [N,HWA,4], scores f32 [N,HWA]).
    labels / bboxes / n_gt may be the DeviceTensors of augment.preprocess_train ([N,1,1,G] i32, [N,G,1,4] f32, [1,1,1,N]
    i32): they are read where they are, nothing is copied to the host.
    keep_device=True (default off): the three stay where the kernel wrote them -- DeviceTensors [N,HWA,1,1] (labels i32),
    [N,HWA,1,4] and [N,HWA,1,1], each carrying the stream it was made on (`made_on`) -- and the call does not synchronise;
    losses.rpn_loss reads labels and targets in place.  buffers (a dict the caller keeps, default None): the anchors' device
    copy, the workspace and the three results live in it from the first call on, so later calls allocate and upload nothing
    -- and overwrite what the earlier call returned."""
    from ._lib import lib, check
    from .runtime import to_device, to_host, DeviceBuffer, DeviceTensor, synchronize
    on_device = _device_ground_truth(labels, bboxes, n_gt)
    if on_device:
        N, G = labels.shape[0], labels.shape[3]
    else:
        gl, gb, ng = ground_truth(labels, bboxes, n_gt)
        N, G = gl.shape
    yref, xref, href, wref = (np.asarray(v, f32) for v in anchor)
    Hh, Ww = yref.shape if yref.ndim == 2 else (yref.size, 1)
    A = int(href.size)
    sc4 = _scaling(prior_scaling)
    args = (float(allowed_border),)
    thr = (float(high_thr), float(low_thr))
    if min(N, G, Hh, Ww, A) <= 0 or G > MAX_GT or not np.all(np.isfinite(args + thr)):
        # the library states the error; nothing is allocated for a call that cannot run
        check(lib().xdet_encode_anchors(None, None, Hh, Ww, A, args[0], None, None, None, N, G, thr[0], thr[1], sc4, None, None,
                                        None, None, None))
    n_a = Hh * Ww * A
    if buffers is not None and 'yx' in buffers:          # (the anchors of an encoder do not change)
        yx, hw = buffers['yx'], buffers['hw']
    else:
        yx = _buffer(buffers, 'yx', 0, np.stack([yref.reshape(-1), xref.reshape(-1)], 1).astype(f32))
        hw = _buffer(buffers, 'hw', 0, np.stack([href.reshape(-1), wref.reshape(-1)], 1).astype(f32))
    d_gl, d_gb, d_ng = (labels, bboxes, n_gt) if on_device else (to_device(gl), to_device(gb), to_device(ng))
    ws = _buffer(buffers, 'ws', lib().xdet_targets_workspace_bytes(N, 0, G))
    d_l, d_t, d_s = _buffer(buffers, 'labels', N * n_a * 4), _buffer(buffers, 'targets', N * n_a * 16), _buffer(buffers, 'scores', N * n_a * 4)
    check(lib().xdet_encode_anchors(yx.ptr, hw.ptr, Hh, Ww, A, args[0], d_gl.ptr, d_gb.ptr, d_ng.ptr, N, G, thr[0], thr[1], sc4,
                                    ws.ptr, d_l.ptr, d_t.ptr, d_s.ptr, _h(stream)))
    if keep_device:
        res = []
        for buf, w in ((d_l, 1), (d_t, 4), (d_s, 1)):
            t = DeviceTensor(buf.ptr, (N, n_a, 1, w), w, owner=buf)
            t.made_on, t._inputs = stream, (yx, hw, d_gl, d_gb, d_ng, ws)
            res.append(t)
        return tuple(res)
    synchronize(stream)
    return (to_host(d_l.ptr, (N, n_a), np.int32), to_host(d_t.ptr, (N, n_a, 4), f32), to_host(d_s.ptr, (N, n_a), f32))


def encode_rois(rois, labels, bboxes, n_gt=None, allowed_border=0.1, fg_thr=0.5, bg_high_thr=0.5, bg_low_thr=0.,
                prior_scaling=(1., 1., 1., 1.), rois_per_image=256, fg_fraction=0.25, seed=0, image_ids=None,
                return_all=False, stream=None, keep_device=False, buffers=None):
    """host_encode_rois on the GPU (xdet_encode_rois), same results in the same order.  rois: NumPy [N,R,4], or a
    DeviceTensor / DeviceBuffer holding N * R * 4 floats (then `rois` is not copied; give R through its shape [N,R,1,4] or
    [N,R,4]) -- e.g. the `proposals` buffer of a LightHeadDetector.
    keep_device=True: the results stay where the kernel wrote them and the call does not synchronise -- out_rois and
    out_targets as f32 DeviceTensors [N,P,1,4] (ld 4), out_labels (i32), out_scores and out_index (i32) [N,P,1,1], counts
    (i32) [N,1,1,4] (with return_all the three unsampled arrays likewise), each carrying the stream it was made on
    (`made_on`): model.get_head on a head_rois detector copies the ROIs device to device, losses.HeadLoss reads labels and
    targets in place.  DeviceTensor.numpy() reads f32: download an i32 one with runtime.to_host(t.ptr, shape, np.int32).
    labels / bboxes / n_gt may be the DeviceTensors of augment.preprocess_train, read where they are (as encode_anchors takes
    them).  buffers (a dict the caller keeps, default None): the workspace and every result live in it from the first call on
    -- later calls allocate nothing and overwrite what the earlier call returned."""
    from ._lib import lib, check, InvalidArgumentError
    from .runtime import to_device, to_host, DeviceBuffer, DeviceTensor, synchronize
    gt_on_device = _device_ground_truth(labels, bboxes, n_gt)
    if gt_on_device:
        N, G = labels.shape[0], labels.shape[3]
    else:
        gl, gb, ng = ground_truth(labels, bboxes, n_gt)
        N, G = gl.shape
    if isinstance(rois, DeviceTensor):
        shp = tuple(rois.shape)
        if shp[0] != N or shp[-1] != 4 or rois.ld != 4:
            raise InvalidArgumentError(-1, 'device rois must be [N,R,(1,)4] with N = %d, got %r' % (N, shp))
        R = int(np.prod(shp[1:-1]))
        d_r = rois
    else:
        r = np.ascontiguousarray(rois, f32)
        if r.ndim != 3 or r.shape[0] != N or r.shape[2] != 4:
            raise InvalidArgumentError(-1, 'rois must be [N,R,4] with N = %d, got %r' % (N, r.shape))
        R = r.shape[1]
        d_r = None
    P = int(rois_per_image)
    sc4 = _scaling(prior_scaling)
    fl = (float(allowed_border), float(fg_thr), float(bg_high_thr), float(bg_low_thr))
    fgf = float(fg_fraction)
    if (min(N, G, R) <= 0 or G > MAX_GT or R + G > MAX_CANDIDATES or not 0 < P <= MAX_CANDIDATES or not 0. <= fgf <= 1.
            or not np.all(np.isfinite(fl))):
        check(lib().xdet_encode_rois(None, R, None, None, None, N, G, fl[0], fl[1], fl[2], fl[3], sc4, P, fgf, 0, None, None,
                                     None, None, None, None, None, None, None, None, None, None))
    if d_r is None:
        d_r = to_device(r)
    d_gl, d_gb, d_ng = (labels, bboxes, n_gt) if gt_on_device else (to_device(gl), to_device(gb), to_device(ng))
    d_ids = to_device(np.ascontiguousarray(image_ids, np.int32).reshape(N)) if image_ids is not None else None
    M = R + G
    ws = _buffer(buffers, 'ws', lib().xdet_targets_workspace_bytes(N, M, G))
    o_r, o_t = _buffer(buffers, 'rois', N * P * 16), _buffer(buffers, 'targets', N * P * 16)
    o_l, o_s, o_i, o_c = (_buffer(buffers, 'labels', N * P * 4), _buffer(buffers, 'scores', N * P * 4), _buffer(buffers, 'index', N * P * 4),
                          _buffer(buffers, 'counts', N * 16))
    a_l = a_t = a_s = None
    if return_all:
        a_l, a_t, a_s = DeviceBuffer(N * M * 4), DeviceBuffer(N * M * 16), DeviceBuffer(N * M * 4)
    check(lib().xdet_encode_rois(d_r.ptr, R, d_gl.ptr, d_gb.ptr, d_ng.ptr, N, G, fl[0], fl[1], fl[2], fl[3], sc4, P, fgf,
                                 int(seed) & 0xFFFFFFFF, d_ids.ptr if d_ids is not None else None, ws.ptr, o_r.ptr, o_t.ptr,
                                 o_l.ptr, o_s.ptr, o_i.ptr, o_c.ptr, a_l.ptr if a_l else None, a_t.ptr if a_t else None,
                                 a_s.ptr if a_s else None, _h(stream)))
    if keep_device:
        # (nothing waits here: the inputs and the workspace stay referenced by the first result until it goes)
        held = (d_r, d_gl, d_gb, d_ng, d_ids, ws)
        outs = [(o_r, (N, P, 1, 4)), (o_t, (N, P, 1, 4)), (o_l, (N, P, 1, 1)), (o_s, (N, P, 1, 1)), (o_i, (N, P, 1, 1)), (o_c, (N, 1, 1, 4))]
        if return_all:
            outs += [(a_l, (N, M, 1, 1)), (a_t, (N, M, 1, 4)), (a_s, (N, M, 1, 1))]
        res = []
        for buf, shp in outs:
            t = DeviceTensor(buf.ptr, shp, shp[-1], owner=buf)
            t.made_on, t._inputs = stream, held
            res.append(t)
        return tuple(res)
    synchronize(stream)
    out = (to_host(o_r.ptr, (N, P, 4), f32), to_host(o_t.ptr, (N, P, 4), f32), to_host(o_l.ptr, (N, P), np.int32),
           to_host(o_s.ptr, (N, P), f32), to_host(o_i.ptr, (N, P), np.int32), to_host(o_c.ptr, (N, 4), np.int32))
    if return_all:
        out += (to_host(a_l.ptr, (N, M), np.int32), to_host(a_t.ptr, (N, M, 4), f32), to_host(a_s.ptr, (N, M), f32))
    return out


class AnchorEncoder(object):
    """preprocessing/anchor_manipulator.py:96-683 with the reference's method names and argument order; encoding runs on
    the GPU (xdet_encode_anchors / xdet_encode_rois), decoding through the existing ops.  anchors: the list of per-layer
    (yref, xref, href, wref) that ops.AnchorCreator.get_all_anchors returns."""

    def __init__(self, anchors, num_classes, allowed_borders, positive_threshold, ignore_threshold, prior_scaling,
                 rpn_fg_thres=0.5, rpn_bg_high_thres=0.5, rpn_bg_low_thres=0.):
        self._anchors = anchors
        self._num_classes = num_classes
        self._allowed_borders = allowed_borders
        self._positive_threshold = positive_threshold
        self._ignore_threshold = ignore_threshold
        self._prior_scaling = prior_scaling
        self._rpn_fg_thres = rpn_fg_thres
        self._rpn_bg_high_thres = rpn_bg_high_thres
        self._rpn_bg_low_thres = rpn_bg_low_thres

    def center2point(self, center_y, center_x, height, width):
        two = f32(2.)
        return center_y - height / two, center_x - width / two, center_y + height / two, center_x + width / two

    def point2center(self, ymin, xmin, ymax, xmax):
        height, width = (ymax - ymin), (xmax - xmin)
        return ymin + height / f32(2.), xmin + width / f32(2.), height, width

    def encode_all_anchors(self, labels, bboxes, n_gt=None, stream=None, keep_device=False):
        """labels / bboxes: one image ([g] / [g,4], as in the reference's input pipeline), a list of per-image arrays, or
        padded [N,G] / [N,G,4] with n_gt -> (labels, targets, scores, anchor_boxes, n_layers), lists per layer; labels int64.
        A single image gives arrays without the batch axis.
        keep_device=True (default off): labels (i32), targets and scores stay as xdet_encode_anchors wrote them, DeviceTensors
        per layer with the batch axis (encode_anchors(..., keep_device=True)); nothing is downloaded or synchronised, and from
        the second call on nothing is allocated: the encoder keeps the buffers, so a call overwrites what the last returned."""
        if _device_ground_truth(labels, bboxes, n_gt):      # augment.preprocess_train's outputs, as they are
            single, (gl, gb, ng) = False, (labels, bboxes, n_gt)
        else:
            single = not isinstance(labels, (list, tuple)) and np.asarray(labels).ndim == 1
            if single:
                labels, bboxes = [np.asarray(labels)], [np.asarray(bboxes, f32).reshape(-1, 4)]
            gl, gb, ng = ground_truth(labels, bboxes, n_gt)
        out_l, out_t, out_s, out_b = [], [], [], []
        for layer, anchor in enumerate(self._anchors):
            if keep_device:
                kept = self.__dict__.setdefault('_device_buffers', {}).setdefault(layer, {})
                l, t, s = encode_anchors(anchor, gl, gb, ng, self._allowed_borders[layer], self._positive_threshold,
                                         self._ignore_threshold, self._prior_scaling, stream, True, kept)
                out_l.append(l)
                out_t.append(t)
                out_s.append(s)
                out_b.append(anchor_boxes(anchor)[0])
                continue
            l, t, s = encode_anchors(anchor, gl, gb, ng, self._allowed_borders[layer], self._positive_threshold,
                                     self._ignore_threshold, self._prior_scaling, stream)
            l = l.astype(np.int64)
            out_l.append(l[0] if single else l)
            out_t.append(t[0] if single else t)
            out_s.append(s[0] if single else s)
            out_b.append(anchor_boxes(anchor)[0])
        return out_l, out_t, out_s, out_b, len(self._anchors)

    def ext_encode_rois(self, all_rois, all_labels, all_bboxes, rois_per_image, fg_fraction, allowed_border,
                        head_prior_scaling=[1., 1., 1., 1.], seed=0, n_gt=None, image_ids=None, stream=None, keep_device=False,
                        buffers=None):
        """-> (rois f32 [N,P,4], targets f32 [N,P,4], labels int64 [N,P], scores f32 [N,P]).  all_rois: NumPy [N,R,4] or a
        DeviceTensor (no host copy then); the shuffle is the defined one (module docstring), chosen by `seed`.
        keep_device=True: the four come back as encode_rois(..., keep_device=True) leaves them, DeviceTensors (labels i32) with
        no synchronisation: model.get_head on a head_rois detector and losses.HeadLoss take them as they are."""
        r, t, l, s = encode_rois(all_rois, all_labels, all_bboxes, n_gt, allowed_border, self._rpn_fg_thres,
                                 self._rpn_bg_high_thres, self._rpn_bg_low_thres, head_prior_scaling, rois_per_image,
                                 fg_fraction, seed, image_ids, False, stream, keep_device, buffers)[:4]
        if keep_device:
            return r, t, l, s
        return r, t, l.astype(np.int64), s

    def decode_all_anchors(self, pred_location, squeeze_inner=False):
        """pred_location: per layer [N,Hh,Ww,4A] (or [N,Hh,Ww,A,4]) -> per layer boxes [N,Hh,Ww,A,4] ([N,HWA,4] squeezed)
        through xdet_rpn_decode.  That kernel has the eval path's prior_scaling (1,1,1,1); an encoder built with another
        one raises here."""
        from . import ops
        from ._lib import InvalidArgumentError
        assert len(self._anchors) == len(pred_location), 'predict location not equals to anchor priors.'
        if tuple(float(v) for v in self._prior_scaling) != (1., 1., 1., 1.):
            raise InvalidArgumentError(-1, 'decode_all_anchors: the decode kernel has the eval prior_scaling (1,1,1,1)')
        out = []
        for anchor, loc in zip(self._anchors, pred_location):
            Hh, Ww = np.asarray(anchor[0]).shape
            A = int(np.asarray(anchor[2]).size)
            loc = np.asarray(loc, f32).reshape(-1, Hh, Ww, 4 * A)
            _, boxes = ops.rpn_decode(np.zeros(loc.shape[:3] + (2 * A,), f32), loc, anchor)
            out.append(boxes if squeeze_inner else boxes.reshape(-1, Hh, Ww, A, 4))
        return out

    def ext_decode_rois(self, proposals_roi, pred_location, head_prior_scaling=[1., 1., 1., 1.]):
        from . import ops
        return ops.ext_decode_rois(proposals_roi, pred_location, tuple(head_prior_scaling))
