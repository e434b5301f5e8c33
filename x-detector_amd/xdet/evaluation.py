"""F4: eval bookkeeping behind the detector -- host-side NumPy, same names and
semantics as the reference so a detections dict from `LightHeadDetector.forward` can be scored
exactly the way `bboxes_eval` continues (light_head_rfcn_eval.py:288-338):

  bboxes_jaccard / bboxes_matching     utility/eval_helper.py:671-781
  StreamingTpFp (streaming_tp_fp_arrays), precision_recall,
  average_precision_voc07 / _voc12      utility/metrics.py:102-261
  VOC_LABELS                            dataset/dataset_common.py:27-55

The same bookkeeping on the GPU, behind the forward without a host round trip per step (csrc/evalmatch.hip):
  bboxes_matching_batch                 utility/eval_helper.py:700-830  (xdet_bboxes_matching)
  GpuStreamingTpFp                      streaming_tp_fp_arrays on the device (xdet_tpfp_*); the PR curve and the APs
                                        are the host functions below, fed with its records
"""
import numpy as np

VOC_CLASSES = ('aeroplane', 'bicycle', 'bird', 'boat', 'bottle', 'bus', 'car', 'cat', 'chair', 'cow', 'diningtable',
               'dog', 'horse', 'motorbike', 'person', 'pottedplant', 'sheep', 'sofa', 'train', 'tvmonitor')
_CATEGORY = dict(aeroplane='Vehicle', bicycle='Vehicle', bird='Animal', boat='Vehicle', bottle='Indoor', bus='Vehicle',
                 car='Vehicle', cat='Animal', chair='Indoor', cow='Animal', diningtable='Indoor', dog='Animal',
                 horse='Animal', motorbike='Vehicle', person='Person', pottedplant='Indoor', sheep='Animal',
                 sofa='Indoor', train='Vehicle', tvmonitor='Indoor')
VOC_LABELS = {'none': (0, 'Background')}
VOC_LABELS.update({name: (i + 1, _CATEGORY[name]) for i, name in enumerate(VOC_CLASSES)})


def label2name_table():
    """light_head_rfcn_eval.py:169-174."""
    return {pair[0]: name for name, pair in VOC_LABELS.items()}


def bboxes_jaccard(bbox_ref, bboxes):
    """IoU of one reference box against N boxes, 0 where the union is not positive (safe_divide)."""
    b = np.asarray(bboxes, np.float32).reshape(-1, 4)
    r = np.asarray(bbox_ref, np.float32).reshape(4)
    h = np.maximum(np.minimum(b[:, 2], r[2]) - np.maximum(b[:, 0], r[0]), 0.)
    w = np.maximum(np.minimum(b[:, 3], r[3]) - np.maximum(b[:, 1], r[1]), 0.)
    inter = h * w
    union = -inter + (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1]) + (r[2] - r[0]) * (r[3] - r[1])
    out = np.zeros_like(inter)
    np.divide(inter, union, out=out, where=union > 0)
    return out


def bboxes_matching(label, scores, bboxes, glabels, gbboxes, gdifficults, matching_threshold=0.5):
    """Greedy Pascal-VOC matching of one class's detections (already sorted by score) against the
    ground truth: -> (n_gbboxes, tp[N], fp[N]).  A detection whose best-IoU ground truth is
    `difficult` is neither TP nor FP."""
    scores = np.asarray(scores)
    bboxes = np.asarray(bboxes, np.float32).reshape(-1, 4)
    glabels = np.asarray(glabels).reshape(-1)
    gbboxes = np.asarray(gbboxes, np.float32).reshape(-1, 4)
    gdiff = np.asarray(gdifficults).reshape(-1).astype(bool)
    same = glabels == label
    n_gbboxes = int(np.count_nonzero(same & ~gdiff))
    n = scores.shape[0]
    tp = np.zeros(n, bool)
    fp = np.zeros(n, bool)
    gmatch = np.zeros(glabels.shape[0], bool)
    if glabels.shape[0] == 0:
        return n_gbboxes, tp, np.ones(n, bool) & False
    for i in range(n):
        jac = bboxes_jaccard(bboxes[i], gbboxes) * same
        k = int(np.argmax(jac))
        match = jac[k] > matching_threshold
        if gdiff[k]:
            continue
        tp[i] = match and not gmatch[k]
        fp[i] = gmatch[k] or not match
        if match:
            gmatch[k] = True
    return n_gbboxes, tp, fp


class StreamingTpFp(object):
    """streaming_tp_fp_arrays: accumulates, per class, the ground-truth count and the
    (score, tp, fp) triplets of every detection that is TP or FP (score > 1e-4)."""
    def __init__(self, remove_zero_scores=True):
        self.remove_zero_scores = remove_zero_scores
        self.nobjects = {}
        self.scores, self.tp, self.fp = {}, {}, {}

    def update(self, c, num_gbboxes, tp, fp, scores):
        tp = np.asarray(tp, bool).reshape(-1)
        fp = np.asarray(fp, bool).reshape(-1)
        scores = np.asarray(scores, np.float32).reshape(-1)
        mask = tp | fp
        if self.remove_zero_scores:
            mask &= scores > 1e-4
            tp, fp, scores = tp[mask], fp[mask], scores[mask]
        self.nobjects[c] = self.nobjects.get(c, 0) + int(num_gbboxes)
        for store, v in ((self.scores, scores), (self.tp, tp), (self.fp, fp)):
            store[c] = np.concatenate([store[c], v]) if c in store else v

    def update_image(self, detections, glabels, gbboxes, gdifficults, matching_threshold=0.5):
        """detections: {class: (scores[K], boxes[K,4])} as returned by the detector for one image."""
        for c, (s, b) in detections.items():
            n, tp, fp = bboxes_matching(c, s, b, glabels, gbboxes, gdifficults, matching_threshold)
            self.update(c, n, tp, fp, s)

    def average_precisions(self):
        out07, out12 = {}, {}
        for c in self.nobjects:
            p, r = precision_recall(self.nobjects[c], self.tp[c], self.fp[c], self.scores[c])
            out07[c], out12[c] = average_precision_voc07(p, r), average_precision_voc12(p, r)
        return out07, out12


def precision_recall(num_gbboxes, tp, fp, scores):
    order = np.argsort(-np.asarray(scores, np.float32), kind='stable')
    ctp = np.cumsum(np.asarray(tp, bool)[order].astype(np.float64))
    cfp = np.cumsum(np.asarray(fp, bool)[order].astype(np.float64))
    recall = ctp / num_gbboxes if num_gbboxes > 0 else np.zeros_like(ctp)
    den = ctp + cfp
    precision = np.divide(ctp, den, out=np.zeros_like(ctp), where=den > 0)
    return precision, recall


def average_precision_voc12(precision, recall):
    p = np.concatenate([[0.], np.asarray(precision, np.float64), [0.]])
    r = np.concatenate([[0.], np.asarray(recall, np.float64), [1.]])
    p = np.maximum.accumulate(p[::-1])[::-1]
    return float(np.sum(p[1:] * (r[1:] - r[:-1])))


def average_precision_voc07(precision, recall):
    p = np.concatenate([np.asarray(precision, np.float64), [0.]])
    r = np.concatenate([np.asarray(recall, np.float64), [np.inf]])
    return float(sum(p[r >= t].max() / 11. for t in np.arange(0., 1.1, 0.1)))


# ---- the GPU path (csrc/evalmatch.hip) -------------------------------------------------------------------------

def pad_ground_truth(ground_truths, min_boxes=1):
    """[(glabels[g], gbboxes[g,4], gdifficults[g]) per image] -> (glabels i32 [N,G], gbboxes f32 [N,G,4],
    gdifficults u8 [N,G], n_gt i32 [N]) with G = the largest count (at least min_boxes), zero padded."""
    n_gt = np.array([np.asarray(g[0]).reshape(-1).shape[0] for g in ground_truths], np.int32)
    G = max(int(n_gt.max()) if len(n_gt) else 0, min_boxes)
    N = len(ground_truths)
    glabels, gbboxes, gdiff = np.zeros((N, G), np.int32), np.zeros((N, G, 4), np.float32), np.zeros((N, G), np.uint8)
    for i, (l, b, d) in enumerate(ground_truths):
        k = n_gt[i]
        glabels[i, :k] = np.asarray(l).reshape(-1)
        gbboxes[i, :k] = np.asarray(b, np.float32).reshape(-1, 4)
        gdiff[i, :k] = np.asarray(d).reshape(-1) != 0
    return glabels, gbboxes, gdiff, n_gt


def _padded(glabels, gbboxes, gdifficults, n_gt, N):
    glabels = np.ascontiguousarray(glabels, np.int32)
    if glabels.ndim != 2 or glabels.shape[0] != N:
        from ._lib import InvalidArgumentError
        raise InvalidArgumentError(-1, 'ground truth must be padded to [N,G] / [N,G,4] / [N,G] with N = %d, got glabels %r'
                                   % (N, glabels.shape))
    G = glabels.shape[1]
    gbboxes = np.ascontiguousarray(np.asarray(gbboxes, np.float32).reshape(N, G, 4))
    gdiff = np.ascontiguousarray(np.asarray(gdifficults).reshape(N, G) != 0).astype(np.uint8)
    n_gt = np.full(N, G, np.int32) if n_gt is None else np.ascontiguousarray(n_gt, np.int32).reshape(N)
    return glabels, gbboxes, gdiff, n_gt


def bboxes_matching_batch(det_scores, det_boxes, glabels, gbboxes, gdifficults, n_gt=None, matching_threshold=0.5):
    """eval_helper.bboxes_matching_batch on the GPU: det_scores [N,C,K], det_boxes [N,C,K,4] (class label c + 1, as the
    detector writes them), ground truth padded to [N,G] with n_gt[n] boxes in image n (None: all G) ->
    (n_gbboxes i32 [N,C], tp bool [N,C,K], fp bool [N,C,K]); per (image, class) exactly bboxes_matching's results."""
    from ._lib import lib, check, InvalidArgumentError
    from .runtime import to_device, to_host, DeviceBuffer, synchronize
    s = np.ascontiguousarray(det_scores, np.float32)
    b = np.ascontiguousarray(det_boxes, np.float32)
    if s.ndim != 3 or b.shape != s.shape + (4,):
        raise InvalidArgumentError(-1, 'det_scores must be [N,C,K] and det_boxes [N,C,K,4], got %r / %r' % (s.shape, b.shape))
    N, C, K = s.shape
    gl, gb, gd, ng = _padded(glabels, gbboxes, gdifficults, n_gt, N)
    G = gl.shape[1]
    thr = float(matching_threshold)
    if min(N, C, K, G) <= 0 or G > 512 or not np.isfinite(thr):
        check(lib().xdet_bboxes_matching(None, None, N, C, K, None, None, None, None, G, thr, None, None, None, None))
    bufs = [to_device(a) for a in (s, b, gl, gb, gd, ng)]
    tp, fp, nb = DeviceBuffer(N * C * K), DeviceBuffer(N * C * K), DeviceBuffer(N * C * 4)
    check(lib().xdet_bboxes_matching(bufs[0].ptr, bufs[1].ptr, N, C, K, bufs[2].ptr, bufs[3].ptr, bufs[4].ptr, bufs[5].ptr, G,
                                     thr, tp.ptr, fp.ptr, nb.ptr, None))
    synchronize()
    return (to_host(nb.ptr, (N, C), np.int32), to_host(tp.ptr, (N, C, K), np.uint8).astype(bool),
            to_host(fp.ptr, (N, C, K), np.uint8).astype(bool))


def _ordered(scores, tp, image_id, slot):
    """one class's records in (image_id, slot) order (stable: equal keys keep their arrival order)"""
    order = np.lexsort((slot, image_id))
    return scores[order], tp[order], image_id[order], slot[order]


class GpuStreamingTpFp(object):
    """streaming_tp_fp_arrays with the matching and the accumulation on the GPU (xdet_tpfp_*): update() enqueues the
    matcher and the append behind the forward and returns; records() is the one call that waits.  Per class it holds the
    object count and a record (score, tp, image_id, slot) for every detection that is TP or FP with score > 1e-4.
    Records are ordered by (image_id, slot) before the stable score sort of precision_recall, so the APs do not depend on
    how the images were batched or sharded, and equal those of StreamingTpFp fed image by image in image_id order."""

    def __init__(self, num_classes=21, topk=200, capacity_per_class=1 << 20):
        self.C, self.K, self.capacity = int(num_classes) - 1, int(topk), int(capacity_per_class)
        self._handle = None
        self._staged = None
        self._stream = None          # the stream of the last update: what a read waits for
        self._dev = {}
        self._shards = []            # merged-in host records: (records {c: (scores, tp, image_id, slot)}, nobjects {c: n}, bad)

    # ---- device side ----
    def _acc(self):
        if self._handle is None:
            import ctypes
            from ._lib import lib, check, c_void_p
            h = c_void_p()
            check(lib().xdet_tpfp_create(ctypes.byref(h), self.C, self.K, self.capacity))
            self._handle = h
        return self._handle

    def _upload(self, key, a, stream):
        from ._lib import lib, check
        from .runtime import DeviceBuffer, _host
        buf = self._dev.get(key)
        if buf is None or buf.nbytes < a.nbytes:
            buf = self._dev[key] = DeviceBuffer(max(a.nbytes, 2 * buf.nbytes if buf is not None else 16))
        check(lib().xdet_memcpy_h2d(buf.ptr, _host(a), a.nbytes, stream.handle if stream is not None else None))
        return buf

    def stage(self, image_ids, ground_truths, stream=None):
        """copy the image ids and the ground truth of the next update() to the device on `stream`.  ground_truths: a list
        of (glabels, gbboxes, gdifficults) per image, or the padded tuple (glabels [N,G], gbboxes [N,G,4], gdifficults
        [N,G], n_gt [N] or None)."""
        ids = np.ascontiguousarray(image_ids, np.int32).reshape(-1)
        N = ids.shape[0]
        if isinstance(ground_truths, tuple) and len(ground_truths) == 4:
            gl, gb, gd, ng = _padded(*ground_truths, N=N)
        else:
            if len(ground_truths) != N:
                from ._lib import InvalidArgumentError
                raise InvalidArgumentError(-1, '%d image ids but ground truth of %d images' % (N, len(ground_truths)))
            gl, gb, gd, ng = pad_ground_truth(ground_truths)
        host = {'ids': ids, 'glabels': gl, 'gbboxes': gb, 'gdiff': gd, 'n_gt': ng}
        dev = {k: self._upload(k, a, stream) for k, a in host.items()}
        self._staged = (N, gl.shape[1], dev, host)       # (the host arrays stay referenced until the next stage())

    def enqueue(self, det_scores, det_boxes, n, matching_threshold=0.5, stream=None):
        """xdet_tpfp_update on `stream` with what stage() copied: det_scores / det_boxes are device pointers.  Updates of
        one accumulator belong on one stream: reads wait for the stream of the last update."""
        from ._lib import lib, check, InvalidArgumentError
        from .runtime import _ptr
        if self._staged is None or self._staged[0] != n:
            raise InvalidArgumentError(-1, 'update of %d images without their staged ground truth' % n)
        _, G, dev, _ = self._staged
        self._stream = stream
        check(lib().xdet_tpfp_update(self._acc(), _ptr(det_scores), _ptr(det_boxes), n, dev['ids'].ptr, dev['glabels'].ptr,
                                     dev['gbboxes'].ptr, dev['gdiff'].ptr, dev['n_gt'].ptr, G, float(matching_threshold),
                                     stream.handle if stream is not None else None))

    def update(self, source, det_boxes=None, image_ids=None, ground_truths=None, n=None, matching_threshold=0.5, stream=None):
        """source: a LightHeadDetector (the detections of its last forward, on its stream), or det_scores as a device
        pointer / DeviceBuffer (with det_boxes and n), or NumPy det_scores [n,C,K] with NumPy det_boxes.  Returns at
        once: nothing is read back."""
        if hasattr(source, '_det_scores'):
            n, stream = n or source._N, source.stream
            scores, boxes = source._det_scores, source._det_boxes
        elif isinstance(source, np.ndarray):
            s = np.ascontiguousarray(source, np.float32)
            b = np.ascontiguousarray(det_boxes, np.float32)
            if s.ndim != 3 or s.shape[1:] != (self.C, self.K) or b.shape != s.shape + (4,):
                from ._lib import InvalidArgumentError
                raise InvalidArgumentError(-1, 'det_scores %r / det_boxes %r, want [n,%d,%d] / [n,%d,%d,4]'
                                           % (s.shape, b.shape, self.C, self.K, self.C, self.K))
            n = s.shape[0]
            scores, boxes = self._upload('det_scores', s, stream), self._upload('det_boxes', b, stream)
        else:
            scores, boxes = source, det_boxes
        self.stage(image_ids, ground_truths, stream)
        self.enqueue(scores, boxes, n, matching_threshold, stream)

    def reset(self, stream=None):
        from ._lib import lib, check
        check(lib().xdet_tpfp_reset(self._acc(), stream.handle if stream is not None else None))
        self._shards = []

    def _read_device(self, stream=None):
        import ctypes
        from ._lib import lib, check
        from .runtime import _host
        C = self.C
        counts, nobj = np.zeros(C, np.int32), np.zeros(C, np.int64)
        bad, ovf = ctypes.c_int(), ctypes.c_int()
        stream = stream if stream is not None else self._stream
        h = stream.handle if stream is not None else None
        check(lib().xdet_tpfp_read(self._acc(), _host(counts), _host(nobj), ctypes.byref(bad), ctypes.byref(ovf), 0, None, None,
                                   None, None, h))
        total = int(counts.sum())
        s, t = np.zeros(max(total, 1), np.float32), np.zeros(max(total, 1), np.uint8)
        ids, slots = np.zeros(max(total, 1), np.int32), np.zeros(max(total, 1), np.int32)
        c2 = np.zeros(C, np.int32)
        check(lib().xdet_tpfp_read(self._acc(), _host(c2), _host(nobj), ctypes.byref(bad), ctypes.byref(ovf), total, _host(s),
                                   _host(t), _host(ids), _host(slots), h))
        assert np.array_equal(counts, c2), 'the accumulator was updated while it was read'
        at = np.concatenate([[0], np.cumsum(counts)])
        recs = {c + 1: (s[at[c]:at[c + 1]], t[at[c]:at[c + 1]].astype(bool), ids[at[c]:at[c + 1]], slots[at[c]:at[c + 1]])
                for c in range(C)}
        return recs, {c + 1: int(nobj[c]) for c in range(C)}, int(bad.value), int(ovf.value)

    # ---- host side ----
    @classmethod
    def from_host_records(cls, records, nobjects, num_classes=21, topk=200, bad_images=0):
        """an accumulator that holds only host records ({class: (scores, tp, image_id, slot)}, {class: objects}): a shard
        computed elsewhere, ready for merge()"""
        a = cls(num_classes, topk, 1)
        a._shards.append(({c: tuple(np.asarray(x) for x in r) for c, r in records.items()}, dict(nobjects), int(bad_images)))
        return a

    def _parts(self, stream=None):
        parts, overflow = list(self._shards), 0
        if self._handle is not None:
            recs, nobj, bad, overflow = self._read_device(stream)
            parts.append((recs, nobj, bad))
        return parts, overflow

    def state(self, stream=None):
        """(records {class: (scores, tp, fp, image_id, slot)} ordered by (image_id, slot), nobjects {class: n}, bad_images,
        overflow) of this accumulator and everything merged into it; waits for the enqueued updates"""
        parts, overflow = self._parts(stream)
        out, nobjects, bad = {}, {}, 0
        for c in range(1, self.C + 1):
            cols = [p[0][c] for p in parts if c in p[0]]
            if cols:
                s, t, i, k = (np.concatenate([np.asarray(x[j]) for x in cols]) for j in range(4))
            else:
                s, t, i, k = np.zeros(0, np.float32), np.zeros(0, bool), np.zeros(0, np.int32), np.zeros(0, np.int32)
            s, t, i, k = _ordered(s.astype(np.float32), t.astype(bool), i.astype(np.int64), k.astype(np.int64))
            out[c] = (s, t, ~t, i, k)
            nobjects[c] = sum(int(p[1].get(c, 0)) for p in parts)
        for p in parts:
            bad += p[2]
        return out, nobjects, bad, overflow

    def records(self, stream=None):
        return self.state(stream)[0]

    @property
    def nobjects(self):
        return self.state()[1]

    @property
    def bad_images(self):
        return self.state()[2]

    @property
    def overflow(self):
        return bool(self.state()[3])

    def merge(self, *others):
        """take over the records of other accumulators (shards of one dataset: other streams, other processes through
        from_host_records); host side.  Returns self."""
        for o in others:
            parts, overflow = o._parts()
            if overflow:
                from ._lib import XdetError
                raise XdetError(-3, 'merge: a shard overflowed its capacity_per_class')
            self._shards.extend(parts)
        return self

    def average_precisions(self, allow_bad=False):
        """-> ({class: AP VOC07}, {class: AP VOC12}) through precision_recall / average_precision_voc07 / _voc12"""
        from ._lib import XdetError
        recs, nobjects, bad, overflow = self.state()
        if overflow:
            raise XdetError(-3, 'GpuStreamingTpFp: a class received more records than capacity_per_class = %d; the '
                                'accumulated records are incomplete' % self.capacity)
        if bad and not allow_bad:
            raise XdetError(-4, 'non-finite network outputs / out-of-range activations for %d image(s) (bad_images): they '
                                'were not scored; pass allow_bad=True to score the dataset without them' % bad)
        out07, out12 = {}, {}
        for c, (s, tp, fp, _, _) in recs.items():
            p, r = precision_recall(nobjects[c], tp, fp, s)
            out07[c], out12[c] = average_precision_voc07(p, r), average_precision_voc12(p, r)
        return out07, out12

    def summary(self, allow_bad=False):
        """the figures the reference's eval reports (light_head_rfcn_eval.py:304-338): per-class APs and their mean over
        the classes of the accumulator"""
        ap07, ap12 = self.average_precisions(allow_bad)
        return {'AP_VOC07': ap07, 'AP_VOC12': ap12, 'mAP_VOC07': float(sum(ap07.values()) / len(ap07)),
                'mAP_VOC12': float(sum(ap12.values()) / len(ap12))}

    def __del__(self):
        try:
            if self._handle is not None:
                from ._lib import lib
                lib().xdet_tpfp_destroy(self._handle)
        except Exception:
            pass


# ---- drawing (utility/draw_toolbox.py:72-104) -------------------------------------------------
# Tableau-20 palette, white for background -- the colour table the reference indexes by class id
COLORS_TABLEAU = [(255, 255, 255), (31, 119, 180), (174, 199, 232), (255, 127, 14), (255, 187, 120), (44, 160, 44),
                  (152, 223, 138), (214, 39, 40), (255, 152, 150), (148, 103, 189), (197, 176, 213), (140, 86, 75),
                  (196, 156, 148), (227, 119, 194), (247, 182, 210), (127, 127, 127), (199, 199, 199),
                  (188, 189, 34), (219, 219, 141), (23, 190, 207), (158, 218, 229)]


def bboxes_draw_on_img(img, classes, scores, bboxes, thickness=2):
    """Same contract as the reference's bboxes_draw_on_img: img uint8 [H,W,3] (modified in place and
    returned), bboxes (ymin,xmin,ymax,xmax) in [0,1]; class 0 and boxes thinner than one pixel are
    skipped; corners are `int(coord * shape)`.  Rectangles are rasterised with NumPy (no OpenCV here;
    the outline is `thickness` pixels wide, centred on the box edge like cv2.rectangle); the
    'name/score%' caption is drawn with Pillow when it is importable and silently omitted otherwise."""
    h, w = img.shape[:2]
    names = label2name_table()
    try:
        from PIL import Image, ImageDraw
    except Exception:
        Image = ImageDraw = None
    captions = []
    for i in range(bboxes.shape[0]):
        c = int(classes[i])
        if c < 1:
            continue
        y0, x0 = int(bboxes[i][0] * h), int(bboxes[i][1] * w)
        y1, x1 = int(bboxes[i][2] * h), int(bboxes[i][3] * w)
        if y1 - y0 < 1 or x1 - x0 < 1:
            continue
        color = np.asarray(COLORS_TABLEAU[c % len(COLORS_TABLEAU)], img.dtype)
        lo, hi = thickness // 2, (thickness + 1) // 2

        def span(a, n):
            return slice(max(a - lo, 0), min(a + hi, n))
        ys, xs = slice(max(y0 - lo, 0), min(y1 + hi, h)), slice(max(x0 - lo, 0), min(x1 + hi, w))
        img[span(y0, h), xs] = color
        img[span(y1, h), xs] = color
        img[ys, span(x0, w)] = color
        img[ys, span(x1, w)] = color
        captions.append((x0, max(y0 - 12, 0), '%s/%.1f%%' % (names.get(c, str(c)), float(scores[i]) * 100), tuple(int(v) for v in color)))
    if ImageDraw is not None and captions:
        pil = Image.fromarray(img)
        d = ImageDraw.Draw(pil)
        for x, y, s, col in captions:
            box = d.textbbox((x, y), s)
            d.rectangle(box, fill=col)
            d.text((x, y), s, fill=(255, 255, 255))
        img[...] = np.asarray(pil)
    return img
