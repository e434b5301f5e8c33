"""Inputs of tests/test_gpu_detect_tail.py (the detection tail in the net's form: csrc/detect.hip head_decode_probs_* and
bboxes_eval_kernel<true>) and a plain float64 statement of the decode + softmax pass.  tests/test_detect_tail_math.py proves
on the CPU that each input has the property it is named for.

Every builder returns read-only arrays and caches them: the tests share one copy."""
import numpy as np

f32 = np.float32

# valid ROIs per class of `banded` (class c: V_BANDED[c - 1]): 0, 1, the 64-candidate blocks of the column-bit mask, 2*nms_topk
# +- 1 for nms_topk = 200 (and 2*64, 2*128 for smaller ones), 512 / 513 where rank counting gives way to the bitonic sort, R
V_BANDED = [0, 1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 399, 400, 401, 511, 512, 513, 1023, 1024]
LATTICE_THRESHOLDS = [f32(0.25), f32(1.0 / 3.0), f32(0.5)]

_cache = {}


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


def clustered_boxes(rng, n, cnt, centres=40, jitter=0.02, scale=0.3, inside=False):
    """boxes in tight groups (tests/test_gpu_proposals.py _clustered): many IoU > thr pairs and long suppression chains.
    inside: centres drawn from (0.25, 0.75) and corners clipped to [1/256, 255/256] -- every box strictly inside (0, 1) with
    sides of at least ~0.06"""
    lo, hi = (0.25, 0.75) if inside else (0.1, 0.9)
    c = rng.uniform(lo, hi, (n, centres, 2))
    hw = rng.uniform(0.08, scale, (n, centres, 2))
    k = rng.integers(0, centres, (n, cnt))
    cy = np.take_along_axis(c[..., 0], k, 1) + rng.normal(0, jitter, (n, cnt))
    cx = np.take_along_axis(c[..., 1], k, 1) + rng.normal(0, jitter, (n, cnt))
    h = np.take_along_axis(hw[..., 0], k, 1) * np.exp(rng.normal(0, 0.1, (n, cnt)))
    w = np.take_along_axis(hw[..., 1], k, 1) * np.exp(rng.normal(0, 0.1, (n, cnt)))
    boxes = np.stack([cy - h / 2, cx - w / 2, cy + h / 2, cx + w / 2], -1)
    if inside:
        boxes = np.clip(boxes, 1.0 / 256, 255.0 / 256)
    return boxes.astype(f32)


def banded(R=1024, V=None):
    """-> (logits [R, len(V) + 1], boxes [R, 4]).  The background logit is 0; class c has logit 0 for the ROIs r < V[c - 1]
    and -30 elsewhere: its probability there is 1 / (the number of zero logits of the row) up to e^-30, at least 1/21, and
    e^-30 / . elsewhere -- exactly V[c - 1] ROIs above any threshold between.  A row's zero logits only depend on which V
    lie above r, so a class's scores take at most as many values as there are distinct V below its own: exact ties in
    runs of up to hundreds of ROIs, in ascending score with r (the LAST ROIs of the band rank first)."""
    V = list(V_BANDED if V is None else V)
    key = ('banded', R, tuple(V))
    if key not in _cache:
        rng = np.random.default_rng(20 + R)
        r = np.arange(R)[:, None]
        logits = np.where(r < np.asarray(V)[None, :], 0.0, -30.0)
        logits = np.concatenate([np.zeros((R, 1)), logits], 1).astype(f32)
        boxes = clustered_boxes(rng, 1, R, inside=True)[0]
        _cache[key] = _frozen(logits, boxes)
    return _cache[key]


def lattice(R=256, num_classes=21):
    """-> (logits [R, num_classes], boxes [R, 4]).  Corners are multiples of 1/64 and sides 4, 8 or 16 sixty-fourths, on few
    enough positions that many pairs nest or overlap by half: areas, intersections and unions are small integers over 4096,
    exact in float32, and IoU = 1/4, 1/3 (as float32(1/3): the correctly rounded quotient) and 1/2 all occur.  Logits: every
    class has about 100 ROIs at +4 +- noise over a floor of -4, so ~100 valid ROIs per class with distinct scores."""
    key = ('lattice', R, num_classes)
    if key not in _cache:
        rng = np.random.default_rng(64)
        side = rng.choice([4, 8, 16], (R, 2))
        y0 = 8 + 4 * rng.integers(0, 7, R)
        x0 = 8 + 4 * rng.integers(0, 7, R)
        boxes = (np.stack([y0, x0, y0 + side[:, 0], x0 + side[:, 1]], -1) / 64.0).astype(f32)
        logits = np.full((R, num_classes), -4.0)
        logits[:, 0] = 0.0
        for c in range(1, num_classes):
            on = rng.permutation(R)[:100]
            logits[on, c] = 4.0 + rng.uniform(-1, 1, 100)
        _cache[key] = _frozen(logits.astype(f32), boxes)
    return _cache[key]


def random_logits(n, R, num_classes, spread, seed=0):
    """-> (rois [n, R, 4], cls_reg [n * R, num_classes + 4], logits [n, R, num_classes]): clustered ROIs clipped to the frame,
    normal logits * spread and normal regression values * 0.2 (cls_reg = the head's row: logits, then the regression)"""
    key = ('random', n, R, num_classes, spread, seed)
    if key not in _cache:
        rng = np.random.default_rng(1000 * num_classes + 10 * R + n + seed)
        rois = np.clip(clustered_boxes(rng, n, R, centres=12, jitter=0.03), 0.0, 1.0).astype(f32)
        logits = (rng.standard_normal((n, R, num_classes)) * spread).astype(f32)
        reg = (rng.standard_normal((n, R, 4)) * 0.2).astype(f32)
        cls_reg = np.concatenate([logits, reg], -1).reshape(n * R, num_classes + 4)
        _cache[key] = _frozen(rois, np.ascontiguousarray(cls_reg), logits)
    return _cache[key]


def reference_decode_probs(rois, cls_reg, num_classes):
    """float64: rois [n, 4], cls_reg [n, >= num_classes + 4] -> (boxes [n, 4], probs [n, num_classes]), plain formulas
    (anchor_manipulator.py:671-683 with unit scaling; tf.nn.softmax)"""
    r = np.asarray(rois, np.float64).reshape(-1, 4)
    x = np.asarray(cls_reg, np.float64)
    lg, p = x[:, :num_classes], x[:, num_classes:num_classes + 4]
    e = np.exp(lg - lg.max(1, keepdims=True))
    probs = e / e.sum(1, keepdims=True)
    h, w = r[:, 2] - r[:, 0], r[:, 3] - r[:, 1]
    cy, cx = p[:, 0] * h + r[:, 0] + h / 2, p[:, 1] * w + r[:, 1] + w / 2
    ph, pw = np.exp(p[:, 2]) * h, np.exp(p[:, 3]) * w
    return np.stack([cy - ph / 2, cx - pw / 2, cy + ph / 2, cx + pw / 2], -1), probs


def class_major(probs, R):
    """[N * R, nc] -> [N, nc, R]: the layout of head_decode_probs' probabilities"""
    n, nc = probs.shape
    return np.ascontiguousarray(probs.reshape(n // R, R, nc).transpose(0, 2, 1))


def f32_restatement_probs(logits):
    """the kernels' float32 softmax, operation by operation (class_probs_begin: maximum, exp(x - m), the sum in class order,
    the quotient), with NumPy's float32 exp in place of the device's"""
    lg = np.asarray(logits, f32)
    e = np.exp(lg - lg.max(-1, keepdims=True)).astype(f32)
    s = np.zeros(lg.shape[:-1], f32)
    for k in range(lg.shape[-1]):
        s = (s + e[..., k]).astype(f32)
    return (e / s[..., None]).astype(f32)
