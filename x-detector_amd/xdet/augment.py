"""Training ingest: what the reference's input pipeline does to a decoded image and its ground truth before the network.

  light_head_preprocess_for_train      preprocessing/common_preprocessing.py:328-381 (run on 48 CPU threads,
                                       light_head_rfcn_train.py:42)
  distort_color (fast_mode=False)      preprocessing/common_preprocessing.py:212-262, chosen by
                                       apply_with_random_selector (:193-209, :358-360)
  ssd_random_sample_patch_wrapper      preprocessing/tf_image.py:602-630
  ssd_random_expand                    preprocessing/tf_image.py:547-571
  ssd_random_sample_patch              preprocessing/tf_image.py:393-545
  random_flip_left_right               preprocessing/tf_image.py:322-346
  resize_image (BILINEAR)              preprocessing/tf_image.py:307-319

Two statements of one contract (include/xdet.h):
  preprocess_train         the GPU path (csrc/augment.hip: xdet_preprocess_train_batch)
  host_preprocess_train    NumPy, f32, every product and sum rounded separately -- what the kernels are compared with
TensorFlow is not installed where this project is built, so the contract is pinned by reading the reference, as with
targets.host_* and losses.host_*.

Randomness.  TF's generators cannot be reproduced; as targets.py replaces tf.random_shuffle by a defined order, the draws
of one image are a defined sequence (all arithmetic 32-bit unsigned, mix = targets._mix):
  word            = mix(mix(seed ^ 0x9E3779B9) + image_id)                (the per-image word of targets.shuffle_keys)
  draw(seed, image_id, k) = mix(word ^ (0x80000000 | k)),  0 <= k < 2^31
targets.shuffle_keys feeds mix with word ^ (2 * element + stream), element < 2^30: bit 31 is the stream constant no shuffle
uses, and mix is a bijection, so a draw never equals a sampling key of the same (seed, image).  k counts the draws of one
image in the reference's program order (below); every value is drawn from one u = draw(...):
  uniform float in [lo, hi)   lo + ((u >> 8) * 2^-24) * (hi - lo)            (f32; lo, hi are f32 constants)
  uniform int in [lo, hi)     lo + u % (hi - lo); lo when hi - lo <= 0 (the draw is still consumed).  TF raises
                              InvalidArgumentError for an empty range (ssd_random_expand on an image side below 10).
  multinomial over 7          u % 7
Draw order: sel; the four colour factors in the order the chosen ordering reaches their ops; per attempt of the wrapper:
coin, [ratio, x, y of the expand], the min_iou index, then per round of check_roi_center: (width factor, height factor)
per round of sample_width_height, x, y; after the last attempt: the flip coin.

The steps, on v = u8 * (1/255) (convert_image_dtype):
 1. Colour.  sel = u % 4 picks the order of (B)rightness, (S)aturation, (H)ue, (C)ontrast:
        0: B S H C     1: S B C H     2: C H B S     3: H S C B
    B: v + delta, delta in [-32/255, 32/255).  S: RGB->HSV, s = clip(s * f, 0, 1), HSV->RGB, f in [0.5, 1.5).
    H: RGB->HSV, h = h + delta, h = h - floor(h), HSV->RGB, delta in [-0.2, 0.2).  C: (v - mean_c) * f + mean_c per channel,
    f in [0.5, 1.5).  One clip to [0, 1] at the end.  max(a, b) below means (a < b ? b : a) and min(a, b) (b < a ? b : a).
      RGB->HSV: V = max(max(r, g), b); rng = V - min(min(r, g), b); s = V > 0 ? rng / V : 0; norm = 1 / (6 * rng);
                h = r == V ? norm * (g - b) : g == V ? norm * (b - r) + 2/6 : norm * (r - g) + 4/6;
                h = rng > 0 ? h : 0; h = h < 0 ? h + 1 : h
      HSV->RGB: dh = h * 6; dr = clip(|dh - 3| - 1); dg = clip(2 - |dh - 2|); db = clip(2 - |dh - 4|);
                (r, g, b) = ((1 - s) + s * (dr, dg, db)) * V
    Only + - * /, min, max, floor: f32 NumPy and a kernel compiled with -ffp-contract=off agree bit for bit.
    The contrast mean is the one place where the arithmetic is DEFINED rather than restated.  It is taken over the whole
    source image, after the ops that precede contrast in the ordering:
        mean_c = f32( sum over pixels of int64(rint(v * 65536)) / (H * W * 65536) )
    -- an exact integer sum (rint: ties to even), one f64 division.  It differs from an f32 mean by less than 2^-17,
    below the summation-order noise of any float mean, and does not depend on reduction order, grid size or batch.
 2. Expand and sample (quirks kept): at most 3 attempts, each from the ORIGINAL image and boxes: coin < 0.5 keeps it, else
    the image is placed at a uniform-int offset (x first, then y) on a canvas int32(size * ratio), ratio in [1.1, 4), filled
    with [R,G,B mean]/255, boxes (b * [H,W,H,W] + [y,x,y,x]) / canvas.  min_iou = [-0.1, .1, .3, .5, .7, .9, 1.][u % 7];
    1. returns the attempt unchanged.  check_roi_overlap: rounds while round < 1, or round < 50 and (a kept box has
    jaccard < min_iou, or no box is kept).  (The reference does not bound its `no box is kept` term; an image without
    boxes would never leave.  Here the 50 bounds it too, and the reference's own else-branch -- the whole image with all
    boxes -- is what follows.)  check_roi_center: rounds while round < 1, or round < 20 and no centre is strictly inside
    the roi.  sample_width_height: rounds while round < 1, or round < 10 and one side exceeds twice the other, each round
    [0.3, 0.999) * size for width then height; int32 truncation; x in [0, width - w), y in [0, height - h).
    roi = (y / H, x / W, (y + h) / H, (x + w) / W) in f32; the patch in pixels is int32 of (roi0 * H, roi1 * W,
    (roi2 - roi0) * H, (roi3 - roi1) * W) in f32 -- (y / H) * H can land one below y, kept.  Height or width below 1:
    the attempt's image and boxes, unchanged.  Else boxes b * size - offset, clipped to [0, patch], / patch.
    The wrapper loops while no box passes check_bboxes (area in (0.001, 0.9), both sides > 0.025); afterwards failing
    boxes are dropped; if the loop used all three attempts the ORIGINAL image, labels and boxes are returned -- even
    when the third attempt succeeded (the reference tests index < max_attempt).
 3. Flip when the coin < 0.5: boxes [ymin, 1 - xmax, ymax, 1 - xmin].
 4. TF-legacy bilinear (align_corners=False, as preprocess_eval_kernel documents it) to S x S, * 2, - [R,G,B mean]/127.5,
    HWC -> CHW.
"""
import numpy as np

from .targets import _mix, MAX_GT

f32 = np.float32
AUG_STREAM = 0x80000000
RATIO_LIST = tuple(f32(v) for v in (-0.1, 0.1, 0.3, 0.5, 0.7, 0.9, 1.))
MEANS = (123.68, 116.78, 103.94)
FILL = tuple(f32(m / 255.) for m in MEANS)                      # the canvas colour [R,G,B mean]/255
WHITEN = tuple(f32(m) / f32(127.5) for m in MEANS)              # as preprocess_eval_kernel forms it
ORDERINGS = ('BSHC', 'SBCH', 'CHBS', 'HSCB')
MAX_DELTA = f32(32. / 255.)

# one fixed-size record per image: 32 little-endian 4-byte words, the layout of AugRecord in csrc/augment.hip
RECORD_DTYPE = np.dtype([
    ('valid', '<i4'),            # 0 for an invalid descriptor (then every other word is 0)
    ('canvas', '<i4', 2),        # (h, w) of the canvas the final image was cut from (the image's own size: no expand)
    ('offset', '<i4', 2),        # (y, x) of the source image in the canvas
    ('crop', '<i4', 4),          # (y, x, h, w) of the final image in the canvas
    ('flip', '<i4'),
    ('sel', '<i4'),              # colour ordering
    ('color', '<f4', 4),         # brightness delta, saturation factor, hue delta, contrast factor
    ('mean', '<f4', 3),          # contrast means
    ('attempts', '<i4'),         # attempts the wrapper used (1..3)
    ('fallback', '<i4'),         # 1: all three used, originals returned
    ('n_draws', '<i4'),          # draws consumed
    ('expanded', '<i4'),         # the last attempt: expand taken
    ('min_iou', '<i4'),          # the last attempt: index into the ratio list
    ('tiny_patch', '<i4'),       # some attempt met a patch below one pixel
    ('min_iou_mask', '<i4'),     # bit m: some attempt drew ratio index m
    ('expand_mask', '<i4'),      # bit a: attempt a expanded
    ('n_in', '<i4'),             # ground-truth boxes read
    ('n_out', '<i4'),            # ground-truth boxes written
    ('reserved', '<i4', 4)])
assert RECORD_DTYPE.itemsize == 128


def draw(seed, image_id, k):
    """draw(seed, image_id, k) -> uint32 (module docstring); k may be an array"""
    m = np.uint64(0xFFFFFFFF)
    word = _mix((_mix(np.uint64(int(seed) & 0xFFFFFFFF) ^ np.uint64(0x9E3779B9)) + np.uint64(int(image_id) & 0xFFFFFFFF)) & m)
    kk = np.asarray(k, np.uint64)
    return _mix(word ^ (np.uint64(AUG_STREAM) | kk)).astype(np.uint32)


def uniform_float(u, lo, hi):
    """lo + ((u >> 8) * 2^-24) * (hi - lo) in f32"""
    lo, hi = f32(lo), f32(hi)
    t = f32(int(u) >> 8) * f32(2. ** -24)
    return f32(lo + f32(t * f32(hi - lo)))


def uniform_int(u, lo, hi):
    """lo + u % (hi - lo); lo for an empty range (TF raises there)"""
    r = int(hi) - int(lo)
    return int(lo) if r <= 0 else int(lo) + int(u) % r


class _Draws(object):
    """the draws of one image, in order"""

    def __init__(self, seed, image_id):
        self.seed, self.image_id, self.k = seed, image_id, 0
        self._base, self._block = 0, np.zeros(0, np.uint32)

    def next(self):
        i = self.k - self._base
        if i >= len(self._block):
            self._base = self.k
            self._block = draw(self.seed, self.image_id, np.arange(self.k, self.k + 4096))
            i = 0
        self.k += 1
        return int(self._block[i])

    def uf(self, lo, hi):
        return uniform_float(self.next(), lo, hi)

    def ui(self, lo, hi):
        return uniform_int(self.next(), lo, hi)


# ---- colour ----------------------------------------------------------------------------------------------------------

def _max(a, b):
    return np.where(a < b, b, a).astype(f32)


def _min(a, b):
    return np.where(b < a, b, a).astype(f32)


def _clip01(x):
    return _min(_max(x, f32(0.)), f32(1.))


def rgb_to_hsv(r, g, b):
    V = _max(_max(r, g), b)
    rng = (V - _min(_min(r, g), b)).astype(f32)
    with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
        s = np.where(V > 0, rng / V, f32(0.)).astype(f32)
        norm = (f32(1.) / (f32(6.) * rng)).astype(f32)
        h = np.where(r == V, norm * (g - b),
                     np.where(g == V, (norm * (b - r)).astype(f32) + f32(2. / 6.), (norm * (r - g)).astype(f32) + f32(4. / 6.)))
    h = np.where(rng > 0, h, f32(0.)).astype(f32)
    h = np.where(h < 0, h + f32(1.), h).astype(f32)
    return h, s, V


def hsv_to_rgb(h, s, V):
    dh = (h * f32(6.)).astype(f32)
    dr = _clip01(np.abs(dh - f32(3.)) - f32(1.))
    dg = _clip01(f32(2.) - np.abs(dh - f32(2.)))
    db = _clip01(f32(2.) - np.abs(dh - f32(4.)))
    oms = (f32(1.) - s).astype(f32)
    return tuple((((oms + (s * d).astype(f32)).astype(f32)) * V).astype(f32) for d in (dr, dg, db))


def _op(op, rgb, color, mean):
    r, g, b = rgb
    if op == 'B':
        return tuple((c + color[0]).astype(f32) for c in rgb)
    if op == 'S':
        h, s, V = rgb_to_hsv(r, g, b)
        return hsv_to_rgb(h, _clip01((s * color[1]).astype(f32)), V)
    if op == 'H':
        h, s, V = rgb_to_hsv(r, g, b)
        h = (h + color[2]).astype(f32)
        return hsv_to_rgb((h - np.floor(h)).astype(f32), s, V)
    return tuple((((c - mean[i]).astype(f32) * color[3]).astype(f32) + mean[i]).astype(f32) for i, c in enumerate(rgb))


def fixed_point_mean(rgb):
    """the contrast mean of the module docstring: exact integer sum of rint(v * 65536), one f64 division -> f32 [3]"""
    out = []
    for c in rgb:
        q = np.rint((np.asarray(c, f32) * f32(65536.)).astype(f32)).astype(np.int64)
        out.append(f32(np.float64(int(q.sum())) / np.float64(q.size * 65536)))
    return np.array(out, f32)


def distort_color(image_u8, sel, color):
    """steps 1: uint8 [H,W,3] -> (f32 [H,W,3] in [0,1], contrast means f32 [3]); color = (brightness delta, saturation
    factor, hue delta, contrast factor)"""
    v = (np.asarray(image_u8, np.uint8).astype(f32) * f32(1. / 255.)).astype(f32)
    rgb = (v[..., 0], v[..., 1], v[..., 2])
    color = [f32(c) for c in color]
    mean = None
    for op in ORDERINGS[sel]:
        if op == 'C':
            mean = fixed_point_mean(rgb)
        rgb = _op(op, rgb, color, mean)
    return np.stack([_clip01(c) for c in rgb], -1), mean


# ---- geometry --------------------------------------------------------------------------------------------------------

def check_bboxes(b):
    hh, ww = (b[:, 2] - b[:, 0]).astype(f32), (b[:, 3] - b[:, 1]).astype(f32)
    area = (ww * hh).astype(f32)
    return (area < f32(0.9)) & (area > f32(0.001)) & (ww > f32(0.025)) & (hh > f32(0.025))


def jaccard(roi, b):
    iy0, ix0 = _max(roi[0], b[:, 0]), _max(roi[1], b[:, 1])
    iy1, ix1 = _min(roi[2], b[:, 2]), _min(roi[3], b[:, 3])
    h, w = _max((iy1 - iy0).astype(f32), f32(0.)), _max((ix1 - ix0).astype(f32), f32(0.))
    inter = (h * w).astype(f32)
    roi_area = f32(f32(roi[3] - roi[1]) * f32(roi[2] - roi[0]))
    union = (roi_area + (((b[:, 2] - b[:, 0]).astype(f32) * (b[:, 3] - b[:, 1]).astype(f32)).astype(f32) - inter).astype(f32)).astype(f32)
    with np.errstate(divide='ignore', invalid='ignore'):
        return (inter / union).astype(f32)


def expand_boxes(b, H, W, oy, ox, ch, cw):
    s = np.array([H, W, H, W], f32)
    o = np.array([oy, ox, oy, ox], f32)
    c = np.array([ch, cw, ch, cw], f32)
    return (((b * s).astype(f32) + o).astype(f32) / c).astype(f32)


def sample_patch(A, ch, cw, min_iou, D):
    """sample_patch of ssd_random_sample_patch on the attempt's boxes A [n,4] and its (ch, cw) canvas
    -> (crop (y, x, h, w) or None for the below-one-pixel path, subset mask of the boxes, their new boxes)"""
    n = A.shape[0]
    fh, fw = f32(ch), f32(cw)
    cy, cx = ((A[:, 0] + A[:, 2]).astype(f32) / f32(2.)).astype(f32), ((A[:, 1] + A[:, 3]).astype(f32) / f32(2.)).astype(f32)
    roi = (f32(0.), f32(0.), f32(1.), f32(1.))
    kept = np.ones(n, bool)
    idx = 0
    while idx < 1 or (idx < 50 and (bool((jaccard(roi, A[kept]) < min_iou).any()) or kept.sum() < 1)):
        j = 0
        mask = np.zeros(n, bool)
        while j < 1 or (j < 20 and mask.sum() < 1):
            t = 0
            sw, sh = fw, fh
            while t < 1 or (t < 10 and (sw > f32(sh * f32(2.)) or sh > f32(sw * f32(2.)))):
                sw = f32(D.uf(0.3, 0.999) * fw)
                sh = f32(D.uf(0.3, 0.999) * fh)
                t += 1
            swi, shi = int(sw), int(sh)
            x = D.ui(0, cw - swi)
            y = D.ui(0, ch - shi)
            roi = (f32(f32(y) / fh), f32(f32(x) / fw), f32(f32(y + shi) / fh), f32(f32(x + swi) / fw))
            mask = (cy > roi[0]) & (cx > roi[1]) & (cy < roi[2]) & (cx < roi[3])
            j += 1
        kept = mask
        idx += 1
    if kept.sum() > 0:
        sl = (int(f32(roi[0] * fh)), int(f32(roi[1] * fw)), int(f32(f32(roi[2] - roi[0]) * fh)), int(f32(f32(roi[3] - roi[1]) * fw)))
        sub = kept
    else:
        sl = (0, 0, ch, cw)
        sub = np.ones(n, bool)
    if sl[2] < 1 or sl[3] < 1:
        return None, np.ones(n, bool), A
    b = ((A[sub] * np.array([fh, fw, fh, fw], f32)).astype(f32) - np.array([sl[0], sl[1], sl[0], sl[1]], f32)).astype(f32)
    out = np.stack([_max(f32(0.), b[:, 0]), _max(f32(0.), b[:, 1]), _min(f32(sl[2]), b[:, 2]), _min(f32(sl[3]), b[:, 3])], -1)
    out = out.reshape(-1, 4).astype(f32)
    return sl, sub, (out / np.array([sl[2], sl[3], sl[2], sl[3]], f32)).astype(f32)


def host_geometry(H, W, labels, bboxes, seed, image_id, draws=None):
    """the draws of one image: colour parameters, step 2 and the flip coin -> (labels, bboxes, record) (record['mean'] is
    left 0: it needs the pixels).  draws: another source of next() / uf(lo, hi) / ui(lo, hi) with a counter k (tests)"""
    labels = np.asarray(labels, np.int32).reshape(-1)
    orig = np.asarray(bboxes, f32).reshape(-1, 4)
    rec = np.zeros((), RECORD_DTYPE)
    D = draws if draws is not None else _Draws(seed, image_id)
    rec['valid'] = 1
    rec['n_in'] = len(labels)
    sel = D.next() % 4
    rec['sel'] = sel
    color = [f32(0.)] * 4
    for op in ORDERINGS[sel]:
        if op == 'B':
            color[0] = D.uf(-MAX_DELTA, MAX_DELTA)
        elif op == 'S':
            color[1] = D.uf(0.5, 1.5)
        elif op == 'H':
            color[2] = D.uf(-0.2, 0.2)
        else:
            color[3] = D.uf(0.5, 1.5)
    rec['color'] = color
    index = 0
    n_valid = 0
    while index < 1 or (index < 3 and n_valid < 1):
        if D.uf(0., 1.) < f32(0.5):
            ch, cw, oy, ox, expanded = H, W, 0, 0, 0
            A = orig.copy()
        else:
            ratio = D.uf(1.1, 4.)
            cw, ch = int(f32(f32(W) * ratio)), int(f32(f32(H) * ratio))
            ox = D.ui(0, cw - W)
            oy = D.ui(0, ch - H)
            expanded = 1
            A = expand_boxes(orig, H, W, oy, ox, ch, cw)
            rec['expand_mask'] |= 1 << index
        m = D.next() % 7
        rec['min_iou_mask'] |= 1 << m
        crop, R, RL = (0, 0, ch, cw), A, labels
        if m < 6:
            sl, sub, nb = sample_patch(A, ch, cw, RATIO_LIST[m], D)
            if sl is None:
                rec['tiny_patch'] = 1
            else:
                crop, R, RL = sl, nb, labels[sub]
        index += 1
        n_valid = int(check_bboxes(R).sum())
        rec['expanded'], rec['min_iou'] = expanded, m
    rec['attempts'] = index
    if index < 3:
        keep = check_bboxes(R)
        out_l, out_b = RL[keep], R[keep]
        rec['canvas'], rec['offset'], rec['crop'] = (ch, cw), (oy, ox), crop
    else:
        out_l, out_b = labels, orig
        rec['fallback'] = 1
        rec['canvas'], rec['offset'], rec['crop'] = (H, W), (0, 0), (0, 0, H, W)
    if D.uf(0., 1.) < f32(0.5):
        rec['flip'] = 1
        out_b = np.stack([out_b[:, 0], (f32(1.) - out_b[:, 3]).astype(f32), out_b[:, 2], (f32(1.) - out_b[:, 1]).astype(f32)], -1)
    rec['n_draws'] = D.k
    rec['n_out'] = len(out_l)
    return out_l.astype(np.int32), out_b.reshape(-1, 4).astype(f32), rec


def warp(distorted, rec, S):
    """step 4 on the distorted source image [H,W,3] and the record's geometry -> f32 [3,S,S]"""
    H, W = distorted.shape[:2]
    oy, ox = (int(v) for v in rec['offset'])
    cy, cx, chh, cww = (int(v) for v in rec['crop'])

    def axis(n_in):
        f = (np.arange(S).astype(f32) * f32(f32(n_in) / f32(S))).astype(f32)
        i0 = np.minimum(f.astype(np.int32), n_in - 1)
        return i0, np.minimum(i0 + 1, n_in - 1), (f - i0.astype(f32)).astype(f32)

    y0, y1, ly = axis(chh)
    x0, x1, lx = axis(cww)
    if rec['flip']:
        x0, x1 = cww - 1 - x0, cww - 1 - x1
    fill = np.array(FILL, f32)

    def tap(yy, xx):
        sy, sx = (yy + (cy - oy))[:, None], (xx + (cx - ox))[None, :]
        inside = (sy >= 0) & (sy < H) & (sx >= 0) & (sx < W)
        v = distorted[np.clip(sy, 0, H - 1), np.clip(sx, 0, W - 1)]
        return np.where(inside[..., None], v, fill).astype(f32)

    tl, tr, bl, br = tap(y0, x0), tap(y0, x1), tap(y1, x0), tap(y1, x1)
    lx3, ly3 = lx[None, :, None], ly[:, None, None]
    top = (tl + ((tr - tl).astype(f32) * lx3).astype(f32)).astype(f32)
    bot = (bl + ((br - bl).astype(f32) * lx3).astype(f32)).astype(f32)
    v = (top + ((bot - top).astype(f32) * ly3).astype(f32)).astype(f32)
    v = ((v * f32(2.)).astype(f32) - np.array(WHITEN, f32)).astype(f32)
    return np.ascontiguousarray(v.transpose(2, 0, 1))


def host_preprocess_train(image_u8, labels, bboxes, out_size, seed, image_id):
    """light_head_preprocess_for_train (preprocessing/common_preprocessing.py:328-381, data_format NCHW) for one decoded
    image, restated step by step in f32 with every product and sum rounded separately (module docstring: the steps, the
    draws, and the one defined piece of arithmetic, the contrast mean; tf_image.py:322-346, 393-571, 602-630 for the box
    side).  TensorFlow is not installed where this project is built: the contract is pinned by reading the reference, as
    with targets.host_encode_anchors and losses.host_*.
    image_u8 uint8 [H,W,3]; labels [g]; bboxes f32 [g,4] (ymin, xmin, ymax, xmax in [0,1])
    -> (image f32 [3,S,S], labels i32 [g'], bboxes f32 [g',4], record: RECORD_DTYPE scalar).
    An image with H or W = 0 is the invalid descriptor of the GPU path: NaN planes, no boxes, a zero record."""
    S = int(out_size)
    img = np.asarray(image_u8, np.uint8)
    H, W = int(img.shape[0]), int(img.shape[1])
    if H <= 0 or W <= 0:
        return np.full((3, S, S), np.nan, f32), np.zeros(0, np.int32), np.zeros((0, 4), f32), np.zeros((), RECORD_DTYPE)
    out_l, out_b, rec = host_geometry(H, W, labels, bboxes, seed, image_id)
    distorted, mean = distort_color(img.reshape(H, W, 3), int(rec['sel']), rec['color'])
    rec['mean'] = mean
    return warp(distorted, rec, S), out_l, out_b, rec


# ---- the GPU path (csrc/augment.hip) ---------------------------------------------------------------------------------

def preprocess_train(images, labels, bboxes, out_size, seed, image_ids=None, stream=None, return_records=False):
    """host_preprocess_train for a batch on the GPU: lists of decoded uint8 [H,W,3] images of any sizes and their ground
    truth (per image labels [g], bboxes [g,4]) -> DeviceTensors (images_nchw f32 [N,3,S,S], glabels i32 [N,G],
    gbboxes f32 [N,G,4], n_gt i32 [N]) (+ records: RECORD_DTYPE [N] on the host, when asked for).  One packing
    (ops.pack_images), one upload, one C call (xdet_preprocess_train_batch); the outputs stay in device memory in the layout
    targets.encode_anchors and xdet_net_xception_body read.  G = the largest box count of the batch (at least 1)."""
    from ._lib import lib, check, InvalidArgumentError
    from .runtime import to_device, to_host, DeviceBuffer, DeviceTensor, synchronize
    from .targets import ground_truth
    from . import ops
    imgs = [np.ascontiguousarray(im, np.uint8) for im in images]
    N, S = len(imgs), int(out_size)
    if N == 0 or len(labels) != N or len(bboxes) != N:
        raise InvalidArgumentError(-1, 'preprocess_train: %d images, labels of %d, boxes of %d' % (N, len(labels), len(bboxes)))
    for i, im in enumerate(imgs):
        if im.ndim != 3 or im.shape[2] != 3:
            raise InvalidArgumentError(-1, 'images[%d]: uint8 [H,W,3] expected, got %r' % (i, im.shape))
    gl, gb, ng = ground_truth([np.asarray(l, np.int32).reshape(-1) for l in labels],
                              [np.asarray(b, f32).reshape(-1, 4) for b in bboxes])
    G = gl.shape[1]
    if G == 0:
        gl, gb, G = np.zeros((N, 1), np.int32), np.zeros((N, 1, 4), f32), 1
    packed, offsets, shapes = ops.pack_images(imgs)
    ids = None if image_ids is None else np.ascontiguousarray(image_ids, np.int32).reshape(N)
    if S <= 0 or G > MAX_GT:
        check(lib().xdet_preprocess_train_batch(None, 0, None, None, None, None, None, None, N, G, S, 0, None, None, None, None,
                                                None, None, None))
    # one upload: every input in one host block, 16-byte aligned parts
    parts = [packed, offsets, shapes, gl, gb, ng] + ([ids] if ids is not None else [])
    offs, total = [], 0
    for p in parts:
        offs.append(total)
        total += (p.nbytes + 15) // 16 * 16
    block = np.zeros(max(total, 16), np.uint8)
    for p, o in zip(parts, offs):
        block[o:o + p.nbytes] = np.ascontiguousarray(p).view(np.uint8).reshape(-1)
    d_in = to_device(block)
    ptr = [d_in.ptr + o for o in offs]
    ws = DeviceBuffer(lib().xdet_preprocess_train_workspace_bytes(N, G))
    o_img = DeviceBuffer(N * 3 * S * S * 4 + 512)
    o_l, o_b, o_n = DeviceBuffer(N * G * 4), DeviceBuffer(N * G * 16), DeviceBuffer(max(N * 4, 16))
    o_r = DeviceBuffer(N * RECORD_DTYPE.itemsize) if return_records else None
    check(lib().xdet_preprocess_train_batch(ptr[0], packed.nbytes, ptr[1], ptr[2], ptr[3], ptr[4], ptr[5],
                                            ptr[6] if ids is not None else None, N, G, S, int(seed) & 0xFFFFFFFF, o_img.ptr,
                                            o_l.ptr, o_b.ptr, o_n.ptr, o_r.ptr if o_r else None, ws.ptr,
                                            stream.handle if stream is not None else None))
    synchronize(stream)            # the inputs and the workspace are released on return
    out = (DeviceTensor(o_img.ptr, (N, 3, S, S), S, o_img), DeviceTensor(o_l.ptr, (N, 1, 1, G), G, o_l),
           DeviceTensor(o_b.ptr, (N, G, 1, 4), 4, o_b), DeviceTensor(o_n.ptr, (1, 1, 1, N), N, o_n))
    if return_records:
        out += (to_host(o_r.ptr, (N,), RECORD_DTYPE),)
    return out


def read_ground_truth(glabels, gbboxes, n_gt):
    """the device ground truth of preprocess_train -> NumPy (glabels i32 [N,G], gbboxes f32 [N,G,4], n_gt i32 [N])"""
    from .runtime import to_host
    N, G = glabels.shape[0], glabels.shape[3]
    return (to_host(glabels.ptr, (N, G), np.int32), to_host(gbboxes.ptr, (N, G, 4), f32), to_host(n_gt.ptr, (N,), np.int32))
