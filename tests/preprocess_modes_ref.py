"""TEST INFRASTRUCTURE, NOT PRODUCT CODE: a NumPy restatement of the reference's light_head_preprocess_for_eval with
its `resize` argument (preprocessing/common_preprocessing.py:29-32,383-440) and of the box side of
tf_image.resize_image_bboxes_with_crop_or_pad (tf_image.py:179-305).

TensorFlow is not installed here, so PAD_AND_RESIZE and CENTRAL_CROP cannot be pinned to the reference's own output.
They are restated from the reference's code: whitening first (:392-393), then
  NONE            nothing (:400-402)
  CENTRAL_CROP    resize_image_bboxes_with_crop_or_pad to S x S (:403-406)
  PAD_AND_RESIZE  factor = min(1, min(S/H, S/W)) in f64, resize_shape = int32(floor(factor * (H, W))) (:407-414),
                  resize_image to that shape (TF-legacy bilinear), then crop_or_pad to S x S (:415-418)
  WARP_RESIZE     resize_image to S x S (:419-423).
The TF-legacy bilinear is the oracle's (oracle/lighthead_oracle.py preprocess_for_eval), to which WARP_RESIZE is tied
bit for bit by the tests; PAD_AND_RESIZE uses the same sampler with another output size.  Every box step is f32 in
TF's order: b * [h,w,h,w], + offset, / [th,tw,th,tw].

An invalid descriptor (what include/xdet.h lists) gives NaN planes and a NaN bbox_img, as the product does.
"""
import numpy as np

f32 = np.float32
NONE, CENTRAL_CROP, PAD_AND_RESIZE, WARP_RESIZE = 1, 2, 3, 4
MEANS = np.array([123.68 / 127.5, 116.78 / 127.5, 103.94 / 127.5]).astype(f32)


def whiten(img):
    """convert_image_dtype(float32) * 2 - mean/127.5 (common_preprocessing.py:392-393), HWC f32"""
    return ((np.asarray(img, np.uint8).astype(f32) * f32(1.0 / 255.0)) * f32(2.0) - MEANS).astype(f32)


def bilinear(x, oh, ow):
    """tf.image.resize_images(BILINEAR, align_corners=False) of TF1 (legacy: src = dst * in/out) of HWC f32 x"""
    H, W = x.shape[:2]
    hs, ws = f32(f32(H) / f32(oh)), f32(f32(W) / f32(ow))
    fy = (np.arange(oh, dtype=f32) * hs).astype(f32)
    fx = (np.arange(ow, dtype=f32) * ws).astype(f32)
    y0, x0 = fy.astype(np.int64), fx.astype(np.int64)
    y1, x1 = np.minimum(y0 + 1, H - 1), np.minimum(x0 + 1, W - 1)
    ly = (fy - y0.astype(f32)).astype(f32)[:, None, None]
    lx = (fx - x0.astype(f32)).astype(f32)[None, :, None]
    tl, tr = x[y0][:, x0], x[y0][:, x1]
    bl, br = x[y1][:, x0], x[y1][:, x1]
    top = (tl + ((tr - tl) * lx).astype(f32)).astype(f32)
    bot = (bl + ((br - bl) * lx).astype(f32)).astype(f32)
    return (top + ((bot - top) * ly).astype(f32)).astype(f32)


def pad_resize_shape(H, W, S):
    """common_preprocessing.py:407-414: f64 factor, floor, int32"""
    factor = min(np.float64(1.0), min(np.float64(S) / np.float64(H), np.float64(S) / np.float64(W)))
    return int(np.floor(factor * np.float64(H))), int(np.floor(factor * np.float64(W)))


def crop_or_pad_offsets(h, w, S):
    """tf_image.py:261-274 -> (crop_y, crop_x, pad_y, pad_x, kept_h, kept_w); Python floor division"""
    return max((h - S) // 2, 0), max((w - S) // 2, 0), max((S - h) // 2, 0), max((S - w) // 2, 0), min(S, h), min(S, w)


def bboxes_crop_or_pad(bboxes, height, width, offset_y, offset_x, target_height, target_width):
    """tf_image.py:179-203, f32 in TF's order"""
    b = np.asarray(bboxes, f32).reshape(-1, 4)
    b = (b * np.array([height, width, height, width], f32)).astype(f32)
    b = (b + np.array([offset_y, offset_x, offset_y, offset_x], f32)).astype(f32)
    return (b / np.array([target_height, target_width, target_height, target_width], f32)).astype(f32)


def map_boxes(bboxes, H, W, S, mode):
    """the boxes side of the resize step (bbox_img is row 0 of what the reference maps, :395-399,424-426)"""
    b = np.asarray(bboxes, f32).reshape(-1, 4)
    if mode in (NONE, WARP_RESIZE):
        return b.copy()
    h, w = pad_resize_shape(H, W, S) if mode == PAD_AND_RESIZE else (H, W)
    cy, cx, py, px, kh, kw = crop_or_pad_offsets(h, w, S)
    b = bboxes_crop_or_pad(b, h, w, -cy, -cx, kh, kw)                  # tf_image.py:282-286
    return bboxes_crop_or_pad(b, kh, kw, py, px, S, S)                  # :290-294


def valid(H, W, S, mode, fits=True):
    if H <= 0 or W <= 0 or not fits:
        return False
    if mode == NONE:
        return H == S and W == S
    if mode == PAD_AND_RESIZE:
        rh, rw = pad_resize_shape(H, W, S)
        return rh > 0 and rw > 0
    return True


def preprocess(img, S, mode):
    """uint8 [H,W,3] -> (f32 [3,S,S], bbox_img f32 [4])"""
    img = np.asarray(img, np.uint8)
    H, W = img.shape[:2]
    if not valid(H, W, S, mode):
        return np.full((3, S, S), np.nan, f32), np.full(4, np.nan, f32)
    x = whiten(img)
    if mode == NONE:
        out = x
    elif mode == WARP_RESIZE:
        out = bilinear(x, S, S)
    else:
        h, w = (H, W)
        if mode == PAD_AND_RESIZE:
            h, w = pad_resize_shape(H, W, S)
            x = bilinear(x, h, w)
        cy, cx, py, px, kh, kw = crop_or_pad_offsets(h, w, S)
        out = np.zeros((S, S, 3), f32)
        out[py:py + kh, px:px + kw] = x[cy:cy + kh, cx:cx + kw]
    bbox_img = map_boxes([[0., 0., 1., 1.]], H, W, S, mode)[0]
    return np.ascontiguousarray(out.transpose(2, 0, 1)), bbox_img


def bboxes_resize(bbox_ref, bboxes):
    """tfe.bboxes_resize as bboxes_eval applies it (oracle/lighthead_oracle.py): back to the original image's frame"""
    r = np.asarray(bbox_ref, f32)
    b = np.asarray(bboxes, f32).reshape(-1, 4)
    b = (b - np.array([r[0], r[1], r[0], r[1]], f32)).astype(f32)
    s = np.array([r[2] - r[0], r[3] - r[1], r[2] - r[0], r[3] - r[1]], f32)
    return (b / s).astype(f32)
