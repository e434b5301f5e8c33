"""Training losses: everything of the reference's lighr_head_model_fn between the logits and the scalar loss, with the
gradients with respect to the logits.

  modified_smooth_l1                   light_head_rfcn_train.py:257-275
  select_samples, rpn losses           light_head_rfcn_train.py:312-380
  head_loss_func                       light_head_rfcn_train.py:384-413
  the OHEM top_k and reduce_mean       net/xception_body.py:502-533, 560

Two statements of one contract (include/xdet.h "training losses"):
  rpn_loss / head_loss             the GPU path (csrc/losses.hip: xdet_rpn_loss / xdet_head_loss)
  host_rpn_loss / host_head_loss   NumPy, f32 in the reference's order (dtype=np.float64: the accuracy yardstick) -- what
                                   the kernels are compared with
`HeadLoss` is the `loss_func` of model.get_head(..., is_training=True): it carries labels, targets and fg_ratio, as the
reference's lambda closes over them.

The contract in short.  RPN: S = N * anchors_per_image rows are drawn from the batch flattened by
targets.sample_rois(labels_flat, ones, S, fg_ratio, 0., seed, image=0); ce = mean over them of the 2-way cross entropy with
class [label > 0]; loc = (mean over the selected rows with label > 0 of the box's smooth L1) / fg_ratio (0 without such a
row); a row selected m times carries m times the gradient.  Head: per ROI ce + [label > 0] * smooth L1 / fg_ratio (0 for a
label outside [0, C)); OHEM keeps the K largest per image, descending, equal values in ascending index order; the loss is
the mean over the N * K kept rows.
"""
import collections

import numpy as np

from . import targets as T

f32 = np.float32
MAX_SELECTED = 32768      # N * anchors_per_image
MAX_ROIS = 8192           # P
MAX_CLASSES = 128         # C



class RpnLossResult(collections.namedtuple('RpnLossResult', 'losses sel_index counts grad_cls grad_loc')):
    """The five fields unpack as ever; `grad_device` (an attribute, not a field) is d loss / d rpn_out left on the GPU by
    rpn_loss(..., keep_device=True): a DeviceTensor [N,h,w,6A] with the rpn_out buffer's ld, else None.
    From rpn_loss(..., device_result=True): losses, sel_index and counts are the DeviceBuffers the kernel wrote (f32 [3],
    i32 [S], i32 [4]), grad_cls and grad_loc None, and nothing was synchronised."""
    grad_device = None


HeadLossResult = collections.namedtuple('HeadLossResult', 'losses per_roi select grad_cls grad_reg')


# ---- the NumPy statement ---------------------------------------------------------------------------------------------

def _sl1_consts(sigma, dtype):
    s2 = dtype(sigma) * dtype(sigma)
    return s2, dtype(1.) / s2, dtype(0.5) * s2, dtype(0.5) / s2


def modified_smooth_l1(pred, target, sigma=1., dtype=f32):
    """d = pred - target; |d| < 1 / sigma^2 -> (d * d) * (0.5 * sigma^2), else |d| - 0.5 / sigma^2 (elementwise)"""
    s2, thr, c1, c2 = _sl1_consts(sigma, dtype)
    d = np.asarray(pred, dtype) - np.asarray(target, dtype)
    a = np.abs(d)
    return np.where(a < thr, (d * d) * c1, a - c2).astype(dtype)


def smooth_l1_grad(pred, target, sigma=1., dtype=f32):
    s2, thr, _, _ = _sl1_consts(sigma, dtype)
    d = np.asarray(pred, dtype) - np.asarray(target, dtype)
    return np.where(np.abs(d) < thr, d * s2, np.where(d > 0, dtype(1.), dtype(-1.))).astype(dtype)


def _box_sum(v):
    return ((v[..., 0] + v[..., 1]) + v[..., 2]) + v[..., 3]


def cross_entropy(x, y, dtype=f32):
    """rows x [R,C], classes y [R] -> (ce [R], d ce / d x [R,C]): m = max, s = sum_j exp(x_j - m) in index order,
    ce = log(s) - (x_y - m)"""
    x = np.asarray(x, dtype)
    r = np.arange(x.shape[0])
    m = x.max(1)
    e = np.exp(x - m[:, None]).astype(dtype)
    s = np.zeros(x.shape[0], dtype)
    for j in range(x.shape[1]):
        s = s + e[:, j]
    ce = np.log(s).astype(dtype) - (x[r, y] - m)
    g = e / s[:, None]
    g[r, y] = g[r, y] - dtype(1.)
    return ce.astype(dtype), g.astype(dtype)


def host_rpn_loss(cls_score, bbox_pred, labels, targets, anchors_per_image, fg_ratio, seed=0, sigma=1., dtype=f32):
    """cls_score [N, ..., 2] and bbox_pred [N, ..., 4] per anchor (anchor order = the order of labels [N, n_a] and
    targets [N, n_a, 4]) -> RpnLossResult(losses [ce, loc, total], sel_index i32 [S], counts i32 [4]: |pos|, |neg|, n_keep,
    selected positives; grad_cls [N*n_a, 2], grad_loc [N*n_a, 4])"""
    lab = np.asarray(labels).reshape(-1)
    N = np.asarray(labels).shape[0]
    cls = np.asarray(cls_score, dtype).reshape(-1, 2)
    loc = np.asarray(bbox_pred, dtype).reshape(-1, 4)
    tg = np.asarray(targets, dtype).reshape(-1, 4)
    S = int(N) * int(anchors_per_image)
    idx, (n_pos, n_neg, n_keep) = T.sample_rois(lab, np.ones(lab.shape[0], f32), S, fg_ratio, 0., seed, image=0)
    g_cls, g_loc = np.zeros(cls.shape, dtype), np.zeros(loc.shape, dtype)
    if n_keep == 0:
        return RpnLossResult(np.zeros(3, dtype), idx.astype(np.int32), np.array([n_pos, n_neg, 0, 0], np.int32), g_cls, g_loc)
    y = (lab[idx] > 0).astype(np.int64)
    ce_rows, _ = cross_entropy(cls[idx], y, dtype)
    ce = ce_rows.mean(dtype=dtype)
    pos_rows = idx[y > 0]
    n_sel_pos = len(pos_rows)
    loc_loss = dtype(0.)
    if n_sel_pos:
        loc_loss = _box_sum(modified_smooth_l1(loc[pos_rows], tg[pos_rows], sigma, dtype)).mean(dtype=dtype) / dtype(fg_ratio)
    rows, mult = np.unique(idx, return_counts=True)
    fm = mult.astype(dtype)
    yr = (lab[rows] > 0).astype(np.int64)
    _, g = cross_entropy(cls[rows], yr, dtype)
    g_cls[rows] = g * (fm / dtype(S))[:, None]
    pr = yr > 0
    if n_sel_pos:
        wb = (fm[pr] / dtype(n_sel_pos)) / dtype(fg_ratio)
        g_loc[rows[pr]] = smooth_l1_grad(loc[rows[pr]], tg[rows[pr]], sigma, dtype) * wb[:, None]
    losses = np.array([ce, loc_loss, dtype(ce) + dtype(loc_loss)], dtype)
    return RpnLossResult(losses, idx.astype(np.int32), np.array([n_pos, n_neg, n_keep, n_sel_pos], np.int32), g_cls, g_loc)


def host_head_loss(cls_score, bboxes_reg, labels, targets, fg_ratio, ohem_k=0, sigma=1., dtype=f32):
    """cls_score [N,P,C], bboxes_reg [N,P,4], labels [N,P], targets [N,P,4] -> HeadLossResult(losses [head_loss, ce mean,
    loc mean], per_roi [N,P], select i32 [N,K], grad_cls [N,P,C], grad_reg [N,P,4])"""
    cls = np.asarray(cls_score, dtype)
    reg = np.asarray(bboxes_reg, dtype)
    lab = np.asarray(labels).astype(np.int64)
    tg = np.asarray(targets, dtype)
    N, P, C = cls.shape
    valid = (lab >= 0) & (lab < C)
    y = np.where(valid, lab, 0)
    ce, g = cross_entropy(cls.reshape(-1, C), y.reshape(-1), dtype)
    ce = np.where(valid, ce.reshape(N, P), dtype(0.)).astype(dtype)
    pos = valid & (lab > 0)
    loc = np.where(pos, _box_sum(modified_smooth_l1(reg, tg, sigma, dtype)) / dtype(fg_ratio), dtype(0.)).astype(dtype)
    per_roi = (ce + loc).astype(dtype)
    if ohem_k > 0:
        K = min(int(ohem_k), P)
        select = np.stack([np.lexsort((np.arange(P), -per_roi[n]))[:K] for n in range(N)])       # stable descending
    else:
        K = P
        select = np.tile(np.arange(P), (N, 1))
    rows = np.arange(N)[:, None]
    cnt = dtype(N * K)
    losses = np.array([per_roi[rows, select].sum(dtype=dtype) / cnt, ce[rows, select].sum(dtype=dtype) / cnt,
                       loc[rows, select].sum(dtype=dtype) / cnt], dtype)
    on = np.zeros((N, P), bool)
    on[rows, select] = True
    w = dtype(1.) / cnt
    g_cls = np.where((on & valid)[..., None], g.reshape(N, P, C) * w, dtype(0.)).astype(dtype)
    g_reg = np.where((on & pos)[..., None], (smooth_l1_grad(reg, tg, sigma, dtype) / dtype(fg_ratio)) * w, dtype(0.)).astype(dtype)
    return HeadLossResult(losses, per_roi, select.astype(np.int32), g_cls, g_reg)


# ---- the GPU path (csrc/losses.hip) ----------------------------------------------------------------------------------

def _h(stream):
    return stream.handle if stream is not None else None


def _device(x, dtype):
    """NumPy -> a fresh device copy; anything with a device pointer (.ptr) is used as it is"""
    from .runtime import to_device
    return x if hasattr(x, 'ptr') else to_device(np.ascontiguousarray(x, dtype))


def _round_up(x, m):
    return (x + m - 1) // m * m


def _check_buffers(who, buffers):
    if buffers is not None and not isinstance(buffers, dict):
        from ._lib import InvalidArgumentError
        raise InvalidArgumentError(-1, '%s: buffers must be a dict the caller keeps (filled on the first call), got %s'
                                       % (who, type(buffers).__name__))


def rpn_loss(cls_score, bbox_pred, labels, targets, anchors_per_image, fg_ratio, seed=0, sigma=1., with_grad=True, stream=None,
             keep_device=False, device_result=False, buffers=None):
    """host_rpn_loss on the GPU (xdet_rpn_loss), the same results.  cls_score / bbox_pred: NumPy [N,Hh,Ww,2A] / [N,Hh,Ww,4A]
    (or [N,n,2A] / [N,n,4A]), or the two DeviceTensor views model.get_rpn returns -- then the detector's rpn_out buffer is
    read in place, nothing is copied.  labels [N,n_a] / targets [N,n_a,4]: NumPy or device buffers (DeviceBuffer /
    DeviceTensor, as xdet_encode_anchors wrote them).  The gradients come back in the layout of the inputs:
    grad_cls [N,...,2A], grad_loc [N,...,4A] (None without with_grad).
    keep_device=True (the two views of get_rpn, cls_score [N,h,w,2A] followed by bbox_pred, and with_grad): the result's
    `grad_device` also carries the gradient as the GPU wrote it, a DeviceTensor [N,h,w,6A] with rpn_out's ld -- what
    model.rpn_backward reads.
    device_result=True (default off; goes with keep_device=True and device labels and targets): losses, selection, counts and
    gradient stay on the device -- the result's losses, sel_index and counts are DeviceBuffers -- and the call neither
    downloads nor synchronises.  buffers (a dict the caller keeps, default None): workspace, results and gradient live in
    it from the first call on, so a driver allocates them once; a later call overwrites what the earlier one returned."""
    from ._lib import lib, check, InvalidArgumentError
    from .runtime import to_device, to_host, DeviceBuffer, DeviceTensor, synchronize
    if isinstance(cls_score, DeviceTensor) != isinstance(bbox_pred, DeviceTensor):
        raise InvalidArgumentError(-1, 'rpn_loss: cls_score and bbox_pred must both be NumPy arrays or both views of one device buffer')
    on_device = isinstance(cls_score, DeviceTensor)
    if on_device:
        shp, A = tuple(cls_score.shape), cls_score.shape[-1] // 2
        base = min(cls_score.ptr, bbox_pred.ptr)
        ld, cls_off, box_off = cls_score.ld, (cls_score.ptr - base) // 4, (bbox_pred.ptr - base) // 4
        if (bbox_pred.ld != ld or tuple(bbox_pred.shape[:-1]) != shp[:-1] or bbox_pred.shape[-1] != 4 * A or shp[-1] != 2 * A
                or max(cls_off, box_off) >= ld):
            raise InvalidArgumentError(-1, 'rpn_loss: cls_score [..,2A] and bbox_pred [..,4A] must be channel ranges of one buffer')
    else:
        c, b = np.ascontiguousarray(cls_score, f32), np.ascontiguousarray(bbox_pred, f32)
        shp, A = c.shape, c.shape[-1] // 2
        if c.ndim < 3 or c.shape[-1] != 2 * A or b.shape != c.shape[:-1] + (4 * A,):
            raise InvalidArgumentError(-1, 'rpn_loss: cls_score [N,..,2A] and bbox_pred [N,..,4A] expected, got %r and %r' % (c.shape, b.shape))
        cls_off, box_off = 0, _round_up(2 * A, 4)
        ld = box_off + 4 * A
    if keep_device and not (on_device and with_grad and len(shp) == 4 and cls_off == 0 and box_off == 2 * A):
        raise InvalidArgumentError(-1, 'rpn_loss: keep_device=True needs with_grad and the two DeviceTensor views model.get_rpn '
                                       'returns ([N,h,w,2A] and, right behind it, [N,h,w,4A])')
    if device_result and not (keep_device and hasattr(labels, 'ptr') and hasattr(targets, 'ptr')):
        raise InvalidArgumentError(-1, 'rpn_loss: device_result=True needs keep_device=True and labels and targets in device memory')
    _check_buffers('rpn_loss', buffers)
    N, hw = int(shp[0]), int(np.prod(shp[1:-1]))
    S = N * int(anchors_per_image)
    fgr, sg = float(fg_ratio), float(sigma)
    n_lab = None if hasattr(labels, 'ptr') else int(np.asarray(labels).size)
    if (min(N, hw, A) <= 0 or N * hw * A > (1 << 27) or not 0 < S <= MAX_SELECTED or not 0. < fgr <= 1. or not 0. < sg < np.inf
            or ld % 4 or cls_off % 2 or box_off % 4):
        raise InvalidArgumentError(-1, 'rpn_loss: N = %d, %d anchors per image (N * n_a <= 2^27), anchors_per_image = %r (0 < N * it <= '
                                       '%d), fg_ratio = %r (in (0, 1]), sigma = %r (positive, finite), ld = %d / cls_off = %d / box_off '
                                       '= %d (multiples of 4 / 2 / 4)' % (N, hw * A, anchors_per_image, MAX_SELECTED, fg_ratio, sigma,
                                                                          ld, cls_off, box_off))
    if n_lab is not None and n_lab != N * hw * A:
        raise InvalidArgumentError(-1, 'rpn_loss: %d labels for %d anchors' % (n_lab, N * hw * A))
    if on_device:
        d_in, in_ptr = None, base
    else:
        packed = np.zeros((N, hw, ld), f32)
        packed[..., :2 * A], packed[..., box_off:] = c.reshape(N, hw, 2 * A), b.reshape(N, hw, 4 * A)
        d_in = to_device(packed)
        in_ptr = d_in.ptr
    d_lab, d_tg = _device(labels, np.int32), _device(targets, f32)
    _b = T._buffer
    ws = _b(buffers, 'ws', lib().xdet_losses_workspace_bytes(N, int(anchors_per_image)))
    d_sel, d_cnt, d_loss = _b(buffers, 'select', S * 4), _b(buffers, 'counts', 16), _b(buffers, 'losses', 16)
    d_grad = _b(buffers, 'grad', N * hw * ld * 4) if with_grad else None
    check(lib().xdet_rpn_loss(in_ptr, ld, cls_off, box_off, N, hw, 1, A, d_lab.ptr, d_tg.ptr, int(anchors_per_image), fgr,
                              int(seed) & 0xFFFFFFFF, sg, ws.ptr, d_sel.ptr, d_cnt.ptr, d_loss.ptr, d_grad.ptr if d_grad else None,
                              _h(stream)))
    if device_result:
        res = RpnLossResult(d_loss, d_sel, d_cnt, None, None)
        res.grad_device = DeviceTensor(d_grad.ptr, tuple(shp[:3]) + (6 * A,), ld, owner=d_grad)
        res._inputs = (d_lab, d_tg, ws)                  # (alive with the result: the launch may still be in flight)
        from .train import forward_step
        res.forward_step = forward_step(cls_score, '_rpn_step')
        return res
    synchronize(stream)
    g_cls = g_loc = None
    if with_grad:
        g = to_host(d_grad.ptr, (N, hw, ld), f32)
        g_cls = np.ascontiguousarray(g[..., cls_off:cls_off + 2 * A]).reshape(shp)
        g_loc = np.ascontiguousarray(g[..., box_off:box_off + 4 * A]).reshape(tuple(shp[:-1]) + (4 * A,))
    res = RpnLossResult(to_host(d_loss.ptr, (3,), f32), to_host(d_sel.ptr, (S,), np.int32), to_host(d_cnt.ptr, (4,), np.int32),
                        g_cls, g_loc)
    if keep_device:
        res.grad_device = DeviceTensor(d_grad.ptr, tuple(shp[:3]) + (6 * A,), ld, owner=d_grad)
        from .train import forward_step
        res.forward_step = forward_step(cls_score, '_rpn_step')      # (which weights the forward ran with: rpn_backward's guard)
    return res


def head_loss(cls_score, bboxes_reg, labels, targets, fg_ratio, ohem_k=0, sigma=1., num_classes=None, with_grad=True, stream=None,
              device_grad=None, device_result=False, buffers=None):
    """host_head_loss on the GPU (xdet_head_loss), the same results.  cls_score [N,P,C] / bboxes_reg [N,P,4] as NumPy arrays;
    or cls_score = the detector's `cls_reg` DeviceTensor ([N,P,1,C+4]: C class logits, then the 4 regression outputs) with
    bboxes_reg None -- read in place.  labels [N,P] / targets [N,P,4]: NumPy or device buffers (as xdet_encode_rois wrote
    them).
    device_result=True (default off; a device cls_reg tensor, device labels and targets, with_grad): losses, per_roi and
    select of the result are the DeviceBuffers the kernel wrote (f32 [3], f32 [N,P], i32 [N,K]), grad_cls and grad_reg None,
    the gradient is device_grad's one entry, and the call neither downloads nor synchronises.  buffers (a dict the caller
    keeps, default None): workspace, results and gradient live in it from the first call on."""
    from ._lib import lib, check, InvalidArgumentError
    from .runtime import to_device, to_host, DeviceBuffer, DeviceTensor, synchronize
    if isinstance(cls_score, DeviceTensor):
        if bboxes_reg is not None:
            raise InvalidArgumentError(-1, 'head_loss: a device cls_reg tensor holds the regression outputs too; pass bboxes_reg=None')
        shp = tuple(cls_score.shape)
        N, P = int(shp[0]), int(np.prod(shp[1:-1]))
        C = int(num_classes) if num_classes is not None else int(shp[-1]) - 4
        ld, d_in, in_ptr = cls_score.ld, None, cls_score.ptr
    else:
        c, r = np.ascontiguousarray(cls_score, f32), np.ascontiguousarray(bboxes_reg, f32)
        if c.ndim != 3 or r.shape != c.shape[:2] + (4,):
            raise InvalidArgumentError(-1, 'head_loss: cls_score [N,P,C] and bboxes_reg [N,P,4] expected, got %r and %r' % (c.shape, r.shape))
        N, P, C = c.shape
        ld = _round_up(C + 4, 4)
        d_in = None
    fgr, sg, k = float(fg_ratio), float(sigma), int(ohem_k)
    n_lab = None if hasattr(labels, 'ptr') else int(np.asarray(labels).size)
    if (min(N, P) <= 0 or not 2 <= C <= MAX_CLASSES or P > MAX_ROIS or N > 1024 or C + 4 > ld or k < 0 or not 0. < fgr <= 1.
            or not 0. < sg < np.inf):
        raise InvalidArgumentError(-1, 'head_loss: N = %d (1 .. 1024), P = %d (1 .. %d), C = %d (2 .. %d, C + 4 <= ld = %d), ohem_k = %d '
                                       '(>= 0), fg_ratio = %r (in (0, 1]), sigma = %r (positive, finite)'
                                   % (N, P, MAX_ROIS, C, MAX_CLASSES, ld, k, fg_ratio, sigma))
    if n_lab is not None and n_lab != N * P:
        raise InvalidArgumentError(-1, 'head_loss: %d labels for %d ROIs' % (n_lab, N * P))
    if device_result and not (isinstance(cls_score, DeviceTensor) and with_grad and hasattr(labels, 'ptr') and hasattr(targets, 'ptr')):
        raise InvalidArgumentError(-1, 'head_loss: device_result=True needs the cls_reg DeviceTensor, with_grad and labels and targets '
                                       'in device memory')
    _check_buffers('head_loss', buffers)
    if not isinstance(cls_score, DeviceTensor):
        packed = np.zeros((N, P, ld), f32)
        packed[..., :C], packed[..., C:C + 4] = c, r
        d_in = to_device(packed)
        in_ptr = d_in.ptr
    K = min(k, P) if k > 0 else P
    d_lab, d_tg = _device(labels, np.int32), _device(targets, f32)
    _b = T._buffer
    ws = _b(buffers, 'ws', lib().xdet_losses_workspace_bytes(N, 0))
    d_loss, d_per, d_sel = _b(buffers, 'losses', 16), _b(buffers, 'per_roi', N * P * 4), _b(buffers, 'select', N * K * 4)
    d_grad = _b(buffers, 'grad', N * P * ld * 4) if with_grad else None
    check(lib().xdet_head_loss(in_ptr, ld, 0, C, N, P, C, d_lab.ptr, d_tg.ptr, fgr, k, sg, ws.ptr, d_loss.ptr, d_per.ptr, d_sel.ptr,
                               d_grad.ptr if d_grad else None, _h(stream)))
    if device_result:
        g = DeviceTensor(d_grad.ptr, (N, P, 1, C + 4), ld, owner=d_grad)
        g._inputs = (d_lab, d_tg, ws)                    # (alive with the gradient: the launch may still be in flight)
        if device_grad is not None:
            device_grad.append(g)
        return HeadLossResult(d_loss, d_per, d_sel, None, None)
    synchronize(stream)
    g_cls = g_reg = None
    if with_grad:
        g = to_host(d_grad.ptr, (N, P, ld), f32)
        g_cls, g_reg = np.ascontiguousarray(g[..., :C]), np.ascontiguousarray(g[..., C:C + 4])
        if device_grad is not None:
            device_grad.append(DeviceTensor(d_grad.ptr, (N, P, 1, C + 4), ld, owner=d_grad))
    return HeadLossResult(to_host(d_loss.ptr, (3,), f32), to_host(d_per.ptr, (N, P), f32), to_host(d_sel.ptr, (N, K), np.int32),
                          g_cls, g_reg)


class HeadLoss(object):
    """The `loss_func` of model.get_head(..., is_training=True): the sampled ROIs' labels [N,P] and targets [N,P,4]
    (what the encode_fn of get_proposals returned: NumPy, or the device arrays of ext_encode_rois(..., keep_device=True), labels
    i32, read in place) and fg_ratio, as the reference's lambda closes over them
    (light_head_rfcn_train.py:407).  Calling it with the head's outputs gives the HeadLossResult; get_head leaves the last
    one in `.result` (losses, per_roi, select and the gradients) and returns the scalar; `.grad_device` is d loss / d cls_reg
    on the GPU, in the `cls_reg` buffer's layout (model.head_backward reads it).  device_result=True / buffers=: head_loss's
    mode that leaves losses, per-ROI values and selection on the device and synchronises nothing (the result's three fields are
    DeviceBuffers then), and the dict its buffers live in."""

    def __init__(self, labels, targets, fg_ratio, sigma=1., device_result=False, buffers=None):
        self.labels, self.targets, self.fg_ratio, self.sigma = labels, targets, fg_ratio, sigma
        self.device_result, self.buffers = device_result, buffers    # (head_loss's two arguments of these names; default off)
        self.result = None
        self.grad_device = None

    def __call__(self, cls_score, bboxes_reg=None, ohem_k=0, num_classes=None, stream=None):
        labels = self.labels if hasattr(self.labels, 'ptr') else np.asarray(self.labels).astype(np.int32)
        kept = []
        for t in (labels, self.targets):                 # what encode_rois(..., keep_device=True) left unsynchronised on
            made_on = getattr(t, 'made_on', stream)       # another stream is waited for; anything else is read as it is
            if made_on is not stream:
                from .runtime import synchronize
                synchronize(made_on)
        self.result = head_loss(cls_score, bboxes_reg, labels, self.targets, self.fg_ratio, ohem_k, self.sigma, num_classes,
                                stream=stream, device_grad=kept, device_result=self.device_result, buffers=self.buffers)
        self.grad_device = kept[0] if kept else None
        from .train import forward_step
        self.forward_step = forward_step(cls_score, '_head_step')    # (which weights the forward ran with: head_backward's guard)
        return self.result
