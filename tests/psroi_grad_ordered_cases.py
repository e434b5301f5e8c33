"""Inputs and a NumPy-scalar restatement for the order-exact PsRoiAlign gradient (xdet_psroialign_grad_ordered), shared by
tests/test_psroialign_grad_ordered_math.py (no GPU) and tests/test_gpu_psroialign_grad_ordered.py."""
import numpy as np

F32 = np.float32
SEED = 23          # chosen on the CPU: with it the reversed-ROI restatement differs from the oracle on the heavy-overlap input
# (N, C, H, W, R, grid)
SMALL = (3, 16, 5, 7, 9, 2)        # bank 4, tiny map: every ROI overlaps every other, so order decides the bits
PLANES10K = (2, 36, 50, 50, 64, 3)  # 10 KB planes
NET = (1, 490, 30, 30, 300, 7)     # the net's shape; the channels do not fill the last workgroup
HEAVY = (1, 16, 5, 7, 64, 2)       # all ROIs the same full-image box, 'mean': every pixel sums hundreds of terms


def random_rois(rng, n, r):
    """tests/test_gpu_psroialign.py::random_rois (copied: importing that module would collect its tests twice)"""
    cy, cx = rng.uniform(0.02, 0.98, (n, r)), rng.uniform(0.02, 0.98, (n, r))
    h, w = rng.uniform(0.01, 1.0, (n, r)), rng.uniform(0.01, 1.0, (n, r))
    rois = np.stack([cy, cx, h, w], -1).astype(np.float32)
    # edge cases: full image, 1-pixel, image border, the fallback box, degenerate (zero h / w)
    rois[:, 0] = [0.5, 0.5, 1.0, 1.0]
    rois[:, 1] = [0.5, 0.5, 1. / 30, 1. / 30]
    rois[:, 2] = [0.0, 0.0, 0.3, 0.3]
    rois[:, 3] = [1.0, 1.0, 0.2, 0.2]
    rois[:, 4] = [0.5, 0.5, 0.6, 0.6]
    rois[:, 5] = [0.5, 0.5, 0.0, 0.4]
    rois[:, 6] = [0.5, 0.5, 0.4, 0.0]
    rois[:, 7] = [0.999, 0.001, 0.001, 0.001]
    return rois


_cache = {}


def case(shape, method, oracle):
    """-> (rois, grad [N,R,C], index [N,R,C] from the oracle's forward, reference [N,C,H,W] from the oracle's gradient);
    computed once per (shape, method) and shared -- treat as read-only"""
    key = (shape, method)
    if key not in _cache:
        n, c, h, w, r, g = shape
        rng = np.random.default_rng(SEED)
        feat = rng.standard_normal((n, c, h, w)).astype(F32)
        if shape == HEAVY:
            rois = np.tile(np.array([0.5, 0.5, 1.0, 1.0], F32), (n, r, 1))
        else:
            rois = random_rois(rng, n, max(r, 8))[:, :r]
        grad = rng.standard_normal((n, r, c)).astype(F32)
        if shape != HEAVY:
            grad[:, 2::3] = 0                       # whole rows of zeros, as OHEM leaves them
        _, index = oracle.ps_roi_align(feat, rois, g, g, method)
        index = np.ascontiguousarray(index.reshape(n, r, c))
        ref = oracle.ps_roi_align_grad(feat, rois, grad, index, g, g, method)
        for a in (rois, grad, index, ref):
            a.setflags(write=False)
        _cache[key] = (rois, grad, index, ref)
    return _cache[key]


def grad_np(rois, grad, index, shape, method, reverse_rois=False):
    """NumPy-scalar restatement (NCHW) of the order rule: per output element the contributions are added in the order ROI
    index, sample row i, sample column j, then the corners (iy,ix), (iy1,ix), (iy,ix1), (iy1,ix1), each a separately rounded
    f32 add of a weight evaluated as in oracle/psroialign_ref.c (three double products, fx*fy*g in float).
    reverse_rois: the same terms with the ROIs of an image walked backwards -- another order."""
    n_img, C, H, W, R, gw = shape
    gh = gw
    bank = C // (gw * gh)
    use_max = 'max' in method
    out = np.zeros((n_img, C, H, W), F32)
    FMIN = np.finfo(F32).tiny
    for n in range(n_img):
        for r in (range(R - 1, -1, -1) if reverse_rois else range(R)):
            roi = rois[n, r]
            if roi[2] < FMIN or roi[3] < FMIN:
                continue
            yc = F32(roi[0] * F32(H)); xc = F32(roi[1] * F32(W))
            rh = max(F32(roi[2] * F32(H)), F32(1)); rw = max(F32(roi[3] * F32(W)), F32(1))
            ymin = max(F32(yc - F32(rh / F32(2))), F32(0)); xmin = max(F32(xc - F32(rw / F32(2))), F32(0))
            ymax = min(F32(yc + F32(rh / F32(2))), F32(F32(H) - FMIN)); xmax = min(F32(xc + F32(rw / F32(2))), F32(F32(W) - FMIN))
            bin_w = F32(F32(xmax - xmin) / F32(gw)); bin_h = F32(F32(ymax - ymin) / F32(gh))
            n_w = int(bin_w) + 1; n_h = int(bin_h) + 1
            step_w = F32(bin_w / F32(n_w)); step_h = F32(bin_h / F32(n_h))
            for c in range(C):
                pos = c // bank
                row, col = pos // gw, pos % gw
                x0 = F32(xmin + F32(bin_w * F32(col))); y0 = F32(ymin + F32(bin_h * F32(row)))
                if use_max:
                    pi = int(index[n, r, c])
                    samples = [(pi // n_w, pi % n_w)]
                    g = F32(grad[n, r, c])
                else:
                    samples = [(i, j) for i in range(n_h) for j in range(n_w)]
                    g = F32(grad[n, r, c] / F32(n_w * n_h))
                plane = out[n, c]
                for i, j in samples:
                    x = F32(np.float64(F32(x0 + F32(step_w * F32(j)))) + np.float64(step_w) / 2.)
                    y = F32(np.float64(F32(y0 + F32(step_h * F32(i)))) + np.float64(step_h) / 2.)
                    ix, iy = int(x), int(y)
                    fx32 = F32(x - F32(ix)); fy32 = F32(y - F32(iy))
                    fx = np.float64(fx32); fy = np.float64(fy32)
                    iy1, ix1 = min(iy + 1, H - 1), min(ix + 1, W - 1)
                    g64 = np.float64(g)
                    plane[iy, ix] = F32(plane[iy, ix] + F32((1. - fx) * (1. - fy) * g64))
                    plane[iy1, ix] = F32(plane[iy1, ix] + F32((1. - fx) * fy * g64))
                    plane[iy, ix1] = F32(plane[iy, ix1] + F32(fx * (1. - fy) * g64))
                    plane[iy1, ix1] = F32(plane[iy1, ix1] + F32(F32(fx32 * fy32) * g))
    return out


def corners_of(rois):
    """centre boxes -> corner boxes whose f32 _point2center conversion is returned alongside: (corners, centres) with
    hh = y1 - y0; cy = y0 + hh / 2, each step in f32"""
    rois = np.asarray(rois, F32)
    cy, cx, h, w = (rois[..., k] for k in range(4))
    y0, x0 = (cy - h / F32(2)).astype(F32), (cx - w / F32(2)).astype(F32)
    y1, x1 = (y0 + h).astype(F32), (x0 + w).astype(F32)
    corners = np.stack([y0, x0, y1, x1], -1).astype(F32)
    return corners, point2center(corners)


def point2center(corners):
    corners = np.asarray(corners, F32)
    hh = (corners[..., 2] - corners[..., 0]).astype(F32)
    ww = (corners[..., 3] - corners[..., 1]).astype(F32)
    cy = (corners[..., 0] + (hh / F32(2)).astype(F32)).astype(F32)
    cx = (corners[..., 1] + (ww / F32(2)).astype(F32)).astype(F32)
    return np.stack([cy, cx, hh, ww], -1).astype(F32)


# the refusals of include/xdet.h for xdet_psroialign_grad_ordered, with pointers that are never dereferenced
P = 4096
OK_ARGS = dict(rois=P, grad=P, ld_grad=16, index=P, ld_index=16, out=P, N=1, C=16, H=5, W=7, R=9, gw=2, gh=2, use_max=1,
               layout=0, ldc=16, corners=0)
REFUSALS = [dict(ld_grad=15), dict(ld_index=15), dict(H=512, W=512), dict(index=None), dict(C=18, ld_grad=18, ld_index=18, ldc=18),
            dict(gw=0), dict(layout=2), dict(layout=1, ldc=15), dict(rois=None), dict(grad=None), dict(out=None), dict(N=-1),
            dict(H=0)]


def c_call(l, **kw):
    v = dict(OK_ARGS, **kw)
    return l.xdet_psroialign_grad_ordered(v['rois'], v['grad'], v['ld_grad'], v['index'], v['ld_index'], v['out'], v['N'], v['C'],
                                          v['H'], v['W'], v['R'], v['gw'], v['gh'], v['use_max'], v['layout'], v['ldc'],
                                          v['corners'], None)
