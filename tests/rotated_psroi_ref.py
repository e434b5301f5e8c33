"""TEST INFRASTRUCTURE, NOT PRODUCT CODE: a NumPy restatement of the reference's RotatedPsRoiAlign forward and
gradient (cpp/PSROIPooling/rotated_ps_roi_align_op.cc:163-292, rotated_ps_roi_align_grad_op.cu:37-170).

Every step is written with explicit float32 / float64 types so that it rounds as the reference's C++ does: an
operand that meets a `1.` or `2.` literal is evaluated in double and the result rounded to float; everything else is
float.  (NumPy would keep a float32 array times a Python float in float32 -- hence the explicit casts.)  The forward
is bit-exact against tests/golden/rotated_psroi_golden.npz; the gradient scatters the same per-corner float terms as
the reference's CUDA kernel, summed in another order (agreement to rounding).

Out-of-bounds samples follow the product's rule (include/xdet.h): the integer cell is clamped into [0, size - 1],
the fractional weights stay the reference's.  Where the reference reads in bounds this is the reference itself.
"""
import numpy as np

f32, f64 = np.float32, np.float64
FLT_MIN = f64(np.finfo(np.float32).tiny)
LOWEST = np.finfo(np.float32).min


def _min(a, b):                       # std::min(a, b): (b < a) ? b : a
    return np.where(b < a, b, a)


def _max(a, b):                       # std::max(a, b): (a < b) ? b : a
    return np.where(a < b, b, a)


def vertices(rois, orders, H, W):
    """rois [M,8] f32, orders [M] i32 -> (y [M,4], x [M,4]) f32 in the order the pooling walks them, degenerate [M]"""
    rois = np.asarray(rois, f32).reshape(-1, 8)
    orders = np.asarray(orders, np.int64).reshape(-1)
    ys, xs = rois[:, 0::2] * f32(H), rois[:, 1::2] * f32(W)          # float * int -> float (:187-194)
    start = np.where(orders < 0, 0, orders % 4)                        # order >= 0: vertex order mod 4
    k = (start[:, None] + np.arange(4)[None, :]) % 4
    ys, xs = np.take_along_axis(ys, k, 1), np.take_along_axis(xs, k, 1)
    dy = ys[:, [1, 2, 3, 0]] - ys                                      # side k: vertex k -> k + 1 (:196-199)
    dx = xs[:, [1, 2, 3, 0]] - xs
    ln = (dy * dy + dx * dx).astype(f64)                               # float products, widened
    shift = np.where(orders < 0, (ln[:, 0] + ln[:, 2] > ln[:, 1] + ln[:, 3]).astype(np.int64), 0)   # (:203)
    degenerate = np.any(ln < FLT_MIN, axis=1)                          # (:205-211)
    k = (shift[:, None] + np.arange(4)[None, :]) % 4
    return np.take_along_axis(ys, k, 1), np.take_along_axis(xs, k, 1), degenerate


def bin_geometry(y, x, gw, gh, cap):
    """per (ROI, bin): the four bin corners reduced to what the samples need (:222-255).
    Returns dict of [M,G] arrays: ltx, lbx, gxst, gxsb (column geometry), lty, rty, gysl, gysr (row geometry), nw, nh.
    Sample counts are int(extent) + 1 with the extent clamped to [0, cap = H + W] (the product's cap, never reached
    by a quad inside [0,1])."""
    G = gw * gh
    r = (np.arange(G) // gw)[None, :]
    c = (np.arange(G) % gw)[None, :]
    rf, cf = r.astype(f32), c.astype(f32)
    y0, y1, y2, y3 = (y[:, k:k + 1] for k in range(4))
    x0, x1, x2, x3 = (x[:, k:k + 1] for k in range(4))
    ysl = ((y3 - y0).astype(f64) / f64(gh)).astype(f32)
    ysr = ((y2 - y1).astype(f64) / f64(gh)).astype(f32)
    xst = ((x1 - x0).astype(f64) / f64(gw)).astype(f32)
    xsb = ((x2 - x3).astype(f64) / f64(gw)).astype(f32)
    left_y1 = y0 + rf * ysl
    right_y1 = y1 + rf * ysr
    left_y2 = (y0.astype(f64) + (r + 1.) * ysl.astype(f64)).astype(f32)
    right_y2 = (y1.astype(f64) + (r + 1.) * ysr.astype(f64)).astype(f32)
    lty = left_y1 + (cf * (right_y1 - left_y1)) / f32(gw)
    rty = (left_y1.astype(f64) + ((c + 1.) * (right_y1 - left_y1).astype(f64)) / f64(gw)).astype(f32)
    lby = left_y2 + (cf * (right_y2 - left_y2)) / f32(gw)
    rby = (left_y2.astype(f64) + ((c + 1.) * (right_y2 - left_y2).astype(f64)) / f64(gw)).astype(f32)
    top_x1 = x0 + cf * xst
    bottom_x1 = x3 + cf * xsb
    top_x2 = (x0.astype(f64) + (c + 1.) * xst.astype(f64)).astype(f32)
    bottom_x2 = (x3.astype(f64) + (c + 1.) * xsb.astype(f64)).astype(f32)
    ltx = top_x1 + (rf * (bottom_x1 - top_x1)) / f32(gh)
    lbx = (top_x1.astype(f64) + ((r + 1.) * (bottom_x1 - top_x1).astype(f64)) / f64(gh)).astype(f32)
    rtx = top_x2 + (rf * (bottom_x2 - top_x2)) / f32(gh)
    rbx = (top_x2.astype(f64) + ((r + 1.) * (bottom_x2 - top_x2).astype(f64)) / f64(gh)).astype(f32)
    bw = _max(_min(np.abs(rtx - ltx), np.abs(rty - lty)), _min(np.abs(rbx - lbx), np.abs(rby - lby)))
    bh = _max(_min(np.abs(lbx - ltx), np.abs(lby - lty)), _min(np.abs(rbx - rtx), np.abs(rby - rty)))
    with np.errstate(invalid='ignore'):
        nw = np.trunc(np.clip(np.nan_to_num(bw.astype(f64), nan=0.), 0., cap)).astype(np.int64) + 1
        nh = np.trunc(np.clip(np.nan_to_num(bh.astype(f64), nan=0.), 0., cap)).astype(np.int64) + 1
    gysl = ((lby - lty).astype(f64) / (nh + 1.)).astype(f32)
    gysr = ((rby - rty).astype(f64) / (nh + 1.)).astype(f32)
    gxst = ((rtx - ltx).astype(f64) / (nw + 1.)).astype(f32)
    gxsb = ((rbx - lbx).astype(f64) / (nw + 1.)).astype(f32)
    return dict(ltx=ltx, lbx=lbx, gxst=gxst, gxsb=gxsb, lty=lty, rty=rty, gysl=gysl, gysr=gysr, nw=nw, nh=nh)


def sample_coord(a, b, sa, sb, k):
    """(a + (k + 1.) * sa + b + (k + 1.) * sb) / 2. in double, rounded to float (:263-264); k broadcasts"""
    t = k + 1.
    return ((((a.astype(f64) + t * sa.astype(f64)) + b.astype(f64)) + t * sb.astype(f64)) / 2.).astype(f32)


def cell(v, size):
    """(integer cell clamped into [0, size - 1], its +1 neighbour clamped to size - 1, fraction v - trunc(v), raw cell)"""
    with np.errstate(invalid='ignore'):
        vt = np.trunc(v) + f32(0.)          # (+0: trunc(-0.5) is -0., the reference's (float)(int)v is +0.)
        frac = (v - vt).astype(f32)
        raw = np.clip(np.nan_to_num(vt.astype(f64), nan=0.), -2. ** 31, 2. ** 31 - 1).astype(np.int64)
    i0 = np.clip(raw, 0, size - 1)
    return i0, np.minimum(i0 + 1, size - 1), frac, raw


def _groups(geo, live, chunk=4096):
    """(ROI-bin flat indices) grouped by (nh, nw), in chunks"""
    nh, nw = geo['nh'].ravel(), geo['nw'].ravel()
    idx = np.nonzero(live.ravel())[0]
    if idx.size == 0:
        return
    keys = nh[idx] * 1000003 + nw[idx]
    order = np.argsort(keys, kind='stable')
    idx, keys = idx[order], keys[order]
    cuts = np.nonzero(np.diff(keys))[0] + 1
    for grp in np.split(idx, cuts):
        for s in range(0, grp.size, chunk):
            g = grp[s:s + chunk]
            yield g, int(nh[g[0]]), int(nw[g[0]])


def _samples(geo, g, nh, nw, H, W):
    """for ROI-bins g with nh x nw samples: row cells [B,nh] and column cells [B,nw]"""
    fl = {k: v.ravel()[g][:, None] for k, v in geo.items()}
    ys = sample_coord(fl['lty'], fl['rty'], fl['gysl'], fl['gysr'], np.arange(nh)[None, :])
    xs = sample_coord(fl['ltx'], fl['lbx'], fl['gxst'], fl['gxsb'], np.arange(nw)[None, :])
    return cell(ys, H), cell(xs, W)


def _prepare(inputs, rois, orders, gw, gh):
    N, C, H, W = inputs.shape
    R = np.asarray(rois).shape[1]
    G = gw * gh
    y, x, deg = vertices(np.asarray(rois, f32).reshape(N * R, 8), np.asarray(orders).reshape(N * R), H, W)
    geo = bin_geometry(y, x, gw, gh, H + W)
    live = np.broadcast_to(~deg[:, None], (N * R, G))
    return N, C, H, W, R, G, C // G, geo, live


def forward(inputs, rois, orders, gw, gh, pool_method):
    """inputs [N,C,H,W] f32 NCHW, rois [N,R,8], orders [N,R] -> (pooled [N,R,G,bank] f32, index i32)"""
    inputs = np.asarray(inputs, f32)
    use_max = 'max' in pool_method
    N, C, H, W, R, G, bank, geo, live = _prepare(inputs, rois, orders, gw, gh)
    out = np.zeros((N * R, G, bank), f32)
    idx = np.zeros((N * R, G, bank), np.int32)
    ch = np.arange(bank)
    for g, nh, nw in _groups(geo, live):
        (iy0, iy1, fy, _), (ix0, ix1, fx, _) = _samples(geo, g, nh, nw, H, W)
        m, b = g // G, g % G
        n = (m // R)[:, None, None, None]
        c = (b[:, None] * bank + ch[None, :])[:, :, None, None]            # [B,bank,1,1]
        Y0, Y1 = iy0[:, None, :, None], iy1[:, None, :, None]
        X0, X1 = ix0[:, None, None, :], ix1[:, None, None, :]
        f00, f10 = inputs[n, c, Y0, X0], inputs[n, c, Y1, X0]
        f01, f11 = inputs[n, c, Y0, X1], inputs[n, c, Y1, X1]
        FX, FY = fx[:, None, None, :], fy[:, None, :, None]
        wx0, wy0 = 1. - FX.astype(f64), 1. - FY.astype(f64)
        v = (((wx0 * wy0) * f00 + (wx0 * FY.astype(f64)) * f10) + (FX.astype(f64) * wy0) * f01
             + ((FX * FY) * f11).astype(f64)).astype(f32)                  # [B,bank,nh,nw] (:273-276)
        v = v.reshape(v.shape[0], bank, nh * nw)
        if use_max:
            acc = np.full(v.shape[:2], LOWEST, f32)
            arg = np.zeros(v.shape[:2], np.int32)
            for s in range(nh * nw):                                     # strict <: the first maximum wins
                t = v[:, :, s]
                upd = acc < t
                acc = np.where(upd, t, acc)
                arg = np.where(upd, np.int32(s), arg)
        else:
            acc = np.zeros(v.shape[:2], f32)
            for s in range(nh * nw):                                     # sequential float sum
                acc = (acc + v[:, :, s]).astype(f32)
            acc = (acc / f32(nh * nw)).astype(f32)
            arg = np.zeros(v.shape[:2], np.int32)
        out[m, b] = acc
        idx[m, b] = arg
    return out.reshape(N, R, G, bank), idx.reshape(N, R, G, bank)


def gradient(input_shape, rois, orders, grad, index, gw, gh, pool_method):
    """the CUDA scatter (rotated_ps_roi_align_grad_op.cu:132-166) accumulated in float64: grad_inputs [N,C,H,W] f32"""
    N, C, H, W = input_shape
    use_max = 'max' in pool_method
    _, _, _, _, R, G, bank, geo, live = _prepare(np.empty((N, C, H, W), np.uint8), rois, orders, gw, gh)
    grad = np.asarray(grad, f32).reshape(N * R, G, bank)
    index = np.asarray(index, np.int64).reshape(N * R, G, bank)
    acc = np.zeros(N * C * H * W, f64)
    ch = np.arange(bank)
    for g, nh, nw in _groups(geo, live):
        (iy0, iy1, fy, _), (ix0, ix1, fx, _) = _samples(geo, g, nh, nw, H, W)
        m, b = g // G, g % G
        n = (m // R)[:, None]
        c = b[:, None] * bank + ch[None, :]                                # [B,bank]
        gin = grad[m, b]                                                   # [B,bank]
        if use_max:
            pi = index[m, b]
            (Y0, Y1, FY), (X0, X1, FX) = _sample_at(geo, g, pi // nw, pi % nw, H, W)
            g_ = gin
        else:
            Y0, Y1, FY = (a[:, None, :, None] for a in (iy0, iy1, fy))
            X0, X1, FX = (a[:, None, None, :] for a in (ix0, ix1, fx))
            g_ = (gin / f32(nh * nw)).astype(f32)[:, :, None, None]
            n, c = n[:, :, None, None], c[:, :, None, None]
        gd = g_.astype(f64)
        wx0, wy0 = 1. - FX.astype(f64), 1. - FY.astype(f64)
        terms = [(Y0, X0, ((wx0 * wy0) * gd).astype(f32)), (Y1, X0, ((wx0 * FY.astype(f64)) * gd).astype(f32)),
                 (Y0, X1, ((FX.astype(f64) * wy0) * gd).astype(f32)), (Y1, X1, ((FX * FY) * g_).astype(f32))]
        for Y, X, t in terms:
            flat = ((n * C + c) * H + Y) * W + X
            flat, t = np.broadcast_arrays(flat, t)
            np.add.at(acc, flat.ravel(), t.ravel().astype(f64))
    return acc.astype(f32).reshape(N, C, H, W)


def _sample_at(geo, g, ph, pw, H, W):
    """row / column cells of ONE sample (ph, pw) [B,bank] per ROI-bin g"""
    fl = {k: v.ravel()[g][:, None] for k, v in geo.items()}
    ys = sample_coord(fl['lty'], fl['rty'], fl['gysl'], fl['gysr'], ph)
    xs = sample_coord(fl['ltx'], fl['lbx'], fl['gxst'], fl['gxsb'], pw)
    y0, y1, fy, _ = cell(ys, H)
    x0, x1, fx, _ = cell(xs, W)
    return (y0, y1, fy), (x0, x1, fx)


def out_of_bounds(rois, orders, H, W, gw, gh):
    """[N,R] bool: some sample of the ROI has an integer cell outside the map (where the reference reads outside the
    plane and the product clamps)"""
    rois = np.asarray(rois, f32)
    N, R = rois.shape[:2]
    y, x, deg = vertices(rois.reshape(N * R, 8), np.asarray(orders).reshape(N * R), H, W)
    geo = bin_geometry(y, x, gw, gh, H + W)
    G = gw * gh
    bad = np.zeros(N * R * G, bool)
    for g, nh, nw in _groups(geo, np.broadcast_to(~deg[:, None], (N * R, G))):
        (_, _, _, ry), (_, _, _, rx) = _samples(geo, g, nh, nw, H, W)
        bad[g] = np.any((ry < 0) | (ry > H - 1), 1) | np.any((rx < 0) | (rx > W - 1), 1)
    return bad.reshape(N, R, G).any(2)


def mean_samples(rois, orders, H, W, gw, gh):
    """mean number of samples per output element (non-degenerate ROIs)"""
    rois = np.asarray(rois, f32)
    y, x, deg = vertices(rois.reshape(-1, 8), np.asarray(orders).reshape(-1), H, W)
    geo = bin_geometry(y, x, gw, gh, H + W)
    s = (geo['nh'] * geo['nw'])[~deg]
    return float(s.mean()) if s.size else 0.
