"""The op-level doors of the training path, re-exported by xdet/ops.py: per op the NumPy statement (host_*), the door that
leaves its results on the GPU (*_device) and the door that returns NumPy arrays.  Every *_device door runs in one order -- all
argument checks; uploads and allocations; the single library call; keep-alives -- and synchronises nothing; given dx= / out= /
workspace=, it allocates no activation-sized memory."""
import math

import numpy as np

from ._lib import lib, check, InvalidArgumentError, MomentumSlot, GradSlot, LayerRefresh, PackSlot, CrcSlot
from .runtime import DeviceBuffer, DeviceTensor, to_device, to_host, synchronize

__all__ = ['host_dense_backward', 'dense_backward_device', 'dense_backward',
           'host_conv_backward', 'conv_backward_device', 'conv_backward',
           'host_conv_backward_strided', 'conv_backward_strided_device', 'conv_backward_strided',
           'host_batch_norm_forward', 'host_batch_norm_backward', 'batch_norm_forward_device', 'batch_norm_forward',
           'batch_norm_backward_device', 'batch_norm_backward',
           'host_depthwise_backward', 'depthwise_backward_device', 'depthwise_backward', 'add_rows_device',
           'host_max_pool_backward', 'host_subsample2', 'host_add_upsample2', 'max_pool_backward_device', 'max_pool_backward',
           'subsample2_device', 'add_upsample2_device', 'host_momentum_step', 'momentum_step_device',
           'host_grad_stats', 'grad_stats_device', 'host_clip_scale', 'host_grad_sq',
           'host_bn_fold', 'bn_fold_device', 'refresh_layers_table', 'refresh_layers_device',
           'host_concat', 'host_split', 'concat_device', 'split_device', 'crc32c_table', 'crc32c_launch', 'crc32c_device',
           'host_average_gradients', 'grad_flat_offsets', 'grad_pack_device', 'grad_reduce_ranks_device']


# ---- the operand path every door below takes ------------------------------------------------------------------------------

_FORMS = {2: 'be a matrix', 4: 'have four dimensions', None: 'have rows of channels'}


def _operand(a, who, what, ndim):
    """Describe an operand without touching the GPU: a DeviceTensor ([N,H,W,C] with its ld: N*H*W rows of C), or an array of
    `ndim` dimensions (None: two or more, every leading axis a row axis) -> (shape, rows, width, DeviceTensor or f32 array)"""
    if not isinstance(a, DeviceTensor):
        a = np.ascontiguousarray(a, np.float32)
        if (a.ndim != ndim) if ndim else (a.ndim < 2):
            raise InvalidArgumentError(-1, '%s: %s must %s, got shape %r' % (who, what, _FORMS[ndim], a.shape))
    shape = tuple(a.shape)
    return shape, int(np.prod(shape[:-1])), int(shape[-1]), a


def _check_sizes(rows, widths, said, args, widest=4096, also=True):
    """The size rule of the C doors (include/xdet.h): every factor of the row count and every width positive, no width above
    `widest` (None: no limit), rows * the widest width below 2^31 -- and `also`, the door's own; `said % args` is its sentence"""
    w = max(widths)
    if min(rows + widths) <= 0 or (widest is not None and w > widest) or math.prod(rows) * w >= 2 ** 31 or not also:
        raise InvalidArgumentError(-1, said % args)


_BN_SIZES = '%s: M = %d, C = %d (positive, C at most 4096, M * C below 2^31)'
_POOL_SIZES = '%s: [%d,%d,%d,%d] (sizes positive, C at most 4096, N*H*W*C below 2^31)'


def _given(t, shape, who, what='dx'):
    """a caller's result tensor (dx= / out=) or None: given, it is a DeviceTensor of the result's shape, written with its ld"""
    if t is not None and (not isinstance(t, DeviceTensor) or tuple(t.shape) != tuple(shape)):
        raise InvalidArgumentError(-1, '%s: %s must be a DeviceTensor of shape %r, got %r' % (who, what, tuple(shape), getattr(t, 'shape', None)))
    return t


def _on_device(a, width, padded=False):
    """Put an operand on the device -> (keep-alive, pointer, ld).  A DeviceTensor is read in place with its ld.  An array is
    copied there: densely, ld = width (the dense, conv, batch-norm and depthwise doors), or with padded=True as
    DeviceTensor.from_numpy lays out an [N,H,W,C] activation, ld = channel_ld(C) (the pool and add doors)."""
    if isinstance(a, DeviceTensor):
        return a, a.ptr, a.ld
    if padded:
        return _on_device(DeviceTensor.from_numpy(a), width)
    b = to_device(a)
    return b, b.ptr, width


def _result(given, shape, ld):
    """the caller's tensor, or a new one of this ld"""
    return given if given is not None else DeviceTensor.empty(shape, ld=ld)


def _keep_alive(results, alive, chain=False):
    """Operands and workspace live until the stream has run the call: every result that is not None holds them as _keep.  chain:
    a caller's out may be an operand that a pending call wrote -- on top of what it already keeps alive, and never itself."""
    for r in results:
        if r is not None:
            held = tuple(k for k in alive if k is not r)
            r._keep = (getattr(r, '_keep', None),) + held if chain else held


def _handle(stream):
    return stream.handle if stream else None


# ---- the backward of a dense layer (xdet_dense_backward, csrc/dense_backward.hip) -------------------------------------

def host_dense_backward(x, w, dy, y=None, dtype=np.float32, with_dx=True):
    """The NumPy statement of xdet_dense_backward (include/xdet.h) for a layer y = act(x w + b): x [M,K], w [K,J], dy [M,J],
    y [M,J] the forward's output after its ReLU (None: no ReLU) -> (dx [M,K] = g w^T, dw [K,J] = x^T g, db [J] = column
    sums of g) with g = dy, or dy where y > 0 and 0 elsewhere (an exact zero and a NaN in y both give 0).  dtype float32,
    or float64: the accuracy yardstick.  with_dx=False: dx is None."""
    x, w, dy = np.asarray(x, dtype), np.asarray(w, dtype), np.asarray(dy, dtype)
    g = dy
    if y is not None:
        with np.errstate(invalid='ignore'):
            g = np.where(np.asarray(y, dtype) > 0, dy, dtype(0))
    dx = np.matmul(g, w.T).astype(dtype) if with_dx else None
    return dx, np.matmul(x.T, g).astype(dtype), g.sum(axis=0, dtype=dtype)


def dense_backward_device(x, w, dy, y=None, with_dx=True, stream=None):
    """dense_backward with the results left on the GPU: (dx DeviceTensor [M,1,1,K] with ld K or None, dw DeviceBuffer [K,J],
    db DeviceBuffer [J]); nothing is synchronised."""
    who = 'dense_backward'
    _, M, K, x_in = _operand(x, who, 'x', 2)
    _, Kw, J, w_in = _operand(w, who, 'w', 2)
    _, Md, Jd, dy_in = _operand(dy, who, 'dy', 2)
    bad = (Kw, Md, Jd) != (K, M, J)
    if y is not None:
        _, My, Jy, y_in = _operand(y, who, 'y', 2)
        bad = bad or (My, Jy) != (M, J)
    if bad:
        raise InvalidArgumentError(-1, 'dense_backward: x [M,K], w [K,J], dy [M,J] and y [M,J] expected, got %r'
                                   % ([(M, K), (Kw, J), (Md, Jd)] + ([(My, Jy)] if y is not None else []),))
    _check_sizes((M,), (K, J), 'dense_backward: M = %d, K = %d, J = %d (positive, K and J at most 4096, '
                               'M * max(K, J) below 2^31)', (M, K, J))
    if isinstance(w_in, DeviceTensor) and w_in.ld != J:
        raise InvalidArgumentError(-1, 'dense_backward: w must be dense on the device (ld %d, J = %d)' % (w_in.ld, J))
    kx, px, ldx = _on_device(x_in, K)
    kw, pw, _ = _on_device(w_in, J)
    kd, pd, ldd = _on_device(dy_in, J)
    ky, py, ldy = _on_device(y_in, J) if y is not None else (None, None, 0)
    d_dx = _result(None, (M, 1, 1, K), K) if with_dx else None
    d_dw, d_db = DeviceBuffer(K * J * 4), DeviceBuffer(max(J * 4, 16))
    ws = DeviceBuffer(lib().xdet_dense_backward_workspace_bytes(M, K, J))
    check(lib().xdet_dense_backward(px, ldx, pw, py, ldy, pd, ldd, M, K, J, d_dx.ptr if with_dx else None, K, d_dw.ptr,
                                    d_db.ptr, ws.ptr, _handle(stream)))
    _keep_alive((d_dx, d_dw), (kx, kw, kd, ky, ws))
    return d_dx, d_dw, d_db


def dense_backward(x, w, dy, y=None, with_dx=True, stream=None):
    """host_dense_backward on the GPU (xdet_dense_backward): x [M,K], w [K,J], dy [M,J], y [M,J] or None as NumPy arrays or
    DeviceTensors (read in place with their ld; [N,H,W,C] counts as N*H*W rows of C) -> (dx [M,K] or None, dw [K,J],
    db [J]) as NumPy arrays."""
    d_dx, d_dw, d_db = dense_backward_device(x, w, dy, y, with_dx, stream)
    synchronize(stream)
    J = int((w.shape if isinstance(w, DeviceTensor) else np.shape(w))[-1])
    K = d_dw.nbytes // (4 * J)
    dx = to_host(d_dx.ptr, (d_dx.shape[0], K), np.float32, stream) if d_dx is not None else None
    return dx, to_host(d_dw.ptr, (K, J), np.float32, stream), to_host(d_db.ptr, (J,), np.float32, stream)


# ---- the backward of a stride-1 'SAME' convolution (xdet_conv_backward, csrc/conv_backward.hip) ------------------------

def host_conv_backward(x, w, dy, y=None, relu_in=False, dtype=np.float32, with_dx=True):
    """The NumPy statement of xdet_conv_backward (include/xdet.h) for y = act(conv(xe, w) + b), stride 1, 'SAME', NHWC:
    x [N,H,W,C], w [kh,kw,C,J] (kh, kw odd), dy [N,H,W,J], y [N,H,W,J] the forward's output after its ReLU (None: no ReLU);
    xe = x, or with relu_in x where x > 0 and 0 elsewhere -> (dx [N,H,W,C], dw [kh,kw,C,J], db [J]) with g = dy, or dy where
    y > 0 and 0 elsewhere (an exact zero and a NaN both give 0, in y and in x); with relu_in dx is 0 wherever x > 0 is
    false.  One matrix product per tap, the taps added in storage order.  dtype float32, or float64: the accuracy yardstick.
    with_dx=False: dx is None.  It is host_conv_backward_strided's statement at stride 1, 'SAME'."""
    return host_conv_backward_strided(x, w, dy, y, relu_in, dtype, with_dx, stride=1, padding='SAME')


def conv_backward_device(x, w, dy, y=None, relu_in=False, with_dx=True, stream=None, dx=None, workspace=None):
    """conv_backward with the results left on the GPU: (dx DeviceTensor [N,H,W,C] with x's ld (C for a NumPy x) or None,
    dw DeviceBuffer [kh,kw,C,J], db DeviceBuffer [J]); nothing is synchronised.  A DeviceTensor w is [kh,kw,C,J] dense.
    dx: a DeviceTensor [N,H,W,C] to write instead of a new one (with its ld); workspace: a DeviceBuffer of at least
    xdet_conv_backward_workspace_bytes(N, H, W, C, J, kh, kw) bytes (default: allocated here) -- a chain of calls on one
    stream then allocates no activation-sized memory per call."""
    return _conv_backward_device('conv_backward', x, w, dy, y, relu_in, with_dx, stream, dx, workspace, 1, 'SAME')


def conv_backward(x, w, dy, y=None, relu_in=False, with_dx=True, stream=None):
    """host_conv_backward on the GPU (xdet_conv_backward): x [N,H,W,C], w [kh,kw,C,J], dy [N,H,W,J], y [N,H,W,J] or None as
    NumPy arrays or DeviceTensors (read in place with their ld) -> (dx [N,H,W,C] or None, dw [kh,kw,C,J], db [J]) as NumPy
    arrays."""
    return _conv_results_to_host(conv_backward_device(x, w, dy, y, relu_in, with_dx, stream), w, stream)


# ---- the backward of a conv at stride 1 or 2, 'VALID' or 'SAME' (xdet_conv_backward_strided, csrc/conv_backward.hip) ------

_PADDINGS = {'VALID': 0, 'SAME': 1}          # pad_mode of xdet_conv_create


def _strided_geometry(H, W, kh, kw, stride, padding, who='conv_backward_strided'):
    """-> (Ho, Wo, pt, pl): the output map and the padding in front, by include/xdet.h's rules ('SAME' is TensorFlow's); the
    refusals that need no tensor come from here"""
    if isinstance(stride, bool) or stride not in (1, 2):
        raise InvalidArgumentError(-1, '%s: stride must be 1 or 2, got %r' % (who, stride))
    if not isinstance(padding, str) or padding not in _PADDINGS:
        raise InvalidArgumentError(-1, "%s: padding must be 'VALID' or 'SAME', got %r" % (who, padding))
    if min(kh, kw) <= 0 or kh % 2 == 0 or kw % 2 == 0 or max(kh, kw) > 15:
        raise InvalidArgumentError(-1, '%s: kernel %d x %d (kh and kw odd and at most 15)' % (who, kh, kw))
    if padding == 'SAME':
        Ho, Wo = -(-H // stride), -(-W // stride)
        return Ho, Wo, max((Ho - 1) * stride + kh - H, 0) // 2, max((Wo - 1) * stride + kw - W, 0) // 2
    if kh > H or kw > W:
        raise InvalidArgumentError(-1, "%s: a 'VALID' kernel %d x %d is larger than the map %d x %d" % (who, kh, kw, H, W))
    return (H - kh) // stride + 1, (W - kw) // stride + 1, 0, 0


def host_conv_backward_strided(x, w, dy, y=None, relu_in=False, dtype=np.float32, with_dx=True, stride=1, padding='SAME'):
    """The NumPy statement of xdet_conv_backward_strided (include/xdet.h): host_conv_backward with stride 1 or 2 and padding
    'VALID' or 'SAME' (TensorFlow's: the smaller half in front).  x [N,H,W,C], w [kh,kw,C,J], dy and y [N,Ho,Wo,J] ->
    (dx [N,H,W,C], dw [kh,kw,C,J], db [J]); output pixel (oh, ow) read input pixel (oh*stride + a - pt, ow*stride + b - pl)
    through tap (a, b).  One matrix product per tap, the taps added in storage order: dw's over the strided view of the padded
    xe, dx's over g spread out on a zero map of stride `stride` -- an input pixel under no window gets exactly 0 and its x
    decides nothing.  At stride=1, padding='SAME' this is host_conv_backward."""
    x, w, dy = np.asarray(x, dtype), np.asarray(w, dtype), np.asarray(dy, dtype)
    N, H, W, C = x.shape
    kh, kw, _, J = w.shape
    s = stride
    Ho, Wo, pt, pl = _strided_geometry(H, W, kh, kw, s, padding)
    if dy.shape != (N, Ho, Wo, J):
        raise InvalidArgumentError(-1, 'conv_backward_strided: dy must be [N,Ho,Wo,J] = %r, got %r' % ((N, Ho, Wo, J), dy.shape))
    g, xe = dy, x
    with np.errstate(invalid='ignore'):
        if y is not None:
            g = np.where(np.asarray(y, dtype) > 0, dy, dtype(0))
        if relu_in:
            xe = np.where(x > 0, x, dtype(0))
    hs, ws = (Ho - 1) * s + 1, (Wo - 1) * s + 1               # the extent of the output map laid out at the stride
    xp = np.pad(xe, ((0, 0), (pt, max(hs - 1 + kh - H - pt, 0)), (pl, max(ws - 1 + kw - W - pl, 0)), (0, 0)))
    g2 = g.reshape(-1, J)
    dw = np.empty(w.shape, dtype)
    if with_dx:
        gz = np.zeros((N, H + kh - 1, W + kw - 1, J), dtype)
        gz[:, kh - 1 - pt:kh - 1 - pt + hs:s, kw - 1 - pl:kw - 1 - pl + ws:s] = g
        dx = np.zeros((N * H * W, C), dtype)
    for a in range(kh):
        for b in range(kw):
            dw[a, b] = np.matmul(xp[:, a:a + hs:s, b:b + ws:s].reshape(-1, C).T, g2)
            if with_dx:
                dx += np.matmul(gz[:, kh - 1 - a:kh - 1 - a + H, kw - 1 - b:kw - 1 - b + W].reshape(-1, J), w[a, b].T)
    if not with_dx:
        return None, dw, g2.sum(axis=0, dtype=dtype)
    dx = dx.reshape(x.shape)
    if relu_in:
        with np.errstate(invalid='ignore'):
            dx = np.where(x > 0, dx, dtype(0))
    return dx, dw, g2.sum(axis=0, dtype=dtype)


def conv_backward_strided_device(x, w, dy, y=None, relu_in=False, with_dx=True, stream=None, dx=None, workspace=None, stride=1,
                                 padding='SAME'):
    """conv_backward_strided with the results left on the GPU: (dx DeviceTensor [N,H,W,C] with x's ld (C for a NumPy x) or
    None, dw DeviceBuffer [kh,kw,C,J], db DeviceBuffer [J]); nothing is synchronised.  A DeviceTensor w is [kh,kw,C,J] dense.
    dx: a DeviceTensor [N,H,W,C] to write instead of a new one (with its ld); workspace: a DeviceBuffer of at least
    xdet_conv_backward_strided_workspace_bytes(N, H, W, C, J, kh, kw, stride, padding) bytes (default: allocated here) -- a
    chain of calls on one stream then allocates no activation-sized memory per call."""
    return _conv_backward_device('conv_backward_strided', x, w, dy, y, relu_in, with_dx, stream, dx, workspace, stride, padding)


def conv_backward_strided(x, w, dy, y=None, relu_in=False, with_dx=True, stream=None, stride=1, padding='SAME'):
    """host_conv_backward_strided on the GPU (xdet_conv_backward_strided): x [N,H,W,C], w [kh,kw,C,J], dy [N,Ho,Wo,J],
    y [N,Ho,Wo,J] or None as NumPy arrays or DeviceTensors (read in place with their ld) -> (dx [N,H,W,C] or None,
    dw [kh,kw,C,J], db [J]) as NumPy arrays."""
    d = conv_backward_strided_device(x, w, dy, y, relu_in, with_dx, stream, stride=stride, padding=padding)
    return _conv_results_to_host(d, w, stream)


def _conv_backward_device(who, x, w, dy, y, relu_in, with_dx, stream, dx, workspace, stride, padding):
    """The device door of both conv backwards.  `who` is the door: it names itself in every message and calls its own C entry
    points, xdet_<who> and xdet_<who>_workspace_bytes -- conv_backward's take no geometry and state the two size rules in the
    words of a single map."""
    (N, H, W, C), M, _, x_in = _operand(x, who, 'x', 4)
    (kh, kw, Cw, J), _, _, w_in = _operand(w, who, 'w', 4)
    sd, _, _, dy_in = _operand(dy, who, 'dy', 4)
    if y is not None:
        sy, _, _, y_in = _operand(y, who, 'y', 4)
    Ho, Wo, _, _ = _strided_geometry(H, W, kh, kw, stride, padding, who)
    Mo = N * Ho * Wo
    if who == 'conv_backward':
        c_geometry = ()
        expected = 'conv_backward: x [N,H,W,C], w [kh,kw,C,J], dy [N,H,W,J] and y [N,H,W,J] expected, got %r'
        sizes = ('conv_backward: N*H*W = %d, C = %d, J = %d, kernel %d x %d (sizes positive, kh and kw odd and at most 15, '
                 'C and J at most 4096, N*H*W * max(C, J) below 2^31)' % (M, C, J, kh, kw))
    else:
        c_geometry = (stride, _PADDINGS[padding])
        expected = ('%s: x [N,H,W,C], w [kh,kw,C,J], dy [N,Ho,Wo,J] and y [N,Ho,Wo,J] expected with Ho = %d, Wo = %d '
                    '(stride %d, %s), got %%r' % (who, Ho, Wo, stride, padding))
        sizes = ('%s: N*H*W = %d, N*Ho*Wo = %d, C = %d, J = %d (sizes positive, C and J at most 4096, N*H*W * C and '
                 'N*Ho*Wo * J below 2^31)' % (who, M, Mo, C, J))
    if Cw != C or sd != (N, Ho, Wo, J) or (y is not None and sy != (N, Ho, Wo, J)):
        raise InvalidArgumentError(-1, expected % ([(N, H, W, C), (kh, kw, Cw, J), sd] + ([sy] if y is not None else []),))
    _check_sizes((M,), (C,), sizes, ())
    _check_sizes((Mo,), (J,), sizes, ())
    if isinstance(w_in, DeviceTensor) and w_in.ld != J:
        raise InvalidArgumentError(-1, '%s: w must be dense on the device (ld %d, J = %d)' % (who, w_in.ld, J))
    dx = _given(dx, (N, H, W, C), who) if with_dx else None
    kx, px, ldx = _on_device(x_in, C)
    kw_, pw, _ = _on_device(w_in, J)
    kd, pd, ldd = _on_device(dy_in, J)
    ky, py, ldy = _on_device(y_in, J) if y is not None else (None, None, 0)
    d_dx = _result(dx, (N, H, W, C), ldx) if with_dx else None
    d_dw, d_db = DeviceBuffer(kh * kw * C * J * 4), DeviceBuffer(max(J * 4, 16))
    ws = workspace if workspace is not None else DeviceBuffer(
        getattr(lib(), 'xdet_%s_workspace_bytes' % who)(N, H, W, C, J, kh, kw, *c_geometry))
    check(getattr(lib(), 'xdet_' + who)(px, ldx, pw, py, ldy, pd, ldd, N, H, W, C, J, kh, kw, *c_geometry, 1 if relu_in else 0,
                                        d_dx.ptr if with_dx else None, d_dx.ld if with_dx else ldx, d_dw.ptr, d_db.ptr,
                                        ws.ptr, _handle(stream)))
    _keep_alive((d_dx, d_dw), (kx, kw_, kd, ky, ws))
    return d_dx, d_dw, d_db


def _conv_results_to_host(results, w, stream):
    """a device door's (dx or None, dw, db) as NumPy arrays, dw in w's shape"""
    d_dx, d_dw, d_db = results
    synchronize(stream)
    ws = tuple((w.shape if isinstance(w, DeviceTensor) else np.shape(w)))
    dx = d_dx.numpy(stream=stream) if d_dx is not None else None
    return dx, to_host(d_dw.ptr, ws, np.float32, stream), to_host(d_db.ptr, (ws[-1],), np.float32, stream)


# ---- batch normalisation in both directions and both modes (xdet_batch_norm_*, csrc/batchnorm.hip) ---------------------

def host_batch_norm_forward(x, gamma, beta, eps, training=True, momentum=0.997, moving_mean=None, moving_var=None, relu=False,
                            dtype=np.float32):
    """The NumPy statement of xdet_batch_norm_forward (include/xdet.h): x [..., C] (every leading axis is a row axis), gamma,
    beta, moving_mean, moving_var [C] -> (y like x, save_mean [C], save_invstd [C], new moving_mean, new moving_var).
    training: mean and the CENTRED variance sum (x - mean)^2 / M of the batch, and TensorFlow's fused update of the moving
    statistics, moving -= (moving - batch) * (1 - momentum), the variance times M / max(M - 1, 1) first (None: no update,
    None returned).  Not training: mean and var are the moving statistics, returned as they came.  dtype float32, or
    float64: the accuracy yardstick."""
    x = np.asarray(x, dtype)
    C = x.shape[-1]
    x2 = x.reshape(-1, C)
    M = x2.shape[0]
    gamma, beta = np.asarray(gamma, dtype), np.asarray(beta, dtype)
    mm = None if moving_mean is None else np.asarray(moving_mean, dtype)
    mv = None if moving_var is None else np.asarray(moving_var, dtype)
    if training:
        mean = x2.sum(axis=0, dtype=dtype) / dtype(M)
        d = x2 - mean
        var = (d * d).sum(axis=0, dtype=dtype) / dtype(M)
        if mm is not None:
            keep = dtype(1) - dtype(momentum)
            mm = mm - (mm - mean) * keep
            mv = mv - (mv - var * (dtype(M) / dtype(max(M - 1, 1)))) * keep
    else:
        if mm is None or mv is None:
            raise InvalidArgumentError(-1, 'batch_norm_forward: training=False needs the moving statistics')
        mean, var = mm, mv
    invstd = dtype(1) / np.sqrt(var + dtype(eps))
    y = ((x2 - mean) * invstd) * gamma + beta
    if relu:
        y = np.maximum(y, dtype(0))
    return y.astype(dtype).reshape(x.shape), mean, invstd.astype(dtype), mm, mv


def host_batch_norm_backward(x, y, dy, gamma, save_mean, save_invstd, training=True, dtype=np.float32, with_dx=True):
    """The NumPy statement of xdet_batch_norm_backward: x, dy [..., C], y like x the forward's output after its ReLU (None: no
    ReLU), gamma, save_mean, save_invstd [C] -> (dx like x or None, dgamma [C], dbeta [C]) with g = dy, or dy where y > 0
    and 0 elsewhere (an exact zero and a NaN in y both give 0), xhat = (x - save_mean) * save_invstd, dbeta = sum g,
    dgamma = sum g xhat, dx = gamma invstd (g - dbeta / M - xhat dgamma / M) in training mode and gamma invstd g otherwise."""
    x, dy = np.asarray(x, dtype), np.asarray(dy, dtype)
    C = x.shape[-1]
    x2, g = x.reshape(-1, C), dy.reshape(-1, C)
    M = x2.shape[0]
    gamma, mean, invstd = np.asarray(gamma, dtype), np.asarray(save_mean, dtype), np.asarray(save_invstd, dtype)
    if y is not None:
        with np.errstate(invalid='ignore'):
            g = np.where(np.asarray(y, dtype).reshape(-1, C) > 0, g, dtype(0))
    xhat = (x2 - mean) * invstd
    dbeta = g.sum(axis=0, dtype=dtype)
    dgamma = (g * xhat).sum(axis=0, dtype=dtype)
    dx = None
    if with_dx:
        if training:
            dx = (gamma * invstd) * ((g - dbeta / dtype(M)) - xhat * (dgamma / dtype(M)))
        else:
            dx = (gamma * invstd) * g
        dx = dx.astype(dtype).reshape(x.shape)
    return dx, dgamma, dbeta


def _bn_vec(a, C, what):
    """a [C] vector: a DeviceBuffer / DeviceTensor stays, anything else is copied to the device -> (keep-alive, pointer)"""
    if isinstance(a, (DeviceBuffer, DeviceTensor)):
        return a, a.ptr
    a = np.ascontiguousarray(a, np.float32).reshape(-1)
    if a.shape[0] != C:
        raise InvalidArgumentError(-1, 'batch_norm: %s must hold %d values, got %d' % (what, C, a.shape[0]))
    return _on_device(a, C)[:2]


def batch_norm_forward_device(x, gamma, beta, eps, training=True, momentum=0.997, moving_mean=None, moving_var=None,
                              relu=False, stream=None):
    """batch_norm_forward with the results left on the GPU: (y DeviceTensor with x's shape and ld (C for a NumPy x), save_mean,
    save_invstd, moving_mean, moving_var as DeviceBuffers [C]; the moving ones None when none were given); nothing is
    synchronised.  Moving statistics given as DeviceBuffers are updated in place (training) and returned; NumPy ones are
    copied to the device first."""
    shape, M, C, x_in = _operand(x, 'batch_norm', 'x', None)
    _check_sizes((M,), (C,), _BN_SIZES, ('batch_norm_forward', M, C))
    if (moving_mean is None) != (moving_var is None) or (not training and moving_mean is None):
        raise InvalidArgumentError(-1, 'batch_norm_forward: training=False needs both moving statistics; training mode takes '
                                       'both or neither')
    kx, px, ldx = _on_device(x_in, C)
    kg, pg = _bn_vec(gamma, C, 'gamma')
    kb, pb = _bn_vec(beta, C, 'beta')
    d_mm, pmm = _bn_vec(moving_mean, C, 'moving_mean') if moving_mean is not None else (None, None)
    d_mv, pmv = _bn_vec(moving_var, C, 'moving_var') if moving_var is not None else (None, None)
    d_y = _result(None, shape if len(shape) == 4 else (M, 1, 1, C), ldx)
    d_mean, d_inv = DeviceBuffer(max(C * 4, 16)), DeviceBuffer(max(C * 4, 16))
    ws = DeviceBuffer(lib().xdet_batch_norm_workspace_bytes(M, C))
    check(lib().xdet_batch_norm_forward(px, ldx, M, C, pg, pb, float(eps), 1 if training else 0, float(momentum), pmm, pmv,
                                        1 if relu else 0, d_y.ptr, d_y.ld, d_mean.ptr, d_inv.ptr, ws.ptr, _handle(stream)))
    _keep_alive((d_mean,), (kx, kg, kb, ws, d_y))
    return d_y, d_mean, d_inv, d_mm, d_mv


def batch_norm_forward(x, gamma, beta, eps, training=True, momentum=0.997, moving_mean=None, moving_var=None, relu=False,
                       stream=None):
    """host_batch_norm_forward on the GPU (xdet_batch_norm_forward): x [..., C] as a NumPy array or a DeviceTensor (read in
    place with its ld) -> (y with x's shape, save_mean, save_invstd, moving_mean, moving_var) as NumPy arrays (the moving
    ones None when none were given)."""
    d_y, d_mean, d_inv, d_mm, d_mv = batch_norm_forward_device(x, gamma, beta, eps, training, momentum, moving_mean,
                                                                moving_var, relu, stream)
    synchronize(stream)
    shape = tuple(x.shape) if isinstance(x, DeviceTensor) else np.shape(x)
    C = shape[-1]
    y = to_host(d_y.ptr, (int(np.prod(shape[:-1])), d_y.ld), np.float32, stream)[:, :C].reshape(shape)
    vec = lambda b: to_host(b.ptr, (C,), np.float32, stream) if b is not None else None
    return np.ascontiguousarray(y), vec(d_mean), vec(d_inv), vec(d_mm), vec(d_mv)


def batch_norm_backward_device(x, y, dy, gamma, save_mean, save_invstd, training=True, with_dx=True, stream=None, dx=None,
                               workspace=None):
    """batch_norm_backward with the results left on the GPU: (dx DeviceTensor with x's shape and ld (C for a NumPy x) or None,
    dgamma DeviceBuffer [C], dbeta DeviceBuffer [C]); nothing is synchronised.  dx: a DeviceTensor of x's shape to write
    instead of a new one (with its ld; it must not overlap x); workspace: a DeviceBuffer of at least
    xdet_batch_norm_workspace_bytes(M, C) bytes (default: allocated here)."""
    shape, M, C, x_in = _operand(x, 'batch_norm', 'x', None)
    sd, Md, Cd, dy_in = _operand(dy, 'batch_norm', 'dy', None)
    bad = (Md, Cd) != (M, C)
    if y is not None:
        sy, My, Cy, y_in = _operand(y, 'batch_norm', 'y', None)
        bad = bad or (My, Cy) != (M, C)
    if bad:
        raise InvalidArgumentError(-1, 'batch_norm_backward: x, dy and y of one shape expected, got %r'
                                   % ([shape, sd] + ([sy] if y is not None else []),))
    _check_sizes((M,), (C,), _BN_SIZES, ('batch_norm_backward', M, C))
    shape4 = shape if len(shape) == 4 else (M, 1, 1, C)
    dx = _given(dx, shape4, 'batch_norm_backward') if with_dx else None
    kx, px, ldx = _on_device(x_in, C)
    kd, pd, ldd = _on_device(dy_in, C)
    ky, py, ldy = _on_device(y_in, C) if y is not None else (None, None, 0)
    kg, pg = _bn_vec(gamma, C, 'gamma')
    km, pm = _bn_vec(save_mean, C, 'save_mean')
    ki, pi = _bn_vec(save_invstd, C, 'save_invstd')
    d_dx = _result(dx, shape4, ldx) if with_dx else None
    d_dg, d_db = DeviceBuffer(max(C * 4, 16)), DeviceBuffer(max(C * 4, 16))
    ws = workspace if workspace is not None else DeviceBuffer(lib().xdet_batch_norm_workspace_bytes(M, C))
    check(lib().xdet_batch_norm_backward(px, ldx, py, ldy, pd, ldd, M, C, pg, pm, pi, 1 if training else 0,
                                         d_dx.ptr if with_dx else None, d_dx.ld if with_dx else ldx, d_dg.ptr, d_db.ptr, ws.ptr,
                                         _handle(stream)))
    _keep_alive((d_dg,), (kx, kd, ky, kg, km, ki, ws))
    return d_dx, d_dg, d_db


def batch_norm_backward(x, y, dy, gamma, save_mean, save_invstd, training=True, with_dx=True, stream=None):
    """host_batch_norm_backward on the GPU (xdet_batch_norm_backward): NumPy arrays or DeviceTensors (read in place with their
    ld) -> (dx with x's shape or None, dgamma [C], dbeta [C]) as NumPy arrays."""
    d_dx, d_dg, d_db = batch_norm_backward_device(x, y, dy, gamma, save_mean, save_invstd, training, with_dx, stream)
    synchronize(stream)
    shape = tuple(x.shape) if isinstance(x, DeviceTensor) else np.shape(x)
    C = shape[-1]
    dx = None
    if d_dx is not None:
        dx = np.ascontiguousarray(to_host(d_dx.ptr, (int(np.prod(shape[:-1])), d_dx.ld), np.float32, stream)[:, :C].reshape(shape))
    return dx, to_host(d_dg.ptr, (C,), np.float32, stream), to_host(d_db.ptr, (C,), np.float32, stream)


# ---- the backward of the depthwise 3x3 conv, and the row add (xdet_depthwise_backward / xdet_add_rows,
#      csrc/depthwise_backward.hip) ------------------------------------------------------------------------------------

def host_depthwise_backward(x, k, dy, dilation=1, relu_in=False, dtype=np.float32, with_dx=True):
    """The NumPy statement of xdet_depthwise_backward (include/xdet.h) for y = depthwise3x3(xe, k), stride 1, 'SAME', NHWC:
    x, dy [N,H,W,C], k [3,3,C,1], dilation d; xe = x, or with relu_in x where x > 0 and 0 elsewhere -> (dx [N,H,W,C],
    dw [3,3,C,1]): dx[n,h,w,c] = sum over taps of dy[n, h - (a-1)d, w - (b-1)d, c] * k[a,b,c], the taps in storage order, each
    product rounded and then added (the op's own order: in float32 dx is the op's dx bit for bit, but for the sign of a
    zero), 0 wherever x > 0 is false with relu_in; dw[a,b,c] = sum over pixels of xe[n, h + (a-1)d, w + (b-1)d, c] *
    dy[n,h,w,c], NumPy's sequential sum over the pixels.  Terms outside the image are absent.  dtype float32, or float64: the
    accuracy yardstick.  with_dx=False: dx is None."""
    x, k, dy = np.asarray(x, dtype), np.asarray(k, dtype), np.asarray(dy, dtype)
    N, H, W, C = x.shape
    d = int(dilation)
    xe = x
    if relu_in:
        with np.errstate(invalid='ignore'):
            xe = np.where(x > 0, x, dtype(0))
    border = ((0, 0), (d, d), (d, d), (0, 0))
    xp, gp = np.pad(xe, border), np.pad(dy, border)
    dw = np.empty((3, 3, C, 1), dtype)
    dx = np.zeros(x.shape, dtype) if with_dx else None
    for a in range(3):
        for b in range(3):
            dw[a, b, :, 0] = (xp[:, a * d:a * d + H, b * d:b * d + W] * dy).reshape(-1, C).sum(axis=0, dtype=dtype)
            if with_dx:
                dx += gp[:, (2 - a) * d:(2 - a) * d + H, (2 - b) * d:(2 - b) * d + W] * k[a, b, :, 0]
    if with_dx and relu_in:
        with np.errstate(invalid='ignore'):
            dx = np.where(x > 0, dx, dtype(0))
    return dx, dw


def depthwise_backward_device(x, k, dy, dilation=1, relu_in=False, with_dx=True, stream=None, workspace=None, dx=None):
    """depthwise_backward with the results left on the GPU: (dx DeviceTensor [N,H,W,C] with x's ld (C for a NumPy x) or None,
    dw DeviceBuffer [3,3,C,1]); nothing is synchronised.  A DeviceTensor k is [3,3,C,1] dense (ld 1).  workspace: a
    DeviceBuffer of at least xdet_depthwise_backward_workspace_bytes(N, H, W, C) bytes (default: allocated here).  dx: a
    DeviceTensor [N,H,W,C] to write instead of a new one (with its ld; it must not overlap x or dy)."""
    who = 'depthwise_backward'
    (N, H, W, C), M, _, x_in = _operand(x, who, 'x', 4)
    sk, _, _, k_in = _operand(k, who, 'k', 4)
    sd, _, _, dy_in = _operand(dy, who, 'dy', 4)
    if sk != (3, 3, C, 1) or sd != (N, H, W, C):
        raise InvalidArgumentError(-1, 'depthwise_backward: x [N,H,W,C], k [3,3,C,1] and dy [N,H,W,C] expected, got %r'
                                   % ([(N, H, W, C), sk, sd],))
    _check_sizes((M,), (C,), 'depthwise_backward: N*H*W = %d, C = %d, dilation %r (sizes positive, C at most 4096, '
                             'N*H*W * C below 2^31, dilation 1 or 2)', (M, C, dilation), also=dilation in (1, 2))
    if isinstance(k_in, DeviceTensor) and k_in.ld != 1:
        raise InvalidArgumentError(-1, 'depthwise_backward: k must be dense on the device (ld %d)' % k_in.ld)
    dx = _given(dx, (N, H, W, C), who) if with_dx else None
    kx, px, ldx = _on_device(x_in, C)
    kk, pk, _ = _on_device(k_in, 1)
    kd, pd, ldd = _on_device(dy_in, C)
    d_dx = _result(dx, (N, H, W, C), ldx) if with_dx else None
    d_dw = DeviceBuffer(max(9 * C * 4, 16))
    ws = workspace if workspace is not None else DeviceBuffer(lib().xdet_depthwise_backward_workspace_bytes(N, H, W, C))
    check(lib().xdet_depthwise_backward(px, ldx, pk, pd, ldd, N, H, W, C, int(dilation), 1 if relu_in else 0,
                                        d_dx.ptr if with_dx else None, d_dx.ld if with_dx else ldx, d_dw.ptr, ws.ptr,
                                        _handle(stream)))
    _keep_alive((d_dx, d_dw), (kx, kk, kd, ws))
    return d_dx, d_dw


def depthwise_backward(x, k, dy, dilation=1, relu_in=False, with_dx=True, stream=None):
    """host_depthwise_backward on the GPU (xdet_depthwise_backward): x, dy [N,H,W,C] and k [3,3,C,1] as NumPy arrays or
    DeviceTensors (read in place with their ld) -> (dx [N,H,W,C] or None, dw [3,3,C,1]) as NumPy arrays."""
    d_dx, d_dw = depthwise_backward_device(x, k, dy, dilation, relu_in, with_dx, stream)
    synchronize(stream)
    C = int((x.shape if isinstance(x, DeviceTensor) else np.shape(x))[-1])
    dx = d_dx.numpy(stream=stream) if d_dx is not None else None
    return dx, to_host(d_dw.ptr, (3, 3, C, 1), np.float32, stream)


def add_rows_device(a, b, out=None, stream=None):
    """out = a + b on the GPU (xdet_add_rows): a, b DeviceTensors of one shape, each read with its own ld (NumPy arrays are
    copied to the device first, with ld channel_ld(C)); out: a DeviceTensor of that shape -- it may be a itself -- or None: a
    new one with a's ld.  -> out; nothing is synchronised."""
    sa, M, C, a_in = _operand(a, 'add_rows', 'a', 4)
    sb, _, _, b_in = _operand(b, 'add_rows', 'b', 4)
    if sa != sb or (out is not None and (not isinstance(out, DeviceTensor) or tuple(out.shape) != sa)):
        raise InvalidArgumentError(-1, 'add_rows: a, b and out of one shape expected, got %r'
                                   % ([sa, sb, getattr(out, 'shape', None)],))
    _check_sizes((M,), (C,), 'add_rows: %d rows of %d channels (positive, their product below 2^31)', (M, C), widest=None)
    ta, pa, lda = _on_device(a_in, C, padded=True)
    tb, pb, ldb = _on_device(b_in, C, padded=True)
    out = _result(out, sa, lda)
    check(lib().xdet_add_rows(pa, lda, pb, ldb, out.ptr, out.ld, M, C, _handle(stream)))
    _keep_alive((out,), (ta, tb), chain=True)
    return out


# ---- the backward of max_pooling2d(3, 2, 'same') and the stride-2 gather / scatter of a 1x1 / stride-2 projection
#      (xdet_maxpool3x3s2_backward / xdet_subsample2 / xdet_add_upsample2, csrc/pool_backward.hip) --------------------------

def _same_pad_front(n):
    """TensorFlow's 'SAME' for a 3-wide window at stride 2: (outputs, padding in front): the smaller half of the total"""
    o = -(-n // 2)
    return o, max((o - 1) * 2 + 3 - n, 0) // 2


def host_max_pool_backward(x, dy, dtype=np.float32):
    """The NumPy statement of xdet_maxpool3x3s2_backward (include/xdet.h): x [N,H,W,C], the input of
    max_pooling2d(3, 2, 'same'), dy [N,ceil(H/2),ceil(W/2),C] -> dx [N,H,W,C].  Every window sends its dy to its first maximum
    in row-major window order (strict > against the running best, which starts at the window's first in-image element; padded
    positions are absent), and the shares a pixel receives are added to 0 in ascending (oh, ow) order, each add rounded.
    dtype float32: the op's dx bit for bit; float64: the yardstick."""
    x, dy = np.asarray(x, dtype), np.asarray(dy, dtype)
    N, H, W, C = x.shape
    (Ho, pt), (Wo, pl) = _same_pad_front(H), _same_pad_front(W)
    if dy.shape != (N, Ho, Wo, C):
        raise InvalidArgumentError(-1, 'max_pool_backward: x %r needs dy %r, got %r' % (x.shape, (N, Ho, Wo, C), dy.shape))
    best = np.zeros((N, Ho, Wo, C), dtype)
    bh, bw = np.zeros((N, Ho, Wo, C), np.intp), np.zeros((N, Ho, Wo, C), np.intp)
    has = np.zeros((1, Ho, Wo, 1), bool)
    for a in range(3):
        r = 2 * np.arange(Ho) - pt + a
        rv, rc = (r >= 0) & (r < H), np.clip(r, 0, H - 1)
        for b in range(3):
            c = 2 * np.arange(Wo) - pl + b
            cv, cc = (c >= 0) & (c < W), np.clip(c, 0, W - 1)
            live = (rv[:, None] & cv[None, :])[None, :, :, None]
            v = x[:, rc][:, :, cc]
            with np.errstate(invalid='ignore'):
                take = live & (~has | (v > best))
            best = np.where(take, v, best)
            bh = np.where(take, rc[None, :, None, None], bh)
            bw = np.where(take, cc[None, None, :, None], bw)
            has = has | live
    dx = np.zeros(x.shape, dtype)
    n, c = np.arange(N)[:, None, None, None], np.arange(C)[None, None, None, :]
    # unbuffered and in the index arrays' order: for one (n, pixel, c) the windows arrive ascending in (oh, ow)
    np.add.at(dx, tuple(np.broadcast_arrays(n, bh, bw, c)), dy)
    return dx


def host_subsample2(x, dtype=np.float32):
    """x[:, ::2, ::2]: what a 1x1 / stride-2 'SAME' conv reads of x [N,H,W,C] -> [N,ceil(H/2),ceil(W/2),C]"""
    return np.ascontiguousarray(np.asarray(x, dtype)[:, ::2, ::2])


def host_add_upsample2(a, b, dtype=np.float32):
    """a [N,H,W,C] + the adjoint of host_subsample2 applied to b [N,ceil(H/2),ceil(W/2),C]: b added at the pixels whose h and
    w are both even, a unchanged (its bits) everywhere else"""
    out = np.array(a, dtype)
    b = np.asarray(b, dtype)
    if out.ndim != 4 or b.shape != out[:, ::2, ::2].shape:
        raise InvalidArgumentError(-1, 'add_upsample2: a %r needs b %r, got %r' % (out.shape, out[:, ::2, ::2].shape, b.shape))
    out[:, ::2, ::2] += b
    return out


def max_pool_backward_device(x, dy, dx=None, stream=None):
    """max_pool_backward with the result left on the GPU: dx DeviceTensor [N,H,W,C] with x's ld (channel_ld(C) for a NumPy x);
    nothing is synchronised.  x, dy: DeviceTensors read in place with their ld, or NumPy arrays, copied to the device with ld
    channel_ld(C).  dx: a DeviceTensor [N,H,W,C] to write instead of a new one (with its ld; it must not overlap x or dy)."""
    who = 'max_pool_backward'
    (N, H, W, C), _, _, x_in = _operand(x, who, 'x', 4)
    sd, _, _, dy_in = _operand(dy, who, 'dy', 4)
    if sd != (N, -(-H // 2), -(-W // 2), C):
        raise InvalidArgumentError(-1, 'max_pool_backward: x [N,H,W,C] and dy [N,ceil(H/2),ceil(W/2),C] expected, got %r'
                                   % ([(N, H, W, C), sd],))
    _check_sizes((N, H, W), (C,), _POOL_SIZES, (who, N, H, W, C))
    _given(dx, (N, H, W, C), who)
    tx, px, ldx = _on_device(x_in, C, padded=True)
    td, pd, ldd = _on_device(dy_in, C, padded=True)
    d_dx = _result(dx, (N, H, W, C), ldx)
    check(lib().xdet_maxpool3x3s2_backward(px, ldx, pd, ldd, N, H, W, C, d_dx.ptr, d_dx.ld, _handle(stream)))
    _keep_alive((d_dx,), (tx, td))
    return d_dx


def max_pool_backward(x, dy, stream=None):
    """host_max_pool_backward on the GPU (xdet_maxpool3x3s2_backward) -> dx [N,H,W,C] as a NumPy array"""
    d_dx = max_pool_backward_device(x, dy, stream=stream)
    synchronize(stream)
    return d_dx.numpy(stream=stream)


def subsample2_device(x, out=None, stream=None):
    """host_subsample2 on the GPU (xdet_subsample2): x [N,H,W,C] as a DeviceTensor read with its ld or a NumPy array (copied to
    the device with ld channel_ld(C)) -> out DeviceTensor [N,ceil(H/2),ceil(W/2),C] (a caller's, written with its ld, or a new
    one with ld channel_ld(C)); nothing is synchronised."""
    who = 'subsample2'
    (N, H, W, C), _, _, x_in = _operand(x, who, 'x', 4)
    so = (N, -(-H // 2), -(-W // 2), C)
    _given(out, so, who, 'out')
    _check_sizes((N, H, W), (C,), _POOL_SIZES, (who, N, H, W, C))
    tx, px, ldx = _on_device(x_in, C, padded=True)
    out = _result(out, so, None)
    check(lib().xdet_subsample2(px, ldx, N, H, W, C, out.ptr, out.ld, _handle(stream)))
    _keep_alive((out,), (tx,))
    return out


def add_upsample2_device(a, b, out=None, stream=None):
    """host_add_upsample2 on the GPU (xdet_add_upsample2): a [N,H,W,C], b [N,ceil(H/2),ceil(W/2),C], each read with its own ld
    (NumPy arrays are copied to the device first, with ld channel_ld(C)); out: a DeviceTensor of a's shape -- it may be a
    itself -- or None: a new one with a's ld.  -> out; nothing is synchronised."""
    who = 'add_upsample2'
    (N, H, W, C), _, _, a_in = _operand(a, who, 'a', 4)
    sb, _, _, b_in = _operand(b, who, 'b', 4)
    if sb != (N, -(-H // 2), -(-W // 2), C) or (out is not None and (not isinstance(out, DeviceTensor)
                                                                      or tuple(out.shape) != (N, H, W, C))):
        raise InvalidArgumentError(-1, 'add_upsample2: a [N,H,W,C], b [N,ceil(H/2),ceil(W/2),C] and out like a expected, got %r'
                                   % ([(N, H, W, C), sb, getattr(out, 'shape', None)],))
    _check_sizes((N, H, W), (C,), _POOL_SIZES, (who, N, H, W, C))
    ta, pa, lda = _on_device(a_in, C, padded=True)
    tb, pb, ldb = _on_device(b_in, C, padded=True)
    out = _result(out, (N, H, W, C), lda)
    check(lib().xdet_add_upsample2(pa, lda, pb, ldb, N, H, W, C, out.ptr, out.ld, _handle(stream)))
    _keep_alive((out,), (ta, tb), chain=True)
    return out


# ---- the optimizer step: tf.train.MomentumOptimizer with the reference's L2 term (xdet_momentum_step, csrc/optimizer.hip) --

def host_momentum_step(var, grad, accum, lr, momentum=0.9, weight_decay=0.0, decay=True, dtype=np.float32, scale=np.float32(1)):
    """The NumPy statement of xdet_momentum_step (include/xdet.h) for one variable: var, grad, accum of one shape ->
    (new var, new accum),

        g = grad + weight_decay * var      (decay; g = grad otherwise)
        accum = momentum * accum + g
        var = var - lr * accum

    every operation rounded on its own in `dtype`: float32 is the op's result bit for bit; float64 the yardstick.
    scale (host_clip_scale's result): xdet_momentum_step_clipped, grad * scale in grad's place, one more rounding.  The
    default 1 is exact -- x * 1 is x -- so the call without it keeps the bits of the statement above."""
    var, grad, accum = np.asarray(var, dtype), np.asarray(grad, dtype), np.asarray(accum, dtype)
    with np.errstate(invalid='ignore', over='ignore'):
        grad = grad * dtype(scale)
    g = grad + dtype(weight_decay) * var if decay else grad
    accum = dtype(momentum) * accum + g
    return var - dtype(lr) * accum, accum


def host_clip_scale(grad_sq, clip_norm):
    """The NumPy statement of the clipped step's scale (xdet_momentum_step_clipped, include/xdet.h) from the record's f32
    grad_sq -> an f32 scalar,

        norm  = sqrt(grad_sq)
        scale = clip_norm / max(norm, clip_norm)

    two operations, each correctly rounded in f32: exactly 1 wherever norm <= clip_norm, norm == clip_norm included.  A NaN
    grad_sq gives NaN (the maximum keeps a NaN norm), +inf gives 0."""
    f = np.float32
    clip = f(clip_norm)
    if not np.isfinite(clip) or clip <= 0:
        raise InvalidArgumentError(-1, 'clip_scale: clip_norm must be finite and positive, got %r' % (clip_norm,))
    with np.errstate(invalid='ignore'):
        norm = np.sqrt(f(grad_sq))
        return f(clip / (clip if norm <= clip else norm))


def host_grad_sq(grads):
    """The record's grad_sq bit for bit: the f32 sum of squares of a sequence of gradient arrays, one per slot, in the fixed
    order of include/xdet.h -- a vector's (g0^2 + g1^2) + (g2^2 + g3^2), a thread's (t0 + t1) + (t2 + t3) over its four
    vectors, the 256 threads of a chunk of 4096 elements pairwise, the chunk partials of all slots pairwise under the power
    of two at or above their count; an element beyond a slot's end is +0.  (host_grad_stats is its float64 yardstick.)"""
    f = np.float32
    partials = []
    with np.errstate(invalid='ignore', over='ignore'):
        for g in grads:
            g = np.asarray(g, f).ravel()
            chunks = -(-g.size // 4096)
            x = np.zeros(chunks * 4096, f)
            x[:g.size] = g
            x = x.reshape(chunks, 4, 256, 4)                # element j of a chunk: vector q = j / 4 = i * 256 + thread
            x = x * x
            v = (x[..., 0] + x[..., 1]) + (x[..., 2] + x[..., 3])
            s = (v[:, 0] + v[:, 1]) + (v[:, 2] + v[:, 3])
            w = 128
            while w >= 1:
                s = s[:, :w] + s[:, w:2 * w]
                w >>= 1
            partials.append(s[:, 0])
        p = np.concatenate(partials)
        n, P = p.size, 1
        while P < n:
            P <<= 1
        w = P >> 1
        while w >= 1:
            m = max(0, min(w, n - w))                       # i < w with i + w < n
            p[:m] = p[:m] + p[w:w + m]
            w >>= 1
    return f(p[0])


def _device_array(a, n, who, what, null=True):
    """one array of a table door named `who`: a dense DeviceTensor of n elements or a DeviceBuffer of at least n floats -> pointer
    (null=False: the door itself names a NULL pointer)"""
    if isinstance(a, DeviceTensor):
        if a.ld != a.shape[-1] or math.prod(a.shape) != n:
            raise InvalidArgumentError(-1, '%s: %s must be dense and hold %d elements, got shape %r with ld %d' % (who, what, n, a.shape, a.ld))
    elif not isinstance(a, DeviceBuffer):
        raise InvalidArgumentError(-1, '%s: %s must be a DeviceTensor or a DeviceBuffer (device memory), got %s' % (who, what, type(a).__name__))
    elif a.nbytes < 4 * n:
        raise InvalidArgumentError(-1, '%s: %s holds %d bytes, %d elements need %d' % (who, what, a.nbytes, n, 4 * n))
    if null and not a.ptr:
        raise InvalidArgumentError(-1, '%s: %s is a NULL pointer' % (who, what))
    return a.ptr


def _momentum_table(slots, who):
    """the xdet_momentum_slot table of a sequence of (var, grad, accum, n, decay) -> (table, the slots as a list)"""
    slots = list(slots)
    if not slots:
        raise InvalidArgumentError(-1, '%s: an empty slot table' % who)
    table = (MomentumSlot * len(slots))()
    for i, slot in enumerate(slots):
        if len(slot) != 5:
            raise InvalidArgumentError(-1, '%s: slot %d must be (var, grad, accum, n, decay)' % (who, i))
        var, grad, accum, n, decay = slot
        n = int(n)
        _check_sizes((n,), (1,), who + ': slot %d holds n = %d elements (positive, below 2^31)', (i, n), widest=None)
        ptrs = [_device_array(a, n, who, 'slot %d\'s %s' % (i, what)) for a, what in ((var, 'var'), (grad, 'grad'), (accum, 'accum'))]
        table[i] = MomentumSlot(ptrs[0], ptrs[1], ptrs[2], n, 1 if decay else 0)
    return table, slots


def _table_workspace(workspace, need, who):
    if workspace is not None and (not isinstance(workspace, DeviceBuffer) or workspace.nbytes < need):
        raise InvalidArgumentError(-1, '%s: workspace must be a DeviceBuffer of at least %d bytes' % (who, need))
    return workspace if workspace is not None else DeviceBuffer(need)


def momentum_step_device(slots, lr, momentum=0.9, weight_decay=0.0, l2=False, stream=None, workspace=None, skip=None, l2_out=None,
                         clip=None, scale_out=None):
    """host_momentum_step over a table of variables in one launch (xdet_momentum_step): slots is a sequence of (var, grad, accum,
    n, decay) with var, grad, accum dense DeviceTensors of n elements or DeviceBuffers of at least n floats; var and accum are
    updated in place.  l2=True: -> a DeviceBuffer holding one float, sum over the decayed slots of sum var^2 / 2 on the values
    before the update, summed in the fixed order include/xdet.h documents (None otherwise); l2_out: the caller's buffer for it,
    at least 4 bytes.  workspace: a DeviceBuffer of at least xdet_momentum_step_workspace_bytes bytes (default: allocated
    here).  skip (the record grad_stats_device left, a DeviceBuffer of at least 8 bytes; default None: the plain call): the
    guarded step, xdet_momentum_step_guarded on the record's `nonfinite` word -- where that word is not zero no var and no
    accum byte changes, and l2 is written all the same.
    clip=(stats, clip_norm) (stats: the record grad_stats_device left on the same stream, a DeviceBuffer of at least 16 bytes;
    default None: the calls above): the clipped step, xdet_momentum_step_clipped -- every gradient times host_clip_scale(the
    record's grad_sq, clip_norm), host_momentum_step(..., scale=); guarded by the same record where skip is given (skip must
    then be `stats` itself).  scale_out: the caller's DeviceBuffer of at least 4 bytes that receives the scale (goes with
    clip).  Without the guard a grad_sq that is not finite gives NaN weights (include/xdet.h says which).
    Nothing is synchronised."""
    table, slots = _momentum_table(slots, 'momentum_step')
    if skip is not None and (not isinstance(skip, DeviceBuffer) or skip.nbytes < 8 or not skip.ptr):
        raise InvalidArgumentError(-1, 'momentum_step: skip must be the record of grad_stats_device, a DeviceBuffer of at least 8 bytes')
    if l2_out is not None and (not l2 or not isinstance(l2_out, DeviceBuffer) or l2_out.nbytes < 4 or not l2_out.ptr):
        raise InvalidArgumentError(-1, 'momentum_step: l2_out goes with l2=True and must be a DeviceBuffer of at least 4 bytes')
    if scale_out is not None and (clip is None or not isinstance(scale_out, DeviceBuffer) or scale_out.nbytes < 4 or not scale_out.ptr):
        raise InvalidArgumentError(-1, 'momentum_step: scale_out goes with clip= and must be a DeviceBuffer of at least 4 bytes')
    if clip is not None:
        if not isinstance(clip, (tuple, list)) or len(clip) != 2 or not isinstance(clip[0], DeviceBuffer) or clip[0].nbytes < 16:
            raise InvalidArgumentError(-1, 'momentum_step: clip must be (the record of grad_stats_device, a DeviceBuffer of at least '
                                           '16 bytes, clip_norm)')
        if skip is not None and skip is not clip[0]:
            raise InvalidArgumentError(-1, 'momentum_step: with clip=, skip must be the same record (one record decides both)')
    ws = _table_workspace(workspace, lib().xdet_momentum_step_workspace_bytes(table, len(slots)), 'momentum_step')
    d_l2 = (l2_out if l2_out is not None else DeviceBuffer(16)) if l2 else None
    if clip is not None:
        stats, clip_norm = clip
        # (a NULL stats_dev and a clip_norm that is not finite or <= 0 are the C door's refusals, ahead of any launch)
        check(lib().xdet_momentum_step_clipped(table, len(slots), float(lr), float(momentum), float(weight_decay),
                                               d_l2.ptr if l2 else None, stats.ptr or None, float(clip_norm), 1 if skip is not None else 0,
                                               scale_out.ptr if scale_out is not None else None, ws.ptr, _handle(stream)))
        _keep_alive((d_l2 if l2 else scale_out,), (ws, stats, scale_out) + tuple(a for s in slots for a in s[:3]))
        return d_l2
    if skip is None:
        check(lib().xdet_momentum_step(table, len(slots), float(lr), float(momentum), float(weight_decay),
                                       d_l2.ptr if l2 else None, ws.ptr, _handle(stream)))
    else:
        check(lib().xdet_momentum_step_guarded(table, len(slots), float(lr), float(momentum), float(weight_decay),
                                               d_l2.ptr if l2 else None, skip.ptr + 4, ws.ptr, _handle(stream)))
    _keep_alive((d_l2,), (ws, skip) + tuple(a for s in slots for a in s[:3]))
    return d_l2


# ---- the guard of the step: sum of squares and non-finite count of a table's gradients (xdet_grad_stats, csrc/optimizer.hip) --

def host_grad_stats(grads):
    """The NumPy statement of xdet_grad_stats (include/xdet.h) over a sequence of gradient arrays, one per slot -> (grad_sq,
    nonfinite, first_bad): the float64 sum of squares of every element (the yardstick of the record's f32 grad_sq: NaN or inf
    where the record's is), the number of elements that are NaN, +inf or -inf, and the lowest index of an array that holds
    one, -1 if none does."""
    grad_sq, nonfinite, first_bad = np.float64(0), 0, -1
    for i, g in enumerate(grads):
        g = np.asarray(g, np.float64).ravel()
        with np.errstate(over='ignore', invalid='ignore'):
            grad_sq = grad_sq + np.square(g).sum()
        bad = int(np.count_nonzero(~np.isfinite(g)))
        nonfinite += bad
        if bad and first_bad < 0:
            first_bad = i
    return float(grad_sq), nonfinite, first_bad


GRAD_STATS_DTYPE = np.dtype([('grad_sq', np.float32), ('nonfinite', np.int32), ('first_bad_slot', np.int32), ('zero', np.int32)])


def grad_stats_device(slots, stream=None, workspace=None, out=None):
    """xdet_grad_stats over the gradients of a momentum_step_device table (the same 5-tuples; var and accum are checked as
    there and not read) -> a DeviceBuffer that holds the 16-byte record {f32 grad_sq, i32 nonfinite, i32 first_bad_slot, i32 0}
    (GRAD_STATS_DTYPE; what momentum_step_device takes as skip=).  out: the caller's DeviceBuffer of at least 16 bytes;
    workspace: one of at least xdet_grad_stats_workspace_bytes bytes (defaults: allocated here).  Nothing is synchronised."""
    table, slots = _momentum_table(slots, 'grad_stats')
    if out is not None and (not isinstance(out, DeviceBuffer) or out.nbytes < 16 or not out.ptr):
        raise InvalidArgumentError(-1, 'grad_stats: out must be a DeviceBuffer of at least 16 bytes')
    ws = _table_workspace(workspace, lib().xdet_grad_stats_workspace_bytes(table, len(slots)), 'grad_stats')
    rec = out if out is not None else DeviceBuffer(16)
    check(lib().xdet_grad_stats(table, len(slots), rec.ptr, ws.ptr, _handle(stream)))
    _keep_alive((rec,), (ws,) + tuple(s[1] for s in slots))
    return rec


# ---- the refresh of forward layers from weights on the device (xdet_bn_fold, xdet_layers_refresh_device, csrc/conv_repack.hip) --

def host_bn_fold(gamma, beta, moving_mean, moving_variance, eps, bias=None, dtype=np.float32):
    """The NumPy statement of xdet_bn_fold (include/xdet.h), the inference fold of a batch norm -> (scale, shift),

        scale = gamma / sqrt(moving_variance + eps)
        shift = (beta - moving_mean * scale) + (bias * scale if bias is given else 0)

    every operation rounded on its own in `dtype`: float32 is the op's result bit for bit (the + 0 of a fold without bias turns a
    -0 shift into +0); float64 the yardstick."""
    g, b, m, v = (np.asarray(a, dtype) for a in (gamma, beta, moving_mean, moving_variance))
    with np.errstate(divide='ignore', invalid='ignore'):
        sc = g / np.sqrt(v + dtype(eps))
    return sc, (b - m * sc) + (np.asarray(bias, dtype) * sc if bias is not None else dtype(0))


def bn_fold_device(gamma, beta, moving_mean, moving_variance, eps, bias=None, C=None, stream=None):
    """host_bn_fold on the device (xdet_bn_fold): four (five) device arrays of C floats (DeviceBuffers or dense DeviceTensors
    whose last axis is C; C=: the count, where a buffer is larger than its array) -> (scale, shift) as DeviceBuffers of C floats.
    Nothing is synchronised."""
    arrs = [gamma, beta, moving_mean, moving_variance] + ([bias] if bias is not None else [])
    if not all(isinstance(a, (DeviceBuffer, DeviceTensor)) for a in arrs):
        raise InvalidArgumentError(-1, 'bn_fold: the arrays must be DeviceBuffers or DeviceTensors (device memory)')
    C = int(C) if C is not None else (int(gamma.shape[-1]) if isinstance(gamma, DeviceTensor) else gamma.nbytes // 4)
    if C <= 0 or any(isinstance(a, DeviceBuffer) and a.nbytes < 4 * C for a in arrs):
        raise InvalidArgumentError(-1, 'bn_fold: every array must hold C = %d floats' % C)
    sc, sh = DeviceBuffer(4 * C), DeviceBuffer(4 * C)
    check(lib().xdet_bn_fold(gamma.ptr, beta.ptr, moving_mean.ptr, moving_variance.ptr, bias.ptr if bias is not None else None,
                             float(eps), C, sc.ptr, sh.ptr, _handle(stream)))
    _keep_alive((sc, sh), tuple(arrs))
    return sc, sh


def refresh_layers_table(slots):
    """the argument checks of refresh_layers_device, without touching the GPU -> (the xdet_layer_refresh table, the objects it
    points to): what a caller sizes a workspace from (xdet_layers_refresh_workspace_bytes) ahead of the calls"""
    slots = list(slots)
    if not slots:
        raise InvalidArgumentError(-1, 'refresh_layers: an empty slot table')
    table, arrays = (LayerRefresh * len(slots))(), []
    for i, slot in enumerate(slots):
        slot = tuple(slot) + (None,) * (4 - len(slot)) if 2 <= len(slot) <= 4 else ()
        if not slot:
            raise InvalidArgumentError(-1, 'refresh_layers: slot %d must be (layer, kernel[, scale[, shift]])' % i)
        layer, kernel, scale, shift = slot
        if hasattr(layer, 'taps') and hasattr(layer, 'handle'):       # a SpectralConv: the library refuses it by name of the reason
            n, co = layer.taps * layer.cin * layer.cout, layer.cout
        elif hasattr(layer, 'kh') and hasattr(layer, 'handle'):
            n, co = layer.kh * layer.kw * layer.cin * layer.cout, layer.cout
        elif hasattr(layer, 'C') and hasattr(layer, 'handle'):
            n, co = 9 * layer.C, 0
            if scale is not None or shift is not None:
                raise InvalidArgumentError(-1, 'refresh_layers: slot %d is a depthwise layer: it takes no scale and no shift' % i)
        else:
            raise InvalidArgumentError(-1, 'refresh_layers: slot %d\'s layer must be a Conv2D or a DepthwiseConv2D (a layer object of xdet.ops), got %s'
                                       % (i, type(layer).__name__))
        ptrs = [_device_array(a, m, 'refresh_layers', 'slot %d\'s %s' % (i, what), null=False) if a is not None else None
                for a, m, what in ((kernel, n, 'kernel'), (scale, co, 'scale'), (shift, co, 'shift'))]
        if not ptrs[0]:
            raise InvalidArgumentError(-1, 'refresh_layers: slot %d has no kernel' % i)
        table[i] = LayerRefresh(layer.handle, ptrs[0], ptrs[1], ptrs[2])
        arrays += [a for a in (layer, kernel, scale, shift) if a is not None]
    return table, arrays


def refresh_layers_device(slots, stream=None, workspace=None):
    """Conv2D.set_kernel_device / DepthwiseConv2D.set_kernel_device over a table of layers in a number of launches that does not
    depend on its length (xdet_layers_refresh_device): slots is a sequence of (layer, kernel[, scale[, shift]]) with layer a
    Conv2D or a DepthwiseConv2D, kernel a dense DeviceTensor in the layer's kernel shape (or a DeviceBuffer of that many floats),
    scale / shift (Conv2D only) device arrays of cout floats or None (kept).  Every layer then holds what a layer created from
    the same values would hold, bit for bit.  workspace: a DeviceBuffer of at least xdet_layers_refresh_workspace_bytes bytes
    (default: allocated here and released on return, which waits for the device: pass one to keep the call asynchronous).  With a
    workspace nothing is synchronised, and the caller keeps the workspace and the arrays alive until the stream has run the call.
    The library refuses, by name of the reason, a layer listed twice, a grouped or spectral layer and a layer whose planes copy
    carries a folded batch norm."""
    table, arrays = refresh_layers_table(slots)
    need = lib().xdet_layers_refresh_workspace_bytes(table, len(table))
    if workspace is not None and (not isinstance(workspace, DeviceBuffer) or workspace.nbytes < need):
        raise InvalidArgumentError(-1, 'refresh_layers: workspace must be a DeviceBuffer of at least %d bytes' % need)
    if not need:
        check(lib().xdet_layers_refresh_device(table, len(table), None, _handle(stream)))     # (the library names the reason)
    ws = workspace if workspace is not None else DeviceBuffer(need)
    check(lib().xdet_layers_refresh_device(table, len(table), ws.ptr, _handle(stream)))


# ---- the pack op: dense tensors side by side in a merged one, and back (xdet_tensors_concat / _split, csrc/weight_pack.hip) ----

def host_concat(parts, outer):
    """The NumPy statement of xdet_tensors_concat (include/xdet.h) for one slot: every part, an array of outer * width_p elements
    in any shape, is read as [outer, width_p] -> merged [outer, sum of widths], merged[o, off_p : off_p + width_p] =
    part_p[o, :].  A copy: the bits pass through."""
    outer = int(outer)
    parts = [np.ascontiguousarray(p) for p in parts]
    if outer <= 0 or not 1 <= len(parts) <= 4 or any(p.size == 0 or p.size % outer for p in parts):
        raise InvalidArgumentError(-1, 'tensors_concat: 1 to 4 parts of outer * width elements each, width positive, got outer = %d '
                                       'and sizes %r' % (outer, [p.size for p in parts]))
    return np.ascontiguousarray(np.concatenate([p.reshape(outer, -1) for p in parts], axis=1))


def host_split(merged, outer, widths):
    """The NumPy statement of xdet_tensors_split for one slot: merged, an array of outer * sum(widths) elements in any shape ->
    a list of the parts as [outer, width_p] arrays, part_p[o, :] = merged[o, off_p : off_p + width_p]"""
    outer, widths = int(outer), [int(w) for w in widths]
    m = np.ascontiguousarray(merged)
    if outer <= 0 or not 1 <= len(widths) <= 4 or min(widths) <= 0 or m.size != outer * sum(widths):
        raise InvalidArgumentError(-1, 'tensors_split: merged must hold outer * sum(widths) elements for 1 to 4 positive widths, got '
                                       '%d elements, outer = %d, widths %r' % (m.size, outer, widths))
    m = m.reshape(outer, sum(widths))
    offs = np.cumsum([0] + widths)
    return [np.ascontiguousarray(m[:, a:b]) for a, b in zip(offs[:-1], offs[1:])]


def _pack_table(slots, who):
    """the argument checks of concat_device / split_device, without touching the GPU -> (the xdet_pack_slot table, the arrays it
    points to)"""
    slots = list(slots)
    if not slots:
        raise InvalidArgumentError(-1, '%s: an empty slot table' % who)
    table, arrays = (PackSlot * len(slots))(), []
    for i, slot in enumerate(slots):
        if len(slot) != 3:
            raise InvalidArgumentError(-1, '%s: slot %d must be (merged, outer, [(part, width), ...])' % (who, i))
        merged, outer, parts = slot
        parts = [tuple(p) for p in parts]
        if isinstance(outer, bool) or not isinstance(outer, (int, np.integer)) or outer <= 0:
            raise InvalidArgumentError(-1, '%s: slot %d has outer = %r (a positive integer)' % (who, i, outer))
        if not 1 <= len(parts) <= 4 or any(len(p) != 2 for p in parts):
            raise InvalidArgumentError(-1, '%s: slot %d must have 1 to 4 (part, width) pairs, got %d' % (who, i, len(parts)))
        widths = [int(w) for _, w in parts]
        if min(widths) <= 0 or int(outer) * sum(widths) >= 2 ** 31:
            raise InvalidArgumentError(-1, '%s: slot %d has widths %r at outer = %d (positive, outer * their sum below 2^31)'
                                       % (who, i, widths, outer))
        s = PackSlot()
        s.merged, s.outer, s.n_parts = _device_array(merged, int(outer) * sum(widths), who, 'slot %d\'s merged tensor' % i), int(outer), len(parts)
        for p, (a, w) in enumerate(parts):
            s.part[p], s.width[p] = _device_array(a, int(outer) * int(w), who, 'slot %d\'s part %d' % (i, p)), int(w)
        table[i] = s
        arrays += [merged] + [a for a, _ in parts]
    return table, arrays


def _pack_device(slots, who, sizer, door, stream, workspace):
    table, arrays = _pack_table(slots, who)
    need = sizer(table, len(table))
    if workspace is not None and (not isinstance(workspace, DeviceBuffer) or workspace.nbytes < need):
        raise InvalidArgumentError(-1, '%s: workspace must be a DeviceBuffer of at least %d bytes' % (who, need))
    ws = workspace if workspace is not None else DeviceBuffer(need)
    check(door(table, len(table), ws.ptr, _handle(stream)))
    _keep_alive(arrays[:1], (ws,) + tuple(arrays), chain=True)


def concat_device(slots, stream=None, workspace=None):
    """host_concat over a table of slots in one launch (xdet_tensors_concat): slots is a sequence of (merged, outer, [(part,
    width), ...]) with merged and the 1 to 4 parts dense DeviceTensors of exactly outer * W and outer * width elements (any
    shape) or DeviceBuffers of at least that many floats; merged[o, off_p : off_p + width_p] = part_p[o, :].  workspace: a
    DeviceBuffer of at least xdet_tensors_concat_workspace_bytes bytes (default: allocated here).  Nothing is synchronised."""
    l = lib()
    _pack_device(slots, 'tensors_concat', l.xdet_tensors_concat_workspace_bytes, l.xdet_tensors_concat, stream, workspace)


def split_device(slots, stream=None, workspace=None):
    """host_split over a table of slots in one launch (xdet_tensors_split): the slots of concat_device, copied the other way,
    part_p[o, :] = merged[o, off_p : off_p + width_p].  Two slots may read one merged tensor."""
    l = lib()
    _pack_device(slots, 'tensors_split', l.xdet_tensors_split_workspace_bytes, l.xdet_tensors_split, stream, workspace)


# ---- the checkpoint op (xdet_crc32c, csrc/crc32c.hip): checksum, and optionally copy, a table of device buffers ---------------

def _crc_span(a, who, what):
    """one buffer of the crc32c doors -> (pointer, bytes, the object to keep alive): a DeviceBuffer (all of it), a dense
    DeviceTensor (its elements), or (pointer-like, bytes) -- an integer address, a DeviceBuffer or a DeviceTensor and the bytes
    to take from there"""
    if isinstance(a, DeviceBuffer):
        return a.ptr or 0, int(a.nbytes), a
    if isinstance(a, DeviceTensor):
        if a.ld != a.shape[-1]:
            raise InvalidArgumentError(-1, '%s: %s must be dense, got shape %r with ld %d' % (who, what, a.shape, a.ld))
        return a.ptr, 4 * math.prod(a.shape), a
    if isinstance(a, (tuple, list)) and len(a) == 2:
        at, n = a
        ptr = at.ptr if isinstance(at, (DeviceBuffer, DeviceTensor)) else at
        if ptr is not None and (isinstance(ptr, bool) or not isinstance(ptr, (int, np.integer))):
            raise InvalidArgumentError(-1, '%s: %s has a pointer of type %s' % (who, what, type(ptr).__name__))
        if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or n < 0:
            raise InvalidArgumentError(-1, '%s: %s has bytes = %r (a non-negative integer)' % (who, what, n))
        return int(ptr or 0), int(n), at
    raise InvalidArgumentError(-1, '%s: %s must be a DeviceBuffer, a dense DeviceTensor or (pointer, bytes), got %s'
                               % (who, what, type(a).__name__))


def crc32c_table(buffers, copy_to=None, who='crc32c'):
    """the argument checks of the crc32c doors, without touching the GPU -> (the xdet_crc_slot table, the objects it points to).
    buffers: a sequence of DeviceBuffer / dense DeviceTensor / (pointer, bytes); copy_to: None, or one destination per buffer
    -- None (checksum only), a pointer, a DeviceBuffer or a DeviceTensor that holds at least the buffer's bytes."""
    buffers = list(buffers)
    if not buffers:
        raise InvalidArgumentError(-1, '%s: an empty slot table' % who)
    if len(buffers) > 65536:
        raise InvalidArgumentError(-1, '%s: at most 65536 slots, got %d' % (who, len(buffers)))
    dsts = list(copy_to) if copy_to is not None else [None] * len(buffers)
    if len(dsts) != len(buffers):
        raise InvalidArgumentError(-1, '%s: copy_to names %d destinations for %d buffers' % (who, len(dsts), len(buffers)))
    table, keep = (CrcSlot * len(buffers))(), []
    for i, (a, d) in enumerate(zip(buffers, dsts)):
        ptr, n, obj = _crc_span(a, who, 'buffer %d' % i)
        if n and not ptr:
            raise InvalidArgumentError(-1, '%s: buffer %d is a NULL pointer with %d bytes' % (who, i, n))
        dptr = 0
        if d is not None:
            if isinstance(d, DeviceBuffer):
                dptr, room = d.ptr or 0, d.nbytes
            elif isinstance(d, DeviceTensor):
                dptr, room = d.ptr, 4 * math.prod(d.shape[:-1]) * d.ld
            else:
                dptr, room = int(d), n
            if room < n:
                raise InvalidArgumentError(-1, '%s: destination %d holds %d bytes, the buffer %d' % (who, i, room, n))
        if (ptr | dptr) & 3:
            raise InvalidArgumentError(-1, '%s: slot %d: src and dst must be 4-byte aligned' % (who, i))
        table[i] = CrcSlot(ptr or None, dptr or None, n)
        keep += [obj, d]
    return table, keep


def crc32c_launch(table, out, stream=None, workspace=None, keep=()):
    """xdet_crc32c over a table of crc32c_table: the CRCs go to `out`, a DeviceBuffer of at least 4 bytes per slot (or a device
    address); workspace: a DeviceBuffer of at least xdet_crc32c_workspace_bytes bytes (default: allocated here).  Two launches
    whatever the table; nothing is synchronised.  -> the workspace used"""
    need = lib().xdet_crc32c_workspace_bytes(table, len(table))
    if not need:
        raise InvalidArgumentError(-1, 'crc32c: the table is beyond the limits (65536 slots, 2^22 chunks of 32 KiB)')
    if isinstance(out, DeviceBuffer) and out.nbytes < 4 * len(table):
        raise InvalidArgumentError(-1, 'crc32c: out holds %d bytes, %d slots need %d' % (out.nbytes, len(table), 4 * len(table)))
    ws = _table_workspace(workspace, need, 'crc32c')
    check(lib().xdet_crc32c(table, len(table), out.ptr if isinstance(out, DeviceBuffer) else int(out), ws.ptr, _handle(stream)))
    if isinstance(out, DeviceBuffer):
        out._keep = (ws,) + tuple(keep)
    return ws


def crc32c_device(buffers, copy_to=None, stream=None):
    """The CRC-32C of every buffer of a table of device buffers, computed where they lie (xdet_crc32c) -> np.uint32[n], each
    equal to xdet.tf_checkpoint.crc32c of the buffer's bytes (unmasked; an empty buffer gives 0).  copy_to: one destination
    per buffer (None: none) that receives the buffer's bytes in the same pass, bit for bit.  The call reads the n words back,
    so it synchronises `stream`; crc32c_table / crc32c_launch are the halves that do not."""
    table, keep = crc32c_table(buffers, copy_to)
    out = DeviceBuffer(4 * len(table))
    crc32c_launch(table, out, stream=stream, keep=keep)
    got = to_host(out.ptr, (len(table),), np.uint32, stream)
    out._keep = None
    return got


# ---- the gradient average of data-parallel training (xdet_grad_pack / xdet_grad_reduce_ranks, csrc/grad_average.hip; the
# ---- exchange is xdet.dist.Communicator.average_gradients) --------------------------------------------------------------------

GRAD_CHUNK_MAX = 1 << 24          # elements of a chunk at most: 64 MiB of f32, what one collective moves per rank


def host_average_gradients(per_rank, dtype=np.float32):
    """The NumPy statement of the gradient average (include/xdet.h): per_rank[r][i] is gradient i of rank r -> a list with,
    per gradient,

        s = g[0];  for r = 1 .. world-1:  s = s + g[r];   out = s / world

    every operation rounded on its own in `dtype`: float32 is what every rank holds after
    Communicator.average_gradients, bit for bit; float64 the yardstick.  Refused: no ranks, no gradients, ranks whose counts
    or shapes differ."""
    per_rank = [[np.asarray(g, dtype) for g in grads] for grads in per_rank]
    if not per_rank or not per_rank[0]:
        raise InvalidArgumentError(-1, 'grad_average: needs at least one rank with at least one gradient')
    for r, grads in enumerate(per_rank):
        if len(grads) != len(per_rank[0]):
            raise InvalidArgumentError(-1, 'grad_average: rank %d holds %d gradients, rank 0 holds %d' % (r, len(grads), len(per_rank[0])))
        for i, (g, g0) in enumerate(zip(grads, per_rank[0])):
            if g.shape != g0.shape:
                raise InvalidArgumentError(-1, 'grad_average: gradient %d has shape %r on rank %d and %r on rank 0' % (i, g.shape, r, g0.shape))
    world = dtype(len(per_rank))
    out = []
    with np.errstate(all='ignore'):
        for i in range(len(per_rank[0])):
            s = per_rank[0][i]
            for grads in per_rank[1:]:
                s = s + grads[i]
            out.append(s / world)
    return out


def grad_flat_offsets(sizes):
    """The flat element space of the gradient average (include/xdet.h) for slots of `sizes` elements -> (offsets, T): slot i
    occupies [offsets[i], offsets[i] + sizes[i]), every slot starts on a multiple of 4, T is the padded total."""
    offsets, at = [], 0
    for n in sizes:
        offsets.append(at)
        at += (int(n) + 3) // 4 * 4
    return offsets, at


def _grad_size(a, i):
    """gradient i of a table: a dense DeviceTensor or a DeviceBuffer of whole floats -> its element count"""
    if isinstance(a, DeviceTensor):
        n = math.prod(a.shape)
        if a.ld != a.shape[-1] or n <= 0:
            raise InvalidArgumentError(-1, 'grad_average: gradient %d must be dense and hold elements, got shape %r with ld %d' % (i, a.shape, a.ld))
    elif isinstance(a, DeviceBuffer):
        n = a.nbytes // 4
        if a.nbytes % 4 or n <= 0:
            raise InvalidArgumentError(-1, 'grad_average: gradient %d holds %d bytes, not a positive count of floats' % (i, a.nbytes))
    else:
        raise InvalidArgumentError(-1, 'grad_average: gradient %d must be a DeviceTensor or a DeviceBuffer (device memory), got %s'
                                   % (i, type(a).__name__))
    if not a.ptr:
        raise InvalidArgumentError(-1, 'grad_average: gradient %d is a NULL pointer' % i)
    return n


def _grad_table(tensors, chunk_elems):
    """the checks every door of the gradient average makes ahead of any device work -> (the gradients as a list, xdet_grad_slot table, sizes, T)"""
    try:
        tensors = list(tensors)
    except TypeError:
        tensors = None
    if not tensors:
        raise InvalidArgumentError(-1, 'grad_average: needs a non-empty sequence of gradients')
    if len(tensors) > 65536:
        raise InvalidArgumentError(-1, 'grad_average: at most 65536 gradients, got %d' % len(tensors))
    if isinstance(chunk_elems, bool) or not isinstance(chunk_elems, (int, np.integer)) or chunk_elems <= 0 or chunk_elems % 1024 \
            or chunk_elems > GRAD_CHUNK_MAX:
        raise InvalidArgumentError(-1, 'grad_average: chunk_elems must be a positive multiple of 1024, at most 2^24 (64 MiB of f32), '
                                       'got %r' % (chunk_elems,))
    sizes = tuple(_grad_size(a, i) for i, a in enumerate(tensors))
    table = (GradSlot * len(tensors))()
    for i, (a, n) in enumerate(zip(tensors, sizes)):
        table[i] = GradSlot(a.ptr, n)
    return tensors, table, sizes, grad_flat_offsets(sizes)[1]


def _grad_chunk(chunk, chunk_elems, total):
    """-> the length of chunk `chunk`"""
    n_chunks = -(-total // chunk_elems)
    if isinstance(chunk, bool) or not isinstance(chunk, (int, np.integer)) or not 0 <= chunk < n_chunks:
        raise InvalidArgumentError(-1, 'grad_average: chunk %r is outside the %d chunks of %d elements' % (chunk, n_chunks, chunk_elems))
    return min(chunk_elems, total - chunk * chunk_elems)


def _grad_span(buf, what, offset_elems, need_elems):
    """a caller's chunk buffer: a DeviceBuffer that holds need_elems floats from a 16-byte aligned offset -> pointer"""
    if not isinstance(buf, DeviceBuffer) or isinstance(offset_elems, bool) or not isinstance(offset_elems, (int, np.integer)) \
            or offset_elems < 0 or offset_elems % 4 or buf.nbytes < 4 * (offset_elems + need_elems) or not buf.ptr or buf.ptr % 16:
        raise InvalidArgumentError(-1, 'grad_average: %s must be a 16-byte aligned DeviceBuffer of at least %d floats behind an '
                                       'offset that is a multiple of 4 elements' % (what, need_elems))
    return buf.ptr + 4 * offset_elems


def _grad_workspace(workspace, table, n, world, chunk_elems):
    need = lib().xdet_grad_average_workspace_bytes(table, n, world, chunk_elems)
    if workspace is not None and (not isinstance(workspace, DeviceBuffer) or workspace.nbytes < need):
        raise InvalidArgumentError(-1, 'grad_average: workspace must be a DeviceBuffer of at least %d bytes' % need)
    return workspace if workspace is not None else DeviceBuffer(need)


def grad_pack_device(tensors, chunk, chunk_elems, flat_out=None, offset_elems=0, stream=None, workspace=None):
    """Chunk `chunk` of the flat element space of `tensors` (dense DeviceTensors or DeviceBuffers; xdet_grad_pack) -> flat_out, a
    DeviceBuffer that holds the chunk's length in floats from element `offset_elems` on (default: allocated here), padding
    elements +0.  workspace: a DeviceBuffer of at least xdet_grad_average_workspace_bytes(table, 1, chunk_elems) bytes
    (default: allocated here).  Nothing is synchronised."""
    tensors, table, sizes, total = _grad_table(tensors, chunk_elems)
    length = _grad_chunk(chunk, chunk_elems, total)
    if workspace is not None and not isinstance(workspace, DeviceBuffer):
        raise InvalidArgumentError(-1, 'grad_average: workspace must be a DeviceBuffer')
    ptr = _grad_span(flat_out, 'flat_out', offset_elems, length) if flat_out is not None else None
    ws = _grad_workspace(workspace, table, len(sizes), 1, chunk_elems)
    if flat_out is None:
        flat_out = DeviceBuffer(4 * length)
        ptr = flat_out.ptr
    check(lib().xdet_grad_pack(table, len(sizes), int(chunk), int(chunk_elems), ptr, ws.ptr, _handle(stream)))
    _keep_alive((flat_out,), (ws,) + tuple(tensors))
    return flat_out


def grad_reduce_ranks_device(tensors, chunk, chunk_elems, gathered, world, stream=None, workspace=None):
    """The rank-ordered mean of chunk `chunk` (xdet_grad_reduce_ranks): gathered is a DeviceBuffer of [world][len(chunk)] floats,
    rank-major; the elements of `tensors` that lie in the chunk become host_average_gradients of the `world` slabs, in place.
    No communicator is involved.  workspace as for grad_pack_device.  -> tensors; nothing is synchronised."""
    tensors, table, sizes, total = _grad_table(tensors, chunk_elems)
    length = _grad_chunk(chunk, chunk_elems, total)
    if isinstance(world, bool) or not isinstance(world, (int, np.integer)) or world < 1:
        raise InvalidArgumentError(-1, 'grad_average: world must be a positive integer, got %r' % (world,))
    if workspace is not None and not isinstance(workspace, DeviceBuffer):
        raise InvalidArgumentError(-1, 'grad_average: workspace must be a DeviceBuffer')
    ptr = _grad_span(gathered, 'gathered', 0, world * length)
    ws = _grad_workspace(workspace, table, len(sizes), 1, chunk_elems)
    check(lib().xdet_grad_reduce_ranks(table, len(sizes), int(chunk), int(chunk_elems), ptr, int(world), ws.ptr, _handle(stream)))
    _keep_alive(tensors[:1], (ws, gathered), chain=True)
    return tensors
