"""Operator-level host API: the reference's custom op and the box algebra around it,
same names / argument meaning / error behaviour as the reference, running on HIP.

Inputs may be numpy arrays (copied to the GPU, results copied back -- convenient for
tests) or DeviceTensor / DeviceBuffer objects (stay on the GPU).
"""
import ctypes
import enum

import numpy as np

from ._lib import lib, check, c_void_p, InvalidArgumentError
from .runtime import DeviceBuffer, DeviceTensor, to_device, to_host, synchronize, _ptr, _host, channel_ld


def ps_roi_align(inputs, rois, grid_dim_width, grid_dim_height, pool_method, stream=None):
    """op_module.ps_roi_align (light_head_rfcn_eval.py:143-155; REGISTER_OP
    cpp/PSROIPooling/ps_roi_align_op.cc:38-76).

    inputs [N,C,H,W] f32 NCHW, rois [N,R,4] (cy,cx,h,w) in [0,1]
    -> (pooled_features [N,R,gh*gw,C/(gh*gw)] f32, pooled_index same shape i32).
    Raises InvalidArgumentError for the cases the reference's OP_REQUIRES reject
    (ps_roi_align_op.cc:209-226)."""
    if not isinstance(pool_method, str) or ('mean' not in pool_method and 'max' not in pool_method):
        raise InvalidArgumentError(-1, "Need Attr pool_method to be either 'mean' or 'max', got %r" % (pool_method,))
    if grid_dim_width < 0 or grid_dim_height < 0:
        raise InvalidArgumentError(-1, 'Need Attr grid_dim_width/grid_dim_height >= 0')
    inputs = np.asarray(inputs, np.float32)
    rois = np.asarray(rois, np.float32)
    if inputs.ndim != 4:
        raise InvalidArgumentError(-1, "inputs must be in 'NCHW' format.")
    if rois.ndim != 3 or rois.shape[2] != 4:
        raise InvalidArgumentError(-1, "rois must be in 'batch_size x num_rois x 4' format.")
    if inputs.shape[0] != rois.shape[0]:
        raise InvalidArgumentError(-1, "'batch_size' in inputs and rois don't match.")
    N, C, H, W = inputs.shape
    R = rois.shape[1]
    gs = grid_dim_width * grid_dim_height
    if gs == 0 or C % gs != 0:
        raise InvalidArgumentError(-1, 'channels must be divisible by grid_dim_width * grid_dim_height')
    d_in, d_roi = to_device(inputs), to_device(rois)
    n_out = N * R * C
    d_pool, d_idx = DeviceBuffer(max(n_out * 4, 16)), DeviceBuffer(max(n_out * 4, 16))
    check(lib().xdet_psroialign_fwd(d_in.ptr, d_roi.ptr, d_pool.ptr, d_idx.ptr, N, C, H, W, R, grid_dim_width,
                                    grid_dim_height, 1 if 'max' in pool_method else 0, 0, C, C, 0,
                                    stream.handle if stream else None))
    shape = (N, R, gs, C // gs)
    return to_host(d_pool.ptr, shape, np.float32, stream), to_host(d_idx.ptr, shape, np.int32, stream)


def ps_roi_align_grad(inputs, rois, pooled_features_grad, pooled_index, grid_dim_width, grid_dim_height, pool_method,
                      ordered=False, stream=None):
    """op_module.ps_roi_align_grad (REGISTER_OP cpp/PSROIPooling/ps_roi_align_grad_op.cc:39-57; registered as
    the gradient of PsRoiAlign in cpp/PSROIPooling/test_op.py:93-104).

    inputs [N,C,H,W] (only its shape is used, as in the reference), rois [N,R,4],
    pooled_features_grad / pooled_index [N,R,gh*gw,C/(gh*gw)] -> grad_output [N,C,H,W] f32.
    ordered=True: the same shapes and errors through xdet_psroialign_grad_ordered -- no float atomics, the sums in the
    order of a sequential evaluation (bit-identical to one); H*W is limited (include/xdet.h)."""
    if not isinstance(pool_method, str) or ('mean' not in pool_method and 'max' not in pool_method):
        raise InvalidArgumentError(-1, "Need Attr pool_method to be either 'mean' or 'max', got %r" % (pool_method,))
    shape = tuple(inputs.shape)
    rois = np.asarray(rois, np.float32)
    if len(shape) != 4:
        raise InvalidArgumentError(-1, "inputs must be in 'NCHW' format.")
    if rois.ndim != 3 or rois.shape[2] != 4:
        raise InvalidArgumentError(-1, "rois must be in 'batch_size x num_rois x 4' format.")
    if shape[0] != rois.shape[0]:
        raise InvalidArgumentError(-1, "'batch_size' in inputs and rois don't match.")
    N, C, H, W = shape
    R = rois.shape[1]
    gs = grid_dim_width * grid_dim_height
    if gs <= 0 or C % gs != 0:
        raise InvalidArgumentError(-1, 'channels must be divisible by grid_dim_width * grid_dim_height')
    grad = np.ascontiguousarray(pooled_features_grad, np.float32)
    index = np.ascontiguousarray(pooled_index, np.int32)
    if grad.size != N * R * C or index.size != N * R * C:
        raise InvalidArgumentError(-1, 'pooled_features_grad / pooled_index must hold batch_size*num_rois*channels '
                                       'elements')
    d_roi, d_grad, d_idx = to_device(rois), to_device(grad), to_device(index)
    d_out = DeviceBuffer(max(N * C * H * W * 4, 16))
    if ordered:
        check(lib().xdet_psroialign_grad_ordered(d_roi.ptr, d_grad.ptr, C, d_idx.ptr, C, d_out.ptr, N, C, H, W, R,
                                                 grid_dim_width, grid_dim_height, 1 if 'max' in pool_method else 0, 0, C, 0,
                                                 stream.handle if stream else None))
        return to_host(d_out.ptr, shape, np.float32, stream)
    check(lib().xdet_psroialign_grad(d_roi.ptr, d_grad.ptr, d_idx.ptr, d_out.ptr, N, C, H, W, R, grid_dim_width,
                                     grid_dim_height, 1 if 'max' in pool_method else 0, 0, C,
                                     stream.handle if stream else None))
    return to_host(d_out.ptr, shape, np.float32, stream)


def ps_roi_align_grad_device(rois, grad, index, shape, grid_dim_width, grid_dim_height, pool_method='max',
                             rois_are_corners=False, ld=None, out=None, stream=None):
    """xdet_psroialign_grad_ordered with everything left on the GPU; nothing is synchronised.
    rois: [N,R,4] NumPy array, DeviceBuffer or DeviceTensor (packed rows of 4; corner boxes with rois_are_corners=True);
    grad: DeviceTensor [N,R,1,C] (N*R rows of C with its ld) or a NumPy array of N*R*C elements; index: likewise as i32
    (a DeviceTensor / DeviceBuffer is read as int32), None for 'mean'; shape = (N, H, W, C) of the feature map.
    -> DeviceTensor [N,H,W,C] with channel stride `ld` (default: channel_ld(C)), every element written, padding zero.
    out: a DeviceTensor of that shape to write into instead."""
    if not isinstance(pool_method, str) or ('mean' not in pool_method and 'max' not in pool_method):
        raise InvalidArgumentError(-1, "Need Attr pool_method to be either 'mean' or 'max', got %r" % (pool_method,))
    use_max = 'max' in pool_method
    if len(shape) != 4:
        raise InvalidArgumentError(-1, 'ps_roi_align_grad_device: shape must be (N, H, W, C)')
    N, H, W, C = (int(v) for v in shape)
    gs = grid_dim_width * grid_dim_height
    if gs <= 0 or C % gs != 0:
        raise InvalidArgumentError(-1, 'channels must be divisible by grid_dim_width * grid_dim_height')
    if use_max and index is None:
        raise InvalidArgumentError(-1, "ps_roi_align_grad_device: 'max' needs the forward's pooled_index")
    keep = []

    def rows(a, dtype, what):
        if isinstance(a, DeviceTensor):
            if a.shape[-1] != C:
                raise InvalidArgumentError(-1, 'ps_roi_align_grad_device: %s has %d channels, the map %d' % (what, a.shape[-1], C))
            return a.ptr, a.ld, int(np.prod(a.shape[:-1]))
        a = np.ascontiguousarray(a, dtype)
        if a.size % C:
            raise InvalidArgumentError(-1, 'ps_roi_align_grad_device: %s must hold rows of %d channels' % (what, C))
        b = to_device(a)
        keep.append(b)
        return b.ptr, C, a.size // C
    pg, ldg, ng = rows(grad, np.float32, 'grad')
    pi, ldi, ni = rows(index, np.int32, 'index') if index is not None else (None, C, ng)
    if isinstance(rois, (DeviceTensor, DeviceBuffer)):
        pr = rois.ptr
        nroi = (int(np.prod(rois.shape)) if isinstance(rois, DeviceTensor) else rois.nbytes // 4) // 4
    else:
        r = np.ascontiguousarray(rois, np.float32)
        if r.ndim != 3 or r.shape[2] != 4 or r.shape[0] != N:
            raise InvalidArgumentError(-1, "rois must be in 'batch_size x num_rois x 4' format.")
        b = to_device(r)
        keep.append(b)
        pr, nroi = b.ptr, r.shape[0] * r.shape[1]
    if N <= 0 or ng % N or ni != ng or nroi < ng:
        raise InvalidArgumentError(-1, 'ps_roi_align_grad_device: %d gradient rows, %d index rows, %d ROIs for %d images'
                                   % (ng, ni, nroi, N))
    R = ng // N
    if out is None:
        out = DeviceTensor.empty((N, H, W, C), ld=ld)
    elif tuple(out.shape) != (N, H, W, C):
        raise InvalidArgumentError(-1, 'ps_roi_align_grad_device: out has shape %r, not %r' % (out.shape, (N, H, W, C)))
    check(lib().xdet_psroialign_grad_ordered(pr, pg, ldg, pi, ldi, out.ptr, N, C, H, W, R, grid_dim_width, grid_dim_height,
                                             1 if use_max else 0, 1, out.ld, 1 if rois_are_corners else 0,
                                             stream.handle if stream else None))
    out._keep = (keep, rois, grad, index)      # operands live until the stream has run the call
    return out


def _rotated_checks(inputs_shape, rois, orders, grid_dim_width, grid_dim_height, pool_method):
    """RotatedPSROIAlignOp / RotatedPSROIAlignGradOp's OP_REQUIRES (rotated_ps_roi_align_op.cc:308-343,
    rotated_ps_roi_align_grad_op.cc:397-436), plus a zero grid and C not divisible by gh*gw (the reference divides by
    zero there) -> (N, C, H, W, R, grid_size)"""
    if not isinstance(pool_method, str) or ('mean' not in pool_method and 'max' not in pool_method):
        raise InvalidArgumentError(-1, "Need Attr pool_method to be either 'mean' or 'max', got %r" % (pool_method,))
    if grid_dim_width < 0 or grid_dim_height < 0:
        raise InvalidArgumentError(-1, 'Need Attr grid_dim_width/grid_dim_height >= 0')
    if len(inputs_shape) != 4:
        raise InvalidArgumentError(-1, "inputs must be in 'NCHW' format.")
    if rois.ndim != 3 or rois.shape[2] != 8:
        raise InvalidArgumentError(-1, "rois must be in 'batch_size x num_rois x 8' format.")
    if orders.ndim != 2:
        raise InvalidArgumentError(-1, "orders must be in 'batch_size x num_rois' format.")
    if inputs_shape[0] != rois.shape[0]:
        raise InvalidArgumentError(-1, "'batch_size' in inputs and rois don't match.")
    if orders.shape != rois.shape[:2]:
        raise InvalidArgumentError(-1, "'batch_size' or 'num_rois' in orders and rois don't match.")
    N, C, H, W = (int(d) for d in inputs_shape)
    gs = int(grid_dim_width) * int(grid_dim_height)
    if gs == 0 or C % gs != 0:
        raise InvalidArgumentError(-1, 'channels must be divisible by grid_dim_width * grid_dim_height (> 0)')
    return N, C, H, W, rois.shape[1], gs


def rotated_ps_roi_align(inputs, rois, orders, grid_dim_width, grid_dim_height, pool_method, stream=None):
    """op_module.rotated_ps_roi_align (REGISTER_OP cpp/PSROIPooling/rotated_ps_roi_align_op.cc:38-77).

    inputs [N,C,H,W] f32 NCHW, rois [N,R,8] four vertices (y0,x0,...,y3,x3) in [0,1] clockwise, orders [N,R] i32
    (first vertex; -1: the one starting the shorter side pair) -> (pooled_features [N,R,gh*gw,C/(gh*gw)] f32,
    pooled_index same shape i32).  Bit-exact against the reference's CPU functor; out-of-bounds samples and orders
    outside [-1, 4) as include/xdet.h states.  Raises InvalidArgumentError for the cases the reference's OP_REQUIRES
    reject (and for a zero grid or C not divisible by gh*gw)."""
    inputs = np.asarray(inputs, np.float32)
    rois = np.asarray(rois, np.float32)
    orders = np.asarray(orders)
    N, C, H, W, R, gs = _rotated_checks(inputs.shape, rois, orders, grid_dim_width, grid_dim_height, pool_method)
    orders = np.ascontiguousarray(orders, np.int32)
    d_in, d_roi, d_ord = to_device(inputs), to_device(rois), to_device(orders)
    n_out = N * R * C
    d_pool, d_idx = DeviceBuffer(max(n_out * 4, 16)), DeviceBuffer(max(n_out * 4, 16))
    check(lib().xdet_rotated_psroialign_fwd(d_in.ptr, d_roi.ptr, d_ord.ptr, d_pool.ptr, d_idx.ptr, N, C, H, W, R,
                                            grid_dim_width, grid_dim_height, 1 if 'max' in pool_method else 0, 0, C,
                                            stream.handle if stream else None))
    shape = (N, R, gs, C // gs)
    return to_host(d_pool.ptr, shape, np.float32, stream), to_host(d_idx.ptr, shape, np.int32, stream)


def rotated_ps_roi_align_grad(inputs, rois, orders, pooled_features_grad, pooled_index, grid_dim_width,
                              grid_dim_height, pool_method, stream=None):
    """op_module.rotated_ps_roi_align_grad (REGISTER_OP cpp/PSROIPooling/rotated_ps_roi_align_grad_op.cc:39-60; the
    gradient of RotatedPsRoiAlign, cpp/PSROIPooling/test_op.py:150-162).

    inputs [N,C,H,W] (only its shape is used, as in the reference), rois [N,R,8], orders [N,R],
    pooled_features_grad / pooled_index [N,R,gh*gw,C/(gh*gw)] -> grad_output [N,C,H,W] f32 (float atomics:
    agreement with a sequential evaluation to rounding)."""
    shape = tuple(inputs.shape)
    rois = np.asarray(rois, np.float32)
    orders = np.asarray(orders)
    grad = np.ascontiguousarray(pooled_features_grad, np.float32)
    index = np.ascontiguousarray(pooled_index, np.int32)
    N, C, H, W, R, gs = _rotated_checks(shape, rois, orders, grid_dim_width, grid_dim_height, pool_method)
    if grad.shape != index.shape:
        raise InvalidArgumentError(-1, 'pooled_index and pooled_features_grad must have the same shape')
    if grad.shape != (N, R, gs, C // gs):
        raise InvalidArgumentError(-1, "both pooled_index and pooled_features_grad must have the shape "
                                       "'batch_size x num_rois x grid_size x bank_size'")
    orders = np.ascontiguousarray(orders, np.int32)
    d_roi, d_ord, d_grad, d_idx = to_device(rois), to_device(orders), to_device(grad), to_device(index)
    d_out = DeviceBuffer(max(N * C * H * W * 4, 16))
    check(lib().xdet_rotated_psroialign_grad(d_roi.ptr, d_ord.ptr, d_grad.ptr, d_idx.ptr, d_out.ptr, N, C, H, W, R,
                                             grid_dim_width, grid_dim_height, 1 if 'max' in pool_method else 0, 0, C,
                                             stream.handle if stream else None))
    return to_host(d_out.ptr, shape, np.float32, stream)


PAD_VALID, PAD_SAME, PAD_EXPLICIT = 0, 1, 2


class Conv2D(object):
    """tf.layers.conv2d / dense with folded inference BN or bias (+ReLU) on the f32 MFMA pipe."""
    def __init__(self, kernel_hwio, stride=1, padding='SAME', dilation=1, scale=None, shift=None, relu=False,
                 explicit_pad=0):
        k = np.ascontiguousarray(kernel_hwio, np.float32)
        self.kh, self.kw, self.cin, self.cout = k.shape
        mode = {'VALID': PAD_VALID, 'SAME': PAD_SAME, 'EXPLICIT': PAD_EXPLICIT}[padding]
        sc = None if scale is None else np.ascontiguousarray(scale, np.float32)
        sh = None if shift is None else np.ascontiguousarray(shift, np.float32)
        h = c_void_p()
        check(lib().xdet_conv_create(ctypes.byref(h), self.kh, self.kw, self.cin, self.cout, stride, dilation, mode,
                                     explicit_pad, explicit_pad, _host(k), _host(sc) if sc is not None else None,
                                     _host(sh) if sh is not None else None, 1 if relu else 0))
        self.handle = h

    def set_ksplit(self, ksplit, mode=0, max_parallel_tiles=None):
        """fixed split of the reduction (xdet_conv_set_ksplit): the planes path then runs on the split-K kernel;
        mode 0 = by grid size, 1 = ranges in parallel, 2 = one workgroup per tile -- all bit-identical."""
        if max_parallel_tiles is None:       # the parallel form is chosen for grids up to 448 (tile, range) workgroups
            max_parallel_tiles = 448 // max(int(ksplit), 1)
        check(lib().xdet_conv_set_ksplit(self.handle, int(ksplit), int(mode), int(max_parallel_tiles)))

    def set_kernel_device(self, t, shift=None, stream=None):
        """Rewrite every operand buffer of the layer from a kernel in device memory (xdet_conv_set_kernel_device): t is a dense
        DeviceTensor [kh,kw,cin,cout] (ld cout), shift a DeviceBuffer / DeviceTensor of cout floats or None (kept).  The
        layer then holds what Conv2D(t's values, ...) would hold, bit for bit; nothing is synchronised or read on the host.
        Refused for a grouped or calibrated layer (the library's refusal) and for a wrong shape."""
        want = (self.kh, self.kw, self.cin, self.cout)
        if not isinstance(t, DeviceTensor) or tuple(t.shape) != want or t.ld != self.cout:
            raise InvalidArgumentError(-1, 'Conv2D.set_kernel_device: a dense DeviceTensor of shape %r expected, got %r (ld %r)'
                                       % (want, getattr(t, 'shape', None), getattr(t, 'ld', None)))
        if shift is not None and (not isinstance(shift, (DeviceBuffer, DeviceTensor))
                                  or (isinstance(shift, DeviceBuffer) and shift.nbytes < 4 * self.cout)):
            raise InvalidArgumentError(-1, 'Conv2D.set_kernel_device: shift must be a device array of %d floats' % self.cout)
        check(lib().xdet_conv_set_kernel_device(self.handle, t.ptr, shift.ptr if shift is not None else None,
                                                stream.handle if stream else None))

    def out_shape(self, H, W):
        ho, wo = ctypes.c_int(), ctypes.c_int()
        check(lib().xdet_conv_out_shape(self.handle, H, W, ctypes.byref(ho), ctypes.byref(wo)))
        return ho.value, wo.value

    def __call__(self, x, residual=None, relu_in=False, stream=None, planes=False, staged_tile=False, x8_exp=None):
        """planes=True (split-precision modes only): split x into f16 hi/lo planes first and run the
        LDS-DMA kernel -- the path every big contraction takes inside a net.  staged_tile=True (with planes; 3x3 VALID
        stride 1 over 32 channels, <= 64 outputs): the kernel that stages the input tile once in LDS
        (xdet_conv3x3_patch_forward, block1_conv2 inside a net).  x8_exp (with planes; 1x1 stride-1 layers): the x8 form of
        the planes -- the cross terms of the split-precision product from fp8 copies (xdet_conv_forward_planes_x8); pass the
        exponent e with max|x| * 2^-e in (128, 256]."""
        N, H, W, C = x.shape
        assert C == self.cin, (C, self.cin)
        ho, wo = self.out_shape(H, W)
        out = DeviceTensor.empty((N, ho, wo, self.cout))
        if planes:
            n = -(-N * H * W // 16) * 16 * x.ld
            hi, lo = DeviceBuffer(n * 2 + 512, zero=True), DeviceBuffer(n * 2 + 512, zero=True)
            st = stream.handle if stream else None
            if x8_exp is not None:
                # the x8 form of the planes (pointwise layers): cross terms from fp8 copies scaled by 2^-x8_exp
                assert not staged_tile
                check(lib().xdet_split_f32_x8(x.ptr, hi.ptr, lo.ptr, N * H * W, x.ld, 1 if relu_in else 0, int(x8_exp), st))
                check(lib().xdet_conv_forward_planes_x8(self.handle, hi.ptr, lo.ptr, N, H, W, x.ld, out.ptr, out.ld,
                                                        residual.ptr if residual is not None else None, int(x8_exp), st))
                synchronize(stream)
                return out
            check(lib().xdet_split_f32(x.ptr, hi.ptr, lo.ptr, N * H * W, x.ld, 1 if relu_in else 0, st))
            if staged_tile:
                assert residual is None
                check(lib().xdet_conv3x3_patch_forward(self.handle, hi.ptr, lo.ptr, N, H, W, out.ptr, out.ld, st))
            else:
                check(lib().xdet_conv_forward_planes(self.handle, hi.ptr, lo.ptr, N, H, W, x.ld, out.ptr, out.ld,
                                                     residual.ptr if residual is not None else None, st))
            synchronize(stream)
            return out
        check(lib().xdet_conv_forward(self.handle, x.ptr, N, H, W, x.ld, out.ptr, out.ld,
                                      residual.ptr if residual is not None else None, 1 if relu_in else 0,
                                      stream.handle if stream else None))
        return out

    def emit(self, x=None, in_planes=None, shape=None, x8_exp=None, relu_in=False, residual=None, out=None, out_planes=None,
             planes_ld=0, planes_relu=False, bn=None, out_exp=0, stream=None):
        """The layer with everything its epilogue can write (xdet_conv_forward_emit), as a net's plan asks for it.
        Input: x (f32 DeviceTensor) or in_planes = (hi, lo) buffers with shape = (N, H, W) (x8_exp: the x8 form).
        out: a DeviceTensor or None (planes only); out_planes: (hi, lo) buffers or None; planes_ld: channel stride of a wider
        planes destination; bn = (scale, shift) host arrays [cout]: a BN folded into the planes copy; out_exp: planes * 2^-out_exp.
        The caller owns every buffer (the tests poison them)."""
        if x is not None:
            N, H, W, C = x.shape
            assert C == self.cin, (C, self.cin)
            ld_in = x.ld
        else:
            N, H, W = shape
            ld_in = channel_ld(self.cin)
        sc = sh = None
        if bn is not None:
            sc, sh = (np.ascontiguousarray(a, np.float32) for a in bn)
            assert sc.shape == sh.shape == (self.cout,)
        ih, il = in_planes if in_planes is not None else (None, None)
        oh, ol = out_planes if out_planes is not None else (None, None)
        p = lambda b: b.ptr if b is not None else None
        check(lib().xdet_conv_forward_emit(self.handle, p(x), p(ih), p(il), 0 if x8_exp is None else 1, int(x8_exp or 0),
                                           1 if relu_in else 0, N, H, W, ld_in, p(out), -(-self.cout // 32) * 32, p(residual), p(oh),
                                           p(ol), int(planes_ld), 1 if planes_relu else 0, _host(sc) if sc is not None else None,
                                           _host(sh) if sh is not None else None, int(out_exp),
                                           stream.handle if stream else None))
        synchronize(stream)
        return out

    def __del__(self):
        try:
            lib().xdet_layer_destroy(self.handle)
        except Exception:
            pass


class DepthwiseConv2D(object):
    """depthwise half of tf.layers.separable_conv2d (3x3, stride 1, SAME)."""
    def __init__(self, dw_kernel, dilation=1):
        k = np.ascontiguousarray(dw_kernel, np.float32)
        assert k.shape[:2] == (3, 3) and k.shape[3] == 1
        self.C = k.shape[2]
        h = c_void_p()
        check(lib().xdet_depthwise_create(ctypes.byref(h), self.C, dilation, _host(k)))
        self.handle = h

    def set_kernel_device(self, t, stream=None):
        """Rewrite the layer's taps from a kernel in device memory (xdet_depthwise_set_kernel_device): t is a dense
        DeviceTensor [3,3,C,1] (ld 1); nothing is synchronised or read on the host."""
        if not isinstance(t, DeviceTensor) or tuple(t.shape) != (3, 3, self.C, 1) or t.ld != 1:
            raise InvalidArgumentError(-1, 'DepthwiseConv2D.set_kernel_device: a dense DeviceTensor of shape %r expected, got %r '
                                           '(ld %r)' % ((3, 3, self.C, 1), getattr(t, 'shape', None), getattr(t, 'ld', None)))
        check(lib().xdet_depthwise_set_kernel_device(self.handle, t.ptr, stream.handle if stream else None))

    def __call__(self, x, relu_in=False, stream=None):
        N, H, W, C = x.shape
        out = DeviceTensor.empty((N, H, W, C))
        check(lib().xdet_depthwise_forward(self.handle, x.ptr, N, H, W, x.ld, out.ptr, 1 if relu_in else 0,
                                           stream.handle if stream else None))
        return out

    def __del__(self):
        try:
            lib().xdet_layer_destroy(self.handle)
        except Exception:
            pass


class SeparableConvBN(object):
    """relu_separable_bn_block (net/xception_body.py:220-234): (ReLU ->) depthwise 3x3 -> pointwise 1x1 -> BN
    (folded into scale/shift) (-> ReLU), stride 1, SAME.  fused=True runs the one-kernel form
    (xdet_sepconv_fused_forward; split-precision modes, <= 256 input channels, 128 / 256 outputs), fused=False
    depthwise -> split planes -> pointwise, the form the wide layers of a net use; both give the same bits."""
    def __init__(self, dw_kernel, pw_kernel, scale=None, shift=None, relu=False, dilation=1):
        self.dw = DepthwiseConv2D(dw_kernel, dilation)
        self.pw = Conv2D(pw_kernel, 1, 'SAME', 1, scale, shift, relu)

    def __call__(self, x, relu_in=False, fused=True, stream=None):
        N, H, W, C = x.shape
        if not fused:
            return self.pw(self.dw(x, relu_in=relu_in, stream=stream), stream=stream, planes=True)
        out = DeviceTensor.empty((N, H, W, self.pw.cout))
        check(lib().xdet_sepconv_fused_forward(self.dw.handle, self.pw.handle, x.ptr, N, H, W, x.ld, out.ptr, out.ld,
                                               1 if relu_in else 0, stream.handle if stream else None))
        synchronize(stream)
        return out


def separable_block_then_pool_add(op, x, residual, relu_in=False, stream=None):
    """SeparableConvBN `op` -> max_pooling2d(3, 2, 'same') -> + residual with the pool split between the block's epilogue
    (horizontal half) and a light vertical pass (xdet_sepconv_fused_hpool_forward + xdet_maxpool_v3s2_add)."""
    N, H, W, C = x.shape
    Ho, Wo = -(-H // 2), -(-W // 2)
    hp = DeviceTensor.empty((N, H, Wo, op.pw.cout))
    out = DeviceTensor.empty((N, Ho, Wo, op.pw.cout))
    st = stream.handle if stream else None
    check(lib().xdet_sepconv_fused_hpool_forward(op.dw.handle, op.pw.handle, x.ptr, N, H, W, x.ld, hp.ptr, hp.ld,
                                                 1 if relu_in else 0, st))
    check(lib().xdet_maxpool_v3s2_add(hp.ptr, residual.ptr if residual is not None else None, out.ptr, N, H, Wo,
                                      op.pw.cout, hp.ld, st))
    synchronize(stream)
    return out


def max_pool_3x3_s2_same_add(x, residual=None, stream=None):
    N, H, W, C = x.shape
    out = DeviceTensor.empty((N, -(-H // 2), -(-W // 2), C))
    check(lib().xdet_maxpool3x3s2_add(x.ptr, residual.ptr if residual is not None else None, out.ptr, N, H, W, C,
                                      x.ld, stream.handle if stream else None))
    return out


def planes_bytes(n_pix, ld):
    """bytes of one f16 plane of the xdet_split_f32 layout [ceil(n_pix/16)][ld/32][16][32]"""
    return -(-n_pix // 16) * 16 * ld * 2


def _planes_pair(out, n_pix, ld):
    if out is not None:
        return out
    return DeviceBuffer(planes_bytes(n_pix, ld), zero=True), DeviceBuffer(planes_bytes(n_pix, ld), zero=True)


class SpectralConv(object):
    """A (T,1) [axis 0] or (1,T) [axis 1] SAME convolution (T <= 15 taps, stride 1) over an F x F map in the DFT domain of the
    convolved axis (xdet_spectral_conv_*; the large-separable convs, net/xception_body.py:450-475), with folded
    scale / shift (+ReLU).  kernel [T, cin, cout]; F in (16, 30, 50); split-precision modes only."""
    def __init__(self, kernel, axis, F, scale=None, shift=None, relu=False):
        k = np.ascontiguousarray(kernel, np.float32)
        self.taps, self.cin, self.cout = k.shape
        self.axis, self.F = int(axis), int(F)
        sc = None if scale is None else np.ascontiguousarray(scale, np.float32)
        sh = None if shift is None else np.ascontiguousarray(shift, np.float32)
        h = c_void_p()
        check(lib().xdet_spectral_conv_create(ctypes.byref(h), _host(k), self.taps, self.cin, self.cout, self.axis, self.F,
                                              _host(sc) if sc is not None else None, _host(sh) if sh is not None else None,
                                              1 if relu else 0))
        self.handle = h

    def workspace_bytes(self, N):
        return int(lib().xdet_spectral_conv_workspace_bytes(self.handle, int(N)))

    def set_kernel_device(self, kernel, scale=None, shift=None, stream=None):
        """Rewrite the layer's DFT-domain block matrices from a kernel in device memory (xdet_spectral_conv_set_kernel_device):
        kernel is a dense DeviceTensor [T, cin, cout] (ld cout), scale / shift DeviceBuffers / DeviceTensors of cout floats or
        None (kept).  The layer then holds what SpectralConv(kernel's values, ...) would hold, bit for bit; nothing is
        synchronised or read on the host.  Refused by name: a host array, a wrong shape."""
        want = (self.taps, self.cin, self.cout)
        if not isinstance(kernel, DeviceTensor) or tuple(kernel.shape) != want or kernel.ld != self.cout:
            raise InvalidArgumentError(-1, 'SpectralConv.set_kernel_device: kernel must be a dense DeviceTensor of shape %r (device '
                                       'memory), got %s %r (ld %r)' % (want, type(kernel).__name__, getattr(kernel, 'shape', None),
                                                                       getattr(kernel, 'ld', None)))
        for name, a in (('scale', scale), ('shift', shift)):
            if a is not None and (not isinstance(a, (DeviceBuffer, DeviceTensor))
                                  or (isinstance(a, DeviceBuffer) and a.nbytes < 4 * self.cout)):
                raise InvalidArgumentError(-1, 'SpectralConv.set_kernel_device: %s must be a device array of %d floats, got %s'
                                           % (name, self.cout, type(a).__name__))
        check(lib().xdet_spectral_conv_set_kernel_device(self.handle, kernel.ptr, scale.ptr if scale is not None else None,
                                                         shift.ptr if shift is not None else None,
                                                         stream.handle if stream else None))

    def __call__(self, x, out=None, workspace=None, stream=None):
        """x: DeviceTensor [N,F,F,cin]; out (optional): a DeviceTensor to write into (its ld may exceed round_up(cout,32));
        workspace (optional): a DeviceBuffer of workspace_bytes(N) bytes, any contents"""
        N, H, W, C = x.shape
        assert (H, W, C) == (self.F, self.F, self.cin), (x.shape, self.F, self.cin)
        if out is None:
            out = DeviceTensor.empty((N, H, W, self.cout))
        ws = workspace if workspace is not None else DeviceBuffer(self.workspace_bytes(N))
        check(lib().xdet_spectral_conv_forward(self.handle, x.ptr, N, x.ld, ws.ptr, out.ptr, out.ld,
                                               stream.handle if stream else None))
        synchronize(stream)
        return out

    def __del__(self):
        try:
            lib().xdet_layer_destroy(self.handle)
        except Exception:
            pass


def stem_conv3x3s2(images_nchw, kernel_hwio, scale, shift, out=None, stream=None):
    """block1_conv1 (net/xception_body.py:243-250; xdet_stem_conv3x3s2_forward): images f32 [N,3,S,S], kernel [3,3,3,32],
    scale / shift [32] (folded BN; ReLU follows) -> (hi, lo) planes (ld 32) of the [N,Ho,Ho,32] output, Ho = (S-3)//2 + 1.
    out: a (hi, lo) pair of DeviceBuffers to write into."""
    x = np.ascontiguousarray(images_nchw, np.float32)
    N, C, S, S2 = x.shape
    assert C == 3 and S == S2 and tuple(np.shape(kernel_hwio)) == (3, 3, 3, 32)
    Ho = (S - 3) // 2 + 1
    d_x, d_w = to_device(x), to_device(np.ascontiguousarray(kernel_hwio, np.float32))
    d_sc, d_sh = to_device(np.ascontiguousarray(scale, np.float32)), to_device(np.ascontiguousarray(shift, np.float32))
    hi, lo = _planes_pair(out, N * Ho * Ho, 32)
    check(lib().xdet_stem_conv3x3s2_forward(d_x.ptr, d_w.ptr, d_sc.ptr, d_sh.ptr, hi.ptr, lo.ptr, N, S,
                                            stream.handle if stream else None))
    synchronize(stream)
    return hi, lo


def stem_conv3x3s2_train(images_nchw, kernel_hwio, ld=32, out=None, stream=None):
    """block1_conv1 in training mode (xdet_stem_conv3x3s2_train_forward): images f32 [N,3,S,S], kernel [3,3,3,32] -> the raw f32
    conv output as a DeviceTensor [N,Ho,Ho,32] with pixel stride ld, Ho = (S-3)//2 + 1 -- no BN, no ReLU, no split; channels
    32 .. ld - 1 of a pixel are not written.  out: a DeviceTensor [N,Ho,Ho,32] to write into (with its ld)."""
    x = np.ascontiguousarray(images_nchw, np.float32)
    N, C, S, S2 = x.shape
    assert C == 3 and S == S2 and tuple(np.shape(kernel_hwio)) == (3, 3, 3, 32)
    Ho = (S - 3) // 2 + 1
    d_x, d_w = to_device(x), to_device(np.ascontiguousarray(kernel_hwio, np.float32))
    z = out if out is not None else DeviceTensor.empty((N, Ho, Ho, 32), ld=ld)
    assert tuple(z.shape) == (N, Ho, Ho, 32), z.shape
    check(lib().xdet_stem_conv3x3s2_train_forward(d_x.ptr, d_w.ptr, N, S, z.ptr, z.ld, stream.handle if stream else None))
    synchronize(stream)
    return z


def resnet_stem7x7(conv, images_nchw, stream=None):
    """conv2d_fixed_padding(7, 64, stride 2) of the ResNet v2 stem on its own kernel (xdet_resnet_stem7x7_forward): `conv` a
    Conv2D(7x7x3x64, stride 2, 'EXPLICIT', explicit_pad=3) created in the f16x3 mode, images f32 [N,3,S,S] -> DeviceTensor
    [N,Ho,Ho,64]; the same bits as conv(NHWC images)."""
    x = np.ascontiguousarray(images_nchw, np.float32)
    N, C, S, S2 = x.shape
    assert C == 3 and S == S2
    Ho = (S - 1) // 2 + 1
    d_x = to_device(x)
    out = DeviceTensor.empty((N, Ho, Ho, 64))
    check(lib().xdet_resnet_stem7x7_forward(conv.handle, d_x.ptr, N, S, out.ptr, stream.handle if stream else None))
    synchronize(stream)
    return out


def max_pool_3x3_s2_bn_planes(x, scale, shift, mul=1.0, out=None, second=None, stream=None):
    """max_pooling2d(3, 2, 'same') -> relu(. * scale + shift) * mul as split planes (xdet_maxpool3x3s2_bn_planes; the ResNet
    stem tail, net/resnet_v2.py:311-330 + :142-156).  x: DeviceTensor [N,H,W,C] (ld % 32 == 0); scale / shift [ld].
    second = (hi2_ptr, lo2_ptr, c32_2, mul2): a second copy * mul2 into the channel blocks of a wider planes tensor.
    -> (hi, lo) DeviceBuffers over the N * ceil(H/2) * ceil(W/2) pixels."""
    N, H, W, C = x.shape
    n_pix = N * -(-H // 2) * -(-W // 2)
    d_sc, d_sh = to_device(np.ascontiguousarray(scale, np.float32)), to_device(np.ascontiguousarray(shift, np.float32))
    hi, lo = _planes_pair(out, n_pix, x.ld)
    hi2, lo2, c32_2, mul2 = second if second is not None else (None, None, 0, 1.0)
    check(lib().xdet_maxpool3x3s2_bn_planes(x.ptr, d_sc.ptr, d_sh.ptr, hi.ptr, lo.ptr, N, H, W, C, x.ld, float(mul),
                                            _ptr(hi2), _ptr(lo2), int(c32_2), float(mul2), stream.handle if stream else None))
    synchronize(stream)
    return hi, lo


def resnet_preconv(conv, pre_scale, pre_shift, x, out=None, stream=None):
    """The opening 1x1 conv of a ResNet v2 bottleneck with the pre-activation made on the CU (xdet_resnet_preconv_forward):
    planes of conv(relu(x * pre_scale + pre_shift)); `conv` a 1x1 Conv2D with ReLU, 256 | 512 -> 128 channels, created in the
    f16x3 mode.  x: DeviceTensor [N,H,W,cin] -> (hi, lo) DeviceBuffers (ld 128)."""
    N, H, W, C = x.shape
    assert C == conv.cin and x.ld == C, (C, x.ld, conv.cin)
    d_sc, d_sh = to_device(np.ascontiguousarray(pre_scale, np.float32)), to_device(np.ascontiguousarray(pre_shift, np.float32))
    hi, lo = _planes_pair(out, N * H * W, channel_ld(conv.cout))
    check(lib().xdet_resnet_preconv_forward(conv.handle, d_sc.ptr, d_sh.ptr, x.ptr, N, H, W, hi.ptr, lo.ptr,
                                            stream.handle if stream else None))
    synchronize(stream)
    return hi, lo


class AnchorCreator(object):
    """preprocessing/anchor_manipulator.py:686-757 (single feature layer)."""
    def __init__(self, img_shape, layers_shapes, anchor_scales, extra_anchor_scales, anchor_ratios, layer_steps):
        self._img_shape = img_shape
        self._layers_shapes = layers_shapes
        self._anchor_scales = anchor_scales
        self._extra_anchor_scales = extra_anchor_scales
        self._anchor_ratios = anchor_ratios
        self._layer_steps = layer_steps

    def get_layer_anchors(self, layer_shape, anchor_scale, extra_anchor_scale, anchor_ratio, layer_step, offset=0.5):
        import math
        f = np.float32
        xs, ys = np.meshgrid(np.arange(layer_shape[1]), np.arange(layer_shape[0]))
        y = ((ys.astype(f) + f(offset)) * f(layer_step) / f(self._img_shape[0])).astype(f)
        x = ((xs.astype(f) + f(offset)) * f(layer_step) / f(self._img_shape[1])).astype(f)
        hs = [s for s in extra_anchor_scale] + [s / math.sqrt(r) for s in anchor_scale for r in anchor_ratio]
        ws = [s for s in extra_anchor_scale] + [s * math.sqrt(r) for s in anchor_scale for r in anchor_ratio]
        return y, x, np.array(hs, f), np.array(ws, f), len(hs)

    def get_all_anchors(self):
        all_anchors, num = [], []
        for i, shp in enumerate(self._layers_shapes):
            a = self.get_layer_anchors(shp, self._anchor_scales[i], self._extra_anchor_scales[i],
                                       self._anchor_ratios[i], self._layer_steps[i])
            all_anchors.append(a[:-1])
            num.append(a[-1])
        return all_anchors, num


def rpn_decode(rpn_cls, rpn_box, anchors, stream=None):
    """RPN glue + AnchorEncoder.decode_all_anchors(squeeze_inner=True)
    (light_head_rfcn_eval.py:389-397, anchor_manipulator.py:641-669).
    rpn_cls [N,Hh,Ww,2A], rpn_box [N,Hh,Ww,4A] numpy NHWC -> objectness [N,HWA], boxes [N,HWA,4]."""
    rpn_cls = np.asarray(rpn_cls, np.float32)
    rpn_box = np.asarray(rpn_box, np.float32)
    N, Hh, Ww, A2 = rpn_cls.shape
    A = A2 // 2
    both = np.concatenate([rpn_cls, rpn_box], axis=-1)
    t = DeviceTensor.from_numpy(both)
    yref, xref, href, wref = anchors
    yx = to_device(np.stack([yref.reshape(-1), xref.reshape(-1)], axis=1).astype(np.float32))
    hw = to_device(np.stack([href, wref], axis=1).astype(np.float32))
    n_anchor = Hh * Ww * A
    d_obj, d_box = DeviceBuffer(N * n_anchor * 4), DeviceBuffer(N * n_anchor * 16)
    check(lib().xdet_rpn_decode(t.ptr, t.ld, 0, 2 * A, N, Hh, Ww, A, yx.ptr, hw.ptr, d_obj.ptr, d_box.ptr,
                                stream.handle if stream else None))
    return to_host(d_obj.ptr, (N, n_anchor), np.float32, stream), to_host(d_box.ptr, (N, n_anchor, 4), np.float32, stream)


def get_proposals(object_score, bboxes_pred, encode_fn=None, rpn_pre_nms_top_n=5000, rpn_post_nms_top_n=1000,
                  nms_threshold=0.7, rpn_min_size=16. / 480, is_training=False, data_format='channels_first',
                  return_counts=False, stream=None):
    """net/xception_body.py:402-448.  object_score [N,n], bboxes_pred [N,n,4] -> proposals [N,post_n,4].
    is_training=True (:446-448): the same proposal stage, then encode_fn(proposals) with the proposals handed over on the
    device (a DeviceTensor [N,post_n,1,4]) -> its (rois, targets, labels, scores), e.g. of
    targets.AnchorEncoder.ext_encode_rois."""
    if is_training and encode_fn is None:
        raise InvalidArgumentError(-1, 'get_proposals: is_training=True needs an encode_fn')
    s = np.ascontiguousarray(object_score, np.float32)
    b = np.ascontiguousarray(bboxes_pred, np.float32)
    N, n = s.shape
    d_s, d_b = to_device(s), to_device(b)
    ws = DeviceBuffer(lib().xdet_proposals_workspace_bytes(N, n, rpn_pre_nms_top_n, rpn_post_nms_top_n), zero=True)
    d_r = DeviceBuffer(N * rpn_post_nms_top_n * 16)
    d_c = DeviceBuffer(N * 16)
    check(lib().xdet_get_proposals(d_s.ptr, d_b.ptr, N, n, rpn_pre_nms_top_n, rpn_post_nms_top_n, nms_threshold,
                                   rpn_min_size, ws.ptr, d_r.ptr, d_c.ptr, stream.handle if stream else None))
    if is_training:
        synchronize(stream)
        return encode_fn(DeviceTensor(d_r.ptr, (N, rpn_post_nms_top_n, 1, 4), 4, owner=d_r))
    rois = to_host(d_r.ptr, (N, rpn_post_nms_top_n, 4), np.float32, stream)
    if return_counts:
        return rois, to_host(d_c.ptr, (N, 4), np.int32, stream)
    return rois


def ext_decode_rois(proposals_roi, pred_location, head_prior_scaling=(1., 1., 1., 1.), stream=None):
    """AnchorEncoder.ext_decode_rois (anchor_manipulator.py:671-683); scaling is the eval default 1."""
    assert tuple(head_prior_scaling) == (1., 1., 1., 1.)
    r = np.ascontiguousarray(proposals_roi, np.float32)
    p = np.ascontiguousarray(pred_location, np.float32)
    n = int(np.prod(r.shape[:-1]))
    d_r, d_p, d_o = to_device(r), to_device(p), DeviceBuffer(max(n * 16, 16))
    check(lib().xdet_ext_decode_rois(d_r.ptr, d_p.ptr, 4, n, d_o.ptr, stream.handle if stream else None))
    return to_host(d_o.ptr, r.shape, np.float32, stream)


def bboxes_eval(cls_pred_logits, bboxes_pred, image_shape=(480, 480), bbox_img=(0., 0., 1., 1.), num_classes=21,
                select_threshold=0.01, nms_threshold=0.3, nms_topk=200, train_image_size=480, stream=None):
    """Detection part of bboxes_eval (light_head_rfcn_eval.py:263-287).
    cls_pred_logits [R,num_classes] (or [N,R,nc]), bboxes_pred [R,4] -> {c: (scores[topk], boxes[topk,4])}
    (a list of such dicts for batched input)."""
    c = np.asarray(cls_pred_logits, np.float32)
    b = np.asarray(bboxes_pred, np.float32)
    single = c.ndim == 2
    if single:
        c, b = c[None], b[None]
    N, R, nc = c.shape
    shapes = np.broadcast_to(np.asarray(image_shape, np.int32).reshape(-1, 2), (N, 2))
    bimg = np.broadcast_to(np.asarray(bbox_img, np.float32).reshape(-1, 4), (N, 4))
    d_c, d_b = to_device(c), to_device(b)
    d_s, d_i = to_device(np.ascontiguousarray(shapes)), to_device(np.ascontiguousarray(bimg))
    d_os, d_ob = DeviceBuffer(N * (nc - 1) * nms_topk * 4), DeviceBuffer(N * (nc - 1) * nms_topk * 16)
    check(lib().xdet_bboxes_eval(d_c.ptr, nc, d_b.ptr, N, R, nc, d_s.ptr, d_i.ptr, train_image_size,
                                 train_image_size, select_threshold, nms_threshold, nms_topk, d_os.ptr, d_ob.ptr,
                                 stream.handle if stream else None))
    sc = to_host(d_os.ptr, (N, nc - 1, nms_topk), np.float32, stream)
    bx = to_host(d_ob.ptr, (N, nc - 1, nms_topk, 4), np.float32, stream)
    out = [{k + 1: (sc[n, k], bx[n, k]) for k in range(nc - 1)} for n in range(N)]
    return out[0] if single else out


def head_decode_probs(rois, cls_reg, num_classes, R, form=0, stream=None):
    """xdet_head_decode_probs: the decode + softmax pass of the whole forward (csrc/detect.hip) on its own.
    rois [n,4] (or [N,R,4]), cls_reg 2-D [n,ld]: a row = num_classes logits, 4 regression values and ld - num_classes - 4
    columns that are never read; n = N * R.  -> (boxes [n,4], probs [N,num_classes,R] class-major, bad i32 [N]).
    form 0: the kernel the net gets; 1: one thread per ROI."""
    r = np.ascontiguousarray(rois, np.float32).reshape(-1, 4)
    c = np.ascontiguousarray(cls_reg, np.float32)
    if c.ndim != 2 or c.shape[0] != r.shape[0]:
        raise InvalidArgumentError(-1, 'head_decode_probs: cls_reg must be [n, ld] with one row per ROI, got %r for %d ROIs'
                                   % (c.shape, r.shape[0]))
    n, ld = c.shape
    N = n // R if R > 0 else 0
    d_r, d_c = to_device(r), to_device(c)
    d_b, d_p = DeviceBuffer(max(n * 16, 16)), DeviceBuffer(max(n * num_classes * 4, 16))
    d_bad = DeviceBuffer(max(N * 4, 16), zero=True)
    check(lib().xdet_head_decode_probs(d_r.ptr, d_c.ptr, ld, num_classes, R, n, form, d_b.ptr, d_p.ptr, d_bad.ptr,
                                       stream.handle if stream else None))
    return (to_host(d_b.ptr, (n, 4), np.float32, stream), to_host(d_p.ptr, (N, num_classes, R), np.float32, stream),
            to_host(d_bad.ptr, (N,), np.int32, stream))


def bboxes_eval_from_probs(probs, bboxes_pred, image_shape=(480, 480), bbox_img=(0., 0., 1., 1.), select_threshold=0.01,
                           nms_threshold=0.3, nms_topk=200, train_image_size=480, bad=None, stream=None, wide=False):
    """xdet_bboxes_eval_probs: bboxes_eval from head_decode_probs' outputs, as the whole forward runs it.
    probs [N,num_classes,R] (or [num_classes,R]), bboxes_pred [N*R,4] in any shape, bad: i32 [N] or None
    -> what bboxes_eval returns.
    wide=False: R <= 1024 (the door as ever).  wide=True: xdet_bboxes_eval_probs_wide, R <= 6144 -- the same kernel up to 1024
    ROIs per image, the wide one (keys of all R in LDS, the winners' boxes computed again) beyond, what a net with more than
    1024 proposals runs.  wide='force': xdet_bboxes_eval_probs_wide_only, the wide kernel at any R <= 6144 (tests: the two
    kernels on the same input)."""
    if not any(wide is v for v in (False, True)) and wide != 'force':
        raise InvalidArgumentError(-1, "bboxes_eval_from_probs: wide must be False, True or 'force', got %r" % (wide,))
    door = (lib().xdet_bboxes_eval_probs_wide_only if wide == 'force' else
            lib().xdet_bboxes_eval_probs_wide if wide else lib().xdet_bboxes_eval_probs)
    p = np.ascontiguousarray(probs, np.float32)
    single = p.ndim == 2
    if single:
        p = p[None]
    N, nc, R = p.shape
    b = np.ascontiguousarray(bboxes_pred, np.float32).reshape(N, R, 4)
    shapes = np.broadcast_to(np.asarray(image_shape, np.int32).reshape(-1, 2), (N, 2))
    bimg = np.broadcast_to(np.asarray(bbox_img, np.float32).reshape(-1, 4), (N, 4))
    d_p, d_b = to_device(p), to_device(b)
    d_s, d_i = to_device(np.ascontiguousarray(shapes)), to_device(np.ascontiguousarray(bimg))
    d_bad = None if bad is None else to_device(np.ascontiguousarray(bad, np.int32).reshape(N))
    n_out = max(N * (nc - 1) * nms_topk, 1)
    d_os, d_ob = DeviceBuffer(max(n_out * 4, 16)), DeviceBuffer(max(n_out * 16, 16))
    check(door(d_p.ptr, d_b.ptr, N, R, nc, d_s.ptr, d_i.ptr, train_image_size, train_image_size, select_threshold, nms_threshold,
               nms_topk, d_bad.ptr if d_bad else None, d_os.ptr, d_ob.ptr, stream.handle if stream else None))
    sc = to_host(d_os.ptr, (N, nc - 1, nms_topk), np.float32, stream)
    bx = to_host(d_ob.ptr, (N, nc - 1, nms_topk, 4), np.float32, stream)
    out = [{k + 1: (sc[n, k], bx[n, k]) for k in range(nc - 1)} for n in range(N)]
    return out[0] if single else out


class Resize(enum.IntEnum):
    """The reference's resizing strategies (preprocessing/common_preprocessing.py:29-32), same names and values."""
    NONE = 1
    CENTRAL_CROP = 2
    PAD_AND_RESIZE = 3
    WARP_RESIZE = 4


def _resize_mode(resize):
    try:
        return Resize(int(resize))
    except (TypeError, ValueError):
        raise InvalidArgumentError(-1, 'resize must be one of %s, got %r' % ([m.name for m in Resize], resize))


def _check_image(img, what='image'):
    """uint8 [H,W,3] with H, W > 0 -- the host-side checks, before any GPU work"""
    a = np.asarray(img)
    if a.ndim != 3:
        raise InvalidArgumentError(-1, '%s: Input must be of size [height, width, C>0], got shape %r' % (what, a.shape))
    if a.shape[2] != 3:
        raise InvalidArgumentError(-1, '%s: 3 channels (RGB) expected, got %d' % (what, a.shape[2]))
    if a.shape[0] == 0 or a.shape[1] == 0:
        raise InvalidArgumentError(-1, '%s: empty image %r' % (what, a.shape))
    if a.dtype != np.uint8:
        raise InvalidArgumentError(-1, '%s: uint8 image expected, got %s' % (what, a.dtype))
    return np.ascontiguousarray(a)


def _check_batch(images, out_size, resize, max_images=None):
    mode = _resize_mode(resize)
    S = int(out_size)
    if S <= 0:
        raise InvalidArgumentError(-1, 'out_size must be > 0, got %d' % S)
    if isinstance(images, np.ndarray) and images.ndim == 3:
        raise InvalidArgumentError(-1, 'a list of [H,W,3] images is expected, got one image')
    imgs = [_check_image(im, 'images[%d]' % i) for i, im in enumerate(images)]
    if not imgs:
        raise InvalidArgumentError(-1, 'no images')
    if max_images is not None and len(imgs) > max_images:
        raise InvalidArgumentError(-1, '%d images but at most %d per call' % (len(imgs), max_images))
    _check_sizes_for_mode([im.shape[:2] for im in imgs], S, mode)
    return imgs, S, mode


def _check_sizes_for_mode(shapes, S, mode, who=''):
    """Resize.NONE takes S x S images only; shapes: (H, W) per image"""
    if mode == Resize.NONE:
        for i, (h, w) in enumerate(shapes):
            if (int(h), int(w)) != (S, S):
                raise InvalidArgumentError(-1, '%simages[%d]: Resize.NONE needs %dx%d images, got %dx%d' % (who, i, S, S, h, w))


def pack_images(images):
    """list of uint8 [H,W,3] -> (packed uint8 bytes, offsets i64 [N], image_shapes i32 [N,2]): the layout of
    xdet_preprocess_eval_batch (include/xdet.h)"""
    sizes = [im.size for im in images]
    offsets = np.zeros(len(images), np.int64)
    offsets[1:] = np.cumsum(sizes)[:-1]
    packed = np.concatenate([im.reshape(-1) for im in images])
    shapes = np.array([im.shape[:2] for im in images], np.int32).reshape(-1, 2)
    return packed, offsets, shapes


def resize_geometry(H, W, S, resize):
    """host side of the resize step: (h, w) entering resize_image_bboxes_with_crop_or_pad and its (crop_y, crop_x,
    pad_y, pad_x, kept_h, kept_w) (common_preprocessing.py:403-418, tf_image.py:261-274); None for WARP / NONE"""
    mode = _resize_mode(resize)
    if mode in (Resize.NONE, Resize.WARP_RESIZE):
        return None
    h, w = H, W
    if mode == Resize.PAD_AND_RESIZE:
        factor = min(np.float64(1.0), min(np.float64(S) / np.float64(H), np.float64(S) / np.float64(W)))
        h, w = int(np.floor(factor * np.float64(H))), int(np.floor(factor * np.float64(W)))
    return (h, w), (max((h - S) // 2, 0), max((w - S) // 2, 0), max((S - h) // 2, 0), max((S - w) // 2, 0),
                    min(S, h), min(S, w))


def bboxes_crop_or_pad(bboxes, height, width, offset_y, offset_x, target_height, target_width):
    """tf_image.bboxes_crop_or_pad (tf_image.py:179-203): f32, b * [h,w,h,w] + offset, / [th,tw,th,tw]"""
    f32 = np.float32
    b = np.asarray(bboxes, f32).reshape(-1, 4)
    b = (b * np.array([height, width, height, width], f32)).astype(f32)
    b = (b + np.array([offset_y, offset_x, offset_y, offset_x], f32)).astype(f32)
    return (b / np.array([target_height, target_width, target_height, target_width], f32)).astype(f32)


def _map_gt_boxes(bboxes, H, W, S, mode):
    b = np.asarray(bboxes, np.float32).reshape(-1, 4)
    geom = resize_geometry(H, W, S, mode)
    if geom is None:
        return b.copy()
    (h, w), (cy, cx, py, px, kh, kw) = geom
    return bboxes_crop_or_pad(bboxes_crop_or_pad(b, h, w, -cy, -cx, kh, kw), kh, kw, py, px, S, S)


def light_head_preprocess_batch(images, out_size, resize=Resize.WARP_RESIZE, stream=None):
    """light_head_preprocess_for_eval's image side for a list of uint8 [H,W,3] images of any sizes, one launch
    (xdet_preprocess_eval_batch) -> (planes f32 [N,3,S,S], bbox_img f32 [N,4], image_shapes i32 [N,2])."""
    imgs, S, mode = _check_batch(images, out_size, resize)
    packed, offsets, shapes = pack_images(imgs)
    N = len(imgs)
    d_p, d_o, d_s = to_device(packed), to_device(offsets), to_device(shapes)
    d_out, d_b = DeviceBuffer(N * 3 * S * S * 4), DeviceBuffer(N * 16)
    check(lib().xdet_preprocess_eval_batch(d_p.ptr, packed.nbytes, d_o.ptr, d_s.ptr, N, S, int(mode), d_out.ptr,
                                           d_b.ptr, stream.handle if stream else None))
    return (to_host(d_out.ptr, (N, 3, S, S), np.float32, stream), to_host(d_b.ptr, (N, 4), np.float32, stream),
            shapes)


def light_head_preprocess_for_eval(image, labels=None, bboxes=None, out_shape=(480, 480), data_format='NHWC',
                                   difficults=None, resize=Resize.WARP_RESIZE, stream=None):
    """preprocessing/common_preprocessing.py:383-440:
    uint8 [H,W,3] -> (image f32 [S,S,3] or [3,S,S], labels, bboxes, bbox_img f32 [4]).
    The image goes through xdet_preprocess_eval_batch; the ground-truth `bboxes` through the same crop / pad as
    bbox_img (on the host, f32 in TF's order), and the boxes and labels flagged in `difficults` are removed (:427-431).
    Resize.NONE needs an S x S image (the network input is S x S)."""
    img = _check_image(np.asarray(image, np.uint8))
    if out_shape[0] != out_shape[1]:
        raise InvalidArgumentError(-1, 'square network input expected, got %r' % (tuple(out_shape),))
    S = int(out_shape[0])
    planes, bbox_img, _ = light_head_preprocess_batch([img], S, resize, stream)
    chw = planes[0]
    out = chw if data_format == 'NCHW' else np.ascontiguousarray(chw.transpose(1, 2, 0))
    if bboxes is not None:
        bboxes = _map_gt_boxes(bboxes, img.shape[0], img.shape[1], S, resize)
    if difficults is not None:
        keep = np.logical_not(np.asarray(difficults).astype(bool)).reshape(-1)
        if labels is not None:
            labels = np.asarray(labels)[keep]
        if bboxes is not None:
            bboxes = bboxes[keep]
    return out, labels, bboxes, bbox_img[0]


def light_head_preprocess_for_test(image, out_shape, data_format='NHWC', resize=Resize.WARP_RESIZE, stream=None):
    """preprocessing/common_preprocessing.py:442-458.  (The reference accepts `resize` here but always warps; this
    applies it -- the default is the same.)"""
    return light_head_preprocess_for_eval(image, None, None, out_shape, data_format, resize=resize, stream=stream)[0]


# the training path's doors (the *_backward ops, batch norm, add_rows, subsample2, add_upsample2) are written in xdet/train_ops.py
from .train_ops import *              # noqa: E402,F401,F403  (their names are this module's too)
