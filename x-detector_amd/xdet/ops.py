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
                           nms_threshold=0.3, nms_topk=200, train_image_size=480, bad=None, stream=None):
    """xdet_bboxes_eval_probs: bboxes_eval from head_decode_probs' outputs, as the whole forward runs it.
    probs [N,num_classes,R] (or [num_classes,R]), bboxes_pred [N*R,4] in any shape, bad: i32 [N] or None
    -> what bboxes_eval returns."""
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
    check(lib().xdet_bboxes_eval_probs(d_p.ptr, d_b.ptr, N, R, nc, d_s.ptr, d_i.ptr, train_image_size, train_image_size,
                                       select_threshold, nms_threshold, nms_topk, d_bad.ptr if d_bad else None, d_os.ptr,
                                       d_ob.ptr, stream.handle if stream else None))
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
    if mode == Resize.NONE:
        for i, im in enumerate(imgs):
            if im.shape[:2] != (S, S):
                raise InvalidArgumentError(-1, 'images[%d]: Resize.NONE needs %dx%d images, got %dx%d'
                                           % (i, S, S, im.shape[0], im.shape[1]))
    return imgs, S, mode


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


def _matrix(a, what):
    """a DeviceTensor ([N,H,W,C] with its ld: N*H*W rows of C) or a 2-D array -> (rows, width, DeviceTensor or f32 array)"""
    if isinstance(a, DeviceTensor):
        return int(np.prod(a.shape[:-1])), int(a.shape[-1]), a
    a = np.ascontiguousarray(a, np.float32)
    if a.ndim != 2:
        raise InvalidArgumentError(-1, 'dense_backward: %s must be a matrix, got shape %r' % (what, a.shape))
    return a.shape[0], a.shape[1], a


def dense_backward_device(x, w, dy, y=None, with_dx=True, stream=None):
    """dense_backward with the results left on the GPU: (dx DeviceTensor [M,1,1,K] or None, dw DeviceBuffer [K,J],
    db DeviceBuffer [J]); nothing is synchronised."""
    M, K, dx_in = _matrix(x, 'x')
    Kw, J, dw_in = _matrix(w, 'w')
    Md, Jd, dy_in = _matrix(dy, 'dy')
    bad = (Kw, Md, Jd) != (K, M, J)
    if y is not None:
        My, Jy, y_in = _matrix(y, 'y')
        bad = bad or (My, Jy) != (M, J)
    if bad:
        raise InvalidArgumentError(-1, 'dense_backward: x [M,K], w [K,J], dy [M,J] and y [M,J] expected, got %r'
                                   % ([(M, K), (Kw, J), (Md, Jd)] + ([(My, Jy)] if y is not None else []),))
    if min(M, K, J) <= 0 or max(K, J) > 4096 or M * max(K, J) >= 2 ** 31:
        raise InvalidArgumentError(-1, 'dense_backward: M = %d, K = %d, J = %d (positive, K and J at most 4096, '
                                       'M * max(K, J) below 2^31)' % (M, K, J))
    if isinstance(dw_in, DeviceTensor) and dw_in.ld != J:
        raise InvalidArgumentError(-1, 'dense_backward: w must be dense on the device (ld %d, J = %d)' % (dw_in.ld, J))

    def dev(a, width):
        if isinstance(a, DeviceTensor):
            return a, a.ptr, a.ld
        b = to_device(a)
        return b, b.ptr, width
    kx, px, ldx = dev(dx_in, K)
    kw, pw, _ = dev(dw_in, J)
    kd, pd, ldd = dev(dy_in, J)
    ky, py, ldy = dev(y_in, J) if y is not None else (None, None, 0)
    d_dx = DeviceTensor.empty((M, 1, 1, K), ld=K) if with_dx else None
    d_dw, d_db = DeviceBuffer(K * J * 4), DeviceBuffer(max(J * 4, 16))
    ws = DeviceBuffer(lib().xdet_dense_backward_workspace_bytes(M, K, J))
    check(lib().xdet_dense_backward(px, ldx, pw, py, ldy, pd, ldd, M, K, J, d_dx.ptr if with_dx else None, K, d_dw.ptr,
                                    d_db.ptr, ws.ptr, stream.handle if stream else None))
    if d_dx is not None:
        d_dx._keep = (kx, kw, kd, ky, ws)      # operands and workspace live until the stream has run the call
    d_dw._keep = (kx, kw, kd, ky, ws)
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
    with_dx=False: dx is None."""
    x, w, dy = np.asarray(x, dtype), np.asarray(w, dtype), np.asarray(dy, dtype)
    N, H, W, C = x.shape
    kh, kw, _, J = w.shape
    g, xe = dy, x
    with np.errstate(invalid='ignore'):
        if y is not None:
            g = np.where(np.asarray(y, dtype) > 0, dy, dtype(0))
        if relu_in:
            xe = np.where(x > 0, x, dtype(0))
    ph, pw = kh // 2, kw // 2
    border = ((0, 0), (ph, ph), (pw, pw), (0, 0))
    xp, gp = np.pad(xe, border), np.pad(g, border)
    g2 = g.reshape(-1, J)
    dw = np.empty(w.shape, dtype)
    dx = np.zeros((N * H * W, C), dtype) if with_dx else None
    for a in range(kh):
        for b in range(kw):
            dw[a, b] = np.matmul(xp[:, a:a + H, b:b + W].reshape(-1, C).T, g2)
            if with_dx:
                dx += np.matmul(gp[:, 2 * ph - a:2 * ph - a + H, 2 * pw - b:2 * pw - b + W].reshape(-1, J), w[a, b].T)
    if with_dx:
        dx = dx.reshape(x.shape)
        if relu_in:
            with np.errstate(invalid='ignore'):
                dx = np.where(x > 0, dx, dtype(0))
    return dx, dw, g2.sum(axis=0, dtype=dtype)


def _nhwc(a, what):
    """a DeviceTensor or a 4-D array -> (shape, DeviceTensor or f32 array)"""
    if isinstance(a, DeviceTensor):
        return tuple(a.shape), a
    a = np.ascontiguousarray(a, np.float32)
    if a.ndim != 4:
        raise InvalidArgumentError(-1, 'conv_backward: %s must have four dimensions, got shape %r' % (what, a.shape))
    return a.shape, a


def _own_dx(dx, shape, who):
    """a caller's gradient tensor (the dx= of the *_backward_device calls): a DeviceTensor of dx's shape, written with its ld"""
    if not isinstance(dx, DeviceTensor) or tuple(dx.shape) != tuple(shape):
        raise InvalidArgumentError(-1, '%s: dx must be a DeviceTensor of shape %r, got %r' % (who, tuple(shape), getattr(dx, 'shape', None)))
    return dx


def conv_backward_device(x, w, dy, y=None, relu_in=False, with_dx=True, stream=None, dx=None, workspace=None):
    """conv_backward with the results left on the GPU: (dx DeviceTensor [N,H,W,C] with x's ld (C for a NumPy x) or None,
    dw DeviceBuffer [kh,kw,C,J], db DeviceBuffer [J]); nothing is synchronised.  A DeviceTensor w is [kh,kw,C,J] dense.
    dx: a DeviceTensor [N,H,W,C] to write instead of a new one (with its ld); workspace: a DeviceBuffer of at least
    xdet_conv_backward_workspace_bytes(N, H, W, C, J, kh, kw) bytes (default: allocated here) -- a chain of calls on one
    stream then allocates no activation-sized memory per call."""
    (N, H, W, C), x_in = _nhwc(x, 'x')
    (kh, kw, Cw, J), w_in = _nhwc(w, 'w')
    sd, dy_in = _nhwc(dy, 'dy')
    bad = Cw != C or sd != (N, H, W, J)
    if y is not None:
        sy, y_in = _nhwc(y, 'y')
        bad = bad or sy != (N, H, W, J)
    if bad:
        raise InvalidArgumentError(-1, 'conv_backward: x [N,H,W,C], w [kh,kw,C,J], dy [N,H,W,J] and y [N,H,W,J] expected, got %r'
                                   % ([(N, H, W, C), (kh, kw, Cw, J), sd] + ([sy] if y is not None else []),))
    M = N * H * W
    if (min(M, C, J, kh, kw) <= 0 or kh % 2 == 0 or kw % 2 == 0 or max(kh, kw) > 15 or max(C, J) > 4096
            or M * max(C, J) >= 2 ** 31):
        raise InvalidArgumentError(-1, 'conv_backward: N*H*W = %d, C = %d, J = %d, kernel %d x %d (sizes positive, kh and kw odd '
                                       'and at most 15, C and J at most 4096, N*H*W * max(C, J) below 2^31)' % (M, C, J, kh, kw))
    if isinstance(w_in, DeviceTensor) and w_in.ld != J:
        raise InvalidArgumentError(-1, 'conv_backward: w must be dense on the device (ld %d, J = %d)' % (w_in.ld, J))

    def dev(a, width):
        if isinstance(a, DeviceTensor):
            return a, a.ptr, a.ld
        b = to_device(a)
        return b, b.ptr, width
    kx, px, ldx = dev(x_in, C)
    kw_, pw, _ = dev(w_in, J)
    kd, pd, ldd = dev(dy_in, J)
    ky, py, ldy = dev(y_in, J) if y is not None else (None, None, 0)
    d_dx = None
    if with_dx:
        d_dx = _own_dx(dx, (N, H, W, C), 'conv_backward') if dx is not None else DeviceTensor.empty((N, H, W, C), ld=ldx)
    d_dw, d_db = DeviceBuffer(kh * kw * C * J * 4), DeviceBuffer(max(J * 4, 16))
    ws = workspace if workspace is not None else DeviceBuffer(lib().xdet_conv_backward_workspace_bytes(N, H, W, C, J, kh, kw))
    check(lib().xdet_conv_backward(px, ldx, pw, py, ldy, pd, ldd, N, H, W, C, J, kh, kw, 1 if relu_in else 0,
                                   d_dx.ptr if with_dx else None, d_dx.ld if with_dx else ldx, d_dw.ptr, d_db.ptr, ws.ptr,
                                   stream.handle if stream else None))
    if d_dx is not None:
        d_dx._keep = (kx, kw_, kd, ky, ws)     # operands and workspace live until the stream has run the call
    d_dw._keep = (kx, kw_, kd, ky, ws)
    return d_dx, d_dw, d_db


def conv_backward(x, w, dy, y=None, relu_in=False, with_dx=True, stream=None):
    """host_conv_backward on the GPU (xdet_conv_backward): x [N,H,W,C], w [kh,kw,C,J], dy [N,H,W,J], y [N,H,W,J] or None as
    NumPy arrays or DeviceTensors (read in place with their ld) -> (dx [N,H,W,C] or None, dw [kh,kw,C,J], db [J]) as NumPy
    arrays."""
    d_dx, d_dw, d_db = conv_backward_device(x, w, dy, y, relu_in, with_dx, stream)
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


def _bn_rows(a, what):
    """a DeviceTensor ([N,H,W,C] with its ld) or an array [..., C] -> (shape, M, C, DeviceTensor or f32 array)"""
    if isinstance(a, DeviceTensor):
        return tuple(a.shape), int(np.prod(a.shape[:-1])), int(a.shape[-1]), a
    a = np.ascontiguousarray(a, np.float32)
    if a.ndim < 2:
        raise InvalidArgumentError(-1, 'batch_norm: %s must have rows of channels, got shape %r' % (what, a.shape))
    return a.shape, int(np.prod(a.shape[:-1])), a.shape[-1], a


def _bn_vec(a, C, what):
    """a [C] vector: a DeviceBuffer / DeviceTensor stays, anything else is copied to the device -> (keep-alive, pointer)"""
    if isinstance(a, (DeviceBuffer, DeviceTensor)):
        return a, a.ptr
    a = np.ascontiguousarray(a, np.float32).reshape(-1)
    if a.shape[0] != C:
        raise InvalidArgumentError(-1, 'batch_norm: %s must hold %d values, got %d' % (what, C, a.shape[0]))
    b = to_device(a)
    return b, b.ptr


def _bn_check_sizes(M, C, who):
    if min(M, C) <= 0 or C > 4096 or M * C >= 2 ** 31:
        raise InvalidArgumentError(-1, '%s: M = %d, C = %d (positive, C at most 4096, M * C below 2^31)' % (who, M, C))


def _bn_dev(a, C):
    if isinstance(a, DeviceTensor):
        return a, a.ptr, a.ld
    b = to_device(a)
    return b, b.ptr, C


def batch_norm_forward_device(x, gamma, beta, eps, training=True, momentum=0.997, moving_mean=None, moving_var=None,
                              relu=False, stream=None):
    """batch_norm_forward with the results left on the GPU: (y DeviceTensor with x's shape and ld (C for a NumPy x), save_mean,
    save_invstd, moving_mean, moving_var as DeviceBuffers [C]; the moving ones None when none were given); nothing is
    synchronised.  Moving statistics given as DeviceBuffers are updated in place (training) and returned; NumPy ones are
    copied to the device first."""
    shape, M, C, x_in = _bn_rows(x, 'x')
    _bn_check_sizes(M, C, 'batch_norm_forward')
    if (moving_mean is None) != (moving_var is None) or (not training and moving_mean is None):
        raise InvalidArgumentError(-1, 'batch_norm_forward: training=False needs both moving statistics; training mode takes '
                                       'both or neither')
    kx, px, ldx = _bn_dev(x_in, C)
    kg, pg = _bn_vec(gamma, C, 'gamma')
    kb, pb = _bn_vec(beta, C, 'beta')
    d_mm, pmm = _bn_vec(moving_mean, C, 'moving_mean') if moving_mean is not None else (None, None)
    d_mv, pmv = _bn_vec(moving_var, C, 'moving_var') if moving_var is not None else (None, None)
    d_y = DeviceTensor.empty(shape if len(shape) == 4 else (M, 1, 1, C), ld=ldx)
    d_mean, d_inv = DeviceBuffer(max(C * 4, 16)), DeviceBuffer(max(C * 4, 16))
    ws = DeviceBuffer(lib().xdet_batch_norm_workspace_bytes(M, C))
    check(lib().xdet_batch_norm_forward(px, ldx, M, C, pg, pb, float(eps), 1 if training else 0, float(momentum), pmm, pmv,
                                        1 if relu else 0, d_y.ptr, d_y.ld, d_mean.ptr, d_inv.ptr, ws.ptr,
                                        stream.handle if stream else None))
    d_mean._keep = (kx, kg, kb, ws, d_y)         # operands and workspace live until the stream has run the call
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
    shape, M, C, x_in = _bn_rows(x, 'x')
    sd, Md, Cd, dy_in = _bn_rows(dy, 'dy')
    bad = (Md, Cd) != (M, C)
    if y is not None:
        sy, My, Cy, y_in = _bn_rows(y, 'y')
        bad = bad or (My, Cy) != (M, C)
    if bad:
        raise InvalidArgumentError(-1, 'batch_norm_backward: x, dy and y of one shape expected, got %r'
                                   % ([shape, sd] + ([sy] if y is not None else []),))
    _bn_check_sizes(M, C, 'batch_norm_backward')
    kx, px, ldx = _bn_dev(x_in, C)
    kd, pd, ldd = _bn_dev(dy_in, C)
    ky, py, ldy = _bn_dev(y_in, C) if y is not None else (None, None, 0)
    kg, pg = _bn_vec(gamma, C, 'gamma')
    km, pm = _bn_vec(save_mean, C, 'save_mean')
    ki, pi = _bn_vec(save_invstd, C, 'save_invstd')
    d_dx = None
    if with_dx:
        shape4 = shape if len(shape) == 4 else (M, 1, 1, C)
        d_dx = _own_dx(dx, shape4, 'batch_norm_backward') if dx is not None else DeviceTensor.empty(shape4, ld=ldx)
    d_dg, d_db = DeviceBuffer(max(C * 4, 16)), DeviceBuffer(max(C * 4, 16))
    ws = workspace if workspace is not None else DeviceBuffer(lib().xdet_batch_norm_workspace_bytes(M, C))
    check(lib().xdet_batch_norm_backward(px, ldx, py, ldy, pd, ldd, M, C, pg, pm, pi, 1 if training else 0,
                                         d_dx.ptr if with_dx else None, d_dx.ld if with_dx else ldx, d_dg.ptr, d_db.ptr, ws.ptr,
                                         stream.handle if stream else None))
    d_dg._keep = (kx, kd, ky, kg, km, ki, ws)    # operands and workspace live until the stream has run the call
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
    (N, H, W, C), x_in = _nhwc(x, 'x')
    sk, k_in = _nhwc(k, 'k')
    sd, dy_in = _nhwc(dy, 'dy')
    if tuple(sk) != (3, 3, C, 1) or tuple(sd) != (N, H, W, C):
        raise InvalidArgumentError(-1, 'depthwise_backward: x [N,H,W,C], k [3,3,C,1] and dy [N,H,W,C] expected, got %r'
                                   % ([(N, H, W, C), tuple(sk), tuple(sd)],))
    M = N * H * W
    if min(M, C) <= 0 or C > 4096 or M * C >= 2 ** 31 or dilation not in (1, 2):
        raise InvalidArgumentError(-1, 'depthwise_backward: N*H*W = %d, C = %d, dilation %r (sizes positive, C at most 4096, '
                                       'N*H*W * C below 2^31, dilation 1 or 2)' % (M, C, dilation))
    if isinstance(k_in, DeviceTensor) and k_in.ld != 1:
        raise InvalidArgumentError(-1, 'depthwise_backward: k must be dense on the device (ld %d)' % k_in.ld)

    def dev(a, width):
        if isinstance(a, DeviceTensor):
            return a, a.ptr, a.ld
        b = to_device(a)
        return b, b.ptr, width
    kx, px, ldx = dev(x_in, C)
    kk, pk, _ = dev(k_in, 1)
    kd, pd, ldd = dev(dy_in, C)
    d_dx = None
    if with_dx:
        d_dx = _own_dx(dx, (N, H, W, C), 'depthwise_backward') if dx is not None else DeviceTensor.empty((N, H, W, C), ld=ldx)
    d_dw = DeviceBuffer(max(9 * C * 4, 16))
    ws = workspace if workspace is not None else DeviceBuffer(lib().xdet_depthwise_backward_workspace_bytes(N, H, W, C))
    check(lib().xdet_depthwise_backward(px, ldx, pk, pd, ldd, N, H, W, C, int(dilation), 1 if relu_in else 0,
                                        d_dx.ptr if with_dx else None, d_dx.ld if with_dx else ldx, d_dw.ptr, ws.ptr,
                                        stream.handle if stream else None))
    if d_dx is not None:
        d_dx._keep = (kx, kk, kd, ws)          # operands and workspace live until the stream has run the call
    d_dw._keep = (kx, kk, kd, ws)
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
    copied to the device first); out: a DeviceTensor of that shape -- it may be a itself -- or None: a new one with a's ld.
    -> out; nothing is synchronised."""
    sa, a_in = _nhwc(a, 'a')
    sb, b_in = _nhwc(b, 'b')
    if tuple(sa) != tuple(sb) or (out is not None and (not isinstance(out, DeviceTensor) or tuple(out.shape) != tuple(sa))):
        raise InvalidArgumentError(-1, 'add_rows: a, b and out of one shape expected, got %r'
                                   % ([tuple(sa), tuple(sb), getattr(out, 'shape', None)],))
    M, C = int(np.prod(sa[:3])), int(sa[3])
    if min(M, C) <= 0 or M * C >= 2 ** 31:
        raise InvalidArgumentError(-1, 'add_rows: %d rows of %d channels (positive, their product below 2^31)' % (M, C))
    ta = a_in if isinstance(a_in, DeviceTensor) else DeviceTensor.from_numpy(a_in)
    tb = b_in if isinstance(b_in, DeviceTensor) else DeviceTensor.from_numpy(b_in)
    if out is None:
        out = DeviceTensor.empty(sa, ld=ta.ld)
    check(lib().xdet_add_rows(ta.ptr, ta.ld, tb.ptr, tb.ld, out.ptr, out.ld, M, C, stream.handle if stream else None))
    # operands live until the stream has run the call (on top of what out already keeps alive)
    out._keep = (getattr(out, '_keep', None),) + tuple(t for t in (ta, tb) if t is not out)
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


def _pool_sizes(who, N, H, W, C):
    if min(N, H, W, C) <= 0 or C > 4096 or N * H * W * C >= 2 ** 31:
        raise InvalidArgumentError(-1, '%s: [%d,%d,%d,%d] (sizes positive, C at most 4096, N*H*W*C below 2^31)' % (who, N, H, W, C))


def _pool_dev(a):
    return a if isinstance(a, DeviceTensor) else DeviceTensor.from_numpy(a)


def max_pool_backward_device(x, dy, dx=None, stream=None):
    """max_pool_backward with the result left on the GPU: dx DeviceTensor [N,H,W,C] with x's ld (C for a NumPy x); nothing is
    synchronised.  x, dy: NumPy arrays or DeviceTensors read in place with their ld.  dx: a DeviceTensor [N,H,W,C] to write
    instead of a new one (with its ld; it must not overlap x or dy)."""
    (N, H, W, C), x_in = _nhwc(x, 'x')
    sd, dy_in = _nhwc(dy, 'dy')
    if tuple(sd) != (N, -(-H // 2), -(-W // 2), C):
        raise InvalidArgumentError(-1, 'max_pool_backward: x [N,H,W,C] and dy [N,ceil(H/2),ceil(W/2),C] expected, got %r'
                                   % ([(N, H, W, C), tuple(sd)],))
    _pool_sizes('max_pool_backward', N, H, W, C)
    tx, td = _pool_dev(x_in), _pool_dev(dy_in)
    d_dx = _own_dx(dx, (N, H, W, C), 'max_pool_backward') if dx is not None else DeviceTensor.empty((N, H, W, C), ld=tx.ld)
    check(lib().xdet_maxpool3x3s2_backward(tx.ptr, tx.ld, td.ptr, td.ld, N, H, W, C, d_dx.ptr, d_dx.ld,
                                           stream.handle if stream else None))
    d_dx._keep = (tx, td)                      # operands live until the stream has run the call
    return d_dx


def max_pool_backward(x, dy, stream=None):
    """host_max_pool_backward on the GPU (xdet_maxpool3x3s2_backward) -> dx [N,H,W,C] as a NumPy array"""
    d_dx = max_pool_backward_device(x, dy, stream=stream)
    synchronize(stream)
    return d_dx.numpy(stream=stream)


def subsample2_device(x, out=None, stream=None):
    """host_subsample2 on the GPU (xdet_subsample2): x [N,H,W,C] as a NumPy array or a DeviceTensor read with its ld -> out
    DeviceTensor [N,ceil(H/2),ceil(W/2),C] (a caller's, written with its ld, or a new dense one); nothing is synchronised."""
    (N, H, W, C), x_in = _nhwc(x, 'x')
    so = (N, -(-H // 2), -(-W // 2), C)
    if out is not None and (not isinstance(out, DeviceTensor) or tuple(out.shape) != so):
        raise InvalidArgumentError(-1, 'subsample2: out must be a DeviceTensor of shape %r, got %r' % (so, getattr(out, 'shape', None)))
    _pool_sizes('subsample2', N, H, W, C)
    tx = _pool_dev(x_in)
    if out is None:
        out = DeviceTensor.empty(so)
    check(lib().xdet_subsample2(tx.ptr, tx.ld, N, H, W, C, out.ptr, out.ld, stream.handle if stream else None))
    out._keep = (tx,)
    return out


def add_upsample2_device(a, b, out=None, stream=None):
    """host_add_upsample2 on the GPU (xdet_add_upsample2): a [N,H,W,C], b [N,ceil(H/2),ceil(W/2),C], each read with its own ld
    (NumPy arrays are copied to the device first); out: a DeviceTensor of a's shape -- it may be a itself -- or None: a new
    one with a's ld.  -> out; nothing is synchronised."""
    (N, H, W, C), a_in = _nhwc(a, 'a')
    sb, b_in = _nhwc(b, 'b')
    if tuple(sb) != (N, -(-H // 2), -(-W // 2), C) or (out is not None and (not isinstance(out, DeviceTensor)
                                                                             or tuple(out.shape) != (N, H, W, C))):
        raise InvalidArgumentError(-1, 'add_upsample2: a [N,H,W,C], b [N,ceil(H/2),ceil(W/2),C] and out like a expected, got %r'
                                   % ([(N, H, W, C), tuple(sb), getattr(out, 'shape', None)],))
    _pool_sizes('add_upsample2', N, H, W, C)
    ta, tb = _pool_dev(a_in), _pool_dev(b_in)
    if out is None:
        out = DeviceTensor.empty((N, H, W, C), ld=ta.ld)
    check(lib().xdet_add_upsample2(ta.ptr, ta.ld, tb.ptr, tb.ld, N, H, W, C, out.ptr, out.ld, stream.handle if stream else None))
    out._keep = (getattr(out, '_keep', None),) + tuple(t for t in (ta, tb) if t is not out)
    return out
