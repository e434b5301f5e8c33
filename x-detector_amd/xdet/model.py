"""The Light-Head R-CNN eval graph behind the reference's graph-builder API.

`LightHeadDetector` owns the native net (weights + workspace); the module-level
functions carry the reference's names and argument order (net/xception_body.py:236,
381,402,450,477) and operate on the detector that is current (`with det.scope():`,
the counterpart of `tf.variable_scope(params['model_scope'])`,
light_head_rfcn_eval.py:382).  Tensors are DeviceTensor views of the net's workspace.
"""
import contextlib
import ctypes

import numpy as np

from ._lib import lib, check, c_void_p, LightHeadConfig, XdetError, InvalidArgumentError
from .runtime import DeviceBuffer, DeviceTensor, Stream, to_device, to_host, synchronize, _host

_current = []

LARGE_SEP_VARIABLES = tuple('large_sep_feature/%s/%s/%s' % (br, conv, v) for br in ('Branch_0', 'Branch_1')
                            for conv in ('conv2d', 'conv2d_1') for v in ('kernel', 'bias')) + \
    ('large_sep_feature/batch_normalization/gamma', 'large_sep_feature/batch_normalization/beta')
LARGE_SEP_MOVING = ('large_sep_feature/batch_normalization/moving_mean', 'large_sep_feature/batch_normalization/moving_variance')
LARGE_SEP_EPS, LARGE_SEP_MOMENTUM = 1e-5, 0.997        # net/resnet_v2.py: _BATCH_NORM_EPSILON, _BATCH_NORM_DECAY

# the Xception exit flow (net/xception_body.py:339-376): four separable units (name, dilation, ReLU in front of the depthwise
# conv, ReLU behind the batch norm) and the 1x1 projection of the residual branch
EXIT_FLOW_UNITS = (('block13_sepconv1', 1, True, False), ('block13_sepconv2', 1, True, False),
                   ('block14_sepconv1', 2, False, True), ('block14_sepconv2', 2, False, True))
EXIT_FLOW_BNS = tuple(u[0] + '_bn' for u in EXIT_FLOW_UNITS) + ('batch_normalization_4',)
EXIT_FLOW_VARIABLES = tuple('%s/%s' % (u[0], v) for u in EXIT_FLOW_UNITS for v in ('depthwise_kernel', 'pointwise_kernel')) + \
    ('conv2d_4/kernel',) + tuple('%s/%s' % (b, v) for b in EXIT_FLOW_BNS for v in ('gamma', 'beta'))
EXIT_FLOW_MOVING = tuple('%s/%s' % (b, v) for b in EXIT_FLOW_BNS for v in ('moving_mean', 'moving_variance'))
EXIT_FLOW_EPS, EXIT_FLOW_MOMENTUM = 1e-4, 0.99         # net/xception_body.py: the Xception layers' batch norm

# the Xception middle flow (net/xception_body.py:328-337): eight blocks of three relu -> separable 3x3 -> BN units at 728
# channels, each block closed by a residual add of its input
MIDDLE_FLOW_BLOCKS = tuple(range(5, 13))
MIDDLE_FLOW_UNITS = tuple('block%d_sepconv%d' % (b, i) for b in MIDDLE_FLOW_BLOCKS for i in (1, 2, 3))
MIDDLE_FLOW_VARIABLES = tuple(u + v for u in MIDDLE_FLOW_UNITS for v in ('/depthwise_kernel', '/pointwise_kernel', '_bn/gamma', '_bn/beta'))
MIDDLE_FLOW_MOVING = tuple(u + v for u in MIDDLE_FLOW_UNITS for v in ('_bn/moving_mean', '_bn/moving_variance'))
MIDDLE_FLOW_EPS, MIDDLE_FLOW_MOMENTUM = EXIT_FLOW_EPS, EXIT_FLOW_MOMENTUM

# blocks 2-4 of the Xception entry flow (net/xception_body.py:260-326): a 1x1 / stride-2 projection with its batch norm, two
# (relu ->) separable 3x3 -> BN units, max_pooling2d(3, 2, 'same') and the residual add; block 2's first unit has no ReLU in
# front (its input is the stem's ReLU output)
ENTRY_FLOW_BLOCKS = (2, 3, 4)
ENTRY_FLOW_UNITS = tuple('block%d_sepconv%d' % (b, i) for b in ENTRY_FLOW_BLOCKS for i in (1, 2))


def _entry_block_variables(b):
    return ('conv2d_%d/kernel' % (b - 1), 'batch_normalization_%d/gamma' % (b - 1), 'batch_normalization_%d/beta' % (b - 1)) + \
        tuple('block%d_sepconv%d%s' % (b, i, v) for i in (1, 2) for v in ('/depthwise_kernel', '/pointwise_kernel', '_bn/gamma', '_bn/beta'))


ENTRY_FLOW_VARIABLES = tuple(v for b in ENTRY_FLOW_BLOCKS for v in _entry_block_variables(b))
ENTRY_FLOW_MOVING = tuple('%s/%s' % (bn, v) for b in ENTRY_FLOW_BLOCKS
                          for bn in ('batch_normalization_%d' % (b - 1), 'block%d_sepconv1_bn' % b, 'block%d_sepconv2_bn' % b)
                          for v in ('moving_mean', 'moving_variance'))
ENTRY_FLOW_EPS, ENTRY_FLOW_MOMENTUM = EXIT_FLOW_EPS, EXIT_FLOW_MOMENTUM


def _entry_relu_in(b, i):
    return not (b == 2 and i == 1)


def merge_large_sep(weights, dtype=np.float32):
    """The large-separable block's two branches as one conv pair (net/xception_body.py:450-475; the same fusion as the
    native net's, without the BN fold): both (15,1) convs read the same input -> one kernel [15,1,cin,2*mid] with the
    branches side by side along the outputs and the bias [2*mid]; branch_0b + branch_1b -> one (1,15) kernel [1,15,2*mid,co]
    with the branches stacked along the inputs and the bias b0 + b1.  -> (K_a, b_a, K_b, b_b)"""
    g = lambda br, name: np.asarray(weights['large_sep_feature/%s/%s' % (br, name)], dtype)
    ka = np.ascontiguousarray(np.concatenate([g('Branch_0', 'conv2d/kernel'), g('Branch_1', 'conv2d/kernel')], axis=3))
    ba = np.concatenate([g('Branch_0', 'conv2d/bias'), g('Branch_1', 'conv2d/bias')])
    kb = np.ascontiguousarray(np.concatenate([g('Branch_0', 'conv2d_1/kernel'), g('Branch_1', 'conv2d_1/kernel')], axis=2))
    return ka, ba, kb, g('Branch_0', 'conv2d_1/bias') + g('Branch_1', 'conv2d_1/bias')


def split_large_sep_grads(d_ka, d_ba, d_kb, d_bb, mid):
    """merge_large_sep's adjoint: the gradients of the merged tensors -> the eight conv gradients under the checkpoint's names
    and in its shapes.  Both conv2d_1 biases enter the block as b0 + b1, so both get d_bb."""
    out = {}
    for i, br in enumerate(('Branch_0', 'Branch_1')):
        p, sl = 'large_sep_feature/%s/' % br, slice(i * mid, (i + 1) * mid)
        out[p + 'conv2d/kernel'] = np.ascontiguousarray(d_ka[..., sl])
        out[p + 'conv2d/bias'] = np.ascontiguousarray(d_ba[sl])
        out[p + 'conv2d_1/kernel'] = np.ascontiguousarray(d_kb[:, :, sl, :])
        out[p + 'conv2d_1/bias'] = np.array(d_bb)
    return out


# ---- one `(relu ->) separable 3x3 -> BN (-> relu)` unit in training mode: what the exit flow and the middle flow share ----

def _dense(k):
    """a kernel as the checkpoint stores it -> a dense DeviceTensor (the w / k operand of the backward ops)"""
    b = to_device(k)
    return DeviceTensor(b.ptr, k.shape, k.shape[3], owner=b)


def _bn_state(weights, name, co):
    """a batch norm's vectors on the device: gamma, beta, the moving statistics (updated in place by a training forward) and
    room for the batch statistics"""
    vec = lambda k: to_device(np.ascontiguousarray(weights[name + '/' + k], np.float32))
    return {'gamma': vec('gamma'), 'beta': vec('beta'), 'moving_mean': vec('moving_mean'), 'moving_variance': vec('moving_variance'),
            'save_mean': DeviceBuffer(co * 4), 'save_invstd': DeviceBuffer(co * 4)}


def _pointwise_layers(weights, names):
    """{name: the 1x1 conv of <name>/pointwise_kernel in split precision, f32 out, no scale or shift}"""
    from . import ops
    from .runtime import get_precision, set_precision
    before = get_precision()
    set_precision('f16x3')
    try:
        return {n: ops.Conv2D(np.ascontiguousarray(weights[n + '/pointwise_kernel'], np.float32)) for n in names}
    finally:
        set_precision(before)


def _build_unit(weights, name, dil, relu_in, relu_out, pw, B, H, W, own_y):
    """the depthwise layer, the pointwise conv `pw`, both kernels as dense device tensors for the backward, the BN vectors and
    the tensors a training forward keeps: 't' (the depthwise output), 'z' (the BN input) and, with own_y, 'y' (the BN output)"""
    from . import ops
    kd = np.ascontiguousarray(weights[name + '/depthwise_kernel'], np.float32)
    kp = np.ascontiguousarray(weights[name + '/pointwise_kernel'], np.float32)
    C, J = kp.shape[2], kp.shape[3]
    u = {'name': name, 'dil': dil, 'relu_in': relu_in, 'relu_out': relu_out, 'dw': ops.DepthwiseConv2D(kd, dil), 'pw': pw,
         'K_dw': _dense(kd), 'K_pw': _dense(kp), 'bn': _bn_state(weights, name + '_bn', J),
         't': DeviceTensor.empty((B, H, W, C)), 'z': DeviceTensor.empty((B, H, W, J))}
    if own_y:
        u['y'] = DeviceTensor.empty((B, H, W, J))
    return u


def _bn_train_forward(d, b, z, relu, y, M, ws, eps=EXIT_FLOW_EPS, momentum=EXIT_FLOW_MOMENTUM):
    check(lib().xdet_batch_norm_forward(z.ptr, z.ld, M, z.shape[3], b['gamma'].ptr, b['beta'].ptr, eps, 1, momentum,
                                        b['moving_mean'].ptr, b['moving_variance'].ptr, 1 if relu else 0, y.ptr, y.ld,
                                        b['save_mean'].ptr, b['save_invstd'].ptr, ws.ptr, d.stream.handle))


def _unit_forward(d, u, x, y, n, H, W, ws_bn):
    """y = (relu)(BN(pw(dw((relu)(x))))) with batch statistics, t and z kept in the unit: three calls on the detector's stream"""
    t, z, h = u['t'], u['z'], d.stream.handle
    check(lib().xdet_depthwise_forward(u['dw'].handle, x.ptr, n, H, W, x.ld, t.ptr, 1 if u['relu_in'] else 0, h))
    check(lib().xdet_conv_forward(u['pw'].handle, t.ptr, n, H, W, t.ld, z.ptr, z.ld, None, 0, h))
    _bn_train_forward(d, u['bn'], z, u['relu_out'], y, n * H * W, ws_bn)


def _unit_backward(d, u, x, y, dy, z, t, dev, ws_dw, into=None):
    """d loss / d y -> d loss / d x through the unit's BN (masked by y, the unit's own output, where it ends in a ReLU; None
    otherwise), the 1x1 conv (its bias gradient computed and dropped: the conv has none) and the depthwise conv: three calls
    on the detector's stream.  z, t: the kept BN input and depthwise output; dev: gains the four weight gradients as
    (DeviceBuffer, shape) under the checkpoint's names.  into: {'dz', 'dt', 'dx': DeviceTensors to write, 'ws_bn', 'ws_conv':
    workspaces} -- without it every call allocates its own.  -> (dx, dt, dz)"""
    from . import ops
    into = into or {}
    name, b = u['name'], u['bn']
    dz, dgamma, dbeta = ops.batch_norm_backward_device(z, y, dy, b['gamma'], b['save_mean'], b['save_invstd'], True, stream=d.stream,
                                                       dx=into.get('dz'), workspace=into.get('ws_bn'))
    dt, dkp, _ = ops.conv_backward_device(t, u['K_pw'], dz, None, stream=d.stream, dx=into.get('dt'), workspace=into.get('ws_conv'))
    dx, dkd = ops.depthwise_backward_device(x, u['K_dw'], dt, u['dil'], u['relu_in'], stream=d.stream, workspace=ws_dw,
                                            dx=into.get('dx'))
    J = u['K_pw'].shape[3]
    dev[name + '/depthwise_kernel'], dev[name + '/pointwise_kernel'] = (dkd, u['K_dw'].shape), (dkp, u['K_pw'].shape)
    dev[name + '_bn/gamma'], dev[name + '_bn/beta'] = (dgamma, (J,)), (dbeta, (J,))
    return dx, dt, dz


def _bn_views(out, name, b):
    co = b['save_mean'].nbytes // 4
    for k in ('save_mean', 'save_invstd', 'moving_mean', 'moving_variance'):
        out['%s/%s' % (name, k)] = DeviceTensor(b[k].ptr, (1, 1, 1, co), co, owner=b[k])


class LightHeadDetector(object):
    def __init__(self, weights, image_size=480, max_batch=1, num_classes=21, rpn_pre_nms_top_n=5000,
                 rpn_post_nms_top_n=1000, rpn_nms_thres=0.7, rpn_min_size=None, select_threshold=0.01,
                 nms_threshold=0.3, nms_topk=200, device=None, large_sep='auto', sepconv='fused', rpn_stream='side',
                 conv3x3='patch', pool='split', check_range=False, ksplit=True, cross='f16', workspace=None, pool_sub=None,
                 pool_index=False, rpn_hidden=False, large_sep_train=False, exit_flow_train=False, middle_flow_train=False,
                 entry_flow_train=False):
        """check_range=True: every activation tensor is validated against the f16 range of the split-precision convs
        after each forward (|x| <= 65504, no NaN); a violation raises in detections() / forward().  For validating a
        new checkpoint once: the pass re-reads every activation (~+30 % time).
        workspace='reuse' (default) | 'ssa': dead tensors' workspace blocks are handed to later tensors of the same size, or
        every tensor keeps its own block (check_range=True selects 'ssa' by itself); memory() reports both figures.
        cross='fp8': the cross terms of the split-precision products of the depthwise -> pointwise layers (28 of the 46
        contractions, the dominant ones) are computed from fp8 copies of the operands (the "x8" form, include/xdet.h) -- once
        calibrate() has measured the tensors; until then, and with 'f16', everything is f16x3.
        pool_index=True: the head's PsRoiAlign keeps its argmax sample ids (buffer 'pool_index'), which
        head_backward(..., to_feat=True) needs; the default forward writes none and allocates nothing for them.
        rpn_hidden=True: rpn_head/conv2d keeps its f32 output (buffer 'rpn_hidden'), which rpn_backward needs; the default
        forward writes only the split planes the 1x1 heads read.
        large_sep_train=True: the ten large_sep_feature/ variables are kept as the checkpoint stores them, unfolded, and the
        block's two merged kernels, biases, gamma, beta and moving statistics are put on the device:
        large_sep_kernel(..., is_training=True) then runs the block with batch statistics (xdet_batch_norm_forward) and
        large_sep_backward takes the gradient through it.  The default detector keeps none of this and allocates nothing for
        it; is_training=False is the same forward either way.
        exit_flow_train=True (needs large_sep_train=True: a training-mode `out` is consumed by the training-mode block): the
        exit flow's 19 variables (EXIT_FLOW_VARIABLES) and the moving statistics of its five batch norms are kept unfolded on
        the device, with the tensors a training forward saves and the workspaces, all sized for max_batch:
        model.exit_flow_train() then recomputes the exit flow from `mid_x` with batch statistics into the net's `out`, and
        model.exit_flow_backward takes the gradient through it down to `mid_x`.  The default detector allocates and runs none
        of this.
        middle_flow_train=True (needs exit_flow_train=True: the training-mode `mid_x` it writes is consumed by the training-mode
        exit flow): the net keeps the middle flow's input (option "entry_x", buffer 'entry_x'), and the 96 variables of the 24
        units of blocks 5-12 (MIDDLE_FLOW_VARIABLES) and their moving statistics are kept unfolded on the device with the 72
        tensors a training forward saves (9 per block: t and z of each unit, y1, y2, the block output; ~189 MB per image at
        480 pixels): model.middle_flow_train() recomputes `mid_x` from `entry_x` with batch statistics and refreshes what the
        net derived from it, model.middle_flow_backward takes the gradient from `mid_x` down to `entry_x`.  The default detector
        allocates and runs none of this.
        entry_flow_train=True (needs middle_flow_train=True: the training-mode `entry_x` it writes is consumed by the
        training-mode middle flow): the net keeps the stem's output (option "stem_out", buffer 'stem_out'), and the 33 variables
        of blocks 2-4 (ENTRY_FLOW_VARIABLES) and the moving statistics of their nine batch norms are kept unfolded on the device
        with the tensors a training forward saves (per block the subsampled input xs, the projection's z and r, t, z and y of
        both units and the block's output), the workspaces and the gradient tensors the backward writes, all sized for
        max_batch: model.entry_flow_train() recomputes `entry_x` from `stem_out` with batch statistics,
        model.entry_flow_backward takes the gradient from `entry_x` down to `stem_out`.  The default detector allocates and runs
        none of this."""
        if entry_flow_train and not middle_flow_train:
            raise InvalidArgumentError(-1, 'entry_flow_train=True needs middle_flow_train=True (the training-mode `entry_x` it '
                                           'writes is consumed by the middle flow in training mode)')
        if entry_flow_train:
            miss = [k for k in ENTRY_FLOW_VARIABLES + ENTRY_FLOW_MOVING if k not in weights]
            if miss:
                raise InvalidArgumentError(-1, 'entry_flow_train: the weights lack %s' % ', '.join(miss))
        if middle_flow_train and not exit_flow_train:
            raise InvalidArgumentError(-1, 'middle_flow_train=True needs exit_flow_train=True (the training-mode `mid_x` it writes '
                                           'is consumed by the exit flow in training mode)')
        if middle_flow_train:
            miss = [k for k in MIDDLE_FLOW_VARIABLES + MIDDLE_FLOW_MOVING if k not in weights]
            if miss:
                raise InvalidArgumentError(-1, 'middle_flow_train: the weights lack %s' % ', '.join(miss))
        if exit_flow_train and not large_sep_train:
            raise InvalidArgumentError(-1, 'exit_flow_train=True needs large_sep_train=True (the training-mode `out` it writes is '
                                           'consumed by the large-separable block in training mode)')
        if exit_flow_train:                      # (ahead of the native net, which would miss them under another error)
            miss = [k for k in EXIT_FLOW_VARIABLES + EXIT_FLOW_MOVING if k not in weights]
            if miss:
                raise InvalidArgumentError(-1, 'exit_flow_train: the weights lack %s' % ', '.join(miss))
        if device is not None:
            check(lib().xdet_set_device(int(device)))
        self.cfg = LightHeadConfig(image_size=image_size, max_batch=max_batch, num_classes=num_classes,
                                   rpn_pre_nms_top_n=rpn_pre_nms_top_n, rpn_post_nms_top_n=rpn_post_nms_top_n,
                                   rpn_nms_thres=rpn_nms_thres,
                                   rpn_min_size=(16. / 480) if rpn_min_size is None else rpn_min_size,   # flag default, eval.py:112
                                   select_threshold=select_threshold, nms_threshold=nms_threshold, nms_topk=nms_topk)
        h = c_void_p()
        check(lib().xdet_net_create(ctypes.byref(h), ctypes.byref(self.cfg)))
        self.handle = h
        self._head_kernels = {}            # the dense layers' kernels as the checkpoint stores them (head_backward)
        self._rpn_kernels = {}             # ... and the RPN head's three (rpn_backward)
        for name, arr in weights.items():
            a = np.ascontiguousarray(arr, np.float32)
            if name in ('final_head/subnet_fc/kernel', 'final_head/fc_cls/kernel', 'final_head/fc_loc/kernel'):
                self._head_kernels[name] = a
            if rpn_hidden and name in ('rpn_head/conv2d/kernel', 'rpn_head/conv2d_1/kernel', 'rpn_head/conv2d_2/kernel'):
                self._rpn_kernels[name] = a
            dims = (ctypes.c_int64 * a.ndim)(*a.shape)
            check(lib().xdet_net_set_weight(self.handle, name.encode(), _host(a), a.ndim, dims))
        check(lib().xdet_net_set_option(self.handle, b'large_sep', large_sep.encode()))
        check(lib().xdet_net_set_option(self.handle, b'sepconv', sepconv.encode()))
        check(lib().xdet_net_set_option(self.handle, b'rpn_stream', rpn_stream.encode()))
        check(lib().xdet_net_set_option(self.handle, b'conv3x3', conv3x3.encode()))
        check(lib().xdet_net_set_option(self.handle, b'pool', pool.encode()))
        check(lib().xdet_net_set_option(self.handle, b'check_range', b'on' if check_range else b'off'))
        if workspace is not None:
            check(lib().xdet_net_set_option(self.handle, b'workspace', workspace.encode()))
        if pool_sub is not None:
            check(lib().xdet_net_set_option(self.handle, b'pool_sub', pool_sub.encode()))
        check(lib().xdet_net_set_option(self.handle, b'ksplit', ksplit.encode() if isinstance(ksplit, str) else (b'on' if ksplit else b'off')))
        check(lib().xdet_net_set_option(self.handle, b'cross', cross.encode()))
        if pool_index:
            check(lib().xdet_net_set_option(self.handle, b'pool_index', b'keep'))
        if rpn_hidden:
            check(lib().xdet_net_set_option(self.handle, b'rpn_hidden', b'keep'))
        if middle_flow_train:
            check(lib().xdet_net_set_option(self.handle, b'entry_x', b'keep'))
        if entry_flow_train:
            check(lib().xdet_net_set_option(self.handle, b'stem_out', b'keep'))
        self.pool_index, self.rpn_hidden = bool(pool_index), bool(rpn_hidden)
        check(lib().xdet_net_build(self.handle))
        self.max_batch = max_batch
        self.image_size = image_size
        self.num_classes = num_classes
        self.R = rpn_post_nms_top_n
        self.nms_topk = nms_topk
        self.stream = Stream()
        B, nc, k = max_batch, num_classes - 1, nms_topk
        self._images = DeviceBuffer(B * 3 * image_size * image_size * 4)
        self._det_scores = DeviceBuffer(B * nc * k * 4)
        self._det_boxes = DeviceBuffer(B * nc * k * 16)
        self._N = 0
        self.large_sep_train = bool(large_sep_train)
        if large_sep_train:
            self._build_large_sep_train(weights)
        self.exit_flow_train = bool(exit_flow_train)
        if exit_flow_train:
            self._build_exit_flow_train(weights)
        self.middle_flow_train = bool(middle_flow_train)
        if middle_flow_train:
            self._build_middle_flow_train(weights)
        self.entry_flow_train = bool(entry_flow_train)
        if entry_flow_train:
            self._build_entry_flow_train(weights)

    def _build_large_sep_train(self, weights):
        """the training form of the large-separable block: the merged kernels as conv layers (split precision, f32 out) and as
        dense device tensors for the backward, the BN vectors, and the tensors a training forward keeps"""
        from . import ops
        from .runtime import get_precision, set_precision
        miss = [k for k in LARGE_SEP_VARIABLES + LARGE_SEP_MOVING if k not in weights]
        if miss:
            raise InvalidArgumentError(-1, 'large_sep_train: the weights lack %s' % ', '.join(miss))
        self._large_sep_variables = {k: np.ascontiguousarray(weights[k], np.float32) for k in LARGE_SEP_VARIABLES + LARGE_SEP_MOVING}
        ka, ba, kb, bb = merge_large_sep(self._large_sep_variables)
        before = get_precision()
        set_precision('f16x3')
        try:
            conv_a, conv_b = ops.Conv2D(ka, shift=ba), ops.Conv2D(kb, shift=bb)
        finally:
            set_precision(before)

        def dense(k):
            b = to_device(k)
            return DeviceTensor(b.ptr, k.shape, k.shape[3], owner=b)
        bn = 'large_sep_feature/batch_normalization/'
        B, (_, H, W, _) = self.max_batch, self.buffer('out', 1).shape
        co, mid2 = kb.shape[3], ka.shape[3]
        vec = lambda a: to_device(np.ascontiguousarray(a, np.float32))
        ws = max(lib().xdet_batch_norm_workspace_bytes(n * H * W, co) for n in range(1, B + 1))
        self._lsep = {'conv_a': conv_a, 'conv_b': conv_b, 'K_a': dense(ka), 'K_b': dense(kb), 'mid': mid2 // 2,
                      'gamma': vec(weights[bn + 'gamma']), 'beta': vec(weights[bn + 'beta']),
                      'moving_mean': vec(weights[bn + 'moving_mean']), 'moving_variance': vec(weights[bn + 'moving_variance']),
                      't': DeviceTensor.empty((B, H, W, mid2)), 'z': DeviceTensor.empty((B, H, W, co)),
                      'save_mean': DeviceBuffer(co * 4), 'save_invstd': DeviceBuffer(co * 4), 'ws': DeviceBuffer(ws), 'n': 0}

    def large_sep_saved(self):
        """what the last large_sep_kernel(..., is_training=True) left on the device, as DeviceTensors: 't' [n,h,w,2*mid] =
        conv_a(out) + b_a, 'z' [n,h,w,co] = conv_b(t) + b_b (the batch norm's input), 'save_mean' and 'save_invstd'
        [1,1,1,co] (the batch statistics), 'moving_mean' and 'moving_variance' [1,1,1,co] (after their update)"""
        if not self.large_sep_train or not self._lsep['n']:
            raise InvalidArgumentError(-1, 'large_sep_saved: no large_sep_kernel(..., is_training=True) has run on this detector')
        s, n = self._lsep, self._lsep['n']
        out = {k: DeviceTensor(s[k].ptr, (n,) + s[k].shape[1:], s[k].ld, owner=s[k]) for k in ('t', 'z')}
        co = s['z'].shape[3]
        for k in ('save_mean', 'save_invstd', 'moving_mean', 'moving_variance'):
            out[k] = DeviceTensor(s[k].ptr, (1, 1, 1, co), co, owner=s[k])
        return out

    def _build_exit_flow_train(self, weights):
        """the training form of the exit flow: per separable unit the depthwise layer, the pointwise conv (split precision, f32
        out, no scale or shift), both kernels as dense device tensors for the backward, the BN vectors and the tensors a
        training forward keeps (the depthwise output, the BN input, the BN output); the same for the projection branch"""
        from . import ops
        from .runtime import get_precision, set_precision
        g = lambda k: np.ascontiguousarray(weights[k], np.float32)
        B, (_, H, W, cin) = self.max_batch, self.buffer('mid_x', 1).shape
        pw = _pointwise_layers(weights, [u[0] for u in EXIT_FLOW_UNITS])
        before = get_precision()
        set_precision('f16x3')
        try:
            proj = ops.Conv2D(g('conv2d_4/kernel'))
        finally:
            set_precision(before)
        e = {'n': 0, 'units': [], 'proj': {'conv': proj, 'K': _dense(g('conv2d_4/kernel'))}}
        widths = [proj.cout]
        for name, dil, relu_in, relu_out in EXIT_FLOW_UNITS:
            # (the last batch norm writes the net's `out`)
            u = _build_unit(weights, name, dil, relu_in, relu_out, pw[name], B, H, W, own_y=name != EXIT_FLOW_UNITS[-1][0])
            e['units'].append(u)
            widths += [u['t'].shape[3], u['z'].shape[3]]
        e['proj'].update(bn=_bn_state(weights, 'batch_normalization_4', proj.cout), z=DeviceTensor.empty((B, H, W, proj.cout)),
                         r=DeviceTensor.empty((B, H, W, proj.cout)))
        e['b2'] = DeviceTensor.empty((B, H, W, proj.cout))
        e['ws_bn'] = DeviceBuffer(max(lib().xdet_batch_norm_workspace_bytes(n * H * W, max(widths)) for n in range(1, B + 1)))
        e['ws_dw'] = DeviceBuffer(max(lib().xdet_depthwise_backward_workspace_bytes(n, H, W, max(widths)) for n in range(1, B + 1)))
        self._exit = e

    def exit_flow_saved(self):
        """what the last model.exit_flow_train() left on the device, as DeviceTensors: per separable unit '<unit>/dw' (the
        depthwise conv's output, the pointwise conv's input) and '<unit>/z' (the pointwise conv's output, the batch norm's
        input), 'conv2d_4/z'; 'a', 'r', 'y2' (block13_sepconv2's batch norm output, b2 = y2 + r), 'b2', 'c3'; and per batch
        norm '<bn>/save_mean', '<bn>/save_invstd' (the batch statistics), '<bn>/moving_mean', '<bn>/moving_variance' (after
        their update), each [1,1,1,C]"""
        if not self.exit_flow_train or not self._exit['n']:
            raise InvalidArgumentError(-1, 'exit_flow_saved: no model.exit_flow_train() has run on this detector')
        e, n = self._exit, self._exit['n']
        view = lambda t: DeviceTensor(t.ptr, (n,) + tuple(t.shape[1:]), t.ld, owner=t)
        out = {'conv2d_4/z': view(e['proj']['z']), 'r': view(e['proj']['r']), 'b2': view(e['b2'])}
        for u, y in zip(e['units'], ('a', 'y2', 'c3', None)):
            out[u['name'] + '/dw'], out[u['name'] + '/z'] = view(u['t']), view(u['z'])
            if y:
                out[y] = view(u['y'])
        for name, b in [(u['name'] + '_bn', u['bn']) for u in e['units']] + [('batch_normalization_4', e['proj']['bn'])]:
            _bn_views(out, name, b)
        return out

    def _build_middle_flow_train(self, weights):
        """the training form of the middle flow: per unit what _build_exit_flow_train builds, the BN outputs y1, y2 and the
        block's output (block 12's is the net's `mid_x`), one BN workspace, one depthwise-backward and one conv-backward
        workspace for all units, and the four gradient tensors middle_flow_backward rotates through; all sized for max_batch"""
        B, (_, H, W, C) = self.max_batch, self.buffer('entry_x', 1).shape
        pw = _pointwise_layers(weights, MIDDLE_FLOW_UNITS)
        m = {'n': 0, 'blocks': []}
        for b in MIDDLE_FLOW_BLOCKS:
            units = [_build_unit(weights, 'block%d_sepconv%d' % (b, i), 1, True, False, pw['block%d_sepconv%d' % (b, i)], B, H, W,
                                 own_y=i < 3) for i in (1, 2, 3)]
            m['blocks'].append({'b': b, 'units': units, 'out': DeviceTensor.empty((B, H, W, C)) if b != MIDDLE_FLOW_BLOCKS[-1] else None})
        sizes = range(1, B + 1)
        m['ws_bn'] = DeviceBuffer(max(lib().xdet_batch_norm_workspace_bytes(n * H * W, C) for n in sizes))
        m['ws_dw'] = DeviceBuffer(max(lib().xdet_depthwise_backward_workspace_bytes(n, H, W, C) for n in sizes))
        m['ws_conv'] = DeviceBuffer(max(lib().xdet_conv_backward_workspace_bytes(n, H, W, C, C, 1, 1) for n in sizes))
        m['rot'] = {k: DeviceTensor.empty((B, H, W, C)) for k in ('dz', 'dt', 'da', 'db')}
        self._middle = m

    def middle_flow_saved(self):
        """what the last model.middle_flow_train() left on the device, as DeviceTensors of the n images it ran on: per unit
        '<unit>/dw' (the depthwise conv's output) and '<unit>/z' (the batch norm's input); the block inputs 'x5' (the net's
        `entry_x`) ... 'x12' (block b's output is 'x<b+1>', block 12's the net's `mid_x`); 'block<b>/y1', 'block<b>/y2' (the
        first two batch norm outputs; the third is overwritten by the residual add, y3 + x, in place); and per batch norm
        '<unit>_bn/save_mean', '/save_invstd' (the batch statistics), '/moving_mean', '/moving_variance' (after their update),
        each [1,1,1,728]"""
        if not self.middle_flow_train or not self._middle['n']:
            raise InvalidArgumentError(-1, 'middle_flow_saved: no model.middle_flow_train() has run on this detector')
        m, n = self._middle, self._middle['n']
        view = lambda t: DeviceTensor(t.ptr, (n,) + tuple(t.shape[1:]), t.ld, owner=t)
        out, x = {}, self.buffer('entry_x', n)
        for blk in m['blocks']:
            out['x%d' % blk['b']] = x
            for u, y in zip(blk['units'], ('y1', 'y2', None)):
                out[u['name'] + '/dw'], out[u['name'] + '/z'] = view(u['t']), view(u['z'])
                if y:
                    out['block%d/%s' % (blk['b'], y)] = view(u['y'])
                _bn_views(out, u['name'] + '_bn', u['bn'])
            x = view(blk['out']) if blk['out'] is not None else None
        return out

    def _build_entry_flow_train(self, weights):
        """the training form of blocks 2-4: per block both units as _build_unit builds them (each keeps its y), the projection
        (conv layer in split precision, dense kernel, BN vectors, z and r), the subsampled input xs, the block's output (block
        4's is the net's `entry_x`) and the gradient tensors entry_flow_backward writes inside the block; one BN, one
        depthwise-backward and one conv-backward workspace for all; everything sized for max_batch"""
        from . import ops
        from .runtime import get_precision, set_precision
        g = lambda k: np.ascontiguousarray(weights[k], np.float32)
        B, (_, H, W, cin) = self.max_batch, self.buffer('stem_out', 1).shape
        pw = _pointwise_layers(weights, ENTRY_FLOW_UNITS)
        e = {'n': 0, 'blocks': []}
        sizes, need = range(1, B + 1), {'bn': 0, 'dw': 0, 'conv': 0}
        l = lib()
        for b in ENTRY_FLOW_BLOCKS:
            kname, bn = 'conv2d_%d/kernel' % (b - 1), 'batch_normalization_%d' % (b - 1)
            before = get_precision()
            set_precision('f16x3')
            try:
                proj = ops.Conv2D(g(kname))
            finally:
                set_precision(before)
            c, Ho, Wo = proj.cout, -(-H // 2), -(-W // 2)
            units = [_build_unit(weights, 'block%d_sepconv%d' % (b, i), 1, _entry_relu_in(b, i), False, pw['block%d_sepconv%d' % (b, i)],
                                 B, H, W, own_y=True) for i in (1, 2)]
            full, half = (lambda ch: DeviceTensor.empty((B, H, W, ch))), (lambda ch: DeviceTensor.empty((B, Ho, Wo, ch)))
            e['blocks'].append({'b': b, 'units': units, 'H': H, 'W': W, 'cin': cin, 'c': c, 'xs': half(cin),
                                'proj': {'name': 'conv2d_%d' % (b - 1), 'bn_name': bn, 'conv': proj, 'K': _dense(g(kname)),
                                         'bn': _bn_state(weights, bn, c), 'z': half(c), 'r': half(c)},
                                'out': half(c) if b != ENTRY_FLOW_BLOCKS[-1] else None,
                                # a unit's dz is dead once its conv backward has run: one tensor serves both units
                                'rot': {'dzr': half(c), 'dxs': half(cin), 'dy2': full(c), 'dz': full(c), 'dt2': full(c),
                                        'd2': full(c), 'dt1': full(cin), 'd1': full(cin)}})
            for n in sizes:
                need['bn'] = max(need['bn'], l.xdet_batch_norm_workspace_bytes(n * H * W, c), l.xdet_batch_norm_workspace_bytes(n * Ho * Wo, c))
                need['dw'] = max(need['dw'], l.xdet_depthwise_backward_workspace_bytes(n, H, W, c),
                                 l.xdet_depthwise_backward_workspace_bytes(n, H, W, cin))
                need['conv'] = max(need['conv'], l.xdet_conv_backward_workspace_bytes(n, Ho, Wo, cin, c, 1, 1),
                                   l.xdet_conv_backward_workspace_bytes(n, H, W, cin, c, 1, 1),
                                   l.xdet_conv_backward_workspace_bytes(n, H, W, c, c, 1, 1))
            H, W, cin = Ho, Wo, c
        ex = self.buffer('entry_x', 1)
        if tuple(ex.shape[1:]) != (H, W, cin):
            raise InvalidArgumentError(-1, 'entry_flow_train: block 4 gives %r but the net\'s entry_x is %r' % ((H, W, cin), tuple(ex.shape[1:])))
        e['ws_bn'], e['ws_dw'], e['ws_conv'] = DeviceBuffer(need['bn']), DeviceBuffer(need['dw']), DeviceBuffer(need['conv'])
        self._entry = e

    def entry_flow_saved(self):
        """what the last model.entry_flow_train() left on the device, as DeviceTensors of the n images it ran on: the block
        inputs 'x2' (the net's `stem_out`), 'x3', 'x4' and 'x5' (block 4's output, the net's `entry_x`); per block 'block<b>/xs'
        (the subsampled input), 'conv2d_<b-1>/z' (the projection's output, its batch norm's input), 'block<b>/r' (that batch
        norm's output, the shortcut), 'block<b>/y1', 'block<b>/y2' (the units' batch norm outputs; y2 is the pool's input); per
        unit '<unit>/dw' (the depthwise conv's output) and '<unit>/z' (the batch norm's input); and per batch norm
        '<bn>/save_mean', '/save_invstd' (the batch statistics), '/moving_mean', '/moving_variance' (after their update), each
        [1,1,1,C]"""
        if not self.entry_flow_train or not self._entry['n']:
            raise InvalidArgumentError(-1, 'entry_flow_saved: no model.entry_flow_train() has run on this detector')
        e, n = self._entry, self._entry['n']
        view = lambda t: DeviceTensor(t.ptr, (n,) + tuple(t.shape[1:]), t.ld, owner=t)
        out, x = {}, self.buffer('stem_out', n)
        for blk in e['blocks']:
            b, p = blk['b'], blk['proj']
            out['x%d' % b] = x
            out['block%d/xs' % b], out[p['name'] + '/z'], out['block%d/r' % b] = view(blk['xs']), view(p['z']), view(p['r'])
            _bn_views(out, p['bn_name'], p['bn'])
            for u, y in zip(blk['units'], ('y1', 'y2')):
                out[u['name'] + '/dw'], out[u['name'] + '/z'] = view(u['t']), view(u['z'])
                out['block%d/%s' % (b, y)] = view(u['y'])
                _bn_views(out, u['name'] + '_bn', u['bn'])
            x = view(blk['out']) if blk['out'] is not None else self.buffer('entry_x', n)
        out['x%d' % (ENTRY_FLOW_BLOCKS[-1] + 1)] = x
        return out

    # ---- plumbing -------------------------------------------------------------------
    def buffer(self, name, n=None):
        p = c_void_p()
        dims = (ctypes.c_int64 * 4)()
        ld = ctypes.c_int()
        check(lib().xdet_net_buffer(self.handle, name.encode(), ctypes.byref(p), ctypes.byref(dims), ctypes.byref(ld)))
        d = list(dims)
        d[0] = n or self._N or d[0]
        return DeviceTensor(p.value, d, ld.value, owner=self)

    def flat(self, name, shape, dtype=np.float32):
        p = c_void_p()
        dims = (ctypes.c_int64 * 4)()
        ld = ctypes.c_int()
        check(lib().xdet_net_buffer(self.handle, name.encode(), ctypes.byref(p), ctypes.byref(dims), ctypes.byref(ld)))
        return to_host(p.value, shape, dtype)

    def write(self, name, array):
        """overwrite a workspace buffer from the host (tests: feed one stage the oracle's tensors)."""
        t = self.buffer(name, n=array.shape[0])
        a = np.asarray(array, np.float32)
        if name in ('objectness', 'rpn_boxes', 'proposals', 'head_boxes'):
            flat = np.ascontiguousarray(a)
        else:
            n, h, w, c = a.shape
            flat = np.zeros((n, h, w, t.ld), np.float32)
            flat[..., :c] = a
        check(lib().xdet_memcpy_h2d(t.ptr, _host(flat), flat.nbytes, None))
        synchronize()
        self._N = a.shape[0]

    @contextlib.contextmanager
    def scope(self):
        _current.append(self)
        try:
            yield self
        finally:
            _current.pop()

    def set_images(self, images_nchw):
        a = np.ascontiguousarray(images_nchw, np.float32)
        assert a.ndim == 4 and a.shape[1] == 3 and a.shape[2] == a.shape[3] == self.image_size, a.shape
        assert a.shape[0] <= self.max_batch
        check(lib().xdet_memcpy_h2d(self._images.ptr, _host(a), a.nbytes, self.stream.handle))
        self._N = a.shape[0]
        return self._N

    # ---- the whole forward (lighr_head_model_fn, eval) -----------------------------------
    def forward_device(self, n=None, use_graph=False, images_ptr=None, image_shapes_ptr=None, bbox_img_ptr=None,
                       det_scores_ptr=None, det_boxes_ptr=None):
        """asynchronous: images already resident (set_images or caller-owned device pointer)."""
        n = n or self._N
        check(lib().xdet_net_forward(self.handle, images_ptr or self._images.ptr, n, image_shapes_ptr, bbox_img_ptr,
                                     det_scores_ptr or self._det_scores.ptr, det_boxes_ptr or self._det_boxes.ptr,
                                     1 if use_graph else 0, self.stream.handle))

    def calibrate(self, images_nchw):
        """Choose the activation pre-scale of the split-precision operands from a calibration batch (whitened f32
        [N,3,S,S], N <= max_batch): tensors whose magnitude comes near the f16 range of the hi/lo planes get a
        power-of-two exponent (planes hold x * 2^-e, folded back exactly by the consumer).  Returns {name: e} of the
        tensors that were scaled -- empty for a net whose activations are small, which then stays bit-identical."""
        n = self.set_images(images_nchw)
        k = ctypes.c_int()
        check(lib().xdet_net_calibrate(self.handle, self._images.ptr, n, ctypes.byref(k), self.stream.handle))
        return {name: e for name, e in self.plane_scales().items() if e}

    def x8_planes(self):
        """tensors in the x8 form (cross='fp8', after calibrate()): xdet_net_x8_planes"""
        n = ctypes.c_int()
        check(lib().xdet_net_x8_planes(self.handle, ctypes.byref(n)))
        return n.value

    def plane_scales(self):
        cnt = ctypes.c_int()
        check(lib().xdet_net_plane_scales(self.handle, 0, ctypes.byref(cnt), None))
        ex = (ctypes.c_int * max(cnt.value, 1))()
        check(lib().xdet_net_plane_scales(self.handle, cnt.value, ctypes.byref(cnt), ex))
        buf = ctypes.create_string_buffer(256)
        out = {}
        for i in range(cnt.value):
            check(lib().xdet_net_plane_scale_name(self.handle, i, buf, 256))
            out['%d: %s' % (i, buf.value.decode())] = ex[i]
        return out

    def detections(self, n=None):
        n = n or self._N
        nc, k = self.num_classes - 1, self.nms_topk
        self.stream.synchronize()
        s = to_host(self._det_scores.ptr, (n, nc, k), np.float32)
        b = to_host(self._det_boxes.ptr, (n, nc, k, 4), np.float32)
        if np.isnan(s[:, :, 0]).any():
            # bboxes_eval marks an (image, class) slot NaN when a head logit was not finite (csrc/detect.hip)
            raise XdetError(-4, 'non-finite network outputs / out-of-range activations for image(s) %s: an activation '
                                'left the f16 range of the split-precision convs (|x| > 65504) or the weights are '
                                'broken; use set_precision("f32")'
                            % sorted(set(np.argwhere(np.isnan(s[:, :, 0]))[:, 0].tolist())))
        return s, b

    def forward(self, images_nchw, use_graph=False):
        """images [N,3,S,S] whitened f32 -> list of {class: (scores[topk], boxes[topk,4])}, the
        per-class zero-padded output of bboxes_eval (light_head_rfcn_eval.py:263-287)."""
        n = self.set_images(images_nchw)
        self.forward_device(n, use_graph)
        s, b = self.detections(n)
        return [{c + 1: (s[i, c], b[i, c]) for c in range(self.num_classes - 1)} for i in range(n)]

    def detect_images(self, images, resize=None, use_graph=True):
        """A list of at most max_batch decoded uint8 [H,W,3] images of any sizes -> the list forward() returns, one
        {class: (scores, boxes)} per image, boxes relative to each ORIGINAL image (light_head_rfcn_eval.py:263-287 with
        labels['targets'][-1] = the image's shape, and bbox_img from the resize step).  Ingest (xdet_net_forward_u8:
        light_head_preprocess_for_eval with `resize`, ops.Resize) and the forward run as one launch sequence, or one
        graph (use_graph): image sizes live in device buffers, so batches of other sizes replay the same graph as
        long as the packed bytes fit."""
        n = self._ingest_forward(images, resize, use_graph)
        s, b = self.detections(n)
        return [{c + 1: (s[i, c], b[i, c]) for c in range(self.num_classes - 1)} for i in range(n)]

    def _ingest_forward(self, images, resize, use_graph, before_upload=None):
        """detect_images' asynchronous part: pack, copy, xdet_net_forward_u8 on self.stream -> the number of images.
        before_upload(n): called once the batch is checked, in front of the first copy."""
        from . import ops
        imgs, S, mode = ops._check_batch(images, self.image_size, ops.Resize.WARP_RESIZE if resize is None else resize,
                                         self.max_batch)
        packed, offsets, shapes = ops.pack_images(imgs)
        n = len(imgs)
        if before_upload is not None:
            before_upload(n)
        B = self.max_batch
        if not hasattr(self, '_ingest'):
            # offsets / image_shapes / bbox_img: max_batch entries, allocated once.  packed grows only: a regrown buffer
            # has another pointer and size, so the next call captures a new graph instead of replaying one that
            # reads the old buffer.
            self._ingest = {'offsets': DeviceBuffer(B * 8), 'shapes': DeviceBuffer(B * 8),
                            'bbox_img': DeviceBuffer(B * 16), 'packed': None}
        bufs = self._ingest
        if bufs['packed'] is None or bufs['packed'].nbytes < packed.nbytes:
            cap = max(packed.nbytes, 2 * bufs['packed'].nbytes if bufs['packed'] is not None else 0)
            bufs['packed'] = DeviceBuffer(cap)
        h = self.stream.handle
        check(lib().xdet_memcpy_h2d(bufs['packed'].ptr, _host(packed), packed.nbytes, h))
        check(lib().xdet_memcpy_h2d(bufs['offsets'].ptr, _host(offsets), offsets.nbytes, h))
        check(lib().xdet_memcpy_h2d(bufs['shapes'].ptr, _host(shapes), shapes.nbytes, h))
        # packed_bytes = the buffer's capacity: the graph key stays the same for every batch that fits
        check(lib().xdet_net_forward_u8(self.handle, bufs['packed'].ptr, bufs['packed'].nbytes, bufs['offsets'].ptr,
                                        bufs['shapes'].ptr, n, int(mode), self._images.ptr, bufs['bbox_img'].ptr,
                                        self._det_scores.ptr, self._det_boxes.ptr, 1 if use_graph else 0, h))
        self._N = n
        self._host_keep = (packed, offsets, shapes)      # (referenced until the next call: nothing waits for the copies here)
        return n

    def evaluate_images(self, images, ground_truths, image_ids=None, resize=None, accumulator=None, matching_threshold=0.5,
                        use_graph=True):
        """detect_images' ingest and forward, then the scoring of the detections against the ground truth
        (evaluation.GpuStreamingTpFp: xdet_tpfp_update) on the same stream, with the ground truth copied to the device in
        front of the forward -- light_head_rfcn_eval.py:263-296 for a batch.  Nothing is copied back and the stream is not
        synchronised: the call returns with the work enqueued, the accumulator is read later (records(),
        average_precisions()).  ground_truths: per image (glabels, gbboxes, gdifficults) with boxes (ymin, xmin, ymax,
        xmax) relative to the original image, as glabels_raw / gbboxes_raw / isdifficult; image_ids: one integer per image
        (default: a running count per detector), the order of the dataset.  Returns the accumulator (the detector's own
        unless one is given)."""
        from .evaluation import GpuStreamingTpFp
        if accumulator is None:
            if not hasattr(self, '_accumulator'):
                self._accumulator = GpuStreamingTpFp(self.num_classes, self.nms_topk)
            accumulator = self._accumulator
        if len(ground_truths) != len(images):
            raise InvalidArgumentError(-1, 'evaluate_images: %d images but ground truth of %d' % (len(images), len(ground_truths)))
        if image_ids is None:
            first = getattr(self, '_next_image_id', 0)
            image_ids = np.arange(first, first + len(images), dtype=np.int32)

        def stage(n):
            accumulator.stage(image_ids, ground_truths, self.stream)
        n = self._ingest_forward(images, resize, use_graph, before_upload=stage)
        accumulator.enqueue(self._det_scores.ptr, self._det_boxes.ptr, n, matching_threshold, self.stream)
        self._next_image_id = int(np.max(image_ids)) + 1
        return accumulator

    def evaluate(self, dataset, batch=None, resize=None, accumulator=None, matching_threshold=0.5):
        """dataset: an iterable of (image uint8 [H,W,3], (glabels, gbboxes, gdifficults)) -> {'AP_VOC07': {class: AP},
        'AP_VOC12': {...}, 'mAP_VOC07': ., 'mAP_VOC12': .} as the reference's eval reports them
        (light_head_rfcn_eval.py:304-338); images are numbered in the order they arrive."""
        from .evaluation import GpuStreamingTpFp
        acc = accumulator if accumulator is not None else GpuStreamingTpFp(self.num_classes, self.nms_topk)
        batch = batch or self.max_batch
        images, gts, seen = [], [], 0
        for image, gt in dataset:
            images.append(image)
            gts.append(gt)
            if len(images) == batch:
                self.evaluate_images(images, gts, np.arange(seen, seen + len(images)), resize, acc, matching_threshold)
                seen += len(images)
                images, gts = [], []
        if images:
            self.evaluate_images(images, gts, np.arange(seen, seen + len(images)), resize, acc, matching_threshold)
        return acc.summary()

    def graph_count(self):
        """graphs cached by this detector's net (xdet_net_graph_count)"""
        k = ctypes.c_int()
        check(lib().xdet_net_graph_count(self.handle, ctypes.byref(k)))
        return k.value

    def predictions(self, n=None):
        """the `predictions` dict of the EstimatorSpec (light_head_rfcn_eval.py:429-433)."""
        n = n or self._N
        nc = self.num_classes
        cr = self.buffer('cls_reg', n).numpy().reshape(n, self.R, -1)
        logits = cr[..., :nc]
        e = np.exp(logits - logits.max(-1, keepdims=True))
        prob = e / e.sum(-1, keepdims=True)
        hb = self.flat('head_boxes', (n, self.R, 4))
        return {'classes': prob.argmax(-1), 'probabilities': prob.max(-1), 'bboxes_predict': hb}

    def memory(self):
        """{'allocated_bytes': device memory of workspace + weights, 'recycled_bytes': tensors placed into recycled blocks}"""
        a, r = ctypes.c_size_t(), ctypes.c_size_t()
        check(lib().xdet_net_memory(self.handle, ctypes.byref(a), ctypes.byref(r)))
        return {'allocated_bytes': int(a.value), 'recycled_bytes': int(r.value)}

    def flops_per_image(self):
        v = [ctypes.c_double() for _ in range(4)]
        check(lib().xdet_net_flops_per_image(self.handle, *[ctypes.byref(x) for x in v]))
        return dict(zip(('backbone', 'rpn', 'large_sep', 'head'), [x.value for x in v]))

    def __del__(self):
        try:
            lib().xdet_net_destroy(self.handle)
        except Exception:
            pass


class PipelinedDetector(object):
    """`ways` LightHeadDetector instances, each on its own HIP stream, that process contiguous slices of
    one batch concurrently.  Images are independent units and a detection does not depend on the batch it
    was computed in (tests/test_gpu_fullsize.py::test_batch_invariance), so the result equals the single
    detector's bit for bit; what changes is throughput: the partial last round of workgroups of one
    launch is filled by the other stream's kernels (about +5 % at 2 x 64 images on an MI355X)."""

    def __init__(self, weights, ways=2, max_batch=2, **kw):
        assert ways >= 1 and max_batch >= ways
        self.ways = ways
        self.sub = -(-max_batch // ways)
        self.max_batch = self.sub * ways
        self.nets = [LightHeadDetector(weights, max_batch=self.sub, **kw) for _ in range(ways)]
        n0 = self.nets[0]
        self.image_size, self.num_classes, self.R, self.nms_topk = n0.image_size, n0.num_classes, n0.R, n0.nms_topk
        self._counts = [0] * ways

    def set_images(self, images_nchw):
        n = images_nchw.shape[0]
        assert n <= self.max_batch
        self._counts = []
        for i, net in enumerate(self.nets):
            part = images_nchw[i * self.sub:min(n, (i + 1) * self.sub)]
            self._counts.append(part.shape[0])
            if part.shape[0]:
                net.set_images(part)
        return n

    def forward_device(self, use_graph=True):
        """asynchronous: one launch sequence (or graph replay) per sub-batch, each on its own stream"""
        for net, c in zip(self.nets, self._counts):
            if c:
                net.forward_device(c, use_graph=use_graph)

    def synchronize(self):
        for net in self.nets:
            net.stream.synchronize()

    def detections(self):
        parts = [net.detections(c) for net, c in zip(self.nets, self._counts) if c]
        return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])

    def forward(self, images_nchw, use_graph=True):
        """same contract as LightHeadDetector.forward"""
        n = self.set_images(images_nchw)
        self.forward_device(use_graph)
        s, b = self.detections()
        return [{c + 1: (s[i, c], b[i, c]) for c in range(self.num_classes - 1)} for i in range(n)]

    def flops_per_image(self):
        return self.nets[0].flops_per_image()


def _det():
    if not _current:
        raise XdetError(-3, 'no current LightHeadDetector: use `with detector.scope():`')
    return _current[-1]


def _sync(d):
    d.stream.synchronize()


def _same(t, view):
    return isinstance(t, DeviceTensor) and t.ptr == view.ptr


def XceptionBody(input_image, num_classes, is_training=False, data_format='channels_last'):
    """net/xception_body.py:236-379 -> (mid_outputs, outputs) as DeviceTensors (NHWC).  Forward only: of the training
    graph this package has the target assignment (get_proposals with is_training=True) and the losses (xdet.losses,
    get_head with is_training=True), not the batch-norm updates."""
    assert not is_training, 'forward-only path'
    d = _det()
    a = np.asarray(input_image, np.float32)
    if data_format == 'channels_last':
        a = np.transpose(a, (0, 3, 1, 2))
    n = d.set_images(a)
    check(lib().xdet_net_xception_body(d.handle, d._images.ptr, n, d.stream.handle))
    _sync(d)
    return d.buffer('mid', n), d.buffer('out', n)


def get_rpn(net_input, num_anchors, is_training, data_format, var_scope):
    """net/xception_body.py:381-400 -> (rpn_cls_score [N,h,w,2A], rpn_bbox_pred [N,h,w,4A])."""
    d = _det()
    n = net_input.shape[0]
    if not _same(net_input, d.buffer('mid', n)):
        raise XdetError(-1, 'get_rpn expects the mid_outputs tensor returned by XceptionBody')
    check(lib().xdet_net_get_rpn(d.handle, n, d.stream.handle))
    _sync(d)
    out = d.buffer('rpn_out', n)
    return out.channels(0, 2 * num_anchors), out.channels(2 * num_anchors, 6 * num_anchors)


def large_sep_kernel(net_input, depth_mid, depth_output, is_training, data_format, var_scope):
    """net/xception_body.py:450-475 -> thin feature map [N,h,w,depth_output].
    is_training=True (a detector built with large_sep_train=True): the block as the reference trains it, t = conv_a(out) + b_a,
    z = conv_b(t) + b_b on the merged kernels (xdet_conv_forward, split precision, f32 out), then feat = relu(bn(z)) with the
    batch's statistics and the moving-average updates (xdet_batch_norm_forward, eps 1e-5, momentum 0.997) written straight
    into the net's `feat` buffer -- three calls on the detector's stream with no host round trip in between.  t, z and the
    statistics stay on the device (detector.large_sep_saved()) for large_sep_backward."""
    d = _det()
    n = net_input.shape[0]
    if is_training and not d.large_sep_train:
        raise InvalidArgumentError(-1, 'large_sep_kernel: is_training=True needs a detector built with large_sep_train=True '
                                       '(the default detector folds the moving statistics into the conv weights)')
    view = d.buffer('out', n)
    if not _same(net_input, view):
        d.write('out', net_input.numpy() if isinstance(net_input, DeviceTensor) else net_input)
    if is_training:
        s, feat, h = d._lsep, d.buffer('feat', n), d.stream.handle
        _, H, W, _ = view.shape
        t, z = s['t'], s['z']
        check(lib().xdet_conv_forward(s['conv_a'].handle, view.ptr, n, H, W, view.ld, t.ptr, t.ld, None, 0, h))
        check(lib().xdet_conv_forward(s['conv_b'].handle, t.ptr, n, H, W, t.ld, z.ptr, z.ld, None, 0, h))
        check(lib().xdet_batch_norm_forward(z.ptr, z.ld, n * H * W, z.shape[3], s['gamma'].ptr, s['beta'].ptr, LARGE_SEP_EPS, 1,
                                            LARGE_SEP_MOMENTUM, s['moving_mean'].ptr, s['moving_variance'].ptr, 1, feat.ptr,
                                            feat.ld, s['save_mean'].ptr, s['save_invstd'].ptr, s['ws'].ptr, h))
        s['n'] = n
        _sync(d)
        return feat
    check(lib().xdet_net_large_sep(d.handle, n, d.stream.handle))
    _sync(d)
    return d.buffer('feat', n)


def rpn_decode(rpn_cls_score, rpn_bbox_pred):
    """light_head_rfcn_eval.py:389-397 + labels['rpn_decode_fn'] -> (objectness [N,HWA], boxes [N,HWA,4])
    as numpy arrays; the device copies stay in the net for get_proposals."""
    d = _det()
    n = rpn_cls_score.shape[0]
    check(lib().xdet_net_rpn_decode(d.handle, n, d.stream.handle))
    _sync(d)
    na = d.buffer('objectness', n).shape[1]
    return d.flat('objectness', (n, na)), d.flat('rpn_boxes', (n, na, 4))


def get_proposals(object_score, bboxes_pred, encode_fn, rpn_pre_nms_top_n, rpn_post_nms_top_n, nms_threshold,
                  rpn_min_size, is_training, data_format):
    """net/xception_body.py:402-448 -> proposals [N,post_n,4] numpy.  is_training=True (:446-448): the same proposal
    stage, then encode_fn(proposals) with the net's `proposals` buffer handed over on the device -> its (rois, targets,
    labels, scores) (targets.AnchorEncoder.ext_encode_rois)."""
    if is_training and encode_fn is None:
        raise InvalidArgumentError(-1, 'get_proposals: is_training=True needs an encode_fn')
    d = _det()
    # the native net bakes these in at build time (xdet_lighthead_config): a caller porting reference code
    # with other values must build the detector with them, not get silently different proposals
    want = (d.cfg.rpn_pre_nms_top_n, d.cfg.rpn_post_nms_top_n, np.float32(d.cfg.rpn_nms_thres), np.float32(d.cfg.rpn_min_size))
    got = (rpn_pre_nms_top_n, rpn_post_nms_top_n, np.float32(nms_threshold), np.float32(rpn_min_size))
    if want != got:
        raise InvalidArgumentError(-1, 'get_proposals: (pre_n, post_n, nms_threshold, rpn_min_size) = %r but the '
                                       'detector was built with %r' % (got, want))
    n = object_score.shape[0]
    d.write('objectness', np.asarray(object_score, np.float32))
    d.write('rpn_boxes', np.asarray(bboxes_pred, np.float32))
    check(lib().xdet_net_get_proposals(d.handle, n, d.stream.handle))
    _sync(d)
    if is_training:
        return encode_fn(d.buffer('proposals', n))
    return d.flat('proposals', (n, d.R, 4))


def get_head(net_input, pooling_op, grid_width, grid_height, loss_func, proposals_bboxes, num_classes, is_training,
             using_ohem, ohem_roi_one_image, data_format, var_scope):
    """net/xception_body.py:477-560.  is_training=False -> (cls_score [N,R,nc], bboxes_reg [N,R,4]) numpy.
    is_training=True (:502-533, 560): `proposals_bboxes` are the sampled ROIs of get_proposals' training branch and `loss_func`
    a losses.HeadLoss carrying their labels, targets and fg_ratio; PsRoiAlign and the head run on them, then xdet_head_loss
    on the net's `cls_reg` buffer in place (OHEM keeps the ohem_roi_one_image hardest ROIs per image; the reference's second
    run of the dense layers on the gathered rows has the same weights, so the selected rows' logits are the gathered ones)
    -> the scalar head loss; losses, per-ROI values, the selection and d loss / d cls_reg are in loss_func.result.  The head's
    row count is fixed when the detector is built: proposals_bboxes.shape[1] must equal its rpn_post_nms_top_n (a head detector
    built with rpn_post_nms_top_n = the ROIs sampled per image).  `pooling_op` is accepted for signature parity; the fused HIP
    PsRoiAlign is always used.  head_backward(loss_func) takes the gradient from there through the two dense layers."""
    d = _det()
    if (grid_width, grid_height) != (d.cfg.grid, d.cfg.grid) or num_classes != d.cfg.num_classes:
        raise InvalidArgumentError(-1, 'get_head: grid %dx%d / %d classes but the detector was built with %dx%d / %d'
                                   % (grid_width, grid_height, num_classes, d.cfg.grid, d.cfg.grid, d.cfg.num_classes))
    n = proposals_bboxes.shape[0]
    if is_training:
        from .losses import HeadLoss
        if not isinstance(loss_func, HeadLoss):
            raise InvalidArgumentError(-1, 'get_head: is_training=True needs a losses.HeadLoss as loss_func')
        if proposals_bboxes.shape[1] != d.R:
            raise InvalidArgumentError(-1, 'get_head: %d ROIs per image but the detector was built with rpn_post_nms_top_n = %d'
                                       % (proposals_bboxes.shape[1], d.R))
    elif using_ohem:
        raise InvalidArgumentError(-1, 'get_head: OHEM belongs to the training branch (is_training=True)')
    view = d.buffer('feat', n)
    if not _same(net_input, view):
        d.write('feat', net_input.numpy() if isinstance(net_input, DeviceTensor) else net_input)
    d.write('proposals', np.asarray(proposals_bboxes, np.float32))
    check(lib().xdet_net_get_head(d.handle, n, d.stream.handle))
    _sync(d)
    if is_training:
        res = loss_func(d.buffer('cls_reg', n), None, int(ohem_roi_one_image) if using_ohem else 0, num_classes)
        return float(res.losses[0])
    cr = d.buffer('cls_reg', n).numpy().reshape(n, d.R, -1)
    return cr[..., :num_classes], cr[..., num_classes:num_classes + 4]


def head_backward(loss_func, to_feat=False):
    """The backward of the head's dense layers, called after get_head(..., is_training=True, ...) on the same detector:
    d loss / d cls_reg (loss_func.grad_device, what xdet_head_loss wrote) goes through `fc_cls+fc_loc` (x = the net's `fc`
    buffer, the concatenated [2048, nc + 4] kernel) and then, masked by fc's ReLU, through `subnet_fc` (x = `pooled`) -- two
    calls of xdet_dense_backward on the net's buffers with their own ld.  -> a dict with the six gradients under the
    checkpoint's variable names (final_head/{subnet_fc,fc_cls,fc_loc}/{kernel,bias}, NumPy) and 'pooled': d loss / d pooled
    as a DeviceTensor [N,R,1,C] ([N * R, C] rows, ld C) and 'fc': d loss / d fc (in front of fc's ReLU mask) likewise.
    to_feat=True (a detector built with pool_index=True): d loss / d pooled goes on through xdet_net_head_pool_backward -- the
    order-exact PsRoiAlign gradient on the net's `proposals` and the argmax get_head kept -- on the same stream, with no host
    round trip in between, and the dict gains 'feat': d loss / d feat as a DeviceTensor [N,H,W,C] with the `feat` buffer's
    ld (padding channels zero), what the large-separable backward will read."""
    from . import ops
    d = _det()
    if to_feat and not d.pool_index:
        raise InvalidArgumentError(-1, 'head_backward: to_feat=True needs a detector built with pool_index=True (the head '
                                       'kept no argmax to go back through)')
    g = getattr(loss_func, 'grad_device', None)
    if getattr(loss_func, 'result', None) is None or g is None:
        raise InvalidArgumentError(-1, 'head_backward: the losses ran without a gradient (call get_head(..., is_training=True, '
                                       '...) with this loss_func first)')
    n, nc = g.shape[0], d.cfg.num_classes
    if (g.shape[1], g.shape[3]) != (d.R, nc + 4) or n > d.max_batch:
        raise InvalidArgumentError(-1, 'head_backward: gradient of shape %r but the detector has %d ROIs per image, %d classes, '
                                       'max_batch %d' % (g.shape, d.R, nc, d.max_batch))
    if len(d._head_kernels) != 3:
        raise InvalidArgumentError(-1, 'head_backward: the detector was built without the final_head kernels')
    if not hasattr(d, '_head_kernels_dev'):
        k0 = d._head_kernels['final_head/subnet_fc/kernel']
        k1 = np.concatenate([d._head_kernels['final_head/fc_cls/kernel'], d._head_kernels['final_head/fc_loc/kernel']], axis=1)
        d._head_kernels_dev = []
        for k in (k0, np.ascontiguousarray(k1)):
            b = to_device(k)
            d._head_kernels_dev.append(DeviceTensor(b.ptr, (k.shape[0], 1, 1, k.shape[1]), k.shape[1], owner=b))
    w0, w1 = d._head_kernels_dev
    fc, pooled = d.buffer('fc', n), d.buffer('pooled', n)
    d_feat = None
    if to_feat:                                    # (allocated ahead of the launches, not between the last two)
        fb = d.buffer('feat', n)
        d_feat = DeviceTensor.empty(fb.shape, ld=fb.ld)
    dx1, dw1, db1 = ops.dense_backward_device(fc, w1, g, None, stream=d.stream)
    dx0, dw0, db0 = ops.dense_backward_device(pooled, w0, dx1, fc, stream=d.stream)
    if to_feat:
        check(lib().xdet_net_head_pool_backward(d.handle, n, dx0.ptr, dx0.ld, d_feat.ptr, d.stream.handle))
    _sync(d)
    K0, K1 = w0.shape[0], w1.shape[0]
    kw1, kb1 = to_host(dw1.ptr, (K1, nc + 4)), to_host(db1.ptr, (nc + 4,))
    out = {'final_head/subnet_fc/kernel': to_host(dw0.ptr, (K0, K1)), 'final_head/subnet_fc/bias': to_host(db0.ptr, (K1,)),
           'final_head/fc_cls/kernel': np.ascontiguousarray(kw1[:, :nc]), 'final_head/fc_cls/bias': kb1[:nc].copy(),
           'final_head/fc_loc/kernel': np.ascontiguousarray(kw1[:, nc:]), 'final_head/fc_loc/bias': kb1[nc:].copy(),
           'pooled': DeviceTensor(dx0.ptr, (n, d.R, 1, K0), K0, owner=dx0),
           'fc': DeviceTensor(dx1.ptr, (n, d.R, 1, K1), K1, owner=dx1)}
    if to_feat:
        out['feat'] = d_feat
    return out


def rpn_backward(rpn_loss_result):
    """The backward of the RPN head (net/xception_body.py:381-400), called after get_rpn and losses.rpn_loss(...,
    keep_device=True) on a detector built with rpn_hidden=True: d loss / d rpn_out (rpn_loss_result.grad_device, what
    xdet_rpn_loss wrote) goes through the two 1x1 heads as one dense layer (xdet_dense_backward: x = the net's `rpn_hidden`
    buffer as [N*h*w, 512] rows, the concatenated [512, 6A] kernel) and then, masked by the hidden ReLU, through the 3x3 conv
    (xdet_conv_backward: x = `mid_x` with the ReLU in front of the conv, y = `rpn_hidden`) -- both on the detector's stream
    with no host round trip in between.  -> a dict with the six gradients under the checkpoint's variable names
    (rpn_head/{conv2d,conv2d_1,conv2d_2}/{kernel,bias}, NumPy), 'mid': d loss / d mid_x as a DeviceTensor [N,h,w,728] with
    `mid_x`'s ld (zero where mid_x <= 0) and 'rpn_hidden': d loss / d rpn_hidden (in front of the ReLU mask) [N,h,w,512]."""
    from . import ops
    d = _det()
    if not d.rpn_hidden:
        raise InvalidArgumentError(-1, 'rpn_backward: needs a detector built with rpn_hidden=True (the RPN conv kept no f32 '
                                       'output to go back through)')
    g = getattr(rpn_loss_result, 'grad_device', None)
    if g is None:
        raise InvalidArgumentError(-1, 'rpn_backward: the loss left no gradient on the device (call losses.rpn_loss(..., '
                                       'keep_device=True) on the tensors get_rpn returned)')
    if len(d._rpn_kernels) != 3:
        raise InvalidArgumentError(-1, 'rpn_backward: the detector was built without the rpn_head kernels')
    n, A = g.shape[0], d.cfg.num_anchors
    out_view = d.buffer('rpn_out', min(max(n, 1), d.max_batch))
    if n > d.max_batch or tuple(g.shape[1:]) != tuple(out_view.shape[1:3]) + (6 * A,) or g.ld != out_view.ld:
        raise InvalidArgumentError(-1, 'rpn_backward: gradient of shape %r (ld %d) but the detector\'s rpn_out is %r (ld %d), '
                                       'max_batch %d' % (g.shape, g.ld, tuple(out_view.shape[1:]), out_view.ld, d.max_batch))
    if not hasattr(d, '_rpn_kernels_dev'):
        k0 = d._rpn_kernels['rpn_head/conv2d/kernel']
        k1 = np.ascontiguousarray(np.concatenate([d._rpn_kernels['rpn_head/conv2d_1/kernel'].reshape(-1, 2 * A),
                                                  d._rpn_kernels['rpn_head/conv2d_2/kernel'].reshape(-1, 4 * A)], axis=1))
        b0, b1 = to_device(k0), to_device(k1)
        d._rpn_kernels_dev = (DeviceTensor(b0.ptr, k0.shape, k0.shape[3], owner=b0),
                              DeviceTensor(b1.ptr, (k1.shape[0], 1, 1, k1.shape[1]), k1.shape[1], owner=b1))
    w0, w1 = d._rpn_kernels_dev
    hid, mid_x = d.buffer('rpn_hidden', n), d.buffer('mid_x', n)
    dx1, dw1, db1 = ops.dense_backward_device(hid, w1, g, None, stream=d.stream)
    d_hid = DeviceTensor(dx1.ptr, hid.shape, dx1.ld, owner=dx1)
    dx0, dw0, db0 = ops.conv_backward_device(mid_x, w0, d_hid, hid, relu_in=True, stream=d.stream)
    _sync(d)
    J = w0.shape[3]
    kw1, kb1 = to_host(dw1.ptr, (J, 6 * A)), to_host(db1.ptr, (6 * A,))
    return {'rpn_head/conv2d/kernel': to_host(dw0.ptr, w0.shape), 'rpn_head/conv2d/bias': to_host(db0.ptr, (J,)),
            'rpn_head/conv2d_1/kernel': np.ascontiguousarray(kw1[:, :2 * A]).reshape(1, 1, J, 2 * A),
            'rpn_head/conv2d_1/bias': kb1[:2 * A].copy(),
            'rpn_head/conv2d_2/kernel': np.ascontiguousarray(kw1[:, 2 * A:]).reshape(1, 1, J, 4 * A),
            'rpn_head/conv2d_2/bias': kb1[2 * A:].copy(),
            'mid': dx0, 'rpn_hidden': d_hid}


def large_sep_backward(d_feat):
    """The backward of the large-separable block in training mode, called after large_sep_kernel(..., is_training=True) on a
    detector built with large_sep_train=True: d_feat = head_backward(..., to_feat=True)['feat'] (d loss / d feat, with the
    `feat` buffer's shape and ld) goes through the batch norm and its ReLU (xdet_batch_norm_backward on the kept z, masked
    by the net's own `feat`), then through the merged (1,15) conv (xdet_conv_backward, x = the kept t) and the merged (15,1)
    conv (x = the net's `out`) -- three calls on the detector's stream with no host round trip in between.  -> a dict with the
    ten gradients under the checkpoint's variable names and in its shapes (the merged tensors split back; both conv2d_1
    biases get the merged bias gradient), 'out': d loss / d out as a DeviceTensor [N,h,w,2048] with `out`'s ld, 'z':
    d loss / d z [N,h,w,co] and 't': d loss / d t [N,h,w,2*mid] (what the first conv backward read)."""
    from . import ops
    d = _det()
    if not d.large_sep_train:
        raise InvalidArgumentError(-1, 'large_sep_backward: needs a detector built with large_sep_train=True')
    s = d._lsep
    n = s['n']
    if not n:
        raise InvalidArgumentError(-1, 'large_sep_backward: call large_sep_kernel(..., is_training=True) first')
    feat, out = d.buffer('feat', n), d.buffer('out', n)
    if not isinstance(d_feat, DeviceTensor) or tuple(d_feat.shape) != tuple(feat.shape) or d_feat.ld != feat.ld:
        raise InvalidArgumentError(-1, 'large_sep_backward: d_feat must be a DeviceTensor of shape %r with ld %d, got %r'
                                   % (tuple(feat.shape), feat.ld, (getattr(d_feat, 'shape', None), getattr(d_feat, 'ld', None))))
    saved = d.large_sep_saved()
    dz, dgamma, dbeta = ops.batch_norm_backward_device(saved['z'], feat, d_feat, s['gamma'], s['save_mean'], s['save_invstd'],
                                                       True, stream=d.stream)
    dt, dkb, dbb = ops.conv_backward_device(saved['t'], s['K_b'], dz, None, stream=d.stream)
    d_out, dka, dba = ops.conv_backward_device(out, s['K_a'], dt, None, stream=d.stream)
    _sync(d)
    co, mid2 = s['K_b'].shape[3], s['K_a'].shape[3]
    grads = split_large_sep_grads(to_host(dka.ptr, s['K_a'].shape), to_host(dba.ptr, (mid2,)), to_host(dkb.ptr, s['K_b'].shape),
                                  to_host(dbb.ptr, (co,)), s['mid'])
    grads['large_sep_feature/batch_normalization/gamma'] = to_host(dgamma.ptr, (co,))
    grads['large_sep_feature/batch_normalization/beta'] = to_host(dbeta.ptr, (co,))
    grads['out'], grads['z'], grads['t'] = d_out, dz, dt
    return grads


def exit_flow_train():
    """The Xception exit flow in training mode (net/xception_body.py:339-376), called after XceptionBody(...,
    is_training=False) on a detector built with exit_flow_train=True: the exit flow is computed again from the net's `mid_x`
    buffer with batch statistics -- per separable unit xdet_depthwise_forward, the 1x1 conv (xdet_conv_forward, split
    precision, f32 out) and xdet_batch_norm_forward in training mode (eps 1e-4, momentum 0.99, the ReLU inside where the graph
    has one, the moving statistics updated on their device copies) --

        r  = BN4(conv2d_4(mid_x))                          a  = BN(pw(dw(relu(mid_x))))
        b2 = BN(pw(dw(relu(a)))) + r   (xdet_add_rows)     c3 = relu(BN(pw(dw_dil2(b2))))     out = relu(BN(pw(dw_dil2(c3))))

    all on the detector's stream with no host round trip; the last batch norm writes straight into the net's `out` buffer
    (with its ld), so large_sep_kernel(..., is_training=True), get_head, head_backward and large_sep_backward go on unchanged.
    `mid_x` is not written: get_rpn is unaffected.  What exit_flow_backward needs stays on the device
    (detector.exit_flow_saved()).  -> `out` [N,h,w,2048]."""
    d = _det()
    if not d.exit_flow_train:
        raise InvalidArgumentError(-1, 'exit_flow_train: needs a detector built with exit_flow_train=True (the default detector '
                                       'folds the moving statistics into the conv weights)')
    n = d._N
    if not n:
        raise InvalidArgumentError(-1, 'exit_flow_train: call XceptionBody(..., is_training=False) first')
    e, h, l = d._exit, d.stream.handle, lib()
    mid_x, out = d.buffer('mid_x', n), d.buffer('out', n)
    _, H, W, _ = mid_x.shape
    M = n * H * W

    p = e['proj']
    check(l.xdet_conv_forward(p['conv'].handle, mid_x.ptr, n, H, W, mid_x.ld, p['z'].ptr, p['z'].ld, None, 0, h))
    _bn_train_forward(d, p['bn'], p['z'], False, p['r'], M, e['ws_bn'])
    x = mid_x
    for i, u in enumerate(e['units']):
        y = u.get('y', out)
        _unit_forward(d, u, x, y, n, H, W, e['ws_bn'])
        if i == 1:                                   # block13's residual add behind its second batch norm
            check(l.xdet_add_rows(y.ptr, y.ld, p['r'].ptr, p['r'].ld, e['b2'].ptr, e['b2'].ld, M, y.shape[3], h))
            y = e['b2']
        x = y
    e['n'] = n
    _sync(d)
    return out


def exit_flow_backward(d_out, d_mid=None):
    """The backward of the exit flow in training mode, called after exit_flow_train() on a detector built with
    exit_flow_train=True: d_out = large_sep_backward(...)['out'] (d loss / d out, with the `out` buffer's shape and ld) and
    optionally d_mid = rpn_backward(...)['mid'] (the RPN branch's share of d loss / d mid_x, with `mid_x`'s shape and ld).  Per
    separable unit, last to first: xdet_batch_norm_backward on the kept BN input (masked by the unit's own output where the
    graph has a ReLU: the net's `out`, the kept c3), xdet_conv_backward at 1x1 on the kept depthwise output, then
    xdet_depthwise_backward (dilation 2 in block14; relu_in on `a` and on `mid_x` in block13).  d loss / d b2 feeds both
    batch_normalization_4's backward, whose conv_backward on `mid_x` gives share A, and block13's two units, which give share
    B; the call ends with d loss / d mid_x = (B + A) + d_mid, in that order, by xdet_add_rows -- everything on the detector's
    stream with no host round trip.  The bias gradient xdet_conv_backward insists on is computed and dropped: these convs
    have none.  -> a dict with the 19 gradients under the checkpoint's variable names and in its shapes
    (EXIT_FLOW_VARIABLES, NumPy), 'mid': d loss / d mid_x as a DeviceTensor [N,h,w,728] with `mid_x`'s ld, its addends
    'mid_A' and 'mid_B', and the intermediate gradients 'b2', 'c3', 'a' and 'r' (d loss / d r is d loss / d b2: the same
    tensor), 'dw/<unit>' = d loss / d (the unit's depthwise output) and 'z/<unit>', 'z/conv2d_4' = d loss / d (a batch norm's
    input) likewise."""
    from . import ops
    d = _det()
    if not d.exit_flow_train:
        raise InvalidArgumentError(-1, 'exit_flow_backward: needs a detector built with exit_flow_train=True')
    e = d._exit
    n = e['n']
    if not n:
        raise InvalidArgumentError(-1, 'exit_flow_backward: call exit_flow_train() first')
    out, mid_x = d.buffer('out', n), d.buffer('mid_x', n)
    for what, t, like in (('d_out', d_out, out), ('d_mid', d_mid, mid_x)):
        if t is None and what == 'd_mid':
            continue
        if not isinstance(t, DeviceTensor) or tuple(t.shape) != tuple(like.shape) or t.ld != like.ld:
            raise InvalidArgumentError(-1, 'exit_flow_backward: %s must be a DeviceTensor of shape %r with ld %d, got %r'
                                       % (what, tuple(like.shape), like.ld, (getattr(t, 'shape', None), getattr(t, 'ld', None))))
    saved = d.exit_flow_saved()
    grads, dev = {}, {}

    def unit_backward(u, x, y, dy):
        """-> d loss / d x through BN (masked by y), the 1x1 conv and the depthwise conv"""
        name = u['name']
        dx, dt, dz = _unit_backward(d, u, x, y, dy, saved[name + '/z'], saved[name + '/dw'], dev, e['ws_dw'])
        grads['dw/' + name], grads['z/' + name] = dt, dz
        return dx
    u1, u2, u3, u4 = e['units']
    d_c3 = unit_backward(u4, saved['c3'], out, d_out)
    d_b2 = unit_backward(u3, saved['b2'], saved['c3'], d_c3)
    p = e['proj']
    dzr, dgamma, dbeta = ops.batch_norm_backward_device(saved['conv2d_4/z'], None, d_b2, p['bn']['gamma'], p['bn']['save_mean'],
                                                        p['bn']['save_invstd'], True, stream=d.stream)
    share_a, dk4, _ = ops.conv_backward_device(mid_x, p['K'], dzr, None, relu_in=False, stream=d.stream)
    co = p['K'].shape[3]
    dev['conv2d_4/kernel'] = (dk4, p['K'].shape)
    dev['batch_normalization_4/gamma'], dev['batch_normalization_4/beta'] = (dgamma, (co,)), (dbeta, (co,))
    d_a = unit_backward(u2, saved['a'], None, d_b2)
    share_b = unit_backward(u1, mid_x, None, d_a)
    mid = ops.add_rows_device(share_b, share_a, stream=d.stream)
    if d_mid is not None:
        ops.add_rows_device(mid, d_mid, out=mid, stream=d.stream)
    _sync(d)
    for k, (buf, shape) in dev.items():
        grads[k] = to_host(buf.ptr, shape)
    grads.update({'mid': mid, 'mid_A': share_a, 'mid_B': share_b, 'b2': d_b2, 'r': d_b2, 'c3': d_c3, 'a': d_a, 'z/conv2d_4': dzr})
    return grads


def middle_flow_train():
    """The Xception middle flow in training mode (net/xception_body.py:328-337), called after XceptionBody(...,
    is_training=False) on a detector built with middle_flow_train=True: blocks 5-12 are computed again from the net's `entry_x`
    buffer with batch statistics, per block

        y1 = BN(pw(dw(relu(x))))    y2 = BN(pw(dw(relu(y1))))    y3 = BN(pw(dw(relu(y2))))    x' = y3 + x   (xdet_add_rows)

    -- per unit xdet_depthwise_forward, the 1x1 conv (xdet_conv_forward, split precision, f32 out) and
    xdet_batch_norm_forward in training mode (eps 1e-4, momentum 0.99, the moving statistics updated on their device copies);
    the third batch norm writes the block's output tensor and the add runs on it in place; block 12's is the net's `mid_x`
    (with its ld).  Then xdet_net_mid_refresh re-derives what the net keeps of `mid_x` -- the ReLU split planes the RPN's 3x3
    conv reads and the `mid` buffer -- so get_rpn, rpn_backward and exit_flow_train all see the training-mode tensor.  24 x 3
    calls, 8 adds and the refresh on the detector's stream with no host round trip; `entry_x` is not written.  The exit flow's
    saved state is dropped: exit_flow_backward refuses until exit_flow_train() has run on the new `mid_x`.  What
    middle_flow_backward needs stays on the device (detector.middle_flow_saved()).  -> `mid` [N,h,w,728], the tensor get_rpn
    accepts."""
    d = _det()
    if not d.middle_flow_train:
        raise InvalidArgumentError(-1, 'middle_flow_train: needs a detector built with middle_flow_train=True (the default '
                                       'detector folds the moving statistics into the conv weights and keeps no entry_x)')
    n = d._N
    if not n:
        raise InvalidArgumentError(-1, 'middle_flow_train: call XceptionBody(..., is_training=False) first')
    m, h, l = d._middle, d.stream.handle, lib()
    x, mid_x = d.buffer('entry_x', n), d.buffer('mid_x', n)
    _, H, W, C = x.shape
    for blk in m['blocks']:
        u1, u2, u3 = blk['units']
        out = blk['out'] if blk['out'] is not None else mid_x
        _unit_forward(d, u1, x, u1['y'], n, H, W, m['ws_bn'])
        _unit_forward(d, u2, u1['y'], u2['y'], n, H, W, m['ws_bn'])
        _unit_forward(d, u3, u2['y'], out, n, H, W, m['ws_bn'])
        check(l.xdet_add_rows(out.ptr, out.ld, x.ptr, x.ld, out.ptr, out.ld, n * H * W, C, h))
        x = out
    check(l.xdet_net_mid_refresh(d.handle, n, h))
    m['n'] = n
    d._exit['n'] = 0                                 # what exit_flow_train saved belongs to another mid_x
    _sync(d)
    return d.buffer('mid', n)


def middle_flow_backward(d_mid, intermediates=False):
    """The backward of the middle flow in training mode, called after middle_flow_train() on a detector built with
    middle_flow_train=True: d_mid = exit_flow_backward(...)['mid'] (d loss / d mid_x, with `mid_x`'s shape and ld).  From
    block 12 back to block 5, with g = the gradient of the block's output, y1, y2 the kept batch norm outputs and x the
    block's input:

        d3 = unit_backward(u3, y2, g)    d2 = unit_backward(u2, y1, d3)    d1 = unit_backward(u1, x, d2)
        g' = d1 + g   (xdet_add_rows, in that order)

    where unit_backward is the exit flow's: xdet_batch_norm_backward on the kept BN input (no mask: these units end without a
    ReLU), xdet_conv_backward at 1x1 on the kept depthwise output (its bias gradient computed and dropped), then
    xdet_depthwise_backward with relu_in.  24 x 3 calls and 8 adds on the detector's stream, no float atomics, no host round trip
    until the end: the gradients inside a block go through four tensors the detector owns, the workspaces are the detector's,
    and what the call returns on the device is allocated in front of the first launch.  -> a dict with the 96 gradients under
    the checkpoint's variable names and in its shapes (MIDDLE_FLOW_VARIABLES, NumPy), 'entry': d loss / d entry_x as a
    DeviceTensor [N,h,w,728] with `entry_x`'s ld, and 'x6' ... 'x12': the gradients at the block boundaries ('x<b>' = d loss /
    d (block b's input)).  intermediates=True: also 'dw/<unit>' = d loss / d (the unit's depthwise output), 'z/<unit>' =
    d loss / d (its batch norm's input) and 'd3/block<b>', 'd2/block<b>', 'd1/block<b>' (the units' input gradients; d1 is the
    addend of the join), each in a tensor of its own."""
    d = _det()
    if not d.middle_flow_train:
        raise InvalidArgumentError(-1, 'middle_flow_backward: needs a detector built with middle_flow_train=True')
    m = d._middle
    n = m['n']
    if not n:
        raise InvalidArgumentError(-1, 'middle_flow_backward: call middle_flow_train() first')
    mid_x, entry = d.buffer('mid_x', n), d.buffer('entry_x', n)
    if not isinstance(d_mid, DeviceTensor) or tuple(d_mid.shape) != tuple(mid_x.shape) or d_mid.ld != mid_x.ld:
        raise InvalidArgumentError(-1, 'middle_flow_backward: d_mid must be a DeviceTensor of shape %r with ld %d, got %r'
                                   % (tuple(mid_x.shape), mid_x.ld, (getattr(d_mid, 'shape', None), getattr(d_mid, 'ld', None))))
    from . import ops
    saved = d.middle_flow_saved()
    view = lambda t: DeviceTensor(t.ptr, (n,) + tuple(t.shape[1:]), t.ld, owner=t)
    rot = {k: view(t) for k, t in m['rot'].items()}
    shape = tuple(entry.shape)
    # everything the call returns on the device, allocated ahead of the launches
    grads = {('x%d' % blk['b'] if blk['b'] != MIDDLE_FLOW_BLOCKS[0] else 'entry'): DeviceTensor.empty(shape, ld=entry.ld)
             for blk in m['blocks']}
    if intermediates:
        for blk in m['blocks']:
            for i, u in enumerate(blk['units']):
                grads['d%d/block%d' % (i + 1, blk['b'])] = DeviceTensor.empty(shape, ld=entry.ld)
                grads['dw/' + u['name']], grads['z/' + u['name']] = DeviceTensor.empty(shape), DeviceTensor.empty(shape)
    dev, g = {}, d_mid
    for blk in reversed(m['blocks']):
        b = blk['b']
        u1, u2, u3 = blk['units']
        x, y1, y2 = saved['x%d' % b], saved['block%d/y1' % b], saved['block%d/y2' % b]
        dy = g
        # the three unit gradients alternate between two tensors: a unit's dx is read by the next unit's BN backward only
        for i, u, xin, dst in ((3, u3, y2, 'da'), (2, u2, y1, 'db'), (1, u1, x, 'da')):
            into = {'ws_bn': m['ws_bn'], 'ws_conv': m['ws_conv'], 'dz': rot['dz'], 'dt': rot['dt'], 'dx': rot[dst]}
            if intermediates:
                into.update(dz=grads['z/' + u['name']], dt=grads['dw/' + u['name']], dx=grads['d%d/block%d' % (i, b)])
            dy, _, _ = _unit_backward(d, u, xin, None, dy, saved[u['name'] + '/z'], saved[u['name'] + '/dw'], dev, m['ws_dw'], into)
        g = ops.add_rows_device(dy, g, out=grads['x%d' % b if b != MIDDLE_FLOW_BLOCKS[0] else 'entry'], stream=d.stream)
    _sync(d)
    for t in list(rot.values()) + list(grads.values()):       # the stream has run every call: nothing needs keeping alive, and
        t._keep = None                                         # the wrappers' references form a ring through the rotating views
    for k, (buf, shp) in dev.items():
        grads[k] = to_host(buf.ptr, shp)
    return grads


def entry_flow_train():
    """Blocks 2-4 of the Xception entry flow in training mode (net/xception_body.py:260-326), called after XceptionBody(...,
    is_training=False) on a detector built with entry_flow_train=True: the three blocks are computed again from the net's
    `stem_out` buffer with batch statistics, per block with x its input

        xs = subsample2(x)   (xdet_subsample2)        r  = BN(conv1x1(xs))
        y1 = BN(pw(dw(relu?(x))))                     y2 = BN(pw(dw(relu(y1))))       (no ReLU in front of block2_sepconv1)
        x' = maxpool3x3s2(y2) + r                     (xdet_maxpool3x3s2_add)

    -- the convs by xdet_depthwise_forward and xdet_conv_forward (split precision, f32 out), the batch norms by
    xdet_batch_norm_forward in training mode (eps 1e-4, momentum 0.99, the moving statistics updated on their device copies);
    block 4's x' is written into the net's `entry_x` (with its ld).  33 calls on the detector's stream with no host round
    trip; `stem_out` is not written.  The middle and the exit flow's saved state is dropped: their backwards refuse until
    middle_flow_train() / exit_flow_train() have run on the new tensors.  What entry_flow_backward needs stays on the device
    (detector.entry_flow_saved()).  -> `entry_x` [N,h,w,728]."""
    d = _det()
    if not getattr(d, 'entry_flow_train', False):
        raise InvalidArgumentError(-1, 'entry_flow_train: needs a detector built with entry_flow_train=True (the default detector '
                                       'folds the moving statistics into the conv weights and keeps no stem_out)')
    n = d._N
    if not n:
        raise InvalidArgumentError(-1, 'entry_flow_train: call XceptionBody(..., is_training=False) first')
    e, h, l = d._entry, d.stream.handle, lib()
    x = d.buffer('stem_out', n)
    for blk in e['blocks']:
        (u1, u2), p, xs = blk['units'], blk['proj'], blk['xs']
        H, W, cin, c = blk['H'], blk['W'], blk['cin'], blk['c']
        Ho, Wo = -(-H // 2), -(-W // 2)
        out = blk['out'] if blk['out'] is not None else d.buffer('entry_x', n)
        check(l.xdet_subsample2(x.ptr, x.ld, n, H, W, cin, xs.ptr, xs.ld, h))
        check(l.xdet_conv_forward(p['conv'].handle, xs.ptr, n, Ho, Wo, xs.ld, p['z'].ptr, p['z'].ld, None, 0, h))
        _bn_train_forward(d, p['bn'], p['z'], False, p['r'], n * Ho * Wo, e['ws_bn'])
        _unit_forward(d, u1, x, u1['y'], n, H, W, e['ws_bn'])
        _unit_forward(d, u2, u1['y'], u2['y'], n, H, W, e['ws_bn'])
        y2, r = u2['y'], p['r']
        if not (y2.ld == r.ld == out.ld):
            raise XdetError(-3, 'entry_flow_train: pixel strides %r of y2, r and the block output differ' % ((y2.ld, r.ld, out.ld),))
        check(l.xdet_maxpool3x3s2_add(y2.ptr, r.ptr, out.ptr, n, H, W, c, y2.ld, h))
        x = out
    e['n'] = n
    d._middle['n'] = 0                               # what the later flows saved belongs to another entry_x
    d._exit['n'] = 0
    _sync(d)
    return d.buffer('entry_x', n)


def entry_flow_backward(d_entry, intermediates=False):
    """The backward of blocks 2-4 in training mode, called after entry_flow_train() on a detector built with
    entry_flow_train=True: d_entry = middle_flow_backward(...)['entry'] (d loss / d entry_x, with `entry_x`'s shape and ld).
    From block 4 back to block 2, with g the gradient of the block's output, x the block's input and y1, y2 the kept batch
    norm outputs:

        dzr = BN_backward(proj, g)       dxs, dK = conv_backward(xs, K, dzr)          (the bias gradient is dropped)
        dy2 = maxpool_backward(y2, g)    (xdet_maxpool3x3s2_backward)
        d2  = unit_backward(u2, y1, dy2)       d1 = unit_backward(u1, x, d2)
        g'  = add_upsample2(d1, dxs)     (xdet_add_upsample2: the shortcut's share lands on the even pixels)

    where unit_backward is the other flows': xdet_batch_norm_backward, xdet_conv_backward at 1x1, xdet_depthwise_backward.
    Everything runs on the detector's stream with no host round trip until the end and no float atomics; the gradients inside
    a block go through tensors the detector owns, the workspaces are the detector's, and what the call returns on the device
    is allocated in front of the first launch.  -> a dict with the 33 gradients under the checkpoint's variable names and in
    its shapes (ENTRY_FLOW_VARIABLES, NumPy), 'stem': d loss / d stem_out as a DeviceTensor [N,h,w,64] with `stem_out`'s ld, and
    'x3', 'x4': the gradients at the block boundaries ('x<b>' = d loss / d (block b's input)).  intermediates=True: also
    'dxs/block<b>', 'z/conv2d_<b-1>' (dzr), 'dy2/block<b>', 'd2/block<b>', 'd1/block<b>' and per unit 'dw/<unit>' =
    d loss / d (its depthwise output), 'z/<unit>' = d loss / d (its batch norm's input), each in a tensor of its own."""
    d = _det()
    if not getattr(d, 'entry_flow_train', False):
        raise InvalidArgumentError(-1, 'entry_flow_backward: needs a detector built with entry_flow_train=True')
    e = d._entry
    n = e['n']
    if not n:
        raise InvalidArgumentError(-1, 'entry_flow_backward: call entry_flow_train() first')
    entry = d.buffer('entry_x', n)
    if not isinstance(d_entry, DeviceTensor) or tuple(d_entry.shape) != tuple(entry.shape) or d_entry.ld != entry.ld:
        raise InvalidArgumentError(-1, 'entry_flow_backward: d_entry must be a DeviceTensor of shape %r with ld %d, got %r'
                                   % (tuple(entry.shape), entry.ld, (getattr(d_entry, 'shape', None), getattr(d_entry, 'ld', None))))
    from . import ops
    saved = d.entry_flow_saved()
    view = lambda t: DeviceTensor(t.ptr, (n,) + tuple(t.shape[1:]), t.ld, owner=t)
    first = ENTRY_FLOW_BLOCKS[0]
    # everything the call returns on the device, allocated ahead of the launches
    grads, inner = {}, {}
    for blk in e['blocks']:
        b, x = blk['b'], saved['x%d' % blk['b']]
        grads['stem' if b == first else 'x%d' % b] = DeviceTensor.empty(tuple(x.shape), ld=x.ld)
        rot = {k: view(t) for k, t in blk['rot'].items()}
        if intermediates:
            u1, u2 = blk['units']
            names = {'dzr': 'z/' + blk['proj']['name'], 'dxs': 'dxs/block%d' % b, 'dy2': 'dy2/block%d' % b, 'd2': 'd2/block%d' % b,
                     'd1': 'd1/block%d' % b, 'dt2': 'dw/' + u2['name'], 'dt1': 'dw/' + u1['name'], 'dz': 'z/' + u2['name'],
                     'dz1': 'z/' + u1['name']}
            rot['dz1'] = rot['dz']
            for k, key in names.items():
                grads[key] = rot[k] = DeviceTensor.empty(tuple(rot[k].shape), ld=rot[k].ld)
        else:
            rot['dz1'] = rot['dz']
        inner[b] = rot
    dev, g = {}, d_entry
    for blk in reversed(e['blocks']):
        b, p, rot = blk['b'], blk['proj'], inner[blk['b']]
        u1, u2 = blk['units']
        x, y1, y2 = saved['x%d' % b], saved['block%d/y1' % b], saved['block%d/y2' % b]
        dzr, dgamma, dbeta = ops.batch_norm_backward_device(saved[p['name'] + '/z'], None, g, p['bn']['gamma'], p['bn']['save_mean'],
                                                            p['bn']['save_invstd'], True, stream=d.stream, dx=rot['dzr'],
                                                            workspace=e['ws_bn'])
        dxs, dk, _ = ops.conv_backward_device(saved['block%d/xs' % b], p['K'], dzr, None, stream=d.stream, dx=rot['dxs'],
                                              workspace=e['ws_conv'])
        c = p['K'].shape[3]
        dev[p['name'] + '/kernel'] = (dk, p['K'].shape)
        dev[p['bn_name'] + '/gamma'], dev[p['bn_name'] + '/beta'] = (dgamma, (c,)), (dbeta, (c,))
        dy2 = ops.max_pool_backward_device(y2, g, dx=rot['dy2'], stream=d.stream)
        ws = {'ws_bn': e['ws_bn'], 'ws_conv': e['ws_conv']}
        d2, _, _ = _unit_backward(d, u2, y1, None, dy2, saved[u2['name'] + '/z'], saved[u2['name'] + '/dw'], dev, e['ws_dw'],
                                  dict(ws, dz=rot['dz'], dt=rot['dt2'], dx=rot['d2']))
        d1, _, _ = _unit_backward(d, u1, x, None, d2, saved[u1['name'] + '/z'], saved[u1['name'] + '/dw'], dev, e['ws_dw'],
                                  dict(ws, dz=rot['dz1'], dt=rot['dt1'], dx=rot['d1']))
        g = ops.add_upsample2_device(d1, dxs, out=grads['stem' if b == first else 'x%d' % b], stream=d.stream)
    _sync(d)
    for t in [t for rot in inner.values() for t in rot.values()] + list(grads.values()):   # the stream has run every call: nothing
        t._keep = None                                                                      # needs keeping alive any longer
    for k, (buf, shp) in dev.items():
        grads[k] = to_host(buf.ptr, shp)
    return grads


# ---- the middle flow's host statements: NumPy, any channel count (the weights decide), float64 as the yardstick ----------

def _host_depthwise_forward(x, k, relu_in, dtype):
    x, k = np.asarray(x, dtype), np.asarray(k, dtype)
    N, H, W, C = x.shape
    xp = np.pad(np.maximum(x, dtype(0)) if relu_in else x, ((0, 0), (1, 1), (1, 1), (0, 0)))
    out = np.zeros(x.shape, dtype)
    for a in range(3):
        for b in range(3):
            out += xp[:, a:a + H, b:b + W] * k[a, b, :, 0]
    return out


def host_middle_flow_train(entry_x, weights, dtype=np.float64, blocks=MIDDLE_FLOW_BLOCKS):
    """The NumPy statement of middle_flow_train: entry_x [N,h,w,C] and the blocks' variables and moving statistics under the
    checkpoint's names (C comes from the weights) -> (mid_x, saved): the output of the last block and a dict with
    detector.middle_flow_saved()'s keys for `blocks` -- 'x<b>', '<unit>/dw', '<unit>/z', 'block<b>/y1', 'block<b>/y2', and per
    batch norm '/save_mean', '/save_invstd', '/moving_mean', '/moving_variance' [C] (the moving ones after TensorFlow's
    update as ops.host_batch_norm_forward states it) -- plus 'block<b>/y3'."""
    from . import ops
    x, saved = np.asarray(entry_x, dtype), {}
    for b in blocks:
        saved['x%d' % b] = x
        y = x
        for i in (1, 2, 3):
            u = 'block%d_sepconv%d' % (b, i)
            t = _host_depthwise_forward(y, weights[u + '/depthwise_kernel'], True, dtype)
            z = np.matmul(t, np.asarray(weights[u + '/pointwise_kernel'], dtype)[0, 0])
            bn = u + '_bn/'
            y, mean, invstd, mm, mv = ops.host_batch_norm_forward(z, weights[bn + 'gamma'], weights[bn + 'beta'], MIDDLE_FLOW_EPS,
                                                                  True, MIDDLE_FLOW_MOMENTUM, weights[bn + 'moving_mean'],
                                                                  weights[bn + 'moving_variance'], False, dtype)
            saved[u + '/dw'], saved[u + '/z'], saved['block%d/y%d' % (b, i)] = t, z, y
            saved.update({bn + 'save_mean': mean, bn + 'save_invstd': invstd, bn + 'moving_mean': mm, bn + 'moving_variance': mv})
        x = y + x
    return x, saved


def host_middle_flow_backward(saved, weights, d_mid, dtype=np.float64, blocks=MIDDLE_FLOW_BLOCKS):
    """The NumPy statement of middle_flow_backward(d_mid, intermediates=True): saved = what host_middle_flow_train (or
    detector.middle_flow_saved(), as NumPy arrays) left, d_mid = d loss / d (the last block's output) -> a dict with the four
    gradients of every unit of `blocks` under the checkpoint's names and in its shapes, 'entry' = d loss / d (the first block's
    input), 'x<b>' for every later block, 'dw/<unit>', 'z/<unit>' and 'd3/block<b>', 'd2/block<b>', 'd1/block<b>'.  Composed of ops.host_batch_norm_backward,
    ops.host_conv_backward and ops.host_depthwise_backward."""
    from . import ops
    blocks = tuple(blocks)
    vec = lambda a: np.asarray(a, dtype).reshape(-1)
    g, out = np.asarray(d_mid, dtype), {}
    for b in reversed(blocks):
        dy = g
        for i, xin in ((3, saved['block%d/y2' % b]), (2, saved['block%d/y1' % b]), (1, saved['x%d' % b])):
            u = 'block%d_sepconv%d' % (b, i)
            bn = u + '_bn/'
            dz, dgamma, dbeta = ops.host_batch_norm_backward(saved[u + '/z'], None, dy, weights[bn + 'gamma'], vec(saved[bn + 'save_mean']),
                                                             vec(saved[bn + 'save_invstd']), True, dtype)
            dt, dkp, _ = ops.host_conv_backward(saved[u + '/dw'], weights[u + '/pointwise_kernel'], dz, None, False, dtype)
            dy, dkd = ops.host_depthwise_backward(xin, weights[u + '/depthwise_kernel'], dt, 1, True, dtype)
            out[u + '/depthwise_kernel'], out[u + '/pointwise_kernel'], out[bn + 'gamma'], out[bn + 'beta'] = dkd, dkp, dgamma, dbeta
            out['dw/' + u], out['z/' + u], out['d%d/block%d' % (i, b)] = dt, dz, dy
        g = dy + g
        out['entry' if b == blocks[0] else 'x%d' % b] = g
    return out


# ---- the entry flow's host statements: NumPy, any channel counts and map sizes (the weights and the input decide) ---------

def _host_max_pool_forward(x, dtype):
    """max_pooling2d(3, 2, 'same') of x [N,H,W,C]: padded positions are absent"""
    from .ops import _same_pad_front
    x = np.asarray(x, dtype)
    N, H, W, C = x.shape
    (Ho, pt), (Wo, pl) = _same_pad_front(H), _same_pad_front(W)
    xp = np.full((N, 2 * Ho + 1, 2 * Wo + 1, C), -np.inf, dtype)
    xp[:, pt:pt + H, pl:pl + W] = x
    out = np.full((N, Ho, Wo, C), -np.inf, dtype)
    for a in range(3):
        for b in range(3):
            out = np.maximum(out, xp[:, a:a + 2 * Ho:2, b:b + 2 * Wo:2])
    return out


def host_entry_flow_train(stem_out, weights, dtype=np.float64, blocks=ENTRY_FLOW_BLOCKS):
    """The NumPy statement of entry_flow_train: stem_out [N,h,w,C] (the first block's input) and the blocks' variables and
    moving statistics under the checkpoint's names (the channel counts come from the weights) -> (entry_x, saved): the output
    of the last block and a dict with detector.entry_flow_saved()'s keys for `blocks` -- 'x<b>', 'block<b>/xs',
    'conv2d_<b-1>/z', 'block<b>/r', '<unit>/dw', '<unit>/z', 'block<b>/y1', 'block<b>/y2', and per batch norm '/save_mean',
    '/save_invstd', '/moving_mean', '/moving_variance' [C] (the moving ones after TensorFlow's update as
    ops.host_batch_norm_forward states it)."""
    from . import ops
    x, saved = np.asarray(stem_out, dtype), {}

    def bn_forward(z, bn):
        y, mean, invstd, mm, mv = ops.host_batch_norm_forward(z, weights[bn + 'gamma'], weights[bn + 'beta'], ENTRY_FLOW_EPS, True,
                                                              ENTRY_FLOW_MOMENTUM, weights[bn + 'moving_mean'],
                                                              weights[bn + 'moving_variance'], False, dtype)
        saved.update({bn + 'save_mean': mean, bn + 'save_invstd': invstd, bn + 'moving_mean': mm, bn + 'moving_variance': mv})
        return y
    for b in blocks:
        saved['x%d' % b] = x
        proj = 'conv2d_%d' % (b - 1)
        xs = ops.host_subsample2(x, dtype)
        zr = np.matmul(xs, np.asarray(weights[proj + '/kernel'], dtype)[0, 0])
        r = bn_forward(zr, 'batch_normalization_%d/' % (b - 1))
        saved['block%d/xs' % b], saved[proj + '/z'], saved['block%d/r' % b] = xs, zr, r
        y = x
        for i in (1, 2):
            u = 'block%d_sepconv%d' % (b, i)
            t = _host_depthwise_forward(y, weights[u + '/depthwise_kernel'], _entry_relu_in(b, i), dtype)
            z = np.matmul(t, np.asarray(weights[u + '/pointwise_kernel'], dtype)[0, 0])
            y = bn_forward(z, u + '_bn/')
            saved[u + '/dw'], saved[u + '/z'], saved['block%d/y%d' % (b, i)] = t, z, y
        x = _host_max_pool_forward(y, dtype) + r
    saved['x%d' % (blocks[-1] + 1)] = x
    return x, saved


def host_entry_flow_backward(saved, weights, d_entry, dtype=np.float64, blocks=ENTRY_FLOW_BLOCKS):
    """The NumPy statement of entry_flow_backward(d_entry, intermediates=True): saved = what host_entry_flow_train (or
    detector.entry_flow_saved(), as NumPy arrays) left, d_entry = d loss / d (the last block's output) -> a dict with the eleven
    gradients of every block of `blocks` under the checkpoint's names and in its shapes, 'stem' = d loss / d (the first block's
    input), 'x<b>' for every later block, and 'dxs/block<b>', 'z/conv2d_<b-1>', 'dy2/block<b>', 'd2/block<b>', 'd1/block<b>',
    'dw/<unit>', 'z/<unit>'.  Composed of ops.host_batch_norm_backward, ops.host_conv_backward, ops.host_depthwise_backward,
    ops.host_max_pool_backward and ops.host_add_upsample2."""
    from . import ops
    blocks = tuple(blocks)
    vec = lambda a: np.asarray(a, dtype).reshape(-1)
    g, out = np.asarray(d_entry, dtype), {}
    for b in reversed(blocks):
        proj, bn = 'conv2d_%d' % (b - 1), 'batch_normalization_%d/' % (b - 1)
        dzr, dgamma, dbeta = ops.host_batch_norm_backward(saved[proj + '/z'], None, g, weights[bn + 'gamma'], vec(saved[bn + 'save_mean']),
                                                          vec(saved[bn + 'save_invstd']), True, dtype)
        dxs, dk, _ = ops.host_conv_backward(saved['block%d/xs' % b], weights[proj + '/kernel'], dzr, None, False, dtype)
        out[proj + '/kernel'], out[bn + 'gamma'], out[bn + 'beta'] = dk, dgamma, dbeta
        out['z/' + proj], out['dxs/block%d' % b] = dzr, dxs
        dy = ops.host_max_pool_backward(saved['block%d/y2' % b], g, dtype)
        out['dy2/block%d' % b] = dy
        for i, xin in ((2, saved['block%d/y1' % b]), (1, saved['x%d' % b])):
            u = 'block%d_sepconv%d' % (b, i)
            ubn = u + '_bn/'
            dz, dgamma, dbeta = ops.host_batch_norm_backward(saved[u + '/z'], None, dy, weights[ubn + 'gamma'], vec(saved[ubn + 'save_mean']),
                                                             vec(saved[ubn + 'save_invstd']), True, dtype)
            dt, dkp, _ = ops.host_conv_backward(saved[u + '/dw'], weights[u + '/pointwise_kernel'], dz, None, False, dtype)
            dy, dkd = ops.host_depthwise_backward(xin, weights[u + '/depthwise_kernel'], dt, 1, _entry_relu_in(b, i), dtype)
            out[u + '/depthwise_kernel'], out[u + '/pointwise_kernel'], out[ubn + 'gamma'], out[ubn + 'beta'] = dkd, dkp, dgamma, dbeta
            out['dw/' + u], out['z/' + u], out['d%d/block%d' % (i, b)] = dt, dz, dy
        g = ops.host_add_upsample2(dy, dxs, dtype)
        out['stem' if b == blocks[0] else 'x%d' % b] = g
    return out
