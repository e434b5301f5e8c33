"""The training graph of the Light-Head R-CNN net: what `xdet.model` re-exports under the training names.

Four stages can be rebuilt in training mode (batch statistics, moving-average updates, a backward), each consuming what the one
above it writes: the large-separable block <- the exit flow <- the middle flow <- blocks 2-4 of the entry flow (`STAGES`).  A
detector built with a stage's flag keeps one state object for it (`LargeSepState`, `ExitFlowState`, `MiddleFlowState`,
`EntryFlowState`), made of `BatchNorm`, `SepUnit` and `Projection`; the module-level functions run a stage of the detector
that is current (`with det.scope():`).  The stem -- the two convs in front of block 2 -- is a fifth stage that stands next to
the table (`STEM_STAGE`, `StemState`): it feeds all four.  The head's and the RPN head's backward (`head_backward`, `rpn_backward`) and the NumPy
statements of the middle and the entry flow (`host_*`) live here too, and the optimizer step over the three flows' variables
and, at reach='all', the large-separable block's and both heads' (`MomentumOptimizer`, `piecewise_learning_rate`).
"""
import collections
import contextlib
import math

import numpy as np

from . import train_ops, ops
from ._lib import lib, check, XdetError, InvalidArgumentError, MomentumSlot
from .runtime import DeviceBuffer, DeviceTensor, PinnedBuffer, Event, to_device, to_host, get_precision, set_precision, synchronize, _det, _sync

__all__ = ['LARGE_SEP_VARIABLES', 'LARGE_SEP_MOVING', 'RPN_HEAD_VARIABLES', 'HEAD_VARIABLES', 'LARGE_SEP_EPS', 'LARGE_SEP_MOMENTUM',
           'EXIT_FLOW_UNITS', 'EXIT_FLOW_BNS', 'EXIT_FLOW_VARIABLES', 'EXIT_FLOW_MOVING', 'EXIT_FLOW_EPS', 'EXIT_FLOW_MOMENTUM',
           'MIDDLE_FLOW_BLOCKS', 'MIDDLE_FLOW_UNITS', 'MIDDLE_FLOW_VARIABLES', 'MIDDLE_FLOW_MOVING', 'MIDDLE_FLOW_EPS',
           'MIDDLE_FLOW_MOMENTUM', 'ENTRY_FLOW_BLOCKS', 'ENTRY_FLOW_UNITS', 'ENTRY_FLOW_VARIABLES', 'ENTRY_FLOW_MOVING',
           'ENTRY_FLOW_EPS', 'ENTRY_FLOW_MOMENTUM', 'LARGE_SEP_BIAS_SUM', 'merged_layout', 'merged_shapes', 'merge_large_sep', 'split_large_sep_grads', 'head_backward', 'rpn_backward',
           'large_sep_backward', 'exit_flow_train', 'exit_flow_backward', 'middle_flow_train', 'middle_flow_backward',
           'entry_flow_train', 'entry_flow_backward', 'host_middle_flow_train', 'host_middle_flow_backward',
           'host_entry_flow_train', 'host_entry_flow_backward', 'piecewise_learning_rate', 'decayed', 'eval_net_groups', 'optimizer_variables',
           'MomentumOptimizer', 'StepPending', 'Snapshot', 'checkpoint_names', 'TrainStep', 'StepResult', 'LOGGED_SCALARS', 'STEM_CONVS', 'STEM_VARIABLES', 'STEM_MOVING', 'STEM_EPS', 'STEM_MOMENTUM', 'STEM_STAGE', 'STEM', 'StemState',
           'check_stem', 'stem_train', 'stem_backward', 'host_stem_train', 'host_stem_backward']

LARGE_SEP_VARIABLES = tuple('large_sep_feature/%s/%s/%s' % (br, conv, v) for br in ('Branch_0', 'Branch_1')
                            for conv in ('conv2d', 'conv2d_1') for v in ('kernel', 'bias')) + \
    ('large_sep_feature/batch_normalization/gamma', 'large_sep_feature/batch_normalization/beta')
LARGE_SEP_MOVING = ('large_sep_feature/batch_normalization/moving_mean', 'large_sep_feature/batch_normalization/moving_variance')
LARGE_SEP_EPS, LARGE_SEP_MOMENTUM = 1e-5, 0.997        # net/resnet_v2.py: _BATCH_NORM_EPSILON, _BATCH_NORM_DECAY
# the RPN head (net/xception_body.py:381-400) and the head's dense layers (:536-557): kernel, then bias, per layer, in the order
# the native net's builders read them
RPN_HEAD_VARIABLES = tuple('rpn_head/%s/%s' % (l, v) for l in ('conv2d', 'conv2d_1', 'conv2d_2') for v in ('kernel', 'bias'))
HEAD_VARIABLES = tuple('final_head/%s/%s' % (l, v) for l in ('subnet_fc', 'fc_cls', 'fc_loc') for v in ('kernel', 'bias'))

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

# the stem (net/xception_body.py:243-258): conv 3x3 / stride 2 / 'VALID' 3 -> 32 from the image, conv 3x3 / 'VALID' 32 -> 64,
# each with a batch norm and a ReLU behind it; the second ReLU's output is the entry flow's input, the net's `stem_out`
STEM_CONVS = ('block1_conv1', 'block1_conv2')
STEM_VARIABLES = tuple(c + v for c in STEM_CONVS for v in ('/kernel', '_bn/gamma', '_bn/beta'))
STEM_MOVING = tuple(c + v for c in STEM_CONVS for v in ('_bn/moving_mean', '_bn/moving_variance'))
STEM_EPS, STEM_MOMENTUM = EXIT_FLOW_EPS, EXIT_FLOW_MOMENTUM


def _entry_relu_in(b, i):
    return not (b == 2 and i == 1)


# ---- the merged tensors: how the checkpoint's tensors sit inside the ones the layers and the backwards use ---------------------

_B0, _B1 = 'large_sep_feature/Branch_0/', 'large_sep_feature/Branch_1/'
# the one relation that is no concatenation: the merged (1,15) conv's bias is b_b = b0 + b1, so both addends get d_bb
LARGE_SEP_BIAS_SUM = ('b_b', (_B0 + 'conv2d_1/bias', _B1 + 'conv2d_1/bias'))


def merged_shapes(group, **sizes):
    """{variable: its shape in the checkpoint} of a group merged_layout knows, in the group's variable order, from the same sizes"""
    if group == 'large_sep_feature':
        cin, mid, co = (int(sizes[k]) for k in ('cin', 'mid', 'co'))
        return {br + k: shape for br in (_B0, _B1) for k, shape in (('conv2d/kernel', (15, 1, cin, mid)), ('conv2d/bias', (mid,)),
                                                                  ('conv2d_1/kernel', (1, 15, mid, co)), ('conv2d_1/bias', (co,)))}
    if group == 'rpn_head':
        A, cin, hid = (int(sizes[k]) for k in ('A', 'cin', 'hid'))
        shapes = ((3, 3, cin, hid), (hid,), (1, 1, hid, 2 * A), (2 * A,), (1, 1, hid, 4 * A), (4 * A,))
        return dict(zip(RPN_HEAD_VARIABLES, shapes))
    if group == 'final_head':
        nc, co, fcw = (int(sizes[k]) for k in ('nc', 'co', 'fcw'))
        return dict(zip(HEAD_VARIABLES, ((co, fcw), (fcw,), (fcw, nc), (nc,), (fcw, 4), (4,))))
    raise InvalidArgumentError(-1, "merged_layout: group must be 'large_sep_feature', 'rpn_head' or 'final_head', got %r" % (group,))


def merged_layout(group, **sizes):
    """THE statement of the merges (net/xception_body.py:381-400, 450-475, 536-557): the merged tensors of a group as a list of
    (key, outer, [(variable, width), ...]) -- the vocabulary of host_concat / host_split / concat_device / split_device:
    merged[o, off_p : off_p + width_p] = variable_p read as [outer, width_p].
      'large_sep_feature' (cin, mid, co): K_a = Branch_0 | Branch_1 side by side along the (15,1) convs' outputs, b_a their
        biases, K_b = the (1,15) kernels stacked along the inputs (per tap); with LARGE_SEP_BIAS_SUM that is all eight tensors
      'rpn_head' (A, cin, hid): K_0, b_0 = the 3x3 conv alone; K_1, b_1 = conv2d_1 | conv2d_2 (2A | 4A)
      'final_head' (nc, co, fcw): K_0, b_0 = subnet_fc alone; K_1, b_1 = fc_cls | fc_loc (nc | 4)
    A slot of one part is that variable itself, reshaped.  Every width follows from merged_shapes and the slot's outer."""
    shapes = merged_shapes(group, **sizes)
    names = list(shapes)
    if group == 'large_sep_feature':
        cin = int(sizes['cin'])
        slots = [('K_a', 15 * cin, (names[0], names[4])), ('b_a', 1, (names[1], names[5])), ('K_b', 15, (names[2], names[6]))]
    else:                                              # a layer alone, then two side by side: kernels at outer = their inputs
        k0, k1 = shapes[names[0]], shapes[names[2]]
        slots = [('K_0', math.prod(k0[:-1]), names[0:1]), ('b_0', 1, names[1:2]),
                 ('K_1', math.prod(k1[:-1]), (names[2], names[4])), ('b_1', 1, (names[3], names[5]))]
    return [(key, outer, [(n, math.prod(shapes[n]) // outer) for n in parts]) for key, outer, parts in slots]


def _merge(layout, tensors):
    """{key: merged [outer, W] array} of a layout from {variable: array}: host_concat per slot"""
    return {key: train_ops.host_concat([tensors[n] for n, _ in parts], outer) for key, outer, parts in layout}


def _unmerge(layout, shapes, merged):
    """_merge's inverse and adjoint: {variable: array in its checkpoint shape} from {key: merged array}, host_split per slot"""
    return {n: a.reshape(shapes[n]) for key, outer, parts in layout
            for (n, _), a in zip(parts, train_ops.host_split(merged[key], outer, [w for _, w in parts]))}


def merge_large_sep(weights, dtype=np.float32):
    """The large-separable block's two branches as one conv pair (net/xception_body.py:450-475; the same fusion as the
    native net's, without the BN fold): both (15,1) convs read the same input -> one kernel [15,1,cin,2*mid] with the
    branches side by side along the outputs and the bias [2*mid]; branch_0b + branch_1b -> one (1,15) kernel [1,15,2*mid,co]
    with the branches stacked along the inputs and the bias b0 + b1.  -> (K_a, b_a, K_b, b_b)"""
    w = {k: np.asarray(weights[k], dtype) for k in LARGE_SEP_VARIABLES[:8]}
    (_, _, cin, mid), co = w[_B0 + 'conv2d/kernel'].shape, w[_B0 + 'conv2d_1/kernel'].shape[3]
    m = _merge(merged_layout('large_sep_feature', cin=cin, mid=mid, co=co), w)
    b0, b1 = LARGE_SEP_BIAS_SUM[1]
    return m['K_a'].reshape(15, 1, cin, -1), m['b_a'].reshape(-1), m['K_b'].reshape(1, 15, -1, co), w[b0] + w[b1]


def split_large_sep_grads(d_ka, d_ba, d_kb, d_bb, mid):
    """merge_large_sep's adjoint: the gradients of the merged tensors -> the eight conv gradients under the checkpoint's names
    and in its shapes.  Both conv2d_1 biases enter the block as b0 + b1, so both get d_bb."""
    sizes = dict(cin=d_ka.shape[2], mid=mid, co=d_kb.shape[3])
    out = _unmerge(merged_layout('large_sep_feature', **sizes), merged_shapes('large_sep_feature', **sizes),
                   {'K_a': d_ka, 'b_a': d_ba, 'K_b': d_kb})
    out.update({n: np.array(d_bb) for n in LARGE_SEP_BIAS_SUM[1]})
    return out


# ---- what the stages share ------------------------------------------------------------------------------------------------

@contextlib.contextmanager
def _f16x3():
    """layers built inside are split-precision ones whatever the process-wide setting is"""
    before = get_precision()
    set_precision('f16x3')
    try:
        yield
    finally:
        set_precision(before)


def _dense(k):
    """a kernel as the checkpoint stores it -> a dense DeviceTensor (the w / k operand of the backward ops)"""
    b = to_device(k)
    return DeviceTensor(b.ptr, k.shape, k.shape[3], owner=b)


def _first(t, n):
    """the first n images of a tensor sized for max_batch"""
    return DeviceTensor(t.ptr, (n,) + tuple(t.shape[1:]), t.ld, owner=t)


def _check_grad(fn, what, t, like):
    if not isinstance(t, DeviceTensor) or tuple(t.shape) != tuple(like.shape) or t.ld != like.ld:
        raise InvalidArgumentError(-1, '%s: %s must be a DeviceTensor of shape %r with ld %d, got %r'
                                   % (fn, what, tuple(like.shape), like.ld, (getattr(t, 'shape', None), getattr(t, 'ld', None))))


def _download(dev, grads):
    """the weight gradients a backward left in `dev` as (DeviceBuffer, shape) -> NumPy arrays in `grads` (behind the sync)"""
    for k, (buf, shape) in dev.items():
        grads[k] = to_host(buf.ptr, shape)


def _check_weight_grads(fn, weight_grads):
    if weight_grads not in ('host', 'device'):
        raise InvalidArgumentError(-1, "%s: weight_grads must be 'host' or 'device', got %r" % (fn, weight_grads))


def _deliver(dev, grads, weight_grads):
    """the weight gradients of a flow's backward, behind the sync: 'host' -> NumPy arrays (_download); 'device' -> dense
    DeviceTensors in the checkpoint's shapes that own their memory, nothing downloaded (what MomentumOptimizer.step reads)"""
    if weight_grads == 'host':
        return _download(dev, grads)
    for k, (buf, shape) in dev.items():
        buf._keep = None                                 # (the stream has run: the operands need no keeping alive)
        grads[k] = DeviceTensor(buf.ptr, shape, shape[-1], owner=buf)


def _new_grads(shapes):
    """{name: a dense DeviceTensor of this shape that owns its memory}: what a backward's split writes, allocated ahead of its
    launches"""
    out = {}
    for k, shape in shapes.items():
        buf = DeviceBuffer(max(4 * math.prod(shape), 16))
        out[k] = DeviceTensor(buf.ptr, shape, shape[-1], owner=buf)
    return out


def _as_grad(buf, shape):
    """a gradient a backward op left in a DeviceBuffer of its own -> a dense DeviceTensor of the checkpoint's shape"""
    buf._keep = None                                     # (called behind the sync: the operands need no keeping alive)
    return DeviceTensor(buf.ptr, shape, shape[-1], owner=buf)


# A step of MomentumOptimizer(reach='all') moves the RPN head's and the head's weights, so what get_rpn / get_head and the
# losses left -- `rpn_hidden`, `fc`, `cls_reg`, the loss results and their gradients -- belongs to the old weights.  The
# detector counts such steps (_heads_step), each of the two forwards records the count it ran at (_rpn_step, _head_step) and a
# loss result carries its forward's (forward_step): rpn_backward / head_backward refuse a result whose count is not the
# detector's, until the forward and the loss have run again.  A detector no such optimizer stepped has none of the attributes
# and every count reads 0.
_HEAD_FORWARDS = {'_rpn_step': 'get_rpn and losses.rpn_loss(..., keep_device=True)',
                  '_head_step': 'get_head(..., is_training=True, ...)'}


def heads_ran(d, attr):
    """get_rpn ('_rpn_step') or get_head ('_head_step') has run on the detector's current weights"""
    step = getattr(d, '_heads_step', 0)
    if step or hasattr(d, attr):
        setattr(d, attr, step)


def forward_step(t, attr):
    """what a loss result made from the tensor t (a view of a detector's buffer, or anything else) carries as forward_step"""
    return getattr(getattr(t, '_owner', None), attr, 0)


def _check_step(d, fn, result, attr):
    if getattr(result, 'forward_step', 0) != getattr(d, '_heads_step', 0):
        raise InvalidArgumentError(-1, '%s: call %s first (MomentumOptimizer.step has run since this loss result was made: it and '
                                       'the tensors its forward kept belong to the old weights)' % (fn, _HEAD_FORWARDS[attr]))


def _release(tensors):
    """the stream has run every call: nothing needs keeping alive any longer, and the wrappers' references form a ring through
    the rotating views"""
    for t in tensors:
        t._keep = None


class BatchNorm(object):
    """a batch norm in training mode: gamma, beta, the moving statistics (updated in place by forward) and room for the batch
    statistics, all on the device, under the checkpoint's name"""
    __slots__ = ('name', 'eps', 'momentum', 'co', 'gamma', 'beta', 'moving_mean', 'moving_variance', 'save_mean', 'save_invstd')

    def __init__(self, weights, name, eps=EXIT_FLOW_EPS, momentum=EXIT_FLOW_MOMENTUM):
        self.name, self.eps, self.momentum = name, eps, momentum
        for k in ('gamma', 'beta', 'moving_mean', 'moving_variance'):
            setattr(self, k, to_device(np.ascontiguousarray(weights[name + '/' + k], np.float32)))
        self.co = np.asarray(weights[name + '/gamma']).size
        self.save_mean, self.save_invstd = DeviceBuffer(self.co * 4), DeviceBuffer(self.co * 4)

    def forward(self, d, z, relu, y, M, ws):
        """y = (relu)(BN(z)) over z's M rows with their own statistics, which stay in save_mean / save_invstd"""
        check(lib().xdet_batch_norm_forward(z.ptr, z.ld, M, z.shape[3], self.gamma.ptr, self.beta.ptr, self.eps, 1, self.momentum,
                                            self.moving_mean.ptr, self.moving_variance.ptr, 1 if relu else 0, y.ptr, y.ld,
                                            self.save_mean.ptr, self.save_invstd.ptr, ws.ptr, d.stream.handle))

    def backward(self, d, z, y, dy, dx=None, workspace=None):
        """-> (dz, dgamma, dbeta) on the device; y: the output to mask by where a ReLU follows, else None"""
        return train_ops.batch_norm_backward_device(z, y, dy, self.gamma, self.save_mean, self.save_invstd, True, stream=d.stream,
                                              dx=dx, workspace=workspace)

    def views(self, out, prefix=None):
        """out gains the batch and the moving statistics as [1,1,1,C] tensors under '<name>/...'"""
        prefix = self.name + '/' if prefix is None else prefix
        for k in ('save_mean', 'save_invstd', 'moving_mean', 'moving_variance'):
            b = getattr(self, k)
            out[prefix + k] = DeviceTensor(b.ptr, (1, 1, 1, self.co), self.co, owner=b)


class SepUnit(object):
    """one `(relu ->) separable 3x3 -> BN (-> relu)` unit in training mode, what all three flows are made of: the depthwise
    layer, the pointwise conv `pw`, both kernels as dense device tensors for the backward, the batch norm and the tensors a
    training forward keeps: t (the depthwise output), z (the BN input) and, with own_y, y (the BN output)"""
    __slots__ = ('name', 'dil', 'relu_in', 'relu_out', 'dw', 'pw', 'K_dw', 'K_pw', 'bn', 't', 'z', 'y')

    def __init__(self, weights, name, dil, relu_in, relu_out, pw, B, H, W, own_y):
        kd = np.ascontiguousarray(weights[name + '/depthwise_kernel'], np.float32)
        kp = np.ascontiguousarray(weights[name + '/pointwise_kernel'], np.float32)
        C, J = kp.shape[2], kp.shape[3]
        self.name, self.dil, self.relu_in, self.relu_out = name, dil, relu_in, relu_out
        self.dw, self.pw, self.K_dw, self.K_pw = ops.DepthwiseConv2D(kd, dil), pw, _dense(kd), _dense(kp)
        self.bn = BatchNorm(weights, name + '_bn')
        self.t, self.z = DeviceTensor.empty((B, H, W, C)), DeviceTensor.empty((B, H, W, J))
        self.y = DeviceTensor.empty((B, H, W, J)) if own_y else None

    def forward(self, d, x, y, n, H, W, ws_bn):
        """y = (relu)(BN(pw(dw((relu)(x))))) with batch statistics, t and z kept in the unit: three calls on the detector's stream"""
        t, z, h = self.t, self.z, d.stream.handle
        check(lib().xdet_depthwise_forward(self.dw.handle, x.ptr, n, H, W, x.ld, t.ptr, 1 if self.relu_in else 0, h))
        check(lib().xdet_conv_forward(self.pw.handle, t.ptr, n, H, W, t.ld, z.ptr, z.ld, None, 0, h))
        self.bn.forward(d, z, self.relu_out, y, n * H * W, ws_bn)

    def backward(self, d, x, y, dy, dev, ws_dw, into=None):
        """d loss / d y -> d loss / d x through the unit's BN (masked by y, the unit's own output, where it ends in a ReLU; None
        otherwise), the 1x1 conv (its bias gradient computed and dropped: the conv has none) and the depthwise conv: three calls
        on the detector's stream, on the kept z and t of x's images.  dev: gains the four weight gradients as (DeviceBuffer,
        shape) under the checkpoint's names.  into: {'dz', 'dt', 'dx': DeviceTensors to write, 'ws_bn', 'ws_conv': workspaces}
        -- without it every call allocates its own.  -> (dx, dt, dz)"""
        into = into or {}
        n, name = x.shape[0], self.name
        dz, dgamma, dbeta = self.bn.backward(d, _first(self.z, n), y, dy, into.get('dz'), into.get('ws_bn'))
        dt, dkp, _ = train_ops.conv_backward_device(_first(self.t, n), self.K_pw, dz, None, stream=d.stream, dx=into.get('dt'),
                                              workspace=into.get('ws_conv'))
        dx, dkd = train_ops.depthwise_backward_device(x, self.K_dw, dt, self.dil, self.relu_in, stream=d.stream, workspace=ws_dw,
                                                dx=into.get('dx'))
        J = self.K_pw.shape[3]
        dev[name + '/depthwise_kernel'], dev[name + '/pointwise_kernel'] = (dkd, self.K_dw.shape), (dkp, self.K_pw.shape)
        dev[name + '_bn/gamma'], dev[name + '_bn/beta'] = (dgamma, (J,)), (dbeta, (J,))
        return dx, dt, dz

    def views(self, out, n):
        """out gains '<unit>/dw', '<unit>/z' of the first n images and the batch norm's statistics"""
        out[self.name + '/dw'], out[self.name + '/z'] = _first(self.t, n), _first(self.z, n)
        self.bn.views(out)


def _pointwise_layers(weights, names):
    """{name: the 1x1 conv of <name>/pointwise_kernel in split precision, f32 out, no scale or shift}"""
    with _f16x3():
        return {n: ops.Conv2D(np.ascontiguousarray(weights[n + '/pointwise_kernel'], np.float32)) for n in names}


class Projection(object):
    """the residual branch of an exit- or entry-flow block, r = BN(conv1x1(x)): the conv layer `<name>/kernel` (split precision,
    f32 out, no scale or shift), the kernel as a dense device tensor for the backward, the batch norm and the kept z (the BN
    input) and r, [B,H,W,cout]"""
    __slots__ = ('name', 'conv', 'K', 'bn', 'z', 'r')

    def __init__(self, weights, name, bn_name, B, H, W):
        k = np.ascontiguousarray(weights[name + '/kernel'], np.float32)
        with _f16x3():
            self.conv = ops.Conv2D(k)
        self.name, self.K, self.bn = name, _dense(k), BatchNorm(weights, bn_name)
        self.z, self.r = DeviceTensor.empty((B, H, W, k.shape[3])), DeviceTensor.empty((B, H, W, k.shape[3]))

    def forward(self, d, x, n, H, W, ws_bn):
        z = self.z
        check(lib().xdet_conv_forward(self.conv.handle, x.ptr, n, H, W, x.ld, z.ptr, z.ld, None, 0, d.stream.handle))
        self.bn.forward(d, z, False, self.r, n * H * W, ws_bn)

    def backward(self, d, x, g, dev, into=None):
        """g = d loss / d r -> d loss / d x through the batch norm and the conv (its bias gradient dropped), on the kept z of x's
        images; dev gains '<conv>/kernel', '<bn>/gamma' and '<bn>/beta'.  into: {'dz', 'dx': DeviceTensors to write, 'ws_bn',
        'ws_conv': workspaces} -- without it every call allocates its own.  -> (dx, dzr)"""
        into = into or {}
        dzr, dgamma, dbeta = self.bn.backward(d, _first(self.z, x.shape[0]), None, g, into.get('dz'), into.get('ws_bn'))
        dx, dk, _ = train_ops.conv_backward_device(x, self.K, dzr, None, stream=d.stream, dx=into.get('dx'), workspace=into.get('ws_conv'))
        co = self.K.shape[3]
        dev[self.name + '/kernel'] = (dk, self.K.shape)
        dev[self.bn.name + '/gamma'], dev[self.bn.name + '/beta'] = (dgamma, (co,)), (dbeta, (co,))
        return dx, dzr

    def views(self, out, n, r):
        """out gains '<conv>/z' and r (under that key) of the first n images and the batch norm's statistics"""
        out[self.name + '/z'], out[r] = _first(self.z, n), _first(self.r, n)
        self.bn.views(out)


def _max_over_batches(B, nbytes):
    """a workspace for every batch size up to B"""
    return DeviceBuffer(max(nbytes(n) for n in range(1, B + 1)))


# ---- one state object per stage: built from (detector, weights), sized for max_batch; n = the images its last training forward
# ---- ran on (0: none, or a stage it consumes or a new eval body has run since: _ran, new_body) -----------------------------

class LargeSepState(object):
    """the large-separable block: the merged kernels as conv layers (split precision, f32 out) and as dense device tensors
    for the backward, the batch norm (eps 1e-5, momentum 0.997), the kept t and z and the BN workspace"""

    def __init__(self, d, weights):
        # (the eight conv tensors as the checkpoint stores them: what MomentumOptimizer(reach='all') makes its masters from)
        self.host = {k: np.ascontiguousarray(weights[k], np.float32) for k in LARGE_SEP_VARIABLES[:8]}
        ka, ba, kb, bb = merge_large_sep({k: np.ascontiguousarray(weights[k], np.float32) for k in LARGE_SEP_VARIABLES})
        with _f16x3():
            self.conv_a, self.conv_b = ops.Conv2D(ka, shift=ba), ops.Conv2D(kb, shift=bb)
        B, (_, H, W, _) = d.max_batch, d.buffer('out', 1).shape
        co, mid2 = kb.shape[3], ka.shape[3]
        self.K_a, self.K_b, self.mid, self.n = _dense(ka), _dense(kb), mid2 // 2, 0
        self.bn = BatchNorm(weights, 'large_sep_feature/batch_normalization', LARGE_SEP_EPS, LARGE_SEP_MOMENTUM)
        self.t, self.z = DeviceTensor.empty((B, H, W, mid2)), DeviceTensor.empty((B, H, W, co))
        self.ws = _max_over_batches(B, lambda n: lib().xdet_batch_norm_workspace_bytes(n * H * W, co))

    def forward(self, d, out, n):
        """large_sep_kernel's training branch: out = the net's `out` of n images -> the net's `feat`"""
        feat, h = d.buffer('feat', n), d.stream.handle
        _, H, W, _ = out.shape
        t, z = self.t, self.z
        check(lib().xdet_conv_forward(self.conv_a.handle, out.ptr, n, H, W, out.ld, t.ptr, t.ld, None, 0, h))
        check(lib().xdet_conv_forward(self.conv_b.handle, t.ptr, n, H, W, t.ld, z.ptr, z.ld, None, 0, h))
        self.bn.forward(d, z, True, feat, n * H * W, self.ws)
        _ran(d, LARGE_SEP, n)
        _sync(d)
        return feat

    def saved(self, d):
        out = {'t': _first(self.t, self.n), 'z': _first(self.z, self.n)}
        self.bn.views(out, '')
        return out


class ExitFlowState(object):
    """the exit flow: its four units (the last batch norm writes the net's `out`), the projection, b2 and one BN and one
    depthwise-backward workspace for the widest tensor"""

    def __init__(self, d, weights):
        B, (_, H, W, _) = d.max_batch, d.buffer('mid_x', 1).shape
        pw = _pointwise_layers(weights, [u[0] for u in EXIT_FLOW_UNITS])
        self.n, self.proj = 0, Projection(weights, 'conv2d_4', 'batch_normalization_4', B, H, W)
        self.units = [SepUnit(weights, name, dil, relu_in, relu_out, pw[name], B, H, W, own_y=name != EXIT_FLOW_UNITS[-1][0])
                      for name, dil, relu_in, relu_out in EXIT_FLOW_UNITS]
        co = self.proj.conv.cout
        widest = max([co] + [c for u in self.units for c in (u.t.shape[3], u.z.shape[3])])
        self.b2 = DeviceTensor.empty((B, H, W, co))
        self.ws_bn = _max_over_batches(B, lambda n: lib().xdet_batch_norm_workspace_bytes(n * H * W, widest))
        self.ws_dw = _max_over_batches(B, lambda n: lib().xdet_depthwise_backward_workspace_bytes(n, H, W, widest))

    def saved(self, d):
        n, out = self.n, {}
        self.proj.views(out, n, 'r')
        out['b2'] = _first(self.b2, n)
        for u, y in zip(self.units, ('a', 'y2', 'c3', None)):
            u.views(out, n)
            if y:
                out[y] = _first(u.y, n)
        return out


MiddleBlock = collections.namedtuple('MiddleBlock', 'b units out')        # out: None for the last block (the net's `mid_x`)


class MiddleFlowState(object):
    """the middle flow: per block three units (the first two keep their y) and the block's output, one BN, one
    depthwise-backward and one conv-backward workspace for all units, and the four gradient tensors middle_flow_backward
    rotates through"""

    def __init__(self, d, weights):
        B, (_, H, W, C) = d.max_batch, d.buffer('entry_x', 1).shape
        pw = _pointwise_layers(weights, MIDDLE_FLOW_UNITS)
        self.n, self.blocks = 0, []
        for b in MIDDLE_FLOW_BLOCKS:
            units = [SepUnit(weights, 'block%d_sepconv%d' % (b, i), 1, True, False, pw['block%d_sepconv%d' % (b, i)], B, H, W,
                             own_y=i < 3) for i in (1, 2, 3)]
            self.blocks.append(MiddleBlock(b, units, DeviceTensor.empty((B, H, W, C)) if b != MIDDLE_FLOW_BLOCKS[-1] else None))
        self.ws_bn = _max_over_batches(B, lambda n: lib().xdet_batch_norm_workspace_bytes(n * H * W, C))
        self.ws_dw = _max_over_batches(B, lambda n: lib().xdet_depthwise_backward_workspace_bytes(n, H, W, C))
        self.ws_conv = _max_over_batches(B, lambda n: lib().xdet_conv_backward_workspace_bytes(n, H, W, C, C, 1, 1))
        self.rot = {k: DeviceTensor.empty((B, H, W, C)) for k in ('dz', 'dt', 'da', 'db')}

    def saved(self, d):
        n = self.n
        out, x = {}, d.buffer('entry_x', n)
        for blk in self.blocks:
            out['x%d' % blk.b] = x
            for u, y in zip(blk.units, ('y1', 'y2', None)):
                u.views(out, n)
                if y:
                    out['block%d/%s' % (blk.b, y)] = _first(u.y, n)
            x = _first(blk.out, n) if blk.out is not None else None
        return out


# out: None for the last block (the net's `entry_x`); rot: the gradient tensors entry_flow_backward writes inside the block
EntryBlock = collections.namedtuple('EntryBlock', 'b units H W cin c xs proj out rot')


class EntryFlowState(object):
    """blocks 2-4: per block both units (each keeps its y), the projection, the subsampled input xs, the block's output and the
    gradient tensors of the backward; one BN, one depthwise-backward and one conv-backward workspace for all"""

    def __init__(self, d, weights):
        B, (_, H, W, cin) = d.max_batch, d.buffer('stem_out', 1).shape
        pw = _pointwise_layers(weights, ENTRY_FLOW_UNITS)
        self.n, self.blocks = 0, []
        l, need = lib(), {'bn': [], 'dw': [], 'conv': []}
        for b in ENTRY_FLOW_BLOCKS:
            Ho, Wo = -(-H // 2), -(-W // 2)
            proj = Projection(weights, 'conv2d_%d' % (b - 1), 'batch_normalization_%d' % (b - 1), B, Ho, Wo)
            c = proj.conv.cout
            units = [SepUnit(weights, 'block%d_sepconv%d' % (b, i), 1, _entry_relu_in(b, i), False, pw['block%d_sepconv%d' % (b, i)],
                             B, H, W, own_y=True) for i in (1, 2)]
            full, half = (lambda ch: DeviceTensor.empty((B, H, W, ch))), (lambda ch: DeviceTensor.empty((B, Ho, Wo, ch)))
            # a unit's dz is dead once its conv backward has run: one tensor serves both units
            rot = {'dzr': half(c), 'dxs': half(cin), 'dy2': full(c), 'dz': full(c), 'dt2': full(c), 'd2': full(c), 'dt1': full(cin),
                   'd1': full(cin)}
            self.blocks.append(EntryBlock(b, units, H, W, cin, c, half(cin), proj, half(c) if b != ENTRY_FLOW_BLOCKS[-1] else None, rot))
            for n in range(1, B + 1):
                need['bn'] += [l.xdet_batch_norm_workspace_bytes(n * H * W, c), l.xdet_batch_norm_workspace_bytes(n * Ho * Wo, c)]
                need['dw'] += [l.xdet_depthwise_backward_workspace_bytes(n, H, W, c), l.xdet_depthwise_backward_workspace_bytes(n, H, W, cin)]
                need['conv'] += [l.xdet_conv_backward_workspace_bytes(n, Ho, Wo, cin, c, 1, 1),
                                 l.xdet_conv_backward_workspace_bytes(n, H, W, cin, c, 1, 1),
                                 l.xdet_conv_backward_workspace_bytes(n, H, W, c, c, 1, 1)]
            H, W, cin = Ho, Wo, c
        ex = d.buffer('entry_x', 1)
        if tuple(ex.shape[1:]) != (H, W, cin):
            raise InvalidArgumentError(-1, 'entry_flow_train: block 4 gives %r but the net\'s entry_x is %r' % ((H, W, cin), tuple(ex.shape[1:])))
        self.ws_bn, self.ws_dw, self.ws_conv = DeviceBuffer(max(need['bn'])), DeviceBuffer(max(need['dw'])), DeviceBuffer(max(need['conv']))

    def saved(self, d):
        n = self.n
        out, x = {}, d.buffer('stem_out', n)
        for blk in self.blocks:
            out['x%d' % blk.b] = x
            out['block%d/xs' % blk.b] = _first(blk.xs, n)
            blk.proj.views(out, n, 'block%d/r' % blk.b)
            for u, y in zip(blk.units, ('y1', 'y2')):
                u.views(out, n)
                out['block%d/%s' % (blk.b, y)] = _first(u.y, n)
            x = _first(blk.out, n) if blk.out is not None else d.buffer('entry_x', n)
        out['x%d' % (ENTRY_FLOW_BLOCKS[-1] + 1)] = x
        return out


class StemState(object):
    """the stem: the two kernels as the checkpoint stores them (K1 is what the training-mode conv reads, K2 the backward's
    operand: both the optimizer's masters), both batch norms, block1_conv2 as a conv layer (split precision, f32 out, 3x3
    'VALID'), the image as NHWC rows of 4 floats (block1_conv1's dW reads it), the kept z1, a1 and z2, the three gradient
    tensors of the backward, and one BN and one conv-backward workspace for every batch size up to max_batch"""

    def __init__(self, d, weights):
        k1 = np.ascontiguousarray(weights['block1_conv1/kernel'], np.float32)
        k2 = np.ascontiguousarray(weights['block1_conv2/kernel'], np.float32)
        B, S = d.max_batch, d.image_size
        c1, c2 = k1.shape[3], k2.shape[3]
        H1 = (S - 3) // 2 + 1
        H2 = H1 - 2
        so = d.buffer('stem_out', 1)
        if tuple(k1.shape) != (3, 3, 3, 32) or tuple(k2.shape[:3]) != (3, 3, 32) or tuple(so.shape[1:]) != (H2, H2, c2):
            raise InvalidArgumentError(-1, 'stem_train: block1_conv2 gives %r but the net\'s stem_out is %r (kernels %r and %r)'
                                       % ((H2, H2, c2), tuple(so.shape[1:]), tuple(k1.shape), tuple(k2.shape)))
        self.n, self.S, self.H1, self.H2 = 0, S, H1, H2
        self.K1, self.K2 = _dense(k1), _dense(k2)
        self.bn1 = BatchNorm(weights, 'block1_conv1_bn', STEM_EPS, STEM_MOMENTUM)
        self.bn2 = BatchNorm(weights, 'block1_conv2_bn', STEM_EPS, STEM_MOMENTUM)
        with _f16x3():
            self.conv2 = ops.Conv2D(k2, padding='VALID')
        self.image = DeviceTensor.empty((B, S, S, 3), ld=4)
        self.z1, self.a1, self.z2 = (DeviceTensor.empty(s) for s in ((B, H1, H1, c1), (B, H1, H1, c1), (B, H2, H2, c2)))
        self.dz2, self.da1, self.dz1 = (DeviceTensor.empty(s) for s in ((B, H2, H2, c2), (B, H1, H1, c1), (B, H1, H1, c1)))
        self.db = DeviceBuffer(4 * max(c1, c2))          # the bias gradient xdet_conv_backward_strided insists on: dropped
        l = lib()
        self.ws_bn = _max_over_batches(B, lambda n: max(l.xdet_batch_norm_workspace_bytes(n * H1 * H1, c1),
                                                        l.xdet_batch_norm_workspace_bytes(n * H2 * H2, c2)))
        self.ws_conv = _max_over_batches(B, lambda n: max(l.xdet_conv_backward_strided_workspace_bytes(n, H1, H1, c1, c2, 3, 3, 1, 0),
                                                          l.xdet_conv_backward_strided_workspace_bytes(n, S, S, 3, c1, 3, 3, 2, 0)))

    def saved(self, d):
        n = self.n
        out = {'x1': _first(self.image, n), 'block1_conv1/z': _first(self.z1, n), 'a1': _first(self.a1, n),
               'block1_conv2/z': _first(self.z2, n), 'x2': d.buffer('stem_out', n)}
        self.bn1.views(out)
        self.bn2.views(out)
        return out


# The stages in the order the data flows backward through them, each consuming what the next one writes in training mode:
# (the constructor flag and detector attribute, where the detector keeps the state, its class, the weights it needs, the
# forward its *_saved() names, and why it cannot do without the stage above it in this table)
Stage = collections.namedtuple('Stage', 'flag attr state names forward needs')
STAGES = (
    Stage('large_sep_train', '_lsep', LargeSepState, LARGE_SEP_VARIABLES + LARGE_SEP_MOVING,
          'large_sep_kernel(..., is_training=True)', None),
    Stage('exit_flow_train', '_exit', ExitFlowState, EXIT_FLOW_VARIABLES + EXIT_FLOW_MOVING, 'model.exit_flow_train()',
          'the training-mode `out` it writes is consumed by the large-separable block in training mode'),
    Stage('middle_flow_train', '_middle', MiddleFlowState, MIDDLE_FLOW_VARIABLES + MIDDLE_FLOW_MOVING, 'model.middle_flow_train()',
          'the training-mode `mid_x` it writes is consumed by the exit flow in training mode'),
    Stage('entry_flow_train', '_entry', EntryFlowState, ENTRY_FLOW_VARIABLES + ENTRY_FLOW_MOVING, 'model.entry_flow_train()',
          'the training-mode `entry_x` it writes is consumed by the middle flow in training mode'))
LARGE_SEP, EXIT, MIDDLE, ENTRY = range(4)
# The stem stands next to the table, not in it: it is upstream of every stage of STAGES -- its training forward drops what all
# four had saved, and no training forward of theirs drops what it saved -- and the shared bookkeeping reads its flag as
# getattr(d, 'stem_train', False), so whatever carries exactly the table's four flags behaves as it did.
STEM_STAGE = Stage('stem_train', '_stem', StemState, STEM_VARIABLES + STEM_MOVING, 'model.stem_train()',
                   'the training-mode `stem_out` it writes is consumed by the entry flow in training mode')
STEM = 4


def _stage_of(k):
    return STEM_STAGE if k == STEM else STAGES[k]


def check_stem(stem_on, entry_on, weights):
    """check_stages' two refusals for the stem, ahead of the native net: it needs the entry flow's stage, then its own variables
    and moving statistics"""
    s = STEM_STAGE
    if not stem_on:
        return
    if not entry_on:
        raise InvalidArgumentError(-1, '%s=True needs %s=True (%s)' % (s.flag, STAGES[ENTRY].flag, s.needs))
    miss = [v for v in s.names if v not in weights]
    if miss:
        raise InvalidArgumentError(-1, '%s: the weights lack %s' % (s.flag, ', '.join(miss)))


def check_stages(on, weights):
    """LightHeadDetector.__init__'s refusals, ahead of the native net (which would miss the weights under another error), from
    the last stage of the table up: stage k needs stage k - 1, then its own variables and moving statistics.  on: one flag per
    stage, in the table's order"""
    for k in reversed(range(len(STAGES))):
        s = STAGES[k]
        if not on[k]:
            continue
        if k and not on[k - 1]:
            raise InvalidArgumentError(-1, '%s=True needs %s=True (%s)' % (s.flag, STAGES[k - 1].flag, s.needs))
        miss = [v for v in s.names if v not in weights]
        if miss:
            raise InvalidArgumentError(-1, '%s: the weights lack %s' % (s.flag, ', '.join(miss)))


def build_stages(d, on, weights):
    """the detector gains one flag per stage and, for those that are on, the stage's state"""
    for s, flag in zip(STAGES, on):
        setattr(d, s.flag, bool(flag))
        if flag:
            setattr(d, s.attr, s.state(d, weights))


def saved(d, k):
    """detector.<stage>_saved(): what stage k's last training forward left on the device, as DeviceTensors of its n images
    (k: an index of STAGES, or STEM)"""
    s = _stage_of(k)
    state = getattr(d, s.attr) if getattr(d, s.flag, False) else None
    if state is None or not state.n:
        raise InvalidArgumentError(-1, '%s: no %s has run on this detector' % (s.flag.replace('_train', '_saved'), s.forward))
    return state.saved(d)


def _stage(d, k, fn, first=None, keeps=''):
    """the two refusals an entry point opens with -> (stage k's state, the images to run on).  A backward names the training
    forward it follows (`first`) and runs on that one's images; a training forward follows the eval body and runs on its
    (k: an index of STAGES, or STEM)"""
    s = _stage_of(k)
    if not getattr(d, s.flag, False):
        why = '' if first else ' (the default detector folds the moving statistics into the conv weights%s)' % keeps
        raise InvalidArgumentError(-1, '%s: needs a detector built with %s=True%s' % (fn, s.flag, why))
    state = getattr(d, s.attr)
    n = state.n if first else d._N
    if not n:
        raise InvalidArgumentError(-1, '%s: call %s first' % (fn, first or 'XceptionBody(..., is_training=False)'))
    return state, n


def _ran(d, k, n):
    """stage k's training forward has run on n images: what the stages it feeds had saved belongs to another tensor"""
    for s in STAGES[:k]:
        if getattr(d, s.flag):
            getattr(d, s.attr).n = 0
    getattr(d, STAGES[k].attr).n = n


def _stem_ran(d, n):
    """the stem's training forward has run on n images: it feeds every stage of STAGES, so what all four had saved belongs to
    another `stem_out`"""
    for s in STAGES:
        if getattr(d, s.flag):
            getattr(d, s.attr).n = 0
    getattr(d, STEM_STAGE.attr).n = n


def new_body(d):
    """the eval body is about to run on new images (set_images, a caller-owned image pointer, the uint8 ingest): `stem_out`,
    `entry_x`, `mid_x` and `out` will hold their eval tensors, so what every stage had saved belongs to tensors that are gone.
    Each *_backward and *_saved() refuses until its stage's training forward has run again.  A detector built without
    training flags pays the four attribute reads, and one more for the stem's flag"""
    for s in STAGES:
        if getattr(d, s.flag):
            getattr(d, s.attr).n = 0
    if getattr(d, STEM_STAGE.flag, False):
        getattr(d, STEM_STAGE.attr).n = 0


# ---- the sampled-ROI head (LightHeadDetector(head_rois=P), option "head_rois") -----------------------------------------------

def check_head_rois(head_rois, rpn_post_nms_top_n):
    """the constructor's argument -> None (off) or P; refused by name ahead of the native net: anything but a whole number in
    1..rpn_post_nms_top_n (the C side states the same bound for its option)"""
    if head_rois is None:
        return None
    ok = isinstance(head_rois, (int, np.integer)) and not isinstance(head_rois, bool)
    if not ok or not 1 <= int(head_rois) <= int(rpn_post_nms_top_n):
        raise InvalidArgumentError(-1, 'head_rois must be None (off) or a whole number in 1..rpn_post_nms_top_n (%d), got %r'
                                       % (rpn_post_nms_top_n, head_rois))
    return int(head_rois)


def check_eval_head(eval_head, head_rois):
    """the detector's eval_head argument -> bool; refused ahead of any GPU work: on a detector without head_rois (its one
    head stage runs on all proposals already), anything but a bool"""
    if not isinstance(eval_head, (bool, np.bool_)):
        raise InvalidArgumentError(-1, 'eval_head must be True or False, got %r' % (eval_head,))
    if eval_head and head_rois is None:
        raise InvalidArgumentError(-1, 'eval_head=True needs head_rois=P: a detector without head_rois runs its one head stage on '
                                       'all proposals already and evaluates as it is')
    return bool(eval_head)


def rois_to_head(d, rois, n):
    """get_head on a head_rois detector, handed its ROIs as a DeviceTensor [n,P,(1,)4] of dense corner boxes: one
    device-to-device copy into the net's `head_rois` buffer on the detector's stream; none when it is that buffer.  A tensor
    that ext_encode_rois(..., keep_device=True) made on another stream carries that stream: it is waited for first"""
    view = d.buffer('head_rois', n)
    shp = tuple(rois.shape)
    if rois.ld != 4 or shp[-1] != 4 or shp[0] != n or int(np.prod(shp[1:-1])) != d.head_R:
        raise InvalidArgumentError(-1, 'get_head: device ROIs must be dense corner boxes [N,%d,(1,)4] (ld 4), got %r (ld %d)'
                                       % (d.head_R, shp, rois.ld))
    if rois.ptr == view.ptr:
        return
    made_on = getattr(rois, 'made_on', d.stream)
    if made_on is not d.stream:
        synchronize(made_on)
    check(lib().xdet_memcpy_d2d(view.ptr, rois.ptr, n * d.head_R * 16, d.stream.handle))
    d._head_rois_src = rois                              # (alive until the next hand-over: the copy may still be in flight)


# ---- the head's and the RPN head's backward -----------------------------------------------------------------------------------

def _kernels(weights):
    return [k for k in weights if k.endswith('/kernel')]


def _group_sizes(d, group):
    """merged_layout's sizes of a group, from the detector's own tensors"""
    if group == 'rpn_head':
        _, _, cin, hid = d._rpn_weights['rpn_head/conv2d/kernel'].shape
        return dict(A=d.cfg.num_anchors, cin=cin, hid=hid)
    if group == 'final_head':
        co, fcw = d._head_weights['final_head/subnet_fc/kernel'].shape
        return dict(nc=d.cfg.num_classes, co=co, fcw=fcw)
    s = d._lsep
    return dict(cin=s.K_a.shape[2], mid=s.mid, co=s.K_b.shape[3])


def _operands(d, group):
    """the w operands of the two backwards of a head ('rpn_head', 'final_head'), made once per detector from merged_layout's K
    slots: the first layer's kernel (the RPN's 3x3 conv keeps its shape) and the two layers behind it side by side, as [K,1,1,J]
    dense device tensors (MomentumOptimizer(reach='all') rebuilds them in place after a step)"""
    attr = '_%s_operands' % group
    if not hasattr(d, attr):
        weights = d._rpn_weights if group == 'rpn_head' else d._head_weights
        layout = [slot for slot in merged_layout(group, **_group_sizes(d, group)) if slot[0][0] == 'K']
        out = []
        for (_, outer, parts), k in zip(layout, _merge(layout, weights).values()):
            one = weights[parts[0][0]].shape if len(parts) == 1 else ()
            b = to_device(k)
            out.append(DeviceTensor(b.ptr, one if len(one) == 4 else (outer, 1, 1, k.shape[1]), k.shape[1], owner=b))
        setattr(d, attr, tuple(out))
    return getattr(d, attr)


class _WeightGrads(object):
    """The tail head_backward, rpn_backward and large_sep_backward share: the gradients of a group's merged tensors -> the
    gradients of its variables under the checkpoint's names and in its shapes, by merged_layout.  Made AHEAD of the launches
    (weight_grads='device': the per-variable tensors are allocated here); split(merged) behind them and ahead of the sync, with
    merged = {key: the DeviceBuffer a backward op left} ('device': the one split_device table, 'host': no launch); collect()
    behind the sync -> {variable: dense DeviceTensor | NumPy array}.  A slot of one part is its variable: no copy."""

    def __init__(self, d, group, weight_grads):
        sizes = _group_sizes(d, group)
        self.layout, self.shapes = merged_layout(group, **sizes), merged_shapes(group, **sizes)
        self.sums = (LARGE_SEP_BIAS_SUM,) if group == 'large_sep_feature' else ()
        self.dev = None
        if weight_grads == 'device':
            split = [n for _, _, parts in self.layout if len(parts) > 1 for n, _ in parts] + [n for _, names in self.sums for n in names]
            self.dev = _new_grads({n: self.shapes[n] for n in split})

    def split(self, merged, stream):
        self.merged = merged
        if self.dev is not None:
            self.table = [(merged[key], outer, [(self.dev[n], w) for n, w in parts]) for key, outer, parts in self.layout if len(parts) > 1] + \
                         [(merged[key], 1, [(self.dev[n], math.prod(self.shapes[n]))]) for key, names in self.sums for n in names]
            train_ops.split_device(self.table, stream=stream)

    def collect(self):
        merged, ones = self.merged, [(key, parts[0][0]) for key, _, parts in self.layout if len(parts) == 1]
        if self.dev is not None:
            out = dict(self.dev)
            out.update({n: _as_grad(merged[key], self.shapes[n]) for key, n in ones})
            self.table[0][0]._keep = None                 # (split_device's keep-alive chain: the stream has run)
            return out
        host = {key: to_host(merged[key].ptr, (outer, sum(w for _, w in parts))) for key, outer, parts in self.layout}
        out = _unmerge(self.layout, self.shapes, host)
        for key, names in self.sums:
            d_sum = to_host(merged[key].ptr, self.shapes[names[0]])
            out.update({n: np.array(d_sum) for n in names})
        return out


def head_backward(loss_func, to_feat=False, weight_grads='host'):
    """The backward of the head's dense layers, called after get_head(..., is_training=True, ...) on the same detector:
    d loss / d cls_reg (loss_func.grad_device, what xdet_head_loss wrote) goes through `fc_cls+fc_loc` (x = the net's `fc`
    buffer, the concatenated [2048, nc + 4] kernel) and then, masked by fc's ReLU, through `subnet_fc` (x = `pooled`) -- two
    calls of xdet_dense_backward on the net's buffers with their own ld.  -> a dict with the six gradients under the
    checkpoint's variable names (final_head/{subnet_fc,fc_cls,fc_loc}/{kernel,bias}, NumPy) and 'pooled': d loss / d pooled
    as a DeviceTensor [N,R,1,C] ([N * R, C] rows, ld C) and 'fc': d loss / d fc (in front of fc's ReLU mask) likewise.
    to_feat=True (a detector built with pool_index=True): d loss / d pooled goes on through xdet_net_head_pool_backward -- the
    order-exact PsRoiAlign gradient on the net's `proposals` and the argmax get_head kept -- on the same stream, with no host
    round trip in between, and the dict gains 'feat': d loss / d feat as a DeviceTensor [N,H,W,C] with the `feat` buffer's
    ld (padding channels zero), what the large-separable backward will read.
    weight_grads='device': the six variables come back as dense DeviceTensors in the checkpoint's shapes instead -- fc_cls and
    fc_loc taken apart from the merged dW / db by one split_device table on the detector's stream -- and nothing is downloaded
    (what MomentumOptimizer.step takes at reach='all'); everything else the call returns is unchanged.
    Refused once a step of MomentumOptimizer(reach='all') has run since loss_func's result was made, until get_head has run
    again: `fc`, `pooled` and the gradient belong to the old weights."""
    d = _det()
    _check_weight_grads('head_backward', weight_grads)
    if to_feat and not d.pool_index:
        raise InvalidArgumentError(-1, 'head_backward: to_feat=True needs a detector built with pool_index=True (the head '
                                       'kept no argmax to go back through)')
    g = getattr(loss_func, 'grad_device', None)
    if getattr(loss_func, 'result', None) is None or g is None:
        raise InvalidArgumentError(-1, 'head_backward: the losses ran without a gradient (call get_head(..., is_training=True, '
                                       '...) with this loss_func first)')
    n, nc = g.shape[0], d.cfg.num_classes
    if (g.shape[1], g.shape[3]) != (d.head_R, nc + 4) or n > d.max_batch:
        raise InvalidArgumentError(-1, 'head_backward: gradient of shape %r but the detector has %d ROIs per image, %d classes, '
                                       'max_batch %d' % (g.shape, d.head_R, nc, d.max_batch))
    if len(_kernels(d._head_weights)) != 3:
        raise InvalidArgumentError(-1, 'head_backward: the detector was built without the final_head kernels')
    _check_step(d, 'head_backward', loss_func, '_head_step')
    w0, w1 = _operands(d, 'final_head')
    fc, pooled = d.buffer('fc', n), d.buffer('pooled', n)
    K0, K1 = w0.shape[0], w1.shape[0]
    d_feat = None
    if to_feat:                                    # (allocated ahead of the launches, not between the last two)
        fb = d.buffer('feat', n)
        d_feat = DeviceTensor.empty(fb.shape, ld=fb.ld)
    wg = _WeightGrads(d, 'final_head', weight_grads)
    dx1, dw1, db1 = train_ops.dense_backward_device(fc, w1, g, None, stream=d.stream)
    dx0, dw0, db0 = train_ops.dense_backward_device(pooled, w0, dx1, fc, stream=d.stream)
    if to_feat:
        check(lib().xdet_net_head_pool_backward(d.handle, n, dx0.ptr, dx0.ld, d_feat.ptr, d.stream.handle))
    wg.split({'K_0': dw0, 'b_0': db0, 'K_1': dw1, 'b_1': db1}, d.stream)
    _sync(d)
    out = wg.collect()
    out.update({'pooled': DeviceTensor(dx0.ptr, (n, d.head_R, 1, K0), K0, owner=dx0),
                'fc': DeviceTensor(dx1.ptr, (n, d.head_R, 1, K1), K1, owner=dx1)})
    if to_feat:
        out['feat'] = d_feat
    return out


def rpn_backward(rpn_loss_result, weight_grads='host'):
    """The backward of the RPN head (net/xception_body.py:381-400), called after get_rpn and losses.rpn_loss(...,
    keep_device=True) on a detector built with rpn_hidden=True: d loss / d rpn_out (rpn_loss_result.grad_device, what
    xdet_rpn_loss wrote) goes through the two 1x1 heads as one dense layer (xdet_dense_backward: x = the net's `rpn_hidden`
    buffer as [N*h*w, 512] rows, the concatenated [512, 6A] kernel) and then, masked by the hidden ReLU, through the 3x3 conv
    (xdet_conv_backward: x = `mid_x` with the ReLU in front of the conv, y = `rpn_hidden`) -- both on the detector's stream
    with no host round trip in between.  -> a dict with the six gradients under the checkpoint's variable names
    (rpn_head/{conv2d,conv2d_1,conv2d_2}/{kernel,bias}, NumPy), 'mid': d loss / d mid_x as a DeviceTensor [N,h,w,728] with
    `mid_x`'s ld (zero where mid_x <= 0) and 'rpn_hidden': d loss / d rpn_hidden (in front of the ReLU mask) [N,h,w,512].
    weight_grads='device': the six variables come back as dense DeviceTensors in the checkpoint's shapes instead -- conv2d_1
    and conv2d_2 taken apart from the merged dW / db by one split_device table on the detector's stream -- and nothing is
    downloaded (what MomentumOptimizer.step takes at reach='all'); everything else the call returns is unchanged.
    Refused once a step of MomentumOptimizer(reach='all') has run since the loss result was made, until get_rpn and the loss
    have run again: `rpn_hidden` and the gradient belong to the old weights."""
    d = _det()
    _check_weight_grads('rpn_backward', weight_grads)
    if not d.rpn_hidden:
        raise InvalidArgumentError(-1, 'rpn_backward: needs a detector built with rpn_hidden=True (the RPN conv kept no f32 '
                                       'output to go back through)')
    g = getattr(rpn_loss_result, 'grad_device', None)
    if g is None:
        raise InvalidArgumentError(-1, 'rpn_backward: the loss left no gradient on the device (call losses.rpn_loss(..., '
                                       'keep_device=True) on the tensors get_rpn returned)')
    if len(_kernels(d._rpn_weights)) != 3:
        raise InvalidArgumentError(-1, 'rpn_backward: the detector was built without the rpn_head kernels')
    n, A = g.shape[0], d.cfg.num_anchors
    out_view = d.buffer('rpn_out', min(max(n, 1), d.max_batch))
    if n > d.max_batch or tuple(g.shape[1:]) != tuple(out_view.shape[1:3]) + (6 * A,) or g.ld != out_view.ld:
        raise InvalidArgumentError(-1, 'rpn_backward: gradient of shape %r (ld %d) but the detector\'s rpn_out is %r (ld %d), '
                                       'max_batch %d' % (g.shape, g.ld, tuple(out_view.shape[1:]), out_view.ld, d.max_batch))
    _check_step(d, 'rpn_backward', rpn_loss_result, '_rpn_step')
    w0, w1 = _operands(d, 'rpn_head')
    hid, mid_x = d.buffer('rpn_hidden', n), d.buffer('mid_x', n)
    wg = _WeightGrads(d, 'rpn_head', weight_grads)
    dx1, dw1, db1 = train_ops.dense_backward_device(hid, w1, g, None, stream=d.stream)
    d_hid = DeviceTensor(dx1.ptr, hid.shape, dx1.ld, owner=dx1)
    dx0, dw0, db0 = train_ops.conv_backward_device(mid_x, w0, d_hid, hid, relu_in=True, stream=d.stream)
    wg.split({'K_0': dw0, 'b_0': db0, 'K_1': dw1, 'b_1': db1}, d.stream)
    _sync(d)
    out = wg.collect()
    out.update({'mid': dx0, 'rpn_hidden': d_hid})
    return out


# ---- the four stages, forward and backward -------------------------------------------------------------------------------------

def large_sep_backward(d_feat, weight_grads='host'):
    """The backward of the large-separable block in training mode, called after large_sep_kernel(..., is_training=True) on a
    detector built with large_sep_train=True: d_feat = head_backward(..., to_feat=True)['feat'] (d loss / d feat, with the
    `feat` buffer's shape and ld) goes through the batch norm and its ReLU (xdet_batch_norm_backward on the kept z, masked
    by the net's own `feat`), then through the merged (1,15) conv (xdet_conv_backward, x = the kept t) and the merged (15,1)
    conv (x = the net's `out`) -- three calls on the detector's stream with no host round trip in between.  -> a dict with the
    ten gradients under the checkpoint's variable names and in its shapes (the merged tensors split back; both conv2d_1
    biases get the merged bias gradient), 'out': d loss / d out as a DeviceTensor [N,h,w,2048] with `out`'s ld, 'z':
    d loss / d z [N,h,w,co] and 't': d loss / d t [N,h,w,2*mid] (what the first conv backward read).  Refused once a new eval
    body (set_images, forward, calibrate, detect_images) or a training forward of one of the flows has run since the block's
    own: the kept t and z belong to another `out`.
    weight_grads='device': the ten variables come back as dense DeviceTensors in the checkpoint's shapes instead -- the eight
    conv gradients taken apart from the merged ones by one split_device table on the detector's stream (split_large_sep_grads'
    statement: both conv2d_1 biases get the merged bias gradient) -- and nothing is downloaded (what MomentumOptimizer.step
    takes at reach='all'); everything else the call returns is unchanged."""
    d = _det()
    _check_weight_grads('large_sep_backward', weight_grads)
    s, n = _stage(d, LARGE_SEP, 'large_sep_backward', 'large_sep_kernel(..., is_training=True)')
    feat, out = d.buffer('feat', n), d.buffer('out', n)
    _check_grad('large_sep_backward', 'd_feat', d_feat, feat)
    co = s.K_b.shape[3]
    wg = _WeightGrads(d, 'large_sep_feature', weight_grads)
    dz, dgamma, dbeta = s.bn.backward(d, _first(s.z, n), feat, d_feat)
    dt, dkb, dbb = train_ops.conv_backward_device(_first(s.t, n), s.K_b, dz, None, stream=d.stream)
    d_out, dka, dba = train_ops.conv_backward_device(out, s.K_a, dt, None, stream=d.stream)
    wg.split({'K_a': dka, 'b_a': dba, 'K_b': dkb, 'b_b': dbb}, d.stream)
    _sync(d)
    grads = wg.collect()
    _deliver({s.bn.name + '/gamma': (dgamma, (co,)), s.bn.name + '/beta': (dbeta, (co,))}, grads, weight_grads)
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
    `mid_x` is not written: get_rpn is unaffected.  The large-separable block's saved state is dropped: large_sep_backward
    refuses until large_sep_kernel(..., is_training=True) has run on the new `out`.  What exit_flow_backward needs stays on
    the device (detector.exit_flow_saved()) until the next eval body: whatever puts new images through the net (set_images, hence
    XceptionBody, forward and calibrate; forward_device on a caller's pointer; detect_images) drops the saved state of all four
    stages.  -> `out` [N,h,w,2048]."""
    d = _det()
    e, n = _stage(d, EXIT, 'exit_flow_train')
    h, l = d.stream.handle, lib()
    mid_x, out = d.buffer('mid_x', n), d.buffer('out', n)
    _, H, W, _ = mid_x.shape
    p = e.proj
    p.forward(d, mid_x, n, H, W, e.ws_bn)
    x = mid_x
    for i, u in enumerate(e.units):
        y = u.y if u.y is not None else out
        u.forward(d, x, y, n, H, W, e.ws_bn)
        if i == 1:                                   # block13's residual add behind its second batch norm
            check(l.xdet_add_rows(y.ptr, y.ld, p.r.ptr, p.r.ld, e.b2.ptr, e.b2.ld, n * H * W, y.shape[3], h))
            y = e.b2
        x = y
    _ran(d, EXIT, n)
    _sync(d)
    return out


def exit_flow_backward(d_out, d_mid=None, weight_grads='host'):
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
    input) likewise.  Refused once a new eval body (set_images, forward, calibrate, detect_images) or a training forward of
    the middle or the entry flow has run since exit_flow_train(): the kept tensors belong to another `mid_x`.
    weight_grads='device': the 19 variables come back as dense DeviceTensors in the checkpoint's shapes instead and nothing is
    downloaded (what MomentumOptimizer.step takes); everything else the call returns is unchanged."""
    d = _det()
    _check_weight_grads('exit_flow_backward', weight_grads)
    e, n = _stage(d, EXIT, 'exit_flow_backward', 'exit_flow_train()')
    out, mid_x = d.buffer('out', n), d.buffer('mid_x', n)
    _check_grad('exit_flow_backward', 'd_out', d_out, out)
    if d_mid is not None:
        _check_grad('exit_flow_backward', 'd_mid', d_mid, mid_x)
    grads, dev = {}, {}

    def unit_backward(u, x, y, dy):
        """-> d loss / d x through BN (masked by y), the 1x1 conv and the depthwise conv"""
        dx, grads['dw/' + u.name], grads['z/' + u.name] = u.backward(d, x, y, dy, dev, e.ws_dw)
        return dx
    u1, u2, u3, u4 = e.units
    a, b2, c3 = _first(u1.y, n), _first(e.b2, n), _first(u3.y, n)
    d_c3 = unit_backward(u4, c3, out, d_out)
    d_b2 = unit_backward(u3, b2, c3, d_c3)
    share_a, dzr = e.proj.backward(d, mid_x, d_b2, dev)
    d_a = unit_backward(u2, a, None, d_b2)
    share_b = unit_backward(u1, mid_x, None, d_a)
    mid = train_ops.add_rows_device(share_b, share_a, stream=d.stream)
    if d_mid is not None:
        train_ops.add_rows_device(mid, d_mid, out=mid, stream=d.stream)
    _sync(d)
    _deliver(dev, grads, weight_grads)
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
    middle_flow_backward needs stays on the device (detector.middle_flow_saved()) until the next eval body, which drops the
    saved state of all four stages (see exit_flow_train).  -> `mid` [N,h,w,728], the tensor get_rpn accepts."""
    d = _det()
    m, n = _stage(d, MIDDLE, 'middle_flow_train', keeps=' and keeps no entry_x')
    h, l = d.stream.handle, lib()
    x, mid_x = d.buffer('entry_x', n), d.buffer('mid_x', n)
    _, H, W, C = x.shape
    for blk in m.blocks:
        u1, u2, u3 = blk.units
        out = blk.out if blk.out is not None else mid_x
        u1.forward(d, x, u1.y, n, H, W, m.ws_bn)
        u2.forward(d, u1.y, u2.y, n, H, W, m.ws_bn)
        u3.forward(d, u2.y, out, n, H, W, m.ws_bn)
        check(l.xdet_add_rows(out.ptr, out.ld, x.ptr, x.ld, out.ptr, out.ld, n * H * W, C, h))
        x = out
    check(l.xdet_net_mid_refresh(d.handle, n, h))
    _ran(d, MIDDLE, n)                               # (what exit_flow_train saved belongs to another mid_x)
    _sync(d)
    return d.buffer('mid', n)


def middle_flow_backward(d_mid, intermediates=False, weight_grads='host'):
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
    addend of the join), each in a tensor of its own.  Refused once a new eval body (set_images, forward, calibrate,
    detect_images) or entry_flow_train() has run since middle_flow_train(): the kept tensors belong to another `entry_x`.
    weight_grads='device': the 96 variables come back as dense DeviceTensors in the checkpoint's shapes instead and nothing is
    downloaded (what MomentumOptimizer.step takes); everything else the call returns is unchanged."""
    d = _det()
    _check_weight_grads('middle_flow_backward', weight_grads)
    m, n = _stage(d, MIDDLE, 'middle_flow_backward', 'middle_flow_train()')
    mid_x, entry = d.buffer('mid_x', n), d.buffer('entry_x', n)
    _check_grad('middle_flow_backward', 'd_mid', d_mid, mid_x)
    rot = {k: _first(t, n) for k, t in m.rot.items()}
    shape = tuple(entry.shape)
    key = lambda blk: 'x%d' % blk.b if blk.b != MIDDLE_FLOW_BLOCKS[0] else 'entry'
    # everything the call returns on the device, allocated ahead of the launches
    grads = {key(blk): DeviceTensor.empty(shape, ld=entry.ld) for blk in m.blocks}
    if intermediates:
        for blk in m.blocks:
            for i, u in enumerate(blk.units):
                grads['d%d/block%d' % (i + 1, blk.b)] = DeviceTensor.empty(shape, ld=entry.ld)
                grads['dw/' + u.name], grads['z/' + u.name] = DeviceTensor.empty(shape), DeviceTensor.empty(shape)
    dev, g = {}, d_mid
    inputs = [entry] + [_first(blk.out, n) for blk in m.blocks[:-1]]
    for blk, x in reversed(list(zip(m.blocks, inputs))):
        u1, u2, u3 = blk.units
        dy = g
        # the three unit gradients alternate between two tensors: a unit's dx is read by the next unit's BN backward only
        for i, u, xin, dst in ((3, u3, _first(u2.y, n), 'da'), (2, u2, _first(u1.y, n), 'db'), (1, u1, x, 'da')):
            into = {'ws_bn': m.ws_bn, 'ws_conv': m.ws_conv, 'dz': rot['dz'], 'dt': rot['dt'], 'dx': rot[dst]}
            if intermediates:
                into.update(dz=grads['z/' + u.name], dt=grads['dw/' + u.name], dx=grads['d%d/block%d' % (i, blk.b)])
            dy, _, _ = u.backward(d, xin, None, dy, dev, m.ws_dw, into)
        g = train_ops.add_rows_device(dy, g, out=grads[key(blk)], stream=d.stream)
    _sync(d)
    _release(list(rot.values()) + list(grads.values()))
    _deliver(dev, grads, weight_grads)
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
    (detector.entry_flow_saved()) until the next eval body, which drops the saved state of all four stages (see
    exit_flow_train).  -> `entry_x` [N,h,w,728]."""
    d = _det()
    e, n = _stage(d, ENTRY, 'entry_flow_train', keeps=' and keeps no stem_out')
    h, l = d.stream.handle, lib()
    x = d.buffer('stem_out', n)
    for blk in e.blocks:
        (u1, u2), p, xs = blk.units, blk.proj, blk.xs
        H, W = blk.H, blk.W
        out = blk.out if blk.out is not None else d.buffer('entry_x', n)
        check(l.xdet_subsample2(x.ptr, x.ld, n, H, W, blk.cin, xs.ptr, xs.ld, h))
        p.forward(d, xs, n, -(-H // 2), -(-W // 2), e.ws_bn)
        u1.forward(d, x, u1.y, n, H, W, e.ws_bn)
        u2.forward(d, u1.y, u2.y, n, H, W, e.ws_bn)
        y2, r = u2.y, p.r
        if not (y2.ld == r.ld == out.ld):
            raise XdetError(-3, 'entry_flow_train: pixel strides %r of y2, r and the block output differ' % ((y2.ld, r.ld, out.ld),))
        check(l.xdet_maxpool3x3s2_add(y2.ptr, r.ptr, out.ptr, n, H, W, blk.c, y2.ld, h))
        x = out
    _ran(d, ENTRY, n)                                # (what the later flows saved belongs to another entry_x)
    _sync(d)
    return d.buffer('entry_x', n)


def entry_flow_backward(d_entry, intermediates=False, weight_grads='host'):
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
    d loss / d (its depthwise output), 'z/<unit>' = d loss / d (its batch norm's input), each in a tensor of its own.  Refused
    once a new eval body (set_images, forward, calibrate, detect_images) has run since entry_flow_train(): the kept tensors
    belong to another `stem_out`.
    weight_grads='device': the 33 variables come back as dense DeviceTensors in the checkpoint's shapes instead and nothing is
    downloaded (what MomentumOptimizer.step takes); everything else the call returns is unchanged."""
    d = _det()
    _check_weight_grads('entry_flow_backward', weight_grads)
    e, n = _stage(d, ENTRY, 'entry_flow_backward', 'entry_flow_train()')
    _check_grad('entry_flow_backward', 'd_entry', d_entry, d.buffer('entry_x', n))
    key = lambda blk: 'stem' if blk.b == ENTRY_FLOW_BLOCKS[0] else 'x%d' % blk.b
    inputs = [d.buffer('stem_out', n)] + [_first(blk.out, n) for blk in e.blocks[:-1]]
    # everything the call returns on the device, allocated ahead of the launches
    grads, inner = {}, {}
    for blk, x in zip(e.blocks, inputs):
        b = blk.b
        grads[key(blk)] = DeviceTensor.empty(tuple(x.shape), ld=x.ld)
        rot = {k: _first(t, n) for k, t in blk.rot.items()}
        rot['dz1'] = rot['dz']
        if intermediates:
            u1, u2 = blk.units
            names = {'dzr': 'z/' + blk.proj.name, 'dxs': 'dxs/block%d' % b, 'dy2': 'dy2/block%d' % b, 'd2': 'd2/block%d' % b,
                     'd1': 'd1/block%d' % b, 'dt2': 'dw/' + u2.name, 'dt1': 'dw/' + u1.name, 'dz': 'z/' + u2.name,
                     'dz1': 'z/' + u1.name}
            for k, name in names.items():
                grads[name] = rot[k] = DeviceTensor.empty(tuple(rot[k].shape), ld=rot[k].ld)
        inner[b] = rot
    dev, g = {}, d_entry
    for blk, x in reversed(list(zip(e.blocks, inputs))):
        (u1, u2), rot = blk.units, inner[blk.b]
        ws = {'ws_bn': e.ws_bn, 'ws_conv': e.ws_conv}
        dxs, _ = blk.proj.backward(d, _first(blk.xs, n), g, dev, dict(ws, dz=rot['dzr'], dx=rot['dxs']))
        dy2 = train_ops.max_pool_backward_device(_first(u2.y, n), g, dx=rot['dy2'], stream=d.stream)
        d2, _, _ = u2.backward(d, _first(u1.y, n), None, dy2, dev, e.ws_dw, dict(ws, dz=rot['dz'], dt=rot['dt2'], dx=rot['d2']))
        d1, _, _ = u1.backward(d, x, None, d2, dev, e.ws_dw, dict(ws, dz=rot['dz1'], dt=rot['dt1'], dx=rot['d1']))
        g = train_ops.add_upsample2_device(d1, dxs, out=grads[key(blk)], stream=d.stream)
    _sync(d)
    _release([t for rot in inner.values() for t in rot.values()] + list(grads.values()))
    _deliver(dev, grads, weight_grads)
    return grads


def stem_train(images=None):
    """The stem in training mode (net/xception_body.py:243-258), called after XceptionBody(..., is_training=False) on a detector
    built with stem_train=True: both stem convs are computed again from the images with batch statistics --

        x1 = nhwc4(images)           (xdet_nchw_to_nhwc4: what block1_conv1's dW reads in the backward)
        z1 = conv3x3s2_valid(images, K1)     (xdet_stem_conv3x3s2_train_forward: f32, straight from NCHW and from the master K1)
        a1 = relu(BN(z1))            z2 = conv3x3_valid(a1, K2)   (xdet_conv_forward, split precision, f32 out)
        stem_out = relu(BN(z2))

    -- the batch norms by xdet_batch_norm_forward in training mode (eps 1e-4, momentum 0.99, the moving statistics updated on
    their device copies); the second one writes straight into the net's `stem_out` buffer (with its ld), so entry_flow_train()
    and everything behind it go on unchanged.  Five calls on the detector's stream with no host round trip.  images=None: the
    detector's own image buffer, what set_images, XceptionBody and the ingest doors (detect_images, detect_jpegs) filled, and
    the body's image count; images=: a dense f32 DeviceTensor [n,3,S,S] (NCHW, ld S) from a caller that ran the body on its own
    pointer (forward_device(images_ptr=...)).  The saved state of all four stages of STAGES is dropped: their backwards refuse
    until their training forwards have run on the new tensors.  What stem_backward needs stays on the device
    (detector.stem_saved()) until the next eval body or optimizer step; no other stage's training forward drops it.
    -> `stem_out` [N,h,w,64]."""
    d = _det()
    if images is None or not getattr(d, STEM_STAGE.flag, False):
        s, n = _stage(d, STEM, 'stem_train', keeps=' and keeps no unfolded stem')
        src = d._images.ptr
    else:                                                # (the caller's own body: the detector counted no images for it)
        s = getattr(d, STEM_STAGE.attr)
        S = s.S
        if not isinstance(images, DeviceTensor) or len(images.shape) != 4 or tuple(images.shape[1:]) != (3, S, S) \
                or images.ld != S or not 1 <= images.shape[0] <= d.max_batch:
            raise InvalidArgumentError(-1, 'stem_train: images must be a dense f32 DeviceTensor [n,3,%d,%d] (NCHW, ld %d) of 1 to %d '
                                           'images, got %r (ld %r)' % (S, S, S, d.max_batch, getattr(images, 'shape', None),
                                                                      getattr(images, 'ld', None)))
        n, src = images.shape[0], images.ptr
    h, l = d.stream.handle, lib()
    S, H1, H2 = s.S, s.H1, s.H2
    out = d.buffer('stem_out', n)
    check(l.xdet_nchw_to_nhwc4(src, s.image.ptr, n, 3, S, S, h))
    check(l.xdet_stem_conv3x3s2_train_forward(src, s.K1.ptr, n, S, s.z1.ptr, s.z1.ld, h))
    s.bn1.forward(d, s.z1, True, s.a1, n * H1 * H1, s.ws_bn)
    check(l.xdet_conv_forward(s.conv2.handle, s.a1.ptr, n, H1, H1, s.a1.ld, s.z2.ptr, s.z2.ld, None, 0, h))
    s.bn2.forward(d, s.z2, True, out, n * H2 * H2, s.ws_bn)
    _stem_ran(d, n)                                  # (what every other stage saved belongs to another stem_out)
    _sync(d)
    return out


def stem_backward(d_stem, intermediates=False, weight_grads='host'):
    """The backward of the stem in training mode, called after stem_train() on a detector built with stem_train=True:
    d_stem = entry_flow_backward(...)['stem'] (d loss / d stem_out, with `stem_out`'s shape and ld).

        dz2 = BN_backward(bn2, d_stem)   (masked by the net's `stem_out`)      da1, dK2 = conv_backward(a1, K2, dz2)
        dz1 = BN_backward(bn1, da1)      (masked by the kept a1)               dK1 = conv_backward(x1, K1, dz1)    (no dx)

    -- xdet_batch_norm_backward and xdet_conv_backward_strided (stride 1 and stride 2, 'VALID'; x1 = the NHWC4 image; the bias
    gradients it insists on are computed and dropped): four calls on the detector's stream with no host round trip and no
    float atomics, on tensors, workspaces and results that all exist before the first launch.  There is no image gradient.
    -> a dict with the six gradients under the checkpoint's variable names and in its shapes (STEM_VARIABLES, NumPy).
    intermediates=True: also 'z/block1_conv2' (dz2), 'a/block1_conv1' (da1) and 'z/block1_conv1' (dz1), each in a tensor of
    its own.  Refused once a new eval body (set_images, forward, calibrate, detect_images) or an optimizer step has run since
    stem_train(): the kept tensors belong to other images or weights.
    weight_grads='device': the six variables come back as dense DeviceTensors in the checkpoint's shapes instead and nothing is
    downloaded (what MomentumOptimizer.step takes); everything else the call returns is unchanged."""
    d = _det()
    _check_weight_grads('stem_backward', weight_grads)
    s, n = _stage(d, STEM, 'stem_backward', 'stem_train()')
    out = d.buffer('stem_out', n)
    _check_grad('stem_backward', 'd_stem', d_stem, out)
    S, H1, H2 = s.S, s.H1, s.H2
    c1, c2 = s.K1.shape[3], s.K2.shape[3]
    # everything the call returns on the device, allocated ahead of the launches
    grads = {}
    if intermediates:
        dz2, da1, dz1 = (DeviceTensor.empty((n,) + tuple(t.shape[1:]), ld=t.ld) for t in (s.dz2, s.da1, s.dz1))
        grads.update({'z/block1_conv2': dz2, 'a/block1_conv1': da1, 'z/block1_conv1': dz1})
    else:
        dz2, da1, dz1 = _first(s.dz2, n), _first(s.da1, n), _first(s.dz1, n)
    shapes = dict(zip(STEM_VARIABLES, (tuple(s.K1.shape), (c1,), (c1,), tuple(s.K2.shape), (c2,), (c2,))))
    dev = {v: (DeviceBuffer(max(4 * math.prod(shape), 16)), shape) for v, shape in shapes.items()}
    (dk1, _), (dg1, _), (db1, _), (dk2, _), (dg2, _), (db2, _) = (dev[v] for v in STEM_VARIABLES)
    x1, z1, a1, z2 = s.image, s.z1, s.a1, s.z2
    h, l = d.stream.handle, lib()
    check(l.xdet_batch_norm_backward(z2.ptr, z2.ld, out.ptr, out.ld, d_stem.ptr, d_stem.ld, n * H2 * H2, c2, s.bn2.gamma.ptr,
                                     s.bn2.save_mean.ptr, s.bn2.save_invstd.ptr, 1, dz2.ptr, dz2.ld, dg2.ptr, db2.ptr, s.ws_bn.ptr, h))
    check(l.xdet_conv_backward_strided(a1.ptr, a1.ld, s.K2.ptr, None, 0, dz2.ptr, dz2.ld, n, H1, H1, c1, c2, 3, 3, 1, 0, 0,
                                       da1.ptr, da1.ld, dk2.ptr, s.db.ptr, s.ws_conv.ptr, h))
    check(l.xdet_batch_norm_backward(z1.ptr, z1.ld, a1.ptr, a1.ld, da1.ptr, da1.ld, n * H1 * H1, c1, s.bn1.gamma.ptr,
                                     s.bn1.save_mean.ptr, s.bn1.save_invstd.ptr, 1, dz1.ptr, dz1.ld, dg1.ptr, db1.ptr, s.ws_bn.ptr, h))
    check(l.xdet_conv_backward_strided(x1.ptr, x1.ld, s.K1.ptr, None, 0, dz1.ptr, dz1.ld, n, S, S, 3, c1, 3, 3, 2, 0, 0,
                                       None, x1.ld, dk1.ptr, s.db.ptr, s.ws_conv.ptr, h))
    _sync(d)
    _deliver(dev, grads, weight_grads)
    return grads


# ---- the optimizer step: the reference's schedule and tf.train.MomentumOptimizer over the three flows' variables ---------------

def piecewise_learning_rate(step, base=1e-3, boundaries=(60000, 80000), factors=(1, 0.8, 0.1), end=1e-4):
    """The reference's learning rate at global step `step` (light_head_rfcn_train.py:426-430): tf.train.piecewise_constant over
    `boundaries` with the values base * factor -- the earlier value holds while step <= boundary -- and end_learning_rate as the
    floor.  -> a Python float"""
    if len(factors) != len(boundaries) + 1:
        raise InvalidArgumentError(-1, 'piecewise_learning_rate: %d boundaries need %d factors, got %d'
                                   % (len(boundaries), len(boundaries) + 1, len(factors)))
    i = 0
    while i < len(boundaries) and step > boundaries[i]:
        i += 1
    return max(float(base) * float(factors[i]), float(end))


def decayed(name):
    """the reference's L2 set (light_head_rfcn_train.py:420): every trainable variable whose name contains neither
    'batch_normalization' nor '_bn'"""
    return 'batch_normalization' not in name and '_bn' not in name


def optimizer_variables(on, reach='flows', stem=False):
    """MomentumOptimizer.variables for a detector whose stages are `on` (one flag per stage, in STAGES' order): the entry, the
    middle and the exit flow's variables of the stages that are on, in that order -- and with reach='all' LARGE_SEP_VARIABLES,
    RPN_HEAD_VARIABLES and HEAD_VARIABLES behind them (170 with all stages on).  stem=True (a detector built with
    stem_train=True): STEM_VARIABLES in front of them all -- 154 and 176, the whole network.  This is also the order of the
    gradient exchange."""
    names = tuple(v for k, vs in ((ENTRY, ENTRY_FLOW_VARIABLES), (MIDDLE, MIDDLE_FLOW_VARIABLES), (EXIT, EXIT_FLOW_VARIABLES))
                  if on[k] for v in vs)
    return (STEM_VARIABLES if stem else ()) + names + (LARGE_SEP_VARIABLES + RPN_HEAD_VARIABLES + HEAD_VARIABLES if reach == 'all' else ())


def eval_net_groups(names):
    """The layer groups xdet_net_refresh_weights takes whole, from the names of a refresh table: a unit is
    <u>/depthwise_kernel, <u>/pointwise_kernel and the four arrays of <u>_bn; a projection conv2d_<i>/kernel and the four arrays
    of batch_normalization_<i>.  -> {group: the sorted names given of it}; a name outside the flows' variables and moving
    statistics, and a group given in part, are refused by name."""
    reach = set(ENTRY_FLOW_VARIABLES + MIDDLE_FLOW_VARIABLES + EXIT_FLOW_VARIABLES + ENTRY_FLOW_MOVING + MIDDLE_FLOW_MOVING + EXIT_FLOW_MOVING)
    bn = ('gamma', 'beta', 'moving_mean', 'moving_variance')
    groups = {}
    for n in names:
        if n not in reach:
            raise InvalidArgumentError(-1, 'refresh_weights: %s is outside the reach (the variables and moving statistics of the '
                                           "body's blocks 2-14)" % n)
        head = n.rsplit('/', 1)[0]
        g = head[:-3] if head.endswith('_bn') else head.replace('batch_normalization_', 'conv2d_')
        groups.setdefault(g, []).append(n)
    for g, have in groups.items():
        if g.startswith('conv2d_'):
            want = [g + '/kernel'] + ['batch_normalization_%s/%s' % (g[7:], k) for k in bn]
        else:
            want = [g + '/depthwise_kernel', g + '/pointwise_kernel'] + ['%s_bn/%s' % (g, k) for k in bn]
        miss = sorted(set(want) - set(have))
        if miss or len(have) != len(want):
            raise InvalidArgumentError(-1, 'refresh_weights: the group of %s is given in part: %s' %
                                       (g, (', '.join(miss) + ' is missing') if miss else 'a name is given twice'))
        have.sort()
    return groups


class StepPending(object):
    """What MomentumOptimizer.step(..., sync=False) returns: the step's scalars are still on the device.  read() -> the dict
    step returns with sync=True, after ONE synchronisation of the detector's stream (a second read() returns the same dict
    and touches nothing); it is also what releases the optimizer for its next step.
    A step of data-parallel training with sync=False carries its communicator (`comm`): read() first waits for it with
    comm.wait(), the host wait under the watchdog -- it covers every exchange enqueued so far, so a dead peer is the
    watchdog's error -- and only then synchronises the detector's stream, which by then waits for no peer."""

    def __init__(self, opt, lr, guard, clip=False, comm=None):
        self.opt, self.lr, self.guard, self.clip, self.comm, self.result, self._alive = opt, lr, guard, clip, comm, None, None
        self.l2 = self.stats = self.scale = None           # the device buffers the scalars lie in (set by step)

    def read(self):
        if self.result is not None:
            return self.result
        opt = self.opt
        if self.comm is not None:
            self.comm.wait()
            self.comm = None
        _sync(opt.det)
        if opt.reach == 'all':
            opt._concat[0][0]._keep = None                 # (concat_device's keep-alive chain: the stream has run)
        self.l2._keep = self._alive = None
        out = {'step': None, 'lr': self.lr, 'l2': float(to_host(self.l2.ptr, (1,))[0])}
        if self.guard or self.clip:
            self.stats._keep = None
            rec = to_host(self.stats.ptr, (1,), train_ops.GRAD_STATS_DTYPE)[0]
            with np.errstate(invalid='ignore'):
                out['grad_norm'] = float(np.sqrt(np.float64(rec['grad_sq'])))
        if self.guard:
            skipped = int(rec['nonfinite']) != 0
            if not skipped:
                opt.steps += 1
            out['skipped'] = skipped
            out['first_bad'] = opt.variables[int(rec['first_bad_slot'])] if skipped else None
        if self.clip:
            self.scale._keep = None
            out['clip_scale'] = float(to_host(self.scale.ptr, (1,))[0])
        out['step'] = opt.steps
        opt._pending, self.result = None, out
        return out


def checkpoint_names(variables, batch_norms=(), model_scope='xception_lighthead'):
    """The reference's checkpoint names of a training state, in the order MomentumOptimizer.snapshot() lays it out: every
    variable as '<scope>/<variable>', then every momentum slot as '<scope>/<variable>/Momentum' (tf.train.MomentumOptimizer's
    slot name), then '<scope>/<bn>/moving_mean' and '<scope>/<bn>/moving_variance' of every batch norm name given, and
    'global_step' (outside the scope: tf.train.get_or_create_global_step, light_head_rfcn_train.py:283) last.
    model_scope '' or None: no prefix."""
    pre = model_scope + '/' if model_scope else ''
    return ([pre + v for v in variables] + [pre + v + '/Momentum' for v in variables] +
            ['%s%s/%s' % (pre, bn, k) for bn in batch_norms for k in ('moving_mean', 'moving_variance')] + ['global_step'])


class Snapshot(object):
    """What MomentumOptimizer.snapshot() returns: the training state at the point of the call in stream order -- masters,
    momentum slots, moving statistics and their CRC-32Cs -- on its way into the optimizer's pinned staging.  Nothing has been
    waited for.  write(prefix) / tensors() wait for the snapshot's event (not for the stream: steps enqueued behind the snapshot
    go on); release() hands the staging back without writing.  The optimizer holds one snapshot at a time."""

    def __init__(self, opt, step, layout, total, event):
        self.opt, self.step, self._layout, self._total, self._event, self._done = opt, int(step), layout, total, event, False

    def _arrays(self):
        """-> ({name without scope: a view of the staging}, {the same name: its unmasked CRC-32C as the device computed it})"""
        if self._done:
            raise InvalidArgumentError(-1, 'Snapshot: already written or released (its staging may hold a later snapshot)')
        self._event.synchronize()
        st = self.opt._snap_host
        crcs = st.view(self._total, (len(self._layout),), np.uint32)
        return ({name: st.view(off, shape) for name, off, shape in self._layout},
                {name: int(c) for (name, _, _), c in zip(self._layout, crcs)})

    def _named(self, arrays, base, model_scope):
        pre = model_scope + '/' if model_scope else ''
        out = {pre + k: np.asarray(v, np.float32) for k, v in (base or {}).items() if k not in arrays}
        out.update((pre + k, v) for k, v in arrays.items())
        out['global_step'] = np.asarray(self.step, np.int64)
        return out

    def tensors(self, base=None, model_scope='xception_lighthead'):
        """-> {checkpoint name: host array}, what write() writes (copies: they outlive the snapshot)"""
        arrays, _ = self._arrays()
        return {k: np.array(v) for k, v in self._named(arrays, base, model_scope).items()}

    def write(self, prefix, base=None, model_scope='xception_lighthead'):
        """Wait for the snapshot's event and write a TensorFlow V2 bundle (tf_checkpoint.write_checkpoint) under the reference's
        names (checkpoint_names): '<scope>/<variable>', '<scope>/<variable>/Momentum', the moving statistics and global_step
        (int64, the optimizer's `steps` at the snapshot).  The CRCs of the snapshot's tensors are the ones the device computed
        beside the copy (write_checkpoint(crcs=)): the host does no per-byte work on them.  base: a weights dict that supplies
        the variables outside the optimizer's reach (reach='flows'), checksummed on the host.  Releases the snapshot.
        -> prefix"""
        from .tf_checkpoint import write_checkpoint
        arrays, crcs = self._arrays()
        pre = model_scope + '/' if model_scope else ''
        write_checkpoint(prefix, self._named(arrays, base, model_scope), crcs={pre + k: c for k, c in crcs.items()})
        self.release()
        return prefix

    def release(self):
        """hand the staging back to the optimizer: its next snapshot() or restore() may overwrite it"""
        if not self._done:
            self._event.synchronize()                      # (the copy into the staging must not outlive its owner's claim)
            self._done = True
            if self.opt._snapshot is self:
                self.opt._snapshot = None


class MomentumOptimizer(object):
    """tf.train.MomentumOptimizer(lr, momentum) over the loss the reference minimises, loss + weight_decay * sum l2_loss(v) over
    the variables `decayed` names (light_head_rfcn_train.py:420,435), for the flow stages `det` was built with: the variables
    of ENTRY_FLOW_VARIABLES + MIDDLE_FLOW_VARIABLES + EXIT_FLOW_VARIABLES whose stage is on, in that order (148 with all
    three, 15 + 48 + 9 = 72 of them kernels in the L2 set).  The masters are the buffers the stages already hold -- SepUnit.K_dw,
    SepUnit.K_pw, Projection.K, BatchNorm.gamma, BatchNorm.beta -- updated in place; the optimizer allocates the momentum slots
    (zero) and the step's workspace and holds a second copy of nothing -- what protects the masters from a gradient that is
    not finite is step(..., guard=True), which decides on the device and stores nothing to them when one is.
    Out of its reach (reach='flows', the default): the large-separable block, the head and the RPN head keep their weights (and the stem, on a detector built without stem_train).  The NATIVE EVAL NET
    keeps the weights it last folded -- XceptionBody(..., is_training=False), forward, detect_images and evaluate compute with
    them -- until refresh_eval_net() refolds the body's blocks 2-14 from the masters and the training stages' moving statistics
    on the device (xdet_net_refresh_weights: no host round trip of the weights, no second net, the captured graphs stay).
    reach='all' (a detector built with large_sep_train=True and rpn_hidden=True that was given the rpn_head and final_head
    weights): `variables` is the flows' list as above, then LARGE_SEP_VARIABLES, RPN_HEAD_VARIABLES and HEAD_VARIABLES -- 170
    with all stages on, the 10 conv / dense kernels and their 10 biases of the three new groups in the L2 set (`decayed`; the
    block's gamma and beta are not).  The masters of those 20 tensors are new device copies in the checkpoint's shapes, gamma
    and beta the buffers LargeSepState.bn holds.
    A detector built with stem_train=True: STEM_VARIABLES come first -- 154 variables at reach='flows', 176 at reach='all', the
    whole network: nothing stays at the checkpoint's values.  Their masters are StemState's K1 and K2 (two more kernels in the
    L2 set) and the two batch norms' gamma and beta; block1_conv1's training forward reads K1 in place, block1_conv2's layer
    is one more slot of the refresh table, and refresh_eval_net() hands the eval net's stem over too (xdet_net_refresh_stem)."""

    reach = 'flows'
    _stem = None                                           # StemState of a detector built with stem_train=True
    _pending = None                                        # the StepPending of a step(..., sync=False) that has not been read
    _scale = None                                          # the clipped step's scale on the device (allocated by the first one)
    _snapshot = None                                       # the Snapshot that has been neither written nor released
    _snap_dev = _snap_host = _snap_ws = _snap_event = None  # the snapshot buffer, its pinned staging, the table workspace

    def __init__(self, det, momentum=0.9, weight_decay=2e-4, reach='flows'):
        flows = [(ENTRY, ENTRY_FLOW_VARIABLES), (MIDDLE, MIDDLE_FLOW_VARIABLES), (EXIT, EXIT_FLOW_VARIABLES)]
        on = [(k, names) for k, names in flows if getattr(det, STAGES[k].flag, False)]
        if not on:
            raise InvalidArgumentError(-1, 'MomentumOptimizer: needs a detector built with exit_flow_train=True (and optionally '
                                           'middle_flow_train, entry_flow_train): no flow stage is on')
        if reach not in ('flows', 'all'):
            raise InvalidArgumentError(-1, "MomentumOptimizer: reach must be 'flows' or 'all', got %r" % (reach,))
        if reach == 'all':
            hidden = getattr(det, 'rpn_hidden', False)
            lack = [what for what, have in (('large_sep_train=True', getattr(det, 'large_sep_train', False)), ('rpn_hidden=True', hidden),
                                            ('the three rpn_head kernels and biases in its weights',
                                             not hidden or len(getattr(det, '_rpn_weights', ())) == 6),
                                            ('the three final_head kernels and biases in its weights', len(getattr(det, '_head_weights', ())) == 6))
                    if not have]
            if lack:
                raise InvalidArgumentError(-1, "MomentumOptimizer: reach='all' needs a detector built with %s" % ', '.join(lack))
        self.det, self.momentum, self.weight_decay, self.steps, self.reach = det, float(momentum), float(weight_decay), 0, reach
        self._stages = [k for k, _ in on]
        masters = {}
        for u in self._units():
            masters[u.name + '/depthwise_kernel'], masters[u.name + '/pointwise_kernel'] = (u.K_dw, u.K_dw.shape), (u.K_pw, u.K_pw.shape)
        for p in self._projections():
            masters[p.name + '/kernel'] = (p.K, p.K.shape)
        self._stem = getattr(det, STEM_STAGE.attr) if getattr(det, STEM_STAGE.flag, False) else None
        if self._stem is not None:
            masters['block1_conv1/kernel'], masters['block1_conv2/kernel'] = (self._stem.K1, self._stem.K1.shape), (self._stem.K2, self._stem.K2.shape)
        for bn in self._batch_norms() + self._stem_batch_norms():
            masters[bn.name + '/gamma'], masters[bn.name + '/beta'] = (bn.gamma, (bn.co,)), (bn.beta, (bn.co,))
        on_flags = [getattr(det, s.flag, False) for s in STAGES]
        self._flow_variables = optimizer_variables(on_flags)
        self.variables = optimizer_variables(on_flags, reach, stem=self._stem is not None)
        if reach == 'all':
            self._reach_all(masters)
        self._master = {v: masters[v] for v in self.variables}            # name -> (device array, shape)
        self._decayed = {v: decayed(v) for v in self.variables}
        self._slot = {v: DeviceBuffer(4 * int(np.prod(self._master[v][1])), zero=True) for v in self.variables}
        table = (MomentumSlot * len(self.variables))()
        for i, v in enumerate(self.variables):                            # (sizes only: the workspace depends on nothing else)
            table[i] = MomentumSlot(1, 1, 1, int(np.prod(self._master[v][1])), 0)
        self._ws = DeviceBuffer(lib().xdet_momentum_step_workspace_bytes(table, len(self.variables)))
        # the guard's workspace, its 16-byte record and the step's l2: allocated once, so a step allocates nothing
        self._stats_ws = DeviceBuffer(lib().xdet_grad_stats_workspace_bytes(table, len(self.variables)))
        self._stats, self._l2, self._pending = DeviceBuffer(16), DeviceBuffer(16), None
        self._refresh_ws = None                            # (an optimizer over no layers has none, and step refreshes nothing)
        if self._refresh_slots():
            rtable, _ = train_ops.refresh_layers_table(self._refresh_slots())
            self._refresh_ws = DeviceBuffer(lib().xdet_layers_refresh_workspace_bytes(rtable, len(rtable)))

    def _reach_all(self, masters):
        """reach='all': masters gains the 22 variables of the large-separable block, the RPN head and the head -- new device
        copies of the 20 conv / dense tensors in the checkpoint's shapes, and the block's own gamma / beta -- and the optimizer the
        concat table that rebuilds, from them, every merged tensor a forward layer or a backward reads: K_a, K_b and b_a of
        LargeSepState, the two operands of rpn_backward and the two of head_backward (a one-part slot is a copy), with its
        workspace; b_a and b_b = b0 + b1 live in two buffers the state gains here"""
        d = self.det
        s = d._lsep
        host = dict(s.host)
        host.update(d._rpn_weights)
        host.update(d._head_weights)
        m = {}
        for v in LARGE_SEP_VARIABLES[:8] + RPN_HEAD_VARIABLES + HEAD_VARIABLES:
            a = np.ascontiguousarray(host[v], np.float32)
            b = to_device(a)
            m[v] = DeviceTensor(b.ptr, a.shape, a.shape[-1], owner=b)
            masters[v] = (m[v], a.shape)
        masters[s.bn.name + '/gamma'], masters[s.bn.name + '/beta'] = (s.bn.gamma, (s.bn.co,)), (s.bn.beta, (s.bn.co,))
        mid2, co = s.K_a.shape[3], s.K_b.shape[3]
        s.b_a, s.b_b = DeviceBuffer(4 * mid2), DeviceBuffer(4 * co)
        (r0, r1), (h0, h1) = _operands(d, 'rpn_head'), _operands(d, 'final_head')
        self._bias_sum = tuple(m[v] for v in LARGE_SEP_BIAS_SUM[1]) + (s.b_b, co)
        # merged_layout's slots that have a merged tensor here (the heads' biases are merged by the net itself, refresh_heads)
        merged = {'large_sep_feature': {'K_a': s.K_a, 'b_a': s.b_a, 'K_b': s.K_b}, 'rpn_head': {'K_0': r0, 'K_1': r1},
                  'final_head': {'K_0': h0, 'K_1': h1}}
        self._concat = [(to[key], outer, [(m[v], w) for v, w in parts]) for group, to in merged.items()
                        for key, outer, parts in merged_layout(group, **_group_sizes(d, group)) if key in to]
        table, _ = train_ops._pack_table(self._concat, 'tensors_concat')
        self._concat_ws = DeviceBuffer(lib().xdet_tensors_concat_workspace_bytes(table, len(table)))
        self._head_names = RPN_HEAD_VARIABLES + HEAD_VARIABLES

    def _states(self):
        return [getattr(self.det, STAGES[k].attr) for k in self._stages]

    def _units(self):
        """the SepUnits of the stages that are on, as the stages hold them at this moment"""
        return [u for s in self._states() for u in (s.units if hasattr(s, 'units') else [u for blk in s.blocks for u in blk.units])]

    def _projections(self):
        return [p for s in self._states() for p in ([s.proj] if hasattr(s, 'proj') else [blk.proj for blk in s.blocks if hasattr(blk, 'proj')])]

    def _batch_norms(self):
        return [u.bn for u in self._units()] + [p.bn for p in self._projections()]

    def _stem_batch_norms(self):
        return [self._stem.bn1, self._stem.bn2] if self._stem is not None else []

    def _moving_batch_norms(self):
        """every batch norm whose moving statistics a training forward of this detector moves: the stem's, the flows' and the
        large-separable block's (its training forward moves its statistics too)"""
        lsep = STAGES[LARGE_SEP]
        return self._stem_batch_norms() + self._batch_norms() + ([getattr(self.det, lsep.attr).bn] if getattr(self.det, lsep.flag, False) else [])

    def step(self, grads, lr, comm=None, guard=False, sync=True, clip_norm=None):
        """One update of every variable from `grads`, {name: dense DeviceTensor in the checkpoint's shape} -- the dicts the flows'
        backwards return with weight_grads='device', merged; other keys are ignored -- at learning rate `lr`, on the detector's
        stream: one xdet_momentum_step over all variables; the refresh of the forward layers (every unit's pointwise and
        depthwise layer and every projection's conv, as the units hold them at this moment) from the updated masters by one
        xdet_layers_refresh_device table; and the drop of every stage's saved state, as a new eval
        body drops it: the kept tensors belong to the old weights, so each *_backward refuses until its training forward has run
        again (the eval body need not: `stem_out` does not depend on these variables -- unless the stem is stepped too, and
        then stem_train() writes the new one).
        -> {'step': the number of steps taken, 'lr': lr, 'l2': sum over the L2 set of sum v^2 / 2 before the update, a float}.
        Refused ahead of any launch: a missing gradient (by name), a host array, a wrong shape.
        comm (an xdet.dist.Communicator; data-parallel training, every rank calls step with its own batch's gradients): after
        those refusals and ahead of xdet_momentum_step, the gradients of `self.variables` are replaced in place, in that order
        and on the detector's stream, by their mean over the ranks (Communicator.average_gradients: the rank-ordered f32 sum
        divided by the world size, the same bits on every rank, equal to xdet.ops.host_average_gradients), and the host waits
        for the exchange with comm.wait() before the step's launches -- a dead peer is then the watchdog's error, not a hang
        in the step's own synchronisation.  The ranks' variables and momentum slots stay bit-equal as long as they started
        bit-equal.  What is NOT averaged: each rank's batch-norm moving statistics stay its own (export_weights of any rank
        gives the same variables, but that rank's statistics), and so do the loss scalars -- TrainStep(comm=) averages both
        behind this call.  The result dict is the same, and
        `l2` is unchanged.  comm=None: a single process, no communicator is touched.
        reach='all': `grads` also carries what head_backward, rpn_backward and large_sep_backward return with
        weight_grads='device'.  Behind the one xdet_momentum_step, in this order: one concat_device table rebuilds from the masters
        the merged K_a, K_b and b_a of LargeSepState and the operands rpn_backward and head_backward read, in place (and one
        xdet_add_rows of one row b_b = b0 + b1), so the next backward differentiates the weights the forward used; conv_a and
        conv_b join the xdet_layers_refresh_device table with their biases; and xdet_net_refresh_heads refreshes the net's own RPN
        and head layers, which the eval net and the training forward share.  What get_rpn, get_head and the losses left is stale:
        rpn_backward and head_backward refuse a loss result from before the step until the forward has run again.  The number
        of launches does not depend on the number of variables.
        guard=True: behind the rank average and ahead of the step, xdet_grad_stats runs over the gradients of `self.variables`
        (after the average every rank decides on the same bits) and the step is xdet_momentum_step_guarded on the record's
        count of non-finite elements: where one gradient element is NaN or +-inf no master and no momentum byte changes --
        the host decides nothing and waits for nothing.  Everything behind the step runs either way: the refresh rebuilds the
        same operands from the unchanged masters, and the saved state is dropped all the same (the batch that made it is
        spent).  The result gains 'grad_norm' (the square root of the record's grad_sq, NaN or inf on a skipped step),
        'skipped' and 'first_bad' (the name of the first variable, in `self.variables`' order, whose gradient holds such an
        element, else None); `self.steps`, and the result's 'step', advance only when the step was taken.
        sync=False: nothing is read back and nothing is synchronised; -> a StepPending whose read() synchronises the
        detector's stream once, reads l2 (and the record) and returns the dict above; the keep-alive references the
        synchronisation bounds live until then, and so does `self.steps` under guard=True.  The buffers the scalars lie in are
        the optimizer's own, so the next step is refused until read() has been called.
        With comm and sync=False the host wait for the exchange moves out of the step as well: the StepPending carries the
        communicator and its read() calls comm.wait() (under the watchdog) ahead of the one synchronisation; with sync=True
        the order stays comm.wait(), then the step's launches.
        clip_norm=c (finite, positive; default None: exactly the calls above): xdet_grad_stats runs whether or not guard is
        set, and the step is xdet_momentum_step_clipped on its record -- every gradient times c / max(grad_norm, c), the scale
        computed on the device in f32 (xdet.ops.host_clip_scale) from the norm over ALL variables' loss gradients, without
        the L2 term, behind the rank average; guard=True holds the same step on the same record.  The result gains
        'clip_scale' (1.0 where nothing was clipped) and, guarded or not, 'grad_norm'.  Without the guard a gradient that is
        not finite reaches the weights as NaN (include/xdet.h)."""
        if self._pending is not None:
            raise InvalidArgumentError(-1, 'MomentumOptimizer.step: the result of the last step(..., sync=False) has not been read: '
                                           'call its read() first (the next step writes the same l2 and guard record)')
        if clip_norm is not None and not (isinstance(clip_norm, (int, float, np.floating, np.integer)) and not isinstance(clip_norm, bool)
                                          and np.isfinite(np.float32(clip_norm)) and np.float32(clip_norm) > 0):
            raise InvalidArgumentError(-1, 'MomentumOptimizer.step: clip_norm must be None or a finite positive number, got %r' % (clip_norm,))
        miss = [v for v in self.variables if v not in grads]
        if miss:
            raise InvalidArgumentError(-1, 'MomentumOptimizer.step: the gradients lack %s' % ', '.join(miss))
        for v in self.variables:
            g, (master, shape) = grads[v], self._master[v]
            if not isinstance(g, DeviceTensor) or tuple(g.shape) != tuple(shape) or g.ld != shape[-1]:
                raise InvalidArgumentError(-1, 'MomentumOptimizer.step: the gradient of %s must be a dense DeviceTensor of shape %r '
                                               '(a backward\'s weight_grads=\'device\'), got %s %r'
                                           % (v, tuple(shape), type(g).__name__, getattr(g, 'shape', None)))
        slots = [(self._master[v][0], grads[v], self._slot[v], math.prod(self._master[v][1]), self._decayed[v]) for v in self.variables]
        d = self.det
        clip = clip_norm is not None
        if comm is not None:
            comm.average_gradients([grads[v] for v in self.variables], d.stream)
            if sync:
                comm.wait()
        stats = train_ops.grad_stats_device(slots, stream=d.stream, workspace=self._stats_ws, out=self._stats) if guard or clip else None
        more = {'skip': stats} if guard else {}            # (the default path makes the call it always made)
        if clip:
            if self._scale is None:
                self._scale = DeviceBuffer(16)
            more.update(clip=(stats, clip_norm), scale_out=self._scale)
        if getattr(self, '_l2', None) is not None:
            more['l2_out'] = self._l2
        l2 = train_ops.momentum_step_device(slots, lr, self.momentum, self.weight_decay, l2=True, stream=d.stream, workspace=self._ws, **more)
        self._refresh_from_masters()
        if not guard:                                      # (a guarded step counts once its record has been read)
            self.steps += 1
        self._pending = StepPending(self, float(lr), guard, clip, comm if not sync else None)
        self._pending.l2, self._pending.stats, self._pending.scale = l2, stats, self._scale if clip else None
        return self._pending.read() if sync else self._pending

    def _refresh_from_masters(self):
        """Everything step enqueues behind the momentum step, in its order, so the forward layers and the backwards' operands
        hold what the masters hold: (reach='all') one concat_device table and the b0 + b1 row; the refresh_layers_device table;
        (reach='all') xdet_net_refresh_heads; and the drop of every stage's saved state.  restore() ends with the same calls."""
        d = self.det
        if self.reach == 'all':                            # the merged tensors the layers and the backwards read, from the masters
            train_ops.concat_device(self._concat, stream=d.stream, workspace=self._concat_ws)
            b0, b1, bb, co = self._bias_sum
            check(lib().xdet_add_rows(b0.ptr, co, b1.ptr, co, bb.ptr, co, 1, co, d.stream.handle))
        layers = self._refresh_slots()
        if layers:
            train_ops.refresh_layers_device(layers, stream=d.stream, workspace=self._refresh_ws)
        if self.reach == 'all':
            d.refresh_heads({v: self._master[v][0] for v in self._head_names})
            d._heads_step = getattr(d, '_heads_step', 0) + 1
        new_body(d)

    def _refresh_slots(self):
        """the training forward layers and their masters, as the units hold them at this moment: refresh_layers_device's table"""
        slots = [s for u in self._units() for s in ((u.pw, u.K_pw), (u.dw, u.K_dw))] + [(p.conv, p.K) for p in self._projections()]
        if self._stem is not None:                         # (block1_conv1 reads its master in place: nothing to refresh)
            slots.append((self._stem.conv2, self._stem.K2))
        if self.reach == 'all':                            # the large-separable block's two merged convs, with their biases
            s = self.det._lsep
            slots += [(s.conv_a, s.K_a, None, s.b_a), (s.conv_b, s.K_b, None, s.b_b)]
        return slots

    def eval_net_tensors(self):
        """{name: device array} of everything refresh_eval_net hands to the eval net: the masters of `self.variables` and the moving
        statistics of the batch norms of the stages that are on"""
        out = {v: self._master[v][0] for v in self._flow_variables}
        for bn in self._batch_norms():
            out[bn.name + '/moving_mean'], out[bn.name + '/moving_variance'] = bn.moving_mean, bn.moving_variance
        return out

    def eval_net_large_sep_tensors(self):
        """reach='all': {name: device array} of the large_sep_feature group refresh_eval_net hands to xdet_net_refresh_heads -- the
        ten masters and the training stage's moving statistics"""
        bn = self.det._lsep.bn
        out = {v: self._master[v][0] for v in LARGE_SEP_VARIABLES}
        out[bn.name + '/moving_mean'], out[bn.name + '/moving_variance'] = bn.moving_mean, bn.moving_variance
        return out

    def eval_net_stem_tensors(self):
        """a detector built with stem_train=True: {name: device array} of the two groups refresh_eval_net hands to
        xdet_net_refresh_stem -- both kernels' masters and the four arrays of both batch norms"""
        s = self._stem
        if s is None:
            raise InvalidArgumentError(-1, 'eval_net_stem_tensors: needs a detector built with stem_train=True')
        out = {'block1_conv1/kernel': s.K1, 'block1_conv2/kernel': s.K2}
        for bn in self._stem_batch_norms():
            for k in ('gamma', 'beta', 'moving_mean', 'moving_variance'):
                out['%s/%s' % (bn.name, k)] = getattr(bn, k)
        return out

    def refresh_eval_net(self):
        """Refold the native eval net's layers of the stages that are on from the masters and the training stages' moving statistics
        as the device holds them (LightHeadDetector.refresh_weights: xdet_net_refresh_weights) -> the number of layers refreshed
        (72 with all three flows: 38 convs and 34 depthwise).  Afterwards the eval net computes what a detector built from
        export_weights(...) computes, bit for bit.  Under data-parallel training each rank folds its own moving statistics.
        reach='all': the large_sep_feature group -- the ten masters and the training stage's moving statistics -- goes through
        xdet_net_refresh_heads first (LightHeadDetector.refresh_heads: merged, folded with eps 1e-5 and the bias b0 + b1, the two
        direct-form layers repacked) -> 74.  A net whose block is in the spectral form takes the same merges and fold through its
        two spectral layers (xdet_spectral_conv_set_kernel_device: the DFT-domain block matrices evaluated from the merged
        kernels on the device, no host copy and no array of their size) when the detector was built with spectral_refresh=True
        -> 74 as well; built without it, it refuses that group by name (large_sep='direct' or spectral_refresh=True), ahead of
        any launch of this call.  The RPN head and the head need nothing here: the
        eval net and the training forward share those layers, and step has refreshed them.
        A detector built with stem_train=True: both stem convs go through xdet_net_refresh_stem as well
        (LightHeadDetector.refresh_stem) -> 74 at reach='flows', 76 at reach='all'."""
        if not hasattr(self.det, 'refresh_weights'):
            raise InvalidArgumentError(-1, 'refresh_eval_net: a PipelinedDetector is out of scope: its two nets would each need the call')
        tensors, extra = self.eval_net_tensors(), 0
        if self.reach == 'all':
            self.det.refresh_heads(self.eval_net_large_sep_tensors())
            extra = 2
        if self._stem is not None:
            self.det.refresh_stem(self.eval_net_stem_tensors())
            extra += 2
        self.det.refresh_weights(tensors)
        return len(eval_net_groups(tensors)) + sum(1 for n in tensors if n.endswith('/depthwise_kernel')) + extra

    def read(self):
        """-> {name: ndarray} for every variable and, under '<name>/Momentum', its momentum slot, in the checkpoint's shapes"""
        _sync(self.det)
        out = {}
        for v in self.variables:
            master, shape = self._master[v]
            out[v], out[v + '/Momentum'] = to_host(master.ptr, shape), to_host(self._slot[v].ptr, shape)
        return out

    def export_weights(self, base):
        """a copy of the weights dict `base` with the optimizer's variables and the current moving statistics of the training
        stages' batch norms replaced by what the device holds: fit for a checkpoint, or for a new LightHeadDetector, whose eval net then
        folds the trained weights (refresh_eval_net() does that for this detector's own eval net without the download)"""
        _sync(self.det)
        out = dict(base)
        for v in self.variables:
            master, shape = self._master[v]
            out[v] = to_host(master.ptr, shape)
        for bn in self._moving_batch_norms():
            for k in ('moving_mean', 'moving_variance'):
                out['%s/%s' % (bn.name, k)] = to_host(getattr(bn, k).ptr, (bn.co,))
        return out

    # ---- checkpoints: a device snapshot with CRC-32C, and the way back in ------------------------------------------------

    def _state_layout(self):
        """the training state as snapshot() lays it out: [(name, live device pointer, shape, offset in the snapshot buffer)] of
        every master, every momentum slot (name + '/Momentum') and the moving statistics of every batch norm a training
        forward moves, each on a 16-byte boundary; -> (the list, the buffer's bytes in front of the CRC words)"""
        items = [(v, self._master[v][0].ptr, tuple(self._master[v][1])) for v in self.variables]
        items += [(v + '/Momentum', self._slot[v].ptr, tuple(self._master[v][1])) for v in self.variables]
        for bn in self._moving_batch_norms():
            items += [('%s/%s' % (bn.name, k), getattr(bn, k).ptr, (bn.co,)) for k in ('moving_mean', 'moving_variance')]
        out, off = [], 0
        for name, ptr, shape in items:
            out.append((name, ptr, shape, off))
            off += (4 * math.prod(shape) + 15) // 16 * 16
        return out, off

    def _snapshot_buffers(self, layout, total):
        """the snapshot buffer [state | one CRC word per tensor | a second row of CRC words], its pinned staging, the table's
        workspace and the event: allocated at the first snapshot() or restore()"""
        if self._snap_dev is None:
            n = len(layout)
            table, _ = train_ops.crc32c_table([(1 << 4, 4 * math.prod(shape)) for _, _, shape, _ in layout])   # (sizes only)
            self._snap_ws = DeviceBuffer(lib().xdet_crc32c_workspace_bytes(table, n))
            self._snap_dev = DeviceBuffer(total + 8 * n)
            self._snap_host = PinnedBuffer(total + 4 * n)
            self._snap_event = Event()

    def snapshot(self):
        """The training state of this moment, put aside without a wait -> a train.Snapshot.  On the detector's stream: ONE
        xdet_crc32c table copies every master of `self.variables`, every momentum slot and the moving_mean / moving_variance of
        every batch norm of _moving_batch_norms() into one device buffer the optimizer owns (allocated at the first snapshot)
        and writes their CRC-32Cs behind them; one asynchronous device-to-host copy carries buffer and CRCs into pinned
        staging; an event is recorded.  The snapshot holds the state at the point of the call in stream order: steps enqueued
        later do not reach it, and the host returns at once.  Snapshot.write(prefix) writes the bundle.
        Refused ahead of any launch: the result of the last step has not been read (under the guard the step count is not
        known until read()); a previous snapshot has been neither written nor released (there is one staging buffer)."""
        if self._pending is not None:
            raise InvalidArgumentError(-1, 'MomentumOptimizer.snapshot: the result of the last step(..., sync=False) has not been read: '
                                           'call its read() first (the step count of a guarded step is not known until then)')
        if self._snapshot is not None:
            raise InvalidArgumentError(-1, 'MomentumOptimizer.snapshot: the previous snapshot has been neither written nor released '
                                           '(Snapshot.write / Snapshot.release): its staging is still in use')
        layout, total = self._state_layout()
        self._snapshot_buffers(layout, total)
        d, dev = self.det, self._snap_dev
        table, _ = train_ops.crc32c_table([(ptr, 4 * math.prod(shape)) for _, ptr, shape, _ in layout],
                                          copy_to=[dev.ptr + off for _, _, _, off in layout], who='snapshot')
        train_ops.crc32c_launch(table, dev.ptr + total, stream=d.stream, workspace=self._snap_ws)
        check(lib().xdet_memcpy_d2h_async(self._snap_host.ptr, dev.ptr, total + 4 * len(layout), d.stream.handle))
        self._snap_event.record(d.stream)
        self._snapshot = Snapshot(self, self.steps, [(name, off, shape) for name, _, shape, off in layout], total, self._snap_event)
        return self._snapshot

    def restore(self, prefix, model_scope='xception_lighthead', slots='require'):
        """Take masters, momentum slots, moving statistics and the step count from the TensorFlow V2 bundle `prefix` (what
        Snapshot.write wrote, or the reference's own model.ckpt-N) back onto the device -> {'step': global_step, 'tensors':
        the checkpoint names restored}.  Everything a step needs is checked ahead of any copy -- every variable, its
        '/Momentum', every moving statistic, and global_step, each float32 (global_step int64) in the variable's shape and
        inside its data shard; a refusal (CheckpointError) names what is missing or mis-shaped -- and an unread pending step or
        a live snapshot is refused (InvalidArgumentError).
        Then the tensors' bytes go from the file into the pinned staging and up into the snapshot buffer; ONE xdet_crc32c
        without destinations checksums them THERE, and the host compares the words with the index's CRCs: the bytes are
        checked as they arrived in device memory.  A mismatch raises CheckpointError naming the tensor, and no master, slot
        or statistic has changed.  Only then does one more table copy the buffer into the live tensors, followed by exactly
        the launches step makes behind the momentum step (_refresh_from_masters), so forward layers and backward operands
        match the masters; `steps` = global_step.  refresh_eval_net() afterwards works as after a step.
        slots='zero': a weights-only checkpoint is accepted -- the momentum slots are zeroed whatever the file holds, and the
        step is 0 where global_step is absent.
        Data-parallel: every rank restores the same file and ends bit-equal."""
        from .tf_checkpoint import CheckpointReader, CheckpointError, DT_FLOAT, DT_INT64, mask_crc
        if slots not in ('require', 'zero'):
            raise InvalidArgumentError(-1, "MomentumOptimizer.restore: slots must be 'require' or 'zero', got %r" % (slots,))
        if self._pending is not None:
            raise InvalidArgumentError(-1, 'MomentumOptimizer.restore: the result of the last step(..., sync=False) has not been read: '
                                           'call its read() first')
        if self._snapshot is not None:
            raise InvalidArgumentError(-1, 'MomentumOptimizer.restore: a snapshot has been neither written nor released: its staging '
                                           'is still in use')
        layout, total = self._state_layout()
        pre = model_scope + '/' if model_scope else ''
        rd = CheckpointReader(prefix)
        bad, plan = [], []                                  # plan: (name, entry or None for zeros, live pointer, shape, offset)
        for name, ptr, shape, off in layout:
            zero = slots == 'zero' and name.endswith('/Momentum')
            e = None if zero else rd.entries.get(pre + name)
            if zero:
                pass
            elif e is None:
                bad.append('%s is missing' % (pre + name))
            elif e['sliced'] or e['dtype'] != DT_FLOAT:
                bad.append('%s is not a dense float32 tensor' % (pre + name))
            elif tuple(e['shape']) != tuple(shape) or e['size'] != 4 * math.prod(shape):
                bad.append('%s has shape %r (%d bytes), the variable %r' % (pre + name, tuple(e['shape']), e['size'], tuple(shape)))
            elif e['offset'] + e['size'] > rd._shard(e['shard_id']).size:
                bad.append('%s lies outside its data shard (truncated)' % (pre + name))
            plan.append((name, e, ptr, shape, off))
        g = rd.entries.get('global_step')
        if g is None and slots == 'require':
            bad.append('global_step is missing')
        elif g is not None and (g['dtype'] != DT_INT64 or tuple(g['shape']) != ()):
            bad.append('global_step is not an int64 scalar')
        if bad:
            raise CheckpointError('MomentumOptimizer.restore: %s: %s%s' % (prefix, '; '.join(bad[:8]),
                                                                           ' (and %d more)' % (len(bad) - 8) if len(bad) > 8 else ''))
        step = int(rd.get_tensor('global_step', verify_crc=True)) if g is not None else 0
        if step < 0:
            raise CheckpointError('MomentumOptimizer.restore: %s: global_step is %d' % (prefix, step))
        self._snapshot_buffers(layout, total)
        d, dev, host = self.det, self._snap_dev, self._snap_host
        for name, e, _, shape, off in plan:                 # file -> staging: a copy, no arithmetic and no checksum on the host
            view = host.view(off, (4 * math.prod(shape),), np.uint8)
            if e is None:
                view[:] = 0
            else:
                view[:] = rd._shard(e['shard_id'])[e['offset']:e['offset'] + e['size']]
        n = len(plan)
        check(lib().xdet_memcpy_h2d(dev.ptr, host.ptr, total, d.stream.handle))
        spans = [(dev.ptr + off, 4 * math.prod(shape)) for _, _, _, shape, off in plan]
        table, _ = train_ops.crc32c_table(spans, who='restore')
        train_ops.crc32c_launch(table, dev.ptr + total, stream=d.stream, workspace=self._snap_ws)
        got = to_host(dev.ptr + total, (n,), np.uint32, d.stream)          # (the one wait of a restore)
        for (name, e, _, _, _), c in zip(plan, got):
            if e is not None and e['crc32c'] is not None and mask_crc(int(c)) != e['crc32c']:
                raise CheckpointError('MomentumOptimizer.restore: %s: %s: tensor checksum mismatch (as it arrived in device memory); '
                                      'nothing was restored' % (prefix, pre + name))
        table, _ = train_ops.crc32c_table(spans, copy_to=[ptr for _, _, ptr, _, _ in plan], who='restore')
        train_ops.crc32c_launch(table, dev.ptr + total + 4 * n, stream=d.stream, workspace=self._snap_ws)
        self._refresh_from_masters()
        self.steps = step
        return {'step': step, 'tensors': [pre + name for name, e, _, _, _ in plan if e is not None] + (['global_step'] if g is not None else [])}


# ---- the single-call driver: one training step from a batch ------------------------------------------------------------------

LOGGED_SCALARS = ('rpn_ce_loss', 'rpn_loc_loss', 'rpn_loss', 'head_loss', 'head_ce_loss', 'head_loc_loss', 'total_loss')


class StepResult(object):
    """What TrainStep.step returns: every scalar of the step is still on the device.  read() -> a dict, after ONE
    synchronisation of the detector's stream (the optimizer's StepPending.read(); a second read() returns the same dict):
    the reference's seven logged scalars under the names of light_head_rfcn_train.py:510-516 -- rpn_ce_loss, rpn_loc_loss,
    rpn_loss, head_loss, head_ce_loss, head_loc_loss (f32 as the loss kernels wrote them) and total_loss =
    ((rpn_ce_loss + rpn_loc_loss) + head_loss) + weight_decay * l2 in f32, the order of line 420 -- and l2, grad_norm, skipped,
    first_bad, step and lr as MomentumOptimizer.step(..., guard=True) returns them (grad_norm, skipped and first_bad only
    from a guarded step), and clip_scale from a clipped one.  Under TrainStep(comm=) on more than one rank the six loss
    scalars are their means over the ranks (averaged on the device behind the step) and total_loss is formed from those."""

    def __init__(self, pending, rpn_losses, head_losses, weight_decay):
        self.pending, self._rpn, self._head, self._wd, self.result = pending, rpn_losses, head_losses, weight_decay, None

    def read(self):
        if self.result is None:
            info = self.pending.read()                     # (the one synchronisation; the downloads below wait for nothing)
            rpn, head = to_host(self._rpn.ptr, (3,)), to_host(self._head.ptr, (3,))
            f = np.float32
            with np.errstate(invalid='ignore', over='ignore'):
                total = ((rpn[0] + rpn[1]) + head[0]) + f(self._wd) * f(info['l2'])
            out = dict(zip(LOGGED_SCALARS, (rpn[0], rpn[1], rpn[2], head[0], head[1], head[2], f(total))))
            out.update(info)
            self.result, self._rpn, self._head = out, None, None
        return self.result


class TrainStep(object):
    """One training step in one call: step(images, glabels, gboxes, n_gt, lr, seed) -> StepResult.  The stages are the chain the
    tests make by hand, on ONE detector and in this order, all on the detector's stream: the anchors' labels and targets
    (encoder.encode_all_anchors(..., keep_device=True)); the eval body (xdet_net_xception_body); stem_train on a detector
    built with it, entry_flow_train, middle_flow_train, exit_flow_train; get_rpn, rpn_decode and get_proposals on the net's own
    buffers (the three C calls, no download and upload of objectness and boxes in between); the sampled ROIs
    (encoder.ext_encode_rois(proposals, ..., keep_device=True)); large_sep_kernel in training mode; get_head on the sampled
    ROIs and the head loss with OHEM (losses.HeadLoss(..., device_result=True)); head_backward(to_feat=True), large_sep_backward,
    losses.rpn_loss(..., device_result=True), rpn_backward, exit_flow_backward (with the RPN's share of d mid),
    middle_flow_backward, entry_flow_backward and, with the stem, stem_backward, all with weight_grads='device'; and
    opt.step(grads, lr, guard=guard, sync=False).  Between the first launch and StepResult.read() the host waits for nothing
    and reads nothing back (runtime.deferred: the stages' closing waits are skipped, buffers that start zeroed are zeroed on
    the stream): the same kernels on the same operands as the chain made by hand, so the same bits.
    The inputs are what augment.preprocess_train leaves on the device: images f32 NCHW [N,3,S,S], glabels i32 [N,1,1,G],
    gboxes f32 [N,G,1,4], n_gt i32 [1,1,1,N], N at most max_batch; host arrays (images [N,3,S,S]; labels and boxes as
    targets.ground_truth takes them, n_gt or None) are uploaded first, which waits for the copies.  step_images(images_u8,
    labels, bboxes, lr, seed) runs augment.preprocess_train(..., seed) in front.
    The sampling seeds are functions of `seed` alone (TrainStep.seeds): the RPN's anchor sampling draws with 2 * seed, the ROI
    sampling with 2 * seed + 1, both modulo 2^32; step_images hands `seed` itself to the augmentation.
    guard=True: a gradient that is not finite skips the update on the device (MomentumOptimizer.step).  The loss buffers, the
    anchor and ROI targets and the guard record are allocated on the first step and reused.
    clip_norm=c and comm (an xdet.dist.Communicator) are handed to opt.step(..., sync=False): the gradients are averaged over
    the ranks and clipped to a global norm of c inside the step, and no host wait happens before StepResult.read(), which
    waits for the communicator under its watchdog first.  With comm on more than one rank a second exchange follows the
    optimizer step on the detector's stream: the moving statistics of every batch norm (stem, flows, large-separable block)
    and the six scalars the loss kernels wrote are replaced in place by their mean over the ranks, so export_weights of any
    rank is one dict and read() returns the rank means (total_loss from them and l2, which is rank-equal already).  A
    communicator of one rank launches nothing extra and keeps the bits of comm=None.
    Refused ahead of any launch, in one sentence that lists everything missing: a detector built without head_rois,
    pool_index, rpn_hidden, large_sep_train or one of the three flow stages, an optimizer of another detector or without
    reach='all', and arguments that differ from what the detector was built with."""

    def __init__(self, det, opt, encoder, *, rpn_anchors_per_image=256, rpn_fg_ratio, roi_one_image, fg_ratio, ohem_roi_one_image,
                 nms_threshold, rpn_min_size, guard=True, allowed_border=0.1, comm=None, clip_norm=None):
        lack = [what for what, have in (('head_rois=%r' % (roi_one_image,), getattr(det, 'head_rois', None) is not None),
                                        ('pool_index=True', getattr(det, 'pool_index', False)),
                                        ('rpn_hidden=True', getattr(det, 'rpn_hidden', False)),
                                        ('large_sep_train=True', getattr(det, 'large_sep_train', False)),
                                        ('exit_flow_train=True', getattr(det, 'exit_flow_train', False)),
                                        ('middle_flow_train=True', getattr(det, 'middle_flow_train', False)),
                                        ('entry_flow_train=True', getattr(det, 'entry_flow_train', False))) if not have]
        needs = ['a detector built with ' + ', '.join(lack)] if lack else []
        if getattr(opt, 'det', None) is not det or getattr(opt, 'reach', None) != 'all':
            needs.append("a MomentumOptimizer(det, reach='all') of this detector")
        if needs:
            raise InvalidArgumentError(-1, 'TrainStep: the step needs ' + ' and '.join(needs))
        cfg = det.cfg
        differ = [what for what, ok in (('roi_one_image = %r (head_rois = %r)' % (roi_one_image, det.head_rois), roi_one_image == det.head_rois),
                                        ('nms_threshold = %r (%r)' % (nms_threshold, cfg.rpn_nms_thres),
                                         np.float32(nms_threshold) == np.float32(cfg.rpn_nms_thres)),
                                        ('rpn_min_size = %r (%r)' % (rpn_min_size, cfg.rpn_min_size),
                                         np.float32(rpn_min_size) == np.float32(cfg.rpn_min_size)),
                                        ('ohem_roi_one_image = %r (1 .. roi_one_image)' % (ohem_roi_one_image,),
                                         isinstance(ohem_roi_one_image, (int, np.integer)) and 1 <= ohem_roi_one_image <= det.head_rois),
                                        ('rpn_anchors_per_image = %r (positive)' % (rpn_anchors_per_image,),
                                         isinstance(rpn_anchors_per_image, (int, np.integer)) and rpn_anchors_per_image > 0),
                                        ('an encoder of %d anchor layers (1)' % len(getattr(encoder, '_anchors', ())),
                                         len(getattr(encoder, '_anchors', ())) == 1)) if not ok]
        if differ:
            raise InvalidArgumentError(-1, 'TrainStep: arguments that differ from what the detector was built with: ' + ', '.join(differ))
        self.det, self.opt, self.encoder, self.guard = det, opt, encoder, bool(guard)
        self.rpn_anchors_per_image, self.rpn_fg_ratio = int(rpn_anchors_per_image), float(rpn_fg_ratio)
        self.roi_one_image, self.fg_ratio, self.ohem_roi_one_image = int(roi_one_image), float(fg_ratio), int(ohem_roi_one_image)
        self.allowed_border = float(allowed_border)
        if comm is not None and not (hasattr(comm, 'average_gradients') and hasattr(comm, 'world')):
            raise InvalidArgumentError(-1, 'TrainStep: comm must be an xdet.dist.Communicator, got %s' % type(comm).__name__)
        if clip_norm is not None and not (isinstance(clip_norm, (int, float, np.floating, np.integer)) and not isinstance(clip_norm, bool)
                                          and np.isfinite(np.float32(clip_norm)) and np.float32(clip_norm) > 0):
            raise InvalidArgumentError(-1, 'TrainStep: clip_norm must be None or a finite positive number, got %r' % (clip_norm,))
        self.comm, self.clip_norm = comm, clip_norm
        self._rank_ws = None                               # the workspace of the second exchange (allocated by the first step)
        self._variables = set(opt.variables)
        self._rpn_buffers, self._head_buffers, self._roi_buffers = {}, {}, {}

    @staticmethod
    def seeds(seed):
        """-> (the seed of the RPN's anchor sampling, the seed of the ROI sampling): 2 * seed and 2 * seed + 1 modulo 2^32"""
        return (2 * int(seed)) & 0xFFFFFFFF, (2 * int(seed) + 1) & 0xFFFFFFFF

    def upload(self, images, glabels, gboxes, n_gt=None):
        """-> the four inputs of step as DeviceTensors in preprocess_train's layout: device tensors pass, host arrays are
        uploaded (each upload waits for its copy); a wrong shape is refused"""
        from . import targets as T
        d, S = self.det, self.det.image_size
        if not isinstance(images, DeviceTensor):
            a = np.ascontiguousarray(images, np.float32)
            if a.ndim == 4 and a.shape[1:] == (3, S, S):
                b = to_device(a)
                images = DeviceTensor(b.ptr, a.shape, S, owner=b)
        if (not isinstance(images, DeviceTensor) or len(images.shape) != 4 or tuple(images.shape[1:]) != (3, S, S) or images.ld != S
                or not 1 <= images.shape[0] <= d.max_batch):
            raise InvalidArgumentError(-1, 'TrainStep.step: images must be f32 [n,3,%d,%d] (NCHW, dense) of 1 to %d images, got %r'
                                           % (S, S, d.max_batch, getattr(images, 'shape', None)))
        if not T._device_ground_truth(glabels, gboxes, n_gt):
            gl, gb, ng = T.ground_truth(glabels, gboxes, n_gt)
            if gl.shape[1] == 0:
                gl, gb = np.zeros((gl.shape[0], 1), np.int32), np.zeros((gl.shape[0], 1, 4), np.float32)
            N, G = gl.shape
            bl, bb, bn = to_device(gl.astype(np.int32)), to_device(gb.astype(np.float32)), to_device(ng.astype(np.int32))
            glabels, gboxes, n_gt = (DeviceTensor(bl.ptr, (N, 1, 1, G), G, owner=bl), DeviceTensor(bb.ptr, (N, G, 1, 4), 4, owner=bb),
                                     DeviceTensor(bn.ptr, (1, 1, 1, N), N, owner=bn))
        if glabels.shape[0] != images.shape[0]:
            raise InvalidArgumentError(-1, 'TrainStep.step: ground truth of %d images for %d images' % (glabels.shape[0], images.shape[0]))
        return images, glabels, gboxes, n_gt

    def step(self, images, glabels, gboxes, n_gt, lr, seed):
        from . import losses as L
        from .runtime import deferred
        d, opt, enc = self.det, self.opt, self.encoder
        if opt._pending is not None:
            raise InvalidArgumentError(-1, 'TrainStep.step: the result of the last step has not been read: call its read() first')
        images, glabels, gboxes, n_gt = self.upload(images, glabels, gboxes, n_gt)
        rpn_seed, roi_seed = self.seeds(seed)
        n, S, A, nc = images.shape[0], d.image_size, d.cfg.num_anchors, d.cfg.num_classes
        h, l = d.stream.handle, lib()
        stem = getattr(d, STEM_STAGE.flag, False)
        with d.scope(), deferred(d.stream):
            new_body(d)                                    # (as set_images: the stages' saved state belongs to the images that go)
            check(l.xdet_memcpy_d2d(d._images.ptr, images.ptr, n * 3 * S * S * 4, h))
            d._N = n
            a_l, a_t, _, _, _ = enc.encode_all_anchors(glabels, gboxes, n_gt, stream=d.stream, keep_device=True)
            check(l.xdet_net_xception_body(d.handle, d._images.ptr, n, h))
            if stem:
                stem_train()
            entry_flow_train()
            middle_flow_train()
            exit_flow_train()
            check(l.xdet_net_get_rpn(d.handle, n, h))
            heads_ran(d, '_rpn_step')
            rpn_out = d.buffer('rpn_out', n)
            cls, box = rpn_out.channels(0, 2 * A), rpn_out.channels(2 * A, 6 * A)
            check(l.xdet_net_rpn_decode(d.handle, n, h))
            check(l.xdet_net_get_proposals(d.handle, n, h))
            rois, r_t, r_l, _ = enc.ext_encode_rois(d.buffer('proposals', n), glabels, gboxes, self.roi_one_image, self.fg_ratio,
                                                    self.allowed_border, seed=roi_seed, n_gt=n_gt, stream=d.stream, keep_device=True,
                                                    buffers=self._roi_buffers)
            d._lsep.forward(d, d.buffer('out', n), n)
            loss_func = L.HeadLoss(r_l, r_t, self.fg_ratio, device_result=True, buffers=self._head_buffers)
            rois_to_head(d, rois, n)
            check(l.xdet_net_get_head(d.handle, n, h))
            heads_ran(d, '_head_step')
            head_res = loss_func(d.buffer('cls_reg', n), None, self.ohem_roi_one_image, nc, stream=d.stream)
            sections = [head_backward(loss_func, to_feat=True, weight_grads='device')]
            sections.append(large_sep_backward(sections[0]['feat'], weight_grads='device'))
            rpn_res = L.rpn_loss(cls, box, a_l[0], a_t[0], self.rpn_anchors_per_image, self.rpn_fg_ratio, seed=rpn_seed, stream=d.stream,
                                 keep_device=True, device_result=True, buffers=self._rpn_buffers)
            sections.append(rpn_backward(rpn_res, weight_grads='device'))
            sections.append(exit_flow_backward(sections[1]['out'], sections[2]['mid'], weight_grads='device'))
            sections.append(middle_flow_backward(sections[3]['mid'], weight_grads='device'))
            sections.append(entry_flow_backward(sections[4]['entry'], weight_grads='device'))
            if stem:
                sections.append(stem_backward(sections[5]['stem'], weight_grads='device'))
            grads = {k: v for sec in sections for k, v in sec.items() if k in self._variables}
            more = {}                                      # (the defaults make the call the driver always made)
            if self.comm is not None:
                more['comm'] = self.comm
            if self.clip_norm is not None:
                more['clip_norm'] = self.clip_norm
            pending = opt.step(grads, lr, guard=self.guard, sync=False, **more)
            pending._alive = (sections, images, glabels, gboxes, n_gt, loss_func, rpn_res)   # (until read(): the stream may still run)
            if self.comm is not None and self.comm.world > 1:
                self._average_over_ranks(rpn_res.losses, head_res.losses)
        return StepResult(pending, rpn_res.losses, head_res.losses, opt.weight_decay)

    def _average_over_ranks(self, rpn_losses, head_losses):
        """The second exchange of a data-parallel step, behind the optimizer step on the detector's stream: what stays per
        rank under MomentumOptimizer.step(comm=) -- the moving_mean and moving_variance of every batch norm a training forward
        moves, and the two loss kernels' three scalars each -- becomes its mean over the ranks, in place
        (Communicator.average_gradients on a table of its own: one handshake, on the first step).  l2 is not in the table:
        it is computed from the masters, which are the same bits on every rank, and total_loss follows from the means."""
        tensors = [DeviceTensor(b.ptr, (bn.co,), bn.co, owner=b) for bn in self.opt._moving_batch_norms()
                   for b in (bn.moving_mean, bn.moving_variance)]
        tensors += [DeviceTensor(b.ptr, (3,), 3, owner=b) for b in (rpn_losses, head_losses)]
        chunk = 1 << 20
        if self._rank_ws is None:
            _, table, sizes, _ = train_ops._grad_table(tensors, chunk)
            self._rank_ws = DeviceBuffer(lib().xdet_grad_average_workspace_bytes(table, len(sizes), self.comm.world, chunk))
        self.comm.average_gradients(tensors, self.det.stream, chunk_elems=chunk, workspace=self._rank_ws)

    def step_images(self, images_u8, labels, bboxes, lr, seed):
        """augment.preprocess_train(images_u8, labels, bboxes, the detector's image size, seed) on the detector's stream, then
        step on what it left on the device"""
        from . import augment
        d = self.det
        return self.step(*augment.preprocess_train(images_u8, labels, bboxes, d.image_size, seed, stream=d.stream), lr, seed)


# ---- the flows' host statements: NumPy, any channel counts and map sizes (the weights and the input decide), float64 as the
# ---- yardstick ---------------------------------------------------------------------------------------------------------------

def _host_depthwise_forward(x, k, relu_in, dtype):
    x, k = np.asarray(x, dtype), np.asarray(k, dtype)
    N, H, W, C = x.shape
    xp = np.pad(np.maximum(x, dtype(0)) if relu_in else x, ((0, 0), (1, 1), (1, 1), (0, 0)))
    out = np.zeros(x.shape, dtype)
    for a in range(3):
        for b in range(3):
            out += xp[:, a:a + H, b:b + W] * k[a, b, :, 0]
    return out


def _host_max_pool_forward(x, dtype):
    """max_pooling2d(3, 2, 'same') of x [N,H,W,C]: padded positions are absent"""
    x = np.asarray(x, dtype)
    N, H, W, C = x.shape
    (Ho, pt), (Wo, pl) = train_ops._same_pad_front(H), train_ops._same_pad_front(W)
    xp = np.full((N, 2 * Ho + 1, 2 * Wo + 1, C), -np.inf, dtype)
    xp[:, pt:pt + H, pl:pl + W] = x
    out = np.full((N, Ho, Wo, C), -np.inf, dtype)
    for a in range(3):
        for b in range(3):
            out = np.maximum(out, xp[:, a:a + 2 * Ho:2, b:b + 2 * Wo:2])
    return out


def _host_bn_forward(z, weights, bn, eps, momentum, dtype, saved):
    """y = BN(z) with batch statistics; saved gains the four statistics under '<bn>/...'"""
    y, mean, invstd, mm, mv = train_ops.host_batch_norm_forward(z, weights[bn + '/gamma'], weights[bn + '/beta'], eps, True, momentum,
                                                          weights[bn + '/moving_mean'], weights[bn + '/moving_variance'], False, dtype)
    saved.update({bn + '/save_mean': mean, bn + '/save_invstd': invstd, bn + '/moving_mean': mm, bn + '/moving_variance': mv})
    return y


def _host_unit_forward(x, weights, unit, relu_in, eps, momentum, dtype, saved):
    """y = BN(pw(dw((relu)(x)))); saved gains '<unit>/dw', '<unit>/z' and the batch norm's statistics"""
    t = _host_depthwise_forward(x, weights[unit + '/depthwise_kernel'], relu_in, dtype)
    z = np.matmul(t, np.asarray(weights[unit + '/pointwise_kernel'], dtype)[0, 0])
    saved[unit + '/dw'], saved[unit + '/z'] = t, z
    return _host_bn_forward(z, weights, unit + '_bn', eps, momentum, dtype, saved)


def _host_bn_backward(saved, weights, z, bn, dy, dtype):
    vec = lambda a: np.asarray(a, dtype).reshape(-1)
    return train_ops.host_batch_norm_backward(saved[z], None, dy, weights[bn + '/gamma'], vec(saved[bn + '/save_mean']),
                                        vec(saved[bn + '/save_invstd']), True, dtype)


def _host_unit_backward(x, dy, saved, weights, unit, relu_in, dtype, out):
    """d loss / d y -> d loss / d x through the unit's BN, 1x1 conv and depthwise conv; out gains the unit's four weight
    gradients, 'dw/<unit>' and 'z/<unit>'"""
    bn = unit + '_bn'
    dz, out[bn + '/gamma'], out[bn + '/beta'] = _host_bn_backward(saved, weights, unit + '/z', bn, dy, dtype)
    dt, out[unit + '/pointwise_kernel'], _ = train_ops.host_conv_backward(saved[unit + '/dw'], weights[unit + '/pointwise_kernel'], dz, None, False, dtype)
    dx, out[unit + '/depthwise_kernel'] = train_ops.host_depthwise_backward(x, weights[unit + '/depthwise_kernel'], dt, 1, relu_in, dtype)
    out['dw/' + unit], out['z/' + unit] = dt, dz
    return dx


def host_middle_flow_train(entry_x, weights, dtype=np.float64, blocks=MIDDLE_FLOW_BLOCKS):
    """The NumPy statement of middle_flow_train: entry_x [N,h,w,C] and the blocks' variables and moving statistics under the
    checkpoint's names (C comes from the weights) -> (mid_x, saved): the output of the last block and a dict with
    detector.middle_flow_saved()'s keys for `blocks` -- 'x<b>', '<unit>/dw', '<unit>/z', 'block<b>/y1', 'block<b>/y2', and per
    batch norm '/save_mean', '/save_invstd', '/moving_mean', '/moving_variance' [C] (the moving ones after TensorFlow's
    update as train_ops.host_batch_norm_forward states it) -- plus 'block<b>/y3'."""
    x, saved = np.asarray(entry_x, dtype), {}
    for b in blocks:
        saved['x%d' % b] = x
        y = x
        for i in (1, 2, 3):
            y = saved['block%d/y%d' % (b, i)] = _host_unit_forward(y, weights, 'block%d_sepconv%d' % (b, i), True, MIDDLE_FLOW_EPS,
                                                                   MIDDLE_FLOW_MOMENTUM, dtype, saved)
        x = y + x
    return x, saved


def host_middle_flow_backward(saved, weights, d_mid, dtype=np.float64, blocks=MIDDLE_FLOW_BLOCKS):
    """The NumPy statement of middle_flow_backward(d_mid, intermediates=True): saved = what host_middle_flow_train (or
    detector.middle_flow_saved(), as NumPy arrays) left, d_mid = d loss / d (the last block's output) -> a dict with the four
    gradients of every unit of `blocks` under the checkpoint's names and in its shapes, 'entry' = d loss / d (the first block's
    input), 'x<b>' for every later block, 'dw/<unit>', 'z/<unit>' and 'd3/block<b>', 'd2/block<b>', 'd1/block<b>'.  Composed of train_ops.host_batch_norm_backward,
    train_ops.host_conv_backward and train_ops.host_depthwise_backward."""
    blocks = tuple(blocks)
    g, out = np.asarray(d_mid, dtype), {}
    for b in reversed(blocks):
        dy = g
        for i, xin in ((3, saved['block%d/y2' % b]), (2, saved['block%d/y1' % b]), (1, saved['x%d' % b])):
            dy = out['d%d/block%d' % (i, b)] = _host_unit_backward(xin, dy, saved, weights, 'block%d_sepconv%d' % (b, i), True, dtype, out)
        g = dy + g
        out['entry' if b == blocks[0] else 'x%d' % b] = g
    return out


def host_entry_flow_train(stem_out, weights, dtype=np.float64, blocks=ENTRY_FLOW_BLOCKS):
    """The NumPy statement of entry_flow_train: stem_out [N,h,w,C] (the first block's input) and the blocks' variables and
    moving statistics under the checkpoint's names (the channel counts come from the weights) -> (entry_x, saved): the output
    of the last block and a dict with detector.entry_flow_saved()'s keys for `blocks` -- 'x<b>', 'block<b>/xs',
    'conv2d_<b-1>/z', 'block<b>/r', '<unit>/dw', '<unit>/z', 'block<b>/y1', 'block<b>/y2', and per batch norm '/save_mean',
    '/save_invstd', '/moving_mean', '/moving_variance' [C] (the moving ones after TensorFlow's update as
    train_ops.host_batch_norm_forward states it)."""
    x, saved = np.asarray(stem_out, dtype), {}
    for b in blocks:
        saved['x%d' % b] = x
        proj = 'conv2d_%d' % (b - 1)
        xs = train_ops.host_subsample2(x, dtype)
        zr = np.matmul(xs, np.asarray(weights[proj + '/kernel'], dtype)[0, 0])
        r = _host_bn_forward(zr, weights, 'batch_normalization_%d' % (b - 1), ENTRY_FLOW_EPS, ENTRY_FLOW_MOMENTUM, dtype, saved)
        saved['block%d/xs' % b], saved[proj + '/z'], saved['block%d/r' % b] = xs, zr, r
        y = x
        for i in (1, 2):
            y = saved['block%d/y%d' % (b, i)] = _host_unit_forward(y, weights, 'block%d_sepconv%d' % (b, i), _entry_relu_in(b, i),
                                                                   ENTRY_FLOW_EPS, ENTRY_FLOW_MOMENTUM, dtype, saved)
        x = _host_max_pool_forward(y, dtype) + r
    saved['x%d' % (blocks[-1] + 1)] = x
    return x, saved


def host_entry_flow_backward(saved, weights, d_entry, dtype=np.float64, blocks=ENTRY_FLOW_BLOCKS):
    """The NumPy statement of entry_flow_backward(d_entry, intermediates=True): saved = what host_entry_flow_train (or
    detector.entry_flow_saved(), as NumPy arrays) left, d_entry = d loss / d (the last block's output) -> a dict with the eleven
    gradients of every block of `blocks` under the checkpoint's names and in its shapes, 'stem' = d loss / d (the first block's
    input), 'x<b>' for every later block, and 'dxs/block<b>', 'z/conv2d_<b-1>', 'dy2/block<b>', 'd2/block<b>', 'd1/block<b>',
    'dw/<unit>', 'z/<unit>'.  Composed of train_ops.host_batch_norm_backward, train_ops.host_conv_backward, train_ops.host_depthwise_backward,
    train_ops.host_max_pool_backward and train_ops.host_add_upsample2."""
    blocks = tuple(blocks)
    g, out = np.asarray(d_entry, dtype), {}
    for b in reversed(blocks):
        proj, bn = 'conv2d_%d' % (b - 1), 'batch_normalization_%d' % (b - 1)
        dzr, out[bn + '/gamma'], out[bn + '/beta'] = _host_bn_backward(saved, weights, proj + '/z', bn, g, dtype)
        dxs, out[proj + '/kernel'], _ = train_ops.host_conv_backward(saved['block%d/xs' % b], weights[proj + '/kernel'], dzr, None, False, dtype)
        out['z/' + proj], out['dxs/block%d' % b] = dzr, dxs
        dy = out['dy2/block%d' % b] = train_ops.host_max_pool_backward(saved['block%d/y2' % b], g, dtype)
        for i, xin in ((2, saved['block%d/y1' % b]), (1, saved['x%d' % b])):
            dy = out['d%d/block%d' % (i, b)] = _host_unit_backward(xin, dy, saved, weights, 'block%d_sepconv%d' % (b, i),
                                                                   _entry_relu_in(b, i), dtype, out)
        g = train_ops.host_add_upsample2(dy, dxs, dtype)
        out['stem' if b == blocks[0] else 'x%d' % b] = g
    return out


def _host_valid_conv(x, k, stride, dtype):
    """conv(x [N,H,W,C], k [kh,kw,C,J]) at `stride`, 'VALID': one matrix product per tap, the taps added in storage order"""
    x, k = np.asarray(x, dtype), np.asarray(k, dtype)
    kh, kw = k.shape[:2]
    Ho, Wo = (x.shape[1] - kh) // stride + 1, (x.shape[2] - kw) // stride + 1
    out = np.zeros((x.shape[0], Ho, Wo, k.shape[3]), dtype)
    for a in range(kh):
        for b in range(kw):
            out += np.matmul(x[:, a:a + (Ho - 1) * stride + 1:stride, b:b + (Wo - 1) * stride + 1:stride], k[a, b])
    return out


def host_stem_train(images_nchw, weights, dtype=np.float64):
    """The NumPy statement of stem_train: images [N,3,S,S] and the stem's variables and moving statistics under the checkpoint's
    names (the channel counts come from the weights) -> (stem_out, saved): relu(BN(conv(relu(BN(conv(images)))))) and a dict
    with detector.stem_saved()'s keys -- 'x1' (the images as NHWC), 'block1_conv1/z', 'a1', 'block1_conv2/z', 'x2' (stem_out)
    and per batch norm '/save_mean', '/save_invstd', '/moving_mean', '/moving_variance' [C] (the moving ones after
    TensorFlow's update as train_ops.host_batch_norm_forward states it)."""
    saved = {'x1': np.ascontiguousarray(np.transpose(np.asarray(images_nchw, dtype), (0, 2, 3, 1)))}
    x = saved['x1']
    for conv, stride, z, y in (('block1_conv1', 2, 'block1_conv1/z', 'a1'), ('block1_conv2', 1, 'block1_conv2/z', 'x2')):
        saved[z] = _host_valid_conv(x, weights[conv + '/kernel'], stride, dtype)
        x = saved[y] = np.maximum(_host_bn_forward(saved[z], weights, conv + '_bn', STEM_EPS, STEM_MOMENTUM, dtype, saved), dtype(0))
    return x, saved


def host_stem_backward(saved, weights, d_stem, dtype=np.float64):
    """The NumPy statement of stem_backward(d_stem, intermediates=True): saved = what host_stem_train (or detector.stem_saved(),
    as NumPy arrays) left, d_stem = d loss / d stem_out -> a dict with the six gradients under the checkpoint's names and in
    its shapes, 'z/block1_conv2', 'a/block1_conv1' and 'z/block1_conv1'.  Composed of train_ops.host_batch_norm_backward and
    train_ops.host_conv_backward_strided ('VALID'; stride 1, then stride 2 without dx): there is no image gradient."""
    vec = lambda a: np.asarray(a, dtype).reshape(-1)
    g, out = np.asarray(d_stem, dtype), {}
    for conv, stride, z, y, x, dx in (('block1_conv2', 1, 'block1_conv2/z', 'x2', 'a1', 'a/block1_conv1'),
                                      ('block1_conv1', 2, 'block1_conv1/z', 'a1', 'x1', None)):
        bn = conv + '_bn'
        dz, out[bn + '/gamma'], out[bn + '/beta'] = train_ops.host_batch_norm_backward(
            saved[z], saved[y], g, weights[bn + '/gamma'], vec(saved[bn + '/save_mean']), vec(saved[bn + '/save_invstd']), True, dtype)
        g, out[conv + '/kernel'], _ = train_ops.host_conv_backward_strided(saved[x], weights[conv + '/kernel'], dz, dtype=dtype,
                                                                          with_dx=dx is not None, stride=stride, padding='VALID')
        out['z/' + conv] = dz
        if dx is not None:
            out[dx] = g
    return out
