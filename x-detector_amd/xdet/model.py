"""The Light-Head R-CNN eval graph behind the reference's graph-builder API.

`LightHeadDetector` owns the native net (weights + workspace); the module-level
functions carry the reference's names and argument order (net/xception_body.py:236,
381,402,450,477) and operate on the detector that is current (`with det.scope():`,
the counterpart of `tf.variable_scope(params['model_scope'])`,
light_head_rfcn_eval.py:382).  Tensors are DeviceTensor views of the net's workspace.
The training graph -- the stages a detector can be built to run with batch statistics, their backwards, the head's and the
RPN head's backward and the host statements -- is xdet/train.py; its public names are re-exported here, and
large_sep_kernel(..., is_training=True) and the detector's *_saved() methods hand over to it.
"""
import contextlib
import ctypes

import numpy as np

from ._lib import lib, check, c_void_p, LightHeadConfig, XdetError, InvalidArgumentError
from .runtime import DeviceBuffer, DeviceTensor, Stream, to_host, synchronize, _host, _current, _det, _sync
from . import train as _train
from .train import *                  # noqa: F401,F403  (the training graph's names are this module's too)


class LightHeadDetector(object):
    def __init__(self, weights, image_size=480, max_batch=1, num_classes=21, rpn_pre_nms_top_n=5000,
                 rpn_post_nms_top_n=1000, rpn_nms_thres=0.7, rpn_min_size=None, select_threshold=0.01,
                 nms_threshold=0.3, nms_topk=200, device=None, large_sep='auto', sepconv='fused', rpn_stream='side',
                 conv3x3='patch', pool='split', check_range=False, ksplit=True, cross='f16', workspace=None, pool_sub=None,
                 pool_index=False, rpn_hidden=False, large_sep_train=False, exit_flow_train=False, middle_flow_train=False,
                 entry_flow_train=False, stem_train=False, keep=(), spectral_refresh=False, head_rois=None, eval_head=False):
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
        none of this.
        stem_train=True (needs entry_flow_train=True: the training-mode `stem_out` it writes is consumed by the training-mode
        entry flow): the six variables of the two stem convs (STEM_VARIABLES) and the moving statistics of their two batch
        norms are kept unfolded on the device, with block1_conv2 as a conv layer of its own, the image as NHWC4 rows, the
        tensors a training forward saves (z1, a1, z2), the three gradient tensors of the backward and the workspaces, all sized
        for max_batch: model.stem_train() recomputes `stem_out` from the images with batch statistics, model.stem_backward
        takes the gradient from `stem_out` down to both kernels.  With it MomentumOptimizer steps the whole network.  The
        default detector allocates and runs none of this.
        keep=('stem_out', 'entry_x'): the eval body keeps these tensors as named buffers (the options the training stages
        set for themselves) without any training state -- for looking at the entry flow stage by stage.
        spectral_refresh=True: a detector whose large-separable block is in the spectral form (large_sep='spectral', or 'auto'
        where that resolves to it) lets refresh_heads take the large_sep_feature group: the block matrices of its two spectral
        layers are evaluated from the merged kernels on the device (option "spectral_refresh", include/xdet.h).  The default
        refuses that group on such a detector; the forward is the same either way.
        head_rois=P (1 <= P <= rpn_post_nms_top_n; option "head_rois", include/xdet.h): the head stage -- `pooled`, `fc`,
        `cls_reg`, `pool_index` -- is planned on P rows per image, the ROIs a training step samples from the proposals, and
        reads them from the buffer 'head_rois' [max_batch, P, 1, 4]; the proposal stage keeps rpn_post_nms_top_n.  `head_R` is
        P then (else rpn_post_nms_top_n): get_head(..., is_training=True) takes P ROIs per image, a DeviceTensor of them by a
        device-to-device copy, and head_backward, MomentumOptimizer and refresh_eval_net work on this one detector.  Such a
        detector has no eval forward: forward, calibrate, detect_images, detect_jpegs, evaluate* and
        get_head(..., is_training=False) refuse by naming the option.  The default (None) is the detector as ever.
        eval_head=True (needs head_rois=P; option "eval_head", include/xdet.h): the training detector also evaluates.  A
        second head stage on the same two dense layers runs on all rpn_post_nms_top_n proposals over its own buffers
        ('pooled_eval', 'fc_eval', 'cls_reg_eval'), and forward, detect_images, detect_jpegs and evaluate* work as on a
        detector built without head_rois from the same weights, bit for bit -- after MomentumOptimizer.refresh_eval_net()
        from the trained ones.  An eval forward is a new body: the training stages' saved state is dropped, and the
        sampled-row buffers keep what they held.  calibrate and get_head(..., is_training=False) still refuse.
        rpn_post_nms_top_n may be up to 6144: above 1024 ROIs per image the detection tail is bboxes_eval's wide form."""
        self.head_rois = _train.check_head_rois(head_rois, rpn_post_nms_top_n)
        self.eval_head = _train.check_eval_head(eval_head, self.head_rois)
        stages = (large_sep_train, exit_flow_train, middle_flow_train, entry_flow_train)
        _train.check_stages(stages, weights)
        _train.check_stem(stem_train, entry_flow_train, weights)
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
        # both heads' kernels and biases as the checkpoint stores them: the kernels are what head_backward / rpn_backward make
        # their operands from, all of them MomentumOptimizer(reach='all')'s masters
        self._head_weights, self._rpn_weights = {}, {}
        for name, arr in weights.items():
            a = np.ascontiguousarray(arr, np.float32)
            if name in _train.HEAD_VARIABLES:
                self._head_weights[name] = a
            if rpn_hidden and name in _train.RPN_HEAD_VARIABLES:
                self._rpn_weights[name] = a
            dims = (ctypes.c_int64 * a.ndim)(*a.shape)
            check(lib().xdet_net_set_weight(self.handle, name.encode(), _host(a), a.ndim, dims))
        check(lib().xdet_net_set_option(self.handle, b'large_sep', large_sep.encode()))
        if spectral_refresh:
            check(lib().xdet_net_set_option(self.handle, b'spectral_refresh', b'on'))
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
        if self.head_rois is not None:
            check(lib().xdet_net_set_option(self.handle, b'head_rois', str(self.head_rois).encode()))
        if self.eval_head:
            check(lib().xdet_net_set_option(self.handle, b'eval_head', b'on'))
        if set(keep) - {'stem_out', 'entry_x'}:
            raise InvalidArgumentError(-1, 'keep: %r is not one of stem_out, entry_x' % (sorted(set(keep) - {'stem_out', 'entry_x'}),))
        if middle_flow_train or 'entry_x' in keep:
            check(lib().xdet_net_set_option(self.handle, b'entry_x', b'keep'))
        if entry_flow_train or 'stem_out' in keep:
            check(lib().xdet_net_set_option(self.handle, b'stem_out', b'keep'))
        self.pool_index, self.rpn_hidden = bool(pool_index), bool(rpn_hidden)
        check(lib().xdet_net_build(self.handle))
        self.max_batch = max_batch
        self.image_size = image_size
        self.num_classes = num_classes
        self.R = rpn_post_nms_top_n
        self.head_R = self.head_rois if self.head_rois is not None else self.R      # rows of the head stage
        self.nms_topk = nms_topk
        self.stream = Stream()
        B, nc, k = max_batch, num_classes - 1, nms_topk
        self._images = DeviceBuffer(B * 3 * image_size * image_size * 4)
        self._det_scores = DeviceBuffer(B * nc * k * 4)
        self._det_boxes = DeviceBuffer(B * nc * k * 16)
        self._N = 0
        _train.build_stages(self, stages, weights)       # self.large_sep_train ... self.entry_flow_train and their states
        self.stem_train = bool(stem_train)               # the fifth stage, next to the table (train.STEM_STAGE)
        if stem_train:
            self._stem = _train.StemState(self, weights)

    def large_sep_saved(self):
        """what the last large_sep_kernel(..., is_training=True) left on the device, as DeviceTensors: 't' [n,h,w,2*mid] =
        conv_a(out) + b_a, 'z' [n,h,w,co] = conv_b(t) + b_b (the batch norm's input), 'save_mean' and 'save_invstd'
        [1,1,1,co] (the batch statistics), 'moving_mean' and 'moving_variance' [1,1,1,co] (after their update)"""
        return _train.saved(self, _train.LARGE_SEP)

    def exit_flow_saved(self):
        """what the last model.exit_flow_train() left on the device, as DeviceTensors: per separable unit '<unit>/dw' (the
        depthwise conv's output, the pointwise conv's input) and '<unit>/z' (the pointwise conv's output, the batch norm's
        input), 'conv2d_4/z'; 'a', 'r', 'y2' (block13_sepconv2's batch norm output, b2 = y2 + r), 'b2', 'c3'; and per batch
        norm '<bn>/save_mean', '<bn>/save_invstd' (the batch statistics), '<bn>/moving_mean', '<bn>/moving_variance' (after
        their update), each [1,1,1,C]"""
        return _train.saved(self, _train.EXIT)

    def middle_flow_saved(self):
        """what the last model.middle_flow_train() left on the device, as DeviceTensors of the n images it ran on: per unit
        '<unit>/dw' (the depthwise conv's output) and '<unit>/z' (the batch norm's input); the block inputs 'x5' (the net's
        `entry_x`) ... 'x12' (block b's output is 'x<b+1>', block 12's the net's `mid_x`); 'block<b>/y1', 'block<b>/y2' (the
        first two batch norm outputs; the third is overwritten by the residual add, y3 + x, in place); and per batch norm
        '<unit>_bn/save_mean', '/save_invstd' (the batch statistics), '/moving_mean', '/moving_variance' (after their update),
        each [1,1,1,728]"""
        return _train.saved(self, _train.MIDDLE)

    def entry_flow_saved(self):
        """what the last model.entry_flow_train() left on the device, as DeviceTensors of the n images it ran on: the block
        inputs 'x2' (the net's `stem_out`), 'x3', 'x4' and 'x5' (block 4's output, the net's `entry_x`); per block 'block<b>/xs'
        (the subsampled input), 'conv2d_<b-1>/z' (the projection's output, its batch norm's input), 'block<b>/r' (that batch
        norm's output, the shortcut), 'block<b>/y1', 'block<b>/y2' (the units' batch norm outputs; y2 is the pool's input); per
        unit '<unit>/dw' (the depthwise conv's output) and '<unit>/z' (the batch norm's input); and per batch norm
        '<bn>/save_mean', '/save_invstd' (the batch statistics), '/moving_mean', '/moving_variance' (after their update), each
        [1,1,1,C]"""
        return _train.saved(self, _train.ENTRY)

    def stem_saved(self):
        """what the last model.stem_train() left on the device, as DeviceTensors of the n images it ran on: 'x1' (the images as
        NHWC rows of 4 floats, what block1_conv1's dW reads), 'block1_conv1/z' (the first conv's output, its batch norm's
        input), 'a1' (that batch norm's ReLU output), 'block1_conv2/z', 'x2' (the net's `stem_out`); and per batch norm
        '<bn>/save_mean', '/save_invstd' (the batch statistics), '/moving_mean', '/moving_variance' (after their update), each
        [1,1,1,C]"""
        return _train.saved(self, _train.STEM)

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
        if name in ('objectness', 'rpn_boxes', 'proposals', 'head_boxes', 'head_rois'):
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
        """whitened f32 [N,3,S,S] -> the detector's image buffer (what XceptionBody, forward and calibrate run on) -> N.  The
        eval body that follows overwrites `stem_out`, `entry_x`, `mid_x` and `out`, so every training stage's saved state is
        dropped here: a *_backward or *_saved() refuses until its training forward has run on the new tensors."""
        a = np.ascontiguousarray(images_nchw, np.float32)
        assert a.ndim == 4 and a.shape[1] == 3 and a.shape[2] == a.shape[3] == self.image_size, a.shape
        assert a.shape[0] <= self.max_batch
        _train.new_body(self)                            # (the stages' saved state belongs to the images that go now)
        check(lib().xdet_memcpy_h2d(self._images.ptr, _host(a), a.nbytes, self.stream.handle))
        self._N = a.shape[0]
        return self._N

    # ---- the whole forward (lighr_head_model_fn, eval) -----------------------------------
    def forward_device(self, n=None, use_graph=False, images_ptr=None, image_shapes_ptr=None, bbox_img_ptr=None,
                       det_scores_ptr=None, det_boxes_ptr=None):
        """asynchronous: images already resident (set_images or caller-owned device pointer).  Like set_images, a caller-owned
        pointer drops what the training stages had saved (train.new_body)."""
        n = n or self._N
        if images_ptr:
            _train.new_body(self)                        # (images that never went through set_images)
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

    def refresh_weights(self, tensors):
        """Refresh the eval net's body from weights on the device (xdet_net_refresh_weights): tensors is {checkpoint name: dense
        f32 DeviceTensor or DeviceBuffer in the checkpoint's shape} over whole layer groups of the body's blocks 2-14 (a unit's
        two kernels and the four arrays of its batch norm; a projection's kernel and its batch norm's four; train.eval_net_groups).
        The batch norms are folded on the device, all touched layers repacked by one table, the stream synchronised and the
        host state a calibration works from brought back in line; exponents, plane_scales() and the captured graphs stay.
        Refused ahead of any GPU work, by name: a host array, a name outside the reach, a group given in part."""
        from ._lib import NetWeightDev
        for name, t in tensors.items():
            if not isinstance(t, (DeviceTensor, DeviceBuffer)) or not t.ptr:
                raise InvalidArgumentError(-1, 'refresh_weights: %s must be a DeviceTensor or a DeviceBuffer (device memory), got %s'
                                           % (name, type(t).__name__))
        _train.eval_net_groups(tensors)
        table = (NetWeightDev * max(len(tensors), 1))()
        for i, (name, t) in enumerate(tensors.items()):
            table[i] = NetWeightDev(name.encode(), t.ptr)
        check(lib().xdet_net_refresh_weights(self.handle, table, len(tensors), self.stream.handle))

    def refresh_heads(self, tensors):
        """Refresh the layers the net's plan owns from weights on the device (xdet_net_refresh_heads): tensors is {checkpoint name:
        dense f32 DeviceTensor or DeviceBuffer in the checkpoint's shape} over whole groups -- 'rpn_head' (train.RPN_HEAD_VARIABLES),
        'final_head' (train.HEAD_VARIABLES), 'large_sep_feature' (train.LARGE_SEP_VARIABLES + LARGE_SEP_MOVING; a net whose block
        is in the direct form, large_sep='direct', or a spectral one built with spectral_refresh=True, whose two layers then
        evaluate their DFT-domain block matrices from the merged kernels on the device).  The merges run on the device into
        scratch the net owns, the touched layers are repacked by one table (the spectral layers by their own door), the stream is
        synchronised and the host state a calibration works from brought back in line; exponents, plane_scales() and the
        captured graphs stay.  Refused ahead of any GPU work, by name: a host array, a name outside the three groups, a group
        given in part, a duplicate, the large_sep_feature group on a spectral block built without spectral_refresh=True."""
        from ._lib import NetWeightDev
        for name, t in tensors.items():
            if not isinstance(t, (DeviceTensor, DeviceBuffer)) or not t.ptr:
                raise InvalidArgumentError(-1, 'refresh_heads: %s must be a DeviceTensor or a DeviceBuffer (device memory), got %s'
                                           % (name, type(t).__name__))
        table = (NetWeightDev * max(len(tensors), 1))()
        for i, (name, t) in enumerate(tensors.items()):
            table[i] = NetWeightDev(name.encode(), t.ptr)
        check(lib().xdet_net_refresh_heads(self.handle, table, len(tensors), self.stream.handle))

    def refresh_stem(self, tensors):
        """Refresh the eval net's stem from weights on the device (xdet_net_refresh_stem): tensors is {checkpoint name: dense f32
        DeviceTensor or DeviceBuffer in the checkpoint's shape} over whole groups -- 'block1_conv1' and 'block1_conv2', each
        <conv>/kernel and the four arrays of <conv>_bn (train.STEM_VARIABLES + STEM_MOVING).  The batch norms are folded on the
        device; block1_conv2 is repacked by the table door, block1_conv1's kernel copied into the net's array and its folded
        scale and shift uploaded again at the plane's current exponent; the stream is synchronised and the host state a
        calibration works from brought back in line; exponents, plane_scales() and the captured graphs stay.
        Refused ahead of any GPU work, by name: a host array, a name outside the two groups, a group given in part."""
        from ._lib import NetWeightDev
        for name, t in tensors.items():
            if not isinstance(t, (DeviceTensor, DeviceBuffer)) or not t.ptr:
                raise InvalidArgumentError(-1, 'refresh_stem: %s must be a DeviceTensor or a DeviceBuffer (device memory), got %s'
                                           % (name, type(t).__name__))
        groups = {c: [c + '/kernel'] + ['%s_bn/%s' % (c, k) for k in ('gamma', 'beta', 'moving_mean', 'moving_variance')]
                  for c in _train.STEM_CONVS}
        for name in tensors:
            if not any(name in want for want in groups.values()):
                raise InvalidArgumentError(-1, 'refresh_stem: %s is outside the reach (the kernels and batch norms of block1_conv1 '
                                               'and block1_conv2)' % name)
        for c, want in groups.items():
            miss = [n for n in want if n not in tensors]
            if miss and len(miss) != len(want):
                raise InvalidArgumentError(-1, 'refresh_stem: the group of %s is given in part: %s is missing' % (c, ', '.join(miss)))
        table = (NetWeightDev * max(len(tensors), 1))()
        for i, (name, t) in enumerate(tensors.items()):
            table[i] = NetWeightDev(name.encode(), t.ptr)
        check(lib().xdet_net_refresh_stem(self.handle, table, len(tensors), self.stream.handle))

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

        def upload(bufs):
            h = self.stream.handle
            check(lib().xdet_memcpy_h2d(bufs['packed'].ptr, _host(packed), packed.nbytes, h))
            check(lib().xdet_memcpy_h2d(bufs['offsets'].ptr, _host(offsets), offsets.nbytes, h))
            check(lib().xdet_memcpy_h2d(bufs['shapes'].ptr, _host(shapes), shapes.nbytes, h))
            self._host_keep = (packed, offsets, shapes)  # (referenced until the next call: nothing waits for the copies here)
        return self._forward_u8(n, mode, packed.nbytes, upload, use_graph)

    def _forward_u8(self, n, mode, packed_nbytes, fill, use_graph):
        """The ingest doors' common tail: fill(bufs) puts n images of packed_nbytes bytes into the ingest's device buffers
        ('packed', 'offsets', 'shapes') on self.stream, then xdet_net_forward_u8 runs on them -> n."""
        bufs = self._ingest_buffers(packed_nbytes)
        _train.new_body(self)
        fill(bufs)
        # packed_bytes = the buffer's capacity: the graph key stays the same for every batch that fits
        check(lib().xdet_net_forward_u8(self.handle, bufs['packed'].ptr, bufs['packed'].nbytes, bufs['offsets'].ptr,
                                        bufs['shapes'].ptr, n, int(mode), self._images.ptr, bufs['bbox_img'].ptr,
                                        self._det_scores.ptr, self._det_boxes.ptr, 1 if use_graph else 0, self.stream.handle))
        self._N = n
        return n

    def _ingest_buffers(self, packed_nbytes):
        """the ingest's device buffers, `packed` holding at least packed_nbytes"""
        B = self.max_batch
        if not hasattr(self, '_ingest'):
            # offsets / image_shapes / bbox_img: max_batch entries, allocated once.  packed grows only: a regrown buffer
            # has another pointer and size, so the next call captures a new graph instead of replaying one that
            # reads the old buffer.
            self._ingest = {'offsets': DeviceBuffer(B * 8), 'shapes': DeviceBuffer(B * 8),
                            'bbox_img': DeviceBuffer(B * 16), 'packed': None}
        bufs = self._ingest
        if bufs['packed'] is None or bufs['packed'].nbytes < packed_nbytes:
            cap = max(packed_nbytes, 2 * bufs['packed'].nbytes if bufs['packed'] is not None else 0)
            bufs['packed'] = DeviceBuffer(cap)
        return bufs

    def detect_jpegs(self, datas, resize=None, use_graph=True):
        """detect_images from encoded baseline JPEGs (xdet.jpeg: the accepted forms and the refusals): the entropy streams
        are decoded on the host, the decode kernels write the pixels into the ingest's own packed buffer, and
        xdet_net_forward_u8 runs on them on the same stream -- no pixel upload, no host round trip.  The result equals
        detect_images on the decoded arrays bit for bit, and batches of other sizes replay the same graph."""
        from . import jpeg, ops
        mode = ops._resize_mode(ops.Resize.WARP_RESIZE if resize is None else resize)
        batch = jpeg._check_jpegs(datas, 'detect_jpegs', self.max_batch)
        ops._check_sizes_for_mode(batch.shapes, self.image_size, mode, 'detect_jpegs: ')

        def decode(bufs):
            self._jpeg_workspace = jpeg._decode_into('detect_jpegs', batch, bufs['packed'], bufs['offsets'], bufs['shapes'],
                                                     self.stream, None, getattr(self, '_jpeg_workspace', None))
        n = self._forward_u8(batch.n, mode, batch.nbytes, decode, use_graph)
        s, b = self.detections(n)
        return [{c + 1: (s[i, c], b[i, c]) for c in range(self.num_classes - 1)} for i in range(n)]

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
        cr = self.buffer('cls_reg', n).numpy().reshape(n, self.head_R, -1)
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
    _train.heads_ran(d, '_rpn_step')
    _sync(d)
    out = d.buffer('rpn_out', n)
    return out.channels(0, 2 * num_anchors), out.channels(2 * num_anchors, 6 * num_anchors)


def large_sep_kernel(net_input, depth_mid, depth_output, is_training, data_format, var_scope):
    """net/xception_body.py:450-475 -> thin feature map [N,h,w,depth_output].
    is_training=True (a detector built with large_sep_train=True): the block as the reference trains it, t = conv_a(out) + b_a,
    z = conv_b(t) + b_b on the merged kernels (xdet_conv_forward, split precision, f32 out), then feat = relu(bn(z)) with the
    batch's statistics and the moving-average updates (xdet_batch_norm_forward, eps 1e-5, momentum 0.997) written straight
    into the net's `feat` buffer -- three calls on the detector's stream with no host round trip in between.  t, z and the
    statistics stay on the device (detector.large_sep_saved()) for large_sep_backward, until a training forward of one
    of the flows or a new eval body (set_images, forward, calibrate, detect_images) runs: either drops them."""
    d = _det()
    n = net_input.shape[0]
    if is_training and not d.large_sep_train:
        raise InvalidArgumentError(-1, 'large_sep_kernel: is_training=True needs a detector built with large_sep_train=True '
                                       '(the default detector folds the moving statistics into the conv weights)')
    view = d.buffer('out', n)
    if not _same(net_input, view):
        d.write('out', net_input.numpy() if isinstance(net_input, DeviceTensor) else net_input)
    if is_training:
        return d._lsep.forward(d, view, n)
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
    row count is fixed when the detector is built: proposals_bboxes.shape[1] must equal its head_R -- head_rois on a detector
    built with that option, which then holds the proposal stage at rpn_post_nms_top_n and the head on the sampled set, else
    rpn_post_nms_top_n (a head detector built with rpn_post_nms_top_n = the ROIs sampled per image).  On a head_rois detector
    the ROIs go into the net's `head_rois` buffer: a DeviceTensor [N,P,(1,)4] (what ext_encode_rois(..., keep_device=True)
    returns) by one device-to-device copy on the detector's stream -- none when it is that buffer -- and a host array by an
    upload; is_training=False is refused there, the eval head and its tail need a detector without the option.
    `pooling_op` is accepted for signature parity; the fused HIP
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
        if proposals_bboxes.shape[1] != d.head_R:
            raise InvalidArgumentError(-1, 'get_head: %d ROIs per image but the detector was built with %s = %d'
                                       % (proposals_bboxes.shape[1], 'head_rois' if d.head_rois is not None else 'rpn_post_nms_top_n',
                                          d.head_R))
    elif d.head_rois is not None:
        raise InvalidArgumentError(-1, 'get_head: is_training=False on a detector built with head_rois=%d: its head runs on the '
                                       'sampled ROIs only; the eval head needs a detector built without head_rois' % d.head_rois)
    elif using_ohem:
        raise InvalidArgumentError(-1, 'get_head: OHEM belongs to the training branch (is_training=True)')
    if n > d.max_batch:
        raise InvalidArgumentError(-1, 'get_head: ROIs of %d images but the detector was built with max_batch = %d' % (n, d.max_batch))
    view = d.buffer('feat', n)
    if not _same(net_input, view):
        d.write('feat', net_input.numpy() if isinstance(net_input, DeviceTensor) else net_input)
    if d.head_rois is None:
        d.write('proposals', proposals_bboxes.numpy() if isinstance(proposals_bboxes, DeviceTensor) else
                np.asarray(proposals_bboxes, np.float32))
    elif isinstance(proposals_bboxes, DeviceTensor):
        _train.rois_to_head(d, proposals_bboxes, n)
    else:
        d.write('head_rois', np.asarray(proposals_bboxes, np.float32).reshape(n, d.head_R, 4))
    check(lib().xdet_net_get_head(d.handle, n, d.stream.handle))
    _train.heads_ran(d, '_head_step')
    _sync(d)
    if is_training:
        res = loss_func(d.buffer('cls_reg', n), None, int(ohem_roi_one_image) if using_ohem else 0, num_classes)
        return float(res.losses[0])
    cr = d.buffer('cls_reg', n).numpy().reshape(n, d.head_R, -1)
    return cr[..., :num_classes], cr[..., num_classes:num_classes + 4]
