"""xdet: MI355X-native Light-Head R-CNN forward path (host side of libxdet_hip.so).

The names below mirror the interfaces of HiKapok/X-Detector's eval path:
  ps_roi_align            <- op_module.ps_roi_align          (light_head_rfcn_eval.py:143-155)
  ps_roi_align_grad       <- op_module.ps_roi_align_grad     (cpp/PSROIPooling/test_op.py:93-104)
  rotated_ps_roi_align    <- op_module.rotated_ps_roi_align  (cpp/PSROIPooling/rotated_ps_roi_align_op.cc:38-77)
  rotated_ps_roi_align_grad
                          <- op_module.rotated_ps_roi_align_grad
                                                             (cpp/PSROIPooling/test_op.py:150-162)
  XceptionBody, get_rpn, get_proposals, large_sep_kernel, get_head
                          <- net/xception_body.py:236,381,402,450,477
  AnchorCreator, ext_decode_rois
                          <- preprocessing/anchor_manipulator.py:686-757, 671-683
  bboxes_eval             <- light_head_rfcn_eval.py:263-287
  bboxes_matching_batch, GpuStreamingTpFp (xdet.evaluation; LightHeadDetector.evaluate_images / evaluate)
                          <- eval_helper.bboxes_matching_batch, metrics.streaming_tp_fp_arrays
                                                             (light_head_rfcn_eval.py:288-338)
  AnchorEncoder (encode_all_anchors, ext_encode_rois), encode_anchors, encode_rois, host_encode_anchors, host_encode_rois
  (xdet.targets)          <- preprocessing/anchor_manipulator.py:96-445: the training targets, on the GPU and in NumPy
  rpn_loss, head_loss, HeadLoss, host_rpn_loss, host_head_loss, modified_smooth_l1
  (xdet.losses)           <- light_head_rfcn_train.py:257-275, 312-413; net/xception_body.py:502-533, 560: the training
                             losses (RPN sampling, OHEM) and their gradients with respect to the logits
  augment (preprocess_train, host_preprocess_train, draw)
  (xdet.augment)          <- preprocessing/common_preprocessing.py:212-262, 328-381; preprocessing/tf_image.py:322-346,
                             393-630: the training ingest (colour distortion, expand / patch sampling, flip, warp)
  dense_backward, conv_backward, host_dense_backward, host_conv_backward; rpn_backward, head_backward (xdet.model)
  (xdet.ops)              <- what tf.gradients derives for the reference's dense layers and stride-1 'SAME' convs
                             (net/xception_body.py:381-400, 536-557): the RPN head's and the detection head's backward
  batch_norm_forward, batch_norm_backward, host_batch_norm_forward, host_batch_norm_backward;
  large_sep_kernel(..., is_training=True), large_sep_backward (xdet.model; LightHeadDetector(large_sep_train=True))
  (xdet.ops)              <- tf.layers.batch_normalization with training=True and its gradient (net/xception_body.py:
                             450-475): batch statistics, the moving-average updates, the large-separable block's backward
  depthwise_backward, host_depthwise_backward, add_rows_device; exit_flow_train, exit_flow_backward (xdet.model;
  LightHeadDetector(exit_flow_train=True))
  (xdet.ops)              <- what tf.gradients derives for the depthwise half of tf.layers.separable_conv2d, and the
                             Xception exit flow (net/xception_body.py:339-376) with batch statistics and its backward
  middle_flow_train, middle_flow_backward, host_middle_flow_train, host_middle_flow_backward, MIDDLE_FLOW_UNITS,
  MIDDLE_FLOW_VARIABLES (xdet.model; LightHeadDetector(middle_flow_train=True), detector.middle_flow_saved())
                          <- the Xception middle flow (net/xception_body.py:328-337: blocks 5-12, 24 separable units and
                             eight residual adds) with batch statistics and its backward, from `mid_x` down to `entry_x`
  max_pool_backward, host_max_pool_backward, subsample2_device, add_upsample2_device (xdet.ops); entry_flow_train,
  entry_flow_backward, host_entry_flow_train, host_entry_flow_backward, ENTRY_FLOW_UNITS, ENTRY_FLOW_VARIABLES (xdet.model;
  LightHeadDetector(entry_flow_train=True), detector.entry_flow_saved())
                          <- the gradient of max_pooling2d(3, 2, 'same') and blocks 2-4 of the Xception entry flow
                             (net/xception_body.py:260-326) with batch statistics and their backward, from `entry_x` down to
                             the stem's output `stem_out`
  conv_backward_strided, conv_backward_strided_device, host_conv_backward_strided
  (xdet.ops)              <- what tf.gradients derives for a conv at stride 1 or 2, 'VALID' or 'SAME': the two stem convs
                             (net/xception_body.py:243-258), block1_conv1 at stride 2 from the image and block1_conv2
  host_momentum_step, momentum_step_device (xdet.ops); Conv2D.set_kernel_device, DepthwiseConv2D.set_kernel_device;
  MomentumOptimizer, piecewise_learning_rate (xdet.model; the flow backwards' weight_grads='device')
                          <- tf.train.MomentumOptimizer with the L2 term and the learning-rate schedule of
                             light_head_rfcn_train.py:420-436 over the three flows' variables, and the refresh of their
                             forward layers' operands on the device
  host_concat, host_split, concat_device, split_device (xdet.ops); LightHeadDetector.refresh_heads;
  MomentumOptimizer(det, reach='all'), RPN_HEAD_VARIABLES, HEAD_VARIABLES (xdet.model; head_backward, rpn_backward and
  large_sep_backward with weight_grads='device')
                          <- the same optimizer over the large-separable block, the RPN head and the head as well (170
                             variables): the merges the forward layers are built from, and the split of their gradients, as
                             one table-driven copy on the device
  SpectralConv.set_kernel_device (xdet.ops); LightHeadDetector(spectral_refresh=True)
                          <- nothing in the reference: the DFT-domain block matrices of the spectral large-separable convs
                             evaluated from trained kernels on the device, so refresh_eval_net() covers the default form
  host_average_gradients, grad_pack_device, grad_reduce_ranks_device, grad_flat_offsets (xdet.ops);
  Communicator.average_gradients (xdet.dist); MomentumOptimizer.step(grads, lr, comm=...)
                          <- nothing in the reference (its trainer is one session; xdet_v5_resnet_train.py:144 only
                             anticipates replicate_model_fn): data-parallel training, every rank's gradients become the
                             rank-ordered f32 mean, the same bits on every rank, ahead of the step
  stem_train, stem_backward, host_stem_train, host_stem_backward, STEM_VARIABLES, STEM_MOVING, STEM_STAGE, check_stem
  (xdet.model; LightHeadDetector(stem_train=True), detector.stem_saved(), LightHeadDetector.refresh_stem)
                          <- the two stem convs (net/xception_body.py:243-258) with batch statistics and their backward,
                             block1_conv1 from the NCHW image by a kernel of its own (xdet_stem_conv3x3s2_train_forward); with
                             it MomentumOptimizer steps the whole network, 176 variables, and refreshes the eval net's stem
  host_grad_stats, grad_stats_device, momentum_step_device(..., skip=) (xdet.ops); MomentumOptimizer.step(..., guard=, sync=),
  StepPending, TrainStep, StepResult (xdet.model); encode_all_anchors(..., keep_device=True), losses.rpn_loss / HeadLoss
  (..., device_result=True, buffers=)
                          <- the reference's train_op as one call (light_head_rfcn_train.py:420-436, logged scalars
                             :510-516), with nothing in the reference behind the guard: a pass over the gradients that
                             decides on the device whether the momentum step stores anything
  host_clip_scale, host_grad_sq, host_momentum_step(..., scale=), momentum_step_device(..., clip=, scale_out=) (xdet.ops);
  MomentumOptimizer.step(..., clip_norm=), TrainStep(..., comm=, clip_norm=) (xdet.model)
                          <- nothing in the reference (its trainer neither clips nor runs on more than one device): the
                             gradients scaled to a global norm inside the momentum step, from the guard's record, and the
                             one-call step on `world` ranks -- gradients, moving statistics and logged scalars averaged
                             on the streams, the host waiting only in read()
  jpeg_info, host_jpeg_coefficients, host_decode_jpeg, decode_jpegs_device, decode_jpegs (xdet.jpeg);
  LightHeadDetector.detect_jpegs (xdet.model)
                          <- tf.image.decode_image in front of the eval and training pipelines (dataset/dataset_common.py:542)
                             and the demo's demo/test.jpg: baseline JPEG, entropy decoding on the host, IDCT, upsampling and
                             colour conversion on the GPU, written into the packed batch the ingest reads
The training names above that are marked (xdet.model) are written in xdet/train.py (the stages, their state classes, the
backwards and the host statements) and re-exported by xdet/model.py, which holds the eval graph and the detector classes.
The training names marked (xdet.ops) are written in xdet/train_ops.py and re-exported by xdet/ops.py, which holds the eval path.
Importing this package does not load the HIP library; the first op call does and fails
loudly if it is missing (no CPU fallback).
"""
from ._lib import XdetError, InvalidArgumentError, LightHeadConfig, lib      # noqa: F401
from . import weights                                                         # noqa: F401
from . import targets                                                         # noqa: F401
from . import losses                                                          # noqa: F401
from . import augment                                                         # noqa: F401


def __getattr__(name):
    import importlib
    modules = ('ops', 'train_ops', 'model', 'resnet', 'runtime', 'evaluation', 'targets', 'losses', 'jpeg')
    if name in modules:           # `from . import ops` inside the package asks here first: the module itself, and no other
        return importlib.import_module('.' + name, __name__)
    for mod in modules:
        m = importlib.import_module('.' + mod, __name__)
        if hasattr(m, name):
            return getattr(m, name)
    raise AttributeError(name)
