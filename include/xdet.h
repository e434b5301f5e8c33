/*
 * libxdet_hip.so -- C-ABI of the MI355X-native Light-Head R-CNN forward path.
 *
 * Every entry point replaces one interface of HiKapok/X-Detector's eval path
 * (reference file:line cited per function).  Plain pointers and sizes only; all tensor
 * pointers are DEVICE pointers unless the name ends in _host.  Every function returns
 * 0 on success or a negative code (XDET_ERR_*); xdet_last_error() gives the message.
 * Nothing here synchronises the stream unless stated; `stream` is a hipStream_t (NULL =
 * default stream).  The caller owns every buffer; a net handle owns only its weights and
 * a fixed workspace sized at xdet_net_build().
 *
 * Activation layout inside the library is NHWC with the channel count padded to a
 * multiple of 32 ("ld"); the public PsRoiAlign op also accepts the reference's NCHW.
 * Boxes are (ymin, xmin, ymax, xmax) normalised to [0,1]; ROIs to PsRoiAlign (cy,cx,h,w).
 */
#ifndef XDET_H_
#define XDET_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define XDET_OK 0
#define XDET_ERR_INVALID_ARG (-1) /* the op's OP_REQUIRES -> InvalidArgument, ps_roi_align_op.cc:209-226 */
#define XDET_ERR_HIP (-2)         /* HIP failure; reference: fprintf + exit(-1), ps_roi_align_op.cu:150-155 */
#define XDET_ERR_STATE (-3)
#define XDET_ERR_UNSUPPORTED (-4)

const char* xdet_last_error(void);
int xdet_version(void);
int xdet_device_count(int* n);
int xdet_set_device(int dev);
/* "0000:c1:00.0"-style PCI bus id of HIP device `dev` (what identifies a physical GPU across ranks: the launcher
 * binds a rank to the NUMA node of its GPU with it, bench.py gathers it from every rank); buflen >= 16 */
int xdet_device_pci_bus_id(int dev, char* buf, int buflen);
/* hipMalloc + hipIpcGetMemHandle + hipFree on the current device: 0 if this process can export device memory to a
 * peer process (what RCCL's intra-node transport needs), XDET_ERR_HIP otherwise.  Whether it works depends on
 * HSA_ENABLE_IPC_MODE_LEGACY, which the HSA runtime reads when it starts -- so xdet.launch runs this in a fresh
 * probe process before it decides what to export to the ranks. */
int xdet_probe_ipc(void);
/* Arithmetic of the conv / dense contractions for layers and nets created AFTER the call:
 *   0 = f32 MFMA (v_mfma_f32_32x32x2_f32, exact f32 FMA chains; default)
 *   1 = f16x3: operands split into f16 hi+lo parts, three v_mfma_f32_32x32x16_f16 per product
 *       block, f32 accumulate (~2^-21 relative per product: f32-class accuracy on the 2.5 PFLOP/s pipe)
 *   2 = plain f16 operands (speed mode; drifts beyond 1e-3 through the 40-layer stack) */
int xdet_set_default_precision(int mode);
int xdet_get_default_precision(void);

/* ---- memory / streams (what TF's allocator and stream executor did for the op) ---------- */
int xdet_malloc(void** dptr, size_t bytes);
int xdet_free(void* dptr);
int xdet_memset(void* dptr, int value, size_t bytes, void* stream);
int xdet_memcpy_h2d(void* dst, const void* src_host, size_t bytes, void* stream);
int xdet_memcpy_d2h(void* dst_host, const void* src, size_t bytes, void* stream);
int xdet_memcpy_d2d(void* dst, const void* src, size_t bytes, void* stream);
/* xdet_memcpy_d2h synchronises `stream` before it returns; xdet_memcpy_d2h_async only enqueues the copy and returns (dst_host
 * should be pinned, xdet_malloc_host: into pageable memory the runtime may wait all the same); the bytes are there once an
 * event recorded behind it has been waited for (xdet_event_sync). */
int xdet_memcpy_d2h_async(void* dst_host, const void* src, size_t bytes, void* stream);
int xdet_malloc_host(void** hptr, size_t bytes);  /* page-locked host memory (hipHostMalloc), at least 16 bytes */
int xdet_free_host(void* hptr);                    /* NULL: nothing */
int xdet_stream_create(void** stream);
int xdet_stream_destroy(void* stream);
int xdet_stream_sync(void* stream);
/* hipEvent timing on `stream` (bench.py's roofline leg) */
int xdet_event_create(void** ev);
int xdet_event_destroy(void* ev);
int xdet_event_record(void* ev, void* stream);
int xdet_event_elapsed_ms(void* ev_start, void* ev_stop, float* ms); /* syncs on ev_stop */
int xdet_event_sync(void* ev);                     /* the host waits until everything enqueued ahead of the record has run */

/* ---- A9: PsRoiAlign forward --------------------------------------------------------------
 * Replaces op_module.ps_roi_align(inputs, rois, grid_dim_width, grid_dim_height, pool_method)
 * (light_head_rfcn_eval.py:143-155; REGISTER_OP ps_roi_align_op.cc:38-76; CPU functor
 * :81-201; CUDA kernel ps_roi_align_op.cu:36-132).
 *   feat   f32 [N,C,H,W] (feat_layout 0) or [N,H,W,ldc] (feat_layout 1, first C channels used)
 *   rois   f32 [N,R,4] (cy,cx,h,w) -- or corner boxes when rois_are_corners != 0, in which case
 *          _point2center (net/xception_body.py:215-218) is applied on the fly
 *   pooled f32 [N,R,out_ld] (first C = gh*gw*bank entries per ROI, = [N,R,gh*gw,bank] when out_ld == C; the entries
 *          [C, out_ld) of every row are set to 0, in `index` too: a consumer that reads whole rows finds no stale bytes)
 *   index  i32 same shape, may be NULL.  Degenerate ROI: pooled 0 and index 0.
 * Errors: same argument checks as PSROIAlignOp::Compute (:209-226) -> XDET_ERR_INVALID_ARG. */
int xdet_psroialign_fwd(const float* feat, const float* rois, float* pooled, int32_t* index, int N, int C, int H,
                        int W, int R, int grid_w, int grid_h, int use_max, int feat_layout, int ldc, int out_ld,
                        int rois_are_corners, void* stream);

/* ---- F2: PsRoiAlignGrad (training backward of A9) ---------------------------
 * Replaces op_module.ps_roi_align_grad(inputs, rois, pooled_features_grad, pooled_index,
 * grid_dim_width, grid_dim_height, pool_method) (REGISTER_OP ps_roi_align_grad_op.cc:39-57; CUDA
 * kernel ps_roi_align_grad_op.cu:36-171; python gradient registration test_op.py:93-104).
 *   rois         f32 [N,R,4] (cy,cx,h,w)
 *   grad_pooled  f32 [N,R,C]   (= [N,R,gh*gw,bank])
 *   pooled_index i32 [N,R,C]   the forward's argmax sample ids ('max'; may be NULL for 'mean')
 *   grad_feat    f32 [N,C,H,W] (feat_layout 0) or [N,H,W,ldc] (feat_layout 1); zero-filled, then
 *                accumulated with float atomics exactly as the reference does -- summation order is
 *                therefore unspecified and results agree with a sequential evaluation to rounding. */
int xdet_psroialign_grad(const float* rois, const float* grad_pooled, const int32_t* pooled_index, float* grad_feat,
                         int N, int C, int H, int W, int R, int grid_w, int grid_h, int use_max, int feat_layout,
                         int ldc, void* stream);

/* ---- F2 with a fixed summation order (csrc/psroialign_grad_ordered.hip) -------
 * The same gradient as a pure function of its inputs: no float atomics.  Per output element the contributions are added
 * in the order ROI index, sample row i, sample column j, then the corners (iy,ix), (iy1,ix), (iy,ix1), (iy1,ix1), each a
 * separately rounded f32 add -- the order of a sequential evaluation, so the result is bit-identical to one and two calls
 * give the same bits.  (An ROI whose gradient row is all zero may be skipped: at most the sign of a zero differs.)
 *   rois         f32 [N,R,4] (cy,cx,h,w) -- or corner boxes when rois_are_corners != 0 (_point2center on the fly, as
 *                xdet_psroialign_fwd does)
 *   grad_pooled  f32 [N*R, ld_grad], first C entries of a row used (ld_grad >= C)
 *   pooled_index i32 [N*R, ld_index] likewise ('max'; may be NULL for 'mean', which never reads it).  An index outside
 *                [0, n_h*n_w) contributes nothing for that element; no access ever leaves the map.
 *   grad_feat    f32 [N,C,H,W] (feat_layout 0) or [N,H,W,ldc] (feat_layout 1).  EVERY element is written, the padding
 *                channels [C, ldc) as zeros; N*R == 0 gives all zeros.  Nothing needs to be cleared beforehand.
 * One lane owns the H x W plane of one (n, c) in LDS, so H*W is limited: beyond
 * XDET_PSROIALIGN_GRAD_ORDERED_MAX_PIXELS the call returns XDET_ERR_INVALID_ARG (xdet_psroialign_grad takes such maps).
 * Errors -> XDET_ERR_INVALID_ARG before any GPU work: the checks of xdet_psroialign_grad, ld_grad < C, ld_index < C,
 * ldc < C (feat_layout 1), 'max' with a NULL index, H*W above the limit. */
#define XDET_PSROIALIGN_GRAD_ORDERED_MAX_PIXELS 40448 /* (160 KB of LDS - a 2 KB geometry table) / 4 bytes */
int xdet_psroialign_grad_ordered(const float* rois, const float* grad_pooled, int ld_grad, const int32_t* pooled_index,
                                 int ld_index, float* grad_feat, int N, int C, int H, int W, int R, int grid_w, int grid_h,
                                 int use_max, int feat_layout, int ldc, int rois_are_corners, void* stream);

/* ---- RotatedPsRoiAlign forward (oriented boxes; the rotated op of libps_roi_align.so) -----
 * Replaces op_module.rotated_ps_roi_align(inputs, rois, orders, grid_dim_width, grid_dim_height, pool_method)
 * (REGISTER_OP cpp/PSROIPooling/rotated_ps_roi_align_op.cc:38-77; CPU functor :82-301; argument checks
 * :320-343; CUDA kernel rotated_ps_roi_align_op.cu).  The forward is bit-exact against the CPU functor.
 *   feat    f32 [N,C,H,W] (feat_layout 0) or [N,H,W,ldc] (feat_layout 1, first C channels used), C = gh*gw*bank
 *   rois    f32 [N,R,8]: four vertices (y0,x0,y1,x1,y2,x2,y3,x3) in [0,1], clockwise
 *   orders  i32 [N,R]: the first vertex.  order < 0: vertex 0, moved on by one when side0 + side2 > side1 + side3
 *           (squared lengths, :185-203).  order >= 0: vertex (order mod 4) -- a superset of the documented [-1, 4)
 *           (the reference indexes (2*order + k) % 8).
 *   pooled  f32 [N,R,C] (= [N,R,gh*gw,bank]); index i32 same shape, may be NULL ('max': n_w*pool_h + pool_w of the
 *           first maximum; 'mean': 0).  Same element order and channel mapping as xdet_psroialign_fwd.
 * Degenerate quad (a squared side below FLT_MIN; no convexity test -- concave and self-intersecting quads pool like
 * any other): pooled 0 and index 0, both written as the reference does (:205-211).
 * Out-of-bounds samples (superset): where the reference reads outside the plane -- a sample coordinate <= -1, or an
 * integer part >= the map size -- the integer cell is clamped into [0, size-1] (its +1 neighbour clamped to size-1)
 * and the reference's fractional weights are kept.  Everywhere else, including -1 < coordinate < 0 (extrapolation
 * with in-bounds reads), values are the reference's bit for bit.  Sample counts per bin axis are capped at H + W
 * (never reached by a quad inside [0,1]; bounds the work of a NaN / far-out quad).
 * Errors: the op's checks plus grid > 0 and C divisible by gh*gw (the reference divides by zero there) ->
 * XDET_ERR_INVALID_ARG before any GPU work; HIP failures -> XDET_ERR_HIP. */
int xdet_rotated_psroialign_fwd(const float* feat, const float* rois, const int32_t* orders, float* pooled,
                                int32_t* index, int N, int C, int H, int W, int R, int grid_w, int grid_h, int use_max,
                                int feat_layout, int ldc, void* stream);

/* ---- RotatedPsRoiAlignGrad (training backward of the rotated op) ---------------------------
 * Replaces op_module.rotated_ps_roi_align_grad(inputs, rois, orders, pooled_features_grad, pooled_index,
 * grid_dim_width, grid_dim_height, pool_method) (REGISTER_OP rotated_ps_roi_align_grad_op.cc:39-60; CPU functor
 * :221-390; checks :408-436; CUDA scatter rotated_ps_roi_align_grad_op.cu:37-170).
 *   rois, orders as the forward; grad_pooled f32 [N,R,C]; pooled_index i32 [N,R,C] (the forward's; may be NULL for
 *   'mean'); grad_feat f32 [N,C,H,W] (feat_layout 0) or [N,H,W,ldc] (feat_layout 1): zero-filled, then the same
 *   bilinear weights times the upstream gradient accumulated with float atomics ('max': the sample pooled_index
 *   names; 'mean': every sample, grad / (n_h*n_w) as the CUDA kernel scales it).  Summation order is therefore
 *   unspecified; results agree with the reference to rounding.  Geometry and clamping as the forward. */
int xdet_rotated_psroialign_grad(const float* rois, const int32_t* orders, const float* grad_pooled,
                                 const int32_t* pooled_index, float* grad_feat, int N, int C, int H, int W, int R,
                                 int grid_w, int grid_h, int use_max, int feat_layout, int ldc, void* stream);

/* ---- layer objects: the tf.layers.* kernels the graph builders call ---------------------
 * xdet_conv_create: tf.layers.conv2d / dense (+ folded inference BN / bias, + ReLU)
 * (net/xception_body.py:243-265,381-400,450-475,540-558; net/resnet_v2.py:89-100).
 *   kernel_hwio_host f32 [kh,kw,cin,cout]; scale_host/shift_host f32 [cout] (y = conv*scale+shift),
 *   either may be NULL (1 / 0).  pad_mode 0 = VALID, 1 = SAME (TF rule), 2 = explicit pad_t/pad_l.
 * xdet_conv_forward: in NHWC [N,H,W,ld_in] -> out NHWC [N,Ho,Wo,ld_out]; residual (may be NULL)
 *   has the output shape.  ld_in must be round_up(cin,32) (4 when cin <= 4), ld_out = round_up(cout,32).
 *   relu_in applies ReLU to the input on the fly (the `relu -> conv` edges of the graph). */
int xdet_conv_create(void** layer, int kh, int kw, int cin, int cout, int stride, int dilation, int pad_mode,
                     int pad_t, int pad_l, const float* kernel_hwio_host, const float* scale_host,
                     const float* shift_host, int relu_out);
int xdet_conv_forward(void* layer, const float* in, int N, int H, int W, int ld_in, float* out, int ld_out,
                      const float* residual, int relu_in, void* stream);
int xdet_conv_out_shape(void* layer, int H, int W, int* Ho, int* Wo);
/* Fixed split of the reduction (csrc/conv_mfma_ksplit.hip; layers fed with planes only): the K steps are cut into
 * `ksplit` equal ranges and the result is the left fold ((p_0 + p_1) + ...) of the per-range sums -- a constant of the
 * layer, so results do not depend on the batch.  The net builders choose it from the layer geometry (ResNet-50 stages
 * 3-4, net/resnet_v2.py:142-184; the RPN conv / head GEMMs of a single image); this entry sets it on a stand-alone layer.
 * ksplit 0 = back to the plain kernels, 1 = the split-K kernel with one range (bit-identical to the plain kernels).
 * mode 0 = ranges in parallel when tiles * ksplit <= 448 else one workgroup per tile, 1 / 2 = force either (the two are
 * bit-identical); max_parallel_tiles sizes the scratch slabs of the parallel mode. */
int xdet_conv_set_ksplit(void* layer, int ksplit, int mode, int max_parallel_tiles);
/* Split-precision operand planes (modes 1/2): x = hi + lo, both f16, blocked
 * [ceil(n_pix/16)][ld/32][16][32] with n_pix = N*H*W (16 pixels x 32 channels = one contiguous 1 KB
 * block: what one LDS-DMA instruction of a conv tile ingests); a plane holds ceil(n_pix/16)*16*ld halves.  xdet_split_f32 (x NHWC [n_pix][ld], ld % 32 == 0) writes them element-wise (optionally through a ReLU); xdet_conv_forward_planes runs a
 * layer whose A operand already lives as planes (LDS-DMA kernel, no register staging).  Inside a
 * net the depthwise kernels and split passes produce the planes; these two entry points expose the
 * same kernels for tests. */
int xdet_split_f32(const float* in, uint16_t* hi, uint16_t* lo, int64_t n_pix, int ld, int relu, void* stream);
int xdet_conv_forward_planes(void* layer, const uint16_t* in_hi, const uint16_t* in_lo, int N, int H, int W,
                             int ld_in, float* out, int ld_out, const float* residual, void* stream);
/* The "x8" form of the planes for a pointwise (1x1, stride 1) layer of mode 1 (csrc/conv_params.h): the two cross terms of the
 * split-precision product, a_hi*w_lo + a_lo*w_hi (2^-11 of the result), are computed from fp8 (e4m3, OCP) copies of the
 * operands by one block-scaled MFMA per 32 input channels instead of four f16 MFMAs (the GEMM is 21-26 % faster, one
 * contraction accurate to ~1e-5 instead of ~5e-7 relative: profiles/NOTES_r04.md).  `lo8` has the size and blocking of a
 * `lo` plane; per (pixel, 32-channel block) it holds 32 bytes fp8(hi * 2^-x8_exp) followed by 32 bytes
 * fp8(lo * 2^(11 - x8_exp)).  x8_exp: a power-of-two scale of the tensor such that its largest magnitude * 2^-x8_exp lands in
 * (128, 256] (values beyond 448 * 2^x8_exp saturate in the fp8 copies only).  Inside a net (option "cross" = "fp8") the
 * depthwise kernels write this form and the calibration pass chooses the exponents; these two entries expose the kernels for
 * tests. */
int xdet_split_f32_x8(const float* in, uint16_t* hi, uint16_t* lo8, int64_t n_pix, int ld, int relu, int x8_exp, void* stream);
int xdet_conv_forward_planes_x8(void* layer, const uint16_t* in_hi, const uint16_t* in_lo8, int N, int H, int W, int ld_in,
                                float* out, int ld_out, const float* residual, int x8_exp, void* stream);
/* One conv layer with everything its epilogue can write (csrc/conv_epilogue.h), as Plan::add_conv asks for it inside a net:
 * the f32 output and / or a second copy of it as split planes (xdet_split_f32 layout) for the next layer's LDS-DMA operand.
 * The same ConvLayer::forward as the nets: kernel family and tile follow from the shapes and xdet_conv_set_ksplit.
 *   input    either `in` (f32 NHWC, with relu_in) or `in_hi` / `in_lo` planes (x8 != 0: the x8 form with x8_exp), the other NULL
 *   out      f32 NHWC [N][Ho][Wo][ld_out], or NULL: planes only
 *   out_hi / out_lo   both or neither: planes of relu?(out * s + h), hi = f16(t), lo = f16(t - hi);
 *            ceil(N*Ho*Wo/16)*16 * max(planes_ld, ld_out) halves each.  Channels [cout, ld_out) are +0; the pad rows beyond N*Ho*Wo
 *            are not written.
 *   planes_ld   channel stride of the planes destination: 0 or ld_out = the layer's own planes tensor; a larger multiple of 32 =
 *            a wider (concatenated) operand of which this conv fills blocks [0, ld_out/32) of every 16-pixel group
 *   planes_relu   the planes hold max(., 0) (NaN stays NaN, unlike xdet_split_f32's ReLU-on-load)
 *   bn_scale / bn_shift   host [cout] or NULL: a following inference BN folded into the planes copy, s = bn_scale * 2^-out_exp,
 *            h = bn_shift * 2^-out_exp; implies planes_relu.  Without one s = 2^-out_exp, h = 0 (out_exp = 0: no affine at all).
 *            They REPLACE the layer's planes affine and out_exp and stay set until the next call, so the door is for layers
 *            created with xdet_conv_create, not for a layer that belongs to a net: there it would overwrite the exponent the
 *            calibration chose, without a word.
 * XDET_ERR_INVALID_ARG (never a fall-back) for: planes from a layer created in the f32 mode; no output at all; one plane of the
 * two; planes_ld not a multiple of 32 or below ld_out; a wider destination together with a BN.  A door for tests: the nets
 * reach the same code through their plans. */
int xdet_conv_forward_emit(void* layer, const float* in, const uint16_t* in_hi, const uint16_t* in_lo, int x8, int x8_exp, int relu_in,
                           int N, int H, int W, int ld_in, float* out, int ld_out, const float* residual, uint16_t* out_hi,
                           uint16_t* out_lo, int planes_ld, int planes_relu, const float* bn_scale_host, const float* bn_shift_host,
                           int out_exp, void* stream);
int xdet_layer_destroy(void* layer);
/* depthwise 3x3 SAME stride 1 (the depthwise half of tf.layers.separable_conv2d,
 * net/xception_body.py:224-231); dw_kernel_host f32 [3,3,C,1]; in/out NHWC with stride ld. */
int xdet_depthwise_create(void** layer, int C, int dilation, const float* dw_kernel_host);
int xdet_depthwise_forward(void* layer, const float* in, int N, int H, int W, int ld, float* out, int relu_in,
                           void* stream);
/* relu_separable_bn_block as ONE kernel (net/xception_body.py:220-234: (ReLU ->) depthwise 3x3 -> pointwise 1x1 ->
 * BN, "nothing in between"): the depthwise result stays on the CU instead of crossing HBM as split planes.
 * dw_layer from xdet_depthwise_create (dilation 1), pw_layer a 1x1 stride-1 layer from xdet_conv_create in a
 * split-precision mode (its scale/shift = the folded BN, relu_out as created); <= 256 input channels
 * (multiple of 32) and 128 or 256 outputs; in/out NHWC f32.  Bit-identical to xdet_depthwise_forward ->
 * xdet_split_f32 -> xdet_conv_forward_planes.  Inside a net the entry-flow blocks use it
 * (option "sepconv" = "fused" (default) | "split"). */
int xdet_sepconv_fused_forward(void* dw_layer, void* pw_layer, const float* in, int N, int H, int W, int ld_in, float* out,
                               int ld_out, int relu_in, void* stream);
/* tf.layers.conv2d(3x3, VALID, stride 1, use_bias=False) -> BN (-> ReLU) over 32 input channels and <= 64 outputs
 * (block1_conv2, net/xception_body.py:252-259) with the input tile staged ONCE in LDS: in_hi/in_lo are the split
 * planes of xdet_split_f32 (ld 32), `layer` a matching xdet_conv_create layer in a split-precision mode; out is
 * NHWC f32 [N][H-2][W-2][ld_out].  Bit-identical to xdet_conv_forward_planes on the same layer.  Inside a net:
 * option "conv3x3" = "patch" (default) | "gemm". */
int xdet_conv3x3_patch_forward(void* layer, const uint16_t* in_hi, const uint16_t* in_lo, int N, int H, int W, float* out,
                               int ld_out, void* stream);
/* One ResNet v2 bottleneck block with an identity shortcut (net/resnet_v2.py:142-184 with projection_shortcut = None,
 * strides = 1: shortcut = inputs; BN-ReLU -> conv 1x1 -> BN-ReLU -> conv 3x3 -> BN-ReLU -> conv 1x1; + shortcut) as ONE
 * kernel (csrc/resnet_bneck.hip): the block input is read once per use, the pre-activation and the two narrow
 * intermediates never leave the CU.  conv_a / conv_b / conv_c: layers from xdet_conv_create in mode 1 -- 1x1 Cin -> Cmid
 * with the folded BN that follows it and relu 1; 3x3 SAME stride 1 Cmid -> Cmid likewise; 1x1 Cmid -> Cin, relu 0
 * (Cin 256, Cmid 64: stage 1 of ResNet-50).  x: the block input, NHWC f32 [N][H][W][Cin]; pre_scale / pre_shift
 * (device, [Cin]): the block's first BN folded, i.e. the pre-activation is relu(x * pre_scale + pre_shift) (one fused
 * multiply-add per element, then hi = f16(.), lo = f16(. - hi): what xdet_split_f32 makes of that tensor);
 * out = x + branch.  With out_hi / out_lo given, relu(out * next_scale + next_shift) -- the NEXT block's pre-activation --
 * is also written as planes (xdet_split_f32 layout) for a successor that runs layer by layer.  Bit-identical to
 * xdet_split_f32 + three xdet_conv_forward_planes calls.  Inside xdet_resnet_*: the identity blocks of stage 1
 * (xdet_resnet_set_option "bneck" = "off": three launches per block). */
int xdet_resnet_bneck_forward(void* conv_a, void* conv_b, void* conv_c, const float* pre_scale, const float* pre_shift,
                              const float* x, int N, int H, int W, float* out, const float* next_scale,
                              const float* next_shift, uint16_t* out_hi, uint16_t* out_lo, void* stream);
/* A (taps,1) [axis 0] or (1,taps) [axis 1] SAME convolution in the DFT domain of the convolved axis (csrc/spectral.hip;
 * the large-separable convs, net/xception_body.py:450-475): forward DFT of every line of the F x F map -> one real GEMM
 * [N*F, 2 Cin] x [2 Cin, 2 Cout] per frequency bin (grouped split-precision GEMM; L/2 bins of the shortest even transform
 * without wrap-around into the F outputs, L >= F + 7: 12 / 19 / 29 bins, which the workspace scales with) -> inverse DFT with
 * out = relu?(y * scale + shift).  kernel_host f32 [taps][cin][cout] (taps odd, <= 15); scale_host / shift_host [cout] or NULL;
 * F must be 16, 30 or 50 and the layer must be created in a split-precision mode (anything else: XDET_ERR_INVALID_ARG, nothing
 * is launched).  in: NHWC f32 [N][F][F][ld_in], ld_in = round_up(cin, 32); out: NHWC f32 [N][F][F][ld_out], ld_out a multiple
 * of 4 and >= round_up(cout, 32) (channels [0, round_up(cout, 32)) are written).  workspace: device memory of
 * xdet_spectral_conv_workspace_bytes(layer, N) bytes, 256-byte aligned, any contents (every row that is read back is written
 * first).  An image's result does not depend on the batch it arrives in: how the launchers deal bins and output positions to
 * workgroups changes with N, the arithmetic per element does not.  Inside a net: option "large_sep" = "spectral" | "auto".
 * Destroy with xdet_layer_destroy. */
int xdet_spectral_conv_create(void** layer, const float* kernel_host, int taps, int cin, int cout, int axis, int F,
                              const float* scale_host, const float* shift_host, int relu_out);
size_t xdet_spectral_conv_workspace_bytes(void* layer, int N);
int xdet_spectral_conv_forward(void* layer, const float* in, int N, int ld_in, void* workspace, float* out, int ld_out,
                               void* stream);
/* block1_conv1 of the Xception entry (net/xception_body.py:243-250): 3x3 / stride 2 / VALID, 3 -> 32 channels, folded BN +
 * ReLU, from the NCHW input [N][3][S][S] straight to split planes (xdet_split_f32 layout, ld 32) of the
 * [N][Ho][Ho][32] output, Ho = (S - 3) / 2 + 1.  w27x32 (device): [ky][kx][ci][32]; scale / shift (device): [32].  The planes
 * hold ceil(N*Ho*Ho / 16) * 16 * 32 halves each; pixels past N*Ho*Ho of the last group are not written. */
int xdet_stem_conv3x3s2_forward(const float* in_nchw, const float* w27x32, const float* scale, const float* shift,
                                uint16_t* out_hi, uint16_t* out_lo, int N, int S, void* stream);
/* block1_conv1 in training mode (csrc/stem_train.hip): the same geometry from the same NCHW input, but the raw f32 conv output
 * z [N][Ho][Ho][ld_z] (channels 32 .. ld_z - 1 of a pixel are not written) that the training-mode batch norm takes its
 * statistics from -- no BN, no ReLU, no split.  w (device): [3][3][3][32], the checkpoint's own layout, read in place: an
 * optimizer's master needs no repack.  Arithmetic: per output element one f32 accumulator from 0, the 27 products added by
 * fmaf in (ky, kx, ci) order, which is xdet_stem_conv3x3s2_forward's accumulation in front of its scale and shift.  With an
 * even S the image's last row and column lie under no window and are never read.  An image's result does not depend on the
 * batch it arrives in.  XDET_ERR_INVALID_ARG ahead of any launch: a NULL argument, N < 1, S < 3, ld_z < 32, N * S * S >= 2^31. */
int xdet_stem_conv3x3s2_train_forward(const float* in_nchw, const float* w, int N, int S, float* z, int ld_z, void* stream);
/* conv2d_fixed_padding(7 x 7, 64 filters, stride 2) of the ResNet v2 stem (net/resnet_v2.py:311-320) from the NCHW input
 * [N][3][S][S] with the input patch staged in LDS (csrc/resnet_stem.hip).  `layer`: xdet_conv_create(7, 7, 3, 64, stride 2,
 * pad_mode 2, pad 3 / 3) in mode 1 (f16x3); its scale / shift are applied, its relu_out must be 0.  out: NHWC f32
 * [N][Ho][Ho][64], Ho = (S - 1) / 2 + 1.  Bit-identical to xdet_nchw_to_nhwc4 + xdet_conv_forward on the same layer. */
int xdet_resnet_stem7x7_forward(void* layer, const float* in_nchw, int N, int S, float* out, void* stream);
/* initial_max_pool (3 x 3, stride 2, SAME; net/resnet_v2.py:311-330) + the first block's batch_norm_relu (:142-156) in one pass:
 * in NHWC f32 [N][H][W][ld] (ld % 32 == 0) -> split planes (xdet_split_f32 layout, ld) of relu(pool(in) * scale + shift) * mul
 * over the [N][(H+1)/2][(W+1)/2] pixels; scale / shift (device): [ld].  out_hi2 / out_lo2 (optional, both or neither): a second
 * copy scaled by mul2 into the channel blocks of a wider planes tensor [pix/16][c32_2][16][32], c32_2 >= ld / 32 -- the
 * pointers address this tensor's first channel block in it; its other blocks are not touched. */
int xdet_maxpool3x3s2_bn_planes(const float* in, const float* scale, const float* shift, uint16_t* out_hi, uint16_t* out_lo,
                                int N, int H, int W, int C, int ld, float mul, uint16_t* out_hi2, uint16_t* out_lo2,
                                int c32_2, float mul2, void* stream);
/* The opening 1x1 conv of a ResNet v2 bottleneck with the pre-activation made on the CU (csrc/resnet_preconv.hip;
 * net/resnet_v2.py:142-166): planes of relu(bn_b(conv1x1(relu(x * pre_scale + pre_shift)))).  `layer`: a 1x1 stride-1 layer
 * from xdet_conv_create in mode 1 with the folded bn_b and relu_out 1, Cin 256 or 512 -> 128 outputs (stage 2 of ResNet-50;
 * anything else: XDET_ERR_INVALID_ARG).  x: NHWC f32 [N][H][W][Cin]; pre_scale / pre_shift (device): [Cin]; out planes in the
 * xdet_split_f32 layout, ld 128.  Bit-identical to xdet_split_f32 of relu(x * pre_scale + pre_shift) + xdet_conv_forward_planes
 * + xdet_split_f32 of its output. */
int xdet_resnet_preconv_forward(void* layer, const float* pre_scale, const float* pre_shift, const float* x, int N, int H,
                                int W, uint16_t* out_hi, uint16_t* out_lo, void* stream);
/* The entry-flow tail "separable block -> max_pooling2d(3, 2, 'same') -> tf.add(residual)" (net/xception_body.py:268-286)
 * with the pool split between the two kernels: xdet_sepconv_fused_hpool_forward is xdet_sepconv_fused_forward whose
 * epilogue writes the 3-column / stride-2 maximum of every output row (out_hpooled: NHWC f32 [N][H][(W+1)/2][ld_out]),
 * xdet_maxpool_v3s2_add the 3-row / stride-2 maximum of that (+ residual) -> [N][(H+1)/2][(W+1)/2][ld].  Together
 * bit-identical to xdet_sepconv_fused_forward -> xdet_maxpool3x3s2_add; the full-resolution tensor crosses HBM at half
 * size.  Inside a net: option "pool" = "split" (default: the 237 x 237 block) | "whole" | "split_all". */
int xdet_sepconv_fused_hpool_forward(void* dw_layer, void* pw_layer, const float* in, int N, int H, int W, int ld_in,
                                     float* out_hpooled, int ld_out, int relu_in, void* stream);
int xdet_maxpool_v3s2_add(const float* in_hpooled, const float* residual, float* out, int N, int H, int Wo, int C, int ld,
                          void* stream);
/* tf.layers.max_pooling2d(3,2,'same') + tf.add(residual) (net/xception_body.py:281-286) */
int xdet_maxpool3x3s2_add(const float* in, const float* residual, float* out, int N, int H, int W, int C, int ld,
                          void* stream);
int xdet_nchw_to_nhwc4(const float* in_nchw, float* out_nhwc4, int N, int C, int H, int W, void* stream);
/* F1: light_head_preprocess_for_eval / _for_test (preprocessing/common_preprocessing.py:383-458), fused:
 * uint8 [H,W,3] (device) -> whitened f32, TF-legacy bilinear warp to out_size x out_size, CHW
 * (one image of the [N,3,S,S] network input); bbox_img is the constant [0,0,1,1]. */
int xdet_preprocess_eval(const uint8_t* image_hwc, int H, int W, float* out_chw, int out_size, void* stream);
/* F1, ragged batch: light_head_preprocess_for_eval with its `resize` argument (common_preprocessing.py:383-440) for N
 * images in one launch.  packed: the uint8 HWC images back to back (packed_bytes in all); offsets i64 [N]: byte offset
 * of image n; image_shapes i32 [N][2]: its original (H, W) -- the buffer xdet_net_forward reads as image_shapes.  All
 * three are device memory and are read by the kernel, never taken as launch arguments, so a captured graph serves any
 * mix of sizes.  -> out_nchw f32 [N,3,S,S] (S = out_size), bbox_img f32 [N,4] (16-byte aligned).
 * Values of `resize` = the reference's IntEnum Resize (common_preprocessing.py:29-32):
 *   WARP_RESIZE     TF-legacy bilinear warp to S x S (:435-439), bit-identical to xdet_preprocess_eval.
 *   PAD_AND_RESIZE  factor = min(1, S/H, S/W) in f64, (rh, rw) = floor(factor * (H, W)) (:405-410), warp to rh x rw, then
 *                   centred zero pad (zeros in whitened space: whitening comes first, :392-393).
 *   CENTRAL_CROP    no resize: per axis crop max((H-S)//2, 0), pad max((S-H)//2, 0) (tf_image.py:207-305).
 *   NONE            whitening only; H = W = S required (:400-402).
 * bbox_img: [0,0,1,1] through bboxes_crop_or_pad (tf_image.py:179-203) for the crop and then the pad step, each in f32 as
 * b*[h,w,h,w] + offset, / [th,tw,th,tw]; WARP and NONE give [0,0,1,1].  An invalid descriptor (H or W <= 0, an image
 * that does not lie inside packed, rh or rw = 0, NONE with a size other than S x S) reads nothing: its planes and its
 * bbox_img are NaN, and xdet_bboxes_eval reports a NaN bbox_img as NaN scores for that image only. */
enum { XDET_RESIZE_NONE = 1, XDET_RESIZE_CENTRAL_CROP = 2, XDET_RESIZE_PAD_AND_RESIZE = 3, XDET_RESIZE_WARP = 4 };
int xdet_preprocess_eval_batch(const uint8_t* packed, int64_t packed_bytes, const int64_t* offsets,
                               const int32_t* image_shapes, int N, int out_size, int resize, float* out_nchw,
                               float* bbox_img, void* stream);
/* ---- JPEG decode: the step in front of the ingest (the reference reads encoded JPEGs: dataset/dataset_common.py:542,
 * tf.image.decode_image; demo/test.jpg).  Entropy decoding on the host, pixels on the GPU, written straight into the
 * packed layout above.  The statement every stage equals bit for bit is xdet/jpeg.py (jpeg_info, host_jpeg_coefficients,
 * host_decode_jpeg); the yardstick of that statement is libjpeg's default decode (Pillow / libjpeg-turbo: ISLOW IDCT,
 * fancy upsampling where libjpeg applies it), equal byte for byte on the committed fixtures and on a sweep of every size
 * 1 .. 19 x 1 .. 11 in all three samplings.
 *
 * Accepted: baseline sequential DCT (SOF0), 8-bit samples, Huffman coding, ONE interleaved scan, 8-bit quantisation
 * tables; one component (grayscale, written R = G = B) or three (YCbCr) with luma sampling (1,1), (2,1) or (2,2) and
 * chroma (1,1), i.e. 4:4:4, 4:2:2, 4:2:0; DRI with RST0-7, byte stuffing (FF 00), fill FF bytes in front of markers; up to
 * four tables per class; APPn / COM skipped; height and width in 1 .. 8192.  A stream is complete once every MCU has been
 * decoded: what follows the last MCU (EOI included) is ignored.
 * Refused with XDET_ERR_INVALID_ARG, each by its own message, before anything is written:
 *   "progressive JPEG (SOF2) is not supported", "extended sequential JPEG (SOF1) ...", "lossless or hierarchical JPEG
 *   (SOFn) ...", "arithmetic coding (SOFn / DAC) ..."; "N-bit samples are not supported (8-bit only)"; "16-bit quantisation
 *   tables are not supported"; "N components are not supported (1 or 3)"; "sampling factors HxV of component i are not
 *   supported (4:4:4, 4:2:2, 4:2:0 only)"; "non-interleaved or multiple scans are not supported"; "spectral selection or
 *   successive approximation in a baseline scan"; "an Adobe APP14 marker with transform 0 (RGB data) is not supported" and
 *   "components named R, G, B (RGB data) ..." (both without a JFIF marker, as libjpeg decides); "height 0 (DNL) is not
 *   supported", "DNL marker is not supported", "width 0", "images beyond 8192 x 8192 ..."; "missing quantisation table t",
 *   "missing DC / AC Huffman table t"; "bad Huffman table" (a code that does not fit its length); "undefined Huffman code";
 *   "truncated data" (any read past the end of the data, in the markers or in the entropy-coded bits: a bit behind the
 *   last data byte of a restart interval is never invented); "restart marker missing or out of sequence"; "coefficient
 *   index past 63"; "DC difference category past 11"; "not a JPEG (no SOI marker)", "a marker is expected", "a second SOI
 *   marker", "no scan (EOI in front of SOS)", "more than one frame header (SOF)", "a scan without a frame header",
 *   "malformed <name> segment".
 *
 * The arithmetic (int32, two's complement: products and sums wrap, >> is arithmetic; nothing wraps on a valid image):
 *   entropy   DC = running sum of the differences per component and restart interval, kept as int16 (wrapping); AC values
 *             at their natural (de-zigzagged) index; a ZRL that runs past 63 ends the block, a coefficient past 63 refuses.
 *   IDCT      x = coef * q; jidctint.c with CONST_BITS 13, PASS1_BITS 2: even part z1 = (x2+x6)*4433, t2 = z1 - x6*15137,
 *             t3 = z1 + x2*6270, t0 = (x0+x4)<<13, t1 = (x0-x4)<<13; odd part on (x7,x5,x3,x1) with z5 = (z3+z4)*9633 and
 *             the constants 2446, 16819, 25172, 12299, -7373, -20995, -16069, -3196.  Pass 1 over columns, (v + 1024) >> 11;
 *             pass 2 over rows, (v + (1<<17)) >> 18; range limit y = (v + 128) & 1023: y < 256 -> y, y < 640 -> 255, else 0.
 *   chroma    on the component's true size cw x ch = ceil(W/hs) x ceil(H/vs), never the block padding.  With more than two
 *             chroma columns (cw > 2) libjpeg's fancy upsampling, the edge row / column replicated:
 *             4:2:0: s = 3*p[r] + p[r-1] for output row 2r, 3*p[r] + p[r+1] for row 2r+1; out[2c] = (3*s[c] + s[c-1] + 8) >> 4,
 *             out[2c+1] = (3*s[c] + s[c+1] + 7) >> 4.  4:2:2: out[2c] = (3*p[c] + p[c-1] + 1) >> 2, out[2c+1] = (3*p[c] +
 *             p[c+1] + 2) >> 2, the first and the last column of the 2*cw-wide row the input's own values.
 *             With one or two chroma columns (cw <= 2, i.e. W <= 4) libjpeg does not filter (jdsample.c takes the fancy
 *             routines only for downsampled_width > 2): plain replication in both directions, out[y][x] = p[y / vs][x / 2].
 *   colour    cb, cr centred at 0: R = Y + ((91881*cr + 32768) >> 16), B = Y + ((116130*cb + 32768) >> 16),
 *             G = Y + ((-22554*cb - 46802*cr + 32768) >> 16), each clamped to 0 .. 255.
 *
 * xdet_jpeg_desc: what the marker parser knows of an image.  blocks_x / blocks_y: a component's block grid padded to whole
 * MCUs; coef_offset[c]: the index of component c's first block in the image's coefficient buffer (component-major, then
 * rows of blocks); quant[c]: its quantisation table in natural order. */
typedef struct xdet_jpeg_desc {
  int32_t height, width, components, h_samp, v_samp, restart_interval, mcus_x, mcus_y;
  int32_t blocks_x[3], blocks_y[3];
  int64_t coef_offset[3];
  int64_t total_blocks;
  uint16_t quant[3][64];
} xdet_jpeg_desc;
/* the markers up to SOS -> *desc.  Host only: no device is touched. */
int xdet_jpeg_info(const uint8_t* data_host, int64_t length, xdet_jpeg_desc* desc);
/* the entropy stage of one image.  Host only, usable without a GPU.  coefficients_host: int16 [capacity_blocks][64];
 * block b of the image (desc->coef_offset, above) in natural order, NOT dequantised.  Every block of the padded grids is
 * written; on a refusal the buffer's contents are undefined. */
int xdet_jpeg_entropy_decode(const uint8_t* data_host, int64_t length, int16_t* coefficients_host, int64_t capacity_blocks,
                             xdet_jpeg_desc* desc);
/* bytes of the workspace xdet_jpeg_decode_batch needs for N images, from their descriptors (xdet_jpeg_info's, nothing is
 * parsed again): coefficients, the block table, tables and descriptors, the uint8 component planes.  0 = a refusal. */
size_t xdet_jpeg_decode_workspace_bytes(const xdet_jpeg_desc* descs, int N);
/* N (1 .. 65535) encoded images and their descriptors (descs[n] as xdet_jpeg_info wrote it for datas_host[n]) -> packed:
 * the decoded uint8 HWC images back to back, image n at offsets[n] = 3 * sum of H*W of the images before it; offsets
 * i64 [N] and image_shapes i32 [N][2] (device, either may be NULL) are written too -- the three buffers
 * xdet_preprocess_eval_batch, xdet_preprocess_train_batch and xdet_net_forward_u8 read.
 * Sizes and offsets come from the descriptors; each image is parsed once more, by the thread that decodes it (the Huffman
 * tables live there), and a descriptor that is not the one its image gives is refused like a bad stream.  The entropy
 * streams are decoded on at most `threads` host threads (clamped to 1 .. 16 and to N; never sized from the machine), one
 * image per thread at a time, into pinned staging that the library owns: one buffer per device (the device current at the
 * call, which must be `stream`'s), grown on demand and kept at its high-water mark until the process ends (the front of
 * the workspace: 136 bytes per block, up to about 4.5 GB at the 2^31-byte plane limit), reused from call to call (calls on
 * one device are serialised on it; a call waits for the copy of the call before).  Then one host-to-device copy, and
 * jpeg_idct_kernel (all blocks of the batch, one launch) and jpeg_color_kernel on `stream`; the call does not wait for
 * them.  Every refusal -- as "images[n]: <message>" with the lowest such n -- comes before the first copy: a batch decodes
 * whole or not at all.  Bytes of packed outside the images are not written.
 * workspace: 256-byte aligned, at least xdet_jpeg_decode_workspace_bytes, and alive until the kernels have run.  The host
 * work makes the call unfit for stream capture; the kernels it enqueues precede a captured forward on the same stream. */
int xdet_jpeg_decode_batch(const uint8_t* const* datas_host, const int64_t* lengths, const xdet_jpeg_desc* descs, int N,
                           int threads, uint8_t* packed, int64_t packed_bytes, int64_t* offsets, int32_t* image_shapes,
                           void* workspace, size_t workspace_bytes, void* stream);
/* Training ingest: light_head_preprocess_for_train (preprocessing/common_preprocessing.py:328-381) for N decoded images
 * of any sizes and their ground truth, in one call: random colour distortion (distort_color, fast_mode=False, :212-262),
 * SSD expand and patch sampling (tf_image.py:602-630, 547-571, 393-545), random horizontal flip (tf_image.py:322-346),
 * TF-legacy bilinear warp to S x S (as above), * 2 - [R,G,B mean]/127.5, CHW.  packed / offsets / image_shapes as in
 * xdet_preprocess_eval_batch; glabels i32 [N,G], gbboxes f32 [N,G,4] (ymin, xmin, ymax, xmax in [0,1]), n_gt i32 [N]
 * (clamped to [0,G]); image_ids i32 [N] or NULL (then 0 .. N-1).  All of them device memory, read by the kernels.
 * -> out_nchw f32 [N,3,S,S]; out_glabels / out_gbboxes / out_n_gt in the same layout, boxes in the frame of the network
 * input, in input order, zeros behind out_n_gt -- what xdet_encode_anchors reads.  The statement the kernels are equal to,
 * bit for bit, is xdet/augment.py host_preprocess_train; its module docstring gives every step.  In short:
 *   draws     draw(seed, image_id, k) = mix(word ^ (0x80000000 | k)), word = mix(mix(seed ^ 0x9E3779B9) + image_id), mix the
 *             32-bit finaliser of the shuffle keys below; bit 31 is the stream no shuffle uses.  k counts the draws of one
 *             image in the reference's program order.  float in [lo,hi): lo + ((u >> 8) * 2^-24) * (hi - lo); int in
 *             [lo,hi): lo + u % (hi - lo), lo for an empty range (TF raises); the 7-way multinomial: u % 7.
 *   contrast  the mean is taken over the whole source image after the ops in front of contrast in the drawn ordering and
 *             is DEFINED as f32(sum over pixels of int64(rint(v * 65536)) / (H * W * 65536)): an exact integer sum and one
 *             f64 division, independent of reduction order, grid and batch.
 *   patches   the reference's loops with their bounds (3 attempts x 50 x 20 x 10 rounds); the `no box kept` term of
 *             check_roi_overlap, unbounded in the reference, is bounded by the 50 as well.
 * records (may be NULL): one 128-byte record per image, 32 little-endian words:
 *   0 valid | 1-2 canvas h, w | 3-4 offset y, x of the image in the canvas | 5-8 crop y, x, h, w | 9 flip | 10 colour
 *   ordering | 11-14 f32 brightness delta, saturation factor, hue delta, contrast factor | 15-17 f32 contrast means |
 *   18 attempts used | 19 fallback to the originals | 20 draws consumed | 21 last attempt expanded | 22 last attempt's
 *   min_iou index | 23 a patch below one pixel was met | 24 mask of min_iou indices drawn | 25 mask of attempts that
 *   expanded | 26 boxes read | 27 boxes written | 28-31 zero.
 * An invalid descriptor (H or W <= 0, an image that does not lie inside packed) reads nothing: NaN planes for that image
 * only, out_n_gt = 0, a zero record.  workspace: xdet_preprocess_train_workspace_bytes(N, G) bytes, 16-byte aligned.
 * N <= 0, G <= 0, G > 512, out_size <= 0, packed_bytes < 0 or a NULL required pointer: XDET_ERR_INVALID_ARG before any
 * GPU work. */
size_t xdet_preprocess_train_workspace_bytes(int N, int G);
int xdet_preprocess_train_batch(const uint8_t* packed, int64_t packed_bytes, const int64_t* offsets,
                                const int32_t* image_shapes, const int32_t* glabels, const float* gbboxes,
                                const int32_t* n_gt, const int32_t* image_ids /* may be NULL: 0..N-1 */, int N, int G,
                                int out_size, uint32_t seed, float* out_nchw, int32_t* out_glabels, float* out_gbboxes,
                                int32_t* out_n_gt, void* records /* may be NULL */, void* workspace, void* stream);

/* ---- A4+A6: RPN glue + AnchorEncoder.decode_all_anchors ----------------------------------
 * (light_head_rfcn_eval.py:389-397; preprocessing/anchor_manipulator.py:641-669,698-757)
 *   rpn_out NHWC [N,Hh,Ww,ld]: cls logits at channels [cls_off, cls_off+2A), box deltas at
 *   [box_off, box_off+4A); anchors_yx [Hh*Ww,2] centres, anchors_hw [A,2] sizes.
 *   -> objectness [N,Hh*Ww*A], boxes [N,Hh*Ww*A,4] */
int xdet_rpn_decode(const float* rpn_out, int ld, int cls_off, int box_off, int N, int Hh, int Ww, int A,
                    const float* anchors_yx, const float* anchors_hw, float* objectness, float* boxes, void* stream);

/* ---- A7: get_proposals (net/xception_body.py:402-448) ------------------------------------
 *   objectness [N,n_anchor], boxes [N,n_anchor,4] -> rois [N,post_n,4]; workspace from
 *   xdet_proposals_workspace_bytes().  counts_out (may be NULL) i32 [N,4] device:
 *   {n_valid, n_candidates, n_kept_by_nms, 0}.  nms_thr >= 0; post_n <= 6144 (the kept list lives in LDS).
 *   The NMS is tf.image.non_max_suppression's greedy walk (visit in score order, IoU > thr against boxes kept before,
 *   stop at post_n) computed in panels of 256 / 512 candidates; with N <= 64 an image's panels are spread over a cluster
 *   of up to 16 workgroups that wait for each other inside the kernel (every per-call control word is cleared by the
 *   call itself; a cluster whose members never meet -- it cannot happen on an otherwise working GPU -- gives up after
 *   ~1 s and marks its image, whose detection scores then come out NaN through xdet_net_forward). */
size_t xdet_proposals_workspace_bytes(int N, int n_anchor, int pre_n, int post_n);
int xdet_get_proposals(const float* objectness, const float* boxes, int N, int n_anchor, int pre_n, int post_n,
                       float nms_thr, float min_size, void* workspace, float* rois, int* counts_out, void* stream);

/* ---- A11: AnchorEncoder.ext_decode_rois (anchor_manipulator.py:671-683) ------------------ */
int xdet_ext_decode_rois(const float* rois, const float* reg, int ld_reg, int64_t n, float* out, void* stream);

/* ---- A12: bboxes_eval detection part (light_head_rfcn_eval.py:263-287) -------------------
 *   cls logits [N,R,ld_cls], boxes [N,R,4], image_shapes i32 [N,2] (H,W of the raw image),
 *   bbox_img f32 [N,4] -> det_scores [N,num_classes-1,nms_topk], det_boxes [..,4], zero padded.  An image with a
 *   non-finite head logit or a non-finite bbox_img gets NaN in slot 0 of every class.  A box with a NaN coordinate is
 *   never a detection (the reference's clip keeps the NaN and its filter drops the box); every class whose threshold the
 *   ROI's score passed gets NaN in slot 0. */
int xdet_bboxes_eval(const float* cls, int ld_cls, const float* boxes, int N, int R, int num_classes,
                     const int* image_shapes, const float* bbox_img, int net_h, int net_w, float select_thr,
                     float nms_thr, int nms_topk, float* det_scores, float* det_boxes, void* stream);

/* ---- A11 + A12 in the form xdet_net_forward runs them (a door for tests) -----------------
 * xdet_head_decode_probs: one pass over the n = N*R rows of the head's output: cls_reg [n][ld], a row = num_classes logits
 *   and 4 regression values (columns behind them are never read), rois [n][4] -> boxes [n][4] (xdet_ext_decode_rois),
 *   probs [N][num_classes][R] (the softmax, class-major), bad i32 [N]: the caller zeroes it, an image with a non-finite
 *   logit gets 1, nothing else is written.  form 0: the kernel the net gets (32 lanes per ROI when num_classes + 4 <= 32,
 *   else one thread per ROI); form 1: one thread per ROI for any class count.
 *   XDET_ERR_INVALID_ARG, nothing launched: NULL, num_classes < 2, R < 1, n < 0, n % R != 0, ld < num_classes + 4, rois or
 *   boxes not 16-byte aligned, form outside {0, 1}.
 * xdet_bboxes_eval_probs: xdet_bboxes_eval from those probabilities instead of the logits; bad_per_image (may be NULL):
 *   i32 [N], an image with a non-zero entry gets NaN in slot 0 of every class.  Same limits as xdet_bboxes_eval
 *   (R <= 1024, 1 <= nms_topk <= 256, num_classes >= 2, nms_thr >= 0).
 * xdet_bboxes_eval_probs_wide: the same arguments, outputs and bits for 1 <= R <= 6144 ROIs per image -- 6144 is the proposal
 *   stage's own ceiling for rpn_post_nms_top_n; a training net proposes 1800.  R <= 1024 launches xdet_bboxes_eval_probs'
 *   kernel; above that bboxes_eval_wide_kernel, one workgroup per (image, class) as well: the keys of all R ROIs in LDS
 *   (8 bytes each, R rounded up to 2048 / 4096 / 8192 slots), the same order (descending score, ties to the lower ROI index),
 *   and the boxes of the at most min(2 * nms_topk, 512) winners computed again from `boxes`.  XDET_ERR_INVALID_ARG, nothing
 *   launched: everything xdet_bboxes_eval_probs refuses, and R > 6144 by a sentence that names the bound.
 * xdet_bboxes_eval_probs_wide_only: the wide kernel at any 1 <= R <= 6144 (a door for tests: the two kernels on the same
 *   input give the same bits); otherwise as xdet_bboxes_eval_probs_wide. */
int xdet_head_decode_probs(const float* rois, const float* cls_reg, int ld, int num_classes, int R, int64_t n, int form,
                           float* boxes, float* probs, int32_t* bad, void* stream);
int xdet_bboxes_eval_probs(const float* probs, const float* boxes, int N, int R, int num_classes, const int* image_shapes,
                           const float* bbox_img, int net_h, int net_w, float select_thr, float nms_thr, int nms_topk,
                           const int32_t* bad_per_image /* may be NULL */, float* det_scores, float* det_boxes, void* stream);
int xdet_bboxes_eval_probs_wide(const float* probs, const float* boxes, int N, int R, int num_classes, const int* image_shapes,
                                const float* bbox_img, int net_h, int net_w, float select_thr, float nms_thr, int nms_topk,
                                const int32_t* bad_per_image /* may be NULL */, float* det_scores, float* det_boxes, void* stream);
int xdet_bboxes_eval_probs_wide_only(const float* probs, const float* boxes, int N, int R, int num_classes,
                                     const int* image_shapes, const float* bbox_img, int net_h, int net_w, float select_thr,
                                     float nms_thr, int nms_topk, const int32_t* bad_per_image /* may be NULL */,
                                     float* det_scores, float* det_boxes, void* stream);

/* ---- bboxes_eval, scoring part: eval_helper.bboxes_matching_batch (utility/eval_helper.py:700-830) -----------------
 * The TP / FP flags of every detection slot against the image's ground truth, per (image, class), as the greedy walk of
 * bboxes_matching (:722-781) gives them: IoU in f32 in its operation order, times the 0/1 class mask, FIRST maximum over
 * the boxes, strictly greater than the threshold; a detection whose best box is `difficult` is neither; with no box of
 * the class the best box is box 0 and ITS difficult flag decides.  Every one of the K slots is matched, padding too.
 *   det_scores f32 [N,C,K], det_boxes f32 [N,C,K,4]: what xdet_net_forward / xdet_bboxes_eval write (class label c + 1)
 *   glabels i32 [N,G], gbboxes f32 [N,G,4] (ymin,xmin,ymax,xmax in the detections' frame), gdifficults u8 [N,G],
 *   n_gt i32 [N]: image n has its first n_gt[n] entries (clamped to [0, G]; the rest is never read); G <= 512
 *   -> tp u8 [N,C,K], fp u8 [N,C,K], n_gbboxes i32 [N,C] (boxes of the class that are not difficult)
 * An image the forward marked bad (NaN in slot 0 of a class's scores) is not scored: flags and n_gbboxes 0.
 * det_boxes and gbboxes must be 16-byte aligned.  Errors (N, C, K, G <= 0, G > 512, NULL, threshold not finite) ->
 * XDET_ERR_INVALID_ARG before any GPU work. */
int xdet_bboxes_matching(const float* det_scores, const float* det_boxes, int N, int C, int K, const int32_t* glabels,
                         const float* gbboxes, const uint8_t* gdifficults, const int32_t* n_gt, int G,
                         float matching_threshold, uint8_t* tp, uint8_t* fp, int32_t* n_gbboxes, void* stream);
/* metrics.streaming_tp_fp_arrays (utility/metrics.py:102-170) on the device: per class the object count and one record
 * (score, TP-or-FP, image id, slot) for every slot with (tp | fp) and score > 1e-4.  xdet_tpfp_update = the matcher above
 * + the append, enqueued on `stream`; neither synchronises nor reads anything on the host (the call that first sees a larger
 * N than any before allocates the flag scratch, which the handle owns).  Records of a call land behind the class's cursor
 * in (image index within the call, slot) order whatever the scheduling.  image_ids i32 [N] (device) names the images so
 * that shards can be merged.  A call whose records do not fit the class's capacity appends nothing for that class (no
 * objects either) and sets `overflow`; a bad image adds nothing and is counted in `bad_images`.
 * xdet_tpfp_read is the one host-synchronous call: counts i32 [C], nobjects i64 [C], bad_images, overflow; then, when the
 * four record arrays are given (each records_capacity entries, sized by the caller from an earlier call's counts), the
 * records of class 0, 1, ... back to back.  xdet_tpfp_reset clears counts, objects and both flags.
 * The handle is typed like the net handles: another handle type -> XDET_ERR_INVALID_ARG. */
int xdet_tpfp_create(void** acc, int C, int K, int capacity_per_class);
int xdet_tpfp_destroy(void* acc);
int xdet_tpfp_reset(void* acc, void* stream);
int xdet_tpfp_update(void* acc, const float* det_scores, const float* det_boxes, int N, const int32_t* image_ids,
                     const int32_t* glabels, const float* gbboxes, const uint8_t* gdifficults, const int32_t* n_gt, int G,
                     float matching_threshold, void* stream);
int xdet_tpfp_read(void* acc, int32_t* counts_host, int64_t* nobjects_host, int32_t* bad_images_host, int32_t* overflow_host,
                   int64_t records_capacity, float* scores_host, uint8_t* is_tp_host, int32_t* image_id_host,
                   int32_t* slot_host, void* stream);

/* ---- training targets: AnchorEncoder.encode_all_anchors / ext_encode_rois (preprocessing/anchor_manipulator.py:118-171,
 * 319-445) ---------------------------------------------------------------------------------------------------------
 * What the training script does with the ground truth before any loss, on the device (csrc/targets.hip).  All arithmetic
 * in f32, every operation rounded on its own, in the reference's order.  Ground truth as xdet_bboxes_matching takes it:
 * glabels i32 [N,G], gbboxes f32 [N,G,4] (ymin,xmin,ymax,xmax), n_gt i32 [N] (clamped to [0, G]; nothing behind it is
 * read), G <= 512.  Coordinates are expected finite.
 *   overlap O[g,a]: inter = max(min(ymax) - max(ymin), 0) * max(min(xmax) - max(xmin), 0), union = (area_g + area_a) - inter,
 *     O = union == 0 ? 0 : inter / union, times the 0/1 inside mask of candidate a:
 *     ymin >= -b && xmin >= -b && ymax < f32(1 + b) && xmax < f32(1 + b)   (1 + b formed in double from the float argument)
 *   dual-max match (high, low): best_g[a] = FIRST maximum of column a, mv its value; m = -1 if mv < low, -2 if
 *     low <= mv < high, else best_g.  best_a[g] = FIRST maximum of row g (an all-zero row points at candidate 0).  A
 *     candidate named by some best_a[g] takes the FIRST maximum over g of O[g,a] * [best_a[g] == a] -- box 0 when all of
 *     these are zero -- and score O[that box, a]; every other candidate scores mv.
 *   label = glabels[max(m,0)] * [m > -1] - [m < -1];  target = [m > -1] * (((gcy - yref) / href) / s0, ((gcx - xref) / wref) / s1,
 *     log(gh / href) / s2, log(gw / wref) / s3) of box max(m,0), the multiplication by the mask performed.
 *   An image without participating ground truth: labels 0, targets and scores 0 (the reference fails there).
 * xdet_encode_anchors: candidates are the Hh * Ww * A anchors (anchors_yx [Hh*Ww,2], anchors_hw [A,2], index
 *   (y * Ww + x) * A + k as in xdet_rpn_decode; corners yref -+ href / 2, xref -+ wref / 2), all of the image's boxes take part.
 *   -> labels i32 [N,HWA], targets f32 [N,HWA,4], scores f32 [N,HWA].
 * xdet_encode_rois: boxes with label <= 0 are dropped (order kept, G' left); candidates are the image's R ROIs followed by
 *   those G' boxes (M = R + G' <= 8192 with R + G as the bound), reference point yref = ymin + h / 2, h = ymax - ymin.  Then the
 *   sample: exp_fg = round_half_even(f32(rois_per_image) * fg_fraction); pos = {label > 0}, neg = {label == 0 and score >
 *   bg_low_thr} in index order; fg = pos if |pos| < exp_fg else the first exp_fg of shuffle(pos); exp_bg = rois_per_image -
 *   min(|pos|, exp_fg); bg likewise from neg; keep = fg ++ bg; with n_keep < rois_per_image and left = rois_per_image -
 *   n_keep the output rows are keep[tile(range(n_keep), left / n_keep + 1) ++ shuffle(range(n_keep))[: left % n_keep]].
 *   shuffle(S) = S ordered by (key, element) ascending, key = mix(mix(mix(seed ^ 0x9E3779B9) + image) ^ (2 * element + stream))
 *   in 32-bit unsigned arithmetic, mix(x): x ^= x >> 16; x *= 0x7FEB352D; x ^= x >> 15; x *= 0x846CA68B; x ^= x >> 16;
 *   stream 0 for candidates, 1 for the positions of the tail; image = image_ids[n] (device i32 [N]; NULL: n).
 *   -> out_rois f32 [N,rois_per_image,4], out_targets likewise, out_labels i32, out_scores f32 [N,rois_per_image];
 *   out_index (may be NULL) the candidate index, >= R for a ground-truth box; counts (may be NULL) i32 [N,4]: M, |pos|,
 *   |neg|, n_keep; all_labels / all_targets / all_scores (each may be NULL) the unsampled results [N,R+G], entries behind M:
 *   label -1, zeros.  n_keep == 0 (the reference divides by zero): rows zero, label -1, index -1.
 * workspace: xdet_targets_workspace_bytes(N, n_candidates, G) bytes, 16-byte aligned, n_candidates = R + G for
 *   xdet_encode_rois and 0 for xdet_encode_anchors; it needs no initialisation: every control word is cleared by the call.
 *   Box and target arrays must be 16-byte aligned; prior_scaling4 is four floats on the host.  Neither call synchronises or reads anything on the host.
 * Errors -> XDET_ERR_INVALID_ARG before any GPU work: sizes <= 0, G > 512, R + G > 8192, rois_per_image outside [1, 8192],
 *   fg_fraction outside [0, 1], a NULL required pointer, a border or threshold that is not finite, a prior scaling that is
 *   zero or not finite. */
size_t xdet_targets_workspace_bytes(int N, int n_candidates, int G);
int xdet_encode_anchors(const float* anchors_yx, const float* anchors_hw, int Hh, int Ww, int A, float allowed_border,
                        const int32_t* glabels, const float* gbboxes, const int32_t* n_gt, int N, int G, float high_thr,
                        float low_thr, const float* prior_scaling4, void* workspace, int32_t* labels, float* targets,
                        float* scores, void* stream);
int xdet_encode_rois(const float* rois, int R, const int32_t* glabels, const float* gbboxes, const int32_t* n_gt, int N, int G,
                     float allowed_border, float fg_thr, float bg_high_thr, float bg_low_thr, const float* prior_scaling4,
                     int rois_per_image, float fg_fraction, uint32_t seed, const int32_t* image_ids, void* workspace,
                     float* out_rois, float* out_targets, int32_t* out_labels, float* out_scores, int32_t* out_index,
                     int32_t* counts, int32_t* all_labels, float* all_targets, float* all_scores, void* stream);

/* ---- training losses: everything of lighr_head_model_fn between the logits and the scalar loss
 * (light_head_rfcn_train.py:257-275, 312-413; net/xception_body.py:502-533, 560), with the gradients with respect to the
 * logits (csrc/losses.hip; the NumPy statement of the same contract is xdet/losses.py) ----------------------------------
 * All arithmetic in f32, every operation rounded on its own, in the reference's order.
 *   modified_smooth_l1(d = pred - target; sigma): sigma2 = sigma * sigma; |d| < 1 / sigma2 ? (d * d) * (0.5 * sigma2)
 *     : |d| - 0.5 / sigma2;  derivative d * sigma2, else sign(d).  Over a box: ((s(d0) + s(d1)) + s(d2)) + s(d3).
 *   cross entropy of a row x with class y: m = max x, s = sum_j exp(x_j - m) in index order, ce = log(s) - (x_y - m);
 *     derivative exp(x_j - m) / s - [j == y].
 * xdet_rpn_loss (:312-380).  rpn_out, ld, cls_off, box_off, Hh, Ww, A and the anchor index (y * Ww + x) * A + k as
 *   xdet_rpn_decode takes them (the detector's "rpn_out" buffer goes in as it is); labels i32 [N * n_a] and targets f32
 *   [N * n_a, 4] as xdet_encode_anchors writes them, n_a = Hh * Ww * A.  S = N * anchors_per_image rows are selected from
 *   the batch flattened, by the sampler of xdet_encode_rois above run once over all N * n_a anchors: rois_per_image = S,
 *   fg_fraction = fg_ratio, pos = {label > 0}, neg = {label == 0} (no score condition), element = flat anchor index,
 *   image = 0 -- in NumPy, targets.sample_rois(labels_flat, ones, S, fg_ratio, 0., seed, image=0).
 *   -> sel_index i32 [S] (-1 everywhere when n_keep == 0), counts i32 [4]: |pos|, |neg|, n_keep, the number of selected
 *   rows (with multiplicity) whose label > 0 (n_sel_pos), losses f32 [3]:
 *     ce = (sum over the S selected rows of ce(cls row, label > 0)) / S
 *     loc = ((sum over the selected rows with label > 0 of smooth_l1(box row - target)) / n_sel_pos) / fg_ratio
 *     total = ce + loc.
 *   Where the reference yields NaN or fails: n_sel_pos == 0 -> loc = 0; n_keep == 0 -> all three 0, all gradients 0.
 *   grad_rpn_out (may be NULL): d total / d rpn_out in rpn_out's own layout, same ld: EVERY cls / box channel of every anchor
 *   is written (zeros where not selected; channels outside the two ranges are not touched).  A row selected m times
 *   (m = left / n_keep + 1, plus one inside the tail; 1 when n_keep == S) gets (d ce) * (f32(m) / f32(S)) on its two cls
 *   channels and, with label > 0, (d smooth_l1) * ((f32(m) / f32(n_sel_pos)) / fg_ratio) on its four box channels.
 * xdet_head_loss (:384-413, xception_body.py:502-533, 560).  cls [N,P,C] at cls_reg + cls_off, reg [N,P,4] at cls_reg +
 *   reg_off, row stride ld (the detector's "cls_reg" buffer: cls_off 0, reg_off C); labels i32 [N,P], targets f32 [N,P,4]
 *   as xdet_encode_rois writes them.
 *     per_roi[n,p] = ce(cls row, label) + [label > 0] * (smooth_l1(reg row - target) / fg_ratio); a row whose label is
 *     outside [0, C) (the -1 rows of xdet_encode_rois) has 0 and gradient 0.
 *   ohem_k > 0: K = min(ohem_k, P), select[n,:] = the rows of the K largest per_roi[n,:], descending, equal values in
 *   ascending row order (tf.nn.top_k); the per-ROI value is computed by one instruction sequence for every row, so rows with
 *   equal inputs tie bit for bit.  ohem_k == 0 (using_ohem=False): K = P, select[n,:] = 0 .. P-1.
 *   -> losses f32 [3]: the means over the N * K selected rows of per_roi (head_loss), of its ce term, of its smooth-L1 term
 *   (the reference's two summaries); per_roi f32 [N,P]; select i32 [N,K].
 *   grad_cls_reg (may be NULL): d head_loss / d cls_reg in the buffer's layout: the C + 4 channels of all N * P rows are
 *   written, zero for rows not selected: (d ce) * w and ((d smooth_l1) / fg_ratio) * w, w = 1 / f32(N * K).
 * Every float sum is a tree of a fixed shape: the same call twice gives the same bits.  Neither call synchronises or reads
 * anything on the host.  workspace: xdet_losses_workspace_bytes(N, anchors_per_image) bytes (anchors_per_image 0: enough
 * for xdet_head_loss only; 0 is returned for sizes outside the limits), 16-byte aligned; it needs no initialisation and a
 * workspace sized for a larger N serves a smaller one.
 * Limits: N * n_a <= 2^27, S <= 32768 (N = 128 at 256 anchors per image); N <= 1024, P <= 8192, 2 <= C <= 128.
 * Errors -> XDET_ERR_INVALID_ARG before any GPU work: sizes outside the limits, ld not a multiple of 4 / cls_off odd /
 *   box_off not a multiple of 4 (RPN), channel ranges outside ld or overlapping, fg_ratio outside (0, 1], sigma not positive
 *   and finite, ohem_k < 0, a NULL required pointer, rpn_out / targets / workspace / gradient not 16-byte aligned (RPN). */
size_t xdet_losses_workspace_bytes(int N, int anchors_per_image);
int xdet_rpn_loss(const float* rpn_out, int ld, int cls_off, int box_off, int N, int Hh, int Ww, int A, const int32_t* labels,
                  const float* targets, int anchors_per_image, float fg_ratio, uint32_t seed, float sigma, void* workspace,
                  int32_t* sel_index, int32_t* counts, float* losses, float* grad_rpn_out, void* stream);
int xdet_head_loss(const float* cls_reg, int ld, int cls_off, int reg_off, int N, int P, int C, const int32_t* labels,
                   const float* targets, float fg_ratio, int ohem_k, float sigma, void* workspace, float* losses, float* per_roi,
                   int32_t* select, float* grad_cls_reg, void* stream);

/* ---- the backward of a dense layer y = act(x W + b), act = identity or ReLU (csrc/dense_backward.hip; the NumPy statement
 * of the same contract is xdet.ops.host_dense_backward) -----------------------------------------------------------------
 *   x  f32 [M,K], row stride ld_x          the layer's input
 *   w  f32 [K,J] dense, row-major          the kernel as the checkpoint stores it ([in, out]), on the device
 *   y  f32 [M,J], row stride ld_y, or NULL the forward's output AFTER its ReLU; NULL for a layer without one
 *   dy f32 [M,J], row stride ld_dy         d loss / d y
 *     g  = dy                  if y is NULL
 *        = y > 0 ? dy : 0      otherwise: exact zeros of y mask, and so does a NaN in y (NaN > 0 is false: the gradient
 *                              behind a NaN activation is 0, whatever dy holds there)
 *   -> dx f32 [M,K], row stride ld_dx = g W^T (NULL: skipped);  dw f32 [K,J] dense = x^T g;  db f32 [J] = column sums of g.
 * Columns at or beyond a matrix's width (K for x and dx, J for y and dy) are never read -- padding may hold NaN -- and
 * nothing is written to dx beyond column K - 1.  The detector's buffers go in as they are: dy = the gradient xdet_head_loss
 * wrote (ld of "cls_reg", J = C + 4), x = "fc"; then dy = that call's dx, y = "fc", x = "pooled".
 * Arithmetic: both products on the matrix pipe in split precision: every operand value v is hi = f16(v), lo = f16(v - hi),
 *   a product is hi*hi + hi*lo + lo*hi accumulated in f32 (lo*lo, below 2^-22 of the product, is dropped).  Before the split
 *   each of x, w and g is multiplied by a power of two of its own, 2^(11 - floor(log2(max |v|))) over the operand (columns
 *   inside the width only; 2^0 for an all-zero operand), which a pre-pass finds on the device; the results are multiplied
 *   by the inverse powers.  Both steps are exact, so gradients far below the f16 range keep f32-class accuracy, and scaling
 *   dy by a power of two scales dx, dw and db by exactly that power (bit for bit, short of f32 underflow).  An operand holding
 *   an inf or a NaN makes the outputs it reaches NaN.  db is summed in f32.
 * Order of the sums: dw's sum over the M rows is cut into ranges of
 *     rows_per_range = round_up(ceil(M / max(1, 512 / tiles)), 128),  tiles = ceil(K / 128) * ceil(J / (J <= 32 ? 32 : 128))
 *   rows (integer divisions), each summed on its own and the ranges then added in index order; db is summed over chunks of
 *   max(64, ceil(M / 1024)) rows in row order, the chunks then added in index order.  No float atomics: the same call gives
 *   the same bits; rows computed from batches of different M are not required to agree bit for bit.
 * workspace: xdet_dense_backward_workspace_bytes(M, K, J) bytes (never 0 for sizes inside the limits, 0 outside them); it
 *   needs no initialisation and may be larger.  The call does not synchronise and reads nothing on the host.
 * Limits: K, J <= 4096, M * max(K, J) < 2^31.
 * Errors -> XDET_ERR_INVALID_ARG before any GPU work: a size <= 0 or outside the limits, ld_x < K, ld_dy < J, ld_y < J with
 *   a y, ld_dx < K with a dx, a NULL x, w, dy, dw, db or workspace. */
size_t xdet_dense_backward_workspace_bytes(int M, int K, int J);
int xdet_dense_backward(const float* x, int ld_x, const float* w, const float* y, int ld_y, const float* dy, int ld_dy, int M,
                        int K, int J, float* dx, int ld_dx, float* dw, float* db, void* workspace, void* stream);

/* ---- the backward of a stride-1 'SAME' convolution y = act(conv(xe, w) + b), xe = x or max(x, 0), act = identity or ReLU
 * (csrc/conv_backward.hip: xdet_conv_backward_strided's code at stride 1, 'SAME', always on the 128-row tile of dw; the NumPy
 * statement of the same contract is xdet.ops.host_conv_backward).  NHWC, dilation 1,
 * zero padding of (kh - 1) / 2 rows and (kw - 1) / 2 columns on either side; M = N * H * W pixels -------------------------
 *   x  f32 [N,H,W,C], pixel stride ld_x          the layer's input (relu_in != 0: the conv read max(x, 0))
 *   w  f32 [kh,kw,C,J] dense                     the kernel as the checkpoint stores it (HWIO), on the device
 *   y  f32 [N,H,W,J], pixel stride ld_y, or NULL the forward's output AFTER its ReLU; NULL for a layer without one
 *   dy f32 [N,H,W,J], pixel stride ld_dy         d loss / d y
 *     g  = dy, or y > 0 ? dy : 0 with a y (exact zeros of y mask, and so does a NaN in y, as in xdet_dense_backward)
 *     xe = x,  or x > 0 ? x : 0 with relu_in (a NaN in x counts as 0 and gets the gradient 0)
 *   -> dx f32 [N,H,W,C], pixel stride ld_dx (NULL: skipped): dx[n,h,w,c] = sum over taps (a,b) and j of
 *        g[n, h - a + kh/2, w - b + kw/2, j] * w[a,b,c,j] (terms outside the image are absent), and with relu_in 0 wherever
 *        x > 0 is false;
 *      dw f32 [kh,kw,C,J] dense: dw[a,b,c,j] = sum over pixels of xe[n, h + a - kh/2, w + b - kw/2, c] * g[n,h,w,j];
 *      db f32 [J] = column sums of g.
 * A shift never leaves its image or its image row: what lies outside counts as zero and is not read.  Channels at or beyond
 * a tensor's count (C for x and dx, J for y and dy) are never read -- padding may hold NaN -- and nothing is written to dx
 * beyond channel C - 1.  The detector's buffers go in as they are: x = "mid_x" with relu_in, y = "rpn_hidden", dy = the dx of the
 * xdet_dense_backward call over the RPN's two 1x1 heads.
 * Arithmetic: as xdet_dense_backward -- both products on the matrix pipe in split precision (hi*hi + hi*lo + lo*hi, f32
 *   accumulation), each of xe, w and g under a power of two of its own, 2^(11 - floor(log2(max |v|))) over the operand
 *   (channels inside the count only; 2^0 for an all-zero operand), found by a pre-pass on the device and taken out again
 *   exactly: scaling dy by a power of two scales dx, dw and db by exactly that power.  db is summed in f32.
 * Order of the sums: dx reduces over (tap, j), taps in storage order, in one pipeline.  dw's sum over the M pixels is cut
 *   into ranges by xdet_dense_backward's rule with tiles = ceil(kh * kw * C / 128) * ceil(J / (J <= 32 ? 32 : 128)), the
 *   ranges added in index order; db in chunks of max(64, ceil(M / 1024)) pixels added in index order.  No float atomics:
 *   the same call gives the same bits.
 * workspace: xdet_conv_backward_workspace_bytes(N, H, W, C, J, kh, kw) bytes (never 0 inside the limits, 0 outside them); it
 *   needs no initialisation and may be larger.  The call does not synchronise and reads nothing on the host.  No patch
 *   matrix is written anywhere: both products fetch the shifted pixels as they go.
 * Limits: kh, kw odd and <= 15; C, J <= 4096; M * max(C, J, every ld given) < 2^31.
 * Errors -> XDET_ERR_INVALID_ARG before any GPU work: a size <= 0 or outside the limits, an even kh or kw, ld_x < C,
 *   ld_dy < J, ld_y < J with a y, ld_dx < C with a dx, a NULL x, w, dy, dw, db or workspace. */
size_t xdet_conv_backward_workspace_bytes(int N, int H, int W, int C, int J, int kh, int kw);
int xdet_conv_backward(const float* x, int ld_x, const float* w, const float* y, int ld_y, const float* dy, int ld_dy, int N,
                       int H, int W, int C, int J, int kh, int kw, int relu_in, float* dx, int ld_dx, float* dw, float* db,
                       void* workspace, void* stream);

/* ---- the backward of a convolution at stride 1 or 2, 'VALID' or 'SAME' (csrc/conv_backward.hip; the NumPy statement
 * of the same contract is xdet.ops.host_conv_backward_strided): the stem convs.  Everything xdet_conv_backward's comment says
 * holds here -- NHWC and HWIO, g and xe with their NaN rules, channels at or beyond a count never read or written, dx == NULL
 * skips dx, no synchronisation and no host read, no patch matrix, no float atomics, the same bits from the same call over a
 * workspace of any contents, a power of two on dy taken out of dx, dw and db exactly -- except the geometry ------------------
 *   stride 1 or 2; padding 0 = 'VALID', 1 = 'SAME' (pad_mode of xdet_conv_create); dilation 1; kh, kw odd and <= 15.
 *   x, dx [N,H,W,C] (M = N*H*W pixels);  y, dy [N,Ho,Wo,J] (Mo = N*Ho*Wo pixels);  w, dw [kh,kw,C,J];  db [J].
 *   'VALID': Ho = floor((H - kh) / stride) + 1, no padding.  'SAME' (TensorFlow's): Ho = ceil(H / stride), total padding
 *   max((Ho - 1) * stride + kh - H, 0), the smaller half pt in front.  Wo and pl follow the same rules from W and kw.
 *     dw[a,b,c,j] = sum over n, oh, ow of xe[n, oh*stride + a - pt, ow*stride + b - pl, c] * g[n,oh,ow,j]
 *     dx[n,h,w,c] = sum over taps (a,b) and j of g[n, (h + pt - a) / stride, (w + pl - b) / stride, j] * w[a,b,c,j], over the
 *                   taps for which both quotients are integers inside the output map; with relu_in 0 wherever x > 0 is false
 *     db = column sums of g
 *   Terms outside the image are absent and their pixels are not read.  Under 'VALID' at stride 2 an input row or column that
 *   no window covers (the last row of an even H with kh = 3) is never read -- it may hold NaN -- and gets dx exactly +0: dx
 *   is written completely.
 * Arithmetic and order of the sums: xdet_conv_backward's.  dx reduces over (tap, j), taps in storage order, in one pipeline
 *   (at stride 2 a pixel whose parity does not match a tap feeds that tap zeros).  dw's sum over the Mo OUTPUT pixels is cut
 *   into ranges by xdet_dense_backward's rule with M = Mo, the ranges added in index order.  Two tile shapes:
 *     kh * kw * C > 32 or J > 32: 128 rows of dw by 32 (J <= 32) or 128 columns, tiles = ceil(kh * kw * C / 128) *
 *       ceil(J / (J <= 32 ? 32 : 128)), a range summed in pixel order -- xdet_conv_backward's;
 *     kh * kw * C <= 32 and J <= 32 (block1_conv1: 27 x 32): one tile of 32 x 32, tiles = 1 (up to 512 ranges: the ranges are
 *       the parallelism).  A range is walked in steps of 128 pixels; the pixels [32 q, 32 q + 32) of every step are summed,
 *       in pixel order, into quarter q = 0 .. 3, and a range's sum is ((q0 + q1) + q2) + q3.
 *   db in chunks of max(64, ceil(Mo / 1024)) output pixels added in index order.  At stride 1 'SAME' with kh * kw * C > 32
 *   (or J > 32) the three results have the bits of xdet_conv_backward; dx and db have them always.
 * workspace: xdet_conv_backward_strided_workspace_bytes(...) bytes (never 0 inside the limits, 0 outside them); it needs no
 *   initialisation and may be larger.
 * Limits: C, J <= 4096; M * max(C, ld_x, ld_dx) < 2^31 and Mo * max(J, ld_y, ld_dy) < 2^31.
 * Errors -> XDET_ERR_INVALID_ARG before any GPU work: those of xdet_conv_backward, another stride, another padding, a 'VALID'
 *   geometry with Ho < 1 or Wo < 1. */
size_t xdet_conv_backward_strided_workspace_bytes(int N, int H, int W, int C, int J, int kh, int kw, int stride, int padding);
int xdet_conv_backward_strided(const float* x, int ld_x, const float* w, const float* y, int ld_y, const float* dy, int ld_dy,
                               int N, int H, int W, int C, int J, int kh, int kw, int stride, int padding, int relu_in,
                               float* dx, int ld_dx, float* dw, float* db, void* workspace, void* stream);

/* ---- batch normalisation over NHWC rows, forward and backward, with batch or moving statistics (csrc/batchnorm.hip; the
 * NumPy statements of the same contract are xdet.ops.host_batch_norm_forward / host_batch_norm_backward).  A tensor is
 * M = N * H * W rows of C channels with a row stride ld >= C; every statistic is per channel -----------------------------
 *   x f32 [M,C], row stride ld_x;  gamma, beta f32 [C];  eps, momentum: the layer's constants (the reference uses 1e-5 and
 *   0.997 for the large-separable block, net/resnet_v2.py, and 1e-4 and 0.99 for the Xception layers)
 * Forward, training != 0:
 *     mean[c] = sum_m x[m,c] / M,   var[c] = sum_m (x[m,c] - mean[c])^2 / M   -- centred on the finished mean: two sum passes
 *     over x.  E[x^2] - E[x]^2 is not this contract (it loses the variance of a channel whose mean is large).
 *     invstd = 1 / sqrt(var + eps);  xhat = (x - mean) * invstd;  y = xhat * gamma + beta, then max(., 0) when relu != 0
 *     -> y f32 [M,C], row stride ld_y;  save_mean, save_invstd f32 [C] (what the backward takes)
 *     moving_mean, moving_var f32 [C] (both or neither; NULL: no update): TensorFlow's fused update
 *       moving_mean -= (moving_mean - mean) * (1 - momentum);   moving_var -= (moving_var - var * M / max(M - 1, 1)) * (1 - momentum)
 * Forward, training == 0: the same y with mean = moving_mean, var = moving_var, which are required and not written;
 *     save_mean and save_invstd receive what was used.
 * Backward:  y f32 [M,C], row stride ld_y, or NULL: the forward's output AFTER its ReLU;  dy f32 [M,C], row stride ld_dy
 *     g = dy, or y > 0 ? dy : 0 with a y (exact zeros of y mask, and so does a NaN in y, as in xdet_dense_backward); the
 *     mask is the forward's own y, never a recomputed one.  xhat is recomputed from x, save_mean and save_invstd.
 *     -> dbeta f32 [C] = sum_m g;   dgamma f32 [C] = sum_m g * xhat;
 *        dx f32 [M,C], row stride ld_dx (NULL: skipped; dgamma and dbeta are written all the same)
 *           = gamma * invstd * (g - dbeta / M - xhat * dgamma / M)   training != 0 (the gradient through the statistics)
 *           = gamma * invstd * g                                     training == 0
 * Channels at or beyond C are never read -- padding may hold NaN -- and nothing is written beyond channel C - 1 of y or dx.
 * x must not overlap y or dx (x is read again after the first rows of the output are written).
 * Order of the sums: every per-channel sum over the M rows is cut into chunks of max(64, ceil(M / 1024)) rows (at most 1024
 *   chunks).  Inside a chunk the rows are dealt to sixteen sums by (row - first row of the chunk) mod 16, each added in row
 *   order, and the sixteen are added in index order; the chunks are then added in index order.  All of it depends on M alone:
 *   pointer alignment and strides (vector or scalar loads) do not change a bit.  No float atomics: the same call gives the
 *   same bits, whatever the workspace held.  Every sum is a plain f32 add of plain f32 products (no fused multiply-add, no
 *   rescaling), and the divisions by M are f32 divisions, so scaling dy by a power of two scales dx, dgamma and dbeta by
 *   exactly that power (bit for bit, short of f32 underflow).
 * workspace: xdet_batch_norm_workspace_bytes(M, C) bytes for either call (never 0 inside the limits, 0 outside them); it
 *   needs no initialisation and may be larger.  Neither call synchronises or reads anything on the host.
 * Limits: C <= 4096; M * max(C, every ld given) < 2^31.
 * Errors -> XDET_ERR_INVALID_ARG before any GPU work: a size <= 0 or outside the limits, an ld below C (ld_y and ld_dx only
 *   with a y / dx in the backward), a NULL x, gamma, beta, y, save_mean, save_invstd (forward), a NULL x, dy, gamma,
 *   save_mean, save_invstd, dgamma, dbeta (backward), a NULL workspace, training == 0 without both moving statistics, one
 *   moving statistic without the other. */
size_t xdet_batch_norm_workspace_bytes(int M, int C);
int xdet_batch_norm_forward(const float* x, int ld_x, int M, int C, const float* gamma, const float* beta, float eps,
                            int training, float momentum, float* moving_mean, float* moving_var, int relu, float* y, int ld_y,
                            float* save_mean, float* save_invstd, void* workspace, void* stream);
int xdet_batch_norm_backward(const float* x, int ld_x, const float* y, int ld_y, const float* dy, int ld_dy, int M, int C,
                             const float* gamma, const float* save_mean, const float* save_invstd, int training, float* dx,
                             int ld_dx, float* dgamma, float* dbeta, void* workspace, void* stream);

/* ---- the backward of the depthwise 3x3 conv y = depthwise(xe, k), xe = x or max(x, 0): stride 1, 'SAME', dilation d = 1 or 2
 * (csrc/depthwise_backward.hip; the NumPy statement of the same contract is xdet.ops.host_depthwise_backward).  NHWC, zero
 * padding of d rows and d columns on either side; M = N * H * W pixels ----------------------------------------------------
 *   x  f32 [N,H,W,C], pixel stride ld_x          the layer's input (relu_in != 0: the conv read max(x, 0))
 *   k  f32 [3,3,C,1] dense                       the depthwise kernel as the checkpoint stores it, on the device
 *   dy f32 [N,H,W,C], pixel stride ld_dy         g = d loss / d y
 *     xe = x,  or x > 0 ? x : 0 with relu_in (a NaN in x counts as 0 and gets the gradient 0, as in xdet_conv_backward)
 *   -> dx f32 [N,H,W,C], pixel stride ld_dx (NULL: skipped; dw is written all the same):
 *        dx[n,h,w,c] = sum over taps (a,b) of g[n, h - (a-1)d, w - (b-1)d, c] * k[a,b,c], and with relu_in 0 wherever x > 0
 *        is false;
 *      dw f32 [3,3,C,1] dense: dw[a,b,c] = sum over pixels of xe[n, h + (a-1)d, w + (b-1)d, c] * g[n,h,w,c].
 * A term whose source pixel lies outside the image is absent and its pixel is not read: a shift never leaves its image.
 * Channels at or beyond C are never read -- padding may hold NaN -- and nothing is written to dx beyond channel C - 1.
 * x and dy must not overlap dx.
 * Arithmetic and order of the sums: every term is a plain f32 product, added in f32 to a running sum that starts at 0 (no
 *   fused multiply-add, no rescaling), so scaling dy by a power of two scales dx and dw by exactly that power (bit for bit,
 *   short of f32 underflow).  dx adds its taps in storage order, (0,0), (0,1), ..., (2,2): it is the f32 host statement bit
 *   for bit, but for the sign of a zero.  dw[a,b,c] is summed over the pixel of ITS xe factor, m = (n H + h) W + w in
 *   0 .. M - 1 (the term of pixel m is xe[m] * g[n, h - (a-1)d, w - (b-1)d]): the pixels are cut into chunks of
 *   max(64, ceil(M / 1024)) consecutive m (at most 1024 chunks); inside a chunk the pixels are dealt to four sums by
 *   (m - first m of the chunk) mod 4, each added in pixel order, and the four are added in index order; the chunks are then
 *   added in index order.  All of it depends on (N, H, W) alone: pointer alignment and strides (vector or scalar accesses) do
 *   not change a bit.  No float atomics: the same call gives the same bits, whatever the workspace held.
 * workspace: xdet_depthwise_backward_workspace_bytes(N, H, W, C) bytes (never 0 inside the limits, 0 outside them); it needs
 *   no initialisation and may be larger.  The call does not synchronise and reads nothing on the host.
 * Limits: d = 1 or 2; C <= 4096; M * max(C, every ld given) < 2^31.
 * Errors -> XDET_ERR_INVALID_ARG before any GPU work: a size <= 0 or outside the limits, another dilation, ld_x < C,
 *   ld_dy < C, ld_dx < C with a dx, a NULL x, k, dy, dw or workspace. */
size_t xdet_depthwise_backward_workspace_bytes(int N, int H, int W, int C);
int xdet_depthwise_backward(const float* x, int ld_x, const float* k, const float* dy, int ld_dy, int N, int H, int W, int C,
                            int dilation, int relu_in, float* dx, int ld_dx, float* dw, void* workspace, void* stream);
/* out = a + b over M rows of C channels, f32, each tensor with a row stride ld >= C (the exit flow's residual add behind a
 * training-mode batch norm, and the join of two gradients).  out may be a (or b) itself; any other overlap is not allowed.
 * Nothing at or beyond channel C is read or written.  Limits: C <= 2^24, M * max(ld) < 2^31.  Errors ->
 * XDET_ERR_INVALID_ARG before any GPU work: a size <= 0 or outside the limits, an ld below C, a NULL a, b or out. */
int xdet_add_rows(const float* a, int ld_a, const float* b, int ld_b, float* out, int ld_out, int M, int C, void* stream);

/* ---- the backward of max_pooling2d(3, 2, 'same') and the stride-2 gather / scatter of a 1x1 / stride-2 projection
 *      (csrc/pool_backward.hip): what the Xception entry flow's backward adds to the op set ------------------------------
 * x [N,H,W,C] (the pool's input), dy [N,Ho,Wo,C], dx [N,H,W,C], f32 NHWC, each with a pixel stride ld >= C.  Geometry is
 * TensorFlow's 'SAME': Ho = ceil(H / 2), Wo = ceil(W / 2), total padding max((Ho - 1) * 2 + 3 - H, 0) with the smaller half in
 * front (1 / 1 on an odd extent, 0 / 1 on an even one); a padded position never wins and windows never cross an image.
 *   Each window sends its dy to its FIRST maximum in row-major window order: strict > against the running best, which starts
 *   at the window's first in-image element (so a NaN wins only from that place).  A pixel lies in at most 2 x 2 windows; their
 *   shares are added to 0 in ascending (oh, ow) order, each add rounded: ops.host_max_pool_backward in float32, bit for bit.
 *   dx is written completely (0 where nothing arrives); its columns C .. ld - 1 are not written, and those of x and dy are
 *   read into no result.  A gather over x -- no stored argmax, no float atomics: the same call gives the same bits.
 * Limits: C <= 4096; N * H * W * max(C, every ld) < 2^31.  The call does not synchronise and reads nothing on the host.
 * Errors -> XDET_ERR_INVALID_ARG before any GPU work: a size <= 0 or outside the limits, an ld below C, a NULL x, dy or dx. */
int xdet_maxpool3x3s2_backward(const float* x, int ld_x, const float* dy, int ld_dy, int N, int H, int W, int C, float* dx, int ld_dx,
                               void* stream);
/* out[n,i,j,:] = x[n,2i,2j,:], out [N, ceil(H/2), ceil(W/2), C]: the input a 1x1 / stride-2 'SAME' conv reads (its padding is 0
 * for every H), dense for xdet_conv_backward.  Same limits and errors as above (N, H, W are x's). */
int xdet_subsample2(const float* x, int ld_x, int N, int H, int W, int C, float* out, int ld_out, void* stream);
/* out[n,h,w,:] = a[n,h,w,:] + b[n,h/2,w/2,:] where h and w are both even, a's bits everywhere else; a, out [N,H,W,C],
 * b [N, ceil(H/2), ceil(W/2), C]: the adjoint of xdet_subsample2 added to a, the join of a block's two input gradients.  out
 * may be a itself; any other overlap is not allowed.  Same limits and errors as above. */
int xdet_add_upsample2(const float* a, int ld_a, const float* b, int ld_b, int N, int H, int W, int C, float* out, int ld_out,
                       void* stream);

/* ---- the optimizer step (csrc/optimizer.hip): tf.train.MomentumOptimizer with the reference's L2 term over a table of
 * tensors, and the refresh of a forward layer's operands from a kernel in device memory (csrc/conv_repack.hip) -------------
 * A slot is one variable: var, grad and accum (the momentum slot) are dense f32 arrays of n elements in device memory; var
 * and accum are updated in place.  decay != 0: the variable is in the L2 set (light_head_rfcn_train.py:420,435).  Per
 * element, every operation an f32 operation rounded on its own (no fused multiply-add):
 *     g     = grad + weight_decay * var        (decay != 0;  g = grad otherwise)
 *     accum = momentum * accum + g
 *     var   = var - lr * accum
 * -- the NumPy statement of the same contract is xdet.ops.host_momentum_step, and the call equals it bit for bit (f32
 * denormals and signed zeros included).  One launch serves the whole table: the element space is cut into chunks of 4096
 * consecutive elements of one slot (a slot's last chunk is short; chunks are numbered slot by slot, in table order), one
 * workgroup per chunk; the chunk table is built here and uploaded into the workspace with the slot table.  Accesses are
 * 128-bit wide in a slot whose three pointers are 16-byte aligned.
 * l2 (a device float, or NULL: not computed) = sum over the decayed slots of sum var^2 / 2 on the values BEFORE the update,
 * in f32, in this fixed order (no float atomics: the same call gives the same bits):
 *   - element j of a chunk belongs to vector q = j / 4; vector q to thread q % 256, as its vector i = q / 256 (0..3); an
 *     element beyond the slot's end counts as +0;
 *   - a vector's sum is (v0^2 + v1^2) + (v2^2 + v3^2); a thread's is (t0 + t1) + (t2 + t3) over its four vectors;
 *   - the 256 thread sums of a chunk fold pairwise: for w = 128, 64 .. 1: s[i] += s[i + w] for i < w; s[0] is the chunk's
 *     partial (0 for a chunk of a slot without decay);
 *   - the C chunk partials fold the same way with P = the power of two at or above C: for w = P/2 .. 1: p[i] += p[i + w]
 *     for i < w where i + w < C; l2 = p[0] / 2.
 *   Every term is non-negative and passes through at most 1 + 2 + 2 + 8 + ceil(log2(C)) roundings, which bounds the
 *   relative error against the exact sum by that count times 2^-24 (to first order).
 * workspace: xdet_momentum_step_workspace_bytes(slots, n_slots) bytes of device memory (0 for a table the call refuses); it
 *   needs no initialisation and may be larger; the call after a call on the same stream may reuse it.  The call does not
 *   synchronise.  Limits: at most 65536 slots and 2^22 chunks.
 * Errors -> XDET_ERR_INVALID_ARG before any GPU work, never a skipped slot: a NULL or empty table, a slot with a NULL var,
 *   grad or accum or with n <= 0, a NULL workspace, a table beyond the limits. */
typedef struct {
  float* var;
  const float* grad;
  float* accum;
  int64_t n;
  int decay;
} xdet_momentum_slot;
size_t xdet_momentum_step_workspace_bytes(const xdet_momentum_slot* slots_host, int n_slots);
int xdet_momentum_step(const xdet_momentum_slot* slots_host, int n_slots, float lr, float momentum, float weight_decay, float* l2,
                       void* workspace, void* stream);
/* The guard of the step: whether the gradients of a slot table may be applied, decided on the device.
 * xdet_grad_stats reads `grad` of every slot (var and accum are not looked at and may be anything) in the chunks of
 * xdet_momentum_step -- 4096 consecutive elements of one slot, one workgroup each, 128-bit accesses in a slot whose grad is
 * 16-byte aligned -- and writes ONE 16-byte record to stats_dev (device memory, 4-byte aligned):
 *     float   grad_sq         sum over all slots of sum grad^2, f32, in the fixed order of l2 above (vector, thread, the 256
 *                             threads of a chunk pairwise, the C chunk partials pairwise; not halved).  NaN or +inf when a
 *                             gradient is not finite or the sum overflows
 *     int32_t nonfinite       the number of elements that are NaN, +inf or -inf (it stays at INT32_MAX, never wraps)
 *     int32_t first_bad_slot  the lowest table index of a slot that holds one, -1 if none does
 *     int32_t 0
 * An element beyond a slot's end is absent: it adds +0 and is never counted, whatever lies there.  Two launches, the chunks'
 * partials (sum, count, INT32_MAX-or-slot) and one workgroup that folds them (sum, sum, min) in the order the C partials of
 * l2 fold; no float atomic, no fence, no workgroup that waits for another: the same call gives the same bits.
 * xdet_momentum_step_guarded is xdet_momentum_step with one more argument.  skip_dev (an int32 in device memory, or NULL):
 * every workgroup reads *skip_dev once; non-zero: nothing is stored to any var or accum -- their bytes stay -- while l2 is
 * still written (it is computed from the values before the update either way).  NULL or zero: xdet_momentum_step, the same
 * launches and the same bits.  The intended skip_dev is the address of the record's `nonfinite`, stats_dev + 4, after
 * xdet_grad_stats on the same stream: the host decides nothing and waits for nothing.
 * workspace of xdet_grad_stats: xdet_grad_stats_workspace_bytes(slots, n_slots) bytes (0 for a table the call refuses), under
 * the rules of the step's; the two calls may not share one workspace unless the caller orders them on one stream.
 * Errors and limits as xdet_momentum_step's, with these differences: xdet_grad_stats refuses a slot with a NULL grad (only)
 * and a NULL or misaligned stats_dev. */
size_t xdet_grad_stats_workspace_bytes(const xdet_momentum_slot* slots_host, int n_slots);
int xdet_grad_stats(const xdet_momentum_slot* slots_host, int n_slots, void* stats_dev, void* workspace, void* stream);
int xdet_momentum_step_guarded(const xdet_momentum_slot* slots_host, int n_slots, float lr, float momentum, float weight_decay,
                               float* l2, const int32_t* skip_dev, void* workspace, void* stream);
/* The clipped step: xdet_momentum_step on gradients scaled to a global norm of at most clip_norm, decided on the device.
 * stats_dev is the 16-byte record xdet_grad_stats left on the same stream (device memory, 4-byte aligned).  Every workgroup
 * reads its grad_sq once -- and, with guard != 0, its nonfinite, as the guarded form reads *skip_dev -- and computes
 *     norm  = sqrt(grad_sq)                     f32, correctly rounded (the IEEE square root, no fast form)
 *     scale = clip_norm / max(norm, clip_norm)  f32, correctly rounded; max(a, b) = b where a <= b, else a: a NaN norm stays
 * The norm is the guard's `grad_norm`: over the loss gradients of ALL slots, without the L2 term.  Per element
 *     g = grad * scale;  g += weight_decay * var where the slot's decay is set
 * and the rest is xdet_momentum_step operation for operation and rounding for rounding (one more rounding per element, the
 * product; l2 as there, from the values before the update).  It follows that
 *   - norm <= clip_norm gives scale == 1.0f exactly (x / x is 1), grad * 1.0f is grad, and the call stores the bits of
 *     xdet_momentum_step;
 *   - guard != 0 and nonfinite != 0: nothing is stored to any var or accum -- their bytes stay -- while l2 is still written;
 *   - guard == 0 decides nothing: a NaN grad_sq gives a NaN scale and with it NaN in EVERY var and accum; a grad_sq of +inf
 *     (an infinite element, or a sum that overflowed) gives scale 0, so a finite gradient counts as zero and an infinite one
 *     gives NaN in its element.  That is the caller's choice; the guard is what prevents it.
 * scale_out (a device float, or NULL): workgroup 0 writes the scale it used, by one plain vector store, skipped step or not.
 * The launches are xdet_momentum_step's (the chunks, then the fold of l2), the workspace is xdet_momentum_step_workspace_bytes;
 * no float atomic, no fence, no workgroup that waits for another: the same call gives the same bits.
 * Errors -> XDET_ERR_INVALID_ARG before any GPU work: a clip_norm that is not finite or <= 0, a NULL or misaligned
 *   stats_dev, and everything xdet_momentum_step refuses. */
int xdet_momentum_step_clipped(const xdet_momentum_slot* slots_host, int n_slots, float lr, float momentum, float weight_decay,
                               float* l2, const void* stats_dev, float clip_norm, int guard, float* scale_out, void* workspace,
                               void* stream);
/* Rewrite, on the device and in place, every operand buffer a conv layer (xdet_conv_create) owns from a dense f32
 * [kh,kw,cin,cout] kernel in device memory: the transposed matrix of the f32 mode, or the per-row power-of-two pre-scale, the
 * f16 hi / lo split, the K-blocked copies, the fp8 x8 copy of a pointwise f16x3 layer and the epilogue scale (the scale the
 * layer was created with times 2^-shift of the row).  xdet_conv_create makes the buffers by this same repack, from the kernel
 * it uploads (csrc/conv_repack.hip is the one statement of their layouts), so each buffer holds exactly what xdet_conv_create
 * would have made from the same values; padding rows and channels stay +0.  shift_dev (f32 [cout] in device memory, or NULL: kept) replaces the
 * epilogue shift.  Two passes over the kernel (the row maxima, then exponent, split and scatter) on `stream`, no
 * synchronisation, nothing read on the host.  Errors -> XDET_ERR_INVALID_ARG with the layer unchanged: a NULL kernel, a
 * grouped or spectral layer, a layer that carries an activation or planes exponent or a planes affine (a calibrated or
 * net-owned layer: its scale arrays are no longer the ones it was created with).  The shape is the layer's: the caller
 * vouches for kh * kw * cin * cout floats.  Afterwards the layer's host copy of the scale is stale: a later activation
 * exponent (a plan's calibration) is refused for this layer. */
int xdet_conv_set_kernel_device(void* layer, const float* kernel_hwio_dev, const float* shift_dev, void* stream);
/* The same for a spectral conv layer (xdet_spectral_conv_create, or the two a net owns): every operand buffer of its per-bin
 * GEMM layer from a dense f32 [taps][cin][cout] kernel in device memory, in place.  The layer keeps its kernel as the real block
 * matrices [L/2][2 round_up(cin,32)][2 round_up(cout,32)] of the DFT domain; an element of them is one function of the dense
 * kernel and a table of L/2 x taps cosines and sines (csrc/spectral_weights.h: a double accumulator over the taps in ascending
 * order, every product and sum rounded on its own, one conversion to f32), which the host evaluates at creation and the two
 * repack passes of csrc/conv_repack.hip evaluate per element here, from the layer's device copy of the table.  So each buffer
 * holds exactly what xdet_spectral_conv_create would have made from the same values -- padding rows and columns +0, the sign of
 * a zero included -- and no array of the block matrices' size is allocated: the call needs the layer's own buffers only.
 * An activation exponent e the GEMM layer carries (a net's calibration) is honoured as by xdet_layers_refresh_device: the
 * epilogue scale ends as 2^-shift of the row times 2^e, exact.  scale_dev / shift_dev (f32 [cout] in device memory; NULL: kept)
 * replace the scale and shift of the inverse transform's epilogue, out = relu?(y * scale + shift); channels past cout stay +0.
 * Two passes over the bins on `stream` (and one small launch for scale / shift), no synchronisation, nothing read on the host.
 * Errors -> XDET_ERR_INVALID_ARG before any GPU work and with the layer unchanged: a NULL layer, a NULL kernel, a handle that
 * is not a spectral conv layer.  The shape is the layer's: the caller vouches for taps * cin * cout floats.  Afterwards the
 * GEMM layer's host copy of the epilogue scale is stale, as after xdet_conv_set_kernel_device (a net brings it back in line in
 * xdet_net_refresh_heads). */
int xdet_spectral_conv_set_kernel_device(void* layer, const float* kernel_dev, const float* scale_dev, const float* shift_dev,
                                         void* stream);
/* The same for a depthwise layer (xdet_depthwise_create): its taps [9][round_up(C,32)] from a dense f32 [3,3,C,1] kernel in
 * device memory, padding channels +0.  Errors: a NULL kernel, a layer whose taps carry an activation pre-scale. */
int xdet_depthwise_set_kernel_device(void* layer, const float* k33c1_dev, void* stream);
/* The inference fold of a batch norm on the device (csrc/conv_repack.hip): f32 arrays of C floats in device memory, bias NULL
 * or C floats, no synchronisation.  Per channel, every operation an f32 operation rounded on its own (no fused multiply-add,
 * correctly rounded division and square root), in the order of the host fold a net is built with:
 *     sc    = gamma / sqrtf(moving_variance + eps)
 *     shift = (beta - moving_mean * sc) + (bias ? bias * sc : 0.f)
 * The + 0.f of a fold without bias is kept: it turns a -0 shift into +0, as on the host.  The NumPy statement of the same
 * contract is xdet.ops.host_bn_fold, and the call equals it bit for bit.  Errors: a NULL array (bias excepted), C <= 0. */
int xdet_bn_fold(const float* gamma, const float* beta, const float* moving_mean, const float* moving_variance,
                 const float* bias_or_null, float eps, int C, float* scale_out, float* shift_out, void* stream);
/* The repack of xdet_conv_set_kernel_device / xdet_depthwise_set_kernel_device over a table of layers, in a number of launches
 * that does not depend on the table's length: one clear of the row maxima, one maxima pass and one repack pass over all conv
 * slots, one pass over all depthwise slots (a pass without slots is left out), behind one upload of the slot descriptors and
 * the tile -> slot tables, which are built here.  The per-tile device code is the per-layer doors' own, so a layer refreshed
 * here holds the bits they, and a creation from the same values, would give it.  A slot is one conv layer (xdet_conv_create,
 * or owned by a net) or one depthwise layer; all pointers are device memory.  kernel: as for the per-layer doors.  scale
 * (f32 [cout], conv slots only; NULL: the creation-time epilogue scale is kept) replaces the epilogue scale the layer was
 * created with -- in the split-precision modes the one in front of the rows' pre-scale, in f32 mode the scale itself.
 * shift (f32 [cout], conv slots only; NULL: kept) replaces the epilogue shift.  Layers of different precisions, with or
 * without the x8 copy, may share a table.
 * Unlike the per-layer doors, the table door honours what a net-owned or calibrated layer carries: a conv layer with an
 * activation exponent e ends with the epilogue scale creation plus that exponent would have left (the rescaled scale times
 * 2^e, exact); a depthwise layer with an output exponent e gets its taps times 2^-e; a planes affine that comes from the
 * layer's own output exponent alone is kept.  Refused: a layer whose planes copy carries a folded batch norm, a grouped
 * layer, a spectral layer -- each by name of the reason.
 * The call does not synchronise; the layers' host copies of the scale and of the taps are stale afterwards, as after the
 * per-layer doors.  workspace: xdet_layers_refresh_workspace_bytes(slots, n) bytes of device memory (0 for a table the call
 * refuses); it needs no initialisation and may be larger; a call behind a call on the same stream may reuse it.
 * Errors -> XDET_ERR_INVALID_ARG before any GPU work and with no layer touched: a NULL or empty table, a NULL layer or
 * kernel, a layer listed twice, a refused layer kind, a scale or shift on a depthwise slot, a NULL workspace. */
typedef struct {
  void* layer;
  const float* kernel;
  const float* scale;
  const float* shift;
} xdet_layer_refresh;
size_t xdet_layers_refresh_workspace_bytes(const xdet_layer_refresh* slots_host, int n);
int xdet_layers_refresh_device(const xdet_layer_refresh* slots_host, int n, void* workspace, void* stream);
/* The pack op of the training step (csrc/weight_pack.hip): dense f32 tensors in device memory written side by side into a
 * merged one, and back.  A slot is a merged tensor [outer, W] with W = the sum of its parts' widths, and 1 to 4 dense parts
 * [outer, width_p]; with off_p = the sum of the widths in front of part p,
 *     xdet_tensors_concat:   merged[o, off_p + c] = part_p[o, c]       for o < outer, c < width_p
 *     xdet_tensors_split:    part_p[o, c] = merged[o, off_p + c]
 * -- copies, no arithmetic: every bit pattern (NaN payloads, -0, denormals) arrives as it left, and the NumPy statements
 * xdet.ops.host_concat / host_split equal the calls bit for bit.  This is every merge a plan does on the host when it is built:
 * the large-separable block's K_a (outer 15 * cin, widths mid | mid), K_b (outer 15, widths mid * co | mid * co) and b_a (outer
 * 1), the RPN's conv2d_1 | conv2d_2 (outer 512, widths 2A | 4A; their biases at outer 1) and the head's fc_cls | fc_loc (outer
 * 2048, widths nc | 4); split is the adjoint, which takes the gradients of the merged tensors apart.  Slots are independent:
 * two split slots may read one merged tensor (the gradient of a sum b0 + b1 goes to both addends).
 * One launch serves the whole table: every part's dense element space is cut into runs of 4096 consecutive elements, one
 * workgroup per run; the part and run tables are built here and uploaded into the workspace, as xdet_momentum_step does.  A
 * part moves in 16-byte accesses when its width, its offset and (for outer > 1) W are multiples of 4 and both base pointers
 * are 16-byte aligned, and in dwords otherwise.  Plain vector stores, no atomics; the call does not synchronise.
 * workspace: xdet_tensors_concat_workspace_bytes / _split_workspace_bytes(slots, n_slots) bytes of device memory (the same
 *   figure; 0 for a table the calls refuse); it needs no initialisation and may be larger; a call behind a call on the same
 *   stream may reuse it.  Limits: at most 65536 slots, 2^22 runs, outer * W below 2^31 per slot.
 * Errors -> XDET_ERR_INVALID_ARG before any GPU work, never a skipped slot: a NULL or empty table, a NULL merged or part
 *   pointer, outer <= 0, a width <= 0, n_parts outside 1..4, a NULL workspace, a table beyond the limits. */
typedef struct {
  float* merged;
  int outer;
  int n_parts;
  float* part[4];
  int width[4];
} xdet_pack_slot;
size_t xdet_tensors_concat_workspace_bytes(const xdet_pack_slot* slots_host, int n_slots);
size_t xdet_tensors_split_workspace_bytes(const xdet_pack_slot* slots_host, int n_slots);
int xdet_tensors_concat(const xdet_pack_slot* slots_host, int n_slots, void* workspace, void* stream);
int xdet_tensors_split(const xdet_pack_slot* slots_host, int n_slots, void* workspace, void* stream);

/* ---- the checkpoint op (csrc/crc32c.hip): checksum, and optionally copy, a table of device buffers in one pass --------------
 * For every slot i, crc_out_dev[i] = the CRC-32C of src[0 .. bytes): Castagnoli, reflected polynomial 0x82f63b78, initial
 * register and final xor 0xffffffff, UNMASKED -- exactly what xdet.tf_checkpoint.crc32c(bytes) returns (the NumPy statement;
 * a TensorFlow bundle stores mask_crc of it).  bytes == 0 gives 0 and touches neither src nor dst.
 * Where dst is not NULL, dst[0 .. bytes) receives the same bytes in the same pass: every source byte is read once, no bit is
 * changed (NaN payloads, -0 and denormals arrive as they left), and no byte outside [dst, dst + bytes) is written (a byte
 * tail is stored as bytes).  Slots with and without dst may share a table; src and dst of a slot must not overlap.
 * Pointers must be 4-byte aligned; any length is allowed.  A slot whose src and dst (where given) are both 16-byte aligned
 * moves in 16-byte accesses, every other one in dwords.
 * Two launches serve the whole table, whatever the number of slots: a slot is cut into chunks of xdet_crc32c_chunk_bytes() =
 * 32768 bytes (256 lanes x 128 bytes; a slot's last chunk is short, chunks never cross a slot), one workgroup per chunk
 * writes the chunk's raw register into the workspace, combining its lanes through the CRC's linearity; then one workgroup per
 * slot folds the slot's registers as a tree with powers x^(8n) mod P that are computed here on the host and uploaded with the
 * slot table, as xdet_momentum_step uploads its tables.  Integer arithmetic only: no atomics, no fence, no workgroup waits
 * for another, and the call does not synchronise.
 * workspace: xdet_crc32c_workspace_bytes(slots, n_slots) bytes of device memory (0 for a table the call refuses); it needs no
 *   initialisation and may be larger; a call behind a call on the same stream may reuse it.
 * Limits: at most 65536 slots and 2^22 chunks (128 GiB) per table.
 * Errors -> XDET_ERR_INVALID_ARG before any GPU work: a NULL or empty table, a NULL src with bytes > 0, a src or dst that is
 *   not 4-byte aligned, a NULL (or misaligned) crc_out_dev, a NULL workspace, a table beyond the limits. */
typedef struct {
  const void* src;
  void* dst;
  size_t bytes;
} xdet_crc_slot;
size_t xdet_crc32c_chunk_bytes(void);
size_t xdet_crc32c_workspace_bytes(const xdet_crc_slot* slots_host, int n_slots);
int xdet_crc32c(const xdet_crc_slot* slots_host, int n_slots, uint32_t* crc_out_dev, void* workspace, void* stream);

/* ---- the gradient average of data-parallel training (csrc/grad_average.hip; the exchange itself is
 * xdet_comm_average_gradients in csrc/comm.hip): every rank's gradients become the rank-ordered mean, ahead of the step ------
 * A slot is one dense f32 gradient of n elements in device memory, updated in place.  The table is the same on every rank.
 * Flat element space: slot i occupies [o_i, o_i + n_i) with o_0 = 0 and o_{i+1} = o_i + round_up(n_i, 4); the elements between
 * a slot's end and the next slot's start are padding: +0 in a packed buffer, never written back.  T = o_last +
 * round_up(n_last, 4).  A chunk is chunk_elems consecutive flat elements, chunk c = [c * chunk_elems, min((c + 1) *
 * chunk_elems, T)); chunk_elems is a positive multiple of 1024 and at most 2^24 (chunk_elems * 4 bytes <= 64 MiB: the unit one
 * collective moves per rank); the last chunk is short, and every chunk's length is a multiple of 4.  Both sides of every copy
 * are then 16-byte aligned whenever the slot's pointer is: accesses are 128-bit wide in such a slot and scalar otherwise.
 * Per element, with g[r] the element in rank r's slab, every operation an f32 operation rounded on its own (denormals and
 * signed zeros kept, NaN and inf propagate):
 *     s = g[0];  for r = 1 .. world-1:  s = s + g[r];   out = s / (float)world
 * -- the NumPy statement of the same contract is xdet.ops.host_average_gradients, and the calls equal it bit for bit: the sum
 * runs in rank order on every rank, so every rank ends with the same bits whatever the transport did.
 * xdet_grad_pack: chunk `chunk` of this rank's flat space -> flat_out (f32 [len(chunk)], device memory, 16-byte aligned).
 * xdet_grad_reduce_ranks: gathered (f32 [world][len(chunk)], rank-major, device memory, 16-byte aligned) -> the statement
 *   above, written into the slots' own memory for the elements of that chunk; no other element of a slot is touched.  No
 *   communicator is involved: any world >= 1 runs in one process.
 * Both are one launch, one workgroup per run of 4096 flat elements of the chunk; the slot table and the map from runs to
 * slots are built here and uploaded into the workspace per call, as xdet_momentum_step does.
 * workspace: xdet_grad_average_workspace_bytes(slots, n_slots, world, chunk_elems) bytes of device memory (0 for a table the
 *   calls refuse): the two tables and, for world > 1, one packed chunk and `world` gathered chunks, which
 *   xdet_comm_average_gradients carves from it (the two doors above are handed theirs and use the tables only).  It needs no
 *   initialisation and may be larger; calls on one stream may reuse it.  Nothing synchronises.
 * xdet_comm_average_gradients: the whole exchange.  The communicator's stream waits for an event recorded on `stream` (the
 *   stream the backward ran on); per chunk, on the communicator's stream: pack, ncclAllGather(flat -> gathered, ncclFloat),
 *   reduce; then ev_done is recorded and `stream` waits for it, so whatever the caller enqueues on `stream` next (the optimizer
 *   step) sees the averaged gradients.  No host synchronisation: xdet_comm_wait(comm, NULL) is the host wait under the
 *   watchdog.  world == 1 issues no collective and no launch and leaves the gradients' bits alone.
 * Limits: at most 65536 slots and 2^22 runs.  Errors -> XDET_ERR_INVALID_ARG before any GPU work, never a skipped slot: a NULL
 *   or empty table, a slot with a NULL pointer or n <= 0, chunk_elems that is not a positive multiple of 1024 or is above 2^24,
 *   a chunk index outside the flat space, a NULL workspace, a NULL or misaligned flat_out / gathered, world < 1, a table beyond
 *   the limits.  A communicator the watchdog aborted -> XDET_ERR_STATE, as for the other collectives. */
typedef struct {
  float* grad;
  int64_t n;
} xdet_grad_slot;
size_t xdet_grad_average_workspace_bytes(const xdet_grad_slot* slots_host, int n_slots, int world, int64_t chunk_elems);
int xdet_grad_pack(const xdet_grad_slot* slots_host, int n_slots, int64_t chunk, int64_t chunk_elems, float* flat_out,
                   void* workspace, void* stream);
int xdet_grad_reduce_ranks(const xdet_grad_slot* slots_host, int n_slots, int64_t chunk, int64_t chunk_elems,
                           const float* gathered, int world, void* workspace, void* stream);
int xdet_comm_average_gradients(void* comm, const xdet_grad_slot* slots_host, int n_slots, int64_t chunk_elems, void* workspace,
                                void* stream);

/* ---- the model: lighr_head_model_fn in eval mode (light_head_rfcn_eval.py:364-433) -------
 * Weights enter by TF variable name (scope prefix stripped), TF layouts (HWIO / [in,out]). */
typedef struct {
  int image_size;         /* train_image_size, 480 */
  int max_batch;          /* workspace is sized for this many images per call */
  int num_classes;        /* 21 */
  int num_anchors;        /* 22 */
  int rpn_pre_nms_top_n;  /* 5000 */
  int rpn_post_nms_top_n; /* 1000 (300 in BASELINE config 3) */
  float rpn_nms_thres;    /* 0.7 */
  float rpn_min_size;     /* 16/480 */
  float select_threshold; /* 0.01 */
  float nms_threshold;    /* 0.3 */
  int nms_topk;           /* 200 */
  int grid;               /* 7 */
  int bank;               /* 10 */
} xdet_lighthead_config;

int xdet_net_create(void** net, const xdet_lighthead_config* cfg);
int xdet_net_set_weight(void* net, const char* name, const float* data_host, int ndim, const int64_t* dims);
/* options, before xdet_net_build:
 *   "large_sep" = "auto" | "direct" | "spectral": arithmetic form of large_sep_kernel (net/xception_body.py:450-475).
 *   direct = the (15,1)/(1,15) convs as implicit GEMMs; spectral = the same linear maps evaluated in the DFT
 *   domain of the convolved axis (one GEMM per frequency bin, ~5x fewer MFMA FLOPs; needs a split-precision
 *   mode and a 16/30/50 feature map); auto = spectral whenever those hold, else direct.
 *   The choice is per net, never per call: results do not depend on the batch an image arrives in.
 *   "spectral_refresh" = "off" | "on": a net whose block is in the spectral form keeps pointers to its two spectral layers, and
 *   xdet_net_refresh_heads takes the large_sep_feature group through xdet_spectral_conv_set_kernel_device (on), or refuses
 *   that group on such a net (off, the default).  No effect on a net in the direct form, and none on any forward.
 *   "sepconv" = "fused" | "split": entry-flow separable blocks as one kernel (default) or depthwise + pointwise.
 *   "rpn_stream" = "side" | "main": the RPN / proposal branch forks onto a side stream under the large-separable
 *   convs (default) or stays on the caller's stream (per-kernel profiles without cross-stream sharing).
 *   "conv3x3" = "patch" | "gemm": block1_conv2 on the staged-tile kernel (default) or the implicit-GEMM kernel.
 *   "pool" = "split" | "whole" | "split_all": the horizontal half of the block2 / block3 max-pools in the producing
 *   block's epilogue (default) or the whole pool as its own kernel.
 *   "ksplit" = "on" | "off" | "all": the 2048 -> 25 head GEMM (a single image: 3 tiles against 64 K steps) on the fixed
 *   split-K kernel (on, the default; a layer constant: results identical at every batch size), nothing (off), or the RPN
 *   3x3 conv as well (all: 32 tiles against 207 K steps; faster for one image, 0.9 % slower at bench-size batches).
 *   "workspace" = "reuse" | "ssa" | "poison": see xdet_net_memory.
 *   "pool_sub" = "on" | "off": the vertical pool pass of blocks 2-3 also writes the split planes of the raw subsampled sum (the
 *   next block's 1x1 / stride-2 projection reads those) and stores the sum as relu(sum) (its first separable conv reads that)
 *   -- on (default) -- or leaves both to their own passes (off; the same values either way).
 *   "check_range" = "off" | "on": after each forward validate everything that is turned into f16 against the f16 range --
 *   every split plane (no inf / NaN in the hi plane; the planes hold x * 2^-e after xdet_net_calibrate), the f32 input
 *   of a register-split conv (|x| <= 65504) and of a fused separable block (relu?(x) * sum|taps| * 2^-e <= 65504) -- and
 *   every other activation tensor for NaN / inf; a violation marks the image's detection scores NaN (slot 0 of every
 *   class), as a non-finite RPN score or head logit always does.  A diagnostic for new checkpoints: the pass re-reads
 *   all activations.
 *   "pool_index" = "off" | "keep": the head's PsRoiAlign also writes its argmax sample ids into an i32 buffer
 *   [max_batch * R, C] (ld of "pooled"; xdet_net_buffer "pool_index"), which xdet_net_head_pool_backward needs.  off
 *   (default): the forward is the same call as ever and the buffer does not exist.
 *   "rpn_hidden" = "off" | "keep": rpn_head/conv2d (net/xception_body.py:384) also writes its output after the ReLU as an
 *   f32 tensor [max_batch, h, w, 512] (xdet_net_buffer "rpn_hidden"), the ReLU mask and dense-layer input of the RPN head's
 *   backward (xdet_dense_backward, then xdet_conv_backward).  off (default): the conv writes the split planes its 1x1
 *   heads read and nothing else, and the name is refused.  "rpn_out" has the same bits either way.
 *   "entry_x" = "off" | "keep": block 4's sum -- the input of the middle flow (net/xception_body.py:328), f32, in front of
 *   block5's ReLU -- stays a named buffer [max_batch, h, w, 728] (xdet_net_buffer "entry_x") instead of going back to the
 *   workspace pool when block 5 has read it: what a training-mode middle flow starts from.  off (default): the plan, the
 *   kernels and their arguments are the same as ever and the name is refused.  keep: every tensor of the forward has the same
 *   bits; only addresses inside the workspace move.
 *   "stem_out" = "off" | "keep": the output of block1_conv2 + BN + ReLU -- the input of the entry flow's block 2
 *   (net/xception_body.py:260), f32 in every plan -- stays a named buffer [max_batch, h, w, 64] (xdet_net_buffer "stem_out")
 *   instead of going back to the workspace pool when block 2 has read it: what a training-mode entry flow starts from.  off
 *   (default): the plan, the kernels and their arguments are the same as ever and the name is refused.  keep: every tensor of
 *   the forward has the same bits; only addresses inside the workspace move.
 *   "head_rois" = "off" | "<P>", a whole number in 1..rpn_post_nms_top_n (anything else: XDET_ERR_INVALID_ARG, naming the
 *   option): the head stage of a TRAINING net.  The reference proposes rpn_post_nms_top_n ROIs per image, samples P of them
 *   and runs PsRoiAlign, the head and its backward on those (light_head_rfcn_train.py:86-112, net/xception_body.py:446-448,
 *   502-533).  With P the head stage -- "pooled", "fc", "cls_reg" and, with "pool_index" = "keep", "pool_index" -- is planned
 *   on P rows per image instead of rpn_post_nms_top_n, with the same layers and constants: the plan a net created with
 *   rpn_post_nms_top_n = P has.  The proposal stage keeps rpn_post_nms_top_n ("proposals", xdet_net_get_proposals and its
 *   workspace).  The sampled ROIs live in a new buffer, xdet_net_buffer "head_rois": f32 [max_batch, P, 4] corner boxes in
 *   the layout of "proposals", written by the caller (a device-to-device copy of what xdet_encode_rois left); xdet_net_get_head
 *   and xdet_net_head_pool_backward read it in place of "proposals".  Such a net has no eval tail: xdet_net_forward,
 *   xdet_net_forward_u8, xdet_net_calibrate (which runs whole forwards), xdet_net_head_decode and xdet_net_bboxes_eval return
 *   XDET_ERR_STATE with a sentence that names head_rois, ahead of any launch and of a graph capture.  The refresh doors
 *   (xdet_net_refresh_weights / _heads / _stem) do not depend on the row count and work as ever.  off (default): the net as
 *   ever, byte for byte, and the buffer name is refused.  No kernel belongs to the option: PsRoiAlign, its ordered gradient
 *   and the dense layers take the row count as an argument.
 *   "eval_head" = "off" | "on" (on needs "head_rois" = "<P>": without it xdet_net_build returns XDET_ERR_INVALID_ARG with one
 *   sentence): a second head stage on such a training net, so that the net that trains also evaluates.  It is built on the
 *   SAME two dense layers as the sampled-row stage (what xdet_net_refresh_heads refreshes, it refreshes for both) over its
 *   own buffers "pooled_eval", "fc_eval", "cls_reg_eval" with rpn_post_nms_top_n rows per image: the head plan of a net built
 *   with rpn_post_nms_top_n = R and no head_rois, and the same bits.  xdet_net_forward and xdet_net_forward_u8 (eager and
 *   captured) then run on it: PsRoiAlign from "proposals" into "pooled_eval" (no pool_index), the eval stage, the decode from
 *   "cls_reg_eval" and bboxes_eval (the wide form when rpn_post_nms_top_n > 1024).  They overwrite the body's and the RPN's
 *   buffers and "proposals", and leave "pooled", "fc", "cls_reg", "pool_index" and "head_rois" alone.  The stage entries
 *   xdet_net_head_decode and xdet_net_bboxes_eval (the logits form) stay XDET_ERR_STATE, and so does xdet_net_calibrate, by a
 *   sentence that says why: the training stages and the refresh doors of such a net are built at exponent 0, and a second
 *   input plane on a shared layer has no pre-scale hook.  off (default): the head_rois net as described above, byte for
 *   byte, and the three buffer names are refused. */
int xdet_net_set_option(void* net, const char* key, const char* value);
int xdet_net_build(void* net);     /* folds BN, transposes/pads weights, allocates the workspace */
int xdet_net_destroy(void* net);
/* named workspace buffers (views, owned by the net): "mid","out","rpn_out","feat","objectness",
 * "rpn_boxes","proposals","pooled","fc","cls_reg","head_boxes","prop_counts"; "pool_index" (i32, dims / ld of "pooled")
 * with option "pool_index" = "keep" only, "rpn_hidden" (f32 [max_batch,h,w,512]) with option "rpn_hidden" = "keep" only,
 * "entry_x" (f32 [max_batch,h,w,728]) with option "entry_x" = "keep" only, "stem_out" (f32 [max_batch,h,w,64]) with option
 * "stem_out" = "keep" only, "head_rois" (f32 [max_batch,P,1,4], ld 4) with option "head_rois" = "<P>" only, otherwise
 * XDET_ERR_INVALID_ARG; "mid_x" is "mid" in front of its ReLU.  With "head_rois" = "<P>" the buffers "pooled", "fc", "cls_reg"
 * and "pool_index" have P rows per image, "proposals" and "head_boxes" rpn_post_nms_top_n; "pooled_eval", "fc_eval" and
 * "cls_reg_eval" (rpn_post_nms_top_n rows per image, the dims / ld a net without head_rois has for "pooled", "fc", "cls_reg")
 * with option "eval_head" = "on" only, otherwise XDET_ERR_INVALID_ARG */
int xdet_net_buffer(void* net, const char* name, void** dptr, int64_t dims[4], int* ld);
/* stage entry points = the reference's graph-builder functions (net/xception_body.py) */
int xdet_net_xception_body(void* net, const float* images_nchw, int N, void* stream);  /* :236 -> "mid","out" */
int xdet_net_get_rpn(void* net, int N, void* stream);                                  /* :381 -> "rpn_out" */
/* "mid_x" was rewritten from outside the net (a training-mode middle flow): re-derive from the f32 "mid_x" of the first N
 * images everything else the net keeps of that tensor -- the ReLU split planes rpn_head/conv2d reads (block12_sepconv3's
 * epilogue wrote them; here xdet_split_f32's pass with relu = 1 at the planes' own pre-scale, the same bits on finite data)
 * and the "mid" buffer (ReLU(mid_x)).  A net in f32 precision has no planes: only the copy runs.  On `stream`, without a
 * synchronisation or a host read.  XDET_ERR_INVALID_ARG for N outside 1..max_batch. */
int xdet_net_mid_refresh(void* net, int N, void* stream);
int xdet_net_large_sep(void* net, int N, void* stream);                                /* :450 -> "feat" */
int xdet_net_rpn_decode(void* net, int N, void* stream);                               /* -> "objectness","rpn_boxes" */
int xdet_net_get_proposals(void* net, int N, void* stream);                            /* :402 -> "proposals" */
int xdet_net_get_head(void* net, int N, void* stream);                                 /* :477 -> "cls_reg" */
int xdet_net_head_decode(void* net, int N, void* stream);                              /* -> "head_boxes" */
/* (xdet_net_get_head reads "proposals", rpn_post_nms_top_n rows per image -- or, on a net built with "head_rois" = "<P>",
 * the "head_rois" buffer with P rows; xdet_net_head_decode and xdet_net_bboxes_eval are XDET_ERR_STATE on such a net.) */
/* The head's pooling backward: d loss / d pooled (device, [N*R, ld], first C = grid*grid*bank entries of a row; R = P on a
 * net built with "head_rois" = "<P>") -> d loss / d feat, by xdet_psroialign_grad_ordered on the net's own "proposals"
 * ("head_rois" on such a net; corner boxes), the "pool_index" the last xdet_net_get_head kept, cfg.grid and 'max'.  d_feat: [N, feat.H, feat.W, feat.ld], the layout of the "feat" buffer,
 * every element written (padding channels zero).  XDET_ERR_STATE for a net built with "pool_index" = "off". */
int xdet_net_head_pool_backward(void* net, int N, const float* d_pooled, int ld, float* d_feat, void* stream);
int xdet_net_bboxes_eval(void* net, int N, const int* image_shapes, const float* bbox_img, float* det_scores,
                         float* det_boxes, void* stream);
/* whole forward: images f32 [N,3,S,S] -> det_scores [N,20,topk], det_boxes [N,20,topk,4].
 * image_shapes / bbox_img may be NULL (S x S, [0,0,1,1]).  use_graph != 0 replays a hipGraph
 * of the whole forward.  A graph bakes in every pointer it was captured with, so graphs are cached
 * per argument tuple (N, images, image_shapes, bbox_img, det_scores, det_boxes): the first call with a
 * new tuple captures (and runs) a new graph, later calls with the same tuple replay it; at most 8
 * graphs are kept per net (oldest evicted).  The CONTENTS of the buffers may change between replays,
 * the buffers themselves must stay allocated while their graph is cached.
 * xdet_net_graph_count: number of graphs currently cached (tests).
 * rpn_post_nms_top_n up to 6144: above 1024 ROIs per image the tail is bboxes_eval's wide form (xdet_bboxes_eval_probs_wide);
 * up to 1024 no launch and no argument differs.  On a net built with "head_rois" = "<P>" the forward needs "eval_head" = "on"
 * and runs that stage (XDET_ERR_STATE without). */
int xdet_net_forward(void* net, const float* images_nchw, int N, const int* image_shapes, const float* bbox_img,
                     float* det_scores, float* det_boxes, int use_graph, void* stream);
/* uint8 ingest + whole forward: xdet_preprocess_eval_batch (out_size = the net's S) into images_nchw / bbox_img, then
 * xdet_net_forward with image_shapes and bbox_img, so detections are filtered with each image's original shape
 * (light_head_rfcn_eval.py:277,369,412) and come back relative to the original image (bboxes_resize).  All buffers are
 * the caller's.  use_graph != 0: ingest and forward are ONE graph, cached per argument tuple (N, packed, packed_bytes,
 * offsets, image_shapes, resize, images_nchw, bbox_img, det_scores, det_boxes); the image sizes and offsets are buffer
 * contents, so a replay may carry a batch of other sizes as long as it fits in packed_bytes. */
int xdet_net_forward_u8(void* net, const uint8_t* packed, int64_t packed_bytes, const int64_t* offsets,
                        const int32_t* image_shapes, int N, int resize, float* images_nchw, float* bbox_img,
                        float* det_scores, float* det_boxes, int use_graph, void* stream);
/* Activation pre-scale of the split-precision operands (modes 1 / 2).  An f16 hi part overflows beyond 65504 while the
 * reference computes in f32 everywhere and has BN-less edges (net/xception_body.py:381-400,450-475).  Every tensor that
 * is split into f16 planes carries a power-of-two exponent e: the planes hold x * 2^-e and the consuming contraction
 * folds 2^e back into its epilogue scale -- both exact.  xdet_net_calibrate runs the forward on `images` (device,
 * [N,3,S,S]) until no operand exceeds 4096 (16x headroom) and reports how many tensors got e != 0; a net whose
 * activations are small keeps every exponent at 0 and its results bit for bit.  Cached graphs are dropped.
 * xdet_net_plane_scales / _name: the exponents and what they belong to (exps may be NULL to query the count). */
int xdet_net_calibrate(void* net, const float* images_nchw, int N, int* n_scaled, void* stream);
int xdet_net_plane_scales(void* net, int max_n, int* n_out, int* exps);
int xdet_net_plane_scale_name(void* net, int idx, char* buf, int buflen);
/* option "cross" = "fp8": how many split-precision tensors are in the x8 form (fp8 copies for the cross terms; see
 * xdet_conv_forward_planes_x8) -- 0 until xdet_net_calibrate has measured them, then the 28 depthwise -> pointwise edges of
 * the light-head net (net/xception_body.py:220-234, blocks 5-14). */
int xdet_net_x8_planes(void* net, int* n_on);
int xdet_net_graph_count(void* net, int* count);
/* Refresh the built net's body from trained weights in device memory: names are the checkpoint's, data dense f32 in the
 * checkpoint's shapes.  The reach is the body's blocks 2-14 -- the 72 layers of the entry, middle and exit flows (38 convs, 34
 * depthwise), 148 variables and the 76 moving statistics of their 38 batch norms.  A layer group is refreshed only whole: a
 * unit is <u>/depthwise_kernel, <u>/pointwise_kernel and <u>_bn/{gamma, beta, moving_mean, moving_variance}; a projection is
 * <conv>/kernel and the four arrays of its batch norm.  Any set of whole groups is allowed.
 * The call folds every group's batch norm with xdet_bn_fold into scratch the net owns (one block, allocated at the first refresh: xdet_net_memory then reports it), runs one
 * xdet_layers_refresh_device table over all touched layers on `stream`, synchronises, and brings the host side back in line:
 * every touched layer's host copy of the epilogue scale (at exponent 0) and of the depthwise taps is read back and the layers
 * accept an activation exponent again (xdet_net_calibrate works as on a freshly built net); the range bound of a fused
 * separable block's depthwise result is recomputed from the new taps; a host copy of a weight the net still holds is updated.
 * Every exponent the plan holds is kept, and no pointer or scalar baked into a captured graph changes: xdet_net_graph_count is
 * unchanged and a replayed graph computes with the new weights.  The stem, the RPN head, the large-separable block, the head
 * and the detection tail are untouched.
 * Errors -> XDET_ERR_INVALID_ARG, by name, before any GPU work and with the net unchanged: a name outside the reach (the stem's
 * block1_ layers, rpn_head, large_sep_feature, final_head, anything unknown), a group given in part, a name given twice, a NULL
 * pointer, an empty table, a net that is not built. */
typedef struct {
  const char* name;
  const float* data;
} xdet_net_weight_dev;
int xdet_net_refresh_weights(void* net, const xdet_net_weight_dev* table_host, int n, void* stream);
/* The same for the layers the plan itself owns, outside xdet_net_refresh_weights' reach: the same table, three groups, each
 * taken whole only --
 *   rpn_head:          rpn_head/{conv2d, conv2d_1, conv2d_2}/{kernel, bias}: the 3x3 conv's layer from its kernel and bias,
 *                      the fused 1x1 layer "rpn_head/conv2d_1+2" from conv2d_1 | conv2d_2 side by side (kernels and biases);
 *   final_head:        final_head/{subnet_fc, fc_cls, fc_loc}/{kernel, bias}: "final_head/subnet_fc", and "fc_cls+fc_loc" from
 *                      fc_cls | fc_loc side by side (a split-K layer: it reads the same K-blocked operand copies);
 *   large_sep_feature: the eight conv tensors of Branch_0 and Branch_1 and batch_normalization/{gamma, beta, moving_mean,
 *                      moving_variance}: the branches merged as the plan merges them when it is built (K_a, b_a, K_b), the
 *                      bias b0 + b1 (xdet_add_rows on one row), xdet_bn_fold with eps 1e-5 and that bias, then the two
 *                      direct-form layers -- or, on a net in the spectral form built with the option spectral_refresh=on, the
 *                      same merges, sum and fold into the same scratch, then xdet_spectral_conv_set_kernel_device on the
 *                      (15,1) layer with K_a and shift b_a and on the (1,15) layer with K_b and the folded scale and shift,
 *                      each at its GEMM layer's own activation exponent.
 * The merges are one xdet_tensors_concat table into scratch the net owns (one block at the first call: the two table doors'
 * workspaces and every merged tensor but the large-separable kernels, which are a second block at the first call that names
 * that group; xdet_net_memory reports both), then one xdet_layers_refresh_device table over the touched layers on `stream`,
 * one synchronisation, and the host bookkeeping of xdet_net_refresh_weights: every touched layer's host copy of the epilogue
 * scale is read back (of a spectral layer's GEMM layer: every bin's rows) and the layers accept an activation exponent again.
 * Exponents and captured graphs stay.
 * Errors -> XDET_ERR_INVALID_ARG, by name, before any GPU work and with no layer touched: a name outside the three groups (the
 * body's variables among them), a group given in part, a name given twice, a NULL pointer, an empty table, a net that is not
 * built, and a large_sep_feature group on a net whose block is in the spectral form and that was built without the option
 * spectral_refresh=on (build it with that option, or with large_sep=direct). */
int xdet_net_refresh_heads(void* net, const xdet_net_weight_dev* table_host, int n, void* stream);
/* The same for the stem, the last layers outside the two doors above: the same table, two groups, each taken whole only --
 *   block1_conv1: block1_conv1/kernel [3,3,3,32] and block1_conv1_bn/{gamma, beta, moving_mean, moving_variance};
 *   block1_conv2: block1_conv2/kernel [3,3,32,64] and the four arrays of block1_conv2_bn.
 * block1_conv2 -- and block1_conv1 in a net built in f32 mode, where it is a conv layer -- goes xdet_net_refresh_weights' way:
 * xdet_bn_fold (eps 1e-4) into scratch the net owns (one block at the first call; xdet_net_memory reports it), a slot of one
 * xdet_layers_refresh_device table, one synchronisation, the layer's host copy of the epilogue scale read back.  In the
 * split-precision modes block1_conv1 is the kernel of xdet_stem_conv3x3s2_forward and no layer: its kernel is copied device to
 * device into the net's own array (the same layout), and the fold's scale and shift replace the net's host copies at exponent
 * 0 and are uploaded again times 2^-e, e the current exponent of the plane "block1_conv1 [stem]".  Exponents,
 * xdet_net_plane_scales and captured graphs stay; a replayed graph computes with the new weights.
 * Errors -> XDET_ERR_INVALID_ARG, by name, before any GPU work and with the net unchanged: a name outside the two groups, a
 * group given in part, a name given twice, a NULL pointer, an empty table, a net that is not built. */
int xdet_net_refresh_stem(void* net, const xdet_net_weight_dev* table_host, int n, void* stream);
/* Device memory of the net's workspace and weights in bytes (everything the plan allocated), and how many bytes of
 * tensors were placed into blocks recycled from dead tensors (option "workspace" = "reuse", the default: a builder hands a
 * tensor's block back once its last consumer is planned and a later tensor takes it over -- a planes tensor only a block
 * of exactly its own size, an f32 tensor the best-fitting free block of at most twice its size (NOT re-zeroed: what lies
 * behind the tensor, its 128-float loader slack included, is the predecessor's bytes; no consumer may use them, which
 * "poison" proves) -- the middle flow's 24 x 2 tensors live in a handful of blocks; "ssa": one block per tensor, which
 * option check_range selects by itself because its validation pass reads every tensor after the forward; "poison"
 * (tests): "reuse", with everything behind a recycled f32 tensor filled with NaN bits in front of its producer on every
 * forward -- the detections must still be those of "ssa", bit for bit).  The first xdet_net_refresh_weights adds its scratch
 * (one block: the table workspace for the whole reach and two floats per output channel) to allocated_bytes. */
int xdet_net_memory(void* net, size_t* allocated_bytes, size_t* recycled_bytes);
/* per-kernel accounting of the last build: total dense FLOPs (2*MAC, unpadded) of one image */
int xdet_net_flops_per_image(void* net, double* backbone, double* rpn, double* large_sep, double* head);

/* ---- per-op HIP-event timing (bench.py's roofline leg; the reference's counterpart is the
 * commented-out tf.train.ProfilerHook, light_head_rfcn_train.py:463,522) ---------------------
 * net_kind 0 = light-head net, 1 = resnet trunk.  While enabled every planned op (conv,
 * depthwise, pool ...) is bracketed by an event pair on the launch stream; xdet_profile_read
 * waits for them and returns per-op totals since the last read: ms, launch count and the
 * algorithmic dense FLOPs of one image (0 for non-MFMA ops). */
int xdet_profile_enable(void* net, int net_kind, int enable);
int xdet_profile_read(void* net, int net_kind, int max_ops, int* n_ops, double* ms, int* launches, double* flops);
int xdet_profile_op_name(void* net, int net_kind, int op, char* buf, int buflen);
/* per planned op: FLOPs it EXECUTES on the matrix cores per image (every split-precision product counted; less than
 * 3 x algorithmic for the spectral GEMMs, 0 for VALU ops).  A negative `flops` from xdet_profile_read marks an
 * auxiliary pass (DFT) of the contraction in front of / behind it. */
int xdet_profile_mfma_flops(void* net, int net_kind, int max_ops, int* n_ops, double* issued_flops_per_image);

/* ---- A13: ResNet-50 v2 trunk (net/resnet_v2.py:311-345), BASELINE config 2 --------------- */
int xdet_resnet_create(void** net, int image_size, int max_batch);
int xdet_resnet_set_weight(void* net, const char* name, const float* data_host, int ndim, const int64_t* dims);
/* Before xdet_resnet_build; every key takes "on" (default) | "off".  The off forms are the layer-by-layer plans the fused
 * kernels are tested against (tests/test_gpu_resnet_bneck.py: same bits, or f32 rounding for "projcat"):
 *   "bneck"     stage 1's identity blocks as one kernel (csrc/resnet_bneck.hip) | three launches per block
 *   "preconv"   a block's opening 1x1 conv makes its own pre-activation (csrc/resnet_preconv.hip) | a split pass + the conv
 *   "projcat"   a projection block's shortcut folded into its closing GEMM as extra K | projection GEMM + add
 *   "stem7"     the 7x7 / stride-2 stem conv from the NCHW image (csrc/resnet_stem.hip) | the implicit-GEMM kernel
 *   "stem_pool" the stem's max-pool writes the first block's pre-activation planes | pool, then a split pass
 *   "ksplit"    fixed split-K / one-range ring kernels for stages 2-4 at small batches | the plain kernels */
int xdet_resnet_set_option(void* net, const char* key, const char* value);
int xdet_resnet_build(void* net);
int xdet_resnet_forward(void* net, const float* images_nchw, int N, float* out_nhwc, void* stream);
/* the same forward as a replayed hipGraph (captured on the first call with a given (N, images, out) tuple; needs an
 * explicit stream; falls back to the eager form while per-op profiling is enabled) */
int xdet_resnet_forward_graph(void* net, const float* images_nchw, int N, float* out_nhwc, void* stream);
/* activation pre-scale of the trunk's split-precision operands, as xdet_net_calibrate (xdet_net_plane_scales / _name accept
 * a trunk handle too).  Handles are checked: an entry point given the other net type's handle returns XDET_ERR_INVALID_ARG. */
int xdet_resnet_calibrate(void* net, const float* images_nchw, int N, int* n_scaled, void* stream);
int xdet_resnet_out_shape(void* net, int* Ho, int* Wo, int* C);
int xdet_resnet_flops_per_image(void* net, double* flops);
int xdet_resnet_destroy(void* net);

/* ---- (e) multi-GPU: image-sharded ranks + ONE RCCL all-gather of detections per step ------
 * SURVEY.md 8e.  The reference has nothing to replace here (one tf.estimator session at batch 1,
 * light_head_rfcn_eval.py:212,466-499); BASELINE config 4 asks for this layer.  One process per GPU.
 * xdet_comm_init: call after xdet_set_device.  Rank 0 creates the ncclUniqueId and publishes it at
 *   unique_id_path (temporary name + rename); the other ranks poll for that file for up to timeout_s
 *   seconds (<= 0: 120), then every rank enters ncclCommInitRank.  world == 1 needs no path.
 *   librccl.so is bound by dlopen here, not at library load.
 * xdet_comm_allgather_detections: det_scores [B,C,K] + det_boxes [B,C,K,4] of this rank are packed
 *   into packed_local [B,C,K,5] (score | ymin xmin ymax xmax) and all-gathered into gathered
 *   [world*B,C,K,5] (rank-major).  Runs on the communicator's own stream: it first waits for the
 *   n_producers streams that write the det buffers, and makes those streams wait for the pack, so the
 *   caller may enqueue the next forward immediately -- the gather overlaps it.  No host sync.
 *   det_double_buffered != 0: the caller alternates between two det buffer pairs from call to call;
 *   the producers then only wait for the PREVIOUS call's pack (the one that read the pair they write
 *   next), which removes the once-per-step join of the producer streams.
 * xdet_comm_wait: stream != NULL -> that stream waits for the last gather; NULL -> the host does.
 * xdet_comm_allreduce_max / xdet_comm_barrier: scalar collectives for bench timing (host-synchronous).
 * xdet_comm_allgather_bytes: `bytes` (<= 1 MiB) of host memory from every rank -> world * bytes in rank order,
 *   moved by ncclAllGather on the communicator's stream (rank / device / PCI-bus-id records, per-rank rates).
 * Watchdog: every HOST wait on the communicator's stream (comm_wait(NULL), the scalar collectives, allgather_bytes,
 *   destroy) polls instead of blocking; when RCCL reports an asynchronous error or nothing completes for the
 *   timeout (XDET_COMM_TIMEOUT_S or xdet_comm_set_timeout, default 300 s: the length of ONE wait, so a caller whose
 *   peers legitimately take longer between two collectives raises it) the communicator is aborted
 *   (ncclCommAbort) and the call returns XDET_ERR_STATE, as does every later call -- a rank whose peer died exits
 *   with an error instead of hanging in hipStreamSynchronize.  Host buffers of the scalar / byte collectives are
 *   staged through pinned memory owned by the communicator, so no copy can block the host outside the watchdog.
 * Rank 0 removes a stale id file before it creates the id and removes its own once ncclCommInitRank has returned. */
int xdet_comm_init(void** comm, int rank, int world, const char* unique_id_path, int timeout_s);
int xdet_comm_destroy(void* comm);
int xdet_comm_info(void* comm, int* rank, int* world, int* device, int* rccl_version);
int xdet_pack_detections(const float* det_scores, const float* det_boxes, int64_t n_slots, float* packed, void* stream);
int xdet_comm_allgather_detections(void* comm, const float* det_scores, const float* det_boxes, int n_images,
                                   int n_fg_classes, int topk, float* packed_local, float* gathered,
                                   void* const* producer_streams, int n_producers, int det_double_buffered);
int xdet_comm_wait(void* comm, void* stream);
int xdet_comm_allreduce_max(void* comm, double* value_host);
int xdet_comm_barrier(void* comm);
int xdet_comm_allgather_bytes(void* comm, const void* send_host, void* recv_host, size_t bytes);
int xdet_comm_set_timeout(void* comm, double seconds);
/* which shared object the collective entry points were bound from (realpath of dladdr(ncclAllGather)), and whether it
 * was named by XDET_RCCL_LIB.  XDET_RCCL_LIB is honoured only together with XDET_ALLOW_RCCL_OVERRIDE=1 (the test double of
 * tests/fake_rccl, another RCCL build); otherwise xdet_comm_init fails with XDET_ERR_STATE: a bench never runs silently
 * on a stand-in.  Binds the library if no communicator exists yet. */
int xdet_comm_library(char* path_buf, int buflen, int* overridden);

#ifdef __cplusplus
}
#endif
#endif /* XDET_H_ */
