// The C ABI of include/xdet.h over the layer objects and the two plans.
#include "lighthead.h"
#include "resnet_trunk.h"

namespace xdet {

static thread_local std::string g_last_error;
void set_last_error(const std::string& s) { g_last_error = s; }
int hip_fail(hipError_t e, const char* what, const char* file, int line) {
  char buf[512];
  snprintf(buf, sizeof(buf), "HIP error %d (%s) at %s:%d: %s", (int)e, hipGetErrorString(e), file, line, what);
  g_last_error = buf;
  return XDET_ERR_HIP;
}

static inline hipStream_t S(void* s) { return reinterpret_cast<hipStream_t>(s); }

int g_default_precision = PREC_F32;

}  // namespace xdet

using namespace xdet;

extern "C" {

const char* xdet_last_error(void) { return g_last_error.c_str(); }
int xdet_version(void) { return 1; }
int xdet_device_count(int* n) { XDET_HIP(hipGetDeviceCount(n)); return XDET_OK; }
int xdet_set_device(int dev) { XDET_HIP(hipSetDevice(dev)); return XDET_OK; }
int xdet_device_pci_bus_id(int dev, char* buf, int buflen) {
  XDET_REQUIRE(buf && buflen >= 16, "device_pci_bus_id: need a buffer of >= 16 bytes");
  XDET_HIP(hipDeviceGetPCIBusId(buf, buflen, dev));
  return XDET_OK;
}
int xdet_probe_ipc(void) {
  DevMem<unsigned char> p;
  XDET_TRY(p.alloc(1 << 16));
  hipIpcMemHandle_t h;
  XDET_HIP(hipIpcGetMemHandle(&h, p));
  return XDET_OK;
}
int xdet_set_default_precision(int mode) {
  XDET_REQUIRE(mode == PREC_F32 || mode == PREC_F16X3 || mode == PREC_F16, "precision must be 0 (f32), 1 (f16x3) or 2 (f16)");
  g_default_precision = mode;
  return XDET_OK;
}
int xdet_get_default_precision(void) { return g_default_precision; }

int xdet_malloc(void** dptr, size_t bytes) { XDET_REQUIRE(dptr, "dptr is NULL"); XDET_HIP(hipMalloc(dptr, std::max<size_t>(bytes, 16))); return XDET_OK; }
int xdet_free(void* dptr) { if (dptr) XDET_HIP(hipFree(dptr)); return XDET_OK; }
int xdet_memset(void* dptr, int value, size_t bytes, void* stream) { XDET_HIP(hipMemsetAsync(dptr, value, bytes, S(stream))); return XDET_OK; }
int xdet_memcpy_h2d(void* dst, const void* src, size_t bytes, void* stream) { XDET_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, S(stream))); return XDET_OK; }
int xdet_memcpy_d2h(void* dst, const void* src, size_t bytes, void* stream) { XDET_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, S(stream))); XDET_HIP(hipStreamSynchronize(S(stream))); return XDET_OK; }
int xdet_memcpy_d2h_async(void* dst, const void* src, size_t bytes, void* stream) { XDET_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, S(stream))); return XDET_OK; }
int xdet_malloc_host(void** hptr, size_t bytes) { XDET_REQUIRE(hptr, "hptr is NULL"); XDET_HIP(hipHostMalloc(hptr, std::max<size_t>(bytes, 16), hipHostMallocDefault)); return XDET_OK; }
int xdet_free_host(void* hptr) { if (hptr) XDET_HIP(hipHostFree(hptr)); return XDET_OK; }
int xdet_memcpy_d2d(void* dst, const void* src, size_t bytes, void* stream) { XDET_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, S(stream))); return XDET_OK; }
int xdet_stream_create(void** stream) { hipStream_t s; XDET_HIP(hipStreamCreateWithFlags(&s, hipStreamNonBlocking)); *stream = s; return XDET_OK; }
int xdet_stream_destroy(void* stream) { XDET_HIP(hipStreamDestroy(S(stream))); return XDET_OK; }
int xdet_stream_sync(void* stream) { XDET_HIP(hipStreamSynchronize(S(stream))); return XDET_OK; }
int xdet_event_create(void** ev) { hipEvent_t e; XDET_HIP(hipEventCreate(&e)); *ev = e; return XDET_OK; }
int xdet_event_destroy(void* ev) { XDET_HIP(hipEventDestroy(reinterpret_cast<hipEvent_t>(ev))); return XDET_OK; }
int xdet_event_record(void* ev, void* stream) { XDET_HIP(hipEventRecord(reinterpret_cast<hipEvent_t>(ev), S(stream))); return XDET_OK; }
int xdet_event_sync(void* ev) { XDET_HIP(hipEventSynchronize(reinterpret_cast<hipEvent_t>(ev))); return XDET_OK; }
int xdet_event_elapsed_ms(void* a, void* b, float* ms) {
  XDET_HIP(hipEventSynchronize(reinterpret_cast<hipEvent_t>(b)));
  XDET_HIP(hipEventElapsedTime(ms, reinterpret_cast<hipEvent_t>(a), reinterpret_cast<hipEvent_t>(b)));
  return XDET_OK;
}

int xdet_psroialign_fwd(const float* feat, const float* rois, float* pooled, int32_t* index, int N, int C, int H,
                        int W, int R, int grid_w, int grid_h, int use_max, int feat_layout, int ldc, int out_ld,
                        int rois_are_corners, void* stream) {
  XDET_REQUIRE(feat && rois && pooled, "inputs/rois/pooled_features must not be NULL");
  return launch_psroialign(feat, rois, pooled, index, N, C, H, W, R, grid_w, grid_h, use_max, feat_layout,
                           feat_layout == 0 ? C : ldc, out_ld, rois_are_corners, S(stream));
}

int xdet_psroialign_grad(const float* rois, const float* grad_pooled, const int32_t* pooled_index, float* grad_feat,
                         int N, int C, int H, int W, int R, int grid_w, int grid_h, int use_max, int feat_layout,
                         int ldc, void* stream) {
  return launch_psroialign_grad(rois, grad_pooled, pooled_index, grad_feat, N, C, H, W, R, grid_w, grid_h, use_max,
                                feat_layout, feat_layout == 0 ? C : ldc, S(stream));
}

int xdet_psroialign_grad_ordered(const float* rois, const float* grad_pooled, int ld_grad, const int32_t* pooled_index,
                                 int ld_index, float* grad_feat, int N, int C, int H, int W, int R, int grid_w, int grid_h,
                                 int use_max, int feat_layout, int ldc, int rois_are_corners, void* stream) {
  return launch_psroialign_grad_ordered(rois, grad_pooled, ld_grad, pooled_index, ld_index, grad_feat, N, C, H, W, R, grid_w,
                                        grid_h, use_max, feat_layout, feat_layout == 0 ? C : ldc, rois_are_corners, S(stream));
}

int xdet_rotated_psroialign_fwd(const float* feat, const float* rois, const int32_t* orders, float* pooled,
                                int32_t* index, int N, int C, int H, int W, int R, int grid_w, int grid_h, int use_max,
                                int feat_layout, int ldc, void* stream) {
  return launch_rotated_psroialign(feat, rois, orders, pooled, index, N, C, H, W, R, grid_w, grid_h, use_max,
                                   feat_layout, feat_layout == 0 ? C : ldc, S(stream));
}

int xdet_rotated_psroialign_grad(const float* rois, const int32_t* orders, const float* grad_pooled,
                                 const int32_t* pooled_index, float* grad_feat, int N, int C, int H, int W, int R,
                                 int grid_w, int grid_h, int use_max, int feat_layout, int ldc, void* stream) {
  return launch_rotated_psroialign_grad(rois, orders, grad_pooled, pooled_index, grad_feat, N, C, H, W, R, grid_w,
                                        grid_h, use_max, feat_layout, feat_layout == 0 ? C : ldc, S(stream));
}

int xdet_conv_create(void** layer, int kh, int kw, int cin, int cout, int stride, int dilation, int pad_mode,
                     int pad_t, int pad_l, const float* k, const float* scale, const float* shift, int relu_out) {
  XDET_REQUIRE(layer, "layer is NULL");
  std::unique_ptr<ConvLayer> L(new ConvLayer());
  XDET_TRY(L->init(kh, kw, cin, cout, stride, dilation, pad_mode, pad_t, pad_l, k, scale, shift, relu_out));
  *layer = static_cast<LayerBase*>(L.release());
  return XDET_OK;
}
int xdet_conv_forward(void* layer, const float* in, int N, int H, int W, int ld_in, float* out, int ld_out,
                      const float* residual, int relu_in, void* stream) {
  LayerBase* b = static_cast<LayerBase*>(layer);
  XDET_REQUIRE(b && b->kind == 1, "not a conv layer");
  DeviceGuard guard(b->device);
  ConvIO io;
  io.in = in; io.out = out; io.res = residual; io.relu_in = relu_in;
  return static_cast<ConvLayer*>(b)->forward(io, N, H, W, ld_in, ld_out, S(stream));
}
int xdet_split_f32(const float* in, uint16_t* hi, uint16_t* lo, int64_t n_pix, int ld, int relu, void* stream) {
  XDET_REQUIRE(in && hi && lo, "split: NULL argument");
  return launch_split_f32(in, hi, lo, n_pix, ld, relu, S(stream));
}
int xdet_conv_forward_planes(void* layer, const uint16_t* in_hi, const uint16_t* in_lo, int N, int H, int W,
                             int ld_in, float* out, int ld_out, const float* residual, void* stream) {
  LayerBase* b = static_cast<LayerBase*>(layer);
  XDET_REQUIRE(b && b->kind == 1, "not a conv layer");
  ConvLayer* L = static_cast<ConvLayer*>(b);
  XDET_REQUIRE(L->dma_capable(), "layer was not created in a split-precision mode (or has < 32 input channels)");
  XDET_REQUIRE(in_hi && (in_lo || L->precision == PREC_F16), "conv(planes): NULL planes");
  DeviceGuard guard(L->device);
  ConvIO io;
  io.in_hi = in_hi; io.in_lo = in_lo; io.zeros = L->d_zeros; io.out = out; io.res = residual;
  return L->forward(io, N, H, W, ld_in, ld_out, S(stream));
}
int xdet_split_f32_x8(const float* in, uint16_t* hi, uint16_t* lo8, int64_t n_pix, int ld, int relu, int x8_exp, void* stream) {
  XDET_REQUIRE(in && hi && lo8, "split: NULL argument");
  XDET_REQUIRE(x8_exp > -100 && x8_exp < 100, "split(x8): exponent out of range");
  return launch_split_f32(in, hi, lo8, n_pix, ld, relu, S(stream), 1.f, 1, x8_exp);
}
int xdet_conv_forward_planes_x8(void* layer, const uint16_t* in_hi, const uint16_t* in_lo8, int N, int H, int W, int ld_in,
                                float* out, int ld_out, const float* residual, int x8_exp, void* stream) {
  LayerBase* b = static_cast<LayerBase*>(layer);
  XDET_REQUIRE(b && b->kind == 1, "not a conv layer");
  ConvLayer* L = static_cast<ConvLayer*>(b);
  XDET_REQUIRE(L->dma_capable() && L->d_wt_x8_b, "conv(x8): a pointwise (1x1, stride 1) layer created in the f16x3 mode is needed");
  XDET_REQUIRE(in_hi && in_lo8, "conv(planes): NULL planes");
  XDET_REQUIRE(x8_exp > -100 && x8_exp < 100, "conv(x8): exponent out of range");
  DeviceGuard guard(L->device);
  ConvIO io;
  io.in_hi = in_hi; io.in_lo = in_lo8; io.zeros = L->d_zeros; io.out = out; io.res = residual;
  io.x8 = 1; io.x8_exp = x8_exp;
  return L->forward(io, N, H, W, ld_in, ld_out, S(stream));
}
// A door for tests over stand-alone layers (xdet_conv_create).  Not for a layer that belongs to a net: the planes affine and
// out_exp given here replace the layer's own (a plan's calibration) and stay set.
int xdet_conv_forward_emit(void* layer, const float* in, const uint16_t* in_hi, const uint16_t* in_lo, int x8, int x8_exp, int relu_in,
                           int N, int H, int W, int ld_in, float* out, int ld_out, const float* residual, uint16_t* out_hi,
                           uint16_t* out_lo, int planes_ld, int planes_relu, const float* bn_scale, const float* bn_shift,
                           int out_exp, void* stream) {
  LayerBase* b = static_cast<LayerBase*>(layer);
  XDET_REQUIRE(b && b->kind == 1, "not a conv layer");
  ConvLayer* L = static_cast<ConvLayer*>(b);
  XDET_REQUIRE(L->groups == 1, "conv(emit): grouped GEMMs write no planes");
  XDET_REQUIRE((in != nullptr) != (in_hi != nullptr), "conv(emit): the input is either f32 or planes");
  XDET_REQUIRE(!in_hi || L->dma_capable(), "layer was not created in a split-precision mode (or has < 32 input channels)");
  XDET_REQUIRE(!in_hi || in_lo || L->precision == PREC_F16, "conv(emit): NULL planes");
  XDET_REQUIRE(!in_hi || !relu_in, "conv(emit): planes carry their ReLU already");
  XDET_REQUIRE(!x8 || (in_hi && in_lo && L->d_wt_x8_b && x8_exp > -100 && x8_exp < 100),
               "conv(emit): x8 planes need a pointwise (1x1, stride 1) f16x3 layer and an exponent in (-100, 100)");
  XDET_REQUIRE(out || out_hi || out_lo, "conv(emit): no output at all");
  XDET_REQUIRE((out_hi != nullptr) == (out_lo != nullptr), "conv(emit): the planes copy is a pair of planes");
  const bool emit = out_hi != nullptr;
  XDET_REQUIRE(!emit || L->precision != PREC_F32, "conv(emit): a layer created in the f32 mode writes no planes");
  XDET_REQUIRE(emit || (planes_ld == 0 && !planes_relu && !bn_scale && !bn_shift && out_exp == 0),
               "conv(emit): planes options without planes");
  XDET_REQUIRE((bn_scale != nullptr) == (bn_shift != nullptr), "conv(emit): a planes BN is a scale and a shift");
  XDET_REQUIRE(out_exp > -100 && out_exp < 100, "conv(emit): out_exp out of range");
  XDET_REQUIRE(ld_out == L->ld_out(), "conv: ld_out must be round_up(cout,32)");
  XDET_REQUIRE(planes_ld == 0 || (planes_ld % 32 == 0 && planes_ld >= ld_out),
               "conv(emit): planes_ld must be 0, ld_out or a larger multiple of 32");
  const bool wide = planes_ld > ld_out, folded_bn = bn_scale != nullptr;
  XDET_REQUIRE(!wide || !folded_bn, "conv(emit): a concatenated planes destination takes no folded BN");
  DeviceGuard guard(L->device);
  if (emit && (folded_bn || out_exp != 0 || L->out_exp != 0 || !L->pl_shift.host.empty())) {
    XDET_HIP(hipStreamSynchronize(S(stream)));          // (an earlier call may still read the arrays rewritten below)
    if (folded_bn) {
      XDET_TRY(L->set_planes_bn(std::vector<float>(bn_scale, bn_scale + L->cout), std::vector<float>(bn_shift, bn_shift + L->cout)));
    } else {
      L->pl_scale.host.clear();                         // (set_out_exp fills in the ones)
      L->pl_shift.host.clear();
    }
    XDET_TRY(L->set_out_exp(out_exp));
  }
  ConvIO io;
  io.in = in; io.in_hi = in_hi; io.in_lo = in_lo; io.zeros = in_hi ? L->d_zeros : nullptr; io.relu_in = relu_in;
  io.x8 = x8 ? 1 : 0; io.x8_exp = x8 ? x8_exp : 0;
  io.out = out; io.res = residual;
  if (emit) {
    // as Plan::add_conv fills it: a folded BN implies the planes ReLU; the affine goes in exactly when there is one
    io.out_hi = out_hi; io.out_lo = out_lo;
    io.planes_relu = (planes_relu || folded_bn) ? 1 : 0;
    if (folded_bn || L->out_exp != 0) { io.pl_scale = L->d_pl_scale; io.pl_shift = L->d_pl_shift; }
  }
  const int saved_c32 = L->pl_c32;
  L->pl_c32 = wide ? planes_ld >> 5 : 0;
  const int rc = L->forward(io, N, H, W, ld_in, ld_out, S(stream));
  L->pl_c32 = saved_c32;
  return rc;
}
int xdet_conv_set_ksplit(void* layer, int ksplit, int mode, int max_parallel_tiles) {
  LayerBase* b = static_cast<LayerBase*>(layer);
  XDET_REQUIRE(b && b->kind == 1, "not a conv layer");
  ConvLayer* L = static_cast<ConvLayer*>(b);
  XDET_REQUIRE(mode >= 0 && mode <= 2 && max_parallel_tiles >= 0, "conv_set_ksplit: mode 0|1|2, max_parallel_tiles >= 0");
  DeviceGuard guard(L->device);
  if (ksplit == 0) { L->ksplit = 0; return XDET_OK; }
  XDET_REQUIRE((L->kh == 1 && L->kw == 1) || (L->kh == 3 && L->kw == 3), "conv_set_ksplit: the split-K kernel runs 1x1 and 3x3 filters");
  XDET_TRY(L->enable_ksplit(ksplit, max_parallel_tiles));
  L->ks_mode = mode;
  return XDET_OK;
}
int xdet_conv_out_shape(void* layer, int H, int W, int* Ho, int* Wo) {
  LayerBase* b = static_cast<LayerBase*>(layer);
  XDET_REQUIRE(b && b->kind == 1, "not a conv layer");
  int a, c;
  static_cast<ConvLayer*>(b)->out_shape(H, W, Ho, Wo, &a, &c);
  return XDET_OK;
}
int xdet_layer_destroy(void* layer) {
  if (!layer) return XDET_OK;
  DeviceGuard guard(static_cast<LayerBase*>(layer)->device);
  delete static_cast<LayerBase*>(layer);
  return XDET_OK;
}
int xdet_depthwise_create(void** layer, int C, int dilation, const float* k) {
  XDET_REQUIRE(layer, "layer is NULL");
  std::unique_ptr<DepthwiseLayer> L(new DepthwiseLayer());
  XDET_TRY(L->init(C, dilation, k));
  *layer = static_cast<LayerBase*>(L.release());
  return XDET_OK;
}
int xdet_depthwise_forward(void* layer, const float* in, int N, int H, int W, int ld, float* out, int relu_in,
                           void* stream) {
  LayerBase* b = static_cast<LayerBase*>(layer);
  XDET_REQUIRE(b && b->kind == 2, "not a depthwise layer");
  DeviceGuard guard(b->device);
  return static_cast<DepthwiseLayer*>(b)->forward(in, N, H, W, ld, out, relu_in, S(stream));
}
int xdet_sepconv_fused_forward(void* dw_layer, void* pw_layer, const float* in, int N, int H, int W, int ld_in, float* out,
                               int ld_out, int relu_in, void* stream) {
  LayerBase* a = static_cast<LayerBase*>(dw_layer);
  LayerBase* b = static_cast<LayerBase*>(pw_layer);
  XDET_REQUIRE(a && a->kind == 2 && b && b->kind == 1, "sepconv_fused: need a depthwise and a conv layer");
  DepthwiseLayer* D = static_cast<DepthwiseLayer*>(a);
  ConvLayer* L = static_cast<ConvLayer*>(b);
  XDET_REQUIRE(L->dma_capable() && L->kh == 1 && L->kw == 1 && L->stride == 1 && L->groups == 1,
               "sepconv_fused: the pointwise layer must be a 1x1 stride-1 conv created in a split-precision mode");
  XDET_REQUIRE(D->ld == ld_in && L->ld_in() == ld_in && L->ld_out() == ld_out && ld_out <= L->cout_pad &&
                   sepconv_fused_supported(ld_in, L->cout_pad, D->dil),
               "sepconv_fused: needs <= 256 input channels (multiple of 32), <= 128 or 129..1024 outputs, dilation 1");
  DeviceGuard guard(L->device);
  return launch_sepconv_fused(in, D->d_w, L->d_wt_hi_b, L->d_wt_lo_b, L->d_scale, L->d_shift, out, N, H, W, ld_in, ld_out,
                              L->cout_pad, relu_in, L->relu_out, S(stream));
}
int xdet_conv3x3_patch_forward(void* layer, const uint16_t* in_hi, const uint16_t* in_lo, int N, int H, int W, float* out,
                               int ld_out, void* stream) {
  LayerBase* b = static_cast<LayerBase*>(layer);
  XDET_REQUIRE(b && b->kind == 1, "not a conv layer");
  ConvLayer* L = static_cast<ConvLayer*>(b);
  XDET_REQUIRE(L->dma_capable() && L->groups == 1 && L->ld_in() == 32 && L->ld_out() == ld_out && L->cout_pad == ld_out &&
                   conv3x3_patch_supported(L->kh, L->kw, L->cin, L->cout_pad, L->stride, L->dil, L->pad_mode),
               "conv3x3_patch: needs a 3x3 / stride 1 / VALID conv over 32 channels with <= 64 outputs, split-precision mode");
  XDET_REQUIRE(in_hi && (in_lo || L->precision == PREC_F16), "conv3x3_patch: NULL planes");
  DeviceGuard guard(L->device);
  return launch_conv3x3_patch(in_hi, L->precision == PREC_F16 ? nullptr : in_lo, L->d_wt_hi_b, L->d_wt_lo_b, L->d_scale,
                              L->d_shift, out, N, H, W, ld_out, L->relu_out, S(stream));
}
int xdet_resnet_bneck_forward(void* conv_a, void* conv_b, void* conv_c, const float* pre_scale, const float* pre_shift,
                              const float* x, int N, int H, int W, float* out, const float* next_scale,
                              const float* next_shift, uint16_t* out_hi, uint16_t* out_lo, void* stream) {
  LayerBase* b[3] = {static_cast<LayerBase*>(conv_a), static_cast<LayerBase*>(conv_b), static_cast<LayerBase*>(conv_c)};
  XDET_REQUIRE(b[0] && b[1] && b[2] && b[0]->kind == 1 && b[1]->kind == 1 && b[2]->kind == 1, "resnet_bneck: three conv layers");
  ConvLayer *A = static_cast<ConvLayer*>(b[0]), *B = static_cast<ConvLayer*>(b[1]), *C = static_cast<ConvLayer*>(b[2]);
  XDET_REQUIRE(A->precision == PREC_F16X3 && B->precision == PREC_F16X3 && C->precision == PREC_F16X3 && A->dma_capable() &&
                   B->dma_capable() && C->dma_capable() && A->groups == 1 && B->groups == 1 && C->groups == 1,
               "resnet_bneck: the three layers must be created in mode 1 (f16x3)");
  XDET_REQUIRE(A->kh == 1 && A->kw == 1 && A->stride == 1 && A->relu_out == 1 && B->kh == 3 && B->kw == 3 && B->stride == 1 &&
                   B->dil == 1 && B->pad_mode == 1 && B->relu_out == 1 && C->kh == 1 && C->kw == 1 && C->stride == 1 &&
                   C->relu_out == 0 && A->cout == B->cin && B->cout == C->cin && B->cin == B->cout && C->cout == A->cin &&
                   A->cout_pad == A->cout && B->cout_pad == B->cout && C->cout_pad == C->cout,
               "resnet_bneck: need 1x1 (ReLU) -> 3x3 SAME stride 1 (ReLU) -> 1x1 with Cin -> Cmid -> Cmid -> Cin channels");
  XDET_REQUIRE(resnet_bneck_supported(A->cin, A->cout, C->cout, H, W, N), "resnet_bneck: unsupported channel counts / tensor size");
  XDET_REQUIRE(pre_scale && pre_shift && x && out && (!out_hi || (out_lo && next_scale && next_shift)), "resnet_bneck: NULL argument");
  BneckLaunch a;
  a.x = x; a.pre_sc = pre_scale; a.pre_sh = pre_shift;
  a.wa_hi = A->d_wt_hi_b; a.wa_lo = A->d_wt_lo_b; a.wb_hi = B->d_wt_hi_b; a.wb_lo = B->d_wt_lo_b; a.wc_hi = C->d_wt_hi_b; a.wc_lo = C->d_wt_lo_b;
  a.sc_a = A->d_scale; a.sh_a = A->d_shift; a.sc_b = B->d_scale; a.sh_b = B->d_shift; a.sc_c = C->d_scale; a.sh_c = C->d_shift;
  a.pl_sc = next_scale; a.pl_sh = next_shift;
  a.out = out; a.out_hi = out_hi; a.out_lo = out_lo;
  a.H = H; a.W = W; a.cin = A->cin; a.cmid = A->cout; a.cout = C->cout;
  DeviceGuard guard(A->device);
  return launch_resnet_bneck(a, N, S(stream));
}
int xdet_spectral_conv_create(void** layer, const float* kernel_host, int taps, int cin, int cout, int axis, int F,
                              const float* scale_host, const float* shift_host, int relu_out) {
  XDET_REQUIRE(layer, "layer is NULL");
  std::unique_ptr<SpectralConv> L(new SpectralConv());
  XDET_TRY(L->init(kernel_host, taps, cin, cout, axis, F, scale_host, shift_host, relu_out));
  *layer = static_cast<LayerBase*>(L.release());
  return XDET_OK;
}
// workspace of a batch of N: [x_hi | x_lo | y], each with 512 bytes of slack, each starting 256-byte aligned
struct SpectralWorkspace { unsigned short *x_hi, *x_lo; float* y; };
static SpectralWorkspace spectral_layout(WsWalk& w, const SpectralConv* L, int N) {
  const size_t pl = L->planes_halves(N) + 256;
  return {w.take<unsigned short>(pl), w.take<unsigned short>(pl), w.take<float>(L->y_floats(N) + 128)};
}
size_t xdet_spectral_conv_workspace_bytes(void* layer, int N) {
  LayerBase* b = static_cast<LayerBase*>(layer);
  if (!b || b->kind != 3 || N <= 0) return 0;
  return ws_measure(256, spectral_layout, static_cast<const SpectralConv*>(b), N);
}
int xdet_spectral_conv_forward(void* layer, const float* in, int N, int ld_in, void* workspace, float* out, int ld_out,
                               void* stream) {
  LayerBase* b = static_cast<LayerBase*>(layer);
  XDET_REQUIRE(b && b->kind == 3, "not a spectral conv layer");
  SpectralConv* L = static_cast<SpectralConv*>(b);
  XDET_REQUIRE(in && workspace && out && N > 0 && (int64_t)N * L->F <= (1 << 24), "spectral conv: NULL argument / bad batch");
  XDET_REQUIRE(ld_in == L->cin_ld && ld_out >= L->cout_ld && ld_out % 4 == 0 && (uintptr_t)workspace % 256 == 0,
               "spectral conv: ld_in must be round_up(cin,32), ld_out a multiple of 4 and >= round_up(cout,32), the workspace 256-byte aligned");
  const SpectralWorkspace ws = ws_carve(workspace, 256, spectral_layout, L, N);
  DeviceGuard guard(L->device);
  return L->forward(in, N, ws.x_hi, ws.x_lo, ws.y, out, ld_out, S(stream));
}
int xdet_stem_conv3x3s2_forward(const float* in_nchw, const float* w27x32, const float* scale, const float* shift,
                                uint16_t* out_hi, uint16_t* out_lo, int N, int S_, void* stream) {
  XDET_REQUIRE(in_nchw && w27x32 && scale && shift && out_hi && out_lo, "stem_conv3x3s2: NULL argument");
  XDET_REQUIRE(N > 0 && S_ >= 3 && (int64_t)N * S_ * S_ < ((int64_t)1 << 31), "stem_conv3x3s2: bad batch / image side");
  return launch_stem_conv3x3s2(in_nchw, w27x32, scale, shift, out_hi, out_lo, N, S_, S(stream));
}
int xdet_resnet_stem7x7_forward(void* layer, const float* in_nchw, int N, int S_, float* out, void* stream) {
  LayerBase* b = static_cast<LayerBase*>(layer);
  XDET_REQUIRE(b && b->kind == 1, "not a conv layer");
  ConvLayer* L = static_cast<ConvLayer*>(b);
  XDET_REQUIRE(L->precision == PREC_F16X3 && L->groups == 1 && L->d_wt_hi && L->d_wt_lo && L->relu_out == 0 && L->pad_t == L->pad_l &&
                   L->kp == 224 && resnet_stem7x7_supported(L->kh, L->kw, L->cin, L->cout, L->stride, L->pad_mode, L->pad_t, S_),
               "resnet_stem7x7: needs a 7x7 / stride 2 / explicit pad 3 conv 3 -> 64 without ReLU, created in mode 1 (f16x3), S >= 16");
  XDET_REQUIRE(in_nchw && out && N > 0 && (int64_t)N * S_ * S_ * 16 < ((int64_t)1 << 31), "resnet_stem7x7: NULL argument / bad batch");
  DeviceGuard guard(L->device);
  return launch_resnet_stem7x7(in_nchw, L->d_wt_hi, L->d_wt_lo, L->d_scale, L->d_shift, out, N, S_, S(stream));
}
int xdet_maxpool3x3s2_bn_planes(const float* in, const float* scale, const float* shift, uint16_t* out_hi, uint16_t* out_lo,
                                int N, int H, int W, int C, int ld, float mul, uint16_t* out_hi2, uint16_t* out_lo2,
                                int c32_2, float mul2, void* stream) {
  XDET_REQUIRE(N > 0 && H > 0 && W > 0 && C > 0 && ld > 0, "maxpool + bn planes: bad shape");
  XDET_REQUIRE((out_hi2 == nullptr) == (out_lo2 == nullptr), "maxpool + bn planes: the second destination needs both planes");
  int Ho, Wo, pt, pl;
  same_pad(H, 3, 2, 1, &pt, &Ho);
  same_pad(W, 3, 2, 1, &pl, &Wo);
  return launch_maxpool3x3s2_bn_planes(in, scale, shift, out_hi, out_lo, N, H, W, C, ld, Ho, Wo, pt, pl, mul, S(stream), out_hi2,
                                       out_lo2, c32_2, mul2);
}
int xdet_resnet_preconv_forward(void* layer, const float* pre_scale, const float* pre_shift, const float* x, int N, int H,
                                int W, uint16_t* out_hi, uint16_t* out_lo, void* stream) {
  LayerBase* b = static_cast<LayerBase*>(layer);
  XDET_REQUIRE(b && b->kind == 1, "not a conv layer");
  ConvLayer* L = static_cast<ConvLayer*>(b);
  XDET_REQUIRE(L->precision == PREC_F16X3 && L->dma_capable() && L->groups == 1 && L->kh == 1 && L->kw == 1 && L->stride == 1 &&
                   L->relu_out == 1 && L->cout_pad == L->cout && L->cin_p == L->cin && L->ksplit <= 1,
               "resnet_preconv: needs a 1x1 stride-1 conv with ReLU created in mode 1 (f16x3)");
  XDET_REQUIRE(N > 0 && H > 0 && W > 0 && resnet_preconv_supported(L->cin, L->cout, (int64_t)N * H * W),
               "resnet_preconv: unsupported channel counts (256 | 512 -> 128) / tensor size");
  XDET_REQUIRE(pre_scale && pre_shift && x && out_hi && out_lo, "resnet_preconv: NULL argument");
  DeviceGuard guard(L->device);
  return launch_resnet_preconv(x, pre_scale, pre_shift, L->d_wt_hi_b, L->d_wt_lo_b, L->d_scale, L->d_shift, out_hi, out_lo,
                               (int64_t)N * H * W, L->cin, L->cout, S(stream));
}
int xdet_sepconv_fused_hpool_forward(void* dw_layer, void* pw_layer, const float* in, int N, int H, int W, int ld_in,
                                     float* out_hpooled, int ld_out, int relu_in, void* stream) {
  LayerBase* a = static_cast<LayerBase*>(dw_layer);
  LayerBase* b = static_cast<LayerBase*>(pw_layer);
  XDET_REQUIRE(a && a->kind == 2 && b && b->kind == 1, "sepconv_fused: need a depthwise and a conv layer");
  DepthwiseLayer* D = static_cast<DepthwiseLayer*>(a);
  ConvLayer* L = static_cast<ConvLayer*>(b);
  XDET_REQUIRE(L->dma_capable() && L->kh == 1 && L->kw == 1 && L->stride == 1 && L->groups == 1,
               "sepconv_fused: the pointwise layer must be a 1x1 stride-1 conv created in a split-precision mode");
  XDET_REQUIRE(D->ld == ld_in && L->ld_in() == ld_in && L->ld_out() == ld_out && ld_out <= L->cout_pad &&
                   sepconv_fused_supported(ld_in, L->cout_pad, D->dil),
               "sepconv_fused: needs <= 256 input channels (multiple of 32), <= 128 or 129..1024 outputs, dilation 1");
  int Wo, pl;
  same_pad(W, 3, 2, 1, &pl, &Wo);
  DeviceGuard guard(L->device);
  return launch_sepconv_fused(in, D->d_w, L->d_wt_hi_b, L->d_wt_lo_b, L->d_scale, L->d_shift, out_hpooled, N, H, W, ld_in,
                              ld_out, L->cout_pad, relu_in, L->relu_out, S(stream), pl);
}
int xdet_maxpool_v3s2_add(const float* in_hpooled, const float* residual, float* out, int N, int H, int Wo, int C, int ld,
                          void* stream) {
  int Ho, pt;
  same_pad(H, 3, 2, 1, &pt, &Ho);
  return launch_maxpool_v3s2_add(in_hpooled, residual, out, N, H, Wo, C, ld, Ho, pt, S(stream));
}
int xdet_maxpool3x3s2_add(const float* in, const float* residual, float* out, int N, int H, int W, int C, int ld,
                          void* stream) {
  int Ho, Wo, pt, pl;
  same_pad(H, 3, 2, 1, &pt, &Ho);
  same_pad(W, 3, 2, 1, &pl, &Wo);
  return launch_maxpool3x3s2_add(in, residual, out, N, H, W, C, ld, Ho, Wo, pt, pl, S(stream));
}
int xdet_preprocess_eval(const uint8_t* image_hwc, int H, int W, float* out_chw, int out_size, void* stream) {
  return launch_preprocess_eval(image_hwc, H, W, out_chw, out_size, S(stream));
}
int xdet_preprocess_eval_batch(const uint8_t* packed, int64_t packed_bytes, const int64_t* offsets,
                               const int32_t* image_shapes, int N, int out_size, int resize, float* out_nchw,
                               float* bbox_img, void* stream) {
  return launch_preprocess_batch(packed, packed_bytes, offsets, image_shapes, N, out_size, resize, out_nchw, bbox_img,
                                 S(stream));
}
size_t xdet_preprocess_train_workspace_bytes(int N, int G) {
  if (N <= 0 || G <= 0) return 0;
  return preprocess_train_workspace_bytes(N, G);
}
int xdet_preprocess_train_batch(const uint8_t* packed, int64_t packed_bytes, const int64_t* offsets,
                                const int32_t* image_shapes, const int32_t* glabels, const float* gbboxes,
                                const int32_t* n_gt, const int32_t* image_ids, int N, int G, int out_size, uint32_t seed,
                                float* out_nchw, int32_t* out_glabels, float* out_gbboxes, int32_t* out_n_gt, void* records,
                                void* workspace, void* stream) {
  return launch_preprocess_train(packed, packed_bytes, offsets, image_shapes, glabels, gbboxes, n_gt, image_ids, N, G,
                                 out_size, seed, out_nchw, out_glabels, out_gbboxes, out_n_gt, records, workspace, S(stream));
}
int xdet_nchw_to_nhwc4(const float* in, float* out, int N, int C, int H, int W, void* stream) {
  return launch_nchw_to_nhwc4(in, out, N, C, H, W, 4, S(stream));
}

int xdet_rpn_decode(const float* rpn_out, int ld, int cls_off, int box_off, int N, int Hh, int Ww, int A,
                    const float* anchors_yx, const float* anchors_hw, float* objectness, float* boxes, void* stream) {
  return launch_rpn_decode(rpn_out, ld, cls_off, box_off, N, Hh, Ww, A, anchors_yx, anchors_hw, objectness, boxes,
                           S(stream));
}
size_t xdet_proposals_workspace_bytes(int N, int n_anchor, int pre_n, int post_n) {
  return ws_measure(256, proposal_workspace_layout, N, n_anchor, pre_n, post_n);
}
int xdet_get_proposals(const float* objectness, const float* boxes, int N, int n_anchor, int pre_n, int post_n,
                       float nms_thr, float min_size, void* workspace, float* rois, int* counts_out, void* stream) {
  XDET_REQUIRE(objectness && boxes && workspace && rois, "get_proposals: NULL argument");
  const ProposalWorkspace ws = ws_carve(workspace, 256, proposal_workspace_layout, N, n_anchor, pre_n, post_n);
  XDET_TRY(launch_get_proposals(objectness, boxes, N, n_anchor, pre_n, post_n, nms_thr, min_size, ws, rois, S(stream)));
  if (counts_out) XDET_HIP(hipMemcpyAsync(counts_out, ws.counts, (size_t)N * 16, hipMemcpyDeviceToDevice, S(stream)));
  return XDET_OK;
}
int xdet_ext_decode_rois(const float* rois, const float* reg, int ld_reg, int64_t n, float* out, void* stream) {
  return launch_ext_decode_rois(rois, reg, ld_reg, n, out, S(stream));
}
int xdet_bboxes_eval(const float* cls, int ld_cls, const float* boxes, int N, int R, int num_classes,
                     const int* image_shapes, const float* bbox_img, int net_h, int net_w, float select_thr,
                     float nms_thr, int nms_topk, float* det_scores, float* det_boxes, void* stream) {
  XDET_REQUIRE(cls && boxes && image_shapes && bbox_img && det_scores && det_boxes, "bboxes_eval: NULL argument");
  return launch_bboxes_eval(cls, ld_cls, boxes, N, R, num_classes, image_shapes, bbox_img, net_h, net_w, select_thr,
                            nms_thr, nms_topk, det_scores, det_boxes, S(stream));
}
// The net's form of the same tail (LightHeadNet::forward_eager: launch_head_decode_probs, launch_bboxes_eval_probs) at op level
int xdet_head_decode_probs(const float* rois, const float* cls_reg, int ld, int num_classes, int R, int64_t n, int form,
                           float* boxes, float* probs, int32_t* bad, void* stream) {
  XDET_REQUIRE(rois && cls_reg && boxes && probs && bad, "head_decode_probs: NULL argument");
  XDET_REQUIRE(num_classes >= 2, "head_decode_probs: num_classes must be >= 2");
  XDET_REQUIRE(R >= 1, "head_decode_probs: rois per image must be >= 1");
  XDET_REQUIRE(n >= 0 && n % R == 0, "head_decode_probs: n must be a non-negative multiple of the rois per image");
  XDET_REQUIRE(ld >= num_classes + 4, "head_decode_probs: ld must be >= num_classes + 4");
  XDET_REQUIRE(((uintptr_t)rois & 15) == 0 && ((uintptr_t)boxes & 15) == 0, "head_decode_probs: rois and boxes must be 16-byte aligned");
  XDET_REQUIRE(form == 0 || form == 1, "head_decode_probs: form must be 0 or 1");
  return launch_head_decode_probs(rois, cls_reg, ld, num_classes, R, n, boxes, probs, bad, S(stream), form);
}
int xdet_bboxes_eval_probs(const float* probs, const float* boxes, int N, int R, int num_classes, const int* image_shapes,
                           const float* bbox_img, int net_h, int net_w, float select_thr, float nms_thr, int nms_topk,
                           const int32_t* bad_per_image, float* det_scores, float* det_boxes, void* stream) {
  XDET_REQUIRE(probs && boxes && image_shapes && bbox_img && det_scores && det_boxes, "bboxes_eval_probs: NULL argument");
  return launch_bboxes_eval_probs(probs, boxes, N, R, num_classes, image_shapes, bbox_img, net_h, net_w, select_thr, nms_thr,
                                  nms_topk, det_scores, det_boxes, S(stream), bad_per_image);
}
// 1 <= R <= 6144: the kernel above up to 1024 ROIs per image, the wide one beyond (what a net with more proposals runs)
int xdet_bboxes_eval_probs_wide(const float* probs, const float* boxes, int N, int R, int num_classes, const int* image_shapes,
                                const float* bbox_img, int net_h, int net_w, float select_thr, float nms_thr, int nms_topk,
                                const int32_t* bad_per_image, float* det_scores, float* det_boxes, void* stream) {
  XDET_REQUIRE(probs && boxes && image_shapes && bbox_img && det_scores && det_boxes, "bboxes_eval_probs_wide: NULL argument");
  return launch_bboxes_eval_probs_wide(probs, boxes, N, R, num_classes, image_shapes, bbox_img, net_h, net_w, select_thr, nms_thr,
                                       nms_topk, det_scores, det_boxes, S(stream), bad_per_image, false);
}
// the wide kernel at any R (tests: the two kernels on the same input)
int xdet_bboxes_eval_probs_wide_only(const float* probs, const float* boxes, int N, int R, int num_classes,
                                     const int* image_shapes, const float* bbox_img, int net_h, int net_w, float select_thr,
                                     float nms_thr, int nms_topk, const int32_t* bad_per_image, float* det_scores,
                                     float* det_boxes, void* stream) {
  XDET_REQUIRE(probs && boxes && image_shapes && bbox_img && det_scores && det_boxes, "bboxes_eval_probs_wide_only: NULL argument");
  return launch_bboxes_eval_probs_wide(probs, boxes, N, R, num_classes, image_shapes, bbox_img, net_h, net_w, select_thr, nms_thr,
                                       nms_topk, det_scores, det_boxes, S(stream), bad_per_image, true);
}

// A handle is a void*: both plan types start with their Plan base, whose kind tag says what the pointer really is
// (handing a resnet handle to a light-head entry point used to be undefined behaviour).
static Plan* plan_of(void* net) { return static_cast<Plan*>(net); }
static bool is_plan(void* net) { return net && (plan_of(net)->plan_kind == 0 || plan_of(net)->plan_kind == 1); }
#define XDET_NET_KIND(net, kind, what)                                                                     \
  XDET_REQUIRE((net) != nullptr && plan_of(net)->plan_kind == (kind), what ": not a handle of this net type")
// the typed handle of an entry point: checked, cast, and its device current until the entry point returns
#define XDET_LIGHTHEAD(n, net, what) \
  XDET_NET_KIND(net, 0, what);       \
  LightHeadNet* n = static_cast<LightHeadNet*>(net); \
  DeviceGuard n##_guard(n->device)
#define XDET_RESNET(r, net, what) \
  XDET_NET_KIND(net, 1, what);    \
  ResNetTrunk* r = static_cast<ResNetTrunk*>(net); \
  DeviceGuard r##_guard(r->device)

// ---- light-head net ----
static int set_weight(Plan* p, const char* name, const float* data, int ndim, const int64_t* dims) {
  XDET_REQUIRE(p && name && data && ndim >= 1 && ndim <= 4 && dims, "set_weight: bad arguments");
  HostTensor t;
  size_t n = 1;
  for (int i = 0; i < ndim; ++i) { t.dims.push_back(dims[i]); n *= (size_t)dims[i]; }
  t.v.assign(data, data + n);
  p->w[name] = std::move(t);
  return XDET_OK;
}

int xdet_net_create(void** net, const xdet_lighthead_config* cfg) {
  XDET_REQUIRE(net && cfg, "net/cfg is NULL");
  std::unique_ptr<LightHeadNet> n(new LightHeadNet());
  n->plan_kind = 0;
  n->cfg = *cfg;
  XDET_HIP(hipGetDevice(&n->device));
  *net = n.release();
  return XDET_OK;
}
int xdet_net_set_weight(void* net, const char* name, const float* data, int ndim, const int64_t* dims) {
  XDET_LIGHTHEAD(n, net, "net_set_weight");
  return set_weight(n, name, data, ndim, dims);
}
int xdet_net_set_option(void* net, const char* key, const char* value) {
  XDET_LIGHTHEAD(n, net, "net_set_option");
  XDET_REQUIRE(n && key && value, "set_option: NULL argument");
  XDET_REQUIRE(!n->built, "set_option: the net is already built");
  const std::string k(key), v(value);
  if (k == "large_sep") {
    XDET_REQUIRE(v == "auto" || v == "direct" || v == "spectral", "large_sep must be auto | direct | spectral");
    n->large_sep_mode = v == "auto" ? 0 : v == "direct" ? 1 : 2;
    return XDET_OK;
  }
  if (k == "spectral_refresh") {
    XDET_REQUIRE(v == "on" || v == "off", "spectral_refresh must be on | off");
    n->spectral_refresh = v == "on";
    return XDET_OK;
  }
  if (k == "rpn_stream") {
    XDET_REQUIRE(v == "side" || v == "main", "rpn_stream must be side | main");
    n->rpn_side_stream = v == "side";
    return XDET_OK;
  }
  if (k == "pool_sub") {
    XDET_REQUIRE(v == "on" || v == "off", "pool_sub: on | off");
    n->pool_writes_projection_input = v == "on";
    return XDET_OK;
  }
  if (k == "workspace") {
    XDET_REQUIRE(v == "reuse" || v == "ssa" || v == "poison", "workspace: reuse | ssa | poison");
    XDET_REQUIRE(!(v != "ssa" && n->check_range), "workspace=reuse: check_range validates every tensor after the forward and needs workspace=ssa");
    n->reuse_workspace = v != "ssa";
    n->poison_recycled = v == "poison";
    return XDET_OK;
  }
  if (k == "sepconv") {
    XDET_REQUIRE(v == "fused" || v == "split", "sepconv must be fused | split");
    n->fuse_sepconv = v == "fused";
    return XDET_OK;
  }
  if (k == "ksplit") {
    XDET_REQUIRE(v == "on" || v == "off" || v == "all", "ksplit must be on | off | all");
    n->latency_ksplit = v != "off";
    n->rpn_ksplit = v == "all";
    return XDET_OK;
  }
  if (k == "cross") {
    XDET_REQUIRE(v == "f16" || v == "fp8", "cross must be f16 | fp8");
    n->cross8 = v == "fp8";
    return XDET_OK;
  }
  if (k == "check_range") {
    XDET_REQUIRE(v == "on" || v == "off", "check_range must be on | off");
    n->check_range = v == "on";
    if (n->check_range) n->reuse_workspace = false;   // the validation pass reads every tensor after the forward
    return XDET_OK;
  }
  if (k == "pool") {
    XDET_REQUIRE(v == "split" || v == "whole" || v == "split_all", "pool must be split | whole | split_all");
    n->fuse_hpool = v != "whole";
    if (v == "split_all") n->pool_fuse_min_pixels = 0;
    return XDET_OK;
  }
  if (k == "conv3x3") {
    XDET_REQUIRE(v == "patch" || v == "gemm", "conv3x3 must be patch | gemm");
    n->patch_conv3x3 = v == "patch";
    return XDET_OK;
  }
  if (k == "pool_index") {
    XDET_REQUIRE(v == "keep" || v == "off", "pool_index must be keep | off");
    n->keep_pool_index = v == "keep";
    return XDET_OK;
  }
  if (k == "head_rois") {
    // "off", or the sampled ROIs per image the head stage is planned on: a whole number in 1..rpn_post_nms_top_n
    if (v == "off") { n->head_rois_n = 0; return XDET_OK; }
    char* end = nullptr;
    const long p = v.empty() ? 0 : strtol(v.c_str(), &end, 10);
    XDET_REQUIRE(!v.empty() && end && *end == '\0' && p >= 1 && p <= (long)n->cfg.rpn_post_nms_top_n,
                 "head_rois must be off or a whole number in 1..rpn_post_nms_top_n (" + std::to_string(n->cfg.rpn_post_nms_top_n) +
                     "), got " + v);
    n->head_rois_n = (int)p;
    return XDET_OK;
  }
  if (k == "eval_head") {
    XDET_REQUIRE(v == "on" || v == "off", "eval_head must be on | off");
    n->eval_head = v == "on";
    return XDET_OK;
  }
  if (k == "rpn_hidden") {
    XDET_REQUIRE(v == "keep" || v == "off", "rpn_hidden must be keep | off");
    n->keep_rpn_hidden = v == "keep";
    return XDET_OK;
  }
  if (k == "entry_x") {
    XDET_REQUIRE(v == "keep" || v == "off", "entry_x must be keep | off");
    n->keep_entry_x = v == "keep";
    return XDET_OK;
  }
  if (k == "stem_out") {
    XDET_REQUIRE(v == "keep" || v == "off", "stem_out must be keep | off");
    n->keep_stem_out = v == "keep";
    return XDET_OK;
  }
  set_last_error("unknown option: " + k);
  return XDET_ERR_INVALID_ARG;
}
int xdet_net_build(void* net) {
  XDET_LIGHTHEAD(n, net, "net_build");
  return n->build();
}
int xdet_net_destroy(void* net) {
  if (!net) return XDET_OK;
  XDET_LIGHTHEAD(n, net, "net_destroy");
  delete n;
  return XDET_OK;
}

int xdet_net_buffer(void* net, const char* name, void** dptr, int64_t dims[4], int* ld) {
  XDET_LIGHTHEAD(n, net, "net_buffer");
  XDET_REQUIRE(n && n->built && name && dptr && dims && ld, "net_buffer: bad arguments");
  const std::string s(name);
  const int B = n->max_batch, R = n->cfg.rpn_post_nms_top_n;
  auto from_buf = [&](const Buf& b) { *dptr = b.p; dims[0] = B; dims[1] = b.H; dims[2] = b.W; dims[3] = b.C; *ld = b.ld; };
  if (s == "mid_x") from_buf(n->mid_x);
  else if (s == "mid") { from_buf(n->mid_x); *dptr = n->mid_relu; }
  else if (s == "out") from_buf(n->out);
  else if (s == "rpn_out") from_buf(n->rpn_out);
  else if (s == "feat") from_buf(n->feat);
  else if (s == "pooled") from_buf(n->pooled);
  else if (s == "pool_index") {
    XDET_REQUIRE(n->pool_index != nullptr, "net_buffer: pool_index needs a net built with the option pool_index=keep");
    from_buf(n->pooled);
    *dptr = n->pool_index;
  }
  else if (s == "rpn_hidden") {
    XDET_REQUIRE(n->rpn_hidden.p != nullptr, "net_buffer: rpn_hidden needs a net built with the option rpn_hidden=keep");
    from_buf(n->rpn_hidden);
  }
  else if (s == "entry_x") {
    XDET_REQUIRE(n->entry_x.p != nullptr, "net_buffer: entry_x needs a net built with the option entry_x=keep");
    from_buf(n->entry_x);
  }
  else if (s == "stem_out") {
    XDET_REQUIRE(n->stem_out.p != nullptr, "net_buffer: stem_out needs a net built with the option stem_out=keep");
    from_buf(n->stem_out);
  }
  else if (s == "fc") from_buf(n->fc);
  else if (s == "cls_reg") from_buf(n->cls_reg);
  else if (s == "objectness") { *dptr = n->objectness; dims[0] = B; dims[1] = n->n_anchor; dims[2] = 1; dims[3] = 1; *ld = 1; }
  else if (s == "rpn_boxes") { *dptr = n->rpn_boxes; dims[0] = B; dims[1] = n->n_anchor; dims[2] = 1; dims[3] = 4; *ld = 4; }
  else if (s == "proposals") { *dptr = n->proposals; dims[0] = B; dims[1] = R; dims[2] = 1; dims[3] = 4; *ld = 4; }
  else if (s == "head_rois") {
    XDET_REQUIRE(n->head_rois != nullptr, "net_buffer: head_rois needs a net built with the option head_rois=<P>");
    *dptr = n->head_rois; dims[0] = B; dims[1] = n->head_rois_n; dims[2] = 1; dims[3] = 4; *ld = 4;
  }
  else if (s == "pooled_eval" || s == "fc_eval" || s == "cls_reg_eval") {
    XDET_REQUIRE(n->pooled_eval.p != nullptr, "net_buffer: " + s + " needs a net built with the options head_rois=<P> and eval_head=on");
    from_buf(s == "pooled_eval" ? n->pooled_eval : s == "fc_eval" ? n->fc_eval : n->cls_reg_eval);
  }
  else if (s == "head_boxes") { *dptr = n->head_boxes; dims[0] = B; dims[1] = R; dims[2] = 1; dims[3] = 4; *ld = 4; }
  else if (s == "prop_counts") { *dptr = n->prop_ws.counts; dims[0] = B; dims[1] = 4; dims[2] = 1; dims[3] = 1; *ld = 1; }
  else if (s == "sorted_boxes") { *dptr = n->prop_ws.sboxes; dims[0] = B; dims[1] = n->cfg.rpn_pre_nms_top_n; dims[2] = 1; dims[3] = 4; *ld = 4; }
  else if (s == "sorted_scores") { *dptr = n->prop_ws.sscores; dims[0] = B; dims[1] = n->cfg.rpn_pre_nms_top_n; dims[2] = 1; dims[3] = 1; *ld = 1; }
  else {
    set_last_error("unknown buffer: " + s);
    return XDET_ERR_INVALID_ARG;
  }
  return XDET_OK;
}

int xdet_net_xception_body(void* net, const float* images, int N, void* stream) {
  XDET_LIGHTHEAD(n, net, "net_xception_body");
  XDET_TRY(n->xception_body(images, N, S(stream)));
  // materialise mid_outputs = ReLU(x) for API users (the fused forward applies it on load instead)
  return launch_relu_copy(n->mid_x.p, n->mid_relu, (int64_t)N * n->mid_x.per_image(), S(stream));
}
int xdet_net_mid_refresh(void* net, int N, void* stream) {
  XDET_LIGHTHEAD(n, net, "net_mid_refresh");
  return n->mid_refresh(N, S(stream));
}
int xdet_net_refresh_weights(void* net, const xdet_net_weight_dev* table, int n, void* stream) {
  XDET_LIGHTHEAD(nt, net, "net_refresh_weights");
  return nt->refresh_weights(table, n, S(stream));
}
int xdet_net_refresh_heads(void* net, const xdet_net_weight_dev* table, int n, void* stream) {
  XDET_LIGHTHEAD(nt, net, "net_refresh_heads");
  return nt->refresh_heads(table, n, S(stream));
}
int xdet_net_refresh_stem(void* net, const xdet_net_weight_dev* table, int n, void* stream) {
  XDET_LIGHTHEAD(nt, net, "net_refresh_stem");
  return nt->refresh_stem(table, n, S(stream));
}
int xdet_net_get_rpn(void* net, int N, void* stream) {
  XDET_LIGHTHEAD(n, net, "net_get_rpn");
  XDET_TRY(n->check(N));
  return n->run_stage(ST_RPN, N, S(stream));
}
int xdet_net_large_sep(void* net, int N, void* stream) {
  XDET_LIGHTHEAD(n, net, "net_large_sep");
  XDET_TRY(n->check(N));
  return n->run_stage(ST_LSEP, N, S(stream));
}
int xdet_net_rpn_decode(void* net, int N, void* stream) {
  XDET_LIGHTHEAD(n, net, "net_rpn_decode");
  return n->rpn_decode(N, S(stream));
}
int xdet_net_get_proposals(void* net, int N, void* stream) {
  XDET_LIGHTHEAD(n, net, "net_get_proposals");
  return n->get_proposals(N, S(stream));
}
int xdet_net_get_head(void* net, int N, void* stream) {
  XDET_LIGHTHEAD(n, net, "net_get_head");
  return n->get_head(N, S(stream));
}
int xdet_net_head_pool_backward(void* net, int N, const float* d_pooled, int ld, float* d_feat, void* stream) {
  XDET_LIGHTHEAD(n, net, "net_head_pool_backward");
  return n->head_pool_backward(N, d_pooled, ld, d_feat, S(stream));
}
int xdet_net_head_decode(void* net, int N, void* stream) {
  XDET_LIGHTHEAD(n, net, "net_head_decode");
  return n->head_decode(N, S(stream));
}
int xdet_net_bboxes_eval(void* net, int N, const int* image_shapes, const float* bbox_img, float* det_scores,
                         float* det_boxes, void* stream) {
  XDET_LIGHTHEAD(n, net, "net_bboxes_eval");
  XDET_REQUIRE(net && det_scores && det_boxes, "bboxes_eval: NULL argument");
  return n->bboxes_eval(N, image_shapes, bbox_img, det_scores, det_boxes, S(stream));
}

int xdet_net_forward(void* net, const float* images, int N, const int* image_shapes, const float* bbox_img,
                     float* det_scores, float* det_boxes, int use_graph, void* stream) {
  XDET_LIGHTHEAD(n, net, "net_forward");
  XDET_REQUIRE(n && images && det_scores && det_boxes, "forward: NULL argument");
  XDET_TRY(n->eval_refused("net_forward", /*whole_forward=*/true));      // (ahead of a graph capture)
  XDET_TRY(n->check(N));
  hipStream_t s = S(stream);
  if (!use_graph) return n->forward_eager(images, N, image_shapes, bbox_img, det_scores, det_boxes, s);
  XDET_REQUIRE(s != nullptr, "graph replay needs an explicit (non-default) stream");
  // the cache key is the whole argument tuple: a call with another input, shape, bbox or output buffer captures its own
  // graph (double-buffered outputs keep one graph each)
  const GraphCache::Key key = {{(uintptr_t)N, (uintptr_t)images, (uintptr_t)image_shapes, (uintptr_t)bbox_img,
                                (uintptr_t)det_scores, (uintptr_t)det_boxes, 0, 0, 0, 0}};
  return n->graphs.launch(key, s, [&]() { return n->forward_eager(images, N, image_shapes, bbox_img, det_scores, det_boxes, s); });
}

int xdet_net_forward_u8(void* net, const uint8_t* packed, int64_t packed_bytes, const int64_t* offsets,
                        const int32_t* image_shapes, int N, int resize, float* images, float* bbox_img,
                        float* det_scores, float* det_boxes, int use_graph, void* stream) {
  XDET_LIGHTHEAD(n, net, "net_forward_u8");
  XDET_REQUIRE(n && packed && offsets && image_shapes && images && bbox_img && det_scores && det_boxes,
               "forward_u8: NULL argument");
  XDET_TRY(n->eval_refused("net_forward_u8", /*whole_forward=*/true));   // (ahead of the ingest and of a graph capture)
  XDET_TRY(n->check(N));
  XDET_REQUIRE(resize >= XDET_RESIZE_NONE && resize <= XDET_RESIZE_WARP, "forward_u8: unknown resize mode");
  XDET_REQUIRE(packed_bytes >= 0, "forward_u8: packed_bytes < 0");
  hipStream_t s = S(stream);
  auto run = [&]() {
    XDET_TRY(launch_preprocess_batch(packed, packed_bytes, offsets, image_shapes, N, n->cfg.image_size, resize, images,
                                     bbox_img, s));
    return n->forward_eager(images, N, image_shapes, bbox_img, det_scores, det_boxes, s);
  };
  if (!use_graph) return run();
  XDET_REQUIRE(s != nullptr, "graph replay needs an explicit (non-default) stream");
  // xdet_net_forward's keys carry 0 in the last four slots; resize >= 1 keeps the two apart
  const GraphCache::Key key = {{(uintptr_t)N, (uintptr_t)images, (uintptr_t)image_shapes, (uintptr_t)bbox_img,
                                (uintptr_t)det_scores, (uintptr_t)det_boxes, (uintptr_t)packed, (uintptr_t)packed_bytes,
                                (uintptr_t)offsets, (uintptr_t)resize}};
  return n->graphs.launch(key, s, run);
}

int xdet_net_calibrate(void* net, const float* images, int N, int* n_scaled, void* stream) {
  XDET_LIGHTHEAD(n, net, "net_calibrate");
  return n->calibrate(images, N, S(stream), n_scaled);
}
// (either net type: the list lives in the common Plan base)
int xdet_net_plane_scales(void* net, int max_n, int* n_out, int* exps) {
  XDET_REQUIRE(is_plan(net) && n_out, "plane_scales: bad arguments");
  Plan* n = plan_of(net);
  *n_out = (int)n->pscales.size();
  for (int i = 0; exps && i < max_n && i < *n_out; ++i) exps[i] = n->pscales[i].exp;
  return XDET_OK;
}
int xdet_net_x8_planes(void* net, int* n_on) {
  XDET_REQUIRE(is_plan(net) && n_on, "x8_planes: bad arguments");
  int n = 0;
  for (const auto& p : plan_of(net)->pscales) n += p.x8_ok && p.x8_on;
  *n_on = n;
  return XDET_OK;
}
int xdet_net_plane_scale_name(void* net, int idx, char* buf, int buflen) {
  XDET_REQUIRE(is_plan(net), "plane_scale_name: bad arguments");
  Plan* n = plan_of(net);
  XDET_REQUIRE(buf && buflen > 0 && idx >= 0 && idx < (int)n->pscales.size(), "plane_scale_name: bad arguments");
  snprintf(buf, buflen, "%s", n->pscales[idx].name.c_str());
  return XDET_OK;
}

int xdet_net_graph_count(void* net, int* count) {
  XDET_LIGHTHEAD(n, net, "net_graph_count");
  XDET_REQUIRE(n && count, "graph_count: NULL argument");
  *count = (int)n->graphs.execs.size();
  return XDET_OK;
}

int xdet_net_memory(void* net, size_t* allocated_bytes, size_t* recycled_bytes) {
  XDET_REQUIRE(is_plan(net) && allocated_bytes && recycled_bytes, "net_memory: bad arguments");
  *allocated_bytes = plan_of(net)->allocated_bytes;
  *recycled_bytes = plan_of(net)->ws_recycled_bytes;
  return XDET_OK;
}
int xdet_net_flops_per_image(void* net, double* backbone, double* rpn, double* large_sep, double* head) {
  XDET_LIGHTHEAD(n, net, "net_flops_per_image");
  XDET_REQUIRE(n && n->built, "net not built");
  double f[ST_N] = {};                           // (ST_HEAD_EVAL, the second plan of the same head, is counted nowhere)
  for (const Op& op : n->ops) f[op.stage] += std::max(op.flops, 0.0);
  if (backbone) *backbone = f[ST_BODY] + f[ST_EXIT];
  if (rpn) *rpn = f[ST_RPN];
  if (large_sep) *large_sep = f[ST_LSEP];
  if (head) *head = f[ST_HEAD];
  return XDET_OK;
}

// kind 0 = light-head net, 1 = resnet trunk: the handle must be one
static int as_plan(void* net, int kind, Plan** p) {
  XDET_NET_KIND(net, kind, "profile");
  *p = plan_of(net);
  return XDET_OK;
}
int xdet_profile_enable(void* net, int kind, int enable) {
  Plan* p;
  XDET_TRY(as_plan(net, kind, &p));
  p->profiling = enable != 0;
  return XDET_OK;
}
int xdet_profile_read(void* net, int kind, int max_ops, int* n_ops, double* ms, int* launches, double* flops) {
  XDET_REQUIRE(net && n_ops && ms && launches && flops, "profile_read: NULL argument");
  Plan* p;
  XDET_TRY(as_plan(net, kind, &p));
  return p->profile_read(max_ops, n_ops, ms, launches, flops);
}
int xdet_profile_mfma_flops(void* net, int kind, int max_ops, int* n_ops, double* issued) {
  XDET_REQUIRE(net && n_ops && issued, "profile_mfma_flops: NULL argument");
  Plan* p;
  XDET_TRY(as_plan(net, kind, &p));
  *n_ops = (int)std::min<size_t>(p->ops.size(), (size_t)max_ops);
  const double per_term = g_default_precision == PREC_F16X3 ? 3.0 : 1.0;
  for (int i = 0; i < *n_ops; ++i) {
    const Op& op = p->ops[i];
    issued[i] = op.mfma_flops >= 0.0 ? op.mfma_flops : per_term * std::max(op.flops, 0.0);
  }
  return XDET_OK;
}
int xdet_profile_op_name(void* net, int kind, int op, char* buf, int buflen) {
  XDET_REQUIRE(net && buf && buflen > 0, "profile_op_name: bad arguments");
  Plan* p;
  XDET_TRY(as_plan(net, kind, &p));
  XDET_REQUIRE(op >= 0 && op < (int)p->ops.size(), "profile_op_name: op out of range");
  snprintf(buf, buflen, "%s", p->ops[op].name.c_str());
  return XDET_OK;
}

// ---- resnet trunk ----
int xdet_resnet_create(void** net, int image_size, int max_batch) {
  XDET_REQUIRE(net && image_size >= 64 && max_batch > 0, "resnet_create: bad arguments");
  std::unique_ptr<ResNetTrunk> r(new ResNetTrunk());
  r->plan_kind = 1;
  r->image_size = image_size;
  r->max_batch = max_batch;
  XDET_HIP(hipGetDevice(&r->device));
  *net = r.release();
  return XDET_OK;
}
int xdet_resnet_set_weight(void* net, const char* name, const float* data, int ndim, const int64_t* dims) {
  XDET_RESNET(r, net, "resnet_set_weight");
  return set_weight(r, name, data, ndim, dims);
}
int xdet_resnet_set_option(void* net, const char* key, const char* value) {
  XDET_RESNET(r, net, "resnet_set_option");
  XDET_REQUIRE(r && key && value, "resnet_set_option: NULL argument");
  XDET_REQUIRE(!r->built, "resnet_set_option: the trunk is already built");
  const std::string k(key), v(value);
  XDET_REQUIRE(v == "on" || v == "off", "resnet_set_option: the value must be on | off");
  const bool on = v == "on";
  if (k == "ksplit") r->ksplit_enabled = on;
  else if (k == "stem7") r->stem7_enabled = on;
  else if (k == "stem_pool") r->stem_pool_bn = on;
  else if (k == "bneck") r->bneck_enabled = on;
  else if (k == "projcat") r->projcat_enabled = on;
  else if (k == "preconv") r->preconv_enabled = on;
  else {
    set_last_error("unknown option: " + k);
    return XDET_ERR_INVALID_ARG;
  }
  return XDET_OK;
}
int xdet_resnet_build(void* net) {
  XDET_RESNET(r, net, "resnet_build");
  return r->build();
}
int xdet_resnet_forward(void* net, const float* images, int N, float* out_nhwc, void* stream) {
  XDET_RESNET(r, net, "resnet_forward");
  XDET_REQUIRE(r && r->built && images, "resnet_forward: bad arguments");
  XDET_REQUIRE(N > 0 && N <= r->max_batch, "batch must be in 1..max_batch");
  hipStream_t s = S(stream);
  r->cur_images = images;
  r->bneck_fused_now = r->bneck_all_ok();
  if (!r->stem7_direct) XDET_TRY(launch_nchw_to_nhwc4(images, r->in4.p, N, 3, r->image_size, r->image_size, 4, s));
  XDET_TRY(r->run_stage(0, N, s));
  if (out_nhwc)
    XDET_HIP(hipMemcpyAsync(out_nhwc, r->outb.p, (size_t)N * r->outb.per_image() * 4, hipMemcpyDeviceToDevice, s));
  return XDET_OK;
}
int xdet_resnet_forward_graph(void* net, const float* images, int N, float* out_nhwc, void* stream) {
  XDET_RESNET(r, net, "resnet_forward_graph");
  XDET_REQUIRE(r && r->built && images, "resnet_forward: bad arguments");
  XDET_REQUIRE(N > 0 && N <= r->max_batch, "batch must be in 1..max_batch");
  if (r->profiling) return xdet_resnet_forward(net, images, N, out_nhwc, stream);   // event pairs cannot be replayed
  hipStream_t s = S(stream);
  XDET_REQUIRE(s != nullptr, "graph replay needs an explicit (non-default) stream");
  // (N, images, out, fused forms or not): everything a captured graph bakes in
  const GraphCache::Key key = {{(uintptr_t)N, (uintptr_t)images, (uintptr_t)out_nhwc, (uintptr_t)r->bneck_all_ok(), 0, 0, 0, 0, 0, 0}};
  return r->graphs.launch(key, s, [&]() { return xdet_resnet_forward(net, images, N, out_nhwc, stream); });
}
// activation pre-scale of the trunk's split-precision operands (as xdet_net_calibrate): pre-activation planes
// (bn_relu pass / the previous block's epilogue, whose folded BN carries 2^-e), the inner convs' planes, the strided
// projections' subsample pass
int xdet_resnet_calibrate(void* net, const float* images, int N, int* n_scaled, void* stream) {
  XDET_RESNET(r, net, "resnet_calibrate");
  XDET_REQUIRE(r->built && images && N > 0 && N <= r->max_batch, "resnet_calibrate: bad arguments");
  if (n_scaled) *n_scaled = 0;
  if (r->net_precision == PREC_F32) return XDET_OK;
  r->graphs.clear();                                                  // graphs bake kernel arguments
  return r->calibrate_planes(N, S(stream), n_scaled, [&](hipStream_t st) { return xdet_resnet_forward(net, images, N, nullptr, st); });
}
int xdet_resnet_out_shape(void* net, int* Ho, int* Wo, int* C) {
  XDET_RESNET(r, net, "resnet_out_shape");
  XDET_REQUIRE(r && r->built, "resnet not built");
  *Ho = r->outb.H; *Wo = r->outb.W; *C = r->outb.C;
  return XDET_OK;
}
int xdet_resnet_flops_per_image(void* net, double* flops) {
  XDET_RESNET(r, net, "resnet_flops_per_image");
  XDET_REQUIRE(r && r->built && flops, "resnet not built");
  *flops = r->flops;
  return XDET_OK;
}
int xdet_resnet_destroy(void* net) {
  if (!net) return XDET_OK;
  XDET_RESNET(r, net, "resnet_destroy");
  delete r;
  return XDET_OK;
}

}  // extern "C"
