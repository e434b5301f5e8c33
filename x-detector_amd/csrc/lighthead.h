// The Light-Head R-CNN eval graph (lighr_head_model_fn, light_head_rfcn_eval.py:364-433) as a static launch plan.
#pragma once
#include "merged_layers.h"
#include "plan.h"

namespace xdet {

// ST_EXIT: the exit flow (conv2d_4, blocks 13-14, net/xception_body.py:340-376) -- part of the backbone, its own stage so that
// the RPN branch, which only needs mid_outputs (:339), can fork in front of it
// ST_HEAD_EVAL: the head on all rpn_post_nms_top_n proposals of a net whose ST_HEAD runs on sampled rows (option "eval_head")
enum { ST_BODY = 0, ST_RPN = 1, ST_LSEP = 2, ST_HEAD = 3, ST_EXIT = 4, ST_HEAD_EVAL = 5, ST_N = 6 };

struct LightHeadNet : Plan {
  xdet_lighthead_config cfg;
  bool built = false;
  Buf in4, mid_x, out, rpn_out, feat, pooled, fc, cls_reg;
  float *objectness = nullptr, *rpn_boxes = nullptr, *proposals = nullptr, *head_boxes = nullptr;
  int32_t* pool_index = nullptr;  // [B * R][pooled.ld] argmax sample ids of the head's PsRoiAlign (option "pool_index" = "keep")
  bool keep_pool_index = false;
  // option "head_rois" = "<P>": the head stage is planned on P sampled rows per image (pooled, fc, cls_reg, pool_index) and
  // reads its ROIs from `head_rois` [max_batch, P, 4], corner boxes in the layout of `proposals`; the proposal stage keeps
  // cfg.rpn_post_nms_top_n rows.  0 = off: the head runs on `proposals`.  Such a net has no eval tail (eval_refused)
  // unless it is built with eval_head as well
  int head_rois_n = 0;
  float* head_rois = nullptr;
  // option "eval_head" = "on" (needs head_rois): a second head stage, ST_HEAD_EVAL, on the SAME two layers (hd_head) over its own
  // buffers with cfg.rpn_post_nms_top_n rows per image -- the head plan of a net built without head_rois -- which the whole
  // forward runs on `proposals`; the sampled-row buffers (pooled, fc, cls_reg, pool_index, head_rois) are not touched by it
  bool eval_head = false;
  Buf pooled_eval, fc_eval, cls_reg_eval;
  Buf rpn_hidden;                 // relu(rpn_head/conv2d) as f32 [B,h,w,512] (option "rpn_hidden" = "keep"; p stays NULL without)
  bool keep_rpn_hidden = false;
  Buf entry_x;                    // block 4's sum, the middle flow's input, f32 [B,h,w,728] (option "entry_x" = "keep"; p stays NULL without)
  bool keep_entry_x = false;
  Buf stem_out;                   // relu(BN(block1_conv2)), the entry flow's input, f32 [B,h,w,64] (option "stem_out" = "keep"; p stays NULL without)
  bool keep_stem_out = false;
  float* class_probs = nullptr;   // [B][num_classes][R] softmax of the head's logits, class-major (head_decode_probs_kernel)
  float *anc_yx = nullptr, *anc_hw = nullptr;
  float* mid_relu = nullptr;   // materialised ReLU(x) ("mid_outputs", xception_body.py:339) for API users
  void* prop_ws_mem = nullptr;
  ProposalWorkspace prop_ws;
  int* def_shapes = nullptr;
  float* def_bbox = nullptr;
  int fmap = 0, n_anchor = 0;
  int large_sep_mode = 0;               // 0 = auto, 1 = direct (15,1)/(1,15) convs, 2 = spectral (DFT-domain GEMMs)
  bool large_sep_spectral = false;      // decided at build
  bool spectral_refresh = false;        // option "spectral_refresh" = "off" | "on": refresh_heads takes the large_sep_feature group on a spectral block
  bool rpn_side_stream = true;          // option "rpn_stream" = "side" | "main"
  bool check_range = false;             // option "check_range" = "off" | "on": validate every activation against the f16 range
  bool latency_ksplit = true;           // option "ksplit" = "on" | "off" | "all": fixed split-K for the narrow head GEMM (on),
  bool rpn_ksplit = false;              // ... and the RPN conv as well (all)
  std::vector<std::function<int(int, hipStream_t)>> extra_range_checks;   // tensors that are not plain [N][pixels][ld] (DFT bins)
  bool stem_direct = false;             // block1_conv1 as the dedicated NCHW -> planes kernel
  const float* cur_images = nullptr;
  hipStream_t aux = nullptr;            // side stream of the RPN/proposal branch
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;

  ~LightHeadNet() {
    graphs.clear();              // (before the streams they were captured on)
    // the side stream and its fork / join events (created on the first forward): a net that leaves them behind leaks a
    // hardware queue per instance -- a long test session (~150 nets) ran the runtime out of them and died inside a capture
    if (ev_fork) (void)hipEventDestroy(ev_fork);
    if (ev_join) (void)hipEventDestroy(ev_join);
    if (aux) (void)hipStreamDestroy(aux);
  }

  int build_body();

  int build_rpn();

  // the sizes merged_layers.h describes the three merged groups by (cin: known once build_body has run)
  MergedSizes merged_sizes() const { return {cfg.num_anchors, cfg.num_classes, 512, 2048, out.C, 256, cfg.bank * cfg.grid * cfg.grid}; }
  // a group's conv / dense tensors by role, each checked against its checkpoint shape -> their host arrays
  int need_group(int g, std::initializer_list<std::initializer_list<int64_t>> dims, std::vector<const float*>* by_role) const {
    const std::vector<std::string> names = merged_roles(g);
    size_t role = 0;
    for (const auto& d : dims) {
      const HostTensor* t;
      XDET_TRY(need(names[role++], &t, d));
      by_role->push_back(t->v.data());
    }
    return XDET_OK;
  }

  int large_sep_weights(std::vector<float>* ka, std::vector<float>* ba, std::vector<float>* kb, std::vector<float>* sc,
                        std::vector<float>* sh) const;

  int build_large_sep();

  int build_large_sep_spectral();

  int build_head();

  int build();

  int head_rows() const { return head_rois_n ? head_rois_n : cfg.rpn_post_nms_top_n; }
  const float* head_boxes_in() const { return head_rois_n ? head_rois : proposals; }
  // the eval entries of a net whose head runs on sampled rows: refused ahead of any launch and of a graph capture
  // (whole_forward: xdet_net_forward / _forward_u8, which a net with the option eval_head runs on its second head stage)
  int eval_refused(const char* what, bool whole_forward = false) const {
    if (!head_rois_n || (eval_head && whole_forward)) return XDET_OK;
    if (eval_head) {
      set_last_error(std::string(what) + ": this net was built with the options head_rois=" + std::to_string(head_rois_n) +
                     " and eval_head=on: its eval head runs inside xdet_net_forward / xdet_net_forward_u8 on the buffer "
                     "cls_reg_eval, and this stage entry of the logits form reads cls_reg, which holds the sampled rows; build a "
                     "net without head_rois for the stage entries");
      return XDET_ERR_STATE;
    }
    set_last_error(std::string(what) + ": this net was built with the option head_rois=" + std::to_string(head_rois_n) +
                   " (its head runs on the sampled ROIs of the head_rois buffer, a training net): it has no eval forward and no "
                   "detection tail; build a net without head_rois for those");
    return XDET_ERR_STATE;
  }
  int check(int N) const {
    if (!built) {
      set_last_error("net not built");
      return XDET_ERR_STATE;
    }
    XDET_REQUIRE(N > 0 && N <= max_batch, "batch must be in 1..max_batch");
    return XDET_OK;
  }
  int xception_body(const float* images, int N, hipStream_t s) {
    XDET_TRY(entry_and_middle_flow(images, N, s));
    return run_stage(ST_EXIT, N, s);
  }
  int entry_and_middle_flow(const float* images, int N, hipStream_t s) {      // up to mid_outputs
    XDET_TRY(check(N));
    XDET_REQUIRE(images != nullptr, "images is NULL");
    cur_images = images;         // the stem op reads the NCHW input directly (graphs are keyed on this pointer)
    if (!stem_direct) XDET_TRY(launch_nchw_to_nhwc4(images, in4.p, N, 3, cfg.image_size, cfg.image_size, 4, s));
    return run_stage(ST_BODY, N, s);
  }
  int rpn_decode(int N, hipStream_t s) {
    XDET_TRY(check(N));
    return launch_rpn_decode(rpn_out.p, rpn_out.ld, 0, 2 * cfg.num_anchors, N, fmap, fmap, cfg.num_anchors, anc_yx,
                             anc_hw, objectness, rpn_boxes, s);
  }
  int get_proposals(int N, hipStream_t s) {
    XDET_TRY(check(N));
    return launch_get_proposals(objectness, rpn_boxes, N, n_anchor, cfg.rpn_pre_nms_top_n, cfg.rpn_post_nms_top_n,
                                cfg.rpn_nms_thres, cfg.rpn_min_size, prop_ws, proposals, s);
  }
  int get_head(int N, hipStream_t s) {
    XDET_TRY(check(N));
    const int C = cfg.bank * cfg.grid * cfg.grid;
    XDET_TRY(launch_psroialign(feat.p, head_boxes_in(), pooled.p, pool_index, N, C, feat.H, feat.W, head_rows(),
                               cfg.grid, cfg.grid, 1, 1, feat.ld, pooled.ld, /*corners=*/1, s));
    return run_stage(ST_HEAD, N, s);
  }
  // d loss / d pooled -> d loss / d feat in the layout of `feat`: the order-exact PsRoiAlign gradient on the net's own
  // corner proposals (the sampled ROIs of `head_rois` with that option) and the argmax the last get_head kept
  int head_pool_backward(int N, const float* d_pooled, int ld, float* d_feat, hipStream_t s) {
    XDET_TRY(check(N));
    if (!pool_index) {
      set_last_error("net_head_pool_backward: the net was built with pool_index=off (no argmax to go back through)");
      return XDET_ERR_STATE;
    }
    XDET_REQUIRE(d_pooled && d_feat, "net_head_pool_backward: NULL argument");
    const int C = cfg.bank * cfg.grid * cfg.grid;
    return launch_psroialign_grad_ordered(head_boxes_in(), d_pooled, ld, pool_index, pooled.ld, d_feat, N, C, feat.H, feat.W,
                                          head_rows(), cfg.grid, cfg.grid, 1, 1, feat.ld, /*corners=*/1, s);
  }
  int head_decode(int N, hipStream_t s) {
    XDET_TRY(eval_refused("net_head_decode"));
    XDET_TRY(check(N));
    return launch_ext_decode_rois(proposals, cls_reg.p + cfg.num_classes, cls_reg.ld,
                                  (int64_t)N * cfg.rpn_post_nms_top_n, head_boxes, s);
  }
  // the whole forward's head on a head_rois net (option "eval_head"): all proposals into pooled_eval, no argmax kept
  int get_head_eval(int N, hipStream_t s) {
    XDET_TRY(check(N));
    XDET_REQUIRE(head_rois_n && eval_head && pooled_eval.p, "get_head_eval: the net has no eval head stage");
    const int C = cfg.bank * cfg.grid * cfg.grid;
    XDET_TRY(launch_psroialign(feat.p, proposals, pooled_eval.p, nullptr, N, C, feat.H, feat.W, cfg.rpn_post_nms_top_n,
                               cfg.grid, cfg.grid, 1, 1, feat.ld, pooled_eval.ld, /*corners=*/1, s));
    return run_stage(ST_HEAD_EVAL, N, s);
  }
  // the whole forward: A11 and the softmax A12 starts from in one pass over the ROIs, then A12 from the probabilities
  int head_decode_probs(int N, hipStream_t s) {
    XDET_TRY(check(N));
    const Buf& cls_reg = head_rois_n ? cls_reg_eval : this->cls_reg;       // (rpn_post_nms_top_n rows either way)
    return launch_head_decode_probs(proposals, cls_reg.p, cls_reg.ld, cfg.num_classes, cfg.rpn_post_nms_top_n,
                                    (int64_t)N * cfg.rpn_post_nms_top_n, head_boxes, class_probs, prop_ws.bad, s);
  }
  int bboxes_eval_probs(int N, const int* shapes, const float* bbox, float* ds, float* db, hipStream_t s) {
    XDET_TRY(check(N));
    // more than 1024 ROIs per image (a training net's 1800): the wide form; up to 1024 the launch it always was
    if (cfg.rpn_post_nms_top_n > 1024)
      return launch_bboxes_eval_probs_wide(class_probs, head_boxes, N, cfg.rpn_post_nms_top_n, cfg.num_classes,
                                           shapes ? shapes : def_shapes, bbox ? bbox : def_bbox, cfg.image_size, cfg.image_size,
                                           cfg.select_threshold, cfg.nms_threshold, cfg.nms_topk, ds, db, s, prop_ws.bad);
    return launch_bboxes_eval_probs(class_probs, head_boxes, N, cfg.rpn_post_nms_top_n, cfg.num_classes,
                                    shapes ? shapes : def_shapes, bbox ? bbox : def_bbox, cfg.image_size, cfg.image_size,
                                    cfg.select_threshold, cfg.nms_threshold, cfg.nms_topk, ds, db, s, prop_ws.bad);
  }
  // the stage entry points (xdet_net_head_decode / xdet_net_bboxes_eval): each complete on its own, from "cls_reg" / "head_boxes"
  int bboxes_eval(int N, const int* shapes, const float* bbox, float* ds, float* db, hipStream_t s) {
    XDET_TRY(eval_refused("net_bboxes_eval"));
    XDET_TRY(check(N));
    return launch_bboxes_eval(cls_reg.p, cls_reg.ld, head_boxes, N, cfg.rpn_post_nms_top_n, cfg.num_classes,
                              shapes ? shapes : def_shapes, bbox ? bbox : def_bbox, cfg.image_size, cfg.image_size,
                              cfg.select_threshold, cfg.nms_threshold, cfg.nms_topk, ds, db, s, prop_ws.bad);
  }
  int mid_refresh(int N, hipStream_t s);
  // xdet_net_refresh_weights: the body's blocks 2-14 from trained weights in device memory, through layer_recs
  int refresh_weights(const xdet_net_weight_dev* table, int n, hipStream_t s);
  BodyRefreshScratch rf;                            // one block for the whole reach, allocated at the first refresh; the folds
  std::vector<size_t> rf_off;                       // of a record's channels at rf.scale / rf.shift + rf_off[record]
  int scale_read_back(ConvLayer* L);
  // xdet_net_refresh_stem: block1_conv1 and block1_conv2 from trained weights in device memory.  The direct-form stem keeps
  // no layer: the net holds its kernel's device copy, its folded batch norm at exponent 0 and the plane the exponent belongs to
  int refresh_stem(const xdet_net_weight_dev* table, int n, hipStream_t s);
  BodyRefreshScratch rf_stem;                       // one block, allocated at the first call: conv1's channels, then conv2's
  Pow2Scaled stem_sc, stem_sh;
  float* stem_w = nullptr;
  int stem_pidx = -1;
  static constexpr float stem_eps = 1e-4f;          // net/xception_body.py:20
  // xdet_net_refresh_heads: the layers the plan owns -- the RPN head's two, the head's two dense layers and (direct form) the
  // large-separable block's two -- from the checkpoint's tensors in device memory.  hd_*: the layers, set by the builders
  // (hd_lsep stays NULL in the spectral form; hd_spec: that form's two layers, kept with option "spectral_refresh" = "on" only);
  // hs, hs_k: the merges' scratch, allocated at the first call (that names the block)
  int refresh_heads(const xdet_net_weight_dev* table, int n, hipStream_t s);
  ConvLayer *hd_rpn[2] = {nullptr, nullptr}, *hd_head[2] = {nullptr, nullptr}, *hd_lsep[2] = {nullptr, nullptr};
  SpectralConv* hd_spec[2] = {nullptr, nullptr};
  HeadsRefreshScratch hs;
  LargeSepKernelScratch hs_k;
  int calibrate(const float* images, int N, hipStream_t s, int* n_scaled);
  int forward_eager(const float* images, int N, const int* shapes, const float* bbox, float* ds, float* db,
                    hipStream_t s);
};

}  // namespace xdet
