// LightHeadNet: the builders of the Xception body, the RPN branch, the large-separable convs and the head, and the
// whole forward.
#include "lighthead.h"

namespace xdet {

static inline double nsplit_of(const ConvLayer* L) { return L->precision == PREC_F16X3 ? 3.0 : 1.0; }

int LightHeadNet::build_body() {
  const float eps = 1e-4f;   // net/xception_body.py:20
  const int S = cfg.image_size;
  in4.H = S; in4.W = S; in4.C = 3;
  XDET_TRY(new_buf(S, S, 3, &in4));
  Buf x, r, t;
  if (g_default_precision != PREC_F32) {
    // stem conv straight from the NCHW input to the planes block1_conv2 reads (elementwise.hip): K = 27 fits no
    // matrix-core shape, a VALU kernel with scalar-cache weights is HBM-bound instead of gather-bound
    const HostTensor* kt;
    XDET_TRY(need("block1_conv1/kernel", &kt, {3, 3, 3, 32}));
    std::vector<float> sc, sh;
    float *d_w, *d_sc, *d_sh;
    XDET_TRY(upload(kt->v, &d_w));
    XDET_TRY(upload_bn("block1_conv1_bn", 32, 32, eps, &sc, &sh, &d_sc, &d_sh));
    x = Buf();
    x.H = x.W = (S - 3) / 2 + 1; x.C = 32; x.ld = 32; x.no_f32 = true;
    XDET_TRY(new_planes(&x));
    pscales[x.pidx].name = "block1_conv1 [stem]";
    // (members: xdet_net_refresh_stem replaces the host vectors behind them and uploads again at the plane's exponent)
    stem_sc = Pow2Scaled{sc, d_sc}; stem_sh = Pow2Scaled{sh, d_sh};
    stem_w = d_w; stem_pidx = x.pidx;
    pscales[x.pidx].apply.push_back([this](int e) {  // relu(x*sc + sh) * 2^-e = relu(x*(sc 2^-e) + sh 2^-e), exactly
      XDET_TRY(stem_sc.upload(-e));
      return stem_sh.upload(-e);
    });
    const Buf o = x;
    stem_direct = true;
    ops.push_back({"block1_conv1 [stem, NCHW in]", ST_BODY, 2.0 * o.H * o.W * 27.0 * 32.0, [=](int N, hipStream_t st) {
                     return launch_stem_conv3x3s2(cur_images, d_w, d_sc, d_sh, o.hi, o.lo, N, S, st);
                   }});
    ops.back().mfma_flops = 0.0;      // VALU kernel
  } else {
    ConvArgs c1;
    c1.k = 3; c1.cout = 32; c1.stride = 2; c1.pad_mode = 0; c1.relu_out = 1;
    XDET_TRY(conv_bn("block1_conv1", "block1_conv1_bn", eps, ST_BODY, in4, c1, &x));
  }
  ConvArgs c2;
  c2.k = 3; c2.cout = 64; c2.pad_mode = 0; c2.relu_out = 1;
  XDET_TRY(conv_bn("block1_conv2", "block1_conv2_bn", eps, ST_BODY, x, c2, &t));
  XDET_REQUIRE(!keep_stem_out || (t.p && !t.no_f32), "plan: stem_out=keep, but block1_conv2 writes no f32 output");
  x = t;
  struct Blk { const char* res; const char* bn; const char* s1; const char* s2; int c; int first_relu; };
  const Blk blks[3] = {{"conv2d_1", "batch_normalization_1", "block2_sepconv1", "block2_sepconv2", 128, 0},
                       {"conv2d_2", "batch_normalization_2", "block3_sepconv1", "block3_sepconv2", 256, 1},
                       {"conv2d_3", "batch_normalization_3", "block4_sepconv1", "block4_sepconv2", 728, 1}};
  Buf presub;                                    // raw subsampled planes of x, written by the pool pass that produced x
  bool x_is_relu = false;                        // ... which then stored x as relu(x)
  for (int bi = 0; bi < 3; ++bi) {
    const Blk& b = blks[bi];
    ConvArgs proj;                                 // 1x1 / stride 2 / SAME
    proj.cout = b.c; proj.stride = 2;
    if (presub.hi) proj.presub = &presub;
    XDET_TRY(conv_bn(b.res, b.bn, eps, ST_BODY, x, proj, &r));
    Buf a, p;
    // relu -> sepconv2 (net/xception_body.py:271-277) is the ONLY consumer of sepconv1's BN output: the ReLU is taken
    // in sepconv1's epilogue (one v_max per element on its way out) instead of on sepconv2's 3 x 3 window reads (72 of
    // the stencil's 192 VALU instructions per chunk when the block runs as the fused kernel) -- the same values
    SepArgs s1;
    s1.cout = b.c; s1.pre_relu = x_is_relu ? 0 : b.first_relu; s1.relu_out = 1;
    XDET_TRY(sep_bn(b.s1, eps, ST_BODY, x, s1, &a));
    // The pooled sum of blocks 2 and 3 is read by exactly two consumers, the next block's projection (raw, every second
    // pixel) and its sepconv1 (through a ReLU): where the pool runs as the split vertical pass it writes both forms.
    // (Block 4's sum is the middle flow's residual stream: it stays raw.)
    Buf nsub;
    const bool two_readers = bi < 2 && pool_writes_projection_input && subsample_projections &&
                             g_default_precision != PREC_F32 && b.c % 32 == 0;
    SepArgs s2;
    s2.cout = b.c; s2.pool_res = &r;
    if (two_readers) s2.next_sub = &nsub;
    XDET_TRY(sep_bn(b.s2, eps, ST_BODY, a, s2, &p));
    presub = nsub;
    x_is_relu = nsub.hi != nullptr;
    if (bi == 0 && keep_stem_out) stem_out = x;  // a named buffer: never handed back to the pool
    else release_f32(x);                         // the block input: read by the projection and sepconv1
    release_f32(a);
    release_f32(r);
    x = p;
  }
  for (int blk = 5; blk <= 12; ++blk) {
    const Buf res = x;
    Buf a, b2, c3;
    const std::string pre = "block" + std::to_string(blk);
    SepArgs sep;                                   // ReLU -> 728-wide separable conv -> BN
    sep.cout = 728; sep.pre_relu = 1;
    XDET_TRY(sep_bn(pre + "_sepconv1", eps, ST_BODY, x, sep, &a));
    XDET_TRY(sep_bn(pre + "_sepconv2", eps, ST_BODY, a, sep, &b2));
    sep.res = &res;
    if (blk == 12) sep.emit.planes = 2;            // mid_outputs = ReLU(this) feeds the RPN 3x3 conv (relu planes)
    XDET_TRY(sep_bn(pre + "_sepconv3", eps, ST_BODY, b2, sep, &c3));
    release_f32(a);                              // a block's three tensors die with it: the middle flow lives in four
    release_f32(b2);                             // f32 blocks and one planes pair instead of 24 + 24
    if (blk == 5 && keep_entry_x) entry_x = res;   // a named buffer: never handed back to the pool
    else release_f32(res);
    x = c3;
  }
  mid_x = x;   // mid_outputs = ReLU(mid_x); consumers apply the ReLU on load
  ConvArgs proj4;
  proj4.cout = 1024;
  XDET_TRY(conv_bn("conv2d_4", "batch_normalization_4", eps, ST_EXIT, x, proj4, &r));
  Buf a, b2, c3, d4;
  SepArgs s13;
  s13.cout = 728; s13.pre_relu = 1;
  XDET_TRY(sep_bn("block13_sepconv1", eps, ST_EXIT, x, s13, &a));
  s13.cout = 1024; s13.res = &r;
  XDET_TRY(sep_bn("block13_sepconv2", eps, ST_EXIT, a, s13, &b2));
  SepArgs s14;                                     // :354-364
  s14.cout = 1536; s14.dilation = 2; s14.relu_out = 1;
  XDET_TRY(sep_bn("block14_sepconv1", eps, ST_EXIT, b2, s14, &c3));
  // The large-separable convs run either as direct implicit GEMMs over split planes or in the DFT domain
  // (spectral.hip: ~6x fewer MFMA FLOPs; one GEMM per frequency bin with M = N*fmap rows).  The spectral form
  // wins at every batch size -- at one image the direct (15,1) conv is a 900-row GEMM with K = 30,720 on 32
  // workgroups (0.9 ms), the 19 bins are 304 workgroups of 64 x 64 tiles with K = 4,096 -- so `auto` takes it whenever the
  // feature-map size has a transform instantiated.  Decided per NET, never per call: an image's result
  // does not depend on the batch it arrives in.
  large_sep_spectral = g_default_precision != PREC_F32 && spectral_supported(c3.H) && c3.H == c3.W && large_sep_mode != 1;
  if (large_sep_mode == 2) XDET_REQUIRE(large_sep_spectral, "large_sep=spectral needs a split-precision mode and a 16/30/50 feature map");
  // :366-376; the direct (15,1) conv takes planes, the DFT pass reads f32
  s14.cout = 2048; s14.emit.planes = large_sep_spectral ? 0 : 1;
  XDET_TRY(sep_bn("block14_sepconv2", eps, ST_EXIT, c3, s14, &d4));
  release_f32(a);
  release_f32(r);
  release_f32(b2);
  release_f32(c3);
  out = d4;
  fmap = out.H;
  return XDET_OK;
}

int LightHeadNet::build_rpn() {
  struct PoolGuard { int& p; int old; ~PoolGuard() { p = old; } } pool_guard{ws_pool, ws_pool};
  ws_pool = rpn_side_stream ? 1 : 0;      // the branch runs beside the exit flow: no workspace block shared with the main stream
  const MergedSizes z = merged_sizes();
  const int A = z.A, hw = z.hid;
  std::vector<const float*> t;
  XDET_TRY(need_group(MG_RPN, {{3, 3, 728, hw}, {hw}, {1, 1, hw, 2 * A}, {2 * A}, {1, 1, hw, 4 * A}, {4 * A}}, &t));
  ConvLayer* L0 = keep(new ConvLayer());
  XDET_TRY(L0->init(3, 3, 728, hw, 1, 1, 1, 0, 0, t[HEAD_K0], nullptr, t[HEAD_B0], 1));
  Buf hid;
  ConvEmit hid_emit;
  // only the fused 1x1 heads read it: planes alone -- unless the RPN's backward wants the f32 tensor for its ReLU mask
  hid_emit.planes = keep_rpn_hidden ? 1 : 3;
  // (a single image is 8 x 4 tiles against 207 K steps.  Fixed split-K -- option "ksplit" = "all" -- takes it from 116 to
  //  37 us, but costs the 256 x 256 tile at bench-size batches: 1.92 -> 2.36 ms per 128 images, -0.9 % end to end.
  //  With the fork in front of the exit flow the conv is off the critical path of a single image anyway.)
  hid_emit.ksplit = latency_ksplit && rpn_ksplit;
  XDET_TRY(add_conv("rpn_head/conv2d", ST_RPN, mid_x, L0, nullptr, /*relu_in=*/1, &hid, hid_emit));
  if (keep_rpn_hidden) rpn_hidden = hid;      // a named buffer: never handed back to the pool
  // cls (2A) and box (4A) 1x1 heads share their input: one GEMM over the concatenated filters
  const std::vector<MergedSlot> slots = merged_slots(MG_RPN, z);
  const std::vector<float> kc = merged_concat(slots[SLOT_K], t.data()), bc = merged_concat(slots[SLOT_B], t.data());
  ConvLayer* L1 = keep(new ConvLayer());
  XDET_TRY(L1->init(1, 1, hw, (int)slots[SLOT_K].W(), 1, 1, 1, 0, 0, kc.data(), nullptr, bc.data(), 0));
  XDET_TRY(add_conv("rpn_head/conv2d_1+2", ST_RPN, hid, L1, nullptr, 0, &rpn_out));
  hd_rpn[0] = L0; hd_rpn[1] = L1;
  return XDET_OK;
}

// The large-separable block's weights (net/xception_body.py:450-475) with its two branches fused: both (15,1) convs read
// the same input -> ONE conv with the filters concatenated (2*mid outputs: ka, ba); branch_0b + branch_1b = ONE (1,15) conv
// over the 2*mid stacked channels (kb), whose bias sum is folded into the BN(1e-5) + ReLU behind it (sc, sh)
int LightHeadNet::large_sep_weights(std::vector<float>* ka, std::vector<float>* ba, std::vector<float>* kb, std::vector<float>* sc,
                                    std::vector<float>* sh) const {
  const MergedSizes z = merged_sizes();
  const int cin = z.cin, mid = z.mid, co = z.co;
  std::vector<const float*> t;
  XDET_TRY(need_group(MG_LSEP, {{15, 1, cin, mid}, {mid}, {1, 15, mid, co}, {co}, {15, 1, cin, mid}, {mid}, {1, 15, mid, co}, {co}}, &t));
  const std::vector<MergedSlot> slots = merged_slots(MG_LSEP, z);
  *ka = merged_concat(slots[SLOT_KA], t.data());
  *ba = merged_concat(slots[SLOT_BA], t.data());
  *kb = merged_concat(slots[SLOT_KB], t.data());
  std::vector<float> bsum(co);
  for (int j = 0; j < co; ++j) bsum[j] = t[LSEP_B0][j] + t[LSEP_B1][j];
  return fold_bn("large_sep_feature/batch_normalization", co, 1e-5f, bsum.data(), sc, sh);
}

int LightHeadNet::build_large_sep() {
  const MergedSizes z = merged_sizes();
  const int mid2 = (int)merged_slots(MG_LSEP, z)[SLOT_KA].W(), co = z.co;
  std::vector<float> ka, ba, kb, sc, sh;
  XDET_TRY(large_sep_weights(&ka, &ba, &kb, &sc, &sh));
  ConvLayer* LA = keep(new ConvLayer());
  XDET_TRY(LA->init(15, 1, out.C, mid2, 1, 1, 1, 0, 0, ka.data(), nullptr, ba.data(), 0));
  Buf t;
  // only the (1,15) conv reads it: planes only
  XDET_TRY(add_conv("large_sep_feature/Branch_0+1/conv2d", ST_LSEP, out, LA, nullptr, 0, &t, ConvEmit{3}));
  ConvLayer* LB = keep(new ConvLayer());
  XDET_TRY(LB->init(1, 15, mid2, co, 1, 1, 1, 0, 0, kb.data(), sc.data(), sh.data(), 1));
  XDET_TRY(add_conv("large_sep_feature/Branch_0+1/conv2d_1", ST_LSEP, t, LB, nullptr, 0, &feat));
  hd_lsep[0] = LA; hd_lsep[1] = LB;
  return XDET_OK;
}

// net/xception_body.py:450-475 in the DFT domain of the convolved axis (spectral.hip): per frequency bin one
// real GEMM [N*F, 2*Cin] x [2*Cin, 2*Cout] on the split-precision MFMA kernel (grouped launch), a forward
// DFT pass in front and an inverse pass (+bias / +BN+ReLU) behind each of the two convolutions
int LightHeadNet::build_large_sep_spectral() {
  const MergedSizes z = merged_sizes();
  const int co = z.co, F = out.H, cin = z.cin, mid2 = (int)merged_slots(MG_LSEP, z)[SLOT_KA].W();
  // the same branch fusion as the direct form: (15,1) with 2*mid outputs, (1,15) over the stacked channels
  std::vector<float> ka, kb, ba, sc, sh;
  XDET_TRY(large_sep_weights(&ka, &ba, &kb, &sc, &sh));
  // (15,1) + bias along y, then (1,15) + BN + ReLU along x: the layer the C ABI exposes as xdet_spectral_conv_*
  SpectralConv* SA = keep(new SpectralConv());
  SpectralConv* SB = keep(new SpectralConv());
  XDET_TRY(SA->init(ka.data(), 15, cin, mid2, 0, F, nullptr, ba.data(), 0));
  XDET_TRY(SB->init(kb.data(), 15, mid2, co, 1, F, sc.data(), sh.data(), 1));
  XDET_REQUIRE(SA->cin_ld == out.ld && SA->cout_ld == mid2, "plan: the spectral convs' channel strides");
  if (spectral_refresh) { hd_spec[0] = SA; hd_spec[1] = SB; }
  const int NB = SA->NB, cin_ld = SA->cin_ld, co_ld = SB->cout_ld;
  // workspace, sized for max_batch: rows of every bin are padded to a whole number of 256-row GEMM tiles
  const size_t mp_max = (size_t)round_up(max_batch * F, 256), rows = (size_t)NB * mp_max;
  auto mpad = [F](int N) { return SpectralConv::m_pad(F, N); };
  unsigned short *xa_hi, *xa_lo, *xb_hi, *xb_lo;
  float *y1, *tmid, *y2;
  XDET_TRY(alloc_bytes(rows * 2 * cin_ld * 2 + 512, reinterpret_cast<void**>(&xa_hi)));
  XDET_TRY(alloc_bytes(rows * 2 * cin_ld * 2 + 512, reinterpret_cast<void**>(&xa_lo)));
  XDET_TRY(alloc_bytes(rows * 2 * mid2 * 2 + 512, reinterpret_cast<void**>(&xb_hi)));
  XDET_TRY(alloc_bytes(rows * 2 * mid2 * 2 + 512, reinterpret_cast<void**>(&xb_lo)));
  XDET_TRY(alloc_bytes(rows * 2 * mid2 * 4 + 512, reinterpret_cast<void**>(&y1)));
  XDET_TRY(alloc_bytes((size_t)max_batch * F * F * mid2 * 4 + 512, reinterpret_cast<void**>(&tmid)));
  XDET_TRY(alloc_bytes(rows * 2 * co_ld * 4 + 512, reinterpret_cast<void**>(&y2)));
  XDET_TRY(new_buf(F, F, co, &feat));
  const Buf o = out, ft = feat;
  // check_range covers the DFT-domain tensors too.  A bin sums up to F samples (the DC bin all of them), so the f16
  // range of the planes is reached at activations of ~65504 / F, and tmid is an un-normalised 15-tap conv output:
  // this is where a checkpoint with large activations would overflow first.
  f32_bufs.emplace_back(tmid, (size_t)F * F * mid2);
  // (prop_ws.bad is carved later, in build(): the lambda reads it through `this` at call time)
  extra_range_checks.push_back([=](int N, hipStream_t s) {
    const int mp = mpad(N);
    XDET_TRY(launch_range_check_planes(xa_hi, N, F, 2 * cin_ld, prop_ws.bad, s, NB, mp));
    XDET_TRY(launch_range_check_planes(xb_hi, N, F, 2 * mid2, prop_ws.bad, s, NB, mp));
    // the per-bin products are f32 and never split: NaN / inf only
    XDET_TRY(launch_range_check(y1, N, (size_t)F * 2 * mid2, 3.4028235e38f, prop_ws.bad, s, NB, (size_t)mp * 2 * mid2));
    return launch_range_check(y2, N, (size_t)F * 2 * co_ld, 3.4028235e38f, prop_ws.bad, s, NB, (size_t)mp * 2 * co_ld);
  });
  const std::string pre = "large_sep_feature/Branch_0+1/";
  {
    // activation pre-scale of the DFT-domain operands (SpectralConv::set_in_exp).  These are the tensors with the least
    // headroom: a bin sums up to F samples, and the second one transforms an un-normalised 15-tap conv output.
    PlaneScale pa, pb;
    pa.name = pre + "conv2d/dft_y (DFT-domain planes)";
    pa.hi = xa_hi;
    pa.halves = [=](int N) { return (int64_t)SA->planes_halves(N); };
    pa.apply.push_back([=](int e) { return SA->set_in_exp(e); });
    pb.name = pre + "conv2d_1/dft_x (DFT-domain planes)";
    pb.hi = xb_hi;
    pb.halves = [=](int N) { return (int64_t)SB->planes_halves(N); };
    pb.apply.push_back([=](int e) { return SB->set_in_exp(e); });
    // rows [N*F, m_pad) of a bin are padding that only an earlier, larger batch ever wrote: a measurement over
    // whole bins must not see that batch's (possibly overflowed) values
    const size_t bytes_a = rows * 2 * cin_ld * 2, bytes_b = rows * 2 * mid2 * 2;
    pa.clear = [=](hipStream_t st) { XDET_HIP(hipMemsetAsync(xa_hi, 0, bytes_a, st)); return (int)XDET_OK; };
    pb.clear = [=](hipStream_t st) { XDET_HIP(hipMemsetAsync(xb_hi, 0, bytes_b, st)); return (int)XDET_OK; };
    pscales.push_back(pa);
    pscales.push_back(pb);
  }
  const double fl_a = 2.0 * F * F * (double)cin * mid2 * 15, fl_b = 2.0 * F * F * (double)mid2 * co * 15;
  // flops < 0 marks an auxiliary pass of a contraction: its time counts with the conv kernels, it has no FLOPs of its own
  ops.push_back({pre + "conv2d/dft_y", ST_LSEP, -1.0, [=](int N, hipStream_t s) { return SA->dft_fwd(o.p, N, xa_hi, xa_lo, s); }});
  ops.push_back({pre + "conv2d [spectral]", ST_LSEP, fl_a, [=](int N, hipStream_t s) { return SA->gemm(N, xa_hi, xa_lo, y1, s); }});
  ops.back().mfma_flops = 2.0 * nsplit_of(&SA->G) * NB * (double)F * (2.0 * cin_ld) * (2.0 * mid2);
  ops.push_back({pre + "conv2d/idft_y+bias", ST_LSEP, -1.0, [=](int N, hipStream_t s) { return SA->dft_inv(N, y1, tmid, mid2, s); }});
  ops.push_back({pre + "conv2d_1/dft_x", ST_LSEP, -1.0, [=](int N, hipStream_t s) { return SB->dft_fwd(tmid, N, xb_hi, xb_lo, s); }});
  ops.push_back({pre + "conv2d_1 [spectral]", ST_LSEP, fl_b, [=](int N, hipStream_t s) { return SB->gemm(N, xb_hi, xb_lo, y2, s); }});
  ops.back().mfma_flops = 2.0 * nsplit_of(&SB->G) * NB * (double)F * (2.0 * mid2) * (2.0 * co_ld);
  ops.push_back({pre + "conv2d_1/idft_x+bn+relu", ST_LSEP, -1.0, [=](int N, hipStream_t s) { return SB->dft_inv(N, y2, ft.p, ft.ld, s); }});
  return XDET_OK;
}

int LightHeadNet::build_head() {
  const MergedSizes z = merged_sizes();
  // (the rows of the head stage: the sampled ROIs per image with the option head_rois, else the proposals -- the same
  //  layers and ConvEmit constants either way, so head_rois = P plans what a net built with rpn_post_nms_top_n = P plans)
  const int R = head_rows(), C = z.co, nc = z.nc, fw = z.fcw;
  // With the option eval_head the sampled-row stage's tensors get blocks of their own instead of ones the body has handed back:
  // a training step's pooled, fc and cls_reg then survive an eval forward, whose body would otherwise write through them
  // (1 MiB at 64 rows and 256 pixels).  Without the option the plan is the one it always was.
  struct ReuseGuard { bool& r; bool old; ~ReuseGuard() { r = old; } } reuse_guard{reuse_workspace, reuse_workspace};
  if (eval_head) reuse_workspace = false;
  std::vector<const float*> t;
  XDET_TRY(need_group(MG_HEAD, {{C, fw}, {fw}, {fw, nc}, {nc}, {fw, 4}, {4}}, &t));
  // ROI rows are the GEMM M dimension: treat [N*R, C] as an NHWC tensor with H = R, W = 1
  XDET_TRY(new_buf(R, 1, C, &pooled));
  if (keep_pool_index) XDET_TRY(alloc_bytes((size_t)max_batch * R * pooled.ld * sizeof(int32_t), reinterpret_cast<void**>(&pool_index)));
  ConvLayer* L0 = keep(new ConvLayer());
  XDET_TRY(L0->init(1, 1, C, fw, 1, 1, 0, 0, 0, t[HEAD_K0], nullptr, t[HEAD_B0], 1));
  XDET_TRY(add_conv("final_head/subnet_fc", ST_HEAD, pooled, L0, nullptr, 0, &fc, ConvEmit{1}));
  const std::vector<MergedSlot> slots = merged_slots(MG_HEAD, z);
  const std::vector<float> kc = merged_concat(slots[SLOT_K], t.data()), bc = merged_concat(slots[SLOT_B], t.data());
  ConvLayer* L1 = keep(new ConvLayer());
  XDET_TRY(L1->init(1, 1, fw, (int)slots[SLOT_K].W(), 1, 1, 0, 0, 0, kc.data(), nullptr, bc.data(), 0));
  ConvEmit cls_emit;
  cls_emit.ksplit = latency_ksplit;     // 300 rows x 25 outputs: 3 tiles against 64 K steps
  XDET_TRY(add_conv("final_head/fc_cls+fc_loc", ST_HEAD, fc, L1, nullptr, 0, &cls_reg, cls_emit));
  hd_head[0] = L0; hd_head[1] = L1;
  if (!eval_head) return XDET_OK;
  reuse_workspace = reuse_guard.old;      // (the eval stage takes recycled blocks as the head of a net without head_rois does)
  // The eval stage of a head_rois net: the same two layers, names and ConvEmit constants over buffers of
  // cfg.rpn_post_nms_top_n rows -- what the lines above plan on a net without head_rois.  A layer's split-K form is a constant
  // of the layer, and maybe_ksplit takes it from the buffer's extent: the two extents must come to the same form, or the
  // shared layer would compute one of the two stages on another summation tree than the net it stands for.
  struct KsForm { int ksplit; bool narrow; int64_t tiles; int mode; };
  auto form_of = [](const ConvLayer* L) { return KsForm{L->ksplit, L->ks_narrow, L->ks_tiles, L->ks_mode}; };
  auto same = [](const KsForm& a, const KsForm& b) { return a.ksplit == b.ksplit && a.narrow == b.narrow && a.tiles == b.tiles && a.mode == b.mode; };
  const KsForm f0 = form_of(L0), f1 = form_of(L1);
  const size_t n_ks = ks_layers.size();
  XDET_TRY(new_buf(cfg.rpn_post_nms_top_n, 1, C, &pooled_eval));
  XDET_TRY(add_conv("final_head/subnet_fc [eval]", ST_HEAD_EVAL, pooled_eval, L0, nullptr, 0, &fc_eval, ConvEmit{1}));
  XDET_TRY(add_conv("final_head/fc_cls+fc_loc [eval]", ST_HEAD_EVAL, fc_eval, L1, nullptr, 0, &cls_reg_eval, cls_emit));
  ks_layers.resize(n_ks);                 // (the layers are listed once: finish_ksplit binds a layer's slab, not a stage's)
  XDET_REQUIRE(same(f0, form_of(L0)) && same(f1, form_of(L1)),
               "eval_head: the head's dense layers come to another split-K form on rpn_post_nms_top_n rows than on head_rois rows; "
               "the two stages cannot share their layers at these sizes");
  return XDET_OK;
}

int LightHeadNet::build() {
  XDET_REQUIRE(!built, "net already built");
  XDET_REQUIRE(cfg.max_batch > 0 && cfg.image_size >= 64, "bad max_batch / image_size");
  XDET_REQUIRE(head_rois_n == 0 || (head_rois_n >= 1 && head_rois_n <= cfg.rpn_post_nms_top_n),
               "head_rois must be off or in 1..rpn_post_nms_top_n");
  XDET_REQUIRE(!eval_head || head_rois_n, "eval_head=on needs the option head_rois=<P>: a net without head_rois runs its one head "
                                          "stage on all proposals already");
  XDET_REQUIRE(cfg.num_anchors == 22, "anchor table is the reference's 22-anchor set (1 extra + 7 scales x 3 ratios)");
  max_batch = cfg.max_batch;
  net_precision = g_default_precision;
  ksplit_design_batch = 1;            // the reference evaluates single images (light_head_rfcn_eval.py:212); only layers a
  ksplit_all = false;                 // builder marks (ConvEmit::ksplit) are split
  XDET_TRY(build_body());
  XDET_TRY(build_rpn());
  XDET_TRY(large_sep_spectral ? build_large_sep_spectral() : build_large_sep());
  XDET_TRY(build_head());
  XDET_TRY(finish_ksplit());
  const int B = max_batch, A = cfg.num_anchors, R = cfg.rpn_post_nms_top_n;
  n_anchor = fmap * fmap * A;
  // A5: AnchorCreator.get_layer_anchors (anchor_manipulator.py:698-757), layer_step 16, offset .5
  std::vector<float> yx((size_t)fmap * fmap * 2), hw((size_t)A * 2);
  for (int y = 0; y < fmap; ++y)
    for (int x = 0; x < fmap; ++x) {
      yx[((size_t)y * fmap + x) * 2 + 0] = ((float)y + 0.5f) * 16.f / (float)cfg.image_size;
      yx[((size_t)y * fmap + x) * 2 + 1] = ((float)x + 0.5f) * 16.f / (float)cfg.image_size;
    }
  {
    int a = 0;
    hw[0] = 0.1f; hw[1] = 0.1f; ++a;
    const double scales[7] = {0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8}, ratios[3] = {1., 2., .5};
    for (double sc : scales)
      for (double ra : ratios) {
        hw[a * 2 + 0] = (float)(sc / std::sqrt(ra));
        hw[a * 2 + 1] = (float)(sc * std::sqrt(ra));
        ++a;
      }
  }
  XDET_TRY(upload(yx, &anc_yx));
  XDET_TRY(upload(hw, &anc_hw));
  XDET_TRY(alloc_bytes((size_t)B * n_anchor * 4, reinterpret_cast<void**>(&objectness)));
  XDET_TRY(alloc_bytes((size_t)B * n_anchor * 16, reinterpret_cast<void**>(&rpn_boxes)));
  XDET_TRY(alloc_bytes((size_t)B * R * 16, reinterpret_cast<void**>(&proposals)));
  if (head_rois_n) XDET_TRY(alloc_bytes((size_t)B * head_rois_n * 16, reinterpret_cast<void**>(&head_rois)));
  XDET_TRY(alloc_bytes((size_t)B * R * 16, reinterpret_cast<void**>(&head_boxes)));
  XDET_TRY(alloc_bytes((size_t)B * cfg.num_classes * R * 4, reinterpret_cast<void**>(&class_probs)));
  XDET_TRY(alloc_bytes((size_t)B * mid_x.per_image() * 4, reinterpret_cast<void**>(&mid_relu)));
  XDET_TRY(alloc_bytes(ws_measure(256, proposal_workspace_layout, B, n_anchor, cfg.rpn_pre_nms_top_n, R), &prop_ws_mem));
  prop_ws = ws_carve(prop_ws_mem, 256, proposal_workspace_layout, B, n_anchor, cfg.rpn_pre_nms_top_n, R);
  std::vector<int> shp((size_t)B * 2, cfg.image_size);
  std::vector<float> bb((size_t)B * 4);
  for (int i = 0; i < B; ++i) { bb[i * 4] = 0.f; bb[i * 4 + 1] = 0.f; bb[i * 4 + 2] = 1.f; bb[i * 4 + 3] = 1.f; }
  XDET_TRY(upload(shp, &def_shapes));
  XDET_TRY(upload(bb, &def_bbox));
  w.clear();   // host copies are no longer needed
  built = true;
  return XDET_OK;
}

// Everything the net keeps of mid_x besides the f32 tensor, re-derived from it: the ReLU split planes block12_sepconv3's
// epilogue wrote for the RPN 3x3 conv (the pass Plan::add_split would plan for this Buf, at the planes' own scale and form)
// and the materialised `mid` buffer.  In f32 mode, or where the RPN conv makes its own planes per call, only the copy runs.
int LightHeadNet::mid_refresh(int N, hipStream_t s) {
  XDET_TRY(check(N));
  if (mid_x.hi) {
    XDET_REQUIRE(mid_x.planes_relu && !mid_x.no_f32, "net_mid_refresh: mid_x's planes are not the ReLU planes of an f32 tensor");
    int x8_exp = 0;
    const int x8 = plane_x8(mid_x.pidx, &x8_exp) ? 1 : 0;
    XDET_TRY(launch_split_f32(mid_x.p, mid_x.hi, mid_x.lo, (int64_t)N * mid_x.H * mid_x.W, mid_x.ld, /*relu=*/1, s,
                              pmul(mid_x.pidx), x8, x8_exp));
  }
  return launch_relu_copy(mid_x.p, mid_relu, (int64_t)N * mid_x.per_image(), s);
}

// The name table of a refresh door (xdet_net_refresh_weights, xdet_net_refresh_heads): groups[g] holds a group's label and its
// tensors' names by role.  -> given[g][role], the table's pointers; given[g] stays empty for a group the table does not name.
// Refused, in this order: a NULL name, a name outside the reach, a NULL pointer, a name given twice; then, over the groups
// and roles in order, a group given in part.
struct NameGroup {
  std::string label;
  std::vector<std::string> names;
};
static int parse_weight_table(const std::string& door, const char* reach, const std::vector<NameGroup>& groups,
                              const xdet_net_weight_dev* table, int n, std::vector<std::vector<const float*>>* given) {
  std::map<std::string, std::pair<int, int>> names;
  for (size_t g = 0; g < groups.size(); ++g)
    for (size_t r = 0; r < groups[g].names.size(); ++r) names[groups[g].names[r]] = {(int)g, (int)r};
  given->assign(groups.size(), {});
  for (int i = 0; i < n; ++i) {
    XDET_REQUIRE(table[i].name, door + ": a NULL name");
    const std::string name(table[i].name);
    auto it = names.find(name);
    XDET_REQUIRE(it != names.end(), door + ": " + name + " is outside the reach (" + reach + ")");
    XDET_REQUIRE(table[i].data, door + ": " + name + " is a NULL pointer");
    std::vector<const float*>& g = (*given)[it->second.first];
    g.resize(groups[it->second.first].names.size(), nullptr);
    XDET_REQUIRE(!g[it->second.second], door + ": " + name + " is given twice");
    g[it->second.second] = table[i].data;
  }
  for (size_t g = 0; g < groups.size(); ++g)
    for (size_t r = 0; r < (*given)[g].size(); ++r)
      XDET_REQUIRE((*given)[g][r], door + ": the group of " + groups[g].label + " is given in part: " + groups[g].names[r] + " is missing");
  return XDET_OK;
}

// The eval body from trained weights (include/xdet.h): names -> layer_recs, all checks, then the folds, one table repack, one
// synchronisation, and the host copies the calibration works from.
int LightHeadNet::refresh_weights(const xdet_net_weight_dev* table, int n, hipStream_t s) {
  XDET_REQUIRE(built, "net_refresh_weights: the net is not built");
  XDET_REQUIRE(table && n > 0, "net_refresh_weights: an empty table");
  enum { R_KERNEL, R_GAMMA, R_BETA, R_MEAN, R_VAR, R_DW, R_N };
  // the reach: what conv_bn / sep_bn built of blocks 2-14 (block1_* is the stem), a record's tensors by role
  std::vector<int> reach;
  std::vector<NameGroup> groups;
  for (size_t i = 0; i < layer_recs.size(); ++i) {
    const LayerRec& r = layer_recs[i];
    if (r.bn.empty() || r.prefix.compare(0, 7, "block1_") == 0) continue;
    reach.push_back((int)i);
    groups.push_back({r.prefix, {r.prefix + (r.dw ? "/pointwise_kernel" : "/kernel"), r.bn + "/gamma", r.bn + "/beta", r.bn + "/moving_mean",
                                 r.bn + "/moving_variance"}});
    if (r.dw) groups.back().names.push_back(r.prefix + "/depthwise_kernel");
  }
  std::vector<std::vector<const float*>> given;
  XDET_TRY(parse_weight_table("net_refresh_weights", "the variables and moving statistics of the body's blocks 2-14", groups, table, n, &given));
  if (!rf.ws) {
    rf_off.assign(layer_recs.size(), 0);
    size_t channels = 0;
    std::vector<xdet_layer_refresh> all;
    const float* some = table[0].data;                       // (measuring reads no kernel)
    for (int i : reach) {
      const LayerRec& r = layer_recs[i];
      rf_off[i] = channels;
      channels += (size_t)r.conv->cout;
      all.push_back({r.conv, some, nullptr, nullptr});
      if (r.dw) all.push_back({r.dw, some, nullptr, nullptr});
    }
    const size_t bytes = xdet_layers_refresh_workspace_bytes(all.data(), (int)all.size());
    XDET_REQUIRE(bytes > 0, "net_refresh_weights: the plan holds a layer the table door refuses");
    // one block: either all of the scratch exists or none of it
    void* block = nullptr;
    XDET_TRY(alloc_bytes(ws_measure(256, body_refresh_layout, bytes, channels), &block, false));
    rf = ws_carve(block, 256, body_refresh_layout, bytes, channels);
  }
  std::vector<xdet_layer_refresh> slots;
  std::vector<size_t> on;                                    // the groups the table names, in the reach's order
  for (size_t gi = 0; gi < given.size(); ++gi) {
    const std::vector<const float*>& g = given[gi];
    if (g.empty()) continue;
    on.push_back(gi);
    const LayerRec& r = layer_recs[reach[gi]];
    float *sc = rf.scale + rf_off[reach[gi]], *sh = rf.shift + rf_off[reach[gi]];
    XDET_TRY(xdet_bn_fold(g[R_GAMMA], g[R_BETA], g[R_MEAN], g[R_VAR], nullptr, r.eps, r.conv->cout, sc, sh, s));
    slots.push_back({r.conv, g[R_KERNEL], sc, sh});
    if (r.dw) slots.push_back({r.dw, g[R_DW], nullptr, nullptr});
  }
  XDET_TRY(xdet_layers_refresh_device(slots.data(), (int)slots.size(), rf.ws, s));
  XDET_HIP(hipStreamSynchronize(s));
  // the host side back in line: the scale at exponent 0 (d_scale carries 2^in_exp, exactly), the taps from the kernel itself
  std::vector<float> k;
  auto download = [&](const float* d, size_t count) {
    k.resize(count);
    XDET_HIP(hipMemcpy(k.data(), d, count * sizeof(float), hipMemcpyDeviceToHost));
    return (int)XDET_OK;
  };
  for (size_t gi : on) {
    const std::vector<const float*>& g = given[gi];
    const LayerRec& r = layer_recs[reach[gi]];
    XDET_TRY(scale_read_back(r.conv));
    if (r.dw) {
      DepthwiseLayer* D = r.dw;
      XDET_TRY(download(g[R_DW], (size_t)9 * D->C));
      std::fill(D->taps.host.begin(), D->taps.host.end(), 0.f);
      for (int t = 0; t < 9; ++t)
        for (int c = 0; c < D->C; ++c) D->taps.host[(size_t)t * D->ld + c] = k[(size_t)t * D->C + c];
      D->host_stale = false;
      if (r.pscale >= 0) pscales[r.pscale].bound = depthwise_bound(k.data(), D->C);
    }
    for (size_t role = 0; role < g.size(); ++role) {      // a host copy the net still holds (none once build() has dropped them)
      auto hw = w.find(groups[gi].names[role]);
      if (hw == w.end()) continue;
      XDET_TRY(download(g[role], hw->second.v.size()));
      hw->second.v = k;
    }
  }
  return XDET_OK;
}

// The stem from trained weights (include/xdet.h): block1_conv2 -- and block1_conv1 where conv_bn built it, in f32 mode -- takes
// refresh_weights' own path: the fold, a slot of one table repack, scale_read_back.  block1_conv1 in the direct form keeps no
// layer: its kernel is copied into d_w (the checkpoint's layout), and the fold's scale and shift replace the host vectors
// behind the two Pow2Scaleds, uploaded again at the plane's current exponent.
int LightHeadNet::refresh_stem(const xdet_net_weight_dev* table, int n, hipStream_t s) {
  XDET_REQUIRE(built, "net_refresh_stem: the net is not built");
  XDET_REQUIRE(table && n > 0, "net_refresh_stem: an empty table");
  enum { R_KERNEL, R_GAMMA, R_BETA, R_MEAN, R_VAR };
  const char* const convs[2] = {"block1_conv1", "block1_conv2"};
  const int cout[2] = {32, 64};
  std::vector<NameGroup> groups;
  const LayerRec* rec[2] = {nullptr, nullptr};
  for (int g = 0; g < 2; ++g) {
    const std::string p = convs[g], bn = p + "_bn";
    groups.push_back({p, {p + "/kernel", bn + "/gamma", bn + "/beta", bn + "/moving_mean", bn + "/moving_variance"}});
    for (const LayerRec& r : layer_recs)
      if (r.prefix == p) rec[g] = &r;
  }
  std::vector<std::vector<const float*>> given;
  XDET_TRY(parse_weight_table("net_refresh_stem", "the kernels and batch norms of block1_conv1 and block1_conv2; the body's blocks 2-14 are "
                              "xdet_net_refresh_weights'", groups, table, n, &given));
  XDET_REQUIRE(rec[1] && (rec[0] || (stem_direct && stem_w && stem_pidx >= 0)), "net_refresh_stem: the plan holds no such layers");
  const float* some = table[0].data;                         // (measuring reads no kernel)
  if (!rf_stem.ws) {
    std::vector<xdet_layer_refresh> all;
    for (int g = 0; g < 2; ++g)
      if (rec[g]) all.push_back({rec[g]->conv, some, nullptr, nullptr});
    const size_t bytes = xdet_layers_refresh_workspace_bytes(all.data(), (int)all.size());
    XDET_REQUIRE(bytes > 0, "net_refresh_stem: the plan holds a layer the table door refuses");
    void* block = nullptr;
    XDET_TRY(alloc_bytes(ws_measure(256, body_refresh_layout, bytes, (size_t)(cout[0] + cout[1])), &block, false));
    rf_stem = ws_carve(block, 256, body_refresh_layout, bytes, (size_t)(cout[0] + cout[1]));
  }
  float* const sc[2] = {rf_stem.scale, rf_stem.scale + cout[0]};
  float* const sh[2] = {rf_stem.shift, rf_stem.shift + cout[0]};
  std::vector<xdet_layer_refresh> slots;
  for (int g = 0; g < 2; ++g)
    if (!given[g].empty() && rec[g]) slots.push_back({rec[g]->conv, given[g][R_KERNEL], sc[g], sh[g]});
  // the table door's refusals are met here, ahead of the first launch: no layer is touched by a refused call
  XDET_REQUIRE(slots.empty() || xdet_layers_refresh_workspace_bytes(slots.data(), (int)slots.size()) > 0,
               "net_refresh_stem: the plan holds a layer the table door refuses");
  for (int g = 0; g < 2; ++g) {
    const std::vector<const float*>& t = given[g];
    if (t.empty()) continue;
    XDET_TRY(xdet_bn_fold(t[R_GAMMA], t[R_BETA], t[R_MEAN], t[R_VAR], nullptr, rec[g] ? rec[g]->eps : stem_eps, cout[g], sc[g], sh[g], s));
  }
  const bool direct = !given[0].empty() && !rec[0];
  if (direct) XDET_HIP(hipMemcpyAsync(stem_w, given[0][R_KERNEL], (size_t)27 * 32 * sizeof(float), hipMemcpyDeviceToDevice, s));
  if (!slots.empty()) XDET_TRY(xdet_layers_refresh_device(slots.data(), (int)slots.size(), rf_stem.ws, s));
  XDET_HIP(hipStreamSynchronize(s));
  for (const xdet_layer_refresh& l : slots) XDET_TRY(scale_read_back(static_cast<ConvLayer*>(l.layer)));
  if (direct) {
    XDET_HIP(hipMemcpy(stem_sc.host.data(), sc[0], (size_t)cout[0] * sizeof(float), hipMemcpyDeviceToHost));
    XDET_HIP(hipMemcpy(stem_sh.host.data(), sh[0], (size_t)cout[0] * sizeof(float), hipMemcpyDeviceToHost));
    const int e = pscales[stem_pidx].exp;
    XDET_TRY(stem_sc.upload(-e));
    XDET_TRY(stem_sh.upload(-e));
  }
  return XDET_OK;
}

// behind a table repack and its synchronisation: the layer's host copy of the epilogue scale at exponent 0 (d_scale carries
// 2^in_exp, exactly), so that a calibration may apply an activation exponent to it again
int LightHeadNet::scale_read_back(ConvLayer* L) {
  std::vector<float> k((size_t)L->groups * L->cout_pad);      // (a grouped layer: every group's rows)
  XDET_HIP(hipMemcpy(k.data(), L->d_scale, k.size() * sizeof(float), hipMemcpyDeviceToHost));
  for (float& v : k) v = ldexpf(v, -L->in_exp);
  L->in_scale.host = k;
  L->host_stale = false;
  return XDET_OK;
}

// The layers the plan itself owns from trained weights (include/xdet.h): names -> three groups, all checks, the merges by one
// xdet_tensors_concat table into the net's scratch, the large-separable block's bias sum and fold, one table repack, one
// synchronisation, and the host copies the calibration works from.
int LightHeadNet::refresh_heads(const xdet_net_weight_dev* table, int n, hipStream_t s) {
  XDET_REQUIRE(built, "net_refresh_heads: the net is not built");
  XDET_REQUIRE(table && n > 0, "net_refresh_heads: an empty table");
  std::vector<NameGroup> groups;
  for (int g = 0; g < MG_N; ++g) groups.push_back({merged_group_name(g), merged_roles(g)});
  std::vector<std::vector<const float*>> given;
  XDET_TRY(parse_weight_table("net_refresh_heads", "the rpn_head, final_head and large_sep_feature groups; the body's blocks 2-14 are "
                              "xdet_net_refresh_weights'", groups, table, n, &given));
  bool on[MG_N];
  for (int g = 0; g < MG_N; ++g) on[g] = !given[g].empty();
  XDET_REQUIRE(!on[MG_LSEP] || !large_sep_spectral || spectral_refresh,
               "net_refresh_heads: the large_sep_feature group needs a net whose block is in the direct form (option large_sep=direct): "
               "this net's is in the spectral form, which keeps the kernels as DFT-domain block matrices (option spectral_refresh=on, "
               "set before the build, lets such a net evaluate them on the device)");
  const bool spec = on[MG_LSEP] && large_sep_spectral;          // the block's two layers are SpectralConvs, behind their own door
  ConvLayer* const* hd[MG_N] = {hd_rpn, hd_head, hd_lsep};
  for (int g = 0; g < MG_N; ++g)
    XDET_REQUIRE(!on[g] || (g == MG_LSEP && spec ? hd_spec[0] && hd_spec[1] : hd[g][0] && hd[g][1]), "net_refresh_heads: the plan holds no such layers");
  const MergedSizes z = merged_sizes();
  float* some = reinterpret_cast<float*>(this);              // (measuring reads no tensor)
  // a group's xdet_pack_slots by merged_layers.h: from the table's arrays into the scratch (measuring: `some` for both)
  auto pack_slots = [&](int g, bool measure, std::vector<xdet_pack_slot>* slots) {
    float* const dst[MG_N][3] = {{hs.rpn[0], hs.rpn[1]}, {hs.head[0], hs.head[1]}, {hs_k.k_a, hs.b_a, hs_k.k_b}};
    const std::vector<MergedSlot> ms = merged_slots(g, z);
    for (size_t i = 0; i < ms.size(); ++i) {
      xdet_pack_slot p = {measure ? some : dst[g][i], ms[i].outer, 2, {}, {}};
      for (int k = 0; k < 2; ++k) {
        p.part[k] = measure ? some : const_cast<float*>(given[g][(size_t)ms[i].role[k]]);
        p.width[k] = ms[i].width[k];
      }
      slots->push_back(p);
    }
  };
  if (!hs.pack_ws) {
    // one block: either all of it exists or none; the large-separable block's two merged kernels are a second block, at the
    // first call that names them
    std::vector<xdet_pack_slot> slots;
    for (int g = 0; g < MG_N; ++g)
      if (g != MG_LSEP || !large_sep_spectral || spectral_refresh) pack_slots(g, true, &slots);
    const size_t pack_bytes = xdet_tensors_concat_workspace_bytes(slots.data(), (int)slots.size());
    std::vector<xdet_layer_refresh> all;
    for (ConvLayer* L : {hd_rpn[0], hd_rpn[1], hd_head[0], hd_head[1], hd_lsep[0], hd_lsep[1]})
      if (L) all.push_back({L, some, nullptr, nullptr});
    const size_t rp_bytes = xdet_layers_refresh_workspace_bytes(all.data(), (int)all.size());
    XDET_REQUIRE(pack_bytes > 0 && rp_bytes > 0, "net_refresh_heads: the plan holds a layer the table door refuses");
    void* block = nullptr;
    XDET_TRY(alloc_bytes(ws_measure(256, heads_refresh_layout, pack_bytes, rp_bytes, z), &block, false));
    hs = ws_carve(block, 256, heads_refresh_layout, pack_bytes, rp_bytes, z);
  }
  if (on[MG_LSEP] && !hs_k.k_a) {
    void* block = nullptr;
    XDET_TRY(alloc_bytes(ws_measure(256, large_sep_kernel_layout, z), &block, false));
    hs_k = ws_carve(block, 256, large_sep_kernel_layout, z);
  }
  std::vector<xdet_pack_slot> slots;
  std::vector<xdet_layer_refresh> layers;
  for (int g = 0; g < MG_N; ++g)
    if (on[g]) pack_slots(g, false, &slots);
  if (on[MG_RPN]) {
    layers.push_back({hd_rpn[0], given[MG_RPN][HEAD_K0], nullptr, given[MG_RPN][HEAD_B0]});
    layers.push_back({hd_rpn[1], hs.rpn[SLOT_K], nullptr, hs.rpn[SLOT_B]});
  }
  if (on[MG_HEAD]) {
    layers.push_back({hd_head[0], given[MG_HEAD][HEAD_K0], nullptr, given[MG_HEAD][HEAD_B0]});
    layers.push_back({hd_head[1], hs.head[SLOT_K], nullptr, hs.head[SLOT_B]});
  }
  if (on[MG_LSEP] && !spec) {
    layers.push_back({hd_lsep[0], hs_k.k_a, nullptr, hs.b_a});
    layers.push_back({hd_lsep[1], hs_k.k_b, hs.scale, hs.shift});
  }
  // every refusal the two table doors have is met here, ahead of the first launch: no layer is touched by a refused call
  // (a call that names the spectral block alone has no table of layers)
  XDET_REQUIRE(xdet_tensors_concat_workspace_bytes(slots.data(), (int)slots.size()) > 0 &&
               (layers.empty() || xdet_layers_refresh_workspace_bytes(layers.data(), (int)layers.size()) > 0),
               "net_refresh_heads: the plan holds a layer the table door refuses");
  XDET_TRY(xdet_tensors_concat(slots.data(), (int)slots.size(), hs.pack_ws, s));
  if (on[MG_LSEP]) {
    const std::vector<const float*>& g = given[MG_LSEP];
    const int co = z.co;
    XDET_TRY(xdet_add_rows(g[LSEP_B0], co, g[LSEP_B1], co, hs.b_sum, co, 1, co, s));
    XDET_TRY(xdet_bn_fold(g[LSEP_GAMMA], g[LSEP_BETA], g[LSEP_MEAN], g[LSEP_VAR], hs.b_sum, 1e-5f, co, hs.scale, hs.shift, s));
  }
  if (!layers.empty()) XDET_TRY(xdet_layers_refresh_device(layers.data(), (int)layers.size(), hs.repack_ws, s));
  if (spec) {
    // the spectral form of the two slots above: (15,1) + b_a, then (1,15) + the fold, each layer's block matrices evaluated
    // from the merged kernel on the device (SpectralConv::set_kernel_device) at the grouped layer's own exponent
    XDET_TRY(hd_spec[0]->set_kernel_device(hs_k.k_a, nullptr, hs.b_a, s));
    XDET_TRY(hd_spec[1]->set_kernel_device(hs_k.k_b, hs.scale, hs.shift, s));
  }
  XDET_HIP(hipStreamSynchronize(s));
  for (const xdet_layer_refresh& l : layers) XDET_TRY(scale_read_back(static_cast<ConvLayer*>(l.layer)));
  if (spec)
    for (SpectralConv* S : hd_spec) XDET_TRY(scale_read_back(&S->G));
  return XDET_OK;
}

int LightHeadNet::calibrate(const float* images, int N, hipStream_t s, int* n_scaled) {
  if (head_rois_n && eval_head) {
    set_last_error("net_calibrate: this net was built with the options head_rois=" + std::to_string(head_rois_n) +
                   " and eval_head=on: its training stages and refresh doors are built and tested at exponent 0, and the eval head's "
                   "input plane on the shared dense layers has no pre-scale hook of its own; calibrate a net without head_rois");
    return XDET_ERR_STATE;
  }
  XDET_TRY(eval_refused("net_calibrate"));             // (it measures the planes of whole forwards)
  XDET_TRY(check(N));
  XDET_REQUIRE(images != nullptr, "calibrate: images is NULL");
  if (n_scaled) *n_scaled = 0;
  if (net_precision == PREC_F32 || pscales.empty()) return XDET_OK;
  graphs.clear();                                  // graphs bake kernel arguments (the split passes' multipliers)
  const size_t slots = (size_t)N * (cfg.num_classes - 1) * cfg.nms_topk;
  DevMem<float> ds, db;                            // detections of the calibration forwards: nobody reads them
  XDET_TRY(ds.alloc(slots));
  XDET_TRY(db.alloc(slots * 4));
  return calibrate_planes(N, s, n_scaled, [&](hipStream_t st) { return forward_eager(images, N, nullptr, nullptr, ds, db, st); });
}

int LightHeadNet::forward_eager(const float* images, int N, const int* shapes, const float* bbox, float* ds, float* db,
                  hipStream_t s) {
  XDET_TRY(eval_refused("net_forward", /*whole_forward=*/true));
  XDET_TRY(entry_and_middle_flow(images, N, s));
  // fork: the RPN branch (3x3 conv, 1x1 heads, decode, top-k, NMS -- a long conv and then small latency-bound
  // launches) needs mid_outputs only (net/xception_body.py:339,381-400): it runs on a side stream under the exit flow
  // AND the large-separable convs (round 4; it used to fork behind the exit flow, where a single image's RPN conv --
  // 207 K steps on 64 workgroups -- was the longer branch and sat on the critical path).
  // While per-op profiling is on, the branch stays on the main stream: an event pair around a launch that
  // shares the chip with the other branch's kernels would time the sharing, not the kernel.
  if (profiling || !rpn_side_stream) {
    XDET_TRY(run_stage(ST_EXIT, N, s));
    XDET_TRY(run_stage(ST_RPN, N, s));
    XDET_TRY(rpn_decode(N, s));
    XDET_TRY(get_proposals(N, s));
    XDET_TRY(run_stage(ST_LSEP, N, s));
  } else {
    if (!aux) {
      XDET_HIP(hipStreamCreateWithFlags(&aux, hipStreamNonBlocking));
      XDET_HIP(hipEventCreateWithFlags(&ev_fork, hipEventDisableTiming));
      XDET_HIP(hipEventCreateWithFlags(&ev_join, hipEventDisableTiming));
    }
    XDET_HIP(hipEventRecord(ev_fork, s));
    XDET_HIP(hipStreamWaitEvent(aux, ev_fork, 0));
    // The longer branch (exit flow + large-separable convs: the critical path of a single image) is issued FIRST.  In a
    // captured graph the branch whose nodes were created first continues on the queue of the fork node; the other one
    // starts behind a cross-queue signal -- and when the RPN branch was issued first, the replayed exit flow started only
    // when the RPN 3x3 conv had FINISHED (76 us at one image; rocprofv3 kernel trace of round 6, 29 of 29 steps).
    XDET_TRY(run_stage(ST_EXIT, N, s));
    XDET_TRY(run_stage(ST_LSEP, N, s));
    XDET_TRY(run_stage(ST_RPN, N, aux));
    XDET_TRY(rpn_decode(N, aux));
    XDET_TRY(get_proposals(N, aux));
    XDET_HIP(hipEventRecord(ev_join, aux));
    XDET_HIP(hipStreamWaitEvent(s, ev_join, 0));   // join before the head consumes the proposals
  }
  XDET_TRY(head_rois_n ? get_head_eval(N, s) : get_head(N, s));
  XDET_TRY(head_decode_probs(N, s));
  if (check_range && net_precision != PREC_F32) {
    for (const auto& b : f32_bufs) {
      float limit;
      int relu;
      f32_limit(b.first, &limit, &relu);
      XDET_TRY(launch_range_check(b.first, N, b.second, limit, prop_ws.bad, s, 1, 0, relu));
    }
    for (const auto& b : planes_bufs) XDET_TRY(launch_range_check_planes(b.hi, N, b.pix_per_image, b.ld, prop_ws.bad, s));
    for (const auto& f : extra_range_checks) XDET_TRY(f(N, s));
  }
  return bboxes_eval_probs(N, shapes, bbox, ds, db, s);
}

}  // namespace xdet
