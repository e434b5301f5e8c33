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
    const Pow2Scaled bn_sc{sc, d_sc}, bn_sh{sh, d_sh};
    pscales[x.pidx].apply.push_back([=](int e) {     // relu(x*sc + sh) * 2^-e = relu(x*(sc 2^-e) + sh 2^-e), exactly
      XDET_TRY(bn_sc.upload(-e));
      return bn_sh.upload(-e);
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
  const int A = cfg.num_anchors;
  const HostTensor *k0, *b0, *k1, *b1, *k2, *b2;
  XDET_TRY(need("rpn_head/conv2d/kernel", &k0, {3, 3, 728, 512}));
  XDET_TRY(need("rpn_head/conv2d/bias", &b0, {512}));
  XDET_TRY(need("rpn_head/conv2d_1/kernel", &k1, {1, 1, 512, 2 * A}));
  XDET_TRY(need("rpn_head/conv2d_1/bias", &b1, {2 * A}));
  XDET_TRY(need("rpn_head/conv2d_2/kernel", &k2, {1, 1, 512, 4 * A}));
  XDET_TRY(need("rpn_head/conv2d_2/bias", &b2, {4 * A}));
  ConvLayer* L0 = keep(new ConvLayer());
  XDET_TRY(L0->init(3, 3, 728, 512, 1, 1, 1, 0, 0, k0->v.data(), nullptr, b0->v.data(), 1));
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
  const int co = 6 * A;
  std::vector<float> kc((size_t)512 * co), bc(co);
  for (int ci = 0; ci < 512; ++ci) {
    for (int j = 0; j < 2 * A; ++j) kc[(size_t)ci * co + j] = k1->v[(size_t)ci * 2 * A + j];
    for (int j = 0; j < 4 * A; ++j) kc[(size_t)ci * co + 2 * A + j] = k2->v[(size_t)ci * 4 * A + j];
  }
  for (int j = 0; j < 2 * A; ++j) bc[j] = b1->v[j];
  for (int j = 0; j < 4 * A; ++j) bc[2 * A + j] = b2->v[j];
  ConvLayer* L1 = keep(new ConvLayer());
  XDET_TRY(L1->init(1, 1, 512, co, 1, 1, 1, 0, 0, kc.data(), nullptr, bc.data(), 0));
  XDET_TRY(add_conv("rpn_head/conv2d_1+2", ST_RPN, hid, L1, nullptr, 0, &rpn_out));
  hd_rpn[0] = L0; hd_rpn[1] = L1;
  return XDET_OK;
}

// The large-separable block's weights (net/xception_body.py:450-475) with its two branches fused: both (15,1) convs read
// the same input -> ONE conv with the filters concatenated (2*mid outputs: ka, ba); branch_0b + branch_1b = ONE (1,15) conv
// over the 2*mid stacked channels (kb), whose bias sum is folded into the BN(1e-5) + ReLU behind it (sc, sh)
int LightHeadNet::large_sep_weights(int cin, int mid, int co, std::vector<float>* ka, std::vector<float>* ba, std::vector<float>* kb,
                      std::vector<float>* sc, std::vector<float>* sh) const {
  const HostTensor *a0, *a0b, *a1, *a1b, *c0, *c0b, *c1, *c1b;
  XDET_TRY(need("large_sep_feature/Branch_0/conv2d/kernel", &a0, {15, 1, cin, mid}));
  XDET_TRY(need("large_sep_feature/Branch_0/conv2d/bias", &a0b, {mid}));
  XDET_TRY(need("large_sep_feature/Branch_1/conv2d/kernel", &a1, {15, 1, cin, mid}));
  XDET_TRY(need("large_sep_feature/Branch_1/conv2d/bias", &a1b, {mid}));
  XDET_TRY(need("large_sep_feature/Branch_0/conv2d_1/kernel", &c0, {1, 15, mid, co}));
  XDET_TRY(need("large_sep_feature/Branch_0/conv2d_1/bias", &c0b, {co}));
  XDET_TRY(need("large_sep_feature/Branch_1/conv2d_1/kernel", &c1, {1, 15, mid, co}));
  XDET_TRY(need("large_sep_feature/Branch_1/conv2d_1/bias", &c1b, {co}));
  const int mid2 = 2 * mid;
  ka->resize((size_t)15 * cin * mid2);
  ba->resize(mid2);
  kb->resize((size_t)15 * mid2 * co);
  for (size_t tc = 0; tc < (size_t)15 * cin; ++tc) {
    memcpy(&(*ka)[tc * mid2], &a0->v[tc * mid], mid * sizeof(float));
    memcpy(&(*ka)[tc * mid2 + mid], &a1->v[tc * mid], mid * sizeof(float));
  }
  for (int j = 0; j < mid; ++j) { (*ba)[j] = a0b->v[j]; (*ba)[mid + j] = a1b->v[j]; }
  for (int tap = 0; tap < 15; ++tap)
    for (int ci = 0; ci < mid; ++ci) {
      memcpy(&(*kb)[((size_t)tap * mid2 + ci) * co], &c0->v[((size_t)tap * mid + ci) * co], co * sizeof(float));
      memcpy(&(*kb)[((size_t)tap * mid2 + mid + ci) * co], &c1->v[((size_t)tap * mid + ci) * co], co * sizeof(float));
    }
  std::vector<float> bsum(co);
  for (int j = 0; j < co; ++j) bsum[j] = c0b->v[j] + c1b->v[j];
  return fold_bn("large_sep_feature/batch_normalization", co, 1e-5f, bsum.data(), sc, sh);
}

int LightHeadNet::build_large_sep() {
  const int mid = 256, co = cfg.bank * cfg.grid * cfg.grid;
  std::vector<float> ka, ba, kb, sc, sh;
  XDET_TRY(large_sep_weights(out.C, mid, co, &ka, &ba, &kb, &sc, &sh));
  ConvLayer* LA = keep(new ConvLayer());
  XDET_TRY(LA->init(15, 1, out.C, 2 * mid, 1, 1, 1, 0, 0, ka.data(), nullptr, ba.data(), 0));
  Buf t;
  // only the (1,15) conv reads it: planes only
  XDET_TRY(add_conv("large_sep_feature/Branch_0+1/conv2d", ST_LSEP, out, LA, nullptr, 0, &t, ConvEmit{3}));
  ConvLayer* LB = keep(new ConvLayer());
  XDET_TRY(LB->init(1, 15, 2 * mid, co, 1, 1, 1, 0, 0, kb.data(), sc.data(), sh.data(), 1));
  XDET_TRY(add_conv("large_sep_feature/Branch_0+1/conv2d_1", ST_LSEP, t, LB, nullptr, 0, &feat));
  hd_lsep[0] = LA; hd_lsep[1] = LB;
  return XDET_OK;
}

// net/xception_body.py:450-475 in the DFT domain of the convolved axis (spectral.hip): per frequency bin one
// real GEMM [N*F, 2*Cin] x [2*Cin, 2*Cout] on the split-precision MFMA kernel (grouped launch), a forward
// DFT pass in front and an inverse pass (+bias / +BN+ReLU) behind each of the two convolutions
int LightHeadNet::build_large_sep_spectral() {
  const int mid = 256, co = cfg.bank * cfg.grid * cfg.grid, F = out.H;
  const int cin = out.C, mid2 = 2 * mid;
  // the same branch fusion as the direct form: (15,1) with 2*mid outputs, (1,15) over the stacked channels
  std::vector<float> ka, kb, ba, sc, sh;
  XDET_TRY(large_sep_weights(cin, mid, co, &ka, &ba, &kb, &sc, &sh));
  // (15,1) + bias along y, then (1,15) + BN + ReLU along x: the layer the C ABI exposes as xdet_spectral_conv_*
  SpectralConv* SA = keep(new SpectralConv());
  SpectralConv* SB = keep(new SpectralConv());
  XDET_TRY(SA->init(ka.data(), 15, cin, mid2, 0, F, nullptr, ba.data(), 0));
  XDET_TRY(SB->init(kb.data(), 15, mid2, co, 1, F, sc.data(), sh.data(), 1));
  XDET_REQUIRE(SA->cin_ld == out.ld && SA->cout_ld == mid2, "plan: the spectral convs' channel strides");
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
  const int R = cfg.rpn_post_nms_top_n, C = cfg.bank * cfg.grid * cfg.grid, nc = cfg.num_classes;
  const HostTensor *k0, *b0, *k1, *b1, *k2, *b2;
  XDET_TRY(need("final_head/subnet_fc/kernel", &k0, {C, 2048}));
  XDET_TRY(need("final_head/subnet_fc/bias", &b0, {2048}));
  XDET_TRY(need("final_head/fc_cls/kernel", &k1, {2048, nc}));
  XDET_TRY(need("final_head/fc_cls/bias", &b1, {nc}));
  XDET_TRY(need("final_head/fc_loc/kernel", &k2, {2048, 4}));
  XDET_TRY(need("final_head/fc_loc/bias", &b2, {4}));
  // ROI rows are the GEMM M dimension: treat [N*R, C] as an NHWC tensor with H = R, W = 1
  XDET_TRY(new_buf(R, 1, C, &pooled));
  if (keep_pool_index) XDET_TRY(alloc_bytes((size_t)max_batch * R * pooled.ld * sizeof(int32_t), reinterpret_cast<void**>(&pool_index)));
  ConvLayer* L0 = keep(new ConvLayer());
  XDET_TRY(L0->init(1, 1, C, 2048, 1, 1, 0, 0, 0, k0->v.data(), nullptr, b0->v.data(), 1));
  XDET_TRY(add_conv("final_head/subnet_fc", ST_HEAD, pooled, L0, nullptr, 0, &fc, ConvEmit{1}));
  const int co = nc + 4;
  std::vector<float> kc((size_t)2048 * co), bc(co);
  for (int ci = 0; ci < 2048; ++ci) {
    for (int j = 0; j < nc; ++j) kc[(size_t)ci * co + j] = k1->v[(size_t)ci * nc + j];
    for (int j = 0; j < 4; ++j) kc[(size_t)ci * co + nc + j] = k2->v[(size_t)ci * 4 + j];
  }
  for (int j = 0; j < nc; ++j) bc[j] = b1->v[j];
  for (int j = 0; j < 4; ++j) bc[nc + j] = b2->v[j];
  ConvLayer* L1 = keep(new ConvLayer());
  XDET_TRY(L1->init(1, 1, 2048, co, 1, 1, 0, 0, 0, kc.data(), nullptr, bc.data(), 0));
  ConvEmit cls_emit;
  cls_emit.ksplit = latency_ksplit;     // 300 rows x 25 outputs: 3 tiles against 64 K steps
  XDET_TRY(add_conv("final_head/fc_cls+fc_loc", ST_HEAD, fc, L1, nullptr, 0, &cls_reg, cls_emit));
  hd_head[0] = L0; hd_head[1] = L1;
  return XDET_OK;
}

int LightHeadNet::build() {
  XDET_REQUIRE(!built, "net already built");
  XDET_REQUIRE(cfg.max_batch > 0 && cfg.image_size >= 64, "bad max_batch / image_size");
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

// The eval body from trained weights (include/xdet.h): names -> layer_recs, all checks, then the folds, one table repack, one
// synchronisation, and the host copies the calibration works from.
int LightHeadNet::refresh_weights(const xdet_net_weight_dev* table, int n, hipStream_t s) {
  XDET_REQUIRE(built, "net_refresh_weights: the net is not built");
  XDET_REQUIRE(table && n > 0, "net_refresh_weights: an empty table");
  enum { R_KERNEL, R_GAMMA, R_BETA, R_MEAN, R_VAR, R_DW, R_N };
  auto role_name = [](const LayerRec& r, int role) {
    switch (role) {
      case R_KERNEL: return r.prefix + (r.dw ? "/pointwise_kernel" : "/kernel");
      case R_DW: return r.prefix + "/depthwise_kernel";
      case R_GAMMA: return r.bn + "/gamma";
      case R_BETA: return r.bn + "/beta";
      case R_MEAN: return r.bn + "/moving_mean";
      default: return r.bn + "/moving_variance";
    }
  };
  // the reach: what conv_bn / sep_bn built of blocks 2-14 (block1_* is the stem)
  std::map<std::string, std::pair<int, int>> names;
  std::vector<int> reach;
  for (size_t i = 0; i < layer_recs.size(); ++i) {
    const LayerRec& r = layer_recs[i];
    if (r.bn.empty() || r.prefix.compare(0, 7, "block1_") == 0) continue;
    reach.push_back((int)i);
    for (int role = 0; role < (r.dw ? R_N : R_DW); ++role) names[role_name(r, role)] = {(int)i, role};
  }
  std::map<int, std::array<const float*, R_N>> groups;
  for (int i = 0; i < n; ++i) {
    XDET_REQUIRE(table[i].name, "net_refresh_weights: a NULL name");
    const std::string name(table[i].name);
    auto it = names.find(name);
    XDET_REQUIRE(it != names.end(), "net_refresh_weights: " + name + " is outside the reach (the variables and moving statistics of the "
                                    "body's blocks 2-14)");
    XDET_REQUIRE(table[i].data, "net_refresh_weights: " + name + " is a NULL pointer");
    auto g = groups.find(it->second.first);
    if (g == groups.end()) g = groups.emplace(it->second.first, std::array<const float*, R_N>{}).first;
    XDET_REQUIRE(!g->second[it->second.second], "net_refresh_weights: " + name + " is given twice");
    g->second[it->second.second] = table[i].data;
  }
  for (const auto& g : groups) {
    const LayerRec& r = layer_recs[g.first];
    for (int role = 0; role < (r.dw ? R_N : R_DW); ++role)
      XDET_REQUIRE(g.second[role], "net_refresh_weights: the group of " + r.prefix + " is given in part: " + role_name(r, role) +
                                   " is missing");
  }
  if (!rf_ws) {
    rf_off.assign(layer_recs.size(), 0);
    size_t channels = 0;
    std::vector<xdet_layer_refresh> all;
    const float* some = groups.begin()->second[R_KERNEL];    // (measuring reads no kernel)
    for (int i : reach) {
      const LayerRec& r = layer_recs[i];
      rf_off[i] = channels;
      channels += (size_t)r.conv->cout;
      all.push_back({r.conv, some, nullptr, nullptr});
      if (r.dw) all.push_back({r.dw, some, nullptr, nullptr});
    }
    const size_t bytes = xdet_layers_refresh_workspace_bytes(all.data(), (int)all.size());
    XDET_REQUIRE(bytes > 0, "net_refresh_weights: the plan holds a layer the table door refuses");
    // one block [table workspace | scales | shifts]: either all of the scratch exists or none of it
    const size_t ws_bytes = (bytes + 255) / 256 * 256, fold_bytes = (channels * sizeof(float) + 255) / 256 * 256;
    void* block = nullptr;
    XDET_TRY(alloc_bytes(ws_bytes + 2 * fold_bytes, &block, false));
    rf_scale = reinterpret_cast<float*>(static_cast<char*>(block) + ws_bytes);
    rf_shift = reinterpret_cast<float*>(static_cast<char*>(block) + ws_bytes + fold_bytes);
    rf_ws = block;
  }
  std::vector<xdet_layer_refresh> slots;
  for (const auto& g : groups) {
    const LayerRec& r = layer_recs[g.first];
    float *sc = rf_scale + rf_off[g.first], *sh = rf_shift + rf_off[g.first];
    XDET_TRY(xdet_bn_fold(g.second[R_GAMMA], g.second[R_BETA], g.second[R_MEAN], g.second[R_VAR], nullptr, r.eps, r.conv->cout, sc, sh, s));
    slots.push_back({r.conv, g.second[R_KERNEL], sc, sh});
    if (r.dw) slots.push_back({r.dw, g.second[R_DW], nullptr, nullptr});
  }
  XDET_TRY(xdet_layers_refresh_device(slots.data(), (int)slots.size(), rf_ws, s));
  XDET_HIP(hipStreamSynchronize(s));
  // the host side back in line: the scale at exponent 0 (d_scale carries 2^in_exp, exactly), the taps from the kernel itself
  std::vector<float> k;
  auto download = [&](const float* d, size_t count) {
    k.resize(count);
    XDET_HIP(hipMemcpy(k.data(), d, count * sizeof(float), hipMemcpyDeviceToHost));
    return (int)XDET_OK;
  };
  for (const auto& g : groups) {
    const LayerRec& r = layer_recs[g.first];
    XDET_TRY(scale_read_back(r.conv));
    if (r.dw) {
      DepthwiseLayer* D = r.dw;
      XDET_TRY(download(g.second[R_DW], (size_t)9 * D->C));
      std::fill(D->taps.host.begin(), D->taps.host.end(), 0.f);
      for (int t = 0; t < 9; ++t)
        for (int c = 0; c < D->C; ++c) D->taps.host[(size_t)t * D->ld + c] = k[(size_t)t * D->C + c];
      D->host_stale = false;
      if (r.pscale >= 0) pscales[r.pscale].bound = depthwise_bound(k.data(), D->C);
    }
    for (int role = 0; role < (r.dw ? R_N : R_DW); ++role) {      // a host copy the net still holds (none once build() has dropped them)
      auto hw = w.find(role_name(r, role));
      if (hw == w.end()) continue;
      XDET_TRY(download(g.second[role], hw->second.v.size()));
      hw->second.v = k;
    }
  }
  return XDET_OK;
}

// behind a table repack and its synchronisation: the layer's host copy of the epilogue scale at exponent 0 (d_scale carries
// 2^in_exp, exactly), so that a calibration may apply an activation exponent to it again
int LightHeadNet::scale_read_back(ConvLayer* L) {
  std::vector<float> k((size_t)L->cout_pad);
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
  enum { G_RPN, G_HEAD, G_LSEP, G_N };
  static const char* const group_name[G_N] = {"rpn_head", "final_head", "large_sep_feature"};
  std::vector<std::string> roles[G_N];
  for (const char* l : {"conv2d", "conv2d_1", "conv2d_2"})
    for (const char* v : {"/kernel", "/bias"}) roles[G_RPN].push_back(std::string("rpn_head/") + l + v);
  for (const char* l : {"subnet_fc", "fc_cls", "fc_loc"})
    for (const char* v : {"/kernel", "/bias"}) roles[G_HEAD].push_back(std::string("final_head/") + l + v);
  for (const char* br : {"Branch_0", "Branch_1"})
    for (const char* l : {"/conv2d", "/conv2d_1"})
      for (const char* v : {"/kernel", "/bias"}) roles[G_LSEP].push_back(std::string("large_sep_feature/") + br + l + v);
  for (const char* v : {"gamma", "beta", "moving_mean", "moving_variance"})
    roles[G_LSEP].push_back(std::string("large_sep_feature/batch_normalization/") + v);
  std::map<std::string, std::pair<int, int>> names;
  for (int g = 0; g < G_N; ++g)
    for (size_t r = 0; r < roles[g].size(); ++r) names[roles[g][r]] = {g, (int)r};
  std::vector<const float*> given[G_N];
  bool on[G_N] = {false, false, false};
  for (int g = 0; g < G_N; ++g) given[g].assign(roles[g].size(), nullptr);
  for (int i = 0; i < n; ++i) {
    XDET_REQUIRE(table[i].name, "net_refresh_heads: a NULL name");
    const std::string name(table[i].name);
    auto it = names.find(name);
    XDET_REQUIRE(it != names.end(), "net_refresh_heads: " + name + " is outside the reach (the rpn_head, final_head and "
                                    "large_sep_feature groups; the body's blocks 2-14 are xdet_net_refresh_weights')");
    XDET_REQUIRE(table[i].data, "net_refresh_heads: " + name + " is a NULL pointer");
    const float*& slot = given[it->second.first][it->second.second];
    XDET_REQUIRE(!slot, "net_refresh_heads: " + name + " is given twice");
    slot = table[i].data;
    on[it->second.first] = true;
  }
  for (int g = 0; g < G_N; ++g) {
    if (!on[g]) continue;
    for (size_t r = 0; r < roles[g].size(); ++r)
      XDET_REQUIRE(given[g][r], std::string("net_refresh_heads: the group of ") + group_name[g] + " is given in part: " + roles[g][r] +
                                " is missing");
  }
  XDET_REQUIRE(!on[G_LSEP] || !large_sep_spectral,
               "net_refresh_heads: the large_sep_feature group needs a net whose block is in the direct form (option large_sep=direct): "
               "this net's is in the spectral form, which keeps the kernels as DFT-domain block matrices");
  XDET_REQUIRE((!on[G_RPN] || (hd_rpn[0] && hd_rpn[1])) && (!on[G_HEAD] || (hd_head[0] && hd_head[1])) &&
               (!on[G_LSEP] || (hd_lsep[0] && hd_lsep[1])), "net_refresh_heads: the plan holds no such layers");
  const int A = cfg.num_anchors, nc = cfg.num_classes, mid = 256, co = cfg.bank * cfg.grid * cfg.grid, cin = out.C;
  const int hid = hd_rpn[0]->cout, fcw = hd_head[0]->cout;
  auto up = [](size_t b) { return (b + 255) / 256 * 256; };
  float* some = reinterpret_cast<float*>(this);              // (measuring reads no tensor)
  // the concat slots of a group, from the table's arrays (measuring: from `some`) into the scratch
  auto pack_slots = [&](int g, const std::vector<const float*>& src, std::vector<xdet_pack_slot>* slots) {
    auto at = [&](int r) { return const_cast<float*>(src.empty() ? some : src[(size_t)r]); };
    auto to = [&](float* d) { return src.empty() ? some : d; };
    if (g == G_RPN) {
      slots->push_back({to(hs_rpn_k), hid, 2, {at(2), at(4)}, {2 * A, 4 * A}});
      slots->push_back({to(hs_rpn_b), 1, 2, {at(3), at(5)}, {2 * A, 4 * A}});
    } else if (g == G_HEAD) {
      slots->push_back({to(hs_head_k), fcw, 2, {at(2), at(4)}, {nc, 4}});
      slots->push_back({to(hs_head_b), 1, 2, {at(3), at(5)}, {nc, 4}});
    } else {
      slots->push_back({to(hs_ka), 15 * cin, 2, {at(0), at(4)}, {mid, mid}});
      slots->push_back({to(hs_ba), 1, 2, {at(1), at(5)}, {mid, mid}});
      slots->push_back({to(hs_kb), 15, 2, {at(2), at(6)}, {mid * co, mid * co}});
    }
  };
  if (!hs_block) {
    // one block [pack workspace | repack workspace | rpn k, b | head k, b | b_a, b0 + b1, scale, shift]: either all of it
    // exists or none; the large-separable block's two merged kernels are a second block, at the first call that names them
    std::vector<xdet_pack_slot> slots;
    for (int g = 0; g < G_N; ++g)
      if (g != G_LSEP || !large_sep_spectral) pack_slots(g, {}, &slots);
    const size_t pack_bytes = xdet_tensors_concat_workspace_bytes(slots.data(), (int)slots.size());
    std::vector<xdet_layer_refresh> all;
    for (ConvLayer* L : {hd_rpn[0], hd_rpn[1], hd_head[0], hd_head[1], hd_lsep[0], hd_lsep[1]})
      if (L) all.push_back({L, some, nullptr, nullptr});
    const size_t rp_bytes = xdet_layers_refresh_workspace_bytes(all.data(), (int)all.size());
    XDET_REQUIRE(pack_bytes > 0 && rp_bytes > 0, "net_refresh_heads: the plan holds a layer the table door refuses");
    const size_t sizes[] = {up(pack_bytes), up(rp_bytes), up((size_t)hid * 6 * A * 4), up((size_t)6 * A * 4), up((size_t)fcw * (nc + 4) * 4),
                            up((size_t)(nc + 4) * 4), up((size_t)2 * mid * 4), up((size_t)co * 4), up((size_t)co * 4), up((size_t)co * 4)};
    size_t total = 0;
    for (size_t b : sizes) total += b;
    void* block = nullptr;
    XDET_TRY(alloc_bytes(total, &block, false));
    char* p = static_cast<char*>(block);
    float** dst[] = {nullptr, nullptr, &hs_rpn_k, &hs_rpn_b, &hs_head_k, &hs_head_b, &hs_ba, &hs_bsum, &hs_scale, &hs_shift};
    for (size_t i = 0; i < sizeof(sizes) / sizeof(sizes[0]); ++i) {
      if (i == 0) hs_pack_ws = p;
      else if (i == 1) hs_repack_ws = p;
      else *dst[i] = reinterpret_cast<float*>(p);
      p += sizes[i];
    }
    hs_block = block;
  }
  if (on[G_LSEP] && !hs_ka) {
    const size_t ka_bytes = up((size_t)15 * cin * 2 * mid * 4), kb_bytes = up((size_t)15 * 2 * mid * co * 4);
    void* block = nullptr;
    XDET_TRY(alloc_bytes(ka_bytes + kb_bytes, &block, false));
    hs_ka = static_cast<float*>(block);
    hs_kb = reinterpret_cast<float*>(static_cast<char*>(block) + ka_bytes);
  }
  std::vector<xdet_pack_slot> slots;
  std::vector<xdet_layer_refresh> layers;
  for (int g = 0; g < G_N; ++g)
    if (on[g]) pack_slots(g, given[g], &slots);
  if (on[G_RPN]) {
    layers.push_back({hd_rpn[0], given[G_RPN][0], nullptr, given[G_RPN][1]});
    layers.push_back({hd_rpn[1], hs_rpn_k, nullptr, hs_rpn_b});
  }
  if (on[G_HEAD]) {
    layers.push_back({hd_head[0], given[G_HEAD][0], nullptr, given[G_HEAD][1]});
    layers.push_back({hd_head[1], hs_head_k, nullptr, hs_head_b});
  }
  if (on[G_LSEP]) {
    layers.push_back({hd_lsep[0], hs_ka, nullptr, hs_ba});
    layers.push_back({hd_lsep[1], hs_kb, hs_scale, hs_shift});
  }
  // every refusal the two table doors have is met here, ahead of the first launch: no layer is touched by a refused call
  XDET_REQUIRE(xdet_tensors_concat_workspace_bytes(slots.data(), (int)slots.size()) > 0 &&
               xdet_layers_refresh_workspace_bytes(layers.data(), (int)layers.size()) > 0,
               "net_refresh_heads: the plan holds a layer the table door refuses");
  XDET_TRY(xdet_tensors_concat(slots.data(), (int)slots.size(), hs_pack_ws, s));
  if (on[G_LSEP]) {
    const std::vector<const float*>& g = given[G_LSEP];
    XDET_TRY(xdet_add_rows(g[3], co, g[7], co, hs_bsum, co, 1, co, s));
    XDET_TRY(xdet_bn_fold(g[8], g[9], g[10], g[11], hs_bsum, 1e-5f, co, hs_scale, hs_shift, s));
  }
  XDET_TRY(xdet_layers_refresh_device(layers.data(), (int)layers.size(), hs_repack_ws, s));
  XDET_HIP(hipStreamSynchronize(s));
  for (const xdet_layer_refresh& l : layers) XDET_TRY(scale_read_back(static_cast<ConvLayer*>(l.layer)));
  return XDET_OK;
}

int LightHeadNet::calibrate(const float* images, int N, hipStream_t s, int* n_scaled) {
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
  XDET_TRY(get_head(N, s));
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
