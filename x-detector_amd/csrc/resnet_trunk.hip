// ResNetTrunk::build: stem, sixteen pre-activation bottleneck blocks, closing BN + ReLU.
#include "resnet_trunk.h"

namespace xdet {

int ResNetTrunk::add_bn_relu(const std::string& bn, const Buf& in, Buf* out) {
  std::vector<float> sc, sh;
  float *dsc, *dsh;
  XDET_TRY(upload_bn(bn, in.C, in.ld, 1e-5f, &sc, &sh, &dsc, &dsh));
  XDET_TRY(new_buf(in.H, in.W, in.C, out));
  if (g_default_precision != PREC_F32 && in.ld % 32 == 0) {
    XDET_TRY(new_planes(out));
    pscales[out->pidx].name = bn + " (pre-activation planes)";
  }
  const Buf i = in, o = *out;
  ops.push_back({bn, 0, 0.0, [=](int N, hipStream_t s) {
                   return launch_bn_relu(i.p, dsc, dsh, o.p, o.hi, o.lo, (int64_t)N * i.H * i.W, i.ld, pmul(o.pidx), s);
                 }});
  return XDET_OK;
}


// conv2d_fixed_padding(7, stride 2) and initial_max_pool (net/resnet_v2.py:311-330)
int ResNetTrunk::build_stem(Names* names, Buf* x_out, Carry* carry) {
  XDET_TRY(new_buf(image_size, image_size, 3, &in4));
  Buf x, t;
  ConvArgs c0;                                     // explicit pad 3/3 then VALID (:89-100)
  c0.k = 7; c0.cout = 64; c0.stride = 2; c0.pad_mode = 2; c0.pad_expl = 3;
  ConvLayer* L0 = nullptr;
  XDET_TRY(conv_bn(names->cname(), "", 0.f, 0, in4, c0, &x, &L0));
  // ... on its own kernel, straight from the NCHW input (resnet_stem.hip): the generic small-cin kernel gathers one 16-byte
  // load per (pixel, tap) from an NHWC4 copy of the image; same products, same order
  if (stem7_enabled && g_default_precision == PREC_F16X3 && ops.size() == 1 &&
      resnet_stem7x7_supported(7, 7, 3, 64, 2, 2, 3, image_size)) {
    const Buf o = x;
    const int S = image_size;
    ops[0].run = [=](int N, hipStream_t s) {
      return launch_resnet_stem7x7(cur_images, L0->d_wt_hi, L0->d_wt_lo, L0->d_scale, L0->d_shift, o.p, N, S, s);
    };
    ops[0].name += " [LDS-staged patch, from NCHW]";
    stem7_direct = true;
  }
  // initial_max_pool (:311-330).  On the split path its one reader is the first block's pre-activation, which is read as
  // planes only: pool + that block's bn + ReLU + split in one pass (no pooled f32 tensor, one launch less)
  if (g_default_precision != PREC_F32 && x.ld % 32 == 0 && stem_pool_bn) {
    int Ho, Wo, pt, pl;
    same_pad(x.H, 3, 2, 1, &pt, &Ho);
    same_pad(x.W, 3, 2, 1, &pl, &Wo);
    const std::string bn0 = "batch_normalization";
    std::vector<float> sc, sh;
    float *dsc, *dsh;
    XDET_TRY(upload_bn(bn0, x.C, x.ld, 1e-5f, &sc, &sh, &dsc, &dsh));
    Buf stem_pre;
    stem_pre.H = Ho; stem_pre.W = Wo; stem_pre.C = x.C; stem_pre.ld = x.ld; stem_pre.no_f32 = true;
    XDET_TRY(new_planes(&stem_pre));
    pscales[stem_pre.pidx].name = bn0 + " (pre-activation planes)";
    const Buf i = x, o = stem_pre;
    ops.push_back({"initial_max_pool + " + bn0, 0, 0.0, [=](int N, hipStream_t s) {
                     return launch_maxpool3x3s2_bn_planes(i.p, dsc, dsh, o.hi, o.lo, N, i.H, i.W, i.C, i.ld, Ho, Wo, pt, pl,
                                                          pmul(o.pidx), s, stem_cat_hi, stem_cat_lo, stem_cat_c32, pmul(stem_cat_pidx) * stem_cat_mul);
                   }});
    stem_pool_fused = true;
    carry->fused_pre = stem_pre;                   // (no fused_sc: the first block has no strided projection)
    carry->have_fused = true;
    // block 0 takes its shortcut from a projection of the pre-activation: the pooled tensor has no f32 reader.  `x` keeps the
    // shape only (no pointer, no planes, no flags: the blocks copy it into their output descriptors)
    x = Buf();
    x.H = Ho; x.W = Wo; x.C = stem_pre.C; x.ld = stem_pre.ld;
  } else {
    XDET_TRY(add_pool("initial_max_pool", 0, x, nullptr, &t));
    x = t;
  }
  *x_out = x;
  return XDET_OK;
}

// A projection shortcut folded into the block's closing GEMM (net/resnet_v2.py:160-184: shortcut = projection(pre), output =
// conv3(...) + shortcut, neither followed by a BN): [y2 | pre'] x [w_c ; w_proj] is ONE contraction over cmid + cin
// channels -- no projection launch, no 4f-channel shortcut tensor written and read back (118 / 59 / 29 / 15 MB each way at
// batch 8).  The operand is one planes tensor: the 3x3 conv's epilogue writes its channel blocks [0, cmid/32), the pass that
// makes pre' (the stem's pool + pre-activation pass / the stride-2 subsample of relu(bn(x))) the blocks behind them.  One f32
// accumulation over both parts instead of two roundings and an add: not bit-identical to the two-GEMM form, same tolerance
// against the oracle (tests/test_gpu_resnet.py).
int ResNetTrunk::setup_projcat(Block& k, const Carry& carry) {
  const int f = k.f, s = k.s;
  const Buf &pre = k.pre, &x = k.x;
  const bool cat_s1 = s == 1 && k.st == 0 && pre.hi && pre.pidx >= 0 && !pre.planes_relu;
  const bool cat_s2 = s == 2 && pre.no_f32 && x.p && carry.fused_sc && x.ld % 32 == 0;
  k.cat_on = projcat_enabled && k.b == 0 && g_default_precision == PREC_F16X3 && (cat_s1 || cat_s2) && f % 32 == 0 &&
             pre.ld % 32 == 0 && pre.ld == pre.C;
  if (!k.cat_on) return XDET_OK;
  Buf& cat = k.cat;
  cat.H = (pre.H + s - 1) / s; cat.W = (pre.W + s - 1) / s; cat.C = f + pre.C; cat.ld = f + pre.ld; cat.no_f32 = true;
  XDET_TRY(new_planes(&cat));
  pscales[cat.pidx].name = k.cproj + " + closing conv: [3x3 output | block input] operand";
  const size_t off = (size_t)(f >> 5) << 9;          // halves: the block input's first channel block inside a 16-pixel group
  // The two parts share one weight pre-scale per output channel and one activation pre-scale: balance them.  The block-input
  // part is stored as pre * 2^-cat_d and w_proj enters as w_proj * 2^cat_d (exact), cat_d = the binade distance of the two
  // matrices' largest magnitudes -- a projection whose weights are 2^17 below the closing conv's (and whose input is 2^17
  // above: test_trunk_pre_activations_beyond_the_f16_range) would otherwise lose its lo plane to f16 underflow.
  {
    const HostTensor *kc0, *kp0;
    XDET_TRY(need(k.c3 + "/kernel", &kc0, {1, 1, f, 4 * f}));
    XDET_TRY(need(k.cproj + "/kernel", &kp0, {1, 1, pre.C, 4 * f}));
    float mc = 0.f, mp = 0.f;
    for (float v : kc0->v) mc = std::max(mc, std::fabs(v));
    for (float v : kp0->v) mp = std::max(mp, std::fabs(v));
    int ec = 0, ep = 0;
    if (mc > 0.f && mp > 0.f && std::isfinite(mc) && std::isfinite(mp)) { (void)frexpf(mc, &ec); (void)frexpf(mp, &ep); }
    k.cat_d = ec - ep;
  }
  const float part_mul = ldexpf(1.f, -k.cat_d);
  if (cat_s1 && stem_pool_fused) {                // the stem's pool + pre-activation pass writes the block input twice
    stem_cat_hi = cat.hi + off; stem_cat_lo = cat.lo + off; stem_cat_c32 = cat.ld >> 5; stem_cat_pidx = cat.pidx;
    stem_cat_mul = part_mul;
  } else if (cat_s1) {                            // (two-pass stem, option "stem_pool" = off: a copy of the pre-activation planes)
    const Buf i = pre, o = cat;
    ops.push_back({k.cproj + "/copy of the block input [into the closing conv's operand]", 0, 0.0, [=](int N, hipStream_t s_) {
                     return launch_planes_copy_blocks(i.hi, i.lo, o.hi + off, o.lo + off, (int64_t)N * i.H * i.W, i.ld, o.ld >> 5,
                                                      pmul(o.pidx) * part_mul / pmul(i.pidx), s_);
                   }});
  } else {
    const Buf i = x, o = cat;
    const float *psc = carry.fused_sc, *psh = carry.fused_sh;
    ops.push_back({k.cproj + "/subsample_split [into the closing conv's operand]", 0, 0.0, [=](int N, hipStream_t s_) {
                     return launch_split_f32_subsample2(i.p, o.hi + off, o.lo + off, N, i.H, i.W, i.ld, s_, psc, psh, pmul(o.pidx) * part_mul,
                                                        o.ld >> 5);
                   }});
  }
  k.shortcut = Buf();
  return XDET_OK;
}

// The opening 1x1 of a stage-2 block on resnet_preconv.hip: it makes relu(bn(x)) from the raw block input itself, so
// the producer of x does not write the planes copy (decided per forward with the fused blocks: bneck_all_ok()).
void ResNetTrunk::rewire_preconv(const Block& k, const Carry& carry) {
  const Buf& pre = k.pre;
  ConvLayer* La = k.La;
  const bool preconv = preconv_enabled && g_default_precision == PREC_F16X3 && carry.have_pl && pre.hi && pre.no_f32 && k.x.p &&
                       ops.size() == k.op_first + 1 && k.y1.hi && La->ksplit <= 1 &&     // (a layer with a split reduction keeps its summation tree)
                       resnet_preconv_supported(pre.C, k.f, (int64_t)max_batch * pre.H * pre.W) &&
                       !(bneck_enabled && k.b > 0 && resnet_bneck_supported(pre.C, k.f, 4 * k.f, pre.H, pre.W, max_batch));
  if (!preconv) return;
  preconv_layers.push_back({carry.Lc, La});
  if (k.prev_group >= 0) bneck_groups[k.prev_group].next_fused = true;
  if (carry.drop_idx >= 0) planes_drop_ok[carry.drop_idx] = 1;
  ConvLayer* Lp = carry.Lc;
  const Buf xi = k.x, yo = k.y1;
  const int cin = pre.C, cm = k.f;
  const auto run_a = ops[k.op_first].run;
  ops[k.op_first].run = [=](int N, hipStream_t st) {
    if (!bneck_fused_now) return run_a(N, st);
    return launch_resnet_preconv(xi.p, Lp->d_pl_scale, Lp->d_pl_shift, La->d_wt_hi_b, La->d_wt_lo_b, La->d_scale, La->d_shift,
                                 yo.hi, yo.lo, (int64_t)N * xi.H * xi.W, cin, cm, st);
  };
  ops[k.op_first].name += " [pre-activation on the CU]";
}

// An identity block as ONE kernel (resnet_bneck.hip), reading the raw block input (it applies the pre-activation BN +
// ReLU itself, with the arithmetic of the planes copy the previous block's closing conv writes) and writing the
// pre-activation planes of the next block only if that one runs as three launches.  The three ops stay in the plan:
// a calibration pass measures the inner planes tensors behind them, and a trunk in which any tensor of a fusable
// block carries an activation pre-scale runs every block as three launches (all or nothing per forward: a fused
// block does not write the planes an unfused successor would read).
// Sets k.group where the block qualifies.
void ResNetTrunk::register_bneck(Block& k, const Carry& carry) {
  const Buf& pre = k.pre;
  ConvLayer *La = k.La, *Lb = k.Lb, *Lc = k.Lc;
  const size_t op_first = k.op_first;
  if (!(bneck_enabled && k.b > 0 && g_default_precision == PREC_F16X3 && ops.size() == op_first + 3 && pre.hi && k.y3.hi &&
        carry.have_pl && La->ksplit < 1 && Lb->ksplit < 1 && Lc->ksplit < 1 &&
        resnet_bneck_supported(pre.C, k.f, 4 * k.f, pre.H, pre.W, max_batch)))
    return;
  BneckGroup gr;
  gr.La = La; gr.Lb = Lb; gr.Lc = Lc; gr.Lprev = carry.Lc;
  gr.a.x = k.shortcut.p;
  gr.a.wa_hi = La->d_wt_hi_b; gr.a.wa_lo = La->d_wt_lo_b; gr.a.wb_hi = Lb->d_wt_hi_b; gr.a.wb_lo = Lb->d_wt_lo_b;
  gr.a.wc_hi = Lc->d_wt_hi_b; gr.a.wc_lo = Lc->d_wt_lo_b;
  gr.a.sc_a = La->d_scale; gr.a.sh_a = La->d_shift; gr.a.sc_b = Lb->d_scale; gr.a.sh_b = Lb->d_shift;
  gr.a.sc_c = Lc->d_scale; gr.a.sh_c = Lc->d_shift;
  gr.a.pre_sc = gr.a.pre_sh = gr.a.pl_sc = gr.a.pl_sh = nullptr;     // (the planes affines: read at launch time)
  gr.a.out = k.y3.p; gr.a.out_hi = k.y3.hi; gr.a.out_lo = k.y3.lo;
  gr.a.H = pre.H; gr.a.W = pre.W; gr.a.cin = pre.C; gr.a.cmid = k.f; gr.a.cout = 4 * k.f;
  gr.op_first = op_first;
  if (!bneck_groups.empty() && bneck_groups.back().op_first + 3 == op_first) bneck_groups.back().next_fused = true;
  if (carry.drop_idx >= 0) planes_drop_ok[carry.drop_idx] = 1;
  bneck_groups.push_back(gr);
  const size_t gi = bneck_groups.size() - 1;
  k.group = (int)gi;
  const auto run_a = ops[op_first].run, run_b = ops[op_first + 1].run, run_c = ops[op_first + 2].run;
  ops[op_first].run = [=](int N, hipStream_t st) {
    if (!bneck_fused_now) return run_a(N, st);
    const BneckGroup& G = bneck_groups[gi];
    BneckLaunch l = G.a;
    l.pre_sc = G.Lprev->d_pl_scale; l.pre_sh = G.Lprev->d_pl_shift;
    l.pl_sc = G.Lc->d_pl_scale; l.pl_sh = G.Lc->d_pl_shift;
    if (G.next_fused) l.out_hi = l.out_lo = nullptr;          // the next block makes its own pre-activation
    return launch_resnet_bneck(l, N, st);
  };
  ops[op_first + 1].run = [=](int N, hipStream_t st) { return bneck_fused_now ? (int)XDET_OK : run_b(N, st); };
  ops[op_first + 2].run = [=](int N, hipStream_t st) { return bneck_fused_now ? (int)XDET_OK : run_c(N, st); };
  ops[op_first].name += " [+2: one kernel]";
}

// One pre-activation bottleneck: conv1x1 -> (BN+ReLU fused into its epilogue) -> conv3x3/s -> (BN+ReLU fused) -> conv1x1 +
// shortcut.  *x: the raw block input on entry, the block output on return.
int ResNetTrunk::build_block(Block& k, Buf* x_io, Carry* carry) {
  const int f = k.f, s = k.s;
  const Buf x = *x_io;
  k.x = x;
  k.shortcut = x;
  if (carry->have_fused) k.pre = carry->fused_pre;   // its BN was folded into the producer of x (previous block's epilogue / pool pass)
  else XDET_TRY(add_bn_relu(k.bn_pre, x, &k.pre));
  carry->have_fused = false;
  const Buf& pre = k.pre;
  XDET_TRY(setup_projcat(k, *carry));
  if (!k.cat_on && k.b == 0) {
    ConvArgs cp;
    cp.cout = 4 * f; cp.stride = s;
    if (pre.no_f32 && s > 1) {
      // the pre-activation exists as full-resolution planes only (conv1 reads those); the stride-2 projection
      // takes the raw block input and applies the BN + ReLU to the quarter of the pixels it reads
      cp.pad_mode = 2; cp.pre_sc = carry->fused_sc; cp.pre_sh = carry->fused_sh;
      XDET_TRY(conv_bn(k.cproj, "", 0.f, 0, x, cp, &k.shortcut));
    } else {
      cp.pad_mode = s > 1 ? 2 : 1;
      XDET_TRY(conv_bn(k.cproj, "", 0.f, 0, pre, cp, &k.shortcut));
    }
  }
  k.op_first = ops.size();
  k.prev_group = carry->group;                    // the bneck group of the block before, if it runs fused
  ConvArgs ca;                                    // (the 3x3, stride 1 or 2, takes its input as planes only)
  ca.cout = f; ca.relu_out = 1; ca.emit.planes = 3;
  XDET_TRY(conv_bn(k.c1, k.b1, 1e-5f, 0, pre, ca, &k.y1, &k.La));
  rewire_preconv(k, *carry);
  Buf y2;
  ConvArgs cb;
  cb.k = 3; cb.cout = f; cb.stride = s; cb.pad_mode = s > 1 ? 2 : 1; cb.pad_expl = 1; cb.relu_out = 1;
  cb.emit.planes = 3;                             // the closing 1x1 always does
  if (k.cat_on) cb.emit.into = &k.cat;
  XDET_TRY(conv_bn(k.c2, k.b2, 1e-5f, 0, k.y1, cb, &y2, &k.Lb));
  XDET_REQUIRE(!k.cat_on || (y2.hi == k.cat.hi && y2.H == k.cat.H && y2.W == k.cat.W), "plan: the 3x3 conv did not take the concatenated operand");
  // The next block opens with BN+ReLU of this block's output.  Fold it in: the closing conv writes its f32
  // output (the identity shortcut) AND relu(bn_next(output)) as planes, and the separate element-wise pass
  // disappears.  (A stage opener's strided projection cannot read those full-resolution planes: see above.)
  float *nsc = nullptr, *nsh = nullptr;
  std::vector<float> nsc_host, nsh_host;
  ConvEmit e3;
  int my_drop_idx = -1;                           // this block's closing conv, if its planes copy is optional
  if (!k.bn_next.empty() && g_default_precision != PREC_F32) {
    XDET_TRY(upload_bn(k.bn_next, 4 * f, round_up(4 * f, 32), 1e-5f, &nsc_host, &nsh_host, &nsc, &nsh));
    e3.planes = 1;
    e3.bn_scale = &nsc_host;                      // (host copies: the conv keeps its own device arrays, which carry the
    e3.bn_shift = &nsh_host;                      //  planes' pre-scale; nsc / nsh stay as they are for the projection)
    // (the planes copy of this block's output has one reader, the next block's opening conv: if that block turns out to
    //  run on a kernel that makes its own pre-activation, it marks this conv's planes as droppable)
    if (g_default_precision == PREC_F16X3) e3.optional = &my_drop_idx;
  }
  if (k.cat_on) {
    const HostTensor *kc, *kp;
    XDET_TRY(need(k.c3 + "/kernel", &kc, {1, 1, f, 4 * f}));
    XDET_TRY(need(k.cproj + "/kernel", &kp, {1, 1, pre.C, 4 * f}));
    std::vector<float> kcat(kc->v);                                   // HWIO, 1 x 1: rows = input channels
    for (float v : kp->v) kcat.push_back(ldexpf(v, k.cat_d));           // (the block-input part is stored * 2^-cat_d)
    k.Lc = keep(new ConvLayer());
    XDET_TRY(k.Lc->init(1, 1, f + pre.C, 4 * f, 1, 1, 1, 0, 0, kcat.data(), nullptr, nullptr, 0));
    XDET_TRY(add_conv(k.c3 + " + " + k.cproj + " [shortcut projection folded into the reduction]", 0, k.cat, k.Lc, nullptr, 0, &k.y3, e3));
  } else {
    ConvArgs cc;
    cc.cout = 4 * f; cc.res = &k.shortcut; cc.emit = e3;
    XDET_TRY(conv_bn(k.c3, "", 0.f, 0, y2, cc, &k.y3, &k.Lc));
  }
  if (nsc) register_bneck(k, *carry);
  carry->group = k.group;
  carry->Lc = k.Lc;
  carry->have_pl = nsc != nullptr && g_default_precision != PREC_F32;
  carry->drop_idx = k.group >= 0 ? -1 : my_drop_idx;      // (a fused block never runs its closing conv's op)
  Buf y3 = k.y3;
  if (nsc) {
    carry->fused_pre = y3;                        // same shape; lives as planes only
    carry->fused_pre.p = nullptr;
    carry->fused_pre.no_f32 = true;
    carry->fused_pre.planes_relu = false;
    y3.hi = y3.lo = nullptr;                      // the f32 tensor itself has no planes
    carry->have_fused = true;
    carry->fused_sc = nsc;
    carry->fused_sh = nsh;
  }
  *x_io = y3;
  return XDET_OK;
}

int ResNetTrunk::build() {
  XDET_REQUIRE(!built, "net already built");
  // stages 3-4 at BASELINE config 2's batch 8 are 57 / 15 M tiles against 72- / 144-step K loops: split-K (option "ksplit")
  if (g_default_precision != PREC_F32 && ksplit_enabled) { ksplit_design_batch = 8; ksplit_all = true; }
  net_precision = g_default_precision;
  Names names;
  Carry carry;
  Buf x;
  XDET_TRY(build_stem(&names, &x, &carry));
  const int filters[4] = {64, 128, 256, 512}, blocks[4] = {3, 4, 6, 3}, strides[4] = {1, 2, 2, 2};
  for (int st = 0; st < 4; ++st)
    for (int b = 0; b < blocks[st]; ++b) {
      Block k;
      k.st = st; k.b = b; k.f = filters[st]; k.s = b == 0 ? strides[st] : 1;
      // the block's names, in the order tf.layers created them: pre-activation BN, projection (stage openers), conv / BN / conv / BN / conv
      k.bn_pre = names.bname();
      if (b == 0) k.cproj = names.cname();
      k.c1 = names.cname(); k.b1 = names.bname(); k.c2 = names.cname(); k.b2 = names.bname(); k.c3 = names.cname();
      if (!(st == 3 && b == blocks[st] - 1)) k.bn_next = names.next_bname();   // (the last block's successor is the closing BN below)
      XDET_TRY(build_block(k, &x, &carry));
    }
  XDET_TRY(add_bn_relu(names.bname(), x, &outb));
  for (const Op& op : ops) flops += std::max(op.flops, 0.0);
  w.clear();
  XDET_TRY(finish_ksplit());
  built = true;
  return XDET_OK;
}

}  // namespace xdet
