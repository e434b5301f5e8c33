// The ResNet-50 v2 trunk (net/resnet_v2.py:311-345) as a static launch plan.
#pragma once
#include "plan.h"

namespace xdet {

// A13: ResNet-50 v2 trunk
struct ResNetTrunk : Plan {
  int image_size = 480;
  bool built = false;
  Buf in4, outb;
  double flops = 0;
  bool ksplit_enabled = true;                      // xdet_resnet_set_option "ksplit" = off: the round-3 launch plan (A/B measurements)
  bool stem7_enabled = true;                       // option "stem7" = off: the stem conv on the generic small-cin kernel (A/B runs, tests)
  bool stem7_direct = false;                       // decided at build: the stem op reads the NCHW images itself
  const float* cur_images = nullptr;               // (graphs are keyed on this pointer)
  bool stem_pool_bn = true;                        // option "stem_pool" = off: pool and pre-activation as two passes (A/B runs, tests)
  bool stem_pool_fused = false;                    // decided at build: the pool pass writes the first block's pre-activation planes
  bool bneck_enabled = true;                       // identity blocks the fused kernel supports run as one launch
  // ONE decision per forward, made at the top of xdet_resnet_forward and read by every op: the fused kernels run (and the
  // planes they keep on the CU are not written).  Part of the graph key.  A trunk instance serves one stream at a time.
  bool bneck_fused_now = false;
  bool projcat_enabled = true;                     // option "projcat" = off: projection shortcuts as their own GEMM + a residual add (A/B runs, tests)
  unsigned short *stem_cat_hi = nullptr, *stem_cat_lo = nullptr;   // second destination of the stem's pool + pre-activation pass
  float stem_cat_mul = 1.f;
  int stem_cat_c32 = 0, stem_cat_pidx = -1;        // (stage 1's projection block reads the block input inside a concatenated operand)
  bool preconv_enabled = true;                     // option "preconv" = off: stage 2's opening 1x1 convs read planes (A/B runs, tests)
  struct PreconvLayers { ConvLayer *Lprev, *La; };  // a conv1x1 that makes its pre-activation from the raw input (resnet_preconv.hip)
  std::vector<PreconvLayers> preconv_layers;
  struct BneckGroup {
    ConvLayer *La, *Lb, *Lc, *Lprev;               // the block's three convs; the closing conv of the block before it
    BneckLaunch a;
    size_t op_first;
    bool next_fused = false;
  };
  std::vector<BneckGroup> bneck_groups;
  // one decision per forward (the answer cannot change inside one): no calibration pass is measuring, and no planes tensor a
  // fused kernel keeps on the CU carries an activation pre-scale
  bool planes_dropped() const override { return (!bneck_groups.empty() || !preconv_layers.empty()) && bneck_fused_now; }
  bool bneck_all_ok() const {
    if (after_op) return false;
    for (const BneckGroup& g : bneck_groups)
      if (g.Lprev->out_exp != 0 || g.La->in_exp != 0 || g.La->out_exp != 0 || g.Lb->in_exp != 0 || g.Lb->out_exp != 0 || g.Lc->in_exp != 0)
        return false;
    for (const PreconvLayers& g : preconv_layers)
      if (g.Lprev->out_exp != 0 || g.La->in_exp != 0 || g.La->out_exp != 0) return false;
    return true;
  }

  // Pre-activation bottlenecks (net/resnet_v2.py:142-184).  The BN+ReLU that follows the two inner
  // convs is folded into their epilogues; the one that opens a block cannot be (the raw block input
  // is also the identity shortcut), so it is its own element-wise pass.
  int add_bn_relu(const std::string& bn, const Buf& in, Buf* out);

  // the names tf.layers gives the trunk's convs and BNs, in creation order
  struct Names {
    int ci = 0, bi = 0;
    static std::string nth(const std::string& base, int i) { return i == 0 ? base : base + "_" + std::to_string(i); }
    std::string cname() { return nth("conv2d", ci++); }
    std::string bname() { return nth("batch_normalization", bi++); }
    std::string next_bname() const { return nth("batch_normalization", bi); }
  };
  // what one block hands to the next
  struct Carry {
    ConvLayer* Lc = nullptr;     // the closing conv of the block before (its planes affine is the next block's pre-activation BN)
    int group = -1;              // its bneck group, if it runs fused
    int drop_idx = -1;           // planes_drop_ok entry of its closing conv (-1: none / that block runs fused)
    bool have_pl = false;        // that conv writes the pre-activation planes of this block
    bool have_fused = false;     // ... which then are fused_pre: planes only, made by the producer of the block input
    Buf fused_pre;
    const float *fused_sc = nullptr, *fused_sh = nullptr;   // their BN (a strided projection applies it to its own subsample)
  };
  // one bottleneck block while it is planned
  struct Block {
    int st = 0, b = 0, f = 0, s = 1;               // stage, index in it, inner width, stride
    std::string bn_pre, cproj, c1, b1, c2, b2, c3, bn_next;
    Buf x, pre, shortcut;                          // the raw block input, its pre-activation, what the closing conv adds
    bool cat_on = false;                           // the projection shortcut runs inside the closing GEMM ...
    Buf cat;                                       // ... over this operand [3x3 output | block input * 2^-cat_d]
    int cat_d = 0;
    size_t op_first = 0;                           // the opening conv's op
    int prev_group = -1, group = -1;               // the bneck group of the block before / of this block (-1: three launches)
    ConvLayer *La = nullptr, *Lb = nullptr, *Lc = nullptr;
    Buf y1, y3;
  };
  int build_stem(Names* names, Buf* x, Carry* carry);
  int build_block(Block& k, Buf* x, Carry* carry);
  int setup_projcat(Block& k, const Carry& carry);
  void rewire_preconv(const Block& k, const Carry& carry);
  void register_bneck(Block& k, const Carry& carry);
  int build();
};

}  // namespace xdet
