// Static launch plans: a net is a list of ops over recycled workspace blocks, built once by the op builders below and
// replayed per forward (eagerly or as a captured graph).
#pragma once
#include "layers.h"

#include <array>
#include <functional>
#include <map>
#include <memory>

namespace xdet {

struct HostTensor {
  std::vector<float> v;
  std::vector<int64_t> dims;
};
typedef std::map<std::string, HostTensor> WeightMap;

struct Buf {
  float* p = nullptr;
  unsigned short *hi = nullptr, *lo = nullptr;   // optional split-precision f16 planes of the same tensor
  bool planes_relu = false;                      // the planes hold relu(tensor)
  bool no_f32 = false;                           // only the planes are ever written (p stays unused)
  int pidx = -1;                                 // entry of Plan::pscales: the planes hold x * 2^-exp
  int H = 0, W = 0, C = 0, ld = 0;
  size_t per_image() const { return (size_t)H * W * ld; }
};

// How Plan::add_conv writes its output besides the f32 tensor (the default: f32 only).  Builders set it when they know the
// output's consumers.
struct ConvEmit {
  // 1 = the conv also writes its output as split planes (a consumer on the LDS-DMA path then needs no split pass), 2 = the
  // planes hold relu(output) (for a consumer that applies ReLU on load), 3 = planes ONLY: every consumer is on the LDS-DMA
  // path, the f32 tensor is never written
  int planes = 0;
  // planes == 3: the planes go into channel blocks [0, ld_out/32) of THIS wider planes tensor (same pixels) instead of a
  // tensor of their own -- the left part of a concatenated operand [this conv's output | what another op wrote]
  const Buf* into = nullptr;
  // host, ld floats each: the planes copy is relu(out * scale + shift), a following BN+ReLU pre-activation folded into this
  // conv's epilogue
  const std::vector<float>* bn_scale = nullptr;
  const std::vector<float>* bn_shift = nullptr;
  // non-NULL: the planes copy is only read by the three-launch form of the next block -- a forward in which planes_dropped()
  // says that block runs fused (resnet_bneck.hip makes its own pre-activation from the f32 tensor) does not write it.
  // add_conv stores the planes_drop_ok entry it registered here (-1: none).
  int* optional = nullptr;
  bool ksplit = false;         // a split-K candidate (plans that split only some layers)
};

// What Plan::conv_bn builds, besides its name, BN, stage, input and output: a call site assigns the members it uses.
struct ConvArgs {
  int k = 1, cout = 0, stride = 1;
  int pad_mode = 1;                 // 0 = VALID, 1 = SAME, 2 = explicit: pad_expl in front, k - 1 in all (resnet_v2.fixed_padding)
  int pad_expl = 0;
  int relu_out = 0, relu_in = 0;
  const Buf* res = nullptr;         // residual added in the epilogue
  // 1x1 stride-2 projections only: the input is a raw tensor and the conv reads relu(in * pre_sc + pre_sh) -- the
  // pre-activation BN of a ResNet v2 block, applied in the subsample pass
  const float *pre_sc = nullptr, *pre_sh = nullptr;
  const Buf* presub = nullptr;      // the raw subsampled planes of the input, where its producer already wrote them
  ConvEmit emit;
};

// ... and Plan::sep_bn: (ReLU ->) separable_conv2d -> BN (-> +res) (-> ReLU), net/xception_body.py:220-234
struct SepArgs {
  int cout = 0, pre_relu = 0, dilation = 1, relu_out = 0;
  const Buf* res = nullptr;
  // the block is followed by max_pooling2d(3, 2, 'same') + tf.add(pool_res) (entry flow, net/xception_body.py:281-286): the
  // output is then the pooled sum
  const Buf* pool_res = nullptr;
  // with pool_res, where the pool runs as the split vertical pass: that pass also writes the raw pooled sum's subsampled
  // planes here (what the NEXT block's 1x1 / stride-2 projection reads) and stores relu(sum) as the output; next_sub->hi
  // stays NULL where that form is not taken
  Buf* next_sub = nullptr;
  ConvEmit emit;
};

// Captured forwards of a plan.  A graph bakes in every pointer it was recorded with (and the per-forward decisions), so the
// key holds all of them; the cache is bounded, oldest-first eviction.
struct GraphCache {
  typedef std::array<uintptr_t, 10> Key;
  static constexpr size_t kMax = 8;
  std::map<Key, hipGraphExec_t> execs;
  std::vector<Key> order;      // capture order, for eviction
  void clear() {
    for (auto& g : execs) (void)hipGraphExecDestroy(g.second);
    execs.clear();
    order.clear();
  }
  // replay the graph of `key` on s; without one, capture `forward` on s first
  int launch(const Key& key, hipStream_t s, const std::function<int()>& forward) {
    auto it = execs.find(key);
    if (it == execs.end()) {
      if (execs.size() >= kMax) {
        const Key old = order.front();
        order.erase(order.begin());
        (void)hipGraphExecDestroy(execs[old]);
        execs.erase(old);
      }
      hipGraph_t g = nullptr;
      XDET_HIP(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
      const int rc = forward();
      const hipError_t e = hipStreamEndCapture(s, &g);
      if (rc != XDET_OK || e != hipSuccess) {
        if (g) (void)hipGraphDestroy(g);
        if (rc != XDET_OK) return rc;
        XDET_HIP(e);
      }
      hipGraphExec_t ge = nullptr;
      const hipError_t ei = hipGraphInstantiate(&ge, g, nullptr, nullptr, 0);
      (void)hipGraphDestroy(g);
      XDET_HIP(ei);
      it = execs.emplace(key, ge).first;
      order.push_back(key);
    }
    XDET_HIP(hipGraphLaunch(it->second, s));
    return XDET_OK;
  }
};

struct Op {
  std::string name;
  int stage;
  double flops;      // algorithmic dense 2*MAC per image (0 for non-contraction ops, < 0: auxiliary pass of one)
  std::function<int(int, hipStream_t)> run;
  double mfma_flops = -1.0;   // FLOPs the op actually executes on the matrix cores per image, all products counted
                              // (-1: the default, products-per-term x flops; the spectral GEMMs and VALU convs set it)
};

struct ProfRec { int op; hipEvent_t a, b; };

struct Plan {
  int plan_kind = -1; // 0 = LightHeadNet, 1 = ResNetTrunk: the C-ABI takes void* handles and checks what it was given
  int device = 0;     // HIP device the plan's weights and workspace live on (current device at creation)
  int max_batch = 1;
  bool profiling = false;
  std::vector<ProfRec> prof;
  std::vector<DevMem<unsigned char>> allocs;               // the pool: every block of alloc_bytes(), freed with the plan
  std::vector<std::pair<const float*, size_t>> f32_bufs;   // every activation tensor of new_buf(): (pointer, floats per image)
  struct PlanesRec { const unsigned short* hi; int64_t pix_per_image; int ld; };
  std::vector<PlanesRec> planes_bufs;                      // ... and of new_planes()
  int net_precision = PREC_F32;                            // precision mode the plan was built in
  std::vector<std::unique_ptr<LayerBase>> layers;
  std::vector<Op> ops;
  WeightMap w;
  GraphCache graphs;

  virtual ~Plan() { graphs.clear(); }
  size_t allocated_bytes = 0;
  int alloc_bytes(size_t bytes, void** out, bool zero = true) {
    DevMem<unsigned char> m;
    XDET_TRY(zero ? m.alloc_zeroed(bytes, 256) : m.alloc(bytes, 256));
    allocated_bytes += std::max<size_t>(bytes, 256);
    *out = m.get();
    allocs.push_back(std::move(m));
    return XDET_OK;
  }
  // a plan-owned device copy of a host vector
  template <class T>
  int upload(const std::vector<T>& h, T** d) {
    XDET_TRY(alloc_bytes(h.size() * sizeof(T), reinterpret_cast<void**>(d), false));
    XDET_HIP(hipMemcpy(*d, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
    return XDET_OK;
  }
  // ---- workspace ----
  // One block per intermediate tensor, EXCEPT that a builder may hand a tensor's block back once its last consumer has been
  // planned (release_f32 / release_planes); a later tensor that fits takes it over (best fit, at most 2x its size): the
  // middle flow's 24 x (planes pair + f32 block output) live in a handful of blocks, the entry flow's blocks serve the
  // exit flow and the head.
  // Ops of one stream run in plan order, so a recycled block is never live twice; the side stream (RPN branch) has its own
  // pool.  Named buffers of the graph-builder API (mid_x, out, feat, ...) are never released.  Option "workspace" = "reuse"
  // (default) | "ssa"; check_range needs every tensor intact after the forward and turns reuse off.
  bool reuse_workspace = true;
  // "workspace" = "poison" (tests): as "reuse", and in front of the first op planned after a recycled f32 block was handed
  // out, everything of that block BEYOND the new tensor (its loader slack and the rest of the larger predecessor) is filled
  // with NaN bits on every forward -- if any consumer used a byte from behind its tensor, the detections would differ from
  // the one-block-per-tensor net's (tests/test_gpu_e2e.py)
  bool poison_recycled = false;
  struct PoisonRec { size_t op; float* at; size_t words; };
  std::vector<PoisonRec> poison;
  std::map<void*, size_t> ws_bytes;                      // blocks handed out by take() that are live
  std::multimap<size_t, void*> ws_free[2][2];            // released blocks by size, per stream pool and kind (f32 / planes)
  std::map<void*, int> ws_kind;
  int ws_pool = 0;                                       // 0 = main stream, 1 = side stream
  size_t ws_recycled_bytes = 0;
  int take(size_t bytes, void** out, int kind = 0, size_t slack_bytes = 0);
  void give(void* p) {
    if (!reuse_workspace || !p) return;
    auto it = ws_bytes.find(p);
    if (it == ws_bytes.end()) return;                    // not a take() block, or released already
    ws_free[ws_pool][ws_kind[p]].insert({it->second, p});
    ws_bytes.erase(it);
  }
  void release_f32(const Buf& b) { give(b.p); }
  void release_planes(const Buf& b) { give(b.hi); give(b.lo); }
  int new_buf(int H, int W, int C, Buf* b) {
    b->H = H; b->W = W; b->C = C;
    b->no_f32 = false;                             // (a Buf that was copied from a planes-only tensor must not keep that flag)
    b->ld = C <= 4 ? 4 : round_up(C, 32);
    // +128 floats of slack: the conv loader may read a full 32-channel slice of the last pixel
    XDET_TRY(take(((size_t)max_batch * b->per_image() + 128) * sizeof(float), reinterpret_cast<void**>(&b->p), 0, 128 * sizeof(float)));
    f32_bufs.emplace_back(b->p, b->per_image());
    return XDET_OK;
  }
  const HostTensor* find(const std::string& name) const {
    auto it = w.find(name);
    return it == w.end() ? nullptr : &it->second;
  }
  int need(const std::string& name, const HostTensor** t, std::initializer_list<int64_t> dims) const {
    *t = find(name);
    if (!*t) {
      set_last_error("missing weight: " + name);
      return XDET_ERR_STATE;
    }
    if ((*t)->dims != std::vector<int64_t>(dims)) {
      set_last_error("weight has wrong shape: " + name);
      return XDET_ERR_INVALID_ARG;
    }
    return XDET_OK;
  }
  int fold_bn(const std::string& bn, int C, float eps, const float* bias, std::vector<float>* scale,
              std::vector<float>* shift) const;
  // fold_bn zero-padded to `ld` channels and uploaded (the host copies stay in *scale / *shift)
  int upload_bn(const std::string& bn, int C, int ld, float eps, std::vector<float>* scale, std::vector<float>* shift,
                float** d_scale, float** d_shift) {
    XDET_TRY(fold_bn(bn, C, eps, nullptr, scale, shift));
    scale->resize(ld, 0.f);
    shift->resize(ld, 0.f);
    XDET_TRY(upload(*scale, d_scale));
    return upload(*shift, d_shift);
  }

  // ---- activation pre-scale of the split-precision operands ----
  // An f16 hi part overflows beyond 65504 (the reference computes in f32 everywhere and has BN-less edges:
  // net/xception_body.py:381-400,450-475).  Every tensor that exists as split planes -- in HBM, or inside a fused
  // separable block -- has a power-of-two exponent e: the planes hold x * 2^-e and the consuming contraction folds 2^e
  // back into its epilogue scale, both exact.  e = 0 (no change at all) unless calibrate() measures a tensor above
  // kRangeTarget on a calibration batch.
  struct PlaneScale {
    std::string name;
    int exp = 0;
    const unsigned short* hi = nullptr;               // measured on the planes themselves ...
    std::function<int64_t(int)> halves;               // ... over this many halves for a batch of N
    const float* src = nullptr;                       // or (the operand a fused block keeps on the CU) bounded from its f32
    size_t src_per_image = 0;                         // input: max|x| (after the input ReLU) * bound
    int src_relu = 0;
    float bound = 1.f;
    std::vector<std::function<int(int)>> apply;       // re-derive the device parameters that carry 2^-e / 2^e
    std::function<int(hipStream_t)> clear;            // optional: zero the padding a measurement would otherwise scan
    // x8 form (option "cross" = "fp8"; conv_params.h): planes written by a depthwise tile kernel for ONE pointwise consumer on
    // the LDS-DMA kernels.  Both ends are fixed at build time (x8_ok); the form is switched on by the calibration pass, which
    // measures the tensor and chooses x8_exp so that its largest |hi| * 2^-x8_exp lands in (128, 256].
    bool x8_cand = false, x8_ok = false, x8_on = false;
    int x8_exp = 0;
    float last_max = 0.f;                             // largest magnitude of the operand in the last calibration pass
    int op_index = -1;                                // measured right behind this op of the plan (-1: after the whole forward)
  };
  std::function<int(int, hipStream_t)> after_op;      // calibration hook: called by run_stage behind every op
  bool cross8 = false;                                // option "cross" = "f16" | "fp8"
  bool plane_x8(int pidx, int* e) const {
    const bool on = pidx >= 0 && pscales[pidx].x8_ok && pscales[pidx].x8_on;
    *e = on ? pscales[pidx].x8_exp : 0;
    return on;
  }
  std::vector<PlaneScale> pscales;
  std::vector<const float*> f32_split_inputs;          // f32 tensors a register-split conv reads (no pre-scale exists for them)
  void f32_limit(const float* p, float* limit, int* relu) const;
  static constexpr float kRangeTarget = 4096.f;       // 16x below the f16 maximum: headroom for images unlike the calibration batch
  float pmul(int pidx) const { return pidx >= 0 ? ldexpf(1.f, -pscales[pidx].exp) : 1.f; }
  int set_plane_exp(int pidx, int e) {
    pscales[pidx].exp = e;
    for (auto& f : pscales[pidx].apply) XDET_TRY(f(e));
    return XDET_OK;
  }

  int calibrate_planes(int N, hipStream_t s, int* n_scaled, const std::function<int(hipStream_t)>& run);

  // ---- split-precision planes ----
  unsigned short* zeros = nullptr;
  int get_zeros() {
    if (!zeros) XDET_TRY(alloc_bytes(256, reinterpret_cast<void**>(&zeros)));
    return XDET_OK;
  }
  int new_planes(Buf* b);
  int add_split(const std::string& name, int stage, const Buf& in, int relu, Buf* out);

  // ---- op builders ----
  std::vector<char> planes_drop_ok;      // per registered conv: its one planes reader turned out to be a kernel that does not read them
  virtual bool planes_dropped() const { return false; }
  // Split-K policy (conv_mfma_ksplit.hip).  ksplit_design_batch > 0: a conv whose grid at THAT batch size (a constant
  // of the plan: 8 for the ResNet trunk = BASELINE config 2, 1 for the detector's single-image latency path) leaves
  // most of the 256 CUs idle gets its K steps cut into S ranges, S = what fills the chip at the design batch, at
  // least 8 steps per range.  S depends on the layer and the plan constant only -- never on the batch of a call.
  int ksplit_design_batch = 0;
  bool ksplit_all = false;             // false: only the layers a builder marks (ConvEmit::ksplit) are candidates
  static int pow2_floor(int64_t v) { int r = 1; while ((int64_t)r * 2 <= v) r *= 2; return r; }
  int maybe_ksplit(ConvLayer* L, int Hi, int Wi, int Ho, int Wo, bool marked);
  struct KsLayer { ConvLayer* L; bool aux; };
  std::vector<KsLayer> ks_layers;
  float* ks_slab[2] = {nullptr, nullptr};
  int* ks_ticket[2] = {nullptr, nullptr};
  int finish_ksplit();
  bool fuse_sepconv = true;      // option "sepconv" = "fused" | "split"
  bool subsample_projections = true;
  bool pool_writes_projection_input = true;   // option "pool_sub" = "on" | "off": blocks 2-3's pool pass also writes the next
                                              // projection's subsampled planes and stores relu(sum) (off: A/B runs, tests)
  bool patch_conv3x3 = true;     // option "conv3x3" = "patch" | "gemm"
  bool fuse_hpool = true;        // option "pool" = "split" | "whole": horizontal half of an entry-flow pool in the producer
  int pool_fuse_min_pixels = 100 * 100;   // ... for the 237 x 237 block (+0.8 %) and the 119 x 119 one (time-neutral, -0.9 GB)
  int add_conv(const std::string& name, int stage, const Buf& in_, ConvLayer* L, const Buf* res, int relu_in, Buf* out,
               const ConvEmit& em = {});
  int add_dw(const std::string& name, int stage, const Buf& in, DepthwiseLayer* L, int relu_in, Buf* out,
             bool planes_only = false);
  int add_pool(const std::string& name, int stage, const Buf& in, const Buf* res, Buf* out);
  ConvLayer* keep(ConvLayer* L) { layers.emplace_back(L); return L; }
  DepthwiseLayer* keep(DepthwiseLayer* L) { layers.emplace_back(L); return L; }
  SpectralConv* keep(SpectralConv* L) { layers.emplace_back(L); return L; }

  // What conv_bn / sep_bn made of which checkpoint names: the door a refresh from trained weights reaches the layers by
  // (LightHeadNet::refresh_weights).  A unit (sep_bn) has a depthwise layer, its kernels are <prefix>/depthwise_kernel and
  // <prefix>/pointwise_kernel; a projection (conv_bn) has <prefix>/kernel.  bn is empty for a conv without one.
  struct LayerRec {
    std::string prefix, bn;
    float eps = 0.f;
    ConvLayer* conv = nullptr;
    DepthwiseLayer* dw = nullptr;
    int pscale = -1;                   // a fused separable block: the PlaneScale whose bound comes from the depthwise taps
  };
  std::vector<LayerRec> layer_recs;
  // max over channels of sum_t |w[t, c]| of a dense [3,3,C,1] kernel: what bounds a fused block's depthwise result
  static float depthwise_bound(const float* k33c1, int C) {
    float bound = 0.f;
    for (int c = 0; c < C; ++c) {
      float a = 0.f;
      for (int t = 0; t < 9; ++t) a += std::fabs(k33c1[(size_t)t * C + c]);
      bound = std::max(bound, a);
    }
    return bound;
  }

  // tf.layers.conv2d(use_bias=False) + BN (+ReLU); *layer (optional): the conv layer it made
  int conv_bn(const std::string& name, const std::string& bn, float eps, int stage, const Buf& in, const ConvArgs& args, Buf* out,
              ConvLayer** layer = nullptr);
  int sep_bn(const std::string& name, float eps, int stage, const Buf& in, const SepArgs& args, Buf* out);
  int run_stage(int stage, int N, hipStream_t s);
  int profile_read(int max_ops, int* n_ops, double* ms, int* launches, double* flops);
};

}  // namespace xdet
