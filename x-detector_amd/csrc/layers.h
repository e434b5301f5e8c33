// Layer objects of libxdet_hip.so: a convolution (its operand buffers are laid out by conv_repack.hip, at creation and at
// every refresh) / a depthwise 3x3 with its padded taps, and the number-format helpers they share with the plans.
#pragma once
#include "common.h"
#include "device_mem.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

namespace xdet {

// A device parameter array that carries an exact power-of-two rescale: the host copy at exponent 0 and its device array
// (not owned), re-uploaded as host * 2^e, zero-padded to n floats where the device array is longer than the host copy.
struct Pow2Scaled {
  std::vector<float> host;
  float* dev = nullptr;
  int upload(int e, size_t n = 0) const {
    std::vector<float> v(std::max(n, host.size()), 0.f);
    for (size_t i = 0; i < host.size(); ++i) v[i] = ldexpf(host[i], e);
    XDET_HIP(hipMemcpy(dev, v.data(), v.size() * sizeof(float), hipMemcpyHostToDevice));
    return XDET_OK;
  }
};

extern int g_default_precision;   // precision mode new layers and plans are created in (cabi.hip)

// (the three converters below run on the device too: the operand repack of conv_repack.hip makes the layers' weights with them)
__host__ __device__ static inline unsigned short f32_to_f16_rne(float f) {
  unsigned x;
  __builtin_memcpy(&x, &f, 4);
  const unsigned sign = (x >> 16) & 0x8000u;
  x &= 0x7FFFFFFFu;
  if (x >= 0x47800000u) return (unsigned short)(sign | (x > 0x7F800000u ? 0x7E00u : 0x7C00u));   // inf / nan
  if (x < 0x38800000u) {                       // below 2^-14: subnormal half = round(|f| * 2^24)
    float af;
    __builtin_memcpy(&af, &x, 4);
    return (unsigned short)(sign | (unsigned)lrintf(af * 16777216.0f));
  }
  const unsigned mant = x & 0x7FFFFFu, exp = (x >> 23) - 127 + 15;
  unsigned h = (exp << 10) | (mant >> 13);
  const unsigned rem = mant & 0x1FFFu;
  if (rem > 0x1000u || (rem == 0x1000u && (h & 1u))) ++h;      // round to nearest even (may carry to inf)
  return (unsigned short)(sign | h);
}
// OCP fp8 e4m3 (bias 7, largest 448 = 0x7e, no infinities), round to nearest even, saturating: the format of the x8 cross-term
// operands (conv_params.h; the device side is v_cvt_pk_fp8_f32 in the producing kernels)
__host__ __device__ static inline unsigned char f32_to_e4m3(float f) {
  const unsigned char sgn = std::signbit(f) ? 0x80 : 0;
  const float a = std::fabs(f);
  if (!(a == a)) return 0x7f;
  if (a >= 448.f) return sgn | 0x7e;
  if (a < 0.015625f) {                                   // below the smallest normal 2^-6: subnormals are multiples of 2^-9
    const int q = (int)std::nearbyint(std::ldexp((double)a, 9));
    return sgn | (unsigned char)q;                       // q = 8 is the encoding of 2^-6 itself
  }
  int e;
  (void)std::frexp(a, &e);                               // a = m * 2^e, m in [0.5, 1)
  e -= 1;
  int q = (int)std::nearbyint(std::ldexp((double)a, 3 - e));   // 8 .. 16
  if (q == 16) { q = 8; ++e; }
  return sgn | (unsigned char)(((e + 7) << 3) | (q - 8));
}
__host__ __device__ static inline float f16_to_f32(unsigned short h) {
  const unsigned sign = (unsigned)(h & 0x8000u) << 16, e = (h >> 10) & 0x1Fu, m = h & 0x3FFu;
  float v;
  if (e == 0) v = ldexpf((float)m, -24);
  else if (e == 31) v = m ? NAN : INFINITY;
  else v = ldexpf((float)(m | 0x400u), (int)e - 25);
  unsigned u;
  __builtin_memcpy(&u, &v, 4);
  u |= sign;
  __builtin_memcpy(&v, &u, 4);
  return v;
}

static inline void same_pad(int n, int k, int s, int d, int* before, int* out) {
  const int k_eff = (k - 1) * d + 1;
  *out = (n + s - 1) / s;
  const int total = std::max((*out - 1) * s + k_eff - n, 0);
  *before = total / 2;   // the extra pixel goes to the bottom / right (TF SAME rule)
}

struct LayerBase {
  virtual ~LayerBase() {}
  int kind = 0;   // 1 conv, 2 depthwise, 3 spectral conv
  int device = 0; // the HIP device the weights live on (current device at creation)
};

// what one ConvLayer::forward reads and writes, everything but the geometry (unset members: absent)
struct ConvIO {
  const float* in = nullptr;                               // f32 input (split in registers) ...
  const unsigned short *in_hi = nullptr, *in_lo = nullptr; // ... or the input as f16 planes (LDS-DMA kernel)
  const unsigned short* zeros = nullptr;                   // 256 B of zeros: the planes' out-of-image taps
  float* out = nullptr;                                    // NULL: planes only
  const float* res = nullptr;                              // residual added in the epilogue
  int relu_in = 0;
  unsigned short *out_hi = nullptr, *out_lo = nullptr;     // planes copy of the output: relu?(out * pl_scale + pl_shift)
  int planes_relu = 0;
  const float *pl_scale = nullptr, *pl_shift = nullptr;    // (NULL: no affine)
  int group_rows = 0, group_live_rows = 0;                 // grouped GEMM (groups > 1): rows per group, live rows of each
  int x8 = 0, x8_exp = 0;                                  // in_lo holds x8 records (conv_params.h)
};

struct ConvLayer : LayerBase {
  int kh, kw, cin, cout, stride, dil, pad_mode, pad_t, pad_l, relu_out;
  int groups = 1;     // > 1: grouped GEMM (1x1 only): weight matrix g serves rows [g*group_rows, (g+1)*group_rows)
  int cin_p, kp, cout_pad, n_tile;
  bool small_cin;
  int precision = PREC_F32;
  DevMem<float> d_wt, d_scale, d_shift;
  DevMem<unsigned short> d_wt_hi, d_wt_lo;
  // the same f16 weights K-blocked as [Kp/32][Cout_pad][32] for the LDS-DMA kernel: one K-step of a
  // tile's B operand is then one contiguous run
  DevMem<unsigned short> d_wt_hi_b, d_wt_lo_b;
  DevMem<unsigned short> d_wt_x8_b;      // x8 form of the K-blocked lo plane (conv_params.h): 32 B fp8(w_lo * 2^9) | 32 B fp8(w_hi * 2^-2) per (K block, row)
  DevMem<unsigned short> d_zeros;      // 256 B of zeros on the layer's device: the source of out-of-image taps
  // Activation pre-scale (split-precision range, Plan::calibrate): the A-operand planes hold x * 2^-in_exp and the
  // epilogue scale carries 2^in_exp (exact: powers of two); a planes copy of the output is written as out * 2^-out_exp
  // through the epilogue's pl_scale / pl_shift.  Both 0 unless a calibration found a tensor near the f16 range.
  Pow2Scaled in_scale;                 // d_scale and its host copy at in_exp = 0
  int in_exp = 0, out_exp = 0;
  // Fixed split of the reduction (conv_mfma_ksplit.hip): a constant of the LAYER, set at plan time; once enabled the
  // layer runs on that kernel at every batch size (its two modes are bit-identical), so results never depend on the batch.
  int ksplit = 0;                      // 0 = the layer is not on the split-K kernel
  int ks_mode = 0;                     // 0 = by grid size, 1 = parallel ranges, 2 = one workgroup per tile (tests)
  int pl_c32 = 0;                      // planes destination wider than the output (conv_params.h pl_c32); 0: its own planes tensor
  bool ks_narrow = false;              // 128 x 64 tiles although the layer is a multiple of 128 wide (one range, twice the workgroups)
  int64_t ks_tiles = 0;                // tiles the scratch below was sized for
  // what the launch reads: the layer's own pair below, or the plan's (Plan::finish_ksplit: one per stream, shared by its layers)
  float* d_ks_partial = nullptr;
  int* d_ks_ticket = nullptr;          // 4096 zeroed ints: arrival tickets of the in-kernel fold (conv_params.h ks_ticket)
  DevMem<float> ks_own_partial;        // a stand-alone layer's own scratch (xdet_conv_set_ksplit)
  DevMem<int> ks_own_ticket;
  size_t ks_scratch_bytes(int S, int64_t tiles) const {
    return S > 1 ? (size_t)std::max<int64_t>(tiles, 1) * S * 128 * (cout_pad % 128 == 0 ? 128 : 64) * sizeof(float) : 0;
  }
  // S > 1: the layer allocates its own slab (stand-alone layers behind xdet_conv_set_ksplit); inside a plan the ops of one
  // stream run one after the other, so all its split-K layers borrow ONE slab sized for the largest of them (finish_ksplit)
  int enable_ksplit(int S, int64_t max_parallel_tiles) {
    XDET_REQUIRE(S >= 1 && S <= 16 && dma_capable() && groups == 1, "ksplit: 1..16 ranges, a split-precision non-grouped layer");
    ks_own_partial.reset();
    ks_own_ticket.reset();
    d_ks_partial = nullptr;
    d_ks_ticket = nullptr;
    ks_tiles = std::max<int64_t>(max_parallel_tiles, 1);
    if (S > 1) {
      XDET_TRY(ks_own_partial.alloc(ks_scratch_bytes(S, ks_tiles) / sizeof(float)));
      XDET_TRY(ks_own_ticket.alloc_zeroed(4096));
      d_ks_partial = ks_own_partial;
      d_ks_ticket = ks_own_ticket;
    }
    ksplit = S;
    return XDET_OK;
  }
  DevMem<float> d_pl_scale, d_pl_shift;
  // Every buffer above is filled by the repack of conv_repack.hip from a dense f32 [kh,kw,cin,cout] kernel in device
  // memory: by init() at creation and again by set_kernel_device, which holds what init() would have made of the same
  // values.  What the repack keeps between the two (split-precision layers): the epilogue scale init() was given, in
  // front of the rows' pre-scale, and the row maxima's scratch.  After a refresh in_scale.host no longer describes
  // d_scale: host_stale, and set_in_exp refuses.
  DevMem<float> d_repack_scale0;
  DevMem<unsigned> d_repack_max;
  bool host_stale = false;
  int set_kernel_device(const float* k_hwio, const float* shift, hipStream_t s);
  int set_in_exp(int e) {
    XDET_REQUIRE(!host_stale, "conv: the kernel was refreshed on the device (xdet_conv_set_kernel_device): the host copy of the "
                              "epilogue scale is stale, an activation exponent cannot be applied");
    XDET_TRY(in_scale.upload(e));
    in_exp = e;
    return XDET_OK;
  }
  // planes copy of the output: relu?(out * pl_scale + pl_shift).  Without a folded BN pl = (2^-e, 0); with one (the
  // pre-activation of the next ResNet block, net/resnet_v2.py:142-156) pl = (bn_scale 2^-e, bn_shift 2^-e):
  // relu(x s + h) 2^-e = relu(x (s 2^-e) + h 2^-e), exactly.
  Pow2Scaled pl_scale, pl_shift;   // d_pl_scale / d_pl_shift at e = 0: the folded BN, or (ones, nothing); zero beyond the BN's length
  int set_planes_bn(const std::vector<float>& sc, const std::vector<float>& sh) {
    pl_scale.host = sc;
    pl_shift.host = sh;
    return set_out_exp(0);
  }
  int set_out_exp(int e) {
    const size_t n = (size_t)std::max(cout_pad, ld_out());
    if (!d_pl_scale) {
      XDET_TRY(d_pl_scale.alloc(n));
      XDET_TRY(d_pl_shift.alloc(n));
      pl_scale.dev = d_pl_scale;
      pl_shift.dev = d_pl_shift;
    }
    if (pl_scale.host.empty()) pl_scale.host.assign(n, 1.f);
    XDET_TRY(pl_scale.upload(-e, n));
    XDET_TRY(pl_shift.upload(-e, n));
    out_exp = e;
    return XDET_OK;
  }

  // groups_ > 1: w_hwio is [groups][cin][cout] (1x1), scale/shift are [groups][cout].  Allocates the operand buffers of the
  // layer's precision / small_cin / groups combination, uploads the dense kernel and has the repack fill them
  // (conv_repack.hip); synchronous: the layer is complete on return
  int init(int kh_, int kw_, int cin_, int cout_, int stride_, int dil_, int pad_mode_, int pad_t_, int pad_l_,
           const float* w_hwio, const float* scale, const float* shift, int relu_out_, int groups_ = 1);

  void out_shape(int H, int W, int* Ho, int* Wo, int* pt, int* pl) const {
    if (pad_mode == 1) {
      same_pad(H, kh, stride, dil, pt, Ho);
      same_pad(W, kw, stride, dil, pl, Wo);
    } else {
      *pt = pad_mode == 2 ? pad_t : 0;
      *pl = pad_mode == 2 ? pad_l : 0;
      // explicit padding is symmetric-or-trailing as in resnet_v2.fixed_padding: total = k-1
      const int tot_h = pad_mode == 2 ? (kh - 1) * dil : 0, tot_w = pad_mode == 2 ? (kw - 1) * dil : 0;
      *Ho = (H + tot_h - ((kh - 1) * dil + 1)) / stride + 1;
      *Wo = (W + tot_w - ((kw - 1) * dil + 1)) / stride + 1;
    }
  }
  int ld_in() const { return small_cin ? 4 : round_up(cin, 32); }
  int ld_out() const { return round_up(cout, 32); }
  double flops(int H, int W) const {
    int Ho, Wo, a, b;
    out_shape(H, W, &Ho, &Wo, &a, &b);
    return 2.0 * Ho * Wo * (double)cin * cout * kh * kw;
  }

  int forward(const ConvIO& io, int N, int H, int W, int ldi, int ldo, hipStream_t s) const {
    XDET_REQUIRE(ldi == ld_in(), "conv: ld_in must be round_up(cin,32) (4 for cin<=4)");
    XDET_REQUIRE(ldo == ld_out(), "conv: ld_out must be round_up(cout,32)");
    ConvParams p;
    p.in = io.in; p.wt = d_wt; p.wt_hi = d_wt_hi; p.wt_lo = d_wt_lo; p.out = io.out; p.scale = d_scale; p.shift = d_shift; p.res = io.res;
    p.N = N; p.H = H; p.W = W; p.ldi = ldi; p.ldo = ldo; p.ldr = ldo;
    out_shape(H, W, &p.Ho, &p.Wo, &p.pad_t, &p.pad_l);
    XDET_REQUIRE(p.Ho > 0 && p.Wo > 0, "conv: empty output");
    p.Cin_p = cin_p; p.Kp = kp; p.Cout_pad = cout_pad;
    p.KH = kh; p.KW = kw; p.stride = stride; p.dil = dil;
    p.M = N * p.Ho * p.Wo;
    p.relu_in = io.relu_in; p.relu_out = relu_out;
    p.in_hi = io.in_hi; p.in_lo = io.in_lo; p.zeros = io.zeros;
    p.out_hi = precision == PREC_F32 ? nullptr : io.out_hi; p.out_lo = io.out_lo; p.planes_relu = io.planes_relu;
    p.pl_scale = io.pl_scale; p.pl_shift = io.pl_shift; p.pl_c32 = pl_c32;
    p.group_rows = 0; p.group_wt_stride = 0;
    if (groups > 1) {
      XDET_REQUIRE(io.in_hi && io.group_rows > 0 && io.group_rows % 128 == 0 && (int64_t)io.group_rows * groups == p.M,
                   "conv(grouped): M must be groups * group_rows, group_rows a multiple of 128, input as planes");
      XDET_REQUIRE(io.group_live_rows >= 0 && io.group_live_rows <= io.group_rows, "conv(grouped): live rows beyond the group");
      p.group_rows = io.group_rows;
      p.group_wt_stride = (long long)cout_pad * kp;
      p.group_live_rows = io.group_live_rows;
    }
    if (precision == PREC_F32) return launch_conv_mfma_f32(p, small_cin, n_tile, s);
    if (io.in_hi) {   // A operand already split into f16 planes by its producer: LDS-DMA kernel
      XDET_REQUIRE(!small_cin && io.relu_in == 0, "conv(dma): needs >= 32 input channels and no ReLU-on-load");
      p.wt_hi = d_wt_hi_b; p.wt_lo = d_wt_lo_b;   // K-blocked copies
      if (io.x8) {                                // `in_lo` holds [hi8 | lo8] records: the cross terms run on the fp8 MFMA
        XDET_REQUIRE(d_wt_x8_b && precision == PREC_F16X3 && ksplit < 1, "conv: x8 planes need a pointwise f16x3 layer without a split-K");
        p.wt_lo = d_wt_x8_b; p.x8 = 1; p.x8_exp = io.x8_exp;
      }
      if (ksplit >= 1 && groups == 1) {
        // a split-K layer's summation tree is part of its definition: a batch whose planes leave the kernel's 4 GiB
        // addressing is an error, not a silent change of kernel family (results must not depend on the batch).  ONE range
        // is the plain kernels' reduction (bit-identical): such a layer just runs on them.
        if (!conv_ksplit_supported(kh, kw, (int64_t)N * H * W, ldi, cin_p, cout_pad)) {
          if (ksplit == 1 && !ks_narrow) return launch_conv_mfma_dma(p, n_tile, precision == PREC_F16X3 ? 3 : 1, s);
          XDET_REQUIRE(ksplit == 1, "conv(ksplit): this batch's planes or weights exceed the split-K kernel's 4 GiB addressing (or the "
                                    "filter is not 1x1 / 3x3); a split reduction cannot change kernel family: run smaller batches");
          return launch_conv_mfma_dma(p, 64, precision == PREC_F16X3 ? 3 : 1, s);
        }
        p.ksplit = ksplit; p.ks_partial = d_ks_partial; p.ks_ticket = d_ks_ticket;
        return launch_conv_mfma_ksplit(p, cout_pad % 128 == 0 && !ks_narrow ? 128 : 64, precision == PREC_F16X3 ? 3 : 1, ks_mode, ks_tiles, s);
      }
      return launch_conv_mfma_dma(p, n_tile, precision == PREC_F16X3 ? 3 : 1, s);
    }
    return launch_conv_mfma_split(p, small_cin, n_tile, precision == PREC_F16X3 ? 3 : 1, s);
  }
  // can this layer consume pre-split f16 planes (conv_mfma_dma.hip)?
  bool dma_capable() const { return precision != PREC_F32 && !small_cin; }
};

// One T-tap SAME convolution along one image axis in the DFT domain of that axis (spectral.hip): forward DFT of every
// line -> one real GEMM per frequency bin (a grouped ConvLayer) -> inverse DFT with out = relu?(y * scale + shift).
// The layer owns its tables, block matrices and epilogue arrays; the DFT-domain tensors live in a workspace of the
// caller: split planes x_hi / x_lo of planes_halves(N) halves each and the f32 products y of y_floats(N) floats
// (+ 512 bytes of slack each).  The three passes are separate members so that a plan can time them as three ops.
struct SpectralConv : LayerBase {
  int F = 0, NB = 0, T = 0, axis = 0, cin = 0, cin_ld = 0, cout = 0, cout_ld = 0, relu = 0;
  ConvLayer G;                           // [NB] groups of [2 cin_ld x 2 cout_ld] real block matrices
  DevMem<double> d_tw;                   // the twiddle table of spectral_weights.h: cr [NB][T], then ci [NB][T]
  Pow2Scaled tab_fwd;                    // the forward table carries the operand planes' activation pre-scale 2^-e
  DevMem<float> d_tf, d_ti, d_scale, d_shift;
  // rows per bin at a batch of N: whole 256-row GEMM tiles; a single image or two (N*F <= 128) get the 128-row tile instead
  static int m_pad(int F, int N) { return N * F <= 128 ? 128 : round_up(N * F, 256); }
  int m_pad(int N) const { return m_pad(F, N); }
  size_t planes_halves(int N) const { return (size_t)NB * m_pad(N) * 2 * cin_ld; }
  size_t y_floats(int N) const { return (size_t)NB * m_pad(N) * 2 * cout_ld; }
  // w: [T][cin][cout] (the taps along `axis`: 0 = y, 1 = x); scale / shift: [cout] or NULL (ones / zeros)
  int init(const float* w, int T_, int cin_, int cout_, int axis_, int F_, const float* scale, const float* shift, int relu_) {
    XDET_REQUIRE(w && T_ > 0 && T_ % 2 == 1 && T_ <= kSpectralMaxTaps && cin_ > 0 && cout_ > 0 && (axis_ == 0 || axis_ == 1),
                 "spectral conv: an odd number of taps (<= 15) along axis 0 | 1");
    XDET_REQUIRE(spectral_supported(F_), "spectral conv: the feature-map side must be 16, 30 or 50");
    XDET_REQUIRE(g_default_precision != PREC_F32, "spectral conv: needs a split-precision mode");
    kind = 3;
    F = F_; NB = spectral_points(F) / 2; T = T_; axis = axis_; relu = relu_;
    cin = cin_; cin_ld = round_up(cin, 32); cout = cout_; cout_ld = round_up(cout, 32);
    {
      std::vector<float> wb;
      spectral_weights(w, T, cin, cout, cin_ld, cout_ld, F, &wb);
      XDET_TRY(G.init(1, 1, 2 * cin_ld, 2 * cout_ld, 1, 1, 0, 0, 0, wb.data(), nullptr, nullptr, 0, NB));
    }
    device = G.device;
    {
      std::vector<double> cr, ci;        // what set_kernel_device evaluates the block matrices from, on the device
      spectral_twiddles(T, F, &cr, &ci);
      cr.insert(cr.end(), ci.begin(), ci.end());
      XDET_TRY(d_tw.upload(cr.data(), cr.size()));
    }
    std::vector<float> ti, sc(cout_ld, 0.f), sh(cout_ld, 0.f);
    spectral_tables(F, &tab_fwd.host, &ti);
    for (int c = 0; c < cout; ++c) { sc[c] = scale ? scale[c] : 1.f; sh[c] = shift ? shift[c] : 0.f; }
    XDET_TRY(d_tf.upload(tab_fwd.host.data(), tab_fwd.host.size()));
    XDET_TRY(d_ti.upload(ti.data(), ti.size()));
    XDET_TRY(d_scale.upload(sc.data(), sc.size()));
    XDET_TRY(d_shift.upload(sh.data(), sh.size()));
    tab_fwd.dev = d_tf;
    return XDET_OK;
  }
  // Every operand buffer of G from a dense [T][cin][cout] kernel in device memory, in place (conv_repack.hip): the two passes
  // of the conv repack with spectral_weight_element as their source, at G's own activation exponent -- G then holds what
  // init() followed by set_in_exp(G.in_exp) would have made of the same values.  scale / shift: dense [cout] device arrays
  // that replace the inverse pass's d_scale / d_shift (NULL: kept).  No synchronisation; G.in_scale.host is stale afterwards.
  int set_kernel_device(const float* w, const float* scale, const float* shift, hipStream_t s);
  // the forward transform is linear: 2^-e rides in its table and 2^e in the per-bin GEMM's epilogue scale
  int set_in_exp(int e) {
    XDET_TRY(tab_fwd.upload(-e));
    return G.set_in_exp(e);
  }
  int dft_fwd(const float* in, int N, unsigned short* x_hi, unsigned short* x_lo, hipStream_t s) const {
    return launch_dft_fwd(in, F, cin_ld, axis, N, m_pad(N), d_tf, x_hi, x_lo, s);
  }
  int gemm(int N, const unsigned short* x_hi, const unsigned short* x_lo, float* y, hipStream_t s) const {
    ConvIO io;                   // NB groups of m_pad(N) rows, N * F of them live
    io.in_hi = x_hi; io.in_lo = x_lo; io.zeros = G.d_zeros; io.out = y;
    io.group_rows = m_pad(N); io.group_live_rows = N * F;
    return G.forward(io, 1, 1, NB * m_pad(N), 2 * cin_ld, 2 * cout_ld, s);
  }
  int dft_inv(int N, const float* y, float* out, int ldo, hipStream_t s) const {
    return launch_dft_inv(y, F, 2 * cout_ld, cout_ld, N, m_pad(N), d_ti, d_scale, d_shift, relu, out, ldo, axis, s);
  }
  int forward(const float* in, int N, unsigned short* x_hi, unsigned short* x_lo, float* y, float* out, int ldo,
              hipStream_t s) const {
    XDET_TRY(dft_fwd(in, N, x_hi, x_lo, s));
    XDET_TRY(gemm(N, x_hi, x_lo, y, s));
    return dft_inv(N, y, out, ldo, s);
  }
};

struct DepthwiseLayer : LayerBase {
  int C, dil, ld;
  DevMem<float> d_w;
  Pow2Scaled taps;               // d_w and its host copy: a planes-producing depthwise carries its activation pre-scale in them
  int out_exp = 0;
  bool host_stale = false;       // d_w was rewritten on the device (set_kernel_device, conv_repack.hip): taps.host is not d_w
  int set_kernel_device(const float* k33c1, hipStream_t s);
  int set_out_exp(int e) {       // every partial sum of the FMA chain scales exactly with a power of two
    XDET_REQUIRE(!host_stale, "depthwise: the kernel was refreshed on the device (xdet_depthwise_set_kernel_device): the host "
                              "copy of the taps is stale, an activation exponent cannot be applied");
    XDET_TRY(taps.upload(-e));
    out_exp = e;
    return XDET_OK;
  }
  int init(int C_, int dil_, const float* w33c1) {
    XDET_REQUIRE(C_ > 0 && dil_ > 0 && w33c1, "depthwise: bad arguments");
    kind = 2;
    XDET_HIP(hipGetDevice(&device));
    C = C_; dil = dil_; ld = round_up(C, 32);
    std::vector<float> w((size_t)9 * ld, 0.f);
    for (int t = 0; t < 9; ++t)
      for (int c = 0; c < C; ++c) w[(size_t)t * ld + c] = w33c1[(size_t)t * C + c];
    XDET_TRY(d_w.upload(w.data(), w.size()));
    taps.host = w;
    taps.dev = d_w;
    return XDET_OK;
  }
  int forward(const float* in, int N, int H, int W, int ld_, float* out, int relu_in, hipStream_t s) const {
    XDET_REQUIRE(ld_ == ld, "depthwise: ld must be round_up(C,32)");
    return launch_depthwise3x3(in, d_w, out, N, H, W, C, ld, dil, relu_in, s);
  }
};

}  // namespace xdet
