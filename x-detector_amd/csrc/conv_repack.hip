// The operand buffers of a conv layer, made on the device from a dense f32 kernel in device memory: the one statement of
// their layouts (layers.h names the buffers).  Two callers: ConvLayer::init uploads the kernel it was given and repacks it
// once, at creation (all groups of a grouped layer in one launch); xdet_conv_set_kernel_device (include/xdet.h) repacks a
// layer in place from the optimizer's master copy after a step.  Both run the same two kernels, so a refreshed layer and
// a created one hold the same bits.  The depthwise refresh, xdet_depthwise_set_kernel_device, is here too: its layout is
// DepthwiseLayer::init's padded host copy, restated in five lines.  The table door, xdet_layers_refresh_device, runs the same
// per-tile device code over any number of layers in a fixed number of launches (a tile -> slot table in the workspace), and
// xdet_bn_fold makes a net-owned layer's epilogue scale and shift from the four arrays of its batch norm on the device.
// xdet_spectral_conv_set_kernel_device refreshes the grouped layer of a spectral conv by the same two passes, their source the
// block matrices' element function (spectral_weights.h) instead of a load: the tile code takes its source as a template argument.
//
// The repack makes two passes over the kernel [kh*kw][cin][cout] (a row of the transposed matrix, kh*kw*cin_p values of one
// output channel strided by cout, does not fit in LDS for the 15x1 convs): the largest |w| per output channel (an integer
// atomicMax on the bits of |w|: a maximum has no order to fix), then per 32 (K) x 64 (cout) tile the exponent, the
// pre-scale, the hi / lo split and the scatter into every buffer the layer owns.  The tile is read along cout (256 B per
// K index), transposed through LDS and written along K: 16 B per thread, 64 B per output row of d_wt_hi / d_wt_lo and one
// contiguous 4 KiB run of the K-blocked copies.  The number formats are layers.h's converters.  The file is compiled with
// -ffp-contract=off, as it was when these kernels were part of optimizer.hip.
#include "layers.h"

namespace xdet {

constexpr int RP_T = 256;
constexpr int RP_CO = 64, RP_K = 32;    // a tile: 64 output channels x one K block

// (arrays "per row": [groups][cout_pad]; a matrix: [groups][cout_pad][kp], K-blocked [groups][kp/32][cout_pad][32])
struct ConvRepack {
  const float* w;                       // [groups][taps][cin][cout] dense
  const float* shift;                   // [groups][cout], or NULL: d_shift stays as it is
  float* scale0;                        // per row: the epilogue scale the layer was created with (the table door may replace it)
  unsigned* mx;                         // per row: bits of the largest |w| (pass 1)
  float* wt;                            // f32 mode: the matrix
  unsigned short *hi, *lo, *hi_b, *lo_b;
  unsigned char* x8_b;
  float *d_scale, *d_shift;
  int taps, cin, cout, cin_p, kp, cout_pad;
  // the table door only (the per-layer callers leave them NULL / 0 / their layer's precision):
  const float* scale_new;               // [cout] dense: replaces the creation-time epilogue scale (scale0, or d_scale in f32 mode)
  int in_exp;                           // the layer's activation exponent: d_scale ends as (scale 2^-sh_k) 2^in_exp
  int precision;
  int first_tile, tiles_x;              // the slot's tiles are first_tile + by * tiles_x + bx
};

// Where a tile's values come from: the value of row co, column k of group g's padded [cout_pad][kp] matrix.  The tile code
// below takes the source as a template argument and shares every line behind the fetch.
// A conv layer: a load from the dense kernel, k = tap * cin_p + ci
struct DenseSource {
  __device__ __forceinline__ float operator()(const ConvRepack& a, int g, int co, int k) const {
    const int tap = k / a.cin_p, ci = k - tap * a.cin_p;
    return (tap < a.taps && ci < a.cin && co < a.cout) ? a.w[(((size_t)g * a.taps + tap) * a.cin + ci) * a.cout + co] : 0.f;
  }
};
// The grouped layer of a spectral conv: group g is frequency bin g, and the value is spectral_weight_element of the dense
// [T][cin][cout] kernel and the layer's twiddle table (doubles; a bin's 2 T coefficients are uniform over a workgroup).  A
// tile's 64 threads of one k read 64 neighbouring output channels of each tap: along cout, as the dense source does.
struct SpectralSource {
  const float* w;                       // [T][cin][cout] dense
  const double *cr, *ci;                // [NB][T] each
  int T, cin, cout, cin_ld, cout_ld;
  __device__ __forceinline__ float operator()(const ConvRepack&, int g, int co, int k) const {
    return spectral_weight_element(w, cr, ci, T, cin, cout, cin_ld, cout_ld, g, k, co);
  }
};

template <class Source>
__device__ __forceinline__ void repack_max_tile(const ConvRepack& a, const Source& source, int bx, int by, int g) {
  const int co = bx * RP_CO + (threadIdx.x & (RP_CO - 1));
  const int k0 = by * RP_K + (threadIdx.x / RP_CO) * (RP_K / 4);
  if (co >= a.cout) return;
  float m = 0.f;
#pragma unroll
  for (int i = 0; i < RP_K / 4; ++i) {
    const float f = fabsf(source(a, g, co, k0 + i));
    m = m < f ? f : m;                  // (std::max's own comparison: a NaN never becomes the maximum)
  }
  if (m > 0.f) atomicMax(a.mx + (size_t)g * a.cout_pad + co, __float_as_uint(m));
}

// the epilogue scale of row `grow` in front of the row's pre-scale: the creation-time one, or the table door's replacement
// (which it also leaves in scale0, so that a later per-layer refresh builds on it; padding rows stay +0)
__device__ __forceinline__ float repack_scale0(const ConvRepack& a, float* keep, size_t grow, int co) {
  if (!a.scale_new) return keep[grow];
  const float s = co < a.cout ? a.scale_new[co] : 0.f;
  keep[grow] = s;
  return s;
}

template <class Source>
__device__ __forceinline__ void repack_tile(const ConvRepack& a, const Source& source, int precision, int bx, int kb, int g,
                                            float (*tile)[RP_CO + 1]) {
  const int tid = threadIdx.x;
  const int co0 = bx * RP_CO;
  {
    const int c = tid & (RP_CO - 1), kq = tid / RP_CO;
#pragma unroll
    for (int i = 0; i < RP_K / 4; ++i) tile[kq * (RP_K / 4) + i][c] = source(a, g, co0 + c, kb * RP_K + kq * (RP_K / 4) + i);
  }
  __syncthreads();
  const int c = tid >> 2, q = tid & 3;                      // output row co0 + c, columns kb * 32 + q * 8 .. + 7
  const int co = co0 + c;
  const size_t grow = (size_t)g * a.cout_pad + co;          // the row among all groups' rows
  const size_t row = grow * a.kp + (size_t)kb * RP_K + q * 8;
  if (precision == PREC_F32) {
    float4 lo4 = make_float4(tile[q * 8 + 0][c], tile[q * 8 + 1][c], tile[q * 8 + 2][c], tile[q * 8 + 3][c]);
    float4 hi4 = make_float4(tile[q * 8 + 4][c], tile[q * 8 + 5][c], tile[q * 8 + 6][c], tile[q * 8 + 7][c]);
    *reinterpret_cast<float4*>(a.wt + row) = lo4;
    *reinterpret_cast<float4*>(a.wt + row + 4) = hi4;
    if (kb == 0 && q == 0) {
      if (a.scale_new) {                                 // (f32 mode: d_scale is the scale itself, times 2^in_exp as set_in_exp leaves it)
        const float sc = repack_scale0(a, a.d_scale, grow, co);
        if (a.in_exp) a.d_scale[grow] = ldexpf(sc, a.in_exp);
      }
      if (a.shift && co < a.cout) a.d_shift[grow] = a.shift[(size_t)g * a.cout + co];
    }
    return;
  }
  // per-output-channel power-of-two pre-scale so that max|w| lands in [512, 1024): w_hi cannot overflow f16 and
  // w_lo (~2^-11 |w|) stays a normal f16; undone exactly in the epilogue scale
  const float mx = __uint_as_float(a.mx[grow]);
  int e = 0;
  if (mx > 0.f) (void)frexpf(mx, &e);
  const int sh_k = mx > 0.f ? 10 - e : 0;
  union { unsigned short h[8]; uint4 v; } H, L;
  union { unsigned char b[8]; uint2 v; } X_lo, X_hi;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const float wv = ldexpf(tile[q * 8 + i][c], sh_k);
    const unsigned short h = f32_to_f16_rne(wv);
    H.h[i] = h;
    L.h[i] = precision == PREC_F16X3 ? f32_to_f16_rne(wv - f16_to_f32(h)) : (unsigned short)0;
    if (a.x8_b) {
      X_lo.b[i] = f32_to_e4m3(ldexpf(f16_to_f32(L.h[i]), 9));
      X_hi.b[i] = f32_to_e4m3(ldexpf(f16_to_f32(h), -2));
    }
  }
  const size_t brow = ((size_t)g * (a.kp / RP_K) + kb) * a.cout_pad + co;   // the row of K block kb
  const size_t blk = brow * RP_K + q * 8;
  if (a.hi) *reinterpret_cast<uint4*>(a.hi + row) = H.v;
  if (a.lo) *reinterpret_cast<uint4*>(a.lo + row) = L.v;
  if (a.hi_b) *reinterpret_cast<uint4*>(a.hi_b + blk) = H.v;
  if (a.lo_b) *reinterpret_cast<uint4*>(a.lo_b + blk) = L.v;
  if (a.x8_b) {
    unsigned char* rec = a.x8_b + brow * 64 + q * 8;
    *reinterpret_cast<uint2*>(rec) = X_lo.v;
    *reinterpret_cast<uint2*>(rec + 32) = X_hi.v;
  }
  if (kb == 0 && q == 0) {
    // what init leaves, then what set_in_exp(in_exp) makes of it: two exact power-of-two steps
    const float sc = ldexpf(repack_scale0(a, a.scale0, grow, co), -sh_k);
    a.d_scale[grow] = a.in_exp ? ldexpf(sc, a.in_exp) : sc;
    if (a.shift && co < a.cout) a.d_shift[grow] = a.shift[(size_t)g * a.cout + co];
  }
}

// one layer per launch: ConvLayer::init and xdet_conv_set_kernel_device
__global__ __launch_bounds__(RP_T) void conv_repack_max_kernel(ConvRepack a) {
  repack_max_tile(a, DenseSource(), blockIdx.x, blockIdx.y, blockIdx.z);
}

__global__ __launch_bounds__(RP_T) void conv_repack_kernel(ConvRepack a, int precision) {
  __shared__ float tile[RP_K][RP_CO + 1];
  repack_tile(a, DenseSource(), precision, blockIdx.x, blockIdx.y, blockIdx.z, tile);
}

// the grouped layer of a spectral conv, one bin per blockIdx.z (SpectralConv::set_kernel_device)
__global__ __launch_bounds__(RP_T) void spectral_repack_max_kernel(ConvRepack a, SpectralSource src) {
  repack_max_tile(a, src, blockIdx.x, blockIdx.y, blockIdx.z);
}

__global__ __launch_bounds__(RP_T) void spectral_repack_kernel(ConvRepack a, SpectralSource src, int precision) {
  __shared__ float tile[RP_K][RP_CO + 1];
  repack_tile(a, src, precision, blockIdx.x, blockIdx.y, blockIdx.z, tile);
}

// the inverse pass's arrays [cout_ld] from dense [cout] ones (NULL: kept); channels past cout stay +0
__global__ __launch_bounds__(256) void spectral_epilogue_kernel(const float* __restrict__ scale, const float* __restrict__ shift,
                                                                int cout, float* __restrict__ d_scale, float* __restrict__ d_shift) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= cout) return;
  if (scale) d_scale[c] = scale[c];
  if (shift) d_shift[c] = shift[c];
}

// a table of layers per launch (xdet_layers_refresh_device): workgroup b works on tile b - first_tile of slot tile_slot[b]
__global__ __launch_bounds__(RP_T) void conv_repack_max_table_kernel(const ConvRepack* __restrict__ slots, const int* __restrict__ tile_slot) {
  const ConvRepack a = slots[tile_slot[blockIdx.x]];
  if (a.precision == PREC_F32) return;
  const int t = (int)blockIdx.x - a.first_tile;
  repack_max_tile(a, DenseSource(), t % a.tiles_x, t / a.tiles_x, 0);
}

__global__ __launch_bounds__(RP_T) void conv_repack_table_kernel(const ConvRepack* __restrict__ slots, const int* __restrict__ tile_slot) {
  __shared__ float tile[RP_K][RP_CO + 1];
  const ConvRepack a = slots[tile_slot[blockIdx.x]];
  const int t = (int)blockIdx.x - a.first_tile;
  repack_tile(a, DenseSource(), a.precision, t % a.tiles_x, t / a.tiles_x, 0, tile);
}

// every operand buffer of L from the dense kernel w (device memory); shift NULL: d_shift stays as it is
static ConvRepack conv_repack_args(const ConvLayer& L, const float* w, const float* shift) {
  ConvRepack a;
  a.w = w; a.shift = shift; a.scale0 = L.d_repack_scale0; a.mx = L.d_repack_max;
  a.wt = L.d_wt; a.hi = L.d_wt_hi; a.lo = L.d_wt_lo; a.hi_b = L.d_wt_hi_b; a.lo_b = L.d_wt_lo_b;
  a.x8_b = reinterpret_cast<unsigned char*>(L.d_wt_x8_b.get());
  a.d_scale = L.d_scale; a.d_shift = L.d_shift;
  a.taps = L.kh * L.kw; a.cin = L.cin; a.cout = L.cout; a.cin_p = L.cin_p; a.kp = L.kp; a.cout_pad = L.cout_pad;
  a.scale_new = nullptr; a.in_exp = 0; a.precision = L.precision; a.first_tile = 0; a.tiles_x = a.cout_pad / RP_CO;
  return a;
}

static int launch_conv_repack(const ConvLayer& L, const float* w, const float* shift, hipStream_t s) {
  XDET_REQUIRE(L.cout_pad % RP_CO == 0 && L.kp % RP_K == 0, "conv repack: unexpected padding");
  const ConvRepack a = conv_repack_args(L, w, shift);
  const dim3 grid((unsigned)(a.cout_pad / RP_CO), (unsigned)(a.kp / RP_K), (unsigned)L.groups);
  if (L.precision != PREC_F32) {
    XDET_HIP(hipMemsetAsync(a.mx, 0, (size_t)L.groups * a.cout_pad * sizeof(unsigned), s));
    hipLaunchKernelGGL(conv_repack_max_kernel, grid, dim3(RP_T), 0, s, a);
    XDET_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(conv_repack_kernel, grid, dim3(RP_T), 0, s, a, L.precision);
  XDET_LAUNCH_CHECK();
  return XDET_OK;
}

int ConvLayer::init(int kh_, int kw_, int cin_, int cout_, int stride_, int dil_, int pad_mode_, int pad_t_, int pad_l_,
                    const float* w_hwio, const float* scale, const float* shift, int relu_out_, int groups_) {
  XDET_REQUIRE(kh_ > 0 && kw_ > 0 && cin_ > 0 && cout_ > 0 && stride_ > 0 && dil_ > 0, "conv: bad geometry");
  XDET_REQUIRE(groups_ >= 1 && (groups_ == 1 || (kh_ == 1 && kw_ == 1 && stride_ == 1 && cin_ % 32 == 0)),
               "conv: grouped GEMMs are 1x1, stride 1, cin % 32 == 0");
  groups = groups_;
  XDET_REQUIRE(pad_mode_ >= 0 && pad_mode_ <= 2, "conv: pad_mode must be 0|1|2");
  XDET_REQUIRE(w_hwio != nullptr, "conv: kernel is NULL");
  kind = 1;
  kh = kh_; kw = kw_; cin = cin_; cout = cout_; stride = stride_; dil = dil_;
  pad_mode = pad_mode_; pad_t = pad_t_; pad_l = pad_l_; relu_out = relu_out_;
  small_cin = cin <= 4;
  cin_p = small_cin ? 4 : round_up(cin, 32);
  kp = round_up(kh * kw * cin_p, 32);
  n_tile = round_up(cout, 64) < round_up(cout, 128) ? 64 : 128;
  cout_pad = round_up(cout, n_tile);
  precision = g_default_precision;
  XDET_REQUIRE(groups == 1 || precision != PREC_F32, "conv: grouped GEMMs need a split-precision mode");
  XDET_HIP(hipGetDevice(&device));
  const size_t G = (size_t)groups, mat = (size_t)cout_pad * kp, rows = G * cout_pad;
  std::vector<float> sc(rows, 0.f), sh(rows, 0.f);          // the creation-time scale and the shift, zero in the padded rows
  for (size_t g = 0; g < G; ++g)
    for (int co = 0; co < cout; ++co) {
      sc[g * cout_pad + co] = scale ? scale[g * cout + co] : 1.f;
      sh[g * cout_pad + co] = shift ? shift[g * cout + co] : 0.f;
    }
  if (precision == PREC_F32) {
    XDET_TRY(d_wt.alloc(mat));
    XDET_TRY(d_scale.upload(sc.data(), rows));              // (no pre-scale: the repack leaves it alone)
  } else {
    const bool x3 = precision == PREC_F16X3;
    if (groups == 1) {      // [Cout_pad][Kp] copies: the register-staged kernel (strided / small-cin convs)
      XDET_TRY(d_wt_hi.alloc(mat));
      if (x3) XDET_TRY(d_wt_lo.alloc(mat));
    }
    if (!small_cin) {       // K-blocked copies: the LDS-DMA kernel
      XDET_TRY(d_zeros.alloc_zeroed(128));
      XDET_TRY(d_wt_hi_b.alloc(G * mat));
      if (x3) XDET_TRY(d_wt_lo_b.alloc(G * mat));
      if (x3 && kh == 1 && kw == 1 && stride == 1 && groups == 1) XDET_TRY(d_wt_x8_b.alloc(mat));   // a pointwise layer may be fed x8 planes
    }
    XDET_TRY(d_repack_scale0.upload(sc.data(), rows));
    XDET_TRY(d_repack_max.alloc(rows));
    XDET_TRY(d_scale.alloc(rows));
  }
  XDET_TRY(d_shift.upload(sh.data(), rows));
  DevMem<float> dense;                                      // (freed on return)
  XDET_TRY(dense.upload(w_hwio, G * kh * kw * cin * cout));
  XDET_TRY(launch_conv_repack(*this, dense, nullptr, nullptr));
  XDET_HIP(hipStreamSynchronize(nullptr));
  // the host copy of the epilogue scale (set_in_exp, the calibration) is the device's own
  in_scale.host.resize(rows);
  XDET_HIP(hipMemcpy(in_scale.host.data(), d_scale, rows * sizeof(float), hipMemcpyDeviceToHost));
  in_scale.dev = d_scale;
  return XDET_OK;
}

int ConvLayer::set_kernel_device(const float* k_hwio, const float* shift, hipStream_t s) {
  XDET_REQUIRE(k_hwio, "conv_set_kernel_device: kernel is NULL");
  XDET_REQUIRE(groups == 1, "conv_set_kernel_device: a grouped layer's block matrices are not a conv kernel");
  XDET_REQUIRE(in_exp == 0 && out_exp == 0 && pl_shift.host.empty(),
               "conv_set_kernel_device: the layer carries an activation or planes exponent or a planes affine (a calibrated or "
               "net-owned layer): its scale arrays are not the ones it was created with");
  host_stale = true;
  return launch_conv_repack(*this, k_hwio, shift, s);
}

// The refresh of a spectral conv (layers.h): G's row maxima, then exponent, split and scatter, both passes fed by
// spectral_weight_element instead of a dense matrix -- no buffer of the block matrices' size exists at any time.  What the call
// reads beyond the layer's operand buffers: the dense kernel, the twiddle table, and the row-maxima scratch G owns.
int SpectralConv::set_kernel_device(const float* w, const float* scale, const float* shift, hipStream_t s) {
  XDET_REQUIRE(w, "spectral_conv_set_kernel_device: kernel is NULL");
  XDET_REQUIRE(G.groups == NB && G.precision != PREC_F32 && G.cout_pad == 2 * cout_ld && G.kp == 2 * cin_ld && G.cout_pad % RP_CO == 0 &&
                   G.kp % RP_K == 0 && d_tw,
               "spectral_conv_set_kernel_device: unexpected padding");
  ConvRepack a = conv_repack_args(G, nullptr, nullptr);
  a.in_exp = G.in_exp;
  const SpectralSource src = {w, d_tw.get(), d_tw.get() + (size_t)NB * T, T, cin, cout, cin_ld, cout_ld};
  const dim3 grid((unsigned)(a.cout_pad / RP_CO), (unsigned)(a.kp / RP_K), (unsigned)NB);
  G.host_stale = true;
  XDET_HIP(hipMemsetAsync(a.mx, 0, (size_t)NB * a.cout_pad * sizeof(unsigned), s));
  hipLaunchKernelGGL(spectral_repack_max_kernel, grid, dim3(RP_T), 0, s, a, src);
  XDET_LAUNCH_CHECK();
  hipLaunchKernelGGL(spectral_repack_kernel, grid, dim3(RP_T), 0, s, a, src, G.precision);
  XDET_LAUNCH_CHECK();
  if (scale || shift) {
    hipLaunchKernelGGL(spectral_epilogue_kernel, dim3((unsigned)cdiv(cout, 256)), dim3(256), 0, s, scale, shift, cout, d_scale.get(),
                       d_shift.get());
    XDET_LAUNCH_CHECK();
  }
  return XDET_OK;
}

// tap i of the padded [9][ld] taps from the dense [3,3,C,1] kernel; e: the layer's activation exponent (set_out_exp: taps 2^-e)
__device__ __forceinline__ void depthwise_repack_tap(const float* __restrict__ k, float* __restrict__ w, int C, int ld, int e, int i) {
  if (i >= 9 * ld) return;
  const int t = i / ld, c = i - t * ld;
  const float v = c < C ? k[t * C + c] : 0.f;
  w[i] = e ? ldexpf(v, -e) : v;
}

__global__ __launch_bounds__(256) void depthwise_repack_kernel(const float* __restrict__ k, float* __restrict__ w, int C, int ld) {
  depthwise_repack_tap(k, w, C, ld, 0, blockIdx.x * 256 + threadIdx.x);
}

struct DepthwiseRepack {
  const float* k;
  float* w;
  int C, ld, out_exp, first_tile;
};

__global__ __launch_bounds__(256) void depthwise_repack_table_kernel(const DepthwiseRepack* __restrict__ slots, const int* __restrict__ tile_slot) {
  const DepthwiseRepack a = slots[tile_slot[blockIdx.x]];
  depthwise_repack_tap(a.k, a.w, a.C, a.ld, a.out_exp, ((int)blockIdx.x - a.first_tile) * 256 + threadIdx.x);
}

// The inference fold of a batch norm (Plan::fold_bn's operations in its order, each an f32 operation rounded on its own: the
// file is compiled with -ffp-contract=off, and the division and the square root are the correctly rounded ones -- hipcc's
// default for HIP device code, -fhip-fp32-correctly-rounded-divide-sqrt, which build.py does not turn off).
__global__ __launch_bounds__(256) void bn_fold_kernel(const float* __restrict__ gamma, const float* __restrict__ beta,
                                                      const float* __restrict__ mean, const float* __restrict__ var,
                                                      const float* __restrict__ bias, float eps, int C, float* __restrict__ scale,
                                                      float* __restrict__ shift) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  const float sc = gamma[c] / sqrtf(var[c] + eps);
  scale[c] = sc;
  shift[c] = (beta[c] - mean[c] * sc) + (bias ? bias[c] * sc : 0.f);    // (+ 0.f: a -0 shift becomes +0, as on the host)
}

// The table door's workspace: [conv slots][conv tile -> slot][depthwise slots][depthwise tile -> slot][row maxima], each part
// on a 256-byte boundary; the first four parts are filled on the host and uploaded in one copy.
struct RefreshLayout {
  size_t conv_slots = 0, conv_tiles = 0, dw_slots = 0, dw_tiles = 0, rows = 0;
  static size_t up(size_t b) { return (b + 255) / 256 * 256; }
  size_t off_conv_tiles() const { return up(conv_slots * sizeof(ConvRepack)); }
  size_t off_dw_slots() const { return off_conv_tiles() + up(conv_tiles * 4); }
  size_t off_dw_tiles() const { return off_dw_slots() + up(dw_slots * sizeof(DepthwiseRepack)); }
  size_t off_max() const { return off_dw_tiles() + up(dw_tiles * 4); }     // (= the bytes uploaded)
  size_t bytes() const { return off_max() + up(rows * sizeof(unsigned)); }
};

constexpr size_t RP_MAX_TILES = (size_t)1 << 24;

// why the table door cannot refresh this layer (NULL: it can)
static const char* refresh_refusal(const LayerBase* b) {
  if (b->kind == 3) return "layers_refresh: a spectral layer keeps its kernel as DFT-domain block matrices";
  if (b->kind == 2) return nullptr;
  if (b->kind != 1) return "layers_refresh: not a conv or depthwise layer";
  const ConvLayer* L = static_cast<const ConvLayer*>(b);
  if (L->groups != 1) return "layers_refresh: a grouped layer's block matrices are not a conv kernel";
  if (!L->pl_shift.host.empty()) return "layers_refresh: the layer's planes copy carries a folded batch norm (set_planes_bn)";
  if (L->cout_pad % RP_CO != 0 || L->kp % RP_K != 0) return "layers_refresh: unexpected padding";
  return nullptr;
}

// checks the table and measures it; errors before any GPU work
static int refresh_layout(const xdet_layer_refresh* slots, int n, RefreshLayout* lay) {
  XDET_REQUIRE(slots && n > 0, "layers_refresh: an empty slot table");
  std::vector<const void*> seen;
  seen.reserve((size_t)n);
  for (int i = 0; i < n; ++i) {
    const xdet_layer_refresh& h = slots[i];
    XDET_REQUIRE(h.layer && h.kernel, "layers_refresh: a slot with a NULL layer or kernel");
    seen.push_back(h.layer);
    const LayerBase* b = static_cast<const LayerBase*>(h.layer);
    const char* why = refresh_refusal(b);
    XDET_REQUIRE(!why, why);
    XDET_REQUIRE(b->device == static_cast<const LayerBase*>(slots[0].layer)->device, "layers_refresh: the layers live on different devices");
    if (b->kind == 2) {
      XDET_REQUIRE(!h.scale && !h.shift, "layers_refresh: a depthwise slot takes no scale and no shift");
      lay->dw_slots += 1;
      lay->dw_tiles += (size_t)cdiv(9 * static_cast<const DepthwiseLayer*>(b)->ld, 256);
    } else {
      const ConvLayer* L = static_cast<const ConvLayer*>(b);
      lay->conv_slots += 1;
      lay->conv_tiles += (size_t)(L->cout_pad / RP_CO) * (size_t)(L->kp / RP_K);
      if (L->precision != PREC_F32) lay->rows += (size_t)L->cout_pad;
    }
    XDET_REQUIRE(lay->conv_tiles <= RP_MAX_TILES && lay->dw_tiles <= RP_MAX_TILES, "layers_refresh: more than 2^24 tiles");
  }
  std::sort(seen.begin(), seen.end());
  XDET_REQUIRE(std::adjacent_find(seen.begin(), seen.end()) == seen.end(), "layers_refresh: a layer is listed twice");
  return XDET_OK;
}

int DepthwiseLayer::set_kernel_device(const float* k33c1, hipStream_t s) {
  XDET_REQUIRE(k33c1, "depthwise_set_kernel_device: kernel is NULL");
  XDET_REQUIRE(out_exp == 0, "depthwise_set_kernel_device: the layer's taps carry an activation pre-scale (a calibrated layer)");
  host_stale = true;
  hipLaunchKernelGGL(depthwise_repack_kernel, dim3((unsigned)cdiv(9 * ld, 256)), dim3(256), 0, s, k33c1, d_w.get(), C, ld);
  XDET_LAUNCH_CHECK();
  return XDET_OK;
}

}  // namespace xdet

using namespace xdet;

extern "C" {

int xdet_conv_set_kernel_device(void* layer, const float* kernel_hwio_dev, const float* shift_dev, void* stream) {
  LayerBase* b = static_cast<LayerBase*>(layer);
  XDET_REQUIRE(b && (b->kind == 1 || b->kind == 3), "not a conv layer");
  XDET_REQUIRE(b->kind == 1, "conv_set_kernel_device: a spectral layer keeps its kernel as DFT-domain block matrices");
  DeviceGuard guard(b->device);
  return static_cast<ConvLayer*>(b)->set_kernel_device(kernel_hwio_dev, shift_dev, reinterpret_cast<hipStream_t>(stream));
}

int xdet_spectral_conv_set_kernel_device(void* layer, const float* kernel_dev, const float* scale_dev, const float* shift_dev,
                                         void* stream) {
  LayerBase* b = static_cast<LayerBase*>(layer);
  XDET_REQUIRE(b && b->kind == 3, "spectral_conv_set_kernel_device: not a spectral conv layer");
  DeviceGuard guard(b->device);
  return static_cast<SpectralConv*>(b)->set_kernel_device(kernel_dev, scale_dev, shift_dev, reinterpret_cast<hipStream_t>(stream));
}

int xdet_depthwise_set_kernel_device(void* layer, const float* k33c1_dev, void* stream) {
  LayerBase* b = static_cast<LayerBase*>(layer);
  XDET_REQUIRE(b && b->kind == 2, "not a depthwise layer");
  DeviceGuard guard(b->device);
  return static_cast<DepthwiseLayer*>(b)->set_kernel_device(k33c1_dev, reinterpret_cast<hipStream_t>(stream));
}

int xdet_bn_fold(const float* gamma, const float* beta, const float* moving_mean, const float* moving_variance, const float* bias,
                 float eps, int C, float* scale_out, float* shift_out, void* stream) {
  XDET_REQUIRE(gamma && beta && moving_mean && moving_variance && scale_out && shift_out, "bn_fold: NULL argument");
  XDET_REQUIRE(C > 0, "bn_fold: C must be positive");
  hipLaunchKernelGGL(bn_fold_kernel, dim3((unsigned)cdiv(C, 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), gamma, beta,
                     moving_mean, moving_variance, bias, eps, C, scale_out, shift_out);
  XDET_LAUNCH_CHECK();
  return XDET_OK;
}

size_t xdet_layers_refresh_workspace_bytes(const xdet_layer_refresh* slots, int n) {
  RefreshLayout lay;
  return refresh_layout(slots, n, &lay) == XDET_OK ? lay.bytes() : 0;
}

int xdet_layers_refresh_device(const xdet_layer_refresh* slots, int n, void* workspace, void* stream) {
  RefreshLayout lay;
  XDET_TRY(refresh_layout(slots, n, &lay));
  XDET_REQUIRE(workspace, "layers_refresh: workspace is NULL");
  DeviceGuard guard(static_cast<const LayerBase*>(slots[0].layer)->device);
  char* base = static_cast<char*>(workspace);
  std::vector<char> host(lay.off_max(), 0);
  ConvRepack* cs = reinterpret_cast<ConvRepack*>(host.data());
  int* ct = reinterpret_cast<int*>(host.data() + lay.off_conv_tiles());
  DepthwiseRepack* ds = reinterpret_cast<DepthwiseRepack*>(host.data() + lay.off_dw_slots());
  int* dt = reinterpret_cast<int*>(host.data() + lay.off_dw_tiles());
  unsigned* d_max = reinterpret_cast<unsigned*>(base + lay.off_max());
  int ci = 0, di = 0, ctile = 0, dtile = 0;
  size_t row = 0;
  for (int i = 0; i < n; ++i) {
    const xdet_layer_refresh& h = slots[i];
    LayerBase* b = static_cast<LayerBase*>(h.layer);
    if (b->kind == 2) {
      DepthwiseLayer* D = static_cast<DepthwiseLayer*>(b);
      ds[di] = DepthwiseRepack{h.kernel, D->d_w.get(), D->C, D->ld, D->out_exp, dtile};
      const int tiles = cdiv(9 * D->ld, 256);
      for (int t = 0; t < tiles; ++t) dt[dtile + t] = di;
      dtile += tiles;
      ++di;
      D->host_stale = true;
      continue;
    }
    ConvLayer* L = static_cast<ConvLayer*>(b);
    ConvRepack a = conv_repack_args(*L, h.kernel, h.shift);
    a.scale_new = h.scale; a.in_exp = L->in_exp; a.first_tile = ctile;
    if (L->precision != PREC_F32) {         // the rows' maxima live in the workspace: one clear for the whole table
      a.mx = d_max + row;
      row += (size_t)L->cout_pad;
    }
    cs[ci] = a;
    const int tiles = a.tiles_x * (a.kp / RP_K);
    for (int t = 0; t < tiles; ++t) ct[ctile + t] = ci;
    ctile += tiles;
    ++ci;
    L->host_stale = true;
  }
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  // (a pageable source: the runtime has staged the tables when the call returns)
  XDET_HIP(hipMemcpyAsync(base, host.data(), host.size(), hipMemcpyHostToDevice, s));
  if (lay.rows) {
    XDET_HIP(hipMemsetAsync(d_max, 0, lay.rows * sizeof(unsigned), s));
    hipLaunchKernelGGL(conv_repack_max_table_kernel, dim3((unsigned)ctile), dim3(RP_T), 0, s,
                       reinterpret_cast<const ConvRepack*>(base), reinterpret_cast<const int*>(base + lay.off_conv_tiles()));
    XDET_LAUNCH_CHECK();
  }
  if (ctile) {
    hipLaunchKernelGGL(conv_repack_table_kernel, dim3((unsigned)ctile), dim3(RP_T), 0, s, reinterpret_cast<const ConvRepack*>(base),
                       reinterpret_cast<const int*>(base + lay.off_conv_tiles()));
    XDET_LAUNCH_CHECK();
  }
  if (dtile) {
    hipLaunchKernelGGL(depthwise_repack_table_kernel, dim3((unsigned)dtile), dim3(256), 0, s,
                       reinterpret_cast<const DepthwiseRepack*>(base + lay.off_dw_slots()),
                       reinterpret_cast<const int*>(base + lay.off_dw_tiles()));
    XDET_LAUNCH_CHECK();
  }
  return XDET_OK;
}

}  // extern "C"
