// The optimizer step of the training path (include/xdet.h): xdet_momentum_step, tf.train.MomentumOptimizer over a table of
// tensors in one launch, and the device-side refresh of a forward layer's operands from a dense f32 kernel in device memory,
// xdet_conv_set_kernel_device / xdet_depthwise_set_kernel_device -- what ConvLayer::init / DepthwiseLayer::init (layers.h)
// build on the host at creation, rebuilt in place, bit for bit.
//
// The momentum step is memory-bound: per element it reads var, grad and accum and writes var and accum, 20 bytes, and does
// four flops.  A workgroup of 256 threads owns one chunk of MS_CHUNK = 4096 consecutive elements of ONE slot (a slot's last
// chunk is short; chunks never cross a slot, so a chunk's base is 16 KiB from its slot's and 128-bit accesses depend on the
// slot's three pointers alone).  A thread owns four 4-element vectors, 1 KiB of a wave apart, so every access of a wave is
// one contiguous KiB; all twelve loads are issued before the first use.  The file is compiled with -ffp-contract=off: each
// of the update's operations is rounded on its own, as the NumPy statement (xdet.ops.host_momentum_step) rounds them.
//
// The repack makes two passes over the kernel [kh*kw][cin][cout] (a row of the transposed matrix, kh*kw*cin_p values of one
// output channel strided by cout, does not fit in LDS for the 15x1 convs): the largest |w| per output channel (an integer
// atomicMax on the bits of |w|: a maximum has no order to fix), then per 32 (K) x 64 (cout) tile the exponent, the
// pre-scale, the hi / lo split and the scatter into every buffer the layer owns.  The tile is read along cout (256 B per
// K index), transposed through LDS and written along K: 16 B per thread, 64 B per output row of d_wt_hi / d_wt_lo and one
// contiguous 4 KiB run of the K-blocked copies.  The number formats are layers.h's own converters, compiled for the device.
#include "layers.h"

namespace xdet {

constexpr int MS_T = 256;               // threads of a workgroup
constexpr int MS_CHUNK = 4096;          // elements of a chunk: four float4 per thread
constexpr int MS_MAX_SLOTS = 1 << 16;
constexpr int64_t MS_MAX_CHUNKS = 1 << 22;

struct MomentumSlotDev {                // a slot as the kernel reads it
  float* var;
  const float* grad;
  float* accum;
  long long n;
  int decay, first_chunk;
  int vec, pad;                         // vec: all three pointers are 16-byte aligned
};

// partial[chunk] = the chunk's share of sum v^2 (0 for a slot without decay), by the fixed tree of include/xdet.h
__global__ __launch_bounds__(MS_T) void momentum_step_kernel(const MomentumSlotDev* __restrict__ slots, const int* __restrict__ chunk_slot,
                                                             float lr, float momentum, float weight_decay, float* __restrict__ partial) {
  __shared__ float red[MS_T];
  const int tid = threadIdx.x;
  const MomentumSlotDev s = slots[chunk_slot[blockIdx.x]];
  const long long start = (long long)((int)blockIdx.x - s.first_chunk) * MS_CHUNK;
  const long long left = s.n - start;                       // > 0 by construction of the chunk table
  float v[4][4], g[4][4], a[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const long long j = (long long)(i * MS_T + tid) * 4;    // first element of the vector inside the chunk
    const long long at = start + j;
    if (s.vec && j + 4 <= left) {
      const float4 tv = *reinterpret_cast<const float4*>(s.var + at);
      const float4 tg = *reinterpret_cast<const float4*>(s.grad + at);
      const float4 ta = *reinterpret_cast<const float4*>(s.accum + at);
      v[i][0] = tv.x; v[i][1] = tv.y; v[i][2] = tv.z; v[i][3] = tv.w;
      g[i][0] = tg.x; g[i][1] = tg.y; g[i][2] = tg.z; g[i][3] = tg.w;
      a[i][0] = ta.x; a[i][1] = ta.y; a[i][2] = ta.z; a[i][3] = ta.w;
    } else {
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const bool in = j + c < left;
        v[i][c] = in ? s.var[at + c] : 0.f;
        g[i][c] = in ? s.grad[at + c] : 0.f;
        a[i][c] = in ? s.accum[at + c] : 0.f;
      }
    }
  }
  float t[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    // (an absent element is +0 and adds nothing)
    t[i] = (v[i][0] * v[i][0] + v[i][1] * v[i][1]) + (v[i][2] * v[i][2] + v[i][3] * v[i][3]);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const float gg = s.decay ? g[i][c] + weight_decay * v[i][c] : g[i][c];
      a[i][c] = momentum * a[i][c] + gg;
      v[i][c] = v[i][c] - lr * a[i][c];
    }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const long long j = (long long)(i * MS_T + tid) * 4;
    const long long at = start + j;
    if (s.vec && j + 4 <= left) {
      *reinterpret_cast<float4*>(s.var + at) = make_float4(v[i][0], v[i][1], v[i][2], v[i][3]);
      *reinterpret_cast<float4*>(s.accum + at) = make_float4(a[i][0], a[i][1], a[i][2], a[i][3]);
    } else {
#pragma unroll
      for (int c = 0; c < 4; ++c)
        if (j + c < left) {
          s.var[at + c] = v[i][c];
          s.accum[at + c] = a[i][c];
        }
    }
  }
  if (partial == nullptr) return;                          // (uniform over the grid)
  red[tid] = s.decay ? (t[0] + t[1]) + (t[2] + t[3]) : 0.f;
  __syncthreads();
#pragma unroll
  for (int w = MS_T / 2; w >= 1; w >>= 1) {
    if (tid < w) red[tid] += red[tid + w];
    __syncthreads();
  }
  if (tid == 0) partial[blockIdx.x] = red[0];
}

// one workgroup folds the chunk partials in place: P = the power of two at or above their count, and for w = P/2, P/4 .. 1
// partial[i] += partial[i + w] for every i < w with i + w below the count; *l2 = partial[0] / 2
__global__ __launch_bounds__(1024) void momentum_l2_kernel(float* partial, int n, int P, float* l2) {
  for (int w = P >> 1; w >= 1; w >>= 1) {
    for (int i = threadIdx.x; i < w; i += 1024)
      if (i + w < n) partial[i] += partial[i + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) *l2 = 0.5f * partial[0];
}

static size_t momentum_tables_bytes(int n_slots, int64_t n_chunks) {
  // [slots][chunk -> slot][chunk partials], each part on a 256-byte boundary
  auto up = [](size_t b) { return (b + 255) / 256 * 256; };
  return up((size_t)n_slots * sizeof(MomentumSlotDev)) + 2 * up((size_t)n_chunks * 4);
}

// ---- the repack of a conv layer's operands ---------------------------------------------------------------------------------

constexpr int RP_T = 256;
constexpr int RP_CO = 64, RP_K = 32;    // a tile: 64 output channels x one K block

struct ConvRepack {
  const float* w;                       // [taps][cin][cout] dense
  const float* shift;                   // [cout] or NULL
  const float* scale0;                  // [cout_pad]: the epilogue scale the layer was created with
  unsigned* mx;                         // [cout_pad]: bits of the largest |w| per output channel (pass 1)
  float* wt;                            // f32 mode: [cout_pad][kp]
  unsigned short *hi, *lo, *hi_b, *lo_b;
  unsigned char* x8_b;
  float *d_scale, *d_shift;
  int taps, cin, cout, cin_p, kp, cout_pad;
};

// the value of row co, column k of the padded [cout_pad][kp] matrix: k = tap * cin_p + ci
__device__ __forceinline__ float repack_source(const ConvRepack& a, int co, int k) {
  const int tap = k / a.cin_p, ci = k - tap * a.cin_p;
  return (tap < a.taps && ci < a.cin && co < a.cout) ? a.w[((size_t)tap * a.cin + ci) * a.cout + co] : 0.f;
}

__global__ __launch_bounds__(RP_T) void conv_repack_max_kernel(ConvRepack a) {
  const int co = blockIdx.x * RP_CO + (threadIdx.x & (RP_CO - 1));
  const int k0 = blockIdx.y * RP_K + (threadIdx.x / RP_CO) * (RP_K / 4);
  if (co >= a.cout) return;
  float m = 0.f;
#pragma unroll
  for (int i = 0; i < RP_K / 4; ++i) {
    const float f = fabsf(repack_source(a, co, k0 + i));
    m = m < f ? f : m;                  // (std::max's own comparison: a NaN never becomes the maximum)
  }
  if (m > 0.f) atomicMax(a.mx + co, __float_as_uint(m));
}

__global__ __launch_bounds__(RP_T) void conv_repack_kernel(ConvRepack a, int precision) {
  __shared__ float tile[RP_K][RP_CO + 1];
  const int tid = threadIdx.x;
  const int co0 = blockIdx.x * RP_CO, kb = blockIdx.y;
  {
    const int c = tid & (RP_CO - 1), kq = tid / RP_CO;
#pragma unroll
    for (int i = 0; i < RP_K / 4; ++i) tile[kq * (RP_K / 4) + i][c] = repack_source(a, co0 + c, kb * RP_K + kq * (RP_K / 4) + i);
  }
  __syncthreads();
  const int c = tid >> 2, q = tid & 3;                      // output row co0 + c, columns kb * 32 + q * 8 .. + 7
  const int co = co0 + c;
  const size_t row = (size_t)co * a.kp + (size_t)kb * RP_K + q * 8;
  if (precision == PREC_F32) {
    float4 lo4 = make_float4(tile[q * 8 + 0][c], tile[q * 8 + 1][c], tile[q * 8 + 2][c], tile[q * 8 + 3][c]);
    float4 hi4 = make_float4(tile[q * 8 + 4][c], tile[q * 8 + 5][c], tile[q * 8 + 6][c], tile[q * 8 + 7][c]);
    *reinterpret_cast<float4*>(a.wt + row) = lo4;
    *reinterpret_cast<float4*>(a.wt + row + 4) = hi4;
    if (kb == 0 && q == 0 && a.shift && co < a.cout) a.d_shift[co] = a.shift[co];
    return;
  }
  const float mx = __uint_as_float(a.mx[co]);
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
  const size_t blk = ((size_t)kb * a.cout_pad + co) * RP_K + q * 8;
  if (a.hi) *reinterpret_cast<uint4*>(a.hi + row) = H.v;
  if (a.lo) *reinterpret_cast<uint4*>(a.lo + row) = L.v;
  if (a.hi_b) *reinterpret_cast<uint4*>(a.hi_b + blk) = H.v;
  if (a.lo_b) *reinterpret_cast<uint4*>(a.lo_b + blk) = L.v;
  if (a.x8_b) {
    unsigned char* rec = a.x8_b + ((size_t)kb * a.cout_pad + co) * 64 + q * 8;
    *reinterpret_cast<uint2*>(rec) = X_lo.v;
    *reinterpret_cast<uint2*>(rec + 32) = X_hi.v;
  }
  if (kb == 0 && q == 0) {
    a.d_scale[co] = ldexpf(a.scale0[co], -sh_k);
    if (a.shift && co < a.cout) a.d_shift[co] = a.shift[co];
  }
}

int launch_conv_repack(const ConvRepack& a, int precision, hipStream_t s) {
  const dim3 grid((unsigned)(a.cout_pad / RP_CO), (unsigned)(a.kp / RP_K));
  if (precision != PREC_F32) {
    XDET_HIP(hipMemsetAsync(a.mx, 0, (size_t)a.cout_pad * sizeof(unsigned), s));
    hipLaunchKernelGGL(conv_repack_max_kernel, grid, dim3(RP_T), 0, s, a);
    XDET_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(conv_repack_kernel, grid, dim3(RP_T), 0, s, a, precision);
  XDET_LAUNCH_CHECK();
  return XDET_OK;
}

int ConvLayer::set_kernel_device(const float* k_hwio, const float* shift, hipStream_t s) {
  XDET_REQUIRE(k_hwio, "conv_set_kernel_device: kernel is NULL");
  XDET_REQUIRE(groups == 1, "conv_set_kernel_device: a grouped layer's block matrices are not a conv kernel");
  XDET_REQUIRE(in_exp == 0 && out_exp == 0 && pl_shift.host.empty(),
               "conv_set_kernel_device: the layer carries an activation or planes exponent or a planes affine (a calibrated or "
               "net-owned layer): its scale arrays are not the ones it was created with");
  XDET_REQUIRE(cout_pad % RP_CO == 0 && kp % RP_K == 0, "conv_set_kernel_device: unexpected padding");
  if (precision != PREC_F32 && !d_repack_scale0) {
    XDET_TRY(d_repack_scale0.upload(scale0.data(), scale0.size()));
    XDET_TRY(d_repack_max.alloc((size_t)cout_pad));
  }
  ConvRepack a;
  a.w = k_hwio; a.shift = shift; a.scale0 = d_repack_scale0; a.mx = d_repack_max;
  a.wt = d_wt; a.hi = d_wt_hi; a.lo = d_wt_lo; a.hi_b = d_wt_hi_b; a.lo_b = d_wt_lo_b;
  a.x8_b = reinterpret_cast<unsigned char*>(d_wt_x8_b.get());
  a.d_scale = d_scale; a.d_shift = d_shift;
  a.taps = kh * kw; a.cin = cin; a.cout = cout; a.cin_p = cin_p; a.kp = kp; a.cout_pad = cout_pad;
  host_stale = true;
  return launch_conv_repack(a, precision, s);
}

__global__ __launch_bounds__(256) void depthwise_repack_kernel(const float* __restrict__ k, float* __restrict__ w, int C, int ld) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= 9 * ld) return;
  const int t = i / ld, c = i - t * ld;
  w[i] = c < C ? k[t * C + c] : 0.f;
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

size_t xdet_momentum_step_workspace_bytes(const xdet_momentum_slot* slots, int n_slots) {
  if (!slots || n_slots <= 0 || n_slots > MS_MAX_SLOTS) return 0;
  int64_t chunks = 0;
  for (int i = 0; i < n_slots; ++i) {
    if (slots[i].n <= 0) return 0;
    chunks += cdiv(slots[i].n, MS_CHUNK);
    if (chunks > MS_MAX_CHUNKS) return 0;
  }
  return momentum_tables_bytes(n_slots, chunks);
}

int xdet_momentum_step(const xdet_momentum_slot* slots, int n_slots, float lr, float momentum, float weight_decay, float* l2,
                       void* workspace, void* stream) {
  XDET_REQUIRE(slots && n_slots > 0, "momentum_step: an empty slot table");
  XDET_REQUIRE(n_slots <= MS_MAX_SLOTS, "momentum_step: at most 65536 slots");
  XDET_REQUIRE(workspace, "momentum_step: workspace is NULL");
  std::vector<MomentumSlotDev> dev((size_t)n_slots);
  int64_t chunks = 0;
  for (int i = 0; i < n_slots; ++i) {
    const xdet_momentum_slot& h = slots[i];
    XDET_REQUIRE(h.var && h.grad && h.accum, "momentum_step: a slot with a NULL var, grad or accum");
    XDET_REQUIRE(h.n > 0, "momentum_step: a slot with n <= 0");
    MomentumSlotDev& d = dev[(size_t)i];
    d.var = h.var; d.grad = h.grad; d.accum = h.accum; d.n = h.n; d.decay = h.decay ? 1 : 0;
    d.first_chunk = (int)chunks;
    d.vec = ((reinterpret_cast<uintptr_t>(h.var) | reinterpret_cast<uintptr_t>(h.grad) | reinterpret_cast<uintptr_t>(h.accum)) & 15) == 0;
    d.pad = 0;
    chunks += cdiv(h.n, MS_CHUNK);
    XDET_REQUIRE(chunks <= MS_MAX_CHUNKS, "momentum_step: more than 2^22 chunks of 4096 elements");
  }
  std::vector<int> chunk_slot((size_t)chunks);
  for (int i = 0; i < n_slots; ++i) {
    const int64_t end = i + 1 < n_slots ? dev[(size_t)i + 1].first_chunk : chunks;
    for (int64_t c = dev[(size_t)i].first_chunk; c < end; ++c) chunk_slot[(size_t)c] = i;
  }
  auto up = [](size_t b) { return (b + 255) / 256 * 256; };
  char* base = static_cast<char*>(workspace);
  MomentumSlotDev* d_slots = reinterpret_cast<MomentumSlotDev*>(base);
  int* d_chunk = reinterpret_cast<int*>(base + up(dev.size() * sizeof(MomentumSlotDev)));
  float* d_partial = reinterpret_cast<float*>(reinterpret_cast<char*>(d_chunk) + up((size_t)chunks * 4));
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  // (pageable sources: the runtime has staged both tables when the calls return)
  XDET_HIP(hipMemcpyAsync(d_slots, dev.data(), dev.size() * sizeof(MomentumSlotDev), hipMemcpyHostToDevice, s));
  XDET_HIP(hipMemcpyAsync(d_chunk, chunk_slot.data(), (size_t)chunks * 4, hipMemcpyHostToDevice, s));
  hipLaunchKernelGGL(momentum_step_kernel, dim3((unsigned)chunks), dim3(MS_T), 0, s, d_slots, d_chunk, lr, momentum, weight_decay,
                     l2 ? d_partial : nullptr);
  XDET_LAUNCH_CHECK();
  if (l2) {
    int P = 1;
    while (P < chunks) P <<= 1;
    hipLaunchKernelGGL(momentum_l2_kernel, dim3(1), dim3(1024), 0, s, d_partial, (int)chunks, P, l2);
    XDET_LAUNCH_CHECK();
  }
  return XDET_OK;
}

int xdet_conv_set_kernel_device(void* layer, const float* kernel_hwio_dev, const float* shift_dev, void* stream) {
  LayerBase* b = static_cast<LayerBase*>(layer);
  XDET_REQUIRE(b && (b->kind == 1 || b->kind == 3), "not a conv layer");
  XDET_REQUIRE(b->kind == 1, "conv_set_kernel_device: a spectral layer keeps its kernel as DFT-domain block matrices");
  DeviceGuard guard(b->device);
  return static_cast<ConvLayer*>(b)->set_kernel_device(kernel_hwio_dev, shift_dev, reinterpret_cast<hipStream_t>(stream));
}

int xdet_depthwise_set_kernel_device(void* layer, const float* k33c1_dev, void* stream) {
  LayerBase* b = static_cast<LayerBase*>(layer);
  XDET_REQUIRE(b && b->kind == 2, "not a depthwise layer");
  DeviceGuard guard(b->device);
  return static_cast<DepthwiseLayer*>(b)->set_kernel_device(k33c1_dev, reinterpret_cast<hipStream_t>(stream));
}

}  // extern "C"
