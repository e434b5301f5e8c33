// The optimizer step of the training path (include/xdet.h): xdet_momentum_step, tf.train.MomentumOptimizer over a table of
// tensors in one launch.  (The refresh of the forward layers from the stepped weights is conv_repack.hip.)
//
// The momentum step is memory-bound: per element it reads var, grad and accum and writes var and accum, 20 bytes, and does
// four flops.  A workgroup of 256 threads owns one chunk of MS_CHUNK = 4096 consecutive elements of ONE slot (a slot's last
// chunk is short; chunks never cross a slot, so a chunk's base is 16 KiB from its slot's and 128-bit accesses depend on the
// slot's three pointers alone).  A thread owns four 4-element vectors, 1 KiB of a wave apart, so every access of a wave is
// one contiguous KiB; all twelve loads are issued before the first use.  The file is compiled with -ffp-contract=off: each
// of the update's operations is rounded on its own, as the NumPy statement (xdet.ops.host_momentum_step) rounds them.
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

}  // extern "C"
