// The optimizer step of the training path (include/xdet.h): xdet_momentum_step, tf.train.MomentumOptimizer over a table of
// tensors in one launch; xdet_grad_stats, the pass over the same table's gradients that decides on the device whether the
// step may happen; and xdet_momentum_step_guarded, the step that obeys it.  (The refresh of the forward layers from the
// stepped weights is conv_repack.hip.)
//
// The momentum step is memory-bound: per element it reads var, grad and accum and writes var and accum, 20 bytes, and does
// four flops.  A workgroup of 256 threads owns one chunk of MS_CHUNK = 4096 consecutive elements of ONE slot (a slot's last
// chunk is short; chunks never cross a slot, so a chunk's base is 16 KiB from its slot's and 128-bit accesses depend on the
// slot's three pointers alone).  A thread owns four 4-element vectors, 1 KiB of a wave apart, so every access of a wave is
// one contiguous KiB; all twelve loads are issued before the first use.  The file is compiled with -ffp-contract=off: each
// of the update's operations is rounded on its own, as the NumPy statement (xdet.ops.host_momentum_step) rounds them.
//
// The gradient statistics read grad alone, 4 bytes per element, in the same chunks and through the same two access widths
// (decided by grad's own alignment); all four loads of a thread are issued before the first use.  The sum of squares goes
// down the tree the step uses for v^2; the count of non-finite elements is an integer and needs no order.  Nothing here
// uses a float atomic, a fence or a workgroup that waits for another: the second launch is the barrier.
#include <climits>
#include <cmath>

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

// the 16-byte record xdet_grad_stats writes (include/xdet.h)
struct GradStatsRecord {
  float grad_sq;
  int nonfinite, first_bad_slot, zero;
};

// partial[chunk] = the chunk's share of sum v^2 (0 for a slot without decay), by the fixed tree of include/xdet.h.
// CLIP: the clipped form -- the gradients are scaled by clip_norm / max(sqrt(stats->grad_sq), clip_norm), both operations
// correctly rounded (sqrtf and `/` are the IEEE ones here: the file is built with -fhip-fp32-correctly-rounded-divide-sqrt),
// and `skip` is the record's count where the caller asked for the guard; workgroup 0 leaves the scale in *scale_out.
// !CLIP is the kernel as it was: stats, clip_norm and scale_out are not looked at.
template <bool CLIP>
__global__ __launch_bounds__(MS_T) void momentum_step_kernel(const MomentumSlotDev* __restrict__ slots, const int* __restrict__ chunk_slot,
                                                             float lr, float momentum, float weight_decay, float* __restrict__ partial,
                                                             const int* __restrict__ skip, const GradStatsRecord* __restrict__ stats,
                                                             float clip_norm, float* __restrict__ scale_out) {
  __shared__ float red[MS_T];
  const int tid = threadIdx.x;
  const bool hold = skip != nullptr && *skip != 0;          // (one word, the same for every thread of the grid)
  float scale = 1.f;
  if (CLIP) {
    const float norm = sqrtf(stats->grad_sq);               // (one word again; a NaN norm fails the comparison and stays)
    scale = clip_norm / (norm <= clip_norm ? clip_norm : norm);
    if (scale_out != nullptr && blockIdx.x == 0 && tid == 0) *scale_out = scale;
  }
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
      const float gs = CLIP ? g[i][c] * scale : g[i][c];
      const float gg = s.decay ? gs + weight_decay * v[i][c] : gs;
      a[i][c] = momentum * a[i][c] + gg;
      v[i][c] = v[i][c] - lr * a[i][c];
    }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if (hold) break;                                        // a guarded step that was told to skip stores nothing
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

__device__ __forceinline__ int non_finite(float x) { return (__float_as_uint(x) & 0x7f800000u) == 0x7f800000u ? 1 : 0; }
// (a count is at most 2^34: it stays at INT_MAX rather than wrap to a value that could read as zero)
__device__ __forceinline__ int add_sat(int a, int b) { return (int)min((unsigned)a + (unsigned)b, (unsigned)INT_MAX); }

// per chunk: sq[chunk] = sum g^2 by the tree momentum_step_kernel uses for v^2, cnt[chunk] = the number of non-finite
// elements, bad[chunk] = the chunk's slot if that number is not zero, else INT_MAX.  An element beyond the slot's end is absent
__global__ __launch_bounds__(MS_T) void grad_stats_kernel(const MomentumSlotDev* __restrict__ slots, const int* __restrict__ chunk_slot,
                                                          float* __restrict__ sq, int* __restrict__ cnt, int* __restrict__ bad) {
  __shared__ float red[MS_T];
  __shared__ int num[MS_T];
  const int tid = threadIdx.x;
  const int slot = chunk_slot[blockIdx.x];
  const MomentumSlotDev s = slots[slot];
  const long long start = (long long)((int)blockIdx.x - s.first_chunk) * MS_CHUNK;
  const long long left = s.n - start;                       // > 0 by construction of the chunk table
  float g[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const long long j = (long long)(i * MS_T + tid) * 4;
    const long long at = start + j;
    if (s.vec && j + 4 <= left) {
      const float4 tg = *reinterpret_cast<const float4*>(s.grad + at);
      g[i][0] = tg.x; g[i][1] = tg.y; g[i][2] = tg.z; g[i][3] = tg.w;
    } else {
#pragma unroll
      for (int c = 0; c < 4; ++c) g[i][c] = j + c < left ? s.grad[at + c] : 0.f;
    }
  }
  float t[4];
  int k = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    t[i] = (g[i][0] * g[i][0] + g[i][1] * g[i][1]) + (g[i][2] * g[i][2] + g[i][3] * g[i][3]);
#pragma unroll
    for (int c = 0; c < 4; ++c) k += non_finite(g[i][c]);
  }
  red[tid] = (t[0] + t[1]) + (t[2] + t[3]);
  num[tid] = k;
  __syncthreads();
#pragma unroll
  for (int w = MS_T / 2; w >= 1; w >>= 1) {
    if (tid < w) {
      red[tid] += red[tid + w];
      num[tid] += num[tid + w];                             // (at most 4096: no saturation inside a chunk)
    }
    __syncthreads();
  }
  if (tid == 0) {
    sq[blockIdx.x] = red[0];
    cnt[blockIdx.x] = num[0];
    bad[blockIdx.x] = num[0] ? slot : INT_MAX;
  }
}

// one workgroup folds the three partial arrays in place in momentum_l2_kernel's order -- sum, sum, min -- and writes the record
__global__ __launch_bounds__(1024) void grad_stats_fold_kernel(float* sq, int* cnt, int* bad, int n, int P, GradStatsRecord* out) {
  for (int w = P >> 1; w >= 1; w >>= 1) {
    for (int i = threadIdx.x; i < w; i += 1024)
      if (i + w < n) {
        sq[i] += sq[i + w];
        cnt[i] = add_sat(cnt[i], cnt[i + w]);
        bad[i] = min(bad[i], bad[i + w]);
      }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    GradStatsRecord r;
    r.grad_sq = sq[0];
    r.nonfinite = cnt[0];
    r.first_bad_slot = bad[0] == INT_MAX ? -1 : bad[0];
    r.zero = 0;
    *out = r;
  }
}

static size_t up256(size_t b) { return (b + 255) / 256 * 256; }

static size_t momentum_tables_bytes(int n_slots, int64_t n_chunks, int partials = 1) {
  // [slots][chunk -> slot][chunk partials] (the statistics: three arrays of partials), each part on a 256-byte boundary
  return up256((size_t)n_slots * sizeof(MomentumSlotDev)) + (size_t)(1 + partials) * up256((size_t)n_chunks * 4);
}

// the number of chunks of a table the doors accept, 0 for one they refuse
static int64_t table_chunks(const xdet_momentum_slot* slots, int n_slots) {
  if (!slots || n_slots <= 0 || n_slots > MS_MAX_SLOTS) return 0;
  int64_t chunks = 0;
  for (int i = 0; i < n_slots; ++i) {
    if (slots[i].n <= 0) return 0;
    chunks += cdiv(slots[i].n, MS_CHUNK);
    if (chunks > MS_MAX_CHUNKS) return 0;
  }
  return chunks;
}

// The slot and chunk tables of a host table, uploaded to the front of `workspace` on `s`; grad_only: the statistics' door,
// which reads grad alone (var and accum are not looked at, and grad's alignment alone decides the access width).
// -> d_slots, d_chunk, the first byte behind both tables and the number of chunks
static int upload_tables(const char* who, const xdet_momentum_slot* slots, int n_slots, bool grad_only, void* workspace, hipStream_t s,
                         MomentumSlotDev** d_slots, int** d_chunk, char** behind, int64_t* n_chunks) {
  const std::string w(who);
  XDET_REQUIRE(slots && n_slots > 0, w + ": an empty slot table");
  XDET_REQUIRE(n_slots <= MS_MAX_SLOTS, w + ": at most 65536 slots");
  XDET_REQUIRE(workspace, w + ": workspace is NULL");
  std::vector<MomentumSlotDev> dev((size_t)n_slots);
  int64_t chunks = 0;
  for (int i = 0; i < n_slots; ++i) {
    const xdet_momentum_slot& h = slots[i];
    if (grad_only) XDET_REQUIRE(h.grad, w + ": a slot with a NULL grad");
    else XDET_REQUIRE(h.var && h.grad && h.accum, w + ": a slot with a NULL var, grad or accum");
    XDET_REQUIRE(h.n > 0, w + ": a slot with n <= 0");
    MomentumSlotDev& d = dev[(size_t)i];
    d.var = h.var; d.grad = h.grad; d.accum = h.accum; d.n = h.n; d.decay = h.decay ? 1 : 0;
    d.first_chunk = (int)chunks;
    const uintptr_t bits = grad_only ? reinterpret_cast<uintptr_t>(h.grad)
                                     : reinterpret_cast<uintptr_t>(h.var) | reinterpret_cast<uintptr_t>(h.grad) | reinterpret_cast<uintptr_t>(h.accum);
    d.vec = (bits & 15) == 0;
    d.pad = 0;
    chunks += cdiv(h.n, MS_CHUNK);
    XDET_REQUIRE(chunks <= MS_MAX_CHUNKS, w + ": more than 2^22 chunks of 4096 elements");
  }
  std::vector<int> chunk_slot((size_t)chunks);
  for (int i = 0; i < n_slots; ++i) {
    const int64_t end = i + 1 < n_slots ? dev[(size_t)i + 1].first_chunk : chunks;
    for (int64_t c = dev[(size_t)i].first_chunk; c < end; ++c) chunk_slot[(size_t)c] = i;
  }
  char* base = static_cast<char*>(workspace);
  *d_slots = reinterpret_cast<MomentumSlotDev*>(base);
  *d_chunk = reinterpret_cast<int*>(base + up256(dev.size() * sizeof(MomentumSlotDev)));
  *behind = reinterpret_cast<char*>(*d_chunk) + up256((size_t)chunks * 4);
  *n_chunks = chunks;
  // (pageable sources: the runtime has staged both tables when the calls return)
  XDET_HIP(hipMemcpyAsync(*d_slots, dev.data(), dev.size() * sizeof(MomentumSlotDev), hipMemcpyHostToDevice, s));
  XDET_HIP(hipMemcpyAsync(*d_chunk, chunk_slot.data(), (size_t)chunks * 4, hipMemcpyHostToDevice, s));
  return XDET_OK;
}

// the second launch of a step that computes l2: one workgroup over the chunk partials
static int launch_l2_fold(float* d_partial, int64_t chunks, float* l2, hipStream_t s) {
  int P = 1;
  while (P < chunks) P <<= 1;
  hipLaunchKernelGGL(momentum_l2_kernel, dim3(1), dim3(1024), 0, s, d_partial, (int)chunks, P, l2);
  XDET_LAUNCH_CHECK();
  return XDET_OK;
}

}  // namespace xdet

using namespace xdet;

extern "C" {

size_t xdet_momentum_step_workspace_bytes(const xdet_momentum_slot* slots, int n_slots) {
  const int64_t chunks = table_chunks(slots, n_slots);
  return chunks ? momentum_tables_bytes(n_slots, chunks) : 0;
}

int xdet_momentum_step_guarded(const xdet_momentum_slot* slots, int n_slots, float lr, float momentum, float weight_decay, float* l2,
                               const int32_t* skip_dev, void* workspace, void* stream) {
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  MomentumSlotDev* d_slots;
  int* d_chunk;
  char* behind;
  int64_t chunks;
  XDET_TRY(upload_tables("momentum_step", slots, n_slots, false, workspace, s, &d_slots, &d_chunk, &behind, &chunks));
  float* d_partial = reinterpret_cast<float*>(behind);
  hipLaunchKernelGGL(momentum_step_kernel<false>, dim3((unsigned)chunks), dim3(MS_T), 0, s, d_slots, d_chunk, lr, momentum, weight_decay,
                     l2 ? d_partial : nullptr, skip_dev, (const GradStatsRecord*)nullptr, 0.f, (float*)nullptr);
  XDET_LAUNCH_CHECK();
  if (l2) XDET_TRY(launch_l2_fold(d_partial, chunks, l2, s));
  return XDET_OK;
}

int xdet_momentum_step_clipped(const xdet_momentum_slot* slots, int n_slots, float lr, float momentum, float weight_decay, float* l2,
                               const void* stats_dev, float clip_norm, int guard, float* scale_out, void* workspace, void* stream) {
  XDET_REQUIRE(std::isfinite(clip_norm) && clip_norm > 0.f, "momentum_step_clipped: clip_norm must be finite and positive");
  XDET_REQUIRE(stats_dev, "momentum_step_clipped: stats_dev is NULL");
  XDET_REQUIRE((reinterpret_cast<uintptr_t>(stats_dev) & 3) == 0, "momentum_step_clipped: stats_dev must be 4-byte aligned");
  XDET_REQUIRE((reinterpret_cast<uintptr_t>(scale_out) & 3) == 0, "momentum_step_clipped: scale_out must be 4-byte aligned");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  MomentumSlotDev* d_slots;
  int* d_chunk;
  char* behind;
  int64_t chunks;
  XDET_TRY(upload_tables("momentum_step", slots, n_slots, false, workspace, s, &d_slots, &d_chunk, &behind, &chunks));
  float* d_partial = reinterpret_cast<float*>(behind);
  const GradStatsRecord* rec = static_cast<const GradStatsRecord*>(stats_dev);
  hipLaunchKernelGGL(momentum_step_kernel<true>, dim3((unsigned)chunks), dim3(MS_T), 0, s, d_slots, d_chunk, lr, momentum, weight_decay,
                     l2 ? d_partial : nullptr, guard ? &rec->nonfinite : (const int*)nullptr, rec, clip_norm, scale_out);
  XDET_LAUNCH_CHECK();
  if (l2) XDET_TRY(launch_l2_fold(d_partial, chunks, l2, s));
  return XDET_OK;
}

int xdet_momentum_step(const xdet_momentum_slot* slots, int n_slots, float lr, float momentum, float weight_decay, float* l2,
                       void* workspace, void* stream) {
  return xdet_momentum_step_guarded(slots, n_slots, lr, momentum, weight_decay, l2, nullptr, workspace, stream);
}

size_t xdet_grad_stats_workspace_bytes(const xdet_momentum_slot* slots, int n_slots) {
  const int64_t chunks = table_chunks(slots, n_slots);
  return chunks ? momentum_tables_bytes(n_slots, chunks, 3) : 0;
}

int xdet_grad_stats(const xdet_momentum_slot* slots, int n_slots, void* stats_dev, void* workspace, void* stream) {
  XDET_REQUIRE(stats_dev, "grad_stats: stats_dev is NULL");
  XDET_REQUIRE((reinterpret_cast<uintptr_t>(stats_dev) & 3) == 0, "grad_stats: stats_dev must be 4-byte aligned");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  MomentumSlotDev* d_slots;
  int* d_chunk;
  char* behind;
  int64_t chunks;
  XDET_TRY(upload_tables("grad_stats", slots, n_slots, true, workspace, s, &d_slots, &d_chunk, &behind, &chunks));
  const size_t part = up256((size_t)chunks * 4);
  float* d_sq = reinterpret_cast<float*>(behind);
  int* d_cnt = reinterpret_cast<int*>(behind + part);
  int* d_bad = reinterpret_cast<int*>(behind + 2 * part);
  hipLaunchKernelGGL(grad_stats_kernel, dim3((unsigned)chunks), dim3(MS_T), 0, s, d_slots, d_chunk, d_sq, d_cnt, d_bad);
  XDET_LAUNCH_CHECK();
  int P = 1;
  while (P < chunks) P <<= 1;
  hipLaunchKernelGGL(grad_stats_fold_kernel, dim3(1), dim3(1024), 0, s, d_sq, d_cnt, d_bad, (int)chunks, P,
                     static_cast<GradStatsRecord*>(stats_dev));
  XDET_LAUNCH_CHECK();
  return XDET_OK;
}

}  // extern "C"
