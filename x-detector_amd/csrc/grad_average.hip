// The gradient average of data-parallel training (include/xdet.h): xdet_grad_pack and xdet_grad_reduce_ranks, the two passes
// that xdet_comm_average_gradients (comm.hip) runs on either side of its all-gather.
//
// Both are streaming, memory-bound passes over one chunk of the flat element space: the pack reads the slots and writes the
// chunk (8 bytes per element), the reduce reads `world` slabs and writes the slots (4 * (world + 1) bytes per element).  A
// workgroup of 256 threads owns one run of GA_RUN = 4096 consecutive flat elements of the chunk; a thread owns four 4-element
// vectors, 1 KiB of a wave apart, so every access of a wave is one contiguous KiB, and all of a thread's loads of one slab are
// issued before the first use.  A vector never straddles two slots (slots start on multiples of 4 flat elements), so the slot
// lookup is per vector: the host uploads, per run, the slot that holds the run's first element; the slot of a vector lies
// between its run's entry and the next run's, which is the same slot for all but the runs a slot boundary falls into.
// The reduce adds the slabs in rank order, r = 1 .. world-1 onto slab 0, in registers, divides once and stores once: no
// atomics, no LDS.  The file is compiled with -ffp-contract=off; the division is the correctly rounded f32 division.
#include "grad_average.h"

namespace xdet {

constexpr int GA_T = 256;                 // threads of a workgroup
constexpr int GA_RUN = 4096;              // flat elements of a run: four float4 per thread
constexpr int GA_MAX_SLOTS = 1 << 16;
constexpr int64_t GA_MAX_RUNS = 1 << 22;
constexpr int64_t GA_MAX_CHUNK = 1 << 24; // elements: 64 MiB of f32, the unit one collective moves per rank
constexpr int64_t GA_MAX_N = (int64_t)1 << 35;

struct GradSlotDev {                      // a slot as the kernels read it
  float* grad;
  long long off;                          // its first flat element (a multiple of 4)
  long long n;
  int vec, pad;                           // vec: the pointer is 16-byte aligned
};

// the slot that holds flat element f: the last one in [lo, hi] that starts at or before f
__device__ __forceinline__ GradSlotDev grad_slot_of(const GradSlotDev* __restrict__ slots, int lo, int hi, long long f) {
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (slots[mid].off <= f) lo = mid;
    else hi = mid - 1;
  }
  return slots[lo];
}

// out[p] = flat element start + p for p < len (len a multiple of 4): the slot's element, or +0 in the padding behind a slot
__global__ __launch_bounds__(GA_T) void grad_pack_kernel(const GradSlotDev* __restrict__ slots, const int* __restrict__ runs,
                                                         long long start, int len, float* __restrict__ out) {
  const int lo = runs[blockIdx.x], hi = runs[blockIdx.x + 1];
  float4 v[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int p = (int)blockIdx.x * GA_RUN + (i * GA_T + (int)threadIdx.x) * 4;
    if (p >= len) continue;
    const GradSlotDev s = grad_slot_of(slots, lo, hi, start + p);
    const long long j = start + p - s.off;                  // < s.n: a slot's padding is shorter than a vector
    if (s.vec && j + 4 <= s.n) {
      v[i] = *reinterpret_cast<const float4*>(s.grad + j);
    } else {
      v[i].x = s.grad[j];
      v[i].y = j + 1 < s.n ? s.grad[j + 1] : 0.f;
      v[i].z = j + 2 < s.n ? s.grad[j + 2] : 0.f;
      v[i].w = j + 3 < s.n ? s.grad[j + 3] : 0.f;
    }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int p = (int)blockIdx.x * GA_RUN + (i * GA_T + (int)threadIdx.x) * 4;
    if (p < len) *reinterpret_cast<float4*>(out + p) = v[i];
  }
}

// the slots' elements of the chunk = (((g[0] + g[1]) + g[2]) + ...) / world over the slabs g[r] = gathered + r * len
__global__ __launch_bounds__(GA_T) void grad_reduce_ranks_kernel(const GradSlotDev* __restrict__ slots, const int* __restrict__ runs,
                                                                 long long start, int len, const float* __restrict__ gathered,
                                                                 int world) {
  const int lo = runs[blockIdx.x], hi = runs[blockIdx.x + 1];
  int p[4];
  float4 acc[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    p[i] = (int)blockIdx.x * GA_RUN + (i * GA_T + (int)threadIdx.x) * 4;
    if (p[i] < len) acc[i] = *reinterpret_cast<const float4*>(gathered + p[i]);
  }
  for (int r = 1; r < world; ++r) {
    const float* __restrict__ g = gathered + (size_t)r * (size_t)len;
    float4 t[4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (p[i] < len) t[i] = *reinterpret_cast<const float4*>(g + p[i]);
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (p[i] < len) {
        acc[i].x = acc[i].x + t[i].x; acc[i].y = acc[i].y + t[i].y;
        acc[i].z = acc[i].z + t[i].z; acc[i].w = acc[i].w + t[i].w;
      }
  }
  const float w = (float)world;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if (p[i] >= len) continue;
    const GradSlotDev s = grad_slot_of(slots, lo, hi, start + p[i]);
    const long long j = start + p[i] - s.off;
    const float4 o = make_float4(acc[i].x / w, acc[i].y / w, acc[i].z / w, acc[i].w / w);
    if (s.vec && j + 4 <= s.n) {
      *reinterpret_cast<float4*>(s.grad + j) = o;
    } else {
      s.grad[j] = o.x;
      if (j + 1 < s.n) s.grad[j + 1] = o.y;
      if (j + 2 < s.n) s.grad[j + 2] = o.z;
      if (j + 3 < s.n) s.grad[j + 3] = o.w;
    }
  }
}

static size_t ga_up(size_t b) { return (b + 255) / 256 * 256; }

int grad_plan_check(const xdet_grad_slot* slots, int n_slots, int64_t chunk_elems, int world, const char* who, GradPlan* plan,
                    size_t* bytes) {
  const std::string w(who);
  XDET_REQUIRE(slots && n_slots > 0, w + ": an empty slot table");
  XDET_REQUIRE(n_slots <= GA_MAX_SLOTS, w + ": at most 65536 slots");
  XDET_REQUIRE(chunk_elems > 0 && chunk_elems % 1024 == 0 && chunk_elems <= GA_MAX_CHUNK,
               w + ": chunk_elems must be a positive multiple of 1024, at most 2^24 (64 MiB of f32)");
  XDET_REQUIRE(world >= 1, w + ": world < 1");
  int64_t total = 0;
  for (int i = 0; i < n_slots; ++i) {
    XDET_REQUIRE(slots[i].grad, w + ": a slot with a NULL pointer");
    XDET_REQUIRE(slots[i].n > 0, w + ": a slot with n <= 0");
    XDET_REQUIRE(slots[i].n <= GA_MAX_N, w + ": a slot beyond 2^35 elements");
    total += cdiv(slots[i].n, 4) * 4;
    XDET_REQUIRE(total <= GA_MAX_N, w + ": more than 2^22 runs of the flat element space");
  }
  plan->total = total;
  plan->chunk_elems = chunk_elems;
  plan->n_chunks = cdiv(total, chunk_elems);
  plan->runs_per_chunk = (int)cdiv(chunk_elems, GA_RUN);
  const int64_t runs = plan->n_chunks * plan->runs_per_chunk;
  XDET_REQUIRE(runs <= GA_MAX_RUNS, w + ": more than 2^22 runs of the flat element space");
  // [slots][run -> slot] and, for world > 1, [one packed chunk][world gathered chunks], each part on a 256-byte boundary
  const size_t chunk_bytes = ga_up((size_t)std::min(chunk_elems, total) * 4);
  *bytes = ga_up((size_t)n_slots * sizeof(GradSlotDev)) + ga_up((size_t)(runs + 1) * 4) +
           (world > 1 ? chunk_bytes + ga_up((size_t)world * (size_t)std::min(chunk_elems, total) * 4) : 0);
  return XDET_OK;
}

int grad_plan_upload(const xdet_grad_slot* slots, int n_slots, int64_t chunk_elems, int world, void* workspace, hipStream_t s,
                     const char* who, GradPlan* plan) {
  size_t bytes = 0;
  XDET_TRY(grad_plan_check(slots, n_slots, chunk_elems, world, who, plan, &bytes));
  XDET_REQUIRE(workspace, std::string(who) + ": workspace is NULL");
  std::vector<GradSlotDev> dev((size_t)n_slots);
  int64_t off = 0;
  for (int i = 0; i < n_slots; ++i) {
    GradSlotDev& d = dev[(size_t)i];
    d.grad = slots[i].grad; d.off = off; d.n = slots[i].n;
    d.vec = (reinterpret_cast<uintptr_t>(slots[i].grad) & 15) == 0;
    d.pad = 0;
    off += cdiv(slots[i].n, 4) * 4;
  }
  const int64_t runs = plan->n_chunks * plan->runs_per_chunk;
  std::vector<int> run_slot((size_t)runs + 1);
  int at = 0;                                                // (run starts grow with the run index: one walk)
  for (int64_t g = 0; g < runs; ++g) {
    const int64_t f0 = g / plan->runs_per_chunk * chunk_elems + g % plan->runs_per_chunk * GA_RUN;
    while (at + 1 < n_slots && dev[(size_t)at + 1].off <= f0) ++at;
    run_slot[(size_t)g] = at;
  }
  run_slot[(size_t)runs] = n_slots - 1;
  char* base = static_cast<char*>(workspace);
  GradSlotDev* d_slots = reinterpret_cast<GradSlotDev*>(base);
  int* d_runs = reinterpret_cast<int*>(base + ga_up(dev.size() * sizeof(GradSlotDev)));
  // (pageable sources: the runtime has staged both tables when the calls return)
  XDET_HIP(hipMemcpyAsync(d_slots, dev.data(), dev.size() * sizeof(GradSlotDev), hipMemcpyHostToDevice, s));
  XDET_HIP(hipMemcpyAsync(d_runs, run_slot.data(), run_slot.size() * 4, hipMemcpyHostToDevice, s));
  plan->d_slots = d_slots;
  plan->d_runs = d_runs;
  if (world > 1) {
    const size_t chunk_bytes = ga_up((size_t)std::min(chunk_elems, plan->total) * 4);
    plan->flat = reinterpret_cast<float*>(reinterpret_cast<char*>(d_runs) + ga_up(run_slot.size() * 4));
    plan->gathered = reinterpret_cast<float*>(reinterpret_cast<char*>(plan->flat) + chunk_bytes);
  }
  return XDET_OK;
}

int grad_launch_pack(const GradPlan& plan, int64_t chunk, float* flat_out, hipStream_t s) {
  const int len = (int)plan.chunk_len(chunk);
  hipLaunchKernelGGL(grad_pack_kernel, dim3((unsigned)cdiv(len, GA_RUN)), dim3(GA_T), 0, s, plan.d_slots,
                     plan.d_runs + chunk * plan.runs_per_chunk, (long long)(chunk * plan.chunk_elems), len, flat_out);
  XDET_LAUNCH_CHECK();
  return XDET_OK;
}

int grad_launch_reduce(const GradPlan& plan, int64_t chunk, const float* gathered, int world, hipStream_t s) {
  const int len = (int)plan.chunk_len(chunk);
  hipLaunchKernelGGL(grad_reduce_ranks_kernel, dim3((unsigned)cdiv(len, GA_RUN)), dim3(GA_T), 0, s, plan.d_slots,
                     plan.d_runs + chunk * plan.runs_per_chunk, (long long)(chunk * plan.chunk_elems), len, gathered, world);
  XDET_LAUNCH_CHECK();
  return XDET_OK;
}

}  // namespace xdet

using namespace xdet;

extern "C" {

size_t xdet_grad_average_workspace_bytes(const xdet_grad_slot* slots, int n_slots, int world, int64_t chunk_elems) {
  GradPlan plan;
  size_t bytes = 0;
  return grad_plan_check(slots, n_slots, chunk_elems, world, "grad_average", &plan, &bytes) == XDET_OK ? bytes : 0;
}

int xdet_grad_pack(const xdet_grad_slot* slots, int n_slots, int64_t chunk, int64_t chunk_elems, float* flat_out, void* workspace,
                   void* stream) {
  GradPlan plan;
  size_t bytes = 0;
  XDET_TRY(grad_plan_check(slots, n_slots, chunk_elems, 1, "grad_pack", &plan, &bytes));
  XDET_REQUIRE(chunk >= 0 && chunk < plan.n_chunks, "grad_pack: the chunk index is outside the flat element space");
  XDET_REQUIRE(flat_out && (reinterpret_cast<uintptr_t>(flat_out) & 15) == 0, "grad_pack: flat_out must be a 16-byte aligned device pointer");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  XDET_TRY(grad_plan_upload(slots, n_slots, chunk_elems, 1, workspace, s, "grad_pack", &plan));
  return grad_launch_pack(plan, chunk, flat_out, s);
}

int xdet_grad_reduce_ranks(const xdet_grad_slot* slots, int n_slots, int64_t chunk, int64_t chunk_elems, const float* gathered,
                           int world, void* workspace, void* stream) {
  GradPlan plan;
  size_t bytes = 0;
  XDET_TRY(grad_plan_check(slots, n_slots, chunk_elems, world, "grad_reduce_ranks", &plan, &bytes));
  XDET_REQUIRE(chunk >= 0 && chunk < plan.n_chunks, "grad_reduce_ranks: the chunk index is outside the flat element space");
  XDET_REQUIRE(gathered && (reinterpret_cast<uintptr_t>(gathered) & 15) == 0,
               "grad_reduce_ranks: gathered must be a 16-byte aligned device pointer");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  // (world 1 here: the doors are handed their chunk buffers and take the tables alone from the workspace)
  XDET_TRY(grad_plan_upload(slots, n_slots, chunk_elems, 1, workspace, s, "grad_reduce_ranks", &plan));
  return grad_launch_reduce(plan, chunk, gathered, world, s);
}

}  // extern "C"
