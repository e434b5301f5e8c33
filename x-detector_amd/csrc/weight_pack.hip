// The table-driven pack op of the training step (include/xdet.h): xdet_tensors_concat writes dense parts side by side into a
// merged tensor, merged[o, off_p : off_p + width_p] = part_p[o, :], xdet_tensors_split is the inverse copy.  The merges a plan
// does on the host at build time (the large-separable block's two branches, the fused 1x1 heads of the RPN, the fused
// fc_cls | fc_loc of the head) and the split of their gradients are all this op with other numbers.
//
// Both directions are copies: no arithmetic, so every bit pattern (NaN payloads, -0, denormals) passes through.  The op is
// memory-bound, 8 bytes per element.  A workgroup of 256 threads owns one run of PK_RUN = 4096 consecutive elements of ONE
// part's dense space (a part's last run is short; runs never cross a part).  A thread owns four 4-element vectors, 1 KiB of
// a wave apart, so the dense side of every access of a wave is one contiguous KiB; all four loads are issued before the
// first store.  Element e of a part lies at row e / width, column e % width: a part whose width, offset and merged stride
// are multiples of 4 and whose two base pointers are 16-byte aligned never has a vector straddle a row, and both of its
// addresses are 16-byte aligned -- such a part moves as float4, every other one as single dwords.  Plain vector stores only.
#include "layers.h"

namespace xdet {

constexpr int PK_T = 256;                // threads of a workgroup
constexpr int PK_RUN = 4096;             // elements of a run: four float4 per thread
constexpr int PK_MAX_SLOTS = 1 << 16;
constexpr int PK_MAX_PARTS = 4;
constexpr int64_t PK_MAX_RUNS = 1 << 22;

struct PackPartDev {                     // one part of one slot as the kernel reads it
  float* merged;                         // the slot's merged tensor, advanced to the part's first column
  float* part;
  unsigned width, stride;                // the part's width; the merged tensor's row length
  unsigned n;                            // outer * width: the part's elements
  int first_run;
  int vec, pad;                          // vec: 16-byte accesses are safe (see above)
};

// CONCAT: part -> merged; otherwise merged -> part
template <bool CONCAT>
__global__ __launch_bounds__(PK_T) void tensors_pack_kernel(const PackPartDev* __restrict__ parts, const int* __restrict__ run_part) {
  const PackPartDev p = parts[run_part[blockIdx.x]];
  const unsigned start = (unsigned)((int)blockIdx.x - p.first_run) * PK_RUN;
  const unsigned left = p.n - start;                          // > 0 by construction of the run table
  const int tid = threadIdx.x;
  if (p.vec) {                                                // (uniform over the workgroup)
    float4 v[4];
    unsigned at_m[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const unsigned j = (unsigned)(i * PK_T + tid) * 4;
      const unsigned e = start + j;
      const unsigned row = e / p.width;
      at_m[i] = row * p.stride + (e - row * p.width);
      if (j < left) v[i] = *reinterpret_cast<const float4*>(CONCAT ? p.part + e : p.merged + at_m[i]);   // (n % 4 == 0: whole vectors)
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const unsigned j = (unsigned)(i * PK_T + tid) * 4;
      if (j < left) *reinterpret_cast<float4*>(CONCAT ? p.merged + at_m[i] : p.part + (start + j)) = v[i];
    }
    return;
  }
  // dwords: a wave's 64 lanes read 256 contiguous bytes of the dense side
  constexpr int PER = PK_RUN / PK_T;
  float v[PER];
  unsigned at_m[PER];
#pragma unroll
  for (int i = 0; i < PER; ++i) {
    const unsigned j = (unsigned)(i * PK_T + tid);
    const unsigned e = start + j;
    const unsigned row = e / p.width;
    at_m[i] = row * p.stride + (e - row * p.width);
    if (j < left) v[i] = CONCAT ? p.part[e] : p.merged[at_m[i]];
  }
#pragma unroll
  for (int i = 0; i < PER; ++i) {
    const unsigned j = (unsigned)(i * PK_T + tid);
    if (j < left) {
      if (CONCAT) p.merged[at_m[i]] = v[i];
      else p.part[start + j] = v[i];
    }
  }
}

static size_t pack_up(size_t b) { return (b + 255) / 256 * 256; }

// checks the table and counts its parts and runs; errors before any GPU work
static int pack_measure(const xdet_pack_slot* slots, int n_slots, const char* who, size_t* n_parts, int64_t* n_runs) {
  const std::string w(who);
  XDET_REQUIRE(slots && n_slots > 0, w + ": an empty slot table");
  XDET_REQUIRE(n_slots <= PK_MAX_SLOTS, w + ": at most 65536 slots");
  *n_parts = 0;
  *n_runs = 0;
  for (int i = 0; i < n_slots; ++i) {
    const xdet_pack_slot& h = slots[i];
    XDET_REQUIRE(h.merged, w + ": a slot with a NULL merged tensor");
    XDET_REQUIRE(h.outer > 0, w + ": a slot with outer <= 0");
    XDET_REQUIRE(h.n_parts > 0 && h.n_parts <= PK_MAX_PARTS, w + ": a slot has 1 to 4 parts");
    int64_t total = 0;
    for (int p = 0; p < h.n_parts; ++p) {
      XDET_REQUIRE(h.part[p], w + ": a slot with a NULL part");
      XDET_REQUIRE(h.width[p] > 0, w + ": a part with a width <= 0");
      total += h.width[p];
    }
    XDET_REQUIRE((int64_t)h.outer * total < ((int64_t)1 << 31), w + ": a merged tensor of 2^31 elements or more");
    for (int p = 0; p < h.n_parts; ++p) *n_runs += cdiv((int64_t)h.outer * h.width[p], PK_RUN);
    *n_parts += (size_t)h.n_parts;
    XDET_REQUIRE(*n_runs <= PK_MAX_RUNS, w + ": more than 2^22 runs of 4096 elements");
  }
  return XDET_OK;
}

static size_t pack_workspace_bytes(const xdet_pack_slot* slots, int n_slots) {
  size_t n_parts = 0;
  int64_t n_runs = 0;
  if (pack_measure(slots, n_slots, "tensors_pack", &n_parts, &n_runs) != XDET_OK) return 0;
  // [parts][run -> part], each on a 256-byte boundary
  return pack_up(n_parts * sizeof(PackPartDev)) + pack_up((size_t)n_runs * 4);
}

template <bool CONCAT>
static int pack_launch(const xdet_pack_slot* slots, int n_slots, void* workspace, void* stream) {
  const char* who = CONCAT ? "tensors_concat" : "tensors_split";
  size_t n_parts = 0;
  int64_t n_runs = 0;
  XDET_TRY(pack_measure(slots, n_slots, who, &n_parts, &n_runs));
  XDET_REQUIRE(workspace, std::string(who) + ": workspace is NULL");
  std::vector<PackPartDev> dev;
  std::vector<int> run_part;
  dev.reserve(n_parts);
  run_part.reserve((size_t)n_runs);
  for (int i = 0; i < n_slots; ++i) {
    const xdet_pack_slot& h = slots[i];
    unsigned stride = 0;
    for (int p = 0; p < h.n_parts; ++p) stride += (unsigned)h.width[p];
    unsigned off = 0;
    for (int p = 0; p < h.n_parts; ++p) {
      PackPartDev d;
      d.merged = h.merged + off;
      d.part = h.part[p];
      d.width = (unsigned)h.width[p];
      d.stride = stride;
      d.n = (unsigned)h.outer * d.width;
      d.first_run = (int)run_part.size();
      const bool aligned = ((reinterpret_cast<uintptr_t>(h.merged) | reinterpret_cast<uintptr_t>(h.part[p])) & 15) == 0;
      d.vec = aligned && d.width % 4 == 0 && off % 4 == 0 && (stride % 4 == 0 || h.outer == 1);
      d.pad = 0;
      const int64_t runs = cdiv((int64_t)d.n, PK_RUN);
      run_part.insert(run_part.end(), (size_t)runs, (int)dev.size());
      dev.push_back(d);
      off += d.width;
    }
  }
  char* base = static_cast<char*>(workspace);
  PackPartDev* d_parts = reinterpret_cast<PackPartDev*>(base);
  int* d_runs = reinterpret_cast<int*>(base + pack_up(dev.size() * sizeof(PackPartDev)));
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  // (pageable sources: the runtime has staged both tables when the calls return)
  XDET_HIP(hipMemcpyAsync(d_parts, dev.data(), dev.size() * sizeof(PackPartDev), hipMemcpyHostToDevice, s));
  XDET_HIP(hipMemcpyAsync(d_runs, run_part.data(), run_part.size() * 4, hipMemcpyHostToDevice, s));
  hipLaunchKernelGGL(tensors_pack_kernel<CONCAT>, dim3((unsigned)run_part.size()), dim3(PK_T), 0, s, d_parts, d_runs);
  XDET_LAUNCH_CHECK();
  return XDET_OK;
}

}  // namespace xdet

using namespace xdet;

extern "C" {

size_t xdet_tensors_concat_workspace_bytes(const xdet_pack_slot* slots, int n_slots) { return pack_workspace_bytes(slots, n_slots); }

size_t xdet_tensors_split_workspace_bytes(const xdet_pack_slot* slots, int n_slots) { return pack_workspace_bytes(slots, n_slots); }

int xdet_tensors_concat(const xdet_pack_slot* slots, int n_slots, void* workspace, void* stream) {
  return pack_launch<true>(slots, n_slots, workspace, stream);
}

int xdet_tensors_split(const xdet_pack_slot* slots, int n_slots, void* workspace, void* stream) {
  return pack_launch<false>(slots, n_slots, workspace, stream);
}

}  // extern "C"
