// The checkpoint op of the training path (include/xdet.h): xdet_crc32c, the CRC-32C of a table of device buffers and, where a
// slot names a destination, their copy in the same pass.  It is what lets MomentumOptimizer.snapshot() put the training state
// aside and checksum it at memory rate instead of on the host thread that drives the step.
//
// CRC is linear on the raw register: reg(A || B) = shift_|B|(reg(A)) xor reg_0(B), where shift_n multiplies by x^(8n) mod P
// over GF(2) (reflected: bit 31 of a word is x^0, a multiplication by x is a right shift with a conditional xor of P).
//
// Chunk pass, one launch over all slots.  A slot is cut into units of CRC_UNIT = 128 bytes and a tail below one unit; a chunk
// is CRC_T = 256 consecutive units, CRC_CHUNK = 32 KiB, of ONE slot, owned by one workgroup of 256 lanes.  A lane owns one
// unit: it issues its eight 16-byte loads (32 dwords where the slot's pointers are not 16-byte aligned) before the first use,
// stores them to dst as they came, and runs them through slicing-by-4 tables in LDS (4 KiB, computed by the workgroup itself:
// no table is read from memory).  The lane that owns the slot's first unit starts from 0xffffffff, every other from 0, so the
// initial register needs no separate term.  A slot's last chunk is short: its units are RIGHT-aligned over the lanes, and the
// lanes in front hold 0 -- leading zeros leave a zero register alone -- so every shift of the tree below is a compile-time
// constant.  Six levels inside a wave (lane i takes lane i - w, times x^(8 * 128 * w)), the four waves' registers in order by
// the last lane, and behind them the tail: its dwords and bytes are loaded once by the first lanes, stored, parked in LDS and
// run through the tables by the last lane.  One register per chunk goes to the workspace.
//
// Fold pass, one launch, one workgroup per slot.  All chunks but the last are CRC_CHUNK long: they are right-aligned over P
// lanes (P the power of two at or above their number, at most 256), G consecutive ones per lane folded by Horner's rule with
// the constant x^(8 * CRC_CHUNK), then log2 P tree levels with x^(8 * CRC_CHUNK * G * 2^k) -- so the 31 MB kernel of the
// large-separable block, 970 chunks, is 4 Horner steps and 8 levels, not 970 steps in one lane.  The last chunk's register
// joins behind x^(8 * its length).  Those nine powers per slot are computed on the host and travel with the slot table.
//
// Integer arithmetic only; no atomics, no fence, no workgroup that waits for another: the second launch is the barrier.
#include "layers.h"

namespace xdet {

constexpr int CRC_T = 256;                        // lanes of a workgroup
constexpr int CRC_UNIT = 128;                     // bytes a lane owns
constexpr int CRC_UNIT_DW = CRC_UNIT / 4;
constexpr int CRC_CHUNK = CRC_T * CRC_UNIT;       // bytes of a chunk
constexpr int CRC_MAX_SLOTS = 1 << 16;
constexpr int64_t CRC_MAX_CHUNKS = 1 << 22;
constexpr uint32_t CRC_POLY = 0x82f63b78u;        // Castagnoli, reflected

// a * b mod P (reflected representation)
__host__ __device__ constexpr uint32_t crc_mul(uint32_t a, uint32_t b) {
  uint32_t r = 0;
#pragma unroll
  for (int i = 0; i < 32; ++i) {
    r ^= b & (0u - (a >> 31));
    a <<= 1;
    b = (b >> 1) ^ (CRC_POLY & (0u - (b & 1u)));
  }
  return r;
}

// x^(8 n) mod P
__host__ __device__ constexpr uint32_t crc_xpow8(uint64_t n) {
  uint32_t r = 0x80000000u;                       // x^0
  uint32_t sq = 0x00800000u;                      // x^8
  while (n) {
    if (n & 1) r = crc_mul(r, sq);
    sq = crc_mul(sq, sq);
    n >>= 1;
  }
  return r;
}

constexpr uint32_t CRC_X_WAVE = crc_xpow8(64 * CRC_UNIT);
constexpr uint32_t CRC_X_CHUNK = crc_xpow8(CRC_CHUNK);

struct CrcSlotDev {                               // a slot as the kernels read it
  const unsigned char* src;
  unsigned char* dst;                             // NULL: checksum only
  unsigned long long bytes;
  int first_chunk, n_chunks;
  int vec;                                        // src and dst (where given) are 16-byte aligned
  int P, G;                                       // the fold's lanes and registers per lane (n_chunks > 1)
  uint32_t tail_pow;                              // x^(8 * the last chunk's length)
  uint32_t lvl[8];                                // x^(8 * CRC_CHUNK * G * 2^k)
};

// one dword through the four tables; `tab` is [4][256] in LDS, tab[0] the byte table
__device__ __forceinline__ uint32_t crc_dword(const uint32_t* tab, uint32_t c, uint32_t d) {
  c ^= d;
  return tab[768 + (c & 0xff)] ^ tab[512 + ((c >> 8) & 0xff)] ^ tab[256 + ((c >> 16) & 0xff)] ^ tab[c >> 24];
}

// level K of the tree inside a wave: lane i takes the register of lane i - 2^K in front of its own (2^K units lie between their ends)
template <int K>
__device__ __forceinline__ uint32_t crc_wave_level(uint32_t r, int lane) {
  constexpr uint32_t X = crc_xpow8((uint64_t)CRC_UNIT << K);
  constexpr int m = (2 << K) - 1;
  const uint32_t left = (uint32_t)__shfl_up((int)r, 1u << K, 64);
  return (lane & m) == m ? crc_mul(left, X) ^ r : r;
}

__global__ __launch_bounds__(CRC_T) void crc32c_chunk_kernel(const CrcSlotDev* __restrict__ slots, const int* __restrict__ chunk_slot,
                                                             uint32_t* __restrict__ regs) {
  __shared__ uint32_t tab[4 * 256];
  __shared__ uint32_t tail[CRC_UNIT_DW];          // the slot's tail: whole dwords, then one word of its last 1-3 bytes
  __shared__ uint32_t wave_reg[CRC_T / 64];
  const int tid = threadIdx.x;
  {
    uint32_t c = (uint32_t)tid;
#pragma unroll
    for (int k = 0; k < 8; ++k) c = (c >> 1) ^ (CRC_POLY & (0u - (c & 1u)));
    tab[tid] = c;
    __syncthreads();
#pragma unroll
    for (int t = 1; t < 4; ++t) {
      c = (c >> 8) ^ tab[c & 0xff];
      tab[t * 256 + tid] = c;
    }
  }
  const CrcSlotDev s = slots[chunk_slot[blockIdx.x]];
  const int c = (int)blockIdx.x - s.first_chunk;
  const unsigned long long units = s.bytes / CRC_UNIT;
  const unsigned long long first = (unsigned long long)c * CRC_T;           // the chunk's first unit
  const int u = (int)min((unsigned long long)CRC_T, units - min(units, first));   // its units: 0 only for a slot below one unit
  const bool last = c == s.n_chunks - 1;
  const int rem = last ? (int)(s.bytes % CRC_UNIT) : 0;
  const int lane_unit = tid - (CRC_T - u);                                  // right-aligned
  const bool own = lane_unit >= 0;
  const unsigned long long unit = first + (unsigned long long)max(lane_unit, 0);
  uint32_t d[CRC_UNIT_DW];
  if (own) {
    const unsigned long long at = unit * CRC_UNIT;
    if (s.vec) {
      const uint4* p = reinterpret_cast<const uint4*>(s.src + at);
#pragma unroll
      for (int i = 0; i < CRC_UNIT_DW / 4; ++i) {
        const uint4 v = p[i];
        d[4 * i] = v.x; d[4 * i + 1] = v.y; d[4 * i + 2] = v.z; d[4 * i + 3] = v.w;
      }
      if (s.dst) {
        uint4* q = reinterpret_cast<uint4*>(s.dst + at);
#pragma unroll
        for (int i = 0; i < CRC_UNIT_DW / 4; ++i) q[i] = make_uint4(d[4 * i], d[4 * i + 1], d[4 * i + 2], d[4 * i + 3]);
      }
    } else {
      const uint32_t* p = reinterpret_cast<const uint32_t*>(s.src + at);
#pragma unroll
      for (int i = 0; i < CRC_UNIT_DW; ++i) d[i] = p[i];
      if (s.dst) {
        uint32_t* q = reinterpret_cast<uint32_t*>(s.dst + at);
#pragma unroll
        for (int i = 0; i < CRC_UNIT_DW; ++i) q[i] = d[i];
      }
    }
  }
  // the tail: read once, stored, parked for the last lane
  const unsigned long long tail_at = units * CRC_UNIT;
  const int tail_dw = rem / 4, tail_b = rem % 4;
  if (tid < tail_dw) {
    const uint32_t v = reinterpret_cast<const uint32_t*>(s.src + tail_at)[tid];
    if (s.dst) reinterpret_cast<uint32_t*>(s.dst + tail_at)[tid] = v;
    tail[tid] = v;
  }
  if (tid == tail_dw && tail_b) {
    uint32_t v = 0;
    for (int b = 0; b < tail_b; ++b) {
      const unsigned char x = s.src[tail_at + 4 * (unsigned)tail_dw + b];
      if (s.dst) s.dst[tail_at + 4 * (unsigned)tail_dw + b] = x;
      v |= (uint32_t)x << (8 * b);
    }
    tail[tid] = v;
  }
  __syncthreads();                                // the tables and the tail are in LDS
  uint32_t r = 0;
  if (own) {
    r = unit == 0 ? 0xffffffffu : 0u;
#pragma unroll
    for (int i = 0; i < CRC_UNIT_DW; ++i) r = crc_dword(tab, r, d[i]);
  }
  const int lane = tid & 63;
  r = crc_wave_level<0>(r, lane);
  r = crc_wave_level<1>(r, lane);
  r = crc_wave_level<2>(r, lane);
  r = crc_wave_level<3>(r, lane);
  r = crc_wave_level<4>(r, lane);
  r = crc_wave_level<5>(r, lane);
  if ((tid & 63) == 63) wave_reg[tid >> 6] = r;
  __syncthreads();
  if (tid != CRC_T - 1) return;
  r = wave_reg[0];
#pragma unroll
  for (int w = 1; w < CRC_T / 64; ++w) r = crc_mul(r, CRC_X_WAVE) ^ wave_reg[w];
  if (u == 0 && c == 0) r = 0xffffffffu;          // a slot below one unit: the tail starts the register
  for (int i = 0; i < tail_dw; ++i) r = crc_dword(tab, r, tail[i]);
  if (tail_b) {
    const uint32_t v = tail[tail_dw];
    for (int b = 0; b < tail_b; ++b) r = tab[(r ^ (v >> (8 * b))) & 0xff] ^ (r >> 8);
  }
  regs[blockIdx.x] = r;
}

__global__ __launch_bounds__(CRC_T) void crc32c_fold_kernel(const CrcSlotDev* __restrict__ slots, const uint32_t* __restrict__ regs,
                                                            uint32_t* __restrict__ crc_out) {
  __shared__ uint32_t v[CRC_T];
  const int tid = threadIdx.x;
  const CrcSlotDev& s = slots[blockIdx.x];       // (read in place: lvl is indexed by the level)
  if (s.n_chunks == 0) {                          // an empty slot
    if (tid == 0) crc_out[blockIdx.x] = 0u;
    return;
  }
  const uint32_t* r = regs + s.first_chunk;
  const int full = s.n_chunks - 1;                // chunks of CRC_CHUNK bytes, in front of the last
  if (full == 0) {
    if (tid == 0) crc_out[blockIdx.x] = r[0] ^ 0xffffffffu;
    return;
  }
  const int P = s.P, G = s.G;
  const long long pad = (long long)P * G - full;  // right-aligned: `pad` absent chunks in front
  uint32_t acc = 0;
  if (tid < P) {
    for (int g = 0; g < G; ++g) {
      const long long i = (long long)tid * G + g - pad;
      acc = crc_mul(acc, CRC_X_CHUNK) ^ (i >= 0 ? r[i] : 0u);
    }
  }
  v[tid] = acc;
  __syncthreads();
  for (int k = 0; (1 << k) < P; ++k) {
    const int w = 1 << k;
    if (tid < P && (tid & (2 * w - 1)) == 2 * w - 1) v[tid] = crc_mul(v[tid - w], s.lvl[k]) ^ v[tid];
    __syncthreads();
  }
  if (tid == P - 1) crc_out[blockIdx.x] = (crc_mul(v[tid], s.tail_pow) ^ r[full]) ^ 0xffffffffu;
}

static size_t crc_up(size_t b) { return (b + 255) / 256 * 256; }

// the number of chunks of a slot: its units in chunks of CRC_T, and one chunk for a slot that is only a tail
static int64_t crc_slot_chunks(size_t bytes) {
  if (bytes == 0) return 0;
  const int64_t units = (int64_t)(bytes / CRC_UNIT);
  return units ? cdiv(units, (int64_t)CRC_T) : 1;
}

// checks the table and counts its chunks; errors before any GPU work
static int crc_measure(const xdet_crc_slot* slots, int n_slots, int64_t* n_chunks) {
  XDET_REQUIRE(slots && n_slots > 0, "crc32c: an empty slot table");
  XDET_REQUIRE(n_slots <= CRC_MAX_SLOTS, "crc32c: at most 65536 slots");
  *n_chunks = 0;
  for (int i = 0; i < n_slots; ++i) {
    const xdet_crc_slot& h = slots[i];
    XDET_REQUIRE(h.src || h.bytes == 0, "crc32c: a slot with a NULL src and bytes > 0");
    XDET_REQUIRE(((reinterpret_cast<uintptr_t>(h.src) | reinterpret_cast<uintptr_t>(h.dst)) & 3) == 0,
                 "crc32c: src and dst must be 4-byte aligned");
    *n_chunks += crc_slot_chunks(h.bytes);
    XDET_REQUIRE(*n_chunks <= CRC_MAX_CHUNKS, "crc32c: more than 2^22 chunks of 32 KiB");
  }
  return XDET_OK;
}

}  // namespace xdet

using namespace xdet;

extern "C" {

size_t xdet_crc32c_chunk_bytes(void) { return CRC_CHUNK; }

size_t xdet_crc32c_workspace_bytes(const xdet_crc_slot* slots, int n_slots) {
  int64_t chunks = 0;
  if (crc_measure(slots, n_slots, &chunks) != XDET_OK) return 0;
  // [slots][chunk -> slot][chunk registers], each on a 256-byte boundary
  return crc_up((size_t)n_slots * sizeof(CrcSlotDev)) + 2 * crc_up((size_t)std::max<int64_t>(chunks, 1) * 4);
}

int xdet_crc32c(const xdet_crc_slot* slots, int n_slots, uint32_t* crc_out_dev, void* workspace, void* stream) {
  int64_t chunks = 0;
  XDET_TRY(crc_measure(slots, n_slots, &chunks));
  XDET_REQUIRE(crc_out_dev, "crc32c: crc_out_dev is NULL");
  XDET_REQUIRE((reinterpret_cast<uintptr_t>(crc_out_dev) & 3) == 0, "crc32c: crc_out_dev must be 4-byte aligned");
  XDET_REQUIRE(workspace, "crc32c: workspace is NULL");
  std::vector<CrcSlotDev> dev((size_t)n_slots);
  std::vector<int> chunk_slot;
  chunk_slot.reserve((size_t)chunks);
  for (int i = 0; i < n_slots; ++i) {
    const xdet_crc_slot& h = slots[i];
    CrcSlotDev& d = dev[(size_t)i];
    d = CrcSlotDev();
    d.src = static_cast<const unsigned char*>(h.src);
    d.dst = h.bytes ? static_cast<unsigned char*>(h.dst) : nullptr;
    d.bytes = h.bytes;
    d.first_chunk = (int)chunk_slot.size();
    d.n_chunks = (int)crc_slot_chunks(h.bytes);
    d.vec = ((reinterpret_cast<uintptr_t>(h.src) | reinterpret_cast<uintptr_t>(h.dst)) & 15) == 0;
    d.P = d.G = 1;
    if (d.n_chunks > 1) {
      const int full = d.n_chunks - 1;
      while (d.P < full && d.P < CRC_T) d.P <<= 1;
      d.G = (int)cdiv(full, d.P);
      d.tail_pow = crc_xpow8(h.bytes - (uint64_t)full * CRC_CHUNK);
      d.lvl[0] = crc_xpow8((uint64_t)CRC_CHUNK * (uint64_t)d.G);
      for (int k = 1; k < 8; ++k) d.lvl[k] = crc_mul(d.lvl[k - 1], d.lvl[k - 1]);
    }
    chunk_slot.insert(chunk_slot.end(), (size_t)d.n_chunks, i);
  }
  char* base = static_cast<char*>(workspace);
  CrcSlotDev* d_slots = reinterpret_cast<CrcSlotDev*>(base);
  int* d_chunk = reinterpret_cast<int*>(base + crc_up(dev.size() * sizeof(CrcSlotDev)));
  uint32_t* d_regs = reinterpret_cast<uint32_t*>(reinterpret_cast<char*>(d_chunk) + crc_up((size_t)std::max<int64_t>(chunks, 1) * 4));
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  // (pageable sources: the runtime has staged both tables when the calls return)
  XDET_HIP(hipMemcpyAsync(d_slots, dev.data(), dev.size() * sizeof(CrcSlotDev), hipMemcpyHostToDevice, s));
  if (chunks) {
    XDET_HIP(hipMemcpyAsync(d_chunk, chunk_slot.data(), (size_t)chunks * 4, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(crc32c_chunk_kernel, dim3((unsigned)chunks), dim3(CRC_T), 0, s, d_slots, d_chunk, d_regs);
    XDET_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(crc32c_fold_kernel, dim3((unsigned)n_slots), dim3(CRC_T), 0, s, d_slots, d_regs, crc_out_dev);
  XDET_LAUNCH_CHECK();
  return XDET_OK;
}

}  // extern "C"
