// What the backward kernels on the matrix pipe share (dense_backward.hip, conv_backward.hip): the operand pre-pass that
// finds the three power-of-two scales and db, the fold of dW's range slabs, and the CU side of the split-precision GEMM
// tile with its double-buffered step loop -- everything except how an operand element is fetched from global memory,
// which is each file's own loader.
//
// The tile: 128 x BN outputs (BN 128: 2 x 2 waves of 64 x 64; BN 32: 4 x 1 waves of 32 x 32), reduction steps of 32.  A
// thread holds quads: four consecutive reduction indices of one tile row.  Without TRANS (the reduction index is
// contiguous in memory) eight consecutive threads cover a row's 32 steps; with TRANS (the reduction index is the
// operand's row in memory) consecutive threads take consecutive tile rows, so the global loads coalesce.  A quad is
// masked, scaled (v_ldexp_f32, exact), split into hi / lo halves and written as one 8-byte LDS store each; a stage holds
// A hi, A lo, B hi, B lo as rows of 32 + 8 halves (80 B: every MFMA operand is one conflict-free ds_read_b128).
#pragma once
#include "common.h"
#include "cu_prims.h"
#include <algorithm>

namespace xdet {

constexpr int DB_T = 256;
constexpr int DB_BM = 128;          // tile rows
constexpr int DB_BK = 32;           // reduction step
constexpr int DB_LDH = 40;          // u16 per LDS row: 32 + 8 pad
constexpr int DB_TARGET = 11;       // an operand's largest magnitude is moved into [2^11, 2^12)
constexpr int DB_MAX_CHUNKS = 1024; // row chunks of db
constexpr int DB_MAX_DIM = 4096;    // K, J
// control words at the head of the workspace
enum { DB_MAX_X = 0, DB_MAX_W = 1, DB_MAX_G = 2, DB_EXP_X = 4, DB_EXP_W = 5, DB_EXP_G = 6, DB_CTL_WORDS = 16 };

// db's row chunks and dW's row ranges: everything that shapes a sum depends on the sizes alone.  `k_rows` is the row
// count of dW as a matrix (K of a dense layer, kh * kw * C of a conv).
struct DbSums {
  int rows_per_chunk, n_chunks;     // db
  int bn_dw;                        // column tile of dW
  int rows_per_range, n_ranges;     // dW's reduction over M
};
static inline DbSums db_sums(int M, int k_rows, int J) {
  DbSums p;
  p.rows_per_chunk = (int)std::max<int64_t>(64, cdiv(M, DB_MAX_CHUNKS));
  p.n_chunks = (int)cdiv(M, p.rows_per_chunk);
  p.bn_dw = J <= 32 ? 32 : 128;
  const int64_t tiles = cdiv(k_rows, DB_BM) * cdiv(J, p.bn_dw);
  const int64_t want = std::max<int64_t>(1, 512 / tiles);              // about two workgroups per CU
  p.rows_per_range = (int)(cdiv(cdiv(M, want), 128) * 128);
  p.n_ranges = (int)cdiv(M, p.rows_per_range);
  return p;
}

struct DbWorkspace {
  unsigned* ctl;      // [DB_CTL_WORDS]
  float* partial;     // [n_chunks][J] db's row-chunk sums
  float* slabs;       // [n_ranges][k_rows][J] dW's range sums (more than one range only)
};
// the one description of the workspace of either backward call; its parts are whole words, packed (walk it with an alignment of 4 bytes)
static inline DbWorkspace db_layout(WsWalk& w, const DbSums& p, int k_rows, int J) {
  return {w.take<unsigned>(DB_CTL_WORDS), w.take<float>((size_t)p.n_chunks * J),
          w.take<float>(p.n_ranges > 1 ? (size_t)p.n_ranges * k_rows * J : 0)};
}

// The pre-pass of one call (dense_backward.hip): the largest magnitudes of x [M, x_cols] (relu_x: of max(x, 0), where a
// NaN counts as 0), w [w_rows, J] dense and g = mask(dy, y) [M, J] into ctl[DB_MAX_*] (ctl is zeroed first), their
// exponents into ctl[DB_EXP_*], db's chunk sums into partial [n_chunks][J] and db itself.
// A conv whose output map is not its input map has x of its own row count, x_rows (0: M), and may leave input pixels under
// no window: with x_w > 0 x's rows are the pixels of [x_h, x_w] maps, of which rows below x_hc and columns below x_wc count
// and the others are not read.
struct DbPre {
  const float *x, *w, *y, *dy;
  int ld_x, ld_y, ld_dy, M, x_cols, w_rows, J, relu_x;
  int rows_per_chunk, n_chunks;
  unsigned* ctl;
  float* partial;
  int x_rows, x_h, x_w, x_hc, x_wc;
};
int db_launch_prepass(const DbPre& a, float* db, hipStream_t s);
// dw [n] = slabs [n_ranges][n] added in index order
int db_launch_fold(const float* slabs, int n_ranges, int64_t n, float* dw, hipStream_t s);

static inline int db_vec(const float* p, int ld) { return p && (reinterpret_cast<uintptr_t>(p) & 15) == 0 && ld % 4 == 0; }

__device__ __forceinline__ unsigned db_abs_bits(float v) { return __float_as_uint(v) & 0x7FFFFFFFu; }

// every thread of the workgroup calls it, once per kernel: the workgroup's maximum, then ONE atomic -- a few thousand
// atomics on one address take longer than a stem-sized pre-pass needs for its loads
__device__ __forceinline__ void db_block_max(unsigned v, unsigned* dst) {
  __shared__ unsigned wave_max[DB_T / 64];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = max(v, (unsigned)__shfl_xor((int)v, o));
  if ((threadIdx.x & 63) == 0) wave_max[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    v = max(max(wave_max[0], wave_max[1]), max(wave_max[2], wave_max[3]));
    if (v) atomicMax(dst, v);
  }
}

// the power of two that moves a largest magnitude with the f32 bits m into [2^DB_TARGET, 2^(DB_TARGET + 1)); 0 for 0
__device__ __forceinline__ int db_scale_exp(unsigned m) {
  if (m == 0) return 0;
  const int e = (m >> 23) ? (int)(m >> 23) - 127 : (31 - __clz((int)m)) - 149;
  return DB_TARGET - e;
}

// y > 0 is false for a NaN: the gradient behind a NaN activation is 0
__device__ __forceinline__ float db_mask(float dy, float y) { return y > 0.f ? dy : 0.f; }

// ---- the conv backward's index arithmetic (conv_backward.hip) ----

constexpr int CB_MAX_TAPS = 15;     // kh, kw

// n / d for n < 2^31 as (umulhi(n, mul) + n) >> shift (Granlund & Montgomery's round-up multiplier)
struct CbDiv {
  unsigned mul, shift;
};
static inline CbDiv cb_div(unsigned d) {
  unsigned l = 0;
  while ((1ull << l) < d) ++l;
  return {(unsigned)(((1ull << 32) * ((1ull << l) - d)) / d + 1), l};
}
__device__ __forceinline__ int cb_quot(int n, CbDiv d) { return (int)((__umulhi((unsigned)n, d.mul) + (unsigned)n) >> d.shift); }

// four consecutive floats at p, of which `left` exist
__device__ __forceinline__ void cb_load_row4(const float* __restrict__ p, int left, bool vec, float (&v)[4]) {
  if (vec && left >= 4) {
    const float4 t = *reinterpret_cast<const float4*>(p);
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (e < left) v[e] = p[e];
  }
}

template <int BN>
struct DbTile {
  static constexpr int BM = DB_BM;
  static constexpr int WAVES_N = BN == 32 ? 1 : 2, WAVES_M = 4 / WAVES_N;
  static constexpr int WM = BM / WAVES_M, WN = BN / WAVES_N;
  static constexpr int TM = WM / 32, TN = WN / 32;
  static constexpr int A_IT = BM / 32, B_IT = BN / 32;      // quads per thread per step
  static constexpr int STAGE = (2 * BM + 2 * BN) * DB_LDH;  // u16 per stage: A hi, A lo, B hi, B lo
  static constexpr int LDS_BYTES = 2 * STAGE * (int)sizeof(u16);
};

// quad t (tid + DB_T * i) of an operand with `rows` tile rows (a power of two): its tile row and first reduction step
template <bool TRANS>
__device__ __forceinline__ int db_quad_row(int t, int rows) { return TRANS ? (t & (rows - 1)) : (t >> 3); }
template <bool TRANS>
__device__ __forceinline__ int db_quad_r(int t, int rows) { return 4 * (TRANS ? (t / rows) : (t & 7)); }

// a thread's IT quads of one operand -> its hi / lo rows of a stage; m: the ReLU outputs behind a masked operand, or NULL
template <int ROWS, int IT, bool TRANS>
__device__ __forceinline__ void db_store_quads(u16* hi_rows, u16* lo_rows, const float (&v)[IT][4], const float (*m)[4], int e) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int i = 0; i < IT; ++i) {
    const int t = tid + DB_T * i;
    float s[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) s[k] = ldexpf(m ? db_mask(v[i][k], m[i][k]) : v[i][k], e);
    u32x2 hi, lo;
    split4(s, &hi, &lo);
    const int o = db_quad_row<TRANS>(t, ROWS) * DB_LDH + db_quad_r<TRANS>(t, ROWS);
    *reinterpret_cast<u32x2*>(hi_rows + o) = hi;
    *reinterpret_cast<u32x2*>(lo_rows + o) = lo;
  }
}

template <int BN>
__device__ __forceinline__ void db_zero(f32x16 (&acc)[DbTile<BN>::TM][DbTile<BN>::TN]) {
#pragma unroll
  for (int i = 0; i < DbTile<BN>::TM; ++i)
#pragma unroll
    for (int j = 0; j < DbTile<BN>::TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
}

// one reduction step of a stage: hi*hi + hi*lo + lo*hi on v_mfma_f32_32x32x16_f16
template <int BN>
__device__ __forceinline__ void db_compute(const u16* stage, f32x16 (&acc)[DbTile<BN>::TM][DbTile<BN>::TN]) {
  using T = DbTile<BN>;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wm = wave / T::WAVES_N, wn = wave % T::WAVES_N, frow = lane & 31, fh = lane >> 5;
  const u16* Ah = stage + (wm * T::WM + frow) * DB_LDH + fh * 8;
  const u16* Al = Ah + T::BM * DB_LDH;
  const u16* Bh = stage + 2 * T::BM * DB_LDH + (wn * T::WN + frow) * DB_LDH + fh * 8;
  const u16* Bl = Bh + BN * DB_LDH;
#pragma unroll
  for (int ks = 0; ks < DB_BK / 16; ++ks) {
    f16x8 ah[T::TM], al[T::TM], bh[T::TN], bl[T::TN];
#pragma unroll
    for (int i = 0; i < T::TM; ++i) {
      ah[i] = *reinterpret_cast<const f16x8*>(Ah + i * 32 * DB_LDH + ks * 16);
      al[i] = *reinterpret_cast<const f16x8*>(Al + i * 32 * DB_LDH + ks * 16);
    }
#pragma unroll
    for (int j = 0; j < T::TN; ++j) {
      bh[j] = *reinterpret_cast<const f16x8*>(Bh + j * 32 * DB_LDH + ks * 16);
      bl[j] = *reinterpret_cast<const f16x8*>(Bl + j * 32 * DB_LDH + ks * 16);
    }
    // small cross terms first, the dominant hi*hi term last
#pragma unroll
    for (int i = 0; i < T::TM; ++i)
#pragma unroll
      for (int j = 0; j < T::TN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al[i], bh[j], acc[i][j], 0, 0, 0);
#pragma unroll
    for (int i = 0; i < T::TM; ++i)
#pragma unroll
      for (int j = 0; j < T::TN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[i], bl[j], acc[i][j], 0, 0, 0);
#pragma unroll
    for (int i = 0; i < T::TM; ++i)
#pragma unroll
      for (int j = 0; j < T::TN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[i], bh[j], acc[i][j], 0, 0, 0);
  }
}

// The reduction over `nk` steps on two LDS stages: step kt + 1 is requested from global memory while step kt is
// multiplied, then split into the other stage.  load(kt): the step's operands into the thread's registers; store(stage):
// those registers into a stage; compute(stage): one step of the product.
template <class Load, class Store, class Compute>
__device__ __forceinline__ void db_pipeline(int nk, Load&& load, Store&& store, Compute&& compute) {
  load(0);
  store(0);
  __syncthreads();
  for (int kt = 0; kt < nk; ++kt) {
    const bool more = kt + 1 < nk;
    if (more) load(kt + 1);
    compute(kt & 1);
    if (more) store((kt + 1) & 1);
    __syncthreads();
  }
}

// the tile's outputs: f(row, col, value) for every accumulator element, row / col relative to the tile.  Element reg of a
// lane: row (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5), column lane & 31
template <int BN, class F>
__device__ __forceinline__ void db_for_each_output(const f32x16 (&acc)[DbTile<BN>::TM][DbTile<BN>::TN], F&& f) {
  using T = DbTile<BN>;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wm = wave / T::WAVES_N, wn = wave % T::WAVES_N, frow = lane & 31, fh = lane >> 5;
#pragma unroll
  for (int i = 0; i < T::TM; ++i)
#pragma unroll
    for (int j = 0; j < T::TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r)
        f(wm * T::WM + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * fh, wn * T::WN + j * 32 + frow, acc[i][j][r]);
}

}  // namespace xdet
