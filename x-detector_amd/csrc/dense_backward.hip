// The backward of a dense layer y = act(x W + b) on the gfx950 matrix pipe (xdet_dense_backward, include/xdet.h):
//
//     g  = dy, or dy * (y > 0) behind a ReLU           [M, J]
//     dx = g W^T   [M, K]      dW = x^T g   [K, J]      db = column sums of g   [J]
//
// Both products are split-precision f16 ("f16x3"): every operand is hi = f16(v), lo = f16(v - hi), a product is
// hi*hi + hi*lo + lo*hi on v_mfma_f32_32x32x16_f16 with f32 accumulation.  Gradients are not activations: d loss / d logits
// is of the order 1 / (rows in the batch) and smaller, where the lo half of an f16 split is subnormal or gone.  So each of
// the three operands (x, W, g) is multiplied by a power of two of its own before it is split, chosen ON THE DEVICE from the
// operand's largest magnitude so that this maximum lands in [2^11, 2^12) (the 16x headroom to 65504 of DESIGN §3b), and the
// epilogue multiplies by the inverse powers.  Both steps are exact (v_ldexp_f32), so the outputs of dy * 2^-30 are the
// outputs of dy times 2^-30, bit for bit.  An all-zero operand has the exponent 0: no log2, no division.
//
// Launches of one call, all on the caller's stream, nothing read on the host:
//   db_prepass_kernel   the three maxima (integer atomicMax of the f32 bits: order-free) and db's partial sums over fixed
//                       row chunks (one thread per column walks its chunk in row order)
//   db_final_kernel     db = the chunks added in index order; the three exponents
//   db_gemm_kernel<BN, false>   dx: C[m, k] = sum_j g[m, j] W[k, j] -- both operands have the reduction index contiguous
//   db_gemm_kernel<BN, true>    dW: C[k, j] = sum_m x[m, k] g[m, j] -- both operands have the reduction index as their ROW:
//                       lanes run along the operand's row so the global loads coalesce, and each packs four reduction steps
//                       into one 8-byte LDS write.  The reduction over M is cut into row ranges that depend on (M, K, J)
//                       only (db_plan); a range writes its slab of the workspace
//   db_fold_kernel      dW = the slabs added in index order (skipped for a single range, which writes dW itself)
// No float atomics anywhere: the same call gives the same bits.
//
// The GEMM kernel: a 128 x BN tile (BN 128: 2 x 2 waves of 64 x 64; BN 32 for an output of at most 32 columns: 4 x 1 waves
// of 32 x 32), reduction steps of 32.  Operands are read as f32 from global memory one step ahead into registers (g: dy and
// y, the mask and the scale are applied when the step is stored), split in registers and staged in LDS as hi / lo rows of
// 32 + 8 halves (80 B: every MFMA operand is one conflict-free ds_read_b128, conv_mfma_split.hip's layout), two stages, one
// barrier per step.  Ragged edges in all three dimensions are predicated loads that feed zeros: nothing is read at or beyond
// an operand's width or row count, so padding columns may hold anything.
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

struct DbPlan {
  int rows_per_chunk, n_chunks;     // db
  int bn_dx, bn_dw;                 // column tiles of the two products
  int rows_per_range, n_ranges;     // dW's reduction over M
};

// everything that shapes a sum depends on (M, K, J) alone
static DbPlan db_plan(int M, int K, int J) {
  DbPlan p;
  p.rows_per_chunk = (int)std::max<int64_t>(64, cdiv(M, DB_MAX_CHUNKS));
  p.n_chunks = (int)cdiv(M, p.rows_per_chunk);
  p.bn_dx = K <= 32 ? 32 : 128;
  p.bn_dw = J <= 32 ? 32 : 128;
  const int64_t tiles = cdiv(K, DB_BM) * cdiv(J, p.bn_dw);
  const int64_t want = std::max<int64_t>(1, 512 / tiles);              // about two workgroups per CU
  p.rows_per_range = (int)(cdiv(cdiv(M, want), 128) * 128);
  p.n_ranges = (int)cdiv(M, p.rows_per_range);
  return p;
}

struct DbWorkspace {
  unsigned* ctl;      // [DB_CTL_WORDS]
  float* partial;     // [n_chunks][J] db's row-chunk sums
  float* slabs;       // [n_ranges][K][J] dW's range sums (more than one range only)
};
// the one description of the workspace; its parts are whole words, packed (walk it with an alignment of 4 bytes)
static DbWorkspace db_layout(WsWalk& w, const DbPlan& p, int K, int J) {
  return {w.take<unsigned>(DB_CTL_WORDS), w.take<float>((size_t)p.n_chunks * J),
          w.take<float>(p.n_ranges > 1 ? (size_t)p.n_ranges * K * J : 0)};
}

__device__ __forceinline__ unsigned db_abs_bits(float v) { return __float_as_uint(v) & 0x7FFFFFFFu; }

// every thread of the workgroup calls it
__device__ __forceinline__ void db_block_max(unsigned v, unsigned* dst) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = max(v, (unsigned)__shfl_xor((int)v, o));
  if ((threadIdx.x & 63) == 0 && v) atomicMax(dst, v);
}

// the power of two that moves a largest magnitude with the f32 bits m into [2^DB_TARGET, 2^(DB_TARGET + 1)); 0 for 0
__device__ __forceinline__ int db_scale_exp(unsigned m) {
  if (m == 0) return 0;
  const int e = (m >> 23) ? (int)(m >> 23) - 127 : (31 - __clz((int)m)) - 149;
  return DB_TARGET - e;
}

// y > 0 is false for a NaN: the gradient behind a NaN activation is 0
__device__ __forceinline__ float db_mask(float dy, float y) { return y > 0.f ? dy : 0.f; }

struct DbPre {
  const float *x, *w, *y, *dy;
  int ld_x, ld_y, ld_dy, M, K, J;
  int rows_per_chunk, n_chunks, jblocks, x_blocks, w_blocks;
  unsigned* ctl;
  float* partial;     // [n_chunks][J]
};

__global__ __launch_bounds__(DB_T) void db_prepass_kernel(DbPre a) {
  const int tid = threadIdx.x;
  int b = blockIdx.x;
  unsigned mx = 0;
  const int g_blocks = a.n_chunks * a.jblocks;
  if (b < g_blocks) {
    const int c = b / a.jblocks, j = (b - c * a.jblocks) * DB_T + tid;
    if (j < a.J) {
      const int64_t m0 = (int64_t)c * a.rows_per_chunk, m1 = min((int64_t)a.M, m0 + a.rows_per_chunk);
      float s = 0.f;
      for (int64_t m = m0; m < m1; ++m) {
        float g = a.dy[m * a.ld_dy + j];
        if (a.y) g = db_mask(g, a.y[m * a.ld_y + j]);
        s += g;
        mx = max(mx, db_abs_bits(g));
      }
      a.partial[(int64_t)c * a.J + j] = s;
    }
    db_block_max(mx, a.ctl + DB_MAX_G);
    return;
  }
  b -= g_blocks;
  const bool is_x = b < a.x_blocks;
  if (!is_x) b -= a.x_blocks;
  const float* p = is_x ? a.x : a.w;
  const unsigned width = is_x ? a.K : a.J, ld = is_x ? a.ld_x : a.J;
  const unsigned n = (unsigned)(is_x ? a.M : a.K) * width;          // < 2^31
  const unsigned step = (unsigned)(is_x ? a.x_blocks : a.w_blocks) * DB_T;
  for (unsigned i = (unsigned)b * DB_T + tid; i < n; i += step) {
    const unsigned row = i / width, col = i - row * width;
    mx = max(mx, db_abs_bits(p[(int64_t)row * ld + col]));
  }
  db_block_max(mx, a.ctl + (is_x ? DB_MAX_X : DB_MAX_W));
}

__global__ __launch_bounds__(DB_T) void db_final_kernel(const float* __restrict__ partial, int n_chunks, int J, unsigned* ctl,
                                                        float* __restrict__ db) {
  const int j = blockIdx.x * DB_T + threadIdx.x;
  if (blockIdx.x == 0 && threadIdx.x < 3) ctl[DB_EXP_X + threadIdx.x] = (unsigned)db_scale_exp(ctl[DB_MAX_X + threadIdx.x]);
  if (j >= J) return;
  float s = 0.f;
  for (int c = 0; c < n_chunks; ++c) s += partial[(int64_t)c * J + j];
  db[j] = s;
}

// C[P, Q] = sum over r of A(p, r) B(q, r).  TRANS false: an operand's element (row, r) is at [row * ld + r] (dx: A = g,
// B = W); true: at [r * ld + row] (dW: A = x, B = g).  The masked operand g is A without TRANS and B with it.
struct DbGemm {
  const float *a, *b, *y;       // y: the ReLU output behind g (NULL: none), indexed like g
  int ld_a, ld_b, ld_y;
  int P, Q, R;
  int r_per_range;              // reduction indices per blockIdx.z
  const unsigned* ctl;
  int ea_slot, eb_slot;         // control words holding the two operands' exponents
  float* out;
  int ld_out;
  int64_t range_stride;         // floats between the outputs of two ranges
  int vec_a, vec_b, vec_y;      // !TRANS: rows may be read as aligned float4
};

template <bool TRANS>
__device__ __forceinline__ void db_load4(const float* __restrict__ p, int ld, int row, int r, int rows, int r_end, bool vec,
                                         float (&v)[4]) {
#pragma unroll
  for (int e = 0; e < 4; ++e) v[e] = 0.f;
  if (row >= rows) return;
  if (TRANS) {
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (r + e < r_end) v[e] = p[(int64_t)(r + e) * ld + row];
  } else {
    const float* q = p + (int64_t)row * ld + r;
    if (vec && r + 4 <= r_end) {
      const float4 t = *reinterpret_cast<const float4*>(q);
      v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (r + e < r_end) v[e] = q[e];
    }
  }
}

template <int BN, bool TRANS>
__global__ __launch_bounds__(DB_T) void db_gemm_kernel(DbGemm g) {
  constexpr int BM = DB_BM;
  constexpr int WAVES_N = BN == 32 ? 1 : 2, WAVES_M = 4 / WAVES_N;
  constexpr int WM = BM / WAVES_M, WN = BN / WAVES_N;
  constexpr int TM = WM / 32, TN = WN / 32;
  constexpr int A_IT = BM / 32, B_IT = BN / 32;      // quads (four reduction steps of one row) per thread per step
  constexpr int STAGE = (2 * BM + 2 * BN) * DB_LDH;  // u16 per stage: A hi, A lo, B hi, B lo
  constexpr bool A_MASK = !TRANS, B_MASK = TRANS;

  extern __shared__ __attribute__((aligned(16))) u16 db_smem[];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave / WAVES_N, wn = wave % WAVES_N;
  const int p0 = blockIdx.x * BM, q0 = blockIdx.y * BN;
  const int r0 = blockIdx.z * g.r_per_range, r1 = min(g.R, r0 + g.r_per_range);
  const int nk = (r1 - r0 + DB_BK - 1) / DB_BK;
  const int ea = (int)g.ctl[g.ea_slot], eb = (int)g.ctl[g.eb_slot];

  // quad t of an operand with ROWS tile rows: without TRANS eight consecutive threads cover a row's 32 steps, with TRANS
  // consecutive threads take consecutive rows (the contiguous index in memory)
  auto quad_row = [&](int t, int rows_pow2) { return TRANS ? (t & (rows_pow2 - 1)) : (t >> 3); };
  auto quad_r = [&](int t, int rows_pow2) { return 4 * (TRANS ? (t / rows_pow2) : (t & 7)); };

  struct Regs {
    float a[A_IT][4], b[B_IT][4], m[A_MASK ? A_IT : B_IT][4];
  };

  auto load_global = [&](int kt, Regs& r) {
    const int rk = r0 + kt * DB_BK;
#pragma unroll
    for (int i = 0; i < A_IT; ++i) {
      const int t = tid + DB_T * i, row = p0 + quad_row(t, BM), rr = rk + quad_r(t, BM);
      db_load4<TRANS>(g.a, g.ld_a, row, rr, g.P, r1, g.vec_a, r.a[i]);
      if constexpr (A_MASK) {
        if (g.y) db_load4<TRANS>(g.y, g.ld_y, row, rr, g.P, r1, g.vec_y, r.m[i]);
        else
#pragma unroll
          for (int e = 0; e < 4; ++e) r.m[i][e] = 1.f;
      }
    }
#pragma unroll
    for (int i = 0; i < B_IT; ++i) {
      const int t = tid + DB_T * i, row = q0 + quad_row(t, BN), rr = rk + quad_r(t, BN);
      db_load4<TRANS>(g.b, g.ld_b, row, rr, g.Q, r1, g.vec_b, r.b[i]);
      if constexpr (B_MASK) {
        if (g.y) db_load4<TRANS>(g.y, g.ld_y, row, rr, g.Q, r1, g.vec_y, r.m[i]);
        else
#pragma unroll
          for (int e = 0; e < 4; ++e) r.m[i][e] = 1.f;
      }
    }
  };
  auto store_lds = [&](int buf, const Regs& r) {
    u16* Ah = db_smem + buf * STAGE;
    u16* Al = Ah + BM * DB_LDH;
    u16* Bh = Al + BM * DB_LDH;
    u16* Bl = Bh + BN * DB_LDH;
#pragma unroll
    for (int i = 0; i < A_IT; ++i) {
      const int t = tid + DB_T * i;
      float v[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float t = r.a[i][e];
        if constexpr (A_MASK) t = db_mask(t, r.m[i][e]);
        v[e] = ldexpf(t, ea);
      }
      u32x2 hi, lo;
      split4(v, &hi, &lo);
      const int o = quad_row(t, BM) * DB_LDH + quad_r(t, BM);
      *reinterpret_cast<u32x2*>(Ah + o) = hi;
      *reinterpret_cast<u32x2*>(Al + o) = lo;
    }
#pragma unroll
    for (int i = 0; i < B_IT; ++i) {
      const int t = tid + DB_T * i;
      float v[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float t = r.b[i][e];
        if constexpr (B_MASK) t = db_mask(t, r.m[i][e]);
        v[e] = ldexpf(t, eb);
      }
      u32x2 hi, lo;
      split4(v, &hi, &lo);
      const int o = quad_row(t, BN) * DB_LDH + quad_r(t, BN);
      *reinterpret_cast<u32x2*>(Bh + o) = hi;
      *reinterpret_cast<u32x2*>(Bl + o) = lo;
    }
  };

  f32x16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  const int frow = lane & 31, fh = lane >> 5;

  auto compute = [&](int buf) {
    const u16* Ah = db_smem + buf * STAGE + (wm * WM + frow) * DB_LDH + fh * 8;
    const u16* Al = Ah + BM * DB_LDH;
    const u16* Bh = db_smem + buf * STAGE + 2 * BM * DB_LDH + (wn * WN + frow) * DB_LDH + fh * 8;
    const u16* Bl = Bh + BN * DB_LDH;
#pragma unroll
    for (int ks = 0; ks < DB_BK / 16; ++ks) {
      f16x8 ah[TM], al[TM], bh[TN], bl[TN];
#pragma unroll
      for (int i = 0; i < TM; ++i) {
        ah[i] = *reinterpret_cast<const f16x8*>(Ah + i * 32 * DB_LDH + ks * 16);
        al[i] = *reinterpret_cast<const f16x8*>(Al + i * 32 * DB_LDH + ks * 16);
      }
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        bh[j] = *reinterpret_cast<const f16x8*>(Bh + j * 32 * DB_LDH + ks * 16);
        bl[j] = *reinterpret_cast<const f16x8*>(Bl + j * 32 * DB_LDH + ks * 16);
      }
      // small cross terms first, the dominant hi*hi term last
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al[i], bh[j], acc[i][j], 0, 0, 0);
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[i], bl[j], acc[i][j], 0, 0, 0);
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[i], bh[j], acc[i][j], 0, 0, 0);
    }
  };

  // step kt + 1 is requested from global memory while step kt is multiplied, then split into the other stage
  Regs regs;
  load_global(0, regs);
  store_lds(0, regs);
  __syncthreads();
  for (int kt = 0; kt < nk; ++kt) {
    const bool more = kt + 1 < nk;
    if (more) load_global(kt + 1, regs);
    compute(kt & 1);
    if (more) store_lds((kt + 1) & 1, regs);
    __syncthreads();
  }

  // accumulator element reg of a lane: row (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5), column lane & 31
  float* out = g.out + (int64_t)blockIdx.z * g.range_stride;
  const int back = -(ea + eb);
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      const int col = q0 + wn * WN + j * 32 + frow;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = p0 + wm * WM + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * fh;
        if (row < g.P && col < g.Q) out[(int64_t)row * g.ld_out + col] = ldexpf(acc[i][j][r], back);
      }
    }
}

// dW = the ranges' slabs added in index order
__global__ __launch_bounds__(DB_T) void db_fold_kernel(const float* __restrict__ slabs, int n_ranges, int n, float* __restrict__ dw) {
  for (int i = blockIdx.x * DB_T + threadIdx.x; i < n; i += gridDim.x * DB_T) {
    float s = slabs[i];
    for (int z = 1; z < n_ranges; ++z) s += slabs[(int64_t)z * n + i];
    dw[i] = s;
  }
}

template <int BN, bool TRANS>
static int db_launch_gemm(const DbGemm& g, int n_ranges, hipStream_t s) {
  constexpr int lds = 2 * (2 * DB_BM + 2 * BN) * DB_LDH * (int)sizeof(u16);
  auto kern = db_gemm_kernel<BN, TRANS>;
  static DeviceOnce once;
  XDET_TRY(ensure_dynamic_lds(once, reinterpret_cast<const void*>(kern), lds));
  hipLaunchKernelGGL(kern, dim3((unsigned)cdiv(g.P, DB_BM), (unsigned)cdiv(g.Q, BN), (unsigned)n_ranges), dim3(DB_T), lds, s, g);
  XDET_LAUNCH_CHECK();
  return XDET_OK;
}

static int db_vec(const float* p, int ld) { return p && (reinterpret_cast<uintptr_t>(p) & 15) == 0 && ld % 4 == 0; }

}  // namespace xdet

using namespace xdet;

extern "C" {

size_t xdet_dense_backward_workspace_bytes(int M, int K, int J) {
  if (M <= 0 || K <= 0 || J <= 0 || K > DB_MAX_DIM || J > DB_MAX_DIM || (int64_t)M * std::max(K, J) >= (1ll << 31)) return 0;
  return ws_measure(4, db_layout, db_plan(M, K, J), K, J);
}

int xdet_dense_backward(const float* x, int ld_x, const float* w, const float* y, int ld_y, const float* dy, int ld_dy, int M,
                        int K, int J, float* dx, int ld_dx, float* dw, float* db, void* workspace, void* stream) {
  XDET_REQUIRE(M > 0 && K > 0 && J > 0, "dense_backward: M, K and J must be positive");
  XDET_REQUIRE(K <= DB_MAX_DIM && J <= DB_MAX_DIM && (int64_t)M * std::max(K, J) < (1ll << 31),
               "dense_backward: K and J at most 4096, M * max(K, J) below 2^31");
  XDET_REQUIRE(ld_x >= K && ld_dy >= J && (!y || ld_y >= J) && (!dx || ld_dx >= K),
               "dense_backward: a row stride is below its matrix's width");
  XDET_REQUIRE(x && w && dy && dw && db, "dense_backward: NULL argument");
  XDET_REQUIRE(workspace, "dense_backward: NULL workspace");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const DbPlan pl = db_plan(M, K, J);
  const auto [ctl, partial, slabs] = ws_carve(workspace, 4, db_layout, pl, K, J);

  DbPre a{};
  a.x = x; a.w = w; a.y = y; a.dy = dy;
  a.ld_x = ld_x; a.ld_y = ld_y; a.ld_dy = ld_dy;
  a.M = M; a.K = K; a.J = J;
  a.rows_per_chunk = pl.rows_per_chunk;
  a.n_chunks = pl.n_chunks;
  a.jblocks = (int)cdiv(J, DB_T);
  a.x_blocks = (int)std::min<int64_t>(cdiv((int64_t)M * K, DB_T * 8), 1024);
  a.w_blocks = (int)std::min<int64_t>(cdiv((int64_t)K * J, DB_T * 8), 1024);
  a.ctl = ctl;
  a.partial = partial;
  XDET_HIP(hipMemsetAsync(ctl, 0, DB_CTL_WORDS * 4, s));
  hipLaunchKernelGGL(db_prepass_kernel, dim3((unsigned)(a.n_chunks * a.jblocks + a.x_blocks + a.w_blocks)), dim3(DB_T), 0, s, a);
  XDET_LAUNCH_CHECK();
  hipLaunchKernelGGL(db_final_kernel, dim3((unsigned)cdiv(J, DB_T)), dim3(DB_T), 0, s, partial, pl.n_chunks, J, ctl, db);
  XDET_LAUNCH_CHECK();

  if (dx) {   // C[m, k] = sum_j g[m, j] W[k, j]
    DbGemm g{};
    g.a = dy; g.ld_a = ld_dy; g.y = y; g.ld_y = ld_y;
    g.b = w; g.ld_b = J;
    g.P = M; g.Q = K; g.R = J;
    g.r_per_range = J;
    g.ctl = ctl; g.ea_slot = DB_EXP_G; g.eb_slot = DB_EXP_W;
    g.out = dx; g.ld_out = ld_dx; g.range_stride = 0;
    g.vec_a = db_vec(dy, ld_dy); g.vec_b = db_vec(w, J); g.vec_y = db_vec(y, ld_y);
    XDET_TRY(pl.bn_dx == 32 ? (db_launch_gemm<32, false>(g, 1, s)) : (db_launch_gemm<128, false>(g, 1, s)));
  }
  {           // C[k, j] = sum_m x[m, k] g[m, j]
    DbGemm g{};
    g.a = x; g.ld_a = ld_x;
    g.b = dy; g.ld_b = ld_dy; g.y = y; g.ld_y = ld_y;
    g.P = K; g.Q = J; g.R = M;
    g.r_per_range = pl.rows_per_range;
    g.ctl = ctl; g.ea_slot = DB_EXP_X; g.eb_slot = DB_EXP_G;
    g.out = pl.n_ranges > 1 ? slabs : dw; g.ld_out = J; g.range_stride = (int64_t)K * J;
    XDET_TRY(pl.bn_dw == 32 ? (db_launch_gemm<32, true>(g, pl.n_ranges, s)) : (db_launch_gemm<128, true>(g, pl.n_ranges, s)));
    if (pl.n_ranges > 1) {
      const int n = K * J;
      hipLaunchKernelGGL(db_fold_kernel, dim3((unsigned)std::min<int64_t>(cdiv(n, DB_T), 2048)), dim3(DB_T), 0, s, slabs,
                         pl.n_ranges, n, dw);
      XDET_LAUNCH_CHECK();
    }
  }
  return XDET_OK;
}

}  // extern "C"
