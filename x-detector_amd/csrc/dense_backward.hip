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
//                       only (db_sums, backward_gemm.h); a range writes its slab of the workspace
//   db_fold_kernel      dW = the slabs added in index order (skipped for a single range, which writes dW itself)
// No float atomics anywhere: the same call gives the same bits.
//
// The GEMM kernel: a 128 x BN tile (BN 128: 2 x 2 waves of 64 x 64; BN 32 for an output of at most 32 columns: 4 x 1 waves
// of 32 x 32), reduction steps of 32.  Operands are read as f32 from global memory one step ahead into registers (g: dy and
// y, the mask and the scale are applied when the step is stored), split in registers and staged in LDS as hi / lo rows of
// 32 + 8 halves (80 B: every MFMA operand is one conflict-free ds_read_b128, conv_mfma_split.hip's layout), two stages, one
// barrier per step.  Ragged edges in all three dimensions are predicated loads that feed zeros: nothing is read at or beyond
// an operand's width or row count, so padding columns may hold anything.
#include "backward_gemm.h"

namespace xdet {

// The serial sums below (db's chunks, db itself, the fold) add in index order, one thread per column: only the loads can
// overlap, so each loop asks for DB_AHEAD of them before it adds them in the same order as a plain loop would -- the same
// bits at an eighth of the memory latency (a stem-sized call, 1023 chunks: db_final_kernel 224 -> 37 us, the fold of 510
// slabs 119 -> 24 us).
constexpr int DB_AHEAD = 8;

// DbPre and how its workgroups are dealt out: n_chunks * jblocks for g and db, then x_blocks, then w_blocks
struct DbPreGrid {
  DbPre a;
  int jblocks, x_blocks, w_blocks;
};

__global__ __launch_bounds__(DB_T) void db_prepass_kernel(DbPreGrid p) {
  const DbPre& a = p.a;
  const int tid = threadIdx.x;
  int b = blockIdx.x;
  unsigned mx = 0;
  const int g_blocks = a.n_chunks * p.jblocks;
  if (b < g_blocks) {
    const int c = b / p.jblocks, j = (b - c * p.jblocks) * DB_T + tid;
    if (j < a.J) {
      const int64_t m0 = (int64_t)c * a.rows_per_chunk, m1 = min((int64_t)a.M, m0 + a.rows_per_chunk);
      float s = 0.f;
      int64_t m = m0;
      for (; m + DB_AHEAD <= m1; m += DB_AHEAD) {      // the loads of DB_AHEAD rows in flight, the sum in row order as ever
        float d[DB_AHEAD], v[DB_AHEAD];
#pragma unroll
        for (int u = 0; u < DB_AHEAD; ++u) {
          d[u] = a.dy[(m + u) * a.ld_dy + j];
          v[u] = a.y ? a.y[(m + u) * a.ld_y + j] : 1.f;
        }
#pragma unroll
        for (int u = 0; u < DB_AHEAD; ++u) {
          const float g = db_mask(d[u], v[u]);
          s += g;
          mx = max(mx, db_abs_bits(g));
        }
      }
      for (; m < m1; ++m) {
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
  const bool is_x = b < p.x_blocks;
  if (!is_x) b -= p.x_blocks;
  if (is_x) {
    const unsigned width = a.x_cols, n = (unsigned)(a.x_rows ? a.x_rows : a.M) * width, step = (unsigned)p.x_blocks * DB_T;      // n < 2^31
    for (unsigned i = (unsigned)b * DB_T + tid; i < n; i += step) {
      const unsigned row = i / width, col = i - row * width;
      if (a.x_w) {                                                             // a pixel under no window is not read
        const unsigned line = row / (unsigned)a.x_w;
        if (row - line * a.x_w >= (unsigned)a.x_wc || line % (unsigned)a.x_h >= (unsigned)a.x_hc) continue;
      }
      const float v = a.x[(int64_t)row * a.ld_x + col];
      mx = max(mx, db_abs_bits(a.relu_x ? db_mask(v, v) : v));
    }
  } else {                                                                   // w is dense; a conv's may pass 2^32 elements
    const int64_t n = (int64_t)a.w_rows * a.J, step = (int64_t)p.w_blocks * DB_T;
    for (int64_t i = (int64_t)b * DB_T + tid; i < n; i += step) mx = max(mx, db_abs_bits(a.w[i]));
  }
  db_block_max(mx, a.ctl + (is_x ? DB_MAX_X : DB_MAX_W));
}

__global__ __launch_bounds__(DB_T) void db_final_kernel(const float* __restrict__ partial, int n_chunks, int J, unsigned* ctl,
                                                        float* __restrict__ db) {
  const int j = blockIdx.x * DB_T + threadIdx.x;
  if (blockIdx.x == 0 && threadIdx.x < 3) ctl[DB_EXP_X + threadIdx.x] = (unsigned)db_scale_exp(ctl[DB_MAX_X + threadIdx.x]);
  if (j >= J) return;
  float s = 0.f;
  int c = 0;
  for (; c + DB_AHEAD <= n_chunks; c += DB_AHEAD) {
    float v[DB_AHEAD];
#pragma unroll
    for (int u = 0; u < DB_AHEAD; ++u) v[u] = partial[(int64_t)(c + u) * J + j];
#pragma unroll
    for (int u = 0; u < DB_AHEAD; ++u) s += v[u];
  }
  for (; c < n_chunks; ++c) s += partial[(int64_t)c * J + j];
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
  using T = DbTile<BN>;
  constexpr int BM = T::BM, A_IT = T::A_IT, B_IT = T::B_IT;
  constexpr bool A_MASK = !TRANS, B_MASK = TRANS;

  extern __shared__ __attribute__((aligned(16))) u16 db_smem[];

  const int tid = threadIdx.x;
  const int p0 = blockIdx.x * BM, q0 = blockIdx.y * BN;
  const int r0 = blockIdx.z * g.r_per_range, r1 = min(g.R, r0 + g.r_per_range);
  const int nk = (r1 - r0 + DB_BK - 1) / DB_BK;
  const int ea = (int)g.ctl[g.ea_slot], eb = (int)g.ctl[g.eb_slot];

  struct {
    float a[A_IT][4], b[B_IT][4], m[A_MASK ? A_IT : B_IT][4];
  } r;      // the step in flight

  auto load_global = [&](int kt) {
    const int rk = r0 + kt * DB_BK;
#pragma unroll
    for (int i = 0; i < A_IT; ++i) {
      const int t = tid + DB_T * i, row = p0 + db_quad_row<TRANS>(t, BM), rr = rk + db_quad_r<TRANS>(t, BM);
      db_load4<TRANS>(g.a, g.ld_a, row, rr, g.P, r1, g.vec_a, r.a[i]);
      if constexpr (A_MASK)
        if (g.y) db_load4<TRANS>(g.y, g.ld_y, row, rr, g.P, r1, g.vec_y, r.m[i]);
    }
#pragma unroll
    for (int i = 0; i < B_IT; ++i) {
      const int t = tid + DB_T * i, row = q0 + db_quad_row<TRANS>(t, BN), rr = rk + db_quad_r<TRANS>(t, BN);
      db_load4<TRANS>(g.b, g.ld_b, row, rr, g.Q, r1, g.vec_b, r.b[i]);
      if constexpr (B_MASK)
        if (g.y) db_load4<TRANS>(g.y, g.ld_y, row, rr, g.Q, r1, g.vec_y, r.m[i]);
    }
  };
  auto store_lds = [&](int buf) {
    u16* Ah = db_smem + buf * T::STAGE;
    u16* Bh = Ah + 2 * BM * DB_LDH;
    db_store_quads<BM, A_IT, TRANS>(Ah, Ah + BM * DB_LDH, r.a, A_MASK && g.y ? r.m : nullptr, ea);
    db_store_quads<BN, B_IT, TRANS>(Bh, Bh + BN * DB_LDH, r.b, B_MASK && g.y ? r.m : nullptr, eb);
  };

  f32x16 acc[T::TM][T::TN];
  db_zero<BN>(acc);

  db_pipeline(nk, load_global, store_lds, [&](int buf) { db_compute<BN>(db_smem + buf * T::STAGE, acc); });

  float* out = g.out + (int64_t)blockIdx.z * g.range_stride;
  const int back = -(ea + eb);
  db_for_each_output<BN>(acc, [&](int row, int col, float v) {
    if (p0 + row < g.P && q0 + col < g.Q) out[(int64_t)(p0 + row) * g.ld_out + q0 + col] = ldexpf(v, back);
  });
}

// dW = the ranges' slabs added in index order
__global__ __launch_bounds__(DB_T) void db_fold_kernel(const float* __restrict__ slabs, int n_ranges, int64_t n, float* __restrict__ dw) {
  for (int64_t i = blockIdx.x * DB_T + threadIdx.x; i < n; i += gridDim.x * DB_T) {
    float s = slabs[i];
    int z = 1;
    for (; z + DB_AHEAD <= n_ranges; z += DB_AHEAD) {
      float v[DB_AHEAD];
#pragma unroll
      for (int u = 0; u < DB_AHEAD; ++u) v[u] = slabs[(z + u) * n + i];
#pragma unroll
      for (int u = 0; u < DB_AHEAD; ++u) s += v[u];
    }
    for (; z < n_ranges; ++z) s += slabs[z * n + i];
    dw[i] = s;
  }
}

template <int BN, bool TRANS>
static int db_launch_gemm(const DbGemm& g, int n_ranges, hipStream_t s) {
  constexpr int lds = DbTile<BN>::LDS_BYTES;
  auto kern = db_gemm_kernel<BN, TRANS>;
  static DeviceOnce once;
  XDET_TRY(ensure_dynamic_lds(once, reinterpret_cast<const void*>(kern), lds));
  hipLaunchKernelGGL(kern, dim3((unsigned)cdiv(g.P, DB_BM), (unsigned)cdiv(g.Q, BN), (unsigned)n_ranges), dim3(DB_T), lds, s, g);
  XDET_LAUNCH_CHECK();
  return XDET_OK;
}

int db_launch_prepass(const DbPre& a, float* db, hipStream_t s) {
  DbPreGrid p{a, (int)cdiv(a.J, DB_T), (int)std::min<int64_t>(cdiv((int64_t)(a.x_rows ? a.x_rows : a.M) * a.x_cols, DB_T * 8), 1024),
              (int)std::min<int64_t>(cdiv((int64_t)a.w_rows * a.J, DB_T * 8), 1024)};
  XDET_HIP(hipMemsetAsync(a.ctl, 0, DB_CTL_WORDS * 4, s));
  hipLaunchKernelGGL(db_prepass_kernel, dim3((unsigned)(a.n_chunks * p.jblocks + p.x_blocks + p.w_blocks)), dim3(DB_T), 0, s, p);
  XDET_LAUNCH_CHECK();
  hipLaunchKernelGGL(db_final_kernel, dim3((unsigned)cdiv(a.J, DB_T)), dim3(DB_T), 0, s, a.partial, a.n_chunks, a.J, a.ctl, db);
  XDET_LAUNCH_CHECK();
  return XDET_OK;
}

int db_launch_fold(const float* slabs, int n_ranges, int64_t n, float* dw, hipStream_t s) {
  hipLaunchKernelGGL(db_fold_kernel, dim3((unsigned)std::min<int64_t>(cdiv(n, DB_T), 2048)), dim3(DB_T), 0, s, slabs, n_ranges,
                     n, dw);
  XDET_LAUNCH_CHECK();
  return XDET_OK;
}

}  // namespace xdet

using namespace xdet;

extern "C" {

size_t xdet_dense_backward_workspace_bytes(int M, int K, int J) {
  if (M <= 0 || K <= 0 || J <= 0 || K > DB_MAX_DIM || J > DB_MAX_DIM || (int64_t)M * std::max(K, J) >= (1ll << 31)) return 0;
  return ws_measure(4, db_layout, db_sums(M, K, J), K, J);
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
  const DbSums pl = db_sums(M, K, J);
  const auto [ctl, partial, slabs] = ws_carve(workspace, 4, db_layout, pl, K, J);

  DbPre a{};
  a.x = x; a.w = w; a.y = y; a.dy = dy;
  a.ld_x = ld_x; a.ld_y = ld_y; a.ld_dy = ld_dy;
  a.M = M; a.x_cols = K; a.w_rows = K; a.J = J;
  a.rows_per_chunk = pl.rows_per_chunk;
  a.n_chunks = pl.n_chunks;
  a.ctl = ctl;
  a.partial = partial;
  XDET_TRY(db_launch_prepass(a, db, s));

  if (dx) {   // C[m, k] = sum_j g[m, j] W[k, j]
    DbGemm g{};
    g.a = dy; g.ld_a = ld_dy; g.y = y; g.ld_y = ld_y;
    g.b = w; g.ld_b = J;
    g.P = M; g.Q = K; g.R = J;
    g.r_per_range = J;
    g.ctl = ctl; g.ea_slot = DB_EXP_G; g.eb_slot = DB_EXP_W;
    g.out = dx; g.ld_out = ld_dx; g.range_stride = 0;
    g.vec_a = db_vec(dy, ld_dy); g.vec_b = db_vec(w, J); g.vec_y = db_vec(y, ld_y);
    XDET_TRY(K <= 32 ? (db_launch_gemm<32, false>(g, 1, s)) : (db_launch_gemm<128, false>(g, 1, s)));
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
    if (pl.n_ranges > 1) XDET_TRY(db_launch_fold(slabs, pl.n_ranges, (int64_t)K * J, dw, s));
  }
  return XDET_OK;
}

}  // extern "C"
