// The backward of a stride-1 'SAME' convolution y = act(conv(relu_in ? max(x, 0) : x, W) + b) on the gfx950 matrix pipe
// (xdet_conv_backward, include/xdet.h), NHWC, W as [kh, kw, C, J]:
//
//     g  = dy, or dy * (y > 0) behind a ReLU                                        [M = N H W, J]
//     dW[t, c, j] = sum_m xe[m + t, c] g[m, j]       xe = x or max(x, 0); m + t: pixel m shifted by tap t's offset, zero
//     dx[m, c]    = sum_t sum_j g[m - t, j] W[t, c, j]    (and 0 where relu_in and not x > 0)      outside the image
//     db = column sums of g
//
// Both products are implicit GEMMs on the tile of backward_gemm.h (f16x3 on v_mfma_f32_32x32x16_f16, every operand under a
// power-of-two scale of its own found by dense_backward.hip's pre-pass): the patch matrix [M, kh kw C] is never written,
// the loaders below fetch its elements from x -- or g's shifted rows -- as the steps need them.
//
//   cb_dw_kernel<BN>  C[k, j] = sum_m A(k, m) g[m, j], k = t C + c a column of the patch matrix.  The tile's quad mapping is
//                     the dense dW's (lanes along the operand's row in memory), so a thread keeps ONE k for the whole kernel:
//                     its tap, channel and pixel shift are decoded once, and neighbouring threads of a tile that straddles
//                     two taps simply carry different shifts.  Per quad the first pixel m is decoded into (h, w) by two
//                     multiply-high divisions and stepped from there; a shifted pixel outside its image row or image is fed
//                     as zero, never read.  The sum over m is cut into dense_backward's row ranges and folded in index order.
//   cb_dx_kernel<BN>  C[m, c] = sum_(t, j) g[m - t, j] W[t, c, j]: one K pipeline over kh kw ceil(J / 32) steps, a step
//                     inside one tap (J's ragged tail is zero-fed), so the shift is uniform per step; a thread keeps its
//                     four rows m, decoded once.  Both operands have j contiguous.
// No float atomics: the same call gives the same bits.
#include "backward_gemm.h"

namespace xdet {

struct CbGemm {
  const float *x, *w, *y, *dy;
  int ld_x, ld_y, ld_dy;
  int M, H, W, C, J, kh, kw, relu_in;
  CbDiv by_w, by_h, by_c, by_kw, by_jsteps;
  int jsteps;                   // dx: reduction steps per tap, ceil(J / 32)
  int r_per_range;              // dW: pixels per blockIdx.z
  const unsigned* ctl;
  float* out;
  int ld_out;
  int64_t range_stride;         // dW: floats between the outputs of two ranges
  int vec_w, vec_dy, vec_y;     // dx: rows may be read as aligned float4
};

template <int BN>
__global__ __launch_bounds__(DB_T) void cb_dw_kernel(CbGemm g) {
  using T = DbTile<BN>;
  constexpr int BM = T::BM, A_IT = T::A_IT, B_IT = T::B_IT;

  extern __shared__ __attribute__((aligned(16))) u16 cb_smem[];

  const int tid = threadIdx.x;
  const int p0 = blockIdx.x * BM, q0 = blockIdx.y * BN;
  const int P = g.kh * g.kw * g.C;
  const int r0 = blockIdx.z * g.r_per_range, r1 = min(g.M, r0 + g.r_per_range);
  const int nk = (r1 - r0 + DB_BK - 1) / DB_BK;
  const int ex = (int)g.ctl[DB_EXP_X], eg = (int)g.ctl[DB_EXP_G];

  // A: the thread's column of the patch matrix (db_quad_row<true> does not depend on the quad), B: its column of g
  const int k = p0 + (tid & (BM - 1)), j = q0 + (tid & (BN - 1));
  const bool k_ok = k < P, j_ok = j < g.J;
  const int tap = cb_quot(k, g.by_c), c = k - tap * g.C;
  const int ta = cb_quot(tap, g.by_kw);
  const int da = ta - g.kh / 2, dc = tap - ta * g.kw - g.kw / 2;      // the tap's row and column offset
  const int64_t a_off = ((int64_t)da * g.W + dc) * g.ld_x + c;        // from pixel m's row of x to the element read for it

  struct Regs {
    float a[A_IT][4], b[B_IT][4], m[B_IT][4];
  };

  auto load_global = [&](int kt, Regs& r) {
    const int rk = r0 + kt * DB_BK;
#pragma unroll
    for (int i = 0; i < A_IT; ++i) {
      const int m0 = rk + db_quad_r<true>(tid + DB_T * i, BM);
#pragma unroll
      for (int e = 0; e < 4; ++e) r.a[i][e] = 0.f;
      if (k_ok && m0 < r1) {
        const int row = cb_quot(m0, g.by_w);
        int w = m0 - row * g.W, h = row - cb_quot(row, g.by_h) * g.H;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          if (m0 + e < r1 && (unsigned)(h + da) < (unsigned)g.H && (unsigned)(w + dc) < (unsigned)g.W) {
            const float v = g.x[(int64_t)(m0 + e) * g.ld_x + a_off];
            r.a[i][e] = g.relu_in ? db_mask(v, v) : v;
          }
          if (++w == g.W) {
            w = 0;
            if (++h == g.H) h = 0;
          }
        }
      }
    }
#pragma unroll
    for (int i = 0; i < B_IT; ++i) {
      const int m0 = rk + db_quad_r<true>(tid + DB_T * i, BN);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        r.b[i][e] = r.m[i][e] = 0.f;
        if (j_ok && m0 + e < r1) {
          r.b[i][e] = g.dy[(int64_t)(m0 + e) * g.ld_dy + j];
          if (g.y) r.m[i][e] = g.y[(int64_t)(m0 + e) * g.ld_y + j];
        }
      }
    }
  };
  auto store_lds = [&](int buf, const Regs& r) {
    u16* Ah = cb_smem + buf * T::STAGE;
    u16* Bh = Ah + 2 * BM * DB_LDH;
    db_store_quads<BM, A_IT, true>(Ah, Ah + BM * DB_LDH, r.a, nullptr, ex);
    db_store_quads<BN, B_IT, true>(Bh, Bh + BN * DB_LDH, r.b, g.y ? r.m : nullptr, eg);
  };

  f32x16 acc[T::TM][T::TN];
  db_zero<BN>(acc);

  Regs regs;
  load_global(0, regs);
  store_lds(0, regs);
  __syncthreads();
  for (int kt = 0; kt < nk; ++kt) {
    const bool more = kt + 1 < nk;
    if (more) load_global(kt + 1, regs);
    db_compute<BN>(cb_smem + (kt & 1) * T::STAGE, acc);
    if (more) store_lds((kt + 1) & 1, regs);
    __syncthreads();
  }

  float* out = g.out + (int64_t)blockIdx.z * g.range_stride;
  const int back = -(ex + eg);
  db_for_each_output<BN>(acc, [&](int row, int col, float v) {
    if (p0 + row < P && q0 + col < g.J) out[(int64_t)(p0 + row) * g.J + q0 + col] = ldexpf(v, back);
  });
}

template <int BN>
__global__ __launch_bounds__(DB_T) void cb_dx_kernel(CbGemm g) {
  using T = DbTile<BN>;
  constexpr int BM = T::BM, A_IT = T::A_IT, B_IT = T::B_IT;

  extern __shared__ __attribute__((aligned(16))) u16 cb_smem[];

  const int tid = threadIdx.x;
  const int p0 = blockIdx.x * BM, q0 = blockIdx.y * BN;
  const int nk = g.kh * g.kw * g.jsteps;
  const int eg = (int)g.ctl[DB_EXP_G], ew = (int)g.ctl[DB_EXP_W];

  // the thread's rows (db_quad_row<false>: tid / 8 + 32 i) and where they lie in their image; a row past M lies nowhere
  int mh[A_IT], mw[A_IT];
#pragma unroll
  for (int i = 0; i < A_IT; ++i) {
    const int m = p0 + (tid >> 3) + 32 * i, row = cb_quot(m, g.by_w);
    mw[i] = m - row * g.W;
    mh[i] = m < g.M ? row - cb_quot(row, g.by_h) * g.H : -(1 << 30);
  }
  const int jq = db_quad_r<false>(tid, BM);

  struct Regs {
    float a[A_IT][4], b[B_IT][4], m[A_IT][4];
  };

  auto load_global = [&](int kt, Regs& r) {
    const int tap = cb_quot(kt, g.by_jsteps), j = (kt - tap * g.jsteps) * DB_BK + jq;
    const int ta = cb_quot(tap, g.by_kw);
    const int da = ta - g.kh / 2, dc = tap - ta * g.kw - g.kw / 2;
    const int shift = da * g.W + dc;      // input pixel m fed output pixel m - shift through this tap: dx[m] gathers g[m - shift]
#pragma unroll
    for (int i = 0; i < A_IT; ++i) {
#pragma unroll
      for (int e = 0; e < 4; ++e) r.a[i][e] = r.m[i][e] = 0.f;
      if (j < g.J && (unsigned)(mh[i] - da) < (unsigned)g.H && (unsigned)(mw[i] - dc) < (unsigned)g.W) {
        const int64_t src = p0 + (tid >> 3) + 32 * i - shift;
        cb_load_row4(g.dy + src * g.ld_dy + j, g.J - j, g.vec_dy, r.a[i]);
        if (g.y) cb_load_row4(g.y + src * g.ld_y + j, g.J - j, g.vec_y, r.m[i]);
      }
    }
#pragma unroll
    for (int i = 0; i < B_IT; ++i) {
      const int c = q0 + (tid >> 3) + 32 * i;
#pragma unroll
      for (int e = 0; e < 4; ++e) r.b[i][e] = 0.f;
      if (j < g.J && c < g.C) cb_load_row4(g.w + ((int64_t)tap * g.C + c) * g.J + j, g.J - j, g.vec_w, r.b[i]);
    }
  };
  auto store_lds = [&](int buf, const Regs& r) {
    u16* Ah = cb_smem + buf * T::STAGE;
    u16* Bh = Ah + 2 * BM * DB_LDH;
    db_store_quads<BM, A_IT, false>(Ah, Ah + BM * DB_LDH, r.a, g.y ? r.m : nullptr, eg);
    db_store_quads<BN, B_IT, false>(Bh, Bh + BN * DB_LDH, r.b, nullptr, ew);
  };

  f32x16 acc[T::TM][T::TN];
  db_zero<BN>(acc);

  Regs regs;
  load_global(0, regs);
  store_lds(0, regs);
  __syncthreads();
  for (int kt = 0; kt < nk; ++kt) {
    const bool more = kt + 1 < nk;
    if (more) load_global(kt + 1, regs);
    db_compute<BN>(cb_smem + (kt & 1) * T::STAGE, acc);
    if (more) store_lds((kt + 1) & 1, regs);
    __syncthreads();
  }

  const int back = -(eg + ew);
  db_for_each_output<BN>(acc, [&](int row, int col, float v) {
    const int m = p0 + row, c = q0 + col;
    if (m < g.M && c < g.C) {
      v = ldexpf(v, back);
      if (g.relu_in) v = db_mask(v, g.x[(int64_t)m * g.ld_x + c]);
      g.out[(int64_t)m * g.ld_out + c] = v;
    }
  });
}

template <int BN, bool DW>
static int cb_launch(const CbGemm& g, dim3 grid, hipStream_t s) {
  constexpr int lds = DbTile<BN>::LDS_BYTES;
  auto kern = DW ? cb_dw_kernel<BN> : cb_dx_kernel<BN>;
  static DeviceOnce once;
  XDET_TRY(ensure_dynamic_lds(once, reinterpret_cast<const void*>(kern), lds));
  hipLaunchKernelGGL(kern, grid, dim3(DB_T), lds, s, g);
  XDET_LAUNCH_CHECK();
  return XDET_OK;
}

// inside the limits of include/xdet.h; M = N H W
static bool cb_sizes_ok(int N, int H, int W, int C, int J, int kh, int kw, int64_t* M) {
  if (N <= 0 || H <= 0 || W <= 0 || C <= 0 || J <= 0 || kh <= 0 || kw <= 0) return false;
  if (kh % 2 == 0 || kw % 2 == 0 || kh > CB_MAX_TAPS || kw > CB_MAX_TAPS || C > DB_MAX_DIM || J > DB_MAX_DIM) return false;
  *M = (int64_t)N * H * W;
  return *M * std::max(C, J) < (1ll << 31);
}

}  // namespace xdet

using namespace xdet;

extern "C" {

size_t xdet_conv_backward_workspace_bytes(int N, int H, int W, int C, int J, int kh, int kw) {
  int64_t M;
  if (!cb_sizes_ok(N, H, W, C, J, kh, kw, &M)) return 0;
  return ws_measure(4, db_layout, db_sums((int)M, kh * kw * C, J), kh * kw * C, J);
}

int xdet_conv_backward(const float* x, int ld_x, const float* w, const float* y, int ld_y, const float* dy, int ld_dy, int N,
                       int H, int W, int C, int J, int kh, int kw, int relu_in, float* dx, int ld_dx, float* dw, float* db,
                       void* workspace, void* stream) {
  int64_t M64 = 0;
  XDET_REQUIRE(cb_sizes_ok(N, H, W, C, J, kh, kw, &M64),
               "conv_backward: N, H, W, C, J positive, kh and kw odd and at most 15, C and J at most 4096, N*H*W * max(C, J) "
               "below 2^31");
  XDET_REQUIRE(ld_x >= C && ld_dy >= J && (!y || ld_y >= J) && (!dx || ld_dx >= C),
               "conv_backward: a pixel stride is below its tensor's channel count");
  XDET_REQUIRE(M64 * std::max(std::max(ld_x, ld_dy), std::max(y ? ld_y : 0, dx ? ld_dx : 0)) < (1ll << 31),
               "conv_backward: N*H*W * the largest pixel stride must stay below 2^31");
  XDET_REQUIRE(x && w && dy && dw && db, "conv_backward: NULL argument");
  XDET_REQUIRE(workspace, "conv_backward: NULL workspace");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int M = (int)M64, KR = kh * kw * C;
  const DbSums pl = db_sums(M, KR, J);
  const auto [ctl, partial, slabs] = ws_carve(workspace, 4, db_layout, pl, KR, J);

  DbPre a{};
  a.x = x; a.w = w; a.y = y; a.dy = dy;
  a.ld_x = ld_x; a.ld_y = ld_y; a.ld_dy = ld_dy;
  a.M = M; a.x_cols = C; a.w_rows = KR; a.J = J; a.relu_x = relu_in != 0;
  a.rows_per_chunk = pl.rows_per_chunk;
  a.n_chunks = pl.n_chunks;
  a.ctl = ctl;
  a.partial = partial;
  XDET_TRY(db_launch_prepass(a, db, s));

  CbGemm g{};
  g.x = x; g.w = w; g.y = y; g.dy = dy;
  g.ld_x = ld_x; g.ld_y = ld_y; g.ld_dy = ld_dy;
  g.M = M; g.H = H; g.W = W; g.C = C; g.J = J; g.kh = kh; g.kw = kw; g.relu_in = relu_in != 0;
  g.jsteps = (int)cdiv(J, DB_BK);
  g.by_w = cb_div(W); g.by_h = cb_div(H); g.by_c = cb_div(C); g.by_kw = cb_div(kw); g.by_jsteps = cb_div(g.jsteps);
  g.ctl = ctl;
  if (dx) {
    g.out = dx; g.ld_out = ld_dx;
    g.vec_w = db_vec(w, J); g.vec_dy = db_vec(dy, ld_dy); g.vec_y = db_vec(y, ld_y);
    const unsigned mt = (unsigned)cdiv(M, DB_BM);
    XDET_TRY(C <= 32 ? (cb_launch<32, false>(g, dim3(mt, 1, 1), s))
                     : (cb_launch<128, false>(g, dim3(mt, (unsigned)cdiv(C, 128), 1), s)));
  }
  g.r_per_range = pl.rows_per_range;
  g.out = pl.n_ranges > 1 ? slabs : dw; g.range_stride = (int64_t)KR * J;
  const dim3 grid((unsigned)cdiv(KR, DB_BM), (unsigned)cdiv(J, pl.bn_dw), (unsigned)pl.n_ranges);
  XDET_TRY(pl.bn_dw == 32 ? (cb_launch<32, true>(g, grid, s)) : (cb_launch<128, true>(g, grid, s)));
  if (pl.n_ranges > 1) XDET_TRY(db_launch_fold(slabs, pl.n_ranges, (int64_t)KR * J, dw, s));
  return XDET_OK;
}

}  // extern "C"
