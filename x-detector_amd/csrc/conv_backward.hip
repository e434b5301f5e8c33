// The backward of a convolution y = act(conv(relu_in ? max(x, 0) : x, W) + b) at stride 1 or 2, 'VALID' or TensorFlow's 'SAME',
// on the gfx950 matrix pipe, NHWC, W as [kh, kw, C, J]: xdet_conv_backward_strided (include/xdet.h), and xdet_conv_backward,
// its stride-1 'SAME' door.  Two index spaces: x and dx live on the input map [N, H, W], y, dy and g on the output map
// [N, Ho, Wo]; output pixel (oh, ow) read input pixel (oh s + a - pt, ow s + b - pl) through tap (a, b), pt / pl the padding
// in front.
//
//     g  = dy, or dy * (y > 0) behind a ReLU                                                    [Mo = N Ho Wo, J]
//     dW[a, b, c, j] = sum_(n, oh, ow) xe[n, oh s + a - pt, ow s + b - pl, c] g[n, oh, ow, j]      xe = x or max(x, 0)
//     dx[n, h, w, c] = sum_(a, b) sum_j g[n, (h + pt - a) / s, (w + pl - b) / s, j] W[a, b, c, j]    over the taps whose two
//     db = column sums of g                                            quotients are integers inside the output map
//
// Both products are implicit GEMMs on the tile of backward_gemm.h (f16x3 on v_mfma_f32_32x32x16_f16, every operand under a
// power-of-two scale of its own found by dense_backward.hip's pre-pass): the patch matrix [Mo, kh kw C] is never written,
// the loaders below fetch its elements from x -- or g's rows -- as the steps need them; what lies outside a map is fed as
// zero and never read.
//
//   cb_dw_kernel<BN>  C[k, j] = sum_mo A(k, mo) g[mo, j], k = t C + c a column of the patch matrix.  The tile's quad mapping
//                     is the dense dW's (lanes along the operand's row in memory), so a thread keeps ONE k -- its tap and
//                     channel -- for the whole kernel, and neighbouring threads of a tile that straddles two taps simply
//                     carry different offsets.  Per quad the first output pixel is decoded into (n, oh, ow) by two
//                     multiply-high divisions and stepped from there, and the input pixel follows from it.  The sum over mo
//                     is cut into dense_backward's row ranges (over Mo) and folded in index order.
//   cb_dw_narrow_kernel   the same product on ONE 32 x 32 tile for kh kw C <= 32 and J <= 32 (block1_conv1), the four waves
//                     splitting each 128-pixel step instead of the tile (see there).  xdet_conv_backward_strided only.
//   cb_dx_kernel<BN, SAME>  C[m, c] = sum_(t, j) g[src_t(m), j] W[t, c, j] over the INPUT pixels m: one K pipeline over
//                     kh kw ceil(J / 32) steps, a step inside one tap (J's ragged tail is zero-fed).  A thread keeps its four
//                     rows m decoded as (n, h, w); a row feeds a step only if (h + pt - a, w + pl - b) is a multiple of the
//                     stride inside the output map -- at stride 2 the predicate form: three of four rows of a step feed
//                     zeros.  An input pixel under no window ('VALID' at stride 2 with an even H or W) gets +0 and its x is
//                     not read.  Both operands have j contiguous.
// No float atomics: the same call gives the same bits.
#include "backward_gemm.h"

namespace xdet {

struct CbGemm {
  const float *x, *w, *y, *dy;
  int ld_x, ld_y, ld_dy;
  int M, Mo, H, W, Ho, Wo, C, J, kh, kw, relu_in;
  int s, pt, pl;                // stride, padding in front
  int hc, wc;                   // input rows / columns below these lie under a window
  CbDiv by_w, by_h, by_wo, by_ho, by_c, by_kw, by_jsteps;
  int jsteps;                   // dx: reduction steps per tap, ceil(J / 32)
  int r_per_range;              // dW: output pixels per blockIdx.z
  const unsigned* ctl;
  float* out;
  int ld_out;
  int64_t range_stride;         // dW: floats between the outputs of two ranges
  int vec_w, vec_dy, vec_y;     // dx: rows may be read as aligned float4
};

// dW's A operand: column k = t C + c of the patch matrix at the four output pixels m0 .. m0 + 3 below r1 (k < P, m0 < r1)
__device__ __forceinline__ void cb_load_patch4(const CbGemm& g, int m0, int r1, int da, int dc, int c, float (&v)[4]) {
  const int row = cb_quot(m0, g.by_wo);
  const int n = cb_quot(row, g.by_ho);
  int ow = m0 - row * g.Wo, oh = row - n * g.Ho;
  // the input pixel (ih, iw) and x's element under it are carried next to (oh, ow): s pixels per column, the rest of the
  // input row where the column wraps, the rest of the image where the row wraps (outside the image `at` is not an address)
  int ih = oh * g.s + da, iw = ow * g.s + dc;
  int64_t at = ((int64_t)(n * g.H + ih) * g.W + iw) * g.ld_x + c;
  const int64_t per_col = (int64_t)g.s * g.ld_x, per_row = (int64_t)g.s * (g.W - g.Wo) * g.ld_x;
  const int64_t per_image = (int64_t)(g.H - g.Ho * g.s) * g.W * g.ld_x;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    if (m0 + e < r1 && (unsigned)ih < (unsigned)g.H && (unsigned)iw < (unsigned)g.W) {
      const float x = g.x[at];
      v[e] = g.relu_in ? db_mask(x, x) : x;
    }
    iw += g.s, at += per_col;
    if (++ow == g.Wo) {
      ow = 0, iw = dc, ih += g.s, at += per_row;
      if (++oh == g.Ho) oh = 0, ih = da, at += per_image;
    }
  }
}

template <int BN>
__global__ __launch_bounds__(DB_T) void cb_dw_kernel(CbGemm g) {
  using T = DbTile<BN>;
  constexpr int BM = T::BM, A_IT = T::A_IT, B_IT = T::B_IT;

  extern __shared__ __attribute__((aligned(16))) u16 cb_smem[];

  const int tid = threadIdx.x;
  const int p0 = blockIdx.x * BM, q0 = blockIdx.y * BN;
  const int P = g.kh * g.kw * g.C;
  const int r0 = blockIdx.z * g.r_per_range, r1 = min(g.Mo, r0 + g.r_per_range);
  const int nk = (r1 - r0 + DB_BK - 1) / DB_BK;
  const int ex = (int)g.ctl[DB_EXP_X], eg = (int)g.ctl[DB_EXP_G];

  // A: the thread's column of the patch matrix (db_quad_row<true> does not depend on the quad), B: its column of g
  const int k = p0 + (tid & (BM - 1)), j = q0 + (tid & (BN - 1));
  const bool k_ok = k < P, j_ok = j < g.J;
  const int tap = cb_quot(k, g.by_c), c = k - tap * g.C;
  const int ta = cb_quot(tap, g.by_kw);
  const int da = ta - g.pt, dc = tap - ta * g.kw - g.pl;      // output pixel (oh, ow) reads input pixel (oh s + da, ow s + dc)

  struct {
    float a[A_IT][4], b[B_IT][4], m[B_IT][4];
  } r;      // the step in flight

  auto load_global = [&](int kt) {
    const int rk = r0 + kt * DB_BK;
#pragma unroll
    for (int i = 0; i < A_IT; ++i) {
      const int m0 = rk + db_quad_r<true>(tid + DB_T * i, BM);
#pragma unroll
      for (int e = 0; e < 4; ++e) r.a[i][e] = 0.f;
      if (k_ok && m0 < r1) cb_load_patch4(g, m0, r1, da, dc, c, r.a[i]);
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
  auto store_lds = [&](int buf) {
    u16* Ah = cb_smem + buf * T::STAGE;
    u16* Bh = Ah + 2 * BM * DB_LDH;
    db_store_quads<BM, A_IT, true>(Ah, Ah + BM * DB_LDH, r.a, nullptr, ex);
    db_store_quads<BN, B_IT, true>(Bh, Bh + BN * DB_LDH, r.b, g.y ? r.m : nullptr, eg);
  };

  f32x16 acc[T::TM][T::TN];
  db_zero<BN>(acc);
  db_pipeline(nk, load_global, store_lds, [&](int buf) { db_compute<BN>(cb_smem + buf * T::STAGE, acc); });

  float* out = g.out + (int64_t)blockIdx.z * g.range_stride;
  const int back = -(ex + eg);
  db_for_each_output<BN>(acc, [&](int row, int col, float v) {
    if (p0 + row < P && q0 + col < g.J) out[(int64_t)(p0 + row) * g.J + q0 + col] = ldexpf(v, back);
  });
}

// dW on a 32-row tile, for kh kw C <= 32 and J <= 32 (block1_conv1: 27 x 32, which the 128-row tile feeds 79 % zeros): one
// 32 x 32 tile per workgroup, so the four waves split the reduction instead of the tile.  A step is 128 output pixels, wave w
// multiplies pixels [32 w, 32 w + 32) of it into an accumulator of its own; at the end the four are added in wave order
// through LDS.  Loader, mask, scale and split are cb_dw_kernel's; an LDS row holds a step's 128 + 8 halves.
constexpr int CB_NK = 128;                       // output pixels per step
constexpr int CB_NLD = CB_NK + 8;                // u16 per LDS row (272 B: a wave's ds_read_b128 of 16 rows covers every bank once)
constexpr int CB_NSTAGE = 4 * 32 * CB_NLD;       // u16 per stage: A hi, A lo, B hi, B lo, 32 rows each
constexpr int CB_NLDS = 2 * CB_NSTAGE * (int)sizeof(u16);

__global__ __launch_bounds__(DB_T) void cb_dw_narrow_kernel(CbGemm g) {
  extern __shared__ __attribute__((aligned(16))) u16 cb_smem[];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int P = g.kh * g.kw * g.C;
  const int r0 = blockIdx.z * g.r_per_range, r1 = min(g.Mo, r0 + g.r_per_range);
  const int nk = (r1 - r0 + CB_NK - 1) / CB_NK;
  const int ex = (int)g.ctl[DB_EXP_X], eg = (int)g.ctl[DB_EXP_G];

  // the thread's row of either operand, and its quads: pixels 4 (tid / 32) + 32 i of a step, i = 0 .. 3 -- quad i is wave i's
  const int k = tid & 31, q = 4 * (tid >> 5);
  const bool k_ok = k < P, j_ok = k < g.J;
  const int tap = cb_quot(k, g.by_c), c = k - tap * g.C;
  const int ta = cb_quot(tap, g.by_kw);
  const int da = ta - g.pt, dc = tap - ta * g.kw - g.pl;

  struct {
    float a[4][4], b[4][4], m[4][4];
  } r;

  auto load_global = [&](int kt) {
    const int rk = r0 + kt * CB_NK + q;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int m0 = rk + 32 * i;
#pragma unroll
      for (int e = 0; e < 4; ++e) r.a[i][e] = r.b[i][e] = r.m[i][e] = 0.f;
      if (m0 >= r1) continue;
      if (k_ok) cb_load_patch4(g, m0, r1, da, dc, c, r.a[i]);
      if (j_ok) {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (m0 + e < r1) {
            r.b[i][e] = g.dy[(int64_t)(m0 + e) * g.ld_dy + k];
            if (g.y) r.m[i][e] = g.y[(int64_t)(m0 + e) * g.ld_y + k];
          }
      }
    }
  };
  auto store_lds = [&](int buf) {
    u16* A = cb_smem + buf * CB_NSTAGE + k * CB_NLD + q;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float sa[4], sb[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        sa[e] = ldexpf(r.a[i][e], ex);
        sb[e] = ldexpf(g.y ? db_mask(r.b[i][e], r.m[i][e]) : r.b[i][e], eg);
      }
      u32x2 hi, lo;
      split4(sa, &hi, &lo);
      *reinterpret_cast<u32x2*>(A + 32 * i) = hi;
      *reinterpret_cast<u32x2*>(A + 32 * CB_NLD + 32 * i) = lo;
      split4(sb, &hi, &lo);
      *reinterpret_cast<u32x2*>(A + 64 * CB_NLD + 32 * i) = hi;
      *reinterpret_cast<u32x2*>(A + 96 * CB_NLD + 32 * i) = lo;
    }
  };

  f32x16 acc;
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = 0.f;
  const int frow = lane & 31, fh = lane >> 5;
  auto compute = [&](int buf) {
    const u16* Ah = cb_smem + buf * CB_NSTAGE + frow * CB_NLD + wave * 32 + fh * 8;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      const f16x8 ah = *reinterpret_cast<const f16x8*>(Ah + ks * 16);
      const f16x8 al = *reinterpret_cast<const f16x8*>(Ah + 32 * CB_NLD + ks * 16);
      const f16x8 bh = *reinterpret_cast<const f16x8*>(Ah + 64 * CB_NLD + ks * 16);
      const f16x8 bl = *reinterpret_cast<const f16x8*>(Ah + 96 * CB_NLD + ks * 16);
      // small cross terms first, the dominant hi*hi term last
      acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, bh, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bl, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bh, acc, 0, 0, 0);
    }
  };
  db_pipeline(nk, load_global, store_lds, compute);

  // the four waves' sums, added in wave order (element reg of a lane: row (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5), column lane & 31)
  float* part = reinterpret_cast<float*>(cb_smem);
#pragma unroll
  for (int i = 0; i < 16; ++i) part[wave * 1024 + ((i & 3) + 8 * (i >> 2) + 4 * fh) * 32 + frow] = acc[i];
  __syncthreads();
  float* out = g.out + (int64_t)blockIdx.z * g.range_stride;
  const int back = -(ex + eg);
#pragma unroll
  for (int e = tid; e < 1024; e += DB_T) {
    const float v = ((part[e] + part[1024 + e]) + part[2048 + e]) + part[3072 + e];
    if ((e >> 5) < P && (e & 31) < g.J) out[(e >> 5) * g.J + (e & 31)] = ldexpf(v, back);
  }
}

// SAME: the input map is the output map (stride 1, 'SAME'), known when the kernel is compiled -- the source pixel of a row
// is then the row's own number less the tap's uniform shift.  Only the address differs; the general form gives the same
// addresses and measured 2.8 % slower on rpn_head/conv2d.
template <int BN, bool SAME>
__global__ __launch_bounds__(DB_T) void cb_dx_kernel(CbGemm g) {
  using T = DbTile<BN>;
  constexpr int BM = T::BM, A_IT = T::A_IT, B_IT = T::B_IT;

  extern __shared__ __attribute__((aligned(16))) u16 cb_smem[];

  const int tid = threadIdx.x;
  const int p0 = blockIdx.x * BM, q0 = blockIdx.y * BN;
  const int nk = g.kh * g.kw * g.jsteps;
  const int eg = (int)g.ctl[DB_EXP_G], ew = (int)g.ctl[DB_EXP_W];
  const int sh = g.s - 1;       // stride 1 or 2: a multiple of the stride has no bit under `sh`, its quotient is >> sh

  // the thread's rows (db_quad_row<false>: tid / 8 + 32 i): where they lie in their image and where their image's output
  // map begins; a row past M lies nowhere
  int mh[A_IT], mw[A_IT], mo[A_IT];
#pragma unroll
  for (int i = 0; i < A_IT; ++i) {
    const int m = p0 + (tid >> 3) + 32 * i, row = cb_quot(m, g.by_w), n = cb_quot(row, g.by_h);
    mw[i] = m - row * g.W + g.pl;
    mh[i] = m < g.M ? row - n * g.H + g.pt : -(1 << 30);
    mo[i] = n * g.Ho * g.Wo;
  }
  const int jq = db_quad_r<false>(tid, BM);

  struct {
    float a[A_IT][4], b[B_IT][4], m[A_IT][4];
  } r;      // the step in flight

  auto load_global = [&](int kt) {
    const int tap = cb_quot(kt, g.by_jsteps), j = (kt - tap * g.jsteps) * DB_BK + jq;
    const int ta = cb_quot(tap, g.by_kw), tb = tap - ta * g.kw;
#pragma unroll
    for (int i = 0; i < A_IT; ++i) {
#pragma unroll
      for (int e = 0; e < 4; ++e) r.a[i][e] = r.m[i][e] = 0.f;
      // input pixel (h, w) fed output pixel ((h + pt - a) / s, (w + pl - b) / s) through this tap, if that is one
      const int th = mh[i] - ta, tw = mw[i] - tb;
      int64_t src;
      bool fed;
      if constexpr (SAME) {
        fed = (unsigned)th < (unsigned)g.H && (unsigned)tw < (unsigned)g.W;
        src = p0 + (tid >> 3) + 32 * i - ((ta - g.pt) * g.W + (tb - g.pl));
      } else {
        fed = ((th | tw) & sh) == 0 && ((unsigned)th >> sh) < (unsigned)g.Ho && ((unsigned)tw >> sh) < (unsigned)g.Wo;
        src = mo[i] + (th >> sh) * g.Wo + (tw >> sh);
      }
      if (j < g.J && fed) {
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
  auto store_lds = [&](int buf) {
    u16* Ah = cb_smem + buf * T::STAGE;
    u16* Bh = Ah + 2 * BM * DB_LDH;
    db_store_quads<BM, A_IT, false>(Ah, Ah + BM * DB_LDH, r.a, g.y ? r.m : nullptr, eg);
    db_store_quads<BN, B_IT, false>(Bh, Bh + BN * DB_LDH, r.b, nullptr, ew);
  };

  f32x16 acc[T::TM][T::TN];
  db_zero<BN>(acc);
  db_pipeline(nk, load_global, store_lds, [&](int buf) { db_compute<BN>(cb_smem + buf * T::STAGE, acc); });

  const int back = -(eg + ew);
  const bool holes = g.hc < g.H || g.wc < g.W;      // some input pixels lie under no window: their x is not read
  db_for_each_output<BN>(acc, [&](int row, int col, float v) {
    const int m = p0 + row, c = q0 + col;
    if (m < g.M && c < g.C) {
      v = ldexpf(v, back);
      bool read_x = g.relu_in;
      if (read_x && holes) {
        const int line = cb_quot(m, g.by_w);
        read_x = m - line * g.W < g.wc && line - cb_quot(line, g.by_h) * g.H < g.hc;
      }
      if (read_x) v = db_mask(v, g.x[(int64_t)m * g.ld_x + c]);
      g.out[(int64_t)m * g.ld_out + c] = v;
    }
  });
}

template <void (*KERN)(CbGemm), int LDS>
static int cb_launch(const CbGemm& g, dim3 grid, hipStream_t s) {
  static DeviceOnce once;
  XDET_TRY(ensure_dynamic_lds(once, reinterpret_cast<const void*>(KERN), LDS));
  hipLaunchKernelGGL(KERN, grid, dim3(DB_T), LDS, s, g);
  XDET_LAUNCH_CHECK();
  return XDET_OK;
}
template <int BN, bool DW>
static int cb_launch_tile(const CbGemm& g, dim3 grid, hipStream_t s) {
  constexpr int lds = DbTile<BN>::LDS_BYTES;
  if (!DW && g.s == 1 && g.Ho == g.H && g.Wo == g.W) return cb_launch<cb_dx_kernel<BN, true>, lds>(g, grid, s);
  return cb_launch<DW ? cb_dw_kernel<BN> : cb_dx_kernel<BN, false>, lds>(g, grid, s);
}

// the two maps of a call: output size, padding in front, and how much of the input lies under a window
struct CbGeom {
  int Ho, Wo, pt, pl, hc, wc;
  int64_t M, Mo;
};
static void cb_axis(int n, int k, int s, int same, int* out, int* front, int* covered) {
  *out = same ? (n + s - 1) / s : (n >= k ? (n - k) / s + 1 : 0);
  *front = same ? std::max((*out - 1) * s + k - n, 0) / 2 : 0;
  *covered = std::min(n, (*out - 1) * s + k - *front);
}
// inside the limits of include/xdet.h
static bool cb_sizes_ok(int N, int H, int W, int C, int J, int kh, int kw, int stride, int padding, CbGeom* q) {
  if (N <= 0 || H <= 0 || W <= 0 || C <= 0 || J <= 0 || kh <= 0 || kw <= 0) return false;
  if (kh % 2 == 0 || kw % 2 == 0 || kh > CB_MAX_TAPS || kw > CB_MAX_TAPS || C > DB_MAX_DIM || J > DB_MAX_DIM) return false;
  if ((stride != 1 && stride != 2) || (padding != 0 && padding != 1)) return false;
  cb_axis(H, kh, stride, padding, &q->Ho, &q->pt, &q->hc);
  cb_axis(W, kw, stride, padding, &q->Wo, &q->pl, &q->wc);
  if (q->Ho < 1 || q->Wo < 1) return false;
  q->M = (int64_t)N * H * W;
  q->Mo = (int64_t)N * q->Ho * q->Wo;
  return q->M * C < (1ll << 31) && q->Mo * J < (1ll << 31);
}

// What the two C doors differ in.  At stride 1 'SAME' the maps coincide (M = Mo), so the general limits ARE
// xdet_conv_backward's -- N*H*W * max(C, J), and N*H*W * the largest pixel stride, below 2^31 -- and each door states them
// in its own words.  The 32-row dW tile sums in another order than the 128-row one, and xdet_conv_backward's bits are the
// latter's for every shape.
struct CbDoor {
  const char *who, *sizes, *strides;
  bool narrow_ok;
};
constexpr CbDoor CB_SAME1 = {
    "conv_backward",
    "N, H, W, C, J positive, kh and kw odd and at most 15, C and J at most 4096, N*H*W * max(C, J) below 2^31",
    "N*H*W * the largest pixel stride must stay below 2^31", false};
constexpr CbDoor CB_STRIDED = {
    "conv_backward_strided",
    "N, H, W, C, J positive, kh and kw odd and at most 15, C and J at most 4096, stride 1 or 2, padding 0 ('VALID', the kernel "
    "inside the map) or 1 ('SAME'), N*H*W * C and N*Ho*Wo * J below 2^31",
    "N*H*W * ld_x (ld_dx) and N*Ho*Wo * ld_dy (ld_y) must stay below 2^31", true};

static size_t cb_workspace_bytes(int N, int H, int W, int C, int J, int kh, int kw, int stride, int padding) {
  CbGeom q;
  if (!cb_sizes_ok(N, H, W, C, J, kh, kw, stride, padding, &q)) return 0;
  return ws_measure(4, db_layout, db_sums((int)q.Mo, kh * kw * C, J), kh * kw * C, J);
}

static int cb_run(const CbDoor& door, const float* x, int ld_x, const float* w, const float* y, int ld_y, const float* dy,
                  int ld_dy, int N, int H, int W, int C, int J, int kh, int kw, int stride, int padding, int relu_in, float* dx,
                  int ld_dx, float* dw, float* db, void* workspace, void* stream) {
  const std::string who = std::string(door.who) + ": ";
  CbGeom q{};
  XDET_REQUIRE(cb_sizes_ok(N, H, W, C, J, kh, kw, stride, padding, &q), who + door.sizes);
  XDET_REQUIRE(ld_x >= C && ld_dy >= J && (!y || ld_y >= J) && (!dx || ld_dx >= C),
               who + "a pixel stride is below its tensor's channel count");
  XDET_REQUIRE(q.M * std::max(ld_x, dx ? ld_dx : 0) < (1ll << 31) && q.Mo * std::max(ld_dy, y ? ld_y : 0) < (1ll << 31),
               who + door.strides);
  XDET_REQUIRE(x && w && dy && dw && db, who + "NULL argument");
  XDET_REQUIRE(workspace, who + "NULL workspace");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int M = (int)q.M, Mo = (int)q.Mo, KR = kh * kw * C;
  const DbSums pl = db_sums(Mo, KR, J);
  const auto [ctl, partial, slabs] = ws_carve(workspace, 4, db_layout, pl, KR, J);

  DbPre a{};
  a.x = x; a.w = w; a.y = y; a.dy = dy;
  a.ld_x = ld_x; a.ld_y = ld_y; a.ld_dy = ld_dy;
  a.M = Mo; a.x_cols = C; a.w_rows = KR; a.J = J; a.relu_x = relu_in != 0;
  a.x_rows = M;
  if (q.hc < H || q.wc < W) {
    a.x_h = H; a.x_w = W; a.x_hc = q.hc; a.x_wc = q.wc;
  }
  a.rows_per_chunk = pl.rows_per_chunk;
  a.n_chunks = pl.n_chunks;
  a.ctl = ctl;
  a.partial = partial;
  XDET_TRY(db_launch_prepass(a, db, s));

  CbGemm g{};
  g.x = x; g.w = w; g.y = y; g.dy = dy;
  g.ld_x = ld_x; g.ld_y = ld_y; g.ld_dy = ld_dy;
  g.M = M; g.Mo = Mo; g.H = H; g.W = W; g.Ho = q.Ho; g.Wo = q.Wo; g.C = C; g.J = J; g.kh = kh; g.kw = kw;
  g.relu_in = relu_in != 0;
  g.s = stride; g.pt = q.pt; g.pl = q.pl; g.hc = q.hc; g.wc = q.wc;
  g.jsteps = (int)cdiv(J, DB_BK);
  g.by_w = cb_div(W); g.by_h = cb_div(H); g.by_wo = cb_div(q.Wo); g.by_ho = cb_div(q.Ho);
  g.by_c = cb_div(C); g.by_kw = cb_div(kw); g.by_jsteps = cb_div(g.jsteps);
  g.ctl = ctl;
  if (dx) {
    g.out = dx; g.ld_out = ld_dx;
    g.vec_w = db_vec(w, J); g.vec_dy = db_vec(dy, ld_dy); g.vec_y = db_vec(y, ld_y);
    const unsigned mt = (unsigned)cdiv(M, DB_BM);
    XDET_TRY(C <= 32 ? (cb_launch_tile<32, false>(g, dim3(mt, 1, 1), s))
                     : (cb_launch_tile<128, false>(g, dim3(mt, (unsigned)cdiv(C, 128), 1), s)));
  }
  g.r_per_range = pl.rows_per_range;
  g.out = pl.n_ranges > 1 ? slabs : dw; g.range_stride = (int64_t)KR * J;
  if (door.narrow_ok && KR <= 32 && J <= 32) {      // one 32 x 32 tile: the ranges are all the parallelism there is
    XDET_TRY((cb_launch<cb_dw_narrow_kernel, CB_NLDS>(g, dim3(1, 1, (unsigned)pl.n_ranges), s)));
  } else {
    const dim3 grid((unsigned)cdiv(KR, DB_BM), (unsigned)cdiv(J, pl.bn_dw), (unsigned)pl.n_ranges);
    XDET_TRY(pl.bn_dw == 32 ? (cb_launch_tile<32, true>(g, grid, s)) : (cb_launch_tile<128, true>(g, grid, s)));
  }
  if (pl.n_ranges > 1) XDET_TRY(db_launch_fold(slabs, pl.n_ranges, (int64_t)KR * J, dw, s));
  return XDET_OK;
}

}  // namespace xdet

using namespace xdet;

extern "C" {

size_t xdet_conv_backward_workspace_bytes(int N, int H, int W, int C, int J, int kh, int kw) {
  return cb_workspace_bytes(N, H, W, C, J, kh, kw, 1, 1);
}

int xdet_conv_backward(const float* x, int ld_x, const float* w, const float* y, int ld_y, const float* dy, int ld_dy, int N,
                       int H, int W, int C, int J, int kh, int kw, int relu_in, float* dx, int ld_dx, float* dw, float* db,
                       void* workspace, void* stream) {
  return cb_run(CB_SAME1, x, ld_x, w, y, ld_y, dy, ld_dy, N, H, W, C, J, kh, kw, 1, 1, relu_in, dx, ld_dx, dw, db, workspace,
                stream);
}

size_t xdet_conv_backward_strided_workspace_bytes(int N, int H, int W, int C, int J, int kh, int kw, int stride, int padding) {
  return cb_workspace_bytes(N, H, W, C, J, kh, kw, stride, padding);
}

int xdet_conv_backward_strided(const float* x, int ld_x, const float* w, const float* y, int ld_y, const float* dy, int ld_dy,
                               int N, int H, int W, int C, int J, int kh, int kw, int stride, int padding, int relu_in,
                               float* dx, int ld_dx, float* dw, float* db, void* workspace, void* stream) {
  return cb_run(CB_STRIDED, x, ld_x, w, y, ld_y, dy, ld_dy, N, H, W, C, J, kh, kw, stride, padding, relu_in, dx, ld_dx, dw, db,
                workspace, stream);
}

}  // extern "C"
