// Batch normalisation over NHWC rows in both directions and both modes (xdet_batch_norm_forward / _backward,
// include/xdet.h): M = N H W rows of C channels with a row stride, statistics per channel.
//
//     training:  mean = sum_m x / M,  var = sum_m (x - mean)^2 / M  (centred on the folded mean: two passes over x, never
//                E[x^2] - E[x]^2),  invstd = 1 / sqrt(var + eps);   eval: mean and var are the moving statistics
//     y  = xhat gamma + beta,  xhat = (x - mean) invstd,  then max(., 0) with relu
//     g  = dy, or y > 0 ? dy : 0;   dbeta = sum_m g;   dgamma = sum_m g xhat
//     dx = gamma invstd (g - dbeta / M - xhat dgamma / M)  in training mode,  gamma invstd g  in eval mode
//
// Every pass is memory-bound: channels are contiguous, so a lane owns four consecutive channels (one float4 where the
// pointer and the row stride allow, four scalar loads otherwise -- the same values in the same order either way) and walks
// rows; a workgroup is sixteen waves = sixteen row lanes x 64 channel quads = 256 channels wide, so a thread of a 64-row chunk
// has its four rows in flight at once.
//
//   bn_sum_kernel<MODE>   one workgroup per (row chunk, channel block): row lane r adds the chunk's rows r, r + 16, ... in
//                         row order, the sixteen row lanes are added 0, 1, ..., 15 through LDS, and the chunk's sums go to the
//                         workspace.  MODE 0: sum x; 1: sum (x - mean)^2; 2: sum g and sum g xhat in one pass
//   bn_stats_kernel<MODE> one thread per channel adds the chunks in index order (at most 1024 of them) and finishes: 0 the
//                         mean; 1 var -> invstd and the moving-average updates; 2 dbeta and dgamma; 3 (eval forward, no sums)
//                         the moving statistics -> save_mean, save_invstd
//   bn_apply_kernel<BWD>  the normalise pass (y) or the dx pass over 64 rows x 256 channels per workgroup
// The fold is a launch of its own: no fence, no ticket, no float atomic anywhere, so the same call gives the same bits over
// any workspace contents.  The chunks depend on M alone (bn_sums, batchnorm_layout.h).  The file is compiled with
// -ffp-contract=off: every sum is a plain f32 add of plain f32 products, so dy * 2^k gives dx, dgamma, dbeta * 2^k exactly.
#include "common.h"
#include "batchnorm_layout.h"
#include "channel_quad.h"
#include <algorithm>

namespace xdet {

constexpr int BN_RL = 16;           // row lanes (waves) of a workgroup
constexpr int BN_T = 64 * BN_RL;    // threads: 16 row lanes x 64 channel quads
constexpr int BN_CB = 256;          // channels per workgroup
constexpr int BN_APPLY_ROWS = 64;   // rows per workgroup of the elementwise passes
constexpr int BN_STATS_T = 256;     // threads of the per-channel fold

struct BnArgs {
  const float *x, *y, *dy;          // y: the mask of the backward (NULL: none)
  int ld_x, ld_y, ld_dy, ld_out;
  int M, C;
  int rows_per_chunk, n_chunks;
  int vec_x, vec_y, vec_dy, vec_out;
  int relu, training;
  const float *gamma, *beta, *mean, *invstd, *dgamma, *dbeta;
  float* out;                       // y (forward) or dx (backward)
  float *first, *second;            // the workspace's chunk sums
};

// y > 0 is false for a NaN: the gradient behind a NaN activation is 0
__device__ __forceinline__ float bn_mask(float dy, float y) { return y > 0.f ? dy : 0.f; }

template <int MODE>
__global__ __launch_bounds__(BN_T) void bn_sum_kernel(BnArgs a) {
  __shared__ float red[2][BN_RL][BN_CB];
  const int tid = threadIdx.x, lane = tid & 63, rl = tid >> 6;
  const int c0 = blockIdx.y * BN_CB + lane * 4, left = a.C - c0;
  const int m0 = blockIdx.x * a.rows_per_chunk, m1 = min(a.M, m0 + a.rows_per_chunk);
  float s0[4] = {0.f, 0.f, 0.f, 0.f}, s1[4] = {0.f, 0.f, 0.f, 0.f};
  if (left > 0) {
    float mean[4] = {0.f, 0.f, 0.f, 0.f}, inv[4] = {0.f, 0.f, 0.f, 0.f};
    if (MODE >= 1) quad_load(a.mean + c0, left, false, mean);
    if (MODE == 2) quad_load(a.invstd + c0, left, false, inv);
#pragma unroll 4
    for (int m = m0 + rl; m < m1; m += BN_RL) {
      float x[4];
      quad_load(a.x + (int64_t)m * a.ld_x + c0, left, a.vec_x, x);
      if (MODE == 0) {
#pragma unroll
        for (int e = 0; e < 4; ++e) s0[e] += x[e];
      } else if (MODE == 1) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float d = x[e] - mean[e];
          s0[e] += d * d;
        }
      } else {
        float g[4];
        quad_load(a.dy + (int64_t)m * a.ld_dy + c0, left, a.vec_dy, g);
        if (a.y) {
          float y[4];
          quad_load(a.y + (int64_t)m * a.ld_y + c0, left, a.vec_y, y);
#pragma unroll
          for (int e = 0; e < 4; ++e) g[e] = bn_mask(g[e], y[e]);
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          s0[e] += g[e];
          s1[e] += g[e] * ((x[e] - mean[e]) * inv[e]);
        }
      }
    }
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    red[0][rl][lane * 4 + e] = s0[e];
    if (MODE == 2) red[1][rl][lane * 4 + e] = s1[e];
  }
  __syncthreads();
  const int c = blockIdx.y * BN_CB + tid;
  if (tid < BN_CB && c < a.C) {
    const int64_t o = (int64_t)blockIdx.x * a.C + c;
    float t0 = red[0][0][tid], t1 = MODE == 2 ? red[1][0][tid] : 0.f;
#pragma unroll
    for (int r = 1; r < BN_RL; ++r) {
      t0 += red[0][r][tid];
      if (MODE == 2) t1 += red[1][r][tid];
    }
    a.first[o] = t0;
    if (MODE == 2) a.second[o] = t1;
  }
}

struct BnStats {
  const float *first, *second;
  int n_chunks, M, C;
  float eps, momentum;
  float *moving_mean, *moving_var;      // training forward: updated when given; eval forward: read
  float *save_mean, *save_invstd;
  float *dgamma, *dbeta;
};

template <int MODE>
__global__ __launch_bounds__(BN_STATS_T) void bn_stats_kernel(BnStats a) {
  const int c = blockIdx.x * BN_STATS_T + threadIdx.x;
  if (c >= a.C) return;
  if (MODE == 0) {
    const float mean = fold_chunks(a.first, a.n_chunks, a.C, c) / (float)a.M;
    a.save_mean[c] = mean;
    if (a.moving_mean) a.moving_mean[c] -= (a.moving_mean[c] - mean) * (1.f - a.momentum);
  } else if (MODE == 1) {
    const float var = fold_chunks(a.second, a.n_chunks, a.C, c) / (float)a.M;
    a.save_invstd[c] = 1.f / sqrtf(var + a.eps);
    if (a.moving_var) {
      const float unbiased = var * ((float)a.M / (float)max(a.M - 1, 1));
      a.moving_var[c] -= (a.moving_var[c] - unbiased) * (1.f - a.momentum);
    }
  } else if (MODE == 2) {
    a.dbeta[c] = fold_chunks(a.first, a.n_chunks, a.C, c);
    a.dgamma[c] = fold_chunks(a.second, a.n_chunks, a.C, c);
  } else {
    a.save_mean[c] = a.moving_mean[c];
    a.save_invstd[c] = 1.f / sqrtf(a.moving_var[c] + a.eps);
  }
}

template <bool BWD>
__global__ __launch_bounds__(BN_T) void bn_apply_kernel(BnArgs a) {
  const int tid = threadIdx.x, lane = tid & 63, rl = tid >> 6;
  const int c0 = blockIdx.y * BN_CB + lane * 4, left = a.C - c0;
  if (left <= 0) return;
  const int m0 = blockIdx.x * BN_APPLY_ROWS, m1 = min(a.M, m0 + BN_APPLY_ROWS);
  float mean[4], inv[4], gamma[4], b[4], k[4] = {0.f, 0.f, 0.f, 0.f};
  quad_load(a.mean + c0, left, false, mean);
  quad_load(a.invstd + c0, left, false, inv);
  quad_load(a.gamma + c0, left, false, gamma);
  if (BWD) {
#pragma unroll
    for (int e = 0; e < 4; ++e) b[e] = 0.f;
    if (a.training) {     // b = dbeta / M, k = dgamma / M
      quad_load(a.dbeta + c0, left, false, b);
      quad_load(a.dgamma + c0, left, false, k);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        b[e] = b[e] / (float)a.M;
        k[e] = k[e] / (float)a.M;
      }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) gamma[e] = gamma[e] * inv[e];
  } else {
    quad_load(a.beta + c0, left, false, b);
  }
#pragma unroll 4
  for (int m = m0 + rl; m < m1; m += BN_RL) {
    float x[4] = {0.f, 0.f, 0.f, 0.f}, o[4];
    if (!BWD || a.training) quad_load(a.x + (int64_t)m * a.ld_x + c0, left, a.vec_x, x);
    if (BWD) {
      float g[4];
      quad_load(a.dy + (int64_t)m * a.ld_dy + c0, left, a.vec_dy, g);
      if (a.y) {
        float y[4];
        quad_load(a.y + (int64_t)m * a.ld_y + c0, left, a.vec_y, y);
#pragma unroll
        for (int e = 0; e < 4; ++e) g[e] = bn_mask(g[e], y[e]);
      }
#pragma unroll
      for (int e = 0; e < 4; ++e)
        o[e] = a.training ? gamma[e] * ((g[e] - b[e]) - ((x[e] - mean[e]) * inv[e]) * k[e]) : gamma[e] * g[e];
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        o[e] = ((x[e] - mean[e]) * inv[e]) * gamma[e] + b[e];
        if (a.relu) o[e] = fmaxf(o[e], 0.f);
      }
    }
    quad_store(a.out + (int64_t)m * a.ld_out + c0, left, a.vec_out, o);
  }
}

static bool bn_sizes_ok(int M, int C) { return M > 0 && C > 0 && C <= BN_MAX_C && (int64_t)M * C < (1ll << 31); }

template <int MODE>
static int bn_launch_sum(const BnArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(bn_sum_kernel<MODE>, dim3((unsigned)a.n_chunks, (unsigned)cdiv(a.C, BN_CB)), dim3(BN_T), 0, s, a);
  XDET_LAUNCH_CHECK();
  return XDET_OK;
}
template <int MODE>
static int bn_launch_stats(const BnStats& a, hipStream_t s) {
  hipLaunchKernelGGL(bn_stats_kernel<MODE>, dim3((unsigned)cdiv(a.C, BN_STATS_T)), dim3(BN_STATS_T), 0, s, a);
  XDET_LAUNCH_CHECK();
  return XDET_OK;
}
template <bool BWD>
static int bn_launch_apply(const BnArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(bn_apply_kernel<BWD>, dim3((unsigned)cdiv(a.M, BN_APPLY_ROWS), (unsigned)cdiv(a.C, BN_CB)), dim3(BN_T), 0,
                     s, a);
  XDET_LAUNCH_CHECK();
  return XDET_OK;
}

}  // namespace xdet

using namespace xdet;

extern "C" {

size_t xdet_batch_norm_workspace_bytes(int M, int C) {
  if (!bn_sizes_ok(M, C)) return 0;
  return ws_measure(4, bn_layout, bn_sums(M), C);
}

int xdet_batch_norm_forward(const float* x, int ld_x, int M, int C, const float* gamma, const float* beta, float eps,
                            int training, float momentum, float* moving_mean, float* moving_var, int relu, float* y, int ld_y,
                            float* save_mean, float* save_invstd, void* workspace, void* stream) {
  XDET_REQUIRE(bn_sizes_ok(M, C), "batch_norm_forward: M and C positive, C at most 4096, M * C below 2^31");
  XDET_REQUIRE(ld_x >= C && ld_y >= C, "batch_norm_forward: a row stride is below the channel count");
  XDET_REQUIRE((int64_t)M * std::max(ld_x, ld_y) < (1ll << 31), "batch_norm_forward: M * the largest row stride must stay below 2^31");
  XDET_REQUIRE(x && gamma && beta && y && save_mean && save_invstd, "batch_norm_forward: NULL argument");
  XDET_REQUIRE(workspace, "batch_norm_forward: NULL workspace");
  XDET_REQUIRE(training ? (moving_mean != nullptr) == (moving_var != nullptr) : moving_mean && moving_var,
               "batch_norm_forward: training == 0 needs both moving statistics; training mode takes both or neither");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const BnSums pl = bn_sums(M);
  const auto [first, second] = ws_carve(workspace, 4, bn_layout, pl, C);

  BnArgs a{};
  a.x = x; a.ld_x = ld_x; a.ld_out = ld_y;
  a.M = M; a.C = C;
  a.rows_per_chunk = pl.rows_per_chunk; a.n_chunks = pl.n_chunks;
  a.vec_x = quad_vec(x, ld_x); a.vec_out = quad_vec(y, ld_y);
  a.relu = relu != 0; a.training = training != 0;
  a.gamma = gamma; a.beta = beta; a.mean = save_mean; a.invstd = save_invstd;
  a.out = y;
  a.first = first; a.second = second;

  BnStats st{};
  st.first = first; st.second = second;
  st.n_chunks = pl.n_chunks; st.M = M; st.C = C;
  st.eps = eps; st.momentum = momentum;
  st.moving_mean = moving_mean; st.moving_var = moving_var;
  st.save_mean = save_mean; st.save_invstd = save_invstd;

  if (training) {
    XDET_TRY(bn_launch_sum<0>(a, s));
    XDET_TRY(bn_launch_stats<0>(st, s));
    a.first = second;                     // the centred squares' chunk sums
    XDET_TRY(bn_launch_sum<1>(a, s));
    XDET_TRY(bn_launch_stats<1>(st, s));
  } else {
    XDET_TRY(bn_launch_stats<3>(st, s));
  }
  return bn_launch_apply<false>(a, s);
}

int xdet_batch_norm_backward(const float* x, int ld_x, const float* y, int ld_y, const float* dy, int ld_dy, int M, int C,
                             const float* gamma, const float* save_mean, const float* save_invstd, int training, float* dx,
                             int ld_dx, float* dgamma, float* dbeta, void* workspace, void* stream) {
  XDET_REQUIRE(bn_sizes_ok(M, C), "batch_norm_backward: M and C positive, C at most 4096, M * C below 2^31");
  XDET_REQUIRE(ld_x >= C && ld_dy >= C && (!y || ld_y >= C) && (!dx || ld_dx >= C),
               "batch_norm_backward: a row stride is below the channel count");
  XDET_REQUIRE((int64_t)M * std::max(std::max(ld_x, ld_dy), std::max(y ? ld_y : 0, dx ? ld_dx : 0)) < (1ll << 31),
               "batch_norm_backward: M * the largest row stride must stay below 2^31");
  XDET_REQUIRE(x && dy && gamma && save_mean && save_invstd && dgamma && dbeta, "batch_norm_backward: NULL argument");
  XDET_REQUIRE(workspace, "batch_norm_backward: NULL workspace");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const BnSums pl = bn_sums(M);
  const auto [first, second] = ws_carve(workspace, 4, bn_layout, pl, C);

  BnArgs a{};
  a.x = x; a.y = y; a.dy = dy;
  a.ld_x = ld_x; a.ld_y = ld_y; a.ld_dy = ld_dy; a.ld_out = ld_dx;
  a.M = M; a.C = C;
  a.rows_per_chunk = pl.rows_per_chunk; a.n_chunks = pl.n_chunks;
  a.vec_x = quad_vec(x, ld_x); a.vec_y = quad_vec(y, ld_y); a.vec_dy = quad_vec(dy, ld_dy); a.vec_out = quad_vec(dx, ld_dx);
  a.training = training != 0;
  a.gamma = gamma; a.mean = save_mean; a.invstd = save_invstd; a.dgamma = dgamma; a.dbeta = dbeta;
  a.out = dx;
  a.first = first; a.second = second;
  XDET_TRY(bn_launch_sum<2>(a, s));

  BnStats st{};
  st.first = first; st.second = second;
  st.n_chunks = pl.n_chunks; st.M = M; st.C = C;
  st.dgamma = dgamma; st.dbeta = dbeta;
  XDET_TRY(bn_launch_stats<2>(st, s));
  if (dx) XDET_TRY(bn_launch_apply<true>(a, s));
  return XDET_OK;
}

}  // extern "C"
