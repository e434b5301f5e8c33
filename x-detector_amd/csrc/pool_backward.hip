// The backward of max_pooling2d(3, 2, 'same') (xdet_maxpool3x3s2_backward, include/xdet.h) and the stride-2 gather / scatter
// around a 1x1 / stride-2 projection (xdet_subsample2, xdet_add_upsample2): the three ops the entry flow's backward adds to
// the set.  NHWC f32 with a pixel stride per tensor.
//
// The pool's geometry is TensorFlow's 'SAME': Ho = ceil(H / 2), total padding max((Ho - 1) * 2 + 3 - H, 0) with the smaller
// half in front -- 1 / 1 on an odd extent, 0 / 1 on an even one -- and a padded position never wins.  Window oh covers the
// rows 2 oh - pt .. 2 oh - pt + 2, so row h lies in the windows (h + pt) / 2 - 1 (where h + pt is even) and (h + pt) / 2:
// at most two per axis, four per pixel.
//
//     dx[n,h,w,c] = sum over the windows (oh, ow) that contain (h, w), ascending, of dy[n,oh,ow,c]
//                   where (h, w) is the window's FIRST maximum in row-major order (strict > against the running best, which
//                   starts at the window's first in-image element), each add rounded; 0 where no window chooses the pixel
//
// Written as a gather: the owner of a dx element derives the argmax of its <= 4 windows again from x, so there is no
// atomic, no stored index and no order to fix -- the same call gives the same bits, and the forward pool stays as it is.
// The op is memory-bound: channels are innermost and a thread owns four consecutive ones (channel_quad.h) of a 2 x 2 block
// of pixels; consecutive threads walk the channel quads of a block and then the next block, so every access is a row
// segment.  The 5 x 5 neighbourhood of x a block compares (9 loads per window, four windows per block) is shared with the
// neighbouring pixels of the workgroup and the ones beside it and comes from L1 / L2; HBM sees x once, dy once, dx once.
// An absent tap's address is replaced by a valid one of the image, so a window's nine loads are in flight together.
// The file is compiled with -ffp-contract=off (there is no product here, but it keeps the unit among the exact ones).
#include "common.h"
#include "channel_quad.h"
#include <algorithm>

namespace xdet {

constexpr int PB_T = 256;            // threads of a workgroup: (pixel, channel quad) pairs
constexpr int PB_MAX_C = 4096;

struct PoolBwdArgs {
  const float *x, *dy;
  float* dx;
  int ld_x, ld_dy, ld_dx;
  int H, W, C, Ho, Wo, pt, pl;
  int Kb, Jb;                        // 2 x 2 pixel blocks per image along each axis, in padded coordinates
  int quads;                         // ceil(C / 4)
  int64_t total;                     // N * Kb * Jb * quads
  int vec_x, vec_dy, vec_dx;
};

// A thread owns four channels of the 2 x 2 pixels P in {2k, 2k+1}, Q in {2j, 2j+1} (P = h + pt, Q = w + pl: padded
// coordinates, in which window oh covers the rows 2 oh .. 2 oh + 2).  Those four pixels lie in the same four windows
// (k-1 .. k) x (j-1 .. j) and in no other, so each window's argmax is derived once for all of them: 36 loads per four pixels
// where a thread per pixel took 81.  The windows are walked ascending in (oh, ow), so every pixel adds its shares in that order.
__global__ __launch_bounds__(PB_T) void maxpool3x3s2_bwd_kernel(PoolBwdArgs a) {
  const int64_t idx = (int64_t)blockIdx.x * PB_T + threadIdx.x;
  if (idx >= a.total) return;
  const int q = (int)(idx % a.quads);
  int rest = (int)(idx / a.quads);
  const int j = rest % a.Jb; rest /= a.Jb;
  const int k = rest % a.Kb;
  const int n = rest / a.Kb;
  const int c0 = q * 4, left = a.C - c0;
  const float* __restrict__ px = a.x;
  const float* __restrict__ pg = a.dy;
  const int64_t img = (int64_t)n * a.H * a.W;    // windows stay inside image n: rows and columns are bounded by H and W
  float s[4][4];
#pragma unroll
  for (int p = 0; p < 4; ++p)
#pragma unroll
    for (int e = 0; e < 4; ++e) s[p][e] = 0.f;
#pragma unroll
  for (int dk = 0; dk < 2; ++dk)
#pragma unroll
    for (int dj = 0; dj < 2; ++dj) {
      const int oh = k - 1 + dk, ow = j - 1 + dj;
      if (oh < 0 || oh >= a.Ho || ow < 0 || ow >= a.Wo) continue;
      const int r0 = 2 * oh - a.pt, q0 = 2 * ow - a.pl;
      float v[9][4];
      bool live[9];
#pragma unroll
      for (int t = 0; t < 9; ++t) {
        const int r = r0 + t / 3, c = q0 + t % 3;
        live[t] = r >= 0 && r < a.H && c >= 0 && c < a.W;
        const int64_t src = live[t] ? img + (int64_t)r * a.W + c : img;      // an absent tap's pixel is not read
        quad_load(px + src * a.ld_x + c0, left, a.vec_x, v[t]);
      }
      float g[4];
      quad_load(pg + ((int64_t)n * a.Ho * a.Wo + (int64_t)oh * a.Wo + ow) * a.ld_dy + c0, left, a.vec_dy, g);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float best = 0.f;
        int arg = -1;
#pragma unroll
        for (int t = 0; t < 9; ++t) {
          if (!live[t]) continue;
          if (arg < 0 || v[t][e] > best) {       // strict: the first maximum keeps the window
            best = v[t][e];
            arg = t;
          }
        }
        // the window's taps among the four pixels: its last row / column where it is the block's upper / left window
#pragma unroll
        for (int t = 0; t < 9; ++t) {
          const int ta = t / 3, tb = t % 3;
          const bool mine = (dk == 0 ? ta == 2 : ta < 2) && (dj == 0 ? tb == 2 : tb < 2);
          if (!mine) continue;
          const int slot = (dk == 0 ? 0 : ta) * 2 + (dj == 0 ? 0 : tb);
          if (arg == t) s[slot][e] += g[e];
        }
      }
    }
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const int h = 2 * k + (p >> 1) - a.pt, w = 2 * j + (p & 1) - a.pl;
    if (h < 0 || h >= a.H || w < 0 || w >= a.W) continue;
    quad_store(a.dx + (img + (int64_t)h * a.W + w) * a.ld_dx + c0, left, a.vec_dx, s[p]);
  }
}

// out[n,i,j,:] = x[n,2i,2j,:]
__global__ __launch_bounds__(PB_T) void subsample2_kernel(const float* __restrict__ x, int ld_x, float* __restrict__ out, int ld_out,
                                                          int H, int W, int Ho, int Wo, int C, int quads, int64_t total, int vec_x,
                                                          int vec_out) {
  const int64_t idx = (int64_t)blockIdx.x * PB_T + threadIdx.x;
  if (idx >= total) return;
  const int q = (int)(idx % quads);
  const int m = (int)(idx / quads);
  const int j = m % Wo, i = (m / Wo) % Ho, n = m / (Wo * Ho);
  const int c0 = q * 4, left = C - c0;
  float v[4];
  quad_load(x + ((int64_t)n * H * W + (int64_t)(2 * i) * W + 2 * j) * ld_x + c0, left, vec_x, v);
  quad_store(out + (int64_t)m * ld_out + c0, left, vec_out, v);
}

// out[n,h,w,:] = a[n,h,w,:] + b[n,h/2,w/2,:] where h and w are even, a's bits elsewhere (no __restrict__: out may be a)
__global__ __launch_bounds__(PB_T) void add_upsample2_kernel(const float* a, int ld_a, const float* b, int ld_b, float* out, int ld_out,
                                                             int H, int W, int Ho, int Wo, int C, int quads, int64_t total, int vec_a,
                                                             int vec_b, int vec_out) {
  const int64_t idx = (int64_t)blockIdx.x * PB_T + threadIdx.x;
  if (idx >= total) return;
  const int q = (int)(idx % quads);
  const int m = (int)(idx / quads);
  const int w = m % W, h = (m / W) % H, n = m / (W * H);
  const int c0 = q * 4, left = C - c0;
  float u[4];
  quad_load(a + (int64_t)m * ld_a + c0, left, vec_a, u);
  if (((h | w) & 1) == 0) {
    float v[4];
    quad_load(b + ((int64_t)n * Ho * Wo + (int64_t)(h >> 1) * Wo + (w >> 1)) * ld_b + c0, left, vec_b, v);
#pragma unroll
    for (int e = 0; e < 4; ++e) u[e] = u[e] + v[e];
  }
  quad_store(out + (int64_t)m * ld_out + c0, left, vec_out, u);
}

static bool pb_sizes_ok(int N, int H, int W, int C) {
  if (N <= 0 || H <= 0 || W <= 0 || C <= 0 || C > PB_MAX_C) return false;
  const int64_t rows = (int64_t)N * H;      // (stepwise: no product of more than two ints before it is bounded)
  return rows < (1ll << 31) && rows * W < (1ll << 31) && rows * W * C < (1ll << 31);
}

}  // namespace xdet

using namespace xdet;

extern "C" {

int xdet_maxpool3x3s2_backward(const float* x, int ld_x, const float* dy, int ld_dy, int N, int H, int W, int C, float* dx, int ld_dx,
                               void* stream) {
  XDET_REQUIRE(pb_sizes_ok(N, H, W, C), "maxpool3x3s2_backward: N, H, W and C positive, C at most 4096, N * H * W * C below 2^31");
  XDET_REQUIRE(ld_x >= C && ld_dy >= C && ld_dx >= C, "maxpool3x3s2_backward: a pixel stride is below the channel count");
  const int64_t M = (int64_t)N * H * W;
  XDET_REQUIRE(M * std::max(std::max(ld_x, ld_dy), ld_dx) < (1ll << 31),
               "maxpool3x3s2_backward: N * H * W * the largest pixel stride must stay below 2^31");
  XDET_REQUIRE(x && dy && dx, "maxpool3x3s2_backward: NULL argument");
  PoolBwdArgs a{};
  a.x = x; a.dy = dy; a.dx = dx;
  a.ld_x = ld_x; a.ld_dy = ld_dy; a.ld_dx = ld_dx;
  a.H = H; a.W = W; a.C = C;
  a.Ho = (H + 1) / 2; a.Wo = (W + 1) / 2;
  a.pt = std::max((a.Ho - 1) * 2 + 3 - H, 0) / 2;      // the smaller half in front: 1 on an odd extent, 0 on an even one
  a.pl = std::max((a.Wo - 1) * 2 + 3 - W, 0) / 2;
  a.Kb = (H - 1 + a.pt) / 2 + 1; a.Jb = (W - 1 + a.pl) / 2 + 1;
  a.quads = (C + 3) / 4;
  a.total = (int64_t)N * a.Kb * a.Jb * a.quads;
  a.vec_x = quad_vec(x, ld_x); a.vec_dy = quad_vec(dy, ld_dy); a.vec_dx = quad_vec(dx, ld_dx);
  hipLaunchKernelGGL(maxpool3x3s2_bwd_kernel, dim3((unsigned)cdiv(a.total, PB_T)), dim3(PB_T), 0, reinterpret_cast<hipStream_t>(stream), a);
  XDET_LAUNCH_CHECK();
  return XDET_OK;
}

int xdet_subsample2(const float* x, int ld_x, int N, int H, int W, int C, float* out, int ld_out, void* stream) {
  XDET_REQUIRE(pb_sizes_ok(N, H, W, C), "subsample2: N, H, W and C positive, C at most 4096, N * H * W * C below 2^31");
  XDET_REQUIRE(ld_x >= C && ld_out >= C, "subsample2: a pixel stride is below the channel count");
  XDET_REQUIRE((int64_t)N * H * W * std::max(ld_x, ld_out) < (1ll << 31), "subsample2: N * H * W * the largest pixel stride must stay below 2^31");
  XDET_REQUIRE(x && out, "subsample2: NULL argument");
  const int Ho = (H + 1) / 2, Wo = (W + 1) / 2, quads = (C + 3) / 4;
  const int64_t total = (int64_t)N * Ho * Wo * quads;
  hipLaunchKernelGGL(subsample2_kernel, dim3((unsigned)cdiv(total, PB_T)), dim3(PB_T), 0, reinterpret_cast<hipStream_t>(stream), x, ld_x,
                     out, ld_out, H, W, Ho, Wo, C, quads, total, quad_vec(x, ld_x), quad_vec(out, ld_out));
  XDET_LAUNCH_CHECK();
  return XDET_OK;
}

int xdet_add_upsample2(const float* a, int ld_a, const float* b, int ld_b, int N, int H, int W, int C, float* out, int ld_out,
                       void* stream) {
  XDET_REQUIRE(pb_sizes_ok(N, H, W, C), "add_upsample2: N, H, W and C positive, C at most 4096, N * H * W * C below 2^31");
  XDET_REQUIRE(ld_a >= C && ld_b >= C && ld_out >= C, "add_upsample2: a pixel stride is below the channel count");
  XDET_REQUIRE((int64_t)N * H * W * std::max(std::max(ld_a, ld_b), ld_out) < (1ll << 31),
               "add_upsample2: N * H * W * the largest pixel stride must stay below 2^31");
  XDET_REQUIRE(a && b && out, "add_upsample2: NULL argument");
  const int Ho = (H + 1) / 2, Wo = (W + 1) / 2, quads = (C + 3) / 4;
  const int64_t total = (int64_t)N * H * W * quads;
  hipLaunchKernelGGL(add_upsample2_kernel, dim3((unsigned)cdiv(total, PB_T)), dim3(PB_T), 0, reinterpret_cast<hipStream_t>(stream), a, ld_a,
                     b, ld_b, out, ld_out, H, W, Ho, Wo, C, quads, total, quad_vec(a, ld_a), quad_vec(b, ld_b), quad_vec(out, ld_out));
  XDET_LAUNCH_CHECK();
  return XDET_OK;
}

}  // extern "C"
