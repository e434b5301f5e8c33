// RotatedPsRoiAlign forward and gradient for gfx950 -- replaces the reference's TF custom ops
// (cpp/PSROIPooling/rotated_ps_roi_align_op.cc:163-292 CPU functor; rotated_ps_roi_align_grad_op.cu:37-170 scatter).
//
// THIS FILE IS COMPILED WITH -ffp-contract=off: the geometry is a fixed sequence of separately rounded f32 operations,
// and wherever a `1.` / `2.` literal meets an operand the reference evaluates in double and rounds the result to float
// (edge steps, bin corners, sample positions, the bilinear blend).  Every expression below keeps that tree.
//
// Work decomposition (as psroialign_fwd_kernel): one 64-lane wavefront per (image, roi), the XCD-aware
// image order, lanes over the ROI's C = gh*gw*bank output elements.  The quad's vertices are ordered once per ROI, a
// bin's corners, sample counts and sample-step terms once per element a lane owns (in registers: no exchange between
// lanes), and the sample grid is separable (x depends on the column only, y on the row only, :263-264), so a lane
// hoists its bin's column geometry out of the row loop.
#include "common.h"
#include <cfloat>

namespace xdet {

// ordered vertices (y[k], x[k]) in map units; false for a degenerate quad (a squared side below FLT_MIN, :205-211)
__device__ __forceinline__ bool rot_vertices(const float* __restrict__ roi, int order, int H, int W, float (&y)[4],
                                             float (&x)[4]) {
  const int start = order < 0 ? 0 : order & 3;                 // order >= 0: vertex order mod 4 (reference: [-1, 4))
  float vy[4], vx[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int v = (start + k) & 3;
    vy[k] = roi[2 * v] * (float)H;
    vx[k] = roi[2 * v + 1] * (float)W;
  }
  double len[4];
  bool degenerate = false;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const float dy = vy[(k + 1) & 3] - vy[k], dx = vx[(k + 1) & 3] - vx[k];
    len[k] = (double)(dy * dy + dx * dx);
    degenerate = degenerate || len[k] < (double)FLT_MIN;
  }
  const int shift = order < 0 ? (len[0] + len[2] > len[1] + len[3] ? 1 : 0) : 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    y[k] = shift ? vy[(k + 1) & 3] : vy[k];
    x[k] = shift ? vx[(k + 1) & 3] : vx[k];
  }
  return !degenerate;
}

// what the samples of bin (r, c) need (:222-255): column x = mean of the top- and bottom-edge points, row y = mean of
// the left- and right-edge points
struct RotBin {
  float ltx, lbx, gxst, gxsb;      // x(pw) = (ltx + (pw+1.)*gxst + lbx + (pw+1.)*gxsb) / 2.
  float lty, rty, gysl, gysr;      // y(ph) = (lty + (ph+1.)*gysl + rty + (ph+1.)*gysr) / 2.
  int n_w, n_h;
};

__device__ __forceinline__ float rot_min(float a, float b) { return b < a ? b : a; }   // std::min
__device__ __forceinline__ float rot_max(float a, float b) { return a < b ? b : a; }   // std::max

__device__ __forceinline__ RotBin rot_bin(const float (&y)[4], const float (&x)[4], int r, int c, int gw, int gh,
                                          float cap) {
  const float ysl = (float)((double)(y[3] - y[0]) / (gh * 1.));
  const float ysr = (float)((double)(y[2] - y[1]) / (gh * 1.));
  const float xst = (float)((double)(x[1] - x[0]) / (gw * 1.));
  const float xsb = (float)((double)(x[2] - x[3]) / (gw * 1.));
  const float rf = (float)r, cf = (float)c;
  const float left_y1 = y[0] + rf * ysl;
  const float right_y1 = y[1] + rf * ysr;
  const float left_y2 = (float)((double)y[0] + (r + 1.) * (double)ysl);
  const float right_y2 = (float)((double)y[1] + (r + 1.) * (double)ysr);
  const float lty = left_y1 + cf * (right_y1 - left_y1) / (float)gw;
  const float rty = (float)((double)left_y1 + (c + 1.) * (double)(right_y1 - left_y1) / (double)gw);
  const float lby = left_y2 + cf * (right_y2 - left_y2) / (float)gw;
  const float rby = (float)((double)left_y2 + (c + 1.) * (double)(right_y2 - left_y2) / (double)gw);
  const float top_x1 = x[0] + cf * xst;
  const float bottom_x1 = x[3] + cf * xsb;
  const float top_x2 = (float)((double)x[0] + (c + 1.) * (double)xst);
  const float bottom_x2 = (float)((double)x[3] + (c + 1.) * (double)xsb);
  const float ltx = top_x1 + rf * (bottom_x1 - top_x1) / (float)gh;
  const float lbx = (float)((double)top_x1 + (r + 1.) * (double)(bottom_x1 - top_x1) / (double)gh);
  const float rtx = top_x2 + rf * (bottom_x2 - top_x2) / (float)gh;
  const float rbx = (float)((double)top_x2 + (r + 1.) * (double)(bottom_x2 - top_x2) / (double)gh);
  const float bw = rot_max(rot_min(fabsf(rtx - ltx), fabsf(rty - lty)), rot_min(fabsf(rbx - lbx), fabsf(rby - lby)));
  const float bh = rot_max(rot_min(fabsf(lbx - ltx), fabsf(lby - lty)), rot_min(fabsf(rbx - rtx), fabsf(rby - rty)));
  RotBin b;
  // (int)bw + 1 as the reference, through a float clamped to [0, H + W]: a quad inside [0,1] never reaches the cap;
  // a NaN / far-out one gets a bounded sample count and no undefined conversion
  b.n_w = (int)fminf(fmaxf(bw, 0.f), cap) + 1;
  b.n_h = (int)fminf(fmaxf(bh, 0.f), cap) + 1;
  b.gysl = (float)((double)(lby - lty) / (b.n_h + 1.));
  b.gysr = (float)((double)(rby - rty) / (b.n_h + 1.));
  b.gxst = (float)((double)(rtx - ltx) / (b.n_w + 1.));
  b.gxsb = (float)((double)(rbx - lbx) / (b.n_w + 1.));
  b.ltx = ltx; b.lbx = lbx; b.lty = lty; b.rty = rty;
  return b;
}

// sample coordinate k of a row / column (:263-264)
__device__ __forceinline__ float rot_coord(float a, float b, float sa, float sb, int k) {
  const double t = k + 1.;
  return (float)(((double)a + t * (double)sa + (double)b + t * (double)sb) / 2.);
}

// integer cell (truncated toward zero, clamped into [0, size-1] -- the reference reads outside the plane there), the
// clamped +1 neighbour and the reference's fraction v - (int)v.  (+0.f: trunc(-0.5) is -0.f, (float)(int)-0.5 is +0.f.)
__device__ __forceinline__ void rot_cell(float v, int size, int& i0, int& i1, float& f) {
  const float t = truncf(v) + 0.f;
  f = v - t;
  i0 = (int)fminf(fmaxf(t, 0.f), (float)(size - 1));
  i1 = min(i0 + 1, size - 1);
}

// VEC = channels per lane: 1 (any layout), or 2 for the NHWC form with an even bank and channel stride (each bilinear
// corner one 8-byte load: the gathers' address path is what bounds this family of kernels).
template <int VEC, bool USE_MAX>
__global__ __launch_bounds__(256, 4) void rotated_psroialign_fwd_kernel(const float* __restrict__ feat,
                                                                     const float* __restrict__ rois,
                                                                     const int32_t* __restrict__ orders,
                                                                     float* __restrict__ pooled,
                                                                     int32_t* __restrict__ index, int N, int C, int H,
                                                                     int W, int R, int gw, int gh, int layout, int ldc,
                                                                     int split) {
  const int bank = C / (gw * gh);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  // image order, ROI blocks and the one-ROI-per-workgroup split exactly as psroialign_fwd_kernel
  const int bpi = split ? R : (R + 3) >> 2;
  const int e_first = (split ? wave * 64 : 0) + lane, e_step = split ? 256 : 64;
  const int slot = blockIdx.x >> 3, xcd = blockIdx.x & 7;
  int64_t n;
  int rblk;
  if (N >= 8) {
    n = (int64_t)(slot / bpi) * 8 + xcd;
    rblk = slot % bpi;
  } else {
    const int P = 8 / N;
    n = xcd % N;
    rblk = slot * P + xcd / N;
    if (xcd >= N * P) return;
  }
  const int r_roi = split ? rblk : rblk * 4 + wave;
  if (n >= N || rblk >= bpi || r_roi >= R) return;
  const int64_t nr = n * R + r_roi;
  float* prow = pooled + nr * C;
  int32_t* irow = index ? index + nr * C : nullptr;
  float vy[4], vx[4];
  if (!rot_vertices(rois + nr * 8, orders[nr], H, W, vy, vx)) {   // degenerate: value 0 and index 0 (:205-211)
    for (int e = e_first; e < C; e += e_step) {
      prow[e] = 0.f;
      if (irow) irow[e] = 0;
    }
    return;
  }
  const int sy = layout == 0 ? W : W * ldc, sx = layout == 0 ? 1 : ldc, sc = layout == 0 ? H * W : 1;
  const float* __restrict__ fimg = feat + (size_t)n * H * W * ldc;       // NCHW: ldc == C
  typedef float vecf __attribute__((ext_vector_type(VEC)));
  auto ldv = [&](int off) {
    vecf r;
    if (VEC == 1) r[0] = fimg[off];
    else r = *reinterpret_cast<const vecf*>(fimg + off);                   // 8-byte aligned: even offset (launch check)
    return r;
  };
  constexpr int JMAX = VEC == 2 ? 6 : 8;      // hoisted sample columns (registers: 8 with two channels spill at four waves)
  for (int ev = e_first; ev * VEC < C; ev += e_step) {
    const int e = ev * VEC;                 // first of this lane's VEC channels (one bin: VEC divides bank)
    const int pos = e / bank, row = pos / gw;
    const RotBin bn = rot_bin(vy, vx, row, pos - row * gw, gw, gh, (float)(H + W));
    const int coff = e * sc;
    float acc[VEC];
    int arg[VEC];
#pragma unroll
    for (int u = 0; u < VEC; ++u) {
      acc[u] = USE_MAX ? -FLT_MAX : 0.f;
      arg[u] = 0;
    }
    // (1.-fx)*(1.-fy)*f00 + (1.-fx)*fy*f10 + fx*(1.-fy)*f01 in double, fx*fy*f11 in float, summed left to right (:273-276)
    auto blend = [&](double wx0, float fx, double wy0, float fy, vecf f00, vecf f10, vecf f01, vecf f11, int sidx) {
      const double w00 = wx0 * wy0, w10 = wx0 * (double)fy, w01 = (double)fx * wy0;
      const float fxfy = fx * fy;
#pragma unroll
      for (int u = 0; u < VEC; ++u) {
        const float t = (float)(w00 * f00[u] + w10 * f10[u] + w01 * f01[u] + fxfy * f11[u]);
        if (USE_MAX) {
          if (acc[u] < t) { acc[u] = t; arg[u] = sidx; }
        } else {
          acc[u] += t;
        }
      }
    };
    if (bn.n_w <= JMAX) {
      int xo0[JMAX], xo1[JMAX];
      float fxs[JMAX];
      double wx0[JMAX];
#pragma unroll
      for (int j = 0; j < JMAX; ++j) {
        if (j < bn.n_w) {
          int i0, i1;
          rot_cell(rot_coord(bn.ltx, bn.lbx, bn.gxst, bn.gxsb, j), W, i0, i1, fxs[j]);
          xo0[j] = i0 * sx + coff;
          xo1[j] = i1 * sx + coff;
          wx0[j] = 1. - fxs[j];
        }
      }
      for (int i = 0; i < bn.n_h; ++i) {
        int iy0, iy1;
        float fy;
        rot_cell(rot_coord(bn.lty, bn.rty, bn.gysl, bn.gysr, i), H, iy0, iy1, fy);
        const int yo0 = iy0 * sy, yo1 = iy1 * sy;
        const double wy0 = 1. - fy;
#pragma unroll
        for (int j = 0; j < JMAX; ++j) {
          if (j < bn.n_w)
            blend(wx0[j], fxs[j], wy0, fy, ldv(yo0 + xo0[j]), ldv(yo1 + xo0[j]), ldv(yo0 + xo1[j]), ldv(yo1 + xo1[j]),
                  bn.n_w * i + j);
        }
      }
    } else {                                  // wide bins: no bound on the sample count (a full-map 1 x 1 grid)
      for (int i = 0; i < bn.n_h; ++i) {
        int iy0, iy1;
        float fy;
        rot_cell(rot_coord(bn.lty, bn.rty, bn.gysl, bn.gysr, i), H, iy0, iy1, fy);
        const double wy0 = 1. - fy;
        for (int j = 0; j < bn.n_w; ++j) {
          int ix0, ix1;
          float fx;
          rot_cell(rot_coord(bn.ltx, bn.lbx, bn.gxst, bn.gxsb, j), W, ix0, ix1, fx);
          blend(1. - fx, fx, wy0, fy, ldv(iy0 * sy + ix0 * sx + coff), ldv(iy1 * sy + ix0 * sx + coff),
                ldv(iy0 * sy + ix1 * sx + coff), ldv(iy1 * sy + ix1 * sx + coff), bn.n_w * i + j);
        }
      }
    }
#pragma unroll
    for (int u = 0; u < VEC; ++u) {
      float a = acc[u];
      if (!USE_MAX) a /= (float)(bn.n_h * bn.n_w);
      prow[e + u] = a;
      if (irow) irow[e + u] = USE_MAX ? arg[u] : 0;
    }
  }
}

int launch_rotated_psroialign(const float* feat, const float* rois, const int32_t* orders, float* pooled,
                              int32_t* index, int N, int C, int H, int W, int R, int gw, int gh, int use_max,
                              int layout, int ldc, hipStream_t s) {
  // RotatedPSROIAlignOp::Compute (:320-343), plus what the reference leaves undefined (a zero grid divides by zero)
  XDET_REQUIRE(gw > 0 && gh > 0, "Need Attr grid_dim_width/grid_dim_height > 0");
  XDET_REQUIRE(N >= 0 && C > 0 && H > 0 && W > 0 && R >= 0, "inputs must be in 'NCHW' format.");
  XDET_REQUIRE(C % (gw * gh) == 0, "channels must be divisible by grid_dim_width * grid_dim_height");
  XDET_REQUIRE(layout == 0 || layout == 1, "feat_layout must be 0 (NCHW) or 1 (NHWC)");
  XDET_REQUIRE(ldc >= C, "channel stride must be >= C");
  XDET_REQUIRE(feat && rois && orders && pooled, "inputs/rois/orders/pooled_features must not be NULL");
  if ((int64_t)N * R == 0) return XDET_OK;
  // NCHW with enough ROIs: the one-time transpose to an NHWC scratch copy, then the two-channel NHWC kernel (as
  // launch_psroialign, same rule)
  if (layout == 0 && (C / (gw * gh)) % 2 == 0 && C % 2 == 0 && (int64_t)R * C >= (int64_t)4 * H * W) {
    float* scratch = nullptr;
    int rc = psroi_nhwc_scratch(feat, N, C, H, W, s, &scratch);
    if (rc != XDET_OK) return rc;
    if (scratch) {
      rc = launch_rotated_psroialign(scratch, rois, orders, pooled, index, N, C, H, W, R, gw, gh, use_max, 1, C, s);
      (void)hipFreeAsync(scratch, s);
      return rc;
    }
  }
  const int split = (int64_t)N * R <= 2048 ? 1 : 0;
  const int64_t bpi = split ? R : cdiv(R, 4);
  const int64_t blocks = N >= 8 ? cdiv(N, 8) * 8 * bpi : 8 * cdiv(bpi, 8 / N);
  const int bank = C / (gw * gh);
  const bool two = layout == 1 && bank % 2 == 0 && ldc % 2 == 0 && reinterpret_cast<uintptr_t>(feat) % 8 == 0;
  const int cs = layout == 0 ? C : ldc;
#define XDET_ROT_LAUNCH(V, M)                                                                                      \
  hipLaunchKernelGGL((rotated_psroialign_fwd_kernel<V, M>), dim3((unsigned)blocks), dim3(256), 0, s, feat, rois, \
                     orders, pooled, index, N, C, H, W, R, gw, gh, layout, cs, split)
  if (two && use_max) XDET_ROT_LAUNCH(2, true);
  else if (two) XDET_ROT_LAUNCH(2, false);
  else if (use_max) XDET_ROT_LAUNCH(1, true);
  else XDET_ROT_LAUNCH(1, false);
#undef XDET_ROT_LAUNCH
  XDET_LAUNCH_CHECK();
  return XDET_OK;
}

// Gradient: zero-fill, then one wave per ROI scatters grad * bilinear weight with float atomics
// ('max': the forward's argmax sample only; 'mean': every sample, grad / (n_h n_w) -- the CUDA kernel's scaling,
// rotated_ps_roi_align_grad_op.cu:132-166).  Same geometry and clamping as the forward.
__global__ __launch_bounds__(256) void rotated_psroialign_grad_kernel(const float* __restrict__ rois,
                                                                      const int32_t* __restrict__ orders,
                                                                      const float* __restrict__ grad_pooled,
                                                                      const int32_t* __restrict__ pooled_index,
                                                                      float* __restrict__ grad_out, int N, int C,
                                                                      int H, int W, int R, int gw, int gh,
                                                                      int use_max, int layout, int ldc) {
  const int bank = C / (gw * gh);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t nr = (int64_t)blockIdx.x * 4 + wave;
  if (nr >= (int64_t)N * R) return;
  const int64_t n = nr / R;
  float vy[4], vx[4];
  if (!rot_vertices(rois + nr * 8, orders[nr], H, W, vy, vx)) return;
  const int64_t sy = layout == 0 ? W : (int64_t)W * ldc, sx = layout == 0 ? 1 : ldc, sc = layout == 0 ? (int64_t)H * W : 1;
  float* __restrict__ gimg = grad_out + (size_t)n * H * W * ldc;
  for (int e = lane; e < C; e += 64) {
    const int pos = e / bank, row = pos / gw;
    const RotBin bn = rot_bin(vy, vx, row, pos - row * gw, gw, gh, (float)(H + W));
    const int64_t w = nr * C + e;
    float* __restrict__ gc = gimg + e * sc;
    const int pi = use_max ? pooled_index[w] : 0;
    const int i_lo = use_max ? pi / bn.n_w : 0, i_hi = use_max ? i_lo + 1 : bn.n_h;
    const int j_lo = use_max ? pi % bn.n_w : 0, j_hi = use_max ? j_lo + 1 : bn.n_w;
    const float g = use_max ? grad_pooled[w] : grad_pooled[w] / (float)(bn.n_w * bn.n_h);
    for (int i = i_lo; i < i_hi; ++i) {
      int iy0, iy1;
      float fy;
      rot_cell(rot_coord(bn.lty, bn.rty, bn.gysl, bn.gysr, i), H, iy0, iy1, fy);
      for (int j = j_lo; j < j_hi; ++j) {
        int ix0, ix1;
        float fx;
        rot_cell(rot_coord(bn.ltx, bn.lbx, bn.gxst, bn.gxsb, j), W, ix0, ix1, fx);
        atomicAdd(gc + iy0 * sy + ix0 * sx, (float)((1. - fx) * (1. - fy) * g));
        atomicAdd(gc + iy1 * sy + ix0 * sx, (float)((1. - fx) * fy * g));
        atomicAdd(gc + iy0 * sy + ix1 * sx, (float)(fx * (1. - fy) * g));
        atomicAdd(gc + iy1 * sy + ix1 * sx, (float)(fx * fy * g));
      }
    }
  }
}

int launch_rotated_psroialign_grad(const float* rois, const int32_t* orders, const float* grad_pooled,
                                   const int32_t* pooled_index, float* grad_out, int N, int C, int H, int W, int R,
                                   int gw, int gh, int use_max, int layout, int ldc, hipStream_t s) {
  // RotatedPSROIAlignGradOp::Compute (:408-436)
  XDET_REQUIRE(gw > 0 && gh > 0, "Need Attr grid_dim_width/grid_dim_height > 0");
  XDET_REQUIRE(N >= 0 && C > 0 && H > 0 && W > 0 && R >= 0, "inputs must be in 'NCHW' format.");
  XDET_REQUIRE(C % (gw * gh) == 0, "channels must be divisible by grid_dim_width * grid_dim_height");
  XDET_REQUIRE(layout == 0 || layout == 1, "feat_layout must be 0 (NCHW) or 1 (NHWC)");
  XDET_REQUIRE(ldc >= C, "channel stride must be >= C");
  XDET_REQUIRE(rois && orders && grad_pooled && grad_out && (!use_max || pooled_index),
               "rotated_psroialign_grad: NULL argument");
  XDET_HIP(hipMemsetAsync(grad_out, 0, (size_t)N * ldc * H * W * sizeof(float), s));
  const int64_t n_waves = (int64_t)N * R;
  if (n_waves == 0) return XDET_OK;
  hipLaunchKernelGGL(rotated_psroialign_grad_kernel, dim3((unsigned)cdiv(n_waves, 4)), dim3(256), 0, s, rois, orders,
                     grad_pooled, pooled_index, grad_out, N, C, H, W, R, gw, gh, use_max, layout, ldc);
  XDET_LAUNCH_CHECK();
  return XDET_OK;
}

}  // namespace xdet
