// PsRoiAlignGrad with a fixed summation order: the training backward of csrc/psroialign.hip's forward as a pure
// function of its inputs -- no float atomics, bit-identical to a sequential evaluation.
//
// THIS FILE IS COMPILED WITH -ffp-contract=off: the geometry is the forward's fixed sequence of separately rounded f32
// operations, the weights are double products cast to float, and every accumulation is one rounded f32 add.
//
// The order rule, per output element grad_feat[n, c, y, x]: contributions arrive in the order ROI index r, sample row i,
// sample column j, then the corners (iy,ix), (iy1,ix), (iy,ix1), (iy1,ix1).  Channel c = pos*bank + ch of image n only
// receives from bin pos of that image's ROIs, so ONE LANE owns the whole H x W plane of one (n, c): it walks the image's
// ROIs in index order and never meets another lane.  A workgroup is one wavefront; its lanes own `cpw` neighbouring
// channels whose planes live in LDS as [pixel][cpw] (lanes of one pixel on neighbouring banks; the NHWC write-out is a
// straight copy), at most 160 KB.  Nothing is accumulated in global memory and every element of grad_feat is written.
//
// What is the same for every lane -- the ROI geometry, which depends on (n, r) alone -- is computed 64 ROIs at a time, one
// ROI per lane, into a small LDS table and read back by broadcast; grad_pooled / pooled_index rows are fetched one batch of
// PB ROIs ahead of their use.  What is left on the chain of R ROIs is one LDS round trip per sample.
#include "common.h"
#include <cfloat>

namespace xdet {

constexpr int kOrdGeoWords = 8;          // per ROI: ymin, xmin, bin_h, bin_w, step_h, step_w, n_h, n_w (n_h = 0: contributes nothing)
constexpr int kOrdGeoBytes = 64 * kOrdGeoWords * 4;
constexpr int kOrdLdsBytes = 160 * 1024;
constexpr int kOrdPlaneFloats = (kOrdLdsBytes - kOrdGeoBytes) / 4;
static_assert(kOrdPlaneFloats == XDET_PSROIALIGN_GRAD_ORDERED_MAX_PIXELS, "include/xdet.h documents the pixel limit");
constexpr int PB = 8;                    // ROIs per prefetched batch of gradient / index rows (divides 64)

// One sample's four corner updates on the lane's own plane (element stride cs), in the order (iy,ix), (iy1,ix), (iy,ix1),
// (iy1,ix1), each a separately rounded add.  The four reads are issued together and the aliasing of clamped corners
// (iy1 == iy on the last row, ix1 == ix on the last column) is resolved in registers: the value a later corner adds to is
// the one an earlier corner left at that address.  The stores go out in corner order, so the last one to an address stays.
__device__ __forceinline__ void ordered_sample(float* __restrict__ plane, int cs, int H, int W, float x, float y, float g) {
  if (!(x >= 0.f && x < (float)W && y >= 0.f && y < (float)H)) return;   // (never for a valid sample: nothing leaves the plane)
  const int ix = (int)x, iy = (int)y;
  const float fx = x - (float)ix, fy = y - (float)iy;
  const int iy1 = min(iy + 1, H - 1), ix1 = min(ix + 1, W - 1);
  const float w00 = (float)((1. - fx) * (1. - fy) * g);
  const float w10 = (float)((1. - fx) * fy * g);
  const float w01 = (float)(fx * (1. - fy) * g);
  const float w11 = (float)(fx * fy * g);
  float* p00 = plane + (iy * W + ix) * cs;
  float* p10 = plane + (iy1 * W + ix) * cs;
  float* p01 = plane + (iy * W + ix1) * cs;
  float* p11 = plane + (iy1 * W + ix1) * cs;
  const bool same_row = iy1 == iy, same_col = ix1 == ix;
  const float a = *p00, b = *p10, c = *p01, d = *p11;
  const float v00 = a + w00;
  const float v10 = (same_row ? v00 : b) + w10;
  const float v01 = (same_col ? (same_row ? v10 : v00) : c) + w01;
  const float v11 = (same_row ? v01 : same_col ? v10 : d) + w11;
  *p00 = v00;
  *p10 = v10;
  *p01 = v01;
  *p11 = v11;
}

template <bool USE_MAX>
__global__ __launch_bounds__(64) void psroialign_grad_ordered_kernel(const float* __restrict__ rois,
                                                                    const float* __restrict__ grad_pooled, int ld_grad,
                                                                    const int32_t* __restrict__ pooled_index, int ld_index,
                                                                    float* __restrict__ grad_out, int C, int H, int W, int R,
                                                                    int gw, int gh, int layout, int ldc, int corners, int cpw,
                                                                    int chunks) {
  extern __shared__ __attribute__((aligned(16))) float s_mem[];
  float* s_geo = s_mem;                                   // [64 ROIs][kOrdGeoWords]
  float* s_planes = s_mem + 64 * kOrdGeoWords;            // [H*W][cpw]
  const int lane = threadIdx.x;
  const int n = blockIdx.x / chunks, chunk = blockIdx.x - n * chunks;
  const int c0 = chunk * cpw, cnt = min(cpw, C - c0);
  const int HW = H * W;
  const bool active = lane < cnt;
  const int c = c0 + lane;
  const int bank = C / (gw * gh);
  const int pos = (active ? c : c0) / bank, row = pos / gw, col = pos - row * gw;
  float* plane = s_planes + lane;

  for (int e = lane; e < HW * cpw; e += 64) s_planes[e] = 0.f;

  const float* grow = grad_pooled + (int64_t)n * R * ld_grad + c;
  const int32_t* irow = USE_MAX ? pooled_index + (int64_t)n * R * ld_index + c : nullptr;   // 'mean' never reads it
  float g_cur[PB], g_nxt[PB];
  int p_cur[PB], p_nxt[PB];
  auto fetch = [&](int r_first, float (&g)[PB], int (&p)[PB]) {
#pragma unroll
    for (int k = 0; k < PB; ++k) {
      const int r = r_first + k;
      const bool on = active && r < R;
      g[k] = on ? grow[(int64_t)r * ld_grad] : 0.f;
      p[k] = (USE_MAX && on) ? irow[(int64_t)r * ld_index] : 0;
    }
  };
  fetch(0, g_cur, p_cur);

  for (int rb = 0; rb < R; rb += 64) {
    __syncthreads();                                      // the table's readers of the last round are done
    {
      // geometry of ROI rb + lane: the forward's literal sequence (psroialign_fwd_kernel)
      const int r = rb + lane;
      float o[kOrdGeoWords] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      if (r < R) {
        const float* roi = rois + ((int64_t)n * R + r) * 4;
        float r0 = roi[0], r1 = roi[1], r2 = roi[2], r3 = roi[3];
        if (corners) {   // _point2center, as the forward
          const float hh = r2 - r0, ww = r3 - r1;
          r0 = r0 + hh / 2.f;
          r1 = r1 + ww / 2.f;
          r2 = hh;
          r3 = ww;
        }
        if (!(r2 < FLT_MIN || r3 < FLT_MIN)) {
          const float yc = r0 * (float)H, xc = r1 * (float)W;
          const float rh = fmaxf(r2 * (float)H, 1.f), rw = fmaxf(r3 * (float)W, 1.f);
          const float ymin = fmaxf(yc - rh / 2.f, 0.f), xmin = fmaxf(xc - rw / 2.f, 0.f);
          const float ymax = fminf(yc + rh / 2.f, (float)H - FLT_MIN), xmax = fminf(xc + rw / 2.f, (float)W - FLT_MIN);
          const float bin_w = (xmax - xmin) / (float)gw, bin_h = (ymax - ymin) / (float)gh;
          const int n_w = (int)bin_w + 1, n_h = (int)bin_h + 1;
          if (n_w >= 1 && n_h >= 1) {                     // (a non-finite box: nothing)
            o[0] = ymin; o[1] = xmin; o[2] = bin_h; o[3] = bin_w;
            o[4] = bin_h / (float)n_h;
            o[5] = bin_w / (float)n_w;
            o[6] = __int_as_float(n_h);
            o[7] = __int_as_float(n_w);
          }
        }
      }
      float4* dst = reinterpret_cast<float4*>(s_geo + lane * kOrdGeoWords);
      dst[0] = make_float4(o[0], o[1], o[2], o[3]);
      dst[1] = make_float4(o[4], o[5], o[6], o[7]);
    }
    __syncthreads();
    const int kend = min(64, R - rb);
    for (int kb = 0; kb < kend; kb += PB) {
      fetch(rb + kb + PB, g_nxt, p_nxt);                  // one batch ahead (64 is a multiple of PB: rounds join up)
#pragma unroll
      for (int k = 0; k < PB; ++k) {
        if (kb + k >= kend) break;
        const float grad = g_cur[k];
        // a ROI whose gradient is zero on all of this workgroup's channels adds +-0 terms only: skipped (OHEM)
        if (__builtin_amdgcn_ballot_w64(grad != 0.f) == 0) continue;
        const float4 ga = reinterpret_cast<const float4*>(s_geo + (kb + k) * kOrdGeoWords)[0];
        const float4 gb = reinterpret_cast<const float4*>(s_geo + (kb + k) * kOrdGeoWords)[1];
        const int n_h = __float_as_int(gb.z), n_w = __float_as_int(gb.w);
        if (n_h == 0 || !active) continue;
        const float step_h = gb.x, step_w = gb.y;
        const float x0 = ga.y + ga.w * (float)col, y0 = ga.x + ga.z * (float)row;
        const double half_w = (double)step_w / 2., half_h = (double)step_h / 2.;
        if (USE_MAX) {
          const int pi = p_cur[k];
          if (pi < 0) continue;
          const int i = pi / n_w, j = pi - i * n_w;
          if (i >= n_h) continue;                         // an index outside [0, n_h n_w): nothing
          const float y = (float)((double)(y0 + step_h * (float)i) + half_h);
          const float x = (float)((double)(x0 + step_w * (float)j) + half_w);
          ordered_sample(plane, cpw, H, W, x, y, grad);
        } else {
          const float g = grad / (float)(n_w * n_h);
          for (int i = 0; i < n_h; ++i) {
            const float y = (float)((double)(y0 + step_h * (float)i) + half_h);
            for (int j = 0; j < n_w; ++j) {
              const float x = (float)((double)(x0 + step_w * (float)j) + half_w);
              ordered_sample(plane, cpw, H, W, x, y, g);
            }
          }
        }
      }
#pragma unroll
      for (int k = 0; k < PB; ++k) {
        g_cur[k] = g_nxt[k];
        p_cur[k] = p_nxt[k];
      }
    }
  }
  __syncthreads();

  // write-out: every element of this workgroup's channels, and (NHWC, last chunk) the padding channels [C, ldc) as zeros
  if (layout == 1) {
    float* o = grad_out + (int64_t)n * HW * ldc;
    for (int p = 0; p < HW; ++p)
      if (active) o[(int64_t)p * ldc + c] = s_planes[p * cpw + lane];
    if (chunk == chunks - 1)
      for (int p = 0; p < HW; ++p)
        for (int cc = C + lane; cc < ldc; cc += 64) o[(int64_t)p * ldc + cc] = 0.f;
  } else {
    for (int l = 0; l < cnt; ++l) {
      float* o = grad_out + ((int64_t)n * C + c0 + l) * HW;
      for (int p = lane; p < HW; p += 64) o[p] = s_planes[p * cpw + l];
    }
  }
}

int launch_psroialign_grad_ordered(const float* rois, const float* grad_pooled, int ld_grad, const int32_t* pooled_index,
                                   int ld_index, float* grad_out, int N, int C, int H, int W, int R, int gw, int gh,
                                   int use_max, int layout, int ldc, int corners, hipStream_t s) {
  XDET_REQUIRE(gw > 0 && gh > 0, "psroialign_grad_ordered: Need Attr grid_dim_width/grid_dim_height > 0");
  XDET_REQUIRE(N >= 0 && C > 0 && H > 0 && W > 0 && R >= 0, "psroialign_grad_ordered: inputs must be in 'NCHW' format.");
  XDET_REQUIRE(C % (gw * gh) == 0, "psroialign_grad_ordered: channels must be divisible by grid_dim_width * grid_dim_height");
  XDET_REQUIRE(layout == 0 || layout == 1, "psroialign_grad_ordered: feat_layout must be 0 (NCHW) or 1 (NHWC)");
  XDET_REQUIRE(rois && grad_pooled && grad_out && (!use_max || pooled_index), "psroialign_grad_ordered: NULL argument");
  const int cs = layout == 0 ? C : ldc;
  XDET_REQUIRE(cs >= C, "psroialign_grad_ordered: channel stride must be >= C");
  XDET_REQUIRE(ld_grad >= C && (!pooled_index || ld_index >= C), "psroialign_grad_ordered: ld_grad and ld_index must be >= C");
  XDET_REQUIRE((int64_t)H * W <= XDET_PSROIALIGN_GRAD_ORDERED_MAX_PIXELS,
               "psroialign_grad_ordered: H * W exceeds XDET_PSROIALIGN_GRAD_ORDERED_MAX_PIXELS (one plane must fit the "
               "workgroup's LDS); xdet_psroialign_grad takes maps of any size");
  XDET_REQUIRE((int64_t)N * cs * H * W < ((int64_t)1 << 40) && (int64_t)N * R < ((int64_t)1 << 31),
               "psroialign_grad_ordered: tensor too large");
  if (N == 0) return XDET_OK;
  const int HW = H * W;
  // channels per workgroup: as many planes as the LDS holds (one lane each), then evened out over the chunks; the NCHW
  // write-out reads a channel's pixels at stride cpw, so an odd cpw keeps it off one bank
  const int cap = layout == 0 ? 63 : 64;
  int cpw = std::min(std::min(cap, kOrdPlaneFloats / HW), C);
  cpw = (int)cdiv(C, cdiv(C, cpw));
  if (layout == 0 && cpw > 1 && cpw % 2 == 0 && (int64_t)(cpw + 1) * HW <= kOrdPlaneFloats) ++cpw;   // (even: below the cap)
  const int n_chunks = (int)cdiv(C, cpw);
  const size_t lds = (size_t)kOrdGeoBytes + (size_t)cpw * HW * sizeof(float);
#define XDET_ORD_LAUNCH(M)                                                                                                   \
  do {                                                                                                                       \
    static DeviceOnce once;                                                                                                  \
    XDET_TRY(ensure_dynamic_lds(once, reinterpret_cast<const void*>(&psroialign_grad_ordered_kernel<M>), kOrdLdsBytes));       \
    hipLaunchKernelGGL((psroialign_grad_ordered_kernel<M>), dim3((unsigned)((int64_t)N * n_chunks)), dim3(64), lds, s, rois,   \
                       grad_pooled, ld_grad, pooled_index, ld_index, grad_out, C, H, W, R, gw, gh, layout, cs, corners, cpw,   \
                       n_chunks);                                                                                            \
  } while (0)
  if (use_max) XDET_ORD_LAUNCH(true);
  else XDET_ORD_LAUNCH(false);
#undef XDET_ORD_LAUNCH
  XDET_LAUNCH_CHECK();
  return XDET_OK;
}

}  // namespace xdet
