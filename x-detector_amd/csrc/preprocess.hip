// F1: the step right before the hot path, fused into one kernel --
// light_head_preprocess_for_eval / _for_test (preprocessing/common_preprocessing.py:383-458):
//   uint8 HWC image -> tf.image.convert_image_dtype(float32) * 2 - [R,G,B mean]/127.5
//   -> tf.image.resize_images(BILINEAR, align_corners=False) warp to SxS (tf_image.py:307-319)
//   -> HWC -> CHW (data_format 'NCHW').
// TF1 legacy bilinear: src = dst * (in/out) (no half-pixel centre), lower = trunc(src),
// upper = min(lower+1, in-1), lerp = src - lower; top/bottom lerp in x, then lerp in y.
// Compiled with -ffp-contract=off so every product/sum rounds as TF's separate f32 ops do.
#include "common.h"

#include <algorithm>

namespace xdet {

__device__ __forceinline__ float whiten(unsigned char u, float mean) {
  return ((float)u * (1.0f / 255.0f)) * 2.0f - mean;
}

__global__ void preprocess_eval_kernel(const unsigned char* __restrict__ img, int H, int W, float* __restrict__ out,
                                       int S, float hscale, float wscale) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= S * S) return;
  const int oy = i / S, ox = i - oy * S;
  const float fy = (float)oy * hscale, fx = (float)ox * wscale;
  const int y0 = (int)fy, x0 = (int)fx;
  const int y1 = min(y0 + 1, H - 1), x1 = min(x0 + 1, W - 1);
  const float ly = fy - (float)y0, lx = fx - (float)x0;
  const float means[3] = {123.68f / 127.5f, 116.78f / 127.5f, 103.94f / 127.5f};
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float tl = whiten(img[((size_t)y0 * W + x0) * 3 + c], means[c]);
    const float tr = whiten(img[((size_t)y0 * W + x1) * 3 + c], means[c]);
    const float bl = whiten(img[((size_t)y1 * W + x0) * 3 + c], means[c]);
    const float br = whiten(img[((size_t)y1 * W + x1) * 3 + c], means[c]);
    const float top = tl + (tr - tl) * lx;
    const float bot = bl + (br - bl) * lx;
    out[(size_t)c * S * S + i] = top + (bot - top) * ly;
  }
}

int launch_preprocess_eval(const unsigned char* img, int H, int W, float* out_chw, int S, hipStream_t s) {
  XDET_REQUIRE(img && out_chw && H > 0 && W > 0 && S > 0, "preprocess: bad arguments");
  const float hscale = (float)H / (float)S, wscale = (float)W / (float)S;
  hipLaunchKernelGGL(preprocess_eval_kernel, dim3((unsigned)cdiv((int64_t)S * S, 256)), dim3(256), 0, s, img, H, W,
                     out_chw, S, hscale, wscale);
  XDET_LAUNCH_CHECK();
  return XDET_OK;
}

// ---- ragged batch ingest: light_head_preprocess_for_eval with its `resize` argument --------------------------------
// (common_preprocessing.py:29-32,383-440; tf_image.resize_image_bboxes_with_crop_or_pad / bboxes_crop_or_pad
// :179-305).  Sizes come from device memory (image_shapes, offsets), never from kernel arguments, so one captured graph
// serves any mix of image sizes.  Each workgroup derives its image's geometry itself; every value below is wave-uniform.
namespace {

constexpr int PB_T = 256;           // threads per workgroup
constexpr int PB_ITEMS = 1024;      // (row, 4-column quad) items per workgroup: a band of rows

// Where the resized image sits in the S x S output: rows [py, py + ih) x columns [px, px + iw) hold it, the rest is the
// (whitened-space) zero pad.  Inside, output (y, x) samples the source at
//   bilinear: TF-legacy src = (y - py) * hs, (x - px) * ws over the whole H x W image   (WARP, PAD_AND_RESIZE)
//   direct:   source pixel (y - py + cy, x - px + cx)                                     (CENTRAL_CROP, NONE)
// bbox_img = [0,0,1,1] through bboxes_crop_or_pad twice (crop step, pad step), each b*[h,w,h,w] + offset, / target.
struct PbGeom {
  bool valid, bilinear;
  int H, W, py, px, ih, iw, cy, cx;
  float hs, ws;
  float4 bbox;
};

__device__ __forceinline__ int floordiv2(int a) { return a >= 0 ? a / 2 : -((1 - a) / 2); }   // Python a // 2

// one bboxes_crop_or_pad step on the [0,0,1,1]-derived box b (tf_image.py:179-203), in f32 and in TF's order
__device__ __forceinline__ float4 crop_or_pad_step(float4 b, int h, int w, int oy, int ox, int th, int tw) {
  return make_float4((b.x * (float)h + (float)oy) / (float)th, (b.y * (float)w + (float)ox) / (float)tw,
                     (b.z * (float)h + (float)oy) / (float)th, (b.w * (float)w + (float)ox) / (float)tw);
}

__device__ PbGeom pb_geometry(int64_t packed_bytes, int64_t offset, int H, int W, int S, int mode) {
  PbGeom g;
  g.H = H; g.W = W;
  g.valid = H > 0 && W > 0 && offset >= 0 && offset <= packed_bytes &&
            (int64_t)H * (int64_t)W <= (packed_bytes - offset) / 3;
  g.bilinear = mode == XDET_RESIZE_WARP || mode == XDET_RESIZE_PAD_AND_RESIZE;
  g.py = g.px = g.cy = g.cx = 0;
  g.ih = g.iw = S;
  g.hs = g.ws = 1.f;
  g.bbox = make_float4(0.f, 0.f, 1.f, 1.f);
  int h = H, w = W;                                  // the image entering resize_image_bboxes_with_crop_or_pad
  if (mode == XDET_RESIZE_NONE) {
    g.valid = g.valid && H == S && W == S;
  } else if (mode == XDET_RESIZE_WARP) {
    if (g.valid) { g.hs = (float)H / (float)S; g.ws = (float)W / (float)S; }
  } else {
    if (mode == XDET_RESIZE_PAD_AND_RESIZE && g.valid) {
      // factor = min(1, min(S/H, S/W)) in f64; resize_shape = (int32)floor(factor * (H, W))  (:405-410)
      const double factor = fmin(1.0, fmin((double)S / (double)H, (double)S / (double)W));
      h = (int)floor(factor * (double)H);
      w = (int)floor(factor * (double)W);
      g.valid = h > 0 && w > 0;
      if (g.valid) { g.hs = (float)H / (float)h; g.ws = (float)W / (float)w; }
    }
    if (g.valid) {
      // tf_image.py:261-289: offset_crop = max((h - S) // 2, 0), offset_pad = max((S - h) // 2, 0), per axis
      g.cy = max(floordiv2(h - S), 0);
      g.cx = max(floordiv2(w - S), 0);
      g.py = max(floordiv2(S - h), 0);
      g.px = max(floordiv2(S - w), 0);
      g.ih = min(S, h);
      g.iw = min(S, w);
      g.bbox = crop_or_pad_step(g.bbox, h, w, -g.cy, -g.cx, g.ih, g.iw);
      g.bbox = crop_or_pad_step(g.bbox, g.ih, g.iw, g.py, g.px, S, S);
    }
  }
  if (!g.valid) g.bbox = make_float4(NAN, NAN, NAN, NAN);
  return g;
}

__device__ __forceinline__ float whiten_at(const unsigned char* __restrict__ img, int64_t pix, int c, float mean) {
  return whiten(img[pix * 3 + c], mean);
}

}  // namespace

// grid (bands of rows, N), PB_T threads.  Output-stationary: one item = one output row's 4 consecutive columns in all
// three planes (three float4 stores when VEC).  Pad items only store zeros; an invalid descriptor stores NaN everywhere.
template <bool VEC>
__global__ __launch_bounds__(PB_T) void preprocess_batch_kernel(const unsigned char* __restrict__ packed,
                                                                int64_t packed_bytes,
                                                                const int64_t* __restrict__ offsets,
                                                                const int* __restrict__ image_shapes, int S, int mode,
                                                                int rows_per_band, float* __restrict__ out,
                                                                float* __restrict__ bbox_img) {
  const int n = blockIdx.y;
  const int64_t off = offsets[n];
  const PbGeom g = pb_geometry(packed_bytes, off, image_shapes[2 * n], image_shapes[2 * n + 1], S, mode);
  if (blockIdx.x == 0 && threadIdx.x == 0) *reinterpret_cast<float4*>(bbox_img + 4 * n) = g.bbox;

  const unsigned char* img = packed + (g.valid ? off : 0);
  const float means[3] = {123.68f / 127.5f, 116.78f / 127.5f, 103.94f / 127.5f};
  const int Q = (S + 3) / 4;
  const int y_begin = blockIdx.x * rows_per_band;
  const int items = min(rows_per_band, S - y_begin) * Q;
  const size_t plane = (size_t)S * S;
  float* const o = out + (size_t)n * 3 * plane;
  for (int it = threadIdx.x; it < items; it += PB_T) {
    const int oy = y_begin + it / Q;
    const int ox0 = (it % Q) * 4;
    float v[3][4];
    const int iy = oy - g.py;
    const bool row_in = g.valid && iy >= 0 && iy < g.ih;
    int y0 = 0, y1 = 0;
    float ly = 0.f;
    if (row_in) {
      if (g.bilinear) {
        const float fy = (float)iy * g.hs;
        y0 = min((int)fy, g.H - 1);
        y1 = min(y0 + 1, g.H - 1);
        ly = fy - (float)y0;
      } else {
        y0 = iy + g.cy;
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int ix = ox0 + j - g.px;
      if (!g.valid) {
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c][j] = NAN;
      } else if (!row_in || ix < 0 || ix >= g.iw) {
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c][j] = 0.f;
      } else if (g.bilinear) {
        const float fx = (float)ix * g.ws;
        const int x0 = min((int)fx, g.W - 1);
        const int x1 = min(x0 + 1, g.W - 1);
        const float lx = fx - (float)x0;
        const int64_t r0 = (int64_t)y0 * g.W, r1 = (int64_t)y1 * g.W;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const float tl = whiten_at(img, r0 + x0, c, means[c]);
          const float tr = whiten_at(img, r0 + x1, c, means[c]);
          const float bl = whiten_at(img, r1 + x0, c, means[c]);
          const float br = whiten_at(img, r1 + x1, c, means[c]);
          const float top = tl + (tr - tl) * lx;
          const float bot = bl + (br - bl) * lx;
          v[c][j] = top + (bot - top) * ly;
        }
      } else {
        const int64_t p = (int64_t)y0 * g.W + (ix + g.cx);
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c][j] = whiten_at(img, p, c, means[c]);
      }
    }
    float* const dst = o + (size_t)oy * S + ox0;
    if (VEC) {
#pragma unroll
      for (int c = 0; c < 3; ++c)
        *reinterpret_cast<float4*>(dst + c * plane) = make_float4(v[c][0], v[c][1], v[c][2], v[c][3]);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (ox0 + j < S) {
#pragma unroll
          for (int c = 0; c < 3; ++c) dst[c * plane + j] = v[c][j];
        }
    }
  }
}

int launch_preprocess_batch(const unsigned char* packed, int64_t packed_bytes, const int64_t* offsets,
                            const int* image_shapes, int N, int S, int mode, float* out_nchw, float* bbox_img,
                            hipStream_t s) {
  XDET_REQUIRE(packed && offsets && image_shapes && out_nchw && bbox_img, "preprocess_batch: NULL argument");
  XDET_REQUIRE(N > 0 && N <= 65535 && S > 0 && packed_bytes >= 0, "preprocess_batch: bad sizes");
  XDET_REQUIRE(mode >= XDET_RESIZE_NONE && mode <= XDET_RESIZE_WARP, "preprocess_batch: unknown resize mode");
  XDET_REQUIRE(((uintptr_t)bbox_img & 15) == 0, "preprocess_batch: bbox_img must be 16-byte aligned");
  const int Q = (S + 3) / 4;
  const int rows = std::max(1, PB_ITEMS / Q);
  const dim3 grid((unsigned)cdiv(S, rows), (unsigned)N);
  if (S % 4 == 0 && ((uintptr_t)out_nchw & 15) == 0)
    hipLaunchKernelGGL(preprocess_batch_kernel<true>, grid, dim3(PB_T), 0, s, packed, packed_bytes, offsets,
                       image_shapes, S, mode, rows, out_nchw, bbox_img);
  else
    hipLaunchKernelGGL(preprocess_batch_kernel<false>, grid, dim3(PB_T), 0, s, packed, packed_bytes, offsets,
                       image_shapes, S, mode, rows, out_nchw, bbox_img);
  XDET_LAUNCH_CHECK();
  return XDET_OK;
}

}  // namespace xdet
