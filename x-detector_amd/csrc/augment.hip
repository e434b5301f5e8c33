// Training ingest -- light_head_preprocess_for_train (preprocessing/common_preprocessing.py:328-381): random colour
// distortion (distort_color, fast_mode=False, :212-262), SSD expand and patch sampling
// (tf_image.ssd_random_sample_patch_wrapper :602-630, ssd_random_expand :547-571, ssd_random_sample_patch :393-545), random
// horizontal flip (tf_image.random_flip_left_right :322-346), TF-legacy bilinear warp to S x S, * 2 - [R,G,B mean]/127.5,
// HWC -> CHW -- for a ragged batch of uint8 images, with the ground-truth boxes transformed and filtered alongside.
// The contract (draws, operation order, the fixed-point contrast mean, the record) is stated in xdet/augment.py and
// include/xdet.h; host_preprocess_train there is what these kernels are compared with, bit for bit.  Compiled with
// -ffp-contract=off: every product and sum rounds on its own.
//   augment_geometry_kernel  one wavefront per image: every draw, the whole box side, the record
//   augment_mean_kernel      per-channel fixed-point sums of the partially distorted source image (contrast mean)
//   augment_finish_kernel    sums -> the record's three means; copies the record out
//   augment_pixels_kernel    output-stationary gather: flip / crop / canvas mapping, colour chain per tap, blend, whiten
// Sizes and ground truth come from device memory, as in preprocess_batch_kernel; nothing of the canvas or of the
// distorted full-size image is ever materialised.
#include "common.h"
#include "shuffle.h"

#include <algorithm>

namespace xdet {
namespace {

constexpr int AUG_MAX_GT = 512;
constexpr int AUG_WAVE = 64;
constexpr int AUG_MEAN_BLOCKS = 16;   // workgroups per image in the mean kernel
constexpr int AUG_T = 256;
constexpr int AUG_ITEMS = 1024;       // (row, 4-column quad) items per workgroup of the pixel kernel

// xdet/augment.py RECORD_DTYPE
struct AugRecord {
  int valid;
  int canvas_h, canvas_w, off_y, off_x;
  int crop_y, crop_x, crop_h, crop_w;
  int flip, sel;
  float brightness, saturation, hue, contrast;
  float mean[3];
  int attempts, fallback, n_draws, expanded, min_iou, tiny_patch, min_iou_mask, expand_mask, n_in, n_out;
  int reserved[4];
};
static_assert(sizeof(AugRecord) == 128, "the record is 32 words");

struct AugWorkspace {
  AugRecord* rec;              // [N]
  unsigned long long* sums;    // [N][4] two's-complement fixed-point sums (R, G, B, unused)
};

// the select forms of the contract: max(a, b) = a < b ? b : a, min(a, b) = b < a ? b : a
__device__ __forceinline__ float smax(float a, float b) { return a < b ? b : a; }
__device__ __forceinline__ float smin(float a, float b) { return b < a ? b : a; }
__device__ __forceinline__ float clip01(float x) { return smin(smax(x, 0.f), 1.f); }

__device__ __forceinline__ bool aug_valid(int64_t packed_bytes, int64_t off, int H, int W) {
  return H > 0 && W > 0 && off >= 0 && off <= packed_bytes && (int64_t)H * (int64_t)W <= (packed_bytes - off) / 3;
}

// ---- colour ----------------------------------------------------------------------------------------------------------
struct Rgb { float r, g, b; };
struct Hsv { float h, s, v; };
struct AugColor { float brightness, saturation, hue, contrast, m0, m1, m2; };

__device__ __forceinline__ Hsv rgb_to_hsv(Rgb c) {
  const float V = smax(smax(c.r, c.g), c.b);
  const float rng = V - smin(smin(c.r, c.g), c.b);
  Hsv o;
  o.s = V > 0.f ? rng / V : 0.f;
  const float norm = 1.f / (6.f * rng);
  float h = c.r == V ? norm * (c.g - c.b)
                     : (c.g == V ? norm * (c.b - c.r) + (float)(2.0 / 6.0) : norm * (c.r - c.g) + (float)(4.0 / 6.0));
  h = rng > 0.f ? h : 0.f;
  o.h = h < 0.f ? h + 1.f : h;
  o.v = V;
  return o;
}

__device__ __forceinline__ Rgb hsv_to_rgb(Hsv c) {
  const float dh = c.h * 6.f;
  const float dr = clip01(fabsf(dh - 3.f) - 1.f);
  const float dg = clip01(2.f - fabsf(dh - 2.f));
  const float db = clip01(2.f - fabsf(dh - 4.f));
  const float oms = 1.f - c.s;
  Rgb o;
  o.r = (oms + c.s * dr) * c.v;
  o.g = (oms + c.s * dg) * c.v;
  o.b = (oms + c.s * db) * c.v;
  return o;
}

__device__ __forceinline__ Rgb op_brightness(Rgb c, const AugColor& k) {
  c.r = c.r + k.brightness; c.g = c.g + k.brightness; c.b = c.b + k.brightness;
  return c;
}
__device__ __forceinline__ Rgb op_saturation(Rgb c, const AugColor& k) {
  Hsv h = rgb_to_hsv(c);
  h.s = clip01(h.s * k.saturation);
  return hsv_to_rgb(h);
}
__device__ __forceinline__ Rgb op_hue(Rgb c, const AugColor& k) {
  Hsv h = rgb_to_hsv(c);
  const float t = h.h + k.hue;
  h.h = t - floorf(t);
  return hsv_to_rgb(h);
}
__device__ __forceinline__ Rgb op_contrast(Rgb c, const AugColor& k) {
  c.r = (c.r - k.m0) * k.contrast + k.m0;
  c.g = (c.g - k.m1) * k.contrast + k.m1;
  c.b = (c.b - k.m2) * k.contrast + k.m2;
  return c;
}

// orderings 0: B S H C   1: S B C H   2: C H B S   3: H S C B.  FULL = false: the ops in front of the contrast (what the
// contrast mean is taken over).  One instantiation per ordering: no op is chosen through an index.
template <int SEL, bool FULL>
__device__ __forceinline__ Rgb aug_chain(Rgb c, const AugColor& k) {
  if (SEL == 0) {
    c = op_hue(op_saturation(op_brightness(c, k), k), k);
    if (FULL) c = op_contrast(c, k);
  } else if (SEL == 1) {
    c = op_brightness(op_saturation(c, k), k);
    if (FULL) c = op_hue(op_contrast(c, k), k);
  } else if (SEL == 2) {
    if (FULL) c = op_saturation(op_brightness(op_hue(op_contrast(c, k), k), k), k);
  } else {
    c = op_saturation(op_hue(c, k), k);
    if (FULL) c = op_brightness(op_contrast(c, k), k);
  }
  if (FULL) { c.r = clip01(c.r); c.g = clip01(c.g); c.b = clip01(c.b); }
  return c;
}

__device__ __forceinline__ Rgb load_rgb(const unsigned char* __restrict__ img, int64_t pix) {
  Rgb c;
  c.r = (float)img[pix * 3 + 0] * (1.0f / 255.0f);
  c.g = (float)img[pix * 3 + 1] * (1.0f / 255.0f);
  c.b = (float)img[pix * 3 + 2] * (1.0f / 255.0f);
  return c;
}

// ---- the draws ---------------------------------------------------------------------------------------------------------
// draw(seed, image, k) = mix(word ^ (0x80000000 | k)), word = mix(mix(seed ^ 0x9E3779B9) + image): the per-image word of
// the shuffle keys (targets.hip) with bit 31 set, which no shuffle key (2 * element + stream) has.
struct Draws {
  unsigned word;
  int k;
  __device__ __forceinline__ unsigned next() { return tg_mix(word ^ (0x80000000u | (unsigned)k++)); }
  __device__ __forceinline__ float uf(float lo, float hi) {
    const float t = (float)(next() >> 8) * 0x1p-24f;
    return lo + t * (hi - lo);
  }
  __device__ __forceinline__ int ui(int lo, int hi) {
    const unsigned u = next();
    const int r = hi - lo;
    return r <= 0 ? lo : lo + (int)(u % (unsigned)r);
  }
};

__device__ __forceinline__ bool check_bbox(float b0, float b1, float b2, float b3) {
  const float hh = b2 - b0, ww = b3 - b1;
  const float area = ww * hh;
  return area < 0.9f && area > 0.001f && ww > 0.025f && hh > 0.025f;
}

__device__ __forceinline__ int popc64(unsigned long long v) { return __popcll(v); }

}  // namespace

// grid N, one wavefront.  Everything but the per-box values is wave-uniform: the draw counter, every loop condition
// (ballots), the roi.  Boxes live in LDS: s_a the attempt's boxes (after the optional expand) and their centres, s_r the
// attempt's result.  All loops carry the reference's bounds (3 attempts x 50 x 20 x 10 rounds).
__global__ __launch_bounds__(AUG_WAVE) void augment_geometry_kernel(
    int64_t packed_bytes, const int64_t* __restrict__ offsets, const int* __restrict__ image_shapes,
    const int* __restrict__ glabels, const float* __restrict__ gbboxes, const int* __restrict__ n_gt,
    const int* __restrict__ image_ids, int G, unsigned seed_word, AugWorkspace ws, int* __restrict__ out_glabels,
    float* __restrict__ out_gbboxes, int* __restrict__ out_n_gt) {
  __shared__ float s_a[4][AUG_MAX_GT];
  __shared__ float s_c[2][AUG_MAX_GT];
  __shared__ float s_r[4][AUG_MAX_GT];
  __shared__ int s_rl[AUG_MAX_GT];

  const int n = blockIdx.x;
  const int lane = threadIdx.x;
  const int H = image_shapes[2 * n], W = image_shapes[2 * n + 1];
  const bool valid = aug_valid(packed_bytes, offsets[n], H, W);
  const int* const gl = glabels + (size_t)n * G;
  const float* const gb = gbboxes + (size_t)n * G * 4;
  int* const ol = out_glabels + (size_t)n * G;
  float* const ob = out_gbboxes + (size_t)n * G * 4;
  if (lane < 4) ws.sums[4 * n + lane] = 0ull;

  int r_sel = 0, r_expanded = 0, r_min_iou = 0, r_tiny = 0, r_iou_mask = 0, r_exp_mask = 0, r_fallback = 0;
  float r_brightness = 0.f, r_saturation = 0.f, r_hue = 0.f, r_contrast = 0.f;
  if (!valid) {
    for (int j = lane; j < G; j += AUG_WAVE) {
      ol[j] = 0;
      ob[4 * j + 0] = 0.f; ob[4 * j + 1] = 0.f; ob[4 * j + 2] = 0.f; ob[4 * j + 3] = 0.f;
    }
    if (lane == 0) out_n_gt[n] = 0;
    if (lane < 32) reinterpret_cast<int*>(ws.rec + n)[lane] = 0;
    return;
  }
  const int n_in = min(max(n_gt[n], 0), G);
  const int n_pad = (n_in + AUG_WAVE - 1) / AUG_WAVE * AUG_WAVE;
  Draws D;
  D.word = tg_mix(seed_word + (unsigned)(image_ids ? image_ids[n] : n));
  D.k = 0;

  // colour parameters, each drawn when its op is reached
  const int sel = (int)(D.next() % 4u);
  r_sel = sel;
  {
    const float bd = (float)(32.0 / 255.0);
    // ordering sel as four 2-bit op codes (0 B, 1 S, 2 H, 3 C), first op in the low bits
    const unsigned order = sel == 0 ? 0xE4u /* B S H C */ : sel == 1 ? 0xB1u /* S B C H */ : sel == 2 ? 0x4Bu /* C H B S */
                                                                                                   : 0x36u /* H S C B */;
    for (int i = 0; i < 4; ++i) {
      const unsigned op = (order >> (2 * i)) & 3u;
      if (op == 0) r_brightness = D.uf(-bd, bd);
      else if (op == 1) r_saturation = D.uf(0.5f, 1.5f);
      else if (op == 2) r_hue = D.uf(-0.2f, 0.2f);
      else r_contrast = D.uf(0.5f, 1.5f);
    }
  }

  const float fH = (float)H, fW = (float)W;
  int index = 0, n_valid = 0, n_res = 0;
  int ch = H, cw = W, oy = 0, ox = 0;
  int crop_y = 0, crop_x = 0, crop_h = H, crop_w = W;
  while (index < 1 || (index < 3 && n_valid < 1)) {
    // ---- the attempt's image and boxes: the original, or its expand
    const bool expanded = !(D.uf(0.f, 1.f) < 0.5f);
    ch = H; cw = W; oy = 0; ox = 0;
    if (expanded) {
      const float ratio = D.uf(1.1f, 4.f);
      cw = (int)(fW * ratio);
      ch = (int)(fH * ratio);
      ox = D.ui(0, cw - W);
      oy = D.ui(0, ch - H);
      r_exp_mask |= 1 << index;
    }
    const float fch = (float)ch, fcw = (float)cw;
    __syncthreads();
    for (int j = lane; j < n_in; j += AUG_WAVE) {
      float b0 = gb[4 * j + 0], b1 = gb[4 * j + 1], b2 = gb[4 * j + 2], b3 = gb[4 * j + 3];
      if (expanded) {
        b0 = (b0 * fH + (float)oy) / fch;
        b1 = (b1 * fW + (float)ox) / fcw;
        b2 = (b2 * fH + (float)oy) / fch;
        b3 = (b3 * fW + (float)ox) / fcw;
      }
      s_a[0][j] = b0; s_a[1][j] = b1; s_a[2][j] = b2; s_a[3][j] = b3;
      s_c[0][j] = (b0 + b2) / 2.f;
      s_c[1][j] = (b1 + b3) / 2.f;
    }
    __syncthreads();
    const int m = (int)(D.next() % 7u);
    r_iou_mask |= 1 << m;
    r_expanded = expanded ? 1 : 0;
    r_min_iou = m;
    crop_y = 0; crop_x = 0; crop_h = ch; crop_w = cw;
    bool identity = true;          // the result is the attempt's boxes, all of them
    float r0 = 0.f, r1 = 0.f, r2 = 1.f, r3 = 1.f;
    int n_kept = n_in;
    if (m < 6) {
      const float min_iou = m == 0 ? -0.1f : m == 1 ? 0.1f : m == 2 ? 0.3f : m == 3 ? 0.5f : m == 4 ? 0.7f : 0.9f;
      int idx = 0;
      bool any_below = false;
      while (idx < 1 || (idx < 50 && (any_below || n_kept < 1))) {
        int jr = 0;
        n_kept = 0;
        while (jr < 1 || (jr < 20 && n_kept < 1)) {
          int t = 0;
          float sw = fcw, sh = fch;
          while (t < 1 || (t < 10 && (sw > sh * 2.f || sh > sw * 2.f))) {
            sw = D.uf(0.3f, 0.999f) * fcw;
            sh = D.uf(0.3f, 0.999f) * fch;
            ++t;
          }
          const int swi = (int)sw, shi = (int)sh;
          const int x = D.ui(0, cw - swi);
          const int y = D.ui(0, ch - shi);
          r0 = (float)y / fch;
          r1 = (float)x / fcw;
          r2 = (float)(y + shi) / fch;
          r3 = (float)(x + swi) / fcw;
          int cnt = 0;
          for (int j = lane; j < n_pad; j += AUG_WAVE) {
            bool in = false;
            if (j < n_in) {
              const float cy = s_c[0][j], cx = s_c[1][j];
              in = cy > r0 && cx > r1 && cy < r2 && cx < r3;
            }
            cnt += popc64(__ballot(in));
          }
          n_kept = cnt;
          ++jr;
        }
        ++idx;
        // jaccard of the kept boxes against the roi, for the loop condition
        const float roi_area = (r3 - r1) * (r2 - r0);
        unsigned long long below = 0ull;
        for (int j = lane; j < n_pad; j += AUG_WAVE) {
          bool lo = false;
          if (j < n_in) {
            const float cy = s_c[0][j], cx = s_c[1][j];
            if (cy > r0 && cx > r1 && cy < r2 && cx < r3) {
              const float b0 = s_a[0][j], b1 = s_a[1][j], b2 = s_a[2][j], b3 = s_a[3][j];
              const float iy0 = smax(r0, b0), ix0 = smax(r1, b1), iy1 = smin(r2, b2), ix1 = smin(r3, b3);
              const float h = smax(iy1 - iy0, 0.f), w = smax(ix1 - ix0, 0.f);
              const float inter = h * w;
              const float uni = roi_area + ((b2 - b0) * (b3 - b1) - inter);
              lo = inter / uni < min_iou;
            }
          }
          below |= __ballot(lo);
        }
        any_below = below != 0ull;
      }
      int sy = 0, sx = 0, shh = ch, sww = cw;
      const bool use_mask = n_kept > 0;
      if (use_mask) {
        sy = (int)(r0 * fch);
        sx = (int)(r1 * fcw);
        shh = (int)((r2 - r0) * fch);
        sww = (int)((r3 - r1) * fcw);
      }
      if (shh < 1 || sww < 1) {
        r_tiny = 1;
      } else {
        identity = false;
        crop_y = sy; crop_x = sx; crop_h = shh; crop_w = sww;
        const float fsy = (float)sy, fsx = (float)sx, fsh = (float)shh, fsw = (float)sww;
        int base = 0;
        for (int j = lane; j < n_pad; j += AUG_WAVE) {
          bool in = false;
          float b0 = 0.f, b1 = 0.f, b2 = 0.f, b3 = 0.f;
          int lab = 0;
          if (j < n_in) {
            const float cy = s_c[0][j], cx = s_c[1][j];
            in = !use_mask || (cy > r0 && cx > r1 && cy < r2 && cx < r3);
            b0 = smax(0.f, s_a[0][j] * fch - fsy) / fsh;
            b1 = smax(0.f, s_a[1][j] * fcw - fsx) / fsw;
            b2 = smin(fsh, s_a[2][j] * fch - fsy) / fsh;
            b3 = smin(fsw, s_a[3][j] * fcw - fsx) / fsw;
            lab = gl[j];
          }
          const unsigned long long bal = __ballot(in);
          if (in) {
            const int pos = base + popc64(bal & ((1ull << lane) - 1ull));
            s_r[0][pos] = b0; s_r[1][pos] = b1; s_r[2][pos] = b2; s_r[3][pos] = b3;
            s_rl[pos] = lab;
          }
          base += popc64(bal);
        }
        n_res = base;
      }
    }
    if (identity) {
      for (int j = lane; j < n_in; j += AUG_WAVE) {
        s_r[0][j] = s_a[0][j]; s_r[1][j] = s_a[1][j]; s_r[2][j] = s_a[2][j]; s_r[3][j] = s_a[3][j];
        s_rl[j] = gl[j];
      }
      n_res = n_in;
    }
    __syncthreads();
    ++index;
    int cnt = 0;
    const int res_pad = (n_res + AUG_WAVE - 1) / AUG_WAVE * AUG_WAVE;
    for (int j = lane; j < res_pad; j += AUG_WAVE) {
      const bool ok = j < n_res && check_bbox(s_r[0][j], s_r[1][j], s_r[2][j], s_r[3][j]);
      cnt += popc64(__ballot(ok));
    }
    n_valid = cnt;
  }
  const bool flip = D.uf(0.f, 1.f) < 0.5f;

  // ---- the final ground truth: the last attempt's boxes that pass check_bboxes, or the originals
  int n_out = 0;
  if (index < 3) {
    const int res_pad = (n_res + AUG_WAVE - 1) / AUG_WAVE * AUG_WAVE;
    int base = 0;
    for (int j = lane; j < res_pad; j += AUG_WAVE) {
      float b0 = 0.f, b1 = 0.f, b2 = 0.f, b3 = 0.f;
      int lab = 0;
      bool ok = false;
      if (j < n_res) {
        b0 = s_r[0][j]; b1 = s_r[1][j]; b2 = s_r[2][j]; b3 = s_r[3][j];
        lab = s_rl[j];
        ok = check_bbox(b0, b1, b2, b3);
      }
      const unsigned long long bal = __ballot(ok);
      if (ok) {
        const int pos = base + popc64(bal & ((1ull << lane) - 1ull));
        ol[pos] = lab;
        ob[4 * pos + 0] = b0;
        ob[4 * pos + 1] = flip ? 1.f - b3 : b1;
        ob[4 * pos + 2] = b2;
        ob[4 * pos + 3] = flip ? 1.f - b1 : b3;
      }
      base += popc64(bal);
    }
    n_out = base;
  } else {
    r_fallback = 1;
    ch = H; cw = W; oy = 0; ox = 0;
    crop_y = 0; crop_x = 0; crop_h = H; crop_w = W;
    for (int j = lane; j < n_in; j += AUG_WAVE) {
      const float b0 = gb[4 * j + 0], b1 = gb[4 * j + 1], b2 = gb[4 * j + 2], b3 = gb[4 * j + 3];
      ol[j] = gl[j];
      ob[4 * j + 0] = b0;
      ob[4 * j + 1] = flip ? 1.f - b3 : b1;
      ob[4 * j + 2] = b2;
      ob[4 * j + 3] = flip ? 1.f - b1 : b3;
    }
    n_out = n_in;
  }
  for (int j = n_out + lane; j < G; j += AUG_WAVE) {
    ol[j] = 0;
    ob[4 * j + 0] = 0.f; ob[4 * j + 1] = 0.f; ob[4 * j + 2] = 0.f; ob[4 * j + 3] = 0.f;
  }
  if (lane == 0) {
    out_n_gt[n] = n_out;
    AugRecord* r = ws.rec + n;
    r->valid = 1;
    r->canvas_h = ch; r->canvas_w = cw; r->off_y = oy; r->off_x = ox;
    r->crop_y = crop_y; r->crop_x = crop_x; r->crop_h = crop_h; r->crop_w = crop_w;
    r->flip = flip ? 1 : 0; r->sel = r_sel;
    r->brightness = r_brightness; r->saturation = r_saturation; r->hue = r_hue; r->contrast = r_contrast;
    r->mean[0] = 0.f; r->mean[1] = 0.f; r->mean[2] = 0.f;
    r->attempts = index; r->fallback = r_fallback; r->n_draws = D.k; r->expanded = r_expanded; r->min_iou = r_min_iou;
    r->tiny_patch = r_tiny; r->min_iou_mask = r_iou_mask; r->expand_mask = r_exp_mask; r->n_in = n_in; r->n_out = n_out;
    r->reserved[0] = 0; r->reserved[1] = 0; r->reserved[2] = 0; r->reserved[3] = 0;
  }
}

// grid (AUG_MEAN_BLOCKS, N), AUG_T threads: sum over the source image of rint(v * 65536) as int64, v = the value in front
// of the contrast op of the image's ordering.  Integer sums: any order, any grid gives the same three numbers.  Each
// source byte is read once.
namespace {
template <int SEL>
__device__ __forceinline__ void mean_partial(const unsigned char* __restrict__ img, int64_t n_pix, const AugColor& k,
                                             long long* s) {
  for (int64_t p = (int64_t)blockIdx.x * AUG_T + threadIdx.x; p < n_pix; p += (int64_t)AUG_MEAN_BLOCKS * AUG_T) {
    const Rgb c = aug_chain<SEL, false>(load_rgb(img, p), k);
    s[0] += (long long)rintf(c.r * 65536.f);
    s[1] += (long long)rintf(c.g * 65536.f);
    s[2] += (long long)rintf(c.b * 65536.f);
  }
}
}  // namespace

__global__ __launch_bounds__(AUG_T) void augment_mean_kernel(const unsigned char* __restrict__ packed,
                                                             const int64_t* __restrict__ offsets,
                                                             const int* __restrict__ image_shapes, AugWorkspace ws) {
  const int n = blockIdx.y;
  const AugRecord* rec = ws.rec + n;
  if (!rec->valid) return;
  const int H = image_shapes[2 * n], W = image_shapes[2 * n + 1];
  const unsigned char* img = packed + offsets[n];
  const int64_t n_pix = (int64_t)H * W;
  AugColor k;
  k.brightness = rec->brightness; k.saturation = rec->saturation; k.hue = rec->hue; k.contrast = rec->contrast;
  k.m0 = k.m1 = k.m2 = 0.f;
  long long s[3] = {0, 0, 0};
  switch (rec->sel) {
    case 0: mean_partial<0>(img, n_pix, k, s); break;
    case 1: mean_partial<1>(img, n_pix, k, s); break;
    case 2: mean_partial<2>(img, n_pix, k, s); break;
    default: mean_partial<3>(img, n_pix, k, s); break;
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    long long v = s[c];
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, AUG_WAVE);
    if ((threadIdx.x & (AUG_WAVE - 1)) == 0) atomicAdd(ws.sums + 4 * n + c, (unsigned long long)v);
  }
}

// one thread per image: mean_c = f32(sum_c / (H * W * 65536)) with the division in f64; the record goes to the caller
__global__ void augment_finish_kernel(const int* __restrict__ image_shapes, int N, AugWorkspace ws,
                                      AugRecord* __restrict__ records) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= N) return;
  AugRecord* rec = ws.rec + n;
  if (rec->valid) {
    const double den = (double)image_shapes[2 * n] * (double)image_shapes[2 * n + 1] * 65536.0;
#pragma unroll
    for (int c = 0; c < 3; ++c) rec->mean[c] = (float)((double)(long long)ws.sums[4 * n + c] / den);
  }
  if (records) records[n] = *rec;
}

// grid (bands of rows, N), AUG_T threads.  One item = one output row's 4 consecutive columns in all three planes.
namespace {
struct AugGeom {
  int H, W;
  int dy, dx;        // crop coordinate + (dy, dx) = source coordinate
  int crop_h, crop_w;
  bool flip;
};

template <int SEL>
__device__ __forceinline__ Rgb aug_tap(const unsigned char* __restrict__ img, const AugGeom& g, const AugColor& k, int y,
                                       int x) {
  const int sy = y + g.dy, sx = x + g.dx;
  if (sy >= 0 && sy < g.H && sx >= 0 && sx < g.W)
    return aug_chain<SEL, true>(load_rgb(img, (int64_t)sy * g.W + sx), k);
  Rgb c;                       // the canvas of ssd_random_expand: [R,G,B mean]/255, not distorted
  c.r = (float)(123.68 / 255.0); c.g = (float)(116.78 / 255.0); c.b = (float)(103.94 / 255.0);
  return c;
}

__device__ __forceinline__ float blend(float tl, float tr, float bl, float br, float lx, float ly, float mean) {
  const float top = tl + (tr - tl) * lx;
  const float bot = bl + (br - bl) * lx;
  return (top + (bot - top) * ly) * 2.f - mean;
}

template <int SEL, bool VEC>
__device__ __forceinline__ void pixels_band(const unsigned char* __restrict__ img, const AugGeom& g, const AugColor& k,
                                            int S, int rows_per_band, float* __restrict__ o) {
  const float hs = (float)g.crop_h / (float)S, wsc = (float)g.crop_w / (float)S;
  const int Q = (S + 3) / 4;
  const int y_begin = blockIdx.x * rows_per_band;
  const int items = min(rows_per_band, S - y_begin) * Q;
  const size_t plane = (size_t)S * S;
  for (int it = threadIdx.x; it < items; it += AUG_T) {
    const int oy = y_begin + it / Q;
    const int ox0 = (it % Q) * 4;
    const float fy = (float)oy * hs;
    const int y0 = min((int)fy, g.crop_h - 1);
    const int y1 = min(y0 + 1, g.crop_h - 1);
    const float ly = fy - (float)y0;
    float v[3][4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float fx = (float)(ox0 + j) * wsc;
      int x0 = min((int)fx, g.crop_w - 1);
      int x1 = min(x0 + 1, g.crop_w - 1);
      const float lx = fx - (float)x0;
      if (g.flip) { x0 = g.crop_w - 1 - x0; x1 = g.crop_w - 1 - x1; }
      const Rgb tl = aug_tap<SEL>(img, g, k, y0, x0), tr = aug_tap<SEL>(img, g, k, y0, x1);
      const Rgb bl = aug_tap<SEL>(img, g, k, y1, x0), br = aug_tap<SEL>(img, g, k, y1, x1);
      v[0][j] = blend(tl.r, tr.r, bl.r, br.r, lx, ly, 123.68f / 127.5f);
      v[1][j] = blend(tl.g, tr.g, bl.g, br.g, lx, ly, 116.78f / 127.5f);
      v[2][j] = blend(tl.b, tr.b, bl.b, br.b, lx, ly, 103.94f / 127.5f);
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
}  // namespace

template <bool VEC>
__global__ __launch_bounds__(AUG_T) void augment_pixels_kernel(const unsigned char* __restrict__ packed,
                                                               const int64_t* __restrict__ offsets,
                                                               const int* __restrict__ image_shapes, AugWorkspace ws, int S,
                                                               int rows_per_band, float* __restrict__ out) {
  const int n = blockIdx.y;
  const AugRecord* rec = ws.rec + n;
  const size_t plane = (size_t)S * S;
  float* const o = out + (size_t)n * 3 * plane;
  if (!rec->valid) {           // an invalid descriptor: NaN planes, nothing read
    const int y_begin = blockIdx.x * rows_per_band;
    const int cnt = min(rows_per_band, S - y_begin) * S;
    for (int i = threadIdx.x; i < cnt; i += AUG_T) {
#pragma unroll
      for (int c = 0; c < 3; ++c) o[c * plane + (size_t)y_begin * S + i] = NAN;
    }
    return;
  }
  AugGeom g;
  g.H = image_shapes[2 * n]; g.W = image_shapes[2 * n + 1];
  g.dy = rec->crop_y - rec->off_y; g.dx = rec->crop_x - rec->off_x;
  g.crop_h = rec->crop_h; g.crop_w = rec->crop_w;
  g.flip = rec->flip != 0;
  AugColor k;
  k.brightness = rec->brightness; k.saturation = rec->saturation; k.hue = rec->hue; k.contrast = rec->contrast;
  k.m0 = rec->mean[0]; k.m1 = rec->mean[1]; k.m2 = rec->mean[2];
  const unsigned char* img = packed + offsets[n];
  switch (rec->sel) {          // wave-uniform: one ordering per image
    case 0: pixels_band<0, VEC>(img, g, k, S, rows_per_band, o); break;
    case 1: pixels_band<1, VEC>(img, g, k, S, rows_per_band, o); break;
    case 2: pixels_band<2, VEC>(img, g, k, S, rows_per_band, o); break;
    default: pixels_band<3, VEC>(img, g, k, S, rows_per_band, o); break;
  }
}

// the one description of the workspace: rec[N], sums[N][4], packed (walk it with an alignment of 8 bytes)
static AugWorkspace aug_layout(WsWalk& w, int N) { return {w.take<AugRecord>(N), w.take<unsigned long long>((size_t)N * 4)}; }

size_t preprocess_train_workspace_bytes(int N, int G) {
  (void)G;                     // the boxes of one image live in LDS
  return ws_measure(8, aug_layout, N);
}

int launch_preprocess_train(const unsigned char* packed, int64_t packed_bytes, const int64_t* offsets,
                            const int* image_shapes, const int* glabels, const float* gbboxes, const int* n_gt,
                            const int* image_ids, int N, int G, int S, unsigned seed, float* out_nchw, int* out_glabels,
                            float* out_gbboxes, int* out_n_gt, void* records, void* workspace, hipStream_t s) {
  XDET_REQUIRE(packed && offsets && image_shapes && glabels && gbboxes && n_gt, "preprocess_train: NULL input");
  XDET_REQUIRE(out_nchw && out_glabels && out_gbboxes && out_n_gt && workspace, "preprocess_train: NULL output or workspace");
  XDET_REQUIRE(N > 0 && N <= 65535 && S > 0 && packed_bytes >= 0, "preprocess_train: bad sizes");
  XDET_REQUIRE(G > 0 && G <= AUG_MAX_GT, "preprocess_train: G must be in 1 .. 512");
  XDET_REQUIRE(((uintptr_t)workspace & 15) == 0 && ((uintptr_t)records & 3) == 0, "preprocess_train: unaligned workspace or records");
  const AugWorkspace ws = ws_carve(workspace, 8, aug_layout, N);
  hipLaunchKernelGGL(augment_geometry_kernel, dim3((unsigned)N), dim3(AUG_WAVE), 0, s, packed_bytes, offsets, image_shapes,
                     glabels, gbboxes, n_gt, image_ids, G, tg_mix(seed ^ 0x9E3779B9u), ws, out_glabels, out_gbboxes, out_n_gt);
  XDET_LAUNCH_CHECK();
  hipLaunchKernelGGL(augment_mean_kernel, dim3(AUG_MEAN_BLOCKS, (unsigned)N), dim3(AUG_T), 0, s, packed, offsets, image_shapes,
                     ws);
  XDET_LAUNCH_CHECK();
  hipLaunchKernelGGL(augment_finish_kernel, dim3((unsigned)cdiv(N, 64)), dim3(64), 0, s, image_shapes, N, ws,
                     static_cast<AugRecord*>(records));
  XDET_LAUNCH_CHECK();
  const int Q = (S + 3) / 4;
  const int rows = std::max(1, AUG_ITEMS / Q);
  const dim3 grid((unsigned)cdiv(S, rows), (unsigned)N);
  if (S % 4 == 0 && ((uintptr_t)out_nchw & 15) == 0)
    hipLaunchKernelGGL(augment_pixels_kernel<true>, grid, dim3(AUG_T), 0, s, packed, offsets, image_shapes, ws, S, rows,
                       out_nchw);
  else
    hipLaunchKernelGGL(augment_pixels_kernel<false>, grid, dim3(AUG_T), 0, s, packed, offsets, image_shapes, ws, S, rows,
                       out_nchw);
  XDET_LAUNCH_CHECK();
  return XDET_OK;
}

}  // namespace xdet
