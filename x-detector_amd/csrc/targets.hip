// Training targets on the GPU: what the reference's training script does with the ground truth before any loss.
//   AnchorEncoder.encode_all_anchors (preprocessing/anchor_manipulator.py:118-171, 319-335)  -> xdet_encode_anchors
//   AnchorEncoder.ext_encode_rois    (preprocessing/anchor_manipulator.py:337-445)           -> xdet_encode_rois
// through iou_matrix (:22-46) and do_dual_max_match (:48-94, ignore_between and gt_max_first both true).  The contract is
// written out in include/xdet.h and DESIGN.md 4.28; xdet/targets.py holds the same statement in NumPy.
// Compiled with -ffp-contract=off: every f32 operation rounds on its own, in the reference's order.
//
// Four kernels, no synchronisation inside any of them (a dependency between workgroups is a kernel boundary):
//   tg_prepare_kernel   per image: the ground truth that takes part (all of the first n_gt boxes, or those with label > 0),
//                       compacted in order; clears the row maxima -- the call's only control words
//   tg_colmax_kernel    a lane owns a candidate and walks the boxes: column maximum (first maximum: ascending g, strict >),
//                       and per box the row maximum as a packed 64-bit (IoU bits, ~candidate) atomicMax
//   tg_assign_kernel    resolves the candidates a box points at ("forced"), writes label, target and score
//   tg_sample_kernel    ROIs only, one workgroup per image: foreground / background lists, the shuffle as a sort by
//                       (hash key, element), the up-sampling tail, the gather
#include "common.h"
#include "shuffle.h"

#include <algorithm>
#include <climits>
#include <cmath>

namespace xdet {

constexpr int TG_MAXG = 512;      // ground-truth boxes per image, as in evalmatch.hip
constexpr int TG_T = 256;         // threads of the match kernels: one candidate per lane
constexpr int TG_MAXM = 8192;     // candidates (R + G) and rois_per_image of the ROI form
constexpr int TG_ST = 1024;       // threads of the sample kernel
constexpr unsigned long long TG_ROW_INIT = 0xFFFFFFFFull;     // (IoU 0, candidate 0): where an all-zero row points

struct TgWorkspace {
  int* cn;                      // [N] boxes that take part
  int* clab;                    // [N][G] their labels
  float4* cbox;                 // [N][G] their corners
  unsigned long long* rowmax;   // [N][G] (IoU bits << 32) | ~candidate of the row's first maximum
  int* lab;                     // [N][n_candidates]     per-candidate results of the ROI form (when the caller gives no
  float* sc;                    // [N][n_candidates]     all_* arrays)
  float* tg;                    // [N][n_candidates][4]
};

// the one description of the workspace (n_cand = 0: the anchor form, whose per-candidate results go to the caller's arrays)
static TgWorkspace tg_layout(WsWalk& w, int N, int n_cand, int G) {
  const size_t n = (size_t)N, g = (size_t)G, m = (size_t)n_cand;
  TgWorkspace ws;
  ws.cn = w.take<int>(n);
  ws.clab = w.take<int>(n * g);
  ws.cbox = w.take<float4>(n * g);
  ws.rowmax = w.take<unsigned long long>(n * g);
  ws.lab = w.take<int>(n * m);
  ws.sc = w.take<float>(n * m);
  ws.tg = w.take<float>(n * m * 4);
  return ws;
}

// where the candidates come from: anchors (rois == NULL; index (y * W + x) * A + k as in rpn_decode_kernel) or the image's
// R ROIs followed by its participating ground-truth boxes
struct TgCand {
  const float* anchors_yx;   // [Hh * Ww][2]
  const float* anchors_hw;   // [A][2]
  int A;
  const float* rois;         // [N][R][4]
  int R;
  int M;                     // candidates per image the outputs are laid out for (Hh * Ww * A, or R + G)
  float lo, hi;              // inside mask: min >= lo, max < hi
};

// candidate a of image n -> corners; ref = (yref, xref, href, wref) the targets are encoded against
__device__ __forceinline__ float4 tg_candidate(const TgCand& c, const float4* __restrict__ cbox, int n, int G, int a, float4* ref) {
  if (c.rois == nullptr) {
    const int cell = a / c.A, k = a - cell * c.A;
    const float yr = c.anchors_yx[cell * 2], xr = c.anchors_yx[cell * 2 + 1];
    const float hr = c.anchors_hw[k * 2], wr = c.anchors_hw[k * 2 + 1];
    *ref = make_float4(yr, xr, hr, wr);
    return make_float4(yr - hr / 2.f, xr - wr / 2.f, yr + hr / 2.f, xr + wr / 2.f);       // center2point
  }
  const float4 b = a < c.R ? *reinterpret_cast<const float4*>(c.rois + ((int64_t)n * c.R + a) * 4) : cbox[(int64_t)n * G + (a - c.R)];
  const float h = b.z - b.x, w = b.w - b.y;
  *ref = make_float4(b.x + h / 2.f, b.y + w / 2.f, h, w);                                  // point2center
  return b;
}

__device__ __forceinline__ float tg_inside(const TgCand& c, float4 b) {
  return (b.x >= c.lo && b.y >= c.lo && b.z < c.hi && b.w < c.hi) ? 1.f : 0.f;
}

__device__ __forceinline__ float tg_area(float4 b) { return (b.w - b.y) * (b.z - b.x); }

// iou_matrix times the inside mask: one entry
__device__ __forceinline__ float tg_overlap(float4 g, float ga, float4 b, float ba, float fm) {
  const float h = fmaxf(fminf(g.z, b.z) - fmaxf(g.x, b.x), 0.f);
  const float w = fmaxf(fminf(g.w, b.w) - fmaxf(g.y, b.y), 0.f);
  const float inter = h * w;
  const float uni = (ga + ba) - inter;
  const float v = uni == 0.f ? 0.f : inter / uni;
  return v * fm;
}

// grid N, TG_MAXG threads
__global__ __launch_bounds__(TG_MAXG) void tg_prepare_kernel(const int* __restrict__ glabels, const float* __restrict__ gbboxes,
                                                             const int* __restrict__ n_gt, int G, int positive_only, TgWorkspace ws) {
  __shared__ int s_wave[TG_MAXG / 64];
  const int n = blockIdx.x, g = threadIdx.x, wv = g >> 6, ln = g & 63;
  const int ng = min(max(n_gt[n], 0), G);
  int lab = 0;
  float4 box = make_float4(0.f, 0.f, 0.f, 0.f);
  bool keep = false;
  if (g < ng) {                                    // nothing behind n_gt is read
    lab = glabels[(int64_t)n * G + g];
    box = *reinterpret_cast<const float4*>(gbboxes + ((int64_t)n * G + g) * 4);
    keep = !positive_only || lab > 0;
  }
  const unsigned long long m = __ballot(keep);
  if (ln == 0) s_wave[wv] = __popcll(m);
  __syncthreads();
  int off = 0, total = 0;
  for (int w = 0; w < TG_MAXG / 64; ++w) {
    if (w < wv) off += s_wave[w];
    total += s_wave[w];
  }
  if (keep) {
    const int p = off + __popcll(m & ((1ull << ln) - 1ull));
    ws.clab[(int64_t)n * G + p] = lab;
    ws.cbox[(int64_t)n * G + p] = box;
  }
  if (g < G) ws.rowmax[(int64_t)n * G + g] = TG_ROW_INIT;
  if (g == 0) ws.cn[n] = total;
}

// grid (ceil(M / TG_T), N).  lab / sc receive the column's first maximum (box, value) for tg_assign_kernel.
__global__ __launch_bounds__(TG_T) void tg_colmax_kernel(TgCand c, int G, TgWorkspace ws, int* __restrict__ lab, float* __restrict__ sc) {
  __shared__ float4 s_box[TG_MAXG];
  __shared__ float s_area[TG_MAXG];
  __shared__ unsigned long long s_row[TG_MAXG];
  const int n = blockIdx.y, tid = threadIdx.x, ln = tid & 63;
  const int cn = ws.cn[n];
  const int Mn = c.rois ? c.R + cn : c.M;
  if (blockIdx.x * TG_T >= Mn || cn == 0) return;          // (block-uniform)
  for (int g = tid; g < cn; g += TG_T) {
    const float4 b = ws.cbox[(int64_t)n * G + g];
    s_box[g] = b;
    s_area[g] = tg_area(b);
    s_row[g] = TG_ROW_INIT;
  }
  __syncthreads();
  const int a = blockIdx.x * TG_T + tid;
  const bool have = a < Mn;
  float4 ref, b = make_float4(0.f, 0.f, 0.f, 0.f);
  float fm = 0.f, ba = 0.f;
  if (have) {
    b = tg_candidate(c, ws.cbox, n, G, a, &ref);
    fm = tg_inside(c, b);
    ba = tg_area(b);
  }
  float best = -1.f;           // every entry is >= 0: box 0 always takes over
  int bg = 0;
  for (int g = 0; g < cn; ++g) {
    const float v = have ? tg_overlap(s_box[g], s_area[g], b, ba, fm) : 0.f;
    if (v > best) { best = v; bg = g; }
    // the row's first maximum: only a positive IoU can beat (0, candidate 0); within a wave the lowest lane is the lowest candidate
    const unsigned vb = __float_as_uint(v) & 0x7FFFFFFFu;
    if (__ballot(vb != 0u) == 0ull) continue;
    unsigned mx = vb;
    for (int o = 32; o > 0; o >>= 1) mx = max(mx, (unsigned)__shfl_xor((int)mx, o));
    const unsigned long long same = __ballot(vb == mx);
    if (ln == __ffsll((long long)same) - 1)
      atomicMax(&s_row[g], ((unsigned long long)mx << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)a));
  }
  if (have) {
    lab[(int64_t)n * c.M + a] = bg;
    sc[(int64_t)n * c.M + a] = best;
  }
  __syncthreads();
  for (int g = tid; g < cn; g += TG_T)
    if ((s_row[g] >> 32) != 0ull) atomicMax(&ws.rowmax[(int64_t)n * G + g], s_row[g]);
}

// grid (ceil(M / TG_T), N)
__global__ __launch_bounds__(TG_T) void tg_assign_kernel(TgCand c, int G, TgWorkspace ws, float high, float low, float4 scaling,
                                                         int* __restrict__ lab, float* __restrict__ tg, float* __restrict__ sc) {
  __shared__ float4 s_box[TG_MAXG];
  __shared__ float s_area[TG_MAXG];
  __shared__ int s_lab[TG_MAXG];
  __shared__ unsigned s_besta[TG_MAXG];
  const int n = blockIdx.y, tid = threadIdx.x;
  const int cn = ws.cn[n];
  const int Mn = c.rois ? c.R + cn : c.M;
  const int a = blockIdx.x * TG_T + tid;
  if (a >= Mn || cn == 0) {
    // behind the image's candidates: ignored, zero.  No ground truth: background, zero (the reference would fail here)
    if (a < c.M) {
      const int64_t o = (int64_t)n * c.M + a;
      lab[o] = a >= Mn ? -1 : 0;
      sc[o] = 0.f;
      *reinterpret_cast<float4*>(tg + o * 4) = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    if (cn == 0 || blockIdx.x * TG_T >= Mn) return;        // (block-uniform)
  }
  for (int g = tid; g < cn; g += TG_T) {
    const float4 b = ws.cbox[(int64_t)n * G + g];
    s_box[g] = b;
    s_area[g] = tg_area(b);
    s_lab[g] = ws.clab[(int64_t)n * G + g];
    s_besta[g] = 0xFFFFFFFFu - (unsigned)(ws.rowmax[(int64_t)n * G + g] & 0xFFFFFFFFull);
  }
  __syncthreads();
  if (a >= Mn) return;
  float4 ref;
  const float4 b = tg_candidate(c, ws.cbox, n, G, a, &ref);
  const float fm = tg_inside(c, b), ba = tg_area(b);
  const int64_t o = (int64_t)n * c.M + a;
  const int bg = lab[o];
  const float mv = sc[o];
  int m = mv < low ? -1 : (mv < high ? -2 : bg);
  float score = mv;
  // a candidate that a box points at takes the FIRST maximum over g of O[g, a] * [best_a[g] == a]: box 0 when all are zero
  bool forced = false;
  float fbest = 0.f;
  int fg = 0;
  for (int g = 0; g < cn; ++g) {
    if (s_besta[g] != (unsigned)a) continue;
    forced = true;
    const float v = tg_overlap(s_box[g], s_area[g], b, ba, fm);
    if (v > fbest) { fbest = v; fg = g; }
  }
  if (forced) {
    m = fg;
    score = fbest > 0.f ? fbest : tg_overlap(s_box[0], s_area[0], b, ba, fm);
  }
  const int k = max(m, 0);
  const float4 gb = s_box[k];
  const float mask = m > -1 ? 1.f : 0.f;
  const float gcy = (gb.z + gb.x) / 2.f, gcx = (gb.w + gb.y) / 2.f, gh = gb.z - gb.x, gw = gb.w - gb.y;
  float4 t;
  t.x = mask * (((gcy - ref.x) / ref.z) / scaling.x);
  t.y = mask * (((gcx - ref.y) / ref.w) / scaling.y);
  t.z = mask * (logf(gh / ref.z) / scaling.z);
  t.w = mask * (logf(gw / ref.w) / scaling.w);
  lab[o] = s_lab[k] * (m > -1 ? 1 : 0) - (m < -1 ? 1 : 0);
  sc[o] = score;
  *reinterpret_cast<float4*>(tg + o * 4) = t;
}

// ---- the sampler -------------------------------------------------------------------------------------------------

// shuffle(S) = S ordered by (key, element): key = mix(mix(mix(seed ^ 0x9E3779B9) + image) ^ (2 * element + stream)), mix the
// 32-bit finaliser of shuffle.h -- integers only, the same on the host (xdet/targets.py shuffle_keys)
__device__ __forceinline__ unsigned long long tg_key(unsigned image_word, unsigned element, unsigned stream) {
  return ((unsigned long long)tg_mix(image_word ^ (2u * element + stream)) << 32) | element;
}

// the members of class `cls` among seq[0 .. len) in sequence order, the first `take` of them, to keep[base ...]
// (seq == NULL: the identity sequence).  All TG_ST threads; s_wave: TG_ST / 64 + 1 ints.
__device__ void tg_take(const unsigned long long* seq, int len, const unsigned char* s_cls, int cls, int take, int* keep, int base,
                        int* s_wave) {
  const int tid = threadIdx.x, wv = tid >> 6, ln = tid & 63;
  int carry = 0;
  for (int i0 = 0; i0 < len && carry < take; i0 += TG_ST) {            // (carry is block-uniform)
    const int i = i0 + tid;
    const int e = i < len ? (seq ? (int)(seq[i] & 0xFFFFFFFFull) : i) : 0;
    const bool f = i < len && s_cls[e] == cls;
    const unsigned long long m = __ballot(f);
    if (ln == 0) s_wave[wv] = __popcll(m);
    __syncthreads();
    int off = carry, total = 0;
    for (int w = 0; w < TG_ST / 64; ++w) {
      if (w < wv) off += s_wave[w];
      total += s_wave[w];
    }
    if (f) {
      const int r = off + __popcll(m & ((1ull << ln) - 1ull));
      if (r < take) keep[base + r] = e;
    }
    carry += total;
    __syncthreads();
  }
}

struct TgSample {
  const float* rois;       // [N][R][4]
  int R, G, M;             // M = R + G: the layout of lab / sc / tg
  int rpi, exp_fg;         // rois_per_image, round_half_even(f32(rois_per_image) * fg_fraction)
  float bg_low;
  unsigned seed_word;      // mix(seed ^ 0x9E3779B9)
  const int* image_ids;    // NULL: 0 .. N-1
  int P;                   // sort length: the power of two >= max(M, rois_per_image)
  float* out_rois;
  float* out_targets;
  int* out_labels;
  float* out_scores;
  int* out_index;          // may be NULL
  int* counts;             // may be NULL
};

// grid N, TG_ST threads, dynamic LDS: P sort words, then rois_per_image ints
__global__ __launch_bounds__(TG_ST) void tg_sample_kernel(TgSample p, TgWorkspace ws, const int* __restrict__ lab,
                                                          const float* __restrict__ tg, const float* __restrict__ sc) {
  extern __shared__ unsigned long long s_dyn[];
  __shared__ unsigned char s_cls[TG_MAXM];
  __shared__ int s_wave[TG_ST / 64 + 1];
  __shared__ int s_cnt[2];
  unsigned long long* s_sort = s_dyn;
  int* s_keep = reinterpret_cast<int*>(s_dyn + p.P);
  const int n = blockIdx.x, tid = threadIdx.x;
  const int Mn = p.R + ws.cn[n];
  const unsigned image = p.image_ids ? (unsigned)p.image_ids[n] : (unsigned)n;
  const unsigned word = tg_mix(p.seed_word + image);
  const int64_t row = (int64_t)n * p.M;

  if (tid < 2) s_cnt[tid] = 0;
  __syncthreads();
  int np_ = 0, nn_ = 0;
  for (int i = tid; i < p.P; i += TG_ST) {
    int cls = 0;
    if (i < Mn) {
      const int l = lab[row + i];
      cls = l > 0 ? 1 : ((l == 0 && sc[row + i] > p.bg_low) ? 2 : 0);
    }
    if (i < TG_MAXM) s_cls[i] = (unsigned char)cls;
    np_ += cls == 1;
    nn_ += cls == 2;
    s_sort[i] = i < Mn ? tg_key(word, (unsigned)i, 0u) : ~0ull;
  }
  if (np_) atomicAdd(&s_cnt[0], np_);
  if (nn_) atomicAdd(&s_cnt[1], nn_);
  __syncthreads();
  const int n_pos = s_cnt[0], n_neg = s_cnt[1];
  const bool fg_all = n_pos < p.exp_fg;
  const int n_fg = fg_all ? n_pos : p.exp_fg;
  const int exp_bg = p.rpi - n_fg;
  const bool bg_all = n_neg < exp_bg;
  const int n_bg = bg_all ? n_neg : exp_bg;
  const int n_keep = n_fg + n_bg;
  if (!fg_all || !bg_all) lds_bitonic_sort_u64<TG_ST>(s_sort, p.P);            // (block-uniform; the padding words sort behind the Mn real ones)
  tg_take(fg_all ? nullptr : s_sort, Mn, s_cls, 1, n_fg, s_keep, 0, s_wave);
  tg_take(bg_all ? nullptr : s_sort, Mn, s_cls, 2, n_bg, s_keep, n_fg, s_wave);
  __syncthreads();
  if (tid == 0 && p.counts) {
    int* c = p.counts + (int64_t)n * 4;
    c[0] = Mn; c[1] = n_pos; c[2] = n_neg; c[3] = n_keep;
  }
  // fewer than rois_per_image: every kept one (left div n_keep) + 1 times in order, then the first (left mod n_keep)
  // positions of shuffle(range(n_keep)), stream 1
  int full = p.rpi;
  if (n_keep > 0 && n_keep < p.rpi) {
    const int left = p.rpi - n_keep;
    full = n_keep * (left / n_keep + 1);
    if (left % n_keep) {
      int P2 = 1;
      while (P2 < n_keep) P2 <<= 1;
      for (int i = tid; i < P2; i += TG_ST) s_sort[i] = i < n_keep ? tg_key(word, (unsigned)i, 1u) : ~0ull;
      __syncthreads();
      lds_bitonic_sort_u64<TG_ST>(s_sort, P2);
    }
  }
  for (int j = tid; j < p.rpi; j += TG_ST) {
    const int64_t o = (int64_t)n * p.rpi + j;
    float4 box = make_float4(0.f, 0.f, 0.f, 0.f), t = box;
    int l = -1, e = -1;
    float s = 0.f;
    if (n_keep > 0) {
      const int pos = j < full ? j % n_keep : (int)(s_sort[j - full] & 0xFFFFFFFFull);
      e = s_keep[pos];
      box = e < p.R ? *reinterpret_cast<const float4*>(p.rois + ((int64_t)n * p.R + e) * 4) : ws.cbox[(int64_t)n * p.G + (e - p.R)];
      t = *reinterpret_cast<const float4*>(tg + (row + e) * 4);
      l = lab[row + e];
      s = sc[row + e];
    }
    *reinterpret_cast<float4*>(p.out_rois + o * 4) = box;
    *reinterpret_cast<float4*>(p.out_targets + o * 4) = t;
    p.out_labels[o] = l;
    p.out_scores[o] = s;
    if (p.out_index) p.out_index[o] = e;
  }
}

static DeviceOnce g_sample_once;

static bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// sizes, limits and values first, pointers last: a caller that probes with NULL pointers is told what is wrong with its numbers
static int check_sizes(const char* what, int N, int G, const float* scaling) {
  XDET_REQUIRE(N > 0 && G > 0, std::string(what) + ": N and G must be positive");
  XDET_REQUIRE(G <= TG_MAXG, std::string(what) + ": at most 512 ground-truth boxes per image");
  XDET_REQUIRE(scaling, std::string(what) + ": prior_scaling is NULL");
  for (int i = 0; i < 4; ++i)
    XDET_REQUIRE(std::isfinite(scaling[i]) && scaling[i] != 0.f, std::string(what) + ": prior_scaling must be finite and not zero");
  return XDET_OK;
}

static int check_ground_truth(const char* what, const void* glabels, const void* gbboxes, const void* n_gt, const void* workspace) {
  XDET_REQUIRE(glabels && gbboxes && n_gt && workspace, std::string(what) + ": NULL argument");
  XDET_REQUIRE(aligned16(gbboxes) && aligned16(workspace), std::string(what) + ": gbboxes and the workspace must be 16-byte aligned");
  return XDET_OK;
}

// ymin >= -b, ymax < f32(1 + b) with 1 + b formed in double and rounded once
static void tg_border(float b, float* lo, float* hi) {
  *lo = -b;
  *hi = (float)(1.0 + (double)b);
}

static int launch_match(const TgCand& c, int N, int G, const TgWorkspace& ws, float high, float low, const float* scaling, int* lab,
                        float* tg, float* sc, hipStream_t s) {
  const dim3 grid((c.M + TG_T - 1) / TG_T, N);
  hipLaunchKernelGGL(tg_colmax_kernel, grid, dim3(TG_T), 0, s, c, G, ws, lab, sc);
  XDET_LAUNCH_CHECK();
  hipLaunchKernelGGL(tg_assign_kernel, grid, dim3(TG_T), 0, s, c, G, ws, high, low,
                     make_float4(scaling[0], scaling[1], scaling[2], scaling[3]), lab, tg, sc);
  XDET_LAUNCH_CHECK();
  return XDET_OK;
}

}  // namespace xdet

using namespace xdet;

static inline hipStream_t S(void* s) { return reinterpret_cast<hipStream_t>(s); }

extern "C" {

size_t xdet_targets_workspace_bytes(int N, int n_candidates, int G) {
  if (N <= 0 || G <= 0 || n_candidates < 0) return 0;
  return ws_measure(256, tg_layout, N, n_candidates, G);
}

int xdet_encode_anchors(const float* anchors_yx, const float* anchors_hw, int Hh, int Ww, int A, float allowed_border,
                        const int32_t* glabels, const float* gbboxes, const int32_t* n_gt, int N, int G, float high_thr,
                        float low_thr, const float* prior_scaling4, void* workspace, int32_t* labels, float* targets,
                        float* scores, void* stream) {
  XDET_REQUIRE(Hh > 0 && Ww > 0 && A > 0, "encode_anchors: Hh, Ww and A must be positive");
  XDET_REQUIRE((int64_t)Hh * Ww * A <= INT_MAX / 8, "encode_anchors: too many anchors");
  XDET_TRY(check_sizes("encode_anchors", N, G, prior_scaling4));
  XDET_REQUIRE(std::isfinite(allowed_border) && std::isfinite(high_thr) && std::isfinite(low_thr),
               "encode_anchors: the border and the thresholds must be finite");
  XDET_TRY(check_ground_truth("encode_anchors", glabels, gbboxes, n_gt, workspace));
  XDET_REQUIRE(anchors_yx && anchors_hw && labels && targets && scores, "encode_anchors: NULL argument");
  XDET_REQUIRE(aligned16(targets), "encode_anchors: targets must be 16-byte aligned");
  const TgWorkspace ws = ws_carve(workspace, 256, tg_layout, N, 0, G);
  TgCand c{};
  c.anchors_yx = anchors_yx;
  c.anchors_hw = anchors_hw;
  c.A = A;
  c.M = Hh * Ww * A;
  tg_border(allowed_border, &c.lo, &c.hi);
  hipLaunchKernelGGL(tg_prepare_kernel, dim3(N), dim3(TG_MAXG), 0, S(stream), glabels, gbboxes, n_gt, G, 0, ws);
  XDET_LAUNCH_CHECK();
  return launch_match(c, N, G, ws, high_thr, low_thr, prior_scaling4, labels, targets, scores, S(stream));
}

int xdet_encode_rois(const float* rois, int R, const int32_t* glabels, const float* gbboxes, const int32_t* n_gt, int N, int G,
                     float allowed_border, float fg_thr, float bg_high_thr, float bg_low_thr, const float* prior_scaling4,
                     int rois_per_image, float fg_fraction, uint32_t seed, const int32_t* image_ids, void* workspace,
                     float* out_rois, float* out_targets, int32_t* out_labels, float* out_scores, int32_t* out_index,
                     int32_t* counts, int32_t* all_labels, float* all_targets, float* all_scores, void* stream) {
  XDET_REQUIRE(R > 0, "encode_rois: R must be positive");
  XDET_TRY(check_sizes("encode_rois", N, G, prior_scaling4));
  XDET_REQUIRE((int64_t)R + G <= TG_MAXM, "encode_rois: at most 8192 candidates (R + G) per image");
  XDET_REQUIRE(rois_per_image > 0 && rois_per_image <= TG_MAXM, "encode_rois: rois_per_image must be in [1, 8192]");
  XDET_REQUIRE(fg_fraction >= 0.f && fg_fraction <= 1.f, "encode_rois: fg_fraction must be in [0, 1]");
  XDET_REQUIRE(std::isfinite(allowed_border) && std::isfinite(fg_thr) && std::isfinite(bg_high_thr) && std::isfinite(bg_low_thr),
               "encode_rois: the border and the thresholds must be finite");
  XDET_TRY(check_ground_truth("encode_rois", glabels, gbboxes, n_gt, workspace));
  XDET_REQUIRE(rois && out_rois && out_targets && out_labels && out_scores, "encode_rois: NULL argument");
  XDET_REQUIRE(aligned16(rois) && aligned16(out_rois) && aligned16(out_targets) && aligned16(all_targets),
               "encode_rois: box and target arrays must be 16-byte aligned");
  const int M = R + G;
  const TgWorkspace ws = ws_carve(workspace, 256, tg_layout, N, M, G);
  int* lab = all_labels ? all_labels : ws.lab;
  float* tg = all_targets ? all_targets : ws.tg;
  float* sc = all_scores ? all_scores : ws.sc;
  TgCand c{};
  c.rois = rois;
  c.R = R;
  c.M = M;
  tg_border(allowed_border, &c.lo, &c.hi);
  TgSample p{};
  p.rois = rois;
  p.R = R;
  p.G = G;
  p.M = M;
  p.rpi = rois_per_image;
  p.exp_fg = (int)std::nearbyint((float)rois_per_image * fg_fraction);       // tf.round: half to even
  p.bg_low = bg_low_thr;
  p.seed_word = tg_mix(seed ^ 0x9E3779B9u);
  p.image_ids = image_ids;
  p.P = 1;
  while (p.P < std::max(M, rois_per_image)) p.P <<= 1;
  p.out_rois = out_rois;
  p.out_targets = out_targets;
  p.out_labels = out_labels;
  p.out_scores = out_scores;
  p.out_index = out_index;
  p.counts = counts;
  const int lds = p.P * 8 + rois_per_image * 4;
  XDET_TRY(ensure_dynamic_lds(g_sample_once, reinterpret_cast<const void*>(tg_sample_kernel), TG_MAXM * 8 + TG_MAXM * 4));
  hipLaunchKernelGGL(tg_prepare_kernel, dim3(N), dim3(TG_MAXG), 0, S(stream), glabels, gbboxes, n_gt, G, 1, ws);
  XDET_LAUNCH_CHECK();
  XDET_TRY(launch_match(c, N, G, ws, fg_thr, bg_high_thr, prior_scaling4, lab, tg, sc, S(stream)));
  hipLaunchKernelGGL(tg_sample_kernel, dim3(N), dim3(TG_ST), lds, S(stream), p, ws, lab, tg, sc);
  XDET_LAUNCH_CHECK();
  return XDET_OK;
}

}  // extern "C"
