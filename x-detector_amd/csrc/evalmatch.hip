// The scoring half of bboxes_eval on the GPU (light_head_rfcn_eval.py:288-296): eval_helper.bboxes_matching_batch
// (utility/eval_helper.py:700-830) as bboxes_matching_kernel and the update of metrics.streaming_tp_fp_arrays
// (utility/metrics.py:102-170) as tpfp_append_kernel.  The PR curve and the APs stay on the host (xdet/evaluation.py).
// Compiled with -ffp-contract=off: the IoU must round like the separately rounded f32 operations of the host port.
#include "common.h"
#include "device_mem.h"

#include <climits>
#include <cmath>
#include <memory>

namespace xdet {

constexpr int EM_MAXG = 512;      // ground-truth boxes per image (VOC's largest image has 42)
constexpr int EM_WAVES = 4;       // one wave per (image, class) pair
constexpr int EM_T = EM_WAVES * 64;
constexpr int EM_CPB = 8;         // classes per workgroup: 128 images x 20 classes = 384 workgroups of 4 waves
constexpr int EM_TILE = 4;        // detections a lane holds at a time: i = tile * 256 + t * 64 + lane
constexpr int AP_T = 1024;        // tpfp_append_kernel: one workgroup per class
constexpr int AP_SCAN = 1024;     // images per scan pass of the append kernel

// np.minimum / np.maximum propagate NaN (fminf / fmaxf drop it); a NaN coordinate then reaches the union, fails
// `union > 0` and the IoU is 0, as in evaluation.bboxes_jaccard
__device__ __forceinline__ float np_min(float a, float b) { return (a != a) ? a : ((b != b) ? b : fminf(a, b)); }
__device__ __forceinline__ float np_max(float a, float b) { return (a != a) ? a : ((b != b) ? b : fmaxf(a, b)); }

// The greedy walk of bboxes_matching carries only gmatch[k], and gmatch[k] is only ever set by a detection whose own best
// box is k: with k_i = first argmax_g IoU(det_i, g) * (label_g == class) and match_i = IoU(det_i, k_i) > thr,
//   first_k = min { i : match_i, k_i = k, not difficult_k },  tp_i = !difficult_{k_i} & match_i & (first_{k_i} == i),
//   fp_i = !difficult_{k_i} & !tp_i
// is the same function, and every detection's k_i is independent work.
// grid (N, ceil(C / EM_CPB)), EM_T threads.  The image's ground truth is staged in LDS once per workgroup; a wave takes the
// classes wave, wave + 4, ... of the workgroup's group; a lane owns detections lane, lane + 64, ...; first_k is an LDS
// minimum.  Detections are walked in tiles of 256 in ascending order: a later tile cannot lower first_k below an index of
// an earlier one, so a tile's flags are final once its own minima are in.
__global__ __launch_bounds__(EM_T) void bboxes_matching_kernel(
    const float* __restrict__ det_scores, const float* __restrict__ det_boxes, int C, int K,
    const int* __restrict__ glabels, const float* __restrict__ gbboxes, const unsigned char* __restrict__ gdifficults,
    const int* __restrict__ n_gt, int G, float thr, unsigned char* __restrict__ tp, unsigned char* __restrict__ fp,
    int* __restrict__ n_gbboxes, int* __restrict__ rec_counts, int* __restrict__ bad_per_image) {
  __shared__ float4 s_box[EM_MAXG];
  __shared__ float s_area[EM_MAXG];
  __shared__ int s_lab[EM_MAXG];
  __shared__ unsigned char s_diff[EM_MAXG];
  __shared__ int s_first[EM_WAVES][EM_MAXG];
  __shared__ int s_bad;

  const int n = blockIdx.x;
  const int tid = threadIdx.x, wv = tid >> 6, ln = tid & 63;
  const int ng = min(max(n_gt[n], 0), G);
  if (tid == 0) s_bad = 0;
  __syncthreads();
  for (int g = tid; g < ng; g += EM_T) {
    const float4 b = *reinterpret_cast<const float4*>(gbboxes + ((int64_t)n * G + g) * 4);
    s_box[g] = b;
    s_area[g] = (b.z - b.x) * (b.w - b.y);
    s_lab[g] = glabels[(int64_t)n * G + g];
    s_diff[g] = gdifficults[(int64_t)n * G + g] != 0;
  }
  // the forward's mark of a bad image: NaN in slot 0 of a class's scores (csrc/detect.hip)
  {
    bool isbad = false;
    for (int c = tid; c < C; c += EM_T) {
      const float s0 = det_scores[((int64_t)n * C + c) * K];
      isbad |= s0 != s0;
    }
    if (isbad) s_bad = 1;
  }
  __syncthreads();
  const bool bad = s_bad != 0;
  if (blockIdx.y == 0 && tid == 0 && bad_per_image) bad_per_image[n] = bad ? 1 : 0;

  const int n_tiles = (K + 64 * EM_TILE - 1) / (64 * EM_TILE);
  for (int cw = 0; cw < EM_CPB / EM_WAVES; ++cw) {
    const int c = blockIdx.y * EM_CPB + cw * EM_WAVES + wv;
    const bool have = c < C;
    const bool live = have && !bad && ng > 0;      // (no ground truth: bboxes_matching returns all-false flags)
    const int label = c + 1;
    const int64_t row = ((int64_t)n * C + c) * K;
    if (have) {
      int cnt = 0;
      if (!bad)
        for (int g0 = 0; g0 < ng; g0 += 64) {
          const int g = g0 + ln;
          cnt += __popcll(__ballot(g < ng && s_lab[g] == label && !s_diff[g]));
        }
      if (ln == 0) n_gbboxes[(int64_t)n * C + c] = cnt;
      for (int g = ln; g < ng; g += 64) s_first[wv][g] = INT_MAX;
    }
    __syncthreads();
    int n_rec = 0;
    for (int tile = 0; tile < n_tiles; ++tile) {
      // a detection's state between the two phases: k | match << 16 | difficult_k << 17
      int st[EM_TILE] = {};
      if (live) {
        float4 d[EM_TILE];
        float da[EM_TILE], best[EM_TILE];
        int bk[EM_TILE];
#pragma unroll
        for (int t = 0; t < EM_TILE; ++t) {
          const int i = (tile * EM_TILE + t) * 64 + ln;
          d[t] = i < K ? *reinterpret_cast<const float4*>(det_boxes + (row + i) * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
          da[t] = (d[t].z - d[t].x) * (d[t].w - d[t].y);
          best[t] = -1.f;       // every IoU * mask is >= 0 or NaN: box 0 always takes over
          bk[t] = 0;
        }
        for (int g = 0; g < ng; ++g) {
          const float4 b = s_box[g];
          const float ga = s_area[g];
          const float fm = s_lab[g] == label ? 1.f : 0.f;
#pragma unroll
          for (int t = 0; t < EM_TILE; ++t) {
            const float h = np_max(np_min(b.z, d[t].z) - np_max(b.x, d[t].x), 0.f);
            const float w = np_max(np_min(b.w, d[t].w) - np_max(b.y, d[t].y), 0.f);
            const float inter = h * w;
            const float uni = (-inter + ga) + da[t];
            float v = uni > 0.f ? inter / uni : 0.f;
            v = v * fm;
            // np.argmax: the first maximum, a NaN counting as the largest
            if (v > best[t] || (v != v && best[t] == best[t])) { best[t] = v; bk[t] = g; }
          }
        }
#pragma unroll
        for (int t = 0; t < EM_TILE; ++t) {
          const int i = (tile * EM_TILE + t) * 64 + ln;
          const bool match = best[t] > thr;
          const bool diff = s_diff[bk[t]] != 0;
          st[t] = bk[t] | (match ? 1 << 16 : 0) | (diff ? 1 << 17 : 0);
          if (i < K && match && !diff) atomicMin(&s_first[wv][bk[t]], i);
        }
      }
      __syncthreads();
      if (have) {
#pragma unroll
        for (int t = 0; t < EM_TILE; ++t) {
          const int i = (tile * EM_TILE + t) * 64 + ln;
          bool is_tp = false, is_fp = false;
          if (live && i < K) {
            const bool match = (st[t] >> 16) & 1, diff = (st[t] >> 17) & 1;
            is_tp = !diff && match && s_first[wv][st[t] & 0xFFFF] == i;
            is_fp = !diff && !is_tp;
          }
          bool rec = false;
          if (i < K) {
            tp[row + i] = is_tp;
            fp[row + i] = is_fp;
            rec = (is_tp || is_fp) && det_scores[row + i] > 1e-4f;     // streaming_tp_fp_arrays, remove_zero_scores
          }
          n_rec += __popcll(__ballot(rec));
        }
      }
    }
    if (have && ln == 0 && rec_counts) rec_counts[(int64_t)n * C + c] = n_rec;
    __syncthreads();      // s_first is reused by the wave's next class
  }
}

struct TpfpState {       // device side of the accumulator
  int* cursor;           // [C] records held per class
  long long* nobjects;   // [C]
  int* misc;             // [0] bad_images, [1] overflow
  float* scores;         // [C][cap]
  unsigned char* is_tp;  // [C][cap] 1 = TP, 0 = FP
  int* image_id;         // [C][cap]
  int* slot;             // [C][cap]
};

// grid C, AP_T threads: the class's records of this call land behind its cursor in (image index within the call, slot) order:
// counts per image (the matcher's rec_counts) -> exclusive scan over the images -> scatter; nothing depends on scheduling.
__global__ __launch_bounds__(AP_T) void tpfp_append_kernel(
    const float* __restrict__ det_scores, const unsigned char* __restrict__ tp, const unsigned char* __restrict__ fp,
    const int* __restrict__ n_gbboxes, const int* __restrict__ rec_counts, const int* __restrict__ bad_per_image,
    const int* __restrict__ image_ids, int N, int C, int K, int cap, TpfpState a) {
  __shared__ int s_part[AP_T / 64][2];
  __shared__ int s_tot[2];
  __shared__ int s_offs[AP_SCAN];
  __shared__ int s_carry;
  const int c = blockIdx.x;
  const int tid = threadIdx.x, wv = tid >> 6, ln = tid & 63;

  // totals of the call: records and objects of the class (and, in workgroup 0, the bad images)
  int recs = 0, objs = 0, nbad = 0;
  for (int n = tid; n < N; n += AP_T) {
    recs += rec_counts[(int64_t)n * C + c];
    objs += n_gbboxes[(int64_t)n * C + c];
    if (c == 0) nbad += bad_per_image[n];
  }
  for (int o = 32; o > 0; o >>= 1) {
    recs += __shfl_xor(recs, o);
    objs += __shfl_xor(objs, o);
    nbad += __shfl_xor(nbad, o);
  }
  if (ln == 0) { s_part[wv][0] = recs; s_part[wv][1] = objs; }
  __syncthreads();
  if (tid == 0) {
    int r = 0, o = 0;
    for (int w = 0; w < AP_T / 64; ++w) { r += s_part[w][0]; o += s_part[w][1]; }
    s_tot[0] = r;
    s_tot[1] = o;
    s_carry = 0;
  }
  __syncthreads();
  // bad images: one integer add per wave into the device counter (the sum does not depend on the order)
  if (c == 0 && ln == 0 && nbad) atomicAdd(&a.misc[0], nbad);
  const int total = s_tot[0];
  const int cur = a.cursor[c];
  if (total > cap - cur) {           // the call does not fit: nothing of it is appended for this class
    if (tid == 0) atomicOr(&a.misc[1], 1);
    return;
  }
  float* const o_s = a.scores + (int64_t)c * cap;
  unsigned char* const o_t = a.is_tp + (int64_t)c * cap;
  int* const o_i = a.image_id + (int64_t)c * cap;
  int* const o_k = a.slot + (int64_t)c * cap;
  for (int n0 = 0; n0 < N; n0 += AP_SCAN) {
    const int nn = min(AP_SCAN, N - n0);
    if (wv == 0) {                   // exclusive scan of the images' counts, 64 at a time
      int carry = s_carry;
      for (int j0 = 0; j0 < nn; j0 += 64) {
        const int j = j0 + ln;
        const int v = j < nn ? rec_counts[(int64_t)(n0 + j) * C + c] : 0;
        int inc = v;
        for (int o = 1; o < 64; o <<= 1) {
          const int up = __shfl_up(inc, o);
          if (ln >= o) inc += up;
        }
        if (j < nn) s_offs[j] = carry + inc - v;
        carry += __shfl(inc, 63);
      }
      if (ln == 0) s_carry = carry;
    }
    __syncthreads();
    for (int j = wv; j < nn; j += AP_T / 64) {
      const int n = n0 + j;
      if (rec_counts[(int64_t)n * C + c] == 0) continue;
      const int64_t row = ((int64_t)n * C + c) * K;
      const int id = image_ids[n];
      int pos = cur + s_offs[j];
      for (int k0 = 0; k0 < K; k0 += 64) {
        const int k = k0 + ln;
        bool is_tp = false, rec = false;
        float s = 0.f;
        if (k < K) {
          is_tp = tp[row + k] != 0;
          s = det_scores[row + k];
          rec = (is_tp || fp[row + k] != 0) && s > 1e-4f;
        }
        const unsigned long long m = __ballot(rec);
        if (rec) {
          const int p = pos + __popcll(m & ((1ull << ln) - 1ull));
          o_s[p] = s;
          o_t[p] = is_tp ? 1 : 0;
          o_i[p] = id;
          o_k[p] = k;
        }
        pos += __popcll(m);
      }
    }
    __syncthreads();
  }
  if (tid == 0) {
    a.cursor[c] = cur + total;
    a.nobjects[c] += s_tot[1];
  }
}

// ---- host side ----------------------------------------------------------------------------------------------------

static int check_matching_args(const void* det_scores, const void* det_boxes, int N, int C, int K, const void* glabels,
                               const void* gbboxes, const void* gdifficults, const void* n_gt, int G, float thr) {
  XDET_REQUIRE(N > 0 && C > 0 && K > 0 && G > 0, "bboxes_matching: N, C, K and G must be positive");
  XDET_REQUIRE(G <= EM_MAXG, "bboxes_matching: at most 512 ground-truth boxes per image");
  XDET_REQUIRE(det_scores && det_boxes && glabels && gbboxes && gdifficults && n_gt, "bboxes_matching: NULL argument");
  XDET_REQUIRE((reinterpret_cast<uintptr_t>(det_boxes) & 15) == 0 && (reinterpret_cast<uintptr_t>(gbboxes) & 15) == 0,
               "bboxes_matching: box arrays must be 16-byte aligned");
  XDET_REQUIRE(std::isfinite(thr), "bboxes_matching: the matching threshold must be finite");
  return XDET_OK;
}

static int launch_bboxes_matching(const float* det_scores, const float* det_boxes, int N, int C, int K, const int* glabels,
                           const float* gbboxes, const unsigned char* gdifficults, const int* n_gt, int G, float thr,
                           unsigned char* tp, unsigned char* fp, int* n_gbboxes, int* rec_counts, int* bad_per_image,
                           hipStream_t s) {
  hipLaunchKernelGGL(bboxes_matching_kernel, dim3(N, (C + EM_CPB - 1) / EM_CPB), dim3(EM_T), 0, s, det_scores, det_boxes, C, K,
                     glabels, gbboxes, gdifficults, n_gt, G, thr, tp, fp, n_gbboxes, rec_counts, bad_per_image);
  XDET_LAUNCH_CHECK();
  return XDET_OK;
}

struct TpfpScratch {     // per-batch results of the matcher, read by the append
  unsigned char *tp, *fp;  // [batch][C][K]
  int *n_gb, *rec;         // [batch][C]
  int* bad;                // [batch]
};

// The accumulator handle.  Laid out like the net handles (csrc/plan.h struct Plan: a virtual destructor, then the kind tag), so
// that an entry point given a handle of another type sees a tag that is not its own and returns XDET_ERR_INVALID_ARG.
struct TpfpAccumulator {
  virtual ~TpfpAccumulator() {}
  int plan_kind = 2;     // 0 / 1: the nets
  int C = 0, K = 0, cap = 0;
  int batch = 0;         // images the scratch is sized for
  DevMem<unsigned char> state_mem, scratch_mem;   // one block each: what `st` and `sc` point into
  TpfpState st{};
  TpfpScratch sc{};

  static TpfpState state_layout(WsWalk& w, int C, int cap) {
    const size_t n = (size_t)C * cap;
    return {w.take<int>(C), w.take<long long>(C), w.take<int>(4), w.take<float>(n), w.take<unsigned char>(n), w.take<int>(n),
            w.take<int>(n)};
  }
  static TpfpScratch scratch_layout(WsWalk& w, int N, int C, int K) {
    const size_t slots = (size_t)N * C * K, nc = (size_t)N * C;
    return {w.take<unsigned char>(slots), w.take<unsigned char>(slots), w.take<int>(nc), w.take<int>(nc), w.take<int>(N)};
  }
  // grow only, never shrink
  int reserve(int N) {
    if (N <= batch) return XDET_OK;
    batch = 0;
    // (freeing the smaller block waits for the device: a call that grows the scratch is the one that synchronises)
    XDET_TRY(scratch_mem.alloc(ws_measure(256, scratch_layout, N, C, K)));
    sc = ws_carve(scratch_mem.get(), 256, scratch_layout, N, C, K);
    batch = N;
    return XDET_OK;
  }
};

}  // namespace xdet

using namespace xdet;

static inline hipStream_t S(void* s) { return reinterpret_cast<hipStream_t>(s); }
static TpfpAccumulator* acc_of(void* acc) { return static_cast<TpfpAccumulator*>(acc); }
#define XDET_TPFP(acc, what) \
  XDET_REQUIRE((acc) != nullptr && acc_of(acc)->plan_kind == 2, what ": not a TP/FP accumulator handle")

extern "C" {

int xdet_bboxes_matching(const float* det_scores, const float* det_boxes, int N, int C, int K, const int32_t* glabels,
                         const float* gbboxes, const uint8_t* gdifficults, const int32_t* n_gt, int G,
                         float matching_threshold, uint8_t* tp, uint8_t* fp, int32_t* n_gbboxes, void* stream) {
  XDET_TRY(check_matching_args(det_scores, det_boxes, N, C, K, glabels, gbboxes, gdifficults, n_gt, G, matching_threshold));
  XDET_REQUIRE(tp && fp && n_gbboxes, "bboxes_matching: NULL output");
  return launch_bboxes_matching(det_scores, det_boxes, N, C, K, glabels, gbboxes, gdifficults, n_gt, G, matching_threshold, tp,
                                fp, n_gbboxes, nullptr, nullptr, S(stream));
}

int xdet_tpfp_create(void** acc, int C, int K, int capacity_per_class) {
  XDET_REQUIRE(acc, "tpfp_create: acc is NULL");
  XDET_REQUIRE(C > 0 && K > 0 && capacity_per_class > 0, "tpfp_create: C, K and the capacity must be positive");
  XDET_REQUIRE((int64_t)C * capacity_per_class <= INT_MAX, "tpfp_create: C * capacity_per_class must fit 31 bits");
  std::unique_ptr<TpfpAccumulator> a(new TpfpAccumulator());
  a->C = C;
  a->K = K;
  a->cap = capacity_per_class;
  XDET_TRY(a->state_mem.alloc(ws_measure(256, TpfpAccumulator::state_layout, C, a->cap)));
  a->st = ws_carve(a->state_mem.get(), 256, TpfpAccumulator::state_layout, C, a->cap);
  XDET_TRY(xdet_tpfp_reset(a.get(), nullptr));   // cursor, nobjects and misc start at 0
  XDET_HIP(hipStreamSynchronize(nullptr));   // (the accumulator is used from non-blocking streams, which do not wait for these)
  *acc = a.release();
  return XDET_OK;
}

int xdet_tpfp_destroy(void* acc) {
  XDET_TPFP(acc, "tpfp_destroy");
  delete acc_of(acc);
  return XDET_OK;
}

int xdet_tpfp_reset(void* acc, void* stream) {
  XDET_TPFP(acc, "tpfp_reset");
  TpfpAccumulator* a = acc_of(acc);
  XDET_HIP(hipMemsetAsync(a->st.cursor, 0, (size_t)a->C * 4, S(stream)));
  XDET_HIP(hipMemsetAsync(a->st.nobjects, 0, (size_t)a->C * 8, S(stream)));
  XDET_HIP(hipMemsetAsync(a->st.misc, 0, 16, S(stream)));
  return XDET_OK;
}

int xdet_tpfp_update(void* acc, const float* det_scores, const float* det_boxes, int N, const int32_t* image_ids,
                     const int32_t* glabels, const float* gbboxes, const uint8_t* gdifficults, const int32_t* n_gt, int G,
                     float matching_threshold, void* stream) {
  XDET_TPFP(acc, "tpfp_update");
  TpfpAccumulator* a = acc_of(acc);
  XDET_TRY(check_matching_args(det_scores, det_boxes, N, a->C, a->K, glabels, gbboxes, gdifficults, n_gt, G, matching_threshold));
  XDET_REQUIRE(image_ids, "tpfp_update: image_ids is NULL");
  XDET_TRY(a->reserve(N));
  XDET_TRY(launch_bboxes_matching(det_scores, det_boxes, N, a->C, a->K, glabels, gbboxes, gdifficults, n_gt, G, matching_threshold,
                                  a->sc.tp, a->sc.fp, a->sc.n_gb, a->sc.rec, a->sc.bad, S(stream)));
  hipLaunchKernelGGL(tpfp_append_kernel, dim3(a->C), dim3(AP_T), 0, S(stream), det_scores, a->sc.tp, a->sc.fp, a->sc.n_gb, a->sc.rec,
                     a->sc.bad, image_ids, N, a->C, a->K, a->cap, a->st);
  XDET_LAUNCH_CHECK();
  return XDET_OK;
}

int xdet_tpfp_read(void* acc, int32_t* counts_host, int64_t* nobjects_host, int32_t* bad_images_host, int32_t* overflow_host,
                   int64_t records_capacity, float* scores_host, uint8_t* is_tp_host, int32_t* image_id_host,
                   int32_t* slot_host, void* stream) {
  XDET_TPFP(acc, "tpfp_read");
  TpfpAccumulator* a = acc_of(acc);
  XDET_REQUIRE(counts_host && nobjects_host && bad_images_host && overflow_host, "tpfp_read: NULL argument");
  const bool want = scores_host || is_tp_host || image_id_host || slot_host;
  XDET_REQUIRE(!want || (scores_host && is_tp_host && image_id_host && slot_host && records_capacity >= 0),
               "tpfp_read: give all four record arrays or none");
  int misc[4];
  static_assert(sizeof(long long) == sizeof(int64_t), "nobjects is read as int64");
  XDET_HIP(hipMemcpyAsync(counts_host, a->st.cursor, (size_t)a->C * 4, hipMemcpyDeviceToHost, S(stream)));
  XDET_HIP(hipMemcpyAsync(nobjects_host, a->st.nobjects, (size_t)a->C * 8, hipMemcpyDeviceToHost, S(stream)));
  XDET_HIP(hipMemcpyAsync(misc, a->st.misc, 16, hipMemcpyDeviceToHost, S(stream)));
  XDET_HIP(hipStreamSynchronize(S(stream)));
  *bad_images_host = misc[0];
  *overflow_host = misc[1];
  if (!want) return XDET_OK;
  int64_t total = 0;
  for (int c = 0; c < a->C; ++c) total += counts_host[c];
  XDET_REQUIRE(total <= records_capacity, "tpfp_read: the record arrays are smaller than the sum of the counts");
  int64_t at = 0;
  for (int c = 0; c < a->C; ++c) {
    const size_t k = (size_t)counts_host[c], off = (size_t)c * a->cap;
    if (!k) continue;
    XDET_HIP(hipMemcpyAsync(scores_host + at, a->st.scores + off, k * 4, hipMemcpyDeviceToHost, S(stream)));
    XDET_HIP(hipMemcpyAsync(is_tp_host + at, a->st.is_tp + off, k, hipMemcpyDeviceToHost, S(stream)));
    XDET_HIP(hipMemcpyAsync(image_id_host + at, a->st.image_id + off, k * 4, hipMemcpyDeviceToHost, S(stream)));
    XDET_HIP(hipMemcpyAsync(slot_host + at, a->st.slot + off, k * 4, hipMemcpyDeviceToHost, S(stream)));
    at += (int64_t)k;
  }
  XDET_HIP(hipStreamSynchronize(S(stream)));
  return XDET_OK;
}

}  // extern "C"
