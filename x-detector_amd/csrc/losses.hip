// Training losses on the GPU: everything of lighr_head_model_fn between the logits and the scalar loss
// (light_head_rfcn_train.py:257-275, 312-413; net/xception_body.py:502-533, 560) and the gradients with respect to the logits.
//   select_samples + rpn_cross_entropy + rpn_loc_loss          -> xdet_rpn_loss
//   head_loss_func + the OHEM top_k of get_head + reduce_mean   -> xdet_head_loss
// The contract is written out in include/xdet.h and DESIGN.md 4.29; xdet/losses.py holds the same statement in NumPy.
// Compiled with -ffp-contract=off: every f32 operation rounds on its own.
//
// xdet_rpn_loss.  The selection draws from the whole batch flattened (M = N * Hh * Ww * A anchors, millions), so the
// one-workgroup sampler of targets.hip cannot serve it.  The keys of the defined shuffle are a bijection of the element:
// they are recomputed from the index wherever they are needed and never stored for more than the <= S selected ones.
//   ls_hist_kernel<0>   a pass over the labels: per-workgroup class counts (for the index-order compaction) and the
//                       histogram of the keys' top 8 bits, per class
//   ls_pick_kernel      one workgroup: scans the workgroup counts, decides per class whether it is taken whole (|class| <
//                       expected) or down-sampled, and narrows the radix select of the k-th smallest key by one digit
//   ls_hist_kernel<1,2> + ls_pick_kernel   the next 12 + 12 bits of the keys under the prefix: the exact threshold key
//   ls_compact_kernel   whole classes -> keep[] in index order (prefix sums); down-sampled ones -> their k keys, unordered
//   ls_order_kernel     one workgroup: sorts those keys in LDS (32-bit, <= 32768), turns them back into elements, forms
//                       the up-sampling tail, the multiplicity of every kept row, sel_index and counts
//   ls_fill_kernel      zeroes every cls / box channel of the gradient
//   ls_rows_kernel      a lane per kept row: cross entropy, smooth L1, the row's gradient times its multiplicity
//   ls_final_kernel     the partial sums in a fixed order -> losses
// A dependency between workgroups is a kernel boundary; nothing waits inside a kernel.  Float sums are trees of a fixed
// shape (no float atomics): the same call gives the same bits.  The integer atomics (histograms, the slot claims of the
// unordered key list -- one per workgroup and class, the keys staged in LDS) cannot change a result.
//
// xdet_head_loss: hl_image_kernel, one workgroup per image (a lane per ROI: the per-ROI value is one instruction sequence,
// so duplicated ROIs tie bit for bit; bitonic sort of (~loss bits, index) for the stable descending top-K), hl_final_kernel.
#include "common.h"
#include "shuffle.h"

#include <algorithm>
#include <climits>
#include <cmath>

namespace xdet {

constexpr int LS_T = 512;          // threads of the passes over the labels
constexpr int LS_NB = 1024;        // at most this many workgroups per pass; each owns one contiguous chunk of the anchors
constexpr int LS_OT = 1024;        // threads of the one-workgroup kernels
constexpr int LS_MAXS = 32768;     // N * anchors_per_image: 32-bit keys of one class in 128 KB of LDS
constexpr int LS_RT = 256;         // threads of the rows kernel
constexpr int LS_B0 = 256, LS_B1 = 4096;     // radix digits: 8 + 12 + 12 bits
constexpr int LS_CAP = 2048;       // keys a workgroup of the compaction stages in LDS per class before it claims slots for them
constexpr int HL_T = 256;          // threads of the head kernel
constexpr int HL_MAXP = 8192, HL_MAXC = 128;
enum { LS_NONE = 0, LS_ALL = 1, LS_SELECT = 2 };

struct LsCtl {                     // cleared by the call
  int hist0[2][LS_B0];
  int hist1[2][LS_B1];
  int hist2[2][LS_B1];
  int ccount[2];                   // slots handed out in ckeys
  int pad[2];
};

struct LsState {                   // every field written by the call before it is read
  int n_pos, n_neg, n_fg, n_bg;
  int mode[2];                     // class 0 = positives, 1 = negatives
  int krem[2];                     // keys still to take under `prefix`
  unsigned prefix[2];              // the digits chosen so far; after the third pick the threshold key itself
  int n_sel_pos;                   // selected rows (with multiplicity) whose label > 0
  int pad[5];
};

struct LsWorkspace {
  LsCtl* ctl;
  LsState* st;
  int* blockcnt;                   // [2][LS_NB] members of the class in the workgroup's chunk
  int* blockoff;                   // [2][LS_NB] their exclusive prefix sums
  unsigned* ckeys;                 // [2][S] keys <= threshold of a down-sampled class
  int* keep;                       // [S] fg ++ bg
  int* mult;                       // [S] multiplicity of keep[p] among the S selected rows
  float* partial;                  // [LS_NB][4] per-workgroup loss sums (RPN: rows kernel; head: per image)
};

// the one description of the workspace (S = 0: the head loss, which uses `partial` alone)
static LsWorkspace ls_layout(WsWalk& w, int S) {
  const size_t s = (size_t)S;
  LsWorkspace ws;
  ws.ctl = w.take<LsCtl>(1);
  ws.st = w.take<LsState>(1);
  ws.blockcnt = w.take<int>(2 * LS_NB);
  ws.blockoff = w.take<int>(2 * LS_NB);
  ws.ckeys = w.take<unsigned>(2 * s);
  ws.keep = w.take<int>(s);
  ws.mult = w.take<int>(s);
  ws.partial = w.take<float>((size_t)LS_NB * 4);
  return ws;
}

// ---- arithmetic shared by both losses ------------------------------------------------------------------------------

struct SmoothL1 {
  float sigma2, thr, c1, c2;       // sigma^2, 1 / sigma^2, 0.5 * sigma^2, 0.5 / sigma^2
};
static SmoothL1 make_smooth_l1(float sigma) {
  SmoothL1 s;
  s.sigma2 = sigma * sigma;
  s.thr = 1.f / s.sigma2;
  s.c1 = 0.5f * s.sigma2;
  s.c2 = 0.5f / s.sigma2;
  return s;
}
__device__ __forceinline__ float sl1(const SmoothL1& s, float d) {
  const float a = fabsf(d);
  return a < s.thr ? (d * d) * s.c1 : a - s.c2;
}
__device__ __forceinline__ float sl1_grad(const SmoothL1& s, float d) {
  return fabsf(d) < s.thr ? d * s.sigma2 : (d > 0.f ? 1.f : -1.f);
}

// sum over the workgroup in a fixed tree: lanes of a wave by xor-shuffles, then the waves in order.  All threads call it;
// s_red holds one float per wave.  Every thread gets the total.
template <int T>
__device__ float block_sum(float v, float* s_red) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  __syncthreads();                                  // (s_red may still be read from an earlier call)
  if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = v;
  __syncthreads();
  float t = 0.f;
  for (int w = 0; w < T / 64; ++w) t += s_red[w];
  return t;
}

// exclusive prefix sum over the LS_OT threads of a workgroup; s_wave: LS_OT / 64 ints
__device__ int ls_exscan(int v, int* s_wave, int* total) {
  const int ln = threadIdx.x & 63, wv = threadIdx.x >> 6;
  int inc = v;
  for (int o = 1; o < 64; o <<= 1) {
    const int t = __shfl_up(inc, o);
    if (ln >= o) inc += t;
  }
  __syncthreads();
  if (ln == 63) s_wave[wv] = inc;
  __syncthreads();
  int off = 0, tot = 0;
  for (int w = 0; w < LS_OT / 64; ++w) {
    if (w < wv) off += s_wave[w];
    tot += s_wave[w];
  }
  *total = tot;
  return off + inc - v;
}

// ---- xdet_rpn_loss: the selection ----------------------------------------------------------------------------------

__device__ __forceinline__ int ls_class(int label) { return label > 0 ? 0 : (label == 0 ? 1 : -1); }

// grid nb, LS_T threads; workgroup b owns the anchors [b * chunk, min((b + 1) * chunk, M))
template <int PASS>
__global__ __launch_bounds__(LS_T) void ls_hist_kernel(const int* __restrict__ labels, int M, int chunk, unsigned word, LsWorkspace ws) {
  constexpr int BINS = PASS == 0 ? LS_B0 : LS_B1;
  __shared__ int s_hist[2][BINS];
  __shared__ int s_cnt[2];
  const int tid = threadIdx.x;
  bool on0 = true, on1 = true;
  unsigned pre0 = 0u, pre1 = 0u;
  if (PASS > 0) {
    on0 = ws.st->mode[0] == LS_SELECT;
    on1 = ws.st->mode[1] == LS_SELECT;
    pre0 = ws.st->prefix[0];
    pre1 = ws.st->prefix[1];
    if (!on0 && !on1) return;                      // (uniform over the grid)
  }
  for (int i = tid; i < 2 * BINS; i += LS_T) (&s_hist[0][0])[i] = 0;
  if (tid < 2) s_cnt[tid] = 0;
  __syncthreads();
  const int begin = min((int64_t)blockIdx.x * chunk, (int64_t)M), end = (int)min((int64_t)begin + chunk, (int64_t)M);
  int cnt0 = 0, cnt1 = 0;
  for (int i = begin + tid; i < end; i += LS_T) {
    const int c = ls_class(labels[i]);
    if (c < 0) continue;
    const unsigned key = tg_mix(word ^ (2u * (unsigned)i));
    const bool on = c ? on1 : on0;
    const unsigned pre = c ? pre1 : pre0;
    if (PASS == 0) {
      cnt0 += c == 0;
      cnt1 += c == 1;
      atomicAdd(&s_hist[c][key >> 24], 1);
    } else if (PASS == 1) {
      if (on && (key >> 24) == pre) atomicAdd(&s_hist[c][(key >> 12) & 0xFFFu], 1);
    } else {
      if (on && (key >> 12) == pre) atomicAdd(&s_hist[c][key & 0xFFFu], 1);
    }
  }
  if (PASS == 0) {
    if (cnt0) atomicAdd(&s_cnt[0], cnt0);
    if (cnt1) atomicAdd(&s_cnt[1], cnt1);
  }
  __syncthreads();
  int* g = PASS == 0 ? &ws.ctl->hist0[0][0] : (PASS == 1 ? &ws.ctl->hist1[0][0] : &ws.ctl->hist2[0][0]);
  for (int i = tid; i < 2 * BINS; i += LS_T) {
    const int h = (&s_hist[0][0])[i];
    if (h) atomicAdd(&g[i], h);
  }
  if (PASS == 0 && tid < 2) ws.blockcnt[tid * LS_NB + blockIdx.x] = s_cnt[tid];
}

// one workgroup of LS_OT threads, after pass `pass` of the histograms
__global__ __launch_bounds__(LS_OT) void ls_pick_kernel(int pass, int nb, int S, int exp_fg, LsWorkspace ws) {
  __shared__ int s_wave[LS_OT / 64];
  __shared__ LsState s_st;
  const int tid = threadIdx.x;
  if (pass == 0) {
    int tot[2];
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const int v = tid < nb ? ws.blockcnt[c * LS_NB + tid] : 0;
      const int ex = ls_exscan(v, s_wave, &tot[c]);
      if (tid < nb) ws.blockoff[c * LS_NB + tid] = ex;
    }
    if (tid == 0) {
      LsState st{};
      st.n_pos = tot[0];
      st.n_neg = tot[1];
      st.n_fg = min(tot[0], exp_fg);
      const int exp_bg = S - st.n_fg;
      st.n_bg = min(tot[1], exp_bg);
      st.mode[0] = tot[0] < exp_fg ? LS_ALL : (exp_fg == 0 ? LS_NONE : LS_SELECT);
      st.mode[1] = tot[1] < exp_bg ? LS_ALL : (exp_bg == 0 ? LS_NONE : LS_SELECT);
      st.krem[0] = exp_fg;
      st.krem[1] = exp_bg;
      s_st = st;
    }
  } else if (tid == 0) {
    s_st = *ws.st;
  }
  __syncthreads();
  const int bins = pass == 0 ? LS_B0 : LS_B1, bits = pass == 0 ? 8 : 12;
  for (int c = 0; c < 2; ++c) {
    if (s_st.mode[c] != LS_SELECT) continue;               // (uniform)
    const int* h = pass == 0 ? ws.ctl->hist0[c] : (pass == 1 ? ws.ctl->hist1[c] : ws.ctl->hist2[c]);
    const int krem = s_st.krem[c];
    int v[4], sum = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      v[q] = 4 * tid + q < bins ? h[4 * tid + q] : 0;
      sum += v[q];
    }
    int total;
    int ex = ls_exscan(sum, s_wave, &total);
    if (ex < krem && krem <= ex + sum) {                   // the bin of the krem-th smallest key: one thread
      int b = 0;
      bool found = false;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        if (!found && ex + v[q] >= krem) {
          b = q;
          found = true;
        }
        if (!found) ex += v[q];
      }
      s_st.prefix[c] = (s_st.prefix[c] << bits) | (unsigned)(4 * tid + b);
      s_st.krem[c] = krem - ex;
    }
  }
  __syncthreads();
  if (tid == 0) *ws.st = s_st;
}

// grid nb, LS_T threads
__global__ __launch_bounds__(LS_T) void ls_compact_kernel(const int* __restrict__ labels, int M, int chunk, unsigned word, int S,
                                                          LsWorkspace ws) {
  __shared__ int s_wave[2][LS_T / 64];
  __shared__ unsigned s_keys[2][LS_CAP];
  __shared__ int s_n[2], s_base[2];
  const int tid = threadIdx.x, wv = tid >> 6, ln = tid & 63;
  const LsState st = *ws.st;
  const bool any_sel = st.mode[0] == LS_SELECT || st.mode[1] == LS_SELECT;
  if (tid < 2) s_n[tid] = 0;
  __syncthreads();
  // the staged keys of both classes to ckeys: one slot claim per class instead of one per key
  auto flush = [&]() {
    if (tid < 2) s_base[tid] = s_n[tid] ? atomicAdd(&ws.ctl->ccount[tid], s_n[tid]) : 0;
    __syncthreads();
    for (int c = 0; c < 2; ++c)
      for (int i = tid; i < s_n[c]; i += LS_T)
        if (s_base[c] + i < S) ws.ckeys[(int64_t)c * S + s_base[c] + i] = s_keys[c][i];
    __syncthreads();
    if (tid < 2) s_n[tid] = 0;
    __syncthreads();
  };
  const bool any_all = st.mode[0] == LS_ALL || st.mode[1] == LS_ALL;
  int run0 = ws.blockoff[blockIdx.x], run1 = ws.blockoff[LS_NB + blockIdx.x];
  const int begin = min((int64_t)blockIdx.x * chunk, (int64_t)M), end = (int)min((int64_t)begin + chunk, (int64_t)M);
  for (int i0 = begin; i0 < end; i0 += LS_T) {
    const int i = i0 + tid;
    const int c = i < end ? ls_class(labels[i]) : -1;
    const int mode = c < 0 ? LS_NONE : (c ? st.mode[1] : st.mode[0]);
    if (mode == LS_SELECT) {
      const unsigned key = tg_mix(word ^ (2u * (unsigned)i));
      if (key <= (c ? st.prefix[1] : st.prefix[0])) s_keys[c][atomicAdd(&s_n[c], 1)] = key;      // (room for a tile: see below)
    }
    if (any_sel) {                                         // (uniform)
      __syncthreads();
      const bool full = max(s_n[0], s_n[1]) > LS_CAP - LS_T;     // the next tile adds at most LS_T keys per class
      __syncthreads();                                     // every lane has read the counts before the next tile raises them
      if (full) flush();                                   // (uniform)
    }
    if (!any_all) continue;                                // (uniform)
    const unsigned long long m0 = __ballot(c == 0), m1 = __ballot(c == 1);
    if (ln == 0) {
      s_wave[0][wv] = __popcll(m0);
      s_wave[1][wv] = __popcll(m1);
    }
    __syncthreads();
    int off0 = 0, off1 = 0, tot0 = 0, tot1 = 0;
    for (int w = 0; w < LS_T / 64; ++w) {
      if (w < wv) {
        off0 += s_wave[0][w];
        off1 += s_wave[1][w];
      }
      tot0 += s_wave[0][w];
      tot1 += s_wave[1][w];
    }
    if (mode == LS_ALL) {
      const int r = (c ? st.n_fg + run1 + off1 : run0 + off0) + __popcll((c ? m1 : m0) & ((1ull << ln) - 1ull));
      if (r < S) ws.keep[r] = i;
    }
    run0 += tot0;
    run1 += tot1;
    __syncthreads();
  }
  if (any_sel) flush();
}

// ascending bitonic sort of P (a power of two) 32-bit words in LDS, all LS_OT threads (one pair per thread and pass:
// another loop than lds_bitonic_sort_u64 of shuffle.h)
__device__ void ls_sort(unsigned* s, int P) {
  for (int k = 2; k <= P; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int t = threadIdx.x; t < P / 2; t += LS_OT) {        // pair t: i has bit j clear, its partner has it set
        const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), p = i | j;
        const unsigned x = s[i], y = s[p];
        if ((x > y) == ((i & k) == 0)) { s[i] = y; s[p] = x; }
      }
      __syncthreads();
    }
}

__device__ __forceinline__ int ls_pow2(int n) {
  int p = 1;
  while (p < n) p <<= 1;
  return p;
}

// one workgroup of LS_OT threads, dynamic LDS: pow2(S) words
__global__ __launch_bounds__(LS_OT) void ls_order_kernel(unsigned word, int S, LsWorkspace ws, int* __restrict__ sel_index,
                                                         int* __restrict__ counts) {
  extern __shared__ unsigned s_sort[];
  __shared__ int s_npos;
  const int tid = threadIdx.x;
  const LsState st = *ws.st;
  const int n_keep = st.n_fg + st.n_bg;
  if (tid == 0) s_npos = 0;
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    if (st.mode[c] != LS_SELECT) continue;                 // (uniform)
    const int k = c ? st.n_bg : st.n_fg, base = c ? st.n_fg : 0, P = ls_pow2(k);
    __syncthreads();
    for (int i = tid; i < P; i += LS_OT) s_sort[i] = i < k ? ws.ckeys[(int64_t)c * S + i] : 0xFFFFFFFFu;
    __syncthreads();
    ls_sort(s_sort, P);
    for (int i = tid; i < k; i += LS_OT) ws.keep[base + i] = (int)((tg_unmix(s_sort[i]) ^ word) >> 1);      // stream 0: 2 * element
  }
  // fewer than S: every kept one (left div n_keep) + 1 times in order, then the first (left mod n_keep) positions of
  // shuffle(range(n_keep)), stream 1
  int reps = 1, full = S, rem = 0;
  if (n_keep > 0 && n_keep < S) {
    const int left = S - n_keep;
    reps = left / n_keep + 1;
    full = n_keep * reps;
    rem = left % n_keep;
  }
  for (int p = tid; p < n_keep; p += LS_OT) ws.mult[p] = reps;
  __syncthreads();                                         // keep[] and mult[] of this workgroup are read / rewritten below
  if (rem) {
    const int P = ls_pow2(n_keep);
    for (int i = tid; i < P; i += LS_OT) s_sort[i] = i < n_keep ? tg_mix(word ^ (2u * (unsigned)i + 1u)) : 0xFFFFFFFFu;
    __syncthreads();
    ls_sort(s_sort, P);
  }
  int npos = 0;
  for (int j = tid; j < S; j += LS_OT) {
    int e = -1;
    if (n_keep > 0) {
      int pos;
      if (j < full) {
        pos = j % n_keep;
      } else {
        pos = min((int)((tg_unmix(s_sort[j - full]) ^ word) >> 1), n_keep - 1);
        ws.mult[pos] = reps + 1;
      }
      e = ws.keep[pos];
      npos += pos < st.n_fg;
    }
    sel_index[j] = e;
  }
  if (npos) atomicAdd(&s_npos, npos);
  __syncthreads();
  if (tid == 0) {
    counts[0] = st.n_pos;
    counts[1] = st.n_neg;
    counts[2] = n_keep;
    counts[3] = s_npos;
    ws.st->n_sel_pos = s_npos;
  }
}

// ---- xdet_rpn_loss: losses and gradient ------------------------------------------------------------------------------

struct RpnRows {
  const float* rpn_out;
  int ld, cls_off, box_off, A, S;
  const int* labels;
  const float* targets;
  float fg_ratio;
  SmoothL1 sl;
  float* grad;             // may be NULL
};

// a lane per anchor: its two cls and four box channels
__global__ __launch_bounds__(256) void ls_fill_kernel(float* __restrict__ grad, int ld, int cls_off, int box_off, int A, int64_t total) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t px = i / A;
    const int a = (int)(i - px * A);
    float* row = grad + px * ld;
    *reinterpret_cast<float2*>(row + cls_off + 2 * a) = make_float2(0.f, 0.f);
    *reinterpret_cast<float4*>(row + box_off + 4 * a) = make_float4(0.f, 0.f, 0.f, 0.f);
  }
}

// grid ceil(S / LS_RT), LS_RT threads: lane p owns keep[p]
__global__ __launch_bounds__(LS_RT) void ls_rows_kernel(RpnRows r, LsWorkspace ws) {
  __shared__ float s_red[LS_RT / 64];
  const int p = blockIdx.x * LS_RT + threadIdx.x;
  const int n_keep = ws.st->n_fg + ws.st->n_bg, n_sel_pos = ws.st->n_sel_pos;
  float ce = 0.f, loc = 0.f;
  if (p < n_keep) {
    const int e = ws.keep[p];
    const float fm = (float)ws.mult[p];
    const bool y = r.labels[e] > 0;
    const int64_t px = e / r.A;
    const int a = e - (int)px * r.A;
    const float* row = r.rpn_out + px * r.ld;
    const float l0 = row[r.cls_off + 2 * a], l1 = row[r.cls_off + 2 * a + 1];
    const float mx = fmaxf(l0, l1);
    const float e0 = expf(l0 - mx), e1 = expf(l1 - mx);
    const float s = e0 + e1;
    ce = (logf(s) - ((y ? l1 : l0) - mx)) * fm;
    float4 gb = make_float4(0.f, 0.f, 0.f, 0.f);
    if (y) {
      const float4 b = *reinterpret_cast<const float4*>(row + r.box_off + 4 * a);
      const float4 t = *reinterpret_cast<const float4*>(r.targets + (int64_t)e * 4);
      const float dx = b.x - t.x, dy = b.y - t.y, dz = b.z - t.z, dw = b.w - t.w;
      loc = (((sl1(r.sl, dx) + sl1(r.sl, dy)) + sl1(r.sl, dz)) + sl1(r.sl, dw)) * fm;
      const float wb = (fm / (float)n_sel_pos) / r.fg_ratio;
      gb = make_float4(sl1_grad(r.sl, dx) * wb, sl1_grad(r.sl, dy) * wb, sl1_grad(r.sl, dz) * wb, sl1_grad(r.sl, dw) * wb);
    }
    if (r.grad) {
      float* grow = r.grad + px * r.ld;
      const float wc = fm / (float)r.S;
      *reinterpret_cast<float2*>(grow + r.cls_off + 2 * a) = make_float2((e0 / s - (y ? 0.f : 1.f)) * wc, (e1 / s - (y ? 1.f : 0.f)) * wc);
      if (y) *reinterpret_cast<float4*>(grow + r.box_off + 4 * a) = gb;
    }
  }
  const float sum_ce = block_sum<LS_RT>(ce, s_red);
  const float sum_loc = block_sum<LS_RT>(loc, s_red);
  if (threadIdx.x == 0) {
    ws.partial[blockIdx.x * 4] = sum_ce;
    ws.partial[blockIdx.x * 4 + 1] = sum_loc;
  }
}

// one workgroup of 256 threads: sums of column c of partial[nb][4] in a fixed order
__device__ float final_sum(const float* partial, int nb, int c, float* s_red) {
  float v = 0.f;
  for (int i = threadIdx.x; i < nb; i += 256) v += partial[i * 4 + c];
  return block_sum<256>(v, s_red);
}

__global__ __launch_bounds__(256) void ls_final_kernel(int nb, int S, float fg_ratio, LsWorkspace ws, float* __restrict__ losses) {
  __shared__ float s_red[4];
  const float sum_ce = final_sum(ws.partial, nb, 0, s_red), sum_loc = final_sum(ws.partial, nb, 1, s_red);
  if (threadIdx.x == 0) {
    const int n_keep = ws.st->n_fg + ws.st->n_bg, n_sel_pos = ws.st->n_sel_pos;
    const float ce = n_keep > 0 ? sum_ce / (float)S : 0.f;
    const float loc = n_sel_pos > 0 ? (sum_loc / (float)n_sel_pos) / fg_ratio : 0.f;
    losses[0] = ce;
    losses[1] = loc;
    losses[2] = ce + loc;
  }
}

// ---- xdet_head_loss --------------------------------------------------------------------------------------------------

struct HeadArgs {
  const float* cls_reg;
  int ld, cls_off, reg_off, P, C, K, ohem, P2;
  const int* labels;
  const float* targets;
  float fg_ratio, w;       // w = 1 / f32(N * K)
  SmoothL1 sl;
  float* per_roi;
  int* select;
  float* grad;             // may be NULL
  float* partial;          // [N][4]
};

// row max and sum of exp(x - max) in index order
__device__ __forceinline__ void hl_softmax_terms(const float* x, int C, float* mx, float* s) {
  float m = x[0];
  for (int j = 1; j < C; ++j) m = fmaxf(m, x[j]);
  float t = 0.f;
  for (int j = 0; j < C; ++j) t += expf(x[j] - m);
  *mx = m;
  *s = t;
}

// grid N, HL_T threads, dynamic LDS: P2 sort words, P ce, P loc floats, P selection flags
__global__ __launch_bounds__(HL_T) void hl_image_kernel(HeadArgs a) {
  extern __shared__ unsigned long long s_dyn[];
  __shared__ float s_red[HL_T / 64];
  unsigned long long* s_sort = s_dyn;
  float* s_ce = reinterpret_cast<float*>(s_dyn + a.P2);
  float* s_loc = s_ce + a.P;
  unsigned char* s_sel = reinterpret_cast<unsigned char*>(s_loc + a.P);
  const int n = blockIdx.x, tid = threadIdx.x;
  const int64_t r0 = (int64_t)n * a.P;
  for (int p = tid; p < a.P2; p += HL_T) {
    if (p >= a.P) {
      s_sort[p] = ~0ull;
      continue;
    }
    const float* row = a.cls_reg + (r0 + p) * a.ld;
    const int lab = a.labels[r0 + p];
    float ce = 0.f, loc = 0.f;
    if (lab >= 0 && lab < a.C) {
      float mx, s;
      hl_softmax_terms(row + a.cls_off, a.C, &mx, &s);
      ce = logf(s) - (row[a.cls_off + lab] - mx);
      if (lab > 0) {
        const float* t = a.targets + (r0 + p) * 4;
        const float* g = row + a.reg_off;
        loc = (((sl1(a.sl, g[0] - t[0]) + sl1(a.sl, g[1] - t[1])) + sl1(a.sl, g[2] - t[2])) + sl1(a.sl, g[3] - t[3])) / a.fg_ratio;
      }
    }
    const float l = ce + loc;
    a.per_roi[r0 + p] = l;
    s_ce[p] = ce;
    s_loc[p] = loc;
    s_sel[p] = 0;
    // descending by value, equal values in ascending index order (l >= 0: its bits order like the value)
    s_sort[p] = ((unsigned long long)(~__float_as_uint(l)) << 32) | (unsigned)p;
  }
  __syncthreads();
  if (a.ohem) lds_bitonic_sort_u64<HL_T>(s_sort, a.P2);
  float sl = 0.f, sc = 0.f, so = 0.f;
  for (int r = tid; r < a.K; r += HL_T) {
    const int e = a.ohem ? min((int)(s_sort[r] & 0xFFFFFFFFull), a.P - 1) : r;
    a.select[(int64_t)n * a.K + r] = e;
    s_sel[e] = 1;
    sc += s_ce[e];
    so += s_loc[e];
    sl += s_ce[e] + s_loc[e];
  }
  const float t_l = block_sum<HL_T>(sl, s_red), t_c = block_sum<HL_T>(sc, s_red), t_o = block_sum<HL_T>(so, s_red);
  if (tid == 0) {
    a.partial[n * 4] = t_l;
    a.partial[n * 4 + 1] = t_c;
    a.partial[n * 4 + 2] = t_o;
  }
  if (!a.grad) return;
  // (the block_sum barriers have published s_sel)
  for (int p = tid; p < a.P; p += HL_T) {
    const float* row = a.cls_reg + (r0 + p) * a.ld;
    float* g = a.grad + (r0 + p) * a.ld;
    const int lab = a.labels[r0 + p];
    const bool on = s_sel[p] && lab >= 0 && lab < a.C;
    float mx = 0.f, s = 1.f;
    if (on) hl_softmax_terms(row + a.cls_off, a.C, &mx, &s);
    for (int j = 0; j < a.C; ++j) g[a.cls_off + j] = on ? (expf(row[a.cls_off + j] - mx) / s - (j == lab ? 1.f : 0.f)) * a.w : 0.f;
    const bool reg = on && lab > 0;
    for (int j = 0; j < 4; ++j)
      g[a.reg_off + j] = reg ? (sl1_grad(a.sl, row[a.reg_off + j] - a.targets[(r0 + p) * 4 + j]) / a.fg_ratio) * a.w : 0.f;
  }
}

__global__ __launch_bounds__(256) void hl_final_kernel(const float* __restrict__ partial, int N, float count, float* __restrict__ losses) {
  __shared__ float s_red[4];
  const float t_l = final_sum(partial, N, 0, s_red), t_c = final_sum(partial, N, 1, s_red), t_o = final_sum(partial, N, 2, s_red);
  if (threadIdx.x == 0) {
    losses[0] = t_l / count;
    losses[1] = t_c / count;
    losses[2] = t_o / count;
  }
}

static DeviceOnce g_order_once, g_head_once;

static bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

static int hl_lds_bytes(int P, int P2) { return P2 * 8 + P * 8 + (P + 15) / 16 * 16; }

}  // namespace xdet

using namespace xdet;

static inline hipStream_t S(void* s) { return reinterpret_cast<hipStream_t>(s); }

extern "C" {

size_t xdet_losses_workspace_bytes(int N, int anchors_per_image) {
  if (N <= 0 || N > LS_NB || anchors_per_image < 0 || (int64_t)N * anchors_per_image > LS_MAXS) return 0;
  return ws_measure(256, ls_layout, N * anchors_per_image);
}

int xdet_rpn_loss(const float* rpn_out, int ld, int cls_off, int box_off, int N, int Hh, int Ww, int A, const int32_t* labels,
                  const float* targets, int anchors_per_image, float fg_ratio, uint32_t seed, float sigma, void* workspace,
                  int32_t* sel_index, int32_t* counts, float* losses, float* grad_rpn_out, void* stream) {
  XDET_REQUIRE(N > 0 && Hh > 0 && Ww > 0 && A > 0, "rpn_loss: N, Hh, Ww and A must be positive");
  const int64_t M64 = (int64_t)N * Hh * Ww * A;
  XDET_REQUIRE(M64 <= (1 << 27), "rpn_loss: at most 2^27 anchors in the batch");
  XDET_REQUIRE(anchors_per_image > 0 && (int64_t)N * anchors_per_image <= LS_MAXS,
               "rpn_loss: N * anchors_per_image must be in [1, 32768]");
  XDET_REQUIRE(ld > 0 && ld % 4 == 0 && cls_off >= 0 && cls_off % 2 == 0 && box_off >= 0 && box_off % 4 == 0 &&
                   cls_off + 2 * A <= ld && box_off + 4 * A <= ld && (cls_off + 2 * A <= box_off || box_off + 4 * A <= cls_off),
               "rpn_loss: ld must be a multiple of 4, cls_off even, box_off a multiple of 4, both channel ranges inside ld and disjoint");
  XDET_REQUIRE(fg_ratio > 0.f && fg_ratio <= 1.f, "rpn_loss: fg_ratio must be in (0, 1]");
  XDET_REQUIRE(std::isfinite(sigma) && sigma > 0.f, "rpn_loss: sigma must be positive and finite");
  XDET_REQUIRE(rpn_out && labels && targets && workspace && sel_index && counts && losses, "rpn_loss: NULL argument");
  XDET_REQUIRE(aligned16(rpn_out) && aligned16(targets) && aligned16(workspace) && aligned16(grad_rpn_out),
               "rpn_loss: rpn_out, targets, the workspace and the gradient must be 16-byte aligned");
  const int M = (int)M64, Sn = N * anchors_per_image;
  const int exp_fg = (int)std::nearbyint((float)Sn * fg_ratio);             // tf.round: half to even
  const unsigned word = tg_mix(tg_mix(seed ^ 0x9E3779B9u) + 0u);            // image 0: the batch is one flat population
  const LsWorkspace ws = ws_carve(workspace, 256, ls_layout, Sn);
  const int nb = (int)std::min<int64_t>(cdiv(M, 8 * LS_T), LS_NB);
  const int chunk = round_up((int)cdiv(M, nb), LS_T);
  hipStream_t s = S(stream);
  XDET_TRY(ensure_dynamic_lds(g_order_once, reinterpret_cast<const void*>(ls_order_kernel), LS_MAXS * 4));
  XDET_HIP(hipMemsetAsync(ws.ctl, 0, sizeof(LsCtl), s));
  if (grad_rpn_out) {
    hipLaunchKernelGGL(ls_fill_kernel, dim3((unsigned)std::min<int64_t>(cdiv(M64, 256), 8192)), dim3(256), 0, s, grad_rpn_out, ld,
                       cls_off, box_off, A, M64);
    XDET_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(ls_hist_kernel<0>, dim3(nb), dim3(LS_T), 0, s, labels, M, chunk, word, ws);
  XDET_LAUNCH_CHECK();
  hipLaunchKernelGGL(ls_pick_kernel, dim3(1), dim3(LS_OT), 0, s, 0, nb, Sn, exp_fg, ws);
  XDET_LAUNCH_CHECK();
  hipLaunchKernelGGL(ls_hist_kernel<1>, dim3(nb), dim3(LS_T), 0, s, labels, M, chunk, word, ws);
  XDET_LAUNCH_CHECK();
  hipLaunchKernelGGL(ls_pick_kernel, dim3(1), dim3(LS_OT), 0, s, 1, nb, Sn, exp_fg, ws);
  XDET_LAUNCH_CHECK();
  hipLaunchKernelGGL(ls_hist_kernel<2>, dim3(nb), dim3(LS_T), 0, s, labels, M, chunk, word, ws);
  XDET_LAUNCH_CHECK();
  hipLaunchKernelGGL(ls_pick_kernel, dim3(1), dim3(LS_OT), 0, s, 2, nb, Sn, exp_fg, ws);
  XDET_LAUNCH_CHECK();
  hipLaunchKernelGGL(ls_compact_kernel, dim3(nb), dim3(LS_T), 0, s, labels, M, chunk, word, Sn, ws);
  XDET_LAUNCH_CHECK();
  int P2 = 1;
  while (P2 < Sn) P2 <<= 1;
  hipLaunchKernelGGL(ls_order_kernel, dim3(1), dim3(LS_OT), P2 * 4, s, word, Sn, ws, sel_index, counts);
  XDET_LAUNCH_CHECK();
  RpnRows r{};
  r.rpn_out = rpn_out;
  r.ld = ld;
  r.cls_off = cls_off;
  r.box_off = box_off;
  r.A = A;
  r.S = Sn;
  r.labels = labels;
  r.targets = targets;
  r.fg_ratio = fg_ratio;
  r.sl = make_smooth_l1(sigma);
  r.grad = grad_rpn_out;
  const int nrb = (int)cdiv(Sn, LS_RT);
  hipLaunchKernelGGL(ls_rows_kernel, dim3(nrb), dim3(LS_RT), 0, s, r, ws);
  XDET_LAUNCH_CHECK();
  hipLaunchKernelGGL(ls_final_kernel, dim3(1), dim3(256), 0, s, nrb, Sn, fg_ratio, ws, losses);
  XDET_LAUNCH_CHECK();
  return XDET_OK;
}

int xdet_head_loss(const float* cls_reg, int ld, int cls_off, int reg_off, int N, int P, int C, const int32_t* labels,
                   const float* targets, float fg_ratio, int ohem_k, float sigma, void* workspace, float* losses, float* per_roi,
                   int32_t* select, float* grad_cls_reg, void* stream) {
  XDET_REQUIRE(N > 0 && P > 0 && C > 1, "head_loss: N and P must be positive, C at least 2");
  XDET_REQUIRE(N <= LS_NB && P <= HL_MAXP && C <= HL_MAXC, "head_loss: at most 1024 images, 8192 ROIs per image, 128 classes");
  XDET_REQUIRE(ld > 0 && cls_off >= 0 && reg_off >= 0 && cls_off + C <= ld && reg_off + 4 <= ld &&
                   (cls_off + C <= reg_off || reg_off + 4 <= cls_off),
               "head_loss: both channel ranges must lie inside ld and be disjoint");
  XDET_REQUIRE(ohem_k >= 0, "head_loss: ohem_k must not be negative");
  XDET_REQUIRE(fg_ratio > 0.f && fg_ratio <= 1.f, "head_loss: fg_ratio must be in (0, 1]");
  XDET_REQUIRE(std::isfinite(sigma) && sigma > 0.f, "head_loss: sigma must be positive and finite");
  XDET_REQUIRE(cls_reg && labels && targets && workspace && losses && per_roi && select, "head_loss: NULL argument");
  XDET_REQUIRE(aligned16(workspace), "head_loss: the workspace must be 16-byte aligned");
  HeadArgs a{};
  a.cls_reg = cls_reg;
  a.ld = ld;
  a.cls_off = cls_off;
  a.reg_off = reg_off;
  a.P = P;
  a.C = C;
  a.ohem = ohem_k > 0;
  a.K = a.ohem ? std::min(ohem_k, P) : P;
  a.P2 = 1;
  while (a.P2 < P) a.P2 <<= 1;
  a.labels = labels;
  a.targets = targets;
  a.fg_ratio = fg_ratio;
  a.w = 1.f / (float)((int64_t)N * a.K);
  a.sl = make_smooth_l1(sigma);
  a.per_roi = per_roi;
  a.select = select;
  a.grad = grad_cls_reg;
  a.partial = ws_carve(workspace, 256, ls_layout, 0).partial;
  XDET_TRY(ensure_dynamic_lds(g_head_once, reinterpret_cast<const void*>(hl_image_kernel), hl_lds_bytes(HL_MAXP, HL_MAXP)));
  hipLaunchKernelGGL(hl_image_kernel, dim3(N), dim3(HL_T), hl_lds_bytes(P, a.P2), S(stream), a);
  XDET_LAUNCH_CHECK();
  hipLaunchKernelGGL(hl_final_kernel, dim3(1), dim3(256), 0, S(stream), a.partial, N, (float)((int64_t)N * a.K), losses);
  XDET_LAUNCH_CHECK();
  return XDET_OK;
}

}  // extern "C"
