// The backward of the depthwise 3x3 conv y = depthwise(xe, k), xe = x or max(x, 0), stride 1, 'SAME', dilation d = 1 or 2
// (xdet_depthwise_backward, include/xdet.h), NHWC with a pixel stride per tensor, k as [3,3,C,1]; and the row add
// out = a + b the exit flow joins its branches with (xdet_add_rows).
//
//     dx[n,h,w,c]  = sum over taps (a,b) of g[n, h - (a-1)d, w - (b-1)d, c] * k[a,b,c]          (0 where x > 0 is false with relu_in)
//     dw[a,b,c]    = sum over pixels of xe[n, h + (a-1)d, w + (b-1)d, c] * g[n,h,w,c]
//                  = sum over pixels q of xe[q] * g[q - shift(a,b)]:  indexed by x's pixel, BOTH gradients read the same nine
//                    shifted pixels of g, so one pass makes both -- x and the nine g's are loaded once per pixel, dx is
//                    stored, and the nine products go to per-lane sums.
//
// The op is memory-bound: channels are contiguous, a lane owns four consecutive channels (channel_quad.h) and a wave one
// pixel of 256 channels (1 KB per tensor row), so every access is a full row segment; the nine g rows of a pixel are
// shared with the workgroup's neighbouring pixels and come from L1 / L2 -- HBM sees x and g once and dx once.  The address of
// an absent tap (outside the image) is replaced by the pixel's own, so ten loads are in flight per pixel with no branch
// between them; the term itself is skipped by a scalar branch (the pixel walk and the taps' bounds are wave-uniform).
//
//   dwb_kernel       one workgroup of four waves per (pixel chunk, 256-channel block): wave r takes the chunk's pixels r,
//                    r + 4, ... in order; the four waves' tap sums are added 0, 1, 2, 3 through LDS and go to the workspace
//   dwb_fold_kernel  one thread per (tap, channel) adds the chunks in index order -- a launch of its own: no fence, no ticket,
//                    no float atomic, so the same call gives the same bits over any workspace contents
//   add_rows_kernel  out = a + b over 32 rows x 256 channels per workgroup
// The chunks depend on (N, H, W) alone (dwb_sums, depthwise_backward_layout.h).  The file is compiled with -ffp-contract=off:
// every term is a plain f32 product added in f32, so dy * 2^k gives dx and dw * 2^k exactly.
#include "common.h"
#include "channel_quad.h"
#include "depthwise_backward_layout.h"
#include <algorithm>

namespace xdet {

constexpr int DWB_RL = 4;             // pixel lanes (waves) of a workgroup
constexpr int DWB_T = 64 * DWB_RL;    // threads: 4 pixel lanes x 64 channel quads
constexpr int DWB_CB = 256;           // channels per workgroup
constexpr int DWB_FOLD_T = 256;       // threads of the fold
constexpr int ADD_RL = 4, ADD_T = 64 * ADD_RL;   // the add: 4 row lanes x 64 channel quads
constexpr int ADD_ROWS = 32;          // rows per workgroup of the add
constexpr int ADD_MAX_C = 1 << 24;    // (65536 channel blocks along the grid's y)

struct DwbArgs {
  const float *x, *k, *dy;
  float *dx, *partial;
  int ld_x, ld_dy, ld_dx;
  int H, W, C, M, dil;
  int pixels_per_chunk;
  int vec_x, vec_dy, vec_dx;
  int relu_in;
};

// FAST: every tensor takes float4 accesses and C is a multiple of four, so no lane owns a partial quad: the pixel loop is
// ten unconditional 16-byte loads and one store, without the per-access choice between the vector and the scalar form
// (which, with its exec-mask branches, was most of the instructions a wave issued per pixel).  Same values, same order.
template <bool FAST>
__device__ __forceinline__ void dwb_load(const float* __restrict__ p, int left, bool vec, float (&v)[4]) {
  if (FAST) {
    const float4 t = *reinterpret_cast<const float4*>(p);
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
  } else {
    quad_load(p, left, vec, v);
  }
}

template <bool FAST>
__global__ __launch_bounds__(DWB_T) void dwb_kernel(DwbArgs a) {
  __shared__ float4 red[DWB_RL][DWB_TAPS][DWB_CB / 4];
  const int tid = threadIdx.x, lane = tid & 63;
  // the wave's index as a scalar: the pixel walk, the taps' bounds and the row addresses below are then wave-uniform (scalar
  // unit), and the vector unit is left with the products and sums
  const int rl = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int c0 = blockIdx.y * DWB_CB + lane * 4, left = a.C - c0;
  const int m0 = blockIdx.x * a.pixels_per_chunk, m1 = m0 + min(a.pixels_per_chunk, a.M - m0);
  const bool with_dx = a.dx != nullptr;
  // (x and dy do not overlap dx: the loads of the next pixel may pass the store of this one)
  const float* __restrict__ px = a.x;
  const float* __restrict__ pg = a.dy;
  float* __restrict__ pdx = a.dx;
  float acc[DWB_TAPS][4];
#pragma unroll
  for (int t = 0; t < DWB_TAPS; ++t)
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[t][e] = 0.f;
  if (left > 0 && m0 + rl < m1) {
    float k[DWB_TAPS][4];
#pragma unroll
    for (int t = 0; t < DWB_TAPS; ++t) {
#pragma unroll
      for (int e = 0; e < 4; ++e) k[t][e] = 0.f;
      if (with_dx) quad_load(a.k + t * a.C + c0, left, false, k[t]);
    }
    // (h, w) of the wave's pixel: divided once, then stepped with the pixel
    int w = (m0 + rl) % a.W, h = ((m0 + rl) / a.W) % a.H;
#pragma unroll 1      // (two pixels per trip measured the same and cost forty registers)
    for (int m = m0 + rl; m < m1; m += DWB_RL) {
      float x[4], g[DWB_TAPS][4];
      bool live[DWB_TAPS], interior = true;
      dwb_load<FAST>(px + (int64_t)m * a.ld_x + c0, left, a.vec_x, x);
#pragma unroll
      for (int t = 0; t < DWB_TAPS; ++t) {
        const int dh = (t / 3 - 1) * a.dil, dw = (t % 3 - 1) * a.dil;
        live[t] = h - dh >= 0 && h - dh < a.H && w - dw >= 0 && w - dw < a.W;      // the same for the whole wave
        interior = interior && live[t];
        const int src = live[t] ? m - (dh * a.W + dw) : m;                         // an absent tap's pixel is not read
        dwb_load<FAST>(pg + (int64_t)src * a.ld_dy + c0, left, a.vec_dy, g[t]);
      }
      float xe[4], s[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int e = 0; e < 4; ++e) xe[e] = a.relu_in ? (x[e] > 0.f ? x[e] : 0.f) : x[e];
      if (interior) {       // (scalar branches: most pixels have all nine taps)
#pragma unroll
        for (int t = 0; t < DWB_TAPS; ++t)
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            s[e] += g[t][e] * k[t][e];
            acc[t][e] += xe[e] * g[t][e];
          }
      } else {
#pragma unroll
        for (int t = 0; t < DWB_TAPS; ++t)
          if (live[t]) {    // an absent term is not added
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              s[e] += g[t][e] * k[t][e];
              acc[t][e] += xe[e] * g[t][e];
            }
          }
      }
      if (with_dx) {
        if (a.relu_in) {      // x > 0 is false for a NaN: it gets the gradient 0
#pragma unroll
          for (int e = 0; e < 4; ++e) s[e] = x[e] > 0.f ? s[e] : 0.f;
        }
        if (FAST)
          *reinterpret_cast<float4*>(pdx + (int64_t)m * a.ld_dx + c0) = make_float4(s[0], s[1], s[2], s[3]);
        else
          quad_store(pdx + (int64_t)m * a.ld_dx + c0, left, a.vec_dx, s);
      }
      for (w += DWB_RL; w >= a.W; w -= a.W) h = h + 1 == a.H ? 0 : h + 1;
    }
  }
#pragma unroll
  for (int t = 0; t < DWB_TAPS; ++t) red[rl][t][lane] = make_float4(acc[t][0], acc[t][1], acc[t][2], acc[t][3]);
  __syncthreads();
  const int c = blockIdx.y * DWB_CB + tid;
  if (tid < DWB_CB && c < a.C) {
    const float* r = reinterpret_cast<const float*>(red);
    float* out = a.partial + (int64_t)blockIdx.x * DWB_TAPS * a.C + c;
#pragma unroll
    for (int t = 0; t < DWB_TAPS; ++t) {
      float v = r[(0 * DWB_TAPS + t) * DWB_CB + tid];
#pragma unroll
      for (int q = 1; q < DWB_RL; ++q) v += r[(q * DWB_TAPS + t) * DWB_CB + tid];
      out[t * a.C] = v;
    }
  }
}

__global__ __launch_bounds__(DWB_FOLD_T) void dwb_fold_kernel(const float* __restrict__ partial, int n_chunks, int C,
                                                         float* __restrict__ dw) {
  const int i = blockIdx.x * DWB_FOLD_T + threadIdx.x;  // (tap, channel): dw is [9][C]
  if (i < DWB_TAPS * C) dw[i] = fold_chunks(partial, n_chunks, DWB_TAPS * C, i);
}

// (no __restrict__: out may be a)
__global__ __launch_bounds__(ADD_T) void add_rows_kernel(const float* a, int ld_a, const float* b, int ld_b, float* out,
                                                         int ld_out, int M, int C, int vec_a, int vec_b, int vec_out) {
  const int lane = threadIdx.x & 63, rl = threadIdx.x >> 6;
  const int c0 = blockIdx.y * DWB_CB + lane * 4, left = C - c0;
  if (left <= 0) return;
  const int m0 = blockIdx.x * ADD_ROWS, m1 = m0 + min(ADD_ROWS, M - m0);
#pragma unroll 4
  for (int m = m0 + rl; m < m1; m += ADD_RL) {
    float u[4], v[4], o[4];
    quad_load(a + (int64_t)m * ld_a + c0, left, vec_a, u);
    quad_load(b + (int64_t)m * ld_b + c0, left, vec_b, v);
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = u[e] + v[e];
    quad_store(out + (int64_t)m * ld_out + c0, left, vec_out, o);
  }
}

static bool dwb_sizes_ok(int N, int H, int W, int C) {
  if (N <= 0 || H <= 0 || W <= 0 || C <= 0 || C > DWB_MAX_C) return false;
  const int64_t rows = (int64_t)N * H;      // (stepwise: no product of more than two ints before it is bounded)
  return rows < (1ll << 31) && rows * W < (1ll << 31) && rows * W * C < (1ll << 31);
}

}  // namespace xdet

using namespace xdet;

extern "C" {

size_t xdet_depthwise_backward_workspace_bytes(int N, int H, int W, int C) {
  if (!dwb_sizes_ok(N, H, W, C)) return 0;
  return ws_measure(4, dwb_layout, dwb_sums(N, H, W), C);
}

int xdet_depthwise_backward(const float* x, int ld_x, const float* k, const float* dy, int ld_dy, int N, int H, int W, int C,
                            int dilation, int relu_in, float* dx, int ld_dx, float* dw, void* workspace, void* stream) {
  XDET_REQUIRE(dwb_sizes_ok(N, H, W, C), "depthwise_backward: N, H, W and C positive, C at most 4096, N * H * W * C below 2^31");
  XDET_REQUIRE(dilation == 1 || dilation == 2, "depthwise_backward: the dilation is 1 or 2");
  XDET_REQUIRE(ld_x >= C && ld_dy >= C && (!dx || ld_dx >= C), "depthwise_backward: a pixel stride is below the channel count");
  const int64_t M = (int64_t)N * H * W;
  XDET_REQUIRE(M * std::max(std::max(ld_x, ld_dy), dx ? ld_dx : 0) < (1ll << 31),
               "depthwise_backward: N * H * W * the largest pixel stride must stay below 2^31");
  XDET_REQUIRE(x && k && dy && dw, "depthwise_backward: NULL argument");
  XDET_REQUIRE(workspace, "depthwise_backward: NULL workspace");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const DwbSums pl = dwb_sums(N, H, W);
  const DwbWorkspace ws = ws_carve(workspace, 4, dwb_layout, pl, C);

  DwbArgs a{};
  a.x = x; a.k = k; a.dy = dy; a.dx = dx; a.partial = ws.partial;
  a.ld_x = ld_x; a.ld_dy = ld_dy; a.ld_dx = ld_dx;
  a.H = H; a.W = W; a.C = C; a.M = (int)M; a.dil = dilation;
  a.pixels_per_chunk = pl.pixels_per_chunk;
  a.vec_x = quad_vec(x, ld_x); a.vec_dy = quad_vec(dy, ld_dy); a.vec_dx = quad_vec(dx, ld_dx);
  a.relu_in = relu_in != 0;
  const dim3 grid((unsigned)pl.n_chunks, (unsigned)cdiv(C, DWB_CB));
  if (C % 4 == 0 && a.vec_x && a.vec_dy && (!dx || a.vec_dx))
    hipLaunchKernelGGL(dwb_kernel<true>, grid, dim3(DWB_T), 0, s, a);
  else
    hipLaunchKernelGGL(dwb_kernel<false>, grid, dim3(DWB_T), 0, s, a);
  XDET_LAUNCH_CHECK();
  hipLaunchKernelGGL(dwb_fold_kernel, dim3((unsigned)cdiv(DWB_TAPS * C, DWB_FOLD_T)), dim3(DWB_FOLD_T), 0, s, ws.partial, pl.n_chunks, C,
                     dw);
  XDET_LAUNCH_CHECK();
  return XDET_OK;
}

int xdet_add_rows(const float* a, int ld_a, const float* b, int ld_b, float* out, int ld_out, int M, int C, void* stream) {
  XDET_REQUIRE(M > 0 && C > 0 && C <= ADD_MAX_C, "add_rows: M and C positive, C at most 2^24");
  XDET_REQUIRE(ld_a >= C && ld_b >= C && ld_out >= C, "add_rows: a row stride is below the channel count");
  XDET_REQUIRE((int64_t)M * std::max(std::max(ld_a, ld_b), ld_out) < (1ll << 31),
               "add_rows: M * the largest row stride must stay below 2^31");
  XDET_REQUIRE(a && b && out, "add_rows: NULL argument");
  hipLaunchKernelGGL(add_rows_kernel, dim3((unsigned)cdiv(M, ADD_ROWS), (unsigned)cdiv(C, DWB_CB)), dim3(ADD_T), 0,
                     reinterpret_cast<hipStream_t>(stream), a, ld_a, b, ld_b, out, ld_out, M, C, quad_vec(a, ld_a), quad_vec(b, ld_b),
                     quad_vec(out, ld_out));
  XDET_LAUNCH_CHECK();
  return XDET_OK;
}

}  // extern "C"
