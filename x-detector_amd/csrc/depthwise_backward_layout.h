// How the per-channel tap sums of the depthwise backward (depthwise_backward.hip) are cut, and the workspace that holds their
// partial sums: one layout function for the size entry point and the carve.  (No HIP header: a plain host compiler builds
// this file, tests/test_depthwise_backward_math.py.)
#pragma once
#include "workspace.h"
#include <cstdint>

namespace xdet {

constexpr int DWB_MAX_C = 4096;
constexpr int DWB_MAX_CHUNKS = 1024;    // pixel chunks of a tap sum
constexpr int DWB_TAPS = 9;

// everything that shapes a sum depends on (N, H, W) alone: chunks of max(64, ceil(M / 1024)) pixels of the flat pixel index
// m = (n H + h) W + w, M = N H W -- bn_sums' rule (batchnorm_layout.h)
struct DwbSums {
  int pixels_per_chunk, n_chunks;
};
static inline DwbSums dwb_sums(int N, int H, int W) {
  DwbSums p;
  const int64_t M = (int64_t)N * H * W;
  const int64_t per = (M + DWB_MAX_CHUNKS - 1) / DWB_MAX_CHUNKS;
  p.pixels_per_chunk = (int)(per < 64 ? 64 : per);
  p.n_chunks = (int)((M + p.pixels_per_chunk - 1) / p.pixels_per_chunk);
  return p;
}

struct DwbWorkspace {
  float* partial;     // [n_chunks][9][C] chunk sums of xe * shifted g, taps in storage order
};
// whole words, packed (walk it with an alignment of 4 bytes)
static inline DwbWorkspace dwb_layout(WsWalk& w, const DwbSums& p, int C) {
  return {w.take<float>((size_t)p.n_chunks * DWB_TAPS * C)};
}

}  // namespace xdet
