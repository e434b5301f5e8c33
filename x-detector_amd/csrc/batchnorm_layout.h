// How the per-channel sums of batch norm (batchnorm.hip) are cut, and the workspace that holds their partial sums: one
// layout function for the size entry point and the carve.  (No HIP header: a plain host compiler builds this file,
// tests/test_batch_norm_math.py.)
#pragma once
#include "workspace.h"
#include <cstdint>

namespace xdet {

constexpr int BN_MAX_C = 4096;
constexpr int BN_MAX_CHUNKS = 1024;     // row chunks of a per-channel sum

// everything that shapes a sum depends on M alone: db_sums' rule (backward_gemm.h)
struct BnSums {
  int rows_per_chunk, n_chunks;
};
static inline BnSums bn_sums(int M) {
  BnSums p;
  const int64_t per = ((int64_t)M + BN_MAX_CHUNKS - 1) / BN_MAX_CHUNKS;
  p.rows_per_chunk = (int)(per < 64 ? 64 : per);
  p.n_chunks = (int)(((int64_t)M + p.rows_per_chunk - 1) / p.rows_per_chunk);
  return p;
}

struct BnWorkspace {
  float* first;       // [n_chunks][C] chunk sums: of x (forward), of g (backward)
  float* second;      // [n_chunks][C] chunk sums: of (x - mean)^2 (forward), of g * xhat (backward)
};
// whole words, packed (walk it with an alignment of 4 bytes)
static inline BnWorkspace bn_layout(WsWalk& w, const BnSums& p, int C) {
  return {w.take<float>((size_t)p.n_chunks * C), w.take<float>((size_t)p.n_chunks * C)};
}

}  // namespace xdet
