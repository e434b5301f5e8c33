// Four consecutive channels of an NHWC row, the unit a lane of the row-streaming kernels owns (batchnorm.hip,
// depthwise_backward.hip): one float4 where the pointer and the row stride allow, four scalar accesses otherwise -- the same
// values in the same order either way, so alignment never changes a bit.  And the fold of their per-chunk sums.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace xdet {

// may rows of stride ld behind p be accessed as float4?  (a NULL p: no)
static inline int quad_vec(const void* p, int ld) { return p && (reinterpret_cast<uintptr_t>(p) & 15) == 0 && ld % 4 == 0; }

// four consecutive floats at p, of which `left` exist (the others read as 0 and are never fetched)
__device__ __forceinline__ void quad_load(const float* __restrict__ p, int left, bool vec, float (&v)[4]) {
  if (vec && left >= 4) {
    const float4 t = *reinterpret_cast<const float4*>(p);
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = e < left ? p[e] : 0.f;
  }
}
__device__ __forceinline__ void quad_store(float* __restrict__ p, int left, bool vec, const float (&v)[4]) {
  if (vec && left >= 4) {
    *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (e < left) p[e] = v[e];
  }
}

// chunk sums partial[chunk][stride] of one column added in index order; 32 loads are in flight before the first add (one
// load per add was a dependent round trip per chunk: 113 of them at the large-separable block's size, most of a call's time)
__device__ __forceinline__ float fold_chunks(const float* __restrict__ partial, int n_chunks, int stride, int col) {
  float s = 0.f;
  for (int k = 0; k < n_chunks; k += 32) {
    float v[32];
#pragma unroll
    for (int i = 0; i < 32; ++i) v[i] = partial[(int64_t)min(k + i, n_chunks - 1) * stride + col];
#pragma unroll
    for (int i = 0; i < 32; ++i)
      if (k + i < n_chunks) s += v[i];
  }
  return s;
}

}  // namespace xdet
