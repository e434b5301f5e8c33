// The defined shuffle of the training code (include/xdet.h "training targets"): shuffle(S) = S ordered by (key, element),
// key = mix(mix(mix(seed ^ 0x9E3779B9) + image) ^ (2 * element + stream)), integers only -- the same on the host
// (xdet/targets.py shuffle_keys).  mix is a bijection of the 32-bit words, so for one (seed, image, stream) the keys of
// different elements differ, and the element follows from its key (tg_unmix): a sort may carry the keys alone.
#pragma once
#include <hip/hip_runtime.h>

namespace xdet {

__host__ __device__ __forceinline__ unsigned tg_mix(unsigned x) {
  x ^= x >> 16;
  x *= 0x7FEB352Du;
  x ^= x >> 15;
  x *= 0x846CA68Bu;
  x ^= x >> 16;
  return x;
}

// a^-1 mod 2^32 of an odd a (Newton: a is its own inverse to 3 bits, every step doubles them)
constexpr unsigned tg_inverse32(unsigned a) {
  unsigned x = a;
  for (int i = 0; i < 4; ++i) x *= 2u - a * x;
  return x;
}
static_assert(0x7FEB352Du * tg_inverse32(0x7FEB352Du) == 1u && 0x846CA68Bu * tg_inverse32(0x846CA68Bu) == 1u, "tg_inverse32");

// tg_unmix(tg_mix(x)) == x
__host__ __device__ __forceinline__ unsigned tg_unmix(unsigned x) {
  x ^= x >> 16;
  x *= tg_inverse32(0x846CA68Bu);
  x ^= (x >> 15) ^ (x >> 30);
  x *= tg_inverse32(0x7FEB352Du);
  x ^= x >> 16;
  return x;
}

// ascending bitonic sort of P (a power of two) distinct 64-bit words (keys carrying their elements) in LDS, by all THREADS
// threads of the workgroup; ends with a barrier
template <int THREADS>
__device__ void lds_bitonic_sort_u64(unsigned long long* s, int P) {
  for (int k = 2; k <= P; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = threadIdx.x; i < P; i += THREADS) {
        const int p = i ^ j;
        if (p > i) {
          const unsigned long long x = s[i], y = s[p];
          if ((x > y) == ((i & k) == 0)) { s[i] = y; s[p] = x; }
        }
      }
      __syncthreads();
    }
}

}  // namespace xdet
