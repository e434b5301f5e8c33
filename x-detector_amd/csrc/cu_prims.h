// The CU-level toolkit of the MFMA kernels: register vector types, LDS accessors that may run next to an in-flight
// LDS-DMA, compile-time loops, the f32 -> f16 hi / lo split and the NaN-keeping ReLU.  Device-side helpers only: no
// kernels, no launch code.  A form lives here when at least two kernel files use it unchanged; a variant that differs
// on purpose (sf_relu, sf_split4 / rs_split4: sepconv_fused.hip, resnet_stem.hip) stays in its file under its own name.
// conv_mfma_dma.hip and conv_epilogue.h still carry private copies (f32x16 / f16x8 / u16, cd_ds_read_b128, ep_relu): the
// committed counter profile is pinned to their text, so the dominant kernel adopts this header with its next profiled change.
#pragma once
#include <hip/hip_runtime.h>

namespace xdet {

typedef float f32x16 __attribute__((ext_vector_type(16)));    // one 32x32 MFMA accumulator block of a lane
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));   // a lane's operand of the 32x32x16 f16 MFMA
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned short u16;                                   // f16 bits in memory (planes, weights, LDS tiles)

__device__ __forceinline__ unsigned lds_addr(const void* p) {
  return (unsigned)(size_t)(__attribute__((address_space(3))) void*)(p);
}

// LDS accesses issued while an LDS-writing DMA (global_load_lds / buffer_load ... lds) is in flight.  The compiler cannot
// tell that they never alias the DMA's target and would drain s_waitcnt vmcnt(0) in front of every one of them, stalling
// on the prefetch each step -- so they are inline asm, which it does not track at all.  The caller therefore owes every
// wait itself: `s_waitcnt lgkmcnt(n)` (the LDS returns a wave's accesses in order) before a read's result is used or a
// written location is read back / handed over at a barrier, and an empty `asm volatile("" : "+v"(r))` after the wait to
// keep the consumers behind it; and `s_waitcnt vmcnt(n)` before reading what the DMA wrote.
// addr is a byte address (lds_addr), OFF the instruction's immediate byte offset.
template <int OFF>
__device__ __forceinline__ f16x8 ds_read_h8(unsigned addr) {
  f16x8 r;
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(r) : "v"(addr), "n"(OFF) : "memory");
  return r;
}
template <int OFF>
__device__ __forceinline__ f32x4 ds_read_f4(unsigned addr) {
  f32x4 r;
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(r) : "v"(addr), "n"(OFF) : "memory");
  return r;
}
template <int OFF, typename T>    // T: u32x2 or uint2
__device__ __forceinline__ void ds_write_b64(unsigned addr, T v) {
  static_assert(sizeof(T) == 8, "ds_write_b64 writes eight bytes");
  asm volatile("ds_write_b64 %0, %1 offset:%2" ::"v"(addr), "v"(v), "n"(OFF) : "memory");
}

// static_for<N>([&](auto I) { constexpr int i = decltype(I)::value; ... }): a loop whose index is a constant expression
// (asm immediates, template arguments)
template <int V>
struct int_c { static constexpr int value = V; };
template <int N, typename F, int I = 0>
__device__ __forceinline__ void static_for(F&& f) {
  if constexpr (I < N) {
    f(int_c<I>{});
    static_for<N, F, I + 1>(static_cast<F&&>(f));
  }
}

// hi = f16(v), lo = f16(v - float(hi)) of four values: the planes copy a conv epilogue writes (conv_epilogue.h), so
// every producer of split planes gives the same bits
__device__ __forceinline__ void split4(const float (&t)[4], u32x2* h, u32x2* l) {
  const _Float16 h0 = (_Float16)t[0], h1 = (_Float16)t[1], h2 = (_Float16)t[2], h3 = (_Float16)t[3];
  const f16x4 hv = {h0, h1, h2, h3};
  const f16x4 lv = {(_Float16)(t[0] - (float)h0), (_Float16)(t[1] - (float)h1), (_Float16)(t[2] - (float)h2),
                    (_Float16)(t[3] - (float)h3)};
  *h = __builtin_bit_cast(u32x2, hv);
  *l = __builtin_bit_cast(u32x2, lv);
}
__device__ __forceinline__ void split4(const float4 v, uint2* hi, uint2* lo) {
  const _Float16 h0 = (_Float16)v.x, h1 = (_Float16)v.y, h2 = (_Float16)v.z, h3 = (_Float16)v.w;
  f16x4 hv = {h0, h1, h2, h3};
  f16x4 lv = {(_Float16)(v.x - (float)h0), (_Float16)(v.y - (float)h1), (_Float16)(v.z - (float)h2),
              (_Float16)(v.w - (float)h3)};
  *hi = *reinterpret_cast<uint2*>(&hv);
  *lo = *reinterpret_cast<uint2*>(&lv);
}

// ReLU that keeps NaN (fmaxf(NaN, 0) is 0); conv_epilogue.h ep_relu is the same expression
__device__ __forceinline__ float relu_keep_nan(float v) { return __builtin_elementwise_maximum(v, 0.f); }

}  // namespace xdet
