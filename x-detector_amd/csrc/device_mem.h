// Device RAII.  DevMem<T>: the owner of one hipMalloc block -- null by default, move-only, freed by its destructor; it
// converts to T*, so launch sites read an owned array like the raw pointer it replaces.  DeviceGuard: a HIP device made
// current for a scope.
#pragma once
#include "common.h"

#include <algorithm>
#include <utility>

namespace xdet {

template <class T>
class DevMem {
  T* p_ = nullptr;

 public:
  DevMem() = default;
  DevMem(DevMem&& o) noexcept : p_(std::exchange(o.p_, nullptr)) {}   // (a declared move: the copies are deleted)
  DevMem& operator=(DevMem&& o) noexcept { std::swap(p_, o.p_); return *this; }
  ~DevMem() { reset(); }
  void reset() { if (p_) (void)hipFree(p_); p_ = nullptr; }
  T* get() const { return p_; }
  operator T*() const { return p_; }
  // `count` elements in a block of at least min_bytes; what was held is freed first (hipFree waits for the device)
  int alloc(size_t count, size_t min_bytes = 16) {
    reset();
    void* q = nullptr;
    XDET_HIP(hipMalloc(&q, std::max(count * sizeof(T), min_bytes)));
    p_ = static_cast<T*>(q);
    return XDET_OK;
  }
  int alloc_zeroed(size_t count, size_t min_bytes = 16) {   // the whole block is cleared
    XDET_TRY(alloc(count, min_bytes));
    XDET_HIP(hipMemset(p_, 0, std::max(count * sizeof(T), min_bytes)));
    return XDET_OK;
  }
  int upload(const T* host, size_t count) {
    XDET_TRY(alloc(count));
    XDET_HIP(hipMemcpy(p_, host, count * sizeof(T), hipMemcpyHostToDevice));
    return XDET_OK;
  }
};

// Layers, nets and communicators live on the device that was current when they were created; every entry point that
// launches on their behalf makes that device current for the call (and restores the caller's), so two detectors on two
// GPUs can share one process / one host thread per device.
struct DeviceGuard {
  int prev = -1, want = -1;
  explicit DeviceGuard(int dev) : want(dev) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    if (prev != want) (void)hipSetDevice(want);
  }
  ~DeviceGuard() {
    if (prev >= 0 && prev != want) (void)hipSetDevice(prev);
  }
};

}  // namespace xdet
