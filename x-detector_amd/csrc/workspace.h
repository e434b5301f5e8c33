// One walk both sizes and carves a caller-owned workspace: a layout function takes its members from a WsWalk in order;
// over a NULL base the walk only measures (bytes() is what the caller allocates), over the caller's block it hands out
// the pointers.  The size entry point and the carve of a workspace call the SAME layout function, so they cannot disagree.
// (No HIP header: a plain host compiler builds this file, tests/test_workspace_layout.py.)
#pragma once
#include <cstddef>

namespace xdet {

class WsWalk {
  unsigned char* base_;
  size_t align_, off_ = 0;

 public:
  explicit WsWalk(void* base, size_t align = 256) : base_(static_cast<unsigned char*>(base)), align_(align) {}
  // `count` elements of T (0: an empty part), the part rounded up to the alignment; NULL while measuring
  template <class T>
  T* take(size_t count) {
    unsigned char* p = base_ ? base_ + off_ : nullptr;
    off_ += (count * sizeof(T) + align_ - 1) / align_ * align_;
    return reinterpret_cast<T*>(p);
  }
  size_t bytes() const { return off_; }
};

// the bytes that layout(walk, args...) takes: what the caller of that workspace allocates
template <class Layout, class... Args>
size_t ws_measure(size_t align, Layout layout, Args... args) {
  WsWalk w(nullptr, align);
  layout(w, args...);
  return w.bytes();
}
// ... and what it hands out over the caller's block
template <class Layout, class... Args>
auto ws_carve(void* base, size_t align, Layout layout, Args... args) {
  WsWalk w(base, align);
  return layout(w, args...);
}

}  // namespace xdet
