// Stand-alone check of csrc/workspace.h (built and run by tests/test_workspace_layout.py under ASan + UBSan).
// For every member list and alignment: the measuring walk (NULL base) and the carving walk end at the same offset, every
// pointer is aligned, members are in order and disjoint, the last one ends inside bytes(), and the measuring walk hands
// out NULL only.  Every member is then written in full inside a heap block of exactly bytes() bytes.
#include "workspace.h"

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

struct alignas(16) Vec4 { float v[4]; };
struct Member { size_t elem, count; };

static void* take(xdet::WsWalk& w, const Member& m) {
  switch (m.elem) {
    case 1: return w.take<unsigned char>(m.count);
    case 4: return w.take<int>(m.count);
    case 8: return w.take<unsigned long long>(m.count);
    default: return w.take<Vec4>(m.count);
  }
}

static int check(const char* name, const std::vector<Member>& list, size_t align) {
  xdet::WsWalk measure(nullptr, align);
  for (const Member& m : list)
    if (take(measure, m) != nullptr) { printf("%s: a measuring walk returned a pointer\n", name); return 1; }
  const size_t bytes = measure.bytes();
  unsigned char* base = static_cast<unsigned char*>(aligned_alloc(256, (bytes + 255) / 256 * 256 + 256));
  xdet::WsWalk carve(base, align);             // the members must fit [base, base + bytes)
  unsigned char* prev_end = base;
  int bad = 0;
  for (size_t i = 0; i < list.size(); ++i) {
    unsigned char* p = static_cast<unsigned char*>(take(carve, list[i]));
    const size_t len = list[i].elem * list[i].count;
    if (reinterpret_cast<uintptr_t>(p) % align != 0) { printf("%s: member %zu is not aligned to %zu\n", name, i, align); bad = 1; }
    if (p < prev_end) { printf("%s: member %zu overlaps its predecessor\n", name, i); bad = 1; }
    if (p + len > base + bytes) { printf("%s: member %zu ends past bytes()\n", name, i); bad = 1; }
    if (!bad) memset(p, 0x5a, len);
    prev_end = p + len;
  }
  if (carve.bytes() != bytes) { printf("%s: measured %zu bytes, carved %zu\n", name, bytes, carve.bytes()); bad = 1; }
  if (bytes % align != 0) { printf("%s: bytes() is not a multiple of the alignment\n", name); bad = 1; }
  free(base);
  // the same members in a block of exactly bytes() bytes: ASan faults on a write past it
  if (!bad && bytes) {
    unsigned char* tight = static_cast<unsigned char*>(malloc(bytes));
    xdet::WsWalk w(tight, align);
    for (const Member& m : list) {
      void* p = take(w, m);
      memset(p, 0, m.elem * m.count);
    }
    free(tight);
  }
  return bad;
}

int main() {
  int bad = 0, n = 0;
  // packed words, as the dense-layer backward's workspace
  const std::vector<Member> words = {{4, 16}, {4, 3 * 25}, {4, 0}, {1, 8}, {4, 1}};
  // records and 64-bit sums, as the training ingest's
  const std::vector<Member> recs = {{8, 16 * 5}, {8, 4 * 5}, {1, 3}, {4, 7}, {8, 0}, {8, 1}};
  // everything mixed, with empty parts in front, inside and at the end
  const std::vector<Member> mixed = {{1, 0}, {4, 7}, {16, 3}, {8, 5}, {1, 257}, {4, 0}, {16, 1}, {8, 33}, {1, 1}, {16, 0}};
  const std::vector<Member> one = {{16, 1}};
  const std::vector<Member> none = {};
  bad |= check("words/4", words, 4); ++n;
  bad |= check("recs/8", recs, 8); ++n;
  bad |= check("words/256", words, 256); ++n;
  bad |= check("recs/256", recs, 256); ++n;
  bad |= check("mixed/256", mixed, 256); ++n;
  bad |= check("one/256", one, 256); ++n;
  bad |= check("none/256", none, 256); ++n;
  if (!bad) printf("ok: %d member lists\n", n);
  return bad;
}
