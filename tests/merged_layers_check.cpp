// Stand-alone check of csrc/merged_layers.h (built and run by tests/test_merged_layers.py under ASan + UBSan).
// Per group, at small sizes (head 21|4 at K = 7, RPN 44|88 at hid = 5, large-separable cin 3, mid 2, co 5): the parts are
// filled with distinct values and merged_concat must put merged[o][off_p + j] = part_p[o][j] for every element, into an array
// of exactly count() floats; a group's slots cover each merged tensor exactly once and name no role twice; the role names are
// the checkpoint's.  The two refresh doors' scratch layouts are walked as well: measure == carve, members aligned, in order,
// disjoint, and written in full inside a block of exactly the measured bytes.
#include "merged_layers.h"

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <set>

using namespace xdet;

static int bad = 0;
#define EXPECT(cond, ...) do { if (!(cond)) { printf(__VA_ARGS__); printf("\n"); bad = 1; } } while (0)

// the element count of every conv / dense role of a group, stated here on its own
static std::vector<size_t> role_counts(int g, const MergedSizes& z) {
  const size_t A = z.A, nc = z.nc, hid = z.hid, fcw = z.fcw, cin = z.cin, mid = z.mid, co = z.co;
  if (g == MG_RPN) return {9 * 728 * hid, hid, hid * 2 * A, 2 * A, hid * 4 * A, 4 * A};
  if (g == MG_HEAD) return {co * fcw, fcw, fcw * nc, nc, fcw * 4, 4};
  return {15 * cin * mid, mid, 15 * mid * co, co, 15 * cin * mid, mid, 15 * mid * co, co};
}

static void check_group(int g, const MergedSizes& z, size_t n_slots, const std::vector<std::string>& want_names) {
  const char* name = merged_group_name(g);
  const std::vector<std::string> names = merged_roles(g);
  EXPECT(names == want_names, "%s: the role names are not the checkpoint's", name);
  const std::vector<size_t> counts = role_counts(g, z);
  // every role an exactly sized heap array of distinct values (ASan faults on a read past a part)
  std::vector<float*> parts;
  float next = 1.f;
  for (size_t c : counts) {
    float* p = static_cast<float*>(malloc(c * sizeof(float)));
    for (size_t i = 0; i < c; ++i) p[i] = next++;
    parts.push_back(p);
  }
  const std::vector<MergedSlot> slots = merged_slots(g, z);
  EXPECT(slots.size() == n_slots, "%s: %zu slots, expected %zu", name, slots.size(), n_slots);
  std::set<int> roles;
  for (size_t si = 0; si < slots.size(); ++si) {
    const MergedSlot& s = slots[si];
    EXPECT(s.outer > 0 && s.width[0] > 0 && s.width[1] > 0, "%s slot %zu: outer and widths must be positive", name, si);
    std::vector<int> cover(s.W(), 0);
    size_t off = 0;
    for (int p = 0; p < 2; ++p) {
      EXPECT(s.role[p] >= 0 && (size_t)s.role[p] < counts.size(), "%s slot %zu: part %d is no conv / dense role", name, si, p);
      EXPECT(roles.insert(s.role[p]).second, "%s slot %zu: role %d is a part twice", name, si, s.role[p]);
      EXPECT(counts[(size_t)s.role[p]] == (size_t)s.outer * s.width[p], "%s slot %zu: part %d is not [outer, width]", name, si, p);
      for (int j = 0; j < s.width[p]; ++j) ++cover[off + (size_t)j];
      off += (size_t)s.width[p];
    }
    for (size_t c = 0; c < cover.size(); ++c) EXPECT(cover[c] == 1, "%s slot %zu: column %zu is covered %d times", name, si, c, cover[c]);
    if (bad) break;
    float* merged = static_cast<float*>(malloc(s.count() * sizeof(float)));
    for (size_t i = 0; i < s.count(); ++i) merged[i] = -1.f;
    merged_concat(s, parts.data(), merged);
    off = 0;
    for (int p = 0; p < 2; ++p) {
      for (int o = 0; o < s.outer; ++o)
        for (int j = 0; j < s.width[p]; ++j)
          if (merged[(size_t)o * s.W() + off + (size_t)j] != parts[(size_t)s.role[p]][(size_t)o * s.width[p] + j]) {
            EXPECT(false, "%s slot %zu: merged[%d][%zu + %d] is not part %d's [%d][%d]", name, si, o, off, j, p, o, j);
            o = s.outer;
            break;
          }
      off += (size_t)s.width[p];
    }
    const std::vector<float> again = merged_concat(s, parts.data());
    EXPECT(again.size() == s.count() && memcmp(again.data(), merged, s.count() * sizeof(float)) == 0,
           "%s slot %zu: the two forms of merged_concat differ", name, si);
    free(merged);
  }
  for (float* p : parts) free(p);
}

// measure == carve; the members (pointer, bytes) aligned, in order, disjoint and inside the block; each written in full
template <class Layout, class Members, class... Args>
static void check_walk(const char* name, Layout layout, Members members, Args... args) {
  const size_t bytes = ws_measure(256, layout, args...);
  EXPECT(bytes > 0 && bytes % 256 == 0, "%s: measured %zu bytes", name, bytes);
  for (const auto& m : members(ws_carve(nullptr, 256, layout, args...)))
    EXPECT(m.first == nullptr, "%s: a measuring walk returned a pointer", name);
  unsigned char* base = static_cast<unsigned char*>(aligned_alloc(256, bytes));
  WsWalk w(base, 256);
  const auto carved = layout(w, args...);
  EXPECT(w.bytes() == bytes, "%s: measured %zu bytes, carved %zu", name, bytes, w.bytes());
  unsigned char* prev_end = base;
  size_t i = 0;
  for (const auto& m : members(carved)) {
    unsigned char* p = static_cast<unsigned char*>(m.first);
    EXPECT(reinterpret_cast<uintptr_t>(p) % 256 == 0, "%s: member %zu is not aligned", name, i);
    EXPECT(p >= prev_end, "%s: member %zu overlaps its predecessor", name, i);
    EXPECT(p + m.second <= base + bytes, "%s: member %zu ends past the measured bytes", name, i);
    if (!bad) memset(p, 0x5a, m.second);
    prev_end = p + m.second;
    ++i;
  }
  free(base);
}

typedef std::vector<std::pair<void*, size_t>> Members;

int main() {
  // head 21|4 at K = 7, RPN 44|88 (A = 22) at hid = 5, large-separable cin 3, mid 2, co 5
  const MergedSizes z = {22, 21, 5, 7, 3, 2, 5};
  const std::string b0 = "large_sep_feature/Branch_0/", b1 = "large_sep_feature/Branch_1/", bn = "large_sep_feature/batch_normalization/";
  check_group(MG_RPN, z, 2, {"rpn_head/conv2d/kernel", "rpn_head/conv2d/bias", "rpn_head/conv2d_1/kernel", "rpn_head/conv2d_1/bias",
                             "rpn_head/conv2d_2/kernel", "rpn_head/conv2d_2/bias"});
  check_group(MG_HEAD, z, 2, {"final_head/subnet_fc/kernel", "final_head/subnet_fc/bias", "final_head/fc_cls/kernel", "final_head/fc_cls/bias",
                              "final_head/fc_loc/kernel", "final_head/fc_loc/bias"});
  check_group(MG_LSEP, z, 3, {b0 + "conv2d/kernel", b0 + "conv2d/bias", b0 + "conv2d_1/kernel", b0 + "conv2d_1/bias", b1 + "conv2d/kernel",
                              b1 + "conv2d/bias", b1 + "conv2d_1/kernel", b1 + "conv2d_1/bias", bn + "gamma", bn + "beta", bn + "moving_mean",
                              bn + "moving_variance"});
  // the widths themselves, once: what the three merges are
  const std::vector<MergedSlot> rpn = merged_slots(MG_RPN, z), head = merged_slots(MG_HEAD, z), lsep = merged_slots(MG_LSEP, z);
  EXPECT(rpn[SLOT_K].outer == 5 && rpn[SLOT_K].width[0] == 44 && rpn[SLOT_K].width[1] == 88 && rpn[SLOT_B].outer == 1, "rpn_head: 44|88 at hid 5");
  EXPECT(head[SLOT_K].outer == 7 && head[SLOT_K].width[0] == 21 && head[SLOT_K].width[1] == 4 && head[SLOT_B].outer == 1, "final_head: 21|4 at K 7");
  EXPECT(lsep[SLOT_KA].outer == 45 && lsep[SLOT_KA].W() == 4 && lsep[SLOT_BA].count() == 4 && lsep[SLOT_KB].outer == 15 &&
         lsep[SLOT_KB].W() == 20, "large_sep_feature: K_a [45, 2|2], b_a [1, 2|2], K_b [15, 10|10]");
  // the block's bias sum and batch norm roles are the names they say
  const std::vector<std::string> ln = merged_roles(MG_LSEP);
  EXPECT(ln[LSEP_B0] == b0 + "conv2d_1/bias" && ln[LSEP_B1] == b1 + "conv2d_1/bias" && ln[LSEP_GAMMA] == bn + "gamma" &&
         ln[LSEP_BETA] == bn + "beta" && ln[LSEP_MEAN] == bn + "moving_mean" && ln[LSEP_VAR] == bn + "moving_variance", "the block's roles");

  check_walk("body_refresh", body_refresh_layout,
             [](const BodyRefreshScratch& s) { return Members{{s.ws, 1000}, {s.scale, 4 * 333}, {s.shift, 4 * 333}}; }, (size_t)1000, (size_t)333);
  check_walk("heads_refresh", heads_refresh_layout, [&](const HeadsRefreshScratch& s) {
    return Members{{s.pack_ws, 77}, {s.repack_ws, 4097}, {s.rpn[0], 4 * 5 * 132}, {s.rpn[1], 4 * 132}, {s.head[0], 4 * 7 * 25},
                   {s.head[1], 4 * 25}, {s.b_a, 4 * 4}, {s.b_sum, 4 * 5}, {s.scale, 4 * 5}, {s.shift, 4 * 5}};
  }, (size_t)77, (size_t)4097, z);
  check_walk("large_sep_kernels", large_sep_kernel_layout,
             [](const LargeSepKernelScratch& s) { return Members{{s.k_a, 4 * 45 * 4}, {s.k_b, 4 * 15 * 20}}; }, z);
  if (!bad) printf("ok: 3 groups, 7 slots, 3 scratch layouts\n");
  return bad;
}
