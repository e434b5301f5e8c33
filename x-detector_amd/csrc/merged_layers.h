// THE statement of the merged layers: how the checkpoint's tensors sit inside the tensors the plan's layers use.  Three groups
// (net/xception_body.py:381-400, 450-475, 536-557): the RPN head's conv2d_1 | conv2d_2, the head's fc_cls | fc_loc, and the
// large-separable block's Branch_0 | Branch_1.  A group is its tensors' names in role order and its slots; a slot is one merged
// tensor [outer, W] with two parts [outer, width_p] side by side, merged[o, off_p + c] = part_p[o, c] -- the words of
// xdet_pack_slot (include/xdet.h).  The builders merge host arrays by merged_concat, xdet_net_refresh_heads turns the same
// slots into its xdet_tensors_concat table, and its scratch holds one array per slot.  xdet/train.py's merged_layout is the
// same table in Python.  (No HIP header: a plain host compiler builds this file, tests/test_merged_layers.py.)
#pragma once
#include "workspace.h"

#include <cstring>
#include <string>
#include <vector>

namespace xdet {

enum { MG_RPN, MG_HEAD, MG_LSEP, MG_N };

// A: anchors, nc: classes; hid / fcw: the width of rpn_head/conv2d and of final_head/subnet_fc; cin, mid, co: the
// large-separable block's input, per-branch middle and output channels
struct MergedSizes { int A, nc, hid, fcw, cin, mid, co; };

struct MergedSlot {
  int outer;
  int role[2], width[2];                       // always two parts: a pair of layers, or of branches
  size_t W() const { return (size_t)width[0] + (size_t)width[1]; }
  size_t count() const { return (size_t)outer * W(); }
};

inline const char* merged_group_name(int g) { return g == MG_RPN ? "rpn_head" : g == MG_HEAD ? "final_head" : "large_sep_feature"; }

// the large-separable block's roles beside its slots: b_b = b0 + b1 (the one relation that is no concatenation), folded into
// the batch norm behind the (1,15) conv
enum { LSEP_B0 = 3, LSEP_B1 = 7, LSEP_GAMMA = 8, LSEP_BETA, LSEP_MEAN, LSEP_VAR };
// ... and the heads': the layer in front of the merged pair
enum { HEAD_K0 = 0, HEAD_B0 = 1 };

// a group's tensors under the checkpoint's names, in role order: kernel, bias per layer (per branch); then the block's batch norm
inline std::vector<std::string> merged_roles(int g) {
  std::vector<std::string> names;
  const std::string pre = std::string(merged_group_name(g)) + "/";
  auto layers = [&](const std::string& p, std::initializer_list<const char*> ls) {
    for (const char* l : ls)
      for (const char* v : {"/kernel", "/bias"}) names.push_back(p + l + v);
  };
  if (g == MG_RPN) layers(pre, {"conv2d", "conv2d_1", "conv2d_2"});
  else if (g == MG_HEAD) layers(pre, {"subnet_fc", "fc_cls", "fc_loc"});
  else {
    for (const char* br : {"Branch_0/", "Branch_1/"}) layers(pre + br, {"conv2d", "conv2d_1"});
    for (const char* v : {"gamma", "beta", "moving_mean", "moving_variance"}) names.push_back(pre + "batch_normalization/" + v);
  }
  return names;
}

// a group's merged tensors.  Heads: {kernel, bias} of the two layers side by side; block: {K_a, b_a, K_b} -- both (15,1)
// kernels [15, 1, cin, mid] along the outputs, their biases, and both (1,15) kernels [1, 15, mid, co] stacked along the inputs
inline std::vector<MergedSlot> merged_slots(int g, const MergedSizes& z) {
  if (g == MG_RPN) return {{z.hid, {2, 4}, {2 * z.A, 4 * z.A}}, {1, {3, 5}, {2 * z.A, 4 * z.A}}};
  if (g == MG_HEAD) return {{z.fcw, {2, 4}, {z.nc, 4}}, {1, {3, 5}, {z.nc, 4}}};
  return {{15 * z.cin, {0, 4}, {z.mid, z.mid}}, {1, {1, 5}, {z.mid, z.mid}}, {15, {2, 6}, {z.mid * z.co, z.mid * z.co}}};
}
enum { SLOT_K = 0, SLOT_B = 1, SLOT_KA = 0, SLOT_BA = 1, SLOT_KB = 2 };

// the host merge: merged (count() floats) from the group's host arrays by role
inline void merged_concat(const MergedSlot& s, const float* const* by_role, float* merged) {
  const size_t W = s.W();
  for (int o = 0; o < s.outer; ++o) {
    size_t off = 0;
    for (int p = 0; p < 2; ++p) {
      memcpy(merged + (size_t)o * W + off, by_role[s.role[p]] + (size_t)o * s.width[p], (size_t)s.width[p] * sizeof(float));
      off += (size_t)s.width[p];
    }
  }
}
inline std::vector<float> merged_concat(const MergedSlot& s, const float* const* by_role) {
  std::vector<float> m(s.count());
  merged_concat(s, by_role, m.data());
  return m;
}

// ---- the scratch of the two refresh doors (lighthead.hip), each one block described by one walk ----

// xdet_net_refresh_weights: [the table door's workspace | the folds' scales | shifts], a record's channels at its own offset
struct BodyRefreshScratch {
  void* ws = nullptr;
  float *scale = nullptr, *shift = nullptr;
};
inline BodyRefreshScratch body_refresh_layout(WsWalk& w, size_t ws_bytes, size_t channels) {
  BodyRefreshScratch s;
  s.ws = w.take<unsigned char>(ws_bytes);
  s.scale = w.take<float>(channels);
  s.shift = w.take<float>(channels);
  return s;
}

// xdet_net_refresh_heads: [pack workspace | repack workspace | the heads' merged kernels and biases | b_a, b0 + b1, scale, shift]
struct HeadsRefreshScratch {
  void *pack_ws = nullptr, *repack_ws = nullptr;
  float *rpn[2] = {nullptr, nullptr}, *head[2] = {nullptr, nullptr};
  float *b_a = nullptr, *b_sum = nullptr, *scale = nullptr, *shift = nullptr;
};
inline HeadsRefreshScratch heads_refresh_layout(WsWalk& w, size_t pack_bytes, size_t repack_bytes, MergedSizes z) {
  HeadsRefreshScratch s;
  s.pack_ws = w.take<unsigned char>(pack_bytes);
  s.repack_ws = w.take<unsigned char>(repack_bytes);
  const std::vector<MergedSlot> rpn = merged_slots(MG_RPN, z), head = merged_slots(MG_HEAD, z);
  for (int i = 0; i < 2; ++i) s.rpn[i] = w.take<float>(rpn[i].count());
  for (int i = 0; i < 2; ++i) s.head[i] = w.take<float>(head[i].count());
  s.b_a = w.take<float>(merged_slots(MG_LSEP, z)[SLOT_BA].count());
  s.b_sum = w.take<float>(z.co);
  s.scale = w.take<float>(z.co);
  s.shift = w.take<float>(z.co);
  return s;
}
// ... and the large-separable block's two merged kernels, a block of their own at the first call that names the group
struct LargeSepKernelScratch {
  float *k_a = nullptr, *k_b = nullptr;
};
inline LargeSepKernelScratch large_sep_kernel_layout(WsWalk& w, MergedSizes z) {
  const std::vector<MergedSlot> slots = merged_slots(MG_LSEP, z);
  LargeSepKernelScratch s;
  s.k_a = w.take<float>(slots[SLOT_KA].count());
  s.k_b = w.take<float>(slots[SLOT_KB].count());
  return s;
}

}  // namespace xdet
