#pragma once
// The gradient average of data-parallel training, as csrc/comm.hip calls it (grad_average.hip holds the kernels and the two
// device-only doors; include/xdet.h states the flat element space and the per-element statement).
#include "common.h"

#include <algorithm>

namespace xdet {

struct GradSlotDev;

struct GradPlan {                      // a validated table, uploaded into a workspace
  const GradSlotDev* d_slots = nullptr;
  const int* d_runs = nullptr;         // [n_chunks * runs_per_chunk + 1]: the slot that holds each run's first flat element
  int64_t total = 0;                   // T, the flat element count
  int64_t chunk_elems = 0, n_chunks = 0;
  int runs_per_chunk = 0;
  float* flat = nullptr;               // world > 1: one packed chunk and `world` gathered chunks behind the tables
  float* gathered = nullptr;
  int64_t chunk_len(int64_t chunk) const { return std::min(chunk_elems, total - chunk * chunk_elems); }
};

// every check of the contract (`who` names the caller in the refusal), with no GPU work; workspace may be NULL: sizes only
int grad_plan_check(const xdet_grad_slot* slots, int n_slots, int64_t chunk_elems, int world, const char* who, GradPlan* plan,
                    size_t* bytes);
// the same, then the two tables are uploaded on `s` and the plan's device pointers point into `workspace`
int grad_plan_upload(const xdet_grad_slot* slots, int n_slots, int64_t chunk_elems, int world, void* workspace, hipStream_t s,
                     const char* who, GradPlan* plan);
int grad_launch_pack(const GradPlan& plan, int64_t chunk, float* flat_out, hipStream_t s);
int grad_launch_reduce(const GradPlan& plan, int64_t chunk, const float* gathered, int world, hipStream_t s);

}  // namespace xdet
