// Plan -> Plan passes that run after the lowering (hip_plan.cpp, Planner::run), and the parameter /
// buffer helpers they share with it.  Internal to the planner.
#pragma once

#include <cstring>

#include "hip_plan.h"

namespace die {
namespace passes {

constexpr int kBufGraphIn = -2;
constexpr int kBufGraphOut = -3;

inline uint16_t to_bf16(float f) {
  uint32_t u;
  std::memcpy(&u, &f, 4);
  if ((u & 0x7F800000u) == 0x7F800000u) return static_cast<uint16_t>(u >> 16);  // inf/nan
  u += 0x7FFFu + ((u >> 16) & 1u);
  return static_cast<uint16_t>(u >> 16);
}

inline float from_bf16(uint16_t h) {
  const uint32_t u = static_cast<uint32_t>(h) << 16;
  float f;
  std::memcpy(&f, &u, 4);
  return f;
}

inline size_t round_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// An activation buffer of `bytes_per_sample` bf16 bytes (fp32 mode: hi and lo planes, twice that).
int new_buf(Plan& plan, size_t bytes_per_sample);
// Append to the parameter blob (256-byte aligned); the offset.
size_t push_f32(Plan& plan, const std::vector<float>& v);
size_t push_bf16(Plan& plan, const std::vector<uint16_t>& v);

void fuse_pool_affine(Plan& plan);
void fuse_stem_pool(Plan& plan);
void fuse_conv_pairs(Plan& plan);
void fuse_gap_fc(Plan& plan, int max_batch);
void fold_layernorm(Plan& plan);
void stats_from_producer(Plan& plan);
void mark_side_branches(Plan& plan);
// Buffer lifetimes and arena offsets for batches up to max_batch, and the plan's flop count.
void assign_arena(Plan& plan, int max_batch);

}  // namespace passes
}  // namespace die
