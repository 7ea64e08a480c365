// walk_device.h — small helpers shared by the lane-per-point walk kernels
// (k_walk.hip, k_mic.hip): a point's path bit, the progress-ordered wave
// priority and the block size of a walk launch.
#pragma once

#include "aes_device.h"

namespace dpf_amd {

__device__ __forceinline__ uint32_t PathBit(const uint4& p, int bit_index) {
  if (bit_index >= 128) return 0;
  uint32_t w = bit_index < 32 ? p.x : bit_index < 64 ? p.y : bit_index < 96 ? p.z : p.w;
  return (w >> (bit_index & 31)) & 1u;
}

// Progress-ordered wave priority for the lane-per-point walks: the
// sequencer serves a SIMD's older waves first, so the waves of a round of
// blocks finish one after another and the last ones run below the occupancy
// the LDS needs.  A wave starts at priority 3 and steps down one level per
// quarter of its levels, so the waves behind are served first (the scheme of
// KExpand's DPF_EXPAND_PRIO).  c2's batched 64-key launch 1.587-1.600 ->
// 1.555-1.577 ms (profiles/ab_walk_prio_r06x/); DPF_WALK_PRIO=0 turns it off.
#ifndef DPF_WALK_PRIO
#define DPF_WALK_PRIO 1
#endif
#ifndef DPF_DCF_PRIO
#define DPF_DCF_PRIO 1  // the same per hierarchy level in KDcfEvaluateDirect
#endif
__device__ __forceinline__ void WalkPrio(int level, int num_levels) {
  if constexpr (DPF_WALK_PRIO != 0) {
    if (num_levels < 8) return;
    const int q = (level * 4) / num_levels;  // wave-uniform
    if (level > 0 && q != ((level - 1) * 4) / num_levels) {
      if (q == 1)
        __builtin_amdgcn_s_setprio(2);
      else if (q == 2)
        __builtin_amdgcn_s_setprio(1);
      else
        __builtin_amdgcn_s_setprio(0);
    } else if (level == 0) {
      __builtin_amdgcn_s_setprio(3);
    }
  }
}

// Threads per block for a walk over n points: full blocks once the launch
// fills every CU (two blocks each), smaller ones before that so that small
// launches still spread over all CUs.
static int WalkBlock(int64_t n, int max_block = kPointsBlock) {
  int64_t per = (n + 2 * 256 - 1) / (2 * 256);
  per = (per + 63) / 64 * 64;
  return (int)std::min<int64_t>(max_block, std::max<int64_t>(64, per));
}

}  // namespace dpf_amd
