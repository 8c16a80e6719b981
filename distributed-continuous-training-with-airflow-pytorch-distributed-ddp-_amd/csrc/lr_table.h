// The device learning-rate table (learning-rate schedulers, trainer/lr_schedule.py): per-step rates read on the device,
// indexed by the Adam step count the kernels already keep there - so a captured graph or a persistent launch follows
// a schedule with nothing baked into its arguments and no host work per step.
//
// One fp32 buffer with a fixed address for the whole fit:
//   words 0..3   header {int32 t0, int32 len, 0, 0}
//   words 4..    lr[0 .. len) in fp32
// lr[k] is the rate of the optimizer step that runs after t0 + k steps have been taken; the index is taken - t0,
// clamped to [0, len - 1]; len >= 1 is the writer's duty (the kernels cannot refuse an empty table).  The host evaluates the user's torch scheduler into it (no scheduler formulas here).
#pragma once
#include <hip/hip_runtime.h>

namespace dct {

constexpr int LR_TABLE_HEADER = 4;  // words before lr[0]

// The rate of the step that runs after `taken` steps: the table's when one is set, the scalar otherwise.
// (A kernel whose counter already includes the step it applies passes counter - 1.)
__device__ __forceinline__ float lr_for(const float* __restrict__ tab, float lr, int taken) {
  if (!tab) return lr;
  const int2 h = *reinterpret_cast<const int2*>(tab);  // {t0, len}: one 8-byte load, independent of the counter's
  int k = taken - h.x;
  k = k > h.y - 1 ? h.y - 1 : k;
  k = k < 0 ? 0 : k;
  return tab[LR_TABLE_HEADER + k];
}

}  // namespace dct
