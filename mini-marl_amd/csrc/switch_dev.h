// Device view of the restated ma_gym Switch env (oracle/switch.py), shared by the env kernels (switch.hip) and the
// offpolicy episode collector (offq_collect.hip).
#pragma once
#include "common.h"
#include "minimarl.h"

namespace mm {

struct SwitchState {
  int8_t pos[4][2];
  uint8_t adone[4];
  int32_t steps;
};

// obs feature tables round(c / 6, 2), round(r / 2, 2) (Python floats -> float32), passed by value in
// the kernel arguments (no per-device constant-memory state to initialise)
struct SwitchTab {
  float col[7];
  float row[3];
};

// open cells of the 3 x 7 grid: the middle row and columns 0, 1, 5, 6
__device__ __forceinline__ bool sw_open(int r, int c) {
  return r >= 0 && r < 3 && c >= 0 && c < 7 && (r == 1 || c <= 1 || c >= 5);
}

}  // namespace mm

struct mm_switch {
  mm_switch_cfg cfg;
  mm::SwitchTab tab;
  int64_t E;
  mm::SwitchState* st;
  float* reset_obs;   // [N, D] the (deterministic) reset obs
};
