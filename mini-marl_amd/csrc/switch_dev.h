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

// The rules of oracle/switch.py SwitchOracle.step, element-level only: no LDS, no barrier, no launch geometry, nothing
// about how a caller keeps its cells (switch.hip: int8 pairs in registers; offq_collect.hip: r << 4 | c words in LDS),
// so the test against the other agents' cells stays with each caller.

// agent k starts at (0, 1) (0, 5) (2, 1) (2, 5)[k] and must reach (0, 6) (0, 0) (2, 6) (2, 0)[k], in its own row
__device__ __forceinline__ int sw_home_row(int k) { return k < 2 ? 0 : 2; }
__device__ __forceinline__ int sw_start_col(int k) { return (k & 1) ? 5 : 1; }
__device__ __forceinline__ int sw_target_col(int k) { return (k & 1) ? 0 : 6; }
__device__ __forceinline__ bool sw_at_target(int k, int r, int c) {
  return r == sw_home_row(k) && c == sw_target_col(k);
}

// the cell an agent at (r, c) asks for with act 0 down, 1 left, 2 up, 3 right, and whether it is an open cell of the
// grid; anything else (4 noop) is no move: open is false
struct SwMove {
  int r, c;
  bool open;
};
__device__ __forceinline__ SwMove sw_move(int r, int c, int act) {
  SwMove m;
  m.r = r + (act == 0) - (act == 2);
  m.c = c + (act == 3) - (act == 1);
  m.open = act >= 0 && act < 4 && sw_open(m.r, m.c);
  return m;
}

// an agent is paid kSwTargetReward on the step it reaches its target, the env's step_cost on every other step
constexpr float kSwTargetReward = 5.0f;

// the clock feature: Python's steps / max_steps (a double) rounded to float32
__device__ __forceinline__ float sw_clock(int steps, int max_steps) {
  return (float)((double)steps / (double)max_steps);
}

// agent k's local observation loc[0 .. ld) into the N rows at out: its own row (partial, D = ld), or its slot of every
// agent's row (full observable, D = ld N)
__device__ __forceinline__ void sw_write_local(float* __restrict__ out, int k, int N, int ld, int full,
                                               const float (&loc)[3]) {
  const int D = full ? ld * N : ld;
  if (full) {
    for (int j = 0; j < N; ++j)
      for (int f = 0; f < ld; ++f) out[j * D + k * ld + f] = loc[f];
  } else {
    for (int f = 0; f < ld; ++f) out[k * D + f] = loc[f];
  }
}

}  // namespace mm

struct mm_switch {
  mm_switch_cfg cfg;
  mm::SwitchTab tab;
  int64_t E;
  mm::SwitchState* st;
  float* reset_obs;   // [N, D] the (deterministic) reset obs
};
