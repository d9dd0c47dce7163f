// The Checkers env step inside the rollout kernels (agent_fwd.hip: rollout_step_kernel and the chunk-persistent
// rollout_chunk_kernel / roll_chunk_steps): the LDS layouts of the tile's env state, the nibble-row grid, the
// per-agent move / eat / view update and the local observation as a bit word. The restated dynamics of env.hip
// (oracle/env.py); the two kernels must stay bit-identical (tests/test_gpu_chunk.py), so these pieces of the step
// exist once, here. Where the kernels really differ (the step kernel's rolled agent loop over staged registers, the
// chunk kernel's unrolled loop over LDS position words) the difference stays with the caller: no helper takes a
// "which kernel" flag. The obs k-step loaders stay lambdas at their four call sites in agent_fwd.hip: as a shared
// functor they made instantiations of both kernels spill more.
#pragma once
#include "common.h"

namespace mm {

static constexpr int kRollMaxN = 10;    // 3 ceil(N / 2) <= 16 rows and agent markers 3 + k in a nibble
static constexpr int kRollMaxR = 16;    // rows of 8 cells: one 32-bit nibble word per row

// LDS staging of the env step (after the weight image): coordinate features, the tile's grids as nibble rows
// (row r of env l = cells (r, 0..7) at bits 4c of word l * roll_gbw(R) + r), agent cells r << 4 | c, done flags
struct RollLds {
  int stab, sgrid, spos, sdone, total;
};
__host__ __device__ __forceinline__ int roll_gbw(int R) { return R | 1; }   // odd word stride: fewer bank conflicts
__host__ __device__ __forceinline__ RollLds roll_lds(int R, int C, int N) {
  auto a16 = [](int x) { return (x + 15) & ~15; };
  RollLds m;
  int o = 0;
  m.stab = o;  o = a16(o + (R + C) * 4);
  m.sgrid = o; o = a16(o + 256 * roll_gbw(R) * 4);
  m.spos = o;  o = a16(o + 256 * N);
  m.sdone = o; o = a16(o + 256);
  m.total = o;
  return m;
}
// The chunk kernel's LDS after the weight image: coordinate features, nibble-row grids, 16-bit position words
// (prev_r, prev_c, r, c), dones by step parity, the behavior block's outgoing actions, the group counters
struct RollChunkLds {
  int stab, sgrid, spq, ssa, sdone, shx, sgrp, total;
};
// The fp16x3 step loop runs a block's 256 envs as kRollGroups independent groups of 64: group j is waves 4j .. 4j + 3
// and envs 64j .. 64j + 63 of the tile (the envs those waves own in the forward), words 8j .. 8j + 7 of each agent's
// 32 hand-off words. One wave of the group runs its env dynamics, 64 lanes wide: wave 4j + j, so that the four
// groups' dynamics chains sit on four different SIMDs (wave w runs on SIMD w mod 4).
static constexpr int kRollGroups = 4;
static constexpr int kRollGroupCtrs = 4;   // per group: reads done, dynamics done, reset done, slot-0 stores done
__host__ __device__ __forceinline__ int roll_group_of_wave(int wave) { return wave >> 2; }
__host__ __device__ __forceinline__ int roll_group_env0(int j) { return 64 * j; }
__host__ __device__ __forceinline__ int roll_group_word0(int j) { return 8 * j; }
__host__ __device__ __forceinline__ int roll_group_dyn_wave(int j) { return 4 * j + j; }
__host__ __device__ __forceinline__ RollChunkLds roll_chunk_lds(int R, int C, int N) {
  auto a16 = [](int x) { return (x + 15) & ~15; };
  RollChunkLds m;
  int o = 0;
  m.stab = o;  o = a16(o + (R + C) * 4);
  m.sgrid = o; o = a16(o + 256 * roll_gbw(R) * 4);
  m.spq = o;   o = a16(o + 256 * N * 2);
  m.ssa = o;   o = a16(o + 2 * 256 * 2);
  m.sdone = o; o = a16(o + 2 * 256);
  m.shx = o;   o = a16(o + N * 32 * 4);   // (exact body: the outgoing actions, 256 B; every block: the step's hand-off words)
  m.sgrp = o;  o = a16(o + kRollGroups * kRollGroupCtrs * 4);
  m.total = o;
  return m;
}

// 4 grid bytes (codes < 16) -> 4 nibbles, and back
__device__ __forceinline__ uint32_t nib_pack4(uint32_t x) {
  return (x & 0xFu) | ((x >> 4) & 0xF0u) | ((x >> 8) & 0xF00u) | ((x >> 12) & 0xF000u);
}
__device__ __forceinline__ uint32_t nib_unpack4(uint32_t x) {
  return (x & 0xFu) | ((x & 0xF0u) << 4) | ((x & 0xF00u) << 8) | ((x & 0xF000u) << 12);
}
// position word of the global state (prev_r << 24 | prev_c << 16 | r << 8 | c) -> 16 bits (4 per field), and back
__device__ __forceinline__ uint32_t pos16(int32_t w) {
  return (uint32_t)((((w >> 24) & 15) << 12) | (((w >> 16) & 15) << 8) | (((w >> 8) & 15) << 4) | (w & 15));
}
__device__ __forceinline__ int32_t pos32_from16(uint32_t w) {
  return (int32_t)((((w >> 12) & 15) << 24) | (((w >> 8) & 15) << 16) | (((w >> 4) & 15) << 8) | (w & 15));
}

// one env's grid, R rows of 8 byte cells as 16-byte pieces (2 rows each; RC = 8 R, R even) -> nibble rows
__device__ __forceinline__ void roll_unpack_rows(const uint4* gin, uint32_t* rows, int R) {
#pragma unroll
  for (int j = 0; j < kRollMaxR / 2; ++j)
    if (2 * j < R) {
      const uint4 g = gin[j];
      rows[2 * j] = nib_pack4(g.x) | (nib_pack4(g.y) << 16);
      if (2 * j + 1 < R) rows[2 * j + 1] = nib_pack4(g.z) | (nib_pack4(g.w) << 16);
    }
}
// nibble rows -> the env's grid in the global state; the initial grid where the episode ended (auto-reset)
__device__ __forceinline__ void roll_pack_rows(uint4* gout, const uint32_t* rows, const uint4* init_grid, bool done,
                                               int R) {
#pragma unroll
  for (int j = 0; j < kRollMaxR / 2; ++j)
    if (2 * j < R) {
      uint4 v;
      if (done) {
        v = init_grid[j];
      } else {
        const uint32_t a0 = rows[2 * j], a1 = 2 * j + 1 < R ? rows[2 * j + 1] : 0u;
        v = make_uint4(nib_unpack4(a0 & 0xFFFFu), nib_unpack4(a0 >> 16), nib_unpack4(a1 & 0xFFFFu),
                       nib_unpack4(a1 >> 16));
      }
      gout[j] = v;
    }
}

// Agent k's part of one env step (env_step_wave_kernel's phase 1 on nibble rows, one LDS round trip): w its 16-bit
// position word, a its action (0 down, 1 left, 2 up, 3 right, 4 stay). Moves it if the target cell is inside the grid
// and holds no agent, updates the env's rows and returns the new position word, the reward and whether it ate an apple.
struct RollMove {
  uint32_t w;
  float rew;
  bool ate;
};
__device__ __forceinline__ RollMove roll_agent_step(uint32_t w, int a, int k, uint32_t* rows, int R, int C,
                                                    float step_cost) {
  int r = (w >> 4) & 15, c = w & 15, pr = (w >> 12) & 15, pc = (w >> 8) & 15;
  const int nr = r + (a == 0 ? 1 : (a == 2 ? -1 : 0));
  const int nc = c + (a == 1 ? -1 : (a == 3 ? 1 : 0));
  const bool inside = a != 4 && nr >= 0 && nr < R && nc >= 0 && nc < C;
  // every row this agent may read or write, in one round trip: the target row, its own row, its stale prev row
  const uint32_t w_n = rows[inside ? nr : r], w_r = rows[r], w_p = rows[pr];
  asm volatile("" ::"v"(w_n), "v"(w_r), "v"(w_p));   // all three reads in flight together (not sunk into branches)
  const bool moved = inside && ((w_n >> (4 * nc)) & 15u) < 3u;
  if (moved) {
    pr = r;
    pc = c;
    r = nr;
    c = nc;
  }
  // view update (ma_gym __update_agent_view) when agent_pos != agent_prev_pos: empty at agent_prev_pos, the
  // marker at agent_pos; the fruit under a moving agent is eaten. Branch-free: both rows are written back
  // every agent (unchanged when there is no update; the (r, c) row last, so a shared row gets both edits).
  const bool upd = r != pr || c != pc;
  const uint32_t A = moved ? w_n : w_r;   // row of (r, c)
  const uint32_t B = moved ? w_r : w_p;   // row of (pr, pc)
  const uint32_t item = upd ? (A >> (4 * c)) & 15u : 0u;
  const float mag = (k & 1) == 0 ? 10.0f : 1.0f;   // (selects, no branch: item 1 lemon -mag, 2 apple +mag)
  const uint32_t clr = upd ? ~(15u << (4 * pc)) : ~0u;
  const uint32_t A1 = pr == r ? (A & clr) : A;
  rows[pr] = B & clr;
  rows[r] = upd ? ((A1 & ~(15u << (4 * c))) | ((uint32_t)(3 + k) << (4 * c))) : A1;
  return RollMove{(uint32_t)((pr << 12) | (pc << 8) | (r << 4) | c),
                  step_cost + (item == 2u ? mag : (item == 1u ? -mag : 0.0f)), item == 2u};
}

// The local observation of an agent at (r, c) as a bit word: bit f = feature f (>= 2) of get_agent_obs, i.e. bit
// 2 + 5 cell + ch for the 3 x 3 cells (row-major) x {lemon, apple, even agent, odd agent, wall}; off-grid cells
// are 0 (env.hip obs_value). Item code -> channel bits by a nibble table: 1 lemon, 2 apple, 3 + k agent k.
__device__ __forceinline__ uint64_t roll_obs_word(const uint32_t* rows, int R, int r, int c) {
  const uint32_t wm = r > 0 ? rows[r - 1] : 0u, w0 = rows[r], wp = r + 1 < R ? rows[r + 1] : 0u;
  auto nb3 = [c](uint32_t w) { return (c > 0 ? (w >> (4 * c - 4)) : (w << 4)) & 0xFFFu; };   // cells c-1, c, c+1
  const uint64_t items = (uint64_t)nb3(wm) | ((uint64_t)nb3(w0) << 12) | ((uint64_t)nb3(wp) << 24);
  constexpr uint64_t kLut = 0x4848484848484210ull;   // item -> {lemon 1, apple 2, even agent 4, odd agent 8}
  uint64_t word = 0;
#pragma unroll
  for (int cell = 0; cell < 9; ++cell) {
    const uint32_t it = (uint32_t)(items >> (4 * cell)) & 15u;
    word |= ((kLut >> (4 * it)) & 15ull) << (2 + 5 * cell);
  }
  return word;
}
// roll_obs_word shared by the 4 lanes (c, g = 0..3) of one env in the fp16x3 layout: lane group g < 3 builds the 3 cells
// of grid row r - 1 + g (bits 2 + 15 g .. 16 + 15 g of the word), and two v_permlane16/32_swap ORs per dword combine
// the groups (the 4 lanes of an env differ in lane bits 4 and 5) — the same word, one row read and ~1/3 of the ALU
// per lane. Every lane of the wave must be active.
__device__ __forceinline__ uint64_t roll_obs_word_g(const uint32_t* rows, int R, int r, int c, int g) {
  const int rr = r - 1 + g;
  const uint32_t w = (g < 3 && rr >= 0 && rr < R) ? rows[rr] : 0u;
  const uint32_t f12 = (c > 0 ? (w >> (4 * c - 4)) : (w << 4)) & 0xFFFu;   // cells c-1, c, c+1
  constexpr uint64_t kLut = 0x4848484848484210ull;   // item -> {lemon 1, apple 2, even agent 4, odd agent 8}
  uint32_t f15 = 0;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const uint32_t it = (f12 >> (4 * j)) & 15u;
    f15 |= (uint32_t)((kLut >> (4 * it)) & 15ull) << (5 * j);
  }
  uint32_t lo = g < 2 ? f15 << (2 + 15 * g) : 0u, hi = g == 2 ? f15 : 0u;
  auto or16 = [](uint32_t v) {
    const auto x = __builtin_amdgcn_permlane16_swap(v, v, false, false);
    return x[0] | x[1];
  };
  auto or32 = [](uint32_t v) {
    const auto x = __builtin_amdgcn_permlane32_swap(v, v, false, false);
    return x[0] | x[1];
  };
  lo = or32(or16(lo));
  hi = or32(or16(hi));
  return ((uint64_t)hi << 32) | lo;
}
// features f0 .. f0 + 3 of the word into x[0..3] (the coordinates for f < 2)
__device__ __forceinline__ void roll_feat4(uint64_t word, int f0, float cr, float cc, float* x) {
  const uint32_t fld = f0 < 64 ? (uint32_t)(word >> f0) : 0u;
#pragma unroll
  for (int i = 0; i < 4; ++i) x[i] = (float)((fld >> i) & 1u);
  if (f0 == 0) {
    x[0] = cr;
    x[1] = cc;
  }
}
typedef float f32x4u __attribute__((ext_vector_type(4), aligned(4)));
// store features f0 .. f0 + 3 (< D) of one (env, agent) row
__device__ __forceinline__ void roll_store4(float* dst, int f0, int D, const float* x) {
  if (f0 + 3 < D) {
    *reinterpret_cast<f32x4u*>(dst + f0) = f32x4u{x[0], x[1], x[2], x[3]};
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (f0 + i < D) dst[f0 + i] = x[i];
  }
}

// chunk start: d0 (slot 0 of the env's store row, this agent's part) <- s_t, the observation of the state before the
// step; rows the env's nibble rows, rc the agent's cell r << 4 | c; lane group g of the env's 4 lanes writes features
// 16 q + 4 g .. + 3
__device__ __forceinline__ void roll_store_slot0(const uint32_t* rows, int rc, const float* stab, int R, float* d0,
                                                 int D, int g) {
  const uint64_t wd = roll_obs_word(rows, R, rc >> 4, rc & 15);
  const float cr = stab[rc >> 4], cc = stab[R + (rc & 15)];
  for (int f0 = 4 * g; f0 < D; f0 += 16) {
    float x[4];
    roll_feat4(wd, f0, cr, cc, x);
    roll_store4(d0, f0, D, x);
  }
}

}  // namespace mm
