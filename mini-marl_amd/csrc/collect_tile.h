// What the one-launch collectors share (offq_collect.hip: the recurrent episode collector; moffq_collect.hip: the
// feed-forward transition collector): the exact-f32 MFMA fragment scheme of the agent net's trunk (weight images,
// register-chained layers, LayerNorm), the epsilon-greedy draw, the thread-linear field stores, and the two env tiles
// with their LDS layouts and argument checks. A kernel brings its own net layout (which images follow the trunk), its
// io struct and its step loop.
//
//   weights staged once per block into LDS as exact-f32 MFMA A-operand images (v_mfma_f32_32x32x2_f32, the
//           fragment maps of common.h): k-step s of row block rb, lane (i, h) holds W[32 rb + i][col(s, h)],
//           four k-steps per 16-byte piece, so a wave's ds_read_b128 is contiguous.
//   layers  activations chain through registers: D register s of the producing layer is the B operand of
//           k-step s of the next (kperm). Lane (j, h) holds 32 of row j's 64 features, its partner lane
//           j + 32 the others; a LayerNorm sum is one cross-half shuffle.
//   env     one lane per env steps it in LDS, agents in id order, between two barriers of the step.
//   tiles   CheckersTile  the in-LDS step of rollout_env.h (roll_agent_step / roll_obs_word) on nibble-row grids, step
//           and apple counts in the env lane's registers. The observation (D 47, 24 k-steps of layer 1) is never
//           materialised for the net: LayerNorm 0 and the first layer's B operands come from the 45-bit
//           observation word and the two coordinates.
//           SwitchTile  per env in LDS: the agents' cells r << 4 | c, their done flags, the step count and the clock,
//           moved by the rules of switch_dev.h (oracle/switch.py). Three floats per row [row feature, column feature,
//           clock], so layer 1 is one group of 4 k-steps (features 0..2, the rest zero; its image is 2 KiB, not 12)
//           and LayerNorm 0 is computed from the floats: mean, centred variance, 1 / sqrt(var + eps).
//   records a row's observation is kept as a record (Checkers: bit word + two coordinates; Switch: the three floats)
//           that the stores read through obs_elem. A layout holds REC records per row: observe(row + k OC_ROWS, ..)
//           writes record k of the row, obs_elem(i + k OC_ROWS D) reads it.
#pragma once
#include <algorithm>

#include "common.h"
#include "env_dev.h"
#include "minimarl.h"
#include "rollout_env.h"
#include "switch_dev.h"
#include "trunk.h"

namespace mm {
namespace {

constexpr int OC_D = 47, OC_H = 64, OC_A = 5;
constexpr int OS_D = 3;        // Switch: local observation with the clock
constexpr int OC_ROWS = 128;   // (env, agent) rows of a block: 4 waves x 32
constexpr int OC_MAXE = 64;    // envs of a block's tile

// Checkers: the net (layout Net), then the env tile with REC observation records per row
template <class Net, int REC>
struct CheckersLds : Net {
  static constexpr int stab = Net::net_end;         // [R + C] coordinate features
  static constexpr int init = stab + 32;            // [16] the reset grid as nibble rows
  static constexpr int grid = init + 16;            // [OC_MAXE][roll_gbw(R)] nibble rows
  static constexpr int pos = grid + OC_MAXE * (kRollMaxR | 1);   // [rows] 16-bit position words
  static constexpr int act = pos + OC_ROWS;         // [rows] the step's actions
  static constexpr int rew = act + OC_ROWS;         // [rows] the step's stored rewards
  static constexpr int cr = rew + OC_ROWS, cc = cr + REC * OC_ROWS;    // [REC][rows] coordinates of the observation
  static constexpr int word = cc + REC * OC_ROWS;   // [REC][rows] u64 observation words
  static constexpr int q = word + 2 * REC * OC_ROWS;   // [rows][A]
  static constexpr int done = q + OC_ROWS * OC_A;   // [OC_MAXE]
  static constexpr int total = done + OC_MAXE;
  static_assert((word & 1) == 0, "alignment");
};

// Switch: the net, then the env tile
template <class Net, int REC>
struct SwitchLds : Net {
  static constexpr int stab = Net::net_end;         // [3] row features, [7] column features at + 4
  static constexpr int pos = stab + 12;             // [rows] agent cells r << 4 | c
  static constexpr int adone = pos + OC_ROWS;       // [rows] agent done flags (0 / 1 as floats: the dones field)
  static constexpr int act = adone + OC_ROWS;       // [rows] the step's actions
  static constexpr int rew = act + OC_ROWS;         // [rows] the step's stored rewards
  static constexpr int cr = rew + OC_ROWS, cc = cr + REC * OC_ROWS, ck = cc + REC * OC_ROWS;   // [REC][rows] observation
  static constexpr int q = ck + REC * OC_ROWS;      // [rows][A]
  static constexpr int steps = q + OC_ROWS * OC_A;  // [OC_MAXE] step counts
  static constexpr int clk = steps + OC_MAXE;       // [OC_MAXE] the clock feature of the current state
  static constexpr int done = clk + OC_MAXE;        // [OC_MAXE] all agents done
  static constexpr int total = done + OC_MAXE;
};

// what a tile's rules need from the env handle
struct CheckersEnvArgs {
  const int8_t* init_grid;
  const int32_t* init_pos;
  const float* rtab;
  const float* ctab;
  int R, C, init_apples;
};

struct SwitchEnvArgs {
  SwitchTab tab;
};

// a kernel's arguments: its io struct (with N, max_steps, step_cost) and the tile's env part
template <class Io, class EnvArgs>
struct TileArgs : Io, EnvArgs {};

// A-operand image of W (row-major, leading dimension ld, rows x cols valid, zero outside): RB row blocks, KS k-steps
template <bool CHAIN>
__device__ __forceinline__ void oc_pack(float* dst, const float* __restrict__ W, int ld, int rows, int cols, int RB,
                                        int KS) {
  const int n = RB * KS * 64, s4n = KS >> 2;
  for (int o = threadIdx.x; o < n; o += blockDim.x) {
    const int si = o & 3, lane = (o >> 2) & 63, q = o >> 8;
    const int rb = q / s4n, s = (q - rb * s4n) * 4 + si;
    const int i = lane & 31, h = lane >> 5;
    const int row = 32 * rb + i, col = CHAIN ? 32 * (s >> 4) + kperm(s & 15, h) : 2 * s + h;
    dst[o] = (row < rows && col < cols) ? W[row * ld + col] : 0.0f;
  }
}

// acc[rb] += W[32 rb .. 32 rb + 31][:] x for NRB row blocks over KS k-steps; bval(s) = this lane's B operand of k-step s
template <int NRB, int KS, typename B>
__device__ __forceinline__ void oc_mma(f32x16* acc, const float* sW, int lane, B bval) {
#pragma unroll
  for (int s4 = 0; s4 < KS / 4; ++s4) {
    float av[NRB][4];
#pragma unroll
    for (int rb = 0; rb < NRB; ++rb) {
      const float4 a = *reinterpret_cast<const float4*>(sW + ((rb * (KS / 4) + s4) * 64 + lane) * 4);
      av[rb][0] = a.x;
      av[rb][1] = a.y;
      av[rb][2] = a.z;
      av[rb][3] = a.w;
    }
#pragma unroll
    for (int si = 0; si < 4; ++si) {
      const float b = bval(4 * s4 + si);
#pragma unroll
      for (int rb = 0; rb < NRB; ++rb) acc[rb] = mfma32(av[rb][si], b, acc[rb]);
    }
  }
}

// the 16 entries of a 32-feature vector that lane half h holds: register r <-> feature kperm(r, h)
__device__ __forceinline__ f32x16 oc_vec16(const float* v32, int h) {
  f32x16 o;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const float4 t = *reinterpret_cast<const float4*>(v32 + 8 * q + 4 * h);
    o[4 * q] = t.x;
    o[4 * q + 1] = t.y;
    o[4 * q + 2] = t.z;
    o[4 * q + 3] = t.w;
  }
  return o;
}

// LayerNorm over a row's 64 features (32 in this lane, 32 in lane ^ 32), in place
__device__ __forceinline__ void oc_ln(f32x16 (&v)[2], const float* sw, const float* sb, int h) {
  float s = 0.0f;
#pragma unroll
  for (int kb = 0; kb < 2; ++kb)
#pragma unroll
    for (int r = 0; r < 16; ++r) s += v[kb][r];
  s += __shfl_xor(s, 32);
  const float mu = s * (1.0f / OC_H);
  float q = 0.0f;
#pragma unroll
  for (int kb = 0; kb < 2; ++kb)
#pragma unroll
    for (int r = 0; r < 16; ++r) q = fmaf(v[kb][r] - mu, v[kb][r] - mu, q);
  q += __shfl_xor(q, 32);
  const float rs = 1.0f / sqrtf(q * (1.0f / OC_H) + kLnEps);
#pragma unroll
  for (int kb = 0; kb < 2; ++kb) {
    const f32x16 w = oc_vec16(sw + 32 * kb, h), b = oc_vec16(sb + 32 * kb, h);
#pragma unroll
    for (int r = 0; r < 16; ++r) v[kb][r] = (v[kb][r] - mu) * rs * w[r] + b[r];
  }
}

// base[g0 + i] = gen(i) for i < n, the block's threads on consecutive 16-byte slots (base 16-byte aligned)
template <typename G>
__device__ __forceinline__ void oc_store(float* base, int64_t g0, int n, G gen) {
  const int head = (int)(g0 & 3);
  float* slot0 = base + (g0 - head);
  const int nslot = (head + n + 3) >> 2;
  for (int v = threadIdx.x; v < nslot; v += blockDim.x) {
    const int i0 = 4 * v - head;
    if (i0 >= 0 && i0 + 3 < n) {
      *reinterpret_cast<float4*>(slot0 + 4 * v) = make_float4(gen(i0), gen(i0 + 1), gen(i0 + 2), gen(i0 + 3));
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (i0 + k >= 0 && i0 + k < n) slot0[4 * v + k] = gen(i0 + k);
    }
  }
}

// Stage the trunk of the net (MGeo<D, 64, 5> flat layout at P: W1, W2, the head Wo and their vectors) into the images
// and vectors of L, which names W1 W2 Wo ln0w ln0b b1 ln1w ln1b b2 ln2w ln2b bo; the caller's barrier follows
template <typename L, int D, int KS1>
__device__ __forceinline__ void oc_stage_trunk(float* sm, const float* __restrict__ P) {
  using G = MGeo<D, OC_H, OC_A>;
  const int tid = threadIdx.x;
  oc_pack<false>(sm + L::W1, P + G::W1, G::Dp, OC_H, D, 2, KS1);
  oc_pack<true>(sm + L::W2, P + G::W2, OC_H, OC_H, OC_H, 2, 32);
  oc_pack<true>(sm + L::Wo, P + G::Wo, OC_H, OC_A, OC_H, 1, 32);
  if (tid < 2 * KS1) {
    const int f = 2 * (tid % KS1) + tid / KS1;
    sm[L::ln0w + tid] = f < D ? P[G::ln0_w + f] : 0.0f;
    sm[L::ln0b + tid] = f < D ? P[G::ln0_b + f] : 0.0f;
  }
  if (tid < OC_H) {
    sm[L::b1 + tid] = P[G::b1 + tid];
    sm[L::ln1w + tid] = P[G::ln1_w + tid];
    sm[L::ln1b + tid] = P[G::ln1_b + tid];
    sm[L::b2 + tid] = P[G::b2 + tid];
    sm[L::ln2w + tid] = P[G::ln2_w + tid];
    sm[L::ln2b + tid] = P[G::ln2_b + tid];
  }
  if (tid < 32) sm[L::bo + tid] = tid < OC_A ? P[G::bo + tid] : 0.0f;
}

// Layers 1 and 2 from LayerNorm 0's output (x0[s] = this lane's normalised feature 2 s + h): f2 = LayerNorm 2's output
template <typename L, int KS1>
__device__ __forceinline__ void oc_trunk(const float* sm, const float (&x0)[KS1], f32x16 (&f2)[2], int lane, int h) {
  f32x16 f1[2];
  f1[0] = oc_vec16(sm + L::b1, h);
  f1[1] = oc_vec16(sm + L::b1 + 32, h);
  oc_mma<2, KS1>(f1, sm + L::W1, lane, [&](int s) { return x0[s]; });
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    f1[0][r] = fmaxf(f1[0][r], 0.0f);
    f1[1][r] = fmaxf(f1[1][r], 0.0f);
  }
  oc_ln(f1, sm + L::ln1w, sm + L::ln1b, h);
  f2[0] = oc_vec16(sm + L::b2, h);
  f2[1] = oc_vec16(sm + L::b2 + 32, h);
  oc_mma<2, 32>(f2, sm + L::W2, lane, [&](int s) { return f1[s >> 4][s & 15]; });
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    f2[0][r] = fmaxf(f2[0][r], 0.0f);
    f2[1][r] = fmaxf(f2[1][r], 0.0f);
  }
  oc_ln(f2, sm + L::ln2w, sm + L::ln2b, h);
}

// The head Linear(A) on y (a LayerNorm's output): Q 0..3 land in registers 0..3 of lane half 0 of the result, Q 4 in
// register 0 of half 1
template <typename L>
__device__ __forceinline__ f32x16 oc_head(const float* sm, const f32x16 (&y)[2], int lane, int h) {
  f32x16 qa = oc_vec16(sm + L::bo, h);
  oc_mma<1, 32>(&qa, sm + L::Wo, lane, [&](int s) { return y[s >> 4][s & 15]; });
  return qa;
}

// Epsilon-greedy on the head's result (every lane calls it; the row's owner lane writes): the first maximum, or the
// counter RNG's action where u < eps. sact[row] gets the action, sq[row][A] the Q values when they are wanted
__device__ __forceinline__ void oc_act(uint64_t seed, bool want_q, f32x16 qa, bool owner, int row, uint64_t ctr,
                                       uint64_t rinner, float eps, int* sact, float* sq) {
  const float q4 = __shfl_xor(qa[0], 32);
  if (owner) {
    const float qv[OC_A] = {qa[0], qa[1], qa[2], qa[3], q4};
    int g = 0;
    float best = qv[0];
#pragma unroll
    for (int k = 1; k < OC_A; ++k)
      if (qv[k] > best) {
        best = qv[k];
        g = k;
      }
    const float u = rng_uniform(rng_draw_inner(seed, ctr, rinner));
    const int ra = (int)rng_mod_small(rng_draw_inner(seed ^ 0x5bd1e995ull, ctr, rinner), OC_A);
    sact[row] = u < eps ? ra : g;
    if (want_q) {
#pragma unroll
      for (int k = 0; k < OC_A; ++k) sq[row * OC_A + k] = qv[k];
    }
  }
}

// Checkers tile: nibble-row grids and 16-bit position words in LDS, stepped by rollout_env.h; the env lane keeps the
// step and apple counts in registers. (Both tiles: float arrays of the LDS layout are used as sm[L::x + i], the
// members are the integer views; a is the kernel's TileArgs.)
template <class L_>
struct CheckersTileT {
  using L = L_;
  using EnvArgs = CheckersEnvArgs;
  static constexpr int D = OC_D, KS1 = 24;
  float* sm;
  uint32_t* sgrid = reinterpret_cast<uint32_t*>(sm + L::grid);
  uint32_t* spos = reinterpret_cast<uint32_t*>(sm + L::pos);
  uint64_t* sword = reinterpret_cast<uint64_t*>(sm + L::word);
  int steps = 0, apples = 0;   // the env lane's episode state (lane tid < ne owns env e0 + tid)

  // the coordinate tables and every env's reset state (the handle's init_grid / init_pos); ends behind a barrier
  template <class Args>
  __device__ __forceinline__ void stage(const Args& a, int ne, int nrows) {
    const int tid = threadIdx.x, R = a.R, C = a.C, gbw = roll_gbw(R);
    uint32_t* sinit = reinterpret_cast<uint32_t*>(sm + L::init);
    if (tid < R) {
      sm[L::stab + tid] = a.rtab[tid];
      uint32_t w = 0;
      for (int c = 0; c < C; ++c) w |= ((uint32_t)a.init_grid[tid * C + c] & 15u) << (4 * c);
      sinit[tid] = w;
    }
    if (tid < C) sm[L::stab + R + tid] = a.ctab[tid];
    __syncthreads();
    for (int i = tid; i < ne * R; i += blockDim.x) {
      const int le = i / R, r = i - le * R;
      sgrid[le * gbw + r] = sinit[r];
    }
    for (int i = tid; i < nrows; i += blockDim.x) spos[i] = pos16(a.init_pos[i % a.N]);
    apples = a.init_apples;
    __syncthreads();
  }

  // The env lane puts env le of the tile back to the state stage() gave it: grid rows from the staged init rows,
  // positions, step and apple counts
  template <class Args>
  __device__ __forceinline__ void reset(const Args& a, int le) {
    const uint32_t* sinit = reinterpret_cast<const uint32_t*>(sm + L::init);
    uint32_t* rows = sgrid + le * roll_gbw(a.R);
    for (int r = 0; r < a.R; ++r) rows[r] = sinit[r];
    for (int k = 0; k < a.N; ++k) spos[le * a.N + k] = pos16(a.init_pos[k]);
    steps = 0;
    apples = a.init_apples;
  }

  // The current observation of a row (rrow = row, or 0 for a lane past the tile; rle = its env of the tile) as a bit
  // word + two coordinates: the owner lane leaves that record (at index row) for the stores, which read it through
  // obs_elem. The observation is never materialised for the net: x0[s] = feature 2 s + h after LayerNorm 0, straight
  // from the word
  template <class Args>
  __device__ __forceinline__ void observe(const Args& a, int row, int rrow, int rle, bool owner, int h,
                                          float (&x0)[KS1]) {
    const uint32_t pw = spos[rrow];
    const int pr_ = (pw >> 4) & 15, pc_ = pw & 15;
    const uint64_t wd = roll_obs_word(sgrid + rle * roll_gbw(a.R), a.R, pr_, pc_);
    const float cr = sm[L::stab + pr_], cc = sm[L::stab + a.R + pc_];
    if (owner) {
      sword[row] = wd;
      sm[L::cr + row] = cr;
      sm[L::cc + row] = cc;
    }
    // LayerNorm 0 from the word: 2 coordinates, pc ones, 45 - pc zeros
    const float npc = (float)__popcll(wd);
    const float mu0 = (cr + cc + npc) * (1.0f / OC_D);
    const float dr = cr - mu0, dc = cc - mu0, d1 = 1.0f - mu0;
    const float var0 = (dr * dr + dc * dc + npc * (d1 * d1) + (45.0f - npc) * (mu0 * mu0)) * (1.0f / OC_D);
    const float rs0 = 1.0f / sqrtf(var0 + kLnEps);
    const uint64_t wh = wd >> h;
#pragma unroll
    for (int s4 = 0; s4 < 6; ++s4) {
      const float4 w4 = *reinterpret_cast<const float4*>(sm + L::ln0w + 24 * h + 4 * s4);
      const float4 b4 = *reinterpret_cast<const float4*>(sm + L::ln0b + 24 * h + 4 * s4);
      const float wv[4] = {w4.x, w4.y, w4.z, w4.w}, bv[4] = {b4.x, b4.y, b4.z, b4.w};
#pragma unroll
      for (int si = 0; si < 4; ++si) {
        const int s = 4 * s4 + si;
        const float xv = s == 0 ? (h ? cc : cr) : (float)((uint32_t)(wh >> (2 * s)) & 1u);
        x0[s] = (xv - mu0) * rs0 * wv[si] + bv[si];
      }
    }
  }

  // element i of the tile's [rows][D] observations
  __device__ __forceinline__ float obs_elem(int i) const {
    const int r = i / OC_D, f = i - r * OC_D;
    return f == 0 ? sm[L::cr + r] : (f == 1 ? sm[L::cc + r] : (float)((uint32_t)(sword[r] >> f) & 1u));
  }

  // The env lane steps env le of the tile, agents in id order: each agent's own reward into srew, their agent-order
  // sum into sum; returns whether the env is now done
  template <class Args>
  __device__ __forceinline__ bool step(const Args& a, int le, const int* sact, float* srew, float& sum) {
    const int N = a.N;
    uint32_t* rows = sgrid + le * roll_gbw(a.R);
#pragma unroll 1
    for (int k = 0; k < N; ++k) {
      const RollMove mv = roll_agent_step(spos[le * N + k], sact[le * N + k], k, rows, a.R, a.C, a.step_cost);
      spos[le * N + k] = mv.w;
      srew[le * N + k] = mv.rew;
      apples -= mv.ate ? 1 : 0;
      sum = k == 0 ? mv.rew : sum + mv.rew;
    }
    ++steps;
    return steps >= a.max_steps || apples == 0;
  }

  // dones[t, e, n] of tile row i: Checkers agents have no done flag of their own, so the env's
  template <class Args>
  __device__ __forceinline__ float agent_done(const Args& a, int i) const { return sm[L::done + i / a.N]; }

  // valid_transition of tile row i, read before the step: Checkers agents never leave a running env
  __device__ __forceinline__ float valid_before(int) const { return 1.0f; }
};

// Switch tile: per env in LDS the agents' cells r << 4 | c, their done flags (0 / 1 as floats: they are the dones
// field), the step count and the clock of the current state, stepped by the rules of switch_dev.h
template <class L_>
struct SwitchTileT {
  using L = L_;
  using EnvArgs = SwitchEnvArgs;
  static constexpr int D = OS_D, KS1 = 4;
  float* sm;
  uint32_t* spos = reinterpret_cast<uint32_t*>(sm + L::pos);
  int* ssteps = reinterpret_cast<int*>(sm + L::steps);

  // the feature tables and every env's reset state (the agents' start cells, step 0); ends behind a barrier
  template <class Args>
  __device__ __forceinline__ void stage(const Args& a, int ne, int nrows) {
    const int tid = threadIdx.x;
    if (tid < 3) sm[L::stab + tid] = a.tab.row[tid];
    if (tid < 7) sm[L::stab + 4 + tid] = a.tab.col[tid];
    for (int i = tid; i < nrows; i += blockDim.x) {
      const int k = i % a.N;
      spos[i] = (uint32_t)(sw_home_row(k) << 4 | sw_start_col(k));
      sm[L::adone + i] = 0.0f;
    }
    if (tid < ne) {
      ssteps[tid] = 0;
      sm[L::clk + tid] = 0.0f;
    }
    __syncthreads();
  }

  // As CheckersTileT::reset: start cells, agent done flags, step count, clock
  template <class Args>
  __device__ __forceinline__ void reset(const Args& a, int le) {
    for (int k = 0; k < a.N; ++k) {
      spos[le * a.N + k] = (uint32_t)(sw_home_row(k) << 4 | sw_start_col(k));
      sm[L::adone + le * a.N + k] = 0.0f;
    }
    ssteps[le] = 0;
    sm[L::clk + le] = 0.0f;
  }

  // As CheckersTileT::observe; the record is the observation itself: row feature, column feature, clock
  template <class Args>
  __device__ __forceinline__ void observe(const Args&, int row, int rrow, int rle, bool owner, int h,
                                          float (&x0)[KS1]) {
    const uint32_t pw = spos[rrow];
    const float cr = sm[L::stab + ((pw >> 4) & 3)], cc = sm[L::stab + 4 + (pw & 7)], ck = sm[L::clk + rle];
    if (owner) {
      sm[L::cr + row] = cr;
      sm[L::cc + row] = cc;
      sm[L::ck + row] = ck;
    }
    // LayerNorm 0 over the three floats: mean, centred variance. Lane half h feeds features h and 2 + h (feature 3 is
    // a zero pad: its LayerNorm weight, bias and W1 column are staged as zero)
    const float mu0 = ((cr + cc) + ck) / (float)OS_D;
    const float dr = cr - mu0, dc = cc - mu0, dk = ck - mu0;
    const float var0 = (dr * dr + dc * dc + dk * dk) / (float)OS_D;
    const float rs0 = 1.0f / sqrtf(var0 + kLnEps);
    const float4 w4 = *reinterpret_cast<const float4*>(sm + L::ln0w + 4 * h);
    const float4 b4 = *reinterpret_cast<const float4*>(sm + L::ln0b + 4 * h);
    x0[0] = (h ? dc : dr) * rs0 * w4.x + b4.x;
    x0[1] = (h ? 0.0f : dk) * rs0 * w4.y + b4.y;
    x0[2] = 0.0f;
    x0[3] = 0.0f;
  }

  __device__ __forceinline__ float obs_elem(int i) const {
    const int r = i / OS_D, f = i - r * OS_D;
    return sm[(f == 0 ? L::cr : (f == 1 ? L::cc : L::ck)) + r];
  }

  // As CheckersTileT::step, by oracle/switch.py SwitchOracle.step: the moves act on the cells in LDS, so a move sees
  // the cells as updated so far this step
  template <class Args>
  __device__ __forceinline__ bool step(const Args& a, int le, const int* sact, float* srew, float& sum) {
    const int N = a.N, b = le * N, steps = ssteps[le] + 1;
    const bool timeout = steps >= a.max_steps;
    float* sadone = sm + L::adone;
    bool all = true;
#pragma unroll 1
    for (int k = 0; k < N; ++k) {
      bool ad = sadone[b + k] != 0.0f;
      float rw = a.step_cost;
      if (!ad) {   // a finished agent keeps its cell and goes on receiving step_cost
        const uint32_t cw = spos[b + k];
        int r = (int)(cw >> 4), c = (int)(cw & 15);
        const SwMove m = sw_move(r, c, sact[b + k]);
        const uint32_t nw = (uint32_t)(m.r << 4 | m.c);
        bool ok = m.open;   // and no other agent, finished or not, holds the cell
        for (int j = 0; j < N; ++j) ok = ok && (j == k || spos[b + j] != nw);
        if (ok) {
          spos[b + k] = nw;
          r = m.r;
          c = m.c;
        }
        if (sw_at_target(k, r, c)) {
          ad = true;
          rw = kSwTargetReward;
        }
      }
      ad = ad || timeout;
      sadone[b + k] = ad ? 1.0f : 0.0f;
      srew[b + k] = rw;
      sum = k == 0 ? rw : sum + rw;
      all = all && ad;
    }
    ssteps[le] = steps;
    sm[L::clk + le] = sw_clock(steps, a.max_steps);
    return all;
  }

  // dones[t, e, n] of tile row i: agent n's own flag
  template <class Args>
  __device__ __forceinline__ float agent_done(const Args&, int i) const { return sm[L::adone + i]; }

  // valid_transition of tile row i, read before the step: 1 - the agent's done flag
  __device__ __forceinline__ float valid_before(int i) const { return 1.0f - sm[L::adone + i]; }
};

// ---- host side: the argument checks and their error report, shared by the collectors' entry points
inline const char* range_check(int64_t E, int32_t T) {
  return (E < 1 || E > (int64_t)1 << 24 || T < 1 || T > 65536) ? "E must be in [1, 2^24] and T in [1, 65536]" : nullptr;
}

inline int report(const char* who, const char* why, const mm_offq_dims* d, int64_t E, int32_t T, bool on) {
  if (why && on)
    set_error("%s: unsupported configuration: %s (obs_dim %d hidden %d n_actions %d n_agents %d E %lld T %d)", who, why,
              d ? d->obs_dim : -1, d ? d->hidden : -1, d ? d->n_actions : -1, d ? d->n_agents : -1, (long long)E,
              (int)T);
  return why ? MM_EINVAL : MM_OK;
}

// the collectors feed the agent net the observation alone
inline const char* no_prev_act() {
  return "prev_act_inp is not built for the collectors (the trainer mm_offq_loss_grad has it)";
}

inline int collect_check(const char* who, const mm_env* env, const mm_offq_dims* d, int64_t E, int32_t T, bool rep) {
  const char* why = nullptr;
  if (d && d->prev_act_inp) {
    why = no_prev_act();
  } else if (!env || !d) {
    why = "null env or dims";
  } else {
    const EnvDev& ev = env->d;
    if (d->obs_dim != OC_D || d->hidden != OC_H || d->n_actions != OC_A)
      why = "the agent net must be D 47, H 64, A 5";
    else if (ev.full_obs || ev.D != OC_D)
      why = "the env must give local observations (D 47)";
    else if (d->n_agents != ev.N || ev.N < 1 || ev.N > kRollMaxN)
      why = "dims.n_agents must equal the env's agents, 1..kRollMaxN";
    else if (ev.R > kRollMaxR || ev.C != 8)
      why = "the env grid must have 8 columns and at most 16 rows";
    else
      why = range_check(E, T);
  }
  return report(who, why, d, E, T, rep);
}

inline int collect_switch_check(const char* who, const mm_switch* env, const mm_offq_dims* d, int64_t E, int32_t T,
                                bool rep) {
  const char* why = nullptr;
  if (d && d->prev_act_inp) {
    why = no_prev_act();
  } else if (!env || !d) {
    why = "null env or dims";
  } else {
    const mm_switch_cfg& c = env->cfg;
    if (d->obs_dim != OS_D || d->hidden != OC_H || d->n_actions != OC_A)
      why = "the agent net must be D 3, H 64, A 5";
    else if (c.full_observable)
      why = "the Switch env must give local observations (full_observable is not built for this path)";
    else if (!c.clock)
      why = "the Switch env must have the clock feature (D 3)";
    else if (d->n_agents != c.n_agents || c.n_agents < 2 || c.n_agents > 4)
      why = "dims.n_agents must equal the env's agents, 2..4";
    else
      why = range_check(E, T);
  }
  return report(who, why, d, E, T, rep);
}

inline CheckersEnvArgs checkers_env_args(const EnvDev& ev) {
  return CheckersEnvArgs{ev.init_grid, ev.init_pos, ev.rtab, ev.ctab, ev.R, ev.C, ev.init_apples};
}

}  // namespace
}  // namespace mm
