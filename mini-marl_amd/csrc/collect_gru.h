// What the one-launch episode collectors share (offq_collect.hip: epsilon-greedy on the GRU Q-net for qmix / vdn;
// rmaddpg_collect.hip: Gumbel-softmax sampling of the GRU actor's logits for rmaddpg / rmatd3) on top of collect_tile.h:
// the LDS layout of the staged recurrent net (the trunk, then the GRU images), its staging, the net of one step with the
// hidden state in registers, the launch arguments with their checks and the launch. A kernel brings its action rule and
// its step loop.
#pragma once
#include "collect_tile.h"

namespace mm {
namespace {

// LDS layout of the staged net, float offsets (every weight image and vector starts on 16 bytes). KS1 = k-steps of
// layer 1 (a multiple of 4, 2 KS1 >= D)
template <int KS1>
struct OcNetLds {
  static constexpr int W1 = 0;                      // [2 rb][KS1 / 4][64][4]   col(s, h) = 2 s + h
  static constexpr int W2 = W1 + 2 * KS1 * 64;      // [2 rb][8][64][4]   col(s, h) = 32 (s >> 4) + kperm(s & 15, h)
  static constexpr int Wih = W2 + 2 * 32 * 64;      // [6 rb][8][64][4]
  static constexpr int Whh = Wih + 6 * 32 * 64;     // [6 rb][8][64][4]
  static constexpr int Wo = Whh + 6 * 32 * 64;      // [1 rb][8][64][4]   rows >= A zero
  static constexpr int ln0w = Wo + 32 * 64;         // [2 h][KS1]: feature 2 s + h (D.. -> 0)
  static constexpr int ln0b = ln0w + 2 * KS1;
  static constexpr int b1 = ln0b + 2 * KS1, ln1w = b1 + 64, ln1b = ln1w + 64;
  static constexpr int b2 = ln1b + 64, ln2w = b2 + 64, ln2b = ln2w + 64;
  static constexpr int brz = ln2b + 64;             // [128] b_ih + b_hh of the r and z gates
  static constexpr int bin = brz + 128, bhn = bin + 64;
  static constexpr int lnrw = bhn + 64, lnrb = lnrw + 64;
  static constexpr int bo = lnrb + 64;              // [32] (A.. zero)
  static constexpr int net_end = bo + 32;
  static_assert((KS1 & 3) == 0 && (ln0w & 3) == 0, "alignment");
};

using OcLds = CheckersLds<OcNetLds<24>, 1>;
using OsLds = SwitchLds<OcNetLds<4>, 1>;
static_assert(OcLds::total * 4 <= 160 * 1024, "LDS budget");
static_assert(OsLds::total * 4 <= 160 * 1024, "LDS budget");
using CheckersTile = CheckersTileT<OcLds>;
using SwitchTile = SwitchTileT<OsLds>;

// what the episode kernels take: the net, the exploration stream, the episode fields
struct OcIo {
  const float* P;
  const float* eps;
  const unsigned long long* counter;
  uint64_t counter0, seed;
  float *obs, *acts, *rew, *dones, *dones_env, *q_out, *ret_out;
  int E, T, N, EB, max_steps, common;
  float step_cost;
};

// stage the net (MGeo<D, 64, 5> flat layout at P) into the images and vectors of L; the caller's barrier follows
template <typename L, int D, int KS1>
__device__ __forceinline__ void oc_stage_net(float* sm, const float* __restrict__ P) {
  using G = MGeo<D, OC_H, OC_A>;
  const int tid = threadIdx.x;
  oc_stage_trunk<L, D, KS1>(sm, P);
  oc_pack<true>(sm + L::Wih, P + G::Wih, OC_H, 3 * OC_H, OC_H, 6, 32);
  oc_pack<true>(sm + L::Whh, P + G::Whh, OC_H, 3 * OC_H, OC_H, 6, 32);
  if (tid < OC_H) {
    sm[L::brz + tid] = P[G::bih + tid] + P[G::bhh + tid];
    sm[L::brz + OC_H + tid] = P[G::bih + OC_H + tid] + P[G::bhh + OC_H + tid];
    sm[L::bin + tid] = P[G::bih + 2 * OC_H + tid];
    sm[L::bhn + tid] = P[G::bhh + 2 * OC_H + tid];
    sm[L::lnrw + tid] = P[G::lnr_w + tid];
    sm[L::lnrb + tid] = P[G::lnr_b + tid];
  }
}

// The net of one step from LayerNorm 0's output: x0[s] = this lane's normalised feature 2 s + h. Updates the hidden
// state in place; outputs 0..3 of the head land in registers 0..3 of lane half 0 of the result, output 4 in register 0
// of half 1
template <typename L, int KS1>
__device__ __forceinline__ f32x16 oc_net(const float* sm, const float (&x0)[KS1], f32x16 (&hid)[2], int lane, int h) {
  // ---- layer 1, layer 2
  f32x16 f2[2];
  oc_trunk<L, KS1>(sm, x0, f2, lane, h);
  // ---- GRU: g[0..3] r | z pre-activations (input + hidden side), g[4..5] W_in x + b_in, g[6..7] W_hn h + b_hn
  {
    f32x16 g[8];
#pragma unroll
    for (int kb = 0; kb < 4; ++kb) g[kb] = oc_vec16(sm + L::brz + 32 * kb, h);
#pragma unroll
    for (int kb = 0; kb < 2; ++kb) {
      g[4 + kb] = oc_vec16(sm + L::bin + 32 * kb, h);
      g[6 + kb] = oc_vec16(sm + L::bhn + 32 * kb, h);
    }
    oc_mma<6, 32>(g, sm + L::Wih, lane, [&](int s) { return f2[s >> 4][s & 15]; });
    oc_mma<4, 32>(g, sm + L::Whh, lane, [&](int s) { return hid[s >> 4][s & 15]; });
    oc_mma<2, 32>(g + 6, sm + L::Whh + 4 * 8 * 256, lane, [&](int s) { return hid[s >> 4][s & 15]; });
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float rr = sigmoidf_(g[kb][r]), zz = sigmoidf_(g[2 + kb][r]);
        const float nn = tanhf_(g[4 + kb][r] + rr * g[6 + kb][r]);
        hid[kb][r] = nn + zz * (hid[kb][r] - nn);
      }
  }
  // ---- head: LN, Linear(A)
  f32x16 y[2] = {hid[0], hid[1]};
  oc_ln(y, sm + L::lnrw, sm + L::lnrb, h);
  return oc_head<L>(sm, y, lane, h);
}

// the launch arguments both tiles share; EB = envs of a block's tile
inline int fill_io(OcIo& a, const char* who, const float* P, const mm_offq_collect_io* io, int64_t n_envs, int32_t T,
                   int N, int max_steps, float step_cost) {
  MM_REQUIRE(P && io && io->eps && io->obs && io->acts && io->rewards && io->dones && io->dones_env,
             "%s: null argument (P, io, eps and the five written fields are required)", who);
  const void* al[] = {P, io->obs, io->acts, io->rewards, io->dones, io->dones_env, io->q_out};
  for (const void* p : al) MM_REQUIRE(((uintptr_t)p & 15) == 0, "%s: P and the output fields must be 16-byte aligned", who);
  a.P = P;
  a.eps = io->eps;
  a.counter = reinterpret_cast<const unsigned long long*>(io->counter);
  a.counter0 = io->counter0;
  a.seed = io->seed;
  a.obs = io->obs;
  a.acts = io->acts;
  a.rew = io->rewards;
  a.dones = io->dones;
  a.dones_env = io->dones_env;
  a.q_out = io->q_out;
  a.ret_out = io->ret_out;
  a.E = (int)n_envs;
  a.T = T;
  a.N = N;
  a.EB = std::min(OC_ROWS / N, OC_MAXE);
  a.max_steps = max_steps;
  a.common = io->common_reward ? 1 : 0;
  a.step_cost = step_cost;
  return MM_OK;
}

// the launch of a tile's kernel: its dynamic-LDS attribute (set once per process), one block per EB envs
template <class Env, auto Kernel, class Args>
int launch_episode(const Args& a, int64_t n_envs, hipStream_t s) {
  constexpr int lds = Env::L::total * 4;
  static const hipError_t set_lds_attribute =
      hipFuncSetAttribute((const void*)Kernel, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
  MM_HIP_CHECK(set_lds_attribute);
  const unsigned nb = (unsigned)((n_envs + a.EB - 1) / a.EB);
  hipLaunchKernelGGL(Kernel, dim3(nb), dim3(256), lds, s, a);
  MM_HIP_CHECK(hipGetLastError());
  return MM_OK;
}

}  // namespace
}  // namespace mm
