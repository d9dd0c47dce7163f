// What the feed-forward transition collectors share (moffq_collect.hip: epsilon-greedy on Q for mqmix / mvdn;
// maddpg_collect.hip: Gumbel-softmax sampling of the actor's logits for maddpg / matd3) on top of collect_tile.h: the LDS
// layout of the staged MLP net, what the transition loop adds to a tile, the launch arguments with their checks, the ring
// stores and the launch. A kernel brings its action rule and its step loop.
#pragma once
#include "collect_tile.h"

namespace mm {
namespace {

// LDS layout of the staged feed-forward net, float offsets (images and vectors start on 16 bytes)
template <int KS1>
struct McNetLds {
  static constexpr int W1 = 0;                      // [2 rb][KS1 / 4][64][4]   col(s, h) = 2 s + h
  static constexpr int W2 = W1 + 2 * KS1 * 64;      // [2 rb][8][64][4]   col(s, h) = 32 (s >> 4) + kperm(s & 15, h)
  static constexpr int Wo = W2 + 2 * 32 * 64;       // [1 rb][8][64][4]   rows >= A zero
  static constexpr int ln0w = Wo + 32 * 64;         // [2 h][KS1]: feature 2 s + h (D.. -> 0)
  static constexpr int ln0b = ln0w + 2 * KS1;
  static constexpr int b1 = ln0b + 2 * KS1, ln1w = b1 + 64, ln1b = ln1w + 64;
  static constexpr int b2 = ln1b + 64, ln2w = b2 + 64, ln2b = ln2w + 64;
  static constexpr int bo = ln2b + 64;              // [32] (A.. zero)
  static constexpr int net_end = bo + 32;
  static_assert((KS1 & 3) == 0 && (ln0w & 3) == 0, "alignment");
};

// the tile (two records per row), then what the transition loop adds
template <class Tile>
struct McLds : Tile {
  static constexpr int valid = Tile::total;         // [rows] valid_transition of the step
  static constexpr int adn = valid + OC_ROWS;       // [rows] the agents' done flags after the step
  static constexpr int total = adn + OC_ROWS;
  static constexpr int bytes = total * 4;
};
using McCheckersLds = McLds<CheckersLds<McNetLds<24>, 2>>;
using McSwitchLds = McLds<SwitchLds<McNetLds<4>, 2>>;
static_assert(3 * McCheckersLds::bytes <= 160 * 1024 && 3 * McSwitchLds::bytes <= 160 * 1024, "three blocks per CU");

struct McIo {
  const float* P;
  const float* eps;
  const unsigned long long* counter;
  uint64_t counter0, seed;
  float *obs, *next_obs, *acts, *rew, *dones, *dones_env, *valid, *q_out, *ret_out;
  int32_t* ndone_out;
  int64_t first, size;
  int E, T, N, EB, max_steps, common;
  float step_cost;
};

// base[(s0 + k) X + x] = gen(k X + x) for the k < ne transitions of a block's step: one run, or two where the ring ends
// after n1 of them
template <typename G>
__device__ __forceinline__ void mc_store(float* base, int64_t s0, int n1, int ne, int X, G gen) {
  oc_store(base, s0 * X, n1 * X, gen);
  if (n1 < ne) oc_store(base, 0, (ne - n1) * X, [&](int i) { return gen(i + n1 * X); });
}

// The env phase of a step, between two barriers: lane tid < ne steps env e0 + tid of the tile (every env is live) and
// leaves valid_transition from the state before the step, the stored rewards and the done flags in LDS; the window's
// return and finished episodes add up in its registers. Returns whether the env is now done
template <class Env, class Args>
__device__ __forceinline__ bool mc_env_step(Env& env, const Args& a, float* sm, int tid, float& ret, int& nd) {
  using L = typename Env::L;
  const int N = a.N;
  const int* sact = reinterpret_cast<const int*>(sm + L::act);
  float* srew = sm + L::rew;
  for (int k = 0; k < N; ++k) sm[L::valid + tid * N + k] = env.valid_before(tid * N + k);
  float sum = 0.0f;
  const bool edone = env.step(a, tid, sact, srew, sum);
  if (a.common)
    for (int k = 0; k < N; ++k) srew[tid * N + k] = sum;
  sm[L::done + tid] = edone ? 1.0f : 0.0f;
  for (int k = 0; k < N; ++k) sm[L::adn + tid * N + k] = env.agent_done(a, tid * N + k);
  ret += srew[tid * N];
  nd += edone ? 1 : 0;
  return edone;
}

// The stores of step t, by every thread: the block's transitions j0 .. j0 + ne go to ring slots s0 .. (n1 of them
// before the ring's end); record 0 is obs, record 1 next_obs
template <class Env, class Args>
__device__ __forceinline__ void mc_store_step(const Env& env, const Args& a, const float* sm, int t, int e0, int ne) {
  using L = typename Env::L;
  constexpr int D = Env::D;
  const int N = a.N;
  const int* sact = reinterpret_cast<const int*>(sm + L::act);
  const int64_t j0 = (int64_t)t * a.E + e0;
  const int64_t s0 = (a.first + j0) % a.size;
  const int n1 = a.size - s0 < (int64_t)ne ? (int)(a.size - s0) : ne;
  mc_store(a.obs, s0, n1, ne, N * D, [&](int i) { return env.obs_elem(i); });
  mc_store(a.next_obs, s0, n1, ne, N * D, [&](int i) { return env.obs_elem(i + OC_ROWS * D); });
  mc_store(a.acts, s0, n1, ne, N * OC_A, [&](int i) {
    const int r = i / OC_A;
    return sact[r] == i - r * OC_A ? 1.0f : 0.0f;
  });
  mc_store(a.rew, s0, n1, ne, N, [&](int i) { return sm[L::rew + i]; });
  mc_store(a.dones, s0, n1, ne, N, [&](int i) { return sm[L::adn + i]; });
  mc_store(a.dones_env, s0, n1, ne, 1, [&](int i) { return sm[L::done + i]; });
  mc_store(a.valid, s0, n1, ne, N, [&](int i) { return sm[L::valid + i]; });
}

// the launch arguments both tiles share; EB = envs of a block's tile
int fill_io(McIo& a, const char* who, const float* P, const mm_moffq_collect_io* io, int64_t n_envs, int32_t T, int N,
            int max_steps, float step_cost) {
  MM_REQUIRE(P && io && io->eps && io->obs && io->next_obs && io->acts && io->rewards && io->dones && io->dones_env &&
                 io->valid_transition,
             "%s: null argument (P, io, eps and the seven written fields are required)", who);
  const void* al[] = {P, io->obs, io->next_obs, io->acts, io->rewards, io->dones, io->dones_env, io->valid_transition,
                      io->q_out};
  for (const void* p : al) MM_REQUIRE(((uintptr_t)p & 15) == 0, "%s: P and the output fields must be 16-byte aligned", who);
  MM_REQUIRE(io->size >= n_envs * T && io->first >= 0 && io->first < io->size,
             "%s: the window's T * E = %lld transitions must fit the store (size %lld) and first (%lld) lie in it", who,
             (long long)(n_envs * T), (long long)io->size, (long long)io->first);
  a.P = P;
  a.eps = io->eps;
  a.counter = reinterpret_cast<const unsigned long long*>(io->counter);
  a.counter0 = io->counter0;
  a.seed = io->seed;
  a.obs = io->obs;
  a.next_obs = io->next_obs;
  a.acts = io->acts;
  a.rew = io->rewards;
  a.dones = io->dones;
  a.dones_env = io->dones_env;
  a.valid = io->valid_transition;
  a.q_out = io->q_out;
  a.ret_out = io->ret_out;
  a.ndone_out = io->n_done_out;
  a.first = io->first;
  a.size = io->size;
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
int launch_collect(const Args& a, int64_t n_envs, hipStream_t s) {
  constexpr int lds = Env::L::bytes;
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
