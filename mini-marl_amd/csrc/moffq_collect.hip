// Feed-forward transition collector of offpolicy mqmix / mvdn on gfx950: the collect loop of the reference's MLP
// runner for E lockstep Checkers or Switch envs, a window of T steps from reset in ONE launch, written as T E single
// transitions (MlpReplayBuffer rows, offpolicy/utils/mlp_buffer.py:161-208), every one of them valid: an env that
// finishes is put back to its reset state inside the window instead of idling to the window's end.
//
//   net     the MLP AgentQFunction of moffq.hip, LN(D) -> [Linear, ReLU, LN] x 2 -> Linear(A), read from the 18-tensor
//           trunk vector (the six recurrent tensors are not read). Fragment scheme of collect_tile.h: exact-f32
//           v_mfma_f32_32x32x2_f32 A-operand images in LDS, activations chained through registers, LayerNorm 0 straight
//           from the observation record. No hidden state: a row's registers hold one step's activations only.
//   LDS     McNetLds: W1, W2 and the head image, 36 KiB on Checkers (26 KiB on Switch) where the episode collector's
//           net takes 132; with the vectors and the tile (two observation records per row: obs and next_obs) 52 KiB /
//           37 KiB per block. The freed room goes to residency, not to a larger tile: the block keeps 256 threads and 128 rows,
//           so three blocks share a CU (a step has a phase in which only the env lanes of wave 0 work: one block's env
//           step then overlaps another's MFMA) and a given E still spreads over as many CUs as before. A larger row
//           tile would serialise more envs on the env lanes of one block. Neither choice has been timed.
//   step t  observe (record 0 = obs) -> net -> epsilon-greedy, counter c0 + t, the streams of oc_act | barrier |
//           env lanes: valid_transition from the state before the step, the step, rewards, done flags | barrier |
//           observe again (record 1 = next_obs: the state after the step, the terminal observation at done) | barrier |
//           stores; the env lanes of done envs reset them (the stores read no state the reset writes) | barrier.
//           Every row observes twice a step; reusing record 1 as the next step's record 0 for envs that did not reset
//           is left undone.
//   store   transition j = t E + e goes to ring slot (first + j) % size of every field's [size][row] store. A block's
//           step is the run [e0, e0 + ne) of one t: contiguous, or two runs where it crosses the ring end; each run is
//           written thread-linear with 16-byte stores (scalar head / tail). first = 0, size = T E is a plain staging
//           tensor; a replay ring's stores, cursor and capacity make the launch the insert. T E <= size.
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

// (launch bounds: 3 waves per SIMD = three resident blocks per CU, which caps the kernel at 168 registers)
template <class Env>
__global__ __launch_bounds__(256, 3) void moffq_collect_kernel(TileArgs<McIo, typename Env::EnvArgs> a) {
  using L = typename Env::L;
  constexpr int D = Env::D, KS1 = Env::KS1;
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5;
  const int N = a.N;
  const int e0 = blockIdx.x * a.EB, ne = min(a.EB, a.E - e0), nrows = ne * N;
  int* sact = reinterpret_cast<int*>(sm + L::act);
  float* srew = sm + L::rew;
  float* sq = sm + L::q;
  float* sdone = sm + L::done;
  float* svalid = sm + L::valid;
  float* sadn = sm + L::adn;
  Env env{sm};

  // ---- stage the net and the reset state
  oc_stage_trunk<L, D, KS1>(sm, a.P);
  env.stage(a, ne, nrows);

  // this lane's row of the tile (both lane halves of a row compute its scalars redundantly)
  const int row = wave * 32 + (lane & 31);
  const bool valid = row < nrows;
  const int rle = valid ? row / N : 0, rn = valid ? row - rle * N : 0, rrow = valid ? row : 0;
  const bool owner = valid && h == 0;
  const uint64_t rinner = rng_inner((uint64_t)(e0 + rle), (uint64_t)rn);
  const float eps = *a.eps;
  const uint64_t c0 = a.counter ? (uint64_t)*a.counter : a.counter0;
  bool edone = false;   // the env lane's (lane tid < ne owns env e0 + tid)
  float ret = 0.0f;
  int nd = 0;

  for (int t = 0; t < a.T; ++t) {
    // ---- obs, net, action
    {
      float x0[KS1];   // LayerNorm 0's output: this lane's feature 2 s + h
      env.observe(a, row, rrow, rle, owner, h, x0);
      f32x16 f2[2];
      oc_trunk<L, KS1>(sm, x0, f2, lane, h);
      const f32x16 qa = oc_head<L>(sm, f2, lane, h);
      oc_act(a.seed, a.q_out != nullptr, qa, owner, row, c0 + (uint64_t)t, rinner, eps, sact, sq);
    }
    lds_sync();

    // ---- env step: one lane per env, every env is live
    if (tid < ne) {
      for (int k = 0; k < N; ++k) svalid[tid * N + k] = env.valid_before(tid * N + k);
      float sum = 0.0f;
      edone = env.step(a, tid, sact, srew, sum);
      if (a.common)
        for (int k = 0; k < N; ++k) srew[tid * N + k] = sum;
      sdone[tid] = edone ? 1.0f : 0.0f;
      for (int k = 0; k < N; ++k) sadn[tid * N + k] = env.agent_done(a, tid * N + k);
      ret += srew[tid * N];
      nd += edone ? 1 : 0;
    }
    lds_sync();

    // ---- next_obs: the state after the step, into record 1
    {
      float xn[KS1];
      env.observe(a, row + OC_ROWS, rrow, rle, owner, h, xn);
    }
    lds_sync();

    // ---- the step's transitions j0 .. j0 + ne: ring slots s0 .. (n1 of them before the ring's end)
    const int64_t j0 = (int64_t)t * a.E + e0;
    const int64_t s0 = (a.first + j0) % a.size;
    const int n1 = a.size - s0 < (int64_t)ne ? (int)(a.size - s0) : ne;
    mc_store(a.obs, s0, n1, ne, N * D, [&](int i) { return env.obs_elem(i); });
    mc_store(a.next_obs, s0, n1, ne, N * D, [&](int i) { return env.obs_elem(i + OC_ROWS * D); });
    mc_store(a.acts, s0, n1, ne, N * OC_A, [&](int i) {
      const int r = i / OC_A;
      return sact[r] == i - r * OC_A ? 1.0f : 0.0f;
    });
    mc_store(a.rew, s0, n1, ne, N, [&](int i) { return srew[i]; });
    mc_store(a.dones, s0, n1, ne, N, [&](int i) { return sadn[i]; });
    mc_store(a.dones_env, s0, n1, ne, 1, [&](int i) { return sdone[i]; });
    mc_store(a.valid, s0, n1, ne, N, [&](int i) { return svalid[i]; });
    if (a.q_out) oc_store(a.q_out, j0 * N * OC_A, nrows * OC_A, [&](int i) { return sq[i]; });
    // ---- auto-reset: the env state is read by observe only, which is behind the barriers on both sides
    if (tid < ne && edone) {
      env.reset(a, tid);
      edone = false;
    }
    lds_sync();
  }
  if (tid < ne) {
    if (a.ret_out) a.ret_out[e0 + tid] = ret;
    if (a.ndone_out) a.ndone_out[e0 + tid] = nd;
  }
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
template <class Env>
int launch_collect(const TileArgs<McIo, typename Env::EnvArgs>& a, int64_t n_envs, hipStream_t s) {
  constexpr int lds = Env::L::bytes;
  static const hipError_t set_lds_attribute =
      hipFuncSetAttribute((const void*)moffq_collect_kernel<Env>, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
  MM_HIP_CHECK(set_lds_attribute);
  const unsigned nb = (unsigned)((n_envs + a.EB - 1) / a.EB);
  hipLaunchKernelGGL(moffq_collect_kernel<Env>, dim3(nb), dim3(256), lds, s, a);
  MM_HIP_CHECK(hipGetLastError());
  return MM_OK;
}

}  // namespace
}  // namespace mm

extern "C" {

int mm_moffq_collect_supported(const mm_env* env, const mm_offq_dims* d, int64_t n_envs, int32_t T) {
  return mm::collect_check("moffq_collect", env, d, n_envs, T, false) == MM_OK ? 1 : 0;
}

int mm_moffq_collect(mm_env* env, const mm_offq_dims* d, const float* P, const mm_moffq_collect_io* io, int64_t n_envs,
                     int32_t T, mm_stream_t s) {
  using namespace mm;
  int rc = collect_check("moffq_collect", env, d, n_envs, T, true);
  if (rc) return rc;
  const EnvDev& ev = env->d;
  TileArgs<McIo, CheckersEnvArgs> a;
  rc = fill_io(a, "moffq_collect", P, io, n_envs, T, ev.N, ev.max_steps, ev.step_cost);
  if (rc) return rc;
  static_cast<CheckersEnvArgs&>(a) = checkers_env_args(ev);
  return launch_collect<CheckersTileT<McCheckersLds>>(a, n_envs, (hipStream_t)s);
}

int mm_moffq_collect_switch_supported(const mm_switch* env, const mm_offq_dims* d, int64_t n_envs, int32_t T) {
  return mm::collect_switch_check("moffq_collect_switch", env, d, n_envs, T, false) == MM_OK ? 1 : 0;
}

int mm_moffq_collect_switch(mm_switch* env, const mm_offq_dims* d, const float* P, const mm_moffq_collect_io* io,
                            int64_t n_envs, int32_t T, mm_stream_t s) {
  using namespace mm;
  int rc = collect_switch_check("moffq_collect_switch", env, d, n_envs, T, true);
  if (rc) return rc;
  const mm_switch_cfg& c = env->cfg;
  TileArgs<McIo, SwitchEnvArgs> a;
  rc = fill_io(a, "moffq_collect_switch", P, io, n_envs, T, c.n_agents, c.max_steps, c.step_cost);
  if (rc) return rc;
  a.tab = env->tab;
  return launch_collect<SwitchTileT<McSwitchLds>>(a, n_envs, (hipStream_t)s);
}

}  // extern "C"
