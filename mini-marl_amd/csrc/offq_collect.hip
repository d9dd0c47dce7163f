// Offpolicy QMix / VDN episode collector on gfx950: the collect loop of the reference's magym runner
// (offpolicy/runner/shared/magym_runner.py:40-141, one env at a time there) for E lockstep Checkers or Switch envs,
// a whole T-step episode in ONE launch. Episodes of different envs are independent and the AgentQFunction
// (LN(D) -> [Linear, ReLU, LN] x 2 -> GRU(H) -> LN -> Linear(A), agent_q_function.py:24-57) is shared by all
// agents, so a block owns a tile of envs for the whole episode and nothing is handed between blocks.
//
//   block   256 threads = 4 waves; wave w owns the (env, agent) rows 32 w .. 32 w + 31 of the tile's
//           ne N <= 128 rows (ne = min(128 / N, 64) envs). No row ever changes its wave or lane.
//   weights staged once per block into LDS as exact-f32 MFMA A-operand images (v_mfma_f32_32x32x2_f32, the
//           fragment maps of common.h): k-step s of row block rb, lane (i, h) holds W[32 rb + i][col(s, h)],
//           four k-steps per 16-byte piece, so a wave's ds_read_b128 is contiguous. 132 KiB of the 160 KiB LDS;
//           the env tile (nibble-row grids, positions, the step's actions / rewards / observation words) and
//           the per-feature vectors take the next 14 KiB.
//   layers  activations chain through registers: D register s of the producing layer is the B operand of
//           k-step s of the next (kperm). Lane (j, h) holds 32 of row j's 64 features, its partner lane
//           j + 32 the others; a LayerNorm sum is one cross-half shuffle. The GRU hidden state stays in
//           32 registers per lane for all T steps (zero at t = 0, never reset: the reference keeps calling the
//           policy after done).
//   env     one lane per env steps it in LDS, agents in id order, between two barriers of the step.
//   output  every field of a step is one contiguous run per block ([t][e0 .. e0 + ne)[N][X]); the block
//           writes it thread-linear with 16-byte stores (scalar head / tail where the run is not aligned).
//
// offq_collect_kernel<Env> is the one episode loop: row bookkeeping, hidden state, the net from layer 1's bias on, the
// action draw, the barriers and the stores. An env tile gives its argument struct and LDS layout, the staging of the
// reset state, a row's current observation (the record the stores read and LayerNorm 0's output for the net), the env
// lane's step with its private episode state, and where dones[t, e, n] comes from. The tiles, the trunk of the net
// and the stores live in collect_tile.h, shared with the feed-forward transition collector (moffq_collect.hip):
//   CheckersTile  dones[t, e, n] is the env's flag.
//   SwitchTile  dones[t, e, n] is agent n's own done flag, dones_env[t, e] their conjunction.
//
// The env handle's live state is neither read nor written: every env starts from reset (Checkers: the handle's
// init_grid / init_pos tables; Switch: the fixed start cells) and the episode's state lives in LDS only.
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

// what both kernels take: the net, the exploration stream, the episode fields
struct OcIo {
  const float* P;
  const float* eps;
  const unsigned long long* counter;
  uint64_t counter0, seed;
  float *obs, *acts, *rew, *dones, *dones_env, *q_out, *ret_out;
  int E, T, N, EB, max_steps, common;
  float step_cost;
};
using OcArgs = TileArgs<OcIo, CheckersEnvArgs>;
using OsArgs = TileArgs<OcIo, SwitchEnvArgs>;

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
// state in place; Q 0..3 land in registers 0..3 of lane half 0 of the result, Q 4 in register 0 of half 1
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


// The episode loop, for either tile. Per step: observe, [t = T: store the final observation and stop,] net, action
// draw | barrier | env step by the env lanes | barrier | the step's stores | barrier.
template <class Env>
__global__ __launch_bounds__(256) void offq_collect_kernel(TileArgs<OcIo, typename Env::EnvArgs> a) {
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
  Env env{sm};

  // ---- stage the net and the reset state
  oc_stage_net<L, D, KS1>(sm, a.P);
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
  f32x16 hid[2];
#pragma unroll
  for (int r = 0; r < 16; ++r) hid[0][r] = hid[1][r] = 0.0f;

  for (int t = 0; t <= a.T; ++t) {
    float x0[KS1];   // LayerNorm 0's output: this lane's feature 2 s + h
    env.observe(a, row, rrow, rle, owner, h, x0);
    const int64_t rowbase = ((int64_t)t * a.E + e0) * N;   // row (t, e0, 0) of the [.., E, N, X] fields
    auto obs_gen = [&](int i) { return env.obs_elem(i); };
    if (t == a.T) {
      lds_sync();
      oc_store(a.obs, rowbase * D, nrows * D, obs_gen);
      break;
    }

    const f32x16 qa = oc_net<L, KS1>(sm, x0, hid, lane, h);
    oc_act(a.seed, a.q_out != nullptr, qa, owner, row, c0 + (uint64_t)t, rinner, eps, sact, sq);
    lds_sync();

    // ---- env step: one lane per env; a finished env is not stepped
    if (tid < ne) {
      if (!edone) {
        float sum = 0.0f;
        edone = env.step(a, tid, sact, srew, sum);
        if (a.common)
          for (int k = 0; k < N; ++k) srew[tid * N + k] = sum;
      } else {
        for (int k = 0; k < N; ++k) srew[tid * N + k] = 0.0f;
      }
      sdone[tid] = edone ? 1.0f : 0.0f;
      ret += srew[tid * N];
    }
    lds_sync();

    // ---- the step's episode fields
    oc_store(a.obs, rowbase * D, nrows * D, obs_gen);
    oc_store(a.acts, rowbase * OC_A, nrows * OC_A, [&](int i) {
      const int r = i / OC_A;
      return sact[r] == i - r * OC_A ? 1.0f : 0.0f;
    });
    oc_store(a.rew, rowbase, nrows, [&](int i) { return srew[i]; });
    oc_store(a.dones, rowbase, nrows, [&](int i) { return env.agent_done(a, i); });
    oc_store(a.dones_env, (int64_t)t * a.E + e0, ne, [&](int i) { return sdone[i]; });
    if (a.q_out) oc_store(a.q_out, rowbase * OC_A, nrows * OC_A, [&](int i) { return sq[i]; });
    lds_sync();
  }
  if (a.ret_out && tid < ne) a.ret_out[e0 + tid] = ret;
}

// the launch arguments both kernels share; EB = envs of a block's tile
int fill_io(OcIo& a, const char* who, const float* P, const mm_offq_collect_io* io, int64_t n_envs, int32_t T, int N,
            int max_steps, float step_cost) {
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
template <class Env>
int launch_collect(const TileArgs<OcIo, typename Env::EnvArgs>& a, int64_t n_envs, hipStream_t s) {
  constexpr int lds = Env::L::total * 4;
  static const hipError_t set_lds_attribute =
      hipFuncSetAttribute((const void*)offq_collect_kernel<Env>, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
  MM_HIP_CHECK(set_lds_attribute);
  const unsigned nb = (unsigned)((n_envs + a.EB - 1) / a.EB);
  hipLaunchKernelGGL(offq_collect_kernel<Env>, dim3(nb), dim3(256), lds, s, a);
  MM_HIP_CHECK(hipGetLastError());
  return MM_OK;
}

}  // namespace
}  // namespace mm

extern "C" {

int mm_offq_collect_supported(const mm_env* env, const mm_offq_dims* d, int64_t n_envs, int32_t T) {
  return mm::collect_check("offq_collect", env, d, n_envs, T, false) == MM_OK ? 1 : 0;
}

int mm_offq_collect(mm_env* env, const mm_offq_dims* d, const float* P, const mm_offq_collect_io* io, int64_t n_envs,
                    int32_t T, mm_stream_t s) {
  using namespace mm;
  int rc = collect_check("offq_collect", env, d, n_envs, T, true);
  if (rc) return rc;
  const EnvDev& ev = env->d;
  OcArgs a;
  rc = fill_io(a, "offq_collect", P, io, n_envs, T, ev.N, ev.max_steps, ev.step_cost);
  if (rc) return rc;
  static_cast<CheckersEnvArgs&>(a) = checkers_env_args(ev);
  return launch_collect<CheckersTile>(a, n_envs, (hipStream_t)s);
}

int mm_offq_collect_switch_supported(const mm_switch* env, const mm_offq_dims* d, int64_t n_envs, int32_t T) {
  return mm::collect_switch_check("offq_collect_switch", env, d, n_envs, T, false) == MM_OK ? 1 : 0;
}

int mm_offq_collect_switch(mm_switch* env, const mm_offq_dims* d, const float* P, const mm_offq_collect_io* io,
                           int64_t n_envs, int32_t T, mm_stream_t s) {
  using namespace mm;
  int rc = collect_switch_check("offq_collect_switch", env, d, n_envs, T, true);
  if (rc) return rc;
  const mm_switch_cfg& c = env->cfg;
  OsArgs a;
  rc = fill_io(a, "offq_collect_switch", P, io, n_envs, T, c.n_agents, c.max_steps, c.step_cost);
  if (rc) return rc;
  a.tab = env->tab;
  return launch_collect<SwitchTile>(a, n_envs, (hipStream_t)s);
}

}  // extern "C"
