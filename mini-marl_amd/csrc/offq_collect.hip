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
// and the stores live in collect_tile.h, shared with the feed-forward transition collectors; the staged GRU net, the
// launch arguments and the launch in collect_gru.h, shared with the episode collector of rmaddpg / rmatd3
// (rmaddpg_collect.hip):
//   CheckersTile  dones[t, e, n] is the env's flag.
//   SwitchTile  dones[t, e, n] is agent n's own done flag, dones_env[t, e] their conjunction.
//
// The env handle's live state is neither read nor written: every env starts from reset (Checkers: the handle's
// init_grid / init_pos tables; Switch: the fixed start cells) and the episode's state lives in LDS only.
#include "collect_gru.h"

namespace mm {
namespace {

using OcArgs = TileArgs<OcIo, CheckersEnvArgs>;
using OsArgs = TileArgs<OcIo, SwitchEnvArgs>;

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
  return launch_episode<CheckersTile, offq_collect_kernel<CheckersTile>>(a, n_envs, (hipStream_t)s);
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
  return launch_episode<SwitchTile, offq_collect_kernel<SwitchTile>>(a, n_envs, (hipStream_t)s);
}

}  // extern "C"
