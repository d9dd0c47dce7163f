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
#include "collect_window.h"

namespace mm {
namespace {

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
  float* sq = sm + L::q;
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
    if (tid < ne) edone = mc_env_step(env, a, sm, tid, ret, nd);
    lds_sync();

    // ---- next_obs: the state after the step, into record 1
    {
      float xn[KS1];
      env.observe(a, row + OC_ROWS, rrow, rle, owner, h, xn);
    }
    lds_sync();

    // ---- the step's transitions
    mc_store_step(env, a, sm, t, e0, ne);
    if (a.q_out) oc_store(a.q_out, ((int64_t)t * a.E + e0) * N * OC_A, nrows * OC_A, [&](int i) { return sq[i]; });
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
  using Env = CheckersTileT<McCheckersLds>;
  return launch_collect<Env, moffq_collect_kernel<Env>>(a, n_envs, (hipStream_t)s);
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
  using Env = SwitchTileT<McSwitchLds>;
  return launch_collect<Env, moffq_collect_kernel<Env>>(a, n_envs, (hipStream_t)s);
}

}  // extern "C"
