// Transition collector of offpolicy maddpg / matd3 on gfx950: the collect loop of the reference's MLP runner
// (collecter, offpolicy/runner/shared/magym_runner.py) with MADDPGPolicy.get_actions' discrete exploration
// (algorithm/MADDPGPolicy.py:95-104) for E lockstep Checkers or Switch envs, a window of T steps from reset in ONE
// launch, written as T E single transitions with reset-on-done inside the window. Window, fields, ring stores and env
// tiles are those of moffq_collect.hip (collect_window.h); what differs is the action rule (collect_gumbel.h, shared with
// the episode collector of rmaddpg / rmatd3) and where its noise is made.
//
//   net     the actor of maddpg.hip, LN(D) -> [Linear, ReLU, LN] x 2 -> Linear(A), in the MGeo<D, 64, 5> trunk layout:
//           staged and evaluated by the exact-f32 v_mfma_f32_32x32x2_f32 fragment scheme of collect_tile.h (oc_stage_trunk,
//           oc_trunk, oc_head). 256 threads, 128 (env, agent) rows, three blocks per CU.
//   action  explore: a = argmax_k (logit_k + g_k), first maximum, g_k = rng_gumbel(rng_draw(gumbel_seed, ctr, e, n A + k)),
//           ctr = counter + t: bit for bit what mm_maddpg_gumbel(B = E, gumbel_seed, ctr) leaves at g[n][e][k]. Where
//           u < eps the action is the uniform one; u and it come from the two streams of oc_act (seed, seed ^ 0x5bd1e995,
//           (e, n), ctr). No explore: the first maximum of the logits (onehot_from_logits is multi-hot on an exact tie),
//           no noise, eps ignored.
//   noise   a step needs nrows A <= 640 Gumbel draws, each two f64 logs, and none depends on env state. The env phase of
//           a step occupies only the env lanes of wave 0 (tid < ne <= 64) while waves 1..3 would wait at the barrier: they
//           make the draws of step t + 1 there, thread-linear over the 192 lanes, into ONE LDS slot [rows][A]. The action
//           phase of step t + 1 reads it; step t's noise was consumed before the barrier in front of the env phase that
//           overwrites it. Step 0's draws are made by all threads while the net is staged. No draws without explore or
//           when the block-uniform eps >= 1 (warm-up windows: every action is the uniform one).
//   LDS     the noise takes the tile's q slot [rows][A] (a fourth 640-float slot would not fit three blocks per CU on
//           Checkers: 3 x 52928 B of 163840); the optional q_out (the logits, a test / debug output) is written by the
//           row's owner lane from registers in the action phase.
//   step t  observe (record 0) -> net -> action | barrier | wave 0: env lanes step; waves 1..3: noise of t + 1 | barrier |
//           observe again (record 1 = next_obs) | barrier | stores; env lanes of done envs reset them | barrier.
//           Every row observes twice a step; reusing record 1 as the next step's record 0 for envs that did not reset
//           is left undone.
#include "collect_gumbel.h"
#include "collect_window.h"

namespace mm {
namespace {

struct MdcIo : McIo {
  uint64_t gumbel_seed;
  int explore;
};

// (launch bounds: 3 waves per SIMD = three resident blocks per CU, which caps the kernel at 168 registers)
template <class Env>
__global__ __launch_bounds__(256, 3) void maddpg_collect_kernel(TileArgs<MdcIo, typename Env::EnvArgs> a) {
  using L = typename Env::L;
  constexpr int D = Env::D, KS1 = Env::KS1;
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5;
  const int N = a.N;
  const int e0 = blockIdx.x * a.EB, ne = min(a.EB, a.E - e0), nrows = ne * N;
  int* sact = reinterpret_cast<int*>(sm + L::act);
  float* sg = sm + L::q;   // [rows][A] the Gumbel noise of the coming action phase
  Env env{sm};
  const float eps = *a.eps;
  const uint64_t c0 = a.counter ? (uint64_t)*a.counter : a.counter0;
  const bool noisy = a.explore && eps < 1.0f;

  // ---- stage the net and the reset state; step 0's noise by all threads (env.stage ends behind a barrier)
  oc_stage_trunk<L, D, KS1>(sm, a.P);
  if (noisy) mdc_noise(sg, a.gumbel_seed, c0, e0, N * OC_A, nrows * OC_A, tid, 256);
  env.stage(a, ne, nrows);

  // this lane's row of the tile (both lane halves of a row compute its scalars redundantly)
  const int row = wave * 32 + (lane & 31);
  const bool valid = row < nrows;
  const int rle = valid ? row / N : 0, rn = valid ? row - rle * N : 0, rrow = valid ? row : 0;
  const bool owner = valid && h == 0;
  const uint64_t rinner = rng_inner((uint64_t)(e0 + rle), (uint64_t)rn);
  bool edone = false;   // the env lane's (lane tid < ne owns env e0 + tid)
  float ret = 0.0f;
  int nd = 0;

  for (int t = 0; t < a.T; ++t) {
    // ---- obs, net, action (the logits go out from the owner lane's registers)
    {
      float x0[KS1];   // LayerNorm 0's output: this lane's feature 2 s + h
      env.observe(a, row, rrow, rle, owner, h, x0);
      f32x16 f2[2];
      oc_trunk<L, KS1>(sm, x0, f2, lane, h);
      const f32x16 qa = oc_head<L>(sm, f2, lane, h);
      float* lg = a.q_out ? a.q_out + ((int64_t)t * a.E + e0) * N * OC_A : nullptr;
      mdc_act(a, qa, owner, row, c0 + (uint64_t)t, rinner, eps, noisy, sg, sact, lg);
    }
    lds_sync();

    // ---- env step on the env lanes of wave 0; the other waves make the next step's noise meanwhile
    if (wave == 0) {
      if (tid < ne) edone = mc_env_step(env, a, sm, tid, ret, nd);
    } else if (noisy && t + 1 < a.T) {
      mdc_noise(sg, a.gumbel_seed, c0 + (uint64_t)(t + 1), e0, N * OC_A, nrows * OC_A, tid - 64, 192);
    }
    lds_sync();

    // ---- next_obs: the state after the step, into record 1
    {
      float xn[KS1];
      env.observe(a, row + OC_ROWS, rrow, rle, owner, h, xn);
    }
    lds_sync();

    // ---- the step's transitions
    mc_store_step(env, a, sm, t, e0, ne);
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

int fill_mdc(MdcIo& a, const char* who, const float* PA, const mm_maddpg_collect_io* io, int64_t n_envs, int32_t T, int N,
             int max_steps, float step_cost) {
  const int rc = fill_io(a, who, PA, io ? &io->w : nullptr, n_envs, T, N, max_steps, step_cost);
  if (rc) return rc;
  a.gumbel_seed = io->gumbel_seed;
  a.explore = io->explore ? 1 : 0;
  return MM_OK;
}

}  // namespace
}  // namespace mm

extern "C" {

int mm_maddpg_collect_supported(const mm_env* env, const mm_maddpg_dims* d, int64_t n_envs, int32_t T) {
  return mm::check_checkers("maddpg_collect", env, d, n_envs, T, false) == MM_OK ? 1 : 0;
}

int mm_maddpg_collect(mm_env* env, const mm_maddpg_dims* d, const float* PA, const mm_maddpg_collect_io* io,
                      int64_t n_envs, int32_t T, mm_stream_t s) {
  using namespace mm;
  int rc = check_checkers("maddpg_collect", env, d, n_envs, T, true);
  if (rc) return rc;
  const EnvDev& ev = env->d;
  TileArgs<MdcIo, CheckersEnvArgs> a;
  rc = fill_mdc(a, "maddpg_collect", PA, io, n_envs, T, ev.N, ev.max_steps, ev.step_cost);
  if (rc) return rc;
  static_cast<CheckersEnvArgs&>(a) = checkers_env_args(ev);
  using Env = CheckersTileT<McCheckersLds>;
  return launch_collect<Env, maddpg_collect_kernel<Env>>(a, n_envs, (hipStream_t)s);
}

int mm_maddpg_collect_switch_supported(const mm_switch* env, const mm_maddpg_dims* d, int64_t n_envs, int32_t T) {
  return mm::check_switch("maddpg_collect_switch", env, d, n_envs, T, false) == MM_OK ? 1 : 0;
}

int mm_maddpg_collect_switch(mm_switch* env, const mm_maddpg_dims* d, const float* PA, const mm_maddpg_collect_io* io,
                             int64_t n_envs, int32_t T, mm_stream_t s) {
  using namespace mm;
  int rc = check_switch("maddpg_collect_switch", env, d, n_envs, T, true);
  if (rc) return rc;
  const mm_switch_cfg& c = env->cfg;
  TileArgs<MdcIo, SwitchEnvArgs> a;
  rc = fill_mdc(a, "maddpg_collect_switch", PA, io, n_envs, T, c.n_agents, c.max_steps, c.step_cost);
  if (rc) return rc;
  a.tab = env->tab;
  using Env = SwitchTileT<McSwitchLds>;
  return launch_collect<Env, maddpg_collect_kernel<Env>>(a, n_envs, (hipStream_t)s);
}

}  // extern "C"
