// Episode collector of offpolicy rmaddpg / rmatd3 on gfx950: the collect loop of the reference's magym runner
// (offpolicy/runner/shared/magym_runner.py:40-141) with R_MADDPGPolicy.get_actions' discrete exploration
// (algorithm/rMADDPGPolicy.py:62-133, non-multidiscrete branch, prev_act_inp off) for E lockstep Checkers or Switch envs,
// a whole T-step episode from reset in ONE launch, written in the insert layout of offq_collect.hip. Block shape, env
// tiles, LDS layout, the staged GRU net and its step are those of offq_collect.hip (collect_tile.h, collect_gru.h); the
// action rule is that of maddpg_collect.hip (collect_gumbel.h). What is this kernel's own is how the two meet.
//
//   block   256 threads = 4 waves; wave w owns the (env, agent) rows 32 w .. 32 w + 31 of the tile's ne N <= 128 rows
//           (ne = min(128 / N, 64) envs); one block per CU (the weight images take 132 KiB of the 160 KiB LDS).
//   net     the actor LN(D) -> [Linear, ReLU, LN] x 2 -> GRU(64) -> LN -> Linear(A) in the MGeo<D, 64, 5> layout, staged
//           once per block as exact-f32 v_mfma_f32_32x32x2_f32 A-operand images; activations chain through registers and
//           the hidden state stays in 32 registers per lane for all T steps (zero at t = 0, never reset: the reference
//           keeps calling the policy after done).
//   action  explore: a = argmax_k (logit_k + g_k), first maximum, g_k = rng_gumbel(rng_draw(gumbel_seed, ctr, e, n A + k)),
//           ctr = counter + t: bit for bit what mm_maddpg_gumbel(B = E, gumbel_seed, ctr) leaves at g[n][e][k]. Where
//           u < eps the action is the uniform one; u and it come from the two streams of oc_act (seed, seed ^ 0x5bd1e995,
//           (e, n), ctr). No explore: the first maximum of the logits, no noise, eps ignored.
//   noise   a step needs nrows A <= 640 Gumbel draws, each two f64 logs, none of which depends on env state or on the
//           hidden state. The env phase occupies only the env lanes of wave 0 (tid < ne <= 64): waves 1..3 make the draws
//           of step t + 1 there, thread-linear over their 192 lanes, into the tile's q slot [rows][A]. The action phase of
//           step t + 1 reads it; step t's noise was consumed in front of the barrier that opens the env phase. Step 0's
//           draws are made by all threads while the net is staged.
//   logits  q_out (optional) is written by the row's owner lane from registers in the action phase, since the q slot
//           holds noise: no LDS beyond the tile of offq_collect.hip.
//   warm-up explore && eps >= 1 && no q_out: every action is the uniform one and the hidden state reaches nothing that is
//           stored, so the (block-uniform) branch skips the staging of the net, the net and the noise for the whole
//           episode: such a collect costs the env loop and the stores. With q_out the net runs, the noise is still
//           skipped, and the stored fields are the same bits.
//   step t  observe -> net -> action | barrier | wave 0: env lanes step; waves 1..3: noise of t + 1 | barrier | stores |
//           barrier. t = T: the final observation only. Wave 0's env lanes stay the critical path of the second phase;
//           nothing of step t + 1's net is moved there.
#include "collect_gru.h"
#include "collect_gumbel.h"

namespace mm {
namespace {

static_assert(OcLds::total * 4 <= 160 * 1024 && OsLds::total * 4 <= 160 * 1024, "LDS budget: one block per CU");
static_assert(OcLds::q + OC_ROWS * OC_A <= OcLds::total && OsLds::q + OC_ROWS * OC_A <= OsLds::total, "noise slot");

struct RmcIo : OcIo {
  uint64_t gumbel_seed;
  int explore;
};

template <class Env>
__global__ __launch_bounds__(256) void rmaddpg_collect_kernel(TileArgs<RmcIo, typename Env::EnvArgs> a) {
  using L = typename Env::L;
  constexpr int D = Env::D, KS1 = Env::KS1;
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5;
  const int N = a.N;
  const int e0 = blockIdx.x * a.EB, ne = min(a.EB, a.E - e0), nrows = ne * N;
  int* sact = reinterpret_cast<int*>(sm + L::act);
  float* srew = sm + L::rew;
  float* sg = sm + L::q;   // [rows][A] the Gumbel noise of the coming action phase
  float* sdone = sm + L::done;
  Env env{sm};
  const float eps = *a.eps;
  const uint64_t c0 = a.counter ? (uint64_t)*a.counter : a.counter0;
  const bool noisy = a.explore && eps < 1.0f;
  const bool warm = a.explore && eps >= 1.0f && a.q_out == nullptr;   // nothing stored depends on the net

  // ---- stage the net and the reset state; step 0's noise by all threads (env.stage ends behind a barrier)
  if (!warm) oc_stage_net<L, D, KS1>(sm, a.P);
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
  f32x16 hid[2];
#pragma unroll
  for (int r = 0; r < 16; ++r) hid[0][r] = hid[1][r] = 0.0f;

  for (int t = 0; t <= a.T; ++t) {
    float x0[KS1];   // LayerNorm 0's output: this lane's feature 2 s + h (unused in a warm-up episode)
    env.observe(a, row, rrow, rle, owner, h, x0);
    const int64_t rowbase = ((int64_t)t * a.E + e0) * N;   // row (t, e0, 0) of the [.., E, N, X] fields
    auto obs_gen = [&](int i) { return env.obs_elem(i); };
    if (t == a.T) {
      lds_sync();
      oc_store(a.obs, rowbase * D, nrows * D, obs_gen);
      break;
    }

    // ---- net, action (the logits go out from the owner lane's registers)
    f32x16 qa;
#pragma unroll
    for (int r = 0; r < 16; ++r) qa[r] = 0.0f;
    if (!warm) qa = oc_net<L, KS1>(sm, x0, hid, lane, h);
    mdc_act(a, qa, owner, row, c0 + (uint64_t)t, rinner, eps, noisy, sg, sact,
            a.q_out ? a.q_out + rowbase * OC_A : nullptr);
    lds_sync();

    // ---- env step on the env lanes of wave 0 (a finished env is not stepped); the other waves make the next step's
    // noise meanwhile
    if (wave == 0) {
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
    } else if (noisy && t + 1 < a.T) {
      mdc_noise(sg, a.gumbel_seed, c0 + (uint64_t)(t + 1), e0, N * OC_A, nrows * OC_A, tid - 64, 192);
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
    lds_sync();
  }
  if (a.ret_out && tid < ne) a.ret_out[e0 + tid] = ret;
}

int fill_rmc(RmcIo& a, const char* who, const float* PA, const mm_rmaddpg_collect_io* io, int64_t n_envs, int32_t T, int N,
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

int mm_rmaddpg_collect_supported(const mm_env* env, const mm_maddpg_dims* d, int64_t n_envs, int32_t T) {
  return mm::check_checkers("rmaddpg_collect", env, d, n_envs, T, false) == MM_OK ? 1 : 0;
}

int mm_rmaddpg_collect(mm_env* env, const mm_maddpg_dims* d, const float* PA, const mm_rmaddpg_collect_io* io,
                       int64_t n_envs, int32_t T, mm_stream_t s) {
  using namespace mm;
  int rc = check_checkers("rmaddpg_collect", env, d, n_envs, T, true);
  if (rc) return rc;
  const EnvDev& ev = env->d;
  TileArgs<RmcIo, CheckersEnvArgs> a;
  rc = fill_rmc(a, "rmaddpg_collect", PA, io, n_envs, T, ev.N, ev.max_steps, ev.step_cost);
  if (rc) return rc;
  static_cast<CheckersEnvArgs&>(a) = checkers_env_args(ev);
  return launch_episode<CheckersTile, rmaddpg_collect_kernel<CheckersTile>>(a, n_envs, (hipStream_t)s);
}

int mm_rmaddpg_collect_switch_supported(const mm_switch* env, const mm_maddpg_dims* d, int64_t n_envs, int32_t T) {
  return mm::check_switch("rmaddpg_collect_switch", env, d, n_envs, T, false) == MM_OK ? 1 : 0;
}

int mm_rmaddpg_collect_switch(mm_switch* env, const mm_maddpg_dims* d, const float* PA, const mm_rmaddpg_collect_io* io,
                              int64_t n_envs, int32_t T, mm_stream_t s) {
  using namespace mm;
  int rc = check_switch("rmaddpg_collect_switch", env, d, n_envs, T, true);
  if (rc) return rc;
  const mm_switch_cfg& c = env->cfg;
  TileArgs<RmcIo, SwitchEnvArgs> a;
  rc = fill_rmc(a, "rmaddpg_collect_switch", PA, io, n_envs, T, c.n_agents, c.max_steps, c.step_cost);
  if (rc) return rc;
  a.tab = env->tab;
  return launch_episode<SwitchTile, rmaddpg_collect_kernel<SwitchTile>>(a, n_envs, (hipStream_t)s);
}

}  // extern "C"
