/*
 * minimarl - the one-launch episode collector of offpolicy rmaddpg / rmatd3 (csrc/rmaddpg_collect.hip). Part of the C ABI
 * of minimarl.h, which includes this file: include either. The trainer's entry points (mm_rmaddpg_param_counts ..
 * mm_rmaddpg_step) stay in minimarl_rmaddpg.h.
 */
#ifndef MINIMARL_RMADDPG_COLLECT_H
#define MINIMARL_RMADDPG_COLLECT_H
#include "minimarl.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Episode collector for rmaddpg / rmatd3 (csrc/rmaddpg_collect.hip): the episode loop, fields, env tiles and optional
 * outputs of mm_offq_collect (w: its io struct, same meanings; q_out holds the actor's logits), run with the recurrent
 * actor PA of mm_rmaddpg_* (hidden zero at t = 0, carried over all T steps, not reset at done; last actions are not an
 * input) and the discrete exploration of R_MADDPGPolicy.get_actions (algorithm/rMADDPGPolicy.py:62-133). Per
 * (env e, agent n) row at step t, ctr = counter + t:
 *   explore != 0: a = argmax_k (logit_k + g_k), first maximum, with g the noise mm_maddpg_gumbel(d, g, B = E,
 *     gumbel_seed, ctr) leaves at g[n][e][k], bit for bit; where u < eps the action is the uniform one instead, u and
 *     that action drawn as by mm_offq_collect (w.seed, per-(env, agent) streams, the same ctr). eps >= 1 draws no noise,
 *     and without q_out does not evaluate the actor either (every stored value is the same with and without it).
 *   explore == 0: the first maximum of the logits; no noise, eps ignored.
 * Supported configurations and error reports: as mm_offq_collect / mm_offq_collect_switch, and
 * N (D + A) <= MM_MADDPG_MAX_CRITIC_WIDTH. Null or unsupported arguments return MM_EINVAL with the reason and launch
 * nothing. The launch does not sync; eps and counter are read from device memory. */
typedef struct mm_rmaddpg_collect_io {
  mm_offq_collect_io w;
  uint64_t gumbel_seed;
  int32_t explore;
} mm_rmaddpg_collect_io;
int mm_rmaddpg_collect_supported(const mm_env* env, const mm_maddpg_dims* d, int64_t n_envs, int32_t T);
int mm_rmaddpg_collect(mm_env* env, const mm_maddpg_dims* d, const float* PA, const mm_rmaddpg_collect_io* io,
                       int64_t n_envs, int32_t T, mm_stream_t s);
int mm_rmaddpg_collect_switch_supported(const mm_switch* env, const mm_maddpg_dims* d, int64_t n_envs, int32_t T);
int mm_rmaddpg_collect_switch(mm_switch* env, const mm_maddpg_dims* d, const float* PA, const mm_rmaddpg_collect_io* io,
                              int64_t n_envs, int32_t T, mm_stream_t s);

#ifdef __cplusplus
}
#endif
#endif
