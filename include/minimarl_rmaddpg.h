/*
 * minimarl - the recurrent MADDPG / MATD3 trainer ("rmaddpg" / "rmatd3") of the offpolicy fork (csrc/rmaddpg.hip). Part
 * of the C ABI of minimarl.h, which includes this file: include either.
 *
 * Replaces R_MADDPG.shared_train_policy_on_batch (offpolicy/algorithms/r_maddpg/r_maddpg.py:114-331; R_MATD3 is the
 * same class) with R_MADDPGPolicy (algorithm/rMADDPGPolicy.py) for discrete actions and one shared policy.
 *   actor:  RNNBase(D) -> ACTLayer(A): the 18-tensor trunk layout of mm_offq_* (mm_maddpg_dims, MGeo<D, 64, A>).
 *   critic: RNNBase(Dc) over [cent_obs | cent_act], Dc = N (D + A) <= MM_MADDPG_MAX_CRITIC_WIDTH, the same layout with
 *           W1 rows padded to ceil4(Dc) and nq = 1 (rmaddpg) or 2 (td3) Linear(64, 1) heads in a 4-row Wo / bo slot.
 *           The heads are parameters here (q_outs is an nn.ModuleList): they are trained and part of the norm.
 * Batch = RecReplayBuffer.sample layout: obs [N, T+1, B, D], share_obs [T+1, B, N D], acts one-hot [N, T, B, A],
 * rewards [N, T, B] (agent 0's are used), dones [N, T, B], dones_env [T, B], is_weight [B] (NULL: no PER),
 * gumbel / target_gumbel [N, T, B, A] (actor pass: obs step t; target actions of td3: obs step t + 1;
 * mm_maddpg_gumbel with B := T B fills one). All sequences start from h = 0.
 * One update = mm_rmaddpg_critic_grad, mm_clip_adam on the critic, mm_rmaddpg_actor_grad (reads the UPDATED critic),
 * mm_clip_adam on the actor. No host sync, no host loop over t; same inputs give the same bits (no float atomics).
 * Supported: H = 64, A = 5, D in {3, 47, 94}, N >= 1, T >= 1, B >= 1; anything else MM_EINVAL (-1 from the size
 * query) before any launch.
 */
#ifndef MINIMARL_RMADDPG_H
#define MINIMARL_RMADDPG_H
#include "minimarl.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mm_rmaddpg_batch {
  const float* obs; const float* share_obs; const float* acts; const float* rewards; const float* dones;
  const float* dones_env; const float* is_weight; const float* gumbel; const float* target_gumbel;
  int32_t T, B, huber;
  float gamma, huber_delta, per_eps, per_nu;
} mm_rmaddpg_batch;

int mm_rmaddpg_param_counts(const mm_maddpg_dims* d, int64_t* actor, int64_t* critic);
int64_t mm_rmaddpg_workspace_bytes(const mm_maddpg_dims* d, int32_t T, int32_t B);
/* Critic pass. Target actions: the target actor over all T + 1 obs steps, step t + 1 gives nact[t] (logits == rowmax,
 * or with td3 the one-hot argmax of logits + target_gumbel). Target critic: its state follows the stored
 * x_t = [share_obs[t] | acts[:, t]]; a side cell on [share_obs[t + 1] | nact[t]] from h_t gives min_k q'_t,k.
 * target = (r + gamma (1 - done_env) min q') (1 - curr), curr[t] = done_env[t - 1] (0 at t = 0); err_k = Q_k (1 - curr)
 * - target; loss = sum_k sum w_b f(err_k) / sum (1 - curr), f = e^2 or Huber; priorities (PER only) = mean_k ((1 - nu)
 * mean_t |err_k| + nu max_t |err_k| + per_eps) + per_eps. grad: the critic layout, heads included; stats float[2] =
 * {loss, sum (1 - curr)}. ws: mm_rmaddpg_workspace_bytes(d, T, B), needs no initialisation. */
int mm_rmaddpg_critic_grad(const mm_maddpg_dims* d, const mm_rmaddpg_batch* b, const float* PA_target, const float* PC,
                           const float* PC_target, float* grad, void* ws, int64_t ws_bytes, float* stats,
                           float* priorities, mm_stream_t s);
/* Actor pass: y = softmax(logits + gumbel) of the actor over obs steps 0 .. T - 1, hard = one-hot argmax; the critic's
 * state follows the stored x_t; for each agent i a side cell from h_{t-1} on x_t with agent i's columns replaced by
 * hard_i,t gives Q^i_t (head 0); loss = -sum Q^i_t (1 - acurr_i[t]) / sum (1 - acurr); the gradient reaches the actor
 * straight through (d hard := d y), then by BPTT. grad: the actor layout; stats float[2] = {loss, sum (1 - acurr)}. */
int mm_rmaddpg_actor_grad(const mm_maddpg_dims* d, const mm_rmaddpg_batch* b, const float* PA, const float* PC,
                          float* grad, void* ws, int64_t ws_bytes, float* stats, mm_stream_t s);
/* One actor step: obs [R, D], h_in [R, 64] (NULL: zeros) -> logits [R, 8] (columns 0 .. A - 1; the rest zero),
 * h_out [R, 64], onehot [R, A] (may be NULL: the argmax of logits + gumbel [R, A], or logits == rowmax without gumbel).
 * scratch: 192 R floats. */
int mm_rmaddpg_step(const mm_maddpg_dims* d, const float* PA, const float* obs, const float* h_in, const float* gumbel,
                    float* logits, float* onehot, float* h_out, float* scratch, int64_t R, mm_stream_t s);

#ifdef __cplusplus
}
#endif
#endif
