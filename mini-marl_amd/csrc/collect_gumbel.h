// What the actor collectors share (maddpg_collect.hip: the feed-forward actor of maddpg / matd3, transitions;
// rmaddpg_collect.hip: the GRU actor of rmaddpg / rmatd3, episodes) on top of collect_tile.h: the discrete exploration of
// the policies' get_actions (hard Gumbel-softmax sample of the logits, or the uniform action where u < eps), the Gumbel
// draws of a tile's step, and the argument checks on mm_maddpg_dims (the collectors' checks on the actor's dims, then the
// trainers' critic-width limit).
#pragma once
#include "collect_tile.h"

namespace mm {
namespace {

// sg[i] = the Gumbel draw of tile row i / A, action i % A at step counter ctr, for i = i0, i0 + stride, .. < NA ne
// (NA = N A: row i / A is agent (i % NA) / A of env e0 + i / NA, so the draw's second index n A + k is i % NA)
__device__ __forceinline__ void mdc_noise(float* sg, uint64_t gseed, uint64_t ctr, int e0, int NA, int n, int i0,
                                          int stride) {
  for (int i = i0; i < n; i += stride) {
    const int le = i / NA;
    sg[i] = rng_gumbel(rng_draw(gseed, ctr, (uint64_t)(e0 + le), (uint64_t)(i - le * NA)));
  }
}

// The action of a row from the head's result (every lane calls it; the row's owner lane writes): the first maximum of
// logits (+ sg[row][A] when noisy), or with explore the counter RNG's action where u < eps (the two streams of oc_act
// under a.seed; a.explore says whether). sact[row] gets the action, lg[row][A] (global, may be null) the logits
template <class Io>
__device__ __forceinline__ void mdc_act(const Io& a, f32x16 qa, bool owner, int row, uint64_t ctr, uint64_t rinner,
                                        float eps, bool noisy, const float* sg, int* sact, float* lg) {
  const float q4 = __shfl_xor(qa[0], 32);
  if (owner) {
    const float qv[OC_A] = {qa[0], qa[1], qa[2], qa[3], q4};
    int g = 0;
    float best = noisy ? qv[0] + sg[row * OC_A] : qv[0];
#pragma unroll
    for (int k = 1; k < OC_A; ++k) {
      const float z = noisy ? qv[k] + sg[row * OC_A + k] : qv[k];
      if (z > best) {
        best = z;
        g = k;
      }
    }
    if (a.explore) {
      const float u = rng_uniform(rng_draw_inner(a.seed, ctr, rinner));
      const int ra = (int)rng_mod_small(rng_draw_inner(a.seed ^ 0x5bd1e995ull, ctr, rinner), OC_A);
      g = u < eps ? ra : g;
    }
    sact[row] = g;
    if (lg) {
#pragma unroll
      for (int k = 0; k < OC_A; ++k) lg[row * OC_A + k] = qv[k];
    }
  }
}

// ---- host side: the collectors' checks on the actor's dims, then the trainer's critic-width limit
inline mm_offq_dims actor_dims(const mm_maddpg_dims* d) {
  mm_offq_dims o = {};
  if (d) {
    o.n_agents = d->n_agents;
    o.obs_dim = d->obs_dim;
    o.hidden = d->hidden;
    o.n_actions = d->n_actions;
  }
  return o;
}

inline int width_check(const char* who, const mm_offq_dims& o, int64_t E, int32_t T, bool rep) {
  const bool wide = (int64_t)o.n_agents * (o.obs_dim + o.n_actions) > MM_MADDPG_MAX_CRITIC_WIDTH;
  return report(who, wide ? "the critic input width N (D + A) is above MM_MADDPG_MAX_CRITIC_WIDTH" : nullptr, &o, E, T,
                rep);
}

inline int check_checkers(const char* who, const mm_env* env, const mm_maddpg_dims* d, int64_t E, int32_t T, bool rep) {
  const mm_offq_dims o = actor_dims(d);
  const int rc = collect_check(who, env, d ? &o : nullptr, E, T, rep);
  return rc ? rc : width_check(who, o, E, T, rep);
}

inline int check_switch(const char* who, const mm_switch* env, const mm_maddpg_dims* d, int64_t E, int32_t T, bool rep) {
  const mm_offq_dims o = actor_dims(d);
  const int rc = collect_switch_check(who, env, d ? &o : nullptr, E, T, rep);
  return rc ? rc : width_check(who, o, E, T, rep);
}

}  // namespace
}  // namespace mm
