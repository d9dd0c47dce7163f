// MAPPO per-row loss arithmetic shared by the per-thread path (mappo.hip) and the MFMA passes (mappo_grad.hip):
// Categorical log-softmax, the PPO / clipped-Huber loss seeds d loss / d out (ramppo_network.py:56-209, ppo_update and
// cal_value_loss) and the flush of the logged loss sums. Plain per-row code: a caller brings its row's logits or
// saved log-probs, masks its own tail lanes and adds the logging terms its own way.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "minimarl.h"

namespace mm {

// log-softmax in place (logits -> logp), returns entropy
template <int A>
__device__ __forceinline__ float log_softmax(float (&l)[A]) {
  float mx = l[0];
#pragma unroll
  for (int a = 1; a < A; ++a) mx = fmaxf(mx, l[a]);
  float s = 0.0f;
#pragma unroll
  for (int a = 0; a < A; ++a) s += expf(l[a] - mx);
  const float lse = mx + logf(s);
  float ent = 0.0f;
#pragma unroll
  for (int a = 0; a < A; ++a) {
    l[a] -= lse;
    ent -= expf(l[a]) * l[a];
  }
  return ent;
}

__device__ __forceinline__ float huber_d(float e, float d) { return fabsf(e) <= d ? e : (e > 0.f ? d : -d); }
__device__ __forceinline__ float huber_f(float e, float d) {
  return fabsf(e) <= d ? e * e * 0.5f : d * (fabsf(e) - d * 0.5f);
}

// the three logged terms of a policy row (train_info): surrogate loss and entropy, both x active, and the ratio
struct PolicyTerms {
  float loss, ent, ratio;
};

// Policy seed of buffer row `row` (active flag m, inv_m = 1 / active count) from its log-probs lp and entropy ent:
// dout = d loss / d logits of the clipped surrogate + entropy bonus
template <int A>
__device__ __forceinline__ PolicyTerms policy_seed(const mm_mappo_bwd_args& a, int64_t row, float m, float inv_m,
                                                   const float (&lp)[A], float ent, float (&dout)[A]) {
  const int act = a.act[row];
  float lpa = lp[0];
#pragma unroll
  for (int q = 1; q < A; ++q)
    if (q == act) lpa = lp[q];
  const float adv = (a.adv[row] - a.stats[MM_MST_ADV_MEAN]) / (a.stats[MM_MST_ADV_STD] + 1e-5f);
  const float ratio = expf(lpa - a.old_logp[row]);
  const float s1 = ratio * adv;
  const float rc = fminf(fmaxf(ratio, 1.0f - a.clip), 1.0f + a.clip);
  const float s2 = rc * adv;
  const float inr = (ratio >= 1.0f - a.clip && ratio <= 1.0f + a.clip) ? 1.0f : 0.0f;
  // torch.min backward: the smaller side gets the gradient, ties split it in half
  const float g = s1 < s2 ? 1.0f : (s1 > s2 ? inr : 0.5f + 0.5f * inr);
  const float dlpa = -m * inv_m * adv * ratio * g;
  const float dent = -a.entropy_coef * m * inv_m;
#pragma unroll
  for (int q = 0; q < A; ++q) {
    const float p = expf(lp[q]);
    dout[q] = dlpa * ((q == act ? 1.0f : 0.0f) - p) + dent * (-p * (lp[q] + ent));
  }
  return {-fminf(s1, s2) * m, ent * m, ratio};
}

// Value seed of buffer row `row` from its value v: dout = d loss / d v of the ValueNorm-targeted clipped Huber loss;
// returns the logged loss term (x active)
__device__ __forceinline__ float value_seed(const mm_mappo_bwd_args& a, int64_t row, float m, float inv_m, float v,
                                            float& dout) {
  const float old = a.old_value[row];
  const float tgt = (a.returns[row] - a.stats[MM_MST_VN_MEAN]) / a.stats[MM_MST_VN_STD];
  const float dv = v - old;
  const float vc = old + fminf(fmaxf(dv, -a.clip), a.clip);
  const float eo = tgt - v, ec = tgt - vc;
  const float lo = huber_f(eo, a.huber_delta), lc = huber_f(ec, a.huber_delta);
  const float go = -huber_d(eo, a.huber_delta);
  const float gc = -huber_d(ec, a.huber_delta) * ((dv >= -a.clip && dv <= a.clip) ? 1.0f : 0.0f);
  const float d = lo > lc ? go : (lc > lo ? gc : 0.5f * (go + gc));
  dout = a.value_coef * m * inv_m * d;
  return fmaxf(lo, lc) * m;
}

// Loss sums (logging only, train_info): wave-level sums, one atomic per wave. POLICY: surrogate, entropy and ratio
// sums, else the value loss in lsum0.
template <bool POLICY>
__device__ __forceinline__ void loss_flush(float* loss_acc, float lsum0, float lsum1, float lsum2, float inv_m) {
  if (!loss_acc) return;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    lsum0 += __shfl_xor(lsum0, o);
    lsum1 += __shfl_xor(lsum1, o);
    lsum2 += __shfl_xor(lsum2, o);
  }
  if ((threadIdx.x & 63) == 0) {
    if constexpr (POLICY) {
      atomicAdd(&loss_acc[MM_MLOSS_POLICY], lsum0 * inv_m);
      atomicAdd(&loss_acc[MM_MLOSS_ENTROPY], lsum1 * inv_m);
      atomicAdd(&loss_acc[MM_MLOSS_RATIO], lsum2);
    } else {
      atomicAdd(&loss_acc[MM_MLOSS_VALUE], lsum0 * inv_m);
    }
  }
}

}  // namespace mm
