// Feed-forward transition-batch QMix / VDN trainer ("mqmix" / "mvdn") of the reference's offpolicy fork on
// gfx950: M_QMix.train_policy_on_batch (offpolicy/algorithms/mqmix/mqmix.py:68-218) with M_QMixPolicy
// (algorithm/mQMixPolicy.py:35-113).
//
//   agent  LN(D) -> Linear(D,H) -> ReLU -> LN(H) -> Linear(H,H) -> ReLU -> LN(H) -> Linear(H,A) (MLPBase with
//          layer_N = 1, use_feature_normalization, ReLU, then ACTLayer's Linear), shared by all agents. Stored in
//          the 18-tensor trunk layout (MGeo) of the recurrent trainer: the six recurrent tensors are not read and
//          get exactly zero gradient, so a checkpoint has the shapes of an OffQMix one.
//   mixer  M_QMixer (mq_mixer.py:80-126; per row the arithmetic of QMixer.forward) or the VDN sum.
//   loss   target = r (agent 0) + (1 - done_env) gamma Q'_tot (target nets; double Q: argmax of the behavior net on
//          nobs), err = Q_tot - target, loss = mean_b w_b f(err_b), f = e^2 or Huber; priorities |err| + per_eps.
//
// Not built (the Python class raises, the C ABI returns MM_EINVAL): use_popart, available-action masks,
// multidiscrete actions, layer_N != 1, hypernet_layers = 1, use_conv1d, weight_decay.
//
// Design. The loss is a plain mean over B, so dL/dQ_tot[b] = w_b f'(err_b) / B needs nothing from other
// transitions: forward, loss and backward of a transition are local to it and only the weight gradients are
// reduced. mm_moffq_loss_grad is TWO launches:
//   1. moffq_train_kernel: a block of 4 waves walks tiles of TB = 16 transitions end to end. Per tile
//        phase 1  for each agent n (a 16-row chunk: row i = transition b0 + i of agent n): behavior net on nobs
//                 (double Q: argmax), target net on nobs, behavior net on obs -> Q(a), next Q;
//        phase 2  both mixers over the tile's 16 transitions, err, priorities, loss and Q_tot sums, dQ_tot,
//                 mixer backward, the tile's mixer weight gradients;
//        phase 3  for each agent n: the behavior forward on obs is RECOMPUTED into LDS (the saves of all N chunks,
//                 8 x 16 rows x 480 floats at N = 8, do not fit next to both nets' weights), then the backward
//                 down to W1 / ln0 and the chunk's weight gradients.
//      Every Linear layer (agent and hypernet, forward and dX) and every weight gradient dW = dY^T X is
//      v_mfma_f32_16x16x4_f32 (exact fp32): 16 rows = one tile, 64 output columns = one 16-column tile per wave.
//      Both agent nets' W1 / W2 / Wo are staged into LDS once per block (odd row strides); agent activations
//      live in LDS only. The hypernet weights (3 Hh S + K S floats in the first layers) stream from L2 as MFMA B
//      operands, cent_obs rows as A operands. The mixer's per-tile intermediates (hypernet outputs, 16 x N K for
//      w1) are not bounded by LDS for N K <= 4096, so they sit in a block-private scratch slice that stays in L2.
//      Each block adds its tiles' weight gradients, in tile order, into a block-private partial [agent | mixer | 2].
//   2. moffq_reduce_kernel: grad[e] = sum over blocks in block order; stats = sums / B. No float atomics anywhere,
//      the grid is a function of B alone: two runs give the same bits.
// mm_moffq_q_values is one launch of the same forward (one net staged) over tiles of 16 rows.
//
// The mixer row math (|w1|, ELU, |w2| and their derivatives) is a second copy of offq.hip's: there it is spread over
// lanes of whole kernels that read [T*B]-row arrays, here it runs on a 16-row tile between MFMA calls.
#include <algorithm>

#include "common.h"
#include "minimarl.h"
#include "mq_tile.h"

namespace mm {
namespace {

constexpr int MQ_MAX_BLOCKS = 256;  // one block per CU; also bounds the partials
constexpr int MQ_Q_BLOCKS = 256;

// Forward of one net over a 16-row chunk x (row stride D, global): leaves F0 XH0 A1 XH1 F1 A2 XH2 F2 RS and
// Q [16][8] in LDS (mq_tile.h; weights staged by mq_stage). Ends with a barrier.
template <int D, int H, int A>
__device__ __forceinline__ void mq_agent_fwd(const float* __restrict__ P, const float* w, const float* x, int rows,
                                             float* act) {
  static_assert(H == 64, "64 hidden units: one 16-column MFMA tile per wave");
  mq_mlp_fwd(MGeo<D, H, A>{}, MqL<D>{}, MqL<D>{}, P, w, x, D, D, A, rows, act);
}

// per-block scratch slice (float offsets): per-agent Q and the mixer's tile intermediates
struct MqScr {
  int64_t q0, q1, dqa, act, z1, w1o, w2o, b2o, dw1o, dw2o, db2o, dz1, total;
};
inline MqScr mq_scr(const mm_offq_dims* d) {
  const bool qm = d->mixer == MM_OFFQ_QMIX;
  const int64_t N = d->n_agents, K = qm ? d->mixer_hidden : 0, Hh = qm ? d->hyper_hidden : 0;
  const int64_t ZW = 3 * Hh + K, NK = N * K;
  MqScr s = {};
  int64_t c = 0;
  auto take = [&](int64_t n) {
    const int64_t o = c;
    c += (n + 15) / 16 * 16;
    return o;
  };
  s.q0 = take(N * MQ_TB);
  s.q1 = take(N * MQ_TB);
  s.dqa = take(N * MQ_TB);
  s.act = take(N * MQ_TB);
  s.z1 = take(2 * MQ_TB * ZW);
  s.w1o = take(2 * MQ_TB * NK);
  s.w2o = take(2 * MQ_TB * K);
  s.b2o = take(2 * MQ_TB);
  s.dw1o = take(MQ_TB * NK);
  s.dw2o = take(MQ_TB * K);
  s.db2o = take(MQ_TB);
  s.dz1 = take(MQ_TB * ZW);
  s.total = c;
  return s;
}

struct MqArgs {
  const float* P; const float* PT;
  const float* obs; const float* nobs; const float* cobs; const float* cnobs; const float* acts; const float* rew;
  const float* dn; const float* isw;
  float* part; float* scr; float* prio;
  int64_t pstride;
  int64_t mo[15];
  MqScr so;
  int B, N, S, K, Hh, qmix, double_q, huber, ntiles;
  float gamma, delta, eps, invB;
};

__device__ __forceinline__ float mq_elu(float x) { return x > 0.0f ? x : expm1f(x); }
__device__ __forceinline__ float mq_sign(float x) { return x > 0.0f ? 1.0f : (x < 0.0f ? -1.0f : 0.0f); }

// Hypernets of one mixer over the tile: z1 [16][ZW] = first layers (pre-ReLU; columns w1 | w2 | b1 | b2), then
// w1o [16][NK], w2o [16][K], b2o [16] (second layers, before |.|). s: the tile's cent_obs rows. Ends with a barrier.
__device__ __forceinline__ void mq_hyper_fwd(const MqArgs& a, const float* Pm, const float* s, int rows, float* z1,
                                             float* w1o, float* w2o, float* b2o) {
  const int S = a.S, K = a.K, Hh = a.Hh, ZW = 3 * Hh + K, NK = a.N * K;
  const int col[4] = {0, Hh, 2 * Hh, 2 * Hh + K}, nc[4] = {Hh, Hh, K, Hh}, wi[4] = {0, 4, 8, 10};
  for (int q = 0; q < 4; ++q) {
    const float* bias = Pm + a.mo[wi[q] + 1];
    const int c0 = col[q];
    mq_gemm(s, S, false, rows, Pm + a.mo[wi[q]], S, 1, nc[q], S,
            [&](int i, int n, float v) { z1[i * ZW + c0 + n] = v + bias[n]; });
  }
  __syncthreads();
  mq_gemm(z1, ZW, true, rows, Pm + a.mo[2], Hh, 1, NK, Hh,
          [&](int i, int n, float v) { w1o[i * NK + n] = v + Pm[a.mo[3] + n]; });
  mq_gemm(z1 + Hh, ZW, true, rows, Pm + a.mo[6], Hh, 1, K, Hh,
          [&](int i, int n, float v) { w2o[i * K + n] = v + Pm[a.mo[7] + n]; });
  mq_gemm(z1 + 2 * Hh + K, ZW, true, rows, Pm + a.mo[12], Hh, 1, 1, Hh,
          [&](int i, int n, float v) { b2o[i] = v + Pm[a.mo[13] + n]; });
  __syncthreads();
}

template <int D, int H, int A>
__global__ __launch_bounds__(256) void moffq_train_kernel(MqArgs a) {
  using G = MGeo<D, H, A>;
  using L = MqL<D>;
  extern __shared__ __attribute__((aligned(16))) float sm[];
  float* wb = sm;
  float* wt = sm + L::nW;
  float* act = sm + 2 * L::nW;
  const int tid = threadIdx.x;
  mq_stage<D, H, A>(wb, a.P);
  mq_stage<D, H, A>(wt, a.PT);
  float* part = a.part + blockIdx.x * a.pstride;
  for (int64_t e = tid; e < a.pstride; e += blockDim.x) part[e] = 0.0f;
  float* scr = a.scr + blockIdx.x * a.so.total;
  float* q0 = scr + a.so.q0;
  float* q1 = scr + a.so.q1;
  float* dqa = scr + a.so.dqa;
  int* aidx = reinterpret_cast<int*>(scr + a.so.act);
  __syncthreads();
  const int N = a.N, S = a.S, K = a.K, Hh = a.Hh, ZW = 3 * Hh + K, NK = N * K;
  float* hidc = act + L::A1;   // [16][64] mixer tile values: the agent buffers are idle in phase 2
  float* preb = act + L::XH1;
  float* dpreb = act + L::F1;
  float* sDq = act + L::DQ;
  float* sLs = act + L::LS;
  float* sQt = act + L::QT;
  int* sArg = reinterpret_cast<int*>(act + L::ARG);
  float loss_acc = 0.0f, q_acc = 0.0f;   // thread 0
  for (int tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
    const int b0 = tile * MQ_TB;
    const int rows = min(MQ_TB, a.B - b0);
    // ---------------- phase 1: per-agent Q(s, a) and next Q
    for (int n = 0; n < N; ++n) {
      const int64_t r0 = (int64_t)n * a.B + b0;
      if (a.double_q) {
        mq_agent_fwd<D, H, A>(a.P, wb, a.nobs + r0 * D, rows, act);
        if (tid < rows) {
          const float* q = act + L::Q + tid * 8;
          int gi = 0;
#pragma unroll
          for (int k = 1; k < A; ++k)
            if (q[k] > q[gi]) gi = k;
          sArg[tid] = gi;
        }
        __syncthreads();
      }
      mq_agent_fwd<D, H, A>(a.PT, wt, a.nobs + r0 * D, rows, act);
      if (tid < rows) {
        const float* q = act + L::Q + tid * 8;
        float nq;
        if (a.double_q) {
          nq = q[sArg[tid]];
        } else {
          nq = q[0];
#pragma unroll
          for (int k = 1; k < A; ++k) nq = fmaxf(nq, q[k]);
        }
        q1[n * MQ_TB + tid] = nq;
      }
      __syncthreads();
      mq_agent_fwd<D, H, A>(a.P, wb, a.obs + r0 * D, rows, act);
      if (tid < rows) {
        // action index = first maximum of the one-hot row (mqmix.py:132)
        const float* oh = a.acts + (r0 + tid) * A;
        int ai = 0;
        float best = oh[0];
#pragma unroll
        for (int k = 1; k < A; ++k)
          if (oh[k] > best) {
            best = oh[k];
            ai = k;
          }
        aidx[n * MQ_TB + tid] = ai;
        q0[n * MQ_TB + tid] = act[L::Q + tid * 8 + ai];
      }
      __syncthreads();
    }
    // ---------------- phase 2: mixers, loss, dQ_tot, mixer backward
    const float* s0 = a.qmix ? a.cobs + (int64_t)b0 * S : nullptr;
    float* z1 = scr + a.so.z1;
    float* w1o = scr + a.so.w1o;
    float* w2o = scr + a.so.w2o;
    float* b2o = scr + a.so.b2o;
    for (int y = 0; y < 2; ++y) {
      const float* qy = y ? q1 : q0;
      if (a.qmix) {
        const float* Pm = (y ? a.PT : a.P) + G::total;
        float* z1y = z1 + (int64_t)y * MQ_TB * ZW;
        float* w1y = w1o + (int64_t)y * MQ_TB * NK;
        float* w2y = w2o + y * MQ_TB * K;
        mq_hyper_fwd(a, Pm, (y ? a.cnobs : a.cobs) + (int64_t)b0 * S, rows, z1y, w1y, w2y, b2o + y * MQ_TB);
        for (int e = tid; e < rows * K; e += blockDim.x) {
          const int i = e / K, k = e - i * K;
          float s = 0.0f;
          for (int n = 0; n < N; ++n) s = fmaf(qy[n * MQ_TB + i], fabsf(w1y[(int64_t)i * NK + n * K + k]), s);
          const float pre = s + z1y[i * ZW + 2 * Hh + k];
          if (y == 0) preb[i * 64 + k] = pre;
          hidc[i * 64 + k] = mq_elu(pre) * fabsf(w2y[i * K + k]);
        }
        __syncthreads();
        if (tid < rows) {
          float s = 0.0f;
          for (int k = 0; k < K; ++k) s += hidc[tid * 64 + k];
          sQt[y * MQ_TB + tid] = s + b2o[y * MQ_TB + tid];
        }
      } else if (tid < rows) {
        float s = 0.0f;
        for (int n = 0; n < N; ++n) s += qy[n * MQ_TB + tid];
        sQt[y * MQ_TB + tid] = s;
      }
      __syncthreads();
    }
    if (tid < rows) {
      const int b = b0 + tid;
      const float w = a.isw ? a.isw[b] : 1.0f;
      const float tgt = a.rew[b] + (1.0f - a.dn[b]) * a.gamma * sQt[MQ_TB + tid];
      const float er = sQt[tid] - tgt;
      const float ae = fabsf(er);
      float le, dle;
      if (a.huber) {
        const bool in = ae <= a.delta;
        le = in ? er * er / 2.0f : a.delta * (ae - a.delta / 2.0f);
        dle = in ? er : a.delta * mq_sign(er);
      } else {
        le = er * er;
        dle = 2.0f * er;
      }
      sDq[tid] = w * dle * a.invB;
      sLs[tid] = w * le;
      if (a.isw && a.prio) a.prio[b] = ae + a.eps;
    }
    __syncthreads();
    if (tid == 0)
      for (int i = 0; i < rows; ++i) {
        loss_acc += sLs[i];
        q_acc += sQt[i];
      }
    if (a.qmix) {
      const float* Pm = a.P + G::total;
      float* gm = part + G::total;
      float* dw1o = scr + a.so.dw1o;
      float* dw2o = scr + a.so.dw2o;
      float* db2o = scr + a.so.db2o;
      float* dz1 = scr + a.so.dz1;
      for (int e = tid; e < rows * K; e += blockDim.x) {
        const int i = e / K, k = e - i * K;
        const float g = sDq[i], pre = preb[i * 64 + k], hid = mq_elu(pre), w2k = w2o[i * K + k];
        // |w|' = sign(w) (0 at 0); elu' = 1 (x > 0) or exp(x) = elu(x) + 1
        dw2o[i * K + k] = g * hid * mq_sign(w2k);
        const float dpre = g * fabsf(w2k) * (pre > 0.0f ? 1.0f : hid + 1.0f);
        dz1[i * ZW + 2 * Hh + k] = dpre;
        dpreb[i * 64 + k] = dpre;
        for (int n = 0; n < N; ++n)
          dw1o[(int64_t)i * NK + n * K + k] = q0[n * MQ_TB + i] * dpre * mq_sign(w1o[(int64_t)i * NK + n * K + k]);
      }
      if (tid < rows) db2o[tid] = sDq[tid];
      __syncthreads();
      for (int e = tid; e < rows * N; e += blockDim.x) {
        const int i = e / N, n = e - i * N;
        float s = 0.0f;
        for (int k = 0; k < K; ++k) s = fmaf(fabsf(w1o[(int64_t)i * NK + n * K + k]), dpreb[i * 64 + k], s);
        dqa[n * MQ_TB + i] = s;
      }
      // hypernet hidden deltas: dZ1 part = (D . W_second) * (Z1 part > 0)
      mq_gemm(dw1o, NK, false, rows, Pm + a.mo[2], 1, Hh, Hh, NK,
              [&](int i, int n, float v) { dz1[i * ZW + n] = z1[i * ZW + n] > 0.0f ? v : 0.0f; });
      mq_gemm(dw2o, K, false, rows, Pm + a.mo[6], 1, Hh, Hh, K,
              [&](int i, int n, float v) { dz1[i * ZW + Hh + n] = z1[i * ZW + Hh + n] > 0.0f ? v : 0.0f; });
      for (int e = tid; e < rows * Hh; e += blockDim.x) {
        const int i = e / Hh, h = e - i * Hh, c = 2 * Hh + K + h;
        dz1[i * ZW + c] = z1[i * ZW + c] > 0.0f ? sDq[i] * Pm[a.mo[12] + h] : 0.0f;
      }
      __syncthreads();
      // mixer weight gradients of the tile
      mq_wgrad(dw1o, NK, z1, ZW, true, rows, NK, Hh, gm + a.mo[2], Hh);
      mq_colsum(dw1o, NK, nullptr, 0, rows, NK, gm + a.mo[3]);
      mq_wgrad(dw2o, K, z1 + Hh, ZW, true, rows, K, Hh, gm + a.mo[6], Hh);
      mq_colsum(dw2o, K, nullptr, 0, rows, K, gm + a.mo[7]);
      mq_wgrad(db2o, 1, z1 + 2 * Hh + K, ZW, true, rows, 1, Hh, gm + a.mo[12], Hh);
      mq_colsum(db2o, 1, nullptr, 0, rows, 1, gm + a.mo[13]);
      const int col[4] = {0, Hh, 2 * Hh, 2 * Hh + K}, nr[4] = {Hh, Hh, K, Hh}, wi[4] = {0, 4, 8, 10};
      for (int q = 0; q < 4; ++q) {
        mq_wgrad(dz1 + col[q], ZW, s0, S, false, rows, nr[q], S, gm + a.mo[wi[q]], S);
        mq_colsum(dz1 + col[q], ZW, nullptr, 0, rows, nr[q], gm + a.mo[wi[q] + 1]);
      }
    } else {
      for (int e = tid; e < rows * N; e += blockDim.x) {
        const int i = e / N, n = e - i * N;
        dqa[n * MQ_TB + i] = sDq[i];
      }
    }
    __syncthreads();
    // ---------------- phase 3: per-agent backward (forward recomputed into LDS)
    for (int n = 0; n < N; ++n) {
      const int64_t r0 = (int64_t)n * a.B + b0;
      mq_agent_fwd<D, H, A>(a.P, wb, a.obs + r0 * D, rows, act);
      if (tid < MQ_TB * 8) {
        const int i = tid >> 3, k = tid & 7;
        act[L::DO + tid] = (i < rows && k == aidx[n * MQ_TB + i]) ? dqa[n * MQ_TB + i] : 0.0f;
      }
      __syncthreads();
      mq_mlp_bwd(G{}, L{}, L{}, a.P, wb, D, A, rows, true, true, act, part);
    }
  }
  if (tid == 0) {
    part[a.pstride - 2] = loss_acc;
    part[a.pstride - 1] = q_acc;
  }
}

// grad[e] = sum of the block partials in block order; the last two entries are the loss and Q_tot sums
__global__ __launch_bounds__(256) void moffq_reduce_kernel(const float* __restrict__ part, int64_t pstride, int nblk,
                                                           int64_t total, float* __restrict__ grad,
                                                           float* __restrict__ stats, float invB) {
  const int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (e >= total + 2) return;
  const int64_t src = e < total ? e : pstride - 2 + (e - total);
  float s = 0.0f;
  for (int b = 0; b < nblk; ++b) s += part[b * pstride + src];
  if (e < total) grad[e] = s;
  else stats[e - total] = s * invB;
}

struct MqQArgs {
  const float* P; const float* obs; const int32_t* actions; float* q;
  int64_t R, ntiles;
};

template <int D, int H, int A>
__global__ __launch_bounds__(256) void moffq_q_kernel(MqQArgs a) {
  using L = MqL<D>;
  extern __shared__ __attribute__((aligned(16))) float sm[];
  float* act = sm + L::nW;
  mq_stage<D, H, A>(sm, a.P);
  __syncthreads();
  for (int64_t tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
    const int64_t r0 = tile * MQ_TB;
    const int rows = (int)std::min<int64_t>(MQ_TB, a.R - r0);
    mq_agent_fwd<D, H, A>(a.P, sm, a.obs + r0 * D, rows, act);
    const int i = threadIdx.x >> 3, k = threadIdx.x & 7;
    if (threadIdx.x < MQ_TB * 8 && i < rows) {
      if (a.actions) {
        if (k == 0) {
          const int ai = a.actions[r0 + i];
          a.q[r0 + i] = act[L::Q + i * 8 + (ai < 0 ? 0 : (ai >= A ? A - 1 : ai))];
        }
      } else if (k < A) {
        a.q[(r0 + i) * A + k] = act[L::Q + i * 8 + k];
      }
    }
    __syncthreads();
  }
}

int mq_check(const mm_offq_dims* d) {
  MM_REQUIRE(d && d->n_agents >= 1, "moffq: bad dims");
  MM_REQUIRE(d->mixer == MM_OFFQ_VDN || d->mixer == MM_OFFQ_QMIX, "moffq: mixer must be MM_OFFQ_VDN or MM_OFFQ_QMIX");
  MM_REQUIRE(!d->prev_act_inp, "moffq: prev_act_inp is not built for the feed-forward trainer (mm_offq_loss_grad has it)");
  MM_REQUIRE(d->hidden == 64 && d->n_actions == 5 && (d->obs_dim == 3 || d->obs_dim == 47 || d->obs_dim == 94),
             "moffq: unsupported dims D=%d H=%d A=%d (supported: D 3|47|94, H 64, A 5)", d->obs_dim, d->hidden,
             d->n_actions);
  MM_REQUIRE(d->mixer == MM_OFFQ_VDN ||
                 (d->state_dim >= 1 && d->mixer_hidden >= 1 && d->hyper_hidden >= 1 &&
                  (int64_t)d->n_agents * d->mixer_hidden <= 4096),
             "moffq: QMIX needs state_dim, mixer_hidden, hyper_hidden >= 1 and N*K <= 4096");
  MM_REQUIRE(d->mixer == MM_OFFQ_VDN || d->mixer_hidden <= MM_OFFQ_MAX_MIXER_HIDDEN,
             "moffq: mixer_hidden %d is above the limit of %d (the mixer tile keeps 64 units per transition in LDS)",
             d->mixer_hidden, MM_OFFQ_MAX_MIXER_HIDDEN);
  return MM_OK;
}

int mq_blocks(int B) { return std::min((B + MQ_TB - 1) / MQ_TB, MQ_MAX_BLOCKS); }

template <int D, int H, int A>
struct MoffqShape {
  using G = MGeo<D, H, A>;
  using L = MqL<D>;

  static int set_lds() {
    static bool done = false;
    if (done) return MM_OK;
    MM_HIP_CHECK(hipFuncSetAttribute((const void*)moffq_train_kernel<D, H, A>,
                                     hipFuncAttributeMaxDynamicSharedMemorySize, L::train_bytes));
    MM_HIP_CHECK(hipFuncSetAttribute((const void*)moffq_q_kernel<D, H, A>,
                                     hipFuncAttributeMaxDynamicSharedMemorySize, L::q_bytes));
    done = true;
    return MM_OK;
  }

  static int64_t total(const mm_offq_dims* d) {
    int64_t o[15];
    mm_offq_mixer_offsets(d, o);
    return G::total + o[14];
  }
  static int64_t pstride(const mm_offq_dims* d) { return (total(d) + 2 + 15) / 16 * 16; }
  static int64_t ws_floats(const mm_offq_dims* d, int B) {
    return (int64_t)mq_blocks(B) * (pstride(d) + mq_scr(d).total);
  }

  static int loss_grad(const mm_offq_dims* d, const mm_moffq_batch* b, const float* P, const float* PT, float* grad,
                       float* ws, float* stats, float* prio, hipStream_t s) {
    if (set_lds()) return MM_EHIP;
    const bool qm = d->mixer == MM_OFFQ_QMIX;
    const int nblk = mq_blocks(b->B);
    MqArgs a = {};
    a.P = P;
    a.PT = PT;
    a.obs = b->obs;
    a.nobs = b->nobs;
    a.cobs = b->cent_obs;
    a.cnobs = b->cent_nobs;
    a.acts = b->acts;
    a.rew = b->rewards;
    a.dn = b->dones_env;
    a.isw = b->is_weight;
    a.pstride = pstride(d);
    a.part = ws;
    a.scr = ws + nblk * a.pstride;
    a.prio = prio;
    mm_offq_mixer_offsets(d, a.mo);
    a.so = mq_scr(d);
    a.B = b->B;
    a.N = d->n_agents;
    a.S = qm ? d->state_dim : 0;
    a.K = qm ? d->mixer_hidden : 0;
    a.Hh = qm ? d->hyper_hidden : 0;
    a.qmix = qm;
    a.double_q = b->double_q;
    a.huber = b->huber;
    a.ntiles = (b->B + MQ_TB - 1) / MQ_TB;
    a.gamma = b->gamma;
    a.delta = b->huber_delta;
    a.eps = b->per_eps;
    a.invB = 1.0f / (float)b->B;
    hipLaunchKernelGGL((moffq_train_kernel<D, H, A>), dim3(nblk), dim3(256), (size_t)L::train_bytes, s, a);
    MM_HIP_CHECK(hipGetLastError());
    const int64_t tot = total(d);
    hipLaunchKernelGGL(moffq_reduce_kernel, dim3((unsigned)((tot + 2 + 255) / 256)), dim3(256), 0, s, ws, a.pstride,
                       nblk, tot, grad, stats, a.invB);
    MM_HIP_CHECK(hipGetLastError());
    return MM_OK;
  }

  static int q_values(const float* P, const float* obs, const int32_t* actions, float* q, int64_t R, hipStream_t s) {
    if (set_lds()) return MM_EHIP;
    MqQArgs a = {P, obs, actions, q, R, (R + MQ_TB - 1) / MQ_TB};
    const int nblk = (int)std::min<int64_t>(a.ntiles, MQ_Q_BLOCKS);
    hipLaunchKernelGGL((moffq_q_kernel<D, H, A>), dim3(nblk), dim3(256), (size_t)L::q_bytes, s, a);
    MM_HIP_CHECK(hipGetLastError());
    return MM_OK;
  }
};

#define MM_MOFFQ_DISPATCH(d, CALL)                            \
  do {                                                        \
    if ((d)->obs_dim == 3) {                                  \
      using SH = MoffqShape<3, 64, 5>;                        \
      return CALL;                                            \
    }                                                         \
    if ((d)->obs_dim == 47) {                                 \
      using SH = MoffqShape<47, 64, 5>;                       \
      return CALL;                                            \
    }                                                         \
    using SH = MoffqShape<94, 64, 5>;                         \
    return CALL;                                              \
  } while (0)

int64_t mq_ws_floats(const mm_offq_dims* d, int B) { MM_MOFFQ_DISPATCH(d, SH::ws_floats(d, B)); }

}  // namespace
}  // namespace mm

extern "C" {

int64_t mm_moffq_workspace_bytes(const mm_offq_dims* d, int32_t B) {
  if (mm::mq_check(d) || B < 1) return -1;
  return mm::mq_ws_floats(d, B) * 4;
}

int mm_moffq_loss_grad(const mm_offq_dims* d, const mm_moffq_batch* b, const float* P, const float* PT, float* grad,
                       void* ws, int64_t ws_bytes, float* stats, float* priorities, mm_stream_t s) {
  int rc = mm::mq_check(d);
  if (rc) return rc;
  MM_REQUIRE(b && P && PT && grad && ws && stats, "moffq_loss_grad: null argument");
  MM_REQUIRE(b->obs && b->nobs && b->acts && b->rewards && b->dones_env &&
                 (d->mixer == MM_OFFQ_VDN || (b->cent_obs && b->cent_nobs)),
             "moffq_loss_grad: batch arrays missing");
  MM_REQUIRE(b->B >= 1, "moffq_loss_grad: B must be >= 1");
  MM_REQUIRE(!b->is_weight || priorities, "moffq_loss_grad: PER (is_weight) needs a priorities output");
  const int64_t need = mm_moffq_workspace_bytes(d, b->B);
  MM_REQUIRE(need > 0 && ws_bytes >= need, "moffq_loss_grad: workspace %lld bytes < %lld", (long long)ws_bytes,
             (long long)need);
  using namespace mm;
  MM_MOFFQ_DISPATCH(d, SH::loss_grad(d, b, P, PT, grad, (float*)ws, stats, priorities, (hipStream_t)s));
}

int mm_moffq_q_values(const mm_offq_dims* d, const float* P, const float* obs, const int32_t* actions, float* q,
                      int64_t R, mm_stream_t s) {
  int rc = mm::mq_check(d);
  if (rc) return rc;
  MM_REQUIRE(P && obs && q && R >= 1, "moffq_q_values: bad args");
  using namespace mm;
  MM_MOFFQ_DISPATCH(d, SH::q_values(P, obs, actions, q, R, (hipStream_t)s));
}

}  // extern "C"
