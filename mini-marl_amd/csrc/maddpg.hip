// Feed-forward transition-batch MADDPG / MATD3 trainer ("maddpg" / "matd3") of the reference's offpolicy fork on
// gfx950: MADDPG.shared_train_policy_on_batch (offpolicy/algorithms/maddpg/maddpg.py:90-249) with MADDPGPolicy
// (algorithm/MADDPGPolicy.py:63-151), discrete actions, one shared policy.
//
//   actor   LN(D) -> Linear(D,64) -> ReLU -> LN -> Linear(64,64) -> ReLU -> LN -> Linear(64,A): the agent net of
//           moffq.hip, in the same 18-tensor trunk layout (MGeo<D, 64, A>; recurrent tensors unread, zero gradient).
//   critic  the same trunk over x = [cent_obs | cent_act], width Dc = N D + N A (a runtime value), with nq = 1
//           (maddpg) or 2 (matd3) 64 -> 1 heads kept in the Wo / bo slot (4 rows). The heads are NEVER trained: the
//           reference keeps them in a plain Python list, outside parameters(); their gradient here is exactly zero.
//
// One update is two gradient launches, each followed by a block-order reduction (and mm_clip_adam by the caller):
//   critic pass (maddpg_critic_kernel), per tile of 16 transitions: the target actor on nobs of every agent (16-row
//     chunks) -> target one-hot actions (maddpg: logits == rowmax, multi-hot on an exact tie; matd3: the exact
//     one-hot argmax of logits + target Gumbel noise) written beside cent_nobs in LDS; the target critic -> min over
//     heads; target = r (agent 0) + gamma (1 - done_env) minQ'; the live critic on [cent_obs | stored acts];
//     err_h = target - Q_h, loss sum_h mean_b w_b f(err_h), priorities mean_h |err_h| + per_eps; backward down to
//     ln0 / W1; the tile's weight gradients go into a block-private partial in tile order.
//   actor pass (maddpg_actor_kernel), per tile: (A) the live actor on obs of every agent -> y = softmax(logits + g),
//     hard = argmax; (B) for each agent i the critic input is the stored row with only agent i's A columns replaced
//     by hard_i; the (already updated) critic forward, head 0; backward to the input only, through the Dc-wide
//     feature LayerNorm, down to agent i's A columns: that is dL/dy_i (straight-through); (C) softmax backward and
//     the actor backward with weight gradients (the actor forward is recomputed into LDS, as in moffq.hip phase 3).
//     The loss is -sum Q_i valid_i / sum valid; the 1 / sum valid factor is applied by the reduction.
//   md_reduce_kernel: grad[e] = sum over blocks in block order. No float atomics; the grid is a function of B alone:
//     two runs give the same bits.
// Every Linear (forward, dX, dW) is v_mfma_f32_16x16x4_f32 through mq_tile.h.
//
// Memory. LDS holds one staged actor net, the 64-wide activations of one chunk (shared by the actor and the critic,
// which never run at once) and TWO 16 x (ceil4(Dc) + 1) rows for the critic input (LN in place; G0 reuses F0):
//   (actor weights + activations + 32 (ceil4(Dc) + 1)) floats: Dc 16 (Switch N 2) 58 KB, Dc 104 (Checkers N 2) 89 KB,
//   Dc 198 (D 94, N 2) 123 KB, Dc 416 (N 8) 129 KB of 160 KB.
// The critic weights are STREAMED from L2 as MFMA B operands at every width, W1 [64][ceil4(Dc)] and W2 / heads alike
// (the way moffq.hip streams the hypernet weights): staging W1 at Dc 416 would take 106 KB, and staging only W2 does
// not fit next to a 94-wide actor at Dc 396. Dc <= MM_MADDPG_MAX_CRITIC_WIDTH (416).
// In the actor pass the N critic inputs of a transition are N full first-layer GEMMs; the rank-A correction of one
// shared product is not built.
#include <algorithm>

#include "common.h"
#include "minimarl.h"
#include "mq_tile.h"

namespace mm {
namespace {

constexpr int MD_MAX_BLOCKS = 256;
constexpr int MD_A = 5;
constexpr int MD_LDS_LIMIT = 160 * 1024;

// critic: MGeo<Dc, 64, 4> with a runtime Dc
struct MdGeo {
  int Dp, ln0_w, ln0_b, W1, b1, ln1_w, ln1_b, W2, b2, ln2_w, ln2_b, Wo, bo, total;
};
__host__ __device__ inline MdGeo md_geo(int Dc) {
  MdGeo g;
  const int H = 64;
  g.Dp = (Dc + 3) & ~3;
  g.ln0_w = 0;
  g.ln0_b = g.Dp;
  g.W1 = 2 * g.Dp;
  g.b1 = g.W1 + H * g.Dp;
  g.ln1_w = g.b1 + H;
  g.ln1_b = g.ln1_w + H;
  g.W2 = g.ln1_b + H;
  g.b2 = g.W2 + H * H;
  g.ln2_w = g.b2 + H;
  g.ln2_b = g.ln2_w + H;
  g.Wo = g.ln2_b + H + 6 * H * H + 6 * H + 2 * H;   // past Wih Whh bih bhh lnr_w lnr_b
  g.bo = g.Wo + 4 * H;
  g.total = g.bo + 4;
  return g;
}
// weights read in place from the flat vector
struct MdWL {
  int wW1, ldw1, wW2, ldw2, wWo;
};
// critic activations: the actor's 64-wide buffers plus two wide rows behind them
template <int D>
struct MdCL : MqL<D> {
  int ld0, F0, XH0, G0;
};

struct MdArgs {
  const float* PA; const float* PC; const float* PCT;
  const float* obs; const float* nobs; const float* cobs; const float* cnobs; const float* acts; const float* rew;
  const float* dn; const float* valid; const float* isw; const float* gum;
  float* part; float* scr; float* prio;
  int64_t pstride, sstride;
  MdGeo cg;
  int B, N, S, Dc, nq, td3, huber, ntiles;
  float gamma, delta, eps, invB;
};

template <int D>
__device__ __forceinline__ MdCL<D> md_cl(const MdGeo& cg) {
  MdCL<D> cl;
  cl.ld0 = cg.Dp + 1;
  cl.F0 = MqL<D>::nAct;
  cl.XH0 = cl.F0 + MQ_TB * cl.ld0;
  cl.G0 = cl.F0;
  return cl;
}

// X[i][0 : S] = cent rows, X[i][S + n A + k] = acts[n][b0 + i][k]; agent `hot` takes onehot(sh[hot][i]) instead
__device__ __forceinline__ void md_fill(const MdArgs& a, float* X, int ld, const float* cent, int b0, int rows,
                                        int hot, const int* sh) {
  const int S = a.S, NA = a.N * MD_A;
  for (int e = threadIdx.x; e < rows * S; e += blockDim.x) {
    const int i = e / S, c = e - i * S;
    X[i * ld + c] = cent[(int64_t)(b0 + i) * S + c];
  }
  if (!a.acts) return;
  for (int e = threadIdx.x; e < rows * NA; e += blockDim.x) {
    const int i = e / NA, c = e - i * NA, n = c / MD_A, k = c - n * MD_A;
    X[i * ld + S + c] = n == hot ? (k == sh[n * MQ_TB + i] ? 1.0f : 0.0f)
                                 : a.acts[((int64_t)n * a.B + b0 + i) * MD_A + k];
  }
}

template <int D>
__global__ __launch_bounds__(256) void maddpg_critic_kernel(MdArgs a) {
  using GA = MGeo<D, 64, MD_A>;
  using L = MqL<D>;
  extern __shared__ __attribute__((aligned(16))) float sm[];
  float* wa = sm;
  float* act = sm + L::nW;
  const int tid = threadIdx.x;
  const MdCL<D> cl = md_cl<D>(a.cg);
  const MdWL cw = {a.cg.W1, a.cg.Dp, a.cg.W2, 64, a.cg.Wo};
  mq_stage<D, 64, MD_A>(wa, a.PA);
  float* part = a.part + blockIdx.x * a.pstride;
  for (int64_t e = tid; e < a.pstride; e += blockDim.x) part[e] = 0.0f;
  __syncthreads();
  float* X = act + cl.F0;
  float* sTg = act + L::QT;
  float* sLs = act + L::LS;
  const int N = a.N, S = a.S;
  float loss_acc = 0.0f;   // thread 0
  for (int tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
    const int b0 = tile * MQ_TB;
    const int rows = min(MQ_TB, a.B - b0);
    // ---------------- target actions beside cent_nobs
    for (int e = tid; e < rows * S; e += blockDim.x) {
      const int i = e / S, c = e - i * S;
      X[i * cl.ld0 + c] = a.cnobs[(int64_t)(b0 + i) * S + c];
    }
    for (int n = 0; n < N; ++n) {
      const int64_t r0 = (int64_t)n * a.B + b0;
      mq_mlp_fwd(GA{}, L{}, L{}, a.PA, wa, a.nobs + r0 * D, D, D, MD_A, rows, act);
      if (tid < rows) {
        const float* q = act + L::Q + tid * 8;
        float* xo = X + tid * cl.ld0 + S + n * MD_A;
        if (a.td3) {
          const float* g = a.gum + (r0 + tid) * MD_A;
          int gi = 0;
          float best = q[0] + g[0];
#pragma unroll
          for (int k = 1; k < MD_A; ++k) {
            const float z = q[k] + g[k];
            if (z > best) {
              best = z;
              gi = k;
            }
          }
#pragma unroll
          for (int k = 0; k < MD_A; ++k) xo[k] = k == gi ? 1.0f : 0.0f;
        } else {
          float mx = q[0];
#pragma unroll
          for (int k = 1; k < MD_A; ++k) mx = fmaxf(mx, q[k]);
#pragma unroll
          for (int k = 0; k < MD_A; ++k) xo[k] = q[k] == mx ? 1.0f : 0.0f;
        }
      }
      __syncthreads();
    }
    // ---------------- target critic, min over heads, target
    mq_mlp_fwd(a.cg, cw, cl, a.PCT, a.PCT, X, cl.ld0, a.Dc, a.nq, rows, act);
    if (tid < rows) {
      const int b = b0 + tid;
      float mq = act[L::Q + tid * 8];
      for (int h = 1; h < a.nq; ++h) mq = fminf(mq, act[L::Q + tid * 8 + h]);
      sTg[tid] = a.rew[b] + a.gamma * (1.0f - a.dn[b]) * mq;
    }
    __syncthreads();
    // ---------------- live critic on the stored actions, loss, backward
    md_fill(a, X, cl.ld0, a.cobs, b0, rows, -1, nullptr);
    __syncthreads();
    mq_mlp_fwd(a.cg, cw, cl, a.PC, a.PC, X, cl.ld0, a.Dc, a.nq, rows, act);
    if (tid < MQ_TB * 8) {
      const int i = tid >> 3, h = tid & 7;
      float d = 0.0f;
      if (i < rows && h < a.nq) {
        const float w = a.isw ? a.isw[b0 + i] : 1.0f;
        const float er = sTg[i] - act[L::Q + tid];
        float dle;   // f'(err)
        if (a.huber) dle = fabsf(er) <= a.delta ? er : (er > 0.0f ? a.delta : -a.delta);
        else dle = 2.0f * er;
        d = -w * dle * a.invB;
      }
      act[L::DO + tid] = d;
    }
    if (tid < rows) {
      const int b = b0 + tid;
      const float w = a.isw ? a.isw[b] : 1.0f;
      float ls = 0.0f, ab = 0.0f;
      for (int h = 0; h < a.nq; ++h) {
        const float er = sTg[tid] - act[L::Q + tid * 8 + h];
        const float ae = fabsf(er);
        ab += ae;
        if (a.huber) ls += ae <= a.delta ? er * er / 2.0f : a.delta * (ae - a.delta / 2.0f);
        else ls += er * er;
      }
      sLs[tid] = w * ls;
      if (a.isw && a.prio) a.prio[b] = ab / (float)a.nq + a.eps;
    }
    __syncthreads();
    if (tid == 0)
      for (int i = 0; i < rows; ++i) loss_acc += sLs[i];
    mq_mlp_bwd(a.cg, cw, cl, a.PC, a.PC, a.Dc, a.nq, rows, false, true, act, part);
  }
  if (tid == 0) {
    part[a.pstride - 2] = loss_acc;
    part[a.pstride - 1] = 0.0f;
  }
}

template <int D>
__global__ __launch_bounds__(256) void maddpg_actor_kernel(MdArgs a) {
  using GA = MGeo<D, 64, MD_A>;
  using L = MqL<D>;
  extern __shared__ __attribute__((aligned(16))) float sm[];
  float* wa = sm;
  float* act = sm + L::nW;
  const int tid = threadIdx.x;
  const MdCL<D> cl = md_cl<D>(a.cg);
  const MdWL cw = {a.cg.W1, a.cg.Dp, a.cg.W2, 64, a.cg.Wo};
  mq_stage<D, 64, MD_A>(wa, a.PA);
  float* part = a.part + blockIdx.x * a.pstride;
  for (int64_t e = tid; e < a.pstride; e += blockDim.x) part[e] = 0.0f;
  const int N = a.N, S = a.S;
  float* sy = a.scr + blockIdx.x * a.sstride;            // [N][16][8] y = softmax(logits + g)
  float* sdy = sy + (int64_t)N * MQ_TB * 8;              // [N][16][8] dL/dy
  int* sh = reinterpret_cast<int*>(sdy + (int64_t)N * MQ_TB * 8);   // [N][16] argmax
  __syncthreads();
  float* X = act + cl.F0;
  float* sLs = act + L::LS;
  float* sVs = act + L::DQ;
  float loss_acc = 0.0f, v_acc = 0.0f;   // thread 0
  for (int tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
    const int b0 = tile * MQ_TB;
    const int rows = min(MQ_TB, a.B - b0);
    // ---------------- phase A: Gumbel-softmax of every agent's logits
    for (int n = 0; n < N; ++n) {
      const int64_t r0 = (int64_t)n * a.B + b0;
      mq_mlp_fwd(GA{}, L{}, L{}, a.PA, wa, a.obs + r0 * D, D, D, MD_A, rows, act);
      if (tid < rows) {
        const float* q = act + L::Q + tid * 8;
        const float* g = a.gum + (r0 + tid) * MD_A;
        float z[MD_A];
        int gi = 0;
        float best = q[0] + g[0];
#pragma unroll
        for (int k = 0; k < MD_A; ++k) {
          z[k] = q[k] + g[k];
          if (z[k] > best) {
            best = z[k];
            gi = k;
          }
        }
        float s = 0.0f;
#pragma unroll
        for (int k = 0; k < MD_A; ++k) {
          z[k] = expf(z[k] - best);
          s += z[k];
        }
        float* yo = sy + (n * MQ_TB + tid) * 8;
#pragma unroll
        for (int k = 0; k < MD_A; ++k) yo[k] = z[k] / s;
        sh[n * MQ_TB + tid] = gi;
      }
      __syncthreads();
    }
    // ---------------- phase B: dL/dy_i through the critic, one agent's columns replaced at a time
    for (int i = 0; i < N; ++i) {
      md_fill(a, X, cl.ld0, a.cobs, b0, rows, i, sh);
      __syncthreads();
      mq_mlp_fwd(a.cg, cw, cl, a.PC, a.PC, X, cl.ld0, a.Dc, 1, rows, act);
      if (tid < MQ_TB * 8) {
        const int r = tid >> 3, h = tid & 7;
        act[L::DO + tid] = (r < rows && h == 0) ? -a.valid[(int64_t)i * a.B + b0 + r] : 0.0f;
      }
      if (tid < rows) {
        const float v = a.valid[(int64_t)i * a.B + b0 + tid];
        sLs[tid] = act[L::Q + tid * 8] * v;
        sVs[tid] = v;
      }
      __syncthreads();
      if (tid == 0)
        for (int r = 0; r < rows; ++r) {
          loss_acc += sLs[r];
          v_acc += sVs[r];
        }
      mq_mlp_bwd(a.cg, cw, cl, a.PC, a.PC, a.Dc, 1, rows, false, false, act, nullptr);
      {
        // feature LayerNorm backward over the full width, kept for agent i's A input columns
        const int row = tid >> 4, sub = tid & 15;
        const bool ok = row < rows;
        const float* G0 = act + cl.G0 + row * cl.ld0;
        const float* XH = act + cl.XH0 + row * cl.ld0;
        const float* gw = a.PC + a.cg.ln0_w;
        float sg = 0.f, sgx = 0.f;
        for (int c = sub; c < a.Dc; c += 16) {
          const float gg = ok ? G0[c] * gw[c] : 0.f;
          sg += gg;
          sgx = fmaf(gg, ok ? XH[c] : 0.f, sgx);
        }
        sg = sum16(sg) / (float)a.Dc;
        sgx = sum16(sgx) / (float)a.Dc;
        if (ok && sub < MD_A) {
          const int c = S + i * MD_A + sub;
          sdy[(i * MQ_TB + row) * 8 + sub] = act[L::RS + row] * (G0[c] * gw[c] - sg - XH[c] * sgx);
        }
      }
      __syncthreads();
    }
    // ---------------- phase C: softmax backward, actor backward (forward recomputed into LDS)
    for (int n = 0; n < N; ++n) {
      const int64_t r0 = (int64_t)n * a.B + b0;
      mq_mlp_fwd(GA{}, L{}, L{}, a.PA, wa, a.obs + r0 * D, D, D, MD_A, rows, act);
      if (tid < MQ_TB * 8) {
        const int r = tid >> 3, k = tid & 7;
        float d = 0.0f;
        if (r < rows && k < MD_A) {
          const float* y = sy + (n * MQ_TB + r) * 8;
          const float* dy = sdy + (n * MQ_TB + r) * 8;
          float dot = 0.0f;
#pragma unroll
          for (int j = 0; j < MD_A; ++j) dot = fmaf(y[j], dy[j], dot);
          d = y[k] * (dy[k] - dot);
        }
        act[L::DO + tid] = d;
      }
      __syncthreads();
      mq_mlp_bwd(GA{}, L{}, L{}, a.PA, wa, D, MD_A, rows, true, true, act, part);
    }
  }
  if (tid == 0) {
    part[a.pstride - 2] = loss_acc;
    part[a.pstride - 1] = v_acc;
  }
}

// grad[e] = sum of the block partials in block order. Critic (by_valid 0): stats = {loss sum / B, 0}. Actor
// (by_valid 1): V = sum valid, grad / V, stats = {-(sum Q valid) / V, V}.
__global__ __launch_bounds__(256) void md_reduce_kernel(const float* __restrict__ part, int64_t pstride, int nblk,
                                                        int64_t total, float* __restrict__ grad,
                                                        float* __restrict__ stats, float invB, int by_valid) {
  const int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (e >= total + 2) return;
  const int64_t src = e < total ? e : pstride - 2 + (e - total);
  float s = 0.0f, V = 0.0f;
  for (int b = 0; b < nblk; ++b) {
    s += part[b * pstride + src];
    V += part[b * pstride + pstride - 1];
  }
  if (e < total) grad[e] = by_valid ? s / V : s;
  else if (e == total) stats[0] = by_valid ? -s / V : s * invB;
  else stats[1] = by_valid ? V : 0.0f;
}

struct MdLogitArgs {
  const float* P; const float* obs; const float* gum; float* logits; float* onehot;
  int64_t R, ntiles;
};

// actor logits [R, A]; onehot (optional): argmax of logits + gum, or logits == rowmax without gum
template <int D>
__global__ __launch_bounds__(256) void maddpg_logits_kernel(MdLogitArgs a) {
  using L = MqL<D>;
  extern __shared__ __attribute__((aligned(16))) float sm[];
  float* act = sm + L::nW;
  mq_stage<D, 64, MD_A>(sm, a.P);
  __syncthreads();
  for (int64_t tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
    const int64_t r0 = tile * MQ_TB;
    const int rows = (int)std::min<int64_t>(MQ_TB, a.R - r0);
    mq_mlp_fwd(MGeo<D, 64, MD_A>{}, L{}, L{}, a.P, sm, a.obs + r0 * D, D, D, MD_A, rows, act);
    if ((int)threadIdx.x < rows) {
      const float* q = act + L::Q + threadIdx.x * 8;
      const int64_t r = r0 + threadIdx.x;
      int gi = 0;
      float z[MD_A], mx = 0.0f;
#pragma unroll
      for (int k = 0; k < MD_A; ++k) {
        a.logits[r * MD_A + k] = q[k];
        z[k] = a.gum ? q[k] + a.gum[r * MD_A + k] : q[k];
        if (k == 0 || z[k] > mx) {
          mx = z[k];
          gi = k;
        }
      }
      if (a.onehot) {
#pragma unroll
        for (int k = 0; k < MD_A; ++k) a.onehot[r * MD_A + k] = (a.gum ? k == gi : z[k] == mx) ? 1.0f : 0.0f;
      }
    }
    __syncthreads();
  }
}

// g[(n B + b) A + k] = -log(-log(U + 1e-20) + 1e-20), U = rng_uniform(rng_draw(seed, counter, b, n A + k)). Sums and
// results are f32; each log is evaluated in f64 and rounded, so a host twin reproduces the bits.
__global__ void md_gumbel_kernel(float* g, int N, int B, uint64_t seed, uint64_t counter) {
  const int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (e >= (int64_t)N * B * MD_A) return;
  const int k = (int)(e % MD_A), b = (int)(e / MD_A % B), n = (int)(e / ((int64_t)MD_A * B));
  g[e] = rng_gumbel(rng_draw(seed, counter, (uint64_t)b, (uint64_t)(n * MD_A + k)));
}

int md_blocks(int B) { return std::min((B + MQ_TB - 1) / MQ_TB, MD_MAX_BLOCKS); }
int md_width(const mm_maddpg_dims* d) { return d->n_agents * (d->obs_dim + d->n_actions); }

template <int D>
struct MdShape {
  using GA = MGeo<D, 64, MD_A>;
  using L = MqL<D>;
  static int64_t lds_bytes(int Dc) { return (int64_t)(L::nW + L::nAct + 2 * MQ_TB * (((Dc + 3) & ~3) + 1)) * 4; }

  // the dynamic-LDS attribute of one kernel, set when its size changes (host work off the per-call path)
  static int set_lds(const void* kernel, int bytes, int* last) {
    if (*last == bytes) return MM_OK;
    MM_HIP_CHECK(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
    *last = bytes;
    return MM_OK;
  }
  static int64_t pstride(int64_t total) { return (total + 2 + 15) / 16 * 16; }
  static int64_t sstride(int N) { return ((int64_t)N * MQ_TB * 17 + 15) / 16 * 16; }
  static int64_t ws_floats(const mm_maddpg_dims* d, int B) {
    const int64_t ps = std::max(pstride(GA::total), pstride(md_geo(md_width(d)).total));
    return (int64_t)md_blocks(B) * (ps + sstride(d->n_agents));
  }

  static MdArgs args(const mm_maddpg_dims* d, const mm_maddpg_batch* b, float* ws, int64_t total) {
    MdArgs a = {};
    a.obs = b->obs;
    a.nobs = b->nobs;
    a.cobs = b->cent_obs;
    a.cnobs = b->cent_nobs;
    a.acts = b->acts;
    a.rew = b->rewards;
    a.dn = b->dones_env;
    a.valid = b->valid;
    a.isw = b->is_weight;
    a.pstride = pstride(total);
    a.sstride = sstride(d->n_agents);
    a.part = ws;
    a.scr = ws + md_blocks(b->B) * a.pstride;
    a.cg = md_geo(md_width(d));
    a.B = b->B;
    a.N = d->n_agents;
    a.S = d->n_agents * d->obs_dim;
    a.Dc = md_width(d);
    a.nq = d->td3 ? 2 : 1;
    a.td3 = d->td3;
    a.huber = b->huber;
    a.ntiles = (b->B + MQ_TB - 1) / MQ_TB;
    a.gamma = b->gamma;
    a.delta = b->huber_delta;
    a.eps = b->per_eps;
    a.invB = 1.0f / (float)b->B;
    return a;
  }

  static int critic_grad(const mm_maddpg_dims* d, const mm_maddpg_batch* b, const float* PAT, const float* PC,
                         const float* PCT, float* grad, float* ws, float* stats, float* prio, hipStream_t s) {
    static int lds = -1;
    if (set_lds((const void*)maddpg_critic_kernel<D>, (int)lds_bytes(md_width(d)), &lds)) return MM_EHIP;
    const int64_t tot = md_geo(md_width(d)).total;
    MdArgs a = args(d, b, ws, tot);
    a.PA = PAT;
    a.PC = PC;
    a.PCT = PCT;
    a.gum = b->target_gumbel;
    a.prio = prio;
    const int nblk = md_blocks(b->B);
    hipLaunchKernelGGL((maddpg_critic_kernel<D>), dim3(nblk), dim3(256), (size_t)lds_bytes(a.Dc), s, a);
    MM_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(md_reduce_kernel, dim3((unsigned)((tot + 2 + 255) / 256)), dim3(256), 0, s, ws, a.pstride, nblk,
                       tot, grad, stats, a.invB, 0);
    MM_HIP_CHECK(hipGetLastError());
    return MM_OK;
  }

  static int actor_grad(const mm_maddpg_dims* d, const mm_maddpg_batch* b, const float* PA, const float* PC,
                        float* grad, float* ws, float* stats, hipStream_t s) {
    static int lds = -1;
    if (set_lds((const void*)maddpg_actor_kernel<D>, (int)lds_bytes(md_width(d)), &lds)) return MM_EHIP;
    const int64_t tot = GA::total;
    MdArgs a = args(d, b, ws, tot);
    a.PA = PA;
    a.PC = PC;
    a.gum = b->gumbel;
    const int nblk = md_blocks(b->B);
    hipLaunchKernelGGL((maddpg_actor_kernel<D>), dim3(nblk), dim3(256), (size_t)lds_bytes(a.Dc), s, a);
    MM_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(md_reduce_kernel, dim3((unsigned)((tot + 2 + 255) / 256)), dim3(256), 0, s, ws, a.pstride, nblk,
                       tot, grad, stats, a.invB, 1);
    MM_HIP_CHECK(hipGetLastError());
    return MM_OK;
  }

  static int logits(const mm_maddpg_dims* d, const float* P, const float* obs, const float* gum, float* out,
                    float* onehot, int64_t R, hipStream_t s) {
    static int lds = -1;
    if (set_lds((const void*)maddpg_logits_kernel<D>, L::q_bytes, &lds)) return MM_EHIP;
    MdLogitArgs a = {P, obs, gum, out, onehot, R, (R + MQ_TB - 1) / MQ_TB};
    const int nblk = (int)std::min<int64_t>(a.ntiles, MD_MAX_BLOCKS);
    hipLaunchKernelGGL((maddpg_logits_kernel<D>), dim3(nblk), dim3(256), (size_t)L::q_bytes, s, a);
    MM_HIP_CHECK(hipGetLastError());
    return MM_OK;
  }
};

#define MM_MADDPG_DISPATCH(d, CALL)  \
  do {                               \
    if ((d)->obs_dim == 3) {         \
      using SH = MdShape<3>;         \
      return CALL;                   \
    }                                \
    if ((d)->obs_dim == 47) {        \
      using SH = MdShape<47>;        \
      return CALL;                   \
    }                                \
    using SH = MdShape<94>;          \
    return CALL;                     \
  } while (0)

int64_t md_lds(const mm_maddpg_dims* d) { MM_MADDPG_DISPATCH(d, SH::lds_bytes(md_width(d))); }
int64_t md_ws_floats(const mm_maddpg_dims* d, int B) { MM_MADDPG_DISPATCH(d, SH::ws_floats(d, B)); }
int64_t md_actor_total(const mm_maddpg_dims* d) { MM_MADDPG_DISPATCH(d, SH::GA::total); }

int md_check(const mm_maddpg_dims* d) {
  MM_REQUIRE(d && d->n_agents >= 1, "maddpg: bad dims");
  MM_REQUIRE(d->hidden == 64 && d->n_actions == MD_A && (d->obs_dim == 3 || d->obs_dim == 47 || d->obs_dim == 94),
             "maddpg: unsupported dims D=%d H=%d A=%d (supported: D 3|47|94, H 64, A 5)", d->obs_dim, d->hidden,
             d->n_actions);
  MM_REQUIRE(d->td3 == 0 || d->td3 == 1, "maddpg: td3 must be 0 or 1");
  MM_REQUIRE((int64_t)d->n_agents * (d->obs_dim + d->n_actions) <= MM_MADDPG_MAX_CRITIC_WIDTH,
             "maddpg: critic input width N (D + A) = %lld is above the limit of %d",
             (long long)d->n_agents * (d->obs_dim + d->n_actions), MM_MADDPG_MAX_CRITIC_WIDTH);
  MM_REQUIRE(md_lds(d) <= MD_LDS_LIMIT, "maddpg: %lld bytes of LDS needed, %d available", (long long)md_lds(d),
             MD_LDS_LIMIT);
  return MM_OK;
}

}  // namespace
}  // namespace mm

extern "C" {

int mm_maddpg_param_counts(const mm_maddpg_dims* d, int64_t* actor, int64_t* critic, int64_t* critic_heads) {
  int rc = mm::md_check(d);
  if (rc) return rc;
  MM_REQUIRE(actor && critic && critic_heads, "maddpg_param_counts: null argument");
  const mm::MdGeo g = mm::md_geo(mm::md_width(d));
  *actor = mm::md_actor_total(d);
  *critic = g.total;
  *critic_heads = g.Wo;
  return MM_OK;
}

int64_t mm_maddpg_workspace_bytes(const mm_maddpg_dims* d, int32_t B) {
  if (mm::md_check(d) || B < 1) return -1;
  return mm::md_ws_floats(d, B) * 4;
}

int mm_maddpg_critic_grad(const mm_maddpg_dims* d, const mm_maddpg_batch* b, const float* PA_target, const float* PC,
                          const float* PC_target, float* grad, void* ws, int64_t ws_bytes, float* stats,
                          float* priorities, mm_stream_t s) {
  int rc = mm::md_check(d);
  if (rc) return rc;
  MM_REQUIRE(b && PA_target && PC && PC_target && grad && ws && stats, "maddpg_critic_grad: null argument");
  MM_REQUIRE(b->nobs && b->cent_obs && b->cent_nobs && b->acts && b->rewards && b->dones_env,
             "maddpg_critic_grad: batch arrays missing");
  MM_REQUIRE(!d->td3 || b->target_gumbel, "maddpg_critic_grad: matd3 needs target_gumbel");
  MM_REQUIRE(b->B >= 1, "maddpg_critic_grad: B must be >= 1");
  MM_REQUIRE(!b->is_weight || priorities, "maddpg_critic_grad: PER (is_weight) needs a priorities output");
  const int64_t need = mm_maddpg_workspace_bytes(d, b->B);
  MM_REQUIRE(need > 0 && ws_bytes >= need, "maddpg_critic_grad: workspace %lld bytes < %lld", (long long)ws_bytes,
             (long long)need);
  using namespace mm;
  MM_MADDPG_DISPATCH(d, SH::critic_grad(d, b, PA_target, PC, PC_target, grad, (float*)ws, stats, priorities,
                                        (hipStream_t)s));
}

int mm_maddpg_actor_grad(const mm_maddpg_dims* d, const mm_maddpg_batch* b, const float* PA, const float* PC,
                         float* grad, void* ws, int64_t ws_bytes, float* stats, mm_stream_t s) {
  int rc = mm::md_check(d);
  if (rc) return rc;
  MM_REQUIRE(b && PA && PC && grad && ws && stats, "maddpg_actor_grad: null argument");
  MM_REQUIRE(b->obs && b->cent_obs && b->acts && b->valid && b->gumbel, "maddpg_actor_grad: batch arrays missing");
  MM_REQUIRE(b->B >= 1, "maddpg_actor_grad: B must be >= 1");
  const int64_t need = mm_maddpg_workspace_bytes(d, b->B);
  MM_REQUIRE(need > 0 && ws_bytes >= need, "maddpg_actor_grad: workspace %lld bytes < %lld", (long long)ws_bytes,
             (long long)need);
  using namespace mm;
  MM_MADDPG_DISPATCH(d, SH::actor_grad(d, b, PA, PC, grad, (float*)ws, stats, (hipStream_t)s));
}

int mm_maddpg_logits(const mm_maddpg_dims* d, const float* PA, const float* obs, const float* gumbel, float* logits,
                     float* onehot, int64_t R, mm_stream_t s) {
  int rc = mm::md_check(d);
  if (rc) return rc;
  MM_REQUIRE(PA && obs && logits && R >= 1, "maddpg_logits: bad args");
  using namespace mm;
  MM_MADDPG_DISPATCH(d, SH::logits(d, PA, obs, gumbel, logits, onehot, R, (hipStream_t)s));
}

int mm_maddpg_gumbel(const mm_maddpg_dims* d, float* g, int32_t B, uint64_t seed, uint64_t counter, mm_stream_t s) {
  int rc = mm::md_check(d);
  if (rc) return rc;
  MM_REQUIRE(g && B >= 1, "maddpg_gumbel: bad args");
  const int64_t n = (int64_t)d->n_agents * B * mm::MD_A;
  hipLaunchKernelGGL(mm::md_gumbel_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)s, g,
                     d->n_agents, B, seed, counter);
  MM_HIP_CHECK(hipGetLastError());
  return MM_OK;
}

}  // extern "C"
