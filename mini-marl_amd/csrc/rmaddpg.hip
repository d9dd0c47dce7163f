// Recurrent MADDPG / MATD3 trainer ("rmaddpg" / "rmatd3") of the reference's offpolicy fork on gfx950:
// R_MADDPG.shared_train_policy_on_batch (offpolicy/algorithms/r_maddpg/r_maddpg.py:114-331) with R_MADDPGPolicy
// (algorithm/rMADDPGPolicy.py), discrete actions, one shared policy, episodes from h = 0.
//
//   actor   RNNBase(D) -> Linear(64, A): LN -> Linear -> ReLU -> LN -> Linear -> ReLU -> LN -> GRU -> LN -> head, the
//           18-tensor trunk layout (trunk.h) with an 8-row Wo slot.
//   critic  the same trunk over x = [share_obs | acts], width Dc = N (D + A) (a runtime value), nq = 1 | 2 trained
//           Linear(64, 1) heads in a 4-row Wo slot.
//
// Work split. Everything in front of the GRU has no time dependence, the GRU itself is latency:
//   rm_front_fwd_kernel   16 row-steps per tile: the input row is assembled in LDS (obs; or share_obs | stored acts,
//                         with some agents' A columns replaced by the one-hot of actor logits (+ Gumbel noise)), then
//                         LN0 .. LN2 and gi = W_ih x + b_ih, every Linear on v_mfma_f32_16x16x4_f32 (mq_tile.h), the
//                         weights streamed from L2 as B operands at every width. One runtime-width kernel serves the
//                         actor (D) and the critic (Dc).
//   rm_rec_kernel<MODE>   one wave per sequence, lane j = hidden unit j, its three W_hh rows in 192 VGPRs for the whole
//                         episode, h broadcast through a wave-private LDS slot, no barrier in the time loop. ONE
//                         W_hh h + b_hh product per step serves the chain cell and every side cell that starts from the
//                         same state: PLAIN (chain, LN_r and the heads in the wave), TARGET (side cell on x'_t from
//                         h_t, min over heads), SIDE (N side cells from h_{t-1} on the replaced inputs, head 0, and
//                         their backward down to dL/dgi in the same wave: h is a constant there).
//   rm_loss_kernel        targets, masked errors, loss, R2D2 priorities, dL/dQ (one block, fixed-order sums).
//   rm_rec_bwd_kernel     reverse-time BPTT per sequence, W_hh columns in VGPRs; LN_r and the heads are re-derived
//                         from h_t in the wave. Leaves dgi, dgh_n and the head / LN_r operands per row-step.
//   rm_front_bwd_kernel   per tile: the front forward again (into LDS), dL/dx2 = dgi W_ih, then either the weight
//                         gradients of all 18 tensors into a block-private partial in tile order (wgrad), or the
//                         input-only backward through the Dc-wide LN0 down to agent i's A columns, softmax backward,
//                         dL/dlogits of the actor (actor pass).
//   rm_reduce_kernel      grad[e] = sum of the block partials in block order. No float atomics: same bits every run.
// LDS: 2 x 16 x (ceil4(width) + 1) input rows + 10 x 16 x 65 activations + 0.3 K floats: Dc 16 45 KB, Dc 104 56 KB,
// Dc 198 68 KB, Dc 416 96 KB of 160 KB.
#include <algorithm>

#include "common.h"
#include "minimarl.h"
#include "mq_tile.h"

namespace mm {
namespace {

constexpr int RM_MAX_BLOCKS = 256;
constexpr int RM_A = 5, RM_H = 64, RM_G = 192;
enum { RM_PLAIN = 0, RM_TARGET = 1, RM_SIDE = 2 };

// the trunk layout with runtime input width din and nout head rows
struct RGeo {
  int Dp, Op, ln0_w, ln0_b, W1, b1, ln1_w, ln1_b, W2, b2, ln2_w, ln2_b, Wih, Whh, bih, bhh, lnr_w, lnr_b, Wo, bo, total;
};
__host__ __device__ inline RGeo rm_geo(int din, int nout) {
  RGeo g;
  const int H = RM_H;
  g.Dp = (din + 3) & ~3;
  g.Op = (nout + 3) & ~3;
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
  g.Wih = g.ln2_b + H;
  g.Whh = g.Wih + 3 * H * H;
  g.bih = g.Whh + 3 * H * H;
  g.bhh = g.bih + 3 * H;
  g.lnr_w = g.bhh + 3 * H;
  g.lnr_b = g.lnr_w + H;
  g.Wo = g.lnr_b + H;
  g.bo = g.Wo + g.Op * H;
  g.total = g.bo + g.Op;
  return g;
}
struct RWL {
  int wW1, ldw1, wW2, ldw2, wWo;
};
// LDS carve-up (floats); G0 reuses F0
struct RL {
  int ld0, ldh, F0, XH0, G0, A1, XH1, F1, A2, XH2, F2, G1, G2, Q, DO, RS, nAct;
};
__host__ __device__ inline RL rm_lds(int Dp) {
  RL l;
  l.ld0 = Dp + 1;
  l.ldh = 65;
  l.F0 = 0;
  l.XH0 = l.F0 + MQ_TB * l.ld0;
  l.G0 = l.F0;
  l.A1 = l.XH0 + MQ_TB * l.ld0;
  l.XH1 = l.A1 + MQ_TB * l.ldh;
  l.F1 = l.XH1 + MQ_TB * l.ldh;
  l.A2 = l.F1 + MQ_TB * l.ldh;
  l.XH2 = l.A2 + MQ_TB * l.ldh;
  l.F2 = l.XH2 + MQ_TB * l.ldh;
  l.G1 = l.F2 + MQ_TB * l.ldh;
  l.G2 = l.G1 + MQ_TB * l.ldh;
  l.Q = l.G2 + MQ_TB * l.ldh;
  l.DO = l.Q + MQ_TB * 8;
  l.RS = l.DO + MQ_TB * 8;
  l.nAct = l.RS + 3 * MQ_TB;
  return l;
}

// ------------------------------------------------------------------ input rows
// kind 0 (actor): row r = t NB + n B + b of obs [N, T+1, B, D] (stacked: obs [R, D] as it is).
// kind 1 (critic): row r = i T B + t B + b: [share_obs[t + shift, b] | acts[:, t, b]], where the A columns of every
// agent (replace 1), of agent i (replace 2) or of nobody (replace 0; i = 0) hold the one-hot of the actor logits
// [T (+1)][NB][8] at step t + shift instead: argmax of logits + gum[n, t, b] (first maximum), or logits == rowmax.
struct RmSrc {
  const float* obs; const float* cent; const float* acts; const float* logits; const float* gum;
  int kind, stacked, shift, replace, T, B, N, D, S;
};

__device__ __forceinline__ float rm_onehot(const float* l, const float* g, int k) {
  if (g) {
    int gi = 0;
    float best = l[0] + g[0];
#pragma unroll
    for (int c = 1; c < RM_A; ++c) {
      const float z = l[c] + g[c];
      if (z > best) {
        best = z;
        gi = c;
      }
    }
    return k == gi ? 1.0f : 0.0f;
  }
  float mx = l[0];
#pragma unroll
  for (int c = 1; c < RM_A; ++c) mx = fmaxf(mx, l[c]);
  return l[k] == mx ? 1.0f : 0.0f;
}

__device__ __forceinline__ void rm_fill(const RmSrc& s, float* X, int ld, int64_t r0, int rows) {
  const int NB = s.N * s.B;
  if (s.kind == 0) {
    for (int e = threadIdx.x; e < rows * s.D; e += blockDim.x) {
      const int i = e / s.D, c = e - i * s.D;
      const int64_t r = r0 + i;
      int64_t src = r;
      if (!s.stacked) {
        const int64_t t = r / NB, q = r - t * NB, n = q / s.B, b = q - n * s.B;
        src = (n * (s.T + 1) + t) * s.B + b;
      }
      X[i * ld + c] = s.obs[src * s.D + c];
    }
    return;
  }
  const int64_t TB = (int64_t)s.T * s.B;
  for (int e = threadIdx.x; e < rows * s.S; e += blockDim.x) {
    const int i = e / s.S, c = e - i * s.S;
    const int64_t tb = (r0 + i) % TB;
    X[i * ld + c] = s.cent[(tb + (int64_t)s.shift * s.B) * s.S + c];
  }
  const int NA = s.N * RM_A;
  for (int e = threadIdx.x; e < rows * NA; e += blockDim.x) {
    const int i = e / NA, c = e - i * NA, n = c / RM_A, k = c - n * RM_A;
    const int64_t r = r0 + i, ag = r / TB, tb = r - ag * TB, t = tb / s.B, b = tb - t * s.B;
    const int64_t at = ((int64_t)n * s.T + t) * s.B + b;
    float v;
    if (s.replace == 1 || (s.replace == 2 && n == (int)ag))
      v = rm_onehot(s.logits + (((t + s.shift) * NB + (int64_t)n * s.B + b) * 8), s.gum ? s.gum + at * RM_A : nullptr, k);
    else
      v = s.acts[at * RM_A + k];
    X[i * ld + s.S + c] = v;
  }
}

// ------------------------------------------------------------------ front layers, forward
struct RmFrontArgs {
  const float* P;
  RGeo g;
  RL l;
  RmSrc src;
  float* gi;   // [R][192]
  int64_t R, ntiles;
  int din;
};

__global__ __launch_bounds__(256) void rm_front_fwd_kernel(RmFrontArgs a) {
  extern __shared__ __attribute__((aligned(16))) float act[];
  const RGeo g = a.g;
  const RL l = a.l;
  const RWL wl = {g.W1, g.Dp, g.W2, 64, g.Wo};
  const float* P = a.P;
  for (int64_t tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
    const int64_t r0 = tile * MQ_TB;
    const int rows = (int)std::min<int64_t>(MQ_TB, a.R - r0);
    rm_fill(a.src, act + l.F0, l.ld0, r0, rows);
    __syncthreads();
    mq_mlp_fwd(g, wl, l, P, P, act + l.F0, l.ld0, a.din, 0, rows, act);
    float* gi = a.gi + r0 * RM_G;
    mq_gemm(act + l.F2, l.ldh, false, rows, P + g.Wih, 64, 1, RM_G, 64,
            [&](int i, int n, float v) { gi[i * RM_G + n] = v + P[g.bih + n]; });
    __syncthreads();
  }
}

// ------------------------------------------------------------------ GRU recurrence
__device__ __forceinline__ float rm_rl(float v, int i) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), i));
}
template <int CTRL>
__device__ __forceinline__ float rm_dpp(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, false));
}
// full-wave sum, the same value in every lane
__device__ __forceinline__ float rm_wsum(float v) {
  v += rm_dpp<0xB1>(v);
  v += rm_dpp<0x4E>(v);
  v += rm_dpp<0x124>(v);
  v += rm_dpp<0x128>(v);
  return (rm_rl(v, 0) + rm_rl(v, 16)) + (rm_rl(v, 32) + rm_rl(v, 48));
}

struct RmRecArgs {
  const float* P;
  RGeo g;
  const float* gi;      // chain inputs [L][Q][192]
  const float* gis;     // side inputs: TARGET [L][Q][192], SIDE [N][L][Q][192]
  const float* h0;      // [Q][64] or NULL (zeros)
  const float* dones;   // SIDE: per-agent dones [N][L][Q]
  const float* gum;     // PLAIN, onehot given: [Q][A] or NULL
  float* hs;            // [(L + 1)][Q][64]: block 0 = the initial state, block t + 1 = h_t; or NULL
  float* gates;         // [L][Q][4][64] (r, z, n, W_hn h + b_hn) or NULL
  float* out;           // PLAIN: head outputs [L][Q][8]; TARGET: min_k q' [L][Q]; SIDE: Q^i [N][L][Q]
  float* dgis;          // SIDE: dL/dgi of the side cells [N][L][Q][192], seeded with dL/dQ^i = -(1 - acurr_i)
  float* hout;          // [Q][64] or NULL
  float* onehot;        // PLAIN: [Q][A] of the LAST step (callers pass it with L == 1), or NULL
  int L, Q, N, nout;
};

// one wave per sequence q; lane j owns hidden unit j
template <int MODE>
__global__ __launch_bounds__(256) void rm_rec_kernel(RmRecArgs a) {
  constexpr int H = RM_H;
  const int q = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (q >= a.Q) return;
  const int j = threadIdx.x & 63;
  const float* P = a.P;
  const RGeo g = a.g;
  float wr[H], wz[H], wn[H];
#pragma unroll
  for (int i = 0; i < H; ++i) {
    wr[i] = P[g.Whh + j * H + i];
    wz[i] = P[g.Whh + (H + j) * H + i];
    wn[i] = P[g.Whh + (2 * H + j) * H + i];
  }
  const float br = P[g.bhh + j], bz = P[g.bhh + H + j], bn = P[g.bhh + 2 * H + j];
  const float lnw = P[g.lnr_w + j], lnb = P[g.lnr_b + j];
  float wo[RM_A], bo[RM_A];
#pragma unroll
  for (int k = 0; k < RM_A; ++k) {
    wo[k] = k < a.nout ? P[g.Wo + k * H + j] : 0.0f;
    bo[k] = k < a.nout ? P[g.bo + k] : 0.0f;
  }
  __shared__ __attribute__((aligned(16))) float sm[4][64];
  float* slot = sm[threadIdx.x >> 6];
  float h = a.h0 ? a.h0[(int64_t)q * H + j] : 0.0f;
  if (a.hs) a.hs[(int64_t)q * H + j] = h;
  float ar, az, an;   // W_hh h + b_hh of the current state
  // LN_r and the heads of a 64-vector held one element per lane
  auto head = [&](float v, float& xh, float& rs, float (&qk)[RM_A]) {
    const float mu = rm_wsum(v) * (1.0f / H);
    const float d = v - mu;
    rs = 1.0f / sqrtf(rm_wsum(d * d) * (1.0f / H) + kLnEps);
    xh = d * rs;
    const float y = xh * lnw + lnb;
#pragma unroll
    for (int k = 0; k < RM_A; ++k) {   // nout is wave-uniform: the critic's 1 or 2 heads pay 1 or 2 wave sums
      qk[k] = 0.0f;
      if (k < a.nout) qk[k] = rm_wsum(wo[k] * y) + bo[k];
    }
  };
  const int steps = MODE == RM_TARGET ? a.L + 1 : a.L;
  for (int t = 0; t < steps; ++t) {
    float gr = 0.f, gz = 0.f, gn = 0.f;
    if (t < a.L) {
      const float* gp = a.gi + ((int64_t)t * a.Q + q) * RM_G + j;
      gr = gp[0];
      gz = gp[H];
      gn = gp[2 * H];
    }
    slot[j] = h;
    __builtin_amdgcn_wave_barrier();
    {
      float ar0 = br, az0 = bz, an0 = bn, ar1 = 0.f, az1 = 0.f, an1 = 0.f;
#pragma unroll
      for (int c = 0; c < H / 4; ++c) {
        const float4 t4 = reinterpret_cast<const float4*>(slot)[c];
        ar0 = fmaf(wr[4 * c], t4.x, ar0);
        az0 = fmaf(wz[4 * c], t4.x, az0);
        an0 = fmaf(wn[4 * c], t4.x, an0);
        ar1 = fmaf(wr[4 * c + 1], t4.y, ar1);
        az1 = fmaf(wz[4 * c + 1], t4.y, az1);
        an1 = fmaf(wn[4 * c + 1], t4.y, an1);
        ar0 = fmaf(wr[4 * c + 2], t4.z, ar0);
        az0 = fmaf(wz[4 * c + 2], t4.z, az0);
        an0 = fmaf(wn[4 * c + 2], t4.z, an0);
        ar1 = fmaf(wr[4 * c + 3], t4.w, ar1);
        az1 = fmaf(wz[4 * c + 3], t4.w, az1);
        an1 = fmaf(wn[4 * c + 3], t4.w, an1);
      }
      ar = ar0 + ar1;
      az = az0 + az1;
      an = an0 + an1;
    }
    __builtin_amdgcn_wave_barrier();
    if (MODE == RM_TARGET && t >= 1) {
      const float* sp = a.gis + ((int64_t)(t - 1) * a.Q + q) * RM_G + j;
      const float rr = sigmoidf_(sp[0] + ar), zz = sigmoidf_(sp[H] + az), nn = tanhf_(sp[2 * H] + rr * an);
      float xh, rs, qk[RM_A];
      head(nn + zz * (h - nn), xh, rs, qk);
      if (j == 0) a.out[(int64_t)(t - 1) * a.Q + q] = a.nout > 1 ? fminf(qk[0], qk[1]) : qk[0];
    }
    if (MODE == RM_SIDE) {
      for (int i = 0; i < a.N; ++i) {
        const int64_t r = ((int64_t)i * a.L + t) * a.Q + q;
        const float* sp = a.gis + r * RM_G + j;
        const float rr = sigmoidf_(sp[0] + ar), zz = sigmoidf_(sp[H] + az), nn = tanhf_(sp[2 * H] + rr * an);
        float xh, rs, qk[RM_A];
        head(nn + zz * (h - nn), xh, rs, qk);
        if (j == 0) a.out[r] = qk[0];
        // backward from dL/dQ = -(1 - acurr) to the cell's input projections (h is a constant of this cell)
        const float dq = t > 0 ? a.dones[r - a.Q] - 1.0f : -1.0f;
        const float gg = dq * wo[0] * lnw;
        const float sg = rm_wsum(gg) * (1.0f / H), sgx = rm_wsum(gg * xh) * (1.0f / H);
        const float dhs = rs * (gg - sg - xh * sgx);
        const float dpn = dhs * (1.0f - zz) * (1.0f - nn * nn);
        float* o = a.dgis + r * RM_G + j;
        o[0] = dpn * an * rr * (1.0f - rr);
        o[H] = dhs * (h - nn) * zz * (1.0f - zz);
        o[2 * H] = dpn;
      }
    }
    if (t < a.L) {
      const int64_t r = (int64_t)t * a.Q + q;
      const float rr = sigmoidf_(gr + ar), zz = sigmoidf_(gz + az), nn = tanhf_(gn + rr * an);
      h = nn + zz * (h - nn);
      if (a.hs) a.hs[(r + a.Q) * H + j] = h;
      if (a.gates) {
        float* gt = a.gates + r * 4 * H;
        gt[j] = rr;
        gt[H + j] = zz;
        gt[2 * H + j] = nn;
        gt[3 * H + j] = an;
      }
      if (MODE == RM_PLAIN) {
        float xh, rs, qk[RM_A];
        head(h, xh, rs, qk);
        float mine = 0.0f;
#pragma unroll
        for (int k = 0; k < RM_A; ++k) mine = j == k ? qk[k] : mine;
        if (j < 8) a.out[r * 8 + j] = j < a.nout ? mine : 0.0f;
        if (a.onehot && t == a.L - 1 && j < RM_A) {
          float z[RM_A];
#pragma unroll
          for (int k = 0; k < RM_A; ++k) z[k] = qk[k];
          a.onehot[(int64_t)q * RM_A + j] = rm_onehot(z, a.gum ? a.gum + (int64_t)q * RM_A : nullptr, j);
        }
      }
    }
  }
  if (a.hout) a.hout[(int64_t)q * H + j] = h;
}

// ------------------------------------------------------------------ critic loss
struct RmLossArgs {
  const float* q;       // live critic [T B][8]
  const float* minq;    // [T B]
  const float* rew;     // agent 0 [T B]
  const float* de;      // [T B]
  const float* isw;     // [B] or NULL
  float* dout;          // [T B][8]
  float* prio;          // [B] or NULL
  float* stats;
  int T, B, nq, huber;
  float gamma, delta, eps, nu;
};

// fixed-shape tree over 256 threads: the same order every run
__device__ __forceinline__ float rm_block_sum(float v, float* sh) {
  sh[threadIdx.x] = v;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) sh[threadIdx.x] += sh[threadIdx.x + s];
    __syncthreads();
  }
  const float r = sh[0];
  __syncthreads();
  return r;
}

__global__ __launch_bounds__(256) void rm_loss_kernel(RmLossArgs a) {
  __shared__ float sh[256];
  const int tid = threadIdx.x, TB = a.T * a.B;
  float cnt = 0.0f;
  for (int e = tid; e < TB; e += 256) cnt += e < a.B ? 1.0f : 1.0f - a.de[e - a.B];
  const float M = rm_block_sum(cnt, sh);
  float loss = 0.0f;
  for (int b = tid; b < a.B; b += 256) {
    const float w = a.isw ? a.isw[b] : 1.0f;
    float sa[2] = {0.f, 0.f}, ma[2] = {0.f, 0.f};
    for (int t = 0; t < a.T; ++t) {
      const int e = t * a.B + b;
      const float m = t > 0 ? 1.0f - a.de[e - a.B] : 1.0f;
      const float tg = (a.rew[e] + a.gamma * (1.0f - a.de[e]) * a.minq[e]) * m;
      for (int k = 0; k < a.nq; ++k) {
        const float er = a.q[e * 8 + k] * m - tg;
        const float ae = fabsf(er);
        float f, df;
        if (a.huber) {
          f = ae <= a.delta ? er * er / 2.0f : a.delta * (ae - a.delta / 2.0f);
          df = ae <= a.delta ? er : (er > 0.0f ? a.delta : -a.delta);
        } else {
          f = er * er;
          df = 2.0f * er;
        }
        loss += w * f;
        a.dout[e * 8 + k] = w * df * m / M;
        sa[k] += ae;
        ma[k] = fmaxf(ma[k], ae);
      }
    }
    if (a.prio) {
      float p = 0.0f;
      for (int k = 0; k < a.nq; ++k) p += (1.0f - a.nu) * (sa[k] / (float)a.T) + a.nu * ma[k] + a.eps;
      a.prio[b] = p / (float)a.nq + a.eps;
    }
  }
  const float L = rm_block_sum(loss, sh);
  if (tid == 0) {
    a.stats[0] = L / M;
    a.stats[1] = M;
  }
}

// ------------------------------------------------------------------ BPTT
struct RmRecBwdArgs {
  const float* P;
  RGeo g;
  const float* hs;      // [(L + 1)][Q][64]
  const float* gates;   // [L][Q][4][64]
  const float* dout;    // dL/d(head outputs) [L][Q][8]
  float* dgi;           // [L Q][192]
  float* dghn;          // [L Q][64]
  float* yr; float* dyr; float* xhr;   // LN_r output, its gradient, xhat_r [L Q][64]
  int L, Q, nout;
};

__global__ __launch_bounds__(256) void rm_rec_bwd_kernel(RmRecBwdArgs a) {
  constexpr int H = RM_H;
  const int q = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (q >= a.Q) return;
  const int j = threadIdx.x & 63;
  const float* P = a.P;
  const RGeo g = a.g;
  // column j of W_hh
  float wr[H], wz[H], wn[H];
#pragma unroll
  for (int k = 0; k < H; ++k) {
    wr[k] = P[g.Whh + k * H + j];
    wz[k] = P[g.Whh + (H + k) * H + j];
    wn[k] = P[g.Whh + (2 * H + k) * H + j];
  }
  const float lnw = P[g.lnr_w + j], lnb = P[g.lnr_b + j];
  float wo[RM_A];
#pragma unroll
  for (int k = 0; k < RM_A; ++k) wo[k] = k < a.nout ? P[g.Wo + k * H + j] : 0.0f;
  __shared__ __attribute__((aligned(16))) float sm[4][3 * 64];
  float* slot = sm[threadIdx.x >> 6];
  float dnext = 0.0f;
  for (int t = a.L - 1; t >= 0; --t) {
    const int64_t r = (int64_t)t * a.Q + q;
    const float ht = a.hs[(r + a.Q) * H + j], hin = a.hs[r * H + j];
    const float* gt = a.gates + r * 4 * H;
    const float rr = gt[j], zz = gt[H + j], nn = gt[2 * H + j], ghn = gt[3 * H + j];
    // heads and LN_r
    const float mu = rm_wsum(ht) * (1.0f / H);
    const float dv = ht - mu;
    const float rs = 1.0f / sqrtf(rm_wsum(dv * dv) * (1.0f / H) + kLnEps);
    const float xh = dv * rs;
    float dy = 0.0f;
#pragma unroll
    for (int k = 0; k < RM_A; ++k)
      if (k < a.nout) dy = fmaf(a.dout[r * 8 + k], wo[k], dy);
    a.yr[r * H + j] = xh * lnw + lnb;
    a.dyr[r * H + j] = dy;
    a.xhr[r * H + j] = xh;
    const float gg = dy * lnw;
    const float sg = rm_wsum(gg) * (1.0f / H), sgx = rm_wsum(gg * xh) * (1.0f / H);
    const float dh = rs * (gg - sg - xh * sgx) + dnext;
    const float dz = dh * (hin - nn);
    const float dpn = dh * (1.0f - zz) * (1.0f - nn * nn);
    const float dgr = dpn * ghn * rr * (1.0f - rr);
    const float dgz = dz * zz * (1.0f - zz);
    const float dghn = dpn * rr;
    float* o = a.dgi + r * RM_G;
    o[j] = dgr;
    o[H + j] = dgz;
    o[2 * H + j] = dpn;
    a.dghn[r * H + j] = dghn;
    slot[j] = dgr;
    slot[64 + j] = dgz;
    slot[128 + j] = dghn;
    __builtin_amdgcn_wave_barrier();
    float acc0 = dh * zz, acc1 = 0.0f, acc2 = 0.0f;
#pragma unroll
    for (int c = 0; c < H / 4; ++c) {
      const float4 tr = reinterpret_cast<const float4*>(slot)[c], tz = reinterpret_cast<const float4*>(slot)[16 + c],
                   tn = reinterpret_cast<const float4*>(slot)[32 + c];
      const float vr[4] = {tr.x, tr.y, tr.z, tr.w}, vz[4] = {tz.x, tz.y, tz.z, tz.w}, vn[4] = {tn.x, tn.y, tn.z, tn.w};
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        acc0 = fmaf(wr[4 * c + u], vr[u], acc0);
        acc1 = fmaf(wz[4 * c + u], vz[u], acc1);
        acc2 = fmaf(wn[4 * c + u], vn[u], acc2);
      }
    }
    __builtin_amdgcn_wave_barrier();
    dnext = acc0 + acc1 + acc2;
  }
}

// ------------------------------------------------------------------ front layers, backward
// from G2 = dL/d(F2) in LDS down to G0 = dL/d(F0): mq_mlp_bwd without its head
__device__ __forceinline__ void rm_mlp_bwd(const RGeo& g, const RWL& wl, const RL& l, const float* __restrict__ P,
                                           int din, int rows, bool wgrad, float* act, float* part) {
  float* G2 = act + l.G2;
  float* G1 = act + l.G1;
  float* G0 = act + l.G0;
  if (wgrad) {
    mq_colsum(G2, l.ldh, act + l.XH2, l.ldh, rows, 64, part + g.ln2_w);
    mq_colsum(G2, l.ldh, nullptr, 0, rows, 64, part + g.ln2_b);
  }
  __syncthreads();
  mq_ln_bwd(G2, act + l.XH2, act + l.A2, act + l.RS + 2 * MQ_TB, P + g.ln2_w, rows, 64, l.ldh);
  __syncthreads();
  if (wgrad) {
    mq_wgrad(G2, l.ldh, act + l.F1, l.ldh, false, rows, 64, 64, part + g.W2, 64);
    mq_colsum(G2, l.ldh, nullptr, 0, rows, 64, part + g.b2);
  }
  mq_gemm(G2, l.ldh, false, rows, P + wl.wW2, 1, wl.ldw2, 64, 64, [&](int i, int k, float v) { G1[i * l.ldh + k] = v; });
  __syncthreads();
  if (wgrad) {
    mq_colsum(G1, l.ldh, act + l.XH1, l.ldh, rows, 64, part + g.ln1_w);
    mq_colsum(G1, l.ldh, nullptr, 0, rows, 64, part + g.ln1_b);
  }
  __syncthreads();
  mq_ln_bwd(G1, act + l.XH1, act + l.A1, act + l.RS + MQ_TB, P + g.ln1_w, rows, 64, l.ldh);
  __syncthreads();
  if (wgrad) {
    mq_wgrad(G1, l.ldh, act + l.F0, l.ld0, false, rows, 64, din, part + g.W1, g.Dp);
    mq_colsum(G1, l.ldh, nullptr, 0, rows, 64, part + g.b1);
  }
  __syncthreads();   // G0 is F0
  mq_gemm(G1, l.ldh, false, rows, P + wl.wW1, 1, wl.ldw1, din, 64, [&](int i, int k, float v) { G0[i * l.ld0 + k] = v; });
  __syncthreads();
  if (wgrad) {
    mq_colsum(G0, l.ld0, act + l.XH0, l.ld0, rows, din, part + g.ln0_w);
    mq_colsum(G0, l.ld0, nullptr, 0, rows, din, part + g.ln0_b);
  }
  __syncthreads();
}

struct RmBwdArgs {
  const float* P;
  RGeo g;
  RL l;
  RmSrc src;
  const float* dgi;     // [R][192]
  // wgrad mode
  const float* dghn; const float* hprev; const float* dout; const float* yr; const float* dyr; const float* xhr;
  float* part;
  int64_t pstride;
  // input-only mode (actor pass; rows i T B + t B + b)
  const float* qside;   // [R]
  const float* dones;   // [N][T][B]
  float* dlog;          // dL/dlogits of the actor [T][N B][8]
  float* lv;            // [blocks][2]: sum Q (1 - acurr), sum (1 - acurr)
  int64_t R, ntiles;
  int din, nout, wgrad;
};

__global__ __launch_bounds__(256) void rm_front_bwd_kernel(RmBwdArgs a) {
  extern __shared__ __attribute__((aligned(16))) float act[];
  const RGeo g = a.g;
  const RL l = a.l;
  const RWL wl = {g.W1, g.Dp, g.W2, 64, g.Wo};
  const float* P = a.P;
  const int tid = threadIdx.x;
  float* part = a.wgrad ? a.part + blockIdx.x * a.pstride : nullptr;
  if (a.wgrad)
    for (int64_t e = tid; e < a.pstride; e += blockDim.x) part[e] = 0.0f;
  float loss_acc = 0.0f, v_acc = 0.0f;   // thread 0
  __syncthreads();
  for (int64_t tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
    const int64_t r0 = tile * MQ_TB;
    const int rows = (int)std::min<int64_t>(MQ_TB, a.R - r0);
    rm_fill(a.src, act + l.F0, l.ld0, r0, rows);
    __syncthreads();
    mq_mlp_fwd(g, wl, l, P, P, act + l.F0, l.ld0, a.din, 0, rows, act);
    const float* dgi = a.dgi + r0 * RM_G;
    float* G2 = act + l.G2;
    mq_gemm(dgi, RM_G, false, rows, P + g.Wih, 1, 64, 64, RM_G, [&](int i, int k, float v) { G2[i * l.ldh + k] = v; });
    if (a.wgrad) {
      const float* dghn = a.dghn + r0 * 64;
      const float* hp = a.hprev + r0 * 64;
      const float* dout = a.dout + r0 * 8;
      mq_wgrad(dgi, RM_G, act + l.F2, l.ldh, false, rows, RM_G, 64, part + g.Wih, 64);
      mq_colsum(dgi, RM_G, nullptr, 0, rows, RM_G, part + g.bih);
      mq_wgrad(dgi, RM_G, hp, 64, false, rows, 128, 64, part + g.Whh, 64);
      mq_wgrad(dghn, 64, hp, 64, false, rows, 64, 64, part + g.Whh + 128 * 64, 64);
      mq_colsum(dgi, RM_G, nullptr, 0, rows, 128, part + g.bhh);
      mq_colsum(dghn, 64, nullptr, 0, rows, 64, part + g.bhh + 128);
      mq_wgrad(dout, 8, a.yr + r0 * 64, 64, false, rows, a.nout, 64, part + g.Wo, 64);
      mq_colsum(dout, 8, nullptr, 0, rows, a.nout, part + g.bo);
      mq_colsum(a.dyr + r0 * 64, 64, a.xhr + r0 * 64, 64, rows, 64, part + g.lnr_w);
      mq_colsum(a.dyr + r0 * 64, 64, nullptr, 0, rows, 64, part + g.lnr_b);
    }
    __syncthreads();
    rm_mlp_bwd(g, wl, l, P, a.din, rows, a.wgrad != 0, act, part);
    if (!a.wgrad) {
      // LN0 backward over the full width, kept for the A columns of this row's agent; then the softmax
      const RmSrc& s = a.src;
      const int64_t TB = (int64_t)s.T * s.B;
      const int NB = s.N * s.B;
      {
        const int row = tid >> 4, sub = tid & 15;
        const bool ok = row < rows;
        const int ag = ok ? (int)((r0 + row) / TB) : 0;
        const float* G0 = act + l.G0 + row * l.ld0;
        const float* XH = act + l.XH0 + row * l.ld0;
        const float* gw = P + g.ln0_w;
        float sg = 0.f, sgx = 0.f;
        for (int c = sub; c < a.din; c += 16) {
          const float gg = ok ? G0[c] * gw[c] : 0.f;
          sg += gg;
          sgx = fmaf(gg, ok ? XH[c] : 0.f, sgx);
        }
        sg = sum16(sg) / (float)a.din;
        sgx = sum16(sgx) / (float)a.din;
        if (ok && sub < RM_A) {
          const int c = s.S + ag * RM_A + sub;
          act[l.DO + row * 8 + sub] = act[l.RS + row] * (G0[c] * gw[c] - sg - XH[c] * sgx);
        }
      }
      __syncthreads();
      if (tid < rows) {
        const int64_t r = r0 + tid, ag = r / TB, tb = r - ag * TB, t = tb / s.B, b = tb - t * s.B;
        const int64_t lr = t * NB + ag * s.B + b;
        const float* lg = s.logits + lr * 8;
        const float* gm = s.gum + ((ag * s.T + t) * s.B + b) * RM_A;
        const float* dy = act + l.DO + tid * 8;
        float z[RM_A], best = lg[0] + gm[0], sum = 0.0f, dot = 0.0f;
#pragma unroll
        for (int k = 0; k < RM_A; ++k) {
          z[k] = lg[k] + gm[k];
          best = fmaxf(best, z[k]);
        }
#pragma unroll
        for (int k = 0; k < RM_A; ++k) {
          z[k] = expf(z[k] - best);
          sum += z[k];
        }
#pragma unroll
        for (int k = 0; k < RM_A; ++k) {
          z[k] /= sum;
          dot = fmaf(z[k], dy[k], dot);
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) a.dlog[lr * 8 + k] = k < RM_A ? z[k] * (dy[k] - dot) : 0.0f;
        const float v = t > 0 ? 1.0f - a.dones[(ag * s.T + t - 1) * s.B + b] : 1.0f;
        act[l.Q + tid * 8] = a.qside[r] * v;
        act[l.Q + tid * 8 + 1] = v;
      }
      __syncthreads();
      if (tid == 0)
        for (int i = 0; i < rows; ++i) {
          loss_acc += act[l.Q + i * 8];
          v_acc += act[l.Q + i * 8 + 1];
        }
      __syncthreads();
    }
  }
  if (!a.wgrad && tid == 0) {
    a.lv[blockIdx.x * 2] = loss_acc;
    a.lv[blockIdx.x * 2 + 1] = v_acc;
  }
}

// grad[e] = sum of the block partials in block order. lv (actor pass): V = sum (1 - acurr), grad / V,
// stats = {-(sum Q (1 - acurr)) / V, V}.
__global__ __launch_bounds__(256) void rm_reduce_kernel(const float* __restrict__ part, int64_t pstride, int nblk,
                                                        int64_t total, float* __restrict__ grad,
                                                        const float* __restrict__ lv, int nlv,
                                                        float* __restrict__ stats) {
  const int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (e >= total) return;
  float s = 0.0f;
  for (int b = 0; b < nblk; ++b) s += part[b * pstride + e];
  if (lv) {
    float V = 0.0f, ls = 0.0f;
    for (int b = 0; b < nlv; ++b) {
      ls += lv[2 * b];
      V += lv[2 * b + 1];
    }
    s /= V;
    if (e == 0) {
      stats[0] = -ls / V;
      stats[1] = V;
    }
  }
  grad[e] = s;
}

// ------------------------------------------------------------------ host side
int64_t al16(int64_t x) { return (x + 15) / 16 * 16; }
int rm_width(const mm_maddpg_dims* d) { return d->n_agents * (d->obs_dim + d->n_actions); }
int rm_nq(const mm_maddpg_dims* d) { return d->td3 ? 2 : 1; }
int rm_tile_blocks(int64_t R) { return (int)std::min<int64_t>((R + MQ_TB - 1) / MQ_TB, RM_MAX_BLOCKS); }

struct RmWs {
  int64_t giA, logA, hsA, gatesA, giX, giS, hsC, gatesC, qout, minq, qside, dgi, dghn, yr, dyr, xhr, dout, lv, part,
      pstride, total;
};
RmWs rm_ws(const mm_maddpg_dims* d, int T, int B) {
  const int64_t N = d->n_agents, NB = N * B, TB = (int64_t)T * B, R1 = (T + 1) * NB, RA = T * NB;
  RmWs w;
  int64_t o = 0;
  auto take = [&](int64_t n) {
    const int64_t at = o;
    o += al16(n);
    return at;
  };
  w.giA = take(R1 * RM_G);
  w.logA = take(R1 * 8);
  w.hsA = take(R1 * 64);
  w.gatesA = take(RA * 256);
  w.giX = take(TB * RM_G);
  w.giS = take(RA * RM_G);
  w.hsC = take((T + 1) * (int64_t)B * 64);
  w.gatesC = take(TB * 256);
  w.qout = take(TB * 8);
  w.minq = take(TB);
  w.qside = take(RA);
  w.dgi = take(RA * RM_G);
  w.dghn = take(RA * 64);
  w.yr = take(RA * 64);
  w.dyr = take(RA * 64);
  w.xhr = take(RA * 64);
  w.dout = take(RA * 8);
  w.lv = take(2 * RM_MAX_BLOCKS);
  w.pstride = al16(std::max(rm_geo(d->obs_dim, RM_A).total, rm_geo(rm_width(d), rm_nq(d)).total));
  w.part = take(RM_MAX_BLOCKS * w.pstride);
  w.total = o;
  return w;
}

// the dynamic-LDS limit of a kernel, set on the current device at every launch (per-device state; no host cache)
int rm_set_lds(const void* kernel, int bytes) {
  MM_HIP_CHECK(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
  return MM_OK;
}

int rm_front_fwd(const float* P, int din, int nout, const RmSrc& src, float* gi, int64_t R, hipStream_t s) {
  RmFrontArgs a = {};
  a.P = P;
  a.g = rm_geo(din, nout);
  a.l = rm_lds(a.g.Dp);
  a.src = src;
  a.gi = gi;
  a.R = R;
  a.ntiles = (R + MQ_TB - 1) / MQ_TB;
  a.din = din;
  const int bytes = a.l.nAct * 4;
  if (rm_set_lds((const void*)rm_front_fwd_kernel, bytes)) return MM_EHIP;
  hipLaunchKernelGGL(rm_front_fwd_kernel, dim3(rm_tile_blocks(R)), dim3(256), (size_t)bytes, s, a);
  MM_HIP_CHECK(hipGetLastError());
  return MM_OK;
}

int rm_front_bwd(RmBwdArgs& a, const float* P, int din, int nout, const RmSrc& src, int64_t R, hipStream_t s) {
  a.P = P;
  a.g = rm_geo(din, nout);
  a.l = rm_lds(a.g.Dp);
  a.src = src;
  a.R = R;
  a.ntiles = (R + MQ_TB - 1) / MQ_TB;
  a.din = din;
  a.nout = nout;
  const int bytes = a.l.nAct * 4;
  if (rm_set_lds((const void*)rm_front_bwd_kernel, bytes)) return MM_EHIP;
  hipLaunchKernelGGL(rm_front_bwd_kernel, dim3(rm_tile_blocks(R)), dim3(256), (size_t)bytes, s, a);
  MM_HIP_CHECK(hipGetLastError());
  return MM_OK;
}

template <int MODE>
int rm_rec(const RmRecArgs& a, hipStream_t s) {
  hipLaunchKernelGGL((rm_rec_kernel<MODE>), dim3((a.Q + 3) / 4), dim3(256), 0, s, a);
  MM_HIP_CHECK(hipGetLastError());
  return MM_OK;
}

RmSrc rm_actor_src(const mm_maddpg_dims* d, const mm_rmaddpg_batch* b) {
  RmSrc s = {};
  s.obs = b->obs;
  s.T = b->T;
  s.B = b->B;
  s.N = d->n_agents;
  s.D = d->obs_dim;
  return s;
}
RmSrc rm_critic_src(const mm_maddpg_dims* d, const mm_rmaddpg_batch* b, int shift, int replace, const float* logits,
                    const float* gum) {
  RmSrc s = {};
  s.kind = 1;
  s.cent = b->share_obs;
  s.acts = b->acts;
  s.logits = logits;
  s.gum = gum;
  s.shift = shift;
  s.replace = replace;
  s.T = b->T;
  s.B = b->B;
  s.N = d->n_agents;
  s.D = d->obs_dim;
  s.S = d->n_agents * d->obs_dim;
  return s;
}

// BPTT, the weight-gradient tiles and the reduction of one net whose forward saves are in hs / gates
int rm_net_bwd(const float* P, int din, int nout, const RmSrc& src, const RmWs& w, float* ws, const float* hs,
               const float* gates, int L, int Q, float* grad, const float* lv, int nlv, float* stats, hipStream_t s) {
  RmRecBwdArgs rb = {P, rm_geo(din, nout), hs, gates, ws + w.dout, ws + w.dgi, ws + w.dghn, ws + w.yr, ws + w.dyr,
                     ws + w.xhr, L, Q, nout};
  hipLaunchKernelGGL(rm_rec_bwd_kernel, dim3((Q + 3) / 4), dim3(256), 0, s, rb);
  MM_HIP_CHECK(hipGetLastError());
  const int64_t R = (int64_t)L * Q;
  RmBwdArgs fb = {};
  fb.dgi = ws + w.dgi;
  fb.dghn = ws + w.dghn;
  fb.hprev = hs;
  fb.dout = ws + w.dout;
  fb.yr = ws + w.yr;
  fb.dyr = ws + w.dyr;
  fb.xhr = ws + w.xhr;
  fb.part = ws + w.part;
  fb.pstride = w.pstride;
  fb.wgrad = 1;
  if (rm_front_bwd(fb, P, din, nout, src, R, s)) return MM_EHIP;
  const int64_t tot = rb.g.total;
  hipLaunchKernelGGL(rm_reduce_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, s, ws + w.part, w.pstride,
                     rm_tile_blocks(R), tot, grad, lv, nlv, stats);
  MM_HIP_CHECK(hipGetLastError());
  return MM_OK;
}

int rm_critic_grad(const mm_maddpg_dims* d, const mm_rmaddpg_batch* b, const float* PAT, const float* PC,
                   const float* PCT, float* grad, float* ws, float* stats, float* prio, hipStream_t s) {
  const int N = d->n_agents, T = b->T, B = b->B, NB = N * B, D = d->obs_dim, Dc = rm_width(d), nq = rm_nq(d);
  const int64_t TB = (int64_t)T * B;
  const RmWs w = rm_ws(d, T, B);
  // target actions: the target actor over all T + 1 steps
  if (rm_front_fwd(PAT, D, RM_A, rm_actor_src(d, b), ws + w.giA, (int64_t)(T + 1) * NB, s)) return MM_EHIP;
  RmRecArgs ra = {};
  ra.P = PAT;
  ra.g = rm_geo(D, RM_A);
  ra.gi = ws + w.giA;
  ra.out = ws + w.logA;
  ra.L = T + 1;
  ra.Q = NB;
  ra.N = N;
  ra.nout = RM_A;
  if (rm_rec<RM_PLAIN>(ra, s)) return MM_EHIP;
  // target critic: chain on x_t, side cell on x'_t
  const RmSrc x = rm_critic_src(d, b, 0, 0, nullptr, nullptr);
  if (rm_front_fwd(PCT, Dc, nq, x, ws + w.giX, TB, s)) return MM_EHIP;
  if (rm_front_fwd(PCT, Dc, nq, rm_critic_src(d, b, 1, 1, ws + w.logA, d->td3 ? b->target_gumbel : nullptr),
                   ws + w.giS, TB, s))
    return MM_EHIP;
  RmRecArgs rt = {};
  rt.P = PCT;
  rt.g = rm_geo(Dc, nq);
  rt.gi = ws + w.giX;
  rt.gis = ws + w.giS;
  rt.out = ws + w.minq;
  rt.L = T;
  rt.Q = B;
  rt.N = N;
  rt.nout = nq;
  if (rm_rec<RM_TARGET>(rt, s)) return MM_EHIP;
  // live critic
  if (rm_front_fwd(PC, Dc, nq, x, ws + w.giX, TB, s)) return MM_EHIP;
  RmRecArgs rc = rt;
  rc.P = PC;
  rc.gis = nullptr;
  rc.hs = ws + w.hsC;
  rc.gates = ws + w.gatesC;
  rc.out = ws + w.qout;
  if (rm_rec<RM_PLAIN>(rc, s)) return MM_EHIP;
  RmLossArgs la = {ws + w.qout, ws + w.minq, b->rewards, b->dones_env, b->is_weight, ws + w.dout,
                   b->is_weight ? prio : nullptr, stats, T, B, nq, b->huber, b->gamma, b->huber_delta, b->per_eps,
                   b->per_nu};
  hipLaunchKernelGGL(rm_loss_kernel, dim3(1), dim3(256), 0, s, la);
  MM_HIP_CHECK(hipGetLastError());
  return rm_net_bwd(PC, Dc, nq, x, w, ws, ws + w.hsC, ws + w.gatesC, T, B, grad, nullptr, 0, stats, s);
}

int rm_actor_grad(const mm_maddpg_dims* d, const mm_rmaddpg_batch* b, const float* PA, const float* PC, float* grad,
                  float* ws, float* stats, hipStream_t s) {
  const int N = d->n_agents, T = b->T, B = b->B, NB = N * B, D = d->obs_dim, Dc = rm_width(d), nq = rm_nq(d);
  const int64_t TB = (int64_t)T * B, RA = (int64_t)T * NB;
  const RmWs w = rm_ws(d, T, B);
  const RmSrc ao = rm_actor_src(d, b);
  if (rm_front_fwd(PA, D, RM_A, ao, ws + w.giA, RA, s)) return MM_EHIP;
  RmRecArgs ra = {};
  ra.P = PA;
  ra.g = rm_geo(D, RM_A);
  ra.gi = ws + w.giA;
  ra.hs = ws + w.hsA;
  ra.gates = ws + w.gatesA;
  ra.out = ws + w.logA;
  ra.L = T;
  ra.Q = NB;
  ra.N = N;
  ra.nout = RM_A;
  if (rm_rec<RM_PLAIN>(ra, s)) return MM_EHIP;
  // the updated critic: chain on x_t, N side cells per step on the replaced inputs, backward to their gi
  const RmSrc xr = rm_critic_src(d, b, 0, 2, ws + w.logA, b->gumbel);
  if (rm_front_fwd(PC, Dc, nq, rm_critic_src(d, b, 0, 0, nullptr, nullptr), ws + w.giX, TB, s)) return MM_EHIP;
  if (rm_front_fwd(PC, Dc, nq, xr, ws + w.giS, RA, s)) return MM_EHIP;
  RmRecArgs rs = {};
  rs.P = PC;
  rs.g = rm_geo(Dc, nq);
  rs.gi = ws + w.giX;
  rs.gis = ws + w.giS;
  rs.dones = b->dones;
  rs.out = ws + w.qside;
  rs.dgis = ws + w.dgi;
  rs.L = T;
  rs.Q = B;
  rs.N = N;
  rs.nout = 1;
  if (rm_rec<RM_SIDE>(rs, s)) return MM_EHIP;
  // input-only backward of the side cells' front layers -> dL/dlogits
  RmBwdArgs fb = {};
  fb.dgi = ws + w.dgi;
  fb.qside = ws + w.qside;
  fb.dones = b->dones;
  fb.dlog = ws + w.dout;
  fb.lv = ws + w.lv;
  if (rm_front_bwd(fb, PC, Dc, nq, xr, RA, s)) return MM_EHIP;
  return rm_net_bwd(PA, D, RM_A, ao, w, ws, ws + w.hsA, ws + w.gatesA, T, NB, grad, ws + w.lv, rm_tile_blocks(RA), stats,
                    s);
}

int rm_check(const mm_maddpg_dims* d) {
  MM_REQUIRE(d && d->n_agents >= 1, "rmaddpg: bad dims");
  MM_REQUIRE(d->hidden == 64 && d->n_actions == RM_A && (d->obs_dim == 3 || d->obs_dim == 47 || d->obs_dim == 94),
             "rmaddpg: unsupported dims D=%d H=%d A=%d (supported: D 3|47|94, H 64, A 5)", d->obs_dim, d->hidden,
             d->n_actions);
  MM_REQUIRE(d->td3 == 0 || d->td3 == 1, "rmaddpg: td3 must be 0 or 1");
  MM_REQUIRE((int64_t)d->n_agents * (d->obs_dim + d->n_actions) <= MM_MADDPG_MAX_CRITIC_WIDTH,
             "rmaddpg: critic input width N (D + A) = %lld is above the limit of %d",
             (long long)d->n_agents * (d->obs_dim + d->n_actions), MM_MADDPG_MAX_CRITIC_WIDTH);
  return MM_OK;
}

}  // namespace
}  // namespace mm

extern "C" {

int mm_rmaddpg_param_counts(const mm_maddpg_dims* d, int64_t* actor, int64_t* critic) {
  int rc = mm::rm_check(d);
  if (rc) return rc;
  MM_REQUIRE(actor && critic, "rmaddpg_param_counts: null argument");
  *actor = mm::rm_geo(d->obs_dim, mm::RM_A).total;
  *critic = mm::rm_geo(mm::rm_width(d), mm::rm_nq(d)).total;
  return MM_OK;
}

int64_t mm_rmaddpg_workspace_bytes(const mm_maddpg_dims* d, int32_t T, int32_t B) {
  if (mm::rm_check(d) || T < 1 || B < 1) return -1;
  if ((int64_t)T * B * d->n_agents > (1 << 24)) return -1;   // row-step indices stay far inside 32 bits
  return mm::rm_ws(d, T, B).total * 4;
}

int mm_rmaddpg_critic_grad(const mm_maddpg_dims* d, const mm_rmaddpg_batch* b, const float* PA_target, const float* PC,
                           const float* PC_target, float* grad, void* ws, int64_t ws_bytes, float* stats,
                           float* priorities, mm_stream_t s) {
  int rc = mm::rm_check(d);
  if (rc) return rc;
  MM_REQUIRE(b && PA_target && PC && PC_target && grad && ws && stats, "rmaddpg_critic_grad: null argument");
  MM_REQUIRE(b->obs && b->share_obs && b->acts && b->rewards && b->dones_env,
             "rmaddpg_critic_grad: batch arrays missing");
  MM_REQUIRE(!d->td3 || b->target_gumbel, "rmaddpg_critic_grad: rmatd3 needs target_gumbel");
  MM_REQUIRE(!b->is_weight || priorities, "rmaddpg_critic_grad: PER (is_weight) needs a priorities output");
  const int64_t need = mm_rmaddpg_workspace_bytes(d, b->T, b->B);
  MM_REQUIRE(need > 0 && ws_bytes >= need, "rmaddpg_critic_grad: workspace %lld bytes < %lld (T %d, B %d)",
             (long long)ws_bytes, (long long)need, b->T, b->B);
  return mm::rm_critic_grad(d, b, PA_target, PC, PC_target, grad, (float*)ws, stats, priorities, (hipStream_t)s);
}

int mm_rmaddpg_actor_grad(const mm_maddpg_dims* d, const mm_rmaddpg_batch* b, const float* PA, const float* PC,
                          float* grad, void* ws, int64_t ws_bytes, float* stats, mm_stream_t s) {
  int rc = mm::rm_check(d);
  if (rc) return rc;
  MM_REQUIRE(b && PA && PC && grad && ws && stats, "rmaddpg_actor_grad: null argument");
  MM_REQUIRE(b->obs && b->share_obs && b->acts && b->dones && b->gumbel, "rmaddpg_actor_grad: batch arrays missing");
  const int64_t need = mm_rmaddpg_workspace_bytes(d, b->T, b->B);
  MM_REQUIRE(need > 0 && ws_bytes >= need, "rmaddpg_actor_grad: workspace %lld bytes < %lld (T %d, B %d)",
             (long long)ws_bytes, (long long)need, b->T, b->B);
  return mm::rm_actor_grad(d, b, PA, PC, grad, (float*)ws, stats, (hipStream_t)s);
}

int mm_rmaddpg_step(const mm_maddpg_dims* d, const float* PA, const float* obs, const float* h_in, const float* gumbel,
                    float* logits, float* onehot, float* h_out, float* scratch, int64_t R, mm_stream_t s) {
  int rc = mm::rm_check(d);
  if (rc) return rc;
  MM_REQUIRE(PA && obs && logits && h_out && scratch && R >= 1 && R <= (1 << 24), "rmaddpg_step: bad args");
  using namespace mm;
  RmSrc src = {};
  src.obs = obs;
  src.stacked = 1;
  src.D = d->obs_dim;
  src.N = 1;
  src.B = (int)R;
  if (rm_front_fwd(PA, d->obs_dim, RM_A, src, scratch, R, (hipStream_t)s)) return MM_EHIP;
  RmRecArgs ra = {};
  ra.P = PA;
  ra.g = rm_geo(d->obs_dim, RM_A);
  ra.gi = scratch;
  ra.h0 = h_in;
  ra.gum = gumbel;
  ra.out = logits;
  ra.hout = h_out;
  ra.onehot = onehot;
  ra.L = 1;
  ra.Q = (int)R;
  ra.N = 1;
  ra.nout = RM_A;
  return rm_rec<RM_PLAIN>(ra, (hipStream_t)s);
}

}  // extern "C"
