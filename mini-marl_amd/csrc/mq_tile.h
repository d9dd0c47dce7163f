// 16-row tile helpers of the feed-forward transition-batch trainers (moffq.hip: mqmix / mvdn; maddpg.hip: maddpg /
// matd3): exact-fp32 MFMA GEMM, weight gradient and column sums over a tile, LayerNorm forward / backward of any
// width, and the forward / backward of one LN-MLP net (MLPBase with layer_N = 1 plus a Linear head) over a 16-row
// chunk whose activations live in LDS.
//
// The net helpers take three descriptions by value: the parameter geometry g (offsets into the flat vector: MGeo or a
// runtime-width twin), the weight placement wl (wW1 / wW2 / wWo offsets into w and the row strides ldw1 / ldw2: a
// staged LDS copy or the flat vector itself, streamed from L2 as MFMA B operands) and the activation carve-up l. A
// description is either a struct of static constexpr members (compile-time shapes: everything folds) or one with
// runtime members (the centralized critic's input width).
#pragma once
#include "common.h"
#include "trunk.h"

namespace mm {

typedef float f32x4 __attribute__((ext_vector_type(4)));
constexpr int MQ_TB = 16;           // transitions per tile = rows of one MFMA tile

// v_mfma_f32_16x16x4_f32: A[i = lane & 15][k = lane >> 4], B[k = lane >> 4][j = lane & 15],
// D reg r of lane (j, g = lane >> 4): row 4 g + r, column j
__device__ __forceinline__ f32x4 mfma16(float a, float b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

// C(i, n) = sum_k X[i ldx + k] W[n ldn + k ldk] for i < rows (<= 16), n < ncols; epi(i, n, C). One 16-column tile
// per wave and pass. X and W may be LDS or global. relu_x: max(X, 0) on load.
template <typename Epi>
__device__ __forceinline__ void mq_gemm(const float* X, int64_t ldx, bool relu_x, int rows, const float* W,
                                        int64_t ldn, int64_t ldk, int ncols, int kdim, Epi epi) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, j = lane & 15, g = lane >> 4;
  const bool rok = j < rows;
  const float* xp = X + j * ldx;
  for (int n0 = wave * 16; n0 < ncols; n0 += 64) {
    const bool nok = n0 + j < ncols;
    const float* wp = W + (n0 + j) * ldn;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < kdim; k0 += 4) {
      const int k = k0 + g;
      float av = (rok && k < kdim) ? xp[k] : 0.f;
      if (relu_x) av = fmaxf(av, 0.f);
      const float bv = (nok && k < kdim) ? wp[k * ldk] : 0.f;
      acc = mfma16(av, bv, acc);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (4 * g + r < rows && nok) epi(4 * g + r, n0 + j, acc[r]);
  }
}

// out[m ldo + k] += sum_{r < rows} dY[r ldy + m] X[r ldx + k] for m < M, k < Kc: the tile's rows on the MFMA k
// dimension. An output element always belongs to the same lane of the same wave, which adds into the block-private
// partial in tile order.
__device__ __forceinline__ void mq_wgrad(const float* dY, int64_t ldy, const float* X, int64_t ldx, bool relu_x,
                                         int rows, int M, int Kc, float* out, int64_t ldo) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, j = lane & 15, g = lane >> 4;
  const int MT = (M + 15) >> 4, KT = (Kc + 15) >> 4;
  for (int t = wave; t < MT * KT; t += 4) {
    const int m0 = (t / KT) * 16, k0 = (t % KT) * 16;
    const bool mok = m0 + j < M, kok = k0 + j < Kc;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int r0 = 0; r0 < MQ_TB; r0 += 4) {
      const int r = r0 + g;
      const float av = (r < rows && mok) ? dY[r * ldy + m0 + j] : 0.f;
      float bv = (r < rows && kok) ? X[r * ldx + k0 + j] : 0.f;
      if (relu_x) bv = fmaxf(bv, 0.f);
      acc = mfma16(av, bv, acc);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int m = m0 + 4 * g + r;
      if (m < M && kok) out[m * ldo + k0 + j] += acc[r];
    }
  }
}

// out[m] += sum_{r < rows} dY[r ldy + m] (* X[r ldx + m]) in row order
__device__ __forceinline__ void mq_colsum(const float* dY, int64_t ldy, const float* X, int64_t ldx, int rows, int M,
                                          float* out) {
  for (int m = threadIdx.x; m < M; m += blockDim.x) {
    float s = 0.f;
    for (int r = 0; r < rows; ++r) s += X ? dY[r * ldy + m] * X[r * ldx + m] : dY[r * ldy + m];
    out[m] += s;
  }
}

__device__ __forceinline__ float sum16(float v) {
  v += __shfl_xor(v, 1);
  v += __shfl_xor(v, 2);
  v += __shfl_xor(v, 4);
  v += __shfl_xor(v, 8);
  return v;
}

// LayerNorm of 16 rows, 16 lanes per row: Y = xhat gw + gb, XH = xhat, rs[row]. X may be Y or XH themselves (in
// place, ldx == ld): every element is read and written by the same lane.
__device__ __forceinline__ void mq_ln(const float* X, int64_t ldx, int rows, int ncols, const float* gw,
                                      const float* gb, float* Y, float* XH, int ld, float* rs_out) {
  const int row = threadIdx.x >> 4, sub = threadIdx.x & 15;
  const bool ok = row < rows;
  const float* xp = X + row * ldx;
  float s = 0.f;
  for (int c = sub; c < ncols; c += 16) s += ok ? xp[c] : 0.f;
  const float mu = sum16(s) / (float)ncols;
  float v = 0.f;
  for (int c = sub; c < ncols; c += 16) {
    const float d = ok ? xp[c] - mu : 0.f;
    v = fmaf(d, d, v);
  }
  const float rs = 1.0f / sqrtf(sum16(v) / (float)ncols + kLnEps);
  if (!ok) return;
  for (int c = sub; c < ncols; c += 16) {
    const float xh = (xp[c] - mu) * rs;
    XH[row * ld + c] = xh;
    Y[row * ld + c] = xh * gw[c] + gb[c];
  }
  if (sub == 0) rs_out[row] = rs;
}

// In place: G = dL/dy of a LayerNorm over ncols columns -> dL/dx: rs (g - mean g - xhat mean(g xhat)), g = dy gw.
// Aact: the output of the ReLU in front of the LayerNorm (the result is zero where it is 0), or nullptr for a
// LayerNorm over plain inputs.
__device__ __forceinline__ void mq_ln_bwd(float* G, const float* XH, const float* Aact, const float* rs,
                                          const float* gw, int rows, int ncols, int ld) {
  const int row = threadIdx.x >> 4, sub = threadIdx.x & 15;
  const bool ok = row < rows;
  float sg = 0.f, sgx = 0.f;
  for (int c = sub; c < ncols; c += 16) {
    const float gg = ok ? G[row * ld + c] * gw[c] : 0.f;
    sg += gg;
    sgx = fmaf(gg, ok ? XH[row * ld + c] : 0.f, sgx);
  }
  sg = sum16(sg) / (float)ncols;
  sgx = sum16(sgx) / (float)ncols;
  if (!ok) return;
  for (int c = sub; c < ncols; c += 16) {
    const float dx = rs[row] * (G[row * ld + c] * gw[c] - sg - XH[row * ld + c] * sgx);
    G[row * ld + c] = (!Aact || Aact[row * ld + c] > 0.0f) ? dx : 0.0f;
  }
}

// LDS carve-up (floats) of a net with a compile-time input width. Row strides are odd: 16 rows of one column fall
// into 16 different banks.
template <int D>
struct MqL {
  static constexpr int Dp = (D + 3) & ~3, ld0 = Dp + 1, ldh = 65;
  static constexpr int ldw1 = ld0, ldw2 = ldh;                                                  // staged weights
  static constexpr int wW1 = 0, wW2 = wW1 + 64 * ld0, wWo = wW2 + 64 * ldh, nW = wWo + 8 * ldh;  // one net's weights
  static constexpr int F0 = 0, XH0 = F0 + MQ_TB * ld0, G0 = XH0 + MQ_TB * ld0;
  static constexpr int A1 = G0 + MQ_TB * ld0, XH1 = A1 + MQ_TB * ldh, F1 = XH1 + MQ_TB * ldh;
  static constexpr int A2 = F1 + MQ_TB * ldh, XH2 = A2 + MQ_TB * ldh, F2 = XH2 + MQ_TB * ldh;
  static constexpr int G1 = F2 + MQ_TB * ldh, G2 = G1 + MQ_TB * ldh;
  static constexpr int Q = G2 + MQ_TB * ldh, DO = Q + MQ_TB * 8, RS = DO + MQ_TB * 8;   // RS: rs0, rs1, rs2 [16] each
  static constexpr int DQ = RS + 3 * MQ_TB, LS = DQ + MQ_TB, QT = LS + MQ_TB, ARG = QT + 2 * MQ_TB;
  static constexpr int nAct = ARG + MQ_TB;
  static constexpr int train_bytes = (2 * nW + nAct) * 4, q_bytes = (nW + nAct) * 4;
};

template <int D, int H, int A>
__device__ __forceinline__ void mq_stage(float* w, const float* __restrict__ P) {
  using G = MGeo<D, H, A>;
  using L = MqL<D>;
  for (int e = threadIdx.x; e < 64 * G::Dp; e += blockDim.x)
    w[L::wW1 + (e / G::Dp) * L::ld0 + e % G::Dp] = P[G::W1 + e];
  for (int e = threadIdx.x; e < 64 * 64; e += blockDim.x) w[L::wW2 + (e >> 6) * L::ldh + (e & 63)] = P[G::W2 + e];
  for (int e = threadIdx.x; e < G::Op * 64; e += blockDim.x) w[L::wWo + (e >> 6) * L::ldh + (e & 63)] = P[G::Wo + e];
}

// Forward of one net over a 16-row chunk x (row stride ldx, width din; global, or the F0 rows themselves): leaves F0
// XH0 A1 XH1 F1 A2 XH2 F2 RS and the nout head outputs Q [16][8] in LDS. 64 hidden units: one 16-column MFMA tile
// per wave. Ends with a barrier.
template <class G, class WL, class L>
__device__ __forceinline__ void mq_mlp_fwd(const G g, const WL wl, const L l, const float* __restrict__ P,
                                           const float* w, const float* x, int64_t ldx, int din, int nout, int rows,
                                           float* act) {
  mq_ln(x, ldx, rows, din, P + g.ln0_w, P + g.ln0_b, act + l.F0, act + l.XH0, l.ld0, act + l.RS);
  __syncthreads();
  mq_gemm(act + l.F0, l.ld0, false, rows, w + wl.wW1, wl.ldw1, 1, 64, din,
          [&](int i, int n, float v) { act[l.A1 + i * l.ldh + n] = fmaxf(v + P[g.b1 + n], 0.0f); });
  __syncthreads();
  mq_ln(act + l.A1, l.ldh, rows, 64, P + g.ln1_w, P + g.ln1_b, act + l.F1, act + l.XH1, l.ldh, act + l.RS + MQ_TB);
  __syncthreads();
  mq_gemm(act + l.F1, l.ldh, false, rows, w + wl.wW2, wl.ldw2, 1, 64, 64,
          [&](int i, int n, float v) { act[l.A2 + i * l.ldh + n] = fmaxf(v + P[g.b2 + n], 0.0f); });
  __syncthreads();
  mq_ln(act + l.A2, l.ldh, rows, 64, P + g.ln2_w, P + g.ln2_b, act + l.F2, act + l.XH2, l.ldh,
        act + l.RS + 2 * MQ_TB);
  __syncthreads();
  mq_gemm(act + l.F2, l.ldh, false, rows, w + wl.wWo, wl.ldw2, 1, nout, 64,
          [&](int i, int n, float v) { act[l.Q + i * 8 + n] = v + P[g.bo + n]; });
  __syncthreads();
}

// Backward of the chunk whose forward is in LDS, from dL/d(head outputs) in DO [16][8] (written and fenced by the
// caller) down to G0 = dL/d(F0). wgrad: add the chunk's weight gradients (W1 W2 b1 b2 and the three LayerNorms) into
// part, laid out by g; head_grad: the head's Wo / bo too. l.G0 may be l.F0 (then F0 is consumed first). Ends with a
// barrier.
template <class G, class WL, class L>
__device__ __forceinline__ void mq_mlp_bwd(const G g, const WL wl, const L l, const float* __restrict__ P,
                                           const float* w, int din, int nout, int rows, bool head_grad, bool wgrad,
                                           float* act, float* part) {
  float* dO = act + l.DO;
  float* G2 = act + l.G2;
  float* G1 = act + l.G1;
  float* G0 = act + l.G0;
  if (head_grad) {
    mq_wgrad(dO, 8, act + l.F2, l.ldh, false, rows, nout, 64, part + g.Wo, 64);
    mq_colsum(dO, 8, nullptr, 0, rows, nout, part + g.bo);
  }
  mq_gemm(dO, 8, false, rows, w + wl.wWo, 1, wl.ldw2, 64, nout, [&](int i, int k, float v) { G2[i * l.ldh + k] = v; });
  __syncthreads();
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
  mq_gemm(G2, l.ldh, false, rows, w + wl.wW2, 1, wl.ldw2, 64, 64, [&](int i, int k, float v) { G1[i * l.ldh + k] = v; });
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
  if (l.G0 == l.F0) __syncthreads();
  mq_gemm(G1, l.ldh, false, rows, w + wl.wW1, 1, wl.ldw1, din, 64, [&](int i, int k, float v) { G0[i * l.ld0 + k] = v; });
  __syncthreads();
  if (wgrad) {
    mq_colsum(G0, l.ld0, act + l.XH0, l.ld0, rows, din, part + g.ln0_w);
    mq_colsum(G0, l.ld0, nullptr, 0, rows, din, part + g.ln0_b);
  }
  __syncthreads();
}

}  // namespace mm
