// QMIX / VDN learner: the per-element math and the per-row layouts that every launch shape of learner.hip shares.
// The GRU cell (Mix_Net's GRU over the state and the agents' GRU: forward gates, backward gate gradients), the
// hypernet mixing (y_pre, b2, Q_tot: qmix/_network.py:199-217) and its deltas, and the mixer's save / delta rows.
// Plain per-element code: no LDS staging, no barrier, no launch geometry. A caller brings its own loop, its own
// LDS copies (their layouts differ per kernel) and its own synchronisation. Every launch shape is bit-identical to
// the others because all of them evaluate these expressions; keep an expression's shape when editing one (the
// including file compiles with fp contraction off).
#pragma once
#include "common.h"

namespace mm {

// ------------------------------------------------------------------ row layouts
// One mixer save row, written by the forward per (t, b): the GRU's h_in, gates and W_hn h + b_hn (anh), the new
// hidden, then the hypernet outputs [w1raw (N*K1) | b1 | w2raw | relu(b2 hidden)] (relu'd: the b2 weight gradient
// needs it, and its mask relu(x) > 0 equals x > 0), the mixing pre-activation and the b2 output.
// P: float* / const float* (a view of the row at that base, in global memory or in LDS) or int (P(0): the offsets).
template <typename P>
struct MixSaveRow {
  P hm0, r, z, n, anh, h1, w1raw, b1, w2raw, b2pre, ypre, b2, end;
  __host__ __device__ __forceinline__ MixSaveRow(P p, int Hm, int K1, int N)
      : hm0(p), r(hm0 + Hm), z(r + Hm), n(z + Hm), anh(n + Hm), h1(anh + Hm), w1raw(h1 + Hm), b1(w1raw + N * K1),
        w2raw(b1 + K1), b2pre(w2raw + K1), ypre(b2pre + K1), b2(ypre + K1), end(b2 + 1) {}
};
// One mixer delta row, written by the backward per (t, b): the U operands of the weight-gradient reductions.
template <typename P>
struct MixDeltaRow {
  P dgi, dgh, d_w1, d_b1, d_w2, d_b2pre, dQ, end;   // [3Hm] [3Hm] [N*K1] [K1] [K1] [K1] [1]
  __host__ __device__ __forceinline__ MixDeltaRow(P p, int Hm, int K1, int N)
      : dgi(p), dgh(dgi + 3 * Hm), d_w1(dgh + 3 * Hm), d_b1(d_w1 + N * K1), d_w2(d_b1 + K1), d_b2pre(d_w2 + K1),
        dQ(d_b2pre + K1), end(dQ + 1) {}
};
__host__ __device__ inline int mix_save_dim(int Hm, int K1, int N) { return MixSaveRow<int>(0, Hm, K1, N).end; }
__host__ __device__ inline int mix_delta_dim(int Hm, int K1, int N) { return MixDeltaRow<int>(0, Hm, K1, N).end; }

// ------------------------------------------------------------------ GRU cell
struct GruFwd {
  float r, z, n, h1;
};
// gi_* = W_i* x + b_i*, gh_* = W_h* h0 + b_h*;  h1 = n + z (h0 - n)
__device__ __forceinline__ GruFwd gru_cell_fwd(float gi_r, float gi_z, float gi_n, float gh_r, float gh_z,
                                               float gh_n, float h0) {
  GruFwd c;
  c.r = sigmoidf_(gi_r + gh_r);
  c.z = sigmoidf_(gi_z + gh_z);
  c.n = tanhf_(gi_n + c.r * gh_n);
  c.h1 = c.n + c.z * (h0 - c.n);
  return c;
}
__device__ __forceinline__ void store_gru_save(const MixSaveRow<float*>& row, int i, float h0, float gh_n,
                                               const GruFwd& c) {
  row.hm0[i] = h0;
  row.r[i] = c.r;
  row.z[i] = c.z;
  row.n[i] = c.n;
  row.anh[i] = gh_n;
  row.h1[i] = c.h1;
}

// dh = d loss / d h1. dar, daz, dpn: gradients of the r, z, n pre-activations (the gi side; the gh side is
// dar, daz, dpn_r = dpn r); dh_z = dh z: the direct path to h0.
struct GruBwd {
  float dar, daz, dpn, dpn_r, dh_z;
};
__device__ __forceinline__ GruBwd gru_cell_bwd(float dh, float h0, float r, float z, float n, float anh) {
  const float dn = dh * (1.f - z);
  const float dz = dh * (h0 - n);
  const float dpn = dn * (1.f - n * n);
  const float dr = dpn * anh;
  const float dar = dr * r * (1.f - r);
  const float daz = dz * z * (1.f - z);
  return {dar, daz, dpn, dpn * r, dh * z};
}
// the six global stores of unit f: dgi / dgh = this row's [3H] gate-gradient rows
__device__ __forceinline__ void store_gru_delta(float* dgi, float* dgh, int f, int H, const GruBwd& c) {
  dgi[f] = c.dar;
  dgi[H + f] = c.daz;
  dgi[2 * H + f] = c.dpn;
  dgh[f] = c.dar;
  dgh[H + f] = c.daz;
  dgh[2 * H + f] = c.dpn_r;
}

// ------------------------------------------------------------------ hypernet mixing, forward
// hyp: one row's hypernet outputs [w1raw (N*K1) | b1 | w2raw | b2 hidden pre-ReLU] (the save row's order), q: its
// [N] agent values.  y_pre[k] = sum_i |w1raw[k*N + i]| q_i + b1[k]   (bmm(W1 [K1,N], q [N,1]) + b1)
__device__ __forceinline__ float mix_ypre(int k, int K1, int N, const float* hyp, const float* q) {
  float acc = 0.f;
  for (int i = 0; i < N; ++i) acc += fabsf(hyp[k * N + i]) * q[i];
  return acc + hyp[N * K1 + k];
}
struct MixOut {
  float qtot, b2;
};
// b2 = b2bW . relu(b2 hidden) + b2bb;  Q_tot = sum_k |w2raw_k| relu(y_pre_k) + b2
__device__ __forceinline__ MixOut mix_qtot(int K1, int N, const float* hyp, const float* yp, const float* b2bW,
                                           const float* b2bb) {
  const float* w2raw = hyp + N * K1 + K1;
  const float* b2pre = hyp + N * K1 + 2 * K1;
  float b2 = 0.f;
  for (int k = 0; k < K1; ++k) b2 += b2bW[k] * fmaxf(b2pre[k], 0.f);
  b2 += *b2bb;
  float acc = 0.f;
  for (int k = 0; k < K1; ++k) acc += fabsf(w2raw[k]) * fmaxf(yp[k], 0.f);
  return {acc + b2, b2};
}
// element i < N*K1 + 3*K1 of the save row's hypernet part (from w1raw on) for hyp[i] = v
__device__ __forceinline__ float mix_save_hyp(int i, int K1, int N, float v) {
  return i >= N * K1 + 2 * K1 ? fmaxf(v, 0.f) : v;
}

// ------------------------------------------------------------------ hypernet mixing, backward
// Unit k < K1 of one row: d w2raw_k, d y_pre_k (= d b1_k), d b2 hidden_k and d w1raw[k][0..N) from dQ = d loss /
// d Q_tot, into the delta row and into the caller's scratch row shd [N*K1 + 3*K1] (the transposed mat-vecs' input).
// qa: the row's [N] agent values; b2bW: the b2 output layer's [K1] weights, in global memory or a staged LDS copy
// (a pointer, not the value: the load stays under the ReLU mask as the kernels had it).
__device__ __forceinline__ void mix_hyper_delta(int k, int K1, int N, const MixSaveRow<const float*>& sv,
                                                const float* qa, float dQ, const float* b2bW,
                                                const MixDeltaRow<float*>& dl, float* shd) {
  const int NK = N * K1;
  const float y = fmaxf(sv.ypre[k], 0.f);
  const float w2 = sv.w2raw[k];
  const float dw2 = dQ * y * (w2 > 0.f ? 1.f : (w2 < 0.f ? -1.f : 0.f));
  const float dyp = sv.ypre[k] > 0.f ? dQ * fabsf(w2) : 0.f;
  const float db2p = sv.b2pre[k] > 0.f ? dQ * b2bW[k] : 0.f;
  dl.d_b1[k] = dyp;
  dl.d_w2[k] = dw2;
  dl.d_b2pre[k] = db2p;
  shd[NK + k] = dyp;
  shd[NK + K1 + k] = dw2;
  shd[NK + 2 * K1 + k] = db2p;
  for (int i = 0; i < N; ++i) {
    const float w = sv.w1raw[k * N + i];
    const float dw1 = dyp * qa[i] * (w > 0.f ? 1.f : (w < 0.f ? -1.f : 0.f));
    dl.d_w1[k * N + i] = dw1;
    shd[k * N + i] = dw1;
  }
}
// dqa_i = sum_k dy_pre_k |W1[k,i]|   (dyp = shd + N*K1 of the row)
__device__ __forceinline__ float mix_dqa(int i, int K1, int N, const float* dyp, const float* w1raw) {
  float acc = 0.f;
  for (int k = 0; k < K1; ++k) acc += dyp[k] * fabsf(w1raw[k * N + i]);
  return acc;
}

}  // namespace mm
