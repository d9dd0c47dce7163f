// Offpolicy QMix / VDN episode collector on gfx950: the collect loop of the reference's magym runner
// (offpolicy/runner/shared/magym_runner.py:40-141, one env at a time there) for E lockstep Checkers or Switch envs,
// a whole T-step episode in ONE launch. Episodes of different envs are independent and the AgentQFunction
// (LN(D) -> [Linear, ReLU, LN] x 2 -> GRU(H) -> LN -> Linear(A), agent_q_function.py:24-57) is shared by all
// agents, so a block owns a tile of envs for the whole episode and nothing is handed between blocks.
//
//   block   256 threads = 4 waves; wave w owns the (env, agent) rows 32 w .. 32 w + 31 of the tile's
//           ne N <= 128 rows (ne = min(128 / N, 64) envs). No row ever changes its wave or lane.
//   weights staged once per block into LDS as exact-f32 MFMA A-operand images (v_mfma_f32_32x32x2_f32, the
//           fragment maps of common.h): k-step s of row block rb, lane (i, h) holds W[32 rb + i][col(s, h)],
//           four k-steps per 16-byte piece, so a wave's ds_read_b128 is contiguous. 132 KiB of the 160 KiB LDS;
//           the env tile (nibble-row grids, positions, the step's actions / rewards / observation words) and
//           the per-feature vectors take the next 14 KiB.
//   layers  activations chain through registers: D register s of the producing layer is the B operand of
//           k-step s of the next (kperm). Lane (j, h) holds 32 of row j's 64 features, its partner lane
//           j + 32 the others; a LayerNorm sum is one cross-half shuffle. The GRU hidden state stays in
//           32 registers per lane for all T steps (zero at t = 0, never reset: the reference keeps calling the
//           policy after done).
//   env     the in-LDS Checkers step of rollout_env.h (roll_agent_step / roll_obs_word), one lane per env,
//           agents in id order. The observation is never materialised for the net: LayerNorm 0 and the first
//           layer's B operands come from the 45-bit observation word and the two coordinates.
//   output  every field of a step is one contiguous run per block ([t][e0 .. e0 + ne)[N][X]); the block
//           writes it thread-linear with 16-byte stores (scalar head / tail where the run is not aligned).
//
// Switch (offq_collect_switch_kernel) keeps the block and wave layout, the net from layer 1's bias on, the action
// draw and the output stores (oc_stage_net / oc_net / oc_act / oc_store are shared), and differs in three places:
//   obs     three floats per row [row feature, column feature, clock], so layer 1 is one group of 4 k-steps
//           (features 0..2, the rest zero; its image is 2 KiB, not 12) and LayerNorm 0 is computed from the floats:
//           mean, centred variance, 1 / sqrt(var + eps).
//   env     per env in LDS: the agents' cells r << 4 | c, their done flags, the step count and the clock
//           (float)((double)steps / max_steps), as switch.hip's sw_obs forms it. One lane per env moves the agents
//           in id order by the rules of oracle/switch.py.
//   dones   per agent: dones[t, e, n] is agent n's done flag, dones_env[t, e] their conjunction.
//
// The env handle's live state is neither read nor written: every env starts from reset (Checkers: the handle's
// init_grid / init_pos tables; Switch: the fixed start cells) and the episode's state lives in LDS only.
#include <algorithm>

#include "common.h"
#include "env_dev.h"
#include "minimarl.h"
#include "rollout_env.h"
#include "switch_dev.h"
#include "trunk.h"

namespace mm {
namespace {

constexpr int OC_D = 47, OC_H = 64, OC_A = 5;
constexpr int OS_D = 3;        // Switch: local observation with the clock
constexpr int OC_ROWS = 128;   // (env, agent) rows of a block: 4 waves x 32
constexpr int OC_MAXE = 64;    // envs of a block's tile

// LDS layout of the staged net, float offsets (every weight image and vector starts on 16 bytes). KS1 = k-steps of
// layer 1 (a multiple of 4, 2 KS1 >= D)
template <int KS1>
struct OcNetLds {
  static constexpr int W1 = 0;                      // [2 rb][KS1 / 4][64][4]   col(s, h) = 2 s + h
  static constexpr int W2 = W1 + 2 * KS1 * 64;      // [2 rb][8][64][4]   col(s, h) = 32 (s >> 4) + kperm(s & 15, h)
  static constexpr int Wih = W2 + 2 * 32 * 64;      // [6 rb][8][64][4]
  static constexpr int Whh = Wih + 6 * 32 * 64;     // [6 rb][8][64][4]
  static constexpr int Wo = Whh + 6 * 32 * 64;      // [1 rb][8][64][4]   rows >= A zero
  static constexpr int ln0w = Wo + 32 * 64;         // [2 h][KS1]: feature 2 s + h (D.. -> 0)
  static constexpr int ln0b = ln0w + 2 * KS1;
  static constexpr int b1 = ln0b + 2 * KS1, ln1w = b1 + 64, ln1b = ln1w + 64;
  static constexpr int b2 = ln1b + 64, ln2w = b2 + 64, ln2b = ln2w + 64;
  static constexpr int brz = ln2b + 64;             // [128] b_ih + b_hh of the r and z gates
  static constexpr int bin = brz + 128, bhn = bin + 64;
  static constexpr int lnrw = bhn + 64, lnrb = lnrw + 64;
  static constexpr int bo = lnrb + 64;              // [32] (A.. zero)
  static constexpr int net_end = bo + 32;
  static_assert((KS1 & 3) == 0 && (ln0w & 3) == 0, "alignment");
};

// Checkers: the net, then the env tile
struct OcLds : OcNetLds<24> {
  static constexpr int stab = net_end;              // [R + C] coordinate features
  static constexpr int init = stab + 32;            // [16] the reset grid as nibble rows
  static constexpr int grid = init + 16;            // [OC_MAXE][roll_gbw(R)] nibble rows
  static constexpr int pos = grid + OC_MAXE * (kRollMaxR | 1);   // [rows] 16-bit position words
  static constexpr int act = pos + OC_ROWS;         // [rows] the step's actions
  static constexpr int rew = act + OC_ROWS;         // [rows] the step's stored rewards
  static constexpr int cr = rew + OC_ROWS, cc = cr + OC_ROWS;    // [rows] coordinates of the step's observation
  static constexpr int word = cc + OC_ROWS;         // [rows] u64 observation words
  static constexpr int q = word + 2 * OC_ROWS;      // [rows][A]
  static constexpr int done = q + OC_ROWS * OC_A;   // [OC_MAXE]
  static constexpr int total = done + OC_MAXE;
};
static_assert(OcLds::total * 4 <= 160 * 1024, "LDS budget");
static_assert((OcLds::word & 1) == 0, "alignment");

// Switch: the net, then the env tile
struct OsLds : OcNetLds<4> {
  static constexpr int stab = net_end;              // [3] row features, [7] column features at + 4
  static constexpr int pos = stab + 12;             // [rows] agent cells r << 4 | c
  static constexpr int adone = pos + OC_ROWS;       // [rows] agent done flags (0 / 1 as floats: the dones field)
  static constexpr int act = adone + OC_ROWS;       // [rows] the step's actions
  static constexpr int rew = act + OC_ROWS;         // [rows] the step's stored rewards
  static constexpr int cr = rew + OC_ROWS, cc = cr + OC_ROWS, ck = cc + OC_ROWS;   // [rows] the step's observation
  static constexpr int q = ck + OC_ROWS;            // [rows][A]
  static constexpr int steps = q + OC_ROWS * OC_A;  // [OC_MAXE] step counts
  static constexpr int clk = steps + OC_MAXE;       // [OC_MAXE] the clock feature of the current state
  static constexpr int done = clk + OC_MAXE;        // [OC_MAXE] all agents done
  static constexpr int total = done + OC_MAXE;
};
static_assert(OsLds::total * 4 <= 160 * 1024, "LDS budget");

// what both kernels take: the net, the exploration stream, the episode fields
struct OcIo {
  const float* P;
  const float* eps;
  const unsigned long long* counter;
  uint64_t counter0, seed;
  float *obs, *acts, *rew, *dones, *dones_env, *q_out, *ret_out;
  int E, T, N, EB, max_steps, common;
  float step_cost;
};

struct OcArgs : OcIo {
  const int8_t* init_grid;
  const int32_t* init_pos;
  const float* rtab;
  const float* ctab;
  int R, C, init_apples;
};

struct OsArgs : OcIo {
  SwitchTab tab;
};

// A-operand image of W (row-major, leading dimension ld, rows x cols valid, zero outside): RB row blocks, KS k-steps
template <bool CHAIN>
__device__ __forceinline__ void oc_pack(float* dst, const float* __restrict__ W, int ld, int rows, int cols, int RB,
                                        int KS) {
  const int n = RB * KS * 64, s4n = KS >> 2;
  for (int o = threadIdx.x; o < n; o += blockDim.x) {
    const int si = o & 3, lane = (o >> 2) & 63, q = o >> 8;
    const int rb = q / s4n, s = (q - rb * s4n) * 4 + si;
    const int i = lane & 31, h = lane >> 5;
    const int row = 32 * rb + i, col = CHAIN ? 32 * (s >> 4) + kperm(s & 15, h) : 2 * s + h;
    dst[o] = (row < rows && col < cols) ? W[row * ld + col] : 0.0f;
  }
}

// acc[rb] += W[32 rb .. 32 rb + 31][:] x for NRB row blocks over KS k-steps; bval(s) = this lane's B operand of k-step s
template <int NRB, int KS, typename B>
__device__ __forceinline__ void oc_mma(f32x16* acc, const float* sW, int lane, B bval) {
#pragma unroll
  for (int s4 = 0; s4 < KS / 4; ++s4) {
    float av[NRB][4];
#pragma unroll
    for (int rb = 0; rb < NRB; ++rb) {
      const float4 a = *reinterpret_cast<const float4*>(sW + ((rb * (KS / 4) + s4) * 64 + lane) * 4);
      av[rb][0] = a.x;
      av[rb][1] = a.y;
      av[rb][2] = a.z;
      av[rb][3] = a.w;
    }
#pragma unroll
    for (int si = 0; si < 4; ++si) {
      const float b = bval(4 * s4 + si);
#pragma unroll
      for (int rb = 0; rb < NRB; ++rb) acc[rb] = mfma32(av[rb][si], b, acc[rb]);
    }
  }
}

// the 16 entries of a 32-feature vector that lane half h holds: register r <-> feature kperm(r, h)
__device__ __forceinline__ f32x16 oc_vec16(const float* v32, int h) {
  f32x16 o;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const float4 t = *reinterpret_cast<const float4*>(v32 + 8 * q + 4 * h);
    o[4 * q] = t.x;
    o[4 * q + 1] = t.y;
    o[4 * q + 2] = t.z;
    o[4 * q + 3] = t.w;
  }
  return o;
}

// LayerNorm over a row's 64 features (32 in this lane, 32 in lane ^ 32), in place
__device__ __forceinline__ void oc_ln(f32x16 (&v)[2], const float* sw, const float* sb, int h) {
  float s = 0.0f;
#pragma unroll
  for (int kb = 0; kb < 2; ++kb)
#pragma unroll
    for (int r = 0; r < 16; ++r) s += v[kb][r];
  s += __shfl_xor(s, 32);
  const float mu = s * (1.0f / OC_H);
  float q = 0.0f;
#pragma unroll
  for (int kb = 0; kb < 2; ++kb)
#pragma unroll
    for (int r = 0; r < 16; ++r) q = fmaf(v[kb][r] - mu, v[kb][r] - mu, q);
  q += __shfl_xor(q, 32);
  const float rs = 1.0f / sqrtf(q * (1.0f / OC_H) + kLnEps);
#pragma unroll
  for (int kb = 0; kb < 2; ++kb) {
    const f32x16 w = oc_vec16(sw + 32 * kb, h), b = oc_vec16(sb + 32 * kb, h);
#pragma unroll
    for (int r = 0; r < 16; ++r) v[kb][r] = (v[kb][r] - mu) * rs * w[r] + b[r];
  }
}

// base[g0 + i] = gen(i) for i < n, the block's threads on consecutive 16-byte slots (base 16-byte aligned)
template <typename G>
__device__ __forceinline__ void oc_store(float* base, int64_t g0, int n, G gen) {
  const int head = (int)(g0 & 3);
  float* slot0 = base + (g0 - head);
  const int nslot = (head + n + 3) >> 2;
  for (int v = threadIdx.x; v < nslot; v += blockDim.x) {
    const int i0 = 4 * v - head;
    if (i0 >= 0 && i0 + 3 < n) {
      *reinterpret_cast<float4*>(slot0 + 4 * v) = make_float4(gen(i0), gen(i0 + 1), gen(i0 + 2), gen(i0 + 3));
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (i0 + k >= 0 && i0 + k < n) slot0[4 * v + k] = gen(i0 + k);
    }
  }
}

// stage the net (MGeo<D, 64, 5> flat layout at P) into the images and vectors of L; the caller's barrier follows
template <typename L, int D, int KS1>
__device__ __forceinline__ void oc_stage_net(float* sm, const float* __restrict__ P) {
  using G = MGeo<D, OC_H, OC_A>;
  const int tid = threadIdx.x;
  oc_pack<false>(sm + L::W1, P + G::W1, G::Dp, OC_H, D, 2, KS1);
  oc_pack<true>(sm + L::W2, P + G::W2, OC_H, OC_H, OC_H, 2, 32);
  oc_pack<true>(sm + L::Wih, P + G::Wih, OC_H, 3 * OC_H, OC_H, 6, 32);
  oc_pack<true>(sm + L::Whh, P + G::Whh, OC_H, 3 * OC_H, OC_H, 6, 32);
  oc_pack<true>(sm + L::Wo, P + G::Wo, OC_H, OC_A, OC_H, 1, 32);
  if (tid < 2 * KS1) {
    const int f = 2 * (tid % KS1) + tid / KS1;
    sm[L::ln0w + tid] = f < D ? P[G::ln0_w + f] : 0.0f;
    sm[L::ln0b + tid] = f < D ? P[G::ln0_b + f] : 0.0f;
  }
  if (tid < OC_H) {
    sm[L::b1 + tid] = P[G::b1 + tid];
    sm[L::ln1w + tid] = P[G::ln1_w + tid];
    sm[L::ln1b + tid] = P[G::ln1_b + tid];
    sm[L::b2 + tid] = P[G::b2 + tid];
    sm[L::ln2w + tid] = P[G::ln2_w + tid];
    sm[L::ln2b + tid] = P[G::ln2_b + tid];
    sm[L::brz + tid] = P[G::bih + tid] + P[G::bhh + tid];
    sm[L::brz + OC_H + tid] = P[G::bih + OC_H + tid] + P[G::bhh + OC_H + tid];
    sm[L::bin + tid] = P[G::bih + 2 * OC_H + tid];
    sm[L::bhn + tid] = P[G::bhh + 2 * OC_H + tid];
    sm[L::lnrw + tid] = P[G::lnr_w + tid];
    sm[L::lnrb + tid] = P[G::lnr_b + tid];
  }
  if (tid < 32) sm[L::bo + tid] = tid < OC_A ? P[G::bo + tid] : 0.0f;
}

// The net of one step from LayerNorm 0's output: x0[s] = this lane's normalised feature 2 s + h. Updates the hidden
// state in place; Q 0..3 land in registers 0..3 of lane half 0 of the result, Q 4 in register 0 of half 1
template <typename L, int KS1>
__device__ __forceinline__ f32x16 oc_net(const float* sm, const float (&x0)[KS1], f32x16 (&hid)[2], int lane, int h) {
  // ---- layer 1, layer 2
  f32x16 f1[2], f2[2];
  f1[0] = oc_vec16(sm + L::b1, h);
  f1[1] = oc_vec16(sm + L::b1 + 32, h);
  oc_mma<2, KS1>(f1, sm + L::W1, lane, [&](int s) { return x0[s]; });
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    f1[0][r] = fmaxf(f1[0][r], 0.0f);
    f1[1][r] = fmaxf(f1[1][r], 0.0f);
  }
  oc_ln(f1, sm + L::ln1w, sm + L::ln1b, h);
  f2[0] = oc_vec16(sm + L::b2, h);
  f2[1] = oc_vec16(sm + L::b2 + 32, h);
  oc_mma<2, 32>(f2, sm + L::W2, lane, [&](int s) { return f1[s >> 4][s & 15]; });
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    f2[0][r] = fmaxf(f2[0][r], 0.0f);
    f2[1][r] = fmaxf(f2[1][r], 0.0f);
  }
  oc_ln(f2, sm + L::ln2w, sm + L::ln2b, h);
  // ---- GRU: g[0..3] r | z pre-activations (input + hidden side), g[4..5] W_in x + b_in, g[6..7] W_hn h + b_hn
  {
    f32x16 g[8];
#pragma unroll
    for (int kb = 0; kb < 4; ++kb) g[kb] = oc_vec16(sm + L::brz + 32 * kb, h);
#pragma unroll
    for (int kb = 0; kb < 2; ++kb) {
      g[4 + kb] = oc_vec16(sm + L::bin + 32 * kb, h);
      g[6 + kb] = oc_vec16(sm + L::bhn + 32 * kb, h);
    }
    oc_mma<6, 32>(g, sm + L::Wih, lane, [&](int s) { return f2[s >> 4][s & 15]; });
    oc_mma<4, 32>(g, sm + L::Whh, lane, [&](int s) { return hid[s >> 4][s & 15]; });
    oc_mma<2, 32>(g + 6, sm + L::Whh + 4 * 8 * 256, lane, [&](int s) { return hid[s >> 4][s & 15]; });
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float rr = sigmoidf_(g[kb][r]), zz = sigmoidf_(g[2 + kb][r]);
        const float nn = tanhf_(g[4 + kb][r] + rr * g[6 + kb][r]);
        hid[kb][r] = nn + zz * (hid[kb][r] - nn);
      }
  }
  // ---- head: LN, Linear(A)
  f32x16 y[2] = {hid[0], hid[1]};
  oc_ln(y, sm + L::lnrw, sm + L::lnrb, h);
  f32x16 qa = oc_vec16(sm + L::bo, h);
  oc_mma<1, 32>(&qa, sm + L::Wo, lane, [&](int s) { return y[s >> 4][s & 15]; });
  return qa;
}

// Epsilon-greedy on the head's result (every lane calls it; the row's owner lane writes): the first maximum, or the
// counter RNG's action where u < eps. sact[row] gets the action, sq[row][A] the Q values when they are wanted
__device__ __forceinline__ void oc_act(const OcIo& a, f32x16 qa, bool owner, int row, uint64_t ctr, uint64_t rinner,
                                       float eps, int* sact, float* sq) {
  const float q4 = __shfl_xor(qa[0], 32);
  if (owner) {
    const float qv[OC_A] = {qa[0], qa[1], qa[2], qa[3], q4};
    int g = 0;
    float best = qv[0];
#pragma unroll
    for (int k = 1; k < OC_A; ++k)
      if (qv[k] > best) {
        best = qv[k];
        g = k;
      }
    const float u = rng_uniform(rng_draw_inner(a.seed, ctr, rinner));
    const int ra = (int)rng_mod_small(rng_draw_inner(a.seed ^ 0x5bd1e995ull, ctr, rinner), OC_A);
    sact[row] = u < eps ? ra : g;
    if (a.q_out) {
#pragma unroll
      for (int k = 0; k < OC_A; ++k) sq[row * OC_A + k] = qv[k];
    }
  }
}

__global__ __launch_bounds__(256) void offq_collect_kernel(OcArgs a) {
  using L = OcLds;
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5;
  const int N = a.N, R = a.R, C = a.C, gbw = roll_gbw(R);
  const int e0 = blockIdx.x * a.EB, ne = min(a.EB, a.E - e0), nrows = ne * N;
  uint32_t* sgrid = reinterpret_cast<uint32_t*>(sm + L::grid);
  uint32_t* sinit = reinterpret_cast<uint32_t*>(sm + L::init);
  uint32_t* spos = reinterpret_cast<uint32_t*>(sm + L::pos);
  int* sact = reinterpret_cast<int*>(sm + L::act);
  float* srew = sm + L::rew;
  float* scr = sm + L::cr;
  float* scc = sm + L::cc;
  uint64_t* sword = reinterpret_cast<uint64_t*>(sm + L::word);
  float* sq = sm + L::q;
  float* sdone = sm + L::done;
  const float* stab = sm + L::stab;

  // ---- stage the net and the reset state
  oc_stage_net<L, OC_D, 24>(sm, a.P);
  if (tid < R) {
    sm[L::stab + tid] = a.rtab[tid];
    uint32_t w = 0;
    for (int c = 0; c < C; ++c) w |= ((uint32_t)a.init_grid[tid * C + c] & 15u) << (4 * c);
    sinit[tid] = w;
  }
  if (tid < C) sm[L::stab + R + tid] = a.ctab[tid];
  __syncthreads();
  for (int i = tid; i < ne * R; i += blockDim.x) {
    const int le = i / R, r = i - le * R;
    sgrid[le * gbw + r] = sinit[r];
  }
  for (int i = tid; i < nrows; i += blockDim.x) spos[i] = pos16(a.init_pos[i % N]);
  __syncthreads();

  // this lane's row of the tile (both lane halves of a row compute its scalars redundantly)
  const int row = wave * 32 + (lane & 31);
  const bool valid = row < nrows;
  const int rle = valid ? row / N : 0, rn = valid ? row - rle * N : 0, rrow = valid ? row : 0;
  const bool owner = valid && h == 0;
  const uint64_t rinner = rng_inner((uint64_t)(e0 + rle), (uint64_t)rn);
  const float eps = *a.eps;
  const uint64_t c0 = a.counter ? (uint64_t)*a.counter : a.counter0;
  // the env lane's episode state (lane tid < ne owns env e0 + tid)
  int steps = 0, apples = a.init_apples;
  bool edone = false;
  float ret = 0.0f;
  f32x16 hid[2];
#pragma unroll
  for (int r = 0; r < 16; ++r) hid[0][r] = hid[1][r] = 0.0f;

  for (int t = 0; t <= a.T; ++t) {
    // ---- the observation of the current state as a bit word + two coordinates
    const uint32_t pw = spos[rrow];
    const int pr_ = (pw >> 4) & 15, pc_ = pw & 15;
    const uint64_t wd = roll_obs_word(sgrid + rle * gbw, R, pr_, pc_);
    const float cr = stab[pr_], cc = stab[R + pc_];
    if (owner) {
      sword[row] = wd;
      scr[row] = cr;
      scc[row] = cc;
    }
    const int64_t rowbase = ((int64_t)t * a.E + e0) * N;   // row (t, e0, 0) of the [.., E, N, X] fields
    auto obs_gen = [&](int i) {
      const int r = i / OC_D, f = i - r * OC_D;
      return f == 0 ? scr[r] : (f == 1 ? scc[r] : (float)((uint32_t)(sword[r] >> f) & 1u));
    };
    if (t == a.T) {
      lds_sync();
      oc_store(a.obs, rowbase * OC_D, nrows * OC_D, obs_gen);
      break;
    }

    // ---- LayerNorm 0 from the word: 2 coordinates, pc ones, 45 - pc zeros
    const float npc = (float)__popcll(wd);
    const float mu0 = (cr + cc + npc) * (1.0f / OC_D);
    const float dr = cr - mu0, dc = cc - mu0, d1 = 1.0f - mu0;
    const float var0 = (dr * dr + dc * dc + npc * (d1 * d1) + (45.0f - npc) * (mu0 * mu0)) * (1.0f / OC_D);
    const float rs0 = 1.0f / sqrtf(var0 + kLnEps);
    float x0[24];   // feature 2 s + h, normalised
    {
      const uint64_t wh = wd >> h;
#pragma unroll
      for (int s4 = 0; s4 < 6; ++s4) {
        const float4 w4 = *reinterpret_cast<const float4*>(sm + L::ln0w + 24 * h + 4 * s4);
        const float4 b4 = *reinterpret_cast<const float4*>(sm + L::ln0b + 24 * h + 4 * s4);
        const float wv[4] = {w4.x, w4.y, w4.z, w4.w}, bv[4] = {b4.x, b4.y, b4.z, b4.w};
#pragma unroll
        for (int si = 0; si < 4; ++si) {
          const int s = 4 * s4 + si;
          const float xv = s == 0 ? (h ? cc : cr) : (float)((uint32_t)(wh >> (2 * s)) & 1u);
          x0[s] = (xv - mu0) * rs0 * wv[si] + bv[si];
        }
      }
    }
    const f32x16 qa = oc_net<L, 24>(sm, x0, hid, lane, h);
    oc_act(a, qa, owner, row, c0 + (uint64_t)t, rinner, eps, sact, sq);
    lds_sync();

    // ---- env step: one lane per env, agents in id order; a finished env is not stepped
    if (tid < ne) {
      uint32_t* rows = sgrid + tid * gbw;
      if (!edone) {
        float sum = 0.0f;
#pragma unroll 1
        for (int k = 0; k < N; ++k) {
          const RollMove mv = roll_agent_step(spos[tid * N + k], sact[tid * N + k], k, rows, R, C, a.step_cost);
          spos[tid * N + k] = mv.w;
          srew[tid * N + k] = mv.rew;
          apples -= mv.ate ? 1 : 0;
          sum = k == 0 ? mv.rew : sum + mv.rew;
        }
        if (a.common)
          for (int k = 0; k < N; ++k) srew[tid * N + k] = sum;
        ++steps;
        edone = steps >= a.max_steps || apples == 0;
      } else {
        for (int k = 0; k < N; ++k) srew[tid * N + k] = 0.0f;
      }
      sdone[tid] = edone ? 1.0f : 0.0f;
      ret += srew[tid * N];
    }
    lds_sync();

    // ---- the step's episode fields
    oc_store(a.obs, rowbase * OC_D, nrows * OC_D, obs_gen);
    oc_store(a.acts, rowbase * OC_A, nrows * OC_A, [&](int i) {
      const int r = i / OC_A;
      return sact[r] == i - r * OC_A ? 1.0f : 0.0f;
    });
    oc_store(a.rew, rowbase, nrows, [&](int i) { return srew[i]; });
    oc_store(a.dones, rowbase, nrows, [&](int i) { return sdone[i / N]; });
    oc_store(a.dones_env, (int64_t)t * a.E + e0, ne, [&](int i) { return sdone[i]; });
    if (a.q_out) oc_store(a.q_out, rowbase * OC_A, nrows * OC_A, [&](int i) { return sq[i]; });
    lds_sync();
  }
  if (a.ret_out && tid < ne) a.ret_out[e0 + tid] = ret;
}

__global__ __launch_bounds__(256) void offq_collect_switch_kernel(OsArgs a) {
  using L = OsLds;
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5;
  const int N = a.N;
  const int e0 = blockIdx.x * a.EB, ne = min(a.EB, a.E - e0), nrows = ne * N;
  uint32_t* spos = reinterpret_cast<uint32_t*>(sm + L::pos);
  float* sadone = sm + L::adone;
  int* sact = reinterpret_cast<int*>(sm + L::act);
  float* srew = sm + L::rew;
  float* scr = sm + L::cr;
  float* scc = sm + L::cc;
  float* sck = sm + L::ck;
  float* sq = sm + L::q;
  int* ssteps = reinterpret_cast<int*>(sm + L::steps);
  float* sclk = sm + L::clk;
  float* sdone = sm + L::done;
  const float* stab = sm + L::stab;

  // ---- stage the net and the reset state: agent k starts at (0, 1) (0, 5) (2, 1) (2, 5)[k], step 0
  oc_stage_net<L, OS_D, 4>(sm, a.P);
  if (tid < 3) sm[L::stab + tid] = a.tab.row[tid];
  if (tid < 7) sm[L::stab + 4 + tid] = a.tab.col[tid];
  for (int i = tid; i < nrows; i += blockDim.x) {
    const int k = i % N;
    spos[i] = (uint32_t)((k < 2 ? 0 : 2) << 4 | ((k & 1) ? 5 : 1));
    sadone[i] = 0.0f;
  }
  if (tid < ne) {
    ssteps[tid] = 0;
    sclk[tid] = 0.0f;
  }
  __syncthreads();

  // this lane's row of the tile (both lane halves of a row compute its scalars redundantly)
  const int row = wave * 32 + (lane & 31);
  const bool valid = row < nrows;
  const int rle = valid ? row / N : 0, rn = valid ? row - rle * N : 0, rrow = valid ? row : 0;
  const bool owner = valid && h == 0;
  const uint64_t rinner = rng_inner((uint64_t)(e0 + rle), (uint64_t)rn);
  const float eps = *a.eps;
  const uint64_t c0 = a.counter ? (uint64_t)*a.counter : a.counter0;
  bool edone = false;   // the env lane's (lane tid < ne owns env e0 + tid)
  float ret = 0.0f;
  f32x16 hid[2];
#pragma unroll
  for (int r = 0; r < 16; ++r) hid[0][r] = hid[1][r] = 0.0f;

  for (int t = 0; t <= a.T; ++t) {
    // ---- the observation of the current state: row feature, column feature, clock
    const uint32_t pw = spos[rrow];
    const float cr = stab[(pw >> 4) & 3], cc = stab[4 + (pw & 7)], ck = sclk[rle];
    if (owner) {
      scr[row] = cr;
      scc[row] = cc;
      sck[row] = ck;
    }
    const int64_t rowbase = ((int64_t)t * a.E + e0) * N;   // row (t, e0, 0) of the [.., E, N, X] fields
    auto obs_gen = [&](int i) {
      const int r = i / OS_D, f = i - r * OS_D;
      return f == 0 ? scr[r] : (f == 1 ? scc[r] : sck[r]);
    };
    if (t == a.T) {
      lds_sync();
      oc_store(a.obs, rowbase * OS_D, nrows * OS_D, obs_gen);
      break;
    }

    // ---- LayerNorm 0 over the three floats: mean, centred variance. Lane half h feeds features h and 2 + h
    // (feature 3 is a zero pad: its LayerNorm weight, bias and W1 column are staged as zero)
    const float mu0 = ((cr + cc) + ck) / (float)OS_D;
    const float dr = cr - mu0, dc = cc - mu0, dk = ck - mu0;
    const float var0 = (dr * dr + dc * dc + dk * dk) / (float)OS_D;
    const float rs0 = 1.0f / sqrtf(var0 + kLnEps);
    float x0[4];   // feature 2 s + h, normalised
    {
      const float4 w4 = *reinterpret_cast<const float4*>(sm + L::ln0w + 4 * h);
      const float4 b4 = *reinterpret_cast<const float4*>(sm + L::ln0b + 4 * h);
      x0[0] = (h ? dc : dr) * rs0 * w4.x + b4.x;
      x0[1] = (h ? 0.0f : dk) * rs0 * w4.y + b4.y;
      x0[2] = 0.0f;
      x0[3] = 0.0f;
    }
    const f32x16 qa = oc_net<L, 4>(sm, x0, hid, lane, h);
    oc_act(a, qa, owner, row, c0 + (uint64_t)t, rinner, eps, sact, sq);
    lds_sync();

    // ---- env step (oracle/switch.py SwitchOracle.step): one lane per env, agents in id order on the cells in LDS,
    // so a move sees the cells as updated so far this step; a finished env is not stepped
    if (tid < ne) {
      const int b = tid * N;
      if (!edone) {
        const int steps = ssteps[tid] + 1;
        const bool timeout = steps >= a.max_steps;
        bool all = true;
        float sum = 0.0f;
#pragma unroll 1
        for (int k = 0; k < N; ++k) {
          bool ad = sadone[b + k] != 0.0f;
          float rw = a.step_cost;
          if (!ad) {   // a finished agent keeps its cell and goes on receiving step_cost
            const uint32_t cw = spos[b + k];
            int r = (int)(cw >> 4), c = (int)(cw & 15);
            const int act = sact[b + k];   // 0 down, 1 left, 2 up, 3 right, 4 noop
            if (act < 4) {
              const int nr = r + (act == 0) - (act == 2), nc = c + (act == 3) - (act == 1);
              bool ok = sw_open(nr, nc);
              const uint32_t nw = ok ? (uint32_t)(nr << 4 | nc) : 0u;
              for (int j = 0; j < N; ++j) ok = ok && (j == k || spos[b + j] != nw);
              if (ok) {
                spos[b + k] = nw;
                r = nr;
                c = nc;
              }
            }
            if (r == (k < 2 ? 0 : 2) && c == ((k & 1) ? 0 : 6)) {   // targets (0, 6) (0, 0) (2, 6) (2, 0)
              ad = true;
              rw = 5.0f;
            }
          }
          ad = ad || timeout;
          sadone[b + k] = ad ? 1.0f : 0.0f;
          srew[b + k] = rw;
          sum = k == 0 ? rw : sum + rw;
          all = all && ad;
        }
        if (a.common)
          for (int k = 0; k < N; ++k) srew[b + k] = sum;
        ssteps[tid] = steps;
        sclk[tid] = (float)((double)steps / (double)a.max_steps);
        edone = all;
      } else {
        for (int k = 0; k < N; ++k) srew[b + k] = 0.0f;
      }
      sdone[tid] = edone ? 1.0f : 0.0f;
      ret += srew[b];
    }
    lds_sync();

    // ---- the step's episode fields
    oc_store(a.obs, rowbase * OS_D, nrows * OS_D, obs_gen);
    oc_store(a.acts, rowbase * OC_A, nrows * OC_A, [&](int i) {
      const int r = i / OC_A;
      return sact[r] == i - r * OC_A ? 1.0f : 0.0f;
    });
    oc_store(a.rew, rowbase, nrows, [&](int i) { return srew[i]; });
    oc_store(a.dones, rowbase, nrows, [&](int i) { return sadone[i]; });
    oc_store(a.dones_env, (int64_t)t * a.E + e0, ne, [&](int i) { return sdone[i]; });
    if (a.q_out) oc_store(a.q_out, rowbase * OC_A, nrows * OC_A, [&](int i) { return sq[i]; });
    lds_sync();
  }
  if (a.ret_out && tid < ne) a.ret_out[e0 + tid] = ret;
}

const char* range_check(int64_t E, int32_t T) {
  return (E < 1 || E > (int64_t)1 << 24 || T < 1 || T > 65536) ? "E must be in [1, 2^24] and T in [1, 65536]" : nullptr;
}

int report(const char* who, const char* why, const mm_offq_dims* d, int64_t E, int32_t T, bool on) {
  if (why && on)
    set_error("%s: unsupported configuration: %s (obs_dim %d hidden %d n_actions %d n_agents %d E %lld T %d)", who, why,
              d ? d->obs_dim : -1, d ? d->hidden : -1, d ? d->n_actions : -1, d ? d->n_agents : -1, (long long)E,
              (int)T);
  return why ? MM_EINVAL : MM_OK;
}

int collect_check(const mm_env* env, const mm_offq_dims* d, int64_t E, int32_t T, bool rep) {
  const char* why = nullptr;
  if (!env || !d) {
    why = "null env or dims";
  } else {
    const EnvDev& ev = env->d;
    if (d->obs_dim != OC_D || d->hidden != OC_H || d->n_actions != OC_A)
      why = "the agent net must be D 47, H 64, A 5";
    else if (ev.full_obs || ev.D != OC_D)
      why = "the env must give local observations (D 47)";
    else if (d->n_agents != ev.N || ev.N < 1 || ev.N > kRollMaxN)
      why = "dims.n_agents must equal the env's agents, 1..kRollMaxN";
    else if (ev.R > kRollMaxR || ev.C != 8)
      why = "the env grid must have 8 columns and at most 16 rows";
    else
      why = range_check(E, T);
  }
  return report("offq_collect", why, d, E, T, rep);
}

int collect_switch_check(const mm_switch* env, const mm_offq_dims* d, int64_t E, int32_t T, bool rep) {
  const char* why = nullptr;
  if (!env || !d) {
    why = "null env or dims";
  } else {
    const mm_switch_cfg& c = env->cfg;
    if (d->obs_dim != OS_D || d->hidden != OC_H || d->n_actions != OC_A)
      why = "the agent net must be D 3, H 64, A 5";
    else if (c.full_observable)
      why = "the Switch env must give local observations (full_observable is not built for this path)";
    else if (!c.clock)
      why = "the Switch env must have the clock feature (D 3)";
    else if (d->n_agents != c.n_agents || c.n_agents < 2 || c.n_agents > 4)
      why = "dims.n_agents must equal the env's agents, 2..4";
    else
      why = range_check(E, T);
  }
  return report("offq_collect_switch", why, d, E, T, rep);
}

// the launch arguments both kernels share; EB = envs of a block's tile
int fill_io(OcIo& a, const char* who, const float* P, const mm_offq_collect_io* io, int64_t n_envs, int32_t T, int N,
            int max_steps, float step_cost) {
  MM_REQUIRE(P && io && io->eps && io->obs && io->acts && io->rewards && io->dones && io->dones_env,
             "%s: null argument (P, io, eps and the five written fields are required)", who);
  const void* al[] = {P, io->obs, io->acts, io->rewards, io->dones, io->dones_env, io->q_out};
  for (const void* p : al) MM_REQUIRE(((uintptr_t)p & 15) == 0, "%s: P and the output fields must be 16-byte aligned", who);
  a.P = P;
  a.eps = io->eps;
  a.counter = reinterpret_cast<const unsigned long long*>(io->counter);
  a.counter0 = io->counter0;
  a.seed = io->seed;
  a.obs = io->obs;
  a.acts = io->acts;
  a.rew = io->rewards;
  a.dones = io->dones;
  a.dones_env = io->dones_env;
  a.q_out = io->q_out;
  a.ret_out = io->ret_out;
  a.E = (int)n_envs;
  a.T = T;
  a.N = N;
  a.EB = std::min(OC_ROWS / N, OC_MAXE);
  a.max_steps = max_steps;
  a.common = io->common_reward ? 1 : 0;
  a.step_cost = step_cost;
  return MM_OK;
}

}  // namespace
}  // namespace mm

extern "C" {

int mm_offq_collect_supported(const mm_env* env, const mm_offq_dims* d, int64_t n_envs, int32_t T) {
  return mm::collect_check(env, d, n_envs, T, false) == MM_OK ? 1 : 0;
}

int mm_offq_collect(mm_env* env, const mm_offq_dims* d, const float* P, const mm_offq_collect_io* io, int64_t n_envs,
                    int32_t T, mm_stream_t s) {
  using namespace mm;
  int rc = collect_check(env, d, n_envs, T, true);
  if (rc) return rc;
  const EnvDev& ev = env->d;
  OcArgs a;
  rc = fill_io(a, "offq_collect", P, io, n_envs, T, ev.N, ev.max_steps, ev.step_cost);
  if (rc) return rc;
  constexpr int lds = OcLds::total * 4;
  static const int attr_rc = [&]() -> int {
    MM_HIP_CHECK(hipFuncSetAttribute((const void*)offq_collect_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    return MM_OK;
  }();
  if (attr_rc != MM_OK) return attr_rc;
  a.init_grid = ev.init_grid;
  a.init_pos = ev.init_pos;
  a.rtab = ev.rtab;
  a.ctab = ev.ctab;
  a.R = ev.R;
  a.C = ev.C;
  a.init_apples = ev.init_apples;
  const unsigned nb = (unsigned)((n_envs + a.EB - 1) / a.EB);
  hipLaunchKernelGGL(offq_collect_kernel, dim3(nb), dim3(256), lds, (hipStream_t)s, a);
  MM_HIP_CHECK(hipGetLastError());
  return MM_OK;
}

int mm_offq_collect_switch_supported(const mm_switch* env, const mm_offq_dims* d, int64_t n_envs, int32_t T) {
  return mm::collect_switch_check(env, d, n_envs, T, false) == MM_OK ? 1 : 0;
}

int mm_offq_collect_switch(mm_switch* env, const mm_offq_dims* d, const float* P, const mm_offq_collect_io* io,
                           int64_t n_envs, int32_t T, mm_stream_t s) {
  using namespace mm;
  int rc = collect_switch_check(env, d, n_envs, T, true);
  if (rc) return rc;
  const mm_switch_cfg& c = env->cfg;
  OsArgs a;
  rc = fill_io(a, "offq_collect_switch", P, io, n_envs, T, c.n_agents, c.max_steps, c.step_cost);
  if (rc) return rc;
  constexpr int lds = OsLds::total * 4;
  static const int attr_rc = [&]() -> int {
    MM_HIP_CHECK(
        hipFuncSetAttribute((const void*)offq_collect_switch_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    return MM_OK;
  }();
  if (attr_rc != MM_OK) return attr_rc;
  a.tab = env->tab;
  const unsigned nb = (unsigned)((n_envs + a.EB - 1) / a.EB);
  hipLaunchKernelGGL(offq_collect_switch_kernel, dim3(nb), dim3(256), lds, (hipStream_t)s, a);
  MM_HIP_CHECK(hipGetLastError());
  return MM_OK;
}

}  // extern "C"
