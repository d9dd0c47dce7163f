// The segment-tree and index kernels of the device replay buffers, defined once in recbuf.hip and launched by the
// episode replay (recbuf.hip) and the transition replay (mlpbuf.hip). Trees are f64 heaps [2 itcap], root 1, leaves at
// itcap + i.
#pragma once
#include "common.h"

namespace mm {

// Leaf writes + ancestor re-derivation for n entries. Entry i: leaf idx_i = idx ? idx[i] : (base + i) % mod,
// value = prio ? prio[i] ** a : maxp ** a. Duplicates: the last entry wins (numpy fancy assignment).
// check_len >= 0: entries with idx outside [0, check_len) or prio <= 0 are skipped and flagged in err.
// One block of 1024 threads.
__global__ void erb_set_kernel(double* __restrict__ sum, double* __restrict__ mn, int64_t itcap, int n,
                               const int64_t* __restrict__ idx, int64_t base, int64_t mod,
                               const float* __restrict__ prio, float* maxp, float a, int64_t check_len, int32_t* err);

// Prioritized sample: the reference's sum(0, len - 1) fold (the last filled leaf is left out), then per draw the
// prefix-sum descent and the IS weight. One block of 256 threads.
__global__ void erb_sample_kernel(const double* __restrict__ sum, const double* __restrict__ mn, int64_t itcap,
                                  int64_t len, int B, double beta, const double* __restrict__ fracs, uint64_t seed,
                                  uint64_t counter, int64_t* __restrict__ idx_out, double* __restrict__ w_out,
                                  float* __restrict__ w32_out);

// idx_b = floor(u_b len) from the device counter RNG. Blocks of 256 threads.
__global__ void erb_uniform_kernel(int64_t len, int B, uint64_t seed, uint64_t counter, int64_t* __restrict__ idx_out);

}  // namespace mm
