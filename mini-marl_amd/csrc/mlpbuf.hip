// Offpolicy transition replay on the device: MlpReplayBuffer / PrioritizedMlpReplayBuffer
// (offpolicy/utils/mlp_buffer.py:10-340) over the segment-tree kernels of the episode replay (erb_kernels.h).
//
// A ring of single transitions, field-major: every field is a [size][row] store, so a transition of a field is one
// contiguous row, an insert of n transitions is at most two contiguous runs, and the transition collector
// (moffq_collect.hip) can write the ring in place. Insert and gather are byte movement, one launch each over all
// fields (blockIdx.y = field, a table of field descriptors as kernel argument), thread per float:
//   insert  store[((first + i) % size) R + r] = src[i R + r]: consecutive threads on consecutive floats on both sides;
//   gather  (sample_inds and its _cast transpose) dst[(nf B + b) X + x] = store[idx_b R + nf X + x], a row = Nf agents x
//           X floats: consecutive threads run along x on both sides. The shared fields are Nf = 1. Without store_share
//           the cent_obs / cent_nobs entries of the table point at the obs / next_obs stores with Nf = 1: their row
//           [N, D] is the concatenation over agents, so nothing is stored twice.
// Trees: f64 heaps, leaves written by erb_set_kernel; sampling by erb_sample_kernel / erb_uniform_kernel.
#include <math.h>

#include <algorithm>
#include <vector>

#include "common.h"
#include "erb_kernels.h"
#include "minimarl.h"

namespace {
constexpr int kNF = 9;   // obs, share_obs, acts, rewards, next_obs, next_share_obs, dones, dones_env, valid_transition
}

struct mm_mlpbuf {
  mm_mlpbuf_dims d;
  int64_t size, itcap, filled, current;
  float alpha_f;
  void* alloc;
  float* f[kNF];   // stores [size][R]; NULL for the share fields without store_share
  int R[kNF];
  int Nf[kNF];     // agent split of a row in the gather
  double* sum;
  double* mn;
  float* maxp;
  int32_t* err;
};

namespace mm {
namespace {

struct MlpField {
  float* store;
  const float* src;   // insert source / unused in gather
  float* dst;         // gather destination / unused in insert
  uint32_t R, Nf;
};
struct MlpFieldSet {
  MlpField f[kNF];
  int nf;
};

__global__ __launch_bounds__(256) void mlp_insert_kernel(MlpFieldSet fs, uint32_t n, int64_t first, int64_t size) {
  const MlpField& F = fs.f[blockIdx.y];
  const uint64_t total = (uint64_t)n * F.R;
  for (uint64_t o = (uint64_t)blockIdx.x * 256 + threadIdx.x; o < total; o += (uint64_t)gridDim.x * 256) {
    const uint64_t i = o / F.R, r = o - i * F.R;
    const int64_t slot = (first + (int64_t)i) % size;
    F.store[(size_t)slot * F.R + r] = F.src[o];
  }
}

// an index outside [0, size) reads nothing: its rows are written as 0 and bit 2 of err is set
__global__ __launch_bounds__(256) void mlp_gather_kernel(MlpFieldSet fs, uint32_t B, const int64_t* __restrict__ idx,
                                                         int64_t size, int32_t* err) {
  const MlpField& F = fs.f[blockIdx.y];
  const uint32_t X = F.R / F.Nf;
  const uint64_t total = (uint64_t)B * F.R;
  for (uint64_t o = (uint64_t)blockIdx.x * 256 + threadIdx.x; o < total; o += (uint64_t)gridDim.x * 256) {
    const uint64_t x = o % X, q = o / X, b = q % B, nf = q / B;
    const int64_t slot = idx[b];
    if (slot < 0 || slot >= size) {
      F.dst[o] = 0.0f;
      if (x + nf == 0) atomicOr(err, 4);
      continue;
    }
    F.dst[o] = F.store[(size_t)slot * F.R + nf * X + x];
  }
}

int mlp_grid(const MlpFieldSet& fs, uint32_t units) {
  uint64_t mx = 0;
  for (int i = 0; i < fs.nf; ++i) mx = std::max<uint64_t>(mx, (uint64_t)units * fs.f[i].R);
  return (int)std::min<uint64_t>(std::max<uint64_t>((mx + 255) / 256, 1), 2048);
}

// The ring slot the next insert starts at. The cursor is the reference's current_i = idx_range[-1] + 1, which lies in
// (0, size] after an insert: size stands for slot 0
int64_t first_slot(const mm_mlpbuf* b) { return b->current % b->size; }

// the leaf writes of an insert of n transitions at ring slot first (< size)
int set_leaves(mm_mlpbuf* b, int64_t first, int64_t n, hipStream_t st) {
  if (!b->d.prioritized) return MM_OK;
  // reference: range(idx_range[0], idx_range[1]) = the first slot's leaf unless the second slot wrapped to 0
  const int64_t cnt = b->d.leaf_mode ? n : (first + 1 < b->size ? 1 : 0);
  if (cnt == 0) return MM_OK;
  hipLaunchKernelGGL(erb_set_kernel, dim3(1), dim3(1024), 0, st, b->sum, b->mn, b->itcap, (int)cnt,
                     (const int64_t*)nullptr, first, b->size, (const float*)nullptr, b->maxp, b->alpha_f, (int64_t)-1,
                     (int32_t*)nullptr);
  MM_HIP_CHECK(hipGetLastError());
  return MM_OK;
}

void advance(mm_mlpbuf* b, int64_t n, int64_t* idx_range_host) {
  const int64_t first = first_slot(b);
  if (idx_range_host)
    for (int64_t i = 0; i < n; ++i) idx_range_host[i] = (first + i) % b->size;
  b->current = (first + n - 1) % b->size + 1;
  b->filled = std::min<int64_t>(b->filled + n, b->size);
}

}  // namespace
}  // namespace mm

extern "C" {

int mm_mlpbuf_create(const mm_mlpbuf_dims* d, int64_t buffer_size, double alpha, mm_mlpbuf** out) {
  MM_REQUIRE(d && out && buffer_size >= 1 && buffer_size < (1ll << 30), "mlpbuf_create: bad arguments");
  MM_REQUIRE(d->N >= 1 && d->D >= 1 && d->S >= 1 && d->A >= 1, "mlpbuf_create: bad dims");
  MM_REQUIRE(d->store_share || d->S == d->N * d->D,
             "mlpbuf_create: without store_share the share_obs dim S (%d) must be N * D (%d)", d->S, d->N * d->D);
  mm_mlpbuf* b = new mm_mlpbuf;
  b->d = *d;
  b->size = buffer_size;
  b->itcap = 1;
  while (b->itcap < buffer_size) b->itcap *= 2;
  b->filled = b->current = 0;
  b->alpha_f = (float)alpha;
  const int N = d->N, sh = d->store_share ? d->S : 0;
  const int R[kNF] = {N * d->D, sh, N * d->A, N, N * d->D, sh, N, 1, N};
  const int Nf[kNF] = {N, 1, N, N, N, 1, N, 1, N};
  size_t off[kNF + 1];
  off[0] = 0;
  for (int i = 0; i < kNF; ++i) {
    b->R[i] = R[i];
    b->Nf[i] = Nf[i];
    off[i + 1] = off[i] + (((size_t)buffer_size * R[i] * 4 + 255) & ~size_t(255));
  }
  MM_REQUIRE(off[kNF] < (1ull << 40), "mlpbuf_create: too large");
  const size_t tree_b = ((size_t)2 * b->itcap * 8 + 255) & ~size_t(255);
  const size_t total = off[kNF] + 2 * tree_b + 256;
  void* base = nullptr;
  if (hipMalloc(&base, total) != hipSuccess) {
    delete b;
    mm::set_error("mlpbuf_create: hipMalloc of %zu bytes failed", total);
    return MM_ENOMEM;
  }
  b->alloc = base;
  char* p = static_cast<char*>(base);
  for (int i = 0; i < kNF; ++i) b->f[i] = R[i] ? reinterpret_cast<float*>(p + off[i]) : nullptr;
  b->sum = reinterpret_cast<double*>(p + off[kNF]);
  b->mn = reinterpret_cast<double*>(p + off[kNF] + tree_b);
  b->maxp = reinterpret_cast<float*>(p + off[kNF] + 2 * tree_b);
  b->err = reinterpret_cast<int32_t*>(p + off[kNF] + 2 * tree_b + 4);
  // stores zero, dones / dones_env one (mlp_buffer.py:153-156: "default to done being True")
  std::vector<double> inf_tree(2 * b->itcap, INFINITY);
  const float one = 1.0f;
  bool ok = hipMemset(base, 0, off[kNF] + tree_b) == hipSuccess &&
            hipMemcpy(b->mn, inf_tree.data(), 2 * b->itcap * 8, hipMemcpyHostToDevice) == hipSuccess &&
            hipMemcpy(b->maxp, &one, 4, hipMemcpyHostToDevice) == hipSuccess && hipMemset(b->err, 0, 4) == hipSuccess;
  for (int i = 6; i <= 7 && ok; ++i)
    ok = hipMemsetD32(reinterpret_cast<hipDeviceptr_t>(b->f[i]), 0x3f800000, (size_t)buffer_size * R[i]) == hipSuccess;
  if (!ok || hipDeviceSynchronize() != hipSuccess) {
    (void)hipFree(base);
    delete b;
    mm::set_error("mlpbuf_create: init failed");
    return MM_EHIP;
  }
  *out = b;
  return MM_OK;
}

void mm_mlpbuf_destroy(mm_mlpbuf* b) {
  if (!b) return;
  (void)hipFree(b->alloc);
  delete b;
}

int mm_mlpbuf_insert(mm_mlpbuf* b, int32_t n, const mm_mlpbuf_fields* src, int64_t* idx_range_host, mm_stream_t s) {
  MM_REQUIRE(b && src && n >= 1 && n <= b->size, "mlpbuf_insert: bad arguments (n must be in [1, buffer_size])");
  MM_REQUIRE(!(b->d.prioritized && !b->d.leaf_mode && n < 2),
             "mlpbuf_insert: leaf_mode reference needs n >= 2 (the reference reads idx_range[1])");
  const float* in[kNF] = {src->obs,  src->share_obs, src->acts,      src->rewards,         src->next_obs,
                          src->next_share_obs, src->dones, src->dones_env, src->valid_transition};
  mm::MlpFieldSet fs;
  fs.nf = 0;
  for (int i = 0; i < kNF; ++i) {
    if (!b->f[i]) continue;   // share fields without store_share
    MM_REQUIRE(in[i] != nullptr, "mlpbuf_insert: field %d is NULL", i);
    fs.f[fs.nf++] = {b->f[i], in[i], nullptr, (uint32_t)b->R[i], (uint32_t)b->Nf[i]};
  }
  hipStream_t st = (hipStream_t)s;
  hipLaunchKernelGGL(mm::mlp_insert_kernel, dim3(mm::mlp_grid(fs, n), fs.nf), dim3(256), 0, st, fs, (uint32_t)n,
                     mm::first_slot(b), b->size);
  MM_HIP_CHECK(hipGetLastError());
  const int rc = mm::set_leaves(b, mm::first_slot(b), n, st);
  if (rc) return rc;
  mm::advance(b, n, idx_range_host);
  return MM_OK;
}

int mm_mlpbuf_stores(mm_mlpbuf* b, mm_mlpbuf_fields* out) {
  MM_REQUIRE(b && out, "mlpbuf_stores: bad arguments");
  *out = {b->f[0], b->f[1], b->f[2], b->f[3], b->f[4], b->f[5], b->f[6], b->f[7], b->f[8]};
  return MM_OK;
}

int mm_mlpbuf_advance(mm_mlpbuf* b, int64_t n, int64_t* idx_range_host, mm_stream_t s) {
  MM_REQUIRE(b && n >= 1 && n <= b->size, "mlpbuf_advance: bad arguments (n must be in [1, buffer_size])");
  MM_REQUIRE(!(b->d.prioritized && !b->d.leaf_mode && n < 2), "mlpbuf_advance: leaf_mode reference needs n >= 2");
  const int rc = mm::set_leaves(b, mm::first_slot(b), n, (hipStream_t)s);
  if (rc) return rc;
  mm::advance(b, n, idx_range_host);
  return MM_OK;
}

int64_t mm_mlpbuf_len(const mm_mlpbuf* b) { return b ? b->filled : -1; }
int64_t mm_mlpbuf_current(const mm_mlpbuf* b) { return b ? b->current : -1; }
int64_t mm_mlpbuf_it_capacity(const mm_mlpbuf* b) { return b ? b->itcap : -1; }

int mm_mlpbuf_sample_prioritized(mm_mlpbuf* b, int32_t B, double beta, const double* fracs, uint64_t seed,
                                 uint64_t counter, int64_t* idx_out, double* w_out, float* w32_out, mm_stream_t s) {
  MM_REQUIRE(b && b->d.prioritized && idx_out && B >= 1, "mlpbuf_sample_prioritized: bad arguments");
  MM_REQUIRE(b->filled > B, "mlpbuf_sample_prioritized: Not enough samples in the buffer! (len %lld <= batch %d)",
             (long long)b->filled, B);
  MM_REQUIRE(beta > 0, "mlpbuf_sample_prioritized: beta must be > 0");
  hipLaunchKernelGGL(mm::erb_sample_kernel, dim3(1), dim3(256), 0, (hipStream_t)s, b->sum, b->mn, b->itcap, b->filled,
                     (int)B, beta, fracs, seed, counter, idx_out, w_out, w32_out);
  MM_HIP_CHECK(hipGetLastError());
  return MM_OK;
}

int mm_mlpbuf_sample_uniform(mm_mlpbuf* b, int32_t B, uint64_t seed, uint64_t counter, int64_t* idx_out,
                             mm_stream_t s) {
  MM_REQUIRE(b && idx_out && B >= 1 && b->filled >= 1, "mlpbuf_sample_uniform: bad arguments / empty buffer");
  hipLaunchKernelGGL(mm::erb_uniform_kernel, dim3((B + 255) / 256), dim3(256), 0, (hipStream_t)s, b->filled, (int)B,
                     seed, counter, idx_out);
  MM_HIP_CHECK(hipGetLastError());
  return MM_OK;
}

int mm_mlpbuf_gather(mm_mlpbuf* b, int32_t B, const int64_t* idx, const mm_mlpbuf_fields* dst, mm_stream_t s) {
  MM_REQUIRE(b && idx && dst && B >= 1, "mlpbuf_gather: bad arguments");
  float* out[kNF] = {dst->obs,  dst->share_obs, dst->acts,      dst->rewards,         dst->next_obs,
                     dst->next_share_obs, dst->dones, dst->dones_env, dst->valid_transition};
  mm::MlpFieldSet fs;
  fs.nf = 0;
  for (int i = 0; i < kNF; ++i) {
    if (!out[i]) continue;
    // without store_share a cent_obs row is the obs row of the same transition, taken whole
    const int from = b->f[i] ? i : i - 1;
    fs.f[fs.nf++] = {b->f[from], nullptr, out[i], (uint32_t)b->R[from], (uint32_t)b->Nf[i]};
  }
  if (fs.nf == 0) return MM_OK;
  hipLaunchKernelGGL(mm::mlp_gather_kernel, dim3(mm::mlp_grid(fs, B), fs.nf), dim3(256), 0, (hipStream_t)s, fs,
                     (uint32_t)B, idx, b->size, b->err);
  MM_HIP_CHECK(hipGetLastError());
  return MM_OK;
}

int mm_mlpbuf_update_priorities(mm_mlpbuf* b, const int64_t* idx, const float* prio, int32_t B, mm_stream_t s) {
  MM_REQUIRE(b && b->d.prioritized && idx && prio && B >= 1, "mlpbuf_update_priorities: bad arguments");
  hipLaunchKernelGGL(mm::erb_set_kernel, dim3(1), dim3(1024), 0, (hipStream_t)s, b->sum, b->mn, b->itcap, (int)B, idx,
                     (int64_t)0, (int64_t)1, prio, b->maxp, b->alpha_f, b->filled, b->err);
  MM_HIP_CHECK(hipGetLastError());
  return MM_OK;
}

int mm_mlpbuf_copy_state(mm_mlpbuf* b, double* sum_dst, double* min_dst, float* maxp_dst, int32_t* err_dst,
                         mm_stream_t s) {
  MM_REQUIRE(b, "mlpbuf_copy_state: NULL handle");
  hipStream_t st = (hipStream_t)s;
  const size_t tb = (size_t)2 * b->itcap * 8;
  if (sum_dst) MM_HIP_CHECK(hipMemcpyAsync(sum_dst, b->sum, tb, hipMemcpyDeviceToDevice, st));
  if (min_dst) MM_HIP_CHECK(hipMemcpyAsync(min_dst, b->mn, tb, hipMemcpyDeviceToDevice, st));
  if (maxp_dst) MM_HIP_CHECK(hipMemcpyAsync(maxp_dst, b->maxp, 4, hipMemcpyDeviceToDevice, st));
  if (err_dst) MM_HIP_CHECK(hipMemcpyAsync(err_dst, b->err, 4, hipMemcpyDeviceToDevice, st));
  return MM_OK;
}

}  // extern "C"
