// Negative edges drawn on the device: the contract of framework/graph_utils.negative_sampling - int64
// [2, n_out] node pairs (a, b), a != b, a * n + b not among the sorted unique keys of the positive edges, uniform over all
// such pairs, independently per slot - as a pure function of (seed, *counter, slot, pos_keys, n_nodes).  One thread per slot:
//
//   base = mix64(seed ^ mix64(counter))
//   for t < 64:  c = mulhi64(mix64(base + 64 * slot + t), n^2);  accept unless c / n == c % n or c is a key (binary search)
//   after 64 rejected tries:  c <- (c + 1) mod n^2, at most n^2 times, until one is accepted
//
// The entry refuses graphs where more than half of all n^2 pairs are excluded, so a try is rejected with probability <= 1/2,
// the linear probe is reached with probability <= 2^-64 per slot, and it ends because an allowed pair exists.  No generator
// state, no atomics, no compaction, no count to read back; every loop has a bound.  gnndelete_amd/negatives.py restates the
// stream in numpy (reference_draw), bit for bit.
#include "common.h"

namespace gd {

constexpr int kNegTries = 64;

__device__ __forceinline__ bool negative_allowed(uint64_t c, uint64_t n, const int64_t* __restrict__ keys, int64_t n_keys) {
  if (c / n == c % n) return false;
  int64_t lo = 0, hi = n_keys;                                  // first key >= c; n_keys < 2^62: 63 halvings at the most
  for (int s = 0; s < 64 && lo < hi; ++s) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if ((uint64_t)keys[mid] < c) lo = mid + 1; else hi = mid;
  }
  return !(lo < n_keys && (uint64_t)keys[lo] == c);
}

__global__ __launch_bounds__(256) void negative_edges_kernel(const int64_t* __restrict__ keys, int64_t n_keys, uint64_t n,
                                                             uint64_t seed, const int64_t* __restrict__ counter, int64_t n_out,
                                                             int64_t* __restrict__ out, int64_t ld_out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n_out) return;
  const uint64_t nn = n * n;
  const uint64_t base = mix64(seed ^ mix64(counter ? (uint64_t)*counter : 0ull));
  uint64_t c = 0;
  bool ok = false;
  for (int t = 0; t < kNegTries && !ok; ++t) {
    c = __umul64hi(mix64(base + (uint64_t)kNegTries * (uint64_t)i + (uint64_t)t), nn);
    ok = negative_allowed(c, n, keys, n_keys);
  }
  for (uint64_t k = 0; k < nn && !ok; ++k) {                    // the probe: from the last rejected candidate, one pass at the most
    c = c + 1 == nn ? 0 : c + 1;
    ok = negative_allowed(c, n, keys, n_keys);
  }
  out[i] = (int64_t)(c / n);
  out[ld_out + i] = (int64_t)(c % n);
}

}  // namespace gd

extern "C" int gd_negative_edges(const int64_t* pos_keys, int64_t n_keys, int64_t n_nodes, uint64_t seed, const int64_t* counter,
                                 int64_t n_out, int64_t* out, int64_t ld_out, void* stream) {
  using namespace gd;
  GD_REQUIRE(n_keys >= 0 && n_nodes >= 1 && n_nodes < (1ll << 31) && n_out >= 0 && n_out < (1ll << 36), GD_E_DIM,
             "gd_negative_edges: n_keys=%lld n_nodes=%lld n_out=%lld out of range", (long long)n_keys, (long long)n_nodes,
             (long long)n_out);
  // 2 (n_keys + n_nodes) <= n_nodes^2, written so that no n_keys overflows it
  GD_REQUIRE(n_keys <= n_nodes * n_nodes && n_keys + n_nodes <= n_nodes * n_nodes / 2, GD_E_DIM,
             "gd_negative_edges: %lld keys and %lld self loops exclude more than half of the %lld^2 pairs", (long long)n_keys,
             (long long)n_nodes, (long long)n_nodes);
  if (n_out == 0) return GD_OK;
  GD_REQUIRE(out && (pos_keys || n_keys == 0), GD_E_NULL, "gd_negative_edges: null pointer");
  GD_REQUIRE(ld_out >= n_out, GD_E_DIM, "gd_negative_edges: ld_out=%lld below n_out=%lld", (long long)ld_out, (long long)n_out);
  hipLaunchKernelGGL(negative_edges_kernel, dim3((unsigned)((n_out + 255) / 256)), dim3(256), 0, (hipStream_t)stream, pos_keys, n_keys,
                     (uint64_t)n_nodes, seed, counter, n_out, out, ld_out);
  return launched("negative_edges");
}
