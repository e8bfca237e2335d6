// Resampled ROC-AUC / average precision without the [B, 2k] sort (gnndelete_amd/rankeval.py, Trainer.eval --fused_eval).
//
// Every subset ranks the SAME negatives (`ref`, n_ref scores, label 0) against k positives drawn from ONE pool of m scores, so
// the ranking is split: once per validation the pool is sorted descending and every pool score is located in the ascending ref
// (gd_rank_counts_f32: less / leq per score); per subset a membership bitmap over the pool's sorted positions, a popcount
// prefix and one pass over the set bits give both metrics (gd_subset_rank_metrics).  By sorted position p of the pool:
//
//   u2[p]      = 2 less + (leq - less)         twice the Mann-Whitney credit of the score at p
//   ge_at[p]   = n_ref - less                  the negatives at or above the score at p
//   run_end[p] = the last position whose score equals the score at p
//   AUC_b = double(sum of u2 over the members) / (2 k n_ref)                                     (integer sum: exact)
//   AP_b  = (1 / k) sum over the members p of TP(p) / (TP(p) + ge_at[p]),  TP(p) = members at positions <= run_end[p]
//
// gd_subset_rank_metrics: one 1024-thread block per subset, four phases on the subset's own two workspace rows (bitmap words,
// exclusive popcount prefix per word), each row starting on a 128-byte line of its own:
//   1  zero the bitmap row (plain stores; no memset call)
//   2  OR the members' bits in (integer atomics at L2: the result does not depend on arrival order)
//   3  exclusive popcount prefix per word: a block scan over chunks of 1024 words with a carried total
//   4  thread t walks words t, t + 1024, ...: for every set bit the u2 and AP terms; a fixed-order block reduction
// Between two phases every wave drains its stores / atomics (s_waitcnt vmcnt(0)) and the block meets at a barrier, and every
// load of a word that this launch stored or OR-ed is an L2-served (agent-scope relaxed) load, so no phase can read a line
// that this compute unit's L1 kept from before the store.  The same inputs give the same bits on every call: integer
// atomics, a fixed thread-to-word mapping and a fixed reduction tree; no float atomics.  Every index read from memory
// (idx, pos, run_end) is range-checked before it addresses anything: a NaN score or a broken index gives a meaningless
// value, never an access outside the arrays.
//
// gd_subset_rank_metrics_drawn (--device_subsets) is the same kernel with another member source: phase 2 computes member j of
// subset b instead of reading idx[b, j], so a ranking needs no index matrix and no launches that draw one.  The stream is a
// keyed permutation of [0, m) per subset whose first k outputs are the subset - a pure function of (seed, draw, b, j, m) in
// integer operations (fmix32 = the murmur3 32-bit finaliser, mix64 = the splitmix64 finaliser of common.h):
//
//   bits = max(6, bit_length(m - 1)) rounded up to even;  h = bits / 2;  mask = 2^h - 1            (32 <= m < 2^31: h <= 16)
//   base = mix64(seed ^ mix64(draw));  kb = mix64(base + b);  key[r] = the low 32 bits of mix64(kb + r),  r = 0 .. 11
//   P(v):  L = v >> h, R = v & mask;  twelve times (L, R) <- (R, L ^ (fmix32(R ^ key[r]) & mask));  (L << h) | R
//   e(b, j) = the first of P(j), P(P(j)), ... below m                                              (cycle walking, uint32)
//
// P is a balanced Feistel network, a bijection of [0, 2^bits) whatever the round function; the walk from j < m stays on j's
// cycle of P, which returns to j < m after at most 2^bits applications, so it ends and the loop's bound of 2^bits is never
// reached; j -> e(b, j) is then a bijection of [0, m) (the permutation P induces on the subset [0, m) of its domain), so the
// k members of a subset are distinct - the precondition above.  2^bits < 4 m: fewer than 4 applications per member on
// average.  A subset's twelve keys are computed once per block (threads 0 .. 11, through LDS) and held in scalar registers.
// The OR of phase 2 does not depend on order and phases 1, 3 and 4 are the same code, so the drawn entry gives the bits of
// gd_subset_rank_metrics on the matrix gd_subset_draw writes.  gnndelete_amd/subsets.reference_draw restates the stream.
#include "common.h"

namespace gd {

constexpr int kRankBlock = 1024;                   // threads per subset block = words per scan chunk
constexpr int kRankWaves = kRankBlock / kWave;
constexpr int64_t kRankLineWords = 32;             // 128-byte line

inline int64_t rank_row_words(int64_t m) {         // bitmap (and prefix) words per subset, whole lines
  const int64_t w = (m + 31) / 32;
  return (w + kRankLineWords - 1) / kRankLineWords * kRankLineWords;
}

__global__ __launch_bounds__(256) void rank_counts_kernel(const float* __restrict__ ref, int32_t n_ref, const float* __restrict__ query,
                                                          int64_t m, int32_t* __restrict__ less, int32_t* __restrict__ leq) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= m) return;
  const float q = query[i];
  int32_t lo = 0, hi = n_ref;                                   // first ref >= q; n_ref < 2^31: 31 halvings at the most
  for (int s = 0; s < 32 && lo < hi; ++s) {
    const int32_t mid = lo + ((hi - lo) >> 1);
    if (ref[mid] < q) lo = mid + 1; else hi = mid;
  }
  const int32_t n_less = lo;
  hi = n_ref;                                                   // first ref > q, from there on
  for (int s = 0; s < 32 && lo < hi; ++s) {
    const int32_t mid = lo + ((hi - lo) >> 1);
    if (ref[mid] <= q) lo = mid + 1; else hi = mid;
  }
  less[i] = n_less;
  leq[i] = lo;
}

constexpr int kDrawRounds = 12;                    // Feistel rounds of the subset stream: part of the stream, not a tuning knob

inline int draw_half_bits(int64_t m) {             // h: half the width of the permutation's domain, 3 .. 16 for 32 <= m < 2^31
  int bits = 6;
  while (bits < 32 && (1ll << bits) < m) ++bits;   // bit_length(m - 1), at least 6
  return (bits + 1) / 2;
}

__device__ __forceinline__ uint32_t fmix32(uint32_t x) {       // the murmur3 32-bit finaliser
  x ^= x >> 16;
  x *= 0x85ebca6bu;
  x ^= x >> 13;
  x *= 0xc2b2ae35u;
  return x ^ (x >> 16);
}

// The keys of subset b into key[0 .. 11], the same in every lane (scalar registers).  Every thread of the block calls it
// with the same (seed, draw, b); `slot` is the block's LDS row of kDrawRounds words.  Two barriers inside.
__device__ __forceinline__ void draw_keys(uint64_t seed, uint64_t draw, uint64_t b, uint32_t* slot, uint32_t (&key)[kDrawRounds]) {
  __syncthreads();                                              // (a block that loops over subsets: the last readers are done)
  if (threadIdx.x < kDrawRounds) {
    const uint64_t kb = mix64(mix64(seed ^ mix64(draw)) + b);
    slot[threadIdx.x] = (uint32_t)mix64(kb + (uint64_t)threadIdx.x);
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < kDrawRounds; ++r) key[r] = __builtin_amdgcn_readfirstlane(slot[r]);
}

// Member j (< m) of the subset with these keys: cycle walking on the Feistel permutation of [0, 2^(2h)).  In [0, m) always:
// the bound of 2^(2h) applications is never reached (see above), and a value that reached it would be clamped.
__device__ __forceinline__ uint32_t draw_member(uint32_t j, uint32_t m, int h, const uint32_t (&key)[kDrawRounds]) {
  const uint32_t mask = (1u << h) - 1u;
  uint32_t v = j;
  for (uint64_t n = 0, bound = 1ull << (2 * h); n < bound; ++n) {
    uint32_t l = v >> h, r = v & mask;
#pragma unroll
    for (int i = 0; i < kDrawRounds; ++i) {
      const uint32_t f = l ^ (fmix32(r ^ key[i]) & mask);
      l = r;
      r = f;
    }
    v = (l << h) | r;
    if (v < m) return v;
  }
  return j;                                                     // (unreachable for j < m)
}

// a word this launch stored or OR-ed: served by L2, never by a line the L1 may have kept
__device__ __forceinline__ uint32_t load_l2(uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
// end of a phase: this wave's stores and atomics have reached L2, then the block meets
__device__ __forceinline__ void phase_end() {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
}

// kDrawn = false: member j of subset b is idx[b * ld_idx + j] (seed / draw unused); true: draw_member (idx / ld_idx unused)
template <bool kDrawn>
__global__ __launch_bounds__(kRankBlock) void subset_rank_kernel(const int32_t* __restrict__ u2, const int32_t* __restrict__ ge_at,
                                                                 const int32_t* __restrict__ run_end, const int32_t* __restrict__ pos,
                                                                 const int64_t* __restrict__ idx, int64_t ld_idx, uint64_t seed,
                                                                 uint64_t draw, int half_bits, int64_t n_sub, int32_t k, int32_t m,
                                                                 int32_t n_ref, double* __restrict__ auc, double* __restrict__ ap,
                                                                 uint32_t* workspace, int64_t row_words) {
  __shared__ int32_t wave_count[2][kRankWaves];
  __shared__ uint32_t draw_slot[kDrawRounds];
  __shared__ long long wave_u2[kRankWaves];
  __shared__ double wave_ap[kRankWaves];
  const int64_t b = blockIdx.x;
  if (b >= n_sub) return;                                       // (uniform over the block)
  const int t = threadIdx.x, lane = t & (kWave - 1), wave = t / kWave;
  const int32_t n_words = (int32_t)(((int64_t)m + 31) >> 5);    // <= row_words
  uint32_t* bits = workspace + 2 * b * row_words;
  uint32_t* prefix = bits + row_words;

  // 1: the subset's own bitmap row
  for (int32_t w = t; w < n_words; w += kRankBlock) bits[w] = 0u;
  phase_end();

  // 2: the members' bits, by sorted position
  if constexpr (kDrawn) {
    uint32_t key[kDrawRounds];
    draw_keys(seed, draw, (uint64_t)b, draw_slot, key);
    for (int64_t j = t; j < k; j += kRankBlock) {
      const int64_t e = draw_member((uint32_t)j, (uint32_t)m, half_bits, key);
      if (e < 0 || e >= m) continue;
      const int32_t p = pos[e];
      if (p < 0 || p >= m) continue;
      __hip_atomic_fetch_or(bits + (p >> 5), 1u << (p & 31), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  } else {
    const int64_t* row = idx + b * ld_idx;
    for (int64_t j = t; j < k; j += kRankBlock) {
      const int64_t e = row[j];
      if (e < 0 || e >= m) continue;
      const int32_t p = pos[e];
      if (p < 0 || p >= m) continue;
      __hip_atomic_fetch_or(bits + (p >> 5), 1u << (p & 31), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
  phase_end();

  // 3: exclusive popcount prefix per word; `carry` = the set bits of the chunks before this one, the same in every thread
  int32_t carry = 0;
  for (int32_t base = 0, c = 0; base < n_words; base += kRankBlock, ++c) {
    const int32_t w = base + t;
    const int32_t cnt = w < n_words ? __popc(load_l2(bits + w)) : 0;
    int32_t incl = cnt;                                         // inclusive scan over the wave
#pragma unroll
    for (int off = 1; off < kWave; off <<= 1) {
      const int32_t v = __shfl_up(incl, off);
      if (lane >= off) incl += v;
    }
    if (lane == kWave - 1) wave_count[c & 1][wave] = incl;
    __syncthreads();                                            // (the other parity's slots are read before the next barrier)
    int32_t before = 0, total = 0;
#pragma unroll
    for (int v = 0; v < kRankWaves; ++v) {
      const int32_t n = wave_count[c & 1][v];
      if (v < wave) before += n;
      total += n;
    }
    if (w < n_words) prefix[w] = (uint32_t)(carry + before + incl - cnt);
    carry += total;
  }
  phase_end();

  // 4: every member's terms, words dealt to threads in a fixed pattern
  long long s_u2 = 0;
  double s_ap = 0.0;
  for (int32_t w = t; w < n_words; w += kRankBlock) {
    const uint32_t word = load_l2(bits + w);
    for (uint32_t rest = word; rest != 0u; rest &= rest - 1u) {
      const int64_t at = ((int64_t)w << 5) + (__ffs((int)rest) - 1);
      if (at >= m) break;                                       // (no bit is set there: phase 2 checks p < m)
      const int32_t p = (int32_t)at;
      int32_t re = run_end[p];
      re = re < p ? p : (re >= m ? m - 1 : re);
      const int32_t rw = re >> 5;
      const uint32_t upto = (rw == w ? word : load_l2(bits + rw)) & (0xFFFFFFFFu >> (31 - (re & 31)));
      const double tp = (double)(load_l2(prefix + rw) + (uint32_t)__popc(upto));   // >= 1: p itself is a member
      s_ap += tp / (tp + (double)ge_at[p]);
      s_u2 += (long long)u2[p];
    }
  }
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) {
    s_u2 += __shfl_xor(s_u2, off);
    s_ap += __shfl_xor(s_ap, off);
  }
  if (lane == 0) {
    wave_u2[wave] = s_u2;
    wave_ap[wave] = s_ap;
  }
  __syncthreads();
  if (t == 0) {
    long long su = 0;
    double sa = 0.0;
    for (int v = 0; v < kRankWaves; ++v) {
      su += wave_u2[v];
      sa += wave_ap[v];
    }
    auc[b] = (double)su / (2.0 * (double)k * (double)n_ref);
    ap[b] = sa / (double)k;
  }
}

// gd_subset_draw: block (x, y) writes members x * 1024 .. of the subsets y, y + gridDim.y, ...; one thread per member
__global__ __launch_bounds__(kRankBlock) void subset_draw_kernel(uint64_t seed, uint64_t draw, int half_bits, int64_t n_sub, int32_t k,
                                                                 int32_t m, int64_t* __restrict__ out, int64_t ld_out) {
  __shared__ uint32_t draw_slot[kDrawRounds];
  const int64_t j = (int64_t)blockIdx.x * kRankBlock + threadIdx.x;
  for (int64_t b = blockIdx.y; b < n_sub; b += gridDim.y) {      // (uniform over the block: draw_keys holds barriers)
    uint32_t key[kDrawRounds];
    draw_keys(seed, draw, (uint64_t)b, draw_slot, key);
    if (j < k) out[b * ld_out + j] = (int64_t)draw_member((uint32_t)j, (uint32_t)m, half_bits, key);
  }
}

}  // namespace gd

extern "C" int gd_rank_counts_f32(const float* ref, int64_t n_ref, const float* query, int64_t m, int32_t* less, int32_t* leq,
                                  void* stream) {
  using namespace gd;
  GD_REQUIRE(n_ref >= 1 && n_ref < (1ll << 31) && m >= 0 && m < (1ll << 31), GD_E_DIM,
             "gd_rank_counts_f32: n_ref=%lld m=%lld out of range", (long long)n_ref, (long long)m);
  if (m == 0) return GD_OK;
  GD_REQUIRE(ref && query && less && leq, GD_E_NULL, "gd_rank_counts_f32: null pointer");
  hipLaunchKernelGGL(rank_counts_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, (hipStream_t)stream, ref, (int32_t)n_ref, query,
                     m, less, leq);
  return launched("rank_counts");
}

extern "C" int64_t gd_subset_rank_workspace(int64_t n_sub, int64_t m) {
  if (n_sub < 0 || n_sub >= (1ll << 31) || m < 1 || m >= (1ll << 31)) return -1;
  return n_sub * 2 * gd::rank_row_words(m) * (int64_t)sizeof(uint32_t);
}

extern "C" int gd_subset_rank_metrics(const int32_t* u2, const int32_t* ge_at, const int32_t* run_end, const int32_t* pos,
                                      const int64_t* idx, int64_t ld_idx, int64_t n_sub, int64_t k, int64_t m, int64_t n_ref, double* auc,
                                      double* ap, void* workspace, int64_t workspace_bytes, void* stream) {
  using namespace gd;
  GD_REQUIRE(n_sub >= 0 && n_sub < (1ll << 31) && m >= 1 && m < (1ll << 31) && k >= 1 && k <= m && n_ref >= 1 && n_ref < (1ll << 30),
             GD_E_DIM, "gd_subset_rank_metrics: n_sub=%lld k=%lld m=%lld n_ref=%lld out of range (1 <= k <= m < 2^31, 1 <= n_ref < 2^30)",
             (long long)n_sub, (long long)k, (long long)m, (long long)n_ref);
  if (n_sub == 0) return GD_OK;
  GD_REQUIRE(u2 && ge_at && run_end && pos && idx && auc && ap && workspace, GD_E_NULL, "gd_subset_rank_metrics: null pointer");
  GD_REQUIRE(ld_idx >= k || n_sub == 1, GD_E_DIM, "gd_subset_rank_metrics: ld_idx=%lld below k=%lld", (long long)ld_idx, (long long)k);
  GD_REQUIRE(aligned16(workspace), GD_E_ALIGN, "gd_subset_rank_metrics: workspace not 16-byte aligned");
  GD_REQUIRE(workspace_bytes >= gd_subset_rank_workspace(n_sub, m), GD_E_WORKSPACE,
             "gd_subset_rank_metrics: workspace of %lld bytes, %lld needed", (long long)workspace_bytes,
             (long long)gd_subset_rank_workspace(n_sub, m));
  hipLaunchKernelGGL(subset_rank_kernel<false>, dim3((unsigned)n_sub), dim3(kRankBlock), 0, (hipStream_t)stream, u2, ge_at, run_end, pos, idx,
                     ld_idx, (uint64_t)0, (uint64_t)0, 0, n_sub, (int32_t)k, (int32_t)m, (int32_t)n_ref, auc, ap, (uint32_t*)workspace,
                     rank_row_words(m));
  return launched("subset_rank_metrics");
}

extern "C" int gd_subset_rank_metrics_drawn(const int32_t* u2, const int32_t* ge_at, const int32_t* run_end, const int32_t* pos,
                                            uint64_t seed, uint64_t draw, int64_t n_sub, int64_t k, int64_t m, int64_t n_ref, double* auc,
                                            double* ap, void* workspace, int64_t workspace_bytes, void* stream) {
  using namespace gd;
  GD_REQUIRE(n_sub >= 0 && n_sub < (1ll << 31) && m >= 1 && m < (1ll << 31) && k >= 1 && k <= m && n_ref >= 1 && n_ref < (1ll << 30),
             GD_E_DIM, "gd_subset_rank_metrics_drawn: n_sub=%lld k=%lld m=%lld n_ref=%lld out of range (1 <= k <= m < 2^31, 1 <= n_ref < 2^30)",
             (long long)n_sub, (long long)k, (long long)m, (long long)n_ref);
  GD_REQUIRE(m >= 32, GD_E_DIM, "gd_subset_rank_metrics_drawn: a pool of m=%lld (the subset stream takes 32 and more)", (long long)m);
  if (n_sub == 0) return GD_OK;
  GD_REQUIRE(u2 && ge_at && run_end && pos && auc && ap && workspace, GD_E_NULL, "gd_subset_rank_metrics_drawn: null pointer");
  GD_REQUIRE(aligned16(workspace), GD_E_ALIGN, "gd_subset_rank_metrics_drawn: workspace not 16-byte aligned");
  GD_REQUIRE(workspace_bytes >= gd_subset_rank_workspace(n_sub, m), GD_E_WORKSPACE,
             "gd_subset_rank_metrics_drawn: workspace of %lld bytes, %lld needed", (long long)workspace_bytes,
             (long long)gd_subset_rank_workspace(n_sub, m));
  hipLaunchKernelGGL(subset_rank_kernel<true>, dim3((unsigned)n_sub), dim3(kRankBlock), 0, (hipStream_t)stream, u2, ge_at, run_end, pos,
                     (const int64_t*)nullptr, (int64_t)0, seed, draw, draw_half_bits(m), n_sub, (int32_t)k, (int32_t)m, (int32_t)n_ref, auc, ap,
                     (uint32_t*)workspace, rank_row_words(m));
  return launched("subset_rank_metrics_drawn");
}

extern "C" int gd_subset_draw(uint64_t seed, uint64_t draw, int64_t n_sub, int64_t k, int64_t m, int64_t* out, int64_t ld_out,
                              void* stream) {
  using namespace gd;
  GD_REQUIRE(n_sub >= 0 && n_sub < (1ll << 31) && m >= 32 && m < (1ll << 31) && k >= 1 && k <= m, GD_E_DIM,
             "gd_subset_draw: n_sub=%lld k=%lld m=%lld out of range (1 <= k <= m, 32 <= m < 2^31)", (long long)n_sub, (long long)k,
             (long long)m);
  if (n_sub == 0) return GD_OK;
  GD_REQUIRE(out, GD_E_NULL, "gd_subset_draw: null pointer");
  GD_REQUIRE(ld_out >= k, GD_E_DIM, "gd_subset_draw: ld_out=%lld below k=%lld", (long long)ld_out, (long long)k);
  const unsigned rows = (unsigned)(n_sub < 65535 ? n_sub : 65535);
  hipLaunchKernelGGL(subset_draw_kernel, dim3((unsigned)((k + kRankBlock - 1) / kRankBlock), rows), dim3(kRankBlock), 0, (hipStream_t)stream,
                     seed, draw, draw_half_bits(m), n_sub, (int32_t)k, (int32_t)m, out, ld_out);
  return launched("subset_draw");
}
