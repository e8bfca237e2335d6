// The per-validation scoring of the prepared validation pass (gnndelete_amd/evalpass.py; Trainer.eval and
// NodeClassificationTrainer.eval under --fused_validation, framework/trainer/base.py:229-300 and :754-790 upstream):
//
//   gd_eval_edge_scores_f32   sigmoid(<z[a], z[b]>) of ONE decoded edge list [stage pos | stage neg | Df | Dr], the stage's
//                             BCE-with-logits-on-sigmoid-outputs loss, and the mean / population std of the Df scores;
//   gd_row_nll_eval_f32       mean NLL of log_softmax over the listed rows and the number of rows whose arg-max is the label;
//   gd_eval_triple_scores_f32 the knowledge-graph form (KGTrainer.eval, base.py:495-567): DistMult logits of ONE decoded triple
//                             list, RAW for the stage (with its BCE-with-logits loss), sigmoid for Df / Dr, Df mean / std.
//
// What today's path does with three edge_dot launches, three sigmoids, a cat, a label tensor, a torch loss and numpy on a
// host list (link prediction), or with two host copies and scikit-learn (node classification).  Both are streams followed by
// a one-block finishing launch.  Everything summed is summed in double in a fixed order (per-block partials, then block
// order; the Df scores over a fixed thread stride and a fixed LDS tree): no float atomics, no atomics at all, the same bits
// on every call.
#include "common.h"

#include <limits.h>

namespace gd {

constexpr int kEvalMaxBlocks = 1024;     // partials the finishing thread adds; blocks walk the items grid-strided beyond that
constexpr int kEvalFinishThreads = 1024;

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}
__device__ __forceinline__ int wave_sum_i32(int v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

// One lane group (LPR lanes, float4 loads) per decoded edge k < M, edges taken grid-strided, as edge_bce_kernel (linkpred.hip):
// l_k = <z[a_k], z[b_k]>; an endpoint outside [0, n) reads nothing, scores l = 0 and raises the block's flag.  With
// e = exp(-|l|): score = l >= 0 ? 1 / (1 + e) : e / (1 + e) - 1.0f exactly once e falls below half an ulp of 1, never NaN for
// finite z.  The stage's edges (k < n_stage, label 1 below n_pos) add, in double on the fp32 score s widened,
//     term = s (1 - y) + log1p(exp(-s))        binary_cross_entropy_with_logits applied to the SIGMOID OUTPUT, upstream's quirk
// (every lane of a wave makes the same number of trips: the cross-lane sums are convergent)
template <int LPR>
__global__ __launch_bounds__(256) void eval_edge_scores_kernel(const float* __restrict__ z, int64_t ld_z, int64_t n, int32_t d4,
                                                               const int64_t* __restrict__ src, const int64_t* __restrict__ dst,
                                                               int64_t n_pos, int64_t n_stage, int64_t m_all,
                                                               float* __restrict__ scores, double* __restrict__ partials,
                                                               int32_t* __restrict__ flags) {
  constexpr int G = kWave / LPR;
  __shared__ double red[4];
  __shared__ int bad_s[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int g = lane / LPR, li = lane % LPR;
  const int64_t per_pass = (int64_t)gridDim.x * 4 * G;
  double sum = 0.0;
  int bad = 0;
  for (int64_t base = ((int64_t)blockIdx.x * 4 + wave) * G; base < m_all; base += per_pass) {
    const int64_t k = base + g;
    float l = 0.f;
    if (k < m_all) {
      const int64_t a = src[k], b = dst[k];
      if (a >= 0 && a < n && b >= 0 && b < n) {
        const float4* x = reinterpret_cast<const float4*>(z + a * ld_z);
        const float4* y = reinterpret_cast<const float4*>(z + b * ld_z);
        for (int vec = li; vec < d4; vec += LPR) {
          const float4 xv = x[vec], yv = y[vec];
          l = fmaf(xv.x, yv.x, l); l = fmaf(xv.y, yv.y, l); l = fmaf(xv.z, yv.z, l); l = fmaf(xv.w, yv.w, l);
        }
      } else if (li == 0) {
        bad = 1;
      }
    }
#pragma unroll
    for (int off = 1; off < LPR; off <<= 1) l += __shfl_xor(l, off);
    if (k < m_all && li == 0) {
      const float e = expf(-fabsf(l));
      const float s = l >= 0.f ? 1.f / (1.f + e) : e / (1.f + e);
      scores[k] = s;
      if (k < n_stage) {
        const double sd = (double)s;
        sum += (k < n_pos ? 0.0 : sd) + log1p(exp(-sd));
      }
    }
  }
  sum = wave_sum_f64(sum);
  bad = wave_sum_i32(bad);
  if (lane == 0) {
    red[wave] = sum;
    bad_s[wave] = bad;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    partials[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
    flags[blockIdx.x] = (bad_s[0] | bad_s[1] | bad_s[2] | bad_s[3]) != 0;
  }
}

// The knowledge-graph form of eval_edge_scores_kernel (KGTrainer.eval, base.py:495-567 upstream): one lane group per decoded
// TRIPLE k < M, l_k = sum_j z[a_k, j] rel[t_k, j] z[b_k, j] with the product associated as edge_dot_kernel's DistMult decode
// does ((z_a * rel) rounded, then an fma chain over z_b in the same lane / vector order).  An endpoint outside [0, n) or a type
// outside [0, n_rel) reads nothing, scores l = 0 and raises the block's flag.  The stage's triples (k < n_stage) store the RAW
// logit - upstream ranks and scores the stage without a sigmoid - and add, in double on the fp32 l widened,
//     term = max(l, 0) - l y + log1p(exp(-|l|))        binary_cross_entropy_with_logits, finite at any finite l
// the Df / Dr triples store sigmoid(l) by eval_edge_scores_kernel's two branches.
template <int LPR>
__global__ __launch_bounds__(256) void eval_triple_scores_kernel(const float* __restrict__ z, int64_t ld_z, int64_t n, int32_t d4,
                                                                 const float* __restrict__ rel, int64_t ld_rel, int64_t n_rel,
                                                                 const int64_t* __restrict__ src, const int64_t* __restrict__ dst,
                                                                 const int64_t* __restrict__ etype, int64_t n_pos, int64_t n_stage,
                                                                 int64_t m_all, float* __restrict__ scores,
                                                                 double* __restrict__ partials, int32_t* __restrict__ flags) {
  constexpr int G = kWave / LPR;
  __shared__ double red[4];
  __shared__ int bad_s[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int g = lane / LPR, li = lane % LPR;
  const int64_t per_pass = (int64_t)gridDim.x * 4 * G;
  double sum = 0.0;
  int bad = 0;
  for (int64_t base = ((int64_t)blockIdx.x * 4 + wave) * G; base < m_all; base += per_pass) {
    const int64_t k = base + g;
    float l = 0.f;
    if (k < m_all) {
      const int64_t a = src[k], b = dst[k], t = etype[k];
      if (a >= 0 && a < n && b >= 0 && b < n && t >= 0 && t < n_rel) {
        const float4* x = reinterpret_cast<const float4*>(z + a * ld_z);
        const float4* y = reinterpret_cast<const float4*>(z + b * ld_z);
        const float4* r = reinterpret_cast<const float4*>(rel + t * ld_rel);
        for (int vec = li; vec < d4; vec += LPR) {
          float4 xv = x[vec];
          const float4 yv = y[vec], rv = r[vec];
          xv.x *= rv.x; xv.y *= rv.y; xv.z *= rv.z; xv.w *= rv.w;
          l = fmaf(xv.x, yv.x, l); l = fmaf(xv.y, yv.y, l); l = fmaf(xv.z, yv.z, l); l = fmaf(xv.w, yv.w, l);
        }
      } else if (li == 0) {
        bad = 1;
      }
    }
#pragma unroll
    for (int off = 1; off < LPR; off <<= 1) l += __shfl_xor(l, off);
    if (k < m_all && li == 0) {
      if (k < n_stage) {
        scores[k] = l;
        const double ld = (double)l;
        sum += (ld > 0.0 ? ld : 0.0) - (k < n_pos ? ld : 0.0) + log1p(exp(-fabs(ld)));
      } else {
        const float e = expf(-fabsf(l));
        scores[k] = l >= 0.f ? 1.f / (1.f + e) : e / (1.f + e);
      }
    }
  }
  sum = wave_sum_f64(sum);
  bad = wave_sum_i32(bad);
  if (lane == 0) {
    red[wave] = sum;
    bad_s[wave] = bad;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    partials[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
    flags[blockIdx.x] = (bad_s[0] | bad_s[1] | bad_s[2] | bad_s[3]) != 0;
  }
}

// a[0] <- a[0] + ... + a[kEvalFinishThreads - 1] by a fixed halving tree; returns it in every thread
__device__ __forceinline__ double block_tree_sum(double* a, double v) {
  __syncthreads();                                   // (the previous use of a[] has been read)
  a[threadIdx.x] = v;
  __syncthreads();
  for (int s = kEvalFinishThreads / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) a[threadIdx.x] += a[threadIdx.x + s];
    __syncthreads();
  }
  return a[0];
}

// One block.  stats[0] = (partials added in block order) / n_stage; stats[1], stats[2] = mean and population standard deviation
// of df[0 .. n_df) in double, two passes (mean, then squared deviations: a one-pass sum / sumsq cancels when unlearning has
// driven the Df scores together), thread t taking the elements t, t + 1024, ... in order and the threads added by a fixed
// tree; n_df = 0 gives NaN for both (np.nan upstream).  status = 1 when a block met an endpoint outside [0, n), else 0.
__global__ __launch_bounds__(kEvalFinishThreads) void eval_edge_scores_finish_kernel(const double* __restrict__ partials,
                                                                                     const int32_t* __restrict__ flags, int32_t n_part,
                                                                                     int64_t n_stage, const float* __restrict__ df,
                                                                                     int64_t n_df, double* __restrict__ stats,
                                                                                     int32_t* __restrict__ status) {
  __shared__ double acc[kEvalFinishThreads];
  const int t = threadIdx.x;
  double s = 0.0;
  for (int64_t i = t; i < n_df; i += kEvalFinishThreads) s += (double)df[i];
  const double mean = block_tree_sum(acc, s) / (double)n_df;          // 0 / 0 = NaN for an empty Df
  double q = 0.0;
  for (int64_t i = t; i < n_df; i += kEvalFinishThreads) {
    const double dev = (double)df[i] - mean;
    q = fma(dev, dev, q);
  }
  const double var = block_tree_sum(acc, q) / (double)n_df;
  int any = 0;
  for (int32_t i = t; i < n_part; i += kEvalFinishThreads) any |= flags[i];
  any = __syncthreads_or(any);
  if (t == 0) {
    double total = 0.0;
    for (int32_t i = 0; i < n_part; ++i) total += partials[i];
    stats[0] = total / (double)n_stage;                               // (no stage edges: NaN, the mean over nothing)
    stats[1] = mean;
    stats[2] = sqrt(var);
    *status = any ? 1 : 0;
  }
}

// One lane group (LPR lanes, up to four classes j = li, li + LPR, ... per lane, scalar loads: no alignment beyond the element)
// per listed row i < n_sel, rows taken grid-strided: u = row_idx[i], label y[u].  The arg-max is the LOWEST index among equal
// maxima (torch.argmax's / numpy's rule on a row without NaN); the term, in double with the row maximum subtracted,
//     term = logsumexp(z[u, :d_valid]) - z[u, y[u]] = log1p(sum_{j != y} e_j / e_y)   (m - z_y + log(sum_j e_j) once e_y is tiny)
// A row id outside [0, n_rows) is skipped; a label outside [0, d_valid) counts as wrong with term 0, as row_nll_kernel does.
// The trip count is wave-uniform and a tail group works on a clamped row it does not count.
template <int LPR>
__global__ __launch_bounds__(256) void row_nll_eval_kernel(const float* __restrict__ z, int64_t ld, int64_t n_rows, int32_t d_valid,
                                                           const int32_t* __restrict__ row_idx, int64_t n_sel,
                                                           const int64_t* __restrict__ y, double* __restrict__ partials,
                                                           long long* __restrict__ counts) {
  constexpr int G = kWave / LPR;
  __shared__ double red[4];
  __shared__ int hit_s[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int g = lane / LPR, li = lane % LPR;
  const int64_t per_pass = (int64_t)gridDim.x * 4 * G;
  double sum = 0.0;
  int hits = 0;
  for (int64_t base = ((int64_t)blockIdx.x * 4 + wave) * G; base < n_sel; base += per_pass) {
    const int64_t i = base + g;
    const bool mine = i < n_sel;
    const int64_t u = row_idx[mine ? i : n_sel - 1];
    const bool ok = u >= 0 && u < n_rows;
    const int64_t label = ok ? y[u] : -1;
    const bool labelled = label >= 0 && label < d_valid;
    float zz[4];
    bool valid[4];
    float m = -INFINITY;
    int am = INT_MAX;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int j = li + k * LPR;
      valid[k] = ok && j < d_valid;
      zz[k] = valid[k] ? z[u * ld + j] : 0.f;
      if (valid[k] && (am == INT_MAX || zz[k] > m)) {      // (j ascends: a later equal value does not replace an earlier one)
        m = zz[k];
        am = j;
      }
    }
#pragma unroll
    for (int off = 1; off < LPR; off <<= 1) {
      const float m2 = __shfl_xor(m, off);
      const int a2 = __shfl_xor(am, off);
      if (a2 != INT_MAX && (am == INT_MAX || m2 > m || (m2 == m && a2 < am))) {
        m = m2;
        am = a2;
      }
    }
    // rest = the sum without the label's term, ey = the label's term, zy = its logit (one non-zero lane entry each)
    double rest = 0.0, ey = 0.0, zy = 0.0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const double e = valid[k] ? exp((double)zz[k] - (double)m) : 0.0;
      const bool at = valid[k] && li + k * LPR == label;
      rest += at ? 0.0 : e;
      ey += at ? e : 0.0;
      zy += at ? (double)zz[k] : 0.0;
    }
#pragma unroll
    for (int off = 1; off < LPR; off <<= 1) {
      rest += __shfl_xor(rest, off);
      ey += __shfl_xor(ey, off);
      zy += __shfl_xor(zy, off);
    }
    if (mine && labelled && li == 0) {
      const double gap = (double)m - zy;
      sum += gap < 10.0 ? log1p(rest / ey) : gap + log(rest + ey);
      hits += am == label;
    }
  }
  sum = wave_sum_f64(sum);
  hits = wave_sum_i32(hits);
  if (lane == 0) {
    red[wave] = sum;
    hit_s[wave] = hits;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    partials[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
    counts[blockIdx.x] = (long long)hit_s[0] + hit_s[1] + hit_s[2] + hit_s[3];
  }
}

// loss = (the partials added in block order) / n_sel (n_sel = 0: NaN); correct = the blocks' counts added as integers
__global__ void row_nll_eval_finish_kernel(const double* __restrict__ partials, const long long* __restrict__ counts, int32_t n_part,
                                           int64_t n_sel, double* __restrict__ loss, int64_t* __restrict__ correct) {
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    double s = 0.0;
    long long c = 0;
    for (int32_t i = 0; i < n_part; ++i) {
      s += partials[i];
      c += counts[i];
    }
    *loss = s / (double)n_sel;
    *correct = (int64_t)c;
  }
}

static inline int eval_blocks(int64_t items, int lpr) {
  const int64_t per_block = 4 * (kWave / lpr);
  const int64_t nb = (items + per_block - 1) / per_block;
  return (int)(nb > kEvalMaxBlocks ? kEvalMaxBlocks : nb);
}

// lanes of a row group of gd_row_nll_eval_f32: four classes per lane
static inline int nll_eval_lanes(int d_valid) { return lanes_per_row((d_valid + 3) / 4); }

}  // namespace gd

extern "C" int64_t gd_eval_edge_scores_workspace(int64_t m_all, int32_t d) {
  using namespace gd;
  if (m_all <= 0 || d <= 0 || d % 4 || d > 256) return 2;
  return 2 * (int64_t)eval_blocks(m_all, lanes_per_row(d / 4));
}

extern "C" int gd_eval_edge_scores_f32(const float* z, int64_t ld_z, int64_t n_nodes, int32_t d, const int64_t* src,
                                       const int64_t* dst, int64_t n_pos, int64_t n_neg, int64_t n_df, int64_t n_dr, float* scores,
                                       double* stats, int32_t* status, double* workspace, void* stream) {
  using namespace gd;
  GD_REQUIRE(n_pos >= 0 && n_neg >= 0 && n_df >= 0 && n_dr >= 0 && n_pos < (1ll << 31) && n_neg < (1ll << 31) && n_df < (1ll << 31) &&
                 n_dr < (1ll << 31) && n_pos + n_neg + n_df + n_dr >= 1 && n_pos + n_neg + n_df + n_dr < (1ll << 31),
             GD_E_DIM, "gd_eval_edge_scores_f32: segments %lld / %lld / %lld / %lld (non-negative, 1 <= their sum < 2^31)",
             (long long)n_pos, (long long)n_neg, (long long)n_df, (long long)n_dr);
  GD_REQUIRE(z && src && dst && scores && stats && status && workspace, GD_E_NULL, "gd_eval_edge_scores_f32: null pointer");
  GD_REQUIRE(n_nodes >= 1 && d > 0 && d % 4 == 0 && d <= 256 && ld_z >= d && ld_z % 4 == 0, GD_E_DIM,
             "gd_eval_edge_scores_f32: d=%d must be a multiple of 4 up to 256 with a 16-byte row pitch (ld_z=%lld)", d, (long long)ld_z);
  GD_REQUIRE(aligned16(z), GD_E_ALIGN, "gd_eval_edge_scores_f32: unaligned z");
  GD_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 7u) == 0 && (reinterpret_cast<uintptr_t>(stats) & 7u) == 0, GD_E_ALIGN,
             "gd_eval_edge_scores_f32: stats / workspace must be 8-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  const int64_t n_stage = n_pos + n_neg, m_all = n_stage + n_df + n_dr;
  const int d4 = d / 4;
  const int lpr = lanes_per_row(d4);
  const int nb = eval_blocks(m_all, lpr);
  int32_t* flags = reinterpret_cast<int32_t*>(workspace + nb);
#define GD_EVAL_CASE(LPR) \
  hipLaunchKernelGGL((eval_edge_scores_kernel<LPR>), dim3(nb), dim3(256), 0, s, z, ld_z, n_nodes, d4, src, dst, n_pos, n_stage, m_all, scores, workspace, flags)
  switch (lpr) {
    case 1: GD_EVAL_CASE(1); break;
    case 2: GD_EVAL_CASE(2); break;
    case 4: GD_EVAL_CASE(4); break;
    case 8: GD_EVAL_CASE(8); break;
    case 16: GD_EVAL_CASE(16); break;
    case 32: GD_EVAL_CASE(32); break;
    default: GD_EVAL_CASE(64); break;
  }
#undef GD_EVAL_CASE
  int rc = launched("eval_edge_scores");
  if (rc) return rc;
  hipLaunchKernelGGL(eval_edge_scores_finish_kernel, dim3(1), dim3(kEvalFinishThreads), 0, s, workspace, flags, nb, n_stage,
                     scores + n_stage, n_df, stats, status);
  return launched("eval_edge_scores_finish");
}

extern "C" int64_t gd_eval_triple_scores_workspace(int64_t m_all, int32_t d) { return gd_eval_edge_scores_workspace(m_all, d); }

extern "C" int gd_eval_triple_scores_f32(const float* z, int64_t ld_z, int64_t n_nodes, int32_t d, const float* rel, int64_t ld_rel,
                                         int64_t n_rel, const int64_t* src, const int64_t* dst, const int64_t* etype, int64_t n_pos,
                                         int64_t n_neg, int64_t n_df, int64_t n_dr, float* scores, double* stats, int32_t* status,
                                         double* workspace, void* stream) {
  using namespace gd;
  GD_REQUIRE(n_pos >= 0 && n_neg >= 0 && n_df >= 0 && n_dr >= 0 && n_pos < (1ll << 31) && n_neg < (1ll << 31) && n_df < (1ll << 31) &&
                 n_dr < (1ll << 31) && n_pos + n_neg + n_df + n_dr >= 1 && n_pos + n_neg + n_df + n_dr < (1ll << 31),
             GD_E_DIM, "gd_eval_triple_scores_f32: segments %lld / %lld / %lld / %lld (non-negative, 1 <= their sum < 2^31)",
             (long long)n_pos, (long long)n_neg, (long long)n_df, (long long)n_dr);
  GD_REQUIRE(z && rel && src && dst && etype && scores && stats && status && workspace, GD_E_NULL,
             "gd_eval_triple_scores_f32: null pointer");
  GD_REQUIRE(n_nodes >= 1 && n_rel >= 1 && d > 0 && d % 4 == 0 && d <= 256 && ld_z >= d && ld_z % 4 == 0 && ld_rel >= d && ld_rel % 4 == 0,
             GD_E_DIM, "gd_eval_triple_scores_f32: d=%d must be a multiple of 4 up to 256 with 16-byte row pitches (ld_z=%lld, ld_rel=%lld)",
             d, (long long)ld_z, (long long)ld_rel);
  GD_REQUIRE(aligned16(z) && aligned16(rel), GD_E_ALIGN, "gd_eval_triple_scores_f32: unaligned z / rel");
  GD_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 7u) == 0 && (reinterpret_cast<uintptr_t>(stats) & 7u) == 0, GD_E_ALIGN,
             "gd_eval_triple_scores_f32: stats / workspace must be 8-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  const int64_t n_stage = n_pos + n_neg, m_all = n_stage + n_df + n_dr;
  const int d4 = d / 4;
  const int lpr = lanes_per_row(d4);
  const int nb = eval_blocks(m_all, lpr);
  int32_t* flags = reinterpret_cast<int32_t*>(workspace + nb);
#define GD_EVAL_CASE(LPR)                                                                                                             \
  hipLaunchKernelGGL((eval_triple_scores_kernel<LPR>), dim3(nb), dim3(256), 0, s, z, ld_z, n_nodes, d4, rel, ld_rel, n_rel, src, dst, \
                     etype, n_pos, n_stage, m_all, scores, workspace, flags)
  switch (lpr) {
    case 1: GD_EVAL_CASE(1); break;
    case 2: GD_EVAL_CASE(2); break;
    case 4: GD_EVAL_CASE(4); break;
    case 8: GD_EVAL_CASE(8); break;
    case 16: GD_EVAL_CASE(16); break;
    case 32: GD_EVAL_CASE(32); break;
    default: GD_EVAL_CASE(64); break;
  }
#undef GD_EVAL_CASE
  int rc = launched("eval_triple_scores");
  if (rc) return rc;
  hipLaunchKernelGGL(eval_edge_scores_finish_kernel, dim3(1), dim3(kEvalFinishThreads), 0, s, workspace, flags, nb, n_stage,
                     scores + n_stage, n_df, stats, status);
  return launched("eval_triple_scores_finish");
}

extern "C" int64_t gd_row_nll_eval_workspace(int64_t n_sel, int32_t d_valid) {
  using namespace gd;
  if (n_sel <= 0 || d_valid < 1 || d_valid > 256) return 2;
  return 2 * (int64_t)eval_blocks(n_sel, nll_eval_lanes(d_valid));
}

extern "C" int gd_row_nll_eval_f32(const float* z, int64_t ld, int64_t n_rows, int32_t d_valid, const int32_t* row_idx, int64_t n_sel,
                                   const int64_t* y, double* loss, int64_t* correct, double* workspace, void* stream) {
  using namespace gd;
  GD_REQUIRE(n_sel >= 0 && n_sel < (1ll << 31), GD_E_DIM, "gd_row_nll_eval_f32: n_sel=%lld (0 <= n_sel < 2^31)", (long long)n_sel);
  GD_REQUIRE(d_valid >= 1 && d_valid <= 256, GD_E_DIM, "gd_row_nll_eval_f32: d_valid=%d must lie in [1, 256]", d_valid);
  GD_REQUIRE(n_rows >= 1 && n_rows < (1ll << 31) && ld >= d_valid, GD_E_DIM,
             "gd_row_nll_eval_f32: n_rows=%lld, row pitch %lld must be at least d_valid=%d", (long long)n_rows, (long long)ld, d_valid);
  GD_REQUIRE(z && y && loss && correct && workspace && (row_idx || n_sel == 0), GD_E_NULL, "gd_row_nll_eval_f32: null pointer");
  GD_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 7u) == 0 && (reinterpret_cast<uintptr_t>(loss) & 7u) == 0 &&
                 (reinterpret_cast<uintptr_t>(correct) & 7u) == 0,
             GD_E_ALIGN, "gd_row_nll_eval_f32: loss / correct / workspace must be 8-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  const int lpr = nll_eval_lanes(d_valid);
  const int nb = n_sel ? eval_blocks(n_sel, lpr) : 0;
  long long* counts = reinterpret_cast<long long*>(workspace + nb);
  if (nb) {
#define GD_NLL_EVAL_CASE(LPR) \
  hipLaunchKernelGGL((row_nll_eval_kernel<LPR>), dim3(nb), dim3(256), 0, s, z, ld, n_rows, d_valid, row_idx, n_sel, y, workspace, counts)
    switch (lpr) {
      case 1: GD_NLL_EVAL_CASE(1); break;
      case 2: GD_NLL_EVAL_CASE(2); break;
      case 4: GD_NLL_EVAL_CASE(4); break;
      case 8: GD_NLL_EVAL_CASE(8); break;
      case 16: GD_NLL_EVAL_CASE(16); break;
      case 32: GD_NLL_EVAL_CASE(32); break;
      default: GD_NLL_EVAL_CASE(64); break;
    }
#undef GD_NLL_EVAL_CASE
    int rc = launched("row_nll_eval");
    if (rc) return rc;
  }
  hipLaunchKernelGGL(row_nll_eval_finish_kernel, dim3(1), dim3(64), 0, s, workspace, counts, nb, n_sel, loss, correct);
  return launched("row_nll_eval_finish");
}
