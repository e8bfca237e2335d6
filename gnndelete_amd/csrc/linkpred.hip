// The two pieces the fused backbone step (gnndelete_amd/backbone.py: Trainer.train_fullbatch, framework/trainer/base.py:75-142,
// and RetrainTrainer.train_fullbatch, retrain.py:57-131, without autograd) was missing:
//
//   gd_edge_bce_f32   F.binary_cross_entropy_with_logits over the decoded edges [pos | neg] (labels 1 | 0), value and logit
//                     gradients, the gradients also gathered into incidence order for gd_edge_dot_bwd_f32;
//   gd_col_sum_f32    out[j] = sum_r row_w[r] * [gate[r, j] > 0] * x[r, j]: the bias gradients (dy.sum(0)), the gated form (which
//                     can also store the gated matrix: the ReLU backward and its bias gradient in one pass) and GATConv's
//                     attention-vector gradients;
//   gd_row_nll_f32    F.nll_loss(F.log_softmax(z[:, :d_valid], 1)[rows], y[rows]) over a list of rows, value and logit gradients:
//                     the loss stage of the fused node-classification step (NodeClassificationTrainer.train, base.py:694-752).
//
// All are streams.  Everything that is summed is summed in a fixed order (per-block partials, then one pass in block order):
// no atomics, the same bits on every call.
#include "common.h"

namespace gd {

constexpr int kBceMaxBlocks = 2048;      // partials the finishing thread adds; blocks walk the edges grid-strided beyond that
constexpr int kColSumMaxBlocks = 512;
constexpr int kNllMaxBlocks = 1024;      // as kBceMaxBlocks, for the listed rows of gd_row_nll_f32

// One lane group (LPR lanes) per decoded edge k < M = n_pos + n_neg, edges taken grid-strided: l_k = <z[a_k], z[b_k]>, an
// endpoint outside [0, n) makes it 0 (nothing outside z is read).  Stable forms with e = exp(-|l|):
//     term = max(l, 0) - l y + log1p(e);    sigmoid(l) - y = y ? -sigmoid(-l) : sigmoid(l)   (no 1 - 1 cancellation)
template <int LPR>
__global__ __launch_bounds__(256) void edge_bce_kernel(const float* __restrict__ z, int64_t ld_z, int64_t n, int32_t d4,
                                                       const int64_t* __restrict__ pos, int64_t ld_pos, int64_t n_pos,
                                                       const int64_t* __restrict__ neg, int64_t ld_neg, int64_t m_all,
                                                       float scale, float* __restrict__ w, float* __restrict__ partials) {
  constexpr int G = kWave / LPR;
  __shared__ float red[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int g = lane / LPR, li = lane % LPR;
  const int64_t per_pass = (int64_t)gridDim.x * 4 * G;
  float sum = 0.f;
  // (every lane of a wave makes the same number of trips: the cross-lane sums below are convergent)
  for (int64_t base = ((int64_t)blockIdx.x * 4 + wave) * G; base < m_all; base += per_pass) {
    const int64_t k = base + g;
    float l = 0.f;
    if (k < m_all) {
      const bool is_pos = k < n_pos;
      const int64_t a = is_pos ? pos[k] : neg[k - n_pos];
      const int64_t b = is_pos ? pos[ld_pos + k] : neg[ld_neg + (k - n_pos)];
      if (a >= 0 && a < n && b >= 0 && b < n) {
        const float4* x = reinterpret_cast<const float4*>(z + a * ld_z);
        const float4* y = reinterpret_cast<const float4*>(z + b * ld_z);
        for (int vec = li; vec < d4; vec += LPR) {
          const float4 xv = x[vec], yv = y[vec];
          l = fmaf(xv.x, yv.x, l); l = fmaf(xv.y, yv.y, l); l = fmaf(xv.z, yv.z, l); l = fmaf(xv.w, yv.w, l);
        }
      }
    }
#pragma unroll
    for (int off = 1; off < LPR; off <<= 1) l += __shfl_xor(l, off);
    if (k < m_all && li == 0) {
      const bool is_pos = k < n_pos;
      const float e = expf(-fabsf(l));
      const float big = 1.f / (1.f + e), small = e / (1.f + e);      // sigmoid(|l|), sigmoid(-|l|)
      sum += fmaxf(l, 0.f) - (is_pos ? l : 0.f) + log1pf(e);
      w[k] = is_pos ? -scale * (l >= 0.f ? small : big) : scale * (l >= 0.f ? big : small);
    }
  }
  sum = wave_sum(sum);
  if (lane == 0) red[wave] = sum;
  __syncthreads();
  if (threadIdx.x == 0) partials[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// loss = (1/M) * partials added in block order by one thread; every thread of the grid gathers
// w_inc[k] = w[src_edge[k]] for the incidences k < inc_ptr[n_nodes] (when asked to).
__global__ __launch_bounds__(256) void edge_bce_finish_kernel(const float* __restrict__ partials, int32_t n_part, float inv_m,
                                                              float* __restrict__ loss, const float* __restrict__ w, int64_t n_w,
                                                              const int32_t* __restrict__ src_edge,
                                                              const int64_t* __restrict__ inc_ptr, int64_t n_nodes,
                                                              float* __restrict__ w_inc) {
  if (src_edge) {
    int64_t total = inc_ptr[n_nodes];
    if (total > 2 * n_w) total = 2 * n_w;           // (two incidences per decoded edge: the size of w_inc)
    if (total < 0) total = 0;
    for (int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x; k < total; k += (int64_t)gridDim.x * 256) {
      const int32_t e = src_edge[k];
      w_inc[k] = e >= 0 && e < n_w ? w[e] : 0.f;
    }
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    float s = 0.f;
    for (int32_t i = 0; i < n_part; ++i) s += partials[i];
    *loss = s * inv_m;
  }
}

// Block b owns the rows [b * chunk, (b + 1) * chunk).  Thread t = slot * d4 + c reads the float4 column c of the rows
// slot, slot + n_slots, ... of the range (consecutive threads: consecutive 16 bytes of one row), then the slots of a column
// are added in slot order through LDS and the block's partial row is written.  gated (may be x itself: every element is read
// and then written by the same thread) receives the gated values.
__global__ __launch_bounds__(256) void col_sum_kernel(const float* x, int64_t ld, int64_t n_rows, int32_t d4,
                                                      const float* __restrict__ row_w, const float* __restrict__ gate,
                                                      float* gated, int64_t chunk, float* __restrict__ partials) {
  __shared__ float4 acc_s[256];
  const int n_slots = 256 / d4;
  const int slot = threadIdx.x / d4, c = threadIdx.x % d4;
  const int64_t lo = (int64_t)blockIdx.x * chunk;
  const int64_t hi = lo + chunk < n_rows ? lo + chunk : n_rows;
  float4 acc = f4_zero();
  if (slot < n_slots) {
    for (int64_t r = lo + slot; r < hi; r += n_slots) {
      float4 v = reinterpret_cast<const float4*>(x + r * ld)[c];
      if (gate) {
        const float4 gv = reinterpret_cast<const float4*>(gate + r * ld)[c];
        v.x = gv.x > 0.f ? v.x : 0.f; v.y = gv.y > 0.f ? v.y : 0.f; v.z = gv.z > 0.f ? v.z : 0.f; v.w = gv.w > 0.f ? v.w : 0.f;
        if (gated) reinterpret_cast<float4*>(gated + r * ld)[c] = v;
      }
      acc = f4_fma(row_w ? row_w[r] : 1.f, v, acc);
    }
  }
  acc_s[threadIdx.x] = acc;
  __syncthreads();
  if (threadIdx.x < d4) {
    float4 s = acc_s[threadIdx.x];
    for (int k = 1; k < n_slots; ++k) s = f4_add(s, acc_s[k * d4 + threadIdx.x]);
    reinterpret_cast<float4*>(partials + (int64_t)blockIdx.x * 4 * d4)[threadIdx.x] = s;
  }
}

// out[j] = the n_part partial rows added in block order (n_part = 0: zeros)
__global__ __launch_bounds__(256) void col_sum_finish_kernel(const float* __restrict__ partials, int32_t n_part, int32_t d,
                                                             float* __restrict__ out) {
  for (int j = threadIdx.x; j < d; j += 256) {
    float s = 0.f;
    for (int32_t b = 0; b < n_part; ++b) s += partials[(int64_t)b * d + j];
    out[j] = s;
  }
}

template <int LPR>
__device__ __forceinline__ float group_max(float v) {
#pragma unroll
  for (int off = 1; off < LPR; off <<= 1) v = fmaxf(v, __shfl_xor(v, off));
  return v;
}

// One lane group (LPR lanes, a float4 per lane) per listed row i < n_sel, rows taken grid-strided: u = row_idx[i], label y[u].
//     term = logsumexp(z[u, :d_valid]) - z[u, y[u]];    dz[u, j] = scale (softmax(z[u, :d_valid])_j - [j == y[u]]),  0 for j >= d_valid
// with the row maximum subtracted, in forms that keep a confident row's tiny term and gradient (no lse - z_y, no 1 - 1).  A label outside [0, d_valid) gives term = 0 and a zero dz row; a row id outside [0, n_rows) is
// skipped (nothing outside z / dz is touched).  The trip count is wave-uniform and a tail group works on a clamped row it does not
// write, so every lane of a wave executes every cross-lane step.
template <int LPR>
__global__ __launch_bounds__(256) void row_nll_kernel(const float* __restrict__ z, int64_t ld_z, int64_t n_rows, int32_t d4,
                                                      int32_t d_valid, const int32_t* __restrict__ row_idx, int64_t n_sel,
                                                      const int64_t* __restrict__ y, float scale, float* __restrict__ dz,
                                                      int64_t ld_dz, float* __restrict__ partials) {
  constexpr int G = kWave / LPR;
  __shared__ float red[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int g = lane / LPR, li = lane % LPR;
  const int64_t per_pass = (int64_t)gridDim.x * 4 * G;
  float sum = 0.f;
  for (int64_t base = ((int64_t)blockIdx.x * 4 + wave) * G; base < n_sel; base += per_pass) {
    const int64_t i = base + g;
    const bool mine = i < n_sel;
    const int64_t u = row_idx[mine ? i : n_sel - 1];
    const bool ok = u >= 0 && u < n_rows;
    const bool in = ok && li < d4;
    const int64_t label = ok ? y[u] : -1;
    const bool labelled = label >= 0 && label < d_valid;
    const float4 zv = in ? reinterpret_cast<const float4*>(z + u * ld_z)[li] : f4_zero();
    const float zz[4] = {zv.x, zv.y, zv.z, zv.w};
    bool valid[4];
    float m = -INFINITY;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      valid[k] = in && li * 4 + k < d_valid;
      m = fmaxf(m, valid[k] ? zz[k] : -INFINITY);
    }
    m = group_max<LPR>(m);
    if (!ok) m = 0.f;
    // rest = the sum without the label's term, ey = the label's term, zy = its logit (one non-zero lane entry each: exact sums)
    float e[4], rest = 0.f, ey = 0.f, zy = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      e[k] = valid[k] ? expf(zz[k] - m) : 0.f;
      const bool at = valid[k] && li * 4 + k == label;
      rest += at ? 0.f : e[k];
      ey += at ? e[k] : 0.f;
      zy += at ? zz[k] : 0.f;
    }
    rest = lanes_sum<LPR>(rest);
    ey = lanes_sum<LPR>(ey);
    zy = lanes_sum<LPR>(zy);
    float se = rest + ey;
    if (!ok) se = 1.f;
    // -log softmax_y = log(1 + rest / ey): as it stands while ey has not left the normal range (a confident row has a term far
    // below 1 ulp of its logits), m - zy + log(se) beyond that
    if (mine && labelled && li == 0) sum += (m - zy < 10.f) ? log1pf(rest / ey) : (m - zy) + logf(se);
    if (mine && in) {
      const float r = labelled ? scale / se : 0.f;
      float gr[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        gr[k] = r * e[k];
        if (labelled && li * 4 + k == label) gr[k] = -r * rest;       // softmax_y - 1 = -rest / se, without the 1 - 1
      }
      reinterpret_cast<float4*>(dz + u * ld_dz)[li] = make_float4(gr[0], gr[1], gr[2], gr[3]);
    }
  }
  sum = wave_sum(sum);
  if (lane == 0) red[wave] = sum;
  __syncthreads();
  if (threadIdx.x == 0) partials[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// loss = (1/n_sel) * the partials added in block order by one thread (in fp64: up to 1,024 partials of like sign)
__global__ void row_nll_finish_kernel(const float* __restrict__ partials, int32_t n_part, double inv_n, float* __restrict__ loss) {
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    double s = 0.0;
    for (int32_t i = 0; i < n_part; ++i) s += (double)partials[i];
    *loss = (float)(s * inv_n);
  }
}

static inline int nll_blocks(int64_t n_sel, int lpr) {
  const int64_t per_block = 4 * (kWave / lpr);
  const int64_t nb = (n_sel + per_block - 1) / per_block;
  return (int)(nb > kNllMaxBlocks ? kNllMaxBlocks : nb);
}

static inline int bce_blocks(int64_t m_all, int lpr) {
  const int64_t per_block = 4 * (kWave / lpr);
  const int64_t nb = (m_all + per_block - 1) / per_block;
  return (int)(nb > kBceMaxBlocks ? kBceMaxBlocks : nb);
}

// rows per block: at least four trips of the block's row slots, at most kColSumMaxBlocks blocks
static inline int64_t col_sum_chunk(int64_t n_rows, int d4) {
  const int64_t least = 4 * (256 / d4);
  int64_t chunk = (n_rows + kColSumMaxBlocks - 1) / kColSumMaxBlocks;
  if (chunk < least) chunk = least;
  return chunk;
}
static inline int col_sum_blocks(int64_t n_rows, int d4) {
  const int64_t chunk = col_sum_chunk(n_rows, d4);
  return (int)((n_rows + chunk - 1) / chunk);
}

}  // namespace gd

extern "C" int64_t gd_edge_bce_workspace(int64_t m_all, int32_t d) {
  using namespace gd;
  if (m_all <= 0 || d <= 0 || d % 4) return 1;
  return bce_blocks(m_all, lanes_per_row(d / 4));
}

extern "C" int gd_edge_bce_f32(const float* z, int64_t ld_z, int64_t n_nodes, int32_t d, const int64_t* pos, int64_t ld_pos,
                               int64_t n_pos, const int64_t* neg, int64_t ld_neg, int64_t n_neg, float coef, float* w,
                               float* loss, const int32_t* src_edge, const int64_t* inc_ptr, float* w_inc, float* workspace,
                               void* stream) {
  using namespace gd;
  GD_REQUIRE(n_pos >= 0 && n_neg >= 0 && n_pos < (1ll << 30) && n_neg < (1ll << 30) && n_pos + n_neg >= 1, GD_E_DIM,
             "gd_edge_bce_f32: n_pos=%lld n_neg=%lld (the mean over no edges is NaN upstream)", (long long)n_pos, (long long)n_neg);
  GD_REQUIRE(z && w && loss && workspace && (pos || n_pos == 0) && (neg || n_neg == 0), GD_E_NULL, "gd_edge_bce_f32: null pointer");
  GD_REQUIRE((src_edge == nullptr) == (inc_ptr == nullptr) && (src_edge == nullptr) == (w_inc == nullptr), GD_E_NULL,
             "gd_edge_bce_f32: src_edge, inc_ptr and w_inc go together");
  GD_REQUIRE(n_nodes >= 1 && d > 0 && d % 4 == 0 && d <= 4096 && ld_z >= d && ld_z % 4 == 0 && ld_pos >= n_pos && ld_neg >= n_neg,
             GD_E_DIM, "gd_edge_bce_f32: d=%d must be a multiple of 4 with 16-byte row pitches (ld_z=%lld)", d, (long long)ld_z);
  GD_REQUIRE(aligned16(z), GD_E_ALIGN, "gd_edge_bce_f32: unaligned z");
  hipStream_t s = (hipStream_t)stream;
  const int64_t m_all = n_pos + n_neg;
  const int d4 = d / 4;
  const int lpr = lanes_per_row(d4);
  const int nb = bce_blocks(m_all, lpr);
  const float scale = coef / (float)m_all;
#define GD_BCE_CASE(LPR) \
  hipLaunchKernelGGL((edge_bce_kernel<LPR>), dim3(nb), dim3(256), 0, s, z, ld_z, n_nodes, d4, pos, ld_pos, n_pos, neg, ld_neg, m_all, scale, w, workspace)
  switch (lpr) {
    case 1: GD_BCE_CASE(1); break;
    case 2: GD_BCE_CASE(2); break;
    case 4: GD_BCE_CASE(4); break;
    case 8: GD_BCE_CASE(8); break;
    case 16: GD_BCE_CASE(16); break;
    case 32: GD_BCE_CASE(32); break;
    default: GD_BCE_CASE(64); break;
  }
#undef GD_BCE_CASE
  int rc = launched("edge_bce");
  if (rc) return rc;
  const int64_t fb = src_edge ? (2 * m_all + 255) / 256 : 1;
  hipLaunchKernelGGL(edge_bce_finish_kernel, dim3((unsigned)(fb > 1024 ? 1024 : fb)), dim3(256), 0, s, workspace, nb,
                     1.0f / (float)m_all, loss, w, m_all, src_edge, inc_ptr, n_nodes, w_inc);
  return launched("edge_bce_finish");
}

extern "C" int64_t gd_col_sum_workspace(int64_t n_rows, int32_t d) {
  using namespace gd;
  if (n_rows <= 0 || d <= 0 || d % 4 || d > 1024) return 1;
  return (int64_t)col_sum_blocks(n_rows, d / 4) * d;
}

extern "C" int gd_col_sum_f32(const float* x, int64_t ld, int64_t n_rows, int32_t d, const float* row_w, const float* gate,
                              float* gated, float* out, float* workspace, void* stream) {
  using namespace gd;
  GD_REQUIRE(n_rows >= 0 && n_rows < (1ll << 40) && d > 0 && d % 4 == 0 && d <= 1024 && ld >= d && ld % 4 == 0, GD_E_DIM,
             "gd_col_sum_f32: d=%d must be a multiple of 4 up to 1024 with a 16-byte row pitch (ld=%lld)", d, (long long)ld);
  GD_REQUIRE(out && workspace && (x || n_rows == 0), GD_E_NULL, "gd_col_sum_f32: null pointer");
  GD_REQUIRE(gate || !gated, GD_E_NULL, "gd_col_sum_f32: gated without a gate");
  GD_REQUIRE(aligned16(x) && aligned16(gate) && aligned16(gated) && aligned16(workspace), GD_E_ALIGN, "gd_col_sum_f32: unaligned matrix");
  hipStream_t s = (hipStream_t)stream;
  const int d4 = d / 4;
  const int nb = n_rows ? col_sum_blocks(n_rows, d4) : 0;
  if (nb) {
    hipLaunchKernelGGL(col_sum_kernel, dim3(nb), dim3(256), 0, s, x, ld, n_rows, d4, row_w, gate, gated, col_sum_chunk(n_rows, d4), workspace);
    int rc = launched("col_sum");
    if (rc) return rc;
  }
  hipLaunchKernelGGL(col_sum_finish_kernel, dim3(1), dim3(256), 0, s, workspace, nb, d, out);
  return launched("col_sum_finish");
}

extern "C" int64_t gd_row_nll_workspace(int64_t n_sel, int32_t d) {
  using namespace gd;
  if (n_sel <= 0 || d < 4 || d % 4 || d > 256) return 1;
  return nll_blocks(n_sel, lanes_per_row(d / 4));
}

extern "C" int gd_row_nll_f32(const float* z, int64_t ld_z, int64_t n_rows, int32_t d, int32_t d_valid, const int32_t* row_idx,
                              int64_t n_sel, const int64_t* y, float coef, float* dz, int64_t ld_dz, float* loss, float* workspace,
                              void* stream) {
  using namespace gd;
  GD_REQUIRE(n_sel >= 1 && n_sel < (1ll << 31), GD_E_DIM, "gd_row_nll_f32: n_sel=%lld (the mean over no rows is NaN upstream)",
             (long long)n_sel);
  GD_REQUIRE(d >= 4 && d <= 256 && d % 4 == 0, GD_E_DIM, "gd_row_nll_f32: d=%d must be a multiple of 4 in [4, 256]", d);
  GD_REQUIRE(d_valid >= 1 && d_valid <= d, GD_E_DIM, "gd_row_nll_f32: d_valid=%d must lie in [1, d=%d]", d_valid, d);
  GD_REQUIRE(n_rows >= 1 && n_rows < (1ll << 31) && ld_z >= d && ld_z % 4 == 0 && ld_dz >= d && ld_dz % 4 == 0, GD_E_DIM,
             "gd_row_nll_f32: n_rows=%lld, row pitches %lld / %lld must be multiples of 4, at least d=%d", (long long)n_rows,
             (long long)ld_z, (long long)ld_dz, d);
  GD_REQUIRE(z && row_idx && y && dz && loss && workspace, GD_E_NULL, "gd_row_nll_f32: null pointer");
  GD_REQUIRE(aligned16(z) && aligned16(dz), GD_E_ALIGN, "gd_row_nll_f32: unaligned matrix");
  hipStream_t s = (hipStream_t)stream;
  const int d4 = d / 4;
  const int lpr = lanes_per_row(d4);
  const int nb = nll_blocks(n_sel, lpr);
  const float scale = coef / (float)n_sel;
#define GD_NLL_CASE(LPR) \
  hipLaunchKernelGGL((row_nll_kernel<LPR>), dim3(nb), dim3(256), 0, s, z, ld_z, n_rows, d4, d_valid, row_idx, n_sel, y, scale, dz, ld_dz, workspace)
  switch (lpr) {
    case 1: GD_NLL_CASE(1); break;
    case 2: GD_NLL_CASE(2); break;
    case 4: GD_NLL_CASE(4); break;
    case 8: GD_NLL_CASE(8); break;
    case 16: GD_NLL_CASE(16); break;
    case 32: GD_NLL_CASE(32); break;
    default: GD_NLL_CASE(64); break;
  }
#undef GD_NLL_CASE
  int rc = launched("row_nll");
  if (rc) return rc;
  hipLaunchKernelGGL(row_nll_finish_kernel, dim3(1), dim3(64), 0, s, workspace, nb, 1.0 / (double)n_sel, loss);
  return launched("row_nll_finish");
}
