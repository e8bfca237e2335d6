// The step of the edge-probability trainer (GNNDeleteTrainer.train_fullbatch, framework/trainer/gnndelete.py:221-255)
// without autograd - the pieces the fused step (gnndelete_amd/edgeprob.py) was missing:
//
//   gd_edgeprob_dec_f32   loss_r = MSE(logit(Df edges), logit(negatives)) and the upstream gradient of every decoded edge,
//                         in the decoder's [pos | neg] order and (optionally) gathered into incidence order;
//   gd_edge_incidence     the node-major incidence list gd_edge_dot_bwd_f32 walks, in the order a stable sort of
//                         cat(e0, e1) gives (what ops._EdgeDot.backward builds with torch.sort + searchsorted);
//   gd_rows_add_f32       dz[nodes[i], :] += s * src[i, :] for sorted unique rows (the compact pair-term gradient);
//   gd_edgeprob_record_f32  the epoch's three losses into a device history ring;
//   gd_edgeprob_batch_loss_f32  the loss stage of a GraphSAINT batch of the mini-batch loop (:364-400): both terms over the
//                         decoded list [Df edges | negatives | the batch's S_Df edges with src < dst], their logit
//                         gradients, the incidence list and the gradients in incidence order.
//
// Everything that is summed is summed in a fixed order (per-block partials, then one thread in block order); the only
// atomics are integer counters whose final values do not depend on arrival order.
#include "common.h"

namespace gd {

// One lane group (LPR lanes) per Df edge k: a_k = <z[pos0_k], z[pos1_k]>, b_k = <z[neg0_k], z[neg1_k]>.
// An endpoint outside [0, n) makes its dot product 0 (nothing outside z is read).
template <int LPR>
__global__ __launch_bounds__(256) void edgeprob_dec_kernel(const float* __restrict__ z, int64_t ld_z, int64_t n, int32_t d4,
                                                           const int64_t* __restrict__ pos, int64_t ld_pos,
                                                           const int64_t* __restrict__ neg, int64_t ld_neg, int64_t m,
                                                           float scale, float* __restrict__ w,
                                                           float* __restrict__ partials) {
  constexpr int G = kWave / LPR;
  __shared__ float red[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int g = lane / LPR, li = lane % LPR;
  const int64_t k = ((int64_t)blockIdx.x * 4 + wave) * G + g;
  float a = 0.f, b = 0.f;
  if (k < m) {
    const int64_t p0 = pos[k], p1 = pos[ld_pos + k], q0 = neg[k], q1 = neg[ld_neg + k];
    if (p0 >= 0 && p0 < n && p1 >= 0 && p1 < n) {
      const float4* x = reinterpret_cast<const float4*>(z + p0 * ld_z);
      const float4* y = reinterpret_cast<const float4*>(z + p1 * ld_z);
      for (int vec = li; vec < d4; vec += LPR) {
        const float4 xv = x[vec], yv = y[vec];
        a = fmaf(xv.x, yv.x, a); a = fmaf(xv.y, yv.y, a); a = fmaf(xv.z, yv.z, a); a = fmaf(xv.w, yv.w, a);
      }
    }
    if (q0 >= 0 && q0 < n && q1 >= 0 && q1 < n) {
      const float4* x = reinterpret_cast<const float4*>(z + q0 * ld_z);
      const float4* y = reinterpret_cast<const float4*>(z + q1 * ld_z);
      for (int vec = li; vec < d4; vec += LPR) {
        const float4 xv = x[vec], yv = y[vec];
        b = fmaf(xv.x, yv.x, b); b = fmaf(xv.y, yv.y, b); b = fmaf(xv.z, yv.z, b); b = fmaf(xv.w, yv.w, b);
      }
    }
  }
#pragma unroll
  for (int off = 1; off < LPR; off <<= 1) { a += __shfl_xor(a, off); b += __shfl_xor(b, off); }
  float sq = 0.f;
  if (k < m && li == 0) {
    const float diff = a - b;
    const float wk = scale * diff;
    w[k] = wk;
    w[m + k] = -wk;
    sq = diff * diff;
  }
  sq = wave_sum(sq);
  if (lane == 0) red[wave] = sq;
  __syncthreads();
  if (threadIdx.x == 0) partials[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// loss_r = (1/m) * partials added in block order by one thread; every thread of the grid gathers
// w_inc[k] = w[src_edge[k]] for the incidences k < inc_ptr[n_nodes] (when asked to).
__global__ __launch_bounds__(256) void edgeprob_dec_finish_kernel(const float* __restrict__ partials, int32_t n_part, float inv_m,
                                                                  float* __restrict__ loss, const float* __restrict__ w,
                                                                  int64_t n_w, const int32_t* __restrict__ src_edge,
                                                                  const int64_t* __restrict__ inc_ptr, int64_t n_nodes,
                                                                  float* __restrict__ w_inc) {
  if (src_edge) {
    int64_t total = inc_ptr[n_nodes];
    if (total > 2 * n_w) total = 2 * n_w;           // (two incidences per decoded edge: the size of w_inc)
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

// ---- incidence list.  Entry p of cat(e0, e1) (p < M: endpoint e0[p] of edge p; p >= M: endpoint e1[p - M] of edge p - M)
// belongs to the list of its endpoint; inside a list the entries are in ascending p (a stable sort by endpoint).  An edge
// with an endpoint outside [0, n) has no entries.
__device__ __forceinline__ int64_t inc_key(const int64_t* __restrict__ e0, const int64_t* __restrict__ e1, int64_t m_edges,
                                           int64_t n, int64_t p) {
  const int64_t e = p < m_edges ? p : p - m_edges;
  const int64_t a = e0[e], b = e1[e];
  if (a < 0 || a >= n || b < 0 || b >= n) return -1;
  return p < m_edges ? a : b;
}

__global__ __launch_bounds__(256) void inc_count_kernel(const int64_t* __restrict__ e0, const int64_t* __restrict__ e1,
                                                        int64_t m_edges, int64_t n, int32_t* __restrict__ count) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= 2 * m_edges) return;
  const int64_t v = inc_key(e0, e1, m_edges, n, p);
  if (v >= 0) atomicAdd(&count[v], 1);
}

// exclusive scan of count[0..n) into inc_ptr[0..n] by one block (chunks of consecutive nodes per thread); count is zeroed
// again: the fill pass uses it as the per-node cursor
__global__ __launch_bounds__(1024) void inc_scan_kernel(int32_t* __restrict__ count, int64_t n, int64_t* __restrict__ inc_ptr) {
  __shared__ int64_t part[1024];
  const int t = threadIdx.x;
  const int64_t chunk = (n + 1023) / 1024;
  const int64_t lo = min(n, t * chunk), hi = min(n, lo + chunk);
  int64_t s = 0;
  for (int64_t v = lo; v < hi; ++v) s += count[v];
  part[t] = s;
  __syncthreads();
  for (int off = 1; off < 1024; off <<= 1) {
    const int64_t add = t >= off ? part[t - off] : 0;
    __syncthreads();
    part[t] += add;
    __syncthreads();
  }
  int64_t run = part[t] - s;
  for (int64_t v = lo; v < hi; ++v) {
    inc_ptr[v] = run;
    run += count[v];
    count[v] = 0;
  }
  if (t == 1023) inc_ptr[n] = part[1023];
}

__global__ __launch_bounds__(256) void inc_fill_kernel(const int64_t* __restrict__ e0, const int64_t* __restrict__ e1,
                                                       int64_t m_edges, int64_t n, const int64_t* __restrict__ inc_ptr,
                                                       int32_t* __restrict__ cursor, int32_t* __restrict__ slots) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= 2 * m_edges) return;
  const int64_t v = inc_key(e0, e1, m_edges, n, p);
  if (v >= 0) slots[inc_ptr[v] + atomicAdd(&cursor[v], 1)] = (int32_t)p;
}

// the place of entry p inside its list = the number of entries of that list that come before it in cat(e0, e1)
__global__ __launch_bounds__(256) void inc_rank_kernel(const int64_t* __restrict__ e0, const int64_t* __restrict__ e1,
                                                       int64_t m_edges, int64_t n, const int64_t* __restrict__ inc_ptr,
                                                       const int32_t* __restrict__ slots, int32_t* __restrict__ other,
                                                       int32_t* __restrict__ src_edge) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= 2 * m_edges) return;
  const int64_t v = inc_key(e0, e1, m_edges, n, p);
  if (v < 0) return;
  const int64_t lo = inc_ptr[v], hi = inc_ptr[v + 1];
  int64_t rank = 0;
  for (int64_t j = lo; j < hi; ++j) rank += slots[j] < (int32_t)p ? 1 : 0;
  const int64_t e = p < m_edges ? p : p - m_edges;
  other[lo + rank] = (int32_t)(p < m_edges ? e1[e] : e0[e]);
  src_edge[lo + rank] = (int32_t)e;
}

template <int LPR>
__global__ __launch_bounds__(256) void rows_add_kernel(float* __restrict__ dz, int64_t ld_dz, int64_t n_rows,
                                                       const int32_t* __restrict__ nodes, int32_t n_s,
                                                       const float* __restrict__ src, int64_t ld_src, float s, int32_t d4) {
  constexpr int G = kWave / LPR;
  const int lane = threadIdx.x & 63;
  const int g = lane / LPR, li = lane % LPR;
  const int64_t i = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * G + g;
  if (i >= n_s) return;
  const int64_t row = nodes[i];
  if (row < 0 || row >= n_rows) return;
  float4* out = reinterpret_cast<float4*>(dz + row * ld_dz);
  const float4* in = reinterpret_cast<const float4*>(src + i * ld_src);
  for (int vec = li; vec < d4; vec += LPR) {
    const float4 x = in[vec];
    float4 y = out[vec];
    y.x += s * x.x; y.y += s * x.y; y.z += s * x.z; y.w += s * x.w;
    out[vec] = y;
  }
}

__global__ void edgeprob_record_kernel(const float* __restrict__ loss_r, const float* __restrict__ loss_l, float coef_r,
                                       float coef_l, float* __restrict__ hist, int32_t capacity, int32_t* __restrict__ pos) {
#pragma clang fp contract(off)
  const float r = *loss_r, l = loss_l ? *loss_l : 0.f;
  const int32_t at = *pos % capacity;
  float* h = hist + 3 * (int64_t)at;
  h[0] = coef_r * r + coef_l * l;
  h[1] = l;
  h[2] = r;
  *pos = *pos + 1;
}

static inline int dec_blocks(int64_t m, int lpr) {
  const int64_t per_block = 4 * (kWave / lpr);
  return (int)((m + per_block - 1) / per_block);
}

// ---- the loss stage of a GraphSAINT batch (gd_edgeprob_batch_loss_f32).  Items t < k are the DEC pairs (Df edge t against
// negative t, both dots in z), items t >= k the candidates c = t - k (the same edge in z and in z_ori).
constexpr int kBatchLossMaxBlocks = 2048;

// this lane's share of <tab[i0], tab[i1]>; 0 when an endpoint is outside [0, rows) (nothing outside tab is read)
template <int LPR>
__device__ __forceinline__ float pair_dot_part(const float* __restrict__ tab, int64_t ld, int64_t rows, int64_t i0, int64_t i1,
                                               int32_t d4, int li) {
  float acc = 0.f;
  if (i0 >= 0 && i0 < rows && i1 >= 0 && i1 < rows) {
    const float4* x = reinterpret_cast<const float4*>(tab + i0 * ld);
    const float4* y = reinterpret_cast<const float4*>(tab + i1 * ld);
    for (int vec = li; vec < d4; vec += LPR) {
      const float4 xv = x[vec], yv = y[vec];
      acc = fmaf(xv.x, yv.x, acc); acc = fmaf(xv.y, yv.y, acc); acc = fmaf(xv.z, yv.z, acc); acc = fmaf(xv.w, yv.w, acc);
    }
  }
  return acc;
}

// One lane group per item, the grid walks the k + n_cand items in strides.  Writes the decoded list [pos | neg | candidates]
// ((-1, -1) for a candidate that does not count), the raw difference of every item (0 where nothing counts) and one
// (sum of squares DEC, sum of squares locality, counted candidates) partial per block.
template <int LPR>
__global__ __launch_bounds__(256) void edgeprob_batch_dots_kernel(
    const float* __restrict__ z, int64_t ld_z, int64_t n, const float* __restrict__ z_ori, int64_t ld_o, int64_t n_o, int32_t d4,
    const int64_t* __restrict__ pos, int64_t ld_pos, const int64_t* __restrict__ neg, int64_t ld_neg, int64_t k,
    const int64_t* __restrict__ cand_src, const int64_t* __restrict__ cand_dst, int64_t n_cand, int64_t* __restrict__ dec,
    int64_t ld_dec, float* __restrict__ raw, float* __restrict__ part_e, float* __restrict__ part_l,
    int32_t* __restrict__ part_n) {
  constexpr int G = kWave / LPR;
  __shared__ float red_e[4], red_l[4];
  __shared__ int32_t red_n[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int g = lane / LPR, li = lane % LPR;
  const int64_t total = k + n_cand, per_grid = (int64_t)gridDim.x * 4 * G;
  float sq_e = 0.f, sq_l = 0.f;
  int32_t counted = 0;
  for (int64_t base = (int64_t)blockIdx.x * 4 * G; base < total; base += per_grid) {
    const int64_t t = base + wave * G + g;
    int64_t s0 = -1, s1 = -1;
    float a = 0.f, b = 0.f;
    bool counts = false;
    if (t < k) {
      const int64_t p0 = pos[t], p1 = pos[ld_pos + t], q0 = neg[t], q1 = neg[ld_neg + t];
      a = pair_dot_part<LPR>(z, ld_z, n, p0, p1, d4, li);
      b = pair_dot_part<LPR>(z, ld_z, n, q0, q1, d4, li);
      if (li == 0) {
        dec[t] = p0; dec[ld_dec + t] = p1;
        dec[k + t] = q0; dec[ld_dec + k + t] = q1;
      }
    } else if (t < total) {
      const int64_t c0 = cand_src[t - k], c1 = cand_dst[t - k];
      counts = c0 < c1;
      if (counts) {
        s0 = c0; s1 = c1;
        a = pair_dot_part<LPR>(z, ld_z, n, c0, c1, d4, li);
        b = pair_dot_part<LPR>(z_ori, ld_o, n_o, c0, c1, d4, li);
      }
      if (li == 0) { dec[k + t] = s0; dec[ld_dec + k + t] = s1; }
    }
#pragma unroll
    for (int off = 1; off < LPR; off <<= 1) { a += __shfl_xor(a, off); b += __shfl_xor(b, off); }
    if (t < total && li == 0) {
      const float diff = a - b;               // (0 for a candidate that does not count)
      raw[t] = diff;
      if (t < k) sq_e = fmaf(diff, diff, sq_e);
      else if (counts) { sq_l = fmaf(diff, diff, sq_l); ++counted; }
    }
  }
  sq_e = wave_sum(sq_e);
  sq_l = wave_sum(sq_l);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) counted += __shfl_xor(counted, off);
  if (lane == 0) { red_e[wave] = sq_e; red_l[wave] = sq_l; red_n[wave] = counted; }
  __syncthreads();
  if (threadIdx.x == 0) {
    part_e[blockIdx.x] = (red_e[0] + red_e[1]) + (red_e[2] + red_e[3]);
    part_l[blockIdx.x] = (red_l[0] + red_l[1]) + (red_l[2] + red_l[3]);
    part_n[blockIdx.x] = (red_n[0] + red_n[1]) + (red_n[2] + red_n[3]);
  }
}

// Every block adds the integer partial counts (n_l; order cannot matter), scales the raw differences into w in decoded
// order and, when asked to, gathers w_inc[i] = w[src_edge[i]]; thread 0 of block 0 adds the float partials in block order.
// losses = (coef_e loss_e + coef_l loss_l, loss_e, loss_l); a mean over nothing is 0 / 0 = NaN, as F.mse_loss gives.
__global__ __launch_bounds__(256) void edgeprob_batch_finish_kernel(
    const float* __restrict__ part_e, const float* __restrict__ part_l, const int32_t* __restrict__ part_n, int32_t n_part,
    int64_t k, int64_t n_cand, float coef_e, float coef_l, const float* __restrict__ raw, float* __restrict__ w,
    float* __restrict__ losses, const int32_t* __restrict__ src_edge, const int64_t* __restrict__ inc_ptr, int64_t n_nodes,
    float* __restrict__ w_inc) {
#pragma clang fp contract(off)
  __shared__ int32_t red_n[4];
  int32_t c = 0;
  for (int32_t i = threadIdx.x; i < n_part; i += 256) c += part_n[i];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) c += __shfl_xor(c, off);
  if ((threadIdx.x & 63) == 0) red_n[threadIdx.x >> 6] = c;
  __syncthreads();
  const int32_t n_l = (red_n[0] + red_n[1]) + (red_n[2] + red_n[3]);
  const float scale_e = k > 0 ? coef_e * 2.0f / (float)k : 0.f;
  const float scale_l = n_l > 0 ? coef_l * 2.0f / (float)n_l : 0.f;
  const int64_t n_w = 2 * k + n_cand;
  const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x, stride = (int64_t)gridDim.x * 256;
  // decoded entry e: e < k +diff_e, e < 2k -diff_{e-k}, else candidate e - 2k = item e - k
  for (int64_t e = tid; e < n_w; e += stride)
    w[e] = e < k ? scale_e * raw[e] : e < 2 * k ? -(scale_e * raw[e - k]) : scale_l * raw[e - k];
  if (src_edge) {
    int64_t total = inc_ptr[n_nodes];
    if (total > 2 * n_w) total = 2 * n_w;           // (two incidences per decoded edge: the size of w_inc)
    for (int64_t i = tid; i < total; i += stride) {
      const int64_t e = src_edge[i];
      float v = 0.f;
      if (e >= 0 && e < n_w) v = e < k ? scale_e * raw[e] : e < 2 * k ? -(scale_e * raw[e - k]) : scale_l * raw[e - k];
      w_inc[i] = v;
    }
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    float se = 0.f, sl = 0.f;
    for (int32_t i = 0; i < n_part; ++i) { se += part_e[i]; sl += part_l[i]; }
    const float loss_e = se / (float)k, loss_l = sl / (float)n_l;
    losses[0] = coef_e * loss_e + coef_l * loss_l;
    losses[1] = loss_e;
    losses[2] = loss_l;
  }
}

static inline int batch_loss_blocks(int64_t items, int lpr) {
  const int64_t nb = dec_blocks(items > 0 ? items : 1, lpr);
  return (int)(nb < kBatchLossMaxBlocks ? nb : kBatchLossMaxBlocks);
}

}  // namespace gd

extern "C" int64_t gd_edgeprob_dec_workspace(int64_t m, int32_t d) {
  using namespace gd;
  if (m <= 0 || d <= 0 || d % 4) return 1;
  return dec_blocks(m, lanes_per_row(d / 4));
}

extern "C" int gd_edgeprob_dec_f32(const float* z, int64_t ld_z, int64_t n_nodes, int32_t d, const int64_t* pos,
                                   int64_t ld_pos, const int64_t* neg, int64_t ld_neg, int64_t m, float coef, float* w,
                                   float* loss, const int32_t* src_edge, const int64_t* inc_ptr, float* w_inc,
                                   float* workspace, void* stream) {
  using namespace gd;
  GD_REQUIRE(z && pos && neg && w && loss && workspace, GD_E_NULL, "gd_edgeprob_dec_f32: null pointer");
  GD_REQUIRE((src_edge == nullptr) == (inc_ptr == nullptr) && (src_edge == nullptr) == (w_inc == nullptr), GD_E_NULL,
             "gd_edgeprob_dec_f32: src_edge, inc_ptr and w_inc go together");
  GD_REQUIRE(m >= 1 && m < (1ll << 30), GD_E_DIM, "gd_edgeprob_dec_f32: m=%lld (the MSE of no edges is NaN upstream)", (long long)m);
  GD_REQUIRE(n_nodes >= 1 && d > 0 && d % 4 == 0 && d <= 4096 && ld_z >= d && ld_z % 4 == 0 && ld_pos >= m && ld_neg >= m, GD_E_DIM,
             "gd_edgeprob_dec_f32: d=%d must be a multiple of 4 with 16-byte row pitches (ld_z=%lld)", d, (long long)ld_z);
  GD_REQUIRE(aligned16(z), GD_E_ALIGN, "gd_edgeprob_dec_f32: unaligned z");
  hipStream_t s = (hipStream_t)stream;
  const int d4 = d / 4;
  const int lpr = lanes_per_row(d4);
  const int nb = dec_blocks(m, lpr);
  const float scale = coef * 2.0f / (float)m;
#define GD_DEC_CASE(LPR) \
  hipLaunchKernelGGL((edgeprob_dec_kernel<LPR>), dim3(nb), dim3(256), 0, s, z, ld_z, n_nodes, d4, pos, ld_pos, neg, ld_neg, m, scale, w, workspace)
  switch (lpr) {
    case 1: GD_DEC_CASE(1); break;
    case 2: GD_DEC_CASE(2); break;
    case 4: GD_DEC_CASE(4); break;
    case 8: GD_DEC_CASE(8); break;
    case 16: GD_DEC_CASE(16); break;
    case 32: GD_DEC_CASE(32); break;
    default: GD_DEC_CASE(64); break;
  }
#undef GD_DEC_CASE
  int rc = launched("edgeprob_dec");
  if (rc) return rc;
  const int64_t fb = src_edge ? (4 * m + 255) / 256 : 1;
  hipLaunchKernelGGL(edgeprob_dec_finish_kernel, dim3((unsigned)(fb > 1024 ? 1024 : fb)), dim3(256), 0, s, workspace, nb,
                     1.0f / (float)m, loss, w, 2 * m, src_edge, inc_ptr, n_nodes, w_inc);
  return launched("edgeprob_dec_finish");
}

extern "C" int64_t gd_edge_incidence_workspace(int64_t n_nodes, int64_t n_edges) {
  if (n_nodes < 0 || n_edges < 0) return 0;
  return 4 * (n_nodes + 2 * n_edges) + 16;
}

extern "C" int gd_edge_incidence(const int64_t* e0, const int64_t* e1, int64_t n_edges, int64_t n_nodes, int64_t* inc_ptr,
                                 int32_t* other, int32_t* src_edge, void* workspace, int64_t workspace_bytes, void* stream) {
  using namespace gd;
  GD_REQUIRE(inc_ptr && workspace, GD_E_NULL, "gd_edge_incidence: null pointer");
  GD_REQUIRE(n_edges >= 0 && n_nodes >= 1 && n_nodes < (1ll << 31) && n_edges < (1ll << 29), GD_E_DIM,
             "gd_edge_incidence: n_nodes=%lld n_edges=%lld out of range", (long long)n_nodes, (long long)n_edges);
  GD_REQUIRE(n_edges == 0 || (e0 && e1 && other && src_edge), GD_E_NULL, "gd_edge_incidence: null pointer");
  GD_REQUIRE(workspace_bytes >= gd_edge_incidence_workspace(n_nodes, n_edges), GD_E_WORKSPACE,
             "gd_edge_incidence: workspace of %lld bytes, %lld needed", (long long)workspace_bytes,
             (long long)gd_edge_incidence_workspace(n_nodes, n_edges));
  hipStream_t s = (hipStream_t)stream;
  int32_t* count = reinterpret_cast<int32_t*>(workspace);
  int32_t* slots = count + n_nodes;
  hipError_t e = hipMemsetAsync(count, 0, sizeof(int32_t) * n_nodes, s);
  if (e != hipSuccess) return fail(-(int)e, "gd_edge_incidence: %s", hipGetErrorString(e));
  const dim3 grid((unsigned)((2 * n_edges + 255) / 256));
  int rc;
  if (n_edges > 0) {
    hipLaunchKernelGGL(inc_count_kernel, grid, dim3(256), 0, s, e0, e1, n_edges, n_nodes, count);
    if ((rc = launched("inc_count"))) return rc;
  }
  hipLaunchKernelGGL(inc_scan_kernel, dim3(1), dim3(1024), 0, s, count, n_nodes, inc_ptr);
  if ((rc = launched("inc_scan")) || n_edges == 0) return rc;
  hipLaunchKernelGGL(inc_fill_kernel, grid, dim3(256), 0, s, e0, e1, n_edges, n_nodes, inc_ptr, count, slots);
  if ((rc = launched("inc_fill"))) return rc;
  hipLaunchKernelGGL(inc_rank_kernel, grid, dim3(256), 0, s, e0, e1, n_edges, n_nodes, inc_ptr, slots, other, src_edge);
  return launched("inc_rank");
}

extern "C" int64_t gd_edgeprob_batch_loss_workspace(int64_t k, int64_t n_cand, int32_t d) {
  using namespace gd;
  if (k < 0 || n_cand < 0 || k + n_cand >= (1ll << 28) || d <= 0 || d % 4) return -1;
  return 3 * (int64_t)batch_loss_blocks(k + n_cand, lanes_per_row(d / 4)) + k + n_cand + 4;
}

extern "C" int gd_edgeprob_batch_loss_f32(const float* z, int64_t ld_z, int64_t n_nodes, const float* z_ori, int64_t ld_ori,
                                          int64_t n_ori, int32_t d, const int64_t* pos, int64_t ld_pos, const int64_t* neg,
                                          int64_t ld_neg, int64_t k, const int64_t* cand_src, const int64_t* cand_dst,
                                          int64_t n_cand, float coef_e, float coef_l, int64_t* dec, int64_t ld_dec, float* w,
                                          float* losses, int64_t* inc_ptr, int32_t* other, int32_t* src_edge, float* w_inc,
                                          void* inc_workspace, int64_t inc_workspace_bytes, float* workspace, void* stream) {
  using namespace gd;
  GD_REQUIRE(z && z_ori && dec && w && losses && workspace, GD_E_NULL, "gd_edgeprob_batch_loss_f32: null pointer");
  GD_REQUIRE(k >= 0 && n_cand >= 0 && k + n_cand < (1ll << 28), GD_E_DIM, "gd_edgeprob_batch_loss_f32: k=%lld n_cand=%lld out of range",
             (long long)k, (long long)n_cand);
  GD_REQUIRE((k == 0 || (pos && neg)) && (n_cand == 0 || (cand_src && cand_dst)), GD_E_NULL,
             "gd_edgeprob_batch_loss_f32: null edge list");
  const bool inc = inc_ptr != nullptr;
  GD_REQUIRE(inc == (other != nullptr) && inc == (src_edge != nullptr) && inc == (w_inc != nullptr) && inc == (inc_workspace != nullptr),
             GD_E_NULL, "gd_edgeprob_batch_loss_f32: inc_ptr, other, src_edge, w_inc and inc_workspace go together");
  const int64_t n_w = 2 * k + n_cand;
  GD_REQUIRE(n_nodes >= 1 && n_nodes < (1ll << 31) && n_ori >= 1 && d > 0 && d % 4 == 0 && d <= 4096 && ld_z >= d && ld_z % 4 == 0 &&
                 ld_ori >= d && ld_ori % 4 == 0 && ld_pos >= k && ld_neg >= k && ld_dec >= n_w,
             GD_E_DIM, "gd_edgeprob_batch_loss_f32: d=%d must be a multiple of 4 with 16-byte row pitches (ld_z=%lld, ld_ori=%lld)", d,
             (long long)ld_z, (long long)ld_ori);
  GD_REQUIRE(aligned16(z) && aligned16(z_ori), GD_E_ALIGN, "gd_edgeprob_batch_loss_f32: unaligned z / z_ori");
  GD_REQUIRE(!inc || inc_workspace_bytes >= gd_edge_incidence_workspace(n_nodes, n_w), GD_E_WORKSPACE,
             "gd_edgeprob_batch_loss_f32: incidence workspace of %lld bytes, %lld needed", (long long)inc_workspace_bytes,
             (long long)gd_edge_incidence_workspace(n_nodes, n_w));
  hipStream_t s = (hipStream_t)stream;
  const int d4 = d / 4;
  const int lpr = lanes_per_row(d4);
  const int nb = batch_loss_blocks(k + n_cand, lpr);
  float* part_e = workspace;
  float* part_l = part_e + nb;
  int32_t* part_n = reinterpret_cast<int32_t*>(part_l + nb);
  float* raw = part_l + 2 * nb;
#define GD_BL_CASE(LPR)                                                                                                          \
  hipLaunchKernelGGL((edgeprob_batch_dots_kernel<LPR>), dim3(nb), dim3(256), 0, s, z, ld_z, n_nodes, z_ori, ld_ori, n_ori, d4, pos, \
                     ld_pos, neg, ld_neg, k, cand_src, cand_dst, n_cand, dec, ld_dec, raw, part_e, part_l, part_n)
  switch (lpr) {
    case 1: GD_BL_CASE(1); break;
    case 2: GD_BL_CASE(2); break;
    case 4: GD_BL_CASE(4); break;
    case 8: GD_BL_CASE(8); break;
    case 16: GD_BL_CASE(16); break;
    case 32: GD_BL_CASE(32); break;
    default: GD_BL_CASE(64); break;
  }
#undef GD_BL_CASE
  int rc = launched("edgeprob_batch_dots");
  if (rc) return rc;
  if (inc) {      // the list over all decoded edges: a candidate that does not count is (-1, -1) and gets no entries
    rc = gd_edge_incidence(dec, dec + ld_dec, n_w, n_nodes, inc_ptr, other, src_edge, inc_workspace, inc_workspace_bytes, stream);
    if (rc) return rc;
  }
  const int64_t fb = ((inc ? 2 : 1) * n_w + 255) / 256;
  hipLaunchKernelGGL(edgeprob_batch_finish_kernel, dim3((unsigned)(fb > 1024 ? 1024 : fb < 1 ? 1 : fb)), dim3(256), 0, s, part_e,
                     part_l, part_n, nb, k, n_cand, coef_e, coef_l, raw, w, losses, src_edge, inc_ptr, n_nodes, w_inc);
  return launched("edgeprob_batch_finish");
}

extern "C" int gd_rows_add_f32(float* dz, int64_t ld_dz, int64_t n_rows, const int32_t* nodes, int32_t n_s, const float* src,
                               int64_t ld_src, float scale, int32_t d, void* stream) {
  using namespace gd;
  GD_REQUIRE(n_s >= 0 && n_rows >= 0 && d > 0 && d % 4 == 0 && ld_dz >= d && ld_src >= d && ld_dz % 4 == 0 && ld_src % 4 == 0, GD_E_DIM,
             "gd_rows_add_f32: d=%d must be a multiple of 4 with 16-byte row pitches", d);
  if (n_s == 0) return GD_OK;
  GD_REQUIRE(dz && nodes && src, GD_E_NULL, "gd_rows_add_f32: null pointer");
  GD_REQUIRE(aligned16(dz) && aligned16(src), GD_E_ALIGN, "gd_rows_add_f32: unaligned matrix");
  const int d4 = d / 4;
  const int lpr = lanes_per_row(d4);
  const dim3 grid((unsigned)dec_blocks(n_s, lpr));
#define GD_ADD_CASE(LPR) \
  hipLaunchKernelGGL((rows_add_kernel<LPR>), grid, dim3(256), 0, (hipStream_t)stream, dz, ld_dz, n_rows, nodes, n_s, src, ld_src, scale, d4)
  switch (lpr) {
    case 1: GD_ADD_CASE(1); break;
    case 2: GD_ADD_CASE(2); break;
    case 4: GD_ADD_CASE(4); break;
    case 8: GD_ADD_CASE(8); break;
    case 16: GD_ADD_CASE(16); break;
    case 32: GD_ADD_CASE(32); break;
    default: GD_ADD_CASE(64); break;
  }
#undef GD_ADD_CASE
  return launched("rows_add");
}

extern "C" int gd_edgeprob_record_f32(const float* loss_r, const float* loss_l, float coef_r, float coef_l, float* hist,
                                      int32_t capacity, int32_t* pos, void* stream) {
  using namespace gd;
  GD_REQUIRE(loss_r && hist && pos, GD_E_NULL, "gd_edgeprob_record_f32: null pointer");
  GD_REQUIRE(capacity > 0, GD_E_DIM, "gd_edgeprob_record_f32: capacity must be positive");
  hipLaunchKernelGGL(edgeprob_record_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, loss_r, loss_l, coef_r, coef_l, hist,
                     capacity, pos);
  return launched("edgeprob_record");
}
