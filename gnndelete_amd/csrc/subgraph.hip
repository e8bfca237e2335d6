// GraphSAINT batch on the device: the induced-subgraph cut, the two batch CSRs the unlearning step aggregates over, and
// the per-batch loss terms (framework/trainer/gnndelete_nodeemb.py:352-445 of the reference: saint_subgraph, GCNConv /
// GATConv re-deriving their scatter indices from the batch's edge_index, the DEC / NI losses on fresh negatives).
//
// Everything here is integer work and bit-exact:
//   * the cut marks the batch's nodes in a node-sized (stamp, id) array with a per-batch generation stamp (nothing
//     O(N) is cleared per batch), counts the kept edges of every batch row with one wave per row, turns the counts
//     into row offsets with one single-block scan, and writes the rows again with one wave per row, keeping the order
//     inside a row by a 64-bit ballot + popcount compaction - so the edges come out sorted by (src, dst) exactly as
//     RandomWalkSubgraphSampler.subgraph yields them;
//   * the batch CSRs are gd_csr_from_coo over the same edge list graph.build_csr forms (self loops dropped, one loop
//     per node appended), so their index arrays are the ones build_csr would produce;
//   * the loss terms are sorted by the row of z they touch (gd_csr_from_coo again: rows = segments), which is what
//     makes the gradient accumulation of repeated endpoints deterministic in gd_rowpair_mse_f32.
#include "common.h"

namespace gd {

constexpr int kScanThreads = 1024;
constexpr int kScanWaves = kScanThreads / kWave;
constexpr int kEdgeKinds = 5;   // all, sdf, df, all without self loops, sdf without self loops
constexpr int kNodeKinds = 4;   // S1, S2, NI1, NI2 (node flag bits 0..3)
constexpr int kScanKinds = kEdgeKinds + kNodeKinds;

struct CutLayout {
  size_t row_cnt, row_off, row_flag, total;
};

static size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

static CutLayout cut_layout(int32_t n_b) {
  CutLayout L;
  size_t off = 0;
  L.row_cnt = off; off += align256((size_t)n_b * kEdgeKinds * sizeof(int32_t));
  L.row_off = off; off += align256((size_t)n_b * kEdgeKinds * sizeof(int32_t));
  L.row_flag = off; off += align256((size_t)n_b);
  L.total = off;
  return L;
}

__device__ __forceinline__ bool row_node(const int64_t* nodes, int32_t r, int32_t n_nodes, int32_t* u) {
  const int64_t v = nodes[r];
  *u = (int32_t)v;
  return v >= 0 && v < n_nodes;
}

// stamp the batch's nodes: relabel[v] = generation << 32 | batch id; the row's node flags are copied out
__global__ __launch_bounds__(256) void cut_mark_kernel(const int64_t* __restrict__ nodes, int32_t n_b, int32_t n_nodes,
                                                       const uint8_t* __restrict__ node_flags, int32_t generation,
                                                       int64_t* __restrict__ relabel, uint8_t* __restrict__ row_flag,
                                                       int32_t* __restrict__ counts) {
  const int32_t r = blockIdx.x * 256 + threadIdx.x;
  if (r >= n_b) return;
  int32_t u;
  if (!row_node(nodes, r, n_nodes, &u)) {
    row_flag[r] = 0;
    counts[10] = 1;                                  // every offender writes the same value
    return;
  }
  relabel[u] = ((int64_t)generation << 32) | (int64_t)(uint32_t)r;
  row_flag[r] = node_flags ? node_flags[u] : 0;
}

struct EdgeView {
  bool keep, all_nl, sdf, sdf_nl, df;
  int32_t dst;
};

__device__ __forceinline__ EdgeView edge_view(int32_t j, int32_t end, int32_t r, const int32_t* col, const uint8_t* edge_flags,
                                              const int64_t* relabel, int32_t generation) {
  EdgeView e{false, false, false, false, false, 0};
  if (j >= end) return e;
  const int64_t rl = relabel[col[j]];
  if ((int32_t)(rl >> 32) != generation) return e;
  const uint8_t f = edge_flags[j];
  e.dst = (int32_t)(rl & 0xffffffffll);
  e.keep = true;
  e.all_nl = e.dst != r;
  e.sdf = (f & 1) != 0;
  e.sdf_nl = e.sdf && e.all_nl;
  e.df = (f & 2) != 0;
  return e;
}

// one wave per batch row: kept edges of the row, by kind
__global__ __launch_bounds__(256) void cut_count_kernel(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                        const uint8_t* __restrict__ edge_flags, const int64_t* __restrict__ nodes,
                                                        int32_t n_b, int32_t n_nodes, const int64_t* __restrict__ relabel,
                                                        int32_t generation, int32_t* __restrict__ row_cnt) {
  const int lane = threadIdx.x & 63;
  const int32_t r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= n_b) return;
  int32_t u;
  int32_t c[kEdgeKinds] = {0, 0, 0, 0, 0};
  if (row_node(nodes, r, n_nodes, &u)) {
    const int32_t beg = rowptr[u], end = rowptr[u + 1];
    for (int32_t base = beg; base < end; base += kWave) {
      const EdgeView e = edge_view(base + lane, end, r, col, edge_flags, relabel, generation);
      c[0] += __popcll(__ballot(e.keep));
      c[1] += __popcll(__ballot(e.keep && e.sdf));
      c[2] += __popcll(__ballot(e.keep && e.df));
      c[3] += __popcll(__ballot(e.keep && e.all_nl));
      c[4] += __popcll(__ballot(e.keep && e.sdf_nl));
    }
  }
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < kEdgeKinds; ++k) row_cnt[(int64_t)k * n_b + r] = c[k];
  }
}

// single block: exclusive offsets of the five edge kinds over the rows, the four node lists written in row order,
// totals into counts
__global__ __launch_bounds__(kScanThreads) void cut_scan_kernel(const int32_t* __restrict__ row_cnt, const uint8_t* __restrict__ row_flag,
                                                                int32_t n_b, int32_t* __restrict__ row_off,
                                                                int32_t* __restrict__ row_lists, int32_t* __restrict__ counts) {
  __shared__ int32_t wave_tot[kScanWaves][kScanKinds];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int32_t carry[kScanKinds];
#pragma unroll
  for (int k = 0; k < kScanKinds; ++k) carry[k] = 0;
  for (int32_t base = 0; base < n_b; base += kScanThreads) {
    const int32_t r = base + threadIdx.x;
    int32_t v[kScanKinds], incl[kScanKinds];
    const uint8_t f = r < n_b ? row_flag[r] : 0;
#pragma unroll
    for (int k = 0; k < kEdgeKinds; ++k) v[k] = r < n_b ? row_cnt[(int64_t)k * n_b + r] : 0;
#pragma unroll
    for (int k = 0; k < kNodeKinds; ++k) v[kEdgeKinds + k] = (r < n_b && (f >> k) & 1) ? 1 : 0;
#pragma unroll
    for (int k = 0; k < kScanKinds; ++k) {
      int32_t x = v[k];
#pragma unroll
      for (int off = 1; off < kWave; off <<= 1) {
        const int32_t y = __shfl_up(x, off, kWave);
        if (lane >= off) x += y;
      }
      incl[k] = x;
      if (lane == kWave - 1) wave_tot[wave][k] = x;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kScanKinds; ++k) {
      int32_t before = carry[k], chunk = 0;
      for (int w = 0; w < kScanWaves; ++w) {
        const int32_t t = wave_tot[w][k];
        if (w < wave) before += t;
        chunk += t;
      }
      const int32_t excl = before + incl[k] - v[k];
      if (r < n_b) {
        if (k < kEdgeKinds) row_off[(int64_t)k * n_b + r] = excl;
        else if (v[k]) row_lists[(int64_t)(k - kEdgeKinds) * n_b + excl] = r;
      }
      carry[k] += chunk;
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    counts[0] = n_b;
    counts[1] = carry[0];        // e_all
    counts[2] = carry[1];        // e_sdf
    counts[3] = carry[2];        // m_df
    counts[4] = carry[5];        // |S1_b|
    counts[5] = carry[6];        // |S2_b|
    counts[6] = carry[7];        // |NI1_b|
    counts[7] = carry[8];        // |NI2_b|
    counts[8] = carry[3];        // e_all without self loops
    counts[9] = carry[4];        // e_sdf without self loops
  }
}

__device__ __forceinline__ int32_t ballot_slot(bool pred, int lane, int32_t* base) {
  const uint64_t m = __ballot(pred);
  const int32_t slot = *base + __popcll(m & ((1ull << lane) - 1ull));
  *base += __popcll(m);
  return slot;
}

struct CutOut {
  int64_t* e_index; uint8_t* e_flags; int64_t* all_src; int64_t* all_dst; int64_t* sdf_src; int64_t* sdf_dst; int64_t* df_index;
  int64_t edge_cap;
};

// one wave per batch row again: the kept edges written at the row's offsets, in CSR order inside the row
__global__ __launch_bounds__(256) void cut_write_kernel(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                        const uint8_t* __restrict__ edge_flags, const int64_t* __restrict__ nodes,
                                                        int32_t n_b, int32_t n_nodes, const int64_t* __restrict__ relabel,
                                                        int32_t generation, const int32_t* __restrict__ row_off,
                                                        const int32_t* __restrict__ counts, CutOut out) {
  const int lane = threadIdx.x & 63;
  const int32_t r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= n_b || (int64_t)counts[1] > out.edge_cap) return;      // too small: the caller grows its buffers and cuts again
  int32_t u;
  if (!row_node(nodes, r, n_nodes, &u)) return;
  int32_t o_all = row_off[r], o_df = row_off[2 * (int64_t)n_b + r];
  int32_t o_all_nl = row_off[3 * (int64_t)n_b + r], o_sdf_nl = row_off[4 * (int64_t)n_b + r];
  const int64_t cap = out.edge_cap;
  const int32_t beg = rowptr[u], end = rowptr[u + 1];
  for (int32_t base = beg; base < end; base += kWave) {
    const EdgeView e = edge_view(base + lane, end, r, col, edge_flags, relabel, generation);
    const int32_t s_all = ballot_slot(e.keep, lane, &o_all);
    const int32_t s_df = ballot_slot(e.keep && e.df, lane, &o_df);
    const int32_t s_nl = ballot_slot(e.keep && e.all_nl, lane, &o_all_nl);
    const int32_t s_sdf = ballot_slot(e.keep && e.sdf_nl, lane, &o_sdf_nl);
    if (!e.keep) continue;
    out.e_index[s_all] = r;
    out.e_index[cap + s_all] = e.dst;
    out.e_flags[s_all] = (uint8_t)((e.sdf ? 1 : 0) | (e.df ? 2 : 0));
    if (e.df) { out.df_index[s_df] = r; out.df_index[cap + s_df] = e.dst; }
    if (e.all_nl) { out.all_src[s_nl] = r; out.all_dst[s_nl] = e.dst; }
    if (e.sdf_nl) { out.sdf_src[s_sdf] = r; out.sdf_dst[s_sdf] = e.dst; }
  }
}

// ------------------------------------------------------------------------------------------- batch CSR
__global__ __launch_bounds__(256) void append_loops_kernel(int64_t* __restrict__ src, int64_t* __restrict__ dst, int64_t n_edges,
                                                           int32_t n) {
  const int32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  src[n_edges + i] = i;
  dst[n_edges + i] = i;
}

// pos_fwd[order[k]] = k: the forward CSR slot of every input edge
__global__ __launch_bounds__(256) void invert_order_kernel(const int32_t* __restrict__ order, int64_t nnz, int32_t* __restrict__ pos) {
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (k < nnz) pos[order[k]] = (int32_t)k;
}

// perm_t[k] = pos_fwd[order_t[k]];  val_t[k] = val[perm_t[k]] (gcn)
__global__ __launch_bounds__(256) void perm_t_kernel(const int32_t* __restrict__ order_t, const int32_t* __restrict__ pos_fwd,
                                                     int64_t nnz, const float* __restrict__ val, int32_t* __restrict__ perm_t,
                                                     float* __restrict__ val_t) {
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (k >= nnz) return;
  const int32_t p = pos_fwd[order_t[k]];
  perm_t[k] = p;
  if (val) val_t[k] = val[p];
}

struct CsrLayout {
  size_t order, order_t, pos_fwd, status, coo, coo_bytes, total;
};

static bool csr_layout(int32_t n, int64_t n_edges, CsrLayout* L) {
  const int64_t nnz = n_edges + n;
  const int64_t coo = gd_csr_from_coo_workspace(n, nnz);
  if (coo < 0) return false;
  size_t off = 0;
  L->order = off; off += align256((size_t)nnz * 4);
  L->order_t = off; off += align256((size_t)nnz * 4);
  L->pos_fwd = off; off += align256((size_t)nnz * 4);
  L->status = off; off += 256;
  L->coo = off; off += align256((size_t)coo);
  L->coo_bytes = (size_t)coo;
  L->total = off;
  return true;
}

// ------------------------------------------------------------------------------------------- loss terms
// term t < n_pos: (row pos0[t], target neg0[t]); n_pos <= t < 2 n_pos: (pos1, neg1); then (ni[j], ni[j])
__global__ __launch_bounds__(256) void terms_coo_kernel(const int64_t* __restrict__ pos, int64_t ld_pos, const int64_t* __restrict__ neg,
                                                        int64_t ld_neg, int32_t n_pos, const int32_t* __restrict__ ni, int32_t n_ni,
                                                        int64_t* __restrict__ row, int64_t* __restrict__ tgt) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t n_dec = 2 * (int64_t)n_pos;
  if (t >= n_dec + n_ni) return;
  if (t < n_dec) {
    const int64_t half = t >= n_pos ? 1 : 0, i = t - half * n_pos;
    row[t] = pos[half * ld_pos + i];
    tgt[t] = neg[half * ld_neg + i];
  } else {
    row[t] = ni[t - n_dec];
    tgt[t] = ni[t - n_dec];
  }
}

__global__ __launch_bounds__(256) void terms_kind_kernel(const int32_t* __restrict__ order, int64_t n_terms, int64_t n_dec, float w_dec,
                                                         float w_ni, float* __restrict__ term_w, int32_t* __restrict__ term_kind) {
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (k >= n_terms) return;
  const bool ni = order[k] >= n_dec;
  term_kind[k] = ni ? 1 : 0;
  term_w[k] = ni ? w_ni : w_dec;
}

struct TermsLayout {
  size_t row, tgt, order, status, coo, coo_bytes, total;
};

static bool terms_layout(int32_t n_b, int64_t n_terms, TermsLayout* L) {
  const int64_t coo = gd_csr_from_coo_workspace(n_b, n_terms);
  if (coo < 0) return false;
  size_t off = 0;
  L->row = off; off += align256((size_t)n_terms * 8);
  L->tgt = off; off += align256((size_t)n_terms * 8);
  L->order = off; off += align256((size_t)n_terms * 4);
  L->status = off; off += 256;
  L->coo = off; off += align256((size_t)coo);
  L->coo_bytes = (size_t)coo;
  L->total = off;
  return true;
}

static unsigned blocks_for(int64_t n, int per) { return (unsigned)((n + per - 1) / per); }

}  // namespace gd

extern "C" int64_t gd_induced_subgraph_workspace(int32_t n_b) {
  if (n_b < 0) return -1;
  return (int64_t)gd::cut_layout(n_b).total;
}

extern "C" int gd_induced_subgraph(const int32_t* rowptr, const int32_t* col, const uint8_t* edge_flags, int32_t n_nodes,
                                   const int64_t* nodes, int32_t n_b, const uint8_t* node_flags, int32_t generation,
                                   int64_t* relabel, int64_t edge_cap, int64_t* e_index, uint8_t* e_flags, int64_t* all_src,
                                   int64_t* all_dst, int64_t* sdf_src, int64_t* sdf_dst, int64_t* df_index, int32_t* row_lists,
                                   int32_t* counts, void* workspace, int64_t workspace_bytes, void* stream) {
  using namespace gd;
  GD_REQUIRE(rowptr && col && edge_flags && nodes && relabel && e_index && e_flags && all_src && all_dst && sdf_src && sdf_dst &&
             df_index && row_lists && counts && workspace, GD_E_NULL, "gd_induced_subgraph: null pointer");
  GD_REQUIRE(n_nodes > 0 && n_b > 0 && n_b <= n_nodes && edge_cap >= 0 && edge_cap < (1ll << 31) && generation > 0, GD_E_DIM,
             "gd_induced_subgraph: n_nodes=%d n_b=%d edge_cap=%lld generation=%d", n_nodes, n_b, (long long)edge_cap,
             generation);
  const CutLayout L = cut_layout(n_b);
  GD_REQUIRE(workspace_bytes >= (int64_t)L.total, GD_E_WORKSPACE, "gd_induced_subgraph: workspace %lld < %lld bytes",
             (long long)workspace_bytes, (long long)L.total);
  GD_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 255u) == 0, GD_E_ALIGN, "gd_induced_subgraph: workspace not 256-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  char* ws = reinterpret_cast<char*>(workspace);
  int32_t* row_cnt = reinterpret_cast<int32_t*>(ws + L.row_cnt);
  int32_t* row_off = reinterpret_cast<int32_t*>(ws + L.row_off);
  uint8_t* row_flag = reinterpret_cast<uint8_t*>(ws + L.row_flag);
  hipError_t e = hipMemsetAsync(counts + 10, 0, sizeof(int32_t), s);
  if (e != hipSuccess) return fail(-(int)e, "gd_induced_subgraph: %s", hipGetErrorString(e));
  hipLaunchKernelGGL(cut_mark_kernel, dim3(blocks_for(n_b, 256)), dim3(256), 0, s, nodes, n_b, n_nodes, node_flags, generation,
                     relabel, row_flag, counts);
  hipLaunchKernelGGL(cut_count_kernel, dim3(blocks_for(n_b, 4)), dim3(256), 0, s, rowptr, col, edge_flags, nodes, n_b, n_nodes,
                     relabel, generation, row_cnt);
  hipLaunchKernelGGL(cut_scan_kernel, dim3(1), dim3(kScanThreads), 0, s, row_cnt, row_flag, n_b, row_off, row_lists, counts);
  const CutOut out{e_index, e_flags, all_src, all_dst, sdf_src, sdf_dst, df_index, edge_cap};
  hipLaunchKernelGGL(cut_write_kernel, dim3(blocks_for(n_b, 4)), dim3(256), 0, s, rowptr, col, edge_flags, nodes, n_b, n_nodes,
                     relabel, generation, row_off, counts, out);
  return launched("induced_subgraph");
}

extern "C" int64_t gd_batch_csr_workspace(int32_t n_nodes, int64_t n_edges) {
  gd::CsrLayout L;
  if (n_nodes <= 0 || n_edges < 0 || n_edges + n_nodes >= (1ll << 31) || !gd::csr_layout(n_nodes, n_edges, &L)) return -1;
  return (int64_t)L.total;
}

extern "C" int gd_batch_csr(int64_t* src, int64_t* dst, int64_t n_edges, int32_t n_nodes, int32_t mode, int32_t* rowptr, int32_t* col,
                            float* val, int32_t* rowptr_t, int32_t* col_t, int32_t* perm_t, float* val_t, void* workspace,
                            int64_t workspace_bytes, void* stream) {
  using namespace gd;
  GD_REQUIRE(src && dst && rowptr && col && rowptr_t && col_t && perm_t && workspace, GD_E_NULL, "gd_batch_csr: null pointer");
  GD_REQUIRE(mode == 0 || mode == 1, GD_E_DIM, "gd_batch_csr: mode=%d (0 = gcn, 1 = gat)", mode);
  GD_REQUIRE(mode == 1 || (val && val_t), GD_E_NULL, "gd_batch_csr: gcn mode needs val / val_t");
  GD_REQUIRE(n_nodes > 0 && n_edges >= 0 && n_edges + n_nodes < (1ll << 31), GD_E_DIM, "gd_batch_csr: n_nodes=%d n_edges=%lld",
             n_nodes, (long long)n_edges);
  CsrLayout L;
  GD_REQUIRE(csr_layout(n_nodes, n_edges, &L), GD_E_DIM, "gd_batch_csr: graph too large");
  GD_REQUIRE(workspace_bytes >= (int64_t)L.total, GD_E_WORKSPACE, "gd_batch_csr: workspace %lld < %lld bytes",
             (long long)workspace_bytes, (long long)L.total);
  GD_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 255u) == 0, GD_E_ALIGN, "gd_batch_csr: workspace not 256-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  char* ws = reinterpret_cast<char*>(workspace);
  int32_t* order = reinterpret_cast<int32_t*>(ws + L.order);
  int32_t* order_t = reinterpret_cast<int32_t*>(ws + L.order_t);
  int32_t* pos_fwd = reinterpret_cast<int32_t*>(ws + L.pos_fwd);
  int32_t* status = reinterpret_cast<int32_t*>(ws + L.status);
  const int64_t nnz = n_edges + n_nodes;
  hipLaunchKernelGGL(append_loops_kernel, dim3(blocks_for(n_nodes, 256)), dim3(256), 0, s, src, dst, n_edges, n_nodes);
  int rc = launched("batch_csr loops");
  if (rc) return rc;
  rc = gd_csr_from_coo(src, dst, nnz, n_nodes, rowptr, col, order, status, ws + L.coo, (int64_t)L.coo_bytes, stream);
  if (rc) return rc;
  rc = gd_csr_from_coo(dst, src, nnz, n_nodes, rowptr_t, col_t, order_t, status, ws + L.coo, (int64_t)L.coo_bytes, stream);
  if (rc) return rc;
  if (mode == 0) {
    rc = gd_gcn_norm_f32(rowptr, col, n_nodes, val, stream);
    if (rc) return rc;
  }
  hipLaunchKernelGGL(invert_order_kernel, dim3(blocks_for(nnz, 256)), dim3(256), 0, s, order, nnz, pos_fwd);
  hipLaunchKernelGGL(perm_t_kernel, dim3(blocks_for(nnz, 256)), dim3(256), 0, s, order_t, pos_fwd, nnz, mode == 0 ? val : nullptr,
                     perm_t, val_t);
  return launched("batch_csr perm");
}

extern "C" int64_t gd_batch_loss_terms_workspace(int32_t n_b, int64_t n_terms) {
  gd::TermsLayout L;
  if (n_b <= 0 || n_terms < 0 || n_terms >= (1ll << 31) || !gd::terms_layout(n_b, n_terms, &L)) return -1;
  return (int64_t)L.total;
}

extern "C" int gd_batch_loss_terms(const int64_t* pos, int64_t ld_pos, const int64_t* neg, int64_t ld_neg, int32_t n_pos,
                                   const int32_t* ni, int32_t n_ni, int32_t n_b, float w_dec, float w_ni, int32_t* seg_ptr,
                                   int32_t* term_o, float* term_w, int32_t* term_kind, void* workspace, int64_t workspace_bytes,
                                   void* stream) {
  using namespace gd;
  GD_REQUIRE(seg_ptr && workspace, GD_E_NULL, "gd_batch_loss_terms: null seg_ptr / workspace");
  GD_REQUIRE(n_b > 0 && n_pos >= 0 && n_ni >= 0 && ld_pos >= n_pos && ld_neg >= n_pos, GD_E_DIM,
             "gd_batch_loss_terms: n_b=%d n_pos=%d n_ni=%d ld_pos=%lld ld_neg=%lld", n_b, n_pos, n_ni, (long long)ld_pos,
             (long long)ld_neg);
  GD_REQUIRE(n_pos == 0 || (pos && neg), GD_E_NULL, "gd_batch_loss_terms: null pos / neg");
  GD_REQUIRE(n_ni == 0 || ni, GD_E_NULL, "gd_batch_loss_terms: null ni");
  const int64_t n_terms = 2 * (int64_t)n_pos + n_ni;
  GD_REQUIRE(n_terms == 0 || (term_o && term_w && term_kind), GD_E_NULL, "gd_batch_loss_terms: null term arrays");
  TermsLayout L;
  GD_REQUIRE(n_terms < (1ll << 31) && terms_layout(n_b, n_terms, &L), GD_E_DIM, "gd_batch_loss_terms: too many terms");
  GD_REQUIRE(workspace_bytes >= (int64_t)L.total, GD_E_WORKSPACE, "gd_batch_loss_terms: workspace %lld < %lld bytes",
             (long long)workspace_bytes, (long long)L.total);
  GD_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 255u) == 0, GD_E_ALIGN, "gd_batch_loss_terms: workspace not 256-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  char* ws = reinterpret_cast<char*>(workspace);
  int64_t* row = reinterpret_cast<int64_t*>(ws + L.row);
  int64_t* tgt = reinterpret_cast<int64_t*>(ws + L.tgt);
  int32_t* order = reinterpret_cast<int32_t*>(ws + L.order);
  int32_t* status = reinterpret_cast<int32_t*>(ws + L.status);
  if (n_terms > 0) {
    hipLaunchKernelGGL(terms_coo_kernel, dim3(blocks_for(n_terms, 256)), dim3(256), 0, s, pos, ld_pos, neg, ld_neg, n_pos, ni, n_ni,
                       row, tgt);
    int rc = launched("batch_loss_terms coo");
    if (rc) return rc;
  }
  // rows of z = CSR rows (the segments), targets = columns; ties keep the term order
  int rc = gd_csr_from_coo(tgt, row, n_terms, n_b, seg_ptr, term_o, order, status, ws + L.coo, (int64_t)L.coo_bytes, stream);
  if (rc || n_terms == 0) return rc;
  hipLaunchKernelGGL(terms_kind_kernel, dim3(blocks_for(n_terms, 256)), dim3(256), 0, s, order, n_terms, 2 * (int64_t)n_pos, w_dec,
                     w_ni, term_w, term_kind);
  return launched("batch_loss_terms kind");
}
