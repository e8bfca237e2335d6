// GraphSAINT batch of a KNOWLEDGE graph on the device (KGGNNDeleteNodeembTrainer.train, gnndelete_nodeemb.py:659-846 of the
// reference): the typed induced-subgraph cut and the node-major typed graphs gd_rgcn_conv_f32 aggregates over.
//
// Everything here is integer work and bit-exact (the one float operation is a correctly rounded 1.0f / count):
//   * gd_induced_subgraph_typed is gd_induced_subgraph (subgraph.hip) for typed edges: generation-stamped relabel array, one
//     wave per batch row counting its kept edges, one single-block scan, one wave per row writing them by ballot + popcount
//     compaction - the Dr edges and the decoded Df triples come out in RandomWalkSubgraphSampler.subgraph's order;
//   * gd_batch_typed_csr buckets the batch's Dr edges by node (integer atomics hand out bucket slots; the order they arrive in
//     only permutes a bucket), then RANKS every edge of a bucket by (relation, other endpoint, input position) - a total order,
//     so the sorted position of an edge does not depend on its bucket slot - and cuts the sorted edges into (node, relation)
//     runs with one single-block scan.  No float atomics; the counters are zeroed by the first launch.
#include "common.h"

namespace gd {

constexpr int kTScanThreads = 1024;
constexpr int kTScanWaves = kTScanThreads / kWave;

static size_t t_align256(size_t v) { return (v + 255) & ~(size_t)255; }
static unsigned t_blocks(int64_t n, int per) { return (unsigned)((n + per - 1) / per); }

__device__ __forceinline__ int32_t wave_incl_scan(int32_t x, int lane) {
#pragma unroll
  for (int off = 1; off < kWave; off <<= 1) {
    const int32_t y = __shfl_up(x, off, kWave);
    if (lane >= off) x += y;
  }
  return x;
}

// ------------------------------------------------------------------------------------------- the typed cut
constexpr int kTCutKinds = 4;        // Dr edges, decoded Df triples, list-1 rows, list-2 rows
constexpr uint8_t kRowBad = 0x80;    // row_flag bit of a node id outside [0, n_nodes)

struct TCutLayout {
  size_t row_cnt, row_off, row_flag, total;
};

static TCutLayout tcut_layout(int32_t n_b) {
  TCutLayout L;
  size_t off = 0;
  L.row_cnt = off; off += t_align256((size_t)n_b * 2 * sizeof(int32_t));
  L.row_off = off; off += t_align256((size_t)n_b * 2 * sizeof(int32_t));
  L.row_flag = off; off += t_align256((size_t)n_b);
  L.total = off;
  return L;
}

__device__ __forceinline__ bool trow_node(const int64_t* nodes, int32_t r, int32_t n_nodes, int32_t* u) {
  const int64_t v = nodes[r];
  *u = (int32_t)v;
  return v >= 0 && v < n_nodes;
}

// stamp the batch's nodes: relabel[v] = generation << 32 | batch id; the row's node flags (bits 0, 1) are copied out, an
// id out of range leaves kRowBad there (the scan turns it into the count vector's flag: nothing to clear beforehand)
__global__ __launch_bounds__(256) void tcut_mark_kernel(const int64_t* __restrict__ nodes, int32_t n_b, int32_t n_nodes,
                                                        const uint8_t* __restrict__ node_flags, int32_t generation,
                                                        int64_t* __restrict__ relabel, uint8_t* __restrict__ row_flag) {
  const int32_t r = blockIdx.x * 256 + threadIdx.x;
  if (r >= n_b) return;
  int32_t u;
  if (!trow_node(nodes, r, n_nodes, &u)) {
    row_flag[r] = kRowBad;
    return;
  }
  relabel[u] = ((int64_t)generation << 32) | (int64_t)(uint32_t)r;
  row_flag[r] = node_flags ? (uint8_t)(node_flags[u] & 3) : 0;
}

struct TEdgeView {
  bool dr, dec;
  int32_t dst, type;
};

__device__ __forceinline__ TEdgeView tedge_view(int32_t j, int32_t end, const int32_t* col, const int32_t* etype,
                                                const uint8_t* edge_flags, const int64_t* relabel, int32_t generation,
                                                int32_t num_edge_type) {
  TEdgeView e{false, false, 0, 0};
  if (j >= end) return e;
  const int64_t rl = relabel[col[j]];
  if ((int32_t)(rl >> 32) != generation) return e;
  const uint8_t f = edge_flags[j];
  e.dst = (int32_t)(rl & 0xffffffffll);
  e.type = etype[j];
  e.dr = (f & 1) != 0;
  e.dec = (f & 2) != 0 && e.type < num_edge_type;
  return e;
}

// one wave per batch row: its Dr edges and its decoded Df triples
__global__ __launch_bounds__(256) void tcut_count_kernel(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                         const int32_t* __restrict__ etype, const uint8_t* __restrict__ edge_flags,
                                                         const int64_t* __restrict__ nodes, int32_t n_b, int32_t n_nodes,
                                                         const int64_t* __restrict__ relabel, int32_t generation,
                                                         int32_t num_edge_type, int32_t* __restrict__ row_cnt) {
  const int lane = threadIdx.x & 63;
  const int32_t r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= n_b) return;
  int32_t u, c_dr = 0, c_dec = 0;
  if (trow_node(nodes, r, n_nodes, &u)) {
    const int32_t beg = rowptr[u], end = rowptr[u + 1];
    for (int32_t base = beg; base < end; base += kWave) {
      const TEdgeView e = tedge_view(base + lane, end, col, etype, edge_flags, relabel, generation, num_edge_type);
      c_dr += __popcll(__ballot(e.dr));
      c_dec += __popcll(__ballot(e.dec));
    }
  }
  if (lane == 0) {
    row_cnt[r] = c_dr;
    row_cnt[(int64_t)n_b + r] = c_dec;
  }
}

// single block: exclusive row offsets of the two edge kinds, the two row lists in row order, the count vector
__global__ __launch_bounds__(kTScanThreads) void tcut_scan_kernel(const int32_t* __restrict__ row_cnt, const uint8_t* __restrict__ row_flag,
                                                                  int32_t n_b, int32_t* __restrict__ row_off,
                                                                  int32_t* __restrict__ row_lists, int32_t* __restrict__ counts) {
  __shared__ int32_t wave_tot[kTScanWaves][kTCutKinds];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int32_t carry[kTCutKinds] = {0, 0, 0, 0};
  int bad = 0;
  for (int32_t base = 0; base < n_b; base += kTScanThreads) {
    const int32_t r = base + threadIdx.x;
    const bool in = r < n_b;
    const uint8_t f = in ? row_flag[r] : 0;
    bad |= (f & kRowBad) ? 1 : 0;
    int32_t v[kTCutKinds], incl[kTCutKinds];
    v[0] = in ? row_cnt[r] : 0;
    v[1] = in ? row_cnt[(int64_t)n_b + r] : 0;
    v[2] = (in && (f & 1)) ? 1 : 0;
    v[3] = (in && (f & 2)) ? 1 : 0;
#pragma unroll
    for (int k = 0; k < kTCutKinds; ++k) {
      incl[k] = wave_incl_scan(v[k], lane);
      if (lane == kWave - 1) wave_tot[wave][k] = incl[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kTCutKinds; ++k) {
      int32_t before = carry[k], chunk = 0;
      for (int w = 0; w < kTScanWaves; ++w) {
        const int32_t t = wave_tot[w][k];
        if (w < wave) before += t;
        chunk += t;
      }
      const int32_t excl = before + incl[k] - v[k];
      if (in) {
        if (k < 2) row_off[(int64_t)k * n_b + r] = excl;
        else if (v[k]) row_lists[(int64_t)(k - 2) * n_b + excl] = r;
      }
      carry[k] += chunk;
    }
    __syncthreads();
  }
  bad = __syncthreads_or(bad);
  if (threadIdx.x == 0) {
    counts[0] = n_b;
    counts[1] = carry[0];        // Dr edges
    counts[2] = carry[1];        // decoded Df triples
    counts[3] = carry[2];        // |list 1|
    counts[4] = carry[3];        // |list 2|
    counts[5] = bad ? 1 : 0;
  }
}

__device__ __forceinline__ int32_t tballot_slot(bool pred, int lane, int32_t* base) {
  const uint64_t m = __ballot(pred);
  const int32_t slot = *base + __popcll(m & ((1ull << lane) - 1ull));
  *base += __popcll(m);
  return slot;
}

struct TCutOut {
  int32_t* dr_src; int32_t* dr_dst; int32_t* dr_type; int64_t* df_index; int64_t* df_type;
  int64_t edge_cap;
};

// one wave per batch row again: the kept edges written at the row's offsets, in CSR order inside the row
__global__ __launch_bounds__(256) void tcut_write_kernel(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                         const int32_t* __restrict__ etype, const uint8_t* __restrict__ edge_flags,
                                                         const int64_t* __restrict__ nodes, int32_t n_b, int32_t n_nodes,
                                                         const int64_t* __restrict__ relabel, int32_t generation,
                                                         int32_t num_edge_type, const int32_t* __restrict__ row_off,
                                                         const int32_t* __restrict__ counts, TCutOut out) {
  const int lane = threadIdx.x & 63;
  const int32_t r = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int64_t cap = out.edge_cap;
  if (r >= n_b || (int64_t)counts[1] > cap || (int64_t)counts[2] > cap) return;      // too small: the caller grows and cuts again
  int32_t u;
  if (!trow_node(nodes, r, n_nodes, &u)) return;
  int32_t o_dr = row_off[r], o_dec = row_off[(int64_t)n_b + r];
  const int32_t beg = rowptr[u], end = rowptr[u + 1];
  for (int32_t base = beg; base < end; base += kWave) {
    const TEdgeView e = tedge_view(base + lane, end, col, etype, edge_flags, relabel, generation, num_edge_type);
    const int32_t s_dr = tballot_slot(e.dr, lane, &o_dr);
    const int32_t s_dec = tballot_slot(e.dec, lane, &o_dec);
    if (e.dr && s_dr < cap) { out.dr_src[s_dr] = r; out.dr_dst[s_dr] = e.dst; out.dr_type[s_dr] = e.type; }
    if (e.dec && s_dec < cap) { out.df_index[s_dec] = r; out.df_index[cap + s_dec] = e.dst; out.df_type[s_dec] = e.type; }
  }
}

// ------------------------------------------------------------------------------------------- typed batch CSR
// Direction 0 (fwd): node = target, other = source.  Direction 1 (bwd): node = source, other = target.
struct TCsrLayout {
  size_t cnt, ptr, cur, bkt_e, bkt_key, nkey, eid, pos_f, run_id, total;
};

static TCsrLayout tcsr_layout(int32_t n, int64_t e) {
  TCsrLayout L;
  size_t off = 0;
  const size_t e1 = (size_t)(e > 0 ? e : 1);
  L.cnt = off; off += t_align256((size_t)2 * n * 4);
  L.ptr = off; off += t_align256((size_t)2 * (n + 1) * 4);
  L.cur = off; off += t_align256((size_t)2 * n * 4);
  L.bkt_e = off; off += t_align256(2 * e1 * 4);
  L.bkt_key = off; off += t_align256(2 * e1 * 8);
  L.nkey = off; off += t_align256(2 * e1 * 4);
  L.eid = off; off += t_align256(2 * e1 * 4);
  L.pos_f = off; off += t_align256(e1 * 4);
  L.run_id = off; off += t_align256(2 * e1 * 4);
  L.total = off;
  return L;
}

struct TCsrArgs {
  const int32_t* src; const int32_t* dst; const int32_t* type;
  int32_t n_edges, n, n_rel, edge_cap, seg_cap;
  int32_t* cnt; int32_t* ptr; int32_t* cur; int32_t* bkt_e; int64_t* bkt_key; int32_t* nkey; int32_t* eid; int32_t* pos_f;
  int32_t* run_id;
  int32_t* node_ptr[2]; int32_t* seg_ptr[2]; int32_t* seg_rel[2]; int32_t* col[2]; float* w[2];
  int32_t* status;            // [4]: runs fwd, runs bwd, an edge with an endpoint / relation out of range, a capacity too small
};

__device__ __forceinline__ bool tedge_ok(const TCsrArgs& a, int32_t e, int32_t* s, int32_t* d, int32_t* t) {
  *s = a.src[e]; *d = a.dst[e]; *t = a.type[e];
  return *s >= 0 && *s < a.n && *d >= 0 && *d < a.n && *t >= 0 && *t < a.n_rel;
}

// first launch: the counters of this call
__global__ __launch_bounds__(256) void tcsr_zero_kernel(TCsrArgs a) {
  const int32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i < 2 * a.n) { a.cnt[i] = 0; a.cur[i] = 0; }
  if (i < 4) a.status[i] = 0;
}

__global__ __launch_bounds__(256) void tcsr_count_kernel(TCsrArgs a) {
  const int32_t e = blockIdx.x * 256 + threadIdx.x;
  if (e >= a.n_edges) return;
  int32_t s, d, t;
  if (!tedge_ok(a, e, &s, &d, &t)) { a.status[2] = 1; return; }      // every offender writes the same value
  atomicAdd(&a.cnt[d], 1);
  atomicAdd(&a.cnt[a.n + s], 1);
}

// grid (1, 2): exclusive edge offsets of the nodes, ptr[dir][n + 1]
__global__ __launch_bounds__(kTScanThreads) void tcsr_node_scan_kernel(TCsrArgs a) {
  __shared__ int32_t wave_tot[kTScanWaves];
  const int dir = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int32_t* cnt = a.cnt + (int64_t)dir * a.n;
  int32_t* ptr = a.ptr + (int64_t)dir * (a.n + 1);
  int32_t carry = 0;
  for (int32_t base = 0; base < a.n; base += kTScanThreads) {
    const int32_t i = base + threadIdx.x;
    const int32_t v = i < a.n ? cnt[i] : 0;
    const int32_t incl = wave_incl_scan(v, lane);
    if (lane == kWave - 1) wave_tot[wave] = incl;
    __syncthreads();
    int32_t before = carry, chunk = 0;
    for (int w = 0; w < kTScanWaves; ++w) {
      const int32_t t = wave_tot[w];
      if (w < wave) before += t;
      chunk += t;
    }
    if (i < a.n) ptr[i] = before + incl - v;
    carry += chunk;
    __syncthreads();
  }
  if (threadIdx.x == 0) ptr[a.n] = carry;
}

// every edge takes a slot of its node's bucket (which slot depends on the order the atomics arrive in; the rank below does not)
__global__ __launch_bounds__(256) void tcsr_bucket_kernel(TCsrArgs a) {
  const int32_t e = blockIdx.x * 256 + threadIdx.x;
  if (e >= a.n_edges) return;
  int32_t s, d, t;
  if (!tedge_ok(a, e, &s, &d, &t)) return;
#pragma unroll
  for (int dir = 0; dir < 2; ++dir) {
    const int32_t node = dir ? s : d, other = dir ? d : s;
    const int32_t slot = a.ptr[(int64_t)dir * (a.n + 1) + node] + atomicAdd(&a.cur[(int64_t)dir * a.n + node], 1);
    if (slot < a.n_edges) {
      a.bkt_e[(int64_t)dir * a.n_edges + slot] = e;
      a.bkt_key[(int64_t)dir * a.n_edges + slot] = ((int64_t)t << 32) | (int64_t)other;
    }
  }
}

// one wave per (node, direction): the sorted position of every edge of the bucket = the bucket's start + the number of its
// edges with a smaller (relation, other endpoint, input position)
__global__ __launch_bounds__(256) void tcsr_rank_kernel(TCsrArgs a) {
  const int dir = blockIdx.y, lane = threadIdx.x & 63;
  const int32_t i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= a.n) return;
  const int32_t* ptr = a.ptr + (int64_t)dir * (a.n + 1);
  const int32_t beg = ptr[i], end = ptr[i + 1];
  const int32_t* be = a.bkt_e + (int64_t)dir * a.n_edges;
  const int64_t* bk = a.bkt_key + (int64_t)dir * a.n_edges;
  for (int32_t p = beg + lane; p < end; p += kWave) {
    const int32_t e = be[p];
    const int64_t key = bk[p];
    int32_t rank = 0;
    for (int32_t q = beg; q < end; ++q) {
      const int64_t kq = bk[q];
      rank += (kq < key || (kq == key && be[q] < e)) ? 1 : 0;
    }
    const int32_t pos = beg + rank;
    if (pos >= a.n_edges) continue;
    if (pos < a.edge_cap) a.col[dir][pos] = (int32_t)(key & 0xffffffffll);
    a.nkey[(int64_t)dir * a.n_edges + pos] = i * a.n_rel + (int32_t)(key >> 32);
    a.eid[(int64_t)dir * a.n_edges + pos] = e;
    if (dir == 0) a.pos_f[e] = pos;
  }
}

// grid (1, 2): the (node, relation) runs of the sorted edges
__global__ __launch_bounds__(kTScanThreads) void tcsr_run_scan_kernel(TCsrArgs a) {
  __shared__ int32_t wave_tot[kTScanWaves];
  const int dir = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int32_t n_e = a.ptr[(int64_t)dir * (a.n + 1) + a.n];          // the edges that were in range
  const int32_t* nkey = a.nkey + (int64_t)dir * a.n_edges;
  int32_t* run_id = a.run_id + (int64_t)dir * a.n_edges;
  int32_t carry = 0;
  for (int32_t base = 0; base < n_e; base += kTScanThreads) {
    const int32_t p = base + threadIdx.x;
    const int32_t k = p < n_e ? nkey[p] : 0;
    const int32_t v = (p < n_e && (p == 0 || nkey[p - 1] != k)) ? 1 : 0;
    const int32_t incl = wave_incl_scan(v, lane);
    if (lane == kWave - 1) wave_tot[wave] = incl;
    __syncthreads();
    int32_t before = carry, chunk = 0;
    for (int w = 0; w < kTScanWaves; ++w) {
      const int32_t t = wave_tot[w];
      if (w < wave) before += t;
      chunk += t;
    }
    if (p < n_e) {
      const int32_t run = before + incl - 1;
      run_id[p] = run;
      if (v && run < a.seg_cap) {
        a.seg_ptr[dir][run] = p;
        a.seg_rel[dir][run] = k % a.n_rel;
      }
    }
    carry += chunk;
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    a.status[dir] = carry;
    if (carry <= a.seg_cap) a.seg_ptr[dir][carry] = n_e;
    else a.status[3] = 1;
    if (n_e > a.edge_cap) a.status[3] = 1;
  }
}

// grid (x, 2): node_ptr from the run ids, the weight of every sorted edge = 1 / |its FORWARD run|
__global__ __launch_bounds__(256) void tcsr_finish_kernel(TCsrArgs a) {
  const int dir = blockIdx.y;
  const int32_t t = blockIdx.x * 256 + threadIdx.x;
  const int32_t* ptr = a.ptr + (int64_t)dir * (a.n + 1);
  const int32_t n_e = ptr[a.n];
  if (t <= a.n) {
    const int32_t p = ptr[t];
    a.node_ptr[dir][t] = p < n_e ? a.run_id[(int64_t)dir * a.n_edges + p] : a.status[dir];
  }
  if (t < n_e && t < a.edge_cap) {
    const int32_t pf = dir ? a.pos_f[a.eid[(int64_t)a.n_edges + t]] : t;
    const int32_t run = a.run_id[pf];
    float w = 0.f;
    if (run + 1 <= a.seg_cap && a.status[0] <= a.seg_cap) {
      const int32_t len = a.seg_ptr[0][run + 1] - a.seg_ptr[0][run];
      w = __fdiv_rn(1.0f, (float)len);
    }
    a.w[dir][t] = w;
  }
}

}  // namespace gd

extern "C" int64_t gd_induced_subgraph_typed_workspace(int32_t n_b) {
  if (n_b < 0) return -1;
  return (int64_t)gd::tcut_layout(n_b).total;
}

extern "C" int gd_induced_subgraph_typed(const int32_t* rowptr, const int32_t* col, const int32_t* edge_type,
                                         const uint8_t* edge_flags, int32_t n_nodes, int32_t num_edge_type, const int64_t* nodes,
                                         int32_t n_b, const uint8_t* node_flags, int32_t generation, int64_t* relabel,
                                         int64_t edge_cap, int32_t* dr_src, int32_t* dr_dst, int32_t* dr_type, int64_t* df_index,
                                         int64_t* df_type, int32_t* row_lists, int32_t* counts, void* workspace,
                                         int64_t workspace_bytes, void* stream) {
  using namespace gd;
  GD_REQUIRE(rowptr && col && edge_type && edge_flags && nodes && relabel && dr_src && dr_dst && dr_type && df_index && df_type &&
             row_lists && counts && workspace, GD_E_NULL, "gd_induced_subgraph_typed: null pointer");
  GD_REQUIRE(n_nodes > 0 && n_b > 0 && n_b <= n_nodes && edge_cap >= 0 && edge_cap < (1ll << 31) && generation > 0 &&
             num_edge_type >= 0, GD_E_DIM, "gd_induced_subgraph_typed: n_nodes=%d n_b=%d edge_cap=%lld generation=%d num_edge_type=%d",
             n_nodes, n_b, (long long)edge_cap, generation, num_edge_type);
  const TCutLayout L = tcut_layout(n_b);
  GD_REQUIRE(workspace_bytes >= (int64_t)L.total, GD_E_WORKSPACE, "gd_induced_subgraph_typed: workspace %lld < %lld bytes",
             (long long)workspace_bytes, (long long)L.total);
  GD_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 255u) == 0, GD_E_ALIGN,
             "gd_induced_subgraph_typed: workspace not 256-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  char* ws = reinterpret_cast<char*>(workspace);
  int32_t* row_cnt = reinterpret_cast<int32_t*>(ws + L.row_cnt);
  int32_t* row_off = reinterpret_cast<int32_t*>(ws + L.row_off);
  uint8_t* row_flag = reinterpret_cast<uint8_t*>(ws + L.row_flag);
  hipLaunchKernelGGL(tcut_mark_kernel, dim3(t_blocks(n_b, 256)), dim3(256), 0, s, nodes, n_b, n_nodes, node_flags, generation,
                     relabel, row_flag);
  hipLaunchKernelGGL(tcut_count_kernel, dim3(t_blocks(n_b, 4)), dim3(256), 0, s, rowptr, col, edge_type, edge_flags, nodes, n_b,
                     n_nodes, relabel, generation, num_edge_type, row_cnt);
  hipLaunchKernelGGL(tcut_scan_kernel, dim3(1), dim3(kTScanThreads), 0, s, row_cnt, row_flag, n_b, row_off, row_lists, counts);
  const TCutOut out{dr_src, dr_dst, dr_type, df_index, df_type, edge_cap};
  hipLaunchKernelGGL(tcut_write_kernel, dim3(t_blocks(n_b, 4)), dim3(256), 0, s, rowptr, col, edge_type, edge_flags, nodes, n_b,
                     n_nodes, relabel, generation, num_edge_type, row_off, counts, out);
  return launched("induced_subgraph_typed");
}

extern "C" int64_t gd_batch_typed_csr_workspace(int32_t n_nodes, int64_t n_edges, int32_t n_rel) {
  if (n_nodes <= 0 || n_edges < 0 || n_rel <= 0 || n_edges >= (1ll << 30) || (int64_t)n_nodes * n_rel >= (1ll << 31)) return -1;
  return (int64_t)gd::tcsr_layout(n_nodes, n_edges).total;
}

extern "C" int gd_batch_typed_csr(const int32_t* src, const int32_t* dst, const int32_t* type, int64_t n_edges, int32_t n_nodes,
                                  int32_t n_rel, int64_t edge_cap, int64_t seg_cap, int32_t* node_ptr, int32_t* seg_ptr,
                                  int32_t* seg_rel, int32_t* col, float* w, int32_t* node_ptr_t, int32_t* seg_ptr_t,
                                  int32_t* seg_rel_t, int32_t* col_t, float* w_t, int32_t* status, void* workspace,
                                  int64_t workspace_bytes, void* stream) {
  using namespace gd;
  GD_REQUIRE(node_ptr && seg_ptr && node_ptr_t && seg_ptr_t && status && workspace, GD_E_NULL, "gd_batch_typed_csr: null pointer");
  GD_REQUIRE(n_nodes > 0 && n_rel > 0 && n_edges >= 0 && n_edges < (1ll << 30) && (int64_t)n_nodes * n_rel < (1ll << 31), GD_E_DIM,
             "gd_batch_typed_csr: n_nodes=%d n_rel=%d n_edges=%lld", n_nodes, n_rel, (long long)n_edges);
  GD_REQUIRE(edge_cap >= n_edges && seg_cap >= 0 && edge_cap < (1ll << 31) && seg_cap < (1ll << 31), GD_E_DIM,
             "gd_batch_typed_csr: edge_cap=%lld seg_cap=%lld for %lld edges", (long long)edge_cap, (long long)seg_cap,
             (long long)n_edges);
  GD_REQUIRE(n_edges == 0 || (src && dst && type && seg_rel && col && w && seg_rel_t && col_t && w_t), GD_E_NULL,
             "gd_batch_typed_csr: null edge array");
  const TCsrLayout L = tcsr_layout(n_nodes, n_edges);
  GD_REQUIRE(workspace_bytes >= (int64_t)L.total, GD_E_WORKSPACE, "gd_batch_typed_csr: workspace %lld < %lld bytes",
             (long long)workspace_bytes, (long long)L.total);
  GD_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 255u) == 0, GD_E_ALIGN, "gd_batch_typed_csr: workspace not 256-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  char* ws = reinterpret_cast<char*>(workspace);
  TCsrArgs a;
  a.src = src; a.dst = dst; a.type = type;
  a.n_edges = (int32_t)n_edges; a.n = n_nodes; a.n_rel = n_rel; a.edge_cap = (int32_t)edge_cap; a.seg_cap = (int32_t)seg_cap;
  a.cnt = reinterpret_cast<int32_t*>(ws + L.cnt);
  a.ptr = reinterpret_cast<int32_t*>(ws + L.ptr);
  a.cur = reinterpret_cast<int32_t*>(ws + L.cur);
  a.bkt_e = reinterpret_cast<int32_t*>(ws + L.bkt_e);
  a.bkt_key = reinterpret_cast<int64_t*>(ws + L.bkt_key);
  a.nkey = reinterpret_cast<int32_t*>(ws + L.nkey);
  a.eid = reinterpret_cast<int32_t*>(ws + L.eid);
  a.pos_f = reinterpret_cast<int32_t*>(ws + L.pos_f);
  a.run_id = reinterpret_cast<int32_t*>(ws + L.run_id);
  a.node_ptr[0] = node_ptr; a.node_ptr[1] = node_ptr_t;
  a.seg_ptr[0] = seg_ptr; a.seg_ptr[1] = seg_ptr_t;
  a.seg_rel[0] = seg_rel; a.seg_rel[1] = seg_rel_t;
  a.col[0] = col; a.col[1] = col_t;
  a.w[0] = w; a.w[1] = w_t;
  a.status = status;
  const unsigned eb = t_blocks(n_edges > 0 ? n_edges : 1, 256);
  hipLaunchKernelGGL(tcsr_zero_kernel, dim3(t_blocks(2 * (int64_t)n_nodes > 4 ? 2 * (int64_t)n_nodes : 4, 256)), dim3(256), 0, s, a);
  if (n_edges > 0) hipLaunchKernelGGL(tcsr_count_kernel, dim3(eb), dim3(256), 0, s, a);
  hipLaunchKernelGGL(tcsr_node_scan_kernel, dim3(1, 2), dim3(kTScanThreads), 0, s, a);
  if (n_edges > 0) {
    hipLaunchKernelGGL(tcsr_bucket_kernel, dim3(eb), dim3(256), 0, s, a);
    hipLaunchKernelGGL(tcsr_rank_kernel, dim3(t_blocks(n_nodes, 4), 2), dim3(256), 0, s, a);
  }
  hipLaunchKernelGGL(tcsr_run_scan_kernel, dim3(1, 2), dim3(kTScanThreads), 0, s, a);
  const int64_t span = n_edges > (int64_t)n_nodes + 1 ? n_edges : (int64_t)n_nodes + 1;
  hipLaunchKernelGGL(tcsr_finish_kernel, dim3(t_blocks(span, 256), 2), dim3(256), 0, s, a);
  return launched("batch_typed_csr");
}
