// The decoder's incidence list when only the tail of the decoded edges changes between calls (fresh negatives every epoch
// behind a fixed positive half): gd_edge_incidence_fixed builds an image of the fixed half once, gd_edge_incidence_update
// merges the variable edges' entries into it and writes exactly what gd_edge_incidence writes over the whole list.
//
// Node v's list in the order of a stable sort of cat(e0, e1) by node is
//     [ fixed, e0 = v | variable, e0 = v | fixed, e1 = v | variable, e1 = v ]        each part by ascending edge index
// because every fixed edge index is below every variable one and every e0 entry (position p < M) lies before every e1
// entry (p >= M).  The image holds the first and the third part of every node, already in order, with the node of every
// entry; an update is
//     zero      cnt[0, 2n) = 0                                              (the entry's own first launch: see below)
//     count     per variable edge: its arrival numbers among its nodes' variable source / destination entries
//     scan      inc_ptr = exclusive scan of (fixed entries + variable source + variable destination entries) per node:
//               a sum per 1,024-node tile, one block over the tile sums, then every tile again (three launches)
//     copy      every fixed entry to its place, the destination part shifted by the node's variable source count
//     fill      every variable entry's edge index into its node's part of `slots`, at its arrival number
//     rank      every variable entry's place = the number of smaller edge indices in its part; other / src_edge written
// Seven launches on the stream and nothing else: no memset, no copy, no block waiting on another block.  The integer
// atomics of `count` hand out arrival numbers, which decide only where an edge index sits inside its part of `slots`; the
// rank pass reads the whole part, so what is written does not depend on them.
//
// No count is added twice: cnt is written by this file's kernels only, `zero` is the first launch of every call and the
// launches of one call are ordered by the stream, so `count` always adds to zeros - whatever an earlier call (finished,
// refused half way or on another edge list) left there.  No write index reaches 2 n_edges: `scan` sums, per node,
// exactly the image's count plus the two counts `count` produced, `copy` / `fill` / `rank` write node v's entries at
// inc_ptr[v] + (an offset below that same sum), so every index is below inc_ptr[n] = (valid entries) <= 2 n_edges.  An
// image that belongs to other arguments could break the first half of that sentence, so every store is also guarded by
// the bound itself.
#include "common.h"

namespace gd {

constexpr int kIncTile = 1024;  // nodes per scan block: 256 threads x 4 consecutive nodes

struct IncImage {               // views into an image of (n, n_fixed); all null for "no fixed half"
  const int64_t* fptr;          // [n + 1] node v's fixed entries are [fptr[v], fptr[v + 1])
  const int32_t* nsrc;          // [n]     how many of them are source (e0) entries: those come first
  const int32_t* node;          // [2 F]   the node of every fixed entry
  const int32_t* other;         // [2 F]
  const int32_t* src_edge;      // [2 F]
};

static inline int64_t image_nsrc_offset(int64_t n) { return 8 * (n + 1); }
static inline int64_t image_entries_offset(int64_t n) { return image_nsrc_offset(n) + 4 * (n + (n & 1)); }
static inline int64_t image_bytes(int64_t n, int64_t f) { return image_entries_offset(n) + 24 * f; }

static inline int64_t scan_tiles(int64_t n) { return (n + kIncTile - 1) / kIncTile; }

__device__ __forceinline__ bool inc_valid(int64_t a, int64_t b, int64_t n) { return a >= 0 && a < n && b >= 0 && b < n; }

__global__ __launch_bounds__(256) void incu_zero_kernel(int32_t* __restrict__ cnt, int64_t n2) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n2) cnt[i] = 0;
}

// variable edge lo + i: arrival numbers among node e0's variable source entries and node e1's variable destination entries
__global__ __launch_bounds__(256) void incu_count_kernel(const int64_t* __restrict__ e0, const int64_t* __restrict__ e1, int64_t lo,
                                                         int64_t n_var, int64_t n, int32_t* __restrict__ cnt,
                                                         int32_t* __restrict__ arrival) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n_var) return;
  const int64_t a = e0[lo + i], b = e1[lo + i];
  if (!inc_valid(a, b, n)) return;
  arrival[i] = atomicAdd(&cnt[a], 1);
  arrival[n_var + i] = atomicAdd(&cnt[n + b], 1);
}

__device__ __forceinline__ int64_t inc_degree(const int64_t* __restrict__ fptr, const int32_t* __restrict__ cnt, int64_t n, int64_t v) {
  return (fptr ? fptr[v + 1] - fptr[v] : 0) + (int64_t)cnt[v] + (int64_t)cnt[n + v];
}

// the sum of the 4 nodes of every thread and of the block's tile; part[] afterwards: inclusive sums over the threads
__device__ __forceinline__ int64_t inc_tile_scan(const int64_t* __restrict__ fptr, const int32_t* __restrict__ cnt, int64_t n,
                                                 int64_t* part, int64_t deg[4]) {
  const int t = threadIdx.x;
  const int64_t v0 = (int64_t)blockIdx.x * kIncTile + 4 * t;
  int64_t s = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    deg[k] = v0 + k < n ? inc_degree(fptr, cnt, n, v0 + k) : 0;
    s += deg[k];
  }
  part[t] = s;
  __syncthreads();
  for (int off = 1; off < 256; off <<= 1) {
    const int64_t add = t >= off ? part[t - off] : 0;
    __syncthreads();
    part[t] += add;
    __syncthreads();
  }
  return s;
}

__global__ __launch_bounds__(256) void incu_tile_sum_kernel(const int64_t* __restrict__ fptr, const int32_t* __restrict__ cnt,
                                                            int64_t n, int64_t* __restrict__ tile_sum) {
  __shared__ int64_t part[256];
  int64_t deg[4];
  inc_tile_scan(fptr, cnt, n, part, deg);
  if (threadIdx.x == 255) tile_sum[blockIdx.x] = part[255];
}

// tile_sum[0, n_tiles) -> its exclusive scan in place, the total at [n_tiles]; one block, consecutive chunks per thread
__global__ __launch_bounds__(1024) void incu_tile_offsets_kernel(int64_t* __restrict__ tile_sum, int64_t n_tiles) {
  __shared__ int64_t part[1024];
  const int t = threadIdx.x;
  const int64_t chunk = (n_tiles + 1023) / 1024;
  const int64_t lo = min(n_tiles, t * chunk), hi = min(n_tiles, lo + chunk);
  int64_t s = 0;
  for (int64_t b = lo; b < hi; ++b) s += tile_sum[b];
  part[t] = s;
  __syncthreads();
  for (int off = 1; off < 1024; off <<= 1) {
    const int64_t add = t >= off ? part[t - off] : 0;
    __syncthreads();
    part[t] += add;
    __syncthreads();
  }
  int64_t run = part[t] - s;
  for (int64_t b = lo; b < hi; ++b) {
    const int64_t here = tile_sum[b];
    tile_sum[b] = run;
    run += here;
  }
  if (t == 1023) tile_sum[n_tiles] = part[1023];
}

// inc_ptr[v] for the tile's nodes, inc_ptr[n] by the last tile; nsrc_out (the image being built): the source counts
__global__ __launch_bounds__(256) void incu_tile_apply_kernel(const int64_t* __restrict__ fptr, const int32_t* __restrict__ cnt,
                                                              int64_t n, const int64_t* __restrict__ tile_off, int64_t n_tiles,
                                                              int64_t* __restrict__ inc_ptr, int32_t* __restrict__ nsrc_out) {
  __shared__ int64_t part[256];
  int64_t deg[4];
  const int64_t s = inc_tile_scan(fptr, cnt, n, part, deg);
  const int t = threadIdx.x;
  const int64_t v0 = (int64_t)blockIdx.x * kIncTile + 4 * t;
  int64_t run = tile_off[blockIdx.x] + part[t] - s;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (v0 + k < n) {
      inc_ptr[v0 + k] = run;
      if (nsrc_out) nsrc_out[v0 + k] = cnt[v0 + k];
    }
    run += deg[k];
  }
  if (blockIdx.x == n_tiles - 1 && t == 255) inc_ptr[n] = tile_off[n_tiles];
}

// fixed entry j of the image -> its place: the node's source part stays at the head of the list, the destination part
// moves behind the variable source entries
__global__ __launch_bounds__(256) void incu_copy_kernel(IncImage im, int64_t n, int64_t cap_fixed, const int32_t* __restrict__ cnt,
                                                        const int64_t* __restrict__ inc_ptr, int64_t cap, int32_t* __restrict__ other,
                                                        int32_t* __restrict__ src_edge) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= cap_fixed || j >= im.fptr[n]) return;
  const int64_t v = im.node[j];
  if (v < 0 || v >= n) return;
  const int64_t k = j - im.fptr[v];
  const int64_t at = inc_ptr[v] + k + (k >= im.nsrc[v] ? (int64_t)cnt[v] : 0);
  if (k < 0 || at < 0 || at >= cap) return;               // (an image of other arguments: never past the outputs)
  other[at] = im.other[j];
  src_edge[at] = im.src_edge[j];
}

// where node v's variable source (side 0) / destination (side 1) part begins, and how many entries it has
__device__ __forceinline__ int64_t inc_part(const IncImage& im, const int32_t* __restrict__ cnt, const int64_t* __restrict__ inc_ptr,
                                            int64_t n, int64_t v, int side, int64_t* len) {
  const int64_t fixed = im.fptr ? im.fptr[v + 1] - im.fptr[v] : 0;
  const int64_t fsrc = im.fptr ? (int64_t)im.nsrc[v] : 0;
  *len = cnt[side ? n + v : v];
  return inc_ptr[v] + (side ? fixed + (int64_t)cnt[v] : fsrc);
}

__global__ __launch_bounds__(256) void incu_fill_kernel(const int64_t* __restrict__ e0, const int64_t* __restrict__ e1, int64_t lo,
                                                        int64_t n_var, int64_t n, IncImage im, const int32_t* __restrict__ cnt,
                                                        const int32_t* __restrict__ arrival, const int64_t* __restrict__ inc_ptr,
                                                        int64_t cap, int32_t* __restrict__ slots) {
  const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (q >= 2 * n_var) return;
  const int side = q >= n_var;
  const int64_t i = side ? q - n_var : q;
  const int64_t a = e0[lo + i], b = e1[lo + i];
  if (!inc_valid(a, b, n)) return;
  int64_t len;
  const int64_t at = inc_part(im, cnt, inc_ptr, n, side ? b : a, side, &len) + arrival[q];
  if (at >= 0 && at < cap) slots[at] = (int32_t)(lo + i);
}

// node_out (the image being built): the node of every entry
__global__ __launch_bounds__(256) void incu_rank_kernel(const int64_t* __restrict__ e0, const int64_t* __restrict__ e1, int64_t lo,
                                                        int64_t n_var, int64_t n, IncImage im, const int32_t* __restrict__ cnt,
                                                        const int64_t* __restrict__ inc_ptr, const int32_t* __restrict__ slots,
                                                        int64_t cap, int32_t* __restrict__ other, int32_t* __restrict__ src_edge,
                                                        int32_t* __restrict__ node_out) {
  const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (q >= 2 * n_var) return;
  const int side = q >= n_var;
  const int64_t i = side ? q - n_var : q;
  const int64_t a = e0[lo + i], b = e1[lo + i];
  if (!inc_valid(a, b, n)) return;
  const int64_t v = side ? b : a;
  int64_t len;
  const int64_t begin = inc_part(im, cnt, inc_ptr, n, v, side, &len);
  if (len > n_var) len = n_var;                             // (a part holds variable entries of one side: n_var at the most)
  if (begin < 0 || begin + len > cap) return;
  const int32_t e = (int32_t)(lo + i);
  int64_t rank = 0;
  for (int64_t j = 0; j < len; ++j) rank += slots[begin + j] < e ? 1 : 0;
  if (rank >= len) return;                                  // (never: this entry is in the part and is not below itself)
  const int64_t at = begin + rank;
  other[at] = (int32_t)(side ? a : b);
  src_edge[at] = e;
  if (node_out) node_out[at] = (int32_t)v;
}

// The shared launch sequence over the edges [lo, lo + n_var) of (e0, e1) behind the image im (null views: none).
static int incidence_merge(const int64_t* e0, const int64_t* e1, int64_t lo, int64_t n_var, int64_t n, const IncImage& im,
                           int64_t n_fixed, int64_t* inc_ptr, int32_t* other, int32_t* src_edge, int32_t* nsrc_out, int32_t* node_out,
                           void* workspace, hipStream_t s) {
  const int64_t n_tiles = scan_tiles(n), cap = 2 * (n_fixed + n_var);
  int64_t* tile_sum = reinterpret_cast<int64_t*>(workspace);               // [n_tiles + 1]
  int32_t* cnt = reinterpret_cast<int32_t*>(tile_sum + n_tiles + 1);       // [2 n]: variable source counts | destination counts
  int32_t* arrival = cnt + 2 * n;                                          // [2 n_var]
  int32_t* slots = arrival + 2 * n_var;                                    // [cap], indexed as the outputs are
  const dim3 block(256);
  const auto blocks = [](int64_t items) { return dim3((unsigned)((items + 255) / 256)); };
  int rc;
  hipLaunchKernelGGL(incu_zero_kernel, blocks(2 * n), block, 0, s, cnt, 2 * n);
  if ((rc = launched("incidence zero"))) return rc;
  if (n_var > 0) {
    hipLaunchKernelGGL(incu_count_kernel, blocks(n_var), block, 0, s, e0, e1, lo, n_var, n, cnt, arrival);
    if ((rc = launched("incidence count"))) return rc;
  }
  hipLaunchKernelGGL(incu_tile_sum_kernel, dim3((unsigned)n_tiles), block, 0, s, im.fptr, cnt, n, tile_sum);
  if ((rc = launched("incidence tile sums"))) return rc;
  hipLaunchKernelGGL(incu_tile_offsets_kernel, dim3(1), dim3(1024), 0, s, tile_sum, n_tiles);
  if ((rc = launched("incidence tile offsets"))) return rc;
  hipLaunchKernelGGL(incu_tile_apply_kernel, dim3((unsigned)n_tiles), block, 0, s, im.fptr, cnt, n, tile_sum, n_tiles, inc_ptr, nsrc_out);
  if ((rc = launched("incidence tile apply"))) return rc;
  if (n_fixed > 0) {
    hipLaunchKernelGGL(incu_copy_kernel, blocks(2 * n_fixed), block, 0, s, im, n, 2 * n_fixed, cnt, inc_ptr, cap, other, src_edge);
    if ((rc = launched("incidence copy"))) return rc;
  }
  if (n_var > 0) {
    hipLaunchKernelGGL(incu_fill_kernel, blocks(2 * n_var), block, 0, s, e0, e1, lo, n_var, n, im, cnt, arrival, inc_ptr, cap, slots);
    if ((rc = launched("incidence fill"))) return rc;
    hipLaunchKernelGGL(incu_rank_kernel, blocks(2 * n_var), block, 0, s, e0, e1, lo, n_var, n, im, cnt, inc_ptr, slots, cap, other,
                       src_edge, node_out);
    if ((rc = launched("incidence rank"))) return rc;
  }
  return GD_OK;
}

static inline bool inc_sizes_ok(int64_t n_nodes, int64_t n_edges) {
  return n_edges >= 0 && n_nodes >= 1 && n_nodes < (1ll << 31) && n_edges < (1ll << 29);
}

}  // namespace gd

extern "C" int64_t gd_edge_incidence_fixed_bytes(int64_t n_nodes, int64_t n_fixed) {
  if (n_nodes < 0 || n_fixed < 0) return 0;
  return gd::image_bytes(n_nodes, n_fixed);
}

extern "C" int64_t gd_edge_incidence_update_workspace(int64_t n_nodes, int64_t n_edges) {
  if (n_nodes < 0 || n_edges < 0) return 0;
  return 8 * (gd::scan_tiles(n_nodes) + 1) + 4 * (2 * n_nodes + 4 * n_edges) + 16;
}

extern "C" int gd_edge_incidence_fixed(const int64_t* e0, const int64_t* e1, int64_t n_fixed, int64_t n_nodes, void* image,
                                       int64_t image_bytes, void* workspace, int64_t workspace_bytes, void* stream) {
  using namespace gd;
  GD_REQUIRE(image && workspace, GD_E_NULL, "gd_edge_incidence_fixed: null pointer");
  GD_REQUIRE(inc_sizes_ok(n_nodes, n_fixed), GD_E_DIM, "gd_edge_incidence_fixed: n_nodes=%lld n_fixed=%lld out of range",
             (long long)n_nodes, (long long)n_fixed);
  GD_REQUIRE(n_fixed == 0 || (e0 && e1), GD_E_NULL, "gd_edge_incidence_fixed: null pointer");
  GD_REQUIRE(image_bytes >= gd_edge_incidence_fixed_bytes(n_nodes, n_fixed), GD_E_WORKSPACE,
             "gd_edge_incidence_fixed: image of %lld bytes, %lld needed", (long long)image_bytes,
             (long long)gd_edge_incidence_fixed_bytes(n_nodes, n_fixed));
  GD_REQUIRE(workspace_bytes >= gd_edge_incidence_update_workspace(n_nodes, n_fixed), GD_E_WORKSPACE,
             "gd_edge_incidence_fixed: workspace of %lld bytes, %lld needed", (long long)workspace_bytes,
             (long long)gd_edge_incidence_update_workspace(n_nodes, n_fixed));
  GD_REQUIRE((reinterpret_cast<uintptr_t>(image) & 7u) == 0 && (reinterpret_cast<uintptr_t>(workspace) & 7u) == 0, GD_E_ALIGN,
             "gd_edge_incidence_fixed: image and workspace must be 8-byte aligned");
  char* base = reinterpret_cast<char*>(image);
  int64_t* fptr = reinterpret_cast<int64_t*>(base);
  int32_t* nsrc = reinterpret_cast<int32_t*>(base + image_nsrc_offset(n_nodes));
  int32_t* node = reinterpret_cast<int32_t*>(base + image_entries_offset(n_nodes));
  // the image of the fixed half is the merge of all of it, as variable edges, into no image
  return incidence_merge(e0, e1, 0, n_fixed, n_nodes, IncImage{nullptr, nullptr, nullptr, nullptr, nullptr}, 0, fptr,
                         node + 2 * n_fixed, node + 4 * n_fixed, nsrc, node, workspace, (hipStream_t)stream);
}

extern "C" int gd_edge_incidence_update(const void* image, const int64_t* e0, const int64_t* e1, int64_t n_fixed, int64_t n_edges,
                                        int64_t n_nodes, int64_t* inc_ptr, int32_t* other, int32_t* src_edge, void* workspace,
                                        int64_t workspace_bytes, void* stream) {
  using namespace gd;
  GD_REQUIRE(image && inc_ptr && workspace, GD_E_NULL, "gd_edge_incidence_update: null pointer");
  GD_REQUIRE(inc_sizes_ok(n_nodes, n_edges) && n_fixed >= 0 && n_fixed <= n_edges, GD_E_DIM,
             "gd_edge_incidence_update: n_nodes=%lld n_fixed=%lld n_edges=%lld out of range", (long long)n_nodes, (long long)n_fixed,
             (long long)n_edges);
  GD_REQUIRE(n_edges == 0 || (e0 && e1 && other && src_edge), GD_E_NULL, "gd_edge_incidence_update: null pointer");
  GD_REQUIRE(workspace_bytes >= gd_edge_incidence_update_workspace(n_nodes, n_edges), GD_E_WORKSPACE,
             "gd_edge_incidence_update: workspace of %lld bytes, %lld needed", (long long)workspace_bytes,
             (long long)gd_edge_incidence_update_workspace(n_nodes, n_edges));
  GD_REQUIRE((reinterpret_cast<uintptr_t>(image) & 7u) == 0 && (reinterpret_cast<uintptr_t>(workspace) & 7u) == 0, GD_E_ALIGN,
             "gd_edge_incidence_update: image and workspace must be 8-byte aligned");
  const char* base = reinterpret_cast<const char*>(image);
  const int32_t* node = reinterpret_cast<const int32_t*>(base + image_entries_offset(n_nodes));
  const IncImage im{reinterpret_cast<const int64_t*>(base), reinterpret_cast<const int32_t*>(base + image_nsrc_offset(n_nodes)), node,
                    node + 2 * n_fixed, node + 4 * n_fixed};
  return incidence_merge(e0, e1, n_fixed, n_edges - n_fixed, n_nodes, im, n_fixed, inc_ptr, other, src_edge, nullptr, nullptr,
                         workspace, (hipStream_t)stream);
}
