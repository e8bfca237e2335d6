/*
 * gnndelete_hip.h - C ABI of libgnndelete_hip.so, the MI355X (gfx950) kernels behind the
 * GNNDelete hot path.
 *
 * The reference (mims-harvard/GNNDelete) has no FFI: its hot path runs inside PyTorch and the
 * un-vendored torch_geometric ops.  Each entry below replaces the third-party/PyTorch op chain
 * the reference calls at the cited site (paths relative to /root/reference).  The host-side
 * mirror of the reference's Python operator API (gnndelete_amd/framework) binds these symbols
 * with ctypes; INTEGRATION.md shows the stub a maintainer of the reference would add.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer into caller-owned storage (PyTorch tensors); nothing
 *     is allocated, freed or retained; scratch is passed in explicitly;
 *   - `stream` is a hipStream_t passed as void* (torch.cuda.current_stream().cuda_stream);
 *     every call only enqueues work on it and returns (capturable in a hipGraph);
 *   - matrices are row-major fp32 with an explicit leading dimension (elements);
 *   - graph structure is CSR over TARGET rows with int32 indices:
 *       rowptr[n_rows+1], col[nnz] = source node of each in-edge, val[nnz] = edge weight;
 *   - return value: 0 = ok, >0 = argument error (GD_E_*), <0 = -(hipError_t).
 *     Nothing throws; gd_last_error_string() describes the last failure of the calling thread.
 *   - re-entrant per stream.  Process-wide state is limited to: the thread-local error string; the opt-in
 *     gd_set_matrix_split() switch (initialised from the environment, read at launch time; leave it alone and every
 *     call is a pure function of its arguments); tuning knobs read ONCE from the environment at first use
 *     (GD_SPMM_GRID_CAP, GD_ROWS_GEMM_GRID, GD_ROWS_GEMM_QUEUE, GD_ROWS_GEMM_WS, GD_ROWS_GEMM_WS_MIN_ROWS); the lazily resolved RCCL entry points.
 */
#ifndef GNNDELETE_HIP_H
#define GNNDELETE_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GD_ABI_VERSION 9   /* 2: round-2 signatures (xcd_bounds, interleaved GAT edge values, tile conv, ...); 3: gd_set_matrix_split;
                              4: gd_spmm_csr_onepass_f32, gd_rows_gemm_wgrad_reduce_f32 (dw = NULL in the wgrad entries),
                                 gd_comm_* / gd_allreduce_f32 / gd_exchange_rows_f32, gd_segment_softmax_f32, gd_rowpair_dot_f32, gd_step_tail_f32;
                              5: gd_del_loss_bwd_wgrad_f32, multi-row items of gd_spmm_csr_onepass_f32;
                              6: gd_rows_gemm_ws_covers (weight-stationary form of the row GEMMs), gd_spmm_csr_rowgroup_f32;
                             7: gd_rgcn_wave_conv_f32 / gd_rgcn_wave_covers;
                             8: gd_build_source_hash (the library carries a stamp of the sources it was built from), gd_typed_wgrad_f32,
                                gd_typed_edge_dot_f32, gd_spmm_csr_onepass_aux_f32, gd_del1_loss_wgrad_f32; gd_rowtarget_mse_f32 accepts dz = NULL;
                                gd_agg_gemm_f32 and gd_spmm_csr_rowgroup_f32 removed (opt-in forms nobody defaulted);
                             9: gd_rows_gemm_accumulate_f32; gd_rows_gemm_select_f32 / gd_rows_gemm_dots_f32 run weight-stationary with a selector
                                AND an index list; the one-launch item kernels abort on a misaligned XCD range table instead of deadlocking;
                                gd_induced_subgraph, gd_batch_csr, gd_batch_loss_terms (+ their _workspace queries): the GraphSAINT batch step;
                                gd_edgeprob_dec_f32, gd_edge_incidence (+ their _workspace queries), gd_rows_add_f32, gd_edgeprob_record_f32:
                                the fused edge-probability step (entries added, none changed: the version stays);
                                gd_rowfold_loss_f32 (+ _blocks), gd_rowfold_kld_scale_f32: the folded KLD / cosine row losses (entries added: the version stays);
                                gd_edge_bce_f32, gd_col_sum_f32 (+ their _workspace queries): the fused backbone step (entries added: the version stays);
                                gd_row_nll_f32 (+ its _workspace query): the fused node-classification step (entries added: the version stays);
                                gd_spmm_csr_onepass_wide_f32: 64-float rows summed 16 rows per item on the matrix pipe (entry added: the version stays);
                                gd_spmm_csr_onepass_wide128_f32: the same at 128-float rows (entry added: the version stays);
                                gd_negative_edges: negative edges drawn on the device (entry added: the version stays);
                                gd_edge_incidence_fixed, gd_edge_incidence_update (+ their size queries): the incidence list when only
                                the tail of the decoded edges changes (entries added: the version stays);
                                gd_edgeprob_batch_loss_f32 (+ its _workspace query): the loss stage of the edge-probability GraphSAINT
                                batch step (entries added: the version stays);
                                gd_rank_counts_f32, gd_subset_rank_metrics (+ its _workspace query): resampled AUC / AP without the
                                batched sort (entries added: the version stays);
                                gd_eval_edge_scores_f32, gd_row_nll_eval_f32 (+ their _workspace queries): the per-validation scoring of
                                the prepared validation pass (entries added: the version stays);
                                gd_eval_triple_scores_f32 (+ its _workspace query): the same for the knowledge-graph trainers' DistMult
                                triples (entries added: the version stays);
                                gd_subset_rank_metrics_drawn, gd_subset_draw: the 500 validation subsets drawn inside the rank kernel
                                (entries added: the version stays);
                                gd_rows_gemm_select_chain_f32 (+ its _covers query): conv1's explicit rows formed inside conv2's Linear
                                (entries added: the version stays);
                                gd_induced_subgraph_typed, gd_batch_typed_csr (+ their _workspace queries): the knowledge-graph
                                GraphSAINT batch step (entries added: the version stays) */

enum {
  GD_OK = 0,
  GD_E_NULL = 1,      /* required pointer is NULL */
  GD_E_DIM = 2,       /* unsupported / inconsistent dimension */
  GD_E_ALIGN = 3,     /* pointer or leading dimension not 16-byte aligned where required */
  GD_E_WORKSPACE = 4  /* scratch buffer too small */
};

int gd_abi_version(void);
const char* gd_last_error_string(void);
/* sha256 (first 16 hex digits) over the kernel sources (the .hip, .h and .cpp files of csrc) and this header the library was BUILT from,
 * stamped at build time by the Makefile; gnndelete_amd/_lib.py refuses a library whose stamp differs from the sources next
 * to it (a stale .so travelling with newer sources).  Replaces nothing upstream. */
const char* gd_build_source_hash(void);

/* How the dense fp32 products of the row GEMMs are formed (process-wide switch; initial value from the environment
 * variable GD_MATRIX_SPLIT, else GD_MATRIX_SPLIT_DEFAULT):
 *   0  v_mfma_f32_32x32x2_f32 (the fp32 matrix instruction);
 *   6  (opt-in) every fp32 operand is the exact sum of three bf16 pieces; the product is formed from the six largest of
 *      the nine partial products on v_mfma_f32_32x32x16_bf16, each exact in fp32, accumulated in fp32 (the three left out
 *      are <= 2^-26 of the product): same fp32 inputs and outputs, error against an fp64 product not larger than the fp32
 *      instruction's (rows_gemm.hip; tests/test_kernels_gpu.py).  Used where d_in is 64 / 128 and d_out 96 / 128, and for 128 -> 64.
 * Operands are expected finite and below 2^127 (an infinity, or a value that rounds to one in bf16, turns into NaN where
 * the fp32 instruction would propagate the infinity).  The switch is read at launch time: a hipGraph keeps the kernels it was captured with.  gd_gemm_f32 follows it when k is
 * a multiple of 128.  Replaces nothing upstream (torch.mm on fp32 tensors, framework/models/deletion.py:27). */
#define GD_MATRIX_SPLIT_DEFAULT 0
int gd_matrix_split(void);
int gd_set_matrix_split(int n_products);

/* ---------------------------------------------------------------- message passing ----- */

/* COO -> CSR over TARGET rows, sources of a row ascending, multi-edges kept, ties in input order (stable).
 *   src, dst  [n_edges] int64 device arrays: the two rows of the reference's edge_index (flow source -> target)
 *   rowptr    [n_nodes + 1], col [n_edges] int32 out;  order [n_edges] int32 out or NULL: input position of
 *             the edge stored in CSR slot k
 *   status    device int32 out: 0, or 1 if any endpoint was outside [0, n_nodes) (outputs then undefined;
 *             the caller reads it when it next synchronises - no host sync in here)
 *   workspace >= gd_csr_from_coo_workspace(n_nodes, n_edges) bytes, 256-byte aligned
 * Replaces what torch_geometric re-derives from edge_index inside every conv call (framework/models/gcn.py:16-22,
 * gat.py:16-22, gin.py:26-34) and the sort + coalesce of to_undirected in the Df preprocessing
 * (delete_gnn.py:175-182).  Integer only: bit-exact, independent of the order the edges arrive in. */
int64_t gd_csr_from_coo_workspace(int32_t n_nodes, int64_t n_edges);
int gd_csr_from_coo(const int64_t* src, const int64_t* dst, int64_t n_edges, int32_t n_nodes, int32_t* rowptr,
                    int32_t* col, int32_t* order, int32_t* status, void* workspace, int64_t workspace_bytes,
                    void* stream);


/* GCN symmetric normalisation on a CSR that already contains exactly one self loop per node:
 *   val[k] = deg[i]^-1/2 * deg[col[k]]^-1/2,  deg[i] = rowptr[i+1]-rowptr[i]  (k in row i)
 * Replaces torch_geometric gcn_norm inside GCNConv.forward (framework/models/gcn.py:16,19). */
int gd_gcn_norm_f32(const int32_t* rowptr, const int32_t* col, int32_t n_rows, float* val, void* stream);

/* CSR SpMM / gather-scatter-add:
 *   y[i,:] = self_coef * x[i,:] + sum_{k in row i} (val ? val[k] : 1) * x[col[k],:] + (bias ? bias : 0)
 * d must be a multiple of 4, x/y/bias 16-byte aligned, ldx/ldy multiples of 4.
 * Replaces MessagePassing.propagate (gather + scatter_add) of GCNConv / GINConv
 * (framework/models/gcn.py:11-24, gin.py:11-12,26-34); with the transposed CSR it is the
 * backward of the same op. */
int gd_spmm_csr_f32(const int32_t* rowptr, const int32_t* col, const float* val,
                    const float* x, int64_t ldx, float* y, int64_t ldy, const float* bias,
                    float self_coef, int32_t n_rows, int32_t d, void* stream);

/* Load-balanced form of gd_spmm_csr_f32 for heavy-tailed graphs.  The CSR rows are pre-cut into
 * work items of at most 64 in-edges: items[4*i..] = {row, start, end, slot}; slot = -1 when the
 * item covers its whole row (y written directly), else the index of a d-float partial in
 * `scratch`.  split[4*i..] = {row, first_slot, n_slots, 0} lists the rows cut into several
 * items; their partials are added in slot order by a second kernel (no atomics: deterministic).
 * nnz = length of col/val (index loads are clamped to it instead of being predicated).  The clamp is to nnz - 1, so a
 * table of items over an index array WITHOUT entries has nothing to clamp to: n_items > 0 with nnz <= 0 is GD_E_DIM (no
 * launch) in this entry, in gd_spmm_csr_onepass_f32, gd_spmm_csr_onepass_wide_f32 (and its hosted form) and
 * gd_spmm_csr_onepass_aux_f32.  An edgeless aggregation is the caller's: y = self_coef * x_self + bias.
 * x_self (optional, same pitch ldx): the matrix the self_coef term is read from, y[i] += self_coef *
 * x_self[i,:]; NULL = x itself (GIN's (1+eps) x_i).  With another matrix (or other columns of the
 * same buffer) and self_coef = 1 it is SAGEConv's root path, out = mean_j(x_j W_l) + b + x_i W_r.
 * x_rows = an upper bound on the number of rows of x AND of y (every col id and every item row
 * is < x_rows); when both matrices are smaller than 4 GiB the kernel uses 32-bit row offsets
 * (pass 0 if unknown: 64-bit addressing).
 * xcd_bounds (optional, 9 ascending item indices, [0] = 0, [8] = n_items): the item range each of the 8 XCDs
 * sweeps; NULL = equal eighths.  A placement hint only (balances the bytes each XCD's L2 moves), never results.
 * Same arithmetic, same call sites as gd_spmm_csr_f32. */
int gd_spmm_csr_balanced_f32(const int32_t* items, int32_t n_items, const int32_t* split, int32_t n_split,
                             const int32_t* col, const float* val, const float* x, int64_t ldx,
                             float* y, int64_t ldy, const float* bias, float self_coef,
                             const float* x_self, float* scratch, int32_t d, int32_t nnz, int32_t x_rows,
                             const int32_t* xcd_bounds, void* stream);

/* One-launch form of gd_spmm_csr_balanced_f32 (same arithmetic, same call sites): no scratch rows, no fix-up kernel.
 *   items [n_items, 4], n_items a multiple of 4, in four flavours:
 *     {row, start, end, -1}  a row of at most 64 in-edges (one wave);
 *     {row, start, end, -2}  a GROUP member: a row above 64 in-edges is laid out as four consecutive items at a
 *                            4-aligned position, member w = the w-th contiguous share [start, end) of the row's
 *                            in-edges (shares are multiples of 64 edges, trailing shares may be empty); the block's
 *                            four waves take one member each, the four partial rows are added in LDS in member order and
 *                            written once - deterministic, no atomics;
 *     {-1, 0, 0, -1}         padding;
 *     {row, start, end, -(16 + v)}  MULTI-ROW: up to MAXR CONSECUTIVE light rows row .. row + nr - 1 whose in-edges
 *                            [start, end) are adjacent in the CSR and at most 64 together, summed in ONE visit of a wave (the
 *                            sweep is bound by dependent round trips per visit, not by bytes).  v = c1 | c2 << 7 | c3 << 14 |
 *                            (nr - 1) << 21, c_q = the number of edges of rows 0 .. q - 1 of the item; edge j of the item
 *                            belongs to row (j >= c1) + (j >= c2) + (j >= c3) (fields past nr - 1 are ignored).  MAXR follows
 *                            the width the kernel carries accumulators for: 1 (no such items) for d > 64, 2 for 33 .. 64,
 *                            4 for d <= 32; more rows than MAXR in an item is a caller error (the extra rows are not written).
 *                            A row's sum is associated by edge position in the ITEM: equal to fp32 rounding to its one-row form.
 *   xcd_bounds (required, 9 ascending item indices, all multiples of 4, [0] = 0, [8] = n_items): the item range each of
 *   the 8 XCDs sweeps.  Groups may sit anywhere in a range (the planner puts a range's hub rows first, heaviest first).
 *   INVARIANT (the caller's, SplitPlan.onepass keeps it by construction): every limit is a multiple of 4 and every group starts at
 *   a multiple of 4 - the four waves of a block then always hold one aligned quadruple of items, which is what makes the group
 *   path's block barriers uniform.  The table lives in device memory, so the entry cannot check it without a synchronisation;
 *   the KERNEL aborts the launch (trap -> hipErrorLaunchFailure at the next synchronisation) when a limit of its range is not a
 *   multiple of 4 instead of deadlocking.  The same holds for gd_spmm_csr_onepass_aux_f32 and the one-launch form of
 *   gd_gat_edge_grads_balanced_f32.
 * The sum of a hub row is associated differently from the balanced form's (piece partials in slot order), so the two
 * entries agree to fp32 rounding, not bit for bit; each is bit-reproducible run to run. */
int gd_spmm_csr_onepass_f32(const int32_t* items, int32_t n_items, const int32_t* col, const float* val,
                            const float* x, int64_t ldx, float* y, int64_t ldy, const float* bias, float self_coef,
                            const float* x_self, int32_t d, int32_t nnz, int32_t x_rows, const int32_t* xcd_bounds,
                            void* stream);

/* WIDE form of gd_spmm_csr_onepass_f32 for rows of exactly 64 floats (same arithmetic, same call sites): an item is up to 16
 * CONSECUTIVE light rows whose sums are formed by v_mfma_f32_16x16x4_f32 (Y[16 x 64] = S[16 x E] . X[E x 64], S = edge e's weight
 * in the row of the output row the edge belongs to), one visit of a wave per item.
 *   items [n_items, 4], n_items a multiple of 4:
 *     {row, start, end, -(16 + nr - 1)}  nr <= 16 rows row .. row + nr - 1 whose in-edges [start, end) are adjacent in the CSR and
 *                                        at most 64 together (rows without in-edges get bias + self term only);
 *     {row, start, end, -2}              GROUP member of a row above 64 in-edges, as for gd_spmm_csr_onepass_f32: same trips,
 *                                        same summation order, the same bits as that entry;
 *     {-1, 0, 0, -1}                     padding.
 *   col_tagged [nnz]: col[k] | local_row[k] << 24, local_row = the edge's row minus the first row of its item (0 for the
 *                     edges of group members and of rows outside the plan).  SplitPlan.onepass_wide builds the tags.
 *   d must be 64; x and y below 4 GiB with x_rows (an upper bound on the rows of x AND y) < 2^24 and pitches below 2^24 bytes.
 *   xcd_bounds and its INVARIANT as for gd_spmm_csr_onepass_f32 (the kernel aborts on a range limit that is no multiple of 4).
 * A row's sum is the fmaf chain over its own edges in item order, starting from the bias, + self_coef * x_self[row] at the end:
 * bit-reproducible, equal to fp32 rounding to the other forms.  NON-FINITE INPUTS: the matrix instruction multiplies every
 * gathered row into all 16 rows of the item (by 0 where the edge belongs to another row), so a source row that holds Inf or
 * NaN poisons every row of the items that gather it, not only its true neighbours. */
int gd_spmm_csr_onepass_wide_f32(const int32_t* items, int32_t n_items, const int32_t* col_tagged, const float* val,
                                 const float* x, int64_t ldx, float* y, int64_t ldy, const float* bias, float self_coef,
                                 const float* x_self, int32_t d, int32_t nnz, int32_t x_rows, const int32_t* xcd_bounds,
                                 void* stream);

/* The wide form for rows of exactly 128 floats (entry added: the version stays).  Arguments, checks, items, col_tagged and
 * xcd_bounds as for gd_spmm_csr_onepass_wide_f32 - the items and the row tags do not depend on the width - but d must be 128
 * (any other width: GD_E_DIM).  A trip of four edges loads two float4 per lane from one source row and issues eight matrix
 * instructions that share the one A value.  A GROUP member runs the vector path of gd_spmm_csr_onepass_f32 at d = 128 (two lane
 * groups of 32 lanes): same trips, same summation order, the same bits as that entry.  Every other row is the fmaf chain over its
 * own edges in item order, starting from the bias, + self_coef * x_self[row] at the end.  NON-FINITE INPUTS as above: a source row
 * that holds Inf or NaN poisons every row of the items that gather it (0 x Inf = NaN inside the instruction). */
int gd_spmm_csr_onepass_wide128_f32(const int32_t* items, int32_t n_items, const int32_t* col_tagged, const float* val,
                                    const float* x, int64_t ldx, float* y, int64_t ldy, const float* bias, float self_coef,
                                    const float* x_self, int32_t d, int32_t nnz, int32_t x_rows, const int32_t* xcd_bounds,
                                    void* stream);

/* gd_spmm_csr_onepass_f32 with the edge values read THROUGH a permutation from an interleaved (weight, addend) array kept in
 * another edge order (ABI 8): w[k] = aux[2 perm[k]], and aux_sum[row] = the sum of aux[2 perm[k] + 1] over the row's entries
 * (fixed order).  GATConv's backward forms the attention weights and the logit gradients per edge in TARGET-major order and
 * needs them SOURCE-major for the message gradient dh = A_alpha^T dy and for d a_src: this entry is that aggregation, the
 * transposition pass (gd_gat_transpose_edges_f32) disappears into it.  d in {64, 128}; x and y below 4 GiB with row ids /
 * pitches below 2^24; no bias / self term; items / xcd_bounds as for gd_spmm_csr_onepass_f32 (rows per item <= 2).
 * Replaces the index_select / scatter chain of torch_geometric's GATConv backward (framework/models/gat.py:11-24). */
int gd_spmm_csr_onepass_aux_f32(const int32_t* items, int32_t n_items, const int32_t* col, const int32_t* perm, const float* aux,
                                const float* x, int64_t ldx, float* y, int64_t ldy, float* aux_sum, int32_t d, int32_t nnz,
                                int32_t x_rows, const int32_t* xcd_bounds, void* stream);


/* Per-relation mean aggregation of R-GCN ("typed SpMM") over a relation-major CSR:
 *   rowptr[(r*n_rows + i) .. +1] delimit the in-edges of type r into node i;
 *   y[r][i,:] = mean_{k} x[col[k],:]   (0 when the segment is empty),  y is [R, n_rows, ldy].
 * Replaces the relation loop of RGCNConv.forward (framework/models/rgcn.py:17-22,31-33). */
int gd_rgcn_mean_f32(const int32_t* rowptr, const int32_t* col, const float* x, int64_t ldx,
                     float* y, int64_t ldy, int32_t n_rel, int32_t n_rows, int32_t d, void* stream);

/* GAT (heads=1) fused edge-softmax aggregation over a CSR with one self loop per node:
 *   e_k = LeakyReLU(a_src[col[k]] + a_dst[i], slope); alpha = softmax_k(e) (denominator + 1e-16)
 *   y[i,:] = sum_k alpha_k h[col[k],:] + bias;  alpha (nnz floats, optional) is kept for backward.
 * Replaces GATConv.forward's gather/leaky_relu/softmax/scatter chain (framework/models/gat.py:11-24). */
int gd_gat_aggregate_f32(const int32_t* rowptr, const int32_t* col, const float* a_src, const float* a_dst,
                         const float* h, int64_t ldh, float* y, int64_t ldy, const float* bias,
                         float* alpha_out, float slope, int32_t n_rows, int32_t d, void* stream);

/* Backward of gd_gat_aggregate_f32 w.r.t. h (message path), a_src and a_dst, given dy.
 *   rowptr/col/alpha: forward CSR (target-major) and its saved attention;
 *   rowptr_t/col_t/perm_t: the transposed CSR (source-major) and, per transposed entry, the
 *   index of the same edge in the forward CSR.
 * Outputs: dh [n,d] (message path only), da_src[n], da_dst[n]; scratch de[nnz]. */
int gd_gat_aggregate_bwd_f32(const int32_t* rowptr, const int32_t* col, const float* alpha,
                             const int32_t* rowptr_t, const int32_t* col_t, const int32_t* perm_t,
                             const float* a_src, const float* a_dst, const float* h, int64_t ldh,
                             const float* dy, int64_t lddy, float* dh, int64_t lddh,
                             float* da_src, float* da_dst, float* de, float slope,
                             int32_t n_rows, int32_t d, void* stream);

/* Load-balanced forms of the two GAT entries over the work items of gd_spmm_csr_balanced_f32
 * (<= 64 in-edges per item, hub rows spread over many waves).  Forward: every item computes a
 * local softmax, the items of a split row are merged flash-attention style; instead of the
 * per-edge attention it returns the row statistics rowmax[n] / rowsum[n] (alpha_k =
 * exp(e_k - rowmax_i) / (rowsum_i + 1e-16)).  d must be a power of two in [4, 1024];
 * scratch: gd_gat_balanced_scratch(n_slots, d) floats.
 * gd_gat_edge_grads_balanced_f32 is the target-major half of the backward: ade[nnz][2] = per edge
 * (alpha rebuilt, d loss / d score) interleaved - the source-major half gathers both through the edge
 * permutation, one sector per edge this way -, da_dst[n]; t_row[n] and scratch (n_slots floats) are work
 * space.  The source-major half (dh = sum alpha dy, da_src = sum de) is gd_gat_transpose_edges_f32 +
 * gd_spmm_csr_balanced_f32 on the transposed CSR with val = alpha_t. 
 * gd_gat_edge_grads_balanced_f32 with xcd_bounds (ABI 8; NULL = the piece form above): `items` are then the ONE-LAUNCH items of
 * SplitPlan.onepass(d, multirow=1) - slot -1 = a whole row, slot -2 = member of a group (a hub row as four consecutive,
 * 4-aligned items, one share per wave of a block), row -1 = padding - with the nine item-range limits of the eight XCDs; split
 * must be empty: the members sum the row's t in LDS and each finishes the score gradients of its own edges - no second edge
 * pass, no fix-up launches.  (The forward keeps the piece form: its kernel runs at 64 registers / eight waves per SIMD and a
 * member path with several chunks spills there - measured +200 us on the GAT step, NOTES round 5.) */
int64_t gd_gat_balanced_scratch(int32_t n_slots, int32_t d);
int gd_gat_aggregate_balanced_f32(const int32_t* items, int32_t n_items, const int32_t* split, int32_t n_split,
                                  int32_t n_slots, const int32_t* col, const float* a_src, const float* a_dst,
                                  const float* h, int64_t ldh, float* y, int64_t ldy, const float* bias,
                                  float* rowmax, float* rowsum, float* scratch, float slope,
                                  int32_t d, int32_t nnz, int32_t h_rows /* rows of h, 0 = unknown */, void* stream);
int gd_gat_edge_grads_balanced_f32(const int32_t* items, int32_t n_items, const int32_t* split, int32_t n_split,
                                   const int32_t* col, const float* a_src, const float* a_dst,
                                   const float* rowmax, const float* rowsum, const float* h, int64_t ldh,
                                   const float* dy, int64_t lddy, float* ade, float* da_dst,
                                   float* t_row, float* scratch, float slope, int32_t d, int32_t nnz, const int32_t* xcd_bounds,
        void* stream);

/* GAT attention logits: a1[i] = <h[i,:], v1>, a2[i] = <h[i,:], v2> in one pass over h
 * (alpha_src / alpha_dst of GATConv.forward, framework/models/gat.py:11-12). */
int gd_row_dots_f32(const float* h, int64_t ldh, int32_t n, int32_t d, const float* v1, const float* v2,
                    float* a1, float* a2, void* stream);

/* out[i] = sum of x[perm ? perm[k] : k] over k in [rowptr[i], rowptr[i+1]) - deterministic
 * segment sum (the da_src reduction of the GAT backward). */
int gd_segment_sum_f32(const int32_t* rowptr, const int32_t* perm, const float* x, int32_t n, float* out,
                       void* stream);

/* y[i,:] += a[i] * u[:] + b[i] * v[:]  (d % 4 == 0): the gradient that reaches GATConv's linear output
 * through the attention logits alpha_src = <h, att_src>, alpha_dst = <h, att_dst> (gat.py:11-12 /
 * PyG GATConv), both rank-1 terms in one pass. */
int gd_rank1_add2_f32(float* y, int64_t ldy, int32_t n, int32_t d, const float* a, const float* u,
                      const float* b, const float* v, void* stream);

/* GAT backward, edge quantities moved to the transposed (source-major) edge order in one pass:
 * alpha_t[k] = ade[perm[k]][0] (weights of the transposed SpMM that forms dh) and
 * da_src[j] = sum_{k in source row j} ade[perm[k]][1] (gradient of alpha_src); perm = position of
 * transposed edge k in the forward CSR; ade as written by gd_gat_edge_grads_balanced_f32. */
int gd_gat_transpose_edges_f32(const int32_t* rowptr_t, const int32_t* perm, const float* ade, int32_t n,
                               float* alpha_t, float* da_src, void* stream);

/* Fused R-GCN message passing (PyG RGCNConv aggr='mean', framework/models/rgcn.py:16-38) for constant
 * relation weights - no [R, N, d] per-relation aggregate is formed:
 *     y[i,:] += sum over the (i, r) runs of node i:  ( sum_{e in run} w[e] * x[col[e],:] ) @ W_r
 * Node-major typed graph: node_ptr[n+1] indexes the runs of a node, seg_ptr[S+1] the edges of a run,
 * seg_rel[S] its relation; col/w per edge (forward: w = 1/|run|).  weight = [R, n_blocks, ib, ob]
 * (n_blocks = 1: dense [R, d_in, d_out]).  trans != 0 multiplies by W_r^T instead (input gradient on the
 * transposed graph; then d_in is the forward d_out and vice versa).  y must hold the root/bias term (or
 * zeros) on entry; d_in, d_out <= 128.  Replaces the per-relation masked propagate + einsum loop. */
int gd_rgcn_conv_f32(const int32_t* node_ptr, const int32_t* seg_ptr, const int32_t* seg_rel,
                     const int32_t* col, const float* w, const float* x, int64_t ldx, int32_t d_in,
                     const float* weight, int32_t n_blocks, int32_t trans,
                     float* y, int64_t ldy, int32_t d_out, int32_t n_nodes, void* stream);

/* The same conv regrouped by (64-node tile, relation) so that a relation weight is fetched once per tile instead
 * of once per (node, relation) run, with the tile's outputs held in LDS across all relations
 * (csrc/rgcn_tile.hip).  Supported: d_in, d_out in {64, 128}; weight = [R, 4, ib, ob] (the reference's num_blocks = 4,
 * framework/models/rgcn.py:17-22) or dense [R, 1, d_in, d_out]; gd_rgcn_tile_kl() returns the k range per wave (0 =
 * not supported: use gd_rgcn_conv_f32).
 *
 * packed_w: gd_rgcn_pack_weight_f32(weight [R, n_blocks, ib, ob], ...) -> R * (d_out / 16) * (kl / 16) * 256 floats, the weight of
 * this direction in the lane order of the MFMA operand (trans != 0: W_r^T; d_in / d_out are those of the direction).
 *
 * Tile plan of a typed graph (node-major, every (node, relation) run cut into pieces of <= 16 edges; the k-th piece of
 * a run belongs to pass k): steps are the distinct (tile = node / 64, relation, pass) triples in ascending order,
 *     tile_step_ptr[n_tiles + 1]   steps of a tile              step_rel[S]        relation of a step
 *     step_piece_ptr[S + 1]        pieces of a step (at most 32; a crowded (tile, relation, pass) continues in the next step)
 *     piece[P][2]                  {first edge, (node % 64) | length << 8}, at most one piece per node and step
 *     col[E], w[E]                 source node and weight per edge, in (step, node % 64, source) order
 *     tile_order[n_tiles]          launch order of the tiles (most steps first) or NULL
 * Hubs (nodes with so many pieces that their tile would run long after the others): their pieces may be moved to SLICE
 * rows - row ids >= 64 ceil(n_nodes / 64) in extra tiles (n_tiles > ceil(n_nodes / 64)); slice row v writes row
 * v - 64 ceil(n_nodes / 64) of y_ext [(n_tiles - ceil(n_nodes / 64)) * 64, d_out], and y[hub_node[h]] += the rows
 * y_ext[hub_ptr[h] .. hub_ptr[h + 1]) in order afterwards.  n_hubs = 0 and NULLs when the plan has no slices.
 * y must hold the root / bias term (or zeros) on entry, as for gd_rgcn_conv_f32; relations are accumulated in
 * ascending order: bit-reproducible. */
int32_t gd_rgcn_tile_kl(int32_t d_in, int32_t d_out, int32_t n_blocks, int32_t trans);
int gd_rgcn_pack_weight_f32(const float* weight, int32_t n_rel, int32_t n_blocks, int32_t d_in, int32_t d_out,
                            int32_t trans, float* packed, void* stream);
int gd_rgcn_tile_conv_f32(const int32_t* tile_order, const int32_t* tile_step_ptr, const int32_t* step_rel,
                          const int32_t* step_piece_ptr, const int32_t* piece,
                          const int32_t* col, const float* w, int32_t n_tiles, const float* x, int64_t ldx,
                          int32_t d_in, const float* packed_w, int32_t n_blocks, int32_t trans, float* y, int64_t ldy,
                          int32_t d_out, int32_t n_nodes, const int32_t* hub_node, const int32_t* hub_ptr, int32_t n_hubs,
                          float* y_ext, void* stream);

/* The same conv for the reference's FOUR diagonal blocks (weight = [R, 4, ib, ob], framework/models/rgcn.py:17-22; d_in,
 * d_out in {64, 128}; gd_rgcn_wave_covers() = 1), wave-private form (csrc/rgcn_wave.hip): output block t of a node depends on
 * the input features [t d_in / 4, (t + 1) d_in / 4) only, so one WAVE owns (64-node tile, block t) - no block barrier, the
 * outputs of the job in a wave-private LDS accumulator, the next unit's gathers in flight while this one is multiplied.
 * packed_w as for gd_rgcn_tile_conv_f32 (gd_rgcn_pack_weight_f32 of the direction; the transposed direction is this entry
 * on the transposed plan with the transposed pack, d_in / d_out those of the direction).
 *
 * Unit plan of a typed graph (node-major; every (node, relation) run cut into pieces of <= 4 edges; the pieces of one
 * (tile = node / 64, relation), in (node, piece) order, 16 to a unit):
 *     tile_unit_ptr[n_tiles + 1]   units of a tile, relations ascending;  unit_rel[U + 1]   relation of a unit | s << 16, s = the
 *                                  OR of the slot flags of the unit (which steps of the same-node scan it needs)
 *     n_units = U; EVERY UNIT ARRAY HOLDS ONE MORE, EMPTY UNIT AT INDEX U (relation 0, slot words 0, all pairs unused):
 *                                  what the kernel's software pipeline runs on past the end of a tile
 *     unit_row[U + 1][16]          slot word: node % 64 | flags << 8 | last << 12 (0 for an unused slot).  The slots of one
 *                                  node inside a unit are consecutive; flag bit b = the slot 2^b to the left exists and holds
 *                                  the same node; last = no further slot of this node follows in the unit
 *     unit_edges[U + 1][16][4][2]  (source node, weight as float bits) per edge of a slot; unused pairs = (n_nodes, 0.0f)
 *     job_tile[n_tiles]            launch order of the tiles (most units first) or NULL
 * tile must be 64.  y must hold the root / bias term (or zeros) on entry; relations are accumulated in ascending order,
 * the slots of a node by a fixed scan tree: bit-reproducible. 
 * relu_in != 0 (ABI 8): the conv reads relu(x) - RGCN's second layer reads relu(z1) (framework/models/rgcn.py:36-37) - formed
 * where the gathered rows land instead of in a pass of its own over [n_nodes, d_in]. */
int32_t gd_rgcn_wave_covers(int32_t d_in, int32_t d_out, int32_t n_blocks);
int gd_rgcn_wave_conv_f32(const int32_t* job_tile, int32_t n_tiles, int32_t tile, const int32_t* tile_unit_ptr,
                          int32_t n_units, const int32_t* unit_rel, const int32_t* unit_edges, const int32_t* unit_row,
                          const float* x, int64_t ldx, int32_t d_in, const float* packed_w, int32_t n_blocks, float* y,
                          int64_t ldy, int32_t d_out, int32_t n_nodes, int32_t relu_in, void* stream);

/* Random walks for GraphSAINT mini-batches (torch_geometric GraphSAINTRandomWalkSampler / torch_sparse random_walk as
 * used at framework/trainer/gnndelete_nodeemb.py:379-381, :734-736): out[s * n_walks + w] = node of walker w after s
 * steps (s = 0: start[w]); a step draws one out-neighbour of the current node uniformly from the CSR over SOURCE rows
 * (rowptr / col), a node without out-edges keeps the walker.  The draw is a hash of (seed, w, s): reproducible. */
int gd_random_walk(const int32_t* rowptr, const int32_t* col, int32_t n_nodes, const int64_t* start, int32_t n_walks,
                   int32_t walk_length, uint64_t seed, int64_t* out, void* stream);

/* Negative edges on the device (csrc/negatives.hip): out[i], out[ld_out + i] for i < n_out is a node pair
 * (a, b) with a != b and a * n_nodes + b NOT among pos_keys (framework/graph_utils.positive_edge_keys: sorted ascending,
 * unique, int64; NULL with n_keys == 0: only self loops are excluded), uniform over all such pairs and independent per slot -
 * negative_sampling's contract; duplicates among the negatives are possible, as in the host sampler.  A PURE FUNCTION of its
 * arguments: slot i depends on (seed, *counter, i, pos_keys, n_nodes) only - not on n_out, the launch geometry or another
 * slot; no generator state, no atomics, nothing to read back.  counter: a device scalar that is READ, never written (NULL =
 * 0): a caller that advances it on the stream gets another draw per epoch without a word from the host.  The stream (mix64 = the splitmix64 finaliser, mulhi64 = the
 * upper 64 bits of the 128-bit product):
 *     base = mix64(seed ^ mix64(counter))
 *     try t < 64:  c = mulhi64(mix64(base + 64 i + t), n_nodes^2);  accepted unless c / n == c % n or c is a key
 *     after 64 rejected tries:  c <- (c + 1) mod n_nodes^2, at most n_nodes^2 times, until accepted
 * mulhi64 maps 2^64 values onto n^2 cells: a cell's probability is off by at most n^2 / 2^64 relative (3e-9 at 235,868
 * nodes).  Every loop is bounded: 2 (n_keys + n_nodes) <= n_nodes^2 is required (at most half of all pairs excluded;
 * GD_E_DIM otherwise, as for n_nodes >= 2^31), so a try fails with probability <= 1/2, the probe is reached with
 * probability <= 2^-64 per slot and ends because an allowed pair exists.  n_out == 0: GD_OK, no launch.  ld_out >= n_out;
 * columns at and beyond n_out are not written.  One launch, one thread per slot, no runtime call besides it.
 * gnndelete_amd/negatives.reference_draw restates the stream on the CPU bit for bit. */
int gd_negative_edges(const int64_t* pos_keys, int64_t n_keys, int64_t n_nodes, uint64_t seed, const int64_t* counter,
                      int64_t n_out, int64_t* out, int64_t ld_out, void* stream);

/* Resampled ROC-AUC / average precision without a [B, 2k] sort (csrc/rankeval.hip; gnndelete_amd/rankeval.py holds the wrapper
 * and the numpy restatement).  Every subset ranks the same n_ref negatives (`ref`, label 0) against k positives taken from one
 * pool of m scores (label 1) through a row of pool indices that are DISTINCT WITHIN THE ROW.
 *
 * gd_rank_counts_f32: for each of m query scores, less[i] = the number of ref scores below it and leq[i] = the number at or
 * below it (numpy.searchsorted left / right) as int32; ref [n_ref] ASCENDING, 1 <= n_ref < 2^31, 0 <= m < 2^31 (GD_E_DIM
 * otherwise).  Two bounded binary searches per thread; a NaN query gives 0 / 0.  m == 0: GD_OK, no launch.
 *
 * gd_subset_rank_metrics: with the pool sorted DESCENDING, by sorted position p (int32 [m] each):
 *     u2[p] = less + leq of the score at p,   ge_at[p] = n_ref - less,   run_end[p] = the last position with the same score
 * and pos[e] = the sorted position of pool element e (int32 [m]); idx: int64, row b at idx + b * ld_idx, k indices in [0, m).
 *     auc[b] = double(sum over the row of u2[pos[e]]) / (2 k n_ref)                         (int64 sum: exact)
 *     ap[b]  = (1 / k) sum over the row's positions p of TP(p) / (TP(p) + ge_at[p]),  TP(p) = the row's members at positions
 *              <= run_end[p]                                                                (float64)
 * - sklearn's roc_auc_score (bit-equal to framework/metrics.batched_roc_auc) and average_precision_score (the recall step of a
 * run of equal scores spread over the run's members: the last bits differ from a sum over thresholds).  auc, ap: float64
 * [n_sub].  1 <= k <= m < 2^31, 1 <= n_ref < 2^30, 0 <= n_sub < 2^31, ld_idx >= k (GD_E_DIM otherwise); n_sub == 0: GD_OK, no
 * launch.  workspace: gd_subset_rank_workspace(n_sub, m) BYTES (-1: sizes out of range), 16-byte aligned; its content on
 * entry does not matter (each block zeroes its own rows: no memset call).  One launch, one block per subset; integer atomics
 * only, fixed reduction order: the same bits on every call.  Indices outside [0, m) in idx, pos or run_end are skipped or
 * clamped: a meaningless value, never an access outside the arrays. */
int gd_rank_counts_f32(const float* ref, int64_t n_ref, const float* query, int64_t m, int32_t* less, int32_t* leq, void* stream);
int64_t gd_subset_rank_workspace(int64_t n_sub, int64_t m);
int gd_subset_rank_metrics(const int32_t* u2, const int32_t* ge_at, const int32_t* run_end, const int32_t* pos, const int64_t* idx,
                           int64_t ld_idx, int64_t n_sub, int64_t k, int64_t m, int64_t n_ref, double* auc, double* ap,
                           void* workspace, int64_t workspace_bytes, void* stream);

/* The validation subsets drawn on the device (--device_subsets; csrc/rankeval.hip; gnndelete_amd/subsets.py holds the wrapper and
 * the numpy restatement).  They stand in for the draws of the reference's trainers - base.py:530-539, the knowledge-graph
 * trainer's 500 fresh torch.randperm(|Dr|)[:|Df|] per evaluation, and base.py:263-268, the link trainer's 500 drawn once per
 * request - with a counter-based stream of their own: subset b of draw `draw` under `seed` is the first k outputs of a keyed
 * permutation of [0, m), a pure function of (seed, draw, b, j, m) in integer operations, no generator state.  It is NOT the
 * reference's random stream.  With mix64 the splitmix64 finaliser and fmix32 the murmur3 32-bit finaliser
 * (h ^= h >> 16; h *= 0x85ebca6b; h ^= h >> 13; h *= 0xc2b2ae35; h ^= h >> 16):
 *     bits = max(6, bit_length(m - 1)) rounded up to even;  h = bits / 2;  mask = 2^h - 1
 *     base = mix64(seed ^ mix64(draw));  kb = mix64(base + b);  key[r] = the low 32 bits of mix64(kb + r),  r = 0 .. 11
 *     P(v):  L = v >> h, R = v & mask;  twelve times (L, R) <- (R, L ^ (fmix32(R ^ key[r]) & mask));  (L << h) | R
 *     e(b, j) = the first of P(j), P(P(j)), ... that is below m                       (cycle walking; uint32 throughout)
 * P is a bijection of [0, 2^bits) and the walk from j < m returns to j at the latest, so it ends (the loop is bounded by
 * 2^bits applications, never reached) and j -> e(b, j) is a bijection of [0, m): the k members of a subset are distinct.
 * 2^bits < 4 m: fewer than 4 applications per member on average.  32 <= m < 2^31 (below 32 the domain is too narrow for the
 * twelve rounds to mix: GD_E_DIM).
 *
 * gd_subset_rank_metrics_drawn: gd_subset_rank_metrics with (seed, draw) in place of (idx, ld_idx) - the same kernel, its
 * second phase computing member j of subset b instead of reading idx[b, j]; auc / ap are the bits gd_subset_rank_metrics
 * gives on the matrix gd_subset_draw writes.  Refuses m < 32; every other refusal, the workspace (gd_subset_rank_workspace)
 * and the guarantees are gd_subset_rank_metrics's own.  One launch; no index matrix is read or written.
 *
 * gd_subset_draw: out[b * ld_out + j] = e(b, j) for b < n_sub, j < k as int64; ld_out >= k, entries behind k are not written.
 * 0 <= n_sub < 2^31, 1 <= k <= m (GD_E_DIM otherwise); n_sub == 0: GD_OK, no launch.  One launch, one thread per member. */
int gd_subset_rank_metrics_drawn(const int32_t* u2, const int32_t* ge_at, const int32_t* run_end, const int32_t* pos, uint64_t seed,
                                 uint64_t draw, int64_t n_sub, int64_t k, int64_t m, int64_t n_ref, double* auc, double* ap,
                                 void* workspace, int64_t workspace_bytes, void* stream);
int gd_subset_draw(uint64_t seed, uint64_t draw, int64_t n_sub, int64_t k, int64_t m, int64_t* out, int64_t ld_out, void* stream);

/* The non-MSE row losses of the reference's loss zoo (framework/trainer/gnndelete_nodeemb.py:18-28), value per row
 * pair and gradient with respect to a, in one pass; rows of a / b optionally gathered through ia / ib (int64, NULL =
 * identity):
 *   kind 0  CosineDistance*:  val[r] = 1 - cos(a_r, b_r)  (each norm clamped at 1e-8 as F.cosine_similarity does)
 *   kind 1  BoundedKLD*:      val[r] = KL(softmax(b_r) || softmax(a_r)),  grad[r,:] = softmax(a_r) - softmax(b_r)
 * The caller reduces val over the rows (mean / sum; 1 - exp(-KL / n) for the bounded KLD) and scales grad. */
int gd_rowpair_loss_f32(int32_t kind, const float* a, int64_t ld_a, const int64_t* ia, const float* b, int64_t ld_b,
                        const int64_t* ib, int32_t n_rows, int32_t d, float* val, float* grad, int64_t ld_g, void* stream);

/* ---------------------------------------------------------------- Del operator --------- */

/* Row-subset GEMM on the fp32 matrix cores (v_mfma_f32_32x32x2_f32):
 *   for s in [0,n_sel):  r = idx ? idx[s] : s
 *       out[r,:] = act( in[r,:] ) @ (trans_w ? W^T : W)       W is [d_in, d_out] ([d_out, d_in] if trans_w)
 *   save_in (optional, compact [n_sel, d_in]) receives the gathered input rows (for the weight
 *   gradient); `in` and `out` may alias (rows are fully read before they are written) when
 *   d_in == d_out.  relu_in applies max(0,.) to the gathered rows first.
 *   bias (optional, [d_out]) is added.
 * With idx = S_Df node list and W = deletion_weight this is DeletionLayer.forward
 * (framework/models/deletion.py:17-29: clone + boolean gather + matmul + index_put); with
 * trans_w it is its input-gradient; with idx = NULL it is a dense Linear.
 * Two kernel forms, same results to fp32 rounding (the k order of the accumulation differs):
 *   - weight-stationary (rows_gemm_ws.hip, v_mfma_f32_16x16x4_f32): one wave per SIMD keeps W in its registers; taken
 *     where gd_rows_gemm_ws_covers() says so - widths in {64, 128}, >= 65,536 rows, no save_in (bias: plain calls only), out not
 *     aliasing in, fp32 products (GD_ROWS_GEMM_WS=0 in the environment turns it off);
 *   - LDS-operand (rows_gemm.hip): everything else, down to a scalar kernel for odd widths. */
int gd_rows_gemm_f32(const float* in, int64_t ld_in, const int32_t* idx, int32_t n_sel,
                     const float* w, int32_t d_in, int32_t d_out, int32_t trans_w,
                     const float* bias, int32_t relu_in,
                     float* out, int64_t ld_out, float* save_in, void* stream);

/* The gathering form of gd_rows_gemm_f32 with trans_w = 1:
 *   for s in [0,n_sel):  out[s,:] = act( in[idx[s],:] ) @ W^T (+ bias)       W is [d_out, d_in], `in` has n_in rows
 * out is COMPACT ([n_sel, d_out], pitch ld_out); idx is int64 (a batch's node list), may repeat ids and need not be sorted.
 * An id outside [0, n_in) reads nothing of `in` and gives a row of zeros (plus the bias).  This is layer 1 of a model
 * that trains on GraphSAINT batches: x[nodes] W1^T with the current W1, without a gathered copy of x.
 * The LDS-operand kernel of gd_rows_gemm_f32 under another row map (matrix-core forms and the scalar kernel for odd
 * widths alike, never the weight-stationary form): the result equals, bit for bit, what that kernel gives on the
 * gathered copy of the rows.  One launch; nothing beyond column d_out or row n_sel of out is written.
 * n_sel == 0: GD_OK, no launch.  in == out: GD_E_DIM (rows are read while other rows are written).  n_in above 2^31 - 1,
 * or no row at all with n_sel > 0: GD_E_DIM.  Widths and pitches: those of gd_rows_gemm_f32. */
int gd_rows_gather_gemm_f32(const float* in, int64_t ld_in, int64_t n_in, const int64_t* idx, int32_t n_sel,
                            const float* w, int32_t d_in, int32_t d_out, const float* bias, int32_t relu_in,
                            float* out, int64_t ld_out, void* stream);

/* gd_rows_gemm_f32 over a matrix whose rows live in two buffers of the same shape: row r is read from
 * in_alt where sel[r] != 0 and from in otherwise (e.g. z1 = Del-1 output on the S_Df rows, conv1 output
 * elsewhere: deletion.py:17-29 clones the whole matrix to get this; here neither copy is made). */
int gd_rows_gemm_ws_covers(int32_t n_sel, int32_t d_in, int32_t d_out);   /* 1: plain / sign / gate calls of this size run weight-stationary */

int gd_rows_gemm_select_f32(const float* in, const float* in_alt, const uint8_t* sel, int64_t ld_in,
                            const int32_t* idx, int32_t n_sel, const float* w, int32_t d_in, int32_t d_out,
                            int32_t trans_w, const float* bias, int32_t relu_in,
                            float* out, int64_t ld_out, void* stream);

/* conv2's Linear over a layer-1 output of which only the Del-1 rows exist (the step with conv1's weight folded into W_D1), in
 * one weight-stationary launch:
 *   listed row   r = idx_list[s]:  out[r,:] = relu(z[r,:]) @ W2                 - bit-equal to gd_rows_gemm_select_f32 on that row
 *   explicit row r = idx_expl[s]:  h = a[r,:] @ W1 + b1, pre[r,:] = h, out[r,:] = relu(h) @ W2
 * (the second product takes the first one's accumulators: h is stored for whoever reads conv1's output, never read back).
 * W1 [d_in, d_hid] and W2 [d_hid, d_out] are k-major ([k][n]: a Linear's weight transposed); the two lists are disjoint and
 * sorted; every pitch is a multiple of 4 floats, every buffer 16-byte aligned, out / pre alias nothing.  Only where
 * gd_rows_gemm_select_chain_covers holds: 128 -> 128 -> 64, n_expl > 0, n_list + n_expl >= 65,536 (the weight-stationary range),
 * no split arithmetic; GD_E_DIM otherwise (the caller then keeps gd_rows_gemm_f32 + gd_rows_gemm_select_f32). */
int gd_rows_gemm_select_chain_covers(int32_t n_list, int32_t n_expl, int32_t d_in, int32_t d_hid, int32_t d_out);
int gd_rows_gemm_select_chain_f32(const float* a, int64_t ld_a, const int32_t* idx_expl, int32_t n_expl, const float* w1,
                                  const float* b1, float* pre, int64_t ld_pre, const float* z, int64_t ld_z,
                                  const int32_t* idx_list, int32_t n_list, const float* w2, int32_t d_in, int32_t d_hid,
                                  int32_t d_out, float* out, int64_t ld_out, void* stream);

/* (ABI 9) out[r,:] += in[r,:] @ (trans_w ? W^T : W) for r = idx[s] or s, s < n_sel - the weight-stationary form with the
 * accumulators of a 16-row unit started from the rows of `out` (fetched a unit ahead).  GraphSAGE's root term: SAGEConv is
 * W_l mean_j x_j + b_l + W_r x_i (BASELINE config 3's model; the reference has no SAGE) - the aggregation writes the
 * neighbour term + bias, this call adds x W_r^T in place, in a matrix-bound kernel with memory to spare, instead of the
 * aggregation reading a second row stream (134 -> 104 us on the bench graph).  Only where gd_rows_gemm_ws_covers(n_sel, d_in,
 * d_out) holds (widths in {64, 128}, >= 65,536 rows), 16-byte aligned rows, in != out; GD_E_DIM otherwise (no other form exists:
 * callers below the threshold keep the aggregation's self-row operand). */
int gd_rows_gemm_accumulate_f32(const float* in, int64_t ld_in, const int32_t* idx, int32_t n_sel, const float* w, int32_t d_in,
                                int32_t d_out, int32_t trans_w, float* out, int64_t ld_out, void* stream);

/* Dense out = act(in or in_alt) @ W (+ bias) as gd_rows_gemm_select_f32 (sel / in_alt may be NULL), plus the two
 * row dot products o1[r] = <out[r,:], u1>, o2[r] = <out[r,:], u2> from the epilogue: GATConv's lin_src followed by
 * (x_src * att_src).sum(-1), (x_dst * att_dst).sum(-1) (framework/models/gat.py:11-12) without re-reading the rows
 * just written.  MFMA path only (d_in, d_out multiples of 32, d_out <= 128, weight <= 64 KB). */
int gd_rows_gemm_dots_f32(const float* in, const float* in_alt, const uint8_t* sel, int64_t ld_in, const float* w,
                          int32_t d_in, int32_t d_out, int32_t trans_w, const float* bias, int32_t relu_in, float* out,
                          int64_t ld_out, const int32_t* idx /* NULL = rows 0 .. n_rows-1, else the n_rows listed rows:
                          out / o1 / o2 are written at those row ids */, int32_t n_rows, const float* u1, const float* u2,
                          float* o1, float* o2, void* stream);

/* gd_rows_gemm_f32 that also emits the sign pattern of what it wrote, packed one bit per output
 * feature: sign_bits is compact [n_sel, ceil(d_out/32)] words, bit b of word k of entry s is set
 * iff out[idx[s], 32k + b] > 0.  With W = deletion_weight this is the ReLU gate of F.relu(x1)
 * (deletion.py:66-67) recorded while the Del output is still in registers. */
int gd_rows_gemm_signs_f32(const float* in, int64_t ld_in, const int32_t* idx, int32_t n_sel,
                           const float* w, int32_t d_in, int32_t d_out, int32_t trans_w,
                           const float* bias, int32_t relu_in,
                           float* out, int64_t ld_out, float* save_in, uint32_t* sign_bits, void* stream);

/* The product with the ReLU backward folded into its epilogue:
 *       out[r,n] = gate bit (s,n) ? (in[r,:] @ W)[n] : 0,   r = idx[s]
 * gate_bits: what gd_rows_gemm_signs_f32 wrote for the SAME idx list and d_out (input gradient of
 * `relu -> conv2.lin`, deletion.py:67-68: dh = (dt2 @ W2) * [z1 > 0]).  16 B of gate per row
 * instead of a second [n_sel, d_out] fp32 read. */
int gd_rows_gemm_gated_f32(const float* in, int64_t ld_in, const int32_t* idx, int32_t n_sel,
                           const float* w, int32_t d_in, int32_t d_out, int32_t trans_w,
                           const uint32_t* gate_bits, float* out, int64_t ld_out, void* stream);

/* The ReLU backward alone, on a row subset: out[r,:] = src[r,:] where the gate bit (s, n) is set, else 0, r = idx[s]
 * (gate_bits as written by gd_rows_gemm_signs_f32 for the same idx list; src may be out).  Used where the gradient that
 * has to be gated is a sum of several kernels' outputs (R-GCN: root product + typed conv). */
int gd_gate_rows_f32(const float* src, int64_t ld_src, const int32_t* idx, int32_t n_sel, const uint32_t* gate_bits,
                     int32_t d, float* out, int64_t ld_out, void* stream);

/* The same with a rank-2 correction of the product before the gate:
 *       out[r,n] = gate bit (s,n) ? (in[r,:] @ W)[n] + row_a[r] col_p[n] + row_b[r] col_q[n] : 0
 * GAT's input gradient dh2 = A_alpha^T dy + da_src (x) att_src + da_dst (x) att_dst (framework/models/gat.py through
 * PyG's GATConv) feeds this product; with col_p = att_src @ W, col_q = att_dst @ W (constants of a frozen
 * backbone) the rank-1 terms are added here, on the output side, and the separate pass over dh2 disappears.
 * MFMA widths only (d_in, d_out multiples of 32, d_out <= 128). */
int gd_rows_gemm_gated_rank1_f32(const float* in, int64_t ld_in, const int32_t* idx, int32_t n_sel,
                                 const float* w, int32_t d_in, int32_t d_out, int32_t trans_w,
                                 const uint32_t* gate_bits, const float* row_a, const float* col_p,
                                 const float* row_b, const float* col_q, float* out, int64_t ld_out, void* stream);

/* Weight gradient of the row-subset GEMM:  dW[d_a, d_b] (+)= sum_s a[ia(s),:]^T g[ig(s),:]
 *   ia(s) = a_idx ? a_idx[s] : s, likewise g_idx.  Deterministic split-K: `partials` must hold
 *   gd_rows_gemm_wgrad_workspace(n_sel, d_a, d_b) floats.  accumulate != 0 adds into dW.
 *   relu_mask (optional, same indexing as g through g_idx, ld = ld_g): g is multiplied by
 *   (relu_mask > 0) on the fly (backward through F.relu, deletion.py:67).
 *   g_add (optional, same indexing and ld as g): a second upstream gradient added row by row
 *   after the mask, dW = a^T (mask(g) + g_add) - one pass over `a` for a weight that receives
 *   gradient from two losses (both_all / both_layerwise, gnndelete_nodeemb.py:215-262).
 *   dw = NULL (this entry and gd_rows_gemm_wgrad_loss_f32 with param = NULL): only the per-block partial products are
 *   written; gd_rows_gemm_wgrad_reduce_f32 adds them up later - on another stream if the caller orders it after this
 *   one - so that the launch-sized reduction leaves the step's critical path.
 * Replaces autograd's matmul backward for deletion_weight. */
int64_t gd_rows_gemm_wgrad_workspace(int32_t n_sel, int32_t d_a, int32_t d_b);
int gd_rows_gemm_wgrad_f32(const float* a, int64_t ld_a, const int32_t* a_idx,
                           const float* g, int64_t ld_g, const int32_t* g_idx,
                           const float* relu_mask, const float* g_add, int32_t n_sel, int32_t d_a,
                           int32_t d_b, float* dw, int32_t accumulate, float* partials, void* stream);

/* gd_rows_gemm_wgrad_f32 followed by torch.optim.Adam on `param` with the freshly reduced dW,
 * fused into the split-K reduction (t = *iter + 1; `iter` is a shared iteration counter that
 * gd_loss_finalize_f32 advances once per step). */
int gd_rows_gemm_wgrad_adam_f32(const float* a, int64_t ld_a, const int32_t* a_idx,
                                const float* g, int64_t ld_g, const int32_t* g_idx,
                                const float* relu_mask, const float* g_add, int32_t n_sel, int32_t d_a,
                                int32_t d_b, float* dw, int32_t accumulate, float* partials,
                                float* param, float* exp_avg, float* exp_avg_sq, const int32_t* iter,
                                double lr, double beta1, double beta2, double eps, void* stream);

/* The second half of the weight gradient on its own: dW (+)= sum of the gd_rows_gemm_wgrad_blocks(n_sel) partial
 * products a wgrad entry left in `partials` (called with dw = NULL, same n_sel / d_a / d_b), added in block order
 * (deterministic); param != NULL applies torch.optim.Adam with the reduced gradient in the same launch (t = *iter + 1). */
int gd_rows_gemm_wgrad_reduce_f32(const float* partials, int32_t n_sel, int32_t d_a, int32_t d_b, float* dw,
                                  int32_t accumulate, float* param, float* exp_avg, float* exp_avg_sq,
                                  const int32_t* iter, double lr, double beta1, double beta2, double eps, void* stream);

/* The launch-sized tail of a training step in ONE launch: gd_rows_gemm_wgrad_reduce_f32 (with Adam) for BOTH Del weights and
 * gd_loss_finalize_f32 (per-block loss partials of the two layers -> hist[*pos], ring position, iteration counter).  Weight k
 * (k = 1, 2): partials_k as left by a wgrad entry called with dw = NULL for n_sel_k rows of a [d_k, d_k] weight.  Same
 * summation orders, same Adam arithmetic as the separate entries (t = *iter + 1 for both updates).  `arrive`: one device int32,
 * zero before the first call, private to these calls - the blocks that update the weights check in on it after reading *iter,
 * the finalize block advances *iter when all have (no block reads a counter another block of the launch has already written).
 * Replaces, per iteration, optimizer[0].step(), optimizer[1].step() and the three .item() syncs of the logging block
 * (framework/trainer/gnndelete_nodeemb.py:232-262, 304-311). */
int gd_step_tail_f32(const float* partials1, int32_t n_sel1, int32_t d1, int32_t accumulate1, float* dw1, float* param1,
                     float* exp_avg1, float* exp_avg_sq1, const float* partials2, int32_t n_sel2, int32_t d2,
                     int32_t accumulate2, float* dw2, float* param2, float* exp_avg2, float* exp_avg_sq2, double lr,
                     double beta1, double beta2, double eps, const float* loss_partials1, int32_t n1,
                     const float* loss_partials2, int32_t n2, float* hist, int32_t capacity, int32_t* pos, int32_t* iter,
                     int32_t* arrive, void* stream);
/* (ABI 8) The same launch with the NUMBER OF PARTIAL MATRICES of each weight given instead of derived from a row count
 * (gd_del1_loss_wgrad_f32 leaves gd_del1_loss_wgrad_parts(n_sel) of them - one per compute unit - where the weight-gradient
 * entries leave gd_rows_gemm_wgrad_blocks(n_sel)): same summation order over the partials that exist. */
int gd_step_tail_parts_f32(const float* partials1, int32_t n_part1, int32_t d1, int32_t accumulate1, float* dw1, float* param1,
                           float* exp_avg1, float* exp_avg_sq1, const float* partials2, int32_t n_part2, int32_t d2,
                           int32_t accumulate2, float* dw2, float* param2, float* exp_avg2, float* exp_avg_sq2, double lr,
                           double beta1, double beta2, double eps, const float* loss_partials1, int32_t n1,
                           const float* loss_partials2, int32_t n2, float* hist, int32_t capacity, int32_t* pos, int32_t* iter,
                           int32_t* arrive, void* stream);

/* Weight gradient whose upstream gradient is FORMED while it is fetched, from the folded DEC + NI
 * row-target terms of that layer (see gd_rowtarget_mse_f32): for selected row s with loss slot
 * u = loss_slot[s] >= 0,  g_s = coef[u] * (z[z_idx[s],:] - tm[u,:]),  else 0;  then  + g_add.
 *     dW (+)= sum_s a[ia(s),:]^T g_s        loss_partials[2b], [2b+1] = per-block sums of
 *     cnt |z - tm|^2 over the DEC / NI slots (cnt_signed < 0 marks an NI slot),
 * b < gd_rows_gemm_wgrad_blocks(n_sel); reduce them with gd_loss_finalize_f32.  Replaces
 * gd_rowtarget_mse_f32 + gd_rows_gemm_wgrad_adam_f32 for a layer whose loss gradient feeds nothing
 * but its own Del weight (layer 1 with the backbone frozen): the [S, d] gradient is never written.
 * param != NULL applies Adam as gd_rows_gemm_wgrad_adam_f32 does.  Needs d_a, d_b in {32, 64, 128}. */
int32_t gd_rows_gemm_wgrad_blocks(int32_t n_sel);
int gd_rows_gemm_wgrad_loss_f32(const float* a, int64_t ld_a, const int32_t* a_idx,
                                const float* z, int64_t ld_z, const int32_t* z_idx,
                                const int32_t* loss_slot, const float* tm, const float* coef,
                                const float* cnt_signed, const float* g_add,
                                int32_t n_sel, int32_t d_a, int32_t d_b, float* dw, int32_t accumulate,
                                float* partials, float* loss_partials,
                                float* param, float* exp_avg, float* exp_avg_sq, const int32_t* iter,
                                double lr, double beta1, double beta2, double eps, void* stream);

/* Last-layer Del operator + its folded DEC/NI loss + its input gradient in one pass over the S_Df rows
 * (deletion.py:17-29 forward, gnndelete_nodeemb.py:196-210 loss, autograd's matmul backward):
 *     z = p[idx[s],:] @ W_D ;  dz[s,:] = coef[u] (z - tm[u,:]) (u = loss_slot[s] >= 0, else 0) ;
 *     dp[idx[s],:] = dz[s,:] @ W_D^T ;  loss_partials = per-block (DEC, NI) sums of cnt |z - tm|^2
 * for b < gd_del_loss_bwd_blocks(n_sel).  z is not written (no other consumer during training); dz is
 * compact [n_sel, d] for gd_rows_gemm_wgrad_f32.  d in {32, 64}; p, dz, dp must not alias. */
int32_t gd_del_loss_bwd_blocks(int32_t n_sel);
int gd_del_loss_bwd_f32(const float* p, int64_t ld_p, const int32_t* idx, int32_t n_sel, const float* w, int32_t d,
                        const int32_t* loss_slot, const float* tm, const float* coef, const float* cnt_signed,
                        float* dz, int64_t ld_dz, float* dp, int64_t ld_dp, float* loss_partials, void* stream);

/* The same pass + the Del weight's gradient (autograd's  p[idx,:]^T dz  for DeletionLayer.deletion_weight, deletion.py:17-29):
 *     wgrad_partials[b, :, :] (b < gd_rows_gemm_wgrad_blocks(n_sel), each [d, d] row-major) = per-block sums of p[idx[s],:]^T dz[s,:],
 * laid out and counted like the partials of gd_rows_gemm_wgrad_f32 (dw = NULL), so gd_rows_gemm_wgrad_reduce_f32 / gd_step_tail_f32
 * finish it (fixed order: bit-reproducible).  The launch has that many blocks, so loss_partials holds
 * 2 * gd_rows_gemm_wgrad_blocks(n_sel) floats here.  dz may be NULL (nothing else reads it once the gradient is formed here). */
int gd_del_loss_bwd_wgrad_f32(const float* p, int64_t ld_p, const int32_t* idx, int32_t n_sel, const float* w, int32_t d,
                              const int32_t* loss_slot, const float* tm, const float* coef, const float* cnt_signed,
                              float* dz, int64_t ld_dz, float* dp, int64_t ld_dp, float* loss_partials,
                              float* wgrad_partials, void* stream);
/* (ABI 8) The same with the number of partial slots to fill given: gd_del_loss_bwd_wgrad_parts(n_sel, d) (what the launch has
 * blocks for - one per compute unit in the weight-stationary form of d = 64 at >= 65,536 rows; reduce with
 * gd_step_tail_parts_f32) ... gd_rows_gemm_wgrad_blocks(n_sel); loss_partials holds 2 * n_part floats. */
int32_t gd_del_loss_bwd_wgrad_parts(int32_t n_sel, int32_t d);
int gd_del_loss_bwd_wgrad_parts_f32(const float* p, int64_t ld_p, const int32_t* idx, int32_t n_sel, const float* w, int32_t d,
                                    const int32_t* loss_slot, const float* tm, const float* coef, const float* cnt_signed,
                                    float* dz, int64_t ld_dz, float* dp, int64_t ld_dp, float* loss_partials,
                                    float* wgrad_partials, int32_t n_part, void* stream);
/* The same pass with the Del input gradient FOLDED into the next weight (the GCN / GIN chained step, where nothing reads dp but
 * dt = A^T dp and then (dt W_next) in gd_del1_chain_loss_wgrad_f32 - both linear, the gate behind them): no dp = dz W_D^T; instead
 *     g[idx[s],:] = dz[s,:]   (the rows dp would have gone to, pitch ld_g; other rows untouched)
 *     w_fold[64, h] = W_D^T @ w_next[64, h]   (row-major, contiguous, 16-byte aligned; one fmaf chain over c = 0..63 per output,
 *                                              from the W_D this launch reads: bit-reproducible)
 * so that (A^T g) w_fold = (A^T dp) w_next up to rounding.  loss_partials and wgrad_partials: the bits of
 * gd_del_loss_bwd_wgrad_parts_f32 on the same input, n_part as there.  gd_del_loss_fold_wgrad_covers(n_sel, d, h): 1 for d = 64,
 * h = 128 and >= 65,536 rows (the weight-stationary kernel's range; GD_DEL2_WS=0 turns it off); the entry refuses everything else. */
int32_t gd_del_loss_fold_wgrad_covers(int32_t n_sel, int32_t d, int32_t h);
int gd_del_loss_fold_wgrad_parts_f32(const float* p, int64_t ld_p, const int32_t* idx, int32_t n_sel, const float* w, int32_t d,
                                     const int32_t* loss_slot, const float* tm, const float* coef, const float* cnt_signed,
                                     float* g, int64_t ld_g, const float* w_next, int32_t h, float* w_fold,
                                     float* loss_partials, float* wgrad_partials, int32_t n_part, void* stream);

/* (ABI 8) FIRST-layer Del operator at d = 128, its folded loss and its weight gradient in one pass over the S_Df rows - what
 * gd_rows_gemm_signs_f32 followed by gd_rows_gemm_wgrad_loss_f32 (dw = NULL) compute in two (p read once, z only written):
 *     z[idx[s],:] = p[idx[s],:] @ W_D;   sign_out[s, 4] = packed [z > 0]  (the layout gd_rows_gemm_gated_f32 reads);
 *     g_s = coef[u] (z - tm[u,:]) for u = loss_slot[s] >= 0, else 0;   + g_add[idx[s],:] when g_add != NULL
 *     wgrad_partials[b] = block b's part of p[idx,:]^T g and loss_partials[2b], [2b+1] = its cnt |z - tm|^2 over the DEC / NI slots,
 *     b < n_part: the caller says how many partial slots it wants filled - gd_del1_loss_wgrad_parts(n_sel) (what the launch has
 *     blocks for: reduce with gd_step_tail_parts_f32) up to gd_rows_gemm_wgrad_blocks(n_sel) (slots beyond the launch's blocks are
 *     written as zeros, so that gd_rows_gemm_wgrad_reduce_f32 / gd_step_tail_f32, which count that many, finish it).
 * z must not alias p or g_add.  gd_del1_loss_wgrad_covers(n_sel, d): 1 where callers should prefer it (d = 128, launches of
 * >= 65,536 rows; GD_DEL1_FUSED=0 turns it off).  Replaces DeletionLayer.forward of deletion1 + the layer-1 terms of the loss
 * + autograd's deletion_weight gradient (framework/models/deletion.py:17-29, trainer/gnndelete_nodeemb.py:188-242). */
int32_t gd_del1_loss_wgrad_covers(int32_t n_sel, int32_t d);
int32_t gd_del1_loss_wgrad_parts(int32_t n_sel);
int gd_del1_loss_wgrad_f32(const float* p, int64_t ld_p, const int32_t* idx, int32_t n_sel, const float* w, int32_t d, float* z,
                           int64_t ld_z, uint32_t* sign_out, const int32_t* loss_slot, const float* tm, const float* coef,
                           const float* cnt_signed, const float* g_add, int64_t ld_gadd, float* loss_partials,
                           float* wgrad_partials, int32_t n_part, void* stream);
/* (ABI 8) The same pass with the second gradient stream FORMED in the kernel instead of read (the GCN / GIN layer-wise step, where it
 * is conv2's input gradient of the previous iteration):  g_add[idx[s],:] = (dt[idx[s], 0:64] @ w_next[64, 128]) (.) the sign
 * pattern sign_io[s, 4] holds when the call starts - i.e. the one the PREVIOUS call stored; the call then overwrites it with this
 * z's.  row_a / col_a / row_b / col_b (all four or none): row_a[idx[s]] col_a[:] + row_b[idx[s]] col_b[:] is added to the product
 * before the gate (GATConv's two rank-1 input-gradient terms).  Replaces gd_rows_gemm_gated_f32 / gd_rows_gemm_gated_rank1_f32 (+ its
 * [S, 128] write and read-back) in front of gd_del1_loss_wgrad_f32; d = 128, d_next = 64 only; sign_io 8-byte aligned. */
int gd_del1_chain_loss_wgrad_f32(const float* p, int64_t ld_p, const int32_t* idx, int32_t n_sel, const float* w, int32_t d, float* z,
                                 int64_t ld_z, uint32_t* sign_io, const int32_t* loss_slot, const float* tm, const float* coef,
                                 const float* cnt_signed, const float* dt, int64_t ld_dt, int32_t d_next, const float* w_next,
                                 const float* row_a, const float* col_a, const float* row_b, const float* col_b,
                                 float* loss_partials, float* wgrad_partials, int32_t n_part, void* stream);

/* The chained pass of a step whose FIRST conv's Linear is folded into W_D (GCN, F = H = 128): with a = A^ x (the aggregated inputs,
 * no bias), conv1's output is pre = a W1^T + 1 b1 and on the Del rows it is only read linearly, so
 *     z[idx[s],:] = a[idx[s],:] @ w_fold + bias_fold          w_fold = W1^T W_D [128, 128], bias_fold = b1 W_D [128]
 *     wgrad_partials_t[b][c][i] = block b's part of (a[idx,:]^T g)[i][c]      - TRANSPOSED [128][128] matrices
 *     colsum_partials[b][c]     = block b's part of (1^T g)[c] over its n_sel rows (nothing from the padding of the last 16-row unit)
 * so that dW_D = W1 (a^T g) + b1^T (1^T g) (gd_step_tail_fold1_f32 forms it).  g, sign_io, dt, w_next, the loss terms, the block
 * order and the zero filling of the slots b < n_part behind the launch's blocks: as gd_del1_chain_loss_wgrad_f32 without the rank-1
 * terms.  bias_fold 16-byte aligned; colsum_partials holds n_part * 128 floats.  gd_del1_chain_fold_covers(n_sel, d, h): 1 for
 * d = h = 128 where gd_del1_loss_wgrad_covers(n_sel, h) holds. */
int32_t gd_del1_chain_fold_covers(int32_t n_sel, int32_t d, int32_t h);
int gd_del1_chain_fold_loss_wgrad_f32(const float* a, int64_t ld_a, const int32_t* idx, int32_t n_sel, const float* w_fold,
                                      const float* bias_fold, int32_t d, float* z, int64_t ld_z, uint32_t* sign_io,
                                      const int32_t* loss_slot, const float* tm, const float* coef, const float* cnt_signed,
                                      const float* dt, int64_t ld_dt, int32_t d_next, const float* w_next, float* loss_partials,
                                      float* wgrad_partials_t, float* colsum_partials, int32_t n_part, void* stream);
/* w_fold = W1^T W_D and bias_fold = b1 W_D of that pass from scratch (W1 [128 out, 128 in] row-major, W_D [128, 128]); the
 * arithmetic gd_step_tail_fold1_f32 uses for the next step's pair. */
int gd_layer1_fold_f32(const float* w1, const float* b1, const float* wd, float* w_fold, float* bias_fold, void* stream);
/* gd_step_tail_parts_f32 for that step.  Weight 2, the loss finalize and the check-in protocol are unchanged.  Weight 1 (d1 = 128,
 * accumulate1 must be 0: GD_E_DIM otherwise) is finished per column c from the transposed partials and the column sums:
 *     G[:, c] = sum_b partials1_t[b][c][:],  s[c] = sum_b colsum1[b][c]  (fixed orders);   dw1[:, c] = W1 G[:, c] + b1 s[c];
 *     Adam on param1[:, c];   w_fold[:, c] = W1^T param1[:, c],  bias_fold[c] = b1 . param1[:, c]  from the UPDATED column. */
int gd_step_tail_fold1_f32(const float* partials1_t, const float* colsum1, int32_t n_part1, int32_t d1, int32_t accumulate1,
                           const float* w1, const float* b1, float* dw1, float* param1, float* exp_avg1, float* exp_avg_sq1,
                           float* w_fold, float* bias_fold, const float* partials2, int32_t n_part2, int32_t d2, int32_t accumulate2,
                           float* dw2, float* param2, float* exp_avg2, float* exp_avg_sq2, double lr, double beta1, double beta2,
                           double eps, const float* loss_partials1, int32_t n1, const float* loss_partials2, int32_t n2,
                           float* hist, int32_t capacity, int32_t* pos, int32_t* iter, int32_t* arrive, void* stream);
/* gd_spmm_csr_onepass_wide_f32 (its first 15 arguments, the same y bit for bit) whose launch also carries jobs of
 * gd_step_tail_fold1_f32 as extra blocks in front of the sweep (entry added: the ABI version stays).  The aggregation is
 * fabric-bound with eight small blocks per compute unit; a few hundred short blocks that start first disappear in it, and a step
 * that rides its tail on two such launches makes one launch less.
 *   job 1 (n_part1 > 0; d1 must be 128): weight 1 of gd_step_tail_fold1_f32 - dw1, Adam on param1, w_fold, bias_fold - with the
 *          step number *iter + 1.  w1_t: the transposed copy of w1 ([in][out], constant like w1).  *iter is only read.
 *   job 2 (n_part2 > 0; d2 a multiple of 4, at most 128): weight 2 of that entry with the step number *iter + 1, then the loss
 *          finalize: history row at *pos, *pos advanced modulo capacity, *iter advanced, *arrive back at 0 (it must be 0 at the
 *          launch).  No block waits for another: in a launch with job 2 every job block - of job 1 too, where the launch carries
 *          both - reads *iter first and adds 1 to *arrive when its work is done, and the finalize is run by whichever block's add
 *          comes last, so the counter advances only after every job block of the launch has read it.
 * n_part1 = 0 or n_part2 = 0 leaves that job out (its pointers are not read; job 1 alone touches neither *arrive nor the history);
 * both 0: GD_E_DIM.  Every output is bit-equal to gd_step_tail_fold1_f32's on the same inputs.  A launch with both jobs steps both
 * weights with the same step number.  A step that puts job 1 on one launch and job 2 on a LATER one of the same stream gets the
 * tail's result: job 1's launch has ended before job 2's launch advances *iter.  Nothing depends on the order in which the blocks
 * of a launch are dispatched.
 * n_items must be > 0 (GD_E_DIM: there is no launch to ride on). */
int gd_spmm_csr_onepass_wide_hosted_f32(
    const int32_t* items, int32_t n_items, const int32_t* col_tagged, const float* val, const float* x, int64_t ldx, float* y, int64_t ldy,
    const float* bias, float self_coef, const float* x_self, int32_t d, int32_t nnz, int32_t x_rows, const int32_t* xcd_bounds,
    const float* partials1_t, const float* colsum1, int32_t n_part1, int32_t d1, const float* w1, const float* w1_t, const float* b1,
    float* dw1, float* param1, float* exp_avg1, float* exp_avg_sq1, float* w_fold, float* bias_fold, const float* partials2,
    int32_t n_part2, int32_t d2, int32_t accumulate2, float* dw2, float* param2, float* exp_avg2, float* exp_avg_sq2, double lr,
    double beta1, double beta2, double eps, const float* loss_partials1, int32_t n1, const float* loss_partials2, int32_t n2, float* hist,
    int32_t capacity, int32_t* pos, int32_t* iter, int32_t* arrive, void* stream);

/* ---------------------------------------------------------------- losses --------------- */

/* Fused Deleted-Edge-Consistency + Neighborhood-Influence MSE terms of one layer, value and
 * gradient in one pass (framework/trainer/gnndelete_nodeemb.py:196-210 with nn.MSELoss).
 * Terms are grouped by the row of z they touch:
 *   for u in [0,n_seg): row = seg_row[u]; for t in [seg_ptr[u], seg_ptr[u+1]):
 *       diff = z[row,:] - o[term_o[t],:]
 *       sums[term_kind[t]] += |diff|^2                      (kind 0 = DEC, 1 = NI)
 *       dz[u or row,:] += 2 * term_w[t] * diff
 *   dz_compact != 0 -> dz is [n_seg, ld_dz] indexed by u, else [N, ld_dz] indexed by row
 *   (only the touched rows are written).  sums[2] must be zeroed by the caller; partial sums are
 *   reduced deterministically through `partials` (gd_rowpair_mse_workspace(n_seg) floats). */
int64_t gd_rowpair_mse_workspace(int32_t n_seg);
int gd_rowpair_mse_f32(const float* z, int64_t ld_z, const float* o, int64_t ld_o, int32_t d,
                       const int32_t* seg_ptr, const int32_t* seg_row, int32_t n_seg,
                       const int32_t* term_o, const float* term_w, const int32_t* term_kind,
                       float* dz, int64_t ld_dz, int32_t dz_compact,
                       float* sums, float* partials, void* stream);

/* Pre-folded form of the same losses for runs whose targets never change (full-batch training:
 * z_ori and the negatives are fixed outside the loop, gnndelete_nodeemb.py:177-185).  For every
 * touched row u (row_idx[u], ascending) the caller folds its terms once into the mean target
 * tm[u,:] (compact [n_rows, d]), cnt[u] = number of terms, coef[u] = 2 * w * cnt and a constant
 * K (sum_t |o_t|^2 - cnt |tbar|^2, added on the host):
 *       diff = z[row,:] - tm[u,:];  dz[row,:] = coef[u] * diff;  sums[kind[u]] += cnt[u] * |diff|^2
 * Pure streaming, deterministic; `partials` holds gd_rowtarget_mse_workspace(n_rows) floats;
 * sums[2] is accumulated into (zero it first).  row_idx need not be ascending.  dz = NULL: the loss sums only (rows whose
 * gradient feeds no trainable weight - the layer-1 DEC rows outside the Del-1 mask of a knowledge-graph request). */
int64_t gd_rowtarget_mse_workspace(int32_t n_rows);
int gd_rowtarget_mse_f32(const float* z, int64_t ld_z, const float* tm, int32_t d,
                         const int32_t* row_idx, const float* coef, const float* cnt, const int32_t* kind,
                         int32_t n_rows, float* dz, int64_t ld_dz, float* sums, float* partials, void* stream);
/* (ABI 8) Two such jobs of widths in {64, 128} in ONE launch (sums = NULL form: the per-block partials of each job go to its own
 * array, gd_rowtarget_mse_blocks(n_rows) pairs each): the two stand-alone loss launches a knowledge-graph step needs for its DEC
 * rows (layer 1: loss sums only, dz_a = NULL; layer 2: gradient rows written) are launch-sized on their own. */
int32_t gd_rowtarget_mse_pair_covers(int32_t d_a, int32_t d_b);
int gd_rowtarget_mse_pair_f32(const float* z_a, int64_t ld_z_a, const float* tm_a, int32_t d_a, const int32_t* row_idx_a,
                              const float* coef_a, const float* cnt_a, const int32_t* kind_a, int32_t n_rows_a, float* dz_a,
                              int64_t ld_dz_a, float* partials_a, const float* z_b, int64_t ld_z_b, const float* tm_b, int32_t d_b,
                              const int32_t* row_idx_b, const float* coef_b, const float* cnt_b, const int32_t* kind_b,
                              int32_t n_rows_b, float* dz_b, int64_t ld_dz_b, float* partials_b, void* stream);

/* End-of-step bookkeeping in one launch: reduce the per-block partials of the two layers' loss
 * kernels (called with sums = NULL; n1/n2 = gd_rowtarget_mse_blocks(n_rows)) in a fixed order,
 * add extra_sums[4] (optional), write (r1, l1, r2, l2) to hist[*pos], advance the ring position
 * (mod capacity) and the iteration counter *iter (the Adam step number source). */
int32_t gd_rowtarget_mse_blocks(int32_t n_rows);
int gd_loss_finalize_f32(const float* partials1, int32_t n1, const float* partials2, int32_t n2,
                         const float* extra_sums, float* hist, int32_t capacity, int32_t* pos, int32_t* iter,
                         void* stream);

/* The bounded-KLD and cosine-distance row losses of the loss zoo (see gd_rowpair_loss_f32) in the PRE-FOLDED form of
 * gd_rowtarget_mse_f32, for full-batch runs whose targets never change.  All terms t of a touched row u (row_idx[u], targets
 * o_t, cnt[u] = c of them, one kind per row: 0 = DEC, 1 = NI) are folded once by the caller, in fp64, into tm[u,:] ([n_rows, d]
 * compact); with z = z[row_idx[u], :]:
 *   family 0, cosine distance ((1 - cos(z, o)).mean() | .sum(), each norm clamped at 1e-8):   tm = U = sum_t o_t / max(|o_t|, 1e-8)
 *       sum_t (1 - cos(z, o_t)) = c - <z, U> / max(|z|, 1e-8)                                   added to the sum of kind[u]
 *       dz[row,:] = coef[u] * (-U / |z| + <z, U> z / |z|^3);  where |z| < 1e-8 the denominator is the constant: coef[u] * (-U / 1e-8)
 *       coef[u] = coef_kind / n_kind (n = number of terms of the kind for _mean, 1 for _sum): the gradient is final.
 *   family 1, bounded KLD (1 - exp(-kl_div(log_softmax(z), softmax(o), 'batchmean' | 'sum'))):   tm = T = sum_t softmax(o_t)
 *       sum_t KL(softmax(o_t) || softmax(z)) = K_u + c KL(T / c || softmax(z)),
 *           K_u = sum_t sum_j softmax(o_t)_j log softmax(o_t)_j - sum_j T_j log(T_j / c)  >= 0, a constant the caller keeps
 *           (summed per kind: KL_kind = K_kind + sum_kind; written this way both parts are non-negative and nothing cancels)
 *       c KL(T / c || softmax(z)) = sum_j T_j (log T_j - log c - log_softmax(z)_j)              added to the sum of kind[u]
 *       dz[row,:] = coef[u] * (c softmax(z) - T),  coef[u] = coef_kind;  d loss_kind / d z = exp(-KL_kind / n_kind) / n_kind times
 *       that, a scalar known only after the reduction: gd_rowfold_kld_scale_f32 multiplies it in (pass B).
 * Softmax (stable: the row maximum is subtracted; expf / logf in fp32), dots and norms run over the first d_valid <= d columns
 * only and dz is written as ZERO behind them (a class dimension padded with zero columns: a softmax over the padding would be
 * another function).  d in [4, 128], d % 4 == 0; z and dz are pitched (ld >= d, ld % 4 == 0), only the d columns of the touched
 * rows are written; row_idx need not be ascending.  partials: 2 floats per block (DEC, NI), gd_rowfold_loss_blocks(n_rows)
 * blocks, the layout gd_loss_finalize_f32 / gd_step_tail_parts_f32 reduce.  dz = NULL: the sums only.  One pass: z read once,
 * tm read once, dz written once; no atomics, the same bits every run. */
int32_t gd_rowfold_loss_blocks(int32_t n_rows);
int gd_rowfold_loss_f32(int32_t family, const float* z, int64_t ld_z, const float* tm, int32_t d, int32_t d_valid,
                        const int32_t* row_idx, const float* coef, const float* cnt, const int32_t* kind, int32_t n_rows,
                        float* dz, int64_t ld_dz, float* partials, void* stream);
/* Pass B of the bounded KLD, on the device (no host read, no float atomics), two launches: one block adds the n_blocks =
 * gd_rowfold_loss_blocks(n_rows) partial pairs of pass A up in a fixed order and stores
 *       scales[kind] = exp(-(sum_kind + k_kind) * inv_n_kind) * inv_n_kind     (k = K_kind above, inv_n = 1 / n_kind, or 0: no terms)
 * then a launch over the loss rows multiplies the d columns of dz[row_idx[u], :] by scales[kind[u]].  scales: 2 floats on the
 * device (required).  dz = NULL: the scalars only. */
int gd_rowfold_kld_scale_f32(const float* partials, int32_t n_blocks, float k_dec, float k_ni, float inv_n_dec, float inv_n_ni,
                             const int32_t* row_idx, const int32_t* kind, int32_t n_rows, int32_t d, float* dz, int64_t ld_dz,
                             float* scales, void* stream);

/* Dense transform with a reduction dimension of any width: out[row(s), :] = in[row(s), :] @ W (+ bias), s < n_rows,
 * row(s) = idx[s] or s; in [*, k] with k % 32 == 0 (zero-pad the columns of `in` and the rows of W), W [k, n] row-major
 * (= the TRANSPOSE of a torch Linear weight), n in {32, 64, 96, 128}.  The layer-1 transform x W1^T of the wide
 * bag-of-words inputs (framework/models/gcn.py:11-12, gat.py / gin.py alike; F = 1,639 / 8,710) - W is streamed
 * through LDS in 32-row chunks and the k range is split over several blocks per row group; `workspace` holds
 * gd_gemm_f32_workspace(n_rows, k, n) floats for their partial products (may be NULL when that is 0), which are
 * added in split order: deterministic.  Replaces torch's matmul -> rocBLAS on the path. */
int64_t gd_gemm_f32_workspace(int32_t n_rows, int32_t k, int32_t n);
int gd_gemm_f32(const float* in, int64_t ld_in, const int32_t* idx, int32_t n_rows, const float* w, int32_t k,
                int32_t n, const float* bias, float* out, int64_t ld_out, float* workspace, void* stream);

/* Link decoders.  dot: out[m] = <z[e0[m]], z[e1[m]]>  (framework/models/gcn.py:26-36);
 * distmult: out[m] = sum_c z[e0[m],c] * rel[etype[m],c] * z[e1[m],c]  (rgcn.py:40-47). */
int gd_edge_dot_f32(const float* z, int64_t ld_z, int32_t d, const int64_t* e0, const int64_t* e1,
                    const float* rel, int64_t ld_rel, const int64_t* etype,
                    int64_t n_edges, float* out, void* stream);

/* Input gradient of the decoders (autograd of gcn.py:26-36 / rgcn.py:40-47: two scatter-adds with atomics):
 *     dz[v,:] = sum_{k in [inc_ptr[v], inc_ptr[v+1])} w[k] * z[other[k],:]  (* rel[etype[k],:] for DistMult)
 * over a node-major incidence list of the decoded edges: for every edge m = (a, b) with upstream gradient dout[m] the
 * list of a holds (other = b, w = dout[m], etype = type of m) and the list of b holds (other = a, ...).  Every row of
 * dz is written (zeros where nothing is incident); incidences are added in list order, hubs (> 64 incidences) by the
 * whole wave in a fixed pattern: deterministic, no atomics.  d % 4 == 0, 16-byte aligned rows; dz must not alias z. */
int gd_edge_dot_bwd_f32(const float* z, int64_t ld_z, int32_t d, const int32_t* other, const float* w,
                        const float* rel, int64_t ld_rel, const int32_t* etype, const int64_t* inc_ptr,
                        int64_t n_nodes, float* dz, int64_t ld_dz, void* stream);

/* Edge-probability Neighborhood-Influence term of GNNDeleteTrainer
 * (framework/trainer/gnndelete.py:174-193 pair mask, :239-241 loss) over the n_s x n_s block of
 * 2-hop S_Df nodes, value and gradient in one pass, without forming z z^T:
 *     loss = inv_count * sum_{i>j, T[i][j] >= 0} (sigmoid(z[nodes[i]] . z[nodes[j]]) - T[i][j])^2
 *     dz[i,:] = d loss / d z[nodes[i],:]                      (compact [n_s, d])
 * target: [n_s, n_s] row-major (ld_t), only the strictly lower triangle is read; a negative entry
 * excludes the pair (the Df pairs, :186-190).  inv_count = 1 / number of included pairs.
 * workspace: gd_pairs_sigmoid_mse_workspace(n_s, d) floats.  Replaces the N x N `z @ z.t()`,
 * the N x N boolean mask indexing and their autograd backward. */
int64_t gd_pairs_sigmoid_mse_workspace(int32_t n_s, int32_t d);
int gd_pairs_sigmoid_mse_f32(const float* z, int64_t ld_z, const int32_t* nodes, int32_t n_s, int32_t d,
                             const float* target, int64_t ld_t, float inv_count,
                             float* loss, float* dz, float* workspace, void* stream);

/* ---------------------------------------------------------------- fused edge-probability step (csrc/edgeprob.hip) ---- */

/* DEC term of GNNDeleteTrainer.train_fullbatch (framework/trainer/gnndelete.py:221-233), value and logit gradients:
 *     a_k = <z[pos[0][k]], z[pos[1][k]]>,  b_k = <z[neg[0][k]], z[neg[1][k]]>,  diff_k = a_k - b_k        (k < m)
 *     loss[0] = (1/m) sum_k diff_k^2;   w[k] = coef * 2 * diff_k / m,  w[m + k] = -w[k]
 * i.e. w is d(coef * loss)/d(logit) of the 2m decoded edges in the decoder's [pos | neg] order.  pos / neg: int64
 * [2, m] with row pitches ld_pos / ld_neg (elements); an edge with an endpoint outside [0, n_nodes) counts as a zero dot
 * product (nothing outside z is read).  With src_edge / inc_ptr / w_inc (all three or none; from gd_edge_incidence over
 * the 2m edges [pos | neg] and n_nodes) the finishing launch also writes w_inc[k] = w[src_edge[k]] for every incidence
 * k < inc_ptr[n_nodes] - the order gd_edge_dot_bwd_f32 reads.  loss is summed in a fixed order (one partial per block,
 * added in block order by one thread; no float atomics): the same bits every call.  workspace:
 * gd_edgeprob_dec_workspace(m, d) floats.  d % 4 == 0, 16-byte aligned rows of z (GD_E_DIM / GD_E_ALIGN otherwise);
 * m == 0 is GD_E_DIM (upstream's MSE of nothing is NaN).  Two launches. */
int64_t gd_edgeprob_dec_workspace(int64_t m, int32_t d);
int gd_edgeprob_dec_f32(const float* z, int64_t ld_z, int64_t n_nodes, int32_t d, const int64_t* pos, int64_t ld_pos,
                        const int64_t* neg, int64_t ld_neg, int64_t m, float coef, float* w, float* loss,
                        const int32_t* src_edge, const int64_t* inc_ptr, float* w_inc, float* workspace, void* stream);

/* Node-major incidence list of n_edges edges (e0[k], e1[k]) over n_nodes nodes, as gd_edge_dot_bwd_f32 walks it:
 *     inc_ptr [n_nodes + 1] int64;  other [2 n_edges] int32 = the other endpoint;  src_edge [2 n_edges] int32 = the edge
 * in exactly the order of a STABLE sort of cat(e0, e1) by node id (entry p < n_edges is endpoint e0[p] of edge p, entry
 * p >= n_edges endpoint e1[p - n_edges] of edge p - n_edges) - what ops._EdgeDot.backward builds with torch.sort +
 * searchsorted.  Integer arithmetic only (a histogram, one scan, a fill and a rank pass); the result does not depend on
 * the order the integer atomics arrive in.  An edge with an endpoint outside [0, n_nodes) gets no entries (inc_ptr[n_nodes]
 * < 2 n_edges then; the tail of other / src_edge is not written).  workspace: gd_edge_incidence_workspace() BYTES. */
int64_t gd_edge_incidence_workspace(int64_t n_nodes, int64_t n_edges);
int gd_edge_incidence(const int64_t* e0, const int64_t* e1, int64_t n_edges, int64_t n_nodes, int64_t* inc_ptr,
                      int32_t* other, int32_t* src_edge, void* workspace, int64_t workspace_bytes, void* stream);

/* The same list when only the tail of the decoded edges changes between calls (csrc/incidence.hip): the edges are
 * [fixed | variable], n_fixed of them fixed (the positives), the rest rewritten every epoch (the negatives).  Node v's list in
 * the stable order is [fixed, e0 = v | variable, e0 = v | fixed, e1 = v | variable, e1 = v], each part by ascending edge index.
 *
 * gd_edge_incidence_fixed, once per request: from the edges [0, n_fixed) of (e0, e1), an IMAGE of gd_edge_incidence_fixed_bytes
 * (n_nodes, n_fixed) bytes - per node the fixed entries in stable order (source entries first), how many of them are source
 * entries, and the node of every entry.  workspace: gd_edge_incidence_update_workspace(n_nodes, n_fixed) BYTES.
 *
 * gd_edge_incidence_update, once per epoch: e0 / e1 are the WHOLE list of n_edges edges, of which only [n_fixed, n_edges) is
 * read; the image (of the same n_nodes and n_fixed, READ ONLY here) stands for the rest.  Writes exactly what gd_edge_incidence
 * (e0, e1, n_edges, n_nodes, ...) writes, bit for bit and the same bits every call: per epoch two integer counts per variable
 * edge, a scan over the nodes (three launches: sums per 1,024-node tile, one block over the tile sums, the tiles again), a
 * streaming copy of the fixed entries to their shifted places and a rank of each variable entry among its node's variable
 * entries of the same side (a list of L such entries costs L^2: slow when every variable edge meets one node, still exact).
 * gd_edge_incidence's contract in both halves: an edge with an endpoint outside [0, n_nodes) has no entries, the tail of other /
 * src_edge beyond inc_ptr[n_nodes] is not written; n_edges == n_fixed and n_fixed == 0 are legal.  workspace:
 * gd_edge_incidence_update_workspace(n_nodes, n_edges) BYTES; image and workspace 8-byte aligned (GD_E_ALIGN).
 *
 * Both are kernel launches on the stream and nothing else (no memset, no copy; the counters are zeroed by the first launch of
 * every call, so a count is never added to what an earlier call left), no block waits on another, every loop is bounded by an
 * argument, and every store is guarded by 2 n_edges. */
int64_t gd_edge_incidence_fixed_bytes(int64_t n_nodes, int64_t n_fixed);
int gd_edge_incidence_fixed(const int64_t* e0, const int64_t* e1, int64_t n_fixed, int64_t n_nodes, void* image, int64_t image_bytes,
                            void* workspace, int64_t workspace_bytes, void* stream);
int64_t gd_edge_incidence_update_workspace(int64_t n_nodes, int64_t n_edges);
int gd_edge_incidence_update(const void* image, const int64_t* e0, const int64_t* e1, int64_t n_fixed, int64_t n_edges,
                             int64_t n_nodes, int64_t* inc_ptr, int32_t* other, int32_t* src_edge, void* workspace,
                             int64_t workspace_bytes, void* stream);

/* dz[nodes[i], :] += scale * src[i, :] for i < n_s: the compact [n_s, d] pair-term gradient of
 * gd_pairs_sigmoid_mse_f32 joins a dense [n_rows, d] gradient.  nodes must be UNIQUE (plain vector loads and stores, no
 * atomics); rows outside [0, n_rows) are skipped.  d % 4 == 0, 16-byte aligned rows. */
int gd_rows_add_f32(float* dz, int64_t ld_dz, int64_t n_rows, const int32_t* nodes, int32_t n_s, const float* src,
                    int64_t ld_src, float scale, int32_t d, void* stream);

/* hist[*pos % capacity] = (coef_r * *loss_r + coef_l * *loss_l, *loss_l, *loss_r); ++*pos.  loss_l == NULL: 0.
 * hist: [capacity, 3] floats.  One thread; graph-capturable. */
int gd_edgeprob_record_f32(const float* loss_r, const float* loss_l, float coef_r, float coef_l, float* hist,
                           int32_t capacity, int32_t* pos, void* stream);

/* Loss stage of one GraphSAINT batch of the edge-probability mini-batch loop (GNNDeleteTrainer.train_minibatch,
 * framework/trainer/gnndelete.py:364-400), value and logit gradients of both terms:
 *     a_j = <z[pos[0][j]], z[pos[1][j]]>,  b_j = <z[neg[0][j]], z[neg[1][j]]>                               (j < k)
 *     loss_e = (1/k)   sum_j (a_j - b_j)^2
 *     loss_l = (1/n_l) sum_{c < n_cand: src_c < dst_c} (<z[src_c], z[dst_c]> - <z_ori[src_c], z_ori[dst_c]>)^2
 *     losses = (coef_e loss_e + coef_l loss_l, loss_e, loss_l)
 * The decoded list is [pos (k) | neg (k) | candidates (n_cand)]: dec, int64 [2, ld_dec] (ld_dec >= 2k + n_cand), receives
 * it with (-1, -1) in place of every candidate that does not count (src >= dst), and w [2k + n_cand] receives
 * d(coef_e loss_e + coef_l loss_l)/d(logit) in that order: w[j] = coef_e 2 (a_j - b_j) / k, w[k + j] = -w[j],
 * w[2k + c] = coef_l 2 diff_c / n_l, exactly 0 for a candidate that does not count.  z_ori is its own table (pitch ld_ori,
 * n_ori rows) read at the SAME ids as z.  n_l, the number of candidates with src < dst, is counted on the device in the
 * same pass (integers).  k == 0 makes loss_e (and losses[0]) NaN with no gradient from it, n_l == 0 does the same for
 * loss_l - F.mse_loss of nothing; neither is an error, and the other term's gradient is still written.  An endpoint
 * outside its table ([0, n_nodes) for z, [0, n_ori) for z_ori) makes that dot product 0; nothing outside the tables is
 * read.  With inc_ptr [n_nodes + 1] / other / src_edge / w_inc [2 (2k + n_cand)] / inc_workspace
 * (gd_edge_incidence_workspace(n_nodes, 2k + n_cand) bytes) - all five or none - the entry also runs gd_edge_incidence
 * over dec (a (-1, -1) edge gets no entries) and its finishing launch writes w_inc[i] = w[src_edge[i]] for every incidence
 * i < inc_ptr[n_nodes]: what gd_edge_dot_bwd_f32 reads.  One lane group per item, float4 per lane, both tables of a
 * candidate read by the same group; at most 2,048 blocks walk the items grid-strided, one partial per block, added in
 * block order by one thread (no float atomics): the same bits every call.  workspace:
 * gd_edgeprob_batch_loss_workspace(k, n_cand, d) floats (-1: sizes out of range).  d % 4 == 0, 16-byte aligned rows, any
 * row pitch that is a multiple of 4 (GD_E_DIM / GD_E_ALIGN otherwise).  Two launches around gd_edge_incidence's. */
int64_t gd_edgeprob_batch_loss_workspace(int64_t k, int64_t n_cand, int32_t d);
int gd_edgeprob_batch_loss_f32(const float* z, int64_t ld_z, int64_t n_nodes, const float* z_ori, int64_t ld_ori, int64_t n_ori,
                               int32_t d, const int64_t* pos, int64_t ld_pos, const int64_t* neg, int64_t ld_neg, int64_t k,
                               const int64_t* cand_src, const int64_t* cand_dst, int64_t n_cand, float coef_e, float coef_l,
                               int64_t* dec, int64_t ld_dec, float* w, float* losses, int64_t* inc_ptr, int32_t* other,
                               int32_t* src_edge, float* w_inc, void* inc_workspace, int64_t inc_workspace_bytes,
                               float* workspace, void* stream);

/* ---------------------------------------------------------------- fused backbone step (csrc/linkpred.hip) ---- */

/* Link-prediction loss of Trainer.train_fullbatch and RetrainTrainer.train_fullbatch (framework/trainer/base.py:75-142,
 * retrain.py:57-131), F.binary_cross_entropy_with_logits(decode(z, pos, neg), labels), value and logit gradients over the
 * M = n_pos + n_neg decoded edges in the decoder's [pos | neg] order:
 *     l_k = <z[a_k], z[b_k]>,   y_k = 1 for k < n_pos, else 0
 *     loss[0] = (1/M) sum_k ( max(l_k, 0) - l_k y_k + log1p(exp(-|l_k|)) )     (finite at every finite logit)
 *     w[k] = coef * (sigmoid(l_k) - y_k) / M                                   (formed as -sigmoid(-l) for y = 1: no 1 - 1)
 * pos: int64 [2, n_pos] with row pitch ld_pos (elements), neg likewise; either count may be 0 (its pointer may then be NULL),
 * M == 0 is GD_E_DIM.  An edge with an endpoint outside [0, n_nodes) reads nothing outside z and counts as a ZERO LOGIT: it
 * adds log 2 to the sum and gets w = coef * (0.5 - y) / M; gd_edge_incidence gives such an edge no entries, so that gradient
 * reaches no row.  With src_edge / inc_ptr / w_inc (all three or none; from gd_edge_incidence over the M edges [pos | neg] and
 * n_nodes) the finishing launch also writes w_inc[i] = w[src_edge[i]] for every incidence i < inc_ptr[n_nodes] - the order
 * gd_edge_dot_bwd_f32 reads.  One lane group per edge, float4 per lane; at most 2,048 blocks, which walk the edges
 * grid-strided; one partial per block, added in block order by one thread (no float atomics): the same bits every call.
 * workspace: gd_edge_bce_workspace(M, d) floats.  d % 4 == 0, 16-byte aligned rows of z (GD_E_DIM / GD_E_ALIGN otherwise).
 * Two launches.  Replaces the decoder's output, torch.cat of the labels, the loss and its autograd backward. */
int64_t gd_edge_bce_workspace(int64_t m_all, int32_t d);
int gd_edge_bce_f32(const float* z, int64_t ld_z, int64_t n_nodes, int32_t d, const int64_t* pos, int64_t ld_pos, int64_t n_pos,
                    const int64_t* neg, int64_t ld_neg, int64_t n_neg, float coef, float* w, float* loss,
                    const int32_t* src_edge, const int64_t* inc_ptr, float* w_inc, float* workspace, void* stream);

/* out[j] = sum_r row_w[r] * [gate[r, j] > 0] * x[r, j],  j < d, over a pitched [n_rows, d] matrix (ld elements per row).
 * row_w NULL: weight 1.  gate NULL: no gate; else a matrix of the SAME pitch, the ReLU gate convention of
 * gd_rows_gemm_wgrad_f32's relu_mask (an exact zero is closed); gated (optional, with a gate only; same pitch; may be x
 * itself): receives [gate[r, j] > 0] * x[r, j], the backward through F.relu, in the same pass.  The bias gradients dy.sum(0) of the convs' backward
 * (torch_geometric's GCNConv / GATConv as framework/models/gcn.py:11-12 and gat.py:11-12 build them), the gated form
 * colsum(dh * [p1 > 0]), and GATConv's attention-vector gradients d att_src = sum_r da_src[r] h[r, :] (row_w = da_src).
 * Two levels: blocks own row ranges and write one partial row each, one finishing block adds the partial rows in block order;
 * no atomics, the same bits every call.  d % 4 == 0, d <= 1024, 16-byte aligned rows (GD_E_DIM / GD_E_ALIGN otherwise);
 * n_rows == 0 gives zeros.  workspace: gd_col_sum_workspace(n_rows, d) floats, 16-byte aligned.  Two launches. */
int64_t gd_col_sum_workspace(int64_t n_rows, int32_t d);
int gd_col_sum_f32(const float* x, int64_t ld, int64_t n_rows, int32_t d, const float* row_w, const float* gate, float* gated,
                   float* out, float* workspace, void* stream);

/* The loss stage of the fused node-classification step (NodeClassificationTrainer.train, framework/trainer/base.py:694-752):
 * F.nll_loss(F.log_softmax(z[:, :d_valid], 1)[rows], y[rows]) (mean reduction) and its logit gradients over the n_sel listed
 * rows u = row_idx[i] of a pitched [n_rows, d] matrix:
 *     loss[0] = (1/n_sel) sum_i ( logsumexp(z[u, :d_valid]) - z[u, y[u]] )             (NOT scaled by coef, as gd_edge_bce_f32's)
 *     dz[u, j] = coef / n_sel * (softmax(z[u, :d_valid])_j - [j == y[u]])  for j < d_valid,   0 for d_valid <= j < d
 * The row maximum is subtracted; expf / logf in fp32, the label's term as log1p(sum_{j != y} e_j / e_y) and its gradient as
 * -sum_{j != y} e_j / sum_j e_j (a confident row keeps its tiny term and gradient: no lse - z_y, no 1 - 1).  Only the d columns of the listed rows of dz are written: a caller that
 * wants dL/dz of the whole matrix zeroes dz once.  row_idx (int32) must be unique (two entries of one row would race on its dz
 * row); it need not be ascending.  y is indexed by node id (int64 [n_rows]).  A label outside [0, d_valid) reads nothing
 * outside the row: its row adds nothing to the sum and gets a ZERO dz row, but still counts in n_sel (F.nll_loss raises there;
 * callers reject such labels).  A row id outside [0, n_rows) is skipped the same way.  One lane group per row, float4 per
 * lane; at most 1,024 blocks, which walk the rows grid-strided; one partial per block, added in block order by one thread (no
 * float atomics): the same bits every call.  d % 4 == 0, 4 <= d <= 256, 1 <= d_valid <= d, pitches % 4 == 0 and >= d,
 * n_sel >= 1 (upstream's mean over nothing is NaN) - GD_E_DIM otherwise; 16-byte aligned z / dz - GD_E_ALIGN otherwise.
 * workspace: gd_row_nll_workspace(n_sel, d) floats (= the number of blocks).  Two launches, graph-capturable. */
int64_t gd_row_nll_workspace(int64_t n_sel, int32_t d);
int gd_row_nll_f32(const float* z, int64_t ld_z, int64_t n_rows, int32_t d, int32_t d_valid, const int32_t* row_idx,
                   int64_t n_sel, const int64_t* y, float coef, float* dz, int64_t ld_dz, float* loss, float* workspace,
                   void* stream);

/* ---------------------------------------------------------------- prepared validation --- */

/* The per-validation scoring of the prepared link-prediction validation (gnndelete_amd/evalpass.py; Trainer.eval under
 * --fused_validation, framework/trainer/base.py:229-300 upstream).  ONE decoded edge list (src[k], dst[k]), k < M, laid out
 * [stage pos (n_pos) | stage neg (n_neg) | directed Df (n_df) | Dr (n_dr)], any segment may be empty, 1 <= M < 2^31:
 *     scores[k] = sigmoid(<z[src[k], :d], z[dst[k], :d]>)      with e = exp(-|l|): l >= 0 ? 1 / (1 + e) : e / (1 + e); exactly 1.0f
 *                                                              once e is below half an ulp of 1, never NaN for finite z
 *     stats[0]  = (1 / (n_pos + n_neg)) sum over the stage's edges of  s (1 - y) + log1p(exp(-s)),   s = (double)scores[k],
 *                 y = 1 for k < n_pos: binary_cross_entropy_with_logits applied to the SIGMOID OUTPUTS, as upstream does
 *                 (base.py:243-247); NaN without stage edges
 *     stats[1], stats[2] = mean and POPULATION standard deviation (np.mean / np.std) of the Df scores, in double, two passes
 *                 (mean, then squared deviations); NaN for n_df = 0
 *     status[0] = 1 when an endpoint lies outside [0, n_nodes), else 0: such an edge reads nothing outside z and scores logit 0
 *                 (0.5); wrappers raise IndexError.  Written on every call (no zeroing by the caller).
 * One lane group per edge, float4 loads, at most 1,024 blocks that walk the edges grid-strided, as gd_edge_bce_f32.  The loss
 * terms are formed and added in double: per-block partials, added in block order by the one-block finishing launch, which also
 * re-reads the Df scores in a fixed order (thread stride, then a fixed tree).  No atomics: the same bits on every call.
 * d % 4 == 0, d <= 256, ld_z % 4 == 0 and >= d (GD_E_DIM), 16-byte aligned z, 8-byte aligned stats / workspace (GD_E_ALIGN).
 * workspace: gd_eval_edge_scores_workspace(M, d) doubles.  Two launches, graph-capturable. */
int64_t gd_eval_edge_scores_workspace(int64_t m_all, int32_t d);
int gd_eval_edge_scores_f32(const float* z, int64_t ld_z, int64_t n_nodes, int32_t d, const int64_t* src, const int64_t* dst,
                            int64_t n_pos, int64_t n_neg, int64_t n_df, int64_t n_dr, float* scores, double* stats,
                            int32_t* status, double* workspace, void* stream);

/* The per-validation scoring of the prepared KNOWLEDGE-GRAPH validation (KGTrainer.eval under --fused_validation,
 * framework/trainer/base.py:495-567 upstream).  ONE decoded triple list (src[k], etype[k], dst[k]), k < M, laid out as above
 * [stage pos | stage neg | directed Df | Dr], DistMult table rel [n_rel, d] with row pitch ld_rel:
 *     l_k = sum_j z[src[k], j] rel[etype[k], j] z[dst[k], j]    ((z_a rel) rounded, then one fma chain over z_b per lane: the
 *                                                               association of gd_edge_dot_f32's DistMult decode)
 *     scores[k] = l_k                   for the stage (k < n_pos + n_neg): upstream ranks and scores the stage WITHOUT sigmoid
 *     scores[k] = sigmoid(l_k)          for Df / Dr, by gd_eval_edge_scores_f32's two branches (never NaN for finite inputs)
 *     stats[0]  = (1 / (n_pos + n_neg)) sum over the stage of  max(l, 0) - l y + log1p(exp(-|l|)),   l = (double)scores[k],
 *                 y = 1 for k < n_pos: binary_cross_entropy_with_logits, finite at any finite l; NaN without stage triples
 *     stats[1], stats[2] = mean and POPULATION standard deviation of the Df scores, as gd_eval_edge_scores_f32
 *     status[0] = 1 when an endpoint lies outside [0, n_nodes) or a type outside [0, n_rel), else 0: such a triple reads nothing
 *                 and scores logit 0 (0 in the stage, 0.5 in Df / Dr); wrappers raise IndexError.
 * The launch shape, the double partials, the finishing launch and the argument rules are gd_eval_edge_scores_f32's (the same
 * bits on every call, no atomics); rel additionally 16-byte aligned with ld_rel % 4 == 0 and >= d, n_rel >= 1.
 * workspace: gd_eval_triple_scores_workspace(M, d) doubles.  Two launches, graph-capturable. */
int64_t gd_eval_triple_scores_workspace(int64_t m_all, int32_t d);
int gd_eval_triple_scores_f32(const float* z, int64_t ld_z, int64_t n_nodes, int32_t d, const float* rel, int64_t ld_rel,
                              int64_t n_rel, const int64_t* src, const int64_t* dst, const int64_t* etype, int64_t n_pos,
                              int64_t n_neg, int64_t n_df, int64_t n_dr, float* scores, double* stats, int32_t* status,
                              double* workspace, void* stream);

/* The per-validation scoring of the prepared node-classification validation (NodeClassificationTrainer.eval under
 * --fused_validation, base.py:754-790 upstream) over the n_sel listed rows u = row_idx[i] (int32) of a pitched [n_rows, ld]
 * matrix of d_valid classes, labels y indexed by node id (int64 [n_rows]):
 *     loss[0]    = (1 / n_sel) sum_i ( logsumexp(z[u, :d_valid]) - z[u, y[u]] )        F.nll_loss(F.log_softmax(z, 1)[rows], y[rows])
 *     correct[0] = the number of listed rows whose arg-max over [0, d_valid) equals y[u]
 * The arg-max is the LOWEST index among equal maxima (torch.argmax / numpy.argmax on a row without NaN).  The row maximum is
 * subtracted and the terms are formed in DOUBLE (exp / log / log1p in fp64; the label's term as log1p(sum_{j != y} e_j / e_y)
 * while e_y is not tiny), per-block double partials added in block order, counts added as integers: the same bits every call.
 * A row id outside [0, n_rows) is skipped and a label outside [0, d_valid) counts as wrong with term 0 (both still count in
 * n_sel), as gd_row_nll_f32.  n_sel = 0 gives NaN and 0.  1 <= d_valid <= 256, ld >= d_valid, no alignment beyond the float
 * (scalar loads); 8-byte aligned loss / correct / workspace.  workspace: gd_row_nll_eval_workspace(n_sel, d_valid) doubles.
 * Two launches (one for n_sel = 0), graph-capturable. */
int64_t gd_row_nll_eval_workspace(int64_t n_sel, int32_t d_valid);
int gd_row_nll_eval_f32(const float* z, int64_t ld, int64_t n_rows, int32_t d_valid, const int32_t* row_idx, int64_t n_sel,
                        const int64_t* y, double* loss, int64_t* correct, double* workspace, void* stream);

/* ---------------------------------------------------------------- optimizer ------------ */

/* torch.optim.Adam (no amsgrad, weight_decay 0) on one tensor (delete_gnn.py:221-226).
 * `step` is a device int32 counter incremented by the kernel (graph-capturable). */
int gd_adam_f32(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int32_t* step,
                int64_t n, double lr, double beta1, double beta2, double eps, void* stream);

/* gd_adam_f32 with the step number read from a shared iteration counter (t = *iter + 1). */
int gd_adam_at_f32(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, const int32_t* iter,
                   int64_t n, double lr, double beta1, double beta2, double eps, void* stream);

/* ---------------------------------------------------------------- relational attention -- */

/* Softmax over the entries of every CSR row (torch_geometric.utils.softmax as the reference's RGATConv calls it across
 * the relations of a target node, framework/models/rgat.py:322-337):
 *     alpha[k] = exp(e[k] - max_row) / (sum_row exp(e - max_row) + 1e-16),   k in [rowptr[i], rowptr[i+1])
 * and its backward  de[k] = alpha[k] (dalpha[k] - sum_row alpha dalpha).  Empty rows are skipped. */
int gd_segment_softmax_f32(const int32_t* rowptr, const float* e, int32_t n_rows, float* alpha, void* stream);
int gd_segment_softmax_bwd_f32(const int32_t* rowptr, const float* alpha, const float* dalpha, int32_t n_rows,
                               float* de, void* stream);

/* out[k] = < a[ia[k], :], b[ib[k], :] > for k < n: the gradient of an edge weight of a weighted typed aggregation,
 * d alpha_e = < dm[(relation, target) row of e, :], x[source of e, :] > (autograd of the alpha_e x_j messages,
 * rgat.py:322-337).  float4 path for d % 4 == 0 with 16-byte aligned rows, any d otherwise. */
int gd_rowpair_dot_f32(const float* a, int64_t ld_a, const int32_t* ia, const float* b, int64_t ld_b, const int32_t* ib,
                       int64_t n, int32_t d, float* out, void* stream);

/* Gradients of TRAINABLE relation weights and of per-edge coefficients, straight from relation-major edge lists (no [R, N, d]
 * tensor of per-relation aggregates; ABI 8):
 *   gd_typed_wgrad_f32     dW[r, b] = sum over the edges e of relation r (rel_ptr[r] <= e < rel_ptr[r + 1] of src / dst / w) of
 *                          w[e] * x[src[e], block b]^T dy[dst[e], block b];  dW is [n_rel, n_blocks, d_in / n_blocks, d_out / n_blocks]
 *                          (n_blocks = 1: dense [d_in, d_out] per relation); w = NULL: weight 1.  Edges of a relation are added
 *                          in array order by ONE workgroup per 16 x 16 output tile: bit-reproducible, no atomics.
 *   gd_typed_edge_dot_f32  out[e] = < x[src[e], :], dy[dst[e], :] W_(rel[e])^T > (the gradient of an edge's coefficient when
 *                          the message is coefficient * x_src W_rel), weight as for gd_typed_wgrad_f32's dW.
 * Replace torch.einsum('rnbi,rbio->nbo') over the [R, N, in] mean aggregates and its autograd in the reference's trainable
 * RGCNConv (framework/models/rgcn.py:17-38 under trainer/base.py:394-493, retrain.py:235-339) and the per-edge
 * transforms of RGATConv (framework/models/rgat.py:188-206, :322-337). */
int gd_typed_wgrad_f32(const int32_t* rel_ptr, int32_t n_rel, const int32_t* src, const int32_t* dst, const float* w,
                       const float* x, int64_t ldx, const float* dy, int64_t ldy, int32_t n_blocks, int32_t d_in, int32_t d_out,
                       float* dw, void* stream);
int gd_typed_edge_dot_f32(const int32_t* src, const int32_t* dst, const int32_t* rel, int64_t n_edges, const float* x, int64_t ldx,
                          const float* dy, int64_t ldy, const float* weight, int32_t n_blocks, int32_t d_in, int32_t d_out,
                          float* out, void* stream);

/* ---------------------------------------------------------------- GraphSAINT batches ---- */

/* The induced subgraph of one GraphSAINT batch (torch_geometric saint_subgraph as the reference's mini-batch loop uses it,
 * framework/trainer/gnndelete_nodeemb.py:379-385; RandomWalkSubgraphSampler.subgraph here), cut on the device.
 *   rowptr / col  [n_nodes + 1] / [E]: CSR over SOURCE rows of the training edges, edges of a row sorted by target, ties
 *                 in input order (the sampler's stable (src, dst) sort); edge_flags [E]: one byte per edge in that order,
 *                 bit 0 = sdf_mask, bit 1 = df_mask
 *   nodes [n_b]   int64, the batch's node ids, ascending and unique; row r of the batch is nodes[r]
 *   node_flags    [n_nodes] (optional): bit 0 S1 (sdf_node_1hop_mask), bit 1 S2, bit 2 NI1, bit 3 NI2 (the non-Df masks)
 *   relabel       [n_nodes] int64, zeroed ONCE by the caller: generation << 32 | batch id of the nodes of the latest cut;
 *                 `generation` must differ from (and exceed 0 and) every earlier call's on the same array - nothing is cleared
 *   edge_cap      capacity of the edge outputs.  When the batch has more edges, counts is still written and the edge
 *                 outputs are not: the caller grows its buffers and cuts again (same generation is fine)
 * Outputs (device):
 *   e_index [2, edge_cap] int64 (row 1 at e_index + edge_cap), e_flags [edge_cap]: the induced edges in batch ids, sorted by
 *           (src, dst) - exactly what subgraph() yields - and their flag bytes
 *   all_src / all_dst   [edge_cap + n_b] int64: the batch edges without self loops (what graph.build_csr keeps), in that order
 *   sdf_src / sdf_dst   [edge_cap + n_b] int64: the same for the sdf edges (gd_batch_csr appends the self loops behind them)
 *   df_index [2, edge_cap] int64: the Df edges (the batch's positive DEC pairs)
 *   row_lists [4, n_b] int32: batch rows with node flag bit k set, ascending, list k at row_lists + k * n_b
 *   counts [11] int32: n_b, e_all, e_sdf, m_df, |S1_b|, |S2_b|, |NI1_b|, |NI2_b|, e_all without self loops, e_sdf without
 *           self loops, and 1 if a node id was outside [0, n_nodes) (such rows are cut as empty)
 *   workspace >= gd_induced_subgraph_workspace(n_b) bytes, 256-byte aligned.
 * One wave per batch row; rows of any length (hubs) are walked 64 edges at a time.  Integer only, bit-exact. */
int64_t gd_induced_subgraph_workspace(int32_t n_b);
int gd_induced_subgraph(const int32_t* rowptr, const int32_t* col, const uint8_t* edge_flags, int32_t n_nodes,
                        const int64_t* nodes, int32_t n_b, const uint8_t* node_flags, int32_t generation,
                        int64_t* relabel, int64_t edge_cap, int64_t* e_index, uint8_t* e_flags, int64_t* all_src,
                        int64_t* all_dst, int64_t* sdf_src, int64_t* sdf_dst, int64_t* df_index, int32_t* row_lists,
                        int32_t* counts, void* workspace, int64_t workspace_bytes, void* stream);

/* graph.build_csr(edge_index, n_nodes, mode) for a batch, without a host round trip: src / dst hold n_edges edges without
 * self loops and room for n_nodes more, where the self loops are appended (in place).  Writes the target-major CSR
 * (rowptr [n+1], col [nnz]), the source-major one (rowptr_t, col_t), perm_t [nnz] (forward slot of every transposed entry)
 * and, for mode 0 (gcn), val / val_t (gd_gcn_norm_f32); mode 1 (gat) leaves val / val_t alone (may be NULL).
 * nnz = n_edges + n_nodes.  The index arrays are those build_csr computes from the same edge list (gd_csr_from_coo).
 * workspace >= gd_batch_csr_workspace(n_nodes, n_edges) bytes, 256-byte aligned. */
int64_t gd_batch_csr_workspace(int32_t n_nodes, int64_t n_edges);
int gd_batch_csr(int64_t* src, int64_t* dst, int64_t n_edges, int32_t n_nodes, int32_t mode, int32_t* rowptr, int32_t* col,
                 float* val, int32_t* rowptr_t, int32_t* col_t, int32_t* perm_t, float* val_t, void* workspace,
                 int64_t workspace_bytes, void* stream);

/* The segmented inputs of gd_rowpair_mse_f32 for one layer of a batch (targets change every batch, so the pre-folded
 * gd_rowtarget_mse_f32 form does not apply): DEC terms (z row pos[0][i], target row neg[0][i]) and (pos[1][i], neg[1][i])
 * for i < n_pos with weight w_dec, NI terms (ni[j], ni[j]) with weight w_ni.  Terms are grouped by z row, one segment per
 * batch row (seg_ptr [n_b + 1]; call gd_rowpair_mse_f32 with seg_row = 0 .. n_b-1, n_seg = n_b), ordered by target row
 * inside a segment, ties by term order: the gradient of a repeated endpoint is summed in a fixed order.
 * pos / neg: int64 [2, ld] (row 1 at + ld).  term_o / term_w / term_kind [2 n_pos + n_ni].
 * workspace >= gd_batch_loss_terms_workspace(n_b, 2 n_pos + n_ni) bytes, 256-byte aligned. */
int64_t gd_batch_loss_terms_workspace(int32_t n_b, int64_t n_terms);
int gd_batch_loss_terms(const int64_t* pos, int64_t ld_pos, const int64_t* neg, int64_t ld_neg, int32_t n_pos,
                        const int32_t* ni, int32_t n_ni, int32_t n_b, float w_dec, float w_ni, int32_t* seg_ptr,
                        int32_t* term_o, float* term_w, int32_t* term_kind, void* workspace, int64_t workspace_bytes,
                        void* stream);

/* gd_induced_subgraph for a KNOWLEDGE graph (KGGNNDeleteNodeembTrainer.train, framework/trainer/gnndelete_nodeemb.py:659-846 of
 * the reference; RandomWalkSubgraphSampler.subgraph followed by the trainer's dr_mask / df_mask / forward-type masking here), same
 * conventions: rowptr / col as above, edge_type [E] int32 and edge_flags [E] in that order (bit 0 = dr_mask, bit 1 = df_mask -
 * parallel edges of one pair keep their input order, so do their types), node_flags bit 0 = list 1
 * (sdf_node_1hop_mask_non_df_mask), bit 1 = list 2 (the 2-hop one): the Del rows AND the NI rows of the two layers.
 * Outputs (device), all in batch ids:
 *   dr_src / dr_dst / dr_type [edge_cap] int32: the batch's Dr edges, in subgraph() order (message passing)
 *   df_index [2, edge_cap] int64 (row 1 at + edge_cap), df_type [edge_cap] int64: the Df triples with type < num_edge_type, in
 *           subgraph() order (the decoded positives; what negative_sampling_kg reads)
 *   row_lists [2, n_b] int32: batch rows with node flag bit k, ascending, list k at row_lists + k * n_b
 *   counts [6] int32: n_b, Dr edges, decoded Df triples, |list 1|, |list 2|, and 1 if a node id was outside [0, n_nodes)
 *           (such rows are cut as empty).  When either edge count exceeds edge_cap, counts is written and no edge output is.
 *   workspace >= gd_induced_subgraph_typed_workspace(n_b) bytes, 256-byte aligned.  Integer only, bit-exact; no memset. */
int64_t gd_induced_subgraph_typed_workspace(int32_t n_b);
int gd_induced_subgraph_typed(const int32_t* rowptr, const int32_t* col, const int32_t* edge_type, const uint8_t* edge_flags,
                              int32_t n_nodes, int32_t num_edge_type, const int64_t* nodes, int32_t n_b, const uint8_t* node_flags,
                              int32_t generation, int64_t* relabel, int64_t edge_cap, int32_t* dr_src, int32_t* dr_dst,
                              int32_t* dr_type, int64_t* df_index, int64_t* df_type, int32_t* row_lists, int32_t* counts,
                              void* workspace, int64_t workspace_bytes, void* stream);

/* graph.TypedNodeCSR(edge_index, edge_type, n_nodes, n_rel) for a batch, without a host round trip: the two node-major typed
 * graphs gd_rgcn_conv_f32 reads, from n_edges typed edges (src, dst, type int32, any order).
 *   node_ptr [n_nodes + 1], seg_ptr [seg_cap + 1], seg_rel [seg_cap], col / w [edge_cap]: `fwd` - in-edges sorted by (target,
 *           relation, source), w = 1 / |run| (one correctly rounded division);  the _t arrays: `bwd`, the transpose sorted by
 *           (source, relation, target), every edge carrying the weight of the forward run it belongs to
 *   status [4] int32 (device): runs of fwd, runs of bwd, 1 if an edge had an endpoint or relation out of range (it is left
 *           out), 1 if seg_cap was too small (n_edges always suffices; edge_cap >= n_edges is required)
 * Edges take a slot of their node's bucket by integer atomics and are then ranked inside the bucket by (relation, other
 * endpoint, input position): the result does not depend on the order the atomics arrive in.  No float atomics; the counters are
 * zeroed by the first launch; every store is guarded by the capacities.  The rank costs O(degree^2) per node: batch sizes.
 * workspace >= gd_batch_typed_csr_workspace(n_nodes, n_edges, n_rel) bytes, 256-byte aligned (-1: n_nodes * n_rel >= 2^31). */
int64_t gd_batch_typed_csr_workspace(int32_t n_nodes, int64_t n_edges, int32_t n_rel);
int gd_batch_typed_csr(const int32_t* src, const int32_t* dst, const int32_t* type, int64_t n_edges, int32_t n_nodes, int32_t n_rel,
                       int64_t edge_cap, int64_t seg_cap, int32_t* node_ptr, int32_t* seg_ptr, int32_t* seg_rel, int32_t* col,
                       float* w, int32_t* node_ptr_t, int32_t* seg_ptr_t, int32_t* seg_rel_t, int32_t* col_t, float* w_t,
                       int32_t* status, void* workspace, int64_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------- collectives (RCCL) ---- */

/* The two exchanges of the row-partitioned multi-GPU step (the reference has no distributed code at all: SURVEY
 * section 5; north_star adds "RCCL all-reduce of partial aggregates and Del-operator gradients over xGMI").  One process
 * per GPU; a communicator is an RCCL ncclComm_t behind a void*.  RCCL is looked up at first use (dlsym among the loaded
 * libraries - a PyTorch-ROCm process carries its own librccl - then librccl.so by name): without it these entries return
 * GD_E_NULL and everything else in the library works.  Failures of RCCL itself come back as -(1000 + ncclResult_t).
 *   gd_comm_unique_id   rank 0 fills 128 bytes (ncclUniqueId, HOST memory) and ships them to every rank out of band
 *   gd_comm_init        collective over the n_ranks processes: *comm <- the communicator of `rank` on the CURRENT device
 *   gd_comm_destroy     NULL is accepted
 *   gd_allreduce_f32    buf[0..n) <- sum over ranks, in place, enqueued on `stream`: the packed [dW_D1 | dW_D2 | loss sums]
 *                       buffer of a step (80 KiB, latency-bound) - replaces nothing upstream
 *   gd_exchange_rows_f32  sparse all-to-all of feature rows: send_rows[p] / recv_rows[p] (HOST arrays of n_ranks int64 row
 *                       counts) rows of row_elems floats go to / come from peer p, packed back to back in peer order in
 *                       `send` / `recv` (device); one grouped ncclSend / ncclRecv per non-empty pair on `stream` - xGMI is
 *                       point-to-point, so every pair moves over its own link concurrently.  The halo rows of a layer's
 *                       aggregation (forward) and of its transpose (backward). */
int gd_comm_unique_id(void* id128);
int gd_comm_init(const void* id128, int32_t n_ranks, int32_t rank, void** comm);
int gd_comm_destroy(void* comm);
int gd_allreduce_f32(float* buf, int64_t n, void* comm, void* stream);
int gd_exchange_rows_f32(const float* send, const int64_t* send_rows, float* recv, const int64_t* recv_rows,
                         int32_t row_elems, int32_t n_ranks, void* comm, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GNNDELETE_HIP_H */
