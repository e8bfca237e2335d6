"""GraphSAINT mini-batch unlearning on a fused HIP batch step (--minibatch --fused_minibatch).

The reference trains the Del operators of ogbl-* graphs on GraphSAINT random-walk batches
(framework/trainer/gnndelete_nodeemb.py:352-445); framework.trainer.sampler.train_minibatch runs that loop through
autograd.  NodeembEngine cannot serve it: it is built once per request (locality order, split plans, fp64-folded loss
terms, a captured graph) while a batch changes the graph, the masks, the loss rows and the sizes on every step.
MinibatchNodeembStep is the same idea for shapes that change per batch - an explicit forward, a hand-derived backward
and Adam on the HIP kernels, fed by a device-side subgraph cut:

  1. gd_induced_subgraph: the batch's edges (relabelled, in subgraph() order), its Df edges, its S1 / S2 / NI1 / NI2
     rows and a count vector - the ONE blocking host read of a batch (outside negative_sampling);
  2. gd_batch_csr: the CSRs over all batch edges (z_ori) and over its sdf edges (Del forward / backward), index arrays
     as graph.build_csr makes them, without SplitPlans (the plain per-row kernels fit batch sizes);
  3. frozen layer 1: x W1^T (and GAT's attention scores) is computed ONCE per run for the whole graph and gathered per
     batch, then aggregated over each batch CSR (gd_spmm_csr_f32 / gd_gat_aggregate_f32);
  4. layer 2, both Del operators, negatives (sampler.negative_sampling, the tests' seam), DEC + NI of both layers
     (gd_batch_loss_terms + gd_rowpair_mse_f32: deterministic per-row segments), the layer-wise backward and Adam.

Update order is the autograd loop's: loss1's gradient -> Adam on W_D1; loss2's gradient (W_D2's, and W_D1's, which is
kept and added to the next batch's W_D1 gradient) -> Adam on W_D2.  The per-step losses stay on the device and become
trainer_log['steps'] once per epoch.

MinibatchEdgeprobStep is the batch step of the edge-probability trainer (--unlearning_model gnndelete;
framework/trainer/gnndelete.py:312-450) on the same cut, sdf CSR and layer helpers (_BatchStep): its loss stage is
gd_edgeprob_batch_loss_f32 over [Df edges | negatives | the batch's S_Df edges with src < dst], its backward
EdgeprobEngine's on the batch CSR, one Adam step on both Del weights.

MinibatchBackboneStep is the batch step of the ORIGINAL model's training (train_gnn.py --minibatch --fused_minibatch;
framework/trainer/base.py:144-227): every parameter trains, so there is no frozen layer-1 table - each batch computes
x[nodes] W1^T with the current W1 (gd_rows_gather_gemm_f32), runs both layers over the CSR of all batch edges, the BCE
link-prediction loss over [batch edges | negatives] (gd_edge_bce_f32) and BackboneEngine's backward, then Adam on every
parameter.

MinibatchKGNodeembStep is the batch step of the knowledge-graph trainer (delete_gnn.py --gnn rgcn --fused_minibatch;
framework/trainer/gnndelete_nodeemb.py:659-846): a typed cut (gd_induced_subgraph_typed: the batch's Dr edges with their
relation types, the decoded Df triples, the two row lists), the batch's node-major typed graphs (gd_batch_typed_csr: the
arrays of graph.TypedNodeCSR), both R-GCN convs on gd_rgcn_conv_f32, negatives from utils.negative_sampling_kg, the loss
stage and the layer-wise update of MinibatchNodeembStep."""
import os

import numpy as np
import torch

from . import _lib, ops
from ._lib import check, ptr, stream_ptr

N_COUNTS = 11          # gd_induced_subgraph's count vector


def fused_minibatch_unsupported(model, args, optimizer):
    """None when the fused batch step applies, else the reason it does not (one line)."""
    from .framework.trainer.sampler import data_parallel_world
    from .nn import GATConv, GCNConv
    conv1, conv2 = getattr(model, 'conv1', None), getattr(model, 'conv2', None)
    if not (isinstance(conv1, (GCNConv, GATConv)) and type(conv1) is type(conv2)) or not hasattr(model, 'deletion1'):
        return f'no fused batch step for the {type(model).__name__} backbone (GCN and GAT only)'
    if getattr(args, 'loss_fct', 'mse_mean') not in ('mse_mean', 'mse_sum'):
        return f'--loss_fct {args.loss_fct} is not an MSE loss'
    if data_parallel_world()[1] > 1:
        return 'torch.distributed with more than one rank'
    opts = list(optimizer) if isinstance(optimizer, (list, tuple)) else [optimizer]
    for opt in opts:
        g = opt.param_groups[0]
        if not isinstance(opt, torch.optim.Adam) or g.get('weight_decay', 0) or g.get('amsgrad') or g.get('maximize'):
            return 'the optimizer is not a plain torch.optim.Adam'
    return None


def _grow(n):
    return max(1024, 1 << int(np.ceil(np.log2(max(n, 1) * 1.25))))


class _BatchCSR:
    __slots__ = ('n', 'nnz', 'rowptr', 'col', 'val', 'rowptr_t', 'col_t', 'perm_t', 'val_t')


class BatchCut:
    """The device side of a GraphSAINT batch: the sampler's source-major CSR and flag bytes (packed once per run), the
    node-sized relabel array, and buffers for the cut's outputs (node buffers sized to the batch upper bound, edge
    buffers grown geometrically when a cut reports more)."""

    def __init__(self, data, loader, dev, max_nodes=None):
        self.dev = dev
        self.n = int(loader.n)
        # the sampler's source-major CSR (sorted by (src, dst), stable ties) and one flag byte per edge in that order
        self.rowptr32 = loader.rowptr.to(device=dev, dtype=torch.int32).contiguous()
        self.col32 = loader.dst_sorted.to(device=dev, dtype=torch.int32).contiguous()
        if hasattr(data, 'sdf_mask') and hasattr(data, 'df_mask'):
            order = loader.order.to(data.sdf_mask.device)
            flags = data.sdf_mask.to(torch.uint8) | (data.df_mask.to(torch.uint8) << 1)
            self.edge_flags = flags[order].to(dev).contiguous()
        else:                               # (the backbone's batches: no request, no flagged edge)
            self.edge_flags = torch.zeros(self.col32.numel(), dtype=torch.uint8, device=dev)
        node_flags = torch.zeros(self.n, dtype=torch.uint8)
        for bit, key in enumerate(['sdf_node_1hop_mask', 'sdf_node_2hop_mask', 'sdf_node_1hop_mask_non_df_mask',
                                   'sdf_node_2hop_mask_non_df_mask']):
            if hasattr(data, key):          # (the edge-probability loop has no NI rows: lists 2 and 3 stay empty)
                node_flags |= getattr(data, key).to('cpu', torch.uint8) << bit
        self.node_flags = node_flags.to(dev)
        self.relabel = torch.zeros(self.n, dtype=torch.int64, device=dev)
        self.generation = 0
        self.counts = torch.zeros(N_COUNTS, dtype=torch.int32, device=dev)
        self.n_cap = self.e_cap = 0
        self._bufs = {}
        self._ensure(max_nodes or 1024, 4 * (max_nodes or 1024))
        self.reads = 0                  # blocking host reads made by the cut (the count vector)

    # ---------------------------------------------------------------------------------------------- buffers
    def _ensure(self, n_b, e):
        if n_b <= self.n_cap and e <= self.e_cap:
            return
        self.n_cap, self.e_cap = max(self.n_cap, _grow(n_b)), max(self.e_cap, _grow(e))
        dev, n, c = self.dev, self.n_cap, self.e_cap
        i64 = dict(dtype=torch.int64, device=dev)
        self.e_index = torch.empty(2, c, **i64)
        self.e_flags = torch.empty(c, dtype=torch.uint8, device=dev)
        self.all_src, self.all_dst = torch.empty(c + n, **i64), torch.empty(c + n, **i64)
        self.sdf_src, self.sdf_dst = torch.empty(c + n, **i64), torch.empty(c + n, **i64)
        self.df_index = torch.empty(2, c, **i64)
        self.row_lists = torch.empty(4 * n, dtype=torch.int32, device=dev)     # list k at k * n_b
        self.seg_row = torch.arange(n, dtype=torch.int32, device=dev)

    def _ws(self, key, nbytes):
        if nbytes < 0:
            raise ValueError(f'{key}: batch too large for int32 indices')
        buf = self._bufs.get(key)
        if buf is None or buf.numel() < nbytes:
            buf = self._bufs[key] = torch.empty(max(256, _grow(nbytes)), dtype=torch.uint8, device=self.dev)
        return buf

    # ---------------------------------------------------------------------------------------------- the cut
    def cut(self, nodes):
        """gd_induced_subgraph on one sorted, unique node set -> the host copy of the count vector."""
        nodes = nodes.to(self.dev, torch.int64).contiguous()
        n_b = int(nodes.numel())
        self._ensure(n_b, 0)
        self.generation += 1
        L = _lib.lib()
        while True:
            ws = self._ws('cut', L.gd_induced_subgraph_workspace(n_b))
            check(L.gd_induced_subgraph(ptr(self.rowptr32), ptr(self.col32), ptr(self.edge_flags), self.n, ptr(nodes), n_b,
                                        ptr(self.node_flags), self.generation, ptr(self.relabel), self.e_cap,
                                        ptr(self.e_index), ptr(self.e_flags), ptr(self.all_src), ptr(self.all_dst),
                                        ptr(self.sdf_src), ptr(self.sdf_dst), ptr(self.df_index), ptr(self.row_lists),
                                        ptr(self.counts), ptr(ws), ws.numel(), stream_ptr(self.dev)), 'gd_induced_subgraph')
            cnt = self.counts.tolist()
            self.reads += 1
            if cnt[1] <= self.e_cap:
                break
            self._ensure(n_b, cnt[1])                      # the edge outputs were not written: grow, cut again
        if cnt[10]:
            raise IndexError(f'batch node ids outside [0, {self.n})')
        self.nodes, self.cnt = nodes, cnt
        return cnt

    def rows(self, k, count):
        """Batch rows of the latest cut with node flag bit k (0 S1, 1 S2, 2 NI1, 3 NI2), ascending: int32 [count]."""
        n_b = self.cnt[0]
        return self.row_lists.view(-1)[k * n_b:k * n_b + count]

    def batch_edges(self):
        """(edge_index [2, e_all] int64, flags [e_all] uint8) of the latest cut, views of the step's buffers."""
        e = self.cnt[1]
        return self.e_index[:, :e], self.e_flags[:e]

    def batch_csr(self, sdf, gat):
        """gd_batch_csr over the latest cut's sdf edges (sdf=True) or all its edges; gcn values unless gat."""
        n_b = self.cnt[0]
        n_e = self.cnt[9] if sdf else self.cnt[8]
        src, dst = (self.sdf_src, self.sdf_dst) if sdf else (self.all_src, self.all_dst)
        g = _BatchCSR()
        g.n, g.nnz = n_b, n_e + n_b
        i32 = dict(dtype=torch.int32, device=self.dev)
        g.rowptr, g.rowptr_t = torch.empty(n_b + 1, **i32), torch.empty(n_b + 1, **i32)
        g.col, g.col_t, g.perm_t = torch.empty(g.nnz, **i32), torch.empty(g.nnz, **i32), torch.empty(g.nnz, **i32)
        g.val = g.val_t = None
        if not gat:
            g.val = torch.empty(g.nnz, dtype=torch.float32, device=self.dev)
            g.val_t = torch.empty(g.nnz, dtype=torch.float32, device=self.dev)
        L = _lib.lib()
        ws = self._ws('csr', L.gd_batch_csr_workspace(n_b, n_e))
        check(L.gd_batch_csr(ptr(src), ptr(dst), n_e, n_b, 1 if gat else 0, ptr(g.rowptr), ptr(g.col), ptr(g.val),
                             ptr(g.rowptr_t), ptr(g.col_t), ptr(g.perm_t), ptr(g.val_t), ptr(ws), ws.numel(),
                             stream_ptr(self.dev)), 'gd_batch_csr')
        return g

class _BatchLayers:
    """The layer helpers over a batch CSR that every batch step shares (self.dev, self.gat, self._bufs, self.events)."""

    def _ws(self, key, nbytes):
        if nbytes < 0:
            raise ValueError(f'{key}: batch too large for int32 indices')
        buf = self._bufs.get(key)
        if buf is None or buf.numel() < nbytes:
            buf = self._bufs[key] = torch.empty(max(256, _grow(nbytes)), dtype=torch.uint8, device=self.dev)
        return buf

    def _mark(self, stage):
        if self.events is not None:
            ev = torch.cuda.Event(enable_timing=True)
            ev.record()
            self.events.append((stage, ev))

    # ---------------------------------------------------------------------------------------------- layers
    def _agg(self, g, h, scores, bias, slope):
        """GCNConv / GATConv aggregation of transformed rows h over a batch CSR -> (y, saved attention or None)."""
        y = torch.empty(g.n, h.shape[1], dtype=torch.float32, device=self.dev)
        if not self.gat:
            check(_lib.lib().gd_spmm_csr_f32(ptr(g.rowptr), ptr(g.col), ptr(g.val), ptr(h), h.stride(0), ptr(y), y.stride(0),
                                             ptr(bias), 0.0, g.n, h.shape[1], stream_ptr(self.dev)), 'gd_spmm_csr_f32')
            return y, None
        a_src, a_dst = scores
        alpha = torch.empty(g.nnz, dtype=torch.float32, device=self.dev)
        check(_lib.lib().gd_gat_aggregate_f32(ptr(g.rowptr), ptr(g.col), ptr(a_src), ptr(a_dst), ptr(h), h.stride(0), ptr(y),
                                              y.stride(0), ptr(bias), ptr(alpha), float(slope), g.n, h.shape[1],
                                              stream_ptr(self.dev)), 'gd_gat_aggregate_f32')
        return y, alpha

    def _agg_bwd(self, g, h, scores, alpha, dy, slope, att, att_grads=None):
        """Input gradient of _agg with respect to h (GAT: message path + the score terms' rank-1 rows).  att_grads (GAT): the
        two buffers that receive the attention vectors' gradients, colsum(h, row_w = d a_src / d a_dst)."""
        n, d = g.n, dy.shape[1]
        if not self.gat:
            dh = torch.empty(n, d, dtype=torch.float32, device=self.dev)
            check(_lib.lib().gd_spmm_csr_f32(ptr(g.rowptr_t), ptr(g.col_t), ptr(g.val_t), ptr(dy), dy.stride(0), ptr(dh),
                                             dh.stride(0), None, 0.0, n, d, stream_ptr(self.dev)), 'gd_spmm_csr_f32')
            return dh
        a_src, a_dst = scores
        dh = torch.empty(n, d, dtype=torch.float32, device=self.dev)
        da = torch.empty(2, n, dtype=torch.float32, device=self.dev)
        de = torch.empty(g.nnz, dtype=torch.float32, device=self.dev)
        check(_lib.lib().gd_gat_aggregate_bwd_f32(ptr(g.rowptr), ptr(g.col), ptr(alpha), ptr(g.rowptr_t), ptr(g.col_t),
                                                  ptr(g.perm_t), ptr(a_src), ptr(a_dst), ptr(h), h.stride(0), ptr(dy),
                                                  dy.stride(0), ptr(dh), dh.stride(0), ptr(da[0]), ptr(da[1]), ptr(de),
                                                  float(slope), n, d, stream_ptr(self.dev)), 'gd_gat_aggregate_bwd_f32')
        if att_grads is not None:
            from .backbone import col_sum
            for k in (0, 1):
                col_sum(h, row_w=da[k], out=att_grads[k].view(-1))
        return ops.rank1_add2_(dh, da[0], att[0], da[1], att[1])


class _BatchStep(_BatchLayers):
    """What the batch steps of both unlearning trainers share: a BatchCut, the frozen layer-1 transform of every node and
    the Adam moments of the two Del weights."""

    def __init__(self, model, data, loader, lr, betas, eps, max_nodes=None):
        from .nn import GATConv
        dev = next(model.parameters()).device
        self.dev, self.model = dev, model
        self.lr, self.betas, self.eps = float(lr), (float(betas[0]), float(betas[1])), float(eps)
        self.gat = isinstance(model.conv1, GATConv)
        self.cut = BatchCut(data, loader, dev, max_nodes)
        # frozen layer 1: the feature transform (and GAT's scores) of every node, once
        c1, c2 = model.conv1, model.conv2
        lin1 = c1.lin_src if self.gat else c1.lin
        lin2 = c2.lin_src if self.gat else c2.lin
        with torch.no_grad():
            x = data.x.to(dev, torch.float32)
            self.h1_all = ops.dense(x, lin1.weight.detach(), None, True).contiguous()
            if self.gat:
                a_s, a_d = ops.row_dots(self.h1_all, c1.att_src.detach(), c1.att_dst.detach())
                self.a1_all = torch.stack([a_s, a_d], 1).contiguous()
        self.b1, self.b2 = c1.bias.detach().contiguous(), c2.bias.detach().contiguous()
        self.w2 = lin2.weight.detach().contiguous()                       # [O, H]
        if self.gat:
            self.att2 = (c2.att_src.detach().reshape(-1).contiguous(), c2.att_dst.detach().reshape(-1).contiguous())
            self.slope1, self.slope2 = float(c1.negative_slope), float(c2.negative_slope)
        self.H, self.O = self.h1_all.shape[1], self.w2.shape[0]
        # trainable state: the model's own Del weights are stepped in place
        self.wd1, self.wd2 = model.deletion1.deletion_weight, model.deletion2.deletion_weight
        self.adam = []
        for p in (self.wd1, self.wd2):
            self.adam.append({'m': torch.zeros_like(p.data), 'v': torch.zeros_like(p.data),
                              'step': torch.zeros(1, dtype=torch.int32, device=dev), 'steps': 0})
        self.g1 = torch.zeros_like(self.wd1.data)
        self.g2 = torch.zeros_like(self.wd2.data)
        self._bufs = {}
        self.events = None              # list -> (stage, cuda event) pairs are appended (stage split of the experiment)

    def _layer2(self, g, z1):
        """conv2(relu(z1)) over g -> (y, h, scores, saved attention)."""
        h = ops.rows_gemm(z1, None, self.w2, trans_w=True, relu_in=True)
        scores = ops.row_dots(h, *self.att2) if self.gat else None
        y, alpha = self._agg(g, h, scores, self.b2, self.slope2 if self.gat else 0.0)
        return y, h, scores, alpha

    def _adam(self, k, p, grad):
        st = self.adam[k]
        check(_lib.lib().gd_adam_f32(ptr(p.data), ptr(grad), ptr(st['m']), ptr(st['v']), ptr(st['step']), p.numel(), self.lr,
                                     self.betas[0], self.betas[1], self.eps, stream_ptr(self.dev)), 'gd_adam_f32')
        st['steps'] += 1


class MinibatchNodeembStep(_BatchStep):
    """Owns the per-run state of the fused batch step: a BatchCut, the frozen layer-1 transform of every node, the
    Adam moments and the carried W_D1 gradient."""

    def __init__(self, model, data, loader, alpha, lr, betas, eps, max_nodes=None):
        super().__init__(model, data, loader, lr, betas, eps, max_nodes)
        self.alpha = float(alpha)
        self.g1_live = False            # W_D1 holds loss2's gradient of the previous batch (carried into the next step)

    def _loss(self, z, z_ori, neg, n_pos, ni, n_ni, d, sums):
        """DEC + NI of one layer: sums[0] += sum of squared DEC differences, sums[1] += NI's; -> dz of alpha * DEC_mean +
        (1 - alpha) * NI_mean (a mean over zero rows has no gradient)."""
        L = _lib.lib()
        c = self.cut
        n_b = c.cnt[0]
        n_terms = 2 * n_pos + n_ni
        w_dec = self.alpha / (2 * n_pos * d) if n_pos else 0.0
        w_ni = (1.0 - self.alpha) / (n_ni * d) if n_ni else 0.0
        seg_ptr = torch.empty(n_b + 1, dtype=torch.int32, device=self.dev)
        term_o = torch.empty(max(n_terms, 1), dtype=torch.int32, device=self.dev)
        term_w = torch.empty(max(n_terms, 1), dtype=torch.float32, device=self.dev)
        term_kind = torch.empty(max(n_terms, 1), dtype=torch.int32, device=self.dev)
        ws = self._ws('terms', L.gd_batch_loss_terms_workspace(n_b, n_terms))
        check(L.gd_batch_loss_terms(ptr(c.df_index), c.e_cap, ptr(neg), neg.stride(0), n_pos, ptr(ni), n_ni, n_b, w_dec,
                                    w_ni, ptr(seg_ptr), ptr(term_o), ptr(term_w), ptr(term_kind), ptr(ws), ws.numel(),
                                    stream_ptr(self.dev)), 'gd_batch_loss_terms')
        dz = torch.empty(n_b, d, dtype=torch.float32, device=self.dev)
        part = torch.empty(max(1, L.gd_rowpair_mse_workspace(n_b)), dtype=torch.float32, device=self.dev)
        check(L.gd_rowpair_mse_f32(ptr(z), z.stride(0), ptr(z_ori), z_ori.stride(0), d, ptr(seg_ptr), ptr(c.seg_row), n_b,
                                   ptr(term_o), ptr(term_w), ptr(term_kind), ptr(dz), dz.stride(0), 0, ptr(sums), ptr(part),
                                   stream_ptr(self.dev)), 'gd_rowpair_mse_f32')
        return dz

    # ---------------------------------------------------------------------------------------------- one batch
    def step(self, nodes, sums):
        """One batch of the layer-wise update on `nodes`; sums [4] (zeroed by the caller) receives the squared-difference
        sums (DEC 1, NI 1, DEC 2, NI 2).  Returns the divisors that turn them into the four means."""
        from .framework.trainer import sampler as S
        self._mark('start')
        c = self.cut
        cnt = c.cut(nodes)
        n_b, m_df, n_s1, n_s2, n_ni1, n_ni2 = cnt[0], cnt[3], cnt[4], cnt[5], cnt[6], cnt[7]
        self._mark('cut')
        g_all, g_sdf = c.batch_csr(False, self.gat), c.batch_csr(True, self.gat)
        self._mark('csr')
        H, O = self.H, self.O
        idx1, idx2, ni1, ni2 = (c.rows(k, cnt) for k, cnt in enumerate((n_s1, n_s2, n_ni1, n_ni2)))
        # frozen layer 1 on both graphs (x W1^T and the GAT scores gathered from the per-run table)
        h1 = self.h1_all.index_select(0, c.nodes)
        sc1 = None
        if self.gat:
            a1 = self.a1_all.index_select(0, c.nodes)
            sc1 = (a1[:, 0].contiguous(), a1[:, 1].contiguous())
        z1_ori, _ = self._agg(g_all, h1, sc1, self.b1, self.slope1 if self.gat else 0.0)
        p1, _ = self._agg(g_sdf, h1, sc1, self.b1, self.slope1 if self.gat else 0.0)
        z2_ori = self._layer2(g_all, z1_ori)[0]
        # Del forward on the sdf graph
        wd1, wd2 = self.wd1.data, self.wd2.data
        z1 = p1.clone()
        if n_s1:
            ops.rows_gemm(p1, idx1, wd1, out=z1)
        p2, h2, sc2, alpha2 = self._layer2(g_sdf, z1)
        z2 = p2.clone()
        if n_s2:
            ops.rows_gemm(p2, idx2, wd2, out=z2)
        self._mark('forward')
        edge_index, _ = c.batch_edges()
        neg = S.negative_sampling(edge_index, n_b, m_df).to(self.dev, torch.int64).contiguous()
        self._mark('negatives')
        dz1 = self._loss(z1, z1_ori, neg, m_df, ni1, n_ni1, H, sums[0:2])
        dz2 = self._loss(z2, z2_ori, neg, m_df, ni2, n_ni2, O, sums[2:4])
        self._mark('loss')
        # loss1: W_D1's gradient (+ what loss2 left on it last batch), Adam.  torch would skip a parameter whose .grad is
        # None; the Del layer's autograd node always returns a weight gradient (zeros without S1 rows), so neither
        # parameter is ever skipped on the autograd path and none is here.
        if n_s1:
            ops.rows_gemm_wgrad(p1, idx1, dz1, idx1, n_s1, out=self.g1, accumulate=self.g1_live)
        elif not self.g1_live:
            self.g1.zero_()
        self._adam(0, self.wd1, self.g1)
        # loss2: W_D2's gradient and, through conv2 and the ReLU, a fresh W_D1 gradient that waits for the next batch
        if n_s2:
            ops.rows_gemm_wgrad(p2, idx2, dz2, idx2, n_s2, out=self.g2)
        else:
            self.g2.zero_()
        dp2 = dz2.clone()
        if n_s2:
            ops.rows_gemm(dz2, idx2, wd2, trans_w=True, out=dp2)
        dh2 = self._agg_bwd(g_sdf, h2, sc2, alpha2, dp2, self.slope2 if self.gat else 0.0, self.att2 if self.gat else None)
        dx1 = ops.rows_gemm(dh2, None, self.w2)                  # [n_b, H], before the ReLU gate
        if n_s1:
            ops.rows_gemm_wgrad(p1, idx1, dx1, idx1, n_s1, relu_mask=z1, out=self.g1)
        else:
            self.g1.zero_()
        self.g1_live = True
        self._adam(1, self.wd2, self.g2)
        self._mark('backward')
        return (2 * m_df * H, n_ni1 * H, 2 * m_df * O, n_ni2 * O)

    # ---------------------------------------------------------------------------------------------- optimizer state
    def import_adam_state(self, optimizer):
        opts = list(optimizer) if isinstance(optimizer, (list, tuple)) else [optimizer, optimizer]
        for k, (opt, p) in enumerate(zip(opts, (self.wd1, self.wd2))):
            st = opt.state.get(p)
            if st and 'exp_avg' in st:
                self.adam[k]['m'].copy_(st['exp_avg'])
                self.adam[k]['v'].copy_(st['exp_avg_sq'])
                self.adam[k]['steps'] = int(st['step'])
                self.adam[k]['step'].fill_(self.adam[k]['steps'])
        if self.wd1.grad is not None:                       # a gradient left on W_D1 joins the first step
            self.g1.copy_(self.wd1.grad)
            self.g1_live = True

    def export_adam_state(self, optimizer):
        """Adam moments and step counts into the caller's torch optimizers (as _export_adam_state does for the
        full-graph engine); W_D1 keeps loss2's last gradient as .grad, as after the autograd loop."""
        opts = list(optimizer) if isinstance(optimizer, (list, tuple)) else [optimizer, optimizer]
        for opt, st, p in zip(opts, self.adam, (self.wd1, self.wd2)):
            if st['steps']:
                opt.state[p] = {'step': torch.tensor(float(st['steps'])), 'exp_avg': st['m'].clone(),
                                'exp_avg_sq': st['v'].clone()}
        self.wd1.grad = self.g1.clone() if self.g1_live else None
        self.wd2.grad = None


def _step_log(epoch, sums, div, alpha):
    """The autograd loop's step log from the four squared-difference sums (fp32 means, as MSELoss computes them)."""
    f = np.float32
    with np.errstate(divide='ignore', invalid='ignore'):
        r1, l1, r2, l2 = (f(s) / f(d) for s, d in zip(sums, div))
        loss1 = f(alpha) * r1 + f(1 - alpha) * l1
        loss2 = f(alpha) * r2 + f(1 - alpha) * l2
        return {'Epoch': epoch, 'train_loss': float(loss1 + loss2), 'train_loss_l': float(l1 + l2),
                'train_loss_r': float(r1 + r2)}


def train_minibatch_fused(trainer, model, data, optimizer, args, step_hook=None):
    """framework.trainer.sampler.train_minibatch with the batch step on the HIP kernels: same sampler and negatives
    (same random stream), same update order, logs, validation and checkpoints."""
    from .framework.trainer import sampler as S
    from .framework.trainer._log import wandb_log
    from .framework.trainer.base import _require_gpu, device
    from .framework.trainer.gnndelete_nodeemb import _adam_hyper, _non_df_masks
    _require_gpu()
    data = data.to('cpu')
    _non_df_masks(data)
    data.edge_index = data.train_pos_edge_index
    data.node_id = torch.arange(data.x.shape[0])
    loader = S.make_sampler(data, args.batch_size, args.num_steps)
    model = model.to(device)
    lr, betas, eps = _adam_hyper(optimizer)
    step = MinibatchNodeembStep(model, data, loader, trainer.args.alpha, lr, betas, eps,
                                max_nodes=(loader.walk_length + 1) * max(int(loader.batch_size), 1))
    step.import_adam_state(optimizer)
    trainer._fused_minibatch_step = step
    best_metric = 0
    trainer.trainer_log['steps'] = []
    for epoch in range(args.epochs):
        model.train()
        hist = torch.zeros(max(len(loader), 1), 4, dtype=torch.float32, device=device)
        divs = []
        for i, nodes in enumerate(loader.node_sets()):
            if i >= hist.shape[0]:
                hist = torch.cat([hist, torch.zeros_like(hist)])
            divs.append(step.step(nodes, hist[i]))
            if step_hook is not None:
                step_hook(step)
        sums = {'loss': 0.0, 'loss_l': 0.0, 'loss_r': 0.0}
        for s4, div in zip(hist[:len(divs)].tolist(), divs):
            step_log = _step_log(epoch, s4, div, trainer.args.alpha)
            wandb_log(step_log)
            trainer.trainer_log['steps'].append(step_log)
            sums['loss'] += step_log['train_loss']
            sums['loss_l'] += step_log['train_loss_l']
            sums['loss_r'] += step_log['train_loss_r']
        steps = len(divs)
        if (epoch + 1) % args.valid_freq == 0:
            valid_loss, dt_auc, dt_aup, df_auc, df_aup, df_logit, _, valid_log = trainer.eval(model, data, 'val')
            denom = max(steps - 1, 1)          # upstream divides by the last enumerate index
            train_log = {'epoch': epoch, 'train_loss': sums['loss'] / denom, 'train_loss_l': sums['loss_l'] / denom,
                         'train_loss_r': sums['loss_r'] / denom}
            trainer._record(train_log, valid_log)
            if dt_auc + df_auc > best_metric:
                best_metric = dt_auc + df_auc
                torch.save({'model_state': model.state_dict()}, os.path.join(args.checkpoint_dir, 'model_best.pt'))
            data = data.to('cpu')
    step.export_adam_state(optimizer)
    torch.save({'model_state': {k: v.to('cpu') for k, v in model.state_dict().items()}},
               os.path.join(args.checkpoint_dir, 'model_final.pt'))


# ------------------------------------------------------------------------------------------------ edge-probability batches
def fused_minibatch_edgeprob_unsupported(model, args, optimizer):
    """None when the fused edge-probability batch step applies, else the reason it does not (one line): the rules of
    edgeprob.fused_edgeprob_unsupported."""
    from .edgeprob import fused_edgeprob_unsupported
    reason = fused_edgeprob_unsupported(model, args, optimizer)
    if reason is not None:
        reason = reason.replace('fused edge-probability step', 'fused edge-probability batch step')
    return reason


class MinibatchEdgeprobStep(_BatchStep):
    """The batch step of GNNDeleteTrainer.train_minibatch (the edge-probability loop): forward on the batch's S_Df edges,
    gd_edgeprob_batch_loss_f32 over [Df edges | negatives | S_Df edges with src < dst] against z_ori - the embedding of
    the WHOLE graph, read at the batch-local ids (upstream's quirk) -, EdgeprobEngine's backward on the batch CSR and one
    Adam step on both Del weights."""

    def __init__(self, model, data, loader, z_ori, lr, betas, eps, max_nodes=None):
        super().__init__(model, data, loader, lr, betas, eps, max_nodes)
        self.z_ori = ops._f32_rows(z_ori.detach().to(self.dev)).contiguous()
        if self.H % 4 or self.O % 4 or self.z_ori.shape[1] != self.O:
            raise ValueError(f'MinibatchEdgeprobStep: widths {self.H} / {self.O} must be multiples of 4')
        self.z = None                   # the last batch's embedding (node_embeddings.pt)

    def step(self, nodes, losses):
        """One batch on `nodes`; losses [3] receives (0.5 loss_e + 0.5 loss_l, loss_e, loss_l) on the device."""
        from .framework.trainer import sampler as S
        L, dev = _lib.lib(), self.dev
        self._mark('start')
        c = self.cut
        cnt = c.cut(nodes)
        n_b, k, n_s1, n_s2, n_cand = cnt[0], cnt[3], cnt[4], cnt[5], cnt[9]
        self._mark('cut')
        g = c.batch_csr(True, self.gat)
        self._mark('csr')
        O = self.O
        idx1, idx2 = c.rows(0, n_s1), c.rows(1, n_s2)
        slope1, slope2 = (self.slope1, self.slope2) if self.gat else (0.0, 0.0)
        # forward: frozen layer 1 gathered from the per-run table, Del 1 on S1, conv2 with the ReLU, Del 2 on S2
        h1 = self.h1_all.index_select(0, c.nodes)
        sc1 = None
        if self.gat:
            a1 = self.a1_all.index_select(0, c.nodes)
            sc1 = (a1[:, 0].contiguous(), a1[:, 1].contiguous())
        p1, _ = self._agg(g, h1, sc1, self.b1, slope1)
        wd1, wd2 = self.wd1.data, self.wd2.data
        z1 = p1.clone()
        if n_s1:
            ops.rows_gemm(p1, idx1, wd1, out=z1)
        p2, h2, sc2, alpha2 = self._layer2(g, z1)
        z2 = p2.clone()
        if n_s2:
            ops.rows_gemm(p2, idx2, wd2, out=z2)
        self.z = z2
        self._mark('forward')
        edge_index, _ = c.batch_edges()
        neg = S.negative_sampling(edge_index, n_b, k).to(dev, torch.int64).contiguous()
        self._mark('negatives')
        # loss stage: both terms, the incidence list of what counts, dL/dz2
        n_w = 2 * k + n_cand
        dec = torch.empty(2, max(n_w, 1), dtype=torch.int64, device=dev)
        w = torch.empty(max(n_w, 1), dtype=torch.float32, device=dev)
        w_inc = torch.empty(max(2 * n_w, 1), dtype=torch.float32, device=dev)
        other = torch.empty(max(2 * n_w, 1), dtype=torch.int32, device=dev)
        src_edge = torch.empty(max(2 * n_w, 1), dtype=torch.int32, device=dev)
        inc_ptr = torch.empty(n_b + 1, dtype=torch.int64, device=dev)
        inc_ws = self._ws('incidence', L.gd_edge_incidence_workspace(n_b, n_w))
        ws = self._ws('loss', 4 * L.gd_edgeprob_batch_loss_workspace(k, n_cand, O))
        check(L.gd_edgeprob_batch_loss_f32(ptr(z2), z2.stride(0), n_b, ptr(self.z_ori), self.z_ori.stride(0), self.z_ori.shape[0], O,
                                           ptr(c.df_index), c.e_cap, ptr(neg), neg.stride(0) if k else 0, k, ptr(c.sdf_src),
                                           ptr(c.sdf_dst), n_cand, 0.5, 0.5, ptr(dec), dec.stride(0), ptr(w), ptr(losses),
                                           ptr(inc_ptr), ptr(other), ptr(src_edge), ptr(w_inc), ptr(inc_ws), inc_ws.numel(),
                                           ptr(ws), stream_ptr(dev)), 'gd_edgeprob_batch_loss_f32')
        gz = torch.empty(n_b, O, dtype=torch.float32, device=dev)
        check(L.gd_edge_dot_bwd_f32(ptr(z2), z2.stride(0), O, ptr(other), ptr(w_inc), None, 0, None, ptr(inc_ptr), n_b, ptr(gz),
                                    gz.stride(0), stream_ptr(dev)), 'gd_edge_dot_bwd_f32')
        self._mark('loss')
        # backward: Del 2, conv2 to its input, the ReLU gate folded into Del 1's weight gradient.  The Del layer's autograd node
        # always returns a weight gradient (zeros without rows), so Adam steps both weights on every batch.
        if n_s2:
            ops.rows_gemm_wgrad(p2, idx2, gz, idx2, n_s2, out=self.g2)
            ops.rows_gemm(gz, idx2, wd2, trans_w=True, out=gz)
        else:
            self.g2.zero_()
        if n_s1:
            dh2 = self._agg_bwd(g, h2, sc2, alpha2, gz, slope2, self.att2 if self.gat else None)
            dx1 = ops.rows_gemm(dh2, None, self.w2)                  # [n_b, H], before the ReLU gate
            ops.rows_gemm_wgrad(p1, idx1, dx1, idx1, n_s1, relu_mask=z1, out=self.g1)
        else:
            self.g1.zero_()
        self._adam(0, self.wd1, self.g1)
        self._adam(1, self.wd2, self.g2)
        self._mark('backward')

    # ---------------------------------------------------------------------------------------------- optimizer state
    def import_adam_state(self, optimizer):
        for st, p in zip(self.adam, (self.wd1, self.wd2)):
            have = optimizer.state.get(p)
            if have and 'exp_avg' in have:
                st['m'].copy_(have['exp_avg'])
                st['v'].copy_(have['exp_avg_sq'])
                st['steps'] = int(have['step'])
                st['step'].fill_(st['steps'])

    def export_adam_state(self, optimizer):
        """Adam moments and step count into the caller's optimizer; no gradient is kept (the loop's zero_grad)."""
        for st, p in zip(self.adam, (self.wd1, self.wd2)):
            if st['steps']:
                optimizer.state[p] = {'step': torch.tensor(float(st['steps'])), 'exp_avg': st['m'].clone(),
                                      'exp_avg_sq': st['v'].clone()}
            p.grad = None


def train_minibatch_edgeprob_fused(trainer, model, data, z_ori, optimizer, args, step_hook=None):
    """The epoch loop of GNNDeleteTrainer.train_minibatch with the batch step on the HIP kernels: same sampler and
    negatives (same random stream), same epoch records (upstream's double division and swapped names), model selection,
    checkpoints and optimizer state.  data: on the host, edge_index / node_id set as the loop sets them."""
    import time
    from .framework.trainer import sampler as S
    from .framework.trainer.base import device
    from .framework.trainer.gnndelete_nodeemb import _adam_hyper
    loader = S.make_sampler(data, args.batch_size, args.num_steps)
    lr, betas, eps = _adam_hyper(optimizer)
    step = MinibatchEdgeprobStep(model, data, loader, z_ori, lr, betas, eps,
                                 max_nodes=(loader.walk_length + 1) * max(int(loader.batch_size), 1))
    step.import_adam_state(optimizer)
    trainer._fused_minibatch_step = step
    best_metric = 0
    trainer.trainer_log['steps'] = []
    for epoch in range(args.epochs):
        model.train()
        start = time.time()
        hist = torch.zeros(max(len(loader), 1), 3, dtype=torch.float32, device=device)
        done = 0
        for i, nodes in enumerate(loader.node_sets()):
            if i >= hist.shape[0]:
                hist = torch.cat([hist, torch.zeros_like(hist)])
            step.step(nodes, hist[i])
            done += 1
            if step_hook is not None:
                step_hook(step)
        step_logs = [{'loss': r[0], 'loss_e': r[1], 'loss_l': r[2]} for r in hist[:done].tolist()]   # the epoch's host read
        trainer.trainer_log['steps'].extend(step_logs)
        if (epoch + 1) % args.valid_freq == 0:
            step.export_adam_state(optimizer)               # (a checkpoint below carries the optimizer's state)
            valid_loss, dt_auc, dt_aup, df_auc, df_aup, df_logit, _, valid_log = trainer.eval(model, data, 'val')
            div = max(len(step_logs) - 1, 1)                # upstream divides by the last enumerate index, twice
            tot = {k_: sum(s_[k_] for s_ in step_logs) / div for k_ in ('loss', 'loss_e', 'loss_l')}
            trainer._record({'epoch': epoch, 'train_loss': tot['loss'] / div, 'train_loss_l': tot['loss_e'] / div,
                             'train_loss_e': tot['loss_l'] / div, 'train_time': (time.time() - start) / div / div}, valid_log)
            if dt_auc + df_auc > best_metric:
                best_metric = dt_auc + df_auc
                print(f'Save best checkpoint at epoch {epoch:04d}. Valid loss = {valid_loss:.4f}')
                torch.save({'model_state': model.state_dict(), 'optimizer_state': optimizer.state_dict()},
                           os.path.join(args.checkpoint_dir, 'model_best.pt'))
                if step.z is not None:
                    torch.save(step.z.detach(), os.path.join(args.checkpoint_dir, 'node_embeddings.pt'))
            data = data.to('cpu')
    step.export_adam_state(optimizer)
    torch.save({'model_state': {k_: v.to('cpu') for k_, v in model.state_dict().items()},
                'optimizer_state': optimizer.state_dict()}, os.path.join(args.checkpoint_dir, 'model_final.pt'))


# ------------------------------------------------------------------------------------------------ backbone batches
def fused_minibatch_backbone_unsupported(model, args, optimizer):
    """None when the fused backbone batch step applies (Trainer.train_minibatch with --fused_minibatch), else the reason it
    does not (one line): the rules of backbone.fused_backbone_unsupported for a model that trains on batches."""
    from .framework.trainer.sampler import data_parallel_world
    from .nn import GATConv, GCNConv
    conv1, conv2 = getattr(model, 'conv1', None), getattr(model, 'conv2', None)
    if (not (isinstance(conv1, (GCNConv, GATConv)) and type(conv1) is type(conv2)) or hasattr(model, 'deletion1')
            or hasattr(model, 'node_emb')):
        return f'no fused backbone batch step for the {type(model).__name__} backbone (GCN and GAT only)'
    if data_parallel_world()[1] > 1:
        return 'torch.distributed with more than one rank'
    if isinstance(optimizer, (list, tuple)) or type(optimizer) is not torch.optim.Adam or len(optimizer.param_groups) != 1:
        return 'the optimizer is not one plain torch.optim.Adam'
    g = optimizer.param_groups[0]
    if g.get('weight_decay', 0):
        return 'Adam with weight decay'
    if g.get('amsgrad') or g.get('maximize'):
        return 'Adam with amsgrad / maximize'
    if {id(p) for p in g['params']} != {id(p) for p in model.parameters()} or not all(p.requires_grad for p in g['params']):
        return 'the optimizer does not hold exactly the model\'s parameters'
    hid, out = conv1.out_channels, conv2.out_channels
    if hid % 4 or out % 4 or max(hid, out) > 1024:
        return f'widths {hid} / {out} (multiples of 4 up to 1024)'
    if conv1.in_channels > 1024:
        return f'input width {conv1.in_channels} (the gathering first product takes up to 1024)'
    return None


class MinibatchBackboneStep(_BatchLayers):
    """One batch of Trainer.train_minibatch (BCE link prediction on the batch's edges against one negative per edge) with an
    explicit forward, BackboneEngine's hand-derived backward and the library's Adam on every parameter of the model, which
    is stepped in place.  Shapes change per batch: eager launches, no captured graph.

      cut, CSR over all batch edges;  t1 = x[nodes] W1^T (gd_rows_gather_gemm_f32: layer 1 trains, no per-run table);
      p1 = A t1 + b1;  t2 = relu(p1) W2^T;  z = A t2 + b2 (GAT: row dots + gd_gat_aggregate_f32 per layer);
      negatives from sampler.negative_sampling;  incidence list over [edges | negatives];  gd_edge_bce_f32 -> the caller's
      loss slot;  g = dL/dz;  the backward of BackboneEngine._iteration_gcn / _iteration_gat on the batch CSR, dW1 = q1^T
      x[nodes] through the weight-gradient entry's index list;  one gd_adam_f32 per parameter."""

    def __init__(self, model, data, loader, lr, betas, eps, max_nodes=None):
        from .nn import GATConv
        dev = next(model.parameters()).device
        self.dev, self.model = dev, model
        self.lr, self.betas, self.eps = float(lr), (float(betas[0]), float(betas[1])), float(eps)
        c1, c2 = self.convs = (model.conv1, model.conv2)
        self.gat = isinstance(c1, GATConv)
        self.cut = BatchCut(data, loader, dev, max_nodes)
        self.x = ops._f32_rows(data.x.to(dev, torch.float32))
        self.w1, self.w2 = ((c.lin_src if self.gat else c.lin).weight for c in self.convs)         # [H, F], [O, H]
        F_in, H, O = self.F, self.H, self.O = int(self.w1.shape[1]), int(self.w1.shape[0]), int(self.w2.shape[0])
        if H % 4 or O % 4 or max(H, O, F_in) > 1024 or int(self.x.shape[1]) != F_in or int(self.w2.shape[1]) != H:
            raise ValueError(f'MinibatchBackboneStep: widths {F_in} -> {H} -> {O} (hidden and output: multiples of 4; all up '
                             'to 1024)')
        self.params = list(model.parameters())
        self.grads = {id(p): torch.zeros_like(p.data) for p in self.params}
        self.adam = [{'m': torch.zeros_like(p.data), 'v': torch.zeros_like(p.data),
                      'step': torch.zeros(1, dtype=torch.int32, device=dev), 'steps': 0} for p in self.params]
        self._bufs = {}
        self.events = None              # list -> (stage, cuda event) pairs are appended (stage split of the experiment)
        self.z = None                   # the last batch's embedding (node_embeddings.pt)

    def _grad(self, p):
        return self.grads[id(p)]

    def _att(self, c):
        return c.att_src.data.view(-1), c.att_dst.data.view(-1)

    def _layer(self, k, g, h):
        """conv k's aggregation of the transformed rows h -> (y, scores, saved attention)."""
        c = self.convs[k]
        scores = ops.row_dots(h, *self._att(c)) if self.gat else None
        y, alpha = self._agg(g, h, scores, c.bias.data, float(c.negative_slope) if self.gat else 0.0)
        return y, scores, alpha

    def _layer_bwd(self, k, g, h, scores, alpha, dy):
        """conv k's backward from dy -> dL/dh; GAT's attention-vector gradients go into their buffers."""
        c = self.convs[k]
        if not self.gat:
            return self._agg_bwd(g, h, None, None, dy, 0.0, None)
        return self._agg_bwd(g, h, scores, alpha, dy, float(c.negative_slope), self._att(c),
                             att_grads=(self._grad(c.att_src), self._grad(c.att_dst)))

    # ---------------------------------------------------------------------------------------------- one batch
    @torch.no_grad()
    def step(self, nodes, loss_slot):
        """One batch on `nodes`; loss_slot (one fp32 element on the device) receives the batch's BCE loss, NaN for a batch
        without decoded edges (the loop's mean over nothing), whose gradients are zero and whose Adam step still runs."""
        from .backbone import col_sum
        from .framework.trainer import sampler as S
        L, dev = _lib.lib(), self.dev
        self._mark('start')
        c = self.cut
        cnt = c.cut(nodes)
        n_b, e_b = cnt[0], cnt[1]
        self._mark('cut')
        g = c.batch_csr(False, self.gat)
        self._mark('csr')
        c1, c2 = self.convs
        w1, w2, H, O = self.w1.data, self.w2.data, self.H, self.O
        t1 = ops.rows_gather_gemm(self.x, c.nodes, w1)
        p1, sc1, al1 = self._layer(0, g, t1)
        t2 = ops.rows_gemm(p1, None, w2, trans_w=True, relu_in=True)
        z, sc2, al2 = self._layer(1, g, t2)
        self.z = z
        self._mark('forward')
        edges = c.e_index[:, :e_b]
        neg = S.negative_sampling(edges, n_b, e_b).to(dev, torch.int64)
        m_all = e_b + int(neg.shape[1])
        self._mark('negatives')
        if m_all == 0:
            loss_slot.fill_(float('nan'))
            for p in self.params:
                self._grad(p).zero_()
            self._mark('loss')
        else:
            dec = torch.cat([edges, neg], 1)                            # [2, M] contiguous: [batch edges | negatives]
            inc_ptr = torch.empty(n_b + 1, dtype=torch.int64, device=dev)
            other = torch.empty(2 * m_all, dtype=torch.int32, device=dev)
            src_edge = torch.empty(2 * m_all, dtype=torch.int32, device=dev)
            inc_ws = self._ws('incidence', L.gd_edge_incidence_workspace(n_b, m_all))
            check(L.gd_edge_incidence(ptr(dec[0]), ptr(dec[1]), m_all, n_b, ptr(inc_ptr), ptr(other), ptr(src_edge), ptr(inc_ws),
                                      inc_ws.numel(), stream_ptr(dev)), 'gd_edge_incidence')
            w = torch.empty(m_all, dtype=torch.float32, device=dev)
            w_inc = torch.empty(2 * m_all, dtype=torch.float32, device=dev)
            bce_ws = self._ws('bce', 4 * max(1, L.gd_edge_bce_workspace(m_all, O)))
            check(L.gd_edge_bce_f32(ptr(z), z.stride(0), n_b, O, ptr(dec), m_all, e_b, dec.data_ptr() + 8 * e_b, m_all,
                                    m_all - e_b, 1.0, ptr(w), ptr(loss_slot), ptr(src_edge), ptr(inc_ptr), ptr(w_inc),
                                    ptr(bce_ws), stream_ptr(dev)), 'gd_edge_bce_f32')
            gz = torch.empty(n_b, O, dtype=torch.float32, device=dev)
            check(L.gd_edge_dot_bwd_f32(ptr(z), z.stride(0), O, ptr(other), ptr(w_inc), None, 0, None, ptr(inc_ptr), n_b,
                                        ptr(gz), gz.stride(0), stream_ptr(dev)), 'gd_edge_dot_bwd_f32')
            self._mark('loss')
            # BackboneEngine's backward on the batch: db2, layer 2 to its input, dW2, the ReLU gate with db1, layer 1, dW1
            col_sum(gz, out=self._grad(c2.bias))
            q2 = self._layer_bwd(1, g, t2, sc2, al2, gz)
            ops.rows_gemm_wgrad(q2, None, p1, None, n_b, relu_mask=p1, out=self._grad(self.w2))
            dx1 = ops.rows_gemm(q2, None, w2)
            col_sum(dx1, gate=p1, gated=dx1, out=self._grad(c1.bias))                   # dp1 in place, db1
            q1 = self._layer_bwd(0, g, t1, sc1, al1, dx1)
            ops.rows_gemm_wgrad(q1, None, self.x, c.nodes.to(torch.int32), n_b, out=self._grad(self.w1))
        for st, p in zip(self.adam, self.params):
            check(L.gd_adam_f32(ptr(p.data), ptr(self._grad(p)), ptr(st['m']), ptr(st['v']), ptr(st['step']), p.numel(), self.lr,
                                self.betas[0], self.betas[1], self.eps, stream_ptr(dev)), 'gd_adam_f32')
            st['steps'] += 1
        self._mark('backward')

    # ---------------------------------------------------------------------------------------------- optimizer state
    def import_adam_state(self, optimizer):
        for st, p in zip(self.adam, self.params):
            have = optimizer.state.get(p)
            if have and 'exp_avg' in have:
                st['m'].copy_(have['exp_avg'])
                st['v'].copy_(have['exp_avg_sq'])
                st['steps'] = int(have['step'])
                st['step'].fill_(st['steps'])

    def export_adam_state(self, optimizer):
        """Adam moments and step count of every parameter into the caller's optimizer; no gradient is kept (the loop's
        zero_grad after the step)."""
        for st, p in zip(self.adam, self.params):
            if st['steps']:
                optimizer.state[p] = {'step': torch.tensor(float(st['steps'])), 'exp_avg': st['m'].clone(),
                                      'exp_avg_sq': st['v'].clone()}
            p.grad = None


def train_minibatch_backbone_fused(trainer, model, data, optimizer, args, step_hook=None):
    """Trainer.train_minibatch with the batch step on the HIP kernels: same sampler and negatives (same random stream), same
    step and epoch records (the losses are read once per epoch), validation, best-validation-loss checkpoint, final
    checkpoint and optimizer state."""
    import time
    from .framework.trainer import sampler as S
    from .framework.trainer._log import wandb_log
    from .framework.trainer.base import _require_gpu, device
    from .framework.trainer.gnndelete_nodeemb import _adam_hyper
    _require_gpu()
    start = time.time()
    best_valid_loss, best_epoch = 1000000, 0
    model = model.to(device)
    data = data.to('cpu')
    data.edge_index = data.train_pos_edge_index
    loader = S.make_sampler(data, args.batch_size, args.num_steps)
    lr, betas, eps = _adam_hyper(optimizer)
    step = MinibatchBackboneStep(model, data, loader, lr, betas, eps,
                                 max_nodes=(loader.walk_length + 1) * max(int(loader.batch_size), 1))
    step.import_adam_state(optimizer)
    trainer._fused_minibatch_step = step
    trainer.trainer_log['steps'] = []
    for epoch in range(args.epochs):
        model.train()
        hist = torch.zeros(max(len(loader), 1), dtype=torch.float32, device=device)
        done = 0
        for i, nodes in enumerate(loader.node_sets()):
            if i >= hist.shape[0]:
                hist = torch.cat([hist, torch.zeros_like(hist)])
            step.step(nodes, hist[i:i + 1])
            done += 1
            if step_hook is not None:
                step_hook(step)
        epoch_loss = 0.0
        for i, loss in enumerate(hist[:done].tolist()):                  # the epoch's host read
            rec = {'epoch': epoch, 'step': i, 'train_loss': loss}
            wandb_log(rec)
            trainer.trainer_log['steps'].append(rec)
            epoch_loss += loss
        if (epoch + 1) % args.valid_freq == 0:
            step.export_adam_state(optimizer)               # (a checkpoint below carries the optimizer's state)
            valid_loss, *_, valid_log = trainer.eval(model, data, 'val')
            trainer._record({'epoch': epoch, 'train_loss': epoch_loss / max(done - 1, 1)}, valid_log)
            if valid_loss < best_valid_loss:
                best_valid_loss, best_epoch = valid_loss, epoch
                print(f'Save best checkpoint at epoch {epoch:04d}. Valid loss = {valid_loss:.4f}')
                torch.save({'model_state': model.state_dict(), 'optimizer_state': optimizer.state_dict()},
                           os.path.join(args.checkpoint_dir, 'model_best.pt'))
                torch.save(step.z.detach(), os.path.join(args.checkpoint_dir, 'node_embeddings.pt'))
            data = data.to('cpu')
    step.export_adam_state(optimizer)
    trainer.trainer_log['training_time'] = time.time() - start
    torch.save({'model_state': model.state_dict(), 'optimizer_state': optimizer.state_dict()},
               os.path.join(args.checkpoint_dir, 'model_final.pt'))
    trainer.trainer_log['best_epoch'], trainer.trainer_log['best_valid_loss'] = best_epoch, best_valid_loss


# ------------------------------------------------------------------------------------------------ knowledge-graph batches
N_COUNTS_KG = 6        # gd_induced_subgraph_typed's count vector


def fused_minibatch_kg_unsupported(model, args, optimizer):
    """None when the fused knowledge-graph batch step applies (KGGNNDeleteNodeembTrainer.train with --fused_minibatch), else the
    reason it does not (one line)."""
    from .framework.trainer.sampler import data_parallel_world
    from .nn import RGCNConv
    conv1, conv2 = getattr(model, 'conv1', None), getattr(model, 'conv2', None)
    if (not (type(conv1) is RGCNConv and type(conv2) is RGCNConv) or not hasattr(model, 'deletion1')
            or not hasattr(model, 'node_emb')):
        return f'no fused knowledge-graph batch step for the {type(model).__name__} backbone (R-GCN only)'
    if getattr(args, 'loss_fct', 'mse_mean') not in ('mse_mean', 'mse_sum'):
        return f'--loss_fct {args.loss_fct} is not an MSE loss'
    if getattr(args, 'loss_type', 'both_layerwise') != 'both_layerwise':
        return f'--loss_type {args.loss_type} (the fused step is the layer-wise update)'
    for conv in (conv1, conv2):
        nb = 1 if conv.num_blocks is None else int(conv.num_blocks)
        d_in, d_out = int(conv.in_channels), int(conv.out_channels)
        if not (0 < d_in <= 128 and 0 < d_out <= 128 and d_in % nb == 0 and d_out % nb == 0 and (d_in // nb) % 2 == 0
                and (d_out // nb) % 2 == 0):
            return f'widths {d_in} -> {d_out} in {nb} blocks (gd_rgcn_conv_f32 takes even block widths up to 128 floats)'
    if not isinstance(optimizer, (list, tuple)) or len(optimizer) != 2:
        return 'the optimizer is not two plain torch.optim.Adam'
    for opt, p in zip(optimizer, (model.deletion1.deletion_weight, model.deletion2.deletion_weight)):
        g = opt.param_groups[0]
        if (type(opt) is not torch.optim.Adam or len(opt.param_groups) != 1 or g.get('weight_decay', 0) or g.get('amsgrad')
                or g.get('maximize') or [id(q) for q in g['params']] != [id(p)]):
            return 'the optimizer is not two plain torch.optim.Adam'
    if data_parallel_world()[1] > 1:
        return 'torch.distributed with more than one rank'
    return None


class _TypedBatchGraph:
    __slots__ = ('n', 'n_edges', 'fwd', 'bwd', 'status')


class KGBatchCut:
    """The device side of a knowledge-graph GraphSAINT batch: the sampler's source-major CSR with one relation type and one
    flag byte per edge (packed once per run), the node-sized relabel array, and buffers for gd_induced_subgraph_typed's
    outputs (node buffers sized to the batch upper bound, edge buffers grown geometrically when a cut reports more)."""

    def __init__(self, data, loader, dev, num_edge_type, max_nodes=None):
        self.dev = dev
        self.n = int(loader.n)
        self.num_edge_type = int(num_edge_type)
        self.rowptr32 = loader.rowptr.to(device=dev, dtype=torch.int32).contiguous()
        self.col32 = loader.dst_sorted.to(device=dev, dtype=torch.int32).contiguous()
        order = loader.order.to(data.edge_type.device)
        self.edge_type32 = data.edge_type[order].to(device=dev, dtype=torch.int32).contiguous()
        flags = data.dr_mask.to(torch.uint8) | (data.df_mask.to(torch.uint8) << 1)
        self.edge_flags = flags[order.to(flags.device)].to(dev).contiguous()
        node_flags = (data.sdf_node_1hop_mask_non_df_mask.to('cpu', torch.uint8)
                      | (data.sdf_node_2hop_mask_non_df_mask.to('cpu', torch.uint8) << 1))
        self.node_flags = node_flags.to(dev).contiguous()
        self.relabel = torch.zeros(self.n, dtype=torch.int64, device=dev)
        self.generation = 0
        self.counts = torch.zeros(N_COUNTS_KG, dtype=torch.int32, device=dev)
        self.n_cap = self.e_cap = 0
        self._bufs = {}
        self._ensure(max_nodes or 1024, 4 * (max_nodes or 1024))
        self.reads = 0                  # blocking host reads made by the cut (the count vector)

    _ws = BatchCut._ws

    def _ensure(self, n_b, e):
        if n_b <= self.n_cap and e <= self.e_cap:
            return
        self.n_cap, self.e_cap = max(self.n_cap, _grow(n_b)), max(self.e_cap, _grow(e))
        dev, n, c = self.dev, self.n_cap, self.e_cap
        self.dr = torch.empty(3, c, dtype=torch.int32, device=dev)              # src, dst, type
        self.df_index = torch.empty(2, c, dtype=torch.int64, device=dev)
        self.df_type = torch.empty(c, dtype=torch.int64, device=dev)
        self.row_lists = torch.empty(2 * n, dtype=torch.int32, device=dev)      # list k at k * n_b
        self.seg_row = torch.arange(n, dtype=torch.int32, device=dev)

    def cut(self, nodes):
        """gd_induced_subgraph_typed on one sorted, unique node set -> the host copy of the count vector."""
        nodes = nodes.to(self.dev, torch.int64).contiguous()
        n_b = int(nodes.numel())
        self._ensure(n_b, 0)
        self.generation += 1
        L = _lib.lib()
        while True:
            ws = self._ws('cut', L.gd_induced_subgraph_typed_workspace(n_b))
            check(L.gd_induced_subgraph_typed(ptr(self.rowptr32), ptr(self.col32), ptr(self.edge_type32), ptr(self.edge_flags),
                                              self.n, self.num_edge_type, ptr(nodes), n_b, ptr(self.node_flags), self.generation,
                                              ptr(self.relabel), self.e_cap, ptr(self.dr[0]), ptr(self.dr[1]), ptr(self.dr[2]),
                                              ptr(self.df_index), ptr(self.df_type), ptr(self.row_lists), ptr(self.counts), ptr(ws),
                                              ws.numel(), stream_ptr(self.dev)), 'gd_induced_subgraph_typed')
            cnt = self.counts.tolist()
            self.reads += 1
            if max(cnt[1], cnt[2]) <= self.e_cap:
                break
            self._ensure(n_b, max(cnt[1], cnt[2]))         # the edge outputs were not written: grow, cut again
        if cnt[5]:
            raise IndexError(f'batch node ids outside [0, {self.n})')
        self.nodes, self.cnt = nodes, cnt
        return cnt

    def rows(self, k, count):
        """Batch rows of the latest cut with node flag bit k (0: list 1, 1: list 2), ascending: int32 [count]."""
        n_b = self.cnt[0]
        return self.row_lists[k * n_b:k * n_b + count]

    def typed_graph(self, n_rel):
        """gd_batch_typed_csr over the latest cut's Dr edges: the arrays of graph.TypedNodeCSR(...).fwd / .bwd."""
        return batch_typed_csr(self.dr[0], self.dr[1], self.dr[2], self.cnt[1], self.cnt[0], n_rel, self._bufs)


def batch_typed_csr(src, dst, etype, n_edges, n_nodes, n_rel, bufs=None, into=None):
    """gd_batch_typed_csr on n_edges typed edges (int32 device arrays) -> a _TypedBatchGraph whose fwd / bwd are
    (node_ptr, seg_ptr, seg_rel, col, w) with room for n_edges runs; status [4] stays on the device.  into: a graph of the
    same sizes whose arrays are written again."""
    dev = src.device
    L = _lib.lib()
    e = int(n_edges)
    g = into
    if g is None or (g.n, g.n_edges) != (int(n_nodes), e):
        g = _TypedBatchGraph()
        g.n, g.n_edges = int(n_nodes), e
        i32 = dict(dtype=torch.int32, device=dev)
        sides = []
        for _ in range(2):
            sides.append((torch.empty(g.n + 1, **i32), torch.empty(e + 1, **i32), torch.empty(max(e, 1), **i32),
                          torch.empty(max(e, 1), **i32), torch.empty(max(e, 1), dtype=torch.float32, device=dev)))
        g.fwd, g.bwd = sides
        g.status = torch.empty(4, **i32)
    nbytes = L.gd_batch_typed_csr_workspace(g.n, e, int(n_rel))
    if nbytes < 0:
        raise ValueError('batch_typed_csr: batch too large for int32 indices')
    if bufs is None:
        ws = torch.empty(max(256, nbytes), dtype=torch.uint8, device=dev)
    else:
        ws = bufs.get('typed_csr')
        if ws is None or ws.numel() < nbytes:
            ws = bufs['typed_csr'] = torch.empty(max(256, _grow(nbytes)), dtype=torch.uint8, device=dev)
    check(L.gd_batch_typed_csr(ptr(src), ptr(dst), ptr(etype), e, g.n, int(n_rel), max(e, 1), e, *(ptr(t) for t in g.fwd),
                               *(ptr(t) for t in g.bwd), ptr(g.status), ptr(ws), ws.numel(), stream_ptr(dev)),
          'gd_batch_typed_csr')
    return g


class MinibatchKGNodeembStep(_BatchLayers):
    """One batch of KGGNNDeleteNodeembTrainer.train (gnndelete_nodeemb.py:659-846 of the reference) with an explicit forward, a
    hand-derived backward and the library's Adam: the typed cut, the batch's two typed graphs, both R-GCN convs on
    gd_rgcn_conv_f32 (root and bias through the row GEMM), the Del rows, negatives from utils.negative_sampling_kg, DEC + NI of
    both layers on gd_batch_loss_terms + gd_rowpair_mse_f32, then loss 1 -> Adam on W_D1, loss 2 -> Adam on W_D2 while its
    W_D1 gradient (through conv2 transposed, the ReLU gate and the Del-1 rows) waits for the next batch.  Shapes change per
    batch: eager launches, no captured graph, one blocking host read (the count vector)."""

    def __init__(self, model, data, loader, num_edge_type, alpha, reduction, lr, betas, eps, max_nodes=None):
        dev = next(model.parameters()).device
        self.dev, self.model, self.gat = dev, model, False
        self.lr, self.betas, self.eps = float(lr), (float(betas[0]), float(betas[1])), float(eps)
        self.alpha, self.reduction = float(alpha), reduction
        self.cut = KGBatchCut(data, loader, dev, num_edge_type, max_nodes)
        c1, c2 = self.convs = (model.conv1, model.conv2)
        self.n_rel = int(c1.num_relations)
        self.nb = tuple(1 if c.num_blocks is None else int(c.num_blocks) for c in self.convs)
        self.emb = model.node_emb.weight.detach().to(torch.float32).contiguous()
        self.emb_ids = data.x.to(dev, torch.int64).reshape(-1).contiguous()
        self.weights = tuple(c.weight.detach().contiguous() for c in self.convs)
        self.roots = tuple(c.root.detach().contiguous() for c in self.convs)              # [in, out]
        self.biases = tuple(c.bias.detach().contiguous() for c in self.convs)
        self.H, self.O = int(c1.out_channels), int(c2.out_channels)
        self.wd1, self.wd2 = model.deletion1.deletion_weight, model.deletion2.deletion_weight
        self.adam = []
        for p in (self.wd1, self.wd2):
            self.adam.append({'m': torch.zeros_like(p.data), 'v': torch.zeros_like(p.data),
                              'step': torch.zeros(1, dtype=torch.int32, device=dev), 'steps': 0})
        self.g1 = torch.zeros_like(self.wd1.data)
        self.g2 = torch.zeros_like(self.wd2.data)
        self.g1_live = False            # W_D1 holds loss2's gradient of the previous batch (carried into the next step)
        self._bufs = {}
        self.events = None              # list -> (stage, cuda event) pairs are appended (stage split of the experiment)

    _adam = _BatchStep._adam
    import_adam_state = MinibatchNodeembStep.import_adam_state
    export_adam_state = MinibatchNodeembStep.export_adam_state

    # ---------------------------------------------------------------------------------------------- layers
    def _typed(self, arrays, x, k, trans, y):
        """y += the typed aggregation of conv k over one side of the batch graph (gd_rgcn_conv_f32, no plan)."""
        node_ptr, seg_ptr, seg_rel, col, w = arrays
        check(_lib.lib().gd_rgcn_conv_f32(ptr(node_ptr), ptr(seg_ptr), ptr(seg_rel), ptr(col), ptr(w), ptr(x), x.stride(0),
                                          x.shape[1], ptr(self.weights[k]), self.nb[k], int(trans), ptr(y), y.stride(0),
                                          y.shape[1], y.shape[0], stream_ptr(self.dev)), 'gd_rgcn_conv_f32')
        return y

    def _conv(self, k, g, x):
        """conv k of the frozen backbone on the batch graph: x root + bias + the per-relation means times W_r."""
        y = ops.rows_gemm(x, None, self.roots[k], trans_w=False, bias=self.biases[k])
        if g.n_edges:
            self._typed(g.fwd, x, k, 0, y)
        return y

    def _loss(self, z, z_ori, neg, n_pos, ni, n_ni, d, sums):
        """DEC + NI of one layer: sums[0] += sum of squared DEC differences, sums[1] += NI's; -> dz of alpha * DEC + (1 - alpha)
        * NI under the run's reduction (a mean over zero rows has no gradient)."""
        L = _lib.lib()
        c = self.cut
        n_b = c.cnt[0]
        n_terms = 2 * n_pos + n_ni
        if self.reduction == 'mean':
            w_dec = self.alpha / (2 * n_pos * d) if n_pos else 0.0
            w_ni = (1.0 - self.alpha) / (n_ni * d) if n_ni else 0.0
        else:
            w_dec, w_ni = self.alpha, 1.0 - self.alpha
        seg_ptr = torch.empty(n_b + 1, dtype=torch.int32, device=self.dev)
        term_o = torch.empty(max(n_terms, 1), dtype=torch.int32, device=self.dev)
        term_w = torch.empty(max(n_terms, 1), dtype=torch.float32, device=self.dev)
        term_kind = torch.empty(max(n_terms, 1), dtype=torch.int32, device=self.dev)
        ws = self._ws('terms', L.gd_batch_loss_terms_workspace(n_b, n_terms))
        check(L.gd_batch_loss_terms(ptr(c.df_index), c.e_cap, ptr(neg), neg.stride(0) if n_pos else 0, n_pos, ptr(ni), n_ni, n_b,
                                    w_dec, w_ni, ptr(seg_ptr), ptr(term_o), ptr(term_w), ptr(term_kind), ptr(ws), ws.numel(),
                                    stream_ptr(self.dev)), 'gd_batch_loss_terms')
        dz = torch.empty(n_b, d, dtype=torch.float32, device=self.dev)
        part = torch.empty(max(1, L.gd_rowpair_mse_workspace(n_b)), dtype=torch.float32, device=self.dev)
        check(L.gd_rowpair_mse_f32(ptr(z), z.stride(0), ptr(z_ori), z_ori.stride(0), d, ptr(seg_ptr), ptr(c.seg_row), n_b,
                                   ptr(term_o), ptr(term_w), ptr(term_kind), ptr(dz), dz.stride(0), 0, ptr(sums), ptr(part),
                                   stream_ptr(self.dev)), 'gd_rowpair_mse_f32')
        return dz

    # ---------------------------------------------------------------------------------------------- one batch
    @torch.no_grad()
    def step(self, nodes, sums):
        """One batch of the layer-wise update on `nodes`; sums [4] (zeroed by the caller) receives the squared-difference
        sums (DEC 1, NI 1, DEC 2, NI 2).  Returns the divisors that turn them into the loop's four loss terms."""
        from .framework import utils as U
        self._mark('start')
        c = self.cut
        cnt = c.cut(nodes)
        n_b, m_df, n_l1, n_l2 = cnt[0], cnt[2], cnt[3], cnt[4]
        self._mark('cut')
        g = c.typed_graph(self.n_rel)
        self._mark('csr')
        H, O = self.H, self.O
        idx1, idx2 = c.rows(0, n_l1), c.rows(1, n_l2)
        wd1, wd2 = self.wd1.data, self.wd2.data
        # forward: the frozen convs on the batch's Dr graph; conv1's output is z1_ori AND the Del-1 input
        x = self.emb.index_select(0, self.emb_ids.index_select(0, c.nodes))
        z1_ori = self._conv(0, g, x)
        z2_ori = self._conv(1, g, torch.relu(z1_ori))
        z1 = z1_ori.clone()
        if n_l1:
            ops.rows_gemm(z1_ori, idx1, wd1, out=z1)
        a1 = torch.relu(z1)
        p2 = self._conv(1, g, a1)
        z2 = p2.clone()
        if n_l2:
            ops.rows_gemm(p2, idx2, wd2, out=z2)
        self._mark('forward')
        dec_index, dec_type = c.df_index[:, :m_df], c.df_type[:m_df]
        neg = U.negative_sampling_kg(edge_index=dec_index, edge_type=dec_type).to(self.dev, torch.int64).contiguous()
        self._mark('negatives')
        dz1 = self._loss(z1, z1_ori, neg, m_df, idx1, n_l1, H, sums[0:2])
        dz2 = self._loss(z2, z2_ori, neg, m_df, idx2, n_l2, O, sums[2:4])
        self._mark('loss')
        # loss1: W_D1's gradient (+ what loss2 left on it last batch), Adam.  The Del layer's autograd node always returns a
        # weight gradient (zeros without rows), so neither parameter is ever skipped by the loop's Adams and none is here.
        if n_l1:
            ops.rows_gemm_wgrad(z1_ori, idx1, dz1, idx1, n_l1, out=self.g1, accumulate=self.g1_live)
        elif not self.g1_live:
            self.g1.zero_()
        self._adam(0, self.wd1, self.g1)
        # loss2: W_D2's gradient and, through conv2 (root + the transposed typed graph), the ReLU gate and the Del-1 rows, a
        # fresh W_D1 gradient that waits for the next batch
        if n_l2:
            ops.rows_gemm_wgrad(p2, idx2, dz2, idx2, n_l2, out=self.g2)
        else:
            self.g2.zero_()
        if n_l1:
            dp2 = dz2.clone()
            if n_l2:
                ops.rows_gemm(dz2, idx2, wd2, trans_w=True, out=dp2)
            dx1 = ops.rows_gemm(dp2, None, self.roots[1], trans_w=True)              # [n_b, H], before the ReLU gate
            if g.n_edges:
                self._typed(g.bwd, dp2, 1, 1, dx1)
            ops.rows_gemm_wgrad(z1_ori, idx1, dx1, idx1, n_l1, relu_mask=z1, out=self.g1)
        else:
            self.g1.zero_()
        self.g1_live = True
        self._adam(1, self.wd2, self.g2)
        self._mark('backward')
        if self.reduction == 'mean':
            return (2 * m_df * H, n_l1 * H, 2 * m_df * O, n_l2 * O)
        return (1, 1, 1, 1)


def _kg_step_log(epoch, sums, div, alpha):
    """The knowledge-graph loop's step record from the four squared-difference sums (fp32, as MSELoss computes them)."""
    f = np.float32
    with np.errstate(divide='ignore', invalid='ignore'):
        r1, l1, r2, l2 = (f(s) / f(d) for s, d in zip(sums, div))
        loss1 = f(alpha) * r1 + f(1 - alpha) * l1
        loss2 = f(alpha) * r2 + f(1 - alpha) * l2
        return {'Epoch': epoch, 'train_loss': float(loss1 + loss2), 'loss_r': float(r1 + r2), 'loss_l': float(l1 + l2)}


def train_minibatch_kg_fused(trainer, model, data, optimizer, args, step_hook=None):
    """KGGNNDeleteNodeembTrainer.train's batch loop with the batch step on the HIP kernels: same sampler and negatives (same
    host random stream), same update order, step records (read once per epoch), validation cadence, model selection and
    checkpoints."""
    from .framework.trainer import sampler as S
    from .framework.trainer._log import wandb_log
    from .framework.trainer.base import _require_gpu, device
    from .framework.trainer.gnndelete_nodeemb import _adam_hyper, _non_df_masks
    _require_gpu()
    model = model.to(device)
    data = data.to('cpu')
    _non_df_masks(data)
    loader = S.make_sampler(data, args.batch_size, args.num_steps)
    lr, betas, eps = _adam_hyper(optimizer)
    alpha = trainer.args.alpha
    step = MinibatchKGNodeembStep(model, data, loader, trainer.args.num_edge_type, alpha,
                                  'mean' if trainer.args.loss_fct == 'mse_mean' else 'sum', lr, betas, eps,
                                  max_nodes=(loader.walk_length + 1) * max(int(loader.batch_size), 1))
    step.import_adam_state(optimizer)
    trainer._fused_minibatch_step = step
    best_metric = 0
    trainer.trainer_log['steps'] = []
    for epoch in range(args.epochs):
        model.train()
        hist = torch.zeros(max(len(loader), 1), 4, dtype=torch.float32, device=device)
        divs = []
        for i, nodes in enumerate(loader.node_sets()):
            if i >= hist.shape[0]:
                hist = torch.cat([hist, torch.zeros_like(hist)])
            divs.append(step.step(nodes, hist[i]))
            if step_hook is not None:
                step_hook(step)
        last = None
        for s4, div in zip(hist[:len(divs)].tolist(), divs):                 # the epoch's host read
            last = _kg_step_log(epoch, s4, div, alpha)
            wandb_log(last)
            trainer.trainer_log['steps'].append(last)
        if (epoch + 1) % trainer.args.valid_freq == 0 and last is not None:
            valid_loss, dt_auc, dt_aup, df_auc, df_aup, df_logit, _, valid_log = trainer.eval(model, data, 'val')
            valid_log['epoch'] = epoch
            trainer._record({'epoch': epoch, 'train_loss': last['train_loss'], 'loss_r': last['loss_r'],
                             'loss_l': last['loss_l']}, valid_log)
            if dt_auc + df_auc > best_metric:
                best_metric = dt_auc + df_auc
                print(f'Save best checkpoint at epoch {epoch:04d}. Valid loss = {valid_loss:.4f}')
                torch.save({'model_state': model.state_dict()}, os.path.join(args.checkpoint_dir, 'model_best.pt'))
            data = data.to('cpu')
    step.export_adam_state(optimizer)
    torch.save({'model_state': {k: v.to('cpu') for k, v in model.state_dict().items()}},
               os.path.join(args.checkpoint_dir, 'model_final.pt'))
