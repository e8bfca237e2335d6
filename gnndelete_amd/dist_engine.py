"""Row-partitioned Del-training step for N GPUs of one node (one process per GPU, RCCL over xGMI).

north_star: "graphs that outgrow one GPU are 1-D partitioned across the 8 GPUs with RCCL exchange of the aggregates
and of the Del-operator gradients".  The partition is by TARGET rows - contiguous equal blocks of the engine's
locality order - which turns the exchange of partial aggregates ([N, d] all-reduce) into an exchange of the layer
INPUT rows a rank's aggregation gathers from other ranks (the halo): fewer bytes, and every row keeps the
summation order it has on one GPU.

Same fused stages as the single-GPU step (engine.NodeembEngine), cut into four hipGraph
segments by the three collectives; the halo pack / unpack copies are part of the graphs:

  A  t1 = x W1^T on the rows this rank's layer-1 aggregation reads (own + halo: the input is replicated and
     recomputing a halo row costs 33 kflop, sending it 512 B)  ->  pre1 = conv1 on OWN rows  ->  Del-1 (+ ReLU sign
     bits)  ->  [layer-wise types] partial dW_D1 with the layer-1 loss formed in the fetch  ->  t2 = relu(.) W2^T
     on own rows  ->  pack the t2 rows other ranks gather
  >> all-to-all #1: t2 halo rows ([*, out] fp32, per-pair sorted row lists both sides derive from the replicated CSR)
  B  unpack  ->  p2 = conv2 aggregation on own rows  ->  Del-2 + layer-2 loss + Del-2 input gradient (one kernel)
     ->  partial dW_D2  ->  pack the dp2 rows other ranks' transposed aggregation gathers
  >> all-to-all #2: dp2 halo rows
  C  unpack  ->  dt2 = A^T dp2 on the own S1 rows  ->  dh[S1] = (dt2 W2) gated by the sign bits  ->  [both_all /
     only2_all] partial dW_D1  ->  loss partial sums  ->  one packed buffer
  >> all-reduce: [dW_D1 | dW_D2 | 4 loss sums]  (128^2 + 64^2 + 4 floats = 80 KiB)
  D  the --loss_type gradient bookkeeping + Adam on both Del weights, identically on every rank;
     loss history, iteration counter.

Overlap (GCN / GIN / GraphSAGE): the exchanges run on a communication stream while the compute stream does the work that
does not need the halo - A2 = the partial dW_D1 (layer-wise types) and the layer-2 aggregation of the INTERIOR rows (own
rows all of whose in-neighbours are own), B2 = the partial dW_D2 and the transposed aggregation of the interior S1 rows;
the BOUNDARY rows follow once the halo has arrived.  (No multi-GPU node was available to this build: the overlap is
correct by construction and covered by the gloo tests; its benefit is unmeasured.)

GCN, GIN, GraphSAGE and GAT backbones.  GAT keeps every softmax on the rank that owns the target row; its backward
needs no second forward-direction exchange: a rank computes the attention gradients of its OWN target rows (it
holds their halo h rows since the forward exchange), which yields partial message gradients for own AND halo source
rows; the halo rows' partials travel back to their owners in the reverse all-to-all and are added there in rank
order (deterministic).  The fused single-GPU configuration is required: folded DEC + NI terms, every loss row inside its Del row
list (always so for the reference's masks), MFMA widths."""
import os

import torch

from . import _lib, ops
from ._lib import check, ptr, stream_ptr
from . import collectives as _collectives
from .collectives import all_reduce_sum, exchange_rows, exchange_rows_reverse, halo_plan, row_blocks
from .engine import LOSS_TYPES, _Adam, _LayerTerms, _loss_coefficients, _loss_slots, _rows_inside
from .graph import SplitPlan, graph_for
from .nn import GATConv, GCNConv, GINConv, RGCNConv, SAGEConv


class PartitionedNodeembEngine:
    def __init__(self, model, x, edge_index, z1_ori, z2_ori, pos_edge, neg_edge, ni_mask1, ni_mask2, rank, world,
                 loss_type='both_layerwise', alpha=0.5, lr=1e-3, reduction='mean', use_graph=True, history=4096,
                 reorder=True, group=None, edge_type=None, overlap=None, loss_fct=None):
        """edge_type (R-GCN, BASELINE config 4): relation type per column of edge_index; x is then the entity id vector
        (the frozen embedding table is replicated and looked up once).
        overlap: run the halo exchanges on a communication stream UNDER the interior-row aggregation and the partial weight
        gradients (True), or every exchange as start + wait on the spot (False: the synchronous program - same kernels, same
        results bit for bit, no cross-stream ordering to get wrong).  None = the environment's GD_DIST_OVERLAP (1 / 0), else
        False: the overlapped program has only ever run with all ranks on one GPU (gloo); until it has been seen on a real
        multi-GPU RCCL group the synchronous one is the default, and bench.py switches the overlap on only after its
        child-process probe has reproduced the synchronous result with it."""
        assert loss_type in LOSS_TYPES, loss_type
        if loss_fct is not None and loss_fct not in ('mse_mean', 'mse_sum'):
            # (the bounded KLD's gradient carries exp(-KL / n), a scalar over ALL ranks' rows: an all-reduce in mid-step)
            raise NotImplementedError(f'PartitionedNodeembEngine runs the MSE losses only (loss_fct={loss_fct!r}): the folded KLD / cosine '
                                      'row losses of NodeembEngine have no row-partitioned form - the KLD scalar would need an all-reduce '
                                      'in mid-step')
        if loss_fct is not None and loss_fct != 'mse_' + reduction:       # (the argument exists for the refusal above only)
            raise ValueError(f'PartitionedNodeembEngine: loss_fct={loss_fct!r} contradicts reduction={reduction!r}')
        conv1, conv2 = model.conv1, model.conv2
        if not isinstance(conv2, (GCNConv, GINConv, SAGEConv, GATConv, RGCNConv)):
            raise NotImplementedError('PartitionedNodeembEngine supports GCN, GIN, GraphSAGE, GAT and R-GCN backbones')
        if isinstance(conv2, RGCNConv):
            assert edge_type is not None, 'R-GCN needs edge_type'
            reorder = False
            x = model.node_emb.weight.detach()[x.to(model.node_emb.weight.device)]
        dev = x.device
        if dev.type != 'cuda':
            raise _lib.GnnDeleteHipError('PartitionedNodeembEngine needs CUDA(HIP) tensors (no CPU fallback)')
        self.model, self.loss_type, self.alpha = model, loss_type, alpha
        self.rank, self.world, self.group = rank, world, group
        self.n = n = x.shape[0]
        m1, m2 = model.deletion1.mask.to(dev), model.deletion2.mask.to(dev)
        ni_mask1, ni_mask2 = ni_mask1.to(dev), ni_mask2.to(dev)
        pos_edge, neg_edge = pos_edge.to(dev), neg_edge.to(dev)
        self.perm = None
        if reorder and edge_index.shape[1] > 0 and n > 4096:
            from .reorder import locality_order
            perm, inv = locality_order(edge_index, n)      # deterministic: identical on every rank
            self.perm = perm
            x = x[perm].contiguous()
            edge_index = inv[edge_index]
            z1_ori, z2_ori = z1_ori[perm], z2_ori[perm]
            m1, m2, ni_mask1, ni_mask2 = m1[perm], m2[perm], ni_mask1[perm], ni_mask2[perm]
            pos_edge, neg_edge = inv[pos_edge], inv[neg_edge]
        self.x = x
        self.chunk, _ = row_blocks(n, world)
        self.lo = lo = min(n, rank * self.chunk)
        self.hi = hi = min(n, lo + self.chunk)
        self.wd1, self.wd2 = model.deletion1.deletion_weight, model.deletion2.deletion_weight
        self.h, self.o = self.wd1.shape[0], self.wd2.shape[0]
        self._mode = {GCNConv: 'gcn', GINConv: 'gin', SAGEConv: 'sage', GATConv: 'gat', RGCNConv: 'rgcn'}[type(conv2)]
        if self.h not in (32, 64, 128) or self.o not in (32, 64) or x.shape[1] % 32 or x.shape[1] * self.h * 4 > 65536:
            raise NotImplementedError('partitioned step: widths must suit the fused kernels (in % 32 == 0, hidden in '
                                      '{32, 64, 128}, out in {32, 64})')
        if self._mode == 'gin' and conv2.nn.out_features > conv2.nn.in_features:
            raise NotImplementedError('partitioned step: a second GIN layer that widens its input')
        # a first GIN layer that widens aggregates BEFORE its Linear (fewer gathered bytes); x is replicated, so that
        # aggregation needs no halo at all
        self._gin_agg_first = self._mode == 'gin' and conv1.nn.out_features > conv1.nn.in_features

        def local(mask):
            idx = mask.nonzero().flatten()
            return idx[(idx >= lo) & (idx < hi)].to(torch.int32)
        self.idx1, self.idx2 = local(m1), local(m2)
        self.s1, self.s2 = int(self.idx1.numel()), int(self.idx2.numel())
        self.own = torch.arange(lo, hi, dtype=torch.int32, device=dev)
        z1_ori, z2_ori = ops._f32_rows(z1_ori), ops._f32_rows(z2_ori)
        coef_r, coef_l = _loss_coefficients(loss_type, alpha)
        self.t1 = _LayerTerms(pos_edge, neg_edge, ni_mask1, z1_ori, coef_r, coef_l, reduction, (lo, hi))
        self.t2 = _LayerTerms(pos_edge, neg_edge, ni_mask2, z2_ori, coef_r, coef_l, reduction, (lo, hi))
        ok = torch.tensor([int(self.t1.folded and self.t2.folded
                               and (self.t1.n_rows == 0 or _rows_inside(self.t1, self.idx1, self.s1))
                               and (self.t2.n_rows == 0 or _rows_inside(self.t2, self.idx2, self.s2)))],
                          dtype=torch.float64, device=dev)
        # constants of the folded losses are per-rank partial sums: reduce them (and the feasibility flag) once
        k = torch.cat([torch.tensor(self.t1.k_const + self.t2.k_const, dtype=torch.float64, device=dev), ok])
        all_reduce_sum(k, world, group)
        if int(round(float(k[4]))) != world and self._mode != 'rgcn':
            raise NotImplementedError('partitioned step: a loss row lies outside its Del row list on some rank')
        if self._mode == 'rgcn' and not (self.t1.folded and self.t2.folded):
            raise NotImplementedError('partitioned R-GCN step: a row carries both DEC and NI terms')
        self.k_const = k[:4].tolist()
        f32 = dict(dtype=torch.float32, device=dev)

        def slots(terms, idx, n_sel):
            # (R-GCN: the loss rows are not members of the Del row lists - no slots, the general loss stages are used)
            if terms.n_rows == 0 or self._mode == 'rgcn':
                return (torch.full((max(n_sel, 1),), -1, dtype=torch.int32, device=dev), torch.zeros(1, **f32))
            return _loss_slots(terms, idx, n_sel, dev)
        self._slot1, self._cnt_signed1 = slots(self.t1, self.idx1, self.s1)
        self._slot2, self._cnt_signed2 = slots(self.t2, self.idx2, self.s2)
        self._tm1 = self.t1.tm if self.t1.n_rows else torch.zeros(1, self.h, **f32)
        self._tm2 = self.t2.tm if self.t2.n_rows else torch.zeros(1, self.o, **f32)
        self._coef1 = self.t1.coef if self.t1.n_rows else torch.zeros(1, **f32)
        self._coef2 = self.t2.coef if self.t2.n_rows else torch.zeros(1, **f32)

        gmode = {'gcn': 'gcn', 'gin': 'sum', 'sage': 'mean', 'gat': 'gat', 'rgcn': 'sum'}[self._mode]
        # (R-GCN: the untyped union graph is only the STRUCTURE the halo lists are derived from)
        self.graph = g = graph_for(edge_index, n, gmode)
        if self._mode == 'rgcn':
            from .graph import TypedNodeCSR
            # typed graph of this rank: in-edges of the own target rows (forward), out-edges of the own source rows with
            # the global mean weights (input gradient); tile plans and packed weights made outside any capture
            self.typed = TypedNodeCSR(edge_index, edge_type.to(dev), n, conv2.num_relations, row_range=(lo, hi))
            for c_, din, dout, tr in ((conv1, x.shape[1], self.h, 0), (conv2, self.h, self.o, 0), (conv2, self.o, self.h, 1)):
                if int(_lib.lib().gd_rgcn_tile_kl(din, dout, c_.num_blocks or 1, tr)) > 0:
                    if ops.rgcn_wave_form(din, dout, c_.num_blocks or 1, n, din) and self.typed.num_relations < 65536:
                        self.typed.wave_plan(bool(tr))
                    else:
                        self.typed.tile_plan(bool(tr))
                    ops.rgcn_packed_weight(c_.weight.detach(), c_.num_blocks or 1, din, dout, tr)
        self.plan = SplitPlan(g.rowptr, row_range=(lo, hi))                    # forward aggregations: own rows
        self.plan_t = SplitPlan(g.rowptr_t, rows=self.idx1) if self.s1 else None   # transposed: own S1 rows only

        def split_rows(rowptr, col, rows):
            """rows (int32 ids) -> (interior, boundary): interior = every gathered row is owned by this rank."""
            deg = (rowptr[1:] - rowptr[:-1]).long()
            tgt = torch.repeat_interleave(torch.arange(n, device=dev), deg)
            c = col.long()
            remote = torch.zeros(n, dtype=torch.bool, device=dev)
            remote[tgt[(c < lo) | (c >= hi)]] = True
            r = rows.long()
            return rows[~remote[r]].contiguous(), rows[remote[r]].contiguous()
        self._overlap = self._mode not in ('gat', 'rgcn')
        if self._overlap:
            i_f, b_f = split_rows(g.rowptr, g.col, self.own)
            self.plan_int, self.plan_bnd = SplitPlan(g.rowptr, rows=i_f), SplitPlan(g.rowptr, rows=b_f)
            self.n_interior = int(i_f.numel())
            if self.s1:
                i_t, b_t = split_rows(g.rowptr_t, g.col_t, self.idx1)
                self.plan_t_int, self.plan_t_bnd = SplitPlan(g.rowptr_t, rows=i_t), SplitPlan(g.rowptr_t, rows=b_t)
                self.n_interior_t = int(i_t.numel())
        self._comm_stream = torch.cuda.Stream(device=dev)
        if overlap is None:
            overlap = os.environ.get('GD_DIST_OVERLAP', '0') == '1'
        self._async = bool(overlap)
        self._gat1_bufs, self._gat2_bufs = {}, {}      # persistent work buffers of the GAT raw ops (ops._ws_buf)
        # ---- halo lists (device-side, one host transfer of the [world, world] count matrix each)
        own_mask = torch.zeros(n, dtype=torch.bool, device=dev)
        own_mask[lo:hi] = True
        s1_mask = m1.clone()
        self.halo_f = halo_plan(g.rowptr, g.col, n, rank, world, self.chunk, None)
        self.halo_b = halo_plan(g.rowptr_t, g.col_t, n, rank, world, self.chunk, s1_mask) if self._mode != 'gat' else None
        self.need1 = torch.unique(torch.cat([self.own.long(), self.halo_f.recv_rows])).to(torch.int32)
        if self._mode == 'gat':
            # transposed aggregation over own + halo SOURCE rows (partial message gradients from the own targets),
            # and the buffers of the reverse exchange that carries the halo rows' partials home
            self.plan_src = SplitPlan(g.rowptr_t, rows=self.need1)
            self.rsend = torch.zeros(max(1, self.halo_f.n_recv), self.o, **f32)
            self.rrecv = torch.zeros(max(1, self.halo_f.n_send), self.o, **f32)
            self.halo_b = self.halo_f                       # (report only: the reverse exchange moves the same rows)
        self.wf = self.h if self._mode == 'rgcn' else self.o        # R-GCN aggregates BEFORE its transform: h-wide halo rows
        self.send_f = torch.zeros(max(1, self.halo_f.n_send), self.wf, **f32)
        self.recv_f = torch.zeros(max(1, self.halo_f.n_recv), self.wf, **f32)
        self.send_b = torch.zeros(max(1, self.halo_b.n_send), self.o, **f32)
        self.recv_b = torch.zeros(max(1, self.halo_b.n_recv), self.o, **f32)

        w_o = 2 * self.o if self._mode == 'sage' else self.o
        if self._mode == 'rgcn':
            self.hbuf = torch.zeros(n, self.h, **f32)               # relu(z1 | pre1): own rows + received halo rows
            self.dxbuf = torch.zeros(n, self.h, **f32)              # conv2's input gradient on the own rows
            # The KG trainer passes the NON-Df masks as Del masks (gnndelete_nodeemb.py:749-751) while its DEC rows are the
            # Df endpoints: loss rows lie OUTSIDE the Del row lists, so this mode runs the general stages - in-place Del
            # operators on copies of the conv outputs, the folded row-target loss kernel, explicit [N, d] gradients
            self.dz1 = torch.zeros(n, self.h, **f32)
            self.z2 = torch.zeros(n, self.o, **f32)
            self.l_sums = torch.zeros(4, **f32)
        self.t1buf = torch.zeros(n, self.h, **f32)                  # x W1^T on the rows need1 (others never read)
        self.t1rbuf = torch.zeros(n, self.h, **f32) if self._mode == 'sage' else None
        self.aggbuf = torch.zeros(n, x.shape[1], **f32) if self._gin_agg_first else None
        self.pre1 = torch.zeros(n, self.h, **f32)
        self.z1 = torch.zeros(n, self.h, **f32)
        self.t2buf = torch.zeros(n, w_o, **f32)                     # (t2_l | t2_r) for GraphSAGE
        self.p2 = torch.zeros(n, self.o, **f32)
        if self._mode == 'sage':
            self.dcat = torch.zeros(n, 2 * self.o, **f32)           # [ dt2 | dp2 ]
            self.dz2 = self.dcat[:, self.o:]
            self._w2cat = torch.cat([conv2.lin_l.weight.detach(), conv2.lin_r.weight.detach()], 0).contiguous()
        else:
            self.dz2 = torch.zeros(n, self.o, **f32)
            self.dt2 = torch.zeros(n, self.o, **f32)
        self.dz2c = torch.zeros(max(1, self.s2), self.o, **f32)
        self.dh = torch.zeros(n, self.h, **f32)
        self.z1_pos = torch.zeros(max(1, self.s1), (self.h + 31) // 32, dtype=torch.int32, device=dev)
        self._sel1 = m1.to(torch.uint8).contiguous()
        hh, oo = self.h * self.h, self.o * self.o
        self.pack = torch.zeros(hh + oo + 4, **f32)                 # [dW_D1 | dW_D2 | r1 l1 r2 l2]
        self.p_g1 = self.pack[:hh].view(self.h, self.h)
        self.p_g2 = self.pack[hh:hh + oo].view(self.o, self.o)
        self.p_sums = self.pack[hh + oo:]
        self.g1 = torch.zeros_like(self.wd1)                        # the .grad of W_D1 / W_D2 (replicated)
        self.g2 = torch.zeros_like(self.wd2)
        self.ws1 = torch.empty(max(1, _lib.lib().gd_rows_gemm_wgrad_workspace(self.s1, self.h, self.h)), **f32)
        self.ws2 = torch.empty(max(1, _lib.lib().gd_rows_gemm_wgrad_workspace(self.s2, self.o, self.o)), **f32)
        self._lp1_blocks = _lib.lib().gd_rows_gemm_wgrad_blocks(self.s1)
        self._lp1 = torch.zeros(2 * max(1, self._lp1_blocks), **f32)
        self._lp2_blocks = _lib.lib().gd_del_loss_bwd_blocks(self.s2)
        self._lp2 = torch.zeros(2 * max(1, self._lp2_blocks), **f32)
        self.iter_ctr = torch.zeros(1, dtype=torch.int32, device=dev)
        self.adam1, self.adam2 = _Adam(self.wd1, lr, iter_ctr=self.iter_ctr), _Adam(self.wd2, lr, iter_ctr=self.iter_ctr)
        self.hist = torch.zeros(history, 4, **f32)
        self.hist_pos = torch.zeros(1, dtype=torch.int32, device=dev)
        self.steps_done = 0
        self._use_graph = use_graph
        self._graphs = None
        self._const_refs = {}
        self.uses_l1 = loss_type in ('both_all', 'both_layerwise', 'only1')
        self.needs_l2_to_w1 = loss_type in ('both_all', 'both_layerwise', 'only2_all')

    # ------------------------------------------------------------------ pieces
    def _spmm(self, transposed, val, x, y, bias, self_coef, x_self=None, plan=None):
        g = self.graph
        if transposed:
            ops._spmm_raw(g.rowptr_t, g.col_t, val, x, bias, self_coef, self.n, plan or self.plan_t, out=y, x_self=x_self)
        else:
            ops._spmm_raw(g.rowptr, g.col, val, x, bias, self_coef, self.n, plan or self.plan, out=y, x_self=x_self)

    def _wgrad1_partial(self, with_loss, g_add):
        """p_g1 = pre1[S1]^T (layer-1 loss gradient and / or g_add) over the OWN S1 rows; the layer-1 loss sums
        come out as per-block partials (no optimizer update here: the gradient is still a partial sum)."""
        if self.s1 == 0:
            self.p_g1.zero_()
            self._lp1.zero_()
            return
        if with_loss:
            check(_lib.lib().gd_rows_gemm_wgrad_loss_f32(
                ptr(self.pre1), self.pre1.stride(0), ptr(self.idx1), ptr(self.z1), self.z1.stride(0), ptr(self.idx1),
                ptr(self._slot1), ptr(self._tm1), ptr(self._coef1), ptr(self._cnt_signed1), ptr(g_add), self.s1, self.h,
                self.h, ptr(self.p_g1), 0, ptr(self.ws1), ptr(self._lp1), None, None, None, None, 0.0, 0.0, 0.0, 0.0,
                stream_ptr(self.x.device)), 'gd_rows_gemm_wgrad_loss_f32')
        else:
            check(_lib.lib().gd_rows_gemm_wgrad_f32(ptr(self.pre1), self.pre1.stride(0), ptr(self.idx1), ptr(g_add),
                                                    g_add.stride(0), ptr(self.idx1), None, None, self.s1, self.h, self.h,
                                                    ptr(self.p_g1), 0, ptr(self.ws1), stream_ptr(self.x.device)),
                  'gd_rows_gemm_wgrad_f32')

    def _layer1_loss_only(self):
        """Loss sums of layer 1 when its gradient feeds no optimizer step (only2_*): the weight-gradient kernel's
        fetch is still the cheapest place to form them, its product is discarded."""
        self._wgrad1_partial(True, None)
        self.p_g1.zero_()

    # ------------------------------------------------------------------ R-GCN segments (own target rows, typed halo)
    def _rgcn_conv_own(self, conv, inp, out, trans, rows):
        """out[rows] = inp[rows] @ root (+ bias) + the typed conv of this rank's restricted graph (forward: in-edges of
        the own rows; trans: the transposed graph of the own source rows with W_r^T)."""
        nb = conv.num_blocks or 1
        ops.rows_gemm(inp, rows, conv.root.detach(), trans_w=bool(trans), bias=None if trans else conv.bias.detach(), out=out)
        ops.rgcn_typed_accumulate(self.typed, inp, conv.weight.detach(), nb, int(trans), out)

    def _seg_a_rgcn(self):
        c1 = self.model.conv1
        lo, hi = self.lo, self.hi
        self._rgcn_conv_own(c1, self.x, self.pre1, 0, self.own)          # x is replicated: layer 1 needs no halo
        self.z1[lo:hi] = self.pre1[lo:hi]                                 # rows outside S1 pass through Del-1 unchanged
        if self.s1:
            ops.rows_gemm(self.pre1, self.idx1, self.wd1, out=self.z1, sign_bits=self.z1_pos)
        self.l_sums.zero_()
        if self.t1.n_rows:
            self.t1.launch(self.z1, self.dz1, self.l_sums[0:2])          # layer-1 loss sums + dz1 on the loss rows
        if self.loss_type != 'only1':
            torch.clamp(self.z1[lo:hi], min=0, out=self.hbuf[lo:hi])
            if self.halo_f.n_send:
                torch.index_select(self.hbuf, 0, self.halo_f.send_rows, out=self.send_f)

    def _wgrad1_rgcn(self, g_add):
        """p_g1 = pre1[S1]^T (dz1 [+ g_add])[S1] over the own S1 rows (dz1 = 0 on rows without loss terms)."""
        if self.s1 == 0:
            self.p_g1.zero_()
            return
        check(_lib.lib().gd_rows_gemm_wgrad_f32(ptr(self.pre1), self.pre1.stride(0), ptr(self.idx1), ptr(self.dz1),
                                                self.dz1.stride(0), ptr(self.idx1), None, ptr(g_add), self.s1, self.h, self.h,
                                                ptr(self.p_g1), 0, ptr(self.ws1), stream_ptr(self.x.device)), 'gd_rows_gemm_wgrad_f32')

    def _layer1_partials_rgcn(self):
        lt = self.loss_type
        if lt == 'both_layerwise':
            self._wgrad1_rgcn(self.dh)                    # dh = the PREVIOUS iteration's layer-2 gradient
        elif lt == 'only1':
            self._wgrad1_rgcn(None)
        else:
            self.p_g1.zero_()

    def _seg_b_rgcn(self):
        lt = self.loss_type
        lo, hi = self.lo, self.hi
        if lt == 'only1':
            self.p_g2.zero_()
            return
        if self.halo_f.n_recv:
            self.hbuf.index_copy_(0, self.halo_f.recv_rows, self.recv_f)
        self._rgcn_conv_own(self.model.conv2, self.hbuf, self.p2, 0, self.own)
        self.z2[lo:hi] = self.p2[lo:hi]
        if self.s2:
            ops.rows_gemm(self.p2, self.idx2, self.wd2, out=self.z2)
        self.dz2[lo:hi].zero_()
        if self.t2.n_rows:
            self.t2.launch(self.z2, self.dz2, self.l_sums[2:4])           # dz2 on the loss rows
        if self.s2:
            check(_lib.lib().gd_rows_gemm_wgrad_f32(ptr(self.p2), self.p2.stride(0), ptr(self.idx2), ptr(self.dz2),
                                                    self.dz2.stride(0), ptr(self.idx2), None, None, self.s2, self.o, self.o,
                                                    ptr(self.p_g2), 0, ptr(self.ws2), stream_ptr(self.x.device)),
                  'gd_rows_gemm_wgrad_f32')
            if self.needs_l2_to_w1:
                ops.rows_gemm(self.dz2, self.idx2, self.wd2, trans_w=True, out=self.dz2)     # dz2 -> dp2 on the Del'd rows
        else:
            self.p_g2.zero_()
        if self.needs_l2_to_w1 and self.halo_b.n_send:
            torch.index_select(self.dz2, 0, self.halo_b.send_rows, out=self.send_b)

    def _seg_c_rgcn(self):
        lt = self.loss_type
        if self.needs_l2_to_w1:
            if self.halo_b.n_recv:
                self.dz2.index_copy_(0, self.halo_b.recv_rows, self.recv_b)
            if self.s1:
                self._rgcn_conv_own(self.model.conv2, self.dz2, self.dxbuf, 1, self.own)
                ops.gate_rows(self.dxbuf, self.idx1, self.z1_pos, self.dh)       # ReLU backward from the packed sign bits
            if lt == 'both_all':
                self._wgrad1_rgcn(self.dh)
            elif lt == 'only2_all':
                if self.s1:
                    check(_lib.lib().gd_rows_gemm_wgrad_f32(ptr(self.pre1), self.pre1.stride(0), ptr(self.idx1), ptr(self.dh),
                                                            self.dh.stride(0), ptr(self.idx1), None, None, self.s1, self.h, self.h,
                                                            ptr(self.p_g1), 0, ptr(self.ws1), stream_ptr(self.x.device)),
                          'gd_rows_gemm_wgrad_f32')
                else:
                    self.p_g1.zero_()
        self.p_sums.copy_(self.l_sums)

    # ------------------------------------------------------------------ the four segments
    def _seg_a(self):
        c1, c2 = self.model.conv1, self.model.conv2
        g, lt = self.graph, self.loss_type
        if self._mode == 'gcn':
            ops.rows_gemm(self.x, self.need1, c1.lin.weight, trans_w=True, const_w=True, out=self.t1buf)
            self._spmm(False, g.val, self.t1buf, self.pre1, c1.bias, 0.0)
            w2 = c2.lin.weight
        elif self._mode == 'gin':
            if self._gin_agg_first:
                self._spmm(False, None, self.x, self.aggbuf, None, 1.0 + c1.eps)
                ops.rows_gemm(self.aggbuf, self.own, c1.nn.weight, trans_w=True, const_w=True, bias=c1.nn.bias, out=self.pre1)
            else:
                ops.rows_gemm(self.x, self.need1, c1.nn.weight, trans_w=True, const_w=True, out=self.t1buf)
                self._spmm(False, None, self.t1buf, self.pre1, c1.nn.bias, 1.0 + c1.eps)
            w2 = c2.nn.weight
        elif self._mode == 'gat':
            ops.rows_gemm(self.x, self.need1, c1.lin_src.weight, trans_w=True, const_w=True, out=self.t1buf)
            a_s, a_d = ops.row_dots(self.t1buf, c1.att_src, c1.att_dst, bufs=self._gat1_bufs)
            ops.gat_forward_raw(g, self.t1buf, a_s, a_d, c1.bias, c1.negative_slope, out=self.pre1, plan=self.plan,
                                bufs=self._gat1_bufs)
            w2 = c2.lin_src.weight
        else:
            ops.rows_gemm(self.x, self.need1, c1.lin_l.weight, trans_w=True, const_w=True, out=self.t1buf)
            ops.rows_gemm(self.x, self.own, c1.lin_r.weight, trans_w=True, const_w=True, out=self.t1rbuf)
            self._spmm(False, g.val, self.t1buf, self.pre1, c1.lin_l.bias, 1.0, x_self=self.t1rbuf)
            w2 = self._w2cat
        if self.s1:
            ops.rows_gemm(self.pre1, self.idx1, self.wd1, out=self.z1, sign_bits=self.z1_pos)
        if not self._overlap:
            self._layer1_partials()
        if lt != 'only1':
            ops.rows_gemm_select(self.pre1, self.z1, self._sel1, w2, trans_w=True, const_w=True, relu_in=True,
                                 out=self.t2buf, idx=self.own)
            if self.halo_f.n_send:
                torch.index_select(self.t2buf[:, :self.o], 0, self.halo_f.send_rows, out=self.send_f)

    def _layer1_partials(self):
        """Partial dW_D1 / layer-1 loss sums of the layer-wise loss types (they only need Del-1's output)."""
        lt = self.loss_type
        if lt == 'both_layerwise':
            self._wgrad1_partial(True, self.dh)          # dh = the PREVIOUS iteration's layer-2 gradient
        elif lt == 'only1':
            self._wgrad1_partial(True, None)
        elif lt == 'only2_layerwise':
            self._layer1_loss_only()                     # its log line adds the layer-1 sums (loss_r = r1 + r2, loss_l = l1 + l2)
        elif lt == 'only2_all':
            self.p_g1.zero_()                            # neither the update nor the log line of only2_all reads layer 1
            self._lp1.zero_()

    def _agg2(self, plan):
        """Layer-2 aggregation of the rows of `plan` (own rows, or their interior / boundary part)."""
        c2, g = self.model.conv2, self.graph
        if self._mode == 'gcn':
            self._spmm(False, g.val, self.t2buf, self.p2, c2.bias, 0.0, plan=plan)
        elif self._mode == 'gin':
            self._spmm(False, None, self.t2buf, self.p2, c2.nn.bias, 1.0 + c2.eps, plan=plan)
        else:
            self._spmm(False, g.val, self.t2buf[:, :self.o], self.p2, c2.lin_l.bias, 1.0, x_self=self.t2buf[:, self.o:], plan=plan)

    def _agg2_t(self, plan):
        """Transposed layer-2 aggregation (conv2's input gradient before the Linear) of the S1 rows of `plan`."""
        c2, g = self.model.conv2, self.graph
        if self._mode == 'sage':
            self._spmm(True, g.val_t, self.dz2, self.dcat[:, :self.o], None, 0.0, plan=plan)
        elif self._mode == 'gcn':
            self._spmm(True, g.val_t, self.dz2, self.dt2, None, 0.0, plan=plan)
        else:
            self._spmm(True, None, self.dz2, self.dt2, None, 1.0 + c2.eps, plan=plan)

    def _wgrad2_partial(self):
        if self.s2:
            check(_lib.lib().gd_rows_gemm_wgrad_f32(ptr(self.p2), self.p2.stride(0), ptr(self.idx2), ptr(self.dz2c),
                                                    self.dz2c.stride(0), None, None, None, self.s2, self.o, self.o,
                                                    ptr(self.p_g2), 0, ptr(self.ws2), stream_ptr(self.x.device)),
                  'gd_rows_gemm_wgrad_f32')
        else:
            self.p_g2.zero_()

    def _seg_a2(self):
        """While exchange #1 is in flight: the layer-1 partials and the layer-2 aggregation of the interior rows."""
        self._layer1_partials()
        if self.loss_type != 'only1':
            self._agg2(self.plan_int)

    def _seg_b(self):
        c2 = self.model.conv2
        g, lt = self.graph, self.loss_type
        if lt == 'only1':
            self._lp2.zero_()
            self.p_g2.zero_()
            return
        if self.halo_f.n_recv:
            self.t2buf[:, :self.o].index_copy_(0, self.halo_f.recv_rows, self.recv_f)
        if self._mode == 'gat':
            # (logits, row statistics and - below - the per-edge gradient buffers are written in one captured segment and read
            #  in later ones: they live in buffers this engine owns, self._gat2_bufs, not in capture-time allocations)
            a_s, a_d = ops.row_dots(self.t2buf, c2.att_src, c2.att_dst, bufs=self._gat2_bufs)   # own + halo rows hold h2
            _, rowmax, rowsum = ops.gat_forward_raw(g, self.t2buf, a_s, a_d, c2.bias, c2.negative_slope, out=self.p2,
                                                    plan=self.plan, bufs=self._gat2_bufs)
            self._gat2 = (a_s, a_d, rowmax, rowsum)
        else:
            self._agg2(self.plan_bnd if self._overlap else self.plan)
        if self.s2:
            check(_lib.lib().gd_del_loss_bwd_f32(
                ptr(self.p2), self.p2.stride(0), ptr(self.idx2), self.s2, ptr(self.wd2), self.o, ptr(self._slot2),
                ptr(self._tm2), ptr(self._coef2), ptr(self._cnt_signed2), ptr(self.dz2c), self.dz2c.stride(0),
                ptr(self.dz2), self.dz2.stride(0), ptr(self._lp2), stream_ptr(self.x.device)), 'gd_del_loss_bwd_f32')
        else:
            self._lp2.zero_()
        if not self._overlap:
            self._wgrad2_partial()
        if self.needs_l2_to_w1 and self._mode != 'gat' and self.halo_b.n_send:
            torch.index_select(self.dz2, 0, self.halo_b.send_rows, out=self.send_b)

    def _seg_b2(self):
        """While exchange #2 is in flight: the partial dW_D2 and the transposed aggregation of the interior S1 rows."""
        if self.loss_type == 'only1':
            return
        self._wgrad2_partial()
        if self.needs_l2_to_w1 and self.s1:
            self._agg2_t(self.plan_t_int)

    def _seg_c_gat_edges(self):
        """GAT only: attention gradients of the OWN target rows -> partial message gradients dt2 for own and halo
        source rows (+ the rank-1 logit terms), halo rows packed for the reverse exchange."""
        if not self.needs_l2_to_w1:
            return
        c2 = self.model.conv2
        a_s, a_d, rowmax, rowsum = self._gat2
        dt2, da_s, da_d = ops.gat_backward_raw(self.graph, self.t2buf, a_s, a_d, rowmax, rowsum, self.dz2, c2.negative_slope,
                                               plan=self.plan, plan_t=self.plan_src, bufs=self._gat2_bufs)
        rows = self.need1.long()
        dt2[rows] += da_s[rows, None] * c2.att_src.detach().view(1, -1)
        dt2[self.lo:self.hi] += da_d[self.lo:self.hi, None] * c2.att_dst.detach().view(1, -1)
        self.dt2 = dt2
        if self.halo_f.n_recv:
            torch.index_select(dt2, 0, self.halo_f.recv_rows, out=self.rsend)

    def _seg_c(self):
        c2 = self.model.conv2
        g, lt = self.graph, self.loss_type
        if self.needs_l2_to_w1 and self._mode == 'gat':
            # partial gradients of the rows this rank owns arrive grouped by sender: added in rank order
            off = 0
            for q, cnt in enumerate(self.halo_f.in_splits):
                if cnt:
                    self.dt2.index_add_(0, self.halo_f.send_rows[off:off + cnt], self.rrecv[off:off + cnt])
                off += cnt
            if self.s1:
                ops.rows_gemm(self.dt2, self.idx1, c2.lin_src.weight, trans_w=False, out=self.dh, gate_bits=self.z1_pos)
            if lt == 'both_all':
                self._wgrad1_partial(True, self.dh)
            elif lt == 'only2_all':
                lp1 = self._lp1.clone()
                self._wgrad1_partial(False, self.dh) if self.s1 else self.p_g1.zero_()
                self._lp1.copy_(lp1)
        elif self.needs_l2_to_w1:
            if self.halo_b.n_recv:
                self.dz2.index_copy_(0, self.halo_b.recv_rows, self.recv_b)
            if self.s1:
                self._agg2_t(self.plan_t_bnd if self._overlap else self.plan_t)
                if self._mode == 'sage':
                    dt2, w2 = self.dcat, self._w2cat
                elif self._mode == 'gcn':
                    dt2, w2 = self.dt2, c2.lin.weight
                else:
                    dt2, w2 = self.dt2, c2.nn.weight
                ops.rows_gemm(dt2, self.idx1, w2, trans_w=False, out=self.dh, gate_bits=self.z1_pos)
            if lt == 'both_all':
                self._wgrad1_partial(True, self.dh)
            elif lt == 'only2_all':
                lp1 = self._lp1.clone()
                self._wgrad1_partial(False, self.dh) if self.s1 else self.p_g1.zero_()
                self._lp1.copy_(lp1)
        # loss partial sums of this rank -> the tail of the packed buffer
        self.p_sums[0:2] = self._lp1.view(-1, 2)[:max(self._lp1_blocks, 1)].sum(0)
        self.p_sums[2:4] = self._lp2.view(-1, 2)[:max(self._lp2_blocks, 1)].sum(0)

    def _seg_d(self):
        lt = self.loss_type
        if lt == 'both_all':                        # upstream never zeroes these gradients
            self.g1.add_(self.p_g1)
            self.g2.add_(self.p_g2)
        else:
            self.g1.copy_(self.p_g1)
            self.g2.copy_(self.p_g2)
        if lt in ('both_all', 'both_layerwise', 'only2_all', 'only1'):
            self.adam1.apply(self.g1)
        if lt != 'only1':
            self.adam2.apply(self.g2)
        check(_lib.lib().gd_loss_finalize_f32(None, 0, None, 0, ptr(self.p_sums), ptr(self.hist), self.hist.shape[0],
                                              ptr(self.hist_pos), ptr(self.iter_ctr), stream_ptr(self.x.device)),
              'gd_loss_finalize_f32')

    def _program(self):
        """The step as a list of compute segments (callables, one hipGraph each) and communication ops ('x', what, mode):
        mode 'async' starts the exchange on the communication stream and lets the compute stream go on; 'wait' makes the
        compute stream wait for it; 'sync' = both at once."""
        if self._mode == 'gat':
            return [self._seg_a, ('x', 'halo_f', 'sync'), self._seg_b, self._seg_c_gat_edges, ('x', 'halo_r', 'sync'),
                    self._seg_c, ('x', 'reduce', 'sync'), self._seg_d]
        if self._mode == 'rgcn':          # the partial weight gradients run under the exchanges
            return [self._seg_a_rgcn, ('x', 'halo_f', 'async'), self._layer1_partials_rgcn, ('x', None, 'wait'), self._seg_b_rgcn,
                    ('x', 'halo_b', 'sync'), self._seg_c_rgcn, ('x', 'reduce', 'sync'), self._seg_d]
        return [self._seg_a, ('x', 'halo_f', 'async'), self._seg_a2, ('x', None, 'wait'), self._seg_b,
                ('x', 'halo_b', 'async'), self._seg_b2, ('x', None, 'wait'), self._seg_c, ('x', 'reduce', 'sync'), self._seg_d]

    def _comm(self, what, mode):
        if self.world == 1 and not _collectives._FORCE:
            return
        if not self._async:                # synchronous program: an 'async' op completes on the spot, its 'wait' is empty
            if what is None:
                return
            mode = 'sync'
        cur = torch.cuda.current_stream()
        if what is not None:
            self._comm_stream.wait_stream(cur)                     # the packed rows are complete
            with torch.cuda.stream(self._comm_stream):
                if what == 'halo_f' and self.loss_type != 'only1':
                    exchange_rows(self.send_f, self.recv_f, self.halo_f, self.world, self.group)
                elif what == 'halo_b' and self.needs_l2_to_w1:
                    exchange_rows(self.send_b, self.recv_b, self.halo_b, self.world, self.group)
                elif what == 'halo_r' and self.needs_l2_to_w1:
                    exchange_rows_reverse(self.rsend, self.rrecv, self.halo_f, self.world, self.group)
                elif what == 'reduce':
                    all_reduce_sum(self.pack, self.world, self.group)
        if mode in ('wait', 'sync'):
            cur.wait_stream(self._comm_stream)

    # ------------------------------------------------------------------ public
    def _mutable_state(self):
        return [self.wd1.data, self.wd2.data, self.g1, self.g2, self.adam1.m, self.adam1.v, self.adam2.m, self.adam2.v,
                self.iter_ctr, self.hist, self.hist_pos, self.dh]

    def _run_eager(self):
        with torch.no_grad(), ops.keep_constants(self._const_refs):
            for op in self._program():
                if isinstance(op, tuple):
                    self._comm(op[1], op[2])
                else:
                    op()

    def _capture(self):
        saved = [t.clone() for t in self._mutable_state()]
        applied = (self.adam1.applied, self.adam2.applied)
        self._run_eager()                                  # warm-up incl. the collectives (all ranks)
        torch.cuda.synchronize()
        prog = []
        # ONE memory pool for all segments: tensors a segment allocates while it is captured (GAT's row statistics and
        # logits, the per-edge gradient buffer) are read by LATER segments' graphs - with a pool per graph they would
        # only stay valid through the Python references
        pool = torch.cuda.graph_pool_handle()
        with torch.no_grad(), ops.keep_constants(self._const_refs):
            for op in self._program():
                if isinstance(op, tuple):
                    prog.append(op)
                    continue
                g = torch.cuda.CUDAGraph()
                # thread_local: the RCCL watchdog thread must not invalidate the capture
                with torch.cuda.graph(g, pool=pool, capture_error_mode='thread_local'):
                    op()
                prog.append(g)
        for t, s in zip(self._mutable_state(), saved):
            t.copy_(s)
        self.adam1.applied, self.adam2.applied = applied
        self._graphs = prog

    def step(self):
        if not self._use_graph:
            self._run_eager()
        else:
            if self._graphs is None:
                self._capture()
            for op in self._graphs:
                if isinstance(op, tuple):
                    self._comm(op[1], op[2])
                else:
                    op.replay()
        self.steps_done += 1

    def halo_report(self):
        """Bytes this rank receives per step in the two row exchanges, and what the dense all-gather would move."""
        row = 4 * self.o
        rowf = 4 * getattr(self, 'wf', self.o)
        rep = {'rank': self.rank, 'world': self.world, 'own_rows': self.hi - self.lo,
               'recv_rows_forward': self.halo_f.n_recv, 'recv_rows_backward': self.halo_b.n_recv,
               'recv_bytes_per_step': rowf * self.halo_f.n_recv + row * self.halo_b.n_recv,
               'send_bytes_per_step': rowf * self.halo_f.n_send + row * self.halo_b.n_send,
               'allgather_bytes_per_step': (rowf + row) * (self.n - (self.hi - self.lo)),
               'layer1_rows_recomputed': int(self.need1.numel()) - (self.hi - self.lo)}
        if self._overlap:
            rep['interior_rows_forward'] = self.n_interior
            rep['interior_rows_backward'] = getattr(self, 'n_interior_t', 0)
            rep['overlap'] = ('exchange on a communication stream under the partial weight gradients + interior-row aggregation'
                              if self._async else 'off (synchronous exchanges; GD_DIST_OVERLAP=1 / overlap=True turns it on)')
        return rep

    def loss_history(self):
        k = min(self.steps_done, self.hist.shape[0])
        s = self.hist[:k].double().cpu()
        kc = self.k_const
        nan = float('nan')
        r1 = (s[:, 0] + kc[0]) / self.t1.n_r if self.t1.count_r else s[:, 0] * nan
        l1 = (s[:, 1] + kc[1]) / self.t1.n_l if self.t1.count_l else s[:, 1] * nan
        r2 = (s[:, 2] + kc[2]) / self.t2.n_r if self.t2.count_r else s[:, 2] * nan
        l2 = (s[:, 3] + kc[3]) / self.t2.n_l if self.t2.count_l else s[:, 3] * nan
        a, lt = self.alpha, self.loss_type
        if lt in ('both_all', 'both_layerwise'):
            loss_r, loss_l = r1 + r2, l1 + l2
            loss = a * loss_r + (1 - a) * loss_l
        elif lt == 'only2_layerwise':
            loss_r, loss_l = r1 + r2, l1 + l2
            loss = a * r2 + (1 - a) * l2
        elif lt == 'only2_all':
            loss_r, loss_l = r2, l2
            loss = l2 + a * r2
        else:
            loss_r, loss_l = r1, l1
            loss = l1 + a * r1
        return torch.stack([loss, loss_r, loss_l], 1)
