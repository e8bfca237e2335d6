"""Link-prediction backbone training (train_gnn.py, delete_gnn.py --unlearning_model retrain; --fused_backbone) on a fused HIP step.

Trainer.train_fullbatch and RetrainTrainer.train_fullbatch (framework/trainer/base.py, retrain.py) run an autograd loop over
ops.dense / ops.spmm / ops.edge_dot: a torch.unique inside negative_sampling, a torch.sort + searchsorted in the decoder's
backward, F.binary_cross_entropy_with_logits and its backward, dy.sum(0) for the biases, torch's Adam, a host read of the loss.
BackboneEngine is the same step with an explicit forward, a hand-derived backward and the library's Adam - EdgeprobEngine's
shape for a model whose every parameter trains: the CSR and its transpose once, the padded / transposed copies of x once, and
the step captured in a hipGraph.

  GCN   t1 = x W1^T;  p1 = A t1 + b1;  t2 = relu(p1) W2^T;  z = A t2 + b2
        loss, w <- gd_edge_bce_f32 (w already in incidence order);   g = dL/dz <- gd_edge_dot_bwd_f32
        db2 = colsum(g);  q2 = A^T g;  dW2 = q2^T relu(p1);  dp1 = (q2 W2) * [p1 > 0], db1 = colsum(dp1) (one pass);
        q1 = A^T dp1;  dW1 = q1^T x
  GAT   per layer h = x W^T, the two row dots, ops.gat_forward_raw;  backward: ops.gat_backward_raw -> (dh, da_src, da_dst),
        d att = colsum(h, row_w = da), ops.rank1_add2_ folds the logit gradients into dh, the same weight gradients
  one gd_adam_f32 per parameter (four / eight tensors);  loss -> a device history ring

The negatives change every epoch: step(neg) copies them into the fixed [2, n_neg] half of the decoded-edge buffer and
rebuilds the incidence list on the device (gd_edge_incidence); everything after that is one graph replay, bit-identical to the
eager step.  Message-passing edges and decoded (positive) edges are separate arguments.

NodeClassifierEngine is the same step for NodeClassificationTrainer.train (train_node.py; framework/trainer/base.py:694-752
upstream): the forward, the backward and Adam are BackboneEngine's, the loss stage is gd_row_nll_f32 over the training rows,
which writes g = dL/dz directly - no decoded edges, no incidence list, so step() takes no argument and is one graph replay.
Layer 2's output width is the class count C; where padded_class_width(C) != C the engine trains zero-padded shadows of layer
2's parameters (the padding stays exactly zero, see _padded_conv2) and refreshes the model's own at the end of every iteration."""
import torch

from . import _lib, ops
from ._lib import check, ptr, stream_ptr
from .capture import capture_iterations
from .negatives import DeviceNegatives


def padded_class_width(C):
    """The layer-2 width the node-classification step runs at for C classes: C itself when it is a multiple of 32, the next
    multiple of 32 below 128 (the widths the matrix-core row kernels take), the next multiple of 4 above that."""
    C = int(C)
    if C % 32 == 0:
        return C
    return (C + 31) // 32 * 32 if C < 128 else (C + 3) // 4 * 4


def fused_backbone_unsupported(model, args, optimizer, task='linkpred'):
    """None when the fused backbone step applies, else the reason it does not (one line).  task: 'linkpred' (Trainer /
    RetrainTrainer) or 'nodecls' (NodeClassificationTrainer: the output width is a class count, padded by the engine)."""
    if task not in ('linkpred', 'nodecls'):
        raise ValueError(f'fused_backbone_unsupported: task {task!r} (linkpred or nodecls)')
    from .framework.trainer.sampler import data_parallel_world
    from .nn import GATConv, GCNConv
    conv1, conv2 = getattr(model, 'conv1', None), getattr(model, 'conv2', None)
    if (not (isinstance(conv1, (GCNConv, GATConv)) and type(conv1) is type(conv2)) or hasattr(model, 'deletion1')
            or hasattr(model, 'node_emb')):
        return f'no fused backbone step for the {type(model).__name__} backbone (GCN and GAT only)'
    if getattr(args, 'minibatch', False):
        return '--minibatch trains on GraphSAINT batches'
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
    if task == 'nodecls':
        if out > 256:
            return f'{out} classes (the fused node-classification step takes up to 256)'
        if hid % 4 or hid > 1024:
            return f'hidden width {hid} (a multiple of 4 up to 1024)'
    elif hid % 4 or out % 4 or max(hid, out) > 1024:
        return f'widths {hid} / {out} (multiples of 4 up to 1024)'
    if conv1.in_channels > 1024 and not ops.mfma_out_width(hid):
        return f'no kernel for a {conv1.in_channels} -> {hid} first product'
    return None


def edge_bce(z, pos, neg, coef=1.0, incidence=None):
    """gd_edge_bce_f32 on device tensors: BCE-with-logits over the decoded edges [pos | neg] (int64 [2, *], either may be None)
    -> (loss [1], w [M], w_inc [2M] or None); incidence = (inc_ptr, src_edge) of gd_edge_incidence over the M edges."""
    L = _lib.lib()
    n_pos = 0 if pos is None else int(pos.shape[1])
    n_neg = 0 if neg is None else int(neg.shape[1])
    m_all, d, dev = n_pos + n_neg, int(z.shape[1]), z.device
    w = torch.empty(max(m_all, 1), dtype=torch.float32, device=dev)
    loss = torch.empty(1, dtype=torch.float32, device=dev)
    ws = torch.empty(max(1, L.gd_edge_bce_workspace(m_all, d)), dtype=torch.float32, device=dev)
    inc_ptr, src_edge = incidence if incidence is not None else (None, None)
    w_inc = torch.empty(max(2 * m_all, 1), dtype=torch.float32, device=dev) if incidence is not None else None
    check(L.gd_edge_bce_f32(ptr(z), z.stride(0), z.shape[0], d, ptr(pos), pos.stride(0) if n_pos else 0, n_pos, ptr(neg),
                            neg.stride(0) if n_neg else 0, n_neg, float(coef), ptr(w), ptr(loss), ptr(src_edge), ptr(inc_ptr),
                            ptr(w_inc), ptr(ws), stream_ptr(dev)), 'gd_edge_bce_f32')
    return loss, w[:m_all], (None if w_inc is None else w_inc[:2 * m_all])


def row_nll(z, rows, y, d_valid, coef=1.0):
    """gd_row_nll_f32 on device tensors: F.nll_loss(F.log_softmax(z[:, :d_valid], 1)[rows], y[rows]) over the listed rows (unique
    node ids; y int64, indexed by node id) -> (loss [1], dz: zeros of z's shape with the listed rows' gradients, times coef)."""
    L = _lib.lib()
    rows = rows.to(device=z.device, dtype=torch.int32).contiguous()
    y = y.to(device=z.device, dtype=torch.int64).contiguous()
    n, d = int(z.shape[0]), int(z.shape[1])
    dz = torch.zeros_like(z)
    loss = torch.empty(1, dtype=torch.float32, device=z.device)
    ws = torch.empty(max(1, L.gd_row_nll_workspace(rows.numel(), d)), dtype=torch.float32, device=z.device)
    check(L.gd_row_nll_f32(ptr(z), z.stride(0), n, d, int(d_valid), ptr(rows), rows.numel(), ptr(y), float(coef), ptr(dz),
                           dz.stride(0), ptr(loss), ptr(ws), stream_ptr(z.device)), 'gd_row_nll_f32')
    return loss, dz


def _padded_conv2(c2, o_pad):
    """conv2 widened to o_pad output columns by ZEROS (weight rows, bias, attention vectors): the module the step trains in
    place of a layer whose width is a class count.  The padding stays exactly zero: g = dL/dz is zero behind the class count
    (gd_row_nll_f32 writes zeros there), so A^T g, dW2, the bias and attention-vector gradients are zero there; t2's padding
    columns are zero (zero weight rows) and add exact zeros to GAT's row dots; Adam on an all-zero gradient history moves
    nothing.  The top-left blocks follow the unpadded trajectory: the same products in the same order plus exact zeros."""
    import torch.nn as nn
    from .nn import GATConv, GCNConv

    def padded(v, dim):
        shape = list(v.shape)
        shape[dim] = o_pad
        out = torch.zeros(shape, dtype=v.dtype, device=v.device)
        out.narrow(dim, 0, v.shape[dim]).copy_(v.detach())
        return nn.Parameter(out, requires_grad=False)
    if isinstance(c2, GATConv):
        s2 = GATConv(c2.in_channels, o_pad, c2.negative_slope)
        s2.lin_src.weight = padded(c2.lin_src.weight, 0)
        s2.lin_dst = s2.lin_src
        s2.att_src, s2.att_dst = padded(c2.att_src, -1), padded(c2.att_dst, -1)
    else:
        s2 = GCNConv(c2.in_channels, o_pad)
        s2.lin.weight = padded(c2.lin.weight, 0)
    s2.bias = padded(c2.bias, 0)
    return s2


def _block(t, like):
    """The top-left block of t with like's shape."""
    return t[tuple(slice(0, k) for k in like.shape)]


def col_sum(x, row_w=None, gate=None, gated=None, out=None, ws=None):
    """out[j] = sum_r row_w[r] * [gate[r, j] > 0] * x[r, j] (gd_col_sum_f32); gated (may be x): receives the gated matrix."""
    L = _lib.lib()
    n, d = int(x.shape[0]), int(x.shape[1])
    if out is None:
        out = torch.empty(d, dtype=torch.float32, device=x.device)
    if ws is None:
        ws = torch.empty(max(4, L.gd_col_sum_workspace(n, d)), dtype=torch.float32, device=x.device)
    for t in (gate, gated):
        assert t is None or (t.stride(0) == x.stride(0) and t.shape == x.shape)
    check(L.gd_col_sum_f32(ptr(x), x.stride(0), n, d, ptr(row_w), ptr(gate), ptr(gated), ptr(out), ptr(ws), stream_ptr(x.device)),
          'gd_col_sum_f32')
    return out


class BackboneEngine(DeviceNegatives):
    """One backbone-training request: model (GCN / GAT of framework/models/backbones.py, every parameter is stepped in place),
    node features, the message-passing edges, the positive decoded edges (int64 [2, P]) and the number of negatives per epoch.
    step(neg) takes the epoch's negatives from the caller; after enable_device_negatives(pos_keys, seed), step_device() draws
    them on the device."""

    def __init__(self, model, x, mp_edges, pos_edges, n_neg, lr, betas, eps, history=4096, use_graph=True):
        self._setup(model, x, mp_edges, lr, betas, eps, history, use_graph)
        dev, n, O = self.dev, self.n, self.O
        L = _lib.lib()
        f32, i64 = dict(dtype=torch.float32, device=dev), dict(dtype=torch.int64, device=dev)
        # the decoded edges [pos | neg]: the positive half is fixed, the negatives' half is rewritten by step()
        P, n_neg = self.P, self.n_neg = int(pos_edges.shape[1]), int(n_neg)
        M = self.M = P + n_neg
        self._n_fixed = P
        if M < 1:
            raise ValueError('BackboneEngine: no decoded edges (upstream\'s mean over nothing is NaN)')
        self.dec = torch.zeros(2, M, **i64)
        self.dec[:, :P] = pos_edges.to(dev)
        self.inc_ptr = torch.zeros(n + 1, **i64)
        self.other = torch.zeros(2 * M, dtype=torch.int32, device=dev)
        self.src_edge = torch.zeros(2 * M, dtype=torch.int32, device=dev)
        self.inc_ws = torch.empty(L.gd_edge_incidence_workspace(n, M), dtype=torch.uint8, device=dev)
        self.w = torch.zeros(M, **f32)
        self.w_inc = torch.zeros(2 * M, **f32)
        self.bce_ws = torch.empty(max(1, L.gd_edge_bce_workspace(M, O)), **f32)

    def _setup(self, model, x, mp_edges, lr, betas, eps, history, use_graph, conv2=None):
        """Everything but the loss stage's buffers.  conv2: the module trained as layer 2 in place of the model's own (a
        zero-padded shadow, NodeClassifierEngine); self.params are the tensors stepped, self.user_params the model's."""
        from .graph import graph_for
        from .nn import GATConv
        dev = next(model.parameters()).device
        self.dev, self.model = dev, model
        self.lr, self.betas, self.eps = float(lr), (float(betas[0]), float(betas[1])), float(eps)
        c1, c2 = self.convs = (model.conv1, model.conv2 if conv2 is None else conv2)
        self.gat = isinstance(c1, GATConv)
        self.x = ops._f32_rows(x.to(dev, torch.float32))
        n = self.n = int(self.x.shape[0])
        mp_edges = mp_edges.to(dev).contiguous()
        self.graph = graph_for(mp_edges, n, 'gat' if self.gat else 'gcn')
        self.w1, self.w2 = ((c.lin_src if self.gat else c.lin).weight for c in self.convs)         # [H, F], [O, H]
        F_in, H, O = self.F, self.H, self.O = int(self.w1.shape[1]), int(self.w1.shape[0]), int(self.w2.shape[0])
        if H % 4 or O % 4 or max(H, O) > 1024 or int(self.x.shape[1]) != F_in or int(self.w2.shape[1]) != H:
            raise ValueError(f'BackboneEngine: widths {F_in} -> {H} -> {O} (hidden and output: multiples of 4 up to 1024)')
        self.user_params = list(model.parameters())
        self.params = self.user_params
        if conv2 is not None:
            stepped = dict(conv2.named_parameters())
            self.params = [stepped[k[len('conv2.'):]] if k.startswith('conv2.') else p for k, p in model.named_parameters()]
        f32, i64 = dict(dtype=torch.float32, device=dev), dict(dtype=torch.int64, device=dev)
        self.grads = {id(p): torch.zeros_like(p.data) for p in self.params}
        L = _lib.lib()
        # the first product and its weight gradient on the constant x: ops._Dense's choice of kernels, its padded / transposed
        # copies of x made once (and shared with it through the constant-operand cache, pinned here)
        self._consts = {}
        mult = 128 if ops.matrix_split() == 6 else 32
        if ops._small_weight(F_in, H) and self.x.stride(0) % 4 == 0:
            self.fwd1 = 'rows'
        elif ops.mfma_out_width(H):
            self.fwd1 = 'wide'
        elif F_in <= 1024:
            self.fwd1 = 'rows'
        else:
            raise ValueError(f'BackboneEngine: no kernel for a {F_in} -> {H} first product')
        if H % 32 == 0 and F_in % 32 == 0 and H <= 128 and F_in <= 128 and H != 96 and F_in != 96:
            self.wgrad1 = 'rows'
        elif ops.mfma_out_width(H) and n >= 32:
            self.wgrad1 = 'xT'
        else:
            self.wgrad1 = 'rows'
        with ops.keep_constants(self._consts):
            if self.fwd1 == 'wide':
                self.xp = ops._cached(f'padx{mult}', self.x, lambda t: ops._pad_cols32(t, mult))
                kp = int(self.xp.shape[1])
                self.w1t = torch.zeros(kp, H, **f32)                  # W1^T, zero rows below F
                self.ws_fwd1 = torch.empty(max(4, L.gd_gemm_f32_workspace(n, kp, H)), **f32)
            if self.wgrad1 == 'xT':
                def transpose_pad(t):
                    mp = (t.shape[0] + mult - 1) // mult * mult
                    xt = torch.zeros(t.shape[1], mp, dtype=torch.float32, device=t.device)
                    xt[:, :t.shape[0]] = t.t()
                    return xt
                self.xt = ops._cached('xT' if mult == 32 else f'xT{mult}', self.x, transpose_pad)
                mp = int(self.xt.shape[1])
                self.dyp = torch.zeros(mp, H, **f32)                  # dL/d(x W1^T), zero rows below n
                self.dw1t = torch.empty(F_in, H, **f32)
                self.ws_wgrad1 = torch.empty(max(4, L.gd_gemm_f32_workspace(F_in, mp, H)), **f32)
        self.loss = torch.zeros(1, **f32)
        # activations and gradients: static buffers (a captured graph replays from their addresses)
        self.t1, self.p1, self.dx1 = (torch.empty(n, H, **f32) for _ in range(3))
        self.q1 = self.dyp[:n] if (self.wgrad1 == 'xT' and not self.gat) else torch.empty(n, H, **f32)
        self.t2, self._z, self.q2 = (torch.empty(n, O, **f32) for _ in range(3))
        self.g = torch.zeros(n, O, **f32)                           # dL/dz (the node-classification loss writes its rows only)
        self.cs_ws = torch.empty(max(4, L.gd_col_sum_workspace(n, max(H, O))), **f32)
        self._bufs = ({}, {})                                       # the GAT layers' row statistics and edge gradients
        self.adam = [{'m': torch.zeros_like(p.data), 'v': torch.zeros_like(p.data),
                      'step': torch.zeros(1, dtype=torch.int32, device=dev), 'steps': 0} for p in self.params]
        self.hist = torch.zeros(int(history), 3, **f32)
        self.hist_pos = torch.zeros(1, dtype=torch.int32, device=dev)
        self.steps_done = 0
        self._use_graph, self._graph = bool(use_graph), None
        self.events = None              # list -> (stage, cuda event) pairs of the eager step (the experiment's stage split)

    def _mark(self, stage):
        if self.events is not None and self._graph is None and not torch.cuda.is_current_stream_capturing():
            ev = torch.cuda.Event(enable_timing=True)
            ev.record()
            self.events.append((stage, ev))

    def _grad(self, p):
        return self.grads[id(p)]

    # ---------------------------------------------------------------------------------------------- the first product
    def _first_product(self, out):
        w1 = self.w1.data
        if self.fwd1 == 'rows':
            return ops.rows_gemm(self.x, None, w1, trans_w=True, out=out)
        self.w1t[:self.F].copy_(w1.t())
        check(_lib.lib().gd_gemm_f32(ptr(self.xp), self.xp.stride(0), None, self.n, ptr(self.w1t), int(self.xp.shape[1]), self.H,
                                     None, ptr(out), out.stride(0), ptr(self.ws_fwd1), stream_ptr(self.dev)), 'gd_gemm_f32')
        return out

    def _first_wgrad(self, dy):
        """dW1 [H, F] = dy^T x into W1's gradient buffer; on the x^T form dy must be self.dyp[:n]."""
        gw1 = self._grad(self.w1)
        if self.wgrad1 == 'rows':
            return ops.rows_gemm_wgrad(dy, None, self.x, None, self.n, out=gw1)
        if dy.data_ptr() != self.dyp.data_ptr():
            self.dyp[:self.n].copy_(dy)
        mp = int(self.xt.shape[1])
        check(_lib.lib().gd_gemm_f32(ptr(self.xt), self.xt.stride(0), None, self.F, ptr(self.dyp), mp, self.H, None, ptr(self.dw1t),
                                     self.dw1t.stride(0), ptr(self.ws_wgrad1), stream_ptr(self.dev)), 'gd_gemm_f32')
        return gw1.copy_(self.dw1t.t())

    # ---------------------------------------------------------------------------------------------- the fixed-shape step
    def _loss_and_dz(self):
        L, dev, z, P = _lib.lib(), self.dev, self._z, self.P
        check(L.gd_edge_bce_f32(ptr(z), z.stride(0), self.n, self.O, ptr(self.dec), self.M, P, self.dec.data_ptr() + 8 * P, self.M,
                                self.n_neg, 1.0, ptr(self.w), ptr(self.loss), ptr(self.src_edge), ptr(self.inc_ptr), ptr(self.w_inc),
                                ptr(self.bce_ws), stream_ptr(dev)), 'gd_edge_bce_f32')
        check(L.gd_edge_dot_bwd_f32(ptr(z), z.stride(0), self.O, ptr(self.other), ptr(self.w_inc), None, 0, None, ptr(self.inc_ptr),
                                    self.n, ptr(self.g), self.g.stride(0), stream_ptr(dev)), 'gd_edge_dot_bwd_f32')
        check(L.gd_edgeprob_record_f32(ptr(self.loss), None, 1.0, 0.0, ptr(self.hist), self.hist.shape[0], ptr(self.hist_pos),
                                       stream_ptr(dev)), 'gd_edgeprob_record_f32')

    def _iteration_gcn(self):
        g, n = self.graph, self.n
        c1, c2 = self.convs
        w2, b1, b2 = self.w2.data, c1.bias.data, c2.bias.data
        self._first_product(self.t1)
        ops._spmm_raw(g.rowptr, g.col, g.val, self.t1, b1, 0.0, n, g.plan, out=self.p1)
        ops.rows_gemm(self.p1, None, w2, trans_w=True, relu_in=True, out=self.t2)
        ops._spmm_raw(g.rowptr, g.col, g.val, self.t2, b2, 0.0, n, g.plan, out=self._z)
        self._mark('forward')
        self._loss_and_dz()
        self._mark('loss')
        col_sum(self.g, out=self._grad(c2.bias), ws=self.cs_ws)
        ops._spmm_raw(g.rowptr_t, g.col_t, g.val_t, self.g, None, 0.0, n, g.plan_t, out=self.q2)
        ops.rows_gemm_wgrad(self.q2, None, self.p1, None, n, relu_mask=self.p1, out=self._grad(self.w2))
        ops.rows_gemm(self.q2, None, w2, out=self.dx1)
        col_sum(self.dx1, gate=self.p1, gated=self.dx1, out=self._grad(c1.bias), ws=self.cs_ws)       # dp1 in place, db1
        ops._spmm_raw(g.rowptr_t, g.col_t, g.val_t, self.dx1, None, 0.0, n, g.plan_t, out=self.q1)
        self._first_wgrad(self.q1)

    def _gat_layer_backward(self, k, h, stats, dy):
        """GATConv k's backward from dy = dL/d(output): the attention-vector gradients into their buffers -> dL/dh.  (The bias
        gradient, colsum(dy), is the caller's: layer 1's comes out of the pass that applies the ReLU gate.)"""
        c = self.convs[k]
        a_s, a_d, rowmax, rowsum = stats
        dh, da_s, da_d = ops.gat_backward_raw(self.graph, h, a_s, a_d, rowmax, rowsum, dy, float(c.negative_slope), bufs=self._bufs[k])
        col_sum(h, row_w=da_s, out=self._grad(c.att_src).view(-1), ws=self.cs_ws)
        col_sum(h, row_w=da_d, out=self._grad(c.att_dst).view(-1), ws=self.cs_ws)
        return ops.rank1_add2_(dh, da_s, c.att_src.data.view(-1), da_d, c.att_dst.data.view(-1))

    def _gat_layer_forward(self, k, h, out):
        c = self.convs[k]
        a_s, a_d = ops.row_dots(h, c.att_src.data.view(-1), c.att_dst.data.view(-1), bufs=self._bufs[k])
        _, rowmax, rowsum = ops.gat_forward_raw(self.graph, h, a_s, a_d, c.bias.data, float(c.negative_slope), out=out, bufs=self._bufs[k])
        return a_s, a_d, rowmax, rowsum

    def _iteration_gat(self):
        n, w2 = self.n, self.w2.data
        self._first_product(self.t1)
        st1 = self._gat_layer_forward(0, self.t1, self.p1)
        ops.rows_gemm(self.p1, None, w2, trans_w=True, relu_in=True, out=self.t2)
        st2 = self._gat_layer_forward(1, self.t2, self._z)
        self._mark('forward')
        self._loss_and_dz()
        self._mark('loss')
        col_sum(self.g, out=self._grad(self.convs[1].bias), ws=self.cs_ws)
        dh2 = self._gat_layer_backward(1, self.t2, st2, self.g)
        ops.rows_gemm_wgrad(dh2, None, self.p1, None, n, relu_mask=self.p1, out=self._grad(self.w2))
        ops.rows_gemm(dh2, None, w2, out=self.dx1)
        col_sum(self.dx1, gate=self.p1, gated=self.dx1, out=self._grad(self.convs[0].bias), ws=self.cs_ws)   # dp1 in place, db1
        dh1 = self._gat_layer_backward(0, self.t1, st1, self.dx1)
        self._first_wgrad(dh1)

    def _iteration(self):
        with torch.no_grad(), ops.keep_constants(self._consts):
            (self._iteration_gat if self.gat else self._iteration_gcn)()
            L = _lib.lib()
            for st, p in zip(self.adam, self.params):
                check(L.gd_adam_f32(ptr(p.data), ptr(self._grad(p)), ptr(st['m']), ptr(st['v']), ptr(st['step']), p.numel(), self.lr,
                                    self.betas[0], self.betas[1], self.eps, stream_ptr(self.dev)), 'gd_adam_f32')
            for p, q in zip(self.params, self.user_params):
                if p is not q:
                    q.data.copy_(_block(p.data, q))                  # the model's own layer 2 <- the shadow's top-left block
            self._mark('backward')

    def _mutable_state(self):
        state = [p.data for p in self.params] + [q.data for p, q in zip(self.params, self.user_params) if p is not q]
        state += [self.hist, self.hist_pos]
        for st in self.adam:
            state += [st['m'], st['v'], st['step']]
        return state

    def _capture(self):
        self._graph = capture_iterations(self._iteration, self._mutable_state)

    # ---------------------------------------------------------------------------------------------- public
    def step(self, neg):
        """One epoch on this epoch's negatives ([2, n_neg] int64, any device)."""
        P, M = self.P, self.M
        if tuple(neg.shape) != (2, self.n_neg):
            raise ValueError(f'BackboneEngine.step: negatives of shape {tuple(neg.shape)}, expected (2, {self.n_neg})')
        self._mark('start')
        if self.n_neg:
            self.dec[:, P:].copy_(neg, non_blocking=True)
        check(_lib.lib().gd_edge_incidence(ptr(self.dec[0]), ptr(self.dec[1]), M, self.n, ptr(self.inc_ptr), ptr(self.other),
                                           ptr(self.src_edge), ptr(self.inc_ws), self.inc_ws.numel(), stream_ptr(self.dev)),
              'gd_edge_incidence')
        self._mark('incidence')
        self._run_iteration()

    def step_device(self):
        """One epoch on negatives drawn on the device (enable_device_negatives first): the draw into the negatives' half of the
        decoded edges, the incidence list merged from the positives' image, the iteration as in step(), the draw counter + 1 -
        stream launches and a graph replay, no host read, no allocation."""
        self._draw_and_merge()
        self._run_iteration()
        self._next_draw()

    def _run_iteration(self):
        if not self._use_graph:
            self._iteration()
        else:
            if self._graph is None:
                self._capture()
            self._graph.replay()
        for st in self.adam:
            st['steps'] += 1
        self.steps_done += 1

    @property
    def z(self):
        """The latest forward's output, [n, layer 2's own width] (a view of the engine's buffer)."""
        return self._z[:, :int(self.model.conv2.out_channels)]

    def last_loss(self):
        """train_loss of the latest step: one blocking host read."""
        return float(self.hist[(self.steps_done - 1) % self.hist.shape[0], 0])

    def loss_history(self):
        """[steps] host tensor of the train losses, oldest first, of the steps the ring still holds."""
        cap = self.hist.shape[0]
        h = self.hist[:, 0].cpu()
        if self.steps_done <= cap:
            return h[:self.steps_done]
        at = self.steps_done % cap
        return torch.cat([h[at:], h[:at]])

    # ---------------------------------------------------------------------------------------------- optimizer state
    def import_adam_state(self, optimizer):
        for st, p in zip(self.adam, self.user_params):
            have = optimizer.state.get(p)
            if have and 'exp_avg' in have:
                for mine, theirs in ((st['m'], have['exp_avg']), (st['v'], have['exp_avg_sq'])):
                    mine.zero_()                                     # (a shadow's padding: zero moments)
                    _block(mine, p).copy_(theirs)
                st['steps'] = int(have['step'])
                st['step'].fill_(st['steps'])

    def export_adam_state(self, optimizer):
        """Adam moments and step count of every parameter into the caller's optimizer; the gradients are not kept (the
        autograd loop's zero_grad after the step)."""
        for st, p in zip(self.adam, self.user_params):
            if st['steps']:
                optimizer.state[p] = {'step': torch.tensor(float(st['steps'])), 'exp_avg': _block(st['m'], p).clone(),
                                      'exp_avg_sq': _block(st['v'], p).clone()}
            p.grad = None


class NodeClassifierEngine(BackboneEngine):
    """One node-classifier training request (NodeClassificationTrainer.train): model (GCN / GAT whose output width is the class
    count C <= 256), node features, the message-passing edges, the labels y (int64, by node id) and the boolean train mask.
    With padded_class_width(C) == C every parameter is stepped in place; otherwise layer 2 is trained on zero-padded shadows
    (self.shadows: parameter name -> padded tensor) and the model's own tensors are refreshed inside every iteration."""

    def __init__(self, model, x, edge_index, y, train_mask, lr, betas, eps, history=4096, use_graph=True):
        dev = next(model.parameters()).device
        C = self.C = int(model.conv2.out_channels)
        if C > 256:
            raise ValueError(f'NodeClassifierEngine: {C} classes (up to 256)')
        rows = train_mask.to(dev).nonzero().flatten()
        if rows.numel() < 1:
            raise ValueError('NodeClassifierEngine: an empty train mask (upstream\'s mean over nothing is NaN)')
        y = y.to(dev, torch.int64).contiguous()
        if y.numel() != int(x.shape[0]) or int(y[rows].min()) < 0 or int(y[rows].max()) >= C:
            raise ValueError(f'NodeClassifierEngine: a training row\'s label lies outside [0, {C})')
        o_pad = padded_class_width(C)
        shadow = _padded_conv2(model.conv2, o_pad).to(dev) if o_pad != C else None
        self._setup(model, x, edge_index, lr, betas, eps, history, use_graph, conv2=shadow)
        self.shadows = {k: p for (k, q), p in zip(model.named_parameters(), self.params) if p is not q}
        self.y, self.rows = y, rows.to(torch.int32).contiguous()
        self.nll_ws = torch.empty(max(1, _lib.lib().gd_row_nll_workspace(self.rows.numel(), self.O)), dtype=torch.float32, device=dev)

    def _loss_and_dz(self):
        L, dev, z, g = _lib.lib(), self.dev, self._z, self.g
        check(L.gd_row_nll_f32(ptr(z), z.stride(0), self.n, self.O, self.C, ptr(self.rows), self.rows.numel(), ptr(self.y), 1.0,
                               ptr(g), g.stride(0), ptr(self.loss), ptr(self.nll_ws), stream_ptr(dev)), 'gd_row_nll_f32')
        check(L.gd_edgeprob_record_f32(ptr(self.loss), None, 1.0, 0.0, ptr(self.hist), self.hist.shape[0], ptr(self.hist_pos),
                                       stream_ptr(dev)), 'gd_edgeprob_record_f32')

    def step(self):
        """One epoch: one graph replay."""
        self._mark('start')
        self._run_iteration()

    def enable_device_negatives(self, pos_keys, seed, counter=0):
        raise TypeError('NodeClassifierEngine: the node-classification step decodes no edges and draws no negatives')
