"""Edge-probability unlearning (--unlearning_model gnndelete --fused_edgeprob) on a fused HIP step.

GNNDeleteTrainer.train_fullbatch (framework/trainer/gnndelete.py) runs the paper's own method as an autograd loop: the
frozen layer 1 again every epoch, two decoder launches and F.mse_loss, a torch.sort + searchsorted for the decoder's
backward, zeros + index_copy_ for the pair term, torch's Adam.  EdgeprobEngine is the same step with an explicit forward,
a hand-derived backward and the library's Adam - MinibatchNodeembStep's shape, with what NodeembEngine does for a fixed
request: layer 1 once, the CSR and its transpose once, and the step captured in a hipGraph.

  z1 = p1, rows S1 <- p1[S1] W_D1;  c2 = conv2(relu(z1));  z2 = c2, rows S2 <- c2[S2] W_D2
  loss_r, w  <- gd_edgeprob_dec_f32 (w already in incidence order);   g <- gd_edge_dot_bwd_f32
  loss_l, dzp <- gd_pairs_sigmoid_mse_f32;   g[nodes] += 0.5 dzp (gd_rows_add_f32)
  dW_D2 = c2[S2]^T g[S2];  g[S2] <- g[S2] W_D2^T;  dh = conv2 backward;  dW_D1 = p1[S1]^T (dh W2 * [z1 > 0])[S1]
  one Adam step on both weights;  (0.5 loss_r + 0.5 loss_l, loss_l, loss_r) -> a device history ring

The negatives change every epoch: step(neg) copies them into a fixed [2, m] slot and rebuilds the incidence list on the
device (gd_edge_incidence); everything after that is one graph replay, bit-identical to the eager step."""
import torch

from . import _lib, ops
from ._lib import check, ptr, stream_ptr
from .capture import capture_iterations
from .negatives import DeviceNegatives


def fused_edgeprob_unsupported(model, args, optimizer):
    """None when the fused edge-probability step applies, else the reason it does not (one line)."""
    from .framework.trainer.sampler import data_parallel_world
    from .nn import GATConv, GCNConv
    conv1, conv2 = getattr(model, 'conv1', None), getattr(model, 'conv2', None)
    if not (isinstance(conv1, (GCNConv, GATConv)) and type(conv1) is type(conv2)) or not hasattr(model, 'deletion1'):
        return f'no fused edge-probability step for the {type(model).__name__} backbone (GCN and GAT only)'
    um = getattr(args, 'unlearning_model', 'gnndelete')
    if 'kld' in um or 'ablation' in um:
        return f'--unlearning_model {um} is not the MSE loss'
    if data_parallel_world()[1] > 1:
        return 'torch.distributed with more than one rank'
    if isinstance(optimizer, (list, tuple)) or not isinstance(optimizer, torch.optim.Adam):
        return 'the optimizer is not one plain torch.optim.Adam'
    g = optimizer.param_groups[0]
    if len(optimizer.param_groups) != 1 or g.get('weight_decay', 0) or g.get('amsgrad') or g.get('maximize'):
        return 'the optimizer is not one plain torch.optim.Adam'
    dels = {id(model.deletion1.deletion_weight), id(model.deletion2.deletion_weight)}
    if {id(p) for p in g['params']} != dels:
        return 'the optimizer does not hold exactly the two Del weights'
    if conv1.out_channels % 4 or conv2.out_channels % 4 or max(conv1.out_channels, conv2.out_channels) > 1024:
        return f'widths {conv1.out_channels} / {conv2.out_channels} (multiples of 4 up to 1024)'
    return None


def edge_incidence(e0, e1, n):
    """gd_edge_incidence: (inc_ptr [n + 1] int64, other [2M] int32, src_edge [2M] int32) of the M edges (e0, e1)."""
    e0, e1 = e0.contiguous().long(), e1.contiguous().long()
    m2 = int(e0.shape[0])
    dev = e0.device
    inc_ptr = torch.empty(n + 1, dtype=torch.int64, device=dev)
    other = torch.empty(max(2 * m2, 1), dtype=torch.int32, device=dev)
    src_edge = torch.empty(max(2 * m2, 1), dtype=torch.int32, device=dev)
    L = _lib.lib()
    ws = torch.empty(L.gd_edge_incidence_workspace(n, m2), dtype=torch.uint8, device=dev)
    check(L.gd_edge_incidence(ptr(e0), ptr(e1), m2, n, ptr(inc_ptr), ptr(other), ptr(src_edge), ptr(ws), ws.numel(),
                              stream_ptr(dev)), 'gd_edge_incidence')
    return inc_ptr, other[:2 * m2], src_edge[:2 * m2]


def edge_incidence_image(e0, e1, n_fixed, n):
    """gd_edge_incidence_fixed: the image (an opaque int64 tensor) of the first n_fixed edges of (e0, e1) over n nodes."""
    e0, e1 = e0.contiguous().long(), e1.contiguous().long()
    dev, L = e0.device, _lib.lib()
    image = torch.empty(L.gd_edge_incidence_fixed_bytes(n, n_fixed) // 8 + 1, dtype=torch.int64, device=dev)
    ws = torch.empty(L.gd_edge_incidence_update_workspace(n, n_fixed) // 8 + 1, dtype=torch.int64, device=dev)
    check(L.gd_edge_incidence_fixed(ptr(e0), ptr(e1), n_fixed, n, ptr(image), 8 * image.numel(), ptr(ws), 8 * ws.numel(),
                                    stream_ptr(dev)), 'gd_edge_incidence_fixed')
    return image


def edge_incidence_update(image, e0, e1, n_fixed, n):
    """gd_edge_incidence_update: edge_incidence(e0, e1, n)'s three arrays from the image of the first n_fixed edges and the
    edges [n_fixed, M) of (e0, e1)."""
    e0, e1 = e0.contiguous().long(), e1.contiguous().long()
    m2 = int(e0.shape[0])
    dev, L = e0.device, _lib.lib()
    inc_ptr = torch.empty(n + 1, dtype=torch.int64, device=dev)
    other = torch.empty(max(2 * m2, 1), dtype=torch.int32, device=dev)
    src_edge = torch.empty(max(2 * m2, 1), dtype=torch.int32, device=dev)
    ws = torch.empty(L.gd_edge_incidence_update_workspace(n, m2) // 8 + 1, dtype=torch.int64, device=dev)
    check(L.gd_edge_incidence_update(ptr(image), ptr(e0), ptr(e1), n_fixed, m2, n, ptr(inc_ptr), ptr(other), ptr(src_edge), ptr(ws),
                                     8 * ws.numel(), stream_ptr(dev)), 'gd_edge_incidence_update')
    return inc_ptr, other[:2 * m2], src_edge[:2 * m2]


def rows_add_(dz, nodes, src, scale):
    """dz[nodes[i], :] += scale * src[i, :] in place for sorted unique int32 rows (gd_rows_add_f32)."""
    n_s = int(nodes.shape[0])
    check(_lib.lib().gd_rows_add_f32(ptr(dz), dz.stride(0), dz.shape[0], ptr(nodes), n_s, ptr(src), src.stride(0), float(scale),
                                     dz.shape[1], stream_ptr(dz.device)), 'gd_rows_add_f32')
    return dz


class EdgeprobEngine(DeviceNegatives):
    """One edge-probability request: model (GCNDelete / GATDelete, its Del weights are stepped in place), node features,
    the S_Df edges of the forward, the Df edges, and the pair term's (nodes int32, dense target, pair count) as
    GNNDeleteTrainer builds them (target None / n_pairs 0: no pair term, loss_l = 0).  step(neg) takes the epoch's negatives
    from the caller; after enable_device_negatives(pos_keys, seed), step_device() draws them on the device."""

    def __init__(self, model, x, e_sdf, df_edges, nodes32, target, n_pairs, lr, betas, eps, history=4096, use_graph=True):
        from .graph import graph_for
        from .nn import GATConv
        dev = next(model.parameters()).device
        self.dev, self.model = dev, model
        self.lr, self.betas, self.eps = float(lr), (float(betas[0]), float(betas[1])), float(eps)
        self.gat = isinstance(model.conv1, GATConv)
        c1, c2 = model.conv1, model.conv2
        n = self.n = int(x.shape[0])
        e_sdf = e_sdf.to(dev).contiguous()
        self.graph = graph_for(e_sdf, n, 'gat' if self.gat else 'gcn')
        with torch.no_grad():                                   # frozen layer 1: once per request
            self.p1 = ops._f32_rows(c1(x.to(dev, torch.float32), e_sdf)).contiguous()
        lin2 = c2.lin_src if self.gat else c2.lin
        self.w2 = lin2.weight.detach().contiguous()             # [O, H]
        self.b2 = c2.bias.detach().contiguous()
        if self.gat:
            self.att2 = (c2.att_src.detach().reshape(-1).contiguous(), c2.att_dst.detach().reshape(-1).contiguous())
            self.slope2 = float(c2.negative_slope)
        H, O = self.H, self.O = int(self.p1.shape[1]), int(self.w2.shape[0])
        if H % 4 or O % 4:
            raise ValueError(f'EdgeprobEngine: widths {H} / {O} must be multiples of 4')

        def rows(layer):
            if layer.mask is None:
                return torch.empty(0, dtype=torch.int32, device=dev)
            return layer._rows.get(layer.mask, dev).contiguous()
        self.idx1, self.idx2 = rows(model.deletion1), rows(model.deletion2)
        self.s1, self.s2 = int(self.idx1.shape[0]), int(self.idx2.shape[0])
        self.wd1, self.wd2 = model.deletion1.deletion_weight, model.deletion2.deletion_weight
        # the decoded edges [pos | neg]: the Df half is fixed, the negatives' half is rewritten by step()
        m = self.m = self._n_fixed = int(df_edges.shape[1])
        if m < 1:
            raise ValueError('EdgeprobEngine: no Df edges (upstream\'s MSE of nothing is NaN)')
        i64 = dict(dtype=torch.int64, device=dev)
        self.dec = torch.zeros(2, 2 * m, **i64)
        self.dec[:, :m] = df_edges.to(dev)
        self.inc_ptr = torch.zeros(n + 1, **i64)
        self.other = torch.zeros(4 * m, dtype=torch.int32, device=dev)
        self.src_edge = torch.zeros(4 * m, dtype=torch.int32, device=dev)
        L = _lib.lib()
        self.inc_ws = torch.empty(L.gd_edge_incidence_workspace(n, 2 * m), dtype=torch.uint8, device=dev)
        f32 = dict(dtype=torch.float32, device=dev)
        self.w = torch.zeros(2 * m, **f32)
        self.w_inc = torch.zeros(4 * m, **f32)
        self.dec_ws = torch.empty(max(1, L.gd_edgeprob_dec_workspace(m, O)), **f32)
        self.loss_r, self.loss_l = torch.zeros(1, **f32), torch.zeros(1, **f32)
        # the pair term
        self.n_pairs = int(n_pairs) if target is not None else 0
        if self.n_pairs:
            self.nodes32, self.target = nodes32.contiguous(), target
            n_s = int(nodes32.shape[0])
            self.dzp = torch.empty(max(1, n_s), O, **f32)
            self.pairs_ws = torch.empty(L.gd_pairs_sigmoid_mse_workspace(n_s, O), **f32)
        # activations and gradients: static buffers (a captured graph replays from their addresses)
        self.z1 = self.p1.clone()                               # rows outside S1 never change
        self.h2 = torch.empty(n, O, **f32)
        self.c2, self.z2, self.g, self.dh = (torch.empty(n, O, **f32) for _ in range(4))
        self.dx1 = torch.empty(n, H, **f32)
        self.g1, self.g2 = torch.zeros_like(self.wd1.data), torch.zeros_like(self.wd2.data)
        self._gat_bufs = {}
        self.adam = [{'m': torch.zeros_like(p.data), 'v': torch.zeros_like(p.data),
                      'step': torch.zeros(1, dtype=torch.int32, device=dev), 'steps': 0} for p in (self.wd1, self.wd2)]
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

    # ---------------------------------------------------------------------------------------------- the fixed-shape step
    def _iteration(self):
        L, dev, g = _lib.lib(), self.dev, self.graph
        n, O, m = self.n, self.O, self.m
        wd1, wd2 = self.wd1.data, self.wd2.data
        # forward
        if self.s1:
            ops.rows_gemm(self.p1, self.idx1, wd1, out=self.z1)
        ops.rows_gemm(self.z1, None, self.w2, trans_w=True, relu_in=True, out=self.h2)
        if self.gat:
            a_s, a_d = ops.row_dots(self.h2, *self.att2, bufs=self._gat_bufs)
            _, rowmax, rowsum = ops.gat_forward_raw(g, self.h2, a_s, a_d, self.b2, self.slope2, out=self.c2, bufs=self._gat_bufs)
        else:
            ops._spmm_raw(g.rowptr, g.col, g.val, self.h2, self.b2, 0.0, n, g.plan, out=self.c2)
        self.z2.copy_(self.c2)
        if self.s2:
            ops.rows_gemm(self.c2, self.idx2, wd2, out=self.z2)
        self._mark('forward')
        # DEC term and the decoder's input gradient; the pair term joins it on its rows
        z2 = self.z2
        check(L.gd_edgeprob_dec_f32(ptr(z2), z2.stride(0), n, O, ptr(self.dec), 2 * m, self.dec.data_ptr() + 8 * m, 2 * m, m, 0.5,
                                    ptr(self.w), ptr(self.loss_r), ptr(self.src_edge), ptr(self.inc_ptr), ptr(self.w_inc),
                                    ptr(self.dec_ws), stream_ptr(dev)), 'gd_edgeprob_dec_f32')
        check(L.gd_edge_dot_bwd_f32(ptr(z2), z2.stride(0), O, ptr(self.other), ptr(self.w_inc), None, 0, None, ptr(self.inc_ptr),
                                    n, ptr(self.g), self.g.stride(0), stream_ptr(dev)), 'gd_edge_dot_bwd_f32')
        if self.n_pairs:
            n_s = int(self.nodes32.shape[0])
            check(L.gd_pairs_sigmoid_mse_f32(ptr(z2), z2.stride(0), ptr(self.nodes32), n_s, O, ptr(self.target),
                                             self.target.stride(0), 1.0 / self.n_pairs, ptr(self.loss_l), ptr(self.dzp),
                                             ptr(self.pairs_ws), stream_ptr(dev)), 'gd_pairs_sigmoid_mse_f32')
            rows_add_(self.g, self.nodes32, self.dzp, 0.5)
        check(L.gd_edgeprob_record_f32(ptr(self.loss_r), ptr(self.loss_l) if self.n_pairs else None, 0.5, 0.5, ptr(self.hist),
                                       self.hist.shape[0], ptr(self.hist_pos), stream_ptr(dev)), 'gd_edgeprob_record_f32')
        self._mark('loss')
        # backward: Del 2, conv2 to its input, the ReLU gate folded into Del 1's weight gradient
        if self.s2:
            ops.rows_gemm_wgrad(self.c2, self.idx2, self.g, self.idx2, self.s2, out=self.g2)
            ops.rows_gemm(self.g, self.idx2, wd2, trans_w=True, out=self.g)
        else:
            self.g2.zero_()
        if self.s1:
            if self.gat:
                dh, da_s, da_d = ops.gat_backward_raw(g, self.h2, a_s, a_d, rowmax, rowsum, self.g, self.slope2, bufs=self._gat_bufs)
                ops.rank1_add2_(dh, da_s, self.att2[0], da_d, self.att2[1])
            else:
                dh = ops._spmm_raw(g.rowptr_t, g.col_t, g.val_t, self.g, None, 0.0, n, g.plan_t, out=self.dh)
            ops.rows_gemm(dh, None, self.w2, out=self.dx1)
            ops.rows_gemm_wgrad(self.p1, self.idx1, self.dx1, self.idx1, self.s1, relu_mask=self.z1, out=self.g1)
        else:
            self.g1.zero_()
        for st, p, grad in zip(self.adam, (self.wd1, self.wd2), (self.g1, self.g2)):
            check(L.gd_adam_f32(ptr(p.data), ptr(grad), ptr(st['m']), ptr(st['v']), ptr(st['step']), p.numel(), self.lr,
                                self.betas[0], self.betas[1], self.eps, stream_ptr(dev)), 'gd_adam_f32')
        self._mark('backward')

    def _mutable_state(self):
        state = [self.wd1.data, self.wd2.data, self.hist, self.hist_pos]
        for st in self.adam:
            state += [st['m'], st['v'], st['step']]
        return state

    def _capture(self):
        self._graph = capture_iterations(self._iteration, self._mutable_state)

    # ---------------------------------------------------------------------------------------------- public
    def step(self, neg):
        """One epoch on this epoch's negatives ([2, m] int64, any device)."""
        m = self.m
        if tuple(neg.shape) != (2, m):
            raise ValueError(f'EdgeprobEngine.step: negatives of shape {tuple(neg.shape)}, expected (2, {m})')
        self._mark('start')
        self.dec[:, m:].copy_(neg, non_blocking=True)
        check(_lib.lib().gd_edge_incidence(ptr(self.dec[0]), ptr(self.dec[1]), 2 * m, self.n, ptr(self.inc_ptr), ptr(self.other),
                                           ptr(self.src_edge), ptr(self.inc_ws), self.inc_ws.numel(), stream_ptr(self.dev)),
              'gd_edge_incidence')
        self._mark('incidence')
        if not self._use_graph:
            self._iteration()
        else:
            if self._graph is None:
                self._capture()
            self._graph.replay()
        for st in self.adam:
            st['steps'] += 1
        self.steps_done += 1

    def step_device(self):
        """One epoch on negatives drawn on the device (enable_device_negatives first): the draw into the negatives' half of the
        decoded edges, the incidence list merged from the Df edges' image, the iteration as in step(), the draw counter + 1 -
        stream launches and a graph replay, no host read, no allocation."""
        self._draw_and_merge()
        if not self._use_graph:
            self._iteration()
        else:
            if self._graph is None:
                self._capture()
            self._graph.replay()
        for st in self.adam:
            st['steps'] += 1
        self.steps_done += 1
        self._next_draw()

    def last_losses(self):
        """(train_loss, loss_l, loss_r) of the latest step: one blocking host read."""
        row = self.hist[(self.steps_done - 1) % self.hist.shape[0]].tolist()
        return row[0], row[1], row[2]

    def loss_history(self):
        """[steps, 3] host tensor (train_loss, loss_l, loss_r), oldest first, of the steps the ring still holds."""
        cap = self.hist.shape[0]
        h = self.hist.cpu()
        if self.steps_done <= cap:
            return h[:self.steps_done]
        at = self.steps_done % cap
        return torch.cat([h[at:], h[:at]])

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
        """Adam moments and step count into the caller's optimizer (as _export_adam_state does for NodeembEngine); the
        gradients are not kept (the autograd loop's zero_grad after the step)."""
        for st, p in zip(self.adam, (self.wd1, self.wd2)):
            if st['steps']:
                optimizer.state[p] = {'step': torch.tensor(float(st['steps'])), 'exp_avg': st['m'].clone(),
                                      'exp_avg_sq': st['v'].clone()}
            p.grad = None
