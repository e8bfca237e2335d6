"""Per-epoch time of edge-probability unlearning (--unlearning_model gnndelete): today's autograd loop
(GNNDeleteTrainer.train_fullbatch without --fused_edgeprob) against the fused HIP step (gnndelete_amd.edgeprob), in one
process, the autograd loop first.

synth-dblp, GCN and GAT (in -> 128 -> 64), --df out --df_size 2.5.  Every epoch draws its negatives inside the timed
region, as the trainer does (the loop: negative_sampling; the engine: negative_sampling_cached).  Per path: 50 warm-up
epochs, then five regions of 50 epochs, each closed by the read of the last loss (the trainer's host read on a validation
epoch); the figure is the median region / 50.  The stage split of the fused step comes from CUDA events around the
eager (uncaptured) step; the negative draw is timed on its own (host clock, device synchronised).  A third leg is the
fused step on the device draw (--device_negatives: step_device, the draw and the incidence merge inside the timed region) on
a copy of the model; its regions alternate with the host-draw leg's.  Prints one JSON line per backbone and writes them all
to --out as one JSON object.

    python tools/experiments/edgeprob_fused.py [--out FILE] [--gnn gcn gat]"""
import argparse
import copy
import json
import os
import sys
import time
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

EPOCHS, REGIONS = 50, 5


def setup(gnn, seed=42):
    from gnndelete_amd.framework.data import prepare_edge_deletion, resolve_df_size
    from gnndelete_amd.framework.models import GATDelete, GCNDelete
    from gnndelete_amd.framework.synth import make_linkpred_dataset
    from gnndelete_amd.framework.trainer.gnndelete import sdf_pair_mask
    torch.manual_seed(seed)
    data, df = make_linkpred_dataset('synth-dblp', seed=seed)
    prepare_edge_deletion(data, df['out'], resolve_df_size(2.5, data.train_pos_edge_index.shape[1]))
    cls = GCNDelete if gnn == 'gcn' else GATDelete
    model = cls(SimpleNamespace(in_dim=data.x.shape[1], hidden_dim=128, out_dim=64), data.sdf_node_1hop_mask,
                data.sdf_node_2hop_mask).cuda()
    data = data.to('cuda')
    edges = data.train_pos_edge_index
    req = SimpleNamespace(data=data, edges=edges, e_sdf=edges[:, data.sdf_mask].contiguous(), df_edges=edges[:, data.df_mask],
                          m=int(data.df_mask.sum()))
    # the pair term's target as the trainer builds it; the original model's logits of the S_Df block from a seeded table
    nodes, pair_mask = sdf_pair_mask(data.num_nodes, data.sdf_node_2hop_mask, req.df_edges)
    req.n_pairs = int(pair_mask.sum())
    g = torch.Generator(device='cuda').manual_seed(seed)
    target = torch.randn(nodes.numel(), nodes.numel(), generator=g, device='cuda').sigmoid()
    target.masked_fill_(~pair_mask, -1.0)
    pad = (-target.shape[0]) % 4
    req.target = F.pad(target, (0, pad), value=-1.0).contiguous() if pad else target.contiguous()
    req.nodes32 = nodes.to(torch.int32).contiguous()
    return model, req


def region(epoch, read, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        epoch()
    read()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n


def measure(gnn):
    from gnndelete_amd import _lib, ops
    from gnndelete_amd.edgeprob import EdgeprobEngine
    from gnndelete_amd.framework import graph_utils as GU
    model, req = setup(gnn)
    data, lr = req.data, 1e-3
    dels = [model.deletion1.deletion_weight, model.deletion2.deletion_weight]
    start = [p.detach().clone() for p in dels]
    res = {'graph': 'synth-dblp', 'gnn': gnn, 'df': 'out', 'df_size': 2.5, 'nodes': int(data.num_nodes),
           'train_edges': int(req.edges.shape[1]), 'sdf_edges': int(req.e_sdf.shape[1]), 'df_edges': req.m,
           's2_nodes': int(req.nodes32.numel()), 'pairs': req.n_pairs, 'epochs_per_region': EPOCHS, 'regions': REGIONS}
    # ---- today's loop (the flag off)
    opt = torch.optim.Adam(dels, lr=lr)
    last = {}

    def autograd_epoch():
        z = model(data.x, req.e_sdf)
        neg = GU.negative_sampling(edge_index=req.edges, num_nodes=data.num_nodes, num_neg_samples=req.m)
        lg = model.decode(z, req.df_edges, neg)
        loss_r = F.mse_loss(lg[:req.m], lg[req.m:])
        loss_l = ops.pairs_sigmoid_mse(z, req.nodes32, req.target, req.n_pairs)
        loss = 0.5 * loss_r + 0.5 * loss_l
        loss.backward()
        opt.step()
        opt.zero_grad()
        last['loss'] = loss
    region(autograd_epoch, lambda: last['loss'].item(), EPOCHS)
    t_auto = [region(autograd_epoch, lambda: last['loss'].item(), EPOCHS) for _ in range(REGIONS)]
    # ---- the fused step (the flag on), from the same starting weights
    with torch.no_grad():
        for p, s in zip(dels, start):
            p.copy_(s)
    t0 = time.perf_counter()
    pos_keys = GU.positive_edge_keys(req.edges, data.num_nodes)
    eng = EdgeprobEngine(model, data.x, req.e_sdf, req.df_edges, req.nodes32, req.target, req.n_pairs, lr, (0.9, 0.999), 1e-8,
                         history=4096)
    draw = lambda: GU.negative_sampling_cached(pos_keys, data.num_nodes, req.m)
    eng.step(draw())                                  # (captures the graph)
    torch.cuda.synchronize()
    res['fused_setup_ms'] = round(1e3 * (time.perf_counter() - t0), 1)
    fused_epoch = lambda: eng.step(draw())
    region(fused_epoch, eng.last_losses, EPOCHS)
    # ---- the fused step on the device draw (--device_negatives), on a copy of the model; its regions alternate with the host leg's
    dev_model = copy.deepcopy(model)
    dev = EdgeprobEngine(dev_model, data.x, req.e_sdf, req.df_edges, req.nodes32, req.target, req.n_pairs, lr, (0.9, 0.999), 1e-8,
                         history=4096)
    dev.enable_device_negatives(pos_keys, 42)
    dev.step_device()                                 # (captures the graph)
    region(dev.step_device, dev.last_losses, EPOCHS)
    t_fused, t_dev = [], []
    for _ in range(REGIONS):
        t_fused.append(region(fused_epoch, eng.last_losses, EPOCHS))
        t_dev.append(region(dev.step_device, dev.last_losses, EPOCHS))
    # ---- where the fused epoch's time goes: the eager negative draw on its own, the eager step's stages by events
    t_draw = [region(draw, lambda: None, EPOCHS) for _ in range(REGIONS)]
    t_draw_unique = [region(lambda: GU.negative_sampling(edge_index=req.edges, num_nodes=data.num_nodes, num_neg_samples=req.m),
                            lambda: None, EPOCHS) for _ in range(REGIONS)]
    eager = EdgeprobEngine(model, data.x, req.e_sdf, req.df_edges, req.nodes32, req.target, req.n_pairs, lr, (0.9, 0.999), 1e-8,
                           use_graph=False)
    stages = []
    for k in range(2 * EPOCHS):
        neg = draw()
        eager.events = []
        eager.step(neg)
        torch.cuda.synchronize()
        ev = eager.events
        if k >= EPOCHS:
            stages.append({b[0]: a[1].elapsed_time(b[1]) for a, b in zip(ev[:-1], ev[1:])})
    ms = lambda ts: round(1e3 * float(np.median(ts)), 4)
    res['autograd_ms_per_epoch'], res['fused_ms_per_epoch'] = ms(t_auto), ms(t_fused)
    res['autograd_regions_ms'] = [round(1e3 * v, 4) for v in t_auto]
    res['fused_regions_ms'] = [round(1e3 * v, 4) for v in t_fused]
    res['ratio'] = round(res['autograd_ms_per_epoch'] / res['fused_ms_per_epoch'], 2)
    res['negative_draw_ms_per_epoch'] = ms(t_draw)
    res['negative_draw_share_of_fused_epoch'] = round(res['negative_draw_ms_per_epoch'] / res['fused_ms_per_epoch'], 3)
    res['negative_draw_with_unique_ms_per_epoch'] = ms(t_draw_unique)
    res['fused_eager_stage_ms'] = {k: round(float(np.median([s[k] for s in stages])), 4) for k in stages[0]}
    res['device_ms_per_epoch'] = ms(t_dev)
    res['device_regions_ms'] = [round(1e3 * v, 4) for v in t_dev]
    res['fused_over_device'] = round(res['fused_ms_per_epoch'] / res['device_ms_per_epoch'], 2)
    eager = EdgeprobEngine(dev_model, data.x, req.e_sdf, req.df_edges, req.nodes32, req.target, req.n_pairs, lr, (0.9, 0.999), 1e-8,
                           use_graph=False)
    eager.enable_device_negatives(pos_keys, 42)
    stages = []
    for k in range(2 * EPOCHS):
        eager.events = []
        eager.step_device()
        torch.cuda.synchronize()
        ev = eager.events
        if k >= EPOCHS:
            stages.append({b[0]: a[1].elapsed_time(b[1]) for a, b in zip(ev[:-1], ev[1:])})
    res['device_eager_stage_ms'] = {k: round(float(np.median([s[k] for s in stages])), 4) for k in stages[0]}
    res['kernel_source_stamp'] = _lib.build_stamp()[0]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--gnn', nargs='+', default=['gcn', 'gat'])
    a = ap.parse_args()
    runs = []
    for gnn in a.gnn:
        runs.append(measure(gnn))
        print(json.dumps(runs[-1]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump({'kernel_source_stamp': runs[0]['kernel_source_stamp'], 'runs': runs}, f, indent=1)
            f.write('\n')


if __name__ == '__main__':
    main()
