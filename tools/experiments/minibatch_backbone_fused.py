"""Per-batch time of the original model's GraphSAINT mini-batch training (train_gnn.py --minibatch): the autograd loop of
Trainer.train_minibatch against the fused HIP batch step (gnndelete_amd.minibatch.MinibatchBackboneStep), in one process.

synth-collab, GCN and GAT (in -> 128 -> 64), 8,192 walk roots, walk length 2, 32 batches per epoch.  One warm-up epoch per
path, then timed epochs with the two paths alternating (autograd, fused, autograd, ...); every path continues from its own
weights and optimizer state.  A batch's time runs from drawing its node set to the end of Adam (sampling and the negatives'
draw included), closed by a device synchronisation.  Prints one JSON line: per backbone the median ms per batch of both
paths and of each timed epoch (the spread over regions), the fused path's median stage split (device events) and its
blocking host reads per batch (the cut's count vector; the negatives' draw on the host is part of both paths).

    python tools/experiments/minibatch_backbone_fused.py [--out FILE] [--epochs K]"""
import argparse
import json
import os
import sys
import time
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))


def setup(seed=42):
    from gnndelete_amd.framework.graph_utils import to_undirected
    from gnndelete_amd.framework.synth import make_linkpred_dataset
    torch.manual_seed(seed)
    data, _ = make_linkpred_dataset('synth-collab', seed=seed)
    data.train_pos_edge_index = to_undirected(data.train_pos_edge_index, num_nodes=data.num_nodes)    # as train_gnn.py
    data.edge_index = data.train_pos_edge_index
    return data


def make_model(gnn, in_dim):
    from gnndelete_amd.framework import models as M
    return {'gcn': M.GCN, 'gat': M.GAT}[gnn](SimpleNamespace(in_dim=in_dim, hidden_dim=128, out_dim=64)).cuda()


def autograd_epoch(model, loader, opt, times):
    """The batch loop of Trainer.train_minibatch, statement for statement."""
    from gnndelete_amd.framework.trainer import sampler as S
    from gnndelete_amd.framework.utils import get_link_labels
    it = iter(loader.node_sets())
    for _ in range(len(loader)):
        t0 = time.perf_counter()
        batch = loader.subgraph(next(it))
        edges = batch.edge_index.to('cuda').contiguous()
        z = model(batch.x.to('cuda'), edges)
        neg = S.negative_sampling(edges, z.size(0), edges.shape[1])
        loss = F.binary_cross_entropy_with_logits(model.decode(z, edges, neg), get_link_labels(edges, neg))
        loss.backward()
        opt.step()
        opt.zero_grad()
        loss.item()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)


def fused_epoch(step, loader, times, stages):
    hist = torch.zeros(len(loader), device='cuda')
    it = iter(loader.node_sets())
    for i in range(len(loader)):
        t0 = time.perf_counter()
        step.events = []
        step.step(next(it), hist[i:i + 1])
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
        ev = step.events
        stages.append({b[0]: a[1].elapsed_time(b[1]) for a, b in zip(ev[:-1], ev[1:])})
    hist.tolist()


def measure(gnn, data, loader, a):
    from gnndelete_amd.minibatch import MinibatchBackboneStep
    lr = 1e-3
    model = make_model(gnn, data.x.shape[1])
    fused_model = make_model(gnn, data.x.shape[1])                    # the fused path trains a copy
    fused_model.load_state_dict(model.state_dict())
    opt = torch.optim.Adam(model.parameters(), lr=lr)
    res = {}
    t0 = time.perf_counter()
    step = MinibatchBackboneStep(fused_model, data, loader, lr, (0.9, 0.999), 1e-8, max_nodes=3 * a.roots)
    torch.cuda.synchronize()
    res['fused_setup_ms'] = round(1e3 * (time.perf_counter() - t0), 1)
    autograd_epoch(model, loader, opt, [])                            # warm-up, one epoch per path
    fused_epoch(step, loader, [], [])
    reads0 = step.cut.reads
    t_auto, t_fused, stages = [], [], []
    for _ in range(a.epochs):                                         # alternating regions
        ta, tf = [], []
        autograd_epoch(model, loader, opt, ta)
        fused_epoch(step, loader, tf, stages)
        t_auto.append(ta)
        t_fused.append(tf)
    ms = lambda ts: round(1e3 * float(np.median(ts)), 3)
    res['autograd_ms_per_batch'] = ms(np.concatenate(t_auto))
    res['fused_ms_per_batch'] = ms(np.concatenate(t_fused))
    res['autograd_ms_per_batch_by_epoch'] = [ms(t_) for t_ in t_auto]
    res['fused_ms_per_batch_by_epoch'] = [ms(t_) for t_ in t_fused]
    res['speedup'] = round(res['autograd_ms_per_batch'] / res['fused_ms_per_batch'], 2)
    res['fused_stage_ms'] = {k: round(float(np.median([s[k] for s in stages])), 3) for k in stages[0]}
    res['fused_host_reads_per_batch'] = (step.cut.reads - reads0) / (a.batches * a.epochs)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--roots', type=int, default=8192)
    ap.add_argument('--batches', type=int, default=32)
    ap.add_argument('--epochs', type=int, default=3, help='timed epochs per path')
    a = ap.parse_args()
    from gnndelete_amd.framework.trainer import sampler as S
    data = setup()
    loader = S.make_sampler(data, a.roots, a.batches)
    res = {'graph': 'synth-collab', 'nodes': int(data.num_nodes), 'train_edges': int(data.train_pos_edge_index.shape[1]),
           'widths': [int(data.x.shape[1]), 128, 64], 'roots': a.roots, 'walk_length': 2, 'batches': a.batches,
           'timed_epochs': a.epochs}
    for gnn in ('gcn', 'gat'):
        res[gnn] = measure(gnn, data, loader, a)
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
