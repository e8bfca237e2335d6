"""Per-batch time of GraphSAINT mini-batch unlearning: the autograd loop (framework.trainer.sampler.train_minibatch)
against the fused HIP batch step (gnndelete_amd.minibatch), in one process.

synth-collab, GCN (in -> 128 -> 64), 5 % IN deletion, 8,192 walk roots, walk length 2, 32 batches per epoch.  Each path
runs one warm-up epoch, then one timed epoch; a batch's time runs from drawing its node set to the end of its Adam
updates (sampling included), closed by a device synchronisation.  Prints one JSON line: the median ms per batch of both
paths, the fused path's median stage split (CUDA events) and its blocking host reads per batch.

    python tools/experiments/minibatch_fused.py [--out FILE]"""
import argparse
import json
import os
import sys
import time
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))


def setup(seed=42):
    from gnndelete_amd.framework.data import prepare_edge_deletion, resolve_df_size
    from gnndelete_amd.framework.models import GCNDelete
    from gnndelete_amd.framework.synth import make_linkpred_dataset
    from gnndelete_amd.framework.trainer.gnndelete_nodeemb import _non_df_masks
    torch.manual_seed(seed)
    data, df = make_linkpred_dataset('synth-collab', seed=seed)
    prepare_edge_deletion(data, df['in'], resolve_df_size(5.0, data.train_pos_edge_index.shape[1]))
    _non_df_masks(data)
    data.edge_index = data.train_pos_edge_index
    model = GCNDelete(SimpleNamespace(in_dim=data.x.shape[1], hidden_dim=128, out_dim=64), data.sdf_node_1hop_mask,
                      data.sdf_node_2hop_mask).cuda()
    return data, model


def autograd_epoch(model, data, loader, opt, alpha, times):
    from gnndelete_amd.framework.trainer import sampler as S
    from gnndelete_amd.framework.trainer.gnndelete_nodeemb import _four_terms
    loss_fct = nn.MSELoss()
    it = iter(loader.node_sets())
    for _ in range(len(loader)):
        t0 = time.perf_counter()
        batch = loader.subgraph(next(it)).to('cuda')
        with torch.no_grad():
            z1_ori, z2_ori = model.get_original_embeddings(batch.x, batch.edge_index, return_all_emb=True)
        z1, z2 = model(batch.x, batch.edge_index[:, batch.sdf_mask].contiguous(), batch.sdf_node_1hop_mask,
                       batch.sdf_node_2hop_mask, return_all_emb=True)
        pos_edge = batch.edge_index[:, batch.df_mask]
        neg_edge = S.negative_sampling(batch.edge_index, batch.x.shape[0], pos_edge.shape[1])
        r1, r2, l1, l2 = _four_terms(loss_fct, z1, z2, z1_ori, z2_ori, pos_edge, neg_edge,
                                     batch.sdf_node_1hop_mask_non_df_mask, batch.sdf_node_2hop_mask_non_df_mask)
        loss1 = alpha * r1 + (1 - alpha) * l1
        loss1.backward(retain_graph=True)
        opt[0].step()
        opt[0].zero_grad()
        loss2 = alpha * r2 + (1 - alpha) * l2
        loss2.backward(retain_graph=True)
        opt[1].step()
        opt[1].zero_grad()
        [(loss1 + loss2).item(), (l1 + l2).item(), (r1 + r2).item()]
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)


def fused_epoch(step, loader, times, stages):
    hist = torch.zeros(len(loader), 4, device='cuda')
    it = iter(loader.node_sets())
    for i in range(len(loader)):
        t0 = time.perf_counter()
        step.events = []
        step.step(next(it), hist[i])
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
        ev = step.events
        stages.append({b[0]: a[1].elapsed_time(b[1]) for a, b in zip(ev[:-1], ev[1:])})
    hist.tolist()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--roots', type=int, default=8192)
    ap.add_argument('--batches', type=int, default=32)
    a = ap.parse_args()
    from gnndelete_amd.framework.trainer import sampler as S
    from gnndelete_amd.minibatch import MinibatchNodeembStep
    data, model = setup()
    alpha, lr = 0.5, 1e-3
    loader = S.make_sampler(data, a.roots, a.batches)
    res = {'graph': 'synth-collab', 'gnn': 'gcn', 'nodes': int(data.num_nodes),
           'train_edges': int(data.train_pos_edge_index.shape[1]), 'roots': a.roots, 'walk_length': 2, 'batches': a.batches}
    # autograd loop
    w1, w2 = model.deletion1.deletion_weight.detach().clone(), model.deletion2.deletion_weight.detach().clone()
    opt = [torch.optim.Adam(model.deletion1.parameters(), lr=lr), torch.optim.Adam(model.deletion2.parameters(), lr=lr)]
    t_auto = []
    autograd_epoch(model, data, loader, opt, alpha, [])
    autograd_epoch(model, data, loader, opt, alpha, t_auto)
    # fused step, from the same starting weights
    with torch.no_grad():
        model.deletion1.deletion_weight.copy_(w1)
        model.deletion2.deletion_weight.copy_(w2)
    model.deletion1.deletion_weight.grad = model.deletion2.deletion_weight.grad = None
    t0 = time.perf_counter()
    step = MinibatchNodeembStep(model, data, loader, alpha, lr, (0.9, 0.999), 1e-8, max_nodes=3 * a.roots)
    torch.cuda.synchronize()
    res['fused_setup_ms'] = round(1e3 * (time.perf_counter() - t0), 1)
    t_fused, stages = [], []
    fused_epoch(step, loader, [], [])
    reads0 = step.cut.reads
    fused_epoch(step, loader, t_fused, stages)
    res['autograd_ms_per_batch'] = round(1e3 * float(np.median(t_auto)), 3)
    res['fused_ms_per_batch'] = round(1e3 * float(np.median(t_fused)), 3)
    res['speedup'] = round(res['autograd_ms_per_batch'] / res['fused_ms_per_batch'], 2)
    res['fused_stage_ms'] = {k: round(float(np.median([s[k] for s in stages])), 3) for k in stages[0]}
    res['fused_host_reads_per_batch'] = (step.cut.reads - reads0) / a.batches
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
