"""Per-batch time of edge-probability GraphSAINT mini-batch unlearning (--unlearning_model gnndelete --minibatch): the
autograd loop of GNNDeleteTrainer.train_minibatch against the fused HIP batch step
(gnndelete_amd.minibatch.MinibatchEdgeprobStep), in one process.

synth-collab, GCN (in -> 128 -> 64), 5 % IN deletion, 8,192 walk roots, walk length 2, 32 batches per epoch.  One warm-up
epoch per path, then timed epochs with the two paths alternating (autograd, fused, autograd, ...); every path continues
from its own weights and optimizer state.  A batch's time runs from drawing its node set to the end of Adam (sampling
included), closed by a device synchronisation.  Prints one JSON line: the median ms per batch of both paths and of each
timed epoch (the spread over regions), the fused path's median stage split (device events) and its blocking host reads
per batch (the cut's count vector; the negatives' draw on the host is part of both paths).

    python tools/experiments/minibatch_edgeprob_fused.py [--out FILE] [--epochs K]"""
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
    from gnndelete_amd.framework.data import prepare_edge_deletion, resolve_df_size
    from gnndelete_amd.framework.models import GCNDelete
    from gnndelete_amd.framework.synth import make_linkpred_dataset
    torch.manual_seed(seed)
    data, df = make_linkpred_dataset('synth-collab', seed=seed)
    prepare_edge_deletion(data, df['in'], resolve_df_size(5.0, data.train_pos_edge_index.shape[1]))
    data.edge_index = data.train_pos_edge_index
    model = GCNDelete(SimpleNamespace(in_dim=data.x.shape[1], hidden_dim=128, out_dim=64), data.sdf_node_1hop_mask,
                      data.sdf_node_2hop_mask).cuda()
    with torch.no_grad():
        dd = data.clone().to('cuda')
        z_ori = model(dd.x, dd.train_pos_edge_index[:, dd.dr_mask])
    return data, model, z_ori


def autograd_epoch(model, z_ori, loader, opt, times):
    """The batch loop of GNNDeleteTrainer.train_minibatch, statement for statement."""
    from gnndelete_amd.framework.trainer import sampler as S
    it = iter(loader.node_sets())
    for _ in range(len(loader)):
        t0 = time.perf_counter()
        batch = loader.subgraph(next(it)).to('cuda')
        ei = batch.edge_index
        e_sdf = ei[:, batch.sdf_mask].contiguous()
        z = model(batch.x, e_sdf, batch.sdf_node_1hop_mask, batch.sdf_node_2hop_mask)
        pos = ei[:, batch.df_mask]
        k = pos.shape[1]
        neg = S.negative_sampling(ei, batch.x.shape[0], k)
        df_logits = model.decode(z, pos, neg)
        loss_e = F.mse_loss(df_logits[:k], df_logits[k:])
        lower = e_sdf[0] < e_sdf[1]
        row, col = e_sdf[0][lower], e_sdf[1][lower]
        logits_ori = (z_ori[row] * z_ori[col]).sum(-1)
        logits = (z[row] * z[col]).sum(-1)
        loss_l = F.mse_loss(logits, logits_ori)
        loss = 0.5 * loss_e + 0.5 * loss_l
        loss.backward()
        opt.step()
        opt.zero_grad()
        [loss.item(), loss_e.item(), loss_l.item()]
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)


def fused_epoch(step, loader, times, stages):
    hist = torch.zeros(len(loader), 3, device='cuda')
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
    ap.add_argument('--epochs', type=int, default=3, help='timed epochs per path')
    a = ap.parse_args()
    from gnndelete_amd.framework.models import GCNDelete
    from gnndelete_amd.framework.trainer import sampler as S
    from gnndelete_amd.minibatch import MinibatchEdgeprobStep
    data, model, z_ori = setup()
    lr = 1e-3
    loader = S.make_sampler(data, a.roots, a.batches)
    res = {'graph': 'synth-collab', 'gnn': 'gcn', 'nodes': int(data.num_nodes),
           'train_edges': int(data.train_pos_edge_index.shape[1]), 'roots': a.roots, 'walk_length': 2, 'batches': a.batches,
           'timed_epochs': a.epochs}
    # the fused path trains a copy: each path continues from its own weights
    fused_model = GCNDelete(SimpleNamespace(in_dim=data.x.shape[1], hidden_dim=128, out_dim=64), data.sdf_node_1hop_mask,
                            data.sdf_node_2hop_mask).cuda()
    fused_model.load_state_dict(model.state_dict())
    opt = torch.optim.Adam([model.deletion1.deletion_weight, model.deletion2.deletion_weight], lr=lr)
    t0 = time.perf_counter()
    step = MinibatchEdgeprobStep(fused_model, data, loader, z_ori, lr, (0.9, 0.999), 1e-8, max_nodes=3 * a.roots)
    torch.cuda.synchronize()
    res['fused_setup_ms'] = round(1e3 * (time.perf_counter() - t0), 1)
    autograd_epoch(model, z_ori, loader, opt, [])                     # warm-up, one epoch per path
    fused_epoch(step, loader, [], [])
    reads0 = step.cut.reads
    t_auto, t_fused, stages = [], [], []
    for _ in range(a.epochs):                                         # alternating regions
        ta, tf = [], []
        autograd_epoch(model, z_ori, loader, opt, ta)
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
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
