"""Per-epoch time of link-prediction backbone training: today's autograd loop (Trainer.train_fullbatch /
RetrainTrainer.train_fullbatch without --fused_backbone) against the fused HIP step (gnndelete_amd.backbone), in one process,
the autograd loop first.

synth-dblp and synth-collab, GCN (in -> 128 -> 64): original training (every training edge) and retrain at --df in
--df_size 5 (the retained edges only).  Every epoch draws its negatives inside the timed region, as the trainers do (the loop:
negative_sampling; the engine: negative_sampling_cached).  Per path: a warm-up region, then five regions of --epochs epochs,
each closed by the read of the last loss (the trainers' host read on a validation epoch) and timed twice - HIP events on the
stream around the region, and the host clock around the same work ending in a device synchronise; the figure is the median
region / epochs.  The stage split of the fused step comes from HIP events around the eager (uncaptured) step; the negative draw
is timed on its own.  Prints one JSON line per run and writes them all to --out as one JSON object.

    python tools/experiments/backbone_fused.py [--out profiles/backbone_fused.json] [--graphs synth-dblp synth-collab] [--gnn gcn]"""
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

REGIONS = 5


def setup(graph, gnn, request, seed=42):
    """-> (model, x, edges, n_neg, num_nodes) as train_gnn.py ('original') or delete_gnn.py --unlearning_model retrain prepare them."""
    from gnndelete_amd.framework.data import prepare_edge_deletion, resolve_df_size
    from gnndelete_amd.framework.graph_utils import to_undirected
    from gnndelete_amd.framework.models import GAT, GCN
    from gnndelete_amd.framework.synth import make_linkpred_dataset
    torch.manual_seed(seed)
    data, df = make_linkpred_dataset(graph, seed=seed)
    if request == 'retrain':
        prepare_edge_deletion(data, df['in'], resolve_df_size(5.0, data.train_pos_edge_index.shape[1]))
        edges = data.train_pos_edge_index[:, data.dr_mask]
    else:
        edges = to_undirected(data.train_pos_edge_index, num_nodes=data.num_nodes)
    model = (GCN if gnn == 'gcn' else GAT)(SimpleNamespace(in_dim=data.x.shape[1], hidden_dim=128, out_dim=64)).cuda()
    return model, data.x.cuda(), edges.cuda().contiguous(), int(edges.shape[1]), int(data.num_nodes)


def region(epoch, read, n):
    """n epochs and the closing host read -> (seconds per epoch by HIP events, by the host clock)."""
    torch.cuda.synchronize()
    first, last = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    first.record()
    for _ in range(n):
        epoch()
    read()
    last.record()
    torch.cuda.synchronize()
    return first.elapsed_time(last) * 1e-3 / n, (time.perf_counter() - t0) / n


def measure(graph, gnn, request, epochs):
    from gnndelete_amd import _lib
    from gnndelete_amd.backbone import BackboneEngine
    from gnndelete_amd.framework import graph_utils as GU
    from gnndelete_amd.framework.utils import get_link_labels
    model, x, edges, n_neg, n = setup(graph, gnn, request)
    lr = 1e-3
    start = [p.detach().clone() for p in model.parameters()]
    res = {'graph': graph, 'gnn': gnn, 'request': request, 'nodes': n, 'features': int(x.shape[1]), 'edges': int(edges.shape[1]),
           'negatives': n_neg, 'epochs_per_region': epochs, 'regions': REGIONS}
    # ---- today's loop (the flag off)
    opt = torch.optim.Adam(model.parameters(), lr=lr)
    last = {}

    def autograd_epoch():
        neg = GU.negative_sampling(edges, n, n_neg)
        z = model(x, edges)
        loss = F.binary_cross_entropy_with_logits(model.decode(z, edges, neg), get_link_labels(edges, neg))
        loss.backward()
        opt.step()
        opt.zero_grad()
        last['loss'] = loss
    region(autograd_epoch, lambda: last['loss'].item(), epochs)
    t_auto = [region(autograd_epoch, lambda: last['loss'].item(), epochs) for _ in range(REGIONS)]
    # RetrainTrainer reads the loss on every epoch
    t_auto_read = [region(lambda: (autograd_epoch(), last['loss'].item()), lambda: None, epochs) for _ in range(REGIONS)]
    # ---- the fused step (the flag on), from the same starting parameters
    with torch.no_grad():
        for p, s in zip(model.parameters(), start):
            p.copy_(s)
    t0 = time.perf_counter()
    pos_keys = GU.positive_edge_keys(edges, n)
    eng = BackboneEngine(model, x, edges, edges, n_neg, lr, (0.9, 0.999), 1e-8, history=4096)
    draw = lambda: GU.negative_sampling_cached(pos_keys, n, n_neg)
    eng.step(draw())                                  # (captures the graph)
    torch.cuda.synchronize()
    res['fused_setup_ms'] = round(1e3 * (time.perf_counter() - t0), 1)
    fused_epoch = lambda: eng.step(draw())
    region(fused_epoch, eng.last_loss, epochs)
    t_fused = [region(fused_epoch, eng.last_loss, epochs) for _ in range(REGIONS)]
    # ---- where the fused epoch's time goes: the negative draw on its own, the eager step's stages by events
    t_draw = [region(draw, lambda: None, epochs) for _ in range(REGIONS)]
    t_draw_unique = [region(lambda: GU.negative_sampling(edges, n, n_neg), lambda: None, epochs) for _ in range(REGIONS)]
    neg = draw()
    t_step = [region(lambda: eng.step(neg), eng.last_loss, epochs) for _ in range(REGIONS)]
    with torch.no_grad():
        for p, s in zip(model.parameters(), start):
            p.copy_(s)
    eager = BackboneEngine(model, x, edges, edges, n_neg, lr, (0.9, 0.999), 1e-8, use_graph=False)
    stages = []
    for k in range(2 * epochs):
        neg = draw()
        eager.events = []
        eager.step(neg)
        torch.cuda.synchronize()
        ev = eager.events
        if k >= epochs:
            stages.append({b[0]: a[1].elapsed_time(b[1]) for a, b in zip(ev[:-1], ev[1:])})
    ms = lambda ts, k: round(1e3 * float(np.median([t[k] for t in ts])), 4)
    for name, ts in (('autograd', t_auto), ('autograd_loss_read_every_epoch', t_auto_read), ('fused', t_fused),
                     ('fused_step_without_draw', t_step), ('negative_draw', t_draw), ('negative_draw_with_unique', t_draw_unique)):
        res[f'{name}_ms_per_epoch'] = ms(ts, 0)
        res[f'{name}_host_clock_ms_per_epoch'] = ms(ts, 1)
    res['autograd_regions_ms'] = [round(1e3 * v[0], 4) for v in t_auto]
    res['fused_regions_ms'] = [round(1e3 * v[0], 4) for v in t_fused]
    res['ratio'] = round(res['autograd_ms_per_epoch'] / res['fused_ms_per_epoch'], 2)
    res['ratio_host_clock'] = round(res['autograd_host_clock_ms_per_epoch'] / res['fused_host_clock_ms_per_epoch'], 2)
    res['fused_eager_stage_ms'] = {k: round(float(np.median([s[k] for s in stages])), 4) for k in stages[0]}
    res['first_product'], res['first_weight_gradient'] = eng.fwd1, eng.wgrad1
    res['final_loss_fused'] = eng.last_loss()
    res['kernel_source_stamp'] = _lib.build_stamp()[0]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--graphs', nargs='+', default=['synth-dblp', 'synth-collab'])
    ap.add_argument('--gnn', nargs='+', default=['gcn'])
    ap.add_argument('--requests', nargs='+', default=['original', 'retrain'])
    ap.add_argument('--epochs', type=int, default=30)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('backbone_fused.py measures on the GPU: none found')
    runs = []
    for graph in a.graphs:
        for gnn in a.gnn:
            for request in a.requests:
                runs.append(measure(graph, gnn, request, a.epochs))
                print(json.dumps(runs[-1]), flush=True)
                if a.out:
                    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                    with open(a.out, 'w') as f:
                        json.dump({'kernel_source_stamp': runs[0]['kernel_source_stamp'], 'runs': runs}, f, indent=1)
                        f.write('\n')


if __name__ == '__main__':
    main()
