"""Per-epoch time of link-prediction backbone training: today's autograd loop (Trainer.train_fullbatch /
RetrainTrainer.train_fullbatch without --fused_backbone) against the fused HIP step (gnndelete_amd.backbone) on the host draw
and on the device draw (--device_negatives: step_device, the draw and the incidence merge inside the timed region), in one
process on three copies of the model, the three legs' regions alternating.  --parent_records embeds the fused legs of records
the PARENT commit's script wrote on the same box: the device leg is to be compared with those, not with this tree's host leg alone.

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
    # ---- three legs on three copies of the model, from the same starting parameters: today's loop (the flag off), the fused
    # step on the host draw (--fused_backbone), the fused step on the device draw (--fused_backbone --device_negatives)
    import copy
    auto_model, dev_model = copy.deepcopy(model), copy.deepcopy(model)
    opt = torch.optim.Adam(auto_model.parameters(), lr=lr)
    last = {}

    def autograd_epoch():
        neg = GU.negative_sampling(edges, n, n_neg)
        z = auto_model(x, edges)
        loss = F.binary_cross_entropy_with_logits(auto_model.decode(z, edges, neg), get_link_labels(edges, neg))
        loss.backward()
        opt.step()
        opt.zero_grad()
        last['loss'] = loss
    t0 = time.perf_counter()
    pos_keys = GU.positive_edge_keys(edges, n)
    eng = BackboneEngine(model, x, edges, edges, n_neg, lr, (0.9, 0.999), 1e-8, history=4096)
    draw = lambda: GU.negative_sampling_cached(pos_keys, n, n_neg)
    eng.step(draw())                                  # (captures the graph)
    torch.cuda.synchronize()
    res['fused_setup_ms'] = round(1e3 * (time.perf_counter() - t0), 1)
    fused_epoch = lambda: eng.step(draw())
    t0 = time.perf_counter()
    dev = BackboneEngine(dev_model, x, edges, edges, n_neg, lr, (0.9, 0.999), 1e-8, history=4096)
    dev.enable_device_negatives(GU.positive_edge_keys(edges, n), 42)
    dev.step_device()                                 # (captures the graph)
    torch.cuda.synchronize()
    res['device_setup_ms'] = round(1e3 * (time.perf_counter() - t0), 1)
    legs = (('autograd', autograd_epoch, lambda: last['loss'].item()), ('fused', fused_epoch, eng.last_loss),
            ('device', dev.step_device, dev.last_loss))
    times = {name: [] for name, _, _ in legs}
    for name, epoch, read in legs:                    # warm-up regions
        region(epoch, read, epochs)
    for _ in range(REGIONS):                          # the legs alternate: a drift of the box meets all three alike
        for name, epoch, read in legs:
            times[name].append(region(epoch, read, epochs))
    t_auto, t_fused, t_dev = times['autograd'], times['fused'], times['device']
    # RetrainTrainer reads the loss on every epoch
    t_auto_read = [region(lambda: (autograd_epoch(), last['loss'].item()), lambda: None, epochs) for _ in range(REGIONS)]
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
    # the device leg: its regions, and the eager step's stages with the draw and the incidence merge inside
    res['device_ms_per_epoch'], res['device_host_clock_ms_per_epoch'] = ms(t_dev, 0), ms(t_dev, 1)
    res['device_regions_ms'] = [round(1e3 * v[0], 4) for v in t_dev]
    res['fused_over_device'] = round(res['fused_ms_per_epoch'] / res['device_ms_per_epoch'], 2)
    with torch.no_grad():
        for p, s in zip(dev_model.parameters(), start):
            p.copy_(s)
    eager = BackboneEngine(dev_model, x, edges, edges, n_neg, lr, (0.9, 0.999), 1e-8, use_graph=False)
    eager.enable_device_negatives(pos_keys, 42)
    stages = []
    for k in range(2 * epochs):
        eager.events = []
        eager.step_device()
        torch.cuda.synchronize()
        ev = eager.events
        if k >= epochs:
            stages.append({b[0]: a[1].elapsed_time(b[1]) for a, b in zip(ev[:-1], ev[1:])})
    res['device_eager_stage_ms'] = {k: round(float(np.median([s[k] for s in stages])), 4) for k in stages[0]}
    res['final_loss_device'] = dev.last_loss()
    res['first_product'], res['first_weight_gradient'] = eng.fwd1, eng.wgrad1
    res['final_loss_fused'] = eng.last_loss()
    res['kernel_source_stamp'] = _lib.build_stamp()[0]
    return res


def parent_legs(paths):
    """The fused legs of the parent commit's records (one list entry per record and run)."""
    out = []
    for path in paths:
        with open(path) as f:
            rec = json.load(f)
        for run in rec['runs']:
            out.append({'record': os.path.basename(path), 'kernel_source_stamp': rec['kernel_source_stamp'],
                        **{k: run[k] for k in ('graph', 'gnn', 'request', 'fused_ms_per_epoch', 'fused_host_clock_ms_per_epoch',
                                               'fused_regions_ms', 'fused_eager_stage_ms', 'negative_draw_ms_per_epoch')}})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--graphs', nargs='+', default=['synth-dblp', 'synth-collab'])
    ap.add_argument('--gnn', nargs='+', default=['gcn'])
    ap.add_argument('--requests', nargs='+', default=['original', 'retrain'])
    ap.add_argument('--epochs', type=int, default=30)
    ap.add_argument('--parent_records', nargs='*', default=[],
                    help='records this script wrote at the PARENT commit on the same box: their fused legs go into --out as "parent"')
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
                        json.dump({'kernel_source_stamp': runs[0]['kernel_source_stamp'], 'runs': runs,
                                   **({'parent': parent_legs(a.parent_records)} if a.parent_records else {})}, f, indent=1)
                        f.write('\n')


if __name__ == '__main__':
    main()
