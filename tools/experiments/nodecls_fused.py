"""Per-epoch time of node-classifier training (train_node.py): today's autograd loop (NodeClassificationTrainer.train without
--fused_backbone) against the fused HIP step (gnndelete_amd.backbone.NodeClassifierEngine), in one process, the two paths
alternating region by region on two copies of the model.

synth-dblp and synth-collab node classification (make_nodecls_dataset: 4 classes), GCN and GAT, in -> 128 -> 4.  Per path: a
warm-up region, then five regions of --epochs epochs, each closed by the read of the last loss (the trainer's host read on a
validation epoch) and timed twice - HIP events on the stream around the region, and the host clock around the same work ending
in a device synchronise; the figure is the median region / epochs.  The stage split of the fused step comes from HIP events
around the eager (uncaptured) step.  Prints one JSON line per run and writes them all to --out as one JSON object.

    python tools/experiments/nodecls_fused.py [--out profiles/nodecls_fused.json] [--graphs synth-dblp synth-collab] [--gnn gcn gat]"""
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

REGIONS = 5


def setup(graph, gnn, seed=42):
    """-> (model, data on the device) as train_node.py prepares them."""
    from gnndelete_amd.framework.models import GAT, GCN
    from gnndelete_amd.framework.synth import make_nodecls_dataset
    torch.manual_seed(seed)
    data = make_nodecls_dataset(graph, seed=seed).to('cuda')
    data.edge_index = data.edge_index.contiguous()
    model = (GCN if gnn == 'gcn' else GAT)(SimpleNamespace(in_dim=data.x.shape[1], hidden_dim=128, out_dim=int(data.num_classes))).cuda()
    return model, data


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


def measure(graph, gnn, epochs):
    from gnndelete_amd import _lib
    from gnndelete_amd.backbone import NodeClassifierEngine, padded_class_width
    model, data = setup(graph, gnn)
    fused_model = copy.deepcopy(model)
    eager_model = copy.deepcopy(model)
    lr = 1e-3
    x, edges, y, mask = data.x, data.edge_index, data.y, data.train_mask
    classes = int(data.num_classes)
    res = {'graph': graph, 'gnn': gnn, 'nodes': int(data.num_nodes), 'features': int(x.shape[1]), 'edges': int(edges.shape[1]),
           'classes': classes, 'padded_width': padded_class_width(classes), 'train_rows': int(mask.sum()), 'hidden': 128,
           'epochs_per_region': epochs, 'regions': REGIONS}
    # ---- today's loop (the flag off)
    opt = torch.optim.Adam(model.parameters(), lr=lr)
    last = {}

    def autograd_epoch():
        z = F.log_softmax(model(x, edges), dim=1)
        loss = F.nll_loss(z[mask], y[mask])
        loss.backward()
        opt.step()
        opt.zero_grad()
        last['loss'] = loss
    # ---- the fused step (the flag on), from the same starting parameters
    t0 = time.perf_counter()
    eng = NodeClassifierEngine(fused_model, x, edges, y, mask, lr, (0.9, 0.999), 1e-8, history=4096)
    eng.step()                                        # (captures the graph)
    torch.cuda.synchronize()
    res['fused_setup_ms'] = round(1e3 * (time.perf_counter() - t0), 1)
    region(autograd_epoch, lambda: last['loss'].item(), epochs)
    region(eng.step, eng.last_loss, epochs)
    t_auto, t_fused = [], []
    for _ in range(REGIONS):                          # alternating: a drift of the clocks or of the machine meets both paths
        t_auto.append(region(autograd_epoch, lambda: last['loss'].item(), epochs))
        t_fused.append(region(eng.step, eng.last_loss, epochs))
    # ---- where the fused epoch's time goes: the eager step's stages by events
    eager = NodeClassifierEngine(eager_model, x, edges, y, mask, lr, (0.9, 0.999), 1e-8, use_graph=False)
    stages = []
    for k in range(2 * epochs):
        eager.events = []
        eager.step()
        torch.cuda.synchronize()
        ev = eager.events
        if k >= epochs:
            stages.append({b[0]: a[1].elapsed_time(b[1]) for a, b in zip(ev[:-1], ev[1:])})
    ms = lambda ts, k: round(1e3 * float(np.median([t[k] for t in ts])), 4)
    for name, ts in (('autograd', t_auto), ('fused', t_fused)):
        res[f'{name}_ms_per_epoch'] = ms(ts, 0)
        res[f'{name}_host_clock_ms_per_epoch'] = ms(ts, 1)
    res['autograd_regions_ms'] = [round(1e3 * v[0], 4) for v in t_auto]
    res['fused_regions_ms'] = [round(1e3 * v[0], 4) for v in t_fused]
    res['ratio'] = round(res['autograd_ms_per_epoch'] / res['fused_ms_per_epoch'], 2)
    res['ratio_host_clock'] = round(res['autograd_host_clock_ms_per_epoch'] / res['fused_host_clock_ms_per_epoch'], 2)
    res['fused_eager_stage_ms'] = {k: round(float(np.median([s[k] for s in stages])), 4) for k in stages[0]}
    res['first_product'], res['first_weight_gradient'] = eng.fwd1, eng.wgrad1
    res['final_loss_autograd'], res['final_loss_fused'] = float(last['loss']), eng.last_loss()
    res['kernel_source_stamp'] = _lib.build_stamp()[0]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--graphs', nargs='+', default=['synth-dblp', 'synth-collab'])
    ap.add_argument('--gnn', nargs='+', default=['gcn', 'gat'])
    ap.add_argument('--epochs', type=int, default=30)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('nodecls_fused.py measures on the GPU: none found')
    runs = []
    for graph in a.graphs:
        for gnn in a.gnn:
            runs.append(measure(graph, gnn, a.epochs))
            print(json.dumps(runs[-1]), flush=True)
            if a.out:
                os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                with open(a.out, 'w') as f:
                    json.dump({'kernel_source_stamp': runs[0]['kernel_source_stamp'], 'runs': runs}, f, indent=1)
                    f.write('\n')


if __name__ == '__main__':
    main()
