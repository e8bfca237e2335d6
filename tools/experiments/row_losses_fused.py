"""Per-epoch time of node-embedding unlearning with --loss_fct kld_mean / cosine_mean: today's autograd loop (the trainer's
loop without --fused_row_losses: HIP-backed model, gd_rowpair_loss_f32 per term, torch's Adam, a host read of the loss every
epoch) against the fused Del step with the folded row losses (NodeembEngine(loss_fct=...), one hipGraph replay per epoch,
the trainer's options cache_layer1 + affected_rows_only), in one process, alternating the two paths region by region.

synth-collab GCN (bench.py's request: in -> 128 -> 64, --df in --df_size 5, both_layerwise) and synth-dblp GCN / GAT.  Where
autograd refuses the layer-wise rule on a backbone (its first epoch raises: a weight stepped between the two backward passes),
both paths are measured under both_all instead; the record says which rule ran.  Both paths start
from the same Del weights with the same negatives.  Per path: warm-up epochs, then REGIONS regions of EPOCHS epochs, each
closed by a device synchronise (the autograd loop reads its loss every epoch, as the trainer does; the fused path reads the
last row of its device-side history at the end of a region, the trainer's read on a validation epoch); the figure is the
median region / EPOCHS.  Also records the largest relative difference of the two paths' losses over the first epochs, so a
ratio is never read without knowing both computed the same thing.  Needs a GPU: there is no CPU timing.

    python tools/experiments/row_losses_fused.py [--out profiles/row_losses_fused.json] [--workloads synth-collab synth-dblp]"""
import argparse
import json
import os
import sys
import time
from types import SimpleNamespace

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

EPOCHS, REGIONS, WARMUP, CHECK = 30, 5, 10, 5


class RuleRefusedByAutograd(Exception):
    pass


def setup(workload, gnn, seed=42):
    from gnndelete_amd.framework.data import prepare_edge_deletion, resolve_df_size
    from gnndelete_amd.framework.graph_utils import negative_sampling
    from gnndelete_amd.framework.models import GATDelete, GCNDelete
    from gnndelete_amd.framework.synth import make_linkpred_dataset
    from gnndelete_amd.framework.utils import seed_everything
    data, df = make_linkpred_dataset(workload, seed=seed)
    seed_everything(seed)
    prepare_edge_deletion(data, df['in'], resolve_df_size(5.0, data.train_pos_edge_index.shape[1]))
    cls = GCNDelete if gnn == 'gcn' else GATDelete
    model = cls(SimpleNamespace(in_dim=data.x.shape[1], hidden_dim=128, out_dim=64), data.sdf_node_1hop_mask, data.sdf_node_2hop_mask)
    neg = negative_sampling(data.train_pos_edge_index, data.num_nodes, int(data.df_mask.sum()))
    keep = torch.ones(data.num_nodes, dtype=torch.bool)
    keep[data.directed_df_edge_index.flatten().unique()] = False
    ni1, ni2 = (data.sdf_node_1hop_mask & keep).cuda(), (data.sdf_node_2hop_mask & keep).cuda()
    return data.to('cuda'), model.cuda(), neg.cuda(), ni1, ni2


def region(epoch, read, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        epoch()
    read()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n


def measure(workload, gnn, loss_fct, loss_type='both_layerwise', alpha=0.5, lr=1e-3):
    from gnndelete_amd import _lib
    from gnndelete_amd.engine import NodeembEngine
    from gnndelete_amd.framework.trainer.gnndelete_nodeemb import _autograd_update, _four_terms, get_loss_fct
    data, model, neg, ni1, ni2 = setup(workload, gnn)
    E = data.train_pos_edge_index
    e_dr, e_sdf, pos = E[:, data.dr_mask].contiguous(), E[:, data.sdf_mask].contiguous(), E[:, data.df_mask]
    with torch.no_grad():
        z1o, z2o = model.get_original_embeddings(data.x, e_dr, return_all_emb=True)
    dels = [model.deletion1.deletion_weight, model.deletion2.deletion_weight]
    start = [p.detach().clone() for p in dels]
    res = {'graph': workload, 'gnn': gnn, 'loss_fct': loss_fct, 'loss_type': loss_type, 'df': 'in', 'df_size': 5.0,
           'nodes': int(data.num_nodes), 'sdf_edges': int(e_sdf.shape[1]), 'df_edges': int(pos.shape[1]),
           's1_nodes': int(data.sdf_node_1hop_mask.sum()), 's2_nodes': int(data.sdf_node_2hop_mask.sum()),
           'epochs_per_region': EPOCHS, 'regions': REGIONS}
    # ---- today's loop (the flag off)
    fct = get_loss_fct(loss_fct)
    opt = [torch.optim.Adam([dels[0]], lr=lr), torch.optim.Adam([dels[1]], lr=lr)]
    last, auto_log = {}, []

    def autograd_epoch():
        z1, z2 = model(data.x, e_sdf, return_all_emb=True)
        r1, r2, l1, l2 = _four_terms(fct, z1, z2, z1o, z2o, pos, neg, ni1, ni2)
        loss, loss_r, loss_l = _autograd_update(loss_type, alpha, r1, r2, l1, l2, opt)
        last['loss'] = loss.item()                           # (the trainer's per-epoch host read)
    for k in range(CHECK):
        try:
            autograd_epoch()
        except RuntimeError as e:
            if k == 0 and 'inplace' in str(e).replace('-', ''):
                raise RuleRefusedByAutograd(str(e).splitlines()[0]) from None
            raise
        auto_log.append(last['loss'])
    for _ in range(WARMUP):
        autograd_epoch()
    # ---- the fused step (the flag on), from the same starting weights
    fmodel = type(model)(SimpleNamespace(in_dim=data.x.shape[1], hidden_dim=128, out_dim=64), data.sdf_node_1hop_mask,
                         data.sdf_node_2hop_mask).cuda()
    fmodel.load_state_dict(model.state_dict())
    with torch.no_grad():
        fmodel.deletion1.deletion_weight.copy_(start[0])
        fmodel.deletion2.deletion_weight.copy_(start[1])
    t0 = time.perf_counter()
    eng = NodeembEngine(fmodel, data.x, e_sdf, z1o, z2o, pos, neg, ni1, ni2, loss_type=loss_type, alpha=alpha, lr=lr,
                        loss_fct=loss_fct, cache_layer1=True, affected_rows_only=True)
    eng.step()                                                # (captures the graph)
    torch.cuda.synchronize()
    res['fused_setup_ms'] = round(1e3 * (time.perf_counter() - t0), 1)
    for _ in range(CHECK - 1):
        eng.step()
    fused_log = eng.loss_history()[:CHECK, 0].tolist()
    res['first_epochs_largest_relative_loss_difference'] = float(np.max(np.abs(np.array(fused_log) - np.array(auto_log))
                                                                        / np.abs(np.array(auto_log))))
    for _ in range(WARMUP):
        eng.step()
    read_fused = lambda: eng.loss_history()[-1]
    t_auto, t_fused = [], []
    for _ in range(REGIONS):                                  # alternating: both paths see the same machine state
        t_auto.append(region(autograd_epoch, lambda: None, EPOCHS))
        t_fused.append(region(eng.step, read_fused, EPOCHS))
    ms = lambda ts: round(1e3 * float(np.median(ts)), 4)
    res['autograd_ms_per_epoch'], res['fused_ms_per_epoch'] = ms(t_auto), ms(t_fused)
    res['autograd_regions_ms'] = [round(1e3 * v, 4) for v in t_auto]
    res['fused_regions_ms'] = [round(1e3 * v, 4) for v in t_fused]
    res['ratio'] = round(res['autograd_ms_per_epoch'] / res['fused_ms_per_epoch'], 2)
    res['fused_tail_launch'] = bool(eng._tail)
    res['kernel_source_stamp'] = _lib.build_stamp()[0]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--workloads', nargs='+', default=['synth-collab', 'synth-dblp'])
    ap.add_argument('--losses', nargs='+', default=['kld_mean', 'cosine_mean'])
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('row_losses_fused.py measures on the GPU: none found (there is no CPU timing)')
    runs = []
    for workload in a.workloads:
        for gnn in (['gcn'] if workload == 'synth-collab' else ['gcn', 'gat']):
            for loss_fct in a.losses:
                try:
                    runs.append(measure(workload, gnn, loss_fct, 'both_layerwise'))
                except RuleRefusedByAutograd as e:
                    runs.append(dict(measure(workload, gnn, loss_fct, 'both_all'), both_layerwise_refused_by_autograd=str(e)))
                print(json.dumps(runs[-1]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump({'kernel_source_stamp': runs[0]['kernel_source_stamp'], 'runs': runs}, f, indent=1)
            f.write('\n')


if __name__ == '__main__':
    main()
