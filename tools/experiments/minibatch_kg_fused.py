"""Per-batch time of knowledge-graph GraphSAINT mini-batch unlearning (delete_gnn.py --gnn rgcn, the default path of
KGGNNDeleteNodeembTrainer.train): the autograd batch loop against the fused HIP batch step
(gnndelete_amd.minibatch.MinibatchKGNodeembStep, --fused_minibatch), in one process.

Requests: synth-biokg (93,773 nodes, 51 relation types) and synth-wn18 (40,943 nodes, 18 relation types), RGCNDelete
128 -> 128 -> 64, 5 % IN deletion, 64 walk roots, walk length 2, 32 batches per epoch.  One warm-up epoch per path, then timed
epochs with the two paths alternating (autograd, fused, autograd, ...); every path continues from its own weights and optimizer
state.  A batch's time runs from drawing its node set to the end of the second Adam (sampling included), closed by a device
synchronisation.  Prints one JSON line per request: the median ms per batch of both paths and of each timed epoch (the
spread over regions), the fused path's median stage split (device events: cut, typed CSR, forward, negatives, loss, backward +
Adam) and its blocking host reads per batch (the cut's count vector; negative_sampling_kg's reads are part of both paths).

    python tools/experiments/minibatch_kg_fused.py [--out FILE] [--runs synth-biokg synth-wn18] [--epochs K]"""
import argparse
import json
import os
import sys
import time
from types import SimpleNamespace

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

DF, DF_SIZE = 'in', 5.0
DIMS = (128, 128, 64)
ALPHA, LR = 0.5, 1e-3


def setup(graph, seed=42):
    from gnndelete_amd.framework.data import prepare_edge_deletion, resolve_df_size
    from gnndelete_amd.framework.models import RGCNDelete
    from gnndelete_amd.framework.synth import KG_SHAPES, make_kg_dataset
    from gnndelete_amd.framework.trainer.gnndelete_nodeemb import _non_df_masks
    from gnndelete_amd.framework.utils import seed_everything
    nr = KG_SHAPES[graph][1]
    data, df = make_kg_dataset(graph, seed=seed)
    seed_everything(seed)
    prepare_edge_deletion(data, df[DF], resolve_df_size(DF_SIZE, data.train_pos_edge_index.shape[1]), True, nr)
    _non_df_masks(data)
    i, h, o = DIMS

    def model():
        return RGCNDelete(SimpleNamespace(in_dim=i, hidden_dim=h, out_dim=o), data.num_nodes, nr, data.sdf_node_1hop_mask,
                          data.sdf_node_2hop_mask).cuda()
    return data, nr, model


def autograd_epoch(model, loader, opts, nr, times):
    """The batch loop of KGGNNDeleteNodeembTrainer.train, statement for statement."""
    from gnndelete_amd.framework.trainer.gnndelete_nodeemb import _four_terms, get_loss_fct
    from gnndelete_amd.framework.utils import negative_sampling_kg
    loss_fct = get_loss_fct('mse_mean')
    it = iter(loader.node_sets())
    for _ in range(len(loader)):
        t0 = time.perf_counter()
        batch = loader.subgraph(next(it)).to('cuda')
        edge_index = batch.edge_index[:, batch.dr_mask].contiguous()
        edge_type = batch.edge_type[batch.dr_mask].contiguous()
        m1, m2 = batch.sdf_node_1hop_mask_non_df_mask, batch.sdf_node_2hop_mask_non_df_mask
        z1, z2 = model(batch.x, edge_index, edge_type, m1, m2, return_all_emb=True)
        with torch.no_grad():
            z1_ori, z2_ori = model.get_original_embeddings(batch.x, edge_index, edge_type, return_all_emb=True)
        pos_index, pos_type = batch.edge_index[:, batch.df_mask], batch.edge_type[batch.df_mask]
        forward = pos_type < nr
        dec_index, dec_type = pos_index[:, forward], pos_type[forward]
        neg_index = negative_sampling_kg(edge_index=dec_index, edge_type=dec_type)
        r1, r2, l1, l2 = _four_terms(loss_fct, z1, z2, z1_ori, z2_ori, dec_index, neg_index, m1, m2)
        loss1 = ALPHA * r1 + (1 - ALPHA) * l1
        loss1.backward(retain_graph=True)
        opts[0].step()
        opts[0].zero_grad()
        loss2 = ALPHA * r2 + (1 - ALPHA) * l2
        loss2.backward(retain_graph=True)
        opts[1].step()
        opts[1].zero_grad()
        [(loss1 + loss2).item(), (r1 + r2).item(), (l1 + l2).item()]
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


def measure(graph, roots, batches, epochs):
    from gnndelete_amd.framework.trainer import sampler as S
    from gnndelete_amd.minibatch import MinibatchKGNodeembStep
    data, nr, make_model = setup(graph)
    model = make_model()
    fused_model = make_model()                  # the fused path trains a copy: each path continues from its own weights
    fused_model.load_state_dict(model.state_dict())
    loader = S.make_sampler(data, roots, batches)
    res = {'graph': graph, 'gnn': 'rgcn', 'dims': list(DIMS), 'nodes': int(data.num_nodes), 'typed_edges': int(data.edge_index.shape[1]),
           'relation_types': nr, 'roots': roots, 'walk_length': 2, 'batches': batches, 'timed_epochs': epochs}
    opts = [torch.optim.Adam(model.deletion1.parameters(), lr=LR), torch.optim.Adam(model.deletion2.parameters(), lr=LR)]
    t0 = time.perf_counter()
    step = MinibatchKGNodeembStep(fused_model, data, loader, nr, ALPHA, 'mean', LR, (0.9, 0.999), 1e-8, max_nodes=3 * roots)
    torch.cuda.synchronize()
    res['fused_setup_ms'] = round(1e3 * (time.perf_counter() - t0), 1)
    autograd_epoch(model, loader, opts, nr, [])                        # warm-up, one epoch per path
    fused_epoch(step, loader, [], [])
    reads0 = step.cut.reads
    t_auto, t_fused, stages = [], [], []
    for _ in range(epochs):                                            # alternating regions
        ta, tf = [], []
        autograd_epoch(model, loader, opts, nr, ta)
        fused_epoch(step, loader, tf, stages)
        t_auto.append(ta)
        t_fused.append(tf)
    ms = lambda ts: round(1e3 * float(np.median(ts)), 3)
    res['autograd_ms_per_batch'] = ms(np.concatenate(t_auto))
    res['fused_ms_per_batch'] = ms(np.concatenate(t_fused))
    res['autograd_ms_per_batch_by_epoch'] = [ms(t_) for t_ in t_auto]
    res['fused_ms_per_batch_by_epoch'] = [ms(t_) for t_ in t_fused]
    res['autograd_over_fused'] = round(res['autograd_ms_per_batch'] / res['fused_ms_per_batch'], 2)
    spread = max(res['autograd_ms_per_batch_by_epoch']) - min(res['autograd_ms_per_batch_by_epoch'])
    res['fused_below_autograd_by_more_than_its_spread'] = bool(res['autograd_ms_per_batch'] - res['fused_ms_per_batch'] > spread)
    res['fused_stage_ms'] = {k: round(float(np.median([s[k] for s in stages])), 3) for k in stages[0]}
    res['fused_host_reads_per_batch'] = (step.cut.reads - reads0) / (batches * epochs)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--runs', nargs='+', default=['synth-biokg', 'synth-wn18'])
    ap.add_argument('--roots', type=int, default=64)
    ap.add_argument('--batches', type=int, default=32)
    ap.add_argument('--epochs', type=int, default=3, help='timed epochs per path')
    a = ap.parse_args()
    lines = []
    for graph in a.runs:
        lines.append(json.dumps(measure(graph, a.roots, a.batches, a.epochs)))
        print(lines[-1], flush=True)
        if a.out:                                                      # (written after every run: a later run may take long)
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, 'w') as f:
                f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
