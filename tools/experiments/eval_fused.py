"""One validation (Trainer.eval(model, data, 'val')) of an edge-unlearning request on today's torch path - the batched
[500, 2|Df|] sort of framework/metrics.py - against --fused_eval (gnndelete_amd/rankeval.py: one sort of the Dr scores and a
bitmap pass per subset on the HIP rank kernels), in one process, regions alternating.

synth-dblp (--df out --df_size 2.5) and synth-collab (--df in --df_size 5), GCN in -> 128 -> 64, --unlearning_model
gnndelete_nodeemb with its defaults (mse_mean, both_layerwise).  The request first trains for 300 epochs with a validation
every 100 on the torch path, as delete_gnn.py would: the trainer's own train_time of the blocks after the first (which holds
the graph capture) is the per-epoch time, so the share of validation in a default run (valid_freq 100) can be stated.  Then,
on that trained model: two warm-up validations per path, and seven regions per path of three validations each, torch and
fused taking turns; a region is closed by the values the validation returns (host floats: the device has finished).  Per path
the median and the spread (min, max) of a region / 3, and torch.cuda.max_memory_allocated over a region (the peak is reset
before each) next to what was allocated before it.  The ranking alone - the scores already decoded - is timed the same way
(ten calls per region), the values of the two paths are compared, and Trainer.eval's own steps are timed one by one with the
device synchronised after each (validation_steps_ms: where a validation's time goes).  The backbone keeps its seeded initial
weights (no original checkpoint is loaded): the times do not depend on them.  Prints one JSON line per graph and writes them
all to --out as one JSON object.

    python tools/experiments/eval_fused.py [--out FILE] [--graphs synth-dblp synth-collab]"""
import argparse
import json
import os
import sys
import tempfile
import time
from types import SimpleNamespace

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

REQUESTS = {'synth-dblp': ('out', 2.5), 'synth-collab': ('in', 5.0)}
TRAIN_EPOCHS, VALID_FREQ = 300, 100
WARMUP, REGIONS, EVALS, RANKS = 2, 7, 3, 10


def setup(graph, ckpt, seed=42):
    from gnndelete_amd.framework import get_model, get_trainer
    from gnndelete_amd.framework.data import prepare_edge_deletion, resolve_df_size
    from gnndelete_amd.framework.synth import make_linkpred_dataset
    kind, pct = REQUESTS[graph]
    torch.manual_seed(seed)
    data, df = make_linkpred_dataset(graph, seed=seed)
    prepare_edge_deletion(data, df[kind], resolve_df_size(pct, data.train_pos_edge_index.shape[1]))
    args = SimpleNamespace(unlearning_model='gnndelete_nodeemb', gnn='gcn', dataset=graph, checkpoint_dir=ckpt, eval_on_cpu=False,
                           in_dim=int(data.x.shape[1]), hidden_dim=128, out_dim=64, epochs=TRAIN_EPOCHS, valid_freq=VALID_FREQ, lr=1e-3,
                           loss_fct='mse_mean', loss_type='both_layerwise', alpha=0.5, random_seed=seed, fused_eval=False)
    model = get_model(args, data.sdf_node_1hop_mask, data.sdf_node_2hop_mask).cuda()
    opt = [torch.optim.Adam(model.deletion1.parameters(), lr=args.lr), torch.optim.Adam(model.deletion2.parameters(), lr=args.lr)]
    return args, data, model, opt, get_trainer(args)


def region(fn, n):
    """(seconds per call, peak bytes over the region, bytes allocated before it); fn returns host values."""
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n, torch.cuda.max_memory_allocated(), before


def alternate(torch_fn, fused_fn, n):
    for _ in range(WARMUP):
        torch_fn()
        fused_fn()
    legs = {'torch': [], 'fused': []}
    for _ in range(REGIONS):
        legs['torch'].append(region(torch_fn, n))
        legs['fused'].append(region(fused_fn, n))
    out = {}
    for name, rs in legs.items():
        ts = [1e3 * r[0] for r in rs]
        out[name] = {'median_ms': round(float(np.median(ts)), 4), 'min_ms': round(min(ts), 4), 'max_ms': round(max(ts), 4),
                     'spread_ms': round(max(ts) - min(ts), 4), 'regions_ms': [round(t, 4) for t in ts],
                     'peak_allocated_mb': round(max(r[1] for r in rs) / 2 ** 20, 1),
                     'allocated_before_mb': round(max(r[2] for r in rs) / 2 ** 20, 1)}
    out['torch_over_fused'] = round(out['torch']['median_ms'] / out['fused']['median_ms'], 2)
    # the issue's rule for claiming a benefit: the fused median below the torch median by more than the torch path's own spread
    out['fused_below_torch_by_more_than_torch_spread'] = bool(out['torch']['median_ms'] - out['fused']['median_ms'] > out['torch']['spread_ms'])
    return out


@torch.no_grad()
def stage_times(tr, model, data, reps=5):
    """Where one validation's time goes: Trainer.eval's own steps one by one, the device synchronised after each (host clock),
    with the ranking of both paths; median of `reps` passes after one warm-up pass, in ms."""
    import torch.nn.functional as F
    from gnndelete_amd.framework.metrics import batched_average_precision, batched_roc_auc
    from gnndelete_amd.rankeval import subset_auc_ap
    model.eval()
    pos, neg = data.val_pos_edge_index, data.val_neg_edge_index
    n_pos, idx, s = pos.shape[1], tr._df_subset_index, {}

    def df_rank_torch():
        k = len(s['df_list'])
        scores = torch.cat([s['df_t'][None].expand(idx.shape[0], k), s['dr'][idx]], dim=1)
        labels = torch.cat([torch.zeros(k), torch.ones(k)]).to(s['dr'].device)
        return float(batched_roc_auc(scores, labels).mean()), float(batched_average_precision(scores, labels).mean())

    def df_rank_fused():
        auc, ap = subset_auc_ap(s['df'], s['dr'], idx)
        return float(auc.mean()), float(ap.mean())
    steps = [
        ('message_passing_edges', lambda: s.update(e=tr._message_passing_edges(data))),
        ('forward', lambda: s.update(z=model(data.x, s['e']))),
        ('decode_stage_edges', lambda: s.update(lg=model.decode(s['z'], pos, neg).sigmoid(), y=tr.get_link_labels(pos, neg))),
        ('loss', lambda: F.binary_cross_entropy_with_logits(s['lg'], s['y']).cpu().item()),
        ('dt_rank_torch', lambda: (float(batched_roc_auc(s['lg'], s['y'])[0]), float(batched_average_precision(s['lg'], s['y'])[0]))),
        ('dt_rank_fused', lambda: [float(v[0]) for v in subset_auc_ap(s['lg'][n_pos:], s['lg'][:n_pos],
                                                                       torch.arange(n_pos, device=s['lg'].device)[None])]),
        ('df_decode', lambda: s.update(df=model.decode(s['z'], data.directed_df_edge_index).sigmoid())),
        ('df_tolist', lambda: s.update(df_list=s['df'].tolist())),
        ('dr_select_decode', lambda: s.update(dr=model.decode(s['z'], data.train_pos_edge_index[:, data.dr_mask]).sigmoid())),
        ('df_tensor_from_list_torch_only', lambda: s.update(df_t=torch.tensor(s['df_list'], dtype=s['dr'].dtype, device=s['dr'].device))),
        ('df_rank_torch', df_rank_torch),
        ('df_rank_fused', df_rank_fused),
        ('df_logit_mean_std', lambda: (np.mean(s['df_list']), np.std(s['df_list']))),
    ]
    times = {name: [] for name, _ in steps}
    for rep in range(reps + 1):
        for name, fn in steps:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if rep:
                times[name].append(1e3 * (time.perf_counter() - t0))
    return {name: round(float(np.median(ts)), 4) for name, ts in times.items()}


def measure(graph):
    from gnndelete_amd import _lib
    from gnndelete_amd.framework.metrics import batched_average_precision, batched_roc_auc
    from gnndelete_amd.rankeval import subset_auc_ap
    with tempfile.TemporaryDirectory() as ckpt:
        args, data, model, opt, tr = setup(graph, ckpt)
        tr.train(model, data, opt, args, None, None, None)
        blocks = [r['train_time'] for r in tr.trainer_log['log'] if 'train_time' in r]
        data = data.to('cuda')
        res = {'graph': graph, 'gnn': 'gcn', 'df': REQUESTS[graph][0], 'df_size': REQUESTS[graph][1], 'nodes': int(data.num_nodes),
               'dr_edges': int(data.dr_mask.sum()), 'df_edges': int(data.directed_df_edge_index.shape[1]),
               'val_pos_edges': int(data.val_pos_edge_index.shape[1]), 'val_neg_edges': int(data.val_neg_edge_index.shape[1]),
               'subsets': len(tr.df_pos_edge), 'evals_per_region': EVALS, 'regions': REGIONS, 'train_epochs': TRAIN_EPOCHS,
               'train_blocks_ms_per_epoch': [round(1e3 * b, 4) for b in blocks]}
        res['epoch_ms'] = round(1e3 * float(np.median(blocks[1:])), 4)
        last = {}

        def validate(fused):
            tr.args.fused_eval = fused
            last[fused] = tr.eval(model, data, 'val')
        res['validation'] = alternate(lambda: validate(False), lambda: validate(True), EVALS)
        res['eval_path'] = tr.trainer_log.get('eval_path')
        a, b = last[False], last[True]
        res['values'] = {'torch': {'loss': a[0], 'dt_auc': a[1], 'dt_aup': a[2], 'df_auc': a[3], 'df_aup': a[4]},
                         'fused': {'loss': b[0], 'dt_auc': b[1], 'dt_aup': b[2], 'df_auc': b[3], 'df_aup': b[4]}}
        res['auc_equal'] = bool(a[1] == b[1] and a[3] == b[3] and a[0] == b[0] and a[5] == b[5])
        res['aup_max_abs_diff'] = max(abs(a[2] - b[2]), abs(a[4] - b[4]))
        # what validation costs a default run: one validation per VALID_FREQ epochs
        for name in ('torch', 'fused'):
            v = res['validation'][name]['median_ms']
            res['validation'][name]['share_of_run_at_valid_freq_100'] = round(v / (v + VALID_FREQ * res['epoch_ms']), 4)
            res['validation'][name]['epochs_per_validation'] = round(v / res['epoch_ms'], 1)
        # the ranking alone, on the scores of the trained model
        with torch.no_grad():
            z = model(data.x, tr._message_passing_edges(data))
            df_score = model.decode(z, data.directed_df_edge_index).sigmoid()
            dr_score = model.decode(z, data.train_pos_edge_index[:, data.dr_mask]).sigmoid()
        idx, k = tr._df_subset_index, df_score.numel()

        def rank_torch():
            scores = torch.cat([df_score[None].expand(idx.shape[0], k), dr_score[idx]], dim=1)
            labels = torch.cat([torch.zeros(k), torch.ones(k)]).to(dr_score.device)
            return float(batched_roc_auc(scores, labels).mean()), float(batched_average_precision(scores, labels).mean())

        def rank_fused():
            auc, ap = subset_auc_ap(df_score, dr_score, idx)
            return float(auc.mean()), float(ap.mean())
        res['df_ranking_only'] = alternate(rank_torch, rank_fused, RANKS)
        res['validation_steps_ms'] = stage_times(tr, model, data)
        res['kernel_source_stamp'] = _lib.build_stamp()[0]
    return res


def ranking_only(calls=6):
    """The Df ranking at the synth-collab request's sizes on seeded scores, `calls` times: what a kernel trace is taken of
    (rocprofv3 --kernel-trace --stats -- python tools/experiments/eval_fused.py --ranking_only; profiles/eval_fused_kernel_stats.txt)."""
    from gnndelete_amd.rankeval import subset_auc_ap
    g = torch.Generator(device='cuda').manual_seed(1)
    m, k, n_sub = 2016182, 53057, 500
    ref = torch.rand(k, generator=g, device='cuda').mul(0.2).add(0.4).sigmoid()
    pool = torch.rand(m, generator=g, device='cuda').mul(0.3).add(0.4).sigmoid()
    idx = torch.stack([torch.randperm(m, generator=g, device='cuda')[:k] for _ in range(n_sub)])
    torch.cuda.synchronize()
    for _ in range(calls):
        auc, ap = subset_auc_ap(ref, pool, idx)
        print(float(auc.mean()), float(ap.mean()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--graphs', nargs='+', default=list(REQUESTS))
    ap.add_argument('--ranking_only', action='store_true', help='only the Df ranking at collab size on seeded scores (for a kernel trace)')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('eval_fused.py measures on the GPU: no device found')
    if a.ranking_only:
        return ranking_only()
    runs = []
    for graph in a.graphs:
        runs.append(measure(graph))
        print(json.dumps(runs[-1]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump({'kernel_source_stamp': runs[0]['kernel_source_stamp'], 'runs': runs}, f, indent=1)
            f.write('\n')


if __name__ == '__main__':
    main()
