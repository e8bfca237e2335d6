"""One validation of an unlearning request with --fused_eval (Trainer.eval as it stands: the message-passing edges selected and
their CSR / SplitPlans rebuilt on every call, three decodes, host statistics) against the prepared pass of --fused_validation
(gnndelete_amd/evalpass.py: graph, edge list and subsets built once, one scoring launch pair, one host read), in one process,
regions alternating; and the node-classification pair (NodeClassificationTrainer.eval with and without the flag).

Link prediction: synth-collab (--df in --df_size 5) and synth-dblp (--df out --df_size 2.5), GCN in -> 128 -> 64,
--unlearning_model gnndelete_nodeemb with its defaults.  The request first trains for 300 epochs with a validation every 100 on
the --fused_eval path, as delete_gnn.py would: the trainer's own train_time of the blocks after the first (which holds the graph
capture) is the per-epoch time, so a validation can be stated in epochs (epochs_per_validation).  Node classification:
synth-collab, GCN in -> 128 -> 4 classes, --fused_backbone training for 300 epochs likewise.  Then, on that trained model: two
warm-up validations per path and seven regions per path of three validations each, the two paths taking turns; a region is
closed by the host values a validation returns.  Per path the median and the spread (min, max) of a region / 3.  A gain is
claimed only where the prepared median lies below the other path's median by more than that path's own spread.  The prepared
validation's steps are timed one by one with the device synchronised after each (steps_ms: forward, scoring launch, the two
rankings, host reads).  Prints one JSON line per run and writes them all to --out as one JSON object.

    python tools/experiments/validation_fused.py [--out FILE] [--runs link:synth-collab link:synth-dblp node:synth-collab]"""
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
WARMUP, REGIONS, EVALS = 2, 7, 3


def region(fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n


def alternate(base_fn, prepared_fn, n, base_name):
    for _ in range(WARMUP):
        base_fn()
        prepared_fn()
    legs = {base_name: [], 'prepared': []}
    for _ in range(REGIONS):
        legs[base_name].append(1e3 * region(base_fn, n))
        legs['prepared'].append(1e3 * region(prepared_fn, n))
    out = {}
    for name, ts in legs.items():
        out[name] = {'median_ms': round(float(np.median(ts)), 4), 'min_ms': round(min(ts), 4), 'max_ms': round(max(ts), 4),
                     'spread_ms': round(max(ts) - min(ts), 4), 'regions_ms': [round(t, 4) for t in ts]}
    out[f'{base_name}_over_prepared'] = round(out[base_name]['median_ms'] / out['prepared']['median_ms'], 2)
    out[f'prepared_below_{base_name}_by_more_than_its_spread'] = bool(
        out[base_name]['median_ms'] - out['prepared']['median_ms'] > out[base_name]['spread_ms'])
    return out


def timed_steps(steps, reps=5):
    """Median ms of each (name, fn) over `reps` passes after one warm-up pass, the device synchronised after each step."""
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


def epochs_per_validation(res, names, epoch_ms):
    for name in names:
        v = res['validation'][name]['median_ms']
        res['validation'][name]['epochs_per_validation'] = round(v / epoch_ms, 1)
        res['validation'][name]['share_of_run_at_valid_freq_100'] = round(v / (v + VALID_FREQ * epoch_ms), 4)


@torch.no_grad()
def link_steps(tr, model, data):
    from gnndelete_amd import rankeval
    from gnndelete_amd.evalpass import eval_edge_scores
    model.eval()
    plan = tr._validation_plans[('link', 'val')]
    n_pos, n_neg, n_df, n_dr = plan.segments
    n_stage, s = n_pos + n_neg, {}

    def reads():
        torch.cat([s['stats'], s['status'].double(), s['dt'][0], s['dt'][1], s['df'][0].mean()[None], s['df'][1].mean()[None]]).tolist()
        s['scores'][n_stage:n_stage + n_df].tolist()
    return timed_steps([
        ('forward', lambda: s.update(z=model(data.x, plan.edges))),
        ('scoring_launch', lambda: s.update(zip(('scores', 'stats', 'status'), eval_edge_scores(s['z'], plan.src, plan.dst, plan.segments, check=False)))),
        ('dt_ranking', lambda: s.update(dt=rankeval.subset_auc_ap(s['scores'][n_pos:n_stage], s['scores'][:n_pos], plan.all_positives))),
        ('df_ranking', lambda: s.update(df=rankeval.subset_auc_ap(s['scores'][n_stage:n_stage + n_df], s['scores'][n_stage + n_df:], plan.subset_index))),
        ('host_reads', reads),
    ])


def measure_link(graph, seed=42):
    from gnndelete_amd import _lib
    from gnndelete_amd.framework import get_model, get_trainer
    from gnndelete_amd.framework.data import prepare_edge_deletion, resolve_df_size
    from gnndelete_amd.framework.synth import make_linkpred_dataset
    kind, pct = REQUESTS[graph]
    with tempfile.TemporaryDirectory() as ckpt:
        torch.manual_seed(seed)
        data, df = make_linkpred_dataset(graph, seed=seed)
        prepare_edge_deletion(data, df[kind], resolve_df_size(pct, data.train_pos_edge_index.shape[1]))
        args = SimpleNamespace(unlearning_model='gnndelete_nodeemb', gnn='gcn', dataset=graph, checkpoint_dir=ckpt, eval_on_cpu=False,
                               in_dim=int(data.x.shape[1]), hidden_dim=128, out_dim=64, epochs=TRAIN_EPOCHS, valid_freq=VALID_FREQ, lr=1e-3,
                               loss_fct='mse_mean', loss_type='both_layerwise', alpha=0.5, random_seed=seed, fused_eval=True,
                               fused_validation=False)
        model = get_model(args, data.sdf_node_1hop_mask, data.sdf_node_2hop_mask).cuda()
        opt = [torch.optim.Adam(model.deletion1.parameters(), lr=args.lr), torch.optim.Adam(model.deletion2.parameters(), lr=args.lr)]
        tr = get_trainer(args)
        tr.train(model, data, opt, args, None, None, None)
        blocks = [r['train_time'] for r in tr.trainer_log['log'] if 'train_time' in r]
        data = data.to('cuda')
        res = {'task': 'linkpred', 'graph': graph, 'gnn': 'gcn', 'df': kind, 'df_size': pct, 'nodes': int(data.num_nodes),
               'dr_edges': int(data.dr_mask.sum()), 'df_edges': int(data.directed_df_edge_index.shape[1]),
               'val_pos_edges': int(data.val_pos_edge_index.shape[1]), 'val_neg_edges': int(data.val_neg_edge_index.shape[1]),
               'evals_per_region': EVALS, 'regions': REGIONS, 'train_epochs': TRAIN_EPOCHS,
               'train_blocks_ms_per_epoch': [round(1e3 * b, 4) for b in blocks]}
        res['epoch_ms'] = round(1e3 * float(np.median(blocks[1:])), 4)
        last = {}

        def validate(prepared):
            tr.args.fused_validation = prepared
            last[prepared] = tr.eval(model, data, 'val')
        res['validation'] = alternate(lambda: validate(False), lambda: validate(True), EVALS, 'fused_eval')
        res['eval_path'], res['validation_path'] = tr.trainer_log.get('eval_path'), tr.trainer_log.get('validation_path')
        epochs_per_validation(res, ('fused_eval', 'prepared'), res['epoch_ms'])
        keys = ('loss', 'dt_auc', 'dt_aup', 'df_auc', 'df_aup')
        res['values'] = {'fused_eval': dict(zip(keys, last[False][:5])), 'prepared': dict(zip(keys, last[True][:5]))}
        res['df_logit_max_abs_diff'] = float(np.abs(np.array(last[False][5]) - np.array(last[True][5])).max())
        res['prepared_steps_ms'] = link_steps(tr, model, data)
        res['kernel_source_stamp'] = _lib.build_stamp()[0]
    return res


def measure_node(graph, seed=42, classes=4):
    from gnndelete_amd import _lib
    from gnndelete_amd.evalpass import read_row_nll_eval, row_nll_eval
    from gnndelete_amd.framework import get_model
    from gnndelete_amd.framework.synth import make_nodecls_dataset
    from gnndelete_amd.framework.trainer.base import NodeClassificationTrainer
    with tempfile.TemporaryDirectory() as ckpt:
        torch.manual_seed(seed)
        data = make_nodecls_dataset(graph, seed=seed, num_classes=classes)
        args = SimpleNamespace(unlearning_model='original_node', gnn='gcn', dataset=graph, checkpoint_dir=ckpt, eval_on_cpu=False,
                               in_dim=int(data.x.shape[1]), hidden_dim=128, out_dim=classes, epochs=TRAIN_EPOCHS, valid_freq=VALID_FREQ,
                               lr=1e-2, random_seed=seed, fused_backbone=True, fused_validation=False)
        model = get_model(args).cuda()
        opt = torch.optim.Adam(model.parameters(), lr=args.lr)
        tr = NodeClassificationTrainer(args)
        t0 = time.perf_counter()
        tr.train(model, data, opt, args)
        torch.cuda.synchronize()
        train_s = time.perf_counter() - t0
        data = data.to('cuda')
        res = {'task': 'nodecls', 'graph': graph, 'gnn': 'gcn', 'nodes': int(data.num_nodes), 'edges': int(data.edge_index.shape[1]),
               'classes': classes, 'val_rows': int(data.val_mask.sum()), 'evals_per_region': EVALS, 'regions': REGIONS,
               'train_epochs': TRAIN_EPOCHS, 'backbone_step': tr.trainer_log.get('backbone_step')}
        last = {}

        def validate(prepared):
            tr.args.fused_validation = prepared
            last[prepared] = tr.eval(model, data, 'val')
        res['validation'] = alternate(lambda: validate(False), lambda: validate(True), EVALS, 'torch')
        res['validation_path'] = tr.trainer_log.get('validation_path')
        # the epoch time: the whole train call less its validations on the path it ran them on (no flag), per epoch
        n_val = TRAIN_EPOCHS // VALID_FREQ
        res['epoch_ms'] = round((1e3 * train_s - n_val * res['validation']['torch']['median_ms']) / TRAIN_EPOCHS, 4)
        res['epoch_ms_note'] = 'train() wall time less its validations at the measured no-flag median, per epoch; includes the first epoch\'s set-up'
        epochs_per_validation(res, ('torch', 'prepared'), res['epoch_ms'])
        keys = ('loss', 'dt_acc', 'dt_f1')
        res['values'] = {'torch': dict(zip(keys, last[False][:3])), 'prepared': dict(zip(keys, last[True][:3]))}
        plan, s = tr._validation_plans[('node',)], {}
        with torch.no_grad():
            model.eval()
            res['prepared_steps_ms'] = timed_steps([
                ('forward', lambda: s.update(z=model(data.x, plan.edges))),
                ('scoring_launch', lambda: s.update(out=row_nll_eval(s['z'], plan.rows, data.y))),
                ('host_reads', lambda: read_row_nll_eval(s['out'])),
            ])
        res['kernel_source_stamp'] = _lib.build_stamp()[0]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--runs', nargs='+', default=['link:synth-collab', 'link:synth-dblp', 'node:synth-collab'])
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('validation_fused.py measures on the GPU: no device found')
    runs = []
    for run in a.runs:
        task, graph = run.split(':')
        runs.append(measure_link(graph) if task == 'link' else measure_node(graph))
        print(json.dumps(runs[-1]), flush=True)
        if a.out:                                        # (rewritten after every run: a later run that fails leaves the earlier ones)
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, 'w') as f:
                json.dump({'kernel_source_stamp': runs[0]['kernel_source_stamp'], 'runs': runs}, f, indent=1)
                f.write('\n')


if __name__ == '__main__':
    main()
