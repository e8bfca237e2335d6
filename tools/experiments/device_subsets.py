"""One validation of an unlearning request under --fused_validation --device_subsets (gnndelete_amd/subsets.py: the 500 Dr subsets
drawn inside the rank kernel from one host randint) against --fused_validation alone (500 permutations per validation and a
[500, |Df|] int64 index matrix), in one process, regions alternating.  --fused_validation alone is unchanged code and stands for
the tree before the flag existed.

Knowledge-graph requests: synth-biokg (93,773 nodes, 51 relation types, --df in --df_size 5: the request of bench.py --gnn rgcn,
RGCNDelete 128 -> 128 -> 64) and synth-wn18 (40,943 nodes, 18 relation types, the same widths), validated as constructed (the
cost of a validation does not depend on the weights).  Two situations per request:

    device   the data stays on the device between validations (--fullgraph)
    bounce   the data is moved to the host after every validation, as the default mini-batch loops do; the region includes both
             moves, which both paths pay

One warm-up validation per path, then --regions regions per path of --evals validations each, the two paths taking turns; a
region is closed by the host values a validation returns.  Per path the median and the spread (min, max) of a region / evals.
A gain is claimed only where the flagged median lies below the unflagged median by more than the unflagged path's own spread.
Peak allocation during one validation of each path (torch.cuda.max_memory_allocated above the allocation before it), and the
flagged validation's stages one by one with the device synchronised after each (stages_ms): forward, scoring, stage ranking, Df
ranking (drawn, and beside it the unflagged pair: subset draw + ranking through the index matrix), host reads.

Link request: synth-collab (--df in --df_size 5, GCN in -> 128 -> 64).  Its plan draws once per request, so what is compared is
the FIRST validation of a fresh trainer (the plan's build and one validation) and the allocation it leaves behind, then a
second validation on the held plan.  Prints one JSON line per run and writes them all to --out.

    python tools/experiments/device_subsets.py [--out profiles/device_subsets.json] [--runs synth-wn18 synth-biokg synth-collab]
                                               [--regions 5] [--evals 1]"""
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

DF, DF_SIZE = 'in', 5.0
DIMS = (128, 128, 64)
KEYS = ('loss', 'dt_auc', 'dt_aup', 'df_auc', 'df_aup')


def region(fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n


def summary(legs):
    out = {}
    for name, ts in legs.items():
        out[name] = {'median_ms': round(float(np.median(ts)), 3), 'min_ms': round(min(ts), 3), 'max_ms': round(max(ts), 3),
                     'spread_ms': round(max(ts) - min(ts), 3), 'regions_ms': [round(t, 3) for t in ts]}
    out['upstream_draw_over_device_draw'] = round(out['upstream_draw']['median_ms'] / out['device_draw']['median_ms'], 2)
    out['device_draw_below_upstream_draw_by_more_than_its_spread'] = bool(
        out['upstream_draw']['median_ms'] - out['device_draw']['median_ms'] > out['upstream_draw']['spread_ms'])
    return out


def alternate(base_fn, flagged_fn, regions, evals):
    base_fn()
    flagged_fn()
    legs = {'upstream_draw': [], 'device_draw': []}
    for _ in range(regions):
        legs['upstream_draw'].append(1e3 * region(base_fn, evals))
        legs['device_draw'].append(1e3 * region(flagged_fn, evals))
    return summary(legs)


def timed_steps(steps, reps=3):
    """Median ms of each (name, fn) over `reps` passes after one warm-up pass, the device synchronised before and after fn()."""
    times = {name: [] for name, _ in steps}
    for rep in range(reps + 1):
        for name, fn in steps:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if rep:
                times[name].append(1e3 * (time.perf_counter() - t0))
    return {name: round(float(np.median(ts)), 3) for name, ts in times.items()}


def peak_mib(fn):
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return round((torch.cuda.max_memory_allocated() - before) / 2 ** 20, 1)


@torch.no_grad()
def kg_stages(tr, model, data):
    from gnndelete_amd import rankeval
    from gnndelete_amd.evalpass import eval_triple_scores
    model.eval()
    plan = tr._validation_plans[('kg', 'val')]
    n_pos, n_neg, n_df, n_dr = plan.segments
    n_stage, s, dev = n_pos + n_neg, {}, torch.device('cuda')

    def reads():
        torch.cat([s['stats'], s['status'].double(), s['dt'][0], s['dt'][1], s['df'][0].mean()[None], s['df'][1].mean()[None]]).tolist()
        s['scores'][n_stage:n_stage + n_df].tolist()
    df_s, dr_s = (lambda: s['scores'][n_stage:n_stage + n_df]), (lambda: s['scores'][n_stage + n_df:])
    return timed_steps([
        ('forward', lambda: s.update(z=model(data.x, plan.edges, plan.types))),
        ('scoring_launch_pair', lambda: s.update(zip(('scores', 'stats', 'status'), eval_triple_scores(
            s['z'], model.W.detach(), plan.src, plan.dst, plan.etype, plan.segments, check=False)))),
        ('stage_ranking', lambda: s.update(dt=rankeval.subset_auc_ap(s['scores'][n_pos:n_stage], s['scores'][:n_pos], plan.all_positives))),
        ('df_ranking_drawn', lambda: s.update(df=rankeval.subset_auc_ap_drawn(df_s(), dr_s(), int(torch.randint(0, 2 ** 31 - 1, (1,))), 0,
                                                                             plan.N_SUBSETS, n_df))),
        ('upstream_subset_draw', lambda: s.update(idx=plan._draw_subsets(tr, n_dr, n_df, dev))),
        ('df_ranking_through_the_index_matrix', lambda: rankeval.subset_auc_ap(df_s(), dr_s(), s['idx'])),
        ('host_reads', reads),
    ])


def measure_kg(graph, regions, evals, seed=42):
    from gnndelete_amd import _lib
    from gnndelete_amd.framework.data import prepare_edge_deletion, resolve_df_size
    from gnndelete_amd.framework.models import RGCNDelete
    from gnndelete_amd.framework.synth import KG_SHAPES, make_kg_dataset
    from gnndelete_amd.framework.trainer.kg import KGTrainer
    from gnndelete_amd.framework.utils import seed_everything
    nr = KG_SHAPES[graph][1]
    with tempfile.TemporaryDirectory() as ckpt:
        data, df = make_kg_dataset(graph, seed=seed)
        seed_everything(seed)
        prepare_edge_deletion(data, df[DF], resolve_df_size(DF_SIZE, data.train_pos_edge_index.shape[1]), True, nr)
        i, h, o = DIMS
        model = RGCNDelete(SimpleNamespace(in_dim=i, hidden_dim=h, out_dim=o), data.num_nodes, nr, data.sdf_node_1hop_mask,
                           data.sdf_node_2hop_mask).cuda()
        args = SimpleNamespace(unlearning_model='gnndelete_nodeemb', gnn='rgcn', dataset=graph, checkpoint_dir=ckpt, eval_on_cpu=False,
                               in_dim=i, hidden_dim=h, out_dim=o, num_edge_type=nr, random_seed=seed, fused_validation=True, device_subsets=False)
        tr = KGTrainer(args)
        data = data.to('cuda')
        half = data.dr_mask[:data.dr_mask.shape[0] // 2]
        n_df, n_dr = int(data.directed_df_edge_index.shape[1]), int(half.sum())
        res = {'graph': graph, 'trainer': 'KGTrainer', 'gnn': 'rgcn', 'dims': list(DIMS), 'df': DF, 'df_size': DF_SIZE, 'nodes': int(data.num_nodes),
               'relation_types': nr, 'df_triples': n_df, 'dr_triples': n_dr, 'index_matrix_mib': round(500 * n_df * 8 / 2 ** 20, 1),
               'upstream_subset_draw': 'host' if n_dr <= tr.FAST_SUBSETS_ABOVE else 'device', 'regions': regions, 'evals_per_region': evals,
               'model': 'as constructed (not trained)'}
        last = {}

        def validate(flagged, bounce):
            tr.args.device_subsets = flagged
            last[flagged] = tr.eval(model, data, 'val')
            if bounce:
                data.to('cpu')
        for name, bounce in (('device', False), ('bounce', True)):
            res[name] = alternate(lambda: validate(False, bounce), lambda: validate(True, bounce), regions, evals)
            data.to('cuda')
        res['validation_path'], res['subset_draw'] = tr.trainer_log.get('validation_path'), tr.trainer_log.get('subset_draw')
        res['peak_allocation_mib'] = {'upstream_draw': peak_mib(lambda: validate(False, False)), 'device_draw': peak_mib(lambda: validate(True, False))}
        res['values'] = {'upstream_draw': dict(zip(KEYS, last[False][:5])), 'device_draw': dict(zip(KEYS, last[True][:5]))}
        res['stages_ms'] = kg_stages(tr, model, data)
        res['kernel_source_stamp'] = _lib.build_stamp()[0]
    return res


def measure_link(graph, regions, evals, seed=42):
    from gnndelete_amd import _lib
    from gnndelete_amd.framework import get_model
    from gnndelete_amd.framework.data import prepare_edge_deletion, resolve_df_size
    from gnndelete_amd.framework.synth import make_linkpred_dataset
    from gnndelete_amd.framework.trainer.base import Trainer
    with tempfile.TemporaryDirectory() as ckpt:
        torch.manual_seed(seed)
        data, df = make_linkpred_dataset(graph, seed=seed)
        prepare_edge_deletion(data, df[DF], resolve_df_size(DF_SIZE, data.train_pos_edge_index.shape[1]))
        args = dict(unlearning_model='gnndelete_nodeemb', gnn='gcn', dataset=graph, checkpoint_dir=ckpt, eval_on_cpu=False,
                    in_dim=int(data.x.shape[1]), hidden_dim=128, out_dim=64, random_seed=seed, fused_validation=True)
        model = get_model(SimpleNamespace(**args), data.sdf_node_1hop_mask, data.sdf_node_2hop_mask).cuda()
        data = data.to('cuda')
        n_df, n_dr = int(data.directed_df_edge_index.shape[1]), int(data.dr_mask.sum())
        res = {'graph': graph, 'trainer': 'Trainer', 'gnn': 'gcn', 'dims': [args['in_dim'], 128, 64], 'df': DF, 'df_size': DF_SIZE,
               'nodes': int(data.num_nodes), 'df_edges': n_df, 'dr_edges': n_dr, 'index_matrix_mib': round(500 * n_df * 8 / 2 ** 20, 1),
               'regions': regions, 'model': 'as constructed (not trained)'}
        held, last, left = {}, {}, {}

        def first(flagged):
            """A fresh trainer's first validation: the plan's build (edge selection and graphs included, on both paths) and one
            validation; the trainer before it is dropped first, so that its index matrix does not count."""
            held.pop(flagged, None)
            torch.cuda.synchronize()
            before = torch.cuda.memory_allocated()
            tr = held[flagged] = Trainer(SimpleNamespace(device_subsets=flagged, **args))
            last[flagged] = tr.eval(model, data, 'val')
            left[flagged] = round((torch.cuda.memory_allocated() - before) / 2 ** 20, 1)
        res['first_validation'] = alternate(lambda: first(False), lambda: first(True), regions, 1)
        res['allocation_left_by_the_first_validation_mib'] = {'upstream_draw': left[False], 'device_draw': left[True]}
        res['later_validation'] = alternate(lambda: held[False].eval(model, data, 'val'), lambda: held[True].eval(model, data, 'val'), regions, evals)
        res['peak_allocation_mib'] = {'upstream_draw': peak_mib(lambda: held[False].eval(model, data, 'val')),
                                      'device_draw': peak_mib(lambda: held[True].eval(model, data, 'val'))}
        res['validation_path'], res['subset_draw'] = held[True].trainer_log.get('validation_path'), held[True].trainer_log.get('subset_draw')
        res['values'] = {'upstream_draw': dict(zip(KEYS, last[False][:5])), 'device_draw': dict(zip(KEYS, last[True][:5]))}
        res['kernel_source_stamp'] = _lib.build_stamp()[0]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--runs', nargs='+', default=['synth-wn18', 'synth-biokg', 'synth-collab'])
    ap.add_argument('--regions', type=int, default=5)
    ap.add_argument('--evals', type=int, default=1)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('device_subsets.py measures on the GPU: no device found')
    runs = []
    for graph in a.runs:
        runs.append((measure_link if graph == 'synth-collab' else measure_kg)(graph, a.regions, a.evals))
        print(json.dumps(runs[-1]), flush=True)
        if a.out:                                        # (rewritten after every run: a later run that fails leaves the earlier ones)
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, 'w') as f:
                json.dump({'kernel_source_stamp': runs[0]['kernel_source_stamp'], 'runs': runs}, f, indent=1)
                f.write('\n')


if __name__ == '__main__':
    main()
