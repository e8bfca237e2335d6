"""One validation of a knowledge-graph unlearning request as KGTrainer.eval runs it without a flag (the Dr triples selected and
one TypedNodeCSR built per conv on every call, three DistMult decodes, the batched [500, 2|Df|] sort, numpy on a host list)
against the prepared pass of --fused_validation (gnndelete_amd/evalpass.py: KGValidationPlan - the typed graph built once and
shared by the convs, one scoring launch pair, the rank kernels, one host read), in one process, regions alternating.  The
no-flag path is unchanged code and stands for the tree before the pass existed.

Requests: synth-biokg (93,773 nodes, 51 relation types, --df in --df_size 5: the request of bench.py --gnn rgcn, RGCNDelete
128 -> 128 -> 64) and synth-wn18 (40,943 nodes, 18 relation types, the same widths).  The model is validated as constructed (the
cost of a validation does not depend on the weights).  Two situations per request:

    device   the data stays on the device between validations (--fullgraph)
    bounce   the data is moved to the host after every validation, as the default mini-batch loops do (data.to('cpu') after
             eval, data.to(device) inside it); the region includes both moves, which both paths pay

One warm-up validation per path, then --regions regions per path of --evals validations each, the two paths taking turns; a
region is closed by the host values a validation returns.  Per path the median and the spread (min, max) of a region / evals.
A gain is claimed only where the prepared median lies below the no-flag median by more than the no-flag path's own spread.
Peak allocation during one validation of each path (torch.cuda.max_memory_allocated above the allocation before it).  The
prepared validation's steps are timed one by one with the device synchronised after each (steps_ms): the host-to-device move of
the data, the staleness check after that move (the content comparison) and on an identity hit, the edge selection and ONE typed
graph build (what the plan pays once; the no-flag path pays the selection and two builds every time), the forward, the scoring
launch pair, the subset draw, the two rankings, the host reads.  Prints one JSON line per run and writes them all to --out.

    python tools/experiments/kg_validation_fused.py [--out FILE] [--runs synth-biokg synth-wn18] [--regions 5] [--evals 1]"""
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


def region(fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n


def alternate(base_fn, prepared_fn, regions, evals):
    base_fn()
    prepared_fn()
    legs = {'no_flag': [], 'prepared': []}
    for _ in range(regions):
        legs['no_flag'].append(1e3 * region(base_fn, evals))
        legs['prepared'].append(1e3 * region(prepared_fn, evals))
    out = {}
    for name, ts in legs.items():
        out[name] = {'median_ms': round(float(np.median(ts)), 3), 'min_ms': round(min(ts), 3), 'max_ms': round(max(ts), 3),
                     'spread_ms': round(max(ts) - min(ts), 3), 'regions_ms': [round(t, 3) for t in ts]}
    out['no_flag_over_prepared'] = round(out['no_flag']['median_ms'] / out['prepared']['median_ms'], 2)
    out['prepared_below_no_flag_by_more_than_its_spread'] = bool(
        out['no_flag']['median_ms'] - out['prepared']['median_ms'] > out['no_flag']['spread_ms'])
    return out


def timed_steps(steps, reps=3):
    """Median ms of each (name, prepare, fn) over `reps` passes after one warm-up pass; prepare() runs untimed, the device is
    synchronised before and after fn()."""
    times = {name: [] for name, _, _ in steps}
    for rep in range(reps + 1):
        for name, prepare, fn in steps:
            if prepare is not None:
                prepare()
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
def prepared_steps(tr, model, data, nr):
    from gnndelete_amd import rankeval
    from gnndelete_amd.evalpass import eval_triple_scores
    from gnndelete_amd.graph import TypedNodeCSR
    model.eval()
    plan = tr._validation_plans[('kg', 'val')]
    n_pos, n_neg, n_df, n_dr = plan.segments
    n_stage, s, dev = n_pos + n_neg, {}, torch.device('cuda')

    def reads():
        torch.cat([s['stats'], s['status'].double(), s['dt'][0], s['dt'][1], s['df'][0].mean()[None], s['df'][1].mean()[None]]).tolist()
        s['scores'][n_stage:n_stage + n_df].tolist()

    def select():
        s['sel'] = (data.edge_index[:, data.dr_mask].contiguous(), data.edge_type[data.dr_mask].contiguous())
    return timed_steps([
        ('host_to_device_move', lambda: data.to('cpu'), lambda: data.to(dev)),
        ('staleness_check_after_the_move', None, lambda: plan.current(data, 'val', False, dev)),
        ('staleness_check_identity_hit', None, lambda: plan.current(data, 'val', False, dev)),
        ('dr_edge_selection', None, select),
        ('one_typed_graph_build', None, lambda: TypedNodeCSR(s['sel'][0], s['sel'][1], data.num_nodes, 2 * nr)),
        ('forward', None, lambda: s.update(z=model(data.x, plan.edges, plan.types))),
        ('scoring_launch_pair', None, lambda: s.update(zip(('scores', 'stats', 'status'), eval_triple_scores(
            s['z'], model.W.detach(), plan.src, plan.dst, plan.etype, plan.segments, check=False)))),
        ('subset_draw', None, lambda: s.update(idx=plan._draw_subsets(tr, n_dr, n_df, dev))),
        ('stage_ranking', None, lambda: s.update(dt=rankeval.subset_auc_ap(s['scores'][n_pos:n_stage], s['scores'][:n_pos], plan.all_positives))),
        ('df_ranking', None, lambda: s.update(df=rankeval.subset_auc_ap(s['scores'][n_stage:n_stage + n_df], s['scores'][n_stage + n_df:], s['idx']))),
        ('host_reads', None, reads),
    ])


def measure(graph, regions, evals, seed=42):
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
                               in_dim=i, hidden_dim=h, out_dim=o, num_edge_type=nr, random_seed=seed, fused_validation=False)
        tr = KGTrainer(args)
        data = data.to('cuda')
        half = data.dr_mask[:data.dr_mask.shape[0] // 2]
        res = {'graph': graph, 'gnn': 'rgcn', 'dims': list(DIMS), 'df': DF, 'df_size': DF_SIZE, 'nodes': int(data.num_nodes),
               'relation_types': nr, 'typed_dr_edges': int(data.dr_mask.sum()), 'df_triples': int(data.directed_df_edge_index.shape[1]),
               'dr_triples': int(half.sum()), 'val_pos': int(data.val_pos_edge_index.shape[1]), 'val_neg': int(data.val_neg_edge_index.shape[1]),
               'subset_draw': 'host' if int(half.sum()) <= tr.FAST_SUBSETS_ABOVE else 'device', 'regions': regions, 'evals_per_region': evals,
               'model': 'as constructed (not trained)'}
        last = {}

        def validate(prepared, bounce):
            tr.args.fused_validation = prepared
            last[prepared] = tr.eval(model, data, 'val')
            if bounce:
                data.to('cpu')
        for name, bounce in (('device', False), ('bounce', True)):
            res[name] = alternate(lambda: validate(False, bounce), lambda: validate(True, bounce), regions, evals)
            data.to('cuda')
        res['validation_path'] = tr.trainer_log.get('validation_path')
        res['peak_allocation_mib'] = {'no_flag': peak_mib(lambda: validate(False, False)), 'prepared': peak_mib(lambda: validate(True, False))}
        keys = ('loss', 'dt_auc', 'dt_aup', 'df_auc', 'df_aup')
        res['values'] = {'no_flag': dict(zip(keys, last[False][:5])), 'prepared': dict(zip(keys, last[True][:5]))}
        res['df_logit_max_abs_diff'] = float(np.abs(np.array(last[False][5]) - np.array(last[True][5])).max())
        res['prepared_steps_ms'] = prepared_steps(tr, model, data, nr)
        res['kernel_source_stamp'] = _lib.build_stamp()[0]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--runs', nargs='+', default=['synth-wn18', 'synth-biokg'])
    ap.add_argument('--regions', type=int, default=5)
    ap.add_argument('--evals', type=int, default=1)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('kg_validation_fused.py measures on the GPU: no device found')
    runs = []
    for graph in a.runs:
        runs.append(measure(graph, a.regions, a.evals))
        print(json.dumps(runs[-1]), flush=True)
        if a.out:                                        # (rewritten after every run: a later run that fails leaves the earlier ones)
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, 'w') as f:
                json.dump({'kernel_source_stamp': runs[0]['kernel_source_stamp'], 'runs': runs}, f, indent=1)
                f.write('\n')


if __name__ == '__main__':
    main()
