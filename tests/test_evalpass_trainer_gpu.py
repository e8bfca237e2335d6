"""--fused_validation through Trainer.eval and NodeClassificationTrainer.eval on synth-tiny (set up as
tests/test_eval_fused_trainer_gpu.py: GCN, 60 deleted edges, weights large enough that some scores saturate).

Under the flag the scores are the scoring kernel's own sigmoid, so the values are held to what they are derived from, not to the
no-flag path: z is the model's forward on the plan's edges to the bit; the AUCs are metrics.batched_roc_auc on the plan's last
scores to the bit, the AUPs within the 1e-12 of tests/test_metrics.py; loss / Df mean / Df std within 1e-12 of the fp64
restatement on those scores; df_logit is the Df segment; the subset matrix is the no-flag trainer's under the same seed.  A
second validation after ten unrelated graphs builds no CSR and no SplitPlan; an in-place edit of train_pos_edge_index rebuilds;
a forced fallback gives the no-flag values to the bit; `original` ranks only the stage's edges; the node classifier's accuracy is
scikit-learn's on the model's own logits and its loss within 1e-12 relative (the kernel forms the row terms in double)."""
import functools
import math
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
AP_TOL = 1e-12
SUM_TOL = 1e-12


def _args(kind, path, **flags):
    os.makedirs(str(path), exist_ok=True)
    return SimpleNamespace(unlearning_model=kind, gnn='gcn', dataset='synth-tiny', checkpoint_dir=str(path), eval_on_cpu=False,
                           in_dim=32, hidden_dim=64, out_dim=32, epochs=1, valid_freq=1, lr=1e-2, random_seed=42, **flags)


def _prepare():
    from gnndelete_amd.framework.data import Data, prepare_edge_deletion
    from gnndelete_amd.framework.synth import make_linkpred_dataset
    data, df_masks = make_linkpred_dataset('synth-tiny', 42)
    data = Data({k: (v.clone() if torch.is_tensor(v) else v) for k, v in data.items()})
    torch.manual_seed(7)
    prepare_edge_deletion(data, df_masks['in'], 60)
    data.dtrain_mask = data.dr_mask
    return data


@functools.lru_cache(maxsize=None)
def _request():
    """synth-tiny prepared as delete_gnn.py prepares an edge deletion, and one GCN with weights large enough that some scores
    saturate; shared by the tests, changed by none (the test that edits a tensor prepares its own copy)."""
    from gnndelete_amd.framework import get_model
    model = get_model(SimpleNamespace(unlearning_model='retrain', gnn='gcn', in_dim=32, hidden_dim=64, out_dim=32)).cuda()
    with torch.no_grad():
        for p in model.parameters():
            p.mul_(3.0)
    return _prepare(), model


def _eval(path, kind='retrain', stage='val', data=None, **flags):
    from gnndelete_amd.framework.trainer.base import Trainer
    shared, model = _request()
    tr = Trainer(_args(kind, path, **flags))
    torch.manual_seed(11)                                        # the 500 Dr subsets come from the host generator
    return tr, tr.eval(model, shared if data is None else data, stage)


def _same(a, b):
    """Two Trainer.eval tuples equal to the bit (NaN equal to NaN)."""
    flat = lambda t: list(t[:5]) + list(t[5]) + list(t[7].items())       # noqa: E731
    return all(x == y or (isinstance(x, float) and isinstance(y, float) and math.isnan(x) and math.isnan(y)) or
               (isinstance(x, tuple) and x[0] == y[0] and (x[1] == y[1] or (math.isnan(x[1]) and math.isnan(y[1]))))
               for x, y in zip(flat(a), flat(b))) and len(flat(a)) == len(flat(b))


def _check_against_the_scores(tr, out, stage, model, data):
    """The returned values against what they are derived from: the plan's z and scores."""
    from gnndelete_amd.evalpass import reference_edge_stats
    from gnndelete_amd.framework.metrics import batched_average_precision, batched_roc_auc
    plan = tr._validation_plans[('link', stage)]
    loss, dt_auc, dt_aup, df_auc, df_aup, df_logit, all_pairs, log = out
    n_pos, n_neg, n_df, n_dr = plan.segments
    with torch.no_grad():
        assert torch.equal(plan.z, model(data.x, plan.edges))
    assert torch.equal(plan.edges, data.train_pos_edge_index[:, data.dtrain_mask]) and plan.edges.is_contiguous()
    assert plan.decoded.dtype == torch.int64 and tuple(plan.decoded.shape) == (2, n_pos + n_neg + n_df + n_dr)
    s = plan.scores
    label = torch.cat([torch.ones(n_pos), torch.zeros(n_neg)]).cuda()
    assert dt_auc == float(batched_roc_auc(s[:n_pos + n_neg], label)[0])
    assert abs(dt_aup - float(batched_average_precision(s[:n_pos + n_neg], label)[0])) <= AP_TOL
    want_loss, want_mean, want_std = reference_edge_stats(s, plan.segments)
    print(stage, 'loss', loss, want_loss, 'df mean', log[f'{stage}_df_logit_mean'], want_mean, 'df std', log[f'{stage}_df_logit_std'], want_std)
    assert abs(loss - want_loss) <= SUM_TOL
    assert list(log) == [f'{stage}_{k}' for k in ('loss', 'dt_auc', 'dt_aup', 'df_auc', 'df_aup', 'df_logit_mean', 'df_logit_std')]
    assert [log[f'{stage}_{k}'] for k in ('loss', 'dt_auc', 'dt_aup')] == [loss, dt_auc, dt_aup]
    assert all(type(v) is float for v in (loss, dt_auc, dt_aup, df_auc, df_aup)) and all_pairs is None
    if n_df == 0:
        assert df_logit == [] and all(math.isnan(v) for v in (df_auc, df_aup, log[f'{stage}_df_logit_mean'], log[f'{stage}_df_logit_std']))
        return
    df_s, dr_s = s[n_pos + n_neg:n_pos + n_neg + n_df], s[n_pos + n_neg + n_df:]
    assert isinstance(df_logit, list) and df_logit == df_s.tolist()
    assert abs(log[f'{stage}_df_logit_mean'] - want_mean) <= SUM_TOL and abs(log[f'{stage}_df_logit_std'] - want_std) <= SUM_TOL
    assert abs(log[f'{stage}_df_logit_mean'] - np.mean(df_logit)) <= SUM_TOL and abs(log[f'{stage}_df_logit_std'] - np.std(df_logit)) <= SUM_TOL
    idx = tr._df_subset_index
    scores = torch.cat([df_s[None].expand(idx.shape[0], n_df), dr_s[idx]], dim=1)
    labels = torch.cat([torch.zeros(n_df), torch.ones(n_df)]).cuda()
    assert df_auc == float(batched_roc_auc(scores, labels).mean()) == log[f'{stage}_df_auc']
    assert abs(df_aup - float(batched_average_precision(scores, labels).mean())) <= AP_TOL and df_aup == log[f'{stage}_df_aup']
    assert 0.0 < df_auc < 1.0 and 0.0 < dt_auc < 1.0


@pytest.mark.parametrize('stage', ['val', 'test'])
def test_a_prepared_validation_is_derived_from_its_scores(stage, tmp_path, capsys):
    data, model = _request()
    plain, a = _eval(tmp_path / 'p', stage=stage)
    tr, b = _eval(tmp_path / 'f', stage=stage, fused_validation=True)
    assert '--fused_validation:' not in capsys.readouterr().out  # no fallback line
    assert tr.trainer_log['validation_path'] == 'prepared' and 'validation_path' not in plain.trainer_log
    assert 'eval_path' not in tr.trainer_log
    plan = tr._validation_plans[('link', stage)]
    assert plan.segments == (data[f'{stage}_pos_edge_index'].shape[1], data[f'{stage}_neg_edge_index'].shape[1], 60, int(data.dr_mask.sum()))
    assert torch.equal(plan.decoded.cpu(), torch.cat([data[f'{stage}_pos_edge_index'], data[f'{stage}_neg_edge_index'],
                                                      data.directed_df_edge_index, data.train_pos_edge_index[:, data.dr_mask]], 1).cpu())
    # the same seed gives the same 500 subsets as without the flag
    assert torch.equal(plain._df_subset_index, tr._df_subset_index) and tuple(tr._df_subset_index.shape) == (500, 60)
    assert plan.subset_index is tr._df_subset_index
    _check_against_the_scores(tr, b, stage, model, data)
    # the no-flag path beside it (printed, not held: the kernel's sigmoid is not torch's, and saturated scores may tie differently)
    print(stage, 'no flag', a[:5], 'prepared', b[:5], 'largest df_logit difference', np.abs(np.array(a[5]) - np.array(b[5])).max())
    assert list(a[7]) == list(b[7])                              # the seven log keys in today's order


def test_with_both_flags_the_prepared_pass_decides(tmp_path):
    _, a = _eval(tmp_path / 'a', fused_validation=True)
    tr, b = _eval(tmp_path / 'b', fused_validation=True, fused_eval=True)
    assert tr.trainer_log['validation_path'] == 'prepared' and 'eval_path' not in tr.trainer_log and _same(a, b)


def test_a_second_validation_builds_nothing(tmp_path, monkeypatch):
    from gnndelete_amd import graph
    data, model = _request()
    tr, first = _eval(tmp_path / 'f', fused_validation=True)
    plan = tr._validation_plans[('link', 'val')]
    calls = {'csr': 0, 'plan': 0}
    real_build, real_init = graph.build_csr, graph.SplitPlan.__init__

    def counting_build(*a, **k):
        calls['csr'] += 1
        return real_build(*a, **k)

    def counting_init(self, *a, **k):
        calls['plan'] += 1
        return real_init(self, *a, **k)
    monkeypatch.setattr(graph, 'build_csr', counting_build)
    monkeypatch.setattr(graph.SplitPlan, '__init__', counting_init)
    others = [torch.randint(0, 50, (2, 80), device='cuda') for _ in range(10)]
    for e in others:                                             # more graphs than the LRU holds (8)
        graph.graph_for(e, 50, 'gcn')
    assert calls == {'csr': 10, 'plan': 20}
    second = tr.eval(model, data, 'val')
    assert calls == {'csr': 10, 'plan': 20}, 'a second prepared validation rebuilt its graph'
    assert tr._validation_plans[('link', 'val')] is plan and _same(first, second)
    # without the flag the same sequence rebuilds on every validation (what the plan removes)
    plain, _ = _eval(tmp_path / 'p')
    before = dict(calls)
    plain.eval(model, data, 'val')
    assert calls['csr'] == before['csr'] + 1 and calls['plan'] == before['plan'] + 2
    # a released plan lets its graphs go
    held = len(graph.CACHE.held)
    plan.release()
    assert len(graph.CACHE.held) == held - 1


def test_an_in_place_edit_rebuilds_the_plan(tmp_path):
    from gnndelete_amd.framework.trainer.base import Trainer
    _, model = _request()
    data = _prepare().to('cuda')
    tr = Trainer(_args('retrain', tmp_path / 'f', fused_validation=True))
    torch.manual_seed(11)
    first = tr.eval(model, data, 'val')
    plan = tr._validation_plans[('link', 'val')]
    keep = torch.nonzero(data.dtrain_mask).flatten()[:40]
    data.train_pos_edge_index[1, keep] = 0                       # in place: 40 message-passing edges now end at node 0
    second = tr.eval(model, data, 'val')
    rebuilt = tr._validation_plans[('link', 'val')]
    assert rebuilt is not plan and rebuilt.key != plan.key and not plan._pinned
    assert torch.equal(rebuilt.edges, data.train_pos_edge_index[:, data.dtrain_mask])
    fresh = Trainer(_args('retrain', tmp_path / 'g', fused_validation=True))
    torch.manual_seed(11)
    want = fresh.eval(model, data, 'val')
    assert _same(second, want) and not _same(first, second)
    _check_against_the_scores(tr, second, 'val', model, data)


def test_a_forced_fallback_records_its_reason(tmp_path, monkeypatch, capsys):
    from gnndelete_amd import evalpass
    _, a = _eval(tmp_path / 'p')
    capsys.readouterr()
    monkeypatch.setattr(evalpass, 'validation_unsupported', lambda *a, **k: 'forced by the test')
    tr, b = _eval(tmp_path / 'f', fused_validation=True)
    assert tr.trainer_log['validation_path'] == 'torch: forced by the test' and not getattr(tr, '_validation_plans', None)
    data, model = _request()
    tr.eval(model, data, 'val')                                  # a second validation: no second line
    assert capsys.readouterr().out.count('--fused_validation: forced by the test; validating on the torch path') == 1
    assert _same(a, b)                                           # today's path itself: equal to the bit


def test_original_ranks_only_the_stage_edges(tmp_path):
    data, model = _request()
    _, a = _eval(tmp_path / 'p', kind='original')
    tr, b = _eval(tmp_path / 'f', kind='original', fused_validation=True)
    assert tr.trainer_log['validation_path'] == 'prepared' and len(tr.df_pos_edge) == 0
    plan = tr._validation_plans[('link', 'val')]
    assert plan.segments[2:] == (0, 0) and plan.subset_index is None
    _check_against_the_scores(tr, b, 'val', model, data)
    assert b[5] == [] and math.isnan(b[3]) and math.isnan(b[4]) and math.isnan(a[3]) and list(a[7]) == list(b[7])


def test_pred_all_is_passed_through(tmp_path):
    from gnndelete_amd.framework.trainer.base import Trainer, _all_pairs
    data, model = _request()
    tr = Trainer(_args('retrain', tmp_path / 'f', fused_validation=True))
    torch.manual_seed(11)
    out = tr.eval(model, data, 'test', pred_all=True)
    assert torch.equal(out[6], _all_pairs(tr._validation_plans[('link', 'test')].z))


# ------------------------------------------------------------------------------------------ node classification
@functools.lru_cache(maxsize=None)
def _node_request(gnn, classes):
    from gnndelete_amd.framework import get_model
    from gnndelete_amd.framework.synth import make_nodecls_dataset
    data = make_nodecls_dataset('synth-tiny', 42, num_classes=classes).to('cuda')
    torch.manual_seed(3)
    model = get_model(SimpleNamespace(unlearning_model='original_node', gnn=gnn, in_dim=32, hidden_dim=64, out_dim=classes)).cuda()
    with torch.no_grad():
        for p in model.parameters():
            p.mul_(2.0)
    return data, model


def _node_args(gnn, path, **flags):
    os.makedirs(str(path), exist_ok=True)
    return SimpleNamespace(unlearning_model='original_node', gnn=gnn, dataset='synth-tiny', checkpoint_dir=str(path), eval_on_cpu=False,
                           in_dim=32, hidden_dim=64, out_dim=4, epochs=1, valid_freq=1, lr=1e-2, random_seed=42, **flags)


@pytest.mark.parametrize('gnn, classes', [('gcn', 4), ('gat', 4), ('gcn', 3)])
def test_node_validation_is_accuracy_and_nll_of_the_logits(gnn, classes, tmp_path, monkeypatch):
    from sklearn.metrics import accuracy_score, f1_score
    from gnndelete_amd import graph
    from gnndelete_amd.evalpass import reference_row_nll_eval
    from gnndelete_amd.framework.trainer.base import NodeClassificationTrainer
    data, model = _node_request(gnn, classes)
    plain = NodeClassificationTrainer(_node_args(gnn, tmp_path / 'p'))
    a = plain.eval(model, data, 'val')
    assert 'validation_path' not in plain.trainer_log
    tr = NodeClassificationTrainer(_node_args(gnn, tmp_path / 'f', fused_validation=True))
    for stage in ('val', 'test'):                                # upstream reads val_mask for every stage
        loss, acc, f1, log = tr.eval(model, data, stage)
        assert tr.trainer_log['validation_path'] == 'prepared'
        plan = tr._validation_plans[('node',)]
        with torch.no_grad():
            z = model(data.x, data.edge_index)
        assert torch.equal(plan.z, z) and plan.rows.dtype == torch.int32
        assert torch.equal(plan.rows.long(), data.val_mask.nonzero().flatten())
        pred, y = z[data.val_mask].argmax(1).cpu(), data.y[data.val_mask].cpu()
        assert acc == accuracy_score(y, pred) and f1 == acc and acc == f1_score(y, pred, average='micro')
        want = float(F.nll_loss(F.log_softmax(z.double(), dim=1)[data.val_mask], data.y[data.val_mask]))
        ref_loss, ref_correct = reference_row_nll_eval(z, plan.rows, data.y)
        print(gnn, classes, stage, 'loss', loss, want, ref_loss, 'acc', acc, 'no flag', a[:3])
        assert abs(loss - want) <= SUM_TOL * abs(want) and abs(loss - ref_loss) <= SUM_TOL * abs(ref_loss)
        assert ref_correct == round(acc * plan.n_sel) and 0.0 < acc <= 1.0
        assert list(log) == [f'{stage}_loss', f'{stage}_dt_acc', f'{stage}_dt_f1'] and list(log.values()) == [loss, acc, f1]
        assert all(type(v) is float for v in (loss, acc, f1))
    assert list(a[3]) == ['val_loss', 'val_dt_acc', 'val_dt_f1']      # (the no-flag values are printed above, not held)
    # a second validation builds nothing, also after ten other graphs
    calls = []
    real = graph.build_csr
    monkeypatch.setattr(graph, 'build_csr', lambda *a, **k: calls.append(1) or real(*a, **k))
    for _ in range(10):
        graph.graph_for(torch.randint(0, 50, (2, 80), device='cuda'), 50, 'gcn')
    again = tr.eval(model, data, 'test')
    assert len(calls) == 10 and again == (loss, acc, f1, log)
    # an in-place edit of val_mask lists the rows again
    old = tr._validation_plans[('node',)]
    first_off = int(torch.nonzero(~data.val_mask).flatten()[0])
    try:
        data.val_mask[first_off] = True
        tr.eval(model, data, 'val')
        new = tr._validation_plans[('node',)]
        assert new is not old and new.n_sel == old.n_sel + 1
    finally:
        data.val_mask[first_off] = False
