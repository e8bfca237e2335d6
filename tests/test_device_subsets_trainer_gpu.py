"""--device_subsets through KGTrainer.eval and Trainer.eval (gnndelete_amd/evalpass.py, gnndelete_amd/subsets.py) on the request
of tests/test_kg_evalpass_trainer_gpu.py, built here: 700 nodes, 5,000 triples, 60 deleted, 5 and 25 relation types;
RGCNDelete and one RGATDelete case, widths 32 -> 32 -> 32, weights scaled so that some Df / Dr scores saturate.

With --fused_validation --device_subsets the validation runs the prepared pass, draws ONE host randint and no subsets: everything
but df_auc / df_aup is the --fused_validation value to the bit; df_auc is the mean of metrics.batched_roc_auc on the plan's scores
under subsets.draw(seed, 0, 500, |Df|, |Dr|) to the bit, df_aup within 1e-12.  The subsets are not upstream's, so the two paths'
df_auc / df_aup are held to each other statistically: within six standard errors of a difference of two independent means of
500, both deviations measured here on the plan's scores.  Above FAST_SUBSETS_ABOVE (set to 0) the host generator is left where
the unflagged validation leaves it, and the batch loop and the --fullgraph loop train to the same bits; at the default
threshold the stream differs and the flagged run repeats itself.  What the flag does not take says why and is today's path to
the bit.  The link trainer's plan holds a seed and no index matrix."""
import copy
import functools
import math
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
AP_TOL = 1e-12
N_SUBSETS = 500


# ---------------------------------------------------------------------------------------------- the knowledge-graph request
def _args(path, nr, kind='gnndelete_nodeemb', gnn='rgcn', **flags):
    os.makedirs(str(path), exist_ok=True)
    return SimpleNamespace(unlearning_model=kind, gnn=gnn, dataset='synth-kg-tiny', checkpoint_dir=str(path), eval_on_cpu=False,
                           in_dim=32, hidden_dim=32, out_dim=32, epochs=2, valid_freq=1, lr=1e-2, alpha=0.5, loss_fct='mse_mean',
                           loss_type='both_layerwise', batch_size=30, num_steps=3, num_edge_type=nr, random_seed=42, **flags)


@functools.lru_cache(maxsize=None)
def _prepared(nr, n_df=60):
    """700 nodes, 5,000 triples, n_df deleted; shared, changed by none (every test clones it)."""
    from gnndelete_amd.framework.data import prepare_edge_deletion
    from gnndelete_amd.framework.synth import make_kg_dataset
    data, dfm = make_kg_dataset(None, seed=3, shape=(700, nr, 5000))
    torch.manual_seed(3)
    prepare_edge_deletion(data, dfm['in'], n_df, True, nr)
    return data


def _request(nr, n_df=60):
    return _prepared(nr, n_df).clone()


@functools.lru_cache(maxsize=None)
def _model_state(gnn, nr, out_dim=32, n_df=60):
    from gnndelete_amd.framework import models as M
    data = _prepared(nr, n_df)
    torch.manual_seed(5)
    cls = {'rgcn': M.RGCNDelete, 'rgat': M.RGATDelete}[gnn]
    model = cls(SimpleNamespace(in_dim=32, hidden_dim=32, out_dim=out_dim), data.num_nodes, nr, data.sdf_node_1hop_mask, data.sdf_node_2hop_mask)
    with torch.no_grad():
        for name, p in model.named_parameters():
            if name.endswith('bias'):
                p.copy_(torch.randn_like(p) * 0.1)
            elif name in ('node_emb.weight', 'W'):
                p.mul_(3.0)                                          # embeddings and a DistMult table large enough to saturate scores
    return model


def _model(gnn, nr, out_dim=32, n_df=60):
    return copy.deepcopy(_model_state(gnn, nr, out_dim, n_df)).cuda()


def _eval(path, nr, gnn='rgcn', stage='val', data=None, model=None, fast_above=None, seed=11, **flags):
    from gnndelete_amd.framework.trainer.kg import KGTrainer
    tr = KGTrainer(_args(path, nr, 'gnndelete_nodeemb', gnn, **flags))
    if fast_above is not None:
        tr.FAST_SUBSETS_ABOVE = fast_above
    torch.manual_seed(seed)
    out = tr.eval(_model(gnn, nr) if model is None else model, _request(nr) if data is None else data, stage)
    return tr, out, torch.get_rng_state()


def _seed_of(seed):
    """The validation's one host call under torch.manual_seed(seed); the caller's generator state is put back."""
    state = torch.get_rng_state()
    torch.manual_seed(seed)
    value = int(torch.randint(0, 2 ** 31 - 1, (1,)))
    torch.set_rng_state(state)
    return value


def _same(a, b):
    """Two eval tuples equal to the bit (NaN equal to NaN)."""
    eq = lambda x, y: x == y or (isinstance(x, float) and isinstance(y, float) and math.isnan(x) and math.isnan(y))       # noqa: E731
    return (all(eq(float(x), float(y)) for x, y in zip(a[:5], b[:5])) and a[5] == b[5] and a[6] is None and b[6] is None and
            list(a[7]) == list(b[7]) and all(eq(float(a[7][k]), float(b[7][k])) for k in a[7]))


def _all_but_the_df_ranking(out, stage):
    loss, dt_auc, dt_aup, _, _, df_logit, _, log = out
    return loss, dt_auc, dt_aup, df_logit, log[f'{stage}_df_logit_mean'], log[f'{stage}_df_logit_std'], log[f'{stage}_loss'], log[f'{stage}_dt_auc'], log[f'{stage}_dt_aup']


def _segments(plan):
    n_pos, n_neg, n_df, n_dr = plan.segments
    s = plan.scores
    return s[n_pos + n_neg:n_pos + n_neg + n_df], s[n_pos + n_neg + n_df:], n_df, n_dr


# ---------------------------------------------------------------------------------------------- KGTrainer.eval under the flag
@pytest.mark.parametrize('gnn, nr, stage', [('rgcn', 5, 'val'), ('rgcn', 25, 'test'), ('rgat', 5, 'val')])
def test_the_df_ranking_is_the_drawn_subsets_on_the_plans_scores(gnn, nr, stage, tmp_path, capsys):
    from gnndelete_amd import subsets
    from gnndelete_amd.framework.metrics import batched_average_precision, batched_roc_auc
    model = _model(gnn, nr)
    plain, a, _ = _eval(tmp_path / 'u', nr, gnn, stage=stage, model=model, fused_validation=True)
    tr, b, _ = _eval(tmp_path / 'f', nr, gnn, stage=stage, model=model, fused_validation=True, device_subsets=True)
    out = capsys.readouterr().out
    assert '--device_subsets:' not in out and '--fused_validation:' not in out                   # no fallback line
    assert tr.trainer_log['validation_path'] == 'prepared' and tr.trainer_log['subset_draw'] == 'device'
    assert 'subset_draw' not in plain.trainer_log
    plan = tr._validation_plans[('kg', stage)]
    assert plan.subsets is None and plain._validation_plans[('kg', stage)].subsets is not None
    # everything but the Df ranking: the --fused_validation values to the bit
    assert _all_but_the_df_ranking(a, stage) == _all_but_the_df_ranking(b, stage) and list(a[7]) == list(b[7])
    assert torch.equal(plan.scores, plain._validation_plans[('kg', stage)].scores)
    # the Df ranking: the stream's subsets under the validation's one randint, on the plan's scores
    df_s, dr_s, n_df, n_dr = _segments(plan)
    assert (n_df, plan.subset_seed) == (60, _seed_of(11)) and n_dr > 4000
    idx = subsets.draw(plan.subset_seed, 0, N_SUBSETS, n_df, n_dr)
    assert np.array_equal(idx[:3].cpu().numpy(), subsets.reference_draw(plan.subset_seed, 0, 3, n_df, n_dr))
    scores = torch.cat([df_s[None].expand(N_SUBSETS, n_df), dr_s[idx]], dim=1)
    labels = torch.cat([torch.zeros(n_df), torch.ones(n_df)]).cuda()
    df_auc, df_aup = b[3], b[4]
    print(stage, 'df_auc', df_auc, 'upstream draw', a[3], 'df_aup', df_aup, 'upstream draw', a[4])
    assert df_auc == float(batched_roc_auc(scores, labels).mean()) == b[7][f'{stage}_df_auc']
    assert abs(df_aup - float(batched_average_precision(scores, labels).mean())) <= AP_TOL and df_aup == b[7][f'{stage}_df_aup']
    assert type(df_auc) is float and type(df_aup) is float and 0.0 < df_auc < 1.0
    # the same seed again: the same tuple; another seed: other subsets
    _, again, _ = _eval(tmp_path / 'g', nr, gnn, stage=stage, model=model, fused_validation=True, device_subsets=True)
    assert _same(again, b)
    other, c, _ = _eval(tmp_path / 'h', nr, gnn, stage=stage, model=model, seed=12, fused_validation=True, device_subsets=True)
    assert other._validation_plans[('kg', stage)].subset_seed == _seed_of(12) != plan.subset_seed
    assert c[3] != df_auc and _all_but_the_df_ranking(c, stage) == _all_but_the_df_ranking(b, stage)


@pytest.mark.parametrize('gnn, nr', [('rgcn', 5), ('rgcn', 25), ('rgat', 5)])
def test_the_two_draws_agree_within_six_standard_errors(gnn, nr, tmp_path):
    """df_auc / df_aup are means over 500 subsets on either path, from independent draws: their difference is held to six standard
    errors, sqrt((s_f^2 + s_u^2) / 500), with s_f and s_u the (population) standard deviations of the 500 per-subset values of
    each path, measured on the plan's scores with that path's subsets."""
    from gnndelete_amd import rankeval, subsets
    model = _model(gnn, nr)
    plain, a, _ = _eval(tmp_path / 'u', nr, gnn, model=model, fused_validation=True)
    tr, b, _ = _eval(tmp_path / 'f', nr, gnn, model=model, fused_validation=True, device_subsets=True)
    plan_u, plan_f = plain._validation_plans[('kg', 'val')], tr._validation_plans[('kg', 'val')]
    df_s, dr_s, n_df, n_dr = _segments(plan_f)
    assert torch.equal(plan_u.scores, plan_f.scores)
    per_u = rankeval.subset_auc_ap(df_s, dr_s, plan_u.subsets)
    per_f = rankeval.subset_auc_ap(df_s, dr_s, subsets.draw(plan_f.subset_seed, 0, N_SUBSETS, n_df, n_dr))
    for name, at, u, f in (('df_auc', 3, per_u[0], per_f[0]), ('df_aup', 4, per_u[1], per_f[1])):
        assert u.numel() == f.numel() == N_SUBSETS
        assert a[at] == float(u.mean()) and b[at] == float(f.mean())             # the per-subset values ARE the paths' own
        s_u, s_f = float(u.std(unbiased=False)), float(f.std(unbiased=False))
        bound = 6.0 * math.sqrt((s_f ** 2 + s_u ** 2) / N_SUBSETS)
        print(gnn, nr, name, 'device', b[at], 'upstream', a[at], 'difference', abs(b[at] - a[at]), 'bound', bound, 's_f', s_f, 's_u', s_u)
        assert s_u > 0.0 and s_f > 0.0
        assert abs(b[at] - a[at]) <= bound


# ---------------------------------------------------------------------------------------------- the host random stream
def test_above_the_threshold_the_host_stream_is_the_unflagged_one(tmp_path):
    model = _model('rgcn', 5)
    plain, a, state_a = _eval(tmp_path / 'u', 5, model=model, fast_above=0, fused_validation=True)
    tr, b, state_b = _eval(tmp_path / 'f', 5, model=model, fast_above=0, fused_validation=True, device_subsets=True)
    assert tr.trainer_log['subset_draw'] == 'device' and tr._validation_plans[('kg', 'val')].subsets is None
    assert torch.equal(state_a, state_b)
    torch.manual_seed(11)
    assert not torch.equal(torch.get_rng_state(), state_a)           # (the validation did draw from it)
    assert _all_but_the_df_ranking(a, 'val') == _all_but_the_df_ranking(b, 'val')


def test_at_the_default_threshold_the_stream_differs_and_the_run_repeats(tmp_path):
    model = _model('rgcn', 5)
    _, a, state_a = _eval(tmp_path / 'u', 5, model=model, fused_validation=True)
    _, b, state_b = _eval(tmp_path / 'f', 5, model=model, fused_validation=True, device_subsets=True)
    _, c, state_c = _eval(tmp_path / 'g', 5, model=model, fused_validation=True, device_subsets=True)
    assert not torch.equal(state_a, state_b)                         # one randint instead of 500 randperms
    assert torch.equal(state_b, state_c) and _same(b, c)


def _node_sets(data, count=3, size=150):
    g = torch.Generator().manual_seed(9)
    df_nodes = data.directed_df_edge_index.flatten().unique()
    return [torch.cat([df_nodes, torch.randperm(data.num_nodes, generator=g)[:size]]).unique() for _ in range(count)]


def _train(path, nr, **flags):
    from gnndelete_amd.framework.trainer import kg as TK
    data, model = _request(nr), _model('rgcn', nr)
    args = _args(path, nr, **flags)
    opt = [torch.optim.Adam(model.deletion1.parameters(), lr=args.lr), torch.optim.Adam(model.deletion2.parameters(), lr=args.lr)]
    tr = TK.KGGNNDeleteNodeembTrainer(args)
    torch.manual_seed(21)
    tr.train(model, data, opt, args)
    return tr, model


@pytest.mark.parametrize('fullgraph', [False, True])
def test_through_the_loops_the_training_does_not_move(fullgraph, tmp_path, monkeypatch):
    """KGGNNDeleteNodeembTrainer.train on three injected node sets, two epochs, a validation after each, and the same through
    --fullgraph, with FAST_SUBSETS_ABOVE = 0: the steps / the loss history are the --fused_validation run's to the bit, because
    the validation leaves the host random stream where that run leaves it."""
    from gnndelete_amd.framework.trainer import sampler as S
    from gnndelete_amd.framework.trainer.base import Trainer
    sets = _node_sets(_prepared(5))
    monkeypatch.setattr(S, 'make_sampler', lambda d, batch_size, num_steps, walk_length=2: S.FixedNodeSets(d, sets))
    monkeypatch.setattr(Trainer, 'FAST_SUBSETS_ABOVE', 0)
    extra = dict(fullgraph=True) if fullgraph else {}
    plain, m_a = _train(tmp_path / 'u', 5, fused_validation=True, **extra)
    tr, m_b = _train(tmp_path / 'f', 5, fused_validation=True, device_subsets=True, **extra)
    assert tr.trainer_log['validation_path'] == 'prepared' and tr.trainer_log['subset_draw'] == 'device'
    assert tr._validation_plans[('kg', 'val')].subsets is None and 'subset_draw' not in plain.trainer_log
    if fullgraph:
        assert len(tr.trainer_log['loss_history']) >= 2 and tr.trainer_log['loss_history'] == plain.trainer_log['loss_history']
    else:
        assert len(tr.trainer_log['steps']) == 6 and tr.trainer_log['steps'] == plain.trainer_log['steps']
    assert torch.equal(m_a.deletion1.deletion_weight, m_b.deletion1.deletion_weight) and torch.equal(m_a.deletion2.deletion_weight, m_b.deletion2.deletion_weight)
    vals_a = [r for r in plain.trainer_log['log'] if 'val_dt_auc' in r]
    vals_b = [r for r in tr.trainer_log['log'] if 'val_dt_auc' in r]
    assert len(vals_a) == len(vals_b) == 2
    for ra, rb in zip(vals_a, vals_b):
        assert [rb[f'val_{k}'] for k in ('loss', 'dt_auc', 'dt_aup', 'df_logit_mean', 'df_logit_std')] == \
               [ra[f'val_{k}'] for k in ('loss', 'dt_auc', 'dt_aup', 'df_logit_mean', 'df_logit_std')]
        assert 0.0 < rb['val_df_auc'] < 1.0


# ---------------------------------------------------------------------------------------------- fallbacks
def test_without_fused_validation_the_flag_changes_nothing(tmp_path, capsys):
    model = _model('rgcn', 5)
    _, a, state_a = _eval(tmp_path / 'u', 5, model=model)
    tr, b, state_b = _eval(tmp_path / 'f', 5, model=model, device_subsets=True)
    assert tr.trainer_log['subset_draw'] == 'upstream: --fused_validation is missing' and 'validation_path' not in tr.trainer_log
    assert _same(a, b) and torch.equal(state_a, state_b)
    assert capsys.readouterr().out.count('--device_subsets: --fused_validation is missing; drawing the validation subsets as upstream does') == 1


def test_a_pool_under_32_keeps_upstreams_draw(tmp_path):
    """10 deleted triples and a Dr cut to 25 (and their reverse edges, for the message passing)."""
    data = _request(5, n_df=10)
    half_n = data.dr_mask.shape[0] // 2
    keep = data.dr_mask[:half_n].nonzero().flatten()[:25]
    mask = torch.zeros_like(data.dr_mask)
    mask[keep] = True
    mask[keep + half_n] = True
    data.dr_mask = mask
    model = _model('rgcn', 5, n_df=10)
    plain, a, state_a = _eval(tmp_path / 'u', 5, model=model, data=data.clone(), fused_validation=True)
    tr, b, state_b = _eval(tmp_path / 'f', 5, model=model, data=data.clone(), fused_validation=True, device_subsets=True)
    assert plain.trainer_log['validation_path'] == tr.trainer_log['validation_path'] == 'prepared'
    assert tr._validation_plans[('kg', 'val')].segments[2:] == (10, 25)
    assert tr.trainer_log['subset_draw'] == 'upstream: a pool of 25 scores (the subset stream takes 32 and more)'
    assert tuple(tr._validation_plans[('kg', 'val')].subsets.shape) == (N_SUBSETS, 10)
    assert _same(a, b) and torch.equal(state_a, state_b)


def test_a_model_the_prepared_pass_refuses_keeps_upstreams_draw(tmp_path):
    model = copy.deepcopy(_model_state('rgcn', 5, 6)).cuda()         # out_dim = 6: no multiple of 4
    _, a, state_a = _eval(tmp_path / 'p', 5, model=model)
    _, u, state_u = _eval(tmp_path / 'u', 5, model=model, fused_validation=True)
    tr, b, state_b = _eval(tmp_path / 'f', 5, model=model, fused_validation=True, device_subsets=True)
    assert tr.trainer_log['validation_path'] == 'torch: DistMult width 6 (a multiple of 4 up to 256)'
    assert tr.trainer_log['subset_draw'] == 'upstream: the prepared pass fell back (DistMult width 6 (a multiple of 4 up to 256))'
    assert _same(a, b) and _same(u, b) and torch.equal(state_a, state_b) and torch.equal(state_u, state_b)


# ---------------------------------------------------------------------------------------------- the link trainer
@functools.lru_cache(maxsize=None)
def _link_request():
    """synth-tiny prepared as delete_gnn.py prepares an edge deletion, and one GCN with weights large enough that some scores
    saturate; shared, changed by none."""
    from gnndelete_amd.framework import get_model
    from gnndelete_amd.framework.data import Data, prepare_edge_deletion
    from gnndelete_amd.framework.synth import make_linkpred_dataset
    data, df_masks = make_linkpred_dataset('synth-tiny', 42)
    data = Data({k: (v.clone() if torch.is_tensor(v) else v) for k, v in data.items()})
    torch.manual_seed(7)
    prepare_edge_deletion(data, df_masks['in'], 60)
    data.dtrain_mask = data.dr_mask
    model = get_model(SimpleNamespace(unlearning_model='retrain', gnn='gcn', in_dim=32, hidden_dim=64, out_dim=32)).cuda()
    with torch.no_grad():
        for p in model.parameters():
            p.mul_(3.0)
    return data, model


def _link_eval(path, seed=11, **flags):
    from gnndelete_amd.framework.trainer.base import Trainer
    os.makedirs(str(path), exist_ok=True)
    data, model = _link_request()
    tr = Trainer(SimpleNamespace(unlearning_model='retrain', gnn='gcn', dataset='synth-tiny', checkpoint_dir=str(path), eval_on_cpu=False,
                                 in_dim=32, hidden_dim=64, out_dim=32, epochs=1, valid_freq=1, lr=1e-2, random_seed=42, **flags))
    torch.manual_seed(seed)
    return tr, tr.eval(model, data, 'val'), data, model


def test_the_link_plan_holds_a_seed_and_no_index_matrix(tmp_path):
    from gnndelete_amd import rankeval, subsets
    from gnndelete_amd.framework.metrics import batched_average_precision, batched_roc_auc
    plain, a, _, _ = _link_eval(tmp_path / 'u', fused_validation=True)
    tr, b, data, model = _link_eval(tmp_path / 'f', fused_validation=True, device_subsets=True)
    state_b = torch.get_rng_state()
    assert tr.trainer_log['validation_path'] == 'prepared' and tr.trainer_log['subset_draw'] == 'device'
    plan = tr._validation_plans[('link', 'val')]
    assert plan.drawn and plan.subset_index is None and plan.subset_seed == _seed_of(11)
    assert '_df_subset_index' not in tr.__dict__ and tr.df_pos_edge == []                     # the trainer's own draw is untouched
    assert plain._df_subset_index is not None and len(plain.df_pos_edge) == N_SUBSETS
    df_s, dr_s, n_df, n_dr = _segments(plan)
    assert n_df > 0 and n_dr >= 32
    # everything but the Df ranking is the --fused_validation value; the Df ranking is the stream's subsets on the plan's scores
    assert _all_but_the_df_ranking(a, 'val') == _all_but_the_df_ranking(b, 'val')
    idx = subsets.draw(plan.subset_seed, 0, N_SUBSETS, n_df, n_dr)
    scores = torch.cat([df_s[None].expand(N_SUBSETS, n_df), dr_s[idx]], dim=1)
    labels = torch.cat([torch.zeros(n_df), torch.ones(n_df)]).cuda()
    assert b[3] == float(batched_roc_auc(scores, labels).mean()) == b[7]['val_df_auc']
    assert abs(b[4] - float(batched_average_precision(scores, labels).mean())) <= AP_TOL and b[4] == b[7]['val_df_aup']
    # six standard errors between the two draws, both deviations measured on the plan's scores
    per_u = rankeval.subset_auc_ap(df_s, dr_s, plain._df_subset_index)
    per_f = rankeval.subset_auc_ap(df_s, dr_s, idx)
    for name, at, u, f in (('df_auc', 3, per_u[0], per_f[0]), ('df_aup', 4, per_u[1], per_f[1])):
        bound = 6.0 * math.sqrt((float(f.std(unbiased=False)) ** 2 + float(u.std(unbiased=False)) ** 2) / N_SUBSETS)
        print('link', name, 'device', b[at], 'upstream', a[at], 'difference', abs(b[at] - a[at]), 'bound', bound)
        assert abs(b[at] - a[at]) <= bound
    # a second validation of the request: the same plan, the same seed, the same subsets, no further host draw
    second = tr.eval(model, data, 'val')
    assert tr._validation_plans[('link', 'val')] is plan and plan.subset_seed == _seed_of(11)
    assert _same(second, b) and torch.equal(torch.get_rng_state(), state_b)
    assert '_df_subset_index' not in tr.__dict__ and tr.df_pos_edge == []
