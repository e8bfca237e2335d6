"""--fused_validation through KGTrainer.eval (gnndelete_amd/evalpass.py: KGValidationPlan, prepared_kg_validation) on the
requests of tests/test_engine_gpu.py::_kg_request: 700 nodes, 5,000 triples, 60 deleted, once with 5 relation types (dense
relation weights) and once with 25 (block-diagonal); RGCNDelete and one RGATDelete case, widths 32 -> 32 -> 32, weights scaled so
that some Df / Dr scores saturate.

Under the flag the scores are the scoring kernel's own, so the values are held to what they are derived from: z is the model's
forward on the plan's triples to the bit; the AUCs are metrics.batched_roc_auc on the plan's scores to the bit (the stage on its
raw logits, Df-versus-Dr under the plan's latest subsets), the AUPs within 1e-12; loss / Df mean / Df std within 1e-12 relative
of reference_triple_stats on those scores; df_logit is the Df segment.  The 500 subsets and the host generator's state after the
call are the no-flag path's under the same seed, on the host-draw branch and (FAST_SUBSETS_ABOVE = 0) on the device-draw branch.
The golden fixture of tests/test_cli_gpu.py holds the flag to the reference's values with that test's tolerances.  Typed graphs
are counted: one per plan instead of one per conv per validation, none after other graphs or a host round trip, one after an
in-place edit.  Through the batch loop and the --fullgraph loop the training is the no-flag run's to the bit and one plan is
built.  What the pass does not take falls back to the no-flag tuple."""
import copy
import functools
import math
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from helpers import hip_model, load_golden, split_fixture

pytestmark = pytest.mark.gpu
AP_TOL = 1e-12
SUM_TOL = 1e-12
KEYS = ('loss', 'dt_auc', 'dt_aup', 'df_auc', 'df_aup', 'df_logit_mean', 'df_logit_std')


def _args(path, nr, kind='gnndelete_nodeemb', gnn='rgcn', **flags):
    os.makedirs(str(path), exist_ok=True)
    return SimpleNamespace(unlearning_model=kind, gnn=gnn, dataset='synth-kg-tiny', checkpoint_dir=str(path), eval_on_cpu=False,
                           in_dim=32, hidden_dim=32, out_dim=32, epochs=2, valid_freq=1, lr=1e-2, alpha=0.5, loss_fct='mse_mean',
                           loss_type='both_layerwise', batch_size=30, num_steps=3, num_edge_type=nr, random_seed=42, **flags)


@functools.lru_cache(maxsize=None)
def _prepared(nr):
    """tests/test_engine_gpu.py::_kg_request(700, 5000, nr, seed=3, n_df=60); shared, changed by none (every test clones it)."""
    from gnndelete_amd.framework.data import prepare_edge_deletion
    from gnndelete_amd.framework.synth import make_kg_dataset
    data, dfm = make_kg_dataset(None, seed=3, shape=(700, nr, 5000))
    torch.manual_seed(3)
    prepare_edge_deletion(data, dfm['in'], 60, True, nr)
    return data


def _request(nr):
    return _prepared(nr).clone()


@functools.lru_cache(maxsize=None)
def _model_state(gnn, nr, out_dim=32):
    from gnndelete_amd.framework import models as M
    data = _prepared(nr)
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


def _model(gnn, nr, out_dim=32):
    return copy.deepcopy(_model_state(gnn, nr, out_dim)).cuda()


def _eval(path, nr, gnn='rgcn', kind='gnndelete_nodeemb', stage='val', data=None, model=None, fast_above=None, seed=11, **flags):
    from gnndelete_amd.framework.trainer.kg import KGTrainer
    tr = KGTrainer(_args(path, nr, kind, gnn, **flags))
    if fast_above is not None:
        tr.FAST_SUBSETS_ABOVE = fast_above
    torch.manual_seed(seed)
    out = tr.eval(_model(gnn, nr) if model is None else model, _request(nr) if data is None else data, stage)
    return tr, out, torch.get_rng_state()


def _same(a, b):
    """Two KGTrainer.eval tuples equal to the bit (NaN equal to NaN)."""
    eq = lambda x, y: x == y or (isinstance(x, float) and isinstance(y, float) and math.isnan(x) and math.isnan(y))       # noqa: E731
    return (all(eq(float(x), float(y)) for x, y in zip(a[:5], b[:5])) and a[5] == b[5] and a[6] is None and b[6] is None and
            list(a[7]) == list(b[7]) and all(eq(float(a[7][k]), float(b[7][k])) for k in a[7]))


def _check_against_the_scores(tr, out, stage, model, data):
    from gnndelete_amd.evalpass import reference_triple_stats
    from gnndelete_amd.framework.metrics import batched_average_precision, batched_roc_auc
    plan = tr._validation_plans[('kg', stage)]
    loss, dt_auc, dt_aup, df_auc, df_aup, df_logit, all_pairs, log = out
    n_pos, n_neg, n_df, n_dr = plan.segments
    n_stage = n_pos + n_neg
    with torch.no_grad():
        assert torch.equal(plan.z, model(data.x, plan.edges, plan.types))
    assert torch.equal(plan.edges, data.edge_index[:, data.dr_mask]) and torch.equal(plan.types, data.edge_type[data.dr_mask])
    s = plan.scores
    label = torch.cat([torch.ones(n_pos), torch.zeros(n_neg)]).cuda()
    assert dt_auc == float(batched_roc_auc(s[:n_stage], label)[0])
    assert abs(dt_aup - float(batched_average_precision(s[:n_stage], label)[0])) <= AP_TOL
    want_loss, want_mean, want_std = reference_triple_stats(s, plan.segments)
    print(stage, 'loss', loss, want_loss, 'df mean', log[f'{stage}_df_logit_mean'], want_mean, 'df std', log[f'{stage}_df_logit_std'], want_std,
          '| stage logits in', float(s[:n_stage].min()), float(s[:n_stage].max()))
    assert abs(loss - want_loss) <= SUM_TOL * abs(want_loss)
    assert list(log) == [f'{stage}_{k}' for k in KEYS]
    assert [log[f'{stage}_{k}'] for k in KEYS[:5]] == [loss, dt_auc, dt_aup, df_auc, df_aup] or n_df == 0
    assert all(type(v) is float for v in (loss, dt_auc, dt_aup)) and all_pairs is None and 0.0 < dt_auc < 1.0
    if n_df == 0:
        assert df_logit == [] and all(math.isnan(v) for v in (df_auc, df_aup, log[f'{stage}_df_logit_mean'], log[f'{stage}_df_logit_std']))
        return
    df_s, dr_s = s[n_stage:n_stage + n_df], s[n_stage + n_df:]
    assert isinstance(df_logit, list) and df_logit == df_s.tolist()
    assert abs(log[f'{stage}_df_logit_mean'] - want_mean) <= SUM_TOL * abs(want_mean) and abs(log[f'{stage}_df_logit_std'] - want_std) <= SUM_TOL * want_std
    idx = plan.subsets
    assert tuple(idx.shape) == (500, n_df) and idx.dtype == torch.int64 and int(idx.min()) >= 0 and int(idx.max()) < n_dr
    scores = torch.cat([df_s[None].expand(500, n_df), dr_s[idx]], dim=1)
    labels = torch.cat([torch.zeros(n_df), torch.ones(n_df)]).cuda()
    assert df_auc == float(batched_roc_auc(scores, labels).mean()) == log[f'{stage}_df_auc']
    assert abs(df_aup - float(batched_average_precision(scores, labels).mean())) <= AP_TOL and df_aup == log[f'{stage}_df_aup']
    assert 0.0 < df_auc < 1.0
    saturated = int((dr_s == 1.0).sum() + (df_s == 1.0).sum()), int((dr_s < 1e-6).sum() + (df_s < 1e-6).sum())
    print(stage, 'scores exactly 1:', saturated[0], 'below 1e-6:', saturated[1])
    assert saturated[0] > 0 and saturated[1] > 0


@pytest.fixture
def typed_builds(monkeypatch):
    from gnndelete_amd import graph
    built = []
    init = graph.TypedNodeCSR.__init__

    def counted(self, *a, **k):
        built.append(1)
        return init(self, *a, **k)
    monkeypatch.setattr(graph.TypedNodeCSR, '__init__', counted)
    return built


@pytest.mark.parametrize('gnn, nr, stage', [('rgcn', 5, 'val'), ('rgcn', 25, 'test'), ('rgat', 5, 'val')])
def test_a_prepared_kg_validation_is_derived_from_its_scores(gnn, nr, stage, tmp_path, capsys):
    data, model = _request(nr), _model(gnn, nr)
    plain, a, _ = _eval(tmp_path / 'p', nr, gnn, stage=stage, data=_request(nr), model=model)
    tr, b, _ = _eval(tmp_path / 'f', nr, gnn, stage=stage, data=data, model=model, fused_validation=True)
    assert '--fused_validation:' not in capsys.readouterr().out      # no fallback line
    assert tr.trainer_log['validation_path'] == 'prepared' and 'validation_path' not in plain.trainer_log
    plan = tr._validation_plans[('kg', stage)]
    half = data.dr_mask[:data.dr_mask.shape[0] // 2]
    assert plan.segments == (data[f'{stage}_pos_edge_index'].shape[1], data[f'{stage}_neg_edge_index'].shape[1], 60, int(half.sum()))
    assert torch.equal(plan.decoded, torch.cat([data[f'{stage}_pos_edge_index'], data[f'{stage}_neg_edge_index'], data.directed_df_edge_index,
                                                data.train_pos_edge_index[:, half]], 1))
    et = data[f'{stage}_edge_type']
    assert torch.equal(plan.etype, torch.cat([et, et, data.directed_df_edge_type, data.train_edge_type[half]]))
    _check_against_the_scores(tr, b, stage, model, data)
    # the no-flag path beside it (printed, not held: the kernel's sigmoid is not torch's, the decode may differ in a last bit)
    print(stage, 'no flag', a[:5], 'prepared', b[:5], 'largest df_logit difference', np.abs(np.array(a[5]) - np.array(b[5])).max())
    assert list(a[7]) == list(b[7])                                  # the seven log keys in eval's order
    np.testing.assert_allclose(b[:5], a[:5], rtol=1e-2)              # (sanity only: the same quantities)


@pytest.mark.parametrize('fast_above', [None, 0])
def test_the_same_seed_gives_the_same_subsets_and_random_stream(fast_above, tmp_path, monkeypatch):
    """Once as is (500 host permutations), once with FAST_SUBSETS_ABOVE = 0 on the trainer instances (one host randint seeding
    500 device permutations): the no-flag path's picks, recorded at its ranking, are the plan's subsets, and the host generator
    is left in the same state."""
    from gnndelete_amd.framework.trainer import kg as TK
    picked = []
    real = TK.batched_roc_auc

    def recording(scores, labels):
        picked.append(scores)
        return real(scores, labels)
    monkeypatch.setattr(TK, 'batched_roc_auc', recording)
    model = _model('rgcn', 5)
    plain, a, state_a = _eval(tmp_path / 'p', 5, model=model, fast_above=fast_above)
    tr, b, state_b = _eval(tmp_path / 'f', 5, model=model, fast_above=fast_above, fused_validation=True)
    assert tr.trainer_log['validation_path'] == 'prepared' and len(picked) == 2        # the stage and the 500 rows, of the no-flag call
    assert torch.equal(state_a, state_b)
    torch.manual_seed(11)
    assert not torch.equal(torch.get_rng_state(), state_a)           # (the validation did draw from it)
    plan = tr._validation_plans[('kg', 'val')]
    n_pos, n_neg, n_df, n_dr = plan.segments
    # the no-flag path ranked [Df | Dr[picks]] rows of torch's scores; the plan's subsets select the same Dr entries
    with torch.no_grad():
        z = model(plan_x := _request(5).x.cuda(), plan.edges, plan.types)
        dr = model.decode(z, plan.decoded[:, n_pos + n_neg + n_df:], plan.etype[n_pos + n_neg + n_df:]).sigmoid()
    assert plan_x.shape[0] == 700 and torch.equal(picked[1][:, n_df:], dr[plan.subsets])
    if fast_above is None:
        assert bool((plan.subsets[:, 1:] > plan.subsets[:, :-1]).all())      # upstream's sorted host picks
    # and a second validation draws fresh subsets, as upstream does
    first = plan.subsets
    torch.set_rng_state(state_b)                                     # (the stream as the first validation left it)
    tr.eval(model, _request(5), 'val')
    assert tr._validation_plans[('kg', 'val')] is plan and not torch.equal(plan.subsets, first)


def test_the_golden_fixture_under_the_flag(tmp_path):
    """tests/test_cli_gpu.py::test_kg_eval_matches_reference_golden with the flag: the reference's values, that test's tolerances."""
    from gnndelete_amd.framework.data import Data
    from gnndelete_amd.framework.trainer import kg as TK
    fx = load_golden('eval_kg.npz')
    state, data, rest = split_fixture(fx)
    R_ = int(rest['num_edge_type'])
    m = hip_model('rgcn', state, data['sdf_node_1hop_mask'], data['sdf_node_2hop_mask'], num_nodes=data['num_nodes'], num_edge_type=R_)
    args = SimpleNamespace(unlearning_model='gnndelete_nodeemb', dataset='WordNet18', checkpoint_dir=str(tmp_path), eval_on_cpu=False,
                           num_edge_type=R_, fused_validation=True)
    tr = TK.KGTrainer(args)
    torch.manual_seed(int(rest['eval_seed']))
    loss, dt_auc, dt_aup, df_auc, df_aup, df_logit, _, log = tr.eval(m, Data(data), 'test')
    assert tr.trainer_log['validation_path'] == 'prepared'
    print('loss', loss, float(rest['test_loss']), 'dt', dt_auc, float(rest['test_dt_auc']), dt_aup, float(rest['test_dt_aup']),
          'df', df_auc, float(rest['test_df_auc']), df_aup, float(rest['test_df_aup']))
    assert abs(loss - float(rest['test_loss'])) < 1e-4
    assert abs(dt_auc - float(rest['test_dt_auc'])) < 2e-3 and abs(dt_aup - float(rest['test_dt_aup'])) < 2e-3
    assert abs(df_auc - float(rest['test_df_auc'])) < 2e-3 and abs(df_aup - float(rest['test_df_aup'])) < 2e-3
    np.testing.assert_allclose(np.array(df_logit), rest['test_df_logit'], rtol=1e-4)


def test_typed_graphs_are_built_once(tmp_path, typed_builds):
    from gnndelete_amd import graph
    from gnndelete_amd.framework.trainer.kg import KGTrainer
    nr = 5
    model, data = _model('rgcn', nr), _request(nr)
    # without the flag: one typed graph per conv on every validation
    plain = KGTrainer(_args(tmp_path / 'p', nr))
    plain.eval(model, _request(nr), 'val')
    assert len(typed_builds) == 2
    plain.eval(model, _request(nr), 'val')
    assert len(typed_builds) == 4
    del typed_builds[:]
    tr = KGTrainer(_args(tmp_path / 'f', nr, fused_validation=True))
    first = tr.eval(model, data, 'val')
    plan = tr._validation_plans[('kg', 'val')]
    assert len(typed_builds) == 1 and graph.TYPED.pinned(plan.edges, plan.types)         # ONE graph for conv1 and conv2
    # ten other typed graphs go through the model (each displaces the convs' one slot)
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():
        for _ in range(10):
            ei = torch.randint(0, data.num_nodes, (2, 300), generator=g).cuda()
            model(data.x, ei, torch.randint(0, 2 * nr, (300,), generator=g).cuda())
    assert len(typed_builds) == 1 + 20
    second = tr.eval(model, data, 'val')
    assert len(typed_builds) == 21 and tr._validation_plans[('kg', 'val')] is plan
    assert second[0] == first[0] and second[1:3] == first[1:3] and second[5] == first[5]        # (the subsets are fresh: Df AUC / AUP move)
    # the mini-batch loops' round trip: every tensor is a new one of equal contents
    key = plan.key
    data = data.to('cpu')
    third = tr.eval(model, data, 'val')
    assert len(typed_builds) == 21 and tr._validation_plans[('kg', 'val')] is plan and plan.key != key
    assert third[0] == first[0] and third[5] == first[5] and all(s is data[k] for s, k in zip(plan._sources, ('edge_index', 'edge_type', 'dr_mask')))
    # an in-place edit of data.edge_type: a new plan, a new graph, the old pair unpinned
    flip = int(data.dr_mask.nonzero()[0])
    data.edge_type[flip] = (data.edge_type[flip] + 1) % (2 * nr)
    fourth = tr.eval(model, data, 'val')
    new_plan = tr._validation_plans[('kg', 'val')]
    assert len(typed_builds) == 22 and new_plan is not plan and not graph.TYPED.pinned(plan.edges, plan.types)
    assert graph.TYPED.pinned(new_plan.edges, new_plan.types) and int(new_plan.types[0]) != int(plan.types[0])
    assert tr.trainer_log['validation_path'] == 'prepared' and np.isfinite(fourth[0])
    new_plan.release()
    assert not graph.TYPED.pinned(new_plan.edges, new_plan.types)


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
    """KGGNNDeleteNodeembTrainer.train on three injected node sets, two epochs, a validation after each (the batch loop moves
    the data to the host in between), and the same through --fullgraph: the steps / the loss history are the no-flag run's to
    the bit - the validation leaves the host random stream where the no-flag path leaves it - and ONE plan is built."""
    from gnndelete_amd import evalpass
    from gnndelete_amd.framework.trainer import sampler as S
    sets = _node_sets(_prepared(5))
    monkeypatch.setattr(S, 'make_sampler', lambda d, batch_size, num_steps, walk_length=2: S.FixedNodeSets(d, sets))
    plans = []
    init = evalpass.KGValidationPlan.__init__

    def counted(self, *a, **k):
        plans.append(1)
        return init(self, *a, **k)
    monkeypatch.setattr(evalpass.KGValidationPlan, '__init__', counted)
    extra = dict(fullgraph=True) if fullgraph else {}
    plain, m_a = _train(tmp_path / 'p', 5, **extra)
    assert plans == [] and 'validation_path' not in plain.trainer_log
    tr, m_b = _train(tmp_path / 'f', 5, fused_validation=True, **extra)
    assert tr.trainer_log['validation_path'] == 'prepared' and plans == [1]
    if fullgraph:
        assert len(tr.trainer_log['loss_history']) >= 2 and tr.trainer_log['loss_history'] == plain.trainer_log['loss_history']
    else:
        assert len(tr.trainer_log['steps']) == 6 and tr.trainer_log['steps'] == plain.trainer_log['steps']
    assert torch.equal(m_a.deletion1.deletion_weight, m_b.deletion1.deletion_weight) and torch.equal(m_a.deletion2.deletion_weight, m_b.deletion2.deletion_weight)
    vals_a = [r for r in plain.trainer_log['log'] if 'val_dt_auc' in r]
    vals_b = [r for r in tr.trainer_log['log'] if 'val_dt_auc' in r]
    assert len(vals_a) == len(vals_b) == 2 and [list(r) for r in vals_a] == [list(r) for r in vals_b]
    print('no flag', vals_a[-1], 'prepared', vals_b[-1])
    for ra, rb in zip(vals_a, vals_b):
        np.testing.assert_allclose([rb[f'val_{k}'] for k in KEYS], [ra[f'val_{k}'] for k in KEYS], rtol=1e-2)


def test_what_the_pass_does_not_take_falls_back_to_the_no_flag_values(tmp_path, capsys):
    from gnndelete_amd import evalpass
    from gnndelete_amd.framework import get_model
    from gnndelete_amd.framework.trainer.kg import KGTrainer
    # out_dim = 6: no multiple of 4
    model = copy.deepcopy(_model_state('rgcn', 5, 6)).cuda()
    _, a, state_a = _eval(tmp_path / 'p', 5, model=model)
    tr, b, state_b = _eval(tmp_path / 'f', 5, model=model, fused_validation=True)
    assert _same(a, b) and torch.equal(state_a, state_b)
    assert tr.trainer_log['validation_path'] == 'torch: DistMult width 6 (a multiple of 4 up to 256)' and '_validation_plans' not in tr.__dict__
    assert capsys.readouterr().out.count('--fused_validation: DistMult width 6 (a multiple of 4 up to 256); validating on the torch path') == 1
    # a homogeneous model handed to the hook
    gcn = get_model(SimpleNamespace(unlearning_model='retrain', gnn='gcn', in_dim=32, hidden_dim=32, out_dim=32)).cuda()
    tr = KGTrainer(_args(tmp_path / 'g', 5, fused_validation=True))
    assert evalpass.prepared_kg_validation(tr, gcn, _request(5).to('cuda'), 'val', False, torch.device('cuda')) is None
    assert tr.trainer_log['validation_path'].startswith('torch: no prepared knowledge-graph validation for the GCN model')


def test_original_ranks_only_the_stage(tmp_path):
    model = _model('rgcn', 5)
    _, a, _ = _eval(tmp_path / 'p', 5, kind='original', model=model)
    data = _request(5)
    tr, b, _ = _eval(tmp_path / 'f', 5, kind='original', model=model, data=data, fused_validation=True)
    plan = tr._validation_plans[('kg', 'val')]
    assert tr.trainer_log['validation_path'] == 'prepared' and plan.segments[2:] == (0, 0) and plan.subsets is None
    assert b[5] == [] and all(math.isnan(v) for v in (b[3], b[4], b[7]['val_df_logit_mean'], b[7]['val_df_logit_std']))
    assert a[5] == [] and math.isnan(a[3]) and list(a[7]) == list(b[7])
    _check_against_the_scores(tr, b, 'val', model, data)
    np.testing.assert_allclose(b[:3], a[:3], rtol=1e-2)
