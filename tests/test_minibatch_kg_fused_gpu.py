"""The fused knowledge-graph batch step (gnndelete_amd.minibatch.MinibatchKGNodeembStep, delete_gnn.py --gnn rgcn
--fused_minibatch): the reference's trajectory, the autograd batch loop on a second request, and the fall-backs."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from helpers import hip_model, load_golden, rel_l2, split_fixture, t

pytestmark = pytest.mark.gpu


def _lists(fx, prefix, count_key):
    return [t(fx[f'{prefix}::{i}']) for i in range(int(fx[count_key]))]


def _fixture():
    fx = load_golden('traj_kg_rgcn.npz')
    state, data, rest = split_fixture(fx)
    return fx, state, data, rest, int(rest['num_edge_type'])


def _args(tmp_path, rest, R_, sets, **kw):
    epochs = int(rest['epochs'])
    base = dict(unlearning_model='gnndelete_nodeemb', dataset='WordNet18', checkpoint_dir=str(tmp_path), eval_on_cpu=False,
                epochs=epochs, valid_freq=epochs, lr=float(rest['lr']), alpha=float(rest['alpha']), loss_fct='mse_mean',
                loss_type='both_layerwise', gnn='rgcn', batch_size=30, num_steps=len(sets), num_edge_type=R_, fused_minibatch=True)
    base.update(kw)
    return SimpleNamespace(**base)


def test_fused_kg_step_reproduces_reference_trajectory(tmp_path, monkeypatch):
    """test_cli_gpu.py::test_kg_trainer_reproduces_reference_trajectory with fused_minibatch=True: the reference's batches,
    negative_sampling_kg and the closing validation's subsets re-drawn from the recorded seed; same assertions and bounds."""
    from gnndelete_amd.framework.data import Data
    from gnndelete_amd.framework.trainer import kg as TK
    from gnndelete_amd.framework.trainer import sampler as S
    fx, state, data, rest, R_ = _fixture()
    m = hip_model('rgcn', state, data['sdf_node_1hop_mask'], data['sdf_node_2hop_mask'], num_nodes=data['num_nodes'],
                  num_edge_type=R_)
    sets = _lists(fx, 'batch', 'n_batches')
    monkeypatch.setattr(S, 'make_sampler', lambda d, batch_size, num_steps, walk_length=2: S.FixedNodeSets(d, sets))
    args = _args(tmp_path, rest, R_, sets)
    opt = [torch.optim.Adam(m.deletion1.parameters(), lr=args.lr), torch.optim.Adam(m.deletion2.parameters(), lr=args.lr)]
    tr = TK.KGGNNDeleteNodeembTrainer(args)
    torch.manual_seed(int(rest['seed']))
    tr.train(m, Data(data), opt, args)
    assert tr.trainer_log['minibatch_step'] == 'fused'
    steps = tr.trainer_log['steps']
    assert len(steps) == len(rest['train_loss'])
    for key in ['train_loss', 'loss_r', 'loss_l']:
        np.testing.assert_allclose([s_[key] for s_ in steps], rest[key], rtol=1e-4, atol=1e-8, err_msg=key)
    assert rel_l2(m.deletion1.deletion_weight.detach().cpu(), rest['final_w1']) < 1e-4
    assert rel_l2(m.deletion2.deletion_weight.detach().cpu(), rest['final_w2']) < 1e-4
    vals = [r for r in tr.trainer_log['log'] if 'val_dt_auc' in r]
    assert abs(vals[-1]['val_loss'] - float(rest['val_loss'][-1])) < 1e-4
    assert abs(vals[-1]['val_dt_auc'] - float(rest['val_dt_auc'][-1])) < 2e-3
    assert abs(vals[-1]['val_df_auc'] - float(rest['val_df_auc'][-1])) < 2e-3
    assert tr._fused_minibatch_step.cut.reads == len(steps)          # one blocking host read per batch


def _small_sets(data):
    """Four batches of 30 nodes: three random ones holding Df endpoints, one of nodes no Df edge touches."""
    n = int(data['num_nodes'])
    g = torch.Generator().manual_seed(21)
    df_nodes = data['directed_df_edge_index'].flatten().unique()
    touched = torch.zeros(n, dtype=torch.bool)
    touched[data['edge_index'][:, data['df_mask']].flatten()] = True
    touched[df_nodes] = True
    sets = []
    for _ in range(3):
        pick = torch.cat([df_nodes[torch.randperm(df_nodes.numel(), generator=g)[:14]], torch.randperm(n, generator=g)[:30]])
        sets.append(pick.unique()[:30].sort().values)
    sets.insert(2, (~touched).nonzero().flatten()[:30])
    return sets


def _run_small(tmp_path, monkeypatch, fused, **kw):
    from gnndelete_amd.framework.data import Data
    from gnndelete_amd.framework.trainer import kg as TK
    from gnndelete_amd.framework.trainer import sampler as S
    fx, state, data, rest, R_ = _fixture()
    m = kw.pop('model', None) or hip_model('rgcn', state, data['sdf_node_1hop_mask'], data['sdf_node_2hop_mask'],
                                           num_nodes=data['num_nodes'], num_edge_type=R_)
    sets = kw.pop('sets', None) or _small_sets(data)
    make_opt = kw.pop('make_opt', None)
    monkeypatch.setattr(S, 'make_sampler', lambda d, batch_size, num_steps, walk_length=2: S.FixedNodeSets(d, sets))
    args = _args(tmp_path, rest, R_, sets, fused_minibatch=fused, **kw)
    if make_opt is None:
        opt = [torch.optim.Adam(m.deletion1.parameters(), lr=args.lr), torch.optim.Adam(m.deletion2.parameters(), lr=args.lr)]
    else:
        opt = make_opt(m, args.lr)
    tr = TK.KGGNNDeleteNodeembTrainer(args)
    torch.manual_seed(77)                               # negative_sampling_kg and the validation subsets: the host stream
    tr.train(m, Data(dict(data)), opt, args)
    return tr, m, opt, float(torch.rand(1))


def test_fused_kg_step_matches_autograd_loop(tmp_path, monkeypatch):
    """mse_sum, 4 batches of 30 nodes (one without a Df triple), 3 epochs: step records, Del weights, Adam state and the host
    random stream after train against the autograd loop.  Bounds: the project's rtol / rel-L2 1e-4 (fp32 sums in another
    order; bit equality is not asked)."""
    _, _, data, _, _ = _fixture()
    sets = _small_sets(data)
    assert [s_.numel() for s_ in sets] == [30] * 4
    (ta, ma, oa, ra), (tf, mf, of, rf) = (_run_small(tmp_path, monkeypatch, fused, loss_fct='mse_sum', epochs=3, valid_freq=3)
                                          for fused in (False, True))
    assert 'minibatch_step' not in ta.trainer_log and tf.trainer_log['minibatch_step'] == 'fused'
    assert len(tf.trainer_log['steps']) == len(ta.trainer_log['steps']) == 12
    assert ta.trainer_log['steps'][2]['loss_r'] == 0.0             # the batch without a Df triple: the sum over nothing
    for key in ['Epoch', 'train_loss', 'loss_r', 'loss_l']:
        a = np.array([s_[key] for s_ in ta.trainer_log['steps']], dtype=np.float64)
        f = np.array([s_[key] for s_ in tf.trainer_log['steps']], dtype=np.float64)
        print(key, 'max rel diff', float(np.nanmax(np.abs(f - a) / np.maximum(np.abs(a), 1e-30))))
        np.testing.assert_allclose(f, a, rtol=1e-4, atol=1e-8, err_msg=key, equal_nan=True)
    for name in ('deletion1', 'deletion2'):
        pa, pf = getattr(ma, name).deletion_weight, getattr(mf, name).deletion_weight
        print(name, 'rel-L2', rel_l2(pf.detach().cpu(), pa.detach().cpu()))
        assert rel_l2(pf.detach().cpu(), pa.detach().cpu()) < 1e-4
    assert ra == rf                                                 # the host random stream after train
    for opa, opf in zip(oa, of):
        (pa,), (pf,) = opa.param_groups[0]['params'], opf.param_groups[0]['params']
        sa, sf = opa.state[pa], opf.state[pf]
        assert float(sa['step']) == float(sf['step']) == 12
        for k in ['exp_avg', 'exp_avg_sq']:
            assert rel_l2(sf[k].cpu(), sa[k].cpu()) < 1e-4, k
    assert rel_l2(mf.deletion1.deletion_weight.grad.cpu(), ma.deletion1.deletion_weight.grad.cpu()) < 1e-4
    la, lf = ([r for r in tr.trainer_log['log'] if 'val_dt_auc' in r][-1] for tr in (ta, tf))
    assert abs(la['val_loss'] - lf['val_loss']) < 1e-4 and abs(la['val_dt_auc'] - lf['val_dt_auc']) < 2e-3


def test_fused_kg_step_logs_nan_for_a_mean_over_no_triple(tmp_path, monkeypatch):
    """mse_mean on the batch without a Df triple: upstream's MSE of nothing is NaN, logged as such, and the step is still taken."""
    _, _, data, _, _ = _fixture()
    sets = _small_sets(data)[2:3]
    (ta, ma, oa, _), (tf, mf, of, _) = (_run_small(tmp_path, monkeypatch, fused, sets=sets, epochs=2, valid_freq=2)
                                        for fused in (False, True))
    for tr in (ta, tf):
        assert all(np.isnan(s_['loss_r']) and np.isnan(s_['train_loss']) for s_ in tr.trainer_log['steps'])
    np.testing.assert_allclose([s_['loss_l'] for s_ in tf.trainer_log['steps']], [s_['loss_l'] for s_ in ta.trainer_log['steps']],
                               rtol=1e-4)
    for name, opa, opf in zip(('deletion1', 'deletion2'), oa, of):
        pa, pf = getattr(ma, name).deletion_weight, getattr(mf, name).deletion_weight
        assert float(opa.state[pa]['step']) == float(opf.state[pf]['step']) == 2          # the step was taken
        assert bool(torch.isfinite(pf).all()) and rel_l2(pf.detach().cpu(), pa.detach().cpu()) < 1e-4


def _rgat(state, data, R_):
    from gnndelete_amd.framework import models as M
    torch.manual_seed(5)
    return M.RGATDelete(SimpleNamespace(in_dim=32, hidden_dim=32, out_dim=16), int(data['num_nodes']), R_,
                        data['sdf_node_1hop_mask'], data['sdf_node_2hop_mask']).cuda()


def _wide(state, data, R_):
    from gnndelete_amd.framework import models as M
    torch.manual_seed(5)
    return M.RGCNDelete(SimpleNamespace(in_dim=32, hidden_dim=136, out_dim=16), int(data['num_nodes']), R_,
                        data['sdf_node_1hop_mask'], data['sdf_node_2hop_mask']).cuda()


FALLBACKS = {
    'rgat': (dict(model=_rgat), 'R-GCN only'),
    'loss_fct': (dict(loss_fct='cosine_mean'), 'is not an MSE loss'),
    'loss_type': (dict(loss_type='both_all'), '--loss_type both_all'),
    'widths': (dict(model=_wide), 'widths 32 -> 136'),
    'optimizer': (dict(make_opt=lambda m, lr: [torch.optim.Adam(m.deletion1.parameters(), lr=lr, weight_decay=1e-3),
                                               torch.optim.Adam(m.deletion2.parameters(), lr=lr)]), 'two plain torch.optim.Adam'),
    'ranks': (dict(), 'more than one rank'),
}


@pytest.mark.parametrize('why', sorted(FALLBACKS))
def test_fused_kg_step_falls_back(why, tmp_path, monkeypatch, capsys):
    """Each case the fused step does not take: one line says why, trainer_log['minibatch_step'] records it, and the
    autograd loop runs as without the flag (same Del weights, bit for bit)."""
    from gnndelete_amd.framework.trainer import sampler as S
    kw, text = FALLBACKS[why]
    _, state, data, _, R_ = _fixture()
    sets = _small_sets(data)[:2]
    if why == 'ranks':
        monkeypatch.setattr(S, 'data_parallel_world', lambda: (0, 2))
        monkeypatch.setattr(S, 'sync_gradients', lambda optimizer: None)
    res = []
    for fused in (False, True):
        kw_run = dict(kw)
        if 'model' in kw_run:
            kw_run['model'] = kw_run['model'](state, data, R_)
        res.append(_run_small(tmp_path, monkeypatch, fused, sets=sets, epochs=1, valid_freq=1, **kw_run))
    out = capsys.readouterr().out
    line = [l for l in out.splitlines() if l.startswith('--fused_minibatch:')]
    assert len(line) == 1 and text in line[0] and 'running the autograd mini-batch loop' in line[0]
    (ta, ma, _, ra), (tf, mf, _, rf) = res
    assert 'minibatch_step' not in ta.trainer_log
    assert tf.trainer_log['minibatch_step'].startswith('autograd: ') and text in tf.trainer_log['minibatch_step']
    assert len(tf.trainer_log['steps']) == 2 and ra == rf
    for name in ('deletion1', 'deletion2'):
        assert torch.equal(getattr(ma, name).deletion_weight.detach(), getattr(mf, name).deletion_weight.detach())
