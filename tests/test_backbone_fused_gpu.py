"""The fused backbone step (gnndelete_amd.backbone, --fused_backbone) through Trainer and RetrainTrainer: the reference's golden
trajectories, seeded requests with fresh negatives every epoch against the oracle's fp64 loop (held to what an fp32 ensemble of
the same oracle delivers, and to today's autograd path), the edge cases of the lists, reproducibility, resuming, the exported
optimizer state, the fallbacks and the CLI.

Measured on an MI355X, rel-L2 to the fp64 loop over the fresh-negatives requests (both shapes) and the edge cases, GCN and GAT:
  parameters  fused 3.7e-8 ... 4.5e-7   fp32 oracle ensemble 3.7e-8 ... 3.6e-7
  updates     fused 6.2e-8 ... 6.9e-6   ensemble 5.1e-8 ... 6.1e-6   (final - initial; largest on the attention vectors)
  moments     fused 6.1e-8 ... 1.0e-6   ensemble 5.0e-8 ... 1.1e-6
  losses      fused 6.7e-8 ... 2.1e-7   ensemble 0 ... 2.0e-7
so the floors (5e-5 parameters, updates and moments, 1e-5 losses) decide every case here; today's autograd path sits in the
same ranges."""
import functools
import json
import os
import subprocess
import sys
from types import SimpleNamespace
from unittest import mock

import numpy as np
import pytest
import torch

from helpers import load_golden, rel_l2, split_fixture, t

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLOOR = 5e-5                                  # tests/helpers.py: assert_del_weights_within_fp32_spread (weights and moments)
LOSS_FLOOR = 1e-5                             # tests/test_edgeprob_kernels_gpu.py: TOL, the kernel suite's bound on the loss values
CEILING = 1e-4                                # the golden trajectories' bound on the parameters
W_KEY = {'gcn': 'conv1.lin.weight', 'gat': 'conv1.lin_src.weight', 'gin': 'conv1.nn.weight', 'sage': 'conv1.lin_l.weight'}


def _assert_checkpoint_has_moments(path, model):
    ck = torch.load(path)
    state = ck['optimizer_state']['state']
    n_params = len(list(model.parameters()))
    assert set(ck['model_state']) == set(model.state_dict()) and sorted(state) == list(range(n_params))
    for k, p in enumerate(model.parameters()):
        assert float(state[k]['step']) >= 1
        for key in ('exp_avg', 'exp_avg_sq'):
            assert state[k][key].shape == p.shape and bool(torch.isfinite(state[k][key]).all())
        assert float(state[k]['exp_avg_sq'].abs().max()) > 0


# ------------------------------------------------------------------------------------------ golden trajectories
@pytest.mark.parametrize('gnn', ['gcn', 'gat'])
def test_fused_backbone_reproduces_reference_training(tmp_path, monkeypatch, gnn):
    """test_cli_gpu.py::test_original_trainer_reproduces_reference_training with the flag: same assertions, tolerances."""
    from gnndelete_amd.framework import get_model
    from gnndelete_amd.framework.data import Data
    from gnndelete_amd.framework.trainer import base as TB
    fx = load_golden(f'orig_{gnn}.npz')
    state, data, rest = split_fixture(fx)
    key = W_KEY[gnn]
    key2 = key.replace('conv1', 'conv2')
    args = SimpleNamespace(unlearning_model='original', gnn=gnn, dataset='Cora', checkpoint_dir=str(tmp_path),
                           in_dim=state[key].shape[1], hidden_dim=state[key].shape[0], out_dim=state[key2].shape[0],
                           eval_on_cpu=False, epochs=int(rest['epochs']), valid_freq=1, lr=float(rest['lr']), fused_backbone=True)
    m = get_model(args)
    res = m.load_state_dict(state, strict=False)
    assert not res.unexpected_keys and not [k for k in res.missing_keys if 'lin_dst' not in k]
    neg = t(rest['neg']).cuda()
    monkeypatch.setattr(TB, 'negative_sampling', lambda *a, **k: neg)
    opt = torch.optim.Adam(m.parameters(), lr=args.lr)
    tr = TB.Trainer(args)
    torch.manual_seed(int(rest['eval_seed']))
    tr.train(m, Data(data), opt, args)
    assert tr.trainer_log['backbone_step'] == 'fused'
    logs = [r for r in tr.trainer_log['log'] if 'train_loss' in r]
    assert len(logs) == args.epochs
    np.testing.assert_allclose([r['train_loss'] for r in logs], rest['train_loss'], rtol=1e-4)
    final = {k[len('final::'):]: v for k, v in fx.items() if k.startswith('final::')}
    checked = 0
    for k, v in m.state_dict().items():
        if k in final:
            assert rel_l2(v.cpu(), final[k]) < 1e-4, k
            checked += 1
    assert checked >= 4
    _assert_checkpoint_has_moments(os.path.join(str(tmp_path), 'model_best.pt'), m)
    z = torch.load(os.path.join(str(tmp_path), 'node_embeddings.pt'))
    assert z.shape == (data['num_nodes'], args.out_dim) and bool(torch.isfinite(z).all())
    assert all(p.grad is None for p in m.parameters())


def test_fused_backbone_reproduces_reference_retrain(tmp_path, monkeypatch):
    """test_cli_gpu.py::test_retrain_trainer_reproduces_reference with the flag: same assertions, tolerances."""
    from gnndelete_amd.framework import get_model, get_trainer
    from gnndelete_amd.framework.data import Data
    from gnndelete_amd.framework.trainer import retrain as TR
    fx = load_golden('retrain_gcn.npz')
    state, data, rest = split_fixture(fx)
    w1, w2 = state['conv1.lin.weight'], state['conv2.lin.weight']
    epochs = int(rest['epochs'])
    args = SimpleNamespace(unlearning_model='retrain', gnn='gcn', dataset='Cora', checkpoint_dir=str(tmp_path),
                           in_dim=w1.shape[1], hidden_dim=w1.shape[0], out_dim=w2.shape[0], eval_on_cpu=False, epochs=epochs,
                           valid_freq=epochs, lr=float(rest['lr']), fused_backbone=True)
    m = get_model(args)
    m.load_state_dict(state)
    n_negs = int(rest['n_negs'])
    negs = iter([t(fx[f'negs::{i}']) for i in range(n_negs)])
    n_dr = int(data['dr_mask'].sum())

    def fake_neg(edge_index, num_nodes, num_neg_samples):
        assert edge_index.shape[1] == n_dr and num_neg_samples == n_dr          # Dr only
        return next(negs).to(edge_index.device)
    monkeypatch.setattr(TR, 'negative_sampling', fake_neg)
    tr = get_trainer(args)
    assert isinstance(tr, TR.RetrainTrainer)
    opt = torch.optim.Adam(m.parameters(), lr=args.lr)
    torch.manual_seed(int(rest['eval_seed']))
    d = Data(data)
    d.dtrain_mask = d.dr_mask
    tr.train(m, d, opt, args)
    assert tr.trainer_log['backbone_step'] == 'fused'
    assert [s_['Epoch'] for s_ in tr.trainer_log['steps']] == list(range(epochs))
    np.testing.assert_allclose([s_['train_loss'] for s_ in tr.trainer_log['steps']], rest['train_loss'], rtol=1e-4)
    final = {k[len('final::'):]: v for k, v in fx.items() if k.startswith('final::')}
    for k, v in m.state_dict().items():
        assert rel_l2(v.cpu(), final[k]) < 1e-4, k
    vals = [r for r in tr.trainer_log['log'] if 'val_dt_auc' in r]
    assert abs(vals[-1]['val_dt_auc'] - float(rest['val_dt_auc'][-1])) < 2e-3
    assert abs(vals[-1]['val_df_auc'] - float(rest['val_df_auc'][-1])) < 2e-3
    for name in ('model_best.pt', 'model_final.pt'):
        _assert_checkpoint_has_moments(os.path.join(str(tmp_path), name), m)
        assert float(torch.load(os.path.join(str(tmp_path), name))['optimizer_state']['state'][0]['step']) == epochs


# ------------------------------------------------------------------------------------------ seeded requests
def _request(f=32, n=400, n_edges=1600, hub=80, isolate=3, seed=0, keep=1.0):
    """A seeded training request: ~n_edges undirected random edges, node 0 joined to `hub` others, the last `isolate` nodes
    without an edge; train_pos_edge_index holds both directions; dr_mask keeps a share `keep` of the undirected edges."""
    g = torch.Generator().manual_seed(seed)
    e = torch.randint(1, n - isolate, (2, n_edges), generator=g)
    e = e[:, e[0] != e[1]]
    spokes = torch.randperm(n - isolate - 1, generator=g)[:hub] + 1
    e = torch.cat([e, torch.stack([torch.zeros(hub, dtype=torch.long), spokes])], 1)
    e = torch.unique(torch.stack([e.min(0).values, e.max(0).values]), dim=1)
    kept = torch.rand(e.shape[1], generator=g) < keep
    return {'num_nodes': n, 'x': torch.randn(n, f, generator=g), 'train_pos_edge_index': torch.cat([e, e.flip(0)], 1),
            'dr_mask': torch.cat([kept, kept])}


def _negatives(data, epochs, seed, fewer=50):
    from gnndelete_amd.framework import graph_utils as GU
    g = torch.Generator().manual_seed(seed)
    E = data['train_pos_edge_index'][:, data['dr_mask']]
    return [GU.negative_sampling(E, data['num_nodes'], max(E.shape[1] - fewer, 0), generator=g) for _ in range(epochs)]


def _initial_state(gnn, dims, seed=7):
    from gnndelete_amd.framework import models as M
    torch.manual_seed(seed)
    m = {'gcn': M.GCN, 'gat': M.GAT, 'gin': M.GIN, 'sage': M.SAGE}[gnn](SimpleNamespace(in_dim=dims[0], hidden_dim=dims[1],
                                                                                        out_dim=dims[2]))
    return {k: v.detach().clone() for k, v in m.state_dict().items()}


def _named(model):
    return dict(model.named_parameters())                 # (shared tensors once: lin_src / lin_dst)


def _result(model, opt, losses, state):
    params = {k: p.detach().cpu().double() for k, p in _named(model).items()}
    out = {'params': params, 'updates': {k: v - state[k].double() for k, v in params.items()},
           'losses': torch.as_tensor(losses, dtype=torch.float64), 'steps': {}}
    for k, p in _named(model).items():
        st = opt.state[p]
        out['steps'][k] = float(st['step'])
        for key in ('exp_avg', 'exp_avg_sq'):
            out[f'{key}'] = {**out.get(key, {}), k: st[key].detach().cpu().double()}
    return out


def _oracle_loop(gnn, dims, state, data, negs, lr, dtype=torch.float64, perm=None):
    """oracle.gnndelete_ref.retrain_fullbatch on the CPU in `dtype` (dr_mask all true: the original-training case).  perm = a
    seed: the edge list is permuted first - another summation order in every scatter, another correct implementation."""
    from oracle import gnndelete_ref as R
    torch.set_num_threads(min(32, torch.get_num_threads()))
    ref = R.TwoLayer(gnn, *dims)
    missing = ref.load_state_dict(state, strict=False)
    assert not missing.unexpected_keys and not [k for k in missing.missing_keys if 'lin_dst' not in k]
    ref = ref.to(dtype)
    d = {'x': data['x'].to(dtype), 'train_pos_edge_index': data['train_pos_edge_index'], 'dr_mask': data['dr_mask']}
    if perm is not None:
        order = torch.randperm(d['dr_mask'].numel(), generator=torch.Generator().manual_seed(perm))
        d['train_pos_edge_index'], d['dr_mask'] = d['train_pos_edge_index'][:, order], d['dr_mask'][order]
    made, real = [], torch.optim.Adam
    with mock.patch.object(torch.optim, 'Adam', lambda *a, **k: made.append(real(*a, **k)) or made[-1]):
        losses = R.retrain_fullbatch(ref, d, len(negs), lr, negs)
    return _result(ref, made[0], losses, state)


@functools.lru_cache(maxsize=None)
def _references(gnn, dims, case):
    """(data, negatives, initial state, fp64 loop, fp32 ensemble) of a named request: computed once, shared, never changed."""
    data, negs = _case(case, dims[0])
    state = _initial_state(gnn, dims)
    ref = _oracle_loop(gnn, dims, state, data, negs, 1e-3)
    ens = [_oracle_loop(gnn, dims, state, data, negs, 1e-3, torch.float32, perm) for perm in (None, 1, 2)]
    return data, negs, state, ref, ens


def _trainer_run(kind, gnn, dims, state, data, negs, fused, tmp_path, monkeypatch, lr=1e-3, engine_kw=None, valid_freq=None,
                 resume=None, make_opt=None, extra=None):
    """Trainer.train ('original') or RetrainTrainer.train ('retrain') on the HIP model with each epoch's negatives injected
    through the module-level seam.  resume = an earlier run: a second train call on its model and its optimizer."""
    from gnndelete_amd.framework import models as M
    from gnndelete_amd.framework.data import Data
    from gnndelete_amd.framework.trainer import base as TB, retrain as TR
    if resume:
        m = resume['model']
    else:
        m = {'gcn': M.GCN, 'gat': M.GAT, 'gin': M.GIN, 'sage': M.SAGE}[gnn](SimpleNamespace(in_dim=dims[0], hidden_dim=dims[1],
                                                                                            out_dim=dims[2]))
        m.load_state_dict(state)
        m = m.cuda()
    os.makedirs(str(tmp_path), exist_ok=True)
    it = iter(negs)
    mod = TR if kind == 'retrain' else TB
    monkeypatch.setattr(mod, 'negative_sampling', lambda *a, **k: next(it).cuda())
    if engine_kw:
        from gnndelete_amd import backbone as BB
        orig = getattr(BB.BackboneEngine, 'wrapped', BB.BackboneEngine)
        with_kw = lambda *a, **k: orig(*a, **{**k, **engine_kw})
        with_kw.wrapped = orig
        monkeypatch.setattr(BB, 'BackboneEngine', with_kw)
    args = SimpleNamespace(unlearning_model=kind, gnn=gnn, dataset='Cora', checkpoint_dir=str(tmp_path), eval_on_cpu=False,
                           epochs=len(negs), valid_freq=valid_freq or (len(negs) if kind == 'retrain' else 1), lr=lr,
                           **({'fused_backbone': True} if fused else {}), **(extra or {}))
    opt = resume['opt'] if resume else (make_opt or (lambda ps: torch.optim.Adam(ps, lr=lr)))(list(m.parameters()))
    tr = (TR.RetrainTrainer if kind == 'retrain' else TB.Trainer)(args)
    # the request has no validation split: the epoch records are what is under test, not Trainer.eval
    monkeypatch.setattr(tr, 'eval', lambda *a, **k: (0.0, 0.0, 0.0, 0.0, 0.0, [], None, {}))
    d = Data({k: (v.clone() if torch.is_tensor(v) else v) for k, v in data.items()})
    if kind == 'original':
        d.train_pos_edge_index = d.train_pos_edge_index[:, d.dr_mask]          # base.Trainer trains on every edge it is given
        d.dr_mask = torch.ones(d.train_pos_edge_index.shape[1], dtype=torch.bool)
    tr.train(m, d, opt, args)
    if kind == 'retrain':
        losses = [s['train_loss'] for s in tr.trainer_log['steps']]
    else:
        losses = [r['train_loss'] for r in tr.trainer_log['log'] if 'train_loss' in r]
    out = _result(m, opt, losses, state) if isinstance(opt, torch.optim.Adam) else {'losses': torch.as_tensor(losses, dtype=torch.float64)}
    out.update(tr=tr, model=m, opt=opt)
    return out


def _distances(run, ref):
    d = {}
    for group in ('params', 'updates', 'exp_avg', 'exp_avg_sq'):
        for k, want in ref[group].items():
            d[f'{group} {k}'] = rel_l2(run[group][k], want)
    d['losses'] = rel_l2(run['losses'], ref['losses'])
    return d


def _assert_within_ensemble(tag, run, ens, ref, autograd=None):
    """The run's rel-L2 to the fp64 loop <= min(max(2 x the largest of the fp32 oracle ensemble, floor), 1e-4) for every
    parameter, every update (final - initial), both Adam moments of every parameter and the loss series; floor = 5e-5
    (weights, updates, moments) / 1e-5 (losses).  autograd = today's path on the same request: it is held to the same bound,
    and the fused distance is also <= max(2 x its distance, floor), as test_edgeprob_fused_gpu._assert_within_spread holds it."""
    dr, de = _distances(run, ref), [_distances(e, ref) for e in ens]
    da = _distances(autograd, ref) if autograd is not None else None
    for k in dr:
        print(f'[{tag}] {k}: rel-L2 to the fp64 loop: fused {dr[k]:.2e} / fp32 oracle ensemble ' + ' '.join(f'{d[k]:.2e}' for d in de)
              + (f' / autograd {da[k]:.2e}' if da else ''))
    for k in dr:
        floor = LOSS_FLOOR if k == 'losses' else FLOOR
        assert dr[k] <= min(max(2.0 * max(d[k] for d in de), floor), CEILING), (tag, k, dr[k], [d[k] for d in de])
        if da is not None:
            assert da[k] <= min(max(2.0 * max(d[k] for d in de), floor), CEILING), (tag, 'the autograd path', k, da[k])
            assert dr[k] <= max(2.0 * da[k], floor), (tag, 'against the autograd path', k, dr[k], da[k])
    assert run['steps'] == ref['steps']
    return dr


def _case(name, f):
    if name == 'fresh':
        data = _request(f=f)
        return data, _negatives(data, 8, seed=3)
    if name == 'no_negatives':
        data = _request(f=f, n=200, n_edges=600, hub=70, seed=11)
        return data, _negatives(data, 4, seed=4, fewer=10 ** 9)
    if name == 'repeated_negative':
        data = _request(f=f, n=200, n_edges=600, hub=70, seed=12)
        negs = _negatives(data, 4, seed=5)
        for neg in negs:
            neg[:, 1] = neg[:, 0]                           # the same pair twice
            neg[:, 2] = neg[:, 0].flip(0)                   # and once the other way round
        return data, negs
    if name == 'negative_hub':
        # node 5 in 90 negatives of every epoch (more than 64 decoded incidences from the negatives' half alone) and an
        # isolated node in the decoded list
        data = _request(f=f, n=200, n_edges=600, hub=70, seed=13)
        negs = _negatives(data, 4, seed=6)
        for neg in negs:
            neg[0, 10:100] = 5
            neg[:, 3] = torch.tensor([199, 5])
            neg[1, 10:100] = torch.where(neg[1, 10:100] == 5, torch.tensor(6), neg[1, 10:100])
        return data, negs
    if name == 'retrain_5pct':
        data = _request(f=f, seed=14, keep=0.95)
        return data, _negatives(data, 6, seed=7)
    raise KeyError(name)


@pytest.mark.parametrize('dims', [(32, 32, 16), (100, 64, 32)], ids=['32-32-16', '100-64-32'])
@pytest.mark.parametrize('gnn', ['gcn', 'gat'])
def test_fused_backbone_with_fresh_negatives_every_epoch(gnn, dims, tmp_path, monkeypatch):
    data, negs, state, ref, ens = _references(gnn, dims, 'fresh')
    E = data['train_pos_edge_index']
    deg = torch.bincount(E[0], minlength=400)
    assert int(deg[0]) == 80 and int((deg == 0).sum()) >= 3 and 3000 <= E.shape[1] <= 3400
    assert negs[0].shape[1] == E.shape[1] - 50 and not torch.equal(negs[0], negs[1])
    autograd = _trainer_run('retrain', gnn, dims, state, data, negs, False, tmp_path / 'a', monkeypatch)
    fused = _trainer_run('retrain', gnn, dims, state, data, negs, True, tmp_path / 'f', monkeypatch)
    assert fused['tr'].trainer_log['backbone_step'] == 'fused' and 'backbone_step' not in autograd['tr'].trainer_log
    eng = fused['tr']._backbone
    assert (eng.fwd1, eng.wgrad1) == (('rows', 'rows') if dims[0] == 32 else ('wide', 'xT'))
    _assert_within_ensemble(f'fresh negatives {gnn} {dims}', fused, ens, ref, autograd)
    assert len(fused['losses']) == 8 and all(p.grad is None for p in fused['model'].parameters())
    # the original-model trainer on the same request takes the same step
    orig = _trainer_run('original', gnn, dims, state, data, negs, True, tmp_path / 'o', monkeypatch)
    assert orig['tr'].trainer_log['backbone_step'] == 'fused'
    for k, v in fused['params'].items():
        assert torch.equal(orig['params'][k], v), k
    assert torch.equal(orig['losses'], fused['losses'])


@pytest.mark.parametrize('gnn', ['gcn', 'gat'])
@pytest.mark.parametrize('name', ['no_negatives', 'repeated_negative', 'negative_hub', 'retrain_5pct'])
def test_fused_backbone_edge_cases(name, gnn, tmp_path, monkeypatch):
    dims = (32, 32, 16)
    data, negs, state, ref, ens = _references(gnn, dims, name)
    if name == 'no_negatives':
        assert all(neg.shape == (2, 0) for neg in negs)
    if name == 'retrain_5pct':
        assert 0.9 < float(data['dr_mask'].float().mean()) < 0.99
    fused = _trainer_run('retrain', gnn, dims, state, data, negs, True, tmp_path / 'f', monkeypatch)
    assert fused['tr'].trainer_log['backbone_step'] == 'fused'
    if name == 'negative_hub':
        eng = fused['tr']._backbone
        inc = (eng.inc_ptr[1:] - eng.inc_ptr[:-1]).cpu()
        assert int(inc[5]) > 64 + int(torch.bincount(data['train_pos_edge_index'].flatten(), minlength=200)[5])
    _assert_within_ensemble(f'{name} {gnn}', fused, ens, ref)


@pytest.mark.parametrize('gnn', ['gcn', 'gat'])
def test_fused_backbone_eager_replay_and_rerun_agree_bit_for_bit(gnn, tmp_path, monkeypatch):
    dims = (100, 64, 32)
    data = _request(f=dims[0], n=200, n_edges=700, hub=70, seed=21)
    negs = _negatives(data, 5, seed=8)
    state = _initial_state(gnn, dims)
    runs = [_trainer_run('retrain', gnn, dims, state, data, negs, True, tmp_path / str(k), monkeypatch, engine_kw=kw)
            for k, kw in enumerate(({'use_graph': True}, {'use_graph': False}, {'use_graph': True}))]
    assert runs[0]['tr']._backbone._graph is not None and runs[1]['tr']._backbone._graph is None
    hist = [r['tr']._backbone.loss_history() for r in runs]
    assert hist[0].shape == (5,) and all(float(v.abs().max()) > 0 for v in runs[0]['updates'].values())
    for r, h in zip(runs[1:], hist[1:]):
        for group in ('params', 'exp_avg', 'exp_avg_sq'):
            for k, v in runs[0][group].items():
                assert torch.equal(r[group][k], v), (group, k)
        assert torch.equal(h, hist[0])
    assert torch.equal(hist[0].double(), runs[0]['losses'])          # the epoch records are the ring's rows
    assert runs[0]['tr']._backbone.last_loss() == float(hist[0][-1])
    with pytest.raises(ValueError):
        runs[0]['tr']._backbone.step(negs[0][:, :-1].cuda())


@pytest.mark.parametrize('kind', ['original', 'retrain'])
def test_fused_backbone_resumes_on_the_same_model_and_optimizer(kind, tmp_path, monkeypatch):
    gnn, dims = 'gcn', (32, 32, 16)
    data = _request(f=dims[0], n=200, n_edges=700, hub=70, seed=22)
    negs = _negatives(data, 8, seed=9)
    state = _initial_state(gnn, dims)
    whole = _trainer_run(kind, gnn, dims, state, data, negs, True, tmp_path / 'w', monkeypatch)
    first = _trainer_run(kind, gnn, dims, state, data, negs[:4], True, tmp_path / 'h', monkeypatch)
    assert set(first['steps'].values()) == {4.0}
    second = _trainer_run(kind, gnn, dims, state, data, negs[4:], True, tmp_path / 'h', monkeypatch, resume=first)
    assert second['tr'].trainer_log['backbone_step'] == 'fused' and set(second['steps'].values()) == {8.0}
    for group in ('params', 'exp_avg', 'exp_avg_sq'):
        for k, v in whole[group].items():
            assert torch.equal(second[group][k], v), (group, k)
    assert torch.equal(torch.cat([first['losses'], second['losses']]), whole['losses'])


# ------------------------------------------------------------------------------------------ fallbacks
@pytest.mark.parametrize('what', ['gin', 'sage', 'sgd', 'weight_decay', 'minibatch'])
def test_fused_backbone_falls_back_to_the_autograd_loop(what, tmp_path, monkeypatch, capsys):
    gnn = what if what in ('gin', 'sage') else 'gcn'
    dims = (32, 32, 16)
    data = _request(f=dims[0], n=120, n_edges=400, hub=20, seed=31)
    negs = _negatives(data, 3, seed=9)
    state = _initial_state(gnn, dims)
    make_opt = {'sgd': lambda ps: torch.optim.SGD(ps, lr=1e-2),
                'weight_decay': lambda ps: torch.optim.Adam(ps, lr=1e-3, weight_decay=5e-4)}.get(what)
    extra = {'minibatch': True} if what == 'minibatch' else None
    want = {'gin': 'no fused backbone step for the GIN backbone (GCN and GAT only)',
            'sage': 'no fused backbone step for the SAGE backbone (GCN and GAT only)',
            'sgd': 'the optimizer is not one plain torch.optim.Adam', 'weight_decay': 'Adam with weight decay',
            'minibatch': '--minibatch trains on GraphSAINT batches'}[what]
    for kind in ('original', 'retrain'):
        plain = _trainer_run(kind, gnn, dims, state, data, negs, False, tmp_path / f'{kind}p', monkeypatch, make_opt=make_opt, extra=extra)
        capsys.readouterr()
        flag = _trainer_run(kind, gnn, dims, state, data, negs, True, tmp_path / f'{kind}f', monkeypatch, make_opt=make_opt, extra=extra)
        out = capsys.readouterr().out
        assert out.count(f'--fused_backbone: {want}; running the autograd loop') == 1
        assert flag['tr'].trainer_log['backbone_step'] == want and not hasattr(flag['tr'], '_backbone')
        assert 'backbone_step' not in plain['tr'].trainer_log
        # the same records as the run without the flag
        for key in ('log', 'steps'):
            a, b = plain['tr'].trainer_log.get(key), flag['tr'].trainer_log.get(key)
            assert (a is None) == (b is None)
            if a is not None:
                assert [sorted(r) for r in a] == [sorted(r) for r in b]
                assert [r.get('epoch', r.get('Epoch')) for r in a] == [r.get('epoch', r.get('Epoch')) for r in b]
        assert len(flag['losses']) == 3 and rel_l2(flag['losses'], plain['losses']) < 1e-6
        for (k, p), (_, q) in zip(flag['model'].state_dict().items(), plain['model'].state_dict().items()):
            assert rel_l2(p.cpu(), q.cpu()) < 1e-5, k
        assert sorted(os.listdir(str(tmp_path / f'{kind}p'))) == sorted(os.listdir(str(tmp_path / f'{kind}f')))


# ------------------------------------------------------------------------------------------ CLI
def test_cli_fused_backbone(tmp_path):
    cwd = str(tmp_path)
    # (upstream's overrides make the original model's run 2,000 epochs whatever --epochs says: the tests' knobs come after them)
    env = dict(os.environ, PYTHONPATH=ROOT, GNNDELETE_FORCE_EPOCHS='20', GNNDELETE_FORCE_VALID_FREQ='10')

    def run(cmd):
        r = subprocess.run([sys.executable] + cmd, cwd=cwd, env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        return r.stdout
    common = ['--dataset', 'synth-tiny', '--gnn', 'gcn', '--random_seed', '42']
    run([os.path.join(ROOT, 'prepare_dataset.py'), '--dataset', 'synth-tiny', '--seeds', '42'])
    files = {}
    for tag, flag in (('plain', []), ('fused', ['--fused_backbone'])):
        base = ['--checkpoint_dir', os.path.join(cwd, tag)]
        run([os.path.join(ROOT, 'train_gnn.py')] + common + base + flag)
        run([os.path.join(ROOT, 'delete_gnn.py')] + common + base + ['--unlearning_model', 'retrain', '--df', 'in', '--df_size', '5']
            + flag)
        dirs = {'original': os.path.join(cwd, tag, 'synth-tiny', 'gcn', 'original', '42'),
                'retrain': os.path.join(cwd, tag, 'synth-tiny', 'gcn', 'retrain', 'in-5.0-42')}
        files[tag] = {k: sorted(os.listdir(v)) for k, v in dirs.items()}
        for k, v in dirs.items():
            with open(os.path.join(v, 'trainer_log.json')) as f:
                log = json.load(f)
            assert log.get('backbone_step') == ('fused' if flag else None), (tag, k)
            assert [r['epoch'] for r in log['log'] if 'train_loss' in r] == [9, 19]
            assert 0.0 <= log['dt_auc'] <= 1.0
            if k == 'retrain':
                assert [s['Epoch'] for s in log['steps']] == list(range(20))
                assert all(np.isfinite(s['train_loss']) for s in log['steps'])
            ck = torch.load(os.path.join(v, 'model_best.pt'))
            assert all(bool(torch.isfinite(w).all()) for w in ck['model_state'].values())
            assert len(ck['optimizer_state']['state']) == 4 and 'exp_avg' in ck['optimizer_state']['state'][0]
    assert files['plain'] == files['fused'] and 'node_embeddings.pt' in files['fused']['original']
