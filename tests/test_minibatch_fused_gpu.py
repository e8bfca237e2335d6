"""The fused GraphSAINT batch step (gnndelete_amd.minibatch, --minibatch --fused_minibatch): the device cut and batch CSRs
bit-identical to the sampler's subgraph() and graph.build_csr, and the step's trajectory against the reference's and
against the autograd mini-batch loop."""
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from helpers import hip_model, load_golden, rel_l2, split_fixture, t

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lists(fx, prefix, count_key):
    return [t(fx[f'{prefix}::{i}']) for i in range(int(fx[count_key]))]


def _synthetic(n=3000, m=24000, seed=5):
    """Directed edges with multi-edges, self loops and one hub of ~2,000 out-edges; random sdf / df / node masks."""
    from gnndelete_amd.framework.data import Data
    g = torch.Generator().manual_seed(seed)
    ei = torch.randint(0, n, (2, m), generator=g)
    hub = torch.stack([torch.zeros(2000, dtype=torch.long), torch.randint(0, n, (2000,), generator=g)])
    ei = torch.cat([ei, hub, ei[:, :50], torch.arange(20).repeat(2, 1)], 1)
    e = ei.shape[1]
    sdf = torch.rand(e, generator=g) < 0.6
    df = sdf & (torch.rand(e, generator=g) < 0.1)
    d = Data(num_nodes=n, edge_index=ei, x=torch.randn(n, 8, generator=g), sdf_mask=sdf, df_mask=df)
    for k in ['sdf_node_1hop_mask', 'sdf_node_2hop_mask', 'sdf_node_1hop_mask_non_df_mask', 'sdf_node_2hop_mask_non_df_mask']:
        d[k] = torch.rand(n, generator=g) < 0.4
    return d


def _node_sets(n, g):
    """Random sets, a set holding the hub (node 0), single nodes (17 has a self loop), all nodes."""
    return [torch.randperm(n, generator=g)[:700].sort().values,
            torch.cat([torch.zeros(1, dtype=torch.long), torch.randperm(n - 1, generator=g)[:400] + 1]).sort().values,
            torch.tensor([17]), torch.tensor([3]), torch.arange(n)]


def test_cut_is_bit_identical_to_subgraph():
    from gnndelete_amd.framework.trainer.sampler import RandomWalkSubgraphSampler
    from gnndelete_amd.minibatch import BatchCut
    d = _synthetic()
    dev = torch.device('cuda')
    sampler = RandomWalkSubgraphSampler(d.clone().to(dev), batch_size=100)
    cut = BatchCut(d, sampler, dev, max_nodes=64)            # small buffers: the first big batches grow them
    sets = _node_sets(d.num_nodes, torch.Generator().manual_seed(1))
    # a set with no induced edge: nodes that share no edge
    ei = d.edge_index
    lonely = torch.tensor([v for v in range(100, 3000) if int(((ei[0] == v) | (ei[1] == v)).sum()) == 0][:5] or [2999])
    sets.append(lonely.sort().values)
    for nodes in sets:
        cnt = cut.cut(nodes.to(dev))
        ref = sampler.subgraph(nodes.to(dev))
        got_ei, got_f = cut.batch_edges()
        assert torch.equal(got_ei, ref.edge_index), nodes.numel()
        assert torch.equal(got_f & 1, ref.sdf_mask.to(torch.uint8)) and torch.equal(got_f >> 1, ref.df_mask.to(torch.uint8))
        assert cnt[:4] == [nodes.numel(), ref.edge_index.shape[1], int(ref.sdf_mask.sum()), int(ref.df_mask.sum())]
        for k, key in enumerate(['sdf_node_1hop_mask', 'sdf_node_2hop_mask', 'sdf_node_1hop_mask_non_df_mask',
                                 'sdf_node_2hop_mask_non_df_mask']):
            rows = ref[key].nonzero().flatten().to(torch.int32)
            assert cnt[4 + k] == rows.numel() and torch.equal(cut.rows(k, rows.numel()), rows)
        assert torch.equal(cut.df_index[:, :cnt[3]], ref.edge_index[:, ref.df_mask])
    assert cut.e_cap >= d.edge_index.shape[1]


@pytest.mark.parametrize('mode', ['gcn', 'gat'])
def test_batch_csrs_match_build_csr(mode):
    from gnndelete_amd.framework.trainer.sampler import RandomWalkSubgraphSampler
    from gnndelete_amd.graph import build_csr
    from gnndelete_amd.minibatch import BatchCut
    d = _synthetic(seed=9)
    dev = torch.device('cuda')
    sampler = RandomWalkSubgraphSampler(d.clone().to(dev), batch_size=100)
    cut = BatchCut(d, sampler, dev)
    for nodes in _node_sets(d.num_nodes, torch.Generator().manual_seed(2)):
        cut.cut(nodes.to(dev))
        ref_b = sampler.subgraph(nodes.to(dev))
        for sdf in (False, True):
            ei = ref_b.edge_index[:, ref_b.sdf_mask] if sdf else ref_b.edge_index
            ref = build_csr(ei.contiguous(), nodes.numel(), mode)
            got = cut.batch_csr(sdf, mode == 'gat')
            for key in ['rowptr', 'col', 'rowptr_t', 'col_t', 'perm_t']:
                assert torch.equal(getattr(got, key), getattr(ref, key)), (key, sdf)
            if mode == 'gcn':
                assert torch.equal(got.val, ref.val) and torch.equal(got.val_t, ref.val_t)


def _traj_setup(tmp_path, monkeypatch, fused, sets=None, negs=True, gnn='gat', state_seed=None):
    from gnndelete_amd.framework.data import Data
    from gnndelete_amd.framework.trainer import gnndelete_nodeemb as TN
    from gnndelete_amd.framework.trainer import sampler as S
    fx = load_golden('traj_minibatch_gat.npz')
    state, data, rest = split_fixture(fx)
    if gnn == 'gcn':
        from gnndelete_amd.framework import models as M
        torch.manual_seed(state_seed)
        i, h, o = data['x'].shape[1], 32, 16
        m = M.GCNDelete(SimpleNamespace(in_dim=i, hidden_dim=h, out_dim=o), data['sdf_node_1hop_mask'],
                        data['sdf_node_2hop_mask']).cuda()
    else:
        m = hip_model(gnn, state, data['sdf_node_1hop_mask'], data['sdf_node_2hop_mask'])
    sets = sets if sets is not None else _lists(fx, 'batch', 'n_batches')
    monkeypatch.setattr(S, 'make_sampler', lambda d, batch_size, num_steps, walk_length=2: S.FixedNodeSets(d, sets))
    if negs:
        it = iter(_lists(fx, 'negs', 'n_negs'))
        monkeypatch.setattr(S, 'negative_sampling', lambda ei, n, k: next(it).to(ei.device))
    epochs = int(rest['epochs'])
    args = SimpleNamespace(unlearning_model='gnndelete_nodeemb', dataset='ogbl-synth', checkpoint_dir=str(tmp_path),
                           eval_on_cpu=False, epochs=epochs, valid_freq=epochs, lr=float(rest['lr']),
                           alpha=float(rest['alpha']), loss_fct='mse_mean', loss_type='both_layerwise', gnn=gnn,
                           batch_size=40, num_steps=len(sets), minibatch=True, fused_minibatch=fused)
    opt = [torch.optim.Adam(m.deletion1.parameters(), lr=args.lr), torch.optim.Adam(m.deletion2.parameters(), lr=args.lr)]
    tr = TN.GNNDeleteNodeembTrainer(args)
    torch.manual_seed(int(rest['eval_seed']))
    tr.train(m, Data(data), opt, args)
    return tr, m, opt, rest, data


def test_fused_minibatch_reproduces_reference_trajectory(tmp_path, monkeypatch):
    tr, m, _, rest, _ = _traj_setup(tmp_path, monkeypatch, True)
    assert tr.trainer_log['minibatch_step'] == 'fused'
    steps = tr.trainer_log['steps']
    assert len(steps) == len(rest['train_loss'])
    for key in ['train_loss', 'train_loss_l', 'train_loss_r']:
        np.testing.assert_allclose([s_[key] for s_ in steps], rest[key], rtol=1e-4, atol=1e-8, err_msg=key)
    assert rel_l2(m.deletion1.deletion_weight.detach().cpu(), rest['final_w1']) < 1e-4
    assert rel_l2(m.deletion2.deletion_weight.detach().cpu(), rest['final_w2']) < 1e-4
    vals = [r for r in tr.trainer_log['log'] if 'val_dt_auc' in r]
    assert abs(vals[-1]['val_dt_auc'] - float(rest['val_dt_auc'][-1])) < 2e-3
    assert abs(vals[-1]['val_df_auc'] - float(rest['val_df_auc'][-1])) < 2e-3
    assert tr._fused_minibatch_step.cut.reads == len(steps)          # one blocking host read per batch


def _edge_case_sets():
    """The fixture's node sets plus a batch without a Df edge and one without an S1 row."""
    fx = load_golden('traj_minibatch_gat.npz')
    _, data, _ = split_fixture(fx)
    n = int(data['x'].shape[0])
    df_nodes = set(data['directed_df_edge_index'].flatten().tolist())
    s1 = data['sdf_node_1hop_mask']
    no_df = torch.tensor([v for v in range(n) if v not in df_nodes][:60])
    no_s1 = (~s1).nonzero().flatten()[:60]
    return _lists(fx, 'batch', 'n_batches') + [no_df.sort().values, no_s1.sort().values]


@pytest.mark.parametrize('gnn', ['gcn', 'gat'])
def test_fused_minibatch_matches_autograd_loop(gnn, tmp_path, monkeypatch):
    sets = _edge_case_sets()
    runs = []
    for fused in (False, True):
        torch.manual_seed(1234)                         # negatives from sampler.negative_sampling: the same draws
        runs.append(_traj_setup(tmp_path, monkeypatch, fused, sets=sets, negs=False, gnn=gnn, state_seed=7))
    (ta, ma, oa, _, _), (tf, mf, of, _, _) = runs
    assert ta.trainer_log['minibatch_step'] == 'autograd' and tf.trainer_log['minibatch_step'] == 'fused'
    for key in ['train_loss', 'train_loss_l', 'train_loss_r']:
        a = np.array([s_[key] for s_ in ta.trainer_log['steps']])
        f = np.array([s_[key] for s_ in tf.trainer_log['steps']])
        assert np.array_equal(np.isfinite(a), np.isfinite(f)), key
        assert not np.isfinite(a).all(), 'the edge-case batches log a mean over zero rows'
        np.testing.assert_allclose(f[np.isfinite(f)], a[np.isfinite(a)], rtol=1e-4, atol=1e-8, err_msg=key)
    for pa, pf in [(ma.deletion1.deletion_weight, mf.deletion1.deletion_weight),
                   (ma.deletion2.deletion_weight, mf.deletion2.deletion_weight)]:
        assert rel_l2(pf.detach().cpu(), pa.detach().cpu()) < 1e-4
    for opa, opf in zip(oa, of):
        (pa,), (pf,) = opa.param_groups[0]['params'], opf.param_groups[0]['params']
        sa, sf = opa.state[pa], opf.state[pf]
        assert float(sa['step']) == float(sf['step'])
        for k in ['exp_avg', 'exp_avg_sq']:
            assert rel_l2(sf[k].cpu(), sa[k].cpu()) < 1e-4, k
    assert rel_l2(mf.deletion1.deletion_weight.grad.cpu(), ma.deletion1.deletion_weight.grad.cpu()) < 1e-4


def test_fused_minibatch_is_reproducible(tmp_path, monkeypatch):
    sets = _edge_case_sets()
    out = []
    for _ in range(2):
        torch.manual_seed(99)
        tr, m, _, _, _ = _traj_setup(tmp_path, monkeypatch, True, sets=sets, negs=False)
        out.append(([s_['train_loss'] for s_ in tr.trainer_log['steps']], m.deletion1.deletion_weight.detach().cpu().clone(),
                    m.deletion2.deletion_weight.detach().cpu().clone()))
    assert np.array_equal(np.array(out[0][0]), np.array(out[1][0]), equal_nan=True)
    assert torch.equal(out[0][1], out[1][1]) and torch.equal(out[0][2], out[1][2])


def test_fused_minibatch_falls_back_for_gin(tmp_path, monkeypatch, capsys):
    from gnndelete_amd.framework import models as M
    from gnndelete_amd.framework.data import Data
    from gnndelete_amd.framework.trainer import gnndelete_nodeemb as TN
    from gnndelete_amd.framework.trainer import sampler as S
    fx = load_golden('traj_minibatch_gat.npz')
    _, data, rest = split_fixture(fx)
    sets = _lists(fx, 'batch', 'n_batches')
    monkeypatch.setattr(S, 'make_sampler', lambda d, batch_size, num_steps, walk_length=2: S.FixedNodeSets(d, sets))
    res = []
    for fused in (False, True):
        torch.manual_seed(3)
        m = M.GINDelete(SimpleNamespace(in_dim=data['x'].shape[1], hidden_dim=32, out_dim=16), data['sdf_node_1hop_mask'],
                        data['sdf_node_2hop_mask']).cuda()
        args = SimpleNamespace(unlearning_model='gnndelete_nodeemb', dataset='ogbl-synth', checkpoint_dir=str(tmp_path),
                               eval_on_cpu=False, epochs=2, valid_freq=2, lr=float(rest['lr']), alpha=float(rest['alpha']),
                               loss_fct='mse_mean', loss_type='both_layerwise', gnn='gin', batch_size=40, num_steps=len(sets),
                               minibatch=True, fused_minibatch=fused)
        opt = [torch.optim.Adam(m.deletion1.parameters(), lr=args.lr), torch.optim.Adam(m.deletion2.parameters(), lr=args.lr)]
        tr = TN.GNNDeleteNodeembTrainer(args)
        torch.manual_seed(11)
        tr.train(m, Data(dict(data)), opt, args)
        res.append((tr, m.deletion2.deletion_weight.detach().cpu().clone()))
    assert 'no fused batch step for the GINDelete backbone' in capsys.readouterr().out
    assert res[1][0].trainer_log['minibatch_step'] == 'autograd'
    assert torch.equal(res[0][1], res[1][1])


def test_cli_fused_minibatch_agrees_with_autograd_loop(tmp_path, monkeypatch):
    import subprocess
    import sys
    monkeypatch.setenv('GNNDELETE_FORCE_EPOCHS', '2')
    monkeypatch.setenv('GNNDELETE_FORCE_VALID_FREQ', '2')
    monkeypatch.setenv('GNNDELETE_FORCE_NUM_STEPS', '3')
    from gnndelete_amd.framework.synth import make_linkpred_dataset
    data, df = make_linkpred_dataset(None, seed=42, shape=(800, 32, 4000, 'dense'))
    logs = []
    for flag in ([], ['--fused_minibatch']):
        cwd = str(tmp_path / ('fused' if flag else 'autograd'))
        data_dir = os.path.join(cwd, 'data', 'ogbl-synth')
        os.makedirs(data_dir)
        data.save(os.path.join(data_dir, 'd_42.pt'))
        torch.save(df, os.path.join(data_dir, 'df_42.pt'))
        common = ['--dataset', 'ogbl-synth', '--gnn', 'gcn', '--random_seed', '42', '--batch_size', '200']
        env = dict(os.environ, PYTHONPATH=ROOT)
        for cmd in (['train_gnn.py'] + common,
                    ['delete_gnn.py'] + common + ['--unlearning_model', 'gnndelete_nodeemb', '--df', 'in', '--df_size', '5',
                                                  '--minibatch'] + flag):
            r = subprocess.run([sys.executable, os.path.join(ROOT, cmd[0])] + cmd[1:], cwd=cwd, env=env, capture_output=True,
                               text=True, timeout=900)
            assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        out = os.path.join(cwd, 'checkpoint', 'ogbl-synth', 'gcn', 'gnndelete_nodeemb',
                           'mse_mean-both_layerwise-0.5-non_connected', 'in-5.0-42')
        with open(os.path.join(out, 'trainer_log.json')) as f:
            logs.append(json.load(f))
    assert logs[0]['minibatch_step'] == 'autograd' and logs[1]['minibatch_step'] == 'fused'
    assert abs(logs[0]['dt_auc'] - logs[1]['dt_auc']) < 2e-3
