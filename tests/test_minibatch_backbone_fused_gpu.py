"""The fused backbone batch step (gnndelete_amd.minibatch.MinibatchBackboneStep, train_gnn.py --minibatch --fused_minibatch):
its trajectory against the reference's (tests/golden/orig_minibatch_gcn.npz, at the bounds tests/test_cli_gpu.py holds the
autograd loop to on the same file) and against the autograd mini-batch loop on a seeded graph with edge-case batches;
reproducibility; continuation through the checkpoint's optimizer state; the checkpoints; the fall-back; one CLI run."""
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from helpers import load_golden, rel_l2, split_fixture, t

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lists(fx, prefix, count_key):
    return [t(fx[f'{prefix}::{i}']) for i in range(int(fx[count_key]))]


def test_fused_step_reproduces_reference_trajectory(tmp_path, monkeypatch):
    """tests/test_cli_gpu.py::test_original_minibatch_trainers_reproduce_reference's GCN half with the flag: same seams
    (the node sets and negatives the reference's loop consumed), same bounds."""
    from gnndelete_amd.framework import get_model
    from gnndelete_amd.framework.data import Data
    from gnndelete_amd.framework.trainer import base as TB
    from gnndelete_amd.framework.trainer import sampler as S
    fx = load_golden('orig_minibatch_gcn.npz')
    state, data, rest = split_fixture(fx)
    w1, w2 = state['conv1.lin.weight'], state['conv2.lin.weight']
    sets, negs = _lists(fx, 'batch', 'n_batches'), iter(_lists(fx, 'negs', 'n_negs'))
    monkeypatch.setattr(S, 'make_sampler', lambda d, batch_size, num_steps, walk_length=2: S.FixedNodeSets(d, sets))
    monkeypatch.setattr(S, 'negative_sampling', lambda ei, n, k: next(negs).to(ei.device))
    epochs = int(rest['epochs'])
    args = SimpleNamespace(unlearning_model='original', gnn='gcn', dataset='ogbl-synth', checkpoint_dir=str(tmp_path),
                           in_dim=w1.shape[1], hidden_dim=w1.shape[0], out_dim=w2.shape[0], eval_on_cpu=False, epochs=epochs,
                           valid_freq=epochs, lr=float(rest['lr']), batch_size=40, num_steps=len(sets), minibatch=True,
                           fused_minibatch=True)
    m = get_model(args)
    m.load_state_dict(state)
    opt = torch.optim.Adam(m.parameters(), lr=args.lr)
    tr = TB.Trainer(args)
    torch.manual_seed(int(rest['eval_seed']))
    tr.train(m, Data(data), opt, args)
    assert tr.trainer_log['minibatch_step'] == 'fused'
    steps = tr.trainer_log['steps']
    assert [set(s_) for s_ in steps] == [{'epoch', 'step', 'train_loss'}] * (epochs * len(sets))
    assert [(s_['epoch'], s_['step']) for s_ in steps] == [(e, i) for e in range(epochs) for i in range(len(sets))]
    np.testing.assert_allclose([s_['train_loss'] for s_ in steps], rest['train_loss'], rtol=1e-4)
    final = {k[len('final::'):]: v for k, v in fx.items() if k.startswith('final::')}
    for k, v in m.state_dict().items():
        assert rel_l2(v.cpu(), final[k]) < 1e-4, k
    vals = [r for r in tr.trainer_log['log'] if 'val_loss' in r]
    assert abs(vals[-1]['val_loss'] - float(rest['val_loss'][-1])) < 1e-4
    assert tr._fused_minibatch_step.cut.reads == epochs * len(sets)          # one blocking host read per batch
    assert all(p.grad is None for p in m.parameters())


# ------------------------------------------------------------------------------------------------ the seeded graph
N_NODES, N_EDGES, HUB, N_LONELY, HUB_DEG = 3000, 24000, 20, 20, 129


def _graph(in_dim, seed=13):
    """3,000 nodes and 24,000 random directed edges (multi-edges and self loops included) among nodes 21 .. n - 1; nodes
    0 .. 19 only have edges to nodes outside that range (no edge among the twenty); node 20, the hub, has exactly 129
    out-edges, to distinct nodes.  -> (data, the hub's targets)."""
    from gnndelete_amd.framework.data import Data
    g = torch.Generator().manual_seed(seed)
    ei = torch.randint(HUB + 1, N_NODES, (2, N_EDGES), generator=g)
    lonely = torch.stack([torch.randint(0, N_LONELY, (40,), generator=g), torch.randint(HUB + 1, N_NODES, (40,), generator=g)])
    targets = torch.randperm(N_NODES - 100, generator=g)[:HUB_DEG] + 100
    hub = torch.stack([torch.full_like(targets, HUB), targets])
    ei = torch.cat([ei, lonely, lonely.flip(0), hub], 1)
    d = Data(num_nodes=N_NODES, x=torch.randn(N_NODES, in_dim, generator=g), train_pos_edge_index=ei,
             dtrain_mask=torch.ones(ei.shape[1], dtype=torch.bool),
             val_pos_edge_index=torch.randint(0, N_NODES, (2, 300), generator=g),
             val_neg_edge_index=torch.randint(0, N_NODES, (2, 300), generator=g))
    d.dr_mask = d.dtrain_mask
    return d, targets


def _node_sets(targets, seed=5):
    g = torch.Generator().manual_seed(seed)
    pick = lambda k: torch.randperm(N_NODES, generator=g)[:k].sort().values
    return [pick(600), pick(600), pick(600), torch.arange(N_LONELY), torch.tensor([500]), pick(31), pick(33),
            torch.cat([torch.tensor([HUB]), targets]).sort().values]


def _counter_negatives():
    """A stand-in for sampler.negative_sampling whose k-th call depends on k alone (not on the global random stream)."""
    calls = [0]

    def draw(edge_index, num_nodes, num_neg_samples):
        calls[0] += 1
        g = torch.Generator().manual_seed(calls[0])
        return torch.randint(0, max(int(num_nodes), 1), (2, int(num_neg_samples)), generator=g).to(edge_index.device)
    return draw


def _train(tmp_path, monkeypatch, gnn, dims, fused, epochs=2, valid_freq=1, sets=None, negatives='sampler', model_state=None,
           optimizer_state=None, seed=1234):
    """Trainer.train on the seeded graph.  fused None: no fused_minibatch attribute at all.  negatives: 'sampler' (the
    module's own draws after torch.manual_seed(seed)) or a callable."""
    from gnndelete_amd.framework import get_model
    from gnndelete_amd.framework.trainer import base as TB
    from gnndelete_amd.framework.trainer import sampler as S
    data, targets = _graph(dims[0])
    sets = sets if sets is not None else _node_sets(targets)
    monkeypatch.setattr(S, 'make_sampler', lambda d, batch_size, num_steps, walk_length=2: S.FixedNodeSets(d, sets))
    if negatives != 'sampler':
        monkeypatch.setattr(S, 'negative_sampling', negatives)
    os.makedirs(str(tmp_path), exist_ok=True)
    args = SimpleNamespace(unlearning_model='original', gnn=gnn, dataset='ogbl-synth', checkpoint_dir=str(tmp_path),
                           in_dim=dims[0], hidden_dim=dims[1], out_dim=dims[2], eval_on_cpu=False, epochs=epochs,
                           valid_freq=valid_freq, lr=1e-2, batch_size=40, num_steps=len(sets), minibatch=True)
    if fused is not None:
        args.fused_minibatch = fused
    torch.manual_seed(77)
    m = get_model(args).cuda()
    if model_state is not None:
        m.load_state_dict(model_state)
    opt = torch.optim.Adam(m.parameters(), lr=args.lr)
    if optimizer_state is not None:
        opt.load_state_dict(optimizer_state)
    tr = TB.Trainer(args)
    torch.manual_seed(seed)
    tr.train(m, data, opt, args)
    return tr, m, opt, sets


def _losses(tr):
    return np.array([s_['train_loss'] for s_ in tr.trainer_log['steps']])


@pytest.mark.parametrize('dims', [(32, 32, 16), (12, 20, 8)], ids=['32-32-16', '12-20-8'])
@pytest.mark.parametrize('gnn', ['gcn', 'gat'])
def test_fused_step_matches_autograd_loop(gnn, dims, tmp_path, monkeypatch):
    ta, ma, oa, sets = _train(tmp_path / 'autograd', monkeypatch, gnn, dims, None)
    tf, mf, of, _ = _train(tmp_path / 'fused', monkeypatch, gnn, dims, True)
    assert 'minibatch_step' not in ta.trainer_log and tf.trainer_log['minibatch_step'] == 'fused'      # (no flag: nothing changes)
    a, f = _losses(ta), _losses(tf)
    print('losses', a, f)
    assert len(a) == len(f) == 2 * len(sets)
    assert np.array_equal(np.isfinite(a), np.isfinite(f)), (a, f)
    assert np.isnan(a).any(), 'the batches without an edge log the BCE of nothing'
    assert np.isnan(a[3]) and np.isnan(a[4]) and np.isfinite(a[[0, 1, 2, 7]]).all()
    np.testing.assert_allclose(f[np.isfinite(f)], a[np.isfinite(a)], rtol=1e-4)
    for (name, pa), pf in zip(ma.named_parameters(), mf.parameters()):
        sa, sf = oa.state[pa], of.state[pf]
        figures = (rel_l2(pf.detach().cpu(), pa.detach().cpu()), rel_l2(sf['exp_avg'].cpu(), sa['exp_avg'].cpu()),
                   rel_l2(sf['exp_avg_sq'].cpu(), sa['exp_avg_sq'].cpu()))
        print(name, figures)
        assert max(figures) < 1e-4, (name, figures)
        assert float(sa['step']) == float(sf['step']) == len(f)              # Adam stepped on the NaN batches too
        assert pa.grad is None and pf.grad is None
    for rec_a, rec_f in zip([r for r in ta.trainer_log['log'] if 'train_loss' in r],
                            [r for r in tf.trainer_log['log'] if 'train_loss' in r]):
        assert rec_a['epoch'] == rec_f['epoch'] and np.isnan(rec_a['train_loss']) and np.isnan(rec_f['train_loss'])
    assert ta.trainer_log['best_epoch'] == tf.trainer_log['best_epoch']
    assert abs(ta.trainer_log['best_valid_loss'] - tf.trainer_log['best_valid_loss']) < 1e-4
    assert tf._fused_minibatch_step.cut.reads == len(f)


def test_fused_step_is_reproducible(tmp_path, monkeypatch):
    out = []
    for _ in range(2):
        tr, m, _, _ = _train(tmp_path, monkeypatch, 'gat', (12, 20, 8), True)
        assert tr.trainer_log['minibatch_step'] == 'fused'
        out.append((_losses(tr), [p.detach().cpu().clone() for p in m.parameters()]))
    assert np.array_equal(out[0][0], out[1][0], equal_nan=True)
    assert all(torch.equal(p, q) for p, q in zip(out[0][1], out[1][1]))


@pytest.mark.parametrize('gnn', ['gcn', 'gat'])
def test_a_second_train_call_continues_the_first(gnn, tmp_path, monkeypatch):
    dims = (32, 32, 16)
    whole, mw, ow, _ = _train(tmp_path / 'whole', monkeypatch, gnn, dims, True, epochs=4, valid_freq=4,
                              negatives=_counter_negatives())
    draw = _counter_negatives()
    first, m1, _, _ = _train(tmp_path / 'first', monkeypatch, gnn, dims, True, epochs=2, valid_freq=2, negatives=draw)
    ckpt = torch.load(os.path.join(str(tmp_path / 'first'), 'model_final.pt'), map_location='cpu')
    assert set(ckpt) == {'model_state', 'optimizer_state'} and len(ckpt['optimizer_state']['state']) == len(list(m1.parameters()))
    second, m2, o2, _ = _train(tmp_path / 'second', monkeypatch, gnn, dims, True, epochs=2, valid_freq=2, negatives=draw,
                               model_state=ckpt['model_state'], optimizer_state=ckpt['optimizer_state'])
    assert np.array_equal(np.concatenate([_losses(first), _losses(second)]), _losses(whole), equal_nan=True)
    for pw, p2 in zip(mw.parameters(), m2.parameters()):
        assert torch.equal(pw.detach(), p2.detach())
        for k in ('exp_avg', 'exp_avg_sq'):
            assert torch.equal(ow.state[pw][k].cpu(), o2.state[p2][k].cpu()), k
        assert float(ow.state[pw]['step']) == float(o2.state[p2]['step']) == len(_losses(whole))


def test_checkpoints_hold_the_last_batch_embedding_and_the_optimizer_state(tmp_path, monkeypatch):
    tr, m, opt, sets = _train(tmp_path, monkeypatch, 'gcn', (32, 32, 16), True)
    z = torch.load(os.path.join(str(tmp_path), 'node_embeddings.pt'), map_location='cpu')
    assert tuple(z.shape) == (sets[-1].numel(), 16)                         # the z of the epoch's last batch
    best = torch.load(os.path.join(str(tmp_path), 'model_best.pt'), map_location='cpu')
    final = torch.load(os.path.join(str(tmp_path), 'model_final.pt'), map_location='cpu')
    n_params = len(list(m.parameters()))
    for ck in (best, final):
        assert set(ck) == {'model_state', 'optimizer_state'}
        assert len(ck['optimizer_state']['state']) == n_params
        assert all(set(s_) == {'step', 'exp_avg', 'exp_avg_sq'} for s_ in ck['optimizer_state']['state'].values())
    steps_at_best = (tr.trainer_log['best_epoch'] + 1) * len(sets)
    assert {float(s_['step']) for s_ in best['optimizer_state']['state'].values()} == {float(steps_at_best)}
    for k, v in m.state_dict().items():
        assert torch.equal(final['model_state'][k].cpu(), v.cpu())
    assert {'training_time', 'best_epoch', 'best_valid_loss', 'steps'} <= set(tr.trainer_log)


def test_gin_falls_back_with_the_reason(tmp_path, monkeypatch, capsys):
    sets = [s_ for i, s_ in enumerate(_node_sets(_graph(12)[1])) if i in (0, 1, 2, 7)]     # (batches with edges)
    res = []
    for fused in (None, True):
        tr, m, _, _ = _train(tmp_path, monkeypatch, 'gin', (12, 20, 8), fused, sets=sets, epochs=1)
        res.append((tr, [p.detach().cpu().clone() for p in m.parameters()]))
    out = capsys.readouterr().out
    line = '--fused_minibatch: no fused backbone batch step for the GIN backbone (GCN and GAT only); running the autograd ' \
           'mini-batch loop'
    assert out.count(line) == 1
    assert res[1][0].trainer_log['minibatch_step'] == 'autograd' and 'minibatch_step' not in res[0][0].trainer_log
    assert all(torch.equal(p, q) for p, q in zip(res[0][1], res[1][1]))
    assert np.array_equal(_losses(res[0][0]), _losses(res[1][0]), equal_nan=True)


def test_cli_fused_minibatch_agrees_with_autograd_loop(tmp_path, monkeypatch):
    import subprocess
    import sys
    monkeypatch.setenv('GNNDELETE_FORCE_EPOCHS', '2')
    monkeypatch.setenv('GNNDELETE_FORCE_VALID_FREQ', '2')
    monkeypatch.setenv('GNNDELETE_FORCE_NUM_STEPS', '3')
    from gnndelete_amd.framework.synth import make_linkpred_dataset
    data, df = make_linkpred_dataset(None, seed=42, shape=(800, 32, 4000, 'dense'))
    logs = {}
    # GCN without and with the flag, and GIN with it: the fall-back is the run whose log says 'autograd'
    for tag, gnn, flag in (('plain', 'gcn', []), ('fused', 'gcn', ['--fused_minibatch']), ('gin', 'gin', ['--fused_minibatch'])):
        cwd = str(tmp_path / tag)
        data_dir = os.path.join(cwd, 'data', 'ogbl-synth')
        os.makedirs(data_dir)
        data.save(os.path.join(data_dir, 'd_42.pt'))
        torch.save(df, os.path.join(data_dir, 'df_42.pt'))
        cmd = ['train_gnn.py', '--dataset', 'ogbl-synth', '--gnn', gnn, '--random_seed', '42', '--batch_size', '200',
               '--minibatch'] + flag
        r = subprocess.run([sys.executable, os.path.join(ROOT, cmd[0])] + cmd[1:], cwd=cwd, env=dict(os.environ, PYTHONPATH=ROOT),
                           capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        with open(os.path.join(cwd, 'checkpoint', 'ogbl-synth', gnn, 'original', '42', 'trainer_log.json')) as f:
            logs[tag] = json.load(f)
    assert 'minibatch_step' not in logs['plain'] and logs['fused']['minibatch_step'] == 'fused'
    assert logs['gin']['minibatch_step'] == 'autograd'
    assert len(logs['plain']['steps']) == len(logs['fused']['steps']) == 6
    assert abs(logs['plain']['best_valid_loss'] - logs['fused']['best_valid_loss']) < 1e-3
