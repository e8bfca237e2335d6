"""The fused edge-probability GraphSAINT batch step (gnndelete_amd.minibatch.MinibatchEdgeprobStep, --unlearning_model
gnndelete --minibatch --fused_minibatch): its trajectory against the reference's (tests/golden/traj_edgeprob_minibatch_*.npz,
at the bounds tests/test_cli_gpu.py holds the autograd loop to on the same files) and against the autograd mini-batch loop,
edge-case batches included; reproducibility; the fall-backs; one CLI run."""
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from helpers import hip_model, load_golden, rel_l2, split_fixture, t

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ('loss', 'loss_e', 'loss_l')


def _lists(fx, prefix, count_key):
    return [t(fx[f'{prefix}::{i}']) for i in range(int(fx[count_key]))]


def _run(tmp_path, monkeypatch, gnn, fused, sets=None, negs=True, model=None, um='gnndelete', flag=True):
    """GNNDeleteTrainer.train on the fixture's graph: the fixture's node sets and negatives unless given others
    (negs=False: sampler.negative_sampling's own draws).  fused None: no fused_minibatch attribute at all."""
    from gnndelete_amd.framework.data import Data
    from gnndelete_amd.framework.trainer import gnndelete as TG
    from gnndelete_amd.framework.trainer import sampler as S
    fx = load_golden(f'traj_edgeprob_minibatch_{gnn if gnn in ("gcn", "gat") else "gcn"}.npz')
    state, data, rest = split_fixture(fx)
    m = model if model is not None else hip_model(gnn, state, data['sdf_node_1hop_mask'], data['sdf_node_2hop_mask'])
    sets = sets if sets is not None else _lists(fx, 'batch', 'n_batches')
    monkeypatch.setattr(S, 'make_sampler', lambda d, batch_size, num_steps, walk_length=2: S.FixedNodeSets(d, sets))
    if negs:
        it = iter(_lists(fx, 'negs', 'n_negs'))
        monkeypatch.setattr(S, 'negative_sampling', lambda ei, n, k: next(it).to(ei.device))
    epochs = int(rest['epochs'])
    os.makedirs(str(tmp_path), exist_ok=True)
    args = SimpleNamespace(unlearning_model=um, dataset='ogbl-synth', checkpoint_dir=str(tmp_path), eval_on_cpu=False,
                           epochs=epochs, valid_freq=epochs, lr=float(rest['lr']), gnn=gnn, batch_size=40, num_steps=len(sets),
                           minibatch=True)
    if fused is not None:
        args.fused_minibatch = fused
    opt = torch.optim.Adam([{'params': [p for n_, p in m.named_parameters() if 'del' in n_], 'weight_decay': 0.0}], lr=args.lr)
    tr = TG.GNNDeleteTrainer(args)
    torch.manual_seed(int(rest['eval_seed']))
    data.pop('dtrain_mask', None)                                     # the trainer defaults it to dr_mask
    tr.train(m, Data(data), opt, args)
    return tr, m, opt, rest, len(sets)


@pytest.mark.parametrize('gnn', ['gcn', 'gat'])
def test_fused_step_reproduces_reference_trajectory(gnn, tmp_path, monkeypatch):
    tr, m, _, rest, n_sets = _run(tmp_path, monkeypatch, gnn, True)
    assert tr.trainer_log['minibatch_step'] == 'fused'
    epochs = int(rest['epochs'])
    assert len(tr.trainer_log['steps']) == epochs * n_sets
    assert tr._fused_minibatch_step.cut.reads == epochs * n_sets          # one blocking host read per batch
    logged = [r for r in tr.trainer_log['log'] if 'train_loss' in r][-1]
    for key in ['train_loss', 'train_loss_l', 'train_loss_e']:
        np.testing.assert_allclose(logged[key], rest['log_' + key][-1], rtol=1e-4, atol=1e-9, err_msg=key)
    assert rel_l2(m.deletion1.deletion_weight.detach().cpu(), rest['final_w1']) < 1e-4
    assert rel_l2(m.deletion2.deletion_weight.detach().cpu(), rest['final_w2']) < 1e-4
    vals = [r for r in tr.trainer_log['log'] if 'val_dt_auc' in r]
    assert abs(vals[-1]['val_dt_auc'] - float(rest['val_dt_auc'][-1])) < 2e-3
    assert abs(vals[-1]['val_df_auc'] - float(rest['val_df_auc'][-1])) < 2e-3
    assert m.deletion1.deletion_weight.grad is None and m.deletion2.deletion_weight.grad is None


def _edge_case_sets(gnn):
    """The fixture's node sets plus a batch without a Df edge, a batch of nodes that share no edge and a batch without
    an S1 row."""
    fx = load_golden(f'traj_edgeprob_minibatch_{gnn}.npz')
    _, data, _ = split_fixture(fx)
    n = int(data['x'].shape[0])
    ei = data['train_pos_edge_index']
    df_nodes = set(ei[:, data['df_mask']].flatten().tolist())
    no_df = torch.tensor([v for v in range(n) if v not in df_nodes][:60])
    adj = {(int(a), int(b)) for a, b in ei.t().tolist()}
    lonely = []
    for v in range(n):                                              # greedy independent set: no edge inside it, no self loop
        if (v, v) not in adj and all((v, u) not in adj and (u, v) not in adj for u in lonely):
            lonely.append(v)
        if len(lonely) == 12:
            break
    no_s1 = (~data['sdf_node_1hop_mask']).nonzero().flatten()[:60]
    return _lists(fx, 'batch', 'n_batches') + [no_df.sort().values, torch.tensor(lonely), no_s1.sort().values]


@pytest.mark.parametrize('gnn', ['gcn', 'gat'])
def test_fused_step_matches_autograd_loop(gnn, tmp_path, monkeypatch):
    sets = _edge_case_sets(gnn)
    runs = []
    for fused in (False, True):
        torch.manual_seed(1234)                         # negatives from sampler.negative_sampling: the same draws
        runs.append(_run(tmp_path / ('fused' if fused else 'autograd'), monkeypatch, gnn, fused, sets=sets, negs=False))
    (ta, ma, oa, _, _), (tf, mf, of, _, _) = runs
    assert 'minibatch_step' not in ta.trainer_log and tf.trainer_log['minibatch_step'] == 'fused'   # (no flag: nothing changes)
    assert len(ta.trainer_log['steps']) == len(tf.trainer_log['steps'])
    for key in KEYS:
        a = np.array([s_[key] for s_ in ta.trainer_log['steps']])
        f = np.array([s_[key] for s_ in tf.trainer_log['steps']])
        assert np.array_equal(np.isfinite(a), np.isfinite(f)), (key, a, f)
        np.testing.assert_allclose(f[np.isfinite(f)], a[np.isfinite(a)], rtol=1e-4, atol=1e-9, err_msg=key)
    assert any(np.isnan(s_['loss']) for s_ in ta.trainer_log['steps']), 'the edge-case batches log the MSE of nothing'
    for name in ('deletion1', 'deletion2'):
        pa, pf = getattr(ma, name).deletion_weight, getattr(mf, name).deletion_weight
        assert rel_l2(pf.detach().cpu(), pa.detach().cpu()) < 1e-4, name
        sa, sf = oa.state[pa], of.state[pf]
        assert float(sa['step']) == float(sf['step']) == len(tf.trainer_log['steps'])
        for k in ['exp_avg', 'exp_avg_sq']:
            assert rel_l2(sf[k].cpu(), sa[k].cpu()) < 1e-4, (name, k)
        assert pa.grad is None and pf.grad is None
    for name in ('model_best.pt', 'model_final.pt'):
        ca = torch.load(os.path.join(str(tmp_path / 'autograd'), name), map_location='cpu')
        cf = torch.load(os.path.join(str(tmp_path / 'fused'), name), map_location='cpu')
        assert set(ca) == set(cf) == {'model_state', 'optimizer_state'}, name
        assert set(ca['optimizer_state']) == set(cf['optimizer_state'])
        assert set(ca['optimizer_state']['state']) == set(cf['optimizer_state']['state']) == {0, 1}
        for i in (0, 1):
            assert set(ca['optimizer_state']['state'][i]) == set(cf['optimizer_state']['state'][i])
            assert float(ca['optimizer_state']['state'][i]['step']) == float(cf['optimizer_state']['state'][i]['step'])
    za = torch.load(os.path.join(str(tmp_path / 'autograd'), 'node_embeddings.pt'), map_location='cpu')
    zf = torch.load(os.path.join(str(tmp_path / 'fused'), 'node_embeddings.pt'), map_location='cpu')
    assert za.shape == zf.shape and rel_l2(zf, za) < 1e-4                       # the last batch's z


def test_fused_step_is_reproducible(tmp_path, monkeypatch):
    sets = _edge_case_sets('gat')
    out = []
    for _ in range(2):
        torch.manual_seed(99)
        tr, m, _, _, _ = _run(tmp_path, monkeypatch, 'gat', True, sets=sets, negs=False)
        assert tr.trainer_log['minibatch_step'] == 'fused'
        out.append((np.array([[s_[k] for k in KEYS] for s_ in tr.trainer_log['steps']]),
                    m.deletion1.deletion_weight.detach().cpu().clone(), m.deletion2.deletion_weight.detach().cpu().clone()))
    assert np.array_equal(out[0][0], out[1][0], equal_nan=True)
    assert torch.equal(out[0][1], out[1][1]) and torch.equal(out[0][2], out[1][2])


def _fallback_runs(tmp_path, monkeypatch, make_model, um):
    res = []
    for fused in (None, True):
        torch.manual_seed(3)
        m = make_model()
        torch.manual_seed(5)
        tr, m, _, _, _ = _run(tmp_path, monkeypatch, 'gcn', fused, negs=False, model=m, um=um)
        res.append((tr, m.deletion1.deletion_weight.detach().cpu().clone(), m.deletion2.deletion_weight.detach().cpu().clone()))
    return res


def test_gin_falls_back_with_the_reason(tmp_path, monkeypatch, capsys):
    from gnndelete_amd.framework import models as M
    _, data, _ = split_fixture(load_golden('traj_edgeprob_minibatch_gcn.npz'))
    make = lambda: M.GINDelete(SimpleNamespace(in_dim=data['x'].shape[1], hidden_dim=32, out_dim=16), data['sdf_node_1hop_mask'],
                               data['sdf_node_2hop_mask']).cuda()
    plain, flagged = _fallback_runs(tmp_path, monkeypatch, make, 'gnndelete')
    assert '--fused_minibatch: no fused edge-probability batch step for the GINDelete backbone (GCN and GAT only); running the ' \
           'autograd mini-batch loop' in capsys.readouterr().out
    assert flagged[0].trainer_log['minibatch_step'] == 'autograd' and 'minibatch_step' not in plain[0].trainer_log
    assert torch.equal(plain[1], flagged[1]) and torch.equal(plain[2], flagged[2])
    assert np.array_equal(np.array([[s_[k] for k in KEYS] for s_ in plain[0].trainer_log['steps']]),
                          np.array([[s_[k] for k in KEYS] for s_ in flagged[0].trainer_log['steps']]), equal_nan=True)


def test_kld_model_name_falls_back_with_the_reason(tmp_path, monkeypatch, capsys):
    fx = load_golden('traj_edgeprob_minibatch_gcn.npz')
    state, data, _ = split_fixture(fx)
    make = lambda: hip_model('gcn', state, data['sdf_node_1hop_mask'], data['sdf_node_2hop_mask'])
    plain, flagged = _fallback_runs(tmp_path, monkeypatch, make, 'gnndelete_kld')
    assert '--fused_minibatch: --unlearning_model gnndelete_kld is not the MSE loss; running the autograd mini-batch loop' \
        in capsys.readouterr().out
    assert flagged[0].trainer_log['minibatch_step'] == 'autograd'
    assert torch.equal(plain[1], flagged[1]) and torch.equal(plain[2], flagged[2])


def test_cli_fused_minibatch_agrees_with_autograd_loop(tmp_path, monkeypatch):
    import subprocess
    import sys
    monkeypatch.setenv('GNNDELETE_FORCE_EPOCHS', '2')
    monkeypatch.setenv('GNNDELETE_FORCE_VALID_FREQ', '2')
    monkeypatch.setenv('GNNDELETE_FORCE_NUM_STEPS', '3')
    from gnndelete_amd.framework.synth import make_linkpred_dataset
    data, df = make_linkpred_dataset(None, seed=42, shape=(800, 32, 4000, 'dense'))
    logs = []
    cwd = str(tmp_path)
    data_dir = os.path.join(cwd, 'data', 'ogbl-synth')
    os.makedirs(data_dir)
    data.save(os.path.join(data_dir, 'd_42.pt'))
    torch.save(df, os.path.join(data_dir, 'df_42.pt'))
    common = ['--dataset', 'ogbl-synth', '--gnn', 'gcn', '--random_seed', '42', '--batch_size', '200']
    delete = ['delete_gnn.py'] + common + ['--unlearning_model', 'gnndelete', '--df', 'in', '--df_size', '5', '--minibatch']
    env = dict(os.environ, PYTHONPATH=ROOT)
    # one original model; the two requests write the same checkpoint directory, so each log is read before the next run
    for cmd in (['train_gnn.py'] + common, delete, delete + ['--fused_minibatch']):
        r = subprocess.run([sys.executable, os.path.join(ROOT, cmd[0])] + cmd[1:], cwd=cwd, env=env, capture_output=True,
                           text=True, timeout=900)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        if cmd[0] == 'train_gnn.py':
            continue
        found = [os.path.join(b, 'trainer_log.json') for b, _, fs in os.walk(os.path.join(cwd, 'checkpoint', 'ogbl-synth', 'gcn',
                                                                                         'gnndelete')) if 'trainer_log.json' in fs]
        assert len(found) == 1, found
        with open(found[0]) as f:
            logs.append(json.load(f))
    assert logs[0].get('minibatch_step') is None and logs[1]['minibatch_step'] == 'fused'
    assert len(logs[0]['steps']) == len(logs[1]['steps']) == 6
    for key in KEYS:
        a, f = (np.array([s_[key] for s_ in lg['steps']], dtype=np.float64) for lg in logs)
        assert np.array_equal(np.isfinite(a), np.isfinite(f)), key
        np.testing.assert_allclose(f[np.isfinite(f)], a[np.isfinite(a)], rtol=1e-4, atol=1e-9, err_msg=key)
    assert abs(logs[0]['dt_auc'] - logs[1]['dt_auc']) < 2e-3 and abs(logs[0]['df_auc'] - logs[1]['df_auc']) < 2e-3
