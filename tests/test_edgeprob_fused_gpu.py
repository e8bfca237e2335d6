"""The fused edge-probability step (gnndelete_amd.edgeprob, --unlearning_model gnndelete --fused_edgeprob) through
GNNDeleteTrainer: the reference's golden trajectories, an fp64 loop written from the oracle's parts with negatives that
change every epoch (the fused path held to the project's fp32-spread convention against today's autograd path, and
against an fp32 ensemble of the oracle itself, which shares no kernel with it), the edge cases of the row lists,
reproducibility, the exported optimizer state, the fallback and the CLI.

Measured on an MI355X, rel-L2 to the fp64 loop over the fresh-negatives and the edge-case requests (GCN and GAT):
  weights   fused 6.6e-8 ... 8.2e-6   fp32 oracle ensemble 3.7e-8 ... 8.3e-6   (both largest on far_negative gcn, W_D2)
  moments   fused 1.1e-7 ... 5.4e-6   ensemble 1.2e-7 ... 5.4e-6
  losses    fused 3.2e-8 ... 2.8e-7   ensemble 2.6e-8 ... 4.3e-7
so the floors (5e-5 weights and moments, 1e-5 losses) decide every case here."""
import json
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from helpers import hip_model, load_golden, oracle_model, rel_l2, split_fixture, t

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLOOR = 5e-5                                  # tests/helpers.py: assert_del_weights_within_fp32_spread
CEILING = 1e-4                                # the golden trajectories' bound on the weights (first test below)
LOSS_FLOOR = 1e-5                             # tests/test_edgeprob_kernels_gpu.py: TOL, the kernel suite's bound on the loss values


# ------------------------------------------------------------------------------------------ golden trajectories
@pytest.mark.parametrize('gnn', ['gcn', 'gat'])
def test_fused_edgeprob_reproduces_reference_trajectory(tmp_path, monkeypatch, gnn):
    """test_cli_gpu.py::test_edgeprob_trainer_reproduces_reference_trajectory with the flag: same assertions, tolerances."""
    from gnndelete_amd.framework.data import Data
    from gnndelete_amd.framework.trainer import gnndelete as TE
    fx = load_golden(f'traj_edgeprob_{gnn}.npz')
    state, data, rest = split_fixture(fx)
    m = hip_model(gnn, state, data['sdf_node_1hop_mask'], data['sdf_node_2hop_mask'])
    neg = t(rest['neg']).cuda()
    monkeypatch.setattr(TE, 'negative_sampling', lambda **kw: neg)
    epochs = int(rest['epochs'])
    args = SimpleNamespace(unlearning_model='gnndelete', dataset='Cora', checkpoint_dir=str(tmp_path),
                           eval_on_cpu=False, epochs=epochs, valid_freq=1, lr=float(rest['lr']), fused_edgeprob=True)
    opt = torch.optim.Adam([p for n, p in m.named_parameters() if 'del' in n], lr=args.lr)
    tr = TE.GNNDeleteTrainer(args)
    torch.manual_seed(int(rest['eval_seed']))
    tr.train(m, Data(data), opt, args, logits_ori=t(rest['logits_ori']))
    assert tr.trainer_log['edgeprob_step'] == 'fused'
    logs = [r for r in tr.trainer_log['log'] if 'train_loss_l' in r]
    assert len(logs) == epochs
    assert set(logs[0]) >= {'train_loss', 'train_loss_l', 'train_loss_r', 'train_time'}
    np.testing.assert_allclose([r['train_loss'] for r in logs], rest['train_loss'], rtol=1e-4)
    np.testing.assert_allclose([r['train_loss_l'] for r in logs], rest['loss_l'], rtol=1e-4)
    np.testing.assert_allclose([r['train_loss_r'] for r in logs], rest['loss_r'], rtol=1e-4)
    assert rel_l2(m.deletion1.deletion_weight.detach().cpu(), rest['final_w1']) < 1e-4
    assert rel_l2(m.deletion2.deletion_weight.detach().cpu(), rest['final_w2']) < 1e-4
    for name in ('model_best.pt', 'model_final.pt'):
        ck = torch.load(os.path.join(str(tmp_path), name))
        assert 'optimizer_state' in ck and 'deletion1.deletion_weight' in ck['model_state']


# ------------------------------------------------------------------------------------------ seeded requests
def _request(n=400, f=32, n_edges=1600, n_df=20, seed=0, isolate=0):
    """A seeded unlearning request as delete_gnn.py prepares it: directed random edges a < b, n_df of them deleted (2 n_df
    directed Df edges after symmetrising), the 1-hop / 2-hop S_Df masks, a random [n, n] table of original logits."""
    from gnndelete_amd.framework.data import Data, prepare_edge_deletion
    g = torch.Generator().manual_seed(seed)
    e = torch.randint(0, n - isolate, (2, n_edges), generator=g)
    e = e[:, e[0] != e[1]]
    e = torch.unique(torch.stack([e.min(0).values, e.max(0).values]), dim=1)
    data = Data(num_nodes=n, x=torch.randn(n, f, generator=g), train_pos_edge_index=e)
    state = torch.get_rng_state()
    torch.manual_seed(seed + 1)
    data = prepare_edge_deletion(data, torch.ones(e.shape[1], dtype=torch.bool), n_df)
    torch.set_rng_state(state)
    logits_ori = torch.randn(n, n, generator=g)
    return data, logits_ori


def _negatives(data, epochs, seed):
    """A fresh negative list per epoch, drawn once and injected into every path."""
    from gnndelete_amd.framework import graph_utils as GU
    g = torch.Generator().manual_seed(seed)
    E = data['train_pos_edge_index']
    return [GU.negative_sampling(E, data['num_nodes'], int(data['df_mask'].sum()), generator=g) for _ in range(epochs)]


def _initial_state(gnn, data, hidden=32, out=16, seed=7):
    from gnndelete_amd.framework import models as M
    torch.manual_seed(seed)
    cls = {'gcn': M.GCNDelete, 'gat': M.GATDelete, 'gin': M.GINDelete}[gnn]
    m = cls(SimpleNamespace(in_dim=data['x'].shape[1], hidden_dim=hidden, out_dim=out), data['sdf_node_1hop_mask'],
            data['sdf_node_2hop_mask'])
    return {k: v.detach().clone() for k, v in m.state_dict().items()}


def _oracle_loop(gnn, state, data, logits_ori, negs, lr, dtype=torch.float64, perm=None):
    """The reference's epoch (oracle.gnndelete_ref.edgeprob_fullbatch) on the CPU in `dtype` with the negatives of each
    epoch.  perm = a seed: the S_Df edge list is permuted first - another summation order in every scatter of the forward
    and its backward, i.e. another correct implementation of the same arithmetic (helpers.oracle_runner's perm)."""
    from oracle import gnndelete_ref as R
    m1, m2 = data['sdf_node_1hop_mask'], data['sdf_node_2hop_mask']
    ref = oracle_model(gnn, state, m1, m2).to(dtype)
    E = data['train_pos_edge_index']
    df_edges, e_sdf = E[:, data['df_mask']], E[:, data['sdf_mask']]
    if perm is not None:
        e_sdf = e_sdf[:, torch.randperm(e_sdf.shape[1], generator=torch.Generator().manual_seed(perm))]
    pairs = R.sdf_pair_index(data['num_nodes'], m2, df_edges)
    ori_pairs = logits_ori.to(dtype)[pairs[0], pairs[1]]
    opt = torch.optim.Adam([p for n, p in ref.named_parameters() if 'del' in n], lr=lr)
    x = data['x'].to(dtype)
    losses = []
    for neg in negs:
        ref.train()
        z = ref(x, e_sdf)
        loss_r, loss_l = R.edgeprob_terms(ref, z, df_edges, neg, pairs, ori_pairs)
        loss = 0.5 * loss_r + 0.5 * loss_l
        loss.backward()
        opt.step()
        opt.zero_grad()
        losses.append([float(loss.detach()), float(loss_l.detach()), float(loss_r.detach())])
    with torch.no_grad():
        z1, z2 = ref(x, e_sdf, return_all_emb=True)
    return dict(w1=ref.deletion1.deletion_weight.detach(), w2=ref.deletion2.deletion_weight.detach(),
                losses=torch.tensor(losses, dtype=torch.float64), opt=opt, params=[ref.deletion1.deletion_weight,
                                                                                    ref.deletion2.deletion_weight],
                z1=z1, z2=z2, n_pairs=int(pairs.shape[1]))


def _fp64_loop(gnn, state, data, logits_ori, negs, lr):
    return _oracle_loop(gnn, state, data, logits_ori, negs, lr, torch.float64)


def _fp32_ensemble(gnn, state, data, logits_ori, negs, lr):
    """Three fp32 runs of the fp64 loop's own arithmetic, the S_Df edges in the given order and in two permuted ones:
    what fp32 can deliver on this request, measured on an implementation that shares no kernel with the step under test."""
    return [_oracle_loop(gnn, state, data, logits_ori, negs, lr, torch.float32, perm) for perm in (None, 1, 2)]


def _trainer_run(gnn, state, data, logits_ori, negs, lr, fused, tmp_path, monkeypatch, engine_kw=None, valid_freq=1, resume=None):
    """GNNDeleteTrainer.train on the HIP model with the epoch's negatives injected through the module-level seam.
    resume = an earlier run: a second train call on its model and its optimizer."""
    from gnndelete_amd.framework.data import Data
    from gnndelete_amd.framework.trainer import gnndelete as TE
    m = resume['model'] if resume else hip_model(gnn, state, data['sdf_node_1hop_mask'], data['sdf_node_2hop_mask'])
    os.makedirs(str(tmp_path), exist_ok=True)
    it = iter(negs)
    monkeypatch.setattr(TE, 'negative_sampling', lambda **kw: next(it).cuda())
    if engine_kw:
        from gnndelete_amd import edgeprob as EP
        orig = getattr(EP.EdgeprobEngine, 'wrapped', EP.EdgeprobEngine)
        with_kw = lambda *a, **k: orig(*a, **{**k, **engine_kw})
        with_kw.wrapped = orig
        monkeypatch.setattr(EP, 'EdgeprobEngine', with_kw)
    args = SimpleNamespace(unlearning_model='gnndelete', dataset='Cora', checkpoint_dir=str(tmp_path), eval_on_cpu=False,
                           epochs=len(negs), valid_freq=valid_freq, lr=lr, fused_edgeprob=fused)
    opt = resume['opt'] if resume else torch.optim.Adam([p for n, p in m.named_parameters() if 'del' in n], lr=lr)
    tr = TE.GNNDeleteTrainer(args)
    # the request has no validation split: the epoch records are what is under test, not Trainer.eval
    monkeypatch.setattr(tr, 'eval', lambda *a, **k: (0.0, 0.0, 0.0, 0.0, 0.0, [], None, {}))
    tr.train(m, Data({k: (v.clone() if torch.is_tensor(v) else v) for k, v in data.items()}), opt, args, logits_ori=logits_ori)
    logs = [r for r in tr.trainer_log['log'] if 'train_loss_l' in r]
    losses = torch.tensor([[r['train_loss'], r['train_loss_l'], r['train_loss_r']] for r in logs], dtype=torch.float64)
    return dict(w1=m.deletion1.deletion_weight.detach().cpu(), w2=m.deletion2.deletion_weight.detach().cpu(), losses=losses,
                opt=opt, params=[m.deletion1.deletion_weight, m.deletion2.deletion_weight], tr=tr, model=m,
                epochs=[r['epoch'] for r in logs])


def _distances(run, ref):
    d = {'W_D1': rel_l2(run['w1'], ref['w1']), 'W_D2': rel_l2(run['w2'], ref['w2'])}
    for k, name in enumerate(('loss', 'loss_l', 'loss_r')):
        if float(ref['losses'][:, k].abs().max()) > 0:
            d[name] = rel_l2(run['losses'][:, k], ref['losses'][:, k])
        else:
            assert float(run['losses'][:, k].abs().max()) == 0, name
    return d


def _assert_within_spread(tag, fused, autograd, ref):
    """The fused path's distance to fp64 <= max(2 x today's autograd path's, 5e-5), for both weights and the loss series."""
    df, da = _distances(fused, ref), _distances(autograd, ref)
    for k in df:
        print(f'[{tag}] {k}: rel-L2 to the fp64 loop: fused {df[k]:.2e} / autograd {da[k]:.2e}  (fused vs autograd '
              f'{rel_l2(fused["w1" if k == "W_D1" else "w2"], autograd["w1" if k == "W_D1" else "w2"]) if k.startswith("W") else float("nan"):.2e})')
    for k in df:
        assert df[k] <= max(2.0 * da[k], FLOOR), (tag, k, df[k], da[k])


def _moment_distances(run, ref):
    """rel-L2 of Adam's two moments of both weights to the fp64 loop's."""
    out = {}
    for k in (0, 1):
        have, want = run['opt'].state[run['params'][k]], ref['opt'].state[ref['params'][k]]
        for key in ('exp_avg', 'exp_avg_sq'):
            out[f'W_D{k + 1} {key}'] = rel_l2(have[key].detach().cpu(), want[key])
    return out


def _assert_within_ensemble(tag, fused, ens, ref, moments=True):
    """The fused path's distance to the fp64 loop <= max(2 x the largest distance of the fp32 oracle ensemble, floor), for
    both weights, the three loss series and (moments) Adam's moments.  floor = 5e-5 for the weights and the moments
    (helpers.assert_del_weights_within_fp32_spread), 1e-5 for the losses (the kernel suite's bound on these values).  The
    yardstick is the oracle alone: no kernel of the library runs in it.  Never above CEILING, whatever the ensemble does
    on the host at hand.  -> (the fused distances, the members')."""
    df, de = _distances(fused, ref), [_distances(e, ref) for e in ens]
    if moments:
        df.update(_moment_distances(fused, ref))
        for d, e in zip(de, ens):
            d.update(_moment_distances(e, ref))
    for k in df:
        print(f'[{tag}] {k}: rel-L2 to the fp64 loop: fused {df[k]:.2e} / fp32 oracle ensemble ' + ' '.join(f'{d[k]:.2e}' for d in de))
    for k in df:
        floor = LOSS_FLOOR if k.startswith('loss') else FLOOR
        assert df[k] <= min(max(2.0 * max(d[k] for d in de), floor), CEILING), (tag, k, df[k], [d[k] for d in de])
    return df, de


def _assert_rows_behave(run, ref, data):
    """Rows outside the Del lists pass through untouched (z1 = the frozen layer 1, z2 = conv2's output) and every row of
    the embeddings the final weights give - listed or not - is the fp64 loop's."""
    eng = run['tr']._edgeprob_engine
    m1, m2 = data['sdf_node_1hop_mask'].cuda(), data['sdf_node_2hop_mask'].cuda()
    assert torch.equal(eng.z1[~m1], eng.p1[~m1]) and torch.equal(eng.z2[~m2], eng.c2[~m2])
    E = data['train_pos_edge_index']
    with torch.no_grad():
        z1, z2 = run['model'](data['x'].cuda(), E[:, data['sdf_mask']].contiguous().cuda(), return_all_emb=True)
    # (1e-4: the golden trajectories' bound on the weights, which the embeddings are linear in; rows of z1 outside S1 are
    # the frozen layer 1 alone and are held to the kernel suite's 1e-5)
    assert rel_l2(z1.cpu(), ref['z1']) < 1e-4 and rel_l2(z2.cpu(), ref['z2']) < 1e-4
    assert rel_l2(z1[~m1].cpu(), ref['z1'][~m1.cpu()]) < 1e-5
    assert rel_l2(z2[~m2].cpu(), ref['z2'][~m2.cpu()]) < 1e-4
    assert bool(torch.isfinite(run['w1']).all()) and bool(torch.isfinite(run['w2']).all())


@pytest.mark.parametrize('gnn', ['gcn', 'gat'])
def test_fused_edgeprob_with_fresh_negatives_every_epoch(gnn, tmp_path, monkeypatch):
    data, logits_ori = _request()
    assert 30 <= int(data['df_mask'].sum()) <= 50
    negs = _negatives(data, 8, seed=3)
    assert not torch.equal(negs[0], negs[1])
    state = _initial_state(gnn, data)
    ref = _fp64_loop(gnn, state, data, logits_ori, negs, 1e-3)
    autograd = _trainer_run(gnn, state, data, logits_ori, negs, 1e-3, False, tmp_path / 'a', monkeypatch)
    fused = _trainer_run(gnn, state, data, logits_ori, negs, 1e-3, True, tmp_path / 'f', monkeypatch)
    assert fused['tr'].trainer_log['edgeprob_step'] == 'fused' and 'edgeprob_step' not in autograd['tr'].trainer_log
    _assert_within_spread(f'fresh negatives {gnn}', fused, autograd, ref)
    _assert_within_ensemble(f'fresh negatives {gnn}', fused, _fp32_ensemble(gnn, state, data, logits_ori, negs, 1e-3), ref)
    _assert_rows_behave(fused, ref, data)
    # optimizer state: the autograd path's step count, moments within the weights' bound
    sf, sa = fused['opt'].state_dict()['state'], autograd['opt'].state_dict()['state']
    assert sorted(sf) == sorted(sa) == [0, 1]
    for k in (0, 1):
        assert float(sf[k]['step']) == float(sa[k]['step']) == 8.0
        want = ref['opt'].state[ref['params'][k]]
        for key in ('exp_avg', 'exp_avg_sq'):
            d_f, d_a = rel_l2(sf[k][key].cpu(), want[key]), rel_l2(sa[k][key].cpu(), want[key])
            print(f'[optimizer state {gnn}] W_D{k + 1} {key}: fused {d_f:.2e} / autograd {d_a:.2e}')
            assert d_f <= max(2.0 * d_a, FLOOR), (k, key, d_f, d_a)
    assert all(p.grad is None for p in fused['params'])


def _edge_case(name):
    """-> (data, logits_ori, negatives or None (drawn), what must hold)."""
    if name == 'no_pairs':
        # S2 = the two ends of the one Df edge: its only pair is a Df pair
        data, ori = _request(n=120, n_edges=400, n_df=1, seed=11)
        df = data['train_pos_edge_index'][:, data['df_mask']]
        for key in ('sdf_node_1hop_mask', 'sdf_node_2hop_mask'):
            mask = torch.zeros(120, dtype=torch.bool)
            mask[df.flatten()] = True
            data[key] = mask
        return data, ori, None
    if name == 'far_negative':
        # nodes 110.. have no edge at all: outside S2 and outside every neighbourhood of S1
        data, ori = _request(n=120, n_edges=400, n_df=6, seed=12, isolate=10)
        negs = _negatives(data, 4, seed=5)
        for k, neg in enumerate(negs):
            neg[:, 0] = torch.tensor([111 + k, 115])
            neg[:, 1] = torch.tensor([int(data['sdf_node_1hop_mask'].nonzero()[0]), 117])
        assert not bool(data['sdf_node_2hop_mask'][110:].any())
        return data, ori, negs
    if name == 'single_s1':
        data, ori = _request(n=120, n_edges=400, n_df=4, seed=13)
        mask = torch.zeros(120, dtype=torch.bool)
        mask[int(data['sdf_node_1hop_mask'].nonzero()[0])] = True
        data['sdf_node_1hop_mask'] = mask
        return data, ori, None
    if name == 'odd_s2':
        data, ori = _request(n=120, n_edges=400, n_df=6, seed=14)
        keep = data['sdf_node_2hop_mask'].nonzero().flatten()[:37]
        assert keep.numel() == 37
        mask = torch.zeros(120, dtype=torch.bool)
        mask[keep] = True
        data['sdf_node_2hop_mask'] = mask
        return data, ori, None
    raise KeyError(name)


@pytest.mark.parametrize('gnn', ['gcn', 'gat'])
@pytest.mark.parametrize('name', ['no_pairs', 'far_negative', 'single_s1', 'odd_s2'])
def test_fused_edgeprob_edge_cases(name, gnn, tmp_path, monkeypatch):
    data, logits_ori, negs = _edge_case(name)
    negs = negs if negs is not None else _negatives(data, 4, seed=6)
    state = _initial_state(gnn, data)
    ref = _fp64_loop(gnn, state, data, logits_ori, negs, 1e-3)
    if name == 'no_pairs':
        assert ref['n_pairs'] == 0 and float(ref['losses'][:, 1].abs().max()) == 0
    else:
        assert ref['n_pairs'] > 0
    autograd = _trainer_run(gnn, state, data, logits_ori, negs, 1e-3, False, tmp_path / 'a', monkeypatch)
    fused = _trainer_run(gnn, state, data, logits_ori, negs, 1e-3, True, tmp_path / 'f', monkeypatch)
    assert fused['tr'].trainer_log['edgeprob_step'] == 'fused'
    _assert_within_spread(f'{name} {gnn}', fused, autograd, ref)
    _assert_within_ensemble(f'{name} {gnn}', fused, _fp32_ensemble(gnn, state, data, logits_ori, negs, 1e-3), ref)
    _assert_rows_behave(fused, ref, data)


@pytest.mark.parametrize('gnn', ['gcn', 'gat'])
def test_fused_edgeprob_eager_replay_and_rerun_agree_bit_for_bit(gnn, tmp_path, monkeypatch):
    data, logits_ori = _request(n=200, n_edges=700, n_df=8, seed=21)
    negs = _negatives(data, 5, seed=8)
    state = _initial_state(gnn, data)
    runs = [_trainer_run(gnn, state, data, logits_ori, negs, 1e-3, True, tmp_path / str(k), monkeypatch, engine_kw=kw)
            for k, kw in enumerate(({'use_graph': True}, {'use_graph': False}, {'use_graph': True}))]
    assert runs[0]['tr']._edgeprob_engine._graph is not None and runs[1]['tr']._edgeprob_engine._graph is None
    hist = [r['tr']._edgeprob_engine.loss_history() for r in runs]
    assert hist[0].shape == (5, 3) and not torch.equal(state['deletion2.deletion_weight'], runs[0]['w2'])
    for r, h in zip(runs[1:], hist[1:]):
        assert torch.equal(r['w1'], runs[0]['w1']) and torch.equal(r['w2'], runs[0]['w2']) and torch.equal(h, hist[0])
    assert torch.equal(hist[0].double(), runs[0]['losses'])          # the epoch records are the ring's rows


def test_fused_edgeprob_falls_back_for_gin(tmp_path, monkeypatch, capsys):
    data, logits_ori = _request(n=120, n_edges=400, n_df=4, seed=31)
    negs = _negatives(data, 2, seed=9)
    state = _initial_state('gin', data)
    run = _trainer_run('gin', state, data, logits_ori, negs, 1e-3, True, tmp_path / 'g', monkeypatch)
    out = capsys.readouterr().out
    assert '--fused_edgeprob: no fused edge-probability step for the GINDelete backbone' in out
    assert run['tr'].trainer_log['edgeprob_step'] == 'autograd' and not hasattr(run['tr'], '_edgeprob_engine')
    assert len(run['losses']) == 2 and bool(torch.isfinite(run['w2']).all())
    # without the flag the trainer does not even import the engine's module
    monkeypatch.delitem(sys.modules, 'gnndelete_amd.edgeprob', raising=False)
    plain = _trainer_run('gcn', _initial_state('gcn', data), data, logits_ori, negs, 1e-3, False, tmp_path / 'p', monkeypatch)
    assert 'gnndelete_amd.edgeprob' not in sys.modules and 'edgeprob_step' not in plain['tr'].trainer_log


def test_cli_fused_edgeprob(tmp_path):
    cwd = str(tmp_path)
    env = dict(os.environ, PYTHONPATH=ROOT)

    def run(cmd):
        r = subprocess.run([sys.executable] + cmd, cwd=cwd, env=env, capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    common = ['--dataset', 'synth-tiny', '--gnn', 'gcn', '--random_seed', '42']
    run([os.path.join(ROOT, 'prepare_dataset.py'), '--dataset', 'synth-tiny', '--seeds', '42'])
    run([os.path.join(ROOT, 'train_gnn.py')] + common + ['--epochs', '30', '--valid_freq', '10'])
    run([os.path.join(ROOT, 'delete_gnn.py')] + common + ['--unlearning_model', 'gnndelete', '--df', 'in', '--df_size', '5',
                                                          '--epochs', '20', '--valid_freq', '10', '--fused_edgeprob'])
    out = os.path.join(cwd, 'checkpoint', 'synth-tiny', 'gcn', 'gnndelete', 'mse_mean-both_layerwise-0.5-non_connected', 'in-5.0-42')
    with open(os.path.join(out, 'trainer_log.json')) as f:
        log = json.load(f)
    assert log['edgeprob_step'] == 'fused' and len(log['log']) >= 2
    assert {'train_loss', 'train_loss_l', 'train_loss_r', 'train_time'} <= set(log['log'][0]) | set(log['log'][1])
    ck = torch.load(os.path.join(out, 'model_final.pt'))
    for k in ('deletion1.deletion_weight', 'deletion2.deletion_weight'):
        w = ck['model_state'][k]
        assert bool(torch.isfinite(w).all()) and not torch.equal(w, torch.full_like(w, 1e-3)), k
    assert float(ck['optimizer_state']['state'][0]['step']) == 20.0
