"""The fused node-classification step (gnndelete_amd.backbone.NodeClassifierEngine, train_node.py --fused_backbone) through
NodeClassificationTrainer.train: the reference's golden trajectories (with the flag, and without it: today's loop), seeded
requests against an fp64 loop over the oracle's TwoLayer (held to what an fp32 ensemble of the same loop delivers, and to
today's autograd path: test_backbone_fused_gpu._assert_within_ensemble's rule and numbers), the zero padding of the layer-2
shadows, the edge cases of the train mask and the labels, reproducibility, resuming, the fallbacks and the CLI.

The seeded requests use lr 1e-3 and request seed 3.  Adam divides every element's step by the size of its own gradient
history, so an element whose gradient is within rounding of zero moves by rounding noise at full step size, in any fp32
implementation.  Where a request has such an element the comparison measures that element, not the step: at lr 1e-2 the
(32, 128, 40) GCN request has a ReLU gate that flips (fp32 oracle ensemble 2e-3); with request seed 0 the ensemble itself reaches
7e-5 on the (100, 64, 7) GCN request; with request seed 2 one element of GAT's W2 at (32, 128, 40) - row 5, column 51 of 5,120 -
carries 98 % of the squared distance of today's autograd path (5.3e-5 on that update, every other quantity below 8e-6) and 97 %
of the fused step's (9.2e-6), measured on an MI355X.  With seed 3 the ensemble stays below 1e-5 on every quantity of every
request here (computed on the CPU), so the floors decide.

Measured on an MI355X, rel-L2 to the fp64 loop over the seeded requests (five shapes) and the edge cases, GCN and GAT:
  parameters  fused 2.1e-8 ... 1.9e-6   fp32 oracle ensemble 2.1e-8 ... 3.0e-6   today's autograd path 2.1e-8 ... 6.4e-6
  updates     fused 4.3e-8 ... 8.7e-6   ensemble 2.3e-8 ... 1.6e-5               autograd 4.1e-8 ... 9.3e-6
  moments     fused 6.6e-8 ... 5.5e-6   ensemble 3.0e-8 ... 1.3e-5               autograd 1.4e-7 ... 1.9e-6
  losses      fused 1.6e-8 ... 2.8e-7   ensemble 3.4e-8 ... 3.2e-7               autograd 4.0e-8 ... 7.6e-8"""
import functools
import json
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from helpers import load_golden, rel_l2, split_fixture
from test_backbone_fused_gpu import (_assert_checkpoint_has_moments, _assert_within_ensemble, _initial_state, _request,
                                     _result)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W_KEY = {'gcn': 'conv1.lin.weight', 'gat': 'conv1.lin_src.weight'}
EPOCHS, LR = 8, 1e-3


# ------------------------------------------------------------------------------------------ golden trajectories
@pytest.mark.parametrize('fused', [True, False], ids=['fused', 'loop'])
@pytest.mark.parametrize('tag', ['gcn', 'gat', 'gcn_c3'])
def test_node_classifier_reproduces_reference_training(tmp_path, tag, fused):
    """The reference's real NodeClassificationTrainer.train (tests/golden/make_golden_nodecls_orig.py) with the flag, and
    without it (today's loop on the same fixtures)."""
    from gnndelete_amd.framework import get_model
    from gnndelete_amd.framework.data import Data
    from gnndelete_amd.framework.trainer import base as TB
    gnn = tag.split('_')[0]
    fx = load_golden(f'orig_nodecls_{tag}.npz')
    state, data, rest = split_fixture(fx)
    key = W_KEY[gnn]
    key2 = key.replace('conv1', 'conv2')
    classes = int(rest['classes'])
    assert state[key2].shape[0] == classes and classes == (3 if tag == 'gcn_c3' else 4)
    args = SimpleNamespace(unlearning_model='original_node', gnn=gnn, dataset='DBLP', checkpoint_dir=str(tmp_path),
                           in_dim=state[key].shape[1], hidden_dim=state[key].shape[0], out_dim=classes, eval_on_cpu=False,
                           epochs=int(rest['epochs']), valid_freq=int(rest['valid_freq']), lr=float(rest['lr']),
                           **({'fused_backbone': True} if fused else {}))
    m = get_model(args)
    res = m.load_state_dict(state, strict=False)
    assert not res.unexpected_keys and not [k for k in res.missing_keys if 'lin_dst' not in k]
    opt = torch.optim.Adam(m.parameters(), lr=args.lr)
    tr = TB.NodeClassificationTrainer(args)
    tr.train(m, Data(data), opt, args)
    assert tr.trainer_log.get('backbone_step') == ('fused' if fused else None)
    logs = [r for r in tr.trainer_log['log'] if 'train_loss' in r]
    vals = [r for r in tr.trainer_log['log'] if 'val_dt_acc' in r]
    assert [r['epoch'] for r in logs] == [2, 5]
    print(tag, fused, [r['train_loss'] for r in logs], rest['train_loss'])
    np.testing.assert_allclose([r['train_loss'] for r in logs], rest['train_loss'], rtol=1e-4)
    assert [r['val_dt_acc'] for r in vals] == [float(v) for v in rest['val_dt_acc']]
    assert [r['val_dt_f1'] for r in vals] == [float(v) for v in rest['val_dt_f1']]
    np.testing.assert_allclose([r['val_loss'] for r in vals], rest['val_loss'], rtol=1e-4)
    final = {k[len('final::'):]: v for k, v in fx.items() if k.startswith('final::')}
    checked = 0
    for k, v in m.state_dict().items():
        if k in final:
            print(tag, fused, k, rel_l2(v.cpu(), final[k]))
            assert rel_l2(v.cpu(), final[k]) < 1e-4, k
            checked += 1
    assert checked >= 4
    for name in ('model_best.pt', 'model_final.pt'):
        _assert_checkpoint_has_moments(os.path.join(str(tmp_path), name), m)
    assert float(torch.load(os.path.join(str(tmp_path), 'model_final.pt'))['optimizer_state']['state'][0]['step']) == args.epochs
    z = torch.load(os.path.join(str(tmp_path), 'node_embeddings.pt'))
    assert z.shape == (data['num_nodes'], classes) and bool(torch.isfinite(z).all())
    assert float((z.double().exp().sum(1) - 1).abs().max()) < 1e-5
    assert all(p.grad is None for p in m.parameters())
    best_epoch, best_acc = 0, 0
    for ep, acc in zip((2, 5), rest['val_dt_acc']):                            # model selection by dt_acc, as the loop's
        if float(acc) > best_acc:
            best_epoch, best_acc = ep, float(acc)
    assert tr.trainer_log['best_epoch'] == best_epoch and tr.trainer_log['best_valid_acc'] == best_acc


# ------------------------------------------------------------------------------------------ seeded requests
def _nodecls_request(f, classes, case='plain', n=400, seed=3):
    """test_backbone_fused_gpu._request (400 nodes, node 0 a hub of 80, three isolated nodes) with labels and a train mask of
    about 60 % of the nodes, node 0 and an isolated node included."""
    req = _request(f=f, n=n, seed=seed)
    g = torch.Generator().manual_seed(seed + 100)
    y = torch.randint(0, classes, (n,), generator=g)
    mask = torch.rand(n, generator=g) < 0.6
    mask[0] = mask[n - 1] = True
    if case == 'one_row':
        mask[:] = False
        mask[0] = True                         # the hub: the row with the longest aggregation and attention softmax
    elif case == 'every_row':
        mask[:] = True
    elif case == 'one_class':
        y[:] = classes - 1
    return {'num_nodes': n, 'x': req['x'], 'edge_index': req['train_pos_edge_index'], 'y': y, 'train_mask': mask,
            'val_mask': ~mask}


def _oracle_loop(gnn, dims, state, req, epochs=EPOCHS, lr=LR, dtype=torch.float64, perm=None):
    """NodeClassificationTrainer.train without validation on the oracle's TwoLayer, on the CPU in `dtype`.  perm = a seed: the
    edge list is permuted first - another summation order in every scatter, another correct implementation."""
    from oracle import gnndelete_ref as R
    torch.set_num_threads(min(32, torch.get_num_threads()))
    ref = R.TwoLayer(gnn, *dims)
    missing = ref.load_state_dict(state, strict=False)
    assert not missing.unexpected_keys and not [k for k in missing.missing_keys if 'lin_dst' not in k]
    ref = ref.to(dtype)
    x, E, y, mask = req['x'].to(dtype), req['edge_index'], req['y'], req['train_mask']
    if perm is not None:
        E = E[:, torch.randperm(E.shape[1], generator=torch.Generator().manual_seed(perm))]
    opt = torch.optim.Adam(ref.parameters(), lr=lr)
    losses = []
    for _ in range(epochs):
        ref.train()
        z = F.log_softmax(ref(x, E), dim=1)
        loss = F.nll_loss(z[mask], y[mask])
        loss.backward()
        opt.step()
        opt.zero_grad()
        losses.append(float(loss.detach()))
    return _result(ref, opt, losses, state)


@functools.lru_cache(maxsize=None)
def _references(gnn, dims, case='plain'):
    """(request, initial state, fp64 loop, fp32 ensemble): computed once, shared, never changed."""
    req = _nodecls_request(dims[0], dims[2], case)
    state = _initial_state(gnn, dims)
    ref = _oracle_loop(gnn, dims, state, req)
    ens = [_oracle_loop(gnn, dims, state, req, dtype=torch.float32, perm=perm) for perm in (None, 1, 2)]
    return req, state, ref, ens


def _trainer_run(gnn, dims, state, req, fused, tmp_path, monkeypatch, epochs=EPOCHS, lr=LR, engine_kw=None, resume=None,
                 make_opt=None):
    """NodeClassificationTrainer.train on the HIP model, one record per epoch.  resume = an earlier run: a second train call on
    its model and its optimizer."""
    from gnndelete_amd.framework import models as M
    from gnndelete_amd.framework.data import Data
    from gnndelete_amd.framework.trainer import base as TB
    if resume:
        m = resume['model']
    else:
        m = {'gcn': M.GCN, 'gat': M.GAT, 'gin': M.GIN, 'sage': M.SAGE}[gnn](SimpleNamespace(in_dim=dims[0], hidden_dim=dims[1],
                                                                                            out_dim=dims[2]))
        m.load_state_dict(state)
        m = m.cuda()
    os.makedirs(str(tmp_path), exist_ok=True)
    if engine_kw:
        from gnndelete_amd import backbone as BB
        orig = getattr(BB.NodeClassifierEngine, 'wrapped', BB.NodeClassifierEngine)
        with_kw = lambda *a, **k: orig(*a, **{**k, **engine_kw})
        with_kw.wrapped = orig
        monkeypatch.setattr(BB, 'NodeClassifierEngine', with_kw)
    args = SimpleNamespace(unlearning_model='original_node', gnn=gnn, dataset='DBLP', checkpoint_dir=str(tmp_path),
                           eval_on_cpu=False, epochs=epochs, valid_freq=1, lr=lr, **({'fused_backbone': True} if fused else {}))
    opt = resume['opt'] if resume else (make_opt or (lambda ps: torch.optim.Adam(ps, lr=lr)))(list(m.parameters()))
    tr = TB.NodeClassificationTrainer(args)
    # the epoch records are what is under test, not NodeClassificationTrainer.eval
    monkeypatch.setattr(tr, 'eval', lambda *a, **k: (0.0, 0.0, 0.0, {}))
    tr.train(m, Data({k: (v.clone() if torch.is_tensor(v) else v) for k, v in req.items()}), opt, args)
    losses = [r['train_loss'] for r in tr.trainer_log['log'] if 'train_loss' in r]
    out = _result(m, opt, losses, state) if isinstance(opt, torch.optim.Adam) else {'losses': torch.as_tensor(losses, dtype=torch.float64)}
    out.update(tr=tr, model=m, opt=opt)
    return out


def _assert_padding_is_zero(eng, classes):
    """The padding blocks of every layer-2 shadow and of its two moments are exactly zero; the model's own tensors are the
    shadows' top-left blocks."""
    from gnndelete_amd.backbone import padded_class_width
    names = [k for k, _ in eng.model.named_parameters()]
    if padded_class_width(classes) == classes:
        assert eng.shadows == {} and all(p is q for p, q in zip(eng.params, eng.user_params))
        return
    assert sorted(eng.shadows) == sorted(k for k in names if k.startswith('conv2.')) and len(eng.shadows) == (4 if eng.gat else 2)
    for k, p, q, st in zip(names, eng.params, eng.user_params, eng.adam):
        if not k.startswith('conv2.'):
            assert p is q
            continue
        assert p is eng.shadows[k] and p.shape != q.shape and padded_class_width(classes) in p.shape
        block = tuple(slice(0, s) for s in q.shape)
        for tensor in (p.data, st['m'], st['v']):
            pad = tensor.clone()
            assert float(pad[block].abs().max()) > 0, k
            pad[block] = 0
            assert not bool(pad.any()), k                          # exactly zero
        assert torch.equal(p.data[block], q.data), k


DIMS = [(32, 32, 4), (32, 32, 3), (100, 64, 7), (100, 64, 32), (32, 128, 40)]


@pytest.mark.parametrize('dims', DIMS, ids=['-'.join(map(str, d)) for d in DIMS])
@pytest.mark.parametrize('gnn', ['gcn', 'gat'])
def test_fused_node_classifier_against_the_fp64_loop(gnn, dims, tmp_path, monkeypatch):
    req, state, ref, ens = _references(gnn, dims)
    deg = torch.bincount(req['edge_index'][0], minlength=400)
    share = float(req['train_mask'].float().mean())
    assert int(deg[0]) == 80 and int((deg == 0).sum()) >= 3 and int(deg[399]) == 0 and 0.5 < share < 0.7
    assert bool(req['train_mask'][0]) and bool(req['train_mask'][399])
    autograd = _trainer_run(gnn, dims, state, req, False, tmp_path / 'a', monkeypatch)
    fused = _trainer_run(gnn, dims, state, req, True, tmp_path / 'f', monkeypatch)
    assert fused['tr'].trainer_log['backbone_step'] == 'fused' and 'backbone_step' not in autograd['tr'].trainer_log
    _assert_within_ensemble(f'node classification {gnn} {dims}', fused, ens, ref, autograd)
    assert len(fused['losses']) == EPOCHS and all(p.grad is None for p in fused['model'].parameters())
    eng = fused['tr']._backbone
    assert eng.z.shape == (400, dims[2]) and eng.steps_done == EPOCHS
    _assert_padding_is_zero(eng, dims[2])
    # .z is this epoch's forward: the logits the last recorded loss was taken on
    z = eng.z.double().cpu()
    want = F.nll_loss(F.log_softmax(z, 1)[req['train_mask']], req['y'][req['train_mask']])
    assert abs(float(want) - eng.last_loss()) <= 1e-5 * float(want)


@pytest.mark.parametrize('classes', [3, 4, 7, 32, 40])
@pytest.mark.parametrize('gnn', ['gcn', 'gat'])
def test_layer_two_shadows_keep_their_padding_exactly_zero(gnn, classes):
    """The engine on its own, 8 steps at lr 1e-2 (larger steps than the requests above)."""
    from gnndelete_amd.backbone import NodeClassifierEngine
    from gnndelete_amd.framework import models as M
    dims = (32, 32, classes)
    req = _nodecls_request(32, classes, n=200, seed=3)
    state = _initial_state(gnn, dims)
    m = {'gcn': M.GCN, 'gat': M.GAT}[gnn](SimpleNamespace(in_dim=32, hidden_dim=32, out_dim=classes))
    m.load_state_dict(state)
    m = m.cuda()
    own = [p.data_ptr() for p in m.parameters()]
    eng = NodeClassifierEngine(m, req['x'].cuda(), req['edge_index'].cuda(), req['y'].cuda(), req['train_mask'].cuda(), 1e-2,
                               (0.9, 0.999), 1e-8)
    for _ in range(8):
        eng.step()
    torch.cuda.synchronize()
    _assert_padding_is_zero(eng, classes)
    assert [p.data_ptr() for p in m.parameters()] == own                       # the model's tensors are refreshed, not replaced
    for k, p in m.named_parameters():
        assert not torch.equal(p.detach().cpu(), state[k]), k                  # ... and every one of them has moved
    if classes == 32:
        assert eng.shadows == {} and [p.data_ptr() for p in eng.params] == own  # the model's tensors are the ones stepped
    hist = eng.loss_history()
    assert hist.shape == (8,) and float(hist[-1]) < float(hist[0]) and eng.last_loss() == float(hist[-1])
    # the exported moments have the parameters' own shapes; importing them back pads them with zeros
    opt = torch.optim.Adam(m.parameters(), lr=1e-2)
    eng.export_adam_state(opt)
    for p in m.parameters():
        assert opt.state[p]['exp_avg'].shape == p.shape and opt.state[p]['exp_avg_sq'].shape == p.shape
        assert float(opt.state[p]['step']) == 8
    again = NodeClassifierEngine(m, req['x'].cuda(), req['edge_index'].cuda(), req['y'].cuda(), req['train_mask'].cuda(), 1e-2,
                                 (0.9, 0.999), 1e-8)
    again.import_adam_state(opt)
    for a, b in zip(again.adam, eng.adam):
        assert torch.equal(a['m'], b['m']) and torch.equal(a['v'], b['v']) and a['steps'] == 8 and int(a['step']) == 8


@pytest.mark.parametrize('gnn', ['gcn', 'gat'])
@pytest.mark.parametrize('case', ['one_row', 'every_row', 'one_class'])
def test_fused_node_classifier_edge_cases(case, gnn, tmp_path, monkeypatch):
    dims = (32, 32, 4)
    req, state, ref, ens = _references(gnn, dims, case)
    assert int(req['train_mask'].sum()) == {'one_row': 1, 'every_row': 400}.get(case, int(req['train_mask'].sum()))
    if case == 'one_class':
        assert req['y'].unique().tolist() == [3]
    fused = _trainer_run(gnn, dims, state, req, True, tmp_path / 'f', monkeypatch)
    assert fused['tr'].trainer_log['backbone_step'] == 'fused'
    _assert_within_ensemble(f'{case} {gnn}', fused, ens, ref)
    _assert_padding_is_zero(fused['tr']._backbone, 4)


def test_engine_refuses_what_the_loss_cannot_take():
    from gnndelete_amd.backbone import NodeClassifierEngine
    from gnndelete_amd.framework import models as M
    req = _nodecls_request(32, 4, n=200, seed=3)

    def make(classes=4, y=None, mask=None):
        m = M.GCN(SimpleNamespace(in_dim=32, hidden_dim=32, out_dim=classes)).cuda()
        return NodeClassifierEngine(m, req['x'].cuda(), req['edge_index'].cuda(), (req['y'] if y is None else y).cuda(),
                                    (req['train_mask'] if mask is None else mask).cuda(), 1e-3, (0.9, 0.999), 1e-8)
    with pytest.raises(ValueError, match='empty train mask'):
        make(mask=torch.zeros(200, dtype=torch.bool))
    for bad in (4, -1):
        y = req['y'].clone()
        y[0] = bad                                                             # node 0 is a training row
        with pytest.raises(ValueError, match='label'):
            make(y=y)
    y = req['y'].clone()
    y[~req['train_mask']] = 99                                                 # labels off the training rows are not read
    make(y=y).step()
    with pytest.raises(ValueError, match='300 classes'):
        make(classes=300)


# ------------------------------------------------------------------------------------------ bits
@pytest.mark.parametrize('gnn', ['gcn', 'gat'])
def test_eager_replay_and_rerun_agree_bit_for_bit(gnn, tmp_path, monkeypatch):
    dims = (100, 64, 7)
    req = _nodecls_request(dims[0], dims[2], n=200, seed=21)
    state = _initial_state(gnn, dims)
    runs = [_trainer_run(gnn, dims, state, req, True, tmp_path / str(k), monkeypatch, epochs=5, engine_kw=kw)
            for k, kw in enumerate(({'use_graph': True}, {'use_graph': False}, {'use_graph': True}))]
    assert runs[0]['tr']._backbone._graph is not None and runs[1]['tr']._backbone._graph is None
    hist = [r['tr']._backbone.loss_history() for r in runs]
    assert hist[0].shape == (5,) and all(float(v.abs().max()) > 0 for v in runs[0]['updates'].values())
    for r, h in zip(runs[1:], hist[1:]):
        for group in ('params', 'exp_avg', 'exp_avg_sq'):
            for k, v in runs[0][group].items():
                assert torch.equal(r[group][k], v), (group, k)
        assert torch.equal(h, hist[0])
        assert torch.equal(r['tr']._backbone.z, runs[0]['tr']._backbone.z)
    assert torch.equal(hist[0].double(), runs[0]['losses'])          # the epoch records are the ring's rows
    assert runs[0]['tr']._backbone.last_loss() == float(hist[0][-1])


@pytest.mark.parametrize('gnn,classes', [('gcn', 4), ('gat', 7), ('gcn', 32)])
def test_resumes_on_the_same_model_and_optimizer(gnn, classes, tmp_path, monkeypatch):
    dims = (32, 32, classes)
    req = _nodecls_request(32, classes, n=200, seed=22)
    state = _initial_state(gnn, dims)
    whole = _trainer_run(gnn, dims, state, req, True, tmp_path / 'w', monkeypatch, epochs=8)
    first = _trainer_run(gnn, dims, state, req, True, tmp_path / 'h', monkeypatch, epochs=4)
    assert set(first['steps'].values()) == {4.0}
    second = _trainer_run(gnn, dims, state, req, True, tmp_path / 'h', monkeypatch, epochs=4, resume=first)
    assert second['tr'].trainer_log['backbone_step'] == 'fused' and set(second['steps'].values()) == {8.0}
    for group in ('params', 'exp_avg', 'exp_avg_sq'):
        for k, v in whole[group].items():
            assert torch.equal(second[group][k], v), (group, k)
    assert torch.equal(torch.cat([first['losses'], second['losses']]), whole['losses'])


# ------------------------------------------------------------------------------------------ fallbacks
@pytest.mark.parametrize('what', ['gin', 'sage', 'sgd', 'weight_decay', 'classes_300'])
def test_falls_back_to_the_autograd_loop(what, tmp_path, monkeypatch, capsys):
    gnn = what if what in ('gin', 'sage') else 'gcn'
    dims = (32, 32, 300 if what == 'classes_300' else 4)
    req = _nodecls_request(32, dims[2], n=120, seed=31)
    state = _initial_state(gnn, dims)
    make_opt = {'sgd': lambda ps: torch.optim.SGD(ps, lr=1e-2),
                'weight_decay': lambda ps: torch.optim.Adam(ps, lr=1e-3, weight_decay=5e-4)}.get(what)
    want = {'gin': 'no fused backbone step for the GIN backbone (GCN and GAT only)',
            'sage': 'no fused backbone step for the SAGE backbone (GCN and GAT only)',
            'sgd': 'the optimizer is not one plain torch.optim.Adam', 'weight_decay': 'Adam with weight decay',
            'classes_300': '300 classes (the fused node-classification step takes up to 256)'}[what]
    plain = _trainer_run(gnn, dims, state, req, False, tmp_path / 'p', monkeypatch, epochs=3, make_opt=make_opt)
    capsys.readouterr()
    flag = _trainer_run(gnn, dims, state, req, True, tmp_path / 'f', monkeypatch, epochs=3, make_opt=make_opt)
    out = capsys.readouterr().out
    assert out.count(f'--fused_backbone: {want}; running the autograd loop') == 1
    assert flag['tr'].trainer_log['backbone_step'] == want and not hasattr(flag['tr'], '_backbone')
    assert 'backbone_step' not in plain['tr'].trainer_log                      # without the flag: no such key
    a, b = plain['tr'].trainer_log['log'], flag['tr'].trainer_log['log']
    assert [sorted(r) for r in a] == [sorted(r) for r in b] and [r.get('epoch') for r in a] == [r.get('epoch') for r in b]
    assert len(flag['losses']) == 3 and rel_l2(flag['losses'], plain['losses']) < 1e-6
    for (k, p), (_, q) in zip(flag['model'].state_dict().items(), plain['model'].state_dict().items()):
        assert rel_l2(p.cpu(), q.cpu()) < 1e-5, k
    assert sorted(os.listdir(str(tmp_path / 'p'))) == sorted(os.listdir(str(tmp_path / 'f')))


# ------------------------------------------------------------------------------------------ CLI
def test_cli_train_node_fused_backbone(tmp_path):
    env = dict(os.environ, PYTHONPATH=ROOT, GNNDELETE_FORCE_EPOCHS='20', GNNDELETE_FORCE_VALID_FREQ='10')

    def run(cmd, cwd):
        r = subprocess.run([sys.executable] + cmd, cwd=cwd, env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        return r.stdout
    common = ['--dataset', 'synth-tiny', '--gnn', 'gat', '--random_seed', '42']
    logs, files = {}, {}
    for tag, flag in (('plain', []), ('fused', ['--fused_backbone'])):
        cwd = str(tmp_path / tag)
        os.makedirs(cwd)
        run([os.path.join(ROOT, 'train_node.py')] + common + flag, cwd)
        out = os.path.join(cwd, 'checkpoint_node', 'synth-tiny', 'gat', 'original', '42')
        with open(os.path.join(out, 'trainer_log.json')) as f:
            logs[tag] = json.load(f)
        files[tag] = sorted(os.listdir(out))
        ck = torch.load(os.path.join(out, 'model_best.pt'))
        assert all(bool(torch.isfinite(w).all()) for w in ck['model_state'].values())
        assert ck['model_state']['conv2.lin_src.weight'].shape[0] == 4
        assert len(ck['optimizer_state']['state']) == 8 and 'exp_avg' in ck['optimizer_state']['state'][0]
        z = torch.load(os.path.join(out, 'node_embeddings.pt'))
        assert z.shape == (600, 4) and float((z.double().exp().sum(1) - 1).abs().max()) < 1e-5
    assert logs['fused'].pop('backbone_step') == 'fused' and 'backbone_step' not in logs['plain']
    assert sorted(logs['plain']) == sorted(logs['fused']) and files['plain'] == files['fused']
    assert [sorted(r) for r in logs['plain']['log']] == [sorted(r) for r in logs['fused']['log']]
    assert [r['epoch'] for r in logs['fused']['log'] if 'train_loss' in r] == [9, 19]
    assert abs(logs['plain']['best_valid_acc'] - logs['fused']['best_valid_acc']) <= 2e-3
    assert logs['plain']['best_epoch'] == logs['fused']['best_epoch'] and 0.0 <= logs['fused']['dt_acc'] <= 1.0
    # the unlearning request starts from the fused run's checkpoint
    cwd = str(tmp_path / 'fused')
    run([os.path.join(ROOT, 'delete_node.py')] + common + ['--unlearning_model', 'gnndelete_nodeemb', '--df', 'in',
                                                           '--df_size', '5'], cwd)
    out = os.path.join(cwd, 'checkpoint_node', 'synth-tiny', 'gat', 'gnndelete_nodeemb-node_deletion',
                       'mse_mean-both_layerwise-0.5-non_connected', 'in-5.0-42')
    with open(os.path.join(out, 'trainer_log.json')) as f:
        log = json.load(f)
    assert 0.0 <= log['dt_acc'] <= 1.0 and 'dt_f1' in log
