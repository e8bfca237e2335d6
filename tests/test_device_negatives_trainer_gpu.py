"""--device_negatives through the trainers on synth-tiny: train_gnn.py-shaped (Trainer), delete_gnn.py --unlearning_model retrain
(RetrainTrainer) and --unlearning_model gnndelete (GNNDeleteTrainer) with the fused flag - trainer_log['negatives'] == 'device',
finite losses, a backbone loss that falls, identical checkpoints for one seed and other negatives for another - and the three
fallbacks (the fused flag missing, more than half of all pairs excluded, a replaced negative_sampling), each with its printed
reason and the host path's results bit for bit."""
import functools
import os
from types import SimpleNamespace

import pytest
import torch

pytestmark = pytest.mark.gpu
NO_EVAL = (0.0, 0.0, 0.0, 0.0, 0.0, [], None, {})


@functools.lru_cache(maxsize=None)
def _synth_tiny():
    from gnndelete_amd.framework.synth import make_linkpred_dataset
    return make_linkpred_dataset('synth-tiny', 42)


def _copy(data):
    from gnndelete_amd.framework.data import Data
    return Data({k: (v.clone() if torch.is_tensor(v) else v) for k, v in data.items()})


def _args(kind, path, seed, epochs, **flags):
    os.makedirs(str(path), exist_ok=True)
    return SimpleNamespace(unlearning_model=kind, gnn='gcn', dataset='synth-tiny', checkpoint_dir=str(path), eval_on_cpu=False,
                           in_dim=32, hidden_dim=64, out_dim=32, epochs=epochs, valid_freq=5, lr=1e-2, random_seed=seed, **flags)


def _run(kind, path, seed=42, epochs=20, device_negatives=True, fused=True):
    """One trainer run on synth-tiny as the CLIs prepare it -> (trainer, model, optimizer)."""
    from gnndelete_amd.framework import get_model, get_trainer
    from gnndelete_amd.framework.data import prepare_edge_deletion
    from gnndelete_amd.framework.graph_utils import to_undirected
    data, df_masks = _synth_tiny()
    data = _copy(data)
    flag = 'fused_edgeprob' if kind == 'gnndelete' else 'fused_backbone'
    args = _args(kind, path, seed, epochs, **{flag: fused, 'device_negatives': device_negatives})
    torch.manual_seed(7)
    logits_ori = None
    if kind == 'original':
        data.train_pos_edge_index = to_undirected(data.train_pos_edge_index, num_nodes=data.num_nodes)
        data.dtrain_mask = torch.ones(data.train_pos_edge_index.shape[1], dtype=torch.bool)
        data.dr_mask = data.dtrain_mask
        model = get_model(args)
    else:
        prepare_edge_deletion(data, df_masks['in'], 60)
        if kind == 'retrain':
            data.dtrain_mask = data.dr_mask
            model = get_model(args)
        else:
            model = get_model(args, data.sdf_node_1hop_mask, data.sdf_node_2hop_mask)
            logits_ori = torch.randn(data.num_nodes, data.num_nodes, generator=torch.Generator().manual_seed(3)).cuda()
    model = model.cuda()
    params = [p for n, p in model.named_parameters() if 'del' in n] if kind == 'gnndelete' else list(model.parameters())
    opt = torch.optim.Adam(params, lr=args.lr)
    tr = get_trainer(args)
    if kind == 'gnndelete':
        tr.train(model, data, opt, args, logits_ori, None, None)
    else:
        tr.train(model, data, opt, args)
    return tr, model, opt


def _same_checkpoint(a, b, name):
    ca, cb = torch.load(os.path.join(str(a), name)), torch.load(os.path.join(str(b), name))
    if not isinstance(ca, dict):
        return torch.equal(ca, cb)
    same = all(torch.equal(ca['model_state'][k], cb['model_state'][k]) for k in ca['model_state'])
    sa, sb = ca['optimizer_state']['state'], cb['optimizer_state']['state']
    return same and sorted(sa) == sorted(sb) and all(torch.equal(sa[k][key], sb[k][key]) for k in sa for key in sa[k])


@pytest.mark.parametrize('kind', ['original', 'retrain', 'gnndelete'])
def test_trainers_draw_on_the_device(kind, tmp_path, capsys):
    runs = [_run(kind, tmp_path / tag, seed) for tag, seed in (('a', 42), ('b', 42), ('c', 43))]
    out = capsys.readouterr().out
    assert '--device_negatives:' not in out                      # no fallback line
    engines = [getattr(tr, '_edgeprob_engine' if kind == 'gnndelete' else '_backbone') for tr, _, _ in runs]
    for (tr, model, _), eng in zip(runs, engines):
        assert tr.trainer_log['negatives'] == 'device'
        assert tr.trainer_log['edgeprob_step' if kind == 'gnndelete' else 'backbone_step'] == 'fused'
        assert eng.steps_done == 20 and int(eng._neg['counter']) == 20 and eng._neg['seed'] == tr.args.random_seed
        records = [r for r in tr.trainer_log['log'] if 'train_loss' in r]
        assert [r['epoch'] for r in records] == [4, 9, 14, 19]
        hist = eng.loss_history()
        assert hist.shape[0] == 20 and bool(torch.isfinite(hist).all())
        assert all(bool(torch.isfinite(p).all()) for p in model.parameters())
        if kind == 'retrain':
            assert [s['Epoch'] for s in tr.trainer_log['steps']] == list(range(20))
        if kind != 'gnndelete':
            assert records[-1]['train_loss'] < records[0]['train_loss']
        # the negatives are what the kernel's CPU restatement gives for (the excluded edges, the seed, the last epoch)
        neg = eng.dec[:, eng._n_fixed:].cpu()
        from gnndelete_amd.negatives import reference_draw
        assert torch.equal(neg, reference_draw(eng._neg['keys'], eng.n, tr.args.random_seed, 19, neg.shape[1]))
    assert sorted(os.listdir(str(tmp_path / 'a'))) == sorted(os.listdir(str(tmp_path / 'b')))
    names = sorted(f for f in os.listdir(str(tmp_path / 'a')) if f.endswith('.pt'))
    assert 'model_best.pt' in names
    assert ('model_final.pt' in names) == (kind != 'original') and ('node_embeddings.pt' in names) == (kind == 'original')
    for name in names:
        assert _same_checkpoint(tmp_path / 'a', tmp_path / 'b', name), name
    fixed = engines[0]._n_fixed
    assert torch.equal(engines[0].dec, engines[1].dec)
    assert torch.equal(engines[0].dec[:, :fixed], engines[2].dec[:, :fixed])
    assert not torch.equal(engines[0].dec[:, fixed:], engines[2].dec[:, fixed:])           # another seed: other negatives


# ------------------------------------------------------------------------------------------ fallbacks
def _small_request(dense, seed=5):
    """A request without a validation split (Trainer.eval is stubbed): 120 nodes and ~700 directed edges, or - dense - 14 nodes
    with about two thirds of all pairs as edges."""
    g = torch.Generator().manual_seed(seed)
    if dense:
        n = 14
        a, b = torch.meshgrid(torch.arange(n), torch.arange(n), indexing='ij')
        keep = (a < b) & ((a + b) % 3 != 0)
        e = torch.stack([a[keep], b[keep]])
    else:
        n = 120
        e = torch.randint(0, n, (2, 400), generator=g)
        e = torch.unique(torch.stack([e.min(0).values, e.max(0).values])[:, e[0] != e[1]], dim=1)
    E = torch.cat([e, e.flip(0)], 1)
    return {'num_nodes': n, 'x': torch.randn(n, 32, generator=g), 'train_pos_edge_index': E,
            'dr_mask': torch.ones(E.shape[1], dtype=torch.bool)}


def _fallback_run(kind, request, path, monkeypatch, fused, device_negatives, replace_sampler):
    from gnndelete_amd.framework import get_model, graph_utils as GU
    from gnndelete_amd.framework.data import Data
    from gnndelete_amd.framework.trainer import base as TB, retrain as TR
    mod = TR if kind == 'retrain' else TB
    if replace_sampler:
        gen = torch.Generator().manual_seed(77)
        monkeypatch.setattr(mod, 'negative_sampling',
                            lambda edge_index, num_nodes, num_neg_samples: GU.negative_sampling(edge_index, num_nodes, num_neg_samples,
                                                                                                generator=gen))
    else:
        monkeypatch.setattr(mod, 'negative_sampling', GU.negative_sampling)
    args = _args(kind, path, 42, 6, fused_backbone=fused, device_negatives=device_negatives)
    torch.manual_seed(7)                                         # the model's initial state and the host sampler's stream
    model = get_model(args).cuda()
    opt = torch.optim.Adam(model.parameters(), lr=args.lr)
    tr = (TR.RetrainTrainer if kind == 'retrain' else TB.Trainer)(args)
    monkeypatch.setattr(tr, 'eval', lambda *a, **k: NO_EVAL)
    d = Data({k: (v.clone() if torch.is_tensor(v) else v) for k, v in request.items()})
    d.dtrain_mask = d.dr_mask
    tr.train(model, d, opt, args)
    return tr, model, opt


@pytest.mark.parametrize('kind', ['original', 'retrain'])
@pytest.mark.parametrize('what', ['no_fused_flag', 'dense_graph', 'replaced_sampler'])
def test_fallbacks_keep_the_host_draw_bit_for_bit(what, kind, tmp_path, monkeypatch, capsys):
    request = _small_request(dense=what == 'dense_graph')
    n, keys = request['num_nodes'], request['train_pos_edge_index'].shape[1]
    fused, replace = what != 'no_fused_flag', what == 'replaced_sampler'
    want = {'no_fused_flag': '--fused_backbone is missing or fell back', 'replaced_sampler': 'negative_sampling has been replaced',
            'dense_graph': f'{keys} positive pairs and {n} self loops exclude more than half of the {n}^2 node pairs'}[what]
    plain = _fallback_run(kind, request, tmp_path / 'p', monkeypatch, fused, False, replace)
    capsys.readouterr()
    flag = _fallback_run(kind, request, tmp_path / 'f', monkeypatch, fused, True, replace)
    out = capsys.readouterr().out
    assert out.count(f'--device_negatives: {want}; drawing the negatives on the host') == 1
    assert flag[0].trainer_log['negatives'] == want and 'negatives' not in plain[0].trainer_log
    if fused:
        assert flag[0].trainer_log['backbone_step'] == 'fused' and flag[0]._backbone._neg is None
    for key in ('log', 'steps'):
        assert plain[0].trainer_log.get(key) == flag[0].trainer_log.get(key)
    for (k, p), (_, q) in zip(flag[1].state_dict().items(), plain[1].state_dict().items()):
        assert torch.equal(p, q), k
    for p, q in zip(flag[1].parameters(), plain[1].parameters()):
        for key in ('exp_avg', 'exp_avg_sq', 'step'):
            assert torch.equal(flag[2].state[p][key], plain[2].state[q][key]), key


def test_gnndelete_fallbacks_say_why(tmp_path, monkeypatch, capsys):
    """GNNDeleteTrainer: without --fused_edgeprob and with a replaced negative_sampling the host draw stays."""
    from gnndelete_amd.framework import graph_utils as GU
    from gnndelete_amd.framework.trainer import gnndelete as TE
    tr, _, _ = _run('gnndelete', tmp_path / 'a', epochs=5, fused=False)
    assert tr.trainer_log['negatives'] == '--fused_edgeprob is missing or fell back' and not hasattr(tr, '_edgeprob_engine')
    gen = torch.Generator().manual_seed(1)
    monkeypatch.setattr(TE, 'negative_sampling', lambda edge_index, num_nodes, num_neg_samples:
                        GU.negative_sampling(edge_index, num_nodes, num_neg_samples, generator=gen))
    tr, model, _ = _run('gnndelete', tmp_path / 'b', epochs=5)
    assert tr.trainer_log['negatives'] == 'negative_sampling has been replaced' and tr._edgeprob_engine._neg is None
    assert tr._edgeprob_engine.steps_done == 5 and bool(torch.isfinite(model.deletion2.deletion_weight).all())
    out = capsys.readouterr().out
    assert out.count('--device_negatives: --fused_edgeprob is missing or fell back; drawing the negatives on the host') == 1
    assert out.count('--device_negatives: negative_sampling has been replaced; drawing the negatives on the host') == 1
