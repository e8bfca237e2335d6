"""The fused Del step with the folded KLD / cosine row losses (NodeembEngine(loss_fct=...), --fused_row_losses): trajectories
against autograd on the CPU oracle with the reference's loss functions and update rules (oracle.gnndelete_ref.nodeemb_epoch,
same state, same injected negatives), against the autograd loop of this build, graph replay vs eager, the trainer's options,
the padded class dimension, and the trainer / flag.  Bounds, in every case: the loss log rtol 1e-4 / atol 1e-7, both Del weights
rel-L2 < 1e-4 (the project's standing bound for this comparison).  The few (case, weight) pairs measured to miss the weight
bound are named one by one in ENSEMBLE below and held to the fp32-ensemble test of tests/helpers.py instead."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from helpers import hip_model, load_golden, oracle_model, rel_l2, split_fixture, t

pytestmark = pytest.mark.gpu

FIXTURES = {'gcn': ('gcn', 'traj_gcn_both_all.npz'), 'gat': ('gat', 'traj_gat_both_layerwise.npz'),
            'wide_gcn': ('gcn', 'traj_wide_gcn_both_all.npz'), 'wide_gat': ('gat', 'traj_wide_gat_both_layerwise.npz'),
            'gin': ('gin', 'traj_gin_both_layerwise.npz')}
LOSSES = ['kld_mean', 'kld_sum', 'cosine_mean', 'cosine_sum']
KEYS = ['train_loss', 'loss_r', 'loss_l']


@functools.lru_cache(maxsize=None)
def _request(key):
    """-> (gnn, state, data, alpha, lr, epochs, neg, ni1, ni2) of a committed fixture, or of a seeded request on the graph of
    traj_gcn_both_all.npz for 'sage' (32 -> 128 -> 64) and 'cls4-<gnn>' (32 -> 128 -> 4 classes: the node-deletion shape)."""
    from oracle import gnndelete_ref as R
    if key in FIXTURES:
        gnn, name = FIXTURES[key]
        state, data, rest = split_fixture(load_golden(name))
        alpha, lr, epochs = float(rest['alpha']), float(rest['lr']), int(rest['epochs'])
    else:
        gnn, out = ('sage', 64) if key == 'sage' else (key.split('-')[1], 4)
        _, data, rest = split_fixture(load_golden('traj_gcn_both_all.npz'))
        g = torch.Generator().manual_seed(21)
        data = dict(data, x=torch.randn(data['x'].shape[0], 32, generator=g) * 0.3)
        torch.manual_seed(22)
        mo = R.TwoLayerDelete(gnn, 32, 128, out, data['sdf_node_1hop_mask'], data['sdf_node_2hop_mask'])
        with torch.no_grad():      # (Del weights away from the ones/1000 start: the layer-2 products should matter)
            mo.deletion1.deletion_weight.copy_(torch.eye(128) * 0.6 + 0.02 * torch.randn(128, 128, generator=g))
            mo.deletion2.deletion_weight.copy_(torch.eye(out) * 0.7 + 0.05 * torch.randn(out, out, generator=g))
        state = {k: v.clone() for k, v in mo.state_dict().items()}
        alpha, lr, epochs = 0.4, 0.01, 6
    ni1, ni2 = R.non_df_masks(data['x'].shape[0], data['directed_df_edge_index'], data['sdf_node_1hop_mask'],
                              data['sdf_node_2hop_mask'])
    return gnn, state, data, alpha, lr, epochs, t(rest['neg']), ni1, ni2


@functools.lru_cache(maxsize=None)
def _oracle(key, loss_fct, loss_type, dtype=torch.float32, perm=None):
    """The CPU oracle's run of the request: (log [epochs, 3], W_D1, W_D2).  Computed once per case, shared, never modified.
    dtype / perm: the members of the fp32 ensemble (helpers.assert_del_weights_within_fp32_spread) - float64, or float32 with
    the edge lists permuted by the seed `perm`."""
    from oracle import gnndelete_ref as R
    gnn, state, data, alpha, lr, epochs, neg, ni1, ni2 = _request(key)
    torch.set_num_threads(min(16, torch.get_num_threads()))
    m = oracle_model(gnn, state, data['sdf_node_1hop_mask'], data['sdf_node_2hop_mask']).to(dtype)
    m.relational = False
    E = data['train_pos_edge_index']
    e_dr, e_sdf = E[:, data['dr_mask']], E[:, data['sdf_mask']]
    if perm is not None:
        gp = torch.Generator().manual_seed(perm)
        e_dr, e_sdf = e_dr[:, torch.randperm(e_dr.shape[1], generator=gp)], e_sdf[:, torch.randperm(e_sdf.shape[1], generator=gp)]
    x = data['x'].to(dtype)
    with torch.no_grad():
        z1o, z2o = m.get_original_embeddings(x, e_dr, return_all_emb=True)
    tg = dict(z1_ori=z1o, z2_ori=z2o, pos_edge=E[:, data['df_mask']], neg_edge=neg, ni_mask1=ni1, ni_mask2=ni2)
    opt = R.make_optimizer(m, loss_type, lr)
    logs = [R.nodeemb_epoch(m, lambda: m(x, e_sdf, return_all_emb=True), tg, opt, loss_type, alpha, R.LOSSES[loss_fct])
            for _ in range(epochs)]
    return (np.array([[l[k] for k in KEYS] for l in logs]), m.deletion1.deletion_weight.detach().double().clone(),
            m.deletion2.deletion_weight.detach().double().clone())


def _engine(key, loss_fct, loss_type, use_graph, **opts):
    from gnndelete_amd.engine import NodeembEngine
    gnn, state, data, alpha, lr, epochs, neg, ni1, ni2 = _request(key)
    m = hip_model(gnn, state, data['sdf_node_1hop_mask'], data['sdf_node_2hop_mask'])
    dev = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in data.items()}
    E = dev['train_pos_edge_index']
    with torch.no_grad():
        z1o, z2o = m.get_original_embeddings(dev['x'], E[:, dev['dr_mask']], return_all_emb=True)
    eng = NodeembEngine(m, dev['x'], E[:, dev['sdf_mask']].contiguous(), z1o, z2o, E[:, dev['df_mask']], neg.cuda(), ni1, ni2,
                        loss_type=loss_type, alpha=alpha, lr=lr, use_graph=use_graph, loss_fct=loss_fct, **opts)
    return eng, m, epochs


# The cases measured on an MI355X to miss rel-L2 < 1e-4 in a Del weight, eager and graph replay alike (they agree bit for bit):
# (fixture, loss_fct, loss_type, reference) -> the weights that miss.  Every other (case, weight) of this file meets the bound,
# W_D2 of the cases below included.  Per entry: the fused step's distance to the reference it misses, its distance to the fp64
# oracle, and the distances of the fp32 oracle ensemble (unpermuted, edge lists permuted with seeds 1-3) to the fp64 oracle.  On
# all but the first the fused step is closer to the fp64 oracle than the fp32 oracle it is compared with: the single fp32 run is
# the noisy side (Adam's first updates are +-lr per entry whatever the gradient's size, so summation-order noise reaches the
# weight undamped).  These weights are held to helpers.assert_del_weights_within_fp32_spread (distance to the fp64 oracle
# <= max(2 x the ensemble's largest, 5e-5)); the loss log of these cases is held to rtol 1e-4 / atol 1e-7 like every other.
ENSEMBLE = {
    # to the fp32 oracle 1.03e-04; to fp64 1.04e-04; ensemble 7.4e-06 8.1e-05 6.2e-05 6.6e-05
    ('gat', 'cosine_mean', 'both_all', 'oracle'): ('W_D1',),
    # to the fp32 oracle 1.12e-04; to fp64 3.71e-05; ensemble 7.9e-05 8.0e-05 3.4e-05 7.5e-05
    ('wide_gcn', 'cosine_mean', 'both_layerwise', 'oracle'): ('W_D1',),
    # to the fp32 oracle 1.10e-04; to fp64 4.34e-05; ensemble 7.6e-05 7.9e-05 5.8e-05 9.6e-05
    ('wide_gcn', 'cosine_sum', 'both_all', 'oracle'): ('W_D1',),
    # to the fp32 oracle 2.36e-04; to fp64 6.37e-05; ensemble 2.0e-04 1.1e-04 1.3e-04 1.6e-04
    ('wide_gat', 'cosine_sum', 'both_layerwise', 'oracle'): ('W_D1',),
    # to the fp32 oracle 3.57e-04; to fp64 7.68e-05; ensemble 3.0e-04 1.7e-04 1.9e-04 2.5e-04
    ('wide_gat', 'cosine_sum', 'both_all', 'oracle'): ('W_D1',),
    # to the fp32 oracle 1.20e-04; to fp64 2.02e-05; ensemble 9.9e-05 8.1e-05 9.5e-05 4.3e-05
    ('sage', 'kld_sum', 'both_all', 'oracle'): ('W_D1',),
    # to the autograd loop 1.11e-04; to fp64 6.37e-05 (the loop itself is one more fp32 run); ensemble as above
    ('wide_gat', 'cosine_sum', 'both_layerwise', 'loop'): ('W_D1',),
}


def _assert_trajectory(tag, eng, m, key, loss_fct, loss_type, reference=None):
    """reference = (log, W_D1, W_D2) of another fp32 run to compare with instead of the CPU oracle's: the autograd loop of this
    build.  Same bounds against either; a weight listed in ENSEMBLE for the case is held to the fp32-ensemble test instead."""
    want_log, want_w1, want_w2 = reference if reference is not None else _oracle(key, loss_fct, loss_type)
    hist = eng.loss_history().numpy()
    w1, w2 = m.deletion1.deletion_weight.detach().cpu(), m.deletion2.deletion_weight.detach().cpu()
    dist = {'W_D1': rel_l2(w1, want_w1), 'W_D2': rel_l2(w2, want_w2)}
    print(f'[{tag}] rel-L2 of W_D1 {dist["W_D1"]:.2e}, of W_D2 {dist["W_D2"]:.2e}; largest relative log difference '
          f'{float(np.max(np.abs(hist - want_log) / np.maximum(np.abs(want_log), 1e-30))):.2e}')
    for col, k in enumerate(KEYS):
        np.testing.assert_allclose(hist[:, col], want_log[:, col], rtol=1e-4, atol=1e-7, err_msg=k)
    listed = ENSEMBLE.get((key, loss_fct, loss_type, 'oracle' if reference is None else 'loop'), ())
    for name, d in dist.items():
        assert name in listed or d < 1e-4, (name, dist)
    if listed:
        from helpers import assert_del_weights_within_fp32_spread
        ens = [_oracle(key, loss_fct, loss_type, torch.float32, perm)[1:] for perm in (None, 1, 2, 3)]
        assert_del_weights_within_fp32_spread(tag, (w1, w2), _oracle(key, loss_fct, loss_type, torch.float64)[1:], ens, hist.shape[0])


# only2_all runs with kld_mean on the narrow GCN fixture: with a cosine loss that rule is chaotic in fp32 on all four fixtures
# (the fp32 oracle ensemble ends 0.15 - 0.97 rel-L2 from the fp64 oracle in W_D1: Adam normalises a W_D1 gradient that is
# rounding noise), with kld_mean the ensemble sits at 1.8e-06 on this fixture (5.3e-05 ... 6.3e-04 on the other three).
CASES = ([(k, f, lt) for k in ('gcn', 'gat', 'wide_gcn', 'wide_gat') for f in LOSSES for lt in ('both_layerwise', 'both_all')]
         + [('wide_gat', 'kld_mean', 'only1'), ('gcn', 'kld_mean', 'only2_all'), ('gat', 'cosine_sum', 'only2_layerwise'),
            ('gin', 'kld_mean', 'both_layerwise'), ('sage', 'cosine_mean', 'both_layerwise'), ('sage', 'kld_sum', 'both_all')])


@pytest.mark.parametrize('use_graph', [False, True])
@pytest.mark.parametrize('key,loss_fct,loss_type', CASES)
def test_fused_step_follows_the_cpu_oracle(key, loss_fct, loss_type, use_graph):
    eng, m, epochs = _engine(key, loss_fct, loss_type, use_graph)
    assert eng.family == loss_fct.split('_')[0] and eng.t1.folded and eng.t2.folded
    for _ in range(epochs):
        eng.step()
    _assert_trajectory(f'{key} {loss_fct} {loss_type} graph={use_graph}', eng, m, key, loss_fct, loss_type)


@pytest.mark.parametrize('key,loss_fct,loss_type', [('wide_gcn', 'kld_mean', 'both_all'), ('wide_gat', 'kld_mean', 'both_layerwise'),
                                                    ('wide_gcn', 'cosine_sum', 'both_all'), ('wide_gat', 'cosine_sum', 'both_layerwise')])
def test_fused_step_follows_the_autograd_loop_of_this_build(key, loss_fct, loss_type):
    """get_loss_fct(name) + _autograd_update around the HIP-backed model with torch's Adam: what --loss_fct kld_* / cosine_*
    runs without the flag."""
    from gnndelete_amd.framework.trainer.gnndelete_nodeemb import _autograd_update, _four_terms, get_loss_fct
    from oracle import gnndelete_ref as R
    gnn, state, data, alpha, lr, epochs, neg, ni1, ni2 = _request(key)
    m = hip_model(gnn, state, data['sdf_node_1hop_mask'], data['sdf_node_2hop_mask'])
    dev = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in data.items()}
    E = dev['train_pos_edge_index']
    e_sdf, pos = E[:, dev['sdf_mask']].contiguous(), E[:, dev['df_mask']]
    with torch.no_grad():
        z1o, z2o = m.get_original_embeddings(dev['x'], E[:, dev['dr_mask']], return_all_emb=True)
    opt = R.make_optimizer(m, loss_type, lr)
    fct = get_loss_fct(loss_fct)
    log = []
    for _ in range(epochs):
        z1, z2 = m(dev['x'], e_sdf, return_all_emb=True)
        r1, r2, l1, l2 = _four_terms(fct, z1, z2, z1o, z2o, pos, neg.cuda(), ni1.cuda(), ni2.cuda())
        log.append([float(v) for v in _autograd_update(loss_type, alpha, r1, r2, l1, l2, opt)])
    eng, mf, _ = _engine(key, loss_fct, loss_type, True)
    for _ in range(epochs):
        eng.step()
    _assert_trajectory(f'{key} {loss_fct} {loss_type} vs autograd loop', eng, mf, key, loss_fct, loss_type,
                       reference=(np.array(log), m.deletion1.deletion_weight.detach().double().cpu(),
                                  m.deletion2.deletion_weight.detach().double().cpu()))


@pytest.mark.parametrize('key,loss_fct', [('wide_gcn', 'kld_mean'), ('wide_gat', 'cosine_mean'), ('gat', 'kld_mean'), ('gcn', 'cosine_mean')])
def test_graph_replay_equals_eager_bit_for_bit(key, loss_fct):
    a, ma, _ = _engine(key, loss_fct, 'both_layerwise', False)
    b, mb, _ = _engine(key, loss_fct, 'both_layerwise', True)
    for _ in range(5):
        a.step()
        b.step()
    assert b._graph is not None and a._graph is None
    assert torch.equal(ma.deletion1.deletion_weight, mb.deletion1.deletion_weight)
    assert torch.equal(ma.deletion2.deletion_weight, mb.deletion2.deletion_weight)
    assert torch.equal(a.loss_history(), b.loss_history())
    assert not torch.equal(ma.deletion2.deletion_weight.cpu(), _request(key)[1]['deletion2.deletion_weight'])


@pytest.mark.parametrize('cache_layer1', [False, True])
@pytest.mark.parametrize('affected_rows_only', [False, True])
def test_trainer_options_keep_the_trajectory(cache_layer1, affected_rows_only):
    eng, m, epochs = _engine('wide_gcn', 'kld_mean', 'both_layerwise', True, cache_layer1=cache_layer1,
                             affected_rows_only=affected_rows_only)
    assert eng.cache_layer1 == cache_layer1 and eng._rows_only == affected_rows_only
    for _ in range(epochs):
        eng.step()
    _assert_trajectory(f'cache_layer1={cache_layer1} rows_only={affected_rows_only}', eng, m, 'wide_gcn', 'kld_mean', 'both_layerwise')


@pytest.mark.parametrize('gnn,loss_fct', [('gcn', 'kld_mean'), ('gat', 'kld_mean'), ('gcn', 'cosine_mean'), ('gat', 'kld_sum')])
def test_class_dimension_four_runs_the_losses_at_the_true_width(gnn, loss_fct):
    """out_dim = 4 classes: the engine pads layer 2 to 64 columns; the KLD softmax must still run over the 4 true columns
    (a softmax over 60 padding zeros is another function), and W_D2's padding must not move."""
    key = f'cls4-{gnn}'
    eng, m, epochs = _engine(key, loss_fct, 'both_layerwise', True)
    assert eng.o == 64 and eng._user_wd2 is not None and eng.t2.d_valid == 4 and tuple(m.deletion2.deletion_weight.shape) == (4, 4)
    for _ in range(epochs):
        eng.step()
    wpad = eng.wd2.detach().clone()
    assert torch.equal(wpad[:4, :4], m.deletion2.deletion_weight.detach())
    wpad[:4, :4] = 0
    assert float(wpad.abs().max()) == 0.0, 'padding rows / columns of W_D2 never move'
    _assert_trajectory(f'{key} {loss_fct}', eng, m, key, loss_fct, 'both_layerwise')


@pytest.mark.parametrize('loss_fct', ['kld_mean', 'cosine_sum'])
def test_the_mse_fused_forms_are_off_and_the_tail_launch_stays(loss_fct):
    eng, _, _ = _engine('wide_gat', loss_fct, 'both_layerwise', True)
    assert not (eng._fuse_loss1 or eng._fuse_l2 or eng._fuse_del1 or eng._fuse_wg2 or eng._chain1 or eng._out_pair)
    assert eng._tail and eng._split1 and eng._split2
    mse, _, _ = _engine('wide_gat', 'mse_mean', 'both_layerwise', True)
    assert mse._fuse_loss1 and mse._fuse_l2 and mse._tail and mse.family == 'mse'
    narrow, _, _ = _engine('gat', loss_fct, 'both_layerwise', True)
    assert not narrow._tail and not narrow._fuse_loss1


def test_unsupported_requests_are_refused_with_a_reason():
    from gnndelete_amd.engine import NodeembEngine
    gnn, state, data, alpha, lr, epochs, neg, ni1, ni2 = _request('gat')
    m = hip_model(gnn, state, data['sdf_node_1hop_mask'], data['sdf_node_2hop_mask'])
    dev = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in data.items()}
    E = dev['train_pos_edge_index']
    with torch.no_grad():
        z1o, z2o = m.get_original_embeddings(dev['x'], E[:, dev['dr_mask']], return_all_emb=True)
    args = (m, dev['x'], E[:, dev['sdf_mask']].contiguous(), z1o, z2o, E[:, dev['df_mask']], neg.cuda())
    with pytest.raises(ValueError, match='linear_cka'):
        NodeembEngine(*args, ni1, ni2, loss_fct='linear_cka')
    with pytest.raises(ValueError, match='one kind of term per row'):            # NI rows that include the Df endpoints
        NodeembEngine(*args, data['sdf_node_1hop_mask'], data['sdf_node_2hop_mask'], loss_fct='kld_mean')
    from gnndelete_amd.dist_engine import PartitionedNodeembEngine
    with pytest.raises(NotImplementedError, match='all-reduce'):
        PartitionedNodeembEngine(*args, ni1, ni2, 0, 1, loss_fct='kld_mean')


# ------------------------------------------------------------------------------------------ trainer / flag
def _trainer_run(tmp_path, monkeypatch, loss_fct, fused, data=None, no_fused_step=False):
    from gnndelete_amd.framework.data import Data
    from gnndelete_amd.framework.trainer import gnndelete_nodeemb as TN
    gnn, state, fdata, alpha, lr, epochs, neg, _, _ = _request('wide_gat')
    data = fdata if data is None else data
    m = hip_model(gnn, state, data['sdf_node_1hop_mask'], data['sdf_node_2hop_mask'])
    neg = neg.cuda()
    monkeypatch.setattr(TN, 'negative_sampling', lambda *a, **k: neg)
    args = SimpleNamespace(unlearning_model='gnndelete_nodeemb', dataset='Cora', checkpoint_dir=str(tmp_path), eval_on_cpu=False,
                           epochs=epochs, valid_freq=epochs, lr=lr, alpha=alpha, loss_fct=loss_fct, loss_type='both_layerwise',
                           gnn=gnn, fused_row_losses=fused, no_fused_step=no_fused_step)
    tmp_path.mkdir(parents=True, exist_ok=True)
    opt = [torch.optim.Adam(m.deletion1.parameters(), lr=lr), torch.optim.Adam(m.deletion2.parameters(), lr=lr)]
    tr = TN.GNNDeleteNodeembTrainer(args)
    torch.manual_seed(7)
    tr.train(m, Data(data), opt, args)
    return tr, m, opt


def test_trainer_runs_kld_on_the_fused_step_with_the_flag(tmp_path, monkeypatch, capsys):
    tr, m, opt = _trainer_run(tmp_path / 'fused', monkeypatch, 'kld_mean', True)
    assert tr.trainer_log['nodeemb_step'] == 'fused' and '--fused_row_losses' not in capsys.readouterr().out
    epochs = _request('wide_gat')[5]
    assert len(tr.trainer_log['loss_history']) == epochs
    # the exported Adam state is that of the MSE fused path: same keys, same step count as an mse_mean run of this trainer
    mse, mm, mopt = _trainer_run(tmp_path / 'mse', monkeypatch, 'mse_mean', False)
    assert 'nodeemb_step' not in mse.trainer_log and len(mse.trainer_log['loss_history']) == epochs
    for o_, p_, mo_, mp_ in ((opt[0], m.deletion1.deletion_weight, mopt[0], mm.deletion1.deletion_weight),
                             (opt[1], m.deletion2.deletion_weight, mopt[1], mm.deletion2.deletion_weight)):
        st, mst = o_.state[p_], mo_.state[mp_]
        assert set(st) == set(mst) == {'step', 'exp_avg', 'exp_avg_sq'} and float(st['step']) == float(mst['step'])
        assert st['exp_avg'].shape == p_.shape and bool(torch.isfinite(st['exp_avg']).all()) and float(st['exp_avg_sq'].sum()) > 0
    plain, mp, _ = _trainer_run(tmp_path / 'plain', monkeypatch, 'kld_mean', False)
    assert 'nodeemb_step' not in plain.trainer_log and 'loss_history' not in plain.trainer_log
    d1 = rel_l2(m.deletion1.deletion_weight.detach().cpu(), mp.deletion1.deletion_weight.detach().cpu())
    d2 = rel_l2(m.deletion2.deletion_weight.detach().cpu(), mp.deletion2.deletion_weight.detach().cpu())
    print(f'trainer, kld_mean with / without --fused_row_losses: rel-L2 of W_D1 {d1:.2e}, of W_D2 {d2:.2e}')
    assert d1 < 1e-4 and d2 < 1e-4
    last_f = [r for r in tr.trainer_log['log'] if 'train_loss' in r][-1]
    last_p = [r for r in plain.trainer_log['log'] if 'train_loss' in r][-1]
    for k in KEYS:
        np.testing.assert_allclose(last_f[k], last_p[k], rtol=1e-4, atol=1e-7, err_msg=k)


def test_trainer_falls_back_to_the_autograd_loop_with_a_reason(tmp_path, monkeypatch, capsys):
    tr, m, _ = _trainer_run(tmp_path / 'cka', monkeypatch, 'linear_cka', True)
    out = capsys.readouterr().out
    assert '--fused_row_losses: no folded form of --loss_fct linear_cka' in out and '; running the autograd loop' in out
    assert tr.trainer_log['nodeemb_step'] == 'autograd' and bool(torch.isfinite(m.deletion2.deletion_weight).all())
    # a request whose Neighborhood-Influence rows contain an endpoint of a deleted edge: the list of directed Df edges the NI
    # masks are cut with misses the deleted edges of one node
    data = dict(_request('wide_gat')[2])
    ddf = data['directed_df_edge_index']
    data['directed_df_edge_index'] = ddf[:, (ddf != ddf[0, 0]).all(0)]
    tr, m, _ = _trainer_run(tmp_path / 'mixed', monkeypatch, 'kld_mean', True, data=data)
    out = capsys.readouterr().out
    assert '--fused_row_losses: a Neighborhood-Influence row is an endpoint of a deleted edge' in out
    assert tr.trainer_log['nodeemb_step'] == 'autograd' and bool(torch.isfinite(m.deletion2.deletion_weight).all())
    tr, m, _ = _trainer_run(tmp_path / 'off', monkeypatch, 'cosine_mean', True, no_fused_step=True)
    assert '--fused_row_losses: --no_fused_step is set; running the autograd loop' in capsys.readouterr().out
    assert tr.trainer_log['nodeemb_step'] == 'autograd'
