"""step_device() of BackboneEngine and EdgeprobEngine (negatives drawn by gd_negative_edges, the incidence list merged by
gd_edge_incidence_update, plain launches around the captured iteration) against step(neg) on the negatives
gnndelete_amd.negatives.reference_draw gives for the same (keys, seed, counter): two engines on deep copies of one model,
three epochs, and every parameter, both Adam moments, z, the loss history and the three incidence arrays equal bit for bit -
eager and replayed.  A graph the draw does not take is refused before any launch."""
import copy
from types import SimpleNamespace

import pytest
import torch

pytestmark = pytest.mark.gpu
LR, BETAS, EPS, SEED = 1e-3, (0.9, 0.999), 1e-8, 1234


def _graph(n=300, n_edges=1200, hub=70, isolate=3, seed=0):
    """~n_edges undirected random edges in both directions, node 0 joined to `hub` others, the last nodes without an edge."""
    g = torch.Generator().manual_seed(seed)
    e = torch.randint(1, n - isolate, (2, n_edges), generator=g)
    e = e[:, e[0] != e[1]]
    spokes = torch.randperm(n - isolate - 1, generator=g)[:hub] + 1
    e = torch.cat([e, torch.stack([torch.zeros(hub, dtype=torch.long), spokes])], 1)
    e = torch.unique(torch.stack([e.min(0).values, e.max(0).values]), dim=1)
    return torch.cat([e, e.flip(0)], 1), g


def _assert_engines_equal(a, b, params_a, params_b, z_a, z_b):
    for k, (p, q) in enumerate(zip(params_a, params_b)):
        assert torch.equal(p.data, q.data), f'parameter {k}'
    for k, (s, t) in enumerate(zip(a.adam, b.adam)):
        assert torch.equal(s['m'], t['m']) and torch.equal(s['v'], t['v']) and torch.equal(s['step'], t['step']), f'moments {k}'
        assert s['steps'] == t['steps'] == 3
    assert torch.equal(z_a, z_b)
    ha, hb = a.loss_history(), b.loss_history()
    assert ha.shape[0] == 3 and torch.equal(ha, hb) and bool(torch.isfinite(ha).all())
    assert torch.equal(a.dec, b.dec)
    total = int(a.inc_ptr[-1])
    assert total == 2 * a.dec.shape[1]                          # every decoded edge is valid: the whole arrays are compared
    assert torch.equal(a.inc_ptr, b.inc_ptr) and torch.equal(a.other, b.other) and torch.equal(a.src_edge, b.src_edge)


@pytest.mark.parametrize('use_graph', [False, True], ids=['eager', 'replayed'])
@pytest.mark.parametrize('dims', [(32, 32, 16), (100, 64, 32)], ids=['32-32-16', '100-64-32'])
@pytest.mark.parametrize('gnn', ['gcn', 'gat'])
def test_backbone_step_device_equals_step_on_the_reference_draw(gnn, dims, use_graph):
    from gnndelete_amd.backbone import BackboneEngine
    from gnndelete_amd.framework import graph_utils as GU, models as M
    from gnndelete_amd.negatives import reference_draw
    n = 300
    edges, g = _graph(n)
    x = torch.randn(n, dims[0], generator=g)
    n_neg = edges.shape[1] - 50
    torch.manual_seed(7)
    model = {'gcn': M.GCN, 'gat': M.GAT}[gnn](SimpleNamespace(in_dim=dims[0], hidden_dim=dims[1], out_dim=dims[2])).cuda()
    models = [copy.deepcopy(model) for _ in range(2)]
    host, dev = (BackboneEngine(m, x.cuda(), edges.cuda(), edges.cuda(), n_neg, LR, BETAS, EPS, history=16, use_graph=use_graph)
                 for m in models)
    keys = GU.positive_edge_keys(edges, n)
    dev.enable_device_negatives(keys.cuda(), SEED)
    draws = [reference_draw(keys, n, SEED, k, n_neg) for k in range(3)]
    assert not torch.equal(draws[0], draws[1])
    for k in range(3):
        host.step(draws[k].cuda())
        dev.step_device()
    torch.cuda.synchronize()
    assert (dev._graph is not None) == use_graph
    assert int(dev._neg['counter']) == 3
    assert torch.equal(dev.dec[:, edges.shape[1]:].cpu(), draws[2])
    _assert_engines_equal(host, dev, list(models[0].parameters()), list(models[1].parameters()), host.z, dev.z)
    assert any(float((p.data - q.data).abs().max()) > 0 for p, q in zip(models[0].parameters(), model.parameters()))


def _edgeprob_request(gnn, n=300, f=32, n_edges=1200, n_df=20, seed=0):
    """What GNNDeleteTrainer.train_fullbatch hands EdgeprobEngine for a seeded request of n_df deleted undirected edges."""
    from gnndelete_amd.framework import models as M
    from gnndelete_amd.framework.data import Data, prepare_edge_deletion
    from gnndelete_amd.framework.trainer.gnndelete import sdf_pair_mask
    g = torch.Generator().manual_seed(seed)
    e = torch.randint(0, n, (2, n_edges), generator=g)
    e = e[:, e[0] != e[1]]
    e = torch.unique(torch.stack([e.min(0).values, e.max(0).values]), dim=1)
    data = Data(num_nodes=n, x=torch.randn(n, f, generator=g), train_pos_edge_index=e)
    state = torch.get_rng_state()
    torch.manual_seed(seed + 1)
    data = prepare_edge_deletion(data, torch.ones(e.shape[1], dtype=torch.bool), n_df)
    torch.manual_seed(7)
    model = {'gcn': M.GCNDelete, 'gat': M.GATDelete}[gnn](SimpleNamespace(in_dim=f, hidden_dim=32, out_dim=16),
                                                          data['sdf_node_1hop_mask'], data['sdf_node_2hop_mask']).cuda()
    torch.set_rng_state(state)
    E = data['train_pos_edge_index'].cuda()
    df_edges, e_sdf = E[:, data['df_mask'].cuda()], E[:, data['sdf_mask'].cuda()].contiguous()
    nodes, pair_mask = sdf_pair_mask(n, data['sdf_node_2hop_mask'].cuda(), df_edges)
    target = torch.randn(n, n, generator=g).cuda()[nodes][:, nodes].sigmoid()
    target.masked_fill_(~pair_mask, -1.0)
    pad = (target.shape[0] + 3) // 4 * 4 - target.shape[0]
    if pad:
        target = torch.nn.functional.pad(target, (0, pad), value=-1.0)
    return model, data['x'].cuda(), E, e_sdf, df_edges, nodes.to(torch.int32).contiguous(), target.contiguous(), int(pair_mask.sum())


@pytest.mark.parametrize('use_graph', [False, True], ids=['eager', 'replayed'])
@pytest.mark.parametrize('gnn', ['gcn', 'gat'])
def test_edgeprob_step_device_equals_step_on_the_reference_draw(gnn, use_graph):
    from gnndelete_amd.edgeprob import EdgeprobEngine
    from gnndelete_amd.framework import graph_utils as GU
    from gnndelete_amd.negatives import reference_draw
    n = 300
    model, x, E, e_sdf, df_edges, nodes32, target, n_pairs = _edgeprob_request(gnn, n)
    m = df_edges.shape[1]
    assert m == 40 and n_pairs > 0
    models = [copy.deepcopy(model) for _ in range(2)]
    host, dev = (EdgeprobEngine(mm, x, e_sdf, df_edges, nodes32, target, n_pairs, LR, BETAS, EPS, history=16, use_graph=use_graph)
                 for mm in models)
    keys = GU.positive_edge_keys(E, n)                          # the host draw excludes every train edge, not only Df
    dev.enable_device_negatives(keys, SEED, counter=5)
    draws = [reference_draw(keys, n, SEED, 5 + k, m) for k in range(3)]
    for k in range(3):
        host.step(draws[k].cuda())
        dev.step_device()
    torch.cuda.synchronize()
    assert (dev._graph is not None) == use_graph and int(dev._neg['counter']) == 8
    dels = [[mm.deletion1.deletion_weight, mm.deletion2.deletion_weight] for mm in models]
    _assert_engines_equal(host, dev, dels[0], dels[1], host.z2, dev.z2)
    assert float((dels[0][1].data - model.deletion2.deletion_weight.data).abs().max()) > 0


def test_a_graph_with_more_than_half_of_all_pairs_excluded_is_refused_before_any_launch():
    from gnndelete_amd.backbone import BackboneEngine
    from gnndelete_amd.framework import graph_utils as GU, models as M
    n = 12
    a, b = torch.meshgrid(torch.arange(n), torch.arange(n), indexing='ij')
    edges = torch.stack([a.flatten(), b.flatten()])
    edges = edges[:, (edges[0] != edges[1]) & ((edges[0] + edges[1]) % 3 != 0)]            # about two thirds of all pairs
    keys = GU.positive_edge_keys(edges, n)
    assert 2 * (keys.numel() + n) > n * n
    torch.manual_seed(1)
    model = M.GCN(SimpleNamespace(in_dim=8, hidden_dim=8, out_dim=8)).cuda()
    eng = BackboneEngine(model, torch.randn(n, 8).cuda(), edges.cuda(), edges.cuda(), 10, LR, BETAS, EPS, history=16)
    before = eng.dec.clone()
    with pytest.raises(ValueError, match='exclude more than half'):
        eng.enable_device_negatives(keys.cuda(), SEED)
    with pytest.raises(RuntimeError, match='enable_device_negatives'):
        eng.step_device()
    torch.cuda.synchronize()
    assert eng._neg is None and eng.steps_done == 0 and torch.equal(eng.dec, before)
