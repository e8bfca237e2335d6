"""Which kernel forms NodeembEngine runs on the small requests of this suite: the facts it computed from each request and the
forms engine.plan_step chose from them, against tests/golden/engine_forms.json (recorded from the engine before the forms were
decided in one function).  The decision depends on width classes and set relations, not on row counts - except the 65,536-row
threshold of the fused Del-1 pass, which test_step_plan_cpu.py and test_full_size_gpu.py cover."""
import functools
import json
import os

import pytest
import torch

from helpers import GOLDEN, hip_model, load_golden, split_fixture, t

pytestmark = pytest.mark.gpu

TRAJ = [('gat', 'both_layerwise'), ('gat', 'both_all'), ('gat', 'only2_layerwise'), ('gat', 'only2_all'), ('gat', 'only1'),
        ('gin', 'both_layerwise'), ('gcn', 'both_all'), ('gcn', 'only2_layerwise'), ('gcn', 'only1')]
# base request -> (builder, its arguments)
BASES = {f'traj_{g}_{lt}': ('fixture', g, f'traj_{g}_{lt}.npz', lt, None) for g, lt in TRAJ}
BASES.update({
    'wide_gcn_both_all': ('fixture', 'gcn', 'traj_wide_gcn_both_all.npz', 'both_all', None),
    'wide_gat_both_layerwise': ('fixture', 'gat', 'traj_wide_gat_both_layerwise.npz', 'both_layerwise', None),
    'kld_wide_gat': ('fixture', 'gat', 'traj_wide_gat_both_layerwise.npz', 'both_layerwise', 'kld_mean'),
    'cosine_gcn': ('fixture', 'gcn', 'traj_gcn_both_all.npz', 'both_all', 'cosine_sum'),
    'sage_native': ('seeded', 'sage', 'traj_gcn_both_all.npz', None, 11),       # (gnn, graph of, input width or the fixture's, seed)
    'gin_native': ('seeded', 'gin', 'traj_gin_both_layerwise.npz', 128, 9),
    'gat_native': ('seeded', 'gat', 'traj_gat_both_layerwise.npz', 64, 3),
    'rgcn_narrow': ('kg', (32, 32, 16), 21),
    'rgcn_native': ('kg', (64, 128, 64), 5),
})
OPTS = {'plain': {}, 'cache': dict(cache_layer1=True), 'rows': dict(affected_rows_only=True),
        'cache+rows': dict(cache_layer1=True, affected_rows_only=True)}
KNOBS = ('GD_NO_FUSED_WGRAD2', 'GD_NO_STEP_TAIL', 'GD_NO_SPLIT', 'GD_NO_FUSED_LOSS1', 'GD_NO_FUSED_L2')
# every base under the four option pairs, and under each of the five knobs the trajectory tests force the fallbacks with
CASES = [(b, o, None) for b in BASES for o in OPTS] + [(b, 'plain', k) for b in BASES for k in KNOBS]


def case_id(base, opts, knob):
    return f'{base}/{opts}/{knob or "-"}'


@functools.lru_cache(maxsize=None)
def _request(base):
    """The request of a base, built once and never modified: (gnn, state, keyword arguments of NodeembEngine on the device)."""
    from oracle import gnndelete_ref as R
    kind = BASES[base][0]
    if kind == 'kg':
        from types import SimpleNamespace
        from gnndelete_amd.framework.models import RGCNDelete
        from test_engine_gpu import _kg_request
        _, (i, h, o), nr = BASES[base]
        data = _kg_request(700, 5000, nr, seed=3, n_df=60)
        n = data.num_nodes
        ni1, ni2 = R.non_df_masks(n, data.directed_df_edge_index, data.sdf_node_1hop_mask, data.sdf_node_2hop_mask)
        torch.manual_seed(5)
        make = lambda: RGCNDelete(SimpleNamespace(in_dim=i, hidden_dim=h, out_dim=o), n, nr, ni1, ni2)
        m = make().cuda()
        state = {k: v.clone() for k, v in m.state_dict().items()}
        ei, et = data.edge_index[:, data.dr_mask].cuda().contiguous(), data.edge_type[data.dr_mask].cuda().contiguous()
        pos, pt = data.edge_index[:, data.df_mask], data.edge_type[data.df_mask]
        torch.manual_seed(9)
        neg = R.negative_sampling_kg(pos[:, pt < nr], pt[pt < nr]).cuda()
        with torch.no_grad():
            z1o, z2o = m.get_original_embeddings(data.x.cuda(), ei, et, return_all_emb=True)
        return make, state, dict(x=data.x.cuda(), edge_index=ei, z1_ori=z1o, z2_ori=z2o, pos_edge=pos[:, pt < nr].cuda(), neg_edge=neg,
                                 ni_mask1=ni1, ni_mask2=ni2, loss_type='both_layerwise', alpha=0.4, lr=1e-2, edge_type=et)
    if kind == 'fixture':
        _, gnn, name, loss_type, loss_fct = BASES[base]
        state, data, rest = split_fixture(load_golden(name))
        more = dict(loss_type=loss_type, alpha=float(rest['alpha']), lr=float(rest['lr']), loss_fct=loss_fct)
    else:
        _, gnn, name, width, seed = BASES[base]
        _, data, rest = split_fixture(load_golden(name))
        torch.manual_seed(seed)
        if width:
            data = dict(data, x=torch.randn(data['x'].shape[0], width) * 0.3)
        mo = R.TwoLayerDelete(gnn, data['x'].shape[1], 128, 64, data['sdf_node_1hop_mask'], data['sdf_node_2hop_mask'])
        state = {k: v.clone() for k, v in mo.state_dict().items()}
        more = dict(loss_type='both_layerwise', alpha=0.4, lr=0.01)
    make = lambda: hip_model(gnn, state, data['sdf_node_1hop_mask'], data['sdf_node_2hop_mask'])
    ni1, ni2 = R.non_df_masks(data['x'].shape[0], data['directed_df_edge_index'], data['sdf_node_1hop_mask'],
                              data['sdf_node_2hop_mask'])
    E = data['train_pos_edge_index'].cuda()
    with torch.no_grad():
        z1o, z2o = make().get_original_embeddings(data['x'].cuda(), E[:, data['dr_mask'].cuda()], return_all_emb=True)
    return make, state, dict(x=data['x'].cuda(), edge_index=E[:, data['sdf_mask'].cuda()].contiguous(), z1_ori=z1o, z2_ori=z2o,
                             pos_edge=E[:, data['df_mask'].cuda()], neg_edge=t(rest['neg']).cuda(), ni_mask1=ni1, ni_mask2=ni2, **more)


def build_case(base, opts, knob, environ=os.environ):
    """The engine of a case on a fresh model (the knob is set only while the constructor runs)."""
    from gnndelete_amd.engine import NodeembEngine
    make, state, kw = _request(base)
    model = make()
    model.load_state_dict(state, strict=False)
    model = model.cuda()
    before = environ.get(knob) if knob else None
    if knob:
        environ[knob] = '1'
    try:
        return NodeembEngine(model, use_graph=False, **kw, **OPTS[opts])
    finally:
        if knob and before is None:
            del environ[knob]
        elif knob:
            environ[knob] = before


@functools.lru_cache(maxsize=None)
def _recorded():
    with open(os.path.join(GOLDEN, 'engine_forms.json')) as f:
        return {row['case']: row for row in json.load(f)}


def test_every_case_has_a_recorded_row():
    assert sorted(_recorded()) == sorted(case_id(*c) for c in CASES)


@pytest.mark.parametrize('base,opts,knob', CASES, ids=[case_id(*c) for c in CASES])
def test_engine_runs_the_recorded_forms(base, opts, knob):
    from gnndelete_amd.engine import Knobs
    row = _recorded()[case_id(base, opts, knob)]
    eng = build_case(base, opts, knob)
    eng.step()
    eng.step()
    assert eng.knobs == Knobs(**row['knobs'])
    assert eng.facts._asdict() == row['facts']
    assert eng.forms._asdict() == row['forms']
    for name, on in row['forms'].items():           # the attributes the step, bench.py and the other tests read
        assert getattr(eng, '_' + name) == on, name
    assert torch.isfinite(eng.loss_history()).all()
