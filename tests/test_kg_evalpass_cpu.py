"""The prepared knowledge-graph validation on the host (gnndelete_amd/evalpass.py, KGTrainer.eval under --fused_validation): the
new ABI entry and its argument checks, reference_triple_scores against a direct fp64 torch DistMult decode, every reason of
kg_validation_unsupported, the typed-graph registry of gnndelete_amd/graph.py on CPU tensors (TypedNodeCSR, the relation-major
CSR and RGATConv's edge orders are plain torch index work), and KGValidationPlan's content-checked staleness key.  No GPU."""
import ctypes
import functools
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F


def test_the_entry_is_declared_bound_and_checks_its_arguments():
    from gnndelete_amd import _lib
    names = ['gd_eval_triple_scores_f32', 'gd_eval_triple_scores_workspace']
    declared = _lib.declared_symbols()
    assert all(n in declared and n in _lib.PROTOTYPES for n in names)
    L = _lib.lib()
    assert all(hasattr(L, n) for n in names)
    assert L.gd_abi_version() == 9 and _lib.ABI_VERSION == 9
    with open(_lib.HEADER_PATH) as f:
        header = f.read()
    assert '#define GD_ABI_VERSION 9' in header and all(n + '(' in header for n in names)
    i64, i32, p = ctypes.c_int64, ctypes.c_int32, ctypes.c_void_p
    restype, argtypes = _lib.PROTOTYPES['gd_eval_triple_scores_f32']
    assert restype is ctypes.c_int and argtypes == [p, i64, i64, i32, p, i64, i64, p, p, p, i64, i64, i64, i64, p, p, p, p, p]
    assert _lib.PROTOTYPES['gd_eval_triple_scores_workspace'] == (i64, [i64, i32])
    assert L.gd_eval_triple_scores_f32.argtypes == argtypes
    # the workspace of the edge entry: a partial and a flag per block
    for m, d in ((1, 4), (257, 4), (9, 256), (4096 + 37, 256), (262144 + 5, 4), (10 ** 7, 64), (0, 4), (5, 6)):
        assert L.gd_eval_triple_scores_workspace(m, d) == L.gd_eval_edge_scores_workspace(m, d)
    # refused before anything is launched (these run without a GPU)
    mem = ctypes.create_string_buffer(8 * 64)
    a = ctypes.addressof(mem) + (-ctypes.addressof(mem) % 16)
    call = lambda z=a, ld=4, d=4, rel=a, ldr=4, nr=2, src=a, seg=(1, 1, 0, 0): L.gd_eval_triple_scores_f32(      # noqa: E731
        z, ld, 2, d, rel, ldr, nr, src, a, a, *seg, a, a, a, a, None)
    assert call(seg=(0, 0, 0, 0)) == 2 and b'segments' in L.gd_last_error_string()
    assert call(seg=(1, -1, 0, 0)) == 2
    assert call(ld=6, d=6, ldr=6) == 2 and b'multiple of 4' in L.gd_last_error_string()          # d % 4
    assert call(ld=260, d=260, ldr=260) == 2                                                        # d > 256
    assert call(ld=4, d=8, ldr=8) == 2 and call(ld=8, d=8, ldr=4) == 2                              # a pitch below d
    assert call(ldr=6) == 2                                                                         # a pitch that is no 16 bytes
    assert call(nr=0) == 2
    assert call(src=None) == 1 and call(rel=None) == 1
    assert call(z=a + 4) == 3 and call(rel=a + 4) == 3 and b'unaligned' in L.gd_last_error_string()


def _triple_case(seed, n, n_rel, d, segments, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    z, rel = torch.randn(n, d, generator=g) * scale, torch.randn(n_rel, d, generator=g)
    m = sum(segments)
    return z, rel, torch.randint(0, n, (m,), generator=g), torch.randint(0, n, (m,), generator=g), torch.randint(0, n_rel, (m,), generator=g)


def _rel_close(got, want, tol=1e-12):
    return abs(got - want) <= tol * max(abs(want), 1e-300)


@pytest.mark.parametrize('segments', [(65, 63, 1, 130), (7, 5, 0, 0), (1, 1, 1, 1), (0, 4, 3, 0), (3, 0, 2, 5)])
def test_reference_triple_scores_is_the_fp64_distmult_decode(segments):
    from gnndelete_amd.evalpass import reference_triple_scores, reference_triple_stats
    z, rel, src, dst, et = _triple_case(2, 40, 5, 12, segments, 0.9)
    n_pos, n_neg, n_df, n_dr = segments
    n_stage = n_pos + n_neg
    s64, loss, mean, std = reference_triple_scores(z, rel, src, dst, et, segments)
    logit = (z.double()[src] * rel.double()[et] * z.double()[dst]).sum(1)
    assert s64.dtype == np.float64
    assert np.abs(s64[:n_stage] - logit[:n_stage].numpy()).max(initial=0.0) <= 1e-12 * max(1.0, float(logit.abs().max()))
    assert np.abs(s64[n_stage:] - torch.sigmoid(logit[n_stage:]).numpy()).max(initial=0.0) <= 4e-16
    # the statistics are those of the fp32 values the kernel stores: raw logits in the stage, sigmoid outputs beyond it
    s32 = torch.from_numpy(s64.astype(np.float32)).double()
    label = torch.cat([torch.ones(n_pos), torch.zeros(n_neg)]).double()
    if n_stage:
        assert _rel_close(loss, float(F.binary_cross_entropy_with_logits(s32[:n_stage], label)))
    else:
        assert math.isnan(loss)
    df = s32[n_stage:n_stage + n_df].numpy()
    if n_df:
        assert _rel_close(mean, float(np.mean(df))) and abs(std - float(np.std(df))) <= 1e-12 * max(float(np.std(df)), 1e-3)
    else:
        assert math.isnan(mean) and math.isnan(std)
    given = (torch.rand(sum(segments)) * 4 - 2).float()
    assert np.array_equal(reference_triple_scores(z, rel, src, dst, et, segments, given)[1:], reference_triple_stats(given, segments),
                          equal_nan=True)
    with pytest.raises(ValueError, match='do not add up'):
        reference_triple_scores(z, rel, src, dst, et, (1, 1, 1, 0) if sum(segments) != 3 else (1, 1, 1, 1))


def test_reference_triple_scores_edges():
    from gnndelete_amd.evalpass import reference_triple_scores, reference_triple_stats
    # logits +-200: the loss terms are |l| or 0 to the bit of fp64, nothing overflows
    loss, mean, std = reference_triple_stats(np.array([200.0, -200.0, 200.0, -200.0, 0.5], dtype=np.float32), (2, 2, 1, 0))
    assert loss == pytest.approx((0.0 + 200.0 + 200.0 + 0.0) / 4, rel=1e-15) and mean == 0.5 and std == 0.0
    want = float(F.binary_cross_entropy_with_logits(torch.tensor([200.0, -200.0, 200.0, -200.0]).double(), torch.tensor([1.0, 1.0, 0.0, 0.0]).double()))
    assert _rel_close(loss, want)
    # through the decode: z and rel chosen so that the logits are exactly +-200 and 0; a type and an endpoint out of range score 0
    z = torch.tensor([[10.0, 0.0, 0.0, 0.0], [-10.0, 0.0, 0.0, 0.0], [0.0, 0.0, 0.0, 0.0]])
    rel = torch.tensor([[2.0, 1.0, 1.0, 1.0], [-2.0, 1.0, 1.0, 1.0]])
    src, dst, et = torch.tensor([0, 0, 2, 0, 0, 0, 0, 0]), torch.tensor([0, 1, 2, 7, 0, 0, 1, 0]), torch.tensor([0, 0, 0, 0, 2, 0, 0, 1])
    s64, loss, mean, std = reference_triple_scores(z, rel, src, dst, et, (2, 3, 3, 0))
    assert s64[:5].tolist() == [200.0, -200.0, 0.0, 0.0, 0.0]
    assert s64[5] == 1.0 and 0.0 < s64[6] < 1e-80 and 0.0 < s64[7] < 1e-80
    assert np.isfinite(loss) and _rel_close(loss, (0.0 + 200.0 + 3 * math.log(2.0)) / 5) and np.isfinite(mean)
    # no stage triples: NaN loss; no Df: NaN mean / std
    loss, mean, std = reference_triple_stats(np.array([0.25, 0.75], dtype=np.float32), (0, 0, 2, 0))
    assert math.isnan(loss) and mean == 0.5 and std == 0.25
    loss, mean, std = reference_triple_stats(np.array([0.25, 0.75], dtype=np.float32), (1, 1, 0, 0))
    assert np.isfinite(loss) and math.isnan(mean) and math.isnan(std)


def _kg_model(kind='rgcn', delete=False, out_dim=8, nr=3):
    from gnndelete_amd.framework import models as M
    args = SimpleNamespace(in_dim=8, hidden_dim=8, out_dim=out_dim)
    cls = getattr(M, kind.upper() + ('Delete' if delete else ''))
    return cls(args, 6, nr)


def test_every_kg_fallback_has_its_reason():
    from gnndelete_amd.evalpass import kg_validation_unsupported
    from gnndelete_amd.framework import get_model
    from gnndelete_amd.rankeval import fused_eval_unsupported
    for kind in ('rgcn', 'rgat'):
        assert kg_validation_unsupported(_kg_model(kind)) is None and kg_validation_unsupported(_kg_model(kind, delete=True)) is None
    kg = _kg_model()
    gcn = get_model(SimpleNamespace(unlearning_model='retrain', gnn='gcn', in_dim=8, hidden_dim=16, out_dim=32))
    reasons = [
        kg_validation_unsupported(gcn),
        kg_validation_unsupported(torch.nn.Linear(3, 3)),
        kg_validation_unsupported(kg, 32, on_gpu=False),
        kg_validation_unsupported(kg, 32, torch.float64),
        kg_validation_unsupported(kg, 6),
        kg_validation_unsupported(kg, 260),
        kg_validation_unsupported(kg, rankings=[(10, 100, 10), (0, 100, 10)]),
        kg_validation_unsupported(kg, 64, rankings=[(10, 100, 101)]),
    ]
    assert reasons == [
        'no prepared knowledge-graph validation for the GCN model (RGCN, RGAT and their Delete wrappers only)',
        'no prepared knowledge-graph validation for the Linear model (RGCN, RGAT and their Delete wrappers only)',
        'the embeddings or the DistMult table are not on the GPU',
        'torch.float64 embeddings or DistMult table (float32 only)',
        'DistMult width 6 (a multiple of 4 up to 256)',
        'DistMult width 260 (a multiple of 4 up to 256)',
        fused_eval_unsupported(0, 100, 10),
        fused_eval_unsupported(10, 100, 101),
    ]
    assert len(set(reasons)) == len(reasons) and all(r and '\n' not in r for r in reasons)
    assert kg_validation_unsupported(kg, 4) is None and kg_validation_unsupported(kg, 256, rankings=[(3, 9, 3)]) is None
    assert kg_validation_unsupported(kg, 0) == 'DistMult width 0 (a multiple of 4 up to 256)'


# ------------------------------------------------------------------------------------------ the typed-graph registry
@pytest.fixture
def typed_builds(monkeypatch):
    """Counts the constructions of the three per-graph structures (the real builders run: plain torch on CPU tensors)."""
    from gnndelete_amd import graph, nn as gnn
    counts = {'nodes': 0, 'rel': 0, 'orders': 0}
    init, rel, orders = graph.TypedNodeCSR.__init__, gnn.build_typed_csr, gnn.RGATConv._build_edge_orders

    def counted_init(self, *a, **k):
        counts['nodes'] += 1
        return init(self, *a, **k)

    def counted_rel(*a, **k):
        counts['rel'] += 1
        return rel(*a, **k)

    def counted_orders(self, *a, **k):
        counts['orders'] += 1
        return orders(self, *a, **k)
    monkeypatch.setattr(graph.TypedNodeCSR, '__init__', counted_init)
    monkeypatch.setattr(gnn, 'build_typed_csr', counted_rel)
    monkeypatch.setattr(gnn.RGATConv, '_build_edge_orders', counted_orders)
    return counts


def _pair(seed, n=9, r=4, e=30):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, n, (2, e), generator=g), torch.randint(0, r, (e,), generator=g)


def test_a_pinned_pair_is_built_once_for_every_conv(typed_builds):
    from gnndelete_amd import graph
    from gnndelete_amd.nn import RGATConv, RGCNConv
    n, r = 9, 4
    c1, c2, a1, a2 = RGCNConv(8, 8, r), RGCNConv(8, 4, r), RGATConv(8, 8, r), RGATConv(8, 4, r)
    ei, et = _pair(0)
    graph.TYPED.pin(ei, et)
    try:
        tg = c1._typed_node_csr(ei, et, n)
        assert c2._typed_node_csr(ei, et, n) is tg and a1._typed_node_csr(ei, et, n) is tg and a2._typed_node_csr(ei, et, n) is tg
        rel = c1._typed_csr(ei, et, n)
        assert c2._typed_csr(ei, et, n) is rel
        orders = a1._edge_orders(ei, et, n)
        assert a2._edge_orders(ei, et, n) is orders
        assert typed_builds == {'nodes': 1, 'rel': 1, 'orders': 1}
        assert c1._typed_nodes is None and c1._typed is None and getattr(a1, '_orders', None) is None       # the one slots are not touched
        # other graphs pass through the convs: the pinned structures stay
        for seed in range(1, 11):
            oi, ot = _pair(seed)
            for conv in (c1, c2, a1, a2):
                conv._typed_node_csr(oi, ot, n)
            c1._typed_csr(oi, ot, n)
            a1._edge_orders(oi, ot, n)
        assert typed_builds == {'nodes': 1 + 40, 'rel': 1 + 10, 'orders': 1 + 10}
        assert c2._typed_node_csr(ei, et, n) is tg and c1._typed_csr(ei, et, n) is rel and a2._edge_orders(ei, et, n) is orders
        assert typed_builds == {'nodes': 41, 'rel': 11, 'orders': 11}
        # another node or relation count is another structure
        assert c1._typed_node_csr(ei, et, n + 1) is not tg and typed_builds['nodes'] == 42
        assert RGCNConv(8, 8, r + 1)._typed_node_csr(ei, et, n) is not tg and typed_builds['nodes'] == 43
        # an in-place edit of either tensor rebuilds once, for both convs again
        et[0] = (et[0] + 1) % r
        tg2 = c1._typed_node_csr(ei, et, n)
        assert tg2 is not tg and c2._typed_node_csr(ei, et, n) is tg2 and typed_builds['nodes'] == 44
        ei[0, 0] = (ei[0, 0] + 1) % n
        assert a1._edge_orders(ei, et, n) is not orders and a2._edge_orders(ei, et, n) is a1._edge_orders(ei, et, n)
        assert typed_builds['orders'] == 12
        # pins count
        graph.TYPED.pin(ei, et)
        graph.TYPED.unpin(ei, et)
        assert graph.TYPED.pinned(ei, et) and c1._typed_node_csr(ei, et, n) is c2._typed_node_csr(ei, et, n)
    finally:
        graph.TYPED.unpin(ei, et)
    assert not graph.TYPED.pinned(ei, et) and (id(ei), id(et)) not in graph.TYPED.held
    graph.TYPED.unpin(ei, et)                                        # once too often: nothing happens
    # gone after unpin: the one-slot path again, one graph per conv
    before = dict(typed_builds)
    assert c1._typed_node_csr(ei, et, n) is not c2._typed_node_csr(ei, et, n)
    assert typed_builds['nodes'] == before['nodes'] + 2 and c1._typed_nodes is not None


def test_an_unpinned_pair_takes_the_one_slot_path(typed_builds):
    from gnndelete_amd import graph
    from gnndelete_amd.nn import RGATConv, RGCNConv
    n, r = 9, 4
    c1, c2, a1 = RGCNConv(8, 8, r), RGCNConv(8, 4, r), RGATConv(8, 8, r)
    ei, et = _pair(0)
    held_before = dict(graph.TYPED.held)
    tg = c1._typed_node_csr(ei, et, n)
    assert c1._typed_node_csr(ei, et, n) is tg and c1._typed_nodes[1] is tg and typed_builds['nodes'] == 1
    assert c2._typed_node_csr(ei, et, n) is not tg and typed_builds['nodes'] == 2                  # one each, as before
    oi, ot = _pair(1)
    c1._typed_node_csr(oi, ot, n)
    assert c1._typed_node_csr(ei, et, n) is not tg and typed_builds['nodes'] == 4                  # the slot was overwritten
    assert c1._typed_csr(ei, et, n) is c1._typed_csr(ei, et, n) and typed_builds['rel'] == 1
    tc = a1._edge_orders(ei, et, n)
    assert a1._edge_orders(ei, et, n) is tc and a1._orders[1] is tc and typed_builds['orders'] == 1
    assert set(graph.TYPED.held) == set(held_before) and graph.TYPED.get('nodes', ei, et, n, r, lambda: 1 / 0) is None
    # the structures of a pinned pair are those the one-slot path builds
    graph.TYPED.pin(ei, et)
    try:
        shared = c2._typed_node_csr(ei, et, n)
        own = c1._typed_nodes[1]
        assert all(torch.equal(x, y) for x, y in zip(shared.fwd + shared.bwd, own.fwd + own.bwd))
        assert all(torch.equal(x, y) for x, y in zip(c2._typed_csr(ei, et, n), c1._typed[1]))
        held_orders = RGATConv(8, 4, r)._edge_orders(ei, et, n)
        assert sorted(held_orders) == sorted(tc) and all(torch.equal(held_orders[k], tc[k]) for k in tc if torch.is_tensor(tc[k]))
    finally:
        graph.TYPED.unpin(ei, et)


# ------------------------------------------------------------------------------------------ the plan
@functools.lru_cache(maxsize=None)
def _prepared():
    from gnndelete_amd.framework.data import prepare_edge_deletion
    from gnndelete_amd.framework.synth import make_kg_dataset
    data, dfm = make_kg_dataset(None, seed=3, shape=(120, 3, 700))
    state = torch.get_rng_state()
    torch.manual_seed(3)
    prepare_edge_deletion(data, dfm['in'], 20, True, 3)
    torch.set_rng_state(state)
    return data


def _request():
    return _prepared().clone()


def _trainer(kind='gnndelete_nodeemb'):
    return SimpleNamespace(args=SimpleNamespace(unlearning_model=kind), FAST_SUBSETS_ABOVE=1 << 18, trainer_log={})


def test_the_plan_is_built_from_cpu_data_as_eval_builds_its_lists(monkeypatch):
    from gnndelete_amd import _lib, evalpass, graph
    monkeypatch.setattr(_lib, 'lib', lambda: 1 / 0)                  # no kernel, not even the library, in __init__
    data = _request()
    plan = evalpass.KGValidationPlan(_trainer(), data, 'val', 'cpu')
    try:
        assert torch.equal(plan.edges, data.edge_index[:, data.dr_mask]) and plan.edges.is_contiguous()
        assert torch.equal(plan.types, data.edge_type[data.dr_mask]) and graph.TYPED.pinned(plan.edges, plan.types)
        half = data.dr_mask[:data.dr_mask.shape[0] // 2]
        n_pos, n_neg = data.val_pos_edge_index.shape[1], data.val_neg_edge_index.shape[1]
        assert plan.segments == (n_pos, n_neg, 20, int(half.sum())) and n_pos > 0 and int(half.sum()) == data.train_pos_edge_index.shape[1] - 20
        assert plan.decoded.dtype == torch.int64 and plan.etype.dtype == torch.int64 and plan.decoded.is_contiguous()
        assert torch.equal(plan.decoded, torch.cat([data.val_pos_edge_index, data.val_neg_edge_index, data.directed_df_edge_index,
                                                    data.train_pos_edge_index[:, half]], 1))
        assert torch.equal(plan.etype, torch.cat([data.val_edge_type, data.val_edge_type, data.directed_df_edge_type, data.train_edge_type[half]]))
        assert plan.src is not None and torch.equal(plan.src, plan.decoded[0]) and torch.equal(plan.dst, plan.decoded[1])
        assert torch.equal(plan.all_positives, torch.arange(n_pos)[None])
        assert plan.rankings() == [(n_neg, n_pos, n_pos), (20, int(half.sum()), 20)]
    finally:
        plan.release()
    assert not graph.TYPED.pinned(plan.edges, plan.types)
    # `original` decodes the stage only
    plan = evalpass.KGValidationPlan(_trainer('original'), data, 'test', 'cpu')
    n_pos = data.test_pos_edge_index.shape[1]
    assert plan.segments == (n_pos, data.test_neg_edge_index.shape[1], 0, 0) and plan.decoded.shape[1] == 2 * n_pos
    assert torch.equal(plan.etype, torch.cat([data.test_edge_type, data.test_edge_type])) and len(plan.rankings()) == 1
    plan.release()


def test_the_staleness_key_survives_the_round_trip_and_sees_every_edit():
    from gnndelete_amd.evalpass import KGValidationPlan
    data = _request()
    plan = KGValidationPlan(_trainer(), data, 'val', 'cpu')
    edges, decoded = plan.edges, plan.decoded
    names = ('edge_index', 'edge_type', 'dr_mask', 'val_pos_edge_index', 'val_neg_edge_index', 'val_edge_type', 'directed_df_edge_index',
             'directed_df_edge_type', 'train_pos_edge_index', 'train_edge_type')
    assert [s is data[k] for s, k in zip(plan._sources, names)] == [True] * 10
    # identity hit: nothing is compared
    key = plan.key
    assert plan.current(data, 'val', False, 'cpu') and plan.key is key
    assert not plan.current(data, 'test', False, 'cpu') and not plan.current(data, 'val', True, 'cpu') and not plan.current(data, 'val', False, 'cuda:0')
    # the round trip: every source is another tensor of equal contents -> adopted, everything derived kept
    moved = data.clone()
    assert plan.current(moved, 'val', False, 'cpu') and plan.key != key
    assert all(s is moved[k] for s, k in zip(plan._sources, names)) and plan.edges is edges and plan.decoded is decoded
    assert plan.current(moved, 'val', False, 'cpu')                  # and now by identity
    # a tensor that is no source of this plan may change
    moved.test_pos_edge_index[0, 0] += 1
    moved.x = moved.x.clone()
    assert plan.current(moved, 'val', False, 'cpu')
    # one entry of dr_mask changed in another copy: rebuild (and the plan is left as it was)
    changed = moved.clone()
    changed.dr_mask[5] = ~changed.dr_mask[5]
    assert not plan.current(changed, 'val', False, 'cpu') and all(s is moved[k] for s, k in zip(plan._sources, names))
    for k in names:
        other = moved.clone()
        other[k].view(-1)[-1] = other[k].view(-1)[-1] + 1 if other[k].dtype != torch.bool else ~other[k].view(-1)[-1]
        assert not plan.current(other, 'val', False, 'cpu'), k
    # another shape or dtype is not compared at all
    other = moved.clone()
    other.val_pos_edge_index = other.val_pos_edge_index[:, :-1]
    assert not plan.current(other, 'val', False, 'cpu')
    other = moved.clone()
    other.edge_type = other.edge_type.int()
    assert not plan.current(other, 'val', False, 'cpu')
    # an in-place edit of a held source is seen through its version, whatever the values
    moved.edge_type[0] = moved.edge_type[0]
    assert not plan.current(moved, 'val', False, 'cpu')
    assert not plan.current(moved.clone(), 'val', False, 'cpu')      # (the held tensor is no longer the one the plan was derived from)
    plan.release()


def test_the_hook_records_its_reason_once_and_returns_none(capsys):
    from gnndelete_amd import evalpass
    from gnndelete_amd.framework import get_model
    tr = _trainer()
    gcn = get_model(SimpleNamespace(unlearning_model='retrain', gnn='gcn', in_dim=8, hidden_dim=16, out_dim=32))
    for _ in range(2):
        assert evalpass.prepared_kg_validation(tr, gcn, _request(), 'val', False, 'cpu') is None
    reason = 'no prepared knowledge-graph validation for the GCN model (RGCN, RGAT and their Delete wrappers only)'
    assert tr.trainer_log['validation_path'] == 'torch: ' + reason
    assert capsys.readouterr().out.count(f'--fused_validation: {reason}; validating on the torch path') == 1
    # a width the kernel does not take is refused before a plan is built (the model's table is on the host here: said first)
    assert evalpass.prepared_kg_validation(tr, _kg_model(out_dim=6), _request(), 'val', False, 'cpu') is None
    assert tr.trainer_log['validation_path'] == 'torch: the embeddings or the DistMult table are not on the GPU'
    assert '_validation_plans' not in tr.__dict__


def test_the_kg_trainer_consults_the_flag_first(tmp_path, monkeypatch):
    from gnndelete_amd import evalpass
    from gnndelete_amd.framework.trainer import kg as TK
    calls = []
    monkeypatch.setattr(evalpass, 'prepared_kg_validation', lambda tr, model, data, stage, pred_all, dev: calls.append((stage, pred_all)))
    monkeypatch.setattr(TK, '_require_gpu', lambda: None)
    monkeypatch.setattr(TK, 'device', torch.device('cpu'))

    class Stop(Exception):
        pass

    def stop(*a, **k):
        raise Stop
    model = _kg_model(nr=3)
    monkeypatch.setattr(type(model), 'forward', stop)
    mk = lambda **flags: SimpleNamespace(dataset='synth-kg-tiny', unlearning_model='retrain', checkpoint_dir=str(tmp_path), **flags)       # noqa: E731
    for cls in (TK.KGTrainer, TK.KGGNNDeleteNodeembTrainer):
        with pytest.raises(Stop):
            cls(mk()).eval(model, _request(), 'val')
        assert calls == []
        with pytest.raises(Stop):                                    # the hook gave None: today's path runs
            cls(mk(fused_validation=True)).eval(model, _request(), 'test', True)
        assert calls == [('test', True)]
        calls.clear()
    from gnndelete_amd.framework.training_args import EXTRA_FLAGS
    (text,) = [help_ for name, _, _, help_ in EXTRA_FLAGS if name == 'fused_validation']
    assert 'KGTrainer.eval' in text and 'not the knowledge-graph trainer' not in text
