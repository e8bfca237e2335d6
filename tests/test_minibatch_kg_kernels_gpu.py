"""The two integer kernels of the fused knowledge-graph batch step (gnndelete_amd.minibatch): gd_induced_subgraph_typed against
RandomWalkSubgraphSampler.subgraph followed by KGGNNDeleteNodeembTrainer's masking, gd_batch_typed_csr against
graph.TypedNodeCSR - every array bit for bit."""
import pytest
import torch

pytestmark = pytest.mark.gpu

N, R = 60, 6            # 6 relation types, 12 with the reverse ones


def _kg_graph():
    """60 nodes in regions that share no edge:
      0 .. 29   random typed edges and their reverses; node 0 has 80 out-edges to nodes 1 .. 20 (four each, several types);
                5 -> 7 is given three times with types 4, 1, 3 in that input order; some edges are Df, of both directions
      30 .. 39  Dr edges only (no Df triple)
      40 .. 49  Df edges only (no Dr edge), forward and reverse types
      50 .. 59  Dr edges plus Df edges of REVERSE types only (nothing to decode)"""
    from gnndelete_amd.framework.data import Data
    g = torch.Generator().manual_seed(11)

    def rand_edges(lo, hi, m):
        ei = torch.randint(lo, hi, (2, m), generator=g)
        ty = torch.randint(0, R, (m,), generator=g)
        return torch.cat([ei, ei.flip(0)], 1), torch.cat([ty, ty + R])

    parts, types, dr, df = [], [], [], []

    def add(ei, ty, dr_, df_):
        parts.append(ei), types.append(ty), dr.append(dr_), df.append(df_)

    ei, ty = rand_edges(0, 30, 150)
    free = ~(((ei[0] == 5) & (ei[1] == 7)) | ((ei[0] == 7) & (ei[1] == 5)))      # (5 -> 7 belongs to the three parallel edges below)
    ei, ty = ei[:, free], ty[free]
    is_df = torch.rand(ei.shape[1], generator=g) < 0.15
    add(ei, ty, ~is_df, is_df)
    hub = torch.stack([torch.zeros(80, dtype=torch.long), torch.arange(80) % 20 + 1])
    add(hub, torch.arange(80) % 5, torch.ones(80, dtype=torch.bool), torch.zeros(80, dtype=torch.bool))
    ei, ty = rand_edges(30, 40, 25)
    add(ei, ty, torch.ones(50, dtype=torch.bool), torch.zeros(50, dtype=torch.bool))
    ei, ty = rand_edges(40, 50, 25)
    add(ei, ty, torch.zeros(50, dtype=torch.bool), torch.ones(50, dtype=torch.bool))
    ei, ty = rand_edges(50, 60, 30)
    rev_df = (ty >= R) & (torch.rand(60, generator=g) < 0.5)
    add(ei, ty, ~rev_df, rev_df)
    ei, ty, dr_m, df_m = torch.cat(parts, 1), torch.cat(types), torch.cat(dr), torch.cat(df)
    perm = torch.randperm(ei.shape[1], generator=g)
    ei, ty, dr_m, df_m = ei[:, perm], ty[perm], dr_m[perm], df_m[perm]
    # 5 -> 7 three times, types 4, 1, 3 in that input order, far apart in the edge list
    for at, typ in ((100, 4), (201, 1), (ei.shape[1] + 2, 3)):
        ei = torch.cat([ei[:, :at], torch.tensor([[5], [7]]), ei[:, at:]], 1)
        ty = torch.cat([ty[:at], torch.tensor([typ]), ty[at:]])
        dr_m = torch.cat([dr_m[:at], torch.tensor([True]), dr_m[at:]])
        df_m = torch.cat([df_m[:at], torch.tensor([False]), df_m[at:]])
    d = Data(num_nodes=N, x=torch.arange(N), edge_index=ei.contiguous(), edge_type=ty.contiguous(), dr_mask=dr_m, df_mask=df_m)
    d.sdf_node_1hop_mask_non_df_mask = torch.rand(N, generator=g) < 0.4
    d.sdf_node_2hop_mask_non_df_mask = torch.rand(N, generator=g) < 0.6
    return d


def _reference(sampler, nodes):
    """subgraph() + the trainer's masking (kg_batch_cases.cut_reference, shared with the tests past one scan chunk)."""
    from kg_batch_cases import cut_reference
    return cut_reference(sampler, nodes, R)


def _raw_cut(cut, nodes, cap, generation):
    """gd_induced_subgraph_typed into fresh buffers filled with -7, capacity `cap`."""
    from gnndelete_amd import _lib
    from gnndelete_amd._lib import check, ptr, stream_ptr
    dev = cut.dev
    L = _lib.lib()
    n_b = int(nodes.numel())
    c = max(cap, 1)
    out = dict(dr=torch.full((3, c), -7, dtype=torch.int32, device=dev), df_index=torch.full((2, c), -7, dtype=torch.int64, device=dev),
               df_type=torch.full((c,), -7, dtype=torch.int64, device=dev), rows=torch.full((2 * n_b,), -7, dtype=torch.int32, device=dev),
               counts=torch.full((6,), -7, dtype=torch.int32, device=dev))
    ws = torch.empty(max(256, L.gd_induced_subgraph_typed_workspace(n_b)), dtype=torch.uint8, device=dev)
    nodes = nodes.to(dev, torch.int64).contiguous()
    check(L.gd_induced_subgraph_typed(ptr(cut.rowptr32), ptr(cut.col32), ptr(cut.edge_type32), ptr(cut.edge_flags), cut.n, R,
                                      ptr(nodes), n_b, ptr(cut.node_flags), generation, ptr(cut.relabel), cap, ptr(out['dr'][0]),
                                      ptr(out['dr'][1]), ptr(out['dr'][2]), ptr(out['df_index']), ptr(out['df_type']),
                                      ptr(out['rows']), ptr(out['counts']), ptr(ws), ws.numel(), stream_ptr(dev)),
          'gd_induced_subgraph_typed')
    return out


@pytest.fixture(scope='module')
def kg():
    from gnndelete_amd.framework.trainer.sampler import RandomWalkSubgraphSampler
    from gnndelete_amd.minibatch import KGBatchCut
    d = _kg_graph()
    dev = torch.device('cuda')
    sampler = RandomWalkSubgraphSampler(d.clone().to(dev), batch_size=8)
    return d, sampler, KGBatchCut(d, sampler, dev, R, max_nodes=16)


def _assert_cut(cut, sampler, nodes):
    dev = cut.dev
    cnt = cut.cut(nodes.to(dev))
    dr_index, dr_type, dec_index, dec_type, rows, m_df_all = _reference(sampler, nodes.to(dev))
    e_dr, m_dec = dr_index.shape[1], dec_index.shape[1]
    assert cnt == [nodes.numel(), e_dr, m_dec, rows[0].numel(), rows[1].numel(), 0]
    assert torch.equal(cut.dr[:2, :e_dr].long(), dr_index) and torch.equal(cut.dr[2, :e_dr].long(), dr_type)
    assert torch.equal(cut.df_index[:, :m_dec], dec_index) and torch.equal(cut.df_type[:m_dec], dec_type)
    for k in (0, 1):
        assert torch.equal(cut.rows(k, cnt[3 + k]), rows[k])
    return cnt, m_df_all


def test_typed_cut_matches_subgraph_and_the_trainers_masking(kg):
    d, sampler, cut = kg
    g = torch.Generator().manual_seed(2)
    # the hub row (80 out-edges to nodes 1 .. 20: more than 64 inside the batch) and the parallel 5 -> 7 edges
    cnt, _ = _assert_cut(cut, sampler, torch.arange(0, 30))
    src, dst, ty = cut.dr[:, :cnt[1]].long()
    assert int((src == 0).sum()) > 64
    assert ty[(src == 5) & (dst == 7)].tolist() == [4, 1, 3]                  # input order, not type order
    # random batches across the regions, all nodes, single nodes
    for nodes in [torch.randperm(N, generator=g)[:25].sort().values, torch.randperm(N, generator=g)[:40].sort().values,
                  torch.arange(N), torch.tensor([0]), torch.tensor([7])]:
        _assert_cut(cut, sampler, nodes)
    cnt, _ = _assert_cut(cut, sampler, torch.arange(40, 50))                # no Dr edge
    assert cnt[1] == 0 and cnt[2] > 0
    cnt, _ = _assert_cut(cut, sampler, torch.arange(30, 40))                # no Df triple
    assert cnt[1] > 0 and cnt[2] == 0
    cnt, m_df_all = _assert_cut(cut, sampler, torch.arange(50, 60))         # Df edges of reverse types only: nothing decoded
    assert cnt[2] == 0 and m_df_all > 0


def test_typed_cut_flags_a_node_id_out_of_range(kg):
    d, sampler, cut = kg
    nodes = torch.tensor([0, 3, 5, 7, 12, 31, 44, N + 5])
    cut.generation += 1
    out = _raw_cut(cut, nodes, 4096, cut.generation)
    dr_index, dr_type, dec_index, dec_type, rows, _ = _reference(sampler, nodes[:-1].to(cut.dev))       # the bad row is empty
    cnt = out['counts'].tolist()
    assert cnt == [nodes.numel(), dr_index.shape[1], dec_index.shape[1], rows[0].numel(), rows[1].numel(), 1]
    assert torch.equal(out['dr'][:2, :cnt[1]].long(), dr_index) and torch.equal(out['dr'][2, :cnt[1]].long(), dr_type)
    assert torch.equal(out['df_index'][:, :cnt[2]], dec_index) and torch.equal(out['df_type'][:cnt[2]], dec_type)
    n_b = nodes.numel()
    for k in (0, 1):
        assert torch.equal(out['rows'][k * n_b:k * n_b + cnt[3 + k]], rows[k])
    with pytest.raises(IndexError):
        cut.cut(nodes)
    # the flag is this call's own: the next cut of good nodes clears it
    cut.generation += 1
    assert _raw_cut(cut, nodes[:-1], 4096, cut.generation)['counts'].tolist()[5] == 0


def test_typed_cut_with_a_capacity_one_short_writes_counts_only(kg):
    d, sampler, cut = kg
    nodes = torch.arange(0, 30)
    dr_index, dr_type, dec_index, dec_type, rows, _ = _reference(sampler, nodes.to(cut.dev))
    need = max(dr_index.shape[1], dec_index.shape[1])
    cut.generation += 1
    out = _raw_cut(cut, nodes, need - 1, cut.generation)
    assert out['counts'].tolist() == [30, dr_index.shape[1], dec_index.shape[1], rows[0].numel(), rows[1].numel(), 0]
    assert bool((out['dr'] == -7).all()) and bool((out['df_index'] == -7).all()) and bool((out['df_type'] == -7).all())
    out = _raw_cut(cut, nodes, need, cut.generation)                       # the re-cut (same generation)
    assert torch.equal(out['dr'][:2, :dr_index.shape[1]].long(), dr_index) and torch.equal(out['dr'][2, :dr_index.shape[1]].long(), dr_type)
    assert torch.equal(out['df_index'][:, :dec_index.shape[1]], dec_index)
    assert torch.equal(out['df_type'][:dec_index.shape[1]], dec_type)
    # the step's own buffers grow the same way
    cut.e_cap = need - 1
    cut.dr, cut.df_index, cut.df_type = cut.dr[:, :need - 1].contiguous(), cut.df_index[:, :need - 1].contiguous(), cut.df_type[:need - 1]
    reads = cut.reads
    _assert_cut(cut, sampler, nodes)
    assert cut.reads == reads + 2 and cut.e_cap >= need


# ------------------------------------------------------------------------------------------------ gd_batch_typed_csr
def _typed_cases():
    g = torch.Generator().manual_seed(4)
    n, r = 60, 12
    ei = torch.randint(0, 59, (2, 300), generator=g)                        # node 59: no in-edge, no out-edge
    ty = torch.randint(0, r, (300,), generator=g)
    run70 = torch.stack([torch.randint(0, 59, (70,), generator=g), torch.full((70,), 13)])      # 70 type-3 in-edges of node 13
    run1 = torch.tensor([[2], [58]])                                        # node 58's only in-edge: a run of one
    ei = ei[:, ei[1] != 58]
    ty = ty[:ei.shape[1]]
    mixed = (torch.cat([ei, run70, run1], 1), torch.cat([ty, torch.full((70,), 3), torch.tensor([11])]), n, r)
    p = torch.randperm(mixed[0].shape[1], generator=g)
    mixed = (mixed[0][:, p].contiguous(), mixed[1][p].contiguous(), n, r)
    one_rel = (torch.randint(0, 40, (2, 200), generator=g), torch.full((200,), 5), 40, 12)
    empty = (torch.zeros(2, 0, dtype=torch.long), torch.zeros(0, dtype=torch.long), 33, 12)
    many_rel = (torch.randint(0, 60, (2, 500), generator=g), torch.randint(0, 102, (500,), generator=g), 60, 102)
    single = (torch.tensor([[4], [4]]), torch.tensor([0]), 9, 2)
    return {'mixed': mixed, 'one_relation': one_rel, 'zero_edges': empty, 'relations_102': many_rel, 'one_edge': single}


def _assert_typed(got, ref, tag):
    for side in ('fwd', 'bwd'):
        g_, r_ = getattr(got, side), getattr(ref, side)
        s = int(got.status[0 if side == 'fwd' else 1])
        e = got.n_edges
        assert s == r_[2].numel(), (tag, side)
        assert torch.equal(g_[0].cpu(), r_[0]), (tag, side, 'node_ptr')
        assert torch.equal(g_[1][:s + 1].cpu(), r_[1]), (tag, side, 'seg_ptr')
        assert torch.equal(g_[2][:s].cpu(), r_[2]), (tag, side, 'seg_rel')
        assert torch.equal(g_[3][:e].cpu(), r_[3]), (tag, side, 'col')
        assert torch.equal(g_[4][:e].cpu().view(torch.int32), r_[4].view(torch.int32)), (tag, side, 'w')
    assert got.status[2:].tolist() == [0, 0]


@pytest.mark.parametrize('case', ['mixed', 'one_relation', 'zero_edges', 'relations_102', 'one_edge'])
def test_batch_typed_csr_matches_typed_node_csr(case):
    """Against graph.TypedNodeCSR built on the HOST from the same edges (IEEE division: 1 / |run| correctly rounded)."""
    from gnndelete_amd.graph import TypedNodeCSR
    from gnndelete_amd.minibatch import batch_typed_csr
    ei, ty, n, r = _typed_cases()[case]
    ref = TypedNodeCSR(ei, ty, n, r)
    if case == 'mixed':
        lens = (ref.fwd[1][1:] - ref.fwd[1][:-1])
        assert int(lens.max()) >= 70 and int(lens.min()) == 1
        assert int(ref.fwd[0][59]) == int(ref.fwd[0][60])                       # a node with no in-edge
    dev = torch.device('cuda')
    src, dst, et = (v.to(dev, torch.int32).contiguous() for v in (ei[0], ei[1], ty))
    bufs = {}
    got = batch_typed_csr(src, dst, et, ei.shape[1], n, r, bufs)
    _assert_typed(got, ref, case)
    again = batch_typed_csr(src, dst, et, ei.shape[1], n, r, bufs, into=got)       # the same buffers, the same workspace
    assert again is got
    _assert_typed(again, ref, case + ' (second call)')


def test_batch_typed_csr_leaves_out_edges_out_of_range():
    from gnndelete_amd.graph import TypedNodeCSR
    from gnndelete_amd.minibatch import batch_typed_csr
    ei = torch.tensor([[0, 1, 2, 9, 3], [1, 2, 0, 1, 3]])
    ty = torch.tensor([0, 1, 1, 0, 7])
    dev = torch.device('cuda')
    got = batch_typed_csr(*(v.to(dev, torch.int32).contiguous() for v in (ei[0], ei[1], ty)), 5, 4, 2)
    assert got.status.tolist()[2] == 1
    ref = TypedNodeCSR(ei[:, :3], ty[:3], 4, 2)
    s = int(got.status[0])
    assert s == 3 and torch.equal(got.fwd[0].cpu(), ref.fwd[0]) and torch.equal(got.fwd[3][:3].cpu(), ref.fwd[3])
    assert torch.equal(got.bwd[0].cpu(), ref.bwd[0]) and torch.equal(got.bwd[3][:3].cpu(), ref.bwd[3])
