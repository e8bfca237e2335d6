"""The two integer kernels of the fused knowledge-graph batch step (csrc/subgraph_typed.hip) past one 1,024-element chunk of
their single-block scans: gd_induced_subgraph_typed on node sets of 1,023 .. 4,261 rows against
RandomWalkSubgraphSampler.subgraph + the trainer's masking, gd_batch_typed_csr against a plain numpy reference on graphs of
1,023 .. 2,049 nodes, on runs laid out around the sorted positions 1,024 and 2,048, on hubs of 3,000 edges with parallel
edges, and with edges out of range.  The cases are kg_batch_cases.py's; test_kg_batch_cases_cpu.py checks on the host that
they reach the boundaries they are built for and that a scan without its carry cannot reproduce them.  Every array is
compared bit for bit (torch.equal, weights as int32): there is no tolerance in this file."""
import pytest
import torch

import kg_batch_cases as K

pytestmark = pytest.mark.gpu
NR = 25
PAD = 64                        # raw output buffers are this much longer than the capacity they are called with
FILL = -7


@pytest.fixture(scope='module')
def kg():
    from gnndelete_amd.framework.trainer.sampler import RandomWalkSubgraphSampler
    from gnndelete_amd.minibatch import KGBatchCut
    data, info = K.planted_request(NR)
    dev = torch.device('cuda')
    sampler = RandomWalkSubgraphSampler(data.clone().to(dev), batch_size=8)
    return data, info, sampler, KGBatchCut(data, sampler, dev, NR, max_nodes=16)


def _reference(sampler, key):
    """The trainer-masking reference of a node set on the DEVICE sampler (the host one gave the same: the CPU test)."""
    ref = K.cut_reference(sampler, K.node_sets(NR)[key].to(sampler.dev), NR)
    host = K.cut_reference_cpu(key, NR)
    assert all(torch.equal(a.cpu(), b) for a, b in zip(ref[:4], host[:4])) and all(torch.equal(a.cpu(), b) for a, b in zip(ref[4], host[4]))
    return ref


def test_typed_cut_across_scan_chunks_after_larger_cuts(kg):
    """One KGBatchCut built for 16 nodes (its smallest buffers: 1,024 nodes, 1,024 edges): node and edge buffers grow, and
    each smaller cut follows a larger one whose generation stamps are still in the relabel array."""
    from gnndelete_amd.minibatch import KGBatchCut
    data, info, sampler, _ = kg
    cut = KGBatchCut(data, sampler, sampler.dev, NR, max_nodes=16)       # its own: the shared one may have grown already
    assert cut.n_cap < K.CUT_ORDER[0] and cut.e_cap < 5000
    for key in K.CUT_ORDER:
        nodes = K.node_sets(NR)[key]
        dr_index, dr_type, dec_index, dec_type, rows, _ = _reference(sampler, key)
        cnt = cut.cut(nodes.to(cut.dev))
        e_dr, m_dec = dr_index.shape[1], dec_index.shape[1]
        assert cnt == [nodes.numel(), e_dr, m_dec, rows[0].numel(), rows[1].numel(), 0], key
        assert torch.equal(cut.dr[:2, :e_dr].long(), dr_index) and torch.equal(cut.dr[2, :e_dr].long(), dr_type), key
        assert torch.equal(cut.df_index[:, :m_dec], dec_index) and torch.equal(cut.df_type[:m_dec], dec_type), key
        for k in (0, 1):
            assert torch.equal(cut.rows(k, cnt[3 + k]), rows[k]), (key, k)


def _raw_cut(cut, nodes, cap, generation):
    """gd_induced_subgraph_typed into fresh buffers filled with FILL, each PAD elements longer than the capacity `cap` it is
    called with.  df_index is [2, cap] at pitch cap, its PAD elements follow the second row."""
    from gnndelete_amd import _lib
    from gnndelete_amd._lib import check, ptr, stream_ptr
    dev = cut.dev
    L = _lib.lib()
    n_b = int(nodes.numel())
    i32, i64 = dict(dtype=torch.int32, device=dev), dict(dtype=torch.int64, device=dev)
    out = dict(dr_src=torch.full((cap + PAD,), FILL, **i32), dr_dst=torch.full((cap + PAD,), FILL, **i32),
               dr_type=torch.full((cap + PAD,), FILL, **i32), df_index=torch.full((2 * cap + PAD,), FILL, **i64),
               df_type=torch.full((cap + PAD,), FILL, **i64), rows=torch.full((2 * n_b + PAD,), FILL, **i32),
               counts=torch.full((6,), FILL, **i32))
    ws = torch.empty(max(256, L.gd_induced_subgraph_typed_workspace(n_b)), dtype=torch.uint8, device=dev)
    nodes = nodes.to(dev, torch.int64).contiguous()
    check(L.gd_induced_subgraph_typed(ptr(cut.rowptr32), ptr(cut.col32), ptr(cut.edge_type32), ptr(cut.edge_flags), cut.n, NR,
                                      ptr(nodes), n_b, ptr(cut.node_flags), generation, ptr(cut.relabel), cap, ptr(out['dr_src']),
                                      ptr(out['dr_dst']), ptr(out['dr_type']), ptr(out['df_index']), ptr(out['df_type']),
                                      ptr(out['rows']), ptr(out['counts']), ptr(ws), ws.numel(), stream_ptr(dev)),
          'gd_induced_subgraph_typed')
    return out


def _assert_raw(out, ref, n_b, cap, bad):
    """Every array of a raw cut against the reference, the row lists' and the edge buffers' tails still FILL."""
    dr_index, dr_type, dec_index, dec_type, rows, _ = ref
    e_dr, m_dec = dr_index.shape[1], dec_index.shape[1]
    assert out['counts'].tolist() == [n_b, e_dr, m_dec, rows[0].numel(), rows[1].numel(), bad]
    assert torch.equal(out['dr_src'][:e_dr].long(), dr_index[0]) and torch.equal(out['dr_dst'][:e_dr].long(), dr_index[1])
    assert torch.equal(out['dr_type'][:e_dr].long(), dr_type)
    assert torch.equal(out['df_index'][:m_dec], dec_index[0]) and torch.equal(out['df_index'][cap:cap + m_dec], dec_index[1])
    assert torch.equal(out['df_type'][:m_dec], dec_type)
    for k in (0, 1):
        assert torch.equal(out['rows'][k * n_b:k * n_b + rows[k].numel()], rows[k])
        assert bool((out['rows'][k * n_b + rows[k].numel():(k + 1) * n_b] == FILL).all())
    assert bool((out['rows'][2 * n_b:] == FILL).all())
    for name, used in (('dr_src', e_dr), ('dr_dst', e_dr), ('dr_type', e_dr), ('df_type', m_dec)):
        assert bool((out[name][used:] == FILL).all()), name
    assert bool((out['df_index'][m_dec:cap] == FILL).all()) and bool((out['df_index'][cap + m_dec:] == FILL).all())


@pytest.mark.parametrize('size,bad_row', [(1025, 1024), (2049, 2047)])
@pytest.mark.parametrize('bad_id', ['n + 5', '-1'])
def test_typed_cut_flags_a_bad_node_id_in_a_later_chunk(kg, size, bad_row, bad_id):
    """The bad id sits in the second chunk of the scan (its first row / its last row): the flag is OR-ed over every chunk,
    the bad row is empty and on no list, every other row is the reference's."""
    data, info, sampler, cut = kg
    nodes = K.node_sets(NR)[size].clone()
    nodes[bad_row] = cut.n + 5 if bad_id == 'n + 5' else -1
    good = K.node_sets(NR)[size].to(sampler.dev)
    ref = K.cut_reference_with_bad_row(sampler, good, bad_row, NR)
    full = K.cut_reference(sampler, good, NR)
    cap = max(full[0].shape[1], full[2].shape[1]) + 100      # room for the cut of the good nodes below as well
    assert ref[0].shape[1] < full[0].shape[1]                # the bad row had edges
    cut.generation += 1
    out = _raw_cut(cut, nodes, cap, cut.generation)
    _assert_raw(out, ref, size, cap, bad=1)
    assert not bool((out['dr_src'][:ref[0].shape[1]] == bad_row).any()) and not bool((out['dr_dst'][:ref[0].shape[1]] == bad_row).any())
    with pytest.raises(IndexError):
        cut.cut(nodes)
    # the flag is this call's own: the next cut of good nodes reports 0
    cut.generation += 1
    out = _raw_cut(cut, good, cap, cut.generation)
    _assert_raw(out, full, size, cap, bad=0)


@pytest.mark.parametrize('key,order', [(1025, 'dec <= cap < dr'), ('heavy', 'dr <= cap < dec')])
def test_typed_cut_with_a_capacity_between_the_two_counts_writes_counts_only(kg, key, order):
    """tcut_write_kernel's guard is `Dr edges > cap || decoded triples > cap`: each condition alone, at the smallest
    capacity that trips only it.  Nothing but the count vector (and the row lists) is written, the PAD tail included; the
    re-cut at max(dr, dec) with the same generation gives the reference and leaves the tail alone."""
    data, info, sampler, cut = kg
    nodes = K.node_sets(NR)[key]
    ref = _reference(sampler, key)
    e_dr, m_dec = ref[0].shape[1], ref[2].shape[1]
    cap = min(e_dr, m_dec)
    assert (m_dec <= cap < e_dr) if order == 'dec <= cap < dr' else (e_dr <= cap < m_dec)
    cut.generation += 1
    out = _raw_cut(cut, nodes, cap, cut.generation)
    assert out['counts'].tolist() == [nodes.numel(), e_dr, m_dec, ref[4][0].numel(), ref[4][1].numel(), 0]
    for name in ('dr_src', 'dr_dst', 'dr_type', 'df_index', 'df_type'):
        assert bool((out[name] == FILL).all()), name
    cap = max(e_dr, m_dec)
    out = _raw_cut(cut, nodes, cap, cut.generation)          # the re-cut (same generation)
    _assert_raw(out, ref, nodes.numel(), cap, bad=0)


# ------------------------------------------------------------------------------------------------ gd_batch_typed_csr
def _device_edges(name):
    ei, ty, n, r = K.typed_case(name)
    dev = torch.device('cuda')
    return tuple(v.to(dev, torch.int32).contiguous() for v in (ei[0], ei[1], ty)) + (ei.shape[1], n, r)


def _assert_typed(got, ref, tag, bad=0):
    assert got.status.tolist() == [ref.fwd[2].numel(), ref.bwd[2].numel(), bad, 0], tag
    e = ref.n_edges
    for side in ('fwd', 'bwd'):
        g_, r_ = getattr(got, side), getattr(ref, side)
        s = r_[2].numel()
        assert torch.equal(g_[0].cpu(), r_[0]), (tag, side, 'node_ptr')
        assert torch.equal(g_[1][:s + 1].cpu(), r_[1]), (tag, side, 'seg_ptr')
        assert torch.equal(g_[2][:s].cpu(), r_[2]), (tag, side, 'seg_rel')
        assert torch.equal(g_[3][:e].cpu(), r_[3]), (tag, side, 'col')
        assert torch.equal(g_[4][:e].cpu().view(torch.int32), r_[4].view(torch.int32)), (tag, side, 'w')


@pytest.mark.parametrize('name', K.TYPED_CASES)
def test_batch_typed_csr_matches_the_plain_reference(name):
    from gnndelete_amd.minibatch import batch_typed_csr
    src, dst, et, e, n, r = _device_edges(name)
    bad = 1 if name == 'out_of_range' else 0
    bufs = {}
    got = batch_typed_csr(src, dst, et, e, n, r, bufs)
    _assert_typed(got, K.typed_reference(name), name, bad)
    again = batch_typed_csr(src, dst, et, e, n, r, bufs, into=got)       # the same buffers, the counters of the first call
    assert again is got
    _assert_typed(again, K.typed_reference(name), name + ' (second call)', bad)


def test_batch_typed_csr_reuses_a_larger_workspace_with_stale_counters():
    """2,049 nodes, then 1,023 nodes through the same bufs: the workspace is the larger call's, every counter in it is stale."""
    from gnndelete_amd.minibatch import batch_typed_csr
    bufs = {}
    for name in ('n2049', 'n1023', 'hubs', 'n1025_isolated_last'):
        src, dst, et, e, n, r = _device_edges(name)
        size = bufs['typed_csr'].numel() if bufs else 0
        got = batch_typed_csr(src, dst, et, e, n, r, bufs)
        _assert_typed(got, K.typed_reference(name), name)
        if name == 'n1023':
            assert bufs['typed_csr'].numel() == size            # no new allocation


def _raw_typed_csr(name, edge_cap, seg_cap, pad=PAD):
    """gd_batch_typed_csr into output buffers `pad` longer than the capacities, filled with FILL (w: NaN) -> (return code,
    per side (node_ptr, seg_ptr, seg_rel, col, w), status)."""
    from gnndelete_amd import _lib
    from gnndelete_amd._lib import ptr, stream_ptr
    src, dst, et, e, n, r = _device_edges(name)
    dev = src.device
    L = _lib.lib()
    i32 = dict(dtype=torch.int32, device=dev)
    sides = [(torch.full((n + 1 + pad,), FILL, **i32), torch.full((seg_cap + 1 + pad,), FILL, **i32), torch.full((seg_cap + pad,), FILL, **i32),
              torch.full((edge_cap + pad,), FILL, **i32), torch.full((edge_cap + pad,), float('nan'), dtype=torch.float32, device=dev))
             for _ in range(2)]
    status = torch.full((4,), FILL, **i32)
    ws = torch.empty(max(256, L.gd_batch_typed_csr_workspace(n, e, r)), dtype=torch.uint8, device=dev)
    rc = L.gd_batch_typed_csr(ptr(src), ptr(dst), ptr(et), e, n, r, edge_cap, seg_cap, *(ptr(t) for t in sides[0]),
                              *(ptr(t) for t in sides[1]), ptr(status), ptr(ws), ws.numel(), stream_ptr(dev))
    return rc, sides, status


def test_batch_typed_csr_reports_a_run_capacity_one_short():
    """seg_cap = the forward run count - 1 (both sides of this case have the same count): status[3], the true run counts,
    and no store at or past seg_cap + 1 of seg_ptr / seg_cap of seg_rel; the same call with room gives seg_ptr[runs] = E."""
    from gnndelete_amd._lib import check
    name = 'chunk_start_rel'
    ref = K.typed_reference(name)
    runs = (ref.fwd[2].numel(), ref.bwd[2].numel())
    e = ref.n_edges
    seg_cap = runs[0] - 1
    assert runs[1] > seg_cap and e > 2 * K.SCAN
    rc, sides, status = _raw_typed_csr(name, e, seg_cap)
    check(rc, 'gd_batch_typed_csr')
    assert status.tolist() == [runs[0], runs[1], 0, 1]
    for side, r_ in zip(sides, (ref.fwd, ref.bwd)):
        node_ptr, seg_ptr, seg_rel, col, w = side
        assert bool((seg_ptr[seg_cap + 1:] == FILL).all()) and bool((seg_rel[seg_cap:] == FILL).all())
        assert torch.equal(seg_ptr[:seg_cap].cpu(), r_[1][:seg_cap]) and torch.equal(seg_rel[:seg_cap].cpu(), r_[2][:seg_cap])
        assert torch.equal(col[:e].cpu(), r_[3]) and bool((col[e:] == FILL).all()) and bool(torch.isnan(w[e:]).all())
        assert bool((node_ptr[node_ptr.numel() - PAD:] == FILL).all())
    seg_cap = max(runs)
    rc, sides, status = _raw_typed_csr(name, e, seg_cap)
    check(rc, 'gd_batch_typed_csr')
    assert status.tolist() == [runs[0], runs[1], 0, 0]
    for side, r_, s in zip(sides, (ref.fwd, ref.bwd), runs):
        node_ptr, seg_ptr, seg_rel, col, w = side
        assert int(seg_ptr[s]) == e
        assert torch.equal(node_ptr[:-PAD].cpu(), r_[0]) and torch.equal(seg_ptr[:s + 1].cpu(), r_[1]) and torch.equal(seg_rel[:s].cpu(), r_[2])
        assert torch.equal(col[:e].cpu(), r_[3]) and torch.equal(w[:e].cpu().view(torch.int32), r_[4].view(torch.int32))
        assert bool((seg_ptr[s + 1:] == FILL).all()) and bool((seg_rel[s:] == FILL).all()) and bool((col[e:] == FILL).all())
        assert bool(torch.isnan(w[e:]).all())


def test_batch_typed_csr_refuses_an_edge_capacity_below_the_edge_count():
    """The argument check: a non-zero return that _lib.check raises on, and no launch (nothing written)."""
    from gnndelete_amd._lib import GnnDeleteHipError, check
    name = 'chunk_start_rel'
    e = K.typed_reference(name).n_edges
    rc, sides, status = _raw_typed_csr(name, e - 1, e)
    assert rc != 0
    with pytest.raises(GnnDeleteHipError, match='edge_cap'):
        check(rc, 'gd_batch_typed_csr')
    torch.cuda.synchronize()
    assert status.tolist() == [FILL] * 4
    for side in sides:
        assert all(bool((t == FILL).all()) for t in side[:4]) and bool(torch.isnan(side[4]).all())


def test_batch_typed_csr_workspace_refuses_a_key_that_does_not_fit_int32():
    from gnndelete_amd import _lib
    L = _lib.lib()
    assert L.gd_batch_typed_csr_workspace(2 ** 21, 10, 1024) == -1           # node x relation = 2^31
    assert L.gd_batch_typed_csr_workspace(2 ** 21, 10, 1023) > 0
