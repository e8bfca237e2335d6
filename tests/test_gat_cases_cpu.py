"""The inputs of test_gat_kernels_gpu.py, checked without a GPU: that the graphs have the degrees, pieces, groups and visits
they are built for, that every logit regime is what its name says, and that the fp32 restatement ALONE sits inside every bound
the GPU tests hold the kernels to - so a kernel that misses a bound is wrong, not merely fp32.  Every figure is printed
(pytest -s)."""
import pytest
import torch

import gat_cases as C

LIMIT = 1e-4 / C.SOFTMAX_FACTOR          # restatement below this: every bound is under 1e-4, a wrong rescale is 1e-2 ... 1


def test_hub_graph_has_the_listed_degrees_multi_edges_loops_and_isolated_rows():
    from oracle import pyg_semantics as pyg
    gph, lay = C.graph('hub'), C.layout('hub')
    n, gr = gph.n, lay.gr
    assert n == 6000 and gr.rowptr.dtype == torch.int32 and gr.col.dtype == torch.int32
    assert sorted(C.HUB_IN.values()) == [1, 2, 63, 64, 65, 128, 129, 256, 257, 320, 1000, 5000]
    assert sorted(C.HUB_OUT.values()) == [256, 257, 300, 1000]
    for v, k in C.HUB_IN.items():
        assert int(lay.deg[v]) == k, (v, k)
    for v, k in C.HUB_OUT.items():
        assert int(lay.out_deg[v]) == k, (v, k)
    assert gr.nnz == pyg.with_single_self_loops(gph.ei, n).shape[1]                  # loops dropped, one appended per node
    assert int((gph.ei[0] == gph.ei[1]).sum()) >= len(C.EXPLICIT_LOOPS)
    assert int(((lay.rows == lay.col).long()).sum()) == n                             # exactly one loop per node
    key = gph.ei[1] * n + gph.ei[0]
    assert gph.ei.shape[1] - int(key.unique().numel()) >= 50 + 3 * 10                 # multi-edges: background, hubs
    for hub in (1200, 1000, 300):                                                     # a multi-edge inside hub rows
        c = lay.col[int(gr.rowptr[hub]):int(gr.rowptr[hub + 1])]
        assert int(c.numel() - c.unique().numel()) == 3
    iso = slice(n - C.SPEC['hub']['isolated'], n)
    assert bool((lay.deg[iso] == 1).all()) and bool((lay.out_deg[iso] == 1).all())   # the loop alone
    assert int(lay.deg.min()) == 1                                                    # 'gat' graphs have no empty row
    light = torch.ones(n, dtype=torch.bool)
    light[list(C.HUB_IN)] = False
    assert int(lay.deg[light].max()) <= 16 and gr.nnz < 24000                         # a thin background: fp64 at d = 1,024
    # the transposed layout: rows above 256 out-edges are redone by the whole wave in gat_transpose_edge_kernel
    assert int((lay.out_deg > 256).sum()) == 3 and int((lay.out_deg == 256).sum()) == 1


def test_hub_graph_pieces_and_groups():
    from gnndelete_amd.graph import SplitPlan
    lay = C.layout('hub')
    plan = SplitPlan(lay.gr.rowptr)
    pieces = {int(r): int(k) for r, _, k, _ in plan.split.tolist()}
    assert pieces[1200] == 79 and pieces[1100] == 16 and pieces[1000] == 5 and pieces[500] == 2 and 400 not in pieces
    assert max(pieces.values()) > 64                                                  # the fix-up's serial branch
    for d in C.WIDTHS:
        # more pieces than lanes that carry features in the fix-up (d / 4 of them, all 64 from d = 256 on)
        assert any(k > min(d // 4, 64) for k in pieces.values()), d
    assert pieces[1100] > 32 // 4 and pieces[1100] <= 64                              # ... on the one-lane-per-piece branch too
    for d in C.WIDTHS:
        items, n_items, b = plan.onepass(d, multirow=1)
        assert n_items % 4 == 0 and all(int(x) % 4 == 0 for x in b)
        member = items[items[:, 3] == -2]
        rows = member[:, 0].unique().tolist()
        assert sorted(rows) == sorted(pieces)                                         # every split row is a group
        assert any(pieces[r] <= 4 for r in rows) and any(pieces[r] > 4 for r in rows)
        share = (member[:, 2] - member[:, 1])
        assert int(share.max()) > 256 and int(share[member[:, 0] == 1000].max()) == 128   # members that walk several chunks
        assert int(share[member[:, 0] == 900].max()) == 128 and int(share[member[:, 0] == 800].max()) == 64
        first = (items[:, 3] == -2).nonzero().flatten()[::4]
        assert bool((first % 4 == 0).all())


@pytest.mark.parametrize('name,most', [('visit36k', 2), ('visit70k', 3)])
def test_visit_graphs_reach_second_and_third_visits(name, most):
    lay = C.layout(name)
    plan = lay.gr.plan
    for v, k in C.SPEC[name]['hub_in'].items():
        assert int(lay.deg[v]) == k
    assert sorted(set(C.SPEC[name]['hub_in'].values())) == [65, 320, 1000]
    assert float((lay.deg <= 8).float().mean()) > 0.99                                # mostly light rows
    if most == 2:
        assert 32768 < plan.n_items < 65536
    else:
        assert plan.n_items > 65536
    hubs = list(C.SPEC[name]['hub_in'])
    for form, d in [('pieces', 64)] + [('onepass', d) for d in C.VISIT_WIDTHS]:
        rows, visit = C.item_tables(name, form, d)
        counts = torch.bincount(visit).tolist()
        print(f'[{name} {form} d = {d}] items {rows.numel()}  served on visit 1 / 2 / 3: {counts}  '
              + '  '.join(f'hub {h}: {sorted(set(visit[rows == h].tolist()))}' for h in hubs))
        assert len(counts) == most and min(counts) > 0                                # waves with 1, 2 (and 3) visits
        # a wave makes as many visits as the last item it serves: the same wave slot, with and without a later visit
        assert counts[0] == 32768 and counts[-1] < 32768
        later = C.later_visit_rows(name, form, d)
        hub_later = [h for h in hubs if h in set(later.tolist())]
        if form == 'pieces':
            assert hub_later == hubs                                                  # every hub's pieces: a second or later visit
            if most == 3:
                assert int(visit[rows == hubs[0]].min()) == 1 and int(visit[rows == hubs[-1]].min()) == 2
        else:
            # the one-launch items put rows above four pieces first in their range; the 65-edge groups stay in row order
            assert [h for h in hub_later if C.SPEC[name]['hub_in'][h] == 65], hub_later
            assert int(visit[(rows == hubs[-1])].min()) == most - 1
        assert 300 < later.numel() < plan.n_items - 32768 + 1


@pytest.mark.parametrize('name', list(C.SPEC))
def test_logit_regimes_are_what_they_are_named(name):
    lay = C.layout(name)
    rows, col, gr = lay.rows, lay.col, lay.gr
    base = C.logits(name, 'randn')
    for regime in C.REGIMES:
        a_src, a_dst = C.logits(name, regime)
        assert a_src.dtype == a_dst.dtype == torch.float32
        for t in (a_src, a_dst):
            assert torch.equal(torch.round(t * C.GRID) / C.GRID, t)                   # on the grid
        s32 = a_src[col] + a_dst[rows]
        s64 = a_src.double()[col] + a_dst.double()[rows]
        assert torch.equal(s32.double(), s64)                                         # every sum is exact in fp32
        if regime == 'zero':
            assert bool((s32 == 0.0).all()) and float(a_src[0]) == 7.25 and float(a_dst[0]) == -7.25
        if regime == 'negative':
            assert float(s32.max()) < -580
            assert float(torch.exp(torch.nn.functional.leaky_relu(s32, C.SLOPE)).max()) == 0.0    # exp without the max: 0
        if regime == 'wide':
            assert float(s64.max() - s64.min()) > 200 and torch.equal(a_src, base[0] * 40)
            big = max(C.SPEC[name]['hub_in'], key=C.SPEC[name]['hub_in'].get)
            e = torch.nn.functional.leaky_relu(s64[int(gr.rowptr[big]):int(gr.rowptr[big + 1])], C.SLOPE)
            assert float(s64[int(gr.rowptr[big]):int(gr.rowptr[big + 1])].max() - s64[int(gr.rowptr[big]):int(gr.rowptr[big + 1])].min()) > 200
            assert bool(torch.isinf(torch.exp(e.max().float()))) and float((torch.exp((e - e.max()).float()) == 0).float().mean()) > 0.5
        if regime.startswith('dominant'):
            which = regime.split('_')[1]
            raised = (a_src != base[0]).nonzero().flatten().tolist()
            assert torch.equal(a_dst, base[1]) and len(raised) == len(C.dominated_hubs(name))
            for hub in C.dominated_hubs(name):
                lo, hi = int(gr.rowptr[hub]), int(gr.rowptr[hub + 1])
                k = C.edge_slot(name, hub, which)
                src = int(col[k])
                assert src == (C.graph(name).tail if which == 'tail' else C.graph(name).head)[hub] and src in raised
                assert float(a_src[src] - base[0][src]) == 60.0 and int(lay.out_deg[src]) == 2      # this edge and its loop
                assert k == (hi - 1 if which == 'tail' else lo)
                piece = (k - lo) // 64
                assert piece == ((hi - lo - 1) // 64 if which == 'tail' else 0)       # the last / first piece (and group member)
                seg = s64[lo:hi]
                assert int(seg.argmax()) == k - lo and float(seg[k - lo] - seg[torch.arange(hi - lo) != k - lo].max()) > 50


@pytest.mark.parametrize('regime', C.REGIMES)
@pytest.mark.parametrize('d', [8, 64])
def test_fp32_restatement_is_inside_the_gpu_bounds(d, regime):
    """The restatement is finite, its error is above zero and below 1e-4 / 8 for every quantity: each bound max(8 x it,
    2^-22) is under 1e-4 - the slot-wise score gradient included: the features carry one sign per column (gat_cases.case), so
    no dot product <dy, h> cancels inside itself and its magnitude is the sum of the magnitudes behind it."""
    c = C.case('hub', d)
    assert bool((c['dy'][:50, None, :] * c['h'][None, :50, :] >= 0).all())
    assert 0 < int((c['h'][0] > 0).sum()) < d and torch.equal(c['h'][0] > 0, c['dy'][7] > 0)          # both signs, shared per column
    ref = C.reference('hub', regime, d)
    for k in ('y', 'rowmax', 'rowsum', 'alpha', 'de', 'dh', 'da_src', 'da_dst'):
        assert bool(torch.isfinite(ref[k]).all()), k
    r = C.restatement_errors('hub', regime, d)
    b = C.bounds('hub', regime, d)
    print(f'[hub graph {regime:13s} d = {d:3d}] fp32 restatement: ' + '  '.join(f'{k} {v:.2e}' for k, v in r.items() if k != 'finite'))
    assert r['finite']
    for k in ('y', 'y_bias', 'dh', 'dh_full', 'da_src', 'da_dst', 'alpha', 'de', 'rowsum'):
        assert r[k] < LIMIT and b[k] < 1e-4, (k, r[k])
    for k in ('y', 'y_bias', 'dh', 'dh_full', 'da_src', 'da_dst', 'alpha', 'de'):
        assert r[k] > 0, k
    assert r['rowmax'] <= 0.5
    assert float(ref['rowsum'].min()) >= 1.0 and bool((ref['rowsum'] <= C.layout('hub').deg + 1e-9).all())
    if regime == 'zero':
        deg = C.layout('hub').deg.double()
        assert torch.equal(ref['rowsum'], deg) and float((ref['alpha'] - 1 / deg[C.layout('hub').rows]).abs().max()) < 1e-15
        # leaky' at 0 is the slope (torch's convention): sum_j de_ij = slope * sum_j alpha (p - t) = 0 exactly only through it
        p = (C.case('hub', d)['dy'].double()[C.layout('hub').rows] * C.case('hub', d)['h'].double()[C.layout('hub').col]).sum(1)
        t = torch.zeros(6000, dtype=torch.float64).index_add(0, C.layout('hub').rows, ref['alpha'] * p)
        want = C.SLOPE * ref['alpha'] * (p - t[C.layout('hub').rows])
        assert float((ref['de'] - want).abs().max()) <= 1e-12 * float(want.abs().max())


def test_row_subset_and_range_cut_through_the_hubs():
    rows = C.row_subset('hub')
    inside = set(rows.tolist())
    assert {1200, 1000, 900, 400} <= inside and not ({100, 200, 300, 500, 600, 700, 800, 1100} & inside)
    assert {1400, 1600} <= inside and not ({1300, 1500} & inside) and 1800 < len(inside) < 2200 and bool((rows[1:] > rows[:-1]).all())
    lo, hi = C.SUBSET_RANGE
    assert lo == 400 and hi - 1 == 1000 and 300 < lo and hi <= 1100
    # the subset reference: an upstream gradient that is zero outside the rows = what a plan over them computes
    ref, full = C.reference('hub', 'randn', 16, True), C.reference('hub', 'randn', 16)
    out_rows = torch.ones(6000, dtype=torch.bool)
    out_rows[rows] = False
    edge_out = out_rows[C.layout('hub').rows]
    assert float(ref['de'][edge_out].abs().max()) == 0.0 and torch.equal(ref['de'][~edge_out], full['de'][~edge_out])
    assert torch.equal(ref['da_dst'][rows], full['da_dst'][rows]) and float(ref['da_dst'][out_rows].abs().max()) == 0.0
    assert not torch.equal(ref['dh'], full['dh'])
