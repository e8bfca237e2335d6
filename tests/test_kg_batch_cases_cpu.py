"""The inputs of test_minibatch_kg_chunks_gpu.py and test_minibatch_kg_step_fp64_gpu.py, checked without a GPU: that the cases
of kg_batch_cases.py are the cases - every planted row keeps what it claims, every node set of more than one scan chunk has
list entries and Dr edges on both sides of row 1,024, the laid-out runs sit where the run scan's chunks end - so that a case
which stops reaching a boundary fails here instead of passing vacuously on the GPU; that the plain references agree with the
project's other statements of the same thing; that a chunked scan which forgets its carry cannot reproduce them; and that the
fp32 oracle alone stays two orders of magnitude below the step test's bound.  Figures are printed (pytest -s)."""
import numpy as np
import pytest
import torch

import kg_batch_cases as K

NR = 25
MULTI_CHUNK = [key for key in K.CUT_ORDER if key == 'all' or key > K.SCAN]


def _row(sampler, node):
    """(targets, positions in the input edge list) of a node's CSR row, in row order."""
    lo, hi = int(sampler.rowptr[node]), int(sampler.rowptr[node + 1])
    return sampler.dst_sorted[lo:hi], sampler.order[lo:hi]


def test_planted_rows_are_laid_out_as_described():
    data, info = K.planted_request(NR)
    sampler = K.cpu_sampler(NR)
    src = info['sources']
    inside = torch.zeros(int(data.num_nodes), dtype=torch.bool)
    inside[info['inside']] = True
    dst, pos = _row(sampler, src['skip64'])
    assert dst.numel() == 130 and not bool(inside[dst[:64]].any()) and bool(inside[dst[64:]].all())      # ballot block 1 keeps nothing
    assert bool(data.dr_mask[pos].all())
    dst, pos = _row(sampler, src['full64'])
    assert dst.numel() == K.WAVE and bool(inside[dst].all()) and bool(data.dr_mask[pos].all())
    dst, pos = _row(sampler, src['alt'])
    assert dst.numel() == 100 and bool(inside[dst].all())
    assert data.df_mask[pos].tolist() == [False, True] * 50 and data.dr_mask[pos].tolist() == [True, False] * 50
    assert bool((data.edge_type[pos][1::2] < NR).all())                                                 # every Df entry is decoded
    dst, pos = _row(sampler, src['rev'])
    assert data.df_mask[pos].tolist() == [True, True, False] * 30
    ty = data.edge_type[pos]
    assert bool((ty[0::3] < NR).all()) and bool((ty[1::3] >= NR).all())                                 # decoded, reverse, Dr, ...
    for k in K.KEPT_COUNTS:
        dst, pos = _row(sampler, src[f'k{k}'])
        assert dst.numel() == k + 3 and int(inside[dst].sum()) == k and not bool(inside[dst[:3]].any())
    assert bool((data.dr_mask ^ data.df_mask).all())
    assert max(src.values()) == int(data.num_nodes) - 1 == src['last']


@pytest.mark.parametrize('key', K.SET_SIZES + ('all', 'heavy'))
def test_every_planted_kept_count_is_what_it_claims(key):
    """From RandomWalkSubgraphSampler.subgraph + the trainer's masks on the host."""
    data, info = K.planted_request(NR)
    nodes = K.node_sets(NR)[key]
    assert torch.equal(nodes, nodes.unique()) and nodes.numel() == (key if isinstance(key, int) else nodes.numel())
    dr_index, _, dec_index, _, rows, _ = K.cut_reference_cpu(key, NR)
    n_b = nodes.numel()
    per_dr, per_dec = torch.bincount(dr_index[0], minlength=n_b), torch.bincount(dec_index[0], minlength=n_b)
    for name, node in info['sources'].items():
        r = int((nodes == node).nonzero())
        dr, dec = info['kept'][name]
        if key == 'heavy':                                  # no IN target in the set: the planted rows keep nothing
            dr, dec = 0, 0
        elif key == 'all':                                  # the OUT targets are members too
            dr += {'skip64': 64}.get(name, 3 if name.startswith('k') else 0)
        assert (int(per_dr[r]), int(per_dec[r])) == (dr, dec), (key, name)
    if key != 'heavy':
        got = sorted(int(per_dr[int((nodes == info['sources'][f'k{k}']).nonzero())]) - (3 if key == 'all' else 0) for k in K.KEPT_COUNTS)
        assert got == [63, 64, 65, 127, 128, 129]


@pytest.mark.parametrize('key', MULTI_CHUNK)
def test_sets_of_more_than_one_chunk_use_the_carry_of_every_kind(key):
    nodes = K.node_sets(NR)[key]
    dr_index, _, dec_index, _, rows, _ = K.cut_reference_cpu(key, NR)
    assert nodes.numel() > K.SCAN
    for k in (0, 1):                                        # both row lists: a non-zero carry, and a slot that needs it
        assert int((rows[k] < K.SCAN).sum()) > 0 and int((rows[k] >= K.SCAN).sum()) > 0, (key, k)
    per_dr = torch.bincount(dr_index[0], minlength=nodes.numel())
    assert int(per_dr[K.SCAN - 1]) > 0 and int(per_dr[K.SCAN]) > 0, (key, per_dr[K.SCAN - 1:K.SCAN + 1])
    for idx in (dr_index, dec_index):                       # both edge kinds on both sides of the chunk edge
        assert int((idx[0] < K.SCAN).sum()) > 0 and int((idx[0] >= K.SCAN).sum()) > 0, key
    print(key, 'rows', nodes.numel(), 'Dr', dr_index.shape[1], 'decoded Df', dec_index.shape[1], 'lists', rows[0].numel(), rows[1].numel(),
          'largest row', int(per_dr.max()))


def test_the_df_heavy_set_has_more_decoded_triples_than_dr_edges():
    dr_index, _, dec_index, _, _, m_df = K.cut_reference_cpu('heavy', NR)
    assert dec_index.shape[1] > dr_index.shape[1] > 0 and (dec_index.shape[1], dr_index.shape[1]) == (K.HEAVY_DF, K.HEAVY_DR)
    dr_sampled, dec_sampled = K.cut_reference_cpu(1025, NR)[0].shape[1], K.cut_reference_cpu(1025, NR)[2].shape[1]
    assert 0 < dec_sampled < dr_sampled                     # the other order, for the capacity test


def _chunked_exclusive_scan(v, keep_carry):
    """A scan over chunks of SCAN elements; keep_carry False: every chunk starts from 0 again (the mutation)."""
    out = np.zeros_like(v)
    carry = 0
    for base in range(0, v.size, K.SCAN):
        c = v[base:base + K.SCAN]
        out[base:base + K.SCAN] = carry + np.cumsum(c) - c
        if keep_carry:
            carry += int(c.sum())
    return out


@pytest.mark.parametrize('key', MULTI_CHUNK)
def test_a_cut_scan_without_its_carry_cannot_give_these_cuts(key):
    """tcut_scan_kernel with `carry[k] += chunk` removed, restated on the host for each of its four kinds: the offsets of
    the rows from 1,024 on (and with them every output slot after row 1,023) differ from the reference's."""
    nodes = K.node_sets(NR)[key]
    n_b = nodes.numel()
    dr_index, _, dec_index, _, rows, _ = K.cut_reference_cpu(key, NR)
    kinds = [np.bincount(dr_index[0].numpy(), minlength=n_b), np.bincount(dec_index[0].numpy(), minlength=n_b)]
    for r in rows:
        f = np.zeros(n_b, dtype=np.int64)
        f[r.numpy()] = 1
        kinds.append(f)
    for k, v in enumerate(kinds):
        want = np.cumsum(v) - v
        assert np.array_equal(_chunked_exclusive_scan(v, True), want)
        wrong = _chunked_exclusive_scan(v, False)
        used = v[K.SCAN:] > 0                               # rows that write at their offset
        assert (wrong[K.SCAN:][used] != want[K.SCAN:][used]).all() and used.any(), (key, k)


@pytest.mark.parametrize('name', K.TYPED_CASES)
def test_typed_csr_reference_equals_typed_node_csr(name):
    from gnndelete_amd.graph import TypedNodeCSR
    ei, ty, n, r = K.typed_case(name)
    ref = K.typed_reference(name)
    ok = ((ei >= 0) & (ei < n)).all(0) & (ty >= 0) & (ty < r)
    assert int((~ok).sum()) == (40 if name == 'out_of_range' else 0) and ref.n_edges == int(ok.sum())
    other = TypedNodeCSR(ei[:, ok], ty[ok], n, r)
    for side in ('fwd', 'bwd'):
        a, b = getattr(ref, side), getattr(other, side)
        for k, what in enumerate(('node_ptr', 'seg_ptr', 'seg_rel', 'col')):
            assert a[k].dtype == torch.int32 and torch.equal(a[k], b[k].cpu()), (name, side, what)
        assert a[4].dtype == torch.float32 and torch.equal(a[4].view(torch.int32), b[4].cpu().view(torch.int32)), (name, side, 'w')


def test_typed_cases_have_the_shapes_they_are_built_for():
    for name, n in (('n1023', 1023), ('n1024', 1024), ('n1025', 1025), ('n2049', 2049), ('n2049_gap', 2049), ('n1025_isolated_last', 1025)):
        ei, ty, n_, r = K.typed_case(name)
        assert (n_, r) == (n, 12) and abs(ei.shape[1] - 5 * n) < 40
    ref = K.typed_reference('n2049_gap')
    assert int(ref.fwd[0][K.SCAN - 1]) == int(ref.fwd[0][K.SCAN]) == int(ref.fwd[0][K.SCAN + 1])      # no in-edge: equal run offsets
    assert int(ref.bwd[0][K.SCAN - 1]) < int(ref.bwd[0][K.SCAN]) < int(ref.bwd[0][K.SCAN + 1])        # (but out-edges)
    ref = K.typed_reference('n1025_isolated_last')
    assert int(ref.fwd[0][1024]) == int(ref.fwd[0][1025]) and int(ref.bwd[0][1024]) == int(ref.bwd[0][1025])
    ei, ty, n, r = K.typed_case('hubs')
    indeg, outdeg = torch.bincount(ei[1], minlength=n), torch.bincount(ei[0], minlength=n)
    for node, m in K.HUB_IN.items():
        assert m <= int(indeg[node]) <= m + 20              # (+ the background edges that happen to end there)
    assert K.HUB_OUT[1] <= int(outdeg[K.HUB_OUT[0]]) <= K.HUB_OUT[1] + 20
    key = (ei[1] * n + ei[0]) * r + ty                      # parallel edges with equal (relation, other endpoint): the tie-break
    assert int((torch.bincount(key[ei[1] == 77]).max())) >= 3
    assert int((torch.bincount(key[ei[0] == K.HUB_OUT[0]]).max())) >= 3
    ei, ty, n, r = K.typed_case('out_of_range')
    assert int((ei[0] == n).sum()) == 10 and int((ei[1] == -1).sum()) == 10 and int((ty == r).sum()) == 10 and int((ty == -1).sum()) == 10
    ok = ((ei >= 0) & (ei < n)).all(0) & (ty >= 0) & (ty < r)
    assert int(ok.sum()) == 5000 and not bool(ok[0]) and not bool(ok[-1])          # the first and the last edge are bad ones


@pytest.mark.parametrize('name', K.CHUNK_EDGE_CASES)
def test_chunk_edge_cases_sit_on_the_run_scans_chunk_edges(name):
    """From the reference's seg_ptr, on both sides.  A run cannot start at a position and straddle it, so the case is three
    edge lists: two with 1024 and 2048 as run starts, one with a run across each."""
    ref = K.typed_reference(name)
    for side in ('fwd', 'bwd'):
        node_ptr, seg_ptr, seg_rel, _, _ = (t.long() for t in getattr(ref, side))
        assert int(seg_ptr[-1]) > 2 * K.SCAN + 200
        node_of_run = torch.repeat_interleave(torch.arange(node_ptr.numel() - 1), node_ptr[1:] - node_ptr[:-1])
        for edge in (K.SCAN, 2 * K.SCAN):
            member = bool((seg_ptr == edge).any())
            straddling = ((seg_ptr[:-1] < edge) & (edge < seg_ptr[1:])).nonzero().flatten()
            if name == 'chunk_straddle':
                assert not member and straddling.numel() == 1
                i = int(straddling)
                assert int(seg_ptr[i + 1] - seg_ptr[i]) == 70 and int(seg_ptr[i]) == (1000 if edge == K.SCAN else 2030), (name, side)
            else:
                assert member and straddling.numel() == 0
                i = int((seg_ptr == edge).nonzero())
                same_node = int(node_of_run[i - 1]) == int(node_of_run[i])
                assert same_node == (name == 'chunk_start_rel'), (name, side, edge)
                if same_node:
                    assert int(seg_rel[i - 1]) != int(seg_rel[i])


def _run_scan(nkey, across, keep_carry=True):
    """tcsr_run_scan_kernel's run ids on the host.  across: what the first element of a chunk after the first does -
    'read' nkey[p - 1] (the kernel), or take itself for a run 'start' / for 'no-start' without looking."""
    p = np.arange(nkey.size)
    v = np.ones(nkey.size, dtype=np.int64)
    v[1:] = nkey[1:] != nkey[:-1]
    first = (p % K.SCAN == 0) & (p > 0)
    if across != 'read':
        v[first] = 1 if across == 'start' else 0
    return _chunked_exclusive_scan(v, keep_carry) + v - 1


@pytest.mark.parametrize('name', K.TYPED_CASES)
def test_csr_scans_without_carry_or_cross_chunk_read_cannot_give_these_cases(name):
    """The node scan and the run scan of gd_batch_typed_csr restated on the host.  Without the carry every case of more than
    one chunk differs; a run scan that does not read across the chunk edge differs on a straddling run when it assumes a
    start, and on a run that starts there when it assumes none."""
    ref = K.typed_reference(name)
    _, _, n, r = K.typed_case(name)
    for side in ('fwd', 'bwd'):
        node_ptr, seg_ptr, seg_rel, _, _ = (t.long().numpy() for t in getattr(ref, side))
        lens = np.diff(seg_ptr)
        run_of_edge = np.repeat(np.arange(lens.size), lens)
        node_of_run = np.repeat(np.arange(n), np.diff(node_ptr))
        nkey = (node_of_run * r + seg_rel)[run_of_edge]
        assert nkey.size > K.SCAN
        assert np.array_equal(_run_scan(nkey, 'read'), run_of_edge)
        assert not np.array_equal(_run_scan(nkey, 'read', keep_carry=False), run_of_edge)
        if name in K.CHUNK_EDGE_CASES:
            wrong = 'start' if name == 'chunk_straddle' else 'no-start'
            assert not np.array_equal(_run_scan(nkey, wrong)[:2 * K.SCAN + 1], run_of_edge[:2 * K.SCAN + 1]), (name, side)
        deg = np.zeros(n, dtype=np.int64)                   # edges per node -> the node scan's offsets
        np.add.at(deg, node_of_run, lens)
        want = np.cumsum(deg) - deg
        assert np.array_equal(_chunked_exclusive_scan(deg, True), want)
        if n > K.SCAN:
            assert not np.array_equal(_chunked_exclusive_scan(deg, False), want), (name, side)


@pytest.mark.parametrize('key', (1025, 2049, 'heavy'))
def test_cut_reference_equals_saint_subgraph_and_the_same_masks(key):
    """The trainer-masking reference (on the project's sampler) against oracle.pyg_semantics.saint_subgraph + the masking of
    oracle.gnndelete_ref.kg_nodeemb_minibatch."""
    from oracle import pyg_semantics as pyg
    data, _ = K.planted_request(NR)
    nodes = K.node_sets(NR)[key]
    b = pyg.saint_subgraph({k: v for k, v in data.items()}, nodes)
    ei, et = b['edge_index'][:, b['dr_mask']], b['edge_type'][b['dr_mask']]
    pos, pt = b['edge_index'][:, b['df_mask']], b['edge_type'][b['df_mask']]
    fw = pt < NR
    dr_index, dr_type, dec_index, dec_type, rows, m_df = K.cut_reference_cpu(key, NR)
    assert torch.equal(dr_index, ei) and torch.equal(dr_type, et) and torch.equal(dec_index, pos[:, fw]) and torch.equal(dec_type, pt[fw])
    assert m_df == pos.shape[1]
    for r, m in zip(rows, (b['sdf_node_1hop_mask_non_df_mask'], b['sdf_node_2hop_mask_non_df_mask'])):
        assert torch.equal(r.long(), m.nonzero().flatten())


def test_cut_reference_with_a_bad_row_keeps_every_other_row_number():
    nodes = K.node_sets(NR)[1025]
    sampler = K.cpu_sampler(NR)
    full = K.cut_reference_cpu(1025, NR)
    for bad_row in (K.SCAN, 17):
        got = K.cut_reference_with_bad_row(sampler, nodes, bad_row, NR)
        src_kept = full[0][0] != bad_row
        both = src_kept & (full[0][1] != bad_row)          # the bad row is gone as a source and as a target
        assert torch.equal(got[0], full[0][:, both]) and torch.equal(got[1], full[1][both])
        for r_got, r_full in zip(got[4], full[4]):
            assert torch.equal(r_got, r_full[r_full != bad_row])


@pytest.mark.parametrize('config', sorted(K.STEP_CONFIGS))
def test_fp32_oracle_alone_sits_far_below_the_step_bound(config):
    """The step test's bound is max(2 x the fp32 ensemble's distance to fp64, 5e-5) under a ceiling of 1e-4: here the ensemble
    alone, from the initial Del weights, on all seven compared quantities of every batch - below 5e-5, so the floor is the
    bound and it does not depend on what a GPU computes.  Also the batches' shapes."""
    torch.set_num_threads(min(16, torch.get_num_threads()))
    data, nr, dims, state, batches = K.step_request(config)
    assert [b[0] for b in batches] == list(K.STEP_LABELS)
    w1, w2 = state['deletion1.deletion_weight'], state['deletion2.deletion_weight']
    assert (nr > 20) == (config == 'blocks-25')
    for label, nodes, dec, dec_t, neg in batches:
        want = K.step_batch_reference(config, w1, w2, nodes, neg, torch.float64)
        n_b, e_dr, m_dec, n_l1, n_l2 = want['counts']
        assert neg.shape == dec.shape == (2, m_dec) and torch.equal(nodes, nodes.unique())
        if label.startswith('sampled'):
            assert n_b > K.SCAN and e_dr > 20000 and m_dec > 0 and n_l1 > 0 and n_l2 > 0
        if label == '1025 nodes':
            assert n_b == K.SCAN + 1
        if label == '2049 nodes':
            assert n_b == 2 * K.SCAN + 1
        if label == 'no decoded Df triple':
            assert m_dec == 0 and n_l1 > 0 and want['sums'][0] == 0.0 and want['sums'][2] == 0.0
        if label == 'no list-1 row':
            assert n_l1 == 0 and m_dec > 0 and want['sums'][1] == 0.0
        worst = {}
        for perm in K.STEP_PERMS:
            for name, v in K.step_distances(K.step_batch_reference(config, w1, w2, nodes, neg, torch.float32, perm), want).items():
                worst[name] = max(worst.get(name, 0.0), v)
        print(f'[{config}, {label}: {n_b} nodes, {e_dr} Dr edges, {m_dec} decoded] fp32 ensemble to fp64: '
              + ', '.join(f'{k} {v:.1e}' for k, v in worst.items()))
        for gkey, _ in K.STEP_QUANTITIES:
            assert bool(torch.isfinite(want[gkey]).all())
        assert len(worst) == 7 - sum(1 for s_ in want['sums'].tolist() if s_ == 0.0)
        assert max(worst.values()) < 5e-5, (label, worst)
