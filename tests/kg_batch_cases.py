"""Shared inputs and plain references of the knowledge-graph batch-step tests past one 1,024-row scan chunk
(test_kg_batch_cases_cpu.py, test_minibatch_kg_chunks_gpu.py, test_minibatch_kg_step_fp64_gpu.py).

The integer kernels of the step (csrc/subgraph_typed.hip) scan batch rows, batch nodes and sorted edges in one block that
walks chunks of SCAN = 1,024 elements and carries totals from chunk to chunk.  Everything here exists to put something on
both sides of such a chunk edge, and is deterministic from seeds:

  1. kg_request: the synthetic knowledge-graph request (4,000 nodes, 5 % IN deletion) the step test runs on;
  2. planted_request: that graph plus FRESH nodes whose rows are built for the cut's ballot blocks (64 lanes) and slot
     counters, and node sets of 1023 .. 3001 rows, all nodes, and a region with more decoded Df triples than Dr edges;
  3. cut_reference: RandomWalkSubgraphSampler.subgraph + KGGNNDeleteNodeembTrainer's masking (what gd_induced_subgraph_typed
     is held to), cut_reference_with_bad_row for a node list with one id out of range;
  4. typed_csr_reference: gd_batch_typed_csr restated with np.lexsort (independent of graph.TypedNodeCSR), and the typed-CSR
     cases: node counts around the chunk, runs laid out around sorted positions 1024 and 2048 on both sides, hubs with
     parallel edges, edges out of range;
  5. the step test's model, batches, recorded negatives and the float64 / fp32-ensemble batch oracle.

References are computed once per process (lru_cache) and must be left unchanged by their users."""
import functools
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn as nn

SCAN = 1024                     # kTScanThreads: rows / nodes / sorted edges per chunk of the single-block scans
WAVE = 64                       # lanes of a ballot block of the cut's count and write kernels


# ---------------------------------------------------------------------------------------------------------------------
# 1. the request
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def kg_request(n=4000, nr=25, m=60000, seed=42):
    """tools/experiments/minibatch_kg_fused.py::setup on a graph of another shape: -> Data (CPU) with edge_index / edge_type
    (every triple and its reverse, type + nr), dr_mask / df_mask and the S_Df-minus-Df node masks."""
    from gnndelete_amd.framework.data import prepare_edge_deletion, resolve_df_size
    from gnndelete_amd.framework.synth import make_kg_dataset
    from gnndelete_amd.framework.trainer.gnndelete_nodeemb import _non_df_masks
    state = torch.get_rng_state()
    data, df = make_kg_dataset(None, seed, shape=(n, nr, m))
    # (setup's seed_everything(seed), for what prepare_edge_deletion draws from: the host generator alone, put back afterwards -
    # a test that runs later in the same process finds the random streams it would have found without this module)
    torch.default_generator.manual_seed(seed)
    prepare_edge_deletion(data, df['in'], resolve_df_size(5.0, data.train_pos_edge_index.shape[1]), True, nr)
    _non_df_masks(data)
    torch.set_rng_state(state)
    return data


# ---------------------------------------------------------------------------------------------------------------------
# 2. planted rows and node sets
# ---------------------------------------------------------------------------------------------------------------------
KEPT_COUNTS = (63, 64, 65, 127, 128, 129)      # kept Dr edges of a planted source: around one and two ballot blocks
N_OUT, N_IN, N_HEAVY = 70, 140, 40             # fresh targets left out of / put into every node set; the Df-heavy region
HEAVY_DF, HEAVY_DR = 300, 60
SET_SIZES = (1023, 1024, 1025, 2048, 2049, 3001)
CUT_ORDER = (3001, 1025, 'all', 1023, 1024, 2048, 2049)      # larger cuts before smaller ones: stale generation stamps


@functools.lru_cache(maxsize=None)
def planted_request(nr=25):
    """-> (Data, info).  The graph of kg_request(nr=nr) with fresh node ids appended, in this id order (a CSR row is sorted
    by target id, so the OUT targets come first in every planted row):

      out      N_OUT targets that no node set but 'all' holds
      in       N_IN targets that every sized set holds
      heavy    N_HEAVY nodes with HEAVY_DF decoded Df triples and HEAVY_DR Dr edges among themselves
      sources  one planted row each (info['sources'][name] = node id); every node set holds them all, and they are its last
               rows.  Kept entries in a sized set (info['kept'][name] = (Dr edges, decoded Df triples)):
        k63 .. k129   3 Dr edges to OUT, then K Dr edges to IN: K kept, for K in KEPT_COUNTS
        skip64        130 entries: 64 to OUT, then 66 to IN - kept only from the second and third ballot block
        full64        exactly 64 entries, all to IN, all kept
        alt           100 entries to IN, Dr and decoded Df alternating: the two slot counters diverge
        rev           90 entries to IN in the pattern decoded Df, REVERSE-type Df (not decoded), Dr
        last          129 Dr entries to IN and 5 decoded Df; carries both node flags (a set's last row is on both lists)"""
    d0 = kg_request(nr=nr)
    g = torch.Generator().manual_seed(977)
    n0 = int(d0.num_nodes)
    out_t = torch.arange(n0, n0 + N_OUT)
    in_t = torch.arange(n0 + N_OUT, n0 + N_OUT + N_IN)
    heavy = torch.arange(int(in_t[-1]) + 1, int(in_t[-1]) + 1 + N_HEAVY)
    names = [f'k{k}' for k in KEPT_COUNTS] + ['skip64', 'full64', 'alt', 'rev', 'last']
    first = int(heavy[-1]) + 1
    sources = {name: first + i for i, name in enumerate(names)}
    n = first + len(names)
    rows = []                                               # (src, dst, type, is_df)

    def add(src, dst, ty, df):
        dst = torch.as_tensor(dst)
        m = dst.numel()
        src = torch.as_tensor(src).expand(m) if torch.as_tensor(src).dim() == 0 else torch.as_tensor(src)
        rows.append((src, dst, torch.as_tensor(ty).expand(m) if torch.as_tensor(ty).dim() == 0 else torch.as_tensor(ty),
                     torch.as_tensor(df).expand(m) if torch.as_tensor(df).dim() == 0 else torch.as_tensor(df)))

    any_type = lambda m: torch.randint(0, 2 * nr, (m,), generator=g)
    fwd_type = lambda m: torch.randint(0, nr, (m,), generator=g)
    rev_type = lambda m: torch.randint(nr, 2 * nr, (m,), generator=g)
    kept = {}
    for k in KEPT_COUNTS:
        s = sources[f'k{k}']
        add(s, out_t[:3], any_type(3), False)
        add(s, in_t[:k], any_type(k), False)
        kept[f'k{k}'] = (k, 0)
    add(sources['skip64'], out_t[:64], any_type(64), False)
    add(sources['skip64'], in_t[:66], any_type(66), False)
    kept['skip64'] = (66, 0)
    add(sources['full64'], in_t[:64], any_type(64), False)
    kept['full64'] = (64, 0)
    alt_df = torch.arange(100) % 2 == 1
    add(sources['alt'], in_t[:100], torch.where(alt_df, fwd_type(100), any_type(100)), alt_df)
    kept['alt'] = (50, 50)
    phase = torch.arange(90) % 3
    add(sources['rev'], in_t[:90], torch.where(phase == 0, fwd_type(90), torch.where(phase == 1, rev_type(90), any_type(90))),
        phase < 2)
    kept['rev'] = (30, 30)
    add(sources['last'], in_t[:129], any_type(129), False)
    add(sources['last'], in_t[129:134], fwd_type(5), True)
    kept['last'] = (129, 5)
    hd = heavy[torch.randint(0, N_HEAVY, (2, HEAVY_DF + HEAVY_DR), generator=g)]
    add(hd[0, :HEAVY_DF], hd[1, :HEAVY_DF], fwd_type(HEAVY_DF), torch.ones(HEAVY_DF, dtype=torch.bool))
    add(hd[0, HEAVY_DF:], hd[1, HEAVY_DF:], any_type(HEAVY_DR), torch.zeros(HEAVY_DR, dtype=torch.bool))
    src, dst, ty, df = (torch.cat([r[i] for r in rows]) for i in range(4))
    p = torch.randperm(src.numel(), generator=g)            # the input order of the planted edges is not their row order
    src, dst, ty, df = src[p], dst[p], ty[p], df[p]
    from gnndelete_amd.framework.data import Data
    fresh = n - n0
    flag = lambda base, seed_: torch.cat([base, torch.rand(fresh, generator=torch.Generator().manual_seed(seed_)) < 0.5])
    m1, m2 = flag(d0.sdf_node_1hop_mask_non_df_mask, 1), flag(d0.sdf_node_2hop_mask_non_df_mask, 2)
    m1[sources['last']] = m2[sources['last']] = True
    data = Data(num_nodes=n, x=torch.arange(n), edge_index=torch.cat([d0.edge_index, torch.stack([src, dst])], 1).contiguous(),
                edge_type=torch.cat([d0.edge_type, ty]).contiguous(), dr_mask=torch.cat([d0.dr_mask, ~df]),
                df_mask=torch.cat([d0.df_mask, df]))
    data.sdf_node_1hop_mask_non_df_mask, data.sdf_node_2hop_mask_non_df_mask = m1, m2
    info = dict(n_base=n0, out=out_t, inside=in_t, heavy=heavy, sources=sources, kept=kept, num_edge_type=nr)
    return data, info


@functools.lru_cache(maxsize=None)
def node_sets(nr=25):
    """{size | 'all' | 'heavy': sorted unique node ids}.  A sized set = the planted sources, the IN targets and base nodes
    drawn without replacement up to the size; 'heavy' = the Df-heavy region and the sources (no IN target: the planted rows
    keep nothing there)."""
    data, info = planted_request(nr)
    src = torch.tensor(sorted(info['sources'].values()))
    core = torch.cat([info['inside'], src])
    sets = {}
    for size in SET_SIZES:
        g = torch.Generator().manual_seed(5000 + size)
        base = torch.randperm(info['n_base'], generator=g)[:size - core.numel()]
        sets[size] = torch.cat([base, core]).sort().values
        assert sets[size].numel() == size
    sets['all'] = torch.arange(int(data.num_nodes))
    sets['heavy'] = torch.cat([info['heavy'], src]).sort().values
    return sets


@functools.lru_cache(maxsize=None)
def cpu_sampler(nr=25):
    from gnndelete_amd.framework.trainer.sampler import RandomWalkSubgraphSampler
    return RandomWalkSubgraphSampler(planted_request(nr)[0], batch_size=8)


# ---------------------------------------------------------------------------------------------------------------------
# 3. the cut's reference
# ---------------------------------------------------------------------------------------------------------------------
def cut_reference(sampler, nodes, num_edge_type):
    """subgraph() + the trainer's masking (framework/trainer/kg.py: the Dr edges and types, the decoded Df triples, the rows):
    -> (dr_index, dr_type, dec_index, dec_type, [list-1 rows, list-2 rows] int32, number of Df edges of either direction)."""
    b = sampler.subgraph(nodes)
    dr_index, dr_type = b.edge_index[:, b.dr_mask], b.edge_type[b.dr_mask]
    pos_index, pos_type = b.edge_index[:, b.df_mask], b.edge_type[b.df_mask]
    fwd = pos_type < num_edge_type
    rows = [m.nonzero().flatten().to(torch.int32) for m in (b.sdf_node_1hop_mask_non_df_mask, b.sdf_node_2hop_mask_non_df_mask)]
    return dr_index, dr_type, pos_index[:, fwd], pos_type[fwd], rows, pos_index.shape[1]


def cut_reference_with_bad_row(sampler, nodes, bad_row, num_edge_type):
    """The reference of a node list whose entry `bad_row` is out of range: that row is empty and on no list, every other
    row keeps its number.  (The cut of the good nodes with the rows at and after bad_row shifted up by one: the shift is
    monotone, so the edge order stays subgraph()'s.)"""
    good = torch.cat([nodes[:bad_row], nodes[bad_row + 1:]])
    dr_index, dr_type, dec_index, dec_type, rows, m_df = cut_reference(sampler, good, num_edge_type)
    up = lambda t: t + (t >= bad_row).to(t.dtype)
    return up(dr_index), dr_type, up(dec_index), dec_type, [up(r) for r in rows], m_df


@functools.lru_cache(maxsize=None)
def cut_reference_cpu(key, nr=25):
    """cut_reference of a node set of node_sets() on the host sampler (shared by the tests of a process)."""
    return cut_reference(cpu_sampler(nr), node_sets(nr)[key], nr)


# ---------------------------------------------------------------------------------------------------------------------
# 4. gd_batch_typed_csr: a plain reference and the cases
# ---------------------------------------------------------------------------------------------------------------------
def typed_csr_reference(src, dst, etype, n, n_rel):
    """Node-major typed graphs of an edge list in numpy.  Per direction (fwd: node = target, other = source; bwd: node =
    source, other = target): drop the edges with an endpoint or a relation out of range, np.lexsort by (node, relation,
    other endpoint, input position), cut runs where (node, relation) changes, w = float32(1) / float32(|the edge's FORWARD
    run|) for both directions, node_ptr = runs per node.  -> SimpleNamespace(fwd, bwd, n_edges): fwd / bwd =
    (node_ptr int32 [n + 1], seg_ptr int32 [runs + 1], seg_rel int32 [runs], col int32 [E], w float32 [E]) as torch
    tensors, n_edges = the edges in range."""
    src, dst, et = (np.asarray(v, dtype=np.int64) for v in (src, dst, etype))
    ok = (src >= 0) & (src < n) & (dst >= 0) & (dst < n) & (et >= 0) & (et < n_rel)
    pos = np.nonzero(ok)[0]
    s, d, t = src[ok], dst[ok], et[ok]
    e = int(pos.size)

    def side(node, other, w_edge):
        order = np.lexsort((pos, other, t, node))           # the LAST key is the primary one
        node_s, rel_s = node[order], t[order]
        start = np.ones(e, dtype=bool)
        start[1:] = (node_s[1:] != node_s[:-1]) | (rel_s[1:] != rel_s[:-1])
        seg_ptr = np.concatenate([np.nonzero(start)[0], [e]]).astype(np.int64)
        lens = np.diff(seg_ptr)
        if w_edge is None:                                  # forward: the runs' own lengths
            w_sorted = np.repeat(np.float32(1) / lens.astype(np.float32), lens).astype(np.float32)
            w_edge = np.empty(e, dtype=np.float32)
            w_edge[order] = w_sorted
        else:
            w_sorted = w_edge[order]
        node_ptr = np.concatenate([[0], np.cumsum(np.bincount(node_s[start], minlength=n))])
        i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32))
        return (i32(node_ptr), i32(seg_ptr), i32(rel_s[start]), i32(other[order]), torch.from_numpy(np.ascontiguousarray(w_sorted))), w_edge

    fwd, w_edge = side(d, s, None)
    bwd, _ = side(s, d, w_edge)
    return SimpleNamespace(fwd=fwd, bwd=bwd, n_edges=e)


def _laid_out(runs, pool_lo, n, seed):
    """Edges whose FORWARD order is `runs` = [(node, relation, length)] (ascending) from position 0 on, with sources drawn
    from the nodes pool_lo .. n - 1 (above every run's node), plus the same edges flipped: their sources are the runs'
    nodes, so the BACKWARD order begins with the same layout."""
    g = torch.Generator().manual_seed(seed)
    node = torch.cat([torch.full((m,), v) for v, _, m in runs])
    rel = torch.cat([torch.full((m,), r) for _, r, m in runs])
    other = torch.randint(pool_lo, n, (node.numel(),), generator=g)
    ei = torch.cat([torch.stack([other, node]), torch.stack([node, other])], 1)
    ty = torch.cat([rel, rel])
    p = torch.randperm(ei.shape[1], generator=g)
    return ei[:, p].contiguous(), ty[p].contiguous()


def _chunk_edge_case(kind, n_rel=12):
    """Runs laid out around the sorted positions 1024 and 2048 (the run scan's chunk edges), on both sides:
      start_node   a run of a NEW node starts exactly at 1024, and one at 2048
      start_rel    a run ends at 1023 and the next run is the same node's with another relation; the same at 2047 | 2048
                   (the scan's first element of a chunk reads nkey[p - 1] across the chunk edge to see either)
      straddle     a run of 70 starts at 1000, one at 2030: no run starts at the chunk edge
    (three edge lists: a run cannot both start at a position and straddle it)"""
    g = torch.Generator().manual_seed({'start_node': 61, 'start_rel': 62, 'straddle': 63}[kind])
    runs, state = [], {'pos': 0, 'node': 0}

    def node_runs(lengths_by_rel):
        for r, m in sorted(lengths_by_rel.items()):
            runs.append((state['node'], r, m))
            state['pos'] += m
        state['node'] += 1

    def fill_to(target):
        while state['pos'] + 30 < target:
            rels = torch.randperm(n_rel, generator=g)[:int(torch.randint(1, 4, (1,), generator=g))].tolist()
            node_runs({r: int(torch.randint(1, 10, (1,), generator=g)) for r in rels})
        node_runs({int(torch.randint(0, n_rel, (1,), generator=g)): target - state['pos']})
        assert state['pos'] == target

    for edge in (SCAN, 2 * SCAN):
        if kind == 'start_node':
            fill_to(edge)
            node_runs({4: 9})
        elif kind == 'start_rel':
            fill_to(edge - 24)
            node_runs({2: 24, 5: 10})
        else:
            fill_to(edge - (24 if edge == SCAN else 18))
            node_runs({3 if edge == SCAN else 7: 70})
    fill_to(2300)
    n_run_nodes = state['node']
    n = n_run_nodes + 100
    ei, ty = _laid_out(runs, n_run_nodes, n, 7 + len(runs))
    return ei, ty, n, n_rel


def _boundary_case(n, variant=None, n_rel=12):
    g = torch.Generator().manual_seed(3000 + n + {None: 0, 'gap': 1, 'isolated_last': 2}[variant])
    ei = torch.randint(0, n, (2, 5 * n), generator=g)
    ty = torch.randint(0, n_rel, (5 * n,), generator=g)
    if variant == 'gap':                                    # nodes 1023 and 1024 have no in-edge: equal node offsets across the chunk
        keep = (ei[1] != SCAN - 1) & (ei[1] != SCAN)
        ei, ty = ei[:, keep], ty[keep]
    if variant == 'isolated_last':                          # the last node: no in-edge, no out-edge
        keep = (ei != n - 1).all(0)
        ei, ty = ei[:, keep], ty[keep]
    return ei.contiguous(), ty.contiguous(), n, n_rel


HUB_IN = {3: 64, 17: 65, 40: 129, 77: 3000}      # node -> in-edges
HUB_OUT = (120, 3000)                            # (node, out-edges)


def _hub_case(n=300, n_rel=12):
    """Hubs whose edges come from (go to) 50 nodes under 12 relations: parallel edges with equal (relation, other endpoint),
    so an edge's sorted position is decided by its input position."""
    g = torch.Generator().manual_seed(88)
    parts, types = [torch.randint(0, n, (2, 1500), generator=g)], [torch.randint(0, n_rel, (1500,), generator=g)]
    for node, m in HUB_IN.items():
        parts.append(torch.stack([torch.randint(200, 250, (m,), generator=g), torch.full((m,), node)]))
        types.append(torch.randint(0, n_rel, (m,), generator=g))
    node, m = HUB_OUT
    parts.append(torch.stack([torch.full((m,), node), torch.randint(200, 250, (m,), generator=g)]))
    types.append(torch.randint(0, n_rel, (m,), generator=g))
    ei, ty = torch.cat(parts, 1), torch.cat(types)
    p = torch.randperm(ei.shape[1], generator=g)
    return ei[:, p].contiguous(), ty[p].contiguous(), n, n_rel


def _out_of_range_case(n=700, n_rel=12):
    g = torch.Generator().manual_seed(91)
    ei = torch.randint(0, n, (2, 5000), generator=g)
    ty = torch.randint(0, n_rel, (5000,), generator=g)
    bad_ei = torch.randint(0, n, (2, 40), generator=g)
    bad_ty = torch.randint(0, n_rel, (40,), generator=g)
    bad_ei[0, 0:10] = n                                     # src = n
    bad_ei[1, 10:20] = -1                                   # dst = -1
    bad_ty[20:30] = n_rel                                   # type = n_rel
    bad_ty[30:40] = -1                                      # type = -1
    at = torch.cat([torch.tensor([0, 5039]), torch.randperm(5038, generator=g)[:38] + 1])      # scattered; the first and the last edge
    all_ei, all_ty = torch.zeros(2, 5040, dtype=torch.long), torch.zeros(5040, dtype=torch.long)
    is_bad = torch.zeros(5040, dtype=torch.bool)
    is_bad[at] = True
    all_ei[:, is_bad], all_ty[is_bad] = bad_ei, bad_ty
    all_ei[:, ~is_bad], all_ty[~is_bad] = ei, ty
    return all_ei.contiguous(), all_ty.contiguous(), n, n_rel


TYPED_CASES = ('n1023', 'n1024', 'n1025', 'n2049', 'n2049_gap', 'n1025_isolated_last', 'chunk_start_node', 'chunk_start_rel',
               'chunk_straddle', 'hubs', 'out_of_range')
CHUNK_EDGE_CASES = ('chunk_start_node', 'chunk_start_rel', 'chunk_straddle')


@functools.lru_cache(maxsize=None)
def typed_case(name):
    """-> (edge_index int64 [2, E], edge_type int64 [E], n, n_rel)"""
    if name.startswith('chunk_'):
        return _chunk_edge_case(name[len('chunk_'):])
    if name == 'hubs':
        return _hub_case()
    if name == 'out_of_range':
        return _out_of_range_case()
    size, _, variant = name[1:].partition('_')
    return _boundary_case(int(size), variant or None)


@functools.lru_cache(maxsize=None)
def typed_reference(name):
    ei, ty, n, r = typed_case(name)
    return typed_csr_reference(ei[0].numpy(), ei[1].numpy(), ty.numpy(), n, r)


# ---------------------------------------------------------------------------------------------------------------------
# 5. the whole step against float64
# ---------------------------------------------------------------------------------------------------------------------
STEP_CONFIGS = {'blocks-25': (25, (128, 128, 64)),        # more than 20 relation types: 4 diagonal blocks per relation weight
                'dense-6': (6, (32, 32, 16))}             # dense relation weights
STEP_ALPHA, STEP_LR, STEP_ROOTS = 0.5, 1e-3, 900
STEP_PERMS = (None, 1, 2)                                 # edge orders inside each batch of the fp32 ensemble members
STEP_LABELS = ('sampled 0', 'sampled 1', '1025 nodes', '2049 nodes', 'no decoded Df triple', 'no list-1 row')


@functools.lru_cache(maxsize=None)
def step_request(config, seed=42):
    """-> (data, nr, dims, state, batches): the request of a STEP_CONFIGS entry, a seeded RGCNDelete state (Del weights 0.5 I +
    0.05 randn, as oracle_jobs.minibatch_request sets them), and batches = [(label, nodes, dec_index, dec_type, neg)] in
    STEP_LABELS order with negatives drawn by the oracle's negative_sampling_kg under a seeded generator on the oracle's
    decoded triples.  CPU only."""
    from gnndelete_amd.framework import models as M
    from gnndelete_amd.framework.trainer.sampler import RandomWalkSubgraphSampler
    from oracle import gnndelete_ref as R
    from oracle import pyg_semantics as pyg
    nr, dims = STEP_CONFIGS[config]
    data = kg_request(nr=nr, seed=seed)
    n = int(data.num_nodes)
    rng = torch.get_rng_state()
    torch.default_generator.manual_seed(seed + 1)           # the host generator alone, put back below
    model = M.RGCNDelete(SimpleNamespace(in_dim=dims[0], hidden_dim=dims[1], out_dim=dims[2]), n, nr, data.sdf_node_1hop_mask,
                         data.sdf_node_2hop_mask)
    torch.set_rng_state(rng)
    gw = torch.Generator().manual_seed(seed + 2)
    with torch.no_grad():
        for p in (model.deletion1.deletion_weight, model.deletion2.deletion_weight):
            p.copy_(torch.eye(p.shape[0]) * 0.5 + torch.randn(p.shape, generator=gw) * 0.05)
    state = {k: v.detach().clone() for k, v in model.state_dict().items()}
    sampler = RandomWalkSubgraphSampler(data, batch_size=STEP_ROOTS, walk_length=2, num_steps=2,
                                        generator=torch.Generator().manual_seed(seed + 3))
    sets = list(sampler.node_sets())
    gs = torch.Generator().manual_seed(seed + 5)
    sets += [torch.randperm(n, generator=gs)[:size].sort().values for size in (SCAN + 1, 2 * SCAN + 1)]
    df_nodes = torch.zeros(n, dtype=torch.bool)
    df_nodes[data.edge_index[:, data.df_mask].flatten()] = True
    sets += [sets[0][~df_nodes[sets[0]]], sets[1][~data.sdf_node_1hop_mask_non_df_mask[sets[1]]]]
    d = {k: v for k, v in data.items()}
    gn = torch.Generator().manual_seed(seed + 4)
    batches = []
    for label, nodes in zip(STEP_LABELS, sets):
        b = pyg.saint_subgraph(d, nodes)
        pos, pt = b['edge_index'][:, b['df_mask']], b['edge_type'][b['df_mask']]
        fw = pt < nr
        dec, dec_t = pos[:, fw].contiguous(), pt[fw].contiguous()
        batches.append((label, nodes, dec, dec_t, R.negative_sampling_kg(dec, dec_t, generator=gn)))
    return data, nr, dims, state, batches


def step_batch_reference(config, w1, w2, nodes, neg, dtype, perm=None):
    """oracle.gnndelete_ref.TwoLayerDelete('rgcn') on one batch in `dtype` (CPU) from Del weights (w1, w2), as
    kg_nodeemb_minibatch runs it (message passing on the batch's Dr edges, the S_Df-minus-Df node masks as Del masks, DEC on
    the forward-direction Df triples against `neg`, plain MSE): -> dict of dL1/dW_D1, dL2/dW_D1, dL2/dW_D2 (float64) and the
    four squared-difference sums (DEC 1, NI 1, DEC 2, NI 2).  perm: the batch's Dr edge columns (and their types) permuted
    before message passing - another summation order in every scatter (an fp32 ensemble member)."""
    from oracle import gnndelete_ref as R
    from oracle import pyg_semantics as pyg
    data, nr, dims, state, _ = step_request(config)
    ref = R.TwoLayerDelete('rgcn', *dims, num_nodes=int(data.num_nodes), num_edge_type=nr)
    missing = ref.load_state_dict(state, strict=False)
    assert not missing.missing_keys and not missing.unexpected_keys, missing
    with torch.no_grad():
        ref.deletion1.deletion_weight.copy_(w1)
        ref.deletion2.deletion_weight.copy_(w2)
    ref = ref.to(dtype)
    b = pyg.saint_subgraph({k: v for k, v in data.items()}, nodes)
    ei, et = b['edge_index'][:, b['dr_mask']], b['edge_type'][b['dr_mask']]
    pos, pt = b['edge_index'][:, b['df_mask']], b['edge_type'][b['df_mask']]
    pos = pos[:, pt < nr]
    if perm is not None:
        p = torch.randperm(ei.shape[1], generator=torch.Generator().manual_seed(perm))
        ei, et = ei[:, p], et[p]
    m1, m2 = b['sdf_node_1hop_mask_non_df_mask'], b['sdf_node_2hop_mask_non_df_mask']
    with torch.no_grad():
        z1o, z2o = ref.get_original_embeddings(b['x'], ei, et, return_all_emb=True)
    z1, z2 = ref(b['x'], ei, et, m1, m2, return_all_emb=True)
    r1, r2, l1, l2 = R.nodeemb_terms(z1, z2, z1o, z2o, pos, neg, m1, m2, nn.MSELoss())
    a = STEP_ALPHA
    W1, W2 = ref.deletion1.deletion_weight, ref.deletion2.deletion_weight

    def grads(loss, params):
        gs = torch.autograd.grad(loss, params, retain_graph=True, allow_unused=True)
        return [torch.zeros_like(p_).double() if g_ is None else g_.double() for g_, p_ in zip(gs, params)]
    (g1_l1,) = grads(a * r1 + (1 - a) * l1, [W1])
    g1_l2, g2 = grads(a * r2 + (1 - a) * l2, [W1, W2])
    with torch.no_grad():
        def dec(z, zo):
            return float(((torch.cat([z[pos[0]], z[pos[1]]]) - torch.cat([zo[neg[0]], zo[neg[1]]])).double() ** 2).sum())
        sums = torch.tensor([dec(z1, z1o), float(((z1[m1] - z1o[m1]).double() ** 2).sum()), dec(z2, z2o),
                             float(((z2[m2] - z2o[m2]).double() ** 2).sum())], dtype=torch.float64)
    return dict(g1_l1=g1_l1, g1_l2=g1_l2, g2=g2, sums=sums, counts=(int(nodes.numel()), int(ei.shape[1]), int(pos.shape[1]),
                                                                    int(m1.sum()), int(m2.sum())))


STEP_QUANTITIES = (('g1_l1', 'W_D1 gradient handed to Adam (loss1 + carried)'), ('g2', 'W_D2 gradient (loss2)'),
                   ('g1_l2', 'W_D1 gradient carried (loss2)'))
STEP_SUMS = ('DEC 1', 'NI 1', 'DEC 2', 'NI 2')


def step_distances(got, want, carry=None, got_holds_carry=False):
    """The seven compared quantities of a batch: {name: distance of `got` to `want`} - rel-L2 for the three gradients
    (`carry`, the W_D1 gradient the previous batch left, added to want's g1_l1 and - unless got_holds_carry - to got's),
    |difference| / |value| for the four sums; a sum that is 0.0 in `want` (a sum over zero terms) is left out and must be
    asserted exactly by the caller."""
    from helpers import rel_l2
    out = {}
    for key, name in STEP_QUANTITIES:
        add = carry if (key == 'g1_l1' and carry is not None) else 0
        out[name] = rel_l2(got[key] + (0 if got_holds_carry else add), want[key] + add)
    for k, name in enumerate(STEP_SUMS):
        w_ = float(want['sums'][k])
        if w_ != 0.0:
            out[f'{name} sum'] = abs(float(got['sums'][k]) - w_) / abs(w_)
    return out
