"""The fused GraphSAINT batch step (gnndelete_amd.minibatch, --minibatch --fused_minibatch): the device cut and batch CSRs
bit-identical to the sampler's subgraph() and graph.build_csr, and the step's trajectory against the reference's and
against the autograd mini-batch loop."""
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from helpers import hip_model, load_golden, rel_l2, split_fixture, t

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lists(fx, prefix, count_key):
    return [t(fx[f'{prefix}::{i}']) for i in range(int(fx[count_key]))]


def _synthetic(n=3000, m=24000, seed=5):
    """Directed edges with multi-edges, self loops and one hub of ~2,000 out-edges; random sdf / df / node masks."""
    from gnndelete_amd.framework.data import Data
    g = torch.Generator().manual_seed(seed)
    ei = torch.randint(0, n, (2, m), generator=g)
    hub = torch.stack([torch.zeros(2000, dtype=torch.long), torch.randint(0, n, (2000,), generator=g)])
    ei = torch.cat([ei, hub, ei[:, :50], torch.arange(20).repeat(2, 1)], 1)
    e = ei.shape[1]
    sdf = torch.rand(e, generator=g) < 0.6
    df = sdf & (torch.rand(e, generator=g) < 0.1)
    d = Data(num_nodes=n, edge_index=ei, x=torch.randn(n, 8, generator=g), sdf_mask=sdf, df_mask=df)
    for k in ['sdf_node_1hop_mask', 'sdf_node_2hop_mask', 'sdf_node_1hop_mask_non_df_mask', 'sdf_node_2hop_mask_non_df_mask']:
        d[k] = torch.rand(n, generator=g) < 0.4
    return d


def _node_sets(n, g):
    """Random sets, a set holding the hub (node 0), single nodes (17 has a self loop), all nodes."""
    return [torch.randperm(n, generator=g)[:700].sort().values,
            torch.cat([torch.zeros(1, dtype=torch.long), torch.randperm(n - 1, generator=g)[:400] + 1]).sort().values,
            torch.tensor([17]), torch.tensor([3]), torch.arange(n)]


def _assert_cut_matches_subgraph(cut, sampler, nodes):
    """One cut of `nodes` against sampler.subgraph: edges, flags, counts, the four row lists and the Df edges, bit for bit."""
    dev = cut.dev
    cnt = cut.cut(nodes.to(dev))
    ref = sampler.subgraph(nodes.to(dev))
    got_ei, got_f = cut.batch_edges()
    assert torch.equal(got_ei, ref.edge_index), nodes.numel()
    assert torch.equal(got_f & 1, ref.sdf_mask.to(torch.uint8)) and torch.equal(got_f >> 1, ref.df_mask.to(torch.uint8))
    assert cnt[:4] == [nodes.numel(), ref.edge_index.shape[1], int(ref.sdf_mask.sum()), int(ref.df_mask.sum())]
    for k, key in enumerate(['sdf_node_1hop_mask', 'sdf_node_2hop_mask', 'sdf_node_1hop_mask_non_df_mask',
                             'sdf_node_2hop_mask_non_df_mask']):
        rows = ref[key].nonzero().flatten().to(torch.int32)
        assert cnt[4 + k] == rows.numel() and torch.equal(cut.rows(k, rows.numel()), rows)
    assert torch.equal(cut.df_index[:, :cnt[3]], ref.edge_index[:, ref.df_mask])
    ei = ref.edge_index
    assert cnt[8] == int((ei[0] != ei[1]).sum()) and cnt[9] == int((ei[0] != ei[1])[ref.sdf_mask].sum())
    return ref


def test_cut_is_bit_identical_to_subgraph():
    from gnndelete_amd.framework.trainer.sampler import RandomWalkSubgraphSampler
    from gnndelete_amd.minibatch import BatchCut
    d = _synthetic()
    dev = torch.device('cuda')
    sampler = RandomWalkSubgraphSampler(d.clone().to(dev), batch_size=100)
    cut = BatchCut(d, sampler, dev, max_nodes=64)            # small buffers: the first big batches grow them
    sets = _node_sets(d.num_nodes, torch.Generator().manual_seed(1))
    # a set with no induced edge: nodes that share no edge
    ei = d.edge_index
    lonely = torch.tensor([v for v in range(100, 3000) if int(((ei[0] == v) | (ei[1] == v)).sum()) == 0][:5] or [2999])
    sets.append(lonely.sort().values)
    for nodes in sets:
        _assert_cut_matches_subgraph(cut, sampler, nodes)
    assert cut.e_cap >= d.edge_index.shape[1]


@pytest.mark.parametrize('mode', ['gcn', 'gat'])
def test_batch_csrs_match_build_csr(mode):
    from gnndelete_amd.framework.trainer.sampler import RandomWalkSubgraphSampler
    from gnndelete_amd.graph import build_csr
    from gnndelete_amd.minibatch import BatchCut
    d = _synthetic(seed=9)
    dev = torch.device('cuda')
    sampler = RandomWalkSubgraphSampler(d.clone().to(dev), batch_size=100)
    cut = BatchCut(d, sampler, dev)
    for nodes in _node_sets(d.num_nodes, torch.Generator().manual_seed(2)):
        cut.cut(nodes.to(dev))
        ref_b = sampler.subgraph(nodes.to(dev))
        for sdf in (False, True):
            ei = ref_b.edge_index[:, ref_b.sdf_mask] if sdf else ref_b.edge_index
            ref = build_csr(ei.contiguous(), nodes.numel(), mode)
            got = cut.batch_csr(sdf, mode == 'gat')
            for key in ['rowptr', 'col', 'rowptr_t', 'col_t', 'perm_t']:
                assert torch.equal(getattr(got, key), getattr(ref, key)), (key, sdf)
            if mode == 'gcn':
                assert torch.equal(got.val, ref.val) and torch.equal(got.val_t, ref.val_t)


def _traj_setup(tmp_path, monkeypatch, fused, sets=None, negs=True, gnn='gat', state_seed=None):
    from gnndelete_amd.framework.data import Data
    from gnndelete_amd.framework.trainer import gnndelete_nodeemb as TN
    from gnndelete_amd.framework.trainer import sampler as S
    fx = load_golden('traj_minibatch_gat.npz')
    state, data, rest = split_fixture(fx)
    if gnn == 'gcn':
        from gnndelete_amd.framework import models as M
        torch.manual_seed(state_seed)
        i, h, o = data['x'].shape[1], 32, 16
        m = M.GCNDelete(SimpleNamespace(in_dim=i, hidden_dim=h, out_dim=o), data['sdf_node_1hop_mask'],
                        data['sdf_node_2hop_mask']).cuda()
    else:
        m = hip_model(gnn, state, data['sdf_node_1hop_mask'], data['sdf_node_2hop_mask'])
    sets = sets if sets is not None else _lists(fx, 'batch', 'n_batches')
    monkeypatch.setattr(S, 'make_sampler', lambda d, batch_size, num_steps, walk_length=2: S.FixedNodeSets(d, sets))
    if negs:
        it = iter(_lists(fx, 'negs', 'n_negs'))
        monkeypatch.setattr(S, 'negative_sampling', lambda ei, n, k: next(it).to(ei.device))
    epochs = int(rest['epochs'])
    args = SimpleNamespace(unlearning_model='gnndelete_nodeemb', dataset='ogbl-synth', checkpoint_dir=str(tmp_path),
                           eval_on_cpu=False, epochs=epochs, valid_freq=epochs, lr=float(rest['lr']),
                           alpha=float(rest['alpha']), loss_fct='mse_mean', loss_type='both_layerwise', gnn=gnn,
                           batch_size=40, num_steps=len(sets), minibatch=True, fused_minibatch=fused)
    opt = [torch.optim.Adam(m.deletion1.parameters(), lr=args.lr), torch.optim.Adam(m.deletion2.parameters(), lr=args.lr)]
    tr = TN.GNNDeleteNodeembTrainer(args)
    torch.manual_seed(int(rest['eval_seed']))
    tr.train(m, Data(data), opt, args)
    return tr, m, opt, rest, data


def test_fused_minibatch_reproduces_reference_trajectory(tmp_path, monkeypatch):
    tr, m, _, rest, _ = _traj_setup(tmp_path, monkeypatch, True)
    assert tr.trainer_log['minibatch_step'] == 'fused'
    steps = tr.trainer_log['steps']
    assert len(steps) == len(rest['train_loss'])
    for key in ['train_loss', 'train_loss_l', 'train_loss_r']:
        np.testing.assert_allclose([s_[key] for s_ in steps], rest[key], rtol=1e-4, atol=1e-8, err_msg=key)
    assert rel_l2(m.deletion1.deletion_weight.detach().cpu(), rest['final_w1']) < 1e-4
    assert rel_l2(m.deletion2.deletion_weight.detach().cpu(), rest['final_w2']) < 1e-4
    vals = [r for r in tr.trainer_log['log'] if 'val_dt_auc' in r]
    assert abs(vals[-1]['val_dt_auc'] - float(rest['val_dt_auc'][-1])) < 2e-3
    assert abs(vals[-1]['val_df_auc'] - float(rest['val_df_auc'][-1])) < 2e-3
    assert tr._fused_minibatch_step.cut.reads == len(steps)          # one blocking host read per batch


def _edge_case_sets():
    """The fixture's node sets plus a batch without a Df edge and one without an S1 row."""
    fx = load_golden('traj_minibatch_gat.npz')
    _, data, _ = split_fixture(fx)
    n = int(data['x'].shape[0])
    df_nodes = set(data['directed_df_edge_index'].flatten().tolist())
    s1 = data['sdf_node_1hop_mask']
    no_df = torch.tensor([v for v in range(n) if v not in df_nodes][:60])
    no_s1 = (~s1).nonzero().flatten()[:60]
    return _lists(fx, 'batch', 'n_batches') + [no_df.sort().values, no_s1.sort().values]


@pytest.mark.parametrize('gnn', ['gcn', 'gat'])
def test_fused_minibatch_matches_autograd_loop(gnn, tmp_path, monkeypatch):
    sets = _edge_case_sets()
    runs = []
    for fused in (False, True):
        torch.manual_seed(1234)                         # negatives from sampler.negative_sampling: the same draws
        runs.append(_traj_setup(tmp_path, monkeypatch, fused, sets=sets, negs=False, gnn=gnn, state_seed=7))
    (ta, ma, oa, _, _), (tf, mf, of, _, _) = runs
    assert ta.trainer_log['minibatch_step'] == 'autograd' and tf.trainer_log['minibatch_step'] == 'fused'
    for key in ['train_loss', 'train_loss_l', 'train_loss_r']:
        a = np.array([s_[key] for s_ in ta.trainer_log['steps']])
        f = np.array([s_[key] for s_ in tf.trainer_log['steps']])
        assert np.array_equal(np.isfinite(a), np.isfinite(f)), key
        assert not np.isfinite(a).all(), 'the edge-case batches log a mean over zero rows'
        np.testing.assert_allclose(f[np.isfinite(f)], a[np.isfinite(a)], rtol=1e-4, atol=1e-8, err_msg=key)
    for pa, pf in [(ma.deletion1.deletion_weight, mf.deletion1.deletion_weight),
                   (ma.deletion2.deletion_weight, mf.deletion2.deletion_weight)]:
        assert rel_l2(pf.detach().cpu(), pa.detach().cpu()) < 1e-4
    for opa, opf in zip(oa, of):
        (pa,), (pf,) = opa.param_groups[0]['params'], opf.param_groups[0]['params']
        sa, sf = opa.state[pa], opf.state[pf]
        assert float(sa['step']) == float(sf['step'])
        for k in ['exp_avg', 'exp_avg_sq']:
            assert rel_l2(sf[k].cpu(), sa[k].cpu()) < 1e-4, k
    assert rel_l2(mf.deletion1.deletion_weight.grad.cpu(), ma.deletion1.deletion_weight.grad.cpu()) < 1e-4


def test_fused_minibatch_is_reproducible(tmp_path, monkeypatch):
    sets = _edge_case_sets()
    out = []
    for _ in range(2):
        torch.manual_seed(99)
        tr, m, _, _, _ = _traj_setup(tmp_path, monkeypatch, True, sets=sets, negs=False)
        out.append(([s_['train_loss'] for s_ in tr.trainer_log['steps']], m.deletion1.deletion_weight.detach().cpu().clone(),
                    m.deletion2.deletion_weight.detach().cpu().clone()))
    assert np.array_equal(np.array(out[0][0]), np.array(out[1][0]), equal_nan=True)
    assert torch.equal(out[0][1], out[1][1]) and torch.equal(out[0][2], out[1][2])


def test_fused_minibatch_falls_back_for_gin(tmp_path, monkeypatch, capsys):
    from gnndelete_amd.framework import models as M
    from gnndelete_amd.framework.data import Data
    from gnndelete_amd.framework.trainer import gnndelete_nodeemb as TN
    from gnndelete_amd.framework.trainer import sampler as S
    fx = load_golden('traj_minibatch_gat.npz')
    _, data, rest = split_fixture(fx)
    sets = _lists(fx, 'batch', 'n_batches')
    monkeypatch.setattr(S, 'make_sampler', lambda d, batch_size, num_steps, walk_length=2: S.FixedNodeSets(d, sets))
    res = []
    for fused in (False, True):
        torch.manual_seed(3)
        m = M.GINDelete(SimpleNamespace(in_dim=data['x'].shape[1], hidden_dim=32, out_dim=16), data['sdf_node_1hop_mask'],
                        data['sdf_node_2hop_mask']).cuda()
        args = SimpleNamespace(unlearning_model='gnndelete_nodeemb', dataset='ogbl-synth', checkpoint_dir=str(tmp_path),
                               eval_on_cpu=False, epochs=2, valid_freq=2, lr=float(rest['lr']), alpha=float(rest['alpha']),
                               loss_fct='mse_mean', loss_type='both_layerwise', gnn='gin', batch_size=40, num_steps=len(sets),
                               minibatch=True, fused_minibatch=fused)
        opt = [torch.optim.Adam(m.deletion1.parameters(), lr=args.lr), torch.optim.Adam(m.deletion2.parameters(), lr=args.lr)]
        tr = TN.GNNDeleteNodeembTrainer(args)
        torch.manual_seed(11)
        tr.train(m, Data(dict(data)), opt, args)
        res.append((tr, m.deletion2.deletion_weight.detach().cpu().clone()))
    assert 'no fused batch step for the GINDelete backbone' in capsys.readouterr().out
    assert res[1][0].trainer_log['minibatch_step'] == 'autograd'
    assert torch.equal(res[0][1], res[1][1])


def test_cli_fused_minibatch_agrees_with_autograd_loop(tmp_path, monkeypatch):
    import subprocess
    import sys
    monkeypatch.setenv('GNNDELETE_FORCE_EPOCHS', '2')
    monkeypatch.setenv('GNNDELETE_FORCE_VALID_FREQ', '2')
    monkeypatch.setenv('GNNDELETE_FORCE_NUM_STEPS', '3')
    from gnndelete_amd.framework.synth import make_linkpred_dataset
    data, df = make_linkpred_dataset(None, seed=42, shape=(800, 32, 4000, 'dense'))
    logs = []
    for flag in ([], ['--fused_minibatch']):
        cwd = str(tmp_path / ('fused' if flag else 'autograd'))
        data_dir = os.path.join(cwd, 'data', 'ogbl-synth')
        os.makedirs(data_dir)
        data.save(os.path.join(data_dir, 'd_42.pt'))
        torch.save(df, os.path.join(data_dir, 'df_42.pt'))
        common = ['--dataset', 'ogbl-synth', '--gnn', 'gcn', '--random_seed', '42', '--batch_size', '200']
        env = dict(os.environ, PYTHONPATH=ROOT)
        for cmd in (['train_gnn.py'] + common,
                    ['delete_gnn.py'] + common + ['--unlearning_model', 'gnndelete_nodeemb', '--df', 'in', '--df_size', '5',
                                                  '--minibatch'] + flag):
            r = subprocess.run([sys.executable, os.path.join(ROOT, cmd[0])] + cmd[1:], cwd=cwd, env=env, capture_output=True,
                               text=True, timeout=900)
            assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        out = os.path.join(cwd, 'checkpoint', 'ogbl-synth', 'gcn', 'gnndelete_nodeemb',
                           'mse_mean-both_layerwise-0.5-non_connected', 'in-5.0-42')
        with open(os.path.join(out, 'trainer_log.json')) as f:
            logs.append(json.load(f))
    assert logs[0]['minibatch_step'] == 'autograd' and logs[1]['minibatch_step'] == 'fused'
    assert abs(logs[0]['dt_auc'] - logs[1]['dt_auc']) < 2e-3


# ------------------------------------------------------------------------------------------------ cut, CSR and loss-term shapes
_CHUNK_ROWS = {0: 63, 1: 64, 2: 65, 3: 128, 4: 129}       # rows whose out-edges all land in the batch: 1 - 3 ballot chunks


def _boundary_graph(n=3000, m=24000, seed=13):
    """_synthetic's kind of graph, plus rows 0-4 whose ONLY out-edges are 63 / 64 / 65 / 128 / 129 edges to distinct
    targets, and out-edges of node n - 1 (the last row of the sampler's rowptr) -> (data, {row: its targets})."""
    from gnndelete_amd.framework.data import Data
    g = torch.Generator().manual_seed(seed)
    ei = torch.randint(0, n, (2, m), generator=g)
    ei[0] = ei[0].clamp(min=len(_CHUNK_ROWS))
    targets = {r: torch.randperm(n - 100, generator=g)[:k] + 100 for r, k in _CHUNK_ROWS.items()}
    last = torch.stack([torch.full((40,), n - 1), torch.randint(0, n, (40,), generator=g)])
    parts = [ei, last, ei[:, :50], torch.arange(20, 40).repeat(2, 1)]
    parts += [torch.stack([torch.full_like(t_, r), t_]) for r, t_ in targets.items()]
    ei = torch.cat(parts, 1)
    e = ei.shape[1]
    sdf = torch.rand(e, generator=g) < 0.6
    df = sdf & (torch.rand(e, generator=g) < 0.1)
    d = Data(num_nodes=n, edge_index=ei, x=torch.randn(n, 8, generator=g), sdf_mask=sdf, df_mask=df)
    for k in ['sdf_node_1hop_mask', 'sdf_node_2hop_mask', 'sdf_node_1hop_mask_non_df_mask', 'sdf_node_2hop_mask_non_df_mask']:
        d[k] = torch.rand(n, generator=g) < 0.4
    return d, targets


def _sized_set(n, size, g, must=()):
    """A sorted node set of exactly `size` nodes holding `must` (node n - 1 included whenever it fits)."""
    must = torch.as_tensor(sorted(set(must) | ({n - 1} if size > len(must) else set())), dtype=torch.long)[:size]
    rest = torch.ones(n, dtype=torch.bool)
    rest[must] = False
    pool = rest.nonzero().flatten()
    extra = pool[torch.randperm(pool.numel(), generator=g)[:size - must.numel()]]
    return torch.cat([must, extra]).sort().values


def test_cut_at_scan_and_ballot_chunk_boundaries():
    """gd_induced_subgraph against sampler.subgraph, bit for bit, at the cut's shape boundaries: batch sizes around the
    1024-row chunks of cut_scan_kernel (1, 1023, 1024, 1025, 2049, all nodes) and rows with exactly 63 / 64 / 65 / 128 /
    129 in-batch out-edges (the 64-edge ballot chunks of cut_count_kernel / cut_write_kernel)."""
    from gnndelete_amd.framework.trainer.sampler import RandomWalkSubgraphSampler
    from gnndelete_amd.minibatch import BatchCut
    d, targets = _boundary_graph()
    n = d.num_nodes
    dev = torch.device('cuda')
    sampler = RandomWalkSubgraphSampler(d.clone().to(dev), batch_size=100)
    cut = BatchCut(d, sampler, dev)
    g = torch.Generator().manual_seed(3)
    chunk_rows = set(_CHUNK_ROWS) | set(torch.cat(list(targets.values())).tolist())
    sets = [torch.tensor([0]), torch.tensor([n - 1])]
    sets += [_sized_set(n, k, g, chunk_rows if k > len(chunk_rows) else ()) for k in (1023, 1024, 1025, 2049)]
    sets += [torch.arange(n), torch.tensor(sorted(chunk_rows))]
    for nodes in sets:
        ref = _assert_cut_matches_subgraph(cut, sampler, nodes)
        if set(_CHUNK_ROWS) <= set(nodes.tolist()):
            out_deg = torch.bincount(ref.edge_index[0].cpu(), minlength=nodes.numel())
            assert [int(out_deg[r]) for r in _CHUNK_ROWS] == list(_CHUNK_ROWS.values())   # rows 0-4 are batch rows 0-4


def test_cut_generation_stamps_buffer_growth_and_bad_ids():
    """50 overlapping batches on one BatchCut (nodes of batch k that are not in batch k + 1 must leave no edge behind: the
    relabel array is never cleared, only re-stamped), an edge-buffer grow-and-recut halfway through, and an out-of-range
    node id (IndexError from the count vector) after which the same cut still cuts correctly."""
    from gnndelete_amd.framework.trainer.sampler import RandomWalkSubgraphSampler
    from gnndelete_amd.minibatch import BatchCut
    d, _ = _boundary_graph(seed=17)
    n = d.num_nodes
    dev = torch.device('cuda')
    sampler = RandomWalkSubgraphSampler(d.clone().to(dev), batch_size=100)
    cut = BatchCut(d, sampler, dev, max_nodes=64)
    g = torch.Generator().manual_seed(5)
    grown = 0
    for k in range(50):
        width, start = (400, 37 * k) if k < 25 else (2000, 20 * k)     # small batches first, then ~4 x the edge buffer
        window = (torch.arange(width) + start) % n
        nodes = window[torch.rand(width, generator=g) < 0.75].unique()
        if k % 7 == 3:
            nodes = torch.cat([nodes, torch.tensor([n - 1])]).unique()
        e_cap, reads = cut.e_cap, cut.reads
        ref = _assert_cut_matches_subgraph(cut, sampler, nodes)
        if ref.edge_index.shape[1] > e_cap:
            assert cut.reads == reads + 2 and cut.e_cap >= ref.edge_index.shape[1], k     # grown, cut again
            grown += 1
        else:
            assert cut.reads == reads + 1, k
    assert grown >= 1 and cut.e_cap > 1024
    for bad in (torch.tensor([0, 5, n]), torch.tensor([-1, 2, 9])):
        with pytest.raises(IndexError):
            cut.cut(bad.to(dev))
        _assert_cut_matches_subgraph(cut, sampler, _sized_set(n, 1500, g))


def _batch_csr_call(ei, n, gat):
    """gd_batch_csr on edge list `ei` [2, e] (self loops already dropped, as the cut hands them over)."""
    from gnndelete_amd import _lib
    from gnndelete_amd._lib import check, ptr, stream_ptr
    dev = torch.device('cuda')
    e = ei.shape[1]
    src, dst = torch.empty(e + n, dtype=torch.int64, device=dev), torch.empty(e + n, dtype=torch.int64, device=dev)
    src[:e], dst[:e] = ei[0].to(dev), ei[1].to(dev)
    L = _lib.lib()
    nnz = e + n
    i32 = dict(dtype=torch.int32, device=dev)
    out = {k: torch.empty(n + 1, **i32) for k in ('rowptr', 'rowptr_t')}
    out.update({k: torch.empty(nnz, **i32) for k in ('col', 'col_t', 'perm_t')})
    out['val'] = out['val_t'] = None
    if not gat:
        out['val'], out['val_t'] = torch.empty(nnz, device=dev), torch.empty(nnz, device=dev)
    ws = torch.empty(max(256, L.gd_batch_csr_workspace(n, e)), dtype=torch.uint8, device=dev)
    check(L.gd_batch_csr(ptr(src), ptr(dst), e, n, 1 if gat else 0, ptr(out['rowptr']), ptr(out['col']), ptr(out['val']),
                         ptr(out['rowptr_t']), ptr(out['col_t']), ptr(out['perm_t']), ptr(out['val_t']), ptr(ws), ws.numel(),
                         stream_ptr(dev)), 'gd_batch_csr')
    return {k: (v.cpu() if v is not None else None) for k, v in out.items()}


@pytest.mark.parametrize('case', ['no-edges', 'only-self-loops', 'duplicates', 'batch-24k'])
def test_batch_csr_vs_numpy_and_fp64_norm(case):
    """gd_batch_csr against an independent reference: pyg_semantics.with_single_self_loops, a stable numpy argsort per
    direction and pyg_semantics.gcn_norm in float64 (no gd_csr_from_coo / gd_gcn_norm_f32 on the expected side).  Index
    arrays exact; the GCN values within a few fp32 ulps (1 / sqrtf(deg) per endpoint)."""
    from oracle import pyg_semantics as pyg
    g = torch.Generator().manual_seed(len(case))
    if case == 'no-edges':
        n, raw = 7, torch.zeros(2, 0, dtype=torch.long)
    elif case == 'only-self-loops':
        n = 40
        raw = torch.arange(0, n, 3).repeat(2, 1)
    elif case == 'duplicates':
        n = 300
        raw = torch.randint(0, n, (2, 2000), generator=g)
        raw = torch.cat([raw, raw[:, :500], raw[:, :100], torch.arange(0, n, 5).repeat(2, 1)], 1)
        raw = raw[:, torch.randperm(raw.shape[1], generator=g)]
    else:
        n = 24_576
        raw = torch.randint(0, n, (2, 240_000), generator=g)
        raw = torch.cat([raw, raw[:, :1000], torch.stack([torch.randint(0, n, (3000,), generator=g), torch.full((3000,), 5)])], 1)
    loops = raw[0] == raw[1]
    e2 = pyg.with_single_self_loops(raw, n).numpy()
    src, dst = e2[0], e2[1]
    order = np.argsort(dst * n + src, kind='stable')
    order_t = np.argsort(src * n + dst, kind='stable')
    inv = np.empty_like(order)
    inv[order] = np.arange(order.size)
    want = dict(rowptr=np.concatenate([[0], np.cumsum(np.bincount(dst, minlength=n))]), col=src[order],
                rowptr_t=np.concatenate([[0], np.cumsum(np.bincount(src, minlength=n))]), col_t=dst[order_t],
                perm_t=inv[order_t])
    _, w = pyg.gcn_norm(raw, n, torch.float64)
    w = w.numpy()
    for gat in (True, False):
        got = _batch_csr_call(raw[:, ~loops], n, gat)
        for key, val in want.items():
            assert np.array_equal(got[key].numpy().astype(np.int64), val), (case, key, gat)
        if gat:
            continue
        np.testing.assert_allclose(got['val'].numpy(), w[order], rtol=1e-6, atol=0, err_msg=case)
        np.testing.assert_allclose(got['val_t'].numpy(), w[order_t], rtol=1e-6, atol=0, err_msg=case)


def _loss_terms_call(pos, n_pos, neg, ni, n_b, w_dec, w_ni):
    from gnndelete_amd import _lib
    from gnndelete_amd._lib import check, ptr, stream_ptr
    dev = torch.device('cuda')
    L = _lib.lib()
    n_terms = 2 * n_pos + ni.numel()
    pos, neg, ni = pos.to(dev).contiguous(), neg.to(dev).contiguous(), ni.to(dev, torch.int32).contiguous()
    seg_ptr = torch.full((n_b + 1,), -7, dtype=torch.int32, device=dev)
    term_o = torch.empty(max(n_terms, 1), dtype=torch.int32, device=dev)
    term_w = torch.empty(max(n_terms, 1), dtype=torch.float32, device=dev)
    term_kind = torch.empty(max(n_terms, 1), dtype=torch.int32, device=dev)
    ws = torch.empty(max(256, L.gd_batch_loss_terms_workspace(n_b, n_terms)), dtype=torch.uint8, device=dev)
    check(L.gd_batch_loss_terms(ptr(pos), pos.stride(0), ptr(neg), neg.stride(0), n_pos, ptr(ni), int(ni.numel()), n_b, w_dec,
                                w_ni, ptr(seg_ptr), ptr(term_o), ptr(term_w), ptr(term_kind), ptr(ws), ws.numel(),
                                stream_ptr(dev)), 'gd_batch_loss_terms')
    return seg_ptr.cpu().numpy(), term_o[:n_terms].cpu().numpy(), term_w[:n_terms].cpu().numpy(), term_kind[:n_terms].cpu().numpy()


@pytest.mark.parametrize('n_b,n_pos,n_ni,ld_pos,hub', [(500, 300, 200, 1024, False), (500, 0, 150, 0, False),
                                                      (500, 120, 0, 4096, False), (64, 0, 0, 0, False),
                                                      (2000, 700, 400, 700, True), (1, 3, 1, 5, False)])
def test_batch_loss_terms_vs_numpy(n_b, n_pos, n_ni, ld_pos, hub):
    """gd_batch_loss_terms against numpy: the terms (pos0 -> neg0, pos1 -> neg1, then NI rows onto themselves) grouped by
    the z row they touch - what gd_csr_from_coo(targets, rows) yields: a stable sort on (row, target), so a row's terms
    run by target and, for equal targets, in term order.  That order is the summation order of gd_rowpair_mse_f32.
    seg_ptr, term_o and term_kind exact, term_w the DEC / NI weight of each term.  Cases: no DEC terms, no NI terms, none
    at all, pos with a leading dimension above n_pos (the step passes df_index with stride e_cap), one row hit by 1,000
    terms with repeated targets, terms on row n_b - 1."""
    g = torch.Generator().manual_seed(n_b + n_pos)
    pos = torch.zeros(2, max(ld_pos, n_pos, 1), dtype=torch.long)
    pos[:, :n_pos] = torch.randint(0, n_b, (2, n_pos), generator=g)
    neg = torch.randint(0, n_b, (2, n_pos), generator=g)
    if hub:                                      # 1,000 terms on row 7, targets from a small range: equal (row, target) pairs
        pos[0, :500] = 7
        pos[1, :500] = 7
        neg[:, :500] = torch.randint(0, 9, (2, 500), generator=g)
    if n_pos:
        pos[0, n_pos - 1] = n_b - 1
    ni = torch.randperm(n_b, generator=g)[:n_ni].sort().values
    if n_ni:
        ni[-1] = n_b - 1
        ni = ni.unique()
    w_dec, w_ni = 0.25 / max(n_pos, 1), 0.125 / max(ni.numel(), 1)
    seg_ptr, term_o, term_w, term_kind = _loss_terms_call(pos, n_pos, neg, ni, n_b, w_dec, w_ni)
    rows = np.concatenate([pos[0, :n_pos].numpy(), pos[1, :n_pos].numpy(), ni.numpy()])
    tgts = np.concatenate([neg[0].numpy(), neg[1].numpy(), ni.numpy()])
    kind = np.concatenate([np.zeros(2 * n_pos, np.int64), np.ones(ni.numel(), np.int64)])
    order = np.argsort(rows.astype(np.int64) * n_b + tgts, kind='stable')
    assert np.array_equal(seg_ptr, np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n_b))]))
    assert np.array_equal(term_o, tgts[order])
    assert np.array_equal(term_kind, kind[order])
    assert np.array_equal(term_w, np.where(kind[order] == 1, np.float32(w_ni), np.float32(w_dec)).astype(np.float32))
    if hub:
        assert seg_ptr[8] - seg_ptr[7] >= 1000
