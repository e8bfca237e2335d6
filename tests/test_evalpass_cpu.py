"""The prepared validation pass on the host (gnndelete_amd/evalpass.py, --fused_validation): the flag, the two ABI entries and
their argument checks, every reason of validation_unsupported, the numpy restatements against direct fp64 torch / scikit-learn
computations, the staleness key of the plans and the pinned entries of graph.CACHE.  No GPU."""
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F


def test_the_flag_parses_and_defaults_off():
    from gnndelete_amd.framework.training_args import EXTRA_FLAGS, build_parser
    assert 'fused_validation' in [f[0] for f in EXTRA_FLAGS]
    p = build_parser()
    assert p.parse_args([]).fused_validation is False
    a = p.parse_args(['--fused_validation', '--fused_eval', '--unlearning_model', 'gnndelete_nodeemb'])
    assert a.fused_validation is True and a.fused_eval is True and a.unlearning_model == 'gnndelete_nodeemb'
    assert not hasattr(build_parser(extra=False).parse_args([]), 'fused_validation')
    (text,) = [help_ for name, _, _, help_ in EXTRA_FLAGS if name == 'fused_validation']
    assert 'not bit-equal' in text and '--fused_eval' in text


def test_the_entries_are_declared_bound_and_check_their_arguments():
    from gnndelete_amd import _lib
    names = ['gd_eval_edge_scores_f32', 'gd_eval_edge_scores_workspace', 'gd_row_nll_eval_f32', 'gd_row_nll_eval_workspace']
    declared = _lib.declared_symbols()
    assert all(n in declared and n in _lib.PROTOTYPES for n in names)
    assert sorted(declared) == sorted(_lib.PROTOTYPES)
    L = _lib.lib()
    assert L.gd_abi_version() == 9 and _lib.ABI_VERSION == 9
    with open(_lib.HEADER_PATH) as f:
        header = f.read()
    assert '#define GD_ABI_VERSION 9' in header and 'LOWEST index among equal maxima' in header
    # workspaces in doubles: a partial and a flag / count per block, 4 * (64 / lanes per item) items per block, 1,024 blocks at most
    assert L.gd_eval_edge_scores_workspace(1, 4) == 2 and L.gd_eval_edge_scores_workspace(257, 4) == 4
    assert L.gd_eval_edge_scores_workspace(9, 256) == 2 * 3 and L.gd_eval_edge_scores_workspace(10 ** 7, 64) == 2048
    assert L.gd_row_nll_eval_workspace(0, 7) == 2 and L.gd_row_nll_eval_workspace(5000, 7) == 2 * 40
    assert L.gd_row_nll_eval_workspace(5000, 256) == 2048
    # refused before anything is launched (these run without a GPU)
    buf = (8 * 64 * b'\0')
    import ctypes
    mem = ctypes.create_string_buffer(buf, len(buf))
    p = ctypes.addressof(mem) + (-ctypes.addressof(mem) % 16)
    assert L.gd_eval_edge_scores_f32(p, 4, 2, 4, p, p, 0, 0, 0, 0, p, p, p, p, None) == 2                    # no edges
    assert b'segments' in L.gd_last_error_string()
    assert L.gd_eval_edge_scores_f32(p, 6, 2, 6, p, p, 1, 1, 0, 0, p, p, p, p, None) == 2                    # d % 4
    assert L.gd_eval_edge_scores_f32(p, 260, 2, 260, p, p, 1, 1, 0, 0, p, p, p, p, None) == 2                # d > 256
    assert L.gd_eval_edge_scores_f32(p, 4, 2, 8, p, p, 1, 1, 0, 0, p, p, p, p, None) == 2                    # pitch below d
    assert L.gd_eval_edge_scores_f32(p, 4, 2, 4, p, p, 1, -1, 0, 0, p, p, p, p, None) == 2
    assert L.gd_eval_edge_scores_f32(p, 4, 2, 4, None, p, 1, 1, 0, 0, p, p, p, p, None) == 1
    assert L.gd_eval_edge_scores_f32(p + 4, 4, 2, 4, p, p, 1, 1, 0, 0, p, p, p, p, None) == 3
    assert L.gd_row_nll_eval_f32(p, 4, 2, 0, p, 1, p, p, p, p, None) == 2                                    # no classes
    assert L.gd_row_nll_eval_f32(p, 300, 2, 257, p, 1, p, p, p, p, None) == 2
    assert L.gd_row_nll_eval_f32(p, 3, 2, 4, p, 1, p, p, p, p, None) == 2                                    # pitch below the classes
    assert L.gd_row_nll_eval_f32(p, 4, 2, 4, None, 1, p, p, p, p, None) == 1
    assert L.gd_row_nll_eval_f32(p, 4, 2, 4, p, 1, p, p + 4, p, p, None) == 3


def _model(kind='gcn', delete=False, out_dim=32):
    from gnndelete_amd.framework import get_model
    args = SimpleNamespace(unlearning_model='gnndelete_nodeemb' if delete else 'retrain', gnn=kind, in_dim=8, hidden_dim=16, out_dim=out_dim)
    return get_model(args, torch.zeros(5, dtype=torch.bool), torch.zeros(5, dtype=torch.bool)) if delete else get_model(args)


def test_every_fallback_has_its_reason():
    from gnndelete_amd.evalpass import validation_unsupported
    from gnndelete_amd.framework.models import RGCN
    from gnndelete_amd.rankeval import fused_eval_unsupported
    for kind in ('gcn', 'gat', 'gin'):
        assert validation_unsupported(_model(kind)) is None and validation_unsupported(_model(kind, delete=True)) is None
        assert validation_unsupported(_model(kind), 'nodecls') is None
    gcn = _model()
    kg = RGCN(SimpleNamespace(in_dim=8, hidden_dim=8, out_dim=8), 6, 3)
    reasons = [
        validation_unsupported(kg),
        validation_unsupported(torch.nn.Linear(3, 3), 'nodecls'),
        validation_unsupported(gcn, 'linkpred', 32, on_gpu=False),
        validation_unsupported(gcn, 'nodecls', 7, on_gpu=False),
        validation_unsupported(gcn, 'linkpred', 32, torch.float64),
        validation_unsupported(gcn, 'nodecls', 7, torch.float16),
        validation_unsupported(gcn, 'linkpred', 30),
        validation_unsupported(gcn, 'linkpred', 260),
        validation_unsupported(gcn, 'nodecls', 257),
        validation_unsupported(gcn, 'linkpred', rankings=[(10, 100, 10), (0, 100, 10)]),
        validation_unsupported(gcn, 'linkpred', 64, rankings=[(10, 100, 101)]),
    ]
    assert reasons == [
        'no prepared validation for the RGCN model (the homogeneous two-layer backbones and their Delete wrappers only)',
        'no prepared validation for the Linear model (the homogeneous two-layer backbones and their Delete wrappers only)',
        'the embeddings are not on the GPU',
        'the logits are not on the GPU',
        'torch.float64 embeddings (float32 only)',
        'torch.float16 logits (float32 only)',
        'embedding width 30 (a multiple of 4 up to 256)',
        'embedding width 260 (a multiple of 4 up to 256)',
        '257 classes (the scoring kernel takes up to 256)',
        fused_eval_unsupported(0, 100, 10),
        fused_eval_unsupported(10, 100, 101),
    ]
    assert len(set(reasons)) == len(reasons) and all(r and '\n' not in r for r in reasons)
    # what the kernels do take: a class count needs no alignment, an embedding width does
    assert validation_unsupported(gcn, 'nodecls', 1) is None and validation_unsupported(gcn, 'nodecls', 7) is None
    assert validation_unsupported(gcn, 'linkpred', 4) is None and validation_unsupported(gcn, 'linkpred', 256, rankings=[(3, 9, 3)]) is None
    assert validation_unsupported(gcn, 'linkpred', 0) == 'embedding width 0 (a multiple of 4 up to 256)'
    with pytest.raises(ValueError, match='linkpred or nodecls'):
        validation_unsupported(gcn, 'kg')


def _edge_case(seed, n, d, segments, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(n, d, generator=g) * scale
    m = sum(segments)
    return z, torch.randint(0, n, (m,), generator=g), torch.randint(0, n, (m,), generator=g)


@pytest.mark.parametrize('segments', [(65, 63, 1, 130), (7, 5, 0, 0), (1, 1, 1, 1), (0, 4, 3, 0)])
def test_reference_edge_scores_is_the_doubled_sigmoid_loss(segments):
    from gnndelete_amd.evalpass import reference_edge_scores, reference_edge_stats
    z, src, dst = _edge_case(1, 40, 12, segments, 0.6)
    n_pos, n_neg, n_df, n_dr = segments
    s64, loss, mean, std = reference_edge_scores(z, src, dst, segments)
    want = torch.sigmoid((z.double()[src] * z.double()[dst]).sum(1))
    assert s64.dtype == np.float64 and np.abs(s64 - want.numpy()).max() <= 4e-16
    # upstream's quirk: binary_cross_entropy_with_logits on the SIGMOID OUTPUTS (the fp32 scores, widened)
    s32 = torch.from_numpy(s64.astype(np.float32)).double()
    label = torch.cat([torch.ones(n_pos), torch.zeros(n_neg)]).double()
    assert abs(loss - float(F.binary_cross_entropy_with_logits(s32[:n_pos + n_neg], label))) <= 1e-15
    assert 0.31 <= loss <= 1.32
    df = s32[n_pos + n_neg:n_pos + n_neg + n_df]
    if n_df:
        assert abs(mean - float(df.mean())) <= 1e-15 and abs(std - float(df.std(unbiased=False))) <= 1e-15
        assert mean == pytest.approx(np.mean(df.tolist()), abs=1e-15) and std == pytest.approx(np.std(df.tolist()), abs=1e-15)
    else:
        assert math.isnan(mean) and math.isnan(std)
    # the statistics of given scores (the kernel's own) are taken over those
    given = torch.rand(sum(segments)).float()
    assert np.array_equal(reference_edge_scores(z, src, dst, segments, given)[1:], reference_edge_stats(given, segments), equal_nan=True)
    with pytest.raises(ValueError, match='do not add up'):
        reference_edge_scores(z, src, dst, (1, 1, 1, 0) if sum(segments) != 3 else (1, 1, 1, 1))


def test_reference_edge_scores_edges():
    from gnndelete_amd.evalpass import reference_edge_scores, reference_edge_stats
    # all Df scores equal (unlearning has driven them together): two passes leave no cancellation
    for value in (0.5, 0.7310585975646973, 1.0, 1e-30):
        loss, mean, std = reference_edge_stats(np.full(1000 + 4, value, dtype=np.float32), (2, 2, 1000, 0))
        assert std <= 1e-15 and abs(mean - float(np.float32(value))) <= 1e-15
    # no stage edges: NaN loss; no Df: NaN mean / std
    loss, mean, std = reference_edge_stats(np.array([0.25, 0.75], dtype=np.float32), (0, 0, 2, 0))
    assert math.isnan(loss) and mean == 0.5 and std == 0.25
    # saturated logits: finite scores and terms, exactly 1 / next to 0
    z = torch.tensor([[10.0, 0.0, 0.0, 0.0], [-10.0, 0.0, 0.0, 0.0], [0.0, 0.0, 0.0, 0.0]])
    src, dst = torch.tensor([0, 0, 2, 0]), torch.tensor([0, 1, 2, 7])          # logits 100, -100, 0 and an endpoint out of range
    s64, loss, mean, std = reference_edge_scores(z, src, dst, (2, 2, 0, 0))
    assert s64[0] == 1.0 and 0.0 < s64[1] < 1e-43 and s64[2] == 0.5 and s64[3] == 0.5
    assert np.isfinite(loss) and math.isnan(mean)


@pytest.mark.parametrize('classes, pitch', [(1, 1), (3, 3), (4, 6), (7, 7), (64, 64), (256, 260)])
def test_reference_row_nll_eval_is_nll_of_log_softmax(classes, pitch):
    from sklearn.metrics import accuracy_score, f1_score
    from gnndelete_amd.evalpass import reference_row_nll_eval
    g = torch.Generator().manual_seed(classes)
    z = torch.randn(90, pitch, generator=g) * 3
    y = torch.randint(0, classes, (90,), generator=g)
    rows = torch.randperm(90, generator=g)[:65]
    loss, correct = reference_row_nll_eval(z, rows, y, classes)
    zd = z[:, :classes].double()
    want = float(F.nll_loss(F.log_softmax(zd, dim=1)[rows], y[rows]))
    assert abs(loss - want) <= 1e-12 * max(abs(want), 1.0)
    pred = zd[rows].argmax(1)
    acc = correct / rows.numel()
    assert acc == accuracy_score(y[rows], pred) and acc == f1_score(y[rows], pred, average='micro')


def test_reference_row_nll_eval_edges():
    from gnndelete_amd.evalpass import reference_row_nll_eval
    z = torch.tensor([[1.0, 2.0, 2.0], [0.5, 0.5, 0.5], [3.0, 1.0, 3.0], [0.0, 9.0, 0.0]])
    y = torch.tensor([1, 0, 2, 5])
    # ties take the lowest index: row 0 -> 1 (hit), row 1 -> 0 (hit), row 2 -> 0 (miss)
    loss, correct = reference_row_nll_eval(z, [0, 1, 2], y)
    assert correct == 2
    lse = torch.logsumexp(z.double(), 1)
    assert abs(loss - float((lse[0] - 2 + lse[1] - 0.5 + lse[2] - 3) / 3)) <= 1e-15
    # a label out of range counts as wrong with term 0, a row id out of range is skipped; both stay in the divisor
    loss2, correct2 = reference_row_nll_eval(z, [0, 3, 17, -1], y)
    assert correct2 == 1 and abs(loss2 - float(lse[0] - 2) / 4) <= 1e-15
    loss3, correct3 = reference_row_nll_eval(z, [], y)
    assert math.isnan(loss3) and correct3 == 0
    # d_valid below the width: the columns beyond it are not looked at
    assert reference_row_nll_eval(z, [3], torch.tensor([0, 0, 0, 0]), 1) == (0.0, 1)


def _data(stage_edges=6):
    from gnndelete_amd.framework.data import Data
    g = torch.Generator().manual_seed(0)
    e = torch.randint(0, 9, (2, 20), generator=g)
    mask = torch.rand(20, generator=g) < 0.7
    return Data({'x': torch.randn(9, 8, generator=g), 'train_pos_edge_index': e, 'dr_mask': mask, 'dtrain_mask': mask.clone(), 'num_nodes': 9,
                 'val_pos_edge_index': torch.randint(0, 9, (2, stage_edges), generator=g),
                 'val_neg_edge_index': torch.randint(0, 9, (2, stage_edges), generator=g),
                 'test_pos_edge_index': torch.randint(0, 9, (2, stage_edges), generator=g),
                 'test_neg_edge_index': torch.randint(0, 9, (2, stage_edges), generator=g),
                 'directed_df_edge_index': e[:, ~mask].clone(),
                 'val_mask': torch.rand(9, generator=g) < 0.5, 'y': torch.randint(0, 3, (9,), generator=g), 'edge_index': e.clone()})


def test_the_staleness_key_sees_in_place_edits_and_replacements():
    from gnndelete_amd.evalpass import LinkValidationPlan, NodeValidationPlan
    data = _data()
    key = lambda stage='val', original=False: LinkValidationPlan.key_of(data, stage, original, 'cuda:0')       # noqa: E731
    first = key()
    assert key() == first and key('test') != first and key(original=True) != first
    assert LinkValidationPlan.key_of(data, 'val', False, 'cuda:1') != first
    for name in ('train_pos_edge_index', 'dtrain_mask', 'val_pos_edge_index', 'val_neg_edge_index', 'directed_df_edge_index', 'dr_mask'):
        before = key()
        data[name][..., 0] = data[name][..., 0]                      # an in-place write: same values, another _version
        assert key() != before, name
        before = key()
        data[name] = data[name].clone()                              # another tensor in its place
        assert key() != before, name
    before = key()
    data.test_pos_edge_index[0, 0] = 1                               # not a source of the val plan
    assert key() == before and key('test') != LinkValidationPlan.key_of(_data(), 'test', False, 'cuda:0')
    # `original` does not read Df / Dr
    before = key(original=True)
    data.directed_df_edge_index[0, 0] = 2
    assert key(original=True) == before and key() != first
    # without dtrain_mask the message-passing mask is dr_mask
    del data['dtrain_mask']
    before = key()
    data.dr_mask[0] = ~data.dr_mask[0]
    assert key() != before
    nkey = NodeValidationPlan.key_of(data, 'cuda:0')
    for name in ('val_mask', 'y', 'edge_index'):
        before = NodeValidationPlan.key_of(data, 'cuda:0')
        data[name][..., 0] = data[name][..., 0]
        assert NodeValidationPlan.key_of(data, 'cuda:0') != before, name
    assert NodeValidationPlan.key_of(data, 'cuda:0') != nkey and NodeValidationPlan.key_of(data, 'cpu') != NodeValidationPlan.key_of(data, 'cuda:0')


def test_a_pinned_graph_outlives_the_lru(monkeypatch):
    """graph._GraphCache.pin: the graphs of a pinned tensor are built once and held while more graphs than the LRU's capacity
    pass through; an in-place edit rebuilds; unpin lets go.  (build_csr replaced: nothing runs on a device here.)"""
    from gnndelete_amd import graph
    built = []
    monkeypatch.setattr(graph, 'build_csr', lambda e, n, mode: built.append((id(e), mode)) or object())
    cache = graph._GraphCache(capacity=8)
    mine, early = torch.zeros(2, 3, dtype=torch.long), torch.zeros(2, 4, dtype=torch.long)
    g_early = cache.get(early, 5, 'gcn')                             # built before its pin: moves out of the LRU on the next hit
    cache.pin(mine)
    cache.pin(early)
    g_gcn, g_gat = cache.get(mine, 5, 'gcn'), cache.get(mine, 5, 'gat')
    assert cache.get(early, 5, 'gcn') is g_early and len(cache.entries) == 0 and len(cache.held) == 3
    others = [torch.zeros(2, 2, dtype=torch.long) for _ in range(10)]
    for o in others:
        cache.get(o, 5, 'gcn')
    assert len(cache.entries) == 8 and len(built) == 13
    assert cache.get(mine, 5, 'gcn') is g_gcn and cache.get(mine, 5, 'gat') is g_gat and cache.get(early, 5, 'gcn') is g_early
    assert len(built) == 13
    assert cache.get(others[0], 5, 'gcn') is not None and len(built) == 14        # the unpinned one was evicted
    mine[0, 0] = 1                                                   # edited in place: rebuilt, the stale graph dropped
    assert cache.get(mine, 5, 'gcn') is not g_gcn and len(built) == 15 and len(cache.held) == 3
    cache.pin(mine)                                                  # pins count
    cache.unpin(mine)
    assert len(cache.held) == 3
    cache.unpin(mine)
    assert len(cache.held) == 1 and id(mine) not in cache.pins
    cache.unpin(mine)                                                # once too often: nothing happens
    cache.get(mine, 5, 'gcn')
    assert len(built) == 16 and len(cache.held) == 1                 # back in the LRU
    cache.clear()
    assert cache.entries == [] and cache.held == []


def test_the_trainers_consult_the_flag_first(tmp_path, monkeypatch, capsys):
    """Without the flag evalpass is not entered; with it an unsupported model records and prints its reason once and the torch
    path runs (stopped here at its GPU requirement: this machine has none, or at the stand-in below)."""
    from gnndelete_amd import evalpass
    from gnndelete_amd.framework.trainer import base as TB
    calls = []
    monkeypatch.setattr(evalpass, 'validation_unsupported', lambda *a, **k: calls.append(a[1]) or 'forced by the test')
    monkeypatch.setattr(TB, '_require_gpu', lambda: None)
    monkeypatch.setattr(TB, 'device', torch.device('cpu'))

    class Stop(Exception):
        pass

    def stop(*a, **k):
        raise Stop
    model = _model()
    monkeypatch.setattr(type(model), 'forward', stop)
    data = _data()
    mk = lambda **flags: SimpleNamespace(dataset='synth-tiny', unlearning_model='retrain', checkpoint_dir=str(tmp_path), **flags)       # noqa: E731
    for cls, task in ((TB.Trainer, 'linkpred'), (TB.NodeClassificationTrainer, 'nodecls')):
        off = cls(mk())
        with pytest.raises(Stop):
            off.eval(model, data, 'val')
        assert calls == [] and 'validation_path' not in off.trainer_log
        on = cls(mk(fused_validation=True, fused_eval=True))
        for _ in range(2):
            with pytest.raises(Stop):
                on.eval(model, data, 'val')
        assert calls == [task, task] and on.trainer_log['validation_path'] == 'torch: forced by the test'
        assert 'eval_path' not in on.trainer_log                     # (written by the rankings of the torch path only)
        assert capsys.readouterr().out.count('--fused_validation: forced by the test; validating on the torch path') == 1
        calls.clear()
