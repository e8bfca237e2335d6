"""--fused_backbone without a GPU: fused_backbone_unsupported's verdicts on CPU-constructed models and optimizers (one reason
per case), the flag's parsing, and the per-epoch draw of the fused path (negative_sampling_cached on the Dr edge set) against
negative_sampling for the same generator state."""
from types import SimpleNamespace

import pytest
import torch

from gnndelete_amd.backbone import fused_backbone_unsupported
from gnndelete_amd.framework import graph_utils as GU
from gnndelete_amd.framework import models as M
from gnndelete_amd.framework.training_args import build_parser
from helpers import random_graph


def _dims(i=24, h=16, o=8):
    return SimpleNamespace(in_dim=i, hidden_dim=h, out_dim=o)


def _model(name, dims=None):
    dims = dims or _dims()
    if name in ('rgcn', 'rgat'):
        return {'rgcn': M.RGCN, 'rgat': M.RGAT}[name](dims, num_nodes=30, num_edge_type=3)
    return {'gcn': M.GCN, 'gat': M.GAT, 'gin': M.GIN, 'sage': M.SAGE}[name](dims)


ARGS = SimpleNamespace(fused_backbone=True, minibatch=False)


@pytest.mark.parametrize('gnn', ['gcn', 'gat'])
def test_gcn_and_gat_with_one_plain_adam_apply(gnn):
    m = _model(gnn)
    assert fused_backbone_unsupported(m, ARGS, torch.optim.Adam(m.parameters(), lr=1e-3)) is None
    if gnn == 'gat':
        assert len(list(m.parameters())) == 8                       # lin_src and lin_dst are one tensor


@pytest.mark.parametrize('gnn,name', [('gin', 'GIN'), ('sage', 'SAGE'), ('rgcn', 'RGCN'), ('rgat', 'RGAT')])
def test_other_backbones_are_named_in_the_reason(gnn, name):
    m = _model(gnn)
    reason = fused_backbone_unsupported(m, ARGS, torch.optim.Adam(m.parameters(), lr=1e-3))
    assert reason == f'no fused backbone step for the {name} backbone (GCN and GAT only)'


def test_the_delete_models_are_not_backbones():
    mask = torch.zeros(10, dtype=torch.bool)
    m = M.GCNDelete(_dims(), mask, mask)
    reason = fused_backbone_unsupported(m, ARGS, torch.optim.Adam(m.parameters(), lr=1e-3))
    assert reason is not None and 'GCNDelete' in reason


def test_every_other_obstacle_has_a_reason_of_its_own(monkeypatch):
    m = _model('gcn')
    params = list(m.parameters())
    cases = {
        'sgd': (m, ARGS, torch.optim.SGD(params, lr=1e-3)),
        'adamw': (m, ARGS, torch.optim.AdamW(params, lr=1e-3, weight_decay=0.0)),
        'two optimizers': (m, ARGS, [torch.optim.Adam(params[:2], lr=1e-3), torch.optim.Adam(params[2:], lr=1e-3)]),
        'two groups': (m, ARGS, torch.optim.Adam([{'params': params[:2]}, {'params': params[2:]}], lr=1e-3)),
        'weight decay': (m, ARGS, torch.optim.Adam(params, lr=1e-3, weight_decay=5e-4)),
        'amsgrad': (m, ARGS, torch.optim.Adam(params, lr=1e-3, amsgrad=True)),
        'some parameters': (m, ARGS, torch.optim.Adam(params[1:], lr=1e-3)),
        'minibatch': (m, SimpleNamespace(fused_backbone=True, minibatch=True), torch.optim.Adam(params, lr=1e-3)),
    }
    for dims, tag in ((_dims(h=18), 'hidden % 4'), (_dims(o=6), 'out % 4'), (_dims(h=1028), 'hidden > 1024'),
                      (_dims(i=1500, h=20), 'wide input')):
        mm = _model('gat', dims)
        cases[tag] = (mm, ARGS, torch.optim.Adam(mm.parameters(), lr=1e-3))
    reasons = {k: fused_backbone_unsupported(*v) for k, v in cases.items()}
    for k, r in reasons.items():
        assert isinstance(r, str) and r and '\n' not in r, k
    plain = 'the optimizer is not one plain torch.optim.Adam'
    assert reasons['sgd'] == reasons['adamw'] == reasons['two optimizers'] == reasons['two groups'] == plain
    assert reasons['weight decay'] == 'Adam with weight decay'
    assert 'amsgrad' in reasons['amsgrad']
    assert reasons['some parameters'] == 'the optimizer does not hold exactly the model\'s parameters'
    assert '--minibatch' in reasons['minibatch']
    assert reasons['hidden % 4'] == 'widths 18 / 8 (multiples of 4 up to 1024)'
    assert reasons['out % 4'] == 'widths 16 / 6 (multiples of 4 up to 1024)'
    assert reasons['hidden > 1024'] == 'widths 1028 / 8 (multiples of 4 up to 1024)'
    assert reasons['wide input'] == 'no kernel for a 1500 -> 20 first product'
    # one reason per kind of obstacle
    assert len({plain, reasons['weight decay'], reasons['amsgrad'], reasons['some parameters'], reasons['minibatch'],
                reasons['hidden % 4'], reasons['wide input']}) == 7
    # more than one rank
    import torch.distributed as dist
    monkeypatch.setattr(dist, 'is_initialized', lambda: True)
    monkeypatch.setattr(dist, 'get_world_size', lambda *a, **k: 2)
    monkeypatch.setattr(dist, 'get_rank', lambda *a, **k: 0)
    assert fused_backbone_unsupported(m, ARGS, torch.optim.Adam(params, lr=1e-3)) == 'torch.distributed with more than one rank'


def test_a_wide_input_with_a_matrix_core_hidden_width_applies():
    m = _model('gcn', _dims(i=1639, h=128, o=64))
    assert fused_backbone_unsupported(m, ARGS, torch.optim.Adam(m.parameters(), lr=1e-3)) is None


def test_fused_backbone_flag_parses_and_defaults_off():
    assert build_parser().parse_args([]).fused_backbone is False
    assert build_parser().parse_args(['--fused_backbone']).fused_backbone is True
    assert build_parser().parse_args(['--unlearning_model', 'retrain', '--fused_backbone']).fused_backbone is True


@pytest.mark.parametrize('seed', [0, 1])
def test_cached_draw_on_the_dr_edge_set_equals_negative_sampling(seed):
    """RetrainTrainer's request: positives = train_pos_edge_index[:, dr_mask], as many negatives as Dr edges."""
    n = 300
    ei = random_graph(n, 900, seed, loops=False)
    g = torch.Generator().manual_seed(seed + 5)
    dr_mask = torch.rand(ei.shape[1], generator=g) > 0.05
    dr = ei[:, dr_mask].contiguous()
    want = int(dr_mask.sum())
    keys = GU.positive_edge_keys(dr, n)
    torch.manual_seed(77)
    ref = [GU.negative_sampling(edge_index=dr, num_nodes=n, num_neg_samples=want) for _ in range(3)]
    torch.manual_seed(77)
    got = [GU.negative_sampling_cached(keys, n, want) for _ in range(3)]
    for a, b in zip(ref, got):
        assert a.shape == (2, want) and a.dtype == b.dtype and torch.equal(a, b)
    assert not torch.equal(got[0], got[1])
    # the trainers' seam: the cached draw is taken only while the module-level name is the real sampler
    from gnndelete_amd.framework.trainer.base import Trainer
    draw = Trainer._cached_negative_draw(GU.negative_sampling, dr, n)
    torch.manual_seed(77)
    assert torch.equal(draw(want), ref[0])
    assert Trainer._cached_negative_draw(lambda *a, **k: None, dr, n) is None
