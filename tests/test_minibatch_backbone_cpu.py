"""The fused backbone batch step (train_gnn.py --minibatch --fused_minibatch) without a GPU: every verdict of
fused_minibatch_backbone_unsupported on CPU-constructed models and optimizers (one line and one reason per obstacle), the
flag's help text, and the refusals of gd_rows_gather_gemm_f32 that come before any launch."""
import ctypes
from types import SimpleNamespace

import pytest
import torch

from gnndelete_amd import _lib
from gnndelete_amd.framework import models as M
from gnndelete_amd.minibatch import fused_minibatch_backbone_unsupported

ARGS = SimpleNamespace(unlearning_model='original', minibatch=True, fused_minibatch=True)


def _dims(i=24, h=16, o=8):
    return SimpleNamespace(in_dim=i, hidden_dim=h, out_dim=o)


def _model(name, dims=None):
    dims = dims or _dims()
    if name in ('rgcn', 'rgat'):
        return {'rgcn': M.RGCN, 'rgat': M.RGAT}[name](dims, num_nodes=30, num_edge_type=3)
    return {'gcn': M.GCN, 'gat': M.GAT, 'gin': M.GIN, 'sage': M.SAGE}[name](dims)


def _adam(m, **kw):
    return torch.optim.Adam(m.parameters(), lr=1e-3, **kw)


@pytest.mark.parametrize('gnn', ['gcn', 'gat'])
def test_gcn_and_gat_with_one_plain_adam_apply(gnn):
    m = _model(gnn)
    assert fused_minibatch_backbone_unsupported(m, ARGS, _adam(m)) is None
    # an input width that is no multiple of 4 (the reference fixture's in_dim = 10) is no obstacle
    m = _model(gnn, _dims(i=10))
    assert fused_minibatch_backbone_unsupported(m, ARGS, _adam(m)) is None


@pytest.mark.parametrize('gnn,name', [('gin', 'GIN'), ('sage', 'SAGE'), ('rgcn', 'RGCN'), ('rgat', 'RGAT')])
def test_other_backbones_are_refused_by_name(gnn, name):
    m = _model(gnn)
    assert fused_minibatch_backbone_unsupported(m, ARGS, _adam(m)) == \
        f'no fused backbone batch step for the {name} backbone (GCN and GAT only)'


def test_the_delete_models_are_refused_by_name():
    mask = torch.zeros(10, dtype=torch.bool)
    for cls in (M.GCNDelete, M.GATDelete):
        m = cls(_dims(), mask, mask)
        assert fused_minibatch_backbone_unsupported(m, ARGS, _adam(m)) == \
            f'no fused backbone batch step for the {cls.__name__} backbone (GCN and GAT only)'


def test_every_other_obstacle_has_a_reason_of_its_own(monkeypatch):
    m = _model('gcn')
    params = list(m.parameters())
    cases = {
        'sgd': (m, torch.optim.SGD(params, lr=1e-3)),
        'adamw': (m, torch.optim.AdamW(params, lr=1e-3, weight_decay=0.0)),
        'two optimizers': (m, [torch.optim.Adam(params[:2], lr=1e-3), torch.optim.Adam(params[2:], lr=1e-3)]),
        'two groups': (m, torch.optim.Adam([{'params': params[:2]}, {'params': params[2:]}], lr=1e-3)),
        'weight decay': (m, _adam(m, weight_decay=5e-4)),
        'amsgrad': (m, _adam(m, amsgrad=True)),
        'maximize': (m, _adam(m, maximize=True)),
        'some parameters': (m, torch.optim.Adam(params[1:], lr=1e-3)),
    }
    for dims, tag in ((_dims(h=18), 'hidden % 4'), (_dims(o=6), 'out % 4'), (_dims(h=1028), 'hidden > 1024'),
                      (_dims(i=1500, h=128), 'wide input')):
        mm = _model('gat', dims)
        cases[tag] = (mm, _adam(mm))
    reasons = {k: fused_minibatch_backbone_unsupported(mm, ARGS, opt) for k, (mm, opt) in cases.items()}
    for k, r in reasons.items():
        assert isinstance(r, str) and r and '\n' not in r, k
    plain = 'the optimizer is not one plain torch.optim.Adam'
    assert reasons['sgd'] == reasons['adamw'] == reasons['two optimizers'] == reasons['two groups'] == plain
    assert reasons['weight decay'] == 'Adam with weight decay'
    assert reasons['amsgrad'] == reasons['maximize'] == 'Adam with amsgrad / maximize'
    assert reasons['some parameters'] == 'the optimizer does not hold exactly the model\'s parameters'
    assert reasons['hidden % 4'] == 'widths 18 / 8 (multiples of 4 up to 1024)'
    assert reasons['out % 4'] == 'widths 16 / 6 (multiples of 4 up to 1024)'
    assert reasons['hidden > 1024'] == 'widths 1028 / 8 (multiples of 4 up to 1024)'
    assert reasons['wide input'] == 'input width 1500 (the gathering first product takes up to 1024)'
    rank = 'torch.distributed with more than one rank'
    backbone = fused_minibatch_backbone_unsupported(_model('gin'), ARGS, _adam(_model('gin')))
    assert len({plain, reasons['weight decay'], reasons['amsgrad'], reasons['some parameters'], reasons['hidden % 4'],
                reasons['wide input'], rank, backbone}) == 8             # one reason per kind of obstacle
    import torch.distributed as dist
    monkeypatch.setattr(dist, 'is_initialized', lambda: True)
    monkeypatch.setattr(dist, 'get_world_size', lambda *a, **k: 2)
    monkeypatch.setattr(dist, 'get_rank', lambda *a, **k: 0)
    assert fused_minibatch_backbone_unsupported(m, ARGS, _adam(m)) == rank


def test_minibatch_is_no_obstacle_here_and_stays_one_for_the_full_batch_flag():
    from gnndelete_amd.backbone import fused_backbone_unsupported
    m = _model('gcn')
    args = SimpleNamespace(minibatch=True, fused_minibatch=True, fused_backbone=True)
    assert fused_minibatch_backbone_unsupported(m, args, _adam(m)) is None
    assert fused_backbone_unsupported(m, args, _adam(m)) == '--minibatch trains on GraphSAINT batches'


def test_the_flag_names_the_backbone_trainer():
    from gnndelete_amd.framework import training_args as TA
    (text,) = [help_ for name, _, _, help_ in TA.FLAGS + TA.EXTRA_FLAGS if name == 'fused_minibatch']
    assert 'train_gnn.py' in text and 'gnndelete_nodeemb and gnndelete trainers' in text


def test_rows_gather_gemm_is_declared_bound_and_refuses_bad_arguments_before_any_launch():
    assert 'gd_rows_gather_gemm_f32' in _lib.declared_symbols() and 'gd_rows_gather_gemm_f32' in _lib.PROTOTYPES
    L = _lib.lib()
    assert L.gd_abi_version() == 9
    p = ctypes.c_void_p(256).value            # never dereferenced: the checks come first
    q = p + 4096

    def call(inp=p, ld_in=32, n_in=300, idx=p, n_sel=8, w=p, d_in=32, d_out=32, out=q, ld_out=32):
        return L.gd_rows_gather_gemm_f32(inp, ld_in, n_in, idx, n_sel, w, d_in, d_out, None, 0, out, ld_out, None)
    assert call(inp=None) == 1 and b'gd_rows_gather_gemm_f32' in L.gd_last_error_string()
    assert call(idx=None) == 1 and call(w=None) == 1 and call(out=None) == 1
    assert call(out=p) == 2 and b'alias' in L.gd_last_error_string()                  # in == out
    assert call(n_in=0) == 2 and call(n_in=-1) == 2 and call(n_in=1 << 31) == 2
    assert call(n_sel=-1) == 2 and call(d_in=0) == 2 and call(d_out=0) == 2           # gd_rows_gemm_f32's own
    assert call(ld_in=31) == 2 and call(ld_out=31) == 2
    assert call(d_in=1028, ld_in=1028, d_out=20, ld_out=20) == 2                      # the scalar form's d_in <= 1024
    assert call(n_sel=0) == 0 and call(n_sel=0, n_in=0) == 0                          # nothing selected: no launch
