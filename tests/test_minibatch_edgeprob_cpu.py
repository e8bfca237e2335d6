"""The fused edge-probability batch step (--unlearning_model gnndelete --minibatch --fused_minibatch) without a GPU: every
verdict of fused_minibatch_edgeprob_unsupported on CPU-constructed models and optimizers, the flag, the refusals of
gd_edgeprob_batch_loss_f32 that come before any launch, and the rule of the decoded list against the loop's `lower` mask."""
import ctypes
from types import SimpleNamespace

import pytest
import torch

from gnndelete_amd import _lib
from gnndelete_amd.framework import models as M
from gnndelete_amd.framework.training_args import apply_overrides, build_parser
from gnndelete_amd.minibatch import fused_minibatch_edgeprob_unsupported

ARGS = SimpleNamespace(unlearning_model='gnndelete', minibatch=True, fused_minibatch=True)
MASK = torch.zeros(10, dtype=torch.bool)


def decoded_candidates(src, dst):
    """The rule of the batch's decoded list (gd_edgeprob_batch_loss_f32), restated on plain sequences: the candidates that
    count are those with src < dst, each at its own place.  -> the positions kept."""
    return [c for c, (a, b) in enumerate(zip(src, dst)) if a < b]


def _model(gnn, h=16, o=8):
    cls = {'gcn': M.GCNDelete, 'gat': M.GATDelete, 'gin': M.GINDelete}[gnn]
    return cls(SimpleNamespace(in_dim=12, hidden_dim=h, out_dim=o), MASK, MASK)


def _dels(m):
    return [m.deletion1.deletion_weight, m.deletion2.deletion_weight]


def _adam(m, **kw):
    return torch.optim.Adam(_dels(m), lr=1e-3, **kw)


@pytest.mark.parametrize('gnn', ['gcn', 'gat'])
def test_gcn_and_gat_with_one_plain_adam_apply(gnn):
    m = _model(gnn)
    assert fused_minibatch_edgeprob_unsupported(m, ARGS, _adam(m)) is None
    # the optimizer delete_gnn.py builds: one group with weight_decay 0.0
    opt = torch.optim.Adam([{'params': _dels(m), 'weight_decay': 0.0}], lr=1e-3)
    assert fused_minibatch_edgeprob_unsupported(m, ARGS, opt) is None


def test_every_reason(monkeypatch):
    m = _model('gcn')
    gin = _model('gin')
    reason = fused_minibatch_edgeprob_unsupported(gin, ARGS, _adam(gin))
    assert reason == 'no fused edge-probability batch step for the GINDelete backbone (GCN and GAT only)'
    plain = M.GCN(SimpleNamespace(in_dim=12, hidden_dim=16, out_dim=8))
    assert 'GCN backbone' in fused_minibatch_edgeprob_unsupported(plain, ARGS, torch.optim.Adam(plain.parameters(), lr=1e-3))
    for um in ('gnndelete_kld', 'gnndelete_ablation_random', 'gnndelete_ablation_locality'):
        args = SimpleNamespace(unlearning_model=um, minibatch=True, fused_minibatch=True)
        assert fused_minibatch_edgeprob_unsupported(m, args, _adam(m)) == f'--unlearning_model {um} is not the MSE loss'
    not_one_adam = 'the optimizer is not one plain torch.optim.Adam'
    cases = {
        'sgd': torch.optim.SGD(_dels(m), lr=1e-3),
        'two optimizers': [torch.optim.Adam(_dels(m)[:1], lr=1e-3), torch.optim.Adam(_dels(m)[1:], lr=1e-3)],
        'two groups': torch.optim.Adam([{'params': _dels(m)[:1]}, {'params': _dels(m)[1:]}], lr=1e-3),
        'weight decay': _adam(m, weight_decay=5e-4),
        'amsgrad': _adam(m, amsgrad=True),
        'maximize': _adam(m, maximize=True),
    }
    for key, opt in cases.items():
        assert fused_minibatch_edgeprob_unsupported(m, ARGS, opt) == not_one_adam, key
    not_the_dels = 'the optimizer does not hold exactly the two Del weights'
    assert fused_minibatch_edgeprob_unsupported(m, ARGS, torch.optim.Adam(m.parameters(), lr=1e-3)) == not_the_dels
    assert fused_minibatch_edgeprob_unsupported(m, ARGS, torch.optim.Adam(_dels(m)[:1], lr=1e-3)) == not_the_dels
    odd = _model('gat', h=16, o=6)
    assert fused_minibatch_edgeprob_unsupported(odd, ARGS, _adam(odd)) == 'widths 16 / 6 (multiples of 4 up to 1024)'
    import torch.distributed as dist
    monkeypatch.setattr(dist, 'is_initialized', lambda: True)
    monkeypatch.setattr(dist, 'get_world_size', lambda *a, **k: 2)
    monkeypatch.setattr(dist, 'get_rank', lambda *a, **k: 0)
    assert fused_minibatch_edgeprob_unsupported(m, ARGS, _adam(m)) == 'torch.distributed with more than one rank'


def test_flag_parses_with_the_edge_probability_trainer_and_names_both_trainers():
    got = vars(apply_overrides(build_parser().parse_args(['--unlearning_model', 'gnndelete', '--minibatch', '--fused_minibatch'])))
    assert got['fused_minibatch'] is True and got['minibatch'] is True and got['unlearning_model'] == 'gnndelete'
    assert vars(apply_overrides(build_parser().parse_args(['--unlearning_model', 'gnndelete'])))['fused_minibatch'] is False
    from gnndelete_amd.framework import training_args as TA
    (text,) = [help_ for name, _, _, help_ in TA.FLAGS + TA.EXTRA_FLAGS if name == 'fused_minibatch']
    assert 'gnndelete_nodeemb and gnndelete trainers' in text


def test_decoded_list_keeps_what_the_lower_mask_keeps():
    """The loop: lower = e_sdf[0] < e_sdf[1]; row, col = e_sdf[0][lower], e_sdf[1][lower].  The decoded list keeps the same
    candidates in the same order: self loops and src > dst drop out, duplicates stay, each at its own place."""
    src = [3, 5, 5, 2, 9, 4, 4, 4, 0, 7, 7, 1]
    dst = [8, 5, 1, 6, 9, 7, 7, 2, 0, 4, 9, 1]
    e_sdf = torch.tensor([src, dst])
    lower = e_sdf[0] < e_sdf[1]
    keep = decoded_candidates(src, dst)
    assert keep == lower.nonzero().flatten().tolist() == [0, 3, 5, 6, 10]
    assert [src[c] for c in keep] == e_sdf[0][lower].tolist() and [dst[c] for c in keep] == e_sdf[1][lower].tolist()
    # the device list holds every candidate, (-1, -1) in place of one that does not count: compacting it gives the loop's list
    dec = [(a, b) if c in set(keep) else (-1, -1) for c, (a, b) in enumerate(zip(src, dst))]
    assert [e for e in dec if e != (-1, -1)] == list(zip(e_sdf[0][lower].tolist(), e_sdf[1][lower].tolist()))
    assert decoded_candidates([], []) == [] and decoded_candidates([2, 2], [2, 1]) == []


def test_batch_loss_refuses_bad_arguments_before_any_launch():
    L = _lib.lib()
    p = ctypes.c_void_p(256).value            # never dereferenced: the checks come first

    def call(z=p, zo=p, ld=8, d=8, k=4, n_c=4, pos=p, cand=p, inc=None, ld_dec=12):
        return L.gd_edgeprob_batch_loss_f32(z, ld, 8, zo, 8, 8, d, pos, 4, p, 4, k, cand, p, n_c, 0.5, 0.5, p, ld_dec, p, p, inc, None,
                                            None, None, None, 0, p, None)
    assert call(z=None) == 1 and b'gd_edgeprob_batch_loss_f32' in L.gd_last_error_string()
    assert call(zo=None) == 1 and call(pos=None) == 1 and call(cand=None) == 1 and call(inc=p) == 1
    assert call(k=-1) == 2 and call(n_c=-1) == 2 and call(d=6, ld=6) == 2 and call(ld=10) == 2 and call(ld_dec=11) == 2
    assert call(z=p + 4) == 3
    assert L.gd_edgeprob_batch_loss_workspace(-1, 0, 8) == -1 and L.gd_edgeprob_batch_loss_workspace(0, -1, 8) == -1
    assert L.gd_edgeprob_batch_loss_workspace(4, 4, 6) == -1 and L.gd_edgeprob_batch_loss_workspace(1 << 28, 0, 8) == -1
    assert L.gd_edgeprob_batch_loss_workspace(0, 0, 8) >= 4 and L.gd_edgeprob_batch_loss_workspace(1000, 5000, 64) >= 6000
