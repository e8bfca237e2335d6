"""--device_negatives without a GPU: the flag, the fallback reasons, the declarations of the two incidence entries, their size
queries and host-side refusals, and the list order the merge kernels rely on - node v's part of a stable sort of cat(e0, e1)
over [fixed | variable] edges is [fixed e0 = v | variable e0 = v | fixed e1 = v | variable e1 = v], each by ascending edge."""
import numpy as np
import torch


def test_the_flag_parses_and_defaults_off():
    from gnndelete_amd.framework.training_args import EXTRA_FLAGS, build_parser
    assert 'device_negatives' in [f[0] for f in EXTRA_FLAGS]
    p = build_parser()
    assert p.parse_args([]).device_negatives is False
    a = p.parse_args(['--device_negatives', '--fused_backbone', '--random_seed', '7'])
    assert a.device_negatives is True and a.fused_backbone is True and a.random_seed == 7
    assert not hasattr(build_parser(extra=False).parse_args([]), 'device_negatives')


def test_every_fallback_has_its_reason():
    from gnndelete_amd.negatives import device_negatives_fallback, device_negatives_unsupported
    assert device_negatives_fallback('fused_backbone', False, False) == '--fused_backbone is missing or fell back'
    assert device_negatives_fallback('fused_edgeprob', False, True) == '--fused_edgeprob is missing or fell back'
    assert device_negatives_fallback('fused_backbone', True, True, 10, 100) == 'negative_sampling has been replaced'
    assert device_negatives_fallback('fused_backbone', True, False, 10, 100) is None
    dense = device_negatives_fallback('fused_backbone', True, False, 41, 10)
    assert dense == device_negatives_unsupported(41, 10) == '41 positive pairs and 10 self loops exclude more than half of the 10^2 node pairs'
    assert dense.count('\n') == 0
    # the bound itself: 2 (keys + n) <= n^2
    assert device_negatives_fallback('x', True, False, 40, 10) is None and device_negatives_fallback('x', True, False, 41, 10) is not None
    assert device_negatives_fallback('x', True, False, 49, 11) is None and device_negatives_fallback('x', True, False, 50, 11) is not None


def test_trainer_logs_the_reason(capsys, tmp_path):
    """Trainer._device_negative_keys on the host: nothing without the flag; with it, the reason is printed once and logged."""
    from types import SimpleNamespace
    from gnndelete_amd.framework import graph_utils as GU
    from gnndelete_amd.framework.trainer.base import Trainer
    edges = torch.tensor([[0, 1, 2, 3], [1, 2, 3, 4]])
    tr = Trainer(SimpleNamespace(dataset='synth-tiny', unlearning_model='original', checkpoint_dir=str(tmp_path)))
    assert tr._device_negative_keys(SimpleNamespace(), True, GU.negative_sampling, edges, 50) is None and 'negatives' not in tr.trainer_log
    on = SimpleNamespace(device_negatives=True)
    assert tr._device_negative_keys(on, False, GU.negative_sampling, edges, 50) is None
    assert tr.trainer_log['negatives'] == '--fused_backbone is missing or fell back'
    assert tr._device_negative_keys(on, True, lambda *a: None, edges, 50) is None
    assert tr.trainer_log['negatives'] == 'negative_sampling has been replaced'
    assert tr._device_negative_keys(on, True, GU.negative_sampling, edges, 3, 'fused_edgeprob') is None
    assert 'exclude more than half' in tr.trainer_log['negatives']
    out = capsys.readouterr().out
    assert out.count('--device_negatives: ') == 3 and out.count('drawing the negatives on the host') == 3
    keys = tr._device_negative_keys(on, True, GU.negative_sampling, edges, 50)
    assert tr.trainer_log['negatives'] == 'device' and keys.tolist() == [1, 52, 103, 154]
    assert capsys.readouterr().out == ''


def test_the_entries_are_declared_bound_and_refuse_on_the_host():
    from gnndelete_amd import _lib
    names = ['gd_edge_incidence_fixed', 'gd_edge_incidence_fixed_bytes', 'gd_edge_incidence_update', 'gd_edge_incidence_update_workspace']
    declared = _lib.declared_symbols()
    assert all(n in declared and n in _lib.PROTOTYPES for n in names)
    assert sorted(declared) == sorted(_lib.PROTOTYPES)
    L = _lib.lib()
    assert L.gd_abi_version() == 9
    # sizes: the image holds inc_ptr (int64 [n + 1]), the source counts (int32 [n], padded to 8 bytes) and three int32 [2 F] arrays
    assert L.gd_edge_incidence_fixed_bytes(10, 4) == 8 * 11 + 4 * 10 + 24 * 4
    assert L.gd_edge_incidence_fixed_bytes(11, 0) == 8 * 12 + 4 * 12
    assert L.gd_edge_incidence_fixed_bytes(-1, 0) == 0 and L.gd_edge_incidence_update_workspace(5, -1) == 0
    assert L.gd_edge_incidence_update_workspace(10, 6) >= 4 * (2 * 10 + 4 * 6) + 8 * 2
    assert L.gd_edge_incidence_update_workspace(10, 6) >= L.gd_edge_incidence_update_workspace(10, 4)
    # argument errors come back before any launch: no GPU needed
    big = 1 << 40
    assert L.gd_edge_incidence_fixed(None, None, 0, 5, None, big, None, big, None) == 1
    assert b'gd_edge_incidence_fixed' in L.gd_last_error_string()
    assert L.gd_edge_incidence_update(None, None, None, 0, 0, 5, None, None, None, None, big, None) == 1
    assert b'gd_edge_incidence_update' in L.gd_last_error_string()
    fake = 4096                                                  # a non-null, aligned address that is never dereferenced
    assert L.gd_edge_incidence_fixed(fake, fake, 4, 0, fake, big, fake, big, None) == 2                    # n_nodes = 0
    assert L.gd_edge_incidence_fixed(fake, fake, 4, 10, fake, L.gd_edge_incidence_fixed_bytes(10, 4) - 1, fake, big, None) == 4
    assert L.gd_edge_incidence_fixed(fake, fake, 4, 10, fake, big, fake, L.gd_edge_incidence_update_workspace(10, 4) - 1, None) == 4
    assert L.gd_edge_incidence_fixed(None, fake, 4, 10, fake, big, fake, big, None) == 1
    assert L.gd_edge_incidence_update(fake, fake, fake, 7, 6, 10, fake, fake, fake, fake, big, None) == 2   # n_fixed > n_edges
    assert L.gd_edge_incidence_update(fake, fake, fake, 4, 6, 0, fake, fake, fake, fake, big, None) == 2
    assert L.gd_edge_incidence_update(fake, fake, fake, 4, 6, 10, fake, fake, fake, fake,
                                      L.gd_edge_incidence_update_workspace(10, 6) - 1, None) == 4
    assert L.gd_edge_incidence_update(fake, fake, fake, 4, 6, 10, fake, None, fake, fake, big, None) == 1
    assert L.gd_edge_incidence_update(fake + 4, fake, fake, 4, 6, 10, fake, fake, fake, fake, big, None) == 3   # GD_E_ALIGN


def _graphs():
    """The graphs of tests/test_edgeprob_kernels_gpu.py::_incidence_graphs, plus endpoints outside [0, n)."""
    g = torch.Generator().manual_seed(3)
    out = [(1, torch.zeros(2, 5, dtype=torch.long)), (65, torch.tensor([[3, 64], [64, 3]])), (65, torch.randint(0, 65, (2, 131), generator=g))]
    e = torch.randint(0, 4000, (2, 1777), generator=g)
    e[0, 100:300] = 17
    e[1, 250:400] = 17
    e[:, 500:520] = torch.arange(20).repeat(2, 1) + 30
    e[:, 600:610] = e[:, 590:600]
    out.append((5000, e))
    bad = torch.randint(0, 300, (2, 400), generator=g)
    for base in (10, 210):
        bad[0, base], bad[0, base + 1], bad[1, base + 2], bad[1, base + 3] = -1, 300, -1, 300
    out.append((300, bad))
    return [(n, e.numpy()) for n, e in out]


def _four_part_lists(e0, e1, n_fixed, n):
    """(inc_ptr, other, src_edge) by the order the kernels build: per node, fixed source entries, variable source entries, fixed
    destination entries, variable destination entries - each by ascending edge index; edges with a bad endpoint left out."""
    ok = (e0 >= 0) & (e0 < n) & (e1 >= 0) & (e1 < n)
    edge = np.arange(e0.size)
    parts = [(ok & (edge < n_fixed), 0), (ok & (edge >= n_fixed), 0), (ok & (edge < n_fixed), 1), (ok & (edge >= n_fixed), 1)]
    inc_ptr, other, src = [0], [], []
    for v in range(n):
        for mask, side in parts:
            mine = edge[mask & ((e1 if side else e0) == v)]     # ascending edge index
            other += list((e0 if side else e1)[mine])
            src += list(mine)
        inc_ptr.append(len(src))
    return np.array(inc_ptr), np.array(other, dtype=np.int64), np.array(src, dtype=np.int64)


def test_the_four_part_order_is_the_stable_sort():
    for n, e in _graphs():
        e0, e1 = e[0], e[1]
        M = e0.size
        ok = (e0 >= 0) & (e0 < n) & (e1 >= 0) & (e1 < n)
        p = np.arange(2 * M)[np.concatenate([ok, ok])]
        order = p[np.argsort(np.concatenate([e0, e1])[p], kind='stable')]
        want_src = order % M
        want_other = np.where(order >= M, e0[want_src], e1[want_src])
        want_ptr = np.searchsorted(np.sort(np.concatenate([e0, e1])[p]), np.arange(n + 1))
        mid = M // 2 + (1 if (M // 2) % 64 == 0 else 0)
        for n_fixed in sorted({0, min(1, M), mid, M - 1, M}):
            ptr, other, src = _four_part_lists(e0, e1, n_fixed, n)
            assert np.array_equal(ptr, want_ptr) and np.array_equal(src, want_src) and np.array_equal(other, want_other), (n, n_fixed)
