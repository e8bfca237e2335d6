"""The fused GraphSAINT batch step's ABI entries and CLI flag, without a GPU."""
import ctypes

from gnndelete_amd import _lib
from gnndelete_amd.framework.training_args import apply_overrides, build_parser


def _err():
    return _lib.lib().gd_last_error_string().decode()


def test_batch_entries_reject_null_arguments():
    L = _lib.lib()
    args = [None] * 3 + [100, None, 10, None, 1, None, 64] + [None] * 9 + [None, 1 << 20, None]
    assert L.gd_induced_subgraph(*args) == 1 and 'gd_induced_subgraph' in _err()
    assert L.gd_batch_csr(None, None, 10, 5, 0, None, None, None, None, None, None, None, None, 1 << 20, None) == 1
    assert 'gd_batch_csr' in _err()
    assert L.gd_batch_loss_terms(None, 4, None, 4, 4, None, 0, 5, 1.0, 1.0, None, None, None, None, None, 1 << 20, None) == 1
    assert 'gd_batch_loss_terms' in _err()


def test_batch_entries_reject_bad_sizes():
    L = _lib.lib()
    fake = ctypes.c_void_p(256)           # never dereferenced: the size checks come first
    p = fake.value
    args = [p] * 3 + [100, p, 0, p, 1, p, 64] + [p] * 9 + [p, 1 << 20, None]
    assert L.gd_induced_subgraph(*args) == 2           # n_b = 0
    args[7] = 0
    args[5] = 10
    assert L.gd_induced_subgraph(*args) == 2           # generation 0
    assert L.gd_batch_csr(p, p, 10, 5, 3, p, p, p, p, p, p, p, p, 1 << 20, None) == 2   # mode 3
    assert L.gd_batch_csr(p, p, 10, 5, 0, p, p, p, p, p, p, p, p, 16, None) == 4        # workspace too small
    assert L.gd_induced_subgraph_workspace(-1) < 0 and L.gd_batch_csr_workspace(0, 10) < 0
    assert L.gd_batch_loss_terms_workspace(0, 10) < 0 and L.gd_batch_loss_terms_workspace(10, 0) > 0


def test_fused_minibatch_flag_parses_and_defaults_off():
    assert vars(apply_overrides(build_parser().parse_args([])))['fused_minibatch'] is False
    got = vars(apply_overrides(build_parser().parse_args(['--minibatch', '--fused_minibatch'])))
    assert got['fused_minibatch'] is True and got['minibatch'] is True
