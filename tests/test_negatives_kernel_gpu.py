"""gd_negative_edges (csrc/negatives.hip) against its numpy restatement gnndelete_amd.negatives.reference_draw, bit for bit: the
contract graph at block edges, the smallest graph, node products beyond 32 bits, a hub whose row of keys is full but for one
column, the counter forms, a wider row pitch; the return codes; empty keys."""
import functools

import numpy as np
import pytest
import torch

from gnndelete_amd import negatives as N

pytestmark = pytest.mark.gpu
SENTINEL = -7


@functools.lru_cache(maxsize=None)
def graph64():
    n = 64
    rng = np.random.default_rng(0)
    m = rng.random((n, n)) < 0.25
    m[0, 1] = m[n - 1, n - 2] = True
    np.fill_diagonal(m, False)
    return np.flatnonzero(m.ravel()).astype(np.int64)


@functools.lru_cache(maxsize=None)
def graph_big():
    n = 70_001
    return n, np.unique(np.random.default_rng(1).integers(0, n * n, 5000)).astype(np.int64)


@functools.lru_cache(maxsize=None)
def graph_hub():
    """n = 40: node 3's row of keys is full except column 17 (and its own diagonal cell), a few other edges around it."""
    n = 40
    row = [3 * n + b for b in range(n) if b not in (3, 17)]
    rng = np.random.default_rng(4)
    other = [int(k) for k in rng.integers(0, n * n, 60) if k // n != k % n]
    return n, np.unique(np.array(row + other, dtype=np.int64))


def dev(keys):
    return torch.from_numpy(keys).cuda()


def same(keys, n, seed, counter, n_out):
    got = N.device_negative_edges(dev(keys), n, seed, counter, n_out)
    want = N.reference_draw(keys, n, seed, 0 if counter is None else counter, n_out)
    assert got.dtype == torch.int64 and tuple(got.shape) == (2, n_out)
    assert torch.equal(got.cpu(), want)
    return got


@pytest.mark.parametrize('n_out', [1, 63, 64, 65, 257, 5000])
def test_kernel_equals_restatement_on_the_contract_graph(n_out):
    got = same(graph64(), 64, 12345, 0, n_out).cpu()
    assert (got[0] != got[1]).all() and not np.isin((got[0] * 64 + got[1]).numpy(), graph64()).any()


def test_kernel_equals_restatement_on_two_nodes():
    got = same(np.empty(0, dtype=np.int64), 2, 3, 0, 300)
    assert {tuple(p) for p in got.t().tolist()} == {(0, 1), (1, 0)}


def test_kernel_equals_restatement_beyond_32_bits():
    n, keys = graph_big()
    got = same(keys, n, 3, 0, 20_000).cpu()
    assert ((got[0] * n + got[1]) > 2 ** 32).any()


def test_kernel_equals_restatement_on_a_hub_row():
    n, keys = graph_hub()
    got = same(keys, n, 11, 1, 6000).cpu()
    from_hub = got[1][got[0] == 3]
    assert from_hub.numel() > 0 and bool((from_hub == 17).all())


def test_counter_forms():
    keys = graph64()
    null = same(keys, 64, 99, None, 500)
    zero = N.device_negative_edges(dev(keys), 64, 99, torch.zeros(1, dtype=torch.int64, device='cuda'), 500)
    three = same(keys, 64, 99, 3, 500)
    assert torch.equal(null, zero) and not torch.equal(null, three)
    counter = torch.tensor([3], dtype=torch.int64, device='cuda')
    assert torch.equal(N.device_negative_edges(dev(keys), 64, 99, counter, 500), three)
    assert int(counter) == 3                                                                     # read, never written
    big_seed = 2 ** 64 - 5
    same(keys, 64, big_seed, 2 ** 40 + 1, 100)


def test_a_wider_row_pitch_leaves_the_tail_alone():
    keys = graph64()
    out = torch.full((2, 300), SENTINEL, dtype=torch.int64, device='cuda')
    got = N.device_negative_edges(dev(keys), 64, 5, 2, 257, out=out)
    assert got.data_ptr() == out.data_ptr() and tuple(got.shape) == (2, 257)
    assert torch.equal(got.cpu(), N.reference_draw(keys, 64, 5, 2, 257))
    assert bool((out[:, 257:] == SENTINEL).all())


def test_return_codes():
    from gnndelete_amd import _lib
    L = _lib.lib()
    keys = dev(graph64())
    out = torch.full((2, 8), SENTINEL, dtype=torch.int64, device='cuda')
    s = _lib.stream_ptr(out.device)
    assert L.gd_negative_edges(keys.data_ptr(), keys.numel(), 64, 1, None, 0, out.data_ptr(), 8, s) == 0         # GD_OK, no launch
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())
    complete = torch.arange(8 * 8, dtype=torch.int64, device='cuda')
    assert L.gd_negative_edges(complete.data_ptr(), 56, 8, 1, None, 8, out.data_ptr(), 8, s) == 2                # GD_E_DIM
    assert L.gd_negative_edges(None, 0, 1, 1, None, 8, out.data_ptr(), 8, s) == 2
    assert L.gd_negative_edges(None, keys.numel(), 64, 1, None, 8, out.data_ptr(), 8, s) == 1                    # GD_E_NULL
    assert L.gd_negative_edges(keys.data_ptr(), keys.numel(), 64, 1, None, 8, None, 8, s) == 1
    assert L.gd_negative_edges(keys.data_ptr(), keys.numel(), 64, 1, None, 8, out.data_ptr(), 7, s) == 2         # ld_out < n_out
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())
    with pytest.raises(_lib.GnnDeleteHipError):
        N.device_negative_edges(complete[:56], 8, 1, 0, 8)


def test_empty_keys_reject_only_self_loops():
    from gnndelete_amd import _lib
    n, n_out = 9, 4000
    out = torch.empty(2, n_out, dtype=torch.int64, device='cuda')
    _lib.check(_lib.lib().gd_negative_edges(None, 0, n, 21, None, n_out, out.data_ptr(), n_out, _lib.stream_ptr(out.device)))
    assert torch.equal(out.cpu(), N.reference_draw(np.empty(0, dtype=np.int64), n, 21, 0, n_out))
    assert bool((out[0] != out[1]).all())
    assert len({tuple(p) for p in out.t().tolist()}) == n * (n - 1)                              # every off-diagonal pair turns up
    assert torch.equal(N.device_negative_edges(None, n, 21, None, n_out, out=torch.empty_like(out)), out)
