"""gnndelete_amd.negatives on the CPU: reference_draw (the numpy restatement of gd_negative_edges, the kernel's test oracle) holds
negative_sampling's contract, is a pure function of (seed, counter, slot), is uniform over the allowed pairs, survives the edge
shapes and the linear probe; the density precondition; the entry's argument checks."""
import functools

import numpy as np
import pytest
import torch

from gnndelete_amd import negatives as N

DRAWS = 200_000


@functools.lru_cache(maxsize=None)
def graph64():
    """n = 64, a random 25 % of the off-diagonal pairs excluded, the smallest and the largest possible keys among them
    -> (sorted keys int64, the boolean [n, n] table of allowed pairs)."""
    n = 64
    rng = np.random.default_rng(0)
    m = rng.random((n, n)) < 0.25
    m[0, 1] = m[n - 1, n - 2] = True
    np.fill_diagonal(m, False)
    keys = np.flatnonzero(m.ravel()).astype(np.int64)
    assert keys[0] == 1 and keys[-1] == 63 * 64 + 62
    allowed = ~m
    np.fill_diagonal(allowed, False)
    return keys, allowed


def assert_contract(out, n, keys, n_out):
    assert isinstance(out, torch.Tensor) and out.dtype == torch.int64 and tuple(out.shape) == (2, n_out)
    a, b = out[0].numpy(), out[1].numpy()
    assert ((a >= 0) & (a < n) & (b >= 0) & (b < n)).all()
    assert (a != b).all()
    assert not np.isin(a * n + b, keys).any()


def test_reference_draw_contract():
    keys, _ = graph64()
    out = N.reference_draw(keys, 64, 12345, 0, 1000)
    assert_contract(out, 64, keys, 1000)
    assert torch.equal(out, N.reference_draw(torch.from_numpy(keys), 64, 12345, 0, 1000))        # the same arguments, the same tensor
    assert torch.equal(N.reference_draw(keys, 64, 12345, 0, 10), out[:, :10])                   # slot i does not depend on n_out
    assert not torch.equal(out, N.reference_draw(keys, 64, 12345, 1, 1000))                     # the counter
    assert not torch.equal(out, N.reference_draw(keys, 64, 12346, 0, 1000))                     # the seed
    assert tuple(N.reference_draw(keys, 64, 1, 0, 0).shape) == (2, 0)


@pytest.mark.parametrize('seed,counter', [(12345, 0), (12345, 1), (7, 5)])
def test_reference_draw_is_uniform_over_the_allowed_pairs(seed, counter):
    """Pearson's statistic over the k allowed cells against the chi-square distribution's own mean k - 1 and standard
    deviation sqrt(2 (k - 1)): within 5 of them.  Fixed inputs: deterministic."""
    keys, allowed = graph64()
    out = N.reference_draw(keys, 64, seed, counter, DRAWS).numpy()
    cnt = np.bincount(out[0] * 64 + out[1], minlength=64 * 64)
    assert cnt[~allowed.ravel()].sum() == 0
    k = int(allowed.sum())
    assert 2900 < k < 3100
    expect = DRAWS / k
    chi2 = float(((cnt[allowed.ravel()] - expect) ** 2 / expect).sum())
    z = (chi2 - (k - 1)) / np.sqrt(2 * (k - 1))
    print(f'seed {seed} counter {counter}: {k} cells, chi2 {chi2:.1f}, z {z:+.2f}')
    assert abs(chi2 - (k - 1)) <= 5 * np.sqrt(2 * (k - 1))


def test_two_nodes_without_edges_yield_both_pairs():
    out = N.reference_draw(np.empty(0, dtype=np.int64), 2, 3, 0, 200)
    assert_contract(out, 2, np.empty(0, dtype=np.int64), 200)
    assert {tuple(p) for p in out.t().tolist()} == {(0, 1), (1, 0)}


def test_node_products_beyond_32_bits():
    n = 70_001
    keys = np.unique(np.random.default_rng(1).integers(0, n * n, 5000)).astype(np.int64)
    out = N.reference_draw(keys, n, 3, 0, 20_000)
    assert_contract(out, n, keys, 20_000)
    flat = out[0].numpy() * n + out[1].numpy()
    assert (flat > 2 ** 32).any() and flat.max() < n * n


def test_mulhi64_against_python_integers():
    rng = np.random.default_rng(2)
    a = rng.integers(0, 2 ** 64, 1000, dtype=np.uint64)
    for b in (1, 4, 64 * 64, 70_001 ** 2, (2 ** 31 - 1) ** 2):
        want = [(int(v) * b) >> 64 for v in a]
        assert N.mulhi64(a, b).tolist() == want
    assert int(N.mix64(np.uint64(0))) == 0xE220A8397B1DCDAF                                       # splitmix64's first output for seed 0


def test_the_probe_alone_holds_the_contract_and_terminates():
    n = 8
    rng = np.random.default_rng(3)
    off = np.array([a * n + b for a in range(n) for b in range(n) if a != b])
    keys = np.sort(rng.choice(off, n * n // 2 - n, replace=False)).astype(np.int64)           # with the diagonal: exactly half
    assert N.device_negatives_unsupported(keys.size, n) is None
    out = N.reference_draw(keys, n, 5, 0, 500, tries=0)
    assert_contract(out, n, keys, 500)
    assert torch.equal(out, N.reference_draw(keys, n, 5, 0, 500, tries=0))
    assert len({tuple(p) for p in out.t().tolist()}) > 8                                         # it starts from the slot's own candidate
    # a long run of excluded keys: node 0's whole row and node 1's row up to its last column
    n = 16
    run = np.array([k for k in range(2 * n - 1) if k // n != k % n], dtype=np.int64)
    out = N.reference_draw(run, n, 9, 2, 300, tries=0)
    assert_contract(out, n, run, 300)


def test_density_precondition():
    assert N.device_negatives_unsupported(0, 1) is not None                                      # one node: no pair at all
    assert N.device_negatives_unsupported(0, 2) is None
    for n in (3, 8, 50):
        assert N.device_negatives_unsupported(n * (n - 1), n) is not None                        # the complete graph
    assert N.device_negatives_unsupported(8 * 8 // 2 - 8, 8) is None                             # exactly half excluded
    assert N.device_negatives_unsupported(8 * 8 // 2 - 8 + 1, 8) is not None
    assert 'half' in N.device_negatives_unsupported(8 * 8 // 2 - 8 + 1, 8)
    with pytest.raises(ValueError, match='half'):
        N.reference_draw(np.arange(1, 3, dtype=np.int64), 2, 0, 0, 4)


def test_the_entry_validates_before_it_launches():
    """Argument errors come back from the host side of gd_negative_edges: no GPU needed."""
    from gnndelete_amd import _lib
    L = _lib.lib()
    assert L.gd_negative_edges(None, 0, 64, 1, None, 0, None, 0, None) == 0                      # n_out == 0: GD_OK, no launch
    assert L.gd_negative_edges(None, 0, 1, 1, None, 4, None, 4, None) == 2                       # GD_E_DIM: density
    assert L.gd_negative_edges(None, 56, 8, 1, None, 4, None, 4, None) == 2
    assert b'half' in L.gd_last_error_string()
    assert L.gd_negative_edges(None, 5, 64, 1, None, 4, None, 4, None) == 1                      # GD_E_NULL

