"""--device_subsets without a GPU: the numpy restatement of the subset stream (gnndelete_amd/subsets.reference_draw, the kernels'
CPU oracle) - every row distinct and inside the pool, a permutation at k = m, dependence on seed, draw and subset, the widest
domain (bits = 32) and the worst walk ratio (m = 2^16 + 1) - its uniformity beside torch.randperm(m)[:k] under the same
statistics and the same cap, the two entries' declarations and host-side refusals, every reason of
device_subsets_unsupported, and the flag.

Uniformity.  A statistic is chi-squared over cells that are equally likely under a uniform draw, z = (chi2 - dof) /
sqrt(2 dof) its normal approximation, and the cap is |z| <= 5.  Ordered pairs (e(b, 0), e(b, 1)): m (m - 1) cells, B = 100 m
(m - 1) subsets, dof = m (m - 1) - 1.  Inclusion counts: element i is in c_i of B subsets, expected B k / m with variance
B k / m (1 - k / m); sum (c_i - B k / m)^2 / variance over the m elements has m - 1 degrees of freedom (the counts add up to
B k).  Both draws use fixed seeds, so the test is deterministic.  Seeds tried: the stream with seed = 1, draw = 0 and
torch.manual_seed(0) - the first pair tried; both pass at every shape, none was replaced."""
import functools

import numpy as np
import pytest
import torch

Z_CAP = 5.0
STREAM_SEED, TORCH_SEED = 1, 0

SHAPES = [(32, 32, 5), (33, 1, 50), (65, 64, 20), (65536, 513, 3), (65537, 3000, 3), (2 ** 31 - 1, 4096, 2)]      # (m, k, B)


@functools.lru_cache(maxsize=None)
def _drawn(m, k, n_sub, seed=7, draw=0):
    from gnndelete_amd.subsets import reference_draw
    out = reference_draw(seed, draw, n_sub, k, m)
    out.setflags(write=False)
    return out


# ---------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize('m,k,n_sub', SHAPES)
def test_rows_are_distinct_in_range_and_repeatable(m, k, n_sub):
    from gnndelete_amd.subsets import reference_draw
    rows = _drawn(m, k, n_sub)
    assert rows.dtype == np.int64 and rows.shape == (n_sub, k)
    assert int(rows.min()) >= 0 and int(rows.max()) < m
    assert all(np.unique(r).size == k for r in rows)
    assert np.array_equal(reference_draw(7, 0, n_sub, k, m), rows)              # a second call
    # a pure function of (seed, draw, b, j, m): fewer subsets or members are a corner of the same matrix
    assert np.array_equal(reference_draw(7, 0, max(n_sub - 1, 1), max(k // 2, 1), m), rows[:max(n_sub - 1, 1), :max(k // 2, 1)])


@pytest.mark.parametrize('m', [32, 33, 64, 65, 1000, 4099])
def test_k_equal_m_is_a_permutation(m):
    rows = _drawn(m, m, 3)
    assert all(np.array_equal(np.sort(r), np.arange(m)) for r in rows)
    assert not np.array_equal(rows[0], rows[1]) and not np.array_equal(rows[0], np.arange(m))


@pytest.mark.parametrize('m,k', [(33, 8), (65537, 3000), (2 ** 31 - 1, 4096)])
def test_the_result_depends_on_seed_draw_and_subset(m, k):
    from gnndelete_amd.subsets import reference_draw
    base = _drawn(m, k, 3)
    assert not np.array_equal(base[0], base[1]) and not np.array_equal(base[1], base[2])
    assert not np.array_equal(reference_draw(8, 0, 3, k, m), base)
    assert not np.array_equal(reference_draw(7, 1, 3, k, m), base)
    assert not np.array_equal(reference_draw(7 + (1 << 40), 0, 3, k, m), base)     # the seed's upper half counts too
    assert np.array_equal(reference_draw(7 + (1 << 64), 0, 3, k, m), base)         # 64-bit seeds, wrapping


def test_domain_widths():
    from gnndelete_amd.subsets import half_bits
    assert [half_bits(m) for m in (32, 33, 64, 65, 257, 65536, 65537, 2 ** 31 - 1)] == [3, 3, 3, 4, 5, 8, 9, 16]
    # bits = 32: (L << 16) | R stays below 2^32, and members reach the top of the pool's range
    wide = _drawn(2 ** 31 - 1, 4096, 2)
    assert int(wide.max()) > 2 ** 30 and int(wide.max()) < 2 ** 31 - 1 + 1
    # m = 2^16 + 1 in an 18-bit domain: almost three of four outputs are walked past, and the rows are still what they should be
    worst = _drawn(65537, 3000, 3)
    assert int(worst.max()) > 60000 and int(worst.min()) < 5000


def test_a_scalar_restatement_agrees():
    """The stream once more, one member at a time in Python integers: nothing of the vectorised bookkeeping is shared."""
    from gnndelete_amd.negatives import mix64

    def fmix(x):
        x ^= x >> 16
        x = x * 0x85ebca6b & 0xFFFFFFFF
        x ^= x >> 13
        x = x * 0xc2b2ae35 & 0xFFFFFFFF
        return x ^ (x >> 16)

    def mix(z):
        return int(mix64(np.uint64(z & 0xFFFFFFFFFFFFFFFF)))

    def member(seed, draw, b, j, m):
        bits = max(6, (m - 1).bit_length())
        bits += bits & 1
        h = bits // 2
        mask = (1 << h) - 1
        kb = mix(mix(seed ^ mix(draw)) + b)
        keys = [mix(kb + r) & 0xFFFFFFFF for r in range(12)]
        v = j
        while True:
            left, right = v >> h, v & mask
            for r in range(12):
                left, right = right, left ^ (fmix(right ^ keys[r]) & mask)
            v = (left << h) | right
            if v < m:
                return v
    for m, k, n_sub in [(32, 32, 2), (65, 64, 2), (65537, 40, 3), (2 ** 31 - 1, 40, 2)]:
        rows = _drawn(m, k, n_sub)
        assert rows.tolist() == [[member(7, 0, b, j, m) for j in range(k)] for b in range(n_sub)]


# ---------------------------------------------------------------------------------------------- uniformity
def _z_pairs(rows, m):
    rows = np.asarray(rows, dtype=np.int64)
    n_sub = rows.shape[0]
    cells = np.bincount(rows[:, 0] * m + rows[:, 1], minlength=m * m).reshape(m, m).astype(np.float64)
    assert cells.trace() == 0                                    # no pair (i, i): the members are distinct
    off = ~np.eye(m, dtype=bool)
    expected = n_sub / (m * (m - 1))
    chi2, dof = float(((cells[off] - expected) ** 2 / expected).sum()), m * (m - 1) - 1
    return (chi2 - dof) / np.sqrt(2.0 * dof)


def _z_inclusion(rows, m):
    rows = np.asarray(rows, dtype=np.int64)
    n_sub, k = rows.shape
    counts = np.bincount(rows.reshape(-1), minlength=m).astype(np.float64)
    mean = n_sub * k / m
    chi2, dof = float(((counts - mean) ** 2).sum() / (mean * (1.0 - k / m))), m - 1
    return (chi2 - dof) / np.sqrt(2.0 * dof)


def _randperm_rows(m, k, n_sub):
    """torch.randperm(m)[:k], n_sub times, under a fixed torch.manual_seed; the caller's generator state is put back."""
    state = torch.get_rng_state()
    torch.manual_seed(TORCH_SEED)
    rows, perm = np.empty((n_sub, k), dtype=np.int64), torch.empty(m, dtype=torch.int64)
    view = perm.numpy()
    for b in range(n_sub):
        torch.randperm(m, out=perm)
        rows[b] = view[:k]
    torch.set_rng_state(state)
    return rows


@pytest.mark.parametrize('m', [33, 64, 65, 257])
def test_ordered_pairs_are_uniform(m):
    from gnndelete_amd.subsets import reference_draw
    n_sub = 100 * m * (m - 1)
    z = _z_pairs(reference_draw(STREAM_SEED, 0, n_sub, 2, m), m)
    z_ref = _z_pairs(_randperm_rows(m, 2, n_sub), m)
    print(f'pairs m={m} B={n_sub}: stream z = {z:+.3f}, torch.randperm z = {z_ref:+.3f}')
    assert abs(z_ref) <= Z_CAP                                   # (a cap the reference draw fails would be a wrong test)
    assert abs(z) <= Z_CAP


@pytest.mark.parametrize('m,k,n_sub', [(1000, 37, 5000), (4099, 513, 500), (70001, 3000, 500)])
def test_inclusion_counts_are_uniform(m, k, n_sub):
    from gnndelete_amd.subsets import reference_draw
    z = _z_inclusion(reference_draw(STREAM_SEED, 0, n_sub, k, m), m)
    z_ref = _z_inclusion(_randperm_rows(m, k, n_sub), m)
    print(f'inclusion m={m} k={k} B={n_sub}: stream z = {z:+.3f}, torch.randperm z = {z_ref:+.3f}')
    assert abs(z_ref) <= Z_CAP
    assert abs(z) <= Z_CAP


# ---------------------------------------------------------------------------------------------- ABI, refusals, the flag
def test_the_entries_are_declared_bound_and_refuse_on_the_host():
    from gnndelete_amd import _lib
    names = ['gd_subset_rank_metrics_drawn', 'gd_subset_draw']
    declared = _lib.declared_symbols()
    assert all(n in declared and n in _lib.PROTOTYPES for n in names)
    assert sorted(declared) == sorted(_lib.PROTOTYPES)
    with open(_lib.HEADER_PATH) as f:
        header = f.read()
    assert '#define GD_ABI_VERSION 9' in header and 'base.py:530-539' in header and 'base.py:263-268' in header
    L = _lib.lib()
    assert L.gd_abi_version() == 9
    assert all(hasattr(L, n) for n in names)                     # exported
    # argument errors come back before any launch: no GPU needed
    E_NULL, E_DIM, E_ALIGN, E_WS = 1, 2, 3, 4
    p = 256                                                      # any non-null, aligned value: refused before it is used

    def ranked(n_sub=2, k=4, m=40, n_ref=3, ptrs=p, ws=p, ws_bytes=1 << 20):
        return L.gd_subset_rank_metrics_drawn(ptrs, ptrs, ptrs, ptrs, 5, 0, n_sub, k, m, n_ref, ptrs, ptrs, ws, ws_bytes, None)
    for change in [dict(m=31, k=4), dict(m=31, k=31), dict(m=1, k=1), dict(k=41), dict(k=0), dict(k=-1), dict(n_ref=0), dict(n_ref=1 << 30),
                   dict(m=1 << 31), dict(n_sub=-1), dict(n_sub=1 << 31)]:
        assert ranked(**change) == E_DIM, change
        assert ranked(ptrs=None, ws=None, **change) == E_DIM, change
    assert ranked(m=31, k=4) == E_DIM and b'm=31' in L.gd_last_error_string()
    assert ranked(n_sub=0, ptrs=None, ws=None, ws_bytes=0) == 0                  # nothing to do: OK, no launch
    assert ranked(ptrs=None) == E_NULL and ranked(ws=None) == E_NULL
    assert ranked(ws=p + 4) == E_ALIGN
    need = L.gd_subset_rank_workspace(2, 40)
    assert need == 2 * 2 * 128 and ranked(ws_bytes=need - 1) == E_WS
    assert b'workspace of 511 bytes, 512 needed' in L.gd_last_error_string()
    assert ranked(m=32, k=32, ws_bytes=need - 1) == E_WS                         # (the smallest pool gets as far as the workspace)

    def drawn(n_sub=2, k=4, m=40, out=p, ld=4):
        return L.gd_subset_draw(5, 0, n_sub, k, m, out, ld, None)
    for change in [dict(m=31), dict(k=41), dict(k=0), dict(m=1 << 31), dict(n_sub=-1), dict(n_sub=1 << 31)]:
        assert drawn(**change) == E_DIM, change
    assert drawn(n_sub=0, out=None) == 0
    assert drawn(out=None) == E_NULL
    assert drawn(ld=3) == E_DIM and b'ld_out=3 below k=4' in L.gd_last_error_string()


def test_every_refusal_has_its_reason():
    from gnndelete_amd.subsets import device_subsets_unsupported, reference_draw
    assert device_subsets_unsupported(32, 32) is None and device_subsets_unsupported(32, 1) is None
    assert device_subsets_unsupported((1 << 31) - 1, 5) is None
    want = {
        (31, 4): 'a pool of 31 scores (the subset stream takes 32 and more)',
        (0, 0): 'a pool of 0 scores (the subset stream takes 32 and more)',
        (1 << 31, 10): f'a pool of {1 << 31} scores (below 2^31)',
        (100, 0): 'subsets of 0 positives (at least one)',
        (100, 101): 'subsets of 101 positives from a pool of 100',
    }
    for sizes, reason in want.items():
        assert device_subsets_unsupported(*sizes) == reason
    assert len(set(want.values())) == len(want) and all('\n' not in r for r in want.values())
    with pytest.raises(ValueError, match='a pool of 31 scores'):
        reference_draw(1, 0, 2, 4, 31)
    with pytest.raises(ValueError, match='subsets of 41 positives from a pool of 40'):
        reference_draw(1, 0, 2, 41, 40)


def test_wrappers_refuse_before_any_launch():
    from gnndelete_amd import subsets
    from gnndelete_amd.rankeval import subset_auc_ap_drawn
    with pytest.raises(ValueError, match='the scores are not on the GPU'):
        subset_auc_ap_drawn(torch.rand(4), torch.rand(40), 1, 0, 3, 4)
    with pytest.raises(ValueError, match='a pool of 31 scores'):
        subsets.draw(1, 0, 3, 4, 31)
    with pytest.raises(ValueError, match='expected int64'):
        subsets.draw(1, 0, 3, 4, 40, out=torch.empty(3, 4, dtype=torch.int64))       # a host tensor


def test_the_flag_parses_and_defaults_off():
    from gnndelete_amd.framework.training_args import EXTRA_FLAGS, build_parser
    assert 'device_subsets' in [f[0] for f in EXTRA_FLAGS]
    p = build_parser()
    assert p.parse_args([]).device_subsets is False
    a = p.parse_args(['--device_subsets', '--fused_validation'])
    assert a.device_subsets is True and a.fused_validation is True
    assert not hasattr(build_parser(extra=False).parse_args([]), 'device_subsets')


def test_without_the_pass_the_trainers_say_why(capsys, tmp_path):
    """evalpass.subset_draw on the host: nothing without the flag; with it 'device' or the reason, a reason printed once."""
    from types import SimpleNamespace
    from gnndelete_amd import evalpass
    from gnndelete_amd.framework.trainer.base import Trainer
    off = Trainer(SimpleNamespace(dataset='synth-tiny', unlearning_model='original', checkpoint_dir=str(tmp_path)))
    assert evalpass.subset_draw(off, None) is False and evalpass.subset_draw(off, 'x') is False and 'subset_draw' not in off.trainer_log
    tr = Trainer(SimpleNamespace(dataset='synth-tiny', unlearning_model='original', checkpoint_dir=str(tmp_path), device_subsets=True))
    assert evalpass.subset_draw(tr, '--fused_validation is missing') is False
    assert evalpass.subset_draw(tr, '--fused_validation is missing') is False
    assert tr.trainer_log['subset_draw'] == 'upstream: --fused_validation is missing'
    assert capsys.readouterr().out.count('--device_subsets: --fused_validation is missing; drawing the validation subsets as upstream does') == 1
    assert evalpass.subset_draw(tr, None) is True and tr.trainer_log['subset_draw'] == 'device'
    evalpass._fallback(tr, 'no such model')
    assert tr.trainer_log['subset_draw'] == 'upstream: the prepared pass fell back (no such model)'
