"""The entries of --device_subsets (csrc/rankeval.hip) on the GPU.  gd_subset_draw against the numpy restatement
(gnndelete_amd/subsets.reference_draw) to the bit: the narrowest domain, k = m, k above the 1,024-thread stride, both sides of
2^16 (bits = 16 and, the worst walk ratio, 18), the widest domain (bits = 32), and a row pitch above k with a sentinel behind
every row.  gd_subset_rank_metrics_drawn against gd_subset_rank_metrics on gd_subset_draw's matrix to the bit - the two
differ only in where phase 2 takes a member from - and against framework/metrics.batched_* on those rows: AUC equal to the bit,
AP within the 1e-12 of tests/test_metrics.py; at the shapes of tests/test_rankeval_kernels_gpu.py (a partial last bitmap word,
k almost m, k = m, one run of equal scores, several 1024-word scan chunks with continuous and with 5-level scores) plus the
smallest pool; on a workspace full of ones, twice, under another seed, and with no subsets at all."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
AP_TOL = 1e-12
SEED, DRAW = 0x9E3779B97F4A7C15, 3          # a seed with its upper half set: both are 64-bit arguments


# ------------------------------------------------------------------------------------------ gd_subset_draw
DRAWS = [(32, 1, 2), (32, 32, 3), (65, 64, 4), (4099, 2049, 3), (65536, 513, 3), (65537, 3000, 7), (2 ** 31 - 1, 4096, 2)]      # (m, k, B)


@pytest.mark.parametrize('m,k,n_sub', DRAWS)
def test_the_draw_is_the_restatement_to_the_bit(m, k, n_sub):
    from gnndelete_amd import subsets
    want = subsets.reference_draw(SEED, DRAW, n_sub, k, m)
    got = subsets.draw(SEED, DRAW, n_sub, k, m)
    assert got.dtype == torch.int64 and tuple(got.shape) == (n_sub, k) and got.is_cuda
    assert np.array_equal(got.cpu().numpy(), want)
    assert torch.equal(subsets.draw(SEED, DRAW, n_sub, k, m), got)               # a second call
    assert not torch.equal(subsets.draw(SEED + 1, DRAW, n_sub, k, m), got) and not torch.equal(subsets.draw(SEED, DRAW + 1, n_sub, k, m), got)


@pytest.mark.parametrize('m,k,n_sub', [(65, 64, 4), (4099, 2049, 3)])
def test_a_wider_row_pitch_leaves_what_is_behind_a_row_alone(m, k, n_sub):
    from gnndelete_amd import subsets
    wide = torch.full((n_sub, k + 5), -7, dtype=torch.int64, device='cuda')
    got = subsets.draw(SEED, DRAW, n_sub, k, m, out=wide)
    assert got.data_ptr() == wide.data_ptr() and np.array_equal(got.cpu().numpy(), subsets.reference_draw(SEED, DRAW, n_sub, k, m))
    assert bool((wide[:, k:] == -7).all())
    one = torch.full((1, k + 5), -7, dtype=torch.int64, device='cuda')            # a single row
    subsets.draw(SEED, DRAW, 1, k, m, out=one)
    assert np.array_equal(one[:, :k].cpu().numpy(), subsets.reference_draw(SEED, DRAW, 1, k, m)) and bool((one[:, k:] == -7).all())


def test_no_subsets_is_no_launch():
    from gnndelete_amd import subsets
    assert tuple(subsets.draw(SEED, DRAW, 0, 4, 40).shape) == (0, 4)


# ------------------------------------------------------------------------------------------ gd_subset_rank_metrics_drawn
SHAPES = {                      # name: (m, k, n_ref, B, levels)  levels: 0 continuous, 1 all scores equal, n quantised to n values
    'smallest_pool': (32, 32, 1, 2, 0),
    'k_almost_m': (65, 64, 64, 4, 0),
    'k_is_m': (1000, 1000, 37, 1, 0),
    'one_run': (4099, 513, 200, 3, 1),
    'chunks': (70001, 3000, 3000, 7, 0),
    'chunks_5_levels': (70001, 3000, 3000, 7, 5),
}


@functools.lru_cache(maxsize=None)
def _case(name):
    """(ref, pool) on the device, gd_subset_draw's matrix, and the oracle's (auc, ap) on those rows on the host; computed once
    and shared, changed by no test."""
    from gnndelete_amd import subsets
    from gnndelete_amd.framework.metrics import batched_average_precision, batched_roc_auc
    m, k, n_ref, n_sub, levels = SHAPES[name]
    g = torch.Generator().manual_seed(m + k)
    if levels == 0:
        ref, pool = torch.rand(n_ref, generator=g), torch.rand(m, generator=g)
    elif levels == 1:
        ref, pool = torch.full((n_ref,), 0.625), torch.full((m,), 0.625)
    else:
        ref, pool = [torch.randint(0, levels, (n,), generator=g).float() / levels for n in (n_ref, m)]
    ref, pool = ref.cuda(), pool.cuda()
    idx = subsets.draw(SEED, DRAW, n_sub, k, m)
    scores = torch.cat([ref[None].expand(n_sub, -1), pool[idx]], dim=1)
    labels = torch.cat([torch.zeros(n_ref), torch.ones(k)]).cuda()
    return ref, pool, idx, batched_roc_auc(scores, labels).cpu(), batched_average_precision(scores, labels).cpu()


@pytest.mark.parametrize('name', list(SHAPES))
def test_drawn_metrics_are_the_index_matrix_metrics_to_the_bit(name):
    from gnndelete_amd.rankeval import subset_auc_ap, subset_auc_ap_drawn
    ref, pool, idx, want_auc, want_ap = _case(name)
    n_sub, k = idx.shape
    auc, ap = subset_auc_ap_drawn(ref, pool, SEED, DRAW, n_sub, k)
    assert auc.dtype == ap.dtype == torch.float64 and auc.shape == ap.shape == (n_sub,)
    by_idx = subset_auc_ap(ref, pool, idx)
    print(name, 'max |AP - oracle| =', float((ap.cpu() - want_ap).abs().max()), 'AUC equal:', torch.equal(auc.cpu(), want_auc),
          'equal to the index-matrix entry:', torch.equal(auc, by_idx[0]), torch.equal(ap, by_idx[1]))
    assert torch.equal(auc, by_idx[0]) and torch.equal(ap, by_idx[1])
    assert torch.equal(auc.cpu(), want_auc)
    assert float((ap.cpu() - want_ap).abs().max()) <= AP_TOL
    again = subset_auc_ap_drawn(ref, pool, SEED, DRAW, n_sub, k)                 # the same bits on every call
    assert torch.equal(again[0], auc) and torch.equal(again[1], ap)


@pytest.mark.parametrize('name', ['k_almost_m', 'chunks'])
def test_another_seed_or_draw_gives_another_auc(name):
    from gnndelete_amd.rankeval import subset_auc_ap_drawn
    ref, pool, idx, want_auc, _ = _case(name)
    n_sub, k = idx.shape
    for seed, draw in ((SEED + 1, DRAW), (SEED, DRAW + 1)):
        auc, _ = subset_auc_ap_drawn(ref, pool, seed, draw, n_sub, k)
        assert not torch.equal(auc.cpu(), want_auc)


def test_no_subsets_and_refusals():
    from gnndelete_amd.rankeval import subset_auc_ap_drawn
    ref, pool, _, _, _ = _case('k_almost_m')
    auc, ap = subset_auc_ap_drawn(ref, pool, SEED, DRAW, 0, 8)
    assert auc.numel() == 0 and ap.numel() == 0
    with pytest.raises(ValueError, match='a pool of 31 scores'):
        subset_auc_ap_drawn(ref, pool[:31], SEED, DRAW, 2, 8)
    with pytest.raises(ValueError, match='subsets of 66 positives from a pool of 65'):
        subset_auc_ap_drawn(ref, pool, SEED, DRAW, 2, 66)


def test_a_workspace_full_of_ones_is_zeroed_by_the_kernel():
    """The entry itself, the way subset_auc_ap_drawn prepares its inputs, on a workspace whose every bit is set on entry."""
    from gnndelete_amd import _lib
    from gnndelete_amd._lib import check, ptr, stream_ptr
    from gnndelete_amd.rankeval import rank_counts
    ref, pool, idx, want_auc, want_ap = _case('chunks_5_levels')
    m, n_ref, (n_sub, k) = pool.numel(), ref.numel(), idx.shape
    sorted_pool, order = torch.sort(pool, descending=True)
    at = torch.arange(m, dtype=torch.int32, device='cuda')
    pos = torch.empty_like(at)
    pos[order] = at
    less, leq = rank_counts(torch.sort(ref).values, sorted_pool)
    run_end = ((m - 1) - rank_counts(sorted_pool.flip(0), sorted_pool)[0]).contiguous()
    L = _lib.lib()
    n_bytes = L.gd_subset_rank_workspace(n_sub, m)
    ws = torch.full((n_bytes // 4,), -1, dtype=torch.int32, device='cuda')
    auc, ap = torch.empty(n_sub, dtype=torch.float64, device='cuda'), torch.empty(n_sub, dtype=torch.float64, device='cuda')
    u2, ge_at = less + leq, n_ref - less
    check(L.gd_subset_rank_metrics_drawn(ptr(u2), ptr(ge_at), ptr(run_end), ptr(pos), SEED, DRAW, n_sub, k, m, n_ref, ptr(auc), ptr(ap), ptr(ws),
                                         n_bytes, stream_ptr()), 'gd_subset_rank_metrics_drawn')
    assert torch.equal(auc.cpu(), want_auc) and float((ap.cpu() - want_ap).abs().max()) <= AP_TOL
    # each subset's bitmap row now holds exactly its k members, at the sorted positions of gd_subset_draw's row
    words = 2208
    rows = ws.view(n_sub, 2, words)[:, 0, :(m + 31) // 32]
    bits = (rows[:, :, None] >> torch.arange(32, device='cuda', dtype=torch.int32)) & 1
    assert bits.sum(dim=(1, 2)).tolist() == [k] * n_sub
    member = bits.reshape(n_sub, -1)[:, :m].bool()
    want = torch.zeros(n_sub, m, dtype=torch.bool, device='cuda')
    want.scatter_(1, pos[idx].long(), True)
    assert torch.equal(member, want)
