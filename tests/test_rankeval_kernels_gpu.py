"""The rank kernels of --fused_eval (csrc/rankeval.hip) on the GPU: gd_rank_counts_f32 against numpy.searchsorted, and
rankeval.subset_auc_ap against framework/metrics.batched_* on the concatenated score matrix - AUC equal to the bit, AP within
the 1e-12 of tests/test_metrics.py - at the smallest shapes that reach each edge of gd_subset_rank_metrics: a partial last
bitmap word, k almost m, k = m with n_ref != k, one run of equal scores spanning every word, and several 1024-word scan
chunks with runs crossing words and chunks and k above the block size.  Also: the same bits on a second call, a workspace
that arrives full of ones, an index matrix passed as a strided view, and the numpy restatement on the same inputs."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
AP_TOL = 1e-12


# ------------------------------------------------------------------------------------------ gd_rank_counts_f32
def _counts_case(name):
    g = torch.Generator().manual_seed(11)
    if name == 'duplicates':
        ref = torch.randint(0, 40, (300,), generator=g).float() / 8
        query = torch.cat([torch.randint(-3, 44, (1000,), generator=g).float() / 8, torch.rand(500, generator=g) * 5])
    elif name == 'ends':
        ref = torch.tensor([-1.5, -1.5, 0.0, 0.25, 0.25, 0.25, 3.0, 7.0, 7.0])
        query = torch.tensor([-2.0, -1.5, np.nextafter(np.float32(-1.5), np.float32(0)), 0.25, 6.999, 7.0, 7.5, float('inf'), -float('inf')])
    elif name == 'one':
        ref = torch.tensor([0.5])
        query = torch.tensor([0.0, 0.5, 1.0, 0.5, 0.4999])
    else:
        ref = torch.rand(5000, generator=g)
        query = torch.cat([torch.rand(70001, generator=g), ref[:64]])
    return torch.sort(ref).values, query


@pytest.mark.parametrize('name', ['duplicates', 'ends', 'one', 'large'])
def test_rank_counts_match_searchsorted(name):
    from gnndelete_amd.rankeval import rank_counts
    ref, query = _counts_case(name)
    less, leq = rank_counts(ref.cuda(), query.cuda())
    assert less.dtype == leq.dtype == torch.int32
    assert np.array_equal(less.cpu().numpy(), np.searchsorted(ref.numpy(), query.numpy(), side='left'))
    assert np.array_equal(leq.cpu().numpy(), np.searchsorted(ref.numpy(), query.numpy(), side='right'))


def test_rank_counts_of_a_nan_query_stay_in_range():
    from gnndelete_amd.rankeval import rank_counts
    ref = torch.tensor([0.1, 0.2, 0.2, 0.9]).cuda()
    less, leq = rank_counts(ref, torch.tensor([float('nan'), 0.2]).cuda())
    assert less.tolist()[1] == 1 and leq.tolist()[1] == 3
    assert 0 <= less.tolist()[0] <= leq.tolist()[0] <= 4


# ------------------------------------------------------------------------------------------ subset_auc_ap
SHAPES = {                      # name: (m, k, n_ref, B, levels)  levels: 0 continuous, 1 all scores equal, n quantised to n values
    'partial_last_word': (33, 1, 1, 2, 0),
    'k_almost_m': (65, 64, 64, 4, 0),
    'k_is_m': (1000, 1000, 37, 1, 0),
    'one_run': (4099, 513, 200, 3, 1),
    'chunks': (70001, 3000, 3000, 7, 0),
    'chunks_5_levels': (70001, 3000, 3000, 7, 5),
}


@functools.lru_cache(maxsize=None)
def _case(name):
    """(ref, pool, idx) on the device and the oracle's (auc, ap) on the host, computed once and shared."""
    from gnndelete_amd.framework.metrics import batched_average_precision, batched_roc_auc
    m, k, n_ref, n_sub, levels = SHAPES[name]
    g = torch.Generator().manual_seed(m + k)
    if levels == 0:
        ref, pool = torch.rand(n_ref, generator=g), torch.rand(m, generator=g)
    elif levels == 1:
        ref, pool = torch.full((n_ref,), 0.625), torch.full((m,), 0.625)
    else:
        ref, pool = [torch.randint(0, levels, (n,), generator=g).float() / levels for n in (n_ref, m)]
    idx = torch.stack([torch.randperm(m, generator=g)[:k] for _ in range(n_sub)])
    ref, pool, idx = ref.cuda(), pool.cuda(), idx.cuda()
    scores = torch.cat([ref[None].expand(n_sub, -1), pool[idx]], dim=1)
    labels = torch.cat([torch.zeros(n_ref), torch.ones(k)]).cuda()
    return ref, pool, idx, batched_roc_auc(scores, labels).cpu(), batched_average_precision(scores, labels).cpu()


@pytest.mark.parametrize('name', list(SHAPES))
def test_subset_metrics_match_the_batched_sort(name):
    from gnndelete_amd.rankeval import subset_auc_ap
    ref, pool, idx, want_auc, want_ap = _case(name)
    auc, ap = subset_auc_ap(ref, pool, idx)
    assert auc.dtype == ap.dtype == torch.float64 and auc.shape == ap.shape == (idx.shape[0],)
    print(name, 'max |AP - oracle| =', float((ap.cpu() - want_ap).abs().max()), 'AUC equal:', torch.equal(auc.cpu(), want_auc))
    assert torch.equal(auc.cpu(), want_auc)
    assert float((ap.cpu() - want_ap).abs().max()) <= AP_TOL
    again = subset_auc_ap(ref, pool, idx)                        # the same bits on every call
    assert torch.equal(again[0], auc) and torch.equal(again[1], ap)


@pytest.mark.parametrize('name', ['partial_last_word', 'one_run', 'chunks_5_levels'])
def test_numpy_restatement_agrees_with_the_kernels(name):
    from gnndelete_amd.rankeval import reference_subset_auc_ap, subset_auc_ap
    ref, pool, idx, _, _ = _case(name)
    auc, ap = subset_auc_ap(ref, pool, idx)
    r_auc, r_ap = reference_subset_auc_ap(ref, pool, idx)
    assert np.array_equal(auc.cpu().numpy(), r_auc)
    assert np.abs(ap.cpu().numpy() - r_ap).max() <= AP_TOL


def test_saturated_sigmoid_scores_tie_as_the_torch_path_ties_them():
    from gnndelete_amd.framework.metrics import batched_average_precision, batched_roc_auc
    from gnndelete_amd.rankeval import subset_auc_ap
    g = torch.Generator().manual_seed(5)
    ref, pool = (torch.randn(300, generator=g) * 30).sigmoid().cuda(), (torch.randn(2500, generator=g) * 30 + 4).sigmoid().cuda()
    assert int((pool == 1).sum()) > 100 and int((ref == 1).sum()) > 10     # (fp32 sigmoid is exactly 1 from about 17 on)
    idx = torch.stack([torch.randperm(2500, generator=g)[:300] for _ in range(5)]).cuda()
    auc, ap = subset_auc_ap(ref, pool, idx)
    scores = torch.cat([ref[None].expand(5, -1), pool[idx]], dim=1)
    labels = torch.cat([torch.zeros(300), torch.ones(300)]).cuda()
    assert torch.equal(auc, batched_roc_auc(scores, labels))
    assert float((ap - batched_average_precision(scores, labels)).abs().max()) <= AP_TOL


def test_strided_index_views():
    from gnndelete_amd.rankeval import subset_auc_ap
    ref, pool, idx, want_auc, want_ap = _case('k_almost_m')
    n_sub, k = idx.shape
    wide = torch.full((n_sub, 2 * k + 3), -7, dtype=torch.int64, device='cuda')        # rows 2k + 3 apart, junk behind each
    wide[:, :k] = idx
    tall = torch.full((2 * n_sub, k), 1 << 40, dtype=torch.int64, device='cuda')       # every other row
    tall[::2] = idx
    for view in (wide[:, :k], tall[::2], idx.t().contiguous().t()):
        assert view.stride() != idx.stride()
        auc, ap = subset_auc_ap(ref, pool, view)
        assert torch.equal(auc.cpu(), want_auc) and float((ap.cpu() - want_ap).abs().max()) <= AP_TOL
    one = subset_auc_ap(ref, pool, idx[2])                       # a single row, one dimension
    assert float(one[0][0]) == float(want_auc[2])


def test_a_workspace_full_of_ones_is_zeroed_by_the_kernel():
    """The entry itself, the way subset_auc_ap prepares its inputs, on a workspace whose every bit is set on entry."""
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
    last = torch.ones(m, dtype=torch.bool, device='cuda')
    last[:-1] = sorted_pool[1:] != sorted_pool[:-1]
    run_end = torch.where(last, at, at.new_full((), m)).flip(0).cummin(0).values.flip(0).contiguous()
    L = _lib.lib()
    n_bytes = L.gd_subset_rank_workspace(n_sub, m)
    ws = torch.full((n_bytes // 4,), -1, dtype=torch.int32, device='cuda')
    auc, ap = torch.empty(n_sub, dtype=torch.float64, device='cuda'), torch.empty(n_sub, dtype=torch.float64, device='cuda')
    u2, ge_at = less + leq, n_ref - less
    check(L.gd_subset_rank_metrics(ptr(u2), ptr(ge_at), ptr(run_end), ptr(pos), ptr(idx), idx.stride(0), n_sub, k, m, n_ref,
                                   ptr(auc), ptr(ap), ptr(ws), n_bytes, stream_ptr()), 'gd_subset_rank_metrics')
    assert torch.equal(auc.cpu(), want_auc) and float((ap.cpu() - want_ap).abs().max()) <= AP_TOL
    # each subset's bitmap row now holds exactly its k members
    words = 2208
    rows = ws.view(n_sub, 2, words)[:, 0, :(m + 31) // 32]
    bits = ((rows[:, :, None] >> torch.arange(32, device='cuda', dtype=torch.int32)) & 1).sum(dim=(1, 2))
    assert bits.tolist() == [k] * n_sub
