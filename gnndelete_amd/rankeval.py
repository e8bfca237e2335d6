"""Resampled ROC-AUC / average precision without the [B, 2k] sort (csrc/rankeval.hip; Trainer.eval under --fused_eval).

Trainer.eval scores the deleted edges with 500 AUC / AP values: every one ranks the SAME negatives (the Df scores, label 0)
against k positives taken from ONE pool (the Dr scores, label 1) through an index matrix drawn once per request.
framework/metrics.batched_* sorts the [500, 2k] score matrix; here the ranking is split instead:

  once per validation, on the m pool scores: one descending sort of the pool, and the position of every pool score in the
      ascending negatives (gd_rank_counts_f32: less = negatives below it, leq = negatives at or below it) and in the
      ascending pool itself (the same entry: the end of a run of equal scores is m - 1 - the pool scores below it)
  per subset (gd_subset_rank_metrics, one block each): a membership bitmap over the pool's sorted order, a popcount prefix,
      one pass over the set bits

With p a position in the sorted pool, run_end[p] the last position holding the same score, u2[p] = less + leq
(= 2 less + ties) and ge_at[p] = n_ref - less:

  AUC_b = double(sum of u2 over the subset's positions) / (2 k n_ref)          the Mann-Whitney U over k n_ref, ties = 1/2
  AP_b  = (1 / k) sum over the subset's positions p of TP(p) / (TP(p) + ge_at[p])      TP(p) = members at positions <= run_end[p]

The AUC's numerator is an exact integer, so it is the same double as metrics.batched_roc_auc gives; the AP is scikit-learn's
sum over distinct thresholds with the recall step of a run of equal scores spread over the run's members, equal to
metrics.batched_average_precision within rounding (a few 1e-16).  The scores are ranked as given: hand in the same fp32
sigmoid outputs the torch path ranks, so that saturated scores tie the same way.  reference_subset_auc_ap restates the
formulas in numpy and is the kernels' CPU oracle next to framework/metrics.py.

subset_auc_ap_drawn (--device_subsets) is the same ranking without an index matrix: gd_subset_rank_metrics_drawn computes the
members of every subset from (seed, draw) where the other entry reads idx (gnndelete_amd/subsets.py: the stream)."""
import numpy as np
import torch


def fused_eval_unsupported(n_ref, m, k, on_gpu=True, dtype=torch.float32):
    """None when the rank kernels take n_ref negatives against k-subsets of a pool of m scores, else the reason (one line)."""
    n_ref, m, k = int(n_ref), int(m), int(k)
    if not on_gpu:
        return 'the scores are not on the GPU'
    if dtype != torch.float32:
        return f'{dtype} scores (float32 only)'
    if n_ref < 1:
        return f'{n_ref} negatives (at least one)'
    if n_ref >= 1 << 30:
        return f'{n_ref} negatives (below 2^30)'
    if k < 1:
        return f'subsets of {k} positives (at least one)'
    if m >= 1 << 31:
        return f'a pool of {m} scores (below 2^31)'
    if k > m:
        return f'subsets of {k} positives from a pool of {m}'
    return None


def _tables(ref, pool):
    """numpy: (pos by pool element, u2 / ge_at / run_end by sorted position) of a float32 pool against float32 negatives."""
    ref = np.sort(np.asarray(ref, dtype=np.float32).reshape(-1))
    pool = np.asarray(pool, dtype=np.float32).reshape(-1)
    m = pool.size
    order = np.argsort(pool, kind='stable')[::-1]
    sp = pool[order]
    less = np.searchsorted(ref, sp, side='left').astype(np.int64)
    leq = np.searchsorted(ref, sp, side='right').astype(np.int64)
    pos = np.empty(m, dtype=np.int64)
    pos[order] = np.arange(m)
    last = np.ones(m, dtype=bool)
    last[:-1] = sp[1:] != sp[:-1]
    run_end = np.minimum.accumulate(np.where(last, np.arange(m), m)[::-1])[::-1]
    return pos, less + leq, ref.size - less, run_end


def reference_subset_auc_ap(ref, pool, idx):
    """subset_auc_ap on the CPU in numpy -> (auc [B], ap [B]) float64 arrays.  ref [n_ref], pool [m]: float32 scores (arrays or
    tensors); idx [B, k]: pool indices, distinct within a row."""
    if isinstance(ref, torch.Tensor):
        ref = ref.detach().cpu().numpy()
    if isinstance(pool, torch.Tensor):
        pool = pool.detach().cpu().numpy()
    if isinstance(idx, torch.Tensor):
        idx = idx.detach().cpu().numpy()
    idx = np.asarray(idx, dtype=np.int64)
    idx = idx[None] if idx.ndim == 1 else idx
    n_ref, m, (n_sub, k) = int(np.asarray(ref).size), int(np.asarray(pool).size), idx.shape
    reason = fused_eval_unsupported(n_ref, m, k)
    if reason is not None:
        raise ValueError(f'reference_subset_auc_ap: {reason}')
    pos, u2, ge_at, run_end = _tables(ref, pool)
    auc, ap = np.empty(n_sub, dtype=np.float64), np.empty(n_sub, dtype=np.float64)
    for b in range(n_sub):
        p = np.sort(pos[idx[b]])
        member = np.zeros(m, dtype=np.int64)
        member[p] = 1
        tp = np.cumsum(member)[run_end[p]].astype(np.float64)
        auc[b] = float(int(u2[p].sum())) / (2.0 * k * n_ref)
        ap[b] = float(np.sum(tp / (tp + ge_at[p].astype(np.float64)))) / k
    return auc, ap


def rank_counts(ref_sorted, query):
    """gd_rank_counts_f32 -> (less, leq) int32 [m]: for every query score the number of ref_sorted scores below it / at or below
    it.  ref_sorted: ASCENDING float32 device tensor, at least one score; query: float32, same device."""
    from . import _lib
    from ._lib import check, ptr, stream_ptr
    for name, t in (('ref_sorted', ref_sorted), ('query', query)):
        if t.dtype != torch.float32 or t.dim() != 1 or not t.is_cuda or t.device != ref_sorted.device:
            raise ValueError(f'rank_counts: {name} must be a float32 vector on one GPU')
    ref_sorted, query = ref_sorted.contiguous(), query.contiguous()
    dev, m = query.device, query.numel()
    less = torch.empty(m, dtype=torch.int32, device=dev)
    leq = torch.empty(m, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        check(_lib.lib().gd_rank_counts_f32(ptr(ref_sorted), ref_sorted.numel(), ptr(query), m, ptr(less), ptr(leq), stream_ptr(dev)),
              'gd_rank_counts_f32')
    return less, leq


def subset_auc_ap(ref, pool, idx):
    """ROC-AUC and average precision of `ref` (label 0) against pool[idx[b]] (label 1) for every row b -> (auc [B], ap [B]),
    float64 on the device; the values of metrics.batched_roc_auc (bit-equal) / batched_average_precision (within rounding) on
    cat([ref.expand(B, -1), pool[idx]], 1).

    ref [n_ref], pool [m]: float32 device tensors; idx [B, k] (or [k]): int64 pool indices on the same device, any row stride.
    PRECONDITION: the indices of a row are DISTINCT (the trainer's rows are randperm(m)[:k]); a repeated index counts once in
    the ranking but k times in the divisor.  Raises ValueError where fused_eval_unsupported gives a reason."""
    from ._lib import check, ptr, stream_ptr
    if idx.dim() == 1:
        idx = idx[None]
    if idx.dim() != 2 or idx.dtype != torch.int64:
        raise ValueError(f'subset_auc_ap: idx of shape {tuple(idx.shape)} / {idx.dtype}, expected int64 [B, k]')
    on_gpu = ref.is_cuda and pool.is_cuda and idx.is_cuda and ref.device == pool.device == idx.device
    n_ref, m, (n_sub, k) = ref.numel(), pool.numel(), idx.shape
    reason = fused_eval_unsupported(n_ref, m, k, on_gpu, ref.dtype if ref.dtype == pool.dtype else pool.dtype)
    if reason is not None:
        raise ValueError(f'subset_auc_ap: {reason}')
    if k > 1 and idx.stride(1) != 1:
        idx = idx.contiguous()
    L, dev, (u2, ge_at, run_end, pos), (ws, auc, ap) = _prepare(ref, pool, n_sub, 'subset_auc_ap')
    with torch.cuda.device(dev):
        check(L.gd_subset_rank_metrics(ptr(u2), ptr(ge_at), ptr(run_end), ptr(pos), ptr(idx), idx.stride(0) if n_sub > 1 else k, n_sub,
                                       k, m, n_ref, ptr(auc), ptr(ap), ptr(ws), 4 * ws.numel(), stream_ptr(dev)),
              'gd_subset_rank_metrics')
    return auc, ap


def _prepare(ref, pool, n_sub, who):
    """What a ranking of n_sub subsets needs before its per-subset pass -> (library, device, (u2, ge_at, run_end, pos) by the
    formulas above, (workspace, auc, ap) to be filled)."""
    from . import _lib
    n_ref, m, dev = ref.numel(), pool.numel(), pool.device
    # once per call, O(m log m): the pool in descending order and where each of its scores falls among the negatives
    ref_sorted = torch.sort(ref.reshape(-1)).values
    sorted_pool, order = torch.sort(pool.reshape(-1), descending=True)
    at = torch.arange(m, dtype=torch.int32, device=dev)
    pos = torch.empty(m, dtype=torch.int32, device=dev)
    pos[order] = at
    less, leq = rank_counts(ref_sorted, sorted_pool)
    u2 = less + leq
    ge_at = n_ref - less
    # the last position of a score's run = (pool scores at or above it) - 1 = m - 1 - (pool scores below it): the same search,
    # in the pool itself (a reverse cummin over the run ends is one slow scan launch: 5.4 ms at 2 M scores)
    run_end = (m - 1) - rank_counts(sorted_pool.flip(0), sorted_pool)[0]
    # per subset: the HIP pass
    L = _lib.lib()
    n_bytes = L.gd_subset_rank_workspace(n_sub, m)
    if n_bytes < 0:
        raise ValueError(f'{who}: {n_sub} subsets of a pool of {m} are out of range')
    ws = torch.empty(n_bytes // 4 + 4, dtype=torch.int32, device=dev)
    auc = torch.empty(n_sub, dtype=torch.float64, device=dev)
    ap = torch.empty(n_sub, dtype=torch.float64, device=dev)
    return L, dev, (u2, ge_at, run_end, pos), (ws, auc, ap)


def subset_auc_ap_drawn(ref, pool, seed, draw, n_sub, k):
    """subset_auc_ap(ref, pool, subsets.draw(seed, draw, n_sub, k, pool.numel())), bit for bit, without the index matrix:
    gd_subset_rank_metrics_drawn computes member j of subset b (subsets.py: the stream) where the other entry reads idx[b, j].
    ref [n_ref], pool [m]: float32 device tensors, m >= 32.  Raises ValueError where fused_eval_unsupported or
    subsets.device_subsets_unsupported gives a reason."""
    from ._lib import check, ptr, stream_ptr
    from .subsets import device_subsets_unsupported
    on_gpu = ref.is_cuda and pool.is_cuda and ref.device == pool.device
    n_ref, m, n_sub, k = ref.numel(), pool.numel(), int(n_sub), int(k)
    reason = fused_eval_unsupported(n_ref, m, k, on_gpu, ref.dtype if ref.dtype == pool.dtype else pool.dtype)
    if reason is None:
        reason = device_subsets_unsupported(m, k)
    if reason is not None:
        raise ValueError(f'subset_auc_ap_drawn: {reason}')
    L, dev, (u2, ge_at, run_end, pos), (ws, auc, ap) = _prepare(ref, pool, n_sub, 'subset_auc_ap_drawn')
    with torch.cuda.device(dev):
        check(L.gd_subset_rank_metrics_drawn(ptr(u2), ptr(ge_at), ptr(run_end), ptr(pos), int(seed) & 0xFFFFFFFFFFFFFFFF,
                                             int(draw) & 0xFFFFFFFFFFFFFFFF, n_sub, k, m, n_ref, ptr(auc), ptr(ap), ptr(ws), 4 * ws.numel(),
                                             stream_ptr(dev)), 'gd_subset_rank_metrics_drawn')
    return auc, ap
