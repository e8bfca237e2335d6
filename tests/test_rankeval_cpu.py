"""--fused_eval without a GPU: the numpy restatement of the rank formulas (gnndelete_amd/rankeval.reference_subset_auc_ap, the
kernels' CPU oracle) against framework/metrics.batched_* and scikit-learn on small inputs with ties - AUC equal to the bit, AP
within the 1e-12 of tests/test_metrics.py - the flag, every fallback reason, and the entries' declarations, size query and
host-side refusals."""
import numpy as np
import pytest
import torch

AP_TOL = 1e-12          # tests/test_metrics.py's tolerance


def _case(m, k, n_ref, n_sub, levels, seed):
    """ref [n_ref], pool [m] float32 with `levels` distinct values at the most (0: continuous), idx [n_sub, k] distinct per row."""
    g = torch.Generator().manual_seed(seed)
    draw = (lambda n: torch.rand(n, generator=g)) if levels == 0 else (lambda n: torch.randint(0, levels, (n,), generator=g).float() / max(levels, 1))
    ref, pool = draw(n_ref), draw(m)
    idx = torch.stack([torch.randperm(m, generator=g)[:k] for _ in range(n_sub)])
    return ref, pool, idx


def _torch_oracle(ref, pool, idx):
    from gnndelete_amd.framework.metrics import batched_average_precision, batched_roc_auc
    n_sub, k = idx.shape
    scores = torch.cat([ref[None].expand(n_sub, -1), pool[idx]], dim=1)
    labels = torch.cat([torch.zeros(ref.numel()), torch.ones(k)])
    return batched_roc_auc(scores, labels).numpy(), batched_average_precision(scores, labels).numpy()


# (m, k, n_ref, B, levels).  scikit-learn's roc_auc_score is a trapezoid sum over (fpr, tpr) points that are multiples of
# 1 / n_ref and 1 / k: with both powers of two every term and every partial sum is exact, so it IS the correctly rounded
# U / (k n_ref) and `==` is well defined; at other sizes its sum carries its own rounding (0.5614000000000001 for 2807 / 5000
# at k = n_ref = 100, where metrics.batched_roc_auc and the formulas here both give 0.5614) and the comparison with it is
# tests/test_metrics.py's: within 1e-12.  Against metrics.batched_roc_auc the AUC is equal to the bit at every size.
DYADIC = [(33, 1, 1, 2, 0), (33, 8, 4, 3, 3), (65, 64, 64, 4, 4), (40, 32, 8, 2, 0), (50, 16, 8, 3, 1), (200, 64, 32, 5, 6)]
OTHER = [(33, 7, 5, 3, 3), (40, 40, 13, 1, 0), (50, 17, 9, 3, 1), (200, 60, 45, 5, 6), (300, 100, 100, 4, 0)]


@pytest.mark.parametrize('m,k,n_ref,n_sub,levels', DYADIC + OTHER)
def test_reference_matches_metrics_and_sklearn(m, k, n_ref, n_sub, levels):
    from sklearn.metrics import average_precision_score, roc_auc_score
    from gnndelete_amd.rankeval import reference_subset_auc_ap
    ref, pool, idx = _case(m, k, n_ref, n_sub, levels, seed=m + k)
    auc, ap = reference_subset_auc_ap(ref, pool, idx)
    t_auc, t_ap = _torch_oracle(ref, pool, idx)
    assert auc.dtype == np.float64 and ap.dtype == np.float64 and auc.shape == ap.shape == (n_sub,)
    assert np.array_equal(auc, t_auc)
    assert np.abs(ap - t_ap).max() <= AP_TOL
    y = np.r_[np.zeros(n_ref), np.ones(k)]
    for b in range(n_sub):
        s = np.r_[ref.numpy(), pool[idx[b]].numpy()].astype(np.float64)
        if (m, k, n_ref, n_sub, levels) in DYADIC:
            assert auc[b] == roc_auc_score(y, s)
        else:
            assert abs(auc[b] - roc_auc_score(y, s)) <= 1e-12
        assert abs(ap[b] - average_precision_score(y, s)) <= AP_TOL


def test_reference_on_saturated_sigmoid_scores():
    """The trainer ranks fp32 sigmoid outputs: large logits saturate to exactly 1.0 and tie there."""
    from gnndelete_amd.rankeval import reference_subset_auc_ap
    g = torch.Generator().manual_seed(3)
    ref, pool = (torch.randn(40, generator=g) * 30).sigmoid(), (torch.randn(90, generator=g) * 30 + 5).sigmoid()
    assert int((pool == 1).sum()) > 5 and int((ref == 1).sum()) > 1
    idx = torch.stack([torch.randperm(90, generator=g)[:40] for _ in range(6)])
    auc, ap = reference_subset_auc_ap(ref, pool, idx)
    t_auc, t_ap = _torch_oracle(ref, pool, idx)
    assert np.array_equal(auc, t_auc) and np.abs(ap - t_ap).max() <= AP_TOL
    one = reference_subset_auc_ap(ref, pool, idx[2])                # a single row
    assert one[0][0] == auc[2] and one[1][0] == ap[2]


def test_the_flag_parses_and_defaults_off():
    from gnndelete_amd.framework.training_args import EXTRA_FLAGS, build_parser
    assert 'fused_eval' in [f[0] for f in EXTRA_FLAGS]
    p = build_parser()
    assert p.parse_args([]).fused_eval is False
    a = p.parse_args(['--fused_eval', '--unlearning_model', 'gnndelete'])
    assert a.fused_eval is True and a.unlearning_model == 'gnndelete'
    assert not hasattr(build_parser(extra=False).parse_args([]), 'fused_eval')


def test_every_fallback_has_its_reason():
    from gnndelete_amd.rankeval import fused_eval_unsupported, reference_subset_auc_ap
    assert fused_eval_unsupported(10, 100, 10) is None
    assert fused_eval_unsupported(1, 1, 1) is None and fused_eval_unsupported((1 << 30) - 1, (1 << 31) - 1, 5) is None
    want = {
        (0, 100, 10): '0 negatives (at least one)',
        (1 << 30, 100, 10): f'{1 << 30} negatives (below 2^30)',
        (10, 100, 0): 'subsets of 0 positives (at least one)',
        (10, 100, 101): 'subsets of 101 positives from a pool of 100',
        (10, 1 << 31, 10): f'a pool of {1 << 31} scores (below 2^31)',
    }
    for sizes, reason in want.items():
        assert fused_eval_unsupported(*sizes) == reason
    assert fused_eval_unsupported(10, 100, 10, on_gpu=False) == 'the scores are not on the GPU'
    assert fused_eval_unsupported(10, 100, 10, True, torch.float64) == 'torch.float64 scores (float32 only)'
    reasons = list(want.values()) + ['the scores are not on the GPU', 'torch.float64 scores (float32 only)']
    assert len(set(reasons)) == len(reasons) and all('\n' not in r for r in reasons)
    with pytest.raises(ValueError, match='subsets of 5 positives from a pool of 4'):
        reference_subset_auc_ap(np.zeros(3, np.float32), np.zeros(4, np.float32), np.zeros((1, 5), np.int64))


def test_wrapper_refuses_host_tensors():
    from gnndelete_amd.rankeval import subset_auc_ap
    with pytest.raises(ValueError, match='the scores are not on the GPU'):
        subset_auc_ap(torch.rand(4), torch.rand(9), torch.arange(3)[None])
    with pytest.raises(ValueError, match='expected int64'):
        subset_auc_ap(torch.rand(4), torch.rand(9), torch.arange(3, dtype=torch.int32)[None])


def test_trainer_logs_the_path(capsys, tmp_path):
    """Trainer._fused_eval_applies on the host: nothing without the flag; with it 'fused' or the reason, printed once."""
    from types import SimpleNamespace
    from gnndelete_amd.framework.trainer.base import Trainer
    off = Trainer(SimpleNamespace(dataset='synth-tiny', unlearning_model='original', checkpoint_dir=str(tmp_path)))
    assert off._fused_eval_applies(5, 9, 5, torch.zeros(3)) is False and 'eval_path' not in off.trainer_log
    tr = Trainer(SimpleNamespace(dataset='synth-tiny', unlearning_model='original', checkpoint_dir=str(tmp_path), fused_eval=True))
    assert tr._fused_eval_applies(5, 9, 5, torch.zeros(3)) is False
    assert tr.trainer_log['eval_path'] == 'torch: the scores are not on the GPU'
    assert tr._fused_eval_applies(5, 9, 5, torch.zeros(3)) is False          # the same reason again: no second line
    out = capsys.readouterr().out
    assert out.count('--fused_eval: the scores are not on the GPU; ranking with the batched torch sort') == 1
    assert tr._fused_eval_applies(5, 9, 5, torch.zeros(3, device='meta')) is False
    assert capsys.readouterr().out.count('--fused_eval: ') == 0


def test_the_entries_are_declared_bound_and_refuse_on_the_host():
    from gnndelete_amd import _lib
    names = ['gd_rank_counts_f32', 'gd_subset_rank_metrics', 'gd_subset_rank_workspace']
    declared = _lib.declared_symbols()
    assert all(n in declared and n in _lib.PROTOTYPES for n in names)
    assert sorted(declared) == sorted(_lib.PROTOTYPES)
    L = _lib.lib()
    assert L.gd_abi_version() == 9
    # two rows (bitmap, prefix) of whole 128-byte lines per subset
    assert L.gd_subset_rank_workspace(1, 1) == 2 * 128 and L.gd_subset_rank_workspace(3, 1024) == 3 * 2 * 128
    assert L.gd_subset_rank_workspace(3, 1025) == 3 * 2 * 256 and L.gd_subset_rank_workspace(0, 5) == 0
    assert L.gd_subset_rank_workspace(500, 70001) == 500 * 2 * 4 * 2208
    assert L.gd_subset_rank_workspace(-1, 5) == -1 and L.gd_subset_rank_workspace(1, 0) == -1 and L.gd_subset_rank_workspace(1, 1 << 31) == -1
    # argument errors come back before any launch: no GPU needed
    E_NULL, E_DIM, E_WS = 1, 2, 4
    assert L.gd_rank_counts_f32(None, 0, None, 5, None, None, None) == E_DIM
    assert L.gd_rank_counts_f32(None, 5, None, 1 << 31, None, None, None) == E_DIM
    assert L.gd_rank_counts_f32(None, 5, None, 0, None, None, None) == 0
    assert L.gd_rank_counts_f32(None, 5, None, 3, None, None, None) == E_NULL
    bad = [dict(k=0), dict(k=11), dict(m=1 << 31), dict(n_ref=0), dict(n_ref=1 << 30), dict(n_sub=-1)]
    for change in bad:
        a = dict(n_sub=2, k=4, m=10, n_ref=3)
        a.update(change)
        assert L.gd_subset_rank_metrics(None, None, None, None, None, 4, a['n_sub'], a['k'], a['m'], a['n_ref'], None, None, None, 1 << 20,
                                        None) == E_DIM, change
    assert L.gd_subset_rank_metrics(None, None, None, None, None, 4, 0, 4, 10, 3, None, None, None, 0, None) == 0
    assert L.gd_subset_rank_metrics(None, None, None, None, None, 4, 2, 4, 10, 3, None, None, None, 1 << 20, None) == E_NULL
    p = 256                                                     # any non-null, aligned value: refused before it is used
    assert L.gd_subset_rank_metrics(p, p, p, p, p, 3, 2, 4, 10, 3, p, p, p, 1 << 20, None) == E_DIM
    assert b'ld_idx=3 below k=4' in L.gd_last_error_string()
    assert L.gd_subset_rank_metrics(p, p, p, p, p, 4, 2, 4, 10, 3, p, p, p + 4, 1 << 20, None) == 3
    assert L.gd_subset_rank_metrics(p, p, p, p, p, 4, 2, 4, 10, 3, p, p, p, 2 * 2 * 128 - 1, None) == E_WS
