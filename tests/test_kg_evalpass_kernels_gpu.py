"""gd_eval_triple_scores_f32 (csrc/evalpass.hip), the scoring kernel of the prepared knowledge-graph validation, on the GPU against
its numpy restatement (gnndelete_amd/evalpass.py: reference_triple_scores, fp64 throughout).

Every logit within
    (d + 2) * 2^-24 * sum_j |z_aj rel_tj z_bj|
of the fp64 DistMult sum: the first-order bound of a d-term fma chain over products that carry one extra rounding (z_a rel is
rounded before the fma; no term passes through more than d + 1 roundings of at most 2^-24 relative each, counting the cross-lane
additions, and every partial sum is at most the sum of the magnitudes).  Every Df / Dr score within 0.25 x that + 2^-21 of the fp64
sigmoid: slope at most 1/4, and four units in the last place of a value at most 1 for expf and the division - the form of the
edge kernel's bound.  Loss, Df mean and Df std within 1e-12 RELATIVE of the restatement on the kernel's own scores (the terms
are formed in double from fp32 inputs and have one sign, so only the order of summation differs).

Shapes, the smallest that reach every form: d in {4, 8, 32, 64, 128, 256} (lane groups of 1, 2, 8, 16, 32 and 64 lanes: every
instantiation but the 4-lane one, which d = 16 adds), row pitches above d for z and for rel, segment boundaries off every group
and wave multiple, each of the four segments empty in turn, and a second trip of the grid-stride loop at both ends of the lane
groups: 4,096 + 37 triples at d = 256 (four per block, 1,024 blocks) and 262,144 + 5 at d = 4 (256 per block)."""
import functools
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
SUM_TOL = 1e-12

CASES = {                       # name: (n, n_rel, d, ld_z, ld_rel, segments, scale of z)
    'one_each_d4': (5, 2, 4, 4, 4, (1, 1, 1, 1), 1.0),
    'off_multiples_d4': (50, 5, 4, 4, 4, (65, 63, 1, 130), 0.9),
    'off_multiples_d8_pitched': (50, 5, 8, 12, 16, (65, 63, 1, 130), 0.8),
    'off_multiples_d16': (50, 5, 16, 16, 16, (65, 63, 1, 130), 0.7),
    'off_multiples_d32': (50, 7, 32, 32, 32, (65, 63, 1, 130), 0.6),
    'off_multiples_d64_pitched': (50, 7, 64, 68, 72, (65, 63, 3, 130), 0.5),
    'off_multiples_d128': (50, 3, 128, 128, 128, (65, 63, 1, 130), 0.4),
    'off_multiples_d256_pitched': (50, 3, 256, 260, 264, (65, 63, 1, 130), 0.3),
    'no_pos_d32': (30, 4, 32, 32, 32, (0, 9, 5, 7), 0.6),
    'no_neg_d32': (30, 4, 32, 32, 32, (9, 0, 5, 7), 0.6),
    'no_df_d32': (30, 4, 32, 32, 32, (7, 5, 0, 9), 0.6),
    'no_dr_d32': (30, 4, 32, 32, 32, (7, 5, 9, 0), 0.6),
    'stage_only_d64': (30, 4, 64, 64, 64, (7, 5, 0, 0), 0.5),
    'saturated_d32': (60, 5, 32, 32, 32, (70, 66, 33, 131), 4.0),      # logits beyond +-100: saturated sigmoids, a large loss
    'two_trips_d256': (300, 6, 256, 256, 256, (2001, 1999, 70, 63), 0.3),             # M = 4,096 + 37
    'two_trips_d4': (900, 6, 4, 4, 4, (100001, 99999, 3000, 59149), 0.9),             # M = 262,144 + 5
}
assert sum(CASES['two_trips_d256'][5]) == 4096 + 37 and sum(CASES['two_trips_d4'][5]) == 262144 + 5
WORST = {'logit': 0.0, 'sigmoid': 0.0}


@functools.lru_cache(maxsize=None)
def _case(name):
    """(z, rel as views of pitched buffers, src, dst, etype, segments) on the host, the restatement's fp64 scores, the fp64 logits
    and the sum of magnitudes the bound is stated in; computed once and shared."""
    from gnndelete_amd.evalpass import reference_triple_scores
    n, n_rel, d, ld_z, ld_rel, segments, scale = CASES[name]
    g = torch.Generator().manual_seed(sum(segments) + d)
    z = (torch.randn(n, ld_z, generator=g) * scale)[:, :d]
    rel = torch.randn(n_rel, ld_rel, generator=g)[:, :d]
    m = sum(segments)
    src, dst, et = torch.randint(0, n, (m,), generator=g), torch.randint(0, n, (m,), generator=g), torch.randint(0, n_rel, (m,), generator=g)
    s64 = reference_triple_scores(z, rel, src, dst, et, segments)[0]
    prod = z.double()[src] * rel.double()[et] * z.double()[dst]
    return z, rel, src, dst, et, segments, s64, prod.sum(1).numpy(), prod.abs().sum(1).numpy()


def _on_gpu(t):
    """A device copy with the view's row pitch."""
    buf = torch.empty(t.shape[0], t.stride(0), device='cuda')
    out = buf[:, :t.shape[1]]
    out.copy_(t)
    return out


def _check(name, d, segments, s64, l64, mag, scores, stats):
    from gnndelete_amd.evalpass import reference_triple_stats
    n_pos, n_neg, n_df, n_dr = segments
    n_stage = n_pos + n_neg
    got = scores.cpu().numpy()
    assert got.dtype == np.float32 and np.isfinite(got).all()
    logit_bound = (d + 2) * 2.0 ** -24 * mag
    err_l = np.abs(got[:n_stage].astype(np.float64) - l64[:n_stage])
    err_s = np.abs(got[n_stage:].astype(np.float64) - s64[n_stage:])
    sig_bound = 0.25 * logit_bound[n_stage:] + 2.0 ** -21
    frac_l = float((err_l / np.maximum(logit_bound[:n_stage], 1e-300)).max(initial=0.0))
    frac_s = float((err_s / sig_bound).max(initial=0.0))
    WORST['logit'], WORST['sigmoid'] = max(WORST['logit'], frac_l), max(WORST['sigmoid'], frac_s)
    print(name, 'logit error / bound: max', frac_l, 'sigmoid error / bound: max', frac_s, '| largest so far', WORST,
          '| largest |logit|', float(np.abs(l64).max()))
    assert (err_l <= logit_bound[:n_stage]).all() and (err_s <= sig_bound).all()
    assert (got[n_stage:] >= 0).all() and (got[n_stage:] <= 1).all()
    loss, mean, std = reference_triple_stats(got, segments)
    k_loss, k_mean, k_std = stats.tolist()
    print(name, 'loss', k_loss, loss, 'df mean', k_mean, mean, 'df std', k_std, std)
    if n_stage:
        assert abs(k_loss - loss) <= SUM_TOL * abs(loss) and k_loss > 0.0
    else:
        assert math.isnan(k_loss) and math.isnan(loss)
    if n_df:
        assert abs(k_mean - mean) <= SUM_TOL * abs(mean) and abs(k_std - std) <= SUM_TOL * std
    else:
        assert math.isnan(k_mean) and math.isnan(k_std)


@pytest.mark.parametrize('name', list(CASES))
def test_triple_scores_match_the_restatement(name):
    from gnndelete_amd.evalpass import eval_triple_scores
    z, rel, src, dst, et, segments, s64, l64, mag = _case(name)
    zd, rd = _on_gpu(z), _on_gpu(rel)
    assert (zd.stride(0), rd.stride(0)) == CASES[name][3:5]
    args = (zd, rd, src.cuda(), dst.cuda(), et.cuda(), segments)
    scores, stats, status = eval_triple_scores(*args)
    assert scores.dtype == torch.float32 and stats.dtype == torch.float64 and status.dtype == torch.int32 and int(status) == 0
    _check(name, z.shape[1], segments, s64, l64, mag, scores, stats)
    again = eval_triple_scores(*args)
    assert torch.equal(scores, again[0]) and torch.equal(status, again[2])
    assert torch.equal(stats.view(torch.int64), again[1].view(torch.int64))            # the same bits, NaN included


def test_saturated_logits_stay_finite():
    """The saturated case reaches beyond +-100: Df / Dr scores exactly 1 and next to 0, a loss far above log 2, nothing NaN."""
    from gnndelete_amd.evalpass import eval_triple_scores
    z, rel, src, dst, et, segments, s64, l64, mag = _case('saturated_d32')
    n_stage = segments[0] + segments[1]
    assert l64.max() > 100 and l64.min() < -100 and l64[:n_stage].max() > 100 and l64[:n_stage].min() < -100
    scores, stats, _ = eval_triple_scores(_on_gpu(z), _on_gpu(rel), src.cuda(), dst.cuda(), et.cuda(), segments)
    got = scores.cpu().numpy()
    assert np.isfinite(got).all() and (got[n_stage:] == 1.0).any() and (got[n_stage:] < 1e-30).any()
    assert np.isfinite(stats.cpu().numpy()).all() and float(stats[0]) > 5.0
    # exact logits +-200 and 0: the terms are 0, 200 and log 2
    z = torch.tensor([[10.0, 0.0, 0.0, 0.0], [-10.0, 0.0, 0.0, 0.0], [0.0, 0.0, 0.0, 0.0]]).cuda()
    rel = torch.tensor([[2.0, 1.0, 1.0, 1.0]]).cuda()
    src, dst, et = torch.tensor([0, 0, 0, 0, 2, 0, 0]).cuda(), torch.tensor([0, 1, 0, 1, 2, 0, 1]).cuda(), torch.zeros(7, dtype=torch.int64).cuda()
    scores, stats, _ = eval_triple_scores(z, rel, src, dst, et, (2, 3, 2, 0))
    assert scores.tolist()[:5] == [200.0, -200.0, 200.0, -200.0, 0.0] and scores[5] == 1.0 and 0.0 <= float(scores[6]) < 1e-37
    assert abs(float(stats[0]) - (0.0 + 200.0 + 200.0 + 0.0 + math.log(2.0)) / 5) <= 1e-12 * 80


@pytest.mark.parametrize('where', ['src', 'dst', 'etype', 'negative'])
def test_an_item_out_of_range_is_refused_and_writes_nothing_outside(where):
    from gnndelete_amd.evalpass import eval_triple_scores, reference_triple_scores
    z, rel, src, dst, et, segments, s64, l64, mag = _case('off_multiples_d64_pitched')
    src, dst, et = src.clone(), dst.clone(), et.clone()
    n_stage, m = segments[0] + segments[1], sum(segments)
    stage_k, dr_k = 70, m - 1                                        # one item of the stage, one of Dr
    for k in (stage_k, dr_k):
        if where == 'src':
            src[k] = z.shape[0]
        elif where == 'dst':
            dst[k] = z.shape[0] + 10 ** 12
        elif where == 'etype':
            et[k] = rel.shape[0]
        else:
            et[k] = -1
    zd, rd = _on_gpu(z), _on_gpu(rel)
    guard = 64
    buf = torch.full((m + 2 * guard,), 7.0, device='cuda')
    args = (zd, rd, src.cuda(), dst.cuda(), et.cuda(), segments)
    with pytest.raises(IndexError, match='outside'):
        eval_triple_scores(*args, out=buf[guard:guard + m])
    scores, stats, status = eval_triple_scores(*args, check=False, out=buf[guard:guard + m])
    assert int(status) == 1 and scores.data_ptr() == buf[guard:].data_ptr()
    assert (buf[:guard] == 7.0).all() and (buf[guard + m:] == 7.0).all()
    assert float(scores[stage_k]) == 0.0 and float(scores[dr_k]) == 0.5         # logit 0: raw in the stage, its sigmoid in Dr
    want = reference_triple_scores(z, rel, src, dst, et, segments)[0]
    keep = np.ones(m, dtype=bool)
    keep[[stage_k, dr_k]] = False
    assert np.abs(scores.cpu().numpy()[keep] - want[keep]).max() <= 1e-4 and want[stage_k] == 0.0 and want[dr_k] == 0.5


def test_the_wrapper_refuses_what_the_kernel_does_not_take():
    from gnndelete_amd import _lib
    from gnndelete_amd.evalpass import eval_triple_scores
    z, rel = torch.zeros(4, 8, device='cuda'), torch.zeros(3, 8, device='cuda')
    e = torch.zeros(3, dtype=torch.int64, device='cuda')
    seg = (1, 1, 1, 0)
    assert int(eval_triple_scores(z, rel, e, e, e, seg)[2]) == 0
    with pytest.raises(ValueError, match='z must be a float32 matrix'):
        eval_triple_scores(z.double(), rel, e, e, e, seg)
    with pytest.raises(ValueError, match='rel must be a float32'):
        eval_triple_scores(z, rel.double(), e, e, e, seg)
    with pytest.raises(ValueError, match='rel must be a float32'):
        eval_triple_scores(z, torch.zeros(3, 4, device='cuda'), e, e, e, seg)                   # another width than z
    with pytest.raises(ValueError, match=r'etype must be int64 \[3\]'):
        eval_triple_scores(z, rel, e, e, e.int(), seg)
    with pytest.raises(ValueError, match=r'dst must be int64 \[3\]'):
        eval_triple_scores(z, rel, e, e[:2], e, seg)
    with pytest.raises(ValueError, match=r'int64 \[4\]'):
        eval_triple_scores(z, rel, e, e, e, (1, 1, 1, 1))                                       # a segment sum that does not match
    with pytest.raises(ValueError, match='out must be'):
        eval_triple_scores(z, rel, e, e, e, seg, out=torch.zeros(2, device='cuda'))
    with pytest.raises(_lib.GnnDeleteHipError, match='multiple of 4'):                          # odd d
        eval_triple_scores(torch.zeros(4, 6, device='cuda'), torch.zeros(3, 6, device='cuda'), e, e, e, seg)
    with pytest.raises(_lib.GnnDeleteHipError, match='multiple of 4'):                          # d = 260
        eval_triple_scores(torch.zeros(4, 260, device='cuda'), torch.zeros(3, 260, device='cuda'), e, e, e, seg)
    misaligned = torch.zeros(3 * 8 + 1, device='cuda')[1:].view(3, 8)                           # rows 4 bytes off a 16-byte boundary
    with pytest.raises(_lib.GnnDeleteHipError, match='unaligned'):
        eval_triple_scores(z, misaligned, e, e, e, seg)
    with pytest.raises(_lib.GnnDeleteHipError, match='16-byte row pitches'):
        eval_triple_scores(z, torch.zeros(3, 10, device='cuda')[:, :8], e, e, e, seg)           # a pitch of 40 bytes
