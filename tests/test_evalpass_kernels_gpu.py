"""The two scoring kernels of --fused_validation (csrc/evalpass.hip) on the GPU against their numpy restatements
(gnndelete_amd/evalpass.py: reference_edge_scores, reference_row_nll_eval; fp64 throughout).

gd_eval_edge_scores_f32.  Every score within
    0.25 * d * 2^-23 * sum_j |z_aj z_bj|  +  2^-21
of sigmoid of the fp64 dot product: the fp32 dot-product bound through a function of slope at most 1/4, and four units in the
last place of a value at most 1 for expf and the division.  Loss, Df mean and Df std within 1e-12 (absolute) of the
restatement ON THE KERNEL'S OWN SCORES: the terms are formed in double from fp32 inputs, lie in [0.31, 1.32] and have one
sign, so only the order of summation differs.  Shapes: d in {4, 64, 68, 256} (lane groups of 1, 16, 32 and 64 lanes; 68 leaves
half of a 32-lane group without a vector), a row pitch above d once, segment boundaries off every group and wave multiple,
empty Df / Dr, one edge per segment.  At d = 4 a pass of the grid covers 1,024 blocks x 256 edges, so the 70,000-edge case
makes one trip of the grid-stride loop; the 263,000-edge case at d = 4 and the 5,000-edge case at d = 256 (four edges per
block) make two.

gd_row_nll_eval_f32.  The hit count equals numpy's argmax count exactly (random rows have no exact ties; one explicit tie case
pins the lowest-index rule).  The kernel forms the row terms in DOUBLE (exp / log in fp64), so the loss is held to 1e-12
relative of the fp64 restatement, not to the 1e-6 an fp32 expf / logf per row would need.  Classes {1, 3, 4, 7, 64, 256}, a
pitch above the class count, lists of 1, 63, 65 and 5,000 rows (5,000 rows of 256 classes: more than one trip)."""
import functools
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
SUM_TOL = 1e-12


# ------------------------------------------------------------------------------------------ gd_eval_edge_scores_f32
EDGE_CASES = {                  # name: (n, d, ld_z, segments, scale of z)
    'one_each_d4': (5, 4, 4, (1, 1, 1, 1), 1.0),
    'off_multiples_d4': (50, 4, 4, (65, 63, 1, 130), 0.8),
    'off_multiples_d64': (50, 64, 64, (65, 63, 1, 130), 0.25),
    'off_multiples_d68_pitched': (50, 68, 76, (65, 63, 1, 130), 0.25),
    'off_multiples_d256': (50, 256, 256, (65, 63, 1, 130), 0.12),
    'no_df_d64': (30, 64, 64, (7, 5, 0, 0), 0.25),
    'no_df_d4': (30, 4, 4, (7, 5, 0, 0), 1.0),
    'seventy_thousand_d4': (900, 4, 4, (30001, 29999, 4001, 6000), 0.9),
    'two_trips_d4': (900, 4, 4, (100001, 99999, 3000, 60000), 0.9),
    'two_trips_d256': (300, 256, 256, (2001, 1999, 501, 499), 0.12),
}


@functools.lru_cache(maxsize=None)
def _edge_case(name):
    """(z [n, d] as a view of a [n, ld] buffer, src, dst, segments) on the host, and the restatement's fp64 scores; shared."""
    from gnndelete_amd.evalpass import reference_edge_scores
    n, d, ld, segments, scale = EDGE_CASES[name]
    g = torch.Generator().manual_seed(sum(segments) + d)
    buf = torch.randn(n, ld, generator=g) * scale
    z = buf[:, :d]
    m = sum(segments)
    src, dst = torch.randint(0, n, (m,), generator=g), torch.randint(0, n, (m,), generator=g)
    s64 = reference_edge_scores(z, src, dst, segments)[0]
    mag = (z.double()[src].abs() * z.double()[dst].abs()).sum(1).numpy()
    return z, src, dst, segments, s64, mag


def _on_gpu(z):
    """A device copy with the view's row pitch."""
    buf = torch.empty(z.shape[0], z.stride(0), device='cuda')
    out = buf[:, :z.shape[1]]
    out.copy_(z)
    return out


def _check_edge_outputs(z, src, dst, segments, s64, mag, scores, stats):
    from gnndelete_amd.evalpass import reference_edge_stats
    d = z.shape[1]
    got = scores.cpu().numpy()
    err = np.abs(got.astype(np.float64) - s64)
    bound = 0.25 * d * 2.0 ** -23 * mag + 2.0 ** -21
    print('score error / bound: max', float((err / bound).max()), 'worst abs', float(err.max()))
    assert got.dtype == np.float32 and np.isfinite(got).all() and (got >= 0).all() and (got <= 1).all()
    assert (err <= bound).all()
    loss, mean, std = reference_edge_stats(got, segments)
    k_loss, k_mean, k_std = stats.tolist()
    print('loss', k_loss, loss, 'df mean', k_mean, mean, 'df std', k_std, std)
    assert abs(k_loss - loss) <= SUM_TOL and 0.31 <= k_loss <= 1.32
    if segments[2]:
        assert abs(k_mean - mean) <= SUM_TOL and abs(k_std - std) <= SUM_TOL
    else:
        assert math.isnan(k_mean) and math.isnan(k_std)


@pytest.mark.parametrize('name', list(EDGE_CASES))
def test_edge_scores_match_the_restatement(name):
    from gnndelete_amd.evalpass import eval_edge_scores
    z, src, dst, segments, s64, mag = _edge_case(name)
    zd = _on_gpu(z)
    assert zd.stride(0) == EDGE_CASES[name][2]
    scores, stats, status = eval_edge_scores(zd, src.cuda(), dst.cuda(), segments)
    assert scores.dtype == torch.float32 and stats.dtype == torch.float64 and status.dtype == torch.int32 and int(status) == 0
    _check_edge_outputs(z, src, dst, segments, s64, mag, scores, stats)
    again = eval_edge_scores(zd, src.cuda(), dst.cuda(), segments)
    assert torch.equal(scores, again[0]) and torch.equal(status, again[2])
    assert torch.equal(stats.view(torch.int64), again[1].view(torch.int64))            # the same bits, NaN included


def test_saturated_logits_stay_finite():
    """Rows scaled so that the logits reach +-100: scores exactly 1 / next to 0, finite terms, no NaN."""
    from gnndelete_amd.evalpass import eval_edge_scores, reference_edge_scores
    z = torch.tensor([[5.0, 5.0, 5.0, 5.0], [-5.0, -5.0, -5.0, -5.0], [0.0, 0.0, 0.0, 0.0], [0.5, -0.5, 0.25, 0.0],
                      [2.0, 2.0, 2.0, 2.0]])
    src = torch.tensor([0, 0, 2, 3, 0, 1, 0, 1, 3, 4, 4])
    dst = torch.tensor([0, 1, 2, 3, 1, 1, 0, 0, 0, 0, 1])          # logits 100, -100, 0, .5625, -100, 100, 100, -100, 1.25, 40, -40
    segments = (4, 3, 2, 2)
    scores, stats, status = eval_edge_scores(z.cuda(), src.cuda(), dst.cuda(), segments)
    got = scores.tolist()
    assert int(status) == 0 and all(math.isfinite(v) for v in got) and all(math.isfinite(v) for v in stats.tolist())
    assert got[0] == 1.0 and got[5] == 1.0 and got[6] == 1.0 and got[2] == 0.5 and got[9] == 1.0
    assert all(0.0 <= got[i] < 1e-38 for i in (1, 4, 7)) and 0.0 < got[10] < 1e-17
    s64 = reference_edge_scores(z, src, dst, segments)[0]
    mag = (z.double()[src].abs() * z.double()[dst].abs()).sum(1).numpy()
    _check_edge_outputs(z, src, dst, segments, s64, mag, scores, stats)


def test_all_equal_df_scores_have_no_spread():
    """Unlearning drives the Df scores together: two passes (mean, then squared deviations) leave std at rounding level."""
    from gnndelete_amd.evalpass import eval_edge_scores
    z = torch.randn(40, 8, generator=torch.Generator().manual_seed(5)) * 0.4
    n_df = 3000
    src = torch.cat([torch.arange(10), torch.arange(10, 20), torch.full((n_df,), 7), torch.arange(5)])
    dst = torch.cat([torch.arange(10) + 1, torch.arange(10, 20) + 3, torch.full((n_df,), 9), torch.arange(5) + 20])
    scores, stats, status = eval_edge_scores(z.cuda(), src.cuda(), dst.cuda(), (10, 10, n_df, 5))
    _, mean, std = stats.tolist()
    df = scores[20:20 + n_df]
    assert int(status) == 0 and bool((df == df[0]).all())
    assert std <= 1e-15 and abs(mean - float(df[0])) <= 1e-15


@pytest.mark.parametrize('where', ['src', 'dst'])
def test_an_endpoint_out_of_range_is_refused_and_writes_nothing_outside(where):
    from gnndelete_amd.evalpass import eval_edge_scores
    z, src, dst, segments, s64, mag = _edge_case('off_multiples_d64')
    src, dst = src.clone(), dst.clone()
    (src if where == 'src' else dst)[131] = z.shape[0] if where == 'src' else -1
    m, guard = sum(segments), 64
    buf = torch.full((guard + m + guard,), 7.25, device='cuda')
    zd = _on_gpu(z)
    with pytest.raises(IndexError, match='outside'):
        eval_edge_scores(zd, src.cuda(), dst.cuda(), segments, out=buf[guard:guard + m])
    scores, stats, status = eval_edge_scores(zd, src.cuda(), dst.cuda(), segments, check=False, out=buf[guard:guard + m])
    assert int(status) == 1 and scores.data_ptr() == buf[guard:].data_ptr()
    assert bool((buf[:guard] == 7.25).all()) and bool((buf[guard + m:] == 7.25).all())            # guard words either side
    got = scores.cpu().numpy()
    assert got[131] == 0.5                                                                        # logit 0, nothing read
    keep = np.arange(m) != 131
    bound = 0.25 * 64 * 2.0 ** -23 * mag + 2.0 ** -21
    assert (np.abs(got.astype(np.float64) - s64)[keep] <= bound[keep]).all()
    # the flag is written on every call: a clean list afterwards reports 0
    clean = eval_edge_scores(zd, _edge_case('off_multiples_d64')[1].cuda(), _edge_case('off_multiples_d64')[2].cuda(), segments, check=False)
    assert int(clean[2]) == 0


def test_the_wrapper_refuses_what_the_kernel_does_not_take():
    from gnndelete_amd import _lib
    from gnndelete_amd.evalpass import eval_edge_scores
    z = torch.zeros(4, 8, device='cuda')
    e = torch.zeros(3, dtype=torch.int64, device='cuda')
    with pytest.raises(ValueError, match='float32 matrix'):
        eval_edge_scores(z.double(), e, e, (1, 1, 1, 0))
    with pytest.raises(ValueError, match=r'int64 \[3\]'):
        eval_edge_scores(z, e, e[:2], (1, 1, 1, 0))
    with pytest.raises(ValueError, match='out must be'):
        eval_edge_scores(z, e, e, (1, 1, 1, 0), out=torch.zeros(2, device='cuda'))
    with pytest.raises(_lib.GnnDeleteHipError, match='multiple of 4'):
        eval_edge_scores(torch.zeros(4, 6, device='cuda'), e, e, (1, 1, 1, 0))


# ------------------------------------------------------------------------------------------ gd_row_nll_eval_f32
NLL_CASES = {                   # name: (n_rows, classes, pitch, listed rows)
    'c1_one_row': (9, 1, 1, 1),
    'c3_63': (100, 3, 3, 63),
    'c4_65_pitched': (100, 4, 7, 65),
    'c7_65': (100, 7, 7, 65),
    'c64_63_pitched': (100, 64, 70, 63),
    'c256_65': (100, 256, 256, 65),
    'c7_5000': (6000, 7, 7, 5000),
    'c256_5000_pitched': (6000, 256, 260, 5000),
}


@functools.lru_cache(maxsize=None)
def _nll_case(name):
    from gnndelete_amd.evalpass import reference_row_nll_eval
    n, c, pitch, n_sel = NLL_CASES[name]
    g = torch.Generator().manual_seed(n_sel + c)
    buf = torch.randn(n, pitch, generator=g) * 3
    y = torch.randint(0, c, (n,), generator=g)
    rows = torch.randperm(n, generator=g)[:n_sel].to(torch.int32)
    z = buf[:, :c]
    srt = z.sort(1).values
    assert c == 1 or bool((srt[:, -1] > srt[:, -2]).all())                                        # no exact ties at the top
    return z, rows, y, reference_row_nll_eval(z, rows, y)


@pytest.mark.parametrize('name', list(NLL_CASES))
def test_row_nll_eval_matches_the_restatement(name):
    from sklearn.metrics import accuracy_score
    from gnndelete_amd.evalpass import read_row_nll_eval, row_nll_eval
    z, rows, y, (want_loss, want_correct) = _nll_case(name)
    zd = _on_gpu(z)
    assert zd.stride(0) == NLL_CASES[name][2]
    out = row_nll_eval(zd, rows.cuda(), y.cuda())
    loss, correct = read_row_nll_eval(out)
    print(name, 'loss', loss, want_loss, 'correct', correct, want_correct)
    assert correct == want_correct == int((z[rows.long()].double().numpy().argmax(1) == y[rows.long()].numpy()).sum())
    assert abs(loss - want_loss) <= SUM_TOL * abs(want_loss) if want_loss else loss == 0.0
    assert correct / rows.numel() == accuracy_score(y[rows.long()], z[rows.long()].argmax(1))
    assert torch.equal(out.view(torch.int64), row_nll_eval(zd, rows.cuda(), y.cuda()).view(torch.int64))


def test_row_nll_eval_edges():
    """Ties take the lowest index; a label out of range counts as wrong with term 0; a row id out of range is skipped; the empty
    list gives NaN and 0; d_valid below the width ignores the columns beyond it."""
    from gnndelete_amd.evalpass import read_row_nll_eval, reference_row_nll_eval, row_nll_eval
    z = torch.tensor([[1.0, 2.0, 2.0, 0.0, 2.0], [0.5, 0.5, 0.5, 0.5, 0.5], [3.0, 1.0, 3.0, 0.0, 0.0], [0.0, 9.0, 0.0, 0.0, 0.0],
                      [0.0, 0.0, 0.0, 0.0, 7.0], [-50.0, 60.0, -50.0, 0.0, 0.0]])
    y = torch.tensor([1, 0, 2, 5, 4, 0])
    zd, yd = z.cuda(), y.cuda()

    def run(rows, d_valid=None, labels=yd):
        return read_row_nll_eval(row_nll_eval(zd, torch.tensor(rows, dtype=torch.int32).cuda(), labels, d_valid))
    lse = torch.logsumexp(z.double(), 1)
    loss, correct = run([0, 1, 2])
    assert correct == 2                                             # row 0 -> 1 (hit), row 1 -> 0 (hit), row 2 -> 0, label 2 (miss)
    assert abs(loss - float((lse[0] - 2 + lse[1] - 0.5 + lse[2] - 3) / 3)) <= 1e-15
    for rows in ([0, 1, 2], [0, 3, 17, -1], [4], [3], [5]):
        want = reference_row_nll_eval(z, rows, y)
        got = run(rows)
        assert got[1] == want[1] and abs(got[0] - want[0]) <= SUM_TOL * max(abs(want[0]), 1e-300), rows
    assert run([0, 3, 17, -1])[1] == 1 and abs(run([0, 3, 17, -1])[0] - float(lse[0] - 2) / 4) <= 1e-15
    assert abs(run([5])[0] - 110.0) <= 1e-12                       # a confidently wrong row: m - z_y + log(sum), no overflow
    loss, correct = run([])
    assert math.isnan(loss) and correct == 0
    # the first 4 columns only: row 4's maximum (column 4) and label 4 are outside
    assert run([4], 4) == reference_row_nll_eval(z, [4], y, 4) == (0.0, 0)
    zeros = torch.zeros(6, dtype=torch.int64).cuda()
    assert run([3], 1, zeros) == (0.0, 1) and run([2], 2, zeros)[1] == 1
