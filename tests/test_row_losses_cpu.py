"""The folded KLD / cosine row losses of the fused Del step (--fused_row_losses), the parts that need no GPU: the flag, the
per-row fold of engine.fold_row_terms against unfolded fp64 autograd, and the conversion of the raw device sums into the logged
loss values."""
import pytest
import torch
import torch.nn.functional as F

from gnndelete_amd.engine import LOSS_FAMILIES, fold_row_terms, logged_loss, padded_class_width
from gnndelete_amd.framework.training_args import EXTRA_FLAGS, build_parser


def test_fused_row_losses_flag_parses_and_defaults_off():
    assert build_parser().parse_args([]).fused_row_losses is False
    assert build_parser().parse_args(['--loss_fct', 'kld_mean', '--fused_row_losses']).fused_row_losses is True
    assert 'fused_row_losses' in [f[0] for f in EXTRA_FLAGS]
    assert not hasattr(build_parser(extra=False).parse_args([]), 'fused_row_losses')


def test_padded_class_width_follows_the_engine_switch(monkeypatch):
    """What the trainer asks before it promises the fused step: the width the engine will hand gd_rowfold_loss_f32."""
    monkeypatch.delenv('GD_PAD_OUT', raising=False)
    assert padded_class_width(128, 7) == 64 and padded_class_width(128, 4) == 64 and padded_class_width(128, 40) == 40
    assert padded_class_width(64, 7) == 7 and padded_class_width(128, 7, rgcn=True) == 7
    monkeypatch.setenv('GD_PAD_OUT', '32')
    assert padded_class_width(128, 7) == 32
    monkeypatch.setenv('GD_PAD_OUT', '0')
    assert padded_class_width(128, 7) == 7


def _terms(seed, n=40, d=12, n_terms=90):
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(n, d, generator=g, dtype=torch.float64)
    z_ori = torch.randn(n, d, generator=g, dtype=torch.float64) * 2
    # DEC rows 0..14 (several terms each), NI rows 20..39 (one term each, target = the row itself): disjoint, as the masks are
    rows_r = torch.randint(0, 15, (n_terms,), generator=g)
    tgt_r = torch.randint(0, n, (n_terms,), generator=g)
    rows_l = torch.arange(20, 40)[torch.randperm(20, generator=g)]
    rows = torch.cat([rows_r, rows_l])
    tgt = torch.cat([tgt_r, rows_l])
    kind = torch.cat([torch.zeros(n_terms, dtype=torch.int32), torch.ones(20, dtype=torch.int32)])
    return z, z_ori, rows, tgt, kind


def _unfolded_sum(family, z, z_ori, rows, tgt, d_valid):
    a, b = z[rows][:, :d_valid], z_ori[tgt][:, :d_valid]
    if family == 'kld':
        return F.kl_div(F.log_softmax(a, -1), b.softmax(-1), reduction='sum')
    return (1 - F.cosine_similarity(a, b)).sum()


def _folded_sum(family, z, uniq, tm, c, sel, d_valid):
    zz, tt, cc = z[uniq[sel]][:, :d_valid], tm[sel][:, :d_valid], c[sel].double()
    if family == 'kld':
        return (torch.special.xlogy(tt, tt / cc[:, None]) - tt * F.log_softmax(zz, -1)).sum()
    return (cc - (zz * tt).sum(1) / zz.norm(dim=1).clamp(min=1e-8)).sum()


@pytest.mark.parametrize('family', ['kld', 'cosine'])
@pytest.mark.parametrize('d_valid', [12, 5])
def test_fold_matches_unfolded_fp64_autograd(family, d_valid):
    z, z_ori, rows, tgt, kind = _terms(3)
    if family == 'cosine':
        z_ori[7] = 0.0                                                    # a target under the norm clamp
    uniq, tm, c, kind_u, k = fold_row_terms(family, z_ori, rows, tgt, kind, d_valid)
    assert tm.dtype == torch.float64 and tm.shape == (uniq.numel(), 12) and int(c.sum()) == rows.numel()
    assert bool((tm[:, d_valid:] == 0).all())
    assert int(c.max()) > 2 and set(kind_u.tolist()) == {0, 1}
    for kd in (0, 1):
        zr = z.clone().requires_grad_(True)
        ref = _unfolded_sum(family, zr, z_ori, rows[kind == kd], tgt[kind == kd], d_valid)
        g_ref, = torch.autograd.grad(ref, zr)
        zf = z.clone().requires_grad_(True)
        got = _folded_sum(family, zf, uniq, tm, c, kind_u == kd, d_valid) + k[kd]
        g_got, = torch.autograd.grad(got, zf)
        torch.testing.assert_close(got, ref, rtol=1e-12, atol=1e-12)
        torch.testing.assert_close(g_got, g_ref, rtol=1e-11, atol=1e-13)
    assert k[0] >= 0.0 and k[1] == pytest.approx(0.0, abs=1e-12)         # rows with one term: nothing to fold
    if family == 'cosine':
        assert k == [0.0, 0.0]


def test_fold_order_is_fixed_and_empty_request_folds_to_nothing():
    z, z_ori, rows, tgt, kind = _terms(5)
    a = fold_row_terms('kld', z_ori, rows, tgt, kind)
    b = fold_row_terms('kld', z_ori, rows, tgt, kind)
    assert torch.equal(a[1], b[1]) and a[4] == b[4]
    e = torch.zeros(0, dtype=torch.long)
    uniq, tm, c, kind_u, k = fold_row_terms('cosine', z_ori, e, e, e.to(torch.int32))
    assert uniq.numel() == 0 and tm.shape == (0, 12) and k == [0.0, 0.0]


@pytest.mark.parametrize('name', ['kld_mean', 'kld_sum', 'cosine_mean', 'cosine_sum', 'mse_mean'])
def test_raw_sums_convert_to_the_logged_values(name):
    family, reduction = LOSS_FAMILIES[name]
    z, z_ori, rows, tgt, kind = _terms(11)
    sel = kind == 0
    a, b = z[rows[sel]], z_ori[tgt[sel]]
    n_terms = int(sel.sum())
    if family == 'mse':
        ref = F.mse_loss(a, b, reduction=reduction)
        raw, k, n = ((a - b) ** 2).sum() - 3.0, 3.0, (n_terms * a.shape[1] if reduction == 'mean' else 1)
    else:
        uniq, tm, c, kind_u, kc = fold_row_terms(family, z_ori, rows, tgt, kind)
        raw, k, n = _folded_sum(family, z, uniq, tm, c, kind_u == 0, 12), kc[0], (n_terms if reduction == 'mean' else 1)
        if family == 'kld':
            ref = 1 - torch.exp(-F.kl_div(F.log_softmax(a, -1), b.softmax(-1), reduction='batchmean' if reduction == 'mean' else 'sum'))
        else:
            ref = (1 - F.cosine_similarity(a, b)).mean() if reduction == 'mean' else (1 - F.cosine_similarity(a, b)).sum()
    got = logged_loss(family, torch.stack([raw, raw]), k, n)
    torch.testing.assert_close(got, torch.stack([ref, ref]), rtol=1e-12, atol=1e-13)
