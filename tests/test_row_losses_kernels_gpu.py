"""gd_rowfold_loss_f32 / gd_rowfold_kld_scale_f32 (the folded bounded-KLD and cosine-distance row losses of the fused Del step)
through the C ABI, against fp64 torch autograd on the UNFOLDED terms - F.kl_div(F.log_softmax(z[rows]), softmax(o[tgt])) and
F.cosine_similarity - with the fold done here in fp64.

Tolerances are those tests/test_kernels_gpu.py holds gd_rowpair_loss_f32 to against the same fp64 expressions: 1e-5 (relative
L2) on values, 1e-4 on gradients."""
import pytest
import torch
import torch.nn.functional as F

from helpers import rel_l2

pytestmark = pytest.mark.gpu
TOL = 1e-5
N = 500
W = (0.3, 0.7)                      # coef_DEC, coef_NI inside the differentiated loss
COSINE, KLD = 0, 1


def _case(family, d, d_valid, n_rows, kinds='both', reduction='mean', seed=0, extreme=True):
    """A request of n_rows touched rows (not ascending) with 1, 2 or 7 terms each, one kind per row."""
    g = torch.Generator().manual_seed(1000 * d + 10 * n_rows + seed + family)
    z = torch.randn(N, d, generator=g) * 2
    o = torch.randn(N, d, generator=g) * 2
    row_idx = torch.randperm(N, generator=g)[:n_rows]
    if n_rows > 2:
        assert not bool((row_idx[1:] > row_idx[:-1]).all())
    cnt = torch.tensor([1, 2, 7])[torch.arange(n_rows) % 3]
    kind = {'both': (torch.arange(n_rows) // 2) % 2, 'dec': torch.zeros(n_rows, dtype=torch.long),
            'ni': torch.ones(n_rows, dtype=torch.long)}[kinds]
    if n_rows:
        if family == COSINE:
            z[row_idx[0]] = 0.0                                   # the clamp path
        elif n_rows >= 37 and extreme:                            # (alone in a 'mean' it would push exp(-KL / n) under fp32's range)
            z[row_idx[n_rows - 1]] = torch.where(torch.rand(d, generator=g) < 0.5, -80.0, 80.0)     # stable softmax or inf / NaN
            z[row_idx[n_rows - 1], 0] = 80.0
    t_row = torch.repeat_interleave(torch.arange(n_rows), cnt)           # term -> touched row
    tgt = torch.randint(0, N, (t_row.numel(),), generator=g)
    n_kind = [max(1, int((kind[t_row] == k).sum())) if reduction == 'mean' else 1 for k in (0, 1)]
    return dict(family=family, d=d, dv=d_valid, z=z, o=o, row_idx=row_idx, cnt=cnt, kind=kind, t_row=t_row, tgt=tgt, n_kind=n_kind,
                n_rows=n_rows)


def _oracle(c):
    """fp64 autograd on the unfolded terms: per-kind raw sums (sum of KL / of 1 - cos), the bounded loss' gradient w.r.t. z,
    the two KLD scales, and the fold (tm, K per kind) in fp64."""
    dv, fam = c['dv'], c['family']
    z = c['z'].double().requires_grad_(True)
    o = c['o'].double()
    rows_t = c['row_idx'][c['t_row']]
    kind_t = c['kind'][c['t_row']]
    sums, loss, scales = [], z.sum() * 0, []
    for k in (0, 1):
        a, b = z[rows_t[kind_t == k]][:, :dv], o[c['tgt'][kind_t == k]][:, :dv]
        if fam == KLD:
            s = F.kl_div(F.log_softmax(a, -1), b.softmax(-1), reduction='sum')
            loss = loss + W[k] * (1 - torch.exp(-s / c['n_kind'][k]))
            scales.append(float(torch.exp(-s / c['n_kind'][k]) / c['n_kind'][k]) if a.shape[0] else None)
        else:
            s = (1 - F.cosine_similarity(a, b)).sum()
            loss = loss + W[k] * s / c['n_kind'][k]
        sums.append(float(s))
    loss.backward()
    # the fold, in fp64
    u = c['n_rows']
    tm = torch.zeros(u, c['d'], dtype=torch.float64)
    k_const = [0.0, 0.0]
    ot = o[c['tgt']][:, :dv]
    if fam == KLD:
        t = ot.softmax(-1)
        tm[:, :dv].index_add_(0, c['t_row'], t)
        ent = torch.zeros(u, dtype=torch.float64).index_add_(0, c['t_row'], torch.special.xlogy(t, t).sum(1))
        k_row = ent - torch.special.xlogy(tm, tm / c['cnt'][:, None].double()).sum(1)
        k_const = [float(k_row[c['kind'] == k].sum()) for k in (0, 1)]
    else:
        tm[:, :dv].index_add_(0, c['t_row'], ot / ot.norm(dim=1, keepdim=True).clamp(min=1e-8))
    return dict(sums=sums, grad=z.grad, scales=scales, tm=tm, k=k_const)


def _run(c, ref, with_dz=True, pad=8):
    """Pass A (+ pass B for KLD) on pitched z / dz with NaN in the gap.  -> (raw sums [2], dz [N, d] or None, scales or None)."""
    from gnndelete_amd import _lib
    from gnndelete_amd._lib import check, ptr, stream_ptr
    L = _lib.lib()
    dev = torch.device('cuda')
    d, u, fam = c['d'], c['n_rows'], c['family']
    zp = torch.full((N, d + pad), float('nan'), device=dev)
    zp[:, :d] = c['z'].to(dev)
    dzp = torch.full((N, d + pad), float('nan'), device=dev)
    dzp[:, :d] = -3.0
    zv, dz = zp[:, :d], dzp[:, :d]
    tm = ref['tm'].float().to(dev).contiguous()
    row_idx = c['row_idx'].to(torch.int32).to(dev)
    cnt = c['cnt'].float().to(dev)
    kind = c['kind'].to(torch.int32).to(dev)
    wk = torch.tensor(W)[c['kind']]
    coef = (wk if fam == KLD else wk / torch.tensor(c['n_kind'], dtype=torch.float32)[c['kind']]).float().to(dev)
    nb = L.gd_rowfold_loss_blocks(u)
    assert nb == (u + 255) // 256
    part = torch.full((2 * max(1, nb),), 5.0, device=dev)
    st = stream_ptr(dev)
    check(L.gd_rowfold_loss_f32(fam, ptr(zv), zv.stride(0), ptr(tm), d, c['dv'], ptr(row_idx), ptr(coef), ptr(cnt), ptr(kind), u,
                                ptr(dz) if with_dz else None, dz.stride(0) if with_dz else 0, ptr(part), st), 'gd_rowfold_loss_f32')
    scales = None
    if fam == KLD:
        scales = torch.full((2,), -1.0, device=dev)
        inv = [1.0 / c['n_kind'][k] if bool((c['kind'] == k).any()) else 0.0 for k in (0, 1)]
        check(L.gd_rowfold_kld_scale_f32(ptr(part), nb, ref['k'][0], ref['k'][1], inv[0], inv[1], ptr(row_idx), ptr(kind), u, d,
                                         ptr(dz) if with_dz else None, dz.stride(0) if with_dz else 0, ptr(scales), st),
              'gd_rowfold_kld_scale_f32')
    torch.cuda.synchronize()
    assert bool(torch.isnan(zp[:, d:]).all()) and bool(torch.isnan(dzp[:, d:]).all())          # the gap stays NaN
    sums = part[:2 * nb].double().cpu().view(-1, 2).sum(0) if nb else torch.zeros(2, dtype=torch.float64)
    return sums, (dz.cpu() if with_dz else None), (scales.cpu() if scales is not None else None)


def _check(c, ref, sums, dz, scales):
    fam, d, dv = c['family'], c['d'], c['dv']
    for k in (0, 1):
        present = bool((c['kind'] == k).any())
        if not present:
            assert float(sums[k]) == 0.0                                    # the other kind's sum is exactly 0
            continue
        got = float(sums[k]) + ref['k'][k]
        print(f'family {fam} d {d} d_valid {dv} rows {c["n_rows"]} kind {k}: sum {got:.9g} oracle {ref["sums"][k]:.9g}')
        assert abs(got - ref['sums'][k]) <= TOL * abs(ref['sums'][k]), (k, got, ref['sums'][k])
        if fam == KLD:
            assert abs(float(scales[k]) - ref['scales'][k]) <= TOL * ref['scales'][k], (k, float(scales[k]), ref['scales'][k])
    if dz is None:
        return
    touched = torch.zeros(N, dtype=torch.bool)
    touched[c['row_idx']] = True
    assert bool((dz[~touched] == -3.0).all())                               # only the touched rows are written
    assert bool(torch.isfinite(dz).all())
    if dv < d:
        assert bool((dz[touched][:, dv:] == 0).all())                       # zero behind d_valid
    want = ref['grad']
    rows = c['row_idx']
    if fam == COSINE and c['n_rows']:
        r0 = rows[0]                                                        # the all-zero row: -coef U / 1e-8, finite, the oracle's
        assert float(want[r0].abs().max()) > 1e3
        assert rel_l2(dz[r0], want[r0]) < 10 * TOL
        rows = rows[1:]
    if rows.numel():
        assert rel_l2(dz[rows], want[rows]) < 10 * TOL


# (d_valid < d is the KLD case: zero padding adds nothing to the dots and norms of the cosine distance)
@pytest.mark.parametrize('n_rows', [0, 1, 37, 300])
@pytest.mark.parametrize('family,d,d_valid', [(f, d, d) for f in (COSINE, KLD) for d in (4, 16, 64, 128)] + [(KLD, 64, 4)])
def test_folded_row_losses_match_unfolded_fp64_autograd(family, d, d_valid, n_rows):
    c = _case(family, d, d_valid, n_rows)
    ref = _oracle(c)
    sums, dz, scales = _run(c, ref)
    _check(c, ref, sums, dz, scales)
    if n_rows == 0:
        assert bool((dz == -3.0).all())
        return
    # the same sums without a gradient buffer, and the same bits from run to run
    sums0, none, scales0 = _run(c, ref, with_dz=False)
    assert none is None and torch.equal(sums0, sums) and (scales is None or torch.equal(scales0, scales))
    sums2, dz2, scales2 = _run(c, ref)
    assert torch.equal(sums2, sums) and torch.equal(dz2, dz) and (scales is None or torch.equal(scales2, scales))


@pytest.mark.parametrize('n_rows', [37, 300])
@pytest.mark.parametrize('d,d_valid', [(16, 16), (128, 128), (64, 4)])
def test_kld_both_kinds_without_the_extreme_row(d, d_valid, n_rows):
    """The row of +-80 entries dominates the KLD sum of its kind in the cases above, so the relative bound on that kind's sum
    and scale says little about the kind's other rows there: the same requests without that row."""
    c = _case(KLD, d, d_valid, n_rows, extreme=False)
    assert float(c['z'].abs().max()) < 20 and bool((c['kind'] == 0).any()) and bool((c['kind'] == 1).any())
    ref = _oracle(c)
    _check(c, ref, *_run(c, ref))


@pytest.mark.parametrize('reduction', ['mean', 'sum'])
@pytest.mark.parametrize('kinds', ['dec', 'ni'])
@pytest.mark.parametrize('family', [COSINE, KLD])
def test_one_kind_only_and_sum_reduction(family, kinds, reduction):
    c = _case(family, 32, 32, 37, kinds=kinds, reduction=reduction, seed=3)
    if family == KLD and reduction == 'sum':
        c['z'], c['o'] = 0.05 * c['z'], 0.05 * c['o']       # (small logits: keeps exp(-KL_sum) far from underflow, as a real request is)
    ref = _oracle(c)
    sums, dz, scales = _run(c, ref)
    _check(c, ref, sums, dz, scales)
    if family == KLD:
        assert float(scales[1 if kinds == 'dec' else 0]) == 0.0


def test_refusals():
    from gnndelete_amd import _lib
    from gnndelete_amd._lib import ptr, stream_ptr
    L = _lib.lib()
    dev = torch.device('cuda')
    z, tm, dz = torch.zeros(8, 16, device=dev), torch.zeros(4, 16, device=dev), torch.zeros(8, 16, device=dev)
    ri, kd = torch.arange(4, dtype=torch.int32, device=dev), torch.zeros(4, dtype=torch.int32, device=dev)
    f = torch.ones(4, device=dev)
    part, sc = torch.zeros(2, device=dev), torch.zeros(2, device=dev)

    def a(family=1, d=16, d_valid=16, z_=z, ld=16):
        return L.gd_rowfold_loss_f32(family, ptr(z_), ld, ptr(tm), d, d_valid, ptr(ri), ptr(f), ptr(f), ptr(kd), 4, ptr(dz), 16, ptr(part),
                                     stream_ptr(dev))
    assert a() == 0
    for kw, needle in ((dict(family=2), b'family'), (dict(d=10, d_valid=10), b'multiple of 4'), (dict(d_valid=17), b'd_valid'),
                       (dict(d_valid=0), b'd_valid'), (dict(d=132, d_valid=132), b'multiple of 4'), (dict(z_=None), b'null'),
                       (dict(ld=8), b'stride')):
        rc = a(**kw)
        assert rc > 0 and needle in L.gd_last_error_string(), (kw, rc, L.gd_last_error_string())
    b_ok = L.gd_rowfold_kld_scale_f32(ptr(part), 1, 0.0, 0.0, 1.0, 1.0, ptr(ri), ptr(kd), 4, 16, ptr(dz), 16, ptr(sc), stream_ptr(dev))
    assert b_ok == 0
    rc = L.gd_rowfold_kld_scale_f32(ptr(part), 3, 0.0, 0.0, 1.0, 1.0, ptr(ri), ptr(kd), 4, 16, ptr(dz), 16, ptr(sc), stream_ptr(dev))
    assert rc > 0 and b'n_blocks' in L.gd_last_error_string()
    rc = L.gd_rowfold_kld_scale_f32(ptr(part), 1, 0.0, 0.0, 1.0, 1.0, ptr(ri), ptr(kd), 4, 6, ptr(dz), 16, ptr(sc), stream_ptr(dev))
    assert rc > 0 and b'multiple of 4' in L.gd_last_error_string()
    rc = L.gd_rowfold_kld_scale_f32(ptr(part), 1, 0.0, 0.0, 1.0, 1.0, ptr(ri), ptr(kd), 4, 16, ptr(dz), 16, None, stream_ptr(dev))
    assert rc > 0 and b'scales' in L.gd_last_error_string()
    torch.cuda.synchronize()
