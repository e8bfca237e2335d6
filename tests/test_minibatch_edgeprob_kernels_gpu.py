"""gd_edgeprob_batch_loss_f32 (csrc/edgeprob.hip), the loss stage of the edge-probability GraphSAINT batch step, against an
fp64 numpy restatement: both losses, the logit gradients in decoded order [Df edges | negatives | candidates], the decoded
list itself ((-1, -1) for a candidate with src >= dst), the incidence list over it, the gradients in incidence order and,
through gd_edge_dot_bwd_f32, dL/dz.

The bound is TOL = 1e-5 (tests/test_edgeprob_kernels_gpu.py, from tests/test_kernels_gpu.py): z and z_ori are independent
randn tables, so no difference is a cancellation, and the restatement run in fp32 on the CPU meets the same bound
(test_fp32_restatement_meets_the_bound).  Everything else here is an equality of bits or of integers.

Measured on an MI355X, the largest rel. distance to fp64 over all cases: losses 1.5e-6, w rel-L2 6.2e-7, dz rel-L2 6.3e-7."""
import numpy as np
import pytest
import torch

from helpers import rel_l2

pytestmark = pytest.mark.gpu
TOL = 1e-5
N = 300
SEED = 5                                    # of the parametrised cases' inputs: see test_fp32_restatement_meets_the_bound


def _L():
    from gnndelete_amd import _lib
    return _lib.lib()


def _st():
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    return None if t is None or t.numel() == 0 else t.data_ptr()


def _call(z, z_ori, pos, neg, cs, cd, incidence=True, coef=(0.5, 0.5)):
    """The entry on device tensors -> dict(losses [3], w, dec, and with incidence: inc_ptr, other, src_edge, w_inc, total)."""
    from gnndelete_amd import _lib
    L = _L()
    n, d, k, n_c = z.shape[0], z.shape[1], pos.shape[1], cs.shape[0]
    n_w = 2 * k + n_c
    out = dict(losses=torch.full((3,), -9.0, device='cuda'), w=torch.full((max(n_w, 1),), float('nan'), device='cuda'),
               dec=torch.full((2, max(n_w, 1) + 3), -5, dtype=torch.int64, device='cuda'))
    ws = torch.empty(L.gd_edgeprob_batch_loss_workspace(k, n_c, d), device='cuda')
    inc = [None] * 5
    if incidence:
        out['inc_ptr'] = torch.full((n + 1,), 9, dtype=torch.int64, device='cuda')
        out['other'], out['src_edge'] = (torch.full((max(2 * n_w, 1),), -7, dtype=torch.int32, device='cuda') for _ in range(2))
        out['w_inc'] = torch.full((max(2 * n_w, 1),), float('nan'), device='cuda')
        inc_ws = torch.empty(L.gd_edge_incidence_workspace(n, n_w), dtype=torch.uint8, device='cuda')
        inc = [out['inc_ptr'].data_ptr(), out['other'].data_ptr(), out['src_edge'].data_ptr(), out['w_inc'].data_ptr(),
               inc_ws.data_ptr()]
    _lib.check(L.gd_edgeprob_batch_loss_f32(z.data_ptr(), z.stride(0), n, z_ori.data_ptr(), z_ori.stride(0), z_ori.shape[0], d,
                                            _p(pos), pos.stride(0), _p(neg), neg.stride(0), k, _p(cs), _p(cd), n_c, coef[0], coef[1],
                                            out['dec'].data_ptr(), out['dec'].stride(0), out['w'].data_ptr(),
                                            out['losses'].data_ptr(), *inc, inc_ws.numel() if incidence else 0, ws.data_ptr(),
                                            _st()), 'gd_edgeprob_batch_loss_f32')
    out['w'], out['dec'] = out['w'][:n_w], out['dec'][:, :n_w]
    if incidence:
        out['total'] = int(out['inc_ptr'][n])
    return out


def _restate(z, z_ori, pos, neg, cs, cd, dtype=np.float64, coef=(0.5, 0.5)):
    """The loss stage in numpy at `dtype`: (loss, loss_e, loss_l), w in decoded order, counted mask, dL/dz.  A dot product
    with an endpoint outside its table is 0; the mean of nothing is NaN and gives no gradient."""
    zz, zo = z.numpy().astype(dtype), z_ori.numpy().astype(dtype)
    n, k = zz.shape[0], pos.shape[1]

    def dots(tab, e0, e1):
        ok = (e0 >= 0) & (e0 < tab.shape[0]) & (e1 >= 0) & (e1 < tab.shape[0])
        a, b = np.where(ok, e0, 0), np.where(ok, e1, 0)
        return np.where(ok, (tab[a] * tab[b]).sum(-1), 0).astype(dtype)
    pos, neg, cs, cd = pos.numpy(), neg.numpy(), cs.numpy(), cd.numpy()
    diff_e = dots(zz, pos[0], pos[1]) - dots(zz, neg[0], neg[1])
    counted = cs < cd
    diff_l = np.where(counted, dots(zz, cs, cd) - dots(zo, cs, cd), 0).astype(dtype)
    n_l = int(counted.sum())
    nan = dtype(np.nan)
    loss_e = (diff_e ** 2).sum(dtype=dtype) / dtype(k) if k else nan
    loss_l = (diff_l ** 2).sum(dtype=dtype) / dtype(n_l) if n_l else nan
    w_e = dtype(coef[0]) * 2 * diff_e / dtype(k) if k else diff_e
    w_l = dtype(coef[1]) * 2 * diff_l / dtype(n_l) if n_l else np.zeros_like(diff_l)
    w = np.concatenate([w_e, -w_e, w_l]).astype(dtype)
    e0 = np.concatenate([pos[0], neg[0], np.where(counted, cs, -1)])
    e1 = np.concatenate([pos[1], neg[1], np.where(counted, cd, -1)])
    ok = (e0 >= 0) & (e0 < n) & (e1 >= 0) & (e1 < n)
    dz = np.zeros_like(zz)
    np.add.at(dz, e0[ok], w[ok, None] * zz[e1[ok]])
    np.add.at(dz, e1[ok], w[ok, None] * zz[e0[ok]])
    return (dtype(coef[0]) * loss_e + dtype(coef[1]) * loss_l, loss_e, loss_l), w, counted, dz, (e0, e1)


def _dec_edges(k, seed, n=N):
    """[2, k] pos and neg with repeated endpoints, a pos and a neg edge on the same two nodes, a node many edges share."""
    g = torch.Generator().manual_seed(seed)
    pos, neg = torch.randint(0, n, (2, k), generator=g), torch.randint(0, n, (2, k), generator=g)
    if k > 1:
        neg[:, 1] = pos[:, 0].flip(0)
        pos[0, 1] = pos[0, 0]
    if k > 8:
        pos[0, 2:8] = 7
        neg[1, 3:8] = 7
    return pos, neg


def _cands(n_c, seed, n=N):
    """Candidate edges mixing src < dst, src > dst, self loops, repeated edges (both directions) and repeated endpoints;
    from 5,000 on, node 7 is the source of 100 edges that count (the hub path of gd_edge_dot_bwd_f32)."""
    g = torch.Generator().manual_seed(1000 + seed)
    cs, cd = torch.randint(0, n, (n_c,), generator=g), torch.randint(0, n, (n_c,), generator=g)
    if n_c == 1:
        cs[0], cd[0] = 3, 9
    if n_c >= 65:
        cs[2], cd[2] = 5, 5                                   # self loops
        cs[3], cd[3] = n - 1, n - 1
        cs[4], cd[4] = cd[5].clone(), cs[5].clone()           # an edge and its reverse
        cs[6:9], cd[6:9] = cs[9], cd[9]                       # the same edge four times
        cs[20:30] = 11                                        # repeated endpoints
        cd[30:40] = 250
    if n_c >= 5000:
        cs[100:200] = 7
        cd[100:200] = torch.randint(8, n, (100,), generator=g)
    return cs, cd


def _valid_incidence(e0, e1, n):
    """The stable sort of the valid edges' endpoints: entry p of cat(e0, e1) keeps its position p and its edge p mod M."""
    m = e0.shape[0]
    ok = (e0 >= 0) & (e0 < n) & (e1 >= 0) & (e1 < n)
    p = torch.arange(2 * m)[torch.cat([ok, ok])]
    ends_sorted, order = torch.sort(torch.cat([e0, e1])[p], stable=True)
    p = p[order]
    edge = p % m if m else p
    other = torch.where(p >= m, e0[edge], e1[edge]).to(torch.int32)
    return torch.searchsorted(ends_sorted, torch.arange(n + 1)), other, edge.to(torch.int32)


def _close(got, want):
    """A loss against the restatement: NaN where it is NaN, else within TOL relative."""
    if np.isnan(want):
        return bool(np.isnan(got))
    return abs(got - want) <= TOL * abs(want)


def _tables(d, seed, n_ori=N):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(N, d, generator=g), torch.randn(n_ori, d, generator=g)


def _dz(z, r):
    from gnndelete_amd import _lib
    n, d = z.shape
    dz = torch.full((n, d), float('nan'), device='cuda')
    _lib.check(_L().gd_edge_dot_bwd_f32(z.data_ptr(), z.stride(0), d, r['other'].data_ptr(), r['w_inc'].data_ptr(), None, 0, None,
                                       r['inc_ptr'].data_ptr(), n, dz.data_ptr(), d, _st()), 'gd_edge_dot_bwd_f32')
    return dz


def _check(z, z_ori, pos, neg, cs, cd, tag):
    """One case, every output against the fp64 restatement; z also as a view of a wider NaN-padded buffer (equal bits)."""
    want_losses, want_w, counted, want_dz, (e0, e1) = _restate(z, z_ori, pos, neg, cs, cd)
    k, n_c, d = pos.shape[1], cs.shape[0], z.shape[1]
    wide = torch.full((z.shape[0], 2 * d + 4), float('nan'))
    wide[:, d:2 * d] = z
    dev = [t_.cuda() for t_ in (z_ori, pos, neg, cs, cd)]
    runs = [_call(zz, *dev) for zz in (z.cuda(), z.cuda(), wide.cuda()[:, d:2 * d])]
    r = runs[0]
    for other in runs[1:]:                                   # a second call, and another row pitch: equal bits
        for key in ('losses', 'w', 'dec', 'inc_ptr', 'other', 'src_edge', 'w_inc'):
            assert np.array_equal(r[key].cpu().numpy(), other[key].cpu().numpy(), equal_nan=True), key
    got = r['losses'].cpu().numpy().astype(np.float64)
    w = r['w'].cpu()
    print(f'{tag}: losses {got} want {np.array(want_losses)}  w rel_l2 {rel_l2(w, want_w) if w.numel() else 0.0:.2e}')
    for g_, w_ in zip(got, want_losses):
        assert _close(g_, w_), (tag, got, want_losses)
    assert bool(torch.isfinite(w).all())
    if np.abs(want_w).sum() > 0:
        assert rel_l2(w, want_w) < TOL
    assert torch.equal(w[k:2 * k], -w[:k])
    assert bool((w[2 * k:][~torch.from_numpy(counted)] == 0).all())          # exactly 0 where a candidate does not count
    # the decoded list and the incidence list over it
    assert torch.equal(r['dec'].cpu(), torch.from_numpy(np.stack([e0, e1])))
    want_ptr, want_other, want_src = _valid_incidence(torch.from_numpy(e0), torch.from_numpy(e1), z.shape[0])
    total = r['total']
    assert total == want_other.numel() and torch.equal(r['inc_ptr'].cpu(), want_ptr)
    assert torch.equal(r['other'][:total].cpu(), want_other) and torch.equal(r['src_edge'][:total].cpu(), want_src)
    assert torch.equal(r['w_inc'][:total], r['w'][r['src_edge'][:total].long()])
    assert bool(torch.isnan(r['w_inc'][total:]).all())                        # nothing written past the incidences
    # dL/dz through gd_edge_dot_bwd_f32
    dz = _dz(z.cuda(), r).cpu()
    assert bool(torch.isfinite(dz).all())
    if np.abs(want_dz).sum() > 0:
        print(f'{tag}: dz rel_l2 {rel_l2(dz, want_dz):.2e}')
        assert rel_l2(dz, want_dz) < TOL
    else:
        assert bool((dz == 0).all())
    return r


_CASES = [(d, k, n_c) for d in (4, 32, 64, 260) for k in (0, 1, 63, 64, 65, 1000) for n_c in (0, 1, 65, 5000)]


def _case_inputs(d, k, n_c):
    z, z_ori = _tables(d, SEED + 7 * d + k + n_c)
    pos, neg = _dec_edges(k, SEED + k + d)
    cs, cd = _cands(n_c, SEED + n_c + d)
    return z, z_ori, pos, neg, cs, cd


def test_fp32_restatement_meets_the_bound():
    """The bound is usable on EVERY case's inputs: the same arithmetic in fp32 on the CPU (numpy's summation order, not the
    kernel's) stays within TOL / 4 of fp64.  With one or two terms a difference of two random dot products can be small
    against them by chance - a cancellation that no fp32 evaluation resolves to 1e-5; SEED is one for which that does not
    happen in any case, which this test (and not the kernel) decides."""
    for d, k, n_c in _CASES:
        inputs = _case_inputs(d, k, n_c)
        l64, w64, _, dz64, _ = _restate(*inputs)
        l32, w32, _, dz32, _ = _restate(*inputs, dtype=np.float32)
        for a, b in zip(l32, l64):
            assert np.isnan(b) and np.isnan(a) or abs(float(a) - float(b)) <= TOL / 4 * abs(float(b)), (d, k, n_c, l32, l64)
        if np.abs(w64).sum() > 0:
            assert rel_l2(w32.astype(np.float64), w64) < TOL / 4 and rel_l2(dz32.astype(np.float64), dz64) < TOL / 4, (d, k, n_c)


@pytest.mark.parametrize('d,k,n_c', _CASES)
def test_batch_loss_against_fp64(d, k, n_c):
    z, z_ori, pos, neg, cs, cd = _case_inputs(d, k, n_c)
    r = _check(z, z_ori, pos, neg, cs, cd, f'd={d} k={k} n_c={n_c}')
    if n_c >= 5000:
        deg = r['inc_ptr'][1:] - r['inc_ptr'][:-1]
        assert int(deg[7]) > 64                                               # the hub path of gd_edge_dot_bwd_f32
    if k == 0:
        assert bool(torch.isnan(r['losses'][:2]).all())
    if n_c == 0:
        assert bool(torch.isnan(r['losses'][[0, 2]]).all())


@pytest.mark.parametrize('d', [4, 64, 260])
def test_candidates_of_which_nothing_counts(d):
    """src >= dst everywhere: loss_l (and the total) NaN, every candidate's w exactly 0 and no incidence from them; the DEC
    half is what it is without any candidate, bit for bit."""
    z, z_ori = _tables(d, d)
    pos, neg = _dec_edges(65, d)
    g = torch.Generator().manual_seed(d)
    cd = torch.randint(0, N, (700,), generator=g)
    cs = cd + torch.randint(0, 3, (700,), generator=g)
    cs = cs.clamp(max=N - 1).maximum(cd)
    r = _check(z, z_ori, pos, neg, cs, cd, f'nothing counts d={d}')
    alone = _call(z.cuda(), z_ori.cuda(), pos.cuda(), neg.cuda(), cs[:0].cuda(), cd[:0].cuda())
    assert bool(torch.isnan(r['losses'][0])) and bool(torch.isnan(r['losses'][2]))
    assert torch.equal(r['losses'][1], alone['losses'][1]) and torch.equal(r['w'][:130], alone['w'])
    assert bool((r['w'][130:] == 0).all()) and bool((r['dec'][:, 130:] == -1).all())
    assert r['total'] == alone['total'] and torch.equal(r['w_inc'][:r['total']], alone['w_inc'][:r['total']])


def test_no_df_edge_leaves_the_locality_half_correct():
    """k = 0 with candidates: loss_e NaN, the candidates' gradients those of coef_l * loss_l (checked against fp64 in
    _check) and finite."""
    z, z_ori = _tables(64, 3)
    none = torch.zeros(2, 0, dtype=torch.long)
    cs, cd = _cands(5000, 3)
    r = _check(z, z_ori, none, none, cs, cd, 'k=0')
    assert bool(torch.isnan(r['losses'][1])) and bool(torch.isfinite(r['losses'][2])) and float(r['w'].abs().sum()) > 0


@pytest.mark.parametrize('d', [8, 260])
def test_endpoints_outside_the_tables(d):
    """Ids -1 and n in a negative edge and in candidates (z between NaN rows, z_ori between NaN rows): zero dot products,
    no incidence, nothing outside the tables read.  z_ori with more rows than z: id n is outside z but inside z_ori."""
    n = N
    z, _ = _tables(d, d)
    g = torch.Generator().manual_seed(50 + d)
    pos, neg = _dec_edges(200, d)
    neg[0, 20], neg[1, 22] = -1, n
    neg[:, 27] = torch.tensor([n, -1])
    pos[1, 30] = n
    cs, cd = _cands(300, d)
    cs[50], cd[50] = -1, 4                                                    # counts (src < dst), left of both tables
    cs[51], cd[51] = 9, n                                                     # counts, right of z
    cs[52], cd[52] = n, n + 1                                                 # counts, right of z and (first run) of z_ori

    def between_nan(t_):
        buf = torch.full((t_.shape[0] + 2, t_.shape[1]), float('nan'))
        buf[1:-1] = t_
        return buf.cuda()[1:-1]
    for n_ori in (n, n + 17):
        z_ori = torch.randn(n_ori, d, generator=g)
        want_losses, want_w, counted, want_dz, (e0, e1) = _restate(z, z_ori, pos, neg, cs, cd)
        assert bool(counted[50:53].all())
        r = _call(between_nan(z), between_nan(z_ori), pos.cuda(), neg.cuda(), cs.cuda(), cd.cuda())
        got = r['losses'].cpu().numpy().astype(np.float64)
        print(f'd={d} n_ori={n_ori}: losses {got} want {np.array(want_losses)} w rel_l2 {rel_l2(r["w"].cpu(), want_w):.2e}')
        assert all(_close(a, b) for a, b in zip(got, want_losses)) and rel_l2(r['w'].cpu(), want_w) < TOL
        want_ptr, want_other, want_src = _valid_incidence(torch.from_numpy(e0), torch.from_numpy(e1), n)
        assert r['total'] == want_other.numel() == 2 * (700 - 7 - int((~counted).sum()))
        assert torch.equal(r['inc_ptr'].cpu(), want_ptr) and torch.equal(r['src_edge'][:r['total']].cpu(), want_src)
        dz = _dz(between_nan(z), r).cpu()
        assert bool(torch.isfinite(dz).all()) and rel_l2(dz, want_dz) < TOL


def test_z_ori_rows_beyond_z_change_no_bit():
    z, z_ori = _tables(64, 9)
    pos, neg = _dec_edges(65, 9)
    cs, cd = _cands(5000, 9)
    more = torch.cat([z_ori, torch.full((40, 64), float('nan'))])
    dev = [t_.cuda() for t_ in (pos, neg, cs, cd)]
    a, b = _call(z.cuda(), z_ori.cuda(), *dev), _call(z.cuda(), more.cuda(), *dev)
    for key in ('losses', 'w', 'dec', 'inc_ptr', 'other', 'src_edge'):
        assert torch.equal(a[key], b[key]), key
    assert torch.equal(a['w_inc'][:a['total']], b['w_inc'][:b['total']])


@pytest.mark.parametrize('d,k,n_c', [(4, 0, 140000), (260, 1000, 9000)])
def test_past_one_grid(d, k, n_c):
    """d = 4: 2 x 140,000 incidence slots, more than the finishing launch's 1,024 blocks x 256 threads cover in one trip.
    d = 260: 4 items per block, 10,000 items against the first launch's 2,048 blocks."""
    assert 2 * (2 * k + n_c) > 1024 * 256 or k + n_c > 2048 * 4
    n = 5000
    g = torch.Generator().manual_seed(d)
    z, z_ori = torch.randn(n, d, generator=g), torch.randn(n, d, generator=g)
    pos, neg = torch.randint(0, n, (2, k), generator=g), torch.randint(0, n, (2, k), generator=g)
    cs, cd = torch.randint(0, n, (n_c,), generator=g), torch.randint(0, n, (n_c,), generator=g)
    want_losses, want_w, counted, want_dz, (e0, e1) = _restate(z, z_ori, pos, neg, cs, cd)
    dev = [t_.cuda() for t_ in (z, z_ori, pos, neg, cs, cd)]
    r, r2 = _call(*dev), _call(*dev)
    for key in ('losses', 'w', 'dec', 'inc_ptr', 'other', 'src_edge'):
        assert np.array_equal(r[key].cpu().numpy(), r2[key].cpu().numpy(), equal_nan=True), key
    got = r['losses'].cpu().numpy().astype(np.float64)
    print(f'd={d} k={k} n_c={n_c}: losses {got} want {np.array(want_losses)} w rel_l2 {rel_l2(r["w"].cpu(), want_w):.2e}')
    assert all(_close(a, b) for a, b in zip(got, want_losses)) and rel_l2(r['w'].cpu(), want_w) < TOL
    total = r['total']
    assert total == 2 * (2 * k + int(counted.sum()))
    assert torch.equal(r['dec'].cpu(), torch.from_numpy(np.stack([e0, e1])))
    assert torch.equal(r['w_inc'][:total], r['w'][r['src_edge'][:total].long()])       # a NaN left in place compares unequal
    dz = _dz(dev[0], r).cpu()
    assert rel_l2(dz, want_dz) < TOL


def test_without_incidence_buffers_only_losses_and_w():
    z, z_ori = _tables(32, 1)
    pos, neg = _dec_edges(63, 1)
    cs, cd = _cands(65, 1)
    dev = [t_.cuda() for t_ in (z, z_ori, pos, neg, cs, cd)]
    a, b = _call(*dev), _call(*dev, incidence=False)
    assert torch.equal(a['losses'], b['losses']) and torch.equal(a['w'], b['w']) and torch.equal(a['dec'], b['dec'])


def test_refuses_bad_arguments_without_a_launch():
    L = _L()
    z = torch.randn(8, 8, device='cuda')
    e = torch.zeros(2, 4, dtype=torch.long, device='cuda')
    w = torch.full((12,), 3.0, device='cuda')
    dec = torch.full((2, 12), -5, dtype=torch.int64, device='cuda')
    losses = torch.full((3,), 3.0, device='cuda')
    ws = torch.empty(64, device='cuda')

    def call(zp=z.data_ptr(), zo=z.data_ptr(), ld=8, ldo=8, d=8, k=4, n_c=4, posp=e.data_ptr(), cp=e.data_ptr(), wp=w.data_ptr(),
             ld_dec=12, inc=None):
        return L.gd_edgeprob_batch_loss_f32(zp, ld, 8, zo, ldo, 8, d, posp, 4, e.data_ptr(), 4, k, cp, e.data_ptr(), n_c, 0.5, 0.5,
                                            dec.data_ptr(), ld_dec, wp, losses.data_ptr(), inc, None, None, None, None, 0,
                                            ws.data_ptr(), _st())
    assert call(zp=None) == 1 and b'gd_edgeprob_batch_loss_f32' in L.gd_last_error_string()     # GD_E_NULL
    assert call(zo=None) == 1 and call(wp=None) == 1 and call(posp=None) == 1 and call(cp=None) == 1
    assert call(inc=z.data_ptr()) == 1                                         # inc_ptr without the other four
    assert call(k=-1) == 2 and call(n_c=-1) == 2                               # GD_E_DIM: negative counts
    assert call(d=6, ld=6) == 2 and call(ld=10) == 2 and call(ld=4) == 2 and call(ldo=10) == 2 and call(ldo=4) == 2
    assert call(ld_dec=11) == 2                                                # the decoded list does not fit
    assert call(zp=z.data_ptr() + 4) == 3 and call(zo=z.data_ptr() + 4) == 3   # GD_E_ALIGN
    assert L.gd_edgeprob_batch_loss_workspace(-1, 0, 8) == -1 and L.gd_edgeprob_batch_loss_workspace(4, 4, 6) == -1
    torch.cuda.synchronize()
    assert bool((w == 3.0).all()) and bool((losses == 3.0).all()) and bool((dec == -5).all())    # nothing was launched
    assert call() == 0 and call(k=0, posp=None) == 0 and call(n_c=0, cp=None) == 0               # empty halves are no error
