"""gd_del_loss_fold_wgrad_parts_f32 - the weight-stationary Del-2 pass that stores dz where the input gradient went and leaves
W' = W_D2^T W2 for the next chained Del-1 pass - called directly, against gd_del_loss_bwd_wgrad_parts_f32 on the same input.

W_D2 = I + 0.1 randn / 8 is NOT symmetric: with the initial W_D2 = I the two associations (A^T (dz W_D^T)) W2 and
(A^T dz)(W_D^T W2) are bit-identical and a transposed fold would pass.  Row counts: 65,536 (the smallest the form covers) and
65,541 (a last 16-row unit of five live rows); scattered rows of an 80,000-row table; row pitches 64 and 72; a ninth of the rows
without a loss slot.

Bounds: bit equality wherever the fold leaves the arithmetic alone (loss partials, weight-gradient partials, the stored rows
against the parent's dz).  W' against fp64 within twice the error of an fp32 torch product of the same operands (both are
chains of 64 multiply-adds; the factor is room for their order).  The composition through gd_del1_chain_loss_wgrad_f32: z, sign
bits and loss sums bit-equal (they do not read the carried stream), the dW_D1 sums within twice the parent path's error against
an fp64 evaluation of the same input.
"""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

N, D, H = 80000, 64, 128


def _lib():
    from gnndelete_amd import _lib
    return _lib.lib()


def _p(t):
    return None if t is None else t.data_ptr()


def _st():
    return torch.cuda.current_stream().cuda_stream


def _ok(rc, what):
    from gnndelete_amd._lib import check
    check(rc, what)


@functools.lru_cache(maxsize=None)
def _data(n_sel):
    """The input of one row count, built once and never modified."""
    g = torch.Generator(device='cuda').manual_seed(1000 + n_sel)
    dev = 'cuda'

    def randn(*shape):
        return torch.randn(*shape, device=dev, generator=g)
    p = randn(N, D)
    wd = (torch.eye(D, device=dev) + 0.1 * randn(D, D) / 8).contiguous()
    assert float((wd - wd.t()).abs().max()) > 1e-2
    w2 = (randn(D, H) / 8).contiguous()
    idx = torch.sort(torch.randperm(N, device=dev, generator=g)[:n_sel]).values.to(torch.int32)
    n_slots = n_sel - n_sel // 9
    slot = torch.full((n_sel,), -1, dtype=torch.int32, device=dev)
    slot[torch.randperm(n_sel, device=dev, generator=g)[:n_slots]] = torch.randperm(n_slots, device=dev, generator=g).to(torch.int32)
    tm = randn(n_slots, D)
    coef = torch.rand(n_slots, device=dev, generator=g) * 1e-3
    cnt = torch.randint(1, 4, (n_slots,), device=dev, generator=g).float() * torch.where(torch.rand(n_slots, device=dev, generator=g) < 0.3, -1.0, 1.0)
    return dict(p=p, wd=wd, w2=w2, idx=idx, slot=slot, tm=tm, coef=coef, cnt=cnt, s=n_sel)


def _pitched(t, pitch, fill=None):
    """A [rows, pitch] buffer whose first columns hold t (fill = None) or `fill` everywhere; returns the [rows, width] view."""
    rows, width = t.shape
    buf = torch.full((rows, pitch), float('nan') if fill is None else fill, device=t.device)
    if fill is None:
        buf[:, :width] = t
    return buf[:, :width], buf


def _both(n_sel, pitch):
    """(parent, fold) results of the two entries on _data(n_sel) at row pitch `pitch` for p and the gradient buffer."""
    L, Dt = _lib(), _data(n_sel)
    s = Dt['s']
    nb = L.gd_del_loss_bwd_wgrad_parts(s, D)
    assert L.gd_del_loss_fold_wgrad_covers(s, D, H) == 1 and 1 <= nb <= L.gd_rows_gemm_wgrad_blocks(s)
    pv, _ = _pitched(Dt['p'], pitch)
    head = [_p(pv), pv.stride(0), _p(Dt['idx']), s, _p(Dt['wd']), D, _p(Dt['slot']), _p(Dt['tm']), _p(Dt['coef']), _p(Dt['cnt'])]
    out = {}
    # parent: dz (compact) + dp on the listed rows
    dz = torch.full((s, D), float('nan'), device='cuda')
    dp, dp_buf = _pitched(torch.empty(N, D, device='cuda'), pitch, fill=float('nan'))
    lp, ws = torch.full((2 * nb,), 5.0, device='cuda'), torch.full((nb * D * D,), 3.0, device='cuda')
    _ok(L.gd_del_loss_bwd_wgrad_parts_f32(*head, _p(dz), dz.stride(0), _p(dp), dp.stride(0), _p(lp), _p(ws), nb, _st()), 'parent')
    out['parent'] = dict(dz=dz, dp=dp, lp=lp, ws=ws)
    # fold: dz on the listed rows of the full-size buffer + W'
    g, g_buf = _pitched(torch.empty(N, D, device='cuda'), pitch, fill=float('nan'))
    wf = torch.full((D, H), float('nan'), device='cuda')
    lp_f, ws_f = torch.full((2 * nb,), 5.0, device='cuda'), torch.full((nb * D * D,), 3.0, device='cuda')
    _ok(L.gd_del_loss_fold_wgrad_parts_f32(*head, _p(g), g.stride(0), _p(Dt['w2']), H, _p(wf), _p(lp_f), _p(ws_f), nb, _st()), 'fold')
    wf2 = torch.full((D, H), float('nan'), device='cuda')
    _ok(L.gd_del_loss_fold_wgrad_parts_f32(*head, _p(g), g.stride(0), _p(Dt['w2']), H, _p(wf2), _p(lp_f), _p(ws_f), nb, _st()), 'fold again')
    out['fold'] = dict(g=g, g_buf=g_buf, wf=wf, wf2=wf2, lp=lp_f, ws=ws_f)
    torch.cuda.synchronize()
    return out, nb


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def test_coverage_query_and_refusal():
    L = _lib()
    assert L.gd_del_loss_fold_wgrad_covers(65536, 64, 128) == 1
    for n_sel, d, h in ((65535, 64, 128), (65536, 32, 128), (65536, 64, 64), (65536, 128, 128), (0, 64, 128)):
        assert L.gd_del_loss_fold_wgrad_covers(n_sel, d, h) == 0, (n_sel, d, h)
    t = torch.zeros(1000, 64, device='cuda')
    i32 = torch.zeros(1000, dtype=torch.int32, device='cuda')
    w2, wf = torch.zeros(64, 128, device='cuda'), torch.zeros(64, 128, device='cuda')
    rc = L.gd_del_loss_fold_wgrad_parts_f32(_p(t), 64, _p(i32), 1000, _p(t), 64, _p(i32), _p(t), _p(t), _p(t), _p(t.clone()), 64, _p(w2), 128,
                                            _p(wf), _p(t), _p(t), 1, _st())
    assert rc != 0 and b'not covered' in L.gd_last_error_string()


@pytest.mark.parametrize('pitch', [64, 72])
@pytest.mark.parametrize('n_sel', [65536, 65541])
def test_fold_pass_against_the_parent_pass(n_sel, pitch):
    Dt = _data(n_sel)
    out, nb = _both(n_sel, pitch)
    par, fold = out['parent'], out['fold']
    li = Dt['idx'].long()
    # the loss partials and the weight-gradient partials: the same bits
    assert torch.equal(fold['lp'], par['lp'])
    assert torch.equal(fold['ws'], par['ws'])
    assert not bool(torch.isnan(par['dz']).any()) and float(par['dz'].abs().max()) > 0
    assert int((Dt['slot'] < 0).sum()) > 1000 and float(par['dz'][Dt['slot'] < 0].abs().max()) == 0.0        # rows without a loss term
    # the stored rows are the parent's dz, row for row
    assert torch.equal(fold['g'][li], par['dz'])
    # rows outside the list, and the padding columns of every row, are untouched
    canary = torch.isnan(fold['g_buf'])
    listed = torch.zeros(N, dtype=torch.bool, device='cuda')
    listed[li] = True
    assert bool(canary[~listed].all()) and bool(canary[:, D:].all()) and not bool(canary[listed][:, :D].any())
    # W' = W_D^T W2
    want = Dt['wd'].double().t() @ Dt['w2'].double()
    err_torch = _rel(Dt['wd'].cpu().t().contiguous() @ Dt['w2'].cpu(), want.cpu())
    err = _rel(fold['wf'], want)
    transposed = _rel(Dt['wd'].double() @ Dt['w2'].double(), want)
    print(f'[fold n_sel={n_sel} pitch={pitch}] MEASURED W\' rel-L2 to fp64 {err:.2e} (fp32 torch product {err_torch:.2e}; W_D W2 instead of '
          f'W_D^T W2 would be {transposed:.2e})')
    assert err <= 2.0 * err_torch, (err, err_torch)
    assert transposed > 1e3 * err_torch
    assert torch.equal(fold['wf'], fold['wf2'])                           # two launches, the same bits


@functools.lru_cache(maxsize=None)
def _graph(seed, per_row=8):
    """A^T as (target row, source row, weight): per_row entries for every row of the table.  The weights are 16 times those of a
    normalised adjacency: the layer-1 loss term p^T (z - tbar) has a coherent diagonal (z ~ p), and with unit-scale weights the
    carried stream is 0.02 of dW_D1 - too little for a bound on dW_D1 to say anything about it."""
    g = torch.Generator(device='cuda').manual_seed(seed)
    dst = torch.arange(N, device='cuda').repeat_interleave(per_row)
    src = torch.randint(0, N, (N * per_row,), device='cuda', generator=g)
    val = 16.0 * torch.rand(N * per_row, device='cuda', generator=g) / per_row ** 0.5
    return dst, src, val


def _aggregate(rows, dtype):
    dst, src, val = _graph(7)
    out = torch.zeros(N, rows.shape[1], dtype=dtype, device='cuda')
    return out.index_add_(0, dst, rows.to(dtype)[src] * val.to(dtype)[:, None])


def test_fold_composes_with_the_chained_del1_pass():
    """A^T (stored rows) with W' against A^T dp2 with W2 through gd_del1_chain_loss_wgrad_f32."""
    L = _lib()
    n_sel, pitch, s1 = 65541, 72, 66000
    Dt = _data(n_sel)
    out, _ = _both(n_sel, pitch)
    li2 = Dt['idx'].long()
    g_fold = torch.zeros(N, D, device='cuda')
    g_fold[li2] = out['fold']['g'][li2]
    dp_par = torch.zeros(N, D, device='cuda')
    dp_par[li2] = out['parent']['dp'][li2]
    dt_fold, dt_par = _aggregate(g_fold, torch.float32), _aggregate(dp_par, torch.float32)
    # layer-1 side
    gen = torch.Generator(device='cuda').manual_seed(5)
    p1 = torch.randn(N, H, device='cuda', generator=gen)
    w1 = (torch.eye(H, device='cuda') + 0.05 * torch.randn(H, H, device='cuda', generator=gen)).contiguous()
    idx1 = torch.sort(torch.randperm(N, device='cuda', generator=gen)[:s1]).values.to(torch.int32)
    n_slots = s1 - s1 // 9
    slot = torch.full((s1,), -1, dtype=torch.int32, device='cuda')
    slot[torch.randperm(s1, device='cuda', generator=gen)[:n_slots]] = torch.randperm(n_slots, device='cuda', generator=gen).to(torch.int32)
    tm = torch.randn(n_slots, H, device='cuda', generator=gen)
    coef = torch.rand(n_slots, device='cuda', generator=gen) * 1e-3
    cnt = torch.randint(1, 4, (n_slots,), device='cuda', generator=gen).float() * torch.where(torch.rand(n_slots, device='cuda', generator=gen) < 0.3, -1.0, 1.0)
    prev = torch.randint(-2 ** 31, 2 ** 31 - 1, (s1, 4), device='cuda', dtype=torch.int64, generator=gen).to(torch.int32)
    nb = L.gd_del1_loss_wgrad_parts(s1)
    ws_n = max(1, L.gd_rows_gemm_wgrad_workspace(s1, H, H))

    def chain(dt, w_next):
        z, bits = torch.zeros(N, H, device='cuda'), prev.clone()
        lp, ws = torch.zeros(2 * nb, device='cuda'), torch.zeros(ws_n, device='cuda')
        _ok(L.gd_del1_chain_loss_wgrad_f32(_p(p1), p1.stride(0), _p(idx1), s1, _p(w1), H, _p(z), z.stride(0), _p(bits), _p(slot), _p(tm),
                                           _p(coef), _p(cnt), _p(dt), dt.stride(0), D, _p(w_next), None, None, None, None, _p(lp), _p(ws), nb,
                                           _st()), 'chain')
        return z, bits, lp, ws[:nb * H * H].view(nb, H, H).double().sum(0)
    z_f, bits_f, lp_f, dw_f = chain(dt_fold, out['fold']['wf'])
    z_p, bits_p, lp_p, dw_p = chain(dt_par, Dt['w2'])
    assert torch.equal(z_f, z_p) and torch.equal(bits_f, bits_p) and torch.equal(lp_f, lp_p)
    # fp64 evaluation of the same input
    wd64, w264 = Dt['wd'].double(), Dt['w2'].double()
    z2 = Dt['p'].double()[li2] @ wd64
    has = Dt['slot'] >= 0
    u = Dt['slot'].clamp(min=0).long()
    dz64 = torch.where(has[:, None], Dt['coef'].double()[u][:, None] * (z2 - Dt['tm'].double()[u]), torch.zeros_like(z2))
    dp64 = torch.zeros(N, D, dtype=torch.float64, device='cuda')
    dp64[li2] = dz64 @ wd64.t()
    li1 = idx1.long()
    dh64 = _aggregate(dp64, torch.float64)[li1] @ w264
    gate = ((prev.long()[:, :, None] >> torch.arange(32, device='cuda')) & 1).reshape(s1, H).bool()
    z1 = p1.double()[li1] @ w1.double()
    has1 = slot >= 0
    u1 = slot.clamp(min=0).long()
    g64 = torch.where(has1[:, None], coef.double()[u1][:, None] * (z1 - tm.double()[u1]), torch.zeros_like(z1)) + torch.where(gate, dh64, torch.zeros_like(dh64))
    dw64 = p1.double()[li1].t() @ g64
    stream = p1.double()[li1].t() @ torch.where(gate, dh64, torch.zeros_like(dh64))
    err_f, err_p = _rel(dw_f, dw64), _rel(dw_p, dw64)
    print(f'[fold composition] MEASURED dW_D1 rel-L2 to fp64: folded {err_f:.3e}, parent {err_p:.3e}; the two {_rel(dw_f, dw_p):.3e} apart; '
          f'the carried stream is {float(stream.norm() / dw64.norm()):.2f} of dW_D1')
    assert float(stream.norm() / dw64.norm()) > 0.1, 'the carried stream must matter in the sums the bound is about'
    assert err_f <= 2.0 * err_p, f'dW_D1 rel-L2 to fp64: folded {err_f:.3e}, parent {err_p:.3e}'
