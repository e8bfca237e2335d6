"""The two kernels of the fused backbone step (csrc/linkpred.hip) against fp64 torch, with the kernel suite's bound (TOL of
tests/test_edgeprob_kernels_gpu.py).

gd_edge_bce_f32: F.binary_cross_entropy_with_logits over [pos | neg] and its autograd gradient in fp64 - every lane-group
width, one-sided lists, pitched z and edge buffers, logits at 0, about +-30 and beyond +-100, the gather into incidence order
(a hub included), endpoints outside [0, n), past the 2,048-block grid, equal bits on two calls, and the refusals.
gd_col_sum_f32: plain, gated (exact zeros closed), row-weighted and both, the gated matrix written in place, pitched rows,
more than one block, equal bits, and the refusals.

Measured on an MI355X (largest rel. distance to fp64 over the cases; the bound is TOL = 1e-5):
  BCE, every case of this file        loss 4.5e-7   w rel-L2 4.5e-7   dL/dz through gd_edge_dot_bwd_f32 7.3e-8
  column sums, every case             rel-L2 3.5e-7   largest error / column's sum of magnitudes 1.2e-7
Everything else in this file is an equality of bits."""
import pytest
import torch
import torch.nn.functional as F

from helpers import rel_l2

pytestmark = pytest.mark.gpu
TOL = 1e-5                                   # tests/test_edgeprob_kernels_gpu.py: TOL
N = 300


def _L():
    from gnndelete_amd import _lib
    return _lib.lib()


def _st():
    return torch.cuda.current_stream().cuda_stream


def _edges(n_pos, n_neg, seed, n=N):
    g = torch.Generator().manual_seed(seed)
    pos, neg = torch.randint(0, n, (2, n_pos), generator=g), torch.randint(0, n, (2, n_neg), generator=g)
    if n_pos > 8:
        pos[0, 2:8] = 7                                # a node that many edges share
    if n_neg > 8:
        neg[1, 3:8] = 7
        neg[:, 1] = neg[:, 0]                          # a repeated negative
    return pos, neg


def _bce_fp64(z, pos, neg, coef=1.0):
    """(loss, w [M]) of F.binary_cross_entropy_with_logits and its autograd gradient in fp64; an edge with an endpoint outside
    [0, n) has the logit 0 (the header's rule)."""
    n = z.shape[0]
    e = torch.cat([pos, neg], 1)
    ok = ((e >= 0) & (e < n)).all(0)
    c = torch.where(ok, e, torch.zeros_like(e))
    logits = (torch.where(ok, (z.double()[c[0]] * z.double()[c[1]]).sum(-1), torch.zeros(e.shape[1], dtype=torch.float64))
              .requires_grad_(True))
    label = torch.cat([torch.ones(pos.shape[1]), torch.zeros(neg.shape[1])]).double()
    loss = F.binary_cross_entropy_with_logits(logits, label)
    (coef * loss).backward()
    return float(loss), logits.grad, logits.detach()


def _check(tag, loss, w, want_loss, want_w):
    assert bool(torch.isfinite(loss).all()) and bool(torch.isfinite(w).all())
    d_loss, d_w = abs(float(loss) - want_loss) / want_loss, rel_l2(w.cpu(), want_w)
    print(f'{tag} loss rel {d_loss:.2e}  w rel_l2 {d_w:.2e}')
    assert d_loss <= TOL and d_w < TOL


@pytest.mark.parametrize('d', [4, 16, 64, 128, 260])
@pytest.mark.parametrize('n_pos,n_neg', [(1, 0), (0, 1), (63, 65), (64, 64), (257, 300)])
def test_bce_value_and_gradient_against_fp64(n_pos, n_neg, d):
    from gnndelete_amd.backbone import edge_bce
    g = torch.Generator().manual_seed(100 * n_pos + n_neg + d)
    z = torch.randn(N, d, generator=g) * (2.0 / d ** 0.25)
    pos, neg = _edges(n_pos, n_neg, n_pos + d)
    want_loss, want_w, _ = _bce_fp64(z, pos, neg)
    # z as a view of a wider buffer whose pad columns hold NaN; pos / neg as the halves of one [2, M + 5] buffer
    wide = torch.full((N, 2 * d + 4), float('nan'))
    wide[:, d:2 * d] = z
    zc, zp = z.cuda(), wide.cuda()[:, d:2 * d]
    dec = torch.full((2, n_pos + n_neg + 5), -12345, dtype=torch.long)
    dec[:, :n_pos], dec[:, n_pos:n_pos + n_neg] = pos, neg
    dec = dec.cuda()
    outs = []
    for zz, pp, nn in ((zc, pos.cuda() if n_pos else None, neg.cuda() if n_neg else None),
                       (zp, dec[:, :n_pos], dec[:, n_pos:n_pos + n_neg])):
        loss, w, _ = edge_bce(zz, pp, nn)
        loss2, w2, _ = edge_bce(zz, pp, nn)
        assert torch.equal(loss, loss2) and torch.equal(w, w2)               # two calls: equal bits
        _check(f'n_pos={n_pos} n_neg={n_neg} d={d}', loss, w, want_loss, want_w)
        outs.append((loss, w))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])    # the pitches change no bit


@pytest.mark.parametrize('scale', [0.0, 1.0, 5.5, 12.0, 40.0])
def test_bce_is_stable_at_large_logits(scale):
    """Rows of +-scale / sqrt(d) * ones give logits of exactly 0 and about +-scale^2: 0, 1, 30, 144 and 1,600, of both signs
    in both halves.  The loss and every w stay finite and equal the fp64 values (a positive edge at l = 144 has the
    gradient -exp(-144) / M, which 1 / (1 + e) - 1 would round to 0)."""
    from gnndelete_amd.backbone import edge_bce
    d, n = 16, 40
    g = torch.Generator().manual_seed(int(scale * 10))
    sign = torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0)
    z = sign[:, None] * (scale / d ** 0.5) * (1 + 0.02 * torch.rand(n, d, generator=g))
    z[:3] = 0                                                                  # logits of exactly 0
    pos, neg = torch.randint(0, n, (2, 70), generator=g), torch.randint(0, n, (2, 50), generator=g)
    want_loss, want_w, logits = _bce_fp64(z, pos, neg)
    if scale >= 5.5:
        assert float(logits.max()) > 0.9 * scale ** 2 and float(logits.min()) < -0.9 * scale ** 2
    loss, w, _ = edge_bce(z.cuda(), pos.cuda(), neg.cuda())
    _check(f'scale={scale}', loss, w, want_loss, want_w)
    # every entry on its own, the tiny ones included.  Autograd's fp64 gradient is sigmoid(l) - 1 for a positive edge, which
    # at l = 30 has lost 2^-53 / exp(-30) = 1e-3 of its value to the subtraction: the entries are held against the same
    # gradient written without it, -sigmoid(-l) / M for a positive edge, in fp64 (equal to autograd's wherever that is exact)
    n_pos, M = pos.shape[1], pos.shape[1] + neg.shape[1]
    exact = torch.cat([-torch.sigmoid(-logits[:n_pos]), torch.sigmoid(logits[n_pos:])]) / M
    assert rel_l2(exact, want_w) < 1e-12
    want_w = exact
    big = want_w.abs() > 1e-30
    # (the relative error of exp(-|l|) is the absolute error of l: d fused multiply-adds at |l| <= 1.1 scale^2, 2^-24 each)
    assert float(((w.cpu().double() - want_w)[big] / want_w[big]).abs().max()) < 4 * d * 2.0 ** -24 * max(1.0, 1.1 * scale ** 2)
    assert float(w.cpu().double()[~big].abs().max() if bool((~big).any()) else 0.0) < 1e-30


@pytest.mark.parametrize('d', [16, 64])
def test_bce_gathers_w_into_incidence_order(d):
    """w_inc == w[src_edge] exactly against gd_edge_incidence's list, with a node of more than 64 incidences; through
    gd_edge_dot_bwd_f32 the result is autograd's through ops.edge_dot with the same upstream gradients, bit for bit."""
    from gnndelete_amd import _lib, ops
    from gnndelete_amd.backbone import edge_bce
    from gnndelete_amd.edgeprob import edge_incidence
    n_pos, n_neg, n = 333, 280, N
    g = torch.Generator().manual_seed(d)
    z = (torch.randn(n, d, generator=g) * 0.5).cuda()
    pos, neg = _edges(n_pos, n_neg, 11)
    pos[0, 20:120] = 5                                   # a hub of the decoded edges
    dec = torch.cat([pos, neg], 1).cuda()
    inc_ptr, other, src_edge = edge_incidence(dec[0], dec[1], n)
    assert int((inc_ptr[1:] - inc_ptr[:-1]).max()) > 64
    loss, w, w_inc = edge_bce(z, dec[:, :n_pos], dec[:, n_pos:], incidence=(inc_ptr, src_edge))
    loss0, w0, none = edge_bce(z, dec[:, :n_pos], dec[:, n_pos:])
    assert none is None and torch.equal(loss, loss0) and torch.equal(w, w0)
    assert w_inc.shape == (2 * (n_pos + n_neg),) and torch.equal(w_inc, w[src_edge.long()])
    dz = torch.full((n, d), float('nan'), device='cuda')
    _lib.check(_L().gd_edge_dot_bwd_f32(z.data_ptr(), d, d, other.data_ptr(), w_inc.data_ptr(), None, 0, None, inc_ptr.data_ptr(),
                                       n, dz.data_ptr(), d, _st()), 'gd_edge_dot_bwd_f32')
    zg = z.clone().requires_grad_(True)
    ops.edge_dot(zg, dec[0], dec[1]).backward(w)
    assert torch.equal(dz, zg.grad)
    # and that is the gradient of the loss in fp64
    z64 = z.double().cpu().requires_grad_(True)
    e = dec.cpu()
    label = torch.cat([torch.ones(n_pos), torch.zeros(n_neg)]).double()
    F.binary_cross_entropy_with_logits((z64[e[0]] * z64[e[1]]).sum(-1), label).backward()
    print(f'd={d} dL/dz rel_l2 {rel_l2(dz.cpu(), z64.grad):.2e}')
    assert rel_l2(dz.cpu(), z64.grad) < TOL


@pytest.mark.parametrize('d', [8, 260])
def test_bce_out_of_range_endpoint_is_a_zero_logit(d):
    """Ids -1 and n only, z between NaN rows: the edge reads nothing, adds log 2 to the sum and gets coef (0.5 - y) / M."""
    from gnndelete_amd.backbone import edge_bce
    from gnndelete_amd.edgeprob import edge_incidence
    n, n_pos, n_neg = N, 150, 140
    g = torch.Generator().manual_seed(d)
    z = torch.randn(n, d, generator=g) * (2.0 / d ** 0.25)
    pos, neg = _edges(n_pos, n_neg, 3 * d)
    pos[0, 20], pos[1, 22], neg[1, 24], neg[0, 25] = -1, n, n, -1
    pos[:, 27], neg[:, 28] = torch.tensor([-1, n]), torch.tensor([n, -1])
    buf = torch.full((n + 2, d), float('nan'))
    buf[1:-1] = z
    zdev = buf.cuda()[1:-1]
    want_loss, want_w, _ = _bce_fp64(z, pos, neg, coef=0.5)
    dec = torch.cat([pos, neg], 1).cuda()
    inc_ptr, other, src_edge = edge_incidence(dec[0], dec[1], n)
    total = int(inc_ptr[n])
    assert total == 2 * (n_pos + n_neg - 6)
    loss, w, w_inc = edge_bce(zdev, dec[:, :n_pos], dec[:, n_pos:], coef=0.5, incidence=(inc_ptr, src_edge))
    _check(f'd={d} out of range', loss, w, want_loss, want_w)
    M = n_pos + n_neg
    quarter = float(torch.tensor(0.5) / torch.tensor(float(M)) * 0.5)                 # fp32: (coef / M) * sigmoid(0)
    assert float(w[20]) == float(w[27]) == -quarter and float(w[n_pos + 24]) == float(w[n_pos + 28]) == quarter
    assert torch.equal(w_inc[:total], w[src_edge[:total].long()])


def test_bce_past_one_grid():
    """d = 4: 256 edges per block, 2,048 blocks at most - M = 600,000 makes every block take a second trip (and some a
    third), and the finishing launch gathers 1.2 M incidences with its 1,024 blocks."""
    from gnndelete_amd.backbone import edge_bce
    from gnndelete_amd.edgeprob import edge_incidence
    n, d, n_pos, n_neg = 5000, 4, 310000, 290000
    assert n_pos + n_neg > 2048 * 256 and 2 * (n_pos + n_neg) > 1024 * 256
    g = torch.Generator().manual_seed(70)
    z = torch.randn(n, d, generator=g)
    pos, neg = torch.randint(0, n, (2, n_pos), generator=g), torch.randint(0, n, (2, n_neg), generator=g)
    want_loss, want_w, _ = _bce_fp64(z, pos, neg)
    dec = torch.cat([pos, neg], 1).cuda()
    inc_ptr, _, src_edge = edge_incidence(dec[0], dec[1], n)
    zdev = z.cuda()
    loss, w, w_inc = edge_bce(zdev, dec[:, :n_pos], dec[:, n_pos:], incidence=(inc_ptr, src_edge))
    loss2, w2, w_inc2 = edge_bce(zdev, dec[:, :n_pos], dec[:, n_pos:], incidence=(inc_ptr, src_edge))
    assert torch.equal(loss, loss2) and torch.equal(w, w2) and torch.equal(w_inc, w_inc2)
    _check('M=600000 d=4', loss, w, want_loss, want_w)
    assert torch.equal(w_inc, w[src_edge.long()])


def test_bce_refuses_bad_arguments_without_a_launch():
    L = _L()
    z = torch.randn(8, 8, device='cuda')
    e = torch.zeros(2, 4, dtype=torch.long, device='cuda')
    w = torch.full((8,), 3.0, device='cuda')
    loss = torch.full((1,), 3.0, device='cuda')
    ws = torch.empty(16, device='cuda')
    assert L.gd_edge_bce_workspace(8, 8) >= 1 and L.gd_edge_bce_workspace(0, 8) == 1

    def call(zp=z.data_ptr(), ld=8, d=8, n_pos=4, n_neg=4, wp=w.data_ptr(), src=None, pos=e.data_ptr()):
        return L.gd_edge_bce_f32(zp, ld, 8, d, pos, 4, n_pos, e.data_ptr(), 4, n_neg, 1.0, wp, loss.data_ptr(), src, None, None,
                                 ws.data_ptr(), _st())
    assert call(n_pos=0, n_neg=0) == 2 and b'gd_edge_bce_f32' in L.gd_last_error_string()       # GD_E_DIM: M == 0
    assert call(n_pos=-1) == 2 and call(n_pos=5) == 2                                            # a count below 0, above its pitch
    assert call(zp=None) == 1 and call(wp=None) == 1 and call(pos=None) == 1                     # GD_E_NULL
    assert call(src=e.data_ptr()) == 1                                                           # src_edge without inc_ptr / w_inc
    assert call(d=6, ld=6) == 2 and call(d=8, ld=10) == 2 and call(d=8, ld=4) == 2               # d % 4, pitch % 4, pitch < d
    assert call(zp=z.data_ptr() + 4) == 3 and b'gd_edge_bce_f32' in L.gd_last_error_string()     # GD_E_ALIGN
    torch.cuda.synchronize()
    assert bool((w == 3.0).all()) and float(loss) == 3.0                                         # nothing was launched
    assert call() == 0 and call(n_pos=0, pos=None) == 0 and call(n_neg=0) == 0                   # one-sided lists are legal
    torch.cuda.synchronize()
    assert bool(torch.isfinite(loss).all())


# ------------------------------------------------------------------------------------------ gd_col_sum_f32
def _col_sum_case(n_rows, d, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n_rows, d, generator=g)
    gate = torch.randn(n_rows, d, generator=g)
    gate[torch.rand(n_rows, d, generator=g) < 0.2] = 0.0            # exact zeros: closed
    gate[0, 0] = -0.0
    row_w = torch.randn(n_rows, generator=g)
    return x, gate, row_w


def _pitched(t, pad_value=float('nan')):
    """t as a view of a wider device buffer (4 spare columns on each side, filled with pad_value)."""
    wide = torch.full((t.shape[0], t.shape[1] + 8), pad_value)
    wide[:, 4:-4] = t
    return wide.cuda()[:, 4:-4]


@pytest.mark.parametrize('d', [4, 16, 64, 128, 260])
@pytest.mark.parametrize('n_rows', [1, 63, 64, 65, 4097])
def test_col_sum_against_fp64(n_rows, d):
    from gnndelete_amd.backbone import col_sum
    x, gate, row_w = _col_sum_case(n_rows, d, 10 * n_rows + d)
    x64, open64, w64 = x.double(), (gate > 0).double(), row_w.double()
    want = {'plain': x64.sum(0), 'gated': (x64 * open64).sum(0), 'weighted': (w64[:, None] * x64).sum(0),
            'both': (w64[:, None] * x64 * open64).sum(0)}
    scale = {'plain': x64.abs().sum(0), 'gated': (x64 * open64).abs().sum(0), 'weighted': (w64[:, None] * x64).abs().sum(0),
             'both': (w64[:, None] * x64 * open64).abs().sum(0)}
    xc, gc, wc = x.cuda(), gate.cuda(), row_w.cuda()
    xp, gp = _pitched(x), _pitched(gate)
    for key, kw, kwp in (('plain', {}, {}), ('gated', dict(gate=gc), dict(gate=gp)), ('weighted', dict(row_w=wc), dict(row_w=wc)),
                         ('both', dict(row_w=wc, gate=gc), dict(row_w=wc, gate=gp))):
        out = col_sum(xc, **kw)
        assert torch.equal(out, col_sum(xc, **kw))                                  # two calls: equal bits
        assert torch.equal(out, col_sum(xp, **kwp))                                 # the pitch changes no bit
        # also per column against its sum of magnitudes (what fp32 summation is relative to; a column sum cancels)
        err = float(((out.cpu().double() - want[key]).abs() / scale[key].clamp_min(1e-30)).max())
        print(f'n_rows={n_rows} d={d} {key}: rel_l2 {rel_l2(out.cpu(), want[key]):.2e}   largest error / sum of magnitudes {err:.2e}')
        assert rel_l2(out.cpu(), want[key]) < TOL and err < TOL


@pytest.mark.parametrize('n_rows,d', [(65, 16), (4097, 64), (700, 260)])
def test_col_sum_writes_the_gated_matrix_in_place(n_rows, d):
    from gnndelete_amd.backbone import col_sum
    x, gate, _ = _col_sum_case(n_rows, d, n_rows + d)
    want = torch.where(gate > 0, x, torch.zeros_like(x))
    sentinel = -777.25
    xp, gp = _pitched(x, sentinel), _pitched(gate, sentinel)
    ref = col_sum(x.cuda(), gate=gate.cuda())
    out = col_sum(xp, gate=gp, gated=xp)
    assert torch.equal(out, ref)
    assert torch.equal(xp.cpu(), want)                                               # exact, zeros where the gate is closed
    whole = xp._base if xp._base is not None else xp
    assert bool((whole[:, :4] == sentinel).all()) and bool((whole[:, -4:] == sentinel).all())    # the pad columns untouched
    # into another matrix: x itself stays
    x2, dst = x.cuda(), torch.full((n_rows, d), sentinel, device='cuda')
    assert torch.equal(col_sum(x2, gate=gate.cuda(), gated=dst), ref)
    assert torch.equal(dst.cpu(), want) and torch.equal(x2.cpu(), x)


def test_col_sum_of_no_rows_is_zero():
    from gnndelete_amd.backbone import col_sum
    out = torch.full((8,), 3.0, device='cuda')
    col_sum(torch.empty(0, 8, device='cuda'), out=out)
    assert bool((out == 0).all())


def test_col_sum_refuses_bad_arguments_without_a_launch():
    L = _L()
    x = torch.ones(8, 8, device='cuda')
    out = torch.full((8,), 3.0, device='cuda')
    ws = torch.empty(64, device='cuda')
    assert L.gd_col_sum_workspace(8, 8) >= 8 and L.gd_col_sum_workspace(8, 6) == 1

    def call(xp=x.data_ptr(), ld=8, d=8, n_rows=8, gate=None, gated=None, outp=out.data_ptr(), wsp=ws.data_ptr()):
        return L.gd_col_sum_f32(xp, ld, n_rows, d, None, gate, gated, outp, wsp, _st())
    assert call(d=6, ld=6) == 2 and b'gd_col_sum_f32' in L.gd_last_error_string()                # GD_E_DIM: d % 4
    assert call(d=1028, ld=1028) == 2 and call(ld=4) == 2 and call(ld=10) == 2 and call(n_rows=-1) == 2
    assert call(xp=None) == 1 and call(outp=None) == 1 and call(wsp=None) == 1                   # GD_E_NULL
    assert call(gated=x.data_ptr()) == 1                                                         # gated without a gate
    assert call(xp=x.data_ptr() + 4) == 3 and call(gate=x.data_ptr() + 4) == 3                   # GD_E_ALIGN
    assert b'gd_col_sum_f32' in L.gd_last_error_string()
    torch.cuda.synchronize()
    assert bool((out == 3.0).all())                                                              # nothing was launched
    assert call() == 0
    assert bool((out == 8.0).all())
