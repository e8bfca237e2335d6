"""The kernels of the fused edge-probability step (csrc/edgeprob.hip): the DEC term against fp64 numpy, the device-built
incidence list against the arrays ops._EdgeDot.backward builds (and through gd_edge_dot_bwd_f32 against that backward, bit
for bit), and the row add against index_add_."""
import numpy as np
import pytest
import torch

from helpers import rel_l2

pytestmark = pytest.mark.gpu
TOL = 1e-5                                   # tests/test_kernels_gpu.py: the bound of its edge_dot / rowpair_mse values
N = 300


def _L():
    from gnndelete_amd import _lib
    return _lib.lib()


def _st():
    return torch.cuda.current_stream().cuda_stream


def _dec(z, pos, neg, coef=0.5, incidence=None):
    """gd_edgeprob_dec_f32 on device tensors -> (loss [1], w [2m], w_inc or None)."""
    from gnndelete_amd import _lib
    L = _L()
    m, d = pos.shape[1], z.shape[1]
    w = torch.full((2 * m,), float('nan'), device='cuda')
    loss = torch.full((1,), float('nan'), device='cuda')
    ws = torch.empty(max(1, L.gd_edgeprob_dec_workspace(m, d)), device='cuda')
    src_edge = inc_ptr = w_inc = None
    if incidence is not None:
        inc_ptr, src_edge = incidence
        w_inc = torch.full((4 * m,), float('nan'), device='cuda')
    _lib.check(L.gd_edgeprob_dec_f32(z.data_ptr(), z.stride(0), z.shape[0], d, pos.data_ptr(), pos.stride(0), neg.data_ptr(),
                                     neg.stride(0), m, coef, w.data_ptr(), loss.data_ptr(),
                                     None if src_edge is None else src_edge.data_ptr(),
                                     None if inc_ptr is None else inc_ptr.data_ptr(),
                                     None if w_inc is None else w_inc.data_ptr(), ws.data_ptr(), _st()), 'gd_edgeprob_dec_f32')
    return loss, w, w_inc


def _edges(m, seed):
    """[2, m] pos and neg with repeated endpoints and (m > 1) a pos and a neg edge sharing both nodes."""
    g = torch.Generator().manual_seed(seed)
    pos = torch.randint(0, N, (2, m), generator=g)
    neg = torch.randint(0, N, (2, m), generator=g)
    if m > 1:
        neg[:, 1] = pos[:, 0].flip(0)                  # the same two nodes as a positive edge
        pos[0, 1] = pos[0, 0]                          # a repeated endpoint
    if m > 8:
        pos[0, 2:8] = 7                                # a node that many edges share
        neg[1, 3:8] = 7
    return pos, neg


@pytest.mark.parametrize('d', [4, 32, 64])
@pytest.mark.parametrize('m', [1, 63, 64, 65, 1000])
def test_dec_value_and_gradient_against_fp64(m, d):
    g = torch.Generator().manual_seed(100 * m + d)
    z = torch.randn(N, d, generator=g)
    pos, neg = _edges(m, m + d)
    z64, p, q = z.double().numpy(), pos.numpy(), neg.numpy()      # index arrays: a one-element tensor would index as a scalar
    a = (z64[p[0]] * z64[p[1]]).sum(-1)
    b = (z64[q[0]] * z64[q[1]]).sum(-1)
    diff = a - b
    want_loss = (diff ** 2).mean()
    want_w = np.concatenate([0.5 * 2 * diff / m, -0.5 * 2 * diff / m])
    # z as a view of a wider buffer whose pad columns hold NaN; pos / neg as halves of one [2, 2m] buffer
    wide = torch.full((N, 2 * d + 4), float('nan'))
    wide[:, d:2 * d] = z
    zc, zp = z.cuda(), wide.cuda()[:, d:2 * d]
    dec = torch.cat([pos, neg], 1).cuda()
    outs = []
    for zz, pp, nn in ((zc, pos.cuda(), neg.cuda()), (zp, dec[:, :m], dec[:, m:])):
        loss, w, _ = _dec(zz, pp, nn)
        loss2, w2, _ = _dec(zz, pp, nn)
        assert torch.equal(loss, loss2) and torch.equal(w, w2)               # two calls: equal bits
        print(f'm={m} d={d} loss rel {abs(float(loss) - want_loss) / want_loss:.2e}  w rel_l2 {rel_l2(w.cpu(), want_w):.2e}')
        assert abs(float(loss) - want_loss) <= TOL * want_loss
        assert rel_l2(w.cpu(), want_w) < TOL
        assert torch.equal(w[m:], -w[:m])
        outs.append((loss, w))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])    # the pitch changes no bit


def test_dec_refuses_bad_arguments_without_a_launch():
    from gnndelete_amd import _lib
    L = _L()
    z = torch.randn(8, 8, device='cuda')
    e = torch.zeros(2, 4, dtype=torch.long, device='cuda')
    w = torch.full((8,), 3.0, device='cuda')
    loss = torch.full((1,), 3.0, device='cuda')
    ws = torch.empty(16, device='cuda')

    def call(zp=z.data_ptr(), ld=8, d=8, m=4, wp=w.data_ptr(), src=None):
        return L.gd_edgeprob_dec_f32(zp, ld, 8, d, e.data_ptr(), 4, e.data_ptr(), 4, m, 0.5, wp, loss.data_ptr(), src, None, None,
                                     ws.data_ptr(), _st())
    assert call(m=0) == 2 and b'm=0' in L.gd_last_error_string()              # GD_E_DIM: upstream's MSE of nothing is NaN
    assert call(zp=None) == 1 and call(wp=None) == 1                           # GD_E_NULL
    assert call(src=e.data_ptr()) == 1                                         # src_edge without inc_ptr / w_inc
    assert call(d=6, ld=6) == 2 and call(d=8, ld=10) == 2 and call(d=8, ld=4) == 2      # d % 4, pitch % 4, pitch < d
    assert call(zp=z.data_ptr() + 4) == 3                                      # GD_E_ALIGN
    torch.cuda.synchronize()
    assert bool((w == 3.0).all()) and float(loss) == 3.0                       # nothing was launched
    assert call() == 0


def _reference_incidence(e0, e1, n):
    """The arrays of ops._EdgeDot.backward (ops.py: one stable sort of cat(e0, e1), searchsorted over n + 1 keys)."""
    m = e0.shape[0]
    ends = torch.cat([e0, e1])
    ends_sorted, order = torch.sort(ends, stable=True)
    edge = order % m
    other = torch.where(order >= m, e0[edge], e1[edge]).to(torch.int32)
    inc_ptr = torch.searchsorted(ends_sorted, torch.arange(n + 1, device=e0.device))
    return inc_ptr, other, edge.to(torch.int32)


def _incidence_graphs():
    g = torch.Generator().manual_seed(3)
    out = [('n1', 1, torch.zeros(2, 5, dtype=torch.long)),                                     # one node: self pairs only
           ('M2', 65, torch.tensor([[3, 64], [64, 3]])),                                        # M = 2
           ('n65', 65, torch.randint(0, 65, (2, 131), generator=g))]                            # M no multiple of 64
    e = torch.randint(0, 4000, (2, 1777), generator=g)                                         # nodes 4000.. have no incidence
    e[0, 100:300] = 17                                                                         # a hub: > 64 incidences, both sides
    e[1, 250:400] = 17
    e[:, 500:520] = torch.arange(20).repeat(2, 1) + 30                                         # self pairs
    e[:, 600:610] = e[:, 590:600]                                                              # repeated edges
    out.append(('n5000', 5000, e))
    return out


@pytest.mark.parametrize('name,n,e', _incidence_graphs(), ids=[g[0] for g in _incidence_graphs()])
def test_incidence_list_equals_the_stable_sort(name, n, e):
    from gnndelete_amd.edgeprob import edge_incidence
    e = e.cuda()
    want = _reference_incidence(e[0], e[1], n)
    got = edge_incidence(e[0], e[1], n)
    got2 = edge_incidence(e[0], e[1], n)
    for a, b, c, key in zip(got, want, got2, ('inc_ptr', 'other', 'src_edge')):
        assert a.dtype == b.dtype and torch.equal(a, b), key
        assert torch.equal(a, c), key
    if name == 'n5000':
        deg = got[0][1:] - got[0][:-1]
        assert int(deg.max()) > 64 and int((deg == 0).sum()) >= 1000


@pytest.mark.parametrize('d', [16, 64])
def test_incidence_feeds_edge_dot_backward_bit_for_bit(d):
    """gd_edgeprob_dec_f32 (w gathered into incidence order) + gd_edge_incidence + gd_edge_dot_bwd_f32 against autograd
    through ops.edge_dot with the same upstream gradients."""
    from gnndelete_amd import _lib, ops
    from gnndelete_amd.edgeprob import edge_incidence
    m, n = 333, N
    g = torch.Generator().manual_seed(d)
    z = torch.randn(n, d, generator=g).cuda()
    pos, neg = _edges(m, 11)
    pos[0, 20:120] = 5                                   # a hub of the decoded edges
    dec = torch.cat([pos, neg], 1).cuda()
    inc_ptr, other, src_edge = edge_incidence(dec[0], dec[1], n)
    _, w, w_inc = _dec(z, dec[:, :m], dec[:, m:], incidence=(inc_ptr, src_edge))
    assert torch.equal(w_inc, w[src_edge.long()])
    dz = torch.full((n, d), float('nan'), device='cuda')
    _lib.check(_L().gd_edge_dot_bwd_f32(z.data_ptr(), d, d, other.data_ptr(), w_inc.data_ptr(), None, 0, None, inc_ptr.data_ptr(),
                                       n, dz.data_ptr(), d, _st()), 'gd_edge_dot_bwd_f32')
    zg = z.clone().requires_grad_(True)
    ops.edge_dot(zg, dec[0], dec[1]).backward(w)
    assert torch.equal(dz, zg.grad)


@pytest.mark.parametrize('d', [4, 20, 64, 260])
def test_rows_add_is_exact_and_leaves_other_rows_alone(d):
    from gnndelete_amd.edgeprob import rows_add_
    g = torch.Generator().manual_seed(d)
    n, n_s, sentinel = 500, 137, -777.25
    nodes = torch.randperm(n, generator=g)[:n_s].sort().values
    buf = torch.full((n, d + 8), sentinel)
    base = torch.randn(n_s, d, generator=g)
    buf[nodes, 4:4 + d] = base
    src_buf = torch.full((n_s, 2 * d), float('nan'))
    src_buf[:, d:] = torch.randn(n_s, d, generator=g)
    dev_buf, dev_src = buf.cuda(), src_buf.cuda()
    rows_add_(dev_buf[:, 4:4 + d], nodes.to(torch.int32).cuda(), dev_src[:, d:], 0.5)
    want = buf.clone()
    want[:, 4:4 + d] = want[:, 4:4 + d].index_add_(0, nodes, 0.5 * src_buf[:, d:])
    assert torch.equal(dev_buf.cpu(), want)              # listed rows exact, unlisted rows and pad columns keep the sentinel
    rows_add_(dev_buf[:, 4:4 + d], nodes[:0].to(torch.int32).cuda(), dev_src[:, d:], 0.5)
    assert torch.equal(dev_buf.cpu(), want)
