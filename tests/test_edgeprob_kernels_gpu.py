"""The kernels of the fused edge-probability step (csrc/edgeprob.hip): the DEC term against fp64 numpy, the device-built
incidence list against the arrays ops._EdgeDot.backward builds (and through gd_edge_dot_bwd_f32 against that backward, bit
for bit), and the row add against index_add_.

Every lane-group width of the decoder (d = 4 ... 1024: 1 ... 64 lanes per row, up to four trips of the strided loop and a
ragged last trip), endpoints outside [0, n) (ids -1 and n only, with NaN / sentinel rows on both sides of every buffer a
broken guard would touch), the finish kernel past one grid (m = 70,000), the scan's chunk edges, no edge at all, reuse of
one workspace for another edge list, the history ring's wrap, and the refusals of every entry.

Measured on an MI355X (largest rel. distance to fp64 over the cases; the bound is TOL = 1e-5):
  decoder, d = 4 ... 1024, m = 1 ... 1000     loss 5.2e-7   w rel-L2 2.6e-7
  decoder with out-of-range endpoints          loss 1.7e-7   w rel-L2 8.2e-8
  decoder at m = 70,000, d = 8                 loss 3.8e-8   w rel-L2 6.2e-8
Everything else in this file is an equality of bits or of integers."""
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


def _edges(m, seed, n=N):
    """[2, m] pos and neg with repeated endpoints and (m > 1) a pos and a neg edge sharing both nodes."""
    g = torch.Generator().manual_seed(seed)
    pos = torch.randint(0, n, (2, m), generator=g)
    neg = torch.randint(0, n, (2, m), generator=g)
    if m > 1:
        neg[:, 1] = pos[:, 0].flip(0)                  # the same two nodes as a positive edge
        pos[0, 1] = pos[0, 0]                          # a repeated endpoint
    if m > 8:
        pos[0, 2:8] = 7                                # a node that many edges share
        neg[1, 3:8] = 7
    return pos, neg


def _dec_fp64(z, pos, neg):
    """(loss, w [2m]) of the DEC term in fp64 numpy; an edge with an endpoint outside [0, n) has the dot product 0."""
    z64, n, m = z.double().numpy(), z.shape[0], pos.shape[1]

    def dots(e):
        e = e.numpy()                                  # index arrays: a one-element tensor would index as a scalar
        ok = ((e >= 0) & (e < n)).all(0)
        c = np.where(ok, e, 0)
        return np.where(ok, (z64[c[0]] * z64[c[1]]).sum(-1), 0.0)
    diff = dots(pos) - dots(neg)
    return (diff ** 2).mean(), np.concatenate([0.5 * 2 * diff / m, -0.5 * 2 * diff / m])


# d -> lanes per row (lanes_per_row(d / 4)): 4 -> 1, 8 -> 2, 16 -> 4, 32 -> 8, 64 -> 16, 128 -> 32, 256 -> 64 (one trip each),
# 260 -> 64 with a second trip of one lane, 1024 -> 64 with four trips
_DEC_CASES = [(m, d) for d in (4, 32, 64) for m in (1, 63, 64, 65, 1000)] + \
             [(m, d) for d in (8, 16, 128, 256, 260, 1024) for m in (1, 17, 1000)]


@pytest.mark.parametrize('m,d', _DEC_CASES)
def test_dec_value_and_gradient_against_fp64(m, d):
    g = torch.Generator().manual_seed(100 * m + d)
    z = torch.randn(N, d, generator=g)
    pos, neg = _edges(m, m + d)
    want_loss, want_w = _dec_fp64(z, pos, neg)
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


def _check_rows_add(d, n, n_s):
    from gnndelete_amd.edgeprob import rows_add_
    g = torch.Generator().manual_seed(d + n_s)
    sentinel = -777.25
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


@pytest.mark.parametrize('d', [4, 20, 64, 260])
def test_rows_add_is_exact_and_leaves_other_rows_alone(d):
    _check_rows_add(d, 500, 137)


@pytest.mark.parametrize('d,n_s', [(4, 1), (4, 255), (4, 256), (4, 257), (1024, 5)])
def test_rows_add_at_group_edges(d, n_s):
    """d = 4: one lane per row, 256 rows per block - one row, one row short of a block, a full block, one row into the
    second block.  d = 1024: 64 lanes per row, four trips of the strided loop."""
    _check_rows_add(d, 500, n_s)


# ------------------------------------------------------------------------------------------ endpoints outside [0, n)
# Only the ids -1 and n occur, and every buffer that a broken range test would index with them has spare rows (NaN or a
# sentinel) on both sides: a kernel without its guard gives a wrong answer here, it does not leave its allocation.
def _edges_with_bad_ends(m, d, n):
    """_edges with out-of-range ids in pos only, in neg only, at both ends of one edge, and in the last decoded edge of a
    block and the first of the next (a block holds 4 * 64 / lanes_per_row edges)."""
    lpr = 1
    while lpr < d // 4 and lpr < 64:
        lpr <<= 1
    per_block = 4 * (64 // lpr)
    assert per_block in (4, 16, 128) and m > per_block + 30
    pos, neg = _edges(m, 5 * d, n)
    pos[0, 20], pos[1, 22] = -1, n                       # pos only
    neg[1, 24], neg[0, 25] = n, -1                       # neg only
    pos[:, 27] = torch.tensor([-1, n])                   # both ends of one edge
    neg[:, 28] = torch.tensor([n, -1])
    pos[0, per_block - 1], neg[1, per_block] = n, -1     # either side of a block's edge
    return pos, neg


def _between_nan_rows(z):
    buf = torch.full((z.shape[0] + 2, z.shape[1]), float('nan'))
    buf[1:-1] = z
    return buf.cuda()[1:-1]


def _valid_incidence(e0, e1, n):
    """The stable sort of the valid edges' endpoints: entry p of cat(e0, e1) keeps its position p and its edge p mod M."""
    m = e0.shape[0]
    ok = (e0 >= 0) & (e0 < n) & (e1 >= 0) & (e1 < n)
    p = torch.arange(2 * m)[torch.cat([ok, ok])]
    ends_sorted, order = torch.sort(torch.cat([e0, e1])[p], stable=True)
    p = p[order]
    edge = p % m
    other = torch.where(p >= m, e0[edge], e1[edge]).to(torch.int32)
    return torch.searchsorted(ends_sorted, torch.arange(n + 1)), other, edge.to(torch.int32), int(ok.sum())


def _carved(n_elems, dtype, sentinel, spare):
    """-> (whole buffer, the view [spare : spare + n_elems]) on the device, every element = sentinel."""
    whole = torch.full((n_elems + 2 * spare,), sentinel, dtype=dtype, device='cuda')
    return whole, whole[spare:spare + n_elems]


@pytest.mark.parametrize('d', [8, 64, 260])
def test_out_of_range_endpoints_have_no_dot_product_and_no_incidence(d):
    from gnndelete_amd import _lib
    L = _L()
    n, m = N, 200
    g = torch.Generator().manual_seed(d)
    z = torch.randn(n, d, generator=g)
    pos, neg = _edges_with_bad_ends(m, d, n)
    zdev = _between_nan_rows(z)
    # the decoder alone
    want_loss, want_w = _dec_fp64(z, pos, neg)
    loss, w, _ = _dec(zdev, pos.cuda(), neg.cuda())
    assert bool(torch.isfinite(loss).all()) and bool(torch.isfinite(w).all())
    print(f'd={d} loss rel {abs(float(loss) - want_loss) / want_loss:.2e}  w rel_l2 {rel_l2(w.cpu(), want_w):.2e}')
    assert abs(float(loss) - want_loss) <= TOL * want_loss and rel_l2(w.cpu(), want_w) < TOL
    # the incidence list of [pos | neg]: workspace, inc_ptr and both outputs carved out of sentinel-filled allocations
    dec = torch.cat([pos, neg], 1)
    M = 2 * m
    nbytes = L.gd_edge_incidence_workspace(n, M)
    ws_all, ws = _carved(nbytes, torch.uint8, 0xA5, 32)
    ptr_all, inc_ptr = _carved(n + 1, torch.int64, 3, 2)
    oth_all, other = _carved(2 * M, torch.int32, -7, 4)
    src_all, src_edge = _carved(2 * M, torch.int32, -7, 4)
    e = dec.cuda()
    _lib.check(L.gd_edge_incidence(e[0].data_ptr(), e[1].data_ptr(), M, n, inc_ptr.data_ptr(), other.data_ptr(),
                                   src_edge.data_ptr(), ws.data_ptr(), nbytes, _st()), 'gd_edge_incidence')
    want_ptr, want_other, want_src, n_valid = _valid_incidence(dec[0], dec[1], n)
    assert n_valid == M - 8
    total = int(inc_ptr[n])
    assert total == 2 * n_valid
    assert torch.equal(inc_ptr.cpu(), want_ptr)
    assert torch.equal(other[:total].cpu(), want_other) and torch.equal(src_edge[:total].cpu(), want_src)
    assert bool((other[total:] == -7).all()) and bool((src_edge[total:] == -7).all())
    for whole, spare, sentinel in ((ws_all, 32, 0xA5), (ptr_all, 2, 3), (oth_all, 4, -7), (src_all, 4, -7)):
        assert bool((whole[:spare] == sentinel).all()) and bool((whole[-spare:] == sentinel).all())
    # the decoder with that list: w gathered for the incidences that exist, nothing written past them
    loss2, w2, w_inc = _dec(zdev, e[:, :m], e[:, m:], incidence=(inc_ptr, src_edge))
    assert torch.equal(loss2, loss) and torch.equal(w2, w)
    assert torch.equal(w_inc[:total], w[src_edge[:total].long()])
    assert bool(torch.isnan(w_inc[total:]).all()) and w_inc[total:].numel() == 16


@pytest.mark.parametrize('d', [8, 260])
def test_rows_add_skips_rows_outside_the_matrix(d):
    from gnndelete_amd.edgeprob import rows_add_
    g = torch.Generator().manual_seed(d)
    n, sentinel = 60, -777.25
    nodes = torch.tensor([-1, 0, 5, 6, 31, 59, n], dtype=torch.int32)
    buf = torch.full((n + 2, d), sentinel)
    buf[1:-1] = torch.randn(n, d, generator=g)
    src = torch.randn(nodes.numel(), d, generator=g)
    dev = buf.cuda()
    rows_add_(dev[1:-1], nodes.cuda(), src.cuda(), 0.5)
    want = buf.clone()
    want[1:-1].index_add_(0, nodes[1:-1].long(), 0.5 * src[1:-1])
    assert torch.equal(dev.cpu(), want)                   # valid rows exact; rows -1 and n skipped, the sentinel rows intact


# ------------------------------------------------------------------------------------------ past one grid, scan edges
def test_dec_finish_gathers_past_one_grid():
    """m = 70,000: 4m = 280,000 incidences, more than the finish kernel's 1,024 blocks x 256 threads cover in one trip."""
    from gnndelete_amd.edgeprob import edge_incidence
    m, n, d = 70000, 5000, 8
    assert 4 * m > 1024 * 256
    g = torch.Generator().manual_seed(70)
    z = torch.randn(n, d, generator=g)
    pos, neg = torch.randint(0, n, (2, m), generator=g), torch.randint(0, n, (2, m), generator=g)
    want_loss, want_w = _dec_fp64(z, pos, neg)
    dec = torch.cat([pos, neg], 1).cuda()
    inc = edge_incidence(dec[0], dec[1], n)
    for a, b, key in zip(inc, _reference_incidence(dec[0], dec[1], n), ('inc_ptr', 'other', 'src_edge')):
        assert a.dtype == b.dtype and torch.equal(a, b), key
    assert int(inc[0][n]) == 4 * m and int((inc[0][1:] - inc[0][:-1]).max()) < 120      # no long list
    zdev = z.cuda()
    loss, w, w_inc = _dec(zdev, dec[:, :m], dec[:, m:], incidence=(inc[0], inc[2]))
    loss2, w2, w_inc2 = _dec(zdev, dec[:, :m], dec[:, m:], incidence=(inc[0], inc[2]))
    assert torch.equal(loss, loss2) and torch.equal(w, w2) and torch.equal(w_inc, w_inc2)
    print(f'm={m} d={d} loss rel {abs(float(loss) - want_loss) / want_loss:.2e}  w rel_l2 {rel_l2(w.cpu(), want_w):.2e}')
    assert abs(float(loss) - want_loss) <= TOL * want_loss and rel_l2(w.cpu(), want_w) < TOL
    assert torch.equal(w_inc, w[inc[2].long()])           # all 4m entries (a NaN left in place compares unequal)


@pytest.mark.parametrize('n', [1023, 1024, 1025, 2048, 2049])
def test_incidence_scan_at_chunk_edges(n):
    """inc_scan_kernel gives each of its 1,024 threads ceil(n / 1024) consecutive nodes: 1 up to n = 1024, 2 up to 2048,
    then 3.  Nodes 0 and n - 1 have entries and six nodes without any lie across the edge between two chunks."""
    from gnndelete_amd.edgeprob import edge_incidence
    chunk = (n + 1023) // 1024
    lo = 500 * chunk - 3
    g = torch.Generator().manual_seed(n)
    allowed = torch.cat([torch.arange(lo), torch.arange(lo + 6, n)])
    e = allowed[torch.randint(0, allowed.numel(), (2, 3 * n), generator=g)]
    e[:, 0] = torch.tensor([0, n - 1])
    e = e.cuda()
    got, want = edge_incidence(e[0], e[1], n), _reference_incidence(e[0], e[1], n)
    for a, b, key in zip(got, want, ('inc_ptr', 'other', 'src_edge')):
        assert a.dtype == b.dtype and torch.equal(a, b), key
    deg = (got[0][1:] - got[0][:-1]).cpu()
    assert int(deg[0]) > 0 and int(deg[n - 1]) > 0 and int(deg[lo:lo + 6].sum()) == 0 and (lo + 3) % chunk == 0


def test_incidence_of_no_edges():
    from gnndelete_amd import _lib
    L = _L()
    n = 1025
    inc_ptr = torch.full((n + 1,), 9, dtype=torch.int64, device='cuda')
    ws = torch.empty(L.gd_edge_incidence_workspace(n, 0), dtype=torch.uint8, device='cuda')
    _lib.check(L.gd_edge_incidence(None, None, 0, n, inc_ptr.data_ptr(), None, None, ws.data_ptr(), ws.numel(), _st()),
               'gd_edge_incidence')
    assert bool((inc_ptr == 0).all())
    from gnndelete_amd.edgeprob import edge_incidence
    none = torch.zeros(0, dtype=torch.long, device='cuda')
    ptr2, other, src_edge = edge_incidence(none, none, n)
    assert torch.equal(ptr2, inc_ptr) and other.numel() == 0 and src_edge.numel() == 0


def test_incidence_workspace_and_outputs_are_reusable():
    """What EdgeprobEngine.step does every epoch: the entry on the same workspace and output buffers with another edge
    list.  1,777 edges, then 300, then the 1,777 again; each result is a fresh-buffer call's, bit for bit."""
    from gnndelete_amd import _lib
    from gnndelete_amd.edgeprob import edge_incidence
    L = _L()
    n = 5000
    a = _incidence_graphs()[-1][2].cuda()
    gb = torch.Generator().manual_seed(9)
    b = torch.randint(0, n, (2, 300), generator=gb).cuda()
    cap = a.shape[1]
    ws = torch.empty(L.gd_edge_incidence_workspace(n, cap), dtype=torch.uint8, device='cuda')
    inc_ptr = torch.empty(n + 1, dtype=torch.int64, device='cuda')
    other, src_edge = (torch.empty(2 * cap, dtype=torch.int32, device='cuda') for _ in range(2))
    for name, e in (('A', a), ('B', b), ('A again', a)):
        M = e.shape[1]
        e0, e1 = e[0].contiguous(), e[1].contiguous()
        _lib.check(L.gd_edge_incidence(e0.data_ptr(), e1.data_ptr(), M, n, inc_ptr.data_ptr(), other.data_ptr(),
                                       src_edge.data_ptr(), ws.data_ptr(), ws.numel(), _st()), 'gd_edge_incidence')
        fresh = edge_incidence(e0, e1, n)
        assert torch.equal(inc_ptr, fresh[0]), name
        assert torch.equal(other[:2 * M], fresh[1]) and torch.equal(src_edge[:2 * M], fresh[2]), name


# ------------------------------------------------------------------------------------------ the history ring
def _record(loss_r, loss_l, hist, capacity, pos):
    from gnndelete_amd import _lib
    _lib.check(_L().gd_edgeprob_record_f32(loss_r.data_ptr(), None if loss_l is None else loss_l.data_ptr(), 0.5, 0.5,
                                           hist.data_ptr(), capacity, pos.data_ptr(), _st()), 'gd_edgeprob_record_f32')


@pytest.mark.parametrize('capacity,with_l', [(3, True), (1, True), (3, False)])
def test_record_writes_one_row_of_the_ring_and_wraps(capacity, with_l):
    g = torch.Generator().manual_seed(capacity)
    sentinel = -3.5
    spare = 8                                             # sentinel rows on both sides of the ring
    whole = torch.full((capacity + 2 * spare, 3), sentinel, device='cuda')
    hist = whole[spare:spare + capacity]
    pos = torch.zeros(1, dtype=torch.int32, device='cuda')
    want = torch.full((capacity + 2 * spare, 3), sentinel)
    half = torch.tensor(0.5)
    for k in range(7):
        r, l = torch.rand(1, generator=g) * 3 + 0.1, torch.rand(1, generator=g) * 3 + 0.1
        _record(r.cuda(), l.cuda() if with_l else None, hist, capacity, pos)
        if not with_l:
            l = torch.zeros(1)
        want[spare + k % capacity] = torch.cat([half * r + half * l, l, r])          # fp32, as the kernel (no contraction)
        assert int(pos) == k + 1
        assert torch.equal(whole.cpu(), want), k          # the row at k mod capacity, every other row unchanged


# ------------------------------------------------------------------------------------------ refusals
def test_incidence_refuses_bad_arguments_without_a_launch():
    L = _L()
    n, M = 10, 6
    e = torch.randint(0, n, (2, M), device='cuda')
    e0, e1 = e[0].contiguous(), e[1].contiguous()
    inc_ptr = torch.full((n + 1,), 9, dtype=torch.int64, device='cuda')
    other, src_edge = (torch.full((2 * M,), -7, dtype=torch.int32, device='cuda') for _ in range(2))
    nbytes = L.gd_edge_incidence_workspace(n, M)
    ws = torch.full((nbytes,), 0xA5, dtype=torch.uint8, device='cuda')

    def call(e0p=e0.data_ptr(), n_edges=M, n_nodes=n, ip=inc_ptr.data_ptr(), size=nbytes):
        return L.gd_edge_incidence(e0p, e1.data_ptr(), n_edges, n_nodes, ip, other.data_ptr(), src_edge.data_ptr(), ws.data_ptr(),
                                   size, _st())
    assert call(size=nbytes - 1) == 4 and b'gd_edge_incidence' in L.gd_last_error_string()        # GD_E_WORKSPACE
    assert call(n_nodes=0) == 2 and b'gd_edge_incidence' in L.gd_last_error_string()               # GD_E_DIM
    assert call(n_edges=-1) == 2
    assert call(ip=None) == 1 and b'gd_edge_incidence' in L.gd_last_error_string()                 # GD_E_NULL
    assert call(e0p=None) == 1
    torch.cuda.synchronize()
    assert bool((inc_ptr == 9).all()) and bool((other == -7).all()) and bool((src_edge == -7).all())
    assert bool((ws == 0xA5).all())                                                                # not even the memset
    assert call() == 0


def test_rows_add_refuses_bad_arguments_without_a_launch():
    L = _L()
    dz = torch.full((8, 8), 3.0, device='cuda')
    src = torch.ones(4, 8, device='cuda')
    nodes = torch.arange(4, dtype=torch.int32, device='cuda')

    def call(dzp=dz.data_ptr(), ld=8, nodesp=nodes.data_ptr(), n_s=4, srcp=src.data_ptr(), d=8):
        return L.gd_rows_add_f32(dzp, ld, 8, nodesp, n_s, srcp, 8, 0.5, d, _st())
    assert call(d=6) == 2 and b'gd_rows_add_f32' in L.gd_last_error_string()                      # GD_E_DIM: d % 4
    assert call(ld=4) == 2 and call(ld=10) == 2                                                    # pitch < d, pitch % 4
    assert call(dzp=dz.data_ptr() + 4) == 3 and b'gd_rows_add_f32' in L.gd_last_error_string()    # GD_E_ALIGN
    assert call(dzp=None) == 1 and call(nodesp=None) == 1 and call(srcp=None) == 1                 # GD_E_NULL
    assert b'gd_rows_add_f32' in L.gd_last_error_string()
    assert call(n_s=0) == 0 and call(n_s=0, dzp=None, nodesp=None, srcp=None) == 0                 # nothing to add: OK
    torch.cuda.synchronize()
    assert bool((dz == 3.0).all())
    assert call() == 0
    assert torch.equal(dz[:4], torch.full((4, 8), 3.5, device='cuda')) and bool((dz[4:] == 3.0).all())


def test_record_refuses_bad_arguments_without_a_launch():
    L = _L()
    hist = torch.full((2, 3), -3.5, device='cuda')
    pos = torch.zeros(1, dtype=torch.int32, device='cuda')
    r = torch.ones(1, device='cuda')

    def call(rp=r.data_ptr(), hp=hist.data_ptr(), capacity=2, pp=pos.data_ptr()):
        return L.gd_edgeprob_record_f32(rp, None, 0.5, 0.5, hp, capacity, pp, _st())
    assert call(capacity=0) == 2 and b'gd_edgeprob_record_f32' in L.gd_last_error_string()        # GD_E_DIM
    assert call(capacity=-1) == 2
    assert call(hp=None) == 1 and b'gd_edgeprob_record_f32' in L.gd_last_error_string()           # GD_E_NULL
    assert call(pp=None) == 1 and call(rp=None) == 1
    torch.cuda.synchronize()
    assert bool((hist == -3.5).all()) and int(pos) == 0
    assert call() == 0
    assert hist[0].tolist() == [0.5, 0.0, 1.0] and int(pos) == 1
