"""gd_edge_incidence_fixed + gd_edge_incidence_update (csrc/incidence.hip) against gd_edge_incidence over the concatenated
list [fixed | variable], which tests/test_edgeprob_kernels_gpu.py pins to the stable sort: every comparison is an equality of
bits on inc_ptr and on other / src_edge up to inc_ptr[n]; the outputs start as sentinels, sit between sentinel words, and
what lies beyond inc_ptr[n] must still be the sentinel afterwards.

Graphs of test_edgeprob_kernels_gpu._incidence_graphs at every split (0, 1, the middle off a multiple of 64, M - 1, M); a list
of 300 variable entries on one node (more than one 256-thread block of entries; O(L^2) in the rank pass, still exact), on
either side and on both, and the same hub in the fixed half; one edge in both halves; endpoints -1 and n; the scan's edges
(4 nodes per thread, 1,024 per block, 1,024 tile sums per pass of the one-block kernel, i.e. n = 1024^2 + 1); reuse of one
image, workspace and outputs for other variable halves; the refusals."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _L():
    from gnndelete_amd import _lib
    return _lib.lib()


def _st():
    return torch.cuda.current_stream().cuda_stream


def _carved(n_elems, dtype, sentinel, spare=8):
    whole = torch.full((n_elems + 2 * spare,), sentinel, dtype=dtype, device='cuda')
    return whole, whole[spare:spare + n_elems]


def _oracle(e, n):
    """gd_edge_incidence over all of e (int64 [2, M] on the device) into sentinel-filled arrays -> (inc_ptr, other, src_edge)."""
    from gnndelete_amd import _lib
    L, M = _L(), e.shape[1]
    inc_ptr = torch.full((n + 1,), 9, dtype=torch.int64, device='cuda')
    other, src_edge = (torch.full((max(2 * M, 1),), -7, dtype=torch.int32, device='cuda') for _ in range(2))
    ws = torch.empty(L.gd_edge_incidence_workspace(n, M), dtype=torch.uint8, device='cuda')
    e0, e1 = e[0].contiguous(), e[1].contiguous()
    _lib.check(L.gd_edge_incidence(e0.data_ptr(), e1.data_ptr(), M, n, inc_ptr.data_ptr(), other.data_ptr(), src_edge.data_ptr(),
                                   ws.data_ptr(), ws.numel(), _st()), 'gd_edge_incidence')
    return inc_ptr, other, src_edge


def _image(e, n_fixed, n):
    from gnndelete_amd.edgeprob import edge_incidence_image
    return edge_incidence_image(e[0], e[1], n_fixed, n)


def _update(image, e, n_fixed, n):
    """The update into sentinel-filled, sentinel-fenced arrays -> (inc_ptr, other, src_edge); the fences are checked here."""
    from gnndelete_amd import _lib
    L, M = _L(), e.shape[1]
    nbytes = L.gd_edge_incidence_update_workspace(n, M)
    ws_all, ws = _carved(nbytes // 8 + 1, torch.int64, 0x5A5A5A5A5A5A5A5A)
    ptr_all, inc_ptr = _carved(n + 1, torch.int64, 9)
    oth_all, other = _carved(max(2 * M, 2), torch.int32, -7)
    src_all, src_edge = _carved(max(2 * M, 2), torch.int32, -7)
    e0, e1 = e[0].contiguous(), e[1].contiguous()
    _lib.check(L.gd_edge_incidence_update(image.data_ptr(), e0.data_ptr(), e1.data_ptr(), n_fixed, M, n, inc_ptr.data_ptr(),
                                          other.data_ptr(), src_edge.data_ptr(), ws.data_ptr(), 8 * ws.numel(), _st()),
               'gd_edge_incidence_update')
    for whole, sentinel in ((ws_all, 0x5A5A5A5A5A5A5A5A), (ptr_all, 9), (oth_all, -7), (src_all, -7)):
        assert bool((whole[:8] == sentinel).all()) and bool((whole[-8:] == sentinel).all())
    return inc_ptr, other, src_edge


def _assert_same(got, want, n, what):
    total = int(want[0][n])
    assert torch.equal(got[0], want[0]), f'{what}: inc_ptr'
    assert torch.equal(got[1][:total], want[1][:total]), f'{what}: other'
    assert torch.equal(got[2][:total], want[2][:total]), f'{what}: src_edge'
    assert bool((got[1][total:] == -7).all()) and bool((got[2][total:] == -7).all()), f'{what}: written beyond inc_ptr[n]'
    return total


def _check(e, n, n_fixed, what=''):
    e = e.cuda()
    want = _oracle(e, n)
    got = _update(_image(e, n_fixed, n), e, n_fixed, n)
    return _assert_same(got, want, n, f'{what} n_fixed={n_fixed}')


def _splits(M):
    mid = M // 2
    if mid % 64 == 0:
        mid += 1
    return sorted({0, min(1, M), min(mid, M), max(M - 1, 0), M})


def _incidence_graphs():
    """The graphs of tests/test_edgeprob_kernels_gpu.py::_incidence_graphs."""
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
def test_update_equals_the_full_rebuild_at_every_split(name, n, e):
    M = e.shape[1]
    splits = _splits(M)
    assert splits[0] == 0 and splits[-1] == M and all(s % 64 or s in (0, M) for s in splits)
    for n_fixed in splits:
        total = _check(e, n, n_fixed, name)
        assert total == 2 * M
    if name == 'n5000':
        ptr = _oracle(e.cuda(), n)[0]
        deg = ptr[1:] - ptr[:-1]
        assert int(deg.max()) > 64 and int((deg == 0).sum()) >= 1000


@pytest.mark.parametrize('side', ['source', 'destination', 'both'])
@pytest.mark.parametrize('hub_is', ['variable', 'fixed'])
def test_a_list_longer_than_one_block(side, hub_is):
    """300 edges on node 7 on one side (or both: 300 self pairs) in one half, 100 random edges in the other."""
    n, hub = 50, 7
    g = torch.Generator().manual_seed(300)
    rest = torch.randint(0, n, (2, 100), generator=g)
    heavy = torch.randint(0, n, (2, 300), generator=g)
    if side in ('source', 'both'):
        heavy[0] = hub
    if side in ('destination', 'both'):
        heavy[1] = hub
    e, n_fixed = (torch.cat([rest, heavy], 1), 100) if hub_is == 'variable' else (torch.cat([heavy, rest], 1), 300)
    assert _check(e, n, n_fixed, f'{side} hub in the {hub_is} half') == 800
    ptr = _oracle(e.cuda(), n)[0]
    assert int(ptr[hub + 1] - ptr[hub]) >= 300 > 256


def test_the_same_edge_in_both_halves():
    g = torch.Generator().manual_seed(11)
    a = torch.randint(0, 40, (2, 77), generator=g)
    a[:, 5] = a[:, 4]                                     # and twice inside each half
    assert _check(torch.cat([a, a], 1), 40, 77, 'duplicates') == 4 * 77


def test_out_of_range_endpoints_have_no_entries_in_either_half():
    """-1 and n, as e0 and as e1, in the fixed and in the variable half: 8 edges without entries."""
    n, F, V = 300, 203, 197
    g = torch.Generator().manual_seed(8)
    e = torch.randint(0, n, (2, F + V), generator=g)
    for base in (10, F + 10):
        e[0, base], e[0, base + 1], e[1, base + 2], e[1, base + 3] = -1, n, -1, n
    assert _check(e, n, F, 'bad endpoints') == 2 * (F + V - 8)
    assert _check(e, n, 0, 'bad endpoints') == 2 * (F + V - 8)
    assert _check(e, n, F + V, 'bad endpoints') == 2 * (F + V - 8)


@pytest.mark.parametrize('n,edge,m', [(1023, 512, 3000), (1024, 512, 3000), (1025, 1024, 3000), (2048, 1024, 6000), (2049, 1024, 6000),
                                      (2049, 2048, 6000), (1024 * 1024 + 1, 1024 * 512, 20000), (1024 * 1024 + 1, 1024 * 1024, 20000)])
def test_scan_edges(n, edge, m):
    """The scan gives a thread 4 consecutive nodes and a block 1,024; the one-block pass over the tile sums gives each of its
    1,024 threads ceil(tiles / 1024) consecutive tiles (2 from n = 1024^2 + 1 on, where thread 255's end is node 1024 * 512).
    Nodes 0 and n - 1 have entries in both halves; the nodes [edge - 3, edge + 3) below n - 1 have none."""
    g = torch.Generator().manual_seed(n + edge)
    lo, hi = edge - 3, min(edge + 3, n - 1)
    allowed = torch.cat([torch.arange(lo), torch.arange(hi, n)])
    e = allowed[torch.randint(0, allowed.numel(), (2, m), generator=g)]
    F = m // 2 + 1
    e[:, 0] = torch.tensor([0, n - 1])
    e[:, F] = torch.tensor([n - 1, 0])
    assert _check(e, n, F, f'n={n}') == 2 * m
    ptr = _oracle(e.cuda(), n)[0]
    deg = (ptr[1:] - ptr[:-1]).cpu()
    assert int(deg[0]) >= 2 and int(deg[n - 1]) >= 2 and int(deg[lo:hi].sum()) == 0 and hi > lo


def test_one_image_many_updates_on_the_same_buffers():
    """What step_device does every epoch: one image, then the update on the same workspace and outputs with another variable
    half - 1,777 - F edges, then 300, then the first again; each result is a fresh-buffer full rebuild's, the image's bytes do
    not change, and two calls on the same input give the same bits."""
    from gnndelete_amd import _lib
    from gnndelete_amd.edgeprob import edge_incidence
    L = _L()
    n, F = 5000, 1001
    a = _incidence_graphs()[-1][2].cuda()
    gb = torch.Generator().manual_seed(9)
    b = torch.cat([a[:, :F], torch.randint(0, n, (2, 300), generator=gb).cuda()], 1)
    image = _image(a, F, n)
    before = image.clone()
    cap = a.shape[1]
    ws = torch.empty(L.gd_edge_incidence_update_workspace(n, cap) // 8 + 1, dtype=torch.int64, device='cuda')
    inc_ptr = torch.empty(n + 1, dtype=torch.int64, device='cuda')
    other, src_edge = (torch.empty(2 * cap, dtype=torch.int32, device='cuda') for _ in range(2))
    kept = {}
    for name, e in (('A', a), ('B', b), ('A again', a), ('A a third time', a)):
        M = e.shape[1]
        e0, e1 = e[0].contiguous(), e[1].contiguous()
        _lib.check(L.gd_edge_incidence_update(image.data_ptr(), e0.data_ptr(), e1.data_ptr(), F, M, n, inc_ptr.data_ptr(),
                                              other.data_ptr(), src_edge.data_ptr(), ws.data_ptr(), 8 * ws.numel(), _st()),
                   'gd_edge_incidence_update')
        fresh = edge_incidence(e0, e1, n)
        assert torch.equal(inc_ptr, fresh[0]), name
        assert torch.equal(other[:2 * M], fresh[1]) and torch.equal(src_edge[:2 * M], fresh[2]), name
        if name.startswith('A a'):
            for x, y in zip(kept['A'], (inc_ptr, other, src_edge)):
                assert torch.equal(x, y), name
        kept[name] = (inc_ptr.clone(), other.clone(), src_edge.clone())
    assert torch.equal(image, before)


def test_refusals_launch_nothing():
    L = _L()
    n, M, F = 10, 6, 4
    e = torch.randint(0, n, (2, M), device='cuda')
    e0, e1 = e[0].contiguous(), e[1].contiguous()
    inc_ptr = torch.full((n + 1,), 9, dtype=torch.int64, device='cuda')
    other, src_edge = (torch.full((2 * M,), -7, dtype=torch.int32, device='cuda') for _ in range(2))
    img_bytes, ws_bytes = L.gd_edge_incidence_fixed_bytes(n, F), L.gd_edge_incidence_update_workspace(n, M)
    assert img_bytes > 0 and ws_bytes >= L.gd_edge_incidence_update_workspace(n, F) > 0
    image = torch.full((img_bytes // 8 + 1,), 0x5A, dtype=torch.int64, device='cuda')
    ws = torch.full((ws_bytes // 8 + 1,), 0x5A, dtype=torch.int64, device='cuda')

    def fixed(e0p=e0.data_ptr(), n_fixed=F, n_nodes=n, img=image.data_ptr(), isize=img_bytes, wsp=ws.data_ptr(),
              wsize=L.gd_edge_incidence_update_workspace(n, F)):
        return L.gd_edge_incidence_fixed(e0p, e1.data_ptr(), n_fixed, n_nodes, img, isize, wsp, wsize, _st())

    def update(img=image.data_ptr(), e0p=e0.data_ptr(), n_fixed=F, n_edges=M, n_nodes=n, ip=inc_ptr.data_ptr(), wsp=ws.data_ptr(),
               wsize=ws_bytes):
        return L.gd_edge_incidence_update(img, e0p, e1.data_ptr(), n_fixed, n_edges, n_nodes, ip, other.data_ptr(), src_edge.data_ptr(),
                                          wsp, wsize, _st())
    assert fixed(isize=img_bytes - 1) == 4 and b'gd_edge_incidence_fixed' in L.gd_last_error_string()       # GD_E_WORKSPACE
    assert fixed(wsize=L.gd_edge_incidence_update_workspace(n, F) - 1) == 4
    assert fixed(n_nodes=0) == 2 and b'gd_edge_incidence_fixed' in L.gd_last_error_string()                  # GD_E_DIM
    assert fixed(n_fixed=-1) == 2
    assert fixed(img=None) == 1 and b'gd_edge_incidence_fixed' in L.gd_last_error_string()                   # GD_E_NULL
    assert fixed(wsp=None) == 1 and fixed(e0p=None) == 1
    assert update(wsize=ws_bytes - 1) == 4 and b'gd_edge_incidence_update' in L.gd_last_error_string()
    assert update(n_nodes=0) == 2 and b'gd_edge_incidence_update' in L.gd_last_error_string()
    assert update(n_fixed=M + 1) == 2 and update(n_fixed=-1) == 2 and update(n_edges=-1) == 2
    assert update(img=None) == 1 and b'gd_edge_incidence_update' in L.gd_last_error_string()
    assert update(ip=None) == 1 and update(wsp=None) == 1 and update(e0p=None) == 1
    torch.cuda.synchronize()
    assert bool((inc_ptr == 9).all()) and bool((other == -7).all()) and bool((src_edge == -7).all())
    assert bool((ws == 0x5A).all()) and bool((image == 0x5A).all())                                          # not even the zeroing
    assert fixed() == 0 and update() == 0


def test_no_variable_and_no_fixed_edges_at_all():
    """n_edges == n_fixed == 0: inc_ptr is all zeros, nothing else is touched, null edge pointers are fine."""
    from gnndelete_amd import _lib
    L = _L()
    n = 1025
    image = torch.empty(L.gd_edge_incidence_fixed_bytes(n, 0) // 8 + 1, dtype=torch.int64, device='cuda')
    ws = torch.empty(L.gd_edge_incidence_update_workspace(n, 0) // 8 + 1, dtype=torch.int64, device='cuda')
    inc_ptr = torch.full((n + 1,), 9, dtype=torch.int64, device='cuda')
    _lib.check(L.gd_edge_incidence_fixed(None, None, 0, n, image.data_ptr(), 8 * image.numel(), ws.data_ptr(), 8 * ws.numel(), _st()),
               'gd_edge_incidence_fixed')
    _lib.check(L.gd_edge_incidence_update(image.data_ptr(), None, None, 0, 0, n, inc_ptr.data_ptr(), None, None, ws.data_ptr(),
                                          8 * ws.numel(), _st()), 'gd_edge_incidence_update')
    assert bool((inc_ptr == 0).all())
